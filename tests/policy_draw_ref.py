"""TEST INFRASTRUCTURE.  The policy draw of an auto-reset (include/cagpu.h CaPolicyDraw) restated in NumPy on
oracle/philox_ref.py: what the step kernels and cagpu_policy_draw must write into the flag words, slot by slot."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.philox_ref import MASK, philox4x32_10  # noqa: E402

ENSURE_SLOT = 0xFFFFFFFE   # the counter word of the ensure rule's uniform (no agent index reaches it)
DRAW_BITS = 0xFC0          # bits 6..11 of a flag word: IS_LEARNING, STILL_LEARNING, the policy id


def uniform_at(seed, g, k, c3):
    """the step kernels' uniform for a 128-bit counter: Philox4x32-10, key = seed, counter = (g lo, g hi, k, c3)"""
    w = philox4x32_10((g & MASK, (g >> 32) & MASK, k & MASK, c3 & MASK), (seed & MASK, (seed >> 32) & MASK))
    return ((w[0] >> 5) * 67108864.0 + (w[1] >> 6)) / 9007199254740992.0


def cdf_of(distr):
    """np.random.choice's own normalisation: p.cumsum() divided by its last element"""
    cdf = np.asarray(distr, np.float64).cumsum()
    return cdf / cdf[-1]


def index_of(cdf, u):
    """#{j : cdf[j] <= u}, clamped to P - 1 (searchsorted(side='right'))"""
    return min(int(np.searchsorted(cdf, u, side="right")), len(cdf) - 1)


def draw_env(seed, g, k, present, cdf, ensure=-1):
    """pool index of every slot of global env g in its episode k -> int array [N], -1 for absent slots"""
    present = np.asarray(present, bool)
    out = np.full(present.size, -1, np.int64)
    slots = np.flatnonzero(present)
    for a in slots:
        out[a] = index_of(cdf, uniform_at(seed, g, k, int(a)))
    if ensure is not None and ensure >= 0 and slots.size and not (out[slots] == ensure).any():
        n = slots.size
        r = min(int(np.floor(n * uniform_at(seed, g, k, ENSURE_SLOT))), n - 1)
        out[slots[r]] = ensure
    return out


def draw_batch(seed, env_ids, episodes, present, cdf, ensure=-1):
    """draw_env for a batch: env_ids [E] (global), episodes [E], present [E, N] -> [E, N]"""
    return np.stack([draw_env(seed, int(g), int(k), p, cdf, ensure) for g, k, p in zip(env_ids, episodes, present)])


def apply_bits(flags, index, pool_bits):
    """the flag words after the draw: present slots take the pool entry's bits 6..11, absent ones keep theirs"""
    flags = np.asarray(flags).astype(np.int64) & 0xFFFFFFFF
    bits = np.asarray(pool_bits, np.int64)[np.maximum(index, 0)] & DRAW_BITS
    return np.where(index >= 0, (flags & ~DRAW_BITS) | bits, flags)
