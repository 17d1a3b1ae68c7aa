"""The sampled GA3C-CADRL policy (include/cagpu.h, CaGa3cSample) restated in NumPy on oracle/philox_ref.py -- test
infrastructure, written from the header's text: the uniform of an address (g, k, a, s), the softmax's running sums, the
choice, the log-probability and the entropy.  Twice: in float64 (sample64: the yardstick of logp / entropy, and the judge of
which rows lie near a tie) and in NumPy float32 as a plain restatement of the rule's own arithmetic (sample32).

NEAR_TIE: a row is near a tie if |u * S64 - c64_j| < NEAR_TIE * S64 for some j < 10.  The device compares float32
quantities: 11 terms q_j, each off by at most 2 ulp from expf plus half an ulp from its own rounding, summed with half an
ulp per addition -- every c_j and S within 11 * 3 ulp / 2^24 < 2e-6 relative of the exact value in the worst case of all
errors aligned --, and (float)u and the product u * S add 2^-24 each: below 4e-6 relative in all.  The bound is twice
that.  A row that is not near a tie has the same index in exact arithmetic and in any float32 evaluation of the rule."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.philox_ref import philox4x32_10  # noqa: E402

MASK = 0xFFFFFFFF
NL = 11
NEAR_TIE = 8e-6

# the sampler fixture: seeds chosen on the CPU so that no row is near a tie (tests/test_ga3c_sample_host.py asserts it)
FIXTURE_SEED = 0x5A3C0FFEE1234567
FIXTURE_RNG = 2
TEMPERATURES = (0.5, 1.0, 4.0)
N_AGENTS = 6


def _u64(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64)


def uniform(seed, g, k, a, s):
    """u of every address: words 0, 1 of block B0 = philox4x32_10((g lo, g hi, k, (s << 10) | a), (seed lo, seed hi)), 53 bits"""
    g, k, a, s = np.broadcast_arrays(_u64(g), _u64(k), _u64(a), _u64(s))
    key = (np.uint64(seed & MASK), np.uint64((seed >> 32) & MASK))
    w3 = ((s << np.uint64(10)) | a) & np.uint64(MASK)
    b0 = philox4x32_10((g & np.uint64(MASK), (g >> np.uint64(32)) & np.uint64(MASK), k & np.uint64(MASK), w3), key)
    return ((b0[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b0[1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def inv_temperature(temperature):
    """1 / temperature as the library divides it: in float32"""
    return np.float32(1.0) / np.float32(temperature)


def sample64(u, logits, temperature):
    """the rule in float64 on the float32 logits and the float32 inv_T -> (index, logp, entropy, near_tie) per row; a row
    with a NaN logit: index 0, logp = entropy = NaN, not near a tie"""
    l = np.asarray(logits, np.float32).astype(np.float64).reshape(-1, NL)
    u = np.asarray(u, np.float64).reshape(-1)
    bad = np.isnan(l).any(axis=1)
    l = np.where(bad[:, None], 0.0, l)
    z = (l - l.max(axis=1, keepdims=True)) * float(inv_temperature(temperature))
    q = np.exp(z)
    c = np.cumsum(q, axis=1)
    S = c[:, -1]
    x = u * S
    idx = np.minimum((x[:, None] >= c).sum(axis=1), NL - 1)
    near = (np.abs(x[:, None] - c[:, :NL - 1]) < NEAR_TIE * S[:, None]).any(axis=1) & ~bad
    logp = z[np.arange(len(z)), idx] - np.log(S)
    ent = np.log(S) - (q * z).sum(axis=1) / S
    idx = np.where(bad, 0, idx)
    return idx.astype(np.int64), np.where(bad, np.nan, logp), np.where(bad, np.nan, ent), near


def sample32(u, logits, temperature):
    """the rule in NumPy float32, operation by operation as the header states it -> (index, logp, entropy)"""
    f = np.float32
    l = np.asarray(logits, f).reshape(-1, NL)
    u = np.asarray(u, np.float64).reshape(-1)
    inv_T = inv_temperature(temperature)
    n = l.shape[0]
    idx, logp, ent = np.zeros(n, np.int64), np.zeros(n, f), np.zeros(n, f)
    for r in range(n):
        row = l[r]
        if np.isnan(row).any():
            idx[r], logp[r], ent[r] = 0, np.nan, np.nan
            continue
        m = row.max()
        z = ((row - m) * inv_T).astype(f)
        q = np.exp(z).astype(f)
        c, run, w = np.zeros(NL, f), f(0), f(0)
        for j in range(NL):
            run = f(run + q[j])
            c[j] = run
            w = f(w + f(q[j] * z[j]))
        S = c[NL - 1]
        x = f(f(u[r]) * S)
        j = NL - 1
        for t in range(NL - 1):
            if x < c[t]:
                j = t
                break
        idx[r] = j
        logp[r] = f(z[j] - np.log(S).astype(f))
        ent[r] = f(np.log(S).astype(f) - f(w / S))
    return idx, logp, ent


def greedy64(logits, temperature):
    """logp of the first maximum and the entropy, float64: what an agent that does not sample gets"""
    l = np.asarray(logits, np.float32).astype(np.float64).reshape(-1, NL)
    z = (l - l.max(axis=1, keepdims=True)) * float(inv_temperature(temperature))
    q = np.exp(z)
    S = q.sum(axis=1)
    idx = l.argmax(axis=1)
    return idx, z[np.arange(len(z)), idx] - np.log(S), np.log(S) - (q * z).sum(axis=1) / S


def fixture():
    """the sampler fixture: 2048 rows -> dict(g, k, a, s, logits [2048, 11] float32, temperature [2048]).  Rows 0 .. 1023 are
    crafted (equal logits, one logit 80 above the rest, one 200 below in the middle of the row, descending and ascending
    ramps, random rows), rows 1024 .. 2047 the shipped checkpoint's logits on the golden observations
    (tests/golden/ga3c_graph.npz); the address fields sweep g >= 2^32, k, a = 0 and a = N_AGENTS - 1, s = 0 and s large; the
    temperatures cycle through TEMPERATURES"""
    rng = np.random.default_rng(FIXTURE_RNG)
    n = 2048
    real = np.load(os.path.join(REPO, "tests", "golden", "ga3c_graph.npz"))["logits_IROS18"].astype(np.float32)
    lg = np.zeros((n, NL), np.float32)
    for r in range(1024):
        kind = r % 8
        base = rng.normal(0.0, 2.0, NL).astype(np.float32)
        if kind == 0:
            row = np.full(NL, np.float32(rng.normal(0.0, 3.0)), np.float32)           # equal logits
        elif kind == 1:
            row = base.copy()
            row[rng.integers(0, NL)] = base.max() + np.float32(80.0)                  # probability exactly 1
        elif kind == 2:
            row = base.copy()
            row[rng.integers(1, NL - 1)] = base.min() - np.float32(200.0)             # q = 0 in the middle of the row
        elif kind == 3:
            row = (np.float32(rng.uniform(0.1, 1.5)) * np.arange(NL, 0, -1)).astype(np.float32)   # descending ramp
        elif kind == 4:
            row = (np.float32(rng.uniform(0.1, 1.5)) * np.arange(NL)).astype(np.float32)          # ascending ramp
        else:
            row = base
        lg[r] = row
    lg[1024:] = real[:1024]
    g = rng.integers(0, 1 << 20, n).astype(np.int64)
    g[::3] += 1 << 32
    g[1::7] = (1 << 33) + rng.integers(0, 1 << 31, len(g[1::7]))
    k = rng.integers(0, 3000, n).astype(np.int64)
    k[::5] = 0
    a = rng.integers(0, N_AGENTS, n).astype(np.int64)
    a[::4] = 0
    a[1::4] = N_AGENTS - 1
    s = rng.integers(0, 400, n).astype(np.int64)
    s[::6] = 0
    s[1::6] = (1 << 22) - 1 - rng.integers(0, 1000, len(s[1::6]))
    temp = np.array(TEMPERATURES, np.float64)[np.arange(n) % 3]
    return dict(g=g, k=k, a=a, s=s, logits=lg, temperature=temp)
