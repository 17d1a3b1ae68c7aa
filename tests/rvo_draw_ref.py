"""The RVO draw (include/cagpu.h, CaRvoDraw) restated in NumPy on oracle/philox_ref.py -- test infrastructure, written from
the header's text: the two Philox blocks of an address (g, k, a, s), the three uniforms, the window test of the
anti-collaborative branch, the bit's evolution over an episode and the Box-Muller normal of the heading noise."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle.philox_ref import philox4x32_10  # noqa: E402

MASK = 0xFFFFFFFF
NONCOOP = 1 << 18
TWO_PI = 6.283185307179586


def _u64(x):
    return np.asarray(x, dtype=np.int64).astype(np.uint64)


def blocks(seed, g, k, a, s):
    """B0 and B1 of every address -> two tuples of four uint64 arrays (32-bit words)"""
    g, k, a, s = np.broadcast_arrays(_u64(g), _u64(k), _u64(a), _u64(s))
    key = (np.uint64(seed & MASK), np.uint64((seed >> 32) & MASK))
    w3 = ((s << np.uint64(10)) | a) & np.uint64(MASK)
    c01 = (g & np.uint64(MASK), (g >> np.uint64(32)) & np.uint64(MASK))
    b0 = philox4x32_10(c01 + (k & np.uint64(MASK), w3), key)
    b1 = philox4x32_10(c01 + ((k | np.uint64(0x80000000)) & np.uint64(MASK), w3), key)
    return b0, b1


def _uniform(w, w2):
    return ((w >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w2 >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def uniforms(seed, g, k, a, s):
    """u0, u1 (block B0) and v0 (block B1) of every address: float64 arrays in [0, 1)"""
    b0, b1 = blocks(seed, g, k, a, s)
    return _uniform(b0[0], b0[1]), _uniform(b0[2], b0[3]), _uniform(b1[0], b1[1])


def noncoop_draw(seed, c, g, k, a, s):
    """what a redraw at the address gives: u0 < 1 - |c|"""
    return uniforms(seed, g, k, a, s)[0] < 1.0 - abs(float(c))


def window(t, T, dt):
    """the clock t lies within dt of a multiple of T (float64, rint = to nearest even)"""
    t = np.asarray(t, np.float64)
    m = np.fmod(t, float(T))
    return (np.rint(m * 1000.0) / 1000.0 < dt) | (np.rint((float(T) - m) * 1000.0) / 1000.0 < dt)


def z_normal(seed, g, k, a, s):
    """z = sqrt(-2 log(1 - u1)) cos(2 pi v0): evaluated in np.longdouble on the double operands 1 - u1 and 2 pi v0 the rule
    names, rounded to double once"""
    _, u1, v0 = uniforms(seed, g, k, a, s)
    one_minus = (1.0 - u1).astype(np.longdouble)          # exact in float64
    arg = (TWO_PI * v0).astype(np.longdouble)             # rounds once, in float64, as the rule says
    return (np.sqrt(np.longdouble(-2.0) * np.log(one_minus)) * np.cos(arg)).astype(np.float64)


def noise(seed, std, g, k, a, s):
    return float(std) * z_normal(seed, g, k, a, s)


def next_bit(bit, queried, t, T, dt, seed, c, g, k, a, s):
    """the CA_RVO_NONCOOP bit after a step's query: redrawn for queried agents inside the window, carried otherwise"""
    redraw = np.asarray(queried, bool) & window(t, T, dt)
    return np.where(redraw, noncoop_draw(seed, c, g, k, a, s), np.asarray(bit, bool))


def episode_bits(seed, c, T, dt, g, k, a, steps, step_dt):
    """the bit of ONE agent over an episode it is queried in at every step: clock accumulated in float64 from 0"""
    out, bit, t = [], False, 0.0
    for s in range(int(steps)):
        bit = bool(next_bit(bit, True, t, T, dt, seed, c, g, k, a, s))
        out.append(bit)
        t = t + step_dt
    return np.array(out)
