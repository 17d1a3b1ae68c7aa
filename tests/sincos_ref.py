"""Operands, high-precision reference and bars for the step kernels' short-range sin / cos of a heading (sincos_heading,
csrc/cagpu.hip): shared by tests/test_gpu_move_edges.py (the device's answers) and tests/test_move_scenes_host.py (the
reference itself against mpmath).  numpy only.

The bars are the ones the kernel's own comment claims: at most 1 ulp (of the true value, as a float64) from the true value, or,
for an operand within 1e-11 of a multiple of pi / 2 -- where the result is ~1e-12 and the two-part reduction constant limits
the absolute error instead -- an absolute error below 1e-26.  Besides: s^2 + c^2 within 4 ulps of 1, sin(-x) = -sin(x) and
cos(-x) = cos(x) by bits."""
import math

import numpy as np

SEED = 20240611
DRAWS = 65536
NEAR = 1e-11
ABS_BAR = 1e-26
ULP_BAR = 1.0


def _around(x, n):
    """x and the n doubles either side of it"""
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def edge_operands():
    """every double within 4 ulps of k pi / 4 for k = -4 .. 4 (+-pi and the switch points of the reduction's rint among them),
    +-0, the smallest normal, the largest subnormal, 2^-k for k = 1 .. 60, the doubles either side of each of these, and the
    negative of everything"""
    tiny = np.finfo(np.float64).tiny
    x = []
    for k in range(-4, 5):
        x += _around(np.float64(k) * (np.pi / 4), 4)
    for v in [np.float64(0.0), tiny, np.nextafter(tiny, 0.0)] + [np.float64(2.0) ** -k for k in range(1, 61)]:
        x += _around(v, 1)
    x = np.array(x, np.float64)
    return np.concatenate([x, -x])


def operands():
    """the edge operands and DRAWS uniform draws from [-pi, pi) with a fixed seed, with their negatives: float64 [n], the second
    half the negative of the first, element by element"""
    e = edge_operands()
    e = e[:e.size // 2]
    u = np.random.default_rng(SEED).uniform(-np.pi, np.pi, DRAWS)
    x = np.concatenate([e, u])
    return np.concatenate([x, -x])


def reference(x):
    """sin and cos in np.longdouble, which must be the 64-bit-mantissa format or better (asserted: fails, never skips)"""
    assert np.finfo(np.longdouble).machep <= -63, "np.longdouble is no wider than float64 here: no reference for sin / cos"
    xl = np.asarray(x, np.float64).astype(np.longdouble)
    return np.sin(xl), np.cos(xl)


def ulp_of(v):
    """the spacing of float64 at |v| (v: longdouble)"""
    a = np.abs(np.asarray(v, np.longdouble)).astype(np.float64)
    return (np.nextafter(a, np.inf) - a).astype(np.longdouble)


def measure(x, s, c):
    """-> dict of the measured maxima of the device's (s, c) for operands x (layout of operands())"""
    x, s, c = (np.asarray(a, np.float64) for a in (x, s, c))
    rs, rc = reference(x)
    q = x / (np.pi / 2)
    near = np.abs(x - np.rint(q) * (np.pi / 2)) <= NEAR
    out = dict(n=int(x.size), near=int(near.sum()))
    for name, got, ref in (("sin", s, rs), ("cos", c, rc)):
        err = np.abs(got.astype(np.longdouble) - ref)
        ulps = (err / ulp_of(ref)).astype(np.float64)
        small = near & (np.abs(ref) < 1e-10)      # the member of the pair that is ~0 there
        out[name + "_max_ulp"] = float(ulps[~small].max())
        out[name + "_max_abs_near"] = float(err[small].max()) if small.any() else 0.0
        out[name + "_max_ulp_near"] = float(ulps[small].max()) if small.any() else 0.0
        out[name + "_bad"] = int(((ulps > ULP_BAR) & ~(small & (err < ABS_BAR))).sum())
    one = s.astype(np.longdouble) ** 2 + c.astype(np.longdouble) ** 2 - 1
    out["norm_max_ulp"] = float(np.abs(one).max() / np.finfo(np.float64).eps)
    h = x.size // 2
    out["sin_odd_bad"] = int((s[:h].view(np.int64) != (-s[h:]).view(np.int64)).sum())
    out["cos_even_bad"] = int((c[:h].view(np.int64) != c[h:].view(np.int64)).sum())
    out["sin_odd_first"] = [float(v) for v in x[:h][s[:h].view(np.int64) != (-s[h:]).view(np.int64)][:4]]
    return out


def check(m):
    """the bars, on measure()'s dict"""
    assert m["sin_bad"] == 0 and m["cos_bad"] == 0, "beyond 1 ulp of the true value (and 1e-26 near a multiple of pi / 2): %r" % (m,)
    assert m["norm_max_ulp"] <= 4.0, "s^2 + c^2 is %g ulps from 1" % m["norm_max_ulp"]
    assert m["sin_odd_bad"] == 0, "sin(-x) != -sin(x) by bits for %d operands, first %r" % (m["sin_odd_bad"], m["sin_odd_first"])
    assert m["cos_even_bad"] == 0, "cos(-x) != cos(x) by bits for %d operands" % m["cos_even_bad"]


def report(m):
    return ("sincos_heading on %d operands (%d within 1e-11 of a multiple of pi/2): max error sin %.3f ulp, cos %.3f ulp; near a "
            "multiple of pi/2 the vanishing member is off by at most %.3g absolute (%.3g ulp); |s^2 + c^2 - 1| <= %.2f ulp; "
            "sin(-x) = -sin(x) fails for %d, cos(-x) = cos(x) for %d operands" % (
                m["n"], m["near"], m["sin_max_ulp"], m["cos_max_ulp"], max(m["sin_max_abs_near"], m["cos_max_abs_near"]),
                max(m["sin_max_ulp_near"], m["cos_max_ulp_near"]), m["norm_max_ulp"], m["sin_odd_bad"], m["cos_even_bad"]))


def mpmath_cross_check(x):
    """np.longdouble's sin / cos against mpmath at 40 digits -> the largest error of the longdouble reference in units of the
    float64 ulp of the true value (it must be far below the 1 ulp it is used to measure)"""
    import mpmath
    mpmath.mp.dps = 40
    rs, rc = reference(x)
    worst = 0.0
    for xi, si, ci in zip(np.asarray(x, np.float64), rs, rc):
        for got, true in ((si, mpmath.sin(mpmath.mpf(float(xi)))), (ci, mpmath.cos(mpmath.mpf(float(xi))))):
            hi = np.float64(got)
            lo = np.float64(got - np.longdouble(hi))
            err = abs((mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))) - true)
            t = abs(float(true))
            ulp = float(np.nextafter(t, math.inf) - t)
            worst = max(worst, float(err / mpmath.mpf(ulp)))
    return worst
