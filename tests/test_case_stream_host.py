"""The case stream without a GPU: the C ABI of cagpu_generate_cases_at / cagpu_stream_refill (include/cagpu.h
CaCaseStream), its ctypes mirror, every argument check that returns before anything is launched, and the host restatement
the GPU tests lean on (tests/case_stream_ref.py): the window rule and the attempt counts."""
import ctypes
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import case_stream_ref as ref  # noqa: E402

B = ctypes.byref
FIELDS = [("double", "table"), ("int32_t", "held"), ("int32_t", "seen"), ("int64_t", "work_index"), ("int64_t", "work_row"),
          ("int32_t", "work_count"), ("int32_t", "counts"), ("int32_t", "status"), ("int32_t", "window"),
          ("int32_t", "n_min, n_max, n_ranges"), ("const double", "side_ranges"),
          ("double", "speed_lo, speed_hi, radius_lo, radius_hi"), ("uint64_t", "seed")]


def _header():
    return open(os.path.join(REPO, "include", "cagpu.h")).read()


def test_header_declares_the_stream_and_keeps_version_12():
    hdr = _header()
    assert "#define CAGPU_VERSION 12" in hdr
    body = re.search(r"typedef struct CaCaseStream \{(.*?)\} CaCaseStream;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const double|double|int32_t|int64_t|uint64_t)\s*\*?\s*([\w, ]+);", body)
    assert fields == FIELDS, fields
    args = lambda name: [" ".join(a.split()) for a in re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1).split(",")]
    ragged = args("cagpu_generate_cases_ragged")
    assert ragged[0] == "int64_t num_cases"
    # the arguments of cagpu_generate_cases_ragged, num_cases replaced by the list
    assert args("cagpu_generate_cases_at") == ["const int64_t *case_index", "const int64_t *out_row", "const int32_t *count",
                                               "int64_t M"] + ragged[1:]
    assert args("cagpu_stream_refill") == ["const CaParams *p", "const CaState *s", "const CaAutoReset *ar",
                                           "const CaCaseStream *cs", "void *stream"]
    # the overrun bit is documented beside bits 0 - 2
    doc = re.search(r"/\* Device-side fault word.*?\*/", hdr, re.S).group(0)
    for bit in ("bit 0", "bit 1", "bit 2", "bit 3"):
        assert bit in doc, bit


def test_library_exports_and_binding_mirror_the_header():
    from gym_collision_avoidance_amd import _native as nat
    lib = nat.lib()
    assert lib.cagpu_version() == 12 == nat.ABI_VERSION
    for n in ("cagpu_generate_cases_at", "cagpu_stream_refill"):
        assert n in nat.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    P = ctypes.sizeof(ctypes.c_void_p)
    S = nat.CaCaseStream
    names = [f[0] for f in S._fields_]
    assert names == [n.strip() for _, group in FIELDS for n in group.split(",")]
    assert ctypes.sizeof(S) == 9 * P + 16 + 32 + 8 == 128
    assert [getattr(S, n).offset for n in names] == [0, P, 2 * P, 3 * P, 4 * P, 5 * P, 6 * P, 7 * P, 8 * P, 8 * P + 4,
                                                     8 * P + 8, 8 * P + 12, 8 * P + 16, 9 * P + 16, 9 * P + 24, 9 * P + 32,
                                                     9 * P + 40, 9 * P + 48]
    assert len(lib.cagpu_generate_cases_at.argtypes) == len(lib.cagpu_generate_cases_ragged.argtypes) + 3 == 18
    assert len(lib.cagpu_stream_refill.argtypes) == 5
    # no existing struct grew
    assert ctypes.sizeof(nat.CaStepEx) == 56 and ctypes.sizeof(nat.CaPolicyDraw) == 32
    assert ctypes.sizeof(nat.CaAutoReset) == 56
    assert nat.FAULT_STREAM_OVERRUN == 1 << 3


RG = np.ascontiguousarray([[0, 5, 4.0, 5.0], [5, 100, 6.0, 8.0]], dtype=np.float64)
PLAIN = np.ascontiguousarray([4.0, 4.0], dtype=np.float64)
FAKE = 0x1000


def _at(lib, **kw):
    a = dict(case_index=FAKE, out_row=None, count=None, M=8, max_agents=10, n_min=2, n_max=10, side_ranges=RG.ctypes.data,
             n_ranges=2, speed_lo=0.5, speed_hi=2.0, radius_lo=0.2, radius_hi=0.8, seed=3, cases=FAKE, counts=None, status=None)
    a.update(kw)
    rc = lib.cagpu_generate_cases_at(a["case_index"], a["out_row"], a["count"], a["M"], a["max_agents"], a["n_min"], a["n_max"],
                                     a["side_ranges"], a["n_ranges"], a["speed_lo"], a["speed_hi"], a["radius_lo"],
                                     a["radius_hi"], a["seed"], a["cases"], a["counts"], a["status"], None)
    return rc, lib.cagpu_last_error()


def test_generate_cases_at_rejects_bad_arguments_before_any_device_use():
    """device pointers that are never dereferenced: every call fails an argument check, nothing is launched"""
    from gym_collision_avoidance_amd import _native as nat
    lib = nat.lib()
    gap = np.ascontiguousarray([[0, 5, 4.0, 5.0], [6, 100, 6.0, 8.0]], dtype=np.float64)      # no range holds 5 agents
    bad_side = np.ascontiguousarray([[0, 100, 4.0, 3.0]], dtype=np.float64)
    zero_side, down_side = np.ascontiguousarray([0.0, 4.0]), np.ascontiguousarray([4.0, 3.0])
    for bad, word in ((dict(M=0), b"entries"), (dict(M=-3), b"entries"), (dict(M=1 << 31), b"entries"),
                      (dict(case_index=None), b"NULL case_index"), (dict(cases=None), b"NULL cases"),
                      (dict(max_agents=0), b"max_agents"), (dict(max_agents=1025), b"max_agents"),
                      (dict(side_ranges=None), b"side_ranges"), (dict(n_ranges=-1), b"n_ranges"),
                      (dict(n_ranges=9), b"at most 8"), (dict(n_max=-1), b"n_min <= n_max"),
                      (dict(n_min=0), b"n_min <= n_max"), (dict(n_min=7, n_max=3), b"n_min <= n_max"),
                      (dict(n_max=11), b"n_min <= n_max"), (dict(side_ranges=gap.ctypes.data), b"no side range"),
                      (dict(side_ranges=bad_side.ctypes.data, n_ranges=1), b"positive and ordered"),
                      (dict(speed_lo=0.0), b"bounds"), (dict(speed_hi=0.4), b"bounds"), (dict(radius_lo=-1.0), b"bounds"),
                      (dict(radius_hi=0.1), b"bounds"),
                      # the plain form: n_ranges = 0, side_ranges = HOST [2]
                      (dict(n_ranges=0, n_max=0, side_ranges=zero_side.ctypes.data), b"bounds"),
                      (dict(n_ranges=0, n_max=0, side_ranges=down_side.ctypes.data), b"bounds")):
        rc, msg = _at(lib, **bad)
        assert rc == nat.CA_EINVAL and b"cagpu_generate_cases_at" in msg and word in msg, (bad, rc, msg)
    # the two older entry points keep their messages
    rc = lib.cagpu_generate_cases(0, 10, 4.0, 4.0, 0.5, 2.0, 0.2, 0.8, 3, FAKE, None, None)
    assert rc == nat.CA_EINVAL and lib.cagpu_last_error() == b"cagpu_generate_cases: bad sizes"
    rc = lib.cagpu_generate_cases_ragged(4, 10, 2, 11, RG.ctypes.data, 2, 0.5, 2.0, 0.2, 0.8, 3, FAKE, None, None, None)
    assert rc == nat.CA_EINVAL and lib.cagpu_last_error() == b"cagpu_generate_cases_ragged: need 1 <= n_min <= n_max <= max_agents"
    rc = lib.cagpu_generate_cases(4, 10, 4.0, 4.0, 0.5, 2.0, 0.2, 0.8, 3, None, None, None)
    assert rc == nat.CA_EINVAL and lib.cagpu_last_error() == b"cagpu_generate_cases: NULL cases"


def test_stream_refill_rejects_bad_arguments_before_any_device_use():
    from gym_collision_avoidance_amd import _native as nat
    from gym_collision_avoidance_amd import core
    lib = nat.lib()
    E, N, W = 6, 4, 3
    p = core.make_params(E, N, ragged=1)
    s = nat.CaState(reset_count=FAKE)
    good_cs = dict(table=0x2000, held=0x3000, seen=0x4000, work_index=0x5000, work_row=0x6000, work_count=0x7000, window=W,
                   n_min=2, n_max=4, n_ranges=2, side_ranges=RG.ctypes.data, speed_lo=0.5, speed_hi=2.0, radius_lo=0.2,
                   radius_hi=0.8, seed=9)
    good_ar = dict(table=0x2000, n_cases=E * W, env_id_offset=0, case_stride=E, heading_seed=5)

    def call(cs=None, ar=None, p_=p, s_=s, null=None):
        c = nat.CaCaseStream(**dict(good_cs, **(cs or {})))
        a = nat.CaAutoReset(**dict(good_ar, **(ar or {})))
        args = dict(p=B(p_), s=B(s_), ar=B(a), cs=B(c))
        if null:
            args[null] = None
        rc = lib.cagpu_stream_refill(args["p"], args["s"], args["ar"], args["cs"], None)
        return rc, lib.cagpu_last_error()

    for null in ("p", "s", "ar", "cs"):
        rc, msg = call(null=null)
        assert rc == nat.CA_EINVAL and b"cagpu_stream_refill" in msg and b"NULL argument" in msg, (null, msg)
    rc, msg = call(s_=nat.CaState())
    assert rc == nat.CA_EINVAL and b"reset_count" in msg
    rc, msg = call(p_=core.make_params(0, N))
    assert rc == nat.CA_EINVAL and b"bad sizes" in msg
    rc, msg = call(p_=core.make_params(E, 1025, ragged=1), cs=dict(n_max=0, n_min=0))
    assert rc == nat.CA_EINVAL and b"max_agents" in msg
    big = core.make_params(1 << 30, N, ragged=1)
    rc, msg = call(p_=big, ar=dict(case_stride=1 << 30))
    assert rc == nat.CA_EINVAL and b"does not fit" in msg
    for bad, word in ((dict(window=0), b"window"), (dict(window=-2), b"window"), (dict(table=None), b"NULL pointer"),
                      (dict(held=None), b"NULL pointer"), (dict(seen=None), b"NULL pointer"),
                      (dict(work_index=None), b"NULL pointer"), (dict(work_row=None), b"NULL pointer"),
                      (dict(work_count=None), b"NULL pointer"), (dict(side_ranges=None), b"side_ranges"),
                      (dict(n_ranges=-1), b"n_ranges"), (dict(n_max=5), b"n_min <= n_max"), (dict(n_min=0), b"n_min <= n_max"),
                      (dict(speed_lo=0.0), b"bounds"), (dict(radius_hi=0.1), b"bounds")):
        rc, msg = call(cs=bad)
        assert rc == nat.CA_EINVAL and b"cagpu_stream_refill" in msg and word in msg, (bad, rc, msg)
    for bad, word in ((dict(table=0x9000), b"must name the window"), (dict(n_cases=E * W + 1), b"must name the window"),
                      (dict(case_stride=E + 1), b"must name the window"), (dict(reset_obs=0x8000), b"reset_obs"),
                      (dict(reset_plan=0x8000), b"reset_obs"), (dict(env_id_offset=-1), b"2^32"),
                      (dict(env_id_offset=(1 << 32) - E + 1), b"2^32")):
        rc, msg = call(ar=bad)
        assert rc == nat.CA_EINVAL and b"cagpu_stream_refill" in msg and word in msg, (bad, rc, msg)


def test_window_rule_and_case_index():
    """with case_stride = E and n_cases = E * W the auto-reset formula is slot k % W of the env's own window: W
    consecutive episodes of an env never share a row, and no two envs ever do -- for any shard offset"""
    for E, W, off in ((5, 3, 0), (37, 2, 30), (4, 1, 7), (6, 8, (1 << 32) - 6)):
        owner = {}
        for e in range(E):
            for k in range(3 * W + 2):
                r = ref.window_row(off, e, k, E, W)
                assert 0 <= r < E * W
                assert r == ref.window_row(off, e, k % W, E, W)
                assert owner.setdefault(r, e) == e
            assert len({ref.window_row(off, e, k, E, W) for k in range(5, 5 + W)}) == W
        assert len(owner) == E * W
    assert ref.case_index(3, 5) == (3 << 32) | 5 and ref.case_index((1 << 32) - 1, (1 << 31) - 1) < 1 << 64


def test_host_restatement_counts_attempts():
    """host_cases_at: the cases of tests/test_host_logic.py's host_cases_from_philox at the same indices, a case is a
    function of its 64-bit index alone, and the attempt counts add up to the draws the stream handed out"""
    from tests.test_host_logic import host_cases_from_philox
    cases, counts, kinds, attempts = ref.host_cases_at(1, range(24), 10, ref.REF_SIDE, num_agents=(2, 10))
    want, w_kinds = host_cases_from_philox(1, 24, 10, ref.REF_SIDE, num_agents=(2, 10))
    assert np.array_equal(cases, want) and kinds == w_kinds
    assert all(len(a) == c for a, c in zip(attempts, counts))
    assert all(min(a) >= (0 if k == "swap" else 1) for a, k in zip(attempts, kinds))
    assert all(a[0] == a[1] == 0 for a, k in zip(attempts, kinds) if k == "swap")
    far = [ref.case_index(2 ** 31, 7), ref.case_index(5, 2 ** 31 - 1), 11]
    a = ref.host_cases_at(9, far, 4, 4.0)[0]
    b = ref.host_cases_at(9, far[::-1], 4, 4.0)[0]
    assert np.array_equal(a, b[::-1]) and not np.array_equal(a[0], a[1])
    assert np.array_equal(a[2], host_cases_from_philox(9, 12, 4, 4.0)[0][11])
    fam, rand_max, circ_max = ref.coverage(kinds, attempts)
    assert fam == {"swap", "circle", "rand"} and rand_max >= 2 and circ_max >= 1


def test_binding_maps_the_distribution_like_generate_cases():
    """core.BatchedSim._case_dist: the plain form (n_ranges = 0, HOST [2]) where generate_cases() calls cagpu_generate_cases,
    the ragged arguments where it calls cagpu_generate_cases_ragged"""
    from gym_collision_avoidance_amd import core
    d = core.BatchedSim._case_dist
    n_lo, n_hi, rg, n = d(10, 4.0, None)
    assert (n_lo, n_hi, n) == (0, 0, 0) and rg.tolist() == [4.0, 4.0]
    assert d(10, (4.0, 8.0), None)[2].tolist() == [4.0, 8.0]
    n_lo, n_hi, rg, n = d(10, ref.REF_SIDE, (2, 10))
    assert (n_lo, n_hi, n) == (2, 10, 2) and rg.tolist() == [[0, 5, 4, 5], [5, 100, 6, 8]]
    n_lo, n_hi, rg, n = d(10, 4.0, (2, 6))
    assert (n_lo, n_hi, n) == (2, 6, 1) and rg.tolist() == [[0, 1 << 30, 4.0, 4.0]]
    assert d(7, ref.REF_SIDE, None)[:2] == (7, 7)
