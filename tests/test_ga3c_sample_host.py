"""The sampled GA3C-CADRL policy, the experience tape's C ABI and GAE without a GPU: the two restatements
(tests/ga3c_sample_ref.py, tests/gae_ref.py) held to their purpose, the committed sampler fixture free of near ties, the
CaGa3cSample layout and exports of include/cagpu.h, and every argument rejection of cagpu_ga3c_sample,
cagpu_ga3c_sample_at and cagpu_gae -- fake non-null pointers, nothing launched (the pattern of tests/test_rvo_draw_host.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import ga3c_sample_ref as ref  # noqa: E402
from tests import gae_ref  # noqa: E402
from tests import rvo_draw_ref  # noqa: E402

B = ctypes.byref
SEED = ref.FIXTURE_SEED

# (n, E, N) of the GAE fixtures: E * N in {1, 63, 65, 130}, n in {1, 2, 17}
GAE_SHAPES = [(1, 1, 1), (2, 9, 7), (17, 5, 13), (17, 13, 10), (1, 13, 5), (2, 1, 1)]
GAE_PARAMS = [(0.0, 0.0), (1.0, 1.0), (0.99, 0.95)]


def _nat():
    from gym_collision_avoidance_amd import _native as nat
    return nat, nat.lib()


# ---------------------------------------------------------------- the restatements
def test_uniform_is_the_rvo_draws_u0():
    rng = np.random.default_rng(1)
    n = 5000
    g, k, a, s = rng.integers(0, 1 << 34, n), rng.integers(0, 1 << 31, n), rng.integers(0, 1024, n), rng.integers(0, 1 << 22, n)
    g[:3], k[:3], a[:3], s[:3] = (0, (1 << 32) - 1, 1 << 32), (0, 0x7FFFFFFF, 1), (0, 1023, 0), (0, (1 << 22) - 1, 1)
    for seed in (SEED, 1, 0xFFFFFFFFFFFFFFFF):
        u = ref.uniform(seed, g, k, a, s)
        assert np.array_equal(u, rvo_draw_ref.uniforms(seed, g, k, a, s)[0])
        assert (u >= 0).all() and (u < 1).all()
    assert (ref.uniform(SEED, g, k, a, s) != ref.uniform(SEED + 1, g, k, a, s)).all()


def test_fixture_has_no_near_tie_and_both_restatements_agree():
    fx = ref.fixture()
    assert fx["logits"].shape == (2048, 11) and fx["logits"].dtype == np.float32
    assert (fx["g"] >= 1 << 32).sum() > 500 and (fx["a"] == 0).any() and (fx["a"] == ref.N_AGENTS - 1).any()
    assert (fx["s"] == 0).any() and (fx["s"] > (1 << 22) - 2000).any() and (fx["s"] < 1 << 22).all() and (fx["k"] == 0).any()
    u = ref.uniform(SEED, fx["g"], fx["k"], fx["a"], fx["s"])
    seen = np.zeros(11, np.int64)
    for T in ref.TEMPERATURES:
        m = fx["temperature"] == T
        i64, lp64, en64, near = ref.sample64(u[m], fx["logits"][m], T)
        assert not near.any(), "temperature %g: rows %s of the fixture are near a tie" % (T, np.flatnonzero(m)[near])
        i32, lp32, en32 = ref.sample32(u[m], fx["logits"][m], T)
        assert np.array_equal(i64, i32)
        assert (np.abs(lp32 - lp64) <= 2e-6 * (1 + np.abs(lp64))).all()
        assert (np.abs(en32 - en64) <= 4e-6 * (1 + np.abs(en64))).all()
        assert (en64 >= -1e-12).all() and (en64 <= np.log(11) + 1e-12).all() and (lp64 <= 0).all()
        seen += np.bincount(i64, minlength=11)
    assert (seen > 20).all(), seen          # every index is drawn
    # equal logits: the index is floor(11 u); one logit 80 above the rest at temperature <= 1: that one
    l = np.zeros((1000, 11), np.float32) + np.float32(0.7)
    uu = np.random.default_rng(2).random(1000)
    assert np.array_equal(ref.sample64(uu, l, 1.0)[0], np.floor(11 * uu).astype(np.int64))
    l[:, 4] += 80
    i, lp, en, _ = ref.sample64(uu, l, 1.0)
    assert (i == 4).all() and np.abs(lp).max() < 1e-30 and np.abs(en).max() < 1e-30


def test_sampled_frequencies_follow_the_softmax():
    n = 200000
    rng = np.random.default_rng(3)
    g, k, a, s = rng.integers(0, 1 << 33, n), rng.integers(0, 50, n), rng.integers(0, 6, n), rng.integers(0, 1 << 22, n)
    row = np.array([0.3, -1.0, 2.0, 0.0, 1.5, -3.0, 0.2, 0.9, -0.4, 1.1, 0.0], np.float32)
    for T in (0.5, 4.0):
        p = np.exp(row.astype(np.float64) / T)
        p /= p.sum()
        i = ref.sample64(ref.uniform(SEED, g, k, a, s), np.broadcast_to(row, (n, 11)), T)[0]
        f = np.bincount(i, minlength=11) / n
        assert (np.abs(f - p) <= 4.5 * np.sqrt(p * (1 - p) / n)).all(), (T, f, p)


def test_bad_rows():
    l = np.zeros((3, 11), np.float32)
    l[1, 5] = np.nan
    for fn in (ref.sample64, ref.sample32):
        out = fn(np.array([0.9, 0.9, 0.9]), l, 1.0)
        assert out[0].tolist() == [9, 0, 9] and np.isnan(out[1]).tolist() == [False, True, False]


@pytest.mark.parametrize("n,E,N", GAE_SHAPES)
def test_gae_float32_loop_against_float64(n, E, N):
    d = gae_ref.synthetic(n, E, N, seed=100 + n + E * N)
    for gamma, lam in GAE_PARAMS:
        a32, r32 = gae_ref.gae32(gamma=gamma, lam=lam, **d)
        a64, r64 = gae_ref.gae64(gamma=gamma, lam=lam, **d)
        assert a32.dtype == np.float32 and r32.dtype == np.float32
        for x, y in ((a32, a64), (r32, r64)):
            assert np.abs(x - y).max() <= 1e-5 * max(1.0, float(np.abs(y).max())), (gamma, lam)
        assert (a32[~d["live"]] == 0).all() and (r32[~d["live"]] == 0).all()
        end = d["live"] & (d["done"] | d["game_over"][:, :, None])
        want = (d["reward"] - d["value"]).astype(np.float32)
        assert np.array_equal(a32[end], want[end])       # terminal: delta = reward - value, nothing behind it
        if gamma == 0.0:
            assert np.array_equal(a32[d["live"]], want[d["live"]])


def test_gae_fixtures_take_every_branch():
    counts = {}
    for n, E, N in GAE_SHAPES:
        d = gae_ref.synthetic(n, E, N, seed=100 + n + E * N)
        counts[(n, E * N)] = gae_ref.branches(d["live"], d["done"], d["game_over"])
    big = counts[(17, 130)]
    assert big["not_live"] > 100 and big["done"] > 100 and big["game_over_only"] > 50 and big["plain"] > 500, big
    assert counts[(17, 65)]["game_over_only"] > 0 and counts[(2, 63)]["not_live"] > 0
    n1 = counts[(1, 1)]
    assert n1 == dict(not_live=0, done=0, game_over_only=1, plain=0), n1      # n = 1: one slot, ended by game_over only
    n1b = counts[(1, 65)]
    assert n1b["done"] > 0 and n1b["plain"] > 0 and n1b["not_live"] > 0, n1b
    # the placements synthetic() promises: endings at t = 0 and t = n - 1, consecutive endings, a gap before last_value
    d = gae_ref.synthetic(17, 13, 10, seed=0)
    fl = lambda x: x.reshape(17, 130)
    assert fl(d["done"])[0, 0] and fl(d["done"])[16, 0] and fl(d["done"])[0:2, 1].all() and not fl(d["live"])[16, 1]
    assert not fl(d["live"])[2:4, 2].any() and fl(d["live"])[4, 2]
    # a gap at the end: last_value is not read
    a, _ = gae_ref.gae32(gamma=0.99, lam=0.95, **d)
    d2 = dict(d, last_value=np.where(np.arange(130).reshape(13, 10) == 1, np.float32(1e6), d["last_value"]))
    assert np.array_equal(a, gae_ref.gae32(gamma=0.99, lam=0.95, **d2)[0])


# ---------------------------------------------------------------- the ABI
def test_struct_layout_and_exports():
    nat, lib = _nat()
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    body = re.search(r"typedef struct CaGa3cSample \{(.*?)\} CaGa3cSample;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [m[1] for m in re.findall(r"(\w+)\s*\*?(\w+);", body)]
    assert names == [f[0] for f in nat.CaGa3cSample._fields_]
    assert ctypes.sizeof(nat.CaGa3cSample) == 128
    assert [getattr(nat.CaGa3cSample, f).offset for f in names] == [0, 8, 12] + list(range(16, 32, 8)) + [32, 36] + \
        list(range(40, 128, 8))
    for n in ("cagpu_ga3c_sample", "cagpu_ga3c_sample_at", "cagpu_gae"):
        assert n in nat.EXPORTS and re.search(r"\bint %s\(" % n, hdr) and hasattr(lib, n), n
    assert len(lib.cagpu_ga3c_sample.argtypes) == 9 and len(lib.cagpu_ga3c_sample_at.argtypes) == 13
    assert len(lib.cagpu_gae.argtypes) == 14
    assert nat.FAULT_GA3C_SAMPLE_NAN == 32 and "bit 5 = a logits row with a NaN" in hdr


def _fake(nat, E=4, N=4):
    from gym_collision_avoidance_amd import core
    p = core.make_params(E, N)
    fake = 0x1000
    s = nat.CaState(**{n: fake for n in nat.STATE_FIELDS if n not in ("next_action", "turning_dir", "rvo_collab",
                                                                       "rvo_heading_noise", "ext_state")})
    return p, s


def _good(nat, **kw):
    d = dict(seed=SEED, temperature=1.0, greedy=0, mask=0x3000, logits=0x2000, logp=0x2000)
    d.update(kw)
    return nat.CaGa3cSample(**d)


def test_ga3c_sample_rejections():
    nat, lib = _nat()
    p, s = _fake(nat)
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    ar = nat.CaAutoReset(table=0x4000, n_cases=4, env_id_offset=0, case_stride=4, heading_seed=77)
    pd = nat.CaPolicyDraw(cdf=0x5000, policy_bits=0x5000, num_policies=2, ensure=-1, seed=99)
    m = nat.CaMap(static_bits=0x2000, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=55)
    rd = nat.CaRvoDraw(seed=33, collab_coeff=-0.5, anti_collab_t=1.0, noise_std=0.5)

    def call(g, p_=p, s_=s, ext=0x6000, others=True):
        o = (B(ar), B(pd), B(ms), B(rd)) if others else (None, None, None, None)
        rc = lib.cagpu_ga3c_sample(None if p_ is None else B(p_), None if s_ is None else B(s_), *o,
                                   None if g is None else B(g), ext, None)
        return rc, lib.cagpu_last_error()

    cases = [
        (dict(g=None), b"NULL pointer"), (dict(g=_good(nat), p_=None), b"NULL pointer"), (dict(g=_good(nat), s_=None), b"NULL pointer"),
        (dict(g=_good(nat), ext=None), b"NULL pointer"), (dict(g=_good(nat, logits=None)), b"NULL pointer"),
        (dict(g=_good(nat, logp=None)), b"NULL pointer"),
        (dict(g=_good(nat, seed=0)), b"seed must not be 0"), (dict(g=_good(nat, seed=0), others=False), b"seed must not be 0"),
        (dict(g=_good(nat, seed=77)), b"seed equals"), (dict(g=_good(nat, seed=99)), b"seed equals"),
        (dict(g=_good(nat, seed=55)), b"seed equals"), (dict(g=_good(nat, seed=33)), b"seed equals"),
        (dict(g=_good(nat, temperature=0.0)), b"temperature"), (dict(g=_good(nat, temperature=-1.0)), b"temperature"),
        (dict(g=_good(nat, temperature=float("nan"))), b"temperature"), (dict(g=_good(nat, temperature=float("inf"))), b"temperature"),
        (dict(g=_good(nat, greedy=1, temperature=0.0)), b"temperature"),
        (dict(g=_good(nat, address=0x6004)), b"8-byte aligned"),
        (dict(g=_good(nat, slot_obs=0x7000)), b"slot_obs needs obs"), (dict(g=_good(nat, slot_value=0x7000)), b"slot_value needs value"),
    ]
    for kw, text in cases:
        rc, msg = call(**kw)
        assert rc == nat.CA_EINVAL and text in msg and b"cagpu_ga3c_sample" in msg, (text, rc, msg)
    for f in ("flags", "step_num", "reset_count"):
        keep = getattr(s, f)
        setattr(s, f, None)
        rc, msg = call(_good(nat))
        assert rc == nat.CA_EINVAL and b"NULL pointer" in msg, f
        setattr(s, f, keep)
    from gym_collision_avoidance_amd import core
    rc, msg = call(_good(nat), p_=core.make_params(2, 1025))
    assert rc == nat.CA_EINVAL and b"bad sizes" in msg
    assert lib.cagpu_last_kernel() == before      # nothing was launched


def test_ga3c_sample_at_rejections():
    nat, lib = _nat()
    f = 0x1000

    def call(seed=SEED, T=1.0, N=4, g=f, k=f, a=f, s=f, lg=f, n=8, o0=f, o1=f, o2=f):
        rc = lib.cagpu_ga3c_sample_at(seed, T, N, g, k, a, s, lg, n, o0, o1, o2, None)
        return rc, lib.cagpu_last_error()

    for kw in (dict(g=None), dict(k=None), dict(a=None), dict(s=None), dict(lg=None), dict(o0=None, o1=None, o2=None),
               dict(N=0), dict(N=1025), dict(n=-1)):
        rc, msg = call(**kw)
        assert rc == nat.CA_EINVAL and b"cagpu_ga3c_sample_at" in msg, (kw, rc, msg)
    rc, msg = call(seed=0)
    assert rc == nat.CA_EINVAL and b"seed must not be 0" in msg
    for T in (0.0, -2.0, float("nan"), float("inf")):
        rc, msg = call(T=T)
        assert rc == nat.CA_EINVAL and b"temperature" in msg, T
    assert call(n=0)[0] == nat.CA_OK            # n == 0 does nothing


def test_gae_rejections():
    nat, lib = _nat()
    f = 0x1000
    names = ("reward", "value", "last_value", "live", "done", "game_over", "adv", "ret")

    def call(n=4, EN=16, N=4, gamma=0.99, lam=0.95, **ptr):
        q = {k: f for k in names}
        q.update(ptr)
        rc = lib.cagpu_gae(n, EN, N, q["reward"], q["value"], q["last_value"], q["live"], q["done"], q["game_over"], gamma, lam,
                           q["adv"], q["ret"], None)
        return rc, lib.cagpu_last_error()

    for k in names:
        rc, msg = call(**{k: None})
        assert rc == nat.CA_EINVAL and b"cagpu_gae: NULL pointer" in msg, k
    for kw in (dict(n=0), dict(n=-3), dict(EN=0), dict(N=0), dict(EN=17)):
        rc, msg = call(**kw)
        assert rc == nat.CA_EINVAL and b"cagpu_gae: n < 1" in msg, kw
    for kw in (dict(gamma=-0.1), dict(gamma=1.5), dict(lam=-0.1), dict(lam=2.0), dict(gamma=float("nan"))):
        rc, msg = call(**kw)
        assert rc == nat.CA_EINVAL and b"gamma and lambda" in msg, kw
