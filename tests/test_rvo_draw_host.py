"""The RVO draw (CaRvoDraw, cagpu_step_noise, cagpu_rvo_draw_at of include/cagpu.h) without a GPU: the rule's restatement
(tests/rvo_draw_ref.py) against Python's own arithmetic and against the distributions it claims, the struct's layout, and
every argument rejection -- fake non-null pointers, nothing launched (the pattern of tests/test_step_ex_host.py)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import rvo_draw_ref as ref  # noqa: E402

B, A = ctypes.byref, ctypes.addressof
SEED = 0x5EED0123456789AB


def _nat():
    from gym_collision_avoidance_amd import _native as nat
    return nat, nat.lib()


# ---------------------------------------------------------------- the rule
@pytest.mark.parametrize("T", [0.3, 1.0, 2.5])
def test_window_equals_pythons_round(T):
    DT = 0.1
    t = 0.0
    for step in range(400):
        want = round(t % T, 3) < DT or round(T - t % T, 3) < DT
        assert bool(ref.window(t, T, DT)) == want, (T, step, t)
        t = t + DT
    assert bool(ref.window(0.0, T, DT))   # every episode's first query redraws


def _addresses(n, rng):
    return (rng.integers(0, 1 << 33, n), rng.integers(0, 50, n), rng.integers(0, 1024, n), rng.integers(0, 1 << 22, n))


@pytest.mark.parametrize("c", [-0.6, -0.1, -0.95])
def test_noncoop_frequency(c):
    n = 100000
    g, k, a, s = _addresses(n, np.random.default_rng(1))
    p = 1.0 - abs(c)
    freq = ref.noncoop_draw(SEED, c, g, k, a, s).mean()
    assert abs(freq - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (freq, p)


def test_z_is_standard_normal():
    from scipy import stats
    g, k, a, s = _addresses(100000, np.random.default_rng(2))
    z = ref.z_normal(SEED, g, k, a, s)
    assert np.isfinite(z).all() and np.abs(z).max() <= 8.6
    pv = stats.kstest(z, "norm").pvalue
    assert pv > 1e-3, pv


def test_distinct_addresses_distinct_blocks():
    # neighbours in every coordinate, both blocks of each: all different
    base = [(g, k, a, s) for g in (0, 1, 1 << 32) for k in (0, 1, 7) for a in (0, 1, 1023) for s in (0, 1, (1 << 22) - 1)]
    g, k, a, s = (np.array(x) for x in zip(*base))
    b0, b1 = ref.blocks(SEED, g, k, a, s)
    rows = {tuple(int(w[i]) for w in b) for b in (b0, b1) for i in range(len(base))}
    assert len(rows) == 2 * len(base)
    # (s, a) fill word 3 without overlap
    assert len({(int(si) << 10) | int(ai) for ai in (0, 1, 1023) for si in (0, 1, 2, (1 << 22) - 1)}) == 12
    # the two branches read different words: u0 is words 0, 1 and u1 words 2, 3 of B0; v0 comes from B1
    u0, u1, v0 = ref.uniforms(SEED, g, k, a, s)
    assert (u0 != u1).all() and (u0 != v0).all() and (u1 != v0).all()
    # another key, another stream
    assert (ref.uniforms(SEED + 1, g, k, a, s)[0] != u0).all()


def test_episode_bits_follow_the_window():
    c, T, DT = -0.6, 0.3, 0.1
    bits = ref.episode_bits(SEED, c, T, DT, g=5, k=2, a=3, steps=40, step_dt=DT)
    t, prev = 0.0, False
    for s in range(40):
        want = bool(ref.noncoop_draw(SEED, c, 5, 2, 3, s)) if ref.window(t, T, DT) else prev
        assert bits[s] == want
        prev, t = want, t + DT


# ---------------------------------------------------------------- the ABI
def test_struct_layout_and_exports():
    nat, lib = _nat()
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert "#define CAGPU_VERSION 12" in hdr and lib.cagpu_version() == 12
    body = re.search(r"typedef struct CaRvoDraw \{(.*?)\} CaRvoDraw;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*\*?(\w+);", body) == [("uint64_t", "seed"), ("double", "collab_coeff"), ("double", "anti_collab_t"),
                                                      ("double", "noise_std"), ("uint8_t", "noise_mask"), ("int64_t", "address")]
    assert [f[0] for f in nat.CaRvoDraw._fields_] == ["seed", "collab_coeff", "anti_collab_t", "noise_std", "noise_mask", "address"]
    assert ctypes.sizeof(nat.CaRvoDraw) == 48
    assert [getattr(nat.CaRvoDraw, f[0]).offset for f in nat.CaRvoDraw._fields_] == [0, 8, 16, 24, 32, 40]
    assert re.search(r"CA_RVO_NONCOOP = 1u << 18", hdr) and nat.RVO_NONCOOP == 1 << 18 == ref.NONCOOP
    assert nat.RVO_NONCOOP > nat.PLAN_VALID
    for n in ("cagpu_step_noise", "cagpu_rvo_draw_at"):
        assert n in nat.EXPORTS and re.search(r"\bint %s\(" % n, hdr) and hasattr(lib, n), n
    assert len(lib.cagpu_step_noise.argtypes) == 9 and len(lib.cagpu_rvo_draw_at.argtypes) == 10


def _fake(nat, E=4, N=4):
    from gym_collision_avoidance_amd import core
    p = core.make_params(E, N)
    fake = 0x1000
    s = nat.CaState(**{n: fake for n in nat.STATE_FIELDS if n not in ("next_action", "turning_dir", "rvo_collab",
                                                                       "rvo_heading_noise", "ext_state")})
    o = nat.CaOut(obs=fake, rewards=fake, done=fake, game_over=fake)
    return p, s, o


def _good(nat, **kw):
    d = dict(seed=SEED, collab_coeff=-0.6, anti_collab_t=0.3, noise_std=0.5, noise_mask=0x3000, address=None)
    d.update(kw)
    return nat.CaRvoDraw(**d)


def test_step_noise_rejections():
    nat, lib = _nat()
    p, s, o = _fake(nat)
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    ar = nat.CaAutoReset(table=0x4000, n_cases=4, env_id_offset=0, case_stride=4, heading_seed=77)
    pd = nat.CaPolicyDraw(cdf=0x5000, policy_bits=0x5000, num_policies=2, ensure=-1, seed=99)
    m = nat.CaMap(static_bits=0x2000, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=55)

    def call(rd, ar_=None, draw=None, x=None, tape=None):
        rc = lib.cagpu_step_noise(B(p), B(s), B(o), tape, None if ar_ is None else B(ar_), x, None if draw is None else B(draw),
                                  B(rd), None)
        return rc, lib.cagpu_last_error()

    cases = [
        (_good(nat, seed=0), {}, b"seed must not be 0"),
        (_good(nat, seed=77), dict(ar_=ar), b"seed equals"),
        (_good(nat, seed=99), dict(ar_=ar, draw=pd), b"seed equals"),
        (_good(nat, seed=55), dict(x=B(nat.CaStepEx(n_steps=1, set=A(ms)))), b"seed equals"),
        (_good(nat, anti_collab_t=0.0), {}, b"anti_collab_t"),
        (_good(nat, anti_collab_t=-1.0), {}, b"anti_collab_t"),
        (_good(nat, anti_collab_t=float("nan")), {}, b"anti_collab_t"),
        (_good(nat, noise_std=-0.5), {}, b"noise_std"),
        (_good(nat, noise_std=float("nan")), {}, b"noise_std"),
        (_good(nat, collab_coeff=0.5, noise_mask=None), {}, b"both branches"),
        (_good(nat, collab_coeff=float("nan"), noise_mask=None), {}, b"both branches"),
        (_good(nat, address=0x6004), {}, b"8-byte aligned"),
    ]
    for rd, kw, text in cases:
        rc, msg = call(rd, **kw)
        assert rc == nat.CA_EINVAL and text in msg and b"cagpu_step_noise" in msg, (text, rc, msg)
    # T <= 0 is only read with c < 0
    rc, msg = call(_good(nat, collab_coeff=0.5, anti_collab_t=0.0, address=0x6004))
    assert rc == nat.CA_EINVAL and b"8-byte aligned" in msg
    # the caller's own numbers beside a CaRvoDraw
    for f in ("rvo_collab", "rvo_heading_noise"):
        setattr(s, f, 0x1000)
        rc, msg = call(_good(nat))
        assert rc == nat.CA_EINVAL and b"beside a CaRvoDraw" in msg, (f, rc, msg)
        setattr(s, f, None)
    # behind the tape's rejections, which stand behind the older ones
    bad_tape = nat.CaActionTape(actions=0x7008, step_stride=2 * 4 * 4)
    rc, msg = call(_good(nat, seed=0), tape=B(bad_tape))
    assert rc == nat.CA_EINVAL and b"CaActionTape.actions" in msg
    rc, msg = call(_good(nat, seed=0), x=B(nat.CaStepEx(n_steps=0)))
    assert rc == nat.CA_EINVAL and b"n_steps must be >= 1" in msg
    s.ext_state = 0x1000
    rc, msg = call(_good(nat, seed=0), x=B(nat.CaStepEx(n_steps=2)))
    assert rc == nat.CA_EINVAL and b"ONE step" in msg
    s.ext_state = None
    assert lib.cagpu_last_kernel() == before      # nothing was selected, let alone launched


def test_null_rd_is_step_tape():
    nat, lib = _nat()
    p, s, o = _fake(nat)
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    m = nat.CaMap(static_bits=0x2000, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=7)
    calls = [
        (None, nat.CaStepEx(n_steps=0)),
        (None, nat.CaStepEx(n_steps=1, snapshot_delta=64)),
        (None, nat.CaStepEx(n_steps=1, map=A(m), set=A(ms))),
        (nat.CaActionTape(actions=0x7008, step_stride=32), nat.CaStepEx(n_steps=2)),
        (nat.CaActionTape(actions=0x7000, step_stride=3), nat.CaStepEx(n_steps=2)),
        (nat.CaActionTape(actions=None, step_stride=32), None),
    ]
    for tape, x in calls:
        args = (B(p), B(s), B(o), None if tape is None else B(tape), None, None if x is None else B(x), None)
        rc_old = lib.cagpu_step_tape(*args, None)
        msg_old = lib.cagpu_last_error()
        rc_new = lib.cagpu_step_noise(*args, None, None)
        assert rc_old == nat.CA_EINVAL and rc_new == rc_old and lib.cagpu_last_error() == msg_old, (rc_old, rc_new, msg_old)
    assert lib.cagpu_step_noise(None, None, None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_last_kernel() == before


def test_rvo_draw_at_rejections():
    nat, lib = _nat()
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    f = 0x1000
    good = _good(nat)

    def call(rd=good, N=4, g=f, k=f, a=f, s=f, n=8, o0=f, o1=f):
        rc = lib.cagpu_rvo_draw_at(None if rd is None else B(rd), N, g, k, a, s, n, o0, o1, None)
        return rc, lib.cagpu_last_error()

    for kw in (dict(rd=None), dict(g=None), dict(k=None), dict(a=None), dict(s=None), dict(o0=None, o1=None), dict(N=0),
               dict(N=1025), dict(n=-1)):
        rc, msg = call(**kw)
        assert rc == nat.CA_EINVAL and b"cagpu_rvo_draw_at" in msg, (kw, rc, msg)
    rc, msg = call(rd=_good(nat, seed=0))
    assert rc == nat.CA_EINVAL and b"seed must not be 0" in msg
    for std in (-1.0, float("nan")):
        rc, msg = call(rd=_good(nat, noise_std=std))
        assert rc == nat.CA_EINVAL and b"noise_std" in msg
    assert call(n=0)[0] == nat.CA_OK            # n == 0 does nothing
    assert lib.cagpu_last_kernel() == before
