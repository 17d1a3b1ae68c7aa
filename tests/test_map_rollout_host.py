"""Maps in fused launches without a GPU: the C ABI of cagpu_step_ex_maps / cagpu_map_draw (include/cagpu.h), their ctypes
mirror, the argument checks that return before anything is launched, and the rule of the episode log's `map` column
(episodes.map_column) against a replay of what the device does.

Nothing here launches: every call is made to fail an argument check.  "Passes the checks up to the launch" is shown with a
call whose ONLY fault is a CaAutoReset without cases -- the last check before the launch, behind the map rules."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

B, A = ctypes.byref, ctypes.addressof


def _nat():
    from gym_collision_avoidance_amd import _native as nat
    return nat, nat.lib()


def _fake(nat):
    """host structs whose device pointers are never dereferenced (test_step_ex_host.py's)"""
    from gym_collision_avoidance_amd import core
    p = core.make_params(4, 4)
    fake = 0x1000
    s = nat.CaState(**{n: fake for n in nat.STATE_FIELDS if n not in ("next_action", "turning_dir", "rvo_collab",
                                                                       "rvo_heading_noise", "ext_state")})
    o = nat.CaOut(obs=fake, rewards=fake, done=fake, game_over=fake)
    m = nat.CaMap(static_bits=0x2000, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=7)
    return p, s, o, m, ms


def test_header_binding_and_library_agree_on_the_new_exports():
    nat, lib = _nat()
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert "#define CAGPU_VERSION 12" in hdr and lib.cagpu_version() == 12 == nat.ABI_VERSION
    assert ctypes.sizeof(nat.CaStepEx) == 56 and len(nat.CaStepEx._fields_) == 8
    decl = re.search(r"int cagpu_step_ex_maps\((.*?)\);", hdr, re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "const CaParams *p", "const CaState *s", "const CaOut *o", "const double *ext_actions", "const CaAutoReset *ar",
        "const CaStepEx *x", "const struct CaPolicyDraw *draw", "void *stream"]
    assert lib.cagpu_step_ex_maps.argtypes == lib.cagpu_step_draw.argtypes
    for n in ("cagpu_step_ex_maps", "cagpu_map_draw"):
        assert n in nat.EXPORTS and re.search(r"\bint %s\(" % n, hdr) and hasattr(lib, n), n
        assert getattr(lib, n).restype is ctypes.c_int
    assert len(lib.cagpu_map_draw.argtypes) == 7


def test_argument_checks_of_step_ex_maps():
    nat, lib = _nat()
    p, s, o, m, ms = _fake(nat)
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    no_cases = nat.CaAutoReset(table=None, n_cases=0)   # the one fault of the "good" calls: checked last, behind the map rules

    def maps(ar=None, draw=None, **fields):
        rc = lib.cagpu_step_ex_maps(B(p), B(s), B(o), None, ar, B(nat.CaStepEx(**fields)), draw, None)
        return rc, lib.cagpu_last_error()

    def old(ar=None, **fields):
        rc = lib.cagpu_step_ex(B(p), B(s), B(o), None, ar, B(nat.CaStepEx(**fields)), None)
        return rc, lib.cagpu_last_error()

    # map and set at once
    for fields in (dict(n_steps=1, map=A(m), set=A(ms)), dict(n_steps=3, ring=1, map=A(m), set=A(ms))):
        rc, msg = maps(**fields)
        assert rc == nat.CA_EINVAL and b"cagpu_step_ex_maps: a CaMap and a CaMapSet at once" in msg, (fields, msg)
    # a bad set, single- and multi-step
    for n, ring in ((1, 0), (3, 0), (3, 1)):
        for bad in ("env_map", "bits", "num_maps", "rows", "cell"):
            _, _, _, _, b = _fake(nat)
            if bad == "env_map":
                b.env_map = None
            elif bad == "bits":
                b.map.static_bits = None
            elif bad == "num_maps":
                b.num_maps = 0
            elif bad == "rows":
                b.map.rows = 0
            else:
                b.map.cell = 0.0
            rc, msg = maps(n_steps=n, ring=ring, set=A(b))
            assert rc == nat.CA_EINVAL and b"CaMapSet" in msg, (n, ring, bad, msg)
    # a bad single map
    bm = nat.CaMap(static_bits=0x2000, rows=0, cols=160, cell=0.1)
    rc, msg = maps(n_steps=3, map=A(bm), ar=None)
    assert rc == nat.CA_EINVAL and b"bad CaMap" in msg, msg
    # the per-step inputs belong to ONE step, with a map as without
    for name in ("ext_state", "rvo_collab", "rvo_heading_noise"):
        setattr(s, name, 0x1000)
        for fields in (dict(n_steps=2, map=A(m)), dict(n_steps=1, ring=1, set=A(ms)), dict(n_steps=2)):
            rc, msg = maps(**fields)
            assert rc == nat.CA_EINVAL and b"ONE step" in msg, (name, fields, msg)
        setattr(s, name, None)
    # n_steps, snapshot_delta: the general rules hold
    rc, msg = maps(n_steps=0, map=A(m))
    assert rc == nat.CA_EINVAL and b"n_steps must be >= 1" in msg
    rc, msg = maps(n_steps=3, snapshot_delta=64, set=A(ms))
    assert rc == nat.CA_EINVAL and b"snapshot_delta without ring" in msg
    # a draw is checked as in cagpu_step_draw
    d = nat.CaPolicyDraw(cdf=None, policy_bits=None, num_policies=2, ensure=-1, seed=5)
    rc, msg = maps(n_steps=3, map=A(m), draw=B(d))
    assert rc == nat.CA_EINVAL and b"cagpu_step_ex_maps: NULL CaPolicyDraw.cdf" in msg, msg
    # a good map / set with n_steps = 3 or a ring passes every map rule: what is left is the CaAutoReset without cases --
    # and the same arguments through cagpu_step_ex are refused for the map
    for fields in (dict(n_steps=3, map=A(m)), dict(n_steps=3, set=A(ms)), dict(n_steps=3, ring=1, map=A(m)),
                   dict(n_steps=1, ring=1, set=A(ms))):
        rc, msg = maps(ar=B(no_cases), **fields)
        assert rc == nat.CA_EINVAL and b"bad CaAutoReset" in msg, (fields, msg)
        rc, msg = old(ar=B(no_cases), **fields)
        assert rc == nat.CA_EINVAL and b"cagpu_step_ex" in msg and b"n_steps > 1 or ring" in msg, (fields, msg)
        rc = lib.cagpu_step_draw(B(p), B(s), B(o), None, B(no_cases), B(nat.CaStepEx(**fields)), None, None)
        assert rc == nat.CA_EINVAL and b"n_steps > 1 or ring" in lib.cagpu_last_error()
    # all NULL
    assert lib.cagpu_step_ex_maps(None, None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_last_kernel() == before      # nothing was selected, let alone launched


def test_argument_checks_of_map_draw():
    nat, lib = _nat()
    ok = 0x1000
    for args in ((0, 3, ok, ok, 4, ok), (5, 0, ok, ok, 4, ok), (5, 3, None, ok, 4, ok), (5, 3, ok, None, 4, ok),
                 (5, 3, ok, ok, 4, None), (5, 3, ok, ok, -1, ok)):
        assert lib.cagpu_map_draw(*args, None) == nat.CA_EINVAL, args
        assert b"cagpu_map_draw" in lib.cagpu_last_error()
    assert lib.cagpu_map_draw(5, 3, ok, ok, 0, ok, None) == nat.CA_OK     # n == 0: nothing to do, nothing launched


def _toy_draw(key, e, k, M):
    """stands in for CaMapSet.map_seed's Philox draw: any pure function of (key, env, count) serves the rule"""
    return int((key * 2654435761 + e * 40503 + k * 9973) % 1000003 % M)


@pytest.mark.parametrize("seed", range(6))
def test_map_column_rule_against_a_replay(seed):
    """Replays what the device and the host do to env_map -- host assignments (reset-time or set_env_map), key changes,
    auto-resets that draw under the key in force -- and records the map every episode really ran on.  map_column, given
    only what BatchedSim tracks (the last assignment and its episode, the first episode decided under the key in force)
    and the draws under the CURRENT key, must name that map or -1, never another one; and it must know every episode
    from the last assignment on while the key has not been replaced since."""
    from gym_collision_avoidance_amd import episodes
    rng = np.random.default_rng(seed)
    E, M = 40, 5
    rows_k, rows_e, truth, args = [], [], [], {n: [] for n in ("given_ep", "given_map", "key_from")}
    final_key = None
    keyed_final = bool(seed % 2)
    for e in range(E):
        key = int(rng.integers(1, 1 << 40)) if rng.random() < 0.7 else 0
        rc, env_map = 0, int(rng.integers(M))
        given_ep, given_map, key_from = 0, env_map, 0
        ran, key_changed_at = [], []
        for _ in range(int(rng.integers(3, 30))):
            ev = rng.random()
            if ev < 0.7:                      # an episode ends: logged with index rc, then the auto-reset's draw
                ran.append(env_map)
                rc += 1
                if key:
                    env_map = _toy_draw(key, e, rc, M)
            elif ev < 0.85:                   # set_env_map
                env_map = int(rng.integers(M))
                given_ep, given_map = rc, env_map
            else:                             # set_map_seed (0: draws off)
                key = int(rng.integers(1, 1 << 40)) if rng.random() < 0.6 else 0
                key_from = rc + 1
                key_changed_at.append(rc)
        # one key for the whole batch at drain time: envs whose last key differs get one more change "now"
        if final_key is None:
            final_key = key if (bool(key) == keyed_final) else (12345 if keyed_final else 0)
        if key != final_key:
            key_from = rc + 1
            key_changed_at.append(rc)
        for k, m in enumerate(ran):
            rows_k.append(k); rows_e.append(e); truth.append(m)
            for n, v in (("given_ep", given_ep), ("given_map", given_map), ("key_from", key_from)):
                args[n].append(v)
    k, env, truth = np.array(rows_k), np.array(rows_e), np.array(truth)
    drawn = np.array([_toy_draw(final_key, int(e), int(kk), M) for e, kk in zip(env, k)])
    got = episodes.map_column(k, np.array(args["given_ep"]), np.array(args["given_map"]), np.array(args["key_from"]),
                              bool(final_key), drawn)
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == k.shape
    known = got >= 0
    assert np.array_equal(got[known], truth[known])           # never a wrong index
    assert ((got == -1) | known).all() and known.any()
    must = (np.array(args["key_from"]) == 0) & (k >= np.array(args["given_ep"]))   # (the key never changed)
    assert known[must].all()


def test_map_column_on_torch_tensors():
    torch = pytest.importorskip("torch")
    from gym_collision_avoidance_amd import episodes
    k = torch.tensor([0, 1, 2, 3, 0, 1])
    got = episodes.map_column(k, torch.tensor([0, 0, 0, 0, 1, 1]), torch.tensor([4, 4, 4, 4, 2, 2], dtype=torch.int32),
                              torch.tensor([0, 0, 3, 3, 0, 0]), True, torch.tensor([9, 1, 2, 3, 9, 9], dtype=torch.int32))
    # records 0-1 (given in episode 0, the key in force throughout): the given map, then the draw; records 2-3 (key in force
    # from episode 3 on): unknown, the draw; records 4-5 (given in episode 1): episode 0 ran before that -- unknown --,
    # episode 1 on the given map
    assert got.dtype == torch.int64 and got.tolist() == [4, 1, -1, 3, -1, 2]
    got = episodes.map_column(k, torch.tensor([0, 0, 0, 0, 1, 1]), torch.tensor([4, 4, 4, 4, 2, 2]),
                              torch.tensor([0, 0, 1, 1, 5, 5]), False, torch.zeros(6, dtype=torch.int32))
    # no key: the given map holds from its episode on, if the draws stopped no later than in the episode after it
    assert got.tolist() == [4, 4, 4, 4, -1, 2]
