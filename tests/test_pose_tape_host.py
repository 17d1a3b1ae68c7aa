"""The per-slot map sensors of a fused launch without a GPU (include/cagpu.h: cagpu_tape_poses, cagpu_laserscan_slots,
cagpu_laserscan_history): the two rules as tests/pose_tape_ref.py states them, held to REFERENCE-RECORDED episodes
(tests/golden/*.npz: the full per-step state, from which tests/test_trajectory_host.py::tape_of builds the tape the step
kernels would have written) and to tests/laserscan_ref.py's own history roll; the C ABI of the three entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import golden_util as gu  # noqa: E402
from tests import laserscan_ref as lref  # noqa: E402
from tests import pose_tape_ref as ptr  # noqa: E402
from tests.test_trajectory_host import tape_of  # noqa: E402

GARBAGE = -12345.678   # what the columns the kernels leave alone hold (NaN in a second pass)


def _start(ep, n_slots):
    """the recorded state at t = 0, padded with absent slots (zeros, as a ragged reset leaves them)"""
    out = {f: np.zeros((1, n_slots)) for f in ("pos_x", "pos_y", "heading", "radius")}
    for f in out:
        out[f][0, :ep.N] = ep.col(0, f)
    out["step_num"] = np.zeros((1, n_slots), np.int32)
    out["step_num"][0, :ep.N] = ep.col(0, "step_num")
    return out


def _assert_slot(got, t, ep, t_state, what):
    for f in ("pos_x", "pos_y", "heading", "radius"):
        assert np.array_equal(got[f][t, 0, :ep.N], ep.col(t_state, f)), "%s: %s" % (what, f)
        assert (got[f][t, 0, ep.N:] == 0).all(), what
    assert np.array_equal(got["step_num"][t, 0, :ep.N], ep.col(t_state, "step_num").astype(np.int32)), "%s: step_num" % what


@pytest.mark.parametrize("garbage", [GARBAGE, np.nan])
@pytest.mark.parametrize("name", gu.SCENARIOS)
def test_restated_poses_equal_the_recorded_state_after_every_step(name, garbage):
    meta, eps = gu.load(name)
    moved = 0
    for c, ep in eps.items():
        n_slots = ep.N + 1
        rows = tape_of(ep, n_slots, garbage)[:, None]            # [T, 1, n_slots, 12]
        got = ptr.poses(_start(ep, n_slots), rows, np.zeros((ep.T, 1), np.uint8))
        for t in range(ep.T):
            _assert_slot(got, t, ep, t + 1, "%s case %d step %d" % (name, c, t))
        moved += int((rows[..., 11] >= 0).sum())
        assert (rows[..., 11] < 0).any()                          # rows whose other columns are garbage were in it
    assert moved > 0


@pytest.mark.parametrize("name", gu.SCENARIOS)
def test_synthetic_reset_between_two_golden_episodes(name):
    """two recorded episodes of one env back to back, the first ending in a game over with a table attached: the slot of
    the reset holds the second episode's recorded START state (heading included), the slots behind it its states"""
    meta, eps = gu.load(name)
    keys = sorted(eps)
    first, second = eps[keys[0]], eps[keys[-1]]
    assert first.N == second.N
    n_slots = first.N + 1
    rows = np.concatenate([tape_of(first, n_slots, np.nan), tape_of(second, n_slots, np.nan)])[:, None]
    over = np.zeros((first.T + second.T, 1), np.uint8)
    over[first.T - 1] = 1
    case, head = second.case()
    table = np.zeros((3, n_slots, 6))
    table[2, :second.N] = case
    calls = []

    def next_start(e, k):
        calls.append((e, k))
        row = ptr.table_case(e, k, n_cases=3, env_id_offset=1, num_envs=1)     # episode 1 of env 0: case (1 + 0 + 1) % 3
        hd = None
        if not meta["evaluate"]:      # training mode: the reference draws the initial headings (the heading-seed path)
            hd = np.zeros(n_slots)
            hd[:second.N] = head
        return ptr.start_pose(table[row], ragged=True, headings=hd)

    got = ptr.poses(_start(first, n_slots), rows, over, reset_count=[0], next_start=next_start)
    assert calls == [(0, 1)]
    for t in range(first.T - 1):
        _assert_slot(got, t, first, t + 1, "%s first episode step %d" % (name, t))
    _assert_slot(got, first.T - 1, second, 0, "%s the reset" % name)
    assert (got["step_num"][first.T - 1] == 0).all()
    for t in range(second.T):
        _assert_slot(got, first.T + t, second, t + 1, "%s second episode step %d" % (name, t))


def test_start_pose_of_a_ragged_table_row():
    row = np.array([[1., 2., 4., 6., 1., .3], [0., 0., 0., 0., 0., 0.], [-1., 0., 3., 0., 1., -.5]])
    px, py, hd, rad = ptr.start_pose(row, ragged=True)
    assert px.tolist() == [1., 0., 0.] and py.tolist() == [2., 0., 0.] and rad.tolist() == [.3, 0., 0.]
    assert hd[0] == np.arctan2(4., 3.) and hd[1] == 0. and hd[2] == 0.
    px, py, hd, rad = ptr.start_pose(row, ragged=False)
    assert rad.tolist() == [.3, 0., -.5] and px[2] == -1. and hd[2] == 0.0


@pytest.mark.parametrize("first_at", [(0, 4, 8), (4,), (8,), (0,), (), (2, 3)])
def test_history_rule_equals_the_sensor_roll(first_at):
    """tests/laserscan_ref.py rolls one measurement at a time; the rule restates any slot from the index rows alone.  A
    first measurement at the start, inside and at the end of the sequence, and none at all (only the carried history)."""
    rng = np.random.default_rng(5 + len(first_at))
    n, A, H, B = 9, 5, 3, 7
    idx = rng.integers(0, 256, (n, A, B)).astype(np.uint8)
    carried = rng.integers(0, 256, (A, H, B)).astype(np.uint8)
    step_num = rng.integers(1, 50, (n, A)).astype(np.int32)
    for u in first_at:
        step_num[u, :3] = 0           # (agents 3 and 4 never start an episode inside the sequence)
    step_num[6, 4] = 0 if first_at else step_num[6, 4]
    hist = carried
    for t in range(n):
        hist = lref.roll_history(hist, idx[t], step_num[t] == 0)
        assert np.array_equal(ptr.history(idx, step_num, carried, t), hist), t
    wrong = lref.roll_history(carried, idx[0], step_num[0] == 0, wrong_way=True)
    assert not np.array_equal(ptr.history(idx, step_num, carried, 0), wrong)


def test_header_library_and_binding_agree_on_the_new_symbols():
    from gym_collision_avoidance_amd import _native as nat
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert "#define CAGPU_VERSION 12" in hdr and "typedef struct CaPoseRing" in hdr
    lib = nat.lib()
    assert lib.cagpu_version() == 12 == nat.ABI_VERSION
    assert ctypes.sizeof(nat.CaPoseRing) == 48
    for n in ("cagpu_tape_poses", "cagpu_laserscan_slots", "cagpu_laserscan_history"):
        assert ("int %s(" % n) in hdr and n in nat.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    # every older struct keeps its size
    assert ctypes.sizeof(nat.CaStepEx) == 56 and ctypes.sizeof(nat.CaTraj) == 16 and ctypes.sizeof(nat.CaScan) == 64
    assert ctypes.sizeof(nat.CaMapSet) == 64 and ctypes.sizeof(nat.CaAutoReset) == 56


def _aligned(n_bytes=4096):
    buf = (ctypes.c_char * (n_bytes + 16))()
    base = ctypes.addressof(buf)
    return buf, base + (-base) % 16


def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    """host-only: every one of these returns CA_EINVAL before anything is launched (the pointers are host addresses)"""
    from gym_collision_avoidance_amd import _native as nat, core
    lib, B = nat.lib(), ctypes.byref
    keep, a = _aligned()
    p = core.make_params(4, 10)
    st = nat.CaState(pos_x=a, pos_y=a, heading=a, radius=a, step_num=a, reset_count=a)
    tj = nat.CaTraj(rows=a, episode=None)
    ring = nat.CaPoseRing(pos_x=a, pos_y=a, heading=a, radius=a, step_num=a, env_map=None)
    ar = nat.CaAutoReset(table=a, n_cases=3, case_stride=4)
    ms = nat.CaMapSet(map=nat.CaMap(static_bits=a, rows=160, cols=160, cell=0.1, origin_r=80., origin_c=80.), env_map=a,
                      num_maps=2, map_seed=7)

    def poses(p_=p, st_=st, em=None, tj_=tj, over=a, n=3, ar_=ar, ms_=None, ring_=ring):
        ref = lambda x: None if x is None else B(x)
        return lib.cagpu_tape_poses(ref(p_), ref(st_), em, ref(tj_), over, n, ref(ar_), ref(ms_), ref(ring_), None)

    def err(rc, word):
        assert rc == nat.CA_EINVAL, rc
        assert word.encode() in lib.cagpu_last_error(), lib.cagpu_last_error()

    for kw in (dict(p_=None), dict(st_=None), dict(tj_=None), dict(over=None), dict(ring_=None)):
        err(poses(**kw), "NULL")
    err(poses(p_=core.make_params(4, 2000)), "sizes")
    bad = core.make_params(4, 10)
    bad.num_envs = 0
    err(poses(p_=bad), "sizes")
    err(poses(n=-1), "n_steps")
    err(poses(st_=nat.CaState(pos_x=a, pos_y=a, heading=a, radius=a, step_num=a)), "state pointer")      # no reset_count
    err(poses(tj_=nat.CaTraj(rows=None)), "traj->rows")
    err(poses(tj_=nat.CaTraj(rows=a + 8)), "aligned")
    err(poses(ms_=ms), "start_env_map")                                 # a set without the start maps
    err(poses(ms_=ms, em=a), "env_map")                                 # ... without the ring's env_map
    err(poses(ms_=nat.CaMapSet(num_maps=0), em=a), "num_maps")
    err(poses(ar_=nat.CaAutoReset(table=None, n_cases=3)), "CaAutoReset")
    err(poses(ring_=nat.CaPoseRing(pos_x=a, pos_y=a + 8, heading=a, radius=a, step_num=a)), "aligned")
    err(poses(ring_=nat.CaPoseRing(pos_x=a, pos_y=a, heading=a, radius=a, step_num=None)), "CaPoseRing")
    assert poses(n=0) == nat.CA_OK                                      # nothing to do, nothing launched

    sc = nat.CaScan(hist=a, out=a, num_beams=512, num_to_store=3, num_ranges=60, min_angle=-1.5, max_angle=1.5,
                    range_res=0.1, max_range=6.0)
    mp = nat.CaMap(static_bits=None, rows=160, cols=160, cell=0.1, origin_r=80., origin_c=80.)

    def slots(p_=p, ring_=ring, n=3, mp_=mp, ms_=None, sc_=sc, idx=a):
        ref = lambda x: None if x is None else B(x)
        return lib.cagpu_laserscan_slots(ref(p_), ref(ring_), n, ref(mp_), ref(ms_), ref(sc_), idx, None)

    for kw in (dict(p_=None), dict(ring_=None), dict(sc_=None), dict(mp_=None)):
        err(slots(**kw), "NULL")
    err(slots(ms_=ms), "map and set at once")
    err(slots(p_=bad), "sizes")
    err(slots(n=-2), "n_steps")
    err(slots(idx=None), "idx")
    err(slots(idx=a + 4), "aligned")
    err(slots(mp_=None, ms_=ms), "env_map")                             # the ring of a set launch carries its maps
    err(slots(mp_=None, ms_=nat.CaMapSet(num_maps=2)), "CaMapSet")
    err(slots(ring_=nat.CaPoseRing(pos_x=None, pos_y=a, heading=a, radius=a, step_num=a)), "CaPoseRing")
    err(slots(sc_=nat.CaScan(num_beams=1, num_to_store=3, num_ranges=60)), "CaScan")
    err(slots(mp_=nat.CaMap(rows=0, cols=160, cell=0.1)), "CaMap")
    assert slots(n=0) == nat.CA_OK

    def history(p_=p, sc_=sc, idx=a, sn=a, n=5, first=0, count=5, ho=a + 64, out=a + 128):
        ref = lambda x: None if x is None else B(x)
        return lib.cagpu_laserscan_history(ref(p_), ref(sc_), idx, sn, n, first, count, ho, out, None)

    for kw in (dict(p_=None), dict(sc_=None)):
        err(history(**kw), "NULL")
    err(history(p_=bad), "sizes")
    err(history(sc_=nat.CaScan(hist=a, num_beams=512, num_to_store=0, num_ranges=60)), "CaScan")
    for kw in (dict(n=0, count=0), dict(first=-1), dict(count=-1), dict(first=3, count=3), dict(first=5, count=1)):
        err(history(**kw), "slots")
    for kw in (dict(idx=None), dict(sn=None), dict(idx=a + 1), dict(sn=a + 4)):
        err(history(**kw), "aligned")
    err(history(sc_=nat.CaScan(hist=None, num_beams=512, num_to_store=3, num_ranges=60)), "CaScan.hist")
    err(history(ho=None, out=None), "outputs")
    err(history(ho=a + 8), "aligned")
    err(history(ho=a, count=2), "in place")                              # hist_out == CaScan.hist: one slot only
    assert history(count=0) == nat.CA_OK
    del keep
