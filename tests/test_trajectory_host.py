"""The trajectory tape without a GPU: the C ABI of the recording entry points (include/cagpu.h CaTraj, cagpu_step_traj,
cagpu_rollout_traj) and the host-side assembly (gym_collision_avoidance_amd/trajectory.py) against REFERENCE-RECORDED
episodes: tests/golden/*.npz hold the reference's full per-step state, which determines its global_state_history rows
exactly (a row is logged on exactly the steps step_num rises; its clock is the one before the step, everything else the
state after it, and the logged speed is the action speed act0)."""
import ctypes
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import golden_util as gu  # noqa: E402

HIST_COLS = ("t", "pos_x", "pos_y", "goal_x", "goal_y", "radius", "pref_speed", "vel_x", "vel_y", "act0", "heading")


def reference_histories(ep):
    """the reference's global_state_history[:step_num] of every agent of a golden episode, cut straight from the
    recorded state: list over agents of [len, 11]"""
    i = gu.COLS.index
    out = []
    for a in range(ep.N):
        rows = []
        for t in range(ep.T):
            before, after = ep.state[t, a], ep.state[t + 1, a]
            if after[i("step_num")] == before[i("step_num")] + 1:
                rows.append([before[i("t")]] + [after[i(c)] for c in HIST_COLS[1:]])
        out.append(np.array(rows, dtype=np.float64).reshape(-1, 11))
    return out


def tape_of(ep, n_slots, garbage):
    """rows [T, n_slots, 12] of one env as the step kernels write them: a full row where the agent moved, column 11 = -1
    and `garbage` in the other columns elsewhere; slots beyond the episode's agents are absent (never move)"""
    i = gu.COLS.index
    rows = np.full((ep.T, n_slots, 12), garbage, dtype=np.float64)
    rows[..., 11] = -1.0
    for t in range(ep.T):
        for a in range(ep.N):
            before, after = ep.state[t, a], ep.state[t + 1, a]
            if after[i("step_num")] == before[i("step_num")] + 1:
                rows[t, a, :11] = [before[i("t")]] + [after[i(c)] for c in HIST_COLS[1:]]
                rows[t, a, 11] = before[i("step_num")]
    return rows


def test_header_library_and_binding_agree_on_the_recording_abi():
    from gym_collision_avoidance_amd import _native as nat
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert "#define CAGPU_VERSION 12" in hdr
    assert "typedef struct CaTraj" in hdr and "int cagpu_step_traj(" in hdr and "int cagpu_rollout_traj(" in hdr
    lib = nat.lib()
    assert lib.cagpu_version() == 12 == nat.ABI_VERSION
    assert ctypes.sizeof(nat.CaTraj) == 16
    assert "cagpu_step_traj" in nat.EXPORTS and "cagpu_rollout_traj" in nat.EXPORTS
    for n in ("cagpu_step_traj", "cagpu_rollout_traj"):
        assert getattr(lib, n).restype is ctypes.c_int


def test_recording_calls_with_bad_arguments_are_loud_errors_not_crashes():
    """host-only: every one of these returns before anything is launched"""
    from gym_collision_avoidance_amd import _native as nat, core
    lib = nat.lib()
    B = ctypes.byref
    assert lib.cagpu_step_traj(None, None, None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert b"NULL" in lib.cagpu_last_error()
    assert lib.cagpu_rollout_traj(None, None, None, None, None, 3, 1, 0, None, None) == nat.CA_EINVAL
    assert b"NULL" in lib.cagpu_last_error()
    p, s, o = core.make_params(4, 10), nat.CaState(), nat.CaOut()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    # NULL traj / NULL rows
    for tj in (None, B(nat.CaTraj(rows=None, episode=None)), B(nat.CaTraj(rows=None, episode=base))):
        assert lib.cagpu_step_traj(B(p), B(s), B(o), None, None, None, None, tj, None) == nat.CA_EINVAL
        assert b"CaTraj" in lib.cagpu_last_error()
        assert lib.cagpu_rollout_traj(B(p), B(s), B(o), None, None, 5, 0, 0, tj, None) == nat.CA_EINVAL
        assert b"CaTraj" in lib.cagpu_last_error()
    # misaligned rows (8 bytes off a 16-byte boundary), misaligned episode
    for tj in (nat.CaTraj(rows=base + 8, episode=None), nat.CaTraj(rows=base, episode=base + 2)):
        assert lib.cagpu_step_traj(B(p), B(s), B(o), None, None, None, None, B(tj), None) == nat.CA_EINVAL
        assert b"aligned" in lib.cagpu_last_error()
        assert lib.cagpu_rollout_traj(B(p), B(s), B(o), None, None, 5, 1, 0, B(tj), None) == nat.CA_EINVAL
        assert b"aligned" in lib.cagpu_last_error()
    # a good CaTraj in front of NULL state pointers: the mirrored call's own checks still apply
    ok = nat.CaTraj(rows=base, episode=None)
    assert lib.cagpu_step_traj(B(p), B(s), B(o), None, None, None, None, B(ok), None) == nat.CA_EINVAL
    assert b"NULL" in lib.cagpu_last_error()
    m, ms = nat.CaMap(), nat.CaMapSet()
    assert lib.cagpu_step_traj(B(p), B(s), B(o), None, None, B(m), B(ms), B(ok), None) == nat.CA_EINVAL
    assert b"CaMapSet" in lib.cagpu_last_error()
    assert lib.cagpu_rollout_traj(B(p), B(s), B(o), None, None, 5, 0, 64, B(ok), None) == nat.CA_EINVAL
    assert b"snapshot_delta" in lib.cagpu_last_error()


@pytest.mark.parametrize("name", gu.SCENARIOS)
def test_golden_state_determines_the_reference_history(name):
    """what the tape test below rests on, for every recorded scenario: step_num rises by 0 or 1 per step, t rises by dt on
    exactly those steps, the position is unchanged on the others, and vel == act0 * (cos heading, sin heading) with zero
    error for unicycle agents, i.e. act0 is the logged speed"""
    meta, eps = gu.load(name)
    i = gu.COLS.index
    for ep in eps.values():
        st = ep.state
        dsn = np.diff(st[:, :, i("step_num")], axis=0)
        assert set(np.unique(dsn)) <= {0.0, 1.0}
        moved = dsn == 1
        dt_ = np.diff(st[:, :, i("t")], axis=0)
        assert np.allclose(dt_[moved], meta["dt"], rtol=0, atol=1e-12) and (dt_[~moved] == 0).all()
        for c in ("pos_x", "pos_y"):
            assert (np.diff(st[:, :, i(c)], axis=0)[~moved] == 0).all()
        uni = np.broadcast_to(ep.dynamics[None] != 2, moved.shape) & moved
        after = st[1:]
        h, a0 = after[:, :, i("heading")], after[:, :, i("act0")]
        assert np.array_equal((a0 * np.cos(h))[uni], after[:, :, i("vel_x")][uni])
        assert np.array_equal((a0 * np.sin(h))[uni], after[:, :, i("vel_y")][uni])


@pytest.mark.parametrize("name", gu.SCENARIOS)
def test_episodes_reassembles_the_reference_history_exactly(name):
    """a tape built from reference-recorded episodes -- two episodes of one env back to back under different episode ids,
    one padded absent slot, another env beside it, NaN in the columns the kernels leave alone -- comes back as exactly the
    [step_num, 11] arrays cut from the golden state"""
    from gym_collision_avoidance_amd import trajectory
    meta, eps = gu.load(name)
    keys = sorted(eps)
    first, second = eps[keys[0]], eps[keys[-1]]
    n_slots = first.N + 1
    one = np.concatenate([tape_of(first, n_slots, np.nan), tape_of(second, n_slots, np.nan)])
    T = one.shape[0]
    rows = np.full((T, 2, n_slots, 12), np.nan)
    rows[..., 11] = -1.0
    rows[:, 1] = one
    rows[:first.T, 0] = tape_of(first, n_slots, 7.0)      # env 0: one episode, then nothing moves
    episode = np.zeros((T, 2), dtype=np.int32)
    episode[:first.T, 1], episode[first.T:, 1] = 3, 4
    got = trajectory.episodes(rows, episode, 1)
    assert len(got) == 2 and all(len(g) == n_slots for g in got)
    for g, ep in zip(got, (first, second)):
        want = reference_histories(ep)
        for a in range(ep.N):
            assert g[a].dtype == np.float64 and g[a].shape == want[a].shape
            assert np.array_equal(g[a], want[a]), "agent %d" % a
            assert g[a].shape[0] == int(ep.state[-1, a, gu.COLS.index("step_num")])
        assert g[ep.N].shape == (0, 11)
    assert sum(h.shape[0] for h in reference_histories(first)) > 0
    only = trajectory.episodes(rows, episode, 0)
    assert len(only) == 1 and all(np.array_equal(x, y) for x, y in zip(only[0][:first.N], reference_histories(first)))
    # a host-side reset between the two episodes leaves `episode` alone and shows in `epoch`
    epoch = np.zeros((T, 2), dtype=np.int32)
    epoch[first.T:, 1] = 1
    again = trajectory.episodes(rows, np.zeros((T, 2), dtype=np.int32), 1, epoch=epoch)
    assert len(again) == 2 and all(np.array_equal(x, y) for g, h in zip(again, got) for x, y in zip(g, h))
    assert trajectory.episodes(rows[:0], episode[:0], 0) == []


def test_rvo10_golden_moved_and_idle_counts():
    meta, eps = gu.load("rvo10")
    i = gu.COLS.index("step_num")
    moved = sum(int((np.diff(ep.state[:, :, i], axis=0) == 1).sum()) for ep in eps.values())
    total = sum(ep.T * ep.N for ep in eps.values())
    assert (moved, total - moved) == (5211, 2459)


def test_dataset_samples_against_plain_slicing():
    from gym_collision_avoidance_amd import trajectory
    meta, eps = gu.load("rvo4_swap")
    ep = eps[sorted(eps)[0]]
    hist = reference_histories(ep)
    ego, other = hist[0], hist[1]
    assert ego.shape[0] > 35 and other.shape[0] > 0
    dt = float(meta["dt"])
    goal = ego[0, 3:5]
    H = int(3.0 / dt)
    out = trajectory.dataset_samples(ego, other, goal, dt)
    assert len(out) == ego.shape[0]
    dh = np.diff(np.concatenate([ego[:1, 10], ego[:, 10]]))
    dh = (dh + np.pi) % (2 * np.pi) - np.pi
    for t, d in enumerate(out):
        hi = min(ego.shape[0], t + H)
        assert np.array_equal(d["control_command"], [ego[t, 9], dh[t] / dt])
        assert d["predicted_cmd"].shape == (1, hi - t, 2)
        assert np.array_equal(d["predicted_cmd"][0, :, 0], ego[t:hi, 9])
        assert np.array_equal(d["predicted_cmd"][0, :, 1], dh[t:hi] / dt)
        assert np.array_equal(d["future_positions"], ego[t:hi, 1:3])
        assert np.array_equal(d["robot_state"], ego[t, [1, 2, 10]])
        assert np.array_equal(d["goal_position"], goal)
        tt = min(t, other.shape[0] - 1)
        assert np.array_equal(d["pedestrian_state"]["position"], other[tt, 1:3])
        assert np.array_equal(d["pedestrian_state"]["velocity"], other[t, 7:9] if t < other.shape[0] else np.zeros(2))
    assert out[-1]["future_positions"].shape == (1, 2) and out[0]["future_positions"].shape == (min(H, ego.shape[0]), 2)
    # the heading before the first row, where the caller knows it; the reference script's own quotient
    h0 = ego[0, 10] - 0.25
    assert np.isclose(trajectory.dataset_samples(ego, other, goal, dt, initial_heading=h0)[0]["control_command"][1], 0.25 / dt)
    ref = trajectory.dataset_samples(ego, other, goal, dt, angular="heading")
    assert all(np.array_equal(d["control_command"], [ego[t, 9], ego[t, 10] / dt]) for t, d in enumerate(ref))
    # a shorter horizon, and an ego that outlives the other agent
    short = trajectory.dataset_samples(ego, other[:5], goal, dt, horizon_secs=0.5)
    assert short[0]["future_positions"].shape[0] == int(0.5 / dt)
    assert np.array_equal(short[20]["pedestrian_state"]["position"], other[4, 1:3])
    assert np.array_equal(short[20]["pedestrian_state"]["velocity"], np.zeros(2))
