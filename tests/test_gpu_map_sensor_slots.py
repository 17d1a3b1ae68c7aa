"""Laser scans and occupancy windows for every step of a fused launch (include/cagpu.h: cagpu_tape_poses,
cagpu_laserscan_slots, cagpu_laserscan_history; BatchedSim.rollout(..., keep_steps=True, map_sensors=True)) against a twin
that runs n x (step(), laserscan(), occupancy_grid()).  Every comparison is bit for bit: uint8 indices and float32 words
equal.  Shapes, walls, tables and chunks are tests/test_gpu_map_rollout.py's; the coverage a comparison rests on (auto-resets
inside a launch, in its first and last slot, twice in one launch; several maps drawn) is asserted on the TWIN's game_over."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import golden_util as gu
from tests.test_gpu_map_rollout import CHUNKS, FAMILIES, MAP_KEY, WALL, _last_kernel, _maps, _cases, _mods, _same, _sim, _snap

pytestmark = pytest.mark.gpu

POSE = ("pos_x", "pos_y", "heading", "radius", "step_num")


def _build(N, E, pipeline, kind, table, B=512, H=3, heading_seed=0, plugins=None, packed=False, **kw):
    """kind: "map" (one map) or "set" (3 maps, drawn anew at every auto-reset); both sensors configured and read once on
    the reset state, so the history a launch finds is a real one"""
    sim = _sim(E, N, pipeline, reward_collision_wall=WALL, **kw)
    grids = _maps(3, 50 + N)
    sim.set_map(grids[1] if kind == "map" else grids, num_beams=B, num_to_store=H, **({"map_seed": MAP_KEY} if kind == "set" else {}))
    sim.set_occupancy_grid(packed=packed)
    if plugins is not None:
        sim.set_plugins(plugins)
    sim.set_fixture_table(table, heading_seed=heading_seed)
    sim.reset_from_table()
    sim.laserscan()
    sim.occupancy_grid()
    return sim


def _occ_of(sim):
    return sim.occ if sim.occ is not None else sim.occ_bits


def _twin_step(b, ext=None):
    """one step of the twin and its sensors -> what slot t of the fused launch must hold"""
    b.step(ext)
    b.laserscan()
    b.occupancy_grid()
    w = dict(scan=b.scan.clone(), hist=b.scan_hist.clone(), occ=_occ_of(b).clone(), over=b.game_over.clone().bool())
    w.update({f: b.state[f].clone() for f in POSE})
    if b.env_map is not None:
        w["env_map"] = b.env_map.clone()
    return w


def _check_chunk(a, want, what):
    """every slot of a's kept sensors and poses against the twin's record; the sim's own sensor state against the last"""
    n, k = len(want), a.kept_map_sensors
    assert k is not None and k.n == n
    all_scan, all_idx, all_occ = k.laserscan(), k.laserscan_index(), k.occupancy_grid()
    assert all_scan.dtype == torch.float32 and all_idx.dtype == torch.uint8 and all_scan.shape[0] == n
    for t, w in enumerate(want):
        for f in POSE + (("env_map",) if "env_map" in w else ()):
            assert torch.equal(k.poses[f][t], w[f]), "%s slot %d: pose %s" % (what, t, f)
        assert torch.equal(all_idx[t], w["hist"]), "%s slot %d: scan_hist" % (what, t)
        assert torch.equal(all_scan[t].view(torch.int32), w["scan"].view(torch.int32)), "%s slot %d: scan" % (what, t)
        assert torch.equal(all_occ[t], w["occ"]), "%s slot %d: occupancy" % (what, t)
    for t in sorted({0, n // 2, n - 1}):       # a single slot expanded on its own
        assert torch.equal(k.laserscan(t).view(torch.int32), want[t]["scan"].view(torch.int32)), "%s slot %d alone" % (what, t)
        assert torch.equal(k.laserscan_index(t), want[t]["hist"]) and torch.equal(k.occupancy_grid(t), want[t]["occ"])
    assert torch.equal(a.scan.view(torch.int32), want[-1]["scan"].view(torch.int32)), "%s: sim.scan" % what
    assert torch.equal(a.scan_hist, want[-1]["hist"]) and torch.equal(_occ_of(a), want[-1]["occ"]), "%s: sim sensors" % what


class Cover(object):
    """conditions on the INPUTS, read off the twin's game_over [n, E] of every chunk"""

    def __init__(self):
        self.inside = self.first = self.last = self.twice = 0

    def add(self, want):
        over = torch.stack([w["over"] for w in want]).cpu().numpy()
        if over.shape[0] > 1:
            self.inside += int(over.sum())
            self.first += int(over[0].sum())
            self.last += int(over[-1].sum())
            self.twice += int((over.sum(0) >= 2).sum())


def _run(a, b, chunks=CHUNKS, tape=None):
    cover, t0 = Cover(), 0
    for n in chunks:
        want = [_twin_step(b, None if tape is None else tape[t0 + t]) for t in range(n)]
        ring = a.rollout(n, None if tape is None else tape[t0:t0 + n], keep_steps=True, map_sensors=True)
        assert torch.equal(ring[3].bool(), torch.stack([w["over"] for w in want]))
        _check_chunk(a, want, "chunk of %d at step %d" % (n, t0))
        _same(_snap(a), _snap(b), "state after the chunk of %d" % n)
        cover.add(want)
        t0 += n
    a.check_faults()
    return cover


@pytest.mark.parametrize("kind", ["map", "set"])
@pytest.mark.parametrize("N,E,pipeline", FAMILIES)
def test_every_slot_equals_single_steps(N, E, pipeline, kind):
    """fails on the parent: rollout() has no map_sensors there"""
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    a, b = _build(N, E, pipeline, kind, table), _build(N, E, pipeline, kind, table)
    first = None if kind == "map" else b.env_map.cpu().numpy().copy()
    c = _run(a, b)
    print("N=%d E=%d pipeline=%s %s: resets inside launches %d, in a first slot %d, in a last slot %d, envs twice in one %d"
          % (N, E, pipeline, kind, c.inside, c.first, c.last, c.twice))
    assert c.inside > 0
    # asked of the N = 4 and N = 10 families together: a reset in the first slot of a launch, one in the last, an env that
    # resets twice in one launch.  The N = 4 table meets all three alone; the N = 10 table has no reset in a first slot
    if N == 4:
        assert c.first > 0 and c.last > 0 and c.twice > 0
    elif N == 10:
        assert c.last > 0 and c.twice > 0
    if kind == "set":
        rc = b.state["reset_count"].cpu().numpy()
        assert len(set(b.env_map.cpu().numpy()[rc > 0].tolist())) >= 2
        assert bool((torch.stack([p for p in a.kept_map_sensors.poses["env_map"]]).cpu().numpy() != first[None]).any())


@pytest.mark.parametrize("kind", ["map", "set"])
def test_other_beam_counts_and_history_depths(kind):
    """B = 48: the per-beam stores of the march and the history kernel; H = 2 and 5 beside the reference's 3; the packed
    occupancy format"""
    N, E = 10, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    for B, H, packed in ((48, 3, True), (512, 2, False), (48, 5, False), (50, 3, False)):
        a, b = (_build(N, E, False, kind, table, B=B, H=H, packed=packed) for _ in range(2))
        assert (a.occ is None) == packed
        c = _run(a, b, chunks=(7, 13))
        assert c.inside > 0


def test_action_tape_on_top():
    nat, core, _ = _mods()
    N, E = 4, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    pol = np.full((E, N), nat.POL_RVO, np.int32)
    pol[:, 0] = nat.POL_EXTERNAL
    a, b = (_build(N, E, False, "set", table, plugins=pol) for _ in range(2))
    rng = np.random.default_rng(8)
    T = sum(CHUNKS)
    tape = np.zeros((T, E, N, 2))
    tape[..., 0] = rng.uniform(0.2, 1.5, (T, E, N))
    tape[..., 1] = rng.uniform(-0.5, 0.5, (T, E, N))
    tape = torch.as_tensor(tape, device=a.device)
    c = _run(a, b, tape=tape)
    assert c.inside > 0
    free = _build(N, E, False, "set", table, plugins=pol)
    free.rollout(T, tape[0])
    assert not torch.equal(free.state["pos_x"], a.state["pos_x"])      # the tape steered


@pytest.mark.parametrize("mode", ["heading_seed", "ragged"])
def test_poses_with_a_heading_seed_and_a_ragged_table(mode):
    N, E = 10, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    kw = {}
    if mode == "ragged":
        counts = np.random.default_rng(3).integers(2, N + 1, table.shape[0])
        for c, k in enumerate(counts):
            table[c, k:] = 0.0
        kw["ragged"] = 1
    else:
        kw["heading_seed"] = 0x5EED
    for kind in ("map", "set"):
        a, b = (_build(N, E, False, kind, table, **kw) for _ in range(2))
        c = _run(a, b)
        assert c.inside > 0 and c.twice > 0
        if mode == "ragged":
            absent = (b.state["flags"] & _mods()[0].ABSENT) != 0
            assert bool(absent.any()) and bool((a.kept_map_sensors.poses["radius"][-1][absent] == 0).all())


def test_tape_poses_entry_point_on_a_recorded_chunk():
    """cagpu_tape_poses called by hand on the chunk record_trajectories() kept: the ring equals the twin's state"""
    import ctypes as C
    nat, core, _ = _mods()
    N, E, n = 10, 40, 28
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    a, b = _build(N, E, True, "set", table), _build(N, E, True, "set", table)
    a.record_trajectories()
    start = {f: a.state[f].clone() for f in POSE + ("reset_count",)}
    start_map = a.env_map.clone()
    ring = a.rollout(n, keep_steps=True)
    rows = a.trajectories()["rows"]
    assert rows.shape[0] == n
    rows[rows[..., 11] < 0] = float("nan")          # nothing but column 11 of a row that did not move is read
    rows[..., 11] = torch.nan_to_num(rows[..., 11], nan=-1.0)
    out = {f: torch.empty((n, E, N), dtype=torch.int32 if f == "step_num" else torch.float64, device=a.device) for f in POSE}
    out["env_map"] = torch.empty((n, E), dtype=torch.int32, device=a.device)
    pr = nat.CaPoseRing(**{f: t.data_ptr() for f, t in out.items()})
    cs = nat.CaState(**{f: t.data_ptr() for f, t in start.items()})
    nat.check(a.lib.cagpu_tape_poses(C.byref(a.p), C.byref(cs), start_map.data_ptr(), C.byref(nat.CaTraj(rows=rows.data_ptr())),
                                     ring[3].data_ptr(), n, a._ar_ref, C.byref(a._maps), C.byref(pr), a._stream()))
    resets = 0
    for t in range(n):
        b.step()
        resets += int(b.game_over.sum())
        for f in POSE:
            assert torch.equal(out[f][t], b.state[f]), (t, f)
        assert torch.equal(out["env_map"][t], b.env_map), t
    assert resets > 0


def test_golden_laser_episode_as_one_launch():
    """tests/golden/laser4.npz, the reference-recorded episode, as ONE fused launch over an action tape: every slot's scan
    against the recorded one, held to what test_gpu_parity.py::test_laserscan_golden_episode holds single steps to"""
    from tests.test_gpu_parity import _golden_sim, _laser_idx
    meta, eps = gu.load("laser4")
    ep = eps[0]
    g = _golden_sim(meta, ep)
    g.set_map(ep.static_map)
    cases, head = ep.case()
    g.reset(cases[None], headings=head[None])
    mism = int((_laser_idx(g.laserscan().cpu().numpy()[0]) != ep.laser[0]).sum())
    g.rollout(ep.T, np.asarray(ep.ext)[:, None], keep_steps=True, map_sensors=True)
    scans = g.kept_map_sensors.laserscan().cpu().numpy()
    for t in range(ep.T):
        mism += int((_laser_idx(scans[t, 0]) != ep.laser[t + 1]).sum())
    assert mism <= 3, mism       # a sample within 1 ulp of a cell edge may floor differently (libm cos / sin)
    i = gu.COLS.index
    np.testing.assert_allclose(g.kept_map_sensors.poses["pos_x"].cpu().numpy()[:, 0], ep.state[1:, :, i("pos_x")], rtol=0, atol=1e-4)


def test_single_launch_batches_fill_the_same_object():
    """stochastic RVO draws run between steps: rollout() advances by single launches and calls the sensors per step"""
    N, E = 4, 12
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    a, b = (_build(N, E, False, "map", table) for _ in range(2))
    for s in (a, b):
        s.set_rvo_stochastic(heading_noise=np.ones((E, N), bool), seed=11)
    want = [_twin_step(b) for _ in range(9)]
    a.rollout(9, keep_steps=True, map_sensors=True)
    _check_chunk(a, want, "single launches")


def test_refusals_come_before_any_launch():
    nat, core, _ = _mods()
    N, E = 4, 12
    table = _cases(3 * E + 1, N, 104, near=1.0)
    a = _build(N, E, False, "map", table)
    a.step()
    before, name = _snap(a), _last_kernel()
    with pytest.raises(nat.CagpuError, match="keep_steps"):
        a.rollout(5, map_sensors=True)
    a.set_case_stream(window=4, seed=3)
    a.reset_from_stream()
    a.step()
    before, name = _snap(a), _last_kernel()
    with pytest.raises(nat.CagpuError, match="case stream"):
        a.rollout(5, keep_steps=True, map_sensors=True)
    assert _last_kernel() == name and a.kept_map_sensors is None
    _same(_snap(a), before, "a refused rollout")
    free = _sim(E, N, False, reward_collision_wall=WALL)
    free.set_fixture_table(table)
    free.reset_from_table()
    with pytest.raises(nat.CagpuError, match="set_map"):
        free.rollout(5, keep_steps=True, map_sensors=True)
    # the byte budget: the launch that would exceed it raises, nothing is taken
    c = _build(N, E, False, "map", table)
    c.record_trajectories(max_bytes=20 * c.traj_step_bytes)
    before = _snap(c)
    with pytest.raises(nat.CagpuError, match="max_bytes"):
        c.rollout(19, keep_steps=True, map_sensors=True)
    _same(_snap(c), before, "over the budget")
    assert c.tape_bytes == 0
    c.rollout(2, keep_steps=True, map_sensors=True)
    assert c.tape_bytes == 2 * c.traj_step_bytes


@pytest.mark.parametrize("pipeline,kind,fresh", [(True, "set", True), (False, "map", True), (True, "map", False),
                                                  (False, "set", False)])
def test_ring_hands_out_the_sensors_of_every_step(pipeline, kind, fresh):
    """enable_lookahead(k, map_sensors=True) against a twin without a ring, over several refills and one rewind in the
    middle of a ring; the sensor tensors are read WITHOUT sync() (plain attributes): they are the handed-out step's"""
    N, E = 10, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    a, b = _build(N, E, pipeline, kind, table), _build(N, E, pipeline, kind, table)
    assert a.lookahead_ok()
    a.enable_lookahead(8, fresh=fresh, map_sensors=True)
    resets = [0]

    def sensors(what):
        assert torch.equal(a.scan.view(torch.int32), b.scan.view(torch.int32)), "%s: scan" % what
        assert torch.equal(a.scan_hist, b.scan_hist) and torch.equal(_occ_of(a), _occ_of(b)), "%s: hist / occupancy" % what

    def slot(what):
        obs, rew, done, over = a.step_lookahead()
        w = _twin_step(b)
        resets[0] += int(w["over"].sum())
        assert torch.equal(obs, b.obs) and torch.equal(rew, b.rewards) and torch.equal(over, w["over"]), what
        sensors(what)

    for t in range(8):
        slot("ring 1 slot %d" % t)
    for t in range(5):
        slot("ring 2 slot %d" % t)
    ahead = a._state["reset_count"].clone()
    st = a.state                      # a state read: the rewind, in the middle of the second ring
    assert a._la["rewinds"] == 1 and st is a._state
    assert int((ahead - a._state["reset_count"]).sum()) > 0          # the steps thrown away held auto-resets
    _same(_snap(a), _snap(b), "after the rewind at slot 5 of 8")
    sensors("after the rewind")
    for t in range(19):
        slot("after the rewind, step %d" % t)
    _same(_snap(a), _snap(b), "at the end")
    assert a._la["fills"] >= 4 and resets[0] > 0
    assert a._traj is None and not a._traj_on        # the tape of a refill is transient
    a.check_faults()


def _laser_env(Env, E, grids, per_env, **kw):
    env = Env(num_envs=E, **kw)
    env.set_fixture_suite(4, policies="RVO", table=_cases(3 * E + 1, 4, 104, near=1.0))
    env.set_static_map(list(grids) if per_env else grids[0], per_env=per_env)
    return env


@pytest.mark.parametrize("per_env", [False, True])
def test_env_senses_the_map_in_the_ring(per_env):
    from tests import envtools
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        E, grids = 12, _maps(3, 31)
        ring, roll, b = _laser_env(Env, E, grids, per_env), _laser_env(Env, E, grids, per_env), _laser_env(Env, E, grids, per_env, lookahead=0)
        ring.sense_map_in_ring()
        roll.sense_map_in_ring()
        for env in (ring, roll, b):
            np.random.seed(23)
            env.reset()
            env._sim.p.reward_collision_wall = WALL
            env._sim.p.reward_min = min(env._sim.p.reward_min, WALL)
        assert ring._la_on and not b._la_on and ring._sim._la["ms"]
        resets = 0
        for n in (1, 6, 17):
            scans, occs = [], []
            for t in range(n):
                obs, rew, over, _, info = b.step(None)
                resets += int(over.sum())
                o2, r2, over2, _, info2 = ring.step(None)
                assert torch.equal(o2, obs) and torch.equal(r2, rew) and torch.equal(over2, over)
                assert torch.equal(ring.laserscan.view(torch.int32), b.laserscan.view(torch.int32)), (n, t)      # every row
                assert not ring._map_stale
                scans.append(b.laserscan.clone())
                if b.occupancy_grid is not None:
                    assert torch.equal(ring.occupancy_grid, b.occupancy_grid)
                    occs.append(b.occupancy_grid.clone())
                if n == 17 and t == 9:
                    ring._sim.state          # a state read in the middle of a ring: the rewind
                    assert torch.equal(ring.laserscan.view(torch.int32), b.laserscan.view(torch.int32))
            o1, r1, over1, _, info1 = roll.rollout(n, keep_steps=True)
            assert torch.equal(o1[-1], obs) and torch.equal(over1[-1], over)
            assert torch.equal(info1["laserscan"].view(torch.int32), torch.stack(scans).view(torch.int32))
            if occs:
                assert torch.equal(info1["occupancy_grid"], torch.stack(occs))
            assert torch.equal(roll.laserscan.view(torch.int32), b.laserscan.view(torch.int32))
            if per_env:
                assert torch.equal(roll.map_index, b.map_index)
        assert ring._sim._la["fills"] > 1 and ring._sim._la["rewinds"] >= 1 and resets > 0
        # a step with its own dt goes through sync(), a single launch and the env's own scan: the history keeps counting steps
        b.step(None, dt=Config.DT / 2)
        ring.step(None, dt=Config.DT / 2)
        assert torch.equal(ring.laserscan.view(torch.int32), b.laserscan.view(torch.int32))
        ring.sense_map_in_ring(False)
        assert not ring._la_on
        b.step(None)
        ring.step(None)
        assert torch.equal(ring.laserscan.view(torch.int32), b.laserscan.view(torch.int32))
    finally:
        envtools.default()


def test_off_means_off():
    """a sim that went through the feature and one that never heard of it: without map_sensors every launch names the same
    kernel (the strings tests/test_gpu_map_rollout.py pins), the transient tape is gone, and states and outputs are equal"""
    N, E = 10, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    for pipeline in (True, False):
        a, b = _build(N, E, pipeline, "set", table), _build(N, E, pipeline, "set", table)
        a.rollout(9, keep_steps=True, map_sensors=True)
        used = _last_kernel()
        b.rollout(9, keep_steps=True)
        plain = _last_kernel()
        # the transient tape rode on the one launch that asked for the sensors ...
        # (the pipelined kernel names its tape instantiation; the general kernel's string never shows a tape)
        assert (" traj" in used) == pipeline and " traj" not in plain and used.replace(" traj", "") == plain
        assert plain.startswith("ca_pipe_kernel<10, 4, true>" if pipeline else "ca_kernel<256, ") and " set" in plain
        assert a._traj is None and not a._traj_on and b.kept_map_sensors is None      # ... and is gone
        names = {}
        for s in (a, b):
            got = names.setdefault(s, [])
            s.step()
            got.append(_last_kernel())
            s.rollout(7)
            got.append(_last_kernel())
            s.rollout(5, keep_steps=True)
            got.append(_last_kernel())
            assert s.kept_map_sensors is None
            s.laserscan()
            got.append(_last_kernel())          # (a scan names no kernel: still the rollout's string)
            s.enable_lookahead(8)
            for t in range(8):
                s.step_lookahead()
                if t == 0:
                    got.append(_last_kernel())
            s.sync()
            s.laserscan()
        assert names[a] == names[b] and all(" traj" not in k for k in names[a]), names
        assert names[a][0].endswith(" map") and " set" in names[a][1] and names[a][3] == names[a][2]
        # (the newest row: a's history counted the nine steps of its first rollout, b's did not)
        assert torch.equal(a.scan[:, :, 0].view(torch.int32), b.scan[:, :, 0].view(torch.int32))
        assert torch.equal(a.scan_hist[:, :, 0], b.scan_hist[:, :, 0])
        _same(_snap(a), _snap(b), "with and without the feature")
