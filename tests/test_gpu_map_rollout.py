"""Static maps in fused launches (include/cagpu.h cagpu_step_ex_maps): rollout(n) and the look-ahead ring of a batch with a
map or a map set are n single steps, bit for bit -- walls, map draws at the auto-resets, the records on top, the env API.

Shapes, walls and tables are tests/test_gpu_map_sets.py's.  reward_collision_wall has a value nothing else produces, so a
wall collision shows in `rewards`; every comparison asserts that its window held wall collisions and auto-resets."""
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import envtools
from tests.test_gpu_map_sets import STATE, _cases, _draw, _last_kernel, _maps, _mods, _sim

pytestmark = pytest.mark.gpu

WALL = -0.375      # reward_collision_wall: exact in float32; getting-close rewards lie in [-0.2, -0.1], a collision pays -0.25
FAMILIES = [(4, 40, False), (10, 40, False), (10, 40, True), (70, 6, False), (50, 12, False)]
MAP_KEY = 4242     # set_map's map_seed: equal seeds give twins the same key at every explicit reset
CHUNKS = (1, 7, 28)


def _build(N, E, pipeline, kind, table, **kw):
    """kind: "map" (one map), "set" (3 maps, drawn anew at every auto-reset), None (no map)"""
    sim = _sim(E, N, pipeline, reward_collision_wall=WALL, **kw)
    if kind == "map":
        sim.set_map(_maps(3, 50 + N)[1])
    elif kind == "set":
        sim.set_map(_maps(3, 50 + N), map_seed=MAP_KEY)
    sim.set_fixture_table(table)
    sim.reset_from_table()
    return sim


def _snap(sim, envs=slice(None)):
    st = sim.state
    d = {n: st[n][envs].cpu().numpy().copy() for n in STATE}
    d.update(obs=sim.obs[envs].cpu().numpy().copy(), rewards=sim.rewards[envs].cpu().numpy().copy(),
             done=sim.done[envs].cpu().numpy().copy(), game_over=sim.game_over[envs].cpu().numpy().copy())
    if sim.env_map is not None:
        d["env_map"] = sim.env_map[envs].cpu().numpy().copy()
    return d


def _same(a, b, what):
    assert sorted(a) == sorted(b)
    for n in a:
        assert np.array_equal(a[n], b[n], equal_nan=True), "%s: %s differs" % (what, n)


def _wall_hits(sim):
    return int((sim.rewards == WALL).sum())


def _fused_name(N, pipeline, n, kind):
    """what cagpu_last_kernel() must say of a rollout of n steps"""
    k = _last_kernel()
    # " set": the n-step kernels' MSET instantiations ran (a set, fused); " map": every other launch with a map or a set
    sfx = " set" if (kind == "set" and n > 1 and N <= 64) else " map"
    assert k.endswith(sfx) or (sfx + " ") in k, k
    assert (" set" in k) == (sfx == " set"), k
    if N > 64:
        assert k.startswith("ca_big_kernel"), k          # (a rollout is n launches of the large-env kernel)
    elif pipeline:
        assert k.startswith("ca_pipe_kernel<%d, 4, %s>" % (N, "true" if n > 1 else "false")), k
    else:
        m = re.match(r"ca_kernel<(\d+), (true|false), (\d+), (true|false), ", k)
        assert m and m.group(4) == ("true" if n > 1 else "false"), k


def _check_draws(sim, first, key, M):
    rc = sim.state["reset_count"].cpu().numpy()
    got = sim.env_map.cpu().numpy()
    want = np.array([first[e] if rc[e] == 0 else _draw(key, e, int(rc[e]), M) for e in range(len(rc))])
    assert np.array_equal(got, want)
    return set(got[rc > 0].tolist())


@pytest.mark.parametrize("kind", ["map", "set"])
@pytest.mark.parametrize("N,E,pipeline", FAMILIES)
def test_rollout_equals_single_steps(N, E, pipeline, kind):
    """fails on the parent: there rollout() builds its launch without the map -- no walls, no map draws"""
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    a, b, c = _build(N, E, pipeline, kind, table), _build(N, E, pipeline, kind, table), _build(N, E, pipeline, None, table)
    first = None
    if kind == "set":
        assert a.map_seed == b.map_seed != 0
        first = a.env_map.cpu().numpy().copy()
    hits, t = 0, 0
    for n in CHUNKS:
        a.rollout(n)
        _fused_name(N, pipeline, n, kind)
        c.rollout(n)
        assert " map" not in _last_kernel() and " set" not in _last_kernel()
        for _ in range(n):
            b.step()
            hits += _wall_hits(b)
        t += n
        _same(_snap(a), _snap(b), "%s after %d steps" % (kind, t))
    resets = int(b.state["reset_count"].sum())
    print("N=%d E=%d pipeline=%s %s: %d wall collisions, %d auto-resets in %d steps" % (N, E, pipeline, kind, hits, resets, t))
    assert hits > 0 and resets > 0
    if kind == "set":
        drawn = _check_draws(a, first, a.map_seed, 3)
        assert len(drawn) >= 2, drawn
    sa, sc = _snap(a), _snap(c)
    assert any(not np.array_equal(sa[n], sc[n], equal_nan=True) for n in STATE)     # without the map: another run
    a.check_faults()


def test_split_rollout_carries_the_set():
    """a batch too large for the fused n-step kernel to be resident at once: launch_main runs the rollout as single
    launches, each with the set"""
    N, M = 10, 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    E = 6 * (4 * cus + 8)          # 6-env tiles, more workgroups than four per CU
    table = _cases(1024, N, 110, near=1.0)
    a, b = _build(N, E, False, "set", table), _build(N, E, False, "set", table)
    first = a.env_map.cpu().numpy().copy()
    sample = np.r_[0:16, E // 2:E // 2 + 16, E - 16:E]
    hits = 0
    for n in (7, 13):
        a.rollout(n)
        k = _last_kernel()
        m = re.match(r"ca_kernel<256, (true|false), 10, (true|false), ", k)
        assert m and m.group(2) == "false" and k.endswith(" map"), k      # the single-step instantiation ran last
        for _ in range(n):
            b.step()
            hits += _wall_hits(b)
        assert _last_kernel() == k
        _same(_snap(a, sample), _snap(b, sample), "split, %d steps" % n)
        assert torch.equal(a.env_map, b.env_map) and torch.equal(a.state["reset_count"], b.state["reset_count"])
    assert hits > 0 and int(b.state["reset_count"].sum()) > 0
    rc = a.state["reset_count"].cpu().numpy()
    got = a.env_map.cpu().numpy()
    for e in sample:
        assert got[e] == (first[e] if rc[e] == 0 else _draw(a.map_seed, int(e), int(rc[e]), M))
    a.check_faults()


@pytest.mark.parametrize("pipeline,kind,fresh", [(True, "map", True), (True, "set", True), (False, "map", True),
                                                  (False, "set", True), (True, "set", False)])
def test_ring_equals_single_steps(pipeline, kind, fresh):
    N, E = 10, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    a, b = _build(N, E, pipeline, kind, table), _build(N, E, pipeline, kind, table)
    assert a.lookahead_ok()
    a.enable_lookahead(8, fresh=fresh)
    hits = [0]

    def slot(what):
        obs, rew, done, over = a.step_lookahead()
        b.step()
        hits[0] += _wall_hits(b)
        assert torch.equal(obs, b.obs) and torch.equal(rew, b.rewards), what
        assert torch.equal(done, b.done.bool()) and torch.equal(over, b.game_over.bool()), what

    for t in range(8):
        slot("ring 1 slot %d" % t)
    k = _last_kernel()      # (b's single step ran last; the ring's own launch is checked through its snapshot mode below)
    assert " map" in k, k
    assert list(a._la["in_kernel"].values()) == [pipeline]      # in-kernel snapshot: the pipelined n-step kernel only
    for t in range(5):
        slot("ring 2 slot %d" % t)
    ahead = None if kind == "map" else a._env_map.clone()       # (the ring has run 8 steps: 3 more than were handed out)
    rc_ahead = a._state["reset_count"].clone()
    a.sync()
    assert a._la["rewinds"] == 1
    _same(_snap(a), _snap(b), "after sync() at slot 5 of 8")
    if kind == "set":
        # the rewind had something to restore: some env auto-reset in the three steps thrown away
        assert int((rc_ahead - a._state["reset_count"]).sum()) > 0
        assert bool((ahead != a.env_map).any())          # ... and drew another map: a rewind without the restore fails here
        assert a.env_map is a._env_map
    for t in range(11):
        slot("after the rewind, step %d" % t)
    _same(_snap(a), _snap(b), "at the end")
    assert hits[0] > 0 and int(b.state["reset_count"].sum()) > 0
    if kind == "set":
        assert len(set(a.env_map.cpu().numpy().tolist())) >= 2
    a.check_faults()


def _owned(flags):
    """the bits of a flag word the step kernels decide (CA_PLAN_VALID is the pipelined policy query's, not an ending)"""
    return flags & _mods()[0].KERNEL_FLAG_BITS


def _episodes_np(sim):
    ep = sim.episodes()
    ep["flags"] = _owned(ep["flags"])
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in ep.items()}


@pytest.mark.parametrize("pipeline", [True, False])
def test_records_on_top_of_a_set(pipeline):
    """the episode log with its `map` column and the final record, in a fused rollout and in a ring, against single steps"""
    N, E, M = 10, 40, 3
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    sims = [_build(N, E, pipeline, "set", table) for _ in range(3)]
    roll, ring, b = sims
    for s in sims:
        s.log_episodes(capacity=64)
        s.keep_final()
    ring.enable_lookahead(8)
    latest_obs = torch.zeros_like(b.final_obs)
    latest_flags = torch.zeros_like(b.final_flags)
    ended = torch.zeros((E,), dtype=torch.bool, device=b.device)
    truth = {}
    for n in (9, 15):
        ended[:] = False
        for t in range(n):
            before, rc = b.env_map.cpu().numpy().copy(), b.state["reset_count"].cpu().numpy().copy()
            b.step()
            over = b.game_over.bool()
            for e in np.nonzero(over.cpu().numpy())[0]:
                truth[(int(e), int(rc[e]))] = int(before[e])       # the map env e held while its episode rc[e] ran
            latest_obs = torch.where(over[:, None, None], b.final_obs, latest_obs)
            latest_flags = torch.where(over[:, None], b.final_flags, latest_flags)
            ended |= over
            obs, rew, done, g_over = ring.step_lookahead()
            fo, ff = ring.lookahead_final()
            assert torch.equal(obs, b.obs) and torch.equal(g_over, over)
            assert torch.equal(fo[over], b.final_obs[over]) and torch.equal(_owned(ff[over]), _owned(b.final_flags[over]))
        roll.rollout(n)
        assert _last_kernel().startswith("ca_pipe_kernel<10, 4, true>" if pipeline else "ca_kernel<256,") and " set" in _last_kernel()
        # after rollout(n) the record holds every env's most recent ending of the n steps
        assert bool(ended.any())
        assert torch.equal(roll.final_obs[ended], latest_obs[ended]) and torch.equal(_owned(roll.final_flags[ended]), _owned(latest_flags[ended]))
        assert torch.equal(roll.env_map, b.env_map)
    ring.sync()
    assert torch.equal(ring.env_map, b.env_map)
    want = _episodes_np(b)
    assert want["dropped"] == 0 and len(want["env"]) > 0 and "map" in want
    assert want["map"].dtype == np.int64 and len(set(want["map"].tolist())) >= 2
    assert [truth[(int(e), int(k))] for e, k in zip(want["env"], want["episode"])] == want["map"].tolist()
    assert (want["episode"] > 0).any()          # some episode ran on a map drawn on the device
    for s, what in ((roll, "rollout"), (ring, "ring")):
        got = _episodes_np(s)
        assert sorted(got) == sorted(want)
        for k in want:
            assert np.array_equal(got[k], want[k]), "%s: %s" % (what, k)
    # a key replaced after the fact: the draws of the logged episodes cannot be recomputed -- unknown, never a wrong index
    b.step()
    b.set_map_seed(b.map_seed ^ 0x55)
    for _ in range(12):
        b.step()
    late = _episodes_np(b)
    assert len(late["env"]) > 0
    old = late["map"][late["episode"] > 0]
    assert len(old) and ((old == -1) | (old >= 0)).all() and (old == -1).any()


def _laser_env(Env, E, grids, per_env):
    env = Env(num_envs=E)
    env.set_fixture_suite(4, policies="RVO", table=_cases(3 * E + 1, 4, 104, near=1.0))
    env.set_static_map(list(grids) if per_env else grids[0], per_env=per_env)
    return env


@pytest.mark.parametrize("per_env", [False, True])
def test_env_rollout_and_on_demand_sensing(per_env):
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        E, grids = 12, _maps(3, 31)
        envs = [_laser_env(Env, E, grids, per_env) for _ in range(3)]
        roll, lazy, b = envs
        lazy.sense_map_on_demand()
        for env in envs:
            np.random.seed(23)      # (the per-env map draws and the device key come from numpy's stream: the same for all three)
            env.reset()
            env._sim.p.reward_collision_wall = WALL
            env._sim.p.reward_min = min(env._sim.p.reward_min, WALL)
        assert not b._la_on and not roll._la_on and lazy._la_on          # the ring: only with the opt-in
        assert torch.equal(roll._sim.env_map, b._sim.env_map) if per_env else roll._sim.env_map is None
        hits = resets = 0
        for n in (1, 6, 17):
            for t in range(n):
                obs, rew, over, _, info = b.step(None)
                hits += int((rew == WALL).sum())
                resets += int(over.sum())
                o2, r2, over2, _, info2 = lazy.step(None)
                assert torch.equal(o2, obs) and torch.equal(r2, rew) and torch.equal(over2, over)
                assert torch.equal(info2["which_agents_done"], info["which_agents_done"])
            o1, r1, over1, _, info1 = roll.rollout(n)
            assert (" set" if (per_env and n > 1) else " map") in _last_kernel()
            assert torch.equal(o1, obs) and torch.equal(r1, rew) and torch.equal(over1, over)
            assert torch.equal(info1["which_agents_done"], info["which_agents_done"])
            # the newest scan row is the scan of the state: the same after one rollout as after n scanned steps
            assert torch.equal(roll.laserscan[:, :, 0], b.laserscan[:, :, 0])
            scan = lazy.laserscan      # computed now, on the step last handed out (rewinds the ring)
            assert torch.equal(scan[:, :, 0], b.laserscan[:, :, 0])
            assert lazy.laserscan is scan and not lazy._map_stale
        assert lazy._sim._la["fills"] > 0 and hits > 0 and resets > 0
        if per_env:
            assert torch.equal(roll.map_index, b.map_index) and torch.equal(lazy.map_index, b.map_index)
        lazy.sense_map_on_demand(False)
        assert not lazy._la_on and lazy._sim._la is None
        lazy.step(None)
        b.step(None)
        assert torch.equal(lazy.laserscan[:, :, 0], b.laserscan[:, :, 0])
        # switched on after reset(): the ring comes back with the length the byte budget gives NOW (the final record on)
        lazy.keep_final_observations()
        lazy.sense_map_on_demand()
        assert lazy._la_on and lazy._sim._la["n"] == lazy._ring_len(lazy._sim)
        for t in range(10):
            obs, rew, over = b.step(None)[:3]
            o2, r2, over2 = lazy.step(None)[:3]
            assert torch.equal(o2, obs) and torch.equal(r2, rew) and torch.equal(over2, over)
            if per_env and t in (2, 7):      # mid-ring: the maps of the step last handed out, not those drawn ahead
                assert torch.equal(lazy.map_index, b.map_index)
        assert torch.equal(lazy.laserscan[:, :, 0], b.laserscan[:, :, 0])
    finally:
        envtools.default()


SUITE_COLUMNS = ("num_agents", "policy", "test_case", "total_reward", "steps", "time_to_goal", "total_time_to_goal",
                 "extra_time_to_goal", "collision", "all_at_goal", "any_stuck", "outcome")


def test_run_suite_logged_on_a_map_batch():
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        import importlib
        rs = importlib.import_module("gym_collision_avoidance_amd.experiments.run_full_test_suite")
        grid = np.zeros((160, 160), bool)
        grid[:, 78:82] = True           # a wall along x = 0: the suite's crossing cases run into it
        a = rs.run_suite_logged("RVO", 4, range(16), static_map=grid, chunk=64)
        assert " map" in _last_kernel()
        b, free = rs.run_suite("RVO", 4, range(16), static_map=grid), rs.run_suite("RVO", 4, range(16))
        assert tuple(a.columns) == tuple(b.columns) == SUITE_COLUMNS and len(a) == len(b) == 16
        for col in SUITE_COLUMNS:
            x, y = a[col].tolist(), b[col].tolist()
            if col in ("total_reward", "time_to_goal", "extra_time_to_goal"):
                x, y = np.stack(x), np.stack(y)
            assert np.array_equal(np.asarray(x), np.asarray(y)), col
        assert b["collision"].sum() > free["collision"].sum()       # the walls decided episodes
    finally:
        envtools.default()


def test_nothing_moved_without_a_map():
    nat, core, _ = _mods()
    N, E = 10, 40
    table = _cases(3 * E + 1, N, 100 + N, near=1.0)
    for pipeline in (True, False):
        a, b = _build(N, E, pipeline, None, table), _build(N, E, pipeline, None, table)
        names = []
        a.step(); b.step()
        names.append(_last_kernel())
        a.rollout(9)
        names.append(_last_kernel())
        for _ in range(9):
            b.step()
        _same(_snap(a), _snap(b), "map-less rollout")
        a.enable_lookahead(8)
        for t in range(8):
            obs, rew, done, over = a.step_lookahead()
            if t == 0:
                names.append(_last_kernel())
            b.step()
            assert torch.equal(obs, b.obs) and torch.equal(rew, b.rewards) and torch.equal(over, b.game_over.bool())
        a.sync()
        _same(_snap(a), _snap(b), "map-less ring")
        for k in names:
            assert " map" not in k and " set" not in k, k
            assert re.search(r"(tile_envs=\d+|mode=\d+( fair)?)$", k), k      # the strings end where they always ended
        assert names[1].startswith("ca_pipe_kernel<10, 4, true>" if pipeline else "ca_kernel<256, ")
        assert int(b.state["reset_count"].sum()) > 0
