"""OccupancyGridSensor on the GPU (include/cagpu.h cagpu_occupancy_grid / _maps, csrc/cagpu_occ.inc).  Every comparison is
BIT-EXACT: the output is boolean and the index arithmetic is float64 with true divisions, so there is no tolerance to
choose.  Ground truth: windows recorded from the unmodified reference (tests/golden/occgrid.npz) and the numpy restatement
tests/occupancy_ref.py, which tests/test_occupancy_golden.py pins to those recordings."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import envtools
from tests import occupancy_ref as oref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "occgrid.npz")
OCC_CONFIGS = os.path.join(REPO, "tests", "occupancy_configs.py")


def _mods():
    from gym_collision_avoidance_amd import _native as nat
    from gym_collision_avoidance_amd import core
    return nat, core


def _unpack(bits, width):
    return np.unpackbits(bits, axis=-1, bitorder="little")[..., :width].astype(bool)


def _sim(E, N, pipeline=False, **kw):
    _, core = _mods()
    kw.setdefault("max_obs", min(N - 1, 9))
    return core.BatchedSim(core.make_params(E, N, **kw), pipeline=pipeline)


def _cases(px, py, radius):
    """[E, N] positions / radii -> case rows whose goals are the starts (nobody needs to move here)"""
    c = np.zeros(px.shape + (6,))
    c[..., 0], c[..., 1], c[..., 2], c[..., 3], c[..., 4], c[..., 5] = px, py, px, py, 1.0, radius
    return c


def _state(sim):
    st = sim.state
    return [st[n].cpu().numpy() for n in ("pos_x", "pos_y", "radius")]


def _want(sim, static, **kw):
    px, py, rad = _state(sim)
    env_map = None if sim.env_map is None else sim.env_map.cpu().numpy()
    return oref.occupancy_batch(static, px, py, rad, env_map=env_map, **kw)


def _maps(M, seed, rows=160, cols=160):
    rng = np.random.default_rng(seed)
    out = np.zeros((M, rows, cols), bool)
    for m in range(M):
        out[m] = rng.random((rows, cols)) < 0.01
        r0 = (rows // 5) + (rows // 2) * m // max(M, 1)
        out[m, r0:r0 + 4, cols // 16 + 7 * m:cols - cols // 16 - 5 * m] = True
        out[m, rows // 8:rows - rows // 8, cols // 4 + 25 * m:cols // 4 + 3 + 25 * m] = True
        out[m, 0, :] = out[m, -1, :] = out[m, :, 0] = out[m, :, -1] = True      # the outermost cells: the crop's edges
    return out


def _scene(E, N, seed, ragged=False, half_x=11.0, half_y=11.0):
    """positions uniform over the map and 3 m beyond it (windows inside, partly outside, wholly outside), a third of them
    on the 0.1 / 0.05 m lattice, radii 0.2 .. 1.5; ragged: the last slots of some envs are empty (radius 0)"""
    rng = np.random.default_rng(seed)
    px, py = rng.uniform(-half_x, half_x, (E, N)), rng.uniform(-half_y, half_y, (E, N))
    lat = rng.random((E, N)) < 1 / 3
    step = np.where(rng.random((E, N)) < 0.5, 0.1, 0.05)
    px = np.where(lat, np.round(np.round(px / step) * step, 2), px)
    py = np.where(lat, np.round(np.round(py / step) * step, 2), py)
    px[0, 0], py[0, 0] = -10.4, 2.8
    if N > 1:
        px[0, 1], py[0, 1] = -8.8, 8.8                       # where the reference's sensor raises
    rad = rng.uniform(0.2, 1.5, (E, N))
    if ragged:
        count = rng.integers(1, N + 1, E)
        count[0] = N
        rad[np.arange(N)[None, :] >= count[:, None]] = 0.0
    return px, py, rad


# ---------------------------------------------------------------------------------------------- 1. the reference's windows
def test_golden_episode_and_scenes_equal_the_reference():
    g = np.load(GOLD)
    static = _unpack(g["ep_static"], 160)
    state, want, valid = g["ep_state"], _unpack(g["ep_windows"], 50), g["ep_valid"]
    sim = _sim(1, 4)
    sim.set_map(static)
    sim.set_occupancy_grid()
    sim.reset(_cases(state[:1, :, 0], state[:1, :, 1], state[:1, :, 2]))
    checked = 0
    for t in range(len(state)):          # the reference's state of step t, re-injected
        st = sim.state
        for k, n in enumerate(("pos_x", "pos_y", "radius")):
            st[n].copy_(torch.from_numpy(state[t:t + 1, :, k].copy()))
        got = sim.occupancy_grid()
        assert got.dtype == torch.bool and tuple(got.shape) == (1, 4, 50, 50)
        got = got.cpu().numpy()
        for a in range(4):
            if valid[t, a]:
                assert np.array_equal(got[0, a], want[t, a]), "episode step %d agent %d" % (t, a)
                checked += 1
    assert checked >= 0.98 * valid.size
    # the single-shot scenes in one batch: scene s on grid s % 5 -- a map set
    grids = _unpack(g["sc_grids"], 160)
    state, want, valid = g["sc_state"], _unpack(g["sc_windows"], 50), g["sc_valid"]
    S, A = state.shape[:2]
    sim = _sim(S, A)
    sim.set_map(grids, env_map=np.arange(S) % len(grids))
    sim.set_occupancy_grid()
    sim.reset(_cases(state[..., 0], state[..., 1], state[..., 2]))
    got = sim.occupancy_grid().cpu().numpy()
    ok = valid.astype(bool)
    assert ok.mean() >= 0.98 and np.array_equal(got[ok], want[ok])
    # ... and the lattice positions the reference answers at all
    lat, lat_valid, lat_want = g["lat_xy"], g["lat_valid"], _unpack(g["lat_windows"], 50)
    sim = _sim(len(lat), 2)                                  # (slot 1: a bystander far outside the map)
    sim.set_map(None)
    sim.set_occupancy_grid()
    far = np.full((len(lat), 1), 30.0)
    sim.reset(_cases(np.hstack([lat[:, :1], far]), np.hstack([lat[:, 1:], far]), np.full((len(lat), 2), 0.5)))
    got = sim.occupancy_grid().cpu().numpy()[:, 0]
    assert np.array_equal(got, _want(sim, np.zeros((160, 160), bool))[:, 0])
    for k in np.nonzero(lat_valid)[0]:
        assert np.array_equal(got[k], lat_want[k])


# ---------------------------------------------------------------------------------------------- 2. random scenes
GEOMETRIES = [(4, 40), (10, 40), (50, 12), (70, 6), (300, 3)]     # test_gpu_map_sets.KERNELS' shapes + one above 256 agents


@pytest.mark.parametrize("N,E", GEOMETRIES)
@pytest.mark.parametrize("ragged", [False, True])
def test_random_scenes_equal_the_restatement(N, E, ragged):
    static = _maps(1, N)[0]
    px, py, rad = _scene(E, N, 10 * N + ragged, ragged=ragged)
    sim = _sim(E, N, ragged=int(ragged))
    sim.set_map(static)
    sim.set_occupancy_grid()
    sim.reset(_cases(px, py, rad))
    got = sim.occupancy_grid().cpu().numpy()
    spx, spy, srad = _state(sim)
    live = rad > 0                                            # (a reset leaves the empty slots at the origin, radius 0)
    assert np.array_equal(spx[live], px[live]) and np.array_equal(spy[live], py[live]) and np.array_equal(srad, rad)
    assert bool((srad == 0).any()) == ragged
    want = _want(sim, static)
    assert got.shape == (E, N, 50, 50) and np.array_equal(got, want)
    far = np.maximum(np.abs(spx), np.abs(spy))
    assert (far < 5.5).any() and (far > 10.5).any() and want.any() and not want.all()
    assert not want[far > 10.6].any()                         # wholly outside the map: zeros


@pytest.mark.parametrize("N,E", [(4, 40), (50, 12)])
def test_non_square_window(N, E):
    static = _maps(1, 3)[0]
    px, py, rad = _scene(E, N, 77 + N)
    sim = _sim(E, N)
    sim.set_map(static)
    sim.set_occupancy_grid(x_width=3, y_width=6.4)
    sim.reset(_cases(px, py, rad))
    got = sim.occupancy_grid().cpu().numpy()
    assert got.shape == (E, N, 64, 30)
    assert np.array_equal(got, _want(sim, static, x_width=3, y_width=6.4))


@pytest.mark.parametrize("N,E", [(10, 40), (70, 6)])
def test_non_default_map(N, E):
    rows, cols = 96, 200                                        # 9.6 m x 20 m: 7 words per row, the last one partial
    static = _maps(1, 5, rows, cols)[0]
    px, py, rad = _scene(E, N, 99 + N, half_x=13.0, half_y=8.0)
    sim = _sim(E, N)
    sim.set_map(static, rows=rows, cols=cols)
    sim.set_occupancy_grid()
    sim.reset(_cases(px, py, rad))
    got = sim.occupancy_grid().cpu().numpy()
    want = _want(sim, static)
    assert np.array_equal(got, want) and want.any()
    sim.set_map(static, rows=rows, cols=cols)                   # set_map() again drops the buffers
    assert sim.occ is None and sim.occ_bits is None
    with pytest.raises(AssertionError):
        sim.occupancy_grid()


def test_small_windows_and_odd_sizes():
    """windows narrower than a 16-byte chunk and sizes that leave an env's block unaligned (N H W odd): the byte-wise ends"""
    static = _maps(1, 8)[0]
    for (N, E, xw, yw) in [(3, 9, 0.5, 0.7), (2, 17, 0.1, 0.1), (5, 7, 1.7, 0.3), (7, 5, 25.6, 0.9)]:
        px, py, rad = _scene(E, N, int(10 * xw) + N, half_x=9.0, half_y=9.0)
        sim = _sim(E, N)
        sim.set_map(static)
        sim.set_occupancy_grid(x_width=xw, y_width=yw, packed="both")
        sim.reset(_cases(px, py, rad))
        got = sim.occupancy_grid().cpu().numpy()
        want = _want(sim, static, x_width=xw, y_width=yw)
        assert got.shape == want.shape == (E, N, int(yw / 0.1), int(xw / 0.1))
        assert np.array_equal(got, want), (N, E, xw, yw)
        assert np.array_equal(sim.occ_bits.cpu().numpy().view(np.uint32), oref.pack_rows(want)), (N, E, xw, yw)


# ---------------------------------------------------------------------------------------------- 3. the two formats
@pytest.mark.parametrize("N,E", [(10, 40), (300, 3)])
def test_bits_equal_packed_cells(N, E):
    static = _maps(1, 2)[0]
    px, py, rad = _scene(E, N, 5 + N)
    sims = {}
    for packed in (False, True, "both"):
        sim = _sim(E, N)
        sim.set_map(static)
        sim.set_occupancy_grid(packed=packed)
        sim.reset(_cases(px, py, rad))
        ret = sim.occupancy_grid()
        assert ret is (sim.occ_bits if packed is True else sim.occ)
        sims[packed] = sim
    assert sims[False].occ_bits is None and sims[True].occ is None
    cells = sims["both"].occ.cpu().numpy()
    bits = sims["both"].occ_bits.cpu().numpy().view(np.uint32)
    assert bits.shape == (E, N, 50, 2)
    pad = np.zeros((E, N, 50, 64), np.uint8)
    pad[..., :50] = cells
    assert np.array_equal(bits, np.packbits(pad, axis=-1, bitorder="little").view(np.uint32))
    assert np.array_equal(cells, _want(sims["both"], static))
    assert np.array_equal(sims[False].occ.cpu().numpy(), cells)             # cells only
    assert np.array_equal(sims[True].occ_bits.cpu().numpy().view(np.uint32), bits)   # bits only
    assert sims["both"]._occ_cells.max().item() == 1                        # 0 / 1 bytes behind the bool view


# ---------------------------------------------------------------------------------------------- 4. map sets
def _table(C, N, seed, near=1.0, side=7.0):
    rng = np.random.default_rng(seed)
    c = np.zeros((C, N, 6))
    c[..., 0:2] = rng.uniform(-side, side, (C, N, 2))
    c[..., 2:4] = c[..., 0:2] + rng.uniform(-near, near, (C, N, 2))
    c[..., 4] = rng.uniform(0.5, 2.0, (C, N))
    c[..., 5] = rng.uniform(0.2, 0.5, (C, N))
    return c


def test_set_of_one_equals_the_single_map_call():
    N, E = 10, 40
    grid = _maps(1, 6)[0]
    px, py, rad = _scene(E, N, 61)
    one, set1 = _sim(E, N), _sim(E, N)
    one.set_map(grid)
    set1.set_map(grid[None], env_map=np.zeros(E, np.int64))
    for s in (one, set1):
        s.set_occupancy_grid(packed="both")
        s.reset(_cases(px, py, rad))
        s.occupancy_grid()
    assert set1.num_maps == 1
    assert torch.equal(one.occ, set1.occ) and torch.equal(one.occ_bits, set1.occ_bits) and one.occ.any()


@pytest.mark.parametrize("N,E", [(10, 40), (70, 6)])
def test_map_set_equals_separate_single_map_sims(N, E):
    M = 4 if E % 4 == 0 else 3
    B = E // M
    grids = _maps(M, 7 + N)
    px, py, rad = _scene(E, N, 71 + N)
    big = _sim(E, N)
    big.set_map(grids, env_map=np.arange(E) // B)
    big.set_occupancy_grid()
    big.reset(_cases(px, py, rad))
    got = big.occupancy_grid()
    for m in range(M):
        part = slice(m * B, (m + 1) * B)
        s = _sim(B, N)
        s.set_map(grids[m])
        s.set_occupancy_grid()
        s.reset(_cases(px[part], py[part], rad[part]))
        assert torch.equal(s.occupancy_grid(), got[part]), "map %d" % m
    assert np.array_equal(got.cpu().numpy(), _want(big, grids))


def test_window_shows_the_new_map_after_auto_resets():
    N, E, M = 4, 40, 5
    grids = _maps(M, 3)
    sim = _sim(E, N, max_time_ratio=0.6)
    sim.set_map(grids, map_seed=12345)
    sim.set_occupancy_grid()
    sim.set_fixture_table(_table(E + 5, N, 300, near=1.0))
    sim.reset_from_table()
    first = sim.env_map.cpu().numpy().copy()
    changed = False
    for t in range(60):
        sim.step()
        got = sim.occupancy_grid().cpu().numpy()
        now = sim.env_map.cpu().numpy()
        assert np.array_equal(got, _want(sim, grids)), "step %d" % t      # (_want reads the env's CURRENT map index)
        changed |= bool((now != first).any())
    assert changed and int(sim.state["reset_count"].max()) >= 2
    # the windows of envs that changed maps differ from what their first map would show
    moved = np.nonzero(now != first)[0]
    px, py, rad = _state(sim)
    old = oref.occupancy_batch(grids, px[moved], py[moved], rad[moved], env_map=first[moved])
    assert not np.array_equal(old, got[moved])


def test_out_of_range_index_gives_an_empty_static_part_and_fault_bit_2():
    """C ABI directly (the host path refuses such an index): a bits buffer of M + 1 grids whose grid M is fully occupied,
    num_maps = M, and index M written into env 0 -- that env's windows must show its agents on an EMPTY map, and
    check_faults() must name bit 2.  A flag in device memory: no GPU fault is involved."""
    nat, core = _mods()
    N, E, M = 4, 8, 2
    grids = np.zeros((M + 1, 160, 160), bool)
    grids[:M] = _maps(M, 41)
    grids[M] = True
    px, py, rad = _scene(E, N, 43, half_x=6.0, half_y=6.0)
    bad = _sim(E, N)
    bad.set_map(grids)
    bad.set_occupancy_grid()
    bad.reset(_cases(px, py, rad))
    env_map = torch.tensor([M] + [e % M for e in range(1, E)], dtype=torch.int32, device=bad.device)
    ms = nat.CaMapSet(map=nat.CaMap.from_buffer_copy(bad._map), env_map=env_map.data_ptr(), num_maps=M, map_seed=0)
    ms.map.static_bits = bad._map_bits.data_ptr()
    bad.check_faults()
    torch.cuda.synchronize()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nat.check(nat.lib().cagpu_occupancy_grid_maps(ctypes.byref(bad.p), ctypes.byref(bad._cs), ctypes.byref(ms),
                                                  ctypes.byref(bad._occ), stream))
    torch.cuda.synchronize()
    got = bad.occ.cpu().numpy()
    want = oref.occupancy_batch(grids[:M], px, py, rad, env_map=env_map.cpu().numpy())
    assert np.array_equal(got, want)
    assert got[0].any() and np.array_equal(got[0], oref.occupancy(np.zeros((160, 160), bool), px[0], py[0], rad[0]))
    with pytest.raises(nat.CagpuError, match="bit 2"):
        bad.check_faults()
    assert nat.device_faults(clear=True) == 0          # check_faults cleared the word


# ---------------------------------------------------------------------------------------------- 5. full-size geometry
@pytest.mark.parametrize("N", [10, 50])
def test_full_size_batch_after_20_steps(N):
    E = 4096
    static = _maps(1, 9)[0]
    sim = _sim(E, N, pipeline=(N == 10))
    sim.set_map(static)
    sim.set_occupancy_grid(packed="both")
    sim.set_fixture_table(_table(600, N, 500 + N, near=6.0))
    sim.reset_from_table()
    for _ in range(20):
        sim.step()
    sim.occupancy_grid()
    envs = np.random.default_rng(N).choice(E, 64, replace=False)
    envs[:2] = (0, E - 1)
    px, py, rad = [a[envs] for a in _state(sim)]
    want = oref.occupancy_batch(static, px, py, rad)
    idx = torch.from_numpy(envs).to(sim.device)
    assert np.array_equal(sim.occ[idx].cpu().numpy(), want) and want.any()
    assert np.array_equal(sim.occ_bits[idx].cpu().numpy().view(np.uint32), oref.pack_rows(want))
    assert int(sim.occ.sum().item()) == int(torch.count_nonzero(sim._occ_cells).item())   # nothing but 0 / 1 anywhere


# ---------------------------------------------------------------------------------------------- 6. the env API
def _env_want(env, grid):
    st = env._sim.state
    return oref.occupancy_batch(grid, *[st[n].cpu().numpy() for n in ("pos_x", "pos_y", "radius")])


def _import_through_the_alias():
    """`gym_collision_avoidance.envs.sensors.OccupancyGridSensor`, the reference's module path, after install_as() -- in a
    child process (the alias is a process-wide import hook), which touches no device"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r)\n"
            "import gym_collision_avoidance_amd as pkg; pkg.install_as()\n"
            "from gym_collision_avoidance.envs.sensors.OccupancyGridSensor import OccupancyGridSensor as A\n"
            "from gym_collision_avoidance_amd.envs.sensors.OccupancyGridSensor import OccupancyGridSensor as B\n"
            "from gym_collision_avoidance.envs import test_cases as tc\n"
            "assert A is B and tc.sensor_dict['occupancy_grid'] is A and A().name == 'occupancy_grid'\n"
            "print('alias ok')\n" % REPO)
    env = dict(os.environ, GYM_CONFIG_PATH=os.path.join(REPO, "tests", "env_configs.py"), GYM_CONFIG_CLASS="Laser4")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "alias ok" in out.stdout, out.stderr[-2000:]


@pytest.mark.parametrize("with_laser", [False, True])
def test_env_api_single_env(with_laser):
    Config, tc, Env = envtools.fresh("OccLaser4" if with_laser else "Occ4", OCC_CONFIGS)
    try:
        from gym_collision_avoidance_amd.envs.agent import Agent
        from gym_collision_avoidance_amd.envs.dynamics.UnicycleDynamics import UnicycleDynamics
        from gym_collision_avoidance_amd.envs.sensors import LaserScanSensor, OccupancyGridSensor, OtherAgentsStatesSensor
        if with_laser:
            _import_through_the_alias()
        sensors = [OtherAgentsStatesSensor, OccupancyGridSensor] + ([LaserScanSensor] if with_laser else [])
        grid = _maps(1, 12)[0]
        grid[70:90, 70:90] = False
        starts = [(-3.03, 0.41, 3.2, 0.3), (3.11, -0.37, -3.0, 0.2), (0.23, 5.87, 0.1, -5.5), (6.93, 6.41, -2.0, -1.0)]
        agents = [Agent(px, py, gx, gy, 0.3 + 0.05 * i, 1.0, None, tc.policy_dict["RVO"], UnicycleDynamics, sensors, i)
                  for i, (px, py, gx, gy) in enumerate(starts)]
        env = Env()
        env.set_static_map(grid)
        env.set_agents(agents)
        obs, _ = env.reset()

        def check(obs, what):
            want = _env_want(env, grid)[0]
            assert tuple(env.occupancy_grid.shape) == (1, 4, 50, 50) and env.occupancy_grid.dtype == torch.bool
            assert np.array_equal(env.occupancy_grid.cpu().numpy()[0], want), what
            for i, a in enumerate(env.agents):
                assert obs[i]["occupancy_grid"].shape == (50, 50) and obs[i]["occupancy_grid"].dtype == bool
                assert np.array_equal(obs[i]["occupancy_grid"], want[i]), what
                assert np.array_equal(a.get_sensor_data("occupancy_grid"), want[i]), what
                assert np.array_equal(a.sensors[1].sense(env.agents, i, env.map), want[i]), what
                assert np.array_equal(a.get_observation_dict(env.agents)["occupancy_grid"], want[i]), what
            assert want.any()
            if with_laser:
                assert obs[0]["laserscan"].shape == (3, 512)

        check(obs, "reset")
        for t in range(12):
            obs, _, _, _, _ = env.step({})
            check(obs, "step %d" % t)
        obs, _, _, _, _ = env.rollout(5)
        check(obs, "rollout")
        # agents that disagree about the window: one tensor cannot hold both
        agents[1].sensors[1].set_args({"x_width": 3})
        env.set_agents(agents)
        with pytest.raises(ValueError, match="x_width"):
            env.reset()
        # without the sensor the env has no window tensor
        plain = [Agent(px, py, gx, gy, 0.3, 1.0, None, tc.policy_dict["RVO"], UnicycleDynamics,
                       [OtherAgentsStatesSensor, LaserScanSensor], i) for i, (px, py, gx, gy) in enumerate(starts)]
        env.set_agents(plain)
        with pytest.raises(RuntimeError, match="occupancy_grid"):   # ... which this Config's STATES_IN_OBS asks for
            env.reset()
        assert env.occupancy_grid is None
    finally:
        envtools.default()


@pytest.mark.parametrize("with_laser", [False, True])
def test_env_api_batched_with_auto_reset(with_laser):
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        E = 64
        grid = _maps(1, 13)[0]
        env = Env(num_envs=E)
        env.set_fixture_suite(4, policies="RVO", table=_table(200, 4, 21, near=1.5), agents_sensors=(
            ("other_agents_states", "occupancy_grid") + (("laserscan",) if with_laser else ())))
        env.set_static_map(grid)
        env.reset()
        assert [s.name for s in env.agents[0].sensors][:2] == ["other_agents_states", "occupancy_grid"]

        def check(what):
            occ = env.occupancy_grid
            assert tuple(occ.shape) == (E, 4, 50, 50) and occ.dtype == torch.bool
            assert np.array_equal(occ.cpu().numpy(), _env_want(env, grid)), what

        check("reset")
        for t in range(40):
            env.step(None)
            check("step %d" % t)
        assert int(env._sim.state["reset_count"].sum()) > 0          # auto-resets happened on the way
        env.rollout(7)
        check("rollout")
        assert np.array_equal(env.agents[0].get_sensor_data("occupancy_grid"), env.occupancy_grid[0, 0].cpu().numpy())
    finally:
        envtools.default()


# ---------------------------------------------------------------------------------------------- 7. nothing else moves
def test_a_run_with_the_sensor_equals_the_run_without_it():
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        E = 32
        grid = _maps(1, 14)[0]
        runs = []
        for sensors in (("other_agents_states", "laserscan"), ("other_agents_states", "laserscan", "occupancy_grid")):
            np.random.seed(5)
            env = Env(num_envs=E)
            env.set_fixture_suite(4, policies="RVO", table=_table(100, 4, 22, near=1.5), agents_sensors=sensors)
            env.set_static_map(grid)
            trace = [env.reset()[0].cpu().numpy().copy()]
            for t in range(30):
                obs, rew, over, _, info = env.step(None)
                trace += [obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), over.cpu().numpy().copy(),
                          info["which_agents_done"].cpu().numpy().copy(), env.laserscan.cpu().numpy().copy()]
            st = env._sim.state
            trace += [st[n].cpu().numpy().copy() for n in sorted(st) if n != "next_action"]
            trace.append(env._sim.scan_hist.cpu().numpy().copy())
            runs.append((env, trace))
        (plain, a), (sensed, b) = runs
        assert plain.occupancy_grid is None and sensed.occupancy_grid is not None
        assert len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
        assert int(sensed._sim.state["reset_count"].sum()) > 0
    finally:
        envtools.default()
