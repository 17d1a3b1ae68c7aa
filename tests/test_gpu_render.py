"""Frames rasterised on the device (include/cagpu.h CaRender, core.BatchedSim.render_frames / render_episode, the env's
render()): EVERY comparison is bit-exact -- np.array_equal on uint8 -- against tests/render_ref.py, the NumPy statement of
the drawing rules, fed with the simulator's own state and tape.  The expected episode of a frame is
found here from the tape's counters in plain Python, independently of render.episode_ranges."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import envtools  # noqa: E402
from tests import render_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (128, 128), (67, 93), (400, 500)]
STATE = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed", "time_remaining", "t",
         "slt", "ep_reward", "last_action", "flags", "step_num", "episode_step", "reset_count", "env_stats", "next_action")


def _mods():
    from gym_collision_avoidance_amd import _native as nat
    from gym_collision_avoidance_amd import core
    return nat, core


def _cases(C_, N, seed, side=5.0, near=2.5, ragged=False):
    rng = np.random.default_rng(seed)
    c = np.zeros((C_, N, 6))
    c[..., 0:2] = rng.uniform(-side, side, (C_, N, 2))
    c[..., 2:4] = c[..., 0:2] + rng.uniform(-near, near, (C_, N, 2))
    c[..., 4] = rng.uniform(0.5, 2.0, (C_, N))
    c[..., 5] = rng.uniform(0.2, 0.5, (C_, N))
    if ragged:
        for i in range(C_):
            c[i, int(rng.integers(2, N + 1)):] = 0.0
    return c


def _sim(E, N, seed=1, auto_reset=True, ragged=False, record=True, pipeline=True, **kw):
    nat, core = _mods()
    kw.setdefault("max_time_ratio", 1.5)
    kw.setdefault("max_obs", min(N - 1, 9))
    s = core.BatchedSim(core.make_params(E, N, ragged=int(ragged), **kw), pipeline=pipeline)
    s.set_plugins(nat.POL_RVO)
    table = _cases(3 * E + 1, N, seed, ragged=ragged, side=5.0 if N <= 10 else 7.5)
    if auto_reset:
        s.set_fixture_table(table)
        s.reset_from_table()
    else:
        s.reset(table[:E])
    if record:
        s.record_trajectories()
    return s


def _slots(key, cur, which):
    """slots of the env's current / last earlier episode, from its (epoch, episode) pairs along the tape"""
    mine = [t for t, k in enumerate(key) if k == cur]
    if which == "current":
        return mine
    others = [t for t, k in enumerate(key) if k != cur]
    return [t for t in others if key[t] == key[others[-1]]] if others else []


def _expect(sim, env_ids, size, limits=None, episode="current", upto=None, circles=True, draw_map=True, grids=None):
    """the frames render_frames must return, by tests/render_ref.py"""
    nat, _ = _mods()
    tape = {k: v.cpu().numpy() for k, v in sim.trajectories().items()}
    st = {n: sim.state[n].cpu().numpy() for n in ("pos_x", "pos_y", "goal_x", "goal_y", "radius", "flags", "reset_count")}
    epoch_now = np.zeros(sim.E, np.int64) if sim._traj is None else sim._traj["epoch"].cpu().numpy()
    env_map = None if sim.env_map is None else sim.env_map.cpu().numpy()
    out = []
    for e in env_ids:
        key = list(zip(tape["epoch"][:, e].tolist(), tape["episode"][:, e].tolist()))
        slots = _slots(key, (int(epoch_now[e]), int(st["reset_count"][e])), episode)
        if upto is not None:
            slots = slots[:upto + 1]
        grid = None
        if draw_map and grids is not None:
            grid = grids[env_map[e]] if grids.ndim == 3 else grids
        if not slots:
            agents = [None if st["flags"][e, a] & nat.ABSENT else
                      (st["pos_x"][e, a], st["pos_y"][e, a], st["goal_x"][e, a], st["goal_y"][e, a], st["radius"][e, a])
                      for a in range(sim.N)]
            out.append(R.render(size, limits, agents, circles, snapshot=True, grid=grid))
            continue
        agents = []
        for a in range(sim.N):
            r = tape["rows"][slots, e, a]
            r = r[r[:, 11] >= 0]
            agents.append(r if len(r) else None)
        out.append(R.render(size, limits, agents, circles, grid=grid))
    return np.stack(out)


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%s: %d of %d pixels differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])
    assert (want != 255).any(), "%s: an empty picture proves nothing" % what


# ---------------------------------------------------------------- history frames, both modes, every size
@pytest.mark.parametrize("N,size", [(2, SIZES[0]), (4, SIZES[2]), (10, SIZES[1]), (50, SIZES[0]), (10, SIZES[3]), (4, SIZES[3])])
@pytest.mark.parametrize("circles", [True, False])
def test_current_and_last_episode_after_auto_resets(N, size, circles):
    E = 6
    sim = _sim(E, N, seed=10 + N)
    for _ in range(45):
        sim.step()
    assert int(sim.state["reset_count"].sum()) > 0, "no env auto-reset: 'last' would be all snapshots"
    ids = list(range(E)) if size != SIZES[3] else [0, 3]
    for which in ("current", "last"):
        got = sim.render_frames(ids, size=size, episode=which, circles_along_traj=circles)
        _same(got, _expect(sim, ids, size, episode=which, circles=circles), "N=%d %s %s" % (N, size, which))


def test_ragged_batch_and_default_env_ids():
    sim = _sim(8, 6, seed=3, ragged=True)
    nat, _ = _mods()
    assert (sim.state["flags"] & nat.ABSENT).any()
    _same(sim.render_frames(size=(64, 64)), _expect(sim, range(8), (64, 64)), "ragged snapshot (no row yet)")
    for _ in range(30):
        sim.step()
    for which in ("current", "last"):
        _same(sim.render_frames(size=(67, 93), episode=which), _expect(sim, range(8), (67, 93), episode=which), "ragged " + which)


def test_recording_off_gives_snapshot_frames():
    sim = _sim(5, 10, seed=4, record=False)
    for _ in range(12):
        sim.step()
    for which in ("current", "last"):
        for circles in (True, False):
            _same(sim.render_frames(size=(128, 128), episode=which, circles_along_traj=circles),
                  _expect(sim, range(5), (128, 128), episode=which, circles=circles), "snapshot " + which)
    _same(sim.render_episode(2, size=(64, 64)), _expect(sim, [2], (64, 64), episode="last"), "render_episode without a tape")


def test_host_reset_ends_the_episode():
    sim = _sim(6, 4, seed=5, auto_reset=False)
    for _ in range(10):
        sim.step()
    mask = np.array([1, 0, 1, 0, 0, 1], np.uint8)
    sim.reset(_cases(6, 4, 77), mask=mask)
    _same(sim.render_frames(size=(64, 64)), _expect(sim, range(6), (64, 64)), "current right after a masked reset")
    _same(sim.render_frames(size=(64, 64), episode="last"), _expect(sim, range(6), (64, 64), episode="last"), "last after reset")
    for _ in range(7):
        sim.step()
    for which in ("current", "last"):
        _same(sim.render_frames(size=(64, 64), episode=which), _expect(sim, range(6), (64, 64), episode=which), "later " + which)


def test_upto_and_render_episode_are_the_prefix_frames():
    sim = _sim(4, 4, seed=6)
    for _ in range(40):
        sim.step()
    e = int(torch.argmax(sim.state["reset_count"]))
    assert int(sim.state["reset_count"][e]) > 0
    for which, every in (("last", 1), ("last", 4), ("current", 3)):
        anim = sim.render_episode(e, episode=which, every=every, size=(64, 64))
        from gym_collision_avoidance_amd import render as rd
        tape = sim.trajectories()
        key = list(zip(tape["epoch"][:, e].tolist(), tape["episode"][:, e].tolist()))
        L = len(_slots(key, (int(sim._traj["epoch"][e]), int(sim.state["reset_count"][e])), which))
        lasts = rd.prefix_lasts(L, every)
        assert anim.shape[0] == len(lasts) and lasts[-1] == L - 1 and L > 3
        for j, k in enumerate(lasts):
            single = sim.render_frames([e], size=(64, 64), episode=which, upto=k)
            assert torch.equal(anim[j], single[0]), (which, every, j)
            if j in (0, len(lasts) // 2, len(lasts) - 1):
                _same(single, _expect(sim, [e], (64, 64), episode=which, upto=k), "upto=%d" % k)
        assert not torch.equal(anim[0], anim[-1])


# ---------------------------------------------------------------- maps
def _grids(M, seed):
    rng = np.random.default_rng(seed)
    g = rng.random((M, 160, 160)) < 0.01
    for m in range(M):
        g[m, 30 + 20 * m:34 + 20 * m, 10:150 - 20 * m] = True
        g[m, 20:140, 40 + 25 * m:43 + 25 * m] = True
    g[0, 0, :] = g[0, -1, :] = g[0, :, 0] = g[0, :, -1] = True
    return g


@pytest.mark.parametrize("kind", ["none", "one", "set"])
def test_maps(kind):
    E, N = 12, 4
    sim = _sim(E, N, seed=8, record=False)
    grids = None
    if kind == "one":
        grids = _grids(1, 1)[0]
        sim.set_map(grids)
    elif kind == "set":
        grids = _grids(3, 2)
        sim.set_map(grids, map_seed=4242)
    sim.record_trajectories()
    before = None if sim.env_map is None else sim.env_map.clone()
    for _ in range(45):
        sim.step()
    if kind == "set":
        assert not torch.equal(before, sim.env_map), "no env drew another map"
        assert len(set(sim.env_map.tolist())) > 1
    for size, limits in (((128, 128), None), ((67, 93), ((-9.0, 3.0), (-2.0, 9.5)))):   # (the second window leaves the map)
        got = sim.render_frames(size=size, limits=limits)
        _same(got, _expect(sim, range(E), size, limits, grids=grids), "map %s %s" % (kind, size))
        if grids is not None:
            assert (got.cpu().numpy() == R.WALL).all(axis=-1).any()
            off = sim.render_frames(size=size, limits=limits, draw_map=False)
            _same(off, _expect(sim, range(E), size, limits, grids=grids, draw_map=False), "draw_map=False")


# ---------------------------------------------------------------- clipping
@pytest.mark.parametrize("limits", [((-1.0, 1.0), (-1.0, 1.0)), ((100.0, 101.0), (100.0, 101.0)), ((-0.1, 0.1), (-0.1, 0.1)),
                                    ((-30.0, 30.0), (-5.0, 5.0))])
def test_clipping(limits):
    sim = _sim(6, 10, seed=9)
    for _ in range(30):
        sim.step()
    # a window smaller than one agent, centred ON an agent's last position
    if limits[0] == (-0.1, 0.1):
        x, y = float(sim.state["pos_x"][0, 0]), float(sim.state["pos_y"][0, 0])
        limits = ((x - 0.1, x + 0.1), (y - 0.1, y + 0.1))
    for circles in (True, False):
        got = sim.render_frames(size=(67, 93), limits=limits, circles_along_traj=circles)
        want = _expect(sim, range(6), (67, 93), limits, circles=circles)
        got = got.cpu().numpy()
        assert np.array_equal(got, want), (limits, circles, int((got != want).sum()))
    if limits[0][0] == 100.0:
        assert (got == 255).all()


# ---------------------------------------------------------------- stepping paths
def test_after_rollout_and_in_the_middle_of_a_ring():
    sim = _sim(64, 10, seed=11)
    sim.rollout(25)
    _same(sim.render_frames([0, 5, 63], size=(64, 64)), _expect(sim, [0, 5, 63], (64, 64)), "after rollout")
    sim.enable_lookahead(16, adaptive=False)
    for _ in range(16 + 5):
        sim.step_lookahead()
    assert sim._la["t"] == 5 and sim._la["slots"] is not None
    got = sim.render_frames([1, 2, 40], size=(64, 64), episode="current")     # (rewinds to the step last handed out)
    assert sim._la["slots"] is None and sim._la["rewinds"] == 1
    assert sim.trajectories()["rows"].shape[0] == 25 + 21
    _same(got, _expect(sim, [1, 2, 40], (64, 64)), "mid-ring")
    _same(sim.render_frames([1, 2, 40], size=(64, 64), episode="last"), _expect(sim, [1, 2, 40], (64, 64), episode="last"), "mid-ring last")


def test_all_envs_without_a_gather_and_the_tape_window():
    """env_ids=None inside one chunk of the tape hands the launch a VIEW of the tape, and only the window of slots that
    some frame shows: the same frames as the gathered form, and as the spec"""
    E = 5
    sim = _sim(E, 4, seed=21)
    for _ in range(120):    # (goals at most 3.6 m away at 0.5 m/s or more, 1.5 x that time allowed: every first episode is over)
        sim.step()
    assert int(sim.state["reset_count"].min()) > 0, "an env still in its first episode: the window of 'current' would start at slot 0"
    ids = list(range(E))
    for kw in (dict(episode="current"), dict(episode="last"), dict(episode="last", upto=2)):
        got = sim.render_frames(size=(64, 64), **kw)
        assert torch.equal(got, sim.render_frames(ids, size=(64, 64), **kw)), kw
        _same(got, _expect(sim, ids, (64, 64), **kw), "all envs %s" % (kw,))


# ---------------------------------------------------------------- purity
def _everything(sim, mask_unspecified=False):
    sim.sync()      # (a ring that ran ahead is rewound first: the underscored tensors are then those of the step last handed out)
    d = {n: sim._state[n].clone() for n in STATE}
    d.update(obs=sim._obs.clone(), rewards=sim._rewards.clone(), done=sim._done.clone(), game_over=sim._game_over.clone())
    tape = sim.trajectories()
    if mask_unspecified:
        # two sims: columns 0 - 10 of a row that is none -- column 11 = -1 -- are whatever the tape's buffer held, and a ring
        # that was rewound wrote its buffer in another order than one that was not.  (One sim before / after a call:
        # every byte is compared.)
        tape["rows"] = torch.where(tape["rows"][..., 11:12] >= 0, tape["rows"], torch.full_like(tape["rows"], -1.0))
    d.update({"tape_" + k: v for k, v in tape.items()})
    return d


def test_render_writes_nothing_of_the_simulator():
    nat, _ = _mods()
    sim = _sim(32, 10, seed=12)
    for _ in range(20):
        sim.step()
    kernel = nat.lib().cagpu_last_kernel()
    before = _everything(sim)
    sim.render_frames(size=(64, 64))
    sim.render_frames(size=(64, 64), episode="last", circles_along_traj=False)
    sim.render_episode(3, size=(64, 64))
    assert nat.lib().cagpu_last_kernel() == kernel
    after = _everything(sim)
    for n in before:
        assert torch.equal(before[n].view(torch.uint8), after[n].view(torch.uint8)), n
    sim.step()
    assert nat.lib().cagpu_last_kernel() == kernel


def test_rendering_twin_stays_identical_over_a_ring_served_run():
    a, b = _sim(128, 10, seed=13), _sim(128, 10, seed=13)
    for s in (a, b):
        s.enable_lookahead(16)
    for t in range(70):
        oa, ob = a.step_lookahead(), b.step_lookahead()
        for x, y in zip(oa, ob):
            assert torch.equal(x, y), t
        if t % 7 == 3:
            a.render_frames([0, 9], size=(64, 64))
        if t % 20 == 11:
            a.render_episode(4, size=(64, 64))
    ea, eb = _everything(a, mask_unspecified=True), _everything(b, mask_unspecified=True)
    for n in ea:
        assert torch.equal(ea[n].view(torch.uint8), eb[n].view(torch.uint8)), n
    assert float(a.episode_stats()[0]) > 0


# ---------------------------------------------------------------- the C ABI directly
def _abi(sim, hist, frame_env, frame_col, first, last, size=(64, 64), limits=None, flags=1, over=None):
    nat, _ = _mods()
    from gym_collision_avoidance_amd import render as rd
    dev = sim.device
    H, W = size
    xmin, ymax, s16 = rd.window(size, limits)
    i32 = lambda v: torch.as_tensor(v, dtype=torch.int32, device=dev)
    F = len(frame_env)
    T = 0 if hist is None else hist.shape[0]
    keep = dict(out=torch.full((F, H, W, 3), 7, dtype=torch.uint8, device=dev), fe=i32(frame_env), fc=i32(frame_col), fi=i32(first),
                la=i32(last), work=torch.empty((int(nat.lib().cagpu_render_work_bytes(F, sim.N, T)),), dtype=torch.uint8, device=dev))
    r = nat.CaRender(out=keep["out"].data_ptr(), num_frames=F, height=H, width=W, flags=flags, xmin=xmin, ymax=ymax, s16=s16,
                     frame_env=keep["fe"].data_ptr(), frame_col=keep["fc"].data_ptr(), first=keep["fi"].data_ptr(),
                     last=keep["la"].data_ptr(), hist=None if hist is None else hist.data_ptr(), hist_steps=T,
                     hist_cols=0 if hist is None else hist.shape[1], stride_t=0 if hist is None else hist.stride(0),
                     stride_s=0 if hist is None else hist.stride(1), work=keep["work"].data_ptr(), work_bytes=keep["work"].numel())
    for k, v in (over or {}).items():
        setattr(r, k, (keep["out"].data_ptr() + 4) if v == "misaligned" else v)
    rc = nat.lib().cagpu_render(C.byref(sim.p), C.byref(sim._cs), None, C.byref(r), None)
    torch.cuda.synchronize()
    return rc, keep["out"]


def _synthetic(T, S, N, seed, holes=False):
    rng = np.random.default_rng(seed)
    h = np.zeros((T, S, N, 12))
    h[..., 0] = (0.1 * np.arange(T))[:, None, None]
    start = rng.uniform(-3, 3, (S, N, 2))
    vel = rng.uniform(-0.08, 0.08, (S, N, 2))
    wob = 0.15 * np.sin(0.3 * np.arange(T))[:, None, None]
    h[..., 1] = start[None, ..., 0] + vel[None, ..., 0] * np.arange(T)[:, None, None] + wob
    h[..., 2] = start[None, ..., 1] + vel[None, ..., 1] * np.arange(T)[:, None, None]
    h[..., 3:5] = rng.uniform(-4, 4, (S, N, 2))[None]
    h[..., 5] = rng.uniform(0.2, 0.5, (S, N))[None]
    n = rng.integers(1, T + 1, (S, N))                    # agent (s, a) moves in its first n slots
    valid = np.arange(T)[:, None, None] < n[None]
    if holes:
        valid &= rng.random((T, S, N)) < 0.8
    valid[:, 0, 0] = False                                # one agent without a row
    h[..., 11] = np.where(valid, np.cumsum(valid, axis=0) - 1, -1)
    h[~valid, :11] = np.nan                               # (unspecified columns of rows that are none)
    return h


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("N,T,size", [(10, 120, (64, 64)), (3, 40, (400, 500)), (130, 30, (128, 128))])
def test_synthetic_history_many_primitives_per_tile(N, T, size, holes):
    """a list far longer than the LDS holds (10 x 120 rows inside one 64 x 16 tile: several passes), rows with holes, NaN in
    the columns of rows that are none, one launch for frames of different ranges and columns"""
    sim = _sim(2, N, seed=14, auto_reset=False, record=False)
    S = 3
    h = _synthetic(T, S, N, 20 + N, holes)
    hist = torch.from_numpy(h).to(sim.device)
    frames = [(0, 0, 0, T - 1), (1, 1, 0, T - 1), (0, 2, T // 3, T // 2), (1, 0, 5, 5), (0, 1, 2, 1), (1, 2, -4, T + 9), (0, 7, 0, T - 1)]
    fe, fc, fi, la = zip(*frames)
    for flags in (1, 0):
        rc, out = _abi(sim, hist, fe, fc, fi, la, size=size, flags=flags)
        assert rc == 0
        st = {n: sim.state[n].cpu().numpy() for n in ("pos_x", "pos_y", "goal_x", "goal_y", "radius")}
        for j, (e, c, f0, l0) in enumerate(frames):
            if l0 < f0:
                agents = [(st["pos_x"][e, a], st["pos_y"][e, a], st["goal_x"][e, a], st["goal_y"][e, a], st["radius"][e, a]) for a in range(N)]
                want = R.render(size, None, agents, bool(flags), snapshot=True)
            elif c >= S:
                want = R.render(size, None, [None] * N, bool(flags))
            else:
                blk = h[max(f0, 0):min(l0, T - 1) + 1, c]
                agents = [blk[blk[:, a, 11] >= 0, a] for a in range(N)]
                want = R.render(size, None, [r if len(r) else None for r in agents], bool(flags))
            got = out[j].cpu().numpy()
            assert np.array_equal(got, want), (flags, j, int((got != want).any(axis=-1).sum()))


def test_argument_errors_launch_nothing():
    nat, _ = _mods()
    sim = _sim(2, 4, seed=15, auto_reset=False, record=False)
    hist = torch.from_numpy(_synthetic(8, 2, 4, 1)).to(sim.device)
    ok = dict(hist=hist, frame_env=[0, 1], frame_col=[0, 1], first=[0, 0], last=[7, 7])
    rc, out = _abi(sim, **ok)
    assert rc == 0 and not (out == 7).all()
    bad = [dict(out=None), dict(out="misaligned"), dict(num_frames=0), dict(height=15), dict(width=1025), dict(s16=0.0), dict(s16=float("nan")),
           dict(xmin=float("inf")), dict(frame_env=None), dict(first=None), dict(last=None), dict(hist=None), dict(hist_steps=-1),
           dict(hist_cols=0), dict(stride_t=-1), dict(work=None), dict(work_bytes=16)]
    for over in bad:
        rc, out = _abi(sim, over=over, **ok)
        assert rc == nat.CA_EINVAL, (over, rc)
        assert nat.lib().cagpu_last_error()
        assert (out == 7).all(), over                         # nothing launched: the output still holds its fill
    r = nat.CaRender()
    assert nat.lib().cagpu_render(None, C.byref(sim._cs), None, C.byref(r), None) == nat.CA_EINVAL
    assert nat.lib().cagpu_render_maps(C.byref(sim.p), C.byref(sim._cs), None, C.byref(r), None) == nat.CA_EINVAL
    assert nat.lib().cagpu_render_work_bytes(0, 4, 8) == 0


# ---------------------------------------------------------------- the env API
def test_env_render_and_save_episode_plots(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    # (an evaluation config of its own: under the default training config a batch without a learning agent ends every
    # episode after one step, and which config an earlier test module left behind is not this test's business)
    Config, tc, CollisionAvoidanceEnv = envtools.fresh("Swap4")
    env = CollisionAvoidanceEnv(num_envs=4)
    env.set_fixture_suite(4, "RVO")
    env.record_trajectories()
    env.reset()
    for _ in range(30):
        env.step(None)
    with pytest.raises(NotImplementedError, match="rgb_array"):
        env.render(mode="human")
    frames = env.render(size=(64, 64))
    assert frames.is_cuda and frames.shape == (4, 64, 64, 3) and frames.dtype == torch.uint8
    _same(frames, _expect(env._sim, range(4), (64, 64)), "env.render")
    assert torch.equal(env.render(env_ids=[2], size=(64, 64))[0], frames[2])
    env.set_plot_save_dir(str(tmp_path))
    env.plot_policy_name = "RVO"
    # the two envs whose running episode is the longest on the tape (an env may have auto-reset a step ago)
    sim = env._sim
    tape = sim.trajectories()
    length = [len(_slots(list(zip(tape["epoch"][:, e].tolist(), tape["episode"][:, e].tolist())),
                         (int(sim._traj["epoch"][e]), int(sim.state["reset_count"][e])), "current")) for e in range(4)]
    picks = sorted(sorted(range(4), key=lambda e: -length[e])[:2])
    assert min(length[e] for e in picks) > 3, length
    paths = env.save_episode_plots(picks, animate=True, size=(64, 64))
    assert [os.path.basename(p) for p in paths] == ["%03d_RVO_4agents.png" % e for e in picks]
    for p, e in zip(paths, picks):
        assert np.array_equal(np.asarray(PIL.open(p).convert("RGB")), frames[e].cpu().numpy())
        gif = PIL.open(os.path.join(str(tmp_path), "animations", os.path.basename(p)[:-4] + ".gif"))
        assert gif.n_frames > 2 and gif.size == (64, 64)
    anim = env.render_episode(picks[0], episode="current", size=(64, 64))
    assert anim.shape[0] == length[picks[0]] and torch.equal(anim[-1], frames[picks[0]])
    # a single env: the numpy frame Gym expects
    one = CollisionAvoidanceEnv()
    one.set_agents(tc.get_testcase_two_agents(policies=("RVO", "RVO")))
    one.reset()
    img = one.render(size=(128, 128))
    assert isinstance(img, np.ndarray) and img.shape == (128, 128, 3) and img.dtype == np.uint8 and (img != 255).any()


def test_save_episode_plots_copies_collided_episodes(tmp_path):
    """the reference's `collisions/` copy (visualize.py:138-149): written for an env some agent of which is in collision, and
    only for such an env"""
    PIL = pytest.importorskip("PIL.Image")
    nat, _ = _mods()
    Config, tc, CollisionAvoidanceEnv = envtools.fresh("Swap4")

    def run(policies, steps):
        env = CollisionAvoidanceEnv()
        env.set_agents(tc.get_testcase_two_agents(policies=policies))
        env.record_trajectories()
        env.reset()
        for _ in range(steps):
            if env.step({})[2]:
                break
        return env

    # two non-cooperative agents swapping corners drive straight into each other
    hit = run(("noncoop", "noncoop"), 120)
    assert (hit._sim.state["flags"].cpu().numpy() & nat.IN_COLLISION).any(), "the scene is meant to end in a collision"
    hit.set_plot_save_dir(str(tmp_path / "hit"))
    hit.test_case_index = 7
    (png,) = hit.save_episode_plots(size=(64, 64))
    assert os.path.basename(png) == "007_NonCooperativePolicy_2agents.png"
    copy = os.path.join(str(tmp_path), "hit", "collisions", "007_NonCooperativePolicy_2agents.png")
    frame = hit.render(size=(64, 64))
    _same(frame[None], _expect(hit._sim, [0], (64, 64)), "collided episode")
    for p in (png, copy):
        assert np.array_equal(np.asarray(PIL.open(p).convert("RGB")), frame), p
    # ... and two RVO agents pass each other: no copy
    free = run(("RVO", "RVO"), 30)
    assert not (free._sim.state["flags"].cpu().numpy() & nat.IN_COLLISION).any()
    free.save_episode_plots(directory=str(tmp_path / "free"), size=(64, 64))
    assert os.listdir(str(tmp_path / "free")) == ["000_RVO_2agents.png"]
