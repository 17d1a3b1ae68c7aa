"""The device trajectory tape (include/cagpu.h CaTraj; core.BatchedSim.record_trajectories): the step kernels write the
reference's Agent.global_state_history rows themselves.  The bar: a row of the tape IS the simulator's own state around
that step, bit for bit, in every kernel family, through every stepping path and across auto-resets; recording changes
nothing else; and free-running reference episodes give the reference's log at the bars test_golden_free_running holds.

"bit for bit" = torch.equal on float64.  The columns 0 - 10 of a row whose column 11 is -1 (the agent did not move) are
unspecified (the kernels leave them alone) and never compared."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import envtools  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests.test_gpu_parity import SORT, _golden_sim, _mods  # noqa: E402
from tests.test_trajectory_host import reference_histories  # noqa: E402

pytestmark = pytest.mark.gpu

POST = ("pos_x", "pos_y", "goal_x", "goal_y", "radius", "pref_speed", "vel_x", "vel_y", None, "heading")   # columns 1 - 10


def _last_kernel():
    return _mods()[0].lib().cagpu_last_kernel().decode()


def _fixture_sim(E, N, sort=0, auto_reset=False, pipeline=True, stride=None, **kw):
    nat, core, orc = _mods()
    table = gu.fixtures(N)
    s = core.BatchedSim(core.make_params(E, N, sort_mode=sort, **kw), pipeline=pipeline)
    s.set_plugins(nat.POL_RVO)
    if auto_reset:
        s.set_fixture_table(table, case_stride=stride)
        s.reset_from_table()
    else:
        s.reset(table[np.arange(E) % table.shape[0]])
    return s


class Shadow(object):
    """sim B of the comparison: one launch per step, no recording, its state read around every step"""

    def __init__(self, sim):
        self.sim, self.pre, self.post = sim, [], []

    def step(self, ext=None):
        st = self.sim.state
        self.pre.append({n: st[n].clone() for n in ("t", "step_num", "reset_count")})
        self.sim.step(ext)
        st = self.sim.state
        self.post.append({n: st[n].clone() for n in ("step_num", "last_action") + tuple(c for c in POST if c)})

    def check(self, tape, what):
        rows, episode = tape["rows"], tape["episode"]
        assert rows.shape[0] == len(self.pre) == episode.shape[0], (what, rows.shape, len(self.pre))
        n_moved = 0
        for s, (pre, post) in enumerate(zip(self.pre, self.post)):
            r = rows[s]
            moved = post["step_num"] > pre["step_num"]
            assert torch.equal(moved, r[..., 11] >= 0), "%s step %d: moved pattern" % (what, s)
            assert torch.equal(r[..., 11], torch.where(moved, pre["step_num"].double(), -1.0)), "%s step %d: index" % (what, s)
            assert torch.equal(r[..., 0][moved], pre["t"][moved]), "%s step %d: t" % (what, s)
            for c, name in enumerate(POST):
                want = post["last_action"][..., 0].double() if name is None else post[name]
                assert torch.equal(r[..., 1 + c][moved], want[moved]), "%s step %d: column %d" % (what, s, 1 + c)
            assert torch.equal(episode[s], pre["reset_count"]), "%s step %d: episode" % (what, s)
            n_moved += int(moved.sum())
        return n_moved


# ---------------------------------------------------------------- 4. tape == state, every kernel family
@pytest.mark.parametrize("E,N,sort,kernel", [(600, 10, 0, "ca_pipe_kernel<10, 4, true>"), (333, 6, 1, "ca_kernel<"),
                                             (64, 20, 0, "ca_kernel<")])
def test_tape_equals_state_ring(E, N, sort, kernel):
    # (short clocks: the slowest env of the fixtures would otherwise run for thousands of steps until its time-out)
    a, b = _fixture_sim(E, N, sort, max_time_ratio=2.0), Shadow(_fixture_sim(E, N, sort, max_time_ratio=2.0))
    a.record_trajectories()
    a.enable_lookahead(20)
    over = False
    for s in range(4000):
        fills = a._la["fills"]
        a.step_lookahead()
        if a._la["fills"] != fills:
            k = _last_kernel()
            assert k.startswith(kernel) and (" traj" in k or not kernel.startswith("ca_pipe")), k
        b.step()
        if s % 20 == 19 and bool(b.sim.game_over.all()):
            over = True
            break
    assert over, "episodes did not end"
    tape = a.trajectories()
    moved = b.check(tape, "E=%d N=%d" % (E, N))
    total = tape["rows"].shape[0] * E * N
    assert 0 < moved < total      # agents that wait for their env's game over: idle rows are part of what is checked
    assert int(tape["episode"].abs().sum()) == 0 and int(tape["epoch"].abs().sum()) == 0
    for n in ("pos_x", "pos_y", "heading", "t", "step_num", "flags"):
        assert torch.equal(a.state[n], b.sim.state[n]), n


def test_tape_equals_state_large_env_kernel():
    """8 x 70 on a make_testcase_huge table: mixed policies and dynamics, short clocks (time-outs inside the window), one
    launch per step on both sides"""
    nat, core, orc = _mods()
    from gym_collision_avoidance_amd.envs import test_cases as tc
    E, N, K = 8, 70, 19
    rng = np.random.default_rng(5)
    np.random.seed(70)
    table = tc.make_testcase_huge(E, N, side_length=2.0 * np.sqrt(N) + 3.0, speed_bnds=[0.5, 1.5], radius_bnds=[0.2, 0.5])
    pol = rng.choice([nat.POL_RVO, nat.POL_RVO, nat.POL_RVO, nat.POL_NONCOOP, nat.POL_STATIC, nat.POL_EXTERNAL,
                      nat.POL_LEARNING], (E, N)).astype(np.int32)
    dyn = rng.choice([nat.DYN_UNICYCLE, nat.DYN_UNICYCLE, nat.DYN_MAX_TURN_RATE], (E, N)).astype(np.int32)
    sims = []
    for _ in range(2):
        s = core.BatchedSim(core.make_params(E, N, max_obs=K, max_time_ratio=0.25))
        s.set_plugins(pol, dyn)
        s.reset(table)
        sims.append(s)
    a, b = sims[0], Shadow(sims[1])
    a.record_trajectories()
    for s in range(60):
        ext = rng.uniform(0.0, 1.0, (E, N, 2))
        a.step(ext)
        assert _last_kernel().startswith("ca_big_kernel")
        b.step(ext)
    tape = a.trajectories()
    moved = b.check(tape, "big")
    assert 0 < moved < 60 * E * N
    assert (b.sim.state["flags"] & nat.OUT_OF_TIME).any(), "time-outs must fall into the window"
    # a StaticPolicy agent's logged goal is its position
    st = torch.from_numpy(pol == nat.POL_STATIC).to(tape["rows"].device)
    r0 = tape["rows"][0]
    sel = st & (r0[..., 11] >= 0)
    assert sel.any() and torch.equal(r0[..., 3][sel], r0[..., 1][sel]) and torch.equal(r0[..., 4][sel], r0[..., 2][sel])


# ---------------------------------------------------------------- 5. auto-reset
@pytest.mark.parametrize("E,N,sort", [(600, 10, 0), (333, 6, 1)])
def test_tape_across_auto_resets(E, N, sort):
    from gym_collision_avoidance_amd import trajectory
    n_cases = gu.fixtures(N).shape[0]
    kw = dict(max_time_ratio=1.5)     # (short clocks: two episodes of the slowest env within ~1000 steps)
    a, b = _fixture_sim(E, N, sort, auto_reset=True, **kw), Shadow(_fixture_sim(E, N, sort, auto_reset=True, **kw))
    a.record_trajectories(max_bytes=3 << 30)
    a.enable_lookahead(20)
    for s in range(4000):        # until every env has finished two episodes
        a.step_lookahead()
        b.step()
        b.post[-1] = None        # (only the pre-step reads are compared here)
        if s % 20 == 19 and int(b.sim.state["reset_count"].min()) >= 2:
            break
    T = len(b.pre)
    assert int(b.sim.state["reset_count"].min()) >= 2, "two episodes per env did not fit %d steps" % T
    tape = a.trajectories()
    rows, episode = tape["rows"], tape["episode"]
    assert rows.shape[0] == T
    # `episode` is the reset count as each step starts; index and clock of every row are B's before the step
    for s, pre in enumerate(b.pre):
        assert torch.equal(episode[s], pre["reset_count"]), "episode @%d" % s
        m = rows[s][..., 11] >= 0
        assert torch.equal(rows[s][..., 11][m], pre["step_num"].double()[m]) and torch.equal(rows[s][..., 0][m], pre["t"][m])
    assert int(episode[-1].min()) >= 1, "every env must have started a second episode"
    # episode 0 of every table row, from a batch without auto-reset (held to its own state by the tests above)
    ref = _fixture_sim(n_cases, N, sort, **kw)
    ref.record_trajectories()
    ref.enable_lookahead(20)
    for s in range(2000):
        ref.step_lookahead()
        if s % 20 == 19 and bool(ref.game_over.all()):
            break
    assert bool(ref.game_over.all())
    rt = ref.trajectories()
    rr, re_ = rt["rows"].cpu().numpy(), rt["episode"].cpu().numpy()
    want = {}
    rows_h, ep_h = rows.cpu().numpy(), episode.cpu().numpy()
    complete = 0
    for e in range(0, E, 7):
        eps = trajectory.episodes(rows_h, ep_h, e)
        assert len(eps) == int(ep_h[-1, e]) + 1
        for k, got in enumerate(eps[:-1]):      # (the last one is still running when the tape ends)
            c = (e + k * E) % n_cases
            if c not in want:
                full = trajectory.episodes(rr, re_, c)
                assert len(full) == 1
                want[c] = full[0]
            for x, y in zip(got, want[c]):
                assert x.shape == y.shape and np.array_equal(x, y), "env %d episode %d (case %d)" % (e, k, c)
            if k >= 1:
                first = min((h[0] for h in got if h.shape[0]), key=lambda r: r[0])
                assert first[0] == 0.0
            complete += 1
        # the first row of a later episode: index 0 at t == 0 (rows of the tape itself)
        for s in np.nonzero(np.diff(ep_h[:, e]))[0] + 1:
            r = rows_h[s, e]
            m = r[:, 11] >= 0
            assert m.any() and (r[m, 11] == 0).all() and (r[m, 0] == 0.0).all()
    assert complete > E // 7, complete


# ---------------------------------------------------------------- 6. every path writes the same tape
def _same_tape(x, y, what):
    assert x["rows"].shape == y["rows"].shape, (what, x["rows"].shape, y["rows"].shape)
    assert torch.equal(x["rows"][..., 11], y["rows"][..., 11]), what + ": index column"
    m = x["rows"][..., 11] >= 0
    assert torch.equal(x["rows"][m], y["rows"][m]), what + ": rows"
    assert torch.equal(x["episode"], y["episode"]) and torch.equal(x["epoch"], y["epoch"]), what + ": episode"


def test_every_stepping_path_writes_the_same_tape():
    E, N, T = 600, 10, 150
    tapes, finals = {}, {}

    def run(name, drive, **kw):
        s = _fixture_sim(E, N, auto_reset=True, **kw)
        s.rollout(37)                # (mid-episode, some envs past their first auto-reset)
        s.record_trajectories()
        drive(s)
        tapes[name] = s.trajectories()
        assert tapes[name]["rows"].shape[0] == T, name
        finals[name] = {n: s.state[n].clone() for n in ("pos_x", "heading", "t", "step_num", "reset_count", "env_stats")}

    def steps(s):
        for _ in range(T):
            s.step()

    def chunks(s):
        for n in (1, 7, 1, 1, 30, 2, 50, 13, 45):
            s.rollout(n)

    def ring(fresh):
        def drive(s):
            s.enable_lookahead(16, fresh=fresh)
            for _ in range(T):
                s.step_lookahead()
        return drive

    def rewinding(s):
        s.enable_lookahead(32, adaptive=True, start=8)
        looks = {3, 4, 20, 21, 22, 60, 61, 95, 130}
        for t in range(1, T + 1):
            s.step_lookahead()
            if t in looks:
                s.state["pos_x"]                                    # a rewind in mid-ring
                assert s.trajectories()["rows"].shape[0] == t      # T = the steps handed out
        assert s._la["rewinds"] >= 4

    run("step pipelined", steps)
    assert _last_kernel().startswith("ca_pipe_kernel<10, 4, false>") and " traj" in _last_kernel()
    run("step unpipelined", steps, pipeline=False)
    assert _last_kernel().startswith("ca_kernel<")
    run("rollout chunks", chunks)
    run("ring fresh", ring(True))
    run("ring persistent", ring(False))
    run("ring rewound", rewinding)
    base = tapes["step pipelined"]
    assert int(base["episode"].max()) >= 1 and int((base["rows"][..., 11] >= 0).sum()) > 0
    for name in tapes:
        _same_tape(base, tapes[name], name)
        for n, v in finals[name].items():
            assert torch.equal(v, finals["step pipelined"][n]), (name, n)


def test_stop_clear_and_host_reset_marker():
    nat, core, orc = _mods()
    E, N = 64, 4
    s = _fixture_sim(E, N)
    s.record_trajectories()
    s.rollout(5)
    mask = np.zeros(E, dtype=np.uint8)
    mask[::2] = 1
    table = gu.fixtures(N)
    s.reset(table[np.arange(E) % 500], mask=mask)       # a host-side reset of every other env: no row, a new epoch
    for _ in range(3):
        s.step()
    s.stop_recording()
    s.rollout(4)
    tp = s.trajectories()
    assert tp["rows"].shape[0] == 8
    ep = tp["epoch"].cpu().numpy()
    assert (ep[:5] == 0).all() and (ep[5:, ::2] == 1).all() and (ep[5:, 1::2] == 0).all()
    from gym_collision_avoidance_amd import trajectory
    h0 = trajectory.episodes(tp["rows"], tp["episode"], 0, epoch=tp["epoch"])
    h1 = trajectory.episodes(tp["rows"], tp["episode"], 1, epoch=tp["epoch"])
    assert len(h0) == 2 and len(h1) == 1
    assert h0[0][0].shape[0] == 5 and h0[1][0].shape[0] == 3 and h0[1][0][0, 0] == 0.0 and h1[0][0].shape[0] == 8
    s.clear_trajectories()
    assert s.trajectories()["rows"].shape[0] == 0
    s.record_trajectories()
    s.step()
    assert s.trajectories()["rows"].shape[0] == 1


# ---------------------------------------------------------------- 7. recording changes nothing
def test_recording_changes_nothing():
    nat, core, orc = _mods()
    import ctypes as C
    E, N, T = 4096, 10, 90
    a, b = _fixture_sim(E, N, auto_reset=True), _fixture_sim(E, N, auto_reset=True)
    a.record_trajectories()
    for s in (a, b):
        s.enable_lookahead(20)
    for t in range(T):
        oa, ob = a.step_lookahead(), b.step_lookahead()
        if t % 20 == 0:
            assert _last_kernel() .startswith("ca_pipe_kernel<10, 4, true>")
        for x, y, n in zip(oa, ob, ("obs", "rewards", "done", "game_over")):
            assert torch.equal(x, y), "%s @%d" % (n, t)
    assert a._la["in_kernel"] and list(a._la["in_kernel"].values()) == [True] == list(b._la["in_kernel"].values())
    # the ring call of the recording 4096 x 10 batch still takes its rewind snapshot in the kernel
    prep = a._la_prepare(20)
    assert prep["traj"] is not None and prep["in_kernel"] is True
    assert nat.lib().cagpu_ring_snapshots(C.byref(a.p), C.byref(a._cs), prep["co_ref"], prep["ar_ref"], 20) == 1
    for n in a.state:
        if n == "next_action":
            ok = (a.state["flags"] & nat.PLAN_VALID) != 0
            assert torch.equal(a.state[n][ok], b.state[n][ok])
            continue
        assert torch.equal(a.state[n], b.state[n]), n
    assert torch.equal(a.episode_stats(), b.episode_stats())
    for pipeline in (True, False):     # ... and one launch per step, both kernel families
        c, d = _fixture_sim(300, N, auto_reset=True, pipeline=pipeline), _fixture_sim(300, N, auto_reset=True, pipeline=pipeline)
        c.record_trajectories()
        for t in range(60):
            oc, od = c.step(), d.step()
            assert all(torch.equal(x, y) for x, y in zip(oc, od)) and torch.equal(c.done, d.done)
        assert all(torch.equal(c.state[n], d.state[n]) for n in c.state if n != "next_action")


# ---------------------------------------------------------------- 8. reference parity
def _check_against_reference(tape, ep, name):
    from gym_collision_avoidance_amd import trajectory
    got = trajectory.episodes(tape["rows"], tape["episode"], 0, epoch=tape["epoch"])
    assert len(got) == 1
    want = reference_histories(ep)
    i = gu.COLS.index("step_num")
    rows = tape["rows"].cpu().numpy()[:, 0]
    moved = np.diff(ep.state[:, :, i], axis=0) == 1
    assert np.array_equal(rows[..., 11] >= 0, moved), name + ": moved pattern"
    assert np.array_equal(rows[..., 11][moved], ep.state[:-1, :, i][moved]), name + ": index"
    for a, (g, w) in enumerate(zip(got[0], want)):
        assert g.shape == w.shape, (name, a, g.shape, w.shape)
        d = np.abs(g - w)
        d[:, 10] = np.abs((g[:, 10] - w[:, 10] + np.pi) % (2 * np.pi) - np.pi)      # heading: modulo 2 pi
        assert d[:, :7].max(initial=0.0) <= 1e-4, (name, a, d[:, :7].max())     # t, position, goal, radius, pref_speed
        assert d[:, 7:].max(initial=0.0) <= 1e-3, (name, a, d[:, 7:].max())     # velocities, speed, heading


@pytest.mark.parametrize("name", gu.SCENARIOS)
def test_golden_free_running_history(name):
    meta, eps = gu.load(name)
    for c, ep in eps.items():
        g = _golden_sim(meta, ep)
        cases, head = ep.case()
        g.record_trajectories()
        g.reset(cases[None], headings=head[None])
        for t in range(ep.T):
            g.step(ep.ext[t][None])
        tape = g.trajectories()
        assert tape["rows"].shape[0] == ep.T and int(tape["epoch"].min()) == 1     # (recording began before the reset)
        _check_against_reference(tape, ep, "%s case %d" % (name, c))


def test_golden_history_with_static_map():
    nat, core, orc = _mods()
    meta, eps = gu.load("laser4")
    ep = eps[0]
    g = _golden_sim(meta, ep)
    g.set_map(ep.static_map)
    cases, head = ep.case()
    g.reset(cases[None], headings=head[None])
    g.record_trajectories()
    for t in range(ep.T):
        g.step(ep.ext[t][None])
    assert (g.state["flags"].cpu().numpy() & nat.IN_COLLISION).any()   # the wall collision happened
    _check_against_reference(g.trajectories(), ep, "laser4")


# ---------------------------------------------------------------- 9. env API
def test_env_api_batched_and_single():
    from gym_collision_avoidance_amd import trajectory
    Config, tc, Env = envtools.fresh("Hist4")
    try:
        env = Env(num_envs=64)
        env.set_fixture_suite(4, policies="RVO")
        env.record_trajectories()          # before reset(): survives it
        env.reset()
        for _ in range(45):
            env.step(None)
        assert "ca_pipe_kernel" in _last_kernel() or env._sim._la is not None
        tp = env.trajectories()
        assert tp["rows"].shape == (45, 64, 4, 12) and tp["rows"].is_cuda
        for e in (0, 5, 63):
            want = trajectory.episodes(tp["rows"], tp["episode"], e, epoch=tp["epoch"])
            got = env.episode_histories(e)
            assert len(got) == len(want) and all(np.array_equal(x, y) for g, w in zip(got, want) for x, y in zip(g, w))
        cur = env.episode_histories(0)[-1]
        rc = int(env._sim.state["reset_count"][0])
        for i, ag in enumerate(env.agents):
            h = ag.global_state_history
            if int(tp["episode"][-1, 0]) == rc:
                assert np.array_equal(h, cur[i]) and h.shape == (ag.step_num, 11)
            else:
                assert h.shape == (0, 11)
        assert any(ag.global_state_history.shape[0] > 0 for ag in env.agents) or int(tp["episode"][-1, 0]) != rc
        env.reset()                         # recording survives; the finished agents keep their log
        assert env._sim._traj_on and env.prev_episode_agents[0].global_state_history.shape[1] == 11
        env.step(None)
        assert env.trajectories()["rows"].shape[0] == 46
        env.clear_trajectories()
        assert env.trajectories()["rows"].shape[0] == 0
        # a single env under Config.STORE_HISTORY: the host-side log stays the source; the device tape agrees with it
        one = Env()
        one.set_agents(tc.full_test_suite(4, 3, policies="RVO"))
        one.record_trajectories()
        one.reset()
        for _ in range(40):
            one.step(None)
        tape = one.episode_histories(0)
        assert len(tape) == 1
        for i, ag in enumerate(one.agents):
            host = ag.global_state_history
            assert host.shape == tape[0][i].shape == (ag.step_num, 11) and host.shape[0] > 0
            assert np.array_equal(host[:, 1:], tape[0][i][:, 1:]), "agent %d" % i
            assert np.abs(host[:, 0] - tape[0][i][:, 0]).max() <= 1e-12
    finally:
        envtools.default()


# ---------------------------------------------------------------- 10. budget
@pytest.mark.parametrize("path", ["step", "ring", "rollout"])
def test_budget_raises_before_the_launch(path):
    nat, core, orc = _mods()
    E, N = 300, 10
    s = _fixture_sim(E, N, auto_reset=True)
    per = 96 * E * N + 4 * E
    assert s.traj_step_bytes == per
    s.record_trajectories(max_bytes=5 * per + per // 2)
    if path == "ring":
        s.enable_lookahead(4)
    advance = {"step": s.step, "ring": s.step_lookahead, "rollout": lambda: s.rollout(1)}[path]
    for _ in range(5):
        advance()
    before = {n: s.state[n].clone() for n in ("pos_x", "t", "step_num", "reset_count", "env_stats")}
    tape = s.trajectories()
    assert tape["rows"].shape[0] == 5
    with pytest.raises(nat.CagpuError) as err:
        advance()
    assert "clear_trajectories()" in str(err.value) and str(per) in str(err.value)
    if path == "rollout":
        with pytest.raises(nat.CagpuError):
            s.rollout(3)
    assert all(torch.equal(s.state[n], v) for n, v in before.items()), "no step was taken"
    again = s.trajectories()
    assert again["rows"].shape[0] == 5 and torch.equal(again["rows"][..., 11], tape["rows"][..., 11])
    s.clear_trajectories()
    for _ in range(3):
        advance()
    assert s.trajectories()["rows"].shape[0] == 3 and int(s.state["episode_step"].max()) > 0
    assert not torch.equal(s.state["t"], before["t"])


# ---------------------------------------------------------------- the batched dataset script
def test_trajectory_dataset_creator_small():
    Config, tc, Env = envtools.fresh("Hist4")
    try:
        import importlib
        mod = importlib.import_module("gym_collision_avoidance_amd.experiments.run_trajectory_dataset_creator")
        data = mod.create_dataset(num_test_cases=21, num_envs=8, seed=3)
        assert len(data) == 21 and all(len(ep) > 0 for ep in data)
        dt = Config.DT
        for ep in data:
            n = len(ep)
            for t, d in enumerate(ep):
                assert d["future_positions"].shape == (min(n - t, int(3.0 / dt)), 2)
                assert d["predicted_cmd"].shape == (1, d["future_positions"].shape[0], 2)
                assert np.array_equal(d["future_positions"][0], d["robot_state"][:2])
                assert np.array_equal(d["goal_position"], ep[0]["goal_position"])
            # the robot ends its episode at its goal, or was stopped by a collision / the clock
            assert np.isfinite(ep[-1]["robot_state"]).all() and np.isfinite(ep[-1]["pedestrian_state"]["position"]).all()
        # the same seed gives the same dataset whatever the batch size
        again = mod.create_dataset(num_test_cases=21, num_envs=5, seed=3)
        for x, y in zip(data, again):
            assert len(x) == len(y) and all(np.array_equal(p["robot_state"], q["robot_state"]) for p, q in zip(x, y))
    finally:
        envtools.default()


# ---------------------------------------------------------------- the other step() paths record the same way
@pytest.mark.parametrize("path", ["rvo_stochastic", "map_set", "ext_state"])
def test_step_paths_with_per_step_inputs_record_their_own_state(path):
    """step() with stochastic RVO draws, with a map set (walls + auto-reset map draws) and with externally integrated
    motion: the tape's rows are the recording simulator's own state around every step"""
    nat, core, orc = _mods()
    E, N = 96, 4
    s = _fixture_sim(E, N, auto_reset=(path == "map_set"))
    rng = np.random.default_rng(11)
    if path == "rvo_stochastic":
        s.set_rvo_stochastic(heading_noise=np.ones((E, N), bool), collab_coeff=-0.5, seed=5)
    elif path == "map_set":
        maps = np.zeros((3, 160, 160), dtype=bool)
        maps[1, 70:90, 70:90] = True
        maps[2, :, 100:104] = True
        s.set_map(maps, map_seed=9)
    else:
        dyn = np.zeros((E, N), dtype=np.int64)
        dyn[:, 1] = nat.DYN_EXTERNAL
        s.set_plugins(nat.POL_RVO, dyn)
    s.record_trajectories()
    sh = Shadow(s)
    for t in range(50):
        if path == "ext_state":
            st = s.state
            ext = torch.full((E, N, 5), float("nan"), dtype=torch.float64, device=st["pos_x"].device)
            ext[:, 1, 0], ext[:, 1, 1] = st["pos_x"][:, 1] + 0.01 * t, st["pos_y"][:, 1] - 0.02
            ext[:, 1, 2], ext[:, 1, 3], ext[:, 1, 4] = 0.1 * t, -0.2, 0.3
            sh.pre.append({n: st[n].clone() for n in ("t", "step_num", "reset_count")})
            s.step(ext_state=ext)
            st = s.state
            sh.post.append({n: st[n].clone() for n in ("step_num", "last_action") + tuple(c for c in POST if c)})
        else:
            sh.step()
    tape = s.trajectories()
    if path == "map_set":
        # (an auto-reset replaces the post-step state: compare what precedes the step, as in the auto-reset test)
        for i, pre in enumerate(sh.pre):
            m = tape["rows"][i][..., 11] >= 0
            assert torch.equal(tape["episode"][i], pre["reset_count"])
            assert torch.equal(tape["rows"][i][..., 11][m], pre["step_num"].double()[m])
            assert torch.equal(tape["rows"][i][..., 0][m], pre["t"][m])
        assert "ca_pipe_kernel" in _last_kernel() and " traj" in _last_kernel()
    else:
        assert sh.check(tape, path) > 0
