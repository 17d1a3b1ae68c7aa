"""The final record (include/cagpu.h CaFinal; core.BatchedSim.keep_final; env.keep_final_observations): the observation
rows and flag words of an episode's terminal step, saved by the step kernels before the auto-reset overwrites them.

The record is a copy of values the same kernel computed, so every comparison here is BIT FOR BIT (torch.equal): against a
twin batch that runs the same episodes without auto-reset, whose `obs` and `state["flags"]` at its game over are what the
record must hold.  Rows of envs that did not end an episode in a step are unspecified and never compared."""
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
from tests.test_gpu_parity import _mods  # noqa: E402

pytestmark = pytest.mark.gpu

# `cagpu_last_kernel()` of the parent commit's build (the one before the final record existed) for the bench.py default
# path -- 4096 envs x 10 RVO agents, look-ahead ring of 20 --, printed by that build on an MI355X (256 CUs)
PARENT_BENCH_KERNEL = "ca_pipe_kernel<10, 4, true> grid=1024 lds=37408 mode=0 fair"


def _last_kernel():
    return _mods()[0].lib().cagpu_last_kernel().decode()


def _owned(flags):
    """the bits of a flag word the step kernels decide (CA_PLAN_VALID is the pipelined policy query's, not an ending)"""
    nat = _mods()[0]
    return flags & nat.KERNEL_FLAG_BITS


def _sim(E, N, table, auto_reset, offset=0, stride=None, policy=None, dynamics=None, heading_seed=0, pipeline=True,
         static_map=None, headings=None, **kw):
    """a batch on `table`: env e starts on case (offset + e) % C; with auto_reset its k-th reset loads case
    (offset + e + k * stride) % C"""
    nat, core, orc = _mods()
    s = core.BatchedSim(core.make_params(E, N, **kw), pipeline=pipeline)
    s.set_plugins(nat.POL_RVO if policy is None else policy, dynamics)
    if static_map is not None:
        s.set_map(static_map, num_beams=8, num_to_store=1)
    C = table.shape[0]
    if auto_reset:
        s.set_fixture_table(table, env_id_offset=offset, case_stride=E if stride is None else stride, heading_seed=heading_seed)
    s.reset(table[(np.arange(E) + offset) % C], headings=headings)
    return s


class Endings(object):
    """the k-th ending of every env, collected on the device while a batch is stepped: the observation / flag words given
    to note() for the envs whose game_over is set, the step it happened in, and (optionally) an extra per-agent tensor"""

    def __init__(self, E, n):
        self.n, self.count, self.steps = n, None, 0
        self.obs, self.flags, self.at, self.extra = [None] * n, [None] * n, [None] * n, [None] * n

    def note(self, over, obs, flags, extra=None):
        over = over.bool()
        if self.count is None:
            self.count = torch.zeros_like(over, dtype=torch.int32)
            for k in range(self.n):
                self.obs[k], self.flags[k] = torch.zeros_like(obs), torch.zeros_like(flags)
                self.at[k] = torch.full_like(self.count, -1)
                self.extra[k] = None if extra is None else torch.zeros_like(extra)
        for k in range(self.n):
            m = over & (self.count == k)
            self.obs[k][m] = obs[m]
            self.flags[k][m] = flags[m]
            self.at[k][m] = self.steps
            if extra is not None:
                self.extra[k][m] = extra[m]
        self.count += over.to(torch.int32)
        self.steps += 1

    def all_have(self, k):
        return self.count is not None and int(self.count.min()) >= k


def _run_recorded(a, n_endings=2, max_steps=8000, extra=None, ext=None):
    """step A (auto-reset, record on) one launch per step until every env has ended n_endings episodes"""
    rec = Endings(a.E, n_endings)
    for s in range(max_steps):
        a.step(ext)
        rec.note(a.game_over, a.final_obs, a.final_flags, None if extra is None else extra(a))
        if s % 25 == 24 and rec.all_have(n_endings):
            break
    assert rec.all_have(n_endings), "not every env ended %d episodes in %d steps (min %d)" % (n_endings, max_steps,
                                                                                               int(rec.count.min()))
    return rec


def _run_twin(b, max_steps=8000, ext=None):
    """step a twin WITHOUT auto-reset until every env is over: its first (only) ending, from `obs` and the state's flags"""
    rec = Endings(b.E, 1)
    for s in range(max_steps):
        b.step(ext)
        rec.note(b.game_over, b.obs, b.state["flags"])
        if s % 25 == 24 and rec.all_have(1):
            break
    assert rec.all_have(1), "the twin's episodes did not end"
    return rec


def _same_ending(rec, k, twin, what, off=None):
    """ending k of the recorded batch == the twin's ending: the same step of the episode, rows and owned flag bits"""
    start = torch.zeros_like(rec.at[k]) if k == 0 else rec.at[k - 1] + 1
    assert torch.equal(rec.at[k] - start, twin.at[0]), what + ": episode lengths"
    assert torch.equal(rec.obs[k], twin.obs[0]), what + ": final observation rows"
    assert torch.equal(_owned(rec.flags[k]), _owned(twin.flags[0])), what + ": final flag words"


def _kinds(flags):
    """per env: (all present agents at goal, some agent in collision, no collision and some present agent out of time)"""
    nat = _mods()[0]
    d = nat.decode_flags(flags)
    here = ~d["absent"]
    coll = d["in_collision"].any(dim=1)
    return ((d["at_goal"] | ~here).all(dim=1) & ~coll, coll, ~coll & (d["ran_out_of_time"] & here).any(dim=1))


# ---------------------------------------------------------------- 1. the twin without reset, two episodes of every env
def test_twin_without_reset_two_episodes():
    nat, core, orc = _mods()
    seen = np.zeros(3, dtype=np.int64)
    batches = [
        # (E, N, policies per slot, max_time_ratio)
        (300, 4, None, 1.25),
        (256, 10, None, 1.5),
        (200, 2, nat.POL_NONCOOP, 2.0),      # both agents walk straight at their goals: head-on collisions
        (240, 6, np.array([[nat.POL_RVO, nat.POL_NONCOOP, nat.POL_RVO, nat.POL_RVO, nat.POL_NONCOOP, nat.POL_RVO]]), 1.4),
    ]
    for E, N, pol, mtr in batches:
        table = gu.fixtures(N)
        what = "E=%d N=%d" % (E, N)
        kw = dict(policy=pol, max_time_ratio=mtr)
        a = _sim(E, N, table, True, **kw)
        a.keep_final()
        # (the heading every agent starts its SECOND episode with: read off A's state right after the first auto-reset)
        rec = _run_recorded(a, 2, extra=lambda s: s.state["heading"])
        assert int(a.state["reset_count"].min()) >= 2, what
        _same_ending(rec, 0, _run_twin(_sim(E, N, table, False, **kw)), what + " first episode")
        # twin C starts on env_id_offset + case_stride: its first episode is A's second
        c = _sim(E, N, table, False, offset=E, headings=rec.extra[0], **kw)
        _same_ending(rec, 1, _run_twin(c), what + " second episode")
        for k in range(2):
            goal, coll, tout = _kinds(rec.flags[k])
            assert bool((goal | coll | tout).all()), what + ": every ending is one of the three"
            seen += np.array([int(goal.sum()), int(coll.sum()), int(tout.sum())])
        a.check_faults()
    assert (seen > 0).all(), "all at goal / collision / time-out endings seen: %s" % seen.tolist()


# ---------------------------------------------------------------- 2. every stepping path gives the same record
def test_every_path_agrees_and_the_record_changes_nothing():
    E, N, T = 600, 10, 220
    table = gu.fixtures(N)
    kw = dict(max_time_ratio=1.5)
    OUT = ("obs", "rewards", "done", "game_over")
    STATE = ("pos_x", "pos_y", "heading", "t", "time_remaining", "step_num", "flags", "reset_count", "env_stats", "ep_reward")

    def start(final, **k2):
        s = _sim(E, N, table, True, **dict(kw, **k2))
        s.rollout(37)            # (mid-episode, the first envs past their first auto-reset)
        if final:
            s.keep_final()
        return s

    def collect_steps(s, final):
        outs, fins = [], []
        for _ in range(T):
            s.step()
            outs.append({n: getattr(s, n).clone() for n in OUT})
            if final:
                fins.append((s.final_obs.clone(), s.final_flags.clone()))
        return outs, fins, {n: s.state[n].clone() for n in STATE}

    off_outs, _, off_state = collect_steps(start(False), False)
    assert _last_kernel().startswith("ca_pipe_kernel<10, 4, false> grid=150 ") and "final" not in _last_kernel()
    base_outs, base_fins, base_state = collect_steps(start(True), True)
    assert _last_kernel().startswith("ca_pipe_kernel<10, 4, false> grid=150 ") and _last_kernel().endswith(" final")
    n_defined = 0
    for t in range(T):
        for n in OUT:
            assert torch.equal(base_outs[t][n], off_outs[t][n]), "record on vs off: %s @%d" % (n, t)
        n_defined += int(base_outs[t]["game_over"].sum())
    for n in STATE:
        assert torch.equal(base_state[n], off_state[n]), "record on vs off: state %s" % n
    assert n_defined >= E // 2, "too few endings in the window: %d" % n_defined

    def same_record(t, over, fo, ff, what):
        m = over.bool()
        assert torch.equal(m, base_outs[t]["game_over"].bool()), "%s: game_over @%d" % (what, t)
        assert torch.equal(fo[m], base_fins[t][0][m]), "%s: final rows @%d" % (what, t)
        assert torch.equal(_owned(ff[m]), _owned(base_fins[t][1][m])), "%s: final flags @%d" % (what, t)

    # the unpipelined kernel (ca_kernel, reset_obs copy path), one launch per step: rows and the owned flag bits
    s = start(True, pipeline=False)
    for t in range(T):
        s.step()
        m = s.game_over.bool()
        assert torch.equal(m, base_outs[t]["game_over"].bool())
        assert torch.equal(s.final_obs[m], base_fins[t][0][m]), "ca_kernel: final rows @%d" % t
        assert torch.equal(_owned(s.final_flags[m]), _owned(base_fins[t][1][m])), "ca_kernel: final flags @%d" % t
    assert _last_kernel().startswith("ca_kernel<")

    # the look-ahead ring: fresh rings, one persistent ring, and an adaptive ring with rewinds forced in mid-ring
    for what, ring_kw, looks in (("ring fresh", dict(fresh=True), ()), ("ring persistent", dict(fresh=False), ()),
                                 ("ring rewound", dict(adaptive=True, start=8), (3, 4, 20, 21, 22, 60, 61, 95, 130, 131, 200))):
        s = start(True)
        s.enable_lookahead(32 if looks else 16, **ring_kw)
        for t in range(T):
            fills = s._la["fills"]
            obs, rew, done, over = s.step_lookahead()
            if s._la["fills"] != fills and s._la["len"] > 1:
                assert _last_kernel().startswith("ca_pipe_kernel<10, 4, true>") and _last_kernel().endswith(" final"), _last_kernel()
            fo, ff = s.lookahead_final()
            same_record(t, over, fo, ff, what)
            assert torch.equal(obs, base_outs[t]["obs"]) and torch.equal(rew, base_outs[t]["rewards"]), "%s outputs @%d" % (what, t)
            if (t + 1) in looks:
                fo, ff = fo.clone(), ff.clone()
                s.state["pos_x"]                      # a rewind in mid-ring: restore + replay of the steps handed out
                assert torch.equal(s.final_obs, fo) and torch.equal(s.final_flags, ff), "%s: record across the rewind @%d" % (what, t)
                assert torch.equal(s.obs, base_outs[t]["obs"])
        if looks:
            assert s._la["rewinds"] >= 4
        for n in STATE:
            assert torch.equal(s.state[n], base_state[n]), "%s: state %s" % (what, n)

    # rollout(n): the record of the LAST step
    s = start(True)
    t = 0
    for n in (1, 7, 1, 1, 30, 2, 50, 13, 45, 1, 1, 3, 20, 40, 5):
        s.rollout(n)
        t += n
        same_record(t - 1, s.game_over, s.final_obs, s.final_flags, "rollout(%d)" % n)
        assert torch.equal(s.obs, base_outs[t - 1]["obs"])
    assert t == T
    for n in STATE:
        assert torch.equal(s.state[n], base_state[n]), "rollout: state %s" % n
    s.check_faults()


# ---------------------------------------------------------------- 3. every kernel that auto-resets
def _ragged_table(N, seed=3):
    """the fixture cases with the last 0 .. N - 2 slots of every case emptied (radius 0: absent slots, absent slots last)"""
    t = gu.fixtures(N).copy()
    rng = np.random.default_rng(seed)
    for c in range(t.shape[0]):
        n = int(rng.integers(2, N + 1))
        t[c, n:, :] = 0.0
    return t


def _wall_map():
    """Map(16 m, 16 m, 0.1 m) with a wall along x = 0 (columns 78 .. 81), open at the very top and bottom"""
    m = np.zeros((160, 160), dtype=bool)
    m[10:150, 78:82] = True
    return m


CASES = {
    "pipelined_n10": dict(E=128, N=10, kernel="ca_pipe_kernel<10, 4, false>", final_tag=True),
    "general_n20": dict(E=48, N=20, kernel="ca_kernel<", kw=dict(max_time_ratio=1.2)),
    "ragged": dict(E=128, N=6, kernel="ca_pipe_kernel<6, 10, false>", final_tag=True, table="ragged", kw=dict(ragged=1)),
    "ragged_general": dict(E=96, N=6, kernel="ca_kernel<", table="ragged", pipeline=False, kw=dict(ragged=1)),
    "random_headings": dict(E=128, N=10, kernel="ca_kernel<", heading_seed=77),
    "no_reset_obs_second_pass": dict(E=96, N=5, kernel="ca_kernel<", drop_reset_obs=True),
    "closest_last": dict(E=128, N=6, kernel="ca_kernel<", kw=dict(sort_mode=1)),
    "static_map": dict(E=128, N=4, kernel="ca_pipe_kernel<4, 16, false>", final_tag=True, wall=True,
                       kw=dict(reward_collision_wall=-0.3125)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_kernel_keeps_the_record(name):
    nat, core, orc = _mods()
    c = CASES[name]
    E, N = c["E"], c["N"]
    table = _ragged_table(N) if c.get("table") == "ragged" else gu.fixtures(N)
    kw = dict(max_time_ratio=1.5)
    kw.update(c.get("kw", {}))
    common = dict(pipeline=c.get("pipeline", True), static_map=_wall_map() if c.get("wall") else None, **kw)
    a = _sim(E, N, table, True, heading_seed=c.get("heading_seed", 0), **common)
    if c.get("drop_reset_obs"):       # a table without precomputed reset observations: the tile senses a second time
        a._ar.reset_obs = None
    a.keep_final()
    rec = Endings(E, 2)
    walls, wall = 0, None       # (wall: the agents that hit a wall in their env's current episode)
    for s in range(8000):
        a.step()
        if s == 0:
            k = _last_kernel()
            assert k.startswith(c["kernel"]), k
            assert k.endswith(" final") == bool(c.get("final_tag")), k
        rec.note(a.game_over, a.final_obs, a.final_flags, a.state["heading"])
        if c.get("wall"):
            hit = a.rewards == -0.3125              # (the wall's own reward value: nothing else pays it)
            wall = hit if wall is None else (wall | hit)
            over = a.game_over.bool().unsqueeze(1)
            # a wall collision of the episode that just ended shows as in_collision in the record
            assert bool(((a.final_flags & nat.IN_COLLISION) != 0)[wall & over].all())
            walls += int((wall & over).sum())
            wall = wall & ~over
        if s % 25 == 24 and rec.all_have(2):
            break
    assert rec.all_have(2) and int(a.state["reset_count"].min()) >= 2
    if c.get("wall"):
        assert walls > 0, "no wall collision ended an episode"
    _same_ending(rec, 0, _run_twin(_sim(E, N, table, False, **common)), name + " first episode")
    # (random headings: twin C is given the headings A's auto-reset drew for the second episode)
    _same_ending(rec, 1, _run_twin(_sim(E, N, table, False, offset=E, headings=rec.extra[0], **common)), name + " second episode")
    if c.get("table") == "ragged":
        for k in range(2):
            absent = (rec.flags[k] & nat.ABSENT) != 0
            cases = torch.from_numpy(table[(np.arange(E) + k * E) % table.shape[0], :, 5] <= 0).to(absent.device)
            assert torch.equal(absent, cases) and bool(absent.any()), "absent slots carry CA_ABSENT"
            assert int(rec.obs[k][absent].abs().sum()) == 0, "the final rows of absent slots are zeros"
            assert bool((rec.obs[k][~absent][:, 5] > 0).all())
    a.check_faults()


def test_large_env_kernel_keeps_the_record():
    """6 x 70 on a make_testcase_huge table (the one-thread-per-agent kernel of cagpu_big.inc), mixed policies, short clocks"""
    nat, core, orc = _mods()
    from gym_collision_avoidance_amd.envs import test_cases as tc
    E, N, K, C = 6, 70, 19, 18
    rng = np.random.default_rng(11)
    np.random.seed(71)
    table = tc.make_testcase_huge(C, N, side_length=2.0 * np.sqrt(N) + 3.0, speed_bnds=[0.5, 1.5], radius_bnds=[0.2, 0.5])
    pol = rng.choice([nat.POL_RVO, nat.POL_RVO, nat.POL_NONCOOP, nat.POL_STATIC], (1, N)).astype(np.int32)
    kw = dict(policy=pol, max_obs=K, max_time_ratio=0.3)
    a = _sim(E, N, table, True, **kw)
    a.keep_final()
    rec = Endings(E, 2)
    for s in range(3000):
        a.step()
        if s == 0:
            assert _last_kernel().startswith("ca_big_kernel")
        rec.note(a.game_over, a.final_obs, a.final_flags, a.state["heading"])
        if s % 10 == 9 and rec.all_have(2):
            break
    assert rec.all_have(2) and int(a.state["reset_count"].min()) >= 2
    _same_ending(rec, 0, _run_twin(_sim(E, N, table, False, **kw)), "big first episode")
    _same_ending(rec, 1, _run_twin(_sim(E, N, table, False, offset=E, headings=rec.extra[0], **kw)), "big second episode")
    assert bool(((rec.flags[0] & nat.OUT_OF_TIME) != 0).any())
    # rollout(n) of the large-env kernel is n launches: the single block holds the most recent ending
    b = _sim(E, N, table, True, **kw)
    b.keep_final()
    first = int(rec.at[0].max()) + 1
    b.rollout(first)
    m = rec.at[1] >= first                      # envs whose only ending so far is their first
    assert bool(m.any())
    assert torch.equal(b.final_obs[m], rec.obs[0][m]) and torch.equal(_owned(b.final_flags[m]), _owned(rec.flags[0][m]))


def test_recording_and_the_final_record_together():
    """the tape is unchanged by the record, and the record by the tape -- in every stepping path"""
    E, N, T = 300, 10, 160
    table = gu.fixtures(N)

    def run(traj, final, drive, **k2):
        s = _sim(E, N, table, True, max_time_ratio=1.5, **k2)
        s.rollout(37)
        if traj:
            s.record_trajectories()
        if final:
            s.keep_final()
        fins = drive(s, final)
        return (s.trajectories() if traj else None), fins, s.state["env_stats"].clone()

    def steps(s, final):
        out = []
        for _ in range(T):
            s.step()
            out.append((s.game_over.bool().clone(), s.final_obs.clone(), s.final_flags.clone()) if final else None)
        return out

    def ring(s, final):
        s.enable_lookahead(20)
        out = []
        for _ in range(T):
            over = s.step_lookahead()[3]
            out.append((over.clone(),) + tuple(x.clone() for x in s.lookahead_final()) if final else None)
        return out

    def same_tape(x, y, what):
        assert torch.equal(x["rows"][..., 11], y["rows"][..., 11]), what
        m = x["rows"][..., 11] >= 0
        assert torch.equal(x["rows"][m], y["rows"][m]) and torch.equal(x["episode"], y["episode"]), what

    for drive, kern, k2 in ((steps, "ca_pipe_kernel<10, 4, false>", {}), (ring, "ca_pipe_kernel<10, 4, true>", {}),
                            (steps, "ca_kernel<", dict(pipeline=False))):
        tape_only, _, stats0 = run(True, False, drive, **k2)
        both_tape, both_fin, stats1 = run(True, True, drive, **k2)
        k = _last_kernel()
        assert k.startswith(kern) and (not kern.startswith("ca_pipe") or k.endswith(" traj final")), k
        _, fin_only, stats2 = run(False, True, drive, **k2)
        same_tape(tape_only, both_tape, kern)
        assert torch.equal(stats0, stats1) and torch.equal(stats0, stats2)
        n = 0
        for (o1, fo1, ff1), (o2, fo2, ff2) in zip(both_fin, fin_only):
            assert torch.equal(o1, o2) and torch.equal(fo1[o1], fo2[o1]) and torch.equal(_owned(ff1[o1]), _owned(ff2[o1])), kern
            n += int(o1.sum())
        assert n > 0


# ---------------------------------------------------------------- 4. off means off
def test_off_means_off_on_the_bench_geometry():
    """a sim that never enables the record runs the parent commit's kernel on the bench.py default path"""
    nat, core, orc = _mods()
    E, N = 4096, 10
    s = _sim(E, N, gu.fixtures(N), True)
    assert s.final_obs is None and s.final_flags is None
    s.enable_lookahead(20, fresh=True)
    for _ in range(40):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.sync()
    s.step()
    assert _last_kernel() == PARENT_BENCH_KERNEL.replace("true", "false").replace(" fair", "")
    # ... and with it on, the same selection, grid and block, the flagged instantiation
    s.keep_final()
    s.enable_lookahead(20, fresh=True)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL + " final"
    s.keep_final(False)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.check_faults()


def test_keep_final_refusals():
    nat, core, orc = _mods()
    E, N = 16, 4
    table = gu.fixtures(N)
    s = _sim(E, N, table, False)
    with pytest.raises(nat.CagpuError, match="fixture table"):
        s.keep_final()
    s = _sim(E, N, table, True)
    s.set_sensor_variants([(np.arange(N) == 1, 2, nat.SORT_CLOSEST_LAST)])
    with pytest.raises(nat.CagpuError, match="variants"):
        s.keep_final()
    s.set_sensor_variants(None)
    s.keep_final()
    with pytest.raises(nat.CagpuError, match="keep_final"):
        s.set_sensor_variants([(np.arange(N) == 1, 2, nat.SORT_CLOSEST_LAST)])
    s.step()
    assert s.final_obs.shape == (E, N, s.W) and s.final_flags.shape == (E, N)
    s.set_fixture_table(None)          # no auto-reset any more: the record goes with the table
    assert s.final_obs is None
    s.step()
    assert not _last_kernel().endswith(" final")


# ---------------------------------------------------------------- 5. the env API
def test_env_api_final_observation_and_truncated():
    Config, tc, Env = envtools.fresh("Hist4")
    try:
        Config.MAX_TIME_RATIO = 1.3          # (short clocks: time-outs, and two episodes of every env within the loop)
        E, N = 96, 4

        def make(auto_reset, final, lookahead=None):
            env = Env(num_envs=E, lookahead=lookahead)
            env.set_fixture_suite(N, policies="RVO", auto_reset=auto_reset)
            if final:
                env.keep_final_observations()      # before reset(): survives it
            env.reset()
            return env

        # the default: exactly today's return values
        plain = make(True, False)
        for _ in range(3):
            out = plain.step(None)
            assert out[3] is False and sorted(out[4]) == ["which_agents_done", "which_agents_learning"]
        out = plain.rollout(5)
        assert out[3] is False and sorted(out[4]) == ["which_agents_done", "which_agents_learning"]
        # refusals
        with pytest.raises(ValueError, match="auto_reset"):
            make(False, True)
        with pytest.raises(ValueError, match="batched"):
            Env().keep_final_observations()

        for lookahead in (None, 0):       # served from the look-ahead ring / one launch per step
            a, b = make(True, True, lookahead), make(False, False, 0)
            assert a._sim._fin_on and (a._sim._la is not None) == (lookahead is None)
            first = torch.zeros((E,), dtype=torch.bool, device=a._sim.device)
            n_trunc = n_over = 0
            agents0 = None
            for s in range(3000):
                obs, rew, over, truncated, info = a.step(None)
                b_obs, _, b_over, b_trunc, b_info = b.step(None)
                assert b_trunc is False
                assert sorted(info) == ["final_info", "final_observation", "which_agents_done", "which_agents_learning"]
                assert sorted(info["final_info"]) == ["at_goal", "in_collision", "ran_out_of_time"]
                assert truncated.dtype == torch.bool and truncated.shape == (E,)
                assert info["final_observation"].shape == obs.shape == (E, N, a._sim.W)
                assert not bool((truncated & ~over).any())
                new = over & ~first         # envs ending their FIRST episode now: the twin's game over of the same step
                if bool(new.any()):
                    assert bool(b_over[new].all())
                    assert torch.equal(info["final_observation"][new], b_obs[new])
                    d = {k: v.clone() for k, v in info["final_info"].items()}
                    fl = b._sim.state["flags"]
                    want = {"at_goal": (fl & 1) != 0, "in_collision": (fl & 4) != 0, "ran_out_of_time": (fl & 16) != 0}
                    for k in want:
                        assert torch.equal(d[k][new], want[k][new]), k
                    want_trunc = ~want["in_collision"].any(dim=1) & want["ran_out_of_time"].any(dim=1)
                    assert torch.equal(truncated[new], want_trunc[new])
                    n_trunc += int(truncated[new].sum())
                    n_over += int(new.sum())
                    if bool(new[0]):        # env 0 has Agent views: the twin's per-agent booleans
                        agents0 = [(ag.is_at_goal, ag.in_collision, ag.ran_out_of_time) for ag in b.agents]
                        got = [(bool(d["at_goal"][0, i]), bool(d["in_collision"][0, i]), bool(d["ran_out_of_time"][0, i]))
                               for i in range(N)]
                        assert got == agents0
                        assert bool(truncated[0]) == (not any(x[1] for x in agents0) and any(x[2] for x in agents0))
                    first |= new
                if s % 20 == 19 and bool(first.all()):
                    break
            assert bool(first.all()) and agents0 is not None and n_over == E
            assert 0 < n_trunc < E, "time-outs and other endings both occur: %d of %d" % (n_trunc, E)
            if lookahead is None:
                assert a._sim._la["rewinds"] == 0, "reading the record must not rewind the ring"
            # rollout(): the items of its last step
            out = a.rollout(7)
            assert "final_observation" in out[4] and out[3].shape == (E,) and not bool((out[3] & ~out[2]).any())
            # switching it off again restores the plain return values
            a.keep_final_observations(False)
            out = a.step(None)
            assert out[3] is False and sorted(out[4]) == ["which_agents_done", "which_agents_learning"]
    finally:
        envtools.default()
