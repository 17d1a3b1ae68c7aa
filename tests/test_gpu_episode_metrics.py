"""The episode metrics on the device (include/cagpu.h CaEpMetrics, csrc/cagpu_metrics.inc; core.BatchedSim.measure_episodes /
episode_metrics) against tests/episode_metrics_ref.py, BIT FOR BIT: the reference file states every output as a chain of
single float64 operations in a fixed order, the kernel evaluates the same chain (no multiply-add, one lane per agent adds
in slot order, correctly rounded sqrt, exact remainder), so every comparison here is an equality of bit patterns -- the
sums included; no tolerance is used anywhere.

Synthetic tapes go through the C ABI with NaN in columns 0 - 10 of every row that did not move (a NaN in an output is a
forbidden read); real tapes come from RVO batches on fixture rows, measured through step(), rollout() chunks, a
look-ahead ring with rewinds and with a transient tape, and are held to the reference file run on a twin's whole tape."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import episode_metrics_ref as ref  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests.test_episode_metrics_host import _five_episodes  # noqa: E402
from tests.test_gpu_final_obs import PARENT_BENCH_KERNEL, _last_kernel, _ragged_table, _sim  # noqa: E402
from tests.test_gpu_parity import _mods  # noqa: E402

pytestmark = pytest.mark.gpu

DT, CLOSE = 0.1, 0.2
FLOATS = ("path_length", "min_gap", "turn_sum", "min_gap_t")
INTS = ("moved_steps", "close_steps", "min_gap_partner")


def _bits(x):
    return np.ascontiguousarray(x).view(np.int64)


# ---------------------------------------------------------------- synthetic tapes through the C ABI
def synthetic_tape(N, E, T, seed):
    """ragged slots, agents that stop early or never move, episode changes (one at slot 1, one at the last slot), random
    positions a few radii apart -- and, in env 0, an exact gap tie between two partners of agent 0"""
    rng = np.random.default_rng(seed)
    rows = np.full((T, E, N, 12), np.nan)
    rows[..., 11] = -1.0
    ep = np.zeros((T, E), np.int32)
    for e in range(E):
        change = np.zeros(T, bool)
        change[rng.integers(0, T, size=max(1, T // 9))] = True
        if T >= 2:
            change[1] = change[T - 1] = True
        change[0] = False
        ep[:, e] = 3 * e + np.cumsum(change)        # (an env's first id need not be 0)
        side = 0.6 * math.sqrt(N) + 0.5
        for a in range(N):
            idx = 0
            for t in range(T):
                if t == 0 or change[t]:
                    idx = 0
                    never = rng.random() < 0.15                 # an absent slot of this episode
                    stop = rng.integers(1, 8) if rng.random() < 0.4 else T + 1
                    pos = rng.uniform(-side, side, 2)
                    rad = rng.uniform(0.1, 0.3)
                    hd = rng.uniform(-math.pi, math.pi)
                if never or idx >= stop or (T > 2 and rng.random() < 0.05):   # (a ragged slot: skipped, moves on later)
                    continue
                v = rng.uniform(-1.5, 1.5, 2)
                pos = pos + v * DT
                hd = math.remainder(hd + rng.uniform(-1.0, 1.0), 2 * math.pi)
                rows[t, e, a] = (0.1 * idx, pos[0], pos[1], 9.0, 9.0, rad, 1.0, v[0], v[1], 1.0, hd, idx)
                idx += 1
    if N >= 3:      # a tie: agents 1 and 2 mirrored about agent 0's x axis, equal radii, in a slot of env 0
        t = T - 1 if T < 3 else T // 2
        for a, (x, y) in enumerate(((0.0, 0.0), (0.75, 0.5), (0.75, -0.5))):
            rows[t, 0, a] = (0.7, x, y, 9.0, 9.0, 0.125, 1.0, 0.25, 0.5, 1.0, 0.25, 3)
    return rows, ep


class Device(object):
    """the buffers of one CaEpMetrics on the device and the call"""

    def __init__(self, N, E, C):
        nat, core, _ = _mods()
        self.nat, self.lib = nat, nat.lib()
        self.p = core.make_params(E, N, dt=DT)
        dev = "cuda:0"
        self.vals = torch.zeros((E, C, N, 4), dtype=torch.float64, device=dev)
        self.cnts = torch.zeros((E, C, N, 4), dtype=torch.int32, device=dev)
        self.head = torch.full((E, C), -1, dtype=torch.int32, device=dev)
        nbytes = int(self.lib.cagpu_episode_metrics_carry_bytes(ctypes.byref(self.p)))
        assert nbytes == E * (80 * N + 16)
        self.carry = torch.zeros((E, nbytes // E), dtype=torch.uint8, device=dev)
        self.m = nat.CaEpMetrics(vals=self.vals.data_ptr(), cnts=self.cnts.data_ptr(), head=self.head.data_ptr(), capacity=C,
                                 carry=self.carry.data_ptr(), getting_close_range=CLOSE)

    def process(self, rows, ep):
        """rows / ep: device tensors [T, E, N, 12] / [T, E] (contiguous)"""
        t = self.nat.CaTraj(rows=rows.data_ptr(), episode=ep.data_ptr())
        self.nat.check(self.lib.cagpu_episode_metrics(ctypes.byref(self.p), ctypes.byref(t), int(rows.shape[0]), ctypes.byref(self.m),
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return self

    def out(self):
        torch.cuda.synchronize()
        return self.vals.cpu().numpy(), self.cnts.cpu().numpy(), self.head.cpu().numpy()


def _same(dev_out, want, what):
    vals, cnts, head = dev_out
    assert np.array_equal(head, want.head), what + ": stamps"
    assert np.array_equal(cnts, want.cnts), what + ": moved_steps / close_steps / min_gap_partner"
    for i, n in enumerate(FLOATS):
        assert np.array_equal(_bits(vals[..., i]), _bits(want.vals[..., i])), what + ": " + n
    written = head >= 0
    assert not np.isnan(vals[written][..., :3]).any(), what + ": a NaN was read from a row that did not move"


@pytest.mark.parametrize("N", [1, 2, 10, 63, 64, 65, 130])
def test_synthetic_tapes_equal_the_reference_bit_for_bit(N):
    for E in (1, 5):
        for T in (1, 2, 37):
            rows, ep = synthetic_tape(N, E, T, seed=1000 * N + 10 * E + T)
            drows, dep = torch.from_numpy(rows).cuda(), torch.from_numpy(ep).cuda()
            for C in (1, 2, 16):
                what = "N=%d E=%d T=%d C=%d" % (N, E, T, C)
                want = ref.Metrics(E, N, C, DT, CLOSE).process(rows, ep)
                got = Device(N, E, C).process(drows, dep).out()
                assert _last_kernel().startswith("metrics_kernel<%d> grid=%d threads=%d " % (64 if N <= 64 else 1024, E, -(-N // 64) * 64))
                _same(got, want, what)


@pytest.mark.parametrize("N", [3, 70])
def test_a_gap_tie_goes_to_the_lower_partner(N):
    """agents 1 and 2 mirrored about agent 0's x axis with equal radii: equal gaps to the bit"""
    rows = np.full((2, 1, N, 12), np.nan)
    rows[..., 11] = -1.0
    spots = [(0.0, 0.0), (0.75, 0.5), (0.75, -0.5)] + [(40.0 + 3.0 * a, 7.0) for a in range(3, N)]
    for t in range(2):
        for a, (x, y) in enumerate(spots):
            rows[t, 0, a] = (0.1 * t, x, y, 9.0, 9.0, 0.125, 1.0, 0.0, 0.0, 0.0, 0.0, t)
    ep = np.zeros((2, 1), np.int32)
    want = ref.Metrics(1, N, 1, DT, CLOSE).process(rows, ep)
    assert want.cnts[0, 0, :3, ref.PARTNER].tolist() == [1, 0, 0]
    assert want.vals[0, 0, 0, ref.GAP] == (math.sqrt(0.75 * 0.75 + 0.5 * 0.5) - 0.125) - 0.125
    assert want.vals[0, 0, 0, ref.GAP_T] == 0.0       # (the first of two equal minima in time as well: strictly smaller only)
    _same(Device(N, 1, 1).process(torch.from_numpy(rows).cuda(), torch.from_numpy(ep).cuda()).out(), want, "tie N=%d" % N)


@pytest.mark.parametrize("N,E,C", [(10, 5, 2), (65, 1, 16), (64, 5, 1)])
def test_two_calls_give_the_bytes_of_one(N, E, C):
    T = 37
    rows, ep = synthetic_tape(N, E, T, seed=77 + N)
    drows, dep = torch.from_numpy(rows).cuda(), torch.from_numpy(ep).cuda()
    one = Device(N, E, C).process(drows, dep)
    _same(one.out(), ref.Metrics(E, N, C, DT, CLOSE).process(rows, ep), "one call")
    for cut in range(1, T):
        two = Device(N, E, C).process(drows[:cut], dep[:cut]).process(drows[cut:], dep[cut:])
        torch.cuda.synchronize()
        for n in ("vals", "cnts", "head", "carry"):
            a, b = getattr(one, n), getattr(two, n)
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "cut at %d: %s" % (cut, n)


def test_overwritten_episodes_are_counted_as_dropped():
    from gym_collision_avoidance_amd import episode_metrics as em
    rows, ep, want = _five_episodes(E=3, N=2, C=2)
    d = Device(2, 3, 2).process(torch.from_numpy(rows).cuda(), torch.from_numpy(ep).cuda())
    _same(d.out(), want, "five episodes, two slots")
    rc = torch.tensor([5, 4, 5], device="cuda")
    out, cur = em.drain(d.vals, d.cnts, d.head, torch.zeros(3, dtype=torch.int64, device="cuda"), rc)
    assert out["dropped"] == 9 and out["env"].tolist() == [0, 0, 1, 2, 2] and out["episode"].tolist() == [3, 4, 3, 3, 4]
    tab = ref.episode_table(rows, ep, 0.1, 0.2)
    for i, (e, k) in enumerate(zip(out["env"].tolist(), out["episode"].tolist())):
        assert np.array_equal(_bits(out["min_gap"][i].cpu().numpy()), _bits(tab[(e, k)][0][:, ref.GAP]))
        assert np.array_equal(out["close_steps"][i].cpu().numpy(), tab[(e, k)][1][:, ref.CLOSE])


# ---------------------------------------------------------------- real tapes
def _short_table(N, kind, skip=0, cap=7.0):
    """(table, max_time_ratio): 12 of the fixture cases whose slowest agent needs the least time (those from `skip` on), and
    the ratio at which every episode is over within `cap` s (7 s = 70 steps: two episodes in 150); in case 0 agent 0 and the
    agent whose goal lies furthest from it start overlapping: a collision"""
    if kind == "huge":
        from gym_collision_avoidance_amd.envs import test_cases as tc
        np.random.seed(71)
        table = tc.make_testcase_huge(6, N, side_length=2.0 * np.sqrt(N) + 3.0, speed_bnds=[0.5, 1.5], radius_bnds=[0.2, 0.5])
    else:
        table = (_ragged_table(N) if kind == "ragged" else gu.fixtures(N)).copy()
    here = table[..., 5] > 0
    need = np.where(here, np.hypot(table[..., 2] - table[..., 0], table[..., 3] - table[..., 1]) / np.where(here, table[..., 4], 1.0), 0.0)
    order = np.argsort(need.max(1), kind="stable")[skip:skip + 12]
    table, need = table[order].copy(), need[order]
    far = np.where(table[0, :, 5] > 0, np.hypot(*(table[0, :, 2:4] - table[0, 0, :2]).T), -1.0)
    far[0] = -1.0
    b = int(np.argmax(far))     # (not an agent that would start AT its goal: that one is never marked in collision)
    table[0, b, :2] = table[0, 0, :2] + np.array([0.3 * (table[0, 0, 5] + table[0, b, 5]), 0.0])
    return table, cap / float(need.max())


# Which rows (skip) and which episode length (cap): the step kernels mark an agent in collision by the env's rule
# (collision_avoidance_env.py:394-456) -- ALSO one that ran out of time, stands where it stopped and is run into by a mover
# afterwards, and NOT one that overlaps somebody in the step it reaches its goal --, while an agent's min_gap is measured in
# the steps it moves in.  "collision bit <=> min_gap <= 0" therefore holds on batches in which nobody is run into after it
# stopped and nobody reaches its goal inside somebody; these rows are such batches (most others of the table are not: with
# max_time_ratio < 1 every agent runs out of time somewhere along its way and RVO agents do run into the ones left standing).
REAL = {
    "pipelined_70x10": dict(E=70, N=10, kernel="ca_pipe_kernel<10,", skip=36, cap=5.0),
    "general_9x20": dict(E=9, N=20, kernel="ca_kernel<", skip=12, cap=3.5),
    "big_3x70": dict(E=3, N=70, kernel="ca_big_kernel", kind="huge"),
    "ragged_40x6": dict(E=40, N=6, kernel="ca_pipe_kernel<6,", kind="ragged", kw=dict(ragged=1), skip=12),
}
STEPS = 150


def _records(drains):
    """drains of one sim -> {(env, episode): {name: numpy [N]}}; nothing may have been dropped"""
    out = {}
    for d in drains:
        assert d["dropped"] == 0
        env, k = d["env"].tolist(), d["episode"].tolist()
        cols = {n: d[n].cpu().numpy() for n in FLOATS + INTS}
        for i, key in enumerate(zip(env, k)):
            assert key not in out, "episode %s drained twice" % (key,)
            out[key] = {n: cols[n][i] for n in cols}
    return out


def _same_records(got, want, what):
    assert sorted(got) == sorted(want), what + ": the drained episodes"
    for key in want:
        for n in FLOATS:
            assert np.array_equal(_bits(got[key][n]), _bits(want[key][n])), "%s: %s of %s" % (what, n, key)
        for n in INTS:
            assert np.array_equal(got[key][n], want[key][n]), "%s: %s of %s" % (what, n, key)


@pytest.mark.parametrize("name", sorted(REAL))
def test_real_tapes_four_launch_patterns_equal_the_reference(name):
    nat, core, orc = _mods()
    from gym_collision_avoidance_amd import episodes as eps
    c = REAL[name]
    E, N = c["E"], c["N"]
    table, ratio = _short_table(N, c.get("kind"), c.get("skip", 0), c.get("cap", 7.0))
    kw = dict(max_time_ratio=ratio, **c.get("kw", {}))
    start = lambda: _sim(E, N, table, True, **kw)

    # the twin: one launch per step, the tape kept, the log on -- its whole tape is what the reference file reads
    twin = start()
    twin.log_episodes(capacity=8)
    twin.measure_episodes(capacity=8, keep_tape=True)
    drains, logs = [], []
    for t in range(STEPS):
        twin.step()
        if t % 40 == 39:
            drains.append(twin.episode_metrics())
            logs.append(twin.episodes())
    assert _last_kernel().startswith("metrics_kernel<%d>" % (64 if N <= 64 else 1024))
    drains.append(twin.episode_metrics())
    logs.append(twin.episodes())
    tape = twin.trajectories()
    rows, ep = tape["rows"].cpu().numpy(), tape["episode"].cpu().numpy()
    assert rows.shape == (STEPS, E, N, 12) and not tape["epoch"].any()
    finished = twin.state["reset_count"].cpu().numpy()
    table_ref = ref.episode_table(rows, ep, twin.p.dt, twin.p.getting_close_range)
    want = {key: dict([(n, v[:, i]) for i, n in enumerate(FLOATS)] + [(n, cn[:, i]) for i, n in enumerate(INTS)])
            for key, (v, cn) in table_ref.items() if key[1] < finished[key[0]]}

    # the preconditions, on the reference side: nothing below passes vacuously
    assert (finished >= 2).all(), "every env finishes at least two episodes: %s" % finished.tolist()
    log = {n: torch.cat([d[n] for d in logs]).cpu().numpy() for n in ("env", "episode", "outcome", "flags")}
    assert sum(d["dropped"] for d in logs) == 0 and len(log["env"]) == len(want) == int(finished.sum())
    assert (log["outcome"] == 0).any(), "at least one episode ends in a collision"
    moved = rows[..., 11] >= 0
    last_move = np.where(moved, np.arange(STEPS)[:, None, None], -1)
    stops_early = False
    for (e, k) in want:
        ts = np.flatnonzero(ep[:, e] == k)
        lm = last_move[ts, e].max(0)
        stops_early |= bool(((lm >= 0) & (lm < ts[-1])).any() and (lm == ts[-1]).any())
    assert stops_early, "some agent stops before its episode ends while another still moves"

    got = _records(drains)
    _same_records(got, want, "step()")

    # joined with the log: in collision <=> the gap closed, and moved_steps is the agent's final step_num
    for i, key in enumerate(zip(log["env"].tolist(), log["episode"].tolist())):
        in_coll = (log["flags"][i].astype(np.int64) & nat.IN_COLLISION) != 0
        assert np.array_equal(in_coll, got[key]["min_gap"] <= 0.0), "collision bit vs min_gap, episode %s" % (key,)
        near = np.abs(got[key]["min_gap"]) < 1e-12
        assert not near.any(), "a gap within 1e-12 of zero decides nothing: choose another fixture"
        ts = np.flatnonzero(ep[:, key[0]] == key[1])
        assert np.array_equal(got[key]["moved_steps"], rows[ts, key[0], :, 11].max(0).astype(np.int64) + 1), key

    def run(sim, drive):
        sim.measure_episodes(capacity=8, keep_tape=drive != "transient")
        ds, peak = [], 0
        if drive == "rollout":
            for i in range(STEPS // 5):
                sim.rollout(5)
                if i % 7 == 6:
                    ds.append(sim.episode_metrics())
        elif drive == "ring":
            sim.enable_lookahead(7, fresh=True)
            for t in range(STEPS):
                sim.step_lookahead()
                if t % 31 == 10:
                    assert 0 < sim._la["t"] < sim._la["len"]
                    rewinds = sim._la["rewinds"]
                    sim.state["pos_x"]              # a state read in mid-ring: rewind and replay
                    assert sim._la["rewinds"] == rewinds + 1
                if t % 31 == 20:
                    assert 0 < sim._la["t"] < sim._la["len"]
                    rewinds = sim._la["rewinds"]
                    ds.append(sim.episode_metrics())   # a drain in mid-ring: the part behind the step handed out, no rewind
                    assert sim._la["rewinds"] == rewinds
            sim.sync()
        else:
            for t in range(STEPS):
                sim.step() if t % 2 else sim.rollout(1)
                peak = max(peak, sim.tape_bytes)
            assert peak <= sim.traj_step_bytes and sim.trajectories()["rows"].shape[0] == 0
        ds.append(sim.episode_metrics())
        assert torch.equal(sim.state["reset_count"].cpu(), torch.from_numpy(finished))
        return _records(ds)

    for drive in ("rollout", "ring", "transient"):
        _same_records(run(start(), drive), want, drive)
    probe = start()          # (what the batch itself runs on: the step kernel the case is named for)
    probe.step()
    assert _last_kernel().startswith(c["kernel"]), _last_kernel()
    twin.check_faults()


def test_a_long_run_with_a_transient_tape_stays_within_one_chunk():
    E, N = 70, 10
    table, ratio = _short_table(N, None)
    s = _sim(E, N, table, True, max_time_ratio=ratio)
    s.record_trajectories(max_bytes=8 * s.traj_step_bytes)     # a budget a kept tape would overrun after 8 steps
    s.measure_episodes(capacity=16)
    s.enable_lookahead(8, fresh=True)
    peak, n = 0, 0
    for t in range(400):
        s.step_lookahead()
        peak = max(peak, s.tape_bytes)
        if t % 100 == 99:
            d = s.episode_metrics()
            assert d["dropped"] == 0
            n += int(d["env"].shape[0])
    s.sync()
    assert peak == 8 * s.traj_step_bytes
    for _ in range(20):
        s.step()
        assert s.tape_bytes == 0
    s.rollout(8)
    assert s.tape_bytes == 0
    d = s.episode_metrics()
    assert n + int(d["env"].shape[0]) == int(s.state["reset_count"].sum()) and n > 4 * E
    s.check_faults()


def test_a_masked_reset_discards_only_the_running_episodes_of_its_envs():
    E, N = 16, 10
    table, ratio = _short_table(N, None)
    a, b = (_sim(E, N, table, True, max_time_ratio=ratio) for _ in range(2))
    for s in (a, b):
        s.measure_episodes(capacity=8, keep_tape=True)
        s.rollout(90)
    mask = (np.arange(E) % 2 == 0)
    cases = table[np.arange(E) % table.shape[0]]
    rc_before = a.state["reset_count"].clone()
    a.reset(cases, mask=mask.astype(np.uint8))
    head = a._met["head"].cpu().numpy()
    assert (head[mask] == -1).all() and (head[~mask] >= 0).any(1).all()
    assert not a._met["carry"].cpu().numpy()[mask].any() and a._met["carry"].cpu().numpy()[~mask].any(1).all()
    assert a._met["cursor"].cpu().numpy()[mask].tolist() == [0] * int(mask.sum())
    a.rollout(80)
    b.rollout(80)
    da, db = _records([a.episode_metrics()]), _records([b.episode_metrics()])
    # the envs that were not reset: the same records as the sim nobody touched
    keep = {k: v for k, v in db.items() if not mask[k[0]]}
    _same_records({k: v for k, v in da.items() if not mask[k[0]]}, keep, "untouched envs")
    # the envs that were: episodes counted from 0 again, measured from the reset on -- the reference on the tape behind it
    tape = a.trajectories()
    rows, ep, epoch = (tape[n].cpu().numpy() for n in ("rows", "episode", "epoch"))
    assert (rc_before.cpu().numpy()[mask] >= 1).all() and epoch[-1].tolist() == mask.astype(int).tolist()
    tab = ref.episode_table(rows[90:], ep[90:], a.p.dt, a.p.getting_close_range)
    fin = a.state["reset_count"].cpu().numpy()
    want = {k: dict([(n, v[:, i]) for i, n in enumerate(FLOATS)] + [(n, c[:, i]) for i, n in enumerate(INTS)])
            for k, (v, c) in tab.items() if mask[k[0]] and k[1] < fin[k[0]]}
    assert len(want) >= int(mask.sum())
    _same_records({k: v for k, v in da.items() if mask[k[0]]}, want, "reset envs")


# ---------------------------------------------------------------- off means off
def test_off_means_off_on_the_bench_geometry():
    """a sim that never measures runs the parent commit's kernel on the bench.py default path, and no tape"""
    E, N = 4096, 10
    s = _sim(E, N, gu.fixtures(N), True)
    s.enable_lookahead(20, fresh=True)
    for _ in range(40):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    assert s._met is None and s._traj is None and s.tape_bytes == 0
    nat = _mods()[0]
    with pytest.raises(nat.CagpuError, match="measure_episodes"):
        s.episode_metrics()
    s.measure_episodes()
    for _ in range(40):
        s.step_lookahead()
    assert _last_kernel().startswith(PARENT_BENCH_KERNEL.split(">")[0] + ">") and _last_kernel().endswith(" traj")
    assert s.episode_metrics()["dropped"] == 0
    assert _last_kernel().startswith("metrics_kernel<64> grid=4096 ")
    s.measure_episodes(on=False)
    for _ in range(40):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL and s.tape_bytes == 0
    s.check_faults()


# ---------------------------------------------------------------- the env API and the suite
def test_env_api_episode_log_gains_the_metric_columns():
    from tests import envtools
    Config, tc, Env = envtools.fresh("Hist4")
    try:
        Config.MAX_TIME_RATIO = 1.3
        E, N = 48, 4

        def make(metrics):
            env = Env(num_envs=E)
            env.set_fixture_suite(N, policies="RVO", auto_reset=True)
            env.log_episodes()
            if metrics:
                env.measure_episodes()        # before reset(): survives it
            env.reset()
            return env

        with pytest.raises(ValueError, match="batched"):
            Env().measure_episodes()
        with pytest.raises(RuntimeError, match="measure_episodes"):
            make(False).episode_metrics()
        plain, env = make(False), make(True)
        assert env._sim._met is not None and env._sim._la is not None and plain._sim._met is None
        for _ in range(150):
            a, b = env.step(None), plain.step(None)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        rewinds = env._sim._la["rewinds"]
        log, base = env.episode_log(), plain.episode_log()
        assert env._sim._la["rewinds"] == rewinds, "reading the log must not rewind the ring"
        added = FLOATS + INTS + ("has_metrics", "metrics_dropped")
        assert sorted(log) == sorted(list(base) + list(added))
        M = len(log["env"])
        assert M > E // 2 and log["dropped"] == 0 and log["metrics_dropped"] == 0 and log["has_metrics"].all()
        for n in base:         # the log's own columns are what they are without the metrics
            assert np.array_equal(log[n], base[n]) if isinstance(base[n], np.ndarray) else log[n] == base[n], n
        for n in FLOATS:
            assert log[n].shape == (M, N) and log[n].dtype == np.float64
        for n in INTS:
            assert log[n].shape == (M, N) and log[n].dtype == np.int32
        assert np.array_equal(log["moved_steps"].max(1), log["steps"])     # the last agent to stop moved in every step
        assert (log["path_length"] > 0).all() and (log["min_gap_partner"] >= 0).all()
        assert env._sim.tape_bytes <= env._sim._la["len"] * env._sim.traj_step_bytes   # the tape is transient
        env.measure_episodes(False)
        assert env._sim._met is None and sorted(env.episode_log()) == sorted(base)
    finally:
        envtools.default()


def test_run_suite_logged_with_metrics():
    from tests import envtools
    Config, tc, Env = envtools.fresh("FullTestSuite")
    try:
        import importlib
        rs = importlib.import_module("gym_collision_avoidance_amd.experiments.run_full_test_suite")
        a, b = rs.run_suite_logged("RVO", 4, range(12), metrics=True), rs.run_suite_logged("RVO", 4, range(12))
        new = ("path_length", "min_gap", "turn_sum", "close_steps")
        assert tuple(a.columns) == tuple(b.columns) + new and len(a) == len(b) == 12
        for col in b.columns:
            x, y = a[col].tolist(), b[col].tolist()
            assert np.array_equal(np.asarray(np.stack(x) if isinstance(x[0], np.ndarray) else x),
                                  np.asarray(np.stack(y) if isinstance(y[0], np.ndarray) else y)), col
        gap, coll = np.stack(a["min_gap"].tolist()), np.asarray(a["collision"].tolist())
        assert gap.shape == (12, 4) and np.isfinite(gap).all() and np.stack(a["close_steps"].tolist()).dtype == np.int32
        assert (~coll | (gap <= 0).any(1)).all()      # (whoever moved into somebody closed its own gap)
        assert (np.stack(a["path_length"].tolist()) > 0).all()
    finally:
        envtools.default()
