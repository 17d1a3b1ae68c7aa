"""The episode log (include/cagpu.h CaEpLog; core.BatchedSim.log_episodes / episodes; env.log_episodes / episode_log):
one record per finished episode, stored by the step kernels at the auto-reset that would otherwise overwrite it.

A record is a copy of values the same kernel computed (the three per-agent addends of env_stats[5..7], the flag words, the
episode's step count), so every comparison here is BIT FOR BIT (torch.equal / np.array_equal): against a twin batch that
runs the same episode without auto-reset and is read at its game over, against the log another stepping path wrote, and
against the sums in env_stats."""
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
from tests.test_gpu_final_obs import (CASES, PARENT_BENCH_KERNEL, Endings, _kinds, _last_kernel, _owned,  # noqa: E402
                                      _ragged_table, _sim)
from tests.test_gpu_parity import _mods, _swap_cases  # noqa: E402

pytestmark = pytest.mark.gpu

PER_AGENT = ("total_reward", "time_to_goal", "extra_time_to_goal", "flags")
PER_EPISODE = ("env", "episode", "case", "steps", "outcome")


# ---------------------------------------------------------------- helpers
def _cat(drains):
    """several drains of one sim -> one dict ordered by (env, episode); `dropped` summed"""
    out = {n: torch.cat([d[n] for d in drains]) for n in PER_EPISODE + PER_AGENT}
    order = torch.argsort(out["env"] * (1 << 32) + out["episode"])
    out = {n: v[order] for n, v in out.items()}
    out["dropped"] = sum(d["dropped"] for d in drains)
    return out


def _same_log(a, b, what, owned_flags=False):
    assert a["dropped"] == b["dropped"] == 0, what
    for n in PER_EPISODE + PER_AGENT:
        x, y = a[n], b[n]
        if n == "flags" and owned_flags:    # (CA_PLAN_VALID belongs to the pipelined policy query: unspecified in a record)
            x, y = _owned(x), _owned(y)
        assert x.shape == y.shape and torch.equal(x, y), "%s: %s" % (what, n)


def _episode(log, k, E):
    """episode k of every env out of a concatenated log -> dict of tensors indexed by env (every env must have one)"""
    m = log["episode"] == k
    env = log["env"][m]
    assert torch.equal(env, torch.arange(E, device=env.device)), "every env has exactly one record of episode %d" % k
    return {n: log[n][m] for n in PER_EPISODE + PER_AGENT}


def _latched(b):
    """what a record must hold, from a sim WITHOUT auto-reset, at this step: [E, N, 3] addends + the step count"""
    st = b.state
    return torch.stack([st["ep_reward"], st["t"], st["t"] - st["slt"]], dim=-1), st["episode_step"]


def _run_twin_latched(b, max_steps=8000):
    """step a twin WITHOUT auto-reset until every env is over; its state at its game over (Endings: obs = the addends,
    extra = episode_step)"""
    rec = Endings(b.E, 1)
    for s in range(max_steps):
        b.step()
        add, steps = _latched(b)
        rec.note(b.game_over, add, b.state["flags"], steps)
        if s % 25 == 24 and rec.all_have(1):
            break
    assert rec.all_have(1), "the twin's episodes did not end"
    return rec


def _outcome_of_kinds(flags):
    goal, coll, tout = _kinds(flags)
    assert bool((goal | coll | tout).all())
    return torch.where(coll, 0, torch.where(goal, 1, 2))


def _same_as_twin(ep, twin, what, case_want):
    assert torch.equal(ep["total_reward"], twin.obs[0][..., 0]), what + ": total_reward"
    assert torch.equal(ep["time_to_goal"], twin.obs[0][..., 1]), what + ": time_to_goal"
    assert torch.equal(ep["extra_time_to_goal"], twin.obs[0][..., 2]), what + ": extra_time_to_goal"
    assert torch.equal(_owned(ep["flags"]), _owned(twin.flags[0])), what + ": flag words"
    assert torch.equal(ep["steps"], twin.extra[0].to(torch.int64)), what + ": steps"
    assert torch.equal(ep["steps"], (twin.at[0] + 1).to(torch.int64)), what + ": steps vs the twin's step index"
    assert ep["case"].tolist() == list(case_want), what + ": case"
    assert torch.equal(ep["outcome"], _outcome_of_kinds(twin.flags[0])), what + ": outcome"


def _step_until(a, n_endings, capacity_drain_every=25, max_steps=8000):
    """step `a` (auto-reset, log on) one launch per step until every env has ended n_endings episodes, draining as it goes
    -> (log, headings [n_endings][E, N] every env starts its NEXT episode with)"""
    rec, drains = Endings(a.E, n_endings), []
    for s in range(max_steps):
        a.step()
        rec.note(a.game_over, a.rewards, a.state["flags"], a.state["heading"])
        if s % capacity_drain_every == capacity_drain_every - 1:
            drains.append(a.episodes())
            if rec.all_have(n_endings):
                break
    assert rec.all_have(n_endings)
    return _cat(drains), rec


# ---------------------------------------------------------------- 1. the twin without reset, bit for bit
def test_twin_without_reset_two_episodes_partly_filled_last_tile():
    nat, core, orc = _mods()
    seen = np.zeros(3, dtype=np.int64)
    batches = [   # (E, N, policies per slot, max_time_ratio): E is no multiple of the tile's env count (16 / 4 / 32 / 10)
        (301, 4, None, 1.25),
        (257, 10, None, 1.5),
        (203, 2, nat.POL_NONCOOP, 2.0),
        (241, 6, np.array([[nat.POL_RVO, nat.POL_NONCOOP, nat.POL_RVO, nat.POL_RVO, nat.POL_NONCOOP, nat.POL_RVO]]), 1.4),
    ]
    for E, N, pol, mtr in batches:
        table = gu.fixtures(N)
        C = table.shape[0]
        what = "E=%d N=%d" % (E, N)
        kw = dict(policy=pol, max_time_ratio=mtr)
        a = _sim(E, N, table, True, **kw)
        a.log_episodes(capacity=8)
        log, rec = _step_until(a, 2)
        assert _last_kernel().startswith("ca_pipe_kernel<%d, " % N) and _last_kernel().endswith(" log"), _last_kernel()
        assert a.E % int(_last_kernel().split(",")[1]) != 0, "the last tile is partly filled"
        assert log["dropped"] == 0
        ep0, ep1 = _episode(log, 0, E), _episode(log, 1, E)
        _same_as_twin(ep0, _run_twin_latched(_sim(E, N, table, False, **kw)), what + " first episode", np.arange(E) % C)
        c = _sim(E, N, table, False, offset=E, headings=rec.extra[0], **kw)    # (its first episode is A's second)
        _same_as_twin(ep1, _run_twin_latched(c), what + " second episode", (np.arange(E) + E) % C)
        for ep in (ep0, ep1):
            seen += np.bincount(ep["outcome"].cpu().numpy(), minlength=3)
        a.check_faults()
    assert (seen > 0).all(), "collision / all at goal / stuck endings seen: %s" % seen.tolist()


# ---------------------------------------------------------------- 2. every stepping path writes the same log, and nothing else
def test_every_path_writes_the_same_log_and_changes_nothing_else():
    E, N, T = 600, 10, 220
    table = gu.fixtures(N)
    OUT = ("obs", "rewards", "done", "game_over")
    STATE = ("pos_x", "pos_y", "heading", "t", "time_remaining", "step_num", "flags", "reset_count", "env_stats", "ep_reward")

    def start(log, **k2):
        s = _sim(E, N, table, True, max_time_ratio=1.5, **k2)
        s.rollout(37)            # (mid-episode, the first envs past their first auto-reset: the log starts at their count)
        if log:
            s.log_episodes(capacity=16)
        return s

    # one launch per step, log on against log off in lock step: outputs of every step, then the state
    off, on = start(False), start(True)
    drains = []
    for t in range(T):
        off.step()
        on.step()
        for n in OUT:
            assert torch.equal(getattr(on, n), getattr(off, n)), "log on vs off: %s @%d" % (n, t)
        if t in (50, 51, 140):
            drains.append(on.episodes())
    assert _last_kernel().startswith("ca_pipe_kernel<10, 4, false> grid=150 ") and _last_kernel().endswith(" log")
    drains.append(on.episodes())
    base = _cat(drains)
    base_state = {n: off.state[n].clone() for n in STATE}
    for n in STATE:
        assert torch.equal(on.state[n], base_state[n]), "log on vs off: state %s" % n
    assert base["dropped"] == 0 and int(base["env"].shape[0]) >= E // 2
    rc0 = start(False).state["reset_count"].to(torch.int64)
    assert int(base["env"].shape[0]) == int((base_state["reset_count"].to(torch.int64) - rc0).sum())

    # rollout(n) in uneven chunks
    s = start(True)
    drains = []
    for n in (1, 7, 1, 1, 30, 2, 50, 13, 45, 1, 1, 3, 20, 40, 5):
        s.rollout(n)
        if n in (30, 45, 5):
            drains.append(s.episodes())
    _same_log(_cat(drains), base, "rollout chunks")
    for n in STATE:
        assert torch.equal(s.state[n], base_state[n]), "rollout: state %s" % n

    # the look-ahead ring, with rewinds and drains in mid-ring
    s = start(True)
    s.enable_lookahead(16, fresh=True)
    drains = []
    for t in range(T):
        s.step_lookahead()
        if (t + 1) in (5, 70, 131):
            assert 0 < s._la["t"] < s._la["len"]
            s.sync()                                   # a rewind in mid-ring: the replay rewrites records that are there
        if (t + 1) in (23, 90, 91, 200):
            assert 0 < s._la["t"] < s._la["len"]
            rewinds = s._la["rewinds"]
            drains.append(s.episodes())                # a drain in mid-ring
            assert s._la["rewinds"] == rewinds and s._la["slots"] is not None
    assert _last_kernel().startswith("ca_pipe_kernel<10, 4, true>") and _last_kernel().endswith(" log"), _last_kernel()
    assert s._la["rewinds"] >= 3
    s.sync()
    drains.append(s.episodes())
    _same_log(_cat(drains), base, "ring")
    for n in STATE:
        assert torch.equal(s.state[n], base_state[n]), "ring: state %s" % n

    # the unpipelined kernel
    s = start(True, pipeline=False)
    for t in range(T):
        s.step()
    assert _last_kernel().startswith("ca_kernel<")
    _same_log(_cat([s.episodes()]), base, "ca_kernel", owned_flags=True)
    s.check_faults()


# ---------------------------------------------------------------- 3. every kernel family
def _maps_stack():
    m = np.zeros((3, 160, 160), dtype=bool)
    m[0, 10:150, 78:82] = True     # a wall along x = 0
    m[1, 78:82, 10:150] = True     # a wall along y = 0
    return m                       # (map 2: empty)


FAMILIES = {
    # against = "general": the same batch, pipeline=False, one launch per step; "twin": latched state of a twin without reset
    "ragged_pipelined": dict(case="ragged", against="general"),
    "ragged_general": dict(case="ragged_general", against="twin"),
    "random_headings": dict(case="random_headings", against="twin"),
    "closest_last": dict(case="closest_last", against="twin"),
    "map_set": dict(case="static_map", against="general", maps=True),
}


def _family_sim(c, auto_reset, maps=False, pipeline=None, **over):
    E, N = c["E"], c["N"]
    table = _ragged_table(N) if c.get("table") == "ragged" else gu.fixtures(N)
    kw = dict(max_time_ratio=1.5)
    kw.update(c.get("kw", {}))
    kw.update(over)
    s = _sim(E, N, table, auto_reset, heading_seed=c.get("heading_seed", 0) if auto_reset else 0,
             pipeline=c.get("pipeline", True) if pipeline is None else pipeline, **kw)
    if maps:
        s.set_map(_maps_stack(), num_beams=8, num_to_store=1, env_map=np.arange(E) % 3, map_seed=0)
        s.set_map_seed(12345)
    return s, table


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_every_kernel_family_writes_the_log(name):
    f = FAMILIES[name]
    c = CASES[f["case"]]
    E = c["E"]
    a, table = _family_sim(c, True, maps=f.get("maps", False))
    a.log_episodes(capacity=8)
    log, rec = _step_until(a, 2)
    k = _last_kernel()
    assert k.startswith(c["kernel"]), k
    assert k.endswith(" log") == k.startswith("ca_pipe_kernel"), k
    assert log["dropped"] == 0
    if f["against"] == "general":
        b, _ = _family_sim(c, True, maps=f.get("maps", False), pipeline=False)
        b.log_episodes(capacity=8)
        drains = []
        for s in range(rec.steps):
            b.step()
            if s % 25 == 24:
                drains.append(b.episodes())
        assert _last_kernel().startswith("ca_kernel<")
        drains.append(b.episodes())
        _same_log(log, _cat(drains), name, owned_flags=True)
        if f.get("maps"):
            assert torch.equal(a.env_map, b.env_map) and len(set(a.env_map.tolist())) == 3
    else:
        twin, _ = _family_sim(c, False)
        _same_as_twin(_episode(log, 0, E), _run_twin_latched(twin), name, np.arange(E) % table.shape[0])
        ep1 = _episode(log, 1, E)
        assert ep1["case"].tolist() == list((np.arange(E) + E) % table.shape[0])
        from gym_collision_avoidance_amd import episodes as eplog
        assert torch.equal(ep1["outcome"], eplog.outcome_of(ep1["flags"]))
    if c.get("table") == "ragged":
        ep0 = _episode(log, 0, E)
        absent = (ep0["flags"] & (1 << 16)) != 0
        want = torch.from_numpy(table[np.arange(E) % table.shape[0], :, 5] <= 0).to(absent.device)
        assert torch.equal(absent, want) and bool(absent.any())
    a.check_faults()


def test_large_env_kernel_writes_the_log():
    """6 x 70 on a make_testcase_huge table (the one-thread-per-agent kernel of cagpu_big.inc), as
    test_large_env_kernel_keeps_the_record builds it"""
    nat, core, orc = _mods()
    from gym_collision_avoidance_amd.envs import test_cases as tc
    E, N, K, C = 6, 70, 19, 18
    rng = np.random.default_rng(11)
    np.random.seed(71)
    table = tc.make_testcase_huge(C, N, side_length=2.0 * np.sqrt(N) + 3.0, speed_bnds=[0.5, 1.5], radius_bnds=[0.2, 0.5])
    pol = rng.choice([nat.POL_RVO, nat.POL_RVO, nat.POL_NONCOOP, nat.POL_STATIC], (1, N)).astype(np.int32)
    kw = dict(policy=pol, max_obs=K, max_time_ratio=0.3)
    a = _sim(E, N, table, True, **kw)
    a.log_episodes(capacity=4)
    log, rec = _step_until(a, 2, capacity_drain_every=10, max_steps=3000)
    assert _last_kernel().startswith("ca_big_kernel")
    assert log["dropped"] == 0
    _same_as_twin(_episode(log, 0, E), _run_twin_latched(_sim(E, N, table, False, **kw)), "big first episode", np.arange(E) % C)
    c = _sim(E, N, table, False, offset=E, headings=rec.extra[0], **kw)
    _same_as_twin(_episode(log, 1, E), _run_twin_latched(c), "big second episode", (np.arange(E) + E) % C)
    # rollout(n) of the large-env kernel is n launches: the same log
    b = _sim(E, N, table, True, **kw)
    b.log_episodes(capacity=16)
    b.rollout(rec.steps)
    _same_log(_cat([b.episodes()]), log, "big rollout")


# ---------------------------------------------------------------- 4. the records add up to env_stats, bit for bit
def test_the_records_add_up_to_env_stats():
    E, N = 257, 10
    s = _sim(E, N, gu.fixtures(N), True, max_time_ratio=1.5)
    s.log_episodes(capacity=16)
    drains = []
    for _ in range(6):
        s.rollout(150)
        drains.append(s.episodes())
    log = _cat(drains)
    assert log["dropped"] == 0 and int(log["env"].shape[0]) > 2 * E
    stats = s.state["env_stats"].cpu().numpy()
    env, oc, steps = (log[n].cpu().numpy() for n in ("env", "outcome", "steps"))
    per = [log[n].cpu().numpy() for n in ("total_reward", "time_to_goal", "extra_time_to_goal")]
    want = np.zeros((E, 8))
    for i in range(env.shape[0]):       # (sequential float64 adds, in episode order and agent order: the kernel's own)
        st = want[env[i]]
        st[0] += 1.0
        st[1 + oc[i]] += 1.0
        st[4] += float(steps[i])
        for j, col in enumerate(per):
            tot = 0.0
            for a in range(N):
                tot += float(col[i, a])
            st[5 + j] += tot
    assert np.array_equal(want, stats)
    # the same with cumsum (sequential as well), vectorised over the records
    tot = [np.cumsum(col, axis=1)[:, -1] for col in per]
    for e in (0, 100, E - 1):
        m = env == e
        for j in range(3):
            assert np.cumsum(tot[j][m])[-1] == stats[e, 5 + j]


# ---------------------------------------------------------------- 5. overflow is counted
def test_overflow_is_counted_not_silent():
    nat, core, orc = _mods()
    E, N = 203, 2
    table = gu.fixtures(N)
    kw = dict(policy=nat.POL_NONCOOP, max_time_ratio=2.0)
    small, big = _sim(E, N, table, True, **kw), _sim(E, N, table, True, **kw)
    small.log_episodes(capacity=2)
    big.log_episodes(capacity=64)
    for _ in range(40):
        small.rollout(100)
        big.rollout(100)
        if int(small.state["reset_count"].min()) >= 5:
            break
    rc = small.state["reset_count"].to(torch.int64)
    assert int(rc.min()) >= 5 and int(rc.max()) <= 64 and torch.equal(rc, big.state["reset_count"].to(torch.int64))
    got, full = small.episodes(), big.episodes()
    assert full["dropped"] == 0 and int(full["env"].shape[0]) == int(rc.sum())
    assert got["dropped"] == int((rc - 2).clamp(min=0).sum()) > 0
    newest = full["episode"] >= (rc - 2)[full["env"]]
    assert int(newest.sum()) == 2 * E
    for n in PER_EPISODE + PER_AGENT:
        assert torch.equal(got[n], full[n][newest]), n
    # ... and a second drain finds nothing new and nothing lost
    again = small.episodes()
    assert again["dropped"] == 0 and int(again["env"].shape[0]) == 0


# ---------------------------------------------------------------- 6. a drain in mid-ring neither rewinds nor sees the future
def test_ring_drain_without_rewind():
    E, N = 257, 10
    s = _sim(E, N, gu.fixtures(N), True, max_time_ratio=1.5)
    s.rollout(120)
    s.log_episodes(capacity=32)
    s.enable_lookahead(20, fresh=True)
    handed = torch.zeros((E,), dtype=torch.int64, device=s.device)
    total = 0
    for t in range(1, 96):
        over = s.step_lookahead()[3]
        handed += over.to(torch.int64)
        if t in (7, 13, 20, 27, 39, 40, 55, 95):
            la = s._la
            fills, rewinds, at = la["fills"], la["rewinds"], la["t"]
            ep = s.episodes()
            assert ep["dropped"] == 0
            assert torch.equal(torch.bincount(ep["env"], minlength=E), handed), "records per env @%d" % t
            assert s._la["rewinds"] == rewinds == 0 and s._la["fills"] == fills and s._la["t"] == at
            assert s._la["slots"] is not None
            total += int(handed.sum())
            handed.zero_()
            if at < la["len"]:      # the following slot is still served from the same ring
                s.step_lookahead()
                handed += s._la["ring"][3][at].to(torch.int64)
                assert s._la["fills"] == fills and s._la["t"] == at + 1
    assert total > E // 4
    assert s._la["rewinds"] == 0


# ---------------------------------------------------------------- 7. off means off
def test_off_means_off_on_the_bench_geometry():
    E, N = 4096, 10
    s = _sim(E, N, gu.fixtures(N), True)
    s.enable_lookahead(20, fresh=True)
    for _ in range(40):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.log_episodes()
    s.enable_lookahead(20, fresh=True)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL + " log"      # the same selection, grid and block
    s.log_episodes(on=False)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.sync()
    s.step()
    assert _last_kernel() == PARENT_BENCH_KERNEL.replace("true", "false").replace(" fair", "")
    s.check_faults()


# ---------------------------------------------------------------- 8. the reference's suite through the log
@pytest.mark.parametrize("name", ["n4", "ragged4", "n10"])
def test_reference_suite_outcomes_through_the_log(name):
    """test_reference_suite_outcomes of tests/test_gpu_parity.py -- every assertion, threshold and its one exclusion --
    with 50 auto-resetting envs walking the 500 cases instead of one env per case stepped from the host: rollout(500)
    chunks, a drain after each, the first record of every case.  The final positions that test compares are not part of
    a record; they are read off the trajectory tape recorded beside the log (the last row of every agent in the episode)."""
    nat, core, orc = _mods()
    ref = gu.load_suite(name)
    cases = gu.suite_cases(name)
    C, N = cases.shape[:2]
    E = 50
    g = core.BatchedSim(core.make_params(E, N, ragged=int(name == "ragged4")))
    g.set_plugins(nat.POL_RVO)
    g.set_fixture_table(cases, case_stride=E)
    g.log_episodes(capacity=128)
    g.record_trajectories()
    g.reset_from_table()
    K = C // E
    got = dict(outcome=np.full(C, -1), steps=np.zeros(C, np.int64), time_to_goal=np.zeros((C, N)),
               flags=np.zeros((C, N), np.uint32), pos=np.zeros((C, N, 2)), absent=np.zeros(C, np.int64))
    pos = np.zeros((E, K + 1, N, 2))       # the last position every agent moved to in episode k of env e
    idx = np.arange(E)
    dropped = 0
    for _ in range(40):
        g.rollout(500)
        tape = g.trajectories()
        rows, epi = tape["rows"].cpu().numpy(), tape["episode"].cpu().numpy()
        g.clear_trajectories()
        for i in range(rows.shape[0]):
            k = np.minimum(epi[i], K)
            moved = rows[i, :, :, 11] >= 0
            cur = pos[idx, k]
            cur[moved] = rows[i, :, :, 1:3][moved]
            pos[idx, k] = cur
        ep = g.episodes()
        dropped += ep["dropped"]
        ep = {n: v.cpu().numpy() for n, v in ep.items() if n != "dropped"}
        for i in range(ep["env"].shape[0]):
            c = int(ep["case"][i])
            if got["outcome"][c] >= 0:
                continue                    # (the first record of a case)
            f = ep["flags"][i].astype(np.uint32)
            here = (f >> 16 & 1) == 0
            got["outcome"][c] = ep["outcome"][i]
            got["steps"][c] = ep["steps"][i]
            got["time_to_goal"][c] = ep["time_to_goal"][i] * here
            got["flags"][c] = (f & 0x3F) * here
            got["absent"][c] = (~here).sum()
            got["pos"][c] = pos[ep["env"][i], ep["episode"][i]] * here[:, None]
            assert c == (ep["env"][i] + ep["episode"][i] * E) % C
        if (got["outcome"] >= 0).all():
            break
    assert dropped == 0
    assert (got["outcome"] >= 0).all(), "%d cases without a record" % int((got["outcome"] < 0).sum())
    if name == "ragged4":
        assert np.array_equal(got["absent"], 4 - ref["num_agents"])
    swap = _swap_cases(cases)
    same = (got["outcome"] == ref["outcome"]) & (got["steps"] == ref["steps"]) & (got["flags"] == ref["flags"]).all(1) & \
           (np.abs(got["time_to_goal"] - ref["time_to_goal"]).max(1) < 1e-6) & \
           (np.abs(got["pos"] - ref["pos"]).max((1, 2)) < 1e-3)
    assert same[~swap].all(), "cases %s differ from the reference without an exact swap in them" % np.nonzero(~same & ~swap)[0][:20]
    assert same.mean() > 0.9
    for oc in range(3):
        assert abs(int((got["outcome"] == oc).sum()) - int((ref["outcome"] == oc).sum())) <= 12, (oc, got["outcome"], ref["outcome"])
    assert abs(got["steps"].mean() - ref["steps"].mean()) < 0.05 * ref["steps"].mean()


# ---------------------------------------------------------------- 9. the env API and the suite runner
def test_env_api_episode_log():
    Config, tc, Env = envtools.fresh("Hist4")
    try:
        Config.MAX_TIME_RATIO = 1.3
        E, N = 96, 4

        def make(auto_reset=True, log=True, lookahead=None):
            env = Env(num_envs=E, lookahead=lookahead)
            env.set_fixture_suite(N, policies="RVO", auto_reset=auto_reset)
            if log:
                env.log_episodes()            # before reset(): survives it
            env.reset()
            return env

        # refusals
        with pytest.raises(ValueError, match="auto_reset"):
            make(auto_reset=False)
        with pytest.raises(ValueError, match="batched"):
            Env().log_episodes()
        env = Env(num_envs=E)
        env.set_agents([tc.get_testcase_two_agents(policies=("RVO", "RVO")) for _ in range(E)])
        with pytest.raises(ValueError, match="set_fixture_suite"):
            env.log_episodes()
        with pytest.raises(RuntimeError, match="log_episodes"):
            make(log=False).episode_log()

        # off by default: exactly today's return values; on: the same return values
        plain, env = make(log=False), make()
        assert env._sim._log is not None and env._sim._la is not None
        n_over = torch.zeros((E,), dtype=torch.int64, device=env._sim.device)
        for _ in range(150):
            a, b = env.step(None), plain.step(None)
            assert a[3] is False and sorted(a[4]) == sorted(b[4]) == ["which_agents_done", "which_agents_learning"]
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
            n_over += a[2].to(torch.int64)
        rewinds = env._sim._la["rewinds"]
        log = env.episode_log()
        assert env._sim._la["rewinds"] == rewinds, "reading the log must not rewind the ring"
        M = int(n_over.sum())
        assert M > E // 2 and log["dropped"] == 0
        want = {"env": np.int64, "episode": np.int64, "test_case": np.int64, "num_agents": np.int64, "steps": np.int64,
                "total_reward": np.float64, "time_to_goal": np.float64, "extra_time_to_goal": np.float64,
                "total_time_to_goal": np.float64, "collision": np.bool_, "all_at_goal": np.bool_, "any_stuck": np.bool_,
                "outcome": np.object_}
        assert sorted(log) == sorted(list(want) + ["dropped"]) and isinstance(log["dropped"], int)
        for n, dt in want.items():
            assert isinstance(log[n], np.ndarray) and log[n].dtype == dt, n
            assert log[n].shape == ((M, N) if n in ("total_reward", "time_to_goal", "extra_time_to_goal") else (M,)), n
        assert np.array_equal(np.bincount(log["env"], minlength=E), n_over.cpu().numpy())
        assert set(log["outcome"]) <= {"collision", "all_at_goal", "stuck"} and len(set(log["outcome"])) >= 2
        assert np.array_equal(log["test_case"], (log["env"] + log["episode"] * E) % 500)
        assert (log["num_agents"] == N).all() and (log["steps"] > 0).all()
        assert np.array_equal(log["collision"], log["outcome"] == "collision")
        assert np.array_equal(log["all_at_goal"], log["outcome"] == "all_at_goal")
        assert np.array_equal(log["any_stuck"] | log["collision"], log["outcome"] != "all_at_goal")
        # rollout() logs as well; reset() keeps the log on and starts the count again
        env.rollout(60)
        assert env.episode_log()["dropped"] == 0
        env.reset()
        assert env._sim._log is not None and len(env.episode_log()["env"]) == 0
        env.log_episodes(False)
        assert env._sim._log is None
        out = env.step(None)
        assert out[3] is False and sorted(out[4]) == ["which_agents_done", "which_agents_learning"]
    finally:
        envtools.default()


SUITE_COLUMNS = ("num_agents", "policy", "test_case", "total_reward", "steps", "time_to_goal", "total_time_to_goal",
                 "extra_time_to_goal", "collision", "all_at_goal", "any_stuck", "outcome")


def test_run_suite_logged_equals_run_suite():
    Config, tc, Env = envtools.fresh("FullTestSuite")
    try:
        import importlib
        rs = importlib.import_module("gym_collision_avoidance_amd.experiments.run_full_test_suite")
        a, b = rs.run_suite_logged("RVO", 4, range(24)), rs.run_suite("RVO", 4, range(24))
        assert tuple(a.columns) == tuple(b.columns) == SUITE_COLUMNS and len(a) == len(b) == 24
        for col in SUITE_COLUMNS:
            x, y = a[col].tolist(), b[col].tolist()
            if col in ("total_reward", "time_to_goal", "extra_time_to_goal"):
                x, y = np.stack(x), np.stack(y)
            assert np.array_equal(np.asarray(x), np.asarray(y)), col
        # fewer envs than cases: one row per case in case order; the cases that are the first episode of their env are the
        # same rows (later episodes start at an on-device auto-reset: the device's own arctan2 for the initial heading)
        c = rs.run_suite_logged("RVO", 4, range(24), num_envs=5)
        assert len(c) == 24 and c["test_case"].tolist() == list(range(24)) and set(c["outcome"]) <= {"collision", "all_at_goal", "stuck"}
        for col in ("steps", "outcome", "total_time_to_goal"):
            assert c[col].tolist()[:5] == b[col].tolist()[:5], col
        assert np.array_equal(np.stack(c["total_reward"].tolist()[:5]), np.stack(b["total_reward"].tolist()[:5]))
        # the GA3C-CADRL network between the steps (the general kernel, closest_last sorting)
        a, b = rs.run_suite_logged("GA3C-CADRL-10", 3, range(12)), rs.run_suite("GA3C-CADRL-10", 3, range(12))
        assert len(a) == 12 and a["outcome"].tolist() == b["outcome"].tolist() and a["test_case"].tolist() == list(range(12))
    finally:
        envtools.default()
