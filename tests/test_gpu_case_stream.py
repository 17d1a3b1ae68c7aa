"""The case stream (include/cagpu.h CaCaseStream, cagpu_generate_cases_at, cagpu_stream_refill; core.BatchedSim
.set_case_stream; set_fixture_suite(generate=dict(stream=True, ...))): a fresh random scenario at every on-device
auto-reset.

A scenario is a pure function of (seed, global env id, episode), so every comparison of a stream with something else is
EXACT: the wave-per-case generator against the one-thread-per-case generator, a stream against a twin that runs on a
plain fixture table holding the same scenarios, and one stream driven four ways (single steps, rollouts, a look-ahead ring
with rewinds, two shards).  Only the comparison with the HOST generator has the room of the existing one
(tests/test_gpu_parity.py::test_device_scenarios_match_host_generator): the two libms differ by an ulp.

The stream tests draw short trips under a small max_time_ratio: every episode ends within about two dozen steps."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import case_stream_ref as ref  # noqa: E402
from tests import envtools  # noqa: E402
from tests import golden_util as gu  # noqa: E402
from tests.test_gpu_final_obs import PARENT_BENCH_KERNEL, _last_kernel  # noqa: E402
from tests.test_gpu_final_obs import _sim as _fixture_sim  # noqa: E402
from tests.test_gpu_parity import _mods  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0x5712EA4D
# short trips: a small square, fast agents, thin discs (the generator's own distribution arguments)
SHORT = dict(side_length=[{"num_agents": [0, 3], "side_length": [1.0, 1.5]}, {"num_agents": [3, 100], "side_length": [1.5, 2.0]}],
             speed_bnds=(1.5, 2.0), radius_bnds=(0.15, 0.25))
STATE = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed", "time_remaining", "t",
         "slt", "ep_reward", "last_action", "step_num", "episode_step", "flags", "reset_count", "env_stats")


def _gen_sim(N, ragged=0):
    _, core, _ = _mods()
    return core.BatchedSim(core.make_params(2, N, ragged=ragged))


# ---------------------------------------------------------------- 1. generator against generator
# the three configurations of the comparison; C = 96 cases each.  The crowded one draws LARGE discs (radius 4 .. 8 m in a
# square of half side 4 m): with the reference's default radii the square's 1 % growth per attempt makes room within
# about 40 attempts at any N (measured on the host restatement: at most 42 of a rand-family agent, 9 of a circle agent,
# over seeds 1 - 3 of all three configurations), so no seed reaches the second batch of 64 speculative attempts
GEN_CONFIGS = {
    "n2": dict(N=2, seed=1, kw=dict(side_length=4.0)),
    "ragged10": dict(N=10, seed=1, kw=dict(side_length=ref.REF_SIDE, num_agents=(2, 10))),
    "crowded20": dict(N=20, seed=1, kw=dict(side_length=4.0, radius_bnds=(4.0, 8.0))),
}
_host_cache = {}


def _host(name):
    """the host restatement of a configuration's 96 cases (computed once per session)"""
    if name not in _host_cache:
        c = GEN_CONFIGS[name]
        kw = c["kw"]
        _host_cache[name] = ref.host_cases_at(c["seed"], range(96), c["N"], kw["side_length"],
                                              radius=kw.get("radius_bnds", (0.2, 0.8)), num_agents=kw.get("num_agents"))
    return _host_cache[name]


@pytest.mark.parametrize("name", list(GEN_CONFIGS))
def test_generate_at_equals_the_one_thread_generator(name):
    """generate_cases_at(arange(C)) == generate_cases / generate_cases_ragged for the same seed -- cases, counts and
    status, array_equal -- on inputs that, by the host restatement, hold all three families and (the crowded
    configuration) an agent past its 128th attempt in the rand family and past its 11th in a circle / swap case: the second
    and third batch of 64 speculative attempts, and the circle's growth, are exercised"""
    c = GEN_CONFIGS[name]
    C_, N, kw = 96, c["N"], c["kw"]
    _, _, kinds, attempts = _host(name)
    fam, rand_max, circ_max = ref.coverage(kinds, attempts)
    print(name, "families", sorted(fam), "most attempts: rand", rand_max, "circle / swap", circ_max)
    assert fam == {"swap", "circle", "rand"}
    if name == "crowded20":
        assert rand_max > 128 and circ_max > 11, (rand_max, circ_max)
    g = _gen_sim(N, ragged=int("num_agents" in kw))
    want, w_status, w_counts = g.generate_cases(C_, c["seed"], return_status=True, return_counts=True, **kw) \
        if "num_agents" in kw else g.generate_cases(C_, c["seed"], return_status=True, **kw) + (None,)
    got, g_status, g_counts = g.generate_cases_at(np.arange(C_), c["seed"], return_status=True, return_counts=True, **kw)
    torch.cuda.synchronize()
    differ = int((got != want).reshape(C_, -1).any(dim=1).sum())
    print(name, "cases that differ:", differ, "of", C_)
    assert torch.equal(got, want), "%d of %d cases differ" % (differ, C_)
    assert torch.equal(g_status, w_status) and not bool(g_status.any())
    if w_counts is not None:
        assert torch.equal(g_counts, w_counts)
        assert np.array_equal(g_counts.cpu().numpy(), _host(name)[1])
    else:
        assert bool((g_counts == N).all())


# ---------------------------------------------------------------- 2. arbitrary 64-bit indices
def test_arbitrary_indices_against_the_host_generator():
    """indices (g << 32) | k with g up to 2^31 and scattered rows against the host generator under Philox (which takes
    64-bit case indices): the rule of test_device_scenarios_match_host_generator, at least 97 % within 1e-9; a device-side
    count below M leaves the other rows untouched; a shuffled list gives the same rows"""
    N, M, R = 10, 96, 131
    rng = np.random.default_rng(7)
    gs = np.concatenate([[0, 1, 2 ** 31, 2 ** 31 - 1, 2 ** 16], rng.integers(0, 2 ** 31 + 1, M - 5)]).astype(np.int64)
    ks = np.concatenate([[0, 2 ** 31 - 1, 5, 77, 2 ** 20], rng.integers(0, 2 ** 31, M - 5)]).astype(np.int64)
    idx = (gs << 32) | ks
    assert len(set(idx.tolist())) == M and int(idx.max()) >= 2 ** 63 - 2 ** 33
    rows = rng.permutation(R)[:M].astype(np.int64)
    kw = dict(side_length=ref.REF_SIDE, num_agents=(2, 10))
    g = _gen_sim(N, ragged=1)
    out = torch.full((R, N, 6), -7.0, dtype=torch.float64, device=g.device)
    got, status, counts = g.generate_cases_at(idx, SEED, out=out, out_row=rows, return_status=True, return_counts=True, **kw)
    torch.cuda.synchronize()
    assert got is out
    got_np = got.cpu().numpy()
    want, w_counts, kinds, _ = ref.host_cases_at(SEED, idx.tolist(), N, kw["side_length"], num_agents=kw["num_agents"])
    assert set(kinds) == {"swap", "circle", "rand"} and not bool(status.any())
    same = np.abs(got_np[rows] - want).reshape(M, -1).max(axis=1) <= 1e-9
    print("cases within 1e-9 of the host generator:", int(same.sum()), "of", M)
    assert same.mean() >= 0.97, (same.mean(), [k for k, s_ in zip(kinds, same) if not s_])
    assert np.array_equal(counts.cpu().numpy()[rows], w_counts)
    untouched = np.setdiff1d(np.arange(R), rows)
    assert (got_np[untouched] == -7.0).all()
    # a shuffled list: the same rows, bit for bit
    perm = rng.permutation(M)
    again = g.generate_cases_at(idx[perm], SEED, out=torch.full_like(out, -7.0), out_row=rows[perm], **kw)
    assert torch.equal(again, got)
    # ... and a device-side count: the first 40 entries only
    count = torch.tensor([40], dtype=torch.int32, device=g.device)
    part = g.generate_cases_at(idx, SEED, out=torch.full_like(out, -7.0), out_row=rows, count=count, **kw).cpu().numpy()
    assert np.array_equal(part[rows[:40]], got_np[rows[:40]])
    assert (part[np.setdiff1d(np.arange(R), rows[:40])] == -7.0).all()
    # row m without out_row; a count above M is M
    plain = g.generate_cases_at(idx[:9], SEED, count=torch.tensor([1000], dtype=torch.int32, device=g.device), **kw)
    assert torch.equal(plain, got[torch.as_tensor(rows[:9], device=g.device)])


# ---------------------------------------------------------------- the stream batches
def _stream_sim(E, N, W, offset=0, seed=SEED, pipeline=True, heading_seed=0x4EAD, draw=True, dist=None, num_agents="ragged",
                policy=None, **kw):
    nat, core, _ = _mods()
    na = (2, N) if num_agents == "ragged" else num_agents
    kw.setdefault("max_time_ratio", 1.5)
    s = core.BatchedSim(core.make_params(E, N, ragged=int(na is not None), **kw), pipeline=pipeline)
    s.set_plugins(nat.POL_RVO if policy is None else policy)
    s.set_case_stream(window=W, seed=seed, num_agents=na, heading_seed=heading_seed, env_id_offset=offset,
                      **(SHORT if dist is None else dist))
    if draw:
        s.set_policy_draw([core.policy_word_bits(nat.POL_RVO), core.policy_word_bits(nat.POL_NONCOOP),
                           core.policy_word_bits(nat.POL_STATIC)], [0.6, 0.3, 0.1], seed=0xD1CE)
    s.reset_from_stream()
    return s


def _scenarios(s, E, K, offset=0, seed=SEED, dist=None, num_agents="ragged"):
    """[E, K, N, 6]: scenario (g, k) of every env and the first K episodes, by generate_cases_at itself"""
    na = (2, s.N) if num_agents == "ragged" else num_agents
    g = np.arange(E, dtype=np.int64)[:, None] + offset
    idx = ((g << 32) | np.arange(K, dtype=np.int64)[None, :]).reshape(-1)
    t = s.generate_cases_at(idx, seed, num_agents=na, **(SHORT if dist is None else dist))
    return t.reshape(E, K, s.N, 6)


# ---------------------------------------------------------------- 3. stream content
def test_every_auto_reset_loads_its_own_scenario():
    """E = 67, N = 4, ragged 2 .. 4, W = 3, random headings, a policy draw: after every one of 400 single steps each env
    whose game_over is set stands on row (g << 32) | reset_count[e] of generate_cases_at -- start positions, goals, radii,
    preferred speeds exactly, CA_ABSENT where the row is empty"""
    nat = _mods()[0]
    E, N, W, K = 67, 4, 3, 160
    s = _stream_sim(E, N, W)
    want = _scenarios(s, E, K)
    ar = torch.arange(E, device=s.device)

    def check(envs, what):
        rc = s.state["reset_count"].to(torch.int64)
        assert int(rc.max()) < K
        rows = want[ar, rc]                                      # [E, N, 6]
        present = rows[..., 5] > 0
        for col, name in enumerate(("pos_x", "pos_y", "goal_x", "goal_y", "pref_speed", "radius")):
            a, b = s.state[name][envs], rows[..., col][envs]
            assert torch.equal(torch.where(present[envs], a, b), b), (what, name)
        assert torch.equal((s.state["flags"][envs] & nat.ABSENT) != 0, ~present[envs]), what
        return rc
    check(ar, "episode 0")
    resets = 0
    for step in range(400):
        s.step()
        over = s.game_over.bool()
        if bool(over.any()):
            resets += int(over.sum())
            rc = check(over.nonzero().reshape(-1), "step %d" % step)
    s.check_faults()
    print("auto-resets checked:", resets, "deepest episode:", int(rc.max()))
    assert int(rc.max()) >= 2 * W and int(rc.min()) >= 1


# ---------------------------------------------------------------- 4. the stream is an infinite table
def _twin(s, E, K, **kw):
    """the same batch on a PLAIN fixture table of E * K rows, row e + k * E = scenario (g, k), case_stride = E, with
    reset_obs / reset_plan NULL like the stream's (an env that reset re-senses and is queried at the start of its step)"""
    t = _stream_sim(E, s.N, 1, **kw)       # (the same construction; its stream is replaced by the table below)
    table = _scenarios(s, E, K, **{k_: v for k_, v in kw.items() if k_ in ("dist", "num_agents", "seed")})
    table = table.permute(1, 0, 2, 3).reshape(E * K, s.N, 6).contiguous()
    draw = t._draw
    t.set_fixture_table(table, env_id_offset=0, case_stride=E, heading_seed=kw.get("heading_seed", 0x4EAD))
    t._ar.reset_obs, t._ar.reset_plan = None, None
    assert t._cstream is None and (t._draw is draw)
    t.reset(table[:E])
    return t


def _same_state(a, b, what=""):
    assert torch.equal(a.state["reset_count"], b.state["reset_count"]), what
    assert torch.equal(a._slab, b._slab), "state slab " + what
    for x, y, n in ((a.obs, b.obs, "obs"), (a.rewards, b.rewards, "rewards"), (a.done, b.done, "done"),
                    (a.game_over, b.game_over, "game_over")):
        assert torch.equal(x, y), n + " " + what


@pytest.mark.parametrize("name", ["pipelined", "general", "large70"])
def test_stream_equals_a_table_of_the_same_scenarios(name):
    """the stream (W = 3) against a twin on a fixture table that holds scenario (g, k) in row e + k * E, K larger than any
    reset_count reached: state slab, outputs, env_stats and the episode log's rows (`case` modulo the window) bit for bit.
    "pipelined": a sim built with pipeline=True (CaState.next_action handed over, plans kept in the slab) against
    "general" without it.  With reset_obs NULL -- a stream's, like a table's under heading_seed != 0 -- the library
    launches ca_kernel for both: ca_pipe_kernel resets an env only by copying its reset_obs row (pipe_eligible)."""
    if name == "large70":
        # (70 agents cross tens of metres -- the circle family's radius is N / 2 -- so the episodes are ended by a tiny
        # max_time_ratio instead: everybody runs out of time within about two dozen steps)
        E, N, W, K, steps = 3, 70, 3, 80, 150
        kw = dict(num_agents=None, draw=False, max_time_ratio=0.05,
                  dist=dict(side_length=6.0, speed_bnds=(1.5, 2.0), radius_bnds=(0.1, 0.15)))
    else:
        E, N, W, K, steps = 67, 4, 3, 60, 150
        kw = dict(pipeline=name == "pipelined")
    s = _stream_sim(E, N, W, **kw)
    t = _twin(s, E, K, **kw)
    for b in (s, t):
        b.log_episodes(capacity=K)
    _same_state(s, t, "after the reset")
    for step in range(steps):
        s.step(), t.step()
        if step % 10 == 9 or step == steps - 1:
            _same_state(s, t, "after step %d" % step)
    top = int(s.state["reset_count"].max())
    print(name, "deepest episode", top, "kernel", _last_kernel())
    assert W < top < K, top
    assert torch.equal(s.state["env_stats"], t.state["env_stats"])
    hs, ht = s._log["head"].clone(), t._log["head"].clone()
    valid = ht[..., 0] >= 0
    assert bool(valid.any())
    ht[..., 2] = torch.where(valid, ht[..., 2] % (E * W), ht[..., 2])
    assert torch.equal(hs, ht) and torch.equal(s._log["rows"], t._log["rows"])
    s.check_faults()


# ---------------------------------------------------------------- 5. launch patterns and shards
def _record(s):
    s.log_episodes(capacity=64)
    s.record_trajectories()
    return s


def _log_bytes(s):
    """the log's records of the episodes HANDED OUT (a ring that ran ahead has logged later ones as well), others blanked"""
    rc = s.state["reset_count"]
    assert int(rc.max()) < 64
    head, rows = s._log["head"], s._log["rows"]
    valid = (head[..., 0] >= 0) & (head[..., 0] < rc[:, None])
    return (torch.where(valid.unsqueeze(-1), head, torch.full_like(head, -1)),
            torch.where(valid[..., None, None], rows, torch.zeros_like(rows)))


def _tape(s):
    tr = s.trajectories()
    moved = tr["rows"][..., 11] >= 0
    return tr["rows"][..., 11], torch.where(moved.unsqueeze(-1), tr["rows"], torch.zeros_like(tr["rows"])), tr["episode"]


@pytest.mark.parametrize("W,ring", [(2, dict(k=2)), (8, dict(k=20, adaptive=True))])
def test_launch_patterns_and_shards_see_one_stream(W, ring):
    """the same stream as single steps, as rollout() chunks of uneven lengths, through the look-ahead ring with `state`
    read mid-ring at irregular steps (rewinds), and as two shards (30 + 37 envs): identical state, outputs, episode-log
    bytes and trajectory tape.  (The log's `case` is the window row, which depends on the shard's own size: the shards
    are compared without it.)"""
    E, N, T = 67, 4, (96 if W == 2 else 208)     # (long enough for the deepest env to wrap its window)
    single = _record(_stream_sim(E, N, W))
    for _ in range(T):
        single.step()
    roll = _record(_stream_sim(E, N, W))
    chunks, left = ([1, 2] if W == 2 else [3, 7, 1, 8, 5]), T
    i = 0
    while left:
        n = min(left, chunks[i % len(chunks)])
        roll.rollout(n)
        left, i = left - n, i + 1
    la = _record(_stream_sim(E, N, W))
    la.enable_lookahead(ring["k"], fresh=True, adaptive=ring.get("adaptive", False))
    looks = 0
    for step in range(T):
        la.step_lookahead()
        if (step * 7) % 11 < 3:
            la.state["reset_count"].sum().item()   # (goes through sync(): a rewind when the ring has run ahead)
            looks += 1
    rewinds = la._la["rewinds"]
    la.sync()
    lo, hi = _record(_stream_sim(30, N, W, offset=0)), _record(_stream_sim(37, N, W, offset=30))
    for _ in range(T):
        lo.step(), hi.step()
    print("W", W, "rewinds", rewinds, "looks", looks, "deepest episode", int(single.state["reset_count"].max()),
          "refills", single._cstream["refills"], roll._cstream["refills"], la._cstream["refills"])
    assert rewinds >= 3 and int(single.state["reset_count"].max()) > W
    for other, what in ((roll, "rollout"), (la, "ring")):
        _same_state(single, other, what)
        for a, b in zip(_log_bytes(single), _log_bytes(other)):
            assert torch.equal(a, b), what
        for a, b in zip(_tape(single), _tape(other)):
            assert torch.equal(a, b), what
    for n in STATE:
        assert torch.equal(single.state[n], torch.cat([lo.state[n], hi.state[n]])), n
    for n in ("obs", "rewards", "done", "game_over"):
        assert torch.equal(getattr(single, n), torch.cat([getattr(lo, n), getattr(hi, n)])), n
    head = torch.cat([_log_bytes(lo)[0], _log_bytes(hi)[0]])
    assert torch.equal(_log_bytes(single)[0][..., [0, 1, 3]], head[..., [0, 1, 3]])
    assert torch.equal(_log_bytes(single)[1], torch.cat([_log_bytes(lo)[1], _log_bytes(hi)[1]]))
    for a, b, c in zip(_tape(single), _tape(lo), _tape(hi)):
        assert torch.equal(a, torch.cat([b, c], dim=1))
    for b in (single, roll, la, lo, hi):
        b.check_faults()


# ---------------------------------------------------------------- 6. reset replay, seed, detach
def test_reset_replays_a_new_seed_does_not_and_none_detaches():
    nat, core, _ = _mods()
    E, N, W, T = 40, 4, 3, 60
    s = _stream_sim(E, N, W)
    first = [tuple(x.clone() for x in s.step()) for _ in range(T)]
    keep = [n for n in STATE if n != "env_stats"]      # (the statistics outlive a reset)
    end = {n: s.state[n].clone() for n in keep}
    assert int(s.state["reset_count"].max()) > W
    s.reset_from_stream()
    assert int(s.state["reset_count"].max()) == 0
    for step in range(T):
        for x, y in zip(s.step(), first[step]):
            assert torch.equal(x, y), step
    for n in keep:
        assert torch.equal(s.state[n], end[n]), n
    other = _stream_sim(E, N, W, seed=SEED + 1)
    assert not torch.equal(other.state["pos_x"], _stream_sim(E, N, W).state["pos_x"])
    for _ in range(T):
        other.step()
    assert not torch.equal(other.state["pos_x"], end["pos_x"])
    assert s.stream_case_index(3, 5) == (3 << 32) | 5
    assert np.array_equal(_stream_sim(4, N, W, offset=9).stream_case_index(np.arange(4), 2), ((np.arange(4) + 9) << 32) | 2)
    # detached: a sim that never had a stream
    s.set_case_stream(None)
    assert s._cstream is None and s._ar is None and s._draw is None
    plain = core.BatchedSim(core.make_params(E, N, ragged=1, max_time_ratio=1.5))
    plain.set_plugins(nat.POL_RVO)
    cases = _scenarios(s, E, 1)[:, 0]
    s.set_plugins(nat.POL_RVO)
    s.reset(cases), plain.reset(cases)
    for step in range(40):
        for x, y in zip(s.step(), plain.step()):
            assert torch.equal(x, y), step
    assert int(s.state["reset_count"].max()) == 0 and bool(s.game_over.any())
    for n in keep:
        assert torch.equal(s.state[n], plain.state[n]), n
    s.check_faults()


# ---------------------------------------------------------------- 7. the overrun flag
def test_overrun_raises_bit_3():
    """W = 1 and a ring of 32 steps over two-agent scenarios that end within a few steps: some env finishes two episodes
    inside one launch, the next refill raises bit 3 of the library's status word and check_faults() raises; W = 8 on the
    same run leaves the word 0.  (The library's own flag on healthy kernels, like bits 1 and 2 -- not a hardware fault.)"""
    nat = _mods()[0]
    quick = dict(side_length=1.0, speed_bnds=(2.0, 2.0), radius_bnds=(0.05, 0.1))
    assert nat.device_faults(clear=True) == 0
    for W, want in ((8, 0), (1, nat.FAULT_STREAM_OVERRUN)):
        s = _stream_sim(64, 2, W, dist=quick, num_agents=None, draw=False, heading_seed=0)
        s.enable_lookahead(32, fresh=True)
        for _ in range(32):
            s.step_lookahead()
        rc = s._state["reset_count"]          # (the ring has been consumed to its end: the state is the one handed out)
        torch.cuda.synchronize()
        print("W", W, "episodes finished inside one ring launch: up to", int(rc.max()))
        assert int(rc.max()) >= 2 and int(rc.max()) <= 8
        assert nat.device_faults(clear=False) == 0       # (raised by the refill that follows, not by the step kernels)
        s.step_lookahead()                               # the next ring: its refill sees reset_count - seen > W
        torch.cuda.synchronize()
        assert nat.device_faults(clear=False) == want
        if want:
            with pytest.raises(nat.CagpuError, match="bit 3"):
                s.check_faults()
        else:
            s.check_faults()
        assert nat.device_faults(clear=True) == 0


# ---------------------------------------------------------------- 8. off by default
def test_off_by_default_on_the_bench_geometry():
    """without a stream nothing new is launched: cagpu_last_kernel() of a default step, a ring launch and the bench.py
    geometry is the parent's string -- and the stream's own launches leave that string alone"""
    E, N = 4096, 10
    s = _fixture_sim(E, N, gu.fixtures(N), True)
    assert s._cstream is None
    s.enable_lookahead(20, fresh=True)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.enable_lookahead(0)
    s.step()
    single = PARENT_BENCH_KERNEL.replace("true", "false").replace(" fair", "")
    assert _last_kernel() == single
    s.rollout(5)
    rolled = _last_kernel()
    t = _stream_sim(64, 4, 3)                # (attaches, refills, resets: generator and refill launches)
    t.step()
    mine = _last_kernel()
    t._stream_refill()
    t.generate_cases_at(np.arange(5), 1)
    assert _last_kernel() == mine and "generate" not in mine
    s.step()
    assert _last_kernel() == single
    s.rollout(5)
    assert _last_kernel() == rolled
    s.check_faults()


# ---------------------------------------------------------------- the env API
def test_env_api_streams_fresh_scenarios():
    """set_fixture_suite(generate=dict(stream=True, ...)) with random headings and a policy pool -- the reference's default
    TEST_CASE_ARGS on the device: the batch runs on a case stream, and its envs stand on their own scenarios"""
    Config, tc, Env = envtools.fresh("Swap4")
    try:
        Config.MAX_TIME_RATIO = 1.5
        E, N = 16, 4
        env = Env(num_envs=E)
        env.set_fixture_suite(N, policies=["RVO", "noncoop", "static"], policy_distr=[0.6, 0.3, 0.1], policy_to_ensure="RVO",
                              random_headings=True, env_id_offset=5,
                              generate=dict(stream=True, window=4, seed=SEED, num_agents=(2, N), **SHORT))
        env.reset()
        sim = env._sim
        assert sim._cstream is not None and sim._cstream["W"] == 4 and sim._ar.n_cases == E * 4 and sim._ar.heading_seed != 0
        assert sim.p.ragged == 1 and sim._draw is not None and sim._ar.env_id_offset == 5
        want = _scenarios(sim, E, 12, offset=5)       # (60 steps of these short trips stay below episode 12)
        ar = torch.arange(E, device=sim.device)

        def check():
            rc = sim.state["reset_count"].to(torch.int64)
            rows = want[ar, torch.clamp(rc, max=11)]
            present = rows[..., 5] > 0
            ok = (rc < 12)[:, None] & present
            # (what a step never changes: a StaticPolicy agent's goal becomes its position at its first move)
            assert torch.equal(torch.where(ok, sim.state["radius"], rows[..., 5]), rows[..., 5])
            assert torch.equal(torch.where(ok, sim.state["pref_speed"], rows[..., 4]), rows[..., 4])
            assert bool(ok.any(dim=1).all())
            return rc
        check()
        for _ in range(60):
            env.step(None)
        rc = check()
        assert int(rc.max()) > 4
        sim.check_faults()
        with pytest.raises(ValueError):
            env.set_fixture_suite(N, generate=dict(stream=True, num_cases=5, seed=1))
        with pytest.raises(ValueError):
            env.set_fixture_suite(N, auto_reset=False, generate=dict(stream=True, seed=1))
    finally:
        envtools.default()
