"""The policy draw of an on-device auto-reset (include/cagpu.h CaPolicyDraw; core.BatchedSim.set_policy_draw;
set_fixture_suite(policy_distr=...)) against its NumPy restatement (tests/policy_draw_ref.py).

The draw is a pure function of (seed, global env id, episode number), so every comparison here is EXACT: the flag words
against the restatement, and a batch that draws at its auto-resets against a TWIN without auto-reset that is host-reset to
the same case at each of its game overs and handed the restatement's flag words directly -- state, observations (column 0
included), rewards and done bit for bit at every step.

The tables hold short trips under a small max_time_ratio: every episode ends within about a dozen steps."""
import math
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
from tests import policy_draw_ref as ref  # noqa: E402
from tests.test_gpu_final_obs import PARENT_BENCH_KERNEL, _last_kernel  # noqa: E402
from tests.test_gpu_final_obs import _sim as _fixture_sim  # noqa: E402
from tests.test_gpu_parity import _mods  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 0xD1CE5EED
DISTR = [0.3, 0.5, 0.2]
STATE = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed", "time_remaining", "t",
         "slt", "ep_reward", "last_action", "step_num", "episode_step")


def _pool():
    """three internal policies; the second carries CA_IS_LEARNING so that column 0 of the observation follows the draw"""
    nat, core, _ = _mods()
    return [core.policy_word_bits(nat.POL_RVO), core.policy_word_bits(nat.POL_NONCOOP, is_learning=True),
            core.policy_word_bits(nat.POL_STATIC)]


def _short_table(C, N, seed, counts=None):
    """C cases of N agents on a jittered 1.5 m grid, each 0.55 .. 0.8 m from its goal; counts: (lo, hi) -> ragged, the
    slots past a case's own count emptied (radius 0)"""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(N)))
    grid = np.array([(i % side, i // side) for i in range(N)], np.float64) * 1.5
    t = np.zeros((C, N, 6))
    for c in range(C):
        pos = grid + rng.uniform(-0.2, 0.2, (N, 2))
        ang, d = rng.uniform(-np.pi, np.pi, N), rng.uniform(0.55, 0.8, N)
        t[c, :, 0:2] = pos
        t[c, :, 2:4] = pos + d[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        t[c, :, 4] = rng.uniform(0.8, 1.2, N)
        t[c, :, 5] = rng.uniform(0.15, 0.25, N)
        if counts is not None:
            t[c, int(rng.integers(counts[0], counts[1] + 1)):, :] = 0.0
    return t


class Batch(object):
    """a batch with the draw and auto-reset (`sim`) plus what the restatement needs to follow it"""

    def __init__(self, E, N, table, offset=0, stride=None, distr=DISTR, ensure=None, seed=SEED, heading_seed=0, pool=None,
                 pipeline=True, draw=True, auto_reset=True, **kw):
        nat, core, _ = _mods()
        self.E, self.N, self.table, self.offset = E, N, table, offset
        self.stride = E if stride is None else stride
        self.bits = _pool() if pool is None else pool
        self.cdf, self.ensure, self.seed, self.heading_seed = ref.cdf_of(distr), -1 if ensure is None else ensure, seed, heading_seed
        self.ragged = bool(kw.get("ragged"))
        kw.setdefault("max_time_ratio", 1.5)
        s = self.sim = core.BatchedSim(core.make_params(E, N, **kw), pipeline=pipeline)
        # (the starting word of every slot: a policy id without learning bits, which no pool entry equals)
        s.set_plugins(nat.POL_NONCOOP)
        self.start_bits = nat.POL_NONCOOP << nat.POLICY_SHIFT
        if auto_reset:
            s.set_fixture_table(table, env_id_offset=offset, case_stride=self.stride, heading_seed=heading_seed)
            if draw:
                s.set_policy_draw(self.bits, distr, ensure=ensure, seed=seed)
        self.k = np.zeros(E, np.int64)
        if auto_reset:
            s.reset(table[self.case()])

    def case(self, k=None):
        return (self.offset + np.arange(self.E) + (self.k if k is None else k) * self.stride) % self.table.shape[0]

    def present(self, k=None):
        rows = self.table[self.case(k)]
        return rows[..., 5] > 0 if self.ragged else np.ones(rows.shape[:2], bool)

    def want_index(self, k):
        """the restatement: pool index of every slot for per-env episode numbers k, -1 where the slot is absent"""
        return ref.draw_batch(self.seed, self.offset + np.arange(self.E), k, self.present(k), self.cdf, self.ensure)

    def want_bits(self, k, before):
        """bits 6..11 of every slot in per-env episodes k, given the words `before` the auto-reset: present slots take
        their pool entry's, absent slots keep what they held (the start word, or an earlier episode's draw)"""
        idx = self.want_index(k)
        return np.where(idx >= 0, np.asarray(self.bits)[np.maximum(idx, 0)], before), idx


def _check_rule(b, resets=3, max_steps=200):
    """after every step: policy_ids(), the learning mask and the untouched words of absent slots equal the restatement"""
    nat = _mods()[0]
    s = b.sim
    seen = set()
    bits = np.full((b.E, b.N), b.start_bits, np.int64)
    k_was = np.full(b.E, -1, np.int64)
    for step in range(max_steps + 1):
        k = s.state["reset_count"].cpu().numpy().astype(np.int64)
        assert ((k == k_was) | (k == k_was + 1)).all()      # (at most one auto-reset per env and step: no episode is skipped)
        new, idx = b.want_bits(k, bits)
        bits = np.where((k != k_was)[:, None], new, bits)
        k_was = k
        flags = s.state["flags"].cpu().numpy()
        assert np.array_equal(flags & ref.DRAW_BITS, bits), "bits 6..11 after step %d (absent slots keep theirs)" % step
        assert np.array_equal(s.policy_ids().cpu().numpy(), (bits >> nat.POLICY_SHIFT) & 0xF), "policy ids after step %d" % step
        assert np.array_equal((flags & nat.ABSENT) != 0, idx < 0)
        learn = ((bits & nat.IS_LEARNING) != 0) & (idx >= 0)
        assert np.array_equal(s.learning_mask().cpu().numpy(), learn)
        # column 0 of the observation handed back is the is_learning bit of the CURRENT episode's draw
        assert np.array_equal(s.obs[..., 0].cpu().numpy() != 0, learn)
        seen.update(int(v) for v in k)
        if k.min() >= resets:
            break
        s.step()
    assert k.min() >= resets and set(range(resets + 1)) <= seen, "not every env took %d auto-resets" % resets
    s.check_faults()
    return k


# ---------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("name", ["n4", "n10", "ragged6", "offset"])
def test_policy_ids_follow_the_rule(name):
    E = 37
    if name == "n4":
        b = Batch(E, 4, _short_table(23, 4, 1), ensure=0)
    elif name == "n10":
        b = Batch(E, 10, _short_table(23, 10, 2), ensure=2)
    elif name == "ragged6":
        b = Batch(E, 6, _short_table(29, 6, 3, counts=(2, 6)), distr=[0.9, 0.05, 0.05], ensure=1, ragged=1)
        n = b.present(np.zeros(E, np.int64)).sum(axis=1)
        assert n.min() == 2 and n.max() == 6
    else:
        b = Batch(E, 4, _short_table(23, 4, 4), offset=(1 << 33) + 1001, stride=41, ensure=1)
    _check_rule(b)
    if name == "ragged6":
        # the ensure slot is counted over present slots only: it fired, and never landed on an absent slot
        fired = 0
        for k in range(4):
            kk = np.full(E, k, np.int64)
            plain = ref.draw_batch(b.seed, b.offset + np.arange(E), kk, b.present(kk), b.cdf, -1)
            fired += int(((plain == 1).sum(axis=1) == 0).sum())
        assert fired > 20


# ---------------------------------------------------------------- 2. the twin, bit for bit
class Twin(object):
    """no auto-reset: at each game over the env is host-reset to the case the auto-reset loads and given the restatement's
    flag words, written directly"""

    def __init__(self, a, **kw):
        self.a = a
        b = self.b = Batch(a.E, a.N, a.table, offset=a.offset, stride=a.stride, auto_reset=False, **kw)
        self.sim = b.sim
        self.k = np.zeros(a.E, np.int64)
        self._reset(np.ones(a.E, bool), first=True)

    def _reset(self, mask, first=False):
        a, s = self.a, self.sim
        idx = a.want_index(self.k)
        fl = s._state["flags"].cpu().numpy()
        new = ref.apply_bits(fl, idx, a.bits).astype(np.uint32).view(np.int32)
        fl[mask] = new[mask]
        s._state["flags"].copy_(torch.from_numpy(fl))
        heads = None
        if a.heading_seed and not first:   # (the first reset points every agent at its goal, as the batch's own does)
            heads = np.zeros((a.E, a.N))
            for e in np.flatnonzero(mask):
                for i in range(a.N):
                    heads[e, i] = -math.pi + (2.0 * math.pi) * ref.uniform_at(a.heading_seed, a.offset + int(e), int(self.k[e]), i)
        s.reset(a.table[a.case(self.k)], headings=heads, mask=None if first else mask.astype(np.uint8))

    def step(self):
        s = self.sim
        s.step()
        over = s.game_over.bool().cpu().numpy()
        if over.any():
            self.k[over] += 1
            self._reset(over)
        return s.obs, s.rewards, s.done, s.game_over


def _same_state(a, t, what):
    nat = _mods()[0]
    sa, sb = a.sim.state, t.sim.state
    for n in STATE:
        assert torch.equal(sa[n], sb[n]), "%s: state[%s]" % (what, n)
    assert torch.equal(sa["flags"] & ~nat.PLAN_VALID, sb["flags"] & ~nat.PLAN_VALID), what + ": flag words"
    assert np.array_equal(sa["reset_count"].cpu().numpy(), t.k), what + ": episode numbers"


def _same_out(out, want, what):
    for x, y, n in zip(out, want, ("obs", "rewards", "done", "game_over")):
        assert torch.equal(x.to(y.dtype) if x.dtype != y.dtype else x, y), "%s: %s" % (what, n)


TWINS = {
    "pipelined_n10": dict(E=8, N=10, kernel="ca_pipe_kernel<10, 4, false>", tag=True),
    "general_n7_closest_last": dict(E=8, N=7, kernel="ca_kernel<", kw=dict(sort_mode=1)),
    "random_headings_n4": dict(E=8, N=4, kernel="ca_kernel<", heading_seed=91),
    "big_n65": dict(E=2, N=65, kernel="ca_big_kernel"),
    "ragged_pipelined_n6": dict(E=8, N=6, kernel="ca_pipe_kernel<6, 10, false>", tag=True, counts=(2, 6), kw=dict(ragged=1)),
}


@pytest.mark.parametrize("name", sorted(TWINS))
def test_twin_single_steps(name):
    c = TWINS[name]
    E, N, kw = c["E"], c["N"], c.get("kw", {})
    table = _short_table(11, N, 7, counts=c.get("counts"))
    a = Batch(E, N, table, ensure=1, heading_seed=c.get("heading_seed", 0), **kw)
    t = Twin(a, **kw)
    _same_state(a, t, name + " reset")
    assert torch.equal(a.sim.obs, t.sim.obs), name + ": reset observation"
    for step in range(60):
        out = a.sim.step()
        if step == 0:
            k = _last_kernel()
            assert k.startswith(c["kernel"]) and k.endswith(" draw") == bool(c.get("tag")), k
        want = t.step()
        _same_out((out[0], out[1], a.sim.done, out[2]), want, "%s step %d" % (name, step))
        _same_state(a, t, "%s step %d" % (name, step))
        if t.k.min() >= 3:
            break
    assert t.k.min() >= 3, t.k
    a.sim.check_faults()


def test_twin_rollout():
    E, N = 8, 10
    a = Batch(E, N, _short_table(11, N, 8), ensure=0)
    t = Twin(a)
    for r in range(4):
        out = a.sim.rollout(12)
        k = _last_kernel()
        assert k.startswith("ca_pipe_kernel<10, 4, true>") and k.endswith(" draw"), k
        for _ in range(12):
            want = t.step()
        _same_out((out[0], out[1], a.sim.done, out[2]), want, "rollout %d" % r)
        _same_state(a, t, "rollout %d" % r)
    assert t.k.min() >= 3
    a.sim.check_faults()


def test_twin_ring_with_a_rewind():
    E, N = 8, 10
    a = Batch(E, N, _short_table(11, N, 9), ensure=2)
    t = Twin(a)
    s = a.sim
    s.enable_lookahead(6, fresh=True)
    for step in range(40):
        out = s.step_lookahead()
        want = t.step()
        _same_out(out, want, "ring step %d" % step)
        if step == 9:     # slot 3 of the second ring: reading the state rewinds and replays 4 steps -- which draw as well
            assert s._la["rewinds"] == 0
            _same_state(a, t, "after the rewind")
            assert s._la["rewinds"] == 1
            assert _last_kernel().endswith(" draw"), _last_kernel()
    s.sync()
    _same_state(a, t, "ring end")
    assert t.k.min() >= 3
    s.check_faults()


# ---------------------------------------------------------------- 3. ensure
def test_every_episode_holds_the_ensured_entry():
    E, N = 64, 3
    b = Batch(E, N, _short_table(17, N, 10), distr=[0.98, 0.02], ensure=1, pool=_pool()[:2])
    nat = _mods()[0]
    s = b.sim
    fired = 0
    for step in range(200):
        ids = s.policy_ids().cpu().numpy()
        assert (ids == nat.POL_NONCOOP).any(axis=1).all(), "an episode without the ensured policy at step %d" % step
        k = s.state["reset_count"].cpu().numpy().astype(np.int64)
        assert np.array_equal(ids, (b.want_bits(k, 0)[0] >> nat.POLICY_SHIFT) & 0xF)
        plain = ref.draw_batch(b.seed, np.arange(E), k, b.present(k), b.cdf, -1)
        fired += int(((plain == 1).sum(axis=1) == 0).sum())
        if k.min() >= 5:
            break
        s.step()
    assert k.min() >= 5 and fired > E, "the ensure rule hardly ever fired"


# ---------------------------------------------------------------- 4. shards
def test_two_shards_agree_with_one_batch():
    N = 4
    table = _short_table(19, N, 11)
    whole = Batch(32, N, table, ensure=1)
    lo = Batch(16, N, table, offset=0, stride=32, ensure=1)
    hi = Batch(16, N, table, offset=16, stride=32, ensure=1)
    for step in range(45):
        for b in (whole, lo, hi):
            b.sim.step()
    for n in STATE + ("flags", "reset_count"):
        both = torch.cat([lo.sim.state[n], hi.sim.state[n]])
        assert torch.equal(whole.sim.state[n], both), n
    assert torch.equal(whole.sim.obs, torch.cat([lo.sim.obs, hi.sim.obs]))
    assert int(whole.sim.state["reset_count"].min()) >= 3


# ---------------------------------------------------------------- 5. off means off
def test_off_means_off_on_the_bench_geometry():
    nat, core, _ = _mods()
    E, N = 4096, 10
    s = _fixture_sim(E, N, gu.fixtures(N), True)
    s.enable_lookahead(20, fresh=True)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.set_policy_draw([core.policy_word_bits(nat.POL_RVO), core.policy_word_bits(nat.POL_NONCOOP)], [0.5, 0.5], seed=SEED)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL + " draw"     # the same selection, grid and block
    s.set_policy_draw(None)
    for _ in range(20):
        s.step_lookahead()
    assert _last_kernel() == PARENT_BENCH_KERNEL
    s.check_faults()
    # cagpu_step_draw without a draw is cagpu_step_ex: 20 steps, the same outputs and state
    x, y = _fixture_sim(E, N, gu.fixtures(N), True), _fixture_sim(E, N, gu.fixtures(N), True)
    step_draw = y.lib.cagpu_step_draw
    y._launch = lambda p, st, o, ext, ar, sx, stream: step_draw(p, st, o, ext, ar, sx, None, stream)
    for step in range(20):
        ox, oy = x.step(), y.step()
        for u, v in zip(ox, oy):
            assert torch.equal(u, v), step
    assert _last_kernel() == PARENT_BENCH_KERNEL.replace("true", "false").replace(" fair", "")
    for n in STATE + ("flags", "reset_count", "env_stats", "next_action"):
        assert torch.equal(x.state[n], y.state[n]), n


# ---------------------------------------------------------------- 6. the env API
def test_env_api_policy_draw():
    Config, tc, Env = envtools.fresh("Small3")
    try:
        Config.MAX_TIME_RATIO = 1.5
        E, N, seed = 16, 3, 4242
        table = _short_table(13, N, 12)
        pool, distr = ["noncoop", "learning", "static"], [0.3, 0.4, 0.3]
        cdf = ref.cdf_of(distr)

        def make(**kw):
            env = Env(num_envs=E)
            args = dict(policies=pool, policy_distr=distr, policy_to_ensure="learning", table=table, policy_seed=seed)
            args.update(kw)
            env.set_fixture_suite(N, **args)
            return env

        # refusals, each with its reason
        class Mine(tc.policy_dict["noncoop"]):
            pass
        tc.policy_dict["mine"] = Mine
        try:
            with pytest.raises(ValueError, match="built-in"):
                make(policies=["noncoop", "mine", "static"])
        finally:
            del tc.policy_dict["mine"]
        with pytest.raises(ValueError, match="pool"):
            make(policies="noncoop")
        with pytest.raises(ValueError, match="not in the pool"):
            make(policy_to_ensure="RVO")
        with pytest.raises(ValueError, match="auto_reset"):
            make(auto_reset=False)

        env = make()
        obs, _ = env.reset()
        sim = env._sim
        ext = torch.zeros((E, N, 2), dtype=torch.float64, device=sim.device)
        ext[..., 0] = 1.0
        ext[..., 1] = 0.5
        classes = [tc.policy_dict[n] for n in pool]
        for step in range(120):
            k = sim.state["reset_count"].cpu().numpy().astype(np.int64)
            idx = ref.draw_batch(seed, np.arange(E), k, np.ones((E, N), bool), cdf, 1)
            assert (idx == 1).any(axis=1).all()
            if step:
                mask = info["which_agents_learning"]
                assert mask.dtype == torch.bool and tuple(mask.shape) == (E, N)
                assert np.array_equal(mask.cpu().numpy(), idx == 1), step
                assert sorted(info) == ["which_agents_done", "which_agents_learning"]
            assert np.array_equal(obs[..., 0].cpu().numpy() != 0, idx == 1), step
            assert [type(a.policy) for a in env.agents] == [classes[j] for j in idx[0]], step
            if k.min() >= 3:
                break
            obs, rewards, over, truncated, info = env.step(ext)
        assert k.min() >= 3
        # without policy_distr nothing changes: the dict of env 0's agents, as ever
        plain = Env(num_envs=E)
        plain.set_fixture_suite(N, policies="noncoop", table=table)
        plain.reset()
        info = plain.step(None)[4]
        assert isinstance(info["which_agents_learning"], dict) and plain._sim._draw is None
    finally:
        envtools.default()
