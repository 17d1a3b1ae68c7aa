"""The RVO draw on the GPU (include/cagpu.h CaRvoDraw; core.BatchedSim.set_rvo_draw): RVOPolicy's anti-collaborative bit and
heading noise drawn inside the step kernels.

The long-standing verified path is the per-step input arrays (CaState.rvo_collab / rvo_heading_noise,
test_gpu_parity.py::test_rvo_stochastic_inputs_vs_oracle): a twin batch is fed, step by step, the arrays the rule's
restatement (tests/rvo_draw_ref.py) and cagpu_rvo_draw_at give for its own state, and must equal the batch that draws in
the kernel word for word.  The noise itself is compared with the restatement in the stand-alone kernel only (a cap of
1e-13 * noise_std: |z| <= 8.6 for 53-bit uniforms, the device's log / sqrt / cos are within a few ulp and the argument
2 pi v0 rounds once, i.e. about 1e-14); everything else is bit for bit.

Shapes: 67 x 5 for the general kernel (a partial last tile), 3 x 65 for the large-env kernel (its smallest); T = 0.3,
DT = 0.1, c = -0.6, every second agent masked; short trips under max_time_ratio = 1.5, so envs auto-reset inside 12 steps."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

torch =pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import rvo_draw_ref as ref  # noqa: E402
from tests.test_gpu_map_rollout import _episodes_np, _same, _snap  # noqa: E402
from tests.test_gpu_map_sets import STATE, _last_kernel, _maps, _mods  # noqa: E402
from tests.test_gpu_parity import _compare, _pair, _upload  # noqa: E402
from tests.test_gpu_policy_draw import _short_table  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, CO, T, DT, STD = 0xA11CE5EED, -0.6, 0.3, 0.1, 0.5
FAMILIES = [(67, 5, "ca_kernel<"), (3, 65, "ca_big_kernel")]
STEPS = 12
_TABLES = {}


def _table(N):
    if N not in _TABLES:
        _TABLES[N] = _short_table(23 if N == 5 else 5, N, 40 + N)
    return _TABLES[N]


def _mask(E, N):
    m = np.zeros((E, N), bool)
    m[:, ::2] = True
    return m


def _sim(E, N, draw=True, offset=0, stride=None, total=None, **kw):
    """a batch of RVO agents on the short-trip table with auto-reset; draw: set_rvo_draw with the module's constants"""
    nat, core, _ = _mods()
    total = E if total is None else total
    s = core.BatchedSim(core.make_params(E, N, max_time_ratio=1.5, **kw))
    s.set_plugins(nat.POL_RVO)
    t = _table(N)
    s.set_fixture_table(t, env_id_offset=offset, case_stride=total if stride is None else stride)
    if draw:
        s.set_rvo_draw(SEED, heading_noise=_mask(E, N), collab_coeff=CO, anti_collab_t=T, noise_std=STD)
    s.reset(t[(np.arange(E) + offset) % t.shape[0]])
    return s


def _draw_at(sim, g, k, a, s, c=CO, std=STD, seed=SEED):
    """cagpu_rvo_draw_at for host int arrays of one shape -> (bool draw, float64 noise) of that shape"""
    nat = _mods()[0]
    shape = np.shape(g)
    dev = sim.device
    tg = torch.as_tensor(np.ascontiguousarray(g, np.int64).reshape(-1)).to(dev)
    tk, ta, ts = (torch.as_tensor(np.ascontiguousarray(x, np.int32).reshape(-1)).to(dev) for x in (k, a, s))
    n = tg.numel()
    od = torch.zeros((n,), dtype=torch.uint8, device=dev)
    on = torch.zeros((n,), dtype=torch.float64, device=dev)
    rd = nat.CaRvoDraw(seed=seed, collab_coeff=c, anti_collab_t=T, noise_std=std)
    nat.check(sim.lib.cagpu_rvo_draw_at(C.byref(rd), sim.N, tg.data_ptr(), tk.data_ptr(), ta.data_ptr(), ts.data_ptr(), n,
                                        od.data_ptr(), on.data_ptr(), sim._stream()))
    return od.cpu().numpy().astype(bool).reshape(shape), on.cpu().numpy().reshape(shape)


class Feeder(object):
    """the per-step input arrays of a twin WITHOUT the in-kernel draw, built on the host from the twin's own state: the
    restatement's window test and carried bit, the numbers of cagpu_rvo_draw_at"""

    def __init__(self, sim, offset=0):
        self.sim, self.offset = sim, offset
        self.bit = np.zeros((sim.E, sim.N), bool)
        self.count = None
        self.keep = None

    def arrays(self):
        nat = _mods()[0]
        s = self.sim
        st = s.state
        E, N = s.E, s.N
        t, sn = st["t"].cpu().numpy(), st["step_num"].cpu().numpy()
        fl, rc = st["flags"].cpu().numpy().astype(np.int64), st["reset_count"].cpu().numpy()
        if self.count is not None:
            self.bit[rc != self.count] = False            # (an auto-reset starts the episode without the bit)
        self.count = rc.copy()
        queried = ((fl & nat.DONE) == 0) & (((fl >> nat.POLICY_SHIFT) & 0xF) == nat.POL_RVO) & ((fl & nat.ABSENT) == 0)
        g = np.broadcast_to((np.arange(E) + self.offset)[:, None], (E, N))
        k = np.broadcast_to(rc[:, None], (E, N))
        a = np.broadcast_to(np.arange(N)[None, :], (E, N))
        draw, noise = _draw_at(s, g, k, a, sn)
        self.bit = np.where(queried & ref.window(t, T, DT), draw, self.bit)
        collab = np.where(self.bit, np.float32(0.0), np.float32(CO)).astype(np.float32)
        noise = np.where(_mask(E, N), noise, 0.0)
        return queried, collab, noise

    def step(self):
        s = self.sim
        queried, collab, noise = self.arrays()
        tc, tn = torch.from_numpy(collab).to(s.device), torch.from_numpy(noise).to(s.device)
        self.keep = (tc, tn)
        s._cs.rvo_collab, s._cs.rvo_heading_noise = tc.data_ptr(), tn.data_ptr()
        s.step()
        return queried, self.bit.copy()


# ---------------------------------------------------------------- 1. the stand-alone kernel against the restatement
def test_draw_at_equals_the_restatement():
    nat, core, _ = _mods()
    sim = core.BatchedSim(core.make_params(2, 4))
    rng = np.random.default_rng(7)
    n = 20000
    g = rng.integers(0, 1 << 33, n)
    k = rng.integers(0, 2000, n)
    a = rng.integers(0, 1024, n)
    s = rng.integers(0, 1 << 22, n)
    g[:4], k[:4], a[:4], s[:4] = (0, (1 << 32) - 1, 1 << 32, 5), (0, 0x7FFFFFFF, 1, 0), (0, 1023, 0, 1023), (0, (1 << 22) - 1, 1, 0)
    draw, noise = _draw_at(sim, g, k, a, s)
    assert np.array_equal(draw, ref.noncoop_draw(SEED, CO, g, k, a, s))
    want = ref.noise(SEED, STD, g, k, a, s)
    err = float(np.abs(noise - want).max())
    print("rvo draw: max |device noise - restatement| = %.3e (noise_std = %g, n = %d)" % (err, STD, n))
    assert err <= 1e-13 * STD, err
    assert 0.35 < draw.mean() < 0.45 and abs(noise.std() - STD) < 0.02
    sim.check_faults()


# ---------------------------------------------------------------- 2. the twin, bit for bit
@pytest.mark.parametrize("E,N,kernel", FAMILIES)
def test_twin_with_input_arrays(E, N, kernel):
    nat = _mods()[0]
    a, a1, b = _sim(E, N), _sim(E, N), _sim(E, N, draw=False)
    feed = Feeder(b)
    outs_b, bits_a1, queried_all, bits_ref = [], [], [], []
    for t in range(STEPS):
        queried, bit = feed.step()
        assert _last_kernel().startswith(kernel) and " noise" not in _last_kernel(), _last_kernel()
        outs_b.append((b.obs.clone(), b.rewards.clone(), b.done.clone(), b.game_over.clone()))
        a1.step()
        assert _last_kernel().startswith(kernel) and _last_kernel().endswith(" noise"), _last_kernel()
        queried_all.append(queried)
        bits_ref.append(bit)
        bits_a1.append(a1.rvo_noncoop().cpu().numpy())
        # the reset clears the bit of envs that auto-reset in this step: compare where the agent was queried and the env went on
        same_ep = (a1.state["reset_count"].cpu().numpy() == feed.count)[:, None]
        where = queried & same_ep
        assert np.array_equal(bits_a1[-1][where], bit[where]), "bit 18 against the restatement, step %d" % t
    obs, rew, done, over = a.rollout(STEPS, keep_steps=True)
    assert _last_kernel().startswith(kernel) and _last_kernel().endswith(" noise"), _last_kernel()
    for t in range(STEPS):
        for x, y, n in zip((obs[t], rew[t], done[t], over[t]), outs_b[t], ("obs", "rewards", "done", "game_over")):
            assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x, y.view(torch.uint8) if y.dtype == torch.bool else y), \
                "%s of step %d" % (n, t)
    sa, sa1, sb = _snap(a), _snap(a1), _snap(b)
    _same(sa, sa1, "rollout(12) against 12 single launches, both drawing in the kernel")
    mask = ~np.int64(nat.RVO_NONCOOP | nat.PLAN_VALID)
    for n in STATE:
        x, y = (sa[n], sb[n]) if n != "flags" else (sa[n].astype(np.int64) & mask, sb[n].astype(np.int64) & mask)
        assert np.array_equal(x, y, equal_nan=True), "state %s against the twin with input arrays" % n
    assert not (sb["flags"].astype(np.int64) & nat.RVO_NONCOOP).any()          # only a CaRvoDraw ever writes the bit
    q = np.stack(queried_all)
    assert int(sb["reset_count"].sum()) > 0 and q.any() and not q.all()
    bits = np.stack(bits_ref)[q]
    assert 0.2 < bits.mean() < 0.6, bits.mean()                                  # (1 - |c| = 0.4)
    assert float(np.abs(feed.keep[1].cpu().numpy()).max()) > 0.1               # the noise is there
    a.check_faults()


# ---------------------------------------------------------------- 3. launch patterns
def test_launch_patterns_give_the_same_bytes():
    E, N = 67, 5
    base = _sim(E, N)
    for _ in range(STEPS):
        base.step()
    want = _snap(base)
    assert (want["flags"] & (1 << 18)).any() and int(want["reset_count"].sum()) > 0

    s = _sim(E, N)
    s.rollout(STEPS)
    _same(_snap(s), want, "rollout(12)")

    s = _sim(E, N)
    s.rollout(5)
    s.rollout(7)
    _same(_snap(s), want, "rollout(5) + rollout(7)")

    s = _sim(E, N)
    assert s.lookahead_ok()
    s.enable_lookahead(4, fresh=True)
    for _ in range(6):
        s.step_lookahead()
    assert _last_kernel().endswith(" noise"), _last_kernel()
    s.sync()                                  # a rewind in the middle of the second ring
    assert s._la["rewinds"] == 1
    for _ in range(6):
        out = s.step_lookahead()
    got = _snap(s)
    _same(got, want, "a ring of 4 with a rewind")
    assert torch.equal(out[0], base.obs)

    lo, hi = _sim(33, N, offset=0, total=E), _sim(34, N, offset=33, total=E)
    lo.rollout(STEPS)
    for _ in range(STEPS):
        hi.step()
    a, b = _snap(lo), _snap(hi)
    _same({n: np.concatenate([a[n], b[n]]) for n in a}, want, "two shards")
    base.check_faults()


# ---------------------------------------------------------------- 4. on top of the rest
def test_on_top_of_the_rest():
    nat, core, _ = _mods()
    E, N = 67, 5
    pool = [core.policy_word_bits(nat.POL_RVO), core.policy_word_bits(nat.POL_LEARNING), core.policy_word_bits(nat.POL_RVO)]
    pol = np.full((E, N), nat.POL_RVO)
    pol[:, 1] = nat.POL_LEARNING
    A = torch.as_tensor(np.random.default_rng(3).uniform(0.0, 1.0, (STEPS, E, N, 2))).cuda()
    sims = []
    for _ in range(2):
        s = core.BatchedSim(core.make_params(E, N, max_time_ratio=1.5))
        s.set_plugins(pol)
        s.set_map(_maps(1, 55)[0])
        s.set_fixture_table(_table(N))
        s.set_policy_draw(pool, [0.5, 0.3, 0.2], ensure=1, seed=99)
        s.set_rvo_draw(SEED, heading_noise=_mask(E, N), collab_coeff=CO, anti_collab_t=T, noise_std=STD)
        s.reset_from_table()
        s.log_episodes(capacity=64)
        s.record_trajectories()
        s.keep_final()
        sims.append(s)
    a, b = sims
    obs, rew, done, over = a.rollout(STEPS, A, keep_steps=True)
    k = _last_kernel()
    assert k.startswith("ca_kernel<") and k.endswith(" map tape noise"), k
    fo, ff = a.kept_final
    for t in range(STEPS):
        b.step(A[t])
        assert torch.equal(obs[t], b.obs) and torch.equal(rew[t], b.rewards) and torch.equal(done[t], b.done), "step %d" % t
        ended = b.game_over.bool()
        assert torch.equal(over[t].bool(), ended)
        assert torch.equal(fo[t][ended], b.final_obs[ended]) and torch.equal(ff[t][ended], b.final_flags[ended]), "final record %d" % t
    _same(_snap(a), _snap(b), "after the launch")
    assert int(b.state["reset_count"].sum()) > 0 and bool((b.policy_ids() == nat.POL_LEARNING).any())
    ea, eb = _episodes_np(a), _episodes_np(b)
    assert sorted(ea) == sorted(eb) and len(eb["env"]) > 0 and eb["dropped"] == 0
    for key in eb:
        assert np.array_equal(ea[key], eb[key], equal_nan=True), key
    ta, tb = a.trajectories(), b.trajectories()
    x, y = ta["rows"].cpu().numpy(), tb["rows"].cpu().numpy()
    moved = y[..., 11] >= 0
    assert np.array_equal(x[..., 11], y[..., 11]) and np.array_equal(x[moved], y[moved])
    assert torch.equal(ta["episode"], tb["episode"])
    a.check_faults()


# ---------------------------------------------------------------- 5. replay
def test_replay_of_a_batch_that_draws_in_the_kernel():
    from tests.test_gpu_replay import Original, _same_episode

    class Drawn(Original):
        def __init__(self):
            self.ring = True
            s = self.sim = _sim(9, 5, draw=False, offset=4, stride=7)
            s.set_rvo_draw(SEED, heading_noise=_mask(9, 5), collab_coeff=CO, anti_collab_t=T, noise_std=STD)
            s.record_trajectories()
            s.keep_final()
            s.log_episodes(capacity=64)
            s.measure_episodes(capacity=64, keep_tape=True)
            self.t, self.outs, self.fins = 0, {}, []

    o = Drawn()
    o.run_until(lambda rc: rc.min() >= 3)
    rc = o.counts()
    env, ep = [0, 8, 3], [0, int(rc[8]) - 1, 1]
    rep = o.sim.replay(env, ep, keep_outputs=True)
    assert rep.sim._rd is not None and rep.sim._rd["addr"].cpu().numpy().tolist() == [[4, 0], [12, ep[1]], [7, 1]]
    o.finish()
    finals = sum(_same_episode(o, rep, i, "rvo draw") for i in range(3))
    assert finals >= 1, "terminal observations compared"
    assert bool((o.log["flags"] & (1 << 18)).any()), "no logged flag word carries the bit"
    rep.sim.check_faults()
    # the torch-generator mode is still refused, in its own words
    g = _sim(4, 5, draw=False)
    g.set_rvo_stochastic(heading_noise=_mask(4, 5), collab_coeff=CO, anti_collab_t=T, seed=3)
    with pytest.raises(ValueError, match="generator whose state was not kept"):
        g.replay([0], [0])


# ---------------------------------------------------------------- 6. against the oracle
def test_one_step_against_the_oracle():
    nat, core, orc = _mods()
    E, N = 67, 5
    o, g = _pair(E, N)
    o.s["policy"][:] = orc.POL_RVO
    g.set_plugins(nat.POL_RVO)
    t = _table(N)
    o.reset(t[np.arange(E) % t.shape[0]])
    for _ in range(3):
        o.step()
    _upload(o, g)
    feed = Feeder(g)
    queried, collab, noise = feed.arrays()
    assert queried.any() and (collab == 0).any() and (collab != 0).any()
    o.set_rvo_stochastic(collab, noise)
    g.set_rvo_draw(SEED, heading_noise=_mask(E, N), collab_coeff=CO, anti_collab_t=T, noise_std=STD)
    o.step()
    g.step()
    assert _last_kernel().endswith(" noise")
    _compare(o, g, what="one step with the draw in the kernel")
    assert np.array_equal(g.rvo_noncoop().cpu().numpy()[queried], feed.bit[queried])


# ---------------------------------------------------------------- 7. off means off
PARENT_KERNELS = {"step": "ca_pipe_kernel<10, 4, false> grid=16 lds=37408 mode=0",
                  "rollout": "ca_pipe_kernel<10, 4, true> grid=16 lds=37408 mode=0",
                  "ring": "ca_pipe_kernel<10, 4, true> grid=16 lds=37408 mode=0"}


def test_off_means_off():
    nat, core, _ = _mods()
    from tests import golden_util as gu
    s = core.BatchedSim(core.make_params(64, 10))
    s.set_plugins(nat.POL_RVO)
    table = gu.fixtures(10)
    s.reset(table[np.arange(64) % table.shape[0]])
    s.step()
    assert _last_kernel() == PARENT_KERNELS["step"], _last_kernel()
    s.rollout(20)
    assert _last_kernel() == PARENT_KERNELS["rollout"], _last_kernel()
    s.enable_lookahead(20)
    s.step_lookahead()
    assert _last_kernel() == PARENT_KERNELS["ring"], _last_kernel()
    assert not bool(s.rvo_noncoop().any()) and s._rd is None
    # set_rvo_stochastic still draws through torch, and rollout() still splits into single launches
    s.enable_lookahead(0)
    s.set_rvo_stochastic(heading_noise=_mask(64, 10), collab_coeff=CO, anti_collab_t=T, seed=5)
    assert not s.lookahead_ok()
    s.rollout(3)
    k = _last_kernel()
    m = re.match(r"ca_kernel<(\d+), (true|false), (\d+), (true|false), ", k)
    assert m and m.group(4) == "false" and " noise" not in k, k                           # a single-step launch
    assert s._rvo["noise"] is not None and s._cs.rvo_heading_noise == s._rvo["noise"].data_ptr()
    assert not bool(s.rvo_noncoop().any())
    with pytest.raises(ValueError, match="set_rvo_stochastic"):
        s.set_rvo_draw(SEED, collab_coeff=CO)
    s.check_faults()


# ---------------------------------------------------------------- 8. the env API
def test_env_api_serves_step_none_from_the_ring():
    from tests import envtools
    Config, tc, Env = envtools.fresh("Bench10")
    Config.RVO_COLLAB_COEFF = -0.6
    try:
        outs = []
        for look in (None, 0):
            env = Env(num_envs=16, lookahead=look)
            env.set_fixture_suite(10, "RVO")
            env.draw_rvo_on_device(SEED)
            env.reset()
            sim = env._sim
            assert sim._rd is not None and sim._rvo is None and sim.lookahead_ok()
            assert env._la_on == (look is None)
            steps = []
            for _ in range(12):
                obs, rew, over = env.step(None)[:3]
                steps.append((obs.clone(), rew.clone(), over.clone()))
            if look is None:
                assert sim._la is not None and sim._la["fills"] >= 1, "step(None) did not come from the ring"
            else:
                assert sim._la is None
            assert _last_kernel().endswith(" noise"), _last_kernel()
            outs.append((steps, sim.rvo_noncoop().clone()))
        for t, (x, y) in enumerate(zip(outs[0][0], outs[1][0])):
            assert all(torch.equal(p, q) for p, q in zip(x, y)), "step %d" % t
        assert torch.equal(outs[0][1], outs[1][1]) and bool(outs[0][1].any())
        # without the opt-in such a batch draws through torch's generator, as before
        env = Env(num_envs=16)
        env.set_fixture_suite(10, "RVO")
        env.reset()
        assert env._sim._rd is None and env._sim._rvo is not None and not env._la_on
    finally:
        envtools.default()
