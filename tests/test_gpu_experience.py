"""The experience tape, GAE and in-place weight updates on the GPU (core.BatchedSim.collect / Experience.gae / update_ga3c;
include/cagpu.h cagpu_ga3c_sample's slot pointers, cagpu_gae): the tape against a hand-assembled loop of single steps in the
style of experiments/collect_regression_dataset.py::fill (clone, step, mask), under every launch pattern, shard layout and
batch mix; GAE against the float32 loop of tests/gae_ref.py bit for bit.

Shapes: 6 x 4 on the short-trip table (max_time_ratio = 0.8: every env auto-resets at least twice in 16 steps); a ragged
3 x 7 table; GAE arrays with n in {1, 2, 17} and E * N in {1, 63, 65, 130}."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import gae_ref  # noqa: E402
from tests.test_ga3c_sample_host import GAE_PARAMS, GAE_SHAPES  # noqa: E402
from tests.test_gpu_ga3c_sample import E, N, SEED, STEPS, _mods, evaluated, make_sim, table  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("obs", "action", "logp", "value", "live", "reward", "done", "game_over", "address")
_shared = {}


def by_steps(sim, n, offset=0):
    """the tape of n single step() calls, assembled by hand: clone, step, mask -> dict of tensors shaped like an Experience"""
    rec = {k: [] for k in FIELDS}
    dev = sim.device
    for t in range(n):
        pre = sim.obs.clone()
        flags = sim.state["flags"].clone()
        k = sim.state["reset_count"].clone().long()
        sim.step()
        live = torch.as_tensor(evaluated(flags.cpu().numpy()), device=dev)
        zero = lambda x: torch.where(live.reshape(live.shape + (1,) * (x.dim() - 2)), x, torch.zeros_like(x))
        rec["obs"].append(zero(pre[..., 1:]))
        rec["action"].append(zero(sim._ga3c_ext[..., 0].to(torch.int8)))
        rec["logp"].append(zero(sim.ga3c_logp))
        rec["value"].append(zero(sim.ga3c_value))
        rec["live"].append(live)
        rec["reward"].append(sim.rewards.clone())
        rec["done"].append(sim.done.bool().clone())
        rec["game_over"].append(sim.game_over.bool().clone())
        rec["address"].append(torch.stack([torch.arange(sim.E, device=dev) + offset, k], dim=1))
    return {k: torch.stack(v) for k, v in rec.items()}


def tape_of(*xps):
    return {k: torch.cat([getattr(x, k) for x in xps]) for k in FIELDS}


def same_tape(a, b, what, envs=slice(None)):
    for k in FIELDS:
        x, y = a[k][:, envs], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        if x.dtype == torch.float32:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), "%s: %s differs" % (what, k)


def same_state(a, b, what):
    assert torch.equal(a._slab, b._slab), what + ": state"
    for n_ in ("obs", "rewards", "done", "game_over"):
        assert torch.equal(getattr(a, n_), getattr(b, n_)), what + ": " + n_


def reference_run():
    """the 6 x 4 sampled batch through 16 single steps (shared, never changed)"""
    if "steps" not in _shared:
        s = make_sim()
        _shared["steps"] = (by_steps(s, STEPS), s)
    return _shared["steps"]


# ---------------------------------------------------------------- 3. / 5. the same numbers under every launch pattern
def test_collect_equals_single_steps_under_every_launch_pattern():
    want, s0 = reference_run()
    assert (s0.state["reset_count"].cpu().numpy() >= 2).all() and bool(want["live"].any()) and not bool(want["live"].all())
    a = make_sim()
    xa = a.collect(STEPS)
    same_tape(want, tape_of(xa), "collect(16)")
    same_state(s0, a, "collect(16)")
    b = make_sim()
    x1, x2 = b.collect(5), b.collect(11)
    same_tape(want, tape_of(x1, x2), "collect(5) + collect(11)")
    same_state(s0, b, "collect(5) + collect(11)")
    # last_value is the value the next collect writes into its slot 0 (where that slot is live; zero elsewhere)
    live0 = x2.live[0]
    assert torch.equal(x1.last_value[live0], x2.value[0][live0]) and bool(live0.any())
    assert bool((x1.last_value[~live0] == 0).all())
    assert torch.equal(a.ga3c_logp[xa.live[-1]], xa.logp[-1][xa.live[-1]])
    # the observation rows are optional
    c = make_sim()
    xc = c.collect(STEPS, keep_obs=False)
    assert xc.obs is None and torch.equal(xc.logp, xa.logp) and torch.equal(xc.action, xa.action)
    for s in (a, b, c):
        s.check_faults()


def test_shards_give_the_corresponding_slices():
    want, _ = reference_run()
    lo, hi = make_sim(envs=2, offset=0, total=E), make_sim(envs=4, offset=2, total=E)
    same_tape(want, tape_of(lo.collect(STEPS)), "shard 0..1", envs=slice(0, 2))
    same_tape(want, tape_of(hi.collect(STEPS)), "shard 2..5", envs=slice(2, 6))


def test_replay_of_a_sampled_batch():
    from tests.test_gpu_replay import Original, _same_episode

    class Sampled(Original):
        def __init__(self):
            s = make_sim()
            self.sim, self.ring = s, False
            s.record_trajectories()
            s.keep_final()
            s.log_episodes(capacity=64)
            s.measure_episodes(capacity=64, keep_tape=True)
            t = table()
            s.reset(t[np.arange(E) % t.shape[0]])
            self.t, self.outs, self.fins = 0, {}, []

    o = Sampled()
    o.run_until(lambda rc: rc.min() >= 3)
    rc = o.counts()
    env, ep = [0, E - 1], [1, int(rc[E - 1]) - 1]
    rep = o.sim.replay(env, ep, keep_outputs=True)
    o.finish()
    for i in range(2):
        _same_episode(o, rep, i, "sampled")
    # ... and the replay did sample: a greedy child runs another episode
    assert rep.sim._samp is not None and rep.sim._samp["seed"] == SEED
    rep.sim.check_faults()


# ---------------------------------------------------------------- 4. mixed and ragged
def _check_mixed(sim, n, what):
    """collect(n) against the hand-assembled loop on a twin; NaN in the entries nobody reads changes nothing"""
    twin = _shared.pop("twin")
    want = by_steps(twin, n)
    sim.ga3c_logits.fill_(float("nan"))     # (the network rewrites the rows of the agents it evaluates, nobody reads the rest)
    sim.ga3c_value.fill_(float("nan"))
    xp = sim.collect(n)
    same_tape(want, tape_of(xp), what)
    same_state(twin, sim, what)
    live = xp.live
    assert bool(live.any()) and not bool(live.all()), what
    for k in ("action", "logp", "value"):
        assert bool((getattr(xp, k)[~live] == 0).all()), (what, k)
    assert bool((xp.obs[~live] == 0).all())
    adv, ret = xp.gae(0.99, 0.95)
    assert bool((adv[~live] == 0).all()) and bool((ret[~live] == 0).all()) and bool(torch.isfinite(adv).all())
    sim.check_faults()
    return xp


def test_ragged_table_with_absent_slots():
    kw = dict(envs=3, agents=7, counts=(3, 7))
    _shared["twin"] = make_sim(**kw)
    xp = _check_mixed(make_sim(**kw), 12, "ragged")
    nat, _ = _mods()
    assert xp.live.shape == (12, 3, 7)


def test_rvo_and_static_agents_beside_ga3c():
    nat, _ = _mods()
    pol = np.array([nat.POL_GA3C_CADRL, nat.POL_RVO, nat.POL_STATIC, nat.POL_GA3C_CADRL])
    _shared["twin"] = make_sim(policy=pol)
    xp = _check_mixed(make_sim(policy=pol), STEPS, "mixed policies")
    assert not bool(xp.live[:, :, 1:3].any()) and bool(xp.live[:, :, 0].any()) and bool(xp.live[:, :, 3].any())


def test_policy_draw_makes_ga3c_agents_in_some_episodes_only():
    nat, core = _mods()
    pool = [core.policy_word_bits(nat.POL_GA3C_CADRL), core.policy_word_bits(nat.POL_RVO)]
    draw = ((pool, [0.5, 0.5]), dict(seed=0xD1CE))
    _shared["twin"] = make_sim(draw=draw)
    xp = _check_mixed(make_sim(draw=draw), 24, "policy draw")
    per_episode = {}
    live, addr = xp.live.cpu().numpy(), xp.address.cpu().numpy()
    for t in range(24):
        for e in range(E):
            per_episode.setdefault((e, int(addr[t, e, 1])), set()).add(tuple(live[t, e].tolist()))
    kinds = {frozenset(a for row in rows for a in np.flatnonzero(row)) for rows in per_episode.values()}
    assert len(kinds) > 2, kinds       # different episodes, different GA3C-CADRL agents


# ---------------------------------------------------------------- 6. GAE
def _gae_gpu(d, gamma, lam):
    nat, core = _mods()
    dev = torch.device("cuda", 0)
    t = {k: torch.as_tensor(np.ascontiguousarray(v)).to(dev) for k, v in d.items()}
    xp = core.Experience.__new__(core.Experience)
    sim = _shared.get("gae_sim") or core.BatchedSim(core.make_params(2, 2))
    _shared["gae_sim"] = sim
    xp._sim = sim
    for k, v in t.items():
        setattr(xp, k, v)
    adv, ret = xp.gae(gamma, lam)
    return adv.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("n,En,Nn", GAE_SHAPES)
def test_gae_bit_for_bit_on_synthetic_arrays(n, En, Nn):
    d = gae_ref.synthetic(n, En, Nn, seed=100 + n + En * Nn)
    for gamma, lam in GAE_PARAMS:
        adv, ret = _gae_gpu(d, gamma, lam)
        wa, wr = gae_ref.gae32(gamma=gamma, lam=lam, **d)
        assert adv.tobytes() == wa.tobytes() and ret.tobytes() == wr.tobytes(), (gamma, lam, np.abs(adv - wa).max())


def test_gae_bit_for_bit_on_the_tape():
    s = make_sim()
    xp = s.collect(STEPS)
    d = {k: getattr(xp, k).cpu().numpy() for k in ("reward", "value", "last_value", "live", "done", "game_over")}
    br = gae_ref.branches(d["live"], d["done"], d["game_over"])
    assert br["not_live"] > 0 and br["done"] > 0 and br["plain"] > 0, br
    for gamma, lam in GAE_PARAMS:
        adv, ret = xp.gae(gamma, lam)
        wa, wr = gae_ref.gae32(gamma=gamma, lam=lam, **d)
        assert adv.cpu().numpy().tobytes() == wa.tobytes() and ret.cpu().numpy().tobytes() == wr.tobytes(), (gamma, lam)


# ---------------------------------------------------------------- 7. update_ga3c
def test_update_ga3c_in_place():
    nat, core = _mods()
    other = os.path.join(os.path.dirname(core.GA3C_DEFAULT_WEIGHTS), "..", "run-20190727_192048-qedrf08y", "network_01900000.npz")
    a = make_sim(sample=False)
    ptrs = {k: v.data_ptr() for k, v in a._net_tensors.items()}
    with np.load(other) as z:
        w = {k: torch.as_tensor(np.ascontiguousarray(z[k], np.float32)).to(a.device) for k in z.files
             if k in core._GA3C_SHAPES or k in core._GA3C_NAMES.values() or k.startswith("logits_v")}
    before = a.ga3c_logits.clone()
    a.ga3c()
    first = a.ga3c_logits.clone()
    with pytest.raises(ValueError, match="unknown key"):
        a.update_ga3c(dict(w, nonsense=w["lstm_bias"]))
    with pytest.raises(ValueError, match="shape"):
        a.update_ga3c(dict(w, lstm_bias=w["lstm_bias"][:5]))
    a.ga3c()
    assert torch.equal(a.ga3c_logits, first)            # a refused update changed nothing
    a.update_ga3c(w)
    a.ga3c()
    b = make_sim(sample=False)
    b.load_ga3c(other, keep_logits=True, keep_value=True)
    b.ga3c()
    assert torch.equal(a.ga3c_logits, b.ga3c_logits) and torch.equal(a.ga3c_value, b.ga3c_value)
    assert not torch.equal(a.ga3c_logits, first)
    assert {k: v.data_ptr() for k, v in a._net_tensors.items()} == ptrs
    del before


# ---------------------------------------------------------------- the env form and the experiment script
def test_collect_onpolicy_through_the_env():
    from gym_collision_avoidance_amd.experiments import collect_onpolicy as cop
    env = cop.create_env(num_envs=4, num_agents=3, seed=5, sample_seed=SEED, temperature=2.0)
    env.reset()
    sim = env._sim
    assert sim._samp is not None and sim._samp["seed"] == SEED and sim._samp["temperature"] == 2.0
    b = cop.collect(env, 6, gamma=0.99, lam=0.95)
    M = b["obs"].shape[0]
    assert 0 < M <= 6 * 4 * 3 and b["obs"].shape == (M, sim.W - 1)
    for k in ("action", "logp", "value", "advantage", "returns"):
        assert b[k].shape == (M,), k
    assert b["action"].dtype == torch.int64 and int(b["action"].min()) >= 0 and int(b["action"].max()) <= 10
    assert bool((b["logp"] <= 0).all()) and bool(torch.isfinite(b["advantage"]).all())
    # (under the default, training-mode Config an env without learning agents is over after every step: the six steps
    #  show as auto-resets, under EvaluateConfig as step numbers)
    assert len(b["action"].unique()) > 1
    assert int(sim.state["step_num"].sum()) + int(sim.state["reset_count"].sum()) >= 6 and env.episode_step_number == 6
    env.sample_ga3c_on_device(None)
    assert sim._samp is None
    sim.check_faults()


# ---------------------------------------------------------------- 8. the byte budget
def test_byte_budget_raises_before_anything_is_launched():
    nat, _ = _mods()
    s = make_sim()
    s.step()
    per = s.experience_step_bytes(True)
    assert per == E * N * (14 + 4 * (s.W - 1)) + 17 * E
    s.experience_max_bytes = 4 * per + 4 * E * N
    slab, obs = s._slab.clone(), s.obs.clone()
    last = nat.lib().cagpu_last_kernel()
    with pytest.raises(nat.CagpuError, match="keep_obs=False"):
        s.collect(5)
    assert torch.equal(s._slab, slab) and torch.equal(s.obs, obs) and nat.lib().cagpu_last_kernel() == last
    assert s.collect(4).n == 4
    assert s.collect(5, keep_obs=False).n == 5
