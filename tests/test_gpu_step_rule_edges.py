"""The reward, collision, goal, time-out, done and game-over rules of the STEP kernels and the ranking of their sensor against
the oracle on the threshold scenes of tests/step_rule_scenes.py (what each class is for, that the oracle is right on them and
that the reference says the same: tests/test_step_rule_scenes_host.py), on every launch path of orca_scenes.PATHS: the
pipelined kernel, the tiled kernel with N <= 10, 11 <= N <= 16, N > 16 and the large-env kernel.  A scene is injected into
oracle and sim, both step once, then two more times from the GPU's own bits.  After every step _compare holds masks, done, game
over and num_other_agents_observed exactly; on top of it the (radius, combined radius) columns of every observation slot -- who
sits in the slot -- must equal the oracle's word for word, and on the first step every reward and flag word that the scene fixes
must be the scene's (the two sides of every threshold are at least 0.05 apart in reward; a float32 reward is good to 1e-7).  The
launch must be the intended instantiation and the device's fault word must stay zero.  The second test takes the same three
steps from one rollout(3) and from a look-ahead ring of 3 -- the MULTI instantiations: other code, the same rules -- and holds
them to the single steps bit for bit.  With CAGPU_TEST_DUMP_DIR set to an existing directory a failing case leaves its inputs
there."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import orca_scenes as S
from tests import step_rule_scenes as R
from tests.test_gpu_orca_edges import _kernel_pattern
from tests.test_gpu_parity import F64, _compare, _download, _mods, _upload

pytestmark = pytest.mark.gpu

STEPS = 3
SIDE = 0.025       # half of the least distance between the rewards on the two sides of a threshold


def _pattern(path, N, E, mapped, multi=False):
    if not multi:
        pat = _kernel_pattern(path, N, E)
        return pat[:-1] + (" map$" if mapped else "$") if pat.endswith("$") else pat
    # the n-step instantiations (MULTI = true); a ring may take the read-only form of the tiled kernel
    if path == "pipelined":
        return r"ca_pipe_kernel<%d, %d, true> grid=3 " % (N, S.PIPE_TILE[N])
    return r"ca_kernel<%d, (true|false), %d, true, (true|false), \d+> grid=\d+ " % (512 if N > 32 else 256, N if N in (10, 20) else 0)


def _cases():
    out = []
    for path, shapes in S.PATHS.items():
        for N, E in shapes:
            for cls in R.CLASSES:
                if N < R.MIN_AGENTS[cls]:
                    continue
                for v in R.VARIANTS[cls]:
                    if path == "pipelined" and not R.pipelined_eligible(cls, v):
                        continue
                    out.append((path, cls, v, N, E))
    return out


def _fused_cases():
    """one shape per path, every class: the variant whose rules differ most from the defaults"""
    shape = {"pipelined": (10, 9), "tiled": (7, 19), "gs16": (13, 9), "wave": (33, 3), "big": (65, 3)}
    pick = {"t": "", "c": "clip", "g": "", "o": "learning", "w": "", "m": "", "s": "first-below"}
    return [(path, cls, pick[cls], N, E) for path, (N, E) in shape.items() for cls in R.CLASSES] + \
           [(path, "s", "last-below", N, E) for path, (N, E) in shape.items() if path != "pipelined"]


def _pair(sc, pipeline):
    nat, core, orc = _mods()
    o = orc.Oracle(R.oracle_params(orc, sc))
    R.inject(o, sc)
    g = core.BatchedSim(core.make_params(sc.E, sc.N, **R.sim_kwargs(sc)), record_actions=True, pipeline=pipeline)
    if sc.static_map is not None:
        o.set_map(sc.static_map, rows=R.MAP_ROWS, cols=R.MAP_COLS, cell=R.MAP_CELL)
        g.set_map(sc.static_map, rows=R.MAP_ROWS, cols=R.MAP_COLS, cell=R.MAP_CELL)
    _upload(o, g)
    return o, g


def _dump(name, sc, t, **arrays):
    d = os.environ.get("CAGPU_TEST_DUMP_DIR")
    if d and os.path.isdir(d):
        np.savez(os.path.join(d, "step_rule_edges_%s_step%d.npz" % (name, t)), label=sc.label,
                 **dict({n: getattr(sc, n) for n in S.Scene.FIELDS}, **arrays))


def _slots(obs, K):
    """the (radius, combined radius) columns of every slot: [E, N, K, 2]"""
    return obs[..., 6:].reshape(obs.shape[0], obs.shape[1], K, 7)[..., 4:6]


@pytest.mark.parametrize("path,cls,variant,N,E", _cases(), ids=lambda v: str(v) if v != "" else "-")
def test_step_rules_on_threshold_scenes(path, cls, variant, N, E):
    nat, core, orc = _mods()
    sc = R.build(cls, N, E, variant)
    o, g = _pair(sc, path == "pipelined")
    ext = R.ext_actions(sc)
    ext_dev = None if ext is None else torch.from_numpy(ext).to(g.device)
    pattern = _pattern(path, N, E, sc.static_map is not None)
    name = "%s_%s%s_%d" % (path, cls, "_" + variant if variant else "", N)
    K = sc.max_obs
    slots = held = 0
    for t in range(STEPS):
        if t:
            _download(g, o)
        o.step(ext)
        g.step(ext_dev)
        kern = nat.lib().cagpu_last_kernel().decode()
        assert re.match(pattern, kern), (kern, pattern)
        gobs, grew = g.obs.cpu().numpy(), g.rewards.cpu().numpy().astype(np.float64)
        gfl = g.state["flags"].cpu().numpy().astype(np.uint32)
        try:
            _compare(o, g, what="%s step %d" % (name, t))
            want = _slots(o.obs, K).astype(np.float32)
            got = _slots(gobs, K)
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), "%s step %d: %d observation slots hold another agent, first (env, host, slot) %s" % (
                name, t, int(bad.any(-1).sum()), np.argwhere(bad.any(-1))[:4].tolist())
            slots += int((want[..., 0] > 0).sum())
            if t == 0:
                care = ~np.isnan(sc.expect_reward)
                off = care & (np.abs(grew - np.nan_to_num(sc.expect_reward)) >= SIDE)
                assert not off.any(), "%s: %d rewards on the wrong side of their threshold: (env, agent) %s got %s want %s" % (
                    name, int(off.sum()), np.argwhere(off)[:4].tolist(), grew[off][:4], sc.expect_reward[off][:4])
                mask = np.uint32(R.AT_GOAL | R.IN_COLLISION | R.OUT_OF_TIME)
                wrong = ((gfl & mask) != sc.expect_flags) & sc.expect_care
                assert not wrong.any(), "%s: flag words off the scene's: (env, agent) %s" % (name, np.argwhere(wrong)[:4].tolist())
                held += int(care.sum()) + int(sc.expect_care.sum())
        except AssertionError:
            _dump(name, sc, t, obs=gobs, rewards=grew, flags=gfl, want_obs=o.obs, want_rewards=o.rewards, want_flags=o.s["flags"])
            raise
    assert slots > 0 or N == 2 and cls == "s"
    assert held > 0 or cls == "s"
    assert nat.device_faults(clear=True) == 0
    print("step-rule-edges %-9s %s %-12s N=%-3d E=%-2d K=%-3d slots compared %5d, rewards and flag words held %4d" % (
        path, cls, variant or "-", N, E, K, slots, held))


def _bits(g, outs):
    obs, rew, done, over = outs
    d = {n: g.state[n].cpu().numpy().copy() for n in F64 + ("flags", "step_num", "episode_step", "last_action")}
    d.update(obs=obs.cpu().numpy().copy(), rewards=rew.cpu().numpy().copy(), done=done.cpu().numpy().astype(np.uint8),
             game_over=over.cpu().numpy().astype(np.uint8))
    return d


def _same(a, b, what):
    for n in a:
        x, y = a[n], b[n]
        if n == "flags":
            x, y = x & ~(1 << 17), y & ~(1 << 17)        # (bit 17, PLAN_VALID, is the pipelined kernel's bookkeeping)
        assert x.tobytes() == y.tobytes(), "%s: %s differs" % (what, n)


@pytest.mark.parametrize("path,cls,variant,N,E", _fused_cases(), ids=lambda v: str(v) if v != "" else "-")
def test_fused_steps_equal_single_steps_on_threshold_scenes(path, cls, variant, N, E):
    nat, core, orc = _mods()
    sc = R.build(cls, N, E, variant)
    ext = R.ext_actions(sc)
    mapped = sc.static_map is not None
    # (a) three single steps, the outputs of every one kept
    o, g = _pair(sc, path == "pipelined")
    ext_dev = None if ext is None else torch.from_numpy(ext).to(g.device)
    single = []
    for t in range(STEPS):
        g.step(ext_dev)
        single.append((g.obs.clone(), g.rewards.clone(), g.done.clone(), g.game_over.clone()))
    want = _bits(g, single[-1])
    # (b) one rollout of three steps
    o, r = _pair(sc, path == "pipelined")
    r.rollout(STEPS, ext_dev)
    kern = nat.lib().cagpu_last_kernel().decode()
    assert (" map" in kern) == mapped, kern      # (a fused launch with a map: cagpu_step_ex_maps)
    if path != "big":      # (the large-env kernel takes a rollout as n launches of the single step)
        assert re.match(_pattern(path, N, E, mapped, multi=True), kern), kern
    _same(want, _bits(r, (r.obs, r.rewards, r.done, r.game_over)), "rollout(3) %s %s" % (path, cls))
    # (c) a look-ahead ring of three slots (no external actions in a ring: class w stays with the rollout)
    if ext is None:
        o, k = _pair(sc, path == "pipelined")
        k.enable_lookahead(STEPS, fresh=True)
        for t in range(STEPS):
            obs, rew, done, over = k.step_lookahead()
            for x, y, n in zip((obs, rew, done, over), single[t], ("obs", "rewards", "done", "game_over")):
                assert x.cpu().numpy().astype(y.cpu().numpy().dtype).tobytes() == y.cpu().numpy().tobytes(), "ring slot %d %s" % (t, n)
        kern = nat.lib().cagpu_last_kernel().decode()
        if path != "big":
            assert re.match(_pattern(path, N, E, mapped, multi=True), kern), kern
        _same(want, _bits(k, (obs, rew, done, over)), "ring of 3 %s %s" % (path, cls))
    assert nat.device_faults(clear=True) == 0
    print("step-rule-edges fused %-9s %s %-11s N=%-3d E=%-2d: rollout(3)%s equal three single steps bit for bit" % (
        path, cls, variant or "-", N, E, "" if ext is not None else " and a ring of 3"))
