"""The MOVE of the step kernels -- policy output -> float32 action -> unicycle move -> ego frame -> the float columns of the
observation -- held to the oracle BIT FOR BIT on the angle-edge scenes of tests/move_scenes.py (what each class is for, that
the oracle is right on them and that the reference says the same: tests/test_move_scenes_host.py), on every launch path of
orca_scenes.PATHS at the shapes of the fused step-rule test: the pipelined kernel (10, 9), the tiled kernel with N <= 10 (7, 19),
11 <= N <= 16 (13, 9), N > 16 (33, 3) and the large-env kernel (65, 3).

(a) A scene is injected into oracle and sim; both step once, then twice more from the GPU's own bits.  The oracle runs on the
    DEVICE's libm (tests/device_libm.py: cagpu_debug_libm answers atan2 and the heading's sin / cos, ca_oracle_set_libm feeds
    them to the oracle), the library is built without contraction and the oracle states the reference's numpy operation order,
    so the expected result is equality, not a tolerance: after every step positions, velocities, heading (not modulo anything),
    goal, turning_dir, remaining time and clock, the flag words, last_action, the recorded actions, the rewards and the WHOLE
    observation (the oracle's float64 row cast to float32) are compared as words.  The one difference let through, counted and
    printed, is the sign of a p_parallel / p_orth that is zero on both sides (_Diff.same_obs says where it comes from).  On the first step the values the scene fixes
    must be the scene's own.  The launch must be the intended instantiation and the device's fault word must stay zero.
(b) The same three steps from one rollout(3) and, where no external action is needed, from a look-ahead ring of 3 -- the MULTI
    instantiations -- equal the single steps bit for bit.
(c) sincos_heading against np.longdouble on the operands and at the bars of tests/sincos_ref.py, from ONE launch.

With CAGPU_TEST_DUMP_DIR set to an existing directory a failing case leaves its inputs there."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import move_scenes as M
from tests import orca_scenes as S
from tests import sincos_ref as SR
from tests.device_libm import GpuLibm, step_resolved
from tests.test_gpu_parity import _download, _mods, _upload
from tests.test_gpu_step_rule_edges import _bits, _pattern, _same

pytestmark = pytest.mark.gpu

STEPS = 3
SHAPE = {"pipelined": (10, 9), "tiled": (7, 19), "gs16": (13, 9), "wave": (33, 3), "big": (65, 3)}
assert all(ne in S.PATHS[path] for path, ne in SHAPE.items())
STATE = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "turning_dir", "time_remaining", "t")
FLAG_BITS = 0xFF      # the six agent-state flags and the two learning bits

_libm = GpuLibm()     # one table for the whole module: an operand is evaluated on the device once


def _cases():
    out = [(path, cls, v, N, E) for path, (N, E) in SHAPE.items() for cls in M.CLASSES for v in M.VARIANTS[cls]
           if N >= M.MIN_AGENTS[cls] and (path != "pipelined" or M.pipelined_eligible(cls, v))]
    for cls in M.CLASSES:      # every class on at least the tiled, wave and big paths; n and r on the pipelined one as well
        paths = {c[0] for c in out if c[1] == cls}
        assert {"tiled", "wave", "big"} <= paths and (cls not in "nr" or "pipelined" in paths), (cls, paths)
    return out


def _fused_cases():
    """one variant per class and path: the one that differs most from the defaults; class h with both dynamics"""
    pick = [("h", "unicycle"), ("h", "maxturn"), ("d", ""), ("m", "default"), ("a", "ga3c"), ("n", ""), ("r", "")]
    return [(path, cls, v, N, E) for path, (N, E) in SHAPE.items() for cls, v in pick]


def _pair(sc, pipeline):
    nat, core, orc = _mods()
    o = orc.Oracle(M.oracle_params(orc, sc))
    M.inject(o, sc)
    g = core.BatchedSim(core.make_params(sc.E, sc.N, **M.sim_kwargs(sc)), record_actions=True, pipeline=pipeline)
    _upload(o, g)
    return o, g


def _dump(name, sc, t, **arrays):
    d = os.environ.get("CAGPU_TEST_DUMP_DIR")
    if d and os.path.isdir(d):
        np.savez(os.path.join(d, "move_edges_%s_step%d.npz" % (name, t)), label=sc.label, case=sc.case, policy=sc.policy,
                 dynamics=sc.dynamics, turning_dir=sc.turning_dir, ext=sc.ext, **dict({n: getattr(sc, n) for n in S.Scene.FIELDS}, **arrays))


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


class _Diff(object):
    """word-for-word comparisons of one step, all of them reported together"""

    def __init__(self, what):
        self.what, self.lines, self.words, self.signed_zeros = what, [], 0, 0

    def same(self, name, got, want):
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
        bad = _words(got) != _words(want)
        self.words += int(bad.size)
        if bad.any():
            at = np.argwhere(bad)[:4].tolist()
            self.lines.append("%s: %d of %d words differ, first at %s: got %s want %s" % (
                name, int(bad.sum()), bad.size, at, got[bad][:4].tolist(), want[bad][:4].tolist()))

    def same_obs(self, got, want, K):
        """the whole observation as words.  One difference is let through, counted and printed: a p_parallel or p_orth that is
        zero on both sides with the other sign.  The kernels that take one item per UNORDERED pair (the pipelined kernel, the
        tiled kernel with the agent count compiled in) form the second host's `other - host` as -(rx, ry), which is exact
        except that -(+0) is -0 where the reference's own subtraction gives +0; a product with that zero then carries the
        other sign into a sum of zeros (DESIGN.md section 5 has the two orders side by side).  The values are equal."""
        bad = _words(got) != _words(want)
        col = np.zeros(got.shape[-1], bool)
        for k in range(K):
            col[6 + 7 * k:6 + 7 * k + 2] = True
        zeros = bad & (got == 0.0) & (want == 0.0) & col
        self.signed_zeros += int(zeros.sum())
        self.same("obs", np.where(zeros, want, got), want)

    def check(self):
        assert not self.lines, "%s:\n  %s" % (self.what, "\n  ".join(self.lines))


@pytest.mark.parametrize("path,cls,variant,N,E", _cases(), ids=lambda v: str(v) if v != "" else "-")
def test_move_on_angle_edge_scenes_bit_for_bit(path, cls, variant, N, E):
    nat, core, orc = _mods()
    sc = M.build(cls, N, E, variant)
    o, g = _pair(sc, path == "pipelined")
    ext = M.ext_actions(sc)
    ext_dev = None if ext is None else torch.from_numpy(ext).to(g.device)
    pattern = _pattern(path, N, E, False)
    name = "%s_%s%s_%d" % (path, cls, "_" + variant if variant else "", N)
    words = fixed = zeros = 0
    orc.set_libm(_libm.atan2, _libm.sincos)
    try:
        for t in range(STEPS):
            if t:
                _download(g, o)
            step_resolved(o, _libm, lambda: M.oracle_step(orc, o, ext))
            g.step(ext_dev)
            kern = nat.lib().cagpu_last_kernel().decode()
            assert re.match(pattern, kern), (kern, pattern)
            gs = {n: g.state[n].cpu().numpy() for n in STATE + ("flags", "last_action", "step_num", "episode_step")}
            gobs, grew, gact = g.obs.cpu().numpy(), g.rewards.cpu().numpy(), g.actions.cpu().numpy()
            d = _Diff("%s step %d" % (name, t))
            for n in STATE:
                d.same(n, gs[n], o.view(n))
            d.same("flags", gs["flags"].astype(np.uint32) & FLAG_BITS, o.view("flags") & FLAG_BITS)
            d.same("last_action", gs["last_action"], o.s["last_action"].reshape(E, N, 2))
            d.same("actions", gact, o.actions)
            d.same("rewards", grew, o.rewards.astype(grew.dtype))
            d.same_obs(gobs, o.obs.astype(np.float32), sc.max_obs)
            d.same("done", g.done.cpu().numpy().astype(np.uint8), o.done)
            d.same("game_over", g.game_over.cpu().numpy().astype(np.uint8), o.game_over)
            d.same("step_num", gs["step_num"], o.view("step_num"))
            d.same("episode_step", gs["episode_step"], o.s["episode_step"])
            if t == 0:      # what the scene fixes is the scene's own
                for label, got, want in (("heading", gs["heading"], sc.expect_heading), ("turning_dir", gs["turning_dir"], sc.expect_td),
                                         ("action", gact, sc.expect_action), ("dist_to_goal", gobs[..., 2], sc.expect_dist.astype(np.float32))):
                    held = ~np.isnan(want)
                    d.same("the scene's " + label, got[held], want[held])
                    fixed += int(held.sum())
                d.same("the scene's at-goal flags", gs["flags"].astype(np.uint32) & M.AT_GOAL, sc.expect_flags)
            try:
                d.check()
            except AssertionError:
                _dump(name, sc, t, obs=gobs, rewards=grew, actions=gact, want_obs=o.obs, want_actions=o.actions,
                      **{"got_" + n: gs[n] for n in STATE}, **{"want_" + n: o.view(n) for n in STATE})
                raise
            words += d.words
            zeros += d.signed_zeros
    finally:
        orc.set_libm()
    assert fixed > 0
    assert nat.device_faults(clear=True) == 0
    print("move-edges %-9s %s %-8s N=%-3d E=%-2d: %6d words equal the oracle on the device's libm in %d steps, %4d fixed by the scene, "
          "%d zeros of p_parallel / p_orth with the other sign" % (path, cls, variant or "-", N, E, words, STEPS, fixed, zeros))


@pytest.mark.parametrize("path,cls,variant,N,E", _fused_cases(), ids=lambda v: str(v) if v != "" else "-")
def test_fused_steps_equal_single_steps_on_angle_edge_scenes(path, cls, variant, N, E):
    nat, core, orc = _mods()
    sc = M.build(cls, N, E, variant)
    ext = M.ext_actions(sc)
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
    if path != "big":      # (the large-env kernel takes a rollout as n launches of the single step)
        assert re.match(_pattern(path, N, E, False, multi=True), kern), kern
    _same(want, _bits(r, (r.obs, r.rewards, r.done, r.game_over)), "rollout(3) %s %s" % (path, cls))
    # (c) a look-ahead ring of three slots (no external actions in a ring)
    if ext is None:
        o, k = _pair(sc, path == "pipelined")
        k.enable_lookahead(STEPS, fresh=True)
        for t in range(STEPS):
            obs, rew, done, over = k.step_lookahead()
            for x, y, n in zip((obs, rew, done, over), single[t], ("obs", "rewards", "done", "game_over")):
                assert x.cpu().numpy().astype(y.cpu().numpy().dtype).tobytes() == y.cpu().numpy().tobytes(), "ring slot %d %s" % (t, n)
        kern = nat.lib().cagpu_last_kernel().decode()
        if path != "big":
            assert re.match(_pattern(path, N, E, False, multi=True), kern), kern
        _same(want, _bits(k, (obs, rew, done, over)), "ring of 3 %s %s" % (path, cls))
    assert nat.device_faults(clear=True) == 0
    print("move-edges fused %-9s %s %-8s N=%-3d E=%-2d: rollout(3)%s equal three single steps bit for bit" % (
        path, cls, variant or "-", N, E, "" if ext is not None else " and a ring of 3"))


def test_sincos_heading_against_long_double():
    nat, core, orc = _mods()
    x = SR.operands()
    s, c = nat.debug_libm(1, x)      # one launch
    m = SR.measure(x, s, c)
    print("move-edges " + SR.report(m))
    SR.check(m)
