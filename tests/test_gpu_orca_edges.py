"""The ORCA phases of the STEP kernels against the oracle, bit for bit, on the crowded and degenerate scenes of
tests/orca_scenes.py (what each class is for and that the oracle is right on them: tests/test_orca_scenes_host.py), on every
launch path: the pipelined kernel (plan beside the previous step's sensing half, lp3_wave8), the tiled kernel with N <= 10
(branch-free half-planes, 1-D programmes solved in advance, lp3_wave8), 11 <= N <= 16 (lp3_group<16>), N > 16 (one wave per
querying agent) and the large-env kernel (serial programme over the workspace).  A scene is injected into oracle and sim, both
step once, then three more times from the GPU's own bits (the collided agents are then done, stationary neighbours; the agents
of the near-overlap band stay live).  After every step CaOut.orca_vel must equal the oracle's velocities word for word: no
allowance, nothing excluded.  The usual state / observation comparison is kept, the launch must be the intended
instantiation, and the device's fault word must stay zero.  With CAGPU_TEST_DUMP_DIR set to an existing directory a failing
case leaves its inputs there (see _dump) for a diagnosis on the host."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import orca_scenes as S
from tests.test_gpu_parity import _compare, _download, _mods, _upload

pytestmark = pytest.mark.gpu

STEPS = 4


def _kernel_pattern(path, N, E):
    if path == "pipelined":
        return r"ca_pipe_kernel<%d, %d, false> grid=3 " % (N, S.PIPE_TILE[N])
    if path == "big":
        return r"ca_big_kernel grid=%d " % E      # (one workgroup per env: the workspace holds them all)
    nt = 512 if N > 32 else 256
    nc, te = (10, 4) if N == 10 else ((20, 0) if N == 20 else (0, 0))
    return r"ca_kernel<%d, (true|false), %d, false, false, %d> grid=3 .* tile_envs=%d$" % (nt, nc, te, S.tiled_envs(N))


def _cases():
    out = []
    for path, shapes in S.PATHS.items():
        for N, E in shapes:
            for cls in S.CLASSES:
                if path == "pipelined" and cls == "h":
                    continue      # (a per-agent collaboration array is a per-step input: the pipelined kernel is not eligible)
                out.append((path, cls, N, E, ""))
                if cls == "e" and N > 4:      # (N <= 4: at most one neighbour is in range anyway)
                    out.append((path, cls, N, E, "one_neighbour"))
    out += [("pipelined", cls, N, E, "plan_first") for cls, (N, E) in zip("abcdg", S.PATHS["pipelined"][2:])]
    return out


def _dump(name, o, pre, got, want, t):
    """CAGPU_TEST_DUMP_DIR=<existing directory>: where a failing case leaves the pre-step state and both velocity arrays"""
    d = os.environ.get("CAGPU_TEST_DUMP_DIR")
    if d and os.path.isdir(d):     # the inputs of the differing queries, for a diagnosis on the host
        np.savez(os.path.join(d, "orca_edges_%s_step%d.npz" % (name, t)), got=got, want=want, **pre)


@pytest.mark.parametrize("path,cls,N,E,variant", _cases(), ids=lambda v: str(v) if v != "" else "-")
def test_step_kernel_orca_on_edge_scenes_bit_exact(path, cls, N, E, variant):
    nat, core, orc = _mods()
    sc = S.build(cls, N, E, max_neighbors=1 if variant == "one_neighbour" else None)
    o = orc.Oracle(S.oracle_params(orc, sc))
    S.inject(o, sc)
    g = core.BatchedSim(core.make_params(E, N, rvo_max_neighbors=sc.params.get("rvo_max_neighbors"),
                                         sensing_horizon=sc.params.get("sensing_horizon", np.inf),
                                         ragged=sc.params.get("ragged", 0)),
                        record_actions=True, pipeline=(path == "pipelined"))
    g.set_plugins(nat.POL_RVO)
    _upload(o, g)
    collab = None
    if sc.collab is not None:
        collab = torch.from_numpy(sc.collab).to(g.device)
        g._cs.rvo_collab = collab.data_ptr()
    plan_bit = lambda: (g.state["flags"].cpu().numpy().reshape(-1) >> 17) & 1
    assert not plan_bit().any()                      # an upload forgets the plan: the first step queries in the step itself
    if variant == "plan_first":
        assert g.try_plan() and plan_bit().all()     # ... unless the plan is asked for ahead of it
    pattern = _kernel_pattern(path, N, E)
    compared = differing = excluded = 0
    name = "%s_%s_%d%s" % (path, cls, N, "_" + variant if variant else "")
    for t in range(STEPS):
        if t:
            _download(g, o)
        live = (o.s["flags"] & (orc.DONE | orc.ABSENT)) == 0
        pre = {k: o.s[k].copy() for k in ("pos_x", "pos_y", "vel_x", "vel_y", "goal_x", "goal_y", "radius", "pref_speed", "flags")}
        o.step()
        g.step()
        kern = nat.lib().cagpu_last_kernel().decode()
        assert re.match(pattern, kern), (kern, pattern)
        if path == "pipelined":
            assert plan_bit().all()                  # the following steps take the planned query
        got, want = g.orca_vel.cpu().numpy().reshape(-1, 2), o.orca_vel.reshape(-1, 2)
        bad = got.view(np.uint32) != want.view(np.uint32)
        held = np.ones(bad.shape, bool)                # every word is held to the oracle: no mask
        compared += int(held[live].sum())
        excluded += int((~held)[live].sum())
        differing += int(bad.sum())
        if bad.any():
            _dump(name, o, pre, got, want, t)
            rows = np.nonzero(bad.any(axis=1))[0]
            assert False, "%s step %d: %d of %d ORCA velocity words differ (max %g); agents %s got %s want %s" % (
                name, t, bad.sum(), 2 * live.sum(), np.nanmax(np.abs(got - want)), rows[:6], got[rows[:6]], want[rows[:6]])
        _compare(o, g, what="%s step %d" % (name, t))
    assert compared > 0 and excluded == 0
    assert nat.device_faults(clear=True) == 0
    print("orca-edges %-9s %s N=%-3d E=%-2d %-13s compared %4d differing %d excluded %d" % (path, cls, N, E, variant or "-", compared, differing, excluded))
    del collab
