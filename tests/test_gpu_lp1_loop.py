"""The 1-D programme loop of the pipelined step kernels (p2b_round, csrc/cagpu_pipe.inc: two lines per iteration on whole
float4 rows, wave-uniform row addressing, the interval rule of csrc/cagpu_lp1.inc) at the smallest shapes where it can go wrong,
held to the oracle bit for bit the way tests/test_gpu_orca_edges.py holds the ORCA phases:

  * N = 10 with E = 4 (one full tile) and E = 5 (a partial second tile); with all 40 agents of a tile planned the items of the
    1-D programmes (40 x 9 = 360) do not fit one round of the four O waves, so the S-pair helper round (items 256 - 359) runs;
  * N = 2 and N = 3: the loop runs 0 or 1 iterations and the second line of the only pair is unused; N = 5: an odd highest line;
  * rvo_max_neighbors < N - 1 (class c), a finite sensing horizon (class e, also with one neighbour) and a ragged batch (class
    g): rows at or beyond an agent's neighbour count hold stale lines of an earlier step, which the uniform row addressing
    reads and must not use;
  * single steps (the plan of step t + 1 computed beside step t, and the pre-move pass of a tile without a plan), the fused
    rollout and the look-ahead ring, over a window that contains an auto-reset.

Scenes come from tests/orca_scenes.py; every ORCA velocity word must equal the oracle's, the state / observation comparison
of tests/test_gpu_parity.py is kept, and the device's fault word must stay zero."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import golden_util as gu
from tests import orca_scenes as S
from tests.test_gpu_bench_geometry import Block
from tests.test_gpu_parity import F64, _compare, _download, _mods, _upload

pytestmark = pytest.mark.gpu

STEPS = 4
STATE = F64 + ("last_action", "flags", "step_num", "episode_step", "reset_count", "env_stats")

#        N   E   classes
SHAPES = [(10, 4, "abceg"), (10, 5, "abceg"), (2, 33, "ab"), (3, 22, "abcg"), (5, 13, "bcg")]


def _scene_cases():
    out = []
    for N, E, classes in SHAPES:
        for cls in classes:
            out.append((cls, N, E, ""))
            if cls == "e":
                out.append((cls, N, E, "one_neighbour"))
        out.append(("b", N, E, "plan_first"))
    return out


@pytest.mark.parametrize("cls,N,E,variant", _scene_cases(), ids=lambda v: str(v) if v != "" else "-")
def test_single_steps_on_scenes_bit_exact(cls, N, E, variant):
    nat, core, orc = _mods()
    sc = S.build(cls, N, E, max_neighbors=1 if variant == "one_neighbour" else None)
    o = orc.Oracle(S.oracle_params(orc, sc))
    S.inject(o, sc)
    g = core.BatchedSim(core.make_params(E, N, rvo_max_neighbors=sc.params.get("rvo_max_neighbors"),
                                         sensing_horizon=sc.params.get("sensing_horizon", np.inf),
                                         ragged=sc.params.get("ragged", 0)),
                        record_actions=True, pipeline=True)
    g.set_plugins(nat.POL_RVO)
    _upload(o, g)
    plan_bit = lambda: (g.state["flags"].cpu().numpy().reshape(-1) >> 17) & 1
    if variant == "plan_first":
        assert g.try_plan() and plan_bit().all()
    grid = (E + S.PIPE_TILE[N] - 1) // S.PIPE_TILE[N]
    compared = 0
    for t in range(STEPS):
        if t:
            _download(g, o)
        live = (o.s["flags"] & (orc.DONE | orc.ABSENT)) == 0
        if cls == "b" and N == 10 and t == 0:
            assert live.reshape(E, N)[:4].all()      # a full tile of 40 planned agents: the helper round of the 1-D programmes
        o.step()
        g.step()
        kern = nat.lib().cagpu_last_kernel().decode()
        assert kern.startswith("ca_pipe_kernel<%d, %d, false> grid=%d " % (N, S.PIPE_TILE[N], grid)), kern
        assert plan_bit().all()
        got, want = g.orca_vel.cpu().numpy().reshape(-1, 2), o.orca_vel.reshape(-1, 2)
        bad = got.view(np.uint32) != want.view(np.uint32)
        print("lp1-loop %s N=%d E=%d %s step %d: live %d, differing words %d" % (cls, N, E, variant or "-", t, live.sum(), bad.sum()))
        rows = np.nonzero(bad.any(axis=1))[0]
        assert not bad.any(), "step %d: %d ORCA velocity words differ; agents %s got %s want %s" % (
            t, bad.sum(), rows[:6], got[rows[:6]], want[rows[:6]])
        compared += int(live.sum())
        _compare(o, g, what="%s N=%d E=%d step %d" % (cls, N, E, t))
    assert compared > 0
    assert nat.device_faults(clear=True) == 0


def _sim(N, E, table):
    nat, core, orc = _mods()
    g = core.BatchedSim(core.make_params(E, N, max_obs=N - 1), record_actions=True, pipeline=True)
    g.set_plugins(nat.POL_RVO, nat.DYN_UNICYCLE)
    g.set_fixture_table(table, env_id_offset=0, case_stride=E)
    g.reset_from_table()
    return g


@pytest.mark.parametrize("N,E", [(10, 4), (10, 5), (2, 33), (3, 22)])
def test_rollout_and_ring_equal_single_steps_across_an_auto_reset(N, E):
    """One launch per step, stepped by the oracle from the GPU's own bits (state within the usual tolerance, every ORCA
    velocity word of a queried agent exact) until an env has auto-reset and run on; then the same steps as fused rollouts and
    through the look-ahead ring: state and outputs identical to the single launches bit for bit."""
    nat, core, orc = _mods()
    table = gu.fixtures(N)
    a, b, c = _sim(N, E, table), _sim(N, E, table), _sim(N, E, table)
    warm = 40
    for g in (a, b, c):
        g.rollout(warm)
    blk = Block(a, 0, E, table, orc.POL_RVO)
    resets0 = int(a.state["reset_count"].sum())
    outs, T, after = [], 0, 0
    while (after < 6 or T < 12) and T < 700:
        blk.download()
        was_done = (blk.o.s["flags"] & (orc.DONE | orc.ABSENT)) != 0
        blk.step()
        obs, rew, over = a.step()
        assert nat.lib().cagpu_last_kernel().decode().startswith("ca_pipe_kernel<%d, %d, false>" % (N, S.PIPE_TILE[N]))
        got, want = a.orca_vel.cpu().numpy().reshape(-1, 2), blk.o.orca_vel.reshape(-1, 2)
        bad = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1) & ~was_done
        assert not bad.any(), "step %d: ORCA velocities of %d queried agents differ" % (T, bad.sum())
        blk.compare("N=%d E=%d step %d" % (N, E, T))
        outs.append((obs.clone(), rew.clone()))
        T += 1
        if int(a.state["reset_count"].sum()) > resets0:
            after += 1
    assert after >= 6, "no auto-reset within %d steps" % T
    print("lp1-loop rollout N=%d E=%d: %d steps, %d auto-resets" % (N, E, T, int(a.state["reset_count"].sum()) - resets0))
    # fused rollouts: the plan crosses launch boundaries
    left = T
    for n in (3, 1, 2):
        b.rollout(n)
        left -= n
    b.rollout(left)
    assert nat.lib().cagpu_last_kernel().decode().startswith("ca_pipe_kernel<%d, %d, true>" % (N, S.PIPE_TILE[N]))
    for n in STATE:
        assert torch.equal(a.state[n], b.state[n]), "rollout: %s" % n
    assert torch.equal(a.obs, b.obs) and torch.equal(a.rewards, b.rewards) and torch.equal(a.done, b.done)
    # the look-ahead ring, slot by slot
    c.enable_lookahead(5, fresh=True)
    for t in range(T):
        ob, rb, _, _ = c.step_lookahead()
        assert torch.equal(ob, outs[t][0]) and torch.equal(rb, outs[t][1]), "ring slot of step %d" % t
    for n in STATE:
        assert torch.equal(a.state[n], c.state[n]), "ring: %s" % n
    assert nat.device_faults(clear=True) == 0
