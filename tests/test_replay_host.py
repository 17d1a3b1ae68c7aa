"""The host-only planner of a replay (gym_collision_avoidance_amd/replay.py): the address formulas against their NumPy
restatement (tests/replay_ref.py), every refusal before any library call, the relabelling of the child's records -- and the
three scenarios of the GPU outcome test run through the CPU oracle, so that "all three outcomes were replayed" holds by
construction.  No GPU."""
import os
import sys
import types

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from gym_collision_avoidance_amd import _native as nat  # noqa: E402
from gym_collision_avoidance_amd import replay as rp  # noqa: E402
from tests import replay_ref as ref  # noqa: E402


class _NoLibrary(object):
    """a library every call of which fails the test: the planner must decide before it launches anything"""

    def __getattr__(self, name):
        raise AssertionError("library call %s before the refusal" % name)


def _sim(E=6, N=3, table=True, offset=0, stride=None, n_cases=11, stream=False, reset=True, words=None):
    """what the planner reads of a BatchedSim, and nothing else"""
    ar = None
    if table:
        ar = types.SimpleNamespace(env_id_offset=offset, case_stride=E if stride is None else stride, n_cases=n_cases,
                                   heading_seed=0)
    start = None
    if reset is not False:
        start = np.zeros((E, N, 7))
        if reset is not True:      # a bool mask: the envs that were reset
            start[~np.asarray(reset, bool)] = np.nan
    return types.SimpleNamespace(E=E, N=N, _ar=ar, _cstream={"off": offset} if stream else None, _rvo=None, _variants=[],
                                 _plugin_words=words, _draw=None, _start=start, lib=_NoLibrary())


# ---------------------------------------------------------------- 1. the formulas
@pytest.mark.parametrize("offset,stride,n_cases", [(3, 7, 11), ((1 << 32) - 40, 5, 13), (1001, 41, 23)])
def test_row_and_index_formulas_equal_the_restatement(offset, stride, n_cases):
    E = 6
    assert n_cases % stride and n_cases % E and stride != E     # (a stride that is not E, an n_cases neither divides)
    rng = np.random.default_rng(5)
    env = rng.integers(0, E, 64)
    ep = np.concatenate([rng.integers(0, 50, 60), [0, 1, (1 << 31) - 1, 1 << 30]])
    want_row = ref.table_row(offset, env, ep, stride, n_cases)
    want_idx = ref.stream_index(offset, env, ep)
    assert np.array_equal(rp.table_row(offset, env, ep, stride, n_cases), want_row)
    assert np.array_equal(rp.stream_index(offset, env, ep), want_idx)
    pl = rp.plan(_sim(E=E, offset=offset, stride=stride, n_cases=n_cases), env, ep)
    assert np.array_equal(pl["row"], want_row) and np.array_equal(pl["case"], want_row)
    assert np.array_equal(pl["global_env"], env + offset)
    pl = rp.plan(_sim(E=E, offset=offset, stride=E, n_cases=E * 4, stream=True), env, ep)
    assert np.array_equal(pl["case"], want_idx)
    assert np.array_equal(pl["row"], ref.table_row(offset, env, ep, E, E * 4))     # (the window row: the log's `case`)
    # ints are pairs of length one
    one = rp.plan(_sim(E=E, offset=offset, stride=stride, n_cases=n_cases), 2, 9)
    assert one["env"].tolist() == [2] and one["row"].tolist() == [(offset + 2 + 9 * stride) % n_cases]


@pytest.mark.parametrize("env,ep,why", [([0, 1], [0], "equal length"), ([6], [0], "outside"), ([-1], [0], "outside"),
                                        ([0], [-1], "episode numbers"), ([0.5], [0], "integers"), ([[0]], [[0]], "1-D")])
def test_bad_arguments_raise(env, ep, why):
    with pytest.raises(ValueError, match=why):
        rp.plan(_sim(), env, ep)


def test_global_env_ids_stay_below_2_to_the_32():
    with pytest.raises(ValueError, match="2\\^32"):
        rp.plan(_sim(offset=(1 << 32) - 3), [5], [1])
    rp.plan(_sim(offset=(1 << 32) - 6), [5], [1])


# ---------------------------------------------------------------- 2. the refusals
def _words(E, N, policy=nat.POL_RVO, dynamics=nat.DYN_UNICYCLE):
    pol = np.broadcast_to(np.asarray(policy, np.int64), (E, N))
    dyn = np.broadcast_to(np.asarray(dynamics, np.int64), (E, N))
    return ((pol << nat.POLICY_SHIFT) | (dyn << nat.DYNAMICS_SHIFT)).astype(np.int32)


def test_every_refusal_raises_before_any_library_call():
    E, N = 6, 3
    ok = _sim(E, N, words=_words(E, N))
    rp.plan(ok, [0, 5], [0, 3])                     # (the stub is accepted as it stands)

    def refused(match, sim=None, env=(1,), ep=(2,), **host):
        with pytest.raises(ValueError, match=match):
            rp.plan(_sim(E, N, words=_words(E, N)) if sim is None else sim, list(env), list(ep), **host)

    for pol in (nat.POL_EXTERNAL, nat.POL_LEARNING, nat.POL_LEARNING_GA3C):
        w = _words(E, N)
        w[1, 2] = _words(1, 1, pol)[0, 0]
        refused("external policy", _sim(E, N, words=w))
        rp.plan(_sim(E, N, words=w), [0], [2])      # (another env of the batch is not held to it)
    refused("user Python policies", host_policies=True)
    refused("custom Dynamics", host_dynamics=True)
    w = _words(E, N)
    w[1, 0] = _words(1, 1, nat.POL_RVO, nat.DYN_EXTERNAL)[0, 0]
    refused("custom Dynamics", _sim(E, N, words=w))
    s = _sim(E, N)
    s._rvo = {"gen": None}
    refused("stochastic RVO", s)
    s = _sim(E, N)
    s._variants = [("mask", 2, 0, None)]
    refused("sensor variants", s)
    s = _sim(E, N)
    s._draw = {"pool": np.array([nat.POL_RVO << nat.POLICY_SHIFT, nat.POL_EXTERNAL << nat.POLICY_SHIFT])}
    refused("external policy", s)
    refused("without a fixture table", _sim(E, N, table=False))
    rp.plan(_sim(E, N, table=False), [1], [0])      # (episode 0 needs no table)
    refused("never reset", _sim(E, N, reset=False), ep=(0,))
    refused("never reset", _sim(E, N, reset=np.array([1, 0, 1, 1, 1, 1], bool)), ep=(0,))
    rp.plan(_sim(E, N, reset=np.array([1, 0, 1, 1, 1, 1], bool)), [0, 1], [0, 4])   # (env 1's later episodes are derived)


# ---------------------------------------------------------------- 3. the relabelling
def test_relabelling_maps_child_rows_to_the_parent_labels():
    env, ep, row = np.array([4, 4, 0]), np.array([7, 0, 2]), np.array([9, 3, 5])
    child = {"env": np.array([2, 0, 1]), "episode": np.zeros(3, np.int64), "case": np.array([2, 0, 1]),
             "steps": np.array([12, 10, 11]), "outcome": np.array([2, 0, 1]),
             "total_reward": np.array([[2.0, 2.5], [0.0, 0.5], [1.0, 1.5]])}
    out = rp.relabel(child, env, ep, row, maps=np.array([1, 0, 2]))
    assert out["env"].tolist() == [4, 4, 0] and out["episode"].tolist() == [7, 0, 2] and out["case"].tolist() == [9, 3, 5]
    assert out["map"].tolist() == [1, 0, 2]
    assert out["steps"].tolist() == [10, 11, 12] and out["outcome"].tolist() == [0, 1, 2]     # (ordered by child env)
    assert out["total_reward"].tolist() == [[0.0, 0.5], [1.0, 1.5], [2.0, 2.5]]
    with pytest.raises(ValueError, match="one record"):
        rp.relabel({k: v[:2] for k, v in child.items()}, env, ep, row)


def test_step_bound_covers_the_time_budget():
    cases = np.zeros((2, 2, 6))
    cases[0, 0] = (0, 0, 3.2, 0, 1.0, 0.2)       # 3 m of straight line at 1 m/s, ratio 1.5: 4.5 s = 45 steps
    cases[0, 1] = (0, 1, 0.5, 1, 1.0, 0.2)
    cases[1, 0] = (0, 0, 1, 0, 0.5, 0.2)         # (row 1, slot 1 is empty)
    b = rp.step_bound(cases, 0.1, 0.2, 1.5)
    assert 45 <= b <= 48


# ---------------------------------------------------------------- 4. the outcome scenarios end as intended
def test_outcome_scenarios_end_as_intended_under_the_oracle():
    from oracle import ca_oracle as orc
    if not os.path.exists(orc.LIB_PATH):
        orc.build()
    table, pol, want = ref.outcome_table()
    E, N = table.shape[:2]
    o = orc.Oracle(orc.default_params(E, N, max_time_ratio=ref.OUTCOME_MAX_TIME_RATIO))
    o.set_policies(pol)
    o.reset(table)
    got = np.full(E, -1)
    for _ in range(rp.step_bound(table, 0.1, 0.2, ref.OUTCOME_MAX_TIME_RATIO)):
        o.step()
        fl = o.s["flags"].reshape(E, N)
        now = np.where((fl & 4).any(1), 0, np.where((fl & 1).all(1), 1, 2))
        got = np.where((got < 0) & (o.game_over != 0), now, got)
    assert np.array_equal(got, want), got
