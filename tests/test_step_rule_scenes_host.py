"""The threshold scenes of tests/step_rule_scenes.py held to their purpose on the CPU, before tests/test_gpu_step_rule_edges.py
runs the step kernels on them:
  (1) purpose: on the very scenes the GPU test runs, the oracle's own outcome is what each agent's label says -- every one of
      the neighbouring kinds takes its own branch -- the number of agents per branch is printed and must be above zero, and the
      construction principle holds (nobody moves, every heading is 0, goals on y = const);
  (2) the oracle against the REFERENCE: tests/golden/step_rules.npz was recorded by oracle/gen_step_rule_golden.py from the
      unmodified reference on every class and variant at N in {2, 4, 6, 10, 20}, 3 envs, three steps.  Flags, done, game over,
      num_other_agents_observed and who sits in every observation slot are exact, floats within TOL, nothing excluded (the
      observations are recorded in float32, in which every radius of the scenes is still distinct);
  (3) the oracle at the large shapes (N = 33, 64, 65, 100: no golden) against a plain float64 restatement of the sensor's
      ranking (step_rule_scenes.sensor_order: OtherAgentsStatesSensor.py:20-55 with Python's sorted) and of the reward rule
      (collision_avoidance_env.py:394-512, below), exact in order and masks."""
import math
import os

import numpy as np
import pytest

from oracle import ca_oracle as orc
from tests import orca_scenes as S
from tests import step_rule_scenes as R

TOL = 1e-5      # the suite's bar for floats (tests/test_gpu_parity.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_rules.npz")
GOLDEN_N = (2, 4, 6, 10, 20)
BITS = R.AT_GOAL | R.WAS_AT_GOAL | R.IN_COLLISION | R.WAS_IN_COLLISION | R.OUT_OF_TIME | R.DONE


def _oracle(sc):
    o = orc.Oracle(R.oracle_params(orc, sc))
    R.inject(o, sc)
    if sc.static_map is not None:
        o.set_map(sc.static_map, rows=R.MAP_ROWS, cols=R.MAP_COLS, cell=R.MAP_CELL)
    return o


def _snap(o):
    return {k: o.s[k].copy() for k in ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "flags")}


CASES = [(cls, v, N, E) for N, E in S.SHAPES for cls in R.CLASSES for v in R.VARIANTS[cls] if N >= R.MIN_AGENTS[cls]]


def test_scenes_are_deterministic_prefixes():
    for cls in R.CLASSES:
        for v in R.VARIANTS[cls][:2]:
            a, b = R.build(cls, 6, 3, v), R.build(cls, 6, 5, v)
            for n in S.Scene.FIELDS + ("flags", "policy", "ext", "time_remaining", "label"):
                assert np.array_equal(getattr(b, n)[:3], getattr(a, n)), (cls, v, n)
            assert a.max_obs == b.max_obs and a.params == b.params


def test_every_branch_is_taken_and_nobody_moves():
    counts = {cls: {} for cls in R.CLASSES}
    for cls, v, N, E in CASES:
        sc = R.build(cls, N, E, v)
        o = _oracle(sc)
        before = _snap(o)
        o.step(R.ext_actions(sc))
        after = _snap(o)
        R.check_principle(sc, before, after)
        rew, fl = o.rewards, after["flags"].reshape(E, N)
        care = ~np.isnan(sc.expect_reward)
        assert (np.abs(rew - np.nan_to_num(sc.expect_reward))[care] < 0.025).all(), (cls, v, N, np.argwhere(
            care & (np.abs(rew - np.nan_to_num(sc.expect_reward)) >= 0.025))[:4], rew[care][:8], sc.expect_reward[care][:8])
        mask = np.uint32(R.AT_GOAL | R.IN_COLLISION | R.OUT_OF_TIME)
        assert not (((fl & mask) != sc.expect_flags) & sc.expect_care).any(), (cls, v, N)
        for lab in R.LABELS[cls]:
            counts[cls][lab] = counts[cls].get(lab, 0) + int((sc.label == lab).sum())
        if cls in "tcgow":      # the three neighbouring kinds sit in every scene, each on its own side
            for lab in (1, 2, 3):
                here = sc.label == lab
                assert here.any() or cls in "go" and N == 2, (cls, v, N, lab)      # (g, o at N = 2: the touched labels 4 - 6 take some)
        if cls == "o":
            over = o.game_over.astype(bool)
            done = o.done.astype(bool)
            if v == "all":
                assert np.array_equal(over, done.all(1))
            elif v == "agent0":
                assert np.array_equal(over, done[:, 0])
                assert (done[:, 0] & ~done.all(1)).any() or N == 2      # only agent 0's being done ends it
            else:
                learner = (sc.flags & R.STILL_LEARNING) != 0
                assert over[~learner.any(1)].all() and (~learner.any(1)).any()      # np.all([]) is True: over at once
                assert np.array_equal(over[learner.any(1)], (done | ~learner).all(1)[learner.any(1)])
        if cls == "s" and N >= 3:      # the host's list holds what the class says, and "below" cuts a tied group in two
            h, K = 1, sc.max_obs
            sort = v.split("-")[0]
            present = (sc.flags[0] & R.ABSENT) == 0
            full = R.sensor_order(sc.pos_x[0], sc.pos_y[0], sc.radius[0], present, h, "tti" if sort == "tti" else "first", N, R.HORIZON)
            keys = [R.tie_key(sc, 0, h, j) for j in full]
            assert len(set(keys)) < len(keys), "no tie in the host's list"
            if v.endswith("below"):
                assert keys[K - 1] == keys[K], (cls, v, N, K)
            if N >= 8:
                role = R._sensor_roles(N)
                assert [R.tie_key(sc, 0, h, role[r])[0] for r in ("X", "Y", "X2", "Y2")] == [0.12, 0.13, 0.38, 0.37]
                assert R.tie_key(sc, 0, h, role["Z"])[0] in (1.11, 1.12)
            if N >= 21:
                role = R._sensor_roles(N)
                assert role["F0"] in full and role["F2"] in full and role["F1"] not in full      # at, inside, outside 40 m
        # the second and third step: what has collided / arrived is paid the time-step reward and nothing else
        for t in (1, 2):
            was = after["flags"].reshape(E, N)
            o.step(R.ext_actions(sc))
            now = o.s["flags"].reshape(E, N)
            settled = (was & (R.IN_COLLISION | R.AT_GOAL)) != 0
            present = (sc.flags & R.ABSENT) == 0
            assert (o.rewards[settled & present] == R.R_TIME).all(), (cls, v, N, t)
            assert ((now[(was & R.IN_COLLISION) != 0] & R.WAS_IN_COLLISION) != 0).all()
            assert ((now[(was & R.AT_GOAL) != 0] & R.WAS_AT_GOAL) != 0).all()
            after = _snap(o)
    for cls in R.CLASSES:
        print("step-rule scenes %s: agents per branch %s" % (cls, {R.LABELS[cls][k]: n for k, n in sorted(counts[cls].items())}))
        assert all(n > 0 for n in counts[cls].values()), (cls, counts[cls])


# ---------------------------------------------------------------- (3) the large shapes against a plain restatement
def _hits_wall(sc, x, y, radius):
    """collision_avoidance_env.py:494-506 with Map.py:26-32 (cell of the centre, in_map) and :52-56 (the disc's mask)"""
    m, cell = sc.static_map, R.MAP_CELL
    origin = ((R.MAP_ROWS * cell / 2.) / cell, (R.MAP_COLS * cell / 2.) / cell)
    gx, gy = int(np.floor(origin[0] - y / cell)), int(np.floor(origin[1] + x / cell))
    if not (gx >= 0 and gy >= 0 and gx < m.shape[0] and gy < m.shape[1]):
        return False
    xs, ys = np.arange(0, m.shape[1]), np.arange(0, m.shape[0])
    mask = (xs[np.newaxis, :] - gy) ** 2 + (ys[:, np.newaxis] - gx) ** 2 < (radius / cell) ** 2
    return bool(np.any(m[mask]))


def _reward_rule(sc, e, flags0, time_remaining):
    """collision_avoidance_env.py:394-512 and agent.py:150-153, :235-239 for one env whose agents stand still: float64,
    Python loops in the reference's order -> rewards, flag words"""
    N, p = sc.N, sc.params
    P = [i for i in range(N) if not (flags0[i] & R.ABSENT)]
    fl = {i: int(flags0[i]) for i in P}
    for i in P:      # agent.py:202-241
        if fl[i] & (R.AT_GOAL | R.OUT_OF_TIME | R.IN_COLLISION):
            continue
        gx, gy = sc.pos_x[e, i] - sc.goal_x[e, i], sc.pos_y[e, i] - sc.goal_y[e, i]
        if gx ** 2 + gy ** 2 <= 0.2 ** 2:
            fl[i] |= R.AT_GOAL
        if time_remaining[i] - R.DT <= 0.0:
            fl[i] |= R.OUT_OF_TIME
    coll, nearest = {i: False for i in P}, {i: math.inf for i in P}
    for a in range(len(P)):      # env.py:476-493
        for b in range(a + 1, len(P)):
            i, j = P[a], P[b]
            d = math.sqrt((sc.pos_x[e, i] - sc.pos_x[e, j]) ** 2 + (sc.pos_y[e, i] - sc.pos_y[e, j]) ** 2)
            cr = sc.radius[e, i] + sc.radius[e, j]
            nearest[i], nearest[j] = min(nearest[i], d - cr), min(nearest[j], d - cr)
            if d <= cr:
                coll[i] = coll[j] = True
    rew = np.zeros(N)
    for i in P:      # env.py:411-453
        r = p.get("reward_time_step", 0.0)
        if fl[i] & R.AT_GOAL:
            if not fl[i] & R.WAS_AT_GOAL:
                r = R.R_GOAL
        elif not fl[i] & R.WAS_IN_COLLISION:
            if coll[i]:
                r, fl[i] = R.R_COLL, fl[i] | R.IN_COLLISION
            elif sc.static_map is not None and _hits_wall(sc, sc.pos_x[e, i], sc.pos_y[e, i], sc.radius[e, i]):
                r, fl[i] = p["reward_collision_wall"], fl[i] | R.IN_COLLISION
            else:
                if nearest[i] <= p.get("getting_close_range", 0.2):
                    r = -0.1 - nearest[i] / 2.0
                if abs(float(np.float32(sc.ext[e, i, 1]))) > p.get("wiggly_threshold", math.inf):
                    r += p.get("reward_wiggly", 0.0)
        rew[i] = min(max(r, R.R_COLL), R.R_GOAL)
        if fl[i] & (R.AT_GOAL | R.OUT_OF_TIME | R.IN_COLLISION):
            fl[i] |= R.DONE
    return rew, fl


LARGE = [(cls, v, N, E) for cls, v, N, E in CASES if N in (33, 64, 65, 100)]


@pytest.mark.parametrize("cls,variant,N,E", LARGE, ids=lambda v: str(v) if v != "" else "-")
def test_oracle_at_large_shapes_against_plain_restatement(cls, variant, N, E):
    sc = R.build(cls, N, E, variant)
    o = _oracle(sc)
    o.step(R.ext_actions(sc))
    fl = o.s["flags"].reshape(E, N)
    K, sort = sc.max_obs, (variant.split("-")[0] if cls == "s" else "first")
    slots = 0
    for e in range(E):
        rew, want = _reward_rule(sc, e, sc.flags[e], sc.time_remaining[e])
        for i, w in want.items():
            assert (int(fl[e, i]) & BITS) == (w & BITS), (e, i, hex(int(fl[e, i])), hex(w))
        present = (sc.flags[e] & R.ABSENT) == 0
        assert np.array_equal(o.rewards[e][present], rew[present]), (e, o.rewards[e], rew)
        for a in np.nonzero(present)[0]:
            order = R.sensor_order(sc.pos_x[e], sc.pos_y[e], sc.radius[e], present, a, sort, K,
                                   sc.params.get("sensing_horizon", math.inf), goal=(sc.goal_x[e, a], sc.goal_y[e, a]))
            row = o.obs[e, a]
            assert int(row[1]) == len(order), (e, a, row[1], len(order))
            got = row[6:].reshape(K, 7)[:len(order), 4]
            assert np.array_equal(got, sc.radius[e, order]), (e, a, order[:8], got[:8])      # who sits in every slot
            slots += len(order)
    if cls == "s" and N > 64:      # the ties at indices 63 / 64 and 0 / N - 1 are ties, and the index decides them
        h, e = 1, 0
        present = (sc.flags[e] & R.ABSENT) == 0
        order = R.sensor_order(sc.pos_x[e], sc.pos_y[e], sc.radius[e], present, h, "first", N, R.HORIZON)
        pairs = [(63, 64)] + ([(0, N - 1)] if N > 65 else [])
        for a, b in pairs:
            assert sc.pos_y[e, a] == sc.pos_y[e, b] and sc.pos_x[e, a] == -sc.pos_x[e, b]
            assert order.index(b) == order.index(a) + 1, (a, b, order[:16])
    print("step-rule scenes %s %-12s N=%-3d: %d envs, %d slots equal the plain restatement" % (cls, variant or "-", N, E, slots))


# ---------------------------------------------------------------- (2) the oracle against the reference
_gold = {}


def _golden():
    if not _gold:
        from oracle import gen_step_rule_golden as G
        _gold.update(G.load(GOLDEN))
    return _gold


GOLD_CASES = [(cls, v, N) for cls in R.CLASSES for v in R.VARIANTS[cls] for N in GOLDEN_N]


@pytest.mark.parametrize("cls,variant,N", GOLD_CASES, ids=lambda v: str(v) if v != "" else "-")
def test_oracle_equals_the_reference_on_recorded_scenes(cls, variant, N):
    z = _golden()["%s_%s_%d" % (cls, variant or "-", N)]
    E = 3
    sc = R.build(cls, N, E, variant)
    o = _oracle(sc)
    K, W = sc.max_obs, 6 + 7 * sc.max_obs
    excluded = compared = 0
    for t in range(3):
        o.step(R.ext_actions(sc))
        fl = o.s["flags"].reshape(E, N)
        for e in range(E):
            P = np.nonzero((sc.flags[e] & R.ABSENT) == 0)[0]
            st = z["state"][t, e][:len(P)]          # [agent, 15] as oracle/gen_golden.py _snapshot lays it out
            what = "%s %s N=%d step %d env %d" % (cls, variant, N, t, e)
            assert np.array_equal(z["flags"][t, e][:len(P)] & BITS, fl[e, P] & BITS), "flags " + what
            assert np.array_equal(z["done"][t, e][:len(P)], o.done[e, P]), "done " + what
            assert bool(z["game_over"][t, e]) == bool(o.game_over[e]), "game over " + what
            for c, n in enumerate(("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed",
                                   "time_remaining", "t")):
                np.testing.assert_allclose(o.view(n)[e, P], st[:, c], rtol=0, atol=TOL, err_msg=n + " " + what)
            ref_obs, mine = z["obs"][t, e][:len(P)], o.obs[e, P].astype(np.float32)     # (recorded in float32)
            assert np.array_equal(ref_obs[:, 1], mine[:, 1]), "num_other_agents_observed " + what
            assert np.array_equal(ref_obs[:, 6:].reshape(len(P), K, 7)[..., 4:6],
                                  mine[:, 6:].reshape(len(P), K, 7)[..., 4:6]), "who sits in a slot " + what
            np.testing.assert_allclose(mine, ref_obs, rtol=0, atol=TOL, err_msg="obs " + what)
            rr = z["rewards"][t, e][:len(P)]
            held = ~np.isnan(rr)                         # (TRAIN_SINGLE_AGENT, game_over_mode agent0: the reference returns agent 0's only)
            np.testing.assert_allclose(o.rewards[e, P][held], rr[held], rtol=0, atol=TOL, err_msg="rewards " + what)
            compared += len(P)
    assert compared > 0 and excluded == 0
