"""Deterministic scenes (numpy only) that put the rules of a step ON their thresholds, for tests/test_step_rule_scenes_host.py
and tests/test_gpu_step_rule_edges.py: the collision test d <= r_i + r_j, nearest <= getting_close_range, |heading change| >
wiggly_threshold, q^2 <= near_goal_threshold^2, time_remaining <= 0, the wall test with its in-map gate, d > sensing_horizon, the
1 cm bucket rint(100 gap) with its ties (p_orth, then index) and the clip at max_obs.  build(cls, N, E, variant) -> Scene;
oracle_params(orc, scene); inject(o, scene) writes one into an oracle.Oracle, from where the GPU tests upload it.  Every env is
a function of (class, variant, N, env) alone, so a scene with fewer envs is a prefix of one with more.

THE CONSTRUCTION PRINCIPLE.  No result of sin, cos or atan2 feeds a threshold: every agent stands still during the step (an
ExternalPolicy agent whose commanded speed is 0 -- the static policy will not do, it moves the goal onto the agent and so puts it
at its goal; a LearningPolicy agent whose external action (0, 0.5) scales to speed 0, heading change 0), every heading is 0 before
the step, and every agent whose p_orth breaks a tie has its goal on the line y = const through it, 32 m away, so that ref_prll is
exactly (1, 0) and p_orth is the plain difference of two y coordinates.  Distances come from binary-exact coordinates (centres
(0, 0) and (0.75, 1.0) are 1.25 apart) or from a bisection over the float64 values of ONE coordinate (_solve) that finds the
position at which the rounded quantity, evaluated in the rule's own operation order, lands exactly on the threshold or on the
float64 next to it.  What a rule compares is then a chain of IEEE float64 +, -, *, / and sqrt of given numbers: it has one answer,
and masks, orders and slot contents are compared with nothing excluded.  (check_principle() below is what the host test runs.)

In each class the three neighbouring kinds are: ON the threshold, one ulp INSIDE, one ulp OUTSIDE, the ulp being that of the
quantity the rule rounds; the kinds rotate with (unit + env).  An env is a cross of UNITS (pairs, now and then a triple) 8 m apart
along the four half-axes, far outside each other's ranges (_Env.at).  Radii are 0.25 + i / 512 (distinct, binary exact) except where a class names
them.  Scene.label [E, N] says what an agent is there for (LABELS), Scene.expect_reward [E, N] the reward of the first step where
the class fixes it (NaN elsewhere), Scene.expect_flags / expect_care the flag bits of the first step.

Classes (VARIANTS lists their variants):
  t  touching: pairs at a centre distance exactly fl(r_i + r_j) and one ulp either side; radii binary exact, 0.625 + 0.625 (the
     3-4-5 triangle), 0.2 + 0.3, 0.3 + 0.2, 0.1 + 0.7.  Later steps: was_in_collision -> time-step reward, no close-range reward.
  c  close range: fl(d - fl(r_i + r_j)) exactly getting_close_range, and d one ulp (of d: the grid the difference moves on)
     either side; triples in which an agent has that
     gap to one neighbour and 1/16 m to another, in both index orders (the minimum counts, not the last gap seen).  Variant
     "clip": getting_close_range = 0.45, so that -0.1 - gap / 2 falls below reward_min = -0.25 and is clipped.
  g  goal: q^2 = fl(fl(gx^2) + fl(gy^2)) exactly fl(near_goal_threshold^2) and one ulp either side; in every other unit the
     partner's disc touches the agent in the same step (3-4-5 again): at its goal the agent takes the goal reward and no collision
     while the partner collides; outside it both collide.  Second step at the goal: time-step reward, WAS_AT_GOAL.
  o  time-out and game over: time_remaining = dt (out of time after one step), the float64 below it (likewise) and the one above
     (not yet); every other unit touches as well (time-out and collision in one step).  Variants "all", "agent0", "learning" =
     the three game_over_modes; under "learning" every second env has no still-learning agent (np.all of an empty list: over at
     once), the others have one LearningPolicy agent.
  w  wiggle: wiggly_threshold = 0.15625, reward_wiggly = -0.05; heading-change actions +-threshold and the float32 values next to
     it on both sides; every fourth unit also at a gap of 1/8 m (the wiggle reward is ADDED to the close-range one).
  m  walls: a 32 x 48 map of 0.125 m cells (a row of the bit-packed grid ends inside a word) with walls along the border and two
     single cells inside; discs whose bounding box leaves the map on each side, centres whose cell index is exactly 0 / rows - 1 /
     cols - 1, centres one ulp outside the map with the disc over a wall (in_map is False: no collision), coordinates for which
     origin -+ coord / cell is an integer, radius / cell = 4 exactly with the only wall cell 4 cells away (strict <: no hit) and 3
     cells away (hit), an agent that touches another agent and a wall (agent-collision reward; reward_collision_wall = -0.2).
  s  sensor order: host 1 at the origin, sensing_horizon = 40 m.  Around it: gaps at exact half buckets (0.125 -> 12 beside a
     candidate in bucket 13 that a round-half-up would overtake, 0.375 -> 38 beside one in bucket 37), 1.115 (x 100 rounds across
     the half), twelve candidates on the circle of radius 5 through (+-3, +-4) in ONE bucket with distinct p_orth, among them
     pairs (x, y), (-x, y) tied in bucket and p_orth (the index decides; N > 64: at indices 63 / 64 and 0 / N - 1), candidates at
     exactly 40 m and one ulp either side, the rest beyond the horizon.  Nobody moves, so every time to impact is infinite (0 for
     overlapping discs) and time_to_impact falls through to distance.  Every third env is ragged: its trailing N // 3 slots are
     absent.  Variants: sort mode x max_obs "below" (cuts a tied group of the host's list: one kept, one dropped), "equal"
     (N - 1), "above" (N + 1).

Which launch path runs what: pipelined_eligible() restates cagpu_launch.inc pipe_eligible() for these scenes -- the pipelined kernel
takes external actions and a static map, but only closest_first sorting, so the other two sort modes of class s run on the other
paths only.  MIN_AGENTS is the rule by which a class is skipped at a shape too small for it."""
import math

import numpy as np

from tests.orca_scenes import Scene

CLASSES = "tcgowms"
SORTS = ("first", "last", "tti")          # = CA_SORT_CLOSEST_FIRST, _CLOSEST_LAST, _TIME_TO_IMPACT
OVERS = ("all", "agent0", "learning")     # = CA_OVER_ALL_DONE, _AGENT0, _LEARNING_DONE
VARIANTS = {"t": ("",), "c": ("", "clip"), "g": ("",), "o": OVERS, "w": ("",), "m": ("",),
            "s": tuple("%s-%s" % (s, k) for s in SORTS for k in ("below", "equal", "above"))}
MIN_AGENTS = {c: 2 for c in CLASSES}      # every class has a two-agent form; a shape below its class's minimum is skipped

AT_GOAL, WAS_AT_GOAL, IN_COLLISION, WAS_IN_COLLISION, OUT_OF_TIME, DONE, IS_LEARNING, STILL_LEARNING = (1 << b for b in range(8))
ABSENT = 1 << 16
POL_EXTERNAL, POL_LEARNING = 3, 4         # oracle/ca_oracle.h
DT = 0.1
R_TIME, R_GOAL, R_COLL, R_WALL, R_WIGGLE = -0.01, 1.0, -0.25, -0.2, -0.05
WIGGLE = 0.15625
HORIZON = 40.0
MAP_ROWS, MAP_COLS, MAP_CELL = 32, 48, 0.125
PITCH = 8.0

LABELS = {
    "t": {1: "on: collide", 2: "inside: collide", 3: "outside: close-range reward"},
    "c": {1: "on: close-range reward", 2: "inside: close-range reward", 3: "outside: time-step reward",
          4: "minimum of two gaps"},
    "g": {1: "on: at goal", 2: "inside: at goal", 3: "outside: not at goal", 4: "at goal and touched", 5: "toucher: collides",
          6: "outside and touched: collides"},
    "o": {1: "on: out of time", 2: "below: out of time", 3: "above: not yet", 4: "out of time and collides",
          5: "collides, not out of time"},
    "w": {1: "on: no wiggle", 2: "above: wiggle", 3: "below: no wiggle", 4: "close range, wiggle", 5: "close range, no wiggle"},
    "m": {1: "wall hit", 2: "outside the map: no hit", 3: "R cells away: no hit", 4: "agent and wall: agent reward",
          5: "agent only"},
    "s": {1: "host", 2: "tied pair", 3: "half bucket", 4: "beside a half bucket", 5: "same bucket", 6: "horizon"},
}


def pipelined_eligible(cls, variant):
    """csrc/cagpu_launch.inc pipe_eligible(): no per-step RVO inputs and no ext_state (these scenes have none), an instantiated agent
    count (orca_scenes.PIPE_TILE), closest_first sorting; external actions and a static map do not matter to it"""
    return cls != "s" or variant.startswith("first")


def _solve(fn, target, lo, hi):
    """the float64 v in [lo, hi] (0 < lo) with fn(v) == target, fn non-decreasing: bisection over the bit patterns"""
    a, b = int(np.float64(lo).view(np.int64)), int(np.float64(hi).view(np.int64))
    assert fn(lo) < target <= fn(hi), (fn(lo), target, fn(hi))
    while b - a > 1:                      # fn(a) < target <= fn(b)
        m = (a + b) // 2
        if fn(float(np.int64(m).view(np.float64))) < target:
            a = m
        else:
            b = m
    v = float(np.int64(b).view(np.float64))
    assert fn(v) == target, (fn(v), target)
    return v


def _kind_value(T, kind, quantity_grows_outward=True):
    """kind 0 / 1 / 2 = on / inside / outside the threshold T"""
    if kind == 0:
        return T
    inward = -math.inf if quantity_grows_outward else math.inf
    return float(np.nextafter(T, inward if kind == 1 else -inward))


def _partner_at(xa, target, quantity):
    """(x, y) of a partner of the agent at (xa, 0) whose `quantity(d)` of the centre distance d, evaluated like util.py:17-21
    (sqrt(dx^2 + dy^2)), is exactly `target`: x on the grid of xa's neighbourhood, y a few hundredths, found by _solve"""
    d0 = _solve(quantity, target, 1e-3, 64.0)                       # the distance wanted, as a float64
    xb = xa + math.sqrt(d0 * d0 - 2.0 ** -12) * (1 - 2.0 ** -30)     # leaves y about 1 / 64
    u = xb - xa
    y = _solve(lambda v: quantity(math.sqrt(u * u + v * v)), target, 2.0 ** -10, 0.25)
    return xb, y


def _radius(i):
    return 0.25 + i / 512.0


def _units(N):
    """[(first agent, size)]: pairs, every third unit a triple while five or more agents are left, a last single"""
    out, i = [], 0
    while i < N:
        left = N - i
        size = 3 if (left == 3 or (left >= 5 and len(out) % 3 == 2)) else min(2, left)
        out.append((i, size))
        i += size
    return out


class _Env(object):
    """one env under construction: rows default to a lone, far-sighted, stationary ExternalPolicy agent"""

    def __init__(self, sc, e):
        self.sc, self.e = sc, e
        N = sc.N
        self.arm = 0

    def at(self, k):
        """unit k stands on arm k % 4 of a cross through the origin (the +x, +y, -x, -y axis), PITCH x (1 + k // 4) out: the
        classes lay a unit out along the +x axis and put() turns it by the arm's multiple of 90 degrees, which is exact.
        (A row of 43 units would reach 340 m, where a float32 observation is good to 1.5e-5 only; the cross stays below 100 m.)
        -> the unit's distance from the origin"""
        self.arm = k % 4
        return PITCH * (1 + k // 4)

    def _turn(self, p):
        x, y = p
        return ((x, y), (-y, x), (-x, -y), (y, -x))[self.arm]

    def put(self, i, pos, radius, goal=None, label=0, reward=math.nan, flags=None):
        sc, e = self.sc, self.e
        pos = self._turn(pos)
        sc.pos_x[e, i], sc.pos_y[e, i] = pos
        sc.goal_x[e, i], sc.goal_y[e, i] = (pos[0] + 32.0, pos[1]) if goal is None else self._turn(goal)
        sc.radius[e, i] = radius
        sc.label[e, i], sc.expect_reward[e, i] = label, reward
        sc.expect_care[e, i] = flags is not None
        sc.expect_flags[e, i] = 0 if flags is None else flags


def _new_scene(cls, N, E, variant):
    sc = Scene(cls, E, N)
    sc.variant = variant
    sc.policy = np.full((E, N), POL_EXTERNAL, np.int32)
    sc.ext = np.zeros((E, N, 2), np.float64)
    sc.time_remaining = np.full((E, N), 60.0)
    sc.label = np.zeros((E, N), np.int8)
    sc.expect_reward = np.full((E, N), math.nan)
    sc.expect_flags = np.zeros((E, N), np.uint32)
    sc.expect_care = np.zeros((E, N), bool)
    sc.static_map = None
    sc.max_obs = N - 1
    sc.params = dict(reward_time_step=R_TIME)
    return sc


# ---------------------------------------------------------------- t: touching
T_RADII = (None, (0.625, 0.625), (0.2, 0.3), (0.3, 0.2), (0.1, 0.7))


def _env_t(env, N, e):
    for k, (i, size) in enumerate(_units(N)):
        X, idx = env.at(k), k + e
        if size == 1:
            env.put(i, (X, 0.0), _radius(i))
            continue
        kind, rr = idx % 3, T_RADII[idx % 5]
        ra, rb = (_radius(i), _radius(i + 1)) if rr is None else rr
        cr = ra + rb
        if rr == (0.625, 0.625) and kind == 0:
            pb = (X + 0.75, 1.0)                                         # binary exact: 1.25 apart
        else:
            pb = _partner_at(X, _kind_value(cr, kind), lambda d: d)
        hit = kind != 2
        rew = R_COLL if hit else -0.1 - (math.hypot(pb[0] - X, pb[1]) - cr) / 2.0
        for j, pos, r in ((i, (X, 0.0), ra), (i + 1, pb, rb)):
            env.put(j, pos, r, label=kind + 1, reward=rew, flags=IN_COLLISION if hit else 0)
        if size == 3:
            env.put(i + 2, (X, 4.0), _radius(i + 2))


# ---------------------------------------------------------------- c: close range
def _env_c(env, N, e):
    gcr = env.sc.params["getting_close_range"]
    rmin = R_COLL
    for k, (i, size) in enumerate(_units(N)):
        X, idx = env.at(k), k + e
        if size == 1:
            env.put(i, (X, 0.0), _radius(i))
            continue
        kind = idx % 3
        ia, ib, ic = ((i, i + 1, i + 2), (i + 1, i + 2, i), (i + 2, i, i + 1))[idx % 3] if size == 3 else (i, i + 1, None)
        # fl(d - cr) == range needs d - cr == range in the reals (the subtraction is exact here), so the combined radius carries
        # the range's low bits: d binary exact, cr = d - range < 0.5, r_a binary exact, r_b = cr - r_a.  The difference moves on
        # d's grid, so the neighbouring kinds are d one ulp (of d) smaller and larger.
        d = 0.875 if gcr > 0.25 else 0.625
        cr = d - gcr
        ra = 0.1875 + ia / 2048.0
        rb = cr - ra
        assert cr < 0.5 and d - cr == gcr and ra + rb == cr
        pb = (X + d, 0.0) if kind == 0 else _partner_at(X, _kind_value(d, kind), lambda d: d)
        assert (math.sqrt((pb[0] - X) * (pb[0] - X) + pb[1] * pb[1]) - cr <= gcr) == (kind != 2)
        rew = max(rmin, -0.1 - gcr / 2.0) if kind != 2 else R_TIME
        env.put(ib, pb, rb, label=kind + 1, reward=rew, flags=0)
        if size == 3:          # a's other neighbour is 1/16 m away: a and c take the reward of THAT gap whatever b's kind is
            rc = 0.1875 + ic / 2048.0
            env.put(ic, (X - (ra + rc + 0.0625), 0.0), rc, label=4, reward=-0.1 - 0.0625 / 2.0, flags=0)
            env.put(ia, (X, 0.0), ra, label=4, reward=-0.1 - 0.0625 / 2.0, flags=0)
        else:
            env.put(ia, (X, 0.0), ra, label=kind + 1, reward=rew, flags=0)


# ---------------------------------------------------------------- g: goal and priorities
def _goal_for(X, kind, near_goal=0.2):
    T = _kind_value(near_goal * near_goal, kind)
    gx = 0.1875
    v = _solve(lambda v: gx * gx + v * v, T, 2.0 ** -6, 0.125)
    return (X - gx, -v)


def _env_g(env, N, e):
    for k, (i, size) in enumerate(_units(N)):
        X, idx = env.at(k), k + e
        kind, touch = idx % 3, (idx // 3) % 2 == 1 and size >= 2
        ra = _radius(i)
        at = kind != 2
        if touch:
            la, rew, fl = (4, R_GOAL, AT_GOAL) if at else (6, R_COLL, IN_COLLISION)
        else:
            la, rew, fl = kind + 1, (R_GOAL if at else R_TIME), (AT_GOAL if at else 0)
        env.put(i, (X, 0.0), ra, goal=_goal_for(X, kind), label=la, reward=rew, flags=fl)
        if size >= 2:
            if touch:
                env.put(i + 1, (X + 0.75, 1.0), 1.25 - ra, label=5, reward=R_COLL, flags=IN_COLLISION)
            else:
                env.put(i + 1, (X + 4.0, 0.0), _radius(i + 1), reward=R_TIME, flags=0)
        if size == 3:
            env.put(i + 2, (X, 4.0), _radius(i + 2), reward=R_TIME, flags=0)


# ---------------------------------------------------------------- o: time-out and game over
def _env_o(env, N, e):
    sc = env.sc
    times = (DT, float(np.nextafter(DT, 0.0)), float(np.nextafter(DT, math.inf)))
    for k, (i, size) in enumerate(_units(N)):
        X, idx = env.at(k), k + e
        touch = (idx // 3) % 2 == 1 and size >= 2
        for j in range(i, i + size):
            kind = (j + e) % 3
            out = kind != 2
            sc.time_remaining[env.e, j] = times[kind]
            pos = ((X, 0.0), (X + 0.75, 1.0) if touch else (X + 4.0, 0.0), (X, 4.0))[j - i]
            r = _radius(j)
            if touch and j == i + 1:
                r = 1.25 - _radius(i)
            hit = touch and j < i + 2
            env.put(j, pos, r, label=(4 if out else 5) if hit else kind + 1, reward=R_COLL if hit else R_TIME,
                    flags=(OUT_OF_TIME if out else 0) | (IN_COLLISION if hit else 0))
    if sc.variant == "learning" and env.e % 2 == 1:
        j = 1 % N
        sc.policy[env.e, j] = POL_LEARNING
        sc.flags[env.e, j] |= IS_LEARNING | STILL_LEARNING
        sc.ext[env.e, j] = (0.0, 0.5)       # LearningPolicy.py:29-33: speed 0, heading change max_heading_change x (2 x 0.5 - 1) = 0


# ---------------------------------------------------------------- w: wiggle
def wiggle_actions():
    t = np.float32(WIGGLE)
    up, dn = np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(0.0))
    return [(float(t), False), (float(up), True), (float(dn), False), (-float(t), False), (-float(up), True), (-float(dn), False)]


def _env_w(env, N, e):
    acts = wiggle_actions()
    for k, (i, size) in enumerate(_units(N)):
        X, idx = env.at(k), k + e
        close = idx % 4 == 3 and size >= 2
        for j in range(i, i + size):
            a, wig = acts[(j + e) % 6]
            env.sc.ext[env.e, j] = (0.0, a)
            near = close and j < i + 2
            pos = ((X, 0.0), (X + _radius(i) + _radius(i + 1) + 0.125, 0.0) if close else (X + 4.0, 0.0), (X, 4.0))[j - i]
            base = -0.1 - 0.125 / 2.0 if near else R_TIME
            env.put(j, pos, _radius(j), label=(4 if wig else 5) if near else ((j + e) % 3) + 1,
                    reward=base + (R_WIGGLE if wig else 0.0), flags=0)


# ---------------------------------------------------------------- m: walls
def wall_map():
    m = np.zeros((MAP_ROWS, MAP_COLS), bool)
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    m[16, 30] = m[24, 14] = True
    return m


def _cx(c):
    return (c - MAP_COLS / 2 + 0.5) * MAP_CELL


def _cy(r):
    return (MAP_ROWS / 2 - r - 0.5) * MAP_CELL


def wall_cases():
    """(x, y, radius, label, touching partner or None): see the module docstring, class m"""
    up, dn = math.inf, -math.inf
    return [
        (_cx(1), _cy(16), 0.25, 1, None), (_cx(46), _cy(8), 0.25, 1, None),        # the bounding box leaves the map: left, right,
        (_cx(12), _cy(1), 0.25, 1, None), (_cx(36), _cy(30), 0.25, 1, None),       # top, bottom
        (-3.0, _cy(24), 0.25, 1, None), (_cx(30), 2.0, 0.25, 1, None),             # cell index exactly 0 (24 - 24, 16 - 16)
        (_cx(6), -1.875, 0.25, 1, None), (2.875, _cy(22), 0.25, 1, None),          # exactly rows - 1, cols - 1
        (float(np.nextafter(-3.0, dn)), _cy(6), 0.25, 2, None),                    # one ulp outside: left,
        (_cx(20), float(np.nextafter(2.0, up)), 0.25, 2, None),                    # top,
        (_cx(20), -2.0, 0.25, 2, None),                                            # bottom (16 + 16 = rows exactly)
        (_cx(28), float(np.nextafter(-2.0, 0.0)), 0.25, 2, None),                  # ... one ulp inside it in the reals, but 16 +
        (_cx(41), -2.0 + 2.0 ** -51, 0.25, 1, None),                               # 15.999999999999998 rounds to 32: two ulps do it
        (_cx(26), _cy(16), 0.5, 3, None),                                          # R = 4, the wall cell (16, 30) 4 cells away
        (_cx(11), _cy(24), 0.5, 1, None),                                          # R = 4, the wall cell (24, 14) 3 cells away
        (_cx(46), _cy(14), 0.25, 4, (-0.375, -0.5, 0.375)),                        # wall and agent: 0.625 apart, radii 0.25 + 0.375
    ]


def _env_m(env, N, e):
    cases = wall_cases()
    placed, i = [], 0
    for n in range(len(cases)):
        x, y, r, label, partner = cases[(5 * e + n) % len(cases)]
        need = 2 if partner else 1
        new = [(x, y, r)] + ([(x + partner[0], y + partner[1], partner[2])] if partner else [])
        if i + need > N or any(math.hypot(a[0] - b[0], a[1] - b[1]) - a[2] - b[2] < 0.5 for a in new for b in placed):
            continue
        if r == 0.25 and not partner:
            r = r + (i + 1) * 2.0 ** -12        # (distinct radii; not for the exact-R and the exact-distance cases)
        rew = {1: R_WALL, 2: R_TIME, 3: R_TIME, 4: R_COLL}[label]
        env.put(i, (x, y), r, label=label, reward=rew, flags=0 if label in (2, 3) else IN_COLLISION)
        if partner:
            env.put(i + 1, (new[1][0], new[1][1]), partner[2], label=5, reward=R_COLL, flags=IN_COLLISION)
        placed += new
        i += need
    for j in range(i, N):                   # the others stand outside the map, along the x axis
        env.put(j, (16.0 + 4.0 * (j % 16), 4.0 * (j // 16)), _radius(j), reward=R_TIME, flags=0)


# ---------------------------------------------------------------- s: sensor order
def _sensor_roles(N):
    """role -> agent index for one env of N agents"""
    roles = ["host", "A1", "A2", "X", "Y", "X2", "Y2", "Z", "B1", "B2"] + ["C%d" % k for k in range(8)] + ["F0", "F1", "F2"]
    roles = roles[:N] + ["far%d" % k for k in range(max(0, N - len(roles)))]
    want = {"host": 1 % N}
    if N > 64:
        want.update(A1=63, A2=64)
    if N >= 10:
        want.update(B1=0)
        if N - 1 not in want.values():      # (N = 65: index 64 is A2 already)
            want.update(B2=N - 1)
    free = [i for i in range(N) if i not in want.values()]
    return {r: want[r] if r in want else free.pop(0) for r in roles}


def _env_s(env, N, e):
    rh = 0.25
    tiny = lambda i: 0.3125 + i * 2.0 ** -20         # the circle of radius 5: gaps 4.4375 - i / 2^20, every one in bucket 444
    swap = e % 2 == 1                                # odd envs: the members of a tied pair change sides
    circle = [(5.0, 0.0), (-5.0, 0.0), (0.0, 5.0), (0.0, -5.0), (4.0, 3.0), (-4.0, 3.0), (4.0, -3.0), (-4.0, -3.0)]
    for role, i in sorted(_sensor_roles(N).items(), key=lambda kv: kv[1]):
        r = _radius(i)
        if role == "host":
            env.put(i, (0.0, 0.0), rh, label=1)
        elif role in ("A1", "A2", "B1", "B2"):
            x = 3.0 if (role[1] == "1") != swap else -3.0
            env.put(i, (x, 4.0 if role[0] == "A" else -4.0), tiny(i), label=2)
        elif role == "X":        # gap 1/8: 12.5 -> 12
            env.put(i, (0.0, rh + r + 0.125), r, label=3)
        elif role == "Y":        # bucket 13, p_orth 0 < X's: a round-half-up puts it in front of X
            env.put(i, (-((rh + r) + 0.1275), 0.0), r, label=4)
        elif role == "X2":       # gap 3/8: 37.5 -> 38
            env.put(i, (0.0, -(rh + r + 0.375)), r, label=3)
        elif role == "Y2":       # bucket 37, p_orth 0 > X2's: a round-half-down puts X2 in front of it
            env.put(i, ((rh + r) + 0.3725, 0.0), r, label=4)
        elif role == "Z":        # 100 x 1.115 rounds across the half
            env.put(i, (-((rh + r) + 1.115), 0.0), r, label=4)
        elif role[0] == "C":
            env.put(i, circle[int(role[1:])], tiny(i), label=5)
        elif role == "F0":
            env.put(i, (HORIZON, 0.0), r, label=6)
        elif role == "F1":
            env.put(i, (-float(np.nextafter(HORIZON, math.inf)), 0.0), r, label=6)
        elif role == "F2":
            env.put(i, (0.0, float(np.nextafter(HORIZON, 0.0))), r, label=6)
        else:
            k = int(role[3:])
            env.put(i, (HORIZON + 8.0 + 4.0 * (k % 16), 4.0 * (k // 16) - 8.0), r)
    if e % 3 == 2 and N >= 3:                        # ragged: the trailing slots as a reset leaves them empty
        sc = env.sc
        for n in Scene.FIELDS:
            getattr(sc, n)[e, N - N // 3:] = 1.0 if n == "pref_speed" else 0.0
        sc.flags[e, N - N // 3:] = ABSENT | DONE | AT_GOAL | WAS_AT_GOAL
        sc.time_remaining[e, N - N // 3:] = 0.0
        sc.label[e, N - N // 3:] = 0


def sensor_order(px, py, radius, present, host, sort, clip, horizon=math.inf, goal=None):
    """OtherAgentsStatesSensor.py:20-55 and :78-103 for agents that stand still, in plain float64 with Python's sorted and the
    reference's own keys -> the agent indices of the host's slots.  (Velocities zero: compute_time_to_impact, util.py:23-83,
    returns 0 for overlapping discs -- :31-34 -- and inf otherwise, v_rel being zero.)"""
    crit = []
    ox, oy = 0.0, 1.0                     # ref_orth of a goal on y = const ahead; else agent.py:329-349 from goal = (gx, gy)
    if goal is not None:
        dx, dy = goal[0] - px[host], goal[1] - py[host]
        dist = math.sqrt(dx ** 2 + dy ** 2)
        ox, oy = (-dy / dist, dx / dist) if dist > 1e-8 else (-dy, dx)
    for j in range(len(px)):
        if j == host or not present[j]:
            continue
        rx, ry = px[j] - px[host], py[j] - py[host]
        d = math.sqrt(rx * rx + ry * ry)
        if d > horizon:
            continue
        gap = d - radius[host] - radius[j]
        comb = radius[host] + radius[j]
        tti = 0.0 if (rx * rx + ry * ry - comb * comb) < 0 else math.inf
        crit.append([j, float(np.round(np.float64(gap), 2)), rx * ox + ry * oy, tti])
    if sort == "tti":
        key = lambda x: (-x[3], -x[1], x[2])
        return [x[0] for x in sorted(sorted(crit, key=key)[:clip], key=key)]
    kept = sorted(crit, key=lambda x: (x[1], x[2]))[:clip]
    if sort == "last":
        kept = sorted(kept, key=lambda x: (-x[1], x[2]))
    return [x[0] for x in kept]


def tie_key(sc, e, h, j):
    """(bucket, p_orth) of candidate j for host h of env e, the host's goal being on y = const ahead"""
    rx, ry = sc.pos_x[e, j] - sc.pos_x[e, h], sc.pos_y[e, j] - sc.pos_y[e, h]
    gap = math.sqrt(rx * rx + ry * ry) - sc.radius[e, h] - sc.radius[e, j]
    return (float(np.round(np.float64(gap), 2)), ry)


def _cut(sc, sort):
    """the smallest max_obs that cuts a group of env 0's host list tied in bucket and p_orth (N = 2: nobody to tie with)"""
    e, N = 0, sc.N
    h = 1 % N
    present = (sc.flags[e] & ABSENT) == 0
    full = sensor_order(sc.pos_x[e], sc.pos_y[e], sc.radius[e], present, h, sort, N, HORIZON)
    for K in range(1, len(full)):
        if tie_key(sc, e, h, full[K - 1]) == tie_key(sc, e, h, full[K]):
            return K
    assert N == 2
    return 1


# ---------------------------------------------------------------- build / inject
def build(cls, N, E, variant=""):
    assert cls in CLASSES and variant in VARIANTS[cls] and N >= MIN_AGENTS[cls], (cls, variant, N)
    sc = _new_scene(cls, N, E, variant)
    p = sc.params
    if cls == "c":
        p["getting_close_range"] = 0.45 if variant == "clip" else 0.2
    if cls == "o":
        p["game_over_mode"] = OVERS.index(variant)
    if cls == "w":
        p.update(reward_wiggly=R_WIGGLE, wiggly_threshold=WIGGLE)
    if cls == "m":
        p["reward_collision_wall"] = R_WALL
        sc.static_map = wall_map()
    fn = globals()["_env_" + cls]
    for e in range(E):
        fn(_Env(sc, e), N, e)
    if cls == "s":
        sort, kmode = variant.split("-")
        p.update(sort_mode=SORTS.index(sort), sensing_horizon=HORIZON, ragged=1)
        sc.max_obs = {"below": _cut(sc, "tti" if sort == "tti" else "first"), "equal": N - 1, "above": N + 1}[kmode]
    return sc


def oracle_params(orc, sc):
    """OrcParams for a scene"""
    p = orc.default_params(sc.E, sc.N, max_obs=sc.max_obs, dt=DT, ragged=sc.params.get("ragged", 0))
    for k, v in sc.params.items():
        if k != "ragged":
            setattr(p, k, v)
    return p


def sim_kwargs(sc):
    """keyword arguments of core.make_params for a scene"""
    return dict(sc.params, max_obs=sc.max_obs, dt=DT)


def ext_actions(sc):
    """the external actions of every step, float64 [E, N, 2], or None where they are all zero in effect (an ExternalPolicy
    or LearningPolicy agent without an action stands still: the scenes of every class but w)"""
    return sc.ext if sc.cls == "w" else None


def inject(o, sc):
    """oracle state := scene (call o.set_map(sc.static_map, MAP_ROWS, MAP_COLS, MAP_CELL) for class m as well)"""
    for n in Scene.FIELDS:
        o.s[n][:] = getattr(sc, n).reshape(-1)
    o.s["time_remaining"][:] = sc.time_remaining.reshape(-1)
    o.s["slt"][:] = 7.5
    for n in ("t", "ep_reward", "turning_dir"):
        o.s[n][:] = 0.0
    o.s["last_action"][:] = 0.0
    o.s["flags"][:] = sc.flags.reshape(-1)
    o.s["slt"][(sc.flags.reshape(-1) & ABSENT) != 0] = 0.0
    o.s["policy"][:] = sc.policy.reshape(-1)
    o.s["dynamics"][:] = 0
    for n in ("step_num", "episode_step", "reset_count"):
        o.s[n][:] = 0
    o.s["env_stats"][:] = 0.0


def check_principle(sc, before, after):
    """what the host test asserts of the oracle's states around a step: nobody moved, every heading was 0, every goal of a
    present agent lies on y = const through it unless the class is about the goal itself"""
    live = (sc.flags.reshape(-1) & ABSENT) == 0
    assert np.array_equal(before["pos_x"], after["pos_x"]) and np.array_equal(before["pos_y"], after["pos_y"]), "an agent moved"
    assert not before["heading"].any(), "a heading is not 0"
    assert not after["vel_x"].any() and not after["vel_y"].any(), "a velocity is not 0"
    if sc.cls != "g":
        assert np.array_equal(sc.goal_y.reshape(-1)[live], sc.pos_y.reshape(-1)[live]), "a goal off the agent's y"
        assert (sc.goal_x.reshape(-1)[live] > sc.pos_x.reshape(-1)[live] + 31.0).all()
