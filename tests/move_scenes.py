"""Deterministic scenes (numpy only) that put the MOVE of a step on its angle edges, for tests/test_move_scenes_host.py and
tests/test_gpu_move_edges.py: policy output -> float32 action -> unicycle move -> ego frame -> the float columns of the
observation.  build(cls, N, E, variant) -> Scene; oracle_params(orc, scene); inject(o, scene) writes one into an oracle.Oracle,
from where the GPU tests upload it; oracle_step(orc, o, ext) steps it.  In the style of tests/step_rule_scenes.py.

LAYOUT.  Agent i of an env stands at (4 (1 + i % 8), 4 (i // 8)) m -- binary exact, float32 exact, 4 m from its neighbours, so
that with radii 0.25 + (i % 64) / 512 and at most 0.1 m of travel per step nobody collides or comes into close range -- and has
its goal 16 m away unless the case says otherwise, so that nobody arrives either: nothing ends an episode in the first step
except where a case is about arriving (static agents, the agents 1e-8 m from their goal).  Every operand is finite.

CASES.  Every class is a list of cases; agent i of env e of an N-agent scene takes case (first(N) + e N + i) % len(cases), where
first(N) = 4 (2 + ... + (N - 1)): an env is a function of (class, variant, N, env) alone, a scene with fewer envs is a prefix of
one with more, the recorded scenes (N = 2 .. 6, 4 envs: 80 agents) take the cases 0 .. 79 once each, and every shape of the GPU
tests (at least 90 agents) takes all of them.  No class has more than 80 cases (asserted).

WHAT A SCENE FIXES.  The action is float32, so a case names a float32-representable a1 first and derives the heading from it:
_heading_for(turn, target) finds the float64 heading with fl(turn + heading) == target BY BITS and asserts it (turn: a1, or
fl(fl(clip(a1 / dt)) dt) under UnicycleDynamicsMaxTurnRate).  Scene.expect_heading / expect_td [E, N] (NaN: not fixed),
expect_action [E, N, 2] (float32, NaN: not fixed), expect_dist and expect_flags (the at-goal bit) are the first step's values that follow from
the case without any libm call; Scene.label [E, N] names the branch an agent is there for (LABELS).

Classes (VARIANTS lists their variants):
  h  wrap of the new heading, ExternalPolicy, variants "unicycle" / "maxturn" (the two unicycle dynamics): a1 + heading exactly pi,
     one ulp below, one ulp above; exactly -pi, one ulp below, one ulp above; +0 and -0; more than one turn out (a1 = +-7, +-20 --
     under "maxturn" these are clamped, and headings of +-7.5 and +-19.5 take their place -- and sums exactly fl(+-3 pi)): the
     general loop of wrap_pi.  The expected heading is target -+ n 2 pi in n sequential float64 steps, n the one count that
     lands in [-pi, pi) (util.py:141-146 says that interval); for the six edges n is stated by hand as well.
  d  turning_dir (UnicycleDynamics.py:41-47): injected turning_dir 0, +-1e-5, +-(one ulp inside 1e-5), +-0.1, one ulp either side
     of +-0.1, +-0.05, +-2, +-3 against new headings +0, -0, +-(smallest normal), +-0.75, +-2, -+1: each of the three branches, the
     clamp of -td + nh at +-pi, and agents with UnicycleDynamicsMaxTurnRate, whose turning_dir must stay.
  m  max turn rate (UnicycleDynamicsMaxTurnRate.py:31-33): variant "pow2": dt = 0.125, a1 = +-0.375 (a1 / dt exactly +-3) and
     the float32 either side; variant "default": dt = 0.1 and the three float32 around +-0.3.
  a  action decoding: variant "external" raw values; "learning" e1 in {0, 0.5, 1, 0.25}, e0 in {0, 1, 0.5}; "ga3c" e0 = -1,
     0 .. 10, 11, 10.9, 2.5 for LearningPolicyGA3C and GA3CCADRLPolicy agents (all eleven actions, the clamp, truncation).
  n  non-cooperative and static: NonCooperativePolicy agents facing exactly away from the goal (heading 0, goal along -x:
     heading_ego = -pi, dh = +pi, float32(pi) > pi wraps; once with dy = +0, once with dy = -0 = (-0) - (+0), where atan2 is
     -pi), exactly at it, with the goal along +-y, and off axis; StaticPolicy agents (the goal moves onto them: dist = 0, the
     `<= 1e-8` branch, every ego-frame column zero); ExternalPolicy agents that stand still at (0, 4 i) with the goal at distance
     exactly 1e-8, one ulp below and one above along +x (sqrt(dx dx) == dx asserted): p_parallel of the others is rx dx in the
     first two and rx in the third.
  r  RVO action (RVOPolicy.py:96-111), sensing_horizon = 2 m so that nobody has an ORCA neighbour and rvo2 returns the
     preferred velocity: goal along +x (ang == 0) with headings 0, 0.25, +-0.5 (inside pi/6), exactly pi / 6 (not clipped) and
     one ulp above (clipped, speed 0), +-1 (clipped); goal along -x with dy = +0 and (-0) - (+0); goal below the x axis
     (ang < 0: + 2 pi); an agent so slow (pref_speed 2^-40) that its float32 position does not change: zero displacement.
     NOT built, because no finite operands give them: an agent standing ON its goal (RVOPolicy.py:67 divides by the distance:
     NaN), and dpy = -0 (dpy = float32 position - float64 position of equal values: x - x = +0 whatever the signs).

pipelined_eligible() restates cagpu_launch.inc pipe_eligible() for these scenes: every class runs on every path."""
import ctypes as C
import math

import numpy as np

from tests.orca_scenes import Scene

CLASSES = "hdmanr"
VARIANTS = {"h": ("unicycle", "maxturn"), "d": ("",), "m": ("pow2", "default"), "a": ("external", "learning", "ga3c"),
            "n": ("",), "r": ("",)}
MIN_AGENTS = {c: 2 for c in CLASSES}
MAX_CASES = 80

AT_GOAL, WAS_AT_GOAL, IN_COLLISION, WAS_IN_COLLISION, OUT_OF_TIME, DONE, IS_LEARNING, STILL_LEARNING = (1 << b for b in range(8))
POL_RVO, POL_NONCOOP, POL_STATIC, POL_EXTERNAL, POL_LEARNING, POL_LEARNING_GA3C, POL_GA3C_CADRL = range(7)   # oracle/ca_oracle.h
DYN_UNICYCLE, DYN_MAX_TURN_RATE = 0, 1
PI, TWO_PI = math.pi, 2.0 * math.pi
MIN_NORMAL = float(np.finfo(np.float64).tiny)
MAX_TURN = 3.0                            # UnicycleDynamicsMaxTurnRate.py:8
MAX_HEADING_CHANGE = math.pi / 3          # config.py (LearningPolicy)
RVO_HORIZON = 2.0

LABELS = {
    "h": {1: "pi: wraps", 2: "below pi: stays", 3: "above pi: wraps", 4: "-pi: stays", 5: "below -pi: wraps", 6: "above -pi: stays",
          7: "+0", 8: "-0", 9: "general loop", 10: "clamped turn"},
    "d": {1: "|td| < 1e-5: 0.11 sign(nh)", 2: "td nh < 0: -td + nh", 3: "clamped at +-pi", 4: "decays by 0.1", 5: "decays to 0",
          6: "max turn rate: unchanged"},
    "m": {1: "on the clamp", 2: "inside", 3: "outside: clamped"},
    "a": {1: "external", 2: "learning", 3: "index in range", 4: "index clamped", 5: "index truncated"},
    "n": {1: "away: wraps", 2: "at the goal", 3: "goal on an axis", 4: "off axis", 5: "static: dist 0", 6: "dist = 1e-8: not normalised",
          7: "dist below 1e-8: not normalised", 8: "dist above 1e-8: normalised"},
    "r": {1: "ang == 0", 2: "ang = pi", 3: "ang < 0", 4: "clipped: speed 0", 5: "inside pi / 6", 6: "on pi / 6: not clipped",
          7: "zero displacement"},
}


def up(x):
    return float(np.nextafter(np.float64(x), np.inf))


def dn(x):
    return float(np.nextafter(np.float64(x), -np.inf))


def up32(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def dn32(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def bits(x):
    return int(np.float64(x).view(np.int64))


def pipelined_eligible(cls, variant):
    """csrc/cagpu_launch.inc pipe_eligible(): no per-step RVO inputs and no ext_state (these scenes have none), an instantiated agent
    count (orca_scenes.PIPE_TILE), closest_first sorting (every scene here); external actions, the dynamics and the policies
    do not matter to it"""
    return True


def turn_of(a1, dyn, dt):
    """the heading change the dynamics add for the float32 action a1 (UnicycleDynamics.py:28, UnicycleDynamicsMaxTurnRate.py:31-32)"""
    if dyn == DYN_MAX_TURN_RATE:
        return min(max(a1 / dt, -MAX_TURN), MAX_TURN) * dt
    return a1


def _heading_for(turn, target):
    """the float64 heading with fl(turn + heading) == target by bits (asserted)"""
    h0 = target - turn
    cands, lo, hi = [h0], h0, h0
    for _ in range(8):
        lo, hi = dn(lo), up(hi)
        cands += [lo, hi]
    if target == 0.0 and bits(target) != 0:       # -0 is the sum of two -0 only
        cands = [-0.0]
    for h in cands:
        if bits(turn + h) == bits(target):
            return h
    raise AssertionError("no heading gives %r + h == %r" % (turn, target))


def wrapped(target):
    """-> (the representative of `target` in [-pi, pi) reached by n sequential float64 steps of 2 pi, n signed)"""
    for n in range(0, 8):
        for sgn in (-1, 1):
            x = target
            for _ in range(n):
                x = x + sgn * TWO_PI
            if -PI <= x < PI:
                return x, sgn * n
    raise AssertionError(target)


# ---------------------------------------------------------------- the cases: dicts of what differs from the default agent
def _cases_h(variant):
    dyn = DYN_MAX_TURN_RATE if variant == "maxturn" else DYN_UNICYCLE
    a1s = (0.25, -0.25, 0.125, -0.28125)
    out = []
    edges = [(PI, 1, -1), (dn(PI), 2, 0), (up(PI), 3, -1), (-PI, 4, 0), (dn(-PI), 5, 1), (up(-PI), 6, 0)]
    for k, (target, label, n) in enumerate(edges + edges):
        out.append(dict(a1=a1s[(k + k // 6) % 4], target=target, label=label, n=n))
    out.append(dict(a1=0.25, target=0.0, label=7, n=0))
    out.append(dict(a1=-0.25, target=0.0, label=7, n=0))
    out.append(dict(a1=-0.0, target=-0.0, label=8, n=0))
    for a1 in (7.0, -7.0, 20.0, -20.0):
        if dyn == DYN_UNICYCLE:
            out.append(dict(a1=a1, heading=math.copysign(0.5, a1), label=9))
        else:       # the turn is clamped to +-0.3: the heading itself is what is far out
            out.append(dict(a1=a1, heading=math.copysign(0.5, a1), label=10))
            out.append(dict(a1=math.copysign(0.25, a1), heading=a1 + math.copysign(0.5, a1), label=9))
    for a1, target in ((7.0, 3.0 * PI), (-7.0, -3.0 * PI), (0.25, 3.0 * PI), (-0.25, -3.0 * PI)):
        out.append(dict(a1=a1, target=target, label=9))
    for k, c in enumerate(out):
        c.update(dyn=dyn, e0=(0.5, 1.0, 0.75)[k % 3])
    return out


TD_SMALL = (0.0, dn(1e-5), -dn(1e-5))
TD_OTHER = (1e-5, -1e-5, 0.1, -0.1, up(0.1), -up(0.1), dn(0.1), -dn(0.1), 0.05, -0.05, 2.0, -2.0)
NH_HOW = [(0.75, 0.25, 0.5), (-0.75, -0.25, -0.5), (0.0, 0.25, -0.25), (-0.0, -0.0, -0.0), (MIN_NORMAL, 0.0, MIN_NORMAL),
          (-MIN_NORMAL, 0.0, -MIN_NORMAL), (2.0, 0.5, 1.5), (-2.0, -0.5, -1.5), (1.0, 0.25, 0.75), (-1.0, -0.25, -0.75)]


def _nh_how(nh):
    """(a1, heading) whose float64 sum is the new heading nh by bits (0.0 and -0.0 are one dict key: a list)"""
    return [(a1, h) for v, a1, h in NH_HOW if bits(v) == bits(nh)][0]


def _cases_d(variant):
    pairs = [(td, nh) for td in TD_SMALL + TD_OTHER for nh in (0.75, -0.75)]
    pairs += [(td, nh) for td in (0.0, 1e-5, -1e-5, dn(1e-5), 0.05, -0.05, 2.0, -2.0) for nh in (0.0, -0.0, MIN_NORMAL, -MIN_NORMAL)]
    pairs += [(-2.0, 2.0), (2.0, -2.0), (-3.0, 1.0), (3.0, -1.0), (-2.0, -2.0), (2.0, 2.0)]
    out = []
    for td, nh in pairs:
        a1, heading = _nh_how(nh)
        assert bits(a1 + heading) == bits(nh), (a1, heading, nh)
        if abs(td) in (0.0, dn(1e-5)):                                    # strictly inside 1e-5
            label, want = 1, 0.11 * ((nh > 0) - (nh < 0))
        elif nh != 0.0 and (td > 0) != (nh > 0):                          # opposite signs (a zero heading has none)
            s = -td + nh
            label, want = (3, math.copysign(PI, s)) if abs(s) > PI else (2, s)
        else:
            rest = abs(td) - 0.1
            label, want = (4, math.copysign(rest, td)) if rest > 0.0 else (5, math.copysign(0.0, td))
        out.append(dict(a1=a1, heading=heading, td=td, label=label, want_td=want, want_heading=nh, dyn=DYN_UNICYCLE, e0=0.5))
    for td in (0.0, 0.05, 2.0, -1e-5):
        out.append(dict(a1=0.25, heading=0.5, td=td, label=6, want_td=td, want_heading=0.75, dyn=DYN_MAX_TURN_RATE, e0=0.5))
    return out


def _cases_m(variant):
    out = []
    for h0 in (0.0, 0.5):          # (a heading of 0 keeps the turn's last bit in the sum: the next double of the clamp shows there)
        for s in (1.0, -1.0):
            if variant == "pow2":
                for a1, label in ((0.375, 1), (dn32(0.375), 2), (up32(0.375), 3)):
                    out.append(dict(a1=s * a1, heading=s * h0, label=label, want_heading=s * (min(a1, 0.375) + h0)))
            else:
                t = float(np.float32(0.3))          # 0.300000011920929 > 0.3: a1 / 0.1 > 3
                for a1, label in ((t, 3), (dn32(t), 2), (up32(t), 3)):
                    out.append(dict(a1=s * a1, heading=s * h0, label=label,
                                    want_heading=s * ((3.0 * 0.1 if label == 3 else (a1 / 0.1) * 0.1) + h0)))
    for k, c in enumerate(out):
        c.update(dyn=DYN_MAX_TURN_RATE, e0=(0.5, 1.0)[k % 2], td=0.05, want_td=0.05)
    return out


GA3C_TABLE = [(1.0, -PI / 6), (1.0, -PI / 12), (1.0, 0.0), (1.0, PI / 12), (1.0, PI / 6), (0.5, -PI / 6), (0.5, 0.0), (0.5, PI / 6),
              (0.0, -PI / 6), (0.0, 0.0), (0.0, PI / 6)]      # network.py:7-16, row by row


def _cases_a(variant):
    out = []
    if variant == "external":
        for e0, e1 in ((0.5, 0.25), (1.0, -0.1), (0.3, 0.7), (0.0, 0.0), (1e-3, PI / 6), (0.7, -PI / 3), (1.2, 1e-9), (0.1, -1e-3)):
            out.append(dict(pol=POL_EXTERNAL, e0=e0, a1=e1, label=1, want_action=(e0, e1)))
    elif variant == "learning":
        for e1, dh in ((0.0, -MAX_HEADING_CHANGE), (0.5, 0.0), (1.0, MAX_HEADING_CHANGE), (0.25, -MAX_HEADING_CHANGE / 2)):
            for e0 in (0.0, 1.0, 0.5):
                out.append(dict(pol=POL_LEARNING, e0=e0, a1=e1, label=2, want_action=(None, dh), speed_factor=e0))
    else:
        for pol in (POL_LEARNING_GA3C, POL_GA3C_CADRL):
            for e0, q, label in [(-1.0, 0, 4)] + [(float(q), q, 3) for q in range(11)] + [(11.0, 10, 4), (10.9, 10, 5), (2.5, 2, 5)]:
                out.append(dict(pol=pol, e0=e0, a1=0.0, label=label, want_action=(None, GA3C_TABLE[q][1]),
                                speed_factor=GA3C_TABLE[q][0]))
    for k, c in enumerate(out):
        c.update(heading=(0.5, -0.5, 0.0)[k % 3], dyn=(DYN_UNICYCLE, DYN_MAX_TURN_RATE)[(k // 3) % 2])
    return out


def _cases_n(variant):
    f32pi = float(np.float32(PI))
    away = dict(pol=POL_NONCOOP, heading=0.0, label=1, want_action=(None, f32pi), want_heading=f32pi - TWO_PI)
    out = [dict(away, goal=(-8.0, 0.0)), dict(away, goal=(-8.0, 0.0), minus_zero_dy=True),
           dict(pol=POL_NONCOOP, heading=0.0, goal=(8.0, 0.0), label=2, want_action=(None, -0.0), want_heading=0.0),
           dict(pol=POL_NONCOOP, heading=0.0, goal=(0.0, 8.0), label=3), dict(pol=POL_NONCOOP, heading=0.0, goal=(0.0, -8.0), label=3),
           dict(pol=POL_NONCOOP, heading=0.25, goal=(8.0, 0.0), label=3), dict(pol=POL_NONCOOP, heading=-3.0, goal=(-8.0, 0.0), label=3),
           dict(pol=POL_NONCOOP, heading=0.3, goal=(5.0, -7.0), label=4), dict(pol=POL_NONCOOP, heading=-2.5, goal=(-6.0, 3.0), label=4),
           dict(pol=POL_STATIC, heading=0.0, label=5, want_heading=0.0), dict(pol=POL_STATIC, heading=0.75, label=5, want_heading=0.75)]
    for d, label in ((1e-8, 6), (dn(1e-8), 7), (up(1e-8), 8)):
        assert math.sqrt(d * d + 0.0 * 0.0) == d, d
        out.append(dict(pol=POL_EXTERNAL, heading=0.0, goal=(d, 0.0), label=label, at_origin=True, want_heading=0.0, want_dist=d))
    for c in out:
        c.update(dyn=DYN_UNICYCLE, e0=0.0, a1=0.0)
    # the agents that arrive in the first step (labels 5 .. 8) never stand next to each other in the list, so that every env keeps
    # an agent that does not: no episode ends
    arrive, rest = [c for c in out if c["label"] >= 5], [c for c in out if c["label"] < 5]
    out = []
    while arrive or rest:
        out += [arrive.pop(0)] if arrive else []
        out += [rest.pop(0)] if rest else []
    return out


def _cases_r(variant):
    out = [dict(heading=0.0, goal=(8.0, 0.0), label=1, want_action=(None, 0.0), want_heading=0.0),
           dict(heading=0.25, goal=(8.0, 0.0), label=1, want_action=(None, -0.25), want_heading=0.0),
           dict(heading=0.5, goal=(8.0, 0.0), label=5, want_action=(None, -0.5)), dict(heading=-0.5, goal=(8.0, 0.0), label=5, want_action=(None, 0.5)),
           dict(heading=PI / 6, goal=(8.0, 0.0), label=6, want_action=(None, -(PI / 6))),
           dict(heading=-(PI / 6), goal=(8.0, 0.0), label=6, want_action=(None, PI / 6)),
           dict(heading=up(PI / 6), goal=(8.0, 0.0), label=4, want_action=(0.0, -(PI / 6))),
           dict(heading=-up(PI / 6), goal=(8.0, 0.0), label=4, want_action=(0.0, PI / 6)),
           dict(heading=1.0, goal=(8.0, 0.0), label=4, want_action=(0.0, -(PI / 6))), dict(heading=-1.0, goal=(8.0, 0.0), label=4, want_action=(0.0, PI / 6)),
           dict(heading=3.0, goal=(-8.0, 0.0), label=2), dict(heading=-3.0, goal=(-8.0, 0.0), label=2),
           dict(heading=3.0, goal=(-8.0, 0.0), label=2, minus_zero_dy=True),
           dict(heading=-0.75, goal=(3.0, -4.0), label=3), dict(heading=-2.5, goal=(-3.0, -4.0), label=3),
           dict(heading=0.25, goal=(8.0, 0.0), pref_speed=2.0 ** -40, label=7, want_action=(0.0, -0.25), want_heading=0.0)]
    for c in out:
        c.update(pol=POL_RVO, dyn=DYN_UNICYCLE, e0=0.0, a1=0.0)
    return out


def cases(cls, variant):
    out = globals()["_cases_" + cls](variant)
    assert 0 < len(out) <= MAX_CASES, (cls, variant, len(out))
    return out


def first_case(N):
    return 4 * (N * (N - 1) // 2 - 1)


def dt_of(cls, variant):
    return 0.125 if (cls, variant) == ("m", "pow2") else 0.1


# ---------------------------------------------------------------- build / inject
def build(cls, N, E, variant=""):
    assert cls in CLASSES and variant in VARIANTS[cls] and N >= MIN_AGENTS[cls], (cls, variant, N)
    sc = Scene(cls, E, N)
    sc.variant, sc.dt = variant, dt_of(cls, variant)
    sc.policy = np.full((E, N), POL_EXTERNAL, np.int32)
    sc.dynamics = np.zeros((E, N), np.int32)
    sc.turning_dir = np.zeros((E, N), np.float64)
    sc.ext = np.zeros((E, N, 2), np.float64)
    sc.label = np.zeros((E, N), np.int8)
    sc.case = np.zeros((E, N), np.int32)
    sc.expect_heading = np.full((E, N), math.nan)
    sc.expect_td = np.full((E, N), math.nan)
    sc.expect_dist = np.full((E, N), math.nan)
    sc.expect_action = np.full((E, N, 2), math.nan, np.float32)
    sc.expect_flags = np.zeros((E, N), np.uint32)
    sc.max_obs = N - 1
    sc.params = dict(sensing_horizon=RVO_HORIZON) if cls == "r" else {}
    cs = cases(cls, variant)
    for e in range(E):
        for i in range(N):
            k = (first_case(N) + e * N + i) % len(cs)
            c = cs[k]
            pos = (0.0, 4.0 * i) if c.get("at_origin") else (4.0 * (1 + i % 8), 4.0 * (i // 8))
            dyn, a1 = c["dyn"], c["a1"]
            if "target" in c:          # class h: the heading follows from the float32 a1 and the sum aimed at
                assert float(np.float32(a1)) == a1
                heading = _heading_for(turn_of(a1, dyn, sc.dt), c["target"])
                want, n = wrapped(c["target"])
                assert "n" not in c or c["n"] == n, (c, n)
                sc.expect_heading[e, i] = want
            else:
                heading = c["heading"]
                if cls == "h":
                    sc.expect_heading[e, i] = wrapped(turn_of(float(np.float32(a1)), dyn, sc.dt) + heading)[0]
            gx, gy = c.get("goal", (16.0, 8.0))
            sc.pos_x[e, i], sc.pos_y[e, i] = pos
            sc.goal_x[e, i], sc.goal_y[e, i] = pos[0] + gx, pos[1] + gy
            if c.get("minus_zero_dy"):      # dy = (-0) - (+0) = -0: only an agent of the row y = 0 can have it
                if pos[1] == 0.0:
                    sc.goal_y[e, i] = -0.0
            sc.heading[e, i] = heading
            sc.radius[e, i] = 0.25 + (i % 64) / 512.0
            sc.pref_speed[e, i] = c.get("pref_speed", 1.0 + (i % 4) / 8.0)
            sc.policy[e, i], sc.dynamics[e, i] = c.get("pol", POL_EXTERNAL), dyn
            sc.turning_dir[e, i] = c.get("td", 0.0)
            sc.ext[e, i] = (c["e0"], a1)
            sc.label[e, i], sc.case[e, i] = c["label"], k
            if sc.policy[e, i] in (POL_LEARNING, POL_LEARNING_GA3C):
                sc.flags[e, i] |= IS_LEARNING | STILL_LEARNING
            if "want_heading" in c:
                sc.expect_heading[e, i] = c["want_heading"]
            if "want_td" in c:
                sc.expect_td[e, i] = c["want_td"]
            if "want_dist" in c:
                sc.expect_dist[e, i] = c["want_dist"]
            if "want_action" in c:
                w0, w1 = c["want_action"]
                if w0 is None and "speed_factor" in c:
                    w0 = sc.pref_speed[e, i] * c["speed_factor"]
                if w0 is not None:
                    sc.expect_action[e, i, 0] = w0
                sc.expect_action[e, i, 1] = w1
            arrives = sc.policy[e, i] == POL_STATIC or c.get("at_origin")
            sc.expect_flags[e, i] = AT_GOAL if arrives else 0
    return sc


def oracle_params(orc, sc):
    """OrcParams for a scene"""
    p = orc.default_params(sc.E, sc.N, max_obs=sc.max_obs, dt=sc.dt)
    for k, v in sc.params.items():
        setattr(p, k, v)
    return p


def sim_kwargs(sc):
    """keyword arguments of core.make_params for a scene"""
    return dict(sc.params, max_obs=sc.max_obs, dt=sc.dt)


def ext_actions(sc):
    """the external actions of every step, float64 [E, N, 2], or None for the classes whose policies are all internal"""
    return None if sc.cls in "nr" else sc.ext


def inject(o, sc):
    """oracle state := scene"""
    for n in Scene.FIELDS:
        o.s[n][:] = getattr(sc, n).reshape(-1)
    o.s["time_remaining"][:] = 60.0
    o.s["slt"][:] = 7.5
    for n in ("t", "ep_reward"):
        o.s[n][:] = 0.0
    o.s["turning_dir"][:] = sc.turning_dir.reshape(-1)
    o.s["last_action"][:] = 0.0
    o.s["flags"][:] = sc.flags.reshape(-1)
    o.s["policy"][:] = sc.policy.reshape(-1)
    o.s["dynamics"][:] = sc.dynamics.reshape(-1)
    for n in ("step_num", "episode_step", "reset_count"):
        o.s[n][:] = 0
    o.s["env_stats"][:] = 0.0


def oracle_step(orc, o, ext):
    """ca_oracle_step on the caller's external actions as they are: Oracle.step() would first put the GA3C-CADRL network's
    choice in place of the index these scenes hand to a GA3CCADRLPolicy agent"""
    e = None if ext is None else np.ascontiguousarray(ext, np.float64)
    rc = orc.lib().ca_oracle_step(C.byref(o.p), C.byref(o.cs), C.byref(o.co), None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)))
    assert rc == 0
