"""The angle-edge scenes of tests/move_scenes.py held to their purpose on the CPU, before tests/test_gpu_move_edges.py runs the
step kernels on them:
  (1) restatement: a plain Python float64 restatement of the reference's lines (below, each under its citation) agrees with the
      oracle EXACTLY, by bits, on every value that no sin / cos / atan2 feeds and on every discrete outcome: the new heading in
      classes h, d, m, turning_dir in d and m, the float32 action in a and wherever the scene fixes it, the at-goal flag, the
      clip of the RVO action, dist_to_goal and the unnormalised ego frame in n.  Where libm feeds a value (positions, velocities,
      the headings of classes n and r) the restatement calls CPython's math module and is held to 1e-12;
  (2) branch counts: the restatement counts every branch it takes; every branch the module docstring of move_scenes lists is
      taken by at least one agent at N = 2 and at N = 65 (the table is printed), the scene's own expectations are the oracle's,
      and no episode ends in the first step;
  (3) mutations: one-comparison mutations of the restatement -- `>=` <-> `>` and `<` <-> `<=` in wrap, `<` <-> `<=` at 1e-5, the
      clamp constants +-pi and +-3, `>` <-> `>=` at pi / 6 and at 1e-8 -- each make (1) fail.  The `ang == 0` case of the RVO
      action is the exception, and the test says why: it differs from `ang` only for ang = -0, which needs dpy = -0 beside
      dpx > 0, and dpy = float32 position - float64 position is +0 whenever it is zero (move_scenes docstring, class r);
  (4) golden: tests/golden/move_rules.npz was recorded by oracle/gen_move_golden.py from the unmodified reference on classes h,
      d, m, a (external, learning) and n at N = 2 .. 6.  The oracle equals it exactly wherever no sin / cos / atan2 feeds the
      value (headings of h, d, m, turning_dir, actions of a, flags, goals, clocks) and within TOL of tests/test_oracle_golden.py
      elsewhere (numpy's sin and cos need not be glibc's).  One documented exception, the one test_oracle_golden.py makes for
      mixed5: under numpy >= 2 the reference evaluates `action[1] / dt` of UnicycleDynamicsMaxTurnRate.py:31 in float32; the
      oracle and the kernels follow the float64 reading, so the headings of max-turn-rate agents are held to 1e-7 there;
  (5) the np.longdouble reference that tests/test_gpu_move_edges.py measures sincos_heading with (tests/sincos_ref.py), against
      mpmath at 40 digits on the edge operands, where mpmath imports."""
import math
import os

import numpy as np
import pytest

from oracle import ca_oracle as orc
from tests import move_scenes as M
from tests import sincos_ref as SR

TOL = 1e-5               # tests/test_oracle_golden.py
TOL_MAXTURN = 1e-7       # tests/test_oracle_golden.py REINJECT_TOL["mixed5"]
LIBM = 1e-12
PI = math.pi
NEAR_GOAL = 0.2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "move_rules.npz")
SHAPES = ((2, 65), (65, 3))
MUTATIONS = ("wrap>=", "wrap<", "td<", "td_clamp", "turn_clamp", "pi6", "dist")


def _oracle(sc):
    o = orc.Oracle(M.oracle_params(orc, sc))
    M.inject(o, sc)
    return o


# ---------------------------------------------------------------- (1) the restatement
class Restatement(object):
    """one step of one agent in plain Python float64; mut: the name of ONE mutated comparison or constant (None: none);
    count: {branch name: times taken}"""

    def __init__(self, dt, mut=None):
        self.dt, self.mut, self.count = dt, mut, {}
        # network.py:7-16, as written there
        a = np.mgrid[1.0:1.1:0.5, -np.pi / 6:np.pi / 6 + 0.01:np.pi / 12].reshape(2, -1).T
        a = np.vstack([a, np.mgrid[0.5:0.6:0.5, -np.pi / 6:np.pi / 6 + 0.01:np.pi / 6].reshape(2, -1).T])
        self.actions = np.vstack([a, np.mgrid[0.0:0.1:0.5, -np.pi / 6:np.pi / 6 + 0.01:np.pi / 6].reshape(2, -1).T])

    def took(self, name):
        self.count[name] = self.count.get(name, 0) + 1

    def wrap(self, a, what):      # util.py:141-146
        n = 0
        while (a > PI) if self.mut == "wrap>=" else (a >= PI):
            a -= 2 * PI
            n -= 1
        while (a <= -PI) if self.mut == "wrap<" else (a < -PI):
            a += 2 * PI
            n += 1
        self.took("%s wrap %s" % (what, "none" if n == 0 else ("-2pi" if n == -1 else "+2pi" if n == 1 else "general loop")))
        return a

    def get_ref(self, px, py, gx, gy):      # agent.py:329-349
        dx, dy = gx - px, gy - py
        dist = math.sqrt(dx ** 2 + dy ** 2)
        if (dist >= 1e-8) if self.mut == "dist" else (dist > 1e-8):
            self.took("dist > 1e-8")
            prll = (dx / dist, dy / dist)
        else:
            self.took("dist <= 1e-8")
            prll = (dx, dy)
        return dist, prll, (-prll[1], prll[0])

    def heading_ego(self, prll, heading):      # Dynamics.py:24-41
        return self.wrap(heading - math.atan2(prll[1], prll[0]), "ego")

    def action(self, a, ext, orca_vel):
        """the policy's [speed, heading change] before the float32 store; may move a's goal (StaticPolicy)"""
        pol = a["policy"]
        if pol == M.POL_RVO:      # RVOPolicy.py:96-111 (orca_vel: what rvo2 chose, float32; Agent::update adds v * timeStep in float)
            new = [np.float32(a["px"]) + np.float32(orca_vel[0]) * np.float32(self.dt),
                   np.float32(a["py"]) + np.float32(orca_vel[1]) * np.float32(self.dt)]
            dpx, dpy = float(new[0]) - a["px"], float(new[1]) - a["py"]
            ang1, ang2 = math.atan2(dpy, dpx), math.atan2(0, 1)
            self.took("ang == 0" if ang1 == 0 else ("ang < 0" if ang1 < 0 else "ang > 0"))
            if self.mut == "ang0":      # the kernel's text of `%` without its `ang == 0.0` case
                nh = ang1 + 2 * PI if ang1 < 0.0 else ang1
            else:
                nh = (ang1 - ang2) % (2 * PI)
            dh = self.wrap(nh - a["heading"], "rvo")
            spd = 1 / self.dt * math.sqrt(dpx ** 2 + dpy ** 2)      # np.linalg.norm of two components
            if dpx == 0.0 and dpy == 0.0:
                self.took("zero displacement")
            if (abs(dh) >= PI / 6) if self.mut == "pi6" else (abs(dh) > PI / 6):
                self.took("clipped at pi/6")
                dh = float(np.sign(dh)) * (PI / 6)
                spd = 0.
            else:
                self.took("not clipped")
            return spd, dh
        if pol == M.POL_NONCOOP:      # NonCooperativePolicy.py:21
            _, prll, _ = self.get_ref(a["px"], a["py"], a["gx"], a["gy"])
            return a["pref_speed"], -self.heading_ego(prll, a["heading"])
        if pol == M.POL_STATIC:      # StaticPolicy.py:21-23
            a["gx"], a["gy"] = a["px"], a["py"]
            self.took("static")
            return 0.0, 0.0
        if ext is None:      # (an external policy that is handed nothing: the zero row of all_actions)
            return 0.0, 0.0
        if pol == M.POL_EXTERNAL:      # ExternalPolicy.py:14-16
            return ext[0], ext[1]
        if pol == M.POL_LEARNING:      # LearningPolicy.py:29-33
            return a["pref_speed"] * ext[0], M.MAX_HEADING_CHANGE * (2. * ext[1] - 1.)
        # LearningPolicyGA3C.py:24-26 / GA3CCADRLPolicy.py:81-84; int() truncates, the C ABI clamps the index to 0 .. 10
        q = int(ext[0])
        self.took("index < 0" if q < 0 else ("index > 10" if q > 10 else ("index truncated" if q != ext[0] else "index %d" % q)))
        raw = self.actions[min(max(q, 0), 10)]
        return a["pref_speed"] * raw[0], raw[1]

    def move(self, a, act):
        """agent.py:192-241 with the float32 action `act`"""
        a0, a1 = float(act[0]), float(act[1])
        if a["dynamics"] == M.DYN_MAX_TURN_RATE:      # UnicycleDynamicsMaxTurnRate.py:31-33 (float64: see the module docstring)
            lim = M.up(3.0) if self.mut == "turn_clamp" else 3.0
            rate = a1 / self.dt
            self.took("turn rate " + ("clamped +" if rate > lim else "clamped -" if rate < -lim else
                                      "on the clamp" if abs(rate) == lim else "inside"))
            rate = min(max(rate, -lim), lim)
            nh = self.wrap(rate * self.dt + a["heading"], "move")
        else:
            nh = self.wrap(a1 + a["heading"], "move")      # UnicycleDynamics.py:28
        a["px"] += a0 * math.cos(nh) * self.dt      # :30-32
        a["py"] += a0 * math.sin(nh) * self.dt
        a["vx"], a["vy"] = a0 * math.cos(nh), a0 * math.sin(nh)      # :34-35
        a["heading"] = nh
        if a["dynamics"] == M.DYN_UNICYCLE:      # :41-47
            td = a["td"]
            lim = M.up(PI) if self.mut == "td_clamp" else PI
            if (abs(td) <= 1e-5) if self.mut == "td<" else (abs(td) < 1e-5):
                self.took("td: |td| < 1e-5, nh %s" % ("> 0" if nh > 0 else "< 0" if nh < 0 else "zero"))
                a["td"] = 0.11 * float(np.sign(nh))
            elif td * nh < 0:
                s = -td + nh
                self.took("td: flips" + (", clamped +" if s > lim else ", clamped -" if s < -lim else ""))
                a["td"] = max(-lim, min(lim, s))
            else:
                self.took("td: decays" + (" to 0" if abs(td) - 0.1 <= 0.0 else ""))
                a["td"] = float(np.sign(td)) * max(0.0, abs(td) - 0.1)
        else:
            self.took("td: max turn rate, unchanged")
        # agent.py:150-153
        a["at_goal"] = (a["px"] - a["gx"]) ** 2 + (a["py"] - a["gy"]) ** 2 <= NEAR_GOAL ** 2

    def step(self, a, ext, orca_vel):
        spd, dh = self.action(a, ext, orca_vel)
        act = np.array([spd, dh]).astype(np.float32)      # collision_avoidance_env.py:305-307
        self.move(a, act)
        a["dist"], a["prll"], a["orth"] = self.get_ref(a["px"], a["py"], a["gx"], a["gy"])
        a["heading_ego"] = self.heading_ego(a["prll"], a["heading"])
        a["act"] = act
        return a


def _agents(sc, e):
    return [dict(px=float(sc.pos_x[e, i]), py=float(sc.pos_y[e, i]), gx=float(sc.goal_x[e, i]), gy=float(sc.goal_y[e, i]),
                 heading=float(sc.heading[e, i]), pref_speed=float(sc.pref_speed[e, i]), td=float(sc.turning_dir[e, i]),
                 policy=int(sc.policy[e, i]), dynamics=int(sc.dynamics[e, i])) for i in range(sc.N)]


def _b64(x):
    return np.asarray(x, np.float64).view(np.int64)


def _b32(x):
    return np.asarray(x, np.float32).view(np.int32)


def _disagreements(sc, o, mut=None, count=None):
    """one oracle step has been taken from the scene -> the list of values on which the restatement (mutated or not) differs
    from the oracle: exact ones by bits, libm-fed ones beyond LIBM"""
    R = Restatement(sc.dt, mut)
    ext = M.ext_actions(sc)
    bad = []
    no_libm_heading = sc.cls in "hdma"      # ExternalPolicy and the learning policies: the heading is a sum of given numbers
    for e in range(sc.E):
        agents = [R.step(a, None if ext is None else ext[e, i], o.orca_vel[e, i]) for i, a in enumerate(_agents(sc, e))]
        for i, a in enumerate(agents):
            k = e * sc.N + i
            exact = [("action", _b32(a["act"]), _b32(o.actions[e, i])) if sc.cls in "a" or not np.isnan(sc.expect_action[e, i]).any()
                     else ("action", 0, 0),
                     ("turning_dir", _b64(a["td"]), _b64(o.s["turning_dir"][k])),
                     ("at_goal", int(a["at_goal"]), int(o.s["flags"][k] & M.AT_GOAL)),
                     ("goal", _b64([a["gx"], a["gy"]]), _b64([o.s["goal_x"][k], o.s["goal_y"][k]])),
                     ("speed is 0", a["act"][0] == 0, o.actions[e, i, 0] == 0),
                     ("dist_to_goal", _b64(a["dist"]), _b64(o.obs[e, i, 2]))]
            if no_libm_heading or not np.isnan(sc.expect_heading[e, i]):
                exact.append(("heading", _b64(a["heading"]), _b64(o.s["heading"][k])))
            if sc.label[e, i] in (5, 6, 7, 8) and sc.cls == "n" and sc.N > 1:      # dist <= 1e-8 or next to it: p_parallel and
                j = (i + 1) % sc.N                                               # p_orth of the first other agent, no libm in them
                rx, ry = agents[j]["px"] - a["px"], agents[j]["py"] - a["py"]
                row = o.obs[e, i, 6:].reshape(sc.max_obs, 7)
                slot = [s for s in range(sc.max_obs) if row[s, 4] == sc.radius[e, j]]
                if np.isfinite([rx, ry]).all() and len(slot) == 1:
                    exact.append(("p_parallel", _b64(rx * a["prll"][0] + ry * a["prll"][1]), _b64(row[slot[0], 0])))
                    exact.append(("p_orth", _b64(rx * a["orth"][0] + ry * a["orth"][1]), _b64(row[slot[0], 1])))
            for name, mine, theirs in exact:
                if not np.array_equal(mine, theirs):
                    bad.append((name, e, i, int(sc.label[e, i])))
            for name, mine, theirs in (("pos_x", a["px"], o.s["pos_x"][k]), ("pos_y", a["py"], o.s["pos_y"][k]),
                                       ("vel_x", a["vx"], o.s["vel_x"][k]), ("vel_y", a["vy"], o.s["vel_y"][k]),
                                       ("heading", a["heading"], o.s["heading"][k]), ("heading_ego", a["heading_ego"], o.obs[e, i, 3])):
                d = abs(mine - theirs)
                if name.startswith("heading"):
                    d = min(d, abs(d - 2 * PI))
                if not d <= LIBM:
                    bad.append((name + " (libm)", e, i, int(sc.label[e, i])))
    if count is not None:
        for k, v in R.count.items():
            count[k] = count.get(k, 0) + v
    return bad


CASES = [(cls, v) for cls in M.CLASSES for v in M.VARIANTS[cls]]
_stepped = {}


def _stepped_scene(cls, variant, N, E):
    """(scene, oracle after its first step): computed once, shared, left unchanged"""
    key = (cls, variant, N, E)
    if key not in _stepped:
        sc = M.build(cls, N, E, variant)
        o = _oracle(sc)
        M.oracle_step(orc, o, M.ext_actions(sc))
        _stepped[key] = (sc, o)
    return _stepped[key]


def test_scenes_are_deterministic_prefixes():
    for cls, v in CASES:
        a, b = M.build(cls, 6, 3, v), M.build(cls, 6, 5, v)
        for n in M.Scene.FIELDS + ("flags", "policy", "dynamics", "turning_dir", "ext", "label", "case"):
            assert np.array_equal(getattr(b, n)[:3], getattr(a, n)), (cls, v, n)
        assert a.max_obs == b.max_obs and a.params == b.params


def test_recorded_scenes_take_every_case_once():
    from oracle import gen_move_golden as G
    for cls, v in G.RECORDED:
        seen = np.concatenate([M.build(cls, N, G.ENVS, v).case.reshape(-1) for N in G.AGENT_COUNTS])
        n = len(M.cases(cls, v))
        assert seen.size == M.MAX_CASES and set(seen.tolist()) == set(range(n)), (cls, v)


# every branch section (2) asks for, by the name the restatement counts it under
REQUIRED = {
    "h": ["move wrap none", "move wrap -2pi", "move wrap +2pi", "move wrap general loop", "turn rate clamped +", "turn rate clamped -",
          "turn rate inside"],
    "d": ["td: |td| < 1e-5, nh > 0", "td: |td| < 1e-5, nh < 0", "td: |td| < 1e-5, nh zero", "td: flips", "td: flips, clamped +",
          "td: flips, clamped -", "td: decays", "td: decays to 0", "td: max turn rate, unchanged"],
    "m": ["turn rate on the clamp", "turn rate inside", "turn rate clamped +", "turn rate clamped -", "td: max turn rate, unchanged"],
    "a": ["index < 0", "index > 10", "index truncated"] + ["index %d" % q for q in range(11)],
    "n": ["static", "dist > 1e-8", "dist <= 1e-8", "ego wrap none", "ego wrap -2pi", "move wrap -2pi", "move wrap none"],
    "r": ["ang == 0", "ang < 0", "ang > 0", "clipped at pi/6", "not clipped", "zero displacement", "rvo wrap none", "rvo wrap -2pi"],
}


@pytest.mark.parametrize("N,E", SHAPES)
def test_restatement_equals_the_oracle_and_every_branch_is_taken(N, E):
    for cls in M.CLASSES:
        count, labels = {}, {}
        for v in M.VARIANTS[cls]:
            sc, o = _stepped_scene(cls, v, N, E)
            bad = _disagreements(sc, o, None, count)
            assert not bad, "%s %s N=%d: the restatement differs from the oracle: %s" % (cls, v, N, bad[:6])
            # the scene's own expectations are the oracle's, by bits
            for name, want, got, view in (("heading", sc.expect_heading, o.view("heading"), _b64),
                                          ("turning_dir", sc.expect_td, o.view("turning_dir"), _b64),
                                          ("dist_to_goal", sc.expect_dist, o.obs[..., 2], _b64),
                                          ("action", sc.expect_action, o.actions, _b32)):
                held = ~np.isnan(want)
                assert np.array_equal(view(want[held]), view(got[held])), (cls, v, N, name)
            assert np.array_equal(o.view("flags") & M.AT_GOAL, sc.expect_flags), (cls, v, N)
            assert not (o.view("flags") & (M.IN_COLLISION | M.OUT_OF_TIME)).any() and not o.game_over.any(), (cls, v, N)
            for lab in M.LABELS[cls]:
                labels[lab] = labels.get(lab, 0) + int((sc.label == lab).sum())
        print("move scenes %s N=%-2d: branches taken %s" % (cls, N, dict(sorted(count.items()))))
        print("move scenes %s N=%-2d: agents per label %s" % (cls, N, {M.LABELS[cls][k]: n for k, n in sorted(labels.items())}))
        for name in REQUIRED[cls]:
            assert count.get(name, 0) > 0, "%s N=%d: no agent takes the branch %r" % (cls, N, name)
        assert all(n > 0 for n in labels.values()), (cls, N, labels)


WHERE = {"wrap>=": ("h", "unicycle"), "wrap<": ("h", "unicycle"), "td<": ("d", ""), "td_clamp": ("d", ""), "turn_clamp": ("m", "pow2"),
         "pi6": ("r", ""), "dist": ("n", "")}


@pytest.mark.parametrize("mut", MUTATIONS)
def test_one_comparison_mutations_fail(mut):
    cls, v = WHERE[mut]
    for N, E in SHAPES:
        sc, o = _stepped_scene(cls, v, N, E)
        bad = _disagreements(sc, o, mut)
        names = sorted({b[0] for b in bad})
        print("mutation %-10s on %s %s N=%-2d: %3d values differ from the oracle (%s)" % (mut, cls, v or "-", N, len(bad), ", ".join(names)))
        assert bad, "the mutation %s goes unnoticed on class %s at N=%d" % (mut, cls, N)
        assert any(not n.endswith("(libm)") for n in names), "only libm-fed values notice the mutation %s" % mut


def test_the_ang_equals_zero_case_cannot_be_reached():
    """dropping the `ang == 0.0` case of the RVO action changes the result for ang = -0 alone: atan2(-0, dpx > 0).  dpy is
    float64(float32(py) + v_y ts) - py: a sum is -0 only if both terms are, so the float32 sum is -0 only for py = -0, and then
    dpy = (-0) - (-0) = +0.  The scenes try both signed zeros; the mutated restatement equals the oracle on all of class r."""
    for N, E in SHAPES:
        sc, o = _stepped_scene("r", "", N, E)
        assert not _disagreements(sc, o, "ang0")
    for py in (0.0, -0.0):
        for vy in (0.0, -0.0):
            new = np.float32(py) + np.float32(vy) * np.float32(0.1)
            assert M.bits(float(new) - py) == M.bits(0.0)


# ---------------------------------------------------------------- (4) the oracle against the reference
_gold = {}


def _golden():
    if not _gold:
        from oracle import gen_move_golden as G
        _gold.update(G.load(GOLDEN))
    return _gold


def _gold_cases():
    from oracle import gen_move_golden as G
    return [(cls, v, N) for cls, v in G.RECORDED for N in G.AGENT_COUNTS]


@pytest.mark.parametrize("cls,variant,N", _gold_cases(), ids=lambda v: str(v) if v != "" else "-")
def test_oracle_equals_the_reference_on_recorded_scenes(cls, variant, N):
    from oracle import gen_move_golden as G
    z = _golden()["%s_%s_%d" % (cls, variant or "-", N)]
    E = G.ENVS
    sc = M.build(cls, N, E, variant)
    o = _oracle(sc)
    col = {n: c for c, n in enumerate(G.STATE)}
    maxturn = sc.dynamics == M.DYN_MAX_TURN_RATE
    exact = 0
    for t in range(G.STEPS):
        M.oracle_step(orc, o, M.ext_actions(sc))
        what = "%s %s N=%d step %d" % (cls, variant, N, t)
        ref = lambda n: z["state"][t][..., col[n]]
        bits6 = np.uint32(0x3F)
        assert np.array_equal(z["flags"][t] & bits6, o.view("flags") & bits6), "flags " + what
        for n in ("goal_x", "goal_y", "time_remaining", "t"):
            assert np.array_equal(ref(n), o.view(n)), n + " " + what
            exact += ref(n).size
        # the action: exact where the policy takes it from the caller (no libm), one float32 ulp elsewhere (test_oracle_golden.py)
        given = np.isin(sc.policy, (M.POL_EXTERNAL, M.POL_LEARNING, M.POL_STATIC))
        act, mine = z["action"][t], o.s["last_action"].reshape(E, N, 2)
        assert np.array_equal(act[given], mine[given]), "action " + what
        np.testing.assert_allclose(mine, act, rtol=0, atol=2.5e-7, err_msg="action " + what)
        exact += int(given.sum()) * 2
        # heading and turning_dir: sums and comparisons of given numbers for these policies on the first step; afterwards, and
        # for NonCooperativePolicy, atan2 has fed them
        plain = given & (t == 0 or cls != "n") & ~maxturn
        for n in ("heading", "turning_dir"):
            assert np.array_equal(ref(n)[plain], o.view(n)[plain]), n + " " + what
            exact += int(plain.sum())
            d = np.abs(o.view(n) - ref(n))
            d = np.minimum(d, np.abs(d - 2 * PI)) if n == "heading" else d      # (1e-8 off in the turn changes the side of an edge)
            assert (d[maxturn] <= TOL_MAXTURN).all() and (d <= TOL).all(), "%s %s: %g" % (n, what, d.max())
        for n in ("pos_x", "pos_y", "vel_x", "vel_y"):
            np.testing.assert_allclose(o.view(n), ref(n), rtol=0, atol=TOL, err_msg=n + " " + what)
        mine = o.obs.astype(np.float32)
        assert np.array_equal(z["obs"][t][..., 1], mine[..., 1]), "num_other_agents_observed " + what
        K = sc.max_obs
        assert np.array_equal(z["obs"][t][..., 6:].reshape(E, N, K, 7)[..., 4:6], mine[..., 6:].reshape(E, N, K, 7)[..., 4:6]), \
            "who sits in a slot " + what
        d = np.abs(mine - z["obs"][t])
        d[..., 3] = np.minimum(d[..., 3], np.abs(d[..., 3] - np.float32(2 * PI)))      # heading_ego: an angle
        assert (d <= TOL).all(), "obs %s: %g" % (what, d.max())
        still = (z["action"][t][..., 0] == 0) & ~maxturn      # an agent that stands still has no libm in its dist_to_goal
        assert np.array_equal(z["obs"][t][..., 2][still], mine[..., 2][still]), "dist_to_goal " + what
    assert exact > 0


# ---------------------------------------------------------------- (5) the sin / cos reference itself
def test_long_double_reference_against_mpmath():
    pytest.importorskip("mpmath")
    x = SR.edge_operands()
    assert x.size > 400 and np.isfinite(x).all() and np.abs(x).max() < 3.1416
    worst = SR.mpmath_cross_check(x)
    print("np.longdouble sin / cos on %d edge operands: at most %.2g float64 ulps from mpmath at 40 digits" % (x.size, worst))
    assert worst < 2.0 ** -8      # (the reference measures a 1 ulp bar: its own error must not matter to it)


def test_operands_are_symmetric_and_hold_the_edges():
    x = SR.operands()
    h = x.size // 2
    assert np.array_equal(x[:h].view(np.int64), (-x[h:]).view(np.int64))
    have = set(x.view(np.int64).tolist())
    for v in (0.0, -0.0, math.pi, -math.pi, math.pi / 2, math.pi / 4, np.finfo(np.float64).tiny, 2.0 ** -60, M.up(math.pi), M.dn(-math.pi)):
        assert M.bits(v) in have, v
