"""Deterministic ORCA scenes (numpy only) for tests/test_orca_scenes_host.py and tests/test_gpu_orca_edges.py: full agent
states -- positions, velocities, headings, goals, radii, preferred speeds, flags -- built to drive the ORCA phases of the
step kernels where the fixture episodes never go.  build(cls, N, E) -> Scene; inject(o, scene) writes one into an
oracle.Oracle, from where the GPU tests upload it (tests/test_gpu_parity.py::_upload).

Classes (every env is drawn from a generator seeded by (class, N, env), so a scene with fewer envs is a prefix of one with
more):
  a  crowded: uniform positions in a square so small that discs commonly overlap at 1.05 x radius (the radius RVOPolicy
     hands to rvo2) and some bodies truly overlap, most envs with a knot of four agents that overlap deeply; random
     velocities up to 1.2 x preferred speed, random goals.
  b  near-overlap band: chained partners at a centre distance strictly between r_a + r_b and 1.05 (r_a + r_b): rvo2 takes its
     collision branch (invTimeStep) while the env sees no collision, so these agents stay live on later steps.
  c  symmetric and tied, every coordinate exactly representable in float32, rvo_max_neighbors = min(N - 2, 5) < N - 1 (1 for
     N = 2); three layouts, env e takes layout e % 3: a square lattice whose rows are collinear agents with one common
     velocity (parallel and anti-parallel half-planes: |det| <= eps in linear programme 1 and 3; every third such env in the
     band of class b), head-on pairs on the two axes (the det(relativePosition, w) > 0 tie), integer points of a circle.
  d  boxed in: a patch of a honeycomb whose spacing lies in the band of class b, every velocity zero, every agent slow; agent
     0 sits in the middle and wants to drive into one of the three neighbours around it (six more stand in the next ring).
     Three band neighbours 120 degrees apart each demand a velocity away from them, so linear programme 2 is infeasible
     for every agent that has all three (agent 0 from N = 4 on).  The bodies do not touch: the agents stay live.  (A hexagonal patch would put neighbours exactly opposite each other: anti-parallel lines far
     from the origin, where the float32 programme as published loses its optimum -- see tests/test_orca_scenes_host.py.)
  e  horizon edge: sensing_horizon = 4 m; around agent 0 (at the origin) agents 1, 2, 3 stand at a float32 distance exactly
     at, one ulp inside and one ulp outside the horizon (N < 4: the kinds rotate with the env), the others are scattered on
     both sides of it.  build("e", ..., max_neighbors=1) is the same scene with rvo_max_neighbors = 1.
  f  far from the origin: class a translated by (+-3e4, +-3e4) m, where float32 positions quantise to about 2 mm (inside the
     documented 1e8 m range of INTEGRATION.md).
  g  ragged: class a with ragged = 1 and a random number of absent trailing slots (they enter ORCA at infinity).
  h  per-agent collaboration: class a with an rvo_collab array of 0, 0.5 and 1.

Left out on purpose: two agents with identical position AND identical velocity.  RVO2 itself returns NaN there (w = 0 is
normalised), so it is not a defined case; no builder produces it (checked by the host tests: every oracle velocity is finite).
"""
import math

import numpy as np

CLASSES = "abcdefgh"
ABSENT, DONE, AT_GOAL, WAS_AT_GOAL = 1 << 16, 1 << 5, 1 << 0, 1 << 1    # oracle/ca_oracle.h
HORIZON = 4.0
FAR = 3.0e4

# launch path -> (N, E): E = two full tiles of the path's kernel plus a partial one
PIPE_TILE = {2: 32, 3: 21, 4: 16, 5: 12, 6: 10, 8: 8, 10: 4}


def tiled_envs(N):
    """envs per workgroup of ca_kernel at a small batch (launch_any, csrc/cagpu_launch.inc)"""
    return 4 if N == 10 else 64 // N


PATHS = {
    "pipelined": [(N, 2 * te + 1) for N, te in sorted(PIPE_TILE.items())],
    "tiled": [(N, 2 * tiled_envs(N) + 1) for N in (10, 7, 9)],
    "gs16": [(N, 2 * tiled_envs(N) + 1) for N in (11, 13, 16)],
    "wave": [(N, 2 * tiled_envs(N) + 1) for N in (17, 20, 33, 64)],
    "big": [(65, 3), (100, 3)],
}
SHAPES = sorted({ne for v in PATHS.values() for ne in v})


class Scene(object):
    """state arrays [E, N] float64 (flags: uint32), parameter overrides, optional float32 [E, N] collaboration array"""
    FIELDS = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed")

    def __init__(self, cls, E, N):
        self.cls, self.E, self.N = cls, E, N
        for n in self.FIELDS:
            setattr(self, n, np.zeros((E, N), np.float64))
        self.pref_speed[:] = 1.0
        self.flags = np.zeros((E, N), np.uint32)
        self.params = {}          # sensing_horizon / rvo_max_neighbors / ragged
        self.collab = None


# per-class seeds: chosen once so that the conditions of tests/test_orca_scenes_host.py hold for the oracle alone (its path
# conditions, and its brute-force comparison: the float32 programme as published loses the min-max optimum where two violated
# lines are anti-parallel to within ~0.02 degrees far from the origin, which other seeds of classes a, b and f do contain)
SEEDS = {"a": 11, "b": 4, "c": 0, "d": 0, "e": 0, "f": 0, "g": 0, "h": 0}


def _rng(cls, N, e):
    return np.random.default_rng([ord(cls), N, e, SEEDS[cls]])


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _put(sc, e, pos, vel, goal, radius, speed, heading=None):
    sc.pos_x[e], sc.pos_y[e] = pos[:, 0], pos[:, 1]
    sc.vel_x[e], sc.vel_y[e] = vel[:, 0], vel[:, 1]
    sc.goal_x[e], sc.goal_y[e] = goal[:, 0], goal[:, 1]
    sc.radius[e], sc.pref_speed[e] = radius, speed
    sc.heading[e] = np.arctan2(goal[:, 1] - pos[:, 1], goal[:, 0] - pos[:, 0]) if heading is None else heading


def _random_motion(rng, pos, speed):
    N = pos.shape[0]
    v = rng.uniform(0.0, 1.2, N) * speed
    a = rng.uniform(-math.pi, math.pi, N)
    vel = np.stack([v * np.cos(a), v * np.sin(a)], -1)
    g = rng.uniform(2.0, 8.0, N)
    b = rng.uniform(-math.pi, math.pi, N)
    goal = pos + np.stack([g * np.cos(b), g * np.sin(b)], -1)
    return vel, goal, rng.uniform(-math.pi, math.pi, N)




KNOT = 0.2


def _crowd_env(rng, N):
    """test_orca_random_crowded_configurations' density at its crowded end (half-width 1.2 .. 2.5 m for 10 agents of radius
    0.2 .. 0.6, the area scaled with N).  In seven envs of ten the first (up to) four agents form a knot a few decimetres
    across: each of them overlaps the other three deeply, every one of those collision-branch lines lies outside the speed
    disc on its own, so linear programme 3 starts at the first line and has three lines acting -- what the few lines of a
    small agent count otherwise almost never give.  (Packing the WHOLE env like that was tried: with dozens of deep lines per
    query some pair is nearly anti-parallel in almost every env, and the float32 programme then misses the brute force.)"""
    half = rng.uniform(1.2, 2.5) * math.sqrt(N / 10.0)
    pos = rng.uniform(-half, half, (N, 2))
    if rng.uniform() < 0.7:      # a knot: the first (up to) four agents within a few decimetres of each other
        k = min(N, 4)
        pos[:k] = pos[0] + rng.uniform(-KNOT, KNOT, (k, 2))
    radius = rng.uniform(0.2, 0.6, N)
    speed = rng.uniform(0.5, 1.5, N)
    vel, goal, heading = _random_motion(rng, pos, speed)
    return pos, vel, goal, radius, speed, heading


def _build_a(sc, e, rng):
    _put(sc, e, *_crowd_env(rng, sc.N))


def _build_b(sc, e, rng):
    N = sc.N
    half = rng.uniform(1.0, 2.5) * math.sqrt(N / 10.0)
    radius = rng.uniform(0.2, 0.6, N)
    speed = rng.uniform(0.5, 1.5, N)
    pos = np.zeros((N, 2))
    for i in range(N):
        if i % 3 == 0:                      # an anchor; the next two agents chain on to it
            pos[i] = rng.uniform(-half, half, 2)
        else:
            d = (radius[i - 1] + radius[i]) * rng.uniform(1.005, 1.045)
            a = rng.uniform(-math.pi, math.pi)
            pos[i] = pos[i - 1] + d * np.array([math.cos(a), math.sin(a)])
    vel, goal, heading = _random_motion(rng, pos, speed)
    _put(sc, e, pos, vel, goal, radius, speed, heading)


def circle_points(N):
    """N integer points of a circle x^2 + y^2 = R^2 (R = 5, 25, 65, 1105: products of primes 4k + 1), whole orbits of the
    circle's symmetry group first, mirror images adjacent -> (points [N, 2], R)"""
    for R in (5, 25, 65, 1105):
        orbits = [[(R, 0), (-R, 0), (0, R), (0, -R)]]
        for a in range(1, R):
            b = int(round(math.sqrt(R * R - a * a)))
            if b * b + a * a == R * R and a < b:
                orbits.append([(a, b), (a, -b), (-a, b), (-a, -b), (b, a), (b, -a), (-b, a), (-b, -a)])
        pts = [p for o in orbits for p in o]
        if len(pts) >= N:
            return np.array(pts[:N], np.float64), R
    raise ValueError("no circle with %d integer points" % N)


def _build_c(sc, e, rng):
    N = sc.N
    layout, k = e % 3, e // 3
    radius = np.full(N, (0.25, 0.375, 0.5)[k % 3] if layout == 1 else 0.25)
    speed = np.ones(N)
    pos, vel, goal = np.zeros((N, 2)), np.zeros((N, 2)), np.zeros((N, 2))
    if layout == 0:      # square lattice (at least three agents to a row), the rows moving against each other: the agents of a
        # row are collinear and share one velocity, so their half-planes are exactly parallel / anti-parallel; pitch
        # 0.5078125 = 2 r (1 + 1 / 64) lies inside the band of class b, where anti-parallel lines leave nothing permitted
        side = max(3, int(math.ceil(math.sqrt(N))))
        pitch = (0.5078125, 0.75, 1.0)[k % 3]
        for i in range(N):
            r, c = divmod(i, side)
            pos[i] = (c * pitch, r * pitch)
            vel[i] = (0.5 if r % 2 == 0 else -0.5, 0.0)
            goal[i] = pos[i] + 8.0 * vel[i]
    elif layout == 1:    # head-on pairs: pair p on the x axis (p even) or the y axis (p odd), further out with p
        scale = (1.0, 1.25, 0.75, 1.5)[k % 4]
        for i in range(N):
            p, side = i // 2, 1.0 if i % 2 == 0 else -1.0
            d = (2.0 + 1.5 * (p // 2)) * scale
            ax = np.array([1.0, 0.0]) if p % 2 == 0 else np.array([0.0, 1.0])
            pos[i], vel[i], goal[i] = -side * d * ax, side * ax, side * (d + 4.0) * ax
    else:                # integer points of a circle, everybody heading for the antipode
        pts, R = circle_points(N)
        s = 2.0 ** -round(math.log2(R / max(2.5, N / 5.0))) * (1.0, 2.0)[k % 2]   # about a metre of arc per agent (or two)
        pos = pts * s
        vel = -pos * 2.0 ** -math.ceil(math.log2(R * s))                    # speed in (0.5, 1]
        goal = -pos
    pos, vel, goal = pos + 0.0, vel + 0.0, goal + 0.0     # (no negative zeros)
    assert all(np.array_equal(x, _f32(x)) for x in (pos, vel, goal, radius))
    _put(sc, e, pos, vel, goal, radius, speed, np.round(np.arctan2(vel[:, 1], vel[:, 0]) * 4.0) / 4.0)


def honeycomb_points(N):
    """the N vertices of the unit honeycomb closest to one of them, that one first (at the origin).  Every inner vertex has
    three neighbours at distance 1, 120 degrees apart, and nobody opposite: the triangular lattice i a1 + j a2 without its
    sublattice (i - j) % 3 == 0"""
    m = int(math.ceil(math.sqrt(N))) + 3
    pts = [(i - 1 + 0.5 * j, j * math.sqrt(3.0) / 2.0) for i in range(-m, m + 1) for j in range(-m, m + 1) if (i - j) % 3]
    pts.sort(key=lambda p: (round(p[0] * p[0] + p[1] * p[1], 6), round(math.atan2(p[1], p[0]), 6)))
    return np.array(pts[:N], np.float64)


def _build_d(sc, e, rng):
    N = sc.N
    r = rng.uniform(0.3, 0.6)
    radius = np.full(N, r)
    # slow agents: a band neighbour at pitch 2 r f demands 0.5 x (2.1 - 2 f) r / dt = 0.09 .. 0.24 m/s away from it, which is more
    # than many of these agents can do, so linear programme 2 often fails at its FIRST line and linear programme 3 then has all
    # three band lines to act on; the bodies do not touch, so nearly all of these agents are queried on the later steps too
    speed = rng.uniform(0.05, 0.3, N)
    rot = rng.uniform(-math.pi, math.pi)
    c, s = math.cos(rot), math.sin(rot)
    pitch = 2.0 * r * rng.uniform(1.01, 1.02)
    pos = honeycomb_points(N) @ np.array([[c, s], [-s, c]]) * pitch + rng.uniform(-0.002 * r, 0.002 * r, (N, 2))
    _, goal, heading = _random_motion(rng, pos, speed)
    goal[0] = pos[0] + 5.0 * (pos[1] - pos[0]) / np.hypot(*(pos[1] - pos[0]))   # into a neighbour
    _put(sc, e, pos, np.zeros((N, 2)), goal, radius, speed, heading)


def horizon_offsets():
    """float32 distances exactly at, one ulp inside, one ulp outside the horizon"""
    h = np.float32(HORIZON)
    return [float(h), float(np.nextafter(h, np.float32(0.0))), float(np.nextafter(h, np.float32(np.inf)))]


def _build_e(sc, e, rng):
    N = sc.N
    pos = _f32(rng.uniform(-3.5, 3.5, (N, 2)))
    pos[0] = 0.0
    dirs = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
    offs = horizon_offsets()
    for i in range(1, min(N, 4)):
        kind = (i - 1 + e) % 3 if N < 4 else i - 1
        pos[i] = np.array(dirs[(i + e) % 4]) * offs[kind]
    radius = rng.uniform(0.2, 0.5, N)
    speed = rng.uniform(0.5, 1.5, N)
    vel, goal, heading = _random_motion(rng, pos, speed)
    for i in range(1, min(N, 4)):        # the marked agents drive at agent 0 and agent 0 at the first of them: their lines bind
        u = pos[i] / np.hypot(*pos[i])
        vel[i], goal[i] = -speed[i] * u, -2.0 * pos[i]
    u = pos[1] / np.hypot(*pos[1])
    vel[0], goal[0] = speed[0] * u, 2.0 * pos[1]
    _put(sc, e, pos, vel, goal, radius, speed, heading)


def _build_f(sc, e, rng):
    pos, vel, goal, radius, speed, heading = _crowd_env(_rng("a", sc.N, e), sc.N)     # class a's own envs
    off = np.array([FAR if e & 1 else -FAR, FAR if e & 2 else -FAR])
    _put(sc, e, pos + off, vel, goal + off, radius, speed, heading)


def _build_g(sc, e, rng):
    N = sc.N
    _put(sc, e, *_crowd_env(_rng("a", N, e), N))
    present = int(rng.integers(max(1, (N + 1) // 2), N + 1)) if e % 3 else N   # (every third env is full)
    for n in Scene.FIELDS:      # an empty slot as the reset leaves it (oracle/ca_oracle.cpp reset_env)
        getattr(sc, n)[e, present:] = 1.0 if n == "pref_speed" else 0.0
    sc.flags[e, present:] = ABSENT | DONE | AT_GOAL | WAS_AT_GOAL


def _build_h(sc, e, rng):
    _put(sc, e, *_crowd_env(_rng("a", sc.N, e), sc.N))
    sc.collab[e] = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), sc.N)


def build(cls, N, E, max_neighbors=None):
    sc = Scene(cls, E, N)
    if cls == "h":
        sc.collab = np.zeros((E, N), np.float32)
    fn = globals()["_build_" + cls]
    for e in range(E):
        fn(sc, e, _rng(cls, N, e))
    if cls == "c":
        sc.params["rvo_max_neighbors"] = max(1, min(N - 2, 5))
    if cls == "e":
        sc.params["sensing_horizon"] = HORIZON
    if cls == "g":
        sc.params["ragged"] = 1
    if max_neighbors is not None:
        sc.params["rvo_max_neighbors"] = int(max_neighbors)
    return sc


def oracle_params(orc, sc):
    """OrcParams for a scene"""
    p = orc.default_params(sc.E, sc.N, rvo_max_neighbors=sc.params.get("rvo_max_neighbors"), ragged=sc.params.get("ragged", 0))
    p.sensing_horizon = sc.params.get("sensing_horizon", math.inf)
    return p


def inject(o, sc):
    """oracle state := scene: live RVO agents with unicycle dynamics at the start of a long episode"""
    for n in Scene.FIELDS:
        o.s[n][:] = getattr(sc, n).reshape(-1)
    o.s["time_remaining"][:] = 60.0
    o.s["slt"][:] = 7.5
    for n in ("t", "ep_reward", "turning_dir"):
        o.s[n][:] = 0.0
    o.s["last_action"][:] = 0.0
    o.s["flags"][:] = sc.flags.reshape(-1)
    absent = (sc.flags.reshape(-1) & ABSENT) != 0
    o.s["time_remaining"][absent] = 0.0
    o.s["slt"][absent] = 0.0
    o.s["policy"][:] = 0        # RVO
    o.s["dynamics"][:] = 0      # unicycle
    for n in ("step_num", "episode_step", "reset_count"):
        o.s[n][:] = 0
    o.s["env_stats"][:] = 0.0
    o.set_rvo_stochastic(collab=sc.collab)


def orca_inputs(sc):
    """what RVOPolicy feeds rvo2 from a scene (float32, like oracle/ca_oracle.cpp step_env) -> pos, vel [E, N, 2], radius [E, N],
    present [E, N]"""
    pos = np.stack([sc.pos_x, sc.pos_y], -1).astype(np.float32)
    vel = np.stack([sc.vel_x, sc.vel_y], -1).astype(np.float32)
    radius = ((1 + 5e-2) * sc.radius).astype(np.float32)
    return pos, vel, radius, (sc.flags & ABSENT) == 0


def pair_dist_sq(sc):
    """float32 distSq of every ordered pair as orca_ref::neighbours forms it -> [E, N, N], inf on the diagonal and for absent slots"""
    pos, _, _, present = orca_inputs(sc)
    d = pos[:, :, None, :] - pos[:, None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
    idx = np.arange(sc.N)
    d2[:, idx, idx] = np.inf
    d2[~(present[:, :, None] & present[:, None, :])] = np.inf
    return d2
