"""The ORCA scenes of tests/orca_scenes.py held to their purpose on the CPU, before tests/test_gpu_orca_edges.py runs the step
kernels on them: (1) the oracle's linear-programme log shows that every (class, agent count) drives the programme where the
class is meant to, (2) on those scenes the oracle still agrees with the independent float64 brute force of
oracle/orca_bruteforce.py, (3) every class tells the oracle from a wrong variant of it by at least one velocity bit.

Path conditions (fixed in advance; the counts behind them are printed per (class, N)):
  a, d, f, g  >= 30 queries reach linear programme 3, >= 10 of them with two or more LATER lines acting (the lines after the
              first acting one: bits 16 .. of the log, i.e. three acting lines in all).  N = 2 and 3 build at most two lines
              per query, so that count is 0 there by construction and is not asked for.
  b           >= 30 half-planes built by the collision branch
  c           an exact float32 distSq tie in every env (N >= 3: one neighbour cannot tie) and a 1-D programme rejected by a
              parallel line (N >= 4: rvo_max_neighbors < N - 1 leaves a single line below that)
  e           neighbours on both sides of the horizon, the three marked ones included
Every condition is checked on the very scene the GPU test runs: the E of orca_scenes.PATHS."""
import numpy as np
import pytest

from oracle import ca_oracle as orc
from oracle import orca_bruteforce as bf
from tests import orca_scenes as S
from tests.test_orca_semantics import TOL, _check_env, _orca_inputs_from_state

AGENT_COUNTS = sorted({N for N, _ in S.SHAPES})
GPU_ENVS = dict(S.SHAPES)


def _oracle(sc, **override):
    p = S.oracle_params(orc, sc)
    for k, v in override.items():
        setattr(p, k, v)
    o = orc.Oracle(p)
    S.inject(o, sc)
    return o


def _ties(sc):
    """envs that hold an exact float32 distSq tie between two neighbours of one agent"""
    d2 = np.sort(S.pair_dist_sq(sc), axis=2)
    eq = (d2[:, :, 1:] == d2[:, :, :-1]) & np.isfinite(d2[:, :, 1:])
    return eq.any(axis=(1, 2))


@pytest.mark.parametrize("cls", S.CLASSES)
@pytest.mark.parametrize("N", AGENT_COUNTS)
def test_path_conditions(cls, N):
    E = GPU_ENVS[N]
    sc = S.build(cls, N, E)
    again = S.build(cls, N, E + 2)
    for n in S.Scene.FIELDS + ("flags",):       # deterministic, env by env
        assert np.array_equal(getattr(again, n)[:E], getattr(sc, n)), n
    o = _oracle(sc)
    lg = o.step_logged()
    assert np.isfinite(o.orca_vel).all()                 # (no 0 / 0: identical position and velocity is left out)
    d2 = S.pair_dist_sq(sc)
    ties = _ties(sc)
    pos, vel, radius, present = S.orca_inputs(sc)
    R = radius[:, :, None] + radius[:, None, :]
    band = int(((d2 <= R * R)).sum())                    # half-planes the collision branch builds with every neighbour kept
    print("%s N=%d E=%d: queries %d, linear programme 3 %d, two or more later lines %d, collision-branch lines %d (pairs inside "
          "1.05 x radii: %d), envs with an exact tie %d, parallel pairs in linear programme 1 %d (rejecting: %d), in 3: %d" % (
              cls, N, E, lg["queries"], lg["lp3"], lg["multi"], lg["collision_lines"], band, int(ties.sum()),
              lg["lp1_parallel"], lg["lp1_parallel_reject"], lg["lp3_parallel"]))
    assert lg["queries"] == int(present.sum())
    same = (d2 == 0) & (vel[:, :, None, :] == vel[:, None, :, :]).all(-1)
    assert not same.any(), "identical position and velocity"
    if cls in "adfg":
        assert lg["lp3"] >= 30 and (lg["multi"] >= 10 or N <= 3), lg
    if cls == "b":
        assert lg["collision_lines"] >= 30 and lg["collision_lines"] == band, lg
        # strictly inside the band: the chained partners do not collide for the env (float64 distance > r_a + r_b) ...
        x, y, r = sc.pos_x, sc.pos_y, sc.radius
        i = np.array([k for k in range(N) if k % 3])
        d = np.hypot(x[:, i] - x[:, i - 1], y[:, i] - y[:, i - 1])
        assert (d > r[:, i] + r[:, i - 1]).all() and (d < 1.05 * (r[:, i] + r[:, i - 1])).all()
        # ... and rvo2 sees them overlapping (float32 distSq <= float32 combinedRadiusSq)
        assert (d2[:, i, i - 1] <= (R * R)[:, i, i - 1]).all()
    if cls == "c":
        for n in S.Scene.FIELDS:
            a = getattr(sc, n)
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), n + " is not exact in float32"
        assert sc.params["rvo_max_neighbors"] < max(N - 1, 2)
        if N >= 3:
            assert ties.all(), "envs without an exact distSq tie: %s" % np.nonzero(~ties)[0]
        if N >= 4:
            assert lg["lp1_parallel_reject"] >= 1 and lg["lp3_parallel"] >= 1, lg
    if cls == "d":
        assert not (sc.vel_x.any() or sc.vel_y.any())
        if N >= 4:      # the boxed-in agent itself, three band neighbours around it: infeasible in every env
            assert (lg["log"].reshape(E, N)[:, 0] >= 0).all()
        # inside the band, bodies apart: nearly everybody is still live on the later steps
        x, y, r = sc.pos_x, sc.pos_y, sc.radius
        dd = np.hypot(x[:, :, None] - x[:, None, :], y[:, :, None] - y[:, None, :]) + 1e9 * np.eye(N)
        assert (dd > r[:, :, None] + r[:, None, :]).all()
        assert (o.s["flags"] & orc.IN_COLLISION).mean() < 0.05
    if cls == "e":
        h2 = np.float32(S.HORIZON) * np.float32(S.HORIZON)
        fin = np.isfinite(d2)
        assert (d2[fin] < h2).sum() >= 30 and (d2[fin] >= h2).sum() >= 30
        want = sorted(np.float32(v) * np.float32(v) for v in S.horizon_offsets())    # one ulp inside, at, one ulp outside
        assert want[0] < h2 == want[1] < want[2]
        marked = d2[:, 0, 1:min(N, 4)]
        for w in want:
            assert (marked == w).any(), "no marked neighbour at distSq %r" % w
        assert np.isin(marked, want).all()


@pytest.mark.parametrize("cls", "abdf")
def test_oracle_matches_the_brute_force_on_the_scenes(cls):
    """the oracle's velocities on classes a, b, d, f at N <= 10 against the float64 brute force, exactly as
    tests/test_orca_semantics.py::_check_env does (its TOL, its ambiguous and borderline exclusions); every other env is
    sampled (the brute force enumerates pairs and triples of lines serially), and at most a quarter of the queries of a class
    may be ambiguous or borderline.  The class seeds of orca_scenes.SEEDS were chosen for this test: with others (most class a
    seeds, class b seeds 0 .. 3) a query in a thousand holds two violated lines anti-parallel to within ~0.02 degrees some m/s from the
    origin, where linear programme 3 as published loses the optimum in float32
    (test_the_float32_limit_the_seeds_stay_clear_of keeps one such query on record).  Packing the agents tighter than class a
    does makes that the rule rather than the exception: no seed of forty passed then"""
    stats = dict(feasible=0, infeasible=0, borderline=0, ambiguous=0)
    for N, E in S.SHAPES:
        if N > 10:
            continue
        sc = S.build(cls, N, E)
        o = _oracle(sc)
        pos, vel, pref, radius, vmax = _orca_inputs_from_state(o)
        o.step()
        for e in range(0, E, 2):
            _check_env(pos[e].astype(float), vel[e].astype(float), pref[e].astype(float), radius[e].astype(float),
                       vmax[e].astype(float), o.orca_vel[e], stats)
    total = sum(stats.values())
    print("class %s: %d queries against the brute force: %s; ambiguous + borderline share %.3f" % (
        cls, total, stats, (stats["ambiguous"] + stats["borderline"]) / float(total)))
    assert total >= 400 and stats["infeasible"] >= 100, stats
    assert stats["ambiguous"] + stats["borderline"] <= 0.25 * total, stats


def test_the_float32_limit_the_seeds_stay_clear_of():
    """one query of a seed that was NOT chosen (class b, seed 1, N = 9, env 13, agent 2), kept so that the limit is on record and
    its cause pinned: the oracle misses the min-max penetration by far more than TOL there, and the query does hold two violated
    lines that are anti-parallel to within 1e-3 rad -- their intersection, which linear programme 3 projects on, lies more than
    1e3 m/s out, where the float32 discriminant of the 1-D programme cancels.  This is the
    algorithm as published (oracle/orca_ref.h restates it line by line), not a slip of the restatement."""
    keep = S.SEEDS["b"]
    S.SEEDS["b"] = 1
    try:
        sc = S.build("b", 9, GPU_ENVS[9])
    finally:
        S.SEEDS["b"] = keep
    e, a = 13, 2
    o = _oracle(sc)
    pos, vel, pref, radius, vmax = [x[e].astype(float) for x in _orca_inputs_from_state(o)]
    o.step()
    v = o.orca_vel[e, a].astype(float)
    lines = [bf.half_plane(pos[a], vel[a], radius[a], pos[b], vel[b], radius[b], 5.0, 0.1) for b in range(9) if b != a]
    assert min(m for _, _, m in lines) > 1e-6                       # (not an ambiguous construction)
    pts, nrm = np.array([p for p, _, _ in lines]), np.array([n for _, n, _ in lines])
    sol = bf.solve(pts, nrm, pref[a], vmax[a])
    pen = bf.penetration(pts, nrm, v)
    print("min-max penetration %.4f, the oracle's %.4f, speed %.4f of %.4f" % (sol["minmax"], pen.max(), np.hypot(*v), vmax[a]))
    assert sol["minmax"] > TOL and pen.max() - sol["minmax"] > 100 * TOL
    viol = np.nonzero(pen > 0)[0]
    sines = [(abs(nrm[i, 0] * nrm[j, 1] - nrm[i, 1] * nrm[j, 0]), i, j) for i in viol for j in viol if i < j and nrm[i] @ nrm[j] < 0]
    sine, i, j = min(sines)
    cut = np.linalg.solve(np.array([nrm[i], nrm[j]]), np.array([nrm[i] @ pts[i], nrm[j] @ pts[j]]))   # where the two lines meet
    assert sine < 1e-3 and np.hypot(*cut) > 1e3, (sine, cut)


def _velocities(sc, tie_reverse=False, collab="scene", **override):
    o = _oracle(sc, **override)
    if collab != "scene":
        o.set_rvo_stochastic(collab=collab)
    orc.set_tie_order(tie_reverse)
    try:
        o.step()
    finally:
        orc.set_tie_order(False)
    return o.orca_vel.copy().view(np.uint32)


# the wrong variant of each class: (what it is, scene -> velocity words of the variant)
def _far_to_near(sc):
    near = S.build("a", sc.N, sc.E)      # class f without its translation: positions not quantised to 2 mm
    return _velocities(near)


VARIANTS = {
    "a": ("time horizon 4.9 s instead of 5 s", lambda sc: _velocities(sc, rvo_time_horizon=4.9)),
    "b": ("collision branch with a time step of 0.11 s instead of 0.1 s", lambda sc: _velocities(sc, rvo_dt=0.11)),
    "c": ("tied neighbours visited in reverse order", lambda sc: _velocities(sc, tie_reverse=True)),
    "d": ("collision branch with a time step of 0.11 s instead of 0.1 s", lambda sc: _velocities(sc, rvo_dt=0.11)),
    "e": ("max_neighbors larger by one (the one-neighbour run), and a horizon one float32 ulp further out", None),
    "f": ("positions before the translation (not quantised to 2 mm)", _far_to_near),
    "g": ("absent slots taken for agents (ragged = 0)", lambda sc: _velocities(sc, ragged=0)),
    "h": ("collaboration 0.5 for everybody instead of the per-agent array", lambda sc: _velocities(sc, collab=None)),
}


@pytest.mark.parametrize("cls", S.CLASSES)
def test_each_class_tells_the_oracle_from_a_wrong_variant(cls):
    """a class on which a wrong ORCA gives the same bits could not fail on the GPU either: every class must change at least
    one velocity word under its variant, at every agent count where the variant can matter"""
    what, fn = VARIANTS[cls]
    for N, E in S.SHAPES:
        sc = S.build(cls, N, E)
        if cls == "e":
            one = S.build("e", N, E, max_neighbors=1)
            base1 = _velocities(one)
            changed = int((base1 != _velocities(one, rvo_max_neighbors=2)).sum())
            further = float(np.nextafter(np.float32(S.HORIZON), np.float32(np.inf)))
            changed_h = int((_velocities(sc) != _velocities(sc, sensing_horizon=further)).sum())
            print("class e N=%d: %d words change with max_neighbors 1 -> 2, %d with the horizon one ulp further out" % (
                N, changed, changed_h))
            assert changed_h >= 1                       # the neighbour standing exactly at the horizon comes in
            # (N <= 4: agent 0 and the marked agents are all there is, at most one of them in range: the GPU test leaves the
            # one-neighbour run out there)
            assert changed >= 1 or N <= 4
            continue
        changed = int((_velocities(sc) != fn(sc)).sum())
        print("class %s N=%d: %d of %d velocity words change under: %s" % (cls, N, changed, 2 * E * N, what))
        if cls == "c" and N <= 3:
            # rvo_max_neighbors = 1: a neighbour tied with the one kept is never inserted, in either order.  These scenes are
            # there for the head-on pairs (the det(relativePosition, w) > 0 tie of the leg choice): their one line must bind
            changed = int((_velocities(sc) != _velocities(sc, rvo_time_horizon=4.9)).sum())
            print("class c N=%d: %d velocity words change with a time horizon of 4.9 s" % (N, changed))
        assert changed >= 1, (cls, N, what)
