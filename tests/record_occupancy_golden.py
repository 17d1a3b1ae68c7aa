#!/usr/bin/env python3
"""tests/record_occupancy_golden.py -- RECORDER, not a test (no test imports it).  Runs the UNMODIFIED reference's
OccupancyGridSensor (envs/sensors/OccupancyGridSensor.py) on the reference's own Map and writes
tests/golden/occgrid.npz.  It works only where the reference checkout is present (CA_REFERENCE_ROOT, default
/root/reference) and after `build()` has made oracle/_build/rvo2*.so; its output is committed.

How the reference is made to run (nothing of it is modified or copied): oracle/stubs (gym / imageio / tensorflow
stand-ins) and the reference are put on sys.path, the Config singleton is selected through GYM_CONFIG_PATH /
GYM_CONFIG_CLASS (oracle/golden_configs.py Laser4: USE_STATIC_MAP), and the one name the reference's sensor module uses
without importing it -- `Config` -- is set on that module from outside.  The sensor sets no `name`, so Agent.sense cannot
store its result: `sense()` is called here directly, on `env.map`, after reset / step have returned (by then the
reference's _get_obs has redrawn the agents at their post-move positions, collision_avoidance_env.py:563-569).

Recorded:
  (a) ep_*: one episode of four RVO agents on a map with walls near their paths; starts / goals are drawn uniformly with
      a seed (off-lattice: at multiples of 0.1 m the reference's sensor raises), one agent travels along y ~ 6.5 m, within
      2.5 m of the map's border, so partial windows occur;
  (b) sc_*: single-shot scenes, 6 agents each at uniform positions in [-11, 11]^2 (windows fully inside, partly outside and
      wholly outside the map) with radii in [0.2, 0.8], on one of a few static grids (wall bands + ~1 % random cells).
  (c) lat_*: 40 lattice positions (multiples of 0.1 / 0.05 / 0.25 m as np.arange produces them, i.e. up to a few ulp off the
      decimal value, and the same rounded to the decimal value): (-10.4, 2.8) first, then 39 at which the reference
      RAISES, each verified here by calling it (one agent of radius 0.5 on an empty map) -- the positions at which the tests
      pin the anchoring rule instead; lat_valid says what the reference did, lat_windows holds what it returned.
Per row: px, py, radius of every agent, the window (bit-packed) and `valid` (0: the reference raised -- its two corners
spanned 49 or 51 cells).  At most 2 % of the rows may be invalid (asserted here and again by the test)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("CA_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(HERE, "golden", "occgrid.npz")
N_SCENES, N_SCENE_AGENTS, N_GRIDS, MAX_STEPS, N_LATTICE = 150, 6, 5, 80, 40


def scene_grids(rng):
    grids = np.zeros((N_GRIDS, 160, 160), dtype=bool)
    for g in grids:
        for _ in range(3):                      # a few wall bands, horizontal or vertical
            r0, c0 = rng.integers(0, 150, size=2)
            ln, th = int(rng.integers(20, 70)), int(rng.integers(2, 6))
            if rng.random() < 0.5:
                g[r0:r0 + th, c0:c0 + ln] = True
            else:
                g[r0:r0 + ln, c0:c0 + th] = True
        g |= rng.random(g.shape) < 0.01          # ~1 % random cells
    grids[0, 0, :] = grids[0, -1, :] = grids[0, :, 0] = grids[0, :, -1] = True   # the map's outermost cells
    return grids


def main():
    os.environ["GYM_CONFIG_PATH"] = os.path.join(REPO, "oracle", "golden_configs.py")
    os.environ["GYM_CONFIG_CLASS"] = "Laser4"
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path[:0] = [os.path.join(REPO, "oracle", "stubs"), os.path.join(REPO, "oracle", "_build"), REF]
    import warnings
    warnings.filterwarnings("ignore")
    import rvo2  # noqa: F401  (the oracle's module; fail early if build() has not made it)
    from gym_collision_avoidance.envs import Config
    from gym_collision_avoidance.envs import test_cases as tc
    from gym_collision_avoidance.envs.agent import Agent
    from gym_collision_avoidance.envs.collision_avoidance_env import CollisionAvoidanceEnv
    from gym_collision_avoidance.envs.dynamics.UnicycleDynamics import UnicycleDynamics
    from gym_collision_avoidance.envs.Map import Map
    from gym_collision_avoidance.envs.sensors.LaserScanSensor import LaserScanSensor
    from gym_collision_avoidance.envs.sensors.OtherAgentsStatesSensor import OtherAgentsStatesSensor
    from gym_collision_avoidance.envs.sensors import OccupancyGridSensor as ogs_module
    ogs_module.Config = Config          # the name the reference's module reads without importing it
    sensor = ogs_module.OccupancyGridSensor()

    def sense_all(agents, top_down_map):
        """-> windows bool [N, 50, 50], valid uint8 [N]"""
        wins, valid = [], []
        devnull = open(os.devnull, "w")
        for i in range(len(agents)):
            stdout, sys.stdout = sys.stdout, devnull   # (the reference prints when a window misses the map)
            try:
                w = np.asarray(sensor.sense(agents, i, top_down_map), dtype=bool)
                ok = 1
            except ValueError:
                w, ok = np.zeros((50, 50), dtype=bool), 0
            finally:
                sys.stdout = stdout
            assert w.shape == (50, 50), w.shape
            wins.append(w)
            valid.append(ok)
        return np.array(wins), np.array(valid, dtype=np.uint8)

    out = {}
    # ---------------------------------------------------------------- (a) the episode
    static = np.zeros((160, 160), dtype=bool)   # row = floor(80 - y / 0.1), col = floor(80 + x / 0.1)
    static[40:45, 60:110] = True                # a wall at y ~ 3.8 m, north of the crossing
    static[96:101, 30:75] = True                # a wall at y ~ -1.8 m, south-west
    static[60:100, 118:122] = True              # a pillar at x ~ 4 m
    static[4:8, 20:140] = True                  # a long wall at y ~ 7.4 m, beside the northern agent's path
    static[:, 0:2] = True                       # the western border

    class EnvWithObstacles(CollisionAvoidanceEnv):   # (the reference loads maps from image files through imageio /
        def _init_static_map(self):                  # scipy.misc.imresize, both absent here: inject the array)
            CollisionAvoidanceEnv._init_static_map(self)
            self.map.static_map = static.copy()

    rng = np.random.Generator(np.random.PCG64(20241016))
    f = np.float64

    def mk(px, py, gx, gy, r, ps, i):
        h = np.arctan2(f(gy) - f(py), f(gx) - f(px))
        return Agent(f(px), f(py), f(gx), f(gy), f(r), f(ps), h, tc.policy_dict["RVO"], UnicycleDynamics,
                     [OtherAgentsStatesSensor, LaserScanSensor], i)

    u = lambda lo, hi: float(rng.uniform(lo, hi))
    agents = [mk(u(-4.5, -3.5), u(-0.5, 0.5), u(3.0, 3.6), u(0.5, 1.5), u(0.3, 0.5), u(0.9, 1.2), 0),
              mk(u(3.0, 3.6), u(0.5, 1.5), u(-4.5, -3.5), u(-0.5, 0.5), u(0.3, 0.5), u(0.9, 1.2), 1),
              mk(u(-7.4, -6.6), u(6.2, 6.6), u(6.6, 7.4), u(6.2, 6.6), u(0.3, 0.5), u(1.3, 1.6), 2),   # near the border
              mk(u(-1.0, 1.0), u(-6.5, -5.8), u(-1.0, 1.0), u(2.0, 3.0), u(0.5, 0.8), u(0.9, 1.2), 3)]
    env = EnvWithObstacles()
    env.set_agents(agents)
    env.reset()
    state, wins, valid = [], [], []

    def record():
        state.append([[a.pos_global_frame[0], a.pos_global_frame[1], a.radius] for a in env.agents])
        w, v = sense_all(env.agents, env.map)
        wins.append(w)
        valid.append(v)

    record()
    for _ in range(MAX_STEPS):
        _, _, over, _, _ = env.step({})
        record()
        if over:
            break
    ep_state = np.array(state, dtype=np.float64)          # [T, 4, 3] = px, py, radius
    assert (np.abs(ep_state[:, :, :2]) > 5.5).any(), "no agent came within 2.5 m of the map's border"
    out["ep_static"] = np.packbits(static, axis=-1, bitorder="little")
    out["ep_state"] = ep_state
    out["ep_windows"] = np.packbits(np.array(wins), axis=-1, bitorder="little")   # [T, 4, 50, 7]
    out["ep_valid"] = np.array(valid)

    # ---------------------------------------------------------------- (b) single-shot scenes
    class Disc(object):   # what Map.add_agents_to_map and the sensor read of an agent
        def __init__(self, px, py, radius):
            self.pos_global_frame = np.array([px, py], dtype=np.float64)
            self.radius = radius

    grids = scene_grids(rng)
    sc_state = np.empty((N_SCENES, N_SCENE_AGENTS, 3), dtype=np.float64)
    sc_state[:, :, :2] = rng.uniform(-11.0, 11.0, size=(N_SCENES, N_SCENE_AGENTS, 2))
    sc_state[:, :, 2] = rng.uniform(0.2, 0.8, size=(N_SCENES, N_SCENE_AGENTS))
    wins, valid = [], []
    for s in range(N_SCENES):
        m = Map(16, 16, 0.1)
        m.static_map = grids[s % N_GRIDS].copy()
        discs = [Disc(*row) for row in sc_state[s]]
        m.add_agents_to_map(discs)
        w, v = sense_all(discs, m)
        wins.append(w)
        valid.append(v)
    out["sc_grids"] = np.packbits(grids, axis=-1, bitorder="little")
    out["sc_state"] = sc_state
    out["sc_windows"] = np.packbits(np.array(wins), axis=-1, bitorder="little")
    out["sc_valid"] = np.array(valid)

    # ---------------------------------------------------------------- (c) lattice positions at which the reference raises
    cands = [(-10.4, 2.8)]
    for step in (0.1, 0.05, 0.25):
        # the lattice as a user's np.arange produces it (-11 + k * step: "round" values up to a few ulp), and rounded
        raw = np.arange(-11.0, 11.0 + step / 2, step)
        for ticks in (raw, np.round(raw, 2)):
            pick = rng.integers(0, len(ticks), size=(300, 2))
            cands += [(float(ticks[i]), float(ticks[j])) for i, j in pick]
    def lone(px, py):
        m = Map(16, 16, 0.1)
        discs = [Disc(px, py, 0.5)]
        m.add_agents_to_map(discs)
        w, v = sense_all(discs, m)
        return w[0], int(v[0])

    raising = [c for c in cands[1:] if not lone(*c)[1]]
    print("lattice: the reference raised at %d of %d candidate positions, e.g. %s; at (-10.4, 2.8) it %s"
          % (len(raising), len(cands) - 1, raising[:4], "returned a window" if lone(-10.4, 2.8)[1] else "raised"))
    # on this lattice the raising positions form lines (one coordinate decides): walk along them
    lines_x = sorted({c[0] for c in raising if not lone(c[0], 0.013)[1]})
    lines_y = sorted({c[1] for c in raising if not lone(0.013, c[1])[1]})
    print("         raising whatever y at x in %s, whatever x at y in %s" % (lines_x, lines_y))
    assert lines_x and lines_y
    along = [float(v) for v in np.round(np.arange(-7.5, 7.6, 0.5), 2)]
    more = [(x, along[(3 * k) % len(along)]) for k, x in enumerate(lines_x * 10)] + \
           [(along[(5 * k + 1) % len(along)], y) for k, y in enumerate(lines_y * 10)]
    more = [c for c in more if not lone(*c)[1]]
    lat = [cands[0]] + list(dict.fromkeys(more + raising))[:N_LATTICE - 1]
    assert len(lat) == N_LATTICE
    out["lat_xy"] = np.array(lat, dtype=np.float64)
    res = [lone(*c) for c in lat]
    out["lat_windows"] = np.packbits(np.array([r[0] for r in res]), axis=-1, bitorder="little")
    out["lat_valid"] = np.array([r[1] for r in res], dtype=np.uint8)   # 0: the reference raised there
    assert not out["lat_valid"][1:].any()

    n_rows = out["ep_valid"].size + out["sc_valid"].size
    n_bad = n_rows - int(out["ep_valid"].sum()) - int(out["sc_valid"].sum())
    assert n_bad <= 0.02 * n_rows, "%d of %d recorded rows are invalid (cap: 2 %%)" % (n_bad, n_rows)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("%s: %d episode steps x 4 agents, %d scenes x %d agents, %d of %d rows invalid, %d bytes"
          % (OUT, len(ep_state), N_SCENES, N_SCENE_AGENTS, n_bad, n_rows, os.path.getsize(OUT)))
    print("windows with an occupied cell: episode %d, scenes %d; partial / empty windows among the scenes: %d"
          % (int(np.array(out["ep_windows"]).reshape(-1, 350).any(axis=1).sum()),
             int(np.array(out["sc_windows"]).reshape(-1, 350).any(axis=1).sum()),
             int((np.abs(sc_state[:, :, :2]) > 5.5).any(axis=2).sum())))


if __name__ == "__main__":
    main()
