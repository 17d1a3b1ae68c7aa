#!/usr/bin/env python3
"""oracle/gen_step_rule_golden.py -- TEST INFRASTRUCTURE.  Runs the UNMODIFIED reference on the threshold scenes of
tests/step_rule_scenes.py and records what it says into tests/golden/step_rules.npz: the judge of
tests/test_step_rule_scenes_host.py::test_oracle_equals_the_reference_on_recorded_scenes.

Like oracle/gen_golden.py it works only where the reference is, uses the same stubs and the Config mechanism of
oracle/golden_configs.py (class StepRule, fed through STEP_RULE_CONFIG), and runs every (class, variant, agent count) in its
own subprocess, the Config object being an import-time singleton.  A scene's env becomes the reference's own Agents
(ExternalPolicy / LearningPolicy, UnicycleDynamics, OtherAgentsStatesSensor) at the scene's state -- an absent slot of a ragged
env is simply no agent -- the remaining time is assigned after reset(), the env steps three times on the scene's external actions,
and after every step state, flags, rewards, done, game over and observations (with num_other_agents_observed) are recorded.
The file holds recorded results only; it must stay below 200 KB.

Usage:  python oracle/gen_step_rule_golden.py
        python oracle/gen_step_rule_golden.py --worker CLASS VARIANT N OUT   # (internal)"""
import io
import json
import os
import subprocess
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
REF = os.environ.get("CA_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "step_rules.npz")
AGENT_COUNTS = (2, 4, 6, 10, 20)
ENVS = 3
STEPS = 3
LIMIT = 200 * 1000


def config_of(sc):
    from tests import step_rule_scenes as R
    c = {k: v for k, v in sc.params.items() if k not in ("sort_mode", "game_over_mode", "ragged")}
    c.update(n=sc.N, max_obs=sc.max_obs, sort=("closest_first", "closest_last", "time_to_impact")[sc.params.get("sort_mode", 0)],
             over=R.OVERS[sc.params.get("game_over_mode", 0)], use_map=sc.static_map is not None)
    return c


def worker(cls, variant, N, out):
    from tests import step_rule_scenes as R
    sc = R.build(cls, N, ENVS, variant)
    os.environ["GYM_CONFIG_PATH"] = os.path.join(HERE, "golden_configs.py")
    os.environ["GYM_CONFIG_CLASS"] = "StepRule"
    os.environ["STEP_RULE_CONFIG"] = json.dumps(config_of(sc))
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path[:0] = [os.path.join(HERE, "stubs"), os.path.join(HERE, "_build"), REF]
    import warnings
    warnings.filterwarnings("ignore")
    from gen_golden import _obs_array, _snapshot
    from gym_collision_avoidance.envs import Config
    from gym_collision_avoidance.envs import test_cases as tc
    from gym_collision_avoidance.envs.Map import Map
    from gym_collision_avoidance.envs.agent import Agent
    from gym_collision_avoidance.envs.collision_avoidance_env import CollisionAvoidanceEnv
    from gym_collision_avoidance.envs.dynamics.UnicycleDynamics import UnicycleDynamics
    from gym_collision_avoidance.envs.sensors.OtherAgentsStatesSensor import OtherAgentsStatesSensor

    class EnvWithWalls(CollisionAvoidanceEnv):       # the scene's map instead of an image file (Map.py:13: rows come from
        def _init_static_map(self):                  # x_width, columns from y_width)
            self.map = Map(R.MAP_ROWS * R.MAP_CELL, R.MAP_COLS * R.MAP_CELL, R.MAP_CELL, None)
            assert self.map.static_map.shape == sc.static_map.shape
            self.map.static_map = sc.static_map.copy()

    env = EnvWithWalls() if sc.static_map is not None else CollisionAvoidanceEnv()
    f = np.float64
    K = sc.max_obs
    rec = dict(state=np.zeros((STEPS, ENVS, N, 15)), flags=np.zeros((STEPS, ENVS, N), np.uint32),
               obs=np.zeros((STEPS, ENVS, N, 6 + 7 * K)), rewards=np.full((STEPS, ENVS, N), np.nan),
               done=np.zeros((STEPS, ENVS, N), np.uint8), game_over=np.zeros((STEPS, ENVS), np.uint8))
    for e in range(ENVS):
        P = [i for i in range(N) if not (sc.flags[e, i] & R.ABSENT)]
        assert P == list(range(len(P)))
        agents = [Agent(f(sc.pos_x[e, i]), f(sc.pos_y[e, i]), f(sc.goal_x[e, i]), f(sc.goal_y[e, i]), f(sc.radius[e, i]),
                        f(sc.pref_speed[e, i]), f(sc.heading[e, i]),
                        tc.policy_dict["learning" if sc.policy[e, i] == R.POL_LEARNING else "external"], UnicycleDynamics,
                        [OtherAgentsStatesSensor], i) for i in P]
        env.set_agents(agents)
        env.reset()
        for i, a in enumerate(env.agents):
            a.set_state(f(sc.pos_x[e, i]), f(sc.pos_y[e, i]), f(0.0), f(0.0), f(sc.heading[e, i]))
            a.time_remaining_to_reach_goal = f(sc.time_remaining[e, i])
        actions = {i: np.array(sc.ext[e, i]) for i in P}
        for t in range(STEPS):
            obs, rew, over, _, info = env.step(actions)
            st, fl = _snapshot(env.agents)
            n = len(P)
            rec["state"][t, e, :n], rec["flags"][t, e, :n] = st, fl
            rec["obs"][t, e, :n] = _obs_array(obs, env.agents, Config.STATES_IN_OBS)
            rew = np.asarray(rew, np.float64)
            if rew.ndim == 0:                         # TRAIN_SINGLE_AGENT: the reference hands back agent 0's reward only
                rec["rewards"][t, e, 0] = rew
            else:
                rec["rewards"][t, e, :n] = rew
            rec["done"][t, e, :n] = [info["which_agents_done"][a.id] for a in env.agents]
            rec["game_over"][t, e] = bool(over)
    np.savez(out, **rec)


def save(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same file, byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, a in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zf.writestr(info, buf.getvalue())


def load(path=OUT):
    """-> {case name: {quantity: array [step, env, ...]}} as worker() recorded them (observations: float32)"""
    from tests import step_rule_scenes as R
    with np.load(path) as z:
        flat = {k: z[k] for k in z.files}
    at = {k: 0 for k in flat}
    out = {}
    for name in flat["cases"]:
        cls, variant, N = str(name).split("_")
        N = int(N)
        W = 6 + 7 * R.build(cls, N, ENVS, "" if variant == "-" else variant).max_obs
        shapes = dict(state=(ENVS, N, STEPS, 15), flags=(ENVS, N, STEPS), obs=(ENVS, N, STEPS, W), rewards=(ENVS, N, STEPS),
                      done=(ENVS, N, STEPS), game_over=(ENVS, STEPS))
        case = {}
        for k, shape in shapes.items():
            n = int(np.prod(shape))
            a = flat[k][at[k]:at[k] + n].reshape(shape)
            at[k] += n
            case[k] = np.moveaxis(a, 2, 0) if len(shape) >= 3 else a.T
        out[str(name)] = case
    assert all(at[k] == flat[k].size for k in at if k != "cases")
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
        return
    from tests import step_rule_scenes as R
    subprocess.check_call(["make", "-C", HERE, "-s"])
    parts, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for cls in R.CLASSES:
            for variant in R.VARIANTS[cls]:
                for N in AGENT_COUNTS:
                    part = os.path.join(tmp, "part.npz")
                    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", cls, variant, str(N), part])
                    cases.append("%s_%s_%d" % (cls, variant or "-", N))
                    with np.load(part) as z:
                        for k in z.files:
                            parts.setdefault(k, []).append(z[k])
    # What keeps the file small: one member per quantity, the cases laid end to end in the order of `cases` (load() below cuts
    # them apart again: every shape follows from the scene); observations as float32, the precision the kernels hand them out in
    # (every radius of the scenes stays distinct in float32, so who sits in a slot is still exact); and, nothing moving, the
    # three steps of an agent's row side by side ([env, agent, step, ...]), where zlib finds the repeats.
    out = {"cases": np.array(cases)}
    for k, arrays in parts.items():
        flat = [np.ascontiguousarray(np.moveaxis(a, 0, 2) if a.ndim >= 3 else a.T).reshape(-1) for a in arrays]
        out[k] = np.concatenate(flat).astype(np.float32 if k == "obs" else flat[0].dtype)
    save(OUT, out)
    size = os.path.getsize(OUT)
    print("step rules ok: %d members, %d bytes" % (len(out), size))
    assert size < LIMIT, "tests/golden/step_rules.npz is %d bytes: above the %d of the other goldens of this kind" % (size, LIMIT)


if __name__ == "__main__":
    main()
