#!/usr/bin/env python3
"""oracle/gen_move_golden.py -- TEST INFRASTRUCTURE.  Runs the UNMODIFIED reference on the angle-edge scenes of
tests/move_scenes.py and records what it says into tests/golden/move_rules.npz: the judge of
tests/test_move_scenes_host.py::test_oracle_equals_the_reference_on_recorded_scenes.

Modelled on oracle/gen_step_rule_golden.py: it works only where the reference is, uses the same stubs and the Config class
StepRule of oracle/golden_configs.py (fed through STEP_RULE_CONFIG, with the scene's dt), and runs every (class, variant, agent
count) in its own subprocess.  Recorded: classes h, d, m, a (external and learning -- the index policies need the network's
framework), n at N = 2 .. 6, 4 envs: the 80 agents of a (class, variant) take the cases 0 .. 79 of its list once each.  A scene's
env becomes the reference's own Agents (ExternalPolicy / LearningPolicy / NonCooperativePolicy / StaticPolicy, UnicycleDynamics /
UnicycleDynamicsMaxTurnRate, OtherAgentsStatesSensor) at the scene's state, turning_dir included; the env steps twice on the
scene's external actions and after every step position, velocity, heading, goal, turning_dir, remaining time, clock, the float32
action, flags and the observation are recorded.  The file holds recorded results only; it must stay below the size of
tests/golden/step_rules.npz.

Usage:  python oracle/gen_move_golden.py
        python oracle/gen_move_golden.py --worker CLASS VARIANT N OUT   # (internal)"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
REF = os.environ.get("CA_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(REPO, "tests", "golden", "move_rules.npz")
AGENT_COUNTS = (2, 3, 4, 5, 6)
ENVS = 4
STEPS = 2
RECORDED = (("h", "unicycle"), ("h", "maxturn"), ("d", ""), ("m", "pow2"), ("m", "default"), ("a", "external"), ("a", "learning"),
            ("n", ""))
STATE = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "time_remaining", "t", "turning_dir")


def worker(cls, variant, N, out):
    from tests import move_scenes as M
    sc = M.build(cls, N, ENVS, variant)
    os.environ["GYM_CONFIG_PATH"] = os.path.join(HERE, "golden_configs.py")
    os.environ["GYM_CONFIG_CLASS"] = "StepRule"
    os.environ["STEP_RULE_CONFIG"] = json.dumps(dict(n=N, max_obs=sc.max_obs, sort="closest_first", over="all", dt=sc.dt,
                                                     **sc.params))
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.path[:0] = [os.path.join(HERE, "stubs"), os.path.join(HERE, "_build"), REF]
    import warnings
    warnings.filterwarnings("ignore")
    from gen_golden import _obs_array, _snapshot
    from gym_collision_avoidance.envs import Config
    from gym_collision_avoidance.envs import test_cases as tc
    from gym_collision_avoidance.envs.agent import Agent
    from gym_collision_avoidance.envs.collision_avoidance_env import CollisionAvoidanceEnv
    from gym_collision_avoidance.envs.dynamics.UnicycleDynamics import UnicycleDynamics
    from gym_collision_avoidance.envs.dynamics.UnicycleDynamicsMaxTurnRate import UnicycleDynamicsMaxTurnRate
    from gym_collision_avoidance.envs.sensors.OtherAgentsStatesSensor import OtherAgentsStatesSensor

    assert Config.DT == sc.dt
    policy = {M.POL_NONCOOP: "noncoop", M.POL_STATIC: "static", M.POL_EXTERNAL: "external", M.POL_LEARNING: "learning"}
    dynamics = {M.DYN_UNICYCLE: UnicycleDynamics, M.DYN_MAX_TURN_RATE: UnicycleDynamicsMaxTurnRate}
    env = CollisionAvoidanceEnv()
    f = np.float64
    W = 6 + 7 * sc.max_obs
    rec = dict(state=np.zeros((STEPS, ENVS, N, len(STATE))), action=np.zeros((STEPS, ENVS, N, 2), np.float32),
               flags=np.zeros((STEPS, ENVS, N), np.uint32), obs=np.zeros((STEPS, ENVS, N, W), np.float32))
    for e in range(ENVS):
        agents = [Agent(f(sc.pos_x[e, i]), f(sc.pos_y[e, i]), f(sc.goal_x[e, i]), f(sc.goal_y[e, i]), f(sc.radius[e, i]),
                        f(sc.pref_speed[e, i]), f(sc.heading[e, i]), tc.policy_dict[policy[int(sc.policy[e, i])]],
                        dynamics[int(sc.dynamics[e, i])], [OtherAgentsStatesSensor], i) for i in range(N)]
        env.set_agents(agents)
        env.reset()
        for i, a in enumerate(env.agents):
            a.set_state(f(sc.pos_x[e, i]), f(sc.pos_y[e, i]), f(0.0), f(0.0), f(sc.heading[e, i]))
            a.goal_global_frame = np.array([sc.goal_x[e, i], sc.goal_y[e, i]])      # (bit for bit: a goal of -0.0 stays -0.0)
            a.time_remaining_to_reach_goal = f(60.0)
            a.turning_dir = f(sc.turning_dir[e, i])
        actions = {i: np.array(sc.ext[e, i]) for i in range(N)}
        for t in range(STEPS):
            obs, rew, over, _, info = env.step(actions)
            st, fl = _snapshot(env.agents)      # oracle/gen_golden.py: columns 0 .. 6 = position, velocity, heading, goal; 9, 10 =
            rec["state"][t, e, :, :7] = st[:, :7]                                      # remaining time, clock; 12, 13 = the action
            rec["state"][t, e, :, 7:9] = st[:, 9:11]
            rec["state"][t, e, :, 9] = [a.turning_dir for a in env.agents]
            rec["action"][t, e] = np.array([a.past_actions[0] for a in env.agents]).astype(np.float32)
            assert np.array_equal(rec["action"][t, e].astype(np.float64), st[:, 12:14])      # (the reference stores float32 actions)
            rec["flags"][t, e] = fl
            rec["obs"][t, e] = _obs_array(obs, env.agents, Config.STATES_IN_OBS)
    np.savez(out, **rec)


def load(path=OUT):
    """-> {case name: {quantity: array [step, env, agent, ...]}} as worker() recorded them (observations: float32)"""
    with np.load(path) as z:
        flat = {k: z[k] for k in z.files}
    at = {k: 0 for k in flat}
    out = {}
    for name in flat["cases"]:
        cls, variant, N = str(name).split("_")
        N = int(N)
        shapes = dict(state=(STEPS, ENVS, N, len(STATE)), action=(STEPS, ENVS, N, 2), flags=(STEPS, ENVS, N),
                      obs=(STEPS, ENVS, N, 6 + 7 * (N - 1)))
        case = {}
        for k, shape in shapes.items():
            n = int(np.prod(shape))
            case[k] = flat[k][at[k]:at[k] + n].reshape(shape)
            at[k] += n
        out[str(name)] = case
    assert all(at[k] == flat[k].size for k in at if k != "cases")
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5])
        return
    from oracle.gen_step_rule_golden import save
    subprocess.check_call(["make", "-C", HERE, "-s"])
    parts, cases = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for cls, variant in RECORDED:
            for N in AGENT_COUNTS:
                part = os.path.join(tmp, "part.npz")
                subprocess.check_call([sys.executable, os.path.abspath(__file__), "--worker", cls, variant, str(N), part])
                cases.append("%s_%s_%d" % (cls, variant or "-", N))
                with np.load(part) as z:
                    for k in z.files:
                        parts.setdefault(k, []).append(z[k])
    out = {"cases": np.array(cases)}      # one member per quantity, the cases laid end to end in the order of `cases`
    for k, arrays in parts.items():
        out[k] = np.concatenate([a.reshape(-1) for a in arrays])
    save(OUT, out)
    size = os.path.getsize(OUT)
    limit = os.path.getsize(os.path.join(REPO, "tests", "golden", "step_rules.npz"))
    print("move rules ok: %d cases, %d bytes" % (len(cases), size))
    assert size <= limit, "tests/golden/move_rules.npz is %d bytes: above the %d of step_rules.npz" % (size, limit)


if __name__ == "__main__":
    main()
