"""The two-agent trajectory dataset, all episodes in one recording batch (reference:
experiments/src/run_trajectory_dataset_creator.py, which runs `num_test_cases` random two-agent RVO episodes one after the
other and turns agent 0's `global_state_history` into one record per timestep).

Here the cases are drawn on the device (`set_fixture_suite(generate=...)`: the reference's get_testcase_random with
side_length 7), every env of the batch plays case e, e + E, e + 2 E, ... through the on-device auto-reset, and the
histories come off the device trajectory tape (`env.record_trajectories()`), written by the step kernels at full speed.

    GYM_CONFIG_CLASS=EvaluateConfig python -m gym_collision_avoidance_amd.experiments.run_trajectory_dataset_creator
"""
import os
import pickle

import numpy as np

from gym_collision_avoidance_amd import trajectory
from gym_collision_avoidance_amd.envs.collision_avoidance_env import CollisionAvoidanceEnv


def create_dataset(num_test_cases=500, num_envs=None, seed=0, side_length=7.0, device="cuda:0", horizon_secs=3.0,
                   max_steps=20000, angular="delta"):
    """-> list of `num_test_cases` lists of trajectory.dataset_samples records: entry c belongs to generated case c
    (agent 0 the robot, agent 1 the pedestrian)."""
    C_ = int(num_test_cases)
    E = int(min(C_, 256) if num_envs is None else num_envs)
    env = CollisionAvoidanceEnv(num_envs=max(E, 2), device=device)
    E = env.num_envs
    env.set_fixture_suite(2, policies="RVO", generate=dict(num_cases=C_, seed=int(seed), side_length=float(side_length)),
                          auto_reset=True, case_stride=E, random_headings=False)
    env.record_trajectories()
    env.reset()
    need = np.array([len(range(e, C_, E)) for e in range(E)])      # episodes env e has to finish
    steps = 0
    while steps < max_steps:
        for _ in range(64):
            env.step(None)
        steps += 64
        if (env._sim.state["reset_count"].cpu().numpy() >= need).all():
            break
    dt = env.dt_nominal
    tape = {k: v.cpu().numpy() for k, v in env.trajectories().items()}
    out = [[] for _ in range(C_)]
    for e in range(E):
        eps = trajectory.episodes(tape["rows"], tape["episode"], e, epoch=tape["epoch"])
        for k, (ego, other) in enumerate(eps[:need[e]]):
            if k >= int(tape["episode"][-1, e]) or not ego.shape[0]:
                continue              # (not finished within max_steps)
            out[e + k * E] = trajectory.dataset_samples(ego, other, ego[0, 3:5], dt, horizon_secs=horizon_secs,
                                                        angular=angular)
    return out


def main(num_test_cases=500, results_dir=None):
    trajs = create_dataset(num_test_cases)
    results_dir = results_dir or os.path.join(os.path.dirname(os.path.realpath(__file__)), "results", "trajectory_dataset",
                                              "2_agents", "trajs")
    os.makedirs(results_dir, exist_ok=True)
    fname = os.path.join(results_dir, "RVO.pkl")
    with open(fname, "wb") as f:
        pickle.dump(trajs, f)
    print("dumped %s: %d episodes, %d samples" % (fname, len(trajs), sum(len(t) for t in trajs)))


if __name__ == "__main__":
    main()
    print("Experiment over.")
