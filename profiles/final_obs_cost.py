#!/usr/bin/env python3
"""What the final record (BatchedSim.keep_final / env.keep_final_observations) costs: 4096 x 10 RVO agents, fixture cases
with auto-reset, `step_lookahead()` from a ring of 20 --

  off   the record never enabled (the product path as it was: cagpu_step_ex with CaStepEx.ring, no record)
  on    keep_final(): every ring slot carries its final block, the step kernels save the terminal rows / flag words of
        the envs that auto-reset (CaStepEx.fin)

Synchronised wall clock around blocks of steps, >= --seconds per mode after a warm-up, modes interleaved block by block so
that clock drift hits both alike; the median block of each mode is reported.  `--modes off` measures a library without the
record (the parent commit's build, named by CAGPU_LIB) with the same command.  `--env`: also the env API's default
adaptive ring with the record off / on -- the longest ring its byte budget allows, the length it settled on, us per step.
One JSON line on stdout.

    python profiles/final_obs_cost.py [--envs 4096] [--ring 20] [--seconds 0.6] [--modes off,on] [--env]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block (a multiple of --ring)")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--env", action="store_true")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N = args.envs, 10
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)

    def make(final):
        s = core.BatchedSim(core.make_params(E, N), device=dev)
        s.set_plugins(nat.POL_RVO)
        s.set_fixture_table(table)
        s.reset_from_table()
        s.rollout(150)                       # steady state: envs spread over their episodes
        if final:
            s.keep_final()
        s.enable_lookahead(args.ring, fresh=True)
        return s

    sims = {m: make(m == "on") for m in args.modes.split(",")}
    kernels, endings = {}, {}

    def block(mode):
        s = sims[mode]
        overs = []
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.block):
            overs.append(s.step_lookahead()[3])
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / args.block * 1e6
        kernels[mode] = nat.lib().cagpu_last_kernel().decode()
        endings[mode] = float(torch.stack(overs).float().mean())     # (episodes ending per env and step)
        return dt

    for mode in sims:                        # warm-up: code objects, allocator
        block(mode)
        block(mode)
    times = {m: [] for m in sims}
    while min(sum(v) for v in times.values()) * args.block < args.seconds * 1e6:
        for mode in sims:
            times[mode].append(block(mode))
    out = {"what": "final record cost, us per step of %d x %d (median block of %d steps)" % (E, N, args.block),
           "ring": args.ring, "blocks": {m: len(v) for m, v in times.items()},
           "us_per_step": {m: round(float(np.median(v)), 3) for m, v in times.items()},
           "us_per_step_min_max": {m: [round(min(v), 3), round(max(v), 3)] for m, v in times.items()},
           "endings_per_env_step": {m: round(v, 5) for m, v in endings.items()},
           "final_bytes_per_slot": E * N * (4 * (6 + 7 * (N - 1)) + 4),
           "last_kernel": kernels, "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    u = out["us_per_step"]
    if "on" in u and "off" in u:
        out["on_over_off"] = round(u["on"] / u["off"], 4)
    for s in sims.values():
        s.check_faults()
    if args.env:
        from gym_collision_avoidance_amd.envs.collision_avoidance_env import CollisionAvoidanceEnv
        res = {}
        for mode in sims:
            env = CollisionAvoidanceEnv(num_envs=E)
            env.set_fixture_suite(N)
            if mode == "on":
                env.keep_final_observations()
            env.reset()
            la = env._sim._la
            for _ in range(4 * la["n"]):     # the adaptive ring doubles up to its longest length
                env.step(None)
            steps = 4 * la["n"]
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(steps):
                env.step(None)
            torch.cuda.synchronize(dev)
            res[mode] = {"longest_ring": la["n"], "ring_settled_on": la["cur"], "obs_width": env._sim.W,
                         "us_per_step": round((time.perf_counter() - t0) / steps * 1e6, 3), "steps": steps,
                         "rewinds": la["rewinds"]}
        out["env_default_ring"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
