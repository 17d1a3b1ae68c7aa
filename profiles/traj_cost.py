#!/usr/bin/env python3
"""What the device trajectory tape costs, and what it saves: 4096 x 10 RVO agents, fixture cases with auto-reset,
`step_lookahead()` from a ring of 20 --

  off        recording off (the product path as it was)
  on         record_trajectories(): the step kernels write every agent's history row
  readback   recording off, `sim.state["pos_x"]` read after every step: the only way to get at the paths of a batch
             without the tape (every read rewinds the look-ahead ring and shrinks the next one to one launch per step)

Synchronised wall clock around blocks of steps, >= 0.5 s per mode after a warm-up, modes interleaved block by block so
that clock drift hits all three alike; the median block of each mode is reported.  One JSON line on stdout.

    python profiles/traj_cost.py [--envs 4096] [--ring 20] [--seconds 0.6]
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
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N = args.envs, 10
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)

    def make(record):
        s = core.BatchedSim(core.make_params(E, N), device=dev)
        s.set_plugins(nat.POL_RVO)
        s.set_fixture_table(table)
        s.reset_from_table()
        s.rollout(150)                       # steady state: envs spread over their episodes
        if record:
            s.record_trajectories(max_bytes=(args.block + args.ring) * (96 * E * N + 4 * E))
        s.enable_lookahead(args.ring, fresh=True)
        return s

    sims = {"off": make(False), "on": make(True), "readback": make(False)}
    kernels = {}

    def block(mode):
        s = sims[mode]
        if mode == "on":
            s.clear_trajectories()           # (the budget never ends a block)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if mode == "readback":
            for _ in range(args.block):
                s.step_lookahead()
                s.state["pos_x"].cpu()
        else:
            for _ in range(args.block):
                s.step_lookahead()
        torch.cuda.synchronize(dev)
        kernels[mode] = nat.lib().cagpu_last_kernel().decode()
        return (time.perf_counter() - t0) / args.block * 1e6

    for mode in sims:                        # warm-up: allocator, ring adaptation of the read-back caller
        block(mode)
        block(mode)
    times = {m: [] for m in sims}
    while min(sum(v) for v in times.values()) * args.block < args.seconds * 1e6:
        for mode in sims:
            times[mode].append(block(mode))
    tape = sims["on"].trajectories()
    out = {"what": "trajectory tape cost, us per step of %d x %d (median block of %d steps)" % (E, N, args.block),
           "ring": args.ring, "blocks": {m: len(v) for m, v in times.items()},
           "us_per_step": {m: round(float(np.median(v)), 3) for m, v in times.items()},
           "us_per_step_min_max": {m: [round(min(v), 3), round(max(v), 3)] for m, v in times.items()},
           "tape_bytes_per_step": 96 * E * N + 4 * E, "tape_steps_last_block": int(tape["rows"].shape[0]),
           "moved_fraction_last_block": round(float((tape["rows"][..., 11] >= 0).double().mean()), 4),
           "last_kernel": kernels, "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    u = out["us_per_step"]
    out["on_over_off"] = round(u["on"] / u["off"], 4)
    out["on_faster_than_readback"] = bool(u["on"] < u["readback"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
