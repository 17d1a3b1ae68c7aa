#!/usr/bin/env python3
"""What the episode log (BatchedSim.log_episodes / env.log_episodes) costs: 4096 x 10 RVO agents, fixture cases with
auto-reset, `step_lookahead()` from a ring of 20 --

  off   the log never enabled (the product path as it was: cagpu_step_ex with CaStepEx.ring, no record)
  on    log_episodes(): the step kernels store a 32-byte row per agent and a 16-byte head per env for every env that
        auto-resets (CaStepEx.log, the " final" instantiation of the pipelined kernel with a uniform test inside)
  drain on + one episodes() call per block (a host synchronisation and a handful of torch kernels per drain)

Device events around blocks of steps, >= --seconds per mode after a warm-up, the modes ALTERNATE block by block in one
process so that clock drift hits all alike; the median block of each mode and the spread of the blocks are reported.
`--modes off` measures a library without the record (the parent commit's build, named by CAGPU_LIB) with the same
command.  One JSON line on stdout.

    python profiles/episode_log_cost.py [--envs 4096] [--ring 20] [--seconds 0.6] [--modes off,on,drain]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block (a multiple of --ring)")
    ap.add_argument("--capacity", type=int, default=16)
    ap.add_argument("--modes", default="off,on,drain")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N = args.envs, 10
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)

    def make(mode):
        s = core.BatchedSim(core.make_params(E, N), device=dev)
        s.set_plugins(nat.POL_RVO)
        s.set_fixture_table(table)
        s.reset_from_table()
        s.rollout(150)                       # steady state: envs spread over their episodes
        if mode != "off":
            s.log_episodes(capacity=args.capacity)
        s.enable_lookahead(args.ring, fresh=True)
        return s

    sims = {m: make(m) for m in args.modes.split(",")}
    kernels, endings, logged = {}, {}, {m: 0 for m in sims}
    dropped = {m: 0 for m in sims}

    def block(mode):
        s = sims[mode]
        overs = []
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.block):
            overs.append(s.step_lookahead()[3])
        if mode == "drain":
            ep = s.episodes()
            logged[mode] += int(ep["env"].shape[0])
            dropped[mode] += ep["dropped"]
        e1.record()
        e1.synchronize()
        dt = e0.elapsed_time(e1) * 1e3 / args.block
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
    out = {"what": "episode log cost, us per step of %d x %d (median block of %d steps, device events)" % (E, N, args.block),
           "ring": args.ring, "capacity": args.capacity, "blocks": {m: len(v) for m, v in times.items()},
           "us_per_step": {m: round(float(np.median(v)), 3) for m, v in times.items()},
           "us_per_step_min_max": {m: [round(min(v), 3), round(max(v), 3)] for m, v in times.items()},
           "us_per_step_quartiles": {m: [round(float(np.percentile(v, q)), 3) for q in (25, 75)] for m, v in times.items()},
           "endings_per_env_step": {m: round(v, 5) for m, v in endings.items()},
           "log_bytes": E * args.capacity * (16 + 32 * N),
           "last_kernel": kernels, "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    if "drain" in sims:
        out["drained_episodes"], out["dropped"] = logged["drain"], dropped["drain"]
    u = out["us_per_step"]
    for m in ("on", "drain"):
        if m in u and "off" in u:
            out["%s_over_off" % m] = round(u[m] / u["off"], 4)
    for s in sims.values():
        s.check_faults()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
