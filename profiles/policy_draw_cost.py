#!/usr/bin/env python3
"""What the policy draw (BatchedSim.set_policy_draw; include/cagpu.h CaPolicyDraw) costs: 4096 x 10 agents, fixture cases
with auto-reset, every policy internal --

  off   the draw never enabled: cagpu_step_ex, every slot an RVO agent for good (the product path as it was)
  on    set_policy_draw(pool = RVO / RVO / non-cooperative / static at [0.45, 0.45, 0.05, 0.05], ensure = 0):
        cagpu_step_draw, the " final" instantiation of the pipelined kernel with the draw behind a uniform test in its
        auto-reset branch, no reset_plan (an env that reset is queried on its pre-move state)

in two launch modes: `ring` (step_lookahead() from a ring of --ring steps, the bench.py default) and `step` (one launch per
step, bench.py --mode step).  The pool keeps the work of a step close to the all-RVO batch's (90 % RVO), so the difference
is the draw's own: the instantiation, the lottery at ~1 % of the envs per step, the lost plans.

Device events around blocks of steps, >= --seconds per mode after a warm-up, the modes ALTERNATE block by block in one
process so that clock drift hits all alike; the median block of each mode and the spread of the blocks are reported.  One
JSON line on stdout.

    python profiles/policy_draw_cost.py [--envs 4096] [--ring 20] [--seconds 0.6] [--modes ring_off,ring_on,step_off,step_on]
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
    ap.add_argument("--modes", default="ring_off,ring_on,step_off,step_on")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N = args.envs, 10
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)
    pool = [core.policy_word_bits(p) for p in (nat.POL_RVO, nat.POL_RVO, nat.POL_NONCOOP, nat.POL_STATIC)]

    def make(mode):
        launch, draw = mode.split("_")
        s = core.BatchedSim(core.make_params(E, N), device=dev)
        s.set_plugins(nat.POL_RVO)
        s.set_fixture_table(table)
        if draw == "on":
            s.set_policy_draw(pool, [0.45, 0.45, 0.05, 0.05], ensure=0, seed=0xC0FFEE)
        s.reset_from_table()
        s.rollout(150)                       # steady state: envs spread over their episodes
        if launch == "ring":
            s.enable_lookahead(args.ring, fresh=True)
        return s

    sims = {m: make(m) for m in args.modes.split(",")}
    kernels, endings = {}, {}

    def block(mode):
        s = sims[mode]
        ring = mode.startswith("ring")
        overs = []
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.block):
            overs.append(s.step_lookahead()[3] if ring else s.step()[2].clone())
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
    out = {"what": "policy draw cost, us per step of %d x %d (median block of %d steps, device events)" % (E, N, args.block),
           "ring": args.ring, "blocks": {m: len(v) for m, v in times.items()},
           "us_per_step": {m: round(float(np.median(v)), 3) for m, v in times.items()},
           "us_per_step_min_max": {m: [round(min(v), 3), round(max(v), 3)] for m, v in times.items()},
           "us_per_step_quartiles": {m: [round(float(np.percentile(v, q)), 3) for q in (25, 75)] for m, v in times.items()},
           "endings_per_env_step": {m: round(v, 5) for m, v in endings.items()},
           "last_kernel": kernels, "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    u = out["us_per_step"]
    for launch in ("ring", "step"):
        if launch + "_on" in u and launch + "_off" in u:
            out["%s_on_over_off" % launch] = round(u[launch + "_on"] / u[launch + "_off"], 4)
    for s in sims.values():
        s.check_faults()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
