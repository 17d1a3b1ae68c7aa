#!/usr/bin/env python3
"""What a step of a MAP batch costs in its three launch forms: 4096 x 10 RVO agents between walls, fixture cases with
auto-reset, a single map (`map`) and a set of 16 maps drawn anew at every auto-reset (`set`) --

  step     one launch per step: step()
  rollout  rollout(20): 20 steps fused into one launch (cagpu_step_ex_maps, CaStepEx.n_steps)
  ring     step_lookahead() from a look-ahead ring of 20 (CaStepEx.ring)

Device events around blocks of steps, >= --seconds per case after a warm-up, the cases ALTERNATE block by block in one
process so that clock drift hits all alike; the median block of each case and the spread of the blocks are reported.
`--forms step` runs on a tree without fused map launches (the parent commit) with the same command.  One JSON line.

    python profiles/map_rollout_cost.py [--envs 4096] [--ring 20] [--seconds 0.5] [--forms step,rollout,ring] [--kinds map,set]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def walls(M, seed):
    """M grids of 160 x 160 cells: scattered cells and two bands whose place differs per map"""
    rng = np.random.default_rng(seed)
    out = np.zeros((M, 160, 160), bool)
    for m in range(M):
        out[m] = rng.random((160, 160)) < 0.002
        r0 = 20 + (120 * m) // M
        out[m, r0:r0 + 3, 10 + 3 * m:150 - 3 * m] = True
        out[m, 20:140, 30 + 6 * m:32 + 6 * m] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block (a multiple of --ring)")
    ap.add_argument("--forms", default="step,rollout,ring")
    ap.add_argument("--kinds", default="map,set")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N, L = args.envs, 10, args.ring
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)
    grids = walls(16, 3)

    def make(kind, form):
        s = core.BatchedSim(core.make_params(E, N), device=dev)
        s.set_plugins(nat.POL_RVO)
        if kind == "map":
            s.set_map(grids[0])
        else:
            s.set_map(grids, map_seed=77)
        s.set_fixture_table(table)
        s.reset_from_table()
        for _ in range(150):                 # steady state: envs spread over their episodes (single steps: any tree)
            s.step()
        if form == "ring":
            s.enable_lookahead(L, fresh=True)
        return s

    cases = [(k, f) for k in args.kinds.split(",") for f in args.forms.split(",")]
    sims = {c: make(*c) for c in cases}
    kernels = {}

    def block(case):
        s, form = sims[case], case[1]
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if form == "step":
            for _ in range(args.block):
                s.step()
        elif form == "rollout":
            for _ in range(args.block // L):
                s.rollout(L)
        else:
            for _ in range(args.block):
                s.step_lookahead()
        e1.record()
        e1.synchronize()
        kernels[case] = nat.lib().cagpu_last_kernel().decode()
        return e0.elapsed_time(e1) * 1e3 / args.block

    for case in cases:                       # warm-up: code objects, allocator
        block(case)
        block(case)
    times = {c: [] for c in cases}
    while min(sum(v) for v in times.values()) * args.block < args.seconds * 1e6:
        for case in cases:
            times[case].append(block(case))
    name = lambda c: "%s/%s" % c
    out = {"what": "map batch, us per step of %d x %d (median block of %d steps, device events)" % (E, N, args.block),
           "ring": L, "blocks": {name(c): len(v) for c, v in times.items()},
           "us_per_step": {name(c): round(float(np.median(v)), 3) for c, v in times.items()},
           "us_per_step_min_max": {name(c): [round(min(v), 3), round(max(v), 3)] for c, v in times.items()},
           "collision_episodes_share": {name(c): round(float(s._state["env_stats"][:, 1].sum() / max(1.0, float(s._state["env_stats"][:, 0].sum()))), 4)
                                        for c, s in sims.items()},
           "last_kernel": {name(c): k for c, k in kernels.items()}, "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    for s in sims.values():
        s.check_faults()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
