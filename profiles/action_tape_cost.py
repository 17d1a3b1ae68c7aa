#!/usr/bin/env python3
"""What a step costs a caller who drives ONE agent per env from outside: 4096 x 10, fixture cases with auto-reset, a
LearningPolicy agent in slot 0 of every env among nine RVO agents, actions from a seeded tape A [20, E, N, 2] --

  step      step(A[t]): one launch per step (all such a caller had before the tape)
  tape      rollout(20, A): 20 steps fused into one launch, slot t for step t (cagpu_step_tape)
  tape_keep rollout(20, A, keep_steps=True): the same launch as a ring launch, every step's outputs kept
  internal  rollout(20) of the all-internal twin (ten RVO agents): what the fused launch costs without a tape

Device events around blocks of steps, >= --seconds per case after a warm-up, the cases ALTERNATE block by block in one
process so that clock drift hits all alike; the median block of each case and the spread of the blocks are reported.
One JSON line.

    python profiles/action_tape_cost.py [--envs 4096] [--steps 20] [--seconds 0.5] [--forms step,tape,tape_keep,internal]
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block (a multiple of --steps)")
    ap.add_argument("--forms", default="step,tape,tape_keep,internal")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N, L = args.envs, 10, args.steps
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(1)
    A = np.full((L, E, N, 2), np.nan)                      # (nobody but slot 0 reads its entries)
    A[:, :, 0] = rng.uniform(0.3, 1.0, (L, E, 2))
    A = torch.as_tensor(A).to(dev)

    def make(form):
        s = core.BatchedSim(core.make_params(E, N), device=dev)
        pol = np.full((E, N), nat.POL_RVO)
        if form != "internal":
            pol[:, 0] = nat.POL_LEARNING
        s.set_plugins(pol)
        s.set_fixture_table(table)
        s.reset_from_table()
        for t in range(150):                 # steady state: envs spread over their episodes
            s.step(None if form == "internal" else A[t % L])
        return s

    cases = args.forms.split(",")
    sims = {c: make(c) for c in cases}
    kernels = {}

    def block(form):
        s = sims[form]
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if form == "step":
            for t in range(args.block):
                s.step(A[t % L])
        elif form == "internal":
            for _ in range(args.block // L):
                s.rollout(L)
        else:
            for _ in range(args.block // L):
                s.rollout(L, A, keep_steps=form == "tape_keep")
        e1.record()
        e1.synchronize()
        kernels[form] = nat.lib().cagpu_last_kernel().decode()
        return e0.elapsed_time(e1) * 1e3 / args.block

    for c in cases:                          # warm-up: code objects, allocator
        block(c)
        block(c)
    times = {c: [] for c in cases}
    while min(sum(v) for v in times.values()) * args.block < args.seconds * 1e6:
        for c in cases:
            times[c].append(block(c))
    out = {"what": "one external agent per env, us per step of %d x %d (median block of %d steps, device events)" % (E, N, args.block),
           "steps_per_launch": L, "blocks": {c: len(v) for c, v in times.items()},
           "us_per_step": {c: round(float(np.median(v)), 3) for c, v in times.items()},
           "us_per_step_min_max": {c: [round(min(v), 3), round(max(v), 3)] for c, v in times.items()},
           "episodes": {c: float(s._state["env_stats"][:, 0].sum()) for c, s in sims.items()},
           "last_kernel": dict(kernels), "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    for s in sims.values():
        s.check_faults()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
