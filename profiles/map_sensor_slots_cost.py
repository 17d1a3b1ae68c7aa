#!/usr/bin/env python3
"""What a step of a MAP batch costs WITH its laser scan, and what the slot march costs against single scans --

  map batch (--envs x 10 RVO agents between dense walls, fixture cases with auto-reset), us per step, scan included:
    step+scan   one step launch + one laserscan() per step (the only form before the per-slot sensors)
    ring+slots  step_lookahead() from a ring of --ring with map_sensors: per refill the pose kernel and the slot march,
                per step the history kernel
  config-5 shape (--envs x 50): the sensor kernels alone on a pose ring of --ring slots, us per --ring slots:
    scans       --ring launches of scan_kernel (laserscan())
    march       cagpu_tape_poses + cagpu_laserscan_slots over --ring slots + one cagpu_laserscan_history per slot

Device events around blocks, >= --seconds per case after a warm-up, the cases ALTERNATE block by block in one process so
that clock drift hits all alike; the median block of each case and the spread of the blocks are reported.  `--forms
step+scan,scans` runs on a tree without the per-slot sensors (the parent commit) with the same command.  One JSON line.

    python profiles/map_sensor_slots_cost.py [--envs 4096] [--ring 20] [--seconds 0.5] [--forms step+scan,ring+slots,scans,march]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def walls(seed):
    """160 x 160 cells, dense: scattered cells and a lattice of bands"""
    rng = np.random.default_rng(seed)
    out = rng.random((160, 160)) < 0.004
    for r0 in range(20, 150, 30):
        out[r0:r0 + 3, 10:150] = True
    for c0 in range(30, 150, 40):
        out[20:140, c0:c0 + 2] = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--ring", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block of the map batch (a multiple of --ring)")
    ap.add_argument("--forms", default="step+scan,ring+slots,scans,march")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, L = args.envs, args.ring
    data = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))
    dev = torch.device("cuda", 0)
    grid = walls(3)

    def make(N, warm):
        s = core.BatchedSim(core.make_params(E, N, max_obs=min(N - 1, 19)), device=dev)
        s.set_plugins(nat.POL_RVO)
        s.set_map(grid)
        table = data["n%d" % N] if ("n%d" % N) in data.files else None
        if table is None:              # no fixture set of that size: random cases, as the test suites draw them
            rng = np.random.default_rng(N)
            table = np.zeros((512, N, 6))
            table[..., 0:2] = rng.uniform(-7, 7, (512, N, 2))
            table[..., 2:4] = rng.uniform(-7, 7, (512, N, 2))
            table[..., 4] = rng.uniform(0.5, 2.0, (512, N))
            table[..., 5] = rng.uniform(0.2, 0.5, (512, N))
        s.set_fixture_table(table)
        s.reset_from_table()
        for _ in range(warm):          # steady state: envs spread over their episodes
            s.step()
        s.laserscan()
        return s

    forms = args.forms.split(",")
    sims, kept = {}, {}
    for f in forms:
        if f in ("step+scan", "ring+slots"):
            sims[f] = make(10, 150)
            if f == "ring+slots":
                sims[f].enable_lookahead(L, fresh=True, map_sensors=True)
        else:
            sims[f] = make(50, 40)
            if f == "march":           # one launch to take the tape, the state and the game_over ring from
                s = sims[f]
                s.record_trajectories()
                start = s._map_slots_start()
                ring = s.rollout(L, keep_steps=True)
                tr = s.trajectories()
                ct = nat.CaTraj(rows=tr["rows"].data_ptr(), episode=tr["episode"].data_ptr())
                kept[f] = (start, tr, ct, ring)
    per = {f: (args.block if f in ("step+scan", "ring+slots") else L) for f in forms}

    def block(f):
        s = sims[f]
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if f == "step+scan":
            for _ in range(args.block):
                s.step()
                s.laserscan()
        elif f == "ring+slots":
            for _ in range(args.block):
                s.step_lookahead()
        elif f == "scans":
            for _ in range(L):
                s.laserscan()
        else:
            start, tr, ct, ring = kept[f]
            k = s._map_slots_finish(L, start, ct, ring[3], expand_last=False)
            for t in range(L):
                k.expand_into_sim(t)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / (args.block if f in ("step+scan", "ring+slots") else 1)

    for f in forms:                    # warm-up: code objects, allocator
        block(f)
        block(f)
    times = {f: [] for f in forms}
    while min(sum(v) * (per[f] if f in ("step+scan", "ring+slots") else 1) for f, v in times.items()) < args.seconds * 1e6:
        for f in forms:
            times[f].append(block(f))
    out = {"what": "map batch %d x 10: us per step with the scan (median block of %d steps); config-5 shape %d x 50: us per %d "
                   "slots of sensors alone; device events" % (E, args.block, E, L),
           "ring": L, "blocks": {f: len(v) for f, v in times.items()},
           "us": {f: round(float(np.median(v)), 3) for f, v in times.items()},
           "us_min_max": {f: [round(min(v), 3), round(max(v), 3)] for f, v in times.items()},
           "lib_sha256": bn.file_sha256(nat.LIB_PATH)}
    for s in sims.values():
        s.check_faults()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
