#!/usr/bin/env python3
"""What the episode metrics (BatchedSim.measure_episodes, cagpu_episode_metrics) cost per tape step, at 4096 x 10 and 512 x 100
RVO agents on a recorded tape of `--steps` slots --

  metrics  cagpu_episode_metrics over the tape, per slot
  copy8    reading the same rows once: cagpu_debug_copy8 of the tape's 12 E N doubles per slot (8 bytes read + 8 written
           per element: the streaming time of twice the tape's bytes)
  step     the step that recorded them: rollout(--steps) with recording on, per step

Device events around every block, the three ALTERNATE block by block in one process so that clock drift hits all alike,
>= --seconds per mode after a warm-up; the median block of each and the spread are reported.  One JSON line per geometry.

    python profiles/episode_metrics_cost.py [--steps 64] [--seconds 0.5] [--geometries 4096x10,512x100]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def measure(E, N, steps, seconds):
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    from gym_collision_avoidance_amd.envs import test_cases as tc
    dev = torch.device("cuda", 0)
    if N == 10:
        table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    else:
        np.random.seed(5)
        table = tc.make_testcase_huge(16, N, side_length=2.0 * np.sqrt(N) + 3.0, speed_bnds=[0.5, 1.5], radius_bnds=[0.2, 0.5])
    s = core.BatchedSim(core.make_params(E, N, max_time_ratio=1.5), device=dev)
    s.set_plugins(nat.POL_RVO)
    s.set_fixture_table(table)
    s.reset_from_table()
    s.rollout(100)                          # steady state: envs spread over their episodes
    s.record_trajectories(max_bytes=1 << 34)
    s.rollout(steps)
    step_kernel = nat.lib().cagpu_last_kernel().decode()
    tape = s.trajectories()
    rows, ep = tape["rows"].contiguous(), tape["episode"].contiguous()
    lib, p = nat.lib(), s.p
    cap = 16
    vals = torch.zeros((E, cap, N, 4), dtype=torch.float64, device=dev)
    cnts = torch.zeros((E, cap, N, 4), dtype=torch.int32, device=dev)
    head = torch.full((E, cap), -1, dtype=torch.int32, device=dev)
    carry = torch.zeros((int(lib.cagpu_episode_metrics_carry_bytes(C.byref(p))),), dtype=torch.uint8, device=dev)
    m = nat.CaEpMetrics(vals=vals.data_ptr(), cnts=cnts.data_ptr(), head=head.data_ptr(), capacity=cap, carry=carry.data_ptr(),
                        getting_close_range=p.getting_close_range)
    ct = nat.CaTraj(rows=rows.data_ptr(), episode=ep.data_ptr())
    dst = torch.empty_like(rows)
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def metrics():
        carry.zero_()
        nat.check(lib.cagpu_episode_metrics(C.byref(p), C.byref(ct), steps, C.byref(m), stream()))

    def copy8():
        nat.check(lib.cagpu_debug_copy8(rows.numel(), rows.data_ptr(), dst.data_ptr(), stream()))

    def step():
        s.clear_trajectories()
        s.rollout(steps)

    modes = {"metrics": metrics, "copy8": copy8, "step": step}
    times = {k: [] for k in modes}
    metrics()
    metrics_kernel = lib.cagpu_last_kernel().decode()
    for f in modes.values():
        f()
    torch.cuda.synchronize()
    total = 0.0
    while total < seconds * 1e3 * len(modes):
        for k, f in modes.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
            total += times[k][-1]
    us = lambda k, q: float(np.percentile(times[k], q)) * 1e3 / steps
    out = {"geometry": "%dx%d" % (E, N), "steps_per_block": steps, "blocks": len(times["metrics"]),
           "tape_bytes_per_step": int(rows.numel() // steps * 8), "metrics_kernel": metrics_kernel, "step_kernel": step_kernel,
           "lib": bn.build_info().get("lib_sha256")}
    for k in modes:
        out[k + "_us_per_step"] = {"median": round(us(k, 50), 3), "p10": round(us(k, 10), 3), "p90": round(us(k, 90), 3)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--geometries", default="4096x10,512x100")
    args = ap.parse_args()
    for g in args.geometries.split(","):
        E, N = (int(x) for x in g.split("x"))
        print(json.dumps(measure(E, N, args.steps, args.seconds)), flush=True)


if __name__ == "__main__":
    main()
