#!/usr/bin/env python3
"""profiles/ga3c_query_cost.py -- what a GA3C-CADRL query launch costs (profiles/ga3c_query.md, section 3).

HIP-event time per launch, median of `--reps` launches after `--warm`, for
  * cagpu_ga3c_query on `--rows` random policy vectors [rows, 138] (default 81 920): logits + action, and + value;
  * the simulator path on 4096 x 20 agents, every agent alive (the same 81 920 rows): BatchedSim.ga3c() without and with
    keep_value (compact_kernel + the network kernel, what a config-3 step pays ahead of its step kernel).
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gym_collision_avoidance_amd import _native as nat  # noqa: E402
from gym_collision_avoidance_amd import core  # noqa: E402


def rows_like_the_bench(rng, n, K=19):
    obs = np.zeros((n, 6 + 7 * K), np.float32)
    obs[:, 1] = K
    obs[:, 2] = rng.uniform(0.1, 12.0, n)
    obs[:, 3] = rng.uniform(-np.pi, np.pi, n)
    obs[:, 4] = rng.uniform(0.5, 1.5, n)
    obs[:, 5] = rng.uniform(0.2, 0.8, n)
    obs[:, 6:] = rng.uniform(-3, 3, (n, 7 * K)).astype(np.float32)
    return obs


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    out = np.array(out)
    return {"median_us": float(np.median(out)), "min_us": float(out.min()), "p90_us": float(np.percentile(out, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=81920)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    E, N = a.rows // 20, 20
    obs = rows_like_the_bench(rng, E * N)
    x = torch.from_numpy(np.ascontiguousarray(obs[:, 1:])).cuda()
    res = {"rows": E * N, "device": torch.cuda.get_device_name(0)}
    res["query_logits_action"] = timed(lambda: core.ga3c_query(x, want=("logits", "action")), a.warm, a.reps)
    res["query_logits_action_value"] = timed(lambda: core.ga3c_query(x, want=("logits", "action", "value")), a.warm, a.reps)
    res["query_action"] = timed(lambda: core.ga3c_query(x, want=("action",)), a.warm, a.reps)
    for keep_value in (False, True):
        g = core.BatchedSim(core.make_params(E, N, max_obs=19, sort_mode=1))
        g.set_plugins(nat.POL_GA3C_CADRL)
        g.obs.copy_(torch.from_numpy(obs.reshape(E, N, -1)))
        g.load_ga3c(keep_value=keep_value)
        ext = torch.zeros((E, N, 2), dtype=torch.float64, device=g.device)
        res["sim_path_value" if keep_value else "sim_path_default"] = timed(lambda: g.ga3c(ext), a.warm, a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
