#!/usr/bin/env python3
"""What the case stream (BatchedSim.set_case_stream; include/cagpu.h CaCaseStream) costs: 4096 x 10 RVO agents, the
generator's default distribution, a look-ahead ring of --ring steps --

  table    a fixed table of E * W generated rows (case_stride = E) with reset_obs / reset_plan NULL: the same kernels, the
           same second sensing pass after an auto-reset, no refill
  stream   set_case_stream(window = W): the same plus one cagpu_stream_refill ahead of every ring launch

timed as blocks of --block steps (device events, the two ALTERNATE block by block in one process; median block, quartiles).
Then, on the stream batch's own state:

  refill   the refill alone -- both kernels, device events around one call -- at the stale fraction the run produces: --ring
           steps are stepped between two timed refills, so each regenerates what a ring uses up
  full     cagpu_generate_cases_ragged over the whole E * W window: the only way to refresh a table without the stream
  dense    cagpu_generate_cases_at over a dense list of --dense cases against cagpu_generate_cases on the same cases

One JSON line on stdout.

    python profiles/case_stream_cost.py [--envs 4096] [--window 8] [--ring 20] [--seconds 0.6]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SIDE = [{"num_agents": [0, 5], "side_length": [4, 5]}, {"num_agents": [5, 100], "side_length": [6, 8]}]   # config.py:118-131


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--ring", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--block", type=int, default=200, help="steps per timed block (a multiple of --ring)")
    ap.add_argument("--dense", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=40)
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core
    E, N, W, seed = args.envs, 10, args.window, 0x57A7
    dev = torch.device("cuda", 0)
    dist = dict(side_length=SIDE, num_agents=(2, N))

    def make(mode):
        s = core.BatchedSim(core.make_params(E, N, ragged=1), device=dev)
        s.set_plugins(nat.POL_RVO)
        if mode == "stream":
            s.set_case_stream(window=W, seed=seed, **dist)
            s.reset_from_stream()
        else:
            table = s.generate_cases(E * W, seed, **dist)
            s.set_fixture_table(table, case_stride=E)
            s._ar.reset_obs, s._ar.reset_plan = None, None
            s.reset(table[:E])
        for _ in range(15):                  # steady state: envs spread over their episodes
            s.rollout(min(W, 10))
        s.enable_lookahead(args.ring, fresh=True)
        return s

    sims = {m: make(m) for m in ("table", "stream")}
    endings = {}

    def timed(fn, n=1):
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    def block(mode):
        s, overs = sims[mode], []
        dt = timed(lambda: overs.append(s.step_lookahead()[3]), args.block)
        endings[mode] = float(torch.stack(overs).float().mean())
        return dt

    for mode in sims:
        block(mode)
        block(mode)
    times = {m: [] for m in sims}
    while min(sum(v) for v in times.values()) * args.block < args.seconds * 1e6:
        for mode in sims:
            times[mode].append(block(mode))
    med = {m: float(np.median(v)) for m, v in times.items()}

    # the refill alone, at the stale fraction a ring produces
    s = sims["stream"]
    s.sync()
    s.enable_lookahead(0)
    refill_us, stale = [], []
    for _ in range(args.reps):
        s._stream_refill()
        s._launch(s._p_ref, s._cs_ref, s._co_ref, None, s._ar_ref, core.C.byref(nat.CaStepEx(n_steps=args.ring)), s._stream_handle())
        refill_us.append(timed(s._stream_refill))
        stale.append(int(s._cstream["t"]["work_count"].item()))
    empty_us = [timed(s._stream_refill) for _ in range(args.reps)]        # nothing stale: the floor of the two launches
    # the whole window by the one-thread generator
    full_us = [timed(lambda: s.generate_cases(E * W, seed, **dist)) for _ in range(args.reps)]
    # a dense list, both generators
    g = core.BatchedSim(core.make_params(2, N), device=dev)
    idx = torch.arange(args.dense, device=dev, dtype=torch.int64)
    out = torch.empty((args.dense, N, 6), dtype=torch.float64, device=dev)
    g.generate_cases_at(idx, seed, out=out)
    g.generate_cases(args.dense, seed)
    at_us = [timed(lambda: g.generate_cases_at(idx, seed, out=out)) for _ in range(args.reps)]
    one_us = [timed(lambda: g.generate_cases(args.dense, seed)) for _ in range(args.reps)]
    q = lambda v: [round(float(np.percentile(v, p)), 3) for p in (25, 50, 75)]
    res = {"what": "case stream cost at %d x %d, window %d, ring of %d (device events)" % (E, N, W, args.ring),
           "blocks": {m: len(v) for m, v in times.items()},
           "us_per_step": {m: round(v, 3) for m, v in med.items()},
           "us_per_step_quartiles": {m: [round(float(np.percentile(v, p)), 3) for p in (25, 75)] for m, v in times.items()},
           "us_per_ring": {m: round(v * args.ring, 2) for m, v in med.items()},
           "stream_over_table": round(med["stream"] / med["table"], 4),
           "endings_per_env_step": {m: round(v, 5) for m, v in endings.items()},
           "refill_us_q25_q50_q75": q(refill_us), "refill_stale_rows_median": int(np.median(stale)),
           "refill_stale_fraction": round(float(np.median(stale)) / (E * W), 5),
           "refill_nothing_stale_us_q25_q50_q75": q(empty_us),
           "full_window_one_thread_us_q25_q50_q75": q(full_us), "window_rows": E * W,
           "dense_cases": args.dense, "dense_at_us_q25_q50_q75": q(at_us), "dense_one_thread_us_q25_q50_q75": q(one_us),
           "last_kernel": nat.lib().cagpu_last_kernel().decode(), "lib_sha256": bn.file_sha256(nat.LIB_PATH),
           "git_sha": bn.build_info().get("git_sha")}
    for b in sims.values():
        b.check_faults()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
