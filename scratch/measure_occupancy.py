#!/usr/bin/env python3
"""scratch/measure_occupancy.py -- what the OccupancyGridSensor kernel (csrc/cagpu_occ.inc) costs, on the GPU.

  python scratch/measure_occupancy.py --out profiles/occupancy_grid.json     # the figures below, device events
  rocprofv3 --kernel-trace --stats -d DIR -o occ -- python scratch/measure_occupancy.py --launch-only
                                                                             # kernel time proper, a run of its own
  python scratch/measure_occupancy.py --md profiles/occupancy_grid.json [--stats DIR/occ_results.db]
                                                                             # the note beside the JSON

Figures (every shape warmed up first, >= 0.5 s of launches per figure, contenders alternated block by block in one process):
  * the HIP kernel against the same sensor composed from torch ops on the device -- all a user of the library could do
    without the kernel: the dynamic map by a broadcast compare per agent slot, the crop by a gather -- at 4096 x 10 and
    4096 x 50, `cells` output, after the two were checked equal;
  * both output formats against the HBM bound: algorithmic bytes = output + 24 B of state per agent + one static grid per
    env, over 8 TB/s (bench.py's roofline figure);
  * step + laserscan + occupancy beside step + laserscan at 4096 x 50."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_BYTES_PER_S = 8.0e12
MIN_SECONDS = 0.5


def build(E, N, packed, seed=1):
    import numpy as np
    from gym_collision_avoidance_amd import core
    rng = np.random.default_rng(seed)
    static = rng.random((160, 160)) < 0.01
    static[40:44, 20:140] = True
    static[20:140, 60:63] = True
    sim = core.BatchedSim(core.make_params(E, N, max_obs=min(N - 1, 9), max_time_ratio=1.5), pipeline=(N <= 10))
    sim.set_map(static)
    sim.set_occupancy_grid(packed=packed)
    table = np.zeros((600, N, 6))
    table[..., 0:2] = rng.uniform(-7.5, 7.5, (600, N, 2))
    table[..., 2:4] = rng.uniform(-7.5, 7.5, (600, N, 2))
    table[..., 4] = rng.uniform(0.5, 2.0, (600, N))
    table[..., 5] = rng.uniform(0.2, 0.5, (600, N))
    sim.set_fixture_table(table)
    sim.reset_from_table()
    for _ in range(10):
        sim.step()
    return sim, static


def torch_occupancy(sim, static_t, H=50, W=50, x_width=5., y_width=5.):
    """the sensor from torch ops: bool [E, N, H, W]"""
    import torch
    st = sim._state
    px, py, rad = st["pos_x"], st["pos_y"], st["radius"]
    E, N = px.shape
    R, C = static_t.shape
    cell, origin_r, origin_c = 0.1, (R * 0.1 / 2.) / 0.1, (C * 0.1 / 2.) / 0.1
    gr = torch.floor(origin_r - py / cell)
    gc = torch.floor(origin_c + px / cell)
    inside = (gr >= 0) & (gc >= 0) & (gr < R) & (gc < C)
    rr = (rad / cell) ** 2
    rows = torch.arange(R, device=px.device, dtype=torch.float64).view(1, R, 1)
    cols = torch.arange(C, device=px.device, dtype=torch.float64).view(1, 1, C)
    dyn = static_t.unsqueeze(0).expand(E, R, C).clone()
    for n in range(N):   # (one slot at a time: the [E, N, R, C] broadcast would be 5 GB at N = 50)
        d2 = (cols - gc[:, n].view(E, 1, 1)) ** 2 + (rows - gr[:, n].view(E, 1, 1)) ** 2
        dyn |= (d2 < rr[:, n].view(E, 1, 1)) & inside[:, n].view(E, 1, 1)
    i0 = torch.floor(origin_r - (py + y_width / 2.) / cell).long()
    j0 = torch.floor(origin_c + (px - x_width / 2.) / cell).long()
    r = i0.unsqueeze(-1) + torch.arange(H, device=px.device)          # [E, N, H]
    c = j0.unsqueeze(-1) + torch.arange(W, device=px.device)          # [E, N, W]
    ok = ((r >= 0) & (r < R)).unsqueeze(-1) & ((c >= 0) & (c < C)).unsqueeze(-2)
    idx = r.clamp(0, R - 1).unsqueeze(-1) * C + c.clamp(0, C - 1).unsqueeze(-2)     # [E, N, H, W]
    out = torch.gather(dyn.view(E, 1, R * C).expand(E, N, R * C), 2, idx.view(E, N, H * W)).view(E, N, H, W)
    return out & ok


def timed(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def alternate(contenders, min_seconds=MIN_SECONDS):
    """contenders: {name: callable}; blocks of launches, alternated, until every contender has min_seconds -> {name: seconds
    per launch (total time / launches), launches}"""
    import torch
    for fn in contenders.values():       # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    reps = {}
    for name, fn in contenders.items():  # block size: ~50 ms
        t = timed(fn, 2) / 2
        reps[name] = max(1, int(0.05 / max(t, 1e-7)))
    tot = {n: 0.0 for n in contenders}
    cnt = {n: 0 for n in contenders}
    while min(tot.values()) < min_seconds:
        for name, fn in contenders.items():
            tot[name] += timed(fn, reps[name])
            cnt[name] += reps[name]
    return {n: dict(seconds_per_launch=tot[n] / cnt[n], launches=cnt[n], seconds=tot[n]) for n in contenders}


def algorithmic_bytes(E, N, H, W, packed):
    out = E * N * H * ((W + 31) // 32) * 4 if packed else E * N * H * W
    return out + 24 * E * N + E * 160 * 5 * 4


def measure(out_path):
    import torch
    res = dict(device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, min_seconds_per_figure=MIN_SECONDS,
               shapes={})
    for N in (10, 50):
        E = 4096
        key = "%dx%d" % (E, N)
        sim, static = build(E, N, packed=False)
        static_t = torch.from_numpy(static).to(sim.device)
        got = sim.occupancy_grid()
        ref = torch_occupancy(sim, static_t)
        equal = bool(torch.equal(got, ref))
        assert equal, "the torch composition and the kernel disagree at %s" % key
        r = alternate({"hip_cells": sim.occupancy_grid, "torch_cells": lambda: torch_occupancy(sim, static_t)})
        del ref
        entry = dict(checked_equal=equal, hip_cells=r["hip_cells"], torch_cells=r["torch_cells"],
                     torch_over_hip=r["torch_cells"]["seconds_per_launch"] / r["hip_cells"]["seconds_per_launch"])
        # the two formats against the HBM bound (the packed sim on the same state)
        simb, _ = build(E, N, packed=True)
        rb = alternate({"hip_cells": sim.occupancy_grid, "hip_bits": simb.occupancy_grid})
        for name, packed in (("hip_cells", False), ("hip_bits", True)):
            nbytes = algorithmic_bytes(E, N, 50, 50, packed)
            t = rb[name]["seconds_per_launch"]
            entry["roofline_" + name] = dict(seconds_per_launch=t, launches=rb[name]["launches"], algorithmic_bytes=nbytes,
                                             hbm_bound_seconds=nbytes / HBM_BYTES_PER_S,
                                             share_of_hbm_bound=(nbytes / HBM_BYTES_PER_S) / t)
        if N == 50:     # what enabling the sensor costs per step at config-5 geometry
            def step_scan():
                sim.step()
                sim.laserscan()

            def step_scan_occ():
                sim.step()
                sim.laserscan()
                sim.occupancy_grid()
            rs = alternate({"step_laserscan": step_scan, "step_laserscan_occupancy": step_scan_occ})
            entry["per_step"] = rs
            entry["per_step"]["occupancy_share"] = 1.0 - (rs["step_laserscan"]["seconds_per_launch"] /
                                                          rs["step_laserscan_occupancy"]["seconds_per_launch"])
        res["shapes"][key] = entry
        del sim, simb
        torch.cuda.empty_cache()
    from gym_collision_avoidance_amd import _native as nat
    res["device_faults"] = nat.device_faults(clear=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    json.dump(res, open(out_path, "w"), indent=1)
    print(json.dumps(res))


def launch_only():
    """a handful of launches of every measured shape and format, for a rocprofv3 --kernel-trace --stats run"""
    import torch
    for N in (10, 50):
        for packed in (False, True):
            sim, _ = build(4096, N, packed=packed)
            for _ in range(20):
                sim.occupancy_grid()
            torch.cuda.synchronize()
            del sim
            torch.cuda.empty_cache()


def write_md(json_path, stats_db):
    res = json.load(open(json_path))
    us = lambda s: "%.1f us" % (s * 1e6)
    lines = ["# OccupancyGridSensor kernel: measured cost", "",
             "Written by `scratch/measure_occupancy.py --md` from `%s` (%s; device events, every shape warmed up, at least "
             "%.1f s of launches per figure, contenders alternated block by block in one process)." %
             (os.path.basename(json_path), res["device"], res["min_seconds_per_figure"]), ""]
    lines += ["## Against the same sensor composed from torch ops (`cells` output)", "",
              "| batch | HIP kernel | torch composition | torch / HIP | checked equal |", "|---|---|---|---|---|"]
    for key, e in res["shapes"].items():
        lines.append("| %s | %s | %s | %.1f x | %s |" % (key, us(e["hip_cells"]["seconds_per_launch"]),
                                                         us(e["torch_cells"]["seconds_per_launch"]), e["torch_over_hip"],
                                                         e["checked_equal"]))
    lines += ["", "## Against the HBM bound (algorithmic bytes = output + 24 B of state per agent + one static grid per env, "
              "over %.0f TB/s)" % (res["hbm_bytes_per_s"] / 1e12), "",
              "| batch | format | bytes | bound | measured | share of the bound |", "|---|---|---|---|---|---|"]
    for key, e in res["shapes"].items():
        for name in ("hip_cells", "hip_bits"):
            r = e["roofline_" + name]
            lines.append("| %s | %s | %.1f MB | %s | %s | %.0f %% |" % (key, name[4:], r["algorithmic_bytes"] / 1e6,
                                                                       us(r["hbm_bound_seconds"]), us(r["seconds_per_launch"]),
                                                                       100 * r["share_of_hbm_bound"]))
    for key, e in res["shapes"].items():
        if "per_step" in e:
            p = e["per_step"]
            lines += ["", "## What enabling the sensor costs per step (%s)" % key, "",
                      "step + laserscan: %s; step + laserscan + occupancy: %s (the sensor is %.1f %% of the step)." %
                      (us(p["step_laserscan"]["seconds_per_launch"]), us(p["step_laserscan_occupancy"]["seconds_per_launch"]),
                       100 * p["occupancy_share"])]
    e10 = res["shapes"].get("4096x10")
    if e10:
        c, b = e10["roofline_hip_cells"], e10["roofline_hip_bits"]
        lines += ["", "Reading: the gate (the HIP kernel is not slower than the torch composition) holds by two orders of magnitude at "
                  "both sizes.  Against the HBM bound the `bits` launch moves %.0f %% of the `cells` bytes in %.0f %% of its time: "
                  "a launch carries a per-env chain ahead of its first store (static grid -> LDS, barrier, state, barrier, "
                  "discs, barrier) that one workgroup per env does not hide; the bytes `cells` adds over `bits` leave at "
                  "%.1f TB/s." % (100 * b["algorithmic_bytes"] / c["algorithmic_bytes"],
                                  100 * b["seconds_per_launch"] / c["seconds_per_launch"],
                                  (c["algorithmic_bytes"] - b["algorithmic_bytes"]) /
                                  (c["seconds_per_launch"] - b["seconds_per_launch"]) / 1e12)]
    lines += ["", "## Kernel time proper (rocprofv3 --kernel-trace --stats, a run of its own)", ""]
    if stats_db and os.path.exists(stats_db):
        import sqlite3
        import statistics
        rows = sqlite3.connect(stats_db).execute(
            "select duration, lds_size, scratch_size, vgpr_count, workgroup_x from kernels where name like '%occ_kernel%' "
            "order by dispatch_id").fetchall()
        labels = ["4096x10 cells", "4096x10 bits", "4096x50 cells", "4096x50 bits"]   # launch_only()'s order, 20 launches each
        if len(rows) == 20 * len(labels):
            lines += ["| batch, format | median | min | max |", "|---|---|---|---|"]
            for i, lab in enumerate(labels):
                d = [r[0] for r in rows[20 * i:20 * i + 20]]
                lines.append("| %s | %.1f us | %.1f us | %.1f us |" % (lab, statistics.median(d) / 1e3, min(d) / 1e3, max(d) / 1e3))
            lines += ["", "Dispatch record: %d threads per workgroup, %d B of LDS, %d B of scratch per lane." %
                      (rows[0][4], rows[0][1], rows[0][2])]
        else:
            lines.append("not measured (%d occ_kernel dispatches in the trace, expected %d)" % (len(rows), 20 * len(labels)))
    else:
        lines.append("not measured")
    open(os.path.splitext(json_path)[0] + ".md", "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_grid.json"))
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--md", default=None)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.md:
        write_md(a.md, a.stats)
    elif a.launch_only:
        launch_only()
    else:
        measure(a.out)
