#!/usr/bin/env python3
"""What rendering costs (core.BatchedSim.render_frames / render_episode, csrc/cagpu_render.inc), by HIP events around
blocks of calls after a warm-up, the median block reported:

  (a) render_episode of one recorded 10-agent episode at 128 x 128 and at the reference's 1000 x 800 (one launch pair
      for all frames);
  (b) render_frames of all --envs envs at 64 x 64, episode="last", with and without circles_along_traj;
  (c) the route a caller had before, for 64 envs: tape to the host, trajectory.episodes, one matplotlib Agg figure per
      env drawn by the rules of DESIGN.md section 13 (skipped with a note where matplotlib is absent).

Every line carries the bytes the kernel must write (3 H W per frame) and the rate that makes.  One JSON line on stdout.

    python profiles/render_cost.py [--envs 4096] [--blocks 7] [--reps 5]
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
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls per timed block")
    args = ap.parse_args()
    import torch
    from gym_collision_avoidance_amd import _native as nat, build_native as bn, core, trajectory
    E, N = args.envs, 10
    table = np.load(os.path.join(REPO, "gym_collision_avoidance_amd", "data", "test_cases.npz"))["n10"]
    dev = torch.device("cuda", 0)
    s = core.BatchedSim(core.make_params(E, N), device=dev)
    s.set_plugins(nat.POL_RVO)
    s.set_fixture_table(table)
    s.reset_from_table()
    s.record_trajectories(max_bytes=8 << 30)
    steps = 0
    while steps < 400 and int((s.state["reset_count"] > 0).sum()) < 0.9 * E:     # until most envs have a finished episode
        s.rollout(50)
        steps += 50
    finished = int((s.state["reset_count"] > 0).sum())

    def timed(fn):
        fn()
        fn()                                  # warm-up: code objects, allocator
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(args.blocks):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.reps):
                r = fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / args.reps)
        return float(np.median(out)), r

    res = {"what": "render cost, us per call (median of %d blocks of %d calls, HIP events)" % (args.blocks, args.reps),
           "envs": E, "agents": N, "tape_steps": steps, "envs_with_a_finished_episode": finished,
           "lib_sha256": bn.file_sha256(nat.LIB_PATH)}

    def line(us, frames):
        F, H, W = frames.shape[:3]
        return {"us": round(us, 1), "frames": F, "us_per_frame": round(us / F, 3), "bytes_out": 3 * H * W * F,
                "GB_per_s_out": round(3 * H * W * F / us / 1e3, 2)}

    e = int(torch.argmax(s.state["reset_count"]))
    for size in ((128, 128), (800, 1000)):
        us, fr = timed(lambda: s.render_episode(e, episode="last", size=size))
        res["a_render_episode_%dx%d" % (size[1], size[0])] = line(us, fr)
    for circles in (True, False):
        us, fr = timed(lambda: s.render_frames(size=(64, 64), episode="last", circles_along_traj=circles))
        res["b_render_frames_64x64_%s" % ("circles" if circles else "dots")] = line(us, fr)
    s.check_faults()

    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        res["c_host_route_64_envs"] = "skipped: matplotlib is not installed"
    else:
        from gym_collision_avoidance_amd import render as rd
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        tp = s.trajectories()
        rows, ep, epoch = tp["rows"][:, :64].cpu(), tp["episode"][:, :64].cpu(), tp["epoch"][:, :64].cpu()
        t1 = time.perf_counter()
        for env in range(64):
            eps = trajectory.episodes(rows, ep, env, epoch=epoch)
            agents = eps[-2] if len(eps) > 1 else eps[-1]
            fig = plt.figure(0, figsize=(0.64, 0.64), dpi=100)
            plt.clf()
            ax = fig.add_axes([0, 0, 1, 1])
            for i, h in enumerate(agents):
                if len(h):
                    c = rd.PALETTE[i % 7]
                    ax.plot(h[:, 1], h[:, 2], color=c, linewidth=2)
                    for j in range(0, len(h), 4):
                        ax.add_patch(plt.Circle(h[j, 1:3], radius=h[j, 5], fc=c, ec=c))
            ax.set_xlim(-8, 8)
            ax.set_ylim(-8, 8)
            ax.axis("off")
            fig.canvas.draw()
            np.asarray(fig.canvas.buffer_rgba())
        t2 = time.perf_counter()
        res["c_host_route_64_envs"] = {"tape_to_host_ms": round((t1 - t0) * 1e3, 1), "figures_ms": round((t2 - t1) * 1e3, 1),
                                       "ms_per_env": round((t2 - t0) * 1e3 / 64, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
