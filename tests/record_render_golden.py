#!/usr/bin/env python3
"""tests/record_render_golden.py -- RECORDER, not a test (no test imports it).  Runs the UNMODIFIED reference's
visualize.plot_episode (envs/visualize.py:90-257) under matplotlib's Agg backend on episodes of the reference's own env
stepping RVO agents, and writes tests/golden/render_ref.npz.  It works only where the reference checkout is present
(CA_REFERENCE_ROOT, default /root/reference), matplotlib is installed and `build()` has made oracle/_build/rvo2*.so; its
output is committed.

How the reference is made to run (nothing of it is modified or copied): oracle/stubs (gym / imageio / tensorflow stand-ins)
and the reference are put on sys.path, the Config singleton is selected through GYM_CONFIG_PATH / GYM_CONFIG_CLASS
(oracle/golden_configs.py Bench10) and its STORE_HISTORY attribute is switched on from outside, so that the agents keep
their global_state_history.

Scenes (fixed limits, the reference's own 10 x 8 in figure at 100 dpi = a 1000 x 800 canvas, on which its size-24 time
labels leave most of the picture uncovered): a 2-agent swap, a 4-agent crossing, 10 agents in interleaved
lanes, and the 4-agent crossing again with circles_along_traj=False.  Recorded per scene: the canvas RGB, the axes
rectangle in canvas pixels (row 0 at the top) and the data window it shows, every agent's global_state_history[:step_num]
and radius, the pixel boxes (get_window_extent) of every text label and goal star, and the palette.  The boxes may cover at
most 20 % of the axes rectangle (asserted here and again by the test)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = os.environ.get("CA_REFERENCE_ROOT", "/root/reference")
OUT = os.path.join(HERE, "golden", "render_ref.npz")
FIG_SIZE, DPI = (10, 8), 100
MAX_STEPS = 300


def main():
    os.environ["GYM_CONFIG_PATH"] = os.path.join(REPO, "oracle", "golden_configs.py")
    os.environ["GYM_CONFIG_CLASS"] = "Bench10"
    os.environ["MPLBACKEND"] = "Agg"
    sys.path[:0] = [os.path.join(REPO, "oracle", "stubs"), os.path.join(REPO, "oracle", "_build"), REF]
    import warnings
    warnings.filterwarnings("ignore")
    import rvo2  # noqa: F401  (the oracle's module; fail early if build() has not made it)
    import matplotlib
    import matplotlib.pyplot as plt
    from matplotlib.lines import Line2D
    from matplotlib.text import Text
    from gym_collision_avoidance.envs import Config
    Config.STORE_HISTORY = True
    from gym_collision_avoidance.envs import test_cases as tc
    from gym_collision_avoidance.envs import visualize
    from gym_collision_avoidance.envs.agent import Agent
    from gym_collision_avoidance.envs.collision_avoidance_env import CollisionAvoidanceEnv
    from gym_collision_avoidance.envs.dynamics.UnicycleDynamics import UnicycleDynamics
    from gym_collision_avoidance.envs.sensors.OtherAgentsStatesSensor import OtherAgentsStatesSensor
    matplotlib.rcParams["figure.dpi"] = DPI

    f = np.float64

    def mk(px, py, gx, gy, r, ps, i):
        h = np.arctan2(f(gy) - f(py), f(gx) - f(px))
        return Agent(f(px), f(py), f(gx), f(gy), f(r), f(ps), h, tc.policy_dict["RVO"], UnicycleDynamics,
                     [OtherAgentsStatesSensor], i)

    # ten agents in interleaved lanes, alternately east- and westbound, each drifting one lane sideways
    lanes = [((-2.2 if k % 2 == 0 else 2.2), -3.4 + 0.75 * k) for k in range(10)]
    scenes = [
        ("swap2", True, ((-5.0, 5.0), (-4.0, 4.0)),
         [(-3.5, 0.1, 3.5, 0.0, 0.5, 1.0), (3.5, -0.1, -3.5, 0.0, 0.4, 1.2)]),
        ("cross4", True, ((-6.0, 6.0), (-4.8, 4.8)),
         [(-4.0, 0.3, 4.0, 0.0, 0.5, 1.0), (4.0, -0.2, -4.0, 0.3, 0.4, 1.1), (1.5, -4.0, -1.0, 4.0, 0.45, 0.9),
          (-0.3, 4.0, 0.2, -4.0, 0.35, 1.3)]),
        ("lanes10", True, ((-5.0, 5.0), (-4.0, 4.0)),
         [(x, y, -x, y + (0.75 if k % 4 < 2 else -0.75), 0.2 + 0.01 * k, 1.8 + 0.04 * k) for k, (x, y) in enumerate(lanes)]),
        ("cross4_dots", False, ((-6.0, 6.0), (-4.8, 4.8)),
         [(-4.0, 0.3, 4.0, 0.0, 0.5, 1.0), (4.0, -0.2, -4.0, 0.3, 0.4, 1.1), (1.5, -4.0, -1.0, 4.0, 0.45, 0.9),
          (-0.3, 4.0, 0.2, -4.0, 0.35, 1.3)]),
    ]
    import tempfile
    scratch_dir = tempfile.mkdtemp(prefix="render_golden_")
    out = {"palette": np.array(visualize.plt_colors, dtype=np.float64), "names": np.array([s[0] for s in scenes])}
    for si, (name, circles, limits, spec) in enumerate(scenes):
        agents = [mk(*row, i) for i, row in enumerate(spec)]
        env = CollisionAvoidanceEnv()
        env.set_agents(agents)
        env.reset()
        for _ in range(MAX_STEPS):
            _, _, over, _, _ = env.step({})
            if over:
                break
        visualize.plot_episode(env.agents, True, env_map=None, test_case_index=si, env_id=si, circles_along_traj=circles,
                               plot_save_dir=scratch_dir + "/",   # (plot_episode makes its sub-directories even when it saves nothing)
                               plot_policy_name="RVO", limits=limits, fig_size=FIG_SIZE, show=False, save=False)
        fig = plt.figure(si)
        fig.set_dpi(DPI)
        fig.canvas.draw()
        rgb = np.asarray(fig.canvas.buffer_rgba())[..., :3].copy()
        Hc, Wc = rgb.shape[:2]
        ax = fig.axes[0]
        rend = fig.canvas.get_renderer()
        bb = ax.get_window_extent(rend)                       # display pixels, y up
        rect = np.array([Hc - bb.y1, Hc - bb.y0, bb.x0, bb.x1])      # rows top / bottom, columns left / right
        # the data window the axes rectangle shows (set_aspect('equal') may have changed the limits asked for)
        win = np.array(list(ax.get_xlim()) + list(ax.get_ylim()), dtype=np.float64)
        boxes = []
        for art in list(ax.texts) + [ln for ln in ax.lines if ln.get_marker() == "*"]:
            assert isinstance(art, (Text, Line2D))
            b = art.get_window_extent(rend)
            if isinstance(art, Line2D):                       # (a Line2D's extent is its data point: add the marker's size)
                half = art.get_markersize() * DPI / 72.0 / 2.0 + 1.0
                b = b.expanded(1.0, 1.0)
                b = type(b).from_extents(b.x0 - half, b.y0 - half, b.x1 + half, b.y1 + half)
            boxes.append([Hc - b.y1, Hc - b.y0, b.x0, b.x1])
        boxes = np.array(boxes, dtype=np.float64).reshape(-1, 4)
        mask = np.zeros((Hc, Wc), bool)
        for r0, r1, c0, c1 in boxes:
            mask[max(0, int(np.floor(r0)) - 1):int(np.ceil(r1)) + 1, max(0, int(np.floor(c0)) - 1):int(np.ceil(c1)) + 1] = True
        r0, r1, c0, c1 = int(np.ceil(rect[0])), int(np.floor(rect[1])), int(np.ceil(rect[2])), int(np.floor(rect[3]))
        share = mask[r0:r1, c0:c1].mean()
        print("%s: canvas %dx%d, axes rows %.1f..%.1f cols %.1f..%.1f, window %s, %d agents, %d boxes, masked share %.3f"
              % (name, Wc, Hc, rect[0], rect[1], rect[2], rect[3], win, len(agents), len(boxes), share))
        assert share <= 0.20, "%s: the label / star boxes cover %.1f %% of the axes rectangle (cap: 20 %%)" % (name, 100 * share)
        p = "s%d_" % si
        out[p + "canvas"], out[p + "axes_rect"], out[p + "window"], out[p + "boxes"] = rgb, rect, win, boxes
        out[p + "circles"] = np.array(circles)
        out[p + "radius"] = np.array([a.radius for a in env.agents], dtype=np.float64)
        out[p + "step_num"] = np.array([a.step_num for a in env.agents], dtype=np.int64)
        hist = np.zeros((len(agents), max(a.step_num for a in env.agents), env.agents[0].global_state_history.shape[1]))
        for i, a in enumerate(env.agents):
            hist[i, :a.step_num] = a.global_state_history[:a.step_num]
        out[p + "history"] = hist
        plt.close(fig)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print("%s: %d scenes, %d bytes" % (OUT, len(scenes), os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()
