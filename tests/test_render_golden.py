"""The drawing rules (tests/render_ref.py) against the reference's own pictures: the canvases that
tests/record_render_golden.py recorded from the unmodified visualize.plot_episode under matplotlib's Agg backend
(tests/golden/render_ref.npz).  CPU only.

The spec rasteriser draws every scene into the pixel grid of the recorded axes rectangle (one pixel inside it: the spines
stay out) from the recorded histories; the boxes of the reference's time labels and goal stars -- the stated divergences --
are masked out.  Two figures per scene:
  mismatch  the share of unmasked pixels whose largest channel difference exceeds 32 / 255;
  ink IoU   intersection over union of the "ink" (pixels more than 32 / 255 away from white in some channel).
What remains once labels and stars are masked is the reference's anti-aliasing: its 1 pt (1.4 pixel) rims and 2 pt (2.8 pixel)
lines cover their edge pixels partly, ours (1 and 3 pixels) wholly or not at all -- every differing pixel lies on a rim or
along a line's edge.  Measured on the committed fixture with the rules as they stand (profiles/render.md):
  swap2 0.6149 % / 0.9830, cross4 0.8768 % / 0.9827, lanes10 1.0044 % / 0.9483, cross4_dots 0.5255 % / 0.9760
(mismatch / IoU; with NOTHING masked a trial rasteriser had 2.8 % / 0.93).  The bounds are the worst scene's value plus a
quarter of it: mismatch <= 1.2555 %, 1 - IoU <= 0.0646.  lanes10 sets both (one of its agents circles in place for 16 s:
some 40 overlapping rims in a few hundred pixels), which leaves the other scenes slack; so each scene is ALSO held to its own
figures plus a quarter (SCENE_BOUNDS), which is the tighter check for every scene but lanes10."""
import os

import numpy as np
import pytest

from tests import render_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_ref.npz")
MAX_MISMATCH = 0.012555   # 1.25 x 1.0044 % (lanes10)
MIN_IOU = 1.0 - 0.0646    # 1.25 x (1 - 0.9483) (lanes10)
MAX_MASKED = 0.20
# per scene: (mismatch, 1 - IoU), each 1.25 x the scene's own measured figure above
SCENE_BOUNDS = {"swap2": (1.25 * 0.006149, 1.25 * 0.0170), "cross4": (1.25 * 0.008768, 1.25 * 0.0173),
                "lanes10": (1.25 * 0.010044, 1.25 * 0.0517), "cross4_dots": (1.25 * 0.005255, 1.25 * 0.0240)}


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLD) as z:
        return {k: z[k] for k in z.files}


def _scene(gold, si):
    p = "s%d_" % si
    hist, steps = gold[p + "history"], gold[p + "step_num"]
    agents = []
    for i in range(hist.shape[0]):
        rows = hist[i, :steps[i], :6].copy()
        rows[:, 5] = gold[p + "radius"][i]          # (the reference draws agent.radius; the history's column is the same number)
        agents.append(rows if len(rows) else None)
    return agents, bool(gold[p + "circles"])


def _compare(gold, si):
    """-> mismatch share, ink IoU, masked share of the scene"""
    p = "s%d_" % si
    canvas, rect, win, boxes = gold[p + "canvas"], gold[p + "axes_rect"], gold[p + "window"], gold[p + "boxes"]
    agents, circles = _scene(gold, si)
    r0, r1 = int(np.ceil(rect[0])) + 1, int(np.floor(rect[1])) - 1
    c0, c1 = int(np.ceil(rect[2])) + 1, int(np.floor(rect[3])) - 1
    ppm = (rect[3] - rect[2]) / (win[1] - win[0])
    assert abs(ppm - (rect[1] - rect[0]) / (win[3] - win[2])) < 1e-9 * ppm      # equal aspect
    # canvas pixel (r, c) covers [c, c + 1) x [r, r + 1) of the display: the frame's pixel grid IS the canvas's
    xmin, ymax, s16 = win[0] + (c0 - rect[2]) / ppm, win[3] - (r0 - rect[0]) / ppm, 16 * ppm
    H, W = r1 - r0, c1 - c0
    img = R.draw(R.background(H, W, xmin, ymax, s16), R.primitives(agents, xmin, ymax, s16, H, W, circles))
    ref = canvas[r0:r1, c0:c1].astype(np.int32)
    mask = np.zeros(canvas.shape[:2], bool)
    for b in boxes:
        mask[max(0, int(np.floor(b[0])) - 1):int(np.ceil(b[1])) + 1, max(0, int(np.floor(b[2])) - 1):int(np.ceil(b[3])) + 1] = True
    mask = mask[r0:r1, c0:c1]
    keep = ~mask
    diff = np.abs(img.astype(np.int32) - ref).max(axis=-1)
    ink_a, ink_b = (255 - img.astype(np.int32)).max(axis=-1) > 32, (255 - ref).max(axis=-1) > 32
    union = ((ink_a | ink_b) & keep).sum()
    return (diff > 32)[keep].mean(), ((ink_a & ink_b) & keep).sum() / max(1, union), mask.mean()


def test_spec_matches_the_reference_canvases(gold):
    n = len(gold["names"])
    assert n >= 4
    figures = []
    for si in range(n):
        mis, iou, masked = _compare(gold, si)
        print("%-12s mismatch %.4f %%  ink IoU %.4f  masked %.3f" % (gold["names"][si], 100 * mis, iou, masked))
        figures.append((mis, iou, masked))
    for (mis, iou, masked), name in zip(figures, gold["names"]):
        assert masked <= MAX_MASKED, (name, masked)
        assert mis <= MAX_MISMATCH, (name, mis)
        assert iou >= MIN_IOU, (name, iou)
        own_mis, own_loss = SCENE_BOUNDS[str(name)]
        assert mis <= own_mis and 1.0 - iou <= own_loss, (name, mis, iou)


def test_scenes_cover_what_the_issue_names(gold):
    names = list(gold["names"])
    counts = [gold["s%d_history" % i].shape[0] for i in range(len(names))]
    assert 2 in counts and 4 in counts and 10 in counts
    assert any(not bool(gold["s%d_circles" % i]) for i in range(len(names)))
    assert os.path.getsize(GOLD) < 1 << 20


def test_palette_is_the_recorded_palette(gold):
    from gym_collision_avoidance_amd import render as rd
    assert np.array_equal(np.array(rd.PALETTE), gold["palette"])
    want = np.floor(gold["palette"] * 255 + 0.5).astype(int)
    assert np.array_equal(np.array(rd.PALETTE8), want) and np.array_equal(np.array(R.PALETTE8), want)


def test_disc_rows_are_the_reference_find_nearest_picks(gold):
    """util.find_nearest over arange(0, t_last, 0.4), restated: tile, abs, argmin"""
    checked = 0
    for si in range(len(gold["names"])):
        hist, steps = gold["s%d_history" % si], gold["s%d_step_num" % si]
        for i in range(hist.shape[0]):
            t = hist[i, :steps[i], 0]
            times = np.arange(0.0, t[-1], 0.4)
            tiled = np.tile(np.expand_dims(times, axis=0).transpose(), (1, t.shape[0]))
            idx = np.abs(t - tiled).argmin(axis=1)
            assert R.circle_rows(t) == list(idx) + [len(t) - 1]
            checked += len(idx)
    assert checked > 50
