"""CPU restatement of the LaserScanSensor contract (include/cagpu.h CaMap / CaScan) in plain float64 numpy -- the judge of
tests/test_gpu_laserscan_edges.py, pinned by tests/test_laserscan_ref_host.py to the episode recorded from the unmodified
reference (tests/golden/laser4.npz) and cross-checked against the C++ oracle before it judges anything.

  cell of (x, y) = (floor(origin_r - y / cell), floor(origin_c + x / cell)), origin = ((rows * cell / 2.) / cell,
                   (cols * cell / 2.) / cell), true divisions throughout;
  dynamic map    = static grid OR, for every agent whose cell lies in the grid, the cells with
                   (c - gc)^2 + (r - gr)^2 < (radius / cell)^2; an agent outside the grid paints nothing;
  beam b         = direction heading + linspace(min_angle, max_angle, B)[b], samples at arange(0, max_range, range_res);
                   a sample hits when its cell is in the grid, occupied in the dynamic map and not under the agent's OWN
                   disc (which exists only when the agent's cell is in the grid);
  range index    = the LAST sample whose running hit count is 1 (the sample before the second hit, or the last sample of
                   the beam when there is one hit only); 255 when nothing is hit;
  history        = the first measurement of an episode fills every row, later ones roll the rows down by one and write row 0.

`variant` (scan_indices / decided) and `wrong_way` (roll_history) switch on ONE deliberate mistake each; the host test uses
them to show that every scene of the GPU test tells the right answer from that mistake.  Nothing else may pass them."""
import itertools

import numpy as np

NOTHING = 255
# the kernel's error on the direction cosines (csrc/cagpu_scan.inc: sin / cos of heading + angle by the addition theorem,
# "2 ulp instead of 1"): absolute, 2 ulp of 1.0, for a heading other than 0; for heading == 0.0 the theorem's products are
# by exact 1 and 0, so only the difference of two libms remains: relative
ABS_TRIG_ERR = 4.5e-16
REL_TRIG_ERR = 1e-15


def origin(rows, cols, cell):
    return (rows * cell / 2.) / cell, (cols * cell / 2.) / cell


def cells(x, y, rows, cols, cell, variant=None):
    """world coordinates -> (row, col) as int64 arrays, and whether that cell is in the grid"""
    o_r, o_c = origin(rows, cols, cell)
    if variant == "reciprocal":      # the mistake: a multiplication by the rounded reciprocal instead of the division
        inv = 1.0 / cell
        gr, gc = np.floor(o_r - y * inv), np.floor(o_c + x * inv)
    else:
        gr, gc = np.floor(o_r - y / cell), np.floor(o_c + x / cell)
    gr, gc = gr.astype(np.int64), gc.astype(np.int64)
    return gr, gc, (gr >= 0) & (gc >= 0) & (gr < rows) & (gc < cols)


def _f64(*arrays):
    return [np.atleast_1d(np.asarray(a, np.float64)) for a in arrays]


def dynamic_map(static, px, py, radius, cell, present=None):
    """static: bool [rows, cols]; px, py, radius: [N]; present: bool [N] or None (everyone) -> bool [rows, cols]"""
    dyn = np.array(static, dtype=bool)
    rows, cols = dyn.shape
    px, py, radius = _f64(px, py, radius)
    gr, gc, inside = cells(px, py, rows, cols, cell)
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    for a in range(len(px)):
        if inside[a] and (present is None or present[a]):
            dyn |= (c - gc[a]) ** 2 + (r - gr[a]) ** 2 < (radius[a] / cell) ** 2
    return dyn


def trig_of(heading, num_beams, min_angle, max_angle):
    """(cos, sin) [N, B] of heading + beam angle, as numpy evaluates them"""
    ang = np.linspace(min_angle, max_angle, num_beams)[None, :] + _f64(heading)[0][:, None]
    return np.cos(ang), np.sin(ang)


def scan_indices(static, px, py, heading, radius, cell, num_beams, min_angle, max_angle, range_res, max_range, trig=None,
                 present=None, variant=None):
    """One env's newest scan row: uint8 [N, B], 255 = nothing hit.  trig = (cos, sin) [N, B] overrides the direction
    cosines; present: the agents that exist (the others paint nothing; their own rows are still computed)."""
    static = np.asarray(static, dtype=bool)
    rows, cols = static.shape
    px, py, heading, radius = _f64(px, py, heading, radius)
    dyn = dynamic_map(static, px, py, radius, cell, present)
    ranges = np.arange(0, max_range, range_res)
    cs, sn = trig_of(heading, num_beams, min_angle, max_angle) if trig is None else trig
    er, ec, ego_in = cells(px, py, rows, cols, cell)
    out = np.full((len(px), num_beams), NOTHING, np.uint8)
    for a in range(len(px)):
        x = px[a] + ranges[None, :] * cs[a][:, None]          # [B, R]
        y = py[a] + ranges[None, :] * sn[a][:, None]
        gr, gc, inside = cells(x, y, rows, cols, cell, variant)
        hit = inside & dyn[np.where(inside, gr, 0), np.where(inside, gc, 0)]
        if ego_in[a] and variant != "opaque":                 # (the mistake: the agent sees its own disc)
            hit &= ~((gc - ec[a]) ** 2 + (gr - er[a]) ** 2 < (radius[a] / cell) ** 2)
        if variant == "first":                                 # (the mistake: the first hit itself)
            pick = hit & (np.cumsum(hit, axis=1) == 1)
        else:
            pick = np.cumsum(hit, axis=1) == 1
        last = pick.shape[1] - 1 - np.argmax(pick[:, ::-1], axis=1)
        out[a] = np.where(pick.any(axis=1), last, NOTHING)
    return out


def decided(static, px, py, heading, radius, cell, num_beams, min_angle, max_angle, range_res, max_range, present=None,
            variant=None):
    """(indices, mask): mask [N, B] is True where the index stays the same while cos and sin move by the kernel's error
    bound in each of the 8 combinations of (-, 0, +) x (-, 0, +) other than (0, 0)."""
    px, py, heading, radius = _f64(px, py, heading, radius)
    args = (static, px, py, heading, radius, cell, num_beams, min_angle, max_angle, range_res, max_range)
    cs, sn = trig_of(heading, num_beams, min_angle, max_angle)
    base = scan_indices(*args, trig=(cs, sn), present=present, variant=variant)
    zero_heading = (heading == 0.0)[:, None]

    def moved(v, sign):
        exact = (v == 0.0) | (np.abs(v) == 1.0)
        rel = np.where(exact, v, v * (1.0 + sign * REL_TRIG_ERR))
        return np.where(zero_heading, rel, v + sign * ABS_TRIG_ERR)

    mask = np.ones(base.shape, bool)
    for s_c, s_s in itertools.product((-1, 0, 1), repeat=2):
        if s_c or s_s:
            mask &= scan_indices(*args, trig=(moved(cs, s_c), moved(sn, s_s)), present=present, variant=variant) == base
    return base, mask


def roll_history(hist, newest, first, wrong_way=False):
    """hist uint8 [N, H, B], newest [N, B], first bool [N] -> the history after this measurement (a new array)"""
    hist = np.asarray(hist)
    out = np.roll(hist, -1 if wrong_way else 1, axis=1)      # (wrong_way: the mistake)
    out[:, 0] = newest
    fill = np.asarray(first, bool)
    out[fill] = np.asarray(newest)[fill][:, None, :]
    return out


def ranges_of(idx, range_res, max_range):
    """the float32 observation of range indices: index * range_res, max_range for 255"""
    idx = np.asarray(idx)
    return np.where(idx == NOTHING, np.float32(max_range), (idx.astype(np.float64) * range_res).astype(np.float32))


def wall_hit(static, px, py, radius, cell):
    """bool [N]: the agent's cell is in the grid and its disc covers an occupied STATIC cell"""
    static = np.asarray(static, dtype=bool)
    rows, cols = static.shape
    px, py, radius = _f64(px, py, radius)
    gr, gc, inside = cells(px, py, rows, cols, cell)
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    out = np.zeros(len(px), bool)
    for a in range(len(px)):
        if inside[a]:
            out[a] = static[(c - gc[a]) ** 2 + (r - gr[a]) ** 2 < (radius[a] / cell) ** 2].any()
    return out
