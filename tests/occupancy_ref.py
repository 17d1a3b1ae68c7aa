"""CPU restatement of the OccupancyGridSensor contract in numpy -- the ground truth of tests/test_occupancy_golden.py (which
pins it to windows recorded from the unmodified reference, tests/golden/occgrid.npz) and of tests/test_gpu_occupancy.py.

  dynamic map  = static grid OR a disc per agent (reference Map.add_agents_to_map, Map.py:46-64): agent cell
                 (gr, gc) = (floor(origin_r - py / cell), floor(origin_c + px / cell)); inside the grid -> every cell with
                 (c - gc)^2 + (r - gr)^2 < (radius / cell)^2 is set; outside -> the agent paints nothing;
  window of n  = H x W cells anchored at i0 = floor(origin_r - (py + y_width / 2.) / cell),
                 j0 = floor(origin_c + (px - x_width / 2.) / cell): out[a, b] = dyn[i0 + a, j0 + b], 0 outside the map.
Everything is float64 with true divisions, as numpy evaluates the reference's expressions."""
import numpy as np


def dynamic_map(static, px, py, radius, cell=0.1, origin=None):
    """static: bool [rows, cols]; px, py, radius: [N] -> the dynamic map, bool [rows, cols]"""
    static = np.asarray(static, dtype=bool)
    rows, cols = static.shape
    origin_r, origin_c = (rows * cell / 2.) / cell, (cols * cell / 2.) / cell
    if origin is not None:
        origin_r, origin_c = origin
    dyn = static.copy()
    x = np.arange(0, cols)
    y = np.arange(0, rows)
    for ax, ay, ar in zip(np.asarray(px, np.float64), np.asarray(py, np.float64), np.asarray(radius, np.float64)):
        if not (np.isfinite(ax) and np.isfinite(ay)):
            continue
        gr = int(np.floor(origin_r - ay / cell))
        gc = int(np.floor(origin_c + ax / cell))
        if gr >= 0 and gc >= 0 and gr < rows and gc < cols:
            dyn |= (x[np.newaxis, :] - gc) ** 2 + (y[:, np.newaxis] - gr) ** 2 < (ar / cell) ** 2
    return dyn


def anchor(px, py, rows, cols, cell=0.1, x_width=5., y_width=5.):
    origin_r, origin_c = (rows * cell / 2.) / cell, (cols * cell / 2.) / cell
    i0 = int(np.floor(origin_r - (np.float64(py) + y_width / 2.) / cell))
    j0 = int(np.floor(origin_c + (np.float64(px) - x_width / 2.) / cell))
    return i0, j0


def crop(dyn, px, py, cell=0.1, x_width=5., y_width=5.):
    """one agent's window of the dynamic map `dyn`: bool [H, W]"""
    rows, cols = dyn.shape
    H, W = int(y_width / cell), int(x_width / cell)
    i0, j0 = anchor(px, py, rows, cols, cell, x_width, y_width)
    out = np.zeros((H, W), dtype=bool)
    a0, a1 = max(0, -i0), min(H, rows - i0)   # window rows that exist in the map
    b0, b1 = max(0, -j0), min(W, cols - j0)
    if a1 > a0 and b1 > b0:
        out[a0:a1, b0:b1] = dyn[i0 + a0:i0 + a1, j0 + b0:j0 + b1]
    return out


def occupancy(static, px, py, radius, cell=0.1, x_width=5., y_width=5.):
    """every agent's window of one env: bool [N, H, W] (absent slots of a ragged batch have radius 0: they paint nothing
    but still get a window)"""
    dyn = dynamic_map(static, px, py, radius, cell)
    return np.stack([crop(dyn, ax, ay, cell, x_width, y_width) for ax, ay in zip(px, py)])


def occupancy_batch(static, px, py, radius, env_map=None, **kw):
    """[E, N] state arrays -> bool [E, N, H, W]; static: one grid [rows, cols], or a stack [M, rows, cols] with env_map [E]
    (an index outside [0, M): the empty grid)"""
    static = np.asarray(static, dtype=bool)
    out = []
    for e in range(px.shape[0]):
        if static.ndim == 3:
            m = int(env_map[e])
            grid = static[m] if 0 <= m < static.shape[0] else np.zeros(static.shape[1:], dtype=bool)
        else:
            grid = static
        out.append(occupancy(grid, px[e], py[e], radius[e], **kw))
    return np.stack(out)


def pack_rows(cells):
    """bool [..., W] -> uint32 [..., (W + 31) // 32]: cell b of a row = bit b & 31 of word b >> 5"""
    cells = np.asarray(cells, dtype=bool)
    W = cells.shape[-1]
    WW = (W + 31) // 32
    pad = np.zeros(cells.shape[:-1] + (WW * 32,), dtype=np.uint8)
    pad[..., :W] = cells
    return np.packbits(pad.reshape(cells.shape[:-1] + (WW, 32)), axis=-1, bitorder="little").view(np.uint32)[..., 0]
