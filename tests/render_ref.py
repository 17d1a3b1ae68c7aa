"""tests/render_ref.py -- the drawing rules of DESIGN.md section 13 in NumPy: what a rendered frame must be, bit for bit.

Not a test and independent of the package (it imports nothing of it): tests/test_render_golden.py compares its pictures
with the reference's matplotlib canvases, tests/test_gpu_render.py compares the device kernel with it byte by byte.

A frame is uint8 [H, W, 3].  Pixel (r, c) has its centre at the 1/16-pixel integer point (16 c + 8, 16 r + 8); a world
point becomes (floor((x - xmin) * s16), floor((ymax - y) * s16)), saturated at +-2^20, a radius floor(radius * s16); every
inside test below is int64 arithmetic on those.  Floating point appears only in single roundings (one subtraction, one
multiplication, one division at a time): nothing a fused multiply-add could change.
"""
import numpy as np

PALETTE8 = ((217, 83, 25), (0, 114, 189), (119, 172, 48), (126, 47, 142), (237, 177, 32), (77, 190, 238), (162, 20, 47))
WHITE, WALL = (255, 255, 255), (80, 80, 80)
LIM = 1 << 20
HALF_WIDTH, RIM = 24, 8           # 3-pixel polylines; the rim straddles the radius by half a pixel
DEFAULT_LIMITS = ((-8.0, 8.0), (-8.0, 8.0))


def window(size, limits=None):
    """(H, W), ((xmin, xmax), (ymin, ymax)) -> xmin, ymax, s16 of the frame: equal scale on both axes, the largest at
    which the limits fit, the limits' centre in the middle of the frame"""
    H, W = int(size[0]), int(size[1])
    (x0, x1), (y0, y1) = DEFAULT_LIMITS if limits is None else limits
    x0, x1, y0, y1 = float(x0), float(x1), float(y0), float(y1)
    ppm = min(W / (x1 - x0), H / (y1 - y0))
    return (x0 + x1) / 2 - W / (2 * ppm), (y0 + y1) / 2 + H / (2 * ppm), 16 * ppm


def marker_sizes(H, W):
    """goal diamond half extent, dot radius (1/16 pixel): the reference's 28-pixel star / 10.4-pixel scatter dot (6 pt across plus its 1.5 pt edge) on the
    770-pixel axes of its 1000-pixel canvas (a frame has no margins: it is the axes rectangle), scaled with the frame's
    longer side, at least 2 / 1 pixels"""
    u = max(H, W)
    return max(32, (291 * u) // 1000), max(16, (108 * u) // 1000)


def _fix(v):
    f = np.floor(np.float64(v))
    if not f >= -LIM:          # (NaN too)
        return -LIM
    return int(min(f, LIM))


def _blend(c, a8):
    return tuple((ch * a8 + 255 * (255 - a8) + 127) // 255 for ch in c)


def alpha8(t, max_time):
    q = np.float64(t) / (np.float64(1.2) * np.float64(max_time))
    if not q >= 0.0:
        q = 0.0
    if q > 1.0:
        q = 1.0
    return 255 - int(np.floor(np.float64(q) * np.float64(255.0)))


def circle_rows(times, n=None):
    """indices of the rows that carry a disc: nearest row (first minimum) to each of arange(0, t_last, 0.4) -- at most
    one time per row --, then the last row"""
    times = np.asarray(times, np.float64)
    n = len(times)
    x = times[-1] / np.float64(0.4)
    nk = int(min(np.ceil(x), n)) if x > 0 else 0
    out = []
    for k in range(nk):
        d = np.abs(times - np.float64(k) * np.float64(0.4))
        out.append(int(np.argmin(d)))
    return out + [n - 1]


def primitives(agents, xmin, ymax, s16, H, W, circles=True, snapshot=False):
    """agents: per slot None (absent / no rows) or, for a history frame, a float64 [n >= 1, 6+] array of rows
    (t, px, py, gx, gy, radius, ...); for a snapshot frame (px, py, gx, gy, radius).  -> the draw list."""
    g16, d16 = marker_sizes(H, W)
    fx = lambda x: _fix((np.float64(x) - np.float64(xmin)) * np.float64(s16))
    fy = lambda y: _fix((np.float64(ymax) - np.float64(y)) * np.float64(s16))
    fr = lambda r: max(_fix(np.float64(r) * np.float64(s16)), 0)
    discs, segs, marks = [], [], []
    if snapshot:
        for i, a in enumerate(agents):
            if a is None:
                continue
            c = PALETTE8[i % 7]
            discs.append(("disc", fx(a[0]), fy(a[1]), fr(a[4]), c, c))
            marks.append(("mark", fx(a[2]), fy(a[3]), g16, c))
        return discs + marks
    live = [a for a in agents if a is not None and len(a)]
    max_time = max([1e-4] + [float(a[-1, 0]) for a in live if a[-1, 0] > 1e-4])
    for i, a in enumerate(agents):
        if a is None or not len(a):
            continue
        c = PALETTE8[i % 7]
        n = len(a)
        if circles:
            for j in circle_rows(a[:, 0]):
                discs.append(("disc", fx(a[j, 1]), fy(a[j, 2]), fr(a[j, 5]), _blend(c, alpha8(a[j, 0], max_time)), c))
            for j in range(1, n):
                segs.append(("seg", fx(a[j - 1, 1]), fy(a[j - 1, 2]), fx(a[j, 1]), fy(a[j, 2]), c))
            marks.append(("mark", fx(a[0, 3]), fy(a[0, 4]), g16, c))
        else:
            for j in range(n):
                a8 = 51 + (204 * j) // (n - 1) if n > 1 else 51
                discs.append(("dot", fx(a[j, 1]), fy(a[j, 2]), d16, _blend(c, a8)))
            discs.append(("disc", fx(a[-1, 1]), fy(a[-1, 2]), fr(a[-1, 5]), _blend(c, 179), c))
    return discs + segs + marks


def background(H, W, xmin, ymax, s16, grid=None, cell=0.1):
    """white, dark grey where the pixel centre falls in an occupied cell of the bool grid [rows, cols] (Map.py:26-32 with
    the map centred on the origin)"""
    img = np.empty((H, W, 3), np.uint8)
    img[:] = WHITE
    if grid is None:
        return img
    grid = np.asarray(grid, bool)
    rows, cols = grid.shape
    cell = np.float64(cell)
    origin_r, origin_c = (rows * cell / 2.) / cell, (cols * cell / 2.) / cell
    y = np.float64(ymax) - (16 * np.arange(H) + 8).astype(np.float64) / np.float64(s16)
    x = np.float64(xmin) + (16 * np.arange(W) + 8).astype(np.float64) / np.float64(s16)
    mr, mc = np.floor(origin_r - y / cell), np.floor(origin_c + x / cell)
    okr, okc = (mr >= 0) & (mr < rows), (mc >= 0) & (mc < cols)
    ri, ci = np.where(okr, mr, 0).astype(np.int64), np.where(okc, mc, 0).astype(np.int64)
    occ = grid[ri[:, None], ci[None, :]] & okr[:, None] & okc[None, :]
    img[occ] = WALL
    return img


def draw(img, prims):
    """draws the list onto img in order (later covers earlier)"""
    H, W = img.shape[:2]
    for p in prims:
        kind = p[0]
        if kind == "seg":
            _, x1, y1, x2, y2, c = p
            ext = HALF_WIDTH
            bx0, bx1, by0, by1 = min(x1, x2) - ext, max(x1, x2) + ext, min(y1, y2) - ext, max(y1, y2) + ext
        else:
            x1, y1, R = p[1], p[2], p[3]
            ext = R + (RIM if kind == "disc" else 0)
            bx0, bx1, by0, by1 = x1 - ext, x1 + ext, y1 - ext, y1 + ext
        # pixels whose centre 16 i + 8 may lie in the box
        c0, c1 = max(0, (bx0 - 8) // 16), min(W - 1, (bx1 - 8) // 16 + 1)
        r0, r1 = max(0, (by0 - 8) // 16), min(H - 1, (by1 - 8) // 16 + 1)
        if c0 > c1 or r0 > r1:
            continue
        px = (16 * np.arange(c0, c1 + 1, dtype=np.int64) + 8)[None, :]
        py = (16 * np.arange(r0, r1 + 1, dtype=np.int64) + 8)[:, None]
        dx, dy = px - x1, py - y1
        sub = img[r0:r1 + 1, c0:c1 + 1]
        if kind == "seg":
            ex, ey = x2 - x1, y2 - y1
            tt, L2 = dx * ex + dy * ey, ex * ex + ey * ey
            fx_, fy_ = px - x2, py - y2
            cr = np.minimum(np.abs(dx * ey - dy * ex), 1 << 27)
            inside = np.where(tt <= 0, dx * dx + dy * dy <= HALF_WIDTH ** 2,
                              np.where(tt >= L2, fx_ * fx_ + fy_ * fy_ <= HALF_WIDTH ** 2, cr * cr <= HALF_WIDTH ** 2 * L2))
            sub[inside] = c
        elif kind == "mark":
            sub[(np.abs(dx) + np.abs(dy)) <= R] = p[4]
        elif kind == "dot":
            sub[(dx * dx + dy * dy) <= R * R] = p[4]
        else:
            d2 = dx * dx + dy * dy
            inside = d2 <= (R + RIM) ** 2
            fill = inside & (d2 <= (R - RIM) ** 2) if R >= RIM else np.zeros_like(inside)
            sub[inside & ~fill] = p[5]
            sub[fill] = p[4]
    return img


def render(size, limits, agents, circles=True, snapshot=False, grid=None, cell=0.1):
    """one frame; see primitives() for `agents`"""
    H, W = int(size[0]), int(size[1])
    xmin, ymax, s16 = window(size, limits)
    img = background(H, W, xmin, ymax, s16, grid, cell)
    return draw(img, primitives(agents, xmin, ymax, s16, H, W, circles, snapshot))
