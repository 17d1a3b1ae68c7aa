"""The scenes of tests/test_gpu_laserscan_edges.py, built in one place so that tests/test_laserscan_ref_host.py can examine
on the CPU exactly what the GPU file runs: the share of undecided beams of every scene, the discriminating power of the
lattice scenes, and that every scene tells the numpy reference from a deliberately wrong variant of it.  numpy only."""
import math

import numpy as np

from tests import laserscan_ref as lref


class Scene(object):
    """One batch: a geometry, a static grid (or a stack of them + env_map) and [E, N] agent states"""

    def __init__(self, name, static, cell, range_res, max_range, num_beams, min_angle, max_angle, px, py, heading, radius,
                 num_to_store=3, env_map=None, catches=()):
        self.name, self.static, self.cell = name, np.asarray(static, bool), float(cell)
        self.rows, self.cols = self.static.shape[-2:]
        self.range_res, self.max_range, self.num_beams = float(range_res), float(max_range), int(num_beams)
        self.min_angle, self.max_angle, self.num_to_store = float(min_angle), float(max_angle), int(num_to_store)
        self.px, self.py, self.heading, self.radius = (np.array(v, np.float64, ndmin=2) for v in (px, py, heading, radius))
        self.E, self.N = self.px.shape
        assert self.py.shape == self.heading.shape == self.radius.shape == (self.E, self.N)
        self.env_map = None if env_map is None else np.asarray(env_map, np.int64)
        assert (self.static.ndim == 3) == (self.env_map is not None)
        self.catches = tuple(catches)      # the wrong variants of the reference this scene is meant to catch
        self.num_ranges = len(np.arange(0, self.max_range, self.range_res))
        assert 1 <= self.num_ranges <= 255

    @property
    def ragged(self):
        return bool((self.radius == 0).any())

    def grid(self, e):
        return self.static if self.env_map is None else self.static[self.env_map[e]]

    def map_args(self):
        """keyword arguments of BatchedSim.set_map"""
        kw = dict(static_map=self.static, rows=self.rows, cols=self.cols, cell=self.cell, num_beams=self.num_beams,
                  num_to_store=self.num_to_store, max_range=self.max_range, range_res=self.range_res,
                  min_angle=self.min_angle, max_angle=self.max_angle)
        if self.env_map is not None:
            kw["env_map"] = self.env_map
        return kw

    def scan_args(self):
        """the geometry arguments of laserscan_ref.scan_indices / decided after (static, px, py, heading, radius)"""
        return (self.cell, self.num_beams, self.min_angle, self.max_angle, self.range_res, self.max_range)

    def cases(self):
        """case rows [E, N, 6] whose goals are the starts (nobody needs to move)"""
        c = np.zeros((self.E, self.N, 6))
        c[..., 0], c[..., 1], c[..., 2], c[..., 3], c[..., 4], c[..., 5] = self.px, self.py, self.px, self.py, 1.0, self.radius
        return c

    def decided(self, px=None, py=None, heading=None, radius=None, variant=None):
        """(indices, mask) uint8 / bool [E, N, B] of the given state (default: the scene's own); absent slots (radius 0)
        paint nothing and their own rows are masked out"""
        px, py, heading, radius = (getattr(self, n) if v is None else np.asarray(v, np.float64)
                                   for n, v in (("px", px), ("py", py), ("heading", heading), ("radius", radius)))
        idx = np.zeros((self.E, self.N, self.num_beams), np.uint8)
        mask = np.zeros(idx.shape, bool)
        for e in range(self.E):
            present = radius[e] > 0
            idx[e], mask[e] = lref.decided(self.grid(e), px[e], py[e], heading[e], radius[e], *self.scan_args(),
                                           present=present, variant=variant)
            mask[e] &= present[:, None]
        return idx, mask

    def shifted(self, d):
        """the same scene with every agent moved by d metres in x and y"""
        s = Scene.__new__(Scene)
        s.__dict__.update(self.__dict__)
        s.px, s.py = self.px + d, self.py + d
        return s


def _walls(rows, cols, rng=None, density=0.0):
    """a grid with a horizontal and a vertical wall line, a block and (optionally) scattered cells"""
    g = np.zeros((rows, cols), bool) if rng is None else rng.random((rows, cols)) < density
    g[rows // 8, cols // 16:cols - cols // 16] = True
    g[rows // 16:rows - rows // 16, cols - cols // 5] = True
    g[rows // 2 - 3:rows // 2 + 3, cols // 3:cols // 3 + 6] = True
    return g


# ---------------------------------------------------------------- a. the lattice: every axis-aligned sample on a cell border
def lattice(cell):
    """24 agents on multiples of `cell` (64 x 64 cells, range_res = cell), radii 1 .. 3 cells, every heading exactly 0.0,
    9 beams over [0, 2 pi]: beams 0, 2, 4, 6 and 8 run along the axes.  cell = 0.25: every quotient is exact;
    cell = 0.1: k * 0.1 is not, and the reference's float64 rounding decides every floor."""
    rng = np.random.default_rng(5)
    k = rng.integers(-30, 31, (2, 24))
    k[:, 0], k[:, 1], k[:, 2], k[:, 3] = (-32, 5), (32, -7), (3, 32), (-9, -32)    # exactly on the four map edges
    k[:, 4], k[:, 5] = (0, 0), (1, 0)                                                # the centre, and a neighbour inside its disc
    rad = rng.integers(1, 4, 24)
    rad[4] = 3
    return Scene("lattice_%g" % cell, _walls(64, 64), cell, cell, 30 * cell, 9, 0.0, 2 * math.pi,
                 k[0] * cell, k[1] * cell, np.zeros(24), rad * cell, num_to_store=2,
                 catches=("reciprocal",) if cell == 0.1 else ())


# ---------------------------------------------------------------- b. other geometries, random off-lattice scenes
def _random(name, seed, rows, cols, cell, range_res, max_range, num_beams, min_angle, max_angle, E=3, N=10, H=3, catches=()):
    rng = np.random.default_rng(seed)
    half_x, half_y = cols * cell / 2, rows * cell / 2
    px = rng.uniform(-half_x - 1.0, half_x + 1.0, (E, N))
    py = rng.uniform(-half_y - 1.0, half_y + 1.0, (E, N))
    heading = rng.uniform(-math.pi, math.pi, (E, N))
    radius = rng.uniform(2.0, 8.0, (E, N)) * cell
    return Scene(name, _walls(rows, cols, rng, 0.01), cell, range_res, max_range, num_beams, min_angle, max_angle,
                 px, py, heading, radius, num_to_store=H, catches=catches)


def geometries():
    return [
        _random("wide_72x100", 11, 72, 100, 0.25, 0.15, 7.0, 37, -math.pi, math.pi, catches=("opaque", "first")),
        _random("two_beams_40x33", 12, 40, 33, 0.1, 0.05, 3.0, 2, 0.0, math.pi / 3, H=1, N=24),
        _random("coarse_160x160", 13, 160, 160, 0.1, 0.3, 6.0, 64, -math.pi / 2, math.pi / 2, H=2),
        _random("ranges_255", 14, 60, 52, 0.1, 0.02, 5.1, 16, -math.pi / 2, math.pi / 2),
    ]


# ---------------------------------------------------------------- c. agents and the map edge (the reference's geometry)
def map_edge():
    """the 16 m x 16 m map of 0.1 m cells, 512 beams over +-pi/2, every off-map agent looking at the map"""
    rng = np.random.default_rng(21)
    rows = []     # (px, py, heading, radius)
    for k, (ux, uy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):          # right, left, above, below
        for d, lateral in ((1.0, -3.1), (5.0, 2.3), (6.5, 0.7)):               # 1 m, 5 m and beyond the laser's reach outside
            px, py = ux * (8.0 + d) + abs(uy) * lateral, uy * (8.0 + d) + abs(ux) * lateral
            rows.append((px, py, math.atan2(-uy, -ux) + 0.05 * (k + 1), 0.4))
    for px, py in ((8.0, 1.3), (-8.0, -2.2), (0.6, 8.0), (-3.3, -8.0)):         # exactly on an edge: two in, two out
        rows.append((px, py, math.atan2(-py, -px), 0.5))
    for px, py in ((7.8, 1.0), (-7.8, -2.0), (3.0, 7.85), (-4.0, -7.9), (7.9, 7.9)):   # discs cut by an edge / the corner
        rows.append((px, py, math.atan2(-py, -px) + 0.3, 0.6))
    rows.append((0.0, 0.0, 0.7, 0.5))                                           # two overlapping agents: either's beams
    rows.append((0.3, 0.1, -2.1, 0.5))                                          # start inside the other's disc
    rows.append((-3.0, 2.5, 1.9, 2.0))                                          # a radius of 2 m
    st = np.array(rows).T
    assert st.shape == (4, 24)
    return Scene("map_edge", _walls(160, 160, rng, 0.004), 0.1, 0.1, 6.0, 512, -math.pi / 2, math.pi / 2,
                 st[0], st[1], st[2], st[3], catches=("opaque", "first"))


# ---------------------------------------------------------------- d. range_res of several cells, agents outside
def coarse_outside():
    """range_res = 6 cells: 5 agents beyond every edge, 0.5 .. 5 m outside (1.2, 1.8 and 2.4 m put the first marched sample
    two whole range steps before the map), fanning 64 beams into it, and one agent just inside every edge looking out;
    a wall along every edge row and column"""
    g = _walls(160, 160)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = True
    rows = []
    for k, (ux, uy) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        for j, d in enumerate((0.5, 1.2, 1.8, 2.4, 5.0)):
            lateral = -6.0 + 2.9 * j + 0.37 * k
            px, py = ux * (8.0 + d) + abs(uy) * lateral, uy * (8.0 + d) + abs(ux) * lateral
            rows.append((px, py, math.atan2(-uy, -ux) + 0.013 * (j - 2) + 1e-3, 0.4))
        px, py = ux * 7.33 + abs(uy) * 1.7, uy * 7.33 + abs(ux) * 1.7          # inside, looking out through the edge
        rows.append((px, py, math.atan2(uy, ux) + 0.021, 0.3))
    st = np.array(rows).T
    assert st.shape == (4, 24)
    return Scene("coarse_outside", g, 0.1, 0.6, 6.0, 64, -math.pi / 2, math.pi / 2, st[0], st[1], st[2], st[3])


# ---------------------------------------------------------------- e. the history writers: moving agents
def movers(N, num_beams, num_to_store, E=3):
    """agents that cross the reference's map under RVO (goals on the other side); two sets of case rows, the second for a
    masked reset in the middle of the sequence"""
    rng = np.random.default_rng(100 * N + num_beams)
    cases = np.zeros((2, E, N, 6))
    cases[..., 0:2] = rng.uniform(-5.0, 5.0, (2, E, N, 2))
    cases[..., 2:4] = -cases[..., 0:2] + rng.uniform(-1.0, 1.0, (2, E, N, 2))
    cases[..., 4] = rng.uniform(0.8, 1.6, (2, E, N))
    cases[..., 5] = rng.uniform(0.2, 0.6, (2, E, N))
    heading = rng.uniform(-math.pi, math.pi, (2, E, N))
    sc = Scene("movers_N%d_B%d_H%d" % (N, num_beams, num_to_store), _walls(160, 160, rng, 0.004), 0.1, 0.1, 6.0, num_beams,
               -math.pi / 2, math.pi / 2, cases[0, ..., 0], cases[0, ..., 1], heading[0], cases[0, ..., 5],
               num_to_store=num_to_store)
    sc.case_rows, sc.case_headings = cases, heading
    return sc


MOVERS = [(5, 37, 3), (5, 516, 4), (1, 512, 3), (3, 512, 3), (5, 512, 3), (7, 512, 3)]     # (N, B, H)


# ---------------------------------------------------------------- f. a map set whose rows end in padding bits
def map_set():
    """3 maps of 72 x 100 cells (4 words per row, 28 of their bits padding); 5 envs on maps 2, 0, 1, 1, 2"""
    rng = np.random.default_rng(31)
    grids = np.stack([_walls(72, 100, rng, 0.01) for _ in range(3)])
    grids[0, :, -1] = True                    # the last real column of map 0: the bit next to the padding
    grids[1, 20:50, 60] = True
    grids[2, 50, 10:90] = True
    E, N = 5, 6
    px, py = rng.uniform(-13.0, 13.0, (E, N)), rng.uniform(-9.5, 9.5, (E, N))
    return Scene("map_set", grids, 0.25, 0.25, 8.0, 64, -math.pi, math.pi, px, py, rng.uniform(-math.pi, math.pi, (E, N)),
                 rng.uniform(0.3, 1.2, (E, N)), env_map=[2, 0, 1, 1, 2])


# ---------------------------------------------------------------- g. a ragged batch
def ragged():
    """6 slots, envs of 2, 4 and 6 agents: the empty slots are case rows of radius 0 (a reset leaves them at the origin)"""
    rng = np.random.default_rng(41)
    E, N = 3, 6
    px, py = rng.uniform(-3.0, 3.0, (E, N)), rng.uniform(-3.0, 3.0, (E, N))
    radius = rng.uniform(0.3, 0.8, (E, N))
    heading = rng.uniform(-math.pi, math.pi, (E, N))
    for e, n in enumerate((2, 4, 6)):
        px[e, n:], py[e, n:], radius[e, n:], heading[e, n:] = 0.0, 0.0, 0.0, 0.0
    return Scene("ragged", _walls(160, 160, rng, 0.004), 0.1, 0.1, 6.0, 512, -math.pi / 2, math.pi / 2, px, py, heading, radius)


def static_scenes():
    """every scene whose agents stand still, by name"""
    out = [lattice(0.25), lattice(0.1)] + geometries() + [map_edge(), coarse_outside(), map_set(), ragged()]
    return {s.name: s for s in out}


# ---------------------------------------------------------------- h. wall collisions at another geometry
def wall_scene():
    """72 x 100 cells of 0.25 m: static agents on, beside and just outside wall cells and map edges, some exactly on the
    lattice, pairwise farther apart than the sum of their radii -> (static, px, py, radius), the last three [E, N]"""
    g = np.zeros((72, 100), bool)
    g[20, 10:90] = True            # y in (3.75, 4.0]
    g[30:60, 70] = True            # x in [5.0, 5.25)
    g[0, :] = g[-1, :] = g[:, 0] = g[:, -1] = True
    env0 = [(-8.0, 4.0, 0.5), (-4.0, 4.3, 0.25), (0.0, 4.6, 0.5), (4.0, 3.74, 0.25), (8.5, 1.0, 0.25), (4.74, -3.0, 0.25),
            (4.5, -6.0, 0.5), (-12.5, 0.0, 0.25), (-12.2, -5.0, 0.3), (-12.6, 8.0, 1.0), (-2.0, -9.0, 0.5), (11.0, 9.1, 0.75)]
    env1 = [(-8.0, 3.7, 0.25), (-4.0, 1.0, 0.9), (0.0, 0.0, 1.0), (5.0, -2.0, 0.25), (5.25, -5.0, 0.25), (12.5, 3.0, 0.5),
            (12.3, -8.0, 0.3), (9.0, 9.0, 0.5), (-6.0, -8.6, 0.3), (-10.0, -8.76, 0.2), (-11.0, 8.74, 0.25), (0.0, 9.3, 0.5)]
    st = np.array([env0, env1])
    return g, st[..., 0], st[..., 1], st[..., 2]
