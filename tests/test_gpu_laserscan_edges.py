"""The scan kernel (csrc/cagpu_scan.inc) against the float64 numpy restatement tests/laserscan_ref.py -- which
tests/test_laserscan_ref_host.py pins to the reference's recorded episode and to the C++ oracle -- where the rest of the
suite does not look: samples exactly on cell borders, other grid geometries and beam fans, agents on, across and far
outside the map edges, a range step of several cells, both history writers with every remainder, a map set with padded
rows, a ragged batch, wall collisions on another grid.

The bar everywhere: `scan_hist` equals the reference on EVERY decided beam, no allowance (a beam is decided when its index
survives moving the direction cosines by the kernel's own error bound, laserscan_ref.decided; the host file caps the share
of the others at 0.5 % per scene and at 0 for the lattice scenes), `scan` is float32(index * range_res) or
float32(max_range), and the device fault word stays 0.  The scenes come from tests/laserscan_scenes.py; the reference is
always computed from the state read back from the GPU."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import laserscan_ref as lref
from tests import laserscan_scenes as scenes

pytestmark = pytest.mark.gpu

_cache = {}


def _mods():
    from gym_collision_avoidance_amd import _native as nat
    from gym_collision_avoidance_amd import core
    return nat, core


def _scene(name):
    if "static" not in _cache:
        _cache["static"] = scenes.static_scenes()
    return _cache["static"][name]


def _sim(sc, cases=None, headings=None, policy=None):
    nat, core = _mods()
    sim = core.BatchedSim(core.make_params(sc.E, sc.N, max_obs=max(1, min(sc.N - 1, 9)), ragged=int(sc.ragged)))
    if policy is not None:
        sim.set_plugins(policy)
    sim.set_map(**sc.map_args())
    sim.reset(sc.cases() if cases is None else cases, headings=sc.heading if headings is None else headings)
    return sim


def _state(sim):
    return {n: sim.state[n].cpu().numpy() for n in ("pos_x", "pos_y", "heading", "radius", "step_num")}


class _Judge(object):
    """The reference's history of a sim, advanced scan by scan from the state read back from the GPU"""

    def __init__(self, sim, sc):
        self.sim, self.sc = sim, sc
        shape = (sc.E, sc.N, sc.num_to_store, sc.num_beams)
        self.want = np.full(shape, lref.NOTHING, np.uint8)
        self.known = np.zeros(shape, bool)        # rows written from decided beams only
        self.compared = self.excluded = 0

    def scan(self, what=""):
        sim, sc = self.sim, self.sc
        st = _state(sim)
        scan = sim.laserscan().cpu().numpy()
        got = sim.scan_hist.cpu().numpy()
        idx, mask = sc.decided(st["pos_x"], st["pos_y"], st["heading"], st["radius"])
        present = st["radius"] > 0
        n_present = int(present.sum()) * sc.num_beams
        self.compared += int(mask.sum())
        self.excluded += n_present - int(mask.sum())
        assert n_present - int(mask.sum()) <= 0.005 * n_present, "%s %s: undecided share" % (sc.name, what)
        newest = np.where(mask, idx, got[:, :, 0, :])          # (an undecided beam: keep the histories in step)
        for e in range(sc.E):
            first = st["step_num"][e] == 0
            self.want[e] = lref.roll_history(self.want[e], newest[e], first)
            self.known[e] = lref.roll_history(self.known[e].astype(np.uint8), mask[e].astype(np.uint8), first).astype(bool)
        bad = (got != self.want) & self.known
        assert not bad.any(), "%s %s: %d of %d decided beams differ, first at (env, agent, row, beam) %s: GPU %d, reference %d" % (
            sc.name, what, bad.sum(), self.known.sum(), tuple(np.argwhere(bad)[0]), got[bad][0], self.want[bad][0])
        assert scan.dtype == np.float32 and np.array_equal(scan, lref.ranges_of(got, sc.range_res, sc.max_range)), sc.name
        return got

    def finish(self):
        nat, _ = _mods()
        assert nat.device_faults() == 0
        print("%s: %d beams compared, %d excluded as undecided" % (self.sc.name, self.compared, self.excluded))
        assert self.compared > 0


def _run_static(name, scans=2):
    """reset on the scene, then `scans` scans of the standing agents (the second and later ones from step_num 0 again:
    every row is filled every time)"""
    sc = _scene(name)
    sim = _sim(sc)
    st = _state(sim)
    live = sc.radius > 0
    for n, v in (("pos_x", sc.px), ("pos_y", sc.py), ("heading", sc.heading), ("radius", sc.radius)):
        assert np.array_equal(st[n][live], v[live]), n       # the scene the host file examined, bit for bit
    assert not st["radius"][~live].any() and not st["step_num"].any()
    judge = _Judge(sim, sc)
    for k in range(scans):
        got = judge.scan("scan %d" % k)
    judge.finish()
    return sim, sc, judge, got


# ---------------------------------------------------------------- a. samples exactly on cell borders
@pytest.mark.parametrize("cell", [0.25, 0.1])
def test_lattice_every_axis_sample_on_a_cell_border(cell):
    """24 agents on the lattice, headings exactly 0, beams along the axes: every such sample takes the kernel's cell-border
    fallback (cell_index / step1).  0.25: exact quotients; 0.1: the reference's float64 rounding decides every floor."""
    sim, sc, judge, got = _run_static("lattice_%g" % cell)
    assert judge.excluded == 0 and judge.compared == 2 * 216
    assert (got != lref.NOTHING).any()


# ---------------------------------------------------------------- b. other geometries
@pytest.mark.parametrize("name", ["wide_72x100", "two_beams_40x33", "coarse_160x160", "ranges_255"])
def test_geometry_sweep(name):
    """rows != cols, cols no multiple of 32 or 4, cells of 0.25 m, range_res below and above a cell, fans other than
    +-pi/2, 2 beams, 255 ranges; random off-lattice agents in and around the map"""
    sim, sc, judge, got = _run_static(name)
    if name == "ranges_255":
        assert sc.num_ranges == 255 and (got == 254).any()


# ---------------------------------------------------------------- c. the map edge
def test_agents_on_across_and_outside_the_map_edge():
    """agents 1 m, 5 m and beyond the laser's reach outside every side, exactly on x = +-8 and y = +-8, discs cut by every
    edge and by a corner, two overlapping agents, a radius of 2 m"""
    sim, sc, judge, got = _run_static("map_edge")
    assert (got[0, [2, 5, 8, 11]] == lref.NOTHING).all()      # farther than the laser reaches
    assert all((got[0, a] != lref.NOTHING).any() for a in (0, 3, 6, 9, 20, 21, 22, 23))


# ---------------------------------------------------------------- d. a range step of several cells, agents outside
def test_range_step_of_six_cells_with_agents_outside():
    """range_res = 6 cells, agents 0.5 .. 5 m beyond every edge looking in and just inside every edge looking out: the
    march used to begin and end up to two range steps outside the grid box -- 12 cells, more than the 8 of the LDS grid's
    border -- and read what lies around the grid as cells (50 of this scene's 1536 beams were wrong); at such a range step
    it now keeps to one"""
    sim, sc, judge, got = _run_static("coarse_outside")
    assert (got != lref.NOTHING).any() and (got == lref.NOTHING).any()


# ---------------------------------------------------------------- e. the history writers
@pytest.mark.parametrize("N,B,H", scenes.MOVERS)
def test_history_of_moving_agents(N, B, H):
    """5 scans of agents moving under RVO; B = 512: four beams per thread with 1, 3, 5 and 7 agents (every remainder of the
    staging of four agents), other B: the per-beam writer with 3 and 4 rows.  Before the fourth scan env 1 alone is reset:
    it fills every row, the others roll."""
    nat, core = _mods()
    sc = scenes.movers(N, B, H)
    sim = _sim(sc, sc.case_rows[0], sc.case_headings[0], policy=nat.POL_RVO)
    judge = _Judge(sim, sc)
    for k in range(5):
        if k == 3:
            sim.reset(sc.case_rows[1], headings=sc.case_headings[1], mask=np.array([0, 1, 0], np.uint8))
            step_num = _state(sim)["step_num"]
            assert not step_num[1].any() and step_num[0].all() and step_num[2].all()
        elif k:
            sim.step()
        got = judge.scan("scan %d" % k)
        if k == 2:
            assert all((got[:, :, h] != got[:, :, h + 1]).any() for h in range(2))     # three different rows
        if k == 3:
            assert all(np.array_equal(got[1, :, 0], got[1, :, h]) for h in range(H))   # filled
            assert not np.array_equal(got[0, :, 0], got[0, :, H - 1])                  # rolled
    judge.finish()


def test_unaligned_buffers_take_the_per_beam_writer():
    """cagpu_laserscan with hist and out 4 bytes into larger buffers, B = 512: the bytes of the aligned call, for a fill and
    for a roll, and not a byte outside the arrays"""
    nat, core = _mods()
    sc = scenes.movers(3, 512, 3)
    sim = _sim(sc, sc.case_rows[0], sc.case_headings[0], policy=nat.POL_RVO)
    n = sim.scan_hist.numel()
    assert sim.scan_hist.data_ptr() % 16 == 0 and sim.scan.data_ptr() % 16 == 0
    for phase in ("fill", "roll"):
        big_h = torch.full((n + 32,), 77, dtype=torch.uint8, device=sim.scan_hist.device)
        big_o = torch.full((n + 8,), -5.0, dtype=torch.float32, device=sim.scan_hist.device)
        assert big_h.data_ptr() % 16 == 0 and big_o.data_ptr() % 16 == 0
        big_h[4:4 + n].copy_(sim.scan_hist.view(-1))
        big_o[1:1 + n].copy_(sim.scan.view(-1))
        s0 = sim._scan
        off = nat.CaScan(hist=big_h.data_ptr() + 4, out=big_o.data_ptr() + 4, num_beams=s0.num_beams,
                         num_to_store=s0.num_to_store, num_ranges=s0.num_ranges, min_angle=s0.min_angle,
                         max_angle=s0.max_angle, range_res=s0.range_res, max_range=s0.max_range)
        sim.laserscan()
        nat.check(sim.lib.cagpu_laserscan(ctypes.byref(sim.p), ctypes.byref(sim._cs), ctypes.byref(sim._map),
                                          ctypes.byref(off), sim._stream()))
        torch.cuda.synchronize()
        assert torch.equal(big_h[4:4 + n], sim.scan_hist.view(-1)), phase
        assert torch.equal(big_o[1:1 + n].view(torch.int32), sim.scan.view(-1).view(torch.int32)), phase
        assert (big_h[:4] == 77).all() and (big_h[4 + n:] == 77).all() and big_o[0] == -5.0 and (big_o[1 + n:] == -5.0).all()
        if phase == "fill":
            sim.step()
            assert _state(sim)["step_num"].all()
    hist = sim.scan_hist.cpu().numpy()
    assert (hist[:, :, 0] != hist[:, :, 1]).any() and (hist != lref.NOTHING).any()
    assert nat.device_faults() == 0


# ---------------------------------------------------------------- f. a map set with padded rows
def test_map_set_with_padded_words():
    """3 maps of 72 x 100 cells (28 padding bits per row), env_map = [2, 0, 1, 1, 2]: every env against its own map"""
    sim, sc, judge, got = _run_static("map_set")
    assert sim.num_maps == 3 and sim.env_map.cpu().numpy().tolist() == [2, 0, 1, 1, 2]
    st = _state(sim)
    other, _ = lref.decided(sc.static[0], st["pos_x"][0], st["pos_y"][0], st["heading"][0], st["radius"][0], *sc.scan_args())
    assert (other != got[0, :, 0]).any()                      # env 0 on map 2 does not see what map 0 would show


# ---------------------------------------------------------------- g. a ragged batch
def test_ragged_batch_absent_slots_paint_nothing():
    """envs of 2, 4 and 6 agents in 6 slots: the present agents' scans are the reference's of the present agents alone"""
    nat, core = _mods()
    sim, sc, judge, got = _run_static("ragged")
    assert ((sim.state["flags"].cpu().numpy() & nat.ABSENT) != 0).sum(axis=1).tolist() == [4, 2, 0]
    assert judge.compared + judge.excluded == 2 * 12 * 512


# ---------------------------------------------------------------- h. wall collisions on another grid
def test_wall_collisions_on_a_quarter_metre_grid():
    """72 x 100 cells of 0.25 m, standing agents far from one another on, beside and just outside wall cells and map edges:
    after one step IN_COLLISION is the reference's wall test at the positions read back.  The agents stand because they
    are told to (external actions of speed 0), not as POL_STATIC: a StaticPolicy agent moves its goal onto itself
    (StaticPolicy.py:21-23), is at its goal from its first step on, and an agent at its goal is not tested for collisions
    (collision_avoidance_env.py:394-456) -- its flag could never rise."""
    nat, core = _mods()
    g, px, py, rad = scenes.wall_scene()
    E, N = px.shape
    sim = core.BatchedSim(core.make_params(E, N, max_obs=9))
    sim.set_plugins(nat.POL_EXTERNAL)
    sim.set_map(g, rows=72, cols=100, cell=0.25, num_beams=8, num_to_store=1)
    cases = np.zeros((E, N, 6))
    cases[..., 0], cases[..., 1], cases[..., 2], cases[..., 3], cases[..., 4], cases[..., 5] = px, py, px + 3.0, py, 1.0, rad
    sim.reset(cases)
    sim.step(np.zeros((E, N, 2)))
    st = _state(sim)
    assert np.array_equal(st["pos_x"], px) and np.array_equal(st["pos_y"], py) and st["step_num"].all()
    want = np.stack([lref.wall_hit(g, st["pos_x"][e], st["pos_y"][e], st["radius"][e], 0.25) for e in range(E)])
    got = (sim.state["flags"].cpu().numpy() & nat.IN_COLLISION) != 0
    assert np.array_equal(got, want), (got, want)
    assert want.any() and not want.all()
    assert nat.device_faults() == 0
