"""CPU-only tests of the OccupancyGridSensor: the numpy restatement (tests/occupancy_ref.py) against windows recorded from
the unmodified reference (tests/golden/occgrid.npz, written by tests/record_occupancy_golden.py), the anchoring rule at the
positions where the reference raises, the sensor's registration in the env layer, the C ABI (struct layout, exports,
version) and every argument check of the two entry points that returns before a device call."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import envtools
from tests import occupancy_ref as oref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "occgrid.npz")


def _lattice():
    """40 "round" positions: (-10.4, 2.8), then 39 at which the reference's sense() raises ValueError (its two independently
    floored corners span 49 or 51 cells), each verified against the reference by the recorder (lat_valid: what the reference
    did there; at the literal float -10.4 it returns a window, at -11 + 6 * 0.1 = -10.400000000000002 it raises)
    -> (positions, valid, the reference's windows)"""
    g = np.load(GOLD)
    return [tuple(float(v) for v in row) for row in g["lat_xy"]], g["lat_valid"], _unpack(g["lat_windows"], 50)


def _unpack(bits, width):
    return np.unpackbits(bits, axis=-1, bitorder="little")[..., :width].astype(bool)


def _lib():
    from gym_collision_avoidance_amd import _native as nat
    if not os.path.exists(nat.LIB_PATH):
        from gym_collision_avoidance_amd import build_native
        build_native.build()
    return nat, nat.lib()


def test_restatement_equals_every_valid_golden_row():
    g = np.load(GOLD)
    n_rows = g["ep_valid"].size + g["sc_valid"].size
    n_bad = n_rows - int(g["ep_valid"].sum()) - int(g["sc_valid"].sum())
    assert n_rows >= 1000 and n_bad <= 0.02 * n_rows, (n_bad, n_rows)      # the recorder's cap, asserted on the file
    # (a) the episode
    static = _unpack(g["ep_static"], 160)
    state, want, valid = g["ep_state"], _unpack(g["ep_windows"], 50), g["ep_valid"]
    assert (np.abs(state[:, :, :2]) > 5.5).any()                             # partial windows occur
    assert want.any(axis=(2, 3)).sum() > 100
    checked = 0
    for t in range(len(state)):
        got = oref.occupancy(static, state[t, :, 0], state[t, :, 1], state[t, :, 2])
        for a in range(state.shape[1]):
            if valid[t, a]:
                assert np.array_equal(got[a], want[t, a]), "episode step %d agent %d" % (t, a)
                checked += 1
    # (b) the scenes
    grids = _unpack(g["sc_grids"], 160)
    state, want, valid = g["sc_state"], _unpack(g["sc_windows"], 50), g["sc_valid"]
    kinds = set()
    for s in range(len(state)):
        got = oref.occupancy(grids[s % len(grids)], state[s, :, 0], state[s, :, 1], state[s, :, 2])
        for a in range(state.shape[1]):
            far = max(abs(state[s, a, 0]), abs(state[s, a, 1]))
            kinds.add("inside" if far < 5.5 else "partial" if far < 10.5 else "outside")
            if valid[s, a]:
                assert np.array_equal(got[a], want[s, a]), "scene %d agent %d" % (s, a)
                checked += 1
    assert kinds == {"inside", "partial", "outside"}
    assert checked == n_rows - n_bad


@pytest.mark.parametrize("k", range(40))
def test_restatement_follows_the_anchoring_rule_on_the_lattice(k):
    """where the reference raises, the window is still H x W and is the anchored rule, written out cell by cell with Python
    ints and math.floor"""
    lattice, valid, ref_windows = _lattice()
    assert len(lattice) == 40 and lattice[0] == (-10.4, 2.8) and not valid[1:].any()
    px, py = lattice[k]
    if valid[k]:   # the reference returned a window here after all: then it is the restatement's
        assert np.array_equal(oref.occupancy(np.zeros((160, 160), bool), [px], [py], [0.5])[0], ref_windows[k])
    rng = np.random.default_rng(int(1000 * abs(px) + 10 * abs(py)))
    static = rng.random((160, 160)) < 0.05
    ox, oy, orad = rng.uniform(-8, 8, 5), rng.uniform(-8, 8, 5), rng.uniform(0.2, 0.8, 5)
    xs, ys, rad = np.append(ox, px), np.append(oy, py), np.append(orad, 0.5)
    dyn = oref.dynamic_map(static, xs, ys, rad)
    got = oref.occupancy(static, xs, ys, rad)[-1]
    assert got.shape == (50, 50) and got.dtype == bool
    origin = (160 * 0.1 / 2.) / 0.1
    i0 = math.floor(origin - (py + 5 / 2.) / 0.1)
    j0 = math.floor(origin + (px - 5 / 2.) / 0.1)
    assert (i0, j0) == oref.anchor(px, py, 160, 160)
    for a in range(50):
        for b in range(50):
            r, c = i0 + a, j0 + b
            want = bool(dyn[r, c]) if (0 <= r < 160 and 0 <= c < 160) else False
            assert bool(got[a, b]) == want, (a, b)


def test_dynamic_map_rules():
    static = np.zeros((160, 160), bool)
    # an agent whose centre cell is outside the grid paints nothing, however large
    assert not oref.dynamic_map(static, [8.05], [0.0], [1.5]).any()
    # radius 0 (an absent slot) paints nothing; the test is strict (<)
    assert not oref.dynamic_map(static, [0.0], [0.0], [0.0]).any()
    # (0.3 / 0.1 = 2.9999999999999996 in float64: the cells at distance^2 = 9 are out, the 25 with distance^2 <= 8 are in)
    d = oref.dynamic_map(static, [0.0], [0.0], [0.3])
    assert d[80, 80] and d[80, 82] and d[82, 82] and not d[80, 83] and d.sum() == 25
    # the agent's own disc stays in its window
    assert oref.occupancy(static, [0.0], [0.0], [0.3])[0].sum() == 25


def test_sensor_registration_and_observation_space():
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        from gym_collision_avoidance_amd.envs.sensors import OccupancyGridSensor, LaserScanSensor
        from gym_collision_avoidance_amd.envs.sensors.OccupancyGridSensor import OccupancyGridSensor as Direct
        assert Direct is OccupancyGridSensor and tc.sensor_dict["occupancy_grid"] is OccupancyGridSensor
        s = OccupancyGridSensor()
        assert s.name == "occupancy_grid" and (s.x_width, s.y_width, s.grid_cell_size) == (5, 5, 0.01)
        s.set_args({"x_width": 3, "y_width": 6.4})
        assert (s.x_width, s.y_width) == (3, 6.4)
        w = np.eye(4, dtype=bool)
        r = s.resize(w)
        assert r is not w and np.array_equal(r, w)
        info = Config.STATE_INFO_DICT["occupancy_grid"]
        assert tuple(info["size"]) == (50, 50) and list(info["bounds"]) == [0, 1]
        assert "occupancy_grid" not in Config.STATES_IN_OBS          # off unless a config lists it
        assert LaserScanSensor().name == "laserscan"
    finally:
        envtools.default()
    Config, tc, Env = envtools.fresh("OccLaser4", os.path.join(REPO, "tests", "occupancy_configs.py"))
    try:
        assert "occupancy_grid" in Config.STATES_IN_OBS
        env = Env()
        box = env.observation_space.spaces[0].spaces["occupancy_grid"]
        assert box.shape == (50, 50) and float(box.low.min()) == 0.0 and float(box.high.max()) == 1.0
        assert env.observation[0]["occupancy_grid"].shape == (50, 50)
        assert env.occupancy_grid is None                            # nothing uploaded yet
    finally:
        envtools.default()


def test_sensor_needs_the_static_map_config():
    Config, tc, Env = envtools.fresh("Swap4")
    try:
        from gym_collision_avoidance_amd.envs.sensors import OccupancyGridSensor
        assert not Config.USE_STATIC_MAP
        with pytest.raises(AssertionError):
            OccupancyGridSensor()
    finally:
        envtools.default()


def test_caoccgrid_layout_exports_and_version():
    nat, lib = _lib()
    assert ctypes.sizeof(nat.CaOccGrid) == 40
    assert [getattr(nat.CaOccGrid, n).offset for n in ("cells", "bits", "height", "width", "x_width", "y_width")] == \
        [0, 8, 16, 20, 24, 32]
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert re.search(r"typedef struct CaOccGrid \{[^}]*uint8_t \*cells;[^}]*uint32_t \*bits;[^}]*int32_t height, width;"
                     r"[^}]*double x_width, y_width;[^}]*\} CaOccGrid;", hdr)
    for name in ("cagpu_occupancy_grid", "cagpu_occupancy_grid_maps"):
        assert name in nat.EXPORTS and re.search(r"\bint %s\s*\(" % name, hdr)
        assert getattr(lib, name) is not None
    assert lib.cagpu_version() == nat.ABI_VERSION == int(re.search(r"#define CAGPU_VERSION (\d+)", hdr).group(1)) == 12
    # the structs beside it keep their layout
    assert ctypes.sizeof(nat.CaMap) == 40 and ctypes.sizeof(nat.CaMapSet) == 64


def _fake_args(nat, num_agents=4):
    """host structs whose device pointers are never dereferenced: every call below fails its argument checks first"""
    from gym_collision_avoidance_amd import core
    p = core.make_params(4, num_agents)
    fake = 0x1000
    s = nat.CaState(pos_x=fake, pos_y=fake, radius=fake)
    m = nat.CaMap(static_bits=fake, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    g = nat.CaOccGrid(cells=fake, bits=fake, height=50, width=50, x_width=5.0, y_width=5.0)
    return p, s, m, g


BAD = ["null_params", "null_state", "null_map", "null_grid", "num_envs", "num_agents", "too_many_agents", "rows", "cols",
       "cell", "both_outputs_null", "height_0", "height_257", "width_0", "width_257", "pos_x", "pos_y", "radius",
       "misaligned_cells", "misaligned_bits"]


@pytest.mark.parametrize("what", BAD)
def test_entry_points_reject_bad_arguments_before_any_device_call(what):
    nat, lib = _lib()
    p, s, m, g = _fake_args(nat)
    args = dict(p=ctypes.byref(p), s=ctypes.byref(s), m=ctypes.byref(m), g=ctypes.byref(g))
    if what.startswith("null_"):
        args[{"params": "p", "state": "s", "map": "m", "grid": "g"}[what[5:]]] = None
    elif what == "num_envs":
        p.num_envs = 0
    elif what == "num_agents":
        p.num_agents = 0
    elif what == "too_many_agents":
        p.num_agents = 1025
    elif what == "rows":
        m.rows = 0
    elif what == "cols":
        m.cols = -3
    elif what == "cell":
        m.cell = 0.0
    elif what == "both_outputs_null":
        g.cells, g.bits = None, None
    elif what in ("height_0", "height_257", "width_0", "width_257"):
        setattr(g, what.split("_")[0], int(what.split("_")[1]))
    elif what in ("pos_x", "pos_y", "radius"):
        setattr(s, what, None)
    elif what == "misaligned_cells":
        g.cells = 0x1004
    elif what == "misaligned_bits":
        g.bits = 0x1008
    rc = lib.cagpu_occupancy_grid(args["p"], args["s"], args["m"], args["g"], None)
    assert rc == nat.CA_EINVAL, lib.cagpu_last_error()
    assert b"cagpu_occupancy_grid" in lib.cagpu_last_error()
    if what == "null_map":
        return
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=0)
    rc = lib.cagpu_occupancy_grid_maps(args["p"], args["s"], ctypes.byref(ms), args["g"], None)
    assert rc == nat.CA_EINVAL, lib.cagpu_last_error()


@pytest.mark.parametrize("what", ["null_set", "null_env_map", "null_bits", "zero_maps", "rows", "cell"])
def test_maps_entry_point_goes_through_the_map_set_checks(what):
    nat, lib = _lib()
    p, s, m, g = _fake_args(nat)
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=0)
    if what == "null_env_map":
        ms.env_map = None
    elif what == "null_bits":
        ms.map.static_bits = None
    elif what == "zero_maps":
        ms.num_maps = 0
    elif what == "rows":
        ms.map.rows = 0
    elif what == "cell":
        ms.map.cell = -1.0
    rc = lib.cagpu_occupancy_grid_maps(ctypes.byref(p), ctypes.byref(s), None if what == "null_set" else ctypes.byref(ms),
                                       ctypes.byref(g), None)
    assert rc == nat.CA_EINVAL, lib.cagpu_last_error()
    assert b"CaMapSet" in lib.cagpu_last_error()


def test_a_map_whose_bitmap_does_not_fit_the_lds_is_unsupported():
    nat, lib = _lib()
    p, s, m, g = _fake_args(nat)
    m.rows, m.cols = 2048, 2048          # 512 KB of bits
    assert lib.cagpu_occupancy_grid(ctypes.byref(p), ctypes.byref(s), ctypes.byref(m), ctypes.byref(g), None) == \
        nat.CA_EUNSUPPORTED
    assert b"LDS" in lib.cagpu_last_error()
    # a static_bits of NULL (no obstacles) and a single output are fine as far as the checks go: they fail later, at the
    # launch, which needs a device -- so here only the other direction is shown: the checks above did not object to them
    m.rows, m.cols, m.static_bits = 160, 160, None
    g.cells = None
    p.num_envs = 0
    assert lib.cagpu_occupancy_grid(ctypes.byref(p), ctypes.byref(s), ctypes.byref(m), ctypes.byref(g), None) == nat.CA_EINVAL
    assert b"bad sizes" in lib.cagpu_last_error()


def test_pack_rows_matches_the_bits_format():
    rng = np.random.default_rng(0)
    cells = rng.random((3, 5, 50)) < 0.3
    words = oref.pack_rows(cells)
    assert words.shape == (3, 5, 2) and words.dtype == np.uint32
    for b in range(50):
        assert np.array_equal((words[..., b >> 5] >> np.uint32(b & 31)) & np.uint32(1), cells[..., b].astype(np.uint32))
    assert not (words[..., 1] >> np.uint32(18)).any()        # unused high bits are zero
