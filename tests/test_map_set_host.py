"""CPU-only tests of the map set (include/cagpu.h CaMapSet, v12): version, struct layout, the argument checks of the two
map-set entry points (they fail before anything is launched, so no device is needed) and the env API's input forms."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import envtools

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from gym_collision_avoidance_amd import _native as nat
    so = nat.LIB_PATH
    if not os.path.exists(so):
        from gym_collision_avoidance_amd import build_native
        build_native.build()
    return nat, nat.lib()


def test_abi_version_is_12_everywhere():
    nat, lib = _lib()
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert lib.cagpu_version() == nat.ABI_VERSION == int(re.search(r"#define CAGPU_VERSION (\d+)", hdr).group(1)) == 12
    for name in ("cagpu_step_maps", "cagpu_laserscan_maps"):
        assert name in nat.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr)


def test_camapset_layout_matches_header():
    from gym_collision_avoidance_amd import _native as nat
    assert ctypes.sizeof(nat.CaMapSet) == ctypes.sizeof(nat.CaMap) + 8 + 2 * 4 + 8 == 64
    assert nat.CaMapSet.map.offset == 0
    assert nat.CaMapSet.env_map.offset == 40
    assert nat.CaMapSet.num_maps.offset == 48 and nat.CaMapSet.reserved0.offset == 52
    assert nat.CaMapSet.map_seed.offset == 56
    # the single-map structs keep their v11 layout
    assert ctypes.sizeof(nat.CaMap) == 40 and ctypes.sizeof(nat.CaAutoReset) == 56


def _fake_call_args(nat):
    """host structs whose device pointers are never dereferenced: every call below fails its argument checks first"""
    from gym_collision_avoidance_amd import core
    p = core.make_params(4, 4)
    fake = 0x1000
    s = nat.CaState(**{n: fake for n in nat.STATE_FIELDS if n not in ("next_action", "turning_dir", "rvo_collab",
                                                                       "rvo_heading_noise", "ext_state")})
    o = nat.CaOut(obs=fake, rewards=fake, done=fake, game_over=fake)
    sc = nat.CaScan(hist=fake, out=fake, num_beams=512, num_to_store=3, num_ranges=60, min_angle=-1.5, max_angle=1.5,
                    range_res=0.1, max_range=6.0)
    return p, s, o, sc


def _good_set(nat, fake=0x2000):
    m = nat.CaMap(static_bits=fake, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    return nat.CaMapSet(map=m, env_map=fake, num_maps=3, map_seed=7)


@pytest.mark.parametrize("what", ["null_set", "null_env_map", "null_bits", "zero_maps", "negative_maps", "rows",
                                  "cols", "cell"])
def test_map_set_entry_points_reject_bad_arguments(what):
    nat, lib = _lib()
    p, s, o, sc = _fake_call_args(nat)
    ms = _good_set(nat)
    if what == "null_env_map":
        ms.env_map = None
    elif what == "null_bits":
        ms.map.static_bits = None
    elif what == "zero_maps":
        ms.num_maps = 0
    elif what == "negative_maps":
        ms.num_maps = -2
    elif what == "rows":
        ms.map.rows = 0
    elif what == "cols":
        ms.map.cols = -1
    elif what == "cell":
        ms.map.cell = 0.0
    ref = None if what == "null_set" else ctypes.byref(ms)
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    rc = lib.cagpu_step_maps(ctypes.byref(p), ctypes.byref(s), ctypes.byref(o), None, None, ref, None)
    assert rc == nat.CA_EINVAL, lib.cagpu_last_error()
    assert lib.cagpu_last_kernel() == before      # nothing was selected, let alone launched
    rc = lib.cagpu_laserscan_maps(ctypes.byref(p), ctypes.byref(s), ref, ctypes.byref(sc), None)
    assert rc == nat.CA_EINVAL, lib.cagpu_last_error()
    assert b"CaMapSet" in lib.cagpu_last_error()


def test_env_set_static_map_per_env_accepts_the_three_forms(tmp_path):
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        rng = np.random.default_rng(3)
        grids = [rng.random((160, 160)) < 0.01 for _ in range(3)]
        env = Env()
        env.set_static_map(np.stack(grids), per_env=True)                 # an array [M, 160, 160]
        assert len(env.maps) == 3 and all(np.array_equal(m.static_map, g) for m, g in zip(env.maps, grids))
        env.set_static_map(list(grids[:2]), per_env=True, map_seed=5)    # a list of bool arrays
        assert len(env.maps) == 2 and np.array_equal(env.maps[1].static_map, grids[1])
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None:                                             # a list of image paths (dark = occupied)
            paths = []
            for i, g in enumerate(grids):
                path = str(tmp_path / ("map%d.png" % i))
                Image.fromarray(np.where(g, 0, 255).astype(np.uint8)).save(path)
                paths.append(path)
            env.set_static_map(paths, per_env=True)
            assert len(env.maps) == 3 and all(np.array_equal(m.static_map, g) for m, g in zip(env.maps, grids))
        # without per_env: the single-map behaviour (nothing loaded or drawn here)
        state = np.random.get_state()[1].copy()
        env.set_static_map(np.stack(grids)[0])
        assert env._map_set is None and np.array_equal(np.random.get_state()[1], state)
    finally:
        envtools.default()


@pytest.mark.parametrize("bad", [np.zeros((3, 160, 161), bool), np.zeros((3, 80, 80), bool), [np.zeros((160, 160), bool),
                                                                                                np.zeros((16, 16), bool)],
                                 np.zeros((160,), bool), []])
def test_env_set_static_map_per_env_rejects_wrong_shapes(bad):
    Config, tc, Env = envtools.fresh("Laser4")
    try:
        env = Env()
        with pytest.raises(ValueError):
            env.set_static_map(bad, per_env=True)
    finally:
        envtools.default()
