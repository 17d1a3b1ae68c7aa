"""CPU-only tests of the renderer's host side: the frame descriptors (render.episode_ranges / prefix_lasts: which tape slots
a frame shows) on synthetic counters, the window of a frame, and the CaRender layout / exports of include/cagpu.h and its
ctypes mirror.  The expected ranges are found in plain Python, slot by slot."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from gym_collision_avoidance_amd import _native as nat  # noqa: E402
from gym_collision_avoidance_amd import render as rd  # noqa: E402
from tests import render_ref as R  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(episode, epoch, cur_ep, cur_epoch, which, upto=None):
    T, S = episode.shape
    first, last = [], []
    for s in range(S):
        key = [(int(epoch[t, s]), int(episode[t, s])) for t in range(T)]
        cur = (int(cur_epoch[s]), int(cur_ep[s]))
        mine = [t for t in range(T) if key[t] == cur]
        if which == "last":
            others = [t for t in range(T) if key[t] != cur]
            mine = [t for t in others if key[t] == key[others[-1]]] if others else []
        if upto is not None:
            mine = mine[:upto + 1]
        first.append(mine[0] if mine else 0)
        last.append(mine[-1] if mine else -1)
    return first, last


def _ranges(episode, epoch, cur_ep, cur_epoch, which, upto=None):
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32)
    f, l = rd.episode_ranges(t(episode), t(epoch), t(cur_ep), t(cur_epoch), which, upto)
    assert f.dtype == torch.int32 and l.dtype == torch.int32
    return f.tolist(), l.tolist()


def _agree(episode, epoch, cur_ep, cur_epoch):
    episode, epoch = np.asarray(episode), np.asarray(epoch)
    for which in ("current", "last"):
        for upto in (None, 0, 1, 3, 100):
            got = _ranges(episode, epoch, cur_ep, cur_epoch, which, upto)
            f, l = _plain(episode, epoch, cur_ep, cur_epoch, which, upto)
            # a frame without slots is any pair with last < first
            for s in range(episode.shape[1]):
                if l[s] < f[s]:
                    assert got[1][s] < got[0][s], (which, upto, s, got)
                else:
                    assert (got[0][s], got[1][s]) == (f[s], l[s]), (which, upto, s, got, f, l)


def test_auto_resets_ragged_episode_lengths():
    # env 0: episodes 0 0 0 1 1 2 2 2 (running: 2); env 1: one running episode; env 2: reset at the very last step (running
    # episode 3 has no slot yet); env 3: episodes 4 4 5 5 5 5 5 5 (recording began in episode 4)
    episode = np.array([[0, 0, 0, 1, 1, 2, 2, 2], [0] * 8, [0, 0, 1, 1, 1, 2, 2, 2], [4, 4, 5, 5, 5, 5, 5, 5]]).T
    epoch = np.zeros_like(episode)
    cur = [2, 0, 3, 5]
    assert _ranges(episode, epoch, cur, [0] * 4, "current") == ([5, 0, 8, 2], [7, 7, 7, 7])
    f, l = _ranges(episode, epoch, cur, [0] * 4, "last")
    assert (f[0], l[0]) == (3, 4) and l[1] < f[1] and (f[2], l[2]) == (5, 7) and (f[3], l[3]) == (0, 1)
    assert _ranges(episode, epoch, cur, [0] * 4, "current", upto=1)[1] == [6, 1, 7, 3]
    _agree(episode, epoch, cur, [0] * 4)


def test_host_resets_cut_episodes():
    # a host reset zeroes the auto-reset count and raises the epoch: (epoch, episode) pairs tell the episodes apart even
    # where `episode` repeats
    episode = np.array([[0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 1, 1]]).T
    epoch = np.array([[0, 0, 0, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1]]).T
    assert _ranges(episode, epoch, [0, 0, 1], [1, 1, 1], "current") == ([3, 4, 4], [5, 5, 5])
    assert _ranges(episode, epoch, [0, 0, 1], [1, 1, 1], "last") == ([2, 0, 3], [2, 3, 3])
    # ... and a reset after the last recorded step: nothing of the tape is the running episode
    f, l = _ranges(episode, epoch, [0, 0, 0], [2, 2, 2], "current")
    assert all(b < a for a, b in zip(f, l))
    assert _ranges(episode, epoch, [0, 0, 0], [2, 2, 2], "last") == ([3, 4, 4], [5, 5, 5])
    _agree(episode, epoch, [0, 0, 1], [1, 1, 1])
    _agree(episode, epoch, [0, 0, 0], [2, 2, 2])


def test_empty_tape_and_no_finished_episode():
    none = np.zeros((0, 3), np.int32)
    for which in ("current", "last"):
        f, l = _ranges(none, none, [0, 1, 2], [0, 0, 0], which, upto=2)
        assert len(f) == 3 and all(b < a for a, b in zip(f, l))
    one = np.zeros((5, 2), np.int32)
    f, l = _ranges(one, one, [0, 0], [0, 0], "last")
    assert all(b < a for a, b in zip(f, l))
    with pytest.raises(ValueError):
        rd.episode_ranges(torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32),
                          torch.zeros((1,), dtype=torch.int32), torch.zeros((1,), dtype=torch.int32), "next")


def test_random_tapes_agree_with_the_slot_by_slot_search():
    rng = np.random.default_rng(7)
    for _ in range(40):
        T, S = int(rng.integers(1, 30)), int(rng.integers(1, 6))
        episode, epoch = np.zeros((T, S), np.int64), np.zeros((T, S), np.int64)
        cur_ep, cur_epoch = [], []
        for s in range(S):
            ep = ek = 0
            for t in range(T):
                episode[t, s], epoch[t, s] = ep, ek
                u = rng.random()
                if u < 0.15:
                    ep += 1
                elif u < 0.22:
                    ep, ek = 0, ek + 1
            cur_ep.append(ep)
            cur_epoch.append(ek)
        _agree(episode, epoch, cur_ep, cur_epoch)


def test_animation_prefixes():
    assert rd.prefix_lasts(0) == [] and rd.prefix_lasts(1) == [0] and rd.prefix_lasts(4) == [0, 1, 2, 3]
    assert rd.prefix_lasts(10, 3) == [2, 5, 8, 9] and rd.prefix_lasts(9, 3) == [2, 5, 8] and rd.prefix_lasts(2, 5) == [1]
    for L in range(1, 40):
        for every in (1, 2, 7):
            p = rd.prefix_lasts(L, every)
            assert p[-1] == L - 1 and p == sorted(set(p)) and all((k + 1) % every == 0 for k in p[:-1])


def test_window_equal_scale_and_the_spec_agree():
    for size, limits in [((128, 128), None), ((67, 93), ((-4.0, 4.0), (-2.0, 2.0))), ((400, 500), ((-1.0, 9.0), (0.0, 3.0))),
                         ((1000, 800), ((-0.1, 0.1), (5.0, 5.3)))]:
        xmin, ymax, s16 = rd.window(size, limits)
        assert (xmin, ymax, s16) == R.window(size, limits)          # the same float64 operations in the same order
        (x0, x1), (y0, y1) = rd.DEFAULT_LIMITS if limits is None else limits
        H, W = size
        ppm = s16 / 16
        assert xmin <= x0 + 1e-9 and xmin + W / ppm >= x1 - 1e-9 and ymax >= y1 - 1e-9 and ymax - H / ppm <= y0 + 1e-9
        assert abs((xmin + W / ppm / 2) - (x0 + x1) / 2) < 1e-9 and abs((ymax - H / ppm / 2) - (y0 + y1) / 2) < 1e-9
    assert rd.window((64, 64)) == (-8.0, 8.0, 64.0)
    with pytest.raises(ValueError):
        rd.window((64, 64), ((1.0, 1.0), (0.0, 1.0)))


def test_carender_layout_and_exports():
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    body = re.search(r"typedef struct CaRender \{(.*?)\} CaRender;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        first, rest = re.match(r"(?:const\s+)?\w+\s*(.*)", decl, re.S).group(1), None
        names += [n.strip().lstrip("*").strip() for n in first.split(",")]
    assert names == [f[0] for f in nat.CaRender._fields_]
    r = nat.CaRender
    assert (r.out.offset, r.num_frames.offset, r.flags.offset, r.xmin.offset, r.frame_env.offset) == (0, 8, 20, 24, 48)
    assert (r.hist.offset, r.hist_steps.offset, r.stride_t.offset, r.work.offset, r.work_bytes.offset) == (80, 88, 96, 112, 120)
    assert C.sizeof(r) == 128
    for sym in ("cagpu_render", "cagpu_render_maps", "cagpu_render_work_bytes"):
        assert sym in nat.EXPORTS and re.search(r"\b%s\(" % sym, hdr), sym
    from gym_collision_avoidance_amd import build_native   # (the include is a dependency of the build)
    assert os.path.join(REPO, "gym_collision_avoidance_amd", "csrc", "cagpu_render.inc") in build_native.source_files()


def test_library_exports_and_workspace_size():
    if not os.path.exists(nat.LIB_PATH):        # (a tree that has not been built yet: build it, as tests/test_occupancy_golden.py does)
        from gym_collision_avoidance_amd import build_native
        build_native.build()
    lib = nat.lib()
    assert lib.cagpu_render_work_bytes(3, 10, 0) == 3 * 16 + 3 * 10 * 2 * 32
    assert lib.cagpu_render_work_bytes(2, 4, 50) == 2 * 16 + 2 * 4 * 102 * 32
    assert lib.cagpu_render_work_bytes(0, 4, 50) == 0 and lib.cagpu_render_work_bytes(1, 4, -1) == 0
    r = nat.CaRender()
    assert lib.cagpu_render(None, None, None, C.byref(r), None) == nat.CA_EINVAL      # host-only: checked before any launch
    assert b"cagpu_render" in lib.cagpu_last_error()


def test_env_render_human_mode_points_at_rgb_array():
    from gym_collision_avoidance_amd.envs.collision_avoidance_env import CollisionAvoidanceEnv
    env = CollisionAvoidanceEnv.__new__(CollisionAvoidanceEnv)
    with pytest.raises(NotImplementedError, match="rgb_array"):
        env.render(mode="human")


def test_save_frames_round_trip(tmp_path):
    PIL = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, (5, 16, 24, 3), dtype=np.uint8)
    p = rd.save_frames(str(tmp_path / "sub" / "a.png"), frames[0])
    assert np.array_equal(np.asarray(PIL.open(p).convert("RGB")), frames[0])
    g = PIL.open(rd.save_frames(str(tmp_path / "anim" / "a.gif"), frames, hold_last=2))
    assert g.n_frames == 5 and g.size == (24, 16)
    g.seek(4)
    assert g.info["duration"] == 300
