"""The episode metrics without a GPU: the rules of tests/episode_metrics_ref.py on tiny tapes whose numbers are worked out
by hand, the drain / gather / clear arithmetic of gym_collision_avoidance_amd/episode_metrics.py on numpy and torch-CPU
buffers, the C ABI (include/cagpu.h CaEpMetrics) against its ctypes mirror, and the argument checks that return before
anything is launched."""
import ctypes
import math
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import episode_metrics_ref as ref  # noqa: E402

NAN = float("nan")


def tape(T, E, N):
    """an empty tape: nobody moves, and columns 0 - 10 are NaN -- a NaN in a result is a forbidden read"""
    rows = np.full((T, E, N, 12), NAN)
    rows[..., 11] = -1.0
    return rows, np.zeros((T, E), np.int32)


def move(rows, t, e, a, time, px, py, rad, vx, vy, heading, index):
    rows[t, e, a] = (time, px, py, NAN, NAN, rad, NAN, vx, vy, NAN, heading, index)


def test_two_agents_head_on():
    rows, ep = tape(3, 1, 2)
    for t in range(3):   # 1 m/s towards each other along x, dt = 0.5: centres 3, 2, 1 m apart after the moves
        move(rows, t, 0, 0, 0.5 * t, -1.0 + 0.5 * (t + 1) - 1.0, 0.0, 0.25, 1.0, 0.0, 0.0, t)
        move(rows, t, 0, 1, 0.5 * t, 1.0 - 0.5 * (t + 1) + 1.0, 0.0, 0.25, -1.0, 0.0, math.pi, t)
    m = ref.Metrics(1, 2, 1, dt=0.5, getting_close_range=1.0).process(rows, ep)
    assert m.head.tolist() == [[0]]
    for a in (0, 1):
        assert m.vals[0, 0, a].tolist() == [1.5, 0.5, 0.0, 1.0]       # path 3 x 0.5, gap 1 - 2 x 0.25 at the row of t = 1.0
        assert m.cnts[0, 0, a].tolist() == [3, 1, 1 - a, 0]           # gaps 2.5, 1.5, 0.5: one step within 1.0


def test_an_agent_that_stops_stays_an_obstacle_where_it_stopped():
    T = 7
    rows, ep = tape(T, 1, 2)
    for t in range(3):       # agent 0 walks up the y axis for three steps, then is done at (0, 1.5): NaN rows from there on
        move(rows, t, 0, 0, 0.5 * t, 0.0, 0.5 * (t + 1), 0.5, 0.0, 1.0, 0.5 * math.pi, t)
    xs = [-9.0, -8.0, -7.0, -4.0, 0.0, 4.0, 8.0]     # agent 1 passes it on the line y = 4.5 (3-4-5 triangles)
    for t in range(T):
        move(rows, t, 0, 1, 0.5 * t, xs[t], 4.5, 0.5, 2.0, 0.0, 0.0, t)
    m = ref.Metrics(1, 2, 1, dt=0.5, getting_close_range=2.0).process(rows, ep)
    d = lambda x, y: math.sqrt(x * x + y * y) - 0.5 - 0.5
    g0 = [d(xs[t], 4.5 - 0.5 * (t + 1)) for t in range(3)]            # while both move
    g1 = g0 + [d(x, 3.0) for x in xs[3:]]                             # agent 1 against the place agent 0 stopped at
    assert g1[3:] == [4.0, 2.0, 4.0, math.sqrt(73.0) - 1.0]
    assert m.vals[0, 0, 0].tolist() == [1.5, min(g0), 0.0, 0.5 * g0.index(min(g0))]
    assert m.cnts[0, 0, 0].tolist() == [3, 0, 1, 0]
    assert m.vals[0, 0, 1].tolist() == [7.0, 2.0, 0.0, 2.0]           # closest as it passes, at its row of t = 2.0
    assert m.cnts[0, 0, 1].tolist() == [7, 1, 0, 0]
    assert not np.isnan(m.vals[..., :3]).any()


def test_a_lone_agent_and_slots_nobody_moved_in():
    rows, ep = tape(4, 1, 3)
    for t in (0, 2, 3):      # slot 1 is empty; agents 0 and 2 never move: never seen
        move(rows, t, 0, 1, 0.1 * t, 1.0 * t, 0.0, 0.3, 3.0, 4.0, 0.0, t)
    m = ref.Metrics(1, 3, 2, dt=0.1, getting_close_range=0.2).process(rows, ep)
    assert m.head.tolist() == [[0, -1]]
    v, c = m.vals[0, 0], m.cnts[0, 0]
    assert v[1, :3].tolist() == [0.5 + 0.5 + 0.5, math.inf, 0.0] and math.isnan(v[1, 3])
    assert c[1].tolist() == [3, 0, -1, 0]
    for a in (0, 2):
        assert v[a, :3].tolist() == [0.0, math.inf, 0.0] and math.isnan(v[a, 3]) and c[a].tolist() == [0, 0, -1, 0]


def test_heading_changes_are_wrapped_across_pi():
    hs = [3.0, -3.0, 3.1, 3.1, -3.1]
    rows, ep = tape(len(hs), 1, 1)
    for t, h in enumerate(hs):
        move(rows, t, 0, 0, 0.1 * t, 0.0, 0.0, 0.3, 0.0, 0.0, h, t)
    m = ref.Metrics(1, 1, 1, dt=0.1, getting_close_range=0.2).process(rows, ep)
    two_pi = 2.0 * math.pi
    want = 0.0
    for d in (two_pi - 6.0, two_pi - 6.1, 0.0, two_pi - 6.2):   # the short way round, every time
        want += d
    assert abs(m.vals[0, 0, 0, ref.TURN] - want) < 4 * 2.0 ** -52
    # ... and exactly the sum of IEEE remainders, added in step order
    exact = 0.0
    for a, b in zip(hs, hs[1:]):
        exact = exact + math.fabs(math.remainder(b - a, two_pi))
    assert m.vals[0, 0, 0, ref.TURN] == exact
    assert m.cnts[0, 0, 0].tolist() == [5, 0, -1, 0]


def _five_episodes(E=3, N=2, C=2):
    """a tape on which env e finishes episodes 0 .. 4 of 2 + e steps each (the last one ends with the tape)"""
    lens = [2 + e for e in range(E)]
    T = 5 * max(lens)
    rows, ep = tape(T, E, N)
    for e in range(E):
        for t in range(T):
            k = min(t // lens[e], 4)
            ep[t, e] = k
            if t < 5 * lens[e]:
                i = t % lens[e]
                move(rows, t, e, 0, 0.1 * i, 0.25 * i + e, 0.0, 0.2, 1.0 + k, 0.0, 0.0, i)
                move(rows, t, e, 1, 0.1 * i, 0.25 * i + e, 1.0 + 0.125 * k, 0.2, 0.0, 0.0, 0.0, i)
    return rows, ep, ref.Metrics(E, N, C, dt=0.1, getting_close_range=0.2).process(rows, ep)


def test_drain_gather_and_clear_agree_on_numpy_and_torch():
    import torch
    from gym_collision_avoidance_amd import episode_metrics as em
    rows, ep, m = _five_episodes()
    E, C = 3, 2
    assert m.head.tolist() == [[4, 3]] * E           # episodes 0 - 2 of every env were overwritten
    table = ref.episode_table(rows, ep, 0.1, 0.2)
    carry = np.ones((E, 176), np.uint8)

    def both(f, *arrays):
        return f(*arrays), f(*[torch.from_numpy(np.array(a)) for a in arrays])

    rc = np.array([5, 4, 5])                          # env 1: its last episode is still running as far as the caller knows
    for out, cur in both(lambda v, c, h, cu, r: em.drain(v, c, h, cu, r), m.vals, m.cnts, m.head, np.zeros(E, np.int64), rc):
        assert out["dropped"] == 3 + 3 + 3   # (env 1: episodes 0, 1 fell out of the window, 2 lost its slot to the running 4)
        assert np.asarray(out["env"]).tolist() == [0, 0, 1, 2, 2] and np.asarray(out["episode"]).tolist() == [3, 4, 3, 3, 4]
        assert np.asarray(cur).tolist() == [5, 4, 5]
        for i, (e, k) in enumerate(zip(np.asarray(out["env"]), np.asarray(out["episode"]))):
            v, c = table[(int(e), int(k))]
            for j, n in enumerate(em.FLOAT_COLUMNS):
                assert np.array_equal(np.asarray(out[n][i]), v[:, j], equal_nan=True), n
            for j, n in enumerate(em.INT_COLUMNS):
                assert np.array_equal(np.asarray(out[n][i]), c[:, j]), n
                assert np.asarray(out[n]).dtype == np.int32
        assert np.asarray(out["min_gap"]).shape == (5, 2)
    # a second drain returns the late episode only; a stale stamp (slot rewritten by hand) counts as dropped
    for lib in (np.array, lambda a: torch.from_numpy(np.array(a))):
        head = lib(m.head)
        out, cur = em.drain(lib(m.vals), lib(m.cnts), head, lib(np.array([5, 4, 5])), lib(np.array([5, 5, 5])))
        assert (out["dropped"], np.asarray(out["env"]).tolist(), np.asarray(out["episode"]).tolist()) == (0, [1], [4])
        head[1, 0] = 6
        out, cur = em.drain(lib(m.vals), lib(m.cnts), head, lib(np.array([5, 4, 5])), lib(np.array([5, 5, 5])))
        assert (out["dropped"], np.asarray(out["env"]).tolist(), np.asarray(cur).tolist()) == (1, [], [5, 5, 5])
        # a masked clear: envs 0 and 2 lose carry, stamps and cursor; env 1 keeps all three
        head, cursor, cy = lib(m.head), lib(np.array([5, 4, 5])), lib(carry)
        em.clear(head, cursor, cy, lib(np.array([1, 0, 1], np.uint8)))
        assert np.asarray(head).tolist() == [[-1, -1], [4, 3], [-1, -1]] and np.asarray(cursor).tolist() == [0, 4, 0]
        assert np.asarray(cy).sum(1).tolist() == [0, 176, 0]
        out, cur = em.drain(lib(m.vals), lib(m.cnts), head, cursor, lib(np.array([0, 5, 0])))
        assert (out["dropped"], np.asarray(out["env"]).tolist(), np.asarray(out["episode"]).tolist()) == (0, [1], [4])
        em.clear(head, cursor, cy)
        assert (np.asarray(head) == -1).all() and not np.asarray(cursor).any() and not np.asarray(cy).any()
    # the reference's own clear does the same to its buffers and forgets the running episode
    m.clear(np.array([1, 0, 1]))
    assert m.head.tolist() == [[-1, -1], [4, 3], [-1, -1]] and m.started.tolist() == [False, True, False]


def test_processing_in_pieces_equals_one_call_in_the_reference():
    rows, ep, whole = _five_episodes()
    for cut in (1, 2, 7, rows.shape[0] - 1):
        m = ref.Metrics(3, 2, 2, dt=0.1, getting_close_range=0.2).process(rows[:cut], ep[:cut]).process(rows[cut:], ep[cut:])
        assert np.array_equal(m.vals, whole.vals, equal_nan=True) and np.array_equal(m.cnts, whole.cnts)
        assert np.array_equal(m.head, whole.head)


def test_join_puts_the_metric_columns_beside_the_log_records():
    from gym_collision_avoidance_amd import episode_metrics as em
    log = {"env": np.array([0, 0, 1, 2]), "episode": np.array([0, 1, 0, 3])}
    met = {"env": np.array([0, 2, 1]), "episode": np.array([1, 3, 7])}
    for i, n in enumerate(em.FLOAT_COLUMNS + em.INT_COLUMNS):
        met[n] = np.arange(6).reshape(3, 2) + 10 * i
    li, cols = em.join(log, met)
    assert li.tolist() == [1, 3]
    assert cols["path_length"].tolist() == [[0, 1], [2, 3]] and cols["min_gap_partner"].tolist() == [[60, 61], [62, 63]]


# ---------------------------------------------------------------- the C ABI
def test_header_declares_the_metrics_and_keeps_version_12():
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert "#define CAGPU_VERSION 12" in hdr
    body = re.search(r"typedef struct CaEpMetrics \{(.*?)\} CaEpMetrics;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = re.findall(r"(double|int32_t|void)\s*\*?\s*([\w, ]+);", body)
    assert [(t, [n.strip() for n in names.split(",")]) for t, names in members] == [
        ("double", ["vals"]), ("int32_t", ["cnts"]), ("int32_t", ["head"]), ("int32_t", ["capacity", "reserved0"]),
        ("void", ["carry"]), ("double", ["getting_close_range"])]
    decl = re.search(r"int cagpu_episode_metrics\((.*?)\);", hdr, re.S).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "const CaParams *p", "const CaTraj *traj", "int32_t n_steps", "const CaEpMetrics *m", "void *stream"]
    assert re.search(r"uint64_t cagpu_episode_metrics_carry_bytes\(const CaParams \*p\);", hdr)


def test_library_exports_and_binding_mirror_the_header():
    from gym_collision_avoidance_amd import _native as nat, core
    lib = nat.lib()
    assert lib.cagpu_version() == 12 == nat.ABI_VERSION
    assert "cagpu_episode_metrics" in nat.EXPORTS and "cagpu_episode_metrics_carry_bytes" in nat.EXPORTS
    assert lib.cagpu_episode_metrics.restype is ctypes.c_int
    assert lib.cagpu_episode_metrics_carry_bytes.restype is ctypes.c_uint64
    P = ctypes.sizeof(ctypes.c_void_p)
    M = nat.CaEpMetrics
    assert [f[0] for f in M._fields_] == ["vals", "cnts", "head", "capacity", "reserved0", "carry", "getting_close_range"]
    assert (M.vals.offset, M.cnts.offset, M.head.offset) == (0, P, 2 * P)
    assert (M.capacity.offset, M.reserved0.offset, M.carry.offset) == (3 * P, 3 * P + 4, 3 * P + 8)
    assert M.getting_close_range.offset == 4 * P + 8 and ctypes.sizeof(M) == 4 * P + 16
    assert len(lib.cagpu_episode_metrics.argtypes) == 5
    # the carry: 80 bytes per agent slot and 16 per env, a multiple of 16 per env; nothing for sizes the kernel does not take
    B = ctypes.byref
    assert lib.cagpu_episode_metrics_carry_bytes(B(core.make_params(5, 10))) == 5 * (80 * 10 + 16)
    assert lib.cagpu_episode_metrics_carry_bytes(B(core.make_params(1, 1024))) == 80 * 1024 + 16
    bad = core.make_params(4, 10)
    bad.num_agents = 1025
    assert lib.cagpu_episode_metrics_carry_bytes(B(bad)) == 0
    assert lib.cagpu_episode_metrics_carry_bytes(None) == 0


def test_bad_arguments_return_einval_before_any_device_use():
    from gym_collision_avoidance_amd import _native as nat, core
    lib = nat.lib()
    B = ctypes.byref
    p = core.make_params(4, 10)
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    good_t = dict(rows=base, episode=base)
    good_m = dict(vals=base, cnts=base, head=base, capacity=4, carry=base, getting_close_range=0.2)

    def call(t=None, m=None, n=3, params=p):
        t, m = dict(good_t, **(t or {})), dict(good_m, **(m or {}))
        return lib.cagpu_episode_metrics(B(params), B(nat.CaTraj(**t)), n, B(nat.CaEpMetrics(**m)), None)

    for name in good_t:          # NULL and misaligned tape pointers
        assert call(t={name: None}) == nat.CA_EINVAL and b"cagpu_episode_metrics" in lib.cagpu_last_error()
    assert call(t={"rows": base + 8}) == nat.CA_EINVAL and b"aligned" in lib.cagpu_last_error()
    assert call(t={"episode": base + 2}) == nat.CA_EINVAL
    for name in ("vals", "cnts", "head", "carry"):
        assert call(m={name: None}) == nat.CA_EINVAL
        assert call(m={name: base + (2 if name == "head" else 8)}) == nat.CA_EINVAL and b"aligned" in lib.cagpu_last_error()
    for cap in (0, -3):
        assert call(m={"capacity": cap}) == nat.CA_EINVAL and b"capacity" in lib.cagpu_last_error()
    assert call(n=-1) == nat.CA_EINVAL and b"n_steps" in lib.cagpu_last_error()
    assert call(n=0) == nat.CA_OK        # nothing to do: returns before any launch
    big = core.make_params(4, 10)
    big.num_agents = 1025
    assert call(params=big) == nat.CA_EINVAL
    assert lib.cagpu_episode_metrics(None, None, 1, None, None) == nat.CA_EINVAL
    assert lib.cagpu_episode_metrics(B(p), None, 1, B(nat.CaEpMetrics(**good_m)), None) == nat.CA_EINVAL
    assert lib.cagpu_episode_metrics(B(p), B(nat.CaTraj(**good_t)), 1, None, None) == nat.CA_EINVAL
