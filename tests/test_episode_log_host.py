"""The episode log without a GPU: the C ABI of cagpu_step_log / cagpu_rollout_log (include/cagpu.h CaEpLog), its ctypes
mirror, the argument checks that return before anything is launched, and the slot / cursor / dropped arithmetic of
gym_collision_avoidance_amd/episodes.py on hand-made numpy buffers."""
import ctypes
import os
import re
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def _header():
    return open(os.path.join(REPO, "include", "cagpu.h")).read()


def test_header_declares_the_episode_log_and_keeps_version_12():
    hdr = _header()
    assert "#define CAGPU_VERSION 12" in hdr
    body = re.search(r"typedef struct CaEpLog \{(.*?)\} CaEpLog;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(double|int32_t)\s*\*(\w+);", body) == [("double", "rows"), ("int32_t", "head")]
    assert re.search(r"int32_t\s+capacity,\s*reserved0;", body)
    assert body.index("rows") < body.index("head") < body.index("capacity")
    for name in ("cagpu_step_log", "cagpu_rollout_log"):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        args = [" ".join(a.split()) for a in decl.split(",")]
        assert args[-4:] == ["const CaTraj *traj", "const CaFinal *fin", "const CaEpLog *log", "void *stream"], args
    # the calls mirror the final record's, with one more argument
    n_args = lambda name: len(re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1).split(","))
    assert n_args("cagpu_step_log") == n_args("cagpu_step_final") + 1 == 11
    assert n_args("cagpu_rollout_log") == n_args("cagpu_rollout_final") + 1 == 12


def test_library_exports_and_binding_mirror_the_header():
    from gym_collision_avoidance_amd import _native as nat
    lib = nat.lib()
    assert lib.cagpu_version() == 12 == nat.ABI_VERSION
    for n in ("cagpu_step_log", "cagpu_rollout_log"):
        assert n in nat.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    P = ctypes.sizeof(ctypes.c_void_p)
    assert [f[0] for f in nat.CaEpLog._fields_] == ["rows", "head", "capacity", "reserved0"]
    assert ctypes.sizeof(nat.CaEpLog) == 2 * P + 8
    assert (nat.CaEpLog.rows.offset, nat.CaEpLog.head.offset) == (0, P)
    assert (nat.CaEpLog.capacity.offset, nat.CaEpLog.reserved0.offset) == (2 * P, 2 * P + 4)
    assert len(lib.cagpu_step_log.argtypes) == 11 and len(lib.cagpu_rollout_log.argtypes) == 12
    assert lib.cagpu_step_log.argtypes[:-2] + [lib.cagpu_step_log.argtypes[-1]] == lib.cagpu_step_final.argtypes
    assert lib.cagpu_rollout_log.argtypes[:-2] + [lib.cagpu_rollout_log.argtypes[-1]] == lib.cagpu_rollout_final.argtypes


def test_log_calls_with_bad_arguments_return_einval_before_any_device_use():
    from gym_collision_avoidance_amd import _native as nat, core
    lib = nat.lib()
    B = ctypes.byref
    p, s, o = core.make_params(4, 10), nat.CaState(), nat.CaOut()
    buf = (ctypes.c_double * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ar = nat.CaAutoReset(table=base, n_cases=1, env_id_offset=0, case_stride=4)
    L = nat.CaEpLog

    def step(log, ar_=B(ar), fin=None, traj=None):
        return lib.cagpu_step_log(B(p), B(s), B(o), None, ar_, None, None, traj, fin, log, None)

    def roll(log, ar_=B(ar), fin=None, traj=None, ring=1):
        return lib.cagpu_rollout_log(B(p), B(s), B(o), None, ar_, 3, ring, 0, traj, fin, log, None)

    for call in (step, roll):
        # NULL log / rows / head
        for log in (None, B(L(rows=None, head=None, capacity=4)), B(L(rows=None, head=base, capacity=4)),
                    B(L(rows=base, head=None, capacity=4))):
            assert call(log) == nat.CA_EINVAL
            assert b"CaEpLog" in lib.cagpu_last_error()
        # misaligned pointers (16 bytes each)
        for rows, head in ((base + 8, base), (base, base + 4), (base, base + 8)):
            assert call(B(L(rows=rows, head=head, capacity=4))) == nat.CA_EINVAL
            assert b"CaEpLog" in lib.cagpu_last_error() and b"aligned" in lib.cagpu_last_error()
        # capacity < 1
        for cap in (0, -3):
            assert call(B(L(rows=base, head=base, capacity=cap))) == nat.CA_EINVAL
            assert b"CaEpLog.capacity" in lib.cagpu_last_error()
        # no CaAutoReset: no episode is ever logged
        assert call(B(L(rows=base, head=base, capacity=4)), None) == nat.CA_EINVAL
        assert b"CaEpLog" in lib.cagpu_last_error() and b"CaAutoReset" in lib.cagpu_last_error()
        # a good log gets as far as the checks of the mirrored call (NULL state pointers here): still no launch
        good = B(L(rows=base, head=base, capacity=1))
        assert call(good) == nat.CA_EINVAL
        assert b"CaEpLog" not in lib.cagpu_last_error()
        # the optional final record and tape keep their own checks
        assert call(good, fin=B(nat.CaFinal(obs=None, flags=None))) == nat.CA_EINVAL
        assert b"CaFinal" in lib.cagpu_last_error()
        assert call(good, traj=B(nat.CaTraj(rows=None, episode=None))) == nat.CA_EINVAL
        assert b"CaTraj" in lib.cagpu_last_error()
    # everything NULL
    assert lib.cagpu_step_log(None, None, None, None, None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_rollout_log(None, None, None, None, None, 3, 1, 0, None, None, None, None) == nat.CA_EINVAL
    # a map and a map set at once / a snapshot without a ring
    good = B(L(rows=base, head=base, capacity=1))
    m, ms = nat.CaMap(), nat.CaMapSet()
    assert lib.cagpu_step_log(B(p), B(s), B(o), None, B(ar), B(m), B(ms), None, None, good, None) == nat.CA_EINVAL
    assert b"CaMapSet" in lib.cagpu_last_error()
    assert lib.cagpu_rollout_log(B(p), B(s), B(o), None, B(ar), 3, 0, 256, None, None, good, None) == nat.CA_EINVAL
    assert b"snapshot_delta" in lib.cagpu_last_error()


# ---------------------------------------------------------------- episodes.py on hand-made buffers
def _write(rows, head, e, k, steps=7, case=0, outcome=1, flags=None):
    """what the kernel stores for env e's k-th episode"""
    C, N = rows.shape[1], rows.shape[2]
    sl = k % C
    head[e, sl] = (k, steps, case, outcome)
    for a in range(N):
        rows[e, sl, a, :3] = (100 * e + k + 0.25 * a, 10 * e + k + 0.5, k - 0.125 * a)
    fl = np.full(N, 0x21, np.uint32) if flags is None else np.asarray(flags, np.uint32)
    rows[e, sl, :, 3] = fl.astype(np.uint64).view(np.float64)


def _buffers(E, C, N=2):
    return np.zeros((E, C, N, 4)), np.full((E, C, 4), -1, np.int32), np.zeros(E, np.int64)


def test_drain_orders_by_env_then_episode_and_advances_the_cursor():
    from gym_collision_avoidance_amd import episodes as ep
    rows, head, cur = _buffers(3, 4)
    for e, k in ((2, 0), (0, 0), (2, 1), (0, 1), (0, 2), (2, 2)):   # (written in no particular order; env 1 ends nothing)
        _write(rows, head, e, k, steps=10 * e + k, case=(e + 3 * k) % 5, outcome=k % 3)
    out, cur = ep.drain(rows, head, cur, np.array([3, 0, 3]))
    assert out["env"].tolist() == [0, 0, 0, 2, 2, 2]
    assert out["episode"].tolist() == [0, 1, 2, 0, 1, 2]
    assert out["steps"].tolist() == [0, 1, 2, 20, 21, 22]
    assert out["case"].tolist() == [0, 3, 1, 2, 0, 3]
    assert out["outcome"].tolist() == [0, 1, 2, 0, 1, 2]
    assert out["total_reward"].tolist() == [[0.0, 0.25], [1.0, 1.25], [2.0, 2.25], [200.0, 200.25], [201.0, 201.25], [202.0, 202.25]]
    assert out["time_to_goal"][:, 0].tolist() == [0.5, 1.5, 2.5, 20.5, 21.5, 22.5]
    assert out["extra_time_to_goal"][:, 1].tolist() == [-0.125, 0.875, 1.875, -0.125, 0.875, 1.875]
    assert out["flags"].dtype == np.int32 and out["flags"].tolist() == [[0x21, 0x21]] * 6
    assert out["dropped"] == 0
    assert cur.tolist() == [3, 0, 3]
    # an empty drain: nothing new, the cursor stays
    out, cur = ep.drain(rows, head, cur, np.array([3, 0, 3]))
    assert out["env"].tolist() == [] and out["total_reward"].shape == (0, 2) and out["flags"].shape == (0, 2)
    assert out["dropped"] == 0 and cur.tolist() == [3, 0, 3]
    # the next drain starts at the cursor
    _write(rows, head, 1, 0, steps=5)
    _write(rows, head, 0, 3, steps=6)
    out, cur = ep.drain(rows, head, cur, np.array([4, 1, 3]))
    assert (out["env"].tolist(), out["episode"].tolist(), out["steps"].tolist()) == ([0, 1], [3, 0], [6, 5])
    assert out["dropped"] == 0 and cur.tolist() == [4, 1, 3]


def test_drain_wraps_around_the_ring():
    from gym_collision_avoidance_amd import episodes as ep
    rows, head, cur = _buffers(1, 3)
    for k in range(7):
        _write(rows, head, 0, k, steps=k + 40)
    cur[0] = 4
    env, k, slot, dropped, new = ep.select(head, cur, np.array([7]))
    assert (env.tolist(), k.tolist(), slot.tolist(), dropped, new.tolist()) == ([0, 0, 0], [4, 5, 6], [1, 2, 0], 0, [7])
    out, _ = ep.drain(rows, head, cur, np.array([7]))
    assert out["steps"].tolist() == [44, 45, 46] and out["episode"].tolist() == [4, 5, 6]


def test_drain_counts_what_the_capacity_lost_and_returns_the_newest():
    from gym_collision_avoidance_amd import episodes as ep
    rows, head, cur = _buffers(2, 3)
    for k in range(8):
        _write(rows, head, 0, k, steps=k)
    for k in range(2):
        _write(rows, head, 1, k, steps=70 + k)
    cur[:] = (1, 0)
    out, new = ep.drain(rows, head, cur, np.array([8, 2]))
    assert out["env"].tolist() == [0, 0, 0, 1, 1] and out["episode"].tolist() == [5, 6, 7, 0, 1]
    assert out["steps"].tolist() == [5, 6, 7, 70, 71]
    assert out["dropped"] == 4          # episodes 1 .. 4 of env 0
    assert new.tolist() == [8, 2]


def test_a_stale_stamp_counts_as_dropped():
    from gym_collision_avoidance_amd import episodes as ep
    rows, head, cur = _buffers(2, 4)
    for k in range(3):
        _write(rows, head, 0, k, steps=k)
        _write(rows, head, 1, k, steps=50 + k)
    _write(rows, head, 0, 5, steps=99)     # a ring ran ahead: episode 5 of env 0 already sits in the slot of episode 1
    out, new = ep.drain(rows, head, cur, np.array([3, 3]))
    assert out["env"].tolist() == [0, 0, 1, 1, 1] and out["episode"].tolist() == [0, 2, 0, 1, 2]
    assert out["steps"].tolist() == [0, 2, 50, 51, 52]
    assert out["dropped"] == 1 and new.tolist() == [3, 3]
    # a slot never written (the stamp the caller initialised) is dropped too, not returned as garbage
    rows, head, cur = _buffers(1, 4)
    out, new = ep.drain(rows, head, cur, np.array([2]))
    assert out["env"].tolist() == [] and out["dropped"] == 2 and new.tolist() == [2]


def test_a_masked_reset_clears_one_env_only():
    from gym_collision_avoidance_amd import episodes as ep
    rows, head, cur = _buffers(3, 2)
    for e in range(3):
        for k in range(2):
            _write(rows, head, e, k, steps=10 * e + k)
    cur[:] = (1, 1, 1)
    ep.clear(head, cur, np.array([0, 1, 0], np.uint8))
    assert head[:, :, 0].tolist() == [[0, 1], [-1, -1], [0, 1]]
    assert head[:, :, 1].tolist() == [[0, 1], [10, 11], [20, 21]]      # (only the stamps are touched)
    assert cur.tolist() == [1, 0, 1]
    out, new = ep.drain(rows, head, cur, np.array([2, 0, 2]))        # (the reset env's count restarts at 0)
    assert out["env"].tolist() == [0, 2] and out["episode"].tolist() == [1, 1] and out["dropped"] == 0
    assert new.tolist() == [2, 0, 2]
    ep.clear(head, cur, None)
    assert (head[:, :, 0] == -1).all() and cur.tolist() == [0, 0, 0]


def test_drain_works_on_torch_tensors_too():
    import torch
    from gym_collision_avoidance_amd import episodes as ep
    rows, head, cur = _buffers(2, 3)
    for k in range(5):
        _write(rows, head, 1, k, steps=k, flags=[0x21, 0x10024])
    out, new = ep.drain(torch.from_numpy(rows), torch.from_numpy(head), torch.from_numpy(cur), torch.tensor([0, 5], dtype=torch.int32))
    assert out["env"].tolist() == [1, 1, 1] and out["episode"].tolist() == [2, 3, 4] and out["dropped"] == 2
    assert out["flags"].dtype == torch.int32 and out["flags"].tolist() == [[0x21, 0x10024]] * 3
    assert new.tolist() == [0, 5]
    m = torch.tensor([0, 1], dtype=torch.uint8)
    th, tc_ = torch.from_numpy(head.copy()), new.clone()
    ep.clear(th, tc_, m)
    assert th[:, :, 0].tolist() == [[-1, -1, -1], [-1, -1, -1]] and tc_.tolist() == [0, 0]


def test_outcome_and_flag_decoding_agree_with_decode_flags():
    from gym_collision_avoidance_amd import _native as nat, episodes as ep
    G, Cn, T, A = nat.AT_GOAL | nat.DONE, nat.IN_COLLISION | nat.DONE, nat.OUT_OF_TIME | nat.DONE, \
        nat.ABSENT | nat.DONE | nat.AT_GOAL | nat.WAS_AT_GOAL
    ids = (nat.POL_RVO << nat.POLICY_SHIFT) | (nat.DYN_UNICYCLE << nat.DYNAMICS_SHIFT) | nat.PLAN_VALID
    words = np.array([[G, G | ids, G | nat.WAS_AT_GOAL],          # all at goal
                      [G, Cn, Cn | ids],                          # collision
                      [G, T, G],                                  # stuck (timed out)
                      [Cn, T | ids, G],                           # collision wins over stuck
                      [G, G, A],                                  # a ragged env: the empty slot carries at_goal
                      [T, A, A]], dtype=np.uint32)                # ... and does not rescue a stuck one
    assert ep.ABSENT == nat.ABSENT
    assert ep.outcome_of(words).tolist() == [1, 0, 2, 0, 1, 2]
    d = nat.decode_flags(words)
    want = np.where(d["in_collision"].any(1), 0, np.where(d["at_goal"].all(1), 1, 2))
    assert ep.outcome_of(words).tolist() == want.tolist()
    # the words survive the trip through column 3 of the rows (bit pattern in the low half of a float64, zeros above)
    col = words.astype(np.uint64).view(np.float64)
    back = ep.flag_words(col)
    assert back.dtype == np.int32 and np.array_equal(back.view(np.uint32), words)
    for name, bits in nat.decode_flags(back).items():
        assert np.array_equal(bits, d[name]), name
    # ... and the env API's columns are what run_suite derives from the same words
    rec = {"env": np.arange(6), "episode": np.zeros(6, np.int64), "case": np.arange(6), "steps": np.full(6, 9),
           "outcome": ep.outcome_of(words), "flags": back, "dropped": 0,
           "total_reward": np.ones((6, 3)), "time_to_goal": np.full((6, 3), 2.0), "extra_time_to_goal": np.full((6, 3), 0.5)}
    cols = ep.suite_columns(rec)
    assert cols["outcome"].tolist() == ["all_at_goal", "collision", "stuck", "collision", "all_at_goal", "stuck"]
    assert cols["collision"].tolist() == [False, True, False, True, False, False]
    assert cols["all_at_goal"].tolist() == [True, False, False, False, True, False]
    assert cols["any_stuck"].tolist() == [False, False, True, True, False, True]
    assert cols["num_agents"].tolist() == [3, 3, 3, 3, 2, 1]
    assert cols["time_to_goal"][4].tolist() == [2.0, 2.0, 0.0] and cols["total_reward"][5].tolist() == [1.0, 0.0, 0.0]
    assert cols["total_time_to_goal"].tolist() == [6.0, 6.0, 6.0, 6.0, 4.0, 2.0]
    assert cols["dropped"] == 0 and cols["test_case"].tolist() == list(range(6))
