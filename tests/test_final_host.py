"""The final record without a GPU: the C ABI of cagpu_step_final / cagpu_rollout_final (include/cagpu.h CaFinal), its
ctypes mirror, the argument checks that return before anything is launched, and the host-side flag decoding."""
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


def test_header_declares_the_final_record_and_keeps_version_12():
    hdr = _header()
    assert "#define CAGPU_VERSION 12" in hdr
    assert "typedef struct CaFinal" in hdr
    assert "int cagpu_step_final(" in hdr and "int cagpu_rollout_final(" in hdr
    # the struct is two pointers, observation block first
    body = re.search(r"typedef struct CaFinal \{(.*?)\} CaFinal;", hdr, re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t)\s*\*(\w+);", body, re.M)
    assert fields == [("float", "obs"), ("uint32_t", "flags")]
    # both calls take the optional tape right in front of the record, and the stream last
    for name in ("cagpu_step_final", "cagpu_rollout_final"):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        args = [a.strip() for a in decl.replace("\n", " ").split(",")]
        assert args[-3:] == ["const CaTraj *traj", "const CaFinal *fin", "void *stream"], args


def test_library_exports_and_binding_mirror_the_header():
    from gym_collision_avoidance_amd import _native as nat
    lib = nat.lib()
    assert lib.cagpu_version() == 12 == nat.ABI_VERSION
    for n in ("cagpu_step_final", "cagpu_rollout_final"):
        assert n in nat.EXPORTS
        assert getattr(lib, n).restype is ctypes.c_int
    P = ctypes.sizeof(ctypes.c_void_p)
    assert ctypes.sizeof(nat.CaFinal) == 2 * P
    assert nat.CaFinal.obs.offset == 0 and nat.CaFinal.flags.offset == P
    assert len(lib.cagpu_step_final.argtypes) == 10 and len(lib.cagpu_rollout_final.argtypes) == 11
    # the flag constants the decoder tests are those of the header
    hdr = _header()
    for name, val in (("CA_AT_GOAL", nat.AT_GOAL), ("CA_IN_COLLISION", nat.IN_COLLISION), ("CA_OUT_OF_TIME", nat.OUT_OF_TIME),
                      ("CA_DONE", nat.DONE), ("CA_ABSENT", nat.ABSENT), ("CA_PLAN_VALID", nat.PLAN_VALID)):
        sh = int(re.search(r"%s = 1u << (\d+)" % name, hdr).group(1))
        assert val == 1 << sh, name
    assert not nat.KERNEL_FLAG_BITS & nat.PLAN_VALID
    assert nat.KERNEL_FLAG_BITS & nat.ABSENT and nat.KERNEL_FLAG_BITS & nat.OUT_OF_TIME


def test_final_calls_with_bad_arguments_return_einval_before_any_device_use():
    from gym_collision_avoidance_amd import _native as nat, core
    lib = nat.lib()
    B = ctypes.byref
    p, s, o = core.make_params(4, 10), nat.CaState(), nat.CaOut()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ar = nat.CaAutoReset(table=base, n_cases=1, env_id_offset=0, case_stride=4)

    def step(fin, ar_=B(ar)):
        return lib.cagpu_step_final(B(p), B(s), B(o), None, ar_, None, None, None, fin, None)

    def roll(fin, ar_=B(ar), ring=1):
        return lib.cagpu_rollout_final(B(p), B(s), B(o), None, ar_, 3, ring, 0, None, fin, None)

    for call in (step, roll):
        # NULL record / NULL observation block
        for fin in (None, B(nat.CaFinal(obs=None, flags=None)), B(nat.CaFinal(obs=None, flags=base))):
            assert call(fin) == nat.CA_EINVAL
            assert b"CaFinal" in lib.cagpu_last_error()
        # unaligned pointers
        assert call(B(nat.CaFinal(obs=base + 4, flags=base))) == nat.CA_EINVAL
        assert b"aligned" in lib.cagpu_last_error()
        assert call(B(nat.CaFinal(obs=base, flags=base + 2))) == nat.CA_EINVAL
        assert b"aligned" in lib.cagpu_last_error()
        # a record without auto-reset: nothing is ever overwritten
        assert call(B(nat.CaFinal(obs=base, flags=base)), None) == nat.CA_EINVAL
        assert b"CaAutoReset" in lib.cagpu_last_error()
        # a good record gets as far as the checks of the mirrored call (NULL state pointers here): still no launch
        assert call(B(nat.CaFinal(obs=base, flags=None))) == nat.CA_EINVAL
        assert b"CaFinal" not in lib.cagpu_last_error()
    # everything NULL
    assert lib.cagpu_step_final(None, None, None, None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_rollout_final(None, None, None, None, None, 3, 1, 0, None, None, None) == nat.CA_EINVAL
    # the tape's own checks still apply when a tape is given
    fin = B(nat.CaFinal(obs=base, flags=base))
    assert lib.cagpu_step_final(B(p), B(s), B(o), None, B(ar), None, None, B(nat.CaTraj(rows=None, episode=None)), fin,
                                None) == nat.CA_EINVAL
    assert b"CaTraj" in lib.cagpu_last_error()
    # a map and a map set at once / a snapshot without a ring
    m, ms = nat.CaMap(), nat.CaMapSet()
    assert lib.cagpu_step_final(B(p), B(s), B(o), None, B(ar), B(m), B(ms), None, fin, None) == nat.CA_EINVAL
    assert lib.cagpu_rollout_final(B(p), B(s), B(o), None, B(ar), 3, 0, 256, None, fin, None) == nat.CA_EINVAL


def test_decode_flags_on_hand_made_words():
    from gym_collision_avoidance_amd import _native as nat
    rvo_uni = (nat.POL_RVO << nat.POLICY_SHIFT) | (nat.DYN_UNICYCLE << nat.DYNAMICS_SHIFT)
    words = np.array([
        0,                                                                      # still running
        nat.AT_GOAL | nat.DONE,                                                 # reached the goal this step
        nat.AT_GOAL | nat.WAS_AT_GOAL | nat.DONE | nat.PLAN_VALID,              # ... earlier (the plan bit means nothing here)
        nat.IN_COLLISION | nat.DONE | nat.IS_LEARNING | nat.STILL_LEARNING,     # a learner that collided
        nat.OUT_OF_TIME | nat.DONE | rvo_uni | (3 << nat.POLICY_SHIFT),         # timed out, ids in the upper bits
        nat.OUT_OF_TIME | nat.IN_COLLISION | nat.WAS_IN_COLLISION | nat.DONE,   # collided earlier, clock ran out since
        nat.ABSENT | nat.DONE | nat.AT_GOAL | nat.WAS_AT_GOAL,                  # an empty slot of a ragged batch
    ], dtype=np.uint32)
    want = {"at_goal":         [0, 1, 1, 0, 0, 0, 1],
            "in_collision":    [0, 0, 0, 1, 0, 1, 0],
            "ran_out_of_time": [0, 0, 0, 0, 1, 1, 0],
            "done":            [0, 1, 1, 1, 1, 1, 1],
            "absent":          [0, 0, 0, 0, 0, 0, 1]}
    for src in (words, words.view(np.int32), words.reshape(7, 1), words.tolist()):
        got = nat.decode_flags(src)
        assert set(got) == set(want)
        for name, bits in want.items():
            g = np.asarray(got[name])
            assert g.dtype == bool and g.shape == np.asarray(src).shape, name
            assert g.reshape(-1).tolist() == [bool(b) for b in bits], name
    # the sign bit of an int32 bit pattern does not leak into the decoded bits
    assert not any(bool(np.asarray(v)) for v in nat.decode_flags(np.int32(-2147483648)).values())
    one = nat.decode_flags(int(nat.OUT_OF_TIME | nat.DONE))
    assert one["ran_out_of_time"] is True and one["at_goal"] is False and one["absent"] is False
    # torch tensors (as the simulator keeps its flag words: int32) decode without leaving torch
    import torch
    t = nat.decode_flags(torch.from_numpy(words.view(np.int32).copy()))
    for name, bits in want.items():
        assert t[name].dtype == torch.bool and t[name].tolist() == [bool(b) for b in bits], name
