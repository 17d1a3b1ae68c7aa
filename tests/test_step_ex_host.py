"""The general step entry point without a GPU: the C ABI of cagpu_step_ex / CaStepEx (include/cagpu.h), its ctypes mirror,
and the argument checks that return before anything is launched.  Every bad-argument case that test_host_logic.py,
test_trajectory_host.py, test_final_host.py, test_episode_log_host.py and test_map_set_host.py put through one of the older
entry points is put through cagpu_step_ex with the equivalent CaStepEx here: same return code, same cagpu_last_error()
text.  The one part of a text that may differ is the entry point's OWN NAME where a message carries it ("cagpu_step_traj:
a CaMap and a CaMapSet at once"): it is rewritten to cagpu_step_ex before the comparison.

What cagpu_step_ex cannot express is the older entry points' "my record may not be NULL": a NULL pointer in a CaStepEx
means "not used".  Those cases are marked text=False below -- the equivalent CaStepEx is the same call without the record,
which is rejected too (the state pointers are NULL) with the message of THAT check, so only the return code is compared.
cagpu_step_maps(set = NULL) on otherwise good arguments has no bad CaStepEx at all (it would be a plain step): left out."""
import ctypes
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

B, A = ctypes.byref, ctypes.addressof


def _nat():
    from gym_collision_avoidance_amd import _native as nat
    return nat, nat.lib()


def test_header_binding_and_library_agree_on_the_general_entry_point():
    nat, lib = _nat()
    hdr = open(os.path.join(REPO, "include", "cagpu.h")).read()
    assert "#define CAGPU_VERSION 12" in hdr and lib.cagpu_version() == 12 == nat.ABI_VERSION
    body = re.search(r"typedef struct CaStepEx \{(.*?)\} CaStepEx;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*\*?(\w+);", body) == [("int32_t", "n_steps"), ("int32_t", "ring"), ("int64_t", "snapshot_delta"),
                                                      ("CaMap", "map"), ("CaMapSet", "set"), ("CaTraj", "traj"),
                                                      ("CaFinal", "fin"), ("CaEpLog", "log")]
    decl = re.search(r"int cagpu_step_ex\((.*?)\);", hdr, re.S).group(1)
    assert [" ".join(a.split()) for a in decl.split(",")] == [
        "const CaParams *p", "const CaState *s", "const CaOut *o", "const double *ext_actions", "const CaAutoReset *ar",
        "const CaStepEx *x", "void *stream"]
    assert "cagpu_step_ex" in set(re.findall(r"\b(cagpu_[a-z_]+)\s*\(", hdr))   # (how test_host_logic.py finds declarations)
    assert "cagpu_step_ex" in nat.EXPORTS and lib.cagpu_step_ex.restype is ctypes.c_int
    assert [f[0] for f in nat.CaStepEx._fields_] == ["n_steps", "ring", "snapshot_delta", "map", "set", "traj", "fin", "log"]
    assert ctypes.sizeof(nat.CaStepEx) == 56
    assert (nat.CaStepEx.n_steps.offset, nat.CaStepEx.ring.offset, nat.CaStepEx.snapshot_delta.offset) == (0, 4, 8)
    assert (nat.CaStepEx.map.offset, nat.CaStepEx.set.offset, nat.CaStepEx.traj.offset, nat.CaStepEx.fin.offset,
            nat.CaStepEx.log.offset) == (16, 24, 32, 40, 48)
    assert len(lib.cagpu_step_ex.argtypes) == 7
    assert lib.cagpu_step_ex.argtypes[:5] == lib.cagpu_step.argtypes[:5] and lib.cagpu_step_ex.argtypes[6] is ctypes.c_void_p
    # the eleven older names stay declared, bound and exported
    for n in ("cagpu_step", "cagpu_step_map", "cagpu_step_maps", "cagpu_step_traj", "cagpu_step_final", "cagpu_step_log",
              "cagpu_rollout", "cagpu_rollout_ring", "cagpu_rollout_traj", "cagpu_rollout_final", "cagpu_rollout_log",
              "cagpu_ring_snapshots"):
        assert n in nat.EXPORTS and re.search(r"\bint %s\(" % n, hdr) and hasattr(lib, n), n


class _Ctx(object):
    """the arguments of the older host tests (state pointers all NULL: every call is rejected before it could launch)"""

    def __init__(self):
        from gym_collision_avoidance_amd import core
        self.nat, self.lib = _nat()
        nat = self.nat
        self.p, self.s, self.o = core.make_params(4, 10), nat.CaState(), nat.CaOut()
        self.buf = (ctypes.c_double * 64)()
        base = A(self.buf)
        self.base = base + (-base) % 16
        self.ar = nat.CaAutoReset(table=self.base, n_cases=1, env_id_offset=0, case_stride=4)
        self.m, self.ms = nat.CaMap(), nat.CaMapSet()
        self.keep = []

    def ptr(self, struct):
        """address of a record struct for a CaStepEx field (None stays None)"""
        if struct is None:
            return None
        self.keep.append(struct)
        return A(struct)

    def ref(self, struct):
        return None if struct is None else B(struct)


def _cases():
    """(label, older entry point, its trailing arguments after (p, s, o, ext, ar) as a function of the context,
    with_ar, the equivalent CaStepEx fields as a function of the context, compare the text too)"""
    out = []

    def add(label, name, tail, ex, ar=True, text=True):
        out.append(pytest.param(name, tail, ex, ar, text, id=label))

    T = lambda c, **kw: c.nat.CaTraj(**kw)
    F = lambda c, **kw: c.nat.CaFinal(**kw)
    L = lambda c, **kw: c.nat.CaEpLog(**kw)

    # ---- test_trajectory_host.py (no CaAutoReset in its calls)
    for i, mk in enumerate((lambda c: T(c, rows=None, episode=None), lambda c: T(c, rows=None, episode=c.base))):
        add("traj-null-rows-%d-step" % i, "cagpu_step_traj", lambda c, mk=mk: (None, None, mk(c)),
            lambda c, mk=mk: dict(n_steps=1, traj=mk(c)), ar=False)
        add("traj-null-rows-%d-rollout" % i, "cagpu_rollout_traj", lambda c, mk=mk: (5, 0, 0, mk(c)),
            lambda c, mk=mk: dict(n_steps=5, traj=mk(c)), ar=False)
    add("traj-null-step", "cagpu_step_traj", lambda c: (None, None, None), lambda c: dict(n_steps=1), ar=False, text=False)
    add("traj-null-rollout", "cagpu_rollout_traj", lambda c: (5, 0, 0, None), lambda c: dict(n_steps=5), ar=False, text=False)
    for i, mk in enumerate((lambda c: T(c, rows=c.base + 8, episode=None), lambda c: T(c, rows=c.base, episode=c.base + 2))):
        add("traj-misaligned-%d-step" % i, "cagpu_step_traj", lambda c, mk=mk: (None, None, mk(c)),
            lambda c, mk=mk: dict(n_steps=1, traj=mk(c)), ar=False)
        add("traj-misaligned-%d-ring" % i, "cagpu_rollout_traj", lambda c, mk=mk: (5, 1, 0, mk(c)),
            lambda c, mk=mk: dict(n_steps=5, ring=1, traj=mk(c)), ar=False)
    ok_t = lambda c: T(c, rows=c.base, episode=None)
    add("traj-good-null-state", "cagpu_step_traj", lambda c: (None, None, ok_t(c)), lambda c: dict(n_steps=1, traj=ok_t(c)),
        ar=False)
    add("traj-map-and-set", "cagpu_step_traj", lambda c: (c.m, c.ms, ok_t(c)),
        lambda c: dict(n_steps=1, map=c.m, set=c.ms, traj=ok_t(c)), ar=False)
    add("traj-delta-without-ring", "cagpu_rollout_traj", lambda c: (5, 0, 64, ok_t(c)),
        lambda c: dict(n_steps=5, snapshot_delta=64, traj=ok_t(c)), ar=False)

    # ---- test_final_host.py: step = (map, set, traj, fin), roll = (3, ring = 1, 0, traj, fin)
    def both(label, fin, ar=True, text=True, traj=lambda c: None, tag="final"):
        add("%s-%s-step" % (tag, label), "cagpu_step_final", lambda c: (None, None, traj(c), fin(c)),
            lambda c: dict(n_steps=1, traj=traj(c), fin=fin(c)), ar=ar, text=text)
        add("%s-%s-ring" % (tag, label), "cagpu_rollout_final", lambda c: (3, 1, 0, traj(c), fin(c)),
            lambda c: dict(n_steps=3, ring=1, traj=traj(c), fin=fin(c)), ar=ar, text=text)

    both("null", lambda c: None, text=False)
    both("null-obs-0", lambda c: F(c, obs=None, flags=None))
    both("null-obs-1", lambda c: F(c, obs=None, flags=c.base))
    both("misaligned-obs", lambda c: F(c, obs=c.base + 4, flags=c.base))
    both("misaligned-flags", lambda c: F(c, obs=c.base, flags=c.base + 2))
    both("without-ar", lambda c: F(c, obs=c.base, flags=c.base), ar=False)
    both("good-null-state", lambda c: F(c, obs=c.base, flags=None))
    ok_f = lambda c: F(c, obs=c.base, flags=c.base)
    add("final-bad-tape", "cagpu_step_final", lambda c: (None, None, T(c, rows=None, episode=None), ok_f(c)),
        lambda c: dict(n_steps=1, traj=T(c, rows=None, episode=None), fin=ok_f(c)))
    add("final-map-and-set", "cagpu_step_final", lambda c: (c.m, c.ms, None, ok_f(c)),
        lambda c: dict(n_steps=1, map=c.m, set=c.ms, fin=ok_f(c)))
    add("final-delta-without-ring", "cagpu_rollout_final", lambda c: (3, 0, 256, None, ok_f(c)),
        lambda c: dict(n_steps=3, snapshot_delta=256, fin=ok_f(c)))

    # ---- test_episode_log_host.py: step = (map, set, traj, fin, log), roll = (3, ring = 1, 0, traj, fin, log)
    def lboth(label, log, ar=True, text=True, fin=lambda c: None, traj=lambda c: None):
        add("log-%s-step" % label, "cagpu_step_log", lambda c: (None, None, traj(c), fin(c), log(c)),
            lambda c: dict(n_steps=1, traj=traj(c), fin=fin(c), log=log(c)), ar=ar, text=text)
        add("log-%s-ring" % label, "cagpu_rollout_log", lambda c: (3, 1, 0, traj(c), fin(c), log(c)),
            lambda c: dict(n_steps=3, ring=1, traj=traj(c), fin=fin(c), log=log(c)), ar=ar, text=text)

    lboth("null", lambda c: None, text=False)
    lboth("null-both", lambda c: L(c, rows=None, head=None, capacity=4))
    lboth("null-rows", lambda c: L(c, rows=None, head=c.base, capacity=4))
    lboth("null-head", lambda c: L(c, rows=c.base, head=None, capacity=4))
    for i, (dr, dh) in enumerate(((8, 0), (0, 4), (0, 8))):
        lboth("misaligned-%d" % i, lambda c, dr=dr, dh=dh: L(c, rows=c.base + dr, head=c.base + dh, capacity=4))
    for cap in (0, -3):
        lboth("capacity-%d" % cap, lambda c, cap=cap: L(c, rows=c.base, head=c.base, capacity=cap))
    lboth("without-ar", lambda c: L(c, rows=c.base, head=c.base, capacity=4), ar=False)
    good = lambda c: L(c, rows=c.base, head=c.base, capacity=1)
    lboth("good-null-state", good)
    lboth("bad-final", good, fin=lambda c: F(c, obs=None, flags=None))
    lboth("bad-tape", good, traj=lambda c: T(c, rows=None, episode=None))
    add("log-map-and-set", "cagpu_step_log", lambda c: (c.m, c.ms, None, None, good(c)),
        lambda c: dict(n_steps=1, map=c.m, set=c.ms, log=good(c)))
    add("log-delta-without-ring", "cagpu_rollout_log", lambda c: (3, 0, 256, None, None, good(c)),
        lambda c: dict(n_steps=3, snapshot_delta=256, log=good(c)))
    return out


@pytest.mark.parametrize("name,tail,ex,with_ar,text", _cases())
def test_bad_arguments_of_the_older_entry_points_fail_the_same_way_through_step_ex(name, tail, ex, with_ar, text):
    c = _Ctx()
    lib, nat = c.lib, c.nat
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    ar = B(c.ar) if with_ar else None
    old_args = [c.ref(a) if isinstance(a, ctypes.Structure) else a for a in tail(c)]
    rc_old = getattr(lib, name)(B(c.p), B(c.s), B(c.o), None, ar, *old_args, None)
    msg_old = lib.cagpu_last_error()
    fields = {k: (c.ptr(v) if isinstance(v, ctypes.Structure) else v) for k, v in ex(c).items()}
    rc_new = lib.cagpu_step_ex(B(c.p), B(c.s), B(c.o), None, ar, B(nat.CaStepEx(**fields)), None)
    msg_new = lib.cagpu_last_error()
    assert rc_old == nat.CA_EINVAL and rc_new == rc_old, (rc_old, rc_new, msg_old, msg_new)
    if text:
        assert msg_new == msg_old.replace(name.encode(), b"cagpu_step_ex"), (msg_old, msg_new)
    assert lib.cagpu_last_kernel() == before      # nothing was selected, let alone launched


def test_everything_null_fails_the_same_way():
    """test_host_logic.py: cagpu_step(None ...); the *_host.py files: their entry point with every pointer NULL"""
    nat, lib = _nat()
    assert lib.cagpu_step(None, None, None, None, None, None) == nat.CA_EINVAL
    want = lib.cagpu_last_error()
    assert b"NULL" in want
    assert lib.cagpu_step_ex(None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_last_error() == want
    for fields in (dict(n_steps=1), dict(n_steps=3, ring=1)):
        assert lib.cagpu_step_ex(None, None, None, None, None, B(nat.CaStepEx(**fields)), None) == nat.CA_EINVAL
        assert lib.cagpu_last_error() == want
    # (the older recording entry points name their missing record first: a code, not a text, to compare)
    assert lib.cagpu_step_traj(None, None, None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_rollout_final(None, None, None, None, None, 3, 1, 0, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_step_log(None, None, None, None, None, None, None, None, None, None, None) == nat.CA_EINVAL


def _fake(nat):
    """host structs whose device pointers are never dereferenced (test_map_set_host.py): the calls below get past the NULL
    checks and fail a later argument check, still before anything is launched"""
    from gym_collision_avoidance_amd import core
    p = core.make_params(4, 4)
    fake = 0x1000
    s = nat.CaState(**{n: fake for n in nat.STATE_FIELDS if n not in ("next_action", "turning_dir", "rvo_collab",
                                                                       "rvo_heading_noise", "ext_state")})
    o = nat.CaOut(obs=fake, rewards=fake, done=fake, game_over=fake)
    m = nat.CaMap(static_bits=0x2000, rows=160, cols=160, cell=0.1, origin_r=80.0, origin_c=80.0)
    ms = nat.CaMapSet(map=m, env_map=0x2000, num_maps=3, map_seed=7)
    return p, s, o, m, ms


@pytest.mark.parametrize("what", ["null_env_map", "null_bits", "zero_maps", "negative_maps", "rows", "cols", "cell"])
def test_bad_map_sets_fail_the_same_way_through_step_ex(what):
    """test_map_set_host.py's cases (all but null_set, see the module docstring)"""
    nat, lib = _nat()
    p, s, o, _, ms = _fake(nat)
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
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()
    assert lib.cagpu_step_maps(B(p), B(s), B(o), None, None, B(ms), None) == nat.CA_EINVAL
    want = lib.cagpu_last_error()
    assert b"CaMapSet" in want
    assert lib.cagpu_step_ex(B(p), B(s), B(o), None, None, B(nat.CaStepEx(n_steps=1, set=A(ms))), None) == nat.CA_EINVAL
    assert lib.cagpu_last_error() == want
    assert lib.cagpu_last_kernel() == before


def test_rules_only_the_general_entry_point_can_break():
    nat, lib = _nat()
    p, s, o, m, ms = _fake(nat)
    lib.cagpu_last_kernel.restype = ctypes.c_char_p
    before = lib.cagpu_last_kernel()

    def ex(**fields):
        rc = lib.cagpu_step_ex(B(p), B(s), B(o), None, None, B(nat.CaStepEx(**fields)), None)
        return rc, lib.cagpu_last_error()

    # the n-step kernels take no map: no older entry point reaches such a launch, neither does this one
    for fields in (dict(n_steps=3, map=A(m)), dict(n_steps=1, ring=1, map=A(m)), dict(n_steps=3, set=A(ms)),
                   dict(n_steps=1, ring=1, set=A(ms)), dict(n_steps=4, ring=1, set=A(ms))):
        rc, msg = ex(**fields)
        assert rc == nat.CA_EINVAL and b"cagpu_step_ex" in msg and b"n_steps > 1 or ring" in msg, (fields, rc, msg)
    rc, msg = ex(n_steps=1, map=A(m), set=A(ms))
    assert rc == nat.CA_EINVAL and b"a CaMap and a CaMapSet at once" in msg
    for fields in (dict(n_steps=1, snapshot_delta=256), dict(n_steps=5, snapshot_delta=-16)):
        rc, msg = ex(**fields)
        assert rc == nat.CA_EINVAL and b"snapshot_delta without ring" in msg, (fields, rc, msg)
    for n in (0, -1):
        for ring in (0, 1):
            rc, msg = ex(n_steps=n, ring=ring)
            assert rc == nat.CA_EINVAL and b"n_steps must be >= 1" in msg, (n, ring, rc, msg)
    # the per-step inputs belong to ONE step
    s.ext_state = 0x1000
    for fields in (dict(n_steps=2), dict(n_steps=1, ring=1)):
        rc, msg = ex(**fields)
        assert rc == nat.CA_EINVAL and b"ONE step" in msg, (fields, rc, msg)
    s.ext_state = None
    # all-NULL arguments, with and without a CaStepEx
    assert lib.cagpu_step_ex(None, None, None, None, None, None, None) == nat.CA_EINVAL
    assert lib.cagpu_step_ex(None, None, None, None, None, B(nat.CaStepEx()), None) == nat.CA_EINVAL
    assert lib.cagpu_last_kernel() == before      # nothing was selected, let alone launched
