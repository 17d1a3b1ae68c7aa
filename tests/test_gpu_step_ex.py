"""cagpu_step_ex against the eleven older entry points (include/cagpu.h CaStepEx): for every older entry point and a
representative argument set, 12 steps through the old name and 12 steps through cagpu_step_ex with the equivalent CaStepEx,
from two byte-identical copies of the state slab, must leave the same BYTES everywhere -- state, outputs, tape, final
blocks, episode log, map indices, rewind snapshot -- and select the same kernel.  Both go through the same step_impl, so
anything but equality means the CaStepEx was translated wrongly.

Three kernel families (pipelined N = 3, general N = 7, large-env N = 65), clocks so short that episodes end -- and envs
auto-reset -- inside every 12-step window (asserted: the final record and the log would otherwise be compared on nothing)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tests import golden_util as gu  # noqa: E402
from tests.test_gpu_parity import _mods  # noqa: E402

pytestmark = pytest.mark.gpu

T = 12      # steps per compared window: 12 single-step launches, or one launch of n_steps = 12
CAP = 4     # episode-log slots per env: fewer than the episodes the shortest cases finish in a window (the ring wraps)

# max_time_ratio: the clock of an agent is ratio x its straight-line time; the longest straight-line time of a case is
# <= 17.1 s (n3), <= 33.7 s (n10, whose first 7 agents the general family uses) and <= 83 s (the 65-agent cases), so the
# last agent of every env times out -- and the env auto-resets -- after at most 6 / 11 / 9 steps of 0.1 s
FAMILIES = {
    "pipelined": dict(E=6, N=3, kernel="ca_pipe_kernel<3,", kw=dict(max_time_ratio=0.03)),
    "general": dict(E=6, N=7, kernel="ca_kernel<", kw=dict(max_time_ratio=0.03)),
    "large": dict(E=2, N=65, kernel="ca_big_kernel", kw=dict(max_time_ratio=0.01, max_obs=19)),
}

# (id, older entry point, what its argument set holds).  n: one launch of n_steps = T (otherwise T single steps);
# map: "map" a CaMap / "set" a CaMapSet whose auto-resets draw maps; snap: snapshot_delta != 0
PAIRS = [
    ("step", "cagpu_step", dict()),
    ("step_map", "cagpu_step_map", dict(map="map")),
    ("step_maps", "cagpu_step_maps", dict(map="set")),
    ("step_traj", "cagpu_step_traj", dict(map="map", traj=True)),
    ("step_final", "cagpu_step_final", dict(map="set", traj=True, fin=True)),
    ("step_log", "cagpu_step_log", dict(map="set", traj=True, fin=True, log=True)),
    ("step_log_alone", "cagpu_step_log", dict(log=True)),
    ("rollout", "cagpu_rollout", dict(n=True)),
    ("rollout_ring", "cagpu_rollout_ring", dict(n=True, ring=True)),
    ("rollout_ring_snap", "cagpu_rollout_ring", dict(n=True, ring=True, snap=True)),
    ("rollout_traj", "cagpu_rollout_traj", dict(n=True, traj=True)),
    ("rollout_final", "cagpu_rollout_final", dict(n=True, ring=True, traj=True, fin=True)),
    ("rollout_log", "cagpu_rollout_log", dict(n=True, fin=True, log=True)),
    ("rollout_log_ring", "cagpu_rollout_log", dict(n=True, ring=True, traj=True, fin=True, log=True)),
    ("rollout_log_ring_snap", "cagpu_rollout_log", dict(n=True, ring=True, snap=True, traj=True, fin=True, log=True)),
]
# What a family does not support: the in-kernel rewind snapshot is the pipelined n-step kernel's alone
# (cagpu_ring_snapshots() == 0 for the others, asserted below; a snapshot_delta is CA_EUNSUPPORTED there).  A map or a map
# set with the n-step kernels is not in PAIRS at all: no older entry point takes one, and cagpu_step_ex rejects it
# (tests/test_step_ex_host.py).
UNSUPPORTED = {("general", "rollout_ring_snap"), ("general", "rollout_log_ring_snap"),
               ("large", "rollout_ring_snap"), ("large", "rollout_log_ring_snap")}


def _table(N):
    if N == 65:
        from gym_collision_avoidance_amd.envs import test_cases as tc
        np.random.seed(71)
        return tc.make_testcase_huge(6, N, side_length=2.0 * np.sqrt(N) + 3.0, speed_bnds=[0.5, 1.5], radius_bnds=[0.2, 0.5])
    return np.ascontiguousarray((gu.fixtures(10) if N == 7 else gu.fixtures(N))[:24, :N])


def _wall_map():
    """Map(16 m, 16 m, 0.1 m) with a wall along x = 0, open at the very top and bottom (tests/test_gpu_final_obs.py)"""
    m = np.zeros((160, 160), dtype=bool)
    m[10:150, 78:82] = True
    return m


def _bytes(x):
    return x.contiguous().reshape(-1).view(torch.uint8)


def _same(a, b):
    return torch.equal(_bytes(a), _bytes(b))


def _run(sim, slab0, maps, name, spec, via):
    """T steps from a copy of slab0 through the older entry point `name` (via == "old") or cagpu_step_ex (via == "ex")
    -> dict of everything the launches wrote"""
    nat = _mods()[0]
    lib = nat.lib()
    E, N, W, dev = sim.E, sim.N, sim.W, sim.device
    n, ring, snap_on = bool(spec.get("n")), bool(spec.get("ring")), bool(spec.get("snap"))
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=dev)
    slab, snap = slab0.clone(), torch.zeros_like(slab0)
    d = slab.data_ptr() - sim._slab.data_ptr()
    cs = nat.CaState.from_buffer_copy(sim._cs)
    for f in nat.STATE_FIELDS:
        if getattr(cs, f):
            setattr(cs, f, getattr(cs, f) + d)
    assert not (cs.rvo_collab or cs.rvo_heading_noise or cs.ext_state)
    S = 1 if (n and not ring) else T       # output blocks: a plain n-step launch writes every step to the same one
    # CaFinal.obs must be 16-byte aligned, and a block of E * N * W floats need not be a multiple of that (N = 65 with an
    # odd W): the blocks that single-step launches are pointed at one by one lie a padded pitch apart.  (A ring launch
    # is given block 0 alone and advances the final record with the outputs itself: dense.)
    pitch = E * N * W if n else -(-E * N * W // 4) * 4
    fin_obs = full((S, pitch), -5.0, torch.float32)[:, :E * N * W].unflatten(1, (E, N, W))
    out = dict(slab=slab, obs=full((S, E, N, W), -3.0, torch.float32), rewards=full((S, E, N), -3.0, torch.float32),
               done=full((S, E, N), 7, torch.uint8), game_over=full((S, E), 7, torch.uint8),
               rows=full((T, E, N, 12), -7.0, torch.float64), episode=full((T, E), -7, torch.int32),
               fin_obs=fin_obs, fin_flags=full((S, E, N), -5, torch.int32),
               log_rows=full((E, CAP, N, 4), -9.0, torch.float64), log_head=full((E, CAP, 4), -1, torch.int32),
               env_map=maps["env_map"].clone(), kernels=[])
    if snap_on:
        out["snap"] = snap
    co = nat.CaOut.from_buffer_copy(sim._co)       # (the workspace of the large-env kernel; no actions / orca_vel record)
    co.actions, co.orca_vel = None, None
    m = maps["map"] if spec.get("map") == "map" else None
    ms = None
    if spec.get("map") == "set":
        ms = nat.CaMapSet.from_buffer_copy(maps["set"])
        ms.env_map = out["env_map"].data_ptr()
    tj = nat.CaTraj() if spec.get("traj") else None
    fn = nat.CaFinal() if spec.get("fin") else None
    lg = None
    if spec.get("log"):
        lg = nat.CaEpLog(rows=out["log_rows"].data_ptr(), head=out["log_head"].data_ptr(), capacity=CAP)
    ref = lambda x: None if x is None else C.byref(x)
    adr = lambda x: None if x is None else C.addressof(x)
    n_steps, delta = (T if n else 1), ((snap.data_ptr() - slab.data_ptr()) if snap_on else 0)
    tails = {"cagpu_step": (), "cagpu_step_map": (ref(m),), "cagpu_step_maps": (ref(ms),),
             "cagpu_step_traj": (ref(m), ref(ms), ref(tj)), "cagpu_step_final": (ref(m), ref(ms), ref(tj), ref(fn)),
             "cagpu_step_log": (ref(m), ref(ms), ref(tj), ref(fn), ref(lg)),
             "cagpu_rollout": (n_steps,), "cagpu_rollout_ring": (n_steps, delta),
             "cagpu_rollout_traj": (n_steps, int(ring), delta, ref(tj)),
             "cagpu_rollout_final": (n_steps, int(ring), delta, ref(tj), ref(fn)),
             "cagpu_rollout_log": (n_steps, int(ring), delta, ref(tj), ref(fn), ref(lg))}
    sx = nat.CaStepEx(n_steps=n_steps, ring=int(ring), snapshot_delta=delta, map=adr(m), set=adr(ms), traj=adr(tj),
                      fin=adr(fn), log=adr(lg))
    head = (C.byref(sim.p), C.byref(cs), C.byref(co), None, C.byref(sim._ar))
    for t in range(1 if n else T):
        co.obs, co.rewards = out["obs"][t].data_ptr(), out["rewards"][t].data_ptr()
        co.done, co.game_over = out["done"][t].data_ptr(), out["game_over"][t].data_ptr()
        if tj is not None:
            tj.rows, tj.episode = out["rows"][t].data_ptr(), out["episode"][t].data_ptr()
        if fn is not None:
            fn.obs, fn.flags = out["fin_obs"][t].data_ptr(), out["fin_flags"][t].data_ptr()
        if via == "old":
            rc = getattr(lib, name)(*head, *tails[name], sim._stream())
        else:   # (x == NULL is cagpu_step: the plain pair alternates between NULL and an all-default CaStepEx)
            x = None if (name == "cagpu_step" and t % 2 == 0) else C.byref(sx)
            rc = lib.cagpu_step_ex(*head, x, sim._stream())
        nat.check(rc)
        out["kernels"].append(lib.cagpu_last_kernel().decode())
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_step_ex_writes_the_bytes_of_every_older_entry_point(family):
    nat, core, orc = _mods()
    lib = nat.lib()
    f = FAMILIES[family]
    E, N = f["E"], f["N"]
    table = _table(N)
    sim = core.BatchedSim(core.make_params(E, N, **f["kw"]))
    sim.set_plugins(nat.POL_RVO)
    sim.set_fixture_table(table)
    sim.reset(table[:E])
    # a wall map, and a set of two maps (the wall, an empty one) whose auto-resets draw the env's next map
    sim.set_map(np.stack([_wall_map(), np.zeros((160, 160), dtype=bool)]), num_beams=8, num_to_store=1, map_seed=7)
    one = nat.CaMap.from_buffer_copy(sim._maps.map)    # (grid 0 of the stack: the wall)
    maps = dict(map=one, set=sim._maps, env_map=sim.env_map.clone())
    torch.cuda.synchronize()
    slab0 = sim._slab.clone()
    rc_off = sim._state["reset_count"].data_ptr() - sim._slab.data_ptr()
    resets = lambda slab: slab[rc_off:rc_off + 4 * E].view(torch.int32)
    # which families take the rewind snapshot in the kernel: exactly what UNSUPPORTED says
    can = lib.cagpu_ring_snapshots(C.byref(sim.p), C.byref(sim._cs), C.byref(sim._co), C.byref(sim._ar), T)
    assert can == (1 if family == "pipelined" else 0)
    assert ((family, "rollout_ring_snap") in UNSUPPORTED) == (can == 0)
    ran = 0
    for pid, name, spec in PAIRS:
        if (family, pid) in UNSUPPORTED:
            continue
        old = _run(sim, slab0, maps, name, spec, "old")
        new = _run(sim, slab0, maps, name, spec, "ex")
        what = "%s / %s" % (family, pid)
        assert old["kernels"][0].startswith(f["kernel"]), (what, old["kernels"][0])
        assert old["kernels"] == new["kernels"], (what, old["kernels"], new["kernels"])
        # at least one env auto-resets inside the window (here: every env does)
        ended = resets(old["slab"]) > resets(slab0)
        assert bool(ended.any()), what
        for key in ("slab", "obs", "rewards", "done", "game_over", "rows", "episode", "log_rows", "log_head", "env_map") + \
                   (("snap",) if spec.get("snap") else ()):
            assert _same(old[key], new[key]), (what, key)
        # the final blocks where game_over says so (a plain n-step launch: one block, valid for the envs that ended an episode)
        if spec.get("n") and not spec.get("ring"):
            mask = ended.unsqueeze(0)
        else:
            mask = old["game_over"] != 0
            assert int(mask.sum()) == int((resets(old["slab"]) - resets(slab0)).sum()), what   # (every game over is a reset)
        assert _same(old["fin_obs"][mask], new["fin_obs"][mask]) and _same(old["fin_flags"][mask], new["fin_flags"][mask]), what
        # ... and both runs did write what the pair is about (a comparison of two untouched buffers proves nothing)
        assert not _same(old["slab"], slab0), what
        assert bool((old["obs"] != -3.0).any()) and int(old["game_over"].max()) <= 1, what
        assert bool((old["rows"][..., 11] != -7.0).all()) == bool(spec.get("traj")), what
        assert bool((old["episode"] != -7).all()) == bool(spec.get("traj")), what
        assert bool((old["fin_flags"][mask] != -5).all()) == bool(spec.get("fin")), what
        assert bool((old["fin_obs"] != -5.0).any()) == bool(spec.get("fin")), what
        assert bool((old["log_head"][ended][..., 0] >= 0).any()) == bool(spec.get("log")), what
        if spec.get("snap"):
            assert _same(old["snap"], slab0), what      # the rewind point is the state before the call
        if spec.get("map") == "set":
            assert int(old["env_map"].min()) >= 0 and int(old["env_map"].max()) <= 1, what
        ran += 1
    assert ran == len(PAIRS) - sum(1 for fam, _ in UNSUPPORTED if fam == family)
    assert nat.device_faults() == 0
