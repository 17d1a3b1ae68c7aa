"""Map sensors of every slot of a fused launch (include/cagpu.h: cagpu_tape_poses, cagpu_laserscan_slots,
cagpu_laserscan_history): what BatchedSim.rollout(..., keep_steps=True, map_sensors=True) leaves in
`sim.kept_map_sensors`.

The launch keeps two small rings -- the POSE ring (every agent's pose after each step, restated from the launch's
trajectory tape) and the INDEX ring (the new laser range-index row of every slot, uint8) -- and the scan history the launch
found.  The large observations are expanded from them on request: a slot's history is one launch of the history kernel,
its occupancy windows one launch of the occupancy kernel over the slot's poses."""
import ctypes as C

import torch

from . import _native as nat

POSE_FIELDS = ("pos_x", "pos_y", "heading", "radius", "step_num")


def slot_bytes(E, N, num_beams, with_set):
    """bytes one slot of a launch adds: the pose ring (four float64 and an int32 per agent slot, an int32 per env with a map
    set) and the index ring (a byte per beam)"""
    return E * N * (4 * 8 + 4) + (4 * E if with_set else 0) + E * N * num_beams


class KeptMapSensors(object):
    """the per-slot map sensors of one rollout of n steps.  `poses`: dict of device tensors pos_x, pos_y, heading, radius
    (float64 [n, E, N]), step_num (int32 [n, E, N]) and, with a map set, env_map (int32 [n, E])."""

    def __init__(self, sim, n, poses, idx=None, carried=None, dense=None):
        self._sim, self.n, self.poses = sim, int(n), poses
        self._idx, self._carried = idx, carried
        self._dense = dense     # batches that advance by single launches: the sensors of every step, already expanded
        self._scan = None
        if idx is not None:
            self._scan = nat.CaScan.from_buffer_copy(sim._scan)   # the launch's geometry; hist = the history it found
            self._scan.hist, self._scan.out = carried.data_ptr(), None

    def _slot(self, t):
        t = int(t)
        if not 0 <= t < self.n:
            raise IndexError("slot %d of a launch of %d steps" % (t, self.n))
        return t

    def _history(self, t, want_hist, want_out):
        sim = self._sim
        first, count = (0, self.n) if t is None else (self._slot(t), 1)
        shape = (count,) + tuple(sim.scan_hist.shape)
        hist = torch.empty(shape, dtype=torch.uint8, device=sim.device) if want_hist else None
        out = torch.empty(shape, dtype=torch.float32, device=sim.device) if want_out else None
        nat.check(sim.lib.cagpu_laserscan_history(
            sim._p_ref, C.byref(self._scan), self._idx.data_ptr(), self.poses["step_num"].data_ptr(), self.n, first, count,
            None if hist is None else hist.data_ptr(), None if out is None else out.data_ptr(), sim._stream()))
        pick = (lambda x: x) if t is None else (lambda x: x[0])
        return (None if hist is None else pick(hist)), (None if out is None else pick(out))

    def laserscan(self, t=None):
        """the 'laserscan' observation of slot t, float32 metres [E, N, H, B]; None: of every slot, [n, E, N, H, B]"""
        if self._dense is not None:
            return self._dense["scan"] if t is None else self._dense["scan"][self._slot(t)]
        return self._history(t, False, True)[1]

    def laserscan_index(self, t=None):
        """the range-index history of slot t, uint8 [E, N, H, B] (255: nothing hit); None: of every slot"""
        if self._dense is not None:
            return self._dense["hist"] if t is None else self._dense["hist"][self._slot(t)]
        return self._history(t, True, False)[0]

    def occupancy_grid(self, t=None):
        """the 'occupancy_grid' observation of slot t in the format set_occupancy_grid() chose (bool [E, N, H, W], or the
        bit-packed int32 words where only those were asked for); None: of every slot, a leading [n]"""
        sim = self._sim
        if self._dense is not None:
            if self._dense["occ"] is None:
                raise nat.CagpuError("set_occupancy_grid() was not called before the rollout")
            return self._dense["occ"] if t is None else self._dense["occ"][self._slot(t)]
        if sim._occ is None:
            raise nat.CagpuError("set_occupancy_grid() first")
        first, count = (0, self.n) if t is None else (self._slot(t), 1)
        E, N = sim.E, sim.N
        og = nat.CaOccGrid.from_buffer_copy(sim._occ)
        h, w = int(og.height), int(og.width)
        cells = bits = None
        if sim.occ is not None:
            cells = torch.empty((count, E, N, h, w), dtype=torch.uint8, device=sim.device)
        else:
            bits = torch.empty((count, E, N, h, (w + 31) // 32), dtype=torch.int32, device=sim.device)
        og.cells, og.bits = (None if cells is None else cells.data_ptr()), (None if bits is None else bits.data_ptr())
        self._occ_launch(first, count, og)
        out = cells.view(torch.bool) if cells is not None else bits
        return out if t is None else out[0]

    def _occ_launch(self, first, count, og):
        """occ_kernel over slots first .. first + count - 1 as count x E envs: it is stateless and reads pos_x, pos_y and
        radius only"""
        sim, P = self._sim, self.poses
        E = sim.E
        p = nat.CaParams.from_buffer_copy(sim.p)
        p.num_envs = E * count
        at = lambda x: x.data_ptr() + first * x[0].numel() * x.element_size()
        cs = nat.CaState(pos_x=at(P["pos_x"]), pos_y=at(P["pos_y"]), radius=at(P["radius"]), heading=at(P["heading"]),
                         step_num=at(P["step_num"]))
        if sim._maps is not None:
            ms = nat.CaMapSet.from_buffer_copy(sim._maps)
            ms.env_map = at(P["env_map"])
            nat.check(sim.lib.cagpu_occupancy_grid_maps(C.byref(p), C.byref(cs), C.byref(ms), C.byref(og), sim._stream()))
        else:
            nat.check(sim.lib.cagpu_occupancy_grid(C.byref(p), C.byref(cs), C.byref(sim._map), C.byref(og), sim._stream()))

    def expand_into_sim(self, t):
        """slot t becomes the sim's own sensor state (`scan`, `scan_hist`, the occupancy tensors): the look-ahead ring's
        hand-out -- two launches, no synchronisation"""
        sim = self._sim
        nat.check(sim.lib.cagpu_laserscan_history(
            sim._p_ref, C.byref(self._scan), self._idx.data_ptr(), self.poses["step_num"].data_ptr(), self.n, t, 1,
            sim.scan_hist.data_ptr(), sim.scan.data_ptr(), sim._stream()))
        if sim._occ is not None:
            self._occ_launch(t, 1, sim._occ)
