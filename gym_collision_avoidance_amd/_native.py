"""ctypes binding of libcagpu.so (include/cagpu.h).  The product path: there is NO CPU fallback --
if the HIP library is missing or fails to load this module raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# CAGPU_LIB: load another build of the same ABI (a parent commit's library for a same-box comparison); the library itself
# reads no environment variable
LIB_PATH = os.environ.get("CAGPU_LIB") or os.path.join(HERE, "libcagpu.so")

# ---- constants mirrored from include/cagpu.h
CA_OK, CA_EINVAL, CA_EUNSUPPORTED, CA_ELAUNCH, CA_ENODEVICE = 0, -1, -2, -3, -4
AT_GOAL, WAS_AT_GOAL, IN_COLLISION, WAS_IN_COLLISION, OUT_OF_TIME, DONE, IS_LEARNING, STILL_LEARNING = (
    1 << 0, 1 << 1, 1 << 2, 1 << 3, 1 << 4, 1 << 5, 1 << 6, 1 << 7)
POLICY_SHIFT, DYNAMICS_SHIFT = 8, 12
ABSENT, PLAN_VALID = 1 << 16, 1 << 17
RVO_NONCOOP = 1 << 18   # CA_RVO_NONCOOP: written only by launches with a CaRvoDraw whose collab_coeff < 0
ABI_VERSION = 12  # CAGPU_VERSION of include/cagpu.h: the struct layouts below mirror THAT header
POL_RVO, POL_NONCOOP, POL_STATIC, POL_EXTERNAL, POL_LEARNING, POL_LEARNING_GA3C, POL_GA3C_CADRL = range(7)
DYN_UNICYCLE, DYN_MAX_TURN_RATE, DYN_EXTERNAL = range(3)
SORT_CLOSEST_FIRST, SORT_CLOSEST_LAST, SORT_TIME_TO_IMPACT = range(3)
OVER_ALL_DONE, OVER_AGENT0, OVER_LEARNING_DONE = range(3)

_P = C.c_void_p


class CaParams(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_envs", "num_agents", "max_obs", "sort_mode", "game_over_mode",
                                         "rvo_max_neighbors", "obs_clip", "ragged")] + \
               [(n, C.c_double) for n in ("dt", "near_goal_threshold", "max_time_ratio", "getting_close_range",
                                          "sensing_horizon", "reward_at_goal", "reward_collision", "reward_time_step",
                                          "reward_wiggly", "wiggly_threshold", "reward_min", "reward_max",
                                          "rvo_time_horizon", "rvo_collab_coeff", "max_heading_change",
                                          "reward_collision_wall", "rvo_dt")]


STATE_FIELDS = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed",
                "time_remaining", "t", "slt", "ep_reward", "last_action", "flags", "step_num", "episode_step",
                "reset_count", "env_stats", "next_action", "turning_dir", "rvo_collab", "rvo_heading_noise", "ext_state")
OUT_FIELDS = ("obs", "rewards", "done", "game_over", "actions", "orca_vel", "workspace")


class CaState(C.Structure):
    _fields_ = [(n, _P) for n in STATE_FIELDS]


class CaOut(C.Structure):
    _fields_ = [(n, _P) for n in OUT_FIELDS] + [("workspace_bytes", C.c_uint64)]


class CaAutoReset(C.Structure):
    _fields_ = [("table", _P), ("n_cases", C.c_int32), ("env_id_offset", C.c_int64), ("case_stride", C.c_int64),
                ("reset_obs", _P), ("reset_plan", _P), ("heading_seed", C.c_uint64)]


class CaMap(C.Structure):
    _fields_ = [("static_bits", _P), ("rows", C.c_int32), ("cols", C.c_int32), ("cell", C.c_double),
                ("origin_r", C.c_double), ("origin_c", C.c_double)]


class CaMapSet(C.Structure):
    _fields_ = [("map", CaMap), ("env_map", _P), ("num_maps", C.c_int32), ("reserved0", C.c_int32),
                ("map_seed", C.c_uint64)]


class CaScan(C.Structure):
    _fields_ = [("hist", _P), ("out", _P), ("num_beams", C.c_int32), ("num_to_store", C.c_int32),
                ("num_ranges", C.c_int32), ("reserved0", C.c_int32), ("min_angle", C.c_double),
                ("max_angle", C.c_double), ("range_res", C.c_double), ("max_range", C.c_double)]


class CaOccGrid(C.Structure):
    _fields_ = [("cells", _P), ("bits", _P), ("height", C.c_int32), ("width", C.c_int32), ("x_width", C.c_double),
                ("y_width", C.c_double)]


class CaTraj(C.Structure):
    _fields_ = [("rows", _P), ("episode", _P)]


class CaFinal(C.Structure):
    _fields_ = [("obs", _P), ("flags", _P)]


class CaEpLog(C.Structure):
    _fields_ = [("rows", _P), ("head", _P), ("capacity", C.c_int32), ("reserved0", C.c_int32)]


class CaEpMetrics(C.Structure):
    """the episode metrics' records, ring and carry (cagpu_episode_metrics); include/cagpu.h states the rules"""
    _fields_ = [("vals", _P), ("cnts", _P), ("head", _P), ("capacity", C.c_int32), ("reserved0", C.c_int32), ("carry", _P),
                ("getting_close_range", C.c_double)]


class CaStepEx(C.Structure):
    """one step / rollout launch (cagpu_step_ex).  The five record pointers are plain addresses (C.addressof of a CaMap /
    CaMapSet / CaTraj / CaFinal / CaEpLog, None = not used): whoever stores one keeps that struct alive"""
    _fields_ = [("n_steps", C.c_int32), ("ring", C.c_int32), ("snapshot_delta", C.c_int64), ("map", _P), ("set", _P),
                ("traj", _P), ("fin", _P), ("log", _P)]


class CaPolicyDraw(C.Structure):
    """the policy lottery of an auto-reset (cagpu_step_draw / cagpu_policy_draw); include/cagpu.h states the rule"""
    _fields_ = [("cdf", _P), ("policy_bits", _P), ("num_policies", C.c_int32), ("ensure", C.c_int32), ("seed", C.c_uint64)]


class CaActionTape(C.Structure):
    """an action tape (cagpu_step_tape): slot t of `actions` is step t's [E, N, 2]; include/cagpu.h states the rules"""
    _fields_ = [("actions", _P), ("step_stride", C.c_int64)]


class CaRvoDraw(C.Structure):
    """RVOPolicy's stochastic branches drawn in the step kernels (cagpu_step_noise); include/cagpu.h states the rule"""
    _fields_ = [("seed", C.c_uint64), ("collab_coeff", C.c_double), ("anti_collab_t", C.c_double), ("noise_std", C.c_double),
                ("noise_mask", _P), ("address", _P)]


FAULT_RVO_DRAW_STEP = 16   # bit 4 of the fault word: an agent was queried under a CaRvoDraw at an episode step >= 2^22


class CaGa3cSample(C.Structure):
    """the sampled GA3C-CADRL policy and the pre-step half of an experience tape slot (cagpu_ga3c_sample); include/cagpu.h
    states the rule"""
    _fields_ = [("seed", C.c_uint64), ("temperature", C.c_float), ("greedy", C.c_int32), ("mask", _P), ("agent_net", _P),
                ("net_index", C.c_int32), ("reserved0", C.c_int32), ("address", _P), ("logits", _P), ("logp", _P),
                ("entropy", _P), ("action", _P), ("obs", _P), ("value", _P), ("slot_obs", _P), ("slot_value", _P),
                ("slot_live", _P), ("slot_address", _P)]


FAULT_GA3C_SAMPLE_NAN = 32   # bit 5 of the fault word: a logits row with a NaN reached the sampler


class CaPoseRing(C.Structure):
    """the pose ring of a fused launch (cagpu_tape_poses): slot t = the poses after step t; include/cagpu.h states the rule"""
    _fields_ = [(n, _P) for n in ("pos_x", "pos_y", "heading", "radius", "step_num", "env_map")]


class CaCaseStream(C.Structure):
    """a case stream (cagpu_stream_refill): the window table of a CaAutoReset and what keeps it ahead of the envs;
    include/cagpu.h states the rule.  side_ranges is a HOST pointer: whoever stores it keeps that array alive"""
    _fields_ = [("table", _P), ("held", _P), ("seen", _P), ("work_index", _P), ("work_row", _P), ("work_count", _P),
                ("counts", _P), ("status", _P), ("window", C.c_int32), ("n_min", C.c_int32), ("n_max", C.c_int32),
                ("n_ranges", C.c_int32), ("side_ranges", _P), ("speed_lo", C.c_double), ("speed_hi", C.c_double),
                ("radius_lo", C.c_double), ("radius_hi", C.c_double), ("seed", C.c_uint64)]


FAULT_STREAM_OVERRUN = 8   # bit 3 of the fault word: an env of a case stream ran past its window between two refills

POLICY_DRAW_BITS = 0xFC0   # the bits of a flag word a draw rewrites: IS_LEARNING, STILL_LEARNING, the policy id


class CaRender(C.Structure):
    _fields_ = [("out", _P), ("num_frames", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("flags", C.c_int32),
                ("xmin", C.c_double), ("ymax", C.c_double), ("s16", C.c_double), ("frame_env", _P), ("frame_col", _P),
                ("first", _P), ("last", _P), ("hist", _P), ("hist_steps", C.c_int32), ("hist_cols", C.c_int32),
                ("stride_t", C.c_int64), ("stride_s", C.c_int64), ("work", _P), ("work_bytes", C.c_uint64)]


RENDER_CIRCLES, RENDER_MAP = 1, 2   # CaRender.flags

NET_FIELDS = ("lstm_kernel", "lstm_bias", "layer1_kernel", "layer1_bias", "layer2_kernel", "layer2_bias", "fc1_kernel",
              "fc1_bias", "logits_kernel", "logits_bias", "input_mean", "input_std")


class CaNet(C.Structure):
    _fields_ = [(n, _P) for n in NET_FIELDS] + [("rows_scratch", _P), ("agent_net", _P), ("net_index", C.c_int32),
                                                ("reserved0", C.c_int32), ("packed", _P)]


class CaNetQuery(C.Structure):
    _fields_ = [("x", _P), ("rows", C.c_int64), ("width", C.c_int32), ("reserved0", C.c_int32), ("value_kernel", _P),
                ("value_bias", _P), ("logits", _P), ("value", _P), ("action", _P)]


class CaNetValue(C.Structure):
    _fields_ = [("value_kernel", _P), ("value_bias", _P), ("value", _P)]


class CaNetGrad(C.Structure):
    """one call of the network's backward pass (cagpu_ga3c_grad); include/cagpu.h states the rule and grad's layout"""
    _fields_ = [("x", _P), ("rows", C.c_int64), ("width", C.c_int32), ("accumulate", C.c_int32), ("live", _P),
                ("dlogits", _P), ("dvalue", _P), ("value_kernel", _P), ("value_bias", _P), ("grad", _P), ("work", _P),
                ("work_bytes", C.c_uint64)]


EXPORTS = ("cagpu_version", "cagpu_last_error", "cagpu_last_kernel", "cagpu_reset", "cagpu_step", "cagpu_step_map", "cagpu_rollout",
           "cagpu_orca", "cagpu_observe", "cagpu_laserscan", "cagpu_ga3c", "cagpu_generate_cases", "cagpu_generate_cases_ragged", "cagpu_plan", "cagpu_debug_libm", "cagpu_device_faults", "cagpu_workspace_bytes",
           "cagpu_ga3c_packed_bytes", "cagpu_ga3c_pack", "cagpu_rollout_ring", "cagpu_ring_snapshots", "cagpu_debug_copy8", "cagpu_device_faults_async",
           "cagpu_step_maps", "cagpu_laserscan_maps", "cagpu_occupancy_grid", "cagpu_occupancy_grid_maps",
           "cagpu_step_traj", "cagpu_rollout_traj", "cagpu_step_final", "cagpu_rollout_final",
           "cagpu_step_log", "cagpu_rollout_log", "cagpu_step_ex", "cagpu_step_draw", "cagpu_policy_draw",
           "cagpu_render", "cagpu_render_maps", "cagpu_render_work_bytes", "cagpu_ga3c_query", "cagpu_ga3c_value",
           "cagpu_generate_cases_at", "cagpu_stream_refill", "cagpu_episode_metrics_carry_bytes", "cagpu_episode_metrics",
           "cagpu_step_ex_maps", "cagpu_map_draw", "cagpu_heading_draw", "cagpu_policy_draw_at", "cagpu_step_tape",
           "cagpu_tape_poses", "cagpu_laserscan_slots", "cagpu_laserscan_history", "cagpu_step_noise", "cagpu_rvo_draw_at",
           "cagpu_ga3c_sample", "cagpu_ga3c_sample_at", "cagpu_gae",
           "cagpu_ga3c_grad_floats", "cagpu_ga3c_grad_work_bytes", "cagpu_ga3c_grad")

_lib = None


class CagpuError(RuntimeError):
    pass


def lib():
    """Load libcagpu.so; raise loudly if it is not there (no eager / CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CagpuError("libcagpu.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "(hipcc --offload-arch=gfx950); there is no CPU fallback for the hot path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    L.cagpu_version.restype = C.c_int
    L.cagpu_last_error.restype = C.c_char_p
    got = L.cagpu_version()
    if got != ABI_VERSION:  # a stale or experiment build would silently mis-read the structs above
        raise CagpuError("%s reports ABI version %d, this binding mirrors version %d of include/cagpu.h -- rebuild "
                         "(python -m gym_collision_avoidance_amd.build_native)" % (LIB_PATH, got, ABI_VERSION))
    PP, PS, PO, PA = C.POINTER(CaParams), C.POINTER(CaState), C.POINTER(CaOut), C.POINTER(CaAutoReset)
    L.cagpu_reset.argtypes = [PP, PS, PO, _P, _P, _P, _P]
    L.cagpu_step.argtypes = [PP, PS, PO, _P, PA, _P]
    L.cagpu_rollout.argtypes = [PP, PS, PO, _P, PA, C.c_int32, _P]
    L.cagpu_rollout_ring.argtypes = [PP, PS, PO, _P, PA, C.c_int32, C.c_int64, _P]
    L.cagpu_ring_snapshots.argtypes = [PP, PS, PO, PA, C.c_int32]
    L.cagpu_debug_copy8.argtypes = [C.c_int64, _P, _P, _P]
    L.cagpu_step_map.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaMap), _P]
    L.cagpu_laserscan.argtypes = [PP, PS, C.POINTER(CaMap), C.POINTER(CaScan), _P]
    L.cagpu_step_maps.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaMapSet), _P]
    L.cagpu_laserscan_maps.argtypes = [PP, PS, C.POINTER(CaMapSet), C.POINTER(CaScan), _P]
    L.cagpu_occupancy_grid.argtypes = [PP, PS, C.POINTER(CaMap), C.POINTER(CaOccGrid), _P]
    L.cagpu_occupancy_grid_maps.argtypes = [PP, PS, C.POINTER(CaMapSet), C.POINTER(CaOccGrid), _P]
    L.cagpu_step_traj.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaMap), C.POINTER(CaMapSet), C.POINTER(CaTraj), _P]
    L.cagpu_rollout_traj.argtypes = [PP, PS, PO, _P, PA, C.c_int32, C.c_int32, C.c_int64, C.POINTER(CaTraj), _P]
    L.cagpu_step_final.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaMap), C.POINTER(CaMapSet), C.POINTER(CaTraj),
                                   C.POINTER(CaFinal), _P]
    L.cagpu_rollout_final.argtypes = [PP, PS, PO, _P, PA, C.c_int32, C.c_int32, C.c_int64, C.POINTER(CaTraj),
                                      C.POINTER(CaFinal), _P]
    L.cagpu_step_log.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaMap), C.POINTER(CaMapSet), C.POINTER(CaTraj),
                                 C.POINTER(CaFinal), C.POINTER(CaEpLog), _P]
    L.cagpu_rollout_log.argtypes = [PP, PS, PO, _P, PA, C.c_int32, C.c_int32, C.c_int64, C.POINTER(CaTraj),
                                    C.POINTER(CaFinal), C.POINTER(CaEpLog), _P]
    L.cagpu_step_ex.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaStepEx), _P]
    L.cagpu_step_draw.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaStepEx), C.POINTER(CaPolicyDraw), _P]
    L.cagpu_policy_draw.argtypes = [PP, PS, PO, PA, C.POINTER(CaPolicyDraw), _P, _P]
    L.cagpu_step_ex_maps.argtypes = [PP, PS, PO, _P, PA, C.POINTER(CaStepEx), C.POINTER(CaPolicyDraw), _P]
    L.cagpu_step_tape.argtypes = [PP, PS, PO, C.POINTER(CaActionTape), PA, C.POINTER(CaStepEx), C.POINTER(CaPolicyDraw), _P]
    L.cagpu_step_noise.argtypes = [PP, PS, PO, C.POINTER(CaActionTape), PA, C.POINTER(CaStepEx), C.POINTER(CaPolicyDraw),
                                   C.POINTER(CaRvoDraw), _P]
    L.cagpu_rvo_draw_at.argtypes = [C.POINTER(CaRvoDraw), C.c_int32, _P, _P, _P, _P, C.c_int64, _P, _P, _P]
    L.cagpu_ga3c_sample.argtypes = [PP, PS, PA, C.POINTER(CaPolicyDraw), C.POINTER(CaMapSet), C.POINTER(CaRvoDraw),
                                    C.POINTER(CaGa3cSample), _P, _P]
    L.cagpu_ga3c_sample_at.argtypes = [C.c_uint64, C.c_float, C.c_int32, _P, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P]
    L.cagpu_gae.argtypes = [C.c_int32, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P, C.c_float, C.c_float, _P, _P, _P]
    L.cagpu_map_draw.argtypes = [C.c_uint64, C.c_int32, _P, _P, C.c_int64, _P, _P]
    L.cagpu_heading_draw.argtypes = [C.c_uint64, C.c_int32, _P, _P, C.c_int64, _P, _P]
    L.cagpu_policy_draw_at.argtypes = [C.POINTER(CaPolicyDraw), C.c_int32, _P, _P, _P, C.c_int64, _P, _P]
    L.cagpu_render.argtypes = [PP, PS, C.POINTER(CaMap), C.POINTER(CaRender), _P]
    L.cagpu_render_maps.argtypes = [PP, PS, C.POINTER(CaMapSet), C.POINTER(CaRender), _P]
    L.cagpu_render_work_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.cagpu_render_work_bytes.restype = C.c_uint64
    L.cagpu_observe.argtypes = [PP, PS, PO, _P]
    L.cagpu_plan.argtypes = [PP, PS, _P]
    L.cagpu_orca.argtypes = [C.c_int32, C.c_int32, _P, _P, _P, _P, _P, C.c_float, C.c_float, C.c_float, C.c_int32,
                             C.c_float, _P, _P]
    L.cagpu_ga3c.argtypes = [PP, PS, _P, C.POINTER(CaNet), _P, _P, _P]
    L.cagpu_ga3c_query.argtypes = [C.POINTER(CaNet), C.POINTER(CaNetQuery), _P]
    L.cagpu_ga3c_value.argtypes = [PP, PS, _P, C.POINTER(CaNet), _P, _P, C.POINTER(CaNetValue), _P]
    L.cagpu_generate_cases.argtypes = [C.c_int64, C.c_int32] + [C.c_double] * 6 + [C.c_uint64, _P, _P, _P]
    L.cagpu_generate_cases_ragged.argtypes = ([C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32] + [C.c_double] * 4 +
                                              [C.c_uint64, _P, _P, _P, _P])
    L.cagpu_generate_cases_at.argtypes = ([_P, _P, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int32] +
                                          [C.c_double] * 4 + [C.c_uint64, _P, _P, _P, _P])
    L.cagpu_stream_refill.argtypes = [PP, PS, PA, C.POINTER(CaCaseStream), _P]
    L.cagpu_episode_metrics_carry_bytes.argtypes = [PP]
    L.cagpu_episode_metrics_carry_bytes.restype = C.c_uint64
    L.cagpu_episode_metrics.argtypes = [PP, C.POINTER(CaTraj), C.c_int32, C.POINTER(CaEpMetrics), _P]
    L.cagpu_tape_poses.argtypes = [PP, PS, _P, C.POINTER(CaTraj), _P, C.c_int32, PA, C.POINTER(CaMapSet), C.POINTER(CaPoseRing), _P]
    L.cagpu_laserscan_slots.argtypes = [PP, C.POINTER(CaPoseRing), C.c_int32, C.POINTER(CaMap), C.POINTER(CaMapSet),
                                        C.POINTER(CaScan), _P, _P]
    L.cagpu_laserscan_history.argtypes = [PP, C.POINTER(CaScan), _P, _P, C.c_int32, C.c_int32, C.c_int32, _P, _P, _P]
    L.cagpu_device_faults.argtypes = [_P, C.c_int32]
    L.cagpu_device_faults_async.argtypes = [_P, _P]
    L.cagpu_workspace_bytes.argtypes = [PP]
    L.cagpu_workspace_bytes.restype = C.c_uint64
    L.cagpu_ga3c_packed_bytes.argtypes = []
    L.cagpu_ga3c_packed_bytes.restype = C.c_uint64
    L.cagpu_ga3c_pack.argtypes = [C.POINTER(CaNet), _P, C.c_uint64, _P]
    L.cagpu_debug_libm.argtypes = [C.c_int32, C.c_int32, _P, _P, _P, _P]
    L.cagpu_ga3c_grad_floats.argtypes = []
    L.cagpu_ga3c_grad_floats.restype = C.c_uint64
    L.cagpu_ga3c_grad_work_bytes.argtypes = [C.c_int64]
    L.cagpu_ga3c_grad_work_bytes.restype = C.c_uint64
    L.cagpu_ga3c_grad.argtypes = [C.POINTER(CaNet), C.POINTER(CaNetGrad), _P]
    for n in EXPORTS:
        getattr(L, n)  # AttributeError if a declared symbol is missing
        if n not in ("cagpu_last_error", "cagpu_last_kernel", "cagpu_workspace_bytes", "cagpu_ga3c_packed_bytes",
                     "cagpu_render_work_bytes", "cagpu_episode_metrics_carry_bytes", "cagpu_ga3c_grad_floats",
                     "cagpu_ga3c_grad_work_bytes"):
            getattr(L, n).restype = C.c_int
    L.cagpu_last_error.restype = C.c_char_p
    L.cagpu_last_kernel.restype = C.c_char_p
    _lib = L
    return L


def device_faults(clear=True):
    """cagpu_device_faults: the current device's fault word (0 in normal operation); synchronises the device."""
    v = C.c_uint32(0)
    check(lib().cagpu_device_faults(C.byref(v), 1 if clear else 0))
    return int(v.value)


def debug_libm(op, a, b=None):
    """cagpu_debug_libm on numpy float64 arrays -> (out0, out1): the device's own atan2 / heading sincos / lean divide and
    square root (parity hook, see include/cagpu.h)."""
    import numpy as np
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    b = None if b is None else np.ascontiguousarray(b, np.float64).reshape(-1)
    o0, o1 = np.empty_like(a), np.empty_like(a)
    check(lib().cagpu_debug_libm(op, a.size, a.ctypes.data, None if b is None else b.ctypes.data, o0.ctypes.data, o1.ctypes.data))
    return o0, o1


# the bits of a flag word the step kernels decide (everything but the policy / dynamics ids, the learning bits set by
# set_plugins and PLAN_VALID, which belongs to the pipelined policy query)
KERNEL_FLAG_BITS = AT_GOAL | WAS_AT_GOAL | IN_COLLISION | WAS_IN_COLLISION | OUT_OF_TIME | DONE | ABSENT


def decode_flags(flags):
    """Agent flag words (include/cagpu.h: CaState.flags, CaFinal.flags) -> {name: bool array of the same shape}:
    `at_goal`, `in_collision`, `ran_out_of_time` -- the reference's Agent.is_at_goal / in_collision / ran_out_of_time
    (agent.py:108-112) --, `done` and `absent` (an empty slot of a ragged batch: it carries at_goal and done as well, mask
    with ~absent where only agents count).  Pure host-side bit tests: numpy arrays, torch tensors (any device, int32 as
    the simulator keeps them) and plain ints all work."""
    if not hasattr(flags, "__and__") or isinstance(flags, (list, tuple)):
        import numpy as np
        flags = np.asarray(flags)
    if hasattr(flags, "dtype") and not hasattr(flags, "device"):   # numpy: uint32 words and int32 bit patterns alike
        import numpy as np
        flags = np.asarray(flags).astype(np.int64)
    bit = lambda m: (flags & m) != 0
    return {"at_goal": bit(AT_GOAL), "in_collision": bit(IN_COLLISION), "ran_out_of_time": bit(OUT_OF_TIME),
            "done": bit(DONE), "absent": bit(ABSENT)}


def check(rc):
    if rc != 0:
        raise CagpuError("cagpu error %d: %s" % (rc, lib().cagpu_last_error().decode()))
