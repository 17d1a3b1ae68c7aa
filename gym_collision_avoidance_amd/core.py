"""BatchedSim: the (num_envs x num_agents) simulator state as PyTorch-ROCm tensors + the calls into libcagpu.so.

torch is plumbing here (device memory, streams); every per-step computation happens in the HIP kernels of
csrc/cagpu.hip through the C ABI of include/cagpu.h.  Layout: agent-major SoA, index e*N + a.
Reference objects this replaces: the list[Agent] owned by CollisionAvoidanceEnv (collision_avoidance_env.py:141,
agent.py:29-138) and the per-step loops of collision_avoidance_env.py:156-234.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import torch

from . import _native as nat
from . import episode_metrics
from . import episodes

_F64 = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed",
        "time_remaining", "t", "slt", "ep_reward", "turning_dir")
STAT_NAMES = ("episodes", "collision_episodes", "all_at_goal_episodes", "stuck_episodes", "sum_steps",
              "sum_total_reward", "sum_time_to_goal", "sum_extra_time_to_goal")


def make_params(num_envs, num_agents, max_obs=None, dt=0.1, max_time_ratio=8.0, sort_mode=nat.SORT_CLOSEST_FIRST,
                game_over_mode=nat.OVER_ALL_DONE, rvo_max_neighbors=None, near_goal_threshold=0.2,
                getting_close_range=0.2, sensing_horizon=math.inf, reward_at_goal=1.0, reward_collision=-0.25,
                reward_time_step=0.0, reward_wiggly=0.0, wiggly_threshold=math.inf, reward_min=None, reward_max=None,
                rvo_time_horizon=5.0, rvo_collab_coeff=0.5, max_heading_change=math.pi / 3, obs_clip=None,
                reward_collision_wall=-0.25, rvo_dt=None, ragged=0):
    """CaParams with the reference's Config defaults (config.py:28-86) for an EvaluateConfig-style run."""
    p = nat.CaParams()
    p.num_envs, p.num_agents = int(num_envs), int(num_agents)
    p.max_obs = int(num_agents - 1 if max_obs is None else max_obs)
    p.obs_clip = p.max_obs if obs_clip is None else int(obs_clip)
    p.ragged = int(ragged)   # envs may hold fewer than num_agents agents (case rows with radius <= 0 = empty slots)
    p.sort_mode, p.game_over_mode = int(sort_mode), int(game_over_mode)
    p.rvo_max_neighbors = int(num_agents if rvo_max_neighbors is None else rvo_max_neighbors)
    p.dt, p.near_goal_threshold, p.max_time_ratio = dt, near_goal_threshold, max_time_ratio
    p.getting_close_range, p.sensing_horizon = getting_close_range, sensing_horizon
    p.reward_at_goal, p.reward_collision, p.reward_time_step = reward_at_goal, reward_collision, reward_time_step
    p.reward_wiggly, p.wiggly_threshold = reward_wiggly, wiggly_threshold
    # collision_avoidance_env.py:589-599: clip bounds = min/max of the possible reward values
    vals = [reward_at_goal, reward_collision, reward_time_step, reward_collision_wall, reward_wiggly]
    p.reward_min = min(vals) if reward_min is None else reward_min
    p.reward_max = max(vals) if reward_max is None else reward_max
    p.rvo_time_horizon, p.rvo_collab_coeff = rvo_time_horizon, rvo_collab_coeff
    p.max_heading_change = max_heading_change
    p.reward_collision_wall = reward_collision_wall
    p.rvo_dt = dt if rvo_dt is None else rvo_dt   # RVOPolicy.py:13: Config.DT, whatever dt a later step() is called with
    return p


GA3C_DEFAULT_WEIGHTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "ga3c_cadrl", "IROS18",
                                    "network_01900000.npz")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)   # (see BatchedSim._stream_handle)


def policy_word_bits(policy, is_learning=None, still_learning=None):
    """bits 6..11 of a flag word for a policy id (CA_POL_*): one entry of a policy draw's pool (set_policy_draw).  The
    learning bits default to what set_plugins gives the policy."""
    learn = policy in (nat.POL_LEARNING, nat.POL_LEARNING_GA3C)
    isl = learn if is_learning is None else bool(is_learning)
    stl = learn if still_learning is None else bool(still_learning)
    return (int(policy) << nat.POLICY_SHIFT) | (nat.IS_LEARNING if isl else 0) | (nat.STILL_LEARNING if stl else 0)


class BatchedSim(object):
    PROBE_EVERY = 8   # the device's fault word is probed behind every 8th ring refill (and every 256th single launch)

    def __init__(self, params, device="cuda:0", record_actions=False, pipeline=True):
        """pipeline: hand the kernels CaState.next_action (include/cagpu.h): the step kernel then computes the RVO policy of
        the NEXT step beside the sensing half of this one and the next launch starts at the move -- bit-identical results.
        Code that writes `state[...]` tensors directly must call invalidate_plan() afterwards (or overwrite `flags`
        with words whose PLAN_VALID bit is clear); reset() does it by itself."""
        if not torch.cuda.is_available():
            raise nat.CagpuError("BatchedSim needs a ROCm device: the hot path is HIP-only (no CPU fallback)")
        self.lib = nat.lib()
        self.p = params
        self.device = torch.device(device)
        self._dev_index = self.device.index if self.device.index is not None else 0
        E, N, K = params.num_envs, params.num_agents, params.max_obs
        self.E, self.N, self.K, self.W = E, N, K, 6 + 7 * K
        dev = self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        # The whole simulator state lives in ONE slab (every array a 256-byte-aligned view of it): the look-ahead ring
        # (step_lookahead) snapshots it with one device copy before it runs ahead and restores it the same way when the
        # caller turns out to need the state of a step already handed out.
        specs = [(n, (E, N), torch.float64) for n in _F64] + [
            ("last_action", (E, N, 2), torch.float32), ("flags", (E, N), torch.int32),   # (flags: uint32 bit pattern)
            ("step_num", (E, N), torch.int32), ("episode_step", (E,), torch.int32), ("reset_count", (E,), torch.int32),
            ("env_stats", (E, 8), torch.float64), ("next_action", (E, N, 4), torch.float32)]
        offs, total = [], 0
        for _, shape, dt in specs:
            offs.append(total)
            total += (int(np.prod(shape)) * torch.empty((), dtype=dt).element_size() + 255) // 256 * 256
        self._slab = torch.zeros((total,), dtype=torch.uint8, device=dev)
        self._state = {}
        for (n, shape, dt), off in zip(specs, offs):
            nb = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
            self._state[n] = self._slab[off:off + nb].view(dt).view(shape)
        self._la = None           # the look-ahead ring (enable_lookahead)
        self.pipeline = bool(pipeline)
        self._obs = z((E, N, self.W), torch.float32)
        self._rewards = z((E, N), torch.float32)
        self._done = z((E, N), torch.uint8)
        self._game_over = z((E,), torch.uint8)
        self.actions = z((E, N, 2), torch.float32) if record_actions else None
        self.orca_vel = z((E, N, 2), torch.float32) if record_actions else None
        self._cs = nat.CaState(**{n: self._state[n].data_ptr() for n in nat.STATE_FIELDS if n in self._state})
        self._rvo = None          # RVOPolicy's stochastic branches (set_rvo_stochastic)
        self._rd = None           # ... drawn inside the step kernels instead (set_rvo_draw: CaRvoDraw)
        self._variants = []       # per-agent sensor arguments beyond the primary pair (set_sensor_variants)
        if not self.pipeline:
            self._cs.next_action = None
        self._co = nat.CaOut(obs=self._obs.data_ptr(), rewards=self._rewards.data_ptr(), done=self._done.data_ptr(),
                             game_over=self._game_over.data_ptr(),
                             actions=self.actions.data_ptr() if record_actions else None,
                             orca_vel=self.orca_vel.data_ptr() if record_actions else None)
        # more than 64 agents per env: the large-env kernel's per-pair columns live in a workspace (include/cagpu.h)
        self._workspace = None
        wsb = int(self.lib.cagpu_workspace_bytes(C.byref(self.p)))
        if wsb:
            self._workspace = torch.empty((wsb,), dtype=torch.uint8, device=dev)
            self._co.workspace, self._co.workspace_bytes = self._workspace.data_ptr(), wsb
        # fresh_outputs: every step / rollout writes obs, rewards, done and game_over into NEWLY allocated tensors (the
        # previous ones stay valid and belong to whoever holds them: the env API's "fresh arrays every step" without a
        # copy kernel).  Every element of the four outputs is rewritten by every step launch
        # (tests/test_gpu_parity.py::test_step_rewrites_every_output_element), so nothing is carried over in them.
        self.fresh_outputs = False
        self._ar = None
        # Every step / rollout launch is ONE call, cagpu_step_ex, and what varies between launches is data: self._sx is the
        # CaStepEx of a single step, whose map / set / traj / fin / log addresses are set where the feature is switched
        # (set_map, _traj_switch, keep_final, log_episodes) and point at structs this object holds and rewrites IN PLACE.
        # The references below are made once: p, _cs, _co and _sx are never replaced; _ar is, by set_fixture_table only,
        # which re-makes _ar_ref.
        self._step_ex = self.lib.cagpu_step_ex
        # ... except while a policy draw is on (set_policy_draw): _launch is then cagpu_step_draw with the draw bound in
        self._launch = self._step_ex
        # ... and a fused launch (rollout, ring fill, a rewind's replay) of a batch with a map: cagpu_step_ex_maps, the one
        # entry point that admits CaStepEx.map / .set with n_steps > 1 or ring (_launch_n)
        self._step_ex_maps = self.lib.cagpu_step_ex_maps
        self._draw = None         # the policy draw: dict(c=CaPolicyDraw, cdf, bits, has_ga3c) / None
        self._sx = nat.CaStepEx(n_steps=1)
        self._p_ref, self._cs_ref, self._co_ref, self._sx_ref = C.byref(self.p), C.byref(self._cs), C.byref(self._co), C.byref(self._sx)
        self._ar_ref = None
        # the current stream's raw handle (no torch.cuda.Stream object is built around it: 1.2 -> 0.3 us on the way to a launch)
        self._stream_handle = (functools.partial(_raw_stream, self._dev_index) if _raw_stream else
                               lambda: torch.cuda.current_stream(self.device).cuda_stream)
        self._table = None
        self._keep = []
        self._map = None
        self._maps = None         # a map set (set_map with a stack of maps): CaMapSet; env_map is its device index tensor
        self._map_rng = None      # the generator of the map-set key an explicit reset() draws (set_map's map_seed)
        self._env_map = None
        self._scan = None
        self.scan = None
        self.occ = None           # OccupancyGridSensor windows (set_occupancy_grid): bool [E, N, H, W] / None
        self.occ_bits = None      # ... bit-packed: int32 [E, N, H, (W + 31) // 32] / None
        self._occ = None
        self.ga3c_fused = False   # cagpu_ga3c with obs = NULL: sensing fused into the network kernel (see ga3c())
        self._net = None          # GA3C-CADRL weights (load_ga3c); _nets: {checkpoint index: (CaNet, tensors)}
        self._net_tensors = None
        self._nets = {}
        self._agent_net = None    # int32 [E, N]: which checkpoint an agent runs (set_ga3c_assignment)
        self._has_ga3c = False    # some agent's policy is CA_POL_GA3C_CADRL (set_plugins), or may become it (set_policy_draw)
        self._plugins_ga3c = False
        self._ga3c_ext = None
        self._ga3c_ext2 = None    # the scratch action buffer of collect()'s last_value launch
        self.ga3c_logits = None
        self.ga3c_value = None    # float32 [E, N] (load_ga3c(keep_value=True)): logits_v of the agents ga3c() evaluated
        # the sampled GA3C-CADRL policy (set_ga3c_sampling: CaGa3cSample) and the experience tape (collect)
        self._samp = None         # dict(seed, temperature, mask, addr) / None = greedy
        self._cg = nat.CaGa3cSample(temperature=1.0, greedy=1)
        self._xp = None           # the tape slot the next ga3c() call fills: dict of addresses (collect) / None
        self._samp_logits = None  # the sampler's own logits when load_ga3c did not keep them
        self.ga3c_logp = None     # float32 [E, N]: log-probability of the index played in the last step (evaluated agents)
        self.ga3c_entropy = None  # float32 [E, N]: entropy of the last step's softmax
        self.ga3c_action = None   # int8 [E, N]: the index played
        self.experience_max_bytes = 1 << 30   # the byte budget of ONE experience tape (collect)
        self._fault = None        # the non-blocking fault-word probe of the product path (_fault_probe)
        # (the first probe -- it creates the side stream and the pinned word: milliseconds -- on the second launch of a
        # simulator's life, not 256 launches in, in the middle of somebody's timed loop)
        self._steps_since_probe = 254
        # the trajectory tape (record_trajectories): None = never switched on
        self._traj, self._traj_on = None, False
        self._ct = nat.CaTraj()   # the slot a single-step launch records into (rewritten before every such launch)
        # the final record (keep_final): the terminal observation / flag words of the envs an auto-reset overwrites
        self._fin_on, self._fin_obs, self._fin_flags = False, None, None
        self._cf = nat.CaFinal()
        # the episode log (log_episodes): None = off; dict(rows [E, C, N, 4] f64, head [E, C, 4] i32, cursor [E] i64, cap)
        self._log = None
        self._cl = nat.CaEpLog()
        # the episode metrics (measure_episodes): None = off; dict(vals, cnts [E, C, N, 4], head [E, C], cursor [E] i64,
        # carry [E, bytes] u8, cap, keep_tape, cm=CaEpMetrics, ct=CaTraj of the slots being fed, own_tape)
        self._met = None
        # the case stream (set_case_stream): None = off; dict(c=CaCaseStream, ref, its tensors, every, since, dist)
        self._cstream = None
        # what a replay needs that the running state does not hold (episode_start): the case rows and headings reset()
        # loaded, float64 [E, N, 7] (NaN heading: pointed at the goal; NaN rows: never reset; None before the first
        # reset), the flag words set_plugins gave every slot (host int32 [E, N]; None: never called) and set_map's arguments
        self._start = None
        self._plugin_words = None
        self._map_src = None
        # rollout(keep_steps=True) with keep_final() on: every slot's final block (final_obs [n, E, N, W], final_flags [n, E, N])
        self.kept_final = None
        # rollout(keep_steps=True, map_sensors=True): every slot's laser scan and occupancy windows (map_slots.KeptMapSensors)
        self.kept_map_sensors = None

    # ---------------------------------------------------------------- what the outside reads
    # `state` and the four outputs are those of the step last handed out: reading them goes through sync(), which rewinds a
    # look-ahead ring that has run ahead (a no-op without one); the methods of this class use the underscored names.
    @property
    def state(self):
        self.sync()
        return self._state

    def _synced(name):   # noqa: N805 -- builds the four output properties
        def get(self):
            self.sync()
            return getattr(self, name)

        def put(self, value):
            setattr(self, name, value)
        return property(get, put)
    obs, rewards, done, game_over = _synced("_obs"), _synced("_rewards"), _synced("_done"), _synced("_game_over")
    # the map of every env of a map set (device int32 [E]; None without a set), at the step last handed out: an auto-reset
    # of a look-ahead ring that has run ahead has already drawn the maps of episodes not handed out yet
    env_map = _synced("_env_map")
    # the final record of the step last handed out (keep_final; None while it is off): float32 [E, N, W] / int32 [E, N]
    # (uint32 bit patterns, nat.decode_flags), rows valid where `game_over` is set
    final_obs, final_flags = _synced("_fin_obs"), _synced("_fin_flags")
    del _synced

    # ---------------------------------------------------------------- plumbing
    def _stream(self):
        return C.c_void_p(self._stream_handle())

    def _dev(self, x, dtype):
        if x is None:
            return None
        t = torch.as_tensor(x, dtype=dtype)
        if t.device != self.device:
            t = t.to(self.device)
        return t.contiguous()

    def update_params(self, **changes):
        """Change CaParams fields (e.g. rvo_collab_coeff=0.3) on a live sim.  A pipelined plan -- CaState.next_action of
        every env and the fixture table's reset_plan / reset_obs -- was computed under the parameters in force when it
        was made (RVO horizon / collaboration / dt, sensing horizon, neighbour count, the observation layout), so it is
        forgotten here and the table's reset rows are recomputed.  Writing `sim.p.<field>` directly skips this: call
        update_params() (or invalidate_plan() + set_fixture_table()) instead."""
        self.sync()
        for k_, v in changes.items():
            if k_ in ("num_envs", "num_agents", "max_obs"):
                raise ValueError("%s is fixed at construction (tensor shapes)" % k_)
            if not hasattr(self.p, k_):
                raise AttributeError("CaParams has no field %r" % k_)
            setattr(self.p, k_, v)
        if self._la is not None:
            self._la["in_kernel"].clear()
            self._la["prep"] = None
        self.invalidate_plan()
        if self._table is not None:
            ar = self._ar
            self.set_fixture_table(self._table, env_id_offset=ar.env_id_offset, case_stride=ar.case_stride,
                                   heading_seed=ar.heading_seed)

    def set_rvo_stochastic(self, heading_noise=None, collab_coeff=None, anti_collab_t=1.0, seed=0, noise_std=0.5):
        """RVOPolicy's two stochastic branches for a whole batch, drawn on the DEVICE (torch's Philox generator) right
        before every step launch and handed to the kernel as CaState.rvo_collab / rvo_heading_noise:
          * heading_noise: bool mask broadcastable to [E, N] -- agents whose policy has `heading_noise` set get
            N(0, noise_std) added to their delta heading each query (policies/RVOPolicy.py:118-119);
          * collab_coeff < 0: anti-collaborative agents (RVOPolicy.py:77-88) -- every agent carries the policy object's
            `use_non_coop_policy` (initially True); whenever its clock is within DT of a multiple of anti_collab_t
            (`round(t % T, 3) < DT or round(T - t % T, 3) < DT`) it is redrawn, True with probability 1 - |c|; the ego's
            collaboration coefficient of the query is 0 while it is True, c otherwise.
        Both None: switched off (the deterministic kernels, pipelined plan included).  The reference draws from numpy's
        global stream, one agent after the other: the batched draws are the same distributions, not the same numbers."""
        self.sync()
        if self._rd is not None and not (heading_noise is None and (collab_coeff is None or collab_coeff >= 0)):
            raise ValueError("set_rvo_stochastic: the batch draws these branches inside the step kernels (set_rvo_draw); "
                             "switch that off first -- one source of the numbers per batch")
        # (whichever branch is not configured below must not keep pointing at a tensor of an earlier configuration)
        self._cs.rvo_collab = None
        self._cs.rvo_heading_noise = None
        if heading_noise is None and (collab_coeff is None or collab_coeff >= 0):
            self._rvo = None
            self._cs.rvo_collab = None
            self._cs.rvo_heading_noise = None
            return
        gen = torch.Generator(device=self.device)
        gen.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        mask = None
        if heading_noise is not None:
            mask = torch.from_numpy(np.array(np.broadcast_to(np.asarray(heading_noise, bool), (self.E, self.N)))).to(self.device)
        self._rvo = dict(gen=gen, mask=mask, std=float(noise_std), T=float(anti_collab_t),
                         c=None if (collab_coeff is None or collab_coeff >= 0) else float(collab_coeff),
                         non_coop=torch.ones((self.E, self.N), dtype=torch.bool, device=self.device),  # RVOPolicy.py:33
                         collab=None, noise=None)
        self.invalidate_plan()

    def _rvo_draw(self):
        """this step's draws (see set_rvo_stochastic): a handful of small device ops, no host synchronisation"""
        r = self._rvo
        if r["c"] is not None:
            t, T, dt = self._state["t"], r["T"], float(self.p.rvo_dt)
            tm = torch.remainder(t, T)
            r3 = lambda x: torch.round(x * 1000.0) / 1000.0        # numpy's scalar round(x, 3)
            redraw = (r3(tm) < dt) | (r3(T - tm) < dt)
            u = torch.rand((self.E, self.N), generator=r["gen"], device=self.device, dtype=torch.float64)
            r["non_coop"] = torch.where(redraw, u < (1.0 - abs(r["c"])), r["non_coop"])   # np.random.choice([True, False], p=[1 - |c|, |c|])
            r["collab"] = torch.where(r["non_coop"], 0.0, r["c"]).to(torch.float32).contiguous()
            self._cs.rvo_collab = r["collab"].data_ptr()
        if r["mask"] is not None:
            z = torch.randn((self.E, self.N), generator=r["gen"], device=self.device, dtype=torch.float64)
            r["noise"] = (z * r["std"] * r["mask"]).contiguous()
            self._cs.rvo_heading_noise = r["noise"].data_ptr()

    def set_rvo_draw(self, seed, heading_noise=None, collab_coeff=None, anti_collab_t=1.0, noise_std=0.5, _address=None):
        """set_rvo_stochastic's two branches drawn INSIDE the step kernels (CaRvoDraw of include/cagpu.h states the rule):
        every draw is a pure function of (seed, global env id, episode, agent slot, episode step), so nothing happens between
        two steps -- step(), rollout() with action tapes / keep_steps / map_sensors, the look-ahead ring, a rewind's replay,
        every shard layout and replay() see the same numbers.  The arguments are set_rvo_stochastic's; `seed` must be != 0 and
        differ from the table's heading_seed, the policy draw's seed and the map set's map_seed.  Both branches off
        (heading_noise None and collab_coeff None or >= 0): switched off.  Having set_rvo_stochastic on as well is a
        ValueError.  The anti-collaborative bit of every agent is bit 18 of its flag word: rvo_noncoop()."""
        self.sync()
        if self._la is not None:
            self._la["in_kernel"].clear()
            self._la["prep"] = None
        self.invalidate_plan()
        c = None if (collab_coeff is None or not collab_coeff < 0) else float(collab_coeff)
        if heading_noise is None and c is None:
            self._rd = None
            return
        if self._rvo is not None:
            raise ValueError("set_rvo_draw: set_rvo_stochastic is on for this batch (draws on the host side of every launch); "
                             "switch it off first -- one source of the numbers per batch")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        taken = [0]
        if self._ar is not None:
            taken.append(int(self._ar.heading_seed))
        if self._draw is not None:
            taken.append(int(self._draw["c"].seed))
        if self._maps is not None:
            taken.append(int(self._maps.map_seed))
        if seed in taken:
            raise ValueError("set_rvo_draw: seed must be != 0 and differ from the table's heading_seed, the policy draw's seed "
                             "and the map set's map_seed")
        if c is not None and not float(anti_collab_t) > 0:
            raise ValueError("set_rvo_draw: anti_collab_t must be > 0")
        if not float(noise_std) >= 0:
            raise ValueError("set_rvo_draw: noise_std must be >= 0")
        mask = None
        if heading_noise is not None:
            mask = torch.from_numpy(np.array(np.broadcast_to(np.asarray(heading_noise, bool), (self.E, self.N)))
                                    .astype(np.uint8)).to(self.device).contiguous()
        addr = None if _address is None else self._dev(np.ascontiguousarray(_address, np.int64).reshape(self.E, 2), torch.int64)
        d = nat.CaRvoDraw(seed=seed, collab_coeff=0.0 if c is None else c, anti_collab_t=float(anti_collab_t),
                          noise_std=float(noise_std), noise_mask=None if mask is None else mask.data_ptr(),
                          address=None if addr is None else addr.data_ptr())
        tape = nat.CaActionTape()
        self._rd = dict(c=d, ref=C.byref(d), mask=mask, addr=addr, tape=tape, tape_ref=C.byref(tape),
                        args=dict(seed=seed, collab_coeff=c, anti_collab_t=float(anti_collab_t), noise_std=float(noise_std)))

    def _noise(self, p, s, o, ext, ar, sx, stream, stride=0):
        """the one native call of a batch with set_rvo_draw: cagpu_step_noise (every launch form goes through here)"""
        rd = self._rd
        tape_ref = None
        if ext is not None:
            rd["tape"].actions, rd["tape"].step_stride = ext, stride
            tape_ref = rd["tape_ref"]
        return self.lib.cagpu_step_noise(p, s, o, tape_ref, ar, sx, None if self._draw is None else self._draw["ref"],
                                         rd["ref"], stream)

    def rvo_noncoop(self):
        """bool [E, N]: RVOPolicy's `use_non_coop_policy` of every agent slot as the step last handed out left it (bit 18 of
        the flag word, CA_RVO_NONCOOP; through sync()).  All False without set_rvo_draw(collab_coeff < 0)."""
        return (self.state["flags"] & nat.RVO_NONCOOP) != 0

    def set_sensor_variants(self, variants=None):
        """Agents of one batch whose OtherAgentsStatesSensor arguments differ (the reference gives every agent its own
        sensor object: `sensor.set_args({'agent_sorting_method': ..., 'max_num_other_agents_observed': ...})`,
        sensors/Sensor.py:19-23).  The kernels take ONE obs_clip / sort_mode per launch -- CaParams holds the primary pair --
        so every further pair costs one cagpu_observe launch per step: `variants` = [(mask, obs_clip, sort_mode), ...] with
        mask a bool array broadcastable to [E, N]; after every step / reset / observe the rows of the masked agents are
        replaced by their rows under that pair.  None / []: switched off."""
        self.sync()
        if variants and self._fin_on:
            raise nat.CagpuError("set_sensor_variants: the final record (keep_final) holds the rows the step kernel produced "
                                 "under the primary sensor arguments; per-agent variants are rewritten on the host after the "
                                 "launch and are not applied to it -- switch one of the two off")
        self._variants = []
        for mask, clip, sort in (variants or []):
            m = torch.from_numpy(np.array(np.broadcast_to(np.asarray(mask, bool), (self.E, self.N)))).to(self.device)
            if not (0 <= int(clip) <= self.K):
                raise ValueError("obs_clip %d outside [0, %d]" % (clip, self.K))
            self._variants.append((m.unsqueeze(-1), int(clip), int(sort), torch.empty_like(self._obs)))

    def _apply_sensor_variants(self):
        if not self._variants:
            return
        p, co = self.p, self._co
        keep = (p.obs_clip, p.sort_mode, co.obs)
        try:
            for m, clip, sort, buf in self._variants:
                p.obs_clip, p.sort_mode, co.obs = clip, sort, buf.data_ptr()
                nat.check(self.lib.cagpu_observe(C.byref(p), C.byref(self._cs), C.byref(co), self._stream()))
                torch.where(m, buf, self._obs, out=self._obs)   # (elementwise, no host synchronisation)
        finally:
            p.obs_clip, p.sort_mode, co.obs = keep

    def invalidate_plan(self):
        """Forget the pipelined policy query (CaState.next_action): call after writing state tensors directly."""
        self.sync()
        self._state["flags"].bitwise_and_(~nat.PLAN_VALID)

    # ---------------------------------------------------------------- configuration
    def set_plugins(self, policy, dynamics=None, is_learning=None, still_learning=None):
        """policy / dynamics: int ids (CA_POL_*, CA_DYN_*), broadcastable to [E,N].  The learning bits default to
        what the reference's policy classes set (LearningPolicy.py:9-11: str == 'learning', is_still_learning)."""
        self.sync()
        E, N = self.E, self.N
        pol = np.broadcast_to(np.asarray(policy, np.int64), (E, N))
        dyn = np.broadcast_to(np.asarray(0 if dynamics is None else dynamics, np.int64), (E, N))
        learn = (pol == nat.POL_LEARNING) | (pol == nat.POL_LEARNING_GA3C)
        isl = learn if is_learning is None else np.broadcast_to(np.asarray(is_learning, bool), (E, N))
        stl = learn if still_learning is None else np.broadcast_to(np.asarray(still_learning, bool), (E, N))
        bits = (pol << nat.POLICY_SHIFT) | (dyn << nat.DYNAMICS_SHIFT) | (isl * nat.IS_LEARNING) | \
               (stl * nat.STILL_LEARNING)
        cur = self._state["flags"]
        self._plugin_words = bits.astype(np.int32)
        cur.copy_((cur & (0x3F | nat.ABSENT)) | torch.as_tensor(self._plugin_words, device=self.device))
        self._plugins_ga3c = bool((pol == nat.POL_GA3C_CADRL).any())
        self._has_ga3c = self._plugins_ga3c or (self._draw is not None and self._draw["has_ga3c"])

    def ga3c_rows(self):
        """number of agents the last ga3c() call evaluated (device -> host read: synchronises)"""
        return int(self._net_tensors["rows_scratch"][self.E * self.N].item())

    def load_ga3c(self, weights=None, keep_logits=False, index=0, keep_value=False):
        """Upload the GA3C-CADRL network (GA3CCADRLPolicy.initialize_network, GA3CCADRLPolicy.py:23-47).  `weights`:
        an .npz written by oracle/extract_ga3c_weights.py (default: the shipped IROS18/network_01900000, the
        reference's default checkpoint) or a dict of float32 arrays with the same keys.
        `index`: several checkpoints may be loaded side by side (index 0, 1, ...); set_ga3c_assignment() says which agent
        runs which (the reference gives every agent its own policy object and session).  Without an assignment every
        GA3C-CADRL agent runs checkpoint 0.
        keep_value: also evaluate the network's value head (logits_v_kernel / logits_v_bias of the weights, the graph's
        `Squeeze:0`) in the same launch; `ga3c_value` [E, N] then holds it for the agents ga3c() evaluated (other entries
        keep what they held).  ValueError if the weights carry no value head."""
        self.sync()
        ts = _ga3c_weight_tensors(weights, self.device)
        if keep_value and "value_kernel" not in ts:
            raise ValueError("keep_value=True, but these GA3C-CADRL weights have no logits_v_kernel / logits_v_bias")
        # scratch of cagpu_ga3c: the packed list of the agents that need an action this step (+ their count)
        ts["rows_scratch"] = torch.empty((self.E * self.N + 6,), dtype=torch.int32, device=self.device)
        # the four big matrices as fp16 planes in matrix-core fragment order: split once per checkpoint on the device
        ts["packed"] = torch.empty((int(self.lib.cagpu_ga3c_packed_bytes()),), dtype=torch.uint8, device=self.device)
        net = nat.CaNet(**{f: ts[f].data_ptr() for f in nat.NET_FIELDS + ("rows_scratch", "packed")})
        nat.check(self.lib.cagpu_ga3c_pack(C.byref(net), ts["packed"].data_ptr(), ts["packed"].numel(), self._stream()))
        self._nets[int(index)] = (net, ts)
        if int(index) == 0 or self._net is None:
            self._net_tensors, self._net = ts, net
        if keep_logits or self.ga3c_logits is None:
            self.ga3c_logits = torch.zeros((self.E, self.N, 11), dtype=torch.float32, device=self.device) \
                if keep_logits else None
        if keep_value and self.ga3c_value is None:
            self.ga3c_value = torch.zeros((self.E, self.N), dtype=torch.float32, device=self.device)

    def set_ga3c_assignment(self, index):
        """index: int array broadcastable to [E, N] -- the checkpoint (load_ga3c(..., index=)) each GA3C-CADRL agent runs;
        None: everybody runs checkpoint 0."""
        if index is None:
            self._agent_net = None
            return
        a = np.array(np.broadcast_to(np.asarray(index, np.int32), (self.E, self.N)))   # (a writable copy for torch.from_numpy)
        missing = set(np.unique(a).tolist()) - set(self._nets)
        if missing:
            raise nat.CagpuError("GA3C-CADRL checkpoint index %s assigned but not loaded" % sorted(missing))
        self._agent_net = torch.from_numpy(a).to(self.device)

    def ga3c(self, ext=None, fused=None):
        """Query the network for every live GA3C-CADRL agent on the CURRENT observation; the action indices land in
        `ext[..., 0]` (a float64 [E,N,2] tensor, allocated here if not given), which step() then consumes.
        fused (default: self.ga3c_fused): the kernel computes the ego-centric observation of the agents it evaluates from
        the state arrays itself (cagpu_ga3c with obs = NULL: "obs + network inference fused in-kernel") instead of reading
        the rows the last step stored -- same bits; needs num_agents <= 32, no time_to_impact sorting and no per-agent
        sensor variants.
        With set_ga3c_sampling (or inside collect()) the sampler launch follows the network launch(es): the agents that
        sample get their drawn index in `ext`, and ga3c_logp / ga3c_entropy / ga3c_action are written."""
        self.sync()
        if self._net is None:
            raise nat.CagpuError("GA3C-CADRL agents present but no network loaded: call load_ga3c() "
                                 "(policy.initialize_network() in the env API)")
        if ext is None:
            if self._ga3c_ext is None:
                self._ga3c_ext = torch.zeros((self.E, self.N, 2), dtype=torch.float64, device=self.device)
            ext = self._ga3c_ext
        sampler = self._samp is not None or self._xp is not None
        if sampler and self.ga3c_logits is None and self._samp_logits is None:   # (the sampler reads the logits: its own copy)
            self._samp_logits = torch.zeros((self.E, self.N, 11), dtype=torch.float32, device=self.device)
        lgt = self.ga3c_logits if self.ga3c_logits is not None else (self._samp_logits if sampler else None)
        lg = None if lgt is None else lgt.data_ptr()
        fused = self.ga3c_fused if fused is None else fused
        if fused and (self.N > 32 or self.p.sort_mode == nat.SORT_TIME_TO_IMPACT or self._variants):
            fused = False
        obs_ptr = None if fused else self._obs.data_ptr()
        if self.ga3c_value is not None:
            self._ga3c_with_value(ext, obs_ptr, lg)
        elif self._agent_net is None:      # one checkpoint (index 0) for every GA3C-CADRL agent
            nat.check(self.lib.cagpu_ga3c(C.byref(self.p), C.byref(self._cs), obs_ptr, C.byref(self._net),
                                          ext.data_ptr(), lg, self._stream()))
        else:
            for idx in sorted(self._nets):   # one launch per checkpoint, each over its own agents (CaNet.agent_net / net_index)
                net = self._nets[idx][0]
                net.agent_net, net.net_index = self._agent_net.data_ptr(), idx
                nat.check(self.lib.cagpu_ga3c(C.byref(self.p), C.byref(self._cs), obs_ptr, C.byref(net),
                                              ext.data_ptr(), lg, self._stream()))
                net.agent_net = None
        if sampler:
            self._ga3c_sample(ext, lgt)
        return ext

    def _ga3c_with_value(self, ext, obs_ptr, lg, value=None):
        """ga3c() with the value head (load_ga3c(keep_value=True)): cagpu_ga3c_value instead of cagpu_ga3c, the same
        launches otherwise; every checkpoint writes the value of its own agents into ga3c_value (or `value`)"""
        value = self.ga3c_value if value is None else value

        def launch(net, ts):
            if "value_kernel" not in ts:
                raise ValueError("ga3c_value is kept, but a loaded GA3C-CADRL checkpoint has no value head")
            v = nat.CaNetValue(value_kernel=ts["value_kernel"].data_ptr(), value_bias=ts["value_bias"].data_ptr(),
                               value=value.data_ptr())
            nat.check(self.lib.cagpu_ga3c_value(C.byref(self.p), C.byref(self._cs), obs_ptr, C.byref(net), ext.data_ptr(), lg,
                                                C.byref(v), self._stream()))
        if self._agent_net is None:
            launch(self._net, self._net_tensors)
            return ext
        for idx in sorted(self._nets):
            net, ts = self._nets[idx]
            net.agent_net, net.net_index = self._agent_net.data_ptr(), idx
            try:
                launch(net, ts)
            finally:
                net.agent_net = None
        return ext

    # ---------------------------------------------------------------- the sampled policy and the experience tape
    def set_ga3c_sampling(self, seed, temperature=1.0, mask=None, _address=None):
        """GA3C-CADRL agents SAMPLE their action from the softmax of the logits (CaGa3cSample of include/cagpu.h states the
        rule) instead of playing the argmax: a launch of its own behind the network launch of every ga3c() call.  Every draw
        is a pure function of (seed, global env id, episode, agent slot, episode step) and the logits row, so step(),
        collect(), every shard layout and replay() see the same numbers.  seed: an int != 0 that differs from the table's
        heading_seed, the policy draw's seed, the map set's map_seed and the RVO draw's seed; None: switched off (greedy).
        temperature > 0 divides the logits.  mask: bool broadcastable to [E, N], the agents that sample (None: every
        GA3C-CADRL agent); the others keep the argmax.  ga3c_logp / ga3c_entropy / ga3c_action [E, N] then hold the last
        step's log-probability of the index played, the entropy and the index, for the agents that were evaluated."""
        self.sync()
        if seed is None:
            self._samp = None
            return
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        taken = [0]
        if self._ar is not None:
            taken.append(int(self._ar.heading_seed))
        if self._draw is not None:
            taken.append(int(self._draw["c"].seed))
        if self._maps is not None:
            taken.append(int(self._maps.map_seed))
        if self._rd is not None:
            taken.append(int(self._rd["c"].seed))
        if seed in taken:
            raise ValueError("set_ga3c_sampling: seed must be != 0 and differ from the table's heading_seed, the policy draw's "
                             "seed, the map set's map_seed and the RVO draw's seed")
        if not (float(temperature) > 0 and math.isfinite(float(temperature))):
            raise ValueError("set_ga3c_sampling: temperature must be > 0 and finite")
        m = None
        if mask is not None:
            m = torch.from_numpy(np.array(np.broadcast_to(np.asarray(mask, bool), (self.E, self.N))).astype(np.uint8)) \
                .to(self.device).contiguous()
        addr = None if _address is None else self._dev(np.ascontiguousarray(_address, np.int64).reshape(self.E, 2), torch.int64)
        self._samp = dict(seed=seed, temperature=float(temperature), mask=m, addr=addr)

    def _sample_buffers(self):
        if self.ga3c_logp is None:
            z = lambda dt: torch.zeros((self.E, self.N), dtype=dt, device=self.device)
            self.ga3c_logp, self.ga3c_entropy, self.ga3c_action = z(torch.float32), z(torch.float32), z(torch.int8)

    def _ga3c_sample(self, ext, logits):
        """the sampler launch behind the network launch(es) of a ga3c() call: cagpu_ga3c_sample over every evaluated agent
        (of whichever checkpoint), greedy without set_ga3c_sampling; with a tape slot (collect) its pre-step record"""
        self._sample_buffers()
        g, sm, xp = self._cg, self._samp, self._xp
        g.greedy = 1 if sm is None else 0
        g.seed = 0 if sm is None else sm["seed"]
        g.temperature = 1.0 if sm is None else sm["temperature"]
        g.mask = None if sm is None or sm["mask"] is None else sm["mask"].data_ptr()
        g.address = None if sm is None or sm["addr"] is None else sm["addr"].data_ptr()
        g.agent_net = None      # (one launch for the agents of every checkpoint: an assignment names loaded checkpoints only)
        g.logits = logits.data_ptr()
        g.entropy = self.ga3c_entropy.data_ptr()
        g.obs = self._obs.data_ptr()
        g.value = None if self.ga3c_value is None else self.ga3c_value.data_ptr()
        if xp is None:
            g.logp, g.action = self.ga3c_logp.data_ptr(), self.ga3c_action.data_ptr()
            g.slot_obs = g.slot_value = g.slot_live = g.slot_address = None
        else:
            g.logp, g.action = xp["logp"], xp["action"]
            g.slot_obs, g.slot_value, g.slot_live, g.slot_address = xp["obs"], xp["value"], xp["live"], xp["address"]
        nat.check(self.lib.cagpu_ga3c_sample(self._p_ref, self._cs_ref, self._ar_ref,
                                             None if self._draw is None else self._draw["ref"],
                                             None if self._maps is None else C.byref(self._maps),
                                             None if self._rd is None else self._rd["ref"],
                                             C.byref(g), ext.data_ptr(), self._stream()))

    def experience_step_bytes(self, keep_obs=True):
        """bytes of one step of an experience tape: 14 per agent slot (action, logp, value, live, reward, done) + 17 per env
        (game_over, address), + 4 (W - 1) per agent slot with the observation rows"""
        return self.E * self.N * (14 + (4 * (self.W - 1) if keep_obs else 0)) + 17 * self.E

    def collect(self, n, keep_obs=True):
        """Play n steps and keep the on-policy record of the batch's GA3C-CADRL agents on the device -> Experience (device
        tensors, slot t = step t of this call):
          obs [n, E, N, W - 1] float32 (keep_obs): the row the network read -- the pre-step observation minus is_learning
          action [n, E, N] int8, logp [n, E, N] float32: the index played and its log-probability
          value [n, E, N] float32: the value head of the same forward pass
          live [n, E, N] bool: the agent was evaluated in that step (a GA3C-CADRL agent that was not done); every field
                               above is zero where it is False
          reward [n, E, N] float32, done [n, E, N] bool, game_over [n, E] bool: what the step gave
          last_value [E, N] float32: one more network launch with the value head on the observation after step n - 1 (zero
                               for agents it did not evaluate); it samples nothing and advances nothing
          address [n, E, 2] int64: (global env id, episode) of every env before the step
        The pre-step fields are written by the sampler launch of every step (cagpu_ga3c_sample's slot pointers), the
        post-step fields by the step kernel itself (CaOut points at the slot); no host synchronisation between the first
        launch and the return.  Greedy without set_ga3c_sampling (logp of the argmax).  Needs load_ga3c(keep_value=True).
        The tape counts against experience_max_bytes: a call that would exceed it raises CagpuError before anything is
        launched."""
        n = int(n)
        if n < 1:
            raise ValueError("collect: n must be >= 1")
        self.sync()
        if self._la is not None:
            raise nat.CagpuError("collect: switch the look-ahead ring off first (the network runs between the steps)")
        if self._net is None or self.ga3c_value is None or not self._has_ga3c:
            raise nat.CagpuError("collect: needs GA3C-CADRL agents and load_ga3c(keep_value=True) (env.keep_ga3c_value = True "
                                 "in the env API)")
        per = self.experience_step_bytes(keep_obs)
        total = n * per + 4 * self.E * self.N
        if total > self.experience_max_bytes:
            raise nat.CagpuError("experience tape: %d steps of %d bytes do not fit experience_max_bytes = %d%s; no step was taken"
                                 % (n, per, self.experience_max_bytes,
                                    " -- keep_obs=False takes %d bytes per step" % self.experience_step_bytes(False)
                                    if keep_obs else ""))
        if self._traj_on and self._traj_fit() < n:
            raise nat.CagpuError("collect: the trajectory tape holds %d more steps, %d were asked for; no step was taken"
                                 % (self._traj_fit(), n))
        E, N, dev = self.E, self.N, self.device
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        t = dict(obs=z((n, E, N, self.W - 1), torch.float32) if keep_obs else None, action=z((n, E, N), torch.int8),
                 logp=z((n, E, N), torch.float32), value=z((n, E, N), torch.float32), live=z((n, E, N), torch.uint8),
                 reward=z((n, E, N), torch.float32), done=z((n, E, N), torch.uint8), game_over=z((n, E), torch.uint8),
                 last_value=z((E, N), torch.float32), address=z((n, E, 2), torch.int64))
        self._sample_buffers()
        co = self._co
        keep = (co.rewards, co.done, co.game_over, self.fresh_outputs)
        self.fresh_outputs = False
        # (slot addresses by arithmetic: nine tensor views per step would cost more host time than the sampler launch)
        at = {k: (v.data_ptr(), v[0].numel() * v.element_size()) for k, v in t.items() if v is not None}
        ptr = lambda name, i: at[name][0] + i * at[name][1] if name in at else None
        try:
            for i in range(n):
                self._xp = {k: ptr(k, i) for k in ("obs", "action", "logp", "value", "live", "address")}
                co.rewards, co.done, co.game_over = ptr("reward", i), ptr("done", i), ptr("game_over", i)
                self.step()
        finally:
            self._xp = None
            co.rewards, co.done, co.game_over, self.fresh_outputs = keep
        # the sim's own outputs and last-step records follow the last slot
        self._rewards.copy_(t["reward"][n - 1])
        self._done.copy_(t["done"][n - 1])
        self._game_over.copy_(t["game_over"][n - 1])
        last_live = t["live"][n - 1] != 0
        torch.where(last_live, t["logp"][n - 1], self.ga3c_logp, out=self.ga3c_logp)
        torch.where(last_live, t["action"][n - 1], self.ga3c_action, out=self.ga3c_action)
        # the value of the observation after the last step: the network alone, into the tape
        if self._ga3c_ext2 is None:
            self._ga3c_ext2 = torch.zeros((E, N, 2), dtype=torch.float64, device=dev)
        fused = self.ga3c_fused and not (N > 32 or self.p.sort_mode == nat.SORT_TIME_TO_IMPACT or self._variants)
        self._ga3c_with_value(self._ga3c_ext2, None if fused else self._obs.data_ptr(), None, value=t["last_value"])
        return Experience(self, t)

    def update_ga3c(self, tensors, index=0):
        """New weights for a loaded GA3C-CADRL network without leaving the device: `tensors` is a dict of float32 tensors on
        this sim's device under the checkpoint's own keys and shapes (lstm_kernel ... logits_p_kernel, logits_p_bias,
        input_mean, input_std, and logits_v_kernel [256, 1] / logits_v_bias [1] for a network loaded with a value head); any
        subset.  They are copied into the network's buffers IN PLACE (no reallocation, no host round trip) and the matrix
        planes are packed again (cagpu_ga3c_pack).  ValueError, before anything is copied: an unknown key, a wrong shape,
        dtype or device, or logits_v_* for a network without a value head."""
        self.sync()
        if int(index) not in self._nets:
            raise nat.CagpuError("update_ga3c: no GA3C-CADRL checkpoint loaded at index %s" % index)
        net, ts = self._nets[int(index)]
        dst = {_GA3C_NAMES.get(f, f): (ts[f], _GA3C_SHAPES[f]) for f in nat.NET_FIELDS}
        if "value_kernel" in ts:
            dst["logits_v_kernel"], dst["logits_v_bias"] = (ts["value_kernel"], (256, 1)), (ts["value_bias"], (1,))
        todo = []
        for k, v in tensors.items():
            if k not in dst:
                raise ValueError("update_ga3c: unknown key %r (expected a subset of %s)" % (k, sorted(dst)))
            d, shape = dst[k]
            if not torch.is_tensor(v) or v.dtype != torch.float32 or v.device != d.device or tuple(v.shape) != tuple(shape):
                raise ValueError("update_ga3c: %s must be a float32 tensor of shape %s on %s" % (k, tuple(shape), d.device))
            todo.append((d, v))
        for d, v in todo:
            d.copy_(v.reshape(d.shape))
        nat.check(self.lib.cagpu_ga3c_pack(C.byref(net), ts["packed"].data_ptr(), ts["packed"].numel(), self._stream()))

    def generate_cases(self, num_cases, seed, side_length=4.0, speed_bnds=(0.5, 2.0), radius_bnds=(0.2, 0.8),
                       return_status=False, num_agents=None, return_counts=False):
        """`num_cases` random scenarios for this sim's agent count, drawn ON THE DEVICE by cagpu_generate_cases
        (generate_rand_test_case_multi behind test_cases.get_testcase_random, test_cases.py:212-253): float64 device
        tensor [num_cases, N, 6], ready for reset() / set_fixture_table().  `side_length`: a number, or (lo, hi) to draw
        it per case.  Same (seed, case index) -> same scenario.

        `num_agents=(lo, hi)`: a RAGGED table (cagpu_generate_cases_ragged) -- the agent count of every case drawn in
        lo .. hi <= N like the reference's num_agents=None (test_cases.py:224-227), rows past it zero (empty slots; the
        sim must be built with ragged=1); `side_length` is then a number, (lo, hi), or the reference's list of
        {"num_agents": [lo, hi), "side_length": [lo, hi]} dicts (config.py:118-131)."""
        out = torch.empty((int(num_cases), self.N, 6), dtype=torch.float64, device=self.device)
        status = torch.zeros((int(num_cases),), dtype=torch.int32, device=self.device)
        counts = None
        sp = (float(speed_bnds[0]), float(speed_bnds[1]), float(radius_bnds[0]), float(radius_bnds[1]))
        if num_agents is None and not isinstance(side_length, list):
            lo, hi = (side_length, side_length) if np.isscalar(side_length) else side_length
            nat.check(self.lib.cagpu_generate_cases(int(num_cases), self.N, float(lo), float(hi), *sp,
                                                    int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(), status.data_ptr(),
                                                    self._stream()))
        else:
            n_lo, n_hi = (self.N, self.N) if num_agents is None else (int(num_agents[0]), int(num_agents[1]))
            if isinstance(side_length, list):
                rg = [[c["num_agents"][0], c["num_agents"][1], c["side_length"][0], c["side_length"][1]]
                      for c in side_length]
            else:
                lo, hi = (side_length, side_length) if np.isscalar(side_length) else side_length
                rg = [[0, 1 << 30, lo, hi]]
            rg = np.ascontiguousarray(rg, dtype=np.float64)
            counts = torch.zeros((int(num_cases),), dtype=torch.int32, device=self.device)
            nat.check(self.lib.cagpu_generate_cases_ragged(int(num_cases), self.N, n_lo, n_hi, rg.ctypes.data, len(rg), *sp,
                                                           int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(),
                                                           counts.data_ptr(), status.data_ptr(), self._stream()))
        res = (out,) + ((status,) if return_status else ()) + ((counts,) if return_counts else ())
        return res if len(res) > 1 else out

    @staticmethod
    def _case_dist(N, side_length, num_agents):
        """the generator's distribution arguments in the form cagpu_generate_cases_at takes them -> (n_min, n_max,
        host float64 array, n_ranges); the same mapping generate_cases() applies to its two entry points"""
        if num_agents is None and not isinstance(side_length, list):
            lo, hi = (side_length, side_length) if np.isscalar(side_length) else side_length
            return 0, 0, np.ascontiguousarray([lo, hi], dtype=np.float64), 0
        n_lo, n_hi = (N, N) if num_agents is None else (int(num_agents[0]), int(num_agents[1]))
        if isinstance(side_length, list):
            rg = [[c["num_agents"][0], c["num_agents"][1], c["side_length"][0], c["side_length"][1]] for c in side_length]
        else:
            lo, hi = (side_length, side_length) if np.isscalar(side_length) else side_length
            rg = [[0, 1 << 30, lo, hi]]
        rg = np.ascontiguousarray(rg, dtype=np.float64)
        return n_lo, n_hi, rg, len(rg)

    def generate_cases_at(self, case_index, seed, side_length=4.0, speed_bnds=(0.5, 2.0), radius_bnds=(0.2, 0.8),
                          num_agents=None, out=None, out_row=None, count=None, counts=None, status=None,
                          return_status=False, return_counts=False):
        """The scenarios of the given 64-bit case indices (cagpu_generate_cases_at: one wave per case, bit for bit what
        generate_cases() gives the same (seed, index)): `case_index` int64 [M] (device tensor or array-like); the
        distribution arguments are those of generate_cases().  Entry m lands in row out_row[m] of `out` (default: a new
        [M, N, 6] table, row m); `count`: a device int32 [1] tensor -- only the first min(count, M) entries are
        generated, read on the device.  `counts` / `status`: int32 tensors of out's rows to write into (default: new)."""
        ci = self._dev(case_index, torch.int64).reshape(-1)
        M = int(ci.shape[0])
        if out is None:
            if out_row is not None:
                raise ValueError("generate_cases_at: out_row needs the table `out` its rows index")
            out = torch.zeros((M, self.N, 6), dtype=torch.float64, device=self.device)
        assert out.is_contiguous() and out.dtype == torch.float64 and tuple(out.shape[1:]) == (self.N, 6), out.shape
        R = int(out.shape[0])
        rows = self._dev(out_row, torch.int64)
        if rows is not None:
            rows = rows.reshape(-1)
            # (a convenience call, not the product path: the rows are checked here, the kernel trusts them)
            if int(rows.shape[0]) != M or (M and (int(rows.min()) < 0 or int(rows.max()) >= R)):
                raise ValueError("generate_cases_at: out_row must hold %d rows inside [0, %d)" % (M, R))
        elif M > R:
            raise ValueError("generate_cases_at: %d cases do not fit a table of %d rows" % (M, R))
        counts = torch.zeros((R,), dtype=torch.int32, device=self.device) if counts is None else counts
        status = torch.zeros((R,), dtype=torch.int32, device=self.device) if status is None else status
        assert counts.shape[0] == R and status.shape[0] == R and counts.dtype == status.dtype == torch.int32
        n_lo, n_hi, rg, n_rg = self._case_dist(self.N, side_length, num_agents)
        sp = (float(speed_bnds[0]), float(speed_bnds[1]), float(radius_bnds[0]), float(radius_bnds[1]))
        nat.check(self.lib.cagpu_generate_cases_at(ci.data_ptr() if M else None, None if rows is None else rows.data_ptr(),
                                                   None if count is None else count.data_ptr(), M, self.N, n_lo, n_hi,
                                                   rg.ctypes.data, n_rg, *sp, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                   out.data_ptr(), counts.data_ptr(), status.data_ptr(), self._stream()))
        self._keep = [ci, rows, count]   # keep alive until the stream has consumed them
        res = (out,) + ((status,) if return_status else ()) + ((counts,) if return_counts else ())
        return res if len(res) > 1 else out

    def set_case_stream(self, window=8, seed=0, side_length=4.0, speed_bnds=(0.5, 2.0), radius_bnds=(0.2, 0.8),
                        num_agents=None, heading_seed=0, env_id_offset=0):
        """A FRESH random scenario at every on-device auto-reset (include/cagpu.h CaCaseStream) -- the reference's default
        training configuration, Config.TEST_CASE_FN = "get_testcase_random", which builds a new scenario at every reset():
        episode k of the env with global id g = env_id_offset + e runs scenario(seed, case index (g << 32) | k) of the
        device generator (the distribution arguments are those of generate_cases(); `num_agents=(lo, hi)` needs a sim
        built with ragged=1), whatever the batch size, the sharding, the window or the launch pattern.  The auto-reset
        table becomes a window of `window` upcoming episodes per env ([E * window, N, 6], case_stride = E), and a refill
        (cagpu_stream_refill, no host synchronisation) regenerates the used-up rows ahead of every rollout() and ring
        launch, every max(1, window - 1) single steps and after a host reset().  An env that auto-resets more than
        `window` times between two refills repeats a scenario and raises bit 3 of the fault word (check_faults()).
        Policy draw, final record, episode log, trajectory tape and map set attach to it as to a fixture table (the
        episode log's `case` is the window row; stream_case_index() names the scenario).  window=None: detach, like
        set_fixture_table(None).  A host reset restarts the envs it touches at episode 0: they REPLAY their sequence
        unless `seed` is changed, like cases, headings and policies today."""
        self.sync()
        if self._la is not None:
            self._la["in_kernel"].clear()
            self._la["prep"] = None
        if window is None:
            self._cstream = None
            self.set_fixture_table(None)
            return
        E, N, W, dev = self.E, self.N, int(window), self.device
        if W < 1 or E * W > 0x7FFFFFFF:
            raise ValueError("set_case_stream: window must be >= 1 and num_envs * window < 2^31")
        off = int(env_id_offset)
        if off < 0 or off + E > 1 << 32:
            raise ValueError("set_case_stream: global env ids (env_id_offset + e) must be < 2^32")
        if num_agents is not None and not self.p.ragged:
            raise ValueError("set_case_stream: num_agents=(lo, hi) draws an agent count per episode -- build the sim with ragged=1")
        hs = int(heading_seed) & 0xFFFFFFFFFFFFFFFF
        if self._draw is not None and self._draw["c"].seed == hs:
            raise ValueError("heading_seed equals the policy draw's seed: an agent's heading and policy would be the same uniform")
        n_lo, n_hi, rg, n_rg = self._case_dist(N, side_length, num_agents)
        t = dict(table=torch.zeros((E * W, N, 6), dtype=torch.float64, device=dev),
                 held=torch.full((E, W), -1, dtype=torch.int32, device=dev),
                 seen=torch.zeros((E,), dtype=torch.int32, device=dev),
                 work_index=torch.zeros((E * W,), dtype=torch.int64, device=dev),
                 work_row=torch.zeros((E * W,), dtype=torch.int64, device=dev),
                 work_count=torch.zeros((1,), dtype=torch.int32, device=dev),
                 counts=torch.zeros((E * W,), dtype=torch.int32, device=dev),
                 status=torch.zeros((E * W,), dtype=torch.int32, device=dev))
        c = nat.CaCaseStream(window=W, n_min=n_lo, n_max=n_hi, n_ranges=n_rg, side_ranges=rg.ctypes.data,
                             speed_lo=float(speed_bnds[0]), speed_hi=float(speed_bnds[1]), radius_lo=float(radius_bnds[0]),
                             radius_hi=float(radius_bnds[1]), seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                             **{k_: v.data_ptr() for k_, v in t.items()})
        self._table, self._reset_obs, self._reset_plan = None, None, None
        self._ar = nat.CaAutoReset(table=t["table"].data_ptr(), n_cases=E * W, env_id_offset=off, case_stride=E,
                                   reset_obs=None, reset_plan=None, heading_seed=hs)
        self._ar_ref = C.byref(self._ar)
        self._cstream = dict(c=c, ref=C.byref(c), t=t, rg=rg, W=W, every=max(1, W - 1), since=0, refills=0,
                             refill=self.lib.cagpu_stream_refill,
                             dist=dict(side_length=side_length, speed_bnds=tuple(speed_bnds), radius_bnds=tuple(radius_bnds),
                                       num_agents=num_agents), seed=int(seed) & 0xFFFFFFFFFFFFFFFF, off=off)
        self._stream_refill()   # the window holds the episodes behind the one every env is in from here on

    def _stream_refill(self):
        """cagpu_stream_refill on the current stream.  Called only where the device state is the state LAST HANDED OUT
        (after sync(): ahead of a rollout / ring launch, between single steps, after a host reset).  INVARIANT: a refill
        replaces only rows of episodes <= the handed-out reset_count -- episodes that were loaded already -- and a rewind
        goes back to a snapshot taken BEHIND a refill, so the replay of a rewind never needs a replaced row."""
        st = self._cstream
        rc = st["refill"](self._p_ref, self._cs_ref, self._ar_ref, st["ref"], self._stream_handle())
        if rc != 0:
            nat.check(rc)
        st["since"] = 0
        st["refills"] += 1

    def stream_case_index(self, env, episode):
        """the 64-bit case index of episode `episode` of this shard's env `env` under the attached stream (ints or
        integer arrays, broadcast): (global env id << 32) | episode -- what generate_cases_at() takes"""
        assert self._cstream is not None, "set_case_stream() first"
        g = np.asarray(env, np.int64) + self._cstream["off"]
        out = (g << 32) | np.asarray(episode, np.int64)
        return int(out) if out.ndim == 0 else out

    def reset_from_stream(self):
        """Initial load under a case stream: every env <- episode 0 of its own sequence (cagpu_generate_cases_at + cagpu_reset),
        and the window filled with the episodes behind it."""
        st = self._cstream
        assert st is not None, "set_case_stream() first"
        idx = (torch.arange(self.E, device=self.device, dtype=torch.int64) + st["off"]) << 32
        return self.reset(self.generate_cases_at(idx, st["seed"], **st["dist"]))

    def set_fixture_table(self, table, env_id_offset=0, case_stride=None, heading_seed=0):
        """Enable DummyVecEnv-style auto-reset from a fixture table [C,N,6] (vec_env.py:120-128,
        test_cases.py:593-624): env e's k-th reset loads case (env_id_offset + e + k*case_stride) % C.
        heading_seed != 0: training mode (test_cases.py:558-559) -- an auto-reset draws the initial heading uniformly in
        [-pi, pi) on the device (Philox of seed, global env id, reset count, agent) instead of pointing at the goal."""
        self.sync()
        if self._la is not None:
            self._la["in_kernel"].clear()
            self._la["prep"] = None
        self._cstream = None    # (a table, or none, replaces a case stream)
        if table is None:
            self._ar, self._ar_ref, self._table = None, None, None
            if self._draw is not None:  # (no auto-reset, nothing is ever drawn: the policy draw goes with the table)
                self.set_policy_draw(None)
            if self._fin_on:        # (no auto-reset, nothing is overwritten: the final record goes with the table)
                self.keep_final(False)
            if self._log is not None:   # (... and no episode is ever logged)
                self.log_episodes(on=False)
            if self._met is not None:   # (... or measured)
                self.measure_episodes(on=False)
            return
        t = self._dev(table, torch.float64)
        assert t.dim() == 3 and t.shape[1:] == (self.N, 6), t.shape
        self._table = t
        # the reset observation of every case, computed once by the reset kernel itself on a scratch batch of C envs
        C_ = int(t.shape[0])
        ps = nat.CaParams.from_buffer_copy(self.p)
        ps.num_envs = C_
        scratch = BatchedSim(ps, device=self.device, pipeline=self.pipeline)
        scratch.reset(t)
        self._reset_obs = scratch.obs
        # ... and, for the pipelined step kernel, the first action of every case (CaAutoReset.reset_plan): an RVO agent's
        # plan depends on positions / velocities / radii only, so the scratch batch may take every slot for an RVO agent
        self._reset_plan = None
        if self.pipeline and scratch.try_plan():
            self._reset_plan = scratch.state["next_action"]
        torch.cuda.current_stream(self.device).synchronize()
        self._ar = nat.CaAutoReset(table=t.data_ptr(), n_cases=C_, env_id_offset=int(env_id_offset),
                                   case_stride=int(self.E if case_stride is None else case_stride),
                                   reset_obs=self._reset_obs.data_ptr(),
                                   reset_plan=None if self._reset_plan is None else self._reset_plan.data_ptr(),
                                   heading_seed=int(heading_seed) & 0xFFFFFFFFFFFFFFFF)
        self._ar_ref = C.byref(self._ar)
        if self._draw is not None and self._draw["c"].seed == self._ar.heading_seed:
            raise ValueError("heading_seed equals the policy draw's seed: an agent's heading and policy would be the same uniform")

    def set_policy_draw(self, pool_bits, distr=None, ensure=None, seed=0x706F6C69637931):
        """Draw every agent's policy anew at each auto-reset, on the device (include/cagpu.h CaPolicyDraw) -- the batched
        form of test_cases.py cadrl_test_case_to_agents: np.random.choice(policies, num_agents, p=policy_distr), then
        `policy_to_ensure` written over one random agent if nobody drew it.  Needs a fixture table.
          pool_bits: per pool entry, bits 6..11 of the flag word (policy_word_bits(): IS_LEARNING, STILL_LEARNING, policy id);
          distr:     the pool's probabilities (normalised as np.random.choice does: cumsum / its last element);
          ensure:    None, or the pool index every episode must hold;
          seed:      the Philox key, != 0 and != the table's heading_seed.
        pool_bits None: off.  While it is on, step(), rollout(), the look-ahead ring and the replay of a rewind launch
        through cagpu_step_draw -- the draw is a pure function of (seed, global env id, episode number), so all of them
        and every shard layout produce the same flag words -- and reset() / reset_from_table() run cagpu_policy_draw for
        the envs they touch.  A host reset zeroes reset_count, so those envs REPLAY the policy sequence of their first
        episodes (as they replay their cases and headings); pass a new seed for a new sequence.  Dynamics bits are never
        drawn.  An env that auto-reset starts without a pipelined plan (queried on its pre-move state: bit-identical)."""
        self.sync()
        if self._la is not None:
            self._la["prep"] = None
        if pool_bits is None:
            self._draw, self._launch = None, self._step_ex
            self._has_ga3c = self._plugins_ga3c
            return
        if self._ar is None:
            raise ValueError("set_policy_draw needs a fixture table (set_fixture_table): policies are drawn at auto-resets")
        bits = np.asarray(pool_bits, np.int64).reshape(-1)
        P = bits.size
        prob = np.asarray(distr, np.float64).reshape(-1)
        if not 1 <= P <= 8 or prob.size != P:
            raise ValueError("the pool needs 1..8 entries and one probability per entry")
        if (prob < 0).any() or not prob.sum() > 0:
            raise ValueError("policy_distr must be non-negative with a positive sum")
        if (bits & ~nat.POLICY_DRAW_BITS).any():
            raise ValueError("pool_bits may only hold bits 6..11 (IS_LEARNING, STILL_LEARNING, the policy id)")
        ens = -1 if ensure is None else int(ensure)
        if not -1 <= ens < P:
            raise ValueError("ensure must be None or a pool index")
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if seed == 0 or seed == self._ar.heading_seed:
            raise ValueError("the policy draw's seed must be != 0 and != the table's heading_seed")
        cdf = prob.cumsum()
        cdf /= cdf[-1]
        t_cdf = torch.as_tensor(cdf, dtype=torch.float64).to(self.device)
        t_bits = torch.as_tensor(bits.astype(np.int32)).to(self.device)
        d = nat.CaPolicyDraw(cdf=t_cdf.data_ptr(), policy_bits=t_bits.data_ptr(), num_policies=P, ensure=ens, seed=seed)
        has_ga3c = bool((((bits >> nat.POLICY_SHIFT) & 0xF) == nat.POL_GA3C_CADRL).any())
        self._draw = dict(c=d, ref=C.byref(d), cdf=t_cdf, bits=t_bits, has_ga3c=has_ga3c, pool=bits.copy())
        draw_ref, step_draw = self._draw["ref"], self.lib.cagpu_step_draw
        self._launch = lambda p, s, o, ext, ar, sx, stream: step_draw(p, s, o, ext, ar, sx, draw_ref, stream)
        # (any slot may become a GA3C-CADRL agent at an auto-reset: the network then runs before every step)
        self._has_ga3c = self._plugins_ga3c or has_ga3c

    def _launch_n(self, p, s, o, ext, ar, sx, stream):
        """a fused launch: _launch, or -- where the CaStepEx names a map or a set -- cagpu_step_ex_maps with the draw"""
        if self._rd is not None:   # (set_rvo_draw: cagpu_step_noise carries maps, tape and draw alike)
            return self._noise(p, s, o, ext, ar, sx, stream)
        if self._map is None:
            return self._launch(p, s, o, ext, ar, sx, stream)
        return self._step_ex_maps(p, s, o, ext, ar, sx, None if self._draw is None else self._draw["ref"], stream)

    def _policy_draw_now(self, mask=None):
        """cagpu_policy_draw: the lottery of the episode every (masked) env is in, on the state and column 0 of `obs`"""
        nat.check(self.lib.cagpu_policy_draw(self._p_ref, self._cs_ref, self._co_ref, self._ar_ref, self._draw["ref"],
                                             None if mask is None else mask.data_ptr(), self._stream()))

    def policy_ids(self):
        """int32 [E, N]: the policy id (CA_POL_*) every agent slot runs in the step last handed out (through sync())"""
        return (self.state["flags"] >> nat.POLICY_SHIFT) & 0xF

    def learning_mask(self, still_learning=False):
        """bool [E, N]: CA_IS_LEARNING (still_learning: CA_STILL_LEARNING) of every agent slot that holds an agent (an
        absent slot of a ragged batch keeps the word of its last agent: False here), through sync()"""
        flags = self.state["flags"]
        return ((flags & (nat.STILL_LEARNING if still_learning else nat.IS_LEARNING)) != 0) & ((flags & nat.ABSENT) == 0)

    # ---------------------------------------------------------------- the C-ABI calls
    def reset(self, cases, headings=None, mask=None):
        self.sync()   # (a ring that ran ahead is rewound even for a reset of EVERY env: env_stats outlive a reset and must not
        #                hold episodes of steps that were never handed out)
        if self.fresh_outputs:   # the tensors the last step() handed out belong to their holder: never written again
            self._new_outputs(keep=mask is not None)
        c = self._dev(cases, torch.float64)
        assert tuple(c.shape) == (self.E, self.N, 6), c.shape
        h = self._dev(headings, torch.float64)
        m = self._dev(mask, torch.uint8)
        nat.check(self.lib.cagpu_reset(C.byref(self.p), C.byref(self._cs), C.byref(self._co), c.data_ptr(),
                                       None if h is None else h.data_ptr(), None if m is None else m.data_ptr(),
                                       self._stream()))
        if self._draw is not None:   # episode 0 of the envs this reset touches needs its lottery too
            self._policy_draw_now(m)
        self._keep = [c, h, m]  # keep alive until the stream has consumed them
        # what was loaded, merged under the mask: episode 0 is the caller's choice and cannot be re-derived (episode_start)
        c7 = torch.cat([c, (torch.full((self.E, self.N), math.nan, dtype=torch.float64, device=self.device)
                            if h is None else h.reshape(self.E, self.N)).unsqueeze(-1)], dim=-1)
        if m is None:
            self._start = c7
        else:
            if self._start is None:
                self._start = torch.full_like(c7, math.nan)
            self._start = torch.where((m != 0).reshape(self.E, 1, 1), c7, self._start)
        if self._cstream is not None:   # the reset envs restart at episode 0: their window holds episodes 1 .. W again
            self._stream_refill()
        if self._log is not None:   # the reset envs count their episodes from 0 again: undrained records of theirs are discarded
            episodes.clear(self._log["head"], self._log["cursor"], m)
        if self._met is not None:   # ... and so are their metrics, the running episode's carry included
            self._met_process()
            episode_metrics.clear(self._met["head"], self._met["cursor"], self._met["carry"], m)
        if self._traj is not None:   # a host-side reset logs no row but ends the episode of the envs it touches (tape "epoch")
            tr = self._traj
            tr["epoch"] = tr["epoch"] + (1 if m is None else (m != 0).to(torch.int32))
            tr["open"] = None
        if self._maps is not None and self._map_rng is not None:
            # a fresh key per explicit reset: the auto-reset draws of the new episodes are not those of the last ones
            self._maps.map_seed = int(self._map_rng.integers(1, 1 << 64, dtype=np.uint64))
            self._map_note_key()
        if self._maps is not None:
            self._map_note_assign(m, reset=True)
        self._apply_sensor_variants()
        return self._obs

    def reset_from_table(self, env_id_offset=None):
        """Initial load: env e <- case (env_id_offset + e) % C of the fixture table."""
        assert self._table is not None
        off = self._ar.env_id_offset if env_id_offset is None else env_id_offset
        idx = (torch.arange(self.E, device=self.device) + off) % self._table.shape[0]
        return self.reset(self._table[idx])

    def set_map(self, static_map=None, rows=160, cols=160, cell=0.1, num_beams=512, num_to_store=3, max_range=6.0,
                range_res=0.1, min_angle=-math.pi / 2, max_angle=math.pi / 2, env_map=None, map_seed=0):
        """Static occupancy grid (Map.py:6-24; bool [rows, cols], True = occupied, or None for an empty map) + the
        LaserScanSensor buffers with the reference's hard-coded parameters (LaserScanSensor.py:28-39).  With a map
        set, step() also tests wall collisions (collision_avoidance_env.py:494-506).

        A MAP SET (include/cagpu.h CaMapSet): `static_map` a bool stack [M, rows, cols] -- every env has its own map,
        the device int32 tensor `env_map` [E] (default: env e on map e % M; an explicit one must hold indices in
        [0, M)), and step(), rollout(), the look-ahead ring and laserscan() hand the kernels the CaMapSet (CaStepEx.set /
        cagpu_laserscan_maps; a fused launch through cagpu_step_ex_maps).  map_seed != 0:
        every auto-reset of an env draws its next map on the device (the reference draws a map per episode,
        collision_avoidance_env.py:274-275, :384-385) with a key that every explicit reset() draws anew from a generator
        seeded by map_seed (`map_seed` property: the key in force); 0: every env keeps its map."""
        self.sync()
        bits = None
        self._map_src = dict(static_map=None if static_map is None else np.array(static_map, dtype=bool), rows=rows, cols=cols,
                             cell=cell, num_beams=num_beams, num_to_store=num_to_store, max_range=max_range,
                             range_res=range_res, min_angle=min_angle, max_angle=max_angle)
        self._maps, self._map_rng, self._env_map = None, None, None
        self._sx.map, self._sx.set = None, None   # (re-pointed below, once the new structs exist)
        self.occ, self.occ_bits, self._occ = None, None, None   # (sized by the map's cell: set_occupancy_grid() again)
        M = 0
        if static_map is not None:
            m = np.asarray(static_map).astype(bool)
            M = m.shape[0] if m.ndim == 3 else 0
            if m.shape != ((M, rows, cols) if M else (rows, cols)) or (m.ndim == 3 and M < 1):
                raise ValueError("static map of shape %s: expected [%d, %d] or a stack [M, %d, %d]" % (m.shape, rows, cols,
                                                                                                        rows, cols))
            wpr = (cols + 31) // 32
            pad = np.zeros(m.shape[:-1] + (wpr * 32,), dtype=np.uint8)
            pad[..., :cols] = m
            words = np.packbits(pad.reshape(m.shape[:-1] + (wpr, 32)), axis=-1, bitorder="little").view(np.uint32)
            bits = torch.from_numpy(words.reshape(-1).view(np.int32).copy()).to(self.device)
        self._map_bits = bits
        self._map = nat.CaMap(static_bits=None if bits is None else bits.data_ptr(), rows=rows, cols=cols, cell=cell,
                              origin_r=(rows * cell / 2.) / cell, origin_c=(cols * cell / 2.) / cell)
        if M:
            self._env_map = torch.zeros((self.E,), dtype=torch.int32, device=self.device)
            self._maps = nat.CaMapSet(map=self._map, env_map=self._env_map.data_ptr(), num_maps=M, map_seed=0)
            self.set_env_map(np.arange(self.E) % M if env_map is None else env_map)
            if int(map_seed):
                self._map_rng = np.random.Generator(np.random.PCG64(int(map_seed) & 0xFFFFFFFFFFFFFFFF))
                self._maps.map_seed = int(map_seed) & 0xFFFFFFFFFFFFFFFF
            # which map an episode ran on (episodes()' `map` column; episodes.map_column has the rule): the index an env was
            # GIVEN (reset / set_env_map) with the episode it was in, and the first episode whose draw used the key in force
            self._map_key_from = torch.zeros((self.E,), dtype=torch.int64, device=self.device)
            self._map_note_assign()
        # a single step takes the set, or else the one map (set_map_seed / set_env_map rewrite the CaMapSet / its tensor in place)
        if M:
            self._sx.set = C.addressof(self._maps)
        else:
            self._sx.map = C.addressof(self._map)
        R = len(np.arange(0, max_range, range_res))
        self.scan_hist = torch.full((self.E, self.N, num_to_store, num_beams), 255, dtype=torch.uint8,
                                    device=self.device)
        self.scan = torch.zeros((self.E, self.N, num_to_store, num_beams), dtype=torch.float32, device=self.device)
        self._scan = nat.CaScan(hist=self.scan_hist.data_ptr(), out=self.scan.data_ptr(), num_beams=num_beams,
                                num_to_store=num_to_store, num_ranges=R, min_angle=min_angle, max_angle=max_angle,
                                range_res=range_res, max_range=max_range)

    @property
    def num_maps(self):
        """maps of the attached map set (0: none -- one map, or none, for every env)"""
        return 0 if self._maps is None else int(self._maps.num_maps)

    @property
    def map_seed(self):
        """the key of the map set's auto-reset draws in force (CaMapSet.map_seed; 0: an auto-reset keeps the env's map)"""
        return 0 if self._maps is None else int(self._maps.map_seed)

    def set_map_seed(self, key):
        """replace the key of the map set's auto-reset draws (0: off); the next explicit reset() draws a new one only
        where set_map was given a map_seed"""
        assert self._maps is not None, "set_map() with a stack of maps first"
        self.sync()   # (a ring that ran ahead drew with the old key)
        self._maps.map_seed = int(key) & 0xFFFFFFFFFFFFFFFF
        self._map_note_key()

    def _map_note_key(self):
        """the key changed: the draws of reset counts above the current ones use it"""
        self._map_key_from = self._state["reset_count"].to(torch.int64) + 1

    def _map_note_assign(self, mask=None, reset=False):
        """the envs of `mask` (None: all) were given their map by the host, in the episode they are in now; reset: by an
        explicit reset, which zeroes their reset counts -- every draw of theirs from now on uses the key in force"""
        rc = self._state["reset_count"].to(torch.int64)
        m = torch.ones_like(rc, dtype=torch.bool) if mask is None else mask != 0
        if mask is None:
            self._map_ep0, self._map_val0 = rc, self._env_map.clone()
        else:
            self._map_ep0 = torch.where(m, rc, self._map_ep0)
            self._map_val0 = torch.where(m, self._env_map, self._map_val0)
        if reset:
            self._map_key_from = torch.where(m, torch.zeros_like(rc), self._map_key_from)

    def set_env_map(self, env_map):
        """the map of every env of the map set: ints broadcastable to [E], each in [0, M) (checked here: the device
        only flags an index outside, bit 2 of the fault word, and gives that env an empty map)"""
        assert self._maps is not None, "set_map() with a stack of maps first"
        self.sync()
        idx = np.array(np.broadcast_to(np.asarray(env_map), (self.E,)))
        if not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("env_map must hold integers, got %s" % idx.dtype)
        M = int(self._maps.num_maps)
        if idx.size and (idx.min() < 0 or idx.max() >= M):
            raise ValueError("env_map holds indices outside [0, %d): %s" % (M, sorted(set(idx[(idx < 0) | (idx >= M)].tolist()))[:8]))
        self._env_map.copy_(torch.from_numpy(idx.astype(np.int32)))   # (in place: the CaMapSet points at this tensor)
        self._map_note_assign()

    def laserscan(self):
        """'laserscan' observation [E,N,num_to_store,num_beams] of the current state (call after reset / step)."""
        assert self._map is not None, "set_map() first"
        self.sync()
        if self._maps is not None:
            nat.check(self.lib.cagpu_laserscan_maps(C.byref(self.p), C.byref(self._cs), C.byref(self._maps),
                                                    C.byref(self._scan), self._stream()))
        else:
            nat.check(self.lib.cagpu_laserscan(C.byref(self.p), C.byref(self._cs), C.byref(self._map),
                                               C.byref(self._scan), self._stream()))
        return self.scan

    def set_occupancy_grid(self, x_width=5., y_width=5., packed=False):
        """Buffers of the OccupancyGridSensor (reference sensors/OccupancyGridSensor.py): every agent's window of
        y_width x x_width metres around it, H = int(y_width / cell) rows x W = int(x_width / cell) columns of the map
        given to set_map() (call that first; calling it again drops these buffers).  `self.occ`: bool [E, N, H, W];
        packed=True: `self.occ_bits` instead, int32 [E, N, H, (W + 31) // 32], cell b of a row = bit b & 31 of word b >> 5
        (1/6 of the bytes at W = 50); packed="both": both."""
        assert self._map is not None, "set_map() first"
        self.sync()
        cell = float(self._map.cell)
        H, W = int(y_width / cell), int(x_width / cell)
        if not (1 <= H <= 256 and 1 <= W <= 256):
            raise ValueError("occupancy grid of %d x %d cells: height and width must be in [1, 256]" % (H, W))
        self.occ, self.occ_bits = None, None
        if packed != True:  # noqa: E712 -- False or "both"
            self._occ_cells = torch.zeros((self.E, self.N, H, W), dtype=torch.uint8, device=self.device)
            self.occ = self._occ_cells.view(torch.bool)   # (0 / 1 bytes: no conversion kernel)
        if packed:
            self.occ_bits = torch.zeros((self.E, self.N, H, (W + 31) // 32), dtype=torch.int32, device=self.device)
        self._occ = nat.CaOccGrid(cells=None if self.occ is None else self._occ_cells.data_ptr(),
                                  bits=None if self.occ_bits is None else self.occ_bits.data_ptr(), height=H, width=W,
                                  x_width=float(x_width), y_width=float(y_width))

    def occupancy_grid(self):
        """'occupancy_grid' observation of the current state (call after reset / step): `self.occ` (bool [E,N,H,W]), or
        `self.occ_bits` where set_occupancy_grid(packed=True) asked for the packed form only.  A pure function of the
        state and the env's current map (cagpu_occupancy_grid / _maps, csrc/cagpu_occ.inc)."""
        assert self._occ is not None, "set_occupancy_grid() first"
        self.sync()
        if self._maps is not None:
            nat.check(self.lib.cagpu_occupancy_grid_maps(C.byref(self.p), C.byref(self._cs), C.byref(self._maps),
                                                         C.byref(self._occ), self._stream()))
        else:
            nat.check(self.lib.cagpu_occupancy_grid(C.byref(self.p), C.byref(self._cs), C.byref(self._map),
                                                    C.byref(self._occ), self._stream()))
        return self.occ if self.occ is not None else self.occ_bits

    def _new_outputs(self, keep=False):
        """keep: the new tensors start as copies of the current ones (a masked reset rewrites only some envs' rows)"""
        co = self._co
        new = (lambda t: t.clone()) if keep else torch.empty_like
        self._obs = new(self._obs); co.obs = self._obs.data_ptr()
        self._rewards = new(self._rewards); co.rewards = self._rewards.data_ptr()
        self._done = new(self._done); co.done = self._done.data_ptr()
        self._game_over = new(self._game_over); co.game_over = self._game_over.data_ptr()
        if self._fin_on:   # (the final record handed out with those outputs belongs to their holder as well)
            self._fin_obs, self._fin_flags = new(self._fin_obs), new(self._fin_flags)
            self._cf.obs, self._cf.flags = self._fin_obs.data_ptr(), self._fin_flags.data_ptr()

    def step(self, ext_actions=None, ext_state=None):
        """ext_state: float64 [E, N, 5] = px, py, vx, vy, heading for agents with ExternalDynamics whose motion of THIS step
        was integrated outside (a user Dynamics subclass on the host; NaN rows: none) -- applied by the kernel at the move
        (CaState.ext_state); None: nobody."""
        if self._la is not None:
            self.sync()
        if self._traj_on:     # (first: a tape that is full raises before anything of this step has happened)
            self._traj_slot()
        if self._rvo is not None:
            self._rvo_draw()
        if ext_state is not None or self._cs.ext_state:
            self._ext_state = self._dev(ext_state, torch.float64)
            if self._ext_state is not None:
                assert tuple(self._ext_state.shape) == (self.E, self.N, 5), self._ext_state.shape
            self._cs.ext_state = None if self._ext_state is None else self._ext_state.data_ptr()
        # env.step(None) with built-in policies only (env_utils.py:50): the per-step host path is the one ctypes call below
        # with references made once -- at ~20 us per launch the interpreter is otherwise on the critical path
        fast = ext_actions is None and not self._has_ga3c
        e = ext = None
        if not fast:
            e = self._dev(ext_actions, torch.float64)
            if e is not None:
                assert tuple(e.shape) == (self.E, self.N, 2), e.shape
            if self._has_ga3c:  # policy query on the pre-step observation (collision_avoidance_env.py:319-323)
                if e is not None:  # the caller's external actions travel in the same buffer; never write into theirs
                    if self._ga3c_ext is None:
                        self._ga3c_ext = torch.zeros((self.E, self.N, 2), dtype=torch.float64, device=self.device)
                    self._ga3c_ext.copy_(e)
                e = self.ga3c(None if e is None else self._ga3c_ext)
            ext = None if e is None else e.data_ptr()
        if self.fresh_outputs:
            self._new_outputs()
        if self._cstream is not None:   # a case stream: an env ends at most one episode per step
            if self._cstream["since"] >= self._cstream["every"]:
                self._stream_refill()
            self._cstream["since"] += 1
        rc = (self._launch if self._rd is None else self._noise)(self._p_ref, self._cs_ref, self._co_ref, ext, self._ar_ref,
                                                                  self._sx_ref, self._stream_handle())
        if rc != 0:
            nat.check(rc)
        if fast:
            self._steps_since_probe += 1
            if self._steps_since_probe >= 256:
                self._steps_since_probe = 0
                self._fault_probe()
        else:
            self._keep = [e]
        if self._met is not None:
            self._met_process()
        if self._variants:
            self._apply_sensor_variants()
        return self._obs, self._rewards, self._game_over

    def _action_tape(self, ext_actions, n):
        """rollout()'s external actions -> (float64 device tensor or None, doubles from one step's slot to the next): 0 for
        [E, N, 2], ONE slot held for all steps; E * N * 2 for an action tape [T, E, N, 2], T >= n, slot t for step t.
        Converted once (dtype, device, layout), like every array that goes to the library."""
        if ext_actions is None:
            return None, 0
        shape = tuple(getattr(ext_actions, "shape", None) or np.shape(ext_actions))
        held, E, N = (self.E, self.N, 2), self.E, self.N
        if shape != held and not (len(shape) == 4 and shape[1:] == held and shape[0] >= n):
            raise ValueError("rollout: ext_actions must be [E, N, 2] = %r (one action held for all steps) or an action tape "
                             "[T, E, N, 2] with T >= n_steps = %d, got %r" % (held, n, shape))
        return self._dev(ext_actions, torch.float64), (0 if len(shape) == 3 else E * N * 2)

    def _map_slots_check(self, n, keep_steps):
        """rollout(map_sensors=True): everything that can be refused is refused here, before anything is launched"""
        if not keep_steps:
            raise nat.CagpuError("rollout(map_sensors=True) keeps every step's sensors: it needs keep_steps=True")
        if self._map is None:
            raise nat.CagpuError("rollout(map_sensors=True): set_map() first")
        if self._cstream is not None:
            raise nat.CagpuError("rollout(map_sensors=True): a case stream (set_case_stream) is not supported -- its window of "
                                 "cases changes under the launch, so the start poses of the episodes that begin inside it "
                                 "cannot be restated afterwards; nothing was launched")
        if self.N > 256:
            raise nat.CagpuError("rollout(map_sensors=True): the laser scan supports up to 256 agents per env")

    def _map_slots_budget(self, n, own_tape):
        """the bytes the slots of this launch add -- the pose ring, the index ring and, where recording is off, the transient
        tape -- against the tape's budget (record_trajectories' max_bytes; 1 GiB where it was never called)"""
        from . import map_slots
        tr = self._traj
        budget, used = (1 << 30, 0) if tr is None else (tr["max_bytes"], tr["bytes"])
        per = map_slots.slot_bytes(self.E, self.N, int(self._scan.num_beams), self._maps is not None)
        need = n * (per + self.traj_step_bytes)   # (a recorded chunk is committed to the same budget by the launch itself)
        if used + need > budget:
            raise nat.CagpuError("rollout(map_sensors=True): %d steps need %d bytes (%d per step for the pose and index rings, "
                                 "%d for the tape%s) and %d of max_bytes = %d are in use -- fewer steps, clear_trajectories() "
                                 "or record_trajectories(max_bytes=...); no step was taken"
                                 % (n, need, per, self.traj_step_bytes, " (transient)" if own_tape else "", used, budget))

    def _map_slots_start(self):
        """the few arrays of the state a launch is about to overwrite that the pose ring starts from (copies on the stream)"""
        start = {f: self._state[f].clone() for f in ("pos_x", "pos_y", "heading", "radius", "step_num", "reset_count")}
        if self._maps is not None:
            start["env_map"] = self._env_map.clone()
        return start

    def _map_slots_finish(self, n, start, ct, game_over, expand_last=True):
        """behind a fused launch: the pose ring from the launch's tape, the slot march, and (expand_last) the last slot's
        history into `scan_hist` / `scan` -- three launches, whatever n is"""
        from . import map_slots
        E, N, dev, lib = self.E, self.N, self.device, self.lib
        poses = {f: torch.empty((n, E, N), dtype=torch.int32 if f == "step_num" else torch.float64, device=dev)
                 for f in map_slots.POSE_FIELDS}
        if self._maps is not None:
            poses["env_map"] = torch.empty((n, E), dtype=torch.int32, device=dev)
        pr = nat.CaPoseRing(**{f: t.data_ptr() for f, t in poses.items()})
        cs0 = nat.CaState(**{f: start[f].data_ptr() for f in map_slots.POSE_FIELDS + ("reset_count",)})
        sets = None if self._maps is None else C.byref(self._maps)
        nat.check(lib.cagpu_tape_poses(self._p_ref, C.byref(cs0), None if sets is None else start["env_map"].data_ptr(),
                                       C.byref(ct), game_over.data_ptr(), n, self._ar_ref, sets, C.byref(pr), self._stream()))
        idx = torch.empty((n, E, N, int(self._scan.num_beams)), dtype=torch.uint8, device=dev)
        nat.check(lib.cagpu_laserscan_slots(self._p_ref, C.byref(pr), n, None if sets is not None else C.byref(self._map), sets,
                                            C.byref(self._scan), idx.data_ptr(), self._stream()))
        carried = self.scan_hist.clone()
        kept = map_slots.KeptMapSensors(self, n, poses, idx=idx, carried=carried)
        if not expand_last:    # (the look-ahead ring expands the slot it hands out: step_lookahead)
            return kept
        # the sim's own sensor state becomes the last slot's: what n single laserscan() calls would have left
        nat.check(lib.cagpu_laserscan_history(self._p_ref, C.byref(self._scan), idx.data_ptr(), poses["step_num"].data_ptr(), n,
                                              n - 1, 1, self.scan_hist.data_ptr(), self.scan.data_ptr(), self._stream()))
        if self._occ is not None:
            self.occupancy_grid()      # (stateless: the final state is the last slot's)
        return kept

    def rollout(self, n_steps, ext_actions=None, keep_steps=False, map_sensors=False):
        """n_steps steps in ONE launch (cagpu_step_ex's n_steps) -> the last step's (obs, rewards, game_over).
        ext_actions: [E, N, 2], held for all steps, or an ACTION TAPE [T, E, N, 2] (T >= n_steps): step t of the call plays
        slot t (cagpu_step_tape) -- the step of the CALL, not of the episode: an env that auto-resets in step t plays slot
        t + 1 as the first action of its next episode.  Entries of agents that are not queried (internal policies, done
        agents, absent slots) are never read.  Where the batch needs work between two steps (a GA3C-CADRL network, stochastic
        RVO draws of set_rvo_stochastic -- not those of set_rvo_draw, which the step kernels make themselves) the steps are
        single launches and step t is handed slot t: the same results, one launch per step.
        keep_steps: every step keeps its outputs (a ring launch, CaStepEx.ring, into newly allocated tensors) and the call
        returns (obs [n, E, N, W], rewards [n, E, N], done [n, E, N], game_over [n, E]); `obs` / `rewards` / `done` /
        `game_over` afterwards show the last slot.  With keep_final() on every slot has its own final block: `kept_final` =
        (final_obs [n, E, N, W], final_flags [n, E, N]), rows valid where the slot's game_over is set (None after every other
        rollout); `final_obs` / `final_flags` show the last slot's.  The trajectory tape, the episode log, maps, the policy
        draw, the case stream and the metrics ride on either form as on rollout(n).
        map_sensors (with keep_steps, after set_map): the laser scan and the occupancy windows of EVERY step as well --
        `kept_map_sensors` (map_slots.KeptMapSensors: laserscan(t), laserscan_index(t), occupancy_grid(t), poses), from the
        launch's trajectory tape by kernels of their own (the tape is switched on for this launch
        alone where recording is off); `scan`, `scan_hist` and the occupancy tensors afterwards show the last slot, exactly
        as after n x (step(), laserscan(), occupancy_grid()).  Off by default: no call or kernel changes without it."""
        self.sync()
        n = int(n_steps)
        self.kept_map_sensors = None
        if map_sensors:
            self._map_slots_check(n, keep_steps)
        # (CaState.ext_state belongs to the ONE step() call that was given it: never re-applied by the steps of a rollout)
        self._cs.ext_state, self._ext_state = None, None
        e, stride = self._action_tape(ext_actions, n)
        self.kept_final = None
        if self._has_ga3c or self._rvo is not None:  # the network / the stochastic RVO draws run between steps
            kept, sens = [], []
            for t in range(n):
                self.step(e if stride == 0 else e[t])
                if map_sensors:   # the existing sensors, per step
                    self.laserscan()
                    occ = self.occupancy_grid().clone() if self._occ is not None else None
                    sens.append((self.scan.clone(), self.scan_hist.clone(), occ) +
                                tuple(self._state[f].clone() for f in ("pos_x", "pos_y", "heading", "radius", "step_num")) +
                                ((self._env_map.clone(),) if self._maps is not None else ()))
                if keep_steps:   # (torch.stack copies at the end: until then a step that writes in place must not reach them)
                    own = (lambda x: x) if self.fresh_outputs else (lambda x: x.clone())
                    kept.append(tuple(own(x) for x in (self._obs, self._rewards, self._done, self._game_over) +
                                      ((self._fin_obs, self._fin_flags) if self._fin_on else ())))
            if keep_steps:
                cols = [torch.stack(c) for c in zip(*kept)]
                if self._fin_on:
                    self.kept_final = (cols[4], cols[5])
                if map_sensors:
                    from . import map_slots
                    sc = [torch.stack(c) if c[0] is not None else None for c in zip(*sens)]
                    poses = dict(zip(map_slots.POSE_FIELDS + ("env_map",), sc[3:]))
                    self.kept_map_sensors = map_slots.KeptMapSensors(self, n, poses, dense=dict(scan=sc[0], hist=sc[1], occ=sc[2]))
                return cols[0], cols[1], cols[2], cols[3]
            return self._obs, self._rewards, self._game_over
        if self.fresh_outputs and not keep_steps:
            self._new_outputs()
        if self._cstream is not None:
            self._stream_refill()
        # the n steps' CaStepEx: the map or set of a single step, the tape's own chunk, the single-step final block -- it ends up holding every
        # env's most recent terminal record of the launch -- and the log, every ending in its own slot
        if map_sensors:
            self._map_slots_budget(n, not self._traj_on)
        chunk, ct = self._traj_chunk(n) if self._traj_on else (None, None)
        if map_sensors:
            if ct is None:   # recording is off: a tape for this launch alone, released with the call
                own_tape = self._traj_alloc(n)
                ct = nat.CaTraj(rows=own_tape[0].data_ptr(), episode=own_tape[1].data_ptr())
            start = self._map_slots_start()
        co_ref, fin = self._co_ref, self._sx.fin
        if keep_steps:   # a ring launch without a rewind point: the look-ahead ring's layout, every slot its final block
            ring, fin_ring, cf, co, _ = self._ring_layout(n)
            co_ref, fin = C.byref(co), None if cf is None else C.addressof(cf)
        sx = nat.CaStepEx(n_steps=n, ring=1 if keep_steps else 0, map=self._sx.map, set=self._sx.set,
                          traj=None if ct is None else C.addressof(ct), fin=fin, log=self._sx.log)
        if stride and self._rd is not None:
            nat.check(self._noise(self._p_ref, self._cs_ref, co_ref, e.data_ptr(), self._ar_ref, C.byref(sx),
                                  self._stream_handle(), stride))
        elif stride:
            tape = nat.CaActionTape(actions=e.data_ptr(), step_stride=stride)
            nat.check(self.lib.cagpu_step_tape(self._p_ref, self._cs_ref, co_ref, C.byref(tape), self._ar_ref, C.byref(sx),
                                               None if self._draw is None else self._draw["ref"], self._stream_handle()))
        else:
            nat.check(self._launch_n(self._p_ref, self._cs_ref, co_ref, None if e is None else e.data_ptr(), self._ar_ref,
                                     C.byref(sx), self._stream_handle()))
        if chunk is not None:
            self._traj_commit(chunk)
            if self._met is not None:
                self._met_process()
        self._keep = [e]   # (the tape stays alive until the next launch is queued behind this one)
        if map_sensors:
            self.kept_map_sensors = self._map_slots_finish(n, start, ct, ring[3])
        if keep_steps:
            # the last slot becomes the simulator's current outputs: the caller's own where the next step writes new tensors
            # anyway (fresh_outputs), a copy where it writes in place
            own = (lambda x: x) if self.fresh_outputs else (lambda x: x.clone())
            self._obs, self._rewards, self._done, self._game_over = (own(x[n - 1]) for x in ring)
            self._co.obs, self._co.rewards, self._co.done, self._co.game_over = (
                self._obs.data_ptr(), self._rewards.data_ptr(), self._done.data_ptr(), self._game_over.data_ptr())
            if fin_ring is not None:
                self.kept_final = fin_ring
                self._fin_obs, self._fin_flags = own(fin_ring[0][n - 1]), own(fin_ring[1][n - 1])
                self._cf.obs, self._cf.flags = self._fin_obs.data_ptr(), self._fin_flags.data_ptr()
            self._apply_sensor_variants()
            return ring
        self._apply_sensor_variants()
        return self._obs, self._rewards, self._game_over

    def try_plan(self):
        """cagpu_plan: the policy query of the next step ahead of time (fills state['next_action'], sets PLAN_VALID).
        Returns False where the pipelined kernel has no instantiation for this batch (the step kernels then query the
        policy at the start of the step, as without next_action)."""
        self.sync()
        rc = self.lib.cagpu_plan(C.byref(self.p), C.byref(self._cs), self._stream())
        if rc == nat.CA_EUNSUPPORTED:
            return False
        nat.check(rc)
        return True

    def observe(self):
        self.sync()
        if self.fresh_outputs:   # (cagpu_observe rewrites obs only: the other outputs carry over)
            self._new_outputs(keep=True)
        nat.check(self.lib.cagpu_observe(C.byref(self.p), C.byref(self._cs), C.byref(self._co), self._stream()))
        self._apply_sensor_variants()
        return self._obs

    # ---------------------------------------------------------------- the look-ahead ring behind env.step(None)
    def lookahead_ok(self):
        """can step_lookahead() run this batch?  Every policy has to be answered inside the step kernel and nothing may
        happen BETWEEN two steps on the host or in another kernel: no GA3C-CADRL network, no per-step stochastic RVO
        draws (set_rvo_stochastic; set_rvo_draw draws inside the step kernels and is fine), no per-agent sensor variants
        (extra cagpu_observe launches).  A static map or a map set is carried by the
        ring's launches (walls and map draws are those of single steps); laserscan() / occupancy_grid() go through sync()
        and describe the step last handed out."""
        return not (self._has_ga3c or self._rvo is not None or self._variants)

    def enable_lookahead(self, k, fresh=True, adaptive=False, start=None, map_sensors=False):
        """Serve step(None) from a ring of `k` steps computed ahead of time in ONE launch (CaStepEx.ring): with every
        policy internal a step needs nothing from the host (env_utils.py:45-52 passes None until the episode is over),
        so step_lookahead() hands out slot t of the ring and launches the next k steps when it runs dry -- the fused
        n-step kernel never waits for the slowest workgroup of a step (7.7 instead of 14.9 us per step at 4096 x 10).
        Results are those of k single launches, bit for bit.  Whatever needs the state of the step last handed out --
        reading `state`, a reset, an external action, a parameter change, the episode statistics -- goes through sync(),
        which rewinds (restore the snapshot taken before the launch, re-run the steps already handed out).  `env_map` of a
        map set is read through sync() as well: a ring that has run ahead has drawn the maps of episodes not handed out yet.
        fresh: every refill writes into a NEWLY allocated ring (what step_lookahead returned stays valid and belongs to
        the caller); False: one persistent ring, a slot is overwritten k steps later.  k = 0: off.
        adaptive: k is the LONGEST ring.  A rewind throws the rest of a ring away, so a caller who looks at the state (or
        acts) every m steps should not pay for k: the first ring is `start` steps long (default min(k, 8): a caller who
        reads the state after its first step has wasted at most 7), after a rewind at slot t the next ring is t steps
        long (at least 1 = one launch per step), and a ring consumed to its end doubles the next one up to k -- after a
        rewind only once TWO rings in a row have been used up, so that a caller who looks at the state after every step
        stays at one launch per step instead of alternating between rings of 1 and 2.
        What step_lookahead() returns are VIEWS of the ring's tensors (slot t of `[n, E, N, W]` ...): with fresh=True they
        are never written again and stay valid for as long as the caller holds them, but holding ONE of them keeps the
        whole ring allocated (n slots); clone a slot that is kept long-term.
        map_sensors (after set_map): every refill also keeps the pose ring and the laser's index ring of its slots
        (rollout()'s map_sensors: DESIGN.md section 3m), and every step_lookahead() expands the slot it hands out into
        `scan` / `scan_hist` (one launch of the history kernel) and the occupancy tensors (one of the occupancy kernel),
        without a synchronisation: the sim's sensor state is always that of the step last handed out, with the history
        counting steps, and a rewind needs nothing extra.  Read `scan`, `scan_hist`, `occ` / `occ_bits` directly then:
        laserscan() would measure the same state a second time."""
        self.sync()
        k = int(k)
        if k <= 0:
            self._la = None
            return
        if map_sensors:
            self._map_slots_check(k, True)
        cur = k if not adaptive else max(1, min(k, 8 if start is None else int(start)))
        self._la = dict(n=k, cur=cur, len=0, t=0, slots=None, fresh=bool(fresh), adaptive=bool(adaptive), ring=None,
                        snap=torch.empty_like(self._slab), fills=0, rewinds=0, in_kernel={}, prep=None, co_live=None,
                        streak=2, ms=bool(map_sensors), ms_kept=None)

    def _la_fill(self):
        la = self._la
        if not self.lookahead_ok():
            raise nat.CagpuError("step_lookahead: this batch needs work between two steps (GA3C-CADRL network, stochastic RVO "
                                 "draws or sensor variants) -- use step()")
        if self._cs.ext_state:   # (CaState.ext_state belongs to the ONE step() call that was given it: see rollout())
            self._cs.ext_state, self._ext_state = None, None
        if self._cstream is not None:   # (a ring is launched only when the previous one is used up or sync() has rewound)
            self._stream_refill()
        if self._met is not None:       # (the last ring's slots were all handed out: measured, and released, before the
            self._met_process()         #  tape's budget is asked for this one)
        rec = self._traj_on      # (one look per fill: with recording off a fill does what it did before the tape existed)
        if rec:
            fit = self._traj_fit()   # (a full tape raises here, before anything changes)
        if la["adaptive"] and la["slots"] is not None and la["t"] >= la["len"]:   # the last ring was used up: a longer one --
            la["streak"] += 1                                                     # after a rewind, only the second in a row
            if la["streak"] >= 2:
                la["cur"] = min(la["n"], 2 * la["cur"])
        k = la["cur"]
        if rec and fit < k:
            k = fit                  # (a ring is shortened to what the tape's budget still holds)
        ms = la["ms"]
        if ms:                       # (raises before anything changes: a case stream attached since, the byte budget)
            self._map_slots_check(k, True)
            self._map_slots_budget(k, not rec)
        # Everything a launch needs that does not depend on the moment of the call -- the ring's tensors, the CaOut that names
        # them, the rewind mode, the slot views handed out later -- was prepared behind the PREVIOUS launch (_la_prepare): a
        # caller who synchronises around K steps (bench.py's timed block) has the device idle until this launch is submitted
        prep = la["prep"]
        if prep is None or prep["k"] != k:     # (set_fixture_table / update_params drop a prepared launch)
            prep = self._la_prepare(k)
        la["prep"] = None
        la["ring"] = prep["ring"]
        if not prep["in_kernel"]:
            la["snap"].copy_(self._slab)
        if self._maps is not None:   # env_map is not in the slab: the rewind point of a set keeps its own copy (E int32)
            la["map_snap"] = self._env_map.clone()
        la["fin_ring"] = prep["fin_ring"]
        # the launch's CaStepEx was prepared with the ring (final blocks, the episode log -- its records land in the envs' own
        # rings, not in the output ring); the ring's own chunk of the tape is taken now: slot t of the launch records step t
        chunk = None
        if rec:
            chunk, ct = self._traj_chunk(k, prep["traj"])
            prep["sx"].traj = C.addressof(ct)
        if ms:
            if not rec:              # recording is off: a tape for this launch alone
                own_tape = self._traj_alloc(k)
                ct = nat.CaTraj(rows=own_tape[0].data_ptr(), episode=own_tape[1].data_ptr())
                prep["sx"].traj = C.addressof(ct)
            start = self._map_slots_start()
        rc = self._launch_n(self._p_ref, self._cs_ref, prep["co_ref"], None, prep["ar_ref"], prep["sx_ref"], self._stream_handle())
        if rc != 0:
            nat.check(rc)
        if ms:
            la["ms_kept"] = self._map_slots_finish(k, start, ct, prep["ring"][3], expand_last=False)
        if chunk is not None:
            la["traj"] = self._traj_commit(chunk)
        la["slots"] = prep["slots"]
        la["co_live"] = prep["co"]      # (keeps the ctypes struct the launch was given alive)
        la["t"], la["len"] = 0, k
        la["fills"] += 1
        if la["fills"] % self.PROBE_EVERY == 1:   # (every refill costs a 20-step block 2.6 us: a second queue for the caller's
            self._fault_probe()                   #  synchronisation to wait on; r06_kernel_geometry.md section 7)
        if la["fresh"]:                 # the next ring (tensors, views, arguments), allocated behind this launch
            la["prep"] = self._la_prepare(min(la["n"], 2 * k) if (la["adaptive"] and la["streak"] >= 1) else k)

    def _la_key(self, k):
        """what decides which kernel a ring call of k steps runs (and with it whether the kernel takes the rewind snapshot)"""
        ar = self._ar
        return (k, self.p.sort_mode, ar is not None and bool(ar.reset_obs), bool(self._cs.next_action),
                0 if ar is None else int(ar.heading_seed), 0 if ar is None else C.addressof(ar),
                int(self._sx.map or 0), int(self._sx.set or 0))

    def _ring_layout(self, k, ring=None, fin_ring=None):
        """What a ring launch of k steps (CaStepEx.ring) writes into, stated once for the look-ahead ring and for
        rollout(keep_steps=True) -> (ring, fin_ring, cf, co, slots): the four output tensors [k, ...] (`ring` / `fin_ring`
        given: those are used again), the final blocks and their CaFinal where keep_final() is on (None, None otherwise),
        the CaOut that names slot 0 and the per-slot views handed out later."""
        E, N, dev = self.E, self.N, self.device
        if ring is None:
            ring = (torch.empty((k, E, N, self.W), dtype=torch.float32, device=dev), torch.empty((k, E, N), dtype=torch.float32, device=dev),
                    torch.empty((k, E, N), dtype=torch.uint8, device=dev), torch.empty((k, E), dtype=torch.uint8, device=dev))
        obs, rew, done, over = ring
        cf = None
        if self._fin_on:      # every slot carries its final block (rows valid where the slot's game_over is set)
            if fin_ring is None:
                fin_ring = (torch.empty((k, E, N, self.W), dtype=torch.float32, device=dev),
                            torch.empty((k, E, N), dtype=torch.int32, device=dev))
            cf = nat.CaFinal(obs=fin_ring[0].data_ptr(), flags=fin_ring[1].data_ptr())
        else:
            fin_ring = None
        co = nat.CaOut.from_buffer_copy(self._co)   # (the ring's own CaOut: the workspace of self._co, no actions / orca_vel record)
        co.actions, co.orca_vel = None, None
        co.obs, co.rewards, co.done, co.game_over = obs.data_ptr(), rew.data_ptr(), done.data_ptr(), over.data_ptr()
        # (the kernels write 0 / 1 bytes: reinterpreted as bool without a conversion kernel)
        slots = list(zip(obs.unbind(0), rew.unbind(0), done.view(torch.bool).unbind(0), over.view(torch.bool).unbind(0)))
        return ring, fin_ring, cf, co, slots

    def _la_prepare(self, k):
        la = self._la
        # (fresh=False: ONE persistent ring, a slot is overwritten k steps later)
        again = lambda r: r if (not la["fresh"] and r is not None and r[0].shape[0] == k) else None
        ring, fin_ring, cf, co, slots = self._ring_layout(k, again(la["ring"]), again(la.get("fin_ring")))
        ar_ref = self._ar_ref
        # the rewind point = the state BEFORE the k steps: stored by the pipelined n-step kernel itself as it loads its
        # tiles (snapshot_delta: the snapshot slab has the state slab's layout); by one device copy in front of the launch
        # for the other kernels
        key = self._la_key(k)
        in_kernel = la["in_kernel"].get(key)   # (the cache is dropped by set_fixture_table / update_params)
        if in_kernel is None:
            rc = self.lib.cagpu_ring_snapshots(self._p_ref, self._cs_ref, C.byref(co), ar_ref, k)
            if rc < 0:
                nat.check(rc)
            # (a batch with set_rvo_draw never runs the pipelined kernel: the rewind point is the device copy)
            in_kernel = la["in_kernel"][key] = rc == 1 and self._rd is None
        sx = nat.CaStepEx(n_steps=k, ring=1, snapshot_delta=(la["snap"].data_ptr() - self._slab.data_ptr()) if in_kernel else 0,
                          map=self._sx.map, set=self._sx.set, fin=None if cf is None else C.addressof(cf), log=self._sx.log)
        return dict(k=k, key=key, ring=ring, co=co, co_ref=C.byref(co), ar_ref=ar_ref, in_kernel=in_kernel, slots=slots,
                    fin_ring=fin_ring, cf=cf, sx=sx, sx_ref=C.byref(sx),   # (cf: kept alive for sx.fin)
                    traj=self._traj_alloc(k) if self._traj_on else None)   # (always its own tensors, fresh ring or not)

    def step_lookahead(self):
        """one step(None) served from the look-ahead ring -> (obs [E,N,W], rewards [E,N], done [E,N] bool, game_over [E] bool)"""
        la = self._la
        t = la["t"]
        if la["slots"] is None or t >= la["len"]:
            self._la_fill()
            t = 0
        la["t"] = t + 1
        if la["ms"]:
            la["ms_kept"].expand_into_sim(t)
        return la["slots"][t]

    def lookahead_final(self):
        """the final record of the slot step_lookahead() handed out last -> (final_obs [E,N,W], final_flags [E,N] int32),
        views of the ring like the slot's outputs, WITHOUT a rewind (the `final_obs` / `final_flags` properties go through
        sync() like `obs`); keep_final() must be on"""
        la = self._la
        if la is None or la["slots"] is None or la["t"] < 1 or la.get("fin_ring") is None:
            return self.final_obs, self.final_flags
        fo, ff = la["fin_ring"]
        return fo[la["t"] - 1], ff[la["t"] - 1]

    def sync(self):
        """Make `state`, `obs`, `rewards`, `done`, `game_over` those of the step LAST HANDED OUT by step_lookahead (a no-op
        without a ring, or when the ring has been consumed to its end): restore the snapshot taken before the ring's launch
        and re-run the t steps already handed out -- the same kernels on the same bits.  The ring is dropped; the next
        step_lookahead() launches a new one."""
        la = self._la
        if la is None or la["slots"] is None:
            return
        t, k = la["t"], la["len"]
        obs, rew, done, over = la["ring"]
        la["slots"] = None
        if self._cstream is not None:   # up to k steps since the ring's refill: the next single step refills first
            self._cstream["since"] = self._cstream["every"]
        if t < k:
            la["rewinds"] += 1
            if la["adaptive"]:     # the caller came back after t steps: that is how far the next ring looks ahead
                la["cur"] = max(1, t)
                la["streak"] = 0
        fin_ring = la.get("fin_ring")
        if not la["fresh"]:
            la["ring"] = None      # (the current outputs below live in it: the next fill must not overwrite them)
            la["fin_ring"] = None
        ch = la.pop("traj", None)
        if ch is not None and t < k:   # the tape keeps the t slots handed out; the replay below records nothing
            self._traj["bytes"] -= (k - t) * self.traj_step_bytes
            ch["n"] = t
        if t > 0:                  # the outputs of the last step handed out are the simulator's current outputs
            own = (lambda x: x.clone()) if la["fresh"] else (lambda x: x)   # (a fresh ring's slots belong to the caller)
            self._obs, self._rewards, self._done, self._game_over = own(obs[t - 1]), own(rew[t - 1]), own(done[t - 1]), own(over[t - 1])
            co = self._co
            co.obs, co.rewards, co.done, co.game_over = (self._obs.data_ptr(), self._rewards.data_ptr(), self._done.data_ptr(),
                                                         self._game_over.data_ptr())
            if fin_ring is not None and self._fin_on:   # ... and its final record the current one (the replay below keeps none)
                self._fin_obs, self._fin_flags = own(fin_ring[0][t - 1]), own(fin_ring[1][t - 1])
                self._cf.obs, self._cf.flags = self._fin_obs.data_ptr(), self._fin_flags.data_ptr()
        if t < k:
            self._slab.copy_(la["snap"])
            if self._maps is not None:   # (in place: the CaMapSet points at this tensor)
                self._env_map.copy_(la["map_snap"])
            if t > 0:              # (rewrites slot t - 1 with the values it already holds)
                nat.check(self._launch_n(self._p_ref, self._cs_ref, self._co_ref, None, self._ar_ref,
                                          C.byref(nat.CaStepEx(n_steps=t, map=self._sx.map, set=self._sx.set)),
                                          self._stream_handle()))
        if self._met is not None:   # (the t slots handed out; the replay above recorded nothing)
            self._met_process()

    # ---------------------------------------------------------------- the final record (include/cagpu.h CaFinal)
    @property
    def final_step_bytes(self):
        """bytes the final record adds to one step's outputs (a ring slot): an observation block + a flag word per agent"""
        return self.E * self.N * (4 * self.W + 4)

    def keep_final(self, on=True):
        """Keep, for every env that auto-resets in a step, what the reset overwrites: the observation rows of the terminal
        step (`final_obs`, float32 [E, N, W] -- the vector-env APIs' final_observation / terminal_observation) and the
        agents' flag words as that step left them (`final_flags`, int32 [E, N] bit patterns: nat.decode_flags names the
        endings).  Stored by the step kernels themselves (CaStepEx.fin of cagpu_step_ex) through step(),
        rollout() and step_lookahead() alike; state, outputs and statistics are bit-identical to a run without it.  Rows
        are valid where `game_over` is set and UNSPECIFIED elsewhere.  After rollout(n) the record holds every env's most
        recent ending of those n steps (valid for the last step where `game_over` is set).  Needs a fixture table
        (set_fixture_table: without auto-reset nothing is overwritten, the terminal observation is `obs`); detaching the
        table switches it off.  Not combined with per-agent sensor variants (set_sensor_variants): those rows are rewritten
        on the host after the launch, the record holds what the kernel produced -- whichever comes second raises.  The
        laser-scan / occupancy-grid tensors are computed by their own kernels on the post-reset state and are not part of
        the record.  Off by default: a sim that never calls this runs the calls and kernels it ran before."""
        self.sync()
        on = bool(on)
        if on and self._ar is None:
            raise nat.CagpuError("keep_final: no fixture table attached (set_fixture_table): without auto-reset nothing is "
                                 "overwritten -- the terminal observation is `obs`")
        if on and self._variants:
            raise nat.CagpuError("keep_final: per-agent sensor variants (set_sensor_variants) are rewritten on the host after "
                                 "the launch and are not applied to the final record -- switch one of the two off")
        if on and not self._fin_on:
            self._fin_obs = torch.zeros((self.E, self.N, self.W), dtype=torch.float32, device=self.device)
            self._fin_flags = torch.zeros((self.E, self.N), dtype=torch.int32, device=self.device)
            self._cf.obs, self._cf.flags = self._fin_obs.data_ptr(), self._fin_flags.data_ptr()
        self._fin_on = on
        if not on:
            self._fin_obs, self._fin_flags = None, None
            self._cf.obs, self._cf.flags = None, None
        self._sx.fin = C.addressof(self._cf) if on else None
        if self._la is not None:
            self._la["prep"] = None   # (a prepared ring launch carries, or lacks, its final blocks)
            self._la["fin_ring"] = None

    # ---------------------------------------------------------------- the episode log (include/cagpu.h CaEpLog)
    def log_episodes(self, capacity=16, on=True):
        """Log every finished episode on the device: when an env's episode ends and the env is auto-reset, the step kernel
        itself (CaStepEx.log of cagpu_step_ex, through step(), rollout() and step_lookahead() alike) stores the
        reference's per-episode quantities (run_episode, experiments/src/env_utils.py:56-87) -- per agent total_reward,
        time_to_goal, extra_time_to_goal and the final flag word; per episode its index, length, fixture case and outcome
        -- in slot (episode index % capacity) of the env's own ring; episodes() drains what is new.  State, outputs and
        statistics are bit-identical to a run without it.  `capacity` has to cover the episodes an env can finish between
        two drains PLUS what a look-ahead ring computes ahead (at most one episode per ring step and env): older records
        are overwritten and episodes() reports them as `dropped`.  16 + 32 N bytes per slot: 22 MB at 4096 x 10 and the
        default capacity.  Needs a fixture table (set_fixture_table: without auto-reset no episode is logged); detaching the
        table switches it off.  reset() discards the undrained records of the envs it resets (their episode count restarts
        at 0).  Off by default: a sim that never calls this runs the calls and kernels it ran before."""
        self.sync()
        on = bool(on)
        if on and self._ar is None:
            raise nat.CagpuError("log_episodes: no fixture table attached (set_fixture_table): without auto-reset no episode "
                                 "is ever logged -- read the state when `game_over` shows")
        if on:
            cap = int(capacity)
            if cap < 1:
                raise nat.CagpuError("log_episodes: capacity must be >= 1")
            dev = self.device
            head = torch.full((self.E, cap, 4), -1, dtype=torch.int32, device=dev)
            rows = torch.zeros((self.E, cap, self.N, 4), dtype=torch.float64, device=dev)
            # (a log switched on mid-run starts at the envs' current episode: earlier ones were never written)
            cursor = self._state["reset_count"].to(torch.int64)
            self._log = dict(rows=rows, head=head, cursor=cursor, cap=cap)
            self._cl.rows, self._cl.head, self._cl.capacity = rows.data_ptr(), head.data_ptr(), cap   # (in place: _sx.log)
        else:
            self._log = None
            self._cl.rows, self._cl.head, self._cl.capacity = None, None, 0
        self._sx.log = C.addressof(self._cl) if on else None
        if self._la is not None:
            self._la["prep"] = None   # (a prepared ring launch is re-made: its CaStepEx carries, or lacks, the log)

    def _handed_out_reset_count(self):
        """reset_count [E] at the step LAST HANDED OUT, without a rewind: mid-ring the state has run ahead, so it is the
        count the ring started from (the snapshot slab) plus the game_over slots handed out since -- with a table attached
        every game over is exactly one auto-reset"""
        la = self._la
        if la is None or la["slots"] is None or la["t"] >= la["len"]:
            return self._state["reset_count"]
        off = self._state["reset_count"].data_ptr() - self._slab.data_ptr()
        rc = la["snap"][off:off + 4 * self.E].view(torch.int32).to(torch.int64)
        if la["t"] > 0:
            rc = rc + la["ring"][3][:la["t"]].sum(0, dtype=torch.int64)
        return rc

    def episodes(self):
        """Drain the episode log -> dict of device tensors with the M episodes finished since the last drain, ordered by
        (env, episode): `env`, `episode` (the env's k-th episode since its last reset()), `case` (row of the fixture table it
        ran on), `steps`, `outcome` (0 collision / 1 all at goal / 2 stuck) [M] int64; `total_reward`, `time_to_goal`,
        `extra_time_to_goal` [M, N] float64; `flags` [M, N] int32 (nat.decode_flags); with a map set attached `map` [M] int64, the
        env_map value the env held while the episode ran (-1 where it cannot be known any more: the key was replaced after
        the episode's map was drawn) -- and `dropped`, a Python int: the
        episodes that ended since the last drain but whose records were overwritten first (capacity too small).  Episodes
        of steps a look-ahead ring has computed but not handed out yet stay in the log for a later drain; the call neither
        rewinds nor drops the ring.  Synchronises with the device (M is read back)."""
        if self._log is None:
            raise nat.CagpuError("episodes: the episode log is off (log_episodes)")
        lg = self._log
        out, lg["cursor"] = episodes.drain(lg["rows"], lg["head"], lg["cursor"], self._handed_out_reset_count())
        if self._maps is not None:
            out["map"] = self._episode_maps(out["env"], out["episode"])
        return out

    def _episode_maps(self, env, k):
        """int64 [M]: the env_map value env[i] held while its episode k[i] ran (episodes.map_column; -1: not known)"""
        key, n = self.map_seed, int(env.shape[0])
        drawn = torch.zeros((n,), dtype=torch.int32, device=self.device)
        if key and n:   # cagpu_map_draw: the kernels' own map_draw for (global env id, reset count) pairs
            ge = (env + int(self._ar.env_id_offset if self._ar is not None else 0)).contiguous()
            cnt = k.to(torch.int32).contiguous()
            nat.check(self.lib.cagpu_map_draw(key, self.num_maps, ge.data_ptr(), cnt.data_ptr(), n, drawn.data_ptr(),
                                              self._stream()))
        return episodes.map_column(k, self._map_ep0[env], self._map_val0[env], self._map_key_from[env], bool(key), drawn)

    # ---------------------------------------------------------------- the episode metrics (include/cagpu.h CaEpMetrics)
    def measure_episodes(self, capacity=16, keep_tape=False, on=True):
        """Measure every episode on the device: per agent path_length, min_gap (the closest approach to anybody, its
        partner and time), turn_sum and the steps it moved / spent inside Config.GETTING_CLOSE_RANGE of somebody
        (DESIGN.md section 3j states the rules, tests/episode_metrics_ref.py restates them in NumPy and the kernel
        reproduces that file bit for bit).  A reduction kernel of its own (cagpu_episode_metrics) reads the trajectory
        tape -- recording is switched on if it is off -- after every launch: exactly the slots handed out, once each,
        whether they came from step(), rollout() or a look-ahead ring (the part of the ring behind the step handed out;
        a rewind's replay records nothing); no step kernel changes, and state, outputs and statistics are bit-identical to
        a run without it.  Env e's k-th episode goes to slot k % capacity of its ring -- log_episodes' rule, so the records
        join the log's by (env, episode) --; episode_metrics() drains what is new.  The episode that is RUNNING takes its
        slot with its first measured step: `capacity` has to cover the episodes an env can finish between two drains
        plus one.
        keep_tape=False: the tape is transient -- measured chunks are released and their bytes returned to the tape's
        budget, so an arbitrarily long run stays within record_trajectories' max_bytes; trajectories(), render_episode()
        and render_frames(episode=...) then see only what has not been measured yet (nothing, after a sync).  What the tape
        held when this was called is never measured and never released.  keep_tape=True: the tape is kept as
        record_trajectories() keeps it.
        path_length integrates with CaParams.dt (update_params(dt=...) counts from the next measured slot on): the
        env API's per-call `dt` of a single step is not seen.  An episode that is under way when this is switched on is
        measured from here on only -- switch it on in front of a reset for whole episodes.  Needs a fixture table
        (set_fixture_table), as log_episodes does; detaching the table switches it off.  reset() discards the running
        episode and the undrained records of the envs it resets.  on=False: pending slots are measured, the records are
        dropped, and recording stops if this call had started it.  Off by default: a sim that never calls this runs the
        calls and kernels it ran before."""
        self.sync()
        if self._met is not None:
            self._met_process()
        if not on:
            if self._met is not None:
                own = self._met["own_tape"]
                self._met = None
                if own and self._traj_on:
                    self.stop_recording()
            return
        if self._ar is None:
            raise nat.CagpuError("measure_episodes: no fixture table attached (set_fixture_table): without auto-reset the "
                                 "episodes of an env are not numbered")
        cap = int(capacity)
        if cap < 1:
            raise nat.CagpuError("measure_episodes: capacity must be >= 1")
        own = not self._traj_on
        if own:
            self.record_trajectories(**({} if self._traj is None else {"max_bytes": self._traj["max_bytes"]}))
        tr = self._traj
        for c in tr["chunks"]:      # what the tape holds already stays as it is: not measured, not released
            c["met"], c["kept"] = c["n"], True
        tr["block"], tr["open"] = None, None
        E, N, dev = self.E, self.N, self.device
        per_env = int(self.lib.cagpu_episode_metrics_carry_bytes(self._p_ref)) // E
        mt = dict(vals=torch.zeros((E, cap, N, 4), dtype=torch.float64, device=dev),
                  cnts=torch.zeros((E, cap, N, 4), dtype=torch.int32, device=dev),
                  head=torch.full((E, cap), -1, dtype=torch.int32, device=dev),
                  carry=torch.zeros((E, per_env), dtype=torch.uint8, device=dev),
                  cursor=self._state["reset_count"].to(torch.int64), cap=cap, keep_tape=bool(keep_tape), own_tape=own,
                  ct=nat.CaTraj())
        mt["cm"] = nat.CaEpMetrics(vals=mt["vals"].data_ptr(), cnts=mt["cnts"].data_ptr(), head=mt["head"].data_ptr(),
                                   capacity=cap, carry=mt["carry"].data_ptr(), getting_close_range=self.p.getting_close_range)
        self._met = mt

    def _met_process(self):
        """feed cagpu_episode_metrics every tape slot that was handed out and is not measured yet, in step order; with
        keep_tape=False the chunks measured to their end are released (their bytes go back to the tape's budget, the slot
        of a step() block is taken again by the next step -- behind the kernel that read it, on the same stream)"""
        mt, tr = self._met, self._traj
        if mt is None or tr is None:
            return
        la = self._la
        live = la.get("traj") if (la is not None and la["slots"] is not None and la["t"] < la["len"]) else None
        per_slot, kept = self.E * self.N * 96, []
        mt["cm"].getting_close_range = self.p.getting_close_range
        for c in tr["chunks"]:
            n = min(c["n"], la["t"]) if c is live else c["n"]
            m = c.get("met", 0)
            if n > m:
                mt["ct"].rows = c["rows"].data_ptr() + (c["start"] + m) * per_slot
                mt["ct"].episode = c["ep"].data_ptr() + (c["start"] + m) * self.E * 4
                nat.check(self.lib.cagpu_episode_metrics(self._p_ref, C.byref(mt["ct"]), n - m, C.byref(mt["cm"]),
                                                         self._stream()))
                c["met"] = n
            if mt["keep_tape"] or c is live or c.get("kept") or c.get("met", 0) < c["n"]:
                kept.append(c)
                continue
            tr["bytes"] -= c["n"] * self.traj_step_bytes
            if c is tr["open"]:
                tr["open"] = None
            b = tr["block"]
            if b is not None and b["rows"] is c["rows"] and b["used"] == c["start"] + c["n"]:
                b["used"] = c["start"]
        tr["chunks"] = kept

    def episode_metrics(self):
        """Drain the episode metrics -> dict of device tensors with the M episodes finished since the last drain, ordered
        by (env, episode) as episodes() orders the log's: `env`, `episode` [M] int64; `path_length`, `min_gap`, `turn_sum`,
        `min_gap_t` [M, N] float64; `moved_steps`, `close_steps`, `min_gap_partner` [M, N] int32 -- an agent that never had
        anybody to be close to has min_gap +inf, min_gap_t NaN, min_gap_partner -1; an absent slot all zeros with those --
        and `dropped`, a Python int: the episodes that ended since the last drain but whose records were overwritten first.
        Episodes of steps a look-ahead ring has computed but not handed out stay for a later drain; the call neither
        rewinds nor drops the ring.  Synchronises with the device (M is read back)."""
        if self._met is None:
            raise nat.CagpuError("episode_metrics: the episode metrics are off (measure_episodes)")
        self._met_process()
        mt = self._met
        out, mt["cursor"] = episode_metrics.drain(mt["vals"], mt["cnts"], mt["head"], mt["cursor"],
                                                  self._handed_out_reset_count())
        return out

    # ---------------------------------------------------------------- replay (replay.py; DESIGN.md "Replay")
    def episode_start(self, env, episode, _host=None):
        """The start state of episodes by their ADDRESS: `env` (a local index, as episodes() reports it) and `episode`, ints or
        int sequences of equal length M -> dict of device tensors: `cases` float64 [M, N, 6], `headings` float64 [M, N] (NaN:
        pointed at the goal), `policy_bits` int32 [M, N] (bits 6..11 of the flag word; -1 for an absent slot of a draw),
        `case` int64 [M] (the table row, or the 64-bit index under a case stream), with a map set `map` int64 [M] -- and
        `plan`, the host-side int64 arrays of replay.plan.  Episode 0 is what reset() loaded (kept); an episode k >= 1 is
        rebuilt by the kernels' own rules: the fixture table by the row formula or generate_cases_at(stream_case_index),
        cagpu_heading_draw under a heading_seed, cagpu_policy_draw_at under a policy draw (otherwise the words set_plugins
        gave the env's slots), cagpu_map_draw.  A pure function of the address: episodes that have not run yet are legal.
        Reads nothing of the running state (no look-ahead ring is rewound).  ValueError, before anything is launched, where
        the episode depended on something the batch did not keep (replay.refuse lists the cases)."""
        from . import replay as rp
        pl = rp.plan(self, env, episode, **(_host or {}))
        env, ep = pl["env"], pl["episode"]
        M, N, dev = len(env), self.N, self.device
        on_dev = lambda a, dt=torch.int64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(dev)
        env_t, ep_t = on_dev(env), on_dev(ep)
        cases = torch.zeros((M, N, 6), dtype=torch.float64, device=dev)
        headings = torch.full((M, N), math.nan, dtype=torch.float64, device=dev)
        first, later = np.flatnonzero(ep == 0), np.flatnonzero(ep != 0)
        if first.size:
            kept = self._start.index_select(0, on_dev(env[first]))
            cases.index_copy_(0, on_dev(first), kept[..., :6].contiguous())
            headings.index_copy_(0, on_dev(first), kept[..., 6].contiguous())
        ge, cnt = on_dev(pl["global_env"]), on_dev(ep, torch.int32)
        if later.size:
            at = on_dev(later)
            if self._cstream is not None:
                st = self._cstream
                keep = self._keep
                rows = self.generate_cases_at(on_dev(pl["case"][later]), st["seed"], **st["dist"])
                self._keep = keep + self._keep
            else:
                rows = self._table.index_select(0, on_dev(pl["row"][later]))
            cases.index_copy_(0, at, rows)
            if self._ar.heading_seed:
                g2, c2 = ge.index_select(0, at).contiguous(), cnt.index_select(0, at).contiguous()
                drawn = torch.empty((later.size, N), dtype=torch.float64, device=dev)
                nat.check(self.lib.cagpu_heading_draw(int(self._ar.heading_seed), N, g2.data_ptr(), c2.data_ptr(), later.size,
                                                      drawn.data_ptr(), self._stream()))
                headings.index_copy_(0, at, drawn)
        if self._draw is not None and M:
            present = (cases[..., 5] > 0).to(torch.uint8).contiguous() if self.p.ragged else None
            bits = torch.empty((M, N), dtype=torch.int32, device=dev)
            nat.check(self.lib.cagpu_policy_draw_at(self._draw["ref"], N, ge.data_ptr(), cnt.data_ptr(),
                                                    None if present is None else present.data_ptr(), M, bits.data_ptr(),
                                                    self._stream()))
        else:
            words = np.zeros((M, N), np.int32) if self._plugin_words is None else self._plugin_words[env]
            bits = on_dev(words & nat.POLICY_DRAW_BITS, torch.int32)
        out = {"cases": cases, "headings": headings, "policy_bits": bits, "case": on_dev(pl["case"]), "plan": pl}
        if self._maps is not None:
            out["map"] = self._episode_maps(env_t, ep_t)
            if M and bool((out["map"] < 0).any()):
                raise ValueError("replay: the map of a requested episode is not known any more (episodes() reports it as -1: "
                                 "the map set's key was replaced after that map was drawn)")
        return out

    def _replay_child(self, start, record, capacity):
        """the batch that runs the M episodes of `start` (episode_start) alone: this sim's CaParams, sort mode, ragged and
        pipeline switch, GA3C-CADRL weights and assignment, map (a set: the same stack, env_map = the episodes' maps, no key)
        and occupancy-grid settings; its fixture table is the M case rows with env_id_offset 0 and case_stride M -- child env
        i auto-resets into row i again, so that its terminal step runs the kernels' " final" instantiations and the final
        record, the log and the metrics produce the replay's records -- no heading seed, no policy draw, no case stream"""
        pl = start["plan"]
        env, M, N, dev = pl["env"], len(pl["env"]), self.N, self.device
        ps = nat.CaParams.from_buffer_copy(self.p)
        ps.num_envs = M
        child = BatchedSim(ps, device=dev, pipeline=self.pipeline)
        w = (np.zeros((M, N), np.int32) if self._plugin_words is None else self._plugin_words[env]).astype(np.int64)
        child.set_plugins((w >> nat.POLICY_SHIFT) & 0xF, (w >> nat.DYNAMICS_SHIFT) & 0xF, (w & nat.IS_LEARNING) != 0,
                          (w & nat.STILL_LEARNING) != 0)
        for idx, (_, ts) in self._nets.items():   # the parent's weights and packed planes, a packing list of the child's own
            ts2 = dict(ts)
            ts2["rows_scratch"] = torch.empty((M * N + 6,), dtype=torch.int32, device=dev)
            net = nat.CaNet(**{f: ts2[f].data_ptr() for f in nat.NET_FIELDS + ("rows_scratch", "packed")})
            child._nets[idx] = (net, ts2)
            if ts is self._net_tensors:
                child._net, child._net_tensors = net, ts2
        if self._nets:
            child.ga3c_fused = self.ga3c_fused
            if self.ga3c_value is not None:
                child.ga3c_value = torch.zeros((M, N), dtype=torch.float32, device=dev)
            if self._agent_net is not None:
                child._agent_net = self._agent_net.index_select(0, torch.as_tensor(env, device=dev)).contiguous()
        if self._map_src is not None:
            if self._maps is not None:
                child.set_map(env_map=start["map"].cpu().numpy(), map_seed=0, **self._map_src)
            else:
                child.set_map(**self._map_src)
            if self._occ is not None:
                child.set_occupancy_grid(self._occ.x_width, self._occ.y_width,
                                         packed=False if self.occ_bits is None else (True if self.occ is None else "both"))
        child.set_fixture_table(start["cases"], env_id_offset=0, case_stride=M, heading_seed=0)
        if self._rd is not None:   # the parent's RVO draw under the episodes' own addresses (CaRvoDraw.address)
            mask = None if self._rd["mask"] is None else self._rd["mask"].index_select(0, torch.as_tensor(env, device=dev)).cpu().numpy() != 0
            child.set_rvo_draw(heading_noise=mask, _address=np.stack([pl["global_env"], pl["episode"]], axis=1),
                               **self._rd["args"])
        if self._samp is not None:   # the parent's sampled GA3C-CADRL policy under the episodes' own addresses
            sm = self._samp
            mask = None if sm["mask"] is None else sm["mask"].index_select(0, torch.as_tensor(env, device=dev)).cpu().numpy() != 0
            child.set_ga3c_sampling(sm["seed"], sm["temperature"], mask=mask,
                                    _address=np.stack([pl["global_env"], pl["episode"]], axis=1))
        child.keep_final(True)
        child.log_episodes(capacity=capacity)
        if record:
            child.record_trajectories()
            child.measure_episodes(capacity=capacity + 1, keep_tape=True)
        # the start state: a first reset points every agent at its goal with the DEVICE's arctan2, as an auto-reset without
        # heading seed does; a second one hands those headings back where none was drawn or kept
        child.reset(start["cases"])
        h = start["headings"]
        child.reset(start["cases"], headings=torch.where(torch.isnan(h), child._state["heading"], h))
        # the flag words: bits 6..11 of present slots from the address, no plan (it belongs to the policy it was made for);
        # dynamics bits and the words of absent slots are the plugin words set above
        fl = child._state["flags"]
        here = (fl & nat.ABSENT) == 0
        fl.copy_(torch.where(here, (fl & ~(nat.POLICY_DRAW_BITS | nat.PLAN_VALID)) | (start["policy_bits"] & nat.POLICY_DRAW_BITS), fl))
        child._has_ga3c = child._plugins_ga3c = bool(self._has_ga3c)
        child.observe()   # (column 0 follows the bits)
        return child

    def replay(self, env, episode, record=True, max_steps=None, keep_outputs=False, _host=None):
        """Run episodes again from their address (episode_start) -> replay.Replay: a child batch of the M episodes alone
        (_replay_child) is stepped until every one of them has ended, and its final record, episode log, metrics and -- with
        `record` -- trajectory tape are the replay's, bit for bit what the original run gave or would have given.
        max_steps: default, the most steps any of the M cases can take under max_time_ratio; a replay that needs more
        raises CagpuError.  keep_outputs: also keep obs / rewards / done of every step (Replay.outputs).  The child runs
        under the CURRENT CaParams: an update_params() between the original episode and the replay is the caller's
        business.  This sim is not touched: no state, output, statistic or tape of it changes, and a look-ahead ring
        that has run ahead is not rewound."""
        from . import replay as rp
        return rp.run(self, env, episode, record=record, max_steps=max_steps, keep_outputs=keep_outputs, host=_host)

    # ---------------------------------------------------------------- the trajectory tape (include/cagpu.h CaTraj)
    TRAJ_BLOCK_BYTES = 8 << 20   # step(): slots are taken from blocks of about this size (at most 64 slots), not a tensor per step

    @property
    def tape_bytes(self):
        """bytes of the tape's budget (record_trajectories' max_bytes) in use"""
        return 0 if self._traj is None else self._traj["bytes"]

    @property
    def traj_step_bytes(self):
        """bytes of one recorded step: 96 per agent slot + 4 per env"""
        return 96 * self.E * self.N + 4 * self.E

    def record_trajectories(self, max_bytes=1 << 30):
        """Record every agent's trajectory on the device from the next step on: the step kernels themselves write the
        reference's Agent.global_state_history row (agent.py:257-289) of every agent that moves, through step(),
        rollout() and step_lookahead() alike (CaStepEx.traj of cagpu_step_ex).  Off by default -- the reference's
        Config.STORE_HISTORY default does not switch it on for a batch (96 bytes per agent and step).  max_bytes: the
        budget of the tape; the launch that would take it past the budget raises CagpuError BEFORE it runs (nothing is
        dropped silently, the tape stays valid; clear_trajectories() makes room); a look-ahead ring is shortened to what
        still fits.  Calling it again changes the budget and keeps the tape."""
        self.sync()
        if self._traj is None:
            self._traj = dict(chunks=[], bytes=0, block=None, open=None,
                              epoch=torch.zeros((self.E,), dtype=torch.int32, device=self.device))
        self._traj["max_bytes"] = int(max_bytes)
        self._traj_switch(True)

    def stop_recording(self):
        """the steps from here on are not recorded (nor measured: measure_episodes); the tape stays readable
        (trajectories()) until clear_trajectories()"""
        self.sync()
        if self._met is not None:
            self._met_process()
        self._traj_switch(False)

    def clear_trajectories(self):
        """forget the tape recorded so far (T = 0); recording stays as it is (on / off, budget)"""
        self.sync()
        if self._met is not None:   # (what was handed out is measured before it goes)
            self._met_process()
        tr = self._traj
        if tr is not None:
            tr["chunks"], tr["bytes"], tr["block"], tr["open"] = [], 0, None, None

    def _traj_switch(self, on):
        self._traj_on = bool(on)
        self._sx.traj = C.addressof(self._ct) if self._traj_on else None   # (_traj_slot rewrites _ct in place)
        if self._traj is not None:
            self._traj["open"] = None
        if self._la is not None:
            self._la["prep"] = None   # (a prepared ring launch carries, or lacks, its chunk of the tape)

    def _traj_fit(self):
        """how many more steps the budget holds; raises when it holds none"""
        tr, per = self._traj, self.traj_step_bytes
        fit = (tr["max_bytes"] - tr["bytes"]) // per
        if fit < 1:
            raise nat.CagpuError("trajectory tape full: %d of max_bytes = %d bytes recorded, one more step takes %d bytes "
                                 "(96 * E * N + 4 * E) -- read trajectories() and call clear_trajectories(), or "
                                 "record_trajectories(max_bytes=...) with a larger budget; no step was taken"
                                 % (tr["bytes"], tr["max_bytes"], per))
        return fit

    def _traj_alloc(self, n):
        return (torch.empty((n, self.E, self.N, 12), dtype=torch.float64, device=self.device),
                torch.empty((n, self.E), dtype=torch.int32, device=self.device))

    def _traj_slot(self):
        """point self._ct at the next slot of the current block (step(): one slot per launch)"""
        tr, per = self._traj, self.traj_step_bytes
        fit = self._traj_fit()
        b = tr["block"]
        if b is None or b["used"] >= b["cap"]:
            cap = int(max(1, min(64, self.TRAJ_BLOCK_BYTES // per, fit)))
            rows, ep = self._traj_alloc(cap)
            b = tr["block"] = dict(rows=rows, ep=ep, used=0, cap=cap)
            tr["open"] = None
        c = tr["open"]
        if c is None:       # a run of consecutive slots of one block under one epoch
            c = tr["open"] = dict(rows=b["rows"], ep=b["ep"], start=b["used"], n=0, epoch=tr["epoch"])
            tr["chunks"].append(c)
        self._ct.rows = b["rows"].data_ptr() + b["used"] * self.E * self.N * 96
        self._ct.episode = b["ep"].data_ptr() + b["used"] * self.E * 4
        b["used"] += 1
        c["n"] += 1
        tr["bytes"] += per

    def _traj_chunk(self, n, tensors=None):
        """a chunk of n slots for ONE multi-step launch -> (chunk, CaTraj); raises when the budget does not hold n steps"""
        tr, per = self._traj, self.traj_step_bytes
        if self._traj_fit() < n:
            raise nat.CagpuError("trajectory tape: %d steps of %d bytes (96 * E * N + 4 * E) do not fit the %d bytes left of "
                                 "max_bytes = %d -- clear_trajectories() or a larger budget; no step was taken"
                                 % (n, per, tr["max_bytes"] - tr["bytes"], tr["max_bytes"]))
        if tensors is None or tensors[0].shape[0] != n:
            tensors = self._traj_alloc(n)
        chunk = dict(rows=tensors[0], ep=tensors[1], start=0, n=n, epoch=tr["epoch"])
        return chunk, nat.CaTraj(rows=tensors[0].data_ptr(), episode=tensors[1].data_ptr())

    def _traj_commit(self, chunk):
        tr = self._traj
        tr["chunks"].append(chunk)
        tr["bytes"] += chunk["n"] * self.traj_step_bytes
        tr["open"] = None
        return chunk

    def trajectories(self):
        """The tape recorded since record_trajectories() / the last clear_trajectories(), in step order, on the device:
          rows     float64 [T, E, N, 12]: columns 0 - 10 the reference's global_state_history row (t, px, py, gx, gy,
                   radius, pref_speed, vx, vy, speed, heading), column 11 the row's index in the agent's history --
                   or -1 for an agent that did not move in that step, whose other columns are UNSPECIFIED;
          episode  int32 [T, E]: the env's auto-reset count as the step started;
          epoch    int32 [T, E]: the host-side resets (reset() / reset_from_table()) of the env since recording began --
                   a reset logs no row but ends the episode (trajectory.episodes splits where either counter changes).
        T = the steps handed out (goes through sync()).  Returns copies.  With measure_episodes(keep_tape=False) the tape
        is transient: only the slots not measured yet are here -- none, once the sync has measured them."""
        self.sync()
        tr = self._traj
        E, N, dev = self.E, self.N, self.device
        cs = [] if tr is None else [c for c in tr["chunks"] if c["n"] > 0]
        if not cs:
            return {"rows": torch.empty((0, E, N, 12), dtype=torch.float64, device=dev),
                    "episode": torch.empty((0, E), dtype=torch.int32, device=dev),
                    "epoch": torch.empty((0, E), dtype=torch.int32, device=dev)}
        sl = lambda c, t: t[c["start"]:c["start"] + c["n"]]
        return {"rows": torch.cat([sl(c, c["rows"]) for c in cs]), "episode": torch.cat([sl(c, c["ep"]) for c in cs]),
                "epoch": torch.cat([c["epoch"].unsqueeze(0).expand(c["n"], E) for c in cs])}

    # ---------------------------------------------------------------- frames (include/cagpu.h CaRender)
    RENDER_WORK_BYTES = 256 << 20   # frames are rendered in groups whose primitive lists fit this much scratch

    def _render_counters(self, ids, every=False):
        """the tape's counters of the envs `ids` (device int64 [S]; every: all envs in order, nothing to gather)
        -> episode [T, S], epoch [T, S], 4 bytes per env and slot each"""
        tr = self._traj
        cs = [] if tr is None else [c for c in tr["chunks"] if c["n"] > 0]
        S = int(ids.shape[0])
        if not cs:
            none = torch.empty((0, S), dtype=torch.int32, device=self.device)
            return none, none
        pick = (lambda t, d: t) if every else (lambda t, d: t.index_select(d, ids))
        ep = [pick(c["ep"][c["start"]:c["start"] + c["n"]], 1) for c in cs]
        epoch = [pick(c["epoch"], 0).unsqueeze(0).expand(c["n"], S) for c in cs]
        return (ep[0], epoch[0]) if len(cs) == 1 else (torch.cat(ep), torch.cat(epoch))

    def _render_rows(self, ids, t0, t1, every=False):
        """the slots [t0, t1) of the tape of the envs `ids` as one history block -> rows [t1 - t0, S, N, 12], gathered on
        the device from the chunks that overlap the range only; a range inside one chunk with every env in order is a
        VIEW of the tape, not a copy (the launch reads it through its strides)"""
        pieces, base = [], 0
        for c in self._traj["chunks"]:
            a, b = max(t0, base), min(t1, base + c["n"])
            if a < b:
                t = c["rows"][c["start"] + a - base:c["start"] + b - base]
                pieces.append(t if every else t.index_select(1, ids))
            base += c["n"]
        return pieces[0] if len(pieces) == 1 else torch.cat(pieces)

    def _render_launch(self, frame_env, frame_col, first, last, rows, size, limits, circles, draw_map):
        """F frames from device int32 [F] descriptors and a history block [T, S, N, 12] (or None) -> uint8 [F, H, W, 3]"""
        from . import render as rd
        H, W = int(size[0]), int(size[1])
        xmin, ymax, s16 = rd.window((H, W), limits)
        F = int(frame_env.shape[0])
        T = 0 if rows is None else int(rows.shape[0])
        per = int(self.lib.cagpu_render_work_bytes(1, self.N, T))
        group = max(1, min(F, self.RENDER_WORK_BYTES // per))
        work = torch.empty((int(self.lib.cagpu_render_work_bytes(group, self.N, T)),), dtype=torch.uint8, device=self.device)
        i32 = lambda t: t.to(torch.int32).contiguous()
        frame_env, frame_col, first, last = i32(frame_env), i32(frame_col), i32(first), i32(last)
        flags = (nat.RENDER_CIRCLES if circles else 0) | (nat.RENDER_MAP if draw_map else 0)
        outs = []
        for f0 in range(0, F, group):
            n = min(group, F - f0)
            out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=self.device)
            r = nat.CaRender(out=out.data_ptr(), num_frames=n, height=H, width=W, flags=flags, xmin=xmin, ymax=ymax, s16=s16,
                             frame_env=frame_env[f0:].data_ptr(), frame_col=frame_col[f0:].data_ptr(),
                             first=first[f0:].data_ptr(), last=last[f0:].data_ptr(),
                             hist=None if rows is None else rows.data_ptr(), hist_steps=T,
                             hist_cols=0 if rows is None else int(rows.shape[1]),
                             stride_t=0 if rows is None else int(rows.stride(0)), stride_s=0 if rows is None else int(rows.stride(1)),
                             work=work.data_ptr(), work_bytes=work.numel())
            if self._maps is not None:
                nat.check(self.lib.cagpu_render_maps(C.byref(self.p), C.byref(self._cs), C.byref(self._maps), C.byref(r),
                                                     self._stream()))
            else:
                nat.check(self.lib.cagpu_render(C.byref(self.p), C.byref(self._cs),
                                                None if self._map is None else C.byref(self._map), C.byref(r), self._stream()))
            outs.append(out)
        # (torch's caching allocator keeps a freed block for the stream that used it: the scratch tensors may go out of scope)
        return outs[0] if len(outs) == 1 else torch.cat(outs)

    def render_frames(self, env_ids=None, size=(128, 128), limits=None, episode="current", upto=None, circles_along_traj=True,
                      draw_map=True):
        """One picture per env of `env_ids` (default: all), rasterised on the device (cagpu_render, csrc/cagpu_render.inc;
        the reference's visualize.plot_episode minus text and axes): uint8 device tensor [S, H, W, 3], size = (H, W), showing
        the window `limits` = ((xmin, xmax), (ymin, ymax)) (default: the 16 m x 16 m map extent) at equal scale.
        episode="current": the running episode of each env as the trajectory tape holds it (record_trajectories);
        "last": the most recent episode BEFORE the running one that the tape holds -- what the reference plots at the reset
        that follows an episode; upto=k: the episode as of its k-th recorded step.  An env whose episode has no slot on the
        tape (recording off, right after a reset, no earlier episode) gets a SNAPSHOT frame: the current state, one disc
        per agent and its goal.  The history is gathered from the tape's chunks and the episode boundaries are found from
        the tape's counters on the device: no tape row and no state travels to the host (two integers do: the bounds of
        the tape window that the frames show, so that only its slots are gathered and the scratch is sized by it).  Goes
        through sync(); writes nothing of the simulator."""
        from . import render as rd
        self.sync()
        ids = torch.arange(self.E, device=self.device) if env_ids is None else \
            torch.as_tensor(env_ids, dtype=torch.int64).reshape(-1).to(self.device)
        every = env_ids is None
        ep, epoch = self._render_counters(ids, every)
        cur_epoch = torch.zeros((self.E,), dtype=torch.int32, device=self.device) if self._traj is None else self._traj["epoch"]
        first, last = rd.episode_ranges(ep, epoch, self._state["reset_count"].index_select(0, ids),
                                        cur_epoch.index_select(0, ids), episode, upto)
        rows, T = None, int(ep.shape[0])
        if T > 0:
            # the window of the tape that some frame shows (two integers read back): only its slots are gathered, and the
            # primitive lists are sized by it, not by the whole tape
            has = last >= first
            t0, t1 = torch.stack([torch.where(has, first, torch.full_like(first, T)).min(),
                                  torch.where(has, last, torch.full_like(last, -1)).max()]).tolist()
            if t1 >= t0:
                rows = self._render_rows(ids, t0, t1 + 1, every)
                first, last = first - t0, last - t0
        return self._render_launch(ids, torch.arange(int(ids.shape[0]), device=self.device), first, last, rows, size, limits,
                                   circles_along_traj, draw_map)

    def render_episode(self, env_id, episode="last", every=1, size=(128, 128), limits=None, circles_along_traj=True,
                       draw_map=True):
        """The animation of ONE episode of env `env_id` from ONE launch: uint8 device tensor [F, H, W, 3], frame j showing
        the episode's first (j + 1) * every recorded steps, the last frame all of them (render_frames(upto=...) of the same
        prefixes, bit for bit).  Only the episode's LENGTH is read back (two integers) to size the output; with no such
        episode on the tape the result is one snapshot frame."""
        from . import render as rd
        self.sync()
        ids = torch.as_tensor([int(env_id)], dtype=torch.int64, device=self.device)
        ep, epoch = self._render_counters(ids)
        cur_epoch = torch.zeros((self.E,), dtype=torch.int32, device=self.device) if self._traj is None else self._traj["epoch"]
        first, last = rd.episode_ranges(ep, epoch, self._state["reset_count"].index_select(0, ids),
                                        cur_epoch.index_select(0, ids), episode)
        f0, l0 = int(first[0]), int(last[0])
        lasts = rd.prefix_lasts(l0 - f0 + 1, every)
        if not lasts:
            return self._render_launch(ids, torch.zeros_like(ids), first, last, None, size, limits, circles_along_traj, draw_map)
        rows = self._render_rows(ids, f0, l0 + 1)       # (the episode's slots only: the primitive lists are sized by the block)
        F = len(lasts)
        zero = torch.zeros((F,), dtype=torch.int32, device=self.device)
        return self._render_launch(ids.expand(F), zero, zero, torch.as_tensor(lasts, dtype=torch.int32, device=self.device), rows,
                                   size, limits, circles_along_traj, draw_map)

    # ---------------------------------------------------------------- statistics
    def _fault_probe(self):
        """The device's fault word on the product path, without a synchronisation: a 4-byte copy into pinned host memory
        is queued behind the launch just submitted (cagpu_device_faults_async); the word an EARLIER probe brought back is
        looked at here once its copy has landed.  A raised bit (a hand-over poll of the pipelined kernel ran out, a
        GA3C-CADRL operand left the fp16 range) raises CagpuError through check_faults()."""
        if torch.cuda.is_current_stream_capturing():
            return                   # (a step captured into a HIP graph: events and side streams have no place in the capture)
        fp = self._fault
        if fp is None:
            # the copy runs on a stream of its own: the word is a device global that kernels OR bits into, so the read needs
            # no ordering with the launches -- and on the compute stream a 4-byte device-to-host copy behind every ring launch
            # would sit between the kernel's end and the caller's synchronisation (~5 us of a 200 us block)
            fp = self._fault = dict(buf=torch.zeros((1,), dtype=torch.int32).pin_memory(), ev=torch.cuda.Event(), busy=False, probes=0,
                                    stream=torch.cuda.Stream(device=self.device))
            fp["h"] = (C.c_void_p(fp["buf"].data_ptr()), C.c_void_p(fp["stream"].cuda_stream))
        if fp["busy"]:
            if not fp["ev"].query():
                return               # (still in flight: looked at by a later call)
            fp["busy"] = False
            if int(fp["buf"][0]) != 0:
                self.check_faults()  # (synchronising read + clear; raises)
        with torch.cuda.device(self.device):     # (the word is the CURRENT device's symbol: a process that drives several GPUs)
            rc = self.lib.cagpu_device_faults_async(*fp["h"])
            if rc != 0:
                nat.check(rc)
            fp["ev"].record(fp["stream"])
        fp["busy"] = True
        fp["probes"] += 1

    def check_faults(self):
        """Raise if a step kernel flagged a fault on this device since the last check (cagpu_device_faults: a bounded
        hand-over poll of the pipelined kernel ran out -- the state may be wrong).  Synchronises the device."""
        with torch.cuda.device(self.device):
            f = nat.device_faults(clear=True)
        if f:
            raise nat.CagpuError("device fault word 0x%x:%s%s%s%s the simulator state is not to be trusted" % (
                f, " a hand-over inside the pipelined step kernel timed out;" if f & 1 else "",
                " a GA3C-CADRL operand left the fp16 range of the network kernel's two-plane split (|x| >= 65504, or an "
                "input column was not finite);" if f & 2 else "",
                " bit 2: a map-set env's map index (env_map) lay outside [0, num_maps), that env saw an empty map;" if f & 4 else "",
                " bit 3: an env of a case stream auto-reset more than `window` times between two refills and repeated a "
                "scenario (set_case_stream: a larger window, or shorter launches);" if f & 8 else ""))

    def episode_stats(self, check=True):
        """Per-shard episode counters: float64 [8] (see STAT_NAMES), reduced on the device.  A reporting point: the
        device's fault word is checked here (one small synchronising read)."""
        self.sync()
        if check:
            self.check_faults()
        return self._state["env_stats"].sum(dim=0)


_GA3C_NAMES = {"logits_kernel": "logits_p_kernel", "logits_bias": "logits_p_bias"}
_GA3C_SHAPES = {"lstm_kernel": (71, 256), "lstm_bias": (256,), "layer1_kernel": (68, 256), "layer1_bias": (256,),
                "layer2_kernel": (256, 256), "layer2_bias": (256,), "fc1_kernel": (256, 256), "fc1_bias": (256,),
                "logits_kernel": (256, 11), "logits_bias": (11,), "input_mean": (138,), "input_std": (138,)}


class Experience(object):
    """What BatchedSim.collect(n) recorded (its docstring lists the fields: obs, action, logp, value, live, reward, done,
    game_over, last_value, address -- device tensors, `n` steps); gae() adds advantages and returns."""
    FIELDS = ("obs", "action", "logp", "value", "live", "reward", "done", "game_over", "last_value", "address")

    def __init__(self, sim, t):
        self._sim, self.n = sim, int(t["action"].shape[0])
        for k in self.FIELDS:
            v = t[k]
            setattr(self, k, v.view(torch.bool) if v is not None and v.dtype == torch.uint8 else v)

    def gae(self, gamma=0.99, lam=0.95):
        """-> (advantage, returns), float32 [n, E, N], by cagpu_gae (include/cagpu.h has the rule: float32, every product and
        sum rounded on its own).  Every ending is TERMINAL: where done[t] or game_over[t] is set the agent's episode ended
        in step t and nothing is bootstrapped -- a time-out included, because the network is never queried on a terminal
        observation.  Slots that are not live get 0 and cut the recursion; the last live slot of a column bootstraps from
        last_value."""
        sim = self._sim
        n, E, N = self.reward.shape
        adv, ret = torch.empty_like(self.reward), torch.empty_like(self.reward)
        u8 = lambda v: v.view(torch.uint8).data_ptr()
        nat.check(sim.lib.cagpu_gae(n, E * N, N, self.reward.data_ptr(), self.value.data_ptr(), self.last_value.data_ptr(),
                                    u8(self.live), u8(self.done), u8(self.game_over), float(gamma), float(lam),
                                    adv.data_ptr(), ret.data_ptr(), sim._stream()))
        return adv, ret

    def rows(self):
        """-> (x [n E N, W - 1] float32, live [n E N] bool): every (step, env, agent) slot of the tape as one row, in that
        order -- VIEWS of the tape, no boolean selection and therefore no host synchronisation (what
        experiments/collect_onpolicy.collect pays for its compact batch).  ga3c_grad and ga3c_train.TrainableGA3C take the
        pair as it is: rows that are not live are never read."""
        if self.obs is None:
            raise nat.CagpuError("Experience.rows: the tape was collected with keep_obs=False")
        return self.obs.reshape(-1, self.obs.shape[-1]), self.live.reshape(-1)


def _ga3c_weight_tensors(weights, device):
    """weights (None = the shipped default, an .npz path, or a dict of float32 arrays) -> {CaNet field: device tensor},
    plus value_kernel [256] / value_bias [1] where the weights carry logits_v_*"""
    if weights is None:
        weights = GA3C_DEFAULT_WEIGHTS
    if isinstance(weights, str):
        with np.load(weights) as z:
            weights = {k: z[k] for k in z.files}
    ts = {}
    for f in nat.NET_FIELDS:
        a = np.ascontiguousarray(weights[_GA3C_NAMES.get(f, f)], dtype=np.float32)
        if a.shape != _GA3C_SHAPES[f]:
            raise ValueError("GA3C-CADRL weight %s has shape %s, expected %s" % (f, a.shape, _GA3C_SHAPES[f]))
        ts[f] = torch.from_numpy(a).to(device)
    if "logits_v_kernel" in weights and "logits_v_bias" in weights:
        k = np.ascontiguousarray(weights["logits_v_kernel"], dtype=np.float32)
        b = np.ascontiguousarray(weights["logits_v_bias"], dtype=np.float32)
        if k.shape != (256, 1) or b.shape != (1,):
            raise ValueError("GA3C-CADRL weight logits_v has shapes %s / %s, expected (256, 1) / (1,)" % (k.shape, b.shape))
        ts["value_kernel"] = torch.from_numpy(k.reshape(256)).to(device)
        ts["value_bias"] = torch.from_numpy(b).to(device)
    return ts


# (device, checkpoint) -> (CaNet, its tensors, the weights object).  A checkpoint given as a path is keyed by the path; one
# given as a dict by the dict's IDENTITY (the entry holds the dict, so the id stays its own): a dict changed in place after
# its first query is NOT re-uploaded -- pass a new dict, or call ga3c_query_forget().  Each entry pins 1.3 MB of device
# memory (weights + packed planes); the cache holds the _QUERY_NETS_MAX most recently used and drops the oldest.
_query_nets = {}
_QUERY_NETS_MAX = 16


def ga3c_query_forget():
    """drop every cached device copy of ga3c_query's networks (their memory goes back once no launch uses it)"""
    _query_nets.clear()


def _query_net(weights, device):
    """the uploaded + packed network of ga3c_query, cached per (device, checkpoint): a path by its name, a dict by identity"""
    if weights is None:
        weights = GA3C_DEFAULT_WEIGHTS
    key = (str(device), weights if isinstance(weights, str) else id(weights))
    hit = _query_nets.pop(key, None)   # (re-inserted below: the dict's order is the order of last use)
    if hit is None:
        L = nat.lib()
        ts = _ga3c_weight_tensors(weights, device)
        ts["packed"] = torch.empty((int(L.cagpu_ga3c_packed_bytes()),), dtype=torch.uint8, device=device)
        net = nat.CaNet(**{f: ts[f].data_ptr() for f in nat.NET_FIELDS + ("packed",)})
        with torch.cuda.device(device):
            st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
            nat.check(L.cagpu_ga3c_pack(C.byref(net), ts["packed"].data_ptr(), ts["packed"].numel(), st))
        hit = (net, ts, weights)
        while len(_query_nets) >= _QUERY_NETS_MAX:
            _query_nets.pop(next(iter(_query_nets)))
    _query_nets[key] = hit
    return hit


def ga3c_query(x, weights=None, want=("logits", "value", "action"), device=None):
    """The GA3C-CADRL network on given rows, without a simulator (cagpu_ga3c_query; NetworkVPCore.predict_p and the value
    fetch of GA3C_CADRL/network.py:24-41, :74).  x: [rows, width] policy vectors X = obs[1:] -- a float32 device tensor is
    read in place, anything else (numpy, lists, other dtypes / devices) is copied to `device` (default: x's own device if
    it is a GPU tensor, else cuda:0); width is cropped / zero-padded to 138 as crop_x does.  weights: as load_ga3c (the
    packed weights are cached per device and checkpoint).  want: which of "logits" [rows, 11], "value" [rows], "action"
    int32 [rows] (first maximum) to compute.  Returns {name: device tensor}."""
    want = tuple(want)
    bad = set(want) - {"logits", "value", "action"}
    if bad or not want:
        raise ValueError("ga3c_query: want must name some of logits / value / action, got %r" % (want,))
    if device is None:
        device = x.device if (torch.is_tensor(x) and x.is_cuda) else "cuda:0"
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    xt = torch.as_tensor(x)
    if xt.dim() != 2 or xt.shape[1] < 1:
        raise ValueError("ga3c_query: x must be [rows, width >= 1], got shape %s" % (tuple(xt.shape),))
    xt = xt.to(device=device, dtype=torch.float32).contiguous()
    net, ts, _ = _query_net(weights, device)
    rows = int(xt.shape[0])
    out = {}
    if "logits" in want:
        out["logits"] = torch.empty((rows, 11), dtype=torch.float32, device=device)
    if "value" in want:
        if "value_kernel" not in ts:
            raise ValueError("ga3c_query: these GA3C-CADRL weights have no logits_v_kernel / logits_v_bias (value head)")
        out["value"] = torch.empty((rows,), dtype=torch.float32, device=device)
    if "action" in want:
        out["action"] = torch.empty((rows,), dtype=torch.int32, device=device)
    if rows == 0:   # (an empty tensor has no address to hand over; the C entry point would launch nothing either)
        return out
    ptr = lambda n: out[n].data_ptr() if n in out else None
    q = nat.CaNetQuery(x=xt.data_ptr(), rows=rows, width=int(xt.shape[1]),
                       value_kernel=ts["value_kernel"].data_ptr() if "value" in out else None,
                       value_bias=ts["value_bias"].data_ptr() if "value" in out else None,
                       logits=ptr("logits"), value=ptr("value"), action=ptr("action"))
    with torch.cuda.device(device):
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        nat.check(nat.lib().cagpu_ga3c_query(C.byref(net), C.byref(q), st))
    return out


# ---------------------------------------------------------------- the network's weight gradients (cagpu_ga3c_grad)
# the layout of the flat gradient: the checkpoint's key order and shapes (include/cagpu.h, CaNetGrad)
GA3C_GRAD_LAYOUT = (("lstm_kernel", (71, 256)), ("lstm_bias", (256,)), ("layer1_kernel", (68, 256)), ("layer1_bias", (256,)),
                    ("layer2_kernel", (256, 256)), ("layer2_bias", (256,)), ("fc1_kernel", (256, 256)), ("fc1_bias", (256,)),
                    ("logits_p_kernel", (256, 11)), ("logits_p_bias", (11,)), ("logits_v_kernel", (256, 1)),
                    ("logits_v_bias", (1,)))


def ga3c_grad_offsets():
    """-> {checkpoint key: (offset in floats, shape)} of cagpu_ga3c_grad's flat gradient, and their total as [None]"""
    out, at = {}, 0
    for k, shape in GA3C_GRAD_LAYOUT:
        out[k] = (at, shape)
        at += int(np.prod(shape))
    out[None] = (at, ())
    return out


def ga3c_grad_views(flat):
    """the flat gradient buffer -> {checkpoint key: view of its own shape}"""
    return {k: flat[o:o + int(np.prod(s))].view(s) for k, (o, s) in ga3c_grad_offsets().items() if k is not None}


def ga3c_grad_chunk_rows(rows, max_work_bytes, work_bytes=None):
    """rows per cagpu_ga3c_grad call such that its workspace stays within max_work_bytes: a pure function of the two.  All
    rows where they fit; else the rows are cut into the fewest chunks that fit, of equal size (the last may be shorter).
    work_bytes: rows -> bytes (default: cagpu_ga3c_grad_work_bytes).  ValueError if not even one row fits."""
    wb = work_bytes if work_bytes is not None else (lambda r: int(nat.lib().cagpu_ga3c_grad_work_bytes(int(r))))
    rows, budget = int(rows), int(max_work_bytes)
    if rows <= 0 or wb(rows) <= budget:
        return max(rows, 0)
    if wb(1) > budget:
        raise ValueError("ga3c_grad: max_work_bytes = %d is below the workspace of a single row (%d bytes)" % (budget, wb(1)))
    lo, hi = 1, rows          # wb(lo) <= budget < wb(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if wb(mid) <= budget:
            lo = mid
        else:
            hi = mid
    chunks = -(-rows // lo)
    return -(-rows // chunks)


def _grad_net(weights, device):
    """weights as ga3c_query takes them, or a dict of float32 device tensors under the checkpoint's keys ->
    (CaNet, value_kernel tensor or None, value_bias tensor or None, what keeps the memory alive)"""
    if isinstance(weights, dict) and weights and all(torch.is_tensor(v) for v in weights.values()):
        shapes = dict(GA3C_GRAD_LAYOUT, input_mean=(138,), input_std=(138,))
        ts = {}
        for k, v in weights.items():
            if k not in shapes:
                raise ValueError("ga3c_grad: unknown weight key %r" % (k,))
            if v.dtype != torch.float32 or v.device != device or tuple(v.shape) != shapes[k]:
                raise ValueError("ga3c_grad: %s must be a float32 tensor of shape %s on %s" % (k, shapes[k], device))
            ts[k] = v.detach().contiguous()
        missing = [_GA3C_NAMES.get(f, f) for f in nat.NET_FIELDS if _GA3C_NAMES.get(f, f) not in ts]
        if missing:
            raise ValueError("ga3c_grad: weights lack %s" % ", ".join(missing))
        net = nat.CaNet(**{f: ts[_GA3C_NAMES.get(f, f)].data_ptr() for f in nat.NET_FIELDS})
        return net, ts.get("logits_v_kernel"), ts.get("logits_v_bias"), ts
    net, ts, _ = _query_net(weights, device)
    return net, ts.get("value_kernel"), ts.get("value_bias"), ts


def _ga3c_grad_into(flat, net, value_kernel, value_bias, xt, dlogits, dvalue, live, max_work_bytes):
    """cagpu_ga3c_grad into the flat buffer, chunked in array order under the workspace budget (accumulate from the second
    chunk on).  Every tensor is a contiguous device tensor of the right dtype (or None) by now."""
    L = nat.lib()
    rows, width = int(xt.shape[0]), int(xt.shape[1])
    if rows == 0:
        flat.zero_()
        return flat
    chunk = ga3c_grad_chunk_rows(rows, max_work_bytes)
    work = torch.empty((int(L.cagpu_ga3c_grad_work_bytes(chunk)),), dtype=torch.uint8, device=xt.device)
    at = lambda t, r0, per: None if t is None else t.data_ptr() + r0 * per * t.element_size()
    with torch.cuda.device(xt.device):
        st = C.c_void_p(torch.cuda.current_stream(xt.device).cuda_stream)
        for r0 in range(0, rows, chunk):
            q = nat.CaNetGrad(x=at(xt, r0, width), rows=min(chunk, rows - r0), width=width, accumulate=1 if r0 else 0,
                              live=at(live, r0, 1), dlogits=at(dlogits, r0, 11), dvalue=at(dvalue, r0, 1),
                              value_kernel=None if value_kernel is None else value_kernel.data_ptr(),
                              value_bias=None if value_bias is None else value_bias.data_ptr(),
                              grad=flat.data_ptr(), work=work.data_ptr(), work_bytes=work.numel())
            nat.check(L.cagpu_ga3c_grad(C.byref(net), C.byref(q), st))
    return flat


def ga3c_grad(x, dlogits=None, dvalue=None, live=None, weights=None, max_work_bytes=256 << 20):
    """Weight gradients of the GA3C-CADRL network (cagpu_ga3c_grad; include/cagpu.h states the rule): the SUM over the live
    rows of the row's vector-Jacobian product with the upstream gradients dlogits [rows, 11] (of logits_p) and dvalue [rows]
    (of the value head); at least one of the two.  x: [rows, width] as ga3c_query takes it; live: bool / uint8 [rows] or
    None -- rows with live == 0 are never read.  weights: as ga3c_query, or a dict of float32 device tensors under the
    checkpoint's keys (a learner's current parameters).  -> {checkpoint key: float32 device tensor}, views of ONE flat
    buffer in the order of GA3C_GRAD_LAYOUT (what an all-reduce would take).  The workspace of a call holds ~36 KB per row:
    where it would exceed max_work_bytes the rows are chunked in array order (ga3c_grad_chunk_rows) and accumulated.
    Deterministic: the same inputs and budget give the same bytes."""
    if dlogits is None and dvalue is None:
        raise ValueError("ga3c_grad: give dlogits, dvalue or both")
    device = x.device if (torch.is_tensor(x) and x.is_cuda) else torch.device("cuda:0")
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    xt = torch.as_tensor(x)
    if xt.dim() != 2 or xt.shape[1] < 1:
        raise ValueError("ga3c_grad: x must be [rows, width >= 1], got shape %s" % (tuple(xt.shape),))
    xt = xt.to(device=device, dtype=torch.float32).contiguous()
    rows = int(xt.shape[0])

    def up(t, shape, name, dtype=torch.float32):
        if t is None:
            return None
        t = torch.as_tensor(t)
        if t.dtype == torch.bool:
            t = t.to(torch.uint8) if not t.is_cuda else t.contiguous().view(torch.uint8)
        t = t.to(device=device, dtype=dtype).contiguous()
        if tuple(t.shape) != shape:
            raise ValueError("ga3c_grad: %s must have shape %s, got %s" % (name, shape, tuple(t.shape)))
        return t
    dl, dv = up(dlogits, (rows, 11), "dlogits"), up(dvalue, (rows,), "dvalue")
    lv = up(live, (rows,), "live", torch.uint8)
    net, vk, vb, keep = _grad_net(weights, device)
    if dv is not None and vk is None:
        raise ValueError("ga3c_grad: dvalue given, but these GA3C-CADRL weights have no logits_v_kernel / logits_v_bias")
    flat = torch.empty((ga3c_grad_offsets()[None][0],), dtype=torch.float32, device=device)
    _ga3c_grad_into(flat, net, vk, vb, xt, dl, dv, lv, max_work_bytes)
    del keep
    return ga3c_grad_views(flat)


def orca(pos, vel, pref, radius, max_speed, collab=0.5, time_horizon=5.0, time_step=0.1, max_neighbors=None,
         neighbor_dist=math.inf):
    """Batched replacement of rvo2.PyRVOSimulator.doStep() (RVOPolicy.py:93): float32 device tensors
    pos/vel/pref [E,N,2], radius/max_speed [E,N] -> new velocities [E,N,2]."""
    assert pos.is_cuda and pos.dtype == torch.float32
    E, N = pos.shape[:2]
    ts = [t.contiguous() for t in (pos, vel, pref, radius, max_speed)]
    out = torch.empty((E, N, 2), dtype=torch.float32, device=pos.device)
    st = C.c_void_p(torch.cuda.current_stream(pos.device).cuda_stream)
    nat.check(nat.lib().cagpu_orca(E, N, ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(),
                                   ts[4].data_ptr(), collab, time_horizon, time_step,
                                   N if max_neighbors is None else max_neighbors, neighbor_dist, out.data_ptr(), st))
    return out
