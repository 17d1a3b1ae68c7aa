"""CollisionAvoidanceEnv: drop-in for the reference's gym.Env (gym_collision_avoidance/envs/collision_avoidance_env.py)
backed by the batched HIP simulator.

    env = CollisionAvoidanceEnv()                 # num_envs = 1: the reference's behaviour and return types
    env.set_agents(agents); obs, _ = env.reset()
    obs, rewards, game_over, truncated, info = env.step({0: np.array([1.0, 0.5])})

    venv = CollisionAvoidanceEnv(num_envs=4096)   # batched: tensors on the device, auto-reset from a fixture table
    venv.set_fixture_suite(10, "RVO"); obs = venv.reset()[0]     # obs: float32 [E, N, 6+7K]
    obs, rewards, game_over, _, info = venv.step(None)

Everything `step` computes (policy queries, dynamics, collisions, rewards, sensors, done flags; reference lines
156-234, 284-327, 394-575) happens in ONE launch of the fused kernel (csrc/cagpu.hip).  The host only translates the
reference's call conventions: the actions dict, the nested observation dict, the info dicts keyed by agent.id.
Out of scope here: static maps and map-based sensors.
"""
import copy
import inspect

import numpy as np

from gym_collision_avoidance_amd import _native as nat
from gym_collision_avoidance_amd.envs import Config
from gym_collision_avoidance_amd.envs import test_cases as tc
from gym_collision_avoidance_amd.envs.Map import Map
from gym_collision_avoidance_amd.envs.policies import (ExternalPolicy, GA3CCADRLPolicy, InternalPolicy, LearningPolicy,
                                                       LearningPolicyGA3C, NonCooperativePolicy, RVOPolicy,
                                                       StaticPolicy)
from gym_collision_avoidance_amd.envs.spaces import Box, Dict, Env

_BUILTIN_POLICIES = (RVOPolicy, NonCooperativePolicy, StaticPolicy, ExternalPolicy, LearningPolicy, LearningPolicyGA3C,
                     GA3CCADRLPolicy)
_SORT = {"closest_first": nat.SORT_CLOSEST_FIRST, "closest_last": nat.SORT_CLOSEST_LAST,
         "time_to_impact": nat.SORT_TIME_TO_IMPACT}
_F64 = ("pos_x", "pos_y", "vel_x", "vel_y", "heading", "goal_x", "goal_y", "radius", "pref_speed", "time_remaining",
        "t", "slt", "ep_reward", "turning_dir")


class _HostAgent(object):
    """A mutable stand-in of an Agent for ONE call of a user Dynamics.step(action, dt): the attributes a dynamics model
    writes (agent.py:76-96) are plain values here, everything else reads through to the bound agent."""

    def __init__(self, agent):
        object.__setattr__(self, "_agent", agent)
        self.pos_global_frame = np.array(agent.pos_global_frame, dtype="float64")
        self.vel_global_frame = np.array(agent.vel_global_frame, dtype="float64")
        # (np.float64 scalars, what these attributes are in the reference once np.arctan2 / the dynamics have written them:
        # under numpy >= 2 a float32 action plus a PYTHON float would be evaluated in float32)
        self.heading_global_frame = np.float64(agent.heading_global_frame)
        self.speed_global_frame = np.float64(agent.speed_global_frame)
        self.delta_heading_global_frame = np.float64(agent.delta_heading_global_frame)
        self.turning_dir = np.float64(agent.turning_dir)

    def __getattr__(self, name):
        return getattr(object.__getattribute__(self, "_agent"), name)


class CollisionAvoidanceEnv(Env):
    metadata = {"render.modes": ["human", "rgb_array"], "video.frames_per_second": 30}

    LOOKAHEAD_MAX = 128                  # the default ring: as long as LOOKAHEAD_BYTES of outputs allow, at most this
    LOOKAHEAD_BYTES = 1 << 30            # (per ring; a refill allocates the next ring while the current one is being served)

    def __init__(self, num_envs=1, device="cuda:0", zero_copy=False, lookahead=None):
        """zero_copy (batched mode only): False -- step() / rollout() / reset() return FRESH tensors, like the
        reference's DummyVecEnv returns fresh arrays every step (vec_env.py:120-135): safe to append to a rollout
        buffer or to keep as prev_obs.  True -- they return the simulator's persistent device buffers, which the NEXT
        launch overwrites in place (no copy; for consumers that read the outputs before stepping again).

        lookahead (batched mode only): `step(None)` of a batch whose policies are all internal needs nothing from the
        host (the reference's run_episode passes None until the episode is over, env_utils.py:45-52), so the next
        `lookahead` steps are computed in ONE launch of the fused n-step kernel (cagpu_step_ex, CaStepEx.ring) and step(None)
        hands out one slot of that ring per call -- same results bit for bit, about half the time per step (a fused
        rollout never waits for the slowest workgroup of a step).  Whatever needs the simulator exactly at the step
        last handed out -- an action, a custom `dt`, reset(), reading an agent's state, episode_stats() -- rewinds
        transparently (core.BatchedSim.sync), and the ring adapts: after a rewind at slot t the next ring is t steps long
        (down to one launch per step for a caller who looks at the state every step), the first ring is 8 steps long
        and every ring used up doubles the next one.  `lookahead` = the longest ring; None: as many steps as
        LOOKAHEAD_BYTES (1 GiB) of output tensors hold, at most LOOKAHEAD_MAX (89 at 4096 x 10: 8.9 us per step against
        14.9 with one launch per step; a ring of 20: 9.8) -- unless zero_copy (whose contract is ONE persistent buffer):
        then 0 = off (one launch per step).  What step(None) returns under the ring are VIEWS of one slot of it: never
        written again, valid for as long as they are held, but ONE held observation keeps its whole ring (up to
        LOOKAHEAD_BYTES) allocated -- `.clone()` what goes into a long-lived buffer (a sparse replay sample, prev_obs
        across many steps), or pass a smaller `lookahead`."""
        self.id = 0
        self.num_envs = int(num_envs)
        self.device = device
        self.zero_copy = bool(zero_copy)
        self.lookahead = (0 if zero_copy else None) if lookahead is None else max(0, int(lookahead))
        self._la_on, self._la_dt_ok = False, True
        # GA3C-CADRL: also evaluate the network's value head with every policy query (set before reset();
        # core.BatchedSim.ga3c_value [E, N], GA3CCADRLPolicy.find_next_action_and_value)
        self.keep_ga3c_value = False
        self._initialize_rewards()
        self.num_agents = Config.MAX_NUM_AGENTS_IN_ENVIRONMENT
        self.dt_nominal = Config.DT
        self.collision_dist = Config.COLLISION_DIST
        self.getting_close_range = Config.GETTING_CLOSE_RANGE
        self.evaluate = Config.EVALUATE_MODE
        self.plot_episodes = False  # nothing plots by itself: render() / render_episode() / save_episode_plots() on request
        self.test_case_index = 0
        self.set_testcase(Config.TEST_CASE_FN, dict(Config.TEST_CASE_ARGS))
        # action bounds (collision_avoidance_env.py:86-109)
        self.max_heading_change = np.pi / 3
        self.min_heading_change = -self.max_heading_change
        self.min_speed, self.max_speed = 0.0, 1.0
        self.low_action = np.array([self.min_speed, self.min_heading_change])
        self.high_action = np.array([self.max_speed, self.max_heading_change])
        self.action_space = Box(self.low_action, self.high_action, dtype=np.float32)
        # Dict[agent -> Dict[state -> Box]] observation space + zero observation (:116-139)
        self.observation = {}
        self.observation_space = Dict({})
        for slot in range(Config.MAX_NUM_AGENTS_IN_ENVIRONMENT):
            self.observation[slot] = self._zero_obs()
            self.observation_space.spaces[slot] = Dict({
                s: Box(Config.STATE_INFO_DICT[s]["bounds"][0] * np.ones(Config.STATE_INFO_DICT[s]["size"]),
                       Config.STATE_INFO_DICT[s]["bounds"][1] * np.ones(Config.STATE_INFO_DICT[s]["size"]),
                       dtype=Config.STATE_INFO_DICT[s]["dtype"]) for s in Config.STATES_IN_OBS})
        self.agents = None
        self.default_agents = None
        self.prev_episode_agents = None
        self.static_map_filename = None
        self.map = None
        self._map_set = None      # set_static_map(..., per_env=True)
        self.maps = None          # ... one Map per entry of the set
        self._has_map_index = False   # ... `map_index`, the device int32 [E] map of every env, exists (a property)
        self._map_lazy = False    # sense_map_on_demand(): map sensors when asked for, not after every step
        self._map_stale = False   # ... and a step came since they were last computed
        self._map_ring = False    # sense_map_in_ring(): the ring keeps the map sensors of every slot it computes
        self.episode_step_number = None
        self.episode_number = 0
        self.plot_save_dir = None
        self.plot_policy_name = None
        self.perturbed_obs = None
        self._sim = None
        self._learning_info = None
        self._policy_pool = None  # a policy draw (set_fixture_suite(policy_distr=...)): dict(agents, bits, index)
        self._sim_key = None
        self._snap = None
        self._obs_np = None
        self._scan_np = None
        self._occ_np = None
        self._fixture = None
        self._all_agents = None
        self._host_policies, self._host_by_env, self._groups = [], None, []
        self._host_dynamics, self._hostdyn_by_env, self._ext_state = [], None, None
        self._traj_req = None     # record_trajectories(): dict(max_bytes) while recording is asked for
        self._final_req = False   # keep_final_observations()
        self._log_req = None      # log_episodes(): the capacity asked for (None: default) while the log is asked for
        self._met_req = None      # measure_episodes(): {"capacity", "keep_tape"} while the metrics are asked for

    # ------------------------------------------------------------------ configuration (reference setters)
    def set_agents(self, agents):
        """list[Agent] (used for every env) or, in batched mode, a list of num_envs such lists
        (collision_avoidance_env.py:335-343)."""
        self.default_agents = agents
        self._fixture = None

    def set_fixture_suite(self, num_agents, policies="RVO", agents_dynamics="unicycle", auto_reset=True,
                          env_id_offset=0, case_stride=None, table=None, generate=None, random_headings=None,
                          heading_seed=1, agents_sensors=("other_agents_states",), agent_setup=None,
                          policy_distr=None, policy_to_ensure=None, policy_seed=None):
        """Batched evaluation on the reference's 500-case suite (run_full_test_suite.py:54-130): env e starts on case
        (env_id_offset + e) % 500 and, with auto_reset, its k-th episode loads case (env_id_offset + e + k*stride) % 500
        on the device (DummyVecEnv semantics, vec_env.py:120-128).

        `table`: any float64 [C, num_agents, 6] case table (numpy or device tensor) instead of the reference's pickle.
        `generate`: dict(num_cases=..., seed=..., side_length=4.0 or (lo, hi), speed_bnds=(0.5, 2.0),
        radius_bnds=(0.2, 0.8)) -- the table is drawn ON THE DEVICE by cagpu_generate_cases (the reference's
        get_testcase_random, test_cases.py:212-253) when reset() builds the batch: training-mode resets then never touch
        the host.  With `num_agents=(lo, hi)` in the dict every case also draws its own agent count (the reference's
        num_agents=None; `side_length` may then be the reference's list of {"num_agents", "side_length"} range dicts):
        a ragged table whose short cases leave their last slots empty.
        With `stream=True` in the dict (and `window=8` instead of num_cases) there is no finite table at all: every
        on-device auto-reset loads a FRESH scenario of the same generator (core.BatchedSim.set_case_stream) -- episode k of
        the env with global id env_id_offset + e is scenario (seed, (id << 32) | k) -- which together with
        `random_headings` and `policy_distr` is the reference's default TEST_CASE_ARGS on the device.  Needs auto_reset;
        `case_stride` is not used (a stream's stride is the batch size).
        `random_headings` (default: `not Config.EVALUATE_MODE`, the reference's rule, test_cases.py:553-559): initial
        headings -- at reset() and at every on-device auto-reset -- are uniform in [-pi, pi) instead of pointing at the
        goal; drawn on the device from `heading_seed`.
        `agents_sensors`: the sensor names (test_cases.sensor_dict) of every agent, e.g. ("other_agents_states",
        "laserscan", "occupancy_grid") under Config.USE_STATIC_MAP.
        `agent_setup`: callable(agent), run by reset() on each Agent object it builds for the batch's slots -- what the
        reference's reset_env does after full_test_suite (policy.initialize_network(**spec), sensor.set_args(...),
        run_full_test_suite.py:70-80); every env of the batch runs what those agents describe.
        `policy_distr` (with `policies` a list of names -- the POOL -- and optionally `policy_to_ensure`, the reference's
        argument triple, test_cases.py cadrl_test_case_to_agents): every agent's policy is drawn anew from the pool at
        reset() and at EVERY on-device auto-reset (core.BatchedSim.set_policy_draw; `policy_seed`: the device draws' key,
        default: derived from heading_seed), and `policy_to_ensure` is written over one random agent of an episode
        nobody drew it in.  Pool entries must be built-in policies (a `kernel_id`); GA3C_CADRL with ONE checkpoint for
        the batch.  info["which_agents_learning"] of a batch is then the bool [E, N] mask of the step, env.agents[i].policy
        follows env 0's flag words, and step(None) runs one launch per step (no look-ahead ring).  A reset() starts every
        env at episode 0 again, so it replays the policy sequence of the first episodes."""
        draw = None
        if policy_distr is not None:
            if isinstance(policies, str) or len(policies) != len(policy_distr) or not 1 <= len(policies) <= 8:
                raise ValueError("policy_distr needs `policies` as a pool of 1..8 names, one probability per name")
            for name in policies:
                cls = tc.policy_dict.get(name)
                if cls is None or cls not in _BUILTIN_POLICIES or cls.kernel_id is None:
                    raise ValueError("policy %r cannot be drawn on the device: the pool of a policy draw holds built-in "
                                     "policies only (a user Python policy is queried on the host, agent by agent)" % (name,))
            if policy_to_ensure is not None and policy_to_ensure not in policies:
                raise ValueError("policy_to_ensure %r is not in the pool %r" % (policy_to_ensure, list(policies)))
            if not auto_reset:
                raise ValueError("policy_distr needs auto_reset: the policies are drawn at the on-device auto-resets")
            draw = dict(pool=list(policies), distr=[float(v) for v in policy_distr],
                        ensure=None if policy_to_ensure is None else list(policies).index(policy_to_ensure),
                        base=policy_to_ensure if policy_to_ensure is not None else policies[int(np.argmax(policy_distr))],
                        seed=policy_seed)
        elif policy_to_ensure is not None:
            raise ValueError("policy_to_ensure without policy_distr")
        if generate is not None and generate.get("stream"):
            if table is not None or "seed" not in generate or not auto_reset:
                raise ValueError("generate=dict(stream=True, ...) needs a seed and auto_reset, and takes no table")
            if "num_cases" in generate or int(generate.get("window", 8)) < 1:
                raise ValueError("generate=dict(stream=True, ...) takes window >= 1, not num_cases: a stream has no finite table")
        elif generate is not None:
            assert table is None and int(generate["num_cases"]) >= 1 and "seed" in generate
            table = None
        elif table is None:
            table = tc.fixture_table(num_agents)
        elif not hasattr(table, "data_ptr"):
            table = np.ascontiguousarray(table, dtype=np.float64)
        if table is not None:
            assert table.ndim == 3 and tuple(table.shape[1:]) == (num_agents, 6), table.shape
        self._fixture = dict(table=table, policies=policies, dynamics=agents_dynamics, auto_reset=auto_reset,
                             env_id_offset=env_id_offset, num_agents=num_agents, generate=generate,
                             sensors=tuple(agents_sensors), agent_setup=agent_setup, draw=draw,
                             heading_seed=(int(heading_seed) or 1) if (random_headings if random_headings is not None
                                                                      else not Config.EVALUATE_MODE) else 0,
                             case_stride=self.num_envs if case_stride is None else case_stride)
        self.default_agents = None

    def set_static_map(self, static_map, per_env=False, map_seed=None):
        """The static obstacles used when Config.USE_STATIC_MAP (collision_avoidance_env.py:369-392): the path of a
        binary image file like the reference takes (or a list of paths, one drawn per episode), OR the occupancy grid
        itself as a bool array [160, 160] (True = occupied; row = floor(80 - y/0.1), col = floor(80 + x/0.1),
        Map.py:26-32), or None for an empty map.

        per_env=True: a MAP SET -- `static_map` is a list of image paths, a list of bool grids or an array [M, 160, 160],
        and every env runs its own map: at every reset() each env draws one with np.random (as the reference draws its
        one map, :384-385), and every on-device auto-reset draws the env's next one (core.BatchedSim.set_map).  The
        device draws are keyed by a number that reset() takes from np.random (map_seed None: seeding numpy makes a run
        reproducible) or from a generator seeded with map_seed.  `maps` then holds one Map per entry, `map_index` the
        device int32 [E] map of every env, and `map` still the map of env 0.  Without per_env the behaviour is the
        single-map one above (a list of paths: one draw per reset for the whole batch)."""
        self._map_set = None
        if per_env:
            entries = list(static_map) if isinstance(static_map, (list, tuple)) else list(np.asarray(static_map))
            if not entries:
                raise ValueError("set_static_map(per_env=True) needs at least one map")
            maps = []
            for m in entries:
                if isinstance(m, str):
                    maps.append(Map(16, 16, 0.1, map_filename=m))
                    continue
                grid = np.asarray(m)
                if grid.shape != (160, 160):
                    raise ValueError("a map of the set has shape %s, expected (160, 160) (Map(16 m, 16 m, 0.1 m))" % (grid.shape,))
                maps.append(Map(16, 16, 0.1, static_map=grid.astype(bool)))
            self._map_set = dict(maps=maps, rng=None if map_seed is None else
                                 np.random.Generator(np.random.PCG64(int(map_seed) & 0xFFFFFFFFFFFFFFFF)))
            self.maps = maps
        self.static_map_filename = static_map

    def set_plot_save_dir(self, plot_save_dir):
        self.plot_save_dir = plot_save_dir  # the default directory of save_episode_plots(); step() / reset() never plot

    def set_perturbed_info(self, perturbed_obs):
        self.perturbed_obs = perturbed_obs

    def set_testcase(self, test_case_fn_str, test_case_args):
        """Function of test_cases.py called by reset() when no agents were set (:615-642)."""
        fn = getattr(tc, test_case_fn_str, None)
        assert callable(fn), "no test case function %r" % test_case_fn_str
        accepted = inspect.signature(fn).parameters
        self.test_case_fn = fn
        self.test_case_args = {k: v for k, v in test_case_args.items() if k in accepted}

    # ------------------------------------------------------------------ reset / step
    def reset(self):
        """-> (observation, {}) (:236-282)."""
        if self.evaluate and self.agents is not None:
            self.prev_episode_agents = copy.deepcopy(self.agents)
        if self.episode_step_number is not None and self.episode_step_number > 0:
            self.episode_number += 1
        self.episode_step_number = 0
        per_env = self._init_agents()
        self._upload(per_env)
        for slot in range(Config.MAX_NUM_AGENTS_IN_ENVIRONMENT):
            self.observation[slot] = self._zero_obs()
        return self._get_obs(), {}

    def step(self, actions, dt=None):
        """-> (next_observations, rewards, game_over, False, info) (:156-234).  `actions`: dict {agent index: action}
        for agents with an external policy (may be None / {} when every policy is internal), or, batched, an array
        [E, N, 2]."""
        if self._sim is None:
            raise RuntimeError("call reset() before step()")
        sim = self._sim
        if self._la_on and actions is None and (dt is None or float(dt) == self.dt_nominal):
            # every policy internal, nothing to do between two steps: one slot of the look-ahead ring (see __init__)
            if not self._la_dt_ok:   # (a step with another dt came before: it went through sync(), no ring is in flight)
                sim.p.dt = self.dt_nominal
                self._la_dt_ok = True
            self.episode_step_number += 1
            self._snap = self._obs_np = self._scan_np = None
            # (a ring runs map batches only with sense_map_on_demand, which computes the sensors when asked, or with
            #  sense_map_in_ring, whose hand-out has already made them those of this step)
            self._map_stale = not self._map_ring
            self._occ_np = None
            obs, rewards, done, over = sim.step_lookahead()
            info = {"which_agents_done": done, "which_agents_learning": self._learning_info}
            if sim._fin_on:
                return obs, rewards, over, self._final_items(info, over, *sim.lookahead_final()), info
            return obs, rewards, over, False, info
        if self._la_on:
            sim.sync()             # an action / another dt: the simulator has to stand at the step last handed out
        sim.p.dt = self.dt_nominal if dt is None else float(dt)
        self._la_dt_ok = sim.p.dt == self.dt_nominal
        self.episode_step_number += 1
        ext = self._external_actions(actions)
        sim.step(ext, ext_state=self._ext_state)
        self._snap, self._obs_np, self._scan_np = None, None, None
        if Config.USE_STATIC_MAP:
            if self._map_lazy:
                self._map_stale = True
            else:
                self._map_sensors()
        if Config.STORE_HISTORY and self.num_envs == 1:
            self._record_history()
        if self.num_envs > 1:
            # batched: 'laserscan' (if enabled) is the device tensor env.laserscan [E, N, 3, 512]
            # (.bool() copies; obs / rewards are cloned unless zero_copy: the next launch rewrites the buffers in place)
            # (the kernel writes 0 / 1 bytes: reinterpreted as bool without a conversion kernel)
            import torch
            if self._policy_pool is not None:   # a policy draw: who learns changes with every episode of every env
                learning = sim.learning_mask(still_learning=True)
            else:
                if self._learning_info is None:
                    self._learning_info = {a.id: a.policy.is_still_learning for a in self.agents}
                learning = self._learning_info
            info = {"which_agents_done": self._out(sim.done.view(torch.bool)), "which_agents_learning": learning}
            over = self._out(sim.game_over.view(torch.bool))
            truncated = False
            if sim._fin_on:
                truncated = self._final_items(info, over, self._out(sim.final_obs), sim.final_flags)
            return self._out(sim.obs), self._out(sim.rewards), over, truncated, info
        rewards = sim.rewards[0].double().cpu().numpy()
        done = sim.done[0].cpu().numpy().astype(bool)
        game_over = bool(sim.game_over[0].item())
        if Config.TRAIN_SINGLE_AGENT:
            rewards = rewards[0]
        info = {"which_agents_done": {a.id: bool(done[i]) for i, a in enumerate(self.agents)},
                "which_agents_learning": {a.id: a.policy.is_still_learning for a in self.agents}}
        return self._get_obs(), rewards, game_over, False, info

    # ------------------------------------------------------------------ internals
    def _init_agents(self):
        """-> list (per env) of list[Agent] (:345-367)."""
        E = self.num_envs
        if self._fixture is not None:
            f = self._fixture
            per_env = None  # built on the device from the table; only env 0 gets Agent views
            if f["table"] is None:  # drawn on the device (cagpu_generate_cases); the sim only needs the agent count here
                import torch
                from gym_collision_avoidance_amd import core
                gen = dict(f["generate"])
                scratch = core.BatchedSim(core.make_params(1, f["num_agents"]), device=self.device)
                if gen.pop("stream", False):   # a case stream: the table held here is episode 0 of THIS batch's envs, row e
                    gen.pop("window", None)
                    ids = (torch.arange(E, dtype=torch.int64) + int(f["env_id_offset"])) << 32
                    f["table"] = scratch.generate_cases_at(ids, gen.pop("seed"), **gen)
                else:
                    f["table"] = scratch.generate_cases(gen.pop("num_cases"), gen.pop("seed"), **gen)
                torch.cuda.synchronize()
            idx = 0 if self._streamed(f) else (f["env_id_offset"] + 0) % len(f["table"])
            row0 = f["table"][idx]
            row0 = row0.cpu().numpy() if hasattr(row0, "cpu") else row0
            row0 = row0[row0[:, 5] > 0]   # (a ragged table pads short cases with radius-0 rows: empty slots)
            # (a policy draw: the views start on one pool entry and follow env 0's flag words once they are bound)
            self.agents = tc.cadrl_test_case_to_agents(row0, policies=f["policies"] if f.get("draw") is None else f["draw"]["base"],
                                                       agents_dynamics=f["dynamics"], agents_sensors=f["sensors"])
            if f.get("agent_setup") is not None:
                for a in self.agents:
                    f["agent_setup"](a)
        else:
            if self.default_agents is None:
                if E > 1:
                    # batched: every env draws its own scenario -- with the reference's default TEST_CASE_ARGS also its own
                    # agent count (test_cases.py:224-227) and policy mix: a ragged batch (CA_ABSENT slots)
                    agents = [self.test_case_fn(**self.test_case_args) for _ in range(E)]
                else:
                    agents = self.test_case_fn(**self.test_case_args)
            else:
                agents = self.default_agents
            if len(agents) and isinstance(agents[0], (list, tuple)):
                assert len(agents) == E, "need one agent list per env"
                per_env = [list(a) for a in agents]
            else:
                per_env = [list(agents)] + [None] * (E - 1)
            self.agents = per_env[0]
        for group in ([self.agents] if per_env is None else [g for g in per_env if g is not None]):
            for agent in group:
                agent.max_heading_change = self.max_heading_change
                agent.max_speed = self.max_speed
        return per_env

    @staticmethod
    def _streamed(f):
        """this fixture draws a fresh scenario at every auto-reset (generate=dict(stream=True, ...))"""
        return bool(f.get("generate") and f["generate"].get("stream"))

    def _build_policy_pool(self, f, N):
        """the pool of a policy draw: per entry an agent list of N slots (its policy objects are what the env-0 views hand
        out, and what agent_setup initialises) and the entry's flag-word bits"""
        from gym_collision_avoidance_amd import core
        lists, bits = [], []
        for name in f["draw"]["pool"]:
            g = tc.cadrl_test_case_to_agents(np.ones((N, 6)), policies=name, agents_dynamics=f["dynamics"])
            if f.get("agent_setup") is not None:
                for a in g:
                    f["agent_setup"](a)
            p = g[0].policy
            if getattr(p, "needs_host", False) and self.num_envs == 1:
                raise ValueError("policy %r needs the host for a single env: it cannot be drawn on the device" % (name,))
            lists.append(g)
            bits.append(core.policy_word_bits(p.kernel_id, is_learning=p.str == "learning",
                                              still_learning=bool(p.is_still_learning)))
        index = {}
        for j, b in enumerate(bits):
            index.setdefault(b, j)
        return dict(agents=lists, bits=bits, index=index)

    def _drawn_policy(self, e, a, default):
        """the policy object of slot a as env e's flag word names it (a policy draw; Agent.policy of a bound view)"""
        pool = self._policy_pool
        j = pool["index"].get(int(self._snapshot()["flags"][e, a]) & nat.POLICY_DRAW_BITS)
        return default if j is None else pool["agents"][j][a]._policy

    def _plugin_ids(self, agents):
        pol, dyn, isl, stl = [], [], [], []
        self._host_policies = []   # (of the agent list this was last called for: _upload ends with env 0's)
        self._host_dynamics = []
        for i, a in enumerate(agents):
            p = a.policy
            custom_dyn = a.dynamics_model.kernel_id is None
            # (RVOPolicy's stochastic branches: on the host through find_next_action for a single env -- the reference's own
            # np.random calls --, in a batch as per-step device draws, core.BatchedSim.set_rvo_stochastic)
            builtin = type(p) in _BUILTIN_POLICIES and not (getattr(p, "needs_host", False) and self.num_envs == 1)
            if custom_dyn:
                # A user-defined Dynamics subclass (the plugin API of dynamics/Dynamics.py:15-41): its step(action, dt) runs
                # on the HOST each step with the action of that step, and the state it leaves is applied by the kernel at
                # the move (CaState.ext_state) -- so the agent's action has to be known on the host: its policy is queried
                # there too (every built-in policy but the GA3C-CADRL network is host-callable)
                if isinstance(p, GA3CCADRLPolicy):
                    raise NotImplementedError("a custom Dynamics subclass needs its agent's action on the host; "
                                              "GA3CCADRLPolicy has no host implementation (it runs in cagpu_ga3c)")
                self._host_dynamics.append(i)
            if builtin and not (custom_dyn and not isinstance(p, StaticPolicy)):
                pol.append(p.kernel_id)
            else:  # user plugin: queried on the host, handed to the kernel as a raw command
                pol.append(nat.POL_EXTERNAL)
                self._host_policies.append(i)
            dyn.append(nat.DYN_EXTERNAL if custom_dyn else a.dynamics_model.kernel_id)
            isl.append(p.str == "learning")
            stl.append(bool(p.is_still_learning))
        return pol, dyn, isl, stl

    def _sensor_args(self, groups):
        """-> (K, primary clip, primary sort id, {(clip, sort id): [(env or None, slot), ...]} of the other pairs).  Every
        agent owns its sensor object and its arguments in the reference (sensors/Sensor.py:19-23); the pair most agents use
        goes into CaParams, each further pair costs one cagpu_observe launch per step (core.BatchedSim.set_sensor_variants)."""
        K = Config.MAX_NUM_OTHER_AGENTS_OBSERVED
        per, count = {}, {}
        for e_, g in enumerate(groups):
            for a_, a in enumerate(g):
                pair = (K, Config.AGENT_SORTING_METHOD)
                for s in a.sensors:
                    if getattr(s, "name", None) == "other_agents_states":
                        pair = (min(int(s.max_num_other_agents_observed), K), s.agent_sorting_method)
                if pair[1] not in _SORT:
                    raise ValueError("unknown agent_sorting_method %r" % (pair[1],))
                per.setdefault(pair, []).append((e_, a_))
                count[pair] = count.get(pair, 0) + 1
        primary = max(count, key=lambda k_: (count[k_], k_ == (K, Config.AGENT_SORTING_METHOD))) if count else \
            (K, Config.AGENT_SORTING_METHOD)
        others = {(c_, _SORT[s_]): v for (c_, s_), v in per.items() if (c_, s_) != primary}
        return K, primary[0], _SORT[primary[1]], others

    def _upload(self, per_env):
        import torch
        from gym_collision_avoidance_amd import core
        E = self.num_envs
        agents0 = self.agents
        # N = agent SLOTS per env: the longest agent list of the batch (the table's width in fixture mode); an env with
        # fewer agents leaves its last slots empty (a case row with radius 0 -> CA_ABSENT, include/cagpu.h)
        if self._fixture is not None:
            tab = self._fixture["table"]
            N = int(tab.shape[1])
            ragged = bool((tab[..., 5] <= 0).any())
            if self._streamed(self._fixture):   # (later episodes draw their own count, whatever episode 0 drew)
                ragged = self._fixture["generate"].get("num_agents") is not None
        else:
            lens = [len(g) for g in per_env if g is not None]
            N, ragged = max(lens), len(set(lens)) > 1
        K, clip, sort, sensor_others = self._sensor_args([agents0] if (self._fixture is not None or per_env is None) else
                                                         [g if g is not None else agents0 for g in per_env])
        over = (nat.OVER_ALL_DONE if Config.EVALUATE_MODE else
                nat.OVER_AGENT0 if Config.TRAIN_SINGLE_AGENT else nat.OVER_LEARNING_DONE)
        key = (E, N, K, ragged)
        if self._sim is None or self._sim_key != key:
            params = core.make_params(E, N, max_obs=K, ragged=int(ragged))
            self._sim = core.BatchedSim(params, device=self.device)
            self._sim_key = key
        if self._traj_req is not None and not self._sim._traj_on:   # (asked for before reset(), or the batch was rebuilt)
            self._sim.record_trajectories(**self._traj_req)
        sim, p = self._sim, self._sim.p
        p.obs_clip, p.sort_mode, p.game_over_mode = clip, sort, over
        p.rvo_max_neighbors = Config.MAX_NUM_AGENTS_IN_ENVIRONMENT
        p.dt, p.near_goal_threshold, p.max_time_ratio = Config.DT, Config.NEAR_GOAL_THRESHOLD, Config.MAX_TIME_RATIO
        p.getting_close_range, p.sensing_horizon = Config.GETTING_CLOSE_RANGE, Config.SENSING_HORIZON
        p.reward_at_goal, p.reward_collision = self.reward_at_goal, self.reward_collision_with_agent
        p.reward_collision_wall, p.rvo_dt = self.reward_collision_with_wall, Config.DT   # RVOPolicy.py:13
        p.reward_time_step, p.reward_wiggly = self.reward_time_step, self.reward_wiggly_behavior
        p.wiggly_threshold = self.wiggly_behavior_threshold
        p.reward_min, p.reward_max = self.min_possible_reward, self.max_possible_reward
        p.rvo_time_horizon, p.rvo_collab_coeff = Config.RVO_TIME_HORIZON, Config.RVO_COLLAB_COEFF
        p.max_heading_change = self.max_heading_change
        variants = []
        for (c_, s_), where in sensor_others.items():   # (a fixture batch / one shared agent list: a slot's pair holds for every env)
            mask = np.zeros((E, N), dtype=bool)
            # (a fixture batch: ONE agent list describes the slots of every env; otherwise _sensor_args was given one list
            # per env -- env 0's for the entries that are None -- and `where` names (env, slot) pairs)
            shared = self._fixture is not None or per_env is None
            for e_, a_ in where:
                mask[slice(None) if shared else e_, a_] = True
            variants.append((mask, c_, s_))
        self._policy_pool = None
        if variants and self._fixture is not None and self._fixture.get("draw") is not None:
            raise ValueError("a policy draw with per-agent sensor arguments (set_sensor_variants): a slot's sensor pair "
                             "belongs to the agent object of that slot, which a draw replaces every episode")
        sim.set_sensor_variants(variants)
        if self._fixture is not None:
            f = self._fixture
            drw = f.get("draw")
            slots = agents0 if len(agents0) == N else tc.cadrl_test_case_to_agents(
                np.ones((N, 6)), policies=f["policies"] if drw is None else drw["base"],
                agents_dynamics=f["dynamics"])   # (plugin ids of EVERY slot)
            if slots is not agents0 and f.get("agent_setup") is not None:
                for a in slots:
                    f["agent_setup"](a)
            pol, dyn, isl, stl = self._plugin_ids(slots)
            if slots is not agents0:
                self._plugin_ids(agents0)  # leaves self._host_policies describing env 0
            sim.set_plugins(np.array(pol)[None], np.array(dyn)[None], np.array(isl)[None], np.array(stl)[None])
            if self._streamed(f):
                gen = {k_: v for k_, v in f["generate"].items() if k_ != "stream"}
                sim.set_case_stream(heading_seed=f["heading_seed"], env_id_offset=f["env_id_offset"], **gen)
            else:
                sim.set_fixture_table(f["table"] if f["auto_reset"] else None, env_id_offset=f["env_id_offset"],
                                      case_stride=f["case_stride"], heading_seed=f["heading_seed"])
            if drw is not None:
                self._policy_pool = self._build_policy_pool(f, N)
                seed = drw["seed"]
                if seed is None:   # (a key of its own, never the headings')
                    seed = ((int(f["heading_seed"]) or 1) * 0x9E3779B97F4A7C15 + 0x706F6C) & 0xFFFFFFFFFFFFFFFF
                sim.set_policy_draw(self._policy_pool["bits"], drw["distr"], ensure=drw["ensure"], seed=seed or 1)
            elif sim._draw is not None:
                sim.set_policy_draw(None)
            if self._final_req:    # (asked for before reset(), or the batch was rebuilt)
                self._check_final()
                sim.keep_final(True)
            if self._log_req is not None:    # (asked for before reset(), or the batch was rebuilt)
                self._check_log()
                if sim._log is None:
                    sim.log_episodes(capacity=self._log_capacity())
            if self._met_req is not None:    # (likewise)
                self._check_log("measure_episodes()")
                if sim._met is None:
                    sim.measure_episodes(capacity=self._met_capacity(), keep_tape=self._met_req["keep_tape"])
            idx = np.arange(E) if self._streamed(f) else (np.arange(E) + f["env_id_offset"]) % len(f["table"])
            if hasattr(f["table"], "data_ptr"):
                import torch
                idx = torch.as_tensor(idx, device=f["table"].device)
            heads = None
            if f["heading_seed"]:  # training mode: random initial headings (test_cases.py:558-559), drawn on the device
                import torch
                # a fresh stream per reset() call and per shard (seed, call count, global id of this shard's env 0):
                # successive resets and the shards of a multi-GPU batch draw different headings
                self._heading_resets = getattr(self, "_heading_resets", 0) + 1
                gen = torch.Generator(device=sim.device)
                gen.manual_seed((int(f["heading_seed"]) * 0x9E3779B1 + self._heading_resets * 0x85EBCA77 +
                                 int(f["env_id_offset"]) * 0xC2B2AE3D) & 0x7FFFFFFFFFFFFFFF)
                heads = (torch.rand((E, N), generator=gen, device=sim.device, dtype=torch.float64) * 2.0 - 1.0) * np.pi
            sim.reset(f["table"][idx], headings=heads)
            groups = [agents0]
            self._host_by_env, self._hostdyn_by_env = None, None
        else:
            if self._final_req:
                self._check_final()
            if self._log_req is not None:
                self._check_log()
            sim.set_fixture_table(None)
            groups = [g if g is not None else agents0 for g in per_env]
            ids, self._host_by_env, self._hostdyn_by_env = [], [], []
            for g in groups:
                ids.append(self._plugin_ids(g))
                self._host_by_env.append(list(self._host_policies))
                self._hostdyn_by_env.append(list(self._host_dynamics))
            self._plugin_ids(agents0)  # leaves self._host_policies describing env 0
            pad = lambda v, fill: list(v) + [fill] * (N - len(v))      # (empty slots: ids never read, rows with radius 0)
            sim.set_plugins(*[np.array([pad(x[k], 0) for x in ids]) for k in range(4)])
            rows = [[a._case_row() for a in g] for g in groups]
            cases = np.array([pad([r[0] for r in g], [0.0] * 6) for g in rows], dtype=np.float64)
            heads = np.array([pad([r[1] for r in g], 0.0) for g in rows], dtype=np.float64)
            sim.reset(cases, headings=heads)
        self._groups = groups
        if E > 1 and self._fixture is not None and (self._host_policies or self._host_dynamics):
            # a fixture batch is built on the device from the case table: only env 0 has Agent objects to call a Python
            # policy with.  With explicit agent lists (set_agents([[...], ...]) / the default test-case function) a user
            # policy of ANY env is queried on the host each step: the slow per-agent fallback
            raise NotImplementedError("user-defined Python policies in a fixture-suite batch: hand the batch its agents "
                                      "with set_agents([agents of env 0, agents of env 1, ...]) instead")
        if E > 1 and any(g is None for g in (per_env or [])) and (self._host_policies or self._host_dynamics):
            raise NotImplementedError("user-defined Python policies in a batch need one agent list per env (their policy "
                                      "objects carry per-agent state): set_agents([[...] for each env])")
        if E > 1:   # RVOPolicy.py:77-90, :118-119 for the whole batch
            noise = np.zeros((E, N), dtype=bool)
            for e_, g_ in enumerate(groups):
                for a_, agent in enumerate(g_):
                    if isinstance(agent.policy, RVOPolicy) and agent.policy.heading_noise:
                        noise[slice(None) if self._fixture is not None else e_, a_] = True
            on_device = getattr(self, "_rvo_device_seed", None)
            if on_device is None and sim._rd is not None:
                sim.set_rvo_draw(0)   # (switched off since the last upload)
            if on_device is not None:   # draw_rvo_on_device(): the step kernels draw (core.BatchedSim.set_rvo_draw)
                sim.set_rvo_stochastic()
                sim.set_rvo_draw(on_device, heading_noise=noise if noise.any() else None, collab_coeff=Config.RVO_COLLAB_COEFF,
                                 anti_collab_t=Config.RVO_ANTI_COLLAB_T)
            elif noise.any() or Config.RVO_COLLAB_COEFF < 0:
                # (the seed comes out of numpy's global stream, like the reference's own draws -- only when a stochastic
                # branch is on: a deterministic batch must not shift the stream the scenario builders draw from)
                self._rvo_seed = getattr(self, "_rvo_seed", 0) + 1
                sim.set_rvo_stochastic(heading_noise=noise if noise.any() else None, collab_coeff=Config.RVO_COLLAB_COEFF,
                                       anti_collab_t=Config.RVO_ANTI_COLLAB_T,
                                       seed=int(np.random.randint(1 << 31)) + self._rvo_seed)
            else:
                sim.set_rvo_stochastic()
        else:
            sim.set_rvo_stochastic()
        nets = [a.policy for g in groups for a in g if isinstance(a.policy, GA3CCADRLPolicy)]
        if self._policy_pool is not None:   # (every pool entry's policy objects: any slot may draw the network)
            nets = [a.policy for g in self._policy_pool["agents"] for a in g if isinstance(a.policy, GA3CCADRLPolicy)]
            if len({n.weights_path for n in nets}) > 1:
                raise ValueError("a policy draw with per-agent GA3C-CADRL checkpoints: a drawn slot has no agent object "
                                 "of its own to carry one -- one checkpoint for the batch")
        if nets:  # GA3CCADRLPolicy.initialize_network must have run (the reference has no session otherwise)
            paths = {n.weights_path for n in nets}
            if None in paths:
                raise RuntimeError("a GA3CCADRLPolicy agent was not initialised: call agent.policy.initialize_network()")
            order = sorted(paths)
            for n in nets:   # the host-callable query of these policy objects runs where the env runs
                n.device = n.nn.device = str(sim.device)
            keep_v = bool(self.keep_ga3c_value)
            if getattr(sim, "_net_paths", None) != order or keep_v != (sim.ga3c_value is not None):
                sim._nets.clear()
                sim._net = None
                sim.ga3c_value = None
                for idx, path in enumerate(order):
                    sim.load_ga3c(next(n.weights for n in nets if n.weights_path == path), index=idx, keep_value=keep_v)
                sim._net_paths = order
            if len(order) > 1:
                # agents of one batch on different checkpoints (every agent owns its policy object and session in the
                # reference): one cagpu_ga3c launch per checkpoint over its own agents (CaNet.agent_net / net_index)
                assign = np.zeros((E, N), dtype=np.int32)
                for e_, g_ in enumerate(groups):    # (a fixture batch: one agent list describes the slots of every env)
                    for a_, agent in enumerate(g_):
                        if isinstance(agent.policy, GA3CCADRLPolicy):
                            assign[slice(None) if self._fixture is not None else e_, a_] = order.index(agent.policy.weights_path)
                sim.set_ga3c_assignment(assign)
            else:
                sim.set_ga3c_assignment(None)
            self._apply_ga3c_sampling(sim)
        for e, g in enumerate(groups if self._fixture is None else [agents0]):
            if per_env is None or per_env[e] is not None or e == 0:
                for a_idx, agent in enumerate(g):
                    agent._bind(self, e, a_idx)
        self._snap, self._obs_np, self._scan_np = None, None, None
        self._learning_info = None
        # batched, not zero_copy: every step writes into newly allocated output tensors, so what step() returns is the
        # caller's to keep without a copy kernel -- unless something of ours reads the observation back later (the
        # GA3C-CADRL query, a host-side policy): then the outputs are copies and ours stay private
        host_any = (bool(self._host_policies) or bool(self._host_by_env and any(self._host_by_env)) or
                    bool(self._host_dynamics) or bool(self._hostdyn_by_env and any(self._hostdyn_by_env)))
        sim.fresh_outputs = E > 1 and not self.zero_copy and not nets and not host_any
        # the look-ahead ring (see __init__): every policy answered inside the step kernel, nothing between two steps
        ring = self._ring_len(sim)
        # (a static map: the env scans after every step, so its ring stays off -- unless sense_map_on_demand() defers the scans)
        self._la_but_map = bool(self._policy_pool is None and   # (a draw: the learning mask of every step is read from the state)
                                E > 1 and ring > 0 and not nets and not host_any and
                                not any(a.policy.is_external for g in groups for a in g) and sim.lookahead_ok())
        self._la_on = self._la_but_map and (not Config.USE_STATIC_MAP or self._map_lazy or self._map_ring)
        self._enable_ring(sim)
        self._la_dt_ok = sim.p.dt == self.dt_nominal
        if self._la_on:
            self._learning_info = {a.id: a.policy.is_still_learning for a in self.agents}
        if Config.USE_STATIC_MAP and self._map_set is not None:
            # a map set: every env draws its own map (collision_avoidance_env.py:384-385, once per env), the auto-resets
            # draw on the device under a key taken here
            maps = self._map_set["maps"]
            idx = np.random.randint(len(maps), size=E)
            rng = self._map_set["rng"]
            key = int(rng.integers(1, 1 << 64, dtype=np.uint64)) if rng is not None else \
                int(np.random.randint(1, np.iinfo(np.int64).max, dtype=np.int64))
            sim.set_map(np.stack([m.static_map for m in maps]), num_beams=Config.LASERSCAN_LENGTH,
                        num_to_store=Config.LASERSCAN_NUM_PAST, env_map=idx)
            sim.set_map_seed(key)
            self.map = maps[int(idx[0])]
            self._has_map_index = True
            self._map_sensors(groups)
            self._enable_ring(sim)    # (sense_map_in_ring: the ring's sensor slots need the map just attached)
        elif Config.USE_STATIC_MAP:  # collision_avoidance_env.py:273-274, :378-392: Map(16 m, 16 m, 0.1 m)
            sm = self.static_map_filename
            if isinstance(sm, list) and sm and isinstance(sm[0], str):
                sm = np.random.choice(sm)  # collision_avoidance_env.py:384-385
            self.map = Map(16, 16, 0.1, map_filename=sm) if isinstance(sm, str) else Map(16, 16, 0.1, static_map=sm)
            sim.set_map(self.map.static_map if self.map.static_map.any() else None, num_beams=Config.LASERSCAN_LENGTH,
                        num_to_store=Config.LASERSCAN_NUM_PAST)
            self._map_sensors(groups)
            self._enable_ring(sim)
        if Config.STORE_HISTORY and E == 1:
            self._record_history(initial=True)

    def _external_actions(self, actions):
        """reference actions dict / batched array -> float64 [E, N, 2] (or None when nobody needs one).  Agents whose
        policy is a user-defined Python class (InternalPolicy / ExternalPolicy subclasses: the reference's plugin API,
        InternalPolicy.py:12-23, ExternalPolicy.py:14-16) are queried HERE, on the host, agent by agent and env by env,
        with the reference's arguments -- the slow fallback; built-in policies never pass through this loop."""
        E, N = self.num_envs, self._sim.N
        if self._policy_pool is not None and not isinstance(actions, dict):
            return actions   # (a policy draw: [E, N, 2] for whoever is external in this episode, or None; no host policies)
        host_any = (bool(self._host_policies) or bool(self._host_by_env and any(self._host_by_env)) or
                    bool(self._host_dynamics) or bool(self._hostdyn_by_env and any(self._hostdyn_by_env)))
        if actions is not None and not isinstance(actions, dict) and not host_any:
            return actions  # already [E, N, 2]
        need = [i for i, a in enumerate(self.agents) if a.policy.is_external]
        if not need and not host_any:
            return None
        batched_in = actions is not None and not isinstance(actions, dict)
        if batched_in:
            src = actions.detach().cpu().numpy() if hasattr(actions, "detach") else np.asarray(actions)
            ext = np.array(src, dtype=np.float64).reshape(E, N, 2)
            actions = {}
        else:
            ext = np.zeros((E, N, 2), dtype=np.float64)
            actions = actions or {}
        groups = self._groups if (self._host_by_env is not None and len(self._groups) == E) else [self.agents]
        host_by_env = self._host_by_env if self._host_by_env is not None else [self._host_policies]
        for e, group in enumerate(groups):
            for i in host_by_env[e] if e < len(host_by_env) else ():
                agent = group[i]
                if agent.is_done:  # collision_avoidance_env.py:311
                    continue
                p = agent.policy
                if isinstance(p, ExternalPolicy):
                    raw = src[e, i] if batched_in else actions[i]
                    ext[e, i] = np.asarray(p.external_action_to_action(agent, raw), dtype=np.float64)
                elif isinstance(p, InternalPolicy):
                    ext[e, i] = np.asarray(p.find_next_action(self._obs_dicts(e)[i], group, i), dtype=np.float64)   # (:319-323)
        self._ext_state = None
        dyn_by_env = self._hostdyn_by_env if self._hostdyn_by_env is not None else [self._host_dynamics]
        if any(dyn_by_env):
            # user Dynamics subclasses (Agent.take_action, agent.py:199-220): behind the done gate, step(action, dt) with
            # the float32 action of this step on a mutable stand-in of the agent; the state it leaves travels to the
            # kernel, which applies it at the move (CaState.ext_state)
            dt = float(self._sim.p.dt)
            est = np.full((E, N, 5), np.nan, dtype=np.float64)
            for e, group in enumerate(groups):
                for i in dyn_by_env[e] if e < len(dyn_by_env) else ():
                    agent = group[i]
                    if agent.is_at_goal or agent.ran_out_of_time or agent.in_collision:
                        continue
                    proxy = _HostAgent(agent)
                    dm = agent.dynamics_model
                    dm.agent = proxy
                    try:
                        dm.step(ext[e, i].astype(np.float32), dt)   # (`all_actions` is a float32 array, env.py:305-307)
                    finally:
                        dm.agent = agent
                    est[e, i] = [proxy.pos_global_frame[0], proxy.pos_global_frame[1], proxy.vel_global_frame[0],
                                 proxy.vel_global_frame[1], proxy.heading_global_frame]
            self._ext_state = est
        if not batched_in:
            for i, agent in enumerate(self.agents):
                if i in self._host_policies:
                    continue
                if agent.policy.is_external and i in actions:
                    a = np.asarray(actions[i], dtype=np.float64)
                    if a.ndim == 0:          # LearningPolicyGA3C: a discrete index
                        ext[:, i, 0] = a
                    else:
                        ext[:, i, :a.shape[-1]] = a
        return ext

    def _obs_dicts(self, e):
        """the reference-shaped observation {agent index: {state: array}} of env e (what a policy's find_next_action
        receives, collision_avoidance_env.py:319-323), from the host copy of the observation tensor"""
        if e == 0 and self.num_envs == 1:
            return self.observation
        cache = getattr(self, "_obs_dict_cache", None)
        if cache is None or cache[0] is not self._obs_host():
            cache = (self._obs_host(), {})
            self._obs_dict_cache = cache
        if e not in cache[1]:
            cache[1][e] = {i: self._obs_row_dict(cache[0][e, i], e, i) for i in range(len(self._groups[e]))}
        return cache[1][e]

    def _snapshot(self):
        """host copy of the device state, refreshed at most once per step"""
        if self._snap is None:
            st = self._sim.state
            snap = {n: st[n].cpu().numpy() for n in _F64 + ("flags", "step_num", "last_action", "reset_count")}
            self._snap = snap
        return self._snap

    def _obs_host(self):
        if self._obs_np is None:
            self._obs_np = self._sim.obs.cpu().numpy()
        return self._obs_np

    def _scan_host(self):
        if self._scan_np is None:
            self._map_fresh()
            self._scan_np = self._sim.scan.cpu().numpy()
        return self._scan_np

    def _map_fresh(self):
        """sense_map_on_demand: the map sensors of the step last handed out, computed now if a step came since"""
        if self._map_stale and self._sim is not None and Config.USE_STATIC_MAP:
            self._map_sensors()

    def sense_map_on_demand(self, on=True):
        """Opt-in for Config.USE_STATIC_MAP batches: compute the map sensors (laser scan, occupancy windows) when
        `env.laserscan`, `env.occupancy_grid` or an observation dict asks for them, not after every step.  The scan
        history (LASERSCAN_NUM_PAST rows) then counts those requests instead of the steps.  With every policy internal
        nothing is left to do between two steps, so step(None) is served from the look-ahead ring (see __init__) -- walls
        and map draws are those of single steps; a request rewinds the ring to the step last handed out, and so does reading
        `env.map_index` (the maps of the step last handed out, not those the ring has drawn ahead).  Off by default:
        the env scans after every step and its ring stays off under a static map."""
        on = bool(on)
        if on == self._map_lazy:
            return
        self._map_lazy = on
        if self._sim is None or not Config.USE_STATIC_MAP:
            return
        sim = self._sim
        sim.sync()
        if not on:
            self._map_fresh()
        self._la_on = self._la_but_map and (on or self._map_ring)
        self._enable_ring(sim)
        if self._la_on:
            self._learning_info = {a.id: a.policy.is_still_learning for a in self.agents}

    def sense_map_in_ring(self, on=True):
        """Opt-in for Config.USE_STATIC_MAP batches whose policies are all internal: step(None) is served from the
        look-ahead ring AND `env.laserscan`, `env.occupancy_grid` and the observation dict show the true sensors of every
        step -- the scan history counts steps, not requests (sense_map_on_demand's does).  A refill computes the laser
        index rows of all its slots behind the step launch (core.BatchedSim.enable_lookahead(map_sensors=True)) and every
        step(None) expands the slot it hands out, without a synchronisation.  rollout(n, actions=..., keep_steps=True) then
        returns every step's sensors too: info["laserscan"] [n, E, N, LASERSCAN_NUM_PAST, LASERSCAN_LENGTH] and, where an
        agent lists the OccupancyGridSensor, info["occupancy_grid"] [n, E, N, H, W].  Off by default."""
        on = bool(on)
        if on == self._map_ring:
            return
        self._map_ring = on
        if self._sim is None or not Config.USE_STATIC_MAP:
            return
        sim = self._sim
        sim.sync()
        self._map_fresh()
        self._la_on = self._la_but_map and (on or self._map_lazy)
        self._enable_ring(sim)
        if self._la_on:
            self._learning_info = {a.id: a.policy.is_still_learning for a in self.agents}

    def _enable_ring(self, sim):
        """the look-ahead ring as the switches stand: off, plain, or keeping the map sensors of its slots"""
        ms = bool(self._la_on and self._map_ring and Config.USE_STATIC_MAP and sim._map is not None)
        sim.enable_lookahead(self._ring_len(sim) if self._la_on else 0, fresh=not self.zero_copy, adaptive=True, map_sensors=ms)

    def _map_sensors(self, groups=None):
        """the map sensors of the current state: the laser scan, and the OccupancyGridSensor windows where some agent of
        the batch lists that sensor.  `groups` (the reset upload, right after set_map()): the batch's agent lists, from
        which the window size is taken -- the windows are ONE tensor [E, N, H, W], so every agent must agree on it."""
        sim = self._sim
        if groups is not None:
            from .sensors.OccupancyGridSensor import OccupancyGridSensor
            sizes = {(float(s.x_width), float(s.y_width)) for g in groups for a in g for s in a.sensors
                     if isinstance(s, OccupancyGridSensor)}
            if len(sizes) > 1:
                raise ValueError("OccupancyGridSensor: the agents of a batch must agree on x_width / y_width "
                                 "(one window tensor per batch), got %s" % sorted(sizes))
            if sizes:
                (xw, yw), = sizes
                sim.set_occupancy_grid(x_width=xw, y_width=yw)
        sim.laserscan()
        self._occ_np = None
        self._scan_np = None
        if sim.occ is not None:
            sim.occupancy_grid()
        self._map_stale = False

    def _occ_host(self):
        self._map_fresh()
        if self._occ_np is None:
            self._occ_np = self._sim.occ.cpu().numpy()
        return self._occ_np

    def _write_agent(self, e, a, **fields):
        for name, v in fields.items():
            self._sim.state[name][e, a] = float(v)   # (`state` rewinds a look-ahead ring to the step last handed out)
        self._sim.invalidate_plan()   # (a host write to the state: the pipelined policy query is forgotten)
        self._snap = None

    def _out(self, t):
        """a device output as handed to the caller: the simulator's buffer itself -- zero_copy, or a batch whose every
        step writes into newly allocated tensors (core.BatchedSim.fresh_outputs) -- or a copy"""
        return t if (self.zero_copy or self._sim.fresh_outputs) else t.clone()

    def _zero_obs(self):
        return {s: np.zeros(Config.STATE_INFO_DICT[s]["size"], dtype=Config.STATE_INFO_DICT[s]["dtype"])
                for s in Config.STATES_IN_OBS}

    def _get_obs(self):
        """Batched: the device tensor [E, N, 6+7K].  Single env: the reference's nested dict
        {agent index: {state: array}} (:555-575); slots beyond the agents in the scene keep their zeros."""
        if self.num_envs > 1:
            return self._out(self._sim.obs)
        row = self._obs_host()[0]
        for i in range(len(self.agents)):
            self.observation[i] = self._obs_row_dict(row[i], 0, i)
        return self.observation

    def _obs_row_dict(self, r, e, i):
        """one agent's row of the observation tensor as the reference's {state: array} dict (Config.STATES_IN_OBS)"""
        K = Config.MAX_NUM_OTHER_AGENTS_OBSERVED
        cols = {"is_learning": 0, "num_other_agents": 1, "dist_to_goal": 2, "heading_ego_frame": 3, "pref_speed": 4,
                "radius": 5}
        obs = {}
        for s in Config.STATES_IN_OBS:
            if s == "other_agents_states":
                obs[s] = r[6:6 + 7 * K].astype(np.float64).reshape(K, 7)
            elif s == "laserscan":
                obs[s] = self._scan_host()[e, i].astype(np.float64)
            elif s == "occupancy_grid":
                if self._sim.occ is None:
                    raise RuntimeError("'occupancy_grid' is in Config.STATES_IN_OBS but no agent lists OccupancyGridSensor")
                obs[s] = self._occ_host()[e, i].copy()
            elif s == "other_agent_states":
                obs[s] = r[6:13].astype(np.float64)
            elif s == "is_learning":
                obs[s] = np.array(bool(r[0]))
            elif s == "num_other_agents":
                obs[s] = np.array(int(r[1]))
            elif s in cols:
                obs[s] = np.array(np.float64(r[cols[s]]))
            else:
                raise NotImplementedError("state %r is not produced by the batched simulator" % s)
        return obs

    def _record_history(self, initial=False):
        """Config.STORE_HISTORY: append [t, px, py, gx, gy, radius, pref_speed, vx, vy, speed, heading] for agents
        that moved this step (agent.py:257-289)."""
        if initial:
            return
        for a in self.agents:
            if len(a._history) < a.step_num:
                g, _ = a.to_vector()
                g[0] = a.t - self.dt_nominal  # the reference logs t before incrementing it (agent.py:227-236)
                a._history.append(g)

    def _initialize_rewards(self):
        self.reward_at_goal = Config.REWARD_AT_GOAL
        self.reward_collision_with_agent = Config.REWARD_COLLISION_WITH_AGENT
        self.reward_collision_with_wall = Config.REWARD_COLLISION_WITH_WALL
        self.reward_getting_close = Config.REWARD_GETTING_CLOSE
        self.reward_entered_norm_zone = Config.REWARD_ENTERED_NORM_ZONE
        self.reward_time_step = Config.REWARD_TIME_STEP
        self.reward_wiggly_behavior = Config.REWARD_WIGGLY_BEHAVIOR
        self.wiggly_behavior_threshold = Config.WIGGLY_BEHAVIOR_THRESHOLD
        self.possible_reward_values = np.array([self.reward_at_goal, self.reward_collision_with_agent,
                                                self.reward_time_step, self.reward_collision_with_wall,
                                                self.reward_wiggly_behavior])
        self.min_possible_reward = float(np.min(self.possible_reward_values))
        self.max_possible_reward = float(np.max(self.possible_reward_values))

    @property
    def map_index(self):
        """device int32 [E]: the map of every env of a map set (set_static_map(per_env=True); None otherwise), at the step
        last handed out -- with the look-ahead ring on (sense_map_on_demand) reading it rewinds a ring that has run ahead,
        whose auto-resets have already drawn the maps of episodes not handed out yet"""
        return self._sim.env_map if (self._has_map_index and self._sim is not None) else None

    @property
    def laserscan(self):
        """float32 device tensor [E, N, LASERSCAN_NUM_PAST, LASERSCAN_LENGTH] (Config.USE_STATIC_MAP only)."""
        if self._sim is None:
            return None
        self._map_fresh()
        return self._sim.scan

    @property
    def occupancy_grid(self):
        """bool device tensor [E, N, H, W]: every agent's OccupancyGridSensor window of the current state (H x W =
        y_width x x_width in map cells); None unless some agent of the batch lists the sensor."""
        if self._sim is None:
            return None
        self._map_fresh()
        return self._sim.occ

    # ------------------------------------------------------------------ trajectories (core.BatchedSim.record_trajectories)
    def record_trajectories(self, on=True, max_bytes=None):
        """Record every agent's trajectory ON THE DEVICE, inside the step kernels (the batched form of the reference's
        Config.STORE_HISTORY log, agent.py:257-289): off by default whatever Config.STORE_HISTORY says -- 96 bytes per
        agent and step.  May be called before or after reset() and survives reset().  max_bytes: the tape's budget
        (default 1 GiB); the step that would exceed it raises CagpuError and takes no step."""
        if not on:
            self._traj_req = None
            if self._sim is not None:
                self._sim.stop_recording()
            return
        self._traj_req = {} if max_bytes is None else {"max_bytes": int(max_bytes)}
        if self._sim is not None:
            self._sim.record_trajectories(**self._traj_req)

    def trajectories(self):
        """the tape as device tensors: {"rows": float64 [T, E, N, 12], "episode": int32 [T, E], "epoch": int32 [T, E]}
        (core.BatchedSim.trajectories); T = the steps taken since recording started or was last cleared"""
        if self._sim is None:
            raise RuntimeError("call reset() before trajectories()")
        return self._sim.trajectories()

    def clear_trajectories(self):
        if self._sim is not None:
            self._sim.clear_trajectories()
        self._snap = None

    def episode_histories(self, env_index=0):
        """The recorded episodes of one env (trajectory.episodes): a list over episodes of lists over agent slots of
        [len, 11] arrays -- each the reference's `agent.global_state_history[:step_num]` of that episode.  Only that
        env's part of the tape is copied to the host."""
        from gym_collision_avoidance_amd import trajectory
        e = int(env_index)
        tp = self.trajectories()
        return trajectory.episodes(tp["rows"][:, e:e + 1], tp["episode"][:, e:e + 1], 0, epoch=tp["epoch"][:, e:e + 1])

    def _tape_history(self, e, a):
        """the CURRENT episode's [step_num, 11] log of agent (e, a) from the device tape, or None where the tape is not
        the log's source (recording off; a single env under Config.STORE_HISTORY keeps its host-side log)"""
        sim = self._sim
        if sim is None or not sim._traj_on or (Config.STORE_HISTORY and self.num_envs == 1):
            return None
        snap = self._snapshot()
        cache = snap.setdefault("_hist", {})
        if e not in cache:
            tp = sim.trajectories()
            cur = None
            if tp["rows"].shape[0]:
                # the tape's last episode of this env is the current one unless a reset (on the device or from the host)
                # came after its last recorded step: then the current episode has no row yet
                same = (int(tp["episode"][-1, e]) == int(snap["reset_count"][e]) and
                        int(tp["epoch"][-1, e]) == int(sim._traj["epoch"][e]))
                if same:
                    cur = self.episode_histories(e)[-1]
            cache[e] = cur if cur is not None else [np.zeros((0, 11)) for _ in range(sim.N)]
        return cache[e][a]

    # ------------------------------------------------------------------ frames (core.BatchedSim.render_frames)
    def _render_defaults(self, kw):
        kw.setdefault("limits", Config.PLT_LIMITS)
        kw.setdefault("circles_along_traj", bool(Config.PLOT_CIRCLES_ALONG_TRAJ))
        return kw

    def render(self, mode="rgb_array", env_ids=None, **kw):
        """Frames of the episodes, rasterised on the device (core.BatchedSim.render_frames: the reference's
        visualize.plot_episode minus text and axes; keywords size=(H, W), limits, episode="current" | "last", upto,
        circles_along_traj, draw_map -- limits / circles_along_traj default to Config.PLT_LIMITS /
        PLOT_CIRCLES_ALONG_TRAJ).  num_envs == 1: the uint8 numpy array [H, W, 3] Gym's "rgb_array" mode returns; batched:
        the uint8 device tensor [S, H, W, 3] of `env_ids` (default: all envs).  Trajectories appear where the tape
        records them (record_trajectories()); without it a frame shows the current state."""
        if mode != "rgb_array":
            raise NotImplementedError("render(mode=%r): there is no window to draw into here -- use mode='rgb_array' (frames "
                                      "as arrays) or save_episode_plots() (PNG / GIF files)" % (mode,))
        if self._sim is None:
            raise RuntimeError("call reset() before render()")
        frames = self._sim.render_frames(env_ids, **self._render_defaults(kw))
        return frames[0].cpu().numpy() if self.num_envs == 1 else frames

    def render_episode(self, env_id=0, episode="last", every=1, **kw):
        """the animation frames of one episode of one env, uint8 device tensor [F, H, W, 3], from one launch
        (core.BatchedSim.render_episode)"""
        if self._sim is None:
            raise RuntimeError("call reset() before render_episode()")
        return self._sim.render_episode(env_id, episode=episode, every=every, **self._render_defaults(kw))

    def save_episode_plots(self, env_ids=None, directory=None, animate=False, episode="current", **kw):
        """Write the episode plots of `env_ids` (default: all) as files, named like the reference's
        (visualize.py:27-38, :138-149): `{test_case:03d}_{policy}_{num_agents}agents.png` in `directory` (default: the one
        given to set_plot_save_dir), a copy under `collisions/` where some agent of the env is in collision, and with
        `animate` a GIF of render_episode()'s frames under `animations/`.  test_case = test_case_index (+ the env's index
        in a batch), policy = plot_policy_name or the first agent's policy name.  The collision test reads the CURRENT
        flag words: use it with episode="current" before the env is reset (episode="last" plots the finished episode
        but cannot know how it ended).  Encoded by PIL.  Returns the list of PNG paths.  Nothing plots unless this is
        called: Config.SAVE_EPISODE_PLOTS / ANIMATE_EPISODES have no effect on step() / reset()."""
        import os
        from gym_collision_avoidance_amd import render as rd
        if self._sim is None:
            raise RuntimeError("call reset() before save_episode_plots()")
        directory = self.plot_save_dir if directory is None else directory
        if directory is None:
            raise ValueError("save_episode_plots: no directory given and none set with set_plot_save_dir()")
        ids = list(range(self.num_envs)) if env_ids is None else [int(e) for e in np.asarray(env_ids).reshape(-1)]
        kw = self._render_defaults(kw)
        frames = self._sim.render_frames(ids, episode=episode, **kw).cpu().numpy()
        flags = self._sim.state["flags"][ids].cpu().numpy()
        policy = self.plot_policy_name or self.agents[0].policy.str
        paths = []
        for j, e in enumerate(ids):
            present = (flags[j] & nat.ABSENT) == 0
            name = "%03d_%s_%dagents" % (self.test_case_index + e, policy, int(present.sum()))
            paths.append(rd.save_frames(os.path.join(directory, name + ".png"), frames[j]))
            if ((flags[j] & nat.IN_COLLISION) != 0)[present].any():
                rd.save_frames(os.path.join(directory, "collisions", name + ".png"), frames[j])
            if animate:
                anim = self._sim.render_episode(e, episode=episode, **kw).cpu().numpy()
                rd.save_frames(os.path.join(directory, "animations", name + ".gif"), anim)
        return paths

    # ------------------------------------------------------------------ final observations (core.BatchedSim.keep_final)
    def keep_final_observations(self, on=True):
        """Batched mode with on-device auto-reset (set_fixture_suite(..., auto_reset=True)): keep what an auto-reset
        overwrites.  The observation step() returns for an env whose episode just ended is the RESET observation of its
        next episode; with this switched on the `info` dict of step() / rollout() also carries
          "final_observation": float32 device tensor [E, N, 6+7K], the observation of the terminal step -- the
                               final_observation / terminal_observation of the Gymnasium / SB3 vector APIs;
          "final_info":        {"at_goal", "in_collision", "ran_out_of_time"}: bool device tensors [E, N], the agents'
                               Agent.is_at_goal / in_collision / ran_out_of_time as the terminal step left them
        -- both meaningful ONLY for the envs with game_over set in that step (other rows are unspecified) -- and the fourth
        return value becomes `truncated`, a bool device tensor [E]: the episode ended with no agent in collision and at
        least one agent (of those present) out of time.  rollout(n) reports the items of its last step.  Stored by the
        step kernels themselves: the look-ahead ring keeps serving step(None), a slot's ring memory grows by the record
        (a default-length ring may be shorter).  The 'laserscan' / 'occupancy_grid' tensors are computed by their own
        kernels on the post-reset state and are NOT part of the record.  Off (the default): step() returns exactly what
        it did before -- False and the two `info` keys.  May be called before or after reset() and survives reset()."""
        if not on:
            self._final_req = False
            if self._sim is not None and self._sim._fin_on:
                self._sim.keep_final(False)
                self._resize_ring()
            return
        self._final_req = True
        self._check_final()
        if self._sim is not None and not self._sim._fin_on:
            self._sim.keep_final(True)
            self._resize_ring()

    def _check_final(self):
        if self.num_envs <= 1:
            raise ValueError("keep_final_observations() is for batched envs (num_envs > 1)")
        if self._fixture is None and (self.default_agents is not None or self._sim is not None):
            raise ValueError("keep_final_observations() needs the on-device auto-reset of set_fixture_suite(..., "
                             "auto_reset=True): without it nothing is overwritten")
        if self._fixture is not None and not self._fixture["auto_reset"]:
            raise ValueError("keep_final_observations() with auto_reset=False: no env is ever reset on the device, the "
                             "terminal observation is the one step() returns")

    # ------------------------------------------------------------------ the episode log (core.BatchedSim.log_episodes)
    LOG_CAPACITY = 16

    def log_episodes(self, on=True, capacity=None):
        """Batched mode with on-device auto-reset (set_fixture_suite(..., auto_reset=True)): log every finished episode
        on the device -- the step kernels store run_episode's per-episode statistics (env_utils.py:56-87) at the
        auto-reset that ends the episode, whether the steps come from step(), rollout() or the look-ahead ring --;
        episode_log() returns the episodes finished since it was last called.  `capacity`: episodes the log holds per env
        (default 16): enough for what an env finishes between two episode_log() calls plus what the look-ahead ring
        computes ahead (at most one episode per ring step); what does not fit is reported as `dropped`.  Off (the
        default): step() / rollout() run the kernels they ran before; they return exactly what they did either way.  May
        be called before or after reset() and survives reset() (which discards undrained episodes)."""
        if not on:
            self._log_req = None
            if self._sim is not None and self._sim._log is not None:
                self._sim.log_episodes(on=False)
            return
        self._log_req = {"capacity": None if capacity is None else int(capacity)}
        self._check_log()
        if self._sim is not None:
            self._sim.log_episodes(capacity=self._log_capacity())

    def _log_capacity(self):
        cap = self._log_req["capacity"]
        if cap is not None:
            return cap
        return self.LOG_CAPACITY

    def _check_log(self, who="log_episodes()"):
        if self.num_envs <= 1:
            raise ValueError("%s is for batched envs (num_envs > 1)" % who)
        if self._fixture is None and (self.default_agents is not None or self._sim is not None):
            raise ValueError("%s needs the on-device auto-reset of set_fixture_suite(..., auto_reset=True): "
                             "without it no episode ends on the device" % who)
        if self._fixture is not None and not self._fixture["auto_reset"]:
            raise ValueError("%s with auto_reset=False: no env is ever reset on the device, read the state "
                             "when game_over shows" % who)

    def measure_episodes(self, on=True, capacity=None, keep_tape=False):
        """Batched mode with on-device auto-reset: measure every episode on the device (core.BatchedSim.measure_episodes:
        per agent path_length, min_gap with its partner and time, turn_sum, moved_steps, close_steps -- a reduction kernel
        over the trajectory tape, which becomes transient unless keep_tape is set).  With the log on as well
        (log_episodes) episode_log() gains the metric columns; episode_metrics() drains them on their own.  `capacity`:
        episodes held per env (default: the log's), one of them the running episode.  May be called before or after
        reset() and survives reset() (which discards what was not drained).  Off (the default): nothing changes."""
        if not on:
            self._met_req = None
            if self._sim is not None and self._sim._met is not None:
                self._sim.measure_episodes(on=False)
            return
        self._met_req = {"capacity": None if capacity is None else int(capacity), "keep_tape": bool(keep_tape)}
        self._check_log("measure_episodes()")
        if self._sim is not None:
            self._sim.measure_episodes(capacity=self._met_capacity(), keep_tape=bool(keep_tape))

    def _met_capacity(self):
        cap = self._met_req["capacity"]
        if cap is not None:
            return cap
        return self._log_capacity() if self._log_req is not None else self.LOG_CAPACITY

    def episode_metrics(self):
        """The metrics of the episodes finished since the last call, ordered by (env, episode) -> dict of numpy arrays:
        `env`, `episode` [M]; `path_length`, `min_gap`, `turn_sum`, `min_gap_t` [M, N] float64; `moved_steps`,
        `close_steps`, `min_gap_partner` [M, N] int32; `dropped` (int).  episode_log() drains the same records when both
        are on: use one of the two.  Does not rewind the look-ahead ring."""
        if self._sim is None or self._sim._met is None:
            raise RuntimeError("episode_metrics(): the episode metrics are off (measure_episodes(), then reset())")
        return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in self._sim.episode_metrics().items()}

    def episode_log(self):
        """The episodes finished since the last call (or since log_episodes()), ordered by (env, episode) -> dict of numpy
        arrays in the row schema of experiments.run_full_test_suite.run_suite: `env`, `episode`, `test_case`, `num_agents`
        (slots that hold an agent), `steps` [M]; `total_reward`, `time_to_goal`, `extra_time_to_goal` [M, N] (0 in empty
        slots); `total_time_to_goal`, `collision`, `all_at_goal`, `any_stuck`, `outcome` ("collision" / "all_at_goal" /
        "stuck") [M] -- and `dropped`, the number of episodes that ended but were overwritten before this call (int).
        `env` is this shard's env index (add env_id_offset for the global one).  Does not rewind the look-ahead ring.
        With per-env maps (set_static_map(per_env=True)), additionally `map` [M]: the `map_index` value the env held
        while the episode ran.  With measure_episodes() on, additionally `path_length`, `min_gap`, `turn_sum`, `min_gap_t` [M, N] float64 (NaN where
        the record has no metrics) and `moved_steps`, `close_steps`, `min_gap_partner` [M, N] int32 (-1 there), filled for
        every record whose (env, episode) is in the metrics' drain as well, `has_metrics` [M] bool saying which, and
        `metrics_dropped` (int)."""
        if self._sim is None or self._sim._log is None:
            raise RuntimeError("episode_log(): the episode log is off (log_episodes(), then reset())")
        from gym_collision_avoidance_amd import episodes as eplog
        ep = self._sim.episodes()
        out = eplog.suite_columns({k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in ep.items()})
        if "map" in ep:   # a map set: the map_index value the env held while the episode ran (-1: not known any more)
            out["map"] = ep["map"].cpu().numpy().astype(np.int64)
        if self._sim._met is not None:
            from gym_collision_avoidance_amd import episode_metrics as epmet
            met = self.episode_metrics()
            li, cols = epmet.join(out, met)
            M, N = len(out["env"]), self._sim.N
            out["has_metrics"] = np.zeros(M, bool)
            out["has_metrics"][li] = True
            for n in epmet.FLOAT_COLUMNS:
                out[n] = np.full((M, N), np.nan)
                out[n][li] = cols[n]
            for n in epmet.INT_COLUMNS:
                out[n] = np.full((M, N), -1, np.int32)
                out[n][li] = cols[n]
            out["metrics_dropped"] = int(met["dropped"])
        return out

    def draw_rvo_on_device(self, seed):
        """Batched mode: RVOPolicy's stochastic branches -- `heading_noise` policies, Config.RVO_COLLAB_COEFF < 0 -- are drawn
        inside the step kernels as a pure function of (seed, global env id, episode, agent, episode step)
        (core.BatchedSim.set_rvo_draw; include/cagpu.h CaRvoDraw) instead of by torch's generator before every launch:
        step(None) is then served from the look-ahead ring, and rollout(n) and replay() work for such a batch.  seed: an int
        != 0 (None: back to the per-launch draws).  Call before reset(); takes effect at the next reset()."""
        if seed is not None and (int(seed) & 0xFFFFFFFFFFFFFFFF) == 0:
            raise ValueError("draw_rvo_on_device: seed must be != 0")
        self._rvo_device_seed = None if seed is None else int(seed)

    def sample_ga3c_on_device(self, seed, temperature=1.0, mask=None):
        """Batched mode: GA3C-CADRL agents SAMPLE their action from the softmax of their logits on the device, as a pure
        function of (seed, global env id, episode, agent, episode step) (core.BatchedSim.set_ga3c_sampling; include/cagpu.h
        CaGa3cSample), instead of playing the argmax.  seed: an int != 0 (None: greedy again); temperature > 0; mask: bool
        broadcastable to [num_envs, num_agents], the agents that sample (None: all).  Takes effect at once on a batch that
        has been reset(), and at every later reset()."""
        if seed is not None and (int(seed) & 0xFFFFFFFFFFFFFFFF) == 0:
            raise ValueError("sample_ga3c_on_device: seed must be != 0")
        self._ga3c_sampling = None if seed is None else dict(seed=int(seed), temperature=float(temperature), mask=mask)
        if self._sim is not None:
            self._apply_ga3c_sampling(self._sim)

    def _apply_ga3c_sampling(self, sim):
        samp = getattr(self, "_ga3c_sampling", None)
        if samp is None:
            sim.set_ga3c_sampling(None)
        else:
            sim.set_ga3c_sampling(**samp)

    def collect_experience(self, n, keep_obs=True):
        """Batched mode: play n steps with built-in policies only and return the on-policy record of the GA3C-CADRL agents
        as device tensors (core.BatchedSim.collect -> core.Experience: obs, action, logp, value, live, reward, done,
        game_over, last_value, address; Experience.gae(gamma, lam) gives advantages and returns).  Needs
        env.keep_ga3c_value = True before reset().  No host synchronisation between the first launch and the return."""
        if self._sim is None:
            raise RuntimeError("call reset() before collect_experience()")
        if self._host_policies or (self._host_by_env and any(self._host_by_env)):
            raise RuntimeError("collect_experience: user Python policies are queried on the host, step by step")
        sim = self._sim
        sim.p.dt = self.dt_nominal
        self._la_dt_ok = True
        self.episode_step_number += int(n)
        xp = sim.collect(n, keep_obs=keep_obs)
        self._snap, self._obs_np, self._scan_np = None, None, None
        if Config.USE_STATIC_MAP:   # (once, on the final state, as rollout() does)
            if self._map_lazy:
                self._map_stale = True
            else:
                self._map_sensors()
        return xp

    def replay(self, env_ids, episodes, **kw):
        """Run episodes of the batch again from their address -- `env_ids` (this shard's env indices, as episode_log()
        reports them) and `episodes`, ints or sequences of equal length -- on a child batch (core.BatchedSim.replay;
        keywords record=True, max_steps=None, keep_outputs=False): the log named the episode that failed, this shows it.
        -> replay.Replay: `record`, `final_observation`, `trajectories()`, `histories(i)`, `frames(i)` and `save_plots(dir)`,
        which writes the reference's `{test_case:03d}_{policy}_{N}agents.png` (and `collisions/` for the episodes that
        collided).  Neither the batch nor its look-ahead ring is touched.  ValueError where the episode depended on
        something the batch did not keep: external or user Python policies, custom Dynamics, stochastic RVO draws, sensor
        variants, an episode >= 1 without auto-reset, a map the log reports as -1."""
        if self._sim is None:
            raise RuntimeError("call reset() before replay()")
        host = dict(host_policies=bool(self._host_policies) or bool(self._host_by_env and any(self._host_by_env)),
                    host_dynamics=bool(self._host_dynamics) or bool(self._hostdyn_by_env and any(self._hostdyn_by_env)))
        rep = self._sim.replay(env_ids, episodes, _host=host, **kw)
        rep.plot_policy = self.plot_policy_name or self.agents[0].policy.str
        rep.plot_case_offset = int(self.test_case_index)
        rep.plot_defaults = self._render_defaults({})
        return rep

    def _ring_len(self, sim):
        """the longest look-ahead ring: `lookahead` if given, else what the byte budget holds of the batch's slots (with the
        final record every slot carries its final block as well: the same budget, a shorter ring)"""
        if self.lookahead is not None:
            return self.lookahead
        slot_bytes = self.num_envs * sim.N * (4 * sim.W + 5) + self.num_envs + (sim.final_step_bytes if sim._fin_on else 0)
        if self._map_ring and Config.USE_STATIC_MAP:   # the pose ring, the laser's index ring and the launch's tape
            from gym_collision_avoidance_amd import map_slots
            slot_bytes += map_slots.slot_bytes(self.num_envs, sim.N, Config.LASERSCAN_LENGTH, self._map_set is not None)
            slot_bytes += sim.traj_step_bytes
        return int(min(self.LOOKAHEAD_MAX, max(8, self.LOOKAHEAD_BYTES // slot_bytes)))

    def _resize_ring(self):
        """the default ring length follows the bytes of a slot: recomputed when the final record is toggled"""
        if not self._la_on or self.lookahead is not None:
            return
        self._enable_ring(self._sim)

    def _final_items(self, info, over, final_obs, final_flags):
        """adds "final_observation" / "final_info" to `info` -> truncated [E] (a few elementwise device ops, no sync)"""
        d = nat.decode_flags(final_flags)
        present = ~d["absent"]
        info["final_observation"] = final_obs
        info["final_info"] = {"at_goal": d["at_goal"] & present, "in_collision": d["in_collision"],
                              "ran_out_of_time": d["ran_out_of_time"] & present}
        return over & ~d["in_collision"].any(dim=1) & info["final_info"]["ran_out_of_time"].any(dim=1)

    # ------------------------------------------------------------------ batched extras
    def _action_tape(self, n_steps, actions):
        """rollout()'s `actions` -> float64 [n_steps, E, N, 2]: a ready array / tensor of that shape, or a sequence of
        n_steps items, each what step() accepts (a dict by agent index, batched an [E, N, 2] array), packed by
        _external_actions like a step's"""
        E, N = self.num_envs, self._sim.N
        if hasattr(actions, "shape") and len(actions.shape) == 4:
            if tuple(actions.shape) != (n_steps, E, N, 2):
                raise ValueError("rollout(): actions must be [n_steps, E, N, 2] = %r, got %r"
                                 % ((n_steps, E, N, 2), tuple(actions.shape)))
            return actions
        if len(actions) != n_steps:
            raise ValueError("rollout(): %d steps but %d actions" % (n_steps, len(actions)))
        items = [self._external_actions(a) for a in actions]
        if any(hasattr(a, "device") for a in items):
            import torch
            dev = self._sim.device
            zero = torch.zeros((E, N, 2), dtype=torch.float64, device=dev)
            return torch.stack([zero if a is None else torch.as_tensor(a, dtype=torch.float64).to(dev).reshape(E, N, 2)
                                for a in items])
        zero = np.zeros((E, N, 2), dtype=np.float64)
        return np.stack([zero if a is None else np.asarray(a, dtype=np.float64).reshape(E, N, 2) for a in items])

    def rollout(self, n_steps, actions=None, keep_steps=False):
        """n_steps x `step(None)` in ONE launch (`cagpu_step_ex`, CaStepEx.n_steps): the device-side form of env_utils.run_episode's
        `while not terminated: env.step(None)` loop for scenes whose policies are all internal.  Returns the last step's
        (obs, rewards, game_over, False, info); per-episode results accumulate in episode_stats() through the on-device
        auto-reset.  About 1.4x the throughput of n step() calls at 4096 x 10: a fused rollout never waits for the
        slowest workgroup of a step.
        actions: an ACTION TAPE -- n_steps items, each what step() accepts, or a ready [n_steps, E, N, 2] array / tensor:
        step t of the call plays actions[t] (`cagpu_step_tape`), the step of the CALL whatever episode an env is in (an env
        that auto-resets in step t plays actions[t + 1] as the first action of its next episode).  With it agents with the
        built-in external policies (ExternalPolicy, LearningPolicy, LearningPolicyGA3C, a policy draw whose pool holds them)
        are admitted: open-loop evaluation of an action sequence in one launch.  Host Python policies and custom Dynamics
        need the host between two steps and stay refused.
        keep_steps: the outputs of EVERY step, stacked: (obs [n, E, N, W], rewards [n, E, N], game_over [n, E], False, info)
        with info["which_agents_done"] [n, E, N] (a single env: numpy arrays [n, N, W], [n, N], [n], [n, N])."""
        if self._sim is None:
            raise RuntimeError("call reset() before rollout()")
        n_steps = int(n_steps)
        host_any = bool(self._host_policies or self._host_dynamics or (self._host_by_env and any(self._host_by_env)) or
                        (self._hostdyn_by_env and any(self._hostdyn_by_env)))
        if actions is None:
            if self._policy_pool is not None and any(g[0].policy.is_external for g in self._policy_pool["agents"]):
                raise ValueError("rollout() needs every policy of the draw's pool to be internal")
            if any(a.policy.is_external for a in self.agents) or host_any:
                raise ValueError("rollout() needs every policy to be internal (no external actions between the steps)")
        elif host_any:
            raise ValueError("rollout(actions=...) cannot run user Python policies or custom Dynamics: they are queried on the "
                             "host between two steps -- use step()")
        sim = self._sim
        tape = None if actions is None else self._action_tape(n_steps, actions)
        sim.p.dt = self.dt_nominal
        self.episode_step_number += n_steps
        # sense_map_in_ring: every step's sensors (batched)
        slots = bool(keep_steps and self._map_ring and Config.USE_STATIC_MAP and self.num_envs > 1)
        kept = sim.rollout(n_steps, tape, keep_steps=bool(keep_steps), map_sensors=slots)
        self._snap, self._obs_np, self._scan_np = None, None, None
        if slots:                   # (the sim's sensor tensors already show the last slot)
            self._occ_np, self._map_stale = None, False
        elif Config.USE_STATIC_MAP:   # (once, on the final state: the scan kernel reads the current state)
            if self._map_lazy:
                self._map_stale = True
            else:
                self._map_sensors()
        if keep_steps:
            obs, rewards, done, over = kept
            learning = {a.id: a.policy.is_still_learning for a in self.agents}
            if self.num_envs > 1:
                if self._policy_pool is not None:
                    learning = sim.learning_mask(still_learning=True)
                info = {"which_agents_done": done.bool(), "which_agents_learning": learning}
                if slots:
                    info["laserscan"] = sim.kept_map_sensors.laserscan()
                    if sim.occ is not None:
                        info["occupancy_grid"] = sim.kept_map_sensors.occupancy_grid()
                return obs, rewards, over.bool(), False, info
            info = {"which_agents_done": done[:, 0].cpu().numpy().astype(bool), "which_agents_learning": learning}
            return (obs[:, 0].cpu().numpy(), rewards[:, 0].double().cpu().numpy(), over[:, 0].cpu().numpy().astype(bool), False,
                    info)
        info = {"which_agents_done": sim.done.bool() if self.num_envs > 1 else
                {a.id: bool(d) for a, d in zip(self.agents, sim.done[0].cpu().numpy())},
                "which_agents_learning": {a.id: a.policy.is_still_learning for a in self.agents}}
        if self._policy_pool is not None and self.num_envs > 1:
            info["which_agents_learning"] = sim.learning_mask(still_learning=True)
        if self.num_envs > 1:
            over, truncated = sim.game_over.bool(), False
            if sim._fin_on:   # (the last step's: the record holds every env's most recent ending of the n steps)
                truncated = self._final_items(info, over, self._out(sim.final_obs), sim.final_flags)
            return self._out(sim.obs), self._out(sim.rewards), over, truncated, info
        return self._get_obs(), sim.rewards[0].double().cpu().numpy(), bool(sim.game_over[0].item()), False, info

    def episode_stats(self):
        """{name: value} of the episode counters accumulated on the device (core.STAT_NAMES), this shard only;
        reduce across GPUs with sharding.reduce_episode_stats."""
        from gym_collision_avoidance_amd import core
        vals = self._sim.episode_stats().cpu().numpy()
        return dict(zip(core.STAT_NAMES, [float(v) for v in vals]))
