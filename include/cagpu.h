/* include/cagpu.h -- C ABI of libcagpu.so, the MI355X (gfx950) hot path of the batched
 * collision-avoidance simulator.
 *
 * This is the drop-in boundary.  The reference has no device boundary at
 * all: its only FFI is the Cython `rvo2.PyRVOSimulator` binding.  Each entry point below names
 * the reference interface it replaces (paths relative to
 * /root/reference/gym_collision_avoidance/envs/).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch / C++ types; every data pointer is a DEVICE pointer
 *     into memory owned by the caller (torch tensors in the Python host), 16-byte aligned, valid
 *     until the stream reaches the call.  The library never allocates or frees device memory.
 *   - CaParams / CaState / CaOut / CaAutoReset are HOST structs, copied at call time.
 *   - asynchronous and stream-ordered on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream).  Re-entrant across streams and devices; the only host global is the
 *     thread-local last-error string.  Device globals: the fault word (cagpu_device_faults) and
 *     the per-CU progress table of the n-step kernel's progress-fair priorities -- words tagged
 *     with a per-process launch counter, read for issue priorities only: concurrent launches can
 *     perturb each other's priorities through it, never their results.
 *   - returns 0 on success, a negative CA_E* code otherwise; never throws across the boundary.
 *   - layout: agent-major SoA, index e*num_agents + a (agent fastest), one array per field, so a
 *     wavefront's 64 lanes load 64 consecutive elements.  State is float64 because the
 *     reference's state is (its discrete events -- at-goal, collision, time-out, sort buckets --
 *     are decided on float64 values); observations / rewards leave as float32, the dtype the
 *     reference declares for them (config.py:93-170).
 */
#ifndef CAGPU_H_
#define CAGPU_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAGPU_VERSION 12

/* error codes */
enum { CA_OK = 0, CA_EINVAL = -1, CA_EUNSUPPORTED = -2, CA_ELAUNCH = -3, CA_ENODEVICE = -4 };

/* per-agent flag word.  Bits 0-5 are the reference's Agent booleans (agent.py:108-112,138;
 * env.py:421-424,534-535); bits 6-7 come from the agent's Policy object (Policy.py:11-14,
 * config.py:152-157); bits 8-15 select the built-in policy / dynamics plugin. */
enum {
  CA_AT_GOAL = 1u << 0,
  CA_WAS_AT_GOAL = 1u << 1,
  CA_IN_COLLISION = 1u << 2,
  CA_WAS_IN_COLLISION = 1u << 3,
  CA_OUT_OF_TIME = 1u << 4,
  CA_DONE = 1u << 5,
  CA_IS_LEARNING = 1u << 6,
  CA_STILL_LEARNING = 1u << 7,
  CA_POLICY_SHIFT = 8,  /* 4 bits */
  CA_DYNAMICS_SHIFT = 12, /* 4 bits */
  /* Ragged batches: this agent SLOT holds no agent in the env's current episode.  The reference draws the agent count per
   * episode (test_cases.py:224-227: randint(2, MAX_NUM_AGENTS_IN_ENVIRONMENT + 1)) and every loop of its step runs over
   * len(self.agents) (collision_avoidance_env.py:345-367); here num_agents is the batch-wide MAXIMUM and an env with fewer
   * agents leaves its last slots absent.  Set by cagpu_reset / an auto-reset for a case row whose radius is <= 0 (the
   * padding rows of a ragged table); an absent slot is no neighbour, no collision partner, is not sensed, does not count
   * for game over or the episode statistics, and its outputs are zeros (observation row, reward) / done = 1 -- the zero
   * padding of wrappers.py:143-173.  Absent slots carry CA_DONE | CA_AT_GOAL | CA_WAS_AT_GOAL as well. */
  CA_ABSENT = 1u << 16,
  /* CaState.next_action holds this agent's action for the NEXT step (software-pipelined policy, see next_action).
   * Whoever writes the state arrays of an env directly must clear this bit for its agents (cagpu_reset does). */
  CA_PLAN_VALID = 1u << 17,
  /* RVOPolicy's `use_non_coop_policy` (RVOPolicy.py:33,77-90) of an agent whose anti-collaborative branch is drawn inside
   * the step kernels: written ONLY by launches with a CaRvoDraw whose collab_coeff < 0 (cagpu_step_noise), zero everywhere
   * else.  While it is set the agent's ORCA query runs with collaboration coefficient 0. */
  CA_RVO_NONCOOP = 1u << 18
};
/* policy plugin ids (test_cases.py:68-85 `policy_dict`) */
enum {
  CA_POL_RVO = 0,           /* policies/RVOPolicy.py + rvo2 (ORCA)           */
  CA_POL_NONCOOP = 1,       /* policies/NonCooperativePolicy.py              */
  CA_POL_STATIC = 2,        /* policies/StaticPolicy.py                      */
  CA_POL_EXTERNAL = 3,      /* policies/ExternalPolicy.py: raw [speed, dheading] from ext_actions */
  CA_POL_LEARNING = 4,      /* policies/LearningPolicy.py: scaled ext_actions */
  CA_POL_LEARNING_GA3C = 5, /* policies/LearningPolicyGA3C.py: discrete index in ext_actions[.,0] */
  CA_POL_GA3C_CADRL = 6     /* policies/GA3CCADRLPolicy.py: discrete index written into ext_actions[.,0] by cagpu_ga3c */
};
/* dynamics plugin ids (test_cases.py:93-96 `dynamics_dict`) */
enum {
  CA_DYN_UNICYCLE = 0,      /* dynamics/UnicycleDynamics.py:14-47            */
  CA_DYN_MAX_TURN_RATE = 1, /* dynamics/UnicycleDynamicsMaxTurnRate.py:17-43 */
  CA_DYN_EXTERNAL = 2       /* dynamics/ExternalDynamics.py                  */
};
/* OtherAgentsStatesSensor.agent_sorting_method (sensors/OtherAgentsStatesSensor.py:34-52) */
enum { CA_SORT_CLOSEST_FIRST = 0, CA_SORT_CLOSEST_LAST = 1, CA_SORT_TIME_TO_IMPACT = 2 };
/* game_over rule (collision_avoidance_env.py:537-551) */
enum { CA_OVER_ALL_DONE = 0 /* EVALUATE_MODE */, CA_OVER_AGENT0 = 1 /* TRAIN_SINGLE_AGENT */, CA_OVER_LEARNING_DONE = 2 };

/* The Config constants read on the hot path (config.py:28-86,174) + batch geometry. */
typedef struct CaParams {
  int32_t num_envs, num_agents;
  int32_t max_obs;           /* K = MAX_NUM_OTHER_AGENTS_OBSERVED; obs row = 6 + 7*K floats */
  int32_t sort_mode, game_over_mode;
  int32_t rvo_max_neighbors; /* MAX_NUM_AGENTS_IN_ENVIRONMENT (RVOPolicy.py:15) */
  int32_t obs_clip;          /* OtherAgentsStatesSensor.max_num_other_agents_observed (<= max_obs): only the
                                obs_clip closest others are emitted, the remaining rows stay zero
                                (OtherAgentsStatesSensor.py:39,112) */
  int32_t ragged;            /* != 0: envs may hold fewer than num_agents agents (CA_ABSENT slots: a case row with radius <= 0);
                                0 = every slot holds an agent, whatever its radius (the kernels skip the absent-slot tests) */
  double dt, near_goal_threshold, max_time_ratio, getting_close_range, sensing_horizon;
  double reward_at_goal, reward_collision, reward_time_step, reward_wiggly, wiggly_threshold;
  double reward_min, reward_max; /* np.clip bounds (collision_avoidance_env.py:589-599) */
  double rvo_time_horizon, rvo_collab_coeff;
  double max_heading_change; /* env-wide pi/3 (collision_avoidance_env.py:87), LearningPolicy.py:30 */
  double reward_collision_wall; /* REWARD_COLLISION_WITH_WALL (config.py:33; collision_avoidance_env.py:425-429) */
  double rvo_dt;             /* RVOPolicy.dt = Config.DT (RVOPolicy.py:13): rvo2's timeStep and the 1/dt of the speed
                                read-back (:26, :106) -- NOT the dt of this step() call, which only the dynamics see */
} CaParams;

/* Device pointers to the simulator state; [E*N] unless noted. */
typedef struct CaState {
  double *pos_x, *pos_y;       /* Agent.pos_global_frame                       */
  double *vel_x, *vel_y;       /* Agent.vel_global_frame                       */
  double *heading;             /* Agent.heading_global_frame                   */
  double *goal_x, *goal_y;     /* Agent.goal_global_frame                      */
  double *radius, *pref_speed;
  double *time_remaining;      /* Agent.time_remaining_to_reach_goal           */
  double *t;                   /* Agent.t                                      */
  double *slt;                 /* Agent.straight_line_time_to_reach_goal       */
  double *ep_reward;           /* running sum of this episode's rewards (env_utils.py:51) */
  float *last_action;          /* [E*N,2] Agent.past_actions[0] = [speed, delta heading] */
  uint32_t *flags;
  int32_t *step_num;           /* Agent.step_num                               */
  int32_t *episode_step;       /* [E] CollisionAvoidanceEnv.episode_step_number */
  int32_t *reset_count;        /* [E] auto-resets taken so far                 */
  double *env_stats;           /* [E,8] episodes, collision eps, all-at-goal eps, stuck eps, sum steps,
                                  sum total_reward, sum time_to_goal, sum extra_time_to_goal
                                  (experiments/src/env_utils.py:56-87, reduced to counters) */
  float *next_action;          /* [E*N,4] or NULL.  Software-pipelined policy query: the built-in RVO policy of step t+1
                                  reads the post-move state of step t only (collision_avoidance_env.py:305-323 runs it
                                  BEFORE anyone moves), exactly what the sensing / reward half of step t reads -- so with
                                  this array a step computes both side by side on disjoint waves and stores, per agent,
                                  {speed, delta heading (the float32 `all_actions` pair, env.py:305-307), ORCA velocity x, y}
                                  for the next step, flagged CA_PLAN_VALID; the next cagpu_step / cagpu_rollout then
                                  starts at the move.  Same arithmetic on the same inputs: results are bit-identical to
                                  next_action == NULL.  Agents without a valid plan (after a reset, after the host wrote
                                  the state, external / learning policies) are queried at the start of the step as before. */
  double *turning_dir;         /* [E*N] or NULL (not maintained).  Agent.turning_dir: the CADRL value network's turning
                                  memory, updated by UnicycleDynamics.step only (UnicycleDynamics.py:41-47), zeroed by
                                  Agent.reset (agent.py:133) */
  /* Per-step inputs of RVOPolicy's two stochastic branches (policies/RVOPolicy.py:77-90, :118-119), drawn by the CALLER
   * on the device before the launch (the host mirror does it with torch's device generator: core.BatchedSim
   * .set_rvo_stochastic) -- both NULL in the deterministic case, i.e. always in the reference's shipped configurations:
   *   rvo_collab        float  [E*N] or NULL: the collaboration coefficient of each agent AS THE EGO of its query
   *                     (setAgentCollabCoeff, :86-90) -- Config.RVO_COLLAB_COEFF, or 0 while an anti-collaborative agent
   *                     (RVO_COLLAB_COEFF < 0) is in its non-cooperative phase; NULL: CaParams.rvo_collab_coeff for all.
   *   rvo_heading_noise double [E*N] or NULL: added to the delta heading of an RVO agent's action after the pi/6 clip
   *                     (`delta_heading + np.random.normal(0, 0.5)`, :118-119); 0 for agents without heading_noise.
   * With either one set the policy is queried at the start of the step (the pipelined plan -- next_action -- is not
   * used: the draws belong to the step that consumes them). */
  const float *rvo_collab;
  const double *rvo_heading_noise;
  /* Externally integrated motion, applied AT THE MOVE of this step: device float64 [E*N, 5] = px, py, vx, vy, heading, or NULL.
   * An agent with CA_DYN_EXTERNAL whose row holds no NaN takes that state where the built-in models integrate theirs
   * (Agent.take_action, agent.py:214-220, calls `self.dynamics_model.step(action, dt)` -- here the caller ran its own
   * Dynamics subclass on the host with the action of this step), i.e. AFTER every policy of the step has been queried on
   * the pre-step state, and before the at-goal test, the clocks, collisions and sensing of the same step.  Rows of NaN /
   * agents with another dynamics id are ignored.  With it the policy is queried at the start of the step (like rvo_*). */
  const double *ext_state;
} CaState;

/* Device pointers to what a step hands back (collision_avoidance_env.py:225-234). */
typedef struct CaOut {
  float *obs;        /* [E,N,6+7K]: is_learning, num_other_agents, dist_to_goal, heading_ego_frame,
                        pref_speed, radius, other_agents_states[K][7] -- the array layout of
                        wrappers.py:143-173 (MultiagentDictToMultiagentArrayWrapper) */
  float *rewards;    /* [E,N]                                           */
  uint8_t *done;     /* [E,N] which_agents_done                         */
  uint8_t *game_over;/* [E]                                             */
  float *actions;    /* [E,N,2] the float32 `all_actions` array (env.py:305-307); may be NULL */
  float *orca_vel;   /* [E,N,2] or NULL: for every agent whose RVOPolicy was queried in this step, the velocity rvo2 chose
                        (PyRVOSimulator.doStep + getAgentVelocity, RVOPolicy.py:93) -- what cagpu_orca returns for the same
                        float inputs, bit for bit; 0 for the agents that were not queried.  Parity hook for the ORCA phases of
                        the step kernel itself. */
  void *workspace;   /* device scratch for envs with MORE THAN 64 AGENTS, or NULL.  Up to 64 agents an env is one workgroup tile
                        and every per-(agent, other) quantity lives in LDS; beyond that (the reference's make_testcase_huge /
                        get_testcase_huge, test_cases.py:914-1018: 100 agents) the step runs a one-thread-per-agent kernel
                        (num_agents <= 1024: workgroups of 256 / 512 / 1024 threads) whose per-pair columns live here.
                        cagpu_workspace_bytes(p) says how much. */
  uint64_t workspace_bytes;
} CaOut;

/* Fixture-table auto-reset (the batched form of vec_env.py:120-128 + test_cases.py:593-624):
 * when env e's episode ends its statistics are added to env_stats[e], its k-th reset loads case
 * (env_id_offset + e + k*case_stride) % n_cases of `table` and the observation handed back is the
 * reset observation (rewards / done / game_over stay those of the terminal step; the terminal observation and the
 * agents' final flag words are kept on request: CaFinal, cagpu_step_final / cagpu_rollout_final). */
typedef struct CaAutoReset {
  const double *table; /* device, [n_cases, N, 6] = px, py, gx, gy, pref_speed, radius */
  int32_t n_cases;
  int64_t env_id_offset; /* global id of this shard's env 0 (multi-GPU sharding) */
  int64_t case_stride;   /* normally the global number of envs */
  const float *reset_obs; /* device float [n_cases, N, 6+7*max_obs] or NULL: the reset observation of every case,
                             i.e. o->obs of cagpu_reset(num_envs = n_cases, cases = table) with the same CaParams.
                             With it an auto-reset copies the row; without it the tile runs a second sensing pass. */
  const float *reset_plan; /* device float [n_cases, N, 4] or NULL: CaState.next_action of every case's reset state (cagpu_plan
                              on the state cagpu_reset(num_envs = n_cases, cases = table) leaves), so that an auto-reset
                              env starts its new episode with a valid plan; only read when CaState.next_action is set. */
  uint64_t heading_seed;  /* 0: the initial heading of a reset agent points at its goal (EVALUATE_MODE, test_cases.py:555-557).
                             Otherwise training mode (test_cases.py:558-559: np.random.uniform(-pi, pi)): heading =
                             -pi + 2 pi u, u the Philox4x32-10 uniform of (heading_seed; global env id, reset count, agent)
                             -- a pure function of those, whatever the batch size or sharding; reset_obs is then not
                             used (the observation depends on the heading: second sensing pass). */
} CaAutoReset;

/* Static occupancy grid shared by every env (Map.py:6-24; the env builds Map(16 m, 16 m, 0.1 m), env.py:378-392).
 * Bit-packed, row-major: cell (row, col) is bit (col & 31) of word static_bits[row * ((cols + 31) / 32) + col / 32];
 * row = floor(origin_r - y / cell), col = floor(origin_c + x / cell) (Map.py:26-32). */
typedef struct CaMap {
  const uint32_t *static_bits; /* device; NULL = no static obstacles (agents are still rasterised for the scan) */
  int32_t rows, cols;
  double cell, origin_r, origin_c;
} CaMap;

/* A MAP SET (v12): M static grids of one geometry and a map per env -- the batched form of the reference's list of
 * candidate maps, one of which env.reset() draws for every episode (collision_avoidance_env.py:369-376, :274-275,
 * :384-385).  map.static_bits holds the M grids back to back, grid m at word m * rows * ((cols + 31) / 32), each laid out
 * as a CaMap grid.  An env whose env_map entry lies outside [0, num_maps) reads no map memory (it sees an empty map) and
 * raises bit 2 of the device fault word (cagpu_device_faults). */
typedef struct CaMapSet {
  CaMap map;           /* the geometry every map shares; static_bits = the num_maps grids (must not be NULL) */
  int32_t *env_map;    /* device int32 [E]: the map of env e.  STATE: rewritten by an auto-reset when map_seed != 0 */
  int32_t num_maps, reserved0;
  uint64_t map_seed;   /* 0: an auto-reset keeps the env's map.  Otherwise the k-th auto-reset of env e sets
                          env_map[e] = min(floor(M * u), M - 1), u = the Philox4x32-10 uniform of key map_seed and counter
                          (g lo, g hi, k, 0xFFFFFFFF), g = CaAutoReset.env_id_offset + e (the construction of heading_seed's
                          draws, whose last counter word is an agent index < 1024: the two streams never meet) -- a pure
                          function of (map_seed, global env id, reset count), whatever the batch size or sharding. */
} CaMapSet;

/* LaserScanSensor state + observation (sensors/LaserScanSensor.py:24-44): num_beams beams over
 * [min_angle, max_angle] around the heading, num_ranges samples every range_res metres. */
typedef struct CaScan {
  uint8_t *hist; /* device [E,N,num_to_store,num_beams]: range index per beam, 255 = nothing hit (state) */
  float *out;    /* device [E,N,num_to_store,num_beams]: the 'laserscan' observation in metres */
  int32_t num_beams, num_to_store, num_ranges, reserved0;
  double min_angle, max_angle, range_res, max_range;
} CaScan;

/* OccupancyGridSensor window + outputs (sensors/OccupancyGridSensor.py:15-22, :44): every agent's height x width crop of
 * its env's dynamic map, height = int(y_width / cell), width = int(x_width / cell) (the reference's 5 m x 5 m on the 0.1 m
 * map: 50 x 50).  Two output formats, either pointer may be NULL, not both (device, 16-byte aligned):
 *   cells  uint8  [E,N,height,width], 0 / 1 -- a bool array as the reference returns it;
 *   bits   uint32 [E,N,height,(width + 31) / 32]: cell b of a window row is bit (b & 31) of word b >> 5, unused high bits 0. */
typedef struct CaOccGrid {
  uint8_t *cells;
  uint32_t *bits;
  int32_t height, width;   /* 1 .. 256 each */
  double x_width, y_width; /* metres: the window spans [px - x_width / 2, px + x_width / 2) x (py - y_width / 2, py + y_width / 2] */
} CaOccGrid;

/* Trajectory tape (CaStepEx.traj; cagpu_step_traj / cagpu_rollout_traj): the reference's Agent.global_state_history rows
 * (agent.py:257-289, appended by Agent.take_action with Config.STORE_HISTORY), written by the step kernels themselves.
 * Step t of a call (t = 0 .. n_steps - 1; a single step: t = 0) writes slot t.  Per (slot, env, agent slot):
 *   - an agent that gets past the done gate of Agent.take_action in this step writes all 12 columns:
 *       0 t BEFORE the increment, 1-2 position, 3-4 goal, 5 radius, 6 pref_speed, 7-8 velocity,
 *       9 speed (the float32 action speed widened: Agent.speed_global_frame = past_actions[0][0]), 10 heading
 *     -- position / velocity / heading AFTER the move, goal / radius / pref_speed as held at the move (a StaticPolicy
 *     agent's goal is its position) --, and 11 = Agent.step_num BEFORE the increment as a double: the index of the row in
 *     the reference's global_state_history;
 *   - an agent that does not move (done, or an absent slot of a ragged batch) writes column 11 = -1.0 ONLY: columns
 *     0 - 10 of such a row are LEFT ALONE (whatever the caller's buffer held).
 * The terminal step of an episode is recorded before an auto-reset replaces the state; the first step of the next episode
 * has index 0 and an `episode` entry one higher. */
typedef struct CaTraj {
  double  *rows;     /* device [n_steps, E, N, 12], 16-byte aligned */
  int32_t *episode;  /* device [n_steps, E] or NULL: CaState.reset_count[e] as the step STARTS (before its auto-reset) */
} CaTraj;

/* Final record (CaStepEx.fin; cagpu_step_final / cagpu_rollout_final): what an auto-reset would otherwise overwrite.  For every env whose
 * episode ends in a step AND is auto-reset in it (game_over[e] != 0 with a CaAutoReset attached), the step kernel stores,
 * before the reset replaces them,
 *   obs    the env's observation rows of the TERMINAL step, exactly as the step produced them (is_learning column included;
 *          the rows of absent slots are zeros) -- the `final_observation` / `terminal_observation` of the vector-env APIs;
 *   flags  the agents' flag words as they stand at the end of the terminal step (CA_AT_GOAL / CA_IN_COLLISION /
 *          CA_OUT_OF_TIME / CA_DONE / CA_ABSENT ... as decided by that step; CA_PLAN_VALID is unspecified; with a CaRvoDraw,
 *          CA_RVO_NONCOOP -- bit 18 -- as the terminal step's query left it).
 * Rows of every OTHER env are LEFT ALONE (whatever the caller's buffer held): a row is valid where game_over says so.
 * Slots: the block advances exactly as the CaOut outputs do -- a ring call (every step keeps its outputs) writes step t's
 * records to block t of [n_steps, E, N, 6+7K] / [n_steps, E, N]; a plain cagpu_rollout_final (ring == 0: every step writes
 * the same CaOut buffers) writes every step's records to the SAME single block, which therefore ends up holding each env's
 * MOST RECENT terminal record of the launch (envs that ended no episode in it keep what the buffer held). */
typedef struct CaFinal {
  float    *obs;    /* device [E, N, 6+7K] (ring: [n_steps, E, N, 6+7K]), the layout of CaOut.obs; 16-byte aligned */
  uint32_t *flags;  /* device [E, N] (ring: [n_steps, E, N]) or NULL; 4-byte aligned */
} CaFinal;

/* Episode log (CaStepEx.log; cagpu_step_log / cagpu_rollout_log): one record per FINISHED EPISODE, written by the step kernels at the
 * auto-reset that would otherwise overwrite it -- the per-episode quantities of the reference's run_episode
 * (experiments/src/env_utils.py:56-87), which CaState.env_stats keeps only as sums.  Every env owns a ring of `capacity`
 * slots; when env e ends its k-th episode (k = CaState.reset_count[e] BEFORE the increment) and is auto-reset in the same
 * step, the record goes to slot k % capacity of env e's ring: a pure function of (e, k) -- no atomic, no shared counter, no
 * order between envs -- so one launch per step, cagpu_rollout, a look-ahead ring and a rewind-and-replay all write the same
 * bytes to the same place.  Slots of envs that end no episode are LEFT ALONE; the caller initialises `head` to -1 and
 * recognises a valid slot by its stamp head[..., 0] == k.  An older record is overwritten once the env is `capacity`
 * episodes further. */
typedef struct CaEpLog {
  double  *rows;   /* device [E, C, N, 4], 16-byte aligned.  Per agent slot:
                      0 total_reward (CaState.ep_reward), 1 time_to_goal (t), 2 extra_time_to_goal (t - slt)
                        -- 0..2 are exactly the three per-agent addends that the kernel sums into env_stats[e][5..7];
                      3: the agent's flag word as the terminal step leaves it (what CaFinal.flags holds: with a
                         CaRvoDraw that includes CA_RVO_NONCOOP, bit 18, as the step left it),
                         bit pattern in the low 32 bits of the 8 bytes, high 32 bits zero */
  int32_t *head;   /* device [E, C, 4], 16-byte aligned: {k, steps, case, outcome}
                      k       = reset_count[e] BEFORE the increment (index of the env's episode that just ended)
                      steps   = the value added to env_stats[e][4]
                      case    = row of CaAutoReset.table the ended episode ran on:
                                (env_id_offset + e + k * case_stride) % n_cases
                      outcome = 0 collision / 1 all at goal / 2 stuck (the env_stats[1..3] classification) */
  int32_t capacity, reserved0;   /* C >= 1 */
} CaEpLog;

/* Episode metrics (cagpu_episode_metrics; additive to v12): per-episode path and closest-approach numbers of every agent,
 * reduced from trajectory-tape slots (CaTraj) by a kernel of their own -- no step kernel knows about them.  The rules
 * (tests/episode_metrics_ref.py is their float64 NumPy statement, which the kernel reproduces bit
 * for bit): per env the slots are walked in step order, k = episode[t, e]; an agent has MOVED in a slot where column 11 is
 * >= 0 (columns 0 - 10 of any other row are never read).  Within a slot every moved row first gives its position
 * (columns 1, 2) and radius (5) and marks its agent `seen`; then, per moved agent a:
 *   moved_steps += 1;  path_length += sqrt(vx * vx + vy * vy) * CaParams.dt  (columns 7, 8);
 *   turn_sum += fabs(remainder(heading - last heading, 2 pi)) from the agent's second row of the episode on (column 10);
 *   over the seen agents j != a: g = (sqrt(dx * dx + dy * dy) - radius[a]) - radius[j], its minimum g_min (ties: lowest j);
 *   if there is such a j: close_steps += (g_min <= getting_close_range), and where g_min < min_gap strictly:
 *   min_gap = g_min, min_gap_partner = j, min_gap_t = column 0 of a's row.
 * An agent that is done stays seen, where it stopped, until the episode ends; an agent that never moved in the episode is
 * never seen.  Where episode[t, e] differs from the carried episode id the finished episode's record is written and the
 * env's carry cleared; at the end of every call each env also writes the record of its RUNNING episode (a later call
 * overwrites it).  Episode k of env e goes to slot k % capacity and is valid where head[e, k % capacity] == k -- CaEpLog's
 * rule; a running episode therefore takes the slot of the episode `capacity` before it with its first processed step.
 * Defaults of an agent without a partner: min_gap +inf, min_gap_t NaN, min_gap_partner -1. */
typedef struct CaEpMetrics {
  double  *vals;   /* device [E, C, N, 4], 16-byte aligned: path_length, min_gap, turn_sum, min_gap_t */
  int32_t *cnts;   /* device [E, C, N, 4], 16-byte aligned: moved_steps, close_steps, min_gap_partner, 0 */
  int32_t *head;   /* device [E, C], 4-byte aligned: the stamp k; the caller fills it with -1 */
  int32_t capacity, reserved0;   /* C >= 1 */
  void    *carry;  /* device, cagpu_episode_metrics_carry_bytes(p) bytes, 16-byte aligned, ZEROED by the caller: env e owns
                      bytes [e, e + 1) x (carry bytes / E); zeroing an env's share forgets its running episode */
  double getting_close_range;   /* Config.GETTING_CLOSE_RANGE (CaParams.getting_close_range) */
} CaEpMetrics;

/* Frames of cagpu_render / cagpu_render_maps (additive to v12): F pictures of height x width pixels, each of ONE env, drawn from the
 * current state, the env's static map and a block of trajectory-tape rows by the drawing rules of DESIGN.md section 13.
 * The window: pixel (row r, column c) has its centre at x = xmin + (16 c + 8) / s16, y = ymax - (16 r + 8) / s16,
 * s16 = 16 x pixels per metre (row 0 is the top); a world coordinate becomes the 1/16-pixel integer
 * floor((x - xmin) * s16) / floor((ymax - y) * s16), saturated at +-2^20, and every inside test is integer arithmetic.
 * Frame f shows env frame_env[f] (outside [0, E): a white frame) and the history rows of slots first[f] .. last[f]
 * (clamped to the block) of column frame_col[f] of `hist` (frame_col NULL: column frame_env[f]; a column outside the
 * block: no agents) -- the rows of an agent are the slots whose column 11 is >= 0, in slot order.  last[f] < first[f]: a
 * SNAPSHOT frame of the current state (one disc per agent that is not CA_ABSENT, its goal marker).  Several frames may
 * show one env with growing `last`: the animation of an episode is one call. */
typedef struct CaRender {
  uint8_t *out;             /* device uint8 [F, height, width, 3] RGB, 16-byte aligned */
  int32_t num_frames, height, width; /* F >= 1; height, width in [16, 1024] */
  int32_t flags;            /* bit 0: circles_along_traj (visualize.py:175-228; clear: the scatter mode, :236-251);
                               bit 1: draw the static map */
  double xmin, ymax, s16;
  const int32_t *frame_env; /* device int32 [F] */
  const int32_t *frame_col; /* device int32 [F] or NULL */
  const int32_t *first, *last; /* device int32 [F] */
  const double *hist;       /* device [hist_steps, hist_cols, N, 12], rows as CaTraj.rows holds them, or NULL (no history:
                               every frame with last >= first shows no agents); 16-byte aligned */
  int32_t hist_steps, hist_cols;
  int64_t stride_t, stride_s; /* doubles between two slots / two columns of `hist` (an agent's rows are 12 apart) */
  void *work;               /* device scratch, 16-byte aligned: the frames' primitive lists */
  uint64_t work_bytes;      /* >= cagpu_render_work_bytes(F, N, hist_steps) */
} CaRender;

/* GA3C-CADRL network weights (policies/GA3C_CADRL/checkpoints/<run>/network_*.data-00000-of-00001): device float
 * pointers in the checkpoint's own layout, kernels row-major [in, out].  LSTM gate order i, j, f, o. */
typedef struct CaNet {
  const float *lstm_kernel, *lstm_bias;     /* rnn/lstm_cell/{kernel [71,256], bias [256]}: input = [x_t (7), h (64)] */
  const float *layer1_kernel, *layer1_bias; /* layer1/{kernel [68,256], bias}: input = [host (4), h_final (64)]       */
  const float *layer2_kernel, *layer2_bias; /* layer2/{kernel [256,256], bias}                                        */
  const float *fc1_kernel, *fc1_bias;       /* fullyconnected1/{kernel [256,256], bias}                               */
  const float *logits_kernel, *logits_bias; /* logits_p/{kernel [256,11], bias [11]}                                  */
  const float *input_mean, *input_std;      /* graph constants `Const`, `Const_1` [138] (= config.py:93-149)          */
  /* Scratch for cagpu_ga3c, device int32 [num_envs * num_agents + 6] (the list, its count at [num_envs * num_agents], two
   * 64-bit counters behind it that are tagged with the call's epoch: the scratch needs NO initialisation and nothing an earlier
   * or aborted call left in it matters; the order of the packed rows across workgroups is unspecified), or NULL.  With it the agents that need an action
   * this step (GA3C-CADRL policy, not done: collision_avoidance_env.py:310-312 queries no others) are packed first and
   * only their rows are evaluated -- in steady state about half of the agents of an evaluation batch are done and wait
   * for their env's game over.  NULL: every 64-agent tile that holds at least one such agent is evaluated whole. */
  int32_t *rows_scratch;
  /* Which agents this checkpoint drives (the reference gives every agent its own policy object and network session,
   * GA3CCADRLPolicy.py:23-47, so agents of one scene may run different checkpoints): device int32 [num_envs * num_agents]
   * or NULL.  With it, cagpu_ga3c evaluates only the agents with agent_net[i] == net_index; the caller makes one call per
   * distinct checkpoint (each writes its own agents' entries of ext_actions).  NULL: every live GA3C-CADRL agent. */
  const int32_t *agent_net;
  int32_t net_index, reserved0;
  /* The four big weight matrices as fp16 planes in matrix-core fragment order: device buffer of cagpu_ga3c_packed_bytes()
   * bytes (16-byte aligned), filled ONCE per checkpoint by cagpu_ga3c_pack() from the float32 arrays above (which cagpu_ga3c
   * still reads for the x_t / host inputs, the biases and the logits layer).  Required: cagpu_ga3c fails with CA_EINVAL
   * without it.  The network computes on float32 operands carried as two fp16 planes (22 significant bits); see cagpu_ga3c. */
  const void *packed;
} CaNet;

int cagpu_version(void);
const char *cagpu_last_error(void);
/* Introspection for tests / bench.py: the kernel instantiation and launch geometry the last cagpu_step / rollout /
 * reset / observe call of THIS thread selected, e.g. "ca_kernel<256, false, 10, false, true, 4> grid=1024 ...".
 * The selection depends only on the call's arguments and the device's CU count (never on the environment). */
const char *cagpu_last_kernel(void);

/* Replaces: Agent.reset (agent.py:59-138) for every agent of the envs with mask[e] != 0 (mask NULL =
 * all), in the EVALUATE_MODE form of test_cases.py:545-590 (heading toward the goal unless
 * `headings` [E,N] is given), followed by the reset observation (collision_avoidance_env.py:276-282).
 * cases: device [E,N,6] = px, py, gx, gy, pref_speed, radius; a row with radius <= 0 leaves its slot absent
 * (CA_ABSENT: ragged batches, absent slots last).  The policy / dynamics / learning bits of `flags` must already be
 * set; reset_count[e] is zeroed, CA_PLAN_VALID cleared. */
int cagpu_reset(const CaParams *p, const CaState *s, const CaOut *o, const double *cases, const double *headings,
                const uint8_t *mask, void *stream);

/* Replaces: CollisionAvoidanceEnv.step (collision_avoidance_env.py:156-234) for every env:
 * policy queries on the pre-step state (RVOPolicy / rvo2.doStep, NonCooperative, Static, external),
 * Agent.take_action + UnicycleDynamics.step + update_ego_frame, _check_for_collisions,
 * _compute_rewards, OtherAgentsStatesSensor.sense + observation assembly, _check_which_agents_done.
 * ext_actions: device float64 [E,N,2], read only for agents with an external policy; may be NULL
 * (the reference's `env.step(None)`, env_utils.py:50).  ar == NULL: no auto-reset.
 *
 * THE GENERAL ENTRY POINT (additive to v12).  Every way of launching the step is one CaStepEx: how many steps, whether every
 * step keeps its outputs, and which per-call records the kernels read or write beside the state and the CaOut outputs.  The
 * eleven older names below are fixed conveniences, each equal to one CaStepEx; a NEW per-call record becomes one more
 * pointer HERE (and one in the kernels' argument block), not another pair of entry points.  A HOST struct like the others,
 * copied at call time, and so are the records it points to. */
typedef struct CaStepEx {
  int32_t n_steps;          /* >= 1 */
  int32_t ring;             /* != 0: every step keeps its outputs (cagpu_rollout_ring) */
  int64_t snapshot_delta;   /* ring only */
  const CaMap    *map;      /* each of the five: NULL = not used */
  const CaMapSet *set;
  const CaTraj   *traj;
  const CaFinal  *fin;
  const CaEpLog  *log;
} CaStepEx;                 /* 56 bytes */

/* x == NULL: cagpu_step.  The rules, stated once -- every violation is CA_EINVAL with nothing launched, unless noted:
 *   n_steps  the steps fused into ONE launch (every step still writes its outputs; with ring == 0 the buffers hold the last
 *            step's).  Envs never interact, so no grid-wide sync is needed: the batched form of env_utils.py:45-52
 *            `while not terminated: env.step(None)`.  ext_actions (if any) are held constant over the n_steps (a new action
 *            for every step: cagpu_step_tape, below).  n_steps < 1
 *            is rejected.  The per-step inputs CaState.rvo_collab / rvo_heading_noise / ext_state belong to the ONE step that
 *            consumes them: any of them set with n_steps > 1 or ring is rejected.
 *   ring     != 0: the output pointers of `o` name slot 0 of a ring of n_steps slots and step t of the call writes slot t
 *            (cagpu_rollout_ring has the layout); state, statistics and auto-resets are those of ring == 0.
 *   snapshot_delta  the ring's rewind point (cagpu_rollout_ring): != 0 without ring is rejected; with ring but without the
 *            pipelined n-step kernel (cagpu_ring_snapshots() != 1) it is CA_EUNSUPPORTED.
 *   map      a static map: an agent whose disc covers an occupied static cell collides with the wall
 *            (collision_avoidance_env.py:494-506, :425-429).  map->static_bits == NULL: as without a map; otherwise rows,
 *            cols >= 1 and cell > 0.
 *   set      a map per env (CaMapSet; cagpu_step_maps has the semantics): set->env_map or set->map.static_bits NULL,
 *            num_maps < 1 or a bad geometry is rejected.
 *            map and set at once is rejected.  Either of them with n_steps > 1 or ring is rejected by cagpu_step_ex,
 *            cagpu_step_draw and every older name; cagpu_step_ex_maps (below) is the same call with that one rule lifted.
 *   traj     the trajectory tape (CaTraj): step t of the call records slot t.  traj->rows NULL or not 16-byte aligned, or
 *            traj->episode not 4-byte aligned, is rejected.
 *   fin      the final record (CaFinal) of every env that auto-resets.  fin->obs NULL or not 16-byte aligned,
 *            fin->flags not 4-byte aligned, or fin without ar (nothing is ever overwritten then) is rejected.
 *   log      the episode log (CaEpLog).  log->rows or log->head NULL or not 16-byte aligned, capacity < 1, or log without ar
 *            (no episode is ever logged then) is rejected.
 * A call that is wrong in several ways reports the first of: map and set at once, snapshot_delta without ring, the log,
 * the final record, the tape, params / state / out, the rest.
 * The records change neither the kernel selection nor grid and block: state, outputs and statistics are bit-identical with
 * and without them, and every kernel family (the general, the pipelined single- and n-step and the large-env kernel) writes
 * all three -- the pipelined kernels keep the final record and the log through their " final" instantiations (a template
 * flag; the log behind a uniform test of its pointers inside), the general kernel on both of its reset paths (reset_obs copy
 * / second sensing pass), the general and the large-env kernel behind uniform tests, always with ordinary stores from the
 * lanes that hold the values.  cagpu_last_kernel() shows " traj" / " final" / " log" behind the pipelined kernel's name.  A
 * ring launch logs the episodes of steps that are not handed out yet; a replay from a rewind point rewrites the same
 * records bit for bit. */
int cagpu_step_ex(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                  const CaStepEx *x, void *stream);

/* MAPS IN FUSED LAUNCHES (additive to v12; no new struct).  cagpu_step_draw (cagpu_step_ex when draw == NULL) in every rule
 * but one: x->map or x->set is admitted with n_steps > 1 and with ring.  Map and set at once, a bad CaMapSet and the
 * per-step inputs (rvo_collab / rvo_heading_noise / ext_state) in a multi-step call are rejected as there.
 *   ordering   step t of the launch tests its walls against the map the env holds when step t begins.  An auto-reset in step
 *              t with set->map_seed != 0 stores the env's next map (CaMapSet.map_seed: a function of the key, the global env
 *              id and the env's reset count) AFTER that test: the terminal step sees the old map, step t + 1 the new one --
 *              n single cagpu_step_maps calls, bit for bit.  An index outside [0, num_maps) reads no map memory and raises
 *              bit 2 of the fault word in every step that meets it.
 *   kernels    the kernel choice does not depend on the map: cagpu_ring_snapshots() answers for a ring launch with a map
 *              or a set what it answers without one.  env_map is NOT part of a ring's rewind snapshot (the state slab): a
 *              caller who rewinds a ring of a set with a key restores its own copy of env_map, taken before the launch.
 *              A set in an n-step launch runs the MSET instantiations of the pipelined and the general kernel, which no other
 *              launch selects (cagpu_last_kernel() shows " set"); a rollout that is split into single launches and the
 *              large-env kernel carry the map or set into every launch (" map", as for every single step with a map or set).
 *   sensors    cagpu_laserscan / cagpu_occupancy_grid read the CURRENT state: after an n-step launch that is the final one. */
struct CaPolicyDraw;   /* (defined with cagpu_step_draw below) */
int cagpu_step_ex_maps(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                       const CaStepEx *x, const struct CaPolicyDraw *draw /* may be NULL */, void *stream);

/* ACTION TAPES (additive to v12): cagpu_step_ex_maps with `ext_actions` replaced by a record that may hold a NEW external
 * action for EVERY step of a fused launch -- open-loop evaluation of an action sequence, a learner's or planner's recorded
 * actions, in one launch instead of one per step.  The external action is read at the move of the step that consumes it (never
 * by the policy plan of the step before), so step t reading slot t has no ordering problem. */
typedef struct CaActionTape {
  const double *actions;   /* device float64, slot t = [E, N, 2] in the layout of ext_actions; 16-byte aligned */
  int64_t       step_stride; /* doubles from slot t to slot t + 1: 0 = one slot held for all steps (cagpu_step_ex's rule),
                                otherwise even and >= 2 * E * N */
} CaActionTape;              /* 16 bytes */

/* The rules -- every violation is CA_EINVAL with nothing launched and a cagpu_last_error() text:
 *   tape == NULL      exactly cagpu_step_ex_maps(..., ext_actions = NULL, ...).
 *   step_stride == 0  exactly cagpu_step_ex_maps(..., ext_actions = tape->actions, ...): the same launch, the same bits, the
 *                     same cagpu_last_kernel() string (and, as there, no check of `actions`: NULL = no external actions).
 *   step_stride != 0  step t of the call (t = 0 .. n_steps - 1) reads actions + t * step_stride.  The index is the step of the
 *                     LAUNCH, not the step of the episode: an env that auto-resets in step t plays slot t + 1 as the first
 *                     action of its next episode.  Rejected: tape->actions NULL or not 16-byte aligned; step_stride negative,
 *                     odd, or in (0, 2 * num_envs * num_agents).
 *   everything else   every rule of cagpu_step_ex_maps holds as it does there, in that entry point's own words (a call that is
 *                     wrong in an older way returns its code and its text): maps and sets are admitted in fused launches;
 *                     rvo_collab / rvo_heading_noise / ext_state are rejected with n_steps > 1 or ring; the records and the
 *                     draw are checked as there.  In the order of first-reported errors the two tape rejections stand LAST
 *                     among the CA_EINVAL ones -- behind map and set at once, snapshot_delta without ring, the draw, the log,
 *                     the final record, the trajectory tape, params / state / out, the map set, n_steps, the multi-step rules,
 *                     a bad CaAutoReset and a bad CaMap -- and ahead of the ring's CA_EUNSUPPORTED (snapshot_delta without
 *                     the pipelined n-step kernel).
 *   who is read       only the entries of agents whose external policy is QUERIED in the step (CA_POL_EXTERNAL / _LEARNING /
 *                     _LEARNING_GA3C, not done, present).  Entries of internal policies, of done agents and of the absent
 *                     slots of a ragged batch are never read for effect: a NaN there changes nothing.
 *   kernels           the kernel choice does not depend on the tape.  The n-step forms of the general and the pipelined kernel
 *                     add t * step_stride to the slot address in scalar registers (a kernel argument times the loop counter:
 *                     nothing joins the vector instruction stream, nothing at all where ext_actions is NULL); where a rollout
 *                     is n launches (the large-env kernel; the general kernel beyond one resident round of workgroups) the host
 *                     side advances the pointer per launch.  Every launch with step_stride != 0 shows " tape" at the end of
 *                     cagpu_last_kernel(); every launch without a tape reports the string it always reported.
 *   records           map, map set, trajectory tape, final record, episode log, policy draw and the output ring ride on a tape
 *                     launch exactly as on any other fused launch; a ring's rewind snapshot does not cover the tape (read-only). */
int cagpu_step_tape(const CaParams *p, const CaState *s, const CaOut *o, const CaActionTape *tape,
                    const CaAutoReset *ar, const CaStepEx *x, const struct CaPolicyDraw *draw, void *stream);

/* out[i] = the map a map-set env with global id env_ids[i] takes at its counts[i]-th auto-reset under key `seed`
 * (CaMapSet.map_seed's rule), i < n: device int64 / int32 in, device int32 out.  Lets a host say which map a logged episode
 * ran on without a field in the log record.  CA_EINVAL: NULL pointers, seed == 0, num_maps < 1, n < 0.  n == 0: nothing. */
int cagpu_map_draw(uint64_t seed, int32_t num_maps, const int64_t *env_ids, const int32_t *counts, int64_t n, int32_t *out,
                   void *stream);

/* = cagpu_step_ex with x == NULL (n_steps = 1, no ring, no record). */
int cagpu_step(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
               void *stream);

/* = CaStepEx{n_steps = 1, map}.  map == NULL: cagpu_step. */
int cagpu_step_map(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                   const CaMap *map, void *stream);

/* Replaces: Map.add_agents_to_map (Map.py:46-64) + LaserScanSensor.sense (sensors/LaserScanSensor.py:49-101) for every
 * agent of every env, on the CURRENT state (call after cagpu_reset / cagpu_step): the env's agents are rasterised as
 * discs into a copy of the static grid held in LDS, every beam is marched through it (the agent's own disc is
 * transparent), the result is the range of the last sample before the SECOND hit (the reference's
 * `cumsum == 1` indexing, LaserScanSensor.py:77-81).  An agent with step_num == 0 takes its first measurement (all
 * history rows filled, :84-85), otherwise the history is rolled (:86-88).
 * CA_EUNSUPPORTED, nothing launched: range_res / cell of 6.8 or more, (range_res + 0.01) / cell of 7.8 or more (the LDS grid
 * carries 8 cells of empty border, and a beam is marched from up to one sample before the grid box + 1 cm: below these bounds
 * every sample read lies in the grid or its border, and the indices are the reference's), a map too large for the LDS. */
int cagpu_laserscan(const CaParams *p, const CaState *s, const CaMap *map, const CaScan *scan, void *stream);

/* cagpu_step_map / cagpu_laserscan with a map set (v12): every env tests its walls against, and scans, its OWN map
 * env_map[e].  With set->map_seed != 0 an auto-reset draws the env's next map (CaMapSet.map_seed); the wall test of the
 * terminal step still uses the old map, the next step and the next scan the new one (the reference's reset observation
 * already sees the new map).  Envs with more than 64 agents, the pipelined and the plain step kernels all take a set; the
 * n-step kernels do through cagpu_step_ex_maps only.  cagpu_step_maps = CaStepEx{n_steps = 1, set}; additionally `set` may not be NULL.
 * cagpu_laserscan_maps: CA_EINVAL, nothing launched, for a NULL set and for what cagpu_step_ex rejects of a set. */
int cagpu_step_maps(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                    const CaMapSet *set, void *stream);
int cagpu_laserscan_maps(const CaParams *p, const CaState *s, const CaMapSet *set, const CaScan *scan, void *stream);

/* Replaces: Map.add_agents_to_map (Map.py:46-64) + OccupancyGridSensor.sense (sensors/OccupancyGridSensor.py:24-82) for every
 * agent of every env, on the CURRENT state: the env's dynamic map -- the static grid OR a disc per agent slot around its
 * floored cell, exactly the grid cagpu_laserscan marches through, except that the agent's OWN disc stays in -- is assembled as
 * a bitmap in LDS and every agent's window is cropped from it.  ANCHORING RULE: the window's top-left map cell is
 *   i0 = floor(origin_r - (py + y_width / 2) / cell),  j0 = floor(origin_c + (px - x_width / 2) / cell)
 * (float64, true divisions: the reference's own upper-left corner), out[a, b] = map[i0 + a, j0 + b], 0 for cells outside the
 * map.  DIVERGENCE: the reference computes both corners of the window independently and raises ValueError (a broadcast of
 * 49 or 51 cells into 50) where their floors disagree about the span -- at some "round" positions such as px = -8.8 or
 * py = 8.8 on the 16 m map; this call always returns height x width, identical to the reference wherever the reference
 * returns.  Reads pos_x, pos_y, radius only and writes no simulator state: a pure function of the current state and the env's
 * current map (nothing to do at a reset).  Any num_agents up to 1024.  CA_EINVAL, nothing launched: NULL arguments / state pointers, bad sizes, bad CaMap,
 * both outputs NULL or not 16-byte aligned, height / width outside [1, 256]; CA_EUNSUPPORTED: the map's bitmap
 * (rows x ceil(cols / 32) words) does not fit the LDS.  The _maps form shows every env its OWN map env_map[e]
 * (an index outside the set: empty static part, agents still drawn, bit 2 of the fault word). */
int cagpu_occupancy_grid(const CaParams *p, const CaState *s, const CaMap *map, const CaOccGrid *grid, void *stream);
int cagpu_occupancy_grid_maps(const CaParams *p, const CaState *s, const CaMapSet *set, const CaOccGrid *grid, void *stream);

/* Replaces: visualize.plot_episode / draw_agents (envs/visualize.py:90-257; the per-episode PNG of
 * collision_avoidance_env.py:240-270 and the frames animate_episode glues together) for r->num_frames frames at once,
 * rasterised on the device (csrc/cagpu_render.inc): white background, the env's static grid (dark grey where a pixel centre
 * falls in an occupied cell, Map.py:26-32), then per agent slot the discs along its trajectory (alpha 1 - t / (1.2 max_time)
 * over white, one-pixel rim), the 3-pixel polylines, a goal diamond -- or dots and one disc without circles_along_traj.
 * DIVERGENCES: no text, axes or anti-aliasing, a diamond for the goal star, the map is drawn (the reference has that line
 * commented out, visualize.py:108-109).  Reads pos / goal / radius / flags of the state, the map and `hist`; writes r->out
 * and r->work only: no simulator state, nothing to do at a reset, cagpu_last_kernel() is left alone.  Any num_agents up to
 * 1024; primitives outside the window are clipped.  map may be NULL (or its static_bits): no map.  CA_EINVAL, nothing
 * launched: NULL p / s / r or state pointers, bad sizes, out NULL or not 16-byte aligned, num_frames < 1, height / width
 * outside [16, 1024], xmin / ymax not finite or s16 outside (0, 1e9], frame_env / first / last NULL, hist_steps < 0 or
 * hist_steps > 0 with hist NULL / hist_cols < 1 / a negative stride, hist not 16-byte aligned, a bad CaMap, work NULL /
 * misaligned / too small; the _maps form also: what cagpu_occupancy_grid_maps rejects of a set.  CA_EUNSUPPORTED: more
 * than 2^31 - 1 records per frame or (frame, tile) workgroups.  The _maps form shows every env its OWN map env_map[e] (an
 * index outside the set: no map, bit 2 of the fault word). */
int cagpu_render(const CaParams *p, const CaState *s, const CaMap *map, const CaRender *r, void *stream);
int cagpu_render_maps(const CaParams *p, const CaState *s, const CaMapSet *set, const CaRender *r, void *stream);
/* Bytes of CaRender.work for F frames of N agent slots over a history block of hist_steps slots: 16 F + 32 F N (2 hist_steps + 2)
 * (a 32-byte record per disc, dot, segment and marker; 0 for bad arguments).  Host-only call. */
uint64_t cagpu_render_work_bytes(int32_t num_frames, int32_t num_agents, int32_t hist_steps);

/* Replaces: GA3CCADRLPolicy.find_next_action (policies/GA3CCADRLPolicy.py:49-84) + NetworkVPCore.predict_p
 * (GA3C_CADRL/network.py:24-41, the TF1 graph of the checkpoint) for every agent whose policy is CA_POL_GA3C_CADRL and
 * that is not done: the policy vector X[138] = obs[1:] (zero-padded / cropped), (X - mean) / std, a 64-unit LSTM over
 * the first num_other_agents of the 19 other-agent slots, three 256-wide ReLU layers, logits_p; the argmax (index into
 * network.Actions, network.py:7-16) goes to ext_actions[e,n,0] (and 0 to [e,n,1]), where cagpu_step turns it into
 * [pref_speed * a0, a1] exactly as for CA_POL_LEARNING_GA3C.  obs: device float [E,N,6+7*max_obs], the observation of
 * the CURRENT state (what the reference hands to the policy, collision_avoidance_env.py:319-323) -- or NULL: FUSED SENSING,
 * the kernel computes the ego-centric observation of every agent it evaluates from the state arrays itself
 * (OtherAgentsStatesSensor.sense + the observation assembly, with p->obs_clip / sort_mode / sensing_horizon), bit-identical to
 * the stored row; needs num_agents <= 32 and closest_first / closest_last sorting.  logits (nullable):
 * device float [E,N,11], written for the same agents.  Arithmetic: float32 like the TF graph, on the F16 matrix cores
 * (v_mfma_f32_16x16x32_f16, f32 accumulate): both operands of every contraction are carried as two fp16 planes
 * (x ~ hi + lo, hi = fp16(x), lo = fp16(x - hi): 22 of 24 significant bits, fp16 denormals kept) and three of the four
 * plane products are accumulated -- a product is off by less than
 * 2^-21 of itself (an f32 multiply: 2^-24); layer1's four host inputs and the logits layer run on the exact f32 MFMA
 * (v_mfma_f32_16x16x4_f32; the LSTM does not: that instruction holds the SIMD's VALU).  Logits agree with a float32 evaluation of the graph to ~1e-6 (tests: rtol 1e-4, atol 2e-4).
 * Needs net->packed (cagpu_ga3c_pack). */
int cagpu_ga3c(const CaParams *p, const CaState *s, const float *obs, const CaNet *net, double *ext_actions,
               float *logits, void *stream);

/* Replaces: NetworkVPCore.predict_p / crop_x (GA3C_CADRL/network.py:24-41) and the value fetch `Squeeze:0`
 * (network.py:74, NetworkVP_rnn: logits_v) for ALL `rows` rows of a plain device array x [rows, width] of policy vectors
 * X = obs[1:] (num_other_agents, dist_to_goal, heading_ego_frame, pref_speed, radius, 19 x 7): no simulator, no flag
 * words.  width as crop_x: columns beyond 138 are ignored, missing ones are raw zeros before the normalisation; the
 * sequence length is int(x[:,0]) clamped to 0..19.  Outputs, each nullable (not all): logits [rows,11] (logits_p before
 * the softmax), value [rows] (needs value_kernel / value_bias = logits_v/{kernel [256,1], bias [1]}, device float32),
 * action int32 [rows] (first maximum of the logits, like np.argmax).  The same kernel code and arithmetic as cagpu_ga3c
 * (a row's results are bit-identical to the simulator path's on the same observation); the value is the twelfth column
 * of the padded logits block on the exact f32 MFMA.  rows == 0: CA_OK, nothing launched.  rows >= 2^31:
 * CA_EUNSUPPORTED.  net->rows_scratch / agent_net are not used.  The fp16-range guard (cagpu_device_faults bit 1)
 * applies.  cagpu_last_kernel() names the launch "ga3c_kernel<true> query ...". */
typedef struct CaNetQuery {
  const float *x;                          /* device float32 [rows, width], row-major */
  int64_t rows;
  int32_t width, reserved0;
  const float *value_kernel, *value_bias;  /* logits_v; both NULL: no value */
  float *logits;                           /* [rows, 11] or NULL */
  float *value;                            /* [rows] or NULL */
  int32_t *action;                         /* [rows] or NULL */
} CaNetQuery;
int cagpu_ga3c_query(const CaNet *net, const CaNetQuery *q, void *stream);

/* cagpu_ga3c with the value head: value [E,N] (device float32) is written for exactly the agents cagpu_ga3c evaluates
 * (live GA3C-CADRL agents, of this checkpoint with CaNet.agent_net), every other entry is left alone.  Replaces: the
 * `Squeeze:0` fetch of the reference's find_next_action_and_value-style callers (network.py:74) for those agents.
 * v == NULL: exactly cagpu_ga3c (the same launch).  All three members of v are required.  ext_actions and logits are
 * bit-identical to cagpu_ga3c's.  cagpu_last_kernel() names the launch "ga3c_kernel<true> sim ...". */
typedef struct CaNetValue {
  const float *value_kernel, *value_bias;  /* logits_v/{kernel [256,1], bias [1]} */
  float *value;                            /* [E, N] */
} CaNetValue;
int cagpu_ga3c_value(const CaParams *p, const CaState *s, const float *obs, const CaNet *net, double *ext_actions,
                     float *logits, const CaNetValue *v, void *stream);

/* The size of CaNet.packed, and the one-time split of a checkpoint's weights into it: reads net->lstm_kernel,
 * layer1_kernel, layer2_kernel, fc1_kernel (device float32, the checkpoint's [in, out] layout) and writes `bytes` =
 * cagpu_ga3c_packed_bytes() bytes at `packed` (device, 16-byte aligned); the LSTM kernel's columns are stored multiplied (in
 * float32) by -log2 e (gates i, f, o) / -2 log2 e (gate j): the kernel evaluates the gates as 1 / (1 + 2^z).  Replaces nothing in the reference (TF keeps its
 * variables in one layout); it is this library's equivalent of GA3CCADRLPolicy.initialize_network's checkpoint restore
 * (GA3CCADRLPolicy.py:23-47).  Call again after changing a weight array. */
uint64_t cagpu_ga3c_packed_bytes(void);
int cagpu_ga3c_pack(const CaNet *net, void *packed, uint64_t bytes, void *stream);

/* Replaces: generate_rand_test_case_multi (envs/policies/CADRL/scripts/multi/gen_rand_testcases.py:111-444) behind
 * test_cases.get_testcase_random (envs/test_cases.py:212-253), for num_cases scenarios at once: 15 % two-agent swap +
 * circle, 15 % circle, 70 % rejection-sampled starts / goals in a square of half side `side` (drawn per case from
 * [side_lo, side_hi] when side_hi > side_lo) that grows 1 % per attempt.  cases: device float64 [num_cases, num_agents, 6]
 * = px, py, gx, gy, pref_speed, radius -- the layout cagpu_reset and CaAutoReset.table take.  Randomness is
 * counter-based (Philox4x32-10 keyed by `seed`, counter = (draw, case index)): the same (seed, case index) gives the
 * same scenario whatever num_cases is.  status: device int32 [num_cases] or NULL (0 = every agent was accepted by the
 * reference's rules; 1 = an agent hit the attempt cap and was placed anyway). */
int cagpu_generate_cases(int64_t num_cases, int32_t num_agents, double side_lo, double side_hi, double speed_lo,
                         double speed_hi, double radius_lo, double radius_hi, uint64_t seed, double *cases, int32_t *status,
                         void *stream);

/* The same generator for RAGGED tables -- test_cases.get_testcase_random with num_agents=None and a side_length list
 * (envs/test_cases.py:224-241, the reference's default TEST_CASE_ARGS, config.py:118-131): the agent count of a case is
 * drawn first, uniform over n_min .. n_max (np.random.randint(2, MAX_NUM_AGENTS_IN_ENVIRONMENT + 1)), then the side
 * length from every entry of side_ranges (HOST float64 [n_ranges, 4] = count lo, count hi (exclusive), side lo, side hi;
 * n_ranges <= 8) that holds the count; every count in [n_min, n_max] must be held by an entry (the reference asserts it).
 * cases: device float64 [num_cases, max_agents, 6]; rows past the drawn count are zero (radius 0 = an empty slot of a
 * ragged batch, CaParams.ragged).  counts: device int32 [num_cases] or NULL. */
int cagpu_generate_cases_ragged(int64_t num_cases, int32_t max_agents, int32_t n_min, int32_t n_max,
                                const double *side_ranges, int32_t n_ranges, double speed_lo, double speed_hi,
                                double radius_lo, double radius_hi, uint64_t seed, double *cases, int32_t *counts,
                                int32_t *status, void *stream);

/* The same generator at EXPLICIT 64-bit case indices (additive to v12), one WAVE per case: entry m of the list generates
 * scenario(seed, case_index[m]) -- bit for bit what cagpu_generate_cases / _ragged give that index -- into row out_row[m]
 * of cases / counts / status.  The arguments are those of cagpu_generate_cases_ragged with num_cases replaced by the list:
 *   case_index  device int64 [M]: the case indices (the Philox counter takes all 64 bits);
 *   out_row     device int64 [M] or NULL (row m): where each case lands; the caller keeps the rows inside its table and
 *               distinct;
 *   count       device int32 [1] or NULL (M): only the first min(*count, M) entries are processed, read ON THE DEVICE --
 *               grid and block depend on M only, so a work list built on the device needs no host read-back; the rows of
 *               the other entries are left alone.
 * n_max = 0: every case has max_agents agents.  n_ranges = 0: side_ranges is HOST float64 [2] = side lo, hi, the plain form
 * of cagpu_generate_cases (a draw per case only when hi > lo).  The 64 lanes of a wave evaluate 64 consecutive attempts of
 * the current agent's rejection loop at once and the first accepted one wins (csrc/cagpu_gen.inc):
 * fast on a short list, where one thread per case leaves a wave mostly idle.  CA_EINVAL, nothing launched: M outside
 * 1 .. 2^31 - 1, NULL case_index / cases / side_ranges, max_agents outside 1 .. 1024, n_ranges < 0, and what
 * cagpu_generate_cases_ragged rejects of the distribution. */
int cagpu_generate_cases_at(const int64_t *case_index, const int64_t *out_row, const int32_t *count, int64_t M,
                            int32_t max_agents, int32_t n_min, int32_t n_max, const double *side_ranges, int32_t n_ranges,
                            double speed_lo, double speed_hi, double radius_lo, double radius_hi, uint64_t seed,
                            double *cases, int32_t *counts, int32_t *status, void *stream);

/* CASE STREAM (additive to v12; cagpu_stream_refill): a fresh random scenario at EVERY on-device auto-reset -- the batched
 * form of the reference's default Config.TEST_CASE_FN = "get_testcase_random" (config.py:50-62, test_cases.py:212-253),
 * which builds a new scenario at every reset() -- without a step kernel knowing: the CaAutoReset's table is a WINDOW of
 * W upcoming episodes per env that a refill keeps ahead of the envs.
 * THE RULE, stated once.  With CaAutoReset{table = this table, n_cases = E * W, case_stride = E} the k-th auto-reset of
 * env e loads row (env_id_offset + e + k * E) % (E * W): slot k % W of env e's own W rows.  Write rc for reset_count[e] as a
 * refill sees it: after that refill the rows of episodes rc + 1 .. rc + W hold
 *     scenario(seed, case index = (g << 32) | k),   g = env_id_offset + e (the global env id, required < 2^32), k the episode
 * -- a pure function of (seed, global env id, episode), whatever the batch size, the sharding, the window or the launch
 * pattern.  A refill regenerates exactly the slots whose `held` entry differs from the episode they must hold, so it only
 * ever replaces rows of episodes <= rc.  OVERRUN: an env that auto-resets more than W times between two refills loads a
 * slot that still holds an older episode -- a repeated scenario, never uninitialised memory; the next refill sees
 * reset_count[e] - seen[e] > W and raises bit 3 of the fault word (cagpu_device_faults).
 * reset_obs / reset_plan of the CaAutoReset must be NULL (the rows change under them): the kernels re-sense after an
 * auto-reset and query the new episode's first action at the start of its step, as with heading_seed != 0 / a policy draw. */
typedef struct CaCaseStream {
  double  *table;       /* device [E * W, N, 6]: the window, the table the CaAutoReset points at */
  int32_t *held;        /* device [E, W]: the episode each window slot holds; the caller initialises it to -1 */
  int32_t *seen;        /* device [E]: reset_count[e] at the last refill; the caller initialises it to 0 */
  int64_t *work_index;  /* device [E * W] scratch: the case indices of the stale slots (order unspecified) ...       */
  int64_t *work_row;    /* device [E * W] scratch: ... and their rows                                               */
  int32_t *work_count;  /* device [1] scratch: how many (zeroed by every refill)                                      */
  int32_t *counts;      /* device [E * W] or NULL: the agent count of every row (cagpu_generate_cases_at's counts)   */
  int32_t *status;      /* device [E * W] or NULL: its status                                                        */
  int32_t  window;      /* W >= 1 */
  int32_t  n_min, n_max, n_ranges;   /* the distribution, as cagpu_generate_cases_at takes it */
  const double *side_ranges;         /* HOST [n_ranges, 4], or [2] with n_ranges = 0 */
  double   speed_lo, speed_hi, radius_lo, radius_hi;
  uint64_t seed;
} CaCaseStream;                      /* 128 bytes */

/* One refill, stream-ordered and without any host synchronisation: a small kernel (one thread per (env, slot)) compares
 * `held` with the episode each slot must hold, compacts the stale slots into the work list (wave ballot + one atomic per
 * wave), stamps `held` and `seen` and raises the overrun bit; the wave-per-case generator then runs over the list with the
 * count read on the device.  Of `s` only reset_count is read.  Call it where the device state is the state last handed
 * out (ahead of a rollout / ring launch, every W - 1 single steps).  CA_EINVAL, nothing launched: NULL p / s / ar / cs, bad
 * sizes, NULL reset_count, window < 1, num_envs * window > 2^31 - 1, a NULL pointer among table / held / seen / work_*, a
 * CaAutoReset that does not name the window (table, n_cases = num_envs * window, case_stride = num_envs) or carries
 * reset_obs / reset_plan, env_id_offset < 0 or env_id_offset + num_envs > 2^32, and what cagpu_generate_cases_at rejects
 * of the distribution (num_agents > 1024 included). */
int cagpu_stream_refill(const CaParams *p, const CaState *s, const CaAutoReset *ar, const CaCaseStream *cs, void *stream);

/* n_steps consecutive cagpu_step calls fused into ONE launch: = CaStepEx{n_steps}. */
int cagpu_rollout(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions,
                  const CaAutoReset *ar, int32_t n_steps, void *stream);

/* cagpu_rollout whose every step KEEPS its outputs: the look-ahead ring behind `env.step(None)`.  With every policy internal
 * the reference's `env.step(None)` needs no input from the host (experiments/src/env_utils.py:45-52: `run_episode` passes
 * None until the episode is over), so the next n_steps steps can be computed in one launch and handed out one by one -- but
 * a gym caller wants the outputs of EVERY step, not only the last one's.  Here the output pointers of `o` name slot 0 of a
 * ring of n_steps slots and step t of the call (t = 0 .. n_steps - 1) writes slot t:
 *   o->obs [n_steps, E, N, 6+7K], o->rewards [n_steps, E, N], o->done [n_steps, E, N], o->game_over [n_steps, E],
 *   o->actions / o->orca_vel (if given) [n_steps, E, N, 2].
 * State, statistics and auto-resets are those of cagpu_rollout(n_steps) -- i.e. of n_steps cagpu_step calls, bit for bit
 * (tests/test_gpu_ring.py).  = CaStepEx{n_steps, ring = 1, snapshot_delta}.
 * snapshot_delta (bytes; 0 = none): the REWIND POINT.  A caller that runs ahead must be able to go back (an action arrives
 * for step t < n_steps: restore the state the call started from, cagpu_rollout(t), go on one step at a time).  With all state
 * arrays of `s` in ONE allocation and a second allocation of the same layout snapshot_delta bytes away, the kernel itself
 * stores every state element it loads at its start -- all of `s` that a step reads or writes, env_stats included -- at
 * (its address + snapshot_delta): when the call has run, the second allocation holds the state BEFORE the call.  Only the
 * pipelined n-step kernel does this (cagpu_ring_snapshots() says whether a call with these arguments would); otherwise
 * CA_EUNSUPPORTED and the caller copies the state itself ahead of the call. */
int cagpu_rollout_ring(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions,
                       const CaAutoReset *ar, int32_t n_steps, int64_t snapshot_delta, void *stream);
/* 1: cagpu_rollout_ring with these arguments runs the kernel that takes the snapshot itself (snapshot_delta != 0 accepted);
 * 0: it does not; < 0: the arguments are invalid (CA_E*).  Host-only, launches nothing. */
int cagpu_ring_snapshots(const CaParams *p, const CaState *s, const CaOut *o, const CaAutoReset *ar, int32_t n_steps);

/* The step / rollout calls that also RECORD every agent's trajectory row (CaTraj):
 *   cagpu_step_traj     = CaStepEx{n_steps = 1, map, set, traj}
 *   cagpu_rollout_traj  = CaStepEx{n_steps, ring, snapshot_delta, traj}
 * Additionally `traj` may not be NULL. */
int cagpu_step_traj(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                    const CaMap *map, const CaMapSet *set, const CaTraj *traj, void *stream);
int cagpu_rollout_traj(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                       int32_t n_steps, int32_t ring, int64_t snapshot_delta, const CaTraj *traj, void *stream);

/* The step / rollout calls that also keep the FINAL RECORD (CaFinal), with or without the tape:
 *   cagpu_step_final    = CaStepEx{n_steps = 1, map, set, traj, fin}
 *   cagpu_rollout_final = CaStepEx{n_steps, ring, snapshot_delta, traj, fin}
 * Additionally `fin` may not be NULL (`traj` may). */
int cagpu_step_final(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                     const CaMap *map, const CaMapSet *set, const CaTraj *traj, const CaFinal *fin, void *stream);
int cagpu_rollout_final(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                        int32_t n_steps, int32_t ring, int64_t snapshot_delta, const CaTraj *traj, const CaFinal *fin,
                        void *stream);

/* The step / rollout calls that also write the EPISODE LOG (CaEpLog), with or without the tape and the final record:
 *   cagpu_step_log      = CaStepEx{n_steps = 1, map, set, traj, fin, log}
 *   cagpu_rollout_log   = CaStepEx{n_steps, ring, snapshot_delta, traj, fin, log}
 * Additionally `log` may not be NULL (`traj` and `fin` may). */
int cagpu_step_log(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                   const CaMap *map, const CaMapSet *set, const CaTraj *traj, const CaFinal *fin, const CaEpLog *log,
                   void *stream);
int cagpu_rollout_log(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                      int32_t n_steps, int32_t ring, int64_t snapshot_delta, const CaTraj *traj, const CaFinal *fin,
                      const CaEpLog *log, void *stream);

/* POLICY DRAW (additive to v12; cagpu_step_draw / cagpu_policy_draw): which policy every agent of a NEW episode runs, drawn
 * at the auto-reset itself -- the batched form of test_cases.py cadrl_test_case_to_agents,
 *     names = np.random.choice(policies, num_agents, p=policy_distr)
 *     if policy_to_ensure not in names: names[np.random.randint(len(names))] = policy_to_ensure
 * THE RULE, stated once.  For env e: g = CaAutoReset.env_id_offset + e (the global env id), k = CaState.reset_count[e] of
 * the new episode (AFTER the auto-reset's increment), u(c) = the Philox4x32-10 uniform of key `seed` and counter
 * (g lo, g hi, k, c) -- the construction of CaAutoReset.heading_seed's draws.  The PRESENT slots are those whose new case
 * row has radius > 0 (every slot unless CaParams.ragged).
 *   1. present slot a draws pool index j_a = #{j : cdf[j] <= u(a)}, clamped to P - 1 (np.searchsorted(cdf, u, 'right'):
 *      what np.random.choice does);
 *   2. if ensure >= 0 and no present slot drew `ensure`: r = min(floor(n u(0xFFFFFFFE)), n - 1), n the number of present
 *      slots, and the r-th present slot in slot order takes `ensure`;
 *   3. a present slot's flag word becomes (flags & ~0xFC0) | policy_bits[j]; absent slots keep theirs.
 * A pure function of (seed, g, k): single launches, cagpu_rollout, a ring, a rewind's replay and every shard layout draw
 * the same bits, and no lane needs another lane's result (each recomputes its env's draws; the large-env kernel shares them
 * through LDS).  Bits 12 and up (dynamics, CA_ABSENT, CA_PLAN_VALID) and bits 0 - 5 are never touched by the draw. */
typedef struct CaPolicyDraw {
  const double   *cdf;          /* device [P]: cumsum(policy_distr) / its last element, as np.random.choice computes it */
  const uint32_t *policy_bits;  /* device [P]: bits 6..11 of the flag word of pool entry j (CA_IS_LEARNING,
                                   CA_STILL_LEARNING, the policy id); other bits are ignored */
  int32_t         num_policies; /* P in 1..8 */
  int32_t         ensure;       /* -1, or the pool index every episode must hold */
  uint64_t        seed;         /* != 0, and != CaAutoReset.heading_seed (equal keys would make the heading and the policy
                                   of an agent the same uniform) */
} CaPolicyDraw;                 /* 32 bytes */

/* cagpu_step_ex + the draw at every auto-reset of the call.  d == NULL: exactly cagpu_step_ex.  Otherwise CA_EINVAL, nothing
 * launched (reported behind "snapshot_delta without ring" and ahead of the records): d->cdf or d->policy_bits NULL,
 * num_policies outside 1..8, ensure outside -1 .. P - 1, seed == 0, ar == NULL (no table, no auto-reset, nothing is ever
 * drawn), seed == ar->heading_seed.  Everything of `x` holds as in cagpu_step_ex (a map or a map set: single steps only).
 * With the draw on, CaAutoReset.reset_plan is not used (a plan belongs to the policy it was made for): an env that reset
 * starts its episode without a valid plan and is queried on the pre-move state; column 0 (is_learning) of a row copied from
 * CaAutoReset.reset_obs is written from the drawn bits.  The pipelined kernels draw in their " final" instantiations
 * (cagpu_last_kernel() shows " draw"); without a draw no kernel selection and no kernel code changes. */
int cagpu_step_draw(const CaParams *p, const CaState *s, const CaOut *o, const double *ext_actions, const CaAutoReset *ar,
                    const CaStepEx *x, const CaPolicyDraw *d, void *stream);

/* The same rule applied to the CURRENT state, for the episode k = reset_count[e] each env is in (after cagpu_reset: k = 0,
 * which also needs its lottery) -- a small kernel of its own, envs with env_mask[e] == 0 untouched (NULL: all).  Present
 * slots are those without CA_ABSENT (every slot unless CaParams.ragged); their flag words are rewritten by step 3 and lose
 * CA_PLAN_VALID (a plan belongs to the policy it was made for).  o != NULL: column 0 of the present slots' rows of o->obs
 * is rewritten from the drawn bits as well (o->obs only; the other members are not read).  Of `ar` only env_id_offset and
 * heading_seed are read.  CA_EINVAL, nothing launched: what cagpu_step_draw rejects of d and ar, NULL p / s / d, bad sizes,
 * NULL s->flags / s->reset_count, o given with o->obs NULL. */
int cagpu_policy_draw(const CaParams *p, const CaState *s, const CaOut *o, const CaAutoReset *ar, const CaPolicyDraw *d,
                      const uint8_t *env_mask, void *stream);

/* THE DRAWS OF AN EPISODE'S ADDRESS (additive to v12): the two auto-reset rules above for ARBITRARY (global env id, episode)
 * pairs, as cagpu_map_draw gives the map of a map set and cagpu_generate_cases_at the scenario of a case stream -- with
 * them the start state of any episode of a batch is rebuilt from (seed, global env id, episode number) alone.  Both kernels
 * call the device functions the step kernels call (no rule is stated twice).  env_ids device int64 [n], counts device
 * int32 [n]; pair i is the env with global id env_ids[i] at its counts[i]-th auto-reset (counts[i] >= 1 for an auto-reset;
 * cagpu_policy_draw's episode 0 is counts[i] = 0).
 *   cagpu_heading_draw    out[i, a] (device double [n, num_agents]) = the heading slot a takes under
 *                         CaAutoReset.heading_seed = heading_seed: uniform in [-pi, pi).  One thread per (pair, slot).
 *   cagpu_policy_draw_at  steps 1 and 2 of CaPolicyDraw's rule: out_bits[i, a] = policy_bits[j] & 0xFC0 of the pool entry
 *                         slot a ends up with; `present` (device uint8 [n, num_agents], NULL: every slot) names the slots
 *                         that hold an agent -- the ensure rule counts over them -- and an absent slot gets 0xFFFFFFFF.
 *                         One wave per pair.
 * n == 0: nothing is launched.  CA_EINVAL, nothing launched: a NULL pointer (present excepted), heading_seed == 0, n < 0,
 * num_agents outside 1..1024, and of d what cagpu_step_draw rejects of d alone (cdf / policy_bits NULL, num_policies
 * outside 1..8, ensure outside -1 .. P - 1, seed == 0).  env_ids and counts live on the device and are not read by the
 * host, as in cagpu_map_draw: an id is taken as the 64-bit counter pair (lo, hi) it spells and a count as the 32-bit word
 * it spells -- whoever holds them on the host (BatchedSim.episode_start) rejects ids outside [0, 2^32) and negative
 * counts there. */
int cagpu_heading_draw(uint64_t heading_seed, int32_t num_agents, const int64_t *env_ids, const int32_t *counts, int64_t n,
                       double *out, void *stream);
int cagpu_policy_draw_at(const CaPolicyDraw *d, int32_t num_agents, const int64_t *env_ids, const int32_t *counts,
                         const uint8_t *present, int64_t n, uint32_t *out_bits, void *stream);

/* RVO DRAW (additive to v12): RVOPolicy's two stochastic branches -- anti-collaborative agents (RVOPolicy.py:77-90,
 * Config.RVO_COLLAB_COEFF < 0) and `heading_noise` (RVOPolicy.py:118-119) -- drawn INSIDE the step kernels as a pure function
 * of (seed, global env id, episode, agent slot, episode step), so that a batch with them runs in fused launches, a look-ahead
 * ring, any shard layout and a replay with the same numbers.  (CaState.rvo_collab / rvo_heading_noise, the caller's own
 * numbers for ONE step, stay as they are.)
 *
 * Address of a draw: the queried agent's
 *   g  global env id: env_id_offset + e with a CaAutoReset, e without one;
 *   k  episode: CaState.reset_count[e] as the step finds it (what the heading draw and the policy draw use);
 *      `address` != NULL overrides both: env e draws as (g, k) = (address[2e], address[2e + 1]) whatever its reset count is
 *      (a replay's child batch runs episode k of env g as its local env e);
 *   a  agent slot, 0 .. num_agents - 1 <= 1023;
 *   s  the agent's CaState.step_num as the query sees it (the pre-move state), 0 <= s < 2^22.  A queried agent with
 *      s >= 2^22 is outside the rule: its draw uses the low 22 bits and bit 4 of the fault word is raised.
 * Blocks: B0 = philox4x32_10(counter = (g & 0xFFFFFFFF, g >> 32, k, (s << 10) | a), key = (seed & 0xFFFFFFFF, seed >> 32)),
 *         B1 = the same with counter word 2 = k | 0x80000000 (k >= 0: no episode's B0 is another's B1).
 * Two words w, w' of a block give a uniform in [0, 1) with 53 bits: ((w >> 5) * 2^26 + (w' >> 6)) / 2^53.
 *   u0 = B0 words 0, 1;  u1 = B0 words 2, 3;  v0 = B1 words 0, 1.
 * Who draws: an agent that is QUERIED in the step -- present, not CA_DONE, policy CA_POL_RVO.  Every other slot draws
 * nothing and its CA_RVO_NONCOOP bit is not touched by the query.
 * Anti-collaboration (collab_coeff = c < 0, anti_collab_t = T, DT = CaParams.rvo_dt; all float64): with t the agent's clock
 *   CaState.t before the move and m = fmod(t, T), the bit CA_RVO_NONCOOP of the agent's flag word is REDRAWN when
 *       rint(m * 1000.0) / 1000.0 < DT   or   rint((T - m) * 1000.0) / 1000.0 < DT
 *   (rint: to nearest, ties to even) as  bit = (u0 < 1.0 - fabs(c)),  and kept otherwise.  The query then runs ORCA with the
 *   ego's collaboration coefficient 0.0f while the bit is set and (float)c otherwise (CaParams.rvo_collab_coeff is not
 *   read).  t = 0 lies in the window, so the first query of every episode redraws; an auto-reset under such a CaRvoDraw
 *   clears the bit of all slots of the env, which makes every episode a function of its start state and its address.
 *   The bit is stored with the flag word the step stores anyway.  c >= 0 (or NaN): this branch is off, nothing reads or
 *   writes the bit and the coefficient is CaParams.rvo_collab_coeff.
 * Heading noise (noise_mask != NULL): the float64 delta heading of EVERY queried agent gets
 *       dh = dh + (noise_mask[e * N + a] ? noise_std * z : 0.0),   z = sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * v0)
 *   before it is rounded to the float32 action (an unmasked agent adds +0.0).  z is standard normal (Box-Muller); the
 *   device's libm evaluates it, so it is reproducible on the device (cagpu_rvo_draw_at) and to a few ulp elsewhere.
 * Kernels: the general kernel (single-step and n-step) and the large-env kernel; a launch with a CaRvoDraw never takes the
 * pipelined kernel and is given no next_action / reset_plan plan.  cagpu_last_kernel() ends in " noise". */
typedef struct CaRvoDraw {
  uint64_t       seed;          /* != 0, != heading_seed, != the policy draw's seed, != map_seed */
  double         collab_coeff;  /* < 0: anti-collaborative agents; >= 0: that branch is off */
  double         anti_collab_t; /* Config.RVO_ANTI_COLLAB_T, > 0 (read where collab_coeff < 0) */
  double         noise_std;     /* >= 0 (the reference: 0.5) */
  const uint8_t *noise_mask;    /* device [E*N]; NULL = that branch off */
  const int64_t *address;       /* device [2*E] (g, k) per env, 8-byte aligned, or NULL (above) */
} CaRvoDraw;                    /* 48 bytes */

/* cagpu_step_tape with a CaRvoDraw.  rd == NULL: exactly cagpu_step_tape -- the same launch, the same bits, the same
 * cagpu_last_kernel() string.  With rd every rule of cagpu_step_tape holds in its own words, and BEHIND the tape's
 * rejections in the order of first-reported errors stand, each CA_EINVAL with nothing launched:
 *   CaState.rvo_collab / rvo_heading_noise beside a CaRvoDraw (one source of these numbers per launch);
 *   seed == 0, or seed equal to CaAutoReset.heading_seed, CaPolicyDraw.seed or CaMapSet.map_seed of the call;
 *   collab_coeff < 0 with anti_collab_t not > 0;  noise_std negative or NaN;
 *   both branches off (collab_coeff not < 0 and noise_mask == NULL);  address not 8-byte aligned. */
int cagpu_step_noise(const CaParams *p, const CaState *s, const CaOut *o, const CaActionTape *tape, const CaAutoReset *ar,
                     const CaStepEx *x, const struct CaPolicyDraw *draw, const CaRvoDraw *rd, void *stream);

/* The rule above for n arbitrary addresses, by the device functions the step kernels call: one thread per address
 * (g[i], k[i], a[i], s[i]) -- device int64 / int32 / int32 / int32 [n] --
 *   out_noncoop_draw[i] (device uint8, may be NULL) = (u0 < 1 - |collab_coeff|): what a redraw at that address gives;
 *   out_noise[i]        (device double, may be NULL) = noise_std * z: what a MASKED agent adds (the mask is taken as "all").
 * rd->noise_mask and rd->address are not read.  n == 0: nothing is launched.  CA_EINVAL, nothing launched: rd or an
 * address array NULL, both outputs NULL, seed == 0, noise_std negative or NaN, num_agents outside 1..1024, n < 0. */
int cagpu_rvo_draw_at(const CaRvoDraw *rd, int32_t num_agents, const int64_t *g, const int32_t *k, const int32_t *a,
                      const int32_t *s, int64_t n, uint8_t *out_noncoop_draw, double *out_noise, void *stream);

/* SAMPLED GA3C-CADRL POLICY (additive to v12): the action of a GA3C-CADRL agent drawn from the softmax of its logits as a
 * pure function of (seed, global env id, episode, agent slot, episode step) and the logits row, with its log-probability and
 * the row's entropy -- what an on-policy method needs beside the value head (cagpu_ga3c_value).  A launch of its own that
 * runs AFTER cagpu_ga3c / cagpu_ga3c_value (which wrote `logits` and the argmax into ext_actions) and BEFORE the step; no
 * network kernel and no step kernel is touched.
 *
 * Who is evaluated: exactly the agents the network launch evaluated -- present, not CA_DONE, policy CA_POL_GA3C_CADRL, and
 *   with agent_net != NULL only those with agent_net[i] == net_index.  Entries of every other agent are left alone.
 * Who samples: an evaluated agent whose byte in `mask` (device uint8 [E*N]) is set; mask == NULL: every evaluated agent;
 *   greedy != 0: nobody (seed is then neither read nor checked).  A sampling agent's ext_actions[e, n, 0] is overwritten with
 *   the sampled index (and [e, n, 1] with 0.0); every other evaluated agent plays the index it holds, the first maximum of
 *   its row.
 * Address (g, k, a, s): CaRvoDraw's, word for word -- g = env_id_offset + e with a CaAutoReset and e without one, k =
 *   CaState.reset_count[e], `address` != NULL overrides both per env ((g, k) = (address[2e], address[2e + 1]): a replay's
 *   child batch), a the agent slot, s the agent's CaState.step_num before the move, 0 <= s < 2^22; an evaluated agent that
 *   samples at s >= 2^22 uses the low 22 bits and raises bit 4 of the fault word.
 * Uniform: u = words 0, 1 of block B0 of that address (CaRvoDraw: counter (g lo, g hi, k, (s << 10) | a)) under the key
 *   `seed`, 53 bits: ((w0 >> 5) * 2^26 + (w1 >> 6)) / 2^53.  seed != 0, and different from CaAutoReset.heading_seed,
 *   CaPolicyDraw.seed, CaMapSet.map_seed and CaRvoDraw.seed of the structs passed along.
 * Probabilities, float32, in index order j = 0 .. 10, every operation rounded on its own (no fused multiply-add):
 *   inv_T = 1.0f / temperature (divided on the host);   m = max_j l_j;   z_j = (l_j - m) * inv_T;   q_j = expf(z_j);
 *   c_j = c_(j-1) + q_j (c_-1 = 0);   S = c_10.
 * Choice: the first j with (float)u * S < c_j, and 10 if there is none (np.random.choice's
 *   searchsorted(cdf, u, side="right") without the division by S).
 * Outputs, for EVERY evaluated agent, with i the index that is played (sampled, or held):
 *   logp    = z_i - logf(S)
 *   entropy = logf(S) - (sum_j q_j * z_j) / S       (products rounded, summed in index order, one correctly rounded divide)
 *   action  = i as int8
 * Bad rows: a row with a NaN logit plays index 0 if it samples (the held index otherwise), gets logp = entropy = NaN and
 *   raises bit 5 of the fault word (cagpu_device_faults).
 * expf / logf are the device libm's (<= 2 ulp): reproducible on the device (cagpu_ga3c_sample_at), to a few ulp elsewhere.
 *
 * The pre-step half of an experience tape slot (all four nullable, independent of each other), written by the same launch:
 *   slot_obs     float32 [E, N, W - 1]  the row the network read (obs[e, n, 1:], W = 6 + 7 max_obs) of every evaluated agent
 *   slot_value   float32 [E, N]         value[e, n] of every evaluated agent (`value`: what cagpu_ga3c_value wrote)
 *   slot_live    uint8   [E, N]         1 for an evaluated agent, 0 for every other slot (written for ALL slots)
 *   slot_address int64   [E, 2]         (g, k) of every env
 * logp / entropy / action may point into a tape slot as well. */
typedef struct CaGa3cSample {
  uint64_t       seed;          /* != 0 and no other rule's seed (unless greedy) */
  float          temperature;   /* > 0, finite */
  int32_t        greedy;        /* != 0: nobody samples; the outputs are those of the held argmax */
  const uint8_t *mask;          /* device [E*N] or NULL = every evaluated agent samples */
  const int32_t *agent_net;     /* device [E*N] or NULL (CaNet.agent_net) */
  int32_t        net_index;
  int32_t        reserved0;
  const int64_t *address;       /* device [2*E], 8-byte aligned, or NULL */
  const float   *logits;        /* device [E,N,11]: what the network launch wrote */
  float         *logp;          /* device [E,N] */
  float         *entropy;       /* device [E,N] or NULL */
  int8_t        *action;        /* device [E,N] or NULL */
  const float   *obs;           /* device [E,N,W]: needed with slot_obs */
  const float   *value;         /* device [E,N]: needed with slot_value */
  float         *slot_obs;
  float         *slot_value;
  uint8_t       *slot_live;
  int64_t       *slot_address;
} CaGa3cSample;                 /* 128 bytes */

/* CA_EINVAL, nothing launched: p, s, g, ext_actions, g->logits, g->logp or CaState.flags / step_num / reset_count NULL;
 * num_agents outside 1..1024; without greedy a seed of 0 or one that equals ar->heading_seed, draw->seed, set->map_seed or
 * rd->seed (ar, draw, set and rd may each be NULL: the call has no such rule); temperature not > 0 or not finite; address not
 * 8-byte aligned; slot_obs without obs, slot_value without value.  Asynchronous on `stream`; cagpu_last_kernel() keeps
 * naming the network launch. */
int cagpu_ga3c_sample(const CaParams *p, const CaState *s, const CaAutoReset *ar, const struct CaPolicyDraw *draw,
                      const CaMapSet *set, const CaRvoDraw *rd, const CaGa3cSample *g, double *ext_actions, void *stream);

/* The rule above for n arbitrary (address, logits row) pairs, every row sampling, with no simulator: g / k / a / s device
 * int64 / int32 / int32 / int32 [n], logits device float32 [n, 11]; action (int8), logp, entropy device [n], each may be
 * NULL (not all three).  n == 0: nothing is launched.  CA_EINVAL, nothing launched: an input pointer NULL, no output, seed
 * == 0, temperature not > 0 or not finite, num_agents outside 1..1024, n < 0. */
int cagpu_ga3c_sample_at(uint64_t seed, float temperature, int32_t num_agents, const int64_t *g, const int32_t *k,
                         const int32_t *a, const int32_t *s, const float *logits, int64_t n, int8_t *action, float *logp,
                         float *entropy, void *stream);

/* Generalised advantage estimation over an experience tape of n steps: reward, value float32 [n, EN]; live, done uint8
 * [n, EN]; game_over uint8 [n, EN / num_agents]; last_value float32 [EN] (the value of the observation after step n - 1);
 * adv, ret float32 [n, EN] (all device).  One lane per (env, agent) column i, float32, every product and sum rounded on
 * its own, gl = gamma * lambda multiplied once on the host in float32:
 *   carry = 0; nv = last_value[i]
 *   for t = n - 1 .. 0:
 *     if !live[t, i]:                        adv[t, i] = ret[t, i] = 0; carry = 0; nv = 0; continue
 *     if done[t, i] | game_over[t, i / N]:   nv = 0; carry = 0        (the agent's episode ended in step t: terminal)
 *     delta = (reward[t, i] + gamma * nv) - value[t, i]
 *     carry = delta + gl * carry
 *     adv[t, i] = carry; ret[t, i] = carry + value[t, i]; nv = value[t, i]
 * Every ending is terminal, a time-out included: the network is never queried on a terminal observation, so there is
 * nothing to bootstrap from.  CA_EINVAL, nothing launched: a NULL pointer, n < 1, EN < 1, EN not a multiple of num_agents,
 * gamma or lambda outside [0, 1]. */
int cagpu_gae(int32_t n, int64_t EN, int32_t num_agents, const float *reward, const float *value, const float *last_value,
              const uint8_t *live, const uint8_t *done, const uint8_t *game_over, float gamma, float lambda, float *adv,
              float *ret, void *stream);

/* The policy query of the NEXT step ahead of time (collision_avoidance_env.py:305-323 for the built-in RVO policy):
 * fills s->next_action from the CURRENT state and sets CA_PLAN_VALID, without stepping.  cagpu_step / cagpu_rollout keep
 * the plan up to date by themselves; this entry point exists for states that did not come out of a step (the reset state
 * of a fixture table -> CaAutoReset.reset_plan).  Requires what the pipelined step kernel requires: s->next_action,
 * num_agents in {2, 3, 4, 5, 6, 8, 10}, closest_first sorting (CA_EUNSUPPORTED otherwise: the step kernels then query the
 * policy at the start of the step).  A plan is computed under the CaParams of THIS call (rvo_time_horizon,
 * rvo_collab_coeff, rvo_dt, sensing_horizon, rvo_max_neighbors): whoever changes one of them afterwards must clear
 * CA_PLAN_VALID in the flag words and recompute CaAutoReset.reset_plan / reset_obs -- the library cannot see that a
 * parameter differs from the one a stored plan was made with. */
int cagpu_plan(const CaParams *p, const CaState *s, void *stream);

/* Replaces: rvo2.PyRVOSimulator.doStep() + getAgentVelocity for every agent (call sites
 * RVOPolicy.py:25-28,70-74,86-93): one ORCA velocity per agent from C-float inputs.
 * pos/vel/pref: device float [E,N,2]; radius/max_speed: device float [E,N]; new_vel: device float [E,N,2]. */
int cagpu_orca(int32_t num_envs, int32_t num_agents, const float *pos, const float *vel, const float *pref,
               const float *radius, const float *max_speed, float collab_coeff, float time_horizon, float time_step,
               int32_t max_neighbors, float neighbor_dist, float *new_vel, void *stream);

/* Replaces: OtherAgentsStatesSensor.sense + the observation assembly (OtherAgentsStatesSensor.py:58-144,
 * agent.py:323-327) for the CURRENT state, without stepping: rewrites o->obs only. */
int cagpu_observe(const CaParams *p, const CaState *s, const CaOut *o, void *stream);

/* Bytes of CaOut.workspace the step / reset / observe / rollout calls want for these parameters: 0 up to 64 agents per env,
 * otherwise one share (60 B x threads x num_agents; threads = 256 / 512 / 1024 for up to 256 / 512 / 1024 agents) per
 * workgroup of the large-env kernel, for min(num_envs, 2 x CUs) workgroups (1 x CUs above 256 agents); a smaller workspace
 * works too: fewer workgroups walk the envs.  Host-only call. */
uint64_t cagpu_workspace_bytes(const CaParams *p);

/* Device-side fault word of the CURRENT device (synchronises it): bit 0 = a bounded hand-over poll inside the pipelined
 * step kernel ran out (csrc/cagpu_pipe.inc wait_for), i.e. some launch since the last clear may have produced wrong state.
 * bit 1 = an operand of the GA3C-CADRL network kernel left the range of its two-plane fp16 split (|x| >= 65504: a normalised
 * input or an activation; csrc/cagpu_ga3c.inc), or an input column the network reads -- the four host columns and the
 * 19 x 7 other-agent block, after the normalisation -- was not finite (+-inf or NaN: ReLU would swallow the NaN and the
 * network would answer from zeros), i.e. some cagpu_ga3c / cagpu_ga3c_value / cagpu_ga3c_query call since the last clear
 * chose its actions from saturated or missing values.  Healthy up to the bound: a normalised input of +-65 503.99 leaves
 * the word clear and the logits within the tests' bar of a float64 evaluation (tests/test_gpu_ga3c_edges.py).
 * bit 2 = a map-set env's map index (CaMapSet.env_map) lay outside [0, num_maps) (cagpu_step_maps / cagpu_laserscan_maps /
 * cagpu_occupancy_grid_maps, v12): that env saw an empty map in some call since the last clear.
 * bit 3 = an env of a case stream (CaCaseStream) auto-reset more than `window` times between two refills: it loaded a window
 * slot that still held an older episode, i.e. it REPEATED a scenario (valid memory, a valid case -- but not the stream's);
 * raised by cagpu_stream_refill's kernel.  A larger window, or shorter launches, avoid it.
 * bit 4 = an agent was queried under a CaRvoDraw at an episode step s >= 2^22, outside the draw's address rule (its draw
 * repeated the one of step s - 2^22); a sampling agent of a CaGa3cSample at such a step raises it as well.
 * bit 5 = a logits row with a NaN reached cagpu_ga3c_sample / cagpu_ga3c_sample_at: its agent played index 0 (or kept the
 * index it held) and its logp / entropy are NaN.
 * *faults receives the word; clear != 0 resets it.  0 in normal operation; check it wherever the host synchronises anyway. */
int cagpu_device_faults(uint32_t *faults, int32_t clear);

/* The same word WITHOUT a synchronisation (v11): queues a 4-byte copy into *host_dst -- PINNED host memory of the caller --
 * on `stream`, behind the work already submitted there; the caller reads *host_dst once an event recorded behind this call
 * has completed.  Does not clear.  For the product path of a caller that never synchronises (the look-ahead ring of
 * core.BatchedSim: one probe per refill). */
int cagpu_device_faults_async(uint32_t *host_dst, void *stream);

/* Parity hook (tests only, synchronous, HOST pointers, default stream): evaluates on the device, element by element, the
 * operations through which a step's results can differ from a CPU run of the same algorithm -- no reference analogue:
 *   op 0: out0 = atan2(a, b)            (ROCm's libm; RVOPolicy.py:100, Dynamics.py:36, test_cases.py:554)
 *   op 1: out0, out1 = sin a, cos a     (the step kernels' short-range kernel for a heading in [-pi, pi]; UnicycleDynamics.py:30-35)
 *   op 2 / 3: out0 = the lean float divide a / b / square root of a used inside the ORCA phases, out1 = the correctly rounded one
 *   op 4 / 5: the same for the float64 divide / square root (distances, preferred velocity, ego frame)
 *   op 6: out0, out1 = heading_ego_frame, dist_to_goal of an agent at the origin with heading 0 and goal (a, b)
 * tests/test_gpu_bench_geometry.py runs the CPU oracle on ops 0 / 1 to show that they are the ONLY difference (free-running
 * episodes then agree bit for bit); tests/test_gpu_parity.py pins the operand range in which ops 2 - 5 agree. */
int cagpu_debug_libm(int32_t op, int32_t n, const double *a, const double *b, double *out0, double *out1);

/* Measurement hook (profiles/ only, no reference analogue): dst[i] = src[i] for n float64 elements with the access shape of
 * the step kernels' state loads -- ONE 8-byte element per lane and instruction (global_load_dwordx2 / global_store_dwordx2,
 * 64 consecutive elements per wavefront), device pointers, asynchronous on `stream`.  Its traffic is known exactly (8 n
 * bytes read, 8 n written), which is what the rocprofv3 FETCH_SIZE / WRITE_SIZE counters of the step kernels are calibrated
 * against (profiles/r05_traffic.json: the counters under-report this pattern on gfx950). */
int cagpu_debug_copy8(int64_t n, const double *src, double *dst, void *stream);

/* Episode metrics (CaEpMetrics, additive to v12): process slots 0 .. n_steps - 1 of `traj` -- n_steps CONSECUTIVE steps of
 * the run, following the slots of the previous call on the same carry --; traj->rows and traj->episode are both needed.
 * Only num_envs, num_agents (1 .. 1024) and dt of `p` are read.  CA_EINVAL: a NULL pointer, traj->rows / vals / cnts / carry
 * not 16-byte aligned, traj->episode / head not 4-byte aligned, capacity < 1, n_steps < 0.  n_steps == 0 does nothing.
 * Asynchronous on `stream`; cagpu_last_kernel() names the kernel (metrics_kernel<64>: one wavefront per env up to 64
 * agents; metrics_kernel<1024>: one workgroup per env). */
uint64_t cagpu_episode_metrics_carry_bytes(const CaParams *p);   /* 0 for bad sizes; host-only call */
int cagpu_episode_metrics(const CaParams *p, const CaTraj *traj, int32_t n_steps, const CaEpMetrics *m, void *stream);

/* MAP SENSORS FOR EVERY STEP OF A FUSED LAUNCH (additive to v12).  cagpu_laserscan and
 * cagpu_occupancy_grid read the CURRENT state, which after an n-step launch is the final one.  The three calls below give
 * the sensors of every step of such a launch from what it recorded, with kernels of their own -- no step kernel knows
 * about them (tests/pose_tape_ref.py is the NumPy statement of the two rules).
 *
 * POSE RING: structure-of-arrays, slot t = the poses after step t of the launch; slot t of every array, taken at its
 * pointer offset, is a CaState view that cagpu_laserscan / cagpu_occupancy_grid accept, and the whole ring is one batch of
 * n_steps x num_envs envs (env_map: its map-set indices). */
typedef struct CaPoseRing {
  double  *pos_x, *pos_y, *heading, *radius; /* device [n_steps, E, N], 16-byte aligned */
  int32_t *step_num;                         /* device [n_steps, E, N], 16-byte aligned */
  int32_t *env_map;                          /* device [n_steps, E]; NULL without a map set */
} CaPoseRing;                                /* 48 bytes */

/* The pose ring of one launch of n_steps steps, restated from
 *   start          the state as the launch FOUND it (pos_x, pos_y, heading, radius, step_num [E,N] and reset_count [E] are
 *                  read: the caller copies them on the stream ahead of the launch), start_env_map [E] with a set;
 *   traj           the launch's tape chunk (rows [n_steps, E, N, 12]; episode is not read);
 *   game_over      the launch's game_over ring, uint8 [n_steps, E] (CaOut.game_over of a ring launch);
 *   ar, set        the CaAutoReset and CaMapSet the launch ran with (either may be NULL; of the set only num_maps and
 *                  map_seed are read).
 * THE POSE RULE, per agent slot with t ascending:
 *   1. a row whose column 11 is >= 0 replaces position (columns 1, 2) and heading (column 10); step_num = column 11 + 1;
 *   2. any other row keeps the carried pose (nothing else of such a row is read);
 *   3. where game_over[t, e] is set and ar is given, the pose becomes the START pose of the env's next episode -- the
 *      table row of the auto-reset's case, the heading towards the goal or CaAutoReset.heading_seed's draw, zeros for an
 *      absent slot of a ragged table (CaParams.ragged) -- and step_num 0;
 *   4. with set->map_seed != 0 the slot's env_map entry is the map drawn at that auto-reset (CaMapSet.map_seed).
 * Steps 3 and 4 call the device functions the step kernels call.  A case stream's window (CaCaseStream) changes under
 * the launch that follows a refill: the caller must not use this call with one.  CA_EINVAL, nothing launched: a NULL
 * argument (ar / set / start_env_map without a set excepted), bad sizes, n_steps < 0, a NULL state pointer, traj->rows or
 * a ring array NULL or not 16-byte aligned, ring->env_map NULL with a set, a CaAutoReset without a table.  n_steps == 0
 * does nothing.  cagpu_last_kernel() is left alone by all three calls. */
int cagpu_tape_poses(const CaParams *p, const CaState *start, const int32_t *start_env_map, const CaTraj *traj,
                     const uint8_t *game_over, int32_t n_steps, const CaAutoReset *ar, const CaMapSet *set,
                     const CaPoseRing *ring, void *stream);

/* The laser scan's march over every slot of a pose ring: cagpu_laserscan's staging, rasterisation and march (the same
 * device code, csrc/cagpu_scan.inc) with one workgroup per (slot, env), against `map` or the slot's own map of `set`
 * (exactly one of the two; ring->env_map is used, set->env_map is not read).  Writes only the NEW range-index row of
 * every agent, idx uint8 [n_steps, E, N, num_beams] (255 = nothing hit): no history is read or written and scan->hist /
 * scan->out may be NULL.  CA_EINVAL / CA_EUNSUPPORTED as cagpu_laserscan (num_agents <= 256), and CA_EINVAL for map and
 * set at once, idx NULL or not 16-byte aligned, a bad ring; n_steps x num_envs above 2^31 - 1 is CA_EUNSUPPORTED. */
int cagpu_laserscan_slots(const CaParams *p, const CaPoseRing *ring, int32_t n_steps, const CaMap *map, const CaMapSet *set,
                          const CaScan *scan, uint8_t *idx, void *stream);

/* The LaserScanSensor history of slots first .. first + count - 1 of a launch of n_steps slots.  THE HISTORY RULE
 * (LaserScanSensor.py:84-88): row j of slot t is the index row of slot max(t - j, s), s the latest slot <= t whose
 * step_num (of the pose ring) is 0 -- the first measurement of an episode fills every row --, and a slot before the
 * launch is the history the launch found: slot -1 - r = row r of scan->hist (read only, unless written in place).
 * Outputs, either may be NULL (not both), 16-byte aligned: hist_out uint8 and out float32 metres, both
 * [count, E, N, num_to_store, num_beams].  In place: with count == 1, hist_out == scan->hist (and out == scan->out)
 * leaves exactly the state n_steps single cagpu_laserscan calls leave when slot n_steps - 1 is expanded.  CA_EINVAL,
 * nothing launched: NULL p / scan / idx / step_num / scan->hist, misaligned pointers, a bad CaScan, a slot range outside
 * the launch, hist_out == scan->hist with count != 1.  count == 0 does nothing. */
int cagpu_laserscan_history(const CaParams *p, const CaScan *scan, const uint8_t *idx, const int32_t *step_num, int32_t n_steps,
                            int32_t first, int32_t count, uint8_t *hist_out, float *out, void *stream);

/* ================================ GRADIENTS OF THE GA3C-CADRL NETWORK ================================
 * The reference ships no training code for this network; the rule is this project's, and its judge is a float64 autograd
 * evaluation of the graph tests/ga3c_f64_ref.py states (tests/ga3c_grad_ref.py is the backward pass written out).
 *
 * cagpu_ga3c_grad gives dL/d(weights) of the graph cagpu_ga3c_query evaluates, for upstream gradients on its two outputs:
 * float32 normalisation of x, sequence length int(x[:,0]) clamped to 0..19, an LSTM-64 with gate order i, j, f, o and the
 * forget gate's + 1 whose h and c are frozen behind a row's length, three ReLU layers (a ReLU passes gradient where its
 * pre-activation is > 0), logits_p and logits_v.  Slots at and behind a row's length enter nothing: they are never read.
 *
 * grad: float32 [cagpu_ga3c_grad_floats() = 170 764], the concatenation in the checkpoint's key order and [in, out]
 * row-major layout of lstm_kernel [71,256], lstm_bias [256], layer1_kernel [68,256], layer1_bias [256], layer2_kernel
 * [256,256], layer2_bias [256], fc1_kernel [256,256], fc1_bias [256], logits_p_kernel [256,11], logits_p_bias [11],
 * logits_v_kernel [256,1], logits_v_bias [1] (the last two are written as zeros when dvalue == NULL).  input_mean,
 * input_std and x get no gradient.  The gradient is the plain SUM over the live rows of the row's vector-Jacobian product:
 * a mean or a weighting is the caller's, through dlogits / dvalue.  accumulate == 0: grad is overwritten; accumulate == 1:
 * the call's sum is added to what grad holds (a long batch in chunks under a workspace budget).
 *
 * Arithmetic: float32, every product an exact fused multiply-add on the vector ALU (no reduced-precision operand planes);
 * the backward pass recomputes the activations it needs, the forward kernel is not involved.  DETERMINISTIC: the same inputs
 * give the same bytes of grad whatever `work` held -- no atomics, the rows are summed in S = min(32, ceil(rows / 64))
 * contiguous slices, each in row order, and the slices in slice order.  work: device memory, 4-byte aligned, of at least
 * cagpu_ga3c_grad_work_bytes(rows) bytes (DESIGN.md says what it holds: about 36 KB per row + 0.7 MB per slice); it needs
 * NO initialisation.  Non-finite inputs in live rows: unspecified.
 *
 * rows == 0: CA_OK, nothing launched, grad zeroed unless accumulate; x and work are not looked at (they may be NULL:
 * cagpu_ga3c_grad_work_bytes(0) is 0), every other argument is checked as usual.  rows >= 2^31: CA_EUNSUPPORTED.  CA_EINVAL,
 * grad untouched: NULL net / g / x / grad / work or weight pointer, rows < 0, width < 1, work_bytes too small, dlogits and
 * dvalue both NULL, dvalue without value_kernel / value_bias.  net->packed, rows_scratch and agent_net are not used.
 * cagpu_last_kernel() names the launch "ga3c_grad_kernel ...". */
typedef struct CaNetGrad {
  const float *x; int64_t rows; int32_t width, accumulate;   /* x, rows, width exactly as CaNetQuery (crop_x rule) */
  const uint8_t *live;        /* [rows] or NULL: rows with live == 0 are NEVER READ (NaN there changes nothing) */
  const float *dlogits;       /* [rows, 11] dL/d(logits_p/BiasAdd), or NULL (= 0) */
  const float *dvalue;        /* [rows]     dL/d(Squeeze:0), or NULL (= 0); needs value_kernel / value_bias */
  const float *value_kernel, *value_bias;
  float *grad;                /* [cagpu_ga3c_grad_floats()] float32, see above */
  void *work; uint64_t work_bytes;   /* >= cagpu_ga3c_grad_work_bytes(rows); needs NO initialisation */
} CaNetGrad;                  /* 88 bytes */
uint64_t cagpu_ga3c_grad_floats(void);                 /* host-only */
uint64_t cagpu_ga3c_grad_work_bytes(int64_t rows);     /* host-only; 0 for bad arguments (and for rows == 0) */
int cagpu_ga3c_grad(const CaNet *net, const CaNetGrad *g, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CAGPU_H_ */
