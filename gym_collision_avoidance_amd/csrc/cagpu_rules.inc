// gym_collision_avoidance_amd/csrc/cagpu_rules.inc -- included by cagpu.hip (inside its anonymous namespace, after reset_lane).
//
// The rules of one step of the reference that MORE THAN ONE step kernel applies (ca_kernel, pipe::ca_pipe_kernel,
// big::ca_big_kernel), each stated once.  Values go in, references come out; nothing here knows which kernel calls.
// A kernel whose compiled code a call would change keeps its own text of that rule, under a comment that names the rule
// here (profiles/shared_rules.md has the list and the figures).
// An input that a rule reads only on some of its paths, or late, comes in as a const reference: the caller's read of it
// then happens where the rule reads it and not at the call.

// ORCA velocity -> (speed, heading change) of the float32 action: Agent::update (float position += v * timeStep), then
// RVOPolicy.py:96-111.  (The caller adds rvo_heading_noise, :118-119.)
__device__ __forceinline__ void rvo_action(const float fpx, const float fpy, const F2 v, const float ts, const double px,
                                           const double py, const double heading, const double& inv_rvo_dt, double& spd,
                                           double& dh) {
  const float npx = fpx + v.x * ts, npy = fpy + v.y * ts;
  const double dpx = static_cast<double>(npx) - px, dpy = static_cast<double>(npy) - py;
  const double ang = atan2(dpy, dpx);
  const double nh = (ang < 0.0) ? ang + kTwoPi : ((ang == 0.0) ? 0.0 : ang);  // `% (2*pi)`, :102
  dh = wrap_pi(nh - heading);
  spd = inv_rvo_dt * sqrtd(dpx * dpx + dpy * dpy);  // :106: 1/self.dt * norm
  if (fabs(dh) > kPi / 6) {
    dh = ((dh > 0.0) - (dh < 0.0)) * (kPi / 6);
    spd = 0.0;
  }
}

// The policies whose output (e0, e1) the caller provides.  Any other policy leaves spd / dh alone.
// (pref_speed: read by two of the three policies only)
__device__ __forceinline__ void ext_policy_action(const uint32_t pol, const double e0, const double e1, const double& pref_speed,
                                                  const double max_heading_change, double& spd, double& dh) {
  if (pol == CA_POL_EXTERNAL) {  // ExternalPolicy.py:14-16
    spd = e0;
    dh = e1;
  } else if (pol == CA_POL_LEARNING) {  // LearningPolicy.py:29-33
    dh = max_heading_change * (2. * e1 - 1.);
    spd = pref_speed * e0;
  } else if (pol == CA_POL_LEARNING_GA3C || pol == CA_POL_GA3C_CADRL) {  // LearningPolicyGA3C.py:24-26,
    // GA3CCADRLPolicy.py:81-84 (index from cagpu_ga3c), network.py:7-16
    int q = static_cast<int>(e0);
    q = q < 0 ? 0 : (q > 10 ? 10 : q);
    const int hq = (q < 5) ? q - 2 : ((q - 5) % 3 - 1) * 2;  // heading index in units of pi/12
    const double s0 = (q < 5) ? 1.0 : ((q < 8) ? 0.5 : 0.0);
    spd = pref_speed * s0;
    dh = (hq == -2) ? -kPi / 6 : (hq == -1) ? -kPi / 12 : (hq == 0) ? 0.0 : (hq == 1) ? kPi / 12 : kPi / 6;
  }
}

// Agent.take_action (agent.py:192-241) with the float32 action (a0f, a1f); ext_state (or nullptr): the [.., 5] rows a
// host-side Dynamics subclass integrated, i this agent's row.  -> the agent got past the done gate.
// (The pipelined kernel keeps its own form: it defers the bookkeeping off its critical chain and has no ext_state.)
__device__ __forceinline__ bool move_lane(Lane& r, const float a0f, const float a1f, const CaParams& p, const double* ext_state,
                                          const long i) {
  if (r.flags & (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION)) {
    if (r.flags & CA_AT_GOAL) r.flags |= CA_WAS_AT_GOAL;
    if (r.flags & CA_IN_COLLISION) r.flags |= CA_WAS_IN_COLLISION;
    r.vx = r.vy = 0.0;
    return false;
  }
  r.act0 = a0f;
  r.act1 = a1f;
  const double a0 = a0f, a1 = a1f;
  const uint32_t dyn = (r.flags >> CA_DYNAMICS_SHIFT) & 0xF;
  if (dyn != CA_DYN_EXTERNAL) {
    double nh;
    if (dyn == CA_DYN_MAX_TURN_RATE) {  // UnicycleDynamicsMaxTurnRate.py:31-33
      double trn = a1 / p.dt;
      trn = fmin(fmax(trn, -3.0), 3.0);
      nh = wrap_pi(trn * p.dt + r.heading);
    } else {
      nh = wrap_pi(a1 + r.heading);  // UnicycleDynamics.py:28
    }
    double sn, cs;
    sincos_heading(nh, sn, cs);
    r.px += a0 * cs * p.dt;
    r.py += a0 * sn * p.dt;
    r.vx = a0 * cs;
    r.vy = a0 * sn;
    r.heading = nh;
    if (dyn == CA_DYN_UNICYCLE) r.td = turning_dir_next(r.td, nh);
  } else if (ext_state) {  // agent.py:214-220
    const double* q = ext_state + 5 * i;
    const double npx = q[0], npy = q[1], nvx = q[2], nvy = q[3], nh = q[4];
    if (!(npx != npx || npy != npy || nvx != nvx || nvy != nvy || nh != nh)) {
      r.px = npx; r.py = npy; r.vx = nvx; r.vy = nvy; r.heading = nh;
    }
  }
  const double qx = r.px - r.gx, qy = r.py - r.gy;
  if (qx * qx + qy * qy <= p.near_goal_threshold * p.near_goal_threshold) r.flags |= CA_AT_GOAL;
  else r.flags &= ~static_cast<uint32_t>(CA_AT_GOAL);
  r.tr -= p.dt;
  r.t += p.dt;
  r.step_num += 1;
  if (r.tr <= 0.0) r.flags |= CA_OUT_OF_TIME;
  return true;
}

// The agent's own columns of its observation row: is_learning, dist_to_goal, heading_ego, pref_speed, radius (row[1], the
// number of other agents, belongs to the sensor).  here: the slot holds an agent.
__device__ __forceinline__ void obs_own_columns(float* row, const bool here, const uint32_t flags, const double dist,
                                                const double heading_ego, const double pref_speed, const double radius) {
  row[0] = (here && (flags & CA_IS_LEARNING)) ? 1.f : 0.f;
  row[2] = here ? static_cast<float>(dist) : 0.f;
  row[3] = here ? static_cast<float>(heading_ego) : 0.f;
  row[4] = here ? static_cast<float>(pref_speed) : 0.f;
  row[5] = static_cast<float>(radius);
}

// done / game over of one env from its agents' flag words (collision_avoidance_env.py:514-553): AND / OR of the words, then
// bit tests -- no short-circuit chains (they compile to one dependent LDS round trip + branch per agent)
struct FlagFold {
  uint32_t f_and = ~0u, f_or = 0u, learn_and = ~0u;
  __device__ __forceinline__ void add(const uint32_t f) {
    f_and &= f;
    f_or |= f;
    learn_and &= (f & CA_STILL_LEARNING) ? f : ~0u;  // learners only
  }
  __device__ __forceinline__ bool over(const int mode, const uint32_t first_flag) const {  // first_flag: agent 0's word
    if (mode == CA_OVER_AGENT0) return (first_flag & CA_DONE) != 0;
    if (mode == CA_OVER_LEARNING_DONE) return (learn_and & CA_DONE) != 0;
    return (f_and & CA_DONE) != 0;
  }
  __device__ __forceinline__ bool any_coll() const { return (f_or & CA_IN_COLLISION) != 0; }
  __device__ __forceinline__ bool all_goal() const { return (f_and & CA_AT_GOAL) != 0; }
};

// One finished episode into its env's eight counters (experiments/src/env_utils.py:56-87 reduced to counters); tot_r, ttg,
// extra: the agents' episode reward, time to goal and extra time to goal, summed in agent order by the caller
__device__ __forceinline__ void env_stats_add(double* st, const bool any_coll, const bool all_goal, const int ep_step,
                                              const double tot_r, const double ttg, const double extra) {
  st[0] += 1.0;
  if (any_coll) st[1] += 1.0;
  else if (all_goal) st[2] += 1.0;
  else st[3] += 1.0;
  st[4] += ep_step;
  st[5] += tot_r;
  st[6] += ttg;
  st[7] += extra;
}

// The case of the table that env `env` of this launch takes at its reset_cnt-th auto-reset
__device__ __forceinline__ long reset_case(const KArgs& k, const long env, const int reset_cnt) {
  return (k.env_id_offset + env + static_cast<long>(reset_cnt) * k.case_stride) % k.n_cases;
}

// ... and the heading its agent a starts that episode with in training mode (test_cases.py:558-559): uniform in [-pi, pi);
// 0 without a heading seed (reset_lane then takes the direction to the goal)
__device__ __forceinline__ double reset_heading(const KArgs& k, const long env, const int reset_cnt, const int a) {
  if (!k.heading_seed) return 0.0;
  const unsigned long long ge = static_cast<unsigned long long>(k.env_id_offset + env);
  return -kPi + kTwoPi * gen::uniform_at(k.heading_seed, static_cast<unsigned>(ge), static_cast<unsigned>(ge >> 32),
                                         static_cast<unsigned>(reset_cnt), static_cast<unsigned>(a));
}

// ---- RVOPolicy's stochastic branches drawn in the step kernels (CaRvoDraw in cagpu.h has the rule; ca_kernel,
// big::ca_big_kernel and rvo_draw_at_kernel call these).  A draw's address: (global env id, episode, agent slot, episode step).
struct RvoAddr {
  unsigned g0, g1, k;
};
__device__ __forceinline__ RvoAddr rvo_addr(const KArgs& k, const long env, const int reset_cnt) {
  const unsigned long long g = static_cast<unsigned long long>(k.rd_addr ? k.rd_addr[2 * env] : k.env_id_offset + env);
  const unsigned ep = k.rd_addr ? static_cast<unsigned>(k.rd_addr[2 * env + 1]) : static_cast<unsigned>(reset_cnt);
  return {static_cast<unsigned>(g), static_cast<unsigned>(g >> 32), ep};
}
// counter word 3; an episode step outside the rule raises bit 4 of the fault word
__device__ __forceinline__ unsigned rvo_word3(const int a, const int s) {
  if (static_cast<unsigned>(s) >> 22) atomicOr(&g_fault, 16u);
  return (static_cast<unsigned>(s) << 10) | static_cast<unsigned>(a);
}
// the clock lies within DT of a multiple of T: RVOPolicy.py:78-79 with numpy's round(x, 3) = rint(x * 1000) / 1000
__device__ __forceinline__ bool rvo_redraw_window(const double t, const double T, const double dt) {
  const double m = fmod(t, T);
  return rint(m * 1000.0) / 1000.0 < dt || rint((T - m) * 1000.0) / 1000.0 < dt;
}
// what a redraw of use_non_coop_policy gives: np.random.choice([True, False], p=[1 - |c|, |c|]), RVOPolicy.py:80
__device__ __forceinline__ bool rvo_noncoop_draw(const unsigned long long seed, const RvoAddr ad, const unsigned w3, const double c) {
  double u0, u1;
  gen::uniform2_at(seed, ad.g0, ad.g1, ad.k, w3, u0, u1);
  return u0 < 1.0 - fabs(c);
}
// the number a masked agent adds to its delta heading: std * z, z standard normal (Box-Muller over u1 and the second block's v0)
__device__ __forceinline__ double rvo_noise_draw(const unsigned long long seed, const RvoAddr ad, const unsigned w3, const double std) {
  double u0, u1;
  gen::uniform2_at(seed, ad.g0, ad.g1, ad.k, w3, u0, u1);
  const double v0 = gen::uniform_at(seed, ad.g0, ad.g1, ad.k | 0x80000000u, w3);
  return std * (sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * v0));
}
// The ego's collaboration coefficient of this query (RVOPolicy.py:77-90): redraws CA_RVO_NONCOOP in `flags` inside the window
__device__ __forceinline__ float rvo_collab_draw(const KArgs& k, const RvoAddr ad, const int a, const int s, const double t,
                                                 uint32_t& flags) {
  if (!(k.rd_c < 0.0)) return static_cast<float>(k.p.rvo_collab_coeff);
  if (rvo_redraw_window(t, k.rd_T, k.p.rvo_dt)) {
    if (rvo_noncoop_draw(k.rd_seed, ad, rvo_word3(a, s), k.rd_c)) flags |= CA_RVO_NONCOOP;
    else flags &= ~static_cast<uint32_t>(CA_RVO_NONCOOP);
  }
  return (flags & CA_RVO_NONCOOP) ? 0.0f : static_cast<float>(k.rd_c);
}
// ... and what it adds to its delta heading (RVOPolicy.py:118-119): +0.0 for an unmasked agent
__device__ __forceinline__ double rvo_heading_noise(const KArgs& k, const RvoAddr ad, const int a, const int s, const long i) {
  return k.rd_mask[i] ? rvo_noise_draw(k.rd_seed, ad, rvo_word3(a, s), k.rd_std) : 0.0;
}
