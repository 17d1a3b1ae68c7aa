// gym_collision_avoidance_amd/csrc/cagpu_big.inc -- included by cagpu.hip (inside its anonymous namespace, after ca_kernel).
//
// Envs with MORE THAN 64 AGENTS (the reference's make_testcase_huge / get_testcase_huge, test_cases.py:914-1018, are
// unbounded; 100 agents in its shipped case).  ca_kernel keeps an env in ONE workgroup tile whose two LDS unions are
// quadratic in the agent count -- the ORCA lines of all agents ((N-1) N 25 B = 250 KB at N = 100) and the sensor tiles
// (N N 32 B) -- so it ends at 64.  This kernel trades speed for reach: one workgroup per env, ONE THREAD PER AGENT (workgroups
// of 256, 512 or 1024 threads: up to 1024 agents, the largest workgroup the device runs; round 5 -- make_testcase_huge takes any
// count), every per-(agent, other) quantity in a caller-provided global workspace (column layout [slot][NT]: a wave's lanes
// read consecutive addresses), serial loops where ca_kernel deals pairs over waves.  Same arithmetic, statement by
// statement, as ca_kernel's agent-wave phases and pair phases (every expression below cites the one it restates), so the
// parity bars are the same: tests/test_gpu_parity.py::test_big_envs_vs_oracle.  The incremental ORCA programme is the
// serial form the stand-alone cagpu_orca uses (orca_velocity: rvo2's own loops, IEEE divide / square root).
// Throughput is a few 10^6 agent-steps/s -- three orders of magnitude above the reference's Python at this size, three
// below the tiled kernels; the fast paths are untouched.
namespace big {

constexpr int NT_MAX = 1024;  // the largest agent count (= the largest workgroup)
__host__ __device__ inline int threads_for(int N) { return N <= 256 ? 256 : (N <= 512 ? 512 : 1024); }

// workspace bytes of ONE workgroup: dist^2 float, two line columns float4, sort key int, p_orth / time-to-impact double,
// first-pass rank int -- N slots each, NT lanes wide
__host__ __device__ inline size_t ws_bytes_per_wg(int N) { return static_cast<size_t>(threads_for(N)) * N * (4 + 16 + 16 + 4 + 8 + 8 + 4); }
// LDS of one workgroup: 8 double + 5 float + 1 u32 arrays of NT elements (88 KB at 1024 threads: dynamic)
__host__ __device__ inline size_t lds_bytes(int nt) { return static_cast<size_t>(nt) * (8 * 8 + 5 * 4 + 4); }

// RD: the RVO draw (CaRvoDraw) has instantiations of its own, as in ca_kernel
template <int NT, bool RD = false>
__global__ __launch_bounds__(NT) void ca_big_kernel(const KArgs k, unsigned char* ws, const size_t ws_per_wg) {
  extern __shared__ __attribute__((aligned(16))) unsigned char big_smem[];
  double* sh_px = reinterpret_cast<double*>(big_smem);
  double *sh_py = sh_px + NT, *sh_vx = sh_py + NT, *sh_vy = sh_vx + NT, *sh_rad = sh_vy + NT;
  double *sh_r0 = sh_rad + NT, *sh_r1 = sh_r0 + NT, *sh_r2 = sh_r1 + NT;
  float* sh_fpx = reinterpret_cast<float*>(sh_r2 + NT);
  float *sh_fpy = sh_fpx + NT, *sh_fvx = sh_fpy + NT, *sh_fvy = sh_fvx + NT, *sh_frad = sh_fvy + NT;
  uint32_t* sh_flag = reinterpret_cast<uint32_t*>(sh_frad + NT);
  const CaParams& p = k.p;
  const int N = p.num_agents, K = p.max_obs, W = 6 + 7 * K;
  const int a = threadIdx.x;
  const bool active = a < N;
  unsigned char* base = ws + static_cast<size_t>(blockIdx.x) * ws_per_wg;
  const size_t col = static_cast<size_t>(NT) * N;  // elements of one [N][NT] column block
  float* fcol = reinterpret_cast<float*>(base) + a;                 // [N][NT] ORCA dist^2            (bytes 0 ..)
  float4* Lcol = reinterpret_cast<float4*>(base + col * 4) + a;     // [N][NT] half-planes            (4 col ..)
  float4* Pcol = reinterpret_cast<float4*>(base + col * 20) + a;    // [N][NT] projected lines, lp3   (20 col ..)
  int* kcol = reinterpret_cast<int*>(base + col * 36) + a;          // [N][NT] sort key               (36 col ..)
  double* ocol = reinterpret_cast<double*>(base + col * 40) + a;    // [N][NT] p_orth                 (40 col ..)
  double* tcol = reinterpret_cast<double*>(base + col * 48) + a;    // [N][NT] time to impact         (48 col ..)
  int* rcol = reinterpret_cast<int*>(base + col * 56) + a;          // [N][NT] first-pass rank        (56 .. 60 col)

  for (long e = blockIdx.x; e < p.num_envs; e += gridDim.x) {
    const long i = e * N + (active ? a : 0);
    // ---- load my agent (ca_kernel: "load my agent")
    Lane r;
    r.px = r.py = r.vx = r.vy = r.heading = r.gx = r.gy = 0.0;
    r.rad = r.ps = 1.0; r.tr = r.t = r.slt = r.epr = 0.0; r.td = 0.0;
    r.act0 = r.act1 = 0.f; r.flags = CA_DONE | CA_AT_GOAL | CA_ABSENT; r.step_num = 0;
    int ep_step = 0, reset_cnt = 0;
    if (active) {
      if (k.s.turning_dir) r.td = k.s.turning_dir[i];
      r.px = k.s.pos_x[i]; r.py = k.s.pos_y[i]; r.vx = k.s.vel_x[i]; r.vy = k.s.vel_y[i];
      r.heading = k.s.heading[i]; r.gx = k.s.goal_x[i]; r.gy = k.s.goal_y[i];
      r.rad = k.s.radius[i]; r.ps = k.s.pref_speed[i]; r.tr = k.s.time_remaining[i]; r.t = k.s.t[i];
      r.slt = k.s.slt[i]; r.epr = k.s.ep_reward[i];
      r.act0 = k.s.last_action[2 * i]; r.act1 = k.s.last_action[2 * i + 1];
      r.flags = k.s.flags[i];
      r.step_num = k.s.step_num[i];
      ep_step = k.s.episode_step[e];
      reset_cnt = k.s.reset_count[e];
    }
    bool statics_dirty = false;
    bool do_sense = active;
    float reward = 0.f;
    const auto absent = [&]() { return p.ragged && (r.flags & CA_ABSENT) != 0; };

    if (k.mode == MODE_RESET) {
      do_sense = active && (!k.reset_mask || k.reset_mask[e]);
      if (do_sense) {
        reset_lane(r, k.reset_cases + i * 6, k.reset_headings != nullptr, k.reset_headings ? k.reset_headings[i] : 0.0, p);
        ep_step = 0;
        reset_cnt = 0;
        statics_dirty = true;
      }
    }

    // a map set: this env's grid for the wall tests of this step (one index per env: the workgroup holds the env)
    const uint32_t* wall_bits = k.map.static_bits;
    if (k.env_map && k.mode == MODE_STEP) wall_bits = set_grid(wall_bits, k.map_words, k.num_maps, k.env_map[e], a == 0);
    if (k.mode == MODE_STEP) {
      // ================= A1: float bodies (RVOPolicy.py:57-74); an absent slot sits at infinity
      const uint32_t pol = (r.flags >> CA_POLICY_SHIFT) & 0xF;
      const bool query = active && !(r.flags & CA_DONE);  // env.py:311
      const bool rvo = query && pol == CA_POL_RVO;
      ep_step += 1;  // env.py:183
      sh_fpx[a] = (!active || absent()) ? INFINITY : static_cast<float>(r.px);
      sh_fpy[a] = static_cast<float>(r.py);
      sh_fvx[a] = static_cast<float>(r.vx);
      sh_fvy[a] = static_cast<float>(r.vy);
      sh_frad[a] = static_cast<float>((1 + 5e-2) * r.rad);  // RVOPolicy.py:71
      __syncthreads();
      // ================= policy (env.py:305-323)
      double spd = 0.0, dh = 0.0;
      F2 v_orca = f2(0.f, 0.f);
      if (query) {
        if (pol == CA_POL_RVO) {
          const double gvx = r.gx - r.px, gvy = r.gy - r.py;
          const double sc = divd(r.ps, sqrtd(gvx * gvx + gvy * gvy));  // RVOPolicy.py:66-67
          const F2 pref = f2(static_cast<float>(sc * gvx), static_cast<float>(sc * gvy));
          float collab = k.s.rvo_collab ? k.s.rvo_collab[i] : static_cast<float>(p.rvo_collab_coeff);  // :86-90
          // RVO draw (CaRvoDraw; the RD instantiations): the coefficient and, below, the noise are drawn here
          if (RD) collab = rvo_collab_draw(k, rvo_addr(k, e, reset_cnt), a, r.step_num, r.t, r.flags);
          v_orca = orca_velocity<NT>(sh_fpx, sh_fpy, sh_fvx, sh_fvy, sh_frad, 0, a, N, pref, static_cast<float>(r.ps), collab,
                                     static_cast<float>(p.rvo_time_horizon), static_cast<float>(p.rvo_dt),
                                     static_cast<float>(p.sensing_horizon), p.rvo_max_neighbors, fcol, Lcol, Pcol);
          rvo_action(sh_fpx[a], sh_fpy[a], v_orca, static_cast<float>(p.rvo_dt), r.px, r.py, r.heading, k.inv_rvo_dt, spd, dh);
          if (k.s.rvo_heading_noise) dh = dh + k.s.rvo_heading_noise[i];  // :118-119 (drawn by the caller)
          if (RD && k.rd_mask) dh = dh + rvo_heading_noise(k, rvo_addr(k, e, reset_cnt), a, r.step_num, i);
        } else if (pol == CA_POL_NONCOOP) {  // NonCooperativePolicy.py:21
          const Ego eg = ego_frame(r.px, r.py, r.gx, r.gy, r.heading);
          spd = r.ps;
          dh = -eg.heading_ego;
        } else if (pol == CA_POL_STATIC) {  // StaticPolicy.py:21-23
          r.gx = r.px;
          r.gy = r.py;
          statics_dirty = true;
        } else if (k.ext) {
          ext_policy_action(pol, k.ext[2 * i], k.ext[2 * i + 1], r.ps, p.max_heading_change, spd, dh);
        }
      }
      const float a0f = static_cast<float>(spd), a1f = static_cast<float>(dh);  // float32 `all_actions`
      if (active && k.o.actions) reinterpret_cast<float2*>(k.o.actions)[i] = make_float2(a0f, a1f);
      if (active && k.o.orca_vel)
        reinterpret_cast<float2*>(k.o.orca_vel)[i] = rvo ? make_float2(v_orca.x, v_orca.y) : make_float2(0.f, 0.f);
      // ================= move (Agent.take_action, agent.py:192-241)
      const double t_pre = r.t;         // (the trajectory row holds the clock and the index BEFORE their increments)
      const int index_pre = r.step_num;
      const bool moved = active && move_lane(r, a0f, a1f, p, k.s.ext_state, i);
      if (k.traj_rows && active) {  // trajectory tape (CaTraj): after the move, before any auto-reset of this step
        double* row = k.traj_rows + i * 12;   // (one launch per step: the host advances the slot)
        if (moved) traj_store(row, t_pre, r.px, r.py, r.gx, r.gy, r.rad, r.ps, r.vx, r.vy, r.act0, r.heading, index_pre);
        else row[11] = -1.0;
        if (a == 0 && k.traj_ep) k.traj_ep[e] = reset_cnt;
      }
    }

    // ================= sensing passes: once, and a second time for an env that auto-reset in this step
    for (int pass = 0; pass < 2; ++pass) {
      __syncthreads();  // (everybody is done with the previous contents of the tile)
      sh_px[a] = r.px; sh_py[a] = r.py; sh_vx[a] = r.vx; sh_vy[a] = r.vy;
      sh_rad[a] = (active && !absent()) ? r.rad : 0.0;   // (radius 0 = no agent in this slot, as in ca_kernel's pair phases)
      __syncthreads();
      const bool here = active && !absent();
      const double hx = r.px, hy = r.py, hr = r.rad;
      Ego eg;
      eg.dist = 0.0; eg.prx = eg.pry = eg.orx = eg.ory = eg.heading_ego = 0.0;
      if (here) eg = ego_frame(r.px, r.py, r.gx, r.gy, r.heading);
      // ---- pair pass (ca_kernel P3): collision gap, sort key, p_orth, time to impact of every other agent
      double nearest = INFINITY;
      int cnt = 0;
      if (active) {
        for (int j = 0; j < N; ++j) {
          int key = KEY_NONE;
          double po = 0.0, tti = 0.0;
          if (j != a) {
            const double ox = sh_px[j], oy = sh_py[j], orad = sh_rad[j];
            const double rx = ox - hx, ry = oy - hy;
            const double d = sqrtd(rx * rx + ry * ry);
            const bool both = here && (!p.ragged || orad > 0.0) && (p.ragged ? hr > 0.0 : true);
            if (both) {
              const double gap = d - (hr + orad);   // env.py:458-512
              nearest = (gap < nearest) ? gap : nearest;
            }
            if (both && !(d > p.sensing_horizon)) {
              const double d2o = d - hr - orad;
              key = static_cast<int>(fmin(fmax(rint(d2o * 100.0), -2.0e9), 2.0e9));  // numpy scalar round(x, 2) bucket
              po = rx * (-eg.pry) + ry * eg.prx;
              if (p.sort_mode == CA_SORT_TIME_TO_IMPACT)  // sensor :96-104
                tti = time_to_impact(hx, hy, ox, oy, sh_vx[a], sh_vy[a], sh_vx[j], sh_vy[j], hr + orad);
            }
          }
          kcol[j * NT] = key;
          ocol[j * NT] = po;
          tcol[j * NT] = tti;
          cnt += static_cast<int>(key != KEY_NONE);
        }
      }
      // ---- A3 (first pass of a step only): rewards + collision flag (env.py:394-456)
      if (active && k.mode == MODE_STEP && pass == 0) {
        const bool coll = nearest <= 0.0;
        double rw = p.reward_time_step;
        if (r.flags & CA_AT_GOAL) {
          if (!(r.flags & CA_WAS_AT_GOAL)) rw = p.reward_at_goal;
        } else if (!(r.flags & CA_WAS_IN_COLLISION)) {
          if (coll) {
            rw = p.reward_collision;
            r.flags |= CA_IN_COLLISION;
          } else if (hits_wall_in(k.map, wall_bits, r.px, r.py, r.rad)) {  // env.py:425-429, :494-506
            rw = p.reward_collision_wall;
            r.flags |= CA_IN_COLLISION;
          } else {
            if (nearest <= p.getting_close_range) rw = -0.1 - nearest / 2.0;
            if (fabs(static_cast<double>(r.act1)) > p.wiggly_threshold) rw += p.reward_wiggly;
          }
        }
        rw = fmin(fmax(rw, p.reward_min), p.reward_max);
        if (absent()) rw = 0.0;  // no agent in this slot: the zero padding of wrappers.py:143-173
        r.epr += rw;
        reward = static_cast<float>(rw);
        const bool d = (r.flags & (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION)) != 0;
        if (d) r.flags |= CA_DONE; else r.flags &= ~static_cast<uint32_t>(CA_DONE);
      }
      // ---- rank the candidates and emit the rows (ca_kernel P4; OtherAgentsStatesSensor.py:20-55, 109-143)
      if (do_sense) {
        float* row = k.o.obs + i * W;
        const int keep = cnt < p.obs_clip ? cnt : p.obs_clip;  // sensor :39
        obs_own_columns(row, here, r.flags, eg.dist, eg.heading_ego, r.ps, sh_rad[a]);
        row[1] = static_cast<float>(keep);
        for (int sl = keep; sl < K; ++sl) {  // zero the unfilled rows (sensor :112)
          float* z = row + 6 + 7 * sl;
          z[0] = z[1] = z[2] = z[3] = z[4] = z[5] = z[6] = 0.f;
        }
        const auto emit = [&](const int j, const int slot) {
          const double ox = sh_px[j], oy = sh_py[j], orad = sh_rad[j];
          const double rx = ox - hx, ry = oy - hy;
          float* o7 = row + 6 + 7 * slot;
          o7[0] = static_cast<float>(rx * eg.prx + ry * eg.pry);
          o7[1] = static_cast<float>(rx * (-eg.pry) + ry * eg.prx);
          o7[2] = static_cast<float>(sh_vx[j] * eg.prx + sh_vy[j] * eg.pry);
          o7[3] = static_cast<float>(sh_vx[j] * (-eg.pry) + sh_vy[j] * eg.prx);
          o7[4] = static_cast<float>(orad);
          o7[5] = static_cast<float>(hr + orad);
          o7[6] = static_cast<float>(sqrtd(rx * rx + ry * ry) - hr - orad);
        };
        for (int j = 0; j < N; ++j) {
          const int kj = kcol[j * NT];
          int rank = N;
          if (kj != KEY_NONE) {
            const double oj = ocol[j * NT], tj = tcol[j * NT];
            rank = 0;
            for (int q = 0; q < N; ++q) {
              const int kq = kcol[q * NT];
              if (kq == KEY_NONE) continue;
              const double oq = ocol[q * NT];
              const int lo = static_cast<int>(oq < oj) | (static_cast<int>(oq == oj) & static_cast<int>(q < j));
              if (p.sort_mode == CA_SORT_TIME_TO_IMPACT) {  // key (-tti, -dist, p_orth), sensor :36-38
                const double tq = tcol[q * NT];
                const int lk = static_cast<int>(kq > kj) | (static_cast<int>(kq == kj) & lo);
                rank += static_cast<int>(tq > tj) | (static_cast<int>(tq == tj) & lk);
              } else {
                rank += static_cast<int>(kq < kj) | (static_cast<int>(kq == kj) & lo);
              }
            }
            if (rank >= keep) rank = N;   // clipped away
          }
          if (p.sort_mode == CA_SORT_CLOSEST_LAST) rcol[j * NT] = rank;
          else if (rank < N) emit(j, rank);
        }
        if (p.sort_mode == CA_SORT_CLOSEST_LAST) {  // re-sort the kept ones by (-key, p_orth), stable (sensor :41-43)
          for (int j = 0; j < N; ++j) {
            const int rank = rcol[j * NT];
            if (rank >= N) continue;
            const int kj = kcol[j * NT];
            const double oj = ocol[j * NT];
            int r2 = 0;
            for (int q = 0; q < N; ++q) {
              const int rq = rcol[q * NT];
              if (rq >= N) continue;
              const int kq = kcol[q * NT];
              const double oq = ocol[q * NT];
              const int lo = static_cast<int>(oq < oj) | (static_cast<int>(oq == oj) & static_cast<int>(rq < rank));
              r2 += static_cast<int>(kq > kj) | (static_cast<int>(kq == kj) & lo);
            }
            emit(j, r2);
          }
        }
      }
      if (k.mode != MODE_STEP || pass == 1) break;
      // ================= A4: done / game over (env.py:514-553), auto-reset (vec_env.py:120-128), episode statistics
      do_sense = false;
      sh_flag[a] = active ? r.flags : (CA_DONE | CA_AT_GOAL | CA_ABSENT);
      sh_r0[a] = r.epr; sh_r1[a] = r.t; sh_r2[a] = r.t - r.slt;
      __syncthreads();
      FlagFold fold;
      for (int j = 0; j < N; ++j) fold.add(sh_flag[j]);
      const bool any_coll = fold.any_coll(), all_goal = fold.all_goal();
      const bool over = fold.over(p.game_over_mode, sh_flag[0]);
      if (active) {
        k.o.rewards[i] = reward;
        k.o.done[i] = static_cast<uint8_t>((r.flags & CA_DONE) != 0);
        if (a == 0) k.o.game_over[e] = static_cast<uint8_t>(over);
      }
      if (!(over && k.table)) break;   // (workgroup-uniform: every thread read the same flags)
      if (a == 0) {  // experiments/src/env_utils.py:56-87 reduced to counters, summed in agent order
        double tot_r = 0.0, ttg = 0.0, extra = 0.0;
        for (int j = 0; j < N; ++j) {
          tot_r += sh_r0[j];
          ttg += sh_r1[j];
          extra += sh_r2[j];
        }
        env_stats_add(k.s.env_stats + 8 * e, any_coll, all_goal, ep_step, tot_r, ttg, extra);
      }
      reset_cnt += 1;
      // a map set with a key: the env's next map (CaMapSet.map_seed), one plain store by agent 0's thread
      if (k.map_seed && a == 0) k.env_map[e] = map_draw(k.map_seed, k.env_id_offset + e, reset_cnt, k.num_maps);
      const long c = reset_case(k, e, reset_cnt);
      // policy draw (CaPolicyDraw; workgroup-uniform like the branch it sits on): every thread draws its own slot's pool
      // index once and the env settles the ensure rule through sh_flag (free again: every thread has read the flag words)
      int drawn = -1;
      if (k.draw_cdf) {
        if (active && (!p.ragged || k.table[(c * N + a) * 6 + 5] > 0.0))
          drawn = draw_index(k.draw_cdf, k.draw_n, draw_uniform(k.draw_seed, k.env_id_offset + e, reset_cnt, static_cast<unsigned>(a)));
        __syncthreads();
        sh_flag[a] = static_cast<uint32_t>(drawn);
        __syncthreads();
        if (drawn >= 0 && k.draw_ensure >= 0 && drawn != k.draw_ensure) {
          int n = 0, before = 0;
          bool any = false;
          for (int j = 0; j < N; ++j) {
            const int dj = static_cast<int>(sh_flag[j]);
            n += static_cast<int>(dj >= 0);
            before += static_cast<int>(dj >= 0 && j < a);
            any |= dj == k.draw_ensure;
          }
          if (!any && before == draw_ensure_rank(k.draw_seed, k.env_id_offset + e, reset_cnt, n)) drawn = k.draw_ensure;
        }
      }
      if (active) {
        const double h0 = reset_heading(k, e, reset_cnt, a);
        if (k.fin_obs) {  // final record (CaFinal): this thread's own terminal row and flag word, before the second pass
          const float* src = k.o.obs + i * W;   // (one launch per step: the host advances the block with the outputs)
          float* dst = k.fin_obs + i * W;
          for (int q = 0; q < W; ++q) dst[q] = src[q];
          if (k.fin_flags) k.fin_flags[i] = r.flags;
        }
        // episode log (CaEpLog): this thread's three addends and flag word, and -- agent 0 -- the episode's head
        if (k.log_rows)
          eplog_store(k.log_rows, k.log_head, k.log_cap, e, static_cast<int>(c), k.log_case_step, k.n_cases, N, a,
                      reset_cnt - 1, sh_r0[a], sh_r1[a], sh_r2[a], r.flags, ep_step, any_coll, all_goal);
        reset_lane(r, k.table + (c * N + a) * 6, k.heading_seed != 0, h0, p);
        if (drawn >= 0) r.flags = (r.flags & ~0xFC0u) | (k.draw_bits[drawn] & 0xFC0u);
        if (RD && k.rd_c < 0.0) r.flags &= ~static_cast<uint32_t>(CA_RVO_NONCOOP);  // RVO draw: a new episode starts without the bit
        statics_dirty = true;
        do_sense = true;
      }
      ep_step = 0;
    }

    // ---- store my agent
    if (active && k.mode != MODE_OBSERVE && (k.mode == MODE_STEP || !k.reset_mask || k.reset_mask[e])) {
      k.s.pos_x[i] = r.px; k.s.pos_y[i] = r.py; k.s.vel_x[i] = r.vx; k.s.vel_y[i] = r.vy;
      k.s.heading[i] = r.heading; k.s.time_remaining[i] = r.tr; k.s.t[i] = r.t;
      k.s.ep_reward[i] = r.epr;
      if (k.s.turning_dir) k.s.turning_dir[i] = r.td;
      if (statics_dirty) {
        k.s.goal_x[i] = r.gx; k.s.goal_y[i] = r.gy;
        k.s.radius[i] = r.rad; k.s.pref_speed[i] = r.ps; k.s.slt[i] = r.slt;
      }
      k.s.last_action[2 * i] = r.act0; k.s.last_action[2 * i + 1] = r.act1;
      k.s.flags[i] = r.flags & ~static_cast<uint32_t>(CA_PLAN_VALID);
      k.s.step_num[i] = r.step_num;
      if (a == 0) { k.s.episode_step[e] = ep_step; k.s.reset_count[e] = reset_cnt; }
    }
    __syncthreads();  // (the tile arrays are reused by the workgroup's next env)
  }
}

}  // namespace big
