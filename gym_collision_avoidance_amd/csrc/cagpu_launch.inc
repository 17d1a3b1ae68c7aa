// gym_collision_avoidance_amd/csrc/cagpu_launch.inc -- included by cagpu.hip (inside its anonymous namespace, after every
// kernel).  The host layer that chooses a geometry and launches: the error text (fail), the shared argument check
// (check_params), the one checked launch (launch), the one rule for the dynamic-LDS limit (raise_lds / launch_lds), and the
// launch plans of the step kernels (launch_any -> launch_pipe / launch_big / launch_main) and of the stand-alone ORCA.  The
// entry points that call it are csrc/cagpu_api.inc.
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* detail = "") {
  std::snprintf(g_err, sizeof(g_err), fmt, detail);
  return code;
}

int check_params(const CaParams* p, const CaState* s, const CaOut* o) {
  if (!p || !s || !o) return fail(CA_EINVAL, "cagpu: NULL params/state/out%s");
  if (p->num_envs < 1 || p->num_agents < 1) return fail(CA_EINVAL, "cagpu: num_envs and num_agents must be >= 1%s");
  if (p->num_agents > big::NT_MAX) return fail(CA_EUNSUPPORTED, "cagpu: num_agents > 1024 is not supported (one thread per agent in the large-env kernel, 1024 threads per workgroup)%s");
  if (p->num_agents > 64 && !o->workspace)
    return fail(CA_EINVAL, "cagpu: num_agents > 64 runs the large-env kernel, which needs CaOut.workspace (cagpu_workspace_bytes(p) bytes)%s");
  if (p->max_obs < 0) return fail(CA_EINVAL, "cagpu: max_obs < 0%s");
  if (p->obs_clip < 0 || p->obs_clip > p->max_obs) return fail(CA_EINVAL, "cagpu: obs_clip must be in [0, max_obs]%s");
  if (p->sort_mode < CA_SORT_CLOSEST_FIRST || p->sort_mode > CA_SORT_TIME_TO_IMPACT)
    return fail(CA_EINVAL, "cagpu: unknown sort_mode (OtherAgentsStatesSensor.py:52 raises ValueError)%s");
  if (p->game_over_mode < 0 || p->game_over_mode > 2) return fail(CA_EINVAL, "cagpu: bad game_over_mode%s");
  if (!(p->dt > 0.0) || !(p->rvo_dt > 0.0)) return fail(CA_EINVAL, "cagpu: dt and rvo_dt must be > 0%s");
  if (!o->obs || !o->rewards || !o->done || !o->game_over) return fail(CA_EINVAL, "cagpu: NULL output pointer%s");
  const void* ptrs[] = {s->pos_x, s->pos_y, s->vel_x, s->vel_y, s->heading, s->goal_x, s->goal_y, s->radius,
                        s->pref_speed, s->time_remaining, s->t, s->slt, s->ep_reward, s->last_action, s->flags,
                        s->step_num, s->episode_step, s->reset_count, s->env_stats};
  for (const void* q : ptrs)
    if (!q) return fail(CA_EINVAL, "cagpu: NULL state pointer%s");
  return CA_OK;
}

// ---- the one checked launch: every kernel of the host layer starts here, and a sequence of launches stops at the first
// that fails (cagpu_ga3c_pack and cagpu_debug_libm, which report in their own names, are the two exceptions)
template <typename... P, typename... A>
int launch(void (*kernel)(P...), const dim3 grid, const dim3 block, const size_t lds, hipStream_t st, const A&... args) {
  hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu: kernel launch failed: %s", hipGetErrorString(e));
  return CA_OK;
}

// ---- the one rule for the dynamic-LDS limit.  A launch that asks for more than the 48 KiB default needs the limit of its
// kernel raised on its device first (hipFuncSetAttribute).  Per (kernel, device) the most that was ever set is kept, and the
// runtime is asked again only by a launch that needs more than that: a kernel whose LDS varies per call (the sensors over
// their maps, ca_kernel over N, the stand-alone ORCA) is raised again when a later call outgrows an earlier one, and a
// launch within the mark -- or within the default -- makes no runtime call beyond hipGetDevice (none at all up to 48 KiB).
// A device id outside the table is aliased onto no other device: its launches ask the runtime each time.
// Threads: the marks are relaxed atomics (no lock, nothing allocated), and a mark is published only after the runtime took
// the value, so a launch never trusts a limit nobody set.  The runtime keeps the LAST value it was given, not the largest,
// so a thread whose mark moved under it (another thread raised the same pair meanwhile, and either call may have landed
// last) asks once more, for the larger of the two, until it publishes over the mark it last saw.
constexpr size_t LDS_DEFAULT = 48 * 1024;
constexpr int LDS_DEVICES = 64;
struct LdsLimit { std::atomic<size_t> set[LDS_DEVICES]; };  // (static storage: all 0 = nothing set yet)
template <auto KERNEL> LdsLimit lds_limit{};                // one table per kernel instantiation

int raise_lds(const void* kernel, LdsLimit& limit, const size_t lds) {
  if (lds <= LDS_DEFAULT) return CA_OK;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  std::atomic<size_t>* const mark = (dev >= 0 && dev < LDS_DEVICES) ? &limit.set[dev] : nullptr;
  size_t have = mark ? mark->load(std::memory_order_relaxed) : 0;
  if (lds <= have) return CA_OK;
  for (size_t want = lds;; want = have > want ? have : want) {  // (the mark only grows)
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(want));
    if (e != hipSuccess) return fail(CA_ELAUNCH, "cagpu: hipFuncSetAttribute: %s", hipGetErrorString(e));
    if (!mark || mark->compare_exchange_strong(have, want, std::memory_order_relaxed)) return CA_OK;
  }
}

// a kernel with its table, for the launches that may need the limit raised: kernel_of<&some_kernel<...>>()
template <typename... P>
struct Kernel {
  void (*fn)(P...);
  LdsLimit* limit;
};
template <typename... P> Kernel<P...> kernel_with(void (*fn)(P...), LdsLimit* limit) { return {fn, limit}; }
template <auto KERNEL> auto kernel_of() { return kernel_with(KERNEL, &lds_limit<KERNEL>); }

template <typename... P, typename... A>
int launch_lds(const Kernel<P...>& k, const dim3 grid, const dim3 block, const size_t lds, hipStream_t st, const A&... args) {
  if (const int rc = raise_lds(reinterpret_cast<const void*>(k.fn), *k.limit, lds)) return rc;
  return launch(k.fn, grid, block, lds, st, args...);
}

// ---- launch plan.  Everything that selects a kernel instantiation or a tile geometry is decided here from the
// arguments and the device's CU count alone (no environment variables).
thread_local char g_last_kernel[160] = "";

int device_cus() {  // CU count of the current device, cached per device id
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int c = cache[dev].load(std::memory_order_relaxed);
  if (c <= 0) {
    if (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || c <= 0) c = 256;
    cache[dev].store(c, std::memory_order_relaxed);
  }
  return c;
}

// n single-step launches in place of one n-step launch: the next launch writes the next slot of the caller's output ring
void ring_advance(KArgs& k) {
  k.o.obs += k.ring_obs;
  k.o.rewards += k.ring_agent;
  k.o.done += k.ring_agent;
  k.o.game_over += k.ring_env;
  if (k.o.actions) k.o.actions += 2 * k.ring_agent;
  if (k.o.orca_vel) k.o.orca_vel += 2 * k.ring_agent;
  if (k.traj_rows) k.traj_rows += static_cast<int64_t>(k.p.num_envs) * k.p.num_agents * 12;  // (a tape advances in a plain rollout too)
  if (k.traj_ep) k.traj_ep += k.p.num_envs;
  if (k.fin_obs) k.fin_obs += k.ring_obs;        // (the final record advances with the outputs: not in a plain rollout)
  if (k.fin_flags) k.fin_flags += k.ring_agent;
  if (k.ext) k.ext += k.ext_stride;  // (an action tape's next slot; 0 for a held action)
}

void last_kernel_add(const char* word) {
  std::strncat(g_last_kernel, word, sizeof(g_last_kernel) - std::strlen(g_last_kernel) - 1);
}

// what a map or map-set launch adds to cagpu_last_kernel(): " set" where the n-step kernels' MSET instantiations run (a set
// with n_steps > 1 in one launch), " map" for every other launch with a map or a set -- a single step of a set of one map
// names the kernel its single map does (a map-less launch: the string it always was)
void map_suffix(const KArgs& k, const bool mset = false) {
  last_kernel_add(mset ? " set" : ((k.env_map || k.map.static_bits) ? " map" : ""));
  if (k.ext_stride) last_kernel_add(" tape");
  if (k.rd_seed) last_kernel_add(" noise");  // (an RVO draw, CaRvoDraw: only the kernels that come through here run one)
}

// ---- ca_kernel: the instantiation a launch runs, in two steps.  main_geometry: N and the tile size compiled in (NC, TE)
// where an instantiation exists; main_variant: MULTI (n steps in one launch), RO (an auto-reset copies the case's reset
// observation) and MSET (a map set in an n-step launch: asked for with MULTI only -- the only launches that select it).
struct MainKernel {
  Kernel<KArgs> k;
  int nc, te;  // the NC and TE of the instantiation, as cagpu_last_kernel() spells them
};

template <int NT, bool STAGE, int NC, int TE = 0>
MainKernel main_variant(const bool multi, const bool ro, const bool mset) {
  if (multi && mset) {
    if (ro) return {kernel_of<&ca_kernel<NT, STAGE, NC, true, true, TE, true>>(), NC, TE};
    return {kernel_of<&ca_kernel<NT, STAGE, NC, true, false, TE, true>>(), NC, TE};
  }
  if (multi) {
    if (ro) return {kernel_of<&ca_kernel<NT, STAGE, NC, true, true, TE>>(), NC, TE};
    return {kernel_of<&ca_kernel<NT, STAGE, NC, true, false, TE>>(), NC, TE};
  }
  if (ro) return {kernel_of<&ca_kernel<NT, STAGE, NC, false, true, TE>>(), NC, TE};
  return {kernel_of<&ca_kernel<NT, STAGE, NC, false, false, TE>>(), NC, TE};
}

// ... with an RVO draw (CaRvoDraw): the RD instantiations, which exist in the general form (NC = 0: any N, the tile size read
// from the arguments) only; the n-step one is the MSET form, which carries a set where there is one and costs nothing without
template <int NT, bool STAGE>
MainKernel main_variant_rd(const bool multi, const bool ro) {
  if (multi) {
    if (ro) return {kernel_of<&ca_kernel<NT, STAGE, 0, true, true, 0, true, true>>(), 0, 0};
    return {kernel_of<&ca_kernel<NT, STAGE, 0, true, false, 0, true, true>>(), 0, 0};
  }
  if (ro) return {kernel_of<&ca_kernel<NT, STAGE, 0, false, true, 0, false, true>>(), 0, 0};
  return {kernel_of<&ca_kernel<NT, STAGE, 0, false, false, 0, false, true>>(), 0, 0};
}

template <int NT, bool STAGE>
MainKernel main_geometry(const KArgs& k, const bool multi, const bool ro, const bool mset) {
  if (k.rd_seed) return main_variant_rd<NT, STAGE>(multi, ro);
  if constexpr (NT <= 256) {  // the 512-thread geometry exists for large N only
    if (k.p.num_agents == 10) {  // N and the tile size compiled in
      if (k.tile_envs == ROW / 10) return main_variant<NT, STAGE, 10>(multi, ro, mset);
      if (k.tile_envs == 4) return main_variant<NT, STAGE, 10, 4>(multi, ro, mset);
    }
    if (k.p.num_agents == 20 && k.tile_envs == ROW / 20)  // BASELINE config 3 (4096 x 20)
      return main_variant<NT, STAGE, 20>(multi, ro, mset);
  }
  return main_variant<NT, STAGE, 0>(multi, ro, mset);
}

// one ca_kernel launch of `nt` threads per workgroup and `total` bytes of LDS, with or without the staging area
int launch_main1(const KArgs& k, const int nt, const bool stage, const size_t total, hipStream_t st) {
  const bool multi = k.mode == MODE_STEP && k.n_steps > 1;
  const bool ro = k.mode == MODE_STEP && k.table && k.reset_obs;
  const bool mset = multi && k.env_map;
  const MainKernel m = nt == 512 ? (stage ? main_geometry<512, true>(k, multi, ro, mset) : main_geometry<512, false>(k, multi, ro, mset))
                                 : (stage ? main_geometry<256, true>(k, multi, ro, mset) : main_geometry<256, false>(k, multi, ro, mset));
  const int tile_envs = k.tile_envs;
  const unsigned grid = static_cast<unsigned>((k.p.num_envs + tile_envs - 1) / tile_envs);
  std::snprintf(g_last_kernel, sizeof(g_last_kernel), "ca_kernel<%d, %s, %d, %s, %s, %d> grid=%u lds=%zu tile_envs=%d",
                nt, stage ? "true" : "false", m.nc, multi ? "true" : "false", ro ? "true" : "false", m.te, grid, total,
                tile_envs);
  map_suffix(k, mset);
  return launch_lds(m.k, dim3(grid), dim3(nt), total, st, k);
}

int launch_main(const KArgs& k, const int nt, hipStream_t st) {
  const int N = k.p.num_agents, W = 6 + 7 * k.p.max_obs;
  const int cs = k.col_stride;
  const size_t un_orca = lds_orca_bytes(N, cs);
  const int tti = k.p.sort_mode == CA_SORT_TIME_TO_IMPACT ? 1 : 0;
  size_t un_sense = lds_sense_bytes(N, W, 1, tti, cs);
  bool stage = true;
  size_t total = lds_fixed_bytes() + (un_orca > un_sense ? un_orca : un_sense);
  // Staging the tile's observation block in LDS (one coalesced copy-out) wins while every workgroup of the launch is
  // resident at once; for larger batches the smaller footprint without it (5 instead of 3 workgroups per CU at
  // N = 10) hides more latency: 145 vs 167 us at 32768 envs, 32.9 vs 30.7 us at 4096 (profiles/r01_kernel_geometry.md).
  const int n_cu = device_cus();
  const long wgs = (static_cast<long>(k.p.num_envs) + k.tile_envs - 1) / k.tile_envs;
  // (a fourth staged workgroup per CU fits the LDS on paper at N = 10 but measured 44 us at 5120 envs against 35 us for
  // the unstaged layout, so the staged layout is only kept up to three per CU)
  const long per_cu = static_cast<long>((160 * 1024) / total);
  const long resident_staged = (per_cu < 3 ? per_cu : 3) * n_cu;
  const bool crowded = wgs > resident_staged;
  if (total > 64 * 1024 || crowded) {  // give up the staging area
    un_sense = lds_sense_bytes(N, W, 0, tti, cs);
    stage = false;
    total = lds_fixed_bytes() + (un_orca > un_sense ? un_orca : un_sense);
  }
  if (total > 160 * 1024) return fail(CA_EUNSUPPORTED, "cagpu: num_agents too large for the 160 KiB LDS tile%s");
  // The fused n-step kernel (<= 128 VGPRs: four 4-wave workgroups per CU) only pays while the whole launch is resident
  // at once; otherwise n launches of the single-step kernel are faster (136 vs 158 us / step at 32768 envs) and give
  // bit-identical results (envs never interact; tests/test_gpu_parity.py::test_rollout_equals_repeated_steps).
  const long lds_cap = static_cast<long>((160 * 1024) / total);
  const long reg_cap = (N == 20) ? 2 : 4;  // (ca_kernel's __launch_bounds__)
  const long fused_resident = (lds_cap < reg_cap ? lds_cap : reg_cap) * n_cu;
  if (k.mode == MODE_STEP && k.n_steps > 1 && wgs > fused_resident) {
    KArgs k1 = k;
    k1.n_steps = 1;
    for (int i = 0; i < k.n_steps; ++i) {
      const int rc = launch_main1(k1, 256, stage, total, st);
      if (rc) return rc;
      ring_advance(k1);
    }
    return CA_OK;
  }
  return launch_main1(k, nt, stage, total, st);
}

// The software-pipelined kernel (cagpu_pipe.inc): the caller handed over CaState.next_action, the agent count has an
// instantiation, the sensor sorts closest_first, an attached fixture table comes with its reset observations, and the
// grid suits its 4-env tiles.
bool pipe_eligible(const KArgs& k) {
  const int n = k.p.num_agents;
  if (!k.s.next_action || k.stage_obs) return false;
  if (k.s.rvo_collab || k.s.rvo_heading_noise || k.s.ext_state) return false;  // (per-step inputs belong to the step that consumes them)
  if (k.rd_seed) return false;  // (an RVO draw, CaRvoDraw, is made by the query of the step that consumes it: no plan ahead)
  if (!(n == 10 || n == 8 || n == 6 || n == 5 || n == 4 || n == 3 || n == 2)) return false;  // (the instantiations)
  if (k.mode != MODE_STEP && k.mode != pipe::MODE_PLAN) return false;
  if (k.p.sort_mode != CA_SORT_CLOSEST_FIRST) return false;
  if (k.table && !k.reset_obs) return false;
  // grid: one round of resident workgroups (4 per CU), or at least two -- in between (1.5 rounds at 6144 envs) ca_kernel's
  // 6-env tiles fit the device better: 21.3 vs 22.9 us per step; from 8192 envs on this kernel is ahead again (28.9 vs 33.0
  // us; 32768 envs: 85.1 vs 87.8, fused rollout 65.7 vs 87.5 us per step; profiles/r03_kernel_geometry.md)
  if (n != 10) return true;
  const long wgs = (static_cast<long>(k.p.num_envs) + 3) / 4, cap = 4L * device_cus();
  return wgs <= cap || wgs >= 2 * cap;
}

// the epoch tags of the GA3C-CADRL packing counters (ga3c::tagged_add): no two packings of a process share a tag
uint32_t next_pack_epoch() {
  static std::atomic<uint32_t> epoch_source{static_cast<uint32_t>(std::chrono::steady_clock::now().time_since_epoch().count())};
  return epoch_source.fetch_add(1, std::memory_order_relaxed);
}

// ---- ca_pipe_kernel: the instantiation of a geometry (NC, TE, MULTI) that a launch runs.  Recording (TRAJ) and the final
// record (FINAL) are template flags: the instantiations without them are the code they were before; the episode log and
// the policy draw ride on the FINAL instantiations behind uniform tests of their pointers -- no flags of their own.  A map
// set in an n-step launch has one, MSET, on top of FINAL: the only launches that select it.  FAIR and MSET exist with MULTI
// only, MSET with FINAL only: the caller passes fair = mset = false without MULTI, and fin = true with mset.
using PipeKernel = void (*)(KArgs);
template <int NC, int TE, bool MULTI>
PipeKernel pipe_kernel(const bool fair, const bool traj, const bool fin, const bool mset) {
  using namespace pipe;
  constexpr bool FAIR = MULTI;  // (without MULTI the `fair` cases name the instantiations of their neighbours)
  if constexpr (MULTI) {
    if (mset) {
      if (traj) return fair ? &ca_pipe_kernel<NC, TE, true, true, true, true, true> : &ca_pipe_kernel<NC, TE, true, false, true, true, true>;
      return fair ? &ca_pipe_kernel<NC, TE, true, true, false, true, true> : &ca_pipe_kernel<NC, TE, true, false, false, true, true>;
    }
  }
  if (fin) {
    if (traj) return fair ? &ca_pipe_kernel<NC, TE, MULTI, FAIR, true, true> : &ca_pipe_kernel<NC, TE, MULTI, false, true, true>;
    return fair ? &ca_pipe_kernel<NC, TE, MULTI, FAIR, false, true> : &ca_pipe_kernel<NC, TE, MULTI, false, false, true>;
  }
  if (traj) return fair ? &ca_pipe_kernel<NC, TE, MULTI, FAIR, true> : &ca_pipe_kernel<NC, TE, MULTI, false, true>;
  return fair ? &ca_pipe_kernel<NC, TE, MULTI, FAIR> : &ca_pipe_kernel<NC, TE, MULTI, false>;
}

// KArgs.yield_t of a launch that gets the progress-fair priorities: the lead, in steps, over its CU's slowest workgroup from
// which a workgroup yields (the mechanism and its measurements: PIPE_PRIO in cagpu_pipe.inc)
constexpr int PIPE_YIELD_T = 2;
template <int NC, int TE, bool MULTI>
int launch_pipe2(const KArgs& k0, hipStream_t st) {
  using G = pipe::Geo<NC, TE>;
  static_assert(G::LDS <= 48 * 1024 && (NC != 10 || G::LDS <= 40 * 1024), "three (metric geometry: four) workgroups per CU");
  static_assert(TE <= 32 && NC * TE <= 64 && NC >= 2 && NC <= 10, "one agent wave per half; lp3_wave8 holds at most 9 lines");
  KArgs k = k0;
  const unsigned grid = static_cast<unsigned>((k.p.num_envs + TE - 1) / TE);
  k.inv_h_f = 1.0f / static_cast<float>(k.p.rvo_time_horizon);   // (x86 float division: correctly rounded, like the device's `/`)
  k.inv_dt_f = 1.0f / static_cast<float>(k.p.rvo_dt);
  // progress-fair priorities (PIPE_PRIO): an n-step launch whose workgroups are all resident at once and share their CUs
  k.yield_t = 0;
  if (MULTI) {
    const long cus = device_cus();
    const long per_cu = (160 * 1024) / static_cast<long>(G::LDS) < 4 ? (160 * 1024) / static_cast<long>(G::LDS) : 4;
    if (grid > cus && grid <= per_cu * cus) k.yield_t = PIPE_YIELD_T;
  }
  const bool fair = k.yield_t > 0, mset = MULTI && k.env_map;
  std::snprintf(g_last_kernel, sizeof(g_last_kernel), "ca_pipe_kernel<%d, %d, %s> grid=%u lds=%zu mode=%d%s%s%s%s", NC, TE,
                MULTI ? "true" : "false", grid, static_cast<size_t>(G::LDS), k.mode, fair ? " fair" : "",
                mset ? " set" : ((k.env_map || k.map.static_bits) ? " map" : ""), k.traj_rows ? " traj" : "",
                k.fin_obs ? " final" : "");
  if (k.log_rows) last_kernel_add(" log");
  if (k.draw_cdf) last_kernel_add(" draw");
  if (k.ext_stride) last_kernel_add(" tape");
  const bool fin = mset || k.fin_obs || k.log_rows || k.draw_cdf;
  return launch(pipe_kernel<NC, TE, MULTI>(fair, k.traj_rows != nullptr, fin, mset), dim3(grid), dim3(pipe::PNT), G::LDS, st, k);
}

template <int NC, int TE>
int launch_pipe1(const KArgs& k, hipStream_t st) {
  if (k.mode == MODE_STEP && k.n_steps > 1) return launch_pipe2<NC, TE, true>(k, st);
  return launch_pipe2<NC, TE, false>(k, st);
}

int launch_pipe(const KArgs& k, hipStream_t st) {
  switch (k.p.num_agents) {
    // 4-env tiles at EVERY batch size (1024 workgroups at the metric's 4096 envs, 4 per CU).  Smaller tiles for small batches
    // -- 1 / 2 / 3 envs per tile so that a 1024 / 2048 / 3072-env batch is still one full round of 1024 resident workgroups --
    // were built and measured in round 4 and are SLOWER: 12.41 vs 11.89 us per step at 1024 envs (BASELINE configs[1]), 13.35
    // vs 12.83 at 2048, 14.69 vs 14.05 at 3072 (profiles/r04_kernel_geometry.md).  A workgroup's duration is its serial
    // chain (a tile alone on a CU still needs ~9.5 us), not its pair work, so four times as many workgroups only add their
    // fixed costs and contend for the issue slots the chains need.
    // Round 6, the same question in ring mode (2- and 1-env tiles for grids of at most one 4-env workgroup per CU, same box,
    // 1024 x 10): ring of 64 8.10 -> 8.08 / 7.99 us per step, ring of 20 9.40 -> 9.40 / 9.46, 2000-step rollout 6.73 -> 6.57 / 6.45,
    // one launch per step 11.78 -> 11.92 / 12.18: below the 0.5 us bar in every mode a caller sees; not built
    // (profiles/r06_kernel_geometry.md).
    case 10: return launch_pipe1<10, 4>(k, st);
    case 8: return launch_pipe1<8, 8>(k, st);
    case 6: return launch_pipe1<6, 10>(k, st);
    case 5: return launch_pipe1<5, 12>(k, st);
    case 4: return launch_pipe1<4, 16>(k, st);
    case 3: return launch_pipe1<3, 21>(k, st);
    case 2: return launch_pipe1<2, 32>(k, st);
    default: return fail(CA_EUNSUPPORTED, "cagpu: no pipelined instantiation for this agent count%s");
  }
}

// Envs with more than 64 agents: the one-thread-per-agent kernel of cagpu_big.inc over the caller's workspace; as many
// workgroups as the workspace holds, each walking envs e = blockIdx, blockIdx + grid, ...; a rollout is n launches.
int launch_big(const KArgs& k0, hipStream_t st) {
  KArgs k = k0;
  const int N = k.p.num_agents;
  const size_t per = big::ws_bytes_per_wg(N);
  long wgs = static_cast<long>(k.o.workspace_bytes / per);
  if (wgs < 1) return fail(CA_EINVAL, "cagpu: CaOut.workspace is smaller than one workgroup's share (cagpu_workspace_bytes)%s");
  if (wgs > k.p.num_envs) wgs = k.p.num_envs;
  const int n_steps = (k.mode == MODE_STEP) ? k.n_steps : 1;
  k.n_steps = 1;
  const int nt = big::threads_for(N);
  const size_t lds = big::lds_bytes(nt);  // (1024 threads: 88 KB of LDS, above the default dynamic limit)
  std::snprintf(g_last_kernel, sizeof(g_last_kernel), "ca_big_kernel grid=%ld threads=%d ws_per_wg=%zu mode=%d", wgs, nt, per,
                k.mode);
  map_suffix(k);
  const auto plain = nt == 256 ? kernel_of<&big::ca_big_kernel<256>>()
                               : (nt == 512 ? kernel_of<&big::ca_big_kernel<512>>() : kernel_of<&big::ca_big_kernel<1024>>());
  const auto kernel = !k.rd_seed ? plain   // (an RVO draw, CaRvoDraw: the RD instantiations)
                      : (nt == 256 ? kernel_of<&big::ca_big_kernel<256, true>>()
                                   : (nt == 512 ? kernel_of<&big::ca_big_kernel<512, true>>() : kernel_of<&big::ca_big_kernel<1024, true>>()));
  for (int s = 0; s < n_steps; ++s) {
    const int rc = launch_lds(kernel, dim3(static_cast<unsigned>(wgs)), dim3(nt), lds, st, k,
                              static_cast<unsigned char*>(k.o.workspace), per);
    if (rc) return rc;
    ring_advance(k);
  }
  return CA_OK;
}

// Workgroup size (measured on MI355X at 4096 envs x 10 agents, profiles/r01_kernel_geometry.md): 256 threads for both the
// single-step kernel (30.7 us; 128 -> 39, 384 / 512 -> 40) and the n-step rollout kernel (22.2 us / step; 128 -> 28.8).
// The rollout kernel only reaches that since the build disables machine LICM (build_native.py): hoisted loop invariants
// had cost it 217 VGPRs (2 waves / SIMD: the 683 workgroups of 256 threads no longer fit at once) instead of 139.
int launch_any(const KArgs& k0, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  KArgs k = k0;
  const int N = k.p.num_agents;
  if (pipe_eligible(k)) return launch_pipe(k, st);
  if (k.mode != pipe::MODE_PLAN && N > 64) return launch_big(k, st);
  if (k.mode == pipe::MODE_PLAN) return fail(CA_EUNSUPPORTED, "cagpu_plan: needs CaState.next_action, num_agents in {2, 3, 4, 5, 6, 8, 10}, closest_first sorting and a grid of at most 4 x CUs or at least 8 x CUs tiles%s");
  k.tile_envs = ROW / N;
  k.col_stride = (N > 32) ? (N | 1) : CS_ROW;  // single-env tiles: only the N columns in use (see ca_kernel)
  // N = 10: tiles of 4 envs instead of 6 while that still gives at most 4 workgroups per CU (all co-resident, evenly
  // spread): 27.3 vs 30.9 us at 4096 envs, 23.3 vs 27.6 at 2048; beyond that the 6-env tile wins
  // (profiles/r01_kernel_geometry.md)
  if (N == 10 && k.mode == MODE_STEP && (static_cast<long>(k.p.num_envs) + 3) / 4 <= 4L * device_cus()) k.tile_envs = 4;
  // N > 32: the tile is a single env whose N^2 pair items (and N wave-wide linear programs) keep 8 waves busy, and
  // its LDS footprint allows only one or two workgroups per CU anyway
  return launch_main(k, N > 32 ? 512 : 256, st);
}

int pick_block(int N) { return N <= 64 ? 64 : (N <= 128 ? 128 : 256); }

template <int BLOCK>
int launch_orca(const OrcaArgs& k, hipStream_t st) {
  const int N = k.num_agents;
  const size_t total = static_cast<size_t>(BLOCK) * (5 * 4 + N * 4 + 2 * (N > 1 ? N - 1 : 1) * 16);
  if (total > 160 * 1024) return fail(CA_EUNSUPPORTED, "cagpu: num_agents too large for the 160 KiB LDS tile%s");
  const int tile_envs = BLOCK / N;
  const unsigned grid = static_cast<unsigned>((k.num_envs + tile_envs - 1) / tile_envs);
  return launch_lds(kernel_of<&orca_kernel<BLOCK>>(), dim3(grid), dim3(BLOCK), total, st, k);
}
