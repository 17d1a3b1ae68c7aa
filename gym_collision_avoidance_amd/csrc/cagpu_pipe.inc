// gym_collision_avoidance_amd/csrc/cagpu_pipe.inc -- included by cagpu.hip (inside its anonymous namespace, after ca_kernel).
//
// The software-pipelined step kernel (CaState.next_action, include/cagpu.h).
//
// The reference's step is a strict chain: policy query -> move -> collisions / rewards -> sensing -> done
// (collision_avoidance_env.py:156-234).  But the RVO policy of step t+1 is queried on the state the move of step t leaves
// (env.py:305-323 runs it BEFORE anyone moves), and that is exactly what the collision / sensing half of step t reads:
// after the move the two halves depend on the same tile and NOT on each other.  ca_kernel runs them one after the other on
// the same four waves, three of which wait at barriers while the agent wave walks its chains (SQ_WAIT_ANY 63 % of the wave
// cycles, profiles/r02_rocprof_summary.md).  Here a workgroup is 8 waves with fixed ROLES, each role its own straight-line
// programme (so the agent state of wave 0 does not occupy registers in the pair phases):
//   wave 0       S-agent : move, publish the post-move tile, rewards / collision flag (A3), done / game over / auto-reset (A4)
//   waves 1 - 3  S-pair  : collision gaps + sensor keys per unordered pair (P3), ranks + observation rows (P4), the
//                          reset-observation copy of an auto-reset env
//   wave 4       O-agent : its share of the ORCA pair phases, the scan of linearProgram2, the policy post-processing
//                          (atan2, pi/6 clip: RVOPolicy.py:96-111) -> next_action
//   waves 5 - 7  O-pair  : neighbour ranks + half-planes (P2), every line's 1-D programme (P2b), linearProgram3
// The two halves meet at ONE workgroup barrier per step -- B_P, after wave 0 has published the post-move tile -- and run
// free of each other behind it; every later hand-over is an arrival counter in LDS (sig() / wait_for() below) that only
// the waves concerned wait on:
//
//   wave 0: move + publish | ego frame . (late state) . A3 , A4 ............... store
//   S-pair:                | (P2 share) . P3 . (P2b share) . P4    . reset obs      (. linearProgram3 entries 4 - 6)
//   O     :                | P2   .  P2b  . scan (wave 4) . linearProgram3 . . post -> plan
//                        B_P
// ('.': a counter -- ego frame -> P3, P3 -> A3 / P4, P2 -> P2b, P2b -> scan, scan -> linearProgram3 (all seven pair waves),
//  linearProgram3 -> post, A4 -> reset obs / post; the shares in brackets: a tile with more planned agents than the four O
//  waves hold in one round of P2 / P2b hands the rest to two S-pair waves; `late state`: the arrays first needed here are
//  fetched last at the start of the launch and taken over at this point, so that the move does not wait for them)
// (Until round 3's second half the stages advanced in lock step through three more workgroup barriers: the O half, the
//  longer one, then stood ~1 us per step at barriers waiting for P4; rollout 7.84 -> 7.48 us per step.)
//
// The plan an O half produces -- {float32 speed, float32 delta heading, ORCA velocity} per agent, flagged CA_PLAN_VALID --
// is what the next step's move consumes (the next launch, or the next iteration of the n-step loop).  A tile whose agents
// hold no valid plan (first step after a reset / a host write, an auto-reset without CaAutoReset.reset_plan) runs the O
// half once on the PRE-move state first: the same code on the same inputs as the unpipelined kernel, so results are
// bit-identical either way (tests/test_gpu_parity.py: pipelined vs unpipelined state bit for bit, orca_vel vs the oracle).
// An agent that collides in step t was planned for in vain (the plan covers every agent that is not at its goal, out
// of time or in collision after the MOVE; the collision flag of step t is decided later): its plan is simply not used.
//
// Scope: num_agents compiled in -- 10 (tiles of 4 envs: the metric's geometry) and the reference's other fixture sizes 2,
// 3, 4, 5, 6, 8 (tiles of floor(64 / N) envs) --, closest_first sorting, precomputed reset observations when a fixture
// table is attached; everything else runs ca_kernel (same arithmetic).
namespace pipe {

constexpr int PNT = 512;                  // 8 waves
constexpr int S_PAIR = 192, O_LANES = 256;
enum { M_NEED = 0, M_NLIVE = 1, M_AGAIN = 2, M_CEGO = 3, M_CP3 = 4, M_CP2 = 5, M_CP2B = 6, M_CSCAN = 7, M_CA4 = 8,
       M_CLP3 = 9, M_CRC = 10, M_YIELD = 11, M_PSLOT = 12 };  // sh_misc slots (3 ..: arrival counters)
enum { MODE_PLAN = 3 };                   // (continues MODE_STEP / MODE_RESET / MODE_OBSERVE)

// The workgroup barrier of a step (B_P; B_A once at the start; the n-step loop's B_5 is a full __syncthreads()).  What the
// waves exchange travels through LDS only, so the barrier waits for this wave's LDS traffic (lgkmcnt), not for the
// acknowledgement of its outstanding global stores (vmcnt).  The one place where global stores of different waves to the
// SAME address must stay ordered (the reset-observation copy over rows P4 and A3 wrote) drains vmcnt itself before it
// signals.
#define PIPE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// Barriers among SOME of the workgroup's waves (gfx950 has no named barriers): an arrival counter in LDS.  sig() publishes
// this wave's LDS writes and counts it in; wait_for() polls until `target` waves have arrived.  Every hand-over behind B_P
// is one of these (the list is in the header of this file), so that no wave stands at a barrier for a phase it does not
// depend on (P3 is half as long as P2, P4 half again as long as P2b; the scan and the post run on one wave).  Wave 0 zeroes
// the counters at every publish -- between a step's last wait and the next publish every wave is on its way to a workgroup
// barrier -- so all targets are constants.  The poll is bounded (never a hung device) and falls through when it runs out.
// That is made OBSERVABLE without touching the polls (a bound test behind every poll cost 0.15 us per step, a re-read of
// the counter 0.3 us: each sits on a hand-over of the step's critical chain -- profiles/r04_kernel_geometry.md): at the end
// of every O half wave 4, which by then has waited (directly or through wave 0's A4) for every hand-over of the step,
// AUDITS the arrival counters -- each must hold exactly its target.  A miscounted hand-over (an edit of the helper counts)
// or a poll that ran out before its producer arrived leaves a counter off its target; bit 0 of the device's fault word is
// raised, which the host reads with cagpu_device_faults() (core.BatchedSim.check_faults(), after every GPU test).
// (g_fault, the device's fault word, is defined in cagpu.hip: bit 0 is this file's, bit 1 the GA3C-CADRL range guard's)
__device__ __forceinline__ void sig(int* c) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// SL: the s_sleep between two polls (x 64 cycles).  A poll is an LDS read + a v_readfirstlane: it takes a VALU issue slot from
// the waves that work.  The hand-overs of a step's critical chain poll at SL = 1; a wave whose wait is NOT on that chain as a
// rule (NC_SLEEP: the S-pair waves behind their P4, the O-pair waves behind their 1-D programmes) sleeps longer.
// Measured (r06g, same box; VALU instructions of a 50-step launch 211.9 M -> 208.3 M at 4, LDS instructions 30.2 M -> 27.8 M):
// 2000-step rollout 7.73 -> 7.70 (2) / 7.70 (4) / 7.72 (8) us per step, ring of 50 9.03 -> 9.01 / 9.00 / 9.02; 1024 envs (one
// workgroup per CU: the wake-up counts, the issue slots do not) 7.96 -> 7.96 / 7.97 / 8.04.  2 it is.
constexpr int NC_SLEEP = 2;
template <int SL = 1>
__device__ __forceinline__ void wait_for(int* c, const int target) {
  for (int spin = 0; spin < (1 << 22); ++spin) {
    const int v = __builtin_amdgcn_readfirstlane(__hip_atomic_load(c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (v >= target) break;
    __builtin_amdgcn_s_sleep(SL);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int SL = 1>
__device__ __forceinline__ void wait_for2(int* c1, const int t1, int* c2, const int t2) {  // both, one LDS round trip per poll
  for (int spin = 0; spin < (1 << 22); ++spin) {
    const int v1 = __hip_atomic_load(c1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const int v2 = __hip_atomic_load(c2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (__builtin_amdgcn_readfirstlane(v1) >= t1 && __builtin_amdgcn_readfirstlane(v2) >= t2) break;
    __builtin_amdgcn_s_sleep(SL);
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Wave priorities (s_setprio): wave 0's chains and the linearProgram3 / scan / post stages at 3 (everybody else of the
// workgroup waits for them), the ORCA pair phases at 2; the sensing pair phases P3 / P4 at S_PRIO / S_PRIO4.
// Measured in one gpurun call (profiles/r03_kernel_geometry.md): P3 / P4 at 1 / 0: 15.55 us per step; 0 / 0: 15.66; 1 / 1:
// 15.66; 2 / 2: 16.4; 3 / 3: 16.8 -- the CU's VALU issue is nearly saturated now, and what the ORCA chain (the longer half)
// does not get it cannot make up.
constexpr int S_PRIO = 1, S_PRIO4 = 0, O_PRIO = 2;

// Progress-fair issue priorities among the workgroups that share a CU (round 6; KArgs.yield_t = T > 0, set by the launcher for an
// n-step launch whose whole grid is resident at once).  A short n-step launch ends with its slowest workgroup, and within a CU
// the slowness is systematic: the hardware arbitrates waves of equal s_setprio oldest first, so the workgroups dispatched last
// (blocks b + 512, b + 768 of a CU's four) run ~10 % slower than their CU-mates for the whole launch -- every one of the twelve last
// finishers of a 20-step launch had a block index >= 512 (profiles/r06_kernel_geometry.md).  Every workgroup therefore
// publishes the number of steps it has completed in a per-CU table in global memory (row keyed by the hardware's CU id, slot
// from a per-CU arrival counter) and reads its CU-mates' once per step -- on the first S-pair wave, at the end of its step,
// where nobody waits for it --; a workgroup that is >= T steps ahead of the slowest one of its CU runs its next step with every
// wave at priority <= Y_LEVEL.  Only s_setprio operands depend on it: results cannot change.  Measured (same box,
// 4096 x 10): spread of the workgroups' totals within a CU 11.4 -> 5.2 us, 20-step launch 10.23 -> 9.83 us per step, 50-step 9.36 ->
// 9.02, 2000-step rollout 7.66 -> 7.73 (the exchange + yielding cost ~1 % where no tail is left to win).
constexpr int Y_LEVEL = 1;
__device__ unsigned int g_cu_slot[16 * 256];
__device__ unsigned int g_prog[16 * 256 * 4];
// FAIR is a template parameter of the kernel: the instantiation without it is round 5's code to the instruction (every PIPE_PRIO
// a plain s_setprio) and serves every launch the launcher does not switch the mechanism on for -- grids that are not resident at
// once, one workgroup per CU, single steps; the branches around the priorities alone cost 1.6 - 1.9 % there (r06f).
#define PIPE_PRIO(x) do { if (FAIR && yield_) __builtin_amdgcn_s_setprio((x) < Y_LEVEL ? (x) : Y_LEVEL); else __builtin_amdgcn_s_setprio(x); } while (0)
// The yield flag of a step travels in bit 8 of the word every wave reads behind the publish barrier anyway (M_NLIVE: the tile's
// planned agents, <= 64): no LDS read of its own on any wave's way out of the barrier.  The exchange writes M_YIELD before B_5,
// wave 0 folds it into the next publish.
#define PIPE_NLIVE(word) ((word) & 0xFF)
#define PIPE_YIELD_OF(word) (FAIR && ((word) >> 8) != 0)
// PIPE_ONCE(var) <phase>: the phase as the body of a loop of ONE trip that ends by handing `var` through an empty asm (a VGPR
// in, the same VGPR out: no instruction).  What is left of a switch that could run a phase twice for counter measurements; the
// switch is gone, the shape stays because the compiler's output rests on it: the one-trip loop changes how the loops inside
// the phase are strength-reduced, the empty asm where `var` lives.  Without it all 112 instantiations of the kernel come out
// as other code (other scalar registers, other instruction counts), and that is a change to measure, not to slip into a clean-up.
#define PIPE_ONCE(var) for (int once_ = 0; once_ < 1; ++once_, ({ asm volatile("" : "+v"(var)); }))

// floor(w / n) for the item decomposition of the 1-D programmes (w < 1200 items, n <= 64 planned agents) as (w * kMagic20.v[n]) >> 20:
// exact on that range (checked exhaustively), two integer instructions per item and one scalar table load per wave and step
// where the float form needed an IEEE 1 / n per wave and round (12 VALU instructions) + four per item (round 6).
struct Magic20 {
  unsigned int v[65];
  constexpr Magic20() : v() {
    for (int n = 1; n < 65; ++n) v[n] = (1u << 20) / static_cast<unsigned>(n) + 1u;
  }
};
__constant__ const Magic20 kMagic20 = Magic20();

template <int NC, int TE>
struct Geo {
  static constexpr int N = NC, TILE_N = TE * NC, GN = NC - 1;
  static constexpr int CS = TILE_N | 1;   // odd column stride of the [slot][CS] tiles (see CS_ROW in cagpu.hip)
  static constexpr int LINES = (NC - 1) * CS, CELLS = NC * CS;
  static constexpr size_t FIXED = ROW * (17 * 8 + 16 + 10 * 4 + 9 * 4) + 68 * 4 + 48 * 4;
  static constexpr size_t ORCA = (static_cast<size_t>(LINES) * 25 + 15) / 16 * 16;
  static constexpr size_t SENSE = (static_cast<size_t>(CELLS) * 32 + 15) / 16 * 16;
  static constexpr size_t LDS = FIXED + ORCA + SENSE;
};

// Every role programme reads the kernel arguments through its OWN laundered view of the kernarg segment: otherwise the
// loads the three programmes have in common (most of CaParams) are merged into the entry block, where 48 SGPRs of them
// are spilled at once (and a kernel with SGPR spills is given a scratch segment it never touches).
#if defined(__HIP_DEVICE_COMPILE__)
#define PIPE_ROLE_KARGS()                                                        \
  typedef __attribute__((address_space(4))) const KArgs RoleKArgs;               \
  RoleKArgs* k_ptr_ = (RoleKArgs*)__builtin_amdgcn_kernarg_segment_ptr();        \
  asm volatile("" : "+s"(k_ptr_));                                               \
  RoleKArgs& k = *k_ptr_;                                                        \
  auto& p = k.p
#else
#define PIPE_ROLE_KARGS() const KArgs& k = karg; const CaParams& p = k.p
#endif

// TRAJ: the instantiation also records the trajectory tape (CaTraj, KArgs.traj_rows != nullptr).  A template flag and not
// a uniform test: the programmes below are tuned down to their register counts, and the instantiations without the flag are
// the code they were before the tape existed.
// FINAL: the instantiation also keeps the final record (CaFinal, KArgs.fin_obs != nullptr) of the envs that auto-reset: wave 0
// stores the terminal flag words in A4, the S-pair waves save the terminal rows in front of their reset-observation copy.
// A template flag for the same reason.
// MSET: the n-step form (MULTI) also runs the map-set code of the single-step form -- the per-env grid of A3, the map draw
// of an auto-reset.  Only a set launch with n_steps > 1 selects it (pipe_kernel in cagpu_launch.inc, always together with FINAL).  A flag of its
// own and not a uniform test inside the FINAL instantiations: behind a test the set code cost those kernels -- which
// map-less launches with the final record, the episode log or the policy draw run -- their register budget (scratch
// spills inside the step loop at N = 10); with the flag every instantiation without it is the code it was.
template <int NC, int TE, bool MULTI, bool FAIR = false, bool TRAJ = false, bool FINAL = false, bool MSET = false>
__global__ __launch_bounds__(PNT, 8) void ca_pipe_kernel(const KArgs karg) {
  static_assert(MULTI || !FAIR, "progress-fair priorities belong to the n-step kernel");
  using G = Geo<NC, TE>;
  constexpr int N = NC, CS = G::CS, GN = G::GN, TILE_N = G::TILE_N;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int K = karg.p.max_obs, W = 6 + 7 * K;
  const int tid = threadIdx.x;
  const int role = __builtin_amdgcn_readfirstlane(tid >> 6);
  // (Round 6, measured and not built: block -> tile through a table that deals the tiles to the CUs snake-wise by planned-agent
  //  count -- the CUs' totals correlate 0.83 with it.  Probed from the host: 20-step launch 197.2 -> 192.5 us, spread of the CUs'
  //  totals 9.1 -> 6.7 us; 50-step launch 462.6 -> 466.4: the counts at the start of a launch say little about its second half.
  //  A sort per launch for 2 % of a short one: profiles/r06_kernel_geometry.md.)
  const long env0 = static_cast<long>(blockIdx.x) * TE;
  const long tile_base = env0 * N;

  // ---- LDS
  double* sh_px = reinterpret_cast<double*>(smem);
  double* sh_py = sh_px + ROW;
  double* sh_vx = sh_py + ROW;
  double* sh_vy = sh_vx + ROW;
  double* sh_rad = sh_vy + ROW;
  double* sh_prx = sh_rad + ROW;   // ego frame ref_prll (ref_orth = (-pry, prx))
  double* sh_pry = sh_prx + ROW;
  double* sh_head = sh_pry + ROW;  // heading (the policy post-processing of the O half)
  double* sh_gx = sh_head + ROW;   // goal / preferred speed: the preferred velocity of the O half
  double* sh_gy = sh_gx + ROW;
  double* sh_ps = sh_gy + ROW;
  double* sh_r0 = sh_ps + ROW;     // episode reward / Agent.t (parked by wave 0; A4 sums them per env) / t - slt
  double* sh_r1 = sh_r0 + ROW;
  double* sh_r2 = sh_r1 + ROW;
  double* sh_tr = sh_r2 + ROW;     // parked by wave 0: time_remaining, straight-line time
  double* sh_slt = sh_tr + ROW;
  double* sh_td = sh_slt + ROW;    // parked by wave 0: Agent.turning_dir (where CaState.turning_dir is given)
  float4* sh_plan = reinterpret_cast<float4*>(sh_td + ROW);  // the plan of the NEXT step, O half -> wave 0
  float* sh_fpx = reinterpret_cast<float*>(sh_plan + ROW);   // ORCA's float bodies
  float* sh_fpy = sh_fpx + ROW;
  float* sh_fvx = sh_fpy + ROW;
  float* sh_fvy = sh_fvx + ROW;
  float* sh_frad = sh_fvy + ROW;
  float* sh_fms = sh_frad + ROW;   // speed limit (float pref_speed)
  float* sh_fprx = sh_fms + ROW;   // preferred velocity (float)
  float* sh_fpry = sh_fprx + ROW;
  float* sh_vrx = sh_fpry + ROW;   // ORCA velocity of a linearProgram3 agent
  float* sh_vry = sh_vrx + ROW;
  uint32_t* sh_flag = reinterpret_cast<uint32_t*>(sh_vry + ROW);
  int* sh_isq = reinterpret_cast<int*>(sh_flag + ROW);  // 1: this agent is planned for (queries ORCA)
  int* sh_q = sh_isq + ROW;                             // compact list of those agents
  int* sh_nb = sh_q + ROW;                              // neighbour count
  int* sh_w0 = sh_nb + ROW;                             // [5][ROW] wave 0's per-lane scalars, parked across the step loop
  int* sh_q3 = sh_w0 + 5 * ROW;                         // linearProgram3 queue: [0] = length, [1 ..] = entries (68 ints)
  int* sh_rc = sh_q3 + 68;                              // [32] case index + 1 of an env that auto-reset in this step
  int* sh_misc = sh_rc + 32;                            // [16] M_*
  unsigned char* un = smem + G::FIXED;
  float4* Lmat = reinterpret_cast<float4*>(un);                      // [N-1][CS] half-planes
  float2* Rmat = reinterpret_cast<float2*>(Lmat + G::LINES);         // [N-1][CS] 1-D optimum on line i
  uint8_t* okmat = reinterpret_cast<uint8_t*>(Rmat + G::LINES);      // [N-1][CS] line i feasible
  double* omat = reinterpret_cast<double*>(un + G::ORCA);            // [N][CS] p_orth
  double* gmat = omat + G::CELLS;                                    // [N][CS] centre distance - combined radius
  double* pmat = gmat + G::CELLS;                                    // [N][CS] p_prll (the observation row's first entry)
  int* kmat = reinterpret_cast<int*>(pmat + G::CELLS);               // [N][CS] sort key
  float* d2mat = reinterpret_cast<float*>(kmat + G::CELLS);          // [N][CS] dist_2_other

  const bool plan_mode = karg.mode == MODE_PLAN;
  const int n_steps = plan_mode ? 0 : (MULTI ? karg.n_steps : 1);
  const bool ragged = karg.p.ragged != 0;

  // ================= P2 (one round of one wave): every (planned agent, other) pair of the agents sh_q[c0 + wvq * APW ..):
  // neighbour rank (ascending distSq, ties by index: Agent::insertAgentNeighbor) + ORCA half-plane.  A wave holds WHOLE
  // agents, lane = (agent, one of its N - 1 others).  Shared by the O waves (wvq 0 - 3) and the S-pair helpers (wvq 4, 5).
  constexpr int P2_APW = 64 / GN;     // agents per wave
  constexpr int P2_APR = 4 * P2_APW;  // agents per round of the four O waves
  constexpr int P2_HELPERS = 2;
  const auto p2_round = [&](const int c0, const int wvq, const int wl, const int n_live, const bool unlimited,
                            const float range_sq, const int max_nb, const float collab, const float inv_h,
                            const float inv_dt) {
    const int g = div_small<GN>(wl, 0.f), jo = wl - __mul24(g, GN);
    const int gbase = (wl - jo) << 2;  // ds_bpermute byte address of the first lane of my agent's group
    const int c = c0 + wvq * P2_APW + g;
    const bool valid = (g < P2_APW) && (c < n_live);
    const int ag = sh_q[valid ? c : 0];
    const int eb = __mul24(div_small<N>(ag, 0.f), N), aa = ag - eb;
    const int j = jo + ((jo >= aa) ? 1 : 0);  // my other agent (index order is kept: ties by index)
    const F2 mpos = f2(sh_fpx[ag], sh_fpy[ag]);
    float dj = INFINITY;
    if (valid && j < N) {
      const F2 d = mpos - f2(sh_fpx[eb + j], sh_fpy[eb + j]);
      dj = dotf(d, d);
      if (!unlimited && !(dj < range_sq)) dj = INFINITY;
    }
    int rank = 0, cnt = N - 1, tie = 0;
#pragma unroll
    for (int q = 0; q < GN; ++q) {
      const float dq = __int_as_float(__builtin_amdgcn_ds_bpermute(gbase + 4 * q, __float_as_int(dj)));
      rank += static_cast<int>(dq < dj);
      tie += static_cast<int>(dq == dj);
    }
    if (__any(tie > 1 && dj < INFINITY)) {  // (a distance always equals itself)
#pragma unroll
      for (int q = 0; q < GN; ++q) {
        const float dq = __int_as_float(__builtin_amdgcn_ds_bpermute(gbase + 4 * q, __float_as_int(dj)));
        rank += static_cast<int>(dq == dj) & static_cast<int>(q < jo);
      }
    }
    if (!unlimited || ragged) {  // a finite neighborDist / absent slots: count who is a neighbour
      cnt = 0;
#pragma unroll
      for (int q = 0; q < GN; ++q)
        cnt += static_cast<int>(__int_as_float(__builtin_amdgcn_ds_bpermute(gbase + 4 * q, __float_as_int(dj))) < INFINITY);
    }
    const int n = cnt < max_nb ? cnt : max_nb;
    if (valid) {
      if (jo == 0) sh_nb[ag] = n;
      if (dj < INFINITY && rank < n) {
        Lmat[rank * CS + ag] = half_plane_sel(mpos, f2(sh_fvx[ag], sh_fvy[ag]), sh_frad[ag],
                                               f2(sh_fpx[eb + j], sh_fpy[eb + j]), f2(sh_fvx[eb + j], sh_fvy[eb + j]),
                                               sh_frad[eb + j], collab, inv_h, inv_dt);
      }
    }
  };

  // ================= P2b (one round of 64-lane waves): linearProgram1 of line i against the lines before it, one thread per
  // (agent, i), highest lines first (see ca_kernel): the 1-D optimum on line i depends on the lines [0, i), the speed disc and
  // the preferred velocity only, so linearProgram2 shrinks to the scan of the O half.  Item w = base_ + to.  Shared by the O
  // waves and the S-pair helpers (a tile whose items do not fit one round of the four O waves).
  const auto p2b_round = [&](const int base_, const int to, const int n_live, const unsigned magic) {
    const int n_lp1 = n_live * (N - 1);
    const int w = base_ + to;
    const bool item = w < n_lp1;
    const int w_lo = base_ + (to & ~63);  // the wave's first item holds its highest line
    if (w_lo >= n_lp1) return;            // wave-uniform: no item of this wave in this round
    const int i_hi = __builtin_amdgcn_readfirstlane((N - 2) - static_cast<int>((static_cast<unsigned>(w_lo) * magic) >> 20));
    const int wq = item ? static_cast<int>((static_cast<unsigned>(w) * magic) >> 20) : 0;   // floor(w / n_live): see kMagic20
    const int i = item ? (N - 2) - wq : 0;
    const int ag = sh_q[item ? w - wq * n_live : 0];
    const bool live = item && i < sh_nb[ag];
    const float4 li = Lmat[i * CS + ag];
    const F2 Pi = f2(li.x, li.y), Di = f2(li.z, li.w);
    const float radius = sh_fms[ag];
    const F2 opt = f2(sh_fprx[ag], sh_fpry[ag]);
    const float dp = dotf(Pi, Di);
    const float disc = sqf(dp) + sqf(radius) - dotf(Pi, Pi);
    bool ok = !(disc < 0.0f);
    const float sd = sqrtq(ok ? disc : 0.0f);
    float t_lo = -dp - sd;
    float t_hi = -dp + sd;
    // intersect line i with the lines m < i, TWO per iteration.  Each line stays the float4 it is fetched as (ds_read_b128: one
    // conflict-free LDS pass; the same eight dwords as two-dword reads a row apart would put four lanes on every bank) and its
    // halves are used where they land: (x, y) = Pm and (z, w) = Dm are adjacent registers, so Pi - Pm is one packed subtract
    // and either determinant one packed multiply against the swapped halves of the other operand + one subtract -- Pi / Di
    // stand in one register pair each for the whole loop.  Only the two quotients are paired ACROSS the lines (den and num
    // are computed straight into the halves of a pair), so the divide chains run packed.  (Pairing the determinants across
    // the lines as well, as the compiler did with the scalar text, saves two multiplies and costs ten register copies per
    // iteration to line the components up.)  The lines are fetched one iteration ahead into the OTHER of two register sets
    // (A, B): no copy from `next` to `current` either.
    // Rows are wave-uniform: iteration m reads rows (m, m + 1) for every lane, m + 1 <= i_hi <= N - 2; the fetch ahead is
    // held to the last pair of rows (PAIR_HI, PAIR_HI + 1) = (N - 3, N - 2), so no read leaves rows 0 .. N - 2 of Lmat
    // (N = 2: Lmat is one row, the "next row" is the same row; its loop never runs).
    // What a row at or beyond an agent's neighbour count n holds is stale -- a line of an earlier step, or whatever the LDS
    // held at the launch.  Nothing of it reaches a stored result: a line m enters t_lo / t_hi / ok only through use0 / use1
    // (m < i), every value here is private to its lane, and `live` gates both stores -- a live item has i < n, so the lines
    // it uses, m < i < n, were all written by this step's P2; an item with i >= n may read stale rows and is not stored.
    typedef float v2f __attribute__((ext_vector_type(2)));
    typedef float v4f __attribute__((ext_vector_type(4)));
    constexpr int PAIR_HI = (N >= 3) ? N - 3 : 0, NEXT_ROW = (N >= 3) ? CS : 0;
    const float4* const lcol = Lmat + ag;
    const v2f Pi2 = v2f{Pi.x, Pi.y}, Di2 = v2f{Di.x, Di.y};
    float eps = kRvoEps;  // one scalar register for the whole loop
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+s"(eps));
#endif
    // (the empty asm behind a fetch keeps it where it is written, one iteration ahead of its use: left alone the compiler sinks
    //  the loads to their first use, and the loop stands at s_waitcnt for every line it has just asked for)
    const auto pair_at = [&](const int m, v4f& l0, v4f& l1) {  // m: uniform
      const v4f* const q = reinterpret_cast<const v4f*>(lcol + (m < PAIR_HI ? m : PAIR_HI) * CS);
      l0 = q[0];
      l1 = q[NEXT_ROW];
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" ::: "memory");
#endif
    };
    const auto lines2 = [&](const int m, const v4f l0, const v4f l1) {
      const bool use0 = m < i, use1 = m + 1 < i;  // (i <= i_hi: the wave's first item holds its highest line)
      const v2f dP0 = Pi2 - l0.xy, dP1 = Pi2 - l1.xy;
      const v2f a0 = Di2 * l0.wz, a1 = Di2 * l1.wz;  // detf(Di, Dm) = Di.x Dm.y - Di.y Dm.x
      const v2f c0 = l0.zw * dP0.yx, c1 = l1.zw * dP1.yx;  // detf(Dm, Pi - Pm)
      float den0 = a0.x - a0.y, den1 = a1.x - a1.y, num0 = c0.x - c0.y, num1 = c1.x - c1.y;
#if defined(__HIP_DEVICE_COMPILE__)
      // (four plain subtracts, each into its half of a pair: as one expression the compiler pairs them across the lines and
      //  pays three copies per packed subtract)
      asm volatile("" : "+v"(den0), "+v"(den1), "+v"(num0), "+v"(num1));
#endif
      const v2f den = v2f{den0, den1}, num = v2f{num0, num1};
      const bool par0 = fabsf(den0) <= eps, par1 = fabsf(den1) <= eps;
      ok = ok & !(use0 & par0 & (num0 < 0.0f)) & !(use1 & par1 & (num1 < 0.0f));
      // divq(num, den) for both lines at once.  A parallel line's quotient (den ~ 0: anything, inf and NaN included) is never
      // looked at: lp1_interval_pair reads tt only behind |den| > eps, so the divisor needs no `par ? 1 : den`.
      v2f y = v2f{__builtin_amdgcn_rcpf(den0), __builtin_amdgcn_rcpf(den1)};
      const v2f e = __builtin_elementwise_fma(-den, y, v2f(1.0f));
      y = __builtin_elementwise_fma(e, y, y);
      v2f q = num * y;
      v2f r = __builtin_elementwise_fma(-den, q, num);
      q = __builtin_elementwise_fma(r, y, q);
      r = __builtin_elementwise_fma(-den, q, num);
      const v2f tt = __builtin_elementwise_fma(r, y, q);
      lp1_interval_pair(use0, use1, den0, den1, tt.x, tt.y, t_lo, t_hi, eps);
    };
    v4f a0_, a1_, b0_, b1_;
    pair_at(0, a0_, a1_);
    for (int m = 0; m < i_hi; m += 4) {
      pair_at(m + 2, b0_, b1_);
      lines2(m, a0_, a1_);
      if (m + 2 >= i_hi) break;
      pair_at(m + 4, a0_, a1_);
      lines2(m + 2, b0_, b1_);
    }
    ok = ok && !(t_lo > t_hi);
    const float t = dotf(Di, opt - Pi);
    const float tc = (t < t_lo) ? t_lo : ((t > t_hi) ? t_hi : t);
    const F2 res = Pi + tc * Di;
    if (live) {
      Rmat[i * CS + ag] = make_float2(res.x, res.y);
      okmat[i * CS + ag] = ok ? 1 : 0;
    }
  };

  if (role == 0) {
    // =====================================================================================================================
    // wave 0: the S-agent programme (one lane per agent).  Registers hold what every phase touches (position, velocity,
    // heading, flags, the last action); what one phase of a step reads -- goal, radius, preferred speed, the clocks, the
    // episode reward -- is parked in the lane's LDS column between uses, so the programme fits the 64 VGPRs of 8 waves / SIMD.
    PIPE_ROLE_KARGS();
    int lane = tid;
    int le = div_small<NC>(lane, 0.f), a = lane - le * N;
    bool active = (lane < TILE_N) && (env0 + le < p.num_envs);
    int ebase = active ? le * N : 0;
    // (global indices are written as (uniform array + tile base)[lane]: no 64-bit per-lane index to keep alive)
    float* obs_tile = k.o.obs + tile_base * W;
    long out_base = tile_base, out_env = env0;  // n-step kernel: + this step's slot of the caller's output ring (cagpu_rollout_ring)
    // trajectory tape (TRAJ): this tile's rows / its envs' episode entries in the slot of the current step (uniform pointers)
    double* traj_tile = TRAJ ? k.traj_rows + tile_base * 12 : nullptr;
    int32_t* traj_ep = (TRAJ && k.traj_ep) ? k.traj_ep + env0 : nullptr;
    double px = 0.0, py = 0.0, vx = 0.0, vy = 0.0, heading = 0.0;
    float act0 = 0.f, act1 = 0.f;
    uint32_t flags = CA_DONE | CA_AT_GOAL;
    int step_num = 0, ep_step = 0, reset_cnt = 0;
    float4 plan = make_float4(0.f, 0.f, 0.f, 0.f);
    double* const sh_epr = sh_r0;  // parked: episode reward, Agent.t (A4 reads exactly these two columns of its env)
    double* const sh_t = sh_r1;
    // fetched at the start but first needed AFTER the publish barrier (parked / taken over there, first step only): the
    // move does not wait for them -- a launch's 1024 workgroups all load at once and the burst is bandwidth-bound
    // (with 8 instead of 19 arrays in front of the move the load phase measured 1.04 instead of 1.48 us)
    double l_t, l_slt, l_epr, l_td;
    float l_a0, l_a1;
    int l_sn, l_es, l_rc;
    {
      double gx = 0.0, gy = 0.0, rad = 1.0, ps = 1.0, tr = 0.0;
      // Every array's base pointer first, then every load back to back: left to itself the compiler fetched the kernarg
      // segment in four pieces, each with its own scalar-cache round trip between the groups of loads, and sank the plan's
      // load behind the test of the flags (a second memory round trip) -- all of it in front of the workgroup's first
      // barrier, where seven waves wait for this one.
      const double* const q_px = k.s.pos_x + tile_base; const double* const q_py = k.s.pos_y + tile_base;
      const double* const q_vx = k.s.vel_x + tile_base; const double* const q_vy = k.s.vel_y + tile_base;
      const double* const q_hd = k.s.heading + tile_base;
      const double* const q_gx = k.s.goal_x + tile_base; const double* const q_gy = k.s.goal_y + tile_base;
      const double* const q_rad = k.s.radius + tile_base; const double* const q_ps = k.s.pref_speed + tile_base;
      const double* const q_tr = k.s.time_remaining + tile_base; const double* const q_t = k.s.t + tile_base;
      const double* const q_slt = k.s.slt + tile_base; const double* const q_epr = k.s.ep_reward + tile_base;
      const double* const q_td = k.s.turning_dir ? k.s.turning_dir + tile_base : q_t;  // (zeroed below where not given)
      const float2* const q_la = reinterpret_cast<const float2*>(k.s.last_action) + tile_base;
      const uint32_t* const q_fl = k.s.flags + tile_base;
      const int32_t* const q_sn = k.s.step_num + tile_base;
      const int32_t* const q_es = k.s.episode_step + env0; const int32_t* const q_rc = k.s.reset_count + env0;
      const float4* const q_pl = reinterpret_cast<const float4*>(k.s.next_action) + tile_base;
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" :: "s"(q_px), "s"(q_py), "s"(q_vx), "s"(q_vy), "s"(q_hd), "s"(q_gx), "s"(q_gy), "s"(q_rad), "s"(q_ps),
                   "s"(q_tr), "s"(q_t), "s"(q_slt), "s"(q_epr), "s"(q_td), "s"(q_la), "s"(q_fl), "s"(q_sn), "s"(q_es),
                   "s"(q_rc), "s"(q_pl));
#endif
      float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
      if (active) {
        flags = q_fl[lane];
        pl = q_pl[lane];
        px = q_px[lane]; py = q_py[lane]; heading = q_hd[lane];
        gx = q_gx[lane]; gy = q_gy[lane]; tr = q_tr[lane];
        ps = q_ps[lane]; rad = q_rad[lane];
        vx = q_vx[lane]; vy = q_vy[lane];   // (first read by the publish)
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(pl.x), "+v"(pl.y), "+v"(pl.z), "+v"(pl.w));  // (the plan is fetched whatever the flags say)
#endif
        if (flags & CA_PLAN_VALID) plan = pl;
      }
      // The arrays first needed behind the publish barrier: issued LAST (loads return in order) and for every lane -- a
      // lane without an agent reads agent 0's and never uses it --, so that no merge with a default value stands between
      // the load and its first use: the move does not wait for these.
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("" ::: "memory");  // (the scheduler must not move these loads in front of the ones above)
#endif
      {
        const int li = active ? lane : 0, lei = active ? le : 0;
        l_t = q_t[li]; l_slt = q_slt[li]; l_epr = q_epr[li]; l_td = q_td[li];
        const float2 la = q_la[li];
        l_a0 = la.x; l_a1 = la.y;
        l_sn = q_sn[li];
        l_es = q_es[lei];
        l_rc = q_rc[lei];
      }
      sh_gx[lane] = gx; sh_gy[lane] = gy; sh_ps[lane] = ps; sh_rad[lane] = rad;
      sh_frad[lane] = static_cast<float>((1 + 5e-2) * rad);  // RVOPolicy.py:71 (changes with the radius only: load, reset)
      sh_tr[lane] = tr;
      if (MULTI) {  // (the n-step kernel keeps nothing per lane in registers across its loop: parked here, waits included)
        act0 = l_a0; act1 = l_a1; step_num = l_sn; ep_step = l_es; reset_cnt = l_rc;
        sh_t[lane] = l_t; sh_slt[lane] = l_slt; sh_epr[lane] = l_epr; sh_td[lane] = k.s.turning_dir ? l_td : 0.0;
      }
      // cagpu_rollout_ring's rewind point: the state this launch STARTS from, stored -- exactly as it was loaded -- at the same
      // addresses + snap_delta bytes (a second allocation with the layout of the caller's state slab).  Fire-and-forget
      // stores of values that are in registers anyway; replaces a 5 us copy kernel + its launch in front of every ring.
      if (MULTI && k.snap_delta != 0) {
        const long sd = k.snap_delta;
        auto mirror = [sd](auto* ptr) {
          return reinterpret_cast<std::remove_const_t<std::remove_pointer_t<decltype(ptr)>>*>(
              reinterpret_cast<char*>(const_cast<std::remove_const_t<std::remove_pointer_t<decltype(ptr)>>*>(ptr)) + sd);
        };
        if (active) {
          mirror(q_px)[lane] = px; mirror(q_py)[lane] = py; mirror(q_vx)[lane] = vx; mirror(q_vy)[lane] = vy;
          mirror(q_hd)[lane] = heading; mirror(q_gx)[lane] = gx; mirror(q_gy)[lane] = gy; mirror(q_rad)[lane] = rad;
          mirror(q_ps)[lane] = ps; mirror(q_tr)[lane] = tr; mirror(q_t)[lane] = l_t; mirror(q_slt)[lane] = l_slt;
          mirror(q_epr)[lane] = l_epr;
          if (k.s.turning_dir) mirror(q_td)[lane] = l_td;
          mirror(q_la)[lane] = make_float2(l_a0, l_a1);
          mirror(q_fl)[lane] = flags;
          mirror(q_sn)[lane] = l_sn;
          mirror(q_pl)[lane] = pl;   // (the raw plan word: `plan` is only taken from it when its flag is valid)
          if (a == 0) { mirror(q_es)[le] = l_es; mirror(q_rc)[le] = l_rc; }
        }
        {  // env_stats [E, 8]: not loaded otherwise (8 doubles per env of the tile)
          const double* es = k.s.env_stats + env0 * 8;
          const long left = (static_cast<long>(p.num_envs) - env0) * 8;
#pragma unroll
          for (int q = lane; q < TE * 8; q += 64)
            if (q < left) mirror(es)[q] = es[q];
        }
      }
    }
    bool plan_ok = (flags & CA_PLAN_VALID) != 0;
    bool statics_dirty = false;
    float reward = 0.f;
    // the self entries of the sensor tiles (never sensed, no gap: the pair phases only write the rest)
    if (lane < TILE_N) {
      kmat[a * CS + lane] = KEY_NONE;
      omat[a * CS + lane] = 0.0;
      d2mat[a * CS + lane] = 0.f;
      gmat[a * CS + lane] = INFINITY;
    }
    bool need;
    {
      const bool wants = active && !(flags & CA_DONE) && ((flags >> CA_POLICY_SHIFT) & 0xF) == CA_POL_RVO && !plan_ok;
      need = plan_mode || (__ballot(wants) != 0ull);
      if (lane == 0) sh_misc[M_NEED] = need ? 1 : 0;
      if (lane >= 3 && lane < 16) sh_misc[lane] = 0;  // the arrival counters
      if (lane < 32) sh_rc[lane] = 0;  // (envs beyond num_envs never write theirs)
    }
    __builtin_amdgcn_s_setprio(3);
    bool yield_ = false;

    // publish the tile.  pre: the PRE-move state, for the O half only (a tile without a valid plan).
    double eg_dist = 0.0, eg_hego = 0.0;
    auto publish = [&](const bool pre) {
      sh_px[lane] = px; sh_py[lane] = py; sh_head[lane] = heading;
      // (an absent slot of a ragged batch sits at infinity: distSq = inf = "not a neighbour" for everybody)
      sh_fpx[lane] = (ragged && (flags & CA_ABSENT)) ? INFINITY : static_cast<float>(px);
      sh_fpy[lane] = static_cast<float>(py);
      sh_fvx[lane] = static_cast<float>(vx);
      sh_fvy[lane] = static_cast<float>(vy);
      // who is planned for: pre-move, exactly the agents the reference queries (env.py:311: not done); post-move, every
      // agent that can still be "not done" when the next step starts (the collision flag of this step comes later)
      const uint32_t stop = pre ? CA_DONE : (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION);
      const bool q = active && !(flags & stop) && ((flags >> CA_POLICY_SHIFT) & 0xF) == CA_POL_RVO;
      const unsigned long long qm = __ballot(q);
      if (q) sh_q[__popcll(qm & ((1ull << lane) - 1ull))] = lane;
      sh_isq[lane] = q ? 1 : 0;
      if (lane == 0) {
        sh_q3[0] = 0;
        sh_misc[M_NLIVE] = __popcll(qm) | ((FAIR && !pre && yield_) ? 0x100 : 0);
      }
      // the arrival counters start from zero in every pass: nobody is between a sig() and its wait_for() when wave 0
      // publishes (all waves are on their way to the barrier that follows)
      if (lane >= 3 && lane < 16 && lane != M_YIELD && lane != M_PSLOT) sh_misc[lane] = 0;
      if (!pre) { sh_vx[lane] = vx; sh_vy[lane] = vy; }
    };

    PIPE_SYNC();  // B_A: `need`
    int step = 0;
    for (;;) {
      if (MULTI) {  // hide the loop invariance of everything derived from the thread id (see the O programme)
        int lane_l = tid;
        asm volatile("" : "+v"(lane_l));
        lane = lane_l;
        le = div_small<NC>(lane, 0.f); a = lane - le * N;
        active = (lane < TILE_N) && (env0 + le < p.num_envs);
        ebase = active ? le * N : 0;
      }
      if (need) {
        publish(true);
        PIPE_SYNC();  // B_N1
        PIPE_SYNC();  // B_N6 (the O half is through: P2 .. post)
        plan = sh_plan[lane];
        plan_ok = true;
        need = false;
      }
      if (step >= n_steps) break;
      // ================= move: the action of this step (env.py:305-323) and Agent.take_action (agent.py:192-241)
      bool turned = false;  // UnicycleDynamics.step ran for this lane (Agent.turning_dir follows, off the critical path)
      bool moved = false;   // Agent.take_action got past its done gate: the action / step / clock bookkeeping follows below
      float mv_a0 = 0.f, mv_a1 = 0.f;
      {
        // (the parked columns this block reads, fetched before the trigonometry instead of behind it)
        double gx_m = sh_gx[lane], gy_m = sh_gy[lane];
        const double tr_m = sh_tr[lane];
        const uint32_t pol_ = (flags >> CA_POLICY_SHIFT) & 0xF;
        const bool query = active && !(flags & CA_DONE);  // env.py:311
        float a0f = 0.f, a1f = 0.f;
        if (query) {
          if (pol_ == CA_POL_RVO) {  // planned by the O half (RVOPolicy.py:50-122): already the float32 `all_actions` pair
            a0f = plan.x;
            a1f = plan.y;
          } else {
            double spd = 0.0, dh = 0.0;
            if (pol_ == CA_POL_NONCOOP) {  // NonCooperativePolicy.py:21
              const Ego eg = ego_frame(px, py, gx_m, gy_m, heading);
              spd = sh_ps[lane];
              dh = -eg.heading_ego;
            } else if (pol_ == CA_POL_STATIC) {  // StaticPolicy.py:21-23
              sh_gx[lane] = px; sh_gy[lane] = py;
              gx_m = px; gy_m = py;
              statics_dirty = true;
            } else if (k.ext) {
              // (an action tape, cagpu_step_tape: step t of the launch reads slot t -- a kernel argument times the loop counter,
              //  in scalar registers; ext_stride = 0: one slot held for all steps)
              const double* const ex = k.ext + 2 * tile_base + (MULTI ? step * k.ext_stride : 0);
              ext_policy_action(pol_, ex[2 * lane], ex[2 * lane + 1], sh_ps[lane], p.max_heading_change, spd, dh);
            }
            a0f = static_cast<float>(spd);  // float32 `all_actions`
            a1f = static_cast<float>(dh);
          }
        }
        if (active && k.o.actions) (reinterpret_cast<float2*>(k.o.actions) + out_base)[lane] = make_float2(a0f, a1f);
        if (active && k.o.orca_vel)
          (reinterpret_cast<float2*>(k.o.orca_vel) + out_base)[lane] =
              (query && pol_ == CA_POL_RVO) ? make_float2(plan.z, plan.w) : make_float2(0.f, 0.f);
        if (active) {
          if (flags & (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION)) {
            if (flags & CA_AT_GOAL) flags |= CA_WAS_AT_GOAL;
            if (flags & CA_IN_COLLISION) flags |= CA_WAS_IN_COLLISION;
            vx = vy = 0.0;
          } else {
            moved = true;
            mv_a0 = a0f;
            mv_a1 = a1f;
            const double a0 = a0f, a1 = a1f;
            const uint32_t dyn = (flags >> CA_DYNAMICS_SHIFT) & 0xF;
            if (dyn != CA_DYN_EXTERNAL) {
              double nh;
              if (dyn == CA_DYN_MAX_TURN_RATE) {  // UnicycleDynamicsMaxTurnRate.py:31-33
                double trn = a1 / p.dt;
                trn = fmin(fmax(trn, -3.0), 3.0);
                nh = wrap_pi(trn * p.dt + heading);
              } else {
                nh = wrap_pi(a1 + heading);  // UnicycleDynamics.py:28
              }
              double sn, cs;
              sincos_heading(nh, sn, cs);
              px += a0 * cs * p.dt;
              py += a0 * sn * p.dt;
              vx = a0 * cs;
              vy = a0 * sn;
              heading = nh;
              turned = dyn == CA_DYN_UNICYCLE;
            }
            const double qx = px - gx_m, qy = py - gy_m;
            if (qx * qx + qy * qy <= p.near_goal_threshold * p.near_goal_threshold) flags |= CA_AT_GOAL;
            else flags &= ~static_cast<uint32_t>(CA_AT_GOAL);
            const double tr = tr_m - p.dt;
            sh_tr[lane] = tr;
            if (tr <= 0.0) flags |= CA_OUT_OF_TIME;
          }
        }
      }
      publish(false);
      PIPE_SYNC();  // B_P
      PIPE_ONCE(px)
      {  // the ego frame (agent.py:329-349, Dynamics.py:24-41) is the S half's business: the O half is already in P2
        const Ego eg = ego_frame(px, py, sh_gx[lane], sh_gy[lane], heading);
        sh_prx[lane] = eg.prx;
        sh_pry[lane] = eg.pry;
        eg_dist = eg.dist;
        eg_hego = eg.heading_ego;
      }
      sig(&sh_misc[M_CEGO]);
      // ---- while the S-pair waves work on P3: what the launch's first step fetched for the phases from here on, then the
      // bookkeeping of the move (agent.py:212-213, :235-239; env.py:183)
      if (!MULTI && step == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        // (pins the first uses of the late values HERE: the compiler otherwise hoists `l_es + 1` and friends up to the loads
        // and waits for them in front of the move)
        asm volatile("" : "+v"(l_t), "+v"(l_slt), "+v"(l_epr), "+v"(l_td), "+v"(l_a0), "+v"(l_a1), "+v"(l_sn), "+v"(l_es), "+v"(l_rc));
#endif
        if (!k.s.turning_dir) l_td = 0.0;
        act0 = l_a0; act1 = l_a1; step_num = l_sn; ep_step = l_es; reset_cnt = l_rc;
        sh_t[lane] = l_t; sh_slt[lane] = l_slt; sh_epr[lane] = l_epr; sh_td[lane] = l_td;
      }
      ep_step += 1;
      if (TRAJ) {
        // The trajectory row (CaTraj), here because the agent wave waits for P3 below anyway: the clock and the index are
        // still those BEFORE their increments, position / velocity / heading those after the move, the parked goal is the
        // one the move used (StaticPolicy: the position), and no auto-reset of this step has happened yet (A4).
        if (active) {
          double* row = traj_tile + __mul24(lane, 12);
          if (moved) traj_store(row, sh_t[lane], px, py, sh_gx[lane], sh_gy[lane], sh_rad[lane], sh_ps[lane], vx, vy, mv_a0, heading, step_num);
          else row[11] = -1.0;
          if (a == 0 && traj_ep) traj_ep[le] = reset_cnt;
        }
      }
      if (moved) {
        act0 = mv_a0; act1 = mv_a1;
        step_num += 1;
        sh_t[lane] = sh_t[lane] + p.dt;
      }
      // Agent.turning_dir (UnicycleDynamics.py:41-47)
      if (k.s.turning_dir && turned) sh_td[lane] = turning_dir_next(sh_td[lane], heading);
      // a map set (the single-step kernel, and the n-step form's MSET instantiations, which only a set launch selects;
      // uniform test): the env's grid for the wall tests of A3, its index read by the env's agent 0 lane (before the wait,
      // which hides the load) and handed to the others -- in an n-step launch what the same lane stored at the last auto-reset
      const bool wall_set = (!MULTI || MSET) && k.env_map != nullptr;
      const uint32_t* wall_bits = nullptr;
      if (wall_set) {
        int m = (active && a == 0) ? k.env_map[env0 + le] : 0;
        m = __shfl(m, ebase);
        wall_bits = active ? set_grid(k.map.static_bits, k.map_words, k.num_maps, m, a == 0) : nullptr;
      }
      wait_for(&sh_misc[M_CP3], 3);  // P3 done (the three S-pair waves)
      // ================= A3: rewards + collision flag (env.py:394-456), observation scalars
      if (active) {
        double nearest = INFINITY;
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const double g = gmat[j * CS + lane];
          nearest = (g < nearest) ? g : nearest;
        }
        const bool coll = nearest <= 0.0;  // some d <= r_i + r_j  <=>  min(d - (r_i + r_j)) <= 0
        const double rad = sh_rad[lane];
        double rw = p.reward_time_step;
        if (flags & CA_AT_GOAL) {
          if (!(flags & CA_WAS_AT_GOAL)) rw = p.reward_at_goal;
        } else if (!(flags & CA_WAS_IN_COLLISION)) {
          if (coll) {
            rw = p.reward_collision;
            flags |= CA_IN_COLLISION;
          } else if (wall_set ? hits_wall_in(k.map, wall_bits, px, py, rad)
                              : hits_wall(k.map, px, py, rad)) {  // env.py:425-429, :494-506
            rw = p.reward_collision_wall;
            flags |= CA_IN_COLLISION;
          } else {
            if (nearest <= p.getting_close_range) rw = -0.1 - nearest / 2.0;
            if (fabs(static_cast<double>(act1)) > p.wiggly_threshold) rw += p.reward_wiggly;
          }
        }
        rw = fmin(fmax(rw, p.reward_min), p.reward_max);
        const bool here = !(ragged && (flags & CA_ABSENT));
        if (!here) rw = 0.0;  // no agent in this slot: the zero padding of wrappers.py:143-173
        sh_epr[lane] = sh_epr[lane] + rw;
        reward = static_cast<float>(rw);
        const bool d = (flags & (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION)) != 0;
        if (d) flags |= CA_DONE; else flags &= ~static_cast<uint32_t>(CA_DONE);
        sh_flag[lane] = flags;
        sh_r2[lane] = sh_t[lane] - sh_slt[lane];
        float* row = obs_tile + __mul24(lane, W);  // (obs_own_columns of cagpu_rules.inc, in this kernel's own text)
        row[0] = (here && (flags & CA_IS_LEARNING)) ? 1.f : 0.f;
        row[2] = here ? static_cast<float>(eg_dist) : 0.f;
        row[3] = here ? static_cast<float>(eg_hego) : 0.f;
        row[4] = here ? static_cast<float>(sh_ps[lane]) : 0.f;
        row[5] = static_cast<float>(rad);
      }
      // ================= A4: done / game over (env.py:514-553), auto-reset (vec_env.py:120-128), episode statistics
      bool lost_plan = false;
      {
        bool reset_here = false;
        if (active) {
          uint32_t f_and = ~0u, f_or = 0u, learn_and = ~0u;  // (FlagFold of cagpu_rules.inc, in this kernel's own text)
#pragma unroll
          for (int j = 0; j < N; ++j) {
            const uint32_t f = sh_flag[ebase + j];
            f_and &= f;
            f_or |= f;
            learn_and &= (f & CA_STILL_LEARNING) ? f : ~0u;  // learners only
          }
          const bool all_done = (f_and & CA_DONE) != 0, all_learning_done = (learn_and & CA_DONE) != 0;
          const bool any_coll = (f_or & CA_IN_COLLISION) != 0, all_goal = (f_and & CA_AT_GOAL) != 0;
          bool over = all_done;
          if (p.game_over_mode == CA_OVER_AGENT0) over = (sh_flag[ebase] & CA_DONE) != 0;
          else if (p.game_over_mode == CA_OVER_LEARNING_DONE) over = all_learning_done;
          (k.o.rewards + out_base)[lane] = reward;
          (k.o.done + out_base)[lane] = static_cast<uint8_t>((flags & CA_DONE) != 0);
          if (a == 0) (k.o.game_over + out_env)[le] = static_cast<uint8_t>(over);
          int rc = 0;
          if (over && k.table) {
            if (a == 0) {  // experiments/src/env_utils.py:56-87 reduced to counters, summed in agent order
              double tot_r = 0.0, ttg = 0.0, extra = 0.0;
#pragma unroll
              for (int j = 0; j < N; ++j) {
                tot_r += sh_r0[ebase + j];
                ttg += sh_r1[ebase + j];
                extra += sh_r2[ebase + j];
              }
              env_stats_add(k.s.env_stats + 8 * env0 + 8 * le, any_coll, all_goal, ep_step, tot_r, ttg, extra);
            }
            reset_here = true;
          }
          // (every lane of the env has read its env's columns of sh_r0 / sh_r1 before any of them parks its reset values)
          __builtin_amdgcn_wave_barrier();
          if (reset_here) {
            reset_cnt += 1;
            // (reset_case of cagpu_rules.inc, in this kernel's own text)
            const long c = (k.env_id_offset + env0 + le + static_cast<long>(reset_cnt) * k.case_stride) % k.n_cases;
            // final record (CaFinal): the flag word as the terminal step leaves it, in the slot of this step's outputs
            if (FINAL && k.fin_flags) (k.fin_flags + out_base)[lane] = flags;
            // episode log (CaEpLog; a uniform test inside the FINAL instantiations): this lane's three addends and flag
            // word, and -- agent 0 -- the episode's head, in slot (episode index % capacity) of the env's own ring
            if (FINAL && k.log_rows)
              eplog_store(k.log_rows, k.log_head, k.log_cap, env0 + le, static_cast<int>(c), k.log_case_step, k.n_cases, N, a,
                          reset_cnt - 1, sh_epr[lane], sh_t[lane], sh_r2[lane], flags, ep_step, any_coll, all_goal);
            Lane r;
            r.flags = flags;
            reset_lane(r, k.table + (c * N + a) * 6, false, 0.0, p);
            // policy draw (CaPolicyDraw; a uniform test inside the FINAL instantiations): the new episode's policy bits of this
            // slot, every lane recomputing its env's draws; the S-pair's reset copy reads is_learning from sh_flag behind M_CA4
            if (FINAL && k.draw_cdf) {
              const double* rad = k.table + c * N * 6 + 5;
              r.flags = policy_draw_word(k.draw_cdf, k.draw_bits, k.draw_n, k.draw_ensure, k.draw_seed,
                                         k.env_id_offset + env0 + le, reset_cnt, a, N,
                                         [&](const int j) { return !ragged || rad[j * 6] > 0.0; }, r.flags);
              sh_flag[lane] = r.flags;
            }
            // a map set with a key: the env's next map (CaMapSet.map_seed), one plain store by its agent 0 lane
            if ((!MULTI || MSET) && k.map_seed && a == 0) k.env_map[env0 + le] = map_draw(k.map_seed, k.env_id_offset + env0 + le, reset_cnt, k.num_maps);
            px = r.px; py = r.py; vx = r.vx; vy = r.vy; heading = r.heading;
            act0 = r.act0; act1 = r.act1; flags = r.flags; step_num = r.step_num;
            sh_gx[lane] = r.gx; sh_gy[lane] = r.gy; sh_ps[lane] = r.ps; sh_rad[lane] = r.rad;
            sh_frad[lane] = static_cast<float>((1 + 5e-2) * r.rad);
            sh_tr[lane] = r.tr; sh_t[lane] = r.t; sh_slt[lane] = r.slt; sh_epr[lane] = r.epr; sh_td[lane] = r.td;
            ep_step = 0;
            statics_dirty = true;
            rc = static_cast<int>(c) + 1;
          }
          if (a == 0) sh_rc[le] = rc;
        }
        const unsigned long long rm = __ballot(reset_here);
        lost_plan = reset_here && !k.reset_plan;
        const bool need_next = __ballot(lost_plan) != 0ull;
        if (lane == 0) {
          sh_misc[M_AGAIN] = rm != 0ull ? 1 : 0;
          sh_misc[M_NEED] = need_next ? 1 : 0;
        }
        // (the reset-observation copy overwrites rows this wave stored to in A3: they have to be out first)
        if (rm != 0ull) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        need = need_next;
      }
      sig(&sh_misc[M_CA4]);  // done / auto-reset are decided: M_NEED, M_AGAIN, sh_rc, sh_flag (S-pair's reset copy, O's post)
      ++step;
      plan_ok = !lost_plan;
      if (step >= n_steps) break;
      // The n-step loop carries NOTHING per lane in registers across its back edge: the post-move tile is in LDS anyway
      // (publish), the few other scalars are parked beside it and everything is read back after the barrier -- the
      // allocator then sees the single-step programme (55 VGPRs) instead of spilling 130 registers around the loop.
      // (An env that auto-reset in A4 parks its reset state: the O half's post may still read the old or the new
      // position of such a lane -- either way its result is replaced by the case's reset_plan or never used.)
      sh_px[lane] = px; sh_py[lane] = py; sh_vx[lane] = vx; sh_vy[lane] = vy; sh_head[lane] = heading;
      sh_flag[lane] = flags | (statics_dirty ? 0x80000000u : 0u);
      sh_w0[lane] = step_num; sh_w0[ROW + lane] = ep_step; sh_w0[2 * ROW + lane] = reset_cnt;
      sh_w0[3 * ROW + lane] = __float_as_int(act0); sh_w0[4 * ROW + lane] = __float_as_int(act1);
      if (MULTI) {  // (0 unless the caller keeps every step's outputs)
        obs_tile += k.ring_obs;
        out_base += k.ring_agent;
        out_env += k.ring_env;
        if (TRAJ) {  // (the tape's slots advance whether or not the outputs form a ring)
          traj_tile += static_cast<long>(p.num_envs) * N * 12;
          if (traj_ep) traj_ep += p.num_envs;
        }
      }
      __syncthreads();  // B_5: the plan of the next step (n-step kernel only; a FULL barrier: this step's stores are out)
      if (FAIR) {
        yield_ = sh_misc[M_YIELD] != 0;   // (read with the parked values below: one LDS round trip for all of them)
        PIPE_PRIO(3);
      }
      plan = sh_plan[lane];
      px = sh_px[lane]; py = sh_py[lane]; vx = sh_vx[lane]; vy = sh_vy[lane]; heading = sh_head[lane];
      flags = sh_flag[lane];
      statics_dirty = (flags & 0x80000000u) != 0;
      flags &= 0x7FFFFFFFu;
      step_num = sh_w0[lane]; ep_step = sh_w0[ROW + lane]; reset_cnt = sh_w0[2 * ROW + lane];
      act0 = __int_as_float(sh_w0[3 * ROW + lane]); act1 = __int_as_float(sh_w0[4 * ROW + lane]);
    }

    // ---- store my agent (pointers re-read from the kernarg segment: see ca_kernel)
    if (active) {
#if defined(__HIP_DEVICE_COMPILE__)
      RoleKArgs* ka = (RoleKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
      asm volatile("" : "+s"(ka));
#else
      const KArgs* ka = &k;
#endif
      const uint32_t fl = plan_ok ? (flags | CA_PLAN_VALID) : (flags & ~static_cast<uint32_t>(CA_PLAN_VALID));
      if (plan_mode) {
        (ka->s.flags + tile_base)[lane] = fl;
      } else {
        (ka->s.pos_x + tile_base)[lane] = px; (ka->s.pos_y + tile_base)[lane] = py;
        (ka->s.vel_x + tile_base)[lane] = vx; (ka->s.vel_y + tile_base)[lane] = vy;
        (ka->s.heading + tile_base)[lane] = heading;
        (ka->s.time_remaining + tile_base)[lane] = sh_tr[lane]; (ka->s.t + tile_base)[lane] = sh_t[lane];
        (ka->s.ep_reward + tile_base)[lane] = sh_epr[lane];
        if (ka->s.turning_dir) (ka->s.turning_dir + tile_base)[lane] = sh_td[lane];
        if (statics_dirty) {
          (ka->s.goal_x + tile_base)[lane] = sh_gx[lane]; (ka->s.goal_y + tile_base)[lane] = sh_gy[lane];
          (ka->s.radius + tile_base)[lane] = sh_rad[lane]; (ka->s.pref_speed + tile_base)[lane] = sh_ps[lane];
          (ka->s.slt + tile_base)[lane] = sh_slt[lane];
        }
        (reinterpret_cast<float2*>(ka->s.last_action) + tile_base)[lane] = make_float2(act0, act1);
        (ka->s.flags + tile_base)[lane] = fl;
        (ka->s.step_num + tile_base)[lane] = step_num;
        if (a == 0) { (ka->s.episode_step + env0)[le] = ep_step; (ka->s.reset_count + env0)[le] = reset_cnt; }
      }
    }
  } else if (role < 4) {
    // =====================================================================================================================
    // waves 1 - 3: the S-pair programme
    PIPE_ROLE_KARGS();
    float* obs_tile = k.o.obs + tile_base * W;
    // agents of this tile that exist (the last tile of a batch may hold fewer than TE envs): nothing is stored for the rest
    const int tile_cnt = (static_cast<long>(p.num_envs) * N - tile_base < TILE_N)
                             ? static_cast<int>(static_cast<long>(p.num_envs) * N - tile_base) : TILE_N;
    __builtin_amdgcn_s_setprio(S_PRIO);
    PIPE_SYNC();  // B_A
    if (FAIR && tid == 64) {  // my slot in my CU's row of the progress table (read back every step: nothing carried in registers)
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      const unsigned at = (((xcc & 0xF) << 8) | ((hw >> 8) & 0xFF));
      sh_misc[M_PSLOT] = static_cast<int>(at * 4 + (atomicAdd(&g_cu_slot[at], 1u) & 3u));
    }
    bool need = sh_misc[M_NEED] != 0;
    int step = 0;
    for (;;) {
      if (need) {
        PIPE_SYNC();  // B_N1
        PIPE_SYNC();  // B_N6
        need = false;
      }
      if (step >= n_steps) break;
      int ts_l = tid - 64;  // 0 .. 191 (laundered per step: see the O programme)
      asm volatile("" : "+v"(ts_l));
      const int ts = ts_l;
      PIPE_SYNC();  // B_P
      const int nl_word = __builtin_amdgcn_readfirstlane(sh_misc[M_NLIVE]);
      const bool yield_ = PIPE_YIELD_OF(nl_word);
      if (FAIR) PIPE_PRIO(S_PRIO);
      // (FAIR: the CU-mates' progress words, fetched here -- a device-scope load, ~2 us under load -- and looked at at the end
      // of the step)
      unsigned prog_seen = 0;
      if (FAIR && ts < 64)
        prog_seen = __hip_atomic_load(&g_prog[(static_cast<unsigned>(sh_misc[M_PSLOT]) & ~3u) + (ts & 3)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // ---- P2 helper: a tile with more planned agents than the four O waves hold in one round (28 of 40) hands the next
      // two waves' worth to the first two of these waves, which would otherwise wait for wave 0's ego frames now
      {
        const int n_live = PIPE_NLIVE(nl_word);
        const int hw = __builtin_amdgcn_readfirstlane(ts >> 6);
        if (n_live > P2_APR && hw < P2_HELPERS) {
          PIPE_PRIO(O_PRIO);  // (the O half waits for these half-planes)
          const float range_sq = sqf(static_cast<float>(p.sensing_horizon));
          int wl = ts & 63;
          PIPE_ONCE(wl)
          // (1 / time horizon, 1 / rvo_dt: the correctly rounded float quotients, divided once on the host -- KArgs.inv_h_f /
          // inv_dt_f -- instead of two IEEE divisions per helper wave and step)
          p2_round(0, 4 + hw, wl, n_live, !(range_sq < INFINITY), range_sq, p.rvo_max_neighbors,
                   static_cast<float>(p.rvo_collab_coeff), k.inv_h_f, k.inv_dt_f);
          sig(&sh_misc[M_CP2]);
          PIPE_PRIO(S_PRIO);
        }
      }
      wait_for(&sh_misc[M_CEGO], 1);  // wave 0's ego frames
      // ================= P3: every UNORDERED pair {a, b} of an env: centre distance -> collision gap, sensor key, p_orth
      // (env.py:458-512; OtherAgentsStatesSensor.py:76-107).  The float64 square root and the horizon test are the same
      // for both directions; d - r_host - r_other (operand order) and p_orth (the host's frame) are direction-specific.
      // Per env: the pairs (a, a + s mod N), s = 1 .. (N-1)/2, and for even N the N/2 antipodal pairs: N (N - 1) / 2.
      {
        constexpr int HALF = (N - 1) / 2, PE = N * (N - 1) / 2;
        constexpr int n_un = TE * PE;
        int ts2 = ts;
        PIPE_ONCE(ts2)
#pragma unroll
        for (int base_ = 0; base_ < n_un; base_ += S_PAIR) {
          const int w = base_ + ts2;
          if (w >= n_un) continue;
          const int le2 = div_small<PE>(w, 0.f);
          const int u = w - __mul24(le2, PE), eb = __mul24(le2, N);
          int a1, b1;
          if (u < N * HALF) {
            const int sft = div_small<N>(u, 0.f);
            a1 = u - __mul24(sft, N);
            b1 = a1 + sft + 1;
            b1 -= (b1 >= N) ? N : 0;
          } else {
            a1 = u - N * HALF;
            b1 = a1 + N / 2;
          }
          const int ga = eb + a1, gb = eb + b1;
          const double ax = sh_px[ga], ay = sh_py[ga], ar = sh_rad[ga];
          const double bx = sh_px[gb], by = sh_py[gb], br = sh_rad[gb];
          const double rx = bx - ax, ry = by - ay;  // other - host for host a; exactly negated for host b
          const double d = sqrtd(rx * rx + ry * ry);
          int key_ab = KEY_NONE, key_ba = KEY_NONE;
          double po_ab = 0.0, po_ba = 0.0, d2_ab = 0.0, d2_ba = 0.0;
          const bool both = !ragged || (ar > 0.0 && br > 0.0);  // (an absent slot of a ragged batch has radius 0)
          // p_prll of the other agent in the host's frame (the row's first entry, sensor :119-121): the expressions of the
          // emission phase, evaluated here where rx / ry are at hand (b's view: other - host = -(rx, ry), exactly)
          const double prx_a = sh_prx[ga], pry_a = sh_pry[ga], prx_b = sh_prx[gb], pry_b = sh_pry[gb];
          pmat[b1 * CS + ga] = rx * prx_a + ry * pry_a;
          pmat[a1 * CS + gb] = (-rx) * prx_b + (-ry) * pry_b;
          if (both && !(d > p.sensing_horizon)) {
            d2_ab = d - ar - br;
            d2_ba = d - br - ar;
            // numpy scalar round(x, 2) bucket; ordering of k == ordering of k/100 (an integer: exact as int32)
            key_ab = static_cast<int>(fmin(fmax(rint(d2_ab * 100.0), -2.0e9), 2.0e9));
            key_ba = static_cast<int>(fmin(fmax(rint(d2_ba * 100.0), -2.0e9), 2.0e9));
            po_ab = rx * (-pry_a) + ry * prx_a;
            po_ba = (-rx) * (-pry_b) + (-ry) * prx_b;
          }
          kmat[b1 * CS + ga] = key_ab;
          omat[b1 * CS + ga] = po_ab;
          d2mat[b1 * CS + ga] = static_cast<float>(d2_ab);
          gmat[b1 * CS + ga] = both ? d - (ar + br) : INFINITY;
          kmat[a1 * CS + gb] = key_ba;
          omat[a1 * CS + gb] = po_ba;
          d2mat[a1 * CS + gb] = static_cast<float>(d2_ba);
          gmat[a1 * CS + gb] = both ? d - (br + ar) : INFINITY;
        }
      }
      sig(&sh_misc[M_CP3]);
      // ---- P2b helper: items 256 .. 383 of a tile whose 1-D programmes do not fit one round of the four O waves
      {
        const int n_live = PIPE_NLIVE(nl_word);
        const int hw = __builtin_amdgcn_readfirstlane(ts >> 6);
        if (n_live * (N - 1) > O_LANES && hw < P2_HELPERS) {
          PIPE_PRIO(O_PRIO);
          wait_for(&sh_misc[M_CP2], 4 + ((n_live > P2_APR) ? P2_HELPERS : 0));  // every half-plane, the preferred velocities
          p2b_round(O_LANES, (hw << 6) + (ts & 63), n_live, kMagic20.v[n_live]);
          sig(&sh_misc[M_CP2B]);
          PIPE_PRIO(S_PRIO);
        }
      }
      wait_for(&sh_misc[M_CP3], 3);
      // ================= P4: rank the candidates of every agent and emit its rows (OtherAgentsStatesSensor.py:20-55,
      // 109-143): one item per (agent, other), N - 1 lanes per agent
      PIPE_PRIO(S_PRIO4);
      {
        constexpr int n_p4 = TILE_N * GN;
        int ts2 = ts;
        PIPE_ONCE(ts2)
#pragma unroll
        for (int base_ = 0; base_ < n_p4; base_ += S_PAIR) {
          const int w = base_ + ts2;
          if (w >= n_p4) continue;
          const int ag = div_small<GN>(w, 0.f);
          if (ag >= tile_cnt) continue;
          const int jo = w - __mul24(ag, GN);
          const int eb = __mul24(div_small<N>(ag, 0.f), N), aa = ag - eb;
          const int j = jo + ((jo >= aa) ? 1 : 0);
          const int kj = kmat[j * CS + ag];
          const double oj = omat[j * CS + ag];
          // Pass 1 ranks by the distance bucket alone; the (p_orth, index) tie-break runs as a second pass in the waves
          // that hold a row with two candidates in one 1 cm bucket (see ca_kernel)
          int rank = 0, cnt = N - 1;
          int kq[N];
#pragma unroll
          for (int q = 0; q < N; ++q) {
            kq[q] = kmat[q * CS + ag];
            rank += static_cast<int>(kq[q] < kj);
          }
          // the (p_orth, index) tie-break, candidate by candidate: only where some lane of the wave shares its 1 cm
          // bucket with candidate q are the float64 p_orth values fetched and compared (two lanes of a tied row meet in two
          // of the N iterations; a pass over all N for every wave that holds a tie was a third of this phase)
#pragma unroll
          for (int q = 0; q < N; ++q) {
            const bool tq = (kq[q] == kj) && (q != j);
            if (__any(tq)) {
              const double oq = omat[q * CS + ag];
              rank += static_cast<int>(tq) & (static_cast<int>(oq < oj) | (static_cast<int>(oq == oj) & static_cast<int>(q < j)));
            }
          }
          if (p.sensing_horizon < INFINITY || ragged) {
            cnt = 0;
#pragma unroll
            for (int q = 0; q < N; ++q) cnt += static_cast<int>(kq[q] != KEY_NONE);
          }
          const int keep = cnt < p.obs_clip ? cnt : p.obs_clip;  // sensor :39
          float* row = obs_tile + __mul24(ag, W);
          if (jo == 0) row[1] = static_cast<float>(keep);  // num_other_agents_observed
          for (int sl = jo; sl < K; sl += GN)              // zero the unfilled rows (sensor :112)
            if (sl >= keep) {
              float* z = row + 6 + 7 * sl;
              z[0] = z[1] = z[2] = z[3] = z[4] = z[5] = z[6] = 0.f;
            }
          if (!((kj != KEY_NONE) && (rank < keep))) continue;
          const double hr = sh_rad[ag], prx = sh_prx[ag], pry = sh_pry[ag];
          const double orad = sh_rad[eb + j];
          const double ovx = sh_vx[eb + j], ovy = sh_vy[eb + j];
          float* o7 = row + 6 + 7 * rank;
          o7[0] = static_cast<float>(pmat[j * CS + ag]);  // p_prll, p_orth: computed with the pair's distance (P3)
          o7[1] = static_cast<float>(oj);
          o7[2] = static_cast<float>(ovx * prx + ovy * pry);
          o7[3] = static_cast<float>(ovx * (-pry) + ovy * prx);
          o7[4] = static_cast<float>(orad);
          o7[5] = static_cast<float>(hr + orad);
          o7[6] = d2mat[j * CS + ag];
        }
      }
      PIPE_PRIO(S_PRIO);
      wait_for<NC_SLEEP>(&sh_misc[M_CA4], 1);  // wave 0's A4: who is done, which envs reset
      need = sh_misc[M_NEED] != 0;
      if (sh_misc[M_AGAIN]) {
        // ---- the observation of a freshly reset env is a pure function of its fixture case: computed once (cagpu_reset
        // on the whole table), copied here over rows P4 (these waves) and A3 (wave 0, drained before its sig()) stored: every
        // earlier store of the workgroup to them has to be out before the copy's
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        sig(&sh_misc[M_CRC]);  // (the P4 rows of all three waves)
        wait_for(&sh_misc[M_CRC], 3);
        for (int le2 = 0; le2 < TE; ++le2) {  // workgroup-uniform: at most a few envs of a tile reset per step
          const int c1 = sh_rc[le2];
          if (!c1) continue;
          const float* src = k.reset_obs + static_cast<long>(c1 - 1) * N * W;
          float* dst = obs_tile + le2 * N * W;
          // final record (CaFinal): the terminal rows are complete in the output block by now (the fences above: P4 of the
          // three waves, A3 of wave 0) -- every lane saves the elements it is about to overwrite, in the block that advances
          // with the output ring
          // (k.fin_obs == nullptr inside a FINAL instantiation: the episode log alone is on)
          float* fin = (FINAL && k.fin_obs) ? k.fin_obs + (dst - k.o.obs) : nullptr;
          for (int q = ts; q < N * W; q += S_PAIR) {
            const int a2 = q / W, col = q - a2 * W;
            if (FINAL && fin) fin[q] = dst[q];
            float v = src[q];
            if (col == 0)  // (is_learning comes from the live flags; the row of an absent slot is all zeros: radius 0)
              v = ((sh_flag[le2 * N + a2] & CA_IS_LEARNING) && !(ragged && !(src[q + 5] > 0.f))) ? 1.f : 0.f;
            dst[q] = v;
          }
        }
      }
      // linearProgram3: the four O waves solve queue entries 0 - 3 (+ 7 k); these three waves, idle by now, take entries
      // 4 - 6 (+ 7 k), so that a tile with up to seven infeasible agents (the slowest tiles of a launch) needs ONE round
      wait_for<NC_SLEEP>(&sh_misc[M_CSCAN], 1);  // the O half's scan: the queue is complete
      const int n3s = sh_q3[0];
      if (n3s > 4) {
        PIPE_PRIO(3);
        const int wv = __builtin_amdgcn_readfirstlane(ts >> 6);
        for (int q3 = 4 + wv; q3 < n3s; q3 += 7) {
          const int ent = sh_q3[1 + q3], agf = ent & 0xFF, ff = (ent >> 8) & 0xFF;
          F2 v = f2(sh_vrx[agf], sh_vry[agf]);
          lp3_wave8(Lmat + agf, CS, (ent >> 16) & 0xFF, ff, sh_fms[agf], v, ts & 63);
          if ((ts & 63) == 0) { sh_vrx[agf] = v.x; sh_vry[agf] = v.y; }
          sig(&sh_misc[M_CLP3]);
        }
        PIPE_PRIO(S_PRIO);
      }
      if (FAIR && ts < 64) {  // the progress exchange with the CU's other workgroups (see PIPE_PRIO above)
        const unsigned ps = static_cast<unsigned>(sh_misc[M_PSLOT]);
        const unsigned seen = prog_seen;
        const unsigned seq = static_cast<unsigned>(k.launch_seq) & 0xFFFFu;
        const unsigned mine = static_cast<unsigned>(step) & 0xFFFFu;
        const unsigned sv = ((seen >> 16) == seq && (ts & 3) != static_cast<int>(ps & 3u) && ts < 4) ? (seen & 0xFFFFu) : 0xFFFFu;
        unsigned m = mine + 1u;   // (completed steps, this one included; the others' counts are theirs as of the middle of this step)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned o = __builtin_amdgcn_readlane(sv, q);
          m = o < m ? o : m;
        }
        if (ts == 0) {
          sh_misc[M_YIELD] = (mine + 1u - m >= static_cast<unsigned>(k.yield_t)) ? 1 : 0;
          __hip_atomic_store(&g_prog[ps], (seq << 16) | ((mine + 1u) & 0xFFFFu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      if (ts < 64) {  // the audit of the arrival counters (see sig() / wait_for()), on a wave nobody waits for any more:
        // behind the scan's signal every counter but M_CLP3 (whose only waiter, wave 4, polls it right now) and M_CRC
        // (this wave's own) is final and must hold exactly its target
        const int n_live = PIPE_NLIVE(nl_word);
        const int slot = ts & 15;
        const int want = (slot == M_CEGO) ? 1 : (slot == M_CP3) ? 3 : (slot == M_CP2) ? 4 + ((n_live > P2_APR) ? P2_HELPERS : 0)
                       : (slot == M_CP2B) ? 4 + ((n_live * (N - 1) > O_LANES) ? P2_HELPERS : 0) : (slot == M_CSCAN) ? 1
                       : (slot == M_CA4) ? 1 : -1;
        const bool off = ts < 16 && want >= 0 && sh_misc[slot] != want;
        if (__ballot(off) != 0ull && ts == 0) atomicOr(&g_fault, 1u);
      }
      ++step;
      if (step >= n_steps) break;
      if (MULTI) obs_tile += k.ring_obs;  // (the next step's slot of the caller's output ring; 0 without one)
      __syncthreads();  // B_5
    }
  } else {
    // =====================================================================================================================
    // waves 4 - 7: the O programme (ORCA of the published tile -> the plan of the next step).  Wave 4 is its agent wave.
    PIPE_ROLE_KARGS();
    const bool w4 = role == 4;
    const float range_sq = sqf(static_cast<float>(p.sensing_horizon));
    const bool unlimited = !(range_sq < INFINITY);
    const float inv_h = k.inv_h_f;    // 1.0f / float(p.rvo_time_horizon), correctly rounded on the host (launch_pipe2)
    const float inv_dt = k.inv_dt_f;  // 1.0f / float(p.rvo_dt): RVOPolicy.py:13,26
    const float collab = static_cast<float>(p.rvo_collab_coeff);
    PIPE_SYNC();  // B_A
    bool need = sh_misc[M_NEED] != 0;
    int step = 0;

    // publish barrier -> P2 | (O waves) | P2b | B | scan | B | [lp3 | B] | post
    auto orca_half = [&](const bool pre, const bool last) {
      // (everything derived from the thread id is re-derived per call from a laundered copy: otherwise LICM hoists dozens
      // of per-thread addresses / predicates out of the programme's loop and the allocator spills them -- see ca_kernel)
      int to_l = tid - 256;  // 0 .. 255
      asm volatile("" : "+v"(to_l));
      const int to = to_l;
      const int lane = to & 63;  // (agent index on wave 4)
      const int nl_word = __builtin_amdgcn_readfirstlane(sh_misc[M_NLIVE]);
      const bool yield_ = !pre && PIPE_YIELD_OF(nl_word);
      if (w4) PIPE_PRIO(3); else PIPE_PRIO(O_PRIO);
      // ================= P2: every (planned agent, other) pair: neighbour rank (ascending distSq, ties by index:
      // Agent::insertAgentNeighbor) + ORCA half-plane.  A wave holds WHOLE agents, lane = (agent, one of its N - 1 others).
      const int n_live = PIPE_NLIVE(nl_word);
      const unsigned magic = kMagic20.v[n_live];   // (a scalar load, issued here, first used in P2b)
      const bool isq = w4 && sh_isq[lane] != 0;
      // (steady state, more planned agents than the four O waves hold in one round: two S-pair waves take the next two
      // waves' worth beside them -- see the S-pair programme; 83 % of a launch's last-finishing tiles had a second round)
      const int helpers = (!pre && n_live > P2_APR) ? P2_HELPERS : 0;
      {
        const int wv = to >> 6;
        int wl = to & 63;
        PIPE_ONCE(wl) {
          p2_round(0, wv, wl, n_live, unlimited, range_sq, p.rvo_max_neighbors, collab, inv_h, inv_dt);
          for (int c0 = (4 + helpers) * P2_APW; c0 < n_live; c0 += P2_APR)  // uniform
            p2_round(c0, wv, wl, n_live, unlimited, range_sq, p.rvo_max_neighbors, collab, inv_h, inv_dt);
        }
        if (isq) {  // the preferred velocity (float64 sqrt + divide), while the other waves finish the pairs
          const double vx = sh_gx[lane] - sh_px[lane], vy = sh_gy[lane] - sh_py[lane];
          const double ps = sh_ps[lane];
          const double sc = divd(ps, sqrtd(vx * vx + vy * vy));  // RVOPolicy.py:66-67
          const F2 opt = f2(static_cast<float>(sc * vx), static_cast<float>(sc * vy));
          const float radius = static_cast<float>(ps);
          sh_fprx[lane] = opt.x;
          sh_fpry[lane] = opt.y;
          sh_fms[lane] = radius;
          // linearProgram2's starting point (the preferred velocity inside the speed disc), here instead of at the head of
          // the scan: this wave waits for the other waves' half-planes now anyway
          F2 res0 = opt;
          if (dotf(opt, opt) > sqf(radius)) res0 = radius * unitq(opt);
          sh_vrx[lane] = res0.x;
          sh_vry[lane] = res0.y;
        }
      }
      sig(&sh_misc[M_CP2]);
      wait_for(&sh_misc[M_CP2], 4 + helpers);  // the half-planes of all four O waves (and the helpers)
      // ================= P2b: every line's 1-D programme (p2b_round above).  Steady state, more items than one round of the
      // four O waves holds (256 of up to 360): the next two waves' worth goes to the S-pair helpers (between their P3 and P4)
      const int n_lp1 = n_live * (N - 1);
      const int helpers_b = (!pre && n_lp1 > O_LANES) ? P2_HELPERS : 0;
      {
        int to2 = to;
        PIPE_ONCE(to2) {
          p2b_round(0, to2, n_live, magic);
          for (int base_ = O_LANES + 64 * helpers_b; base_ < n_lp1; base_ += O_LANES) p2b_round(base_, to2, n_live, magic);  // uniform
        }
      }
      sig(&sh_misc[M_CP2B]);
      if (w4) wait_for(&sh_misc[M_CP2B], 4 + helpers_b);  // every line's 1-D programme (the scan runs on wave 4 alone)
      // ================= linearProgram2 = a scan over the lines, one lane per agent (wave 4); infeasible programmes are
      // queued for linearProgram3
      int failf = NOFAIL;
      F2 v_orca = f2(0.f, 0.f);
      if (isq) {
        const int n = sh_nb[lane];
        F2 res = f2(sh_vrx[lane], sh_vry[lane]);  // (the clipped preferred velocity: see P2)
#pragma unroll
        for (int i = 0; i < N - 1; ++i) {
          const float4 li = Lmat[i * CS + lane];
          const float2 ri = Rmat[i * CS + lane];
          const int oki = okmat[i * CS + lane];
          const float dt = detf(f2(li.z, li.w), f2(li.x, li.y) - res);
          const int hit = static_cast<int>(i < n) & static_cast<int>(failf == NOFAIL) & static_cast<int>(dt > 0.0f);
          const int take = hit & (oki != 0 ? 1 : 0);
          res.x = take ? ri.x : res.x;
          res.y = take ? ri.y : res.y;
          failf = (hit & (take ^ 1)) ? i : failf;
        }
        v_orca = res;
        if (failf != NOFAIL) {
          sh_vrx[lane] = res.x;
          sh_vry[lane] = res.y;
          sh_q3[1 + atomicAdd(&sh_q3[0], 1)] = lane | (failf << 8) | (n << 16);
        }
      }
      if (w4) sig(&sh_misc[M_CSCAN]);
      else wait_for<NC_SLEEP>(&sh_misc[M_CSCAN], 1);  // the linearProgram3 queue is complete (wave 4 wrote it itself)
      const int n3 = sh_q3[0];
      // ================= linearProgram3 for the queued agents: one WAVE per agent (lp3_wave8, cagpu_grouplp.inc)
      if (n3 > 0) {
        PIPE_PRIO(3);
        const int wv = __builtin_amdgcn_readfirstlane(to >> 6);
        // (in the steady-state step the S-pair waves take the entries q with q % 7 >= 4; in the pre-move pass of a tile
        // without a plan those waves only pass barriers and the O waves take every entry)
        for (int q3 = wv; q3 < n3; q3 += (pre ? 4 : 7)) {
          const int ent = sh_q3[1 + q3], agf = ent & 0xFF, ff = (ent >> 8) & 0xFF;  // (bits 16 ..: the line count)
          F2 v = f2(sh_vrx[agf], sh_vry[agf]);
          lp3_wave8(Lmat + agf, CS, (ent >> 16) & 0xFF, ff, sh_fms[agf], v, to & 63);
          if ((to & 63) == 0) { sh_vrx[agf] = v.x; sh_vry[agf] = v.y; }
          sig(&sh_misc[M_CLP3]);
        }
      }
      // every queue entry is solved (wave 4 only: by these waves and the S-pair waves), and what wave 0's A4 decided in the
      // meantime (steady state only): envs that auto-reset, tiles that lost their plan -- polled together
      if (w4) wait_for2(&sh_misc[M_CLP3], n3, &sh_misc[M_CA4], pre ? 0 : 1);
      else wait_for2<NC_SLEEP>(&sh_misc[M_CLP3], 0, &sh_misc[M_CA4], pre ? 0 : 1);
      if (n3 > 0 && failf != NOFAIL) v_orca = f2(sh_vrx[lane], sh_vry[lane]);
      const bool need_next = !pre && sh_misc[M_NEED] != 0;
      // ================= post: Agent::update + RVOPolicy.py:96-111 -> the float32 action pair of the next step
      if (w4) {
        float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
        PIPE_ONCE(v_orca.x)
        if (isq) {
          // (rvo_action of cagpu_rules.inc, in this kernel's own text: the call changes its instructions)
          const float tsf = static_cast<float>(p.rvo_dt);
          const double px = sh_px[lane], py = sh_py[lane];
          const float npx = sh_fpx[lane] + v_orca.x * tsf, npy = sh_fpy[lane] + v_orca.y * tsf;
          const double dpx = static_cast<double>(npx) - px, dpy = static_cast<double>(npy) - py;
          const double ang = atan2(dpy, dpx);
          const double nh = (ang < 0.0) ? ang + kTwoPi : ((ang == 0.0) ? 0.0 : ang);  // `% (2*pi)`, :102
          double dh = wrap_pi(nh - sh_head[lane]);
          double spd = k.inv_rvo_dt * sqrtd(dpx * dpx + dpy * dpy);  // RVOPolicy.py:106: 1/self.dt * norm
          if (fabs(dh) > kPi / 6) {
            dh = ((dh > 0.0) - (dh < 0.0)) * (kPi / 6);
            spd = 0.0;
          }
          pl = make_float4(static_cast<float>(spd), static_cast<float>(dh), v_orca.x, v_orca.y);
        }
        const int le = div_small<NC>(lane, 0.f), a = lane - le * N;
        const bool active = (lane < TILE_N) && (env0 + le < p.num_envs);
        if (!pre && active && k.reset_plan) {  // an env that auto-reset in this step starts from its case's plan
          const int c1 = sh_rc[le];
          if (c1) pl = reinterpret_cast<const float4*>(k.reset_plan)[static_cast<long>(c1 - 1) * N + a];
        }
        sh_plan[lane] = pl;
        // (an env that lost its plan -- auto-reset without reset_plan -- stores a stale row: wave 0 clears CA_PLAN_VALID)
        if (last && active) (reinterpret_cast<float4*>(k.s.next_action) + tile_base)[lane] = pl;
      }
      return need_next;
    };

    for (;;) {  // (one call site: the half is inlined once)
      const bool pre = need;
      if (!pre && step >= n_steps) break;
      PIPE_SYNC();  // B_N1 / B_P
      const bool need_next = orca_half(pre, pre ? plan_mode : (step + 1 >= n_steps));
      if (pre) {
        PIPE_SYNC();  // B_N6
        need = false;
      } else {
        need = need_next;
        ++step;
        if (step >= n_steps) break;
        __syncthreads();  // B_5
      }
    }
  }
}

}  // namespace pipe
