// gym_collision_avoidance_amd/csrc/cagpu.hip -- the MI355X (gfx950 / CDNA4) hot path behind include/cagpu.h.
//
// One fused kernel advances every env by one (or n) simulation step(s):
//   policy (ORCA / non-coop / static / external)  -> RVOPolicy.py:50-122 + rvo2, NonCooperativePolicy.py:21, ...
//   move (unicycle integration, ego frame)        -> agent.py:192-241, UnicycleDynamics.py:14-47, Dynamics.py:24-41
//   all-pairs collision + nearest distance        -> collision_avoidance_env.py:458-512
//   rewards                                       -> collision_avoidance_env.py:394-456
//   ego-centric sorted other-agent observation    -> OtherAgentsStatesSensor.py:58-144
//   done / game over / fixture auto-reset + stats -> collision_avoidance_env.py:514-553, vec_env.py:120-128
//
// Mapping (wave64, no MFMA: this is branchy element-wise geometry): one WORKGROUP per tile of WHOLE
// envs (floor(64 / num_agents) envs = up to 64 agents; 4 envs at the benchmark's 10 agents), so every neighbour an
// agent needs is owned by the same workgroup and travels through LDS, never through HBM:
//   * HBM loads/stores are agent-major SoA -> lane i touches element base+i: fully coalesced;
//   * serial per-agent chains (the scan of the linear programme, float64 trig, rewards, flags) run one LANE per agent
//     on wave 0, the tile's "agent wave";
//   * the O(N^2) pairwise work (ORCA half-planes, the 1-D programmes of the linear programme, collision gaps, sensor
//     keys / ranks / rows) runs one THREAD per (agent, other) -- or per (agent, line), or per unordered pair -- across
//     all waves, reading the tile's positions / velocities / radii from LDS; where a wave holds whole agents the lanes
//     of an agent exchange through ds_bpermute / DPP instead;
//   * per-(agent, slot) work arrays live in LDS as [slot][agent] columns -> bank-conflict free;
//   * the observation rows go straight to HBM (or, for small launches, are staged in LDS and leave as one block).
// A workgroup's step is a chain of dependent phases; the launch is latency-bound, not bandwidth-bound (DESIGN.md
// section 4, profiles/r02_kernel_geometry.md): wave priorities, few barriers and short chains are what matter.
// Envs never interact, so n-step rollouts need no grid-wide synchronisation.
//
// Numerics: float64 state in the reference's operation order, the action pair rounded to float32
// (env.py:305-307), ORCA in float with the RVO2 operation order.  Built with -ffp-contract=off: a
// fused multiply-add in `dx*dx + dy*dy <= r*r` would change discrete events.
//
// This file is the one translation unit and holds the device code; the host half is included at its end:
// cagpu_launch.inc (which kernel and geometry a call runs, the checked launch) and cagpu_api.inc (the extern "C" entries).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <type_traits>

#include "cagpu.h"

namespace {

constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 2.0 * kPi;
#include "cagpu_lp1.inc"  // kRvoEps + the interval rule of linearProgram1 (host and device)

enum { MODE_STEP = 0, MODE_RESET = 1, MODE_OBSERVE = 2 };

struct KArgs {
  CaParams p;
  CaState s;
  CaOut o;
  const double* ext;
  // auto reset
  const double* table;
  int32_t n_cases;
  int64_t env_id_offset, case_stride;
  const float* reset_obs;  // [n_cases, N, W] reset observation of every case (nullptr: re-sense after an auto-reset)
  const float* reset_plan; // [n_cases, N, 4] next_action of every case's reset state (pipelined kernel only)
  unsigned long long heading_seed;  // != 0: random initial headings at an auto-reset (training mode)
  // explicit reset
  const double* reset_cases;
  const double* reset_headings;
  const uint8_t* reset_mask;
  CaMap map;  // static obstacles for wall collisions (static_bits == NULL: none)
  int32_t n_steps, mode, stage_obs;
  int32_t tile_envs;  // envs per workgroup (<= ROW / num_agents)
  int32_t col_stride; // columns of the per-(agent, slot) LDS tiles: ROW, or N for single-env tiles (N > 32)
  double inv_rvo_dt;  // 1 / p.rvo_dt (RVOPolicy.py:106), divided once on the host
  // cagpu_rollout_ring: step t of the launch writes its outputs to slot t of the caller's ring -- element strides between
  // the slots of the observation block (E N W), of the per-agent outputs (E N; x 2 for the action pairs) and of game_over (E);
  // all 0 everywhere else (every step writes the same buffers)
  int64_t ring_obs, ring_agent, ring_env;
  // cagpu_rollout_ring: != 0: the pipelined n-step kernel also stores the state it starts from at (address + snap_delta)
  int64_t snap_delta;
  int32_t reserved0;  // always 0, read by nobody: keeps the kernarg offsets of the members after it
  int32_t launch_seq;  // a per-process launch counter: tags the words of the n-step kernel's per-CU progress table (cagpu_pipe.inc)
  float inv_h_f, inv_dt_f;  // pipelined kernels: 1.0f / float(p.rvo_time_horizon), 1.0f / float(p.rvo_dt) -- IEEE float quotients, set by launch_pipe2
  int32_t yield_t;     // > 0: progress-fair priorities among the workgroups of a CU (PIPE_PRIO in cagpu_pipe.inc); set by launch_pipe2
  // map set (cagpu_step_maps; env_map == nullptr everywhere else): env e's grid is map.static_bits + env_map[e] * map_words.
  // Only the single-step kernels read these (the n-step instantiations compile the set code out).
  int32_t* env_map;
  int64_t map_words;         // rows * words per row: one map of the set
  int32_t num_maps;
  unsigned long long map_seed;  // != 0: an auto-reset draws the env's next map (CaMapSet.map_seed)
  // trajectory tape (cagpu_step_traj / cagpu_rollout_traj; nullptr everywhere else): slot 0 of CaTraj.rows [n, E, N, 12] and
  // of CaTraj.episode [n, E].  Step t of a launch writes slot t whether or not the outputs form a ring: the slot strides
  // are E N 12 doubles / E ints (the kernels derive them from p).
  double* traj_rows;
  int32_t* traj_ep;
  // final record (cagpu_step_final / cagpu_rollout_final; nullptr everywhere else): block 0 of CaFinal.obs / CaFinal.flags.
  // The blocks advance with the output ring (ring_obs / ring_agent: 0 unless every step keeps its outputs).
  float* fin_obs;
  uint32_t* fin_flags;
  // episode log (cagpu_step_log / cagpu_rollout_log; nullptr everywhere else): CaEpLog.rows [E, C, N, 4] / CaEpLog.head
  // [E, C, 4] and the capacity C.  The blocks never advance: a record's slot is a function of (env, episode index) alone.
  double* log_rows;
  int32_t* log_head;
  int32_t log_cap;
  int32_t log_case_step;  // case_stride mod n_cases in [0, n_cases): the case an episode ran on from the next one's, no division
  // policy draw (cagpu_step_draw; nullptr everywhere else): the members of CaPolicyDraw.  Appended: every older member keeps
  // its kernarg offset
  const double* draw_cdf;
  const uint32_t* draw_bits;
  unsigned long long draw_seed;
  int32_t draw_n, draw_ensure;
  // action tape (cagpu_step_tape; 0 everywhere else): doubles from the slot `ext` names to the slot of the next step.  Step t of
  // an n-step launch reads ext + t * ext_stride (a kernel argument times the loop counter: scalar registers); where a rollout
  // is n launches the host advances `ext` itself (ring_advance).  Appended, like the draw
  int64_t ext_stride;
  // RVO draw (cagpu_step_noise; rd_seed == 0 everywhere else): the members of CaRvoDraw.  Appended, like the tape; the
  // pipelined kernels never see a launch with it (pipe_eligible)
  unsigned long long rd_seed;
  double rd_c, rd_T, rd_std;
  const uint8_t* rd_mask;
  const int64_t* rd_addr;
};

// One agent's share of an episode-log record (CaEpLog): env e ends its episode number `ep` (its reset count before the
// increment) and every agent lane stores its 32-byte row of slot ep % C of the env's own ring as two 16-byte stores;
// agent 0's lane stores the 16-byte head {ep, steps, case, outcome} as well.  Plain stores, no ordering between envs.
// `next_case` is the table row the auto-reset is about to load, (env_id_offset + e + (ep + 1) case_stride) mod n_cases: the
// ended episode ran on the row case_step = case_stride mod n_cases before it.
__device__ __forceinline__ void eplog_store(double* const rows, int32_t* const head, const int cap, const long e,
                                            const int next_case, const int case_step, const int n_cases, const int N,
                                            const int a, const int ep, const double ep_reward, const double t,
                                            const double extra, const uint32_t flags, const int steps, const bool any_coll,
                                            const bool all_goal) {
  const long slot = e * cap + ep % cap;
  double2* q = reinterpret_cast<double2*>(rows + (slot * N + a) * 4);
  q[0] = make_double2(ep_reward, t);
  q[1] = make_double2(extra, __longlong_as_double(static_cast<long long>(flags)));  // (low 32 bits: the word; high 32: zero)
  if (a == 0) {
    int c = next_case - case_step;
    if (c < 0) c += n_cases;
    *reinterpret_cast<int4*>(head + slot * 4) = make_int4(ep, steps, c, any_coll ? 0 : (all_goal ? 1 : 2));
  }
}

// One row of the trajectory tape (CaTraj): the reference's global_state_history row (agent.py:275-287) + its index.
// 96 bytes = six 16-byte stores; the rows of a tile's lanes are contiguous.
__device__ __forceinline__ void traj_store(double* row, const double t, const double px, const double py, const double gx,
                                           const double gy, const double rad, const double ps, const double vx,
                                           const double vy, const float speed, const double heading, const int index) {
  double2* q = reinterpret_cast<double2*>(row);
  q[0] = make_double2(t, px);
  q[1] = make_double2(py, gx);
  q[2] = make_double2(gy, rad);
  q[3] = make_double2(ps, vx);
  q[4] = make_double2(vy, static_cast<double>(speed));
  q[5] = make_double2(heading, static_cast<double>(index));
}
// ... columns 1 - 11 of a row whose column 0 (the clock before the move) is already out
__device__ __forceinline__ void traj_store_tail(double* row, const double px, const double py, const double gx, const double gy,
                                                const double rad, const double ps, const double vx, const double vy,
                                                const float speed, const double heading, const int index) {
  row[1] = px;
  double2* q = reinterpret_cast<double2*>(row);
  q[1] = make_double2(py, gx);
  q[2] = make_double2(gy, rad);
  q[3] = make_double2(ps, vx);
  q[4] = make_double2(vy, static_cast<double>(speed));
  q[5] = make_double2(heading, static_cast<double>(index));
}

// A map-set env's grid (KArgs / ScanArgs .env_map): map m of the set, or nullptr -- no walls, no map memory read -- for an
// index outside [0, num_maps), which raises bit 2 of the fault word when `report` (one lane per env reports).
__device__ unsigned int g_fault = 0u;
__device__ __forceinline__ const uint32_t* set_grid(const uint32_t* bits, const long words, const int num_maps, const int m,
                                                    const bool report) {
  if (m >= 0 && m < num_maps) return bits + static_cast<long>(m) * words;
  if (report) atomicOr(&g_fault, 4u);
  return nullptr;
}

// ---------------------------------------------------------------- small math helpers
struct F2 {
  float x, y;
};
__device__ __forceinline__ F2 f2(float x, float y) { F2 v; v.x = x; v.y = y; return v; }
__device__ __forceinline__ F2 operator+(F2 a, F2 b) { return f2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ F2 operator-(F2 a, F2 b) { return f2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ F2 operator*(float s, F2 a) { return f2(s * a.x, s * a.y); }
__device__ __forceinline__ float dotf(F2 a, F2 b) { return a.x * b.x + a.y * b.y; }
__device__ __forceinline__ float detf(F2 a, F2 b) { return a.x * b.y - a.y * b.x; }
__device__ __forceinline__ float sqf(float a) { return a * a; }
// IEEE correctly-rounded float divide / sqrt: plain `/` and sqrtf under hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt (passed explicitly by build_native.py).  NOT __fsqrt_rn:
// in this ROCm that intrinsic maps to the native (not correctly rounded) square root.
__device__ __forceinline__ float divf(float a, float b) { return a / b; }
__device__ __forceinline__ float sqrtf_rn(float a) { return sqrtf(a); }
// The same two operations for the step kernel's ORCA phases: the compiler's correctly rounded sequences WITHOUT their range
// handling (v_div_scale / v_div_fixup; the 2^32 rescaling and the class test of the square root) -- the same arithmetic
// whenever no operand, intermediate or result is denormal, huge or NaN: 8 instead of 11 and 9 instead of 14 instructions,
// all of them on dependent chains (linearProgram1 / 3 are chains of divisions).  scratch/divsqrt_check.hip: identical
// bits on 2^28 random operands with exponents in [-60, 60] (division, reciprocal) / x in [2^-80, 2^80] (square root).
// ORCA's operands are velocities, positions and their differences -- 0 (handled: 0 / b = 0, sqrt(0) = 0) or 1e-16 .. 1e8
// in magnitude.  The stand-alone cagpu_orca kernel keeps the compiler's `/` and sqrtf for arbitrary inputs, and both
// are held to the same oracle bit for bit (tests/test_gpu_parity.py).
__device__ __forceinline__ float divq(float a, float b) {
  float y = __builtin_amdgcn_rcpf(b);
  const float e = __builtin_fmaf(-b, y, 1.0f);
  y = __builtin_fmaf(e, y, y);
  float q = a * y;
  float r = __builtin_fmaf(-b, q, a);
  q = __builtin_fmaf(r, y, q);
  r = __builtin_fmaf(-b, q, a);
  return __builtin_fmaf(r, y, q);
}
__device__ __forceinline__ float sqrtq(float x) {
  const float s = __builtin_amdgcn_sqrtf(x);
  const float s_dn = __int_as_float(__float_as_int(s) - 1), s_up = __int_as_float(__float_as_int(s) + 1);
  const float r_dn = __builtin_fmaf(-s_dn, s, x), r_up = __builtin_fmaf(-s_up, s, x);
  float o = (r_dn <= 0.0f) ? s_dn : s;
  o = (r_up > 0.0f) ? s_up : o;
  return (x == 0.0f) ? x : o;
}
// ... and for float64 (distances, preferred velocity, ego frame: UnicycleDynamics / Dynamics / the sensor): the compiler's
// sequences are rsq + 9 multiply-adds (square root) and rcp + 2 Newton steps + one residual correction (divide); the range
// handling around them (v_ldexp / v_cmp_class / v_div_scale / v_div_fixup) costs 8 and 3 more instructions per call.
// scratch/divsqrt_check.hip: identical bits on 2^28 random operands with exponents in [-300, 300] / [-600, 600].
__device__ __forceinline__ double divd(double a, double b) {
  double y = __builtin_amdgcn_rcp(b);
  y = __builtin_fma(__builtin_fma(-b, y, 1.0), y, y);
  y = __builtin_fma(__builtin_fma(-b, y, 1.0), y, y);
  const double q = a * y;
  return __builtin_fma(__builtin_fma(-b, q, a), y, q);
}
__device__ __forceinline__ double sqrtd(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double r = __builtin_fma(-h, g, 0.5);
  g = __builtin_fma(g, r, g);
  h = __builtin_fma(h, r, h);
  g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
  g = __builtin_fma(__builtin_fma(-g, g, x), h, g);
  return (x == 0.0) ? x : g;
}
// RVO2's Vector2 / float: multiply by the reciprocal
__device__ __forceinline__ F2 over(F2 a, float s) { const float inv = divf(1.0f, s); return f2(a.x * inv, a.y * inv); }
__device__ __forceinline__ F2 unitf(F2 a) { return over(a, sqrtf_rn(dotf(a, a))); }
__device__ __forceinline__ F2 unitq(F2 a) { const float inv = divq(1.0f, sqrtq(dotf(a, a))); return f2(a.x * inv, a.y * inv); }

__device__ __forceinline__ double wrap_pi(double a) {  // util.py:141-146 ([-pi, pi))
  if (a >= kPi) a -= kTwoPi;   // first iteration of the reference's while loops, branch-free
  if (a < -kPi) a += kTwoPi;
  if (!(a < kPi) || a < -kPi) {  // more than one turn out of range: the general loops (bounded)
    for (int it = 0; it < 4096 && a >= kPi; ++it) a -= kTwoPi;
    for (int it = 0; it < 4096 && a < -kPi; ++it) a += kTwoPi;
  }
  return a;
}

// sin and cos of a heading in [-pi, pi] (UnicycleDynamics.py:29-32): Cody-Waite reduction by pi/2 (two-part constant,
// |k| <= 2) and the fdlibm kernel polynomials -- ~45 instructions where the general-range libm sincos needs ~150.
// Accuracy (checked against long-double libm on 2e7 arguments; tests/test_gpu_move_edges.py holds the claim on the edge
// operands and 65 536 draws: 0.776 / 0.709 ulp): <= 1 ulp, except within 1e-11 of a multiple of pi/2
// where the ABSOLUTE error stays below 1e-26 (the result itself is ~1e-12 there); 97.6 % of the results are
// bit-identical to glibc's.  The products these feed are positions of order 1..10 m.
__device__ __forceinline__ void sincos_heading(double x, double& s, double& c) {
  // (x * 2/pi + 0.0 in one fma: the same product, but +0 for x = -0, so that -kf below is -0 and r, y and the sine keep
  // the sign of x = -0 like libm's -- with a plain product sin(-0) came out +0)
  const double kf = rint(__builtin_fma(x, 6.36619772367581382433e-01, 0.0));
  const int k = static_cast<int>(kf);
  const double r = __builtin_fma(-kf, 1.57079632673412561417e+00, x);  // first 33 bits of pi/2: exact product
  const double w = kf * 6.07710050650619224932e-11;                     // pi/2 - the 33 bits
  const double y = r - w;
  const double yt = (r - y) - w;
  const double z = y * y;
  const double v = z * y;
  const double rs = __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, 1.58969099521155010221e-10,
                    -2.50507602534068634195e-08), 2.75573137070700676789e-06), -1.98412698298579493134e-04),
                    8.33333333332248946124e-03);
  const double sn = y - ((z * (0.5 * yt - v * rs) - yt) - v * -1.66666666666666324348e-01);
  const double rc = z * __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z, __builtin_fma(z,
                    -1.13596475577881948265e-11, 2.08757232129817482790e-09), -2.75573143513906633035e-07),
                    2.48015872894767294178e-05), -1.38888888888741095749e-03), 4.16666666666666019037e-02);
  const double hz = 0.5 * z;
  const double ww = 1.0 - hz;
  const double cs = ww + (((1.0 - ww) - hz) + (z * rc - y * yt));
  const bool swap = (k & 1) != 0;
  const double s0 = swap ? cs : sn, c0 = swap ? sn : cs;
  s = (k & 2) ? -s0 : s0;
  c = (((k + 1) & 2) != 0) ? -c0 : c0;
}

// ---------------------------------------------------------------- ORCA (RVO2 algorithm, C float)
// Lines live in LDS as float4 {point.x, point.y, dir.x, dir.y}, slot-major: line k of this lane
// is L[k * STRIDE].  The permitted half-plane is to the left of dir through point.
template <int STRIDE>
__device__ bool lp1(const float4* L, int k, float radius, F2 opt, bool dir_opt, F2& res) {
  const float4 lk = L[k * STRIDE];
  const F2 pk = f2(lk.x, lk.y), dk = f2(lk.z, lk.w);
  const float dp = dotf(pk, dk);
  const float disc = sqf(dp) + sqf(radius) - dotf(pk, pk);
  if (disc < 0.0f) return false;
  const float sd = sqrtf_rn(disc);
  float t_lo = -dp - sd;
  float t_hi = -dp + sd;
  for (int i = 0; i < k; ++i) {
    const float4 li = L[i * STRIDE];
    const F2 pi = f2(li.x, li.y), di = f2(li.z, li.w);
    const float den = detf(dk, di);
    const float num = detf(di, pk - pi);
    if (fabsf(den) <= kRvoEps) {
      if (num < 0.0f) return false;
      continue;
    }
    const float t = divf(num, den);
    if (den >= 0.0f) t_hi = (t < t_hi) ? t : t_hi;
    else t_lo = (t_lo < t) ? t : t_lo;
    if (t_lo > t_hi) return false;
  }
  if (dir_opt) {
    if (dotf(opt, dk) > 0.0f) res = pk + t_hi * dk;
    else res = pk + t_lo * dk;
  } else {
    const float t = dotf(dk, opt - pk);
    if (t < t_lo) res = pk + t_lo * dk;
    else if (t > t_hi) res = pk + t_hi * dk;
    else res = pk + t * dk;
  }
  return true;
}

template <int STRIDE>
__device__ int lp2(const float4* L, int n, float radius, F2 opt, bool dir_opt, F2& res) {
  if (dir_opt) res = radius * opt;
  else if (dotf(opt, opt) > sqf(radius)) res = radius * unitf(opt);
  else res = opt;
  for (int i = 0; i < n; ++i) {
    const float4 li = L[i * STRIDE];
    if (detf(f2(li.z, li.w), f2(li.x, li.y) - res) > 0.0f) {
      const F2 keep = res;
      if (!lp1<STRIDE>(L, i, radius, opt, dir_opt, res)) {
        res = keep;
        return i;
      }
    }
  }
  return n;
}

template <int STRIDE>
__device__ void lp3(const float4* L, float4* P, int n, int begin, float radius, F2& res) {
  float depth = 0.0f;
  for (int i = begin; i < n; ++i) {
    const float4 li = L[i * STRIDE];
    const F2 pi = f2(li.x, li.y), di = f2(li.z, li.w);
    if (detf(di, pi - res) > depth) {
      int m = 0;
      for (int j = 0; j < i; ++j) {
        const float4 lj = L[j * STRIDE];
        const F2 pj = f2(lj.x, lj.y), dj = f2(lj.z, lj.w);
        const float D = detf(di, dj);
        F2 pt;
        if (fabsf(D) <= kRvoEps) {
          if (dotf(di, dj) > 0.0f) continue;
          pt = 0.5f * (pi + pj);
        } else {
          pt = pi + divf(detf(dj, pi - pj), D) * di;
        }
        const F2 dr = unitf(dj - di);
        P[m * STRIDE] = make_float4(pt.x, pt.y, dr.x, dr.y);
        ++m;
      }
      const F2 keep = res;
      if (lp2<STRIDE>(P, m, radius, f2(-di.y, di.x), true, res) < m) res = keep;
      depth = detf(di, pi - res);
    }
  }
}

// Half-plane induced on `me` by `ot` (Agent::computeNewVelocity, agent part).
__device__ __forceinline__ float4 half_plane(F2 mpos, F2 mvel, float mrad, F2 opos, F2 ovel, float orad, float collab,
                                             float inv_h, float time_step) {
  const F2 rp = opos - mpos;
  const F2 rv = mvel - ovel;
  const float d2 = dotf(rp, rp);
  const float R = mrad + orad;
  const float R2 = sqf(R);
  F2 dir, u;
  if (d2 > R2) {
    const F2 w = rv - inv_h * rp;
    const float w2 = dotf(w, w);
    const float dp1 = dotf(w, rp);
    if (dp1 < 0.0f && sqf(dp1) > R2 * w2) {
      const float wl = sqrtf_rn(w2);
      const F2 uw = over(w, wl);
      dir = f2(uw.y, -uw.x);
      u = (R * inv_h - wl) * uw;
    } else {
      const float leg = sqrtf_rn(d2 - R2);
      if (detf(rp, w) > 0.0f) {
        dir = over(f2(rp.x * leg - rp.y * R, rp.x * R + rp.y * leg), d2);
      } else {
        const F2 t = over(f2(rp.x * leg + rp.y * R, -rp.x * R + rp.y * leg), d2);
        dir = f2(-t.x, -t.y);
      }
      const float dp2 = dotf(rv, dir);
      u = dp2 * dir - rv;
    }
  } else {
    const float inv_dt = divf(1.0f, time_step);
    const F2 w = rv - inv_dt * rp;
    const float wl = sqrtf_rn(dotf(w, w));
    const F2 uw = over(w, wl);
    dir = f2(uw.y, -uw.x);
    u = (R * inv_dt - wl) * uw;
  }
  const F2 pt = mvel + collab * u;
  return make_float4(pt.x, pt.y, dir.x, dir.y);
}

// The same half-plane without divergent branches (step kernel): the three cases of computeNewVelocity share ONE square
// root and ONE reciprocal on selected inputs -- cut-off disc: sqrt(w.w), 1 / |w| (also the overlap case, which is the
// cut-off disc of a one-step horizon); legs: sqrt(distSq - R^2), 1 / distSq -- so a wave whose lanes fall into different
// cases runs the long dependent chain once instead of once per case.  Every selected expression is the one above:
// bit-identical results (tests: the stand-alone cagpu_orca kernel keeps the branchy form, both match the oracle).
__device__ __forceinline__ float4 half_plane_sel(F2 mpos, F2 mvel, float mrad, F2 opos, F2 ovel, float orad, float collab,
                                                 float inv_h, float inv_dt) {
  const F2 rp = opos - mpos;
  const F2 rv = mvel - ovel;
  const float d2 = dotf(rp, rp);
  const float R = mrad + orad;
  const float R2 = sqf(R);
  const bool far = d2 > R2;
  const float kk = far ? inv_h : inv_dt;
  const F2 w = rv - kk * rp;
  const float w2 = dotf(w, w);
  const float dp1 = dotf(w, rp);
  const bool disc = !far || (dp1 < 0.0f && sqf(dp1) > R2 * w2);
  const float sq = sqrtq(disc ? w2 : (d2 - R2));  // |w|  or  the leg length
  const float inv = divq(1.0f, disc ? sq : d2);
  // cut-off disc (and overlap)
  const F2 uw = f2(w.x * inv, w.y * inv);
  const F2 dir_a = f2(uw.y, -uw.x);
  const F2 u_a = (R * kk - sq) * uw;
  // legs
  const bool left = detf(rp, w) > 0.0f;
  const float bx = left ? (rp.x * sq - rp.y * R) : (rp.x * sq + rp.y * R);
  const float by = left ? (rp.x * R + rp.y * sq) : (-rp.x * R + rp.y * sq);
  const F2 t = f2(bx * inv, by * inv);
  const F2 dir_b = left ? t : f2(-t.x, -t.y);
  const float dp2 = dotf(rv, dir_b);
  const F2 u_b = dp2 * dir_b - rv;
  const F2 dir = disc ? dir_a : dir_b;
  const F2 u = disc ? u_a : u_b;
  const F2 pt = mvel + collab * u;
  return make_float4(pt.x, pt.y, dir.x, dir.y);
}

// New ORCA velocity of the agent on this lane.  fpx/fpy/fvx/fvy/frad: the tile's float bodies in LDS,
// `ebase` = LDS index of agent 0 of my env, `a` my agent index, N agents per env.  dcol: [N][STRIDE]
// float scratch column, L / P: [N-1][STRIDE] float4 line columns (all already offset to my lane).
template <int STRIDE>
__device__ F2 orca_velocity(const float* fpx, const float* fpy, const float* fvx, const float* fvy, const float* frad,
                            int ebase, int a, int N, F2 pref, float max_speed, float collab, float time_horizon,
                            float time_step, float neighbor_dist, int max_nb, float* dcol, float4* L, float4* P) {
  const F2 mpos = f2(fpx[ebase + a], fpy[ebase + a]);
  const F2 mvel = f2(fvx[ebase + a], fvy[ebase + a]);
  const float mrad = frad[ebase + a];
  const float range_sq = sqf(neighbor_dist);
  // neighbour list = others with distSq < rangeSq, ascending by distSq, ties by index, first max_nb
  int cnt = 0;
  for (int j = 0; j < N; ++j) {
    float d2 = INFINITY;
    if (j != a) {
      const F2 d = mpos - f2(fpx[ebase + j], fpy[ebase + j]);
      d2 = dotf(d, d);
      if (d2 < range_sq) ++cnt; else d2 = INFINITY;
    }
    dcol[j * STRIDE] = d2;
  }
  const int n = cnt < max_nb ? cnt : max_nb;
  const float inv_h = divf(1.0f, time_horizon);
  for (int j = 0; j < N; ++j) {
    const float dj = dcol[j * STRIDE];
    if (j == a || !(dj < INFINITY)) continue;
    int rank = 0;
    for (int q = 0; q < N; ++q) {
      const float dq = dcol[q * STRIDE];
      rank += (dq < dj) || (dq == dj && q < j);
    }
    if (rank >= n) continue;
    L[rank * STRIDE] = half_plane(mpos, mvel, mrad, f2(fpx[ebase + j], fpy[ebase + j]), f2(fvx[ebase + j], fvy[ebase + j]),
                                  frad[ebase + j], collab, inv_h, time_step);
  }
  F2 v;
  const int fail = lp2<STRIDE>(L, n, max_speed, pref, false, v);
  if (fail < n) lp3<STRIDE>(L, P, n, fail, max_speed, v);
  return v;
}

// ---------------------------------------------------------------- ego frame (agent.py:329-349, Dynamics.py:24-41)
struct Ego {
  double dist, prx, pry, orx, ory, heading_ego;
};
__device__ __forceinline__ Ego ego_frame(double px, double py, double gx, double gy, double heading) {
  Ego e;
  const double dx = gx - px, dy = gy - py;
  e.dist = sqrtd(dx * dx + dy * dy);
  if (e.dist > 1e-8) {
    e.prx = divd(dx, e.dist);
    e.pry = divd(dy, e.dist);
  } else {
    e.prx = dx;
    e.pry = dy;
  }
  e.orx = -e.pry;
  e.ory = e.prx;
  e.heading_ego = wrap_pi(heading - atan2(e.pry, e.prx));
  return e;
}

// time to impact of `host` with `other` (util.py:23-83 compute_time_to_impact + :101-127 tangent_vecs_from_external_pt),
// float64 in the numpy operation order; only used by the time_to_impact sorting mode of the sensor
__device__ double time_to_impact(double hx, double hy, double ox, double oy, double hvx, double hvy, double ovx,
                                 double ovy, double r) {
  const double v0 = hvx - ovx, v1 = hvy - ovy;
  const double xp = hx, yp = hy, a = ox, b = oy;
  const double sq = (xp - a) * (xp - a) + (yp - b) * (yp - b) - r * r;
  if (sq < 0) return 0.0;
  const double st = sqrt(sq);
  const double xnum1 = r * r * (xp - a), xnum2 = r * (yp - b) * st;
  const double ynum1 = r * r * (yp - b), ynum2 = r * (xp - a) * st;
  const double den = (xp - a) * (xp - a) + (yp - b) * (yp - b);
  const double c1x = ((xnum1 + xnum2) / den + a) - xp, c1y = ((ynum1 - ynum2) / den + b) - yp;
  const double c2x = ((xnum1 - xnum2) / den + a) - xp, c2y = ((ynum1 + ynum2) / den + b) - yp;
  const double x11 = c1x * v1 - c1y * v0, x12 = c1x * c2y - c1y * c2x;
  const double x21 = c2x * v1 - c2y * v0, x22 = c2x * c1y - c2y * c1x;
  if (!(x11 * x12 >= 0 && x21 * x22 >= 0)) return INFINITY;
  if (fabs(v0) < 1e-5 && fabs(v1) < 1e-5) return INFINITY;
  const double px = hx, py = hy;
  double x1, x2, y1, y2;
  if (fabs(v0) < 1e-5) {
    x1 = x2 = px;
    const double A = 1, B = -2 * b, Cc = b * b + (px - a) * (px - a) - r * r;
    y1 = (-B + sqrt(B * B - 4 * A * Cc)) / (2 * A);
    y2 = (-B - sqrt(B * B - 4 * A * Cc)) / (2 * A);
  } else {
    const double m = v1 / v0;
    const double A = 1 + m * m;
    const double B = -2 * a + 2 * m * (py - b - m * px);
    const double Cc = a * a - r * r + (m * px - (py - b)) * (m * px - (py - b));
    x1 = (-B + sqrt(B * B - 4 * A * Cc)) / (2 * A);
    x2 = (-B - sqrt(B * B - 4 * A * Cc)) / (2 * A);
    y1 = m * (x1 - px) + py;
    y2 = m * (x2 - px) + py;
  }
  const double d1 = sqrt((x1 - px) * (x1 - px) + (y1 - py) * (y1 - py));
  const double d2 = sqrt((x2 - px) * (x2 - px) + (y2 - py) * (y2 - py));
  const double d = d2 < d1 ? d2 : d1;
  return d / sqrt(v0 * v0 + v1 * v1);
}

// The device's fault word (cagpu_device_faults; defined above KArgs' set_grid): bit 0 = a bounded hand-over poll of the
// pipelined step kernel ran out (cagpu_pipe.inc), bit 1 = a GA3C-CADRL operand left the fp16 range of the network kernel's
// two-plane split (cagpu_ga3c.inc), bit 2 = a map-set env's map index lay outside [0, num_maps) (set_grid), bit 3 = an env of
// a case stream ran past its window between two refills (cagpu_gen.inc stream_refill_kernel).

#include "cagpu_grouplp.inc"

// x / D for small non-negative x: with a compile-time D two full-rate instructions (24-bit multiply by ceil(2^20 / D),
// shift; exact while x * D < 2^20), otherwise the float reciprocal form (convert, add, multiply, convert).  The remainder
// x - q * D likewise takes the 24-bit multiply (v_mul_lo_u32 is a quarter-rate instruction).
template <int D>
__device__ __forceinline__ int div_small(const int x, const float inv_d) {
  if (D > 0) return static_cast<int>(__umul24(static_cast<unsigned>(x), static_cast<unsigned>(((1 << 20) + (D > 0 ? D : 1) - 1) / (D > 0 ? D : 1))) >> 20);
  return static_cast<int>((static_cast<float>(x) + 0.5f) * inv_d);
}

// for (q = 0; q < n; ++q) body(q) in blocks of BLK: with a run-time n (the generic kernel) the loads of a block are in
// flight together instead of one LDS round trip per iteration (N = 50: the rank loop of the sensor took 57 k of the
// step's 155 k cycles as a plain loop); with a compile-time n everything unrolls as before.
template <int BLK, typename F>
__device__ __forceinline__ void for_n(const int n, F&& body) {
  int q = 0;
  for (; q + BLK <= n; q += BLK) {
#pragma unroll
    for (int u = 0; u < BLK; ++u) body(q + u);
  }
#pragma unroll
  for (int u = 0; u < BLK - 1; ++u)
    if (q + u < n) body(q + u);
}

// ---------------------------------------------------------------- main kernel
// Work decomposition of one tile (ROW = 64 agent slots = floor(64/N) whole envs) on a workgroup of NT threads:
//   agent phases  (A*): one LANE per agent, on wave 0 only -- the serial per-agent chains (incremental LP,
//                       float64 atan2/sincos, flags).  The other waves wait at the barrier and cost no issue slots.
//   pair phases   (P*): one THREAD per ordered (agent, other) pair, spread over all NT threads -- ORCA
//                       neighbour distances + half-planes, collision gaps, sensor keys / ranks / row emission.
// Everything the phases exchange lives in LDS; per-(agent, slot) arrays are [slot][ROW] columns so that a phase that
// walks slots for a fixed agent (wave 0) and a phase that walks agents for a fixed slot both stay conflict-free.
constexpr int ROW = 64;
// Column stride of the per-(agent, slot) LDS tiles [slot][CS]: ODD, so that the lanes of one agent, which hold different
// slots -- the half-plane store Lmat[rank * CS + agent] of the ORCA phase: a stride of 64 float4 put all nine of them on
// the same four banks (SQ_LDS_BANK_CONFLICT 767 k cycles per launch at 4096 x 10, profiles/r02_rocprof_summary.md) --
// spread over the banks, while lanes that walk agents for a fixed slot stay consecutive.
constexpr int CS_ROW = ROW + 1;
constexpr int KEY_NONE = 2147483647;  // sort key of a pair that is not sensed (self, beyond the sensing horizon)
#define LP1_UNROLL _Pragma("unroll")
// Workgroup barrier between phases that exchange data through LDS.
#define WG_SYNC() __syncthreads()
// Wave priorities per phase (s_setprio 0..3).  Four workgroups share a CU, so every SIMD holds one wave of each of them,
// usually in different phases.  The agent wave's serial chains (one lane per agent: they are what the workgroup's other
// three waves are waiting for) and the linearProgram3 stragglers issue first (3), then pair phases in the order of the
// step (a workgroup that is behind overtakes one that is ahead: ORCA pairs 2, sensor pairs 1), the emission phase and the
// post-linearProgram3 wait last (0): 21.6 -> 20.3 us per step, rollout 14.1 -> 12.6 (profiles/r02_kernel_geometry.md).
// Variations (sensor phases one level up; ORCA pairs at 3; emission at 1) all measured 0.05 - 0.3 us behind.
#define PRIO(level) __builtin_amdgcn_s_setprio(level)
// Pair items w = 0 .. n_items-1 are dealt to the NT threads in rounds; odd rounds run BACKWARDS over the threads, so the
// last, partial round lands on the highest waves and wave 0 -- the agent wave -- is free for its one-lane-per-agent work
// while the other waves finish the pair phase (400 items on 256 threads: wave 0 has one round, waves 2 and 3 two).
#define FOR_ITEMS_UPTO(w, count)                                                       \
  for (int base_ = 0, odd_ = 0; base_ < (count); base_ += NT, odd_ ^= 1)              \
    if (const int w = base_ + (odd_ ? (NT - 1 - tid) : tid); w < (count))
#define FOR_PAIR_ITEMS(w) FOR_ITEMS_UPTO(w, n_items)

__host__ __device__ inline size_t align16(size_t x) { return (x + 15) & ~static_cast<size_t>(15); }
#include "cagpu_scan.inc"
#include "cagpu_occ.inc"
#include "cagpu_render.inc"
#include "cagpu_metrics.inc"
#include "cagpu_ga3c.inc"
#include "cagpu_ga3c_grad.inc"  // the network's weight gradients (cagpu_ga3c_grad)
#include "cagpu_gen.inc"

// The map a map-set env takes at its k-th auto-reset (CaMapSet.map_seed): min(floor(M u), M - 1), u the Philox uniform of
// (seed; global env id lo, hi, k, 0xFFFFFFFF) -- the reset headings' construction with a last counter word no agent index has
__device__ __forceinline__ int32_t map_draw(const unsigned long long seed, const long ge, const int k, const int num_maps) {
  const unsigned long long g = static_cast<unsigned long long>(ge);
  const double u = gen::uniform_at(seed, static_cast<unsigned>(g), static_cast<unsigned>(g >> 32), static_cast<unsigned>(k),
                                   0xFFFFFFFFu);
  const int m = static_cast<int>(floor(num_maps * u));
  return m < num_maps - 1 ? m : num_maps - 1;
}

// cagpu_map_draw: map_draw for given (global env id, reset count) pairs
__global__ __launch_bounds__(256) void map_draw_kernel(const unsigned long long seed, const int num_maps, const int64_t* env_ids,
                                                        const int32_t* counts, const long n, int32_t* out) {
  const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) out[i] = map_draw(seed, env_ids[i], counts[i], num_maps);
}

// ---- policy draw (CaPolicyDraw in cagpu.h has the rule).  Its uniform for counter word `slot` of env ge's episode k:
__device__ __forceinline__ double draw_uniform(const unsigned long long seed, const long ge, const int k, const unsigned slot) {
  const unsigned long long g = static_cast<unsigned long long>(ge);
  return gen::uniform_at(seed, static_cast<unsigned>(g), static_cast<unsigned>(g >> 32), static_cast<unsigned>(k), slot);
}
// step 1: #{j : cdf[j] <= u}, clamped to P - 1
__device__ __forceinline__ int draw_index(const double* cdf, const int P, const double u) {
  int j = 0;
  for (int q = 0; q < P; ++q) j += static_cast<int>(cdf[q] <= u);
  return j < P - 1 ? j : P - 1;
}
// step 2's slot: the r-th of n present slots takes `ensure`
__device__ __forceinline__ int draw_ensure_rank(const unsigned long long seed, const long ge, const int k, const int n) {
  const int r = static_cast<int>(floor(n * draw_uniform(seed, ge, k, 0xFFFFFFFEu)));
  return r < n - 1 ? r : n - 1;
}
// The flag word of slot a of env ge in episode k.  The lane recomputes the draws of its env's other slots to settle the
// ensure rule (N <= 64 here, a few times per episode): no exchange with another lane.  present(j): slot j holds an agent.
template <typename Present>
__device__ __forceinline__ uint32_t policy_draw_word(const double* cdf, const uint32_t* bits, const int P, const int ensure,
                                                     const unsigned long long seed, const long ge, const int k, const int a,
                                                     const int N, const Present present, const uint32_t flags) {
  if (!present(a)) return flags;
  int mine = draw_index(cdf, P, draw_uniform(seed, ge, k, static_cast<unsigned>(a)));
  if (ensure >= 0 && mine != ensure) {
    int n = 0, before = 0;
    bool any = false;
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      if (!present(j)) continue;
      ++n;
      before += static_cast<int>(j < a);
      if (j != a && !any) any = draw_index(cdf, P, draw_uniform(seed, ge, k, static_cast<unsigned>(j))) == ensure;
    }
    if (!any && before == draw_ensure_rank(seed, ge, k, n)) mine = ensure;
  }
  return (flags & ~0xFC0u) | (bits[mine] & 0xFC0u);
}

// cagpu_policy_draw: the rule on the current state, one thread per agent slot
struct DrawArgs {
  uint32_t* flags;
  const int32_t* reset_count;
  float* obs;           // or nullptr
  const uint8_t* mask;  // or nullptr
  const double* cdf;
  const uint32_t* bits;
  unsigned long long seed;
  long env_id_offset, total;
  int32_t N, W, P, ensure, ragged;
};
__global__ __launch_bounds__(256) void policy_draw_kernel(const DrawArgs d) {
  const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= d.total) return;
  const long e = i / d.N;
  const int a = static_cast<int>(i - e * d.N);
  if (d.mask && !d.mask[e]) return;
  const uint32_t* fl = d.flags + e * d.N;
  const bool ragged = d.ragged != 0;
  const auto present = [&](const int j) { return !(ragged && (fl[j] & CA_ABSENT)); };
  if (!present(a)) return;
  // (the other slots' words are read for CA_ABSENT only, which no thread writes)
  const uint32_t f = policy_draw_word(d.cdf, d.bits, d.P, d.ensure, d.seed, d.env_id_offset + e, d.reset_count[e], a, d.N,
                                      present, fl[a]) & ~static_cast<uint32_t>(CA_PLAN_VALID);
  d.flags[i] = f;
  if (d.obs) d.obs[i * d.W] = (f & CA_IS_LEARNING) ? 1.f : 0.f;
}

// fixed: 7 f64 + 10 f32 + 4 u32 per agent slot (the 3 f64 of the episode scratch alias six ORCA float arrays) + the
// linearProgram3 queue (length + up to ROW entries, then the number of ORCA queries)
__host__ __device__ inline size_t lds_fixed_bytes(int row = ROW) {
  return static_cast<size_t>(row) * (7 * 8 + 10 * 4 + 4 * 4) + align16(static_cast<size_t>(row + 3) * 4);
}
// union, ORCA view: half-planes [N-1][CS] float4, the solution of every line's 1-D programme [N-1][CS] float2 + its
// feasibility byte; the projected lines of linearProgram3 live in the registers of the solving group
__host__ __device__ inline size_t lds_orca_lines(int N, int cs) { return static_cast<size_t>(cs) * (N > 1 ? N - 1 : 1); }
__host__ __device__ inline size_t lds_orca_bytes(int N, int cs = ROW) {
  return lds_orca_lines(N, cs) * (16 + 8) + align16(lds_orca_lines(N, cs));
}
// union, sensor view: p_orth / gap / time-to-impact [N][CS] f64, key i32, dist_2_other f32, rank u8,
// obs staging [ROW*W] f32
__host__ __device__ inline size_t lds_sense_bytes(int N, int W, int stage, int tti, int cs = ROW, int row = ROW) {
  return align16(static_cast<size_t>(cs) * N * ((tti ? 3 : 2) * 8 + 9)) + (stage ? align16(static_cast<size_t>(row) * W * 4) : 0);
}

struct Lane {  // per-lane registers of one agent (wave 0)
  double px, py, vx, vy, heading, gx, gy, rad, ps, tr, t, slt, epr;
  float act0, act1;
  uint32_t flags;
  int32_t step_num;
  double td;  // Agent.turning_dir (only where CaState.turning_dir is given)
};

// Agent.turning_dir after UnicycleDynamics.step turned the agent to heading `nh` (UnicycleDynamics.py:41-47)
__device__ __forceinline__ double turning_dir_next(const double td, const double nh) {
  if (fabs(td) < 1e-5) return 0.11 * ((nh > 0.0) - (nh < 0.0));
  if (td * nh < 0.0) return fmax(-kPi, fmin(kPi, -td + nh));
  return ((td > 0.0) - (td < 0.0)) * fmax(0.0, fabs(td) - 0.1);
}

// test_cases.py:545-557 + agent.py:59-138
// (the heading travels by value: a pointer to a local kept a 16-byte scratch object alive in every instantiation)
template <typename Params>  // (CaParams, or the pipelined kernel's address-space-qualified view of it)
__device__ __forceinline__ void reset_lane(Lane& r, const double* c, const bool has_heading, const double heading,
                                           const Params& p) {
  r.px = c[0]; r.py = c[1]; r.gx = c[2]; r.gy = c[3]; r.ps = c[4]; r.rad = c[5];
  r.vx = r.vy = 0.0;
  r.heading = has_heading ? heading : atan2(c[3] - c[1], c[2] - c[0]);
  const double dx = c[0] - c[2], dy = c[1] - c[3];
  r.slt = (sqrt(dx * dx + dy * dy) - p.near_goal_threshold) / c[4];
  double tr = p.max_time_ratio * r.slt;
  if (p.dt > tr) tr = p.dt;
  r.tr = tr;
  r.t = 0.0;
  r.epr = 0.0;
  r.td = 0.0;
  r.act0 = r.act1 = 0.f;
  r.step_num = 0;
  r.flags &= ~(0x3Fu | CA_ABSENT | CA_PLAN_VALID);
  if (p.ragged && !(c[5] > 0.0)) {  // a padding row of a ragged table: the slot holds no agent in this episode
    r.px = r.py = r.gx = r.gy = r.rad = r.heading = r.slt = r.tr = 0.0;
    r.ps = 1.0;
    r.flags |= CA_ABSENT | CA_DONE | CA_AT_GOAL | CA_WAS_AT_GOAL;
  }
}

#include "cagpu_rules.inc"
#include "cagpu_replay.inc"
#include "cagpu_poses.inc"
#include "cagpu_sample.inc"  // the sampled GA3C-CADRL policy, the experience tape's pre-step record, GAE

// MSET: the n-step form (MULTI) also runs the map-set code of the single-step form -- the per-env grid of A3, the map draw
// of an auto-reset.  A template flag that only a set launch with n_steps > 1 selects (main_variant in cagpu_launch.inc): every other
// instantiation is the code it was before the flag existed.
// RD: the RVO draw (CaRvoDraw) -- instantiations of their own, of the general form (NC = 0) only, which nothing but a launch
// with a draw selects: behind a uniform test of the seed inside the existing instantiations the draw measured 18.0 -> 18.5 us
// per single step and 13.5 -> 13.7 per fused step at 4096 x 10 WITHOUT a draw (profiles/rvo_draw.md), outside the parent's spread.
template <int NT, bool STAGE, int NC, bool MULTI, bool RO, int TE = 0, bool MSET = false, bool RD = false>
// n-step: <= 128 VGPRs (four 4-wave workgroups per CU) -- except N = 20, whose single-step form already needs 172 (two
// workgroups per CU either way): held to 128 its n-step form spilled ~200 VGPRs to scratch around the step loop
__global__ __launch_bounds__(NT, MULTI ? (NC == 20 ? 2 : 4) : 1) void ca_kernel(const KArgs k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const CaParams& p = k.p;
  const int N = NC ? NC : p.num_agents;  // NC > 0: compile-time agent count (loops unroll, divisions fold)
  const int K = p.max_obs, W = 6 + 7 * K;
  const float inv_n = 1.0f / static_cast<float>(N);
  const int tile_envs = TE ? TE : (NC ? ROW / (NC ? NC : 1) : k.tile_envs);  // compile-time in the specialised kernels
  const int tile_n = tile_envs * N;
  const int n_items = tile_n * N;
  const int tid = threadIdx.x;
  // Wave 0 is the workgroup's AGENT WAVE (one lane per agent).  It needs no rotation across workgroups: the dispatcher
  // starts each workgroup of a CU on a different SIMD (scratch/hwid.hip: with 4 workgroups of 4 waves per CU every SIMD
  // holds exactly one wave 0), and rotating the role measured no difference (profiles/r02_kernel_geometry.md).
  const bool wave0 = tid < ROW;
  // identity of the agent on this lane (meaningful on wave 0 only)
  const int lane = tid & (ROW - 1);
  const int le = lane / N, a = lane - le * N;
  const long env0 = static_cast<long>(blockIdx.x) * tile_envs;
  const long e = env0 + le;
  const bool active = wave0 && (lane < tile_n) && (e < p.num_envs);
  const int ebase = active ? le * N : 0;
  const long i = e * N + a;
  const long tile_base = env0 * N;
  float* obs_tile = k.o.obs + tile_base * (6 + 7 * p.max_obs);  // the tile's observation rows (uniform: scalar arithmetic)
  long ring_a = 0, ring_e = 0;  // n-step kernel: this step's slot of the caller's output ring (cagpu_rollout_ring), in elements
  long traj_a = 0, traj_e = 0;  // ... and of the trajectory tape (CaTraj), which advances in a plain rollout too
  int step = 0;                 // the step of the launch (n-step kernel): an action tape's slot (cagpu_step_tape)
  long tile_cnt = static_cast<long>(p.num_envs) * N - tile_base;
  if (tile_cnt > tile_n) tile_cnt = tile_n;

  // ---- LDS
  double* sh_px = reinterpret_cast<double*>(smem);
  double* sh_py = sh_px + ROW;
  double* sh_vx = sh_py + ROW;
  double* sh_vy = sh_vx + ROW;
  double* sh_rad = sh_vy + ROW;
  double* sh_prx = sh_rad + ROW;  // ego frame ref_prll (ref_orth = (-pry, prx))
  double* sh_pry = sh_prx + ROW;
  float* sh_fpx = reinterpret_cast<float*>(sh_pry + ROW);  // ORCA's float bodies (dead once the policy phase is over)
  float* sh_fpy = sh_fpx + ROW;
  float* sh_fvx = sh_fpy + ROW;
  float* sh_fvy = sh_fvx + ROW;
  float* sh_frad = sh_fvy + ROW;
  float* sh_fms = sh_frad + ROW;                      // speed limit (float pref_speed)
  double* sh_r0 = reinterpret_cast<double*>(sh_fpx);  // episode-stat scratch of A3 -> A4: aliases the six arrays above
  double* sh_r1 = sh_r0 + ROW;
  double* sh_r2 = sh_r1 + ROW;
  uint32_t* sh_flag = reinterpret_cast<uint32_t*>(sh_fms + ROW);
  int* sh_q = reinterpret_cast<int*>(sh_flag + ROW);  // 1: this agent queries ORCA this step
  int* sh_nb = sh_q + ROW;                            // its neighbour count n
  int* sh_sense = sh_nb + ROW;                        // 1: (re)write this agent's observation in this pass
  float* sh_vrx = reinterpret_cast<float*>(sh_sense + ROW);  // ORCA velocity of each agent
  float* sh_vry = sh_vrx + ROW;
  float* sh_fprx = sh_vry + ROW;                      // its preferred velocity (float)
  float* sh_fpry = sh_fprx + ROW;
  int* sh_q3 = reinterpret_cast<int*>(sh_fpry + ROW);  // linearProgram3 queue: [0] = length, [1 ..] = entries
  unsigned char* un = smem + lds_fixed_bytes(ROW);
  // Column stride of the per-(agent, slot) tiles: ROW = 64 (a shift) in general; for single-env tiles (N > 32) the N
  // columns actually used, which is what lets two 50-agent workgroups share a CU's LDS.
  const int CS = NC ? CS_ROW : k.col_stride;
  // ORCA view of the union
  float4* Lmat = reinterpret_cast<float4*>(un);                                          // [N-1][CS] half-planes
  float2* Rmat = reinterpret_cast<float2*>(Lmat + lds_orca_lines(N, CS));                // [N-1][CS] 1-D optimum on line i
  uint8_t* okmat = reinterpret_cast<uint8_t*>(Rmat + lds_orca_lines(N, CS));             // [N-1][CS] line i feasible
  // sensor view of the union
  // p_orth and the collision gap stay float64 (they decide order / collisions); the sort bucket rint(100 d) is an
  // integer (int32, KEY_NONE = not sensed) and dist_2_other is only emitted as float32: 25 B per pair instead of 33.
  double* omat = reinterpret_cast<double*>(un);          // [N][CS] p_orth
  double* gmat = omat + static_cast<size_t>(N) * CS;     // [N][CS] centre distance - combined radius
  const int has_tti = (p.sort_mode == CA_SORT_TIME_TO_IMPACT) ? 1 : 0;
  double* tmat = gmat + static_cast<size_t>(N) * CS;     // [N][CS] time to impact (time_to_impact sorting only)
  int* kmat = reinterpret_cast<int*>(tmat + static_cast<size_t>(has_tti ? N : 0) * CS);  // [N][CS] sort key
  float* d2mat = reinterpret_cast<float*>(kmat + static_cast<size_t>(N) * CS);           // [N][CS] dist_2_other
  // (one spare byte per pair behind d2mat: the first-pass ranks closest_last's second pass read until round 4)
  float* sh_obs = reinterpret_cast<float*>(un + align16(static_cast<size_t>(CS) * N * ((has_tti ? 3 : 2) * 8 + 9)));

  // ---- load my agent
  Lane r;
  r.px = r.py = r.vx = r.vy = r.heading = r.gx = r.gy = 0.0;
  r.rad = r.ps = 1.0; r.tr = r.t = r.slt = r.epr = 0.0; r.td = 0.0;
  r.act0 = r.act1 = 0.f; r.flags = CA_DONE | CA_AT_GOAL; r.step_num = 0;
  int ep_step = 0, reset_cnt = 0;
  if (active) {
    if (k.s.turning_dir) r.td = k.s.turning_dir[i];
    r.px = k.s.pos_x[i]; r.py = k.s.pos_y[i]; r.vx = k.s.vel_x[i]; r.vy = k.s.vel_y[i];
    r.heading = k.s.heading[i]; r.gx = k.s.goal_x[i]; r.gy = k.s.goal_y[i];
    r.rad = k.s.radius[i]; r.ps = k.s.pref_speed[i]; r.tr = k.s.time_remaining[i]; r.t = k.s.t[i];
    r.slt = k.s.slt[i]; r.epr = k.s.ep_reward[i];
    const float2 la = reinterpret_cast<const float2*>(k.s.last_action)[i];
    r.act0 = la.x; r.act1 = la.y;
    r.flags = k.s.flags[i];
    r.step_num = k.s.step_num[i];
    ep_step = k.s.episode_step[e];
    reset_cnt = k.s.reset_count[e];
  }
  bool statics_dirty = false;  // goal / radius / pref_speed / slt changed (reset, StaticPolicy)
  bool do_sense = active;
  float reward = 0.f;

  if (k.mode == MODE_RESET) {
    do_sense = active && (!k.reset_mask || k.reset_mask[e]);
    if (do_sense) {
      reset_lane(r, k.reset_cases + i * 6, k.reset_headings != nullptr, k.reset_headings ? k.reset_headings[i] : 0.0, p);
      ep_step = 0;
      reset_cnt = 0;
      statics_dirty = true;
    }
  }

  // The phases are straight-line code in the single-step kernel (lambdas inlined at their call sites): with the
  // n-step loop and the two-pass sensing loop around them the register allocator keeps ~100 more VGPRs alive around
  // the back edges (profiles/r01_kernel_geometry.md).  MULTI = true keeps the step loop for cagpu_rollout.
  auto one_step = [&]() {
    // In the n-step kernel, hide the loop invariance of everything derived from the thread id (one laundered copy
    // per iteration): otherwise LICM hoists dozens of per-thread addresses / predicates out of the step loop and
    // the allocator has to keep them alive across it.
    int tid_l = threadIdx.x;
    if (MULTI) asm volatile("" : "+v"(tid_l));
    const int tid = tid_l;
    const bool wave0 = tid < ROW;
    const int lane = tid & (ROW - 1);
    const int le = lane / N, a = lane - le * N;
    const long e = env0 + le;
    const bool active = wave0 && (lane < tile_n) && (e < p.num_envs);
    const int ebase = active ? le * N : 0;
    const long i = e * N + a;
    if (k.mode == MODE_STEP) {
      // ================= A1: who queries ORCA, float bodies (RVOPolicy.py:57-74)
      const uint32_t pol = (r.flags >> CA_POLICY_SHIFT) & 0xF;
      const bool query = active && !(r.flags & CA_DONE);  // env.py:311
      const bool rvo = query && pol == CA_POL_RVO;
      if (wave0) PRIO(3); else PRIO(2);
      if (wave0) {
        ep_step += 1;  // env.py:183
        // (an absent slot of a ragged batch sits at infinity: distSq = inf = "not a neighbour" for everybody)
        sh_fpx[lane] = (p.ragged && (r.flags & CA_ABSENT)) ? INFINITY : static_cast<float>(r.px);
        sh_fpy[lane] = static_cast<float>(r.py);
        sh_fvx[lane] = static_cast<float>(r.vx);
        sh_fvy[lane] = static_cast<float>(r.vy);
        sh_frad[lane] = static_cast<float>((1 + 5e-2) * r.rad);  // RVOPolicy.py:71
        // compact list of the tile's ORCA queries: in steady state ~40 % of the agents are done and wait for their env's
        // game over (EVALUATE_MODE), and pair items dealt over ALL agents would idle in 4 of 10 lanes of every wave
        const unsigned long long qm = __ballot(rvo);
        if (rvo) sh_q[__popcll(qm & ((1ull << lane) - 1ull))] = lane;
        if (lane == 0) {
          sh_q3[0] = 0;
          sh_q3[ROW + 1] = __popcll(qm);
        }
        // RVO draw (CaRvoDraw; the RD instantiations): the ego's collaboration coefficient of this query, handed
        // to the pair lanes through sh_vrx -- free until the 1-D programmes' results land there behind the next two barriers
        if (RD) {
          float cf = static_cast<float>(p.rvo_collab_coeff);
          if (rvo) cf = rvo_collab_draw(k, rvo_addr(k, e, reset_cnt), a, r.step_num, r.t, r.flags);
          sh_vrx[lane] = cf;
        }
      }
      WG_SYNC();
      F2 v_orca = f2(0.f, 0.f);  // this lane's ORCA velocity (agent wave)
      PRIO(2);
      // ================= P2: every (querying agent, other) pair: neighbour rank (ascending distSq, ties by index:
      // Agent::insertAgentNeighbor) + ORCA half-plane
      const float range_sq = sqf(static_cast<float>(p.sensing_horizon));
      const bool unlimited = !(range_sq < INFINITY);
      const float inv_h = divf(1.0f, static_cast<float>(p.rvo_time_horizon));
      const float inv_dt = divf(1.0f, static_cast<float>(p.rvo_dt));  // RVOPolicy.py:13,26
      const float collab = static_cast<float>(p.rvo_collab_coeff);
      const int n_live = sh_q3[ROW + 1];
      // A wave holds WHOLE agents -- floor(64 / (N - 1)) of them, lane = (agent, one of its N - 1 others) -- so a lane
      // gets the other distances of its agent from its neighbour lanes (ds_bpermute: no recomputation, no LDS round
      // trip) and counts its rank.  At N = 10: 7 agents per wave, 28 per round of the workgroup.
      constexpr int NW = NT / 64;
      const int wv = tid >> 6, wl = tid & 63;
      const int GN = NC ? (NC > 1 ? NC - 1 : 1) : (N > 1 ? N - 1 : 1);  // lanes per agent
      const float inv_gn = 1.0f / static_cast<float>(GN);
      const int apw = 64 / GN;     // agents per wave
      const int apr = NW * apw;    // agents per round of the workgroup
      const int g = div_small<(NC > 1 ? NC - 1 : NC)>(wl, inv_gn), jo = wl - __mul24(g, GN);
      const int gbase = (wl - jo) << 2;  // ds_bpermute byte address of the first lane of my agent's group
#pragma unroll
      for (int c0 = 0; c0 < (NC ? tile_n : n_live); c0 += apr) {
        if (c0 >= n_live) continue;  // workgroup-uniform
        const int c = c0 + wv * apw + g;
        const bool valid = (g < apw) && (c < n_live);
        const int ag = sh_q[valid ? c : 0];
        const int eb = __mul24(div_small<NC>(ag, inv_n), N), aa = ag - eb;
        const int j = jo + ((jo >= aa) ? 1 : 0);  // my other agent (index order is kept: ties by index)
        const F2 mpos = f2(sh_fpx[ag], sh_fpy[ag]);
        float dj = INFINITY;
        if (valid && j < N) {
          const F2 d = mpos - f2(sh_fpx[eb + j], sh_fpy[eb + j]);
          dj = dotf(d, d);
          if (!unlimited && !(dj < range_sq)) dj = INFINITY;
        }
        // rank = number of others that are closer (ties by index: they need two floats to be EQUAL -- symmetric starts --
        // and are settled in a second walk by the waves that hold one)
        int rank = 0, cnt = (N > 1) ? N - 1 : 0, tie = 0;
        for_n<8>(GN, [&](const int q) {
          const float dq = __int_as_float(__builtin_amdgcn_ds_bpermute(gbase + 4 * q, __float_as_int(dj)));
          rank += static_cast<int>(dq < dj);
          tie += static_cast<int>(dq == dj);
        });
        if (__any(tie > 1 && dj < INFINITY)) {  // (a distance always equals itself)
          for_n<8>(GN, [&](const int q) {
            const float dq = __int_as_float(__builtin_amdgcn_ds_bpermute(gbase + 4 * q, __float_as_int(dj)));
            rank += static_cast<int>(dq == dj) & static_cast<int>(q < jo);
          });
        }
        if (!unlimited || p.ragged) {  // a finite neighborDist / absent slots: count who is a neighbour
          cnt = 0;
          for_n<8>(GN, [&](const int q) {
            cnt += static_cast<int>(__int_as_float(__builtin_amdgcn_ds_bpermute(gbase + 4 * q, __float_as_int(dj))) < INFINITY);
          });
        }
        // (neighborDist = inf -- Config.SENSING_HORIZON, RVOPolicy.py:27 -- makes every other agent a neighbour)
        const int n = cnt < p.rvo_max_neighbors ? cnt : p.rvo_max_neighbors;
        if (valid) {
          if (jo == 0) sh_nb[ag] = n;
          if (dj < INFINITY && rank < n) {
            // (the ego's own collaboration coefficient where the caller drew one per agent: RVOPolicy.py:77-90)
            const float cf = RD ? sh_vrx[ag] : (k.s.rvo_collab ? k.s.rvo_collab[env0 * N + ag] : collab);
            Lmat[rank * CS + ag] = half_plane_sel(mpos, f2(sh_fvx[ag], sh_fvy[ag]), sh_frad[ag],
                                                   f2(sh_fpx[eb + j], sh_fpy[eb + j]), f2(sh_fvx[eb + j], sh_fvy[eb + j]),
                                                   sh_frad[eb + j], cf, inv_h, inv_dt);
          }
        }
      }
      if (wave0 && rvo) {  // the preferred velocity (float64 sqrt + divide), while the other waves finish the pairs
        const double vx = r.gx - r.px, vy = r.gy - r.py;
        const double sc = divd(r.ps, sqrtd(vx * vx + vy * vy));  // RVOPolicy.py:66-67
        sh_fprx[lane] = static_cast<float>(sc * vx);
        sh_fpry[lane] = static_cast<float>(sc * vy);
        sh_fms[lane] = static_cast<float>(r.ps);
      }
      WG_SYNC();
      if (N > G16) {
        // ================= more than 16 agents per env: one WAVE per querying agent solves the whole programme
        // cooperatively (lane j = line j): linearProgram2 as "first violated line" ballots with the 1-D programme of that
        // line solved by the lanes holding the lines before it, then linearProgram3 if it ends infeasible
        // (cagpu_grouplp.inc; bit-identical to the sequential algorithm).  Solving EVERY line's 1-D programme in advance,
        // as below, is N^3 / 2 intersections per env -- at N = 50 that and its scan took 37 k of the step's 138 k cycles,
        // for 1.3 .. 3 programmes a query really needs.
        const int wq = tid >> 6, jl = tid & 63;
        for (int c = wq; c < n_live; c += NT / 64) {  // wave-uniform
          const int ag = sh_q[c];
          const int nf = sh_nb[ag];
          const float4 ln = Lmat[((jl < nf) ? jl : 0) * CS + ag];
          F2 v;
          const int f2_ = lp2_group<64>(jl < nf, f2(ln.x, ln.y), f2(ln.z, ln.w), sh_fms[ag], f2(sh_fprx[ag], sh_fpry[ag]), false,
                                        v, jl, jl);
          if (f2_ != NOFAIL) lp3_group<64>(nf, f2_, f2(ln.x, ln.y), f2(ln.z, ln.w), sh_fms[ag], v, jl, jl);
          if (jl == 0) { sh_vrx[ag] = v.x; sh_vry[ag] = v.y; }
        }
        WG_SYNC();
        if (wave0 && rvo) v_orca = f2(sh_vrx[lane], sh_vry[lane]);
        if (wave0) PRIO(3); else PRIO(0);
      } else {
        // ================= P2b: linearProgram1 of EVERY line i against the lines before it, one thread per (agent, i).
        // The 1-D optimum on line i depends on the lines [0, i), the speed disc and the preferred velocity only -- not
        // on the running result of linearProgram2 -- so all of them are computed side by side (min / max are exact and
        // a 1-D programme is infeasible iff its final interval is empty), and linearProgram2 itself shrinks to the scan
        // below: per line one violation test and one select.  Bit-identical to the incremental form.
        // Items are line-major (w = i * n_live + c): the lanes of a wave hold (nearly) the same line index i, so the
        // loop over the lines m < i runs to a wave-uniform bound instead of N - 2 for everybody.
        const int n_lp1 = n_live * (N - 1);
        const float inv_live = 1.0f / static_cast<float>(n_live > 0 ? n_live : 1);
        for (int base_ = 0; base_ < n_lp1; base_ += NT) {
          const int w = base_ + tid;
          const bool item = w < n_lp1;
          // highest lines first: a second round (more than NT / (N - 1) queries in the tile) holds the lines with the
          // FEWEST predecessors, i.e. the cheap ones
          const int w_lo = base_ + (tid & ~63);  // the wave's first item holds its highest line
          const int i_hi = __builtin_amdgcn_readfirstlane((N - 2) - static_cast<int>((static_cast<float>(w_lo) + 0.5f) * inv_live));
          const int wq = item ? static_cast<int>((static_cast<float>(w) + 0.5f) * inv_live) : 0;
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
          auto against = [&](const int m) {  // intersect line i with line m (< i)
            const bool use = m < i;
            const float4 lm = Lmat[(use ? m : 0) * CS + ag];
            const F2 Pm = f2(lm.x, lm.y), Dm = f2(lm.z, lm.w);
            const float den = detf(Di, Dm);
            const float num = detf(Dm, Pi - Pm);
            const bool par = fabsf(den) <= kRvoEps;
            ok = ok && !(use && par && num < 0.0f);
            const float tt = divq(num, par ? 1.0f : den);
            const float c_hi = (use && !par && den >= 0.0f) ? tt : INFINITY;
            const float c_lo = (use && !par && den < 0.0f) ? tt : -INFINITY;
            t_hi = (c_hi < t_hi) ? c_hi : t_hi;
            t_lo = (t_lo < c_lo) ? c_lo : t_lo;
          };
          if (base_ + (tid & ~63) < n_lp1) {  // wave-uniform: this wave has items in this round
            // (run-time trip count on purpose: with all N - 2 iterations unrolled and every load hoisted the waves that
            // hold low lines lose more than the others gain: 18.9 -> 19.3 us)
LP1_UNROLL
            for (int m = 0; m < i_hi; ++m) against(m);
          }
          ok = ok && !(t_lo > t_hi);
          const float t = dotf(Di, opt - Pi);
          const float tc = (t < t_lo) ? t_lo : ((t > t_hi) ? t_hi : t);
          const F2 res = Pi + tc * Di;
          if (live) {
            Rmat[i * CS + ag] = make_float2(res.x, res.y);
            okmat[i * CS + ag] = ok ? 1 : 0;
          }
        }
        WG_SYNC();
        // ================= linearProgram2 = a scan over the lines, one lane per agent (agent wave); infeasible
        // programmes (4.6 % of the queries at N = 10) are queued for the cooperative linearProgram3 pass
        int failf = NOFAIL;
        if (wave0) PRIO(3);
        if (wave0 && rvo) {
          const int n = sh_nb[lane];
          const float radius = sh_fms[lane];
          const F2 opt = f2(sh_fprx[lane], sh_fpry[lane]);
          F2 res = opt;
          if (dotf(opt, opt) > sqf(radius)) res = radius * unitq(opt);
          for_n<8>(NC ? NC - 1 : n, [&](const int i) {
            // The loads do not depend on the running result, so all of them can be in flight before the select chain
            // starts -- provided the tests stay branch-free: the conditions are combined as integers (written with &&
            // the compiler guards every load with its own branch + wait, one LDS round trip per line).
            const float4 li = Lmat[i * CS + lane];
            const float2 ri = Rmat[i * CS + lane];
            const int oki = okmat[i * CS + lane];
            const float dt = detf(f2(li.z, li.w), f2(li.x, li.y) - res);
            const int hit = static_cast<int>(i < n) & static_cast<int>(failf == NOFAIL) & static_cast<int>(dt > 0.0f);
            const int take = hit & (oki != 0 ? 1 : 0);
            res.x = take ? ri.x : res.x;
            res.y = take ? ri.y : res.y;
            failf = (hit & (take ^ 1)) ? i : failf;
          });
          v_orca = res;
          if (failf != NOFAIL) {
            sh_vrx[lane] = res.x;
            sh_vry[lane] = res.y;
            sh_q3[1 + atomicAdd(&sh_q3[0], 1)] = lane | (failf << 8) | (n << 16);
          }
        }
        WG_SYNC();
        // ================= linearProgram3 for the queued agents.  N <= 10 (at most 9 lines): one WAVE per agent, all pair
        // intersections of the embedded linearProgram2 in one step (lp3_wave8); otherwise one 16-lane group per agent
        // while N <= 16 (lane j = half-plane j; ballot + DPP row reductions), the whole wave beyond (cagpu_grouplp.inc)
        const int n3 = sh_q3[0];
        if (n3 > 0) {  // workgroup-uniform
          PRIO(3);
          auto solve3 = [&](auto gs_tag) {
            constexpr int GS = decltype(gs_tag)::value;
            constexpr int GROUPS = NT / GS;
            // queue entry k goes to wave k % (number of waves) first: infeasible agents are solved side by side
            const int jl = tid & (GS - 1), g = tid / GS;
            constexpr int GPW = 64 / GS;  // groups per wave
            for (int q3 = (g % GPW) * (NT / 64) + (g / GPW); q3 < n3; q3 += GROUPS) {
              const int ent = sh_q3[1 + q3], agf = ent & 0xFF, ff = (ent >> 8) & 0xFF;
              const int nf = sh_nb[agf];
              const float4 ln = Lmat[((jl < nf) ? jl : 0) * CS + agf];
              F2 v = f2(sh_vrx[agf], sh_vry[agf]);
              lp3_group<GS>(nf, ff, f2(ln.x, ln.y), f2(ln.z, ln.w), sh_fms[agf], v, jl, tid & 63);
              if (jl == 0) { sh_vrx[agf] = v.x; sh_vry[agf] = v.y; }
            }
          };
          if (N <= 10) {
            const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            for (int q3 = wv; q3 < n3; q3 += NT / 64) {
              const int ent = sh_q3[1 + q3], agf = ent & 0xFF, ff = (ent >> 8) & 0xFF;  // (bits 16 ..: the line count)
              F2 v = f2(sh_vrx[agf], sh_vry[agf]);
              lp3_wave8(Lmat + agf, CS, (ent >> 16) & 0xFF, ff, sh_fms[agf], v, tid & 63);
              if ((tid & 63) == 0) { sh_vrx[agf] = v.x; sh_vry[agf] = v.y; }
            }
          } else if (N <= G16) {
            solve3(std::integral_constant<int, 16>{});
          } else {
            solve3(std::integral_constant<int, 64>{});
          }
          WG_SYNC();
          if (failf != NOFAIL) v_orca = f2(sh_vrx[lane], sh_vry[lane]);
          if (wave0) PRIO(3); else PRIO(0);
        }
      }
      // ================= A2c: policy post-processing (env.py:305-323) and move (agent.py:192-241), one lane per agent
      if (wave0) {
        double spd = 0.0, dh = 0.0;
        if (query) {
          if (pol == CA_POL_RVO) {
            const float ts = static_cast<float>(p.rvo_dt);
            rvo_action(sh_fpx[lane], sh_fpy[lane], v_orca, ts, r.px, r.py, r.heading, k.inv_rvo_dt, spd, dh);
            if (k.s.rvo_heading_noise) dh = dh + k.s.rvo_heading_noise[i];  // RVOPolicy.py:118-119 (drawn by the caller)
            if (RD && k.rd_mask) dh = dh + rvo_heading_noise(k, rvo_addr(k, e, reset_cnt), a, r.step_num, i);  // (drawn here)
          } else if (pol == CA_POL_NONCOOP) {  // NonCooperativePolicy.py:21
            const Ego eg = ego_frame(r.px, r.py, r.gx, r.gy, r.heading);
            spd = r.ps;
            dh = -eg.heading_ego;
          } else if (pol == CA_POL_STATIC) {  // StaticPolicy.py:21-23
            r.gx = r.px;
            r.gy = r.py;
            statics_dirty = true;
          } else if (k.ext) {
            // (this step's slot of an action tape: a kernel argument times the loop counter, uniform; stride 0 without one)
            const double* const ex = MULTI ? k.ext + step * k.ext_stride : k.ext;
            ext_policy_action(pol, ex[2 * i], ex[2 * i + 1], r.ps, p.max_heading_change, spd, dh);
          }
        }
        const float a0f = static_cast<float>(spd), a1f = static_cast<float>(dh);  // float32 `all_actions`
        if (active && k.o.actions) reinterpret_cast<float2*>(k.o.actions)[i + ring_a] = make_float2(a0f, a1f);
        if (active && k.o.orca_vel)  // parity hook: the velocity rvo2 chose for this agent (RVOPolicy.py:93), 0 if not queried
          reinterpret_cast<float2*>(k.o.orca_vel)[i + ring_a] = rvo ? make_float2(v_orca.x, v_orca.y) : make_float2(0.f, 0.f);
        // trajectory tape (CaTraj): who moves (move_lane's done gate) is known before the move, and the row's clock is the one
        // BEFORE its increment: stored here, so that nothing but one predicate lives across the move for the rest of the row
        const bool moved = active && !(r.flags & (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION));
        if (k.traj_rows && moved) k.traj_rows[(i + traj_a) * 12] = r.t;
        if (active) move_lane(r, a0f, a1f, p, k.s.ext_state, i);
        if (k.traj_rows && active) {  // trajectory tape (CaTraj): after the move, before any auto-reset of this step
          double* row = k.traj_rows + (i + traj_a) * 12;
          if (moved) traj_store_tail(row, r.px, r.py, r.gx, r.gy, r.rad, r.ps, r.vx, r.vy, r.act0, r.heading, r.step_num - 1);
          else row[11] = -1.0;
          if (a == 0 && k.traj_ep) k.traj_ep[e + traj_e] = reset_cnt;
        }
      }
      do_sense = active;
    }

    // ================= sensing passes: once, and a second time for envs that auto-reset in this step
    auto sense_pass = [&](const int pass) -> int {
      // ---- A: publish the post-move tile + ego frames (agent.py:329-349, Dynamics.py:24-41)
      Ego eg;
      eg.dist = 0.0; eg.prx = eg.pry = eg.orx = eg.ory = eg.heading_ego = 0.0;
      if (wave0) {
        sh_px[lane] = r.px; sh_py[lane] = r.py; sh_vx[lane] = r.vx; sh_vy[lane] = r.vy; sh_rad[lane] = r.rad;
        if (do_sense) {
          eg = ego_frame(r.px, r.py, r.gx, r.gy, r.heading);
          sh_prx[lane] = eg.prx;
          sh_pry[lane] = eg.pry;
        }
        sh_sense[lane] = do_sense ? 1 : 0;
        if (RO) sh_q[lane] = 0;  // reused below: case index + 1 of an env that auto-resets in this step
      }
      WG_SYNC();

      // ---- P3: every (agent, other) pair: centre distance -> collision gap, sensor key, p_orth
      //      (env.py:458-512; OtherAgentsStatesSensor.py:76-107)
      PRIO(1);
      if (NC != 0 && p.sort_mode != CA_SORT_TIME_TO_IMPACT) {
        // N compiled in: one item per UNORDERED pair {a, b} -- the float64 square root, the collision gap and the
        // horizon test are the same for both directions; only d - r_host - r_other (operand order) and p_orth (the
        // host's frame) are direction-specific.  Per env: the pairs (a, a + s mod N) for s = 1 .. (N-1)/2, for even N
        // the N/2 antipodal pairs, then N self entries: N (N + 1) / 2 items, 220 per 4-env tile = ONE round of 256.
        constexpr int NN = NC ? NC : 2, HALF = (NN - 1) / 2, PE = NN * (NN + 1) / 2;
        const int n_un = tile_envs * PE;
#pragma unroll
        FOR_ITEMS_UPTO(w, n_un) {
          const int le2 = div_small<PE>(w, 1.0f / static_cast<float>(PE));
          const int u = w - __mul24(le2, PE), eb = __mul24(le2, NN);
          if (!sh_sense[eb]) continue;  // sensing is decided per env
          if (u >= PE - NN) {  // self entry: never sensed, no gap
            const int a1 = u - (PE - NN);
            kmat[a1 * CS + eb + a1] = KEY_NONE;
            omat[a1 * CS + eb + a1] = 0.0;
            d2mat[a1 * CS + eb + a1] = 0.f;
            gmat[a1 * CS + eb + a1] = INFINITY;
            continue;
          }
          int a1, b1;
          if (u < NN * HALF) {
            const int sft = div_small<NN>(u, 1.0f / static_cast<float>(NN));
            a1 = u - __mul24(sft, NN);
            b1 = a1 + sft + 1;
            b1 -= (b1 >= NN) ? NN : 0;
          } else {
            a1 = u - NN * HALF;
            b1 = a1 + NN / 2;
          }
          const int ga = eb + a1, gb = eb + b1;
          const double ax = sh_px[ga], ay = sh_py[ga], ar = sh_rad[ga];
          const double bx = sh_px[gb], by = sh_py[gb], br = sh_rad[gb];
          const double rx = bx - ax, ry = by - ay;  // other - host for host a; exactly negated for host b
          const double d = sqrtd(rx * rx + ry * ry);
          int key_ab = KEY_NONE, key_ba = KEY_NONE;
          double po_ab = 0.0, po_ba = 0.0, d2_ab = 0.0, d2_ba = 0.0;
          const bool both = !p.ragged || (ar > 0.0 && br > 0.0);  // (an absent slot of a ragged batch has radius 0)
          if (both && !(d > p.sensing_horizon)) {
            d2_ab = d - ar - br;
            d2_ba = d - br - ar;
            // numpy scalar round(x, 2) bucket; ordering of k == ordering of k/100 (an integer: exact as int32)
            key_ab = static_cast<int>(fmin(fmax(rint(d2_ab * 100.0), -2.0e9), 2.0e9));
            key_ba = static_cast<int>(fmin(fmax(rint(d2_ba * 100.0), -2.0e9), 2.0e9));
            po_ab = rx * (-sh_pry[ga]) + ry * sh_prx[ga];
            po_ba = (-rx) * (-sh_pry[gb]) + (-ry) * sh_prx[gb];
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
      } else {
#pragma unroll
      FOR_PAIR_ITEMS(w) {
        const int ag = div_small<NC>(w, inv_n);
        const int j = w - __mul24(ag, N);
        if (!sh_sense[ag]) continue;
        const int eb = __mul24(div_small<NC>(ag, inv_n), N), aa = ag - eb;
        int key = KEY_NONE;
        double po = 0.0, d2o = 0.0, gap = INFINITY;
        if (j != aa) {
          const double hx = sh_px[ag], hy = sh_py[ag], hr = sh_rad[ag];
          const double ox = sh_px[eb + j], oy = sh_py[eb + j], orad = sh_rad[eb + j];
          const double rx = ox - hx, ry = oy - hy;
          const double d = sqrtd(rx * rx + ry * ry);
          const bool both = !p.ragged || (hr > 0.0 && orad > 0.0);  // (an absent slot of a ragged batch has radius 0)
          if (both) gap = d - (hr + orad);
          if (both && !(d > p.sensing_horizon)) {
            d2o = d - hr - orad;
            // numpy scalar round(x, 2) bucket; ordering of k == ordering of k/100 (an integer: exact as int32)
            key = static_cast<int>(fmin(fmax(rint(d2o * 100.0), -2.0e9), 2.0e9));
            po = rx * (-sh_pry[ag]) + ry * sh_prx[ag];
            if (p.sort_mode == CA_SORT_TIME_TO_IMPACT)  // sensor :96-104
              tmat[j * CS + ag] = time_to_impact(hx, hy, ox, oy, sh_vx[ag], sh_vy[ag], sh_vx[eb + j], sh_vy[eb + j],
                                                  hr + orad);
          }
        }
        kmat[j * CS + ag] = key;
        omat[j * CS + ag] = po;
        d2mat[j * CS + ag] = static_cast<float>(d2o);
        gmat[j * CS + ag] = gap;
      }
      }
      WG_SYNC();

      // ---- P4: rank the candidates of every agent and emit its rows (OtherAgentsStatesSensor.py:20-55,109-143)
      PRIO(0);
#pragma unroll
      FOR_PAIR_ITEMS(w) {
        const int ag = div_small<NC>(w, inv_n);
        const int j = w - __mul24(ag, N);
        if (!sh_sense[ag]) continue;
        const int eb = __mul24(div_small<NC>(ag, inv_n), N), aa = ag - eb;
        const int kj = kmat[j * CS + ag];
        const double oj = omat[j * CS + ag];
        int rank = 0, cnt = 0, lt = 0, same = 0;  // lt / same: candidates in closer buckets / in this one (itself included)
        if (p.sort_mode == CA_SORT_TIME_TO_IMPACT) {  // key (-tti, -dist, p_orth), sensor :36-38
          const bool vj = kj != KEY_NONE;
          const double tj = vj ? tmat[j * CS + ag] : 0.0;
          for_n<8>(N, [&](const int q) {
            const int kq = kmat[q * CS + ag];
            const double oq = omat[q * CS + ag];
            const bool vq = kq != KEY_NONE;
            const double tq = vq ? tmat[q * CS + ag] : 0.0;
            const int lo = static_cast<int>(oq < oj) | (static_cast<int>(oq == oj) & static_cast<int>(q < j));
            const int lk = static_cast<int>(kq > kj) | (static_cast<int>(kq == kj) & lo);
            const int before = static_cast<int>(tq > tj) | (static_cast<int>(tq == tj) & lk);
            rank += static_cast<int>(vq) & static_cast<int>(vj) & before;
            cnt += static_cast<int>(vq);
          });
        } else {
          // Pass 1 ranks by the distance bucket alone (one 4-byte key per candidate, branch-free) and notes WHICH candidates
          // share this one's 1 cm bucket.  The (p_orth, index) tie-break -- an 8-byte load and two float64 compares -- then
          // visits only those: a lane pops the set bits of its own mask, the wave loops while any lane has one left (one or
          // two trips).  Walking all N candidates again whenever some lane of the wave held a tie -- in a dense crowd
          // always -- was the larger half of this phase at N = 50.
          // (the mask is gathered eight candidates at a time as m8 = 2 m8 + (kq == kj): a compare and an add-with-carry per
          // candidate like the rank itself, bit-reversed and shifted into place once per block -- a 64-bit shift by a
          // run-time q per candidate doubled the cost of this loop at N = 50)
          unsigned long long eq = 0ull;
          {
            int q0 = 0;
            for (; q0 + 8 <= N; q0 += 8) {
              unsigned m8 = 0u;
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int kq = kmat[(q0 + u) * CS + ag];
                rank += static_cast<int>(kq < kj);
                m8 = m8 + m8 + static_cast<unsigned>(kq == kj);
              }
              eq |= static_cast<unsigned long long>(__brev(m8) >> 24) << q0;  // (candidate q0 + u sits at bit 7 - u of m8)
            }
#pragma unroll
            for (int u = 0; u < 7; ++u)
              if (q0 + u < N) {
                const int kq = kmat[(q0 + u) * CS + ag];
                rank += static_cast<int>(kq < kj);
                eq |= (kq == kj) ? (1ull << (q0 + u)) : 0ull;
              }
          }
          same = __popcll(eq);  // (a key always equals itself)
          lt = rank;
          eq &= ~(1ull << j);
          if (kj == KEY_NONE) eq = 0ull;  // (not a candidate: its rank is never used)
          while (__any(eq != 0ull)) {
            if (eq != 0ull) {
              const int q = __ffsll(static_cast<long long>(eq)) - 1;
              eq &= eq - 1ull;
              const double oq = omat[q * CS + ag];
              rank += static_cast<int>(oq < oj) | (static_cast<int>(oq == oj) & static_cast<int>(q < j));
            }
          }
          if (p.sensing_horizon < INFINITY || p.ragged) {
            for_n<8>(N, [&](const int q) { cnt += static_cast<int>(kmat[q * CS + ag] != KEY_NONE); });
          } else {
            cnt = N - 1;  // every other agent of the env is sensed
          }
        }
        const int keep = cnt < p.obs_clip ? cnt : p.obs_clip;  // sensor :39
        float* row = (STAGE ? sh_obs : obs_tile) + __mul24(ag, W);
        if (j == aa) row[1] = static_cast<float>(keep);  // num_other_agents_observed
        for (int sl = j; sl < K; sl += N)                // zero the unfilled rows (sensor :112)
          if (sl >= keep) {
            float* z = row + 6 + 7 * sl;
            z[0] = z[1] = z[2] = z[3] = z[4] = z[5] = z[6] = 0.f;
          }
        const bool kept = (j != aa) && (kj != KEY_NONE) && (rank < keep);
        if (!kept) continue;
        // closest_last re-sorts the KEPT ones by (-key, p_orth), stable (sensor :41-43): the buckets in reverse, the order
        // inside a bucket as in the first pass.  No second ranking pass is needed for that: the kept ones of farther buckets
        // are keep - (closer ones, all kept) - (this bucket's kept ones = min(same, keep - lt)), and the place inside the
        // bucket is rank - lt.
        int slot = rank;
        if (p.sort_mode == CA_SORT_CLOSEST_LAST) {
          const int room = keep - lt;
          slot = room - (same < room ? same : room) + (rank - lt);
        }
        const double hx = sh_px[ag], hy = sh_py[ag], hr = sh_rad[ag], prx = sh_prx[ag], pry = sh_pry[ag];
        const double ox = sh_px[eb + j], oy = sh_py[eb + j], orad = sh_rad[eb + j];
        const double ovx = sh_vx[eb + j], ovy = sh_vy[eb + j];
        const double rx = ox - hx, ry = oy - hy;
        float* o7 = row + 6 + 7 * slot;
        o7[0] = static_cast<float>(rx * prx + ry * pry);
        o7[1] = static_cast<float>(rx * (-pry) + ry * prx);
        o7[2] = static_cast<float>(ovx * prx + ovy * pry);
        o7[3] = static_cast<float>(ovx * (-pry) + ovy * prx);
        o7[4] = static_cast<float>(orad);
        o7[5] = static_cast<float>(hr + orad);
        o7[6] = d2mat[j * CS + ag];
      }
      // ---- A3 (wave 0, while the other waves finish the pair items of P4): rewards + collision flag (env.py:394-456),
      // observation scalars
      if (wave0) PRIO(3);
      // a map set (the single-step kernel and the n-step form's MSET instantiations; workgroup-uniform test): the env's
      // grid, its index read by the env's agent 0 lane and handed to the others -- the wall tests of this step see the map
      // the env had when the step began (in an n-step launch: what the same lane stored at the last step's auto-reset)
      const uint32_t* wall_bits = nullptr;
      const bool wall_set = (!MULTI || MSET) && k.env_map != nullptr && k.mode == MODE_STEP && pass == 0;
      if (wall_set && wave0) {
        int m = (active && a == 0) ? k.env_map[e] : 0;
        m = __shfl(m, ebase);
        wall_bits = active ? set_grid(k.map.static_bits, k.map_words, k.num_maps, m, a == 0) : nullptr;
      }
      if (wave0 && active) {
        if (k.mode == MODE_STEP && pass == 0) {
          double nearest = INFINITY;
          for_n<8>(N, [&](const int j) {
            const double g = gmat[j * CS + lane];
            nearest = (g < nearest) ? g : nearest;
          });
          const bool coll = nearest <= 0.0;  // some d <= r_i + r_j  <=>  min(d - (r_i + r_j)) <= 0
          double rw = p.reward_time_step;
          if (r.flags & CA_AT_GOAL) {
            if (!(r.flags & CA_WAS_AT_GOAL)) rw = p.reward_at_goal;
          } else if (!(r.flags & CA_WAS_IN_COLLISION)) {
            if (coll) {
              rw = p.reward_collision;
              r.flags |= CA_IN_COLLISION;
            } else if (wall_set ? hits_wall_in(k.map, wall_bits, r.px, r.py, r.rad)
                                : hits_wall(k.map, r.px, r.py, r.rad)) {  // env.py:425-429, :494-506
              rw = p.reward_collision_wall;
              r.flags |= CA_IN_COLLISION;
            } else {
              if (nearest <= p.getting_close_range) rw = -0.1 - nearest / 2.0;
              if (fabs(static_cast<double>(r.act1)) > p.wiggly_threshold) rw += p.reward_wiggly;
            }
          }
          rw = fmin(fmax(rw, p.reward_min), p.reward_max);
          if (p.ragged && (r.flags & CA_ABSENT)) rw = 0.0;  // no agent in this slot: the zero padding of wrappers.py:143-173
          r.epr += rw;
          reward = static_cast<float>(rw);
          const bool d = (r.flags & (CA_AT_GOAL | CA_OUT_OF_TIME | CA_IN_COLLISION)) != 0;
          if (d) r.flags |= CA_DONE; else r.flags &= ~static_cast<uint32_t>(CA_DONE);
          sh_flag[lane] = r.flags;
          sh_r0[lane] = r.epr;
          sh_r1[lane] = r.t;
          sh_r2[lane] = r.t - r.slt;
        }
        if (do_sense) {
          float* row = (STAGE ? sh_obs : obs_tile) + __mul24(lane, W);
          obs_own_columns(row, !(p.ragged && (r.flags & CA_ABSENT)), r.flags, eg.dist, eg.heading_ego, r.ps, r.rad);
        }
      }

      // No workgroup barrier here: A4 reads what A3 wrote (flags, episode scratch), and both run on the agent wave --
      // a wave-level fence is enough, and A4 overlaps with the other waves' second round of P4 instead of following it.
      if (wave0) wave_sync();

      // ---- A4 (wave 0): done / game over (env.py:514-553), auto-reset (vec_env.py:120-128), episode statistics
      bool need_second = false;
      if (k.mode == MODE_STEP && pass == 0) {
        do_sense = false;
        if (wave0 && active) {
          // AND / OR of the env's flag words, then bit tests: no short-circuit chains (they compile to one dependent
          // LDS round trip + branch per agent)
          uint32_t f_and = ~0u, f_or = 0u, learn_and = ~0u;  // (FlagFold of cagpu_rules.inc, in this kernel's own text)
          for_n<8>(N, [&](const int j) {
            const uint32_t f = sh_flag[ebase + j];
            f_and &= f;
            f_or |= f;
            learn_and &= (f & CA_STILL_LEARNING) ? f : ~0u;  // learners only
          });
          const bool all_done = (f_and & CA_DONE) != 0, all_learning_done = (learn_and & CA_DONE) != 0;
          const bool any_coll = (f_or & CA_IN_COLLISION) != 0, all_goal = (f_and & CA_AT_GOAL) != 0;
          bool over = all_done;
          if (p.game_over_mode == CA_OVER_AGENT0) over = (sh_flag[ebase] & CA_DONE) != 0;
          else if (p.game_over_mode == CA_OVER_LEARNING_DONE) over = all_learning_done;
          k.o.rewards[i + ring_a] = reward;
          k.o.done[i + ring_a] = static_cast<uint8_t>((r.flags & CA_DONE) != 0);
          if (a == 0) k.o.game_over[e + ring_e] = static_cast<uint8_t>(over);
          if (over && k.table) {
            if (a == 0) {  // experiments/src/env_utils.py:56-87 reduced to counters, summed in agent order
              double tot_r = 0.0, ttg = 0.0, extra = 0.0;
              for_n<8>(N, [&](const int j) {  // (summed in agent order)
                tot_r += sh_r0[ebase + j];
                ttg += sh_r1[ebase + j];
                extra += sh_r2[ebase + j];
              });
              env_stats_add(k.s.env_stats + 8 * e, any_coll, all_goal, ep_step, tot_r, ttg, extra);
            }
            reset_cnt += 1;
            const long c = reset_case(k, e, reset_cnt);
            const double h0 = reset_heading(k, e, reset_cnt, a);
            if (k.fin_flags) k.fin_flags[i + ring_a] = r.flags;  // final record (CaFinal): the terminal step's flag word
            // episode log (CaEpLog): the three addends of this lane, its flag word and -- agent 0 -- the episode's head
            if (k.log_rows)
              eplog_store(k.log_rows, k.log_head, k.log_cap, e, static_cast<int>(c), k.log_case_step, k.n_cases, N, a,
                          reset_cnt - 1, sh_r0[lane], sh_r1[lane], sh_r2[lane], r.flags, ep_step, any_coll, all_goal);
            reset_lane(r, k.table + (c * N + a) * 6, k.heading_seed != 0, h0, p);
            if (k.draw_cdf) {  // policy draw (CaPolicyDraw; a uniform test): the new episode's policy bits of this slot
              const double* rad = k.table + c * N * 6 + 5;
              r.flags = policy_draw_word(k.draw_cdf, k.draw_bits, k.draw_n, k.draw_ensure, k.draw_seed, k.env_id_offset + e,
                                         reset_cnt, a, N, [&](const int j) { return !p.ragged || rad[j * 6] > 0.0; }, r.flags);
              if (RO) sh_flag[lane] = r.flags;  // (the copy of the reset observation takes is_learning from here)
            }
            if (RD && k.rd_c < 0.0) r.flags &= ~static_cast<uint32_t>(CA_RVO_NONCOOP);  // RVO draw: a new episode starts without the bit
            // a map set with a key: the env's next map (CaMapSet.map_seed), one plain store by its agent 0 lane
            if ((!MULTI || MSET) && k.map_seed && a == 0) k.env_map[e] = map_draw(k.map_seed, k.env_id_offset + e, reset_cnt, k.num_maps);
            ep_step = 0;
            statics_dirty = true;
            if (RO) {
              if (a == 0) sh_q[lane] = static_cast<int>(c) + 1;  // the env's new case, at its first agent's slot
            } else {
              do_sense = true;
            }
            need_second = true;
          }
        }
      }
      const int again = __syncthreads_or(need_second ? 1 : 0);
      // final record (CaFinal; workgroup-uniform tests): the terminal rows of the envs that reset, from where P4 / A3 left
      // them (LDS when staged, else read back from the output rows: every wave's stores to them are drained first)
      float* fin_tile = nullptr;
      if (again && k.fin_obs) {
        fin_tile = k.fin_obs + (obs_tile - k.o.obs);
        if (!STAGE) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      if (RO && again) {
        __syncthreads();  // (full fence: the copy below overwrites observation rows other threads stored in P4)
        // ---- RO: the observation of a freshly reset env is a pure function of its fixture case: it was computed once
        // (cagpu_reset on the whole table) and is copied here, instead of a second sensing pass for the tile
        for (int le2 = 0; le2 < tile_envs; ++le2) {  // workgroup-uniform: at most a few envs of a tile reset per step
          const int c1 = sh_q[le2 * N];
          if (!c1) continue;
          const float* src = k.reset_obs + static_cast<long>(c1 - 1) * N * W;
          const int base = le2 * N * W;
          for (int q = tid; q < N * W; q += NT) {
            const int a2 = q / W, col = q - a2 * W;
            float v = src[q];
            if (col == 0)  // (is_learning comes from the live flags; the row of an absent slot is all zeros: radius 0)
              v = ((sh_flag[le2 * N + a2] & CA_IS_LEARNING) && !(p.ragged && !(src[q + 5] > 0.f))) ? 1.f : 0.f;
            if (fin_tile) fin_tile[base + q] = STAGE ? sh_obs[base + q] : obs_tile[base + q];  // (same thread, same element)
            if (STAGE) sh_obs[base + q] = v;
            else obs_tile[base + q] = v;
          }
        }
        WG_SYNC();
      }
      if (RO || !again) {
        // ---- the tile's observation block leaves LDS as one contiguous, coalesced copy
        if (STAGE) {
          const long total = tile_cnt * W;
          float* dst = obs_tile;
          if (k.mode == MODE_RESET && k.reset_mask) {
            for (long q = tid; q < total; q += NT) {
              const long ee = env0 + (q / W) / N;
              if (k.reset_mask[ee]) dst[q] = sh_obs[q];
            }
          } else if (((tile_base * W) & 3) == 0 && (total & 3) == 0) {
            const float4* src4 = reinterpret_cast<const float4*>(sh_obs);
            float4* dst4 = reinterpret_cast<float4*>(dst);
            for (long q = tid; q < (total >> 2); q += NT) dst4[q] = src4[q];
          } else {
            for (long q = tid; q < total; q += NT) dst[q] = sh_obs[q];
          }
        }
        return 0;
      }
      if (fin_tile) {
        // (no reset observations to copy: the second pass below overwrites the rows of the envs that reset -- every agent
        // lane of such an env saves its own row first; the rare path: random headings, or a table without reset_obs)
        __syncthreads();
        if (wave0 && need_second) {
          const float* src = (STAGE ? sh_obs : obs_tile) + __mul24(lane, W);
          float* dst = fin_tile + __mul24(lane, W);
          for (int q = 0; q < W; ++q) dst[q] = src[q];
        }
      }
      return 1;  // some env of the tile auto-reset: run the sensing pass once more for it
    };
    if (RO) {
      sense_pass(0);
    } else if (sense_pass(0)) {
      sense_pass(1);
    }
    if (MULTI) WG_SYNC();  // the union is free again before the next step's ORCA view (n-step kernel only)
  };
  if (MULTI) {
    const int n_steps = (k.mode == MODE_STEP) ? k.n_steps : 1;
    for (step = 0; step < n_steps; ++step) {
      one_step();
      obs_tile += k.ring_obs;  // (0 unless the caller keeps every step's outputs: cagpu_rollout_ring)
      ring_a += k.ring_agent;
      ring_e += k.ring_env;
      traj_a += static_cast<long>(p.num_envs) * N;
      traj_e += p.num_envs;
    }
  } else {
    one_step();
  }

  // ---- store my agent.  The pointers are re-read from the kernarg segment here (laundered so the compiler does
  // not keep 19 pointer pairs alive in SGPRs across the whole kernel).
  if (active && k.mode != MODE_OBSERVE && (k.mode == MODE_STEP || !k.reset_mask || k.reset_mask[e])) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(4))) const KArgs ConstKArgs;
    ConstKArgs* ka = (ConstKArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
#else
    const KArgs* ka = &k;
#endif
    ka->s.pos_x[i] = r.px; ka->s.pos_y[i] = r.py; ka->s.vel_x[i] = r.vx; ka->s.vel_y[i] = r.vy;
    ka->s.heading[i] = r.heading; ka->s.time_remaining[i] = r.tr; ka->s.t[i] = r.t;
    ka->s.ep_reward[i] = r.epr;
    if (ka->s.turning_dir) ka->s.turning_dir[i] = r.td;
    if (statics_dirty) {
      ka->s.goal_x[i] = r.gx; ka->s.goal_y[i] = r.gy;
      ka->s.radius[i] = r.rad; ka->s.pref_speed[i] = r.ps; ka->s.slt[i] = r.slt;
    }
    reinterpret_cast<float2*>(ka->s.last_action)[i] = make_float2(r.act0, r.act1);
    ka->s.flags[i] = r.flags & ~static_cast<uint32_t>(CA_PLAN_VALID);  // (this kernel leaves no plan for the next step)
    ka->s.step_num[i] = r.step_num;
    if (a == 0) { ka->s.episode_step[e] = ep_step; ka->s.reset_count[e] = reset_cnt; }
  }
  // (Round 6, measured and dropped: the list of the agents the NEXT network query evaluates, packed here by every tile -- one
  //  epoch-tagged device-scope atomic per tile for its range + one arrival ticket -- so that cagpu_ga3c could skip its packing
  //  launch (6.9 us of a 143 us config-3 step).  1 366 tiles x 2 same-address atomics cost ~43 ns each, serialised: the step
  //  kernel went 34 -> 129 us (config 3: 146 -> 241 us per step, same box).  compact_kernel does the same with 80 workgroups.)
}

#include "cagpu_pipe.inc"
#include "cagpu_big.inc"

// ---------------------------------------------------------------- stand-alone ORCA (rvo2 doStep replacement)
struct OrcaArgs {
  int32_t num_envs, num_agents, max_nb;
  const float *pos, *vel, *pref, *radius, *max_speed;
  float collab, time_horizon, time_step, neighbor_dist;
  float* new_vel;
};

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void orca_kernel(const OrcaArgs k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = k.num_agents;
  const int tile_envs = BLOCK / N, tile_n = tile_envs * N;
  const int lane = threadIdx.x;
  const int le = lane / N, a = lane - le * N, ebase = le * N;
  const long e = static_cast<long>(blockIdx.x) * tile_envs + le;
  const bool active = lane < tile_n && e < k.num_envs;
  const long i = e * N + a;
  float* sh_fpx = reinterpret_cast<float*>(smem);
  float* sh_fpy = sh_fpx + BLOCK;
  float* sh_fvx = sh_fpy + BLOCK;
  float* sh_fvy = sh_fvx + BLOCK;
  float* sh_frad = sh_fvy + BLOCK;
  unsigned char* un = smem + static_cast<size_t>(BLOCK) * 5 * 4;
  float* dcol = reinterpret_cast<float*>(un) + lane;
  float4* Lcol = reinterpret_cast<float4*>(un + static_cast<size_t>(BLOCK) * N * 4) + lane;
  float4* Pcol = Lcol + static_cast<size_t>(N > 1 ? N - 1 : 1) * BLOCK;
  F2 pref = f2(0.f, 0.f);
  float ms = 0.f;
  if (active) {
    const float2 ps = reinterpret_cast<const float2*>(k.pos)[i], vl = reinterpret_cast<const float2*>(k.vel)[i];
    const float2 pf = reinterpret_cast<const float2*>(k.pref)[i];
    sh_fpx[lane] = ps.x; sh_fpy[lane] = ps.y; sh_fvx[lane] = vl.x; sh_fvy[lane] = vl.y;
    sh_frad[lane] = k.radius[i];
    pref = f2(pf.x, pf.y);
    ms = k.max_speed[i];
  }
  __syncthreads();
  if (active) {
    const F2 v = orca_velocity<BLOCK>(sh_fpx, sh_fpy, sh_fvx, sh_fvy, sh_frad, ebase, a, N, pref, ms, k.collab,
                                      k.time_horizon, k.time_step, k.neighbor_dist, k.max_nb, dcol, Lcol, Pcol);
    reinterpret_cast<float2*>(k.new_vel)[i] = make_float2(v.x, v.y);
  }
}

// ---------------------------------------------------------------- parity hook: the device's own libm-dependent operations
// (cagpu_debug_libm).  The step's results differ from a CPU run of the same algorithm only through these: atan2 (ROCm's
// ocml, vs glibc's on the host), the heading's sin / cos (sincos_heading above, a short-range kernel) and the lean
// divide / square root sequences (divq / sqrtq / divd / sqrtd above).
__global__ void debug_libm_kernel(const int n, const int op, const double* a, const double* b, double* o0, double* o1) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = a[i], y = b ? b[i] : 0.0;
  double r0 = 0.0, r1 = 0.0;
  switch (op) {
    case 0: r0 = atan2(x, y); break;                                   // atan2(a, b)
    case 1: sincos_heading(x, r0, r1); break;                          // (sin a, cos a), a in [-pi, pi]
    case 2: r0 = divq(static_cast<float>(x), static_cast<float>(y)); r1 = static_cast<float>(x) / static_cast<float>(y); break;
    case 3: r0 = sqrtq(static_cast<float>(x)); r1 = sqrtf(static_cast<float>(x)); break;
    case 4: r0 = divd(x, y); r1 = x / y; break;
    case 5: r0 = sqrtd(x); r1 = sqrt(x); break;
    case 6: { const Ego e = ego_frame(0.0, 0.0, x, y, 0.0); r0 = e.heading_ego; r1 = e.dist; } break;  // goal (a, b) seen from the origin
    default: break;
  }
  o0[i] = r0;
  if (o1) o1[i] = r1;
}

// cagpu_debug_copy8: a streaming copy with the step kernels' 8-bytes-per-lane access shape (counter calibration)
__global__ __launch_bounds__(256) void copy8_kernel(const long n, const double* __restrict__ src, double* __restrict__ dst) {
  const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// ---------------------------------------------------------------- host side: no device code below this line
#include "cagpu_launch.inc"  // which geometry and instantiation a call runs, the checked launch, the LDS-limit rule

}  // namespace

#include "cagpu_api.inc"  // the extern "C" entry points of include/cagpu.h
