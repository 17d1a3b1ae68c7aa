// gym_collision_avoidance_amd/csrc/cagpu_scan.inc -- included by cagpu.hip (inside its anonymous namespace).
//
// Static map + LaserScanSensor (reference Map.py, sensors/LaserScanSensor.py).  One workgroup per env:
//   1. the env's occupancy grid is assembled in LDS as a bitmap (160 x 160 cells = 3.2 KB): the static grid is copied
//      from HBM (bit-packed), every agent is OR-ed in as a disc around its floored cell (Map.py:46-64);
//   2. every (agent, beam) marches its samples through the LDS bitmap -- the agent's own disc is tested analytically
//      instead of building an ego mask (LaserScanSensor.py:74-77);
//   3. the beam's range index goes into the history (uint8, rolled like np.roll) and out as float32 metres.
// Cell indices must be the reference's float64 `floor(origin -+ coord / cell)`.  Along a beam the grid coordinate is
// affine in the sample index, so one FMA per coordinate gives it to ~1e-13; the reference's own expression (with a
// guarded reciprocal, cell_index) is evaluated only for samples within 1e-9 of a cell border, where the chain of
// roundings could floor differently.  Beams are clipped to the grid box first (samples outside can never hit).

struct ScanArgs {
  CaParams p;
  CaState s;
  CaMap m;
  CaScan sc;
  // map set (cagpu_laserscan_maps; nullptr otherwise): env e scans grid env_map[e] of the num_maps grids at m.static_bits
  const int32_t* env_map;
  int32_t num_maps;
};

// floor(origin + sign * coord / cell) exactly as float64 numpy computes it
__device__ __forceinline__ long cell_index(double origin, double sign, double coord, double cell, double inv_cell) {
  const double q = coord * inv_cell;
  double v = origin + sign * q;
  const double nearest = rint(v);
  const double mag = fmax(fmax(fabs(v), fabs(q)), 1.0);
  if (fabs(v - nearest) <= 1e-12 * mag) v = origin + sign * (coord / cell);  // rare: decide with the true quotient
  return static_cast<long>(floor(v));
}

__device__ __forceinline__ bool grid_bit(const uint32_t* g, int wpr, long r, long c) {
  return (g[r * wpr + (c >> 5)] >> (c & 31)) & 1u;
}

// collision_avoidance_env.py:494-506 + Map.py:54-58: does the agent's disc cover an occupied STATIC cell of the grid
// `bits` (m's geometry; nullptr: no walls)?
template <typename MapT>  // (CaMap, or an address-space-qualified view of it)
__device__ bool hits_wall_in(const MapT& m, const uint32_t* bits, double x, double y, double radius) {
  if (!bits) return false;
  const double fr = floor(m.origin_r - y / m.cell), fc = floor(m.origin_c + x / m.cell);
  if (!(fr >= 0.0 && fc >= 0.0 && fr < m.rows && fc < m.cols)) return false;
  const int gr = static_cast<int>(fr), gc = static_cast<int>(fc);  // (32-bit loop state: this sits inside the agent wave)
  const double rc = radius / m.cell, rr = rc * rc;
  const int R = static_cast<int>(fmin(ceil(rc), 1.0e6));
  const int wpr = (m.cols + 31) >> 5;
  const int r_lo = (gr - R < 0) ? 0 : gr - R, r_hi = (gr + R >= m.rows) ? m.rows - 1 : gr + R;
  const int c_lo = (gc - R < 0) ? 0 : gc - R, c_hi = (gc + R >= m.cols) ? m.cols - 1 : gc + R;
  for (int r = r_lo; r <= r_hi; ++r) {
    const double fdr = static_cast<double>(r - gr);
    for (int c = c_lo; c <= c_hi; ++c) {
      const double fdc = static_cast<double>(c - gc);
      if (fdc * fdc + fdr * fdr < rr && grid_bit(bits, wpr, r, c)) return true;
    }
  }
  return false;
}
// ... of the single map
template <typename MapT>
__device__ bool hits_wall(const MapT& m, double x, double y, double radius) {
  return hits_wall_in(m, m.static_bits, x, y, radius);
}

constexpr int SCAN_NT = 512;
constexpr int SCAN_U = 4;  // samples per iteration of the march (see scan_kernel)
constexpr int SCAN_PAD = 8;  // cells of empty border around the LDS bitmap (beams are clipped to the grid box + ~1 cell)
constexpr int HIST_AG = 4;   // agents whose range indices are staged before their history rows are rolled (scan_kernel)

// The per-env dynamic grid lives in LDS as ONE BYTE per cell (31 KB for the reference's 160 x 160 map + border): the
// march's hit test is then an integer multiply-add for the address, a byte load and a compare -- the bitmap of round 2
// (4.2 KB) cost six more instructions per sample for word address, shift and mask, in a VALU-issue-bound kernel.
__host__ __device__ inline int scan_pitch(int cols) { return (cols + 2 * SCAN_PAD + 3) & ~3; }  // bytes per padded row
__host__ __device__ inline size_t scan_grid_words(int rows, int cols) {  // LDS words of the padded byte grid
  return static_cast<size_t>(rows + 2 * SCAN_PAD) * scan_pitch(cols) / 4;
}

// Round 4, tried and dropped: a CLEARANCE grid (bytes = min(Chebyshev distance to the nearest occupied cell, 7), rebuilt per
// env from the 4 KB occupancy bitmap by six binary dilations + a SWAR accumulate: ~1.4 k instructions per thread and env) and
// a march that jumps max(clearance, 1) samples per iteration (range_res <= one cell, so the samples jumped over lie in free
// cells: first and second hit are the reference's; parity green).  On the config-5 scenes a wave's lanes then need 10.3
// iterations instead of 23.6 samples (wave maximum; the mean beam ends after 19 samples, not 60) -- but a jumping iteration
// costs ~36 instructions (four 64-bit multiply-adds for the fixed-point position, the border test and the exit test per
// sample) against 16 per sample of the four-samples-per-iteration loop below: 1440 vs 1436 us, no gain
// (profiles/r04_kernel_geometry.md section 3).  What did pay at the end of the round, all in the loop below: the border test on
// coordinates biased by its margin, the hit bookkeeping skipped for groups in which no beam of the wave hit anything, the
// per-agent part of a beam's set-up computed once per agent, the clip in float32, the range table: 1436 -> 1162 us.
// SLOTS: the slot march's form (cagpu_laserscan_slots: the (slot, env) pairs of a pose ring as n x E envs) -- the same
// staging, rasterisation and march, but the range indices go out as ONE new row per agent, uint8 [E, N, B] at sc.hist
// (sc.out is not used), instead of into the rolled history.  A template flag: scan_kernel<false> is the code, and takes the
// arguments, that scan_kernel was and took before the flag existed.
template <bool SLOTS>
__global__ __launch_bounds__(SCAN_NT) void scan_kernel(const ScanArgs k) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int N = k.p.num_agents;
  const int rows = k.m.rows, cols = k.m.cols, wpr = (cols + 31) >> 5;
  const int pitch = scan_pitch(cols);  // the LDS grid is padded by SCAN_PAD empty cells on every side: a sample that
                                       // leaves the grid by a cell reads a 0 and needs no bounds test
  const int tid = threadIdx.x;
  const long e = blockIdx.x;
  uint32_t* grid = reinterpret_cast<uint32_t*>(smem);                 // [(rows + 2 PAD) * pitch / 4]: four cells per word
  uint8_t* grid8 = reinterpret_cast<uint8_t*>(smem);
  double* a_px = reinterpret_cast<double*>(smem + align16(scan_grid_words(rows, cols) * 4));
  double* a_py = a_px + N;
  double* a_hd = a_py + N;
  double* a_rr = a_hd + N;   // (radius / cell)^2
  long* a_gr = reinterpret_cast<long*>(a_rr + N);
  long* a_gc = a_gr + N;
  int* a_in = reinterpret_cast<int*>(a_gc + N);
  int* a_R = a_in + N;
  int* a_first = a_R + N;
  double* a_sh = reinterpret_cast<double*>(a_first + N + (N & 1));  // sin / cos of the agent's heading
  double* a_ch = a_sh + N;
  double* a_v0r = a_ch + N;   // the agent's own (padded) grid coordinates: where every one of its beams starts
  double* a_v0c = a_v0r + N;
  double* b_sn = a_v0c + N;                                          // sin / cos of the beam angles (np.linspace)
  double* b_cs = b_sn + k.sc.num_beams;
  int* a_near = reinterpret_cast<int*>(b_cs + k.sc.num_beams);  // the laser reaches the grid box at all
  int* a_rego = a_near + N;   // last sample that can still fall into a cell of the agent's own disc (-1: none)
  int* a_thr = a_rego + N;    // ceil((radius / cell)^2)
  float* a_bx0 = reinterpret_cast<float*>(a_thr + N);  // the grid box (+ 1 cm) relative to the agent: xmin - px, xmax - px,
  float* a_bx1 = a_bx0 + N;                            // ymin - py, ymax - py
  float* a_by0 = a_bx1 + N;
  float* a_by1 = a_by0 + N;
  float* val_tab = a_by1 + N;  // [256] the float32 range of every range index (255 = nothing hit: max_range)
  uint32_t* idx_st = reinterpret_cast<uint32_t*>(val_tab + 256);  // [HIST_AG][B / 4] this round's range indices, 4 beams per word
  const double cell = k.m.cell, inv_cell = 1.0 / k.m.cell;
  // per-agent quantities every one of its 512 beams needs (they cost a float64 square root and a dozen float64
  // operations: computed once per agent below instead of once per beam)
  const double xmin = (0.0 - k.m.origin_c) * cell - 0.01, xmax = (cols - k.m.origin_c) * cell + 0.01;
  const double ymin = (k.m.origin_r - rows) * cell - 0.01, ymax = k.m.origin_r * cell + 0.01;
  const double reach = (k.sc.num_ranges - 1) * k.sc.range_res, res_cells = k.sc.range_res * inv_cell;

  // 1a. static grid -> padded LDS byte grid (cell (r, c) lands at byte (r + PAD) * pitch + c + PAD), four cells per
  // store; per-agent cells.  A map set: this env's own grid (one index per workgroup).
  {
    const uint32_t* sbits = k.m.static_bits;
    if (k.env_map) sbits = set_grid(sbits, static_cast<long>(rows) * wpr, k.num_maps, k.env_map[e], tid == 0);
    const int p4 = pitch >> 2;
    for (int w = tid; w < static_cast<int>(scan_grid_words(rows, cols)); w += SCAN_NT) {
      const int pr = w / p4, c0 = (w - pr * p4) * 4 - SCAN_PAD;  // first of this word's four cells
      const int r = pr - SCAN_PAD;
      uint32_t v = 0u;
      if (sbits && r >= 0 && r < rows) {
        const uint32_t* src = sbits + static_cast<long>(r) * wpr;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c0 + u;
          if (c >= 0 && c < cols) v |= ((src[c >> 5] >> (c & 31)) & 1u) << (8 * u);
        }
      }
      grid[w] = v;
    }
  }
  if (tid < N) {
    const long i = e * N + tid;
    const double px = k.s.pos_x[i], py = k.s.pos_y[i], rad = k.s.radius[i];
    a_px[tid] = px; a_py[tid] = py; a_hd[tid] = k.s.heading[i];
    const long gr = static_cast<long>(floor(k.m.origin_r - py / cell));  // Map.py:28-29 (one true divide per agent)
    const long gc = static_cast<long>(floor(k.m.origin_c + px / cell));
    a_gr[tid] = gr; a_gc[tid] = gc;
    a_in[tid] = (gr >= 0 && gc >= 0 && gr < rows && gc < cols) ? 1 : 0;
    const double rc = rad / cell;
    a_rr[tid] = rc * rc;
    a_R[tid] = static_cast<int>(ceil(rc));
    a_first[tid] = (k.s.step_num[i] == 0) ? 1 : 0;
    sincos(a_hd[tid], &a_sh[tid], &a_ch[tid]);
    // an agent farther than the laser's reach from the grid sees nothing on any beam
    const double ox = fmax(fmax(xmin - px, px - xmax), 0.0), oy = fmax(fmax(ymin - py, py - ymax), 0.0);
    a_near[tid] = (ox * ox + oy * oy <= (reach + 0.02) * (reach + 0.02)) ? 1 : 0;
    a_thr[tid] = static_cast<int>(ceil(rc * rc));
    a_rego[tid] = a_in[tid] ? static_cast<int>((sqrt(rc * rc) + 2.0) / res_cells) + 1 : -1;
    a_v0r[tid] = (k.m.origin_r - py * inv_cell) + static_cast<double>(SCAN_PAD);
    a_v0c[tid] = (k.m.origin_c + px * inv_cell) + static_cast<double>(SCAN_PAD);
    a_bx0[tid] = static_cast<float>(xmin - px); a_bx1[tid] = static_cast<float>(xmax - px);
    a_by0[tid] = static_cast<float>(ymin - py); a_by1[tid] = static_cast<float>(ymax - py);
  }
  for (int q = tid; q < 256; q += SCAN_NT)  // np.arange(...) * range_res as the sensor stores it, once per index
    val_tab[q] = (q == 255) ? static_cast<float>(k.sc.max_range) : static_cast<float>(0.0 + q * k.sc.range_res);
  {  // beam b looks along heading + angle_b: one sincos per beam ANGLE and per AGENT instead of one per (agent, beam);
     // sin / cos of the sum by the addition theorem (2 ulp instead of 1: a sample moves by 1e-15 m)
    const int B_ = k.sc.num_beams;
    const double step_ = (k.sc.max_angle - k.sc.min_angle) / (B_ - 1);
    for (int b = tid; b < B_; b += SCAN_NT) {
      const double base = (b == B_ - 1) ? k.sc.max_angle : b * step_ + k.sc.min_angle;  // np.linspace
      sincos(base, &b_sn[b], &b_cs[b]);
    }
  }
  __syncthreads();
  // 1b. rasterise the agents (Map.py:46-64): one task per (agent, row of its bounding box)
  int Rmax = 0;
  for (int a = 0; a < N; ++a) Rmax = a_R[a] > Rmax ? a_R[a] : Rmax;
  const int win = 2 * Rmax + 1;
  for (int t = tid; t < N * win; t += SCAN_NT) {
    const int a = t / win;
    const long dr = (t - a * win) - Rmax;
    if (!a_in[a] || dr < -a_R[a] || dr > a_R[a]) continue;
    const long r = a_gr[a] + dr;
    if (r < 0 || r >= rows) continue;
    const double rr = a_rr[a], fdr = static_cast<double>(dr);
    for (long dc = -a_R[a]; dc <= a_R[a]; ++dc) {
      const long c = a_gc[a] + dc;
      if (c < 0 || c >= cols) continue;
      const double fdc = static_cast<double>(dc);
      if (fdc * fdc + fdr * fdr < rr) {
        grid8[(r + SCAN_PAD) * pitch + c + SCAN_PAD] = 1;  // (every writer stores the same byte: no atomics)
      }
    }
  }
  __syncthreads();

  // 2./3. beams
  //   * a beam whose bounding box lies outside the grid cannot hit anything (Map.py: cells outside are never set and
  //     LaserScanSensor.py:74-77 masks samples outside the map): decided once per beam with a 1 cm margin;
  //   * along a beam the grid coordinate is affine in the sample index: v(r) = v0 + r * dv (in exact arithmetic; the
  //     reference's chain of float64 roundings stays within 1e-12 of it).  One FMA gives v(r) (shifted by PAD, so it
  //     is positive and float -> int truncation IS the floor); only when its fractional part lies within 1e-9 of a
  //     cell border is the reference's own expression (cell_index) evaluated to decide the floor;
  //   * the agent's own disc is tested on integer cell offsets, and only for the first samples of the beam: a sample
  //     s cells away from the agent cannot fall into a cell of its disc once s > radius / cell + 2;
  //   * the range index is the last sample before the SECOND hit (cumsum == 1, LaserScanSensor.py:77-81): the march is
  //     "find the first hit", then "find the next one".
  const int B = k.sc.num_beams, H = k.sc.num_to_store, R = k.sc.num_ranges;
  const float inv_res_f = static_cast<float>(1.0 / k.sc.range_res);
  // The marched samples start / end `slack` samples before / behind the clipped part [lo, hi] of a beam, so they lie up to
  // (slack + 1) range_res + 1 cm outside the grid box -- and must stay inside the SCAN_PAD cells of empty border around the
  // LDS grid, or the march would read what lies behind (the per-agent arrays) or before the grid as cells.  The extra
  // sample is dropped where it would not fit (range_res above ~3.4 cells): floor / ceil alone leave nearly a whole sample
  // of safety against the float32 clip, and a sample before lo or behind hi is outside the grid: it can never be a hit.
  // laserscan_impl admits only geometries whose slack-0 march fits the border.
  const int slack = ((2.0 * k.sc.range_res + 0.01) * inv_cell + 0.2 < SCAN_PAD) ? 1 : 0;
  // The history (3.): with the reference's 512 beams a round of the loop below is ONE agent; the range indices of HIST_AG
  // agents are staged in LDS (a byte per beam) and the history rows of those agents are then rolled FOUR BEAMS PER THREAD --
  // one dword of range indices per row loaded / stored, one float4 of ranges per row stored -- instead of a byte load, a byte
  // store and a 4-byte store per beam and row (64-byte and 256-byte wave transactions; ~80 of the ~570 wave-instructions
  // per (agent, 64 beams)).  Other beam counts keep the per-beam form.
  const bool vec_hist = (B == SCAN_NT) && ((reinterpret_cast<uintptr_t>(k.sc.hist) | (SLOTS ? 0 : reinterpret_cast<uintptr_t>(k.sc.out))) & 15) == 0;
  for (int t0 = 0; t0 < N * B; t0 += SCAN_NT) {
    const int t = t0 + tid;
    const bool in_range = t < N * B;
    const int a = in_range ? t / B : 0, b = in_range ? t - a * B : 0;
    int idx = 255;
    if (in_range) {
    const double px = a_px[a], py = a_py[a];
    if (a_near[a]) {
      const double sn = b_sn[b] * a_ch[a] + b_cs[b] * a_sh[a], cs = b_cs[b] * a_ch[a] - b_sn[b] * a_sh[a];
      // the sample indices whose point can lie inside the grid box (conservative: 1 cm box margin, +-slack samples; the
      // reciprocals need no more than a few digits)
      // (in float32: the box carries a margin of 1 cm and the range +-1 sample, four orders of magnitude above what
      // float32 loses on coordinates of a few tens of metres)
      float lo = 0.0f, hi = static_cast<float>(reach);
      const float csf = static_cast<float>(cs), snf = static_cast<float>(sn);
      if (fabsf(csf) > 1e-12f) {
        const float ic = __builtin_amdgcn_rcpf(csf);
        const float t0 = a_bx0[a] * ic, t1 = a_bx1[a] * ic;
        lo = fmaxf(lo, fminf(t0, t1));
        hi = fminf(hi, fmaxf(t0, t1));
      } else if (px < xmin || px > xmax) {
        hi = -1.0f;
      }
      if (fabsf(snf) > 1e-12f) {
        const float is = __builtin_amdgcn_rcpf(snf);
        const float t0 = a_by0[a] * is, t1 = a_by1[a] * is;
        lo = fmaxf(lo, fminf(t0, t1));
        hi = fminf(hi, fmaxf(t0, t1));
      } else if (py < ymin || py > ymax) {
        hi = -1.0f;
      }
      if (hi >= lo) {
        int r_lo = static_cast<int>(floorf(lo * inv_res_f)) - slack, r_hi = static_cast<int>(ceilf(hi * inv_res_f)) + slack;
        r_lo = r_lo < 0 ? 0 : r_lo;
        r_hi = r_hi > R - 1 ? R - 1 : r_hi;
        const int er = static_cast<int>(a_gr[a]) + SCAN_PAD, ec = static_cast<int>(a_gc[a]) + SCAN_PAD;  // padded coordinates
        const int ego_thr = a_thr[a], r_ego = a_rego[a];
        const double v0r = a_v0r[a], dvr = -sn * res_cells;
        const double v0c = a_v0c[a], dvc = cs * res_cells;
        // The march, in 32.32 fixed point: along a beam the (padded, hence positive) grid coordinate is affine in the sample
        // index, v(r) = v0 + r dv, so a sample costs two 64-bit integer adds; the cell is the high word and "within
        // 6e-8 of a cell border" is one unsigned compare on the low word (the fixed-point path is within 61 x 2^-32 =
        // 1.4e-8 of the exact affine value, which is within 1e-12 of the reference's chain of float64 roundings: only for
        // such a sample -- a few in 10^7 -- is the reference's own expression (cell_index) evaluated).  Then one LDS word,
        // a bit test, the own-disc test for the first samples; the hit count and the last hit's index are all the state
        // (range index = sample before the SECOND hit, or the last sample if there is only one hit).  ~12 instead of 24
        // instructions per sample of a VALU-issue-bound kernel.
        auto to_fx = [](const double v) -> unsigned long long {
          const double f = floor(v);
          const unsigned hi = static_cast<unsigned>(static_cast<int>(f));
          const unsigned lo = static_cast<unsigned>((v - f) * 4294967296.0);
          return (static_cast<unsigned long long>(hi) << 32) | lo;
        };
        constexpr unsigned MARGIN = 256u;  // 6e-8 cells
        int n_hit = 0, last = 0;
        const double fr0 = static_cast<double>(r_lo);
        // (both coordinates carry a bias of MARGIN: "low word within MARGIN of a border on either side" is then the single
        // compare lo < 2 MARGIN with no add per sample, and the high word is still the cell wherever that test fails --
        // the bias can only carry into it from the MARGIN below a border, which is inside the band)
        unsigned long long vr_fx = to_fx(fma(fr0, dvr, v0r)) + MARGIN, vc_fx = to_fx(fma(fr0, dvc, v0c)) + MARGIN;
        const unsigned long long dvr_fx = to_fx(dvr), dvc_fx = to_fx(dvc);
        // one sample the careful way: border fallback, own-disc test (the first samples of a beam, and the leftovers)
        auto step1 = [&](const int r) {
          int gr = static_cast<int>(vr_fx >> 32), gc = static_cast<int>(vc_fx >> 32);
          const unsigned lr = static_cast<unsigned>(vr_fx), lc = static_cast<unsigned>(vc_fx);
          if ((lr < 2u * MARGIN) | (lc < 2u * MARGIN)) {  // rare: the reference's own rounding decides
            const double rg = 0.0 + r * k.sc.range_res;  // np.arange
            const double x = px + rg * cs, y = py + rg * sn;
            long cr = cell_index(k.m.origin_r, -1.0, y, cell, inv_cell), cc = cell_index(k.m.origin_c, 1.0, x, cell, inv_cell);
            cr = cr < -SCAN_PAD ? -SCAN_PAD : (cr > rows + SCAN_PAD - 1 ? rows + SCAN_PAD - 1 : cr);  // (the border is empty)
            cc = cc < -SCAN_PAD ? -SCAN_PAD : (cc > cols + SCAN_PAD - 1 ? cols + SCAN_PAD - 1 : cc);
            gr = static_cast<int>(cr) + SCAN_PAD;
            gc = static_cast<int>(cc) + SCAN_PAD;
          }
          bool hit = grid8[__mul24(gr, pitch) + gc] != 0;
          if (r <= r_ego) {
            const int dc = gc - ec, dr = gr - er;
            hit = hit && !(__mul24(dc, dc) + __mul24(dr, dr) < ego_thr);
          }
          n_hit += hit ? 1 : 0;
          last = hit ? r : last;
          vr_fx += dvr_fx;
          vc_fx += dvc_fx;
        };
        int r = r_lo;
        // SCAN_U samples per iteration -- their addresses, their byte loads in flight together, ONE border test
        // (the smallest of the 2 SCAN_U distances to a cell border) and one exit test; a group that holds a border case
        // is walked sample by sample
        while (n_hit < 2 && r + (SCAN_U - 1) <= r_hi) {
          unsigned long long vr[SCAN_U], vc[SCAN_U];
          vr[0] = vr_fx; vc[0] = vc_fx;
#pragma unroll
          for (int u = 1; u < SCAN_U; ++u) { vr[u] = vr[u - 1] + dvr_fx; vc[u] = vc[u - 1] + dvc_fx; }
          unsigned m = min(static_cast<unsigned>(vr[0]), static_cast<unsigned>(vc[0]));
#pragma unroll
          for (int u = 1; u < SCAN_U; ++u) m = min(m, min(static_cast<unsigned>(vr[u]), static_cast<unsigned>(vc[u])));
          if (m < 2u * MARGIN) {
            for (int u = 0; u < SCAN_U && n_hit < 2; ++u, ++r) step1(r);
            continue;
          }
          uint8_t h[SCAN_U];
#pragma unroll
          for (int u = 0; u < SCAN_U; ++u)
            h[u] = grid8[__mul24(static_cast<int>(vr[u] >> 32), pitch) + static_cast<int>(vc[u] >> 32)];
          if (r <= r_ego) {  // the first samples of a beam can fall into the agent's own disc, which is transparent
#pragma unroll
            for (int u = 0; u < SCAN_U; ++u) {
              const int dc = static_cast<int>(vc[u] >> 32) - ec, dr = static_cast<int>(vr[u] >> 32) - er;
              h[u] = (__mul24(dc, dc) + __mul24(dr, dr) < ego_thr) ? 0 : h[u];
            }
          }
          unsigned any_h = h[0];
#pragma unroll
          for (int u = 1; u < SCAN_U; ++u) any_h |= h[u];
          if (__any(any_h != 0)) {  // (most groups of a wave's 64 neighbouring beams cross free space only)
#pragma unroll
            for (int u = 0; u < SCAN_U; ++u) {
              const int t = (h[u] != 0) & (n_hit < 2);
              n_hit += t;
              last = t ? r + u : last;
            }
          }
          vr_fx = vr[SCAN_U - 1] + dvr_fx;
          vc_fx = vc[SCAN_U - 1] + dvc_fx;
          r += SCAN_U;
        }
        for (; r <= r_hi && n_hit < 2; ++r) step1(r);
        if (n_hit > 0) idx = (n_hit == 2) ? last - 1 : R - 1;  // one hit: cumsum stays 1 up to the last sample
      }
    }
    }
    if (vec_hist) {
      // (B == SCAN_NT: this round is agent a0 = t0 / B, thread = beam)
      const int a0 = t0 / B, slot = a0 % HIST_AG;
      reinterpret_cast<uint8_t*>(idx_st)[slot * B + tid] = static_cast<uint8_t>(idx);
      const bool last_round = a0 == N - 1;
      if (slot == HIST_AG - 1 || last_round) {
        __syncthreads();
        const int n_ag = slot + 1, first_ag = a0 - slot;
        if constexpr (SLOTS) {  // the staged agents' rows are contiguous: four beams per store, nothing else
          uint32_t* dst = reinterpret_cast<uint32_t*>(k.sc.hist + (e * N + first_ag) * B);
          for (int g = tid; g < n_ag * (B / 4); g += SCAN_NT) dst[g] = idx_st[g];
        } else
        for (int g = tid; g < n_ag * (B / 4); g += SCAN_NT) {
          const int sa = g / (B / 4), q4 = g - sa * (B / 4), ag = first_ag + sa;
          const long ii = e * N + ag;
          uint32_t* hrow = reinterpret_cast<uint32_t*>(k.sc.hist + (ii * H) * B) + q4;   // row h: + h * (B / 4)
          float4* orow = reinterpret_cast<float4*>(k.sc.out + (ii * H) * B) + q4;
          const uint32_t nw = idx_st[sa * (B / 4) + q4];
          const auto ranges = [&](const uint32_t w) {
            return make_float4(val_tab[w & 255u], val_tab[(w >> 8) & 255u], val_tab[(w >> 16) & 255u], val_tab[w >> 24]);
          };
          if (a_first[ag]) {  // LaserScanSensor.py:84-85: the first measurement fills every row
            const float4 v = ranges(nw);
            for (int h = 0; h < H; ++h) { hrow[h * (B / 4)] = nw; orow[h * (B / 4)] = v; }
          } else {            // np.roll(history, 1, axis=0); history[0] = ranges
            uint32_t prev = hrow[0];
            for (int h = 1; h < H; ++h) {
              const uint32_t cur = hrow[h * (B / 4)];
              hrow[h * (B / 4)] = prev;
              orow[h * (B / 4)] = ranges(prev);
              prev = cur;
            }
            hrow[0] = nw;
            orow[0] = ranges(nw);
          }
        }
        __syncthreads();
      }
      continue;
    }
    if (!in_range) continue;
    if constexpr (SLOTS) {
      k.sc.hist[(e * N + a) * B + b] = static_cast<uint8_t>(idx);
      continue;
    }
    const long i = e * N + a;
    uint8_t* hist = k.sc.hist + (i * H) * B + b;
    float* out = k.sc.out + (i * H) * B + b;
    const float val = val_tab[idx];
    if (a_first[a]) {  // LaserScanSensor.py:84-85
      for (int h = 0; h < H; ++h) { hist[h * B] = static_cast<uint8_t>(idx); out[h * B] = val; }
    } else {           // np.roll(history, 1, axis=0); history[0] = ranges
      for (int h = H - 1; h > 0; --h) {
        const uint8_t prev = hist[(h - 1) * B];
        hist[h * B] = prev;
        out[h * B] = val_tab[prev];
      }
      hist[0] = static_cast<uint8_t>(idx);
      out[0] = val;
    }
  }
}
