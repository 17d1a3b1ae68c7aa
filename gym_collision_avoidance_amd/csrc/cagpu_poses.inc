// gym_collision_avoidance_amd/csrc/cagpu_poses.inc -- included by cagpu.hip (inside its anonymous namespace, after
// cagpu_rules.inc: it calls reset_case / reset_heading / reset_lane / map_draw, the functions the step kernels call).
//
// Map sensors for EVERY step of a fused launch (DESIGN.md section 3m), without a step kernel knowing:
//   poses_kernel    the pose of every agent after each step of a launch, restated from the launch's trajectory tape, its
//                   game_over ring and the auto-reset's rules -- slot t of the output is a valid CaState view for
//                   scan_kernel<true> (cagpu_scan.inc) and occ_kernel;
//   scan_hist_kernel  the LaserScanSensor history of any slot range from the per-slot index rows.
// tests/pose_tape_ref.py is the NumPy statement of both rules.  Plain vector loads and stores only.

struct PoseArgs {
  CaParams p;
  // the state as the launch found it
  const double *pos_x, *pos_y, *heading, *radius;
  const int32_t *step_num, *reset_count, *env_map_in;
  // what the launch recorded
  const double* rows;        // [n, E, N, 12]
  const uint8_t* game_over;  // [n, E]
  int32_t n_steps;
  // the auto-reset (table == nullptr: none) and the map set's draw (map_seed == 0: none)
  const double* table;
  int32_t n_cases;
  int64_t env_id_offset, case_stride;
  unsigned long long heading_seed, map_seed;
  int32_t num_maps;
  // the ring
  double *o_px, *o_py, *o_hd, *o_rad;
  int32_t *o_step, *o_map;
};

// One thread per agent slot; the walk over the slots is serial (a carry of five values), a wave reads 64 consecutive rows.
__global__ __launch_bounds__(256) void poses_kernel(const PoseArgs k) {
  const long EN = static_cast<long>(k.p.num_envs) * k.p.num_agents;
  const long i = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= EN) return;
  const int N = k.p.num_agents;
  const long e = i / N;
  const int a = static_cast<int>(i - e * N);
  double px = k.pos_x[i], py = k.pos_y[i], hd = k.heading[i], rad = k.radius[i];
  int32_t sn = k.step_num[i], rc = k.reset_count[e];
  int32_t m = k.env_map_in ? k.env_map_in[e] : 0;
  KArgs ka;  // (reset_case / reset_heading read these four members only)
  ka.env_id_offset = k.env_id_offset; ka.case_stride = k.case_stride; ka.n_cases = k.n_cases; ka.heading_seed = k.heading_seed;
  const double* row = k.rows + i * 12;
  double c11 = row[11];
  for (int t = 0; t < k.n_steps; ++t) {
    const double c11_next = (t + 1 < k.n_steps) ? row[EN * 12 + 11] : -1.0;
    if (c11 >= 0.0) {  // the agent moved: its pose after the move (columns 0 - 10 of any other row are never read)
      px = row[1]; py = row[2]; hd = row[10];
      sn = static_cast<int32_t>(c11) + 1;
    }
    if (k.table && k.game_over[static_cast<long>(t) * k.p.num_envs + e]) {  // the env's next episode starts here
      rc += 1;
      const long c = reset_case(ka, e, rc);
      Lane r;
      r.flags = 0u;
      reset_lane(r, k.table + (c * N + a) * 6, k.heading_seed != 0, reset_heading(ka, e, rc, a), k.p);
      px = r.px; py = r.py; hd = r.heading; rad = r.rad; sn = r.step_num;
      if (k.map_seed) m = map_draw(k.map_seed, k.env_id_offset + e, rc, k.num_maps);
    }
    const long o = static_cast<long>(t) * EN + i;
    k.o_px[o] = px; k.o_py[o] = py; k.o_hd[o] = hd; k.o_rad[o] = rad; k.o_step[o] = sn;
    if (k.o_map && a == 0) k.o_map[static_cast<long>(t) * k.p.num_envs + e] = m;
    row += EN * 12;
    c11 = c11_next;
  }
}

struct ScanHistArgs {
  const uint8_t* idx;        // [n, E, N, B] the slots' new index rows (scan_kernel<true>)
  const int32_t* step_num;   // [n, E, N] of the pose ring
  const uint8_t* carried;    // [E, N, H, B] the history the launch found
  uint8_t* o_hist;           // [count, E, N, H, B] or nullptr
  float* o_out;              // [count, E, N, H, B] or nullptr
  long EN;
  int32_t first, count, B, H;
  double range_res, max_range;
};

// Row j of slot t's history = the index row of slot max(t - j, s), s the latest slot <= t whose step_num is 0 (the first
// measurement of an episode fills every row: LaserScanSensor.py:84-88); a slot before the launch = the carried history,
// slot -1 - r being its row r.  One thread per (slot, agent, W beams), W = 4 (a dword of indices, a float4 of ranges) or 1;
// rows are written from the last to the first and a row reads carried rows BELOW its own index only, so a single slot
// may be expanded in place (o_hist == carried).
template <int W>
__global__ __launch_bounds__(256) void scan_hist_kernel(const ScanHistArgs k) {
  const int BW = k.B / W;
  const long per_slot = k.EN * BW;
  const long g = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  if (g >= per_slot * k.count) return;
  const int ts = static_cast<int>(g / per_slot);
  const long rem = g - ts * per_slot;
  const long i = rem / BW;
  const int q = static_cast<int>(rem - i * BW);
  const int t = k.first + ts, H = k.H, B = k.B;
  int s = -H;  // (anything below t - H + 1: no row reaches that far)
  for (int u = t; u >= 0 && u > t - H; --u)
    if (k.step_num[u * k.EN + i] == 0) { s = u; break; }
  // np.arange(...) * range_res as the sensor stores it (scan_kernel's val_tab)
  const auto range_of = [&](const unsigned v) {
    return v == 255u ? static_cast<float>(k.max_range) : static_cast<float>(0.0 + static_cast<int>(v) * k.range_res);
  };
  for (int j = H - 1; j >= 0; --j) {
    int u = t - j;
    u = u < s ? s : u;
    const uint8_t* src = (u >= 0) ? k.idx + (u * k.EN + i) * B : k.carried + (i * H + (-1 - u)) * B;
    const long o = ((ts * k.EN + i) * H + j) * B;
    if constexpr (W == 4) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(src)[q];
      if (k.o_hist) reinterpret_cast<uint32_t*>(k.o_hist + o)[q] = w;
      if (k.o_out)
        reinterpret_cast<float4*>(k.o_out + o)[q] =
            make_float4(range_of(w & 255u), range_of((w >> 8) & 255u), range_of((w >> 16) & 255u), range_of(w >> 24));
    } else {
      const uint8_t v = src[q];
      if (k.o_hist) k.o_hist[o + q] = v;
      if (k.o_out) k.o_out[o + q] = range_of(v);
    }
  }
}
