// gym_collision_avoidance_amd/csrc/cagpu_metrics.inc -- included by cagpu.hip (inside its anonymous namespace).
//
// Per-episode path and closest-approach metrics (CaEpMetrics, DESIGN.md section 3j): a reduction over trajectory-tape slots
// (CaTraj) that keeps a small carry per env between calls and writes one record per episode into the env's ring, slot
// k % capacity -- the episode log's slot rule.  tests/episode_metrics_ref.py is the NumPy statement of the same rules; every
// expression below is a chain of single IEEE float64 operations (no multiply-add: the library is built with
// -ffp-contract=off and the pragma below says so again for this file), each agent's sums are added by ONE lane in slot
// order, and sqrt / remainder are correctly rounded / exact, so the outputs equal the reference's bit for bit.
//
// One workgroup per env, thread = agent slot; the walk over the slots is serial, everything else parallel:
//   N <= 64          metrics_kernel<64>: the workgroup IS one wave (its barrier is a wait on the wave's own LDS traffic); a
//                    lane's row is 96 contiguous bytes, the wave reads one contiguous block of 96 N bytes per slot;
//   65 <= N <= 1024  metrics_kernel<1024>: ceil(N / 64) waves.
// Positions, radii and the `seen` marks of the env's agents live in LDS (28 bytes per thread); the all-pairs minimum of a
// slot reads them as broadcasts.  Column 11 of slot t + 2 and the columns of slot t + 1 (only of rows that moved: columns
// 0 - 10 of a row that did not move are NEVER read) are loaded before the arithmetic of slot t.
// Reads the tape; writes the records, the stamps and the carry only -- plain vector stores.

struct MetricsArgs {
  const double* rows;       // [T, E, N, 12]
  const int32_t* episode;   // [T, E]
  double* vals;             // [E, C, N, 4]
  int32_t* cnts;            // [E, C, N, 4]
  int32_t* head;            // [E, C]
  unsigned char* carry;     // [E, metrics_carry_env_bytes(N)]
  int32_t E, N, T, C;
  double dt, close_range;
};

// the carry of one env: N x 8 doubles {px, py, radius, heading, path_length, min_gap, turn_sum, min_gap_t}, N x 4 int32
// {bit 0 seen | bit 1 has_heading, moved_steps, close_steps, min_gap_partner}, then {episode id, started, 0, 0}.  All zero
// (started == 0) = nothing carried: the caller's memset is the initial state and the clear of a host-side reset.
__host__ __device__ inline size_t metrics_carry_env_bytes(int N) { return static_cast<size_t>(N) * 80 + 16; }

struct MetricsRow { double t, px, py, rad, vx, vy, hd; };

__device__ inline MetricsRow metrics_load(const double* __restrict__ row) {
  MetricsRow r;
  r.t = row[0]; r.px = row[1]; r.py = row[2]; r.rad = row[5]; r.vx = row[7]; r.vy = row[8]; r.hd = row[10];
  return r;
}

template <int NT_MAX>
__global__ __launch_bounds__(NT_MAX) void metrics_kernel(const MetricsArgs k) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double metrics_lds[];
  const int NT = blockDim.x, a = threadIdx.x, N = k.N, T = k.T;
  const size_t e = blockIdx.x, E = static_cast<size_t>(k.E);
  double* spx = metrics_lds;
  double* spy = spx + NT;
  double* srad = spy + NT;
  int32_t* sseen = reinterpret_cast<int32_t*>(srad + NT);
  const bool mine = a < N;
  const double inf = __builtin_inf(), nan = __builtin_nan("");

  unsigned char* cbase = k.carry + e * metrics_carry_env_bytes(N);
  double* cd = reinterpret_cast<double*>(cbase) + static_cast<size_t>(a) * 8;
  int32_t* ci = reinterpret_cast<int32_t*>(cbase + static_cast<size_t>(N) * 64) + static_cast<size_t>(a) * 4;
  int32_t* ch = reinterpret_cast<int32_t*>(cbase + static_cast<size_t>(N) * 80);
  int32_t id = ch[0];
  bool started = ch[1] != 0;

  double px = 0.0, py = 0.0, rad = 0.0, hd = 0.0, path = 0.0, min_gap = inf, turn = 0.0, min_gap_t = nan;
  int32_t seen = 0, has_hd = 0, moved_steps = 0, close_steps = 0, partner = -1;
  if (started && mine) {
    px = cd[0]; py = cd[1]; rad = cd[2]; hd = cd[3]; path = cd[4]; min_gap = cd[5]; turn = cd[6]; min_gap_t = cd[7];
    seen = ci[0] & 1; has_hd = (ci[0] >> 1) & 1; moved_steps = ci[1]; close_steps = ci[2]; partner = ci[3];
  }
  spx[a] = px; spy[a] = py; srad[a] = rad; sseen[a] = seen;

  auto write_record = [&](int32_t kk) {   // the running episode's record -> slot kk % C of the env's ring
    if (kk < 0) return;
    const size_t slot = e * static_cast<size_t>(k.C) + static_cast<size_t>(kk % k.C);
    if (mine) {
      double* v = k.vals + (slot * N + a) * 4;
      v[0] = path; v[1] = min_gap; v[2] = turn; v[3] = min_gap_t;
      int32_t* c = k.cnts + (slot * N + a) * 4;
      c[0] = moved_steps; c[1] = close_steps; c[2] = partner; c[3] = 0;
    }
    if (a == 0) k.head[slot] = kk;
  };

  const size_t slot_stride = E * N * 12;
  const double* row0 = k.rows + (e * N + (mine ? a : 0)) * 12;
  // software pipeline: c11 of slots t + 1 and t + 2 and the row of slot t + 1 are in flight while slot t is worked on
  double c11_0 = -1.0, c11_1 = -1.0;
  MetricsRow r0 = {}, r1 = {};
  int32_t ep0 = 0, ep1 = 0;
  if (mine) c11_0 = row0[11];
  ep0 = k.episode[e];
  if (T > 1) {
    if (mine) c11_1 = row0[slot_stride + 11];
    ep1 = k.episode[E + e];
  }
  if (c11_0 >= 0.0) r0 = metrics_load(row0);

  for (int t = 0; t < T; ++t) {
    double c11_2 = -1.0;
    int32_t ep2 = 0;
    if (t + 2 < T) {
      if (mine) c11_2 = row0[static_cast<size_t>(t + 2) * slot_stride + 11];
      ep2 = k.episode[static_cast<size_t>(t + 2) * E + e];
    }
    if (c11_1 >= 0.0) r1 = metrics_load(row0 + static_cast<size_t>(t + 1) * slot_stride);   // (c11_1 is -1 past the last slot)

    if (started && ep0 != id) {   // (uniform over the workgroup) the carried episode is over: its record, a clean carry
      write_record(id);
      px = py = rad = hd = path = turn = 0.0; min_gap = inf; min_gap_t = nan;
      seen = has_hd = moved_steps = close_steps = 0; partner = -1;
      sseen[a] = 0;
    }
    id = ep0; started = true;
    const bool moved = c11_0 >= 0.0;
    if (moved) {
      px = r0.px; py = r0.py; rad = r0.rad; seen = 1;
      spx[a] = px; spy[a] = py; srad[a] = rad; sseen[a] = 1;
    }
    __syncthreads();
    if (moved) {
      moved_steps += 1;
      path = path + sqrt(r0.vx * r0.vx + r0.vy * r0.vy) * k.dt;
      if (has_hd) turn = turn + fabs(remainder(r0.hd - hd, 2.0 * M_PI));
      hd = r0.hd; has_hd = 1;
      double g_min = inf;
      int32_t g_j = -1;
      for (int j = 0; j < N; ++j) {
        if (j == a || !sseen[j]) continue;
        const double dx = spx[j] - px, dy = spy[j] - py;
        const double g = (sqrt(dx * dx + dy * dy) - rad) - srad[j];
        if (g_j < 0 || g < g_min) { g_min = g; g_j = j; }
      }
      if (g_j >= 0) {
        close_steps += g_min <= k.close_range ? 1 : 0;
        if (g_min < min_gap) { min_gap = g_min; partner = g_j; min_gap_t = r0.t; }
      }
    }
    __syncthreads();   // (the next slot's positions overwrite what this slot's pairs read)
    c11_0 = c11_1; c11_1 = c11_2; r0 = r1; ep0 = ep1; ep1 = ep2;
  }

  if (!started) return;   // (T == 0 never launches; nothing seen, nothing to store)
  write_record(id);
  if (mine) {
    cd[0] = px; cd[1] = py; cd[2] = rad; cd[3] = hd; cd[4] = path; cd[5] = min_gap; cd[6] = turn; cd[7] = min_gap_t;
    ci[0] = seen | (has_hd << 1); ci[1] = moved_steps; ci[2] = close_steps; ci[3] = partner;
  }
  if (a == 0) { ch[0] = id; ch[1] = 1; ch[2] = 0; ch[3] = 0; }
}
