// gym_collision_avoidance_amd/csrc/cagpu_gen.inc -- included by cagpu.hip (inside its anonymous namespace).
//
// Random scenario generation on the device: generate_rand_test_case_multi (reference
// envs/policies/CADRL/scripts/multi/gen_rand_testcases.py:111-444, the generator behind test_cases.get_testcase_random,
// envs/test_cases.py:212-253) for a whole table of cases at once, so that training-mode resets no longer build every
// scenario in Python.  One thread per case: the generator is a chain of rejection loops over the agents placed so far
// (sequential by construction); a table of 4096 cases x 10 agents takes well under a millisecond.
//
// Randomness: counter-based Philox4x32-10, key = seed, counter = (draw block, case index) -- the k-th uniform draw of
// case c is a pure function of (seed, c, k), independent of the launch geometry.  It cannot reproduce numpy's Mersenne
// stream; what IS kept is the reference's draw ORDER and every accept / reject expression, i.e. this kernel equals the
// host generator (envs/scenario_generator.py, itself bit-identical to the reference under np.random) when that one is
// driven by the same Philox stream (tests/test_gpu_parity.py::test_device_scenarios_match_host_generator).
namespace gen {

struct Args {
  double* cases;  // [C, N, 6] = px, py, gx, gy, pref_speed, radius
  int32_t* status;  // [C] or nullptr: 0 ok, 1 = an agent was placed after the attempt cap (never seen in practice)
  long C;
  int N;
  double side_lo, side_hi, speed_lo, speed_hi, radius_lo, radius_hi;
  unsigned long long seed;
  int max_attempts;
  // ragged tables (test_cases.py:224-241): the agent count of a case drawn in [n_min, n_max] (n_max = 0: always N) and
  // the side length from every {agent-count range: side range} entry that holds the count
  int n_min, n_max, n_ranges;
  double ranges[8][4];  // count lo, count hi (exclusive), side lo, side hi
  int32_t* counts;      // [C] or nullptr: the agent count of each case
};

constexpr double GETTING_CLOSE = 0.2;  // CADRL/scripts/multi/global_var.py:8
constexpr double SEG_EPS = 1e-5;       // global_var.py:9

struct Rng {
  unsigned k0, k1, c2, c3, block;
  unsigned w[4];
  int have;  // doubles left in w
  __device__ void refill() {
    unsigned c0 = block, c1 = 0u, x2 = c2, x3 = c3, q0 = k0, q1 = k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
      const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * x2;
      const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c1 ^ q0, n1 = static_cast<unsigned>(p1);
      const unsigned n2 = static_cast<unsigned>(p0 >> 32) ^ x3 ^ q1, n3 = static_cast<unsigned>(p0);
      c0 = n0; c1 = n1; x2 = n2; x3 = n3;
      q0 += 0x9E3779B9u; q1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = x2; w[3] = x3;
    block += 1u;
    have = 2;
  }
  __device__ double uniform() {  // [0, 1) with 53 random bits (the construction of numpy's legacy random_sample)
    if (have == 0) refill();
    const int o = (2 - have) * 2;
    have -= 1;
    return (static_cast<double>(w[o] >> 5) * 67108864.0 + static_cast<double>(w[o + 1] >> 6)) / 9007199254740992.0;
  }
};

// one uniform in [0, 1) for a 128-bit counter (the step kernel's random reset headings)
__device__ __forceinline__ double uniform_at(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
  unsigned k0 = static_cast<unsigned>(seed), k1 = static_cast<unsigned>(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c1 ^ k0, n1 = static_cast<unsigned>(p1);
    const unsigned n2 = static_cast<unsigned>(p0 >> 32) ^ c3 ^ k1, n3 = static_cast<unsigned>(p0);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return (static_cast<double>(c0 >> 5) * 67108864.0 + static_cast<double>(c1 >> 6)) / 9007199254740992.0;
}

// both uniforms of the same block: words 0, 1 -> ua (uniform_at's), words 2, 3 -> ub (the step kernels' RVO draw, CaRvoDraw)
__device__ __forceinline__ void uniform2_at(unsigned long long seed, unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                            double& ua, double& ub) {
  unsigned k0 = static_cast<unsigned>(seed), k1 = static_cast<unsigned>(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c1 ^ k0, n1 = static_cast<unsigned>(p1);
    const unsigned n2 = static_cast<unsigned>(p0 >> 32) ^ c3 ^ k1, n3 = static_cast<unsigned>(p0);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  ua = (static_cast<double>(c0 >> 5) * 67108864.0 + static_cast<double>(c1 >> 6)) / 9007199254740992.0;
  ub = (static_cast<double>(c2 >> 5) * 67108864.0 + static_cast<double>(c3 >> 6)) / 9007199254740992.0;
}

__device__ __forceinline__ double norm2(double x, double y) { return sqrt(x * x + y * y); }

// gen_rand_testcases.py:91-108
__device__ double dist_point_to_segment(double p1x, double p1y, double p2x, double p2y, double p3x, double p3y) {
  const double dx = p2x - p1x, dy = p2y - p1y;
  const double n = norm2(dx, dy);
  double u = 0.0;
  if (!(n < SEG_EPS)) u = (dx * (p3x - p1x) + dy * (p3y - p1y)) / (n * n);
  u = fmax(0.0, fmin(u, 1.0));
  return norm2(p3x - (p1x + u * dx), p3y - (p1y + u * dy));
}

// find_dist_between_segs, gen_rand_testcases.py:52-88 (single pair): closest approach of x1 -> x2 and y1 -> y2 over the
// same unit time, not counting the start
__device__ double min_dist_moving(double x1x, double x1y, double x2x, double x2y, double y1x, double y1y, double y2x,
                                  double y2y) {
  const double end_dist = norm2(x2x - y2x, x2y - y2y);
  double critical = end_dist;
  const double zx = (x2x - x1x) - (y2x - y1x), zy = (x2y - x1y) - (y2y - y1y);
  if (norm2(zx, zy) > 0.0) {
    const double t = -((x1x - y1x) * zx + (x1y - y1y) * zy) / (zx * zx + zy * zy);
    const double bx = x1x + (x2x - x1x) * t - y1x - (y2x - y1x) * t;
    const double by = x1y + (x2y - x1y) * t - y1y - (y2y - y1y) * t;
    if (t > 0.0 && t < 1.0) critical = norm2(bx, by);
  }
  return fmin(end_dist, critical);
}

// if_permitStraightLineSoln, gen_rand_testcases.py:422-444
__device__ bool straight_lines_are_safe(double x1x, double x1y, double x2x, double x2y, double s1, double y1x, double y1y,
                                        double y2x, double y2y, double s2, double radius) {
  const double t1 = norm2(x2x - x1x, x2y - x1y) / s1, t2 = norm2(y2x - y1x, y2y - y1y) / s2;
  double xcx, xcy, ycx, ycy;
  if (t1 < t2) {
    xcx = x2x; xcy = x2y;
    ycx = y1x + t1 * (y2x - y1x) / t2; ycy = y1y + t1 * (y2y - y1y) / t2;
    if (dist_point_to_segment(ycx, ycy, y2x, y2y, xcx, xcy) < radius) return false;
  } else {
    xcx = x1x + t2 * (x2x - x1x) / t1; xcy = x1y + t2 * (x2y - x1y) / t1;
    ycx = y2x; ycy = y2y;
    if (dist_point_to_segment(xcx, xcy, x2x, x2y, ycx, ycy) < radius) return false;
  }
  const double start_dist = norm2(x1x - y1x, x1y - y1y), end_dist = norm2(xcx - ycx, xcy - ycy);
  const double mid = min_dist_moving(x1x, x1y, xcx, xcy, y1x, y1y, ycx, ycy);
  return !(fmin(fmin(start_dist, end_dist), mid) < radius);
}

// start within (r_j + r_i + 0.2) of an earlier start, or end of an earlier end (gen_rand_testcases.py:178-188 / 352-360)
__device__ bool overlaps_earlier(const double* cs, int i, double sx, double sy, double ex, double ey) {
  const double ri = cs[i * 6 + 5];
  for (int j = 0; j < i; ++j) {
    const double clr = cs[j * 6 + 5] + ri + GETTING_CLOSE;
    if (norm2(sx - cs[j * 6 + 0], sy - cs[j * 6 + 1]) < clr) return true;
    if (norm2(ex - cs[j * 6 + 2], ey - cs[j * 6 + 3]) < clr) return true;
  }
  return false;
}

template <class G>  // (Rng: the sequential stream of generate_kernel; WaveRng: the same stream by position)
__device__ void draw_body(double* cs, int i, G& g, const Args& a) {  // radius, then the larger of two speed draws
  cs[i * 6 + 5] = (a.radius_hi - a.radius_lo) * g.uniform() + a.radius_lo;
  const double s1 = (a.speed_hi - a.speed_lo) * g.uniform() + a.speed_lo;
  const double s2 = (a.speed_hi - a.speed_lo) * g.uniform() + a.speed_lo;
  cs[i * 6 + 4] = fmax(s1, s2);
}

// start / end antipodal on a circle of radius r around (ox, oy); the circle grows 1 % after 11 rejections in a row
__device__ double antipodal_on_circle(double* cs, int i, double r, double ox, double oy, Rng& g, const Args& a, int& capped) {
  int rejected = 0;
  for (int it = 0;; ++it) {
    if (rejected > 10) {
      r *= 1.01;
      rejected = 0;
    }
    const double sa = g.uniform() * 2 * kPi - kPi, ea = kPi + sa;
    const double sx = r * cos(sa) + ox, sy = r * sin(sa) + oy, ex = r * cos(ea) + ox, ey = r * sin(ea) + oy;
    if (it < a.max_attempts && overlaps_earlier(cs, i, sx, sy, ex, ey)) {
      rejected += 1;
      continue;
    }
    if (it >= a.max_attempts) capped = 1;
    cs[i * 6 + 0] = sx; cs[i * 6 + 1] = sy; cs[i * 6 + 2] = ex; cs[i * 6 + 3] = ey;
    return r;
  }
}

__global__ __launch_bounds__(64) void generate_kernel(const Args a) {
  const long c = static_cast<long>(blockIdx.x) * 64 + threadIdx.x;
  if (c >= a.C) return;
  double* cs = a.cases + c * a.N * 6;  // this thread's private rows (written, then re-read by the same thread)
  Rng g;
  g.k0 = static_cast<unsigned>(a.seed); g.k1 = static_cast<unsigned>(a.seed >> 32);
  g.c2 = static_cast<unsigned>(c); g.c3 = static_cast<unsigned>(static_cast<unsigned long long>(c) >> 32);
  g.block = 0u; g.have = 0;
  int capped = 0;
  // test_cases.py:224-227: the agent count first (uniform over n_min .. n_max; slots past it stay empty: radius 0)
  int N = a.N;
  if (a.n_max > 0) {
    N = a.n_min + static_cast<int>(g.uniform() * static_cast<double>(a.n_max - a.n_min + 1));
    N = N > a.n_max ? a.n_max : N;
    for (int i = N * 6; i < a.N * 6; ++i) cs[i] = 0.0;
  }
  if (a.counts) a.counts[c] = N;
  // test_cases.py:229-241: side length drawn per case when a range is given (one draw per entry that holds the count)
  double side = a.side_lo;
  if (a.n_ranges > 0) {
    for (int r = 0; r < a.n_ranges; ++r)
      if (a.ranges[r][0] <= N && N < a.ranges[r][1]) side = a.ranges[r][2] + (a.ranges[r][3] - a.ranges[r][2]) * g.uniform();
  } else if (a.side_hi > a.side_lo) {
    side = a.side_lo + (a.side_hi - a.side_lo) * g.uniform();
  }
  const double dice = g.uniform();  // gen_rand_testcases.py:111-142: 15 % swap, 15 % circle, 70 % random
  if (dice < 0.15) {                // generate_swap_case, :322-377
    const double r_min = N / 2.0;
    double r = g.uniform() * 2.0 + r_min;
    const double r_swap = 1.5 + g.uniform() * 2.0;
    double oy = 1.0 + r_min + g.uniform() * 2.0;
    if (g.uniform() > 0.5) oy = -oy;
    for (int i = 0; i < N; ++i) {
      draw_body(cs, i, g, a);
      if (i == 0) {
        cs[0] = -r_swap; cs[1] = 0.0; cs[2] = r_swap; cs[3] = 0.0;
      } else if (i == 1) {
        cs[6] = r_swap; cs[7] = 0.0; cs[8] = -r_swap; cs[9] = 0.0;
      } else {
        r = antipodal_on_circle(cs, i, r, 0.0, oy, g, a, capped);
      }
    }
  } else if (dice > 0.15 && dice < 0.3) {  // generate_circle_case, :380-420
    double r = g.uniform() * 2.0 + N / 2.0;
    for (int i = 0; i < N; ++i) {
      draw_body(cs, i, g, a);
      r = antipodal_on_circle(cs, i, r, 0.0, 0.0, g, a, capped);
    }
  } else {  // generate_rand_case, :144-231
    for (int i = 0; i < N; ++i) {
      draw_body(cs, i, g, a);
      double sx = 0, sy = 0, ex = 0, ey = 0;
      for (int it = 0;; ++it) {
        side *= 1.01;
        sx = side * 2 * g.uniform() - side; sy = side * 2 * g.uniform() - side;
        ex = side * 2 * g.uniform() - side; ey = side * 2 * g.uniform() - side;
        if (it >= a.max_attempts) { capped = 1; break; }
        if (overlaps_earlier(cs, i, sx, sy, ex, ey)) continue;
        if (i >= 1) {  // too easy: every earlier agent can be passed by driving straight
          bool trivial = true;
          for (int j = 0; j < i && trivial; ++j) {
            const double clr = cs[j * 6 + 5] + cs[i * 6 + 5] + GETTING_CLOSE;
            if (!straight_lines_are_safe(cs[j * 6], cs[j * 6 + 1], cs[j * 6 + 2], cs[j * 6 + 3], cs[j * 6 + 4], sx, sy, ex,
                                         ey, cs[i * 6 + 4], clr))
              trivial = false;
          }
          if (trivial) continue;
        }
        if (norm2(sx - ex, sy - ey) > side * 0.5) break;
      }
      cs[i * 6 + 0] = sx; cs[i * 6 + 1] = sy; cs[i * 6 + 2] = ex; cs[i * 6 + 3] = ey;
    }
  }
  if (a.status) a.status[c] = capped;
}

// ---------------------------------------------------------------- one WAVE per case (cagpu_generate_cases_at)
// The same scenarios as generate_kernel -- same draws, same accept / reject expressions, bit for bit -- for a LIST of
// 64-bit case indices, fast when the list is short (the refill of a case stream regenerates a few percent of a table: one
// thread per case would leave a few active lanes per wave, and the launch would last as long as its slowest rejection chain).
// The stream is counter-based and an attempt consumes a fixed number of uniforms (4 in generate_rand_case, 1 in
// antipodal_on_circle), so the inputs of attempt `it` are known before attempts 0 .. it - 1 have been judged: the 64 lanes
// evaluate 64 consecutive attempts at once, the first accepting lane (ballot, first set bit) IS the sequential chain's
// accepted attempt, and the draw position behind it is where the next agent starts.  What an attempt inherits from the
// rejected ones before it -- side *= 1.01 per attempt, r *= 1.01 after 11 rejections in a row -- every lane rebuilds by the
// same sequence of multiplications (never pow, never a re-associated product: the bits must match).  Placed agents live in LDS.

// the k-th uniform of Rng's stream for (seed, case): block k >> 1, words 0-1 (even k) or 2-3 (odd k)
__device__ __forceinline__ double uniform_k(unsigned k0, unsigned k1, unsigned c2, unsigned c3, unsigned k) {
  unsigned c0 = k >> 1, c1 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = static_cast<unsigned>(p1 >> 32) ^ c1 ^ k0, n1 = static_cast<unsigned>(p1);
    const unsigned n2 = static_cast<unsigned>(p0 >> 32) ^ c3 ^ k1, n3 = static_cast<unsigned>(p0);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  const unsigned hi = (k & 1u) ? c2 : c0, lo = (k & 1u) ? c3 : c1;
  return (static_cast<double>(hi >> 5) * 67108864.0 + static_cast<double>(lo >> 6)) / 9007199254740992.0;
}

struct WaveRng {  // Rng's stream addressed by draw position; every lane of the wave holds the same `pos`
  unsigned k0, k1, c2, c3, pos;
  __device__ double at(unsigned k) const { return uniform_k(k0, k1, c2, c3, k); }
  __device__ double uniform() { return at(pos++); }
};

struct AtArgs {
  Args a;                       // a.C is not used: the list below says which cases
  const long long* case_index;  // [M]
  const long long* out_row;     // [M] or nullptr: row m
  const int32_t* count;         // device, or nullptr: M
  long M;
};

// antipodal_on_circle, 64 attempts at a time: attempt `it` has seen floor(it / 11) growths of the circle
__device__ double antipodal_on_circle_wave(double* cs, int i, double r, double ox, double oy, WaveRng& g, const Args& a,
                                           int& capped, int lane) {
  const unsigned pos0 = g.pos;
  double r_b = r;  // the radius at attempt `base`
  for (int base = 0;; base += 64) {
    const int it = base + lane;
    double rr = r_b;
    for (int j = it / 11 - base / 11; j > 0; --j) rr *= 1.01;
    const double sa = g.at(pos0 + static_cast<unsigned>(it)) * 2 * kPi - kPi, ea = kPi + sa;
    const double sx = rr * cos(sa) + ox, sy = rr * sin(sa) + oy, ex = rr * cos(ea) + ox, ey = rr * sin(ea) + oy;
    const bool cap = it >= a.max_attempts;
    const bool acc = cap || !overlaps_earlier(cs, i, sx, sy, ex, ey);
    const unsigned long long won = __ballot(acc);
    if (won != 0ull) {
      const int w = __ffsll(static_cast<long long>(won)) - 1;
      if (lane == w) { cs[i * 6 + 0] = sx; cs[i * 6 + 1] = sy; cs[i * 6 + 2] = ex; cs[i * 6 + 3] = ey; }
      if (__shfl(static_cast<int>(cap), w)) capped = 1;
      g.pos = pos0 + static_cast<unsigned>(base + w) + 1u;
      return __shfl(rr, w);
    }
    for (int j = (base + 64) / 11 - base / 11; j > 0; --j) r_b *= 1.01;
  }
}

__global__ __launch_bounds__(64) void generate_at_kernel(const AtArgs q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gen_smem[];
  double* cs = reinterpret_cast<double*>(gen_smem);  // [a.N, 6]: the agents placed so far
  const Args& a = q.a;
  const int lane = threadIdx.x;
  long cnt = q.M;
  if (q.count) {
    const long v = *q.count;
    cnt = v < 0 ? 0 : (v < q.M ? v : q.M);
  }
  for (long m = blockIdx.x; m < cnt; m += gridDim.x) {  // (uniform per wave: the barriers below are safe)
    const unsigned long long c = static_cast<unsigned long long>(q.case_index[m]);
    const long row = q.out_row ? static_cast<long>(q.out_row[m]) : m;
    WaveRng g;
    g.k0 = static_cast<unsigned>(a.seed); g.k1 = static_cast<unsigned>(a.seed >> 32);
    g.c2 = static_cast<unsigned>(c); g.c3 = static_cast<unsigned>(c >> 32);
    g.pos = 0u;
    int capped = 0;
    // the draws ahead of the agents: every lane computes them (uniform values), as generate_kernel does
    int N = a.N;
    if (a.n_max > 0) {
      N = a.n_min + static_cast<int>(g.uniform() * static_cast<double>(a.n_max - a.n_min + 1));
      N = N > a.n_max ? a.n_max : N;
    }
    double side = a.side_lo;
    if (a.n_ranges > 0) {
      for (int r = 0; r < a.n_ranges; ++r)
        if (a.ranges[r][0] <= N && N < a.ranges[r][1]) side = a.ranges[r][2] + (a.ranges[r][3] - a.ranges[r][2]) * g.uniform();
    } else if (a.side_hi > a.side_lo) {
      side = a.side_lo + (a.side_hi - a.side_lo) * g.uniform();
    }
    const double dice = g.uniform();
    if (dice < 0.15) {  // generate_swap_case
      const double r_min = N / 2.0;
      double r = g.uniform() * 2.0 + r_min;
      const double r_swap = 1.5 + g.uniform() * 2.0;
      double oy = 1.0 + r_min + g.uniform() * 2.0;
      if (g.uniform() > 0.5) oy = -oy;
      for (int i = 0; i < N; ++i) {
        draw_body(cs, i, g, a);  // (every lane stores the same values)
        if (i == 0) {
          cs[0] = -r_swap; cs[1] = 0.0; cs[2] = r_swap; cs[3] = 0.0;
        } else if (i == 1) {
          cs[6] = r_swap; cs[7] = 0.0; cs[8] = -r_swap; cs[9] = 0.0;
        }
        __syncthreads();
        if (i >= 2) {
          r = antipodal_on_circle_wave(cs, i, r, 0.0, oy, g, a, capped, lane);
          __syncthreads();
        }
      }
    } else if (dice > 0.15 && dice < 0.3) {  // generate_circle_case
      double r = g.uniform() * 2.0 + N / 2.0;
      for (int i = 0; i < N; ++i) {
        draw_body(cs, i, g, a);
        __syncthreads();
        r = antipodal_on_circle_wave(cs, i, r, 0.0, 0.0, g, a, capped, lane);
        __syncthreads();
      }
    } else {  // generate_rand_case: attempt `it` runs on the side after it + 1 growths
      for (int i = 0; i < N; ++i) {
        draw_body(cs, i, g, a);
        __syncthreads();
        const unsigned pos0 = g.pos;
        double side_b = side;  // the side BEFORE attempt `base` grows it
        for (int base = 0;; base += 64) {
          const int it = base + lane;
          double s = side_b;
          for (int j = 0; j <= lane; ++j) s *= 1.01;
          const unsigned p = pos0 + 4u * static_cast<unsigned>(it);
          const double sx = s * 2 * g.at(p) - s, sy = s * 2 * g.at(p + 1u) - s;
          const double ex = s * 2 * g.at(p + 2u) - s, ey = s * 2 * g.at(p + 3u) - s;
          const bool cap = it >= a.max_attempts;
          bool acc = cap;
          if (!cap && !overlaps_earlier(cs, i, sx, sy, ex, ey)) {
            bool trivial = i >= 1;  // too easy: every earlier agent can be passed by driving straight
            for (int j = 0; j < i && trivial; ++j) {
              const double clr = cs[j * 6 + 5] + cs[i * 6 + 5] + GETTING_CLOSE;
              if (!straight_lines_are_safe(cs[j * 6], cs[j * 6 + 1], cs[j * 6 + 2], cs[j * 6 + 3], cs[j * 6 + 4], sx, sy, ex,
                                           ey, cs[i * 6 + 4], clr))
                trivial = false;
            }
            acc = !trivial && norm2(sx - ex, sy - ey) > s * 0.5;
          }
          const unsigned long long won = __ballot(acc);
          if (won != 0ull) {
            const int w = __ffsll(static_cast<long long>(won)) - 1;
            if (lane == w) { cs[i * 6 + 0] = sx; cs[i * 6 + 1] = sy; cs[i * 6 + 2] = ex; cs[i * 6 + 3] = ey; }
            if (__shfl(static_cast<int>(cap), w)) capped = 1;
            side = __shfl(s, w);
            g.pos = pos0 + 4u * static_cast<unsigned>(base + w + 1);
            break;
          }
          side_b = __shfl(s, 63);
        }
        __syncthreads();
      }
    }
    __syncthreads();
    double* dst = a.cases + row * a.N * 6;
    for (int idx = lane; idx < a.N * 6; idx += 64) dst[idx] = idx < N * 6 ? cs[idx] : 0.0;  // (slots past the count stay empty)
    if (lane == 0) {
      if (a.counts) a.counts[row] = N;
      if (a.status) a.status[row] = capped;
    }
    __syncthreads();  // (the next case of this wave reuses the LDS rows)
  }
}

// ---------------------------------------------------------------- the refill of a case stream (cagpu_stream_refill)
// One thread per (env, window slot): the slot of env e that episode k lands in is k % W, and after this kernel it holds the
// one episode of rc + 1 .. rc + W with that residue (rc = reset_count[e]).  Stale slots are compacted into the work list --
// a ballot and ONE atomic per wave; the list's order is unspecified and does not matter (every entry names its own row) --
// and generate_at_kernel then runs over the list with the count read on the device.
struct RefillArgs {
  int E, W;
  long long env_id_offset;
  const int32_t* reset_count;
  int32_t *held, *seen;
  long long *work_index, *work_row;
  int32_t* work_count;
};

__global__ __launch_bounds__(256) void stream_refill_kernel(const RefillArgs q) {
  const long t = static_cast<long>(blockIdx.x) * 256 + threadIdx.x;
  const long total = static_cast<long>(q.E) * q.W;
  bool stale = false;
  long long index = 0, row = 0;
  if (t < total) {
    const int e = static_cast<int>(t / q.W), j = static_cast<int>(t % q.W);
    const int rc = q.reset_count[e];
    // the episode of rc + 1 .. rc + W whose residue is j
    int d = (j - (rc + 1)) % q.W;
    if (d < 0) d += q.W;
    const int k = rc + 1 + d;
    if (q.held[t] != k) {
      stale = true;
      q.held[t] = k;
      const long long g = q.env_id_offset + e;
      index = static_cast<long long>((static_cast<unsigned long long>(g) << 32) | static_cast<unsigned>(k));
      row = (g + static_cast<long long>(j) * q.E) % total;  // = (env_id_offset + e + k * E) % (E * W)
    }
    if (j == 0) {  // (one thread per env reads and stamps `seen`)
      if (rc - q.seen[e] > q.W) atomicOr(&g_fault, 8u);  // overrun: the env loaded a slot that still held an older episode (fault word bit 3)
      q.seen[e] = rc;
    }
  }
  const unsigned long long mask = __ballot(stale);
  if (mask != 0ull) {
    const int lane = threadIdx.x & 63;
    int base = 0;
    const int first = __ffsll(static_cast<long long>(mask)) - 1;
    if (lane == first) base = atomicAdd(q.work_count, __popcll(mask));
    base = __shfl(base, first);
    if (stale) {
      const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
      q.work_index[at] = index;
      q.work_row[at] = row;
    }
  }
}

}  // namespace gen
