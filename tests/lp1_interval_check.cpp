// tests/lp1_interval_check.cpp -- stand-alone host program of tests/test_lp1_interval_host.py.
// lp1_interval_pair (csrc/cagpu_lp1.inc) against the text of p2b_round it replaced: the same (t_lo, t_hi) WORDS for every input.
// Exit status 0: no difference.  Last line: "lp1-interval grid G random R differing D <counter> <n> ...".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#define CAGPU_HD inline
#include "cagpu_lp1.inc"

// the interval update of p2b_round as it stood before lp1_interval_pair (verbatim, the loop's own names)
static void reference(const bool use0, const bool use1, const float den0, const float den1, const float tt0, const float tt1,
                      float& t_lo, float& t_hi) {
  const bool par0 = fabsf(den0) <= kRvoEps, par1 = fabsf(den1) <= kRvoEps;
  const float h0 = (use0 && !par0 && den0 >= 0.0f) ? tt0 : INFINITY;
  const float h1 = (use1 && !par1 && den1 >= 0.0f) ? tt1 : INFINITY;
  const float o0 = (use0 && !par0 && den0 < 0.0f) ? tt0 : -INFINITY;
  const float o1 = (use1 && !par1 && den1 < 0.0f) ? tt1 : -INFINITY;
  const float hh = (h1 < h0) ? h1 : h0, oo = (o0 < o1) ? o1 : o0;
  t_hi = (hh < t_hi) ? hh : t_hi;
  t_lo = (t_lo < oo) ? oo : t_lo;
}

static uint32_t bits(const float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static float from_bits(const uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

struct Stats {
  long n = 0, differing = 0, nan_tt0_present = 0, ties = 0, den_at_eps = 0, use1_false = 0, changed = 0;
};

static void one(Stats& st, const bool use0, const bool use1, const float den0, const float den1, const float tt0, const float tt1,
                const float lo, const float hi) {
  float rl = lo, rh = hi, gl = lo, gh = hi;
  reference(use0, use1, den0, den1, tt0, tt1, rl, rh);
  lp1_interval_pair(use0, use1, den0, den1, tt0, tt1, gl, gh);
  st.n += 1;
  const bool present0 = use0 && !(fabsf(den0) <= kRvoEps) && (den0 >= 0.0f || den0 < 0.0f);
  st.nan_tt0_present += present0 && tt0 != tt0;
  st.ties += present0 && (tt0 == hi || tt0 == lo || (use1 && tt0 == tt1));
  st.den_at_eps += fabsf(den0) == kRvoEps || fabsf(den1) == kRvoEps;
  st.use1_false += !use1;
  st.changed += bits(rl) != bits(lo) || bits(rh) != bits(hi);
  if (bits(rl) != bits(gl) || bits(rh) != bits(gh)) {
    if (st.differing < 20)
      std::printf("DIFF use %d %d den %08x %08x tt %08x %08x lo %08x hi %08x: reference (%08x, %08x) rule (%08x, %08x)\n", use0, use1,
                  bits(den0), bits(den1), bits(tt0), bits(tt1), bits(lo), bits(hi), bits(rl), bits(rh), bits(gl), bits(gh));
    st.differing += 1;
  }
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float e = kRvoEps;
  const std::vector<float> vals = {0.0f, -0.0f, 1.0f, -1.0f, std::nextafter(1.0f, 2.0f), std::nextafter(-1.0f, -2.0f), 2.5f,
                                   -2.5f, inf, -inf, nan, from_bits(0xffc00001u)};
  const std::vector<float> dens = {0.0f, -0.0f, e, -e, std::nextafter(e, 1.0f), std::nextafter(e, 0.0f), -std::nextafter(e, 1.0f),
                                   -std::nextafter(e, 0.0f), 5e-6f, -5e-6f, 1.0f, -1.0f, inf, -inf, nan};
  Stats grid;
  for (int u = 0; u < 4; ++u)
    for (const float d0 : dens)
      for (const float d1 : dens)
        for (const float a : vals)
          for (const float b : vals)
            for (const float lo : vals)
              for (const float hi : vals) one(grid, u & 1, (u & 2) != 0, d0, d1, a, b, lo, hi);

  Stats rnd;
  uint64_t s = 0x9e3779b97f4a7c15ull;
  const auto next = [&]() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return static_cast<uint32_t>(s >> 16);
  };
  std::vector<float> pool = vals;
  pool.insert(pool.end(), dens.begin(), dens.end());
  for (long k = 0; k < (1l << 21); ++k) {
    float f[6];
    for (float& x : f) x = (k & 1) ? pool[next() % pool.size()] : from_bits(next());
    const uint32_t u = next();
    one(rnd, u & 1, (u & 2) != 0, f[0], f[1], f[2], f[3], f[4], f[5]);
  }
  std::printf("lp1-interval grid %ld random %ld differing %ld nan_tt0_present %ld ties %ld den_at_eps %ld use1_false %ld changed %ld\n",
              grid.n, rnd.n, grid.differing + rnd.differing, grid.nan_tt0_present + rnd.nan_tt0_present, grid.ties + rnd.ties,
              grid.den_at_eps + rnd.den_at_eps, grid.use1_false + rnd.use1_false, grid.changed + rnd.changed);
  return (grid.differing + rnd.differing) ? 1 : 0;
}
