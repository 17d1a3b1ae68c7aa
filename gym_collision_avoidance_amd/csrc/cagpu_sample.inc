// gym_collision_avoidance_amd/csrc/cagpu_sample.inc -- included by cagpu.hip (inside its anonymous namespace, after
// cagpu_replay.inc).
//
// On-policy data for the GA3C-CADRL network without the host: the sampled policy (CaGa3cSample in cagpu.h states the rule;
// sample_kernel is a launch of its own between the network launch and the step, sample_at_kernel the same rule for
// arbitrary addresses), the pre-step half of an experience tape slot, and generalised advantage estimation over a tape
// (gae_kernel).  No network kernel and no step kernel is touched: both kernels here read what those wrote.
namespace sample {

constexpr int NL = 11;    // logits per row (network.Actions)
constexpr int NT = 256;   // threads per workgroup: one lane per agent / address / (env, agent) column

struct Row {
  int index;       // the index that is played
  float logp, entropy;
  bool bad;        // a NaN logit
};
// The rule of CaGa3cSample for one row, float32, every product and sum rounded on its own (the library is built with
// -ffp-contract=off; the intrinsics say so where a contraction would otherwise be legal).  `draw`: the agent samples with
// the uniform u; otherwise it plays `held`, the first maximum of the row (what the network kernel wrote).
__device__ __forceinline__ Row sample_row(const float (&l)[NL], const bool draw, const double u, const float inv_T) {
  bool bad = false;
  float m = l[0];
  int held = 0;
#pragma unroll
  for (int j = 0; j < NL; ++j) bad |= (l[j] != l[j]);
#pragma unroll
  for (int j = 1; j < NL; ++j)
    if (l[j] > m) {  // ties -> first, like np.argmax and ga3c_kernel
      m = l[j];
      held = j;
    }
  float z[NL], q[NL], c[NL];
  float run = 0.f, wsum = 0.f;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    z[j] = __fmul_rn(__fsub_rn(l[j], m), inv_T);
    q[j] = expf(z[j]);
    run = __fadd_rn(run, q[j]);
    c[j] = run;
    wsum = __fadd_rn(wsum, __fmul_rn(q[j], z[j]));
  }
  const float S = c[NL - 1];
  int idx = held;
  if (draw) {
    const float x = __fmul_rn(static_cast<float>(u), S);
    idx = NL - 1;
#pragma unroll
    for (int j = NL - 2; j >= 0; --j)
      if (x < c[j]) idx = j;  // the FIRST j with u S < c_j
  }
  float zi = z[0];
#pragma unroll
  for (int j = 1; j < NL; ++j) zi = (idx == j) ? z[j] : zi;
  const float ls = logf(S);
  Row r;
  r.bad = bad;
  r.index = bad ? (draw ? 0 : held) : idx;
  r.logp = bad ? __builtin_nanf("") : __fsub_rn(zi, ls);
  r.entropy = bad ? __builtin_nanf("") : __fsub_rn(ls, wsum / S);
  return r;
}

struct Args {
  unsigned long long seed;   // 0 with greedy
  float inv_T;
  int greedy;
  const uint8_t* mask;       // [B] or nullptr = every evaluated agent
  const int32_t* agent_net;  // [B] or nullptr
  int32_t net_index;
  const int64_t* address;    // [2 E] or nullptr
  const float* logits;       // [B, 11]
  const uint32_t* flags;     // [B]
  const int32_t *step_num, *reset_count;  // [B], [E]
  long env_id_offset;
  long B;
  int N, W;
  double* ext;               // [B, 2]
  float *logp, *entropy;     // [B]; entropy may be nullptr
  int8_t* action;            // [B] or nullptr
  // the pre-step half of a tape slot (all nullable)
  const float* obs;          // [B, W]: the rows the network read
  const float* value;        // [B]: what the value head wrote
  float* slot_obs;           // [B, W - 1]
  float* slot_value;         // [B]
  uint8_t* slot_live;        // [B]: written for EVERY slot
  int64_t* slot_address;     // [E, 2]
};

__global__ __launch_bounds__(NT) void sample_kernel(const Args d) {
  const long i = static_cast<long>(blockIdx.x) * NT + threadIdx.x;
  const bool in = i < d.B;
  const long ic = in ? i : d.B - 1;  // (clamped: no load sits behind the bounds branch)
  const uint32_t f = d.flags[ic];
  bool ev = in && !(f & CA_ABSENT) && ga3c::needs_action(f);
  if (d.agent_net) ev = ev && d.agent_net[ic] == d.net_index;
  float l[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) l[j] = d.logits[ic * NL + j];  // the 11 loads together
  const long e = ic / d.N;
  const int a = static_cast<int>(ic - e * d.N);
  const unsigned long long g = static_cast<unsigned long long>(d.address ? d.address[2 * e] : d.env_id_offset + e);
  const unsigned k = d.address ? static_cast<unsigned>(d.address[2 * e + 1]) : static_cast<unsigned>(d.reset_count[e]);
  const int s = d.step_num[ic];
  const bool draw = ev && !d.greedy && (!d.mask || d.mask[ic] != 0);
  if (d.slot_live && in) d.slot_live[i] = ev ? 1 : 0;
  if (d.slot_address && in && a == 0) {
    d.slot_address[2 * e] = static_cast<int64_t>(g);
    d.slot_address[2 * e + 1] = static_cast<int64_t>(k);
  }
  if (ev) {
    double u = 0.0;
    if (draw) u = gen::uniform_at(d.seed, static_cast<unsigned>(g), static_cast<unsigned>(g >> 32), k, rvo_word3(a, s));
    const Row r = sample_row(l, draw, u, d.inv_T);
    if (r.bad) atomicOr(&g_fault, 32u);
    if (draw) {
      d.ext[2 * i] = static_cast<double>(r.index);
      d.ext[2 * i + 1] = 0.0;
    }
    d.logp[i] = r.logp;
    if (d.entropy) d.entropy[i] = r.entropy;
    if (d.action) d.action[i] = static_cast<int8_t>(r.index);
    if (d.slot_value) d.slot_value[i] = d.value[i];
  }
  // the observation rows of the evaluated agents, a wave at a time: 64 consecutive floats of a row per instruction, the
  // loads of RB rows in flight together (one row at a time the copy waits a memory latency per 256 bytes: 51 us of a
  // 4096 x 20 step, 24 us at 256 x 4)
  if (d.slot_obs) {
    constexpr int RB = 8;
    unsigned long long todo = __ballot(ev);  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const long base = i - lane;  // the wave's first agent
    const int w1 = d.W - 1;
    const float* __restrict__ obs = d.obs;
    float* __restrict__ out = d.slot_obs;
    while (todo) {
      long row[RB];
      int cnt = 0;
#pragma unroll
      for (int q = 0; q < RB; ++q) {
        if (todo) {
          row[q] = base + __ffsll(static_cast<long long>(todo)) - 1;
          todo &= todo - 1;
          cnt = q + 1;
        } else {
          row[q] = row[0];  // (loaded again, not stored)
        }
      }
      for (int c = lane; c < w1; c += 64) {
        float v[RB];
#pragma unroll
        for (int q = 0; q < RB; ++q) v[q] = obs[row[q] * d.W + 1 + c];
#pragma unroll
        for (int q = 0; q < RB; ++q)
          if (q < cnt) out[row[q] * w1 + c] = v[q];
      }
    }
  }
}

// cagpu_ga3c_sample_at: the rule for n arbitrary (g, k, a, s, logits row), every row sampling
struct AtArgs {
  unsigned long long seed;
  float inv_T;
  const int64_t* g;
  const int32_t *k, *a, *s;
  const float* logits;  // [n, 11]
  long n;
  int8_t* action;
  float *logp, *entropy;  // nullable, each
};
__global__ __launch_bounds__(NT) void sample_at_kernel(const AtArgs d) {
  const long i = static_cast<long>(blockIdx.x) * NT + threadIdx.x;
  if (i >= d.n) return;
  float l[NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) l[j] = d.logits[i * NL + j];
  const unsigned long long g = static_cast<unsigned long long>(d.g[i]);
  const double u = gen::uniform_at(d.seed, static_cast<unsigned>(g), static_cast<unsigned>(g >> 32), static_cast<unsigned>(d.k[i]),
                                   rvo_word3(d.a[i], d.s[i]));
  const Row r = sample_row(l, true, u, d.inv_T);
  if (r.bad) atomicOr(&g_fault, 32u);
  if (d.action) d.action[i] = static_cast<int8_t>(r.index);
  if (d.logp) d.logp[i] = r.logp;
  if (d.entropy) d.entropy[i] = r.entropy;
}

// cagpu_gae: one lane per (env, agent) column walks the tape from its last slot to its first; a step's loads are
// consecutive across the lanes, and those of step t - 1 are in flight while step t computes.  cagpu.h has the rule.
struct GaeArgs {
  int n;
  long EN;
  int N;
  const float *reward, *value, *last_value;
  const uint8_t *live, *done, *game_over;
  float gamma, gl;
  float *adv, *ret;
};
struct GaeIn {
  float r, v;
  uint8_t live, end;
};
__device__ __forceinline__ GaeIn gae_load(const GaeArgs& d, const int t, const long i, const long e) {
  const long o = static_cast<long>(t) * d.EN + i;
  GaeIn x;
  x.r = d.reward[o];
  x.v = d.value[o];
  x.live = d.live[o];
  x.end = d.done[o] | d.game_over[static_cast<long>(t) * (d.EN / d.N) + e];
  return x;
}
__global__ __launch_bounds__(NT) void gae_kernel(const GaeArgs d) {
  const long i = static_cast<long>(blockIdx.x) * NT + threadIdx.x;
  if (i >= d.EN) return;
  const long e = i / d.N;
  float carry = 0.f, nv = d.last_value[i];
  GaeIn cur = gae_load(d, d.n - 1, i, e);
  for (int t = d.n - 1; t >= 0; --t) {
    GaeIn nxt = cur;
    if (t > 0) nxt = gae_load(d, t - 1, i, e);
    const long o = static_cast<long>(t) * d.EN + i;
    float adv = 0.f, ret = 0.f;
    if (!cur.live) {
      carry = 0.f;
      nv = 0.f;
    } else {
      if (cur.end) {  // the agent's episode ended in step t: terminal
        nv = 0.f;
        carry = 0.f;
      }
      const float delta = __fsub_rn(__fadd_rn(cur.r, __fmul_rn(d.gamma, nv)), cur.v);
      carry = __fadd_rn(delta, __fmul_rn(d.gl, carry));
      adv = carry;
      ret = __fadd_rn(adv, cur.v);
      nv = cur.v;
    }
    d.adv[o] = adv;
    d.ret[o] = ret;
    cur = nxt;
  }
}

}  // namespace sample
