// gym_collision_avoidance_amd/csrc/cagpu_ga3c.inc -- GA3C-CADRL policy network on the matrix cores.
//
// Replaces GA3CCADRLPolicy.find_next_action (policies/GA3CCADRLPolicy.py:49-84) + the TF1 graph of
// GA3C_CADRL/checkpoints/*/network_*.meta (node names in the comments below; decoded by oracle/extract_ga3c_weights.py).
//
// One workgroup = up to 64 agents (rows) x 4 waves, the whole network per tile with the activations in LDS (float32).
//   * The float32 contractions run on the F16 matrix cores (16 x the rate of the f32 MFMA on gfx950) with float32-class
//     operands: a float32 x is carried as two fp16 planes, hi = fp16(x) and lo = fp16(x - hi) (22 of its 24 significant
//     bits; fp16 denormals are produced by the conversion and multiplied by the MFMA: measured), and a product a * b as the
//     three plane products lo*hi + hi*lo + hi*hi, each exact in the matrix core's f32 accumulate (v_mfma_f32_16x16x32_f16);
//     the dropped lo*lo is below 2^-22 of the product (an f32 multiply rounds at 2^-24; the sum over k is accumulated in
//     f32 either way).  (Rounds 2 - 4: three bf16 planes and six products -- twice the matrix work for the same accuracy.)
//     Weights are split once, on the device, into fragment order (cagpu_ga3c_pack -> CaNet.packed); activations are split
//     by the lane that loads them.
//   * TRANSPOSED products, D[unit][row] = sum_k W[k][unit] * X[row][k]: the weights are the MFMA's A operand, the tile's
//     rows its B operand, so a lane's four results are four CONSECUTIVE units of one row -- one 16-byte LDS store, and for
//     the LSTM the i, j, f, o pre-activations of the same (row, unit) in the same lane: the cell update is lane-local and
//     c never leaves registers.
//   * LSTM: wave w owns hidden units 16w..16w+15 and keeps the split weight fragments of their four gates (h part, K = 64)
//     in registers for all 19 steps; the 7 inputs x_t and the bias ride on one more f16 MFMA per gate (K = 32 as groups
//     of 8), NOT on the f32 MFMA, which blocks the SIMD's VALU (measured).  The dense layers stream their packed fragments
//     from L2 (0.63 MB, shared by every workgroup), one k-block prefetched ahead of the MFMAs; layer1's 4 host inputs and the
//     11 logits stay on the f32 MFMA.  The order of issue of the LSTM step and of layer2 / fc1 is placed by hand (below).
namespace ga3c {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr int TM = 64;        // agents per workgroup
constexpr int NT = 256;       // 4 waves
constexpr int NO = 19;        // other-agent slots the LSTM is unrolled over (Reshape/shape = [-1, 19, 7])
constexpr int XIN = 138;      // width of placeholder X
constexpr int XO_LD = 137;    // normalised other-agent block (133 columns); odd stride: conflict-free column reads
constexpr int HP_LD = 72;     // one fp16 plane of h: 64 units + pad = 144-byte rows, conflict-free 16-byte reads
constexpr int NPL = 2;        // planes a float32 operand is split into: hi = fp16(x), lo = fp16(x - hi)
constexpr int HP_PLANE = TM * HP_LD / 2;  // floats (= dwords) per plane
constexpr int ACT_LD = 260;   // 256-wide activations, leading dimension chosen for conflict-free 16-byte reads
constexpr int XS_RING = 2;                       // steps the staging buffer of x planes holds: this one's and the next one's
constexpr int XS_FLOATS = XS_RING * NPL * TM * 4;  // the planes of x_t: [buffer][plane][row][8] fp16
constexpr int LSTM_FLOATS = TM * XO_LD + NPL * HP_PLANE + XS_FLOATS, DENSE_FLOATS = TM * ACT_LD + TM * 16;
constexpr int UNION_FLOATS = LSTM_FLOATS > DENSE_FLOATS ? LSTM_FLOATS : DENSE_FLOATS;
// CaNet.packed: the fp16 planes of the four big weight matrices in MFMA fragment order, uint4 (8 fp16) per lane:
//   index = ((kb * 16 + cb) * NPL + plane) * 64 + lane;   lane (m, q) holds W[kb * 32 + 8 q + e][cb * 16 + m], e = 0..7
constexpr int PK_LSTM = 0;                          // rnn/lstm_cell/kernel rows 7..70 (h part), K = 64
constexpr int PK_L1 = PK_LSTM + 2 * 16 * NPL * 64;  // layer1/kernel rows 4..67 (h part), K = 64
constexpr int PK_L2 = PK_L1 + 2 * 16 * NPL * 64;    // layer2/kernel, K = 256
constexpr int PK_FC1 = PK_L2 + 8 * 16 * NPL * 64;   // fullyconnected1/kernel, K = 256
constexpr int PK_TOTAL = PK_FC1 + 8 * 16 * NPL * 64;  // 40 960 uint4 = 655 360 bytes
constexpr int MISC = 4;   // [1] / [2]: longest / shortest sequence of the tile
constexpr size_t LDS_BYTES = (TM * 4 + TM + MISC + UNION_FLOATS) * sizeof(float);

struct Args {
  const float* obs;       // [B, W]
  const uint32_t* flags;  // [B]
  long B;
  int W;
  CaNet net;
  double* ext;    // [B, 2]
  float* logits;  // [B, 11] or nullptr
  const int32_t* rows;  // packed list of the rows to evaluate + their count at [B] (compact_kernel), or nullptr
  int slots;            // workgroups resident at once (2 per CU): the tile height is chosen against it
  int force_tile;       // 0 = balanced per-tile heights (what the launchers pass), or 32 / 48 / 64 for every tile
  // FUSED SENSING (obs == nullptr): the kernel computes each evaluated agent's ego-centric observation itself from the
  // simulator state -- OtherAgentsStatesSensor.sense + the observation assembly (OtherAgentsStatesSensor.py:58-144,
  // agent.py:323-327) for exactly the rows the network reads -- instead of fetching the row the step kernel stored
  const double *pos_x, *pos_y, *vel_x, *vel_y, *heading, *goal_x, *goal_y, *radius, *pref_speed;
  int N, K, obs_clip, sort_mode, ragged;
  double sensing_horizon;
};
// What cagpu_ga3c_query / cagpu_ga3c_value add (ga3c_kernel<true> only; the default launch carries none of it).
//   query: the rows are ALL B rows of the plain array Args.obs [B, W - 1] -- the policy vector X itself (no is_learning column
//   ahead of it: Args.W stays "X's width + 1"), no flag words, no packed list; value_kernel / value_bias: logits_v, the
//   twelfth column of the padded logits block (nullptr: the column stays zero); value [B], action [B]: nullable outputs.
struct Ext {
  const float *value_kernel, *value_bias;
  float* value;
  int32_t* action;
  int query;
};

// Who needs an action: GA3C-CADRL agents that are not done (collision_avoidance_env.py:310-312)
__device__ __forceinline__ bool needs_action(uint32_t f) {
  return ((f >> CA_POLICY_SHIFT) & 0xF) == CA_POL_GA3C_CADRL && !(f & CA_DONE);
}

// Packs the indices of the rows that need an action into rows[0 .. count) and the count into rows[B].  Every workgroup
// ranks 4 * CP_NT rows (16 bytes of flags per thread, coalesced): the exclusive prefix of the per-thread counts (0 .. 4)
// comes from three wave ballots (one per bit of the count) and an LDS table of the waves' totals; ONE atomicAdd per
// workgroup on a running total reserves the workgroup's slots.  Rows stay ascending inside a workgroup's range; the
// ranges land in the order the workgroups arrive, which is immaterial: a row's result does not depend on the tile it
// is evaluated in (tests/test_gpu_parity.py::test_ga3c_*).  The last workgroup to finish publishes the total as rows[B].
// The two counters (running total, workgroups done) are 64-bit words behind the list, each TAGGED with the call's epoch in
// its upper half: a word whose tag is not this call's counts as zero (tagged_add), so nothing has to be cleared -- not by a
// memset ahead of the launch (4.9 us of a config-3 step while there was one), not by the last workgroup -- and whatever an
// aborted launch or an uninitialised scratch left there is ignored (a stale tag equals a fresh epoch with probability 2^-32).
// 82 k agents: 80 workgroups, ~4 us (round 2's single workgroup walked all the flags in 25 us, 6 % of a config-3 step).
constexpr int CP_NT = 256;
__device__ __forceinline__ unsigned long long* compact_counters(int32_t* rows, const long B) {  // 8-byte aligned, <= rows + B + 2
  return reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(rows + B + 1) + 7) & ~static_cast<uintptr_t>(7));
}
// *w += add among the callers of ONE epoch; returns the value before (0 for the first caller of the epoch).  Once the word
// carries the epoch's tag it is a plain atomicAdd (no retries: 80 workgroups arriving together on a compare-and-swap loop
// serialised into 35 us of round trips across the XCDs); only the first arrivals race for the swap that installs the tag.
__device__ __forceinline__ uint32_t tagged_add(unsigned long long* w, const uint32_t epoch, const uint32_t add) {
  for (;;) {
    const unsigned long long old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (static_cast<uint32_t>(old >> 32) == epoch)  // (from here on only adds of this epoch change the word)
      return static_cast<uint32_t>(atomicAdd(w, static_cast<unsigned long long>(add)));
    if (atomicCAS(w, old, (static_cast<unsigned long long>(epoch) << 32) + add) == old) return 0u;
  }
}
__global__ __launch_bounds__(CP_NT) void compact_kernel(const uint32_t* __restrict__ flags, long B, int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ agent_net, const int32_t net_index,
                                                        const uint32_t epoch) {
  __shared__ int wtot[CP_NT / 64];
  __shared__ int wg_base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  const long r0 = (static_cast<long>(blockIdx.x) * CP_NT + tid) * 4;
  uint32_t f[4] = {CA_DONE, CA_DONE, CA_DONE, CA_DONE};  // (a done flag: needs no action)
  if (r0 + 3 < B && (reinterpret_cast<uintptr_t>(flags) & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(flags + r0);
    f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (r0 + u < B) f[u] = flags[r0 + u];
  }
  int nd[4], c = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    nd[u] = (needs_action(f[u]) && (!agent_net || agent_net[r0 + u] == net_index)) ? 1 : 0;  // (needs_action: r0 + u < B)
    c += nd[u];
  }
  const unsigned long long b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
  const int before = __popcll(b0 & lt) + 2 * __popcll(b1 & lt) + 4 * __popcll(b2 & lt);
  if (lane == 0) wtot[wv] = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
  __syncthreads();
  int off = before, total = 0;
#pragma unroll
  for (int w = 0; w < CP_NT / 64; ++w) {
    const int t = wtot[w];
    off += (w < wv) ? t : 0;
    total += t;
  }
  unsigned long long* cnt = compact_counters(rows, B);  // [0] rows reserved so far, [1] workgroups done
  if (tid == 0) wg_base = total ? static_cast<int>(tagged_add(&cnt[0], epoch, static_cast<uint32_t>(total))) : 0;
  __syncthreads();
  off += wg_base;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (nd[u]) rows[off++] = static_cast<int32_t>(r0 + u);
  // the last workgroup publishes the count (every slot reservation above happened before its workgroup's arrival here)
  // (no __threadfence(): at agent scope it is a write-back + invalidate of the L2.  What has to be ordered is this
  // workgroup's slot reservation before its arrival ticket -- two device-scope atomics of the same thread, the first has
  // returned (wg_base) before the second is issued; the list itself is read by the NEXT kernel)
  if (tid == 0) {
    if (tagged_add(&cnt[1], epoch, 1u) == gridDim.x - 1u) {
      const unsigned long long all = __hip_atomic_load(&cnt[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      rows[B] = (static_cast<uint32_t>(all >> 32) == epoch) ? static_cast<int32_t>(static_cast<uint32_t>(all)) : 0;
    }
  }
}

// Rows per workgroup tile: 64, 48 or 32 (whole 16-row MFMA blocks), chosen PER TILE.  With the packed list the row count
// is whatever is alive, and one height for the whole launch quantises coarsely: a round of resident tiles (512 slots = 2
// workgroups per CU) costs 297 / 225 / 160 us for 64 / 48 / 32 rows (one forced height per launch, 4096 x 20: a fixed part --
// weights from L2, barriers -- plus ~4.3 us per row of the CU's two tiles), so 26 .. 32 k rows all cost one full round of
// 64-row tiles (profiles/r04_ga3c_rows.json: 310 .. 317 us flat), although 26 k rows are 19 % less work.  Balanced plan:
// the launch takes R = ceil(rows / (64 * slots)) rounds whatever the heights, so spread the rows' 16-row blocks EVENLY
// over the R * slots tiles of those rounds: `rem` tiles of lo + 1 blocks first (the dispatcher starts them first and pairs
// tile t with tile t + 256 on a CU), the others lo blocks.  Every CU then carries the same number of rows (+- 16) and the
// launch time follows the row count instead of its staircase.  Fewer than 2 blocks per tile: uniform 32-row tiles
// (fewer workgroups than slots; a 16-row tile would pay the fixed part for a quarter of the matrix work).
struct Tile {
  int tm;     // rows of this tile (workgroup-uniform)
  long row0;  // its first row in the packed list
};
__device__ __forceinline__ Tile tile_of(const long n_rows, const int slots, const int force_tile, const long t) {
  if (force_tile) return Tile{force_tile, t * force_tile};  // (one height for the launch; the launchers pass 0)
  const long blocks = (n_rows + 15) >> 4;
  if (blocks == 0) return Tile{32, t * 32};  // nothing is alive: every workgroup leaves at once
  const long rounds = (blocks + 4L * slots - 1) / (4L * slots);
  const long tiles = rounds * slots;
  const long lo = blocks / tiles, rem = blocks - lo * tiles;  // (lo == 4 only with rem == 0)
  if (lo < 2) return Tile{32, t * 32};
  return Tile{static_cast<int>(16 * (lo + (t < rem ? 1 : 0))), 16 * (t * lo + (t < rem ? t : rem))};
}

// Gate non-linearities on the hardware transcendental units: exp(x) = v_exp_f32(x * log2 e), 1 / y = v_rcp_f32 (both
// ~1 ulp), i.e. ~5 instructions per sigmoid instead of ~25 for expf + a correctly rounded divide.  With 5 of them per
// LSTM element the accurate forms made the VALU, not the matrix cores, the LSTM's bottleneck (980 -> see profiles/).
// Error ~3e-7 relative, far inside the parity bar on the logits (2e-4).
__device__ __forceinline__ float sigmoidf(float x) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.44269504088896341f));
}
__device__ __forceinline__ float tanh_fast(float x) {  // 2 sigmoid(2x) - 1; saturates cleanly: exp2 -> inf / 0
  return 2.0f * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -2.88539008177792681f)) - 1.0f;
}


// ---- the LSTM step as a hand-placed software pipeline (round 5).
// Measured on this part (scratch/mfma_valu.hip, profiles/r05_mfma_valu.txt): a wave that issues a bf16 / f16 MFMA and then up to TWO
// independent VALU instructions pays nothing for them (56 MFMAs + 112 VALU: 941 cycles against 928 for the MFMAs alone; a
// third costs 4 - 5 cycles each), and two such waves on a SIMD keep its matrix pipe 100 % busy -- whereas a burst of 56 MFMAs
// followed by a burst of 136 VALU costs their SUM in one wave (1572) and two such waves overlap only partly (1087 per unit).
// The compiler issues bursts (and keeps them under sched_group_barrier), so the order is pinned by hand: the gate
// arithmetic of row block rb - 1 is cut into single-instruction micro-ops (25 per element) and two of them follow every
// MFMA of row block rb, behind a sched_barrier(0) each.  PIN: an empty asm volatile the value passes through -- the
// instruction that produces it can sink no further (asm volatile statements keep their order), and one that consumes it
// can rise no further.
#define GA3C_PIN(x) asm volatile("" : "+v"(x))
#define GA3C_FENCE() __builtin_amdgcn_sched_barrier(0)
// The cell update of one row block as single-instruction micro-ops (20 per element: 9 transcendental + 11 plain).  The
// pre-activations arrive PRE-SCALED: the i, f, o columns of the LSTM kernel and bias by -log2 e, the j column by -2 log2 e
// (cagpu_ga3c_pack for the h part, the ax build for the x part and the bias), so sigmoid(x) = 1 / (1 + 2^z) and tanh(x) =
// 2 / (1 + 2^z) - 1 start at the v_exp.  The cell state is kept SCALED as well, c' = -2 log2 e * c (the scale rides on
// tanh(j): K tanh(j) = 2 K / (1 + 2^z) - K), so tanh(c) starts at its v_exp too; and h = sigmoid(o) tanh(c) =
// (1 - 2^c') / ((1 + 2^zo)(1 + 2^c')) takes ONE v_rcp for both quotients (2^c' <= 2^55: the product cannot be inf x 0).
// No packed float32 arithmetic here: measured (scratch/mfma_valu.hip), a v_pk_fma_f32 behind an MFMA waits for the MFMA
// and in the VALU-bound mix of this stage (MFMA, 2 transcendentals, 2 plain) one packed instruction costs what the two
// plain ones cost -- the packed form of this update was slower than the scalar one.
struct Gate {
  float a[4], b[4], c[4], d[4];  // a: i -> sigmoid -> c'_t+1;  b: j -> K tanh, later 2^c', 1 - 2^c';  c: f -> sigmoid * c'_t, later the denominator;  d: o -> 1 + 2^zo -> h_t+1
};
constexpr int GATE_OPS = 80;       // micro-ops of one row block's cell update (20 per element)
constexpr int GATE_OPS_SEL = 88;   // + the two selects per element of a tile with rows of different sequence lengths
// The ORDER the micro-ops are issued in (position -> micro-op = 4 step + element): a list schedule of the update's
// dependency graph (tests/test_host_logic.py checks it) that alternates transcendental and plain instructions -- an MFMA
// hides one v_exp / v_rcp and one plain instruction behind it, not two transcendentals -- longest remaining chain first,
// dependent ops at least two positions apart.
constexpr int GATE_ORDER[GATE_OPS] = {
     4,  8,  5, 20,  9, 24,  6, 21, 10, 25,  7, 22, 11, 26,  0, 23,  1, 27,  2, 16,  3, 17, 36, 18, 40, 19, 37, 44,
    41, 48, 38, 45, 42, 49, 39, 46, 43, 50, 32, 47, 33, 51, 34, 52, 35, 53, 12, 54, 56, 55, 13, 28, 57, 60, 14, 29,
    58, 61, 15, 30, 59, 62, 31, 63, 64, 65, 66, 68, 67, 69, 72, 70, 73, 71, 74, 75, 76, 77, 78, 79};
constexpr int GATE_ORDER_SEL[GATE_OPS_SEL] = {
     4,  8,  5, 20,  9, 24,  6, 21, 10, 25,  7, 22, 11, 26,  0, 23,  1, 27,  2, 16,  3, 17, 36, 18, 40, 19, 37, 44,
    41, 48, 38, 45, 42, 49, 39, 46, 43, 50, 32, 47, 33, 51, 34, 52, 35, 53, 12, 54, 56, 55, 13, 28, 57, 60, 14, 29,
    58, 61, 15, 30, 59, 62, 31, 63, 64, 65, 66, 68, 67, 69, 72, 70, 73, 71, 74, 75, 76, 77, 78, 79, 80, 84, 81, 85,
    82, 86, 83, 87};
// micro-op i: step i / 4 of element i % 4.  z: the four gates' pre-scaled pre-activations (i, j, f, o) of the row block;
// cst: the lane's SCALED cell state c' of the row block, hst: its h.
template <bool ALL_LIVE>
__device__ __forceinline__ void gate_op(const int i, Gate& g, const f32x4 (&z)[4], float (&cst)[4], float (&hst)[4], const bool live) {
  const int s = i >> 2, r = i & 3;
  constexpr float K = -2.88539008177792681f;  // -2 log2 e
  switch (s) {
    case 0: g.a[r] = __builtin_amdgcn_exp2f(z[0][r]); GA3C_PIN(g.a[r]); break;
    case 1: g.b[r] = __builtin_amdgcn_exp2f(z[1][r]); GA3C_PIN(g.b[r]); break;
    case 2: g.c[r] = __builtin_amdgcn_exp2f(z[2][r]); GA3C_PIN(g.c[r]); break;
    case 3: g.d[r] = __builtin_amdgcn_exp2f(z[3][r]); GA3C_PIN(g.d[r]); break;
    case 4: g.a[r] = 1.0f + g.a[r]; GA3C_PIN(g.a[r]); break;
    case 5: g.b[r] = 1.0f + g.b[r]; GA3C_PIN(g.b[r]); break;
    case 6: g.c[r] = 1.0f + g.c[r]; GA3C_PIN(g.c[r]); break;
    case 7: g.d[r] = 1.0f + g.d[r]; GA3C_PIN(g.d[r]); break;                      // 1 + 2^zo: its reciprocal is taken with tanh(c)'s
    case 8: g.a[r] = __builtin_amdgcn_rcpf(g.a[r]); GA3C_PIN(g.a[r]); break;     // sigmoid(i)
    case 9: g.b[r] = __builtin_amdgcn_rcpf(g.b[r]); GA3C_PIN(g.b[r]); break;
    case 10: g.c[r] = __builtin_amdgcn_rcpf(g.c[r]); GA3C_PIN(g.c[r]); break;   // sigmoid(f) (forget_bias is in the bias)
    case 11: g.b[r] = __builtin_fmaf(g.b[r], 2.0f * K, -K); GA3C_PIN(g.b[r]); break;   // K tanh(j)
    case 12: g.c[r] = g.c[r] * cst[r]; GA3C_PIN(g.c[r]); break;
    case 13: g.a[r] = __builtin_fmaf(g.a[r], g.b[r], g.c[r]); GA3C_PIN(g.a[r]); break;   // c'_t+1 = sigmoid(f) c'_t + sigmoid(i) K tanh(j)
    case 14: g.b[r] = __builtin_amdgcn_exp2f(g.a[r]); GA3C_PIN(g.b[r]); break;          // 2^c' = e^(-2 c)
    case 15: g.c[r] = 1.0f + g.b[r]; GA3C_PIN(g.c[r]); break;
    case 16: g.c[r] = g.c[r] * g.d[r]; GA3C_PIN(g.c[r]); break;                          // (1 + 2^c')(1 + 2^zo)
    case 17: g.c[r] = __builtin_amdgcn_rcpf(g.c[r]); GA3C_PIN(g.c[r]); break;
    case 18: g.b[r] = 1.0f - g.b[r]; GA3C_PIN(g.b[r]); break;
    case 19:
      g.d[r] = g.b[r] * g.c[r];   // h_t+1 = sigmoid(o) tanh(c_t+1)
      GA3C_PIN(g.d[r]);
      if (ALL_LIVE) {
        cst[r] = g.a[r];
        hst[r] = g.d[r];
      }
      break;
    case 20: cst[r] = live ? g.a[r] : cst[r]; GA3C_PIN(cst[r]); break;   // GreaterEqual / Select_1 / Select_2: a row past its
    case 21: hst[r] = live ? g.d[r] : hst[r]; GA3C_PIN(hst[r]); break;   // sequence length keeps its state
    default: break;
  }
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_h(const u32x4 a, const u32x4 b, const f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// float32 operands on the f16 matrix cores: x = hi + lo + e with hi = fp16(x), lo = fp16(x - hi) (round to nearest; x - hi is
// exact in float32), |e| <= 2^-22 |x| -- 22 of the 24 significant bits; fp16 denormals included: v_cvt_f16_f32 produces them
// and v_mfma_f32_16x16x32_f16 multiplies them (scratch/f16_denorm.hip), so a small value's low plane keeps an ABSOLUTE
// accuracy of 3e-8.  A product a b is accumulated as lo_a hi_b + hi_a lo_b + hi_a hi_b -- three plane products, each
// exact in the f32 accumulator (11 + 11 bits), the dropped lo_a lo_b below 2^-22 of the product -- against six for the
// three-bf16-plane split of rounds 2 - 4 (a product within 2^-21): HALF the matrix work at the same accuracy (logits
// against float64: max 3.9e-5, mean 1.4e-6; numpy's float32: 2.0e-5 / 1.3e-6; six bf16 products: 3.2e-5 / 1.7e-6;
// tests/test_gpu_parity.py).  Range: fp16
// overflows at 65 504; the network's activations stay three orders of magnitude below.
struct Planes {
  u32x4 p[NPL];
};
__device__ __forceinline__ unsigned int pk2(const float a, const float b) {  // {fp16(a), fp16(b)}, round to nearest: v_cvt_pk_f16_f32
  const f16x2 v = {static_cast<_Float16>(a), static_cast<_Float16>(b)};
  return __builtin_bit_cast(unsigned int, v);
}
__device__ __forceinline__ float lo_part(const float x) { return x - static_cast<float>(static_cast<_Float16>(x)); }
__device__ __forceinline__ Planes split8(const f32x4 v0, const f32x4 v1) {
  Planes s;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = (i < 2) ? v0[2 * i] : v1[2 * i - 4], b = (i < 2) ? v0[2 * i + 1] : v1[2 * i - 3];
    s.p[0][i] = pk2(a, b);
    s.p[1][i] = pk2(lo_part(a), lo_part(b));
  }
  return s;
}
// acc[c] += W[c] * X on the three plane products, smallest first, for the four weight fragments W[c] (planes [c][0..1], the
// A operands) against one fragment of the rows' planes X (the B operand).  The four accumulators are independent, so
// consecutive MFMAs never wait for each other's result.
constexpr int NTERM = 3;
constexpr int TERM[NTERM][2] = {{1, 0}, {0, 1}, {0, 0}};  // (weight plane, row plane): lo*hi, hi*lo, hi*hi
__device__ __forceinline__ void plane_terms(f32x4 (&acc)[4], const u32x4 (&w)[4][NPL], const u32x4 (&x)[NPL]) {
#pragma unroll
  for (int t = 0; t < NTERM; ++t)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = mfma_h(w[c][TERM[t][0]], x[TERM[t][1]], acc[c]);
}

// One 256-wide dense layer, transposed: acc[rb][cb][r] (+)= sum_k W[k][64 wv + 16 cb + 4 q + r] * src[16 rb + m][k], k < 32 NKB.
// `wp`: the layer's packed planes.  The next k-block's twelve fragments are in flight while this one's MFMAs issue.
// PLANES: `src` is the LSTM's h, already split (NPL planes of [TM][HP_LD] fp16); else float32 [TM][ld], split here.
template <int NKB, bool PLANES>
__device__ __forceinline__ void dense_t(const float* src, const int ld, const u32x4* __restrict__ wp, f32x4 (&acc)[4][4],
                                        const int lane, const int m, const int q, const int wv, const int nrb) {
  const u32x4* w0 = wp + (4 * wv) * NPL * 64 + lane;  // + ((kb * 16 + cb) * NPL + plane) * 64
  u32x4 wc[4][NPL], wn[4][NPL];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) wc[cb][pl] = w0[(cb * NPL + pl) * 64];
#pragma unroll 1
  for (int kb = 0; kb < NKB; ++kb) {
    if (kb + 1 < NKB) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) wn[cb][pl] = w0[(((kb + 1) * 16 + cb) * NPL + pl) * 64];
    }
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      if (rb >= nrb) continue;  // workgroup-uniform: this tile holds fewer than 64 rows
      Planes x;
      if constexpr (PLANES) {
        const float* sp = src + ((rb * 16 + m) * HP_LD + kb * 32 + 8 * q) / 2;
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) x.p[pl] = *reinterpret_cast<const u32x4*>(sp + pl * HP_PLANE);
      } else {
        const float* sp = src + (rb * 16 + m) * ld + kb * 32 + 8 * q;
        x = split8(*reinterpret_cast<const f32x4*>(sp), *reinterpret_cast<const f32x4*>(sp + 4));
      }
      plane_terms(acc[rb], wc, x.p);
    }
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) wc[cb][pl] = wn[cb][pl];
  }
}

// The same layer for float32 activations as a hand-placed pipeline (round 5), per tile height NRB: the 24 instructions that
// split the next row block's eight activations into planes are issued two behind each of this row block's 12 MFMAs
// (GA3C_PIN / GA3C_FENCE above) instead of in a burst ahead of them -- the compiler's order left the matrix pipe idle for a
// third of the layer.  g = kb NRB + rb: MFMAs of g with the planes `x`; the raw values of g + 1 (loaded during g - 1) are
// split into `xn`; the raw values of g + 2 are loaded once g + 1's are consumed.
template <int NKB, int NRB>
__device__ __forceinline__ void dense_pipe(const float* src, const int ld, const u32x4* __restrict__ wp, f32x4 (&acc)[4][4],
                                           const int lane, const int m, const int q, const int wv) {
  static_assert(NKB % 2 == 0, "two k-blocks per trip: the weight fragments alternate between two register sets, no copies");
  const u32x4* w0 = wp + (4 * wv) * NPL * 64 + lane;  // + ((kb * 16 + cb) * NPL + plane) * 64
  u32x4 wa[4][NPL], wb[4][NPL];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb)
#pragma unroll
    for (int pl = 0; pl < NPL; ++pl) wa[cb][pl] = w0[(cb * NPL + pl) * 64];
  const float* sp0 = src + m * ld + 8 * q;  // + (rb * 16) * ld + kb * 32
  Planes x = split8(*reinterpret_cast<const f32x4*>(sp0), *reinterpret_cast<const f32x4*>(sp0 + 4));
  float v[8], bk[8];       // raw values of the next row block; their hi planes converted back, then the remainders
  unsigned int pn[NPL][4];  // the planes being built
  {
    const float* sp = sp0 + 16 * ld;
    const f32x4 lo = *reinterpret_cast<const f32x4*>(sp), hi = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = lo[e]; v[4 + e] = hi[e]; }
  }
  // one k-block: `wc` holds its fragments, `wn` receives the next one's
  auto kblock = [&](const int kb, const u32x4 (&wc)[4][NPL], u32x4 (&wn)[4][NPL]) {
    if (kb + 1 < NKB) {
#pragma unroll
      for (int cb = 0; cb < 4; ++cb)
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) wn[cb][pl] = w0[(((kb + 1) * 16 + cb) * NPL + pl) * 64];
    }
#pragma clang loop unroll(full)
    for (int rb = 0; rb < NRB; ++rb) {
      f32x4 nlo, nhi;  // raw values of g + 2
#pragma clang loop unroll(full)
      for (int j = 0; j < 4 * NTERM; ++j) {
        const int c = j & 3, t = j >> 2;
        GA3C_PIN(acc[rb][c]);
        acc[rb][c] = mfma_h(wc[c][TERM[t][0]], x.p[TERM[t][1]], acc[rb][c]);
        GA3C_PIN(acc[rb][c]);
        // micro-ops 2 j, 2 j + 1 of the split: 0..3 the hi plane (v_cvt_pk_f16_f32); 4..11 its halves back to float32;
        // 12..19 the remainders (in place); 20..23 the lo plane
#pragma clang loop unroll(full)
        for (int u = 0; u < 2; ++u) {
          const int k = 2 * j + u;
          if (k < 4) { pn[0][k] = pk2(v[2 * k], v[2 * k + 1]); GA3C_PIN(pn[0][k]); }
          else if (k < 12) {
            const f16x2 hp = __builtin_bit_cast(f16x2, pn[0][(k - 4) >> 1]);
            bk[k - 4] = static_cast<float>(((k - 4) & 1) ? hp.y : hp.x);
            GA3C_PIN(bk[k - 4]);
          }
          else if (k < 20) { bk[k - 12] = v[k - 12] - bk[k - 12]; GA3C_PIN(bk[k - 12]); }
          else if (k < 24) { pn[1][k - 20] = pk2(bk[2 * (k - 20)], bk[2 * (k - 20) + 1]); GA3C_PIN(pn[1][k - 20]); }
        }
        if (j == 10) {  // the raw values of g + 1 are consumed (micro-op 19): load those of g + 2 (behind the last: in-bounds, unused)
          const int kb2 = kb + (rb + 2) / NRB, rb2 = (rb + 2) % NRB;
          const float* sp = sp0 + (rb2 * 16) * ld + kb2 * 32;
          nlo = *reinterpret_cast<const f32x4*>(sp);
          nhi = *reinterpret_cast<const f32x4*>(sp + 4);
        }
        GA3C_FENCE();
      }
#pragma clang loop unroll(full)
      for (int pl = 0; pl < NPL; ++pl) x.p[pl] = u32x4{pn[pl][0], pn[pl][1], pn[pl][2], pn[pl][3]};
#pragma clang loop unroll(full)
      for (int e = 0; e < 4; ++e) { v[e] = nlo[e]; v[4 + e] = nhi[e]; }
    }
  };
#pragma unroll 1
  for (int kb = 0; kb < NKB; kb += 2) {
    kblock(kb, wa, wb);
    kblock(kb + 1, wb, wa);
  }
}

// BiasAdd + Relu; a lane's four results are units 64 wv + 16 cb + 4 q .. + 3 of row 16 rb + m: one 16-byte store each
// (the caller fences with barriers).
// `amax`: running maximum of what this thread stores (the range guard of the two-plane fp16 split: see the kernel's end).
__device__ __forceinline__ void store_relu_t(float* act, const float* __restrict__ bias, const f32x4 (&acc)[4][4], const int m,
                                             const int q, const int wv, const int nrb, float& amax) {
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int u0 = wv * 64 + cb * 16 + 4 * q;
    const f32x4 b = *reinterpret_cast<const f32x4*>(bias + u0);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      if (rb >= nrb) continue;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = fmaxf(acc[rb][cb][r] + b[r], 0.f);
      amax = fmaxf(amax, fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
      *reinterpret_cast<f32x4*>(act + (rb * 16 + m) * ACT_LD + u0) = v;
    }
  }
}

// cagpu_ga3c_pack: one thread per (k-block, column block, lane): W[row0 + kb * 32 + 8 q + e][cb * 16 + m], e = 0..7, split
// into its two fp16 planes (rows past `k_real` are zero).  `ld` = 256 (the checkpoint's [in, out] layout).
// `lstm`: the matrix is rnn/lstm_cell/kernel: its columns are pre-scaled for the gates' 2^z form (struct Gate): i, f, o by
// -log2 e, j (columns 64 .. 127) by -2 log2 e.
__global__ void pack_kernel(const float* __restrict__ w, const int row0, const int k_real, const int nkb, u32x4* __restrict__ out,
                            const int lstm) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= nkb * 16 * 64) return;
  const int lane = idx & 63, cb = (idx >> 6) & 15, kb = idx >> 10;
  const int m = lane & 15, q = lane >> 4;
  float v[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = kb * 32 + 8 * q + e;
    v[e] = (k < k_real) ? w[static_cast<long>(row0 + k) * 256 + cb * 16 + m] : 0.f;
    if (lstm) v[e] *= ((cb >> 2) == 1) ? -2.88539008177792681f : -1.44269504088896341f;
  }
  const Planes s = split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]});
#pragma unroll
  for (int pl = 0; pl < NPL; ++pl) out[((kb * 16 + cb) * NPL + pl) * 64 + lane] = s.p[pl];
}

// The whole network for one tile.  EXT = false is the default launch (cagpu_ga3c); EXT = true adds the query row source,
// the value column and the value / action outputs (cagpu_ga3c_query, cagpu_ga3c_value) -- every addition sits behind
// `if constexpr (EXT)`: the default instantiation contains none of it (its second argument is the empty NoExt).
struct NoExt {};
template <bool EXT>
__global__ __launch_bounds__(NT, 2) void ga3c_kernel(const Args g, const typename std::conditional<EXT, Ext, NoExt>::type ex) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* hostv = reinterpret_cast<float*>(smem);          // [TM][4]  normalised dist_to_goal, heading, pref_speed, radius
  int* seqv = reinterpret_cast<int*>(hostv + TM * 4);     // [TM]     sequence_length
  int* misc = seqv + TM;                                  // [MISC]   [1] / [2] = longest / shortest sequence of the tile
  float* un = reinterpret_cast<float*>(misc + MISC);
  float* xo = un;                                         // [TM][XO_LD]     LSTM phase
  float* hp = xo + TM * XO_LD;                            // [NPL][TM][HP_LD] fp16: the planes of h (LSTM phase)
  float* xs = hp + NPL * HP_PLANE;                        // [XS_RING][NPL][TM][8] fp16: the planes of x_t, x_t+1 (LSTM phase)
  float* act = un;                                        // [TM][ACT_LD]    dense phase
  float* lg = un + TM * ACT_LD;                           // [TM][16]        logits

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  const long n_rows = g.rows ? static_cast<long>(g.rows[g.B]) : g.B;
  const Tile tile = tile_of(n_rows, g.slots, g.force_tile, blockIdx.x);
  const int tm = tile.tm, nrb = tm >> 4;  // rows / 16-row blocks of THIS tile
  const long row0 = tile.row0;

  // ---- the tile's rows: slot t holds packed row rows[row0 + t] (or row row0 + t itself without the packed list)
  if (row0 >= n_rows) return;  // workgroup-uniform (the grid covers the worst case: every row alive, 32-row tiles)
  bool plain = false;
  if constexpr (EXT) plain = ex.query != 0;  // query rows: every row of a plain array of policy vectors
  auto row_of = [&](const int slot) -> long {
    const long t = row0 + slot;
    return (slot < tm && t < n_rows) ? (g.rows ? static_cast<long>(g.rows[t]) : t) : -1;
  };
  bool need = false;
  if (tid < TM) {
    const long i = row_of(tid);
    need = i >= 0 && (g.rows != nullptr || plain ||
                      (needs_action(g.flags[i]) && (!g.net.agent_net || g.net.agent_net[i] == g.net.net_index)));
  }
  if (!__syncthreads_or(need ? 1 : 0)) return;
  // The range guard of the two-plane fp16 split (Planes above): every float32 value that is split on its way to the f16
  // matrix cores -- the normalised other-agent inputs and the outputs of layer1 / layer2 (h is bounded by 1) -- runs through
  // this thread-local maximum; a value at or beyond fp16's largest finite number would become +-inf in its high plane and
  // the network would answer from saturated operands WITHOUT any sign of it (ReLU swallows the NaNs that follow).  Checked
  // once at the kernel's end: bit 1 of the device's fault word (cagpu_device_faults).  ~160 v_max per thread and launch.
  // The INPUT columns -- the other-agent block and the four host columns, which reach layer1 unsplit -- may hold a NaN, and
  // v_max_f32 returns its other operand then: the NaN would leave the maximum alone, ReLU would swallow it
  // (fmaxf(NaN + b, 0) = 0) and the network would answer from zeros with the word clear.  Their maximum is therefore taken
  // on the BIT PATTERNS of |x| as unsigned integers (absmax_bits): non-negative floats order like their patterns, +inf lies
  // above every finite value and every NaN above +inf.  Behind the prologue it becomes the float maximum the activations
  // continue (they are ReLU outputs: never NaN), +inf standing for "out of range" (sticky under v_max_f32).
  constexpr unsigned int FP16_MAX_BITS = 0x477FE000u;  // 65 504.f
  auto absmax_bits = [](const unsigned int mx, const float x) {
    const unsigned int b = __builtin_bit_cast(unsigned int, x) & 0x7FFFFFFFu;
    return b > mx ? b : mx;
  };
  unsigned int xmax = 0u;
  float amax_unused = 0.f;

  // ---- X = obs[1:] zero-padded / cropped to 138 (GA3CCADRLPolicy.py:69-75, network.py:24-35); sub, div.
  // Four threads per row, 35 columns each; every global load is issued before the first use and none sits behind a
  // branch (clamped address + select).  Measured per workgroup: 41 k cycles, against 95 k for a plain strided loop with
  // a dependent load per iteration and 78 k for a lane-contiguous mapping (profiles/r01_kernel_geometry.md).
  if (tid == 0) {
    misc[1] = 0;        // longest sequence of the tile
    misc[2] = 1 << 30;  // shortest sequence among its REAL rows
  }
  for (int idx = tid; idx < NPL * HP_PLANE; idx += NT) hp[idx] = 0.f;  // LSTMCellZeroState
  if (g.obs == nullptr) {
    // ================= FUSED SENSING: "ego-centric obs + network inference fused in-kernel" (BASELINE configs[2]).
    // Four threads per row share the row's N - 1 others; the expressions are the step kernels' (P3 / P4 of ca_kernel, in
    // the host's own view: d - r_host - r_other, the (key, p_orth, index) order, the clip, closest_last's second order),
    // so the float32 values that reach the network are the ones the stored observation row holds, bit for bit
    // (tests/test_gpu_parity.py::test_ga3c_fused_sensing_equals_the_stored_observation).  Scratch (sort keys + first-pass
    // ranks): the planes of h, re-zeroed below.
    static_assert(NT == 4 * TM, "four threads per row");
    constexpr int SN = 32;  // others per row the scratch holds (num_agents <= 32: the network reads 19 of them anyway)
    static_assert(TM * SN <= NPL * HP_PLANE, "the keys fit the planes of h");
    int* skey = reinterpret_cast<int*>(hp);  // [TM][SN] sort key (KEY_NONE: not sensed)
    const int rr = tid >> 2, t4 = tid & 3;
    const long i = row_of(rr);
    const bool row_ok = i >= 0;
    const int N = g.N;
    const long e = row_ok ? i / N : 0;
    const int a = row_ok ? static_cast<int>(i - e * N) : 0;
    const long eb = e * N;
    // Every global load of the row first, all in flight together: the host's state and this thread's eight others
    // (j = t4, t4 + 4, ...; clamped index, never behind a branch).  (Measured: no faster than loading inside the loops --
    // 343.6 vs 344.1 us per launch --: what the fused prologue costs, +30 us against reading the stored rows, is its
    // float64 arithmetic, not its loads; profiles/r04_kernel_geometry.md section 6.)
    constexpr int PT = SN / 4;  // others per thread
    double ox[PT], oy[PT], orad_[PT], ovx[PT], ovy[PT];
    const double hx = g.pos_x[eb + a], hy = g.pos_y[eb + a], hr = g.radius[eb + a];
    const double hgx = g.goal_x[eb + a], hgy = g.goal_y[eb + a], hhd = g.heading[eb + a], hps = g.pref_speed[eb + a];
#pragma unroll
    for (int u = 0; u < PT; ++u) {
      const int j = t4 + 4 * u;
      const long jj = eb + (j < N ? j : 0);
      ox[u] = g.pos_x[jj]; oy[u] = g.pos_y[jj]; orad_[u] = g.radius[jj]; ovx[u] = g.vel_x[jj]; ovy[u] = g.vel_y[jj];
    }
    const Ego eg = ego_frame(hx, hy, hgx, hgy, hhd);
    const auto p_orth = [&](const int j) {  // of other j in this host's frame (recomputed where two keys tie: rare)
      const double rx = g.pos_x[eb + j] - hx, ry = g.pos_y[eb + j] - hy;
      return rx * (-eg.pry) + ry * eg.prx;
    };
    __syncthreads();  // h is zeroed
    {  // every column of X starts as the normalised ZERO (an unfilled slot of the observation is 0, sensor :112)
      constexpr int PER = (XIN + 3) / 4;  // 35
#pragma unroll
      for (int j = 0; j < PER; ++j) {
        const int c = t4 * PER + j;
        if (c >= 5 && c < XIN) xo[rr * XO_LD + c - 5] = (0.f - g.net.input_mean[c]) / g.net.input_std[c];
      }
    }
    double dist_[PT];
#pragma unroll
    for (int u = 0; u < PT; ++u) {
      const int j = t4 + 4 * u;
      int key = KEY_NONE;
      const double rx = ox[u] - hx, ry = oy[u] - hy;
      const double d = sqrtd(rx * rx + ry * ry);
      dist_[u] = d;
      if (row_ok && j < N && j != a) {
        const bool both = !g.ragged || (hr > 0.0 && orad_[u] > 0.0);
        if (both && !(d > g.sensing_horizon))
          key = static_cast<int>(fmin(fmax(rint((d - hr - orad_[u]) * 100.0), -2.0e9), 2.0e9));
      }
      skey[rr * SN + j] = key;
    }
    __syncthreads();
    int cnt = 0;
    for (int q = 0; q < N; ++q) cnt += static_cast<int>(skey[rr * SN + q] != KEY_NONE);
    const int keep = cnt < g.obs_clip ? cnt : g.obs_clip;  // sensor :39 (obs_clip <= max_obs)
#pragma unroll
    for (int u = 0; u < PT; ++u) {
      const int j = t4 + 4 * u;
      const int kj = skey[rr * SN + j];
      if (kj == KEY_NONE) continue;
      int rank = 0, lt = 0, same = 1;  // candidates in closer buckets / in this bucket (itself included)
      for (int q = 0; q < N; ++q) {
        const int kq = skey[rr * SN + q];
        if (kq == KEY_NONE || q == j) continue;
        if (kq < kj) lt += 1;
        else if (kq == kj) {  // the (p_orth, index) tie-break of one 1 cm bucket
          const double oq = p_orth(q), oj = p_orth(j);
          same += 1;
          rank += static_cast<int>(oq < oj) | (static_cast<int>(oq == oj) & static_cast<int>(q < j));
        }
      }
      rank += lt;
      if (rank >= keep) continue;
      int slot = rank;
      if (g.sort_mode == CA_SORT_CLOSEST_LAST) {  // the kept ones by (-key, p_orth), stable (sensor :41-43): the buckets in
        const int room = keep - lt;               // reverse, the order inside a bucket kept (ca_kernel P4, same expression)
        slot = room - (same < room ? same : room) + (rank - lt);
      }
      if (slot >= NO) continue;  // (X holds 19 slots: a wider observation is cropped, network.py:24-35)
      const double rx = ox[u] - hx, ry = oy[u] - hy;
      float v7[7];
      v7[0] = static_cast<float>(rx * eg.prx + ry * eg.pry);
      v7[1] = static_cast<float>(rx * (-eg.pry) + ry * eg.prx);
      v7[2] = static_cast<float>(ovx[u] * eg.prx + ovy[u] * eg.pry);
      v7[3] = static_cast<float>(ovx[u] * (-eg.pry) + ovy[u] * eg.prx);
      v7[4] = static_cast<float>(orad_[u]);
      v7[5] = static_cast<float>(hr + orad_[u]);
      v7[6] = static_cast<float>(dist_[u] - hr - orad_[u]);
#pragma unroll
      for (int f = 0; f < 7; ++f) {
        const int c = 5 + 7 * slot + f;
        const float xn = (v7[f] - g.net.input_mean[c]) / g.net.input_std[c];
        xmax = absmax_bits(xmax, xn);
        xo[rr * XO_LD + c - 5] = xn;
      }
    }
    if (t4 == 0) {  // the host columns of X: num_other_agents (raw: the sequence length), dist_to_goal, heading, pref_speed, radius
      const bool here = row_ok && !(g.ragged && !(hr > 0.0));
      int sl = row_ok ? keep : 0;
      sl = sl < 0 ? 0 : (sl > NO ? NO : sl);
      seqv[rr] = sl;
      atomicMax(&misc[1], sl);
      if (row_ok) atomicMin(&misc[2], sl);
      const float h4[4] = {here ? static_cast<float>(eg.dist) : 0.f, here ? static_cast<float>(eg.heading_ego) : 0.f,
                           here ? static_cast<float>(hps) : 0.f, row_ok ? static_cast<float>(hr) : 0.f};
#pragma unroll
      for (int c = 1; c < 5; ++c) {
        const float xn = (h4[c - 1] - g.net.input_mean[c]) / g.net.input_std[c];
        xmax = absmax_bits(xmax, xn);
        hostv[rr * 4 + c - 1] = xn;
      }
    }
    __syncthreads();
    // give the scratch back (zeros, as the LSTM expects)
    for (int idx = tid; idx < NPL * HP_PLANE; idx += NT) hp[idx] = 0.f;
  } else
  {
    static_assert(NT == 4 * TM, "four threads per row");
    constexpr int PER = (XIN + 3) / 4;  // 35
    const int rr = tid >> 2, c0 = (tid & 3) * PER;
    const long i = row_of(rr);
    const bool row_ok = i >= 0;
    const float* orow = g.obs + (row_ok ? i : 0) * (plain ? g.W - 1 : g.W) + (plain ? 0 : 1);  // (a query row IS obs[1:])
    // input_mean / input_std through LDS: 276 loads per workgroup instead of 70 per thread (105 vector-memory instructions per
    // thread stalled on the 63 a wave may have in flight; the table sits in the union's slack behind the LSTM's share)
    static_assert(UNION_FLOATS - LSTM_FLOATS >= 2 * XIN && XIN <= NT, "room for the table");
    float* ms = un + LSTM_FLOATS;
    if (tid < XIN) {
      ms[tid] = g.net.input_mean[tid];
      ms[XIN + tid] = g.net.input_std[tid];
    }
    float xv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = c0 + j;
      const int cc = c < XIN ? c : XIN - 1;
      const int co = (cc + 1 < g.W) ? cc : g.W - 2;  // W >= 6 (a query: W >= 2)
      xv[j] = orow[co];
    }
    __syncthreads();  // h is zeroed, the table is written
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int c = c0 + j;
      const int cc = c < XIN ? c : XIN - 1;
      const float x = (row_ok && c + 1 < g.W) ? xv[j] : 0.f;
      const float xn = (x - ms[cc]) / ms[XIN + cc];
      if (c == 0) {
        int sl = static_cast<int>(x);  // strided_slice -> ToInt32 -> sequence_length (from the RAW input)
        sl = sl < 0 ? 0 : (sl > NO ? NO : sl);
        seqv[rr] = sl;
        atomicMax(&misc[1], sl);
        if (row_ok) atomicMin(&misc[2], sl);
      } else if (c < 5) {
        xmax = absmax_bits(xmax, xn);
        hostv[rr * 4 + c - 1] = xn;  // strided_slice_1
      } else if (c < XIN) {
        xmax = absmax_bits(xmax, xn);
        xo[rr * XO_LD + c - 5] = xn;  // strided_slice_2
      }
    }
  }
  float amax = xmax < FP16_MAX_BITS ? __builtin_bit_cast(float, xmax) : __builtin_inff();  // (see the guard above)

  // ---- this wave's LSTM weights: gate g4 (i, j, f, o), units 16 wv .. 16 wv + 15 = packed column block 4 g4 + wv.
  // h part: two planes x two k-blocks per gate.  x part (rows 0..6 of the kernel) + bias: the float32 MFMA is NOT used --
  // measured (scratch/mfma_valu.hip, profiles/r05_mfma_valu.txt): v_mfma_f32_16x16x4_f32 blocks the SIMD's VALU for its 32
  // cycles, for both of the SIMD's waves (f32 MFMA + 4 VALU: 58 cycles; two such waves: the sum), where an f16 / bf16 MFMA
  // runs beside two VALU instructions for free; the x part was a quarter of the LSTM's matrix time and all of it
  // VALU-blocking.  Instead the three plane products ride on ONE f16 MFMA per gate whose K = 32 holds four groups of 8
  // (7 inputs + the bias against a constant 1):
  //     group q = 0 .. 2:  (W hi, x hi)  (W hi, x lo)  (W lo, x hi)        slot 7: bias hi / bias lo / 0 against 1.0
  // Lane (m, q) holds group q of unit m (A) / of row m (B); the rows' planes come from a per-step staging buffer in LDS.
  const u32x4* pk = reinterpret_cast<const u32x4*>(g.net.packed);
  u32x4 wh[2][4][NPL];  // [k-block][gate][plane]
  u32x4 ax[4];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int pl = 0; pl < NPL; ++pl) wh[kb][g4][pl] = pk[PK_LSTM + ((kb * 16 + 4 * g4 + wv) * NPL + pl) * 64 + lane];
    const int col = g4 * 64 + wv * 16 + m;
    float v[8];
    const float sc = (g4 == 1) ? -2.88539008177792681f : -1.44269504088896341f;  // the gates' 2^z scale (struct Gate), as pack_kernel's
#pragma unroll
    for (int e = 0; e < 7; ++e) v[e] = g.net.lstm_kernel[e * 256 + col] * sc;
    v[7] = (g.net.lstm_bias[col] + ((g4 == 2) ? 1.0f : 0.f)) * sc;  // forget_bias 1.0 (BasicLSTMCell), folded into the f gate's bias
    const Planes P = split8(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]});
    const u32x4 w1 = (q == 2) ? P.p[1] : P.p[0];                                        // W hi, W hi, W lo, -
    const unsigned int b1 = (q == 0) ? P.p[0][3] : (q == 1) ? P.p[1][3] : 0u;           // bias hi, bias lo, 0
    ax[g4] = (q < 3) ? u32x4{w1[0], w1[1], w1[2], (w1[3] & 0x0000FFFFu) | (b1 & 0xFFFF0000u)} : u32x4{0u, 0u, 0u, 0u};
  }
  // the rows' x_t planes: xs[buffer t & 1][plane][row][8] fp16 (slot 7 = 1.0), written one step ahead by all 256 threads
  // (448 = 64 rows x 7 inputs values per step: thread k takes values k and k + 256)
  unsigned short* const xs16 = reinterpret_cast<unsigned short*>(xs);
  const int k0 = tid, k1 = tid + NT;
  const int xrow0 = k0 / 7, xrow1 = (k1 < TM * 7) ? k1 / 7 : 0;
  const int xsrc0 = xrow0 * XO_LD + (k0 - 7 * xrow0), xsrc1 = xrow1 * XO_LD + (k1 - 7 * xrow1);
  const int xdst0 = xrow0 * 8 + (k0 - 7 * xrow0), xdst1 = xrow1 * 8 + (k1 - 7 * xrow1);
  const bool two = __builtin_amdgcn_readfirstlane(tid) + NT < TM * 7;  // (wave-uniform: waves 0 - 2)
  auto h16 = [](const float x) { return __builtin_bit_cast(unsigned short, static_cast<_Float16>(x)); };
  auto stage_store = [&](const int buf, const float xa, const float xb) {
    unsigned short* d = xs16 + buf * (NPL * TM * 8);
    d[xdst0] = h16(xa);
    d[TM * 8 + xdst0] = h16(lo_part(xa));
    if (two) {
      d[xdst1] = h16(xb);
      d[TM * 8 + xdst1] = h16(lo_part(xb));
    }
  };
  __syncthreads();  // X is complete (the prologue's writes)
  for (int idx = tid; idx < XS_RING * NPL * TM; idx += NT) xs16[idx * 8 + 7] = 0x3C00u;  // fp16 1.0: the bias' partner
  stage_store(0, xo[xsrc0], xo[xsrc1]);                                            // x_0
  // a lane's B operand: row 16 rb + m of plane [hi, lo, hi, -][q] (A is zero for q = 3)
  const float* const xb1 = xs + (((q == 1) ? 1 : 0) * TM + m) * 4;
  __syncthreads();

  // a lane's state: rows 16 rb + m, units 16 wv + 4 q + r
  float cst[4][4], hst[4][4];
  int seqr[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      cst[rb][r] = 0.f;  // rnn/LSTMCellZeroState
      hst[rb][r] = 0.f;
    }
    seqr[rb] = seqv[rb * 16 + m];
  }
  const int tmax = misc[1];

  // ---- rnn/while: dynamic_rnn over the other agents; rows past their sequence_length keep their state.
  // h lives in LDS as its two fp16 planes (ONE buffer): every wave reads all 64 units of its rows' h_t, a barrier, every
  // wave splits and stores its own 16 units of h_t+1 (kept in registers until then), a barrier.
  // The step is instantiated per tile height (NRB row blocks); its order of issue is placed by hand (GA3C_PIN / GA3C_FENCE
  // above): stage s = the 28 MFMAs of row block s with the cell update of row block s - 1 as single-instruction micro-ops
  // between them, three behind each MFMA; the planes of x_t+1 are staged behind the first row block's MFMAs, which have no
  // cell update to carry.
  // ALL_LIVE: every real row of the tile has the tile's longest sequence (the usual case: every agent senses every other),
  // so no row ever keeps its state and the two selects per element go.
  auto lstm_steps = [&](auto nrb_c, auto all_live_c) {
    constexpr int NRB = decltype(nrb_c)::value;
    constexpr bool ALL_LIVE = decltype(all_live_c)::value;
    constexpr int NG = ALL_LIVE ? GATE_OPS : GATE_OPS_SEL;
    constexpr int NM = 4 + 2 * NTERM * 4;  // MFMAs of a row block: 4 for x_t and the bias, 24 for h
    static_assert(4 * NM >= GATE_OPS_SEL, "three micro-ops behind every MFMA, four behind the first NG - 3 NM");
#pragma unroll 1
    for (int t = 0; t < tmax; ++t) {
      // operands of row block 0 (h_t and the planes of x_t are complete: the barrier at the end of the previous step)
      const int xoff = (t & (XS_RING - 1)) * (NPL * TM * 4);
      u32x4 h0[NPL], h1[NPL], b1;
      {
        const float* hr = hp + (m * HP_LD + 8 * q) / 2;
        b1 = *reinterpret_cast<const u32x4*>(xb1 + xoff);
#pragma clang loop unroll(full)
        for (int pl = 0; pl < NPL; ++pl) {
          h0[pl] = *reinterpret_cast<const u32x4*>(hr + pl * HP_PLANE);
          h1[pl] = *reinterpret_cast<const u32x4*>(hr + pl * HP_PLANE + 16);
        }
      }
      f32x4 acc[2][4];
      Gate gt;
      float xn0 = 0.f, xn1 = 0.f;
      // stage s: the MFMAs of row block s (s < NRB) with the cell update of row block s - 1 (s >= 1) between them
#pragma clang loop unroll(full)
      for (int s = 0; s <= NRB; ++s) {
        const int cur = s & 1, prv = cur ^ 1;
        const bool live = (s >= 1) ? (t < seqr[s >= 1 ? s - 1 : 0]) : false;
        if (s < NRB) {
#pragma clang loop unroll(full)
          for (int j = 0; j < NM; ++j) {
            const int c = j & 3;
            if (j >= 4) GA3C_PIN(acc[cur][c]);
            if (j < 4) {  // lstm_cell/MatMul of concat[x_t, h] + BiasAdd: the x part and the bias first
              acc[cur][c] = mfma_h(ax[c], b1, f32x4{0.f, 0.f, 0.f, 0.f});
            } else {
              const int ti = (j - 4) >> 2, kb = ti / NTERM, tr = ti % NTERM;
              acc[cur][c] = mfma_h(wh[kb][c][TERM[tr][0]], (kb ? h1 : h0)[TERM[tr][1]], acc[cur][c]);
            }
            GA3C_PIN(acc[cur][c]);
            // row block s - 1's cell update: three micro-ops behind every MFMA, four behind the first NG - 3 NM
            const int XT = (NG > 3 * NM) ? NG - 3 * NM : 0;
            const int g0 = (j < XT) ? 4 * j : 3 * j + XT, n = (j < XT) ? 4 : 3;
#pragma clang loop unroll(full)
            for (int u = 0; u < 4; ++u)
              if (s >= 1 && u < n && g0 + u < NG)
                gate_op<ALL_LIVE>((ALL_LIVE ? GATE_ORDER[(g0 + u) % GATE_OPS] : GATE_ORDER_SEL[(g0 + u) % GATE_OPS_SEL]), gt, acc[prv], cst[s >= 1 ? s - 1 : 0], hst[s >= 1 ? s - 1 : 0], live);
            // the planes of x_t+1 (behind the first row block: the other buffer; nobody reads it before the next step)
            if (s == 0 && j == 2) {
              xn0 = xo[xsrc0 + (t + 1) * 7];  // (t + 1 = 19 behind the last step: in-bounds, never used)
              xn1 = xo[xsrc1 + (t + 1) * 7];
            }
            if (s == 0 && j == 12) stage_store((t + 1) & (XS_RING - 1), xn0, xn1);
            // the next row block's operands as soon as this one's are dead (x: after 4 MFMAs, h0: after 16; h1: at the end)
            if (j == 15 && s + 1 < NRB) {
              const float* hr = hp + (((s + 1) * 16 + m) * HP_LD + 8 * q) / 2;
              b1 = *reinterpret_cast<const u32x4*>(xb1 + xoff + (s + 1) * 16 * 4);
#pragma clang loop unroll(full)
              for (int pl = 0; pl < NPL; ++pl) h0[pl] = *reinterpret_cast<const u32x4*>(hr + pl * HP_PLANE);
            }
            if (j == NM - 1 && s + 1 < NRB) {
              const float* hr = hp + (((s + 1) * 16 + m) * HP_LD + 8 * q) / 2;
#pragma clang loop unroll(full)
              for (int pl = 0; pl < NPL; ++pl) h1[pl] = *reinterpret_cast<const u32x4*>(hr + pl * HP_PLANE + 16);
            }
            GA3C_FENCE();
          }
        }
        if (s == NRB) {  // the last row block's cell update has no MFMAs to hide behind (the SIMD's other wave has)
#pragma clang loop unroll(full)
          for (int u = 0; u < NG; ++u) gate_op<ALL_LIVE>((ALL_LIVE ? GATE_ORDER[u % GATE_OPS] : GATE_ORDER_SEL[u % GATE_OPS_SEL]), gt, acc[prv], cst[s - 1], hst[s - 1], live);
          GA3C_FENCE();
        }
      }
      __syncthreads();  // every wave has read h_t
#pragma clang loop unroll(full)
      for (int rb = 0; rb < NRB; ++rb) {
        float* hw = hp + ((rb * 16 + m) * HP_LD + wv * 16 + 4 * q) / 2;  // units 16 wv + 4 q .. + 3 of row 16 rb + m
        const float a0 = hst[rb][0], a1 = hst[rb][1], a2 = hst[rb][2], a3 = hst[rb][3];
        *reinterpret_cast<uint2*>(hw) = make_uint2(pk2(a0, a1), pk2(a2, a3));
        *reinterpret_cast<uint2*>(hw + HP_PLANE) = make_uint2(pk2(lo_part(a0), lo_part(a1)), pk2(lo_part(a2), lo_part(a3)));
      }
      __syncthreads();  // h_t+1 and the planes of x_t+1 are complete
    }
  };
  const bool all_live = misc[2] >= tmax;
  using std::integral_constant;
  if (all_live) {
    if (nrb == 4) lstm_steps(integral_constant<int, 4>{}, integral_constant<bool, true>{});
    else if (nrb == 3) lstm_steps(integral_constant<int, 3>{}, integral_constant<bool, true>{});
    else lstm_steps(integral_constant<int, 2>{}, integral_constant<bool, true>{});
  } else {
    if (nrb == 4) lstm_steps(integral_constant<int, 4>{}, integral_constant<bool, false>{});
    else if (nrb == 3) lstm_steps(integral_constant<int, 3>{}, integral_constant<bool, false>{});
    else lstm_steps(integral_constant<int, 2>{}, integral_constant<bool, false>{});
  }

  // ---- layer1_input = concat[host, h_final]: h_final = the planes the last step wrote (all zero without a step), the
  // four host inputs go through one exact f32 MFMA.  The activations take over the LSTM's LDS after the barrier.
  f32x4 acc[4][4];
  auto zero_acc = [&]() {
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  };
  zero_acc();
  {
    float w1[4], hv4[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) w1[cb] = g.net.layer1_kernel[q * 256 + wv * 64 + cb * 16 + m];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) hv4[rb] = hostv[(rb * 16 + m) * 4 + q];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      if (rb >= nrb) continue;
#pragma unroll
      for (int cb = 0; cb < 4; ++cb) acc[rb][cb] = mfma4(w1[cb], hv4[rb], acc[rb][cb]);
    }
  }
  dense_t<2, true>(hp, 0, pk + PK_L1, acc, lane, m, q, wv, nrb);  // layer1/MatMul
  __syncthreads();
  store_relu_t(act, g.net.layer1_bias, acc, m, q, wv, nrb, amax);  // layer1/BiasAdd, layer1/Relu
  __syncthreads();
  zero_acc();
  if (nrb == 4) dense_pipe<8, 4>(act, ACT_LD, pk + PK_L2, acc, lane, m, q, wv);
  else if (nrb == 3) dense_pipe<8, 3>(act, ACT_LD, pk + PK_L2, acc, lane, m, q, wv);
  else dense_pipe<8, 2>(act, ACT_LD, pk + PK_L2, acc, lane, m, q, wv);  // layer2
  __syncthreads();
  store_relu_t(act, g.net.layer2_bias, acc, m, q, wv, nrb, amax);
  __syncthreads();
  zero_acc();
  if (nrb == 4) dense_pipe<8, 4>(act, ACT_LD, pk + PK_FC1, acc, lane, m, q, wv);
  else if (nrb == 3) dense_pipe<8, 3>(act, ACT_LD, pk + PK_FC1, acc, lane, m, q, wv);
  else dense_pipe<8, 2>(act, ACT_LD, pk + PK_FC1, acc, lane, m, q, wv);  // fullyconnected1
  __syncthreads();
  store_relu_t(act, g.net.fc1_bias, acc, m, q, wv, nrb, amax_unused);
  __syncthreads();

  // ---- logits_p: 11 columns = one (padded) column block; wave w takes row block w.  EXT: column 11 of the block is
  // logits_v (the value head, `Squeeze` of the graph) on the same exact-f32 MFMA; the columns do not see each other.
  if (wv < nrb) {  // (wave-uniform)
    f32x4 lacc = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* ap = act + (wv * 16 + m) * ACT_LD + q * 64;
    // all 64 weights of this lane first (clamped column + select: no branch, one memory latency), then the MFMAs
    const int mc = m < 11 ? m : 0;
    float keep = m < 11 ? 1.f : 0.f;
    const float* wp = g.net.logits_kernel + (q * 64) * 11 + mc;
    const float* bp = g.net.logits_bias + mc;
    int ws = 11;
    if constexpr (EXT) {
      if (m == 11 && ex.value_kernel) {  // logits_v/kernel [256, 1], bias [1]
        wp = ex.value_kernel + q * 64;
        bp = ex.value_bias;
        ws = 1;
        keep = 1.f;
      }
    }
    float lw[64];
#pragma unroll
    for (int kk = 0; kk < 64; ++kk) lw[kk] = wp[kk * ws];
    const float bb = *bp * keep;
#pragma unroll
    for (int kk = 0; kk < 64; kk += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(ap + kk);
#pragma unroll
      for (int u = 0; u < 4; ++u) lacc = mfma4(v[u], lw[kk + u] * keep, lacc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) lg[(wv * 16 + q * 4 + r) * 16 + m] = lacc[r] + bb;
  }
  __syncthreads();

  if (!(amax < 65504.f)) atomicOr(&g_fault, 2u);
  (void)amax_unused;
  // ---- argmax(Softmax) -> index into network.Actions (GA3CCADRLPolicy.py:81-83); ties -> first, like np.argmax
  if (tid < TM && need) {
    const long i = row_of(tid);
    const float* l = lg + tid * 16;
    int best = 0;
    float bv = l[0];
#pragma unroll
    for (int c = 1; c < 11; ++c)
      if (l[c] > bv) {
        bv = l[c];
        best = c;
      }
    if constexpr (EXT) {
      if (g.ext) {
        g.ext[2 * i] = static_cast<double>(best);
        g.ext[2 * i + 1] = 0.0;
      }
      if (ex.action) ex.action[i] = best;
      if (ex.value) ex.value[i] = l[11];
    } else {
      g.ext[2 * i] = static_cast<double>(best);
      g.ext[2 * i + 1] = 0.0;
    }
    if (g.logits)
      for (int c = 0; c < 11; ++c) g.logits[i * 11 + c] = l[c];
  }
}

}  // namespace ga3c
