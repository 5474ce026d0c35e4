// Batched policy forward: the convolutional head of
// the reference actor (network.py:70-82, MLP.forward) for B observation rows at
// once — conv 1->5 (3x3, pad 1) over the 7x7 terrain window, BatchNorm, ReLU,
// 2x2 max pool, conv 5->8, BatchNorm, ReLU, 2x2 max pool, linear 8->12, then the
// LayerNorm over [head, rest of the observation] (network.py:83-85). This is
// the part of the network with no batched BLAS form (per-row BatchNorm
// statistics over 7x7 / 3x3 maps); the tanh MLP and Normal heads run as batched
// GEMMs in lnw.rollout.BatchedActor.
//
// One thread per row; the packed parameters (578 + 2 n_in floats, order below,
// written by BatchedActor.packed_features()) are staged once per workgroup in
// LDS and read as broadcasts. Channels are streamed (49 conv outputs live at a
// time).
// bn_running = 0 normalises with each row's own statistics (the reference's
// one-state-at-a-time training-mode calls, ppo.py:504-512), 1 with the running
// ones.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <type_traits>

#include "lnw.h"
#include "lnw_device.h"

namespace {

using namespace lnw;

typedef double f64x4 __attribute__((ext_vector_type(4)));

// the conv head (bn_relu, conv_head_win, conv_head_row, load_tail_q), its packed
// parameter layout and the supported observation width (MAX_IN, obs_width_ok)
#include "lnw_convhead.inc"
// the packed parameter set's layout (FC1 .. NOUT, mlp_bf16x8, policy_pack)
#include "lnw_policypack.inc"

constexpr float LN_EPS = 1e-5f;

extern __shared__ float actor_lds[];

constexpr int CH_THREADS = 256;
constexpr int PA_THREADS = 512;  // lnw_policy_act's block

// LayerNorm over [h, tail] (biased variance; tail = x[49:], n_in - 12 values)
// with its affine, into u[0..n_in)
template <int NI>
__device__ __forceinline__ void layer_norm_tail(const float *P, const float (&tl)[NI - 12], int n_in,
                                                const float (&h)[12], float (&u)[NI]) {
#pragma unroll
  for (int k = 0; k < NI; k++) u[k] = k < 12 ? h[k < 12 ? k : 0] : (k < n_in ? tl[k < 12 ? 0 : k - 12] : 0.f);
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < NI; k++) s += k < n_in ? u[k] : 0.f;
  const float mean = s / (float)n_in;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < NI; k++) q += k < n_in ? (u[k] - mean) * (u[k] - mean) : 0.f;
  const float inv = 1.0f / sqrtf(q / (float)n_in + LN_EPS);
  const float *lw = P + CONV_PARAMS, *lb = P + CONV_PARAMS + n_in;
#pragma unroll
  for (int k = 0; k < NI; k++) u[k] = k < n_in ? (u[k] - mean) * inv * lw[k] + lb[k] : 0.f;
}

// the LayerNorm tail of a row in memory: x[49 .. D - 1], every load issued at
// once (indices clamped into the row, values past n_in - 12 unused)
template <int NT>
__device__ __forceinline__ void load_tail(const float *x, int D, float (&tl)[NT]) {
#pragma unroll
  for (int k = 0; k < NT; k++) tl[k] = x[WIN + k < D ? WIN + k : D - 1];
}

// (the torch implementation's conv head, off the fused path: one wave per
// SIMD, so the compiler has the registers to keep the head out of scratch)
template <int NI>
__global__ __launch_bounds__(CH_THREADS, 1) void features_kernel(const float *params, int obs_dim,
                                                              const float *obs, int B, int bn_running,
                                                              float *out) {
  const int n_in = obs_dim - WIN + 12;
  const int n_par = CONV_PARAMS + 2 * n_in;
  float *P = actor_lds;                           // [n_par] parameters
  // pooled conv1 maps: per wave [45][64], one column per lane (as lnw_policy_act)
  float *pool1 = actor_lds + n_par + (threadIdx.x / WAVE) * 45 * WAVE + (threadIdx.x & (WAVE - 1));
  for (int i = threadIdx.x; i < n_par; i += blockDim.x) P[i] = params[i];
  __syncthreads();
  const bool running = bn_running != 0;
  // (one row per thread, 32-bit row indices checked on the host; the tail is
  // loaded after the head: nothing but the row index lives across it)
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row < B) {
    float h[12];
    conv_head_row(P, obs + (long long)row * obs_dim, pool1, WAVE, running, h);
    float tl[NI - 12], u[NI];
    load_tail(obs + (long long)row * obs_dim, obs_dim, tl);
    layer_norm_tail<NI>(P, tl, n_in, h, u);
    float *o = out + (long long)row * n_in;
#pragma unroll
    for (int k = 0; k < NI; k++)
      if (k < n_in) o[k] = u[k];
  }
}

// ---------------------------------------------------------------------------
// Fused policy step (lnw_policy_act): for every row of one side's observation
// block, the whole reference actor forward (network.py:70-115 / get_dist
// :117-152) and what the MAPPO rollout does with it (ppo.py:497-577) in one
// launch, one thread per row:
//   conv head + LayerNorm (as features_kernel), then fc1 64 / fc2 64 / fc3 32
//   tanh layers and the normal / log-std heads with weights read as wave-
//   uniform scalar loads (every lane of the wave uses the same weight), fp32
//   FMA;
//   NaN heads -> N(0, 1) for the row (the reference returns None there);
//   sample: N(mean, std) from keyed Philox normals (+ N(0, noise)), clamped to
//   [0, 1], and its log-probability; or, forced, the log-probability of given
//   actions (get_dist); or, script_self, that of the side's own scripted row
//   (a learning red side's warm-up, ppo.py:552-557), the row's float64 value
//   going to lnw_step as it stands in the table, no draw consumed;
//   outputs: the f64 action rows of lnw_step (sunk ships 0), the rollout's
//   action / log-probability rows (0 after the episode ended) and the
//   observation copy for the rollout buffer; the lane of ship 0 also writes its
//   env's scripted red rows (red_steps*.csv, ppo.py:560-566) and the action
//   array's row kinds (np.asarray, ppo.py:577).
// Keyed draws (keyed_normal in lnw/rollout.py): uniform k of global row r at
// Philox counter (slot << 40) / 4 + 2 r (+1), slot = (call * T + t) * 4 + which;
// eps = sqrt(-2 log1p(-u_c)) cos(2 pi u_{4+c}); `call` is read from device
// memory so a replayed graph draws fresh values every rollout.
// ---------------------------------------------------------------------------
struct PolicyArgs {
  lnw_policy_args a;
  int n_in;
  int off_b1, off_w1;  // packed MLP: biases b1 | b2 | b3, then the MFMA weight fragments (floats)
};

__device__ __forceinline__ void philox_u8(unsigned long long seed, unsigned long long ctr0, float (&u)[8]) {
#pragma unroll
  for (int b = 0; b < 2; b++) {
    float ub[4];
    philox_u4(seed, ctr0 + (unsigned long long)b, ub);
#pragma unroll
    for (int k = 0; k < 4; k++) u[4 * b + k] = ub[k];
  }
}

// standard normals of (slot, global row): keyed_normal's construction
__device__ __forceinline__ void keyed_eps(unsigned long long seed, unsigned long long slot, long long grow,
                                          float (&eps)[NOUT]) {
  float u[8];
  philox_u8(seed, (slot << 38) + (unsigned long long)grow * 2ull, u);
#pragma unroll
  for (int c = 0; c < NOUT; c++) eps[c] = box_muller(u[c], u[4 + c]);
}

// ---- the MLP on the matrix cores -------------------------------------------
// Each wave runs its 64 rows through fc1 / fc2 / fc3 and the two heads with
// v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation), transposed:
// Y^T = W X^T, so the weights are the A operand (lane l: W[n = 16 nt + (l & 15)]
// [k]) and the activations the B operand (lane l: X[r = 16 rt + (l & 15)][k]),
// and a layer's output tile (lane l, register v: Y[r = 16 rt + (l & 15)]
// [n = 16 nt + 4 (l >> 4) + v]) is already the next layer's B operand for the
// k-steps "quad q = nt, element v" — no LDS round trip between layers. Every
// layer therefore sums over k in the order k = 16 q + 4 g + v (g = l >> 4), and
// the host packs each weight matrix as fragments in that order
// (BatchedActor.packed_policy): float4 [nt][q][lane] = W[16 nt + (lane & 15)]
// [16 q + 4 (lane >> 4) + 0..3], read with one 16-B load per lane.
// The first layer's input (the LayerNorm output, one row per lane) goes through
// a wave-private LDS tile [64 rows][KS] to reach the same layout.
typedef float f32x4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4v mfma4(float a, float b, f32x4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// acc[rt][nt] += W (frags F, NTO output tiles, Q quads) x X (B operand quads
// xq[rt][q] of float4 = 4 k-steps)
template <int NTO, int Q>
__device__ __forceinline__ void mfma_layer(const f32x4v *__restrict__ F, const f32x4v (&xb)[4][Q],
                                           f32x4v (&acc)[4][NTO], int lane) {
#pragma unroll
  for (int q = 0; q < Q; q++) {
    f32x4v w[NTO];
#pragma unroll
    for (int nt = 0; nt < NTO; nt++) w[nt] = F[(nt * Q + q) * WAVE + lane];
#pragma unroll
    for (int v = 0; v < 4; v++)
#pragma unroll
      for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int nt = 0; nt < NTO; nt++) acc[rt][nt] = mfma4(w[nt][v], xb[rt][q][v], acc[rt][nt]);
  }
}

// The same layers on the bf16 matrix cores at f32 accuracy (lnw_policy_act):
// v_mfma_f32_16x16x32_bf16, lane l holding A[l & 15][k = 8 (l >> 4) + j] and
// B[k][l & 15], j = 0..7. Element j of a k-pair p is neuron 32 p + 16 (j / 4) +
// 4 (l >> 4) + j % 4, so the B operand of pair p is just the two f32 quads
// (2p, 2p + 1) of mfma_layer's layout: the chaining stays register-only. Each
// f32 value is split exactly into three bfloat16 terms (x = x0 + x1 + x2, each
// rounded to nearest: 8 + 8 + 8 bits), the weights on the host
// (BatchedActor.packed_policy: planes hi, mid, lo), the activations here; of
// the nine partial products the six above 2^-24 relative are summed (small
// ones first), so a product is exact to about 3 ulp of f32 and the sums match
// the f32 MFMA's within a few ulp, at 6 x 16 cycles per 32 k instead of the
// f32 form's 8 x 32.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split3(const f32x4v &a, const f32x4v &b, bf16x8 &x0, bf16x8 &x1, bf16x8 &x2) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const float x = j < 4 ? a[j] : b[j - 4];
    const __bf16 h = (__bf16)x;
    const float r = x - (float)h;
    const __bf16 m = (__bf16)r;
    x0[j] = h;
    x1[j] = m;
    x2[j] = (__bf16)(r - (float)m);
  }
}

__device__ __forceinline__ f32x4v mfma32(const bf16x8 &a, const bf16x8 &b, f32x4v c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// acc[rt][nt] += W (planes F: hi | mid | lo, each bf16x8 [nt][p][lane]) x X
template <int NTO, int Q>
__device__ __forceinline__ void mfma_layer3(const bf16x8 *__restrict__ F, const f32x4v (&xb)[4][Q],
                                            f32x4v (&acc)[4][NTO], int lane) {
  static_assert(Q % 2 == 0, "k in pairs of quads");
  constexpr int QP = Q / 2, PL = NTO * QP * WAVE;  // plane stride (bf16x8)
#pragma unroll
  for (int p = 0; p < QP; p++) {
    bf16x8 b0[4], b1[4], b2[4];
#pragma unroll
    for (int rt = 0; rt < 4; rt++) split3(xb[rt][2 * p], xb[rt][2 * p + 1], b0[rt], b1[rt], b2[rt]);
#pragma unroll
    for (int nt = 0; nt < NTO; nt++) {
      const int i = (nt * QP + p) * WAVE + lane;
      const bf16x8 w0 = F[i], w1 = F[PL + i], w2 = F[2 * PL + i];
#pragma unroll
      for (int rt = 0; rt < 4; rt++) acc[rt][nt] = mfma32(w2, b0[rt], acc[rt][nt]);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) acc[rt][nt] = mfma32(w1, b1[rt], acc[rt][nt]);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) acc[rt][nt] = mfma32(w0, b2[rt], acc[rt][nt]);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) acc[rt][nt] = mfma32(w1, b0[rt], acc[rt][nt]);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) acc[rt][nt] = mfma32(w0, b1[rt], acc[rt][nt]);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) acc[rt][nt] = mfma32(w0, b0[rt], acc[rt][nt]);
    }
  }
}

template <int NTO>
__device__ __forceinline__ void bias_init(const float *__restrict__ b, f32x4v (&acc)[4][NTO], int g) {
#pragma unroll
  for (int nt = 0; nt < NTO; nt++) {
    const f32x4v bv = *(const f32x4v *)(b + nt * 16 + 4 * g);
#pragma unroll
    for (int rt = 0; rt < 4; rt++) acc[rt][nt] = bv;
  }
}

// tanh(x) = 1 - 2 / (e^(2x) + 1) with the hardware exp2 and reciprocal
// (v_exp_f32, v_rcp_f32: ~1 ulp each): absolute error below 3e-7 over the
// whole range (+-1 exactly at overflow), against ~40 instructions of ocml's
// tanhf. The policy tolerances are 1e-4 (log-probabilities) and 1e-5 (values).
__device__ __forceinline__ float tanh_fast(float x) {
  const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);  // e^(2x) = 2^(2x log2 e)
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

template <int NTO>
__device__ __forceinline__ void tanh_all(f32x4v (&acc)[4][NTO]) {
#pragma unroll
  for (int rt = 0; rt < 4; rt++)
#pragma unroll
    for (int nt = 0; nt < NTO; nt++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[rt][nt][v] = tanh_fast(acc[rt][nt][v]);
}

// fc1 / fc2 / fc3 and both heads of the wave's 64 rows on the matrix cores
// (xb: fc1's B operand), then each row's head outputs brought to its own lane
template <int Q1, class PF>
__device__ __forceinline__ void mlp_heads(const PolicyArgs &pa, PF pofs, const bf16x8 *Fw, const float *xt,
                                          int lane, int g, int m, float (&mean)[NOUT], float (&lsd)[NOUT]) {
  constexpr int KS = 16 * Q1 + 4;  // the tile's row stride (policy_act_kernel)
  const lnw_policy_args &a = pa.a;
  f32x4v xb[4][Q1];
#pragma unroll
  for (int rt = 0; rt < 4; rt++)
#pragma unroll
    for (int q = 0; q < Q1; q++) xb[rt][q] = *(const f32x4v *)(xt + (rt * 16 + m) * KS + 16 * q + 4 * g);
  // weights: three bf16 planes per layer (mfma_layer3), layers in order
  // Fw: the three bf16 planes of every layer (global, or the block's LDS copy)
  constexpr int O2 = 3 * 4 * (Q1 / 2) * WAVE, O3 = O2 + 3 * 4 * 2 * WAVE, OH = O3 + 3 * 2 * 2 * WAVE;
  // b1 [64] | b2 [64] | b3 [32] of the block's parameter set (pofs() floats into params)
  const float *bias = a.params + pofs() + pa.off_b1;
  f32x4v h1[4][4];
  bias_init<4>(bias, h1, g);
  mfma_layer3<4, Q1>(Fw, xb, h1, lane);
  tanh_all<4>(h1);
  f32x4v h2[4][4];
  bias_init<4>(bias + 64, h2, g);
  mfma_layer3<4, 4>(Fw + O2, h1, h2, lane);
  tanh_all<4>(h2);
  f32x4v h3[4][2];
  bias_init<2>(bias + 128, h3, g);
  mfma_layer3<2, 4>(Fw + O3, h2, h3, lane);
  tanh_all<2>(h3);
  f32x4v hh[4][1];
#pragma unroll
  for (int rt = 0; rt < 4; rt++) hh[rt][0] = f32x4v{0.f, 0.f, 0.f, 0.f};
  mfma_layer3<1, 2>(Fw + OH, h3, hh, lane);
  // head outputs of row 16 rt + m sit in lane m (normal head, n = v) and lane
  // 16 + m (log-std head, n = 4 + v) of tile rt: bring row `lane` to lane
  // `lane` (rt = g) for the per-row sampling below
#pragma unroll
  for (int v = 0; v < NOUT; v++) {
    float mv = 0.f, lv = 0.f;
#pragma unroll
    for (int rt = 0; rt < 4; rt++) {
      const float sm = __shfl(hh[rt][0][v], m);
      const float sl = __shfl(hh[rt][0][v], 16 + m);
      mv = g == rt ? sm : mv;
      lv = g == rt ? sl : lv;
    }
    mean[v] = mv;
    lsd[v] = lv;
  }
}

// A wave's rows up to the fc1 tile: conv head + LayerNorm (one row per lane),
// the observation copy for the rollout buffer, and the LayerNorm outputs into
// the wave's fc1 input tile in LDS (xt) for mlp_heads.
// (R: the type of row indices, long long, or int in the population kernel)
template <int NI, class R>
__device__ __forceinline__ void head_to_tile(const PolicyArgs &pa, const float *P, float *warea, int lane,
                                             bool valid, long long e, int i, long long istride, R r0, R rows) {
  constexpr int KS = NI + 4;
  const lnw_policy_args &a = pa.a;
  const int n = a.n, D = a.D, n_in = pa.n_in;
  // ---- conv head + LayerNorm, one row per lane -------------------------------
  // The row's window and LayerNorm tail are loaded once, every load issued
  // together, into registers (the tail's loads were one dependent round trip
  // each behind the k < n_in guard).
  float u[NI];
  if (valid) {
    float h[12];
    {
      const float *x = a.obs + e * istride + (long long)i * D;
      float win[WIN];
#pragma unroll
      for (int k = 0; k < WIN; k++) win[k] = x[k];
      conv_head_win(P, win, warea + lane, WAVE, a.bn_running != 0, h);
    }
    // the tail after the head (its registers are the head's), one batch of loads;
    // the row's address again from an opaque copy of the row index, so no 64-bit
    // address lives across the head (where the register file is full: it went
    // to scratch, and the kernel with it)
    float tl[NI - 12];
    int r_t = (int)(r0 + (threadIdx.x & ~(WAVE - 1)) + lane);
    asm volatile("" : "+v"(r_t));
    const int e_t = r_t / n, i_t = r_t - e_t * n;
    const float *xt = a.obs + (long long)e_t * istride + (long long)i_t * D;
    load_tail_q(xt, D >> 2, tl);
    layer_norm_tail<NI>(P, tl, n_in, h, u);
  } else {
#pragma unroll
    for (int k = 0; k < NI; k++) u[k] = 0.f;
  }
  // ---- observation copy for the rollout buffer: the wave's 64 rows, float4
  // chunks (coalesced; the rows are L2-warm from the conv head's reads). Here,
  // between the VALU-bound head and the MFMA layers, rather than ahead of the
  // head: every workgroup starts at once, so a copy there left the memory
  // system idle during the compute and the ALUs idle during the copy.
  // (in place: lnw_observe_ex wrote the rows into the rollout buffer itself;
  // only the rows of envs whose episode ended are zeroed)
  const bool in_place = a.obs_out == a.obs && a.obs_env_stride == istride;
  if (a.obs_out && (!in_place || a.live)) {
    const int D4 = D >> 2;
    const R rw = r0 + (threadIdx.x & ~(WAVE - 1));
    const R nr = rows - rw < WAVE ? rows - rw : WAVE;
    for (int q = lane; q < nr * D4; q += WAVE) {
      const R rr = rw + q / D4;
      const int c4 = q - (q / D4) * D4;
      const R ee = rr / n;
      const int ii = (int)(rr - ee * n);
      const bool dead = a.live && !a.live[ee];
      if (in_place && !dead) continue;
      f32x4 v = dead ? f32x4{0.f, 0.f, 0.f, 0.f}
                     : *(const f32x4 *)(a.obs + (long long)ee * istride + (long long)ii * D + 4 * c4);
      *(f32x4 *)(a.obs_out + (long long)ee * a.obs_env_stride + (long long)ii * D + 4 * c4) = v;
    }
  }
  // ---- fc1 input tile: the wave's rows into the MFMA B layout ---------------
  // (over the wave's own conv1 area: its lanes are done with it, and a wave's
  // LDS operations complete in order)
  float *xt = warea;
#pragma unroll
  for (int k4 = 0; k4 < NI / 4; k4++)
    *(f32x4v *)(xt + lane * KS + 4 * k4) = f32x4v{u[4 * k4], u[4 * k4 + 1], u[4 * k4 + 2], u[4 * k4 + 3]};
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The phases of a block. PA_THREADS = 512 (one block per CU, two waves per
// SIMD): every wave runs its head, a barrier, then every wave its MLP. A wave's
// head (its conv, LayerNorm and fc1 tile) running while the other wave of its
// SIMD ran its MLP (v_mfma_f32_16x16x32_bf16 chains) came out wrong in lanes
// 48-63 of the head's wave ("The policy kernel's nondeterminism");
// heads beside heads and MLPs beside MLPs are exact. (One block per CU: the
// block's LDS is larger than half the CU's, so no other block's head shares a
// SIMD with these MLPs.)
template <int NI, class PF, class R>
__device__ __forceinline__ void head_and_mlp(const PolicyArgs &pa, const float *P, PF pofs, const bf16x8 *Fw,
                                             float *warea, int lane, int g, int m, bool valid, long long e, int i,
                                             long long istride, R r0, R rows, float (&mean)[NOUT],
                                             float (&lsd)[NOUT]) {
  constexpr int Q1 = NI / 16;
  head_to_tile<NI>(pa, P, warea, lane, valid, e, i, istride, r0, rows);
  __syncthreads();  // every head done before any MLP
  mlp_heads<Q1>(pa, pofs, Fw, warea, lane, g, m, mean, lsd);
}

// Population launch (lnw_policy_act_pop): the local envs in members of G
// consecutive envs, member k acting with the packed set at params + k *
// member_stride. A workgroup serves rows of one member only: block b of member
// k (blockIdx.x = k * bpm + b) takes the member's rows [512 b, 512 b + 512) of
// its G n (fewer in the last member).
struct PolicyPopArgs : PolicyArgs {
  int member_rows;    // G n
  int member_stride;  // floats between the members' packed sets
  int bpm;            // blocks per member
};

template <bool POP>
using PolicyKernelArgs = std::conditional_t<POP, PolicyPopArgs, PolicyArgs>;

template <int NI, bool POP>
__global__ __launch_bounds__(PA_THREADS, 1) void policy_act_kernel(PolicyKernelArgs<POP> pa) {
  constexpr int KS = NI + 4;         // row stride of the wave's fc1 input tile (16-B aligned)
  const lnw_policy_args &a = pa.a;
  const int n_in = pa.n_in;
  const int n_par = CONV_PARAMS + 2 * n_in;
  float *P = actor_lds;                // [n_par] conv head + LayerNorm parameters
  // per wave: [45][64] pooled conv1 maps (one column per lane), then the
  // wave's fc1 input tile [64][KS] over the same floats
  constexpr int WAREA = (45 > KS ? 45 : KS) * WAVE;
  float *warea = actor_lds + ((n_par + 3) & ~3) + (threadIdx.x / WAVE) * WAREA;
  // the block's member (POP), from blockIdx at every use through an opaque
  // copy, so that nothing of it lives across the head, where the registers are
  // full; and its parameter set within params: the one set (0), or its member's
  auto member = [&]() {
    int k = 0;
    if constexpr (POP) {
      k = blockIdx.x / pa.bpm;
      asm volatile("" : "+s"(k));
    }
    return k;
  };
  auto pofs = [&]() -> long long {
    if constexpr (POP) return (long long)member() * pa.member_stride;
    else return 0;
  };
  for (int i = threadIdx.x; i < n_par; i += blockDim.x) P[i] = a.params[pofs() + i];
  // the MLP's weights (three bf16 planes per layer, mlp_bf16x8<NI> of them):
  // at NI = 32 a copy in LDS after the wave areas, loaded once per block while
  // the heads run, so each wave's MFMA chains read their A operands from LDS
  // instead of 51 KB apiece from L2 (at NI = 64 they do not fit beside the
  // larger tiles and stay in global memory)
  const bf16x8 *Fw = (const bf16x8 *)(a.params + pofs() + pa.off_w1);
  if constexpr (NI == 32) {
    bf16x8 *wl = (bf16x8 *)(actor_lds + ((n_par + 3) & ~3) + (PA_THREADS / WAVE) * WAREA);
    for (int i = threadIdx.x; i < mlp_bf16x8<NI>(); i += blockDim.x) wl[i] = Fw[i];
    Fw = wl;
  }
  const int n = a.n, D = a.D;
  // the block's first row and the end of its rows: every row in order, or (POP)
  // the rows of its member, there as 32-bit values (rows + PA_THREADS < 2^31,
  // checked on the host): with 64-bit ones the 64-wide kernel spilled 8 B more
  using R = std::conditional_t<POP, int, long long>;
  auto block_rows = [&](R &first, R &end) {
    if constexpr (POP) {
      const int k = member();
      const long long all = a.E * n, mend = (long long)(k + 1) * pa.member_rows;
      end = (int)(mend < all ? mend : all);
      first = k * pa.member_rows + (int)(blockIdx.x - k * pa.bpm) * PA_THREADS;
    } else {
      end = a.E * n;
      first = (long long)blockIdx.x * PA_THREADS;
    }
  };
  R r0, rows;
  block_rows(r0, rows);
  const long long istride = a.obs_in_env_stride ? a.obs_in_env_stride : (long long)n * D;
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1), g = lane >> 4, m = lane & 15;
  const R r = r0 + threadIdx.x;
  const bool valid = r < rows;  // (every lane stays for the wave-wide MFMAs)
  // (32-bit: rows < 2^31, checked on the host; fewer registers live across the head)
  const int e32 = valid ? (int)r / n : 0;
  const long long e = e32;
  const int i = valid ? (int)r - e32 * n : 0;
  const long long E = a.E;
  const bool alive = valid && a.alive[(long long)(a.own0 + i) * E + e] != 0;
  const bool live = !a.live || (valid && a.live[e] != 0);
  // ---- env-level side work by the lane of ship 0 ---------------------------
  if (valid && i == 0) {
    if (a.script) {  // scripted rows: profile j for red ship j < script_n, zeros past the table
      for (int j = 0; j < a.script_cnt; j++) {
        const int ag = a.script_own0 + j;
        const bool al = a.alive[(long long)ag * E + e] != 0;
        const bool has = j < a.script_n && a.t < a.script_steps;
        f64x4 v = {0.0, 0.0, 0.0, 0.0};
        if (al && has) v = *(const f64x4 *)(a.script + ((long long)j * a.script_steps + a.t) * 4);
        *(f64x4 *)(a.full + (e * a.A + ag) * 4) = v;
      }
    }
    if (a.kinds) {
      bool all = true;
      for (int ag = 0; ag < a.A; ag++) all = all && a.alive[(long long)ag * E + e] != 0;
      const uint8_t k = (a.kinds_f32_all_alive && all) ? (uint8_t)LNW_KIND_F32 : (uint8_t)LNW_KIND_F64;
      for (int ag = 0; ag < a.A; ag++) a.kinds[e * a.A + ag] = k;
      if (a.f32_out) a.f32_out[e * a.f32_env_stride] = k == LNW_KIND_F32 ? 1 : 0;
    }
  }
  // ---- head, fc1 tile and MLP (phases: head_and_mlp) --------------------------
  float mean[NOUT], lsd[NOUT];
  head_and_mlp<NI>(pa, P, pofs, Fw, warea, lane, g, m, valid, e, i, istride, r0, rows, mean, lsd);
  if (!valid) return;
  // the row's env and ship again, from an opaque copy of the row index: so
  // they are recomputed here instead of living across the head (where the
  // register file is full and they would go to scratch)
  int r_o = (int)(blockIdx.x * PA_THREADS + threadIdx.x);
  if constexpr (POP) {  // (from blockIdx again: nothing of it lives across the head)
    R first, end;
    block_rows(first, end);
    r_o = (int)first + (int)threadIdx.x;
  }
  asm volatile("" : "+v"(r_o));
  const int e_o = r_o / n, i_o = r_o - e_o * n;
  float std_[NOUT];
  bool ok = true;
#pragma unroll
  for (int o = 0; o < NOUT; o++) {
    // (the hardware exp2 / reciprocal forms: tanh_fast's absolute error < 3e-7,
    // __expf's a few ulp; NaN, +-inf and overflow behave as tanhf / expf)
    mean[o] = tanh_fast(mean[o]);
    std_[o] = __expf(lsd[o]);
    ok = ok && !isnan(mean[o]) && !isnan(std_[o]);
  }
  // ---- sample / forced actions and log-probabilities -----------------------
  float act[NOUT], lp[NOUT];
  if (a.forced) {  // MLP.get_dist (network.py:117-152): no NaN guard
    const float *fa = a.forced_act + (long long)e_o * a.fa_env_stride + 4 * i_o;
#pragma unroll
    for (int o = 0; o < NOUT; o++) act[o] = fa[o];
  } else if (a.script_self) {  // the side's own scripted rows (ppo.py:552-557): get_dist of the f32 row
    f64x4 sv = {0.0, 0.0, 0.0, 0.0};
    if (i_o < a.script_n && a.t < a.script_steps)
      sv = *(const f64x4 *)(a.script + ((long long)i_o * a.script_steps + a.t) * 4);
#pragma unroll
    for (int o = 0; o < NOUT; o++) act[o] = (float)sv[o];
    // the step takes the table's float64 row itself, not the rounded one
    if (a.full) {
      if (!alive) sv = f64x4{0.0, 0.0, 0.0, 0.0};
      *(f64x4 *)(a.full + ((long long)e_o * a.A + a.own0 + i_o) * 4) = sv;
    }
  } else {
    if (!ok) {
#pragma unroll
      for (int o = 0; o < NOUT; o++) { mean[o] = 0.f; std_[o] = 1.f; }
    }
    const unsigned long long call = a.call_dev ? (unsigned long long)*a.call_dev : 0ull;
    const unsigned long long slot = (call * (unsigned long long)a.T + (unsigned long long)a.t) * 4ull;
    const long long grow = a.row_base + r_o;
    float eps[NOUT];
    keyed_eps(a.seed, slot + (unsigned long long)a.which, grow, eps);
#pragma unroll
    for (int o = 0; o < NOUT; o++) act[o] = mean[o] + std_[o] * eps[o];
    if (a.noise > 0.f) {
      float ne[NOUT];
      keyed_eps(a.seed, slot + (unsigned long long)a.which + 1ull, grow, ne);
#pragma unroll
      for (int o = 0; o < NOUT; o++) act[o] = act[o] + a.noise * ne[o];
    }
#pragma unroll
    for (int o = 0; o < NOUT; o++) act[o] = fminf(fmaxf(act[o], 0.f), 1.f);
  }
  // Normal.log_prob (torch.distributions): -((x - m)^2) / (2 var) - log(std) - log(sqrt(2 pi))
#pragma unroll
  for (int o = 0; o < NOUT; o++) {
    const float d = act[o] - mean[o];
    const float s = std_[o];
    // log(std) is the log-scale itself (the guarded rows carry std 1: log 0), except
    // where an f32 exp overflows to inf or rounds to 0 (below ln 2^-150; the hardware
    // exp may flush the denormals above that, whose log the log-scale stays), as
    // torch's log(exp(.)) does; v_rcp_f32 for 1 / var (1 ulp)
    const float l = (a.forced || a.script_self || ok) ? lsd[o] : 0.f;
    const float ls = (s < INFINITY && l > -103.972f) ? l : logf(s);
    lp[o] = -(d * d) * (0.5f * __builtin_amdgcn_rcpf(s * s)) - ls - 0.91893853320467274178f;
  }
  // ---- outputs --------------------------------------------------------------
  const bool keep = alive && live;
  if (a.full && !a.script_self) {
    f64x4 v = {alive ? (double)act[0] : 0.0, alive ? (double)act[1] : 0.0, alive ? (double)act[2] : 0.0,
               alive ? (double)act[3] : 0.0};
    *(f64x4 *)(a.full + ((long long)e_o * a.A + a.own0 + i_o) * 4) = v;
  }
  if (a.act_out)
    *(f32x4 *)(a.act_out + (long long)e_o * a.act_env_stride + 4 * i_o) =
        keep ? f32x4{act[0], act[1], act[2], act[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
  if (a.logp_out)
    *(f32x4 *)(a.logp_out + (long long)e_o * a.act_env_stride + 4 * i_o) =
        keep ? f32x4{lp[0], lp[1], lp[2], lp[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
}

// ---------------------------------------------------------------------------
// After lnw_step (lnw_rollout_post): the rollout's bookkeeping of step t and
// the critic (network.py:154-172, ppo.py:598-605) on the observations the actor
// saw (the rollout buffer at step t), on the matrix cores like the actor's MLP
// (v_mfma_f32_16x16x4_f32, transposed layers Y^T = W X^T, k order 16 q + 4 g +
// v; see mfma_layer). One workgroup = 64 envs (4 row tiles) x n waves:
//   fc1 (n D -> 32): wave w takes ship w's D inputs (zero-padded to DQ
//        quads), partial sums of all 32 outputs for the 64 envs, added up
//        through LDS by every wave (+ bias, tanh);
//   fc2 (32 -> 64) and fc3 (64 -> 64): the 16-output tiles dealt over the
//        waves, fc2's tiles exchanged through LDS in the MFMA operand layout;
//   fc4 (64 -> 1): each wave's fc3 tiles dotted with w4 in registers, summed
//        over lane groups (shuffles) and waves (LDS);
//   wave 0, lane = env: the value (0 after the episode ended), the rewards,
//   the running flag and the env's new live flag (done == 0 ends it, ppo.py:640).
// Packed critic (BatchedCritic.packed()): fc1 fragments per ship [n][2][DQ]
// [lane] float4, b1 [32], fc2 fragments [4][2][lane], b2 [64], fc3 fragments
// [4][4][lane], b3 [64], w4 [64], b4 (+ 3 zeros).
// ---------------------------------------------------------------------------
constexpr int CF1 = 32, CF2 = 64, CF3 = 64;

struct CriticOffsets { int w1, b1, w2, b2, w3, b3, w4, b4; };

__global__ __launch_bounds__(1024) void rollout_post_kernel(lnw_rollout_post_args a, CriticOffsets co, int dq) {
  const int lane = threadIdx.x & (WAVE - 1), g = lane >> 4, m = lane & 15;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int n = a.n, D = a.D;
  const long long e0 = (long long)blockIdx.x * WAVE;
  const long long e = e0 + lane;
  const bool valid = e < a.E;
  const bool crit = a.critic != nullptr;
  // dynamic LDS: fc1 partials [n][2 nt][4 rt][64] f32x4 | fc2 tiles [4][4 rt][64] f32x4 | fc4 dots [n][64]
  f32x4v *part = (f32x4v *)actor_lds;
  f32x4v *h2s = part + n * 8 * WAVE;
  float *dsum = (float *)(h2s + 16 * WAVE);
  if (crit) {
    const float *C = a.critic;
    // ---- fc1: ship w's inputs --------------------------------------------------
    f32x4v acc[4][2];
#pragma unroll
    for (int rt = 0; rt < 4; rt++) acc[rt][0] = acc[rt][1] = f32x4v{0.f, 0.f, 0.f, 0.f};
    const f32x4v *F1 = (const f32x4v *)(C + co.w1) + (size_t)w * 2 * dq * WAVE;
    // (uniform trip count; MFMAs unrolled inside; quad q + 1's rows and weights
    // are loaded before quad q's MFMAs, so one load latency per wave, not dq)
    auto load_q = [&](int q, f32x4v (&xb)[4], f32x4v &w0, f32x4v &w1) {
      const int k = 16 * q + 4 * g;
#pragma unroll
      for (int rt = 0; rt < 4; rt++) {
        const long long er = e0 + rt * 16 + m;
        xb[rt] = (k < D && er < a.E) ? *(const f32x4v *)(a.obs + er * a.obs_env_stride + (long long)w * D + k)
                                      : f32x4v{0.f, 0.f, 0.f, 0.f};
      }
      w0 = F1[(0 * dq + q) * WAVE + lane];
      w1 = F1[(1 * dq + q) * WAVE + lane];
    };
    f32x4v xb[4], w0, w1;
    load_q(0, xb, w0, w1);
    for (int q = 0; q < dq; q++) {
      f32x4v xn[4], n0, n1;
      if (q + 1 < dq) load_q(q + 1, xn, n0, n1);
#pragma unroll
      for (int v = 0; v < 4; v++)
#pragma unroll
        for (int rt = 0; rt < 4; rt++) {
          acc[rt][0] = mfma4(w0[v], xb[rt][v], acc[rt][0]);
          acc[rt][1] = mfma4(w1[v], xb[rt][v], acc[rt][1]);
        }
      if (q + 1 < dq) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++) xb[rt] = xn[rt];
        w0 = n0;
        w1 = n1;
      }
    }
  #pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) part[((w * 2 + nt) * 4 + rt) * WAVE + lane] = acc[rt][nt];
    __syncthreads();
    f32x4v h1[4][2];
    bias_init<2>(C + co.b1, h1, g);
    for (int v = 0; v < n; v++)
#pragma unroll
      for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) h1[rt][nt] += part[((v * 2 + nt) * 4 + rt) * WAVE + lane];
    tanh_all<2>(h1);
    // ---- fc2: tiles w, w + n, ... ------------------------------------------
    for (int nt = w; nt < 4; nt += n) {
      f32x4v t2[4][1];
      const f32x4v bv = *(const f32x4v *)(C + co.b2 + nt * 16 + 4 * g);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) t2[rt][0] = bv;
      mfma_layer<1, 2>((const f32x4v *)(C + co.w2) + nt * 2 * WAVE, h1, t2, lane);
    #pragma unroll
      for (int rt = 0; rt < 4; rt++) {
#pragma unroll
        for (int v = 0; v < 4; v++) t2[rt][0][v] = tanh_fast(t2[rt][0][v]);
        h2s[(nt * 4 + rt) * WAVE + lane] = t2[rt][0];
      }
    }
    __syncthreads();
    // ---- fc3 + fc4 partial dots ----------------------------------------------
    f32x4v h2[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
      for (int q = 0; q < 4; q++) h2[rt][q] = h2s[(q * 4 + rt) * WAVE + lane];
    float dot[4] = {0.f, 0.f, 0.f, 0.f};
    for (int nt = w; nt < 4; nt += n) {
      f32x4v t3[4][1];
      const f32x4v bv = *(const f32x4v *)(C + co.b3 + nt * 16 + 4 * g);
#pragma unroll
      for (int rt = 0; rt < 4; rt++) t3[rt][0] = bv;
      mfma_layer<1, 4>((const f32x4v *)(C + co.w3) + nt * 4 * WAVE, h2, t3, lane);
          const f32x4v w4 = *(const f32x4v *)(C + co.w4 + nt * 16 + 4 * g);
#pragma unroll
      for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int v = 0; v < 4; v++) dot[rt] = fmaf(w4[v], tanh_fast(t3[rt][0][v]), dot[rt]);
    }
    // lane groups g hold outputs 4 g .. 4 g + 3 of each tile: sum over g
#pragma unroll
    for (int rt = 0; rt < 4; rt++) {
      dot[rt] += __shfl_xor(dot[rt], 16);
      dot[rt] += __shfl_xor(dot[rt], 32);
    }
    if (g == 0) {
#pragma unroll
      for (int rt = 0; rt < 4; rt++) dsum[w * WAVE + rt * 16 + m] = dot[rt];
    }
    __syncthreads();
  }
  if (w != 0 || !valid) return;
  const bool L = !a.live || a.live[e] != 0;
  const bool masked = a.stop_at_done != 0;
  if (crit) {
    float s = 0.f;
    for (int q = 0; q < n; q++) s += dsum[q * WAVE + lane];
    const float v = a.critic[co.b4] + s;
    a.val[e * a.val_env_stride] = (masked && !L) ? 0.0f : v;
  }
  if (a.rew && a.rew_out) {
    for (int q = 0; q < a.n_rew; q++) {
      const double rv = a.rew_f64 ? ((const double *)a.rew)[e * a.n_rew + q]
                                  : (double)((const float *)a.rew)[e * a.n_rew + q];
      a.rew_out[e * a.rew_env_stride + q] = (masked && !L) ? 0.0 : rv;
    }
  }
  if (a.running) a.running[e * a.running_env_stride] = L ? 1 : 0;
  if (masked && a.live && a.done) a.live[e] = (L && a.done[e] != 0) ? 1 : 0;
}

}  // namespace

extern "C" {

int lnw_actor_features(const float *params_dev, int32_t obs_dim, const float *obs_dev, int64_t B,
                       int32_t bn_running, float *out_dev, void *stream) {
  if (!params_dev || !obs_dev || !out_dev || B < 0) return LNW_EINVAL;
  if (!obs_width_ok(obs_dim, false)) return LNW_EUNSUPPORTED;  // (per-value tail loads: any width)
  if (B == 0) return 0;
  const long long blocks = (B + CH_THREADS - 1) / CH_THREADS;  // one row per thread
  if (B >= (1ll << 31) - CH_THREADS) return LNW_EUNSUPPORTED;  // (32-bit rows)
  const int n_par = CONV_PARAMS + 2 * (obs_dim - WIN + 12);
  const size_t lds = (n_par + 45 * CH_THREADS) * sizeof(float);
  if (obs_dim - WIN + 12 <= 32)
    features_kernel<32><<<dim3((unsigned)blocks), dim3(CH_THREADS), lds, (hipStream_t)stream>>>(
        params_dev, obs_dim, obs_dev, (int)B, bn_running, out_dev);
  else
    features_kernel<MAX_IN><<<dim3((unsigned)blocks), dim3(CH_THREADS), lds, (hipStream_t)stream>>>(
        params_dev, obs_dim, obs_dev, (int)B, bn_running, out_dev);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

// Packed MLP part of lnw_policy_act's parameters (BatchedActor.packed_policy()),
// after the conv head block padded to a multiple of 4 floats: b1 [64], b2 [64],
// b3 [32], then the MFMA A-operand fragments of fc1 (n_in zero-padded to K1 =
// 32, or 64 when n_in > 32), fc2, fc3 and the heads (normal rows 0-3, log-std
// rows 4-7, zero rows to 16), each as float4 [n-tile][k-quad][lane] (see
// mfma_layer).
// (pop == NULL: lnw_policy_act's one set for every row)
static int policy_launch(const lnw_policy_args *args, const lnw_policy_pop *pop, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_policy_args &a = *args;
  if (!a.obs || !a.params || !a.alive || a.n <= 0 || a.E < 0 || a.A <= 0 || a.own0 < 0 || a.own0 + a.n > a.A)
    return LNW_EINVAL;
  if (!obs_width_ok(a.D, true)) return LNW_EUNSUPPORTED;
  if (a.forced && !a.forced_act) return LNW_EINVAL;
  if (a.script_self && (!a.script || a.forced)) return LNW_EINVAL;
  if (!a.forced && !a.script_self && a.T <= 0) return LNW_EINVAL;
  if (a.script && (!a.full || a.script_own0 < 0 || a.script_own0 + a.script_cnt > a.A)) return LNW_EINVAL;
  if ((a.kinds_f32_all_alive || a.f32_out) && !a.kinds) return LNW_EINVAL;
  if (a.obs_in_env_stride < 0 || (a.obs_in_env_stride && (a.obs_in_env_stride < (int64_t)a.n * a.D ||
                                                          (a.obs_in_env_stride & 3))))
    return LNW_EINVAL;
  // 16-B aligned rows for the vector copies and stores
  if (((uintptr_t)a.obs & 15) || (a.obs_out && (((uintptr_t)a.obs_out & 15) || (a.obs_env_stride & 3))) ||
      ((a.act_out || a.logp_out) && (a.act_env_stride & 3)) || (a.act_out && ((uintptr_t)a.act_out & 15)) ||
      (a.logp_out && ((uintptr_t)a.logp_out & 15)) || (a.full && ((uintptr_t)a.full & 31)) ||
      (a.script && ((uintptr_t)a.script & 31)))
    return LNW_EINVAL;
  const PolicyPack pk = policy_pack(a.D);
  if (pop && (pop->envs_per_member <= 0 || pop->member_stride < pk.floats || (pop->member_stride & 3) ||
              ((uintptr_t)a.params & 15)))
    return LNW_EINVAL;
  if (a.E == 0) return 0;
  PolicyPopArgs pa;  // (the plain kernels take its PolicyArgs part)
  pa.a = a;
  pa.n_in = pk.n_in;
  pa.off_b1 = pk.off_b1;
  pa.off_w1 = pk.off_w1;
  const long long rows = a.E * a.n;
  if (rows + PA_THREADS >= (1ll << 31)) return LNW_EUNSUPPORTED;  // (32-bit row indices)
  long long nblocks = (rows + PA_THREADS - 1) / PA_THREADS;
  if (pop) {  // members x blocks of one member (the last member may hold fewer envs)
    const long long G = pop->envs_per_member < a.E ? pop->envs_per_member : a.E;
    const long long members = (a.E + G - 1) / G;
    if (pop->member_stride >= (1ll << 31)) return LNW_EUNSUPPORTED;
    pa.member_rows = (int)(G * a.n);  // (<= rows: 32-bit)
    pa.member_stride = (int)pop->member_stride;
    pa.bpm = (pa.member_rows + PA_THREADS - 1) / PA_THREADS;
    nblocks = members * pa.bpm;
    if (nblocks >= (1ll << 31)) return LNW_EUNSUPPORTED;
  }
  const unsigned blocks = (unsigned)nblocks;
  const int npar4 = pk.off_b1;
  size_t lds = (size_t)(npar4 + (PA_THREADS / WAVE) * (pa.n_in <= 32 ? 45 : MAX_IN + 4) * WAVE) * sizeof(float);
  if (pa.n_in <= 32) lds += (size_t)mlp_bf16x8<32>() * 16;  // the MLP weights' LDS copy
  // One block per CU: head_and_mlp's schedule (every head, a barrier, every MLP)
  // keeps a head from running beside an MLP only within the block, so no other
  // block may share the CU. The block asks for more than half of the CU's LDS,
  // padded up should a future layout (a smaller tile, the weights out of LDS, a
  // smaller PA_THREADS) need less.
  static int cu_lds = 0;
  if (!cu_lds) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) != hipSuccess || v <= 0)
      v = 160 * 1024;
    cu_lds = v;
  }
  if (lds <= (size_t)cu_lds / 2) lds = (size_t)cu_lds / 2 + 16;
  const PolicyArgs &plain = pa;
  if (pop && pa.n_in <= 32)
    policy_act_kernel<32, true><<<blocks, PA_THREADS, lds, (hipStream_t)stream>>>(pa);
  else if (pop)
    policy_act_kernel<MAX_IN, true><<<blocks, PA_THREADS, lds, (hipStream_t)stream>>>(pa);
  else if (pa.n_in <= 32)
    policy_act_kernel<32, false><<<blocks, PA_THREADS, lds, (hipStream_t)stream>>>(plain);
  else
    policy_act_kernel<MAX_IN, false><<<blocks, PA_THREADS, lds, (hipStream_t)stream>>>(plain);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

int lnw_policy_act(const lnw_policy_args *args, void *stream) { return policy_launch(args, nullptr, stream); }

int lnw_policy_act_pop(const lnw_policy_args *args, const lnw_policy_pop *pop, void *stream) {
  if (!pop) return LNW_EINVAL;
  return policy_launch(args, pop, stream);
}

// Packed critic: see rollout_post_kernel (BatchedCritic.packed()).
int lnw_rollout_post(const lnw_rollout_post_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_rollout_post_args &a = *args;
  if (a.n <= 0 || a.n > 16 || a.E < 0) return LNW_EINVAL;
  if (a.critic && (!a.obs || !a.val || (a.D & 3) || ((uintptr_t)a.obs & 15) || (a.obs_env_stride & 3) ||
                   ((uintptr_t)a.critic & 15)))
    return LNW_EINVAL;
  if (a.rew_out && (!a.rew || a.n_rew <= 0)) return LNW_EINVAL;
  if (a.E == 0) return 0;
  const int dq = (a.D + 15) / 16;
  CriticOffsets co;
  int o = 0;
  co.w1 = o; o += a.n * 2 * dq * WAVE * 4;
  co.b1 = o; o += CF1;
  co.w2 = o; o += 4 * 2 * WAVE * 4;
  co.b2 = o; o += CF2;
  co.w3 = o; o += 4 * 4 * WAVE * 4;
  co.b3 = o; o += CF3;
  co.w4 = o; o += CF3;
  co.b4 = o;
  const unsigned blocks = (unsigned)((a.E + WAVE - 1) / WAVE);
  const size_t lds = a.critic ? (size_t)(a.n * 8 * WAVE + 16 * WAVE) * 16 + (size_t)a.n * WAVE * 4 : 0;
  rollout_post_kernel<<<blocks, WAVE * a.n, lds, (hipStream_t)stream>>>(a, co, dq);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
