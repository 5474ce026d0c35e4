// MAPPO learner step (lnw_ppo_grad, lnw_ppo_clip_adam): one minibatch update of
// the reference's PPO.learn (ppo.py:321-390) for the blue side on B rows — the
// actor evaluated row by row with each row's own BatchNorm statistics
// (ppo.py:673-693: train() and one state per call), the critic on the rows'
// global states, PPO.gae over the minibatch rows as the sequence and
// popart_normalize, the clipped surrogate with the entropy bonus, the clipped
// RMSE value loss, both gradients, the actor's running statistics after the B
// sequential updates, the global-norm clip and Adam.
//
// A chain of plain launches on the caller's stream, no synchronisation across
// workgroups inside a kernel and no atomics: every cross-workgroup sum is
// per-workgroup partials in the workspace ("slabs"), summed in a fixed order
// with double accumulators by the next launch, so results are bitwise equal
// from run to run and between eager launches and a graph replay.
//
//   features    per row: conv head with the row's statistics, LayerNorm -> the
//               fc1 input, the normalised values and the row's statistics
//   linear_fwd  fc1 / fc2 / fc3 / heads of the actor, fc1 .. fc4 of the critic
//               (its input read in place: the group of row_index / n)
//   advantage   one workgroup: the GAE scan in blocks with carries, the four
//               popart moments, the advantage, the critic loss and dL/dv, double
//   actorloss   per row: log-probability, entropy, ratio, the surrogate's
//               branch, the head gradients; loss partials
//   linear_wgrad / linear_bwd per layer, last to first: dW = dY^T X over chunks
//               of rows into the slab, dX = dY W times the tanh derivative
//   lnbwd, lnwgrad   LayerNorm backward
//   conv2grad   convhead, pool 2, BatchNorm 2 (instance statistics: the batch
//               means of the DDQN pass are the row's own), conv2, pool 1
//   conv1grad   BatchNorm 1 and conv1
//   running     the running statistics after the B updates in minibatch order
//
// The dense layers run on v_mfma_f32_16x16x4_f32: exact f32 products, f32
// accumulation in k order, i.e. the accuracy of an fmaf chain, which the
// gradient bound (8 x the float32 reference's own error) needs with no term to
// drop; the three-term bf16 split of lnw_actor.hip has 6 MFMAs per 32 k against
// 8 here but sums six rounded partial products, and these layers are bound by
// their loads (one 16 x 16 tile per wave, operands straight from L2), not by
// the matrix cores.
// Max pool sends the gradient to the first maximum of the window in row-major
// order (strict >), as torch's max_pool2d does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "lnw.h"
#include "lnw_device.h"

namespace {

using namespace lnw;

#include "lnw_convhead.inc"
#include "lnw_learn.inc"
#include "lnw_adam.inc"

constexpr int LDW = 64;  // row stride of the actor's fc1 input (n_in <= 64, zero padded)
// the features pass's LDS copy of the parameters: the conv head and LayerNorm's w, b [n_in], padded to 8 floats
constexpr int FEAT_LDS = (CONV_PARAMS + 2 * MAX_IN + 7) & ~7;
static_assert(LDW == MAX_IN && FEAT_LDS == 712, "the kernels' LDS sizes are pinned by the resource tests");
constexpr float LN_EPS = 1e-5f;
constexpr int ADV_THREADS = 1024;
constexpr int RUN_TAIL = 2048;  // 0.9^2048 of any float32 is below the smallest float32

// the actor's layers
constexpr int FC1 = 64, FC2 = 64, FC3 = 32, NHEAD = 8;
// the critic's
constexpr int CF1 = 32, CF2 = 64, CF3 = 64;

// slab stride of the two conv passes (their layouts: lnw_learn.inc, S4 with its tail)
constexpr int CONV_SLABW = (S4_N_TAIL + 3) & ~3;

// per-row column fields [field][rows_pad] (floats and ints)
constexpr int WS_V = 0, WS_DV = 1, WS_ADV = 2, WS_LNINV = 3, WS_DH = 4, WS_GY1 = 16, WS_POS1 = 61, WS_T = 66,
              WS_ST = 76, WS_FIELDS = 102;

struct ActorOff { int lnw, lnb, w1, b1, w2, b2, w3, b3, hw, logstd, total; };
struct CriticOff { int w1, b1, w2, b2, w3, b3, w4, b4, total; };

ActorOff actor_off(int n_in) {
  ActorOff o;
  o.lnw = CONV_PARAMS;
  o.lnb = o.lnw + n_in;
  o.w1 = o.lnb + n_in;
  o.b1 = o.w1 + FC1 * n_in;
  o.w2 = o.b1 + FC1;
  o.b2 = o.w2 + FC2 * FC1;
  o.w3 = o.b2 + FC2;
  o.b3 = o.w3 + FC3 * FC2;
  o.hw = o.b3 + FC3;
  o.logstd = o.hw + NHEAD * FC3;
  o.total = o.logstd + 1;
  return o;
}

CriticOff critic_off(int k1) {
  CriticOff o;
  o.w1 = 0;
  o.b1 = CF1 * k1;
  o.w2 = o.b1 + CF1;
  o.b2 = o.w2 + CF2 * CF1;
  o.w3 = o.b2 + CF2;
  o.b3 = o.w3 + CF3 * CF2;
  o.w4 = o.b3 + CF3;
  o.b4 = o.w4 + CF3;
  o.total = o.b4 + 1;
  return o;
}

struct Ws {
  double *dslab;  // [nblk]
  double *retd;   // [rows_pad] GAE returns
  float *fslab;
  float *x0, *xh, *h1, *h2, *h3, *z;  // actor, row-major [rows_pad][64 | 64 | 64 | 64 | 32 | 8]
  float *c1, *c2, *c3;               // critic [rows_pad][32 | 64 | 64]
  float *col;                        // [WS_FIELDS][rows_pad]
  long long rows_pad;
  int nblk, nchunks, chunk_rows, slabw;
};

extern __shared__ float pl_lds[];

// ---- per-row pieces (the shared ones: lnw_learn.inc) ---------------------------------
// a channel's own statistics (mean, biased variance), summed in double: a
// constant map (a dead ship's zero row: every conv1 output is the bias) then has
// mean = the value and variance 0 exactly, as in exact arithmetic. With float
// sums the mean of 49 equal values is a few ulp off, 1 / sqrt(0 + eps) = 316
// scales that to 1e-5, and where conv2's input is constant as well (BatchNorm
// biases at their initial 0) the second BatchNorm scales it by 316 again:
// log-probabilities of such rows came out 6e-3 off the float64 oracle.
template <int N>
__device__ __forceinline__ void inst_stats(const float (&v)[N], float &mean, float &var) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) s += (double)v[i];
  mean = (float)(s / (double)N);
  double q = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const double d = (double)v[i] - (double)mean;
    q += d * d;
  }
  var = (float)(q / (double)N);
}

// conv1 -> BN (the row's statistics) -> ReLU -> 2x2 pool: the pooled maps into
// pc; st: null, or the row's statistics out (mean at [c * sstride], unbiased
// variance at [(13 + c) * sstride])
__device__ __forceinline__ void fwd_p1(const float *P, const float (&win)[WIN], float *pc, float *st,
                                       long long sstride) {
#pragma clang fp contract(fast)
#pragma unroll 1
  for (int c = 0; c < 5; c++) {
    float v[49];
    conv1_ch(P, win, c, v);
    float m, var;
    inst_stats<49>(v, m, var);
    if (st) {
      st[c * sstride] = m;
      st[(13 + c) * sstride] = var * (49.0f / 48.0f);
    }
    bn_relu_pool1(v, c, m, 1.0f / sqrtf(var + BN_EPS), P[B1W + c], P[B1B + c], pc);
  }
}

__device__ __forceinline__ const float *obs_row(const lnw_ppolearn_args &a, long long r) {
  const long long ri = a.row_index ? a.row_index[r] : r;
  return a.obs + ri * a.D;
}

// ---- features: conv head, LayerNorm, the row's statistics ---------------------------
__global__ __launch_bounds__(LEARN_THREADS) void pl_features_kernel(lnw_ppolearn_args a, Ws w, int n_in) {
  float *P = pl_lds;  // [FEAT_LDS]: CONV_PARAMS + 2 n_in
  float *pc = pl_lds + FEAT_LDS + threadIdx.x;
  for (int i = threadIdx.x; i < CONV_PARAMS + 2 * n_in; i += LEARN_THREADS) P[i] = a.actor_params[i];
  __syncthreads();
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  if (r >= a.rows) return;
  const float *row = obs_row(a, r);
  const long long rp = w.rows_pad;
  float *st = w.col + WS_ST * rp + r;
  float h[12];
  {
#pragma clang fp contract(fast)
    {
      float win[WIN];
      load_win(row, win);
      fwd_p1(P, win, pc, st, rp);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) h[k] = P[HB + k];
#pragma unroll 1
    for (int c0 = 0; c0 < 8; c0 += 4) {
      float v2[4][9];
      conv2_raw(P, pc, LEARN_THREADS, c0, v2);
#pragma unroll
      for (int co = 0; co < 4; co++) {
        const int c = c0 + co;
        float m, var;
        inst_stats<9>(v2[co], m, var);
        st[(5 + c) * rp] = m;
        st[(18 + c) * rp] = var * (9.0f / 8.0f);
        const float inv = 1.0f / sqrtf(var + BN_EPS), g = P[B2W + c], b = P[B2B + c];
        const float y0 = fmaxf((v2[co][0] - m) * inv * g + b, 0.f), y1 = fmaxf((v2[co][1] - m) * inv * g + b, 0.f);
        const float y3 = fmaxf((v2[co][3] - m) * inv * g + b, 0.f), y4 = fmaxf((v2[co][4] - m) * inv * g + b, 0.f);
        const float f = fmaxf(fmaxf(y0, y1), fmaxf(y3, y4));
#pragma unroll
        for (int k = 0; k < 12; k++) h[k] += P[HW + k * 8 + c] * f;
      }
    }
  }
  // LayerNorm over [h, row[49 ..]] (biased variance)
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 12; k++) s += h[k];
#pragma unroll 1
  for (int k = 12; k < n_in; k++) s += row[37 + k];
  const float mean = s / (float)n_in;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < 12; k++) q += (h[k] - mean) * (h[k] - mean);
#pragma unroll 1
  for (int k = 12; k < n_in; k++) q += (row[37 + k] - mean) * (row[37 + k] - mean);
  const float inv = 1.0f / sqrtf(q / (float)n_in + LN_EPS);
  w.col[WS_LNINV * rp + r] = inv;
  const float *lw = P + CONV_PARAMS, *lb = lw + n_in;
  float *x0 = w.x0 + r * LDW, *xh = w.xh + r * LDW;
#pragma unroll
  for (int k = 0; k < 12; k++) {
    const float t = (h[k] - mean) * inv;
    xh[k] = t;
    x0[k] = t * lw[k] + lb[k];
  }
#pragma unroll 1
  for (int k = 12; k < LDW; k++) {
    const float t = k < n_in ? (row[37 + k] - mean) * inv : 0.f;
    xh[k] = t;
    x0[k] = k < n_in ? t * lw[k] + lb[k] : 0.f;
  }
}

// ---- dense layers on v_mfma_f32_16x16x4_f32 ---------------------------------------------
// D = A B with lane l holding A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]
// and D[i = 4 (l >> 4) + v][j = l & 15], v = 0..3; one 16 x 16 tile per wave.
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Four accumulators per tile, k dealt round-robin in steps of 4 and summed in
// pairs at the end: the dependent MFMAs of one accumulator are 40 cycles apart
// and four keep the pipe at its issue rate; and a sum over 1200 inputs (the
// critic's fc1 at 12 ships) carries half the rounding of one sequential chain.
__device__ __forceinline__ f32x4 sum4(const f32x4 (&p)[4]) { return (p[0] + p[1]) + (p[2] + p[3]); }

struct Lin {
  const float *X;        // [rows][ldx] inputs (gather: row (idx ? idx[r] : r) / div)
  long long ldx;
  const int64_t *idx;
  int div;
  const float *W;        // [N][K]
  const float *b;        // [N] or null
  int K, N;
  float *Y;              // [rows][ldy] outputs / their gradients
  int ldy;
  long long rows;
  int act;               // tanh
};

__device__ __forceinline__ const float *lin_row(const Lin &L, long long r) {
  if (!L.idx && L.div == 1) return L.X + r * L.ldx;
  const long long ri = L.idx ? L.idx[r] : r;
  return L.X + (ri / L.div) * L.ldx;
}

// Y = act(X W^T + b): i = output, j = row
__global__ __launch_bounds__(256) void pl_linear_fwd_kernel(Lin L) {
  const int lane = threadIdx.x & (WAVE - 1), g = lane >> 4, m = lane & 15;
  const long long rt = (long long)blockIdx.x * 4 + threadIdx.x / WAVE;
  if (rt * 16 >= L.rows) return;  // (wave-uniform)
  const int nt = blockIdx.y;
  const long long r = rt * 16 + m;
  const int o = nt * 16 + m;
  const bool rok = r < L.rows, ook = o < L.N;
  const float *xrow = lin_row(L, rok ? r : L.rows - 1);
  const float *wrow = L.W + (long long)(ook ? o : 0) * L.K;
  f32x4 part[4];
#pragma unroll
  for (int u = 0; u < 4; u++) part[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int ob = nt * 16 + 4 * g + v;
    part[0][v] = (L.b && ob < L.N) ? L.b[ob] : 0.f;
  }
  for (int k0 = 0; k0 < L.K; k0 += 16) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int k = k0 + 4 * u + g;
      const bool kok = k < L.K;
      const float av = (ook && kok) ? wrow[k] : 0.f;
      const float bv = (rok && kok) ? xrow[k] : 0.f;
      part[u] = mfma4(av, bv, part[u]);
    }
  }
  const f32x4 acc = sum4(part);
  if (!rok) return;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int ob = nt * 16 + 4 * g + v;
    if (ob < L.N) L.Y[r * L.ldy + ob] = L.act ? tanhf(acc[v]) : acc[v];
  }
}

// dX = (dY W) (1 - H^2), H the layer's input held where dX goes (in place);
// i = input k, j = row; columns [0, kw) are written (zeros past K)
__global__ __launch_bounds__(256) void pl_linear_bwd_kernel(Lin L, float *dX, int ldd, int kw, int act) {
  const int lane = threadIdx.x & (WAVE - 1), g = lane >> 4, m = lane & 15;
  const long long rt = (long long)blockIdx.x * 4 + threadIdx.x / WAVE;
  if (rt * 16 >= L.rows) return;  // (wave-uniform)
  const int kt = blockIdx.y;
  const long long r = rt * 16 + m;
  const int ka = kt * 16 + m;
  const bool rok = r < L.rows, kok = ka < L.K;
  const float *yrow = L.Y + (rok ? r : 0) * L.ldy;
  const float *wcol = L.W + (kok ? ka : 0);
  f32x4 part[4];
#pragma unroll
  for (int u = 0; u < 4; u++) part[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int o0 = 0; o0 < L.N; o0 += 16) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int o = o0 + 4 * u + g;
      const bool ook = o < L.N;
      const float av = (kok && ook) ? wcol[(long long)o * L.K] : 0.f;
      const float bv = (rok && ook) ? yrow[o] : 0.f;
      part[u] = mfma4(av, bv, part[u]);
    }
  }
  const f32x4 acc = sum4(part);
  if (!rok) return;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int kb = kt * 16 + 4 * g + v;
    if (kb < kw) {
      float d = acc[v];
      if (act) {
        const float hv = dX[r * ldd + kb];
        d = d * (1.0f - hv * hv);
      }
      dX[r * ldd + kb] = d;
    }
  }
}

// slab[chunk][o (K + bias) + k] = sum over the chunk's rows of dY[r][o] X[r][k]
// (k = K: the bias, X = 1); i = output o, j = input k, summed over rows
__global__ __launch_bounds__(256) void pl_linear_wgrad_kernel(Lin L, float *slab, int slabw, int chunk_rows) {
  const int lane = threadIdx.x & (WAVE - 1), g = lane >> 4, m = lane & 15;
  const int kb = L.K + (L.b ? 1 : 0);
  const int ktiles = (kb + 15) / 16, otiles = (L.N + 15) / 16;
  const int t = blockIdx.y * 4 + threadIdx.x / WAVE;
  if (t >= ktiles * otiles) return;  // (wave-uniform)
  const int ot = t / ktiles, kt = t - ot * ktiles;
  const int o = ot * 16 + m, k = kt * 16 + m;
  const bool ook = o < L.N, kin = k < L.K, kone = L.b && k == L.K;
  const long long r0 = (long long)blockIdx.x * chunk_rows;
  long long r1 = r0 + chunk_rows;
  r1 = r1 < L.rows ? r1 : L.rows;
  f32x4 part[4];
#pragma unroll
  for (int u = 0; u < 4; u++) part[u] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long long rr = r0; rr < r1; rr += 16) {
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const long long r = rr + 4 * u + g;
      const bool rok = r < r1;
      const float av = (rok && ook) ? L.Y[r * L.ldy + o] : 0.f;
      float bv = 0.f;
      if (rok && kin) bv = lin_row(L, r)[k];
      if (rok && kone) bv = 1.f;
      part[u] = mfma4(av, bv, part[u]);
    }
  }
  const f32x4 acc = sum4(part);
  float *s = slab + (long long)blockIdx.x * slabw;
#pragma unroll
  for (int v = 0; v < 4; v++) {
    const int ob = ot * 16 + 4 * g + v;
    if (ob < L.N && k < kb) s[ob * kb + k] = acc[v];
  }
}

// the slabs summed per destination (fixed order, double accumulators): one wave
// per destination, lane l takes slabs l, l + 64, ...; destination i = o kb + k
// goes to grad[off_w + o K + k], or grad[off_b + o] for k = K
__global__ __launch_bounds__(256) void pl_reduce_lin_kernel(const float *slab, int slabw, int nslab, int count, int kb,
                                                            int K, float *grad, int off_w, int off_b) {
  const int i = blockIdx.x * 4 + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  if (i >= count) return;  // (wave-uniform)
  double s = 0.0;
  for (int b = lane; b < nslab; b += WAVE) s += (double)slab[(long long)b * slabw + i];
  s = wave_sum_d(s);
  if (lane != 0) return;
  const int o = i / kb, k = i - o * kb;
  grad[k < K ? off_w + o * K + k : off_b + o] = (float)s;
}

// ---- advantage, critic loss (one workgroup) ------------------------------------------------
__device__ __forceinline__ double block_sum_d(double v, double *red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = ADV_THREADS / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(ADV_THREADS) void pl_advantage_kernel(lnw_ppolearn_args a, Ws w, double gamma,
                                                                   double lambda) {
  double *red = (double *)pl_lds;  // [1024]
  double *G = red + ADV_THREADS;   // [1024] a block's scan from a zero carry, then its carry in
  const int t = threadIdx.x;
  const long long B = a.rows;
  const long long Lb = (B + ADV_THREADS - 1) / ADV_THREADS;
  long long lo = (long long)t * Lb, hi = lo + Lb;
  lo = lo < B ? lo : B;
  hi = hi < B ? hi : B;
  const float *V = w.col + WS_V * w.rows_pad;
  const double c = gamma * lambda;
  // GAE (ppo.py:695-714) over the rows as the sequence: g_i = delta_i + c g_{i+1}
  double g = 0.0;
  for (long long i = hi - 1; i >= lo; i--) {
    const double delta = (double)a.rtg[i] + (i < B - 1 ? gamma * (double)V[i + 1] : 0.0) - (double)V[i];
    g = delta + c * g;
  }
  G[t] = g;
  __syncthreads();
  if (t == 0) {
    const double cl = pow(c, (double)Lb);
    double carry = 0.0;
    for (int tt = ADV_THREADS - 1; tt >= 0; tt--) {
      long long l0 = (long long)tt * Lb, l1 = l0 + Lb;
      l0 = l0 < B ? l0 : B;
      l1 = l1 < B ? l1 : B;
      const double mine = G[tt];
      G[tt] = carry;
      const long long len = l1 - l0;
      carry = mine + (len == Lb ? cl : pow(c, (double)len)) * carry;
    }
  }
  __syncthreads();
  g = G[t];
  double s_ret = 0.0, s_rtg = 0.0;
  for (long long i = hi - 1; i >= lo; i--) {
    const double delta = (double)a.rtg[i] + (i < B - 1 ? gamma * (double)V[i + 1] : 0.0) - (double)V[i];
    g = delta + c * g;
    const double ret = g + (double)V[i];
    w.retd[i] = ret;
    s_ret += ret;
    s_rtg += (double)a.rtg[i];
  }
  // popart_normalize (ppo.py:716-729), unbiased std: 0 / 0 and B = 1 give NaN
  const double n = (double)B;
  const double m_ret = block_sum_d(s_ret, red) / n;
  const double m_rtg = block_sum_d(s_rtg, red) / n;
  double q_ret = 0.0, q_rtg = 0.0;
  for (long long i = t; i < B; i += ADV_THREADS) {
    const double d0 = w.retd[i] - m_ret, d1 = (double)a.rtg[i] - m_rtg;
    q_ret += d0 * d0;
    q_rtg += d1 * d1;
  }
  const double sd_ret = sqrt(block_sum_d(q_ret, red) / (n - 1.0));
  const double sd_rtg = sqrt(block_sum_d(q_rtg, red) / (n - 1.0));
  float *adv = w.col + WS_ADV * w.rows_pad;
  for (long long i = t; i < B; i += ADV_THREADS) {
    const float av = (float)((w.retd[i] - m_ret) / sd_ret * sd_rtg + m_rtg);
    adv[i] = av;
    if (a.advantage) a.advantage[i] = av;
    if (a.values) a.values[i] = V[i];
  }
  // critic loss (ppo.py:362): sqrt(mean(max((v - r)^2, (clamp(v, vo -+ eps) - r)^2)))
  double s_l = 0.0;
  for (long long i = t; i < B; i += ADV_THREADS) {
    const float v = V[i], r = a.rtg[i], vo = a.old_values[i];
    const float vc = fminf(fmaxf(v, vo - a.eps_clip), vo + a.eps_clip);
    const float t1 = (v - r) * (v - r), t2 = (vc - r) * (vc - r);
    s_l += (double)(t1 > t2 ? t1 : t2);
  }
  const double loss = sqrt(block_sum_d(s_l, red) / n);
  if (t == 0) a.critic_loss[0] = (float)loss;
  // dL/dv: max's gradient goes to the larger term, evenly at a tie (every
  // in-range row: both halves arrive); clamp passes it inside and on its bounds
  float *dv = w.col + WS_DV * w.rows_pad;
  const double f = 1.0 / (2.0 * n * loss);
  for (long long i = t; i < B; i += ADV_THREADS) {
    const float v = V[i], r = a.rtg[i], vo = a.old_values[i];
    const float lo_ = vo - a.eps_clip, hi_ = vo + a.eps_clip;
    const float vc = fminf(fmaxf(v, lo_), hi_);
    const float t1 = (v - r) * (v - r), t2 = (vc - r) * (vc - r);
    const bool inr = v >= lo_ && v <= hi_;
    const double d = 2.0 * ((double)v - (double)r);
    dv[i] = (float)((inr || t1 > t2) ? d * f : (t1 == t2 ? 0.5 * d * f : 0.0));
  }
}

// ---- actor loss and the head gradients, per row ------------------------------------------------
__global__ __launch_bounds__(LEARN_THREADS) void pl_actorloss_kernel(lnw_ppolearn_args a, Ws w) {
  double *dsl = (double *)pl_lds;  // [LEARN_WAVES]
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
  const float adv = w.col[WS_ADV * w.rows_pad + rc];
  const float lo = 1.0f - a.eps_clip, hi = 1.0f + a.eps_clip;
  const float c = -1.0f / (4.0f * (float)a.rows);
  float *z = w.z + rc * NHEAD;
  const f32x4 zm = *(const f32x4 *)z, zl = *(const f32x4 *)(z + 4);
  const f32x4 act = *(const f32x4 *)(a.actions + rc * 4), old = *(const f32x4 *)(a.old_log_probs + rc * 4);
  f32x4 dm, dl, lpv, env;
  double part = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    // Normal(mean = tanh, std = exp).log_prob / entropy (torch.distributions)
    const float mu = tanhf(zm[j]), sd = expf(zl[j]);
    const float ls = logf(sd), var = sd * sd;
    const float d = act[j] - mu;
    const float lp = -(d * d) / (2.0f * var) - ls - 0.91893853320467274178f;
    const float en = 1.41893853320467274178f + ls;
    const float ratio = expf(lp - old[j]);
    const bool inr = ratio >= lo && ratio <= hi;
    const float s1 = adv * ratio, s2 = fminf(fmaxf(ratio, lo), hi) * adv;
    const float obj = s1 <= s2 ? s1 : s2;
    // min's gradient: to the smaller term, evenly at a tie (every in-range
    // element: both halves arrive); the clamped term passes none out of range
    const float gr = inr ? adv : (s1 > s2 ? 0.f : (s1 == s2 ? 0.5f * adv : adv));
    const float dlp = c * gr * ratio;
    dm[j] = dlp * (d / var) * (1.0f - mu * mu);
    dl[j] = dlp * ((d * d) / var - 1.0f) + c * a.entropy_coef;
    lpv[j] = lp;
    env[j] = en;
    part += (double)obj + (double)a.entropy_coef * (double)en;
  }
  if (valid) {
    *(f32x4 *)z = dm;
    *(f32x4 *)(z + 4) = dl;
    if (a.new_log_probs) *(f32x4 *)(a.new_log_probs + r * 4) = lpv;
    if (a.entropies) *(f32x4 *)(a.entropies + r * 4) = env;
  }
  part = wave_sum_d(valid ? part : 0.0);
  if ((threadIdx.x & (WAVE - 1)) == 0) dsl[threadIdx.x / WAVE] = part;
  __syncthreads();
  if (threadIdx.x == 0) w.dslab[blockIdx.x] = dsl[0] + dsl[1];
}

__global__ __launch_bounds__(WAVE) void pl_actorloss_sum_kernel(lnw_ppolearn_args a, Ws w) {
  double s = 0.0;
  for (int b = threadIdx.x; b < w.nblk; b += WAVE) s += w.dslab[b];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) a.actor_loss[0] = (float)(-(s / (4.0 * (double)a.rows)));
}

// ---- LayerNorm backward ---------------------------------------------------------------------
// per row: the gradient of the head's 12 outputs (the rest of the row is data)
__global__ __launch_bounds__(LEARN_THREADS) void pl_lnbwd_kernel(lnw_ppolearn_args a, Ws w, int n_in) {
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  if (r >= a.rows) return;
  const float *lw = a.actor_params + CONV_PARAMS;
  const float *dx = w.x0 + r * LDW, *xh = w.xh + r * LDW;
  float sg = 0.f, sgx = 0.f;
#pragma unroll 4
  for (int k = 0; k < n_in; k++) {
    const float gk = dx[k] * lw[k];
    sg += gk;
    sgx += gk * xh[k];
  }
  const float inv = w.col[WS_LNINV * w.rows_pad + r];
  const float mg = sg / (float)n_in, mgx = sgx / (float)n_in;
#pragma unroll
  for (int k = 0; k < 12; k++) w.col[(WS_DH + k) * w.rows_pad + r] = inv * ((dx[k] * lw[k] - mg) - xh[k] * mgx);
}

// the LayerNorm affine's gradients: thread k sums a chunk of rows in order
__global__ __launch_bounds__(WAVE) void pl_lnwgrad_kernel(lnw_ppolearn_args a, Ws w, int n_in) {
  const int k = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * w.chunk_rows;
  long long r1 = r0 + w.chunk_rows;
  r1 = r1 < a.rows ? r1 : a.rows;
  float sw = 0.f, sb = 0.f;
  for (long long r = r0; r < r1; r++) {
    const float gk = w.x0[r * LDW + k];
    sw += gk * w.xh[r * LDW + k];
    sb += gk;
  }
  float *s = w.fslab + (long long)blockIdx.x * w.slabw;
  s[k] = sw;
  s[LDW + k] = sb;
}

// ---- conv2 pass: convhead, pool 2, BN2, conv2, pool 1 ------------------------------------------
__global__ __launch_bounds__(LEARN_THREADS) void pl_conv2grad_kernel(lnw_ppolearn_args a, Ws w) {
  float *P = pl_lds;  // [CONV_LDS]
  float *parkA = P + CONV_LDS, *parkB = parkA + PARK;
  float *wsl = parkB + PARK;  // [LEARN_WAVES][S4_N_TAIL]
  for (int i = threadIdx.x; i < CONV_PARAMS; i += LEARN_THREADS) P[i] = a.actor_params[i];
  __syncthreads();
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
  const float vf = valid ? 1.f : 0.f;
  float *pA = parkA + threadIdx.x, *pB = parkB + threadIdx.x;
  const long long rp = w.rows_pad;
  float win[WIN];
  load_win(obs_row(a, rc), win);
  fwd_p1(P, win, pA, nullptr, 0);
#pragma unroll
  for (int k = 0; k < 45; k++) pB[k * LEARN_THREADS] = 0.f;
  float dh[12];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    dh[k] = valid ? w.col[(WS_DH + k) * rp + rc] : 0.f;
    accum(wsl, S4_N_TAIL, S4_HB + k, dh[k]);
  }
  {
#pragma clang fp contract(fast)
#pragma unroll 1
    for (int c0 = 0; c0 < 8; c0 += 4) {
      float dz[4][9];
      conv2_raw(P, pA, LEARN_THREADS, c0, dz);
      // BN2 backward with the row's own statistics: dz = g inv (dy - mean(dy) - xh mean(dy xh)),
      // dy the pooled output's gradient at the pool's position
#pragma unroll
      for (int co = 0; co < 4; co++) {
        const int c = c0 + co;
        float m, var;
        inst_stats<9>(dz[co], m, var);
        const float inv = 1.0f / sqrtf(var + BN_EPS), g = P[B2W + c], b = P[B2B + c];
        const float h0 = (dz[co][0] - m) * inv, h1 = (dz[co][1] - m) * inv;
        const float h3 = (dz[co][3] - m) * inv, h4 = (dz[co][4] - m) * inv;
        int sel;
        const float f = first_max4(fmaxf(h0 * g + b, 0.f), fmaxf(h1 * g + b, 0.f), fmaxf(h3 * g + b, 0.f),
                                   fmaxf(h4 * g + b, 0.f), sel);
        const float xs = sel == 0 ? h0 : sel == 1 ? h1 : sel == 2 ? h3 : h4;
        const int pos = sel < 2 ? sel : sel + 1;
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < 12; k++) {
          d += dh[k] * P[HW + k * 8 + c];
          accum(wsl, S4_N_TAIL, S4_HW + k * 8 + c, dh[k] * f);
        }
        const float gy = f > 0.f ? d : 0.f;
        accum(wsl, S4_N_TAIL, S4_B2W + c, gy * xs);
        accum(wsl, S4_N_TAIL, S4_B2B + c, gy);
        // (the two means and their subtraction in double: with the row's own
        // statistics 1 / sqrt(var + eps) reaches 316 on a constant map, and the
        // rounding of mean(dy) itself, the same in all 9 terms, would add up
        // in conv2's bias gradient, which is zero but for rounding)
        const float gi = g * inv * vf;
        const double m0 = (double)gy / 9.0, m1 = (double)gy * (double)xs / 9.0;
        double sb = 0.0;
#pragma unroll
        for (int q = 0; q < 9; q++) {
          const float xh = (dz[co][q] - m) * inv;
          const float dy = q == pos ? gy : 0.f;
          dz[co][q] = gi * (float)(((double)dy - m0) - (double)xh * m1);
          sb += (double)dz[co][q];
        }
        accum(wsl, S4_N_TAIL, S4_C2B + c, (float)sb);
      }
      conv2_bwd(P, pA, pB, c0, dz, wsl, S4_N_TAIL);
    }
  }
  // through pool 1 and the ReLU: conv1 again, channel by channel
  {
#pragma clang fp contract(fast)
#pragma unroll 1
    for (int c = 0; c < 5; c++) {
      float v[49];
      conv1_ch(P, win, c, v);
      float m, var;
      inst_stats<49>(v, m, var);
      const float inv = 1.0f / sqrtf(var + BN_EPS);
#pragma unroll
      for (int i = 0; i < 49; i++) v[i] = (v[i] - m) * inv;
      float t1, t2;
      unsigned pos1;
      pool1_bwd(v, P[B1W + c], P[B1B + c], pB + c * 9 * LEARN_THREADS, valid,
                w.col + (WS_GY1 + c * 9) * rp + r, rp, pos1, t1, t2);
      if (valid) {
        ((int *)w.col)[(WS_POS1 + c) * rp + r] = (int)pos1;
        // BN1's backward sums over the row's own 49 values
        w.col[(WS_T + c) * rp + r] = t1;
        w.col[(WS_T + 5 + c) * rp + r] = t2;
      }
      accum(wsl, S4_N_TAIL, S4_B1W + c, t2);
      accum(wsl, S4_N_TAIL, S4_B1B + c, t1);
    }
  }
  flush(wsl, S4_N_TAIL, w.fslab + (long long)blockIdx.x * CONV_SLABW);
}

// ---- conv1 pass: BN1 backward, conv1 gradients ---------------------------------------------
__global__ __launch_bounds__(LEARN_THREADS) void pl_conv1grad_kernel(lnw_ppolearn_args a, Ws w) {
  float *P = pl_lds;           // [CONV_LDS]
  float *wsl = P + CONV_LDS;   // [LEARN_WAVES][S5_N]
  for (int i = threadIdx.x; i < CONV_PARAMS; i += LEARN_THREADS) P[i] = a.actor_params[i];
  __syncthreads();
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
  const float vf = valid ? 1.f : 0.f;
  const float *fr = w.col;
  const int *ir = (const int *)w.col;
  const long long rp = w.rows_pad;
  float win[WIN];
  load_win(obs_row(a, rc), win);
  {
#pragma clang fp contract(fast)
#pragma unroll 1
    for (int c = 0; c < 5; c++) {
      float v[49];
      conv1_ch(P, win, c, v);
      float m, var;
      inst_stats<49>(v, m, var);
      const float inv = 1.0f / sqrtf(var + BN_EPS), gi = P[B1W + c] * inv * vf;
      // dz = g inv (dy - mean(dy) - xh mean(dy xh)), the means over the row's own 49
      // values and dy = gy1 at the pool windows' positions; the means and their
      // subtraction in double (see conv2grad)
      const double T0 = (double)fr[(WS_T + c) * rp + rc] / 49.0, T1 = (double)fr[(WS_T + 5 + c) * rp + rc] / 49.0;
      const unsigned pos1 = (unsigned)ir[(WS_POS1 + c) * rp + rc];
      float gyq[9];
#pragma unroll
      for (int q = 0; q < 9; q++) gyq[q] = fr[(WS_GY1 + c * 9 + q) * rp + rc];
#pragma unroll
      for (int i = 0; i < 49; i++) {
        const int ri = i / 7, ci = i % 7;
        float dy = 0.f;
        if (ri < 6 && ci < 6) {
          const int q = (ri / 2) * 3 + ci / 2, k = (ri % 2) * 2 + ci % 2;
          dy = (int)((pos1 >> (2 * q)) & 3u) == k ? gyq[q] : 0.f;
        }
        const float xh = (v[i] - m) * inv;
        v[i] = (float)(((double)dy - T0) - (double)xh * T1);
      }
      double sb = 0.0;  // (the terms cancel: their sum without a rounding of its own)
#pragma unroll
      for (int i = 0; i < 49; i++) {
        v[i] *= gi;
        sb += (double)v[i];
      }
      accum(wsl, S5_N, S5_C1B + c, (float)sb);
      conv1_wgrad(v, win, c, wsl);
    }
  }
  flush(wsl, S5_N, w.fslab + (long long)blockIdx.x * CONV_SLABW);
}

// the conv passes' slabs summed per destination (fixed order, double accumulators)
__global__ __launch_bounds__(256) void pl_reduce_conv_kernel(lnw_ppolearn_args a, Ws w, int kind, int count,
                                                             int logstd) {
  const int i = blockIdx.x * 4 + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  if (i >= count) return;  // (wave-uniform)
  double s = 0.0;
  for (int b = lane; b < w.nblk; b += WAVE) s += (double)w.fslab[(long long)b * CONV_SLABW + i];
  s = wave_sum_d(s);
  if (lane != 0) return;
  a.actor_grad[conv_grad_slot(kind, i, true)] = (float)s;
  // the running statistics' and logstd's slots of the gradient vector are zero
  zero_running_slots(a.actor_grad, kind, i);
  if (kind == RED_CONV1 && i == 0) a.actor_grad[logstd] = 0.f;
}

// ---- running statistics after the B sequential updates (momentum 0.1) ---------------------------
// running = 0.9^B running_0 + 0.1 sum_i 0.9^(B - 1 - i) stat_i, rows in minibatch
// order; one workgroup per statistic, the last RUN_TAIL rows (the weights of
// earlier ones are below the smallest float32)
__global__ __launch_bounds__(256) void pl_running_kernel(lnw_ppolearn_args a, Ws w) {
  double *red = (double *)pl_lds;  // [4]
  const int j = blockIdx.x;        // 0..12 means, 13..25 variances (conv1 5, conv2 8)
  const long long B = a.rows;
  const long long i0 = B > RUN_TAIL ? B - RUN_TAIL : 0;
  const float *st = w.col + (WS_ST + j) * w.rows_pad;
  double s = 0.0;
  for (long long i = i0 + threadIdx.x; i < B; i += 256) s += pow(0.9, (double)(B - 1 - i)) * (double)st[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  s = (red[0] + red[1]) + (red[2] + red[3]);
  const int k = j < 13 ? j : j - 13;
  const int slot = j < 13 ? (k < 5 ? B1M + k : B2M + (k - 5)) : (k < 5 ? B1V + k : B2V + (k - 5));
  a.actor_params[slot] = (float)(pow(0.9, (double)B) * (double)a.actor_params[slot] + 0.1 * s);
}

// ---- global-norm clip and Adam --------------------------------------------------------------
// scale_norm[0] = min(1, max_norm / (norm + 1e-6)), [1] = norm (clip_grad_norm_)
__global__ __launch_bounds__(ADV_THREADS) void pl_norm_kernel(const float *g, long long count, float max_norm,
                                                              float *scale_norm) {
  double *red = (double *)pl_lds;
  double s = 0.0;
  for (long long i = threadIdx.x; i < count; i += ADV_THREADS) s += (double)g[i] * (double)g[i];
  s = block_sum_d(s, red);
  if (threadIdx.x != 0) return;
  const float norm = (float)sqrt(s);
  const float coef = max_norm / (norm + 1e-6f);
  scale_norm[0] = coef < 1.0f ? coef : (coef >= 1.0f ? 1.0f : coef);  // (NaN stays NaN)
  scale_norm[1] = norm;
}

__global__ __launch_bounds__(256) void pl_adam_kernel(float *p, const float *g, float *m, float *v, long long count,
                                                      const long long *step_dev, double lr, double beta1,
                                                      double beta2, double eps, const float *scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  adam_apply(p, m, v, i, g[i] * scale[0], step_dev, lr, beta1, beta2, eps);
}

__global__ void pl_advance_kernel(long long *step_dev) { *step_dev += 1; }

// ---- host ---------------------------------------------------------------------------------------
long long align16(long long b) { return (b + 15) & ~15ll; }

struct Plan {
  long long rows_pad, bytes;
  int nblk, nchunks, chunk_rows, slabw;
  long long o_dslab, o_retd, o_fslab, o_x0, o_xh, o_h1, o_h2, o_h3, o_z, o_c1, o_c2, o_c3, o_col;
};

bool make_plan(long long rows, int n, int D, Plan &p) {
  if (rows < 1 || rows + 256 >= (1ll << 31) || n < 1 || n > 16 || !obs_width_ok(D, true)) return false;
  p.nblk = (int)((rows + LEARN_THREADS - 1) / LEARN_THREADS);
  p.rows_pad = (long long)p.nblk * LEARN_THREADS;
  p.nchunks = (int)((rows + 255) / 256);
  if (p.nchunks > 512) p.nchunks = 512;
  p.chunk_rows = (int)((((rows + p.nchunks - 1) / p.nchunks) + 3) & ~3ll);
  p.nchunks = (int)((rows + p.chunk_rows - 1) / p.chunk_rows);
  const int k1 = n * D;
  int sw = FC1 * (MAX_IN + 1);
  if (CF1 * (k1 + 1) > sw) sw = CF1 * (k1 + 1);
  p.slabw = (sw + 3) & ~3;
  long long slab = (long long)p.nchunks * p.slabw;
  if ((long long)p.nblk * CONV_SLABW > slab) slab = (long long)p.nblk * CONV_SLABW;
  long long o = 0;
  const long long rp = p.rows_pad;
  p.o_dslab = o; o = align16(o + (long long)p.nblk * 8);
  p.o_retd = o; o = align16(o + rp * 8);
  p.o_fslab = o; o = align16(o + slab * 4);
  p.o_x0 = o; o += rp * LDW * 4;
  p.o_xh = o; o += rp * LDW * 4;
  p.o_h1 = o; o += rp * FC1 * 4;
  p.o_h2 = o; o += rp * FC2 * 4;
  p.o_h3 = o; o += rp * FC3 * 4;
  p.o_z = o; o += rp * NHEAD * 4;
  p.o_c1 = o; o += rp * CF1 * 4;
  p.o_c2 = o; o += rp * CF2 * 4;
  p.o_c3 = o; o += rp * CF3 * 4;
  p.o_col = o; o += rp * WS_FIELDS * 4;
  p.bytes = o;
  return true;
}

struct Chain {
  hipStream_t st;
  const Plan *p;
  float *fslab;
  long long rows;

  void fwd(Lin L) const {
    const unsigned rt = (unsigned)((rows + 15) / 16);
    pl_linear_fwd_kernel<<<dim3((rt + 3) / 4, (unsigned)((L.N + 15) / 16)), 256, 0, st>>>(L);
  }
  // L.Y holds dY; the weights' gradient into grad, then dX over the layer's input
  void wgrad(Lin L, float *grad, int off_w, int off_b) const {
    const int kb = L.K + (L.b ? 1 : 0);
    const int tiles = ((kb + 15) / 16) * ((L.N + 15) / 16);
    pl_linear_wgrad_kernel<<<dim3((unsigned)p->nchunks, (unsigned)((tiles + 3) / 4)), 256, 0, st>>>(
        L, fslab, p->slabw, p->chunk_rows);
    const int count = L.N * kb;
    pl_reduce_lin_kernel<<<(unsigned)((count + 3) / 4), 256, 0, st>>>(fslab, p->slabw, p->nchunks, count, kb, L.K,
                                                                     grad, off_w, off_b);
  }
  void bwd(Lin L, float *dX, int ldd, int kw, int act) const {
    const unsigned rt = (unsigned)((rows + 15) / 16);
    pl_linear_bwd_kernel<<<dim3((rt + 3) / 4, (unsigned)((kw + 15) / 16)), 256, 0, st>>>(L, dX, ldd, kw, act);
  }
};

Lin lin(const float *X, long long ldx, const float *W, const float *b, int K, int N, float *Y, int ldy,
        long long rows, int act) {
  Lin L;
  L.X = X; L.ldx = ldx; L.idx = nullptr; L.div = 1;
  L.W = W; L.b = b; L.K = K; L.N = N; L.Y = Y; L.ldy = ldy; L.rows = rows; L.act = act;
  return L;
}

}  // namespace

extern "C" {

int64_t lnw_ppolearn_workspace_bytes(int64_t rows, int32_t n, int32_t D) {
  Plan p;
  return make_plan(rows, n, D, p) ? p.bytes : 0;
}

int lnw_ppo_grad(const lnw_ppolearn_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_ppolearn_args &a = *args;
  if (!a.obs || !a.actions || !a.old_log_probs || !a.rtg || !a.old_values || !a.actor_params || !a.critic_params ||
      !a.actor_grad || !a.critic_grad || !a.actor_loss || !a.critic_loss || !a.workspace)
    return LNW_EINVAL;
  if (a.rows < 1 || a.n < 1) return LNW_EINVAL;
  // 16-B aligned rows for the vector loads and stores
  if (((uintptr_t)a.obs & 15) || ((uintptr_t)a.workspace & 15) || ((uintptr_t)a.actions & 15) ||
      ((uintptr_t)a.old_log_probs & 15) || (a.new_log_probs && ((uintptr_t)a.new_log_probs & 15)) ||
      (a.entropies && ((uintptr_t)a.entropies & 15)))
    return LNW_EINVAL;
  Plan p;
  if (!make_plan(a.rows, a.n, a.D, p)) return LNW_EUNSUPPORTED;
  if (a.workspace_bytes < p.bytes) return LNW_EINVAL;
  const int n_in = a.D - WIN + 12, k1 = a.n * a.D;
  const ActorOff ao = actor_off(n_in);
  const CriticOff co = critic_off(k1);
  char *base = (char *)a.workspace;
  Ws w;
  w.dslab = (double *)(base + p.o_dslab);
  w.retd = (double *)(base + p.o_retd);
  w.fslab = (float *)(base + p.o_fslab);
  w.x0 = (float *)(base + p.o_x0);
  w.xh = (float *)(base + p.o_xh);
  w.h1 = (float *)(base + p.o_h1);
  w.h2 = (float *)(base + p.o_h2);
  w.h3 = (float *)(base + p.o_h3);
  w.z = (float *)(base + p.o_z);
  w.c1 = (float *)(base + p.o_c1);
  w.c2 = (float *)(base + p.o_c2);
  w.c3 = (float *)(base + p.o_c3);
  w.col = (float *)(base + p.o_col);
  w.rows_pad = p.rows_pad;
  w.nblk = p.nblk;
  w.nchunks = p.nchunks;
  w.chunk_rows = p.chunk_rows;
  w.slabw = p.slabw;
  hipStream_t st = (hipStream_t)stream;
  const Chain ch{st, &p, w.fslab, a.rows};
  const unsigned nb = (unsigned)p.nblk;
  const size_t f4 = sizeof(float);
  const long long R = a.rows;
  const float *AP = a.actor_params, *CP = a.critic_params;
  float *V = w.col + WS_V * p.rows_pad, *DV = w.col + WS_DV * p.rows_pad;

  // ---- forward
  pl_features_kernel<<<nb, LEARN_THREADS, (FEAT_LDS + PARK) * f4, st>>>(a, w, n_in);
  const Lin a1 = lin(w.x0, LDW, AP + ao.w1, AP + ao.b1, n_in, FC1, w.h1, FC1, R, 1);
  const Lin a2 = lin(w.h1, FC1, AP + ao.w2, AP + ao.b2, FC1, FC2, w.h2, FC2, R, 1);
  const Lin a3 = lin(w.h2, FC2, AP + ao.w3, AP + ao.b3, FC2, FC3, w.h3, FC3, R, 1);
  const Lin ah = lin(w.h3, FC3, AP + ao.hw, nullptr, FC3, NHEAD, w.z, NHEAD, R, 0);
  ch.fwd(a1);
  ch.fwd(a2);
  ch.fwd(a3);
  ch.fwd(ah);
  Lin c1 = lin(a.obs, k1, CP + co.w1, CP + co.b1, k1, CF1, w.c1, CF1, R, 1);
  c1.idx = a.row_index;
  c1.div = a.n;
  const Lin c2 = lin(w.c1, CF1, CP + co.w2, CP + co.b2, CF1, CF2, w.c2, CF2, R, 1);
  const Lin c3 = lin(w.c2, CF2, CP + co.w3, CP + co.b3, CF2, CF3, w.c3, CF3, R, 1);
  const Lin c4 = lin(w.c3, CF3, CP + co.w4, CP + co.b4, CF3, 1, V, 1, R, 0);
  ch.fwd(c1);
  ch.fwd(c2);
  ch.fwd(c3);
  ch.fwd(c4);
  // ---- advantage, losses, the outputs' gradients
  pl_advantage_kernel<<<1, ADV_THREADS, 2 * ADV_THREADS * sizeof(double), st>>>(a, w, as_decimal(a.gamma),
                                                                              as_decimal(a.lambda_));
  pl_actorloss_kernel<<<nb, LEARN_THREADS, LEARN_WAVES * sizeof(double), st>>>(a, w);
  pl_actorloss_sum_kernel<<<1, WAVE, 0, st>>>(a, w);
  // ---- critic backward (each layer's output buffer holds its gradient; dX goes over the input)
  Lin g4 = c4;
  g4.Y = DV;
  ch.wgrad(g4, a.critic_grad, co.w4, co.b4);
  ch.bwd(g4, w.c3, CF3, CF3, 1);
  ch.wgrad(c3, a.critic_grad, co.w3, co.b3);
  ch.bwd(c3, w.c2, CF2, CF2, 1);
  ch.wgrad(c2, a.critic_grad, co.w2, co.b2);
  ch.bwd(c2, w.c1, CF1, CF1, 1);
  ch.wgrad(c1, a.critic_grad, co.w1, co.b1);
  // ---- actor backward
  ch.wgrad(ah, a.actor_grad, ao.hw, 0);
  ch.bwd(ah, w.h3, FC3, FC3, 1);
  ch.wgrad(a3, a.actor_grad, ao.w3, ao.b3);
  ch.bwd(a3, w.h2, FC2, FC2, 1);
  ch.wgrad(a2, a.actor_grad, ao.w2, ao.b2);
  ch.bwd(a2, w.h1, FC1, FC1, 1);
  ch.wgrad(a1, a.actor_grad, ao.w1, ao.b1);
  ch.bwd(a1, w.x0, LDW, LDW, 0);
  pl_lnwgrad_kernel<<<(unsigned)p.nchunks, WAVE, 0, st>>>(a, w, n_in);
  pl_reduce_lin_kernel<<<(unsigned)((n_in + 3) / 4), 256, 0, st>>>(w.fslab, p.slabw, p.nchunks, n_in, n_in, n_in,
                                                                  a.actor_grad, ao.lnw, 0);
  pl_reduce_lin_kernel<<<(unsigned)((n_in + 3) / 4), 256, 0, st>>>(w.fslab + LDW, p.slabw, p.nchunks, n_in, n_in,
                                                                  n_in, a.actor_grad, ao.lnb, 0);
  pl_lnbwd_kernel<<<nb, LEARN_THREADS, 0, st>>>(a, w, n_in);
  pl_conv2grad_kernel<<<nb, LEARN_THREADS, (size_t)(CONV_LDS + 2 * PARK + LEARN_WAVES * S4_N_TAIL) * f4, st>>>(a, w);
  pl_reduce_conv_kernel<<<(S4_N_TAIL + 3) / 4, 256, 0, st>>>(a, w, RED_CONV2, S4_N_TAIL, ao.logstd);
  pl_conv1grad_kernel<<<nb, LEARN_THREADS, (size_t)(CONV_LDS + LEARN_WAVES * S5_N) * f4, st>>>(a, w);
  pl_reduce_conv_kernel<<<(S5_N + 3) / 4, 256, 0, st>>>(a, w, RED_CONV1, S5_N, ao.logstd);
  if (!a.freeze_running) pl_running_kernel<<<26, 256, 4 * sizeof(double), st>>>(a, w);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

int lnw_ppo_clip_adam(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step_dev,
                      float lr, float beta1, float beta2, float eps, float max_norm, float *scale_norm,
                      void *stream) {
  if (!adam_args_ok(params, grad, m, v, count, step_dev, lr, beta1, beta2, eps) || !scale_norm || !(max_norm > 0.f))
    return LNW_EINVAL;
  if (count == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const AdamHyper h = adam_hyper(lr, beta1, beta2, eps);
  pl_norm_kernel<<<1, ADV_THREADS, ADV_THREADS * sizeof(double), st>>>(grad, count, max_norm, scale_norm);
  pl_adam_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(params, grad, m, v, count,
                                                                  (const long long *)step_dev, h.lr, h.beta1,
                                                                  h.beta2, h.eps, scale_norm);
  pl_advance_kernel<<<1, 1, 0, st>>>((long long *)step_dev);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
