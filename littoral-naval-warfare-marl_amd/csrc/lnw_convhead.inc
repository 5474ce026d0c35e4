// lnw_convhead.inc — the convolutional head the reference's actor and Q-network
// share (network.py:70-82 MLP.forward, network.py:280-291 DMLP.forward): conv
// 1->5 (3x3, pad 1) over the 7x7 terrain window, BatchNorm, ReLU, 2x2 max pool,
// conv 5->8, BatchNorm, ReLU, 2x2 max pool, linear 8->12; one row per thread.
// Included by lnw_actor.hip, lnw_actornoise.hip, lnw_qnet.hip, lnw_qlearn.hip and
// lnw_ppolearn.hip inside their anonymous namespace (after lnw_device.h: WAVE,
// f32x4); the two learners include lnw_learn.inc behind it, which holds the
// backward of this head. The packed parameter layout below is what
// BatchedActor.packed_features() and BatchedQNet.packed() write first.

constexpr int WIN = 49;       // 7x7 terrain window
constexpr int MAX_IN = 64;    // bound of n_in = D - WIN + 12, the head's 12 outputs and the rest of the row
constexpr float BN_EPS = 1e-5f;

// The observation widths D the network kernels take: the window and at most
// MAX_IN network inputs; quads: rows read as float4 (load_tail_q), so D % 4 == 0.
inline bool obs_width_ok(int D, bool quads) { return D >= WIN && D - WIN + 12 <= MAX_IN && !(quads && (D & 3)); }

// packed conv-head parameter layout (floats)
constexpr int C1W = 0, C1B = 45, B1W = 50, B1B = 55, B1M = 60, B1V = 65;
constexpr int C2W = 70, C2B = 430, B2W = 438, B2B = 446, B2M = 454, B2V = 462;
constexpr int HW = 470, HB = 566, CONV_PARAMS = 578;  // then LayerNorm w, b [n_in] each

// BatchNorm of one channel's n values: own statistics (biased variance) or
// running ones, then the affine, then ReLU.
template <int N>
__device__ inline void bn_relu(float (&v)[N], const float *w, const float *b, const float *rm,
                               const float *rv, int c, bool running) {
  float mean, var;
  if (running) {
    mean = rm[c];
    var = rv[c];
  } else {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++) s += v[i];
    mean = s / (float)N;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++) q += (v[i] - mean) * (v[i] - mean);
    var = q / (float)N;
  }
  const float inv = 1.0f / sqrtf(var + BN_EPS);
#pragma unroll
  for (int i = 0; i < N; i++) v[i] = fmaxf((v[i] - mean) * inv * w[c] + b[c], 0.f);
}

// conv1 (1 -> 5, 3x3, pad 1) of the window, output channel c (before BatchNorm)
__device__ __forceinline__ void conv1_ch(const float *P, const float (&win)[WIN], int c, float (&v)[49]) {
#pragma clang fp contract(fast)
  const float *w = P + C1W + c * 9;
#pragma unroll
  for (int i = 0; i < 7; i++)
#pragma unroll
    for (int j = 0; j < 7; j++) {
      float s = P[C1B + c];
#pragma unroll
      for (int ki = 0; ki < 3; ki++)
#pragma unroll
        for (int kj = 0; kj < 3; kj++) {
          const int ii = i + ki - 1, jj = j + kj - 1;
          if (ii >= 0 && ii < 7 && jj >= 0 && jj < 7) s += w[ki * 3 + kj] * win[ii * 7 + jj];
        }
      v[i * 7 + j] = s;
    }
}

// conv2 (5 -> 8, 3x3, pad 1) of the pooled conv1 maps in pc (the thread's column
// of a [45][stride] area), output maps c0 .. c0 + 3 (before BatchNorm). The four
// maps accumulate while the input channels stream in from LDS one at a time (36
// accumulators and 9 inputs live: the head then fits the kernels' registers
// without spilling).
__device__ __forceinline__ void conv2_raw(const float *P, const float *pc, int stride, int c0, float (&v2)[4][9]) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int co = 0; co < 4; co++)
#pragma unroll
    for (int p = 0; p < 9; p++) v2[co][p] = P[C2B + c0 + co];
#pragma unroll 1
  for (int ci = 0; ci < 5; ci++) {
    float pin[9];
#pragma unroll
    for (int k = 0; k < 9; k++) pin[k] = pc[(ci * 9 + k) * stride];
#pragma unroll
    for (int co = 0; co < 4; co++) {
      const float *w = P + C2W + ((c0 + co) * 5 + ci) * 9;
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
          for (int ki = 0; ki < 3; ki++)
#pragma unroll
            for (int kj = 0; kj < 3; kj++) {
              const int ii = i + ki - 1, jj = j + kj - 1;
              if (ii >= 0 && ii < 3 && jj >= 0 && jj < 3) v2[co][i * 3 + j] += w[ki * 3 + kj] * pin[ii * 3 + jj];
            }
    }
  }
}

// 2x2 max pool (7x7 -> 3x3) of conv1's channel c into the thread's column pc of
// a [45][stride] parking area
__device__ __forceinline__ void pool1_park(const float (&v)[49], int c, float *pc, int stride) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int r0 = 2 * i, c0 = 2 * j;
      pc[(c * 9 + i * 3 + j) * stride] =
          fmaxf(fmaxf(v[r0 * 7 + c0], v[r0 * 7 + c0 + 1]), fmaxf(v[(r0 + 1) * 7 + c0], v[(r0 + 1) * 7 + c0 + 1]));
    }
}

// The conv head of one row (network.py:70-82): conv 1->5 over the 7x7 window
// win[0..48] (registers) -> BN -> ReLU -> 2x2 pool, conv 5->8 -> BN -> ReLU ->
// pool, folded into the linear 8->12 (h). P: packed parameters in LDS
// (broadcast reads); pc: the thread's column of a [45][stride] LDS parking area
// for the pooled conv1 maps.
__device__ __forceinline__ void conv_head_win(const float *P, const float (&win)[WIN], float *pc, int stride,
                                              bool running, float (&h)[12]) {
  // multiply-adds fused here and in conv1_ch / conv2_raw (the build's
  // -ffp-contract=off is for the step kernels' bit-exactness; the policy is held
  // to the tolerance of fp32 torch, whose conv kernels fuse them too): half the
  // VALU work of the head
#pragma clang fp contract(fast)
  // conv1 (1 -> 5, 3x3, pad 1) -> BN -> ReLU -> 2x2 max pool (7x7 -> 3x3),
  // one channel at a time (rolled: 49 outputs live)
#pragma unroll 1
  for (int c = 0; c < 5; c++) {
    float v[49];
    conv1_ch(P, win, c, v);
    bn_relu<49>(v, P + B1W, P + B1B, P + B1M, P + B1V, c, running);
    pool1_park(v, c, pc, stride);
  }
  // conv2 (5 -> 8, 3x3, pad 1) -> BN -> ReLU -> 2x2 max pool (3x3 -> 1x1),
  // folded straight into the linear 8 -> 12 (convhead), four output maps at a
  // time (conv2_raw; h sums the maps in channel order).
#pragma unroll
  for (int k = 0; k < 12; k++) h[k] = P[HB + k];
#pragma unroll 1
  for (int c0 = 0; c0 < 8; c0 += 4) {
    float v2[4][9];
    conv2_raw(P, pc, stride, c0, v2);
#pragma unroll
    for (int co = 0; co < 4; co++) {
      bn_relu<9>(v2[co], P + B2W, P + B2B, P + B2M, P + B2V, c0 + co, running);
      const float f = fmaxf(fmaxf(v2[co][0], v2[co][1]), fmaxf(v2[co][3], v2[co][4]));
#pragma unroll
      for (int k = 0; k < 12; k++) h[k] += P[HW + k * 8 + c0 + co] * f;
    }
  }
}

// conv_head_win on a row in memory (features_kernel)
__device__ __forceinline__ void conv_head_row(const float *P, const float *x, float *pc, int stride,
                                              bool running, float (&h)[12]) {
  float win[WIN];
#pragma unroll
  for (int i = 0; i < WIN; i++) win[i] = x[i];
  conv_head_win(P, win, pc, stride, running, h);
}

// What follows the window in a 16-B aligned row of D4 float4 quads (D % 4 == 0;
// the callers check both): tl[k] = x[49 + k], from the quads from x[48] on, one
// dwordx4 per quad instead of one dword load per value, every load issued at
// once (quad indices clamped into the row; the values past D - 49 they
// duplicate are unused)
template <int NT>
__device__ __forceinline__ void load_tail_q(const float *x, int D4, float (&tl)[NT]) {
  constexpr int NQ = (NT + 1 + 3) / 4;  // x[48] .. x[48 + NT]
  const f32x4 *x4 = (const f32x4 *)x;
  f32x4 q[NQ];
#pragma unroll
  for (int j = 0; j < NQ; j++) q[j] = x4[12 + j < D4 ? 12 + j : D4 - 1];
#pragma unroll
  for (int k = 0; k < NT; k++) tl[k] = q[(k + 1) >> 2][(k + 1) & 3];
}
