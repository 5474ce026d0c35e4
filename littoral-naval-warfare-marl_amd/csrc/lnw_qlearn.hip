// DDQN learner step (lnw_qnet_grad, lnw_qnet_adam): the reference's optimize()
// (ddqn.py:153-247) for one side on B transition rows — the TD target from the
// target network in BatchNorm training mode, the policy network's gathered
// Q-values, the MSE loss, its gradient through the three heads, convhead, both
// max pools, both BatchNorms (batch statistics with the batch-mean terms, or the
// running statistics as a fixed affine map) and both convolutions, the running
// statistics' update, and the clamped Adam step.
//
// One thread per row; the cheap forward is recomputed in every pass. A chain of
// plain launches on the caller's stream, no synchronisation across workgroups
// inside a kernel and no atomics: every cross-workgroup sum is per-workgroup
// partials in the workspace ("slabs"), summed in a fixed order by a later
// launch, so results are bitwise equal from run to run.
//
//   moments1   conv1 of state (policy) and next_state (target): per-channel sum
//              and sum of squares, double
//   moments2   BN1, ReLU, pool, conv2: the same for conv2's 8 channels
//   forward    target forward -> y; policy forward -> qs, loss partials, the
//              gradients of convhead and BN2's affine (= BN2's backward sums);
//              per row: head inputs, dL/ds of the three chosen outputs, BN2's
//              incoming gradient and pool positions
//   headgrad   W / b gradients: one wave per (128-row chunk, output), the rows
//              that chose the output in ascending order
//   conv2grad  BN2 backward, conv2's weight gradients, gradient to the pooled
//              conv1 maps, BN1's backward sums; per row: BN1's incoming gradient
//              and pool positions
//   conv1grad  BN1 backward and conv1's weight gradients
//   reduce     after each of the above: the slabs summed per destination
//   stats      batch statistics out, running statistics updated in place
//
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
#include "lnw_qhead.inc"
#include "lnw_adam.inc"

// in the LDS copy of the conv head (CONV_LDS floats): the statistics in use in
// the M / V slots, 1 / sqrt(var + eps) of the 5 + 8 channels behind the packed 578
constexpr int I1 = CONV_PARAMS, I2 = CONV_PARAMS + 5;

// slab layouts (floats per workgroup) of the forward pass (the conv passes': lnw_learn.inc)
constexpr int S3_HW = 0, S3_HB = 96, S3_B2W = 108, S3_B2B = 116, S3_LOSS = 124, S3_N = 125;
constexpr int SLAB_MIN = 384;
enum { RED_FWD = 0, RED_HEAD = 1 };  // (then RED_CONV2, RED_CONV1: lnw_learn.inc)

// per-row workspace fields, each [rows_pad]
constexpr int WS_H = 0, WS_DS = 12, WS_GY2 = 15, WS_GY1 = 23, WS_OIDX = 68, WS_POS2 = 71, WS_POS1 = 72, WS_FIELDS = 77;

extern __shared__ float ql_lds[];

struct Ws {
  double *stat1;  // [2 nets][sum 5, sumsq 5]
  double *stat2;  // [2 nets][sum 8, sumsq 8]
  double *dslab;  // [nblk][32]
  float *fslab;   // [nblk][slabw]
  float *row;     // [WS_FIELDS][rows_pad] (floats and ints)
  long long rows_pad;
  int slabw, nblk;
};

// ---- staging -----------------------------------------------------------------
// P <- the packed conv head; with batch statistics, mean and biased variance from
// the summed moments (s1: conv1 [sum 5, sumsq 5] over n1 values; s2: conv2, or
// null) into the M / V slots; 1 / sqrt(var + eps) behind.
__device__ __forceinline__ void stage_conv(float *P, const float *params, const double *s1, double n1,
                                           const double *s2, double n2, bool batch) {
  for (int i = threadIdx.x; i < CONV_PARAMS; i += LEARN_THREADS) P[i] = params[i];
  __syncthreads();
  const int t = threadIdx.x;
  if (t < 13) {
    const bool first = t < 5;
    const int c = first ? t : t - 5;
    const int nch = first ? 5 : 8;
    const double *s = first ? s1 : s2;
    const int M = first ? B1M : B2M, V = first ? B1V : B2V;
    if (batch && s) {
      const double n = first ? n1 : n2;
      const double mean = s[c] / n;
      double var = s[nch + c] / n - mean * mean;
      var = var < 0.0 ? 0.0 : var;
      P[M + c] = (float)mean;
      P[V + c] = (float)var;
    }
    P[(first ? I1 : I2) + c] = 1.0f / sqrtf(P[V + c] + BN_EPS);
  }
  __syncthreads();
}

// ---- forward pieces (conv1_ch, conv2_raw: lnw_convhead.inc) -----------------------
// conv1 -> BN (statistics in P) -> ReLU -> 2x2 pool: the pooled maps into pc
__device__ __forceinline__ void fwd_p1(const float *P, const float (&win)[WIN], float *pc) {
#pragma unroll 1
  for (int c = 0; c < 5; c++) {
    float v[49];
    conv1_ch(P, win, c, v);
    bn_relu_pool1(v, c, P[B1M + c], P[I1 + c], P[B1W + c], P[B1B + c], pc);
  }
}

// x[12 ..] = obs[49 .. D - 1], zeros past n_in
template <int NI>
__device__ __forceinline__ void load_tail(const float *row, int n_in, float (&x)[NI]) {
#pragma unroll
  for (int k = 12; k < NI; k++) x[k] = k < n_in ? row[37 + k] : 0.f;
}

template <int NI>
__device__ __forceinline__ float head_max(const float *Wl, const float *bl, const float (&x)[NI], int o0, int cnt) {
  float best = 0.f;  // (the outputs are ReLU'd: none is below 0)
#pragma unroll 1
  for (int j = 0; j < cnt; j++) best = fmaxf(best, head_dot<NI>(Wl, bl, x, o0 + j));
  return best;
}

// ---- pass 1: conv1 moments of both nets -----------------------------------------
__global__ __launch_bounds__(LEARN_THREADS) void ql_moments1_kernel(lnw_qlearn_args a, Ws w) {
  float *Pp = ql_lds, *Pt = ql_lds + CONV_LDS;
  double *dsl = (double *)(ql_lds + 2 * CONV_LDS);  // [LEARN_WAVES][20]
  for (int i = threadIdx.x; i < CONV_PARAMS; i += LEARN_THREADS) {
    Pp[i] = a.policy_params[i];
    Pt[i] = a.target_params[i];
  }
  __syncthreads();
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
#pragma unroll 1
  for (int net = 0; net < 2; net++) {
    float win[WIN];
    load_win((net ? a.next_state : a.state) + rc * a.D, win);
    const float *P = net ? Pt : Pp;
#pragma unroll 1
    for (int c = 0; c < 5; c++) {
      float v[49];
      conv1_ch(P, win, c, v);
      double s = 0.0, q = 0.0;
#pragma unroll
      for (int i = 0; i < 49; i++) {
        const double d = (double)v[i];
        s += d;
        q += d * d;
      }
      s = wave_sum_d(valid ? s : 0.0);
      q = wave_sum_d(valid ? q : 0.0);
      if ((threadIdx.x & (WAVE - 1)) == 0) {
        dsl[(threadIdx.x / WAVE) * 20 + net * 10 + c] = s;
        dsl[(threadIdx.x / WAVE) * 20 + net * 10 + 5 + c] = q;
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 20) w.dslab[(long long)blockIdx.x * 32 + threadIdx.x] = dsl[threadIdx.x] + dsl[20 + threadIdx.x];
}

// ---- pass 2: conv2 moments of both nets -------------------------------------------
__global__ __launch_bounds__(LEARN_THREADS) void ql_moments2_kernel(lnw_qlearn_args a, Ws w) {
  float *Pp = ql_lds, *Pt = ql_lds + CONV_LDS;
  float *pc = ql_lds + 2 * CONV_LDS + threadIdx.x;
  double *dsl = (double *)(ql_lds + 2 * CONV_LDS + PARK);  // [LEARN_WAVES][32]
  const double n1 = 49.0 * (double)a.rows;
  stage_conv(Pp, a.policy_params, w.stat1, n1, nullptr, 0.0, a.policy_bn_running == 0);
  stage_conv(Pt, a.target_params, w.stat1 + 10, n1, nullptr, 0.0, true);
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
#pragma unroll 1
  for (int net = 0; net < 2; net++) {
    const float *P = net ? Pt : Pp;
    {
      float win[WIN];
      load_win((net ? a.next_state : a.state) + rc * a.D, win);
      fwd_p1(P, win, pc);
    }
#pragma unroll 1
    for (int c0 = 0; c0 < 8; c0 += 4) {
      float v2[4][9];
      conv2_raw(P, pc, LEARN_THREADS, c0, v2);
#pragma unroll
      for (int co = 0; co < 4; co++) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
          const double d = (double)v2[co][i];
          s += d;
          q += d * d;
        }
        s = wave_sum_d(valid ? s : 0.0);
        q = wave_sum_d(valid ? q : 0.0);
        if ((threadIdx.x & (WAVE - 1)) == 0) {
          dsl[(threadIdx.x / WAVE) * 32 + net * 16 + c0 + co] = s;
          dsl[(threadIdx.x / WAVE) * 32 + net * 16 + 8 + c0 + co] = q;
        }
      }
    }
  }
  __syncthreads();
  if (threadIdx.x < 32) w.dslab[(long long)blockIdx.x * 32 + threadIdx.x] = dsl[threadIdx.x] + dsl[32 + threadIdx.x];
}

// the double slabs summed in a fixed order: out[i] = sum over workgroups; one
// wave per destination, lane l takes slabs l, l + 64, ...
__global__ __launch_bounds__(WAVE) void ql_reduce_d_kernel(const double *slab, int nblk, double *out) {
  const int i = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblk; b += WAVE) s += slab[(long long)b * 32 + i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) out[i] = s;
}

// ---- pass 3: both forwards, loss, head-side gradients --------------------------------
template <int NI>
__global__ __launch_bounds__(LEARN_THREADS) void ql_forward_kernel(lnw_qlearn_args a, Ws w, int n_in) {
  float *Pp = ql_lds, *Pt = Pp + CONV_LDS;
  float *Wp = Pt + CONV_LDS, *Wt = Wp + Q_OUT * NI;
  float *bp = Wt + Q_OUT * NI, *bt = bp + BIAS_PAD;
  float *park = bt + BIAS_PAD;
  float *wsl = park + PARK;  // [LEARN_WAVES][S3_N]
  const double n1 = 49.0 * (double)a.rows, n2 = 9.0 * (double)a.rows;
  stage_conv(Pp, a.policy_params, w.stat1, n1, w.stat2, n2, a.policy_bn_running == 0);
  stage_conv(Pt, a.target_params, w.stat1 + 10, n1, w.stat2 + 16, n2, true);
  stage_heads<NI>(Wp, bp, a.policy_params, n_in, LEARN_THREADS);
  stage_heads<NI>(Wt, bt, a.target_params, n_in, LEARN_THREADS);
  __syncthreads();
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
  float *pc = park + threadIdx.x;
  float x[NI];
  // ---- target: y = float32(double(float32(gamma * max) * done) + reward)
  float y[3];
  {
    const float *row = a.next_state + rc * a.D;
    float h[12];
    // (the batch statistics are in the M / V slots: the running-mode path of the shared head)
    conv_head_row(Pt, row, pc, LEARN_THREADS, true, h);
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = h[k];
    load_tail<NI>(row, n_in, x);
    float nxt[3];
    nxt[0] = head_max<NI>(Wt, bt, x, 0, 2);
    nxt[1] = head_max<NI>(Wt, bt, x, 2, 5);
    nxt[2] = head_max<NI>(Wt, bt, x, 7, 50);
    const float dn = (float)a.done[rc];
#pragma unroll
    for (int hd = 0; hd < 3; hd++) {
      const float t = (a.gamma * nxt[hd]) * dn;
      y[hd] = a.reward_f64 ? (float)((double)t + ((const double *)a.reward)[rc])
                           : t + ((const float *)a.reward)[rc];
    }
  }
  // ---- policy forward
  float f[8], xs[8];
  unsigned pos2 = 0;
  {
#pragma clang fp contract(fast)
    const float *row = a.state + rc * a.D;
    {
      float win[WIN];
      load_win(row, win);
      fwd_p1(Pp, win, pc);
    }
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = Pp[HB + k];
#pragma unroll
    for (int c0 = 0; c0 < 8; c0 += 4) {
      float v2[4][9];
      conv2_raw(Pp, pc, LEARN_THREADS, c0, v2);
#pragma unroll
      for (int co = 0; co < 4; co++) {
        const int c = c0 + co;
        const float m = Pp[B2M + c], inv = Pp[I2 + c], g = Pp[B2W + c], b = Pp[B2B + c];
        const float h0 = (v2[co][0] - m) * inv, h1 = (v2[co][1] - m) * inv;
        const float h3 = (v2[co][3] - m) * inv, h4 = (v2[co][4] - m) * inv;
        int sel;
        f[c] = first_max4(fmaxf(h0 * g + b, 0.f), fmaxf(h1 * g + b, 0.f), fmaxf(h3 * g + b, 0.f),
                          fmaxf(h4 * g + b, 0.f), sel);
        xs[c] = sel == 0 ? h0 : sel == 1 ? h1 : sel == 2 ? h3 : h4;
        pos2 |= (unsigned)(sel < 2 ? sel : sel + 1) << (4 * c);
#pragma unroll
        for (int k = 0; k < 12; k++) x[k] += Pp[HW + k * 8 + c] * f[c];
      }
    }
    load_tail<NI>(row, n_in, x);
  }
  // ---- gathered Q-values, loss, dL/ds
  int oi[3];
  float ds[3], lsum = 0.f;
  {
    const int *act = a.action + rc * a.action_stride;
    oi[0] = min(max(act[0], 0), 1);
    oi[1] = 2 + min(max(act[1], 0), 4);
    oi[2] = 7 + min(max(act[2], 0), 49);
    const float scale = 2.0f / (3.0f * (float)a.rows);
#pragma unroll
    for (int hd = 0; hd < 3; hd++) {
      const float s = head_dot<NI>(Wp, bp, x, oi[hd]);
      const float q = s < 0.f ? 0.f : s;
      const float d = q - y[hd];
      lsum += d * d;
      ds[hd] = (valid && s > 0.f) ? scale * d : 0.f;
      if (valid && a.qs_out) a.qs_out[r * 3 + hd] = q;
      if (valid && a.y_out) a.y_out[r * 3 + hd] = y[hd];
    }
  }
  accum(wsl, S3_N, S3_LOSS, valid ? lsum : 0.f);
  // ---- backward through the heads' first 12 inputs, convhead, pool 2, ReLU
  float dh[12];
#pragma unroll
  for (int k = 0; k < 12; k++)
    dh[k] = (ds[0] * Wp[oi[0] * NI + k] + ds[1] * Wp[oi[1] * NI + k]) + ds[2] * Wp[oi[2] * NI + k];
#pragma unroll
  for (int k = 0; k < 12; k++) {
    accum(wsl, S3_N, S3_HB + k, dh[k]);
#pragma unroll
    for (int c = 0; c < 8; c++) accum(wsl, S3_N, S3_HW + k * 8 + c, dh[k] * f[c]);
  }
  float gy2[8];
#pragma unroll
  for (int c = 0; c < 8; c++) {
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < 12; k++) d += dh[k] * Pp[HW + k * 8 + c];
    gy2[c] = f[c] > 0.f ? d : 0.f;
    accum(wsl, S3_N, S3_B2W + c, gy2[c] * xs[c]);
    accum(wsl, S3_N, S3_B2B + c, gy2[c]);
  }
  if (valid) {
    float *fr = w.row;
    int *ir = (int *)w.row;
    const long long rp = w.rows_pad;
#pragma unroll
    for (int k = 0; k < 12; k++) fr[(WS_H + k) * rp + r] = x[k];
#pragma unroll
    for (int hd = 0; hd < 3; hd++) {
      fr[(WS_DS + hd) * rp + r] = ds[hd];
      ir[(WS_OIDX + hd) * rp + r] = oi[hd];
    }
#pragma unroll
    for (int c = 0; c < 8; c++) fr[(WS_GY2 + c) * rp + r] = gy2[c];
    ir[WS_POS2 * rp + r] = (int)pos2;
  }
  flush(wsl, S3_N, w.fslab + (long long)blockIdx.x * w.slabw);
}

// ---- head gradients: one wave per (chunk of LEARN_THREADS rows, output) ----------------
__global__ __launch_bounds__(WAVE) void ql_headgrad_kernel(lnw_qlearn_args a, Ws w, int n_in) {
  const int o = blockIdx.y, hd = o < 2 ? 0 : (o < 7 ? 1 : 2);
  const int lane = threadIdx.x;
  const float *fr = w.row;
  const int *ir = (const int *)w.row;
  const long long rp = w.rows_pad;
  float acc = 0.f, bsum = 0.f;
#pragma unroll 1
  for (int half = 0; half < LEARN_THREADS / WAVE; half++) {
    const long long r0 = (long long)blockIdx.x * LEARN_THREADS + half * WAVE;
    const long long r = r0 + lane;
    const bool match = r < a.rows && ir[(WS_OIDX + hd) * rp + r] == o;
    const float d = match ? fr[(WS_DS + hd) * rp + r] : 0.f;
    unsigned long long mask = __ballot(match);
    while (mask) {  // (wave-uniform) the matching rows in ascending order
      const int l = __builtin_ctzll(mask);
      mask &= mask - 1;
      const long long rr = r0 + l;
      const float dv = __shfl(d, l);
      float xk = 0.f;
      if (lane < 12)
        xk = fr[(WS_H + lane) * rp + rr];
      else if (lane < n_in)
        xk = a.state[rr * a.D + 37 + lane];
      acc += dv * xk;
      bsum += dv;
    }
  }
  float *slab = w.fslab + (long long)blockIdx.x * w.slabw;
  if (lane < n_in) slab[o * n_in + lane] = acc;
  if (lane == 0) slab[Q_OUT * n_in + o] = bsum;
}

// ---- pass 4: BN2 backward, conv2 gradients, BN1's backward sums ----------------------
__global__ __launch_bounds__(LEARN_THREADS) void ql_conv2grad_kernel(lnw_qlearn_args a, Ws w) {
  float *P = ql_lds;
  float *S = P + CONV_LDS;  // [16] BN2's backward means: sum(dy) / n, sum(dy xh) / n
  float *parkA = S + 16, *parkB = parkA + PARK;
  float *wsl = parkB + PARK;  // [LEARN_WAVES][S4_N]
  const double n1 = 49.0 * (double)a.rows, n2 = 9.0 * (double)a.rows;
  const bool batch = a.policy_bn_running == 0;
  if (threadIdx.x < 8) {
    S[threadIdx.x] = batch ? (float)((double)a.grad[B2B + threadIdx.x] / n2) : 0.f;
    S[8 + threadIdx.x] = batch ? (float)((double)a.grad[B2W + threadIdx.x] / n2) : 0.f;
  }
  stage_conv(P, a.policy_params, w.stat1, n1, w.stat2, n2, batch);
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
  const float vf = valid ? 1.f : 0.f;
  float *pA = parkA + threadIdx.x, *pB = parkB + threadIdx.x;
  const float *fr = w.row;
  const int *ir = (const int *)w.row;
  const long long rp = w.rows_pad;
  float win[WIN];
  load_win(a.state + rc * a.D, win);
  fwd_p1(P, win, pA);
#pragma unroll
  for (int k = 0; k < 45; k++) pB[k * LEARN_THREADS] = 0.f;
  const unsigned pos2 = (unsigned)ir[WS_POS2 * rp + rc];
  {
#pragma clang fp contract(fast)
#pragma unroll 1
    for (int c0 = 0; c0 < 8; c0 += 4) {
      float dz[4][9];
      conv2_raw(P, pA, LEARN_THREADS, c0, dz);
      // BN2 backward: dz = g inv (dy - mean(dy) - xh mean(dy xh)); dy is gy2 at the pool's position
#pragma unroll
      for (int co = 0; co < 4; co++) {
        const int c = c0 + co;
        const float m = P[B2M + c], inv = P[I2 + c], gi = P[B2W + c] * inv * vf;
        const float gy = fr[(WS_GY2 + c) * rp + rc];
        const int pos = (int)((pos2 >> (4 * c)) & 15u);
        float sb = 0.f;
#pragma unroll
        for (int q = 0; q < 9; q++) {
          const float xh = (dz[co][q] - m) * inv;
          const float dy = q == pos ? gy : 0.f;
          dz[co][q] = gi * ((dy - S[c]) - xh * S[8 + c]);
          sb += dz[co][q];
        }
        accum(wsl, S4_N, S4_C2B + c, sb);
      }
      conv2_bwd(P, pA, pB, c0, dz, wsl, S4_N);
    }
  }
  // through pool 1 and the ReLU: conv1 again, channel by channel
  {
#pragma clang fp contract(fast)
#pragma unroll 1
    for (int c = 0; c < 5; c++) {
      float v[49];
      conv1_ch(P, win, c, v);
      const float m = P[B1M + c], inv = P[I1 + c];
#pragma unroll
      for (int i = 0; i < 49; i++) v[i] = (v[i] - m) * inv;
      float t1, t2;
      unsigned pos1;
      pool1_bwd(v, P[B1W + c], P[B1B + c], pB + c * 9 * LEARN_THREADS, valid, w.row + (WS_GY1 + c * 9) * rp + r, rp,
                pos1, t1, t2);
      if (valid) ((int *)w.row)[(WS_POS1 + c) * rp + r] = (int)pos1;
      accum(wsl, S4_N, S4_B1W + c, t2);
      accum(wsl, S4_N, S4_B1B + c, t1);
    }
  }
  flush(wsl, S4_N, w.fslab + (long long)blockIdx.x * w.slabw);
}

// ---- pass 5: BN1 backward, conv1 gradients --------------------------------------------
__global__ __launch_bounds__(LEARN_THREADS) void ql_conv1grad_kernel(lnw_qlearn_args a, Ws w) {
  float *P = ql_lds;
  float *T = P + CONV_LDS;  // [10] BN1's backward means
  float *wsl = T + 16;      // [LEARN_WAVES][S5_N]
  const double n1 = 49.0 * (double)a.rows;
  const bool batch = a.policy_bn_running == 0;
  if (threadIdx.x < 5) {
    T[threadIdx.x] = batch ? (float)((double)a.grad[B1B + threadIdx.x] / n1) : 0.f;
    T[5 + threadIdx.x] = batch ? (float)((double)a.grad[B1W + threadIdx.x] / n1) : 0.f;
  }
  stage_conv(P, a.policy_params, w.stat1, n1, nullptr, 0.0, batch);
  const long long r = (long long)blockIdx.x * LEARN_THREADS + threadIdx.x;
  const bool valid = r < a.rows;
  const long long rc = valid ? r : a.rows - 1;
  const float vf = valid ? 1.f : 0.f;
  const float *fr = w.row;
  const int *ir = (const int *)w.row;
  const long long rp = w.rows_pad;
  float win[WIN];
  load_win(a.state + rc * a.D, win);
  {
#pragma clang fp contract(fast)
#pragma unroll 1
    for (int c = 0; c < 5; c++) {
      float v[49];
      conv1_ch(P, win, c, v);
      const float m = P[B1M + c], inv = P[I1 + c], gi = P[B1W + c] * inv * vf;
      // dz = g inv (dy - mean(dy) - xh mean(dy xh)); dy is gy1 at the pool windows' positions
#pragma unroll
      for (int i = 0; i < 49; i++) v[i] = -T[c] - ((v[i] - m) * inv) * T[5 + c];
      const unsigned pos1 = (unsigned)ir[(WS_POS1 + c) * rp + rc];
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const int q = i * 3 + j, p0 = 2 * i * 7 + 2 * j;
          const float gy = fr[(WS_GY1 + c * 9 + q) * rp + rc];
          const int sel = (int)((pos1 >> (2 * q)) & 3u);
          v[p0] += sel == 0 ? gy : 0.f;
          v[p0 + 1] += sel == 1 ? gy : 0.f;
          v[p0 + 7] += sel == 2 ? gy : 0.f;
          v[p0 + 8] += sel == 3 ? gy : 0.f;
        }
      float sb = 0.f;
#pragma unroll
      for (int i = 0; i < 49; i++) {
        v[i] *= gi;
        sb += v[i];
      }
      accum(wsl, S5_N, S5_C1B + c, sb);
      conv1_wgrad(v, win, c, wsl);
    }
  }
  flush(wsl, S5_N, w.fslab + (long long)blockIdx.x * w.slabw);
}

// ---- the float slabs summed per destination (fixed order, double accumulators) ---------
__global__ __launch_bounds__(256) void ql_reduce_kernel(lnw_qlearn_args a, Ws w, int kind, int count, int n_in) {
  // one wave per destination, lane l takes slabs l, l + 64, ...
  const int i = blockIdx.x * 4 + threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
  if (i >= count) return;  // (wave-uniform)
  double s = 0.0;
  const float *slab = w.fslab + i;
  const long long sw = w.slabw;
  for (int b = lane; b < w.nblk; b += WAVE) s += (double)slab[b * sw];
  s = wave_sum_d(s);
  if (lane != 0) return;
  int dst;
  if (kind == RED_FWD) {
    if (i == S3_LOSS) {
      a.loss[0] = (float)(s / (3.0 * (double)a.rows));
      return;
    }
    dst = i < S3_HB ? HW + i : i < S3_B2W ? HB + (i - S3_HB) : i < S3_B2B ? B2W + (i - S3_B2W) : B2B + (i - S3_B2B);
  } else if (kind == RED_HEAD) {
    dst = CONV_PARAMS + i;
  } else {
    dst = conv_grad_slot(kind, i, false);
  }
  a.grad[dst] = (float)s;
  zero_running_slots(a.grad, kind, i);
}

// ---- batch statistics out, running statistics (momentum 0.1, unbiased variance) ----------
__global__ __launch_bounds__(WAVE) void ql_stats_kernel(lnw_qlearn_args a, Ws w) {
  const int t = threadIdx.x;
  if (t >= 26) return;
  const int net = t / 13, k = t - net * 13;
  const bool first = k < 5;
  const int c = first ? k : k - 5, nch = first ? 5 : 8;
  const double *s = first ? w.stat1 + net * 10 : w.stat2 + net * 16;
  const double n = (first ? 49.0 : 9.0) * (double)a.rows;
  const double mean = s[c] / n;
  double var = s[nch + c] / n - mean * mean;
  var = var < 0.0 ? 0.0 : var;
  if (a.stats_out) {
    a.stats_out[net * 26 + k] = (float)mean;
    a.stats_out[net * 26 + 13 + k] = (float)var;
  }
  if (a.freeze_running || (net == 0 && a.policy_bn_running)) return;
  float *P = net ? a.target_params : a.policy_params;
  const int M = first ? B1M : B2M, V = first ? B1V : B2V;
  const float mom = 0.1f;
  const float unb = (float)(var * (n / (n - 1.0)));
  P[M + c] = mom * (float)mean + (1.0f - mom) * P[M + c];
  P[V + c] = mom * unb + (1.0f - mom) * P[V + c];
}

// ---- Adam (adam_apply: lnw_adam.inc), gradient clamped first ---------------------------------
__global__ __launch_bounds__(256) void ql_adam_kernel(float *p, const float *g, float *m, float *v, long long count,
                                                      const long long *step_dev, double lr, double beta1,
                                                      double beta2, double eps, float clamp) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  float gi = g[i];
  if (clamp > 0.f) gi = fminf(fmaxf(gi, -clamp), clamp);
  adam_apply(p, m, v, i, gi, step_dev, lr, beta1, beta2, eps);
}

__global__ void ql_advance_kernel(long long *step_dev) { *step_dev += 1; }

int slab_width(int n_in) {
  const int head = Q_OUT * n_in + Q_OUT;
  return ((head > SLAB_MIN ? head : SLAB_MIN) + 3) & ~3;
}

}  // namespace

extern "C" {

int64_t lnw_qlearn_workspace_bytes(int64_t rows, int32_t D) {
  if (rows < 1 || rows + LEARN_THREADS >= (1ll << 31) || !obs_width_ok(D, true)) return 0;
  const int64_t nblk = (rows + LEARN_THREADS - 1) / LEARN_THREADS;
  return 512 + nblk * 32 * 8 + nblk * slab_width(D - WIN + 12) * 4 + (int64_t)WS_FIELDS * nblk * LEARN_THREADS * 4;
}

int lnw_qnet_grad(const lnw_qlearn_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_qlearn_args &a = *args;
  if (!a.state || !a.next_state || !a.action || !a.reward || !a.done || !a.policy_params || !a.target_params ||
      !a.grad || !a.loss || !a.workspace)
    return LNW_EINVAL;
  if (a.rows < 1 || a.action_stride < 3) return LNW_EINVAL;
  // 16-B aligned rows for the vector loads
  if (((uintptr_t)a.state & 15) || ((uintptr_t)a.next_state & 15) || ((uintptr_t)a.workspace & 15)) return LNW_EINVAL;
  if (!obs_width_ok(a.D, true)) return LNW_EUNSUPPORTED;
  if (a.rows + LEARN_THREADS >= (1ll << 31)) return LNW_EUNSUPPORTED;
  if (a.workspace_bytes < lnw_qlearn_workspace_bytes(a.rows, a.D)) return LNW_EINVAL;
  const int n_in = a.D - WIN + 12;
  Ws w;
  w.nblk = (int)((a.rows + LEARN_THREADS - 1) / LEARN_THREADS);
  w.slabw = slab_width(n_in);
  w.rows_pad = (long long)w.nblk * LEARN_THREADS;
  char *base = (char *)a.workspace;
  w.stat1 = (double *)base;
  w.stat2 = w.stat1 + 20;
  w.dslab = (double *)(base + 512);
  w.fslab = (float *)(base + 512 + (size_t)w.nblk * 32 * 8);
  w.row = w.fslab + (size_t)w.nblk * w.slabw;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)w.nblk;
  const size_t f4 = sizeof(float);
  ql_moments1_kernel<<<nb, LEARN_THREADS, (2 * CONV_LDS) * f4 + LEARN_WAVES * 20 * 8, st>>>(a, w);
  ql_reduce_d_kernel<<<20, WAVE, 0, st>>>(w.dslab, w.nblk, w.stat1);
  ql_moments2_kernel<<<nb, LEARN_THREADS, (2 * CONV_LDS + PARK) * f4 + LEARN_WAVES * 32 * 8, st>>>(a, w);
  ql_reduce_d_kernel<<<32, WAVE, 0, st>>>(w.dslab, w.nblk, w.stat2);
  const int NI = n_in <= 32 ? 32 : MAX_IN;
  const size_t lds3 = (size_t)(2 * CONV_LDS + 2 * Q_OUT * NI + 2 * BIAS_PAD + PARK + LEARN_WAVES * S3_N) * f4;
  if (NI == 32)
    ql_forward_kernel<32><<<nb, LEARN_THREADS, lds3, st>>>(a, w, n_in);
  else
    ql_forward_kernel<MAX_IN><<<nb, LEARN_THREADS, lds3, st>>>(a, w, n_in);
  ql_reduce_kernel<<<(S3_N + 3) / 4, 256, 0, st>>>(a, w, RED_FWD, S3_N, n_in);
  ql_headgrad_kernel<<<dim3(nb, Q_OUT), WAVE, 0, st>>>(a, w, n_in);
  const int nhead = Q_OUT * n_in + Q_OUT;
  ql_reduce_kernel<<<(nhead + 3) / 4, 256, 0, st>>>(a, w, RED_HEAD, nhead, n_in);
  ql_conv2grad_kernel<<<nb, LEARN_THREADS, (size_t)(CONV_LDS + 16 + 2 * PARK + LEARN_WAVES * S4_N) * f4, st>>>(a, w);
  ql_reduce_kernel<<<(S4_N + 3) / 4, 256, 0, st>>>(a, w, RED_CONV2, S4_N, n_in);
  ql_conv1grad_kernel<<<nb, LEARN_THREADS, (size_t)(CONV_LDS + 16 + LEARN_WAVES * S5_N) * f4, st>>>(a, w);
  ql_reduce_kernel<<<(S5_N + 3) / 4, 256, 0, st>>>(a, w, RED_CONV1, S5_N, n_in);
  ql_stats_kernel<<<1, WAVE, 0, st>>>(a, w);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

int lnw_qnet_adam(float *params, const float *grad, float *m, float *v, int64_t count, int64_t *step_dev, float lr,
                  float beta1, float beta2, float eps, float clamp, void *stream) {
  if (!adam_args_ok(params, grad, m, v, count, step_dev, lr, beta1, beta2, eps)) return LNW_EINVAL;
  if (count == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const AdamHyper h = adam_hyper(lr, beta1, beta2, eps);
  ql_adam_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(params, grad, m, v, count,
                                                                  (const long long *)step_dev, h.lr, h.beta1,
                                                                  h.beta2, h.eps, clamp);
  ql_advance_kernel<<<1, 1, 0, st>>>((long long *)step_dev);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
