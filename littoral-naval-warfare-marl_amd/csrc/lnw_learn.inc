// lnw_learn.inc — what the learner steps share: the DDQN step (lnw_qlearn.hip)
// and the MAPPO step (lnw_ppolearn.hip) both recompute the conv head row by row,
// one thread per row, and send its gradients through the same fixed-order sums.
// Here, once: those sums, the per-row forward pieces with the pools' tie rule,
// the backward blocks of both convolutions and of pool 1, and the slab layout
// of the two conv passes with its map to the gradient vector.
// Included inside the sources' anonymous namespace after lnw_convhead.inc
// (conv1_ch, pool1_park, the packed layout). Device functions and constants
// only: the kernels, their launch chains and everything BatchNorm's statistics
// decide (DDQN: batch moments staged in LDS; MAPPO: the row's own, in double)
// stay in the two sources.
//
// Contraction: the build has -ffp-contract=off and a function does not inherit
// its caller's pragma, so every function below that multiplies and adds carries
// its own `fp contract(fast)`: all of them are called from fused blocks only.
// Each result bit depends on the order written here — the pool's tie rule, the
// wave sum's tree, the slab order — which is why there is one copy. Which
// multiply-adds the compiler then fuses also depends on what it packs into
// two-wide operations around them: after a change here, compare the kernels'
// fma / mul / add counts with the ones before.
// Still twice, in ql_forward_kernel and pl_conv2grad_kernel: pool 2's forward
// with the maximum's position (as a function it cost ql_forward_kernel<64> two
// more VGPRs).

constexpr int LEARN_THREADS = 128;  // rows per workgroup of the per-row passes
constexpr int LEARN_WAVES = LEARN_THREADS / WAVE;
static_assert(LEARN_WAVES == 2, "flush adds the staging rows of two waves");
constexpr int PARK = 45 * LEARN_THREADS;  // pooled conv1 maps, one column per thread
// LDS copy of the conv head's parameters: the packed 578, room behind them for
// 1 / sqrt(var + eps) of the 5 + 8 channels (DDQN's staged statistics), padded
// to whole quads
constexpr int CONV_LDS = (CONV_PARAMS + 5 + 8 + 3) & ~3;
static_assert(CONV_LDS == 592, "the kernels' LDS sizes are pinned by the resource tests");

// ---- slab layouts (floats per workgroup) of the two conv passes -----------------
constexpr int S4_C2W = 0, S4_C2B = 360, S4_B1W = 368, S4_B1B = 373, S4_N = 378;
// the tail only MAPPO's conv2 pass fills: convhead's and BN2's affine gradients
// (DDQN has summed them in its forward pass by then)
constexpr int S4_HW = S4_N, S4_HB = 474, S4_B2W = 486, S4_B2B = 494, S4_N_TAIL = 502;
constexpr int S5_C1W = 0, S5_C1B = 45, S5_N = 50;
enum { RED_CONV2 = 2, RED_CONV1 = 3 };  // (after the passes DDQN alone has)

// the slot in the packed conv-head layout that entry i of a conv pass's slab
// sums into; tail (a constant at both calls): the slab has S4's tail
__device__ __forceinline__ int conv_grad_slot(int pass, int i, bool tail) {
  if (pass == RED_CONV2)
    return i < S4_C2B   ? C2W + i
           : i < S4_B1W ? C2B + (i - S4_C2B)
           : i < S4_B1B ? B1W + (i - S4_B1W)
           : (!tail || i < S4_HW) ? B1B + (i - S4_B1B)
           : i < S4_HB  ? HW + (i - S4_HW)
           : i < S4_B2W ? HB + (i - S4_HB)
           : i < S4_B2B ? B2W + (i - S4_B2W)
                        : B2B + (i - S4_B2B);
  return i < S5_C1B ? C1W + i : C1B + (i - S5_C1B);
}

// the running statistics' slots of a gradient vector are zero: the conv1
// pass's waves of destinations i = 0 .. 7 write them
__device__ __forceinline__ void zero_running_slots(float *grad, int pass, int i) {
  if (pass == RED_CONV1 && i < 5) {
    grad[B1M + i] = 0.f;
    grad[B1V + i] = 0.f;
  }
  if (pass == RED_CONV1 && i < 8) {
    grad[B2M + i] = 0.f;
    grad[B2V + i] = 0.f;
  }
}

// ---- reductions ------------------------------------------------------------
__device__ __forceinline__ float dpp_add(float v, const int ctrl_sel) {
  // (ctrl_sel is a compile-time constant at every call)
  int x = __builtin_bit_cast(int, v), y;
  switch (ctrl_sel) {
    case 0: y = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xf, 0xf, false); break;   // quad_perm [1,0,3,2]
    case 1: y = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xf, 0xf, false); break;   // quad_perm [2,3,0,1]
    case 2: y = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, false); break;  // row_half_mirror
    default: y = __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, false); break; // row_mirror
  }
  return v + __builtin_bit_cast(float, y);
}

// sum over the wave's 64 lanes in a fixed order (all lanes active), wave-uniform
__device__ __forceinline__ float wave_sum(float v) {
  v = dpp_add(v, 0);
  v = dpp_add(v, 1);
  v = dpp_add(v, 2);
  v = dpp_add(v, 3);  // every lane: the sum of its row of 16
  const int x = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 0));
  const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 32));
  const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(x, 48));
  return (r0 + r1) + (r2 + r3);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the workgroup's sum of v into slot idx of its LDS staging [LEARN_WAVES][n]
__device__ __forceinline__ void accum(float *wsl, int n, int idx, float v) {
  const float s = wave_sum(v);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsl[(threadIdx.x / WAVE) * n + idx] = s;
}

__device__ __forceinline__ void flush(const float *wsl, int n, float *slab) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += LEARN_THREADS) slab[i] = wsl[i] + wsl[n + i];
}

// ---- per-row pieces ------------------------------------------------------------
__device__ __forceinline__ void load_win(const float *row, float (&win)[WIN]) {
  const f32x4 *r4 = (const f32x4 *)row;
#pragma unroll
  for (int j = 0; j < 12; j++) {
    const f32x4 q = r4[j];
    win[4 * j] = q[0];
    win[4 * j + 1] = q[1];
    win[4 * j + 2] = q[2];
    win[4 * j + 3] = q[3];
  }
  win[48] = row[48];
}

// first maximum of a window's four values in row-major order (strict >): the
// pools' tie rule, torch's max_pool2d's
__device__ __forceinline__ float first_max4(float a, float b, float c, float d, int &sel) {
  float best = a;
  sel = 0;
  if (b > best) { best = b; sel = 1; }
  if (c > best) { best = c; sel = 2; }
  if (d > best) { best = d; sel = 3; }
  return best;
}

// what follows the statistics (mean m, inv = 1 / sqrt(var + eps)) of conv1's
// channel c in the forward: BatchNorm's affine (g, b), ReLU, and the 2x2 pool
// into the thread's parked column pc
__device__ __forceinline__ void bn_relu_pool1(float (&v)[49], int c, float m, float inv, float g, float b,
                                              float *pc) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int i = 0; i < 49; i++) v[i] = fmaxf((v[i] - m) * inv * g + b, 0.f);
  pool1_park(v, c, pc, LEARN_THREADS);
}

// ---- conv backward blocks ---------------------------------------------------------
// conv2's backward for output maps c0 .. c0 + 3, dz their gradients (before the
// bias): the weight gradients into the workgroup's staging wsl [LEARN_WAVES][n]
// at S4_C2W, and the gradient to the pooled conv1 maps added into the thread's
// column pB; pA: the pooled conv1 maps themselves
__device__ __forceinline__ void conv2_bwd(const float *P, const float *pA, float *pB, int c0,
                                          const float (&dz)[4][9], float *wsl, int n) {
#pragma clang fp contract(fast)
#pragma unroll 1
  for (int ci = 0; ci < 5; ci++) {
    float pin[9], dp[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
      pin[k] = pA[(ci * 9 + k) * LEARN_THREADS];
      dp[k] = 0.f;
    }
#pragma unroll
    for (int co = 0; co < 4; co++) {
      const float *wt = P + C2W + ((c0 + co) * 5 + ci) * 9;
#pragma unroll
      for (int ki = 0; ki < 3; ki++)
#pragma unroll
        for (int kj = 0; kj < 3; kj++) {
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
              const int ii = i + ki - 1, jj = j + kj - 1;
              if (ii >= 0 && ii < 3 && jj >= 0 && jj < 3) {
                s += dz[co][i * 3 + j] * pin[ii * 3 + jj];
                dp[ii * 3 + jj] += wt[ki * 3 + kj] * dz[co][i * 3 + j];
              }
            }
          accum(wsl, n, S4_C2W + ((c0 + co) * 5 + ci) * 9 + ki * 3 + kj, s);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; k++) pB[(ci * 9 + k) * LEARN_THREADS] += dp[k];
  }
}

// through pool 1 and the ReLU for one conv1 channel: v its normalised map
// (v - mean) inv, g and b BatchNorm 1's affine, pBc the channel's 9 parked
// gradients. gy1 [9], rows rp floats apart, takes the gradient at each window's
// maximum where `valid`; pos1 the nine 2-bit places; t1, t2 = sum(gy),
// sum(gy xh): BatchNorm 1's backward sums.
// (The caller normalises: with that loop in here the compiler packs other
// multiplies of the MAPPO kernel differently and fuses 16 more of them.)
__device__ __forceinline__ void pool1_bwd(const float (&v)[49], float g, float b, const float *pBc, bool valid,
                                          float *gy1, long long rp, unsigned &pos1, float &t1, float &t2) {
#pragma clang fp contract(fast)
  t1 = 0.f;
  t2 = 0.f;
  pos1 = 0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int q = i * 3 + j, p0 = 2 * i * 7 + 2 * j;
      const float h0 = v[p0], h1 = v[p0 + 1], h2 = v[p0 + 7], h3 = v[p0 + 8];
      int sel;
      const float best = first_max4(fmaxf(h0 * g + b, 0.f), fmaxf(h1 * g + b, 0.f), fmaxf(h2 * g + b, 0.f),
                                    fmaxf(h3 * g + b, 0.f), sel);
      const float xh = sel == 0 ? h0 : sel == 1 ? h1 : sel == 2 ? h2 : h3;
      const float gy = best > 0.f ? pBc[q * LEARN_THREADS] : 0.f;
      t1 += gy;
      t2 += gy * xh;
      pos1 |= (unsigned)sel << (2 * q);
      if (valid) gy1[q * rp] = gy;
    }
}

// conv1's weight gradients of channel c (v: the gradient of its 7x7 map, win:
// the input window) into the staging wsl [LEARN_WAVES][S5_N]
__device__ __forceinline__ void conv1_wgrad(const float (&v)[49], const float (&win)[WIN], int c, float *wsl) {
#pragma clang fp contract(fast)
#pragma unroll
  for (int ki = 0; ki < 3; ki++)
#pragma unroll
    for (int kj = 0; kj < 3; kj++) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 7; i++)
#pragma unroll
        for (int j = 0; j < 7; j++) {
          const int ii = i + ki - 1, jj = j + kj - 1;
          if (ii >= 0 && ii < 7 && jj >= 0 && jj < 7) s += v[i * 7 + j] * win[ii * 7 + jj];
        }
      accum(wsl, S5_N, S5_C1W + c * 9 + ki * 3 + kj, s);
    }
}
