// lnw_qhead.inc — the three linear heads of the reference Q-network
// (network.py:292-305, DMLP.forward: radar 2, attack 5, movement 50 outputs of
// relu(W x + b) over x = [conv head (12), obs[49:]]) as the acting kernel
// (lnw_qnet.hip) and the learner (lnw_qlearn.hip) both read them: W [57][n_in]
// and b [57] behind the conv head's block in BatchedQNet.packed(), staged in
// LDS with the weight rows zero-padded to NI columns so a row is read as float4
// broadcasts. Included inside their anonymous namespace after lnw_convhead.inc
// (CONV_PARAMS) and their f32x4 typedef.

constexpr int Q_RAD = 2, Q_ATK = 5, Q_MOV = 50, Q_OUT = Q_RAD + Q_ATK + Q_MOV;  // 57
constexpr int BIAS_PAD = (Q_OUT + 3) & ~3;  // the LDS bias block, 16-B aligned behind it

// head weights zero-padded to NI columns, and biases, into LDS; step: the
// workgroup's thread count
template <int NI>
__device__ __forceinline__ void stage_heads(float *Wl, float *bl, const float *params, int n_in, int step) {
  for (int i = threadIdx.x; i < Q_OUT * NI; i += step) {
    const int o = i / NI, k = i - o * NI;
    Wl[i] = k < n_in ? params[CONV_PARAMS + o * n_in + k] : 0.f;
  }
  for (int i = threadIdx.x; i < Q_OUT; i += step) bl[i] = params[CONV_PARAMS + Q_OUT * n_in + i];
}

// W[o] . x + b[o] from the LDS copy: four chains, k = 0, 1, 2, 3 mod 4
template <int NI>
__device__ __forceinline__ float head_dot(const float *Wl, const float *bl, const float (&x)[NI], int o) {
  const f32x4 *w = (const f32x4 *)(Wl + o * NI);
  float s0 = bl[o], s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
  for (int k4 = 0; k4 < NI / 4; k4++) {
    const f32x4 wv = w[k4];
    s0 = fmaf(wv[0], x[4 * k4], s0);
    s1 = fmaf(wv[1], x[4 * k4 + 1], s1);
    s2 = fmaf(wv[2], x[4 * k4 + 2], s2);
    s3 = fmaf(wv[3], x[4 * k4 + 3], s3);
  }
  return (s0 + s1) + (s2 + s3);
}
