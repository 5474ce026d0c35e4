// Fused DDQN acting step (lnw_qnet_act): for every row of one side's
// observation block, the reference Q-network forward (network.py:246-305, DMLP:
// the actor's conv head, then x = [head(12), obs[49:]] — no LayerNorm — into
// three linear heads with bias and ReLU: radar 2, attack 5, movement 50) and
// what the DDQN loop does with it per ship and step (ddqn.py:286-387): the
// epsilon-greedy choice between [argmax radar, argmax attack, argmax movement]
// and a uniform random row, or untrained red's random rows (ddqn.py:316-328),
// written as the int32 action rows lnw_step takes in DISCRETE mode.
//
// One thread per row, as features_kernel. The packed parameters
// (BatchedQNet.packed(): the conv head's 578 floats in lnw_actor_features'
// order, W [57][n_in] with the rows in radar, attack, movement order, b [57])
// are staged once per workgroup in LDS, the weight rows zero-padded to NI
// columns so a row is read as float4 broadcasts. The 57 outputs are streamed:
// each is reduced, ReLU'd, optionally stored (q_out) and folded into its head's
// running first maximum (strict >, so ties keep the lower index as torch.argmax
// does; a NaN beats every number and the first NaN wins, as torch's argmax
// orders them) — no 57-wide register array.
//
// Keyed draws (keyed_normal's convention, lnw/rollout.py): the four uniforms of
// global row g = row_base + e * n + i are one Philox block at counter
// (slot << 38) + g, i.e. what lnw_fill_uniform_f32(seed, offset = (slot << 40)
// + 4 g) yields, so shards of the envs draw what one call over all envs draws.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "lnw.h"
#include "lnw_device.h"

namespace {

using namespace lnw;

typedef int i32x4 __attribute__((ext_vector_type(4)));

#include "lnw_convhead.inc"
#include "lnw_qhead.inc"

constexpr int QN_THREADS = 256;
constexpr int CONV_PAD = (CONV_PARAMS + 3) & ~3;  // 16-B aligned weight rows behind the conv block

extern __shared__ float qnet_lds[];

// the four keyed uniforms of a global row (lnw_fill_uniform_f32's block)
__device__ __forceinline__ void keyed_u4(unsigned long long seed, unsigned long long slot, long long grow,
                                         float (&u)[4]) {
  philox_u4(seed, (slot << 38) + (unsigned long long)grow, u);
}

// One head: outputs o0 .. o0 + cnt - 1 of relu(W x + b), streamed; returns the
// first maximal index (torch.argmax).
template <int NI>
__device__ __forceinline__ int q_head(const float *Wl, const float *bl, const float (&x)[NI], int o0, int cnt,
                                      float *qo) {
  float best = 0.f;
  int bi = 0;
#pragma unroll 1
  for (int j = 0; j < cnt; j++) {
    const int o = o0 + j;
    const float s = head_dot<NI>(Wl, bl, x, o);
    const float q = s < 0.f ? 0.f : s;  // relu: a NaN stays a NaN (torch.relu)
    if (qo) qo[o] = q;
    const bool better = j == 0 || q > best || (q != q && best == best);
    best = better ? q : best;
    bi = better ? j : bi;
  }
  return bi;
}

template <int NI>
__global__ __launch_bounds__(QN_THREADS, 2) void qnet_act_kernel(lnw_qnet_args a, int n_in) {
  float *P = qnet_lds;                         // [578] conv head parameters
  float *Wl = qnet_lds + CONV_PAD;             // [57][NI] head weights, zero past n_in
  float *bl = Wl + Q_OUT * NI;                 // [57] biases
  // pooled conv1 maps: per wave [45][64], one column per lane (as features_kernel)
  float *pool1 = bl + BIAS_PAD + (threadIdx.x / WAVE) * 45 * WAVE + (threadIdx.x & (WAVE - 1));
  for (int i = threadIdx.x; i < CONV_PARAMS; i += blockDim.x) P[i] = a.params[i];
  stage_heads<NI>(Wl, bl, a.params, n_in, blockDim.x);
  __syncthreads();
  const int n = a.n, D = a.D;
  const long long rows = a.E * n;
  const long long r = (long long)blockIdx.x * QN_THREADS + threadIdx.x;
  if (r >= rows) return;
  // (32-bit: rows < 2^31, checked on the host)
  const long long istride = a.obs_in_env_stride ? a.obs_in_env_stride : (long long)n * D;
  float x[NI];
  {
    float h[12];
    const int e = (int)r / n, i = (int)r - e * n;
    conv_head_row(P, a.obs + (long long)e * istride + (long long)i * D, pool1, WAVE, a.bn_running != 0, h);
#pragma unroll
    for (int k = 0; k < 12; k++) x[k] = h[k];
  }
  // the row's env and ship again from an opaque copy of the row index, so no
  // address lives across the head (policy_act_kernel does the same)
  int r_o = (int)(blockIdx.x * QN_THREADS + threadIdx.x);
  asm volatile("" : "+v"(r_o));
  const int e = r_o / n, i = r_o - e * n;
  {
    // x[12 ..] = obs[49 .. D - 1] (16-B aligned rows of D % 4 == 0 floats, checked
    // on the host), zeros past n_in
    float tl[NI - 12];
    const int D4 = D >> 2;
    load_tail_q(a.obs + (long long)e * istride + (long long)i * D, D4, tl);
#pragma unroll
    for (int k = 12; k < NI; k++) x[k] = k < n_in ? tl[k - 12] : 0.f;
  }
  float *qo = a.q_out ? a.q_out + (long long)r_o * Q_OUT : nullptr;
  int act[3];
  act[0] = q_head<NI>(Wl, bl, x, 0, Q_RAD, qo);
  act[1] = q_head<NI>(Wl, bl, x, Q_RAD, Q_ATK, qo);
  act[2] = q_head<NI>(Wl, bl, x, Q_RAD + Q_ATK, Q_MOV, qo);
  // ---- epsilon-greedy (ddqn.py:299-308) --------------------------------------
  float u[4];
  keyed_u4(a.seed, a.slot, a.row_base + r_o, u);
  const float eps = a.eps_env ? a.eps_env[e] : a.eps;
  const bool explore = u[0] < eps;
  if (explore) {
    act[0] = (int)(u[1] * 2.f);
    act[1] = (int)(u[2] * 5.f);
    act[2] = (int)(u[3] * 50.f);
  }
  // ---- outputs: sunk ships and ended envs act [0, 0, 0] (ddqn.py:312) --------
  const bool keep = a.alive[(long long)(a.own0 + i) * a.E + e] != 0 && (!a.live || a.live[e] != 0);
  const i32x4 v = keep ? i32x4{act[0], act[1], act[2], 0} : i32x4{0, 0, 0, 0};
  if (a.full) *(i32x4 *)(a.full + ((long long)e * a.A + a.own0 + i) * 4) = v;
  if (a.act_out) *(i32x4 *)(a.act_out + (long long)e * a.act_env_stride + 4 * i) = v;
  if (a.explored) a.explored[r_o] = (keep && explore) ? 1 : 0;
}

// Untrained red (ddqn.py:316-328): no network. Before episode step 20 the row is
// [randint(0,1), randint(0,1), randint(2,4)]; from then on [randint(0,1), msl,
// randint(0,49)] with msl = randint(1,4) if random() < RED_AGGRESSION and the
// ship has targets, else 0.
__global__ __launch_bounds__(QN_THREADS) void qnet_red_random_kernel(lnw_qnet_args a) {
  const long long rows = a.E * a.n;
  const long long r = (long long)blockIdx.x * QN_THREADS + threadIdx.x;
  if (r >= rows) return;
  const int e = (int)r / a.n, i = (int)r - e * a.n;
  const long long ag = (long long)(a.own0 + i) * a.E + e;
  float u[4];
  keyed_u4(a.seed, a.slot, a.row_base + r, u);
  int act[3];
  act[0] = (int)(u[0] * 2.f);
  if (a.t < 20) {
    act[1] = (int)(u[1] * 2.f);
    act[2] = 2 + (int)(u[2] * 3.f);
  } else {
    act[1] = (u[1] < a.red_aggression && a.tl_cnt[ag] > 0) ? 1 + (int)(u[2] * 4.f) : 0;
    act[2] = (int)(u[3] * 50.f);
  }
  const bool keep = a.alive[ag] != 0 && (!a.live || a.live[e] != 0);
  const i32x4 v = keep ? i32x4{act[0], act[1], act[2], 0} : i32x4{0, 0, 0, 0};
  if (a.full) *(i32x4 *)(a.full + ((long long)e * a.A + a.own0 + i) * 4) = v;
  if (a.act_out) *(i32x4 *)(a.act_out + (long long)e * a.act_env_stride + 4 * i) = v;
  if (a.explored) a.explored[r] = keep ? 1 : 0;
}

}  // namespace

extern "C" {

int lnw_qnet_act(const lnw_qnet_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_qnet_args &a = *args;
  if (a.mode != LNW_QNET_EPS_GREEDY && a.mode != LNW_QNET_RED_RANDOM) return LNW_EINVAL;
  const bool net = a.mode == LNW_QNET_EPS_GREEDY;
  if (!a.alive || a.n <= 0 || a.E < 0 || a.A <= 0 || a.own0 < 0 || a.own0 + a.n > a.A) return LNW_EINVAL;
  if (net && (!a.obs || !a.params)) return LNW_EINVAL;
  if (!net && (!a.tl_cnt || a.q_out)) return LNW_EINVAL;  // (no Q-values without a network)
  if (a.obs_in_env_stride < 0 || (a.obs_in_env_stride && (a.obs_in_env_stride < (int64_t)a.n * a.D ||
                                                          (a.obs_in_env_stride & 3))))
    return LNW_EINVAL;
  // 16-B aligned rows for the vector loads and stores
  if ((net && ((uintptr_t)a.obs & 15)) || (a.full && ((uintptr_t)a.full & 15)) ||
      (a.act_out && (((uintptr_t)a.act_out & 15) || (a.act_env_stride & 3) || a.act_env_stride < (int64_t)a.n * 4)))
    return LNW_EINVAL;
  if (!obs_width_ok(a.D, net)) return LNW_EUNSUPPORTED;  // (no row is read without a network)
  const long long rows = a.E * a.n;
  if (rows + QN_THREADS >= (1ll << 31)) return LNW_EUNSUPPORTED;  // (32-bit row indices)
  if (a.E == 0) return 0;
  const unsigned blocks = (unsigned)((rows + QN_THREADS - 1) / QN_THREADS);
  if (!net) {
    qnet_red_random_kernel<<<blocks, QN_THREADS, 0, (hipStream_t)stream>>>(a);
    return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
  }
  const int n_in = a.D - WIN + 12;
  const int NI = n_in <= 32 ? 32 : MAX_IN;
  const size_t lds = (size_t)(CONV_PAD + Q_OUT * NI + BIAS_PAD + 45 * QN_THREADS) * sizeof(float);
  if (NI == 32)
    qnet_act_kernel<32><<<blocks, QN_THREADS, lds, (hipStream_t)stream>>>(a, n_in);
  else
    qnet_act_kernel<MAX_IN><<<blocks, QN_THREADS, lds, (hipStream_t)stream>>>(a, n_in);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
