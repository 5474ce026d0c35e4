// Parameter-noise exploration (ppo.py:452-482): lnw_actor_perturb writes, for a
// range of population members, the packed parameter set the policy kernel reads
// (BatchedActor.packed_policy()'s format) from the flat actor vector of the
// learner, with member m's keyed noise theta + mask * clamp(sigma z_m, -c, +c)
// added on the way. include/lnw.h has both layouts, the mask and the draws.
//
// One launch, one thread per 16 B of a member's set: a float4 of the conv head
// / LayerNorm block or of the biases, or one lane's eight weights of an MFMA
// fragment, which the thread splits into the three bfloat16 planes (the split
// mlp_layer3 undoes: w = hi + mid + lo exactly) and stores as three 16-B
// vectors. Every output word of a set is written by exactly one thread and
// every value is a pure function of (theta, seed, slot, member, flat index): no
// atomics, bitwise reproducible, and a range of members split over several
// calls gets the same bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lnw.h"
#include "lnw_device.h"

namespace {

using namespace lnw;

// the conv head block's layout (C1W .. CONV_PARAMS, obs_width_ok) and the two
// parameter layouts (policy_pack, actor_flat)
#include "lnw_convhead.inc"
#include "lnw_policypack.inc"

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int PN_THREADS = 256;

struct PerturbArgs {
  lnw_actor_perturb_args a;
  PolicyPack pk;
  ActorFlat fl;
  int k1;      // fc1's padded input width (32 or 64)
  int items;   // 16-B work items of one member's set
  int chunks;  // blocks per member
};

// the noise mask by flat index: conv1, conv2, convhead, the MLP and the heads;
// not the BatchNorms (their running statistics included), the LayerNorm, logstd
__device__ __forceinline__ bool noised(int k, const ActorFlat &fl) {
  if (k < CONV_PARAMS) return k < B1W || (k >= C2W && k < B2W) || k >= HW;
  return k >= fl.fc1w && k < fl.logstd;
}

__device__ __forceinline__ float pick4(const float (&u)[4], unsigned c) {
  return c == 0 ? u[0] : c == 1 ? u[1] : c == 2 ? u[2] : u[3];
}

// one member's parameters by flat index
struct Member {
  const float *theta;
  bool on;                  // noise: sigma != 0
  float sigma, clip;
  unsigned long long seed;
  unsigned long long base;  // index of the member's first uniform: (slot << 40) + 2 P m
  int P;

  // theta_m[k]: the uniforms at base + k (radius) and base + P + k (angle) of
  // the stream lnw_fill_uniform_f32 writes, four per Philox block
  __device__ __forceinline__ float at(int k, const ActorFlat &fl) const {
    const float v = theta[k];
    if (!on || !noised(k, fl)) return v;
    const unsigned long long i0 = base + (unsigned long long)k, i1 = i0 + (unsigned long long)P;
    float u0[4], u1[4];
    philox_u4(seed, i0 >> 2, u0);
    philox_u4(seed, i1 >> 2, u1);
    const float nz = sigma * box_muller(pick4(u0, (unsigned)i0 & 3u), pick4(u1, (unsigned)i1 & 3u));
    return v + fminf(fmaxf(nz, -clip), clip);
  }
};

__global__ __launch_bounds__(PN_THREADS) void actor_perturb_kernel(PerturbArgs pa) {
  const lnw_actor_perturb_args &a = pa.a;
  const ActorFlat &fl = pa.fl;
  const int k = blockIdx.x / pa.chunks;  // the block's member (local)
  const int it = (blockIdx.x - k * pa.chunks) * PN_THREADS + threadIdx.x;
  if (it >= pa.items) return;
  Member M;
  M.theta = a.theta + (long long)k * a.theta_member_stride;
  M.sigma = a.noise_dev ? a.noise_dev[0] : 0.f;
  M.clip = a.noise_dev ? a.noise_dev[1] : 0.f;
  M.on = M.sigma != 0.f;
  M.seed = a.seed;
  M.P = fl.size;
  const unsigned long long call = a.call_dev ? (unsigned long long)*a.call_dev : 0ull;
  const unsigned long long slot = call * (unsigned long long)a.T * 4ull + 3ull;
  M.base = (slot << 40) + (unsigned long long)(a.member0 + k) * 2ull * (unsigned long long)fl.size;
  float *out = a.packed_out + (long long)k * a.member_stride;

  const int n_conv = pa.pk.off_b1 / 4, n_bias = (FC1 + FC2 + FC3) / 4;
  if (it < n_conv + n_bias) {
    // a float4 of the conv head / LayerNorm block (same order in both layouts,
    // zeros past its end) or of b1 | b2 | b3
    int o = 4 * it, f = 4 * it, end = pa.pk.n_par;
    if (it >= n_conv) {
      const int q = 4 * (it - n_conv);
      o = pa.pk.off_b1 + q;
      f = q < FC1 ? fl.fc1b + q : q < FC1 + FC2 ? fl.fc2b + (q - FC1) : fl.fc3b + (q - FC1 - FC2);
      end = fl.size;
    }
    f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = f + c < end ? M.at(f + c, fl) : 0.f;
    *(f32x4 *)(out + o) = v;
    return;
  }
  // one lane's eight weights of a fragment: layer, n-tile nt, k-pair p, lane
  int f = it - n_conv - n_bias;
  const int n1 = 4 * (pa.k1 / 32) * WAVE, n2 = 4 * 2 * WAVE, n3 = 2 * 2 * WAVE;
  int qp, rows, cols, w0, tiles, base;  // k-pairs, W's shape and flat offset, n-tiles, first bf16x8
  if (f < n1) {
    qp = pa.k1 / 32, rows = FC1, cols = pa.pk.n_in, w0 = fl.fc1w, tiles = 4, base = 0;
  } else if (f < n1 + n2) {
    f -= n1, qp = 2, rows = FC2, cols = FC1, w0 = fl.fc2w, tiles = 4, base = 3 * n1;
  } else if (f < n1 + n2 + n3) {
    f -= n1 + n2, qp = 2, rows = FC3, cols = FC2, w0 = fl.fc3w, tiles = 2, base = 3 * (n1 + n2);
  } else {  // normal head rows 0-3, log-std head rows 4-7 (adjacent in the flat vector)
    f -= n1 + n2 + n3, qp = 1, rows = 2 * NOUT, cols = FC3, w0 = fl.heads, tiles = 1, base = 3 * (n1 + n2 + n3);
  }
  const int lane = f & (WAVE - 1), p = (f / WAVE) % qp, nt = f / (WAVE * qp);
  const int row = 16 * nt + (lane & 15);
  bf16x8 hi, mid, lo;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int col = 32 * p + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
    const float x = (row < rows && col < cols) ? M.at(w0 + row * cols + col, fl) : 0.f;
    const __bf16 h = (__bf16)x;
    const float r = x - (float)h;
    const __bf16 m = (__bf16)r;
    hi[j] = h;
    mid[j] = m;
    lo[j] = (__bf16)(r - (float)m);
  }
  bf16x8 *F = (bf16x8 *)(out + pa.pk.off_w1) + base;
  const int plane = tiles * qp * WAVE;
  F[f] = hi;
  F[plane + f] = mid;
  F[2 * plane + f] = lo;
}

}  // namespace

extern "C" {

int64_t lnw_policy_packed_floats(int32_t D) { return obs_width_ok(D, true) ? policy_pack(D).floats : 0; }

int lnw_actor_perturb(const lnw_actor_perturb_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_actor_perturb_args &a = *args;
  if (!a.theta || !a.packed_out || a.members < 0 || a.member0 < 0) return LNW_EINVAL;
  if (!obs_width_ok(a.D, true)) return LNW_EUNSUPPORTED;
  PerturbArgs pa;
  pa.a = a;
  pa.pk = policy_pack(a.D);
  pa.fl = actor_flat(pa.pk.n_in);
  if (a.member_stride < pa.pk.floats || (a.member_stride & 3) || ((uintptr_t)a.packed_out & 15)) return LNW_EINVAL;
  if (a.theta_member_stride < 0 || (a.theta_member_stride && a.theta_member_stride < pa.fl.size)) return LNW_EINVAL;
  if (a.noise_dev && a.T <= 0) return LNW_EINVAL;
  // a member's 2 P uniforms lie below the slot's bits (slot << 40)
  const long long per = 2ll * pa.fl.size;
  if (a.members > (1ll << 40) / per || a.member0 > (1ll << 40) / per - a.members) return LNW_EINVAL;
  if (a.members == 0) return 0;
  pa.k1 = pa.pk.n_in <= 32 ? 32 : MAX_IN;
  // float4s up to the fragments, then one item per 16 B of a plane (three planes)
  pa.items = pa.pk.off_w1 / 4 + (pa.pk.floats - pa.pk.off_w1) / 12;
  pa.chunks = (pa.items + PN_THREADS - 1) / PN_THREADS;
  const long long blocks = a.members * pa.chunks;
  if (blocks >= (1ll << 31)) return LNW_EUNSUPPORTED;
  actor_perturb_kernel<<<(unsigned)blocks, PN_THREADS, 0, (hipStream_t)stream>>>(pa);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
