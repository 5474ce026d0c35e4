// DDQN replay on the device: the two kernels between QCollector's ring and the
// learner step (lnw_qnet_grad), around the keyed draw lnw_ppo_sample, which
// serves unchanged with the ring's priorities as its weights. include/lnw.h has
// the contracts.
//
//   lnw_replay_mark  the priority of the transitions one collector step wrote
//            into ring slot k: one thread per env writes priority[e][k], 1 or
//            the float32 sum of the ships' |reward|.
//   lnw_replay_pack  the drawn transitions as the learner's row tensors, in a
//            buffer of 32-bit words: state, next_state, action, reward, done,
//            every region on a 16-B boundary. One thread per 16 B of the
//            buffer; a slot this rank does not own, or whose row lies outside
//            its ring, and the padding are zero words, so the ranks' buffers
//            summed as integers hold every owner's bits. With src_rank NULL
//            every slot is owned: the local gather. One launch, every word
//            written once.
//
// The buffer has fewer than 2^31 words at every supported shape, so its side
// is indexed in 32 bits; a ring offset can pass 2^31 and is 64-bit. No atomics,
// no workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lnw.h"

namespace {

constexpr int RP_THREADS = 256;
constexpr int RP_MAX_RANKS = 64;

__global__ __launch_bounds__(RP_THREADS) void rp_mark_kernel(lnw_replay_mark_args a) {
  const long long e = (long long)blockIdx.x * RP_THREADS + threadIdx.x;
  if (e >= a.E) return;
  float p = 1.0f;
  if (a.reward) {
    const long long at = ((long long)a.k * a.E + e) * a.n;
    p = 0.0f;
    for (int i = 0; i < a.n; i++)
      p += fabsf(a.reward_f64 ? (float)((const double *)a.reward)[at + i] : ((const float *)a.reward)[at + i]);
  }
  a.priority[e * a.cap + a.k] = p;
}

struct RpPlan {     // in uint4s (16 B) of xbuf unless named words
  uint32_t q;       // one slot's n D floats
  uint32_t rows;    // state and next_state: 2 batch q
  uint32_t act;     // + action: batch n
  uint32_t rew;     // + reward, padded
  uint32_t total;   // + done, padded
  uint32_t bn;      // batch n
  uint32_t rw;      // words of one reward
  long long words;
};

bool rp_plan(long long batch, int n, int D, int reward_f64, RpPlan &p) {
  if (batch < 1 || batch > LNW_SAMPLE_MAX_BATCH || n < 1 || n > 16 || D % 4 || D < 49 || D > 101) return false;
  const long long bn = batch * n;
  p.q = (uint32_t)(n * D / 4);
  p.bn = (uint32_t)bn;
  p.rw = reward_f64 ? 2u : 1u;
  p.rows = (uint32_t)(2 * batch * p.q);
  p.act = p.rows + p.bn;
  p.rew = p.act + (uint32_t)((bn * p.rw + 3) / 4);
  p.total = p.rew + (uint32_t)((bn + 3) / 4);
  p.words = 4ll * p.total;
  return true;
}

// the ring position k E + e of slot s when this rank owns it and its row lies in this ring, else -1
__device__ __forceinline__ long long owned_at(const lnw_replay_pack_args &a, uint32_t s) {
  if (a.src_rank && a.src_rank[s] != a.rank) return -1;
  const long long r = a.row_out[s] - a.row_base;
  if (r < 0 || r >= a.E * a.cap) return -1;  // (never outside: keeps every read inside the ring)
  const long long e = r / a.cap;
  return (r - e * a.cap) * a.E + e;
}

__global__ __launch_bounds__(RP_THREADS) void rp_pack_kernel(lnw_replay_pack_args a, RpPlan p) {
  const uint32_t i = blockIdx.x * RP_THREADS + threadIdx.x;
  if (i >= p.total) return;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (i < p.rows) {
    const uint32_t half = p.rows >> 1;
    const bool next = i >= half;
    const uint32_t t = next ? i - half : i;
    const uint32_t s = t / p.q, j = t - s * p.q;
    const long long at = owned_at(a, s);
    if (at >= 0) v = ((const uint4 *)(next ? a.next_state : a.state))[at * p.q + j];
  } else if (i < p.act) {
    const uint32_t t = i - p.rows;
    const uint32_t s = t / (uint32_t)a.n, ship = t - s * (uint32_t)a.n;
    const long long at = owned_at(a, s);
    if (at >= 0) v = ((const uint4 *)a.action)[at * a.n + ship];
    // (batch n >= batch: these threads also cover the optional index)
    if (a.index_out && t < (uint32_t)a.batch) a.index_out[t] = owned_at(a, t);
  } else {
    const bool done = i >= p.rew;
    const uint32_t w0 = 4u * (i - (done ? p.rew : p.act));
    const uint32_t per = done ? 1u : p.rw;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int c = 0; c < 4; c++) {
      const uint32_t el = (w0 + c) / per, part = (w0 + c) - el * per;
      if (el >= p.bn) continue;  // padding
      const uint32_t s = el / (uint32_t)a.n, ship = el - s * (uint32_t)a.n;
      const long long at = owned_at(a, s);
      if (at < 0) continue;
      w[c] = done ? (uint32_t)a.done[at] : ((const uint32_t *)a.reward)[(at * a.n + ship) * per + part];
    }
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  ((uint4 *)a.xbuf)[i] = v;
}

}  // namespace

extern "C" {

int lnw_replay_mark(const lnw_replay_mark_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_replay_mark_args &a = *args;
  if (!a.priority || ((uintptr_t)a.priority & 3)) return LNW_EINVAL;
  if (a.reward && ((uintptr_t)a.reward & (a.reward_f64 ? 7 : 3))) return LNW_EINVAL;
  if (a.E < 1 || a.cap < 1 || a.k < 0 || a.k >= a.cap || a.E * a.cap >= (1ll << 31)) return LNW_EINVAL;
  if (a.n < 1 || a.n > 16) return LNW_EUNSUPPORTED;
  rp_mark_kernel<<<(unsigned)((a.E + RP_THREADS - 1) / RP_THREADS), RP_THREADS, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

int64_t lnw_replay_pack_words(int64_t batch, int32_t n, int32_t D, int32_t reward_f64) {
  RpPlan p;
  return rp_plan(batch, n, D, reward_f64, p) ? p.words : 0;
}

int lnw_replay_pack(const lnw_replay_pack_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_replay_pack_args &a = *args;
  if (!a.state || !a.next_state || !a.action || !a.reward || !a.done || !a.row_out || !a.xbuf) return LNW_EINVAL;
  RpPlan p;
  if (!rp_plan(a.batch, a.n, a.D, a.reward_f64, p) || a.rank < 0 || a.rank >= RP_MAX_RANKS) return LNW_EUNSUPPORTED;
  if (a.E < 1 || a.cap < 1 || a.E * a.cap >= (1ll << 31) || a.row_base < 0 ||
      a.row_base > (1ll << 40) - a.E * a.cap)
    return LNW_EINVAL;
  if (((uintptr_t)a.state | (uintptr_t)a.next_state | (uintptr_t)a.action | (uintptr_t)a.xbuf) & 15) return LNW_EINVAL;
  if (((uintptr_t)a.reward & (a.reward_f64 ? 7 : 3)) || ((uintptr_t)a.done & 3) || ((uintptr_t)a.src_rank & 3))
    return LNW_EINVAL;
  if (((uintptr_t)a.row_out | (uintptr_t)a.index_out) & 7) return LNW_EINVAL;
  if (a.xbuf_words < p.words) return LNW_EINVAL;
  rp_pack_kernel<<<(p.total + RP_THREADS - 1) / RP_THREADS, RP_THREADS, 0, (hipStream_t)stream>>>(a, p);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
