// Training over sharded rollouts: the two device steps between the ranks' local
// minibatch draws (lnw_ppo_sample) and the learner step (lnw_ppo_grad) that
// every rank then runs on the same rows. include/lnw.h has the contracts.
//
//   lnw_ppo_sample_merge  the first `batch` of the union of W ranks' candidate
//            lists in the total order (key, global row). Every list is already
//            ascending, so a candidate's position in the union is its position
//            in its own list plus, per other list, the number of elements that
//            precede it: one thread per candidate, one binary search per other
//            list, and the candidates that land below `batch` write their slot.
//            Global rows are distinct, so the order is strict, every slot has
//            exactly one writer and nothing depends on another workgroup.
//   lnw_ppo_rows_pack     the payload of every slot this rank owns (the row's
//            group of observations, actions, log-probabilities, rtg, old value)
//            into an exchange buffer of 32-bit words, zero words in the slots it
//            does not own: summed over the ranks as integers, the buffer holds
//            the owners' bits. Two launches, every word written once.
//
// Keys are non-negative doubles (lnw_ppo_sample stores a zero key as +0 and a
// non-finite row as +inf), which order like their bit patterns as unsigned
// 64-bit integers: the merge compares bits. No atomics, no workspace.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lnw.h"

namespace {

typedef unsigned long long u64;

constexpr int PD_THREADS = 256;
constexpr int PD_MAX_RANKS = 64;

__device__ __forceinline__ bool pair_before(u64 ka, int64_t ra, u64 kb, int64_t rb) {
  return ka < kb || (ka == kb && ra < rb);
}

__global__ __launch_bounds__(PD_THREADS) void pd_merge_kernel(lnw_ppo_merge_args a) {
  const long long i = (long long)blockIdx.x * PD_THREADS + threadIdx.x;
  const long long B = a.batch;
  if (i == 0) {
    int64_t bad = 0;
    for (int w = 0; w < a.W; w++) bad += a.lists[(long long)w * a.stride + 2 * B];
    a.status_out[0] = bad;
  }
  if (i >= (long long)a.W * B) return;
  const int w = (int)(i / B);
  const long long p = i - (long long)w * B;
  const int64_t *mine = a.lists + (long long)w * a.stride;
  const u64 key = (u64)mine[p];
  const int64_t row = mine[B + p];
  long long pos = p;
  for (int v = 0; v < a.W && pos < B; v++) {
    if (v == w) continue;
    const int64_t *other = a.lists + (long long)v * a.stride;
    // the number of list v's elements before (key, row): the first index whose element is not
    long long lo = 0, hi = B;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (pair_before((u64)other[mid], other[B + mid], key, row)) lo = mid + 1;
      else hi = mid;
    }
    pos += lo;
  }
  if (pos >= B) return;
  a.key_out[pos] = __builtin_bit_cast(double, key);
  a.row_out[pos] = row;
  a.src_rank[pos] = w;
  a.src_pos[pos] = (int32_t)p;
  a.index_out[pos] = pos * a.n + row % a.n;
}

struct PackPlan {
  long long q;      // float4s of one slot's group of observations
  long long bpad;   // batch rounded up to 4 words
  long long o_act, o_lp, o_rtg, o_val, words;
};

bool pack_plan(long long batch, int n, int D, PackPlan &p) {
  if (batch < 1 || batch > LNW_SAMPLE_MAX_BATCH || n < 1 || n > 16 || D % 4 || D < 49 || D - 37 > 64) return false;
  p.q = (long long)n * D / 4;
  p.bpad = (batch + 3) & ~3ll;
  p.o_act = batch * p.q * 4;
  p.o_lp = p.o_act + 4 * batch;
  p.o_rtg = p.o_lp + 4 * batch;
  p.o_val = p.o_rtg + p.bpad;
  p.words = p.o_val + p.bpad;
  return true;
}

// the local row of slot s when this rank owns it and the row lies in its shard, else -1
__device__ __forceinline__ long long owned_row(const lnw_ppo_pack_args &a, long long s) {
  if (a.src_rank[s] != a.rank) return -1;
  const long long r = a.row_out[s] - a.row_base;
  return r >= 0 && r < a.rows ? r : -1;  // (never outside: keeps every read inside the arrays)
}

// xobs: one thread per float4 of [batch][n][D]
__global__ __launch_bounds__(PD_THREADS) void pd_pack_obs_kernel(lnw_ppo_pack_args a, PackPlan p) {
  const long long i = (long long)blockIdx.x * PD_THREADS + threadIdx.x;
  if (i >= a.batch * p.q) return;
  const long long s = i / p.q, j = i - s * p.q;
  const long long r = owned_row(a, s);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (r >= 0) v = ((const uint4 *)a.obs)[(r / a.n) * p.q + j];
  ((uint4 *)a.xbuf)[i] = v;
}

// the per-row fields: one thread per slot, and the padding words behind rtg and old_values
__global__ __launch_bounds__(PD_THREADS) void pd_pack_rows_kernel(lnw_ppo_pack_args a, PackPlan p) {
  const long long s = (long long)blockIdx.x * PD_THREADS + threadIdx.x;
  if (s >= p.bpad) return;
  uint4 act = make_uint4(0u, 0u, 0u, 0u), lp = act;
  uint32_t rtg = 0u, val = 0u;
  if (s < a.batch) {
    const long long r = owned_row(a, s);
    if (r >= 0) {
      act = ((const uint4 *)a.actions)[r];
      lp = ((const uint4 *)a.log_probs)[r];
      rtg = ((const uint32_t *)a.rtg)[r];
      val = ((const uint32_t *)a.values)[r / a.n];
    }
    ((uint4 *)(a.xbuf + p.o_act))[s] = act;
    ((uint4 *)(a.xbuf + p.o_lp))[s] = lp;
  }
  a.xbuf[p.o_rtg + s] = rtg;
  a.xbuf[p.o_val + s] = val;
}

}  // namespace

extern "C" {

int lnw_ppo_sample_merge(const lnw_ppo_merge_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_ppo_merge_args &a = *args;
  if (!a.lists || !a.key_out || !a.row_out || !a.src_rank || !a.src_pos || !a.index_out || !a.status_out)
    return LNW_EINVAL;
  if (a.W < 1 || a.W > PD_MAX_RANKS || a.batch < 1 || a.batch > LNW_SAMPLE_MAX_BATCH) return LNW_EUNSUPPORTED;
  if (a.n < 1 || a.stride < 2 * a.batch + 1) return LNW_EINVAL;
  if (((uintptr_t)a.lists | (uintptr_t)a.key_out | (uintptr_t)a.row_out | (uintptr_t)a.index_out |
       (uintptr_t)a.status_out) & 7)
    return LNW_EINVAL;
  if (((uintptr_t)a.src_rank | (uintptr_t)a.src_pos) & 3) return LNW_EINVAL;
  const long long items = (long long)a.W * a.batch;
  pd_merge_kernel<<<(unsigned)((items + PD_THREADS - 1) / PD_THREADS), PD_THREADS, 0, (hipStream_t)stream>>>(a);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

int64_t lnw_ppo_pack_words(int64_t batch, int32_t n, int32_t D) {
  PackPlan p;
  return pack_plan(batch, n, D, p) ? p.words : 0;
}

int lnw_ppo_rows_pack(const lnw_ppo_pack_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_ppo_pack_args &a = *args;
  if (!a.obs || !a.actions || !a.log_probs || !a.rtg || !a.values || !a.row_out || !a.src_rank || !a.xbuf)
    return LNW_EINVAL;
  PackPlan p;
  if (!pack_plan(a.batch, a.n, a.D, p)) return LNW_EUNSUPPORTED;
  if (a.rank < 0 || a.rank >= PD_MAX_RANKS || a.rows < 1 || a.rows % a.n || a.row_base < 0 || a.row_base % a.n ||
      a.row_base > (1ll << 40) - a.rows)
    return LNW_EINVAL;
  if (((uintptr_t)a.obs | (uintptr_t)a.actions | (uintptr_t)a.log_probs | (uintptr_t)a.xbuf) & 15) return LNW_EINVAL;
  if (((uintptr_t)a.rtg | (uintptr_t)a.values | (uintptr_t)a.src_rank) & 3) return LNW_EINVAL;
  if ((uintptr_t)a.row_out & 7) return LNW_EINVAL;
  if (a.xbuf_words < p.words) return LNW_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const long long items = a.batch * p.q;
  pd_pack_obs_kernel<<<(unsigned)((items + PD_THREADS - 1) / PD_THREADS), PD_THREADS, 0, st>>>(a, p);
  pd_pack_rows_kernel<<<(unsigned)((p.bpad + PD_THREADS - 1) / PD_THREADS), PD_THREADS, 0, st>>>(a, p);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
