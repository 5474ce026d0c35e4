// MAPPO minibatch draw (lnw_ppo_sample): the learner's prioritised sampler
// (ppo.py:311-319, torch.multinomial without replacement on |rtg| + 1e-5) as a
// keyed draw on the device. Sequential weighted sampling without replacement is
// "the B smallest keys e_r / w_r, e_r ~ Exp(1), in ascending order"; the key of a
// row is a pure function of (seed, slot, global row) (include/lnw.h has the
// definition), so the draw is an exact selection and a sort, not a simulation.
//
// Non-negative doubles order like their bit patterns as unsigned 64-bit
// integers, so everything below works on the keys' bits. One algorithm for every
// batch size, a chain of plain launches:
//
//   init     zeroes the histograms and the counters, pads the candidate arrays
//   hist x 5 most-significant-digit radix select of the batch-th smallest key:
//            digits of 12 (sign and exponent), 13, 13, 13, 13 bits. The first
//            pass computes the keys and stores them (8 B per row: a key is a
//            Philox block, a polynomial log and three double divisions; the later
//            passes stream them at the memory rate instead) and keeps each
//            chunk's smallest key; a later pass counts only the keys under the
//            prefix chosen so far. Each workgroup counts its chunk of rows in LDS
//            and adds its non-empty bins to one of 8 copies of the level's
//            histogram. A later pass, the count and the compaction leave a chunk
//            alone whose smallest key lies above the prefix / above T: at a small
//            batch that is most chunks
//   pick x 5 one workgroup after each pass: sums the copies, finds the digit in
//            which the remaining rank falls, extends the prefix. After the
//            fifth the prefix is the threshold key T itself, and the remaining
//            rank is how many rows of key == T the batch takes
//   count    per workgroup: rows with key < T and key == T, into a slab
//   compact  each workgroup sums the slab before it and writes its rows, in row
//            order, to the candidate arrays: key < T first, then the rows of key
//            == T behind all of them, lowest rows first, up to the batch size
//   sort     bitonic sort of the candidates by (key, row), padded to a power of
//            two: a tile of 2048 in LDS per workgroup for every stride inside a
//            tile, one launch per stride above
//   gather   index, keys, the gathered columns, the status, the counter
//
// The only atomics are integer adds into counts (LDS histograms, the histogram
// copies, the non-finite count) and an integer minimum (a chunk's smallest
// key): results that no arrival order changes. The compaction places every row
// by counts alone (ballot ranks in a wave, the slab across workgroups), and the
// final order is the sort's: results are bitwise equal from run to run and
// under graph replay.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lnw.h"
#include "lnw_device.h"

namespace {

using namespace lnw;

typedef unsigned long long u64;

constexpr int PS_THREADS = 256;
constexpr int PS_MAX_WG = 2048;    // workgroups over the rows (a chunk is a multiple of 256 rows)
constexpr int PS_LEVELS = 5;
constexpr int PS_BINS = 8192;      // 13-bit digits (level 0: 12 bits, 4096 bins)
constexpr int PS_COPIES = 8;       // copies of each level's histogram (workgroup b adds to copy b % 8)
constexpr int PS_TILE = 2048;      // candidates sorted in LDS by one workgroup (24 KiB; 4096 leaves 32 workgroups
                                   // at the largest batch and measured slower)
constexpr int PS_SORT_THREADS = 1024;
constexpr int PS_PICK_THREADS = 1024;
constexpr u64 PS_INF = 0x7FF0000000000000ull;
constexpr u64 PS_PAD = ~0ull;

__host__ __device__ inline int level_shift(int level) { return level == 0 ? 52 : 52 - 13 * level; }
__host__ __device__ inline int level_bins(int level) { return level == 0 ? 4096 : PS_BINS; }

struct Sel { u64 prefix, k_rem; };  // the key bits chosen so far, the rank still to place among the keys under them

struct SampleWs {
  u64 *keys;          // [rows]
  uint32_t *hist;     // [PS_LEVELS][PS_COPIES][PS_BINS]
  Sel *sel;           // [PS_LEVELS + 1]
  u64 *nonfinite;     // [1]
  u64 *cmin;          // [workgroups] the smallest key of each workgroup's chunk
  uint32_t *slab;     // [workgroups][2] rows with key < T, key == T
  u64 *ckeys;         // [P]
  uint32_t *crows;    // [P]
  long long chunk;    // rows per workgroup
  long long P;        // batch rounded up to a power of two
};

struct Plan {
  long long chunk, P, bytes;
  long long o_hist, o_sel, o_nf, o_cmin, o_slab, o_ckeys, o_crows;
  int nwg;
};

bool make_plan(long long rows, long long batch, Plan &p) {
  if (rows < 1 || rows >= (1ll << 31) || batch < 1 || batch > rows || batch > LNW_SAMPLE_MAX_BATCH) return false;
  const long long per = (rows + PS_MAX_WG - 1) / PS_MAX_WG;
  p.chunk = (per + PS_THREADS - 1) / PS_THREADS * PS_THREADS;
  p.nwg = (int)((rows + p.chunk - 1) / p.chunk);
  p.P = 1;
  while (p.P < batch) p.P <<= 1;
  auto up = [](long long b) { return (b + 15) & ~15ll; };
  long long o = up(rows * 8);
  p.o_hist = o;
  o += up((long long)PS_LEVELS * PS_COPIES * PS_BINS * 4);
  p.o_sel = o;
  o += up((PS_LEVELS + 1) * (long long)sizeof(Sel));
  p.o_nf = o;
  o += 16;
  p.o_cmin = o;
  o += up((long long)p.nwg * 8);
  p.o_slab = o;
  o += up((long long)p.nwg * 8);
  p.o_ckeys = o;
  o += up(p.P * 8);
  p.o_crows = o;
  o += up(p.P * 4);
  p.bytes = o;
  return true;
}

// the key bits of local row r (include/lnw.h: lnw_ppo_sample)
__device__ __forceinline__ u64 sample_key(float x, u64 seed, u64 slot, u64 g, bool &nonfinite) {
  const u64 ctr = (slot << 40) + g;
  uint32_t o[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), LNW_SAMPLE_CTR2, LNW_SAMPLE_CTR3};
  philox10(o, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u = u53(o[0], o[1]);
  const double w = (double)(fabsf(x) + 1e-5f);
  const double k = -p_log(1.0 - u) / w;
  nonfinite = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;
  // (k >= 0: clearing the sign bit only turns -0 into +0)
  return nonfinite ? PS_INF : (__builtin_bit_cast(u64, k) & 0x7FFFFFFFFFFFFFFFull);
}

__global__ __launch_bounds__(PS_THREADS) void ps_init_kernel(SampleWs w, long long batch) {
  const long long i0 = (long long)blockIdx.x * PS_THREADS + threadIdx.x, step = (long long)gridDim.x * PS_THREADS;
  for (long long i = i0; i < (long long)PS_LEVELS * PS_COPIES * PS_BINS; i += step) w.hist[i] = 0u;
  for (long long i = batch + i0; i < w.P; i += step) {
    w.ckeys[i] = PS_PAD;
    w.crows[i] = ~0u;
  }
  if (i0 == 0) {
    w.sel[0].prefix = 0;
    w.sel[0].k_rem = (u64)batch;
    w.nonfinite[0] = 0;
  }
}

// One pass of the radix select over a workgroup's chunk of rows. FIRST: compute
// and store the keys, count the non-finite rows, histogram the top digit of
// every key; else histogram this level's digit of the keys under the prefix.
template <bool FIRST>
__global__ __launch_bounds__(PS_THREADS) void ps_hist_kernel(lnw_ppo_sample_args a, SampleWs w, int level) {
  __shared__ uint32_t h[PS_BINS];
  __shared__ uint32_t nf_sh;
  __shared__ u64 min_sh;
  const int tid = threadIdx.x, nb = level_bins(level), shift = level_shift(level);
  u64 prefix = 0;
  if constexpr (!FIRST) {
    // no key of the chunk lies under the prefix: nothing to count (the whole workgroup leaves)
    prefix = w.sel[level].prefix >> (shift + 13);
    if ((w.cmin[blockIdx.x] >> (shift + 13)) > prefix) return;
  }
  for (int b = tid; b < nb; b += PS_THREADS) h[b] = 0u;
  if (tid == 0) {
    nf_sh = 0u;
    min_sh = PS_PAD;
  }
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * w.chunk;
  const long long r1 = r0 + w.chunk < a.rows ? r0 + w.chunk : a.rows;
  if constexpr (FIRST) {
    const u64 slot = a.draw_dev ? (u64)*a.draw_dev : 0ull;
    uint32_t nf = 0;
    u64 lo = PS_PAD;
    for (long long r = r0 + tid; r < r1; r += PS_THREADS) {
      bool bad;
      const u64 key = sample_key(a.rtg[r], a.seed, slot, (u64)(a.row_base + r), bad);
      w.keys[r] = key;
      nf += bad ? 1u : 0u;
      lo = key < lo ? key : lo;
      atomicAdd(&h[(uint32_t)(key >> shift)], 1u);  // (sign bit clear: < 4096)
    }
    if (nf) atomicAdd(&nf_sh, nf);
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
      const u64 other = __shfl_xor(lo, d);
      lo = other < lo ? other : lo;
    }
    if ((tid & (WAVE - 1)) == 0) atomicMin(&min_sh, lo);
  } else {
    for (long long r = r0 + tid; r < r1; r += PS_THREADS) {
      const u64 key = w.keys[r];
      if ((key >> (shift + 13)) == prefix) atomicAdd(&h[(uint32_t)(key >> shift) & (PS_BINS - 1)], 1u);
    }
  }
  __syncthreads();
  uint32_t *H = w.hist + ((size_t)level * PS_COPIES + (blockIdx.x % PS_COPIES)) * PS_BINS;
  for (int b = tid; b < nb; b += PS_THREADS) {
    const uint32_t c = h[b];
    if (c) atomicAdd(&H[b], c);
  }
  if (FIRST && tid == 0) {
    w.cmin[blockIdx.x] = min_sh;
    if (nf_sh) atomicAdd(w.nonfinite, (u64)nf_sh);
  }
}

// After a pass: the digit in which rank k_rem falls among the keys under the
// prefix. One workgroup of 1024: the copies summed into LDS (every load of a
// thread, 8 copies of up to 8 bins, issued before the first use: the kernel is
// one memory latency long, not one per bin), thread t's range of nb / 1024
// consecutive bins summed, a scan over the threads, and the one thread whose
// range holds the rank walks it. (Counts are at most rows < 2^31: 32-bit sums
// are exact.)
__global__ __launch_bounds__(PS_PICK_THREADS) void ps_pick_kernel(SampleWs w, int level) {
  __shared__ uint32_t c[PS_BINS];
  __shared__ uint32_t inc[PS_PICK_THREADS];
  constexpr int PER_MAX = PS_BINS / PS_PICK_THREADS;
  const int tid = threadIdx.x, nb = level_bins(level), per = nb / PS_PICK_THREADS, shift = level_shift(level);
  const uint32_t *H = w.hist + (size_t)level * PS_COPIES * PS_BINS;
  uint32_t v[PER_MAX];
#pragma unroll
  for (int i = 0; i < PER_MAX; i++) {
    const int b = tid + i * PS_PICK_THREADS;
    v[i] = 0u;
    if (b < nb) {
#pragma unroll
      for (int k = 0; k < PS_COPIES; k++) v[i] += H[k * PS_BINS + b];
    }
  }
#pragma unroll
  for (int i = 0; i < PER_MAX; i++) {
    const int b = tid + i * PS_PICK_THREADS;
    if (b < nb) c[b] = v[i];
  }
  __syncthreads();
  uint32_t mine = 0;
  for (int i = 0; i < per; i++) mine += c[tid * per + i];
  inc[tid] = mine;
  __syncthreads();
  for (int d = 1; d < PS_PICK_THREADS; d <<= 1) {
    const uint32_t u = tid >= d ? inc[tid - d] : 0u;
    __syncthreads();
    inc[tid] += u;
    __syncthreads();
  }
  const u64 k = w.sel[level].k_rem, upto = inc[tid], before = upto - mine;
  // (the keys under the prefix number at least k_rem >= 1, so exactly one range holds rank k; were that ever
  // untrue, the last thread still writes the next level, and every later store stays inside its array)
  if ((before < k && k <= upto) || (tid == PS_PICK_THREADS - 1 && k > upto)) {
    u64 cum = before;
    int b = tid * per;
    for (; b < (tid + 1) * per - 1; b++) {
      if (cum + c[b] >= k) break;
      cum += c[b];
    }
    w.sel[level + 1].prefix = w.sel[level].prefix | ((u64)b << shift);
    w.sel[level + 1].k_rem = k > cum ? k - cum : 0;
  }
}

__global__ __launch_bounds__(PS_THREADS) void ps_count_kernel(lnw_ppo_sample_args a, SampleWs w) {
  __shared__ uint32_t cnt[2];
  const int tid = threadIdx.x;
  if (tid < 2) cnt[tid] = 0u;
  __syncthreads();
  const u64 T = w.sel[PS_LEVELS].prefix;
  if (w.cmin[blockIdx.x] > T) {  // (no row of the chunk is drawn)
    if (tid < 2) w.slab[2 * blockIdx.x + tid] = 0u;
    return;
  }
  const long long r0 = (long long)blockIdx.x * w.chunk;
  const long long r1 = r0 + w.chunk < a.rows ? r0 + w.chunk : a.rows;
  uint32_t nl = 0, ne = 0;
  for (long long r = r0 + tid; r < r1; r += PS_THREADS) {
    const u64 key = w.keys[r];
    nl += key < T ? 1u : 0u;
    ne += key == T ? 1u : 0u;
  }
  if (nl) atomicAdd(&cnt[0], nl);
  if (ne) atomicAdd(&cnt[1], ne);
  __syncthreads();
  if (tid < 2) w.slab[2 * blockIdx.x + tid] = cnt[tid];
}

// Stable compaction: candidate position = rows of the same class (key < T, or
// key == T) before this one, from the slab, the tiles before and a ballot.
__global__ __launch_bounds__(PS_THREADS) void ps_compact_kernel(lnw_ppo_sample_args a, SampleWs w) {
  __shared__ uint32_t before[2];
  __shared__ uint32_t wv[PS_THREADS / WAVE][2];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  if (w.slab[2 * blockIdx.x] == 0u && w.slab[2 * blockIdx.x + 1] == 0u) return;
  if (tid < 2) before[tid] = 0u;
  __syncthreads();
  uint32_t bl = 0, be = 0;
  for (int b = tid; b < (int)blockIdx.x; b += PS_THREADS) {
    bl += w.slab[2 * b];
    be += w.slab[2 * b + 1];
  }
  if (bl) atomicAdd(&before[0], bl);
  if (be) atomicAdd(&before[1], be);
  __syncthreads();
  const u64 T = w.sel[PS_LEVELS].prefix, B = (u64)a.batch;
  const u64 need_eq = w.sel[PS_LEVELS].k_rem;
  u64 base_l = before[0], base_e = (B > need_eq ? B - need_eq : 0) + before[1];
  const long long r0 = (long long)blockIdx.x * w.chunk;
  const long long r1 = r0 + w.chunk < a.rows ? r0 + w.chunk : a.rows;
  for (long long t0 = r0; t0 < r1; t0 += PS_THREADS) {
    const long long r = t0 + tid;
    const bool valid = r < r1;
    const u64 key = valid ? w.keys[r] : PS_PAD;
    const bool isl = valid && key < T, ise = valid && key == T;
    const u64 ml = __ballot(isl), me = __ballot(ise);
    if (lane == 0) {
      wv[wave][0] = (uint32_t)__popcll(ml);
      wv[wave][1] = (uint32_t)__popcll(me);
    }
    __syncthreads();
    uint32_t offl = 0, offe = 0, totl = 0, tote = 0;
#pragma unroll
    for (int v = 0; v < PS_THREADS / WAVE; v++) {
      offl += v < wave ? wv[v][0] : 0u;
      offe += v < wave ? wv[v][1] : 0u;
      totl += wv[v][0];
      tote += wv[v][1];
    }
    const u64 below = (1ull << lane) - 1ull;
    if (isl || ise) {
      const u64 pos = isl ? base_l + offl + (u64)__popcll(ml & below) : base_e + offe + (u64)__popcll(me & below);
      if (pos < B) {  // (rows of key == T beyond the batch; and no store ever leaves the arrays)
        w.ckeys[pos] = key;
        w.crows[pos] = (uint32_t)r;
      }
    }
    base_l += totl;
    base_e += tote;
    __syncthreads();
  }
}

__device__ __forceinline__ bool pair_after(u64 ka, uint32_t ra, u64 kb, uint32_t rb) {
  return ka > kb || (ka == kb && ra > rb);
}

// Bitonic sort, the strides inside a tile: merges k_lo .. k_hi, of each the
// strides min(k / 2, tile / 2) .. 1, on a tile of min(P, 2048) candidates in LDS.
__global__ __launch_bounds__(PS_SORT_THREADS) void ps_sort_tile_kernel(SampleWs w, long long k_lo, long long k_hi) {
  __shared__ u64 sk[PS_TILE];
  __shared__ uint32_t sr[PS_TILE];
  const int tid = threadIdx.x;
  const int nl = w.P < PS_TILE ? (int)w.P : PS_TILE;
  const long long base = (long long)blockIdx.x * nl;
  for (int i = tid; i < nl; i += PS_SORT_THREADS) {
    sk[i] = w.ckeys[base + i];
    sr[i] = w.crows[base + i];
  }
  __syncthreads();
  for (long long k = k_lo; k <= k_hi; k <<= 1) {
    for (int j = (int)(k / 2 < nl / 2 ? k / 2 : nl / 2); j > 0; j >>= 1) {
      for (int i = tid; i < nl / 2; i += PS_SORT_THREADS) {
        const int lo = (i / j) * 2 * j + (i % j), hi = lo + j;
        const bool asc = ((base + lo) & k) == 0;
        const u64 ka = sk[lo], kb = sk[hi];
        const uint32_t ra = sr[lo], rb = sr[hi];
        if (pair_after(ka, ra, kb, rb) == asc) {
          sk[lo] = kb; sr[lo] = rb;
          sk[hi] = ka; sr[hi] = ra;
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < nl; i += PS_SORT_THREADS) {
    w.ckeys[base + i] = sk[i];
    w.crows[base + i] = sr[i];
  }
}

// one stride j >= 2048 of merge k, in place
__global__ __launch_bounds__(PS_THREADS) void ps_sort_step_kernel(SampleWs w, long long k, long long j) {
  const long long i = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i >= w.P / 2) return;
  const long long lo = (i / j) * 2 * j + (i % j), hi = lo + j;
  const bool asc = (lo & k) == 0;
  const u64 ka = w.ckeys[lo], kb = w.ckeys[hi];
  const uint32_t ra = w.crows[lo], rb = w.crows[hi];
  if (pair_after(ka, ra, kb, rb) == asc) {
    w.ckeys[lo] = kb; w.crows[lo] = rb;
    w.ckeys[hi] = ka; w.crows[hi] = ra;
  }
}

__global__ __launch_bounds__(PS_THREADS) void ps_gather_kernel(lnw_ppo_sample_args a, SampleWs w) {
  const long long i = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
  if (i == 0) {
    if (a.status) a.status[0] = (int64_t)w.nonfinite[0];
    if (a.advance && a.draw_dev) a.draw_dev[0] += 1;
  }
  if (i >= a.batch) return;
  long long r = (long long)w.crows[i];
  if (r >= a.rows) r = a.rows - 1;  // (never: keeps a gather inside the arrays whatever the select did)
  a.index_out[i] = r;
  if (a.key_out) a.key_out[i] = __builtin_bit_cast(double, w.ckeys[i]);
  if (a.actions && a.actions_out) {
#pragma unroll
    for (int c = 0; c < 4; c++) a.actions_out[4 * i + c] = a.actions[4 * r + c];
  }
  if (a.log_probs && a.log_probs_out) {
#pragma unroll
    for (int c = 0; c < 4; c++) a.log_probs_out[4 * i + c] = a.log_probs[4 * r + c];
  }
  if (a.rtg_out) a.rtg_out[i] = a.rtg[r];
  if (a.values && a.old_values_out) a.old_values_out[i] = a.values[r / a.n];
}

}  // namespace

extern "C" {

int64_t lnw_ppo_sample_workspace_bytes(int64_t rows, int64_t batch) {
  Plan p;
  return make_plan(rows, batch, p) ? p.bytes : 0;
}

int lnw_ppo_sample(const lnw_ppo_sample_args *args, void *stream) {
  if (!args) return LNW_EINVAL;
  const lnw_ppo_sample_args &a = *args;
  if (!a.rtg || !a.index_out || !a.workspace) return LNW_EINVAL;
  if (a.row_base < 0 || a.rows < 1 || a.row_base > (1ll << 40) - a.rows) return LNW_EINVAL;
  if (a.values && a.old_values_out && a.n < 1) return LNW_EINVAL;
  if ((uintptr_t)a.workspace & 15) return LNW_EINVAL;
  Plan p;
  if (!make_plan(a.rows, a.batch, p)) return LNW_EUNSUPPORTED;
  if (a.workspace_bytes < p.bytes) return LNW_EINVAL;
  char *base = (char *)a.workspace;
  SampleWs w;
  w.keys = (u64 *)base;
  w.hist = (uint32_t *)(base + p.o_hist);
  w.sel = (Sel *)(base + p.o_sel);
  w.nonfinite = (u64 *)(base + p.o_nf);
  w.cmin = (u64 *)(base + p.o_cmin);
  w.slab = (uint32_t *)(base + p.o_slab);
  w.ckeys = (u64 *)(base + p.o_ckeys);
  w.crows = (uint32_t *)(base + p.o_crows);
  w.chunk = p.chunk;
  w.P = p.P;
  hipStream_t st = (hipStream_t)stream;
  const unsigned nwg = (unsigned)p.nwg;

  ps_init_kernel<<<160, PS_THREADS, 0, st>>>(w, a.batch);
  ps_hist_kernel<true><<<nwg, PS_THREADS, 0, st>>>(a, w, 0);
  ps_pick_kernel<<<1, PS_PICK_THREADS, 0, st>>>(w, 0);
  for (int level = 1; level < PS_LEVELS; level++) {
    ps_hist_kernel<false><<<nwg, PS_THREADS, 0, st>>>(a, w, level);
    ps_pick_kernel<<<1, PS_PICK_THREADS, 0, st>>>(w, level);
  }
  ps_count_kernel<<<nwg, PS_THREADS, 0, st>>>(a, w);
  ps_compact_kernel<<<nwg, PS_THREADS, 0, st>>>(a, w);
  if (p.P > 1) {
    const long long nl = p.P < PS_TILE ? p.P : PS_TILE;
    const unsigned tiles = (unsigned)(p.P / nl);
    ps_sort_tile_kernel<<<tiles, PS_SORT_THREADS, 0, st>>>(w, 2, nl);
    for (long long k = 2 * nl; k <= p.P; k <<= 1) {
      for (long long j = k / 2; j >= nl; j >>= 1)
        ps_sort_step_kernel<<<(unsigned)((p.P / 2 + PS_THREADS - 1) / PS_THREADS), PS_THREADS, 0, st>>>(w, k, j);
      ps_sort_tile_kernel<<<tiles, PS_SORT_THREADS, 0, st>>>(w, k, k);
    }
  }
  ps_gather_kernel<<<(unsigned)((a.batch + PS_THREADS - 1) / PS_THREADS), PS_THREADS, 0, st>>>(a, w);
  return hipGetLastError() == hipSuccess ? 0 : LNW_EDEVICE;
}

}  // extern "C"
