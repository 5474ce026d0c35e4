// lnw_tables.inc — the terrain-table builders (cell mask, move table, LOS
// table), the batch / query kernels behind the C-ABI's unit entry points
// (lnw_los_batch, A*, moves, path and LOS queries) and the uniform fill.
// Included by lnw_kernels.hip inside its anonymous namespace, after the observe
// and reset kernels (uses the movement and LOS device functions from there).

// ---------------------------------------------------------------------------
// terrain structures
// ---------------------------------------------------------------------------
__global__ void build_mask_kernel(const uint8_t *grid, int G, int W16, int move_thr, int ew_thr,
                                  uint32_t *mask2) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= G * W16) return;
  int x = i / W16, w = i % W16;
  uint32_t v = 0;
  for (int b = 0; b < 16; b++) {
    int y = w * 16 + b;
    if (y >= G) break;
    uint8_t g = grid[x * G + y];
    v |= ((g > move_thr ? 1u : 0u) | (g > ew_thr ? 2u : 0u)) << (2 * b);
  }
  mask2[i] = v;
}

// move table: check_path(start, start + off) for off in [-4,4]^2, per class
// (mv_cls: Combatant speed 3, LandingShip, medium Combatant speed 2)
constexpr int MV_CLASSES = 3;
__global__ __launch_bounds__(64) void build_move_table_kernel(const uint32_t *mask2, int G, int W16,
                                                              uint32_t *mvtab) {
  __shared__ uint32_t open[OPEN_CAP * WAVE];
  long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  long long n = (long long)MV_CLASSES * G * G * MV_W * MV_W;
  if (i >= n) return;
  int off = (int)(i % (MV_W * MV_W));
  long long cell = (i / (MV_W * MV_W)) % ((long long)G * G);
  int cls = (int)(i / ((long long)MV_W * MV_W * G * G));
  int sx = (int)(cell / G), sy = (int)(cell % G);
  int tx = sx + off / MV_W - R_MV, ty = sy + off % MV_W - R_MV;
  MaskBlocked mb{mask2, W16};
  const int type = cls == 0 ? T_SMALL : (cls == 1 ? T_LS : T_MEDIUM);  // (mv_cls inverse)
  bool feas = check_path_dev(mb, mb(sx, sy), G, type, sx, sy, tx, ty,
                             open + threadIdx.x, WAVE);
  if (feas) atomicOr(&mvtab[(cls * (long long)G * G + cell) * MV_WORDS + (off >> 5)], 1u << (off & 31));
}

// LOS table: for every origin cell and offset in [-40,40]^2, bit0 radar clear,
// bit1 EW clear (full march, no early exit). The 2-bit terrain mask is staged
// into LDS once per workgroup (mwords words, when it fits the launch's LDS),
// and each workgroup then walks many (cell, row) items in a grid-stride loop,
// so the mask is read once per resident workgroup rather than once per 256
// items (G = 512: 64 KiB per workgroup).
__global__ __launch_bounds__(256) void build_los_table_kernel(const uint32_t *mask2, int G, int W16,
                                                              uint32_t *lostab, int mwords) {
  uint32_t *lm = (uint32_t *)lds_dyn;
  for (int w = threadIdx.x; w < mwords; w += blockDim.x) lm[w] = mask2[w];
  __syncthreads();
  const uint32_t *msk = mwords ? lm : mask2;
  const long long n = (long long)G * G * LOS_W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    const int row = (int)(i % LOS_W);
    const long long cell = i / LOS_W;
    const int x1 = (int)(cell / G), y1 = (int)(cell % G);
    const int x2 = x1 + row - R_LOS;
    uint32_t words[LOS_ROW_WORDS] = {0, 0, 0, 0, 0, 0};
    if (x2 >= 0 && x2 < G) {
      for (int c = 0; c < LOS_W; c++) {
        const int y2 = y1 + c - R_LOS;
        if (y2 < 0 || y2 >= G) continue;
        const uint32_t b = los_march<false>(msk, W16, x1, y1, x2, y2);
        const int col = c * 2;
        words[col >> 5] |= b << (col & 31);
      }
    }
    uint32_t *dst = lostab + cell * LOS_CELL_WORDS + row * LOS_ROW_WORDS;
#pragma unroll
    for (int w = 0; w < LOS_ROW_WORDS; w++) dst[w] = words[w];
  }
}

// ---------------------------------------------------------------------------
// unit kernels
// ---------------------------------------------------------------------------
// lnw_los_batch (combatant.py:436-456 per ray): every workgroup first builds the
// grid's 2-bit terrain mask (bit0 cell > move_thr, bit1 cell > ew_thr) in LDS,
// then its waves march their share of the rays from it. A lane whose ray has
// ended takes the wave's next unclaimed ray (ballot + popcount of the lanes
// asking), so a wave advances at its lanes' mean ray length instead of
// waiting on its longest ray; a ray stops early once both bits are blocked
// (the result cannot change).
constexpr int LB_THREADS = 256, LB_RAYS_PER_WAVE = 1024;
__global__ __launch_bounds__(LB_THREADS) void los_batch_kernel(const uint8_t *grid, int G, const int16_t *pairs,
                                                               long long n, int move_thr, int ew_thr, uint8_t *out) {
  const int W16 = (G + 15) >> 4;
  uint32_t *lm = (uint32_t *)lds_dyn;
  for (int w = threadIdx.x; w < G * W16; w += LB_THREADS) {
    const int x = w / W16, y0 = (w - x * W16) * 16;
    uint32_t v = 0;
    for (int b = 0; b < 16 && y0 + b < G; b++) {
      const uint8_t g = grid[(size_t)x * G + y0 + b];
      v |= ((g > move_thr ? 1u : 0u) | (g > ew_thr ? 2u : 0u)) << (2 * b);
    }
    lm[w] = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const long long w0 = ((long long)blockIdx.x * (LB_THREADS / WAVE) + (threadIdx.x / WAVE)) * LB_RAYS_PER_WAVE;
  const long long wend = w0 + LB_RAYS_PER_WAVE < n ? w0 + LB_RAYS_PER_WAVE : n;
  long long next = w0;  // the wave's next unclaimed ray (uniform)
  long long idx = -1;   // this lane's ray
  int x = 0, y = 0, x2 = 0, y2 = 0, dx = 0, dy = 0, sx = 1, sy = 1, err = 0;
  uint32_t blk = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  auto claim = [&]() {
    const unsigned long long need = __ballot(idx < 0);
    if (idx < 0) {
      const long long k = next + __popcll(need & below);
      if (k < wend) {
        const uint64_t pr = *(const uint64_t *)(pairs + 4 * k);
        x = (int16_t)(pr & 0xffffu);
        y = (int16_t)((pr >> 16) & 0xffffu);
        x2 = (int16_t)((pr >> 32) & 0xffffu);
        y2 = (int16_t)(pr >> 48);
        dx = abs(x2 - x);
        dy = abs(y2 - y);
        sx = x > x2 ? -1 : 1;
        sy = y > y2 ? -1 : 1;
        err = dx - dy;
        blk = 0;
        idx = k;
      }
    }
    next += __popcll(need);
  };
  claim();
  while (__any(idx >= 0)) {
    if (idx >= 0) {
#pragma unroll 4
      for (int s = 0; s < 8; s++) {
        blk |= cell_bits(lm, W16, x, y);
        if (blk == 3u || (x == x2 && y == y2)) {
          out[idx] = (uint8_t)((~blk) & 3u);
          idx = -1;
          break;
        }
        const int e2 = 2 * err;
        if (e2 > -dy) { err -= dy; x += sx; }
        if (e2 < dx) { err += dx; y += sy; }
      }
    }
    if (next < wend) claim();
  }
}

// grids whose mask does not fit the launch's LDS: one lane per ray from HBM
__global__ void los_batch_global_kernel(const uint8_t *grid, int G, const int16_t *pairs, long long n,
                                        int move_thr, int ew_thr, uint8_t *out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int x1 = pairs[4 * i], y1 = pairs[4 * i + 1], x2 = pairs[4 * i + 2], y2 = pairs[4 * i + 3];
  int dx = abs(x2 - x1), dy = abs(y2 - y1);
  int sx = x1 > x2 ? -1 : 1, sy = y1 > y2 ? -1 : 1;
  int err = dx - dy;
  bool rb = false, eb = false;
  for (;;) {
    uint8_t g = grid[x1 * G + y1];
    rb |= g > move_thr;
    eb |= g > ew_thr;
    if (x1 == x2 && y1 == y2) break;
    int e2 = 2 * err;
    if (e2 > -dy) { err -= dy; x1 += sx; }
    if (e2 < dx) { err += dx; y1 += sy; }
  }
  out[i] = (rb ? 0 : 1) | (eb ? 0 : 2);
}

__global__ __launch_bounds__(64) void astar_batch_kernel(const uint8_t *grid, int G, int thr,
                                                         const int8_t *types, const int16_t *st,
                                                         const int16_t *tg, long long n,
                                                         int16_t *plen, int8_t *kind,
                                                         uint8_t *feas) {
  __shared__ uint32_t open[OPEN_CAP * WAVE];
  long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  int t = types[i];
  int sx = st[2 * i], sy = st[2 * i + 1], tx = tg[2 * i], ty = tg[2 * i + 1];
  GridBlocked gb{grid, G, thr};
  if (abs(tx) > 500 || abs(ty) > 500 || sx < 0 || sy < 0 || sx >= G || sy >= G) {
    plen[i] = -2; kind[i] = -1; feas[i] = 0;
    return;
  }
  int k;
  int len = astar_dev(gb, G, ship_speed(t), sx, sy, tx, ty, k, open + threadIdx.x, WAVE);
  plen[i] = (int16_t)len;
  kind[i] = (int8_t)k;
  feas[i] = check_path_dev(gb, gb(sx, sy), G, t, sx, sy, tx, ty, open + threadIdx.x, WAVE) ? 1 : 0;
}

__global__ __launch_bounds__(64) void move_batch_kernel(KParams P, KState S, const int8_t *types,
                                                        const int16_t *pos, const double *act,
                                                        const uint8_t *is_f32, long long n,
                                                        int32_t *rounded, uint8_t *ok) {
  __shared__ uint32_t open[OPEN_CAP * WAVE];
  long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  int t = types[i];
  int sx = pos[2 * i], sy = pos[2 * i + 1];
  int nx, ny;
  bool fin = move_target_dev(sx, sy, ship_speed(t), act[2 * i], act[2 * i + 1],
                             is_f32[i] ? K_F32 : K_F64, nx, ny);
  rounded[2 * i] = nx;
  rounded[2 * i + 1] = ny;
  bool f = fin && can_move_to_h(P, S, nx, ny) &&
           check_path_h(P, S, t, sx, sy, nx, ny, open + threadIdx.x, WAVE);
  ok[i] = f ? 1 : 0;
}

__global__ __launch_bounds__(64) void path_query_kernel(KParams P, KState S, const int8_t *types,
                                                        const int16_t *st, const int16_t *tg,
                                                        long long n, uint8_t *out) {
  __shared__ uint32_t open[OPEN_CAP * WAVE];
  long long i = (long long)blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  out[i] = check_path_h(P, S, types[i], st[2 * i], st[2 * i + 1], tg[2 * i], tg[2 * i + 1],
                        open + threadIdx.x, WAVE) ? 1 : 0;
}

__global__ void los_query_kernel(KParams P, KState S, const int16_t *pairs, long long n,
                                 uint8_t *out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = (uint8_t)los_q(P, S, S.mask2, pairs[4 * i], pairs[4 * i + 1], pairs[4 * i + 2],
                          pairs[4 * i + 3]);
}

__global__ void fill_uniform_kernel(float *out, long long n, unsigned long long seed,
                                    unsigned long long offset) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long base = i * 4;
  if (base >= n) return;
  float u[4];
  philox_u4(seed, (offset >> 2) + (unsigned long long)i, u);
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (base + k < n) out[base + k] = u[k];
}
