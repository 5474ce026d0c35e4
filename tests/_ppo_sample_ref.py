"""NumPy restatement of lnw_ppo_sample's draw (include/lnw.h), written from the
definition and independent of lnw/ppolearn.py: Philox4x32-10 on uint64 arrays,
u53, the portable p_log in float64 array operations, the weights and the order
by (key, global row). `slot` may be an array: keys() then has one row of keys
per slot."""
import numpy as np

CTR2, CTR3 = 0x13198A2E, 0x03707344  # include/lnw.h: LNW_SAMPLE_CTR2 / 3
M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    for _ in range(10):
        a, b = c0 * np.uint64(0xD2511F53), c2 * np.uint64(0xCD9E8D57)
        c0, c1, c2, c3 = (b >> S32) ^ c1 ^ np.uint64(k0), b & M32, (a >> S32) ^ c3 ^ np.uint64(k1), a & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1


def p_log(x):
    m, e = np.frexp(x)
    e = e.astype(np.int64)
    small = m < 0.70710678118654752
    m[small] *= 2.0
    e[small] -= 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = 1.0 / 19.0
    for d in range(17, 0, -2):
        p = p * z + 1.0 / float(d)
    return 2.0 * s * p + e.astype(np.float64) * 0.6931471805599453


def keys(rtg, seed, slot=0, row_base=0):
    rtg = np.asarray(rtg, np.float32)
    g = np.uint64(row_base) + np.arange(rtg.shape[0], dtype=np.uint64)
    ctr = (np.asarray(slot, np.uint64)[..., None] << np.uint64(40)) + g
    o0, o1 = philox(ctr & M32, ctr >> S32, np.full_like(ctr, CTR2), np.full_like(ctr, CTR3),
                    seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = ((o0 >> np.uint64(5)).astype(np.float64) * 2.0 ** 26 + (o1 >> np.uint64(6)).astype(np.float64)) / 2.0 ** 53
    with np.errstate(all="ignore"):
        w = (np.abs(rtg) + np.float32(1e-5)).astype(np.float64)
        k = -p_log(1.0 - u) / w + 0.0  # (+ 0.0: a zero key is +0)
    return np.where(np.isfinite(rtg), k, np.inf)


def draw(rtg, batch, seed, slot=0, row_base=0):
    """(index [batch] int64 local rows in draw order, their keys)."""
    k = keys(rtg, seed, slot, row_base)
    order = np.lexsort((np.arange(k.shape[-1]), k))[:batch]
    return order.astype(np.int64), k[order]


def merge(parts, batch):
    """The first `batch` of the union of shards' draws [(row_base, index, key)]
    by (key, global row): (global rows, keys)."""
    g = np.concatenate([b + i for b, i, _ in parts])
    k = np.concatenate([k for _, _, k in parts])
    order = np.lexsort((g, k))[:batch]
    return g[order], k[order]
