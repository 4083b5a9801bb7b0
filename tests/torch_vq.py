"""The float64 reference of the vector quantisation (include/gsr_vq.h, fused_vq): true squared distances and their argmin, the
weighted centroid update, Lloyd's algorithm, the error terms both test files use, and the case generators.  numpy only.

Error terms (derived, not measured), u = 2^-24, gamma_n = n u / (1 - n u):
  * a score is a chain of 2 D float32 fmas (D for c2, D for -2 x.c; the scaling by -2 is exact), so it differs from the exact
    |c|^2 - 2 x.c by at most E_ij = gamma_2D (sum_k c_jk^2 + 2 sum_k |x_ik c_jk|) (Higham, Accuracy and Stability, section 3.1: every
    term meets at most 2 D roundings).  A code can be chosen over the true best only when their exact scores are closer than the
    two errors together: d2_true(chosen) <= d2_true(best) + E_chosen + E_best.
  * a centroid is a quotient of two double sums of n exactly formed terms and one rounding to float32:
    |got - S/W| <= u |S/W| + (n + 2) 2^-53 (sum |w x| / W + |S/W|) + the smallest subnormal.
    A term of a list that is added in parts (512 members and more: at most 16 parts of ceil(n / parts)) meets fewer additions than
    the n of the sequential sum, so the bound covers the split as it covers any order of n additions.
"""
import numpy as np

U = 2.0 ** -24

# the kernel's geometry, as far as the shapes under test depend on it (csrc/vq.hip)
TILE = 128          # codes per LDS tile
GROUP_ROWS = 256    # data rows per workgroup

INTEGER_D = (1, 2, 3, 7, 45, 48, 63, 64)
INTEGER_K = (1, 2, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
INTEGER_N = (1, 63, 64, 65, GROUP_ROWS - 1, GROUP_ROWS, GROUP_ROWS + 1, 3 * GROUP_ROWS + 77)
SEPARATED = ((1500, 3, 64, 11), (900, 7, 150, 12), (700, 45, 257, 13))   # (N, D, K, seed)
GENERAL = ((1200, 3, 200, 21, 0.0), (1000, 7, 129, 22, 0.0), (900, 45, 300, 23, 0.0), (800, 45, 130, 24, 50.0), (600, 64, 64, 25, 0.0))
KMEANS_SEPARATED = (1500, 7, 40, 31)


def gamma(n):
    return n * U / (1.0 - n * U)


def dist2_true(x, c):
    """(N, K) float64: sum_k (x_ik - c_jk)^2, formed from the differences"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    out = np.zeros((x.shape[0], c.shape[0]))
    for k in range(x.shape[1]):
        out += (x[:, k, None] - c[None, :, k]) ** 2
    return out


def assign_ref(x, c):
    """-> (idx (N,) int32, d2 (N,) float64, the (N, K) matrix): the argmin of the true squared distance, the lowest index on ties; a row
    that holds a NaN gets -1 and NaN"""
    m = dist2_true(x, c)
    bad = np.isnan(m).all(axis=1)
    idx = np.where(bad, -1, np.argmin(np.where(np.isnan(m), np.inf, m), axis=1)).astype(np.int32)
    d2 = np.where(bad, np.nan, m[np.arange(len(idx)), np.maximum(idx, 0)])
    return idx, d2, m


def score_error(x, c):
    """(N, K) float64: E_ij"""
    x, c = np.abs(np.asarray(x, np.float64)), np.asarray(c, np.float64)
    return gamma(2 * x.shape[1]) * ((c * c).sum(1)[None, :] + 2.0 * x @ np.abs(c).T)


def dist2_rounding(d2, D):
    """what float32(the double chain) may differ from the float64 value by: one rounding, the chain's own error, a subnormal"""
    return U * d2 + (D + 2) * 2.0 ** -52 * d2 + 2.0 ** -149


def update_ref(x, idx, c, w=None):
    """-> (codebook float64 (K, D): S / W, or c's value where a code has no row or W == 0; count (K,) int32; W (K,) float64; the bound
    (K, D) of the header's float32 result against it, 0 where the bits must stay)"""
    x, c = np.asarray(x, np.float64), np.asarray(c, np.float64)
    N, D = x.shape
    K = c.shape[0]
    w = np.ones(N) if w is None else np.asarray(w, np.float64)
    ok = (idx >= 0) & (idx < K)
    j = idx[ok]
    count = np.bincount(j, minlength=K).astype(np.int32)
    W = np.bincount(j, weights=w[ok], minlength=K)
    S, A = np.zeros((K, D)), np.zeros((K, D))
    for d in range(D):
        S[:, d] = np.bincount(j, weights=w[ok] * x[ok, d], minlength=K)
        A[:, d] = np.bincount(j, weights=w[ok] * np.abs(x[ok, d]), minlength=K)
    moved = (count > 0) & (W > 0)
    Ws = np.where(moved, W, 1.0)[:, None]
    new = np.where(moved[:, None], S / Ws, c)
    bound = np.where(moved[:, None], U * np.abs(new) + (count[:, None] + 2.0) * 2.0 ** -53 * (A / Ws + np.abs(new)) + 2.0 ** -149, 0.0)
    return new, count, W, bound


def kmeans_ref(x, init, iters, w=None):
    """Lloyd's algorithm in float64 -> per iteration: (idx, the codebook after the update, inertia, the codebook it assigned against)"""
    c = np.asarray(init, np.float64).copy()
    ww = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    out = []
    for _ in range(iters):
        idx, d2, _ = assign_ref(x, c)
        before = c
        c = update_ref(x, idx, c, w)[0]
        out.append((idx, c, float((ww * d2).sum()), before))
    return out


def gaps(x, c):
    """-> (gap (N,): second-best minus best true squared distance (+inf for K = 1), need (N,): E of the best plus E of the second best)"""
    m = dist2_true(x, c)
    E = score_error(x, c)
    if m.shape[1] == 1:
        return np.full(len(m), np.inf), E[:, 0]
    two = np.argpartition(m, 1, axis=1)[:, :2]
    r = np.arange(len(m))
    a, b = m[r, two[:, 0]], m[r, two[:, 1]]
    return np.abs(a - b), E[r, two[:, 0]] + E[r, two[:, 1]]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def integer_case(N, D, K, seed):
    """small integers, |value| <= 3 (so many exact ties), every score below 2^24: exactly representable throughout"""
    rng = np.random.default_rng(seed)
    return rng.integers(-3, 4, (N, D)).astype(np.float32), rng.integers(-3, 4, (K, D)).astype(np.float32)


def integer_answer(x, c):
    """the exact integer argmin (lowest index) and squared distance"""
    xi, ci = x.astype(np.int64), c.astype(np.int64)
    d2 = (xi * xi).sum(1)[:, None] + (ci * ci).sum(1)[None, :] - 2 * xi @ ci.T
    idx = np.argmin(d2, axis=1)
    return idx.astype(np.int32), d2[np.arange(len(idx)), idx].astype(np.float32)


def general_case(N, D, K, seed, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(offset, 1.0, (N, D))).astype(np.float32), (rng.normal(offset, 1.0, (K, D))).astype(np.float32)


def separated_case(N, D, K, seed):
    """K centres of spread 10, rows within 0.01 of a centre; the codebook is the centres moved by 0.001 -> (x, codebook, label)"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 10.0, (K, D))
    label = rng.integers(0, K, N)
    label[:min(N, K)] = np.arange(min(N, K))   # every centre owns a row
    x = centres[label] + rng.uniform(-0.01, 0.01, (N, D))
    return x.astype(np.float32), (centres + rng.uniform(-0.001, 0.001, (K, D))).astype(np.float32), label.astype(np.int32)
