"""An independent reference for farthest-point sampling (include/pcfm_fps.h),
float64 numpy, shared by tests/test_fps_cpu.py and tests/test_gpu_fps.py.

  * reference(points, m, start): the contract's loop in float64 -- on GRID clouds
    (coordinates integers(0, 2^bits) * 2^-bits, bits <= 10) every difference,
    square and sum is exact in float32 and in float64 alike, so any correct
    implementation returns exactly this index sequence; np.argmax returns the
    first maximum, i.e. the lowest index;
  * min_ratio(points, idx): for picks that cannot be compared index by index
    (random float32 clouds: one differing pick and the sequences part for good),
    the defining property in float64 -- at every round j >= 1 the true dmin of the
    chosen point over the largest true dmin, the smallest such ratio.

PROPERTY_BOUND: the float32 chain's relative error is at most 5u, u = 2^-24 (one
rounding per difference, 2u once squared, one for the product, one per fma; the
running minimum is exact); two compared values give 10u, 12u leaves room for the
second-order terms.
"""
import numpy as np

PROPERTY_BOUND = 1.0 - 12.0 * 2.0 ** -24


def grid_cloud(seed, b, n, d, bits):
    """(b, n, d) float32, every coordinate an integer in [0, 2^bits) times 2^-bits:
    bits = 10 few ties, bits = 3 duplicates and heavy ties."""
    g = np.random.default_rng(seed)
    return (g.integers(0, 1 << bits, (b, n, d)) * 2.0 ** -bits).astype(np.float32)


def random_cloud(seed, b, n, d):
    return np.random.default_rng(seed).standard_normal((b, n, d)).astype(np.float32)


def clamp_start(start, b, n):
    if start is None:
        return np.zeros(b, dtype=np.int64)
    return np.clip(np.asarray(start, dtype=np.int64), 0, n - 1)


def _dist(pos, sel):
    """pos (b, n, k), sel (b,) -> (b, n) float64 squared distances to pos[c, sel[c]]."""
    diff = pos - pos[np.arange(len(pos)), sel][:, None, :]
    return (diff * diff).sum(-1)


def reference(points, m, start=None):
    """points (b, n, d) -> idx (b, m) int64 (n >= 1)."""
    b, n, d = points.shape
    pos = points[..., :min(d, 3)].astype(np.float64)
    idx = np.zeros((b, m), dtype=np.int64)
    if m == 0 or b == 0:
        return idx
    sel = clamp_start(start, b, n)
    dmin = np.full((b, n), np.inf)
    idx[:, 0] = sel
    for j in range(1, m):
        dmin = np.minimum(dmin, _dist(pos, sel))
        sel = np.argmax(dmin, axis=1)          # the first maximum: the lowest index
        idx[:, j] = sel
    return idx


def min_ratio(points, idx):
    """The smallest, over clouds and rounds j >= 1, of
    dmin_j(idx[c][j]) / max_i dmin_j(i), float64, dmin_j from idx[c][:j] itself
    (1.0 where the maximum is 0)."""
    b, n, d = points.shape
    pos = points[..., :min(d, 3)].astype(np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    rows = np.arange(b)
    dmin = np.full((b, n), np.inf)
    worst = 1.0
    for j in range(1, idx.shape[1]):
        dmin = np.minimum(dmin, _dist(pos, idx[:, j - 1]))
        top = dmin.max(axis=1)
        got = dmin[rows, idx[:, j]]
        ratio = np.where(top > 0, got / np.where(top > 0, top, 1.0), 1.0)
        worst = min(worst, float(ratio.min()))
    return worst


def distinct_prefix_ok(points, idx):
    """While a cloud still has a position nobody picked, the farthest point is at a
    distance > 0 from every pick, i.e. a NEW position: the first min(m, U) picks of
    a cloud with U distinct positions have pairwise distinct positions."""
    b, n, d = points.shape
    k = min(d, 3)
    for c in range(b):
        pos = points[c, :, :k]
        u = min(idx.shape[1], len(np.unique(pos, axis=0)))
        if len(np.unique(pos[np.asarray(idx[c, :u], dtype=np.int64)], axis=0)) != u:
            return False
    return True
