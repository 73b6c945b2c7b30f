"""numpy fp64 reference of the approximate EMD over D-component points
(include/pcfm_emd_nd.h, csrc/emd.hip): emd_ref.approxmatch with pair_d2 taken
over the D-component chain of sqdist_nd (csrc/chamfer_search.hpp),

    acc = d1*d1;  acc = fma(d0, d0, acc);  acc = fma(dk, dk, acc), k = 2 .. D-1,

every difference, the product and every fma rounded to fp32 once (formed in fp64
first).  Everything else -- the exp2 argument, the sums, the finalize expressions,
the level order -- is emd_ref's, by calling it."""
import numpy as np

import emd_ref

DIMS = (2, 5, 6)
# emd_ref.GPU_CASES' shapes, each at D = 2, 5 and 6
CASES = tuple((b, n, m, d) for b, n, m, _ in emd_ref.GPU_CASES for d in DIMS)


def clouds(b, n, m, d):
    g = np.random.default_rng(1000 * n + m + d)
    return g.random((b, n, d)).astype(np.float32), g.random((b, m, d)).astype(np.float32)


def _r32(v):
    return v.astype(np.float32).astype(np.float64)


def pair_d2(p1, p2):
    """d2[k, l] of one batch element's float32 points (n, D), (m, D) -> float32 (n, m)."""
    assert p1.dtype == np.float32 and p2.dtype == np.float32 and p1.shape[1] == p2.shape[1] >= 2
    d = _r32(p2[None, :, :].astype(np.float64) - p1[:, None, :].astype(np.float64))
    acc = _r32(d[..., 1] * d[..., 1])
    acc = _r32(d[..., 0] * d[..., 0] + acc)
    for k in range(2, p1.shape[1]):
        acc = _r32(d[..., k] * d[..., k] + acc)
    return acc.astype(np.float32)


def approxmatch(p1, p2):
    """p1 (b, n, D), p2 (b, m, D) float32 -> match (b, m, n) float64."""
    saved = emd_ref.pair_d2
    emd_ref.pair_d2 = pair_d2
    try:
        return emd_ref.approxmatch(p1, p2)
    finally:
        emd_ref.pair_d2 = saved


def matchcost(p1, p2, match):
    """cost (b,) float64 = sum_{k,l} d2(k, l) * match[l, k], d2 the fp32 chain."""
    return np.array([(pair_d2(p1[bb], p2[bb]).astype(np.float64) * match[bb].T).sum()
                     for bb in range(p1.shape[0])])


def matchcost_grads(gcost, p1, p2, match):
    """The closed form in float64 from a given match (b, m, n):
    grad1[k] = g * sum_l 2 match[l, k] (p1[k] - p2[l]), grad2[l] likewise."""
    p1, p2, mt = p1.astype(np.float64), p2.astype(np.float64), 2.0 * match.astype(np.float64)
    g = np.asarray(gcost, np.float64)[:, None, None]
    g1 = (mt.sum(axis=1)[:, :, None] * p1 - np.einsum("blk,bld->bkd", mt, p2)) * g
    g2 = (mt.sum(axis=2)[:, :, None] * p2 - np.einsum("blk,bkd->bld", mt, p1)) * g
    return g1, g2


rel_err = emd_ref.rel_err
