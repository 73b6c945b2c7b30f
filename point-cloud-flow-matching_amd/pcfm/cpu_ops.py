"""Pure-PyTorch CPU backend: the native operators for tensors that are not on a
HIP device (BASELINE.json configs[0], "PVConv/Chamfer via pure-PyTorch
fallback" -- SURVEY.md sections 0.5 and 7.2).

The reference has no CPU path: its `_pvcnn_backend`, `chamfer_3D` and `emd_ext`
modules are JIT-built CUDA and reject CPU tensors
(third_party/pvcnn/modules/functional/src/utils.hpp:7-18).  `pcfm.ops` routes a
call here when its inputs are CPU tensors, so models.py / train.py run
unchanged on a machine without a GPU; tensors on a HIP device always take the
gfx950 kernels (and raise if libpcfm_hip.so is missing).

Every function restates the reference kernel it names with vectorised torch
ops (scatter_add_ / gather / blocked pairwise distances), same inputs, outputs,
dtypes and index conventions.  Arithmetic follows the reference's expressions:
  * voxel average: feat * (float)(1.0 / (double)cnt) per term (vox.cu:66-68);
  * trilinear weights x*y*z in that order, corner k = 4dx + 2dy + dz, hi
    corner only if the fraction is > 0 (trilinear_devox.cu:41-75);
  * squared distances with the fused form nvcc emits, fma(dz, dz, fma(dx, dx,
    dy*dy)), evaluated as an exact float64 product + one rounding per fma;
  * argmin ties keep the lowest index (chamfer3D.cu strict `<`).
Scatter sums run in torch's CPU scatter order, so vox-fwd / devox-bwd /
grouping-bwd / chamfer-bwd can differ from a sequential sum in the last bits,
as the reference's float atomics do.  Tests hold this module against the C
oracle (tests/test_cpu_ops.py); it never imports the oracle.
"""
from __future__ import annotations

import torch

__all__ = [
    "avg_voxelize_forward", "avg_voxelize_backward", "trilinear_devoxelize_forward",
    "trilinear_devoxelize_backward", "ball_query", "grouping_forward", "grouping_backward",
    "chamfer_forward", "chamfer_backward", "approxmatch_forward", "matchcost_forward",
    "matchcost_backward", "chamfer_nd_forward", "chamfer_nd_backward", "chamfer_cross_forward",
    "farthest_point_sample", "occupancy_nodes", "occupancy_counts",
    "approxmatch_forward_nd", "matchcost_forward_nd", "matchcost_backward_nd", "emd_auction",
]

# rows of the query set per pairwise block (bounds the (rows, M) temporaries)
_BLOCK_ELEMS = 1 << 22


def _fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """float32 fma(a, b, c): the float64 product of two floats is exact, so one
    float64 add then the cast to float32 rounds (almost always) once."""
    return (a.double() * b.double() + c.double()).float()


def _sqdist(dx, dy, dz):
    """fma(dz, dz, fma(dx, dx, dy * dy)) in float32 (nvcc's contraction of
    dx*dx + dy*dy + dz*dz; chamfer3D.cu:32-35, ball_query.cu:36-38)."""
    if dx.dtype != torch.float32:
        return dx * dx + dy * dy + dz * dz
    return _fma32(dz, dz, _fma32(dx, dx, dy * dy))


# ---------------------------------------------------------------------------
# voxelization (vox.cu:18-110)
# ---------------------------------------------------------------------------
def _inv_count(cnt: torch.Tensor) -> torch.Tensor:
    """(float)(1.0 / (double)cnt) (vox.cu:66, :104); 0 where cnt == 0."""
    inv = (1.0 / cnt.double().clamp_min(1.0)).float()
    return torch.where(cnt > 0, inv, torch.zeros_like(inv))


def avg_voxelize_forward(features: torch.Tensor, coords: torch.Tensor, resolution: int):
    """grid_stats_kernel + avg_voxelize_kernel -> [out (b,c,r^3), ind (b,n), cnt (b,r^3)]."""
    b, c, n = features.shape
    r = int(resolution)
    s = r * r * r
    ind = coords[:, 0] * (r * r) + coords[:, 1] * r + coords[:, 2]  # int32 (b, n)
    ind64 = ind.long()
    cnt = torch.zeros((b, s), dtype=torch.int32)
    cnt.scatter_add_(1, ind64, torch.ones_like(ind))
    w = torch.gather(_inv_count(cnt), 1, ind64)  # 1/cnt of each point's voxel
    out = torch.zeros((b, c, s), dtype=torch.float32)
    out.scatter_add_(2, ind64[:, None, :].expand(b, c, n), features * w[:, None, :])
    return [out, ind.to(torch.int32), cnt]


def avg_voxelize_backward(grad_y: torch.Tensor, indices: torch.Tensor, cnt: torch.Tensor):
    """avg_voxelize_grad_kernel: grad_x[c, i] = grad_y[c, ind[i]] * (1 / cnt[ind[i]])."""
    b, c, _ = grad_y.shape
    n = indices.shape[1]
    ind64 = indices.long()
    w = torch.gather(_inv_count(cnt), 1, ind64)
    return torch.gather(grad_y, 2, ind64[:, None, :].expand(b, c, n)) * w[:, None, :]


# ---------------------------------------------------------------------------
# trilinear devoxelization (trilinear_devox.cu:21-162)
# ---------------------------------------------------------------------------
def _corners(coords: torch.Tensor, r: int):
    """(inds (b,8,n) int32, wgts (b,8,n) f32) with corner k = 4dx + 2dy + dz."""
    x, y, z = coords[:, 0], coords[:, 1], coords[:, 2]
    xl, yl, zl = torch.floor(x), torch.floor(y), torch.floor(z)
    x1, y1, z1 = x - xl, y - yl, z - zl
    x0, y0, z0 = 1.0 - x1, 1.0 - y1, 1.0 - z1
    wgts = torch.stack([x0 * y0 * z0, x0 * y0 * z1, x0 * y1 * z0, x0 * y1 * z1,
                        x1 * y0 * z0, x1 * y0 * z1, x1 * y1 * z0, x1 * y1 * z1], dim=1)
    base = xl.int() * (r * r) + yl.int() * r + zl.int()
    dz = (z1 > 0).int()
    dy = (y1 > 0).int() * r
    dx = (x1 > 0).int() * (r * r)
    inds = torch.stack([base, base + dz, base + dy, base + dy + dz, base + dx, base + dx + dz,
                        base + dx + dy, base + dx + dy + dz], dim=1)
    return inds.to(torch.int32), wgts


def trilinear_devoxelize_forward(r: int, is_training: bool, coords: torch.Tensor,
                                 features: torch.Tensor):
    """-> [outs (b,c,n), inds (b,8,n) | (1,), wgts (b,8,n) | (1,)]."""
    b, c = features.shape[0], features.shape[1]
    n = coords.shape[2]
    r = int(r)
    s = r * r * r
    inds, wgts = _corners(coords, r)
    valid = (inds >= 0) & (inds < s)  # coords outside [0, r-1] contribute 0
    gi = torch.where(valid, inds, torch.zeros_like(inds)).long()
    gw = torch.where(valid, wgts, torch.zeros_like(wgts))
    feats = features.reshape(b, c, s)

    def term(k):
        return torch.gather(feats, 2, gi[:, k:k + 1, :].expand(b, c, n))

    # w1*f1, then fma(w0, f0, .), then fma(wk, fk, .) for k = 2..7 (nvcc's
    # contraction of the left-to-right sum at :98-102)
    acc = gw[:, 1:2] * term(1)
    acc = _fma32(gw[:, 0:1].expand(b, c, n), term(0), acc)
    for k in range(2, 8):
        acc = _fma32(gw[:, k:k + 1].expand(b, c, n), term(k), acc)
    if is_training:
        return [acc, inds, wgts]
    return [acc, torch.zeros((1,), dtype=torch.int32), torch.zeros((1,), dtype=torch.float32)]


def trilinear_devoxelize_backward(grad_y: torch.Tensor, indices: torch.Tensor,
                                  weights: torch.Tensor, r: int):
    """trilinear_devoxelize_grad_kernel: grad_x[c, idx_k] += w_k * grad_y[c, i]."""
    b, c, n = grad_y.shape
    s = int(r) ** 3
    gx = torch.zeros((b, c, s), dtype=torch.float32)
    valid = (indices >= 0) & (indices < s)
    gi = torch.where(valid, indices, torch.zeros_like(indices)).long()
    gw = torch.where(valid, weights, torch.zeros_like(weights))
    for k in range(8):
        gx.scatter_add_(2, gi[:, k:k + 1, :].expand(b, c, n), gw[:, k:k + 1, :] * grad_y)
    return gx


# ---------------------------------------------------------------------------
# ball query + grouping (ball_query.cu:19-50, grouping.cu:18-77)
# ---------------------------------------------------------------------------
def ball_query(centers_coords: torch.Tensor, points_coords: torch.Tensor, radius: float,
               num_neighbors: int):
    """First u point indices k (ascending) with d^2 < radius^2 per center, the
    first hit repeated into the unused slots, all zeros when nothing is in range."""
    b, _, m = centers_coords.shape
    n = points_coords.shape[2]
    u = int(num_neighbors)
    r2 = torch.tensor(float(radius), dtype=torch.float32) ** 2
    out = torch.zeros((b, m, u), dtype=torch.int32)
    if n == 0 or m == 0 or u == 0:
        return out
    rows = max(1, _BLOCK_ELEMS // n)
    slot = torch.arange(u, dtype=torch.int64)[None, :]
    for bb in range(b):
        p = points_coords[bb]
        for j0 in range(0, m, rows):
            cc = centers_coords[bb, :, j0:j0 + rows]
            # dx = center - point (ball_query.cu:36-38)
            d2 = _sqdist(cc[0][:, None] - p[0][None], cc[1][:, None] - p[1][None],
                         cc[2][:, None] - p[2][None])
            hit = d2 < r2
            # the hits in ascending k: a stable sort on "not a hit" keeps index order
            order = torch.argsort((~hit).to(torch.int8), dim=1, stable=True)
            if u > n:
                order = torch.nn.functional.pad(order, (0, u - n))
            order = order[:, :u]
            nhit = hit.sum(dim=1, keepdim=True)
            take = torch.where(slot < nhit, order, order[:, :1])  # pad with the first hit
            take = torch.where(nhit > 0, take, torch.zeros_like(take))
            out[bb, j0:j0 + cc.shape[1]] = take.to(torch.int32)
    return out


def grouping_forward(features: torch.Tensor, indices: torch.Tensor):
    """out[b, c, m, u] = features[b, c, indices[b, m, u]]."""
    b, c, n = features.shape
    m, u = indices.shape[1], indices.shape[2]
    idx = indices.long().reshape(b, 1, m * u).expand(b, c, m * u)
    return torch.gather(features, 2, idx).reshape(b, c, m, u)


def grouping_backward(grad_y: torch.Tensor, indices: torch.Tensor, n: int):
    """grad_x[b, c, indices[b, m, u]] += grad_y[b, c, m, u]."""
    b, c, m, u = grad_y.shape
    idx = indices.long().reshape(b, 1, m * u).expand(b, c, m * u)
    gx = torch.zeros((b, c, int(n)), dtype=torch.float32)
    gx.scatter_add_(2, idx, grad_y.reshape(b, c, m * u))
    return gx


# ---------------------------------------------------------------------------
# Chamfer (chamfer3D.cu:12-195; D components: chamfer{2,5,6}D, csrc/chamfer_nd.hip)
# ---------------------------------------------------------------------------
def _sqdist_nd(d):
    """Squared length of d (..., D) along the last axis, D >= 2, as ONE float32
    chain: acc = d1*d1; acc = fma(d0, d0, acc); acc = fma(dk, dk, acc) for
    k = 2..D-1 (include/pcfm_chamfer_nd.h).  At D = 3 this is _sqdist."""
    if d.dtype != torch.float32:
        acc = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        for k in range(2, d.shape[-1]):
            acc = acc + d[..., k] * d[..., k]
        return acc
    acc = _fma32(d[..., 0], d[..., 0], d[..., 1] * d[..., 1])
    for k in range(2, d.shape[-1]):
        acc = _fma32(d[..., k], d[..., k], acc)
    return acc


def _nn(q: torch.Tensor, p: torch.Tensor):
    """Nearest p for each q: (dist (b, nq), idx (b, nq) int32), lowest index on ties."""
    b, nq, _ = q.shape
    npt = p.shape[1]
    dist = torch.zeros((b, nq), dtype=q.dtype)
    idx = torch.zeros((b, nq), dtype=torch.int32)
    if npt == 0 or nq == 0:
        return dist, idx
    rows = max(1, _BLOCK_ELEMS // npt)
    for bb in range(b):
        pb = p[bb]
        for j0 in range(0, nq, rows):
            qb = q[bb, j0:j0 + rows]
            # dx = candidate - query (chamfer3D.cu:32-35)
            d = _sqdist_nd(pb[None, :, :] - qb[:, None, :])
            val, arg = torch.min(d, dim=1)  # first minimum on ties
            dist[bb, j0:j0 + qb.shape[0]] = val
            idx[bb, j0:j0 + qb.shape[0]] = arg.to(torch.int32)
    return dist, idx


def chamfer_forward(xyz1, xyz2, dist1, dist2, idx1, idx2) -> None:
    """chamfer_cuda_forward: writes the caller-allocated outputs in place."""
    d, i = _nn(xyz1, xyz2)
    dist1.copy_(d)
    idx1.copy_(i)
    d, i = _nn(xyz2, xyz1)
    dist2.copy_(d)
    idx2.copy_(i)


def chamfer_backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2) -> None:
    """NmDistanceGradKernel (both directions): g = 2 * grad_dist; the query's
    gradient += g * (q - p), the matched point's -= it.  Accumulates, like the
    reference (the callers zero the gradients)."""
    for q, p, gd, ix, gq, gp in ((xyz1, xyz2, graddist1, idx1, gradxyz1, gradxyz2),
                                 (xyz2, xyz1, graddist2, idx2, gradxyz2, gradxyz1)):
        if q.shape[1] == 0 or p.shape[1] == 0:
            continue
        ixl = ix.long()
        gat = ixl[:, :, None].expand(-1, -1, q.shape[2])
        matched = torch.gather(p, 1, gat)
        t = (gd * 2.0)[:, :, None] * (q - matched)
        gq.add_(t)
        gp.scatter_add_(1, gat, -t)


# the same two functions under the names of the D-component entry points: the
# point dimension is read from the tensors
chamfer_nd_forward = chamfer_forward
chamfer_nd_backward = chamfer_backward


def chamfer_cross_forward(a: torch.Tensor, b: torch.Tensor):
    """Every cloud of a (S, N, D) against every cloud of b (R, M, D) -> (ab, ba),
    each (S, R) float32 (include/pcfm_chamfer_cross.h): the minima of _nn (the
    float32 chain), their float64 sum divided by the point count in float64, one
    rounding to float32.  An empty cloud gives 0."""
    s, n, _ = a.shape
    r, m, _ = b.shape
    ab = torch.zeros((s, r), dtype=torch.float32)
    ba = torch.zeros((s, r), dtype=torch.float32)
    if n == 0 or m == 0 or r == 0:
        return ab, ba
    for i in range(s):
        ai = a[i:i + 1].expand(r, n, -1)
        ab[i] = (_nn(ai, b)[0].double().sum(dim=1) / n).float()
        ba[i] = (_nn(b, ai)[0].double().sum(dim=1) / m).float()
    return ab, ba


# ---------------------------------------------------------------------------
# farthest-point sampling (include/pcfm_fps.h, csrc/fps.hip)
# ---------------------------------------------------------------------------
def farthest_point_sample(points: torch.Tensor, m: int, start=None):
    """points (B, N, D) float32, N >= 1 -> (idx (B, m) int32, out (B, m, D)): the
    contract of include/pcfm_fps.h.  idx[:, 0] = start clamped to [0, N - 1] (0
    without one); each later pick is the LOWEST index that maximises the minimum,
    over the picks so far, of the float32 chain distance (_sqdist / _sqdist_nd of
    the differences p_i - p_sel) over the first min(D, 3) components."""
    b, n, d = points.shape
    k = min(d, 3)
    pos = points[..., :k]
    idx = torch.zeros((b, m), dtype=torch.int32)
    if m == 0 or b == 0:
        return idx, torch.empty((b, m, d), dtype=points.dtype)
    rows = torch.arange(b)
    sel = torch.zeros(b, dtype=torch.long) if start is None else start.long().clamp(0, n - 1)
    dmin = torch.full((b, n), float("inf"), dtype=points.dtype)
    idx[:, 0] = sel.to(torch.int32)
    for j in range(1, m):
        diff = pos - pos[rows, sel][:, None, :]
        dist = _sqdist(diff[..., 0], diff[..., 1], diff[..., 2]) if k == 3 else _sqdist_nd(diff)
        dmin = torch.minimum(dmin, dist)
        # the lowest index among equal maxima, as _argmin_first of pcfm.metrics
        top = dmin.max(dim=1, keepdim=True).values
        sel = torch.where(dmin == top, torch.arange(n)[None, :], n).min(dim=1).values
        sel = sel.clamp_max(n - 1)      # a row without a maximum (NaN): still an index
        idx[:, j] = sel.to(torch.int32)
    out = torch.gather(points, 1, idx.long()[:, :, None].expand(-1, -1, d))
    return idx, out


# ---------------------------------------------------------------------------
# occupancy counts (include/pcfm_occupancy.h, csrc/occupancy.hip)
# ---------------------------------------------------------------------------
def _occupancy_kept(r: int) -> torch.Tensor:
    """(r, r, r) bool: node (i, j, k) is kept iff a^2 + b^2 + c^2 <= (r-1)^2 with
    a = 2i - (r-1), b and c likewise (integers)."""
    sq = (2 * torch.arange(r) - (r - 1)) ** 2
    return sq[:, None, None] + sq[None, :, None] + sq[None, None, :] <= (r - 1) ** 2


def _occupancy_rint(u: torch.Tensor, r: int) -> torch.Tensor:
    """clamp(rint(u), 0, r-1) as int64, half to even; a NaN gives 0."""
    return torch.nan_to_num(torch.round(u), nan=0.0).clamp(0, r - 1).long()


def _occupancy_nearest_kept(u: torch.Tensor, r: int, kept: torch.Tensor) -> torch.Tensor:
    """u (P, 3) float32 grid coordinates -> (P,) int64: the kept node of LOWEST
    flat index that minimises _sqdist(u - node) (branch 2 of the header).

    The kernel walks every kept node.  Here the kept k of a column (i, j) are one
    interval [klo, khi], and fma(dz, dz, dxy) does not decrease with |dz| (each
    rounding is monotone), so the column's minimum is at the k of the interval
    nearest to u.z: an (r, r) table of column minima per point, the first column
    that holds the overall minimum, then the first k of that column's interval
    that attains it -- the same node as the walk, ties included."""
    p = u.shape[0]
    grid = torch.arange(r, dtype=torch.float32)
    pos, cols = torch.arange(r), torch.arange(r * r)
    count = kept.sum(dim=2).view(-1)              # kept k per column, symmetric about the centre
    has = count > 0
    klo = torch.div(r - count, 2, rounding_mode="floor")
    khi = r - 1 - klo
    mid = r // 2
    out = torch.empty(p, dtype=torch.long)
    for p0 in range(0, p, 8192):
        v = u[p0:p0 + 8192]
        q = v.shape[0]
        dx, dy, dz = (v[:, a, None] - grid for a in range(3))          # (q, r) float32
        dxy = _fma32(dx[:, :, None], dx[:, :, None], (dy * dy)[:, None, :]).view(q, -1)
        near = torch.minimum(torch.maximum(_occupancy_rint(v[:, 2], r)[:, None], klo), khi)
        dzn = dz.gather(1, near)
        best = torch.where(has, _fma32(dzn, dzn, dxy), float("inf"))   # column minima
        low = best.min(dim=1, keepdim=True).values
        col = torch.where((best == low) & has, cols, r * r).min(dim=1).values
        col = torch.where(col == r * r, mid * r + mid, col)            # NaN: the centre
        row = _fma32(dz, dz, dxy.gather(1, col[:, None]))              # (q, r): that column
        ok = (pos >= klo[col][:, None]) & (pos <= khi[col][:, None]) & (row == low)
        k = torch.where(ok, pos, r).min(dim=1).values
        k = torch.where(k == r, mid, k)
        out[p0:p0 + q] = col * r + k
    return out


def occupancy_nodes(points: torch.Tensor, resolution: int) -> torch.Tensor:
    """points (S, N, D) float32, D >= 3 -> (S, N) int64: the flat index of the kept
    node each point counts in (include/pcfm_occupancy.h).  u = fma(p, r-1, (r-1)/2)
    as the float64 product and sum rounded to float32; branch 1 where rint(u) is
    kept, the nearest-kept-node search only for the other points."""
    r = int(resolution)
    s, n = points.shape[:2]
    pos = points[..., :3].reshape(-1, 3)
    u = _fma32(pos, torch.tensor(float(r - 1)), torch.tensor(0.5 * (r - 1)))
    c = _occupancy_rint(u, r)
    node = (c[:, 0] * r + c[:, 1]) * r + c[:, 2]
    kept = _occupancy_kept(r)
    need = ~kept.view(-1)[node]
    if need.any():
        node[need] = _occupancy_nearest_kept(u[need], r, kept)
    return node.view(s, n)


def occupancy_counts(points: torch.Tensor, resolution: int) -> torch.Tensor:
    """points (S, N, D) float32 -> (r^3,) int32: counts[f] = the points of all S
    clouds counted in node f (occupancy_nodes); a node that is not kept holds 0."""
    r = int(resolution)
    nodes = occupancy_nodes(points, r).reshape(-1)
    return torch.bincount(nodes, minlength=r ** 3).to(torch.int32)


# ---------------------------------------------------------------------------
# approximate EMD (PyTorchEMD/cuda/emd_kernel.cu:24-353)
# ---------------------------------------------------------------------------
def _pair_sqdist(xyz1, xyz2):
    """(b, n, m) squared distances, dx = xyz2 - xyz1 (emd_kernel.cu:59-63)."""
    d = xyz2[:, None, :, :] - xyz1[:, :, None, :]
    return _sqdist(d[..., 0], d[..., 1], d[..., 2])


def _pair_sqdist_nd(p1, p2):
    """(b, n, m) squared distances over all D components, d = p2 - p1, as the
    chain of _sqdist_nd (include/pcfm_emd_nd.h); at D = 3 the bits of _pair_sqdist."""
    return _sqdist_nd(p2[:, None, :, :] - p1[:, :, None, :])


def approxmatch_forward(xyz1: torch.Tensor, xyz2: torch.Tensor) -> torch.Tensor:
    """approxmatch: 10 levels (level = -4^j, j = 7..-2, the last 0) of soft
    matching; -> match (b, m, n)."""
    return _approxmatch(xyz1, xyz2, _pair_sqdist)


def _approxmatch(xyz1, xyz2, pair_sqdist):
    b, n = xyz1.shape[0], xyz1.shape[1]
    m = xyz2.shape[1]
    dt = xyz1.dtype
    match = torch.zeros((b, n, m), dtype=dt)
    if n == 0 or m == 0:
        return match.transpose(1, 2).contiguous()
    multi_l = 1.0 if n >= m else float(m // n)
    multi_r = float(n // m) if n >= m else 1.0
    d2 = pair_sqdist(xyz1, xyz2)
    rem_l = torch.full((b, n), multi_l, dtype=dt)
    rem_r = torch.full((b, m), multi_r, dtype=dt)
    for j in range(7, -3, -1):
        level = 0.0 if j == -2 else -(4.0 ** j)
        e = torch.exp(level * d2)  # (b, n, m)
        rat_l = rem_l / (torch.einsum("bnm,bm->bn", e, rem_r) + 1e-9)
        sum_r = torch.einsum("bnm,bn->bm", e, rat_l) * rem_r
        cons = torch.clamp(rem_r / (sum_r + 1e-9), max=1.0)
        rat_r = cons * rem_r
        rem_r = torch.clamp(rem_r - sum_r, min=0.0)
        w = e * rat_l[:, :, None] * rat_r[:, None, :]
        match += w
        rem_l = torch.clamp(rem_l - w.sum(dim=2), min=0.0)
    return match.transpose(1, 2).contiguous()


def matchcost_forward(xyz1: torch.Tensor, xyz2: torch.Tensor, match: torch.Tensor):
    """cost[b] = sum_{k,l} d2(k, l) * match[b, l, k]."""
    d2 = _pair_sqdist(xyz1, xyz2)  # (b, n, m)
    return (d2 * match.transpose(1, 2)).sum(dim=(1, 2))


def matchcost_backward(grad_cost: torch.Tensor, xyz1: torch.Tensor, xyz2: torch.Tensor,
                       match: torch.Tensor):
    """grad1[k] = g * sum_l 2 match[l, k] (x1_k - x2_l); grad2[l] = g * sum_k
    2 match[l, k] (x2_l - x1_k)."""
    mt = match.transpose(1, 2) * 2.0  # (b, n, m)
    g = grad_cost.to(xyz1.dtype)[:, None, None]
    g1 = (mt.sum(dim=2)[:, :, None] * xyz1 - torch.bmm(mt, xyz2)) * g
    g2 = (mt.sum(dim=1)[:, :, None] * xyz2 - torch.bmm(mt.transpose(1, 2), xyz1)) * g
    return [g1, g2]


# the same three over D-component points (include/pcfm_emd_nd.h, csrc/emd.hip):
# every component enters the squared distance with the same weight
def approxmatch_forward_nd(p1: torch.Tensor, p2: torch.Tensor) -> torch.Tensor:
    """approxmatch over p1 (b, n, D), p2 (b, m, D), D >= 2 -> match (b, m, n); at
    D = 3 the bits of approxmatch_forward."""
    return _approxmatch(p1, p2, _pair_sqdist_nd)


def matchcost_forward_nd(p1: torch.Tensor, p2: torch.Tensor, match: torch.Tensor):
    """cost[b] = sum_{k,l} d2(k, l) * match[b, l, k], d2 over all D components."""
    d2 = _pair_sqdist_nd(p1, p2)  # (b, n, m)
    return (d2 * match.transpose(1, 2)).sum(dim=(1, 2))


def matchcost_backward_nd(grad_cost: torch.Tensor, p1: torch.Tensor, p2: torch.Tensor,
                          match: torch.Tensor):
    """matchcost_backward, whose closed form does not look at D: -> [grad1 (b, n, D),
    grad2 (b, m, D)]."""
    return matchcost_backward(grad_cost, p1, p2, match)


# ---------------------------------------------------------------------------
# assignment EMD by auction (include/pcfm_emd_auction.h, csrc/emd_auction.hip)
# ---------------------------------------------------------------------------
def _auction_pair(c: torch.Tensor, eps_rel: float, max_rounds: int):
    """One pair of the rule of include/pcfm_emd_auction.h on its (n, n) float32 cost
    matrix, n >= 1 -> (assignment (n,) int64, rounds), or (None, -1) for a pair
    that would need a round beyond max_rounds.  Every step is an elementwise
    float32 operation or a maximum, over all bidders of a round at once."""
    n = c.shape[0]
    cmax = torch.where(torch.isnan(c), torch.zeros((), dtype=c.dtype), c).max()
    if float(cmax) == 0.0:
        return torch.arange(n), 0
    eps_final = torch.tensor(eps_rel, dtype=torch.float32) * cmax
    eps = torch.maximum(eps_final, cmax * 0.5)
    price = torch.zeros(n, dtype=torch.float32)
    neg_c = -c
    low32 = 0xFFFFFFFF
    rounds = 0
    while True:                                     # phases
        owner = torch.full((n,), -1, dtype=torch.long)
        assigned = torch.full((n,), -1, dtype=torch.long)
        while True:                                 # rounds
            bidders = (assigned < 0).nonzero()[:, 0]
            u = bidders.numel()
            if u == 0:
                break
            if rounds == max_rounds:
                return None, -1
            rounds += 1
            v = neg_c[bidders] - price[None, :]     # (u, n)
            v1, j1 = v.max(dim=1)                   # the first maximum: the lowest index
            if n == 1:
                v2 = v1
            else:
                v[torch.arange(u), j1] = float("-inf")
                v2 = v.max(dim=1).values
            pj = price[j1]
            bid = pj + ((v1 - v2) + eps)
            up = torch.nextafter(pj, torch.full_like(pj, float("inf")))
            bid = torch.where(bid > pj, bid, up)
            # the highest bid, the lowest person among equals: one max of
            # (float bits of the bid) << 32 | ~person (bids are >= +0)
            key = (bid.view(torch.int32).long() << 32) | (low32 - bidders)
            best = torch.full((n,), -1, dtype=torch.long)
            best.scatter_reduce_(0, j1, key, "amax", include_self=True)
            objs = (best >= 0).nonzero()[:, 0]
            won = best[objs]
            winner = low32 - (won & low32)
            prev = owner[objs]
            assigned[prev[prev >= 0]] = -1
            owner[objs] = winner
            assigned[winner] = objs
            price[objs] = (won >> 32).to(torch.int32).view(torch.float32)
        if bool(eps == eps_final):
            return assigned, rounds
        eps = torch.maximum(eps_final, eps * 0.25)


def emd_auction(p1: torch.Tensor, p2: torch.Tensor, eps_rel: float = 2.0 ** -16,
                max_rounds: int = 1 << 20):
    """The rule of include/pcfm_emd_auction.h in pure PyTorch: p1, p2 (B, n, D)
    float32 -> (assignment (B, n) int32, cost (B,) float32, rounds (B,) int32).
    The costs are the chain of _sqdist_nd (its fused multiply-adds by _fma32).  A
    pair that does not finish within max_rounds has rounds -1, an assignment row
    of -1 and a NaN cost."""
    b, n, _ = p1.shape
    assignment = torch.full((b, n), -1, dtype=torch.int32)
    cost = torch.zeros(b, dtype=torch.float32)
    rounds = torch.zeros(b, dtype=torch.int32)
    if n == 0:
        return assignment, cost, rounds
    for bb in range(b):
        c = _pair_sqdist_nd(p1[bb:bb + 1], p2[bb:bb + 1])[0]
        a, r = _auction_pair(c, float(eps_rel), int(max_rounds))
        rounds[bb] = r
        if a is None:
            cost[bb] = float("nan")
            continue
        assignment[bb] = a.to(torch.int32)
        cost[bb] = c[torch.arange(n), a].double().sum().float()
    return assignment, cost, rounds
