"""Generation metrics between a set of generated clouds and a set of reference
clouds: minimum matching distance (MMD), coverage (COV) and 1-nearest-neighbour
accuracy (1-NNA), under Chamfer distance and under the EMD (the approximate match
or the auction's one-to-one match), and the Jensen-Shannon divergence (JSD)
between the two sets' occupancy histograms.

Each of the first three reduces an (S, R) matrix of cloud-to-cloud distances:

  * pairwise_chamfer -- one launch of the set-against-set kernel
    (csrc/chamfer_cross.hip through ops.chamfer_cross_forward): no cloud is
    copied and no per-point distance is written;
  * pairwise_emd -- the approximate-match cost of PyTorchEMD over gathered
    chunks of pairs (ops.approxmatch_cost_forward, no match matrix written);
  * pairwise_emd_nd -- the same over all D components of the points
    (ops.approxmatch_cost_forward_nd, csrc/emd.hip), so that the EMD figures
    see the colour of xyz+rgb clouds;
  * pairwise_emd_auction -- the cost of a one-to-one match within a stated bound
    of the optimal bijection's (ops.emd_auction, csrc/emd_auction.hip), over all D
    components: symmetric in its two clouds to within that bound.

Clouds larger than the matrices can take (or of different sizes) are first cut
to n_points points each by farthest-point sampling: subsample, one launch of
csrc/fps.hip per set through ops.farthest_point_sample.

JSD looks at a set as one distribution of points in space: occupancy_counts, one
call of csrc/occupancy.hip per set through ops.occupancy_counts, counts the
points of all clouds of a set on an r x r x r grid (the nodes inside the inscribed
sphere), and jsd_from_counts takes the divergence of the two normalised
histograms.

Rows are generated clouds, columns reference clouds.  Nothing here needs a
gradient: everything runs under torch.no_grad(), and every output is on the
inputs' device (HIP tensors take the kernels, CPU tensors pcfm.cpu_ops).
"""
from __future__ import annotations

import torch

from . import _lib, ops

__all__ = ["pairwise_chamfer", "pairwise_emd", "pairwise_emd_nd", "pairwise_emd_auction", "mmd_cov",
           "one_nna", "generation_metrics", "subsample", "occupancy_counts", "jsd_from_counts",
           "jsd"]

# pairs per approxmatch call, at most (the batch is a grid dimension of its kernels)
_EMD_MAX_PAIRS = 32767


@torch.no_grad()
def pairwise_chamfer(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x (S, N, D), y (R, M, D) float32, D in {2, 3, 5, 6} -> (S, R) float32:
    entry [i, j] = mean_p min_q |y[j][q] - x[i][p]|^2 + mean_q min_p |x[i][p] - y[j][q]|^2,
    which for one pair is pcfm.sample.chamfer_l2."""
    ab, ba = ops.chamfer_cross_forward(x.contiguous(), y.contiguous())
    return ab + ba


@torch.no_grad()
def subsample(clouds: torch.Tensor, m: int, start=None) -> torch.Tensor:
    """clouds (S, N, D) float32, D in {2, 3, 5, 6} -> (S, m, D): m points of each
    cloud chosen by farthest-point sampling over the position (the first
    min(D, 3) components; ops.farthest_point_sample), the rows copied bit for
    bit.  start (S,) int32: each cloud's first pick (index 0 without one).  The
    published protocol compares clouds of about 2048 points; m > N raises
    ValueError."""
    if clouds.dim() != 3:
        raise ValueError(f"subsample: expected (S, N, D), got {tuple(clouds.shape)}")
    if not 0 <= m <= clouds.shape[1]:
        raise ValueError(f"subsample: m = {m} outside [0, N = {clouds.shape[1]}]")
    return ops.farthest_point_sample(clouds.contiguous(), m, start)[1]


def _emd_chunk_bytes(pairs: int, n: int, m: int, like: torch.Tensor) -> int:
    """Bytes one approxmatch call over `pairs` gathered pairs holds besides its
    (pairs,) result: the gathered inputs and the kernels' workspace (HIP) or the
    four (pairs, n, m) temporaries of cpu_ops.approxmatch_forward (CPU)."""
    inputs = pairs * (n + m) * 3 * 4
    if like.is_cuda:
        return inputs + _lib.query("pcfm_emd_workspace_bytes", pairs, n, m, 4)
    return inputs + 4 * pairs * n * m * 4


def _emd_nd_chunk_bytes(pairs: int, n: int, m: int, d: int, like: torch.Tensor) -> int:
    """_emd_chunk_bytes for points of d components: the gathered inputs and the
    workspace of include/pcfm_emd_nd.h (HIP), which grows with the pack width."""
    inputs = pairs * (n + m) * d * 4
    if like.is_cuda:
        return inputs + _lib.query("pcfm_emd_nd_workspace_bytes", pairs, n, m, d)
    return inputs + 4 * pairs * n * m * 4


def _emd_pairs_per_chunk(total: int, n: int, m: int, max_bytes: int, like: torch.Tensor,
                         d=None) -> int:
    """Pairs per chunk (<= total, <= _EMD_MAX_PAIRS): the largest count a bisection
    finds whose bytes stay under max_bytes.  d: the N-D entries' component count
    (None: pairwise_emd's 3-D entries)."""
    def chunk_bytes(pairs):
        if d is None:
            return _emd_chunk_bytes(pairs, n, m, like)
        return _emd_nd_chunk_bytes(pairs, n, m, d, like)

    if chunk_bytes(1) > max_bytes:
        raise ValueError(f"pairwise_emd: max_bytes = {max_bytes} is below one pair's "
                         f"{chunk_bytes(1)} bytes")
    lo, hi = 1, max(1, min(total, _EMD_MAX_PAIRS))   # bytes grow with the pair count
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if chunk_bytes(mid) <= max_bytes:
            lo = mid
        else:
            hi = mid - 1
    return lo


@torch.no_grad()
def pairwise_emd(x: torch.Tensor, y: torch.Tensor, max_bytes: int = 1 << 30) -> torch.Tensor:
    """x (S, n, 3), y (R, n, 3) float32 -> (S, R) float32: entry [i, j] = the
    approximate-match cost with xyz1 = x[i], xyz2 = y[j] (PyTorchEMD's forward),
    divided by n.

    ORIENTATION: the approximate match is not symmetric in its two clouds --
    pairwise_emd(x, x) is not a symmetric matrix (entries [i, j] and [j, i]
    differ by more than a tenth of the largest entry on random clouds), and
    pairwise_emd(y, x) is not the transpose of pairwise_emd(x, y).  The first
    argument's clouds are always xyz1; nothing is symmetrised.

    Pairs are gathered in chunks; a chunk's gathered inputs plus the call's
    workspace stay under max_bytes.  The result does not depend on the chunking.
    Anything but D = 3 and equal point counts raises ValueError."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != 3 or y.shape[2] != 3:
        raise ValueError(f"pairwise_emd: expected (S, n, 3) and (R, n, 3), got {tuple(x.shape)} "
                         f"and {tuple(y.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"pairwise_emd: point counts differ ({x.shape[1]} and {y.shape[1]})")
    x, y = x.contiguous(), y.contiguous()
    s, r, n = x.shape[0], y.shape[0], x.shape[1]
    out = torch.empty(s * r, dtype=torch.float32, device=x.device)
    if s * r == 0 or n == 0:
        return out.zero_().view(s, r)
    chunk = _emd_pairs_per_chunk(s * r, n, n, max_bytes, x)
    for p0 in range(0, s * r, chunk):
        p = torch.arange(p0, min(p0 + chunk, s * r), device=x.device)
        i, j = torch.div(p, r, rounding_mode="floor"), p % r
        _, cost = ops.approxmatch_cost_forward(x[i], y[j], want_match=False)
        out[p0:p0 + p.numel()] = cost / n
    return out.view(s, r)


@torch.no_grad()
def pairwise_emd_nd(x: torch.Tensor, y: torch.Tensor, max_bytes: int = 1 << 30) -> torch.Tensor:
    """x (S, n, D), y (R, n, D) float32, D in {2, 3, 5, 6} -> (S, R) float32:
    pairwise_emd with the squared distance taken over all D components, every
    component with the same weight (ops.approxmatch_cost_forward_nd); at D = 3 the
    bits of pairwise_emd.

    ORIENTATION: as for pairwise_emd, the approximate match is not symmetric in
    its two clouds: the first argument's clouds are always p1, pairwise_emd_nd(y, x)
    is not the transpose of pairwise_emd_nd(x, y), and nothing is symmetrised.

    Pairs are gathered in chunks; a chunk's gathered inputs plus the call's
    workspace stay under max_bytes.  The result does not depend on the chunking
    (on HIP tensors by the kernels' contract: a pair's bits do not depend on the
    batch it is in).  An unsupported or unequal D and unequal point counts raise
    ValueError."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != y.shape[2] \
            or x.shape[2] not in ops.EMD_ND_DIMS:
        raise ValueError(f"pairwise_emd_nd: expected (S, n, D) and (R, n, D), D in "
                         f"{ops.EMD_ND_DIMS}, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"pairwise_emd_nd: point counts differ ({x.shape[1]} and {y.shape[1]})")
    x, y = x.contiguous(), y.contiguous()
    s, r, n, d = x.shape[0], y.shape[0], x.shape[1], x.shape[2]
    out = torch.empty(s * r, dtype=torch.float32, device=x.device)
    if s * r == 0 or n == 0:
        return out.zero_().view(s, r)
    chunk = _emd_pairs_per_chunk(s * r, n, n, max_bytes, x, d)
    for p0 in range(0, s * r, chunk):
        p = torch.arange(p0, min(p0 + chunk, s * r), device=x.device)
        i, j = torch.div(p, r, rounding_mode="floor"), p % r
        _, cost = ops.approxmatch_cost_forward_nd(x[i], y[j], want_match=False)
        out[p0:p0 + p.numel()] = cost / n
    return out.view(s, r)


@torch.no_grad()
def pairwise_emd_auction(x: torch.Tensor, y: torch.Tensor, eps_rel: float = 2.0 ** -16,
                         max_rounds: int = 1 << 20, max_bytes: int = 1 << 30) -> torch.Tensor:
    """x (S, n, D), y (R, n, D) float32, D in {2, 3, 5, 6} -> (S, R) float32: entry
    [i, j] = the cost of the one-to-one match the auction finds between x[i] and
    y[j] over all D components (ops.emd_auction, csrc/emd_auction.hip; no
    assignment is written), divided by n: the units of pairwise_emd_nd.

    ORIENTATION: the match is a bijection whose cost is at most
    n * eps_rel * (the pair's largest squared distance) above the optimum's, and
    the optimum does not depend on which cloud comes first.  Entries [i, j] of
    pairwise_emd_auction(x, y) and [j, i] of pairwise_emd_auction(y, x) therefore
    differ by at most eps_rel * (that largest squared distance), which is what
    one_nna's joint matrix assumes.

    Pairs are gathered in chunks; a chunk's gathered inputs (and, on the CPU, the
    pair's cost matrices) stay under max_bytes.  The result does not depend on
    the chunking: a pair's bits do not depend on the batch it is in.  An
    unsupported or unequal D and unequal point counts raise ValueError; a pair
    whose auction does not finish within max_rounds raises RuntimeError."""
    if x.dim() != 3 or y.dim() != 3 or x.shape[2] != y.shape[2] \
            or x.shape[2] not in ops.EMD_ND_DIMS:
        raise ValueError(f"pairwise_emd_auction: expected (S, n, D) and (R, n, D), D in "
                         f"{ops.EMD_ND_DIMS}, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.shape[1] != y.shape[1]:
        raise ValueError(f"pairwise_emd_auction: point counts differ ({x.shape[1]} and "
                         f"{y.shape[1]})")
    x, y = x.contiguous(), y.contiguous()
    s, r, n, d = x.shape[0], y.shape[0], x.shape[1], x.shape[2]
    out = torch.empty(s * r, dtype=torch.float32, device=x.device)
    if s * r == 0 or n == 0:
        return out.zero_().view(s, r)
    # the gathered pair; the CPU backend also holds a pair's cost matrix three times
    pair_bytes = 2 * n * d * 4 + (0 if x.is_cuda else 3 * n * n * 4)
    if pair_bytes > max_bytes:
        raise ValueError(f"pairwise_emd_auction: max_bytes = {max_bytes} is below one pair's "
                         f"{pair_bytes} bytes")
    chunk = min(max_bytes // pair_bytes, s * r, _EMD_MAX_PAIRS)
    unfinished = 0
    for p0 in range(0, s * r, chunk):
        p = torch.arange(p0, min(p0 + chunk, s * r), device=x.device)
        i, j = torch.div(p, r, rounding_mode="floor"), p % r
        _, cost, rounds = ops.emd_auction(x[i], y[j], eps_rel=eps_rel, max_rounds=max_rounds,
                                          want_assignment=False)
        unfinished += int((rounds < 0).sum())
        out[p0:p0 + p.numel()] = cost / n
    if unfinished:
        raise RuntimeError(f"pairwise_emd_auction: {unfinished} of {s * r} pairs did not finish "
                           f"their auction within max_rounds = {max_rounds} rounds")
    return out.view(s, r)


def _argmin_first(m: torch.Tensor, dim: int) -> torch.Tensor:
    """argmin along dim, the LOWEST index among equal minima."""
    lo = m.min(dim=dim, keepdim=True).values
    shape = [1, 1]
    shape[dim] = m.shape[dim]
    pos = torch.arange(m.shape[dim], device=m.device).view(shape)
    return torch.where(m == lo, pos, m.shape[dim]).min(dim=dim).values


def _share(flags: torch.Tensor, dtype) -> torch.Tensor:
    """Share of true entries as a 0-dim `dtype` tensor: an exact count and one
    float64 tensor-by-tensor division, rounded once, so that HIP and CPU give the
    same bits (a mean's rounding depends on the device's reduction, and a division
    by a Python scalar multiplies by a rounded reciprocal on the device)."""
    total = torch.tensor(float(flags.numel()), dtype=torch.float64, device=flags.device)
    return (flags.sum(dtype=torch.float64) / total).to(dtype)


@torch.no_grad()
def mmd_cov(m: torch.Tensor) -> dict:
    """m (S, R): rows generated clouds, columns reference clouds ->
      mmd      mean over the columns of the column minimum (each reference cloud's
               nearest generated cloud);
      mmd_smp  mean over the rows of the row minimum;
      cov      (distinct columns that are some row's argmin) / R.
    Ties: the lowest index."""
    if m.dim() != 2 or m.shape[0] == 0 or m.shape[1] == 0:
        raise ValueError(f"mmd_cov: expected a non-empty (S, R) matrix, got {tuple(m.shape)}")
    hit = torch.zeros(m.shape[1], dtype=torch.bool, device=m.device)
    hit[_argmin_first(m, 1)] = True
    return {"mmd": m.min(dim=0).values.mean(), "mmd_smp": m.min(dim=1).values.mean(),
            "cov": _share(hit, m.dtype)}


@torch.no_grad()
def one_nna(mxx: torch.Tensor, mxy: torch.Tensor, myy: torch.Tensor) -> dict:
    """Leave-one-out 1-nearest-neighbour classification of the S generated
    (label 1) and R reference (label 0) clouds over
        J = [[mxx, mxy], [mxy^T, myy]]   with +inf on the diagonal:
    a column's prediction is the label of its argmin row (lowest index on ties) ->
      acc      share of the columns whose prediction equals their label;
      acc_gen  the same share among the S generated clouds;
      acc_ref  among the R reference clouds.
    0.5 is the aim (the sets cannot be told apart), 1.0 the worst."""
    s, r = mxy.shape
    if tuple(mxx.shape) != (s, s) or tuple(myy.shape) != (r, r) or s == 0 or r == 0:
        raise ValueError(f"one_nna: expected (S, S), (S, R), (R, R), got {tuple(mxx.shape)}, "
                         f"{tuple(mxy.shape)}, {tuple(myy.shape)}")
    j = torch.cat([torch.cat([mxx, mxy], dim=1), torch.cat([mxy.t(), myy], dim=1)], dim=0)
    j = j.clone()
    j.fill_diagonal_(float("inf"))
    label = torch.cat([torch.ones(s, device=j.device), torch.zeros(r, device=j.device)])
    ok = label[_argmin_first(j, 0)] == label
    return {"acc": _share(ok, mxy.dtype), "acc_gen": _share(ok[:s], mxy.dtype),
            "acc_ref": _share(ok[s:], mxy.dtype)}


@torch.no_grad()
def occupancy_counts(clouds: torch.Tensor, resolution: int = 28) -> torch.Tensor:
    """clouds (S, N, D) float32, D in {3, 5, 6}; 3 <= resolution <= 32 -> (r^3,)
    int32 on the clouds' device: how many points of the whole set count in each
    node of the r x r x r grid over the cube [-0.5, 0.5]^3 (ops.occupancy_counts;
    include/pcfm_occupancy.h states the rule).  Only the nodes inside the inscribed
    sphere take points: a point outside it counts in the nearest node inside.  The
    clouds are counted as given -- bringing them into the unit cube is the
    caller's data convention.  r = 28 is the published protocol's resolution.  A
    bad shape, D = 2 or a resolution outside [3, 32] raises ValueError."""
    if clouds.dim() != 3:
        raise ValueError(f"occupancy_counts: expected (S, N, D), got {tuple(clouds.shape)}")
    if clouds.shape[2] not in (3, 5, 6):
        raise ValueError(f"occupancy_counts: D = {clouds.shape[2]} is not 3, 5 or 6 (the grid is "
                         "three-dimensional)")
    if not 3 <= int(resolution) <= 32:
        raise ValueError(f"occupancy_counts: resolution = {resolution} outside [3, 32]")
    return ops.occupancy_counts(clouds.contiguous(), int(resolution))


def _kl_bits_sum(w: torch.Tensor, a: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """sum over the entries with w > 0 of w * log2(2 a / t), float64, in index order."""
    on = w > 0
    return (w[on] * torch.log2(2.0 * a[on] / t[on])).sum()


@torch.no_grad()
def jsd_from_counts(p_counts: torch.Tensor, q_counts: torch.Tensor) -> torch.Tensor:
    """Two count vectors of one length -> the Jensen-Shannon divergence of the
    normalised histograms P = p / sum p, Q = q / sum q, as a 0-dim float64 tensor
    on the inputs' device: H(M) - (H(P) + H(Q)) / 2 with M = (P + Q) / 2 and H the
    entropy in bits (0 log 0 = 0), so the value lies in [0, 1].  The sets may
    differ in size; the normalisation absorbs it.

    It is summed in the equivalent form (KL(P || M) + KL(Q || M)) / 2 over the
    counts themselves: with a = p * sum q and b = q * sum p,
        (sum_i p_i log2(2 a_i / (a_i + b_i))) / sum p, the same with q and b, halved.
    Histograms that are multiples of one another have a == b entry by entry, every
    logarithm is log2(1) and the result is exactly 0; disjoint supports make every
    logarithm log2(2), the sums are sums of integers and the result is exactly 1
    -- which differences of three rounded entropies would not give.

    The two vectors (2 * r^3 * 4 bytes) are copied to the host and the arithmetic
    runs there in float64, in one fixed order; the result goes back to the
    inputs' device.  HIP and CPU inputs therefore give the same bits, at the cost
    of one small copy and a synchronisation per call.  An empty histogram (sum 0)
    raises ValueError."""
    if p_counts.dim() != 1 or p_counts.shape != q_counts.shape:
        raise ValueError(f"jsd_from_counts: expected two vectors of one length, got "
                         f"{tuple(p_counts.shape)} and {tuple(q_counts.shape)}")
    if p_counts.device != q_counts.device:
        raise ValueError("jsd_from_counts: the two vectors are on different devices")
    p, q = p_counts.detach().cpu().double(), q_counts.detach().cpu().double()
    if bool((p < 0).any()) or bool((q < 0).any()):
        raise ValueError("jsd_from_counts: a negative count")
    sp, sq = p.sum(), q.sum()
    if float(sp) <= 0 or float(sq) <= 0:
        raise ValueError("jsd_from_counts: an empty histogram")
    a, b = p * sq, q * sp
    t = a + b
    out = (_kl_bits_sum(p, a, t) / sp + _kl_bits_sum(q, b, t) / sq) / 2
    return out.clamp(0.0, 1.0).to(p_counts.device)


@torch.no_grad()
def jsd(sample: torch.Tensor, ref: torch.Tensor, resolution: int = 28) -> torch.Tensor:
    """sample (S, N, D), ref (R, M, D) float32, D in {3, 5, 6} -> the Jensen-Shannon
    divergence (0-dim float64) between the occupancy histograms of the two sets:
    jsd_from_counts of their occupancy_counts at `resolution`."""
    return jsd_from_counts(occupancy_counts(sample, resolution),
                           occupancy_counts(ref, resolution))


@torch.no_grad()
def generation_metrics(sample: torch.Tensor, ref: torch.Tensor, emd: bool = True,
                       n_points=None, jsd: bool = False, jsd_resolution: int = 28,
                       emd_components: str = "xyz", emd_match: str = "approx") -> dict:
    """sample (S, N, D), ref (R, M, D) float32 -> {mmd_cd, mmd_smp_cd, cov_cd,
    1nna_cd, 1nna_gen_cd, 1nna_ref_cd} and, with emd=True, the same six with
    _emd.  Chamfer runs over all D components (D in {2, 3, 5, 6}).  EMD needs
    N == M and runs over what emd_components names: "xyz", the first three
    components (pairwise_emd; D = 2 raises ValueError), or "all", all D components
    with the same weight (pairwise_emd_nd; D = 2 works), under the same _emd keys.
    Any other value raises ValueError.  The S x S and R x R matrices of 1-NNA
    come from the same kernels, a set against itself.  n_points: both sets go
    through subsample(., n_points) before any matrix is formed, so sets whose
    clouds differ in size (or are too large for the EMD matrix) compare at
    n_points points each; None compares the clouds as given.

    jsd=True adds one key, "jsd": the Jensen-Shannon divergence (0-dim float64)
    of the two sets' occupancy histograms at jsd_resolution, taken on the clouds
    AS GIVEN, before the n_points subsample.  Farthest-point sampling evens out
    density on purpose: a histogram of such a subsample measures the support of
    a shape, not where its points lie.  N and M may differ (the histograms are
    normalised); D = 2 raises ValueError.  With jsd=False the result is what it
    was without the keyword.

    emd_match names the match behind the _emd keys: "approx", the approximate
    match above, or "auction", the one-to-one match of pairwise_emd_auction (at its
    default eps_rel and max_rounds) over the same components -- a symmetric
    distance within a stated bound of the optimal bijection's, at most 2048 points
    a cloud on HIP tensors (n_points brings larger clouds there).  Any other value
    raises ValueError.  With "approx" the result is what it was without the
    keyword."""
    if emd_components not in ("xyz", "all"):
        raise ValueError(f"generation_metrics: emd_components = {emd_components!r} is neither "
                         "'xyz' nor 'all'")
    if emd_match not in ("approx", "auction"):
        raise ValueError(f"generation_metrics: emd_match = {emd_match!r} is neither 'approx' "
                         "nor 'auction'")
    auction = emd_match == "auction"
    extra = {"jsd": _jsd(sample, ref, jsd_resolution)} if jsd else {}
    if n_points is not None:
        sample, ref = subsample(sample, n_points), subsample(ref, n_points)
    sample, ref = sample.contiguous(), ref.contiguous()

    def reduce(pairwise, a, b, tag):
        mxy = pairwise(a, b)
        out = {f"{k}_{tag}": v for k, v in mmd_cov(mxy).items()}
        nna = one_nna(pairwise(a, a), mxy, pairwise(b, b))
        out.update({f"1nna_{tag}": nna["acc"], f"1nna_gen_{tag}": nna["acc_gen"],
                    f"1nna_ref_{tag}": nna["acc_ref"]})
        return out

    out = reduce(pairwise_chamfer, sample, ref, "cd")
    if emd and emd_components == "all":
        out.update(reduce(pairwise_emd_auction if auction else pairwise_emd_nd, sample, ref,
                          "emd"))
    elif emd:
        if sample.shape[-1] < 3 or ref.shape[-1] < 3:
            raise ValueError("generation_metrics: EMD needs at least three components (xyz)")
        out.update(reduce(pairwise_emd_auction if auction else pairwise_emd,
                          sample[..., :3].contiguous(), ref[..., :3].contiguous(), "emd"))
    out.update(extra)
    return out


_jsd = jsd      # generation_metrics' keyword shadows the function
