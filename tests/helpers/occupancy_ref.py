"""An independent reference for the occupancy counts (include/pcfm_occupancy.h)
and the Jensen-Shannon divergence of pcfm/metrics.py, float64 numpy, shared by
tests/test_occupancy_cpu.py and tests/test_gpu_occupancy.py.

  * kept_mask(r): the integer test a^2 + b^2 + c^2 <= (r-1)^2;
  * grid_coords(points, r): u = fma(p, r-1, (r-1)/2) as the float64 product and
    sum rounded to float32;
  * reference_nodes(points, r): the two-branch rule, the search as a float64
    np.argmin over ALL kept nodes in rising flat index (np.argmin returns the first
    minimum, i.e. the lowest flat index).  On LATTICE clouds (coordinates k / 32,
    k an integer, |k| <= 48) u = (r-1) k / 32 + (r-1) / 2 has five fractional bits,
    so u, every difference and every term of the chain are exact in float32 and in
    float64 alike: ties are true ties, and any correct implementation returns
    exactly these nodes;
  * nearest_ratio(points, r, nodes): for random float32 clouds, where the float32
    chain may pick a node a rounding away from the float64 nearest, the defining
    property -- per point of branch 2 the float64 squared distance from u (the
    float32 value, widened) to the assigned node over the smallest over the kept
    nodes; the largest such ratio;
  * jsd_ref(p, q): H(M) - (H(P) + H(Q)) / 2 in bits, float64.

PROPERTY_BOUND = 1 + 8 * 2^-24: the three roundings of the chain (dy * dy and the
two fma) for each of the two compared values, with margin.  (The differences
u - node round as well when |u - node| lies in a higher binade than |u|; counting
them, the first-order worst case is 10 * 2^-24.  The asserted bound is the
tighter one.)
"""
import numpy as np

PROPERTY_BOUND = 1.0 + 8.0 * 2.0 ** -24

KINDS = ("lattice48", "lattice16", "randn02", "randn", "cube")


def kept_mask(r):
    """(r, r, r) bool."""
    sq = (2 * np.arange(r, dtype=np.int64) - (r - 1)) ** 2
    return sq[:, None, None] + sq[None, :, None] + sq[None, None, :] <= (r - 1) ** 2


def lattice_cloud(seed, s, n, d, kmax):
    """(s, n, d) float32, every coordinate k / 32 with an integer |k| <= kmax: kmax =
    48 reaches three times the cube's half width (nearly every point takes branch
    2, ties included), kmax = 16 stays inside the cube."""
    g = np.random.default_rng(seed)
    return (g.integers(-kmax, kmax + 1, (s, n, d)) / 32.0).astype(np.float32)


def cloud(kind, seed, s, n, d):
    """The test clouds: the two lattices, randn * 0.2 (about a tenth of the points
    take branch 2 at r = 28), randn (nearly all) and the uniform cube (half)."""
    if kind.startswith("lattice"):
        return lattice_cloud(seed, s, n, d, int(kind[7:]))
    g = np.random.default_rng(seed)
    if kind == "cube":
        return (g.random((s, n, d)) - 0.5).astype(np.float32)
    x = g.standard_normal((s, n, d)).astype(np.float32)
    return x * np.float32(0.2) if kind == "randn02" else x


def grid_coords(points, r):
    """(S, N, D) float32 -> (S * N, 3) float32 grid coordinates."""
    pos = points[..., :3].reshape(-1, 3).astype(np.float64)
    return (pos * float(r - 1) + 0.5 * (r - 1)).astype(np.float32)


def rint_nodes(u, r):
    """Branch 1: (P, 3) int64 = clamp(rint(u), 0, r-1) (np.rint rounds half to even),
    and whether that node is kept."""
    c = np.clip(np.rint(u), 0, r - 1).astype(np.int64)
    return c, kept_mask(r)[c[:, 0], c[:, 1], c[:, 2]]


def _kept_nodes(r):
    """The kept nodes in rising flat index: flat (K,) int64, coordinates (K, 3) float64."""
    flat = np.flatnonzero(kept_mask(r).reshape(-1))
    ijk = np.stack(np.unravel_index(flat, (r, r, r)), axis=1).astype(np.float64)
    return flat, ijk


def _kept_sqdist(u, ijk):
    """u (P, 3) float64, ijk (K, 3) -> (P, K) float64 squared distances."""
    d = np.zeros((len(u), len(ijk)))
    for a in range(3):
        t = u[:, a, None] - ijk[None, :, a]
        d += t * t
    return d


def reference_nodes(points, r, chunk=128):
    """points (S, N, D) float32 -> (S * N,) int64 flat node index per point."""
    u = grid_coords(points, r)
    c, kept = rint_nodes(u, r)
    node = (c[:, 0] * r + c[:, 1]) * r + c[:, 2]
    search = np.flatnonzero(~kept)
    flat, ijk = _kept_nodes(r)
    u64 = u.astype(np.float64)
    for p0 in range(0, len(search), chunk):
        rows = search[p0:p0 + chunk]
        node[rows] = flat[np.argmin(_kept_sqdist(u64[rows], ijk), axis=1)]
    return node


def reference_counts(points, r):
    return np.bincount(reference_nodes(points, r), minlength=r ** 3).astype(np.int32)


def nearest_ratio(points, r, nodes, chunk=128):
    """nodes (S * N,) the assigned flat indices -> (largest ratio over the branch-2
    points, 1.0 without one; number of branch-2 points).  Branch-1 points must sit
    in rint(u), every point in a kept node: asserted here."""
    u = grid_coords(points, r)
    c, kept = rint_nodes(u, r)
    nodes = np.asarray(nodes).reshape(-1)
    assert kept_mask(r).reshape(-1)[nodes].all(), "a point counted in a node that is not kept"
    first = (c[:, 0] * r + c[:, 1]) * r + c[:, 2]
    assert np.array_equal(nodes[kept], first[kept]), "branch 1: not rint(u)"
    search = np.flatnonzero(~kept)
    _, ijk = _kept_nodes(r)
    u64 = u.astype(np.float64)
    worst = 1.0
    for p0 in range(0, len(search), chunk):
        rows = search[p0:p0 + chunk]
        got = np.stack(np.unravel_index(nodes[rows], (r, r, r)), axis=1).astype(np.float64)
        mine = ((u64[rows] - got) ** 2).sum(-1)
        low = _kept_sqdist(u64[rows], ijk).min(axis=1)
        assert (low > 0).all()          # a point outside the sphere is on no kept node
        worst = max(worst, float((mine / low).max()))
    return worst, len(search)


def jsd_ref(p, q):
    """Two count vectors -> the Jensen-Shannon divergence in bits, float64."""
    p = np.asarray(p, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    p, q = p / p.sum(), q / q.sum()

    def h(x):
        x = x[x > 0]
        return -(x * np.log2(x)).sum()
    return h((p + q) / 2) - (h(p) + h(q)) / 2
