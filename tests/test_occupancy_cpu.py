"""CPU: the occupancy counts (include/pcfm_occupancy.h, csrc/occupancy.hip) and the
Jensen-Shannon divergence the generation metrics take from them
(pcfm/metrics.py), without a GPU -- the fifth ABI table, the host plan and the
host-side refusals, the wrappers' refusals, the CPU backend against the float64
reference of tests/helpers/occupancy_ref.py, jsd_from_counts, the jsd keyword of
generation_metrics, and the resources of the shipped kernels."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import codeobj  # noqa: E402
import occupancy_ref as oref  # noqa: E402

from pcfm import _lib, cpu_ops, metrics, ops  # noqa: E402

HEADER = os.path.join(REPO, "include", "pcfm_occupancy.h")
OCC = sorted(_lib.OCCUPANCY_SIGNATURES)
THREADS, BLOCK_CAP = 1024, 256      # csrc/occupancy.hip: points per block and round, the cap


# ---- 1. the fifth ABI table --------------------------------------------------------
def test_header_and_binding_agree():
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(pcfm_[a-z0-9_]+)\s*\(", text))) == OCC
    for other in (_lib.SIGNATURES, _lib.ND_SIGNATURES, _lib.CROSS_SIGNATURES,
                  _lib.FPS_SIGNATURES):
        assert not set(_lib.OCCUPANCY_SIGNATURES) & set(other)
    lib = _lib.load()
    for name in OCC:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.OCCUPANCY_SIGNATURES[name][1], name  # declared by load()
        assert fn.restype == _lib.OCCUPANCY_SIGNATURES[name][0], name
    assert lib.pcfm_occupancy_abi_version() == 1 == _lib.OCCUPANCY_ABI_VERSION
    # the four older versions are untouched by the new sibling header
    assert lib.pcfm_abi_version() == _lib.ABI_VERSION == 20
    assert lib.pcfm_chamfer_nd_abi_version() == _lib.ND_ABI_VERSION == 1
    assert lib.pcfm_chamfer_cross_abi_version() == _lib.CROSS_ABI_VERSION == 1
    assert lib.pcfm_fps_abi_version() == _lib.FPS_ABI_VERSION == 1


# ---- 2. the host plan and the host-side refusals (no GPU is touched) ------------------
def test_plan_and_refusals_on_the_host():
    lib = _lib.load()
    q = lib.pcfm_occupancy_workspace_bytes

    def err():
        return lib.pcfm_last_error().decode()

    def counts(s, n, d, r, ws_bytes=0):
        return lib.pcfm_occupancy_counts(None, s, n, d, r, None, None, ws_bytes, None)

    for d in range(-1, 9):
        for r in range(-1, 40):
            assert lib.pcfm_occupancy_supported(d, r) == int(d in (3, 5, 6) and 3 <= r <= 32)
    for bad in ((-1, 10), (2, -10)):
        assert counts(*bad, 3, 28) == -1 and "negative size" in err()
        assert q(*bad, 3, 28) == 0
    for d, r in ((2, 28), (4, 28), (0, 28), (7, 28), (3, 2), (3, 33), (6, 0), (6, -5)):
        assert counts(2, 10, d, r, 1 << 40) == -1 and "unsupported" in err()
        assert q(2, 10, d, r) == 0
    # s * n stays below 2^31
    assert counts(1 << 16, 1 << 15, 3, 28, 1 << 40) == -1 and "too large" in err()
    assert q(1 << 16, 1 << 15, 3, 28) == 0
    assert q((1 << 16) - 1, 1 << 15, 3, 28) == BLOCK_CAP * 28 ** 3 * 4
    # one partial histogram per counting block; the blocks are a function of s * n alone:
    # one per THREADS points, BLOCK_CAP at most -- whatever d and however s * n splits
    for r in (3, 9, 28, 32):
        for total, blocks in ((1, 1), (THREADS, 1), (THREADS + 1, 2), (3 * THREADS, 3),
                              (BLOCK_CAP * THREADS, BLOCK_CAP),
                              (BLOCK_CAP * THREADS + 1, BLOCK_CAP), (20_000_000, BLOCK_CAP)):
            for d in (3, 5, 6):
                assert q(1, total, d, r) == blocks * r ** 3 * 4, (r, total, d)
        assert q(1000, 2048, 6, r) == q(2048, 1000, 3, r) == q(1, 2048000, 5, r)
        assert q(0, 100, 3, r) == 0 and q(100, 0, 3, r) == 0
    need = 2 * 28 ** 3 * 4
    assert counts(2, 1000, 6, 28, need - 1) == -1 and f"workspace {need - 1} < {need}" in err()
    with pytest.raises(_lib.PcfmError, match="workspace"):
        _lib.call("pcfm_occupancy_counts", None, 2, 1000, 6, 28, None, None, 0, None)


def test_wrapper_refusals():
    a = torch.zeros(2, 5, 3)
    for bad in (a.double(), torch.zeros(5, 3), torch.zeros(2, 5, 4), torch.zeros(2, 5, 2),
                torch.zeros(5, 2, 3).transpose(0, 1)):
        with pytest.raises(RuntimeError):
            ops.occupancy_counts(bad, 28)
    for r in (2, 33, 0, -1):
        with pytest.raises(RuntimeError):
            ops.occupancy_counts(a, r)
        with pytest.raises(ValueError):
            metrics.occupancy_counts(a, r)
    for bad in (torch.zeros(5, 3), torch.zeros(2, 5, 2), torch.zeros(2, 5, 4)):
        with pytest.raises(ValueError):
            metrics.occupancy_counts(bad)
    # no point: all zeros
    for empty in (torch.zeros(0, 5, 3), torch.zeros(4, 0, 6)):
        c = ops.occupancy_counts(empty, 9)
        assert c.dtype == torch.int32 and c.shape == (729,) and int(c.abs().sum()) == 0
    # a strided view is made contiguous by the metrics wrapper, not by ops
    c = metrics.occupancy_counts(torch.zeros(5, 2, 3).transpose(0, 1))
    assert c.shape == (28 ** 3,) and int(c.sum()) == 10


# ---- 3. the kept nodes -------------------------------------------------------------------
def test_kept_nodes():
    kept = oref.kept_mask(28)
    assert kept.sum() == 10144 and kept.size == 21952
    sq = (2 * np.arange(28) - 27) ** 2
    assert not (sq[:, None, None] + sq[None, :, None] + sq[None, None, :] == 27 ** 2).any()
    # the float32 mask of the published code, norm(grid) <= 0.5, is the same set at r = 28
    g = np.linspace(-0.5, 0.5, 28, dtype=np.float32)
    norm = np.sqrt(g[:, None, None] ** 2 + g[None, :, None] ** 2 + g[None, None, :] ** 2)
    assert np.array_equal(norm <= np.float32(0.5), kept)
    # six nodes exactly on the sphere (the face centres) where r is odd: the test is <=
    for r in (3, 9, 17):
        sq = (2 * np.arange(r) - (r - 1)) ** 2
        on = sq[:, None, None] + sq[None, :, None] + sq[None, None, :] == (r - 1) ** 2
        assert on.sum() >= 6 and oref.kept_mask(r)[on].all()
        mid = (r - 1) // 2
        assert on[0, mid, mid] and on[mid, r - 1, mid]
    for r in range(3, 33):
        assert np.array_equal(cpu_ops._occupancy_kept(r).numpy(), oref.kept_mask(r))
    assert oref.kept_mask(2).sum() == 0


# ---- 4. the CPU backend against the reference: lattice clouds, exact --------------------
def _cpu_counts(pts, r):
    c = ops.occupancy_counts(torch.from_numpy(np.ascontiguousarray(pts)), r)
    assert c.dtype == torch.int32 and tuple(c.shape) == (r ** 3,)
    return c.numpy()


LATTICE = [(48, 3, 1500, 3, 28), (16, 3, 1500, 6, 28), (48, 2, 700, 5, 3), (48, 2, 700, 3, 9),
           (48, 2, 700, 6, 17), (48, 2, 700, 3, 32), (16, 2, 700, 3, 9), (16, 2, 700, 5, 32)]


@pytest.mark.parametrize("kmax,s,n,d,r", LATTICE)
def test_cpu_lattice_clouds_exact(kmax, s, n, d, r):
    pts = oref.lattice_cloud(100 * kmax + r, s, n, d, kmax)
    u = oref.grid_coords(pts, r)
    # the lattice is exact: u is what float64 gives, with five fractional bits
    assert np.array_equal(u.astype(np.float64),
                          pts[..., :3].reshape(-1, 3).astype(np.float64) * (r - 1) + (r - 1) / 2)
    assert np.array_equal(u * 32, np.rint(u * 32))
    _, kept = oref.rint_nodes(u, r)
    half = (np.abs(u - np.floor(u)) == 0.5).any(axis=1)
    print("branch 2:", 1 - kept.mean(), "an axis half-way:", half.mean())
    if kmax == 48 and r == 28:
        assert kept.mean() < 0.1 and half.mean() > 0.03
    if kmax == 16 and r == 28:
        assert kept.mean() > 0.4
    want = oref.reference_nodes(pts, r)
    got = cpu_ops.occupancy_nodes(torch.from_numpy(pts), r).numpy().reshape(-1)
    bad = np.flatnonzero(got != want)
    assert not len(bad), f"first of {len(bad)} differing points: {bad[0]}, u = {u[bad[0]]}"
    assert np.array_equal(_cpu_counts(pts, r), oref.reference_counts(pts, r))


def test_cpu_half_way_points_and_ties():
    """Points placed by hand at r = 28 (node = (p + 0.5) * 27): half-way between two
    nodes rint goes to the even one; outside the sphere, between two kept nodes at
    one distance, the lower flat index wins."""
    r = 28

    def node(*p):
        return int(cpu_ops.occupancy_nodes(torch.tensor([[p]], dtype=torch.float32), r)[0, 0])

    def flat(i, j, k):
        return (i * r + j) * r + k
    assert node(0.0, 0.0, 0.0) == flat(14, 14, 14)            # u = 13.5: half to even
    assert node(1 / 27, 0.0, 0.0) == flat(14, 14, 14)         # u.x = 14.5: even again
    assert node(2 / 27, 0.0, 0.0) == flat(16, 14, 14)         # u.x = 15.5
    assert node(-1 / 27, -1 / 27, -1 / 27) == flat(12, 12, 12)
    # far out on the x axis: u = (13.5 + 27 * 3, 13.5, 13.5).  The four nodes
    # (27, 13..14, 13..14) are not kept (27^2 + 1 + 1 > 27^2); the nearest kept nodes
    # are (26, 13..14, 13..14), all at one distance, and the lowest index wins
    kept = oref.kept_mask(r)
    assert not kept[27, 13, 13] and kept[26, 13, 13]
    assert node(3.0, 0.0, 0.0) == flat(26, 13, 13)
    assert node(-3.0, 0.0, 0.0) == flat(1, 13, 13)
    assert node(0.0, 0.0, 3.0) == flat(13, 13, 26)
    # the reference agrees on all of them
    pts = np.array([[[3, 0, 0], [-3, 0, 0], [0, 0, 3], [0, 0, 0], [2 / 27, 0, 0]]], np.float32)
    assert np.array_equal(cpu_ops.occupancy_nodes(torch.from_numpy(pts), r).numpy().reshape(-1),
                          oref.reference_nodes(pts, r))


# ---- 5. the property on random clouds -----------------------------------------------------
@pytest.mark.parametrize("kind,s,n,d,r", [("randn02", 2, 1500, 3, 28), ("randn", 2, 1000, 6, 28),
                                          ("cube", 2, 1500, 5, 28), ("randn", 2, 1000, 3, 9),
                                          ("cube", 2, 1000, 6, 32), ("randn", 3, 500, 5, 3)])
def test_cpu_random_clouds_property(kind, s, n, d, r):
    pts = oref.cloud(kind, 7 * r + n, s, n, d)
    nodes = cpu_ops.occupancy_nodes(torch.from_numpy(pts), r).numpy()
    ratio, searched = oref.nearest_ratio(pts, r, nodes)
    print(kind, "branch 2:", searched / (s * n), "worst ratio - 1:", ratio - 1.0)
    assert searched > 0
    assert ratio <= oref.PROPERTY_BOUND
    # the reference itself satisfies its own property exactly
    assert oref.nearest_ratio(pts, r, oref.reference_nodes(pts, r))[0] == 1.0
    # the counts are the histogram of the nodes
    assert np.array_equal(_cpu_counts(pts, r), np.bincount(nodes.reshape(-1), minlength=r ** 3))


# ---- 6. sums, zeros, additivity, permutations -----------------------------------------------
@pytest.mark.parametrize("r", [3, 28])
def test_cpu_sums_zeros_additivity_permutations(r):
    a = oref.cloud("randn", 11, 3, 400, 6)
    b = oref.cloud("cube", 12, 2, 400, 6)
    ca, cb = _cpu_counts(a, r), _cpu_counts(b, r)
    assert ca.sum() == 1200 and cb.sum() == 800
    out = ~oref.kept_mask(r).reshape(-1)
    assert not ca[out].any() and not cb[out].any()
    assert np.array_equal(_cpu_counts(np.concatenate([a, b]), r), ca + cb)
    g = np.random.default_rng(3)
    assert np.array_equal(_cpu_counts(a[g.permutation(3)], r), ca)
    assert np.array_equal(_cpu_counts(a[:, g.permutation(400)], r), ca)
    assert np.array_equal(_cpu_counts(a.reshape(1, 1200, 6), r), ca)
    # the colour takes no part
    assert np.array_equal(_cpu_counts(np.ascontiguousarray(a[..., :3]), r), ca)
    # non-finite coordinates: a kept node all the same, and the sum holds
    bad = a.copy()
    bad[0, 5, 0], bad[1, 7, 1], bad[2, 0, 2], bad[2, 9, 2] = np.nan, np.inf, -np.inf, np.nan
    cn = _cpu_counts(bad, r)
    assert cn.sum() == 1200 and not cn[out].any()


# ---- 7. the divergence ------------------------------------------------------------------------
def test_jsd_from_counts():
    assert {"occupancy_counts", "jsd_from_counts", "jsd"} <= set(metrics.__all__)
    g = np.random.default_rng(5)
    n = 28 ** 3

    def counts():
        c = np.zeros(n, dtype=np.int64)
        c[g.choice(n, 1000, replace=False)] = g.integers(1, 5000, 1000)
        return c
    p, q = counts(), counts()
    tp, tq = torch.from_numpy(p), torch.from_numpy(q)
    v = metrics.jsd_from_counts(tp, tq)
    assert v.dtype == torch.float64 and v.dim() == 0
    assert 0.0 < float(v) < 1.0
    assert abs(float(v) - oref.jsd_ref(p, q)) <= 1e-12
    # symmetric, bit for bit
    assert torch.equal(v, metrics.jsd_from_counts(tq, tp))
    # int32 counts (what occupancy_counts returns) give the same bits
    assert torch.equal(v, metrics.jsd_from_counts(tp.int(), tq.int()))
    # equal histograms, however scaled: exactly 0
    for k in (1, 2, 3, 7, 1000):
        assert float(metrics.jsd_from_counts(tp, tp * k)) == 0.0
        assert float(metrics.jsd_from_counts(tp * k, tp * 3)) == 0.0
    # disjoint supports: exactly 1
    lo, hi = p.copy(), q.copy()
    lo[n // 2:], hi[: n // 2] = 0, 0
    assert float(metrics.jsd_from_counts(torch.from_numpy(lo), torch.from_numpy(hi))) == 1.0
    assert float(metrics.jsd_from_counts(torch.tensor([3, 0]), torch.tensor([0, 11]))) == 1.0
    # more random pairs against the reference, sparse and dense
    for _ in range(5):
        p, q = counts(), counts()
        q[: n // 3] = p[: n // 3]
        got = float(metrics.jsd_from_counts(torch.from_numpy(p), torch.from_numpy(q)))
        assert abs(got - oref.jsd_ref(p, q)) <= 1e-12
    for bad in ((torch.zeros(4), torch.ones(4)), (torch.ones(4), torch.zeros(4)),
                (torch.ones(4), torch.ones(5)), (torch.ones(2, 2), torch.ones(2, 2))):
        with pytest.raises(ValueError):
            metrics.jsd_from_counts(*bad)


def test_jsd_of_two_sets():
    a = torch.from_numpy(oref.cloud("randn02", 21, 4, 300, 6))
    b = torch.from_numpy(oref.cloud("cube", 22, 3, 500, 3))
    v = metrics.jsd(a[..., :3].contiguous(), b)
    exp = oref.jsd_ref(oref.reference_counts(a.numpy(), 28), oref.reference_counts(b.numpy(), 28))
    assert abs(float(v) - exp) <= 1e-12
    assert torch.equal(v, metrics.jsd_from_counts(metrics.occupancy_counts(a),
                                                  metrics.occupancy_counts(b)))
    assert float(metrics.jsd(a, a)) == 0.0
    assert float(metrics.jsd(a, torch.cat([a, a]))) == 0.0          # sizes differ: absorbed
    assert float(metrics.jsd(a, a, resolution=9)) == 0.0
    assert float(metrics.jsd(a, a + 2.0, resolution=9)) > 0.0
    assert not torch.equal(metrics.jsd(a, b[..., :3].contiguous().expand(3, 500, 3),
                                       resolution=9), v)


# ---- 8. generation_metrics ---------------------------------------------------------------------
def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_generation_metrics_jsd_keyword():
    g = torch.Generator().manual_seed(6)
    s, r = torch.randn(4, 96, 6, generator=g) * 0.3, torch.randn(3, 80, 6, generator=g) * 0.3
    base = metrics.generation_metrics(s, r, emd=False)
    # jsd=False (the default) returns the dict of before
    _same(base, metrics.generation_metrics(s, r, emd=False, jsd=False))
    got = metrics.generation_metrics(s, r, emd=False, jsd=True)
    assert set(got) - set(base) == {"jsd"} and set(base) <= set(got)
    _same({k: got[k] for k in base}, base)
    assert torch.equal(got["jsd"], metrics.jsd(s, r))
    assert got["jsd"].dtype == torch.float64 and 0.0 < float(got["jsd"]) <= 1.0
    assert torch.equal(metrics.generation_metrics(s, r, emd=False, jsd=True, jsd_resolution=9)
                       ["jsd"], metrics.jsd(s, r, 9))
    # with n_points: taken BEFORE the subsample, on the clouds as given
    m = 24
    sub = metrics.generation_metrics(s, r, n_points=m, jsd=True)
    assert len(sub) == 13
    assert torch.equal(sub["jsd"], metrics.jsd(s, r))
    assert not torch.equal(sub["jsd"], metrics.jsd(metrics.subsample(s, m),
                                                   metrics.subsample(r, m)))
    _same({k: v for k, v in sub.items() if k != "jsd"},
          metrics.generation_metrics(s, r, n_points=m))
    # D = 2: Chamfer runs, the grid does not
    s2, r2 = s[..., :2].contiguous(), r[..., :2].contiguous()
    assert len(metrics.generation_metrics(s2, r2, emd=False)) == 6
    with pytest.raises(ValueError):
        metrics.generation_metrics(s2, r2, emd=False, jsd=True)
    with pytest.raises(ValueError):
        metrics.generation_metrics(s, r, emd=False, jsd=True, jsd_resolution=33)


# ---- 9. the shipped device code -------------------------------------------------------------------
def test_shipped_occupancy_kernels_have_no_scratch(tmp_path):
    assert codeobj.available(), "ROCm LLVM tools absent"
    found = {}
    for co in codeobj.extract(_lib.LIB_PATH, str(tmp_path)):
        for name, res in codeobj.kernel_resources(co).items():
            m = re.search(r"occ_(count|finalize)_kernel", name)
            if m:
                assert m.group(1) not in found, name
                found[m.group(1)] = res
    assert sorted(found) == ["count", "finalize"]
    for key, res in found.items():
        assert res["scratch"] == 0, (key, res)
    # the histogram and the search queue are dynamic LDS (set at launch: 155 652 bytes at
    # r = 32, under the 159 KiB a kernel may ask for); one block fills a CU
    assert found["count"]["lds"] <= 1024 and found["count"]["wg"] == THREADS
    assert found["finalize"]["wg"] == 1024 and found["finalize"]["lds"] == 16 * 64 * 4
