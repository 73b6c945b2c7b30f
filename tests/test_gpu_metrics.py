"""GPU: the set-against-set Chamfer kernel (csrc/chamfer_cross.hip through
include/pcfm_chamfer_cross.h and pcfm.ops.chamfer_cross_forward) and the
generation metrics on it (pcfm/metrics.py) against

  * the N-D kernel pair by pair (existing code, bit-checked at D = 3 against the
    oracle-checked 3-D kernel): the same fp32 minima, their float64 mean;
  * float64 numpy brute force;
  * the C ABI's memory contract (the row runner of tests/test_gpu_abi_contract.py);
  * one-pair EMD calls, and the CPU backend end to end.

Shapes (s, r, n, m): the smallest case; a ragged query tail; a cloud spanning
two query blocks (the workspace path and the finalize kernel); an empty cloud; a
set against itself; and 130 x 127 small clouds, the smallest pair count at which
a block walks a tile of two partner clouds (csrc/chamfer_cross.hip choose_tile:
from 64 blocks per CU), 127 partners not being a multiple of it."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))

import guard_alloc  # noqa: E402,F401  (the allocator run_row places the arenas with)
from test_gpu_abi_contract import Row, run_row  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIMS = (2, 3, 5, 6)
SHAPES = [(1, 1, 1, 1, False), (3, 37, 257, 129, False), (2, 2, 2049, 300, False),
          (2, 3, 100, 0, False), (5, 5, 64, 64, True), (130, 127, 9, 5, False)]
SHAPE_IDS = ["x".join(map(str, s[:4])) + ("-self" if s[4] else "") for s in SHAPES]


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def cu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def np_(t):
    return t.detach().cpu().numpy()


def inputs(s, r, n, m, d, same):
    """Seeded sets a (s, n, d), b (r, m, d).  A third of each b cloud is copied
    from an a cloud (exact hits) and b[0] consists of points of a[0] only (all of
    them when m >= n): ba[0, 0] is an exact 0."""
    g = np.random.default_rng(1000 * d + 7 * s + 5 * r + 3 * n + m)
    a = g.standard_normal((s, n, d)).astype(np.float32)
    if same:
        return a, a
    b = g.standard_normal((r, m, d)).astype(np.float32)
    if n and m:
        k = min(n, m) // 3
        for j in range(r):
            b[j, :k] = a[j % s, :k]
        b[0] = a[0][np.arange(m) % n]
    return a, b


@functools.lru_cache(maxsize=None)
def case(shape, d):
    """(a, b, ab, ba): the inputs (numpy) and one run of the kernel (numpy), shared
    by the tests of a (shape, d) and never modified."""
    from pcfm import ops
    s, r, n, m, same = shape
    a, b = inputs(s, r, n, m, d, same)
    ta = cu(a)
    ab, ba = ops.chamfer_cross_forward(ta, ta if same else cu(b))
    assert ab.shape == ba.shape == (s, r) and ab.dtype == ba.dtype == torch.float32
    return a, b, np_(ab), np_(ba)


# ---- 1. against the N-D kernel, pair by pair ---------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_vs_nd_kernel_pair_by_pair(ops, shape, d):
    s, r, n, m, _ = shape
    a, b, ab, ba = case(shape, d)
    if n == 0 or m == 0:
        assert not ab.any() and not ba.any()
        return
    i, j = np.divmod(np.arange(s * r), r)
    ai, bj = cu(a[i]), cu(b[j])                      # every pair, index-expanded
    d1, d2 = torch.empty(s * r, n, device=DEV), torch.empty(s * r, m, device=DEV)
    i1 = torch.empty(s * r, n, dtype=torch.int32, device=DEV)
    i2 = torch.empty(s * r, m, dtype=torch.int32, device=DEV)
    assert ops._chamfer_nd_forward(ai, bj, d1, d2, i1, i2, d) == 1
    eab = (np_(d1).astype(np.float64).sum(1) / n).astype(np.float32).reshape(s, r)
    eba = (np_(d2).astype(np.float64).sum(1) / m).astype(np.float32).reshape(s, r)
    # the same fp32 minima; 1 ulp for a float64 summation order that is not numpy's
    np.testing.assert_array_max_ulp(ab, eab, maxulp=1)
    np.testing.assert_array_max_ulp(ba, eba, maxulp=1)
    assert ba[0, 0] == 0                             # b[0] lies inside a[0]
    if shape[4]:
        assert not np.diagonal(ab).any() and not np.diagonal(ba).any()
        np.testing.assert_array_equal(ab, ba.T)      # a set against itself


# ---- 2. against float64 brute force ---------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_vs_float64_brute_force(shape, d):
    s, r, n, m, _ = shape
    a, b, ab, ba = case(shape, d)
    if n == 0 or m == 0:
        assert not ab.any() and not ba.any()
        return
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    eab, eba = np.zeros((s, r)), np.zeros((s, r))
    for i in range(s):
        d2 = ((a64[i][None, :, None, :] - b64[:, None, :, :]) ** 2).sum(-1)   # (r, n, m)
        eab[i], eba[i] = d2.min(2).mean(1), d2.min(1).mean(1)
    # (D + 4) * 2^-24 <= 6e-7: the N-D test's (D + 3) * 2^-24 for the fp32 chain plus
    # the final rounding of the mean
    np.testing.assert_allclose(ab, eab, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ba, eba, rtol=1e-6, atol=0)


# ---- 3. determinism and the C ABI's memory contract -------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_two_calls_are_bit_equal(ops, shape, d):
    s, r, n, m, same = shape
    a, b, ab, ba = case(shape, d)
    ta = cu(a)
    tb = ta if same else cu(b)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                    # and on another stream
        ab2, ba2 = ops.chamfer_cross_forward(ta, tb)
    side.synchronize()
    np.testing.assert_array_equal(np_(ab2).view(np.int32), ab.view(np.int32))
    np.testing.assert_array_equal(np_(ba2).view(np.int32), ba.view(np.int32))


def cross_row(d, s, r, n, m):
    def build(seed):
        a, b = inputs(s + seed, r, n, m, d, False)   # seed 1: another draw, cut to shape
        return {"a": cu(a[:s]), "b": cu(b)}

    def call(dd):
        from pcfm import ops
        return list(ops.chamfer_cross_forward(dd["a"], dd["b"]))
    return Row(f"chamfer-cross-d{d}-s{s}r{r}n{n}m{m}", build, call, ["pcfm_chamfer_cross_fwd"])


CROSS_ROWS = [cross_row(d, *s) for d in (2, 6)
              for s in ((3, 37, 257, 129), (2, 2, 2049, 300), (2, 3, 100, 0), (130, 127, 9, 5))]


@pytest.mark.parametrize("row", CROSS_ROWS, ids=[r.id for r in CROSS_ROWS])
def test_memory_contract(ops, row, report):
    run_row(row, report)


def test_every_launching_cross_entry_is_in_a_row():
    from pcfm import _lib
    launching = {n for n in _lib.CROSS_SIGNATURES if n.endswith("_fwd")}
    assert launching == {e for r in CROSS_ROWS for e in r.entries}


def test_einval_launches_and_writes_nothing(ops):
    from pcfm import _lib
    a = torch.randn(2, 300, 4, device=DEV)
    ab, ba = torch.full((2, 2), 7.0, device=DEV), torch.full((2, 2), 7.0, device=DEV)
    with pytest.raises(_lib.PcfmError, match="unsupported dimension"):
        _lib.call("pcfm_chamfer_cross_fwd", a.data_ptr(), a.data_ptr(), 2, 2, 300, 300, 4,
                  ab.data_ptr(), ba.data_ptr(), None, 0, None)
    torch.cuda.synchronize()
    assert (ab == 7).all() and (ba == 7).all()


# ---- 4. pairwise_emd ----------------------------------------------------------------------------
def test_pairwise_emd_matches_one_pair_calls(ops):
    """Bit equality: in csrc/emd.hip's default (row-pass) form a batch element's
    arithmetic does not depend on the batch size -- every pass is grid
    (ceil(rows / 64), b) with the columns split over the block's 16 waves, the
    match/cost kernel grid (ceil(n / 256), ceil(m / 64), b) and the cost finalize
    one block per element over those partials.  (The split count S that
    depends on b sizes only matchcost's and its backward's partials.)"""
    from pcfm import metrics
    g = torch.Generator(device=DEV).manual_seed(12)
    n = 100
    x, y = torch.rand(3, n, 3, device=DEV, generator=g), torch.rand(4, n, 3, device=DEV,
                                                                    generator=g)
    m = metrics.pairwise_emd(x, y)
    assert m.shape == (3, 4) and m.dtype == torch.float32 and m.is_cuda
    for i in range(3):
        for j in range(4):
            _, c = ops.approxmatch_cost_forward(x[i:i + 1], y[j:j + 1], want_match=False)
            assert m[i, j] == c[0] / n, (i, j)       # xyz1 = x[i], xyz2 = y[j]
    # the chunking does not show: 4 pairs per call against all 12 in one
    four = metrics._emd_chunk_bytes(4, n, n, x)
    assert metrics._emd_pairs_per_chunk(12, n, n, four, x) == 4
    assert metrics._emd_pairs_per_chunk(12, n, n, 1 << 30, x) == 12
    assert torch.equal(metrics.pairwise_emd(x, y, max_bytes=four), m)
    with pytest.raises(ValueError):
        metrics.pairwise_emd(torch.rand(2, n, 6, device=DEV), torch.rand(2, n, 6, device=DEV))
    with pytest.raises(ValueError):
        metrics.pairwise_emd(x, y[:, :50].contiguous())


# ---- 5. end to end: HIP against the CPU backend ----------------------------------------------------
def _sets(seed, d):
    g = np.random.default_rng(seed)

    def clouds(k):
        return (g.standard_normal((k, 64, d)) * g.uniform(0.5, 1.5, (k, 1, 1))).astype(np.float32)
    return torch.from_numpy(clouds(7)), torch.from_numpy(clouds(5))


def _gap(m, dim):
    """Smallest relative gap between the minimum and its runner-up along dim."""
    v = torch.sort(m, dim=dim).values
    lo, up = (v[0], v[1]) if dim == 0 else (v[:, 0], v[:, 1])
    return float(((up - lo) / lo).min())


def _end_to_end(pairwise, x, y, tol, tag):
    from pcfm import metrics
    cpu = [pairwise(x, y), pairwise(x, x), pairwise(y, y)]
    # cov_* and 1nna_* are compared exactly: safe only when no decision is close, so
    # every argmin they take must beat its runner-up by 10 x the matrix tolerance
    j = torch.cat([torch.cat([cpu[1], cpu[0]], 1), torch.cat([cpu[0].t(), cpu[2]], 1)], 0).clone()
    j.fill_diagonal_(float("inf"))
    gap = min(_gap(cpu[0], 1), _gap(j, 0))
    print(f"{tag}: smallest argmin gap {gap:.3g}")
    assert gap > 10 * tol, gap
    xd, yd = x.to(DEV), y.to(DEV)
    hip = [pairwise(xd, yd), pairwise(xd, xd), pairwise(yd, yd)]
    for h, c in zip(hip, cpu):
        assert h.is_cuda
        np.testing.assert_allclose(np_(h), c.numpy(), rtol=tol, atol=0)
    hm, cm = metrics.mmd_cov(hip[0]), metrics.mmd_cov(cpu[0])
    hn, cn = metrics.one_nna(hip[1], hip[0], hip[2]), metrics.one_nna(*[cpu[k] for k in (1, 0, 2)])
    for k in ("mmd", "mmd_smp"):
        np.testing.assert_allclose(hm[k].item(), cm[k].item(), rtol=2 * tol)
    assert hm["cov"].item() == cm["cov"].item()
    for k in ("acc", "acc_gen", "acc_ref"):
        assert hn[k].item() == cn[k].item(), k
    return hm, hn


@pytest.mark.parametrize("d,seed", [(3, 300), (6, 600)])
def test_end_to_end_chamfer_vs_cpu_backend(ops, d, seed):
    from pcfm import metrics
    x, y = _sets(seed, d)
    hm, hn = _end_to_end(metrics.pairwise_chamfer, x, y, 1e-6, f"chamfer d={d}")
    out = metrics.generation_metrics(x.to(DEV), y.to(DEV), emd=False)
    assert sorted(out) == ["1nna_cd", "1nna_gen_cd", "1nna_ref_cd", "cov_cd", "mmd_cd",
                           "mmd_smp_cd"]
    assert all(v.is_cuda for v in out.values())
    assert out["mmd_cd"] == hm["mmd"] and out["cov_cd"] == hm["cov"]
    assert out["1nna_cd"] == hn["acc"] and out["1nna_gen_cd"] == hn["acc_gen"]


def test_end_to_end_emd_vs_cpu_backend(ops):
    from pcfm import metrics
    x, y = _sets(300, 3)
    # rtol 1e-4: the project's EMD bar (the kernels use the hardware exp)
    hm, hn = _end_to_end(metrics.pairwise_emd, x, y, 1e-4, "emd")
    x6 = torch.cat([x, torch.zeros_like(x)], dim=2).to(DEV)      # EMD reads xyz only
    y6 = torch.cat([y, torch.ones_like(y)], dim=2).to(DEV)
    out = metrics.generation_metrics(x6, y6)
    assert len(out) == 12
    assert out["mmd_emd"] == hm["mmd"] and out["cov_emd"] == hm["cov"]
    assert out["1nna_emd"] == hn["acc"] and out["1nna_ref_emd"] == hn["acc_ref"]


# ---- 6. timings (recorded, not asserted) -----------------------------------------------------------
def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


@pytest.mark.parametrize("d", [3, 6])
def test_timings_recorded(ops, report, d):
    """S = R = 128, N = M = 2048: ops.chamfer_cross_forward against the route the
    tree offered before it for the same two matrices -- the pairs index-expanded
    (a[i], b[j]: every cloud copied once per partner, 4096 pairs a batch) through
    ops._chamfer_nd_forward, then the two means.  One process, warm-up 3, HIP
    events, median of 7, the two routes alternated."""
    s = r = 128
    n = m = 2048
    g = torch.Generator(device=DEV).manual_seed(d)
    a = torch.randn(s, n, d, device=DEV, generator=g)
    b = torch.randn(r, m, d, device=DEV, generator=g)
    res = {}

    def cross():
        res["cross"] = ops.chamfer_cross_forward(a, b)

    def expanded(chunk=4096):
        ab = torch.empty(s * r, device=DEV)
        ba = torch.empty(s * r, device=DEV)
        for p0 in range(0, s * r, chunk):
            p = torch.arange(p0, min(p0 + chunk, s * r), device=DEV)
            ai, bj = a[torch.div(p, r, rounding_mode="floor")], b[p % r]
            k = p.numel()
            d1, d2 = torch.empty(k, n, device=DEV), torch.empty(k, m, device=DEV)
            i1 = torch.empty(k, n, dtype=torch.int32, device=DEV)
            i2 = torch.empty(k, m, dtype=torch.int32, device=DEV)
            assert ops._chamfer_nd_forward(ai, bj, d1, d2, i1, i2, d) == 1
            ab[p0:p0 + k], ba[p0:p0 + k] = d1.mean(dim=1), d2.mean(dim=1)
        res["expanded"] = (ab.view(s, r), ba.view(s, r))

    for _ in range(3):
        cross()
        expanded()
    torch.cuda.synchronize()
    # the same matrices: torch's fp32 mean of 2048 non-negative terms against the
    # float64 one is off by less than 2048 * 2^-24 whatever its summation order
    for x, y in zip(res["cross"], res["expanded"]):
        torch.testing.assert_close(x, y, rtol=2048 * 2.0 ** -24, atol=0)
    t_cross, t_exp = [], []
    for _ in range(7):
        t_cross.append(_ms(cross))
        t_exp.append(_ms(expanded))
    mc, me = float(np.median(t_cross)), float(np.median(t_exp))
    rec = {"cross_ms": mc, "expanded_nd_ms": me, "expanded_over_cross": me / mc,
           "expanded_spread": (max(t_exp) - min(t_exp)) / me,
           "cross_spread": (max(t_cross) - min(t_cross)) / mc,
           "cross_pairs_per_s": s * r / (mc * 1e-3), "expanded_pairs_per_s": s * r / (me * 1e-3)}
    print(f"d={d}", rec)
    report(f"chamfer_cross/timing_128x128x2048x2048_d{d}", rec)
