"""GPU: the approximate EMD over D-component points (include/pcfm_emd_nd.h,
csrc/emd.hip) -- against the float64 reference of tests/helpers/emd_nd_ref.py,
against the 3-D kernels bit for bit, the gradients against the float64 closed
form, the contract (two runs, a side stream, the batch, degenerate sizes, the
refusals, guarded and stale memory), the fused PH 3 against the unfused passes,
the metrics on top, and the timings."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import emd_nd_ref as ndref  # noqa: E402
from test_gpu_abi_contract import Row, run_row  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-4        # the project's EMD bar (EMD_REF_BOUND["f32"] in tests/test_gpu_ops.py)


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def np_(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def urand(seed, *shape):
    return torch.rand(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


@functools.lru_cache(maxsize=None)
def reference(b, n, m, d):
    a, c = ndref.clouds(b, n, m, d)
    ref = ndref.approxmatch(a, c)
    ref.setflags(write=False)
    return a, c, ref


# ---- 1. against the float64 reference ---------------------------------------------------------
@pytest.mark.parametrize("b,n,m,d", ndref.CASES)
def test_vs_fp64_reference(ops, b, n, m, d):
    """The match approxmatch_cost_forward_nd writes against the numpy fp64 reference
    of what the kernels define (the D-component fp32 chain for d2, the float32 exp2
    argument, exp2 rounded to float32; every sum, division and clamp in fp64), on
    emd_ref.GPU_CASES' shapes at D = 2, 5, 6: max |x - ref| / max ref <= 1e-4, the
    per-batch totals to ten times that (the form of test_emd_vs_fp64_reference), and
    the cost without the match equal in bits to the cost with it."""
    a, c, ref = reference(b, n, m, d)
    match, cost = ops.approxmatch_cost_forward_nd(cu(a), cu(c))
    x = np_(match)
    assert x.shape == ref.shape and np.isfinite(x).all()
    err = ndref.rel_err(x, ref)
    print(f"emd_nd_ref D={d} {(b, n, m)}: {err:.3e}")
    assert err <= BOUND, err
    np.testing.assert_allclose(x.sum(axis=(1, 2), dtype=np.float64), ref.sum(axis=(1, 2)),
                               rtol=10 * BOUND)
    none, cost2 = ops.approxmatch_cost_forward_nd(cu(a), cu(c), want_match=False)
    assert none is None and same(cost, cost2)
    # the fused cost and matchcost of the written match against the float64 sum over that
    # match: summation order only (all terms >= 0), the 3-D test's 1e-5
    own = ndref.matchcost(a, c, x)
    np.testing.assert_allclose(np_(cost), own, rtol=1e-5)
    np.testing.assert_allclose(np_(ops.matchcost_forward_nd(cu(a), cu(c), match)), own, rtol=1e-5)


# ---- 2. against the 3-D kernels, bit for bit --------------------------------------------------
def _three_d(ops, a3, c3, gc):
    match, cost = ops.approxmatch_cost_forward(a3, c3)
    return (match, cost, ops.matchcost_forward(a3, c3, match),
            *ops.matchcost_backward(gc, a3, c3, match))


def _n_d(ops, a, c, gc):
    match, cost = ops.approxmatch_cost_forward_nd(a, c)
    return (match, cost, ops.matchcost_forward_nd(a, c, match),
            *ops.matchcost_backward_nd(gc, a, c, match))


@pytest.mark.parametrize("b,n,m", [(3, 100, 37), (1, 70, 2200)])
def test_bit_identical_to_the_3d_kernels(ops, b, n, m):
    a3, c3, gc = urand(1, b, n, 3), urand(2, b, m, 3), urand(3, b)
    want = _three_d(ops, a3, c3, gc)
    # D = 3 through the N-D entries
    for x, y in zip(_n_d(ops, a3, c3, gc), want):
        assert same(x, y)
    # D = 5, 6 with trailing components that are one constant in both clouds:
    # fma(0, 0, acc) is exact, so d2 is the xyz chain's
    for d, const in ((5, 0.625), (6, 0.3), (6, 0.0)):
        a = torch.cat([a3, torch.full((b, n, d - 3), const, device=DEV)], dim=2).contiguous()
        c = torch.cat([c3, torch.full((b, m, d - 3), const, device=DEV)], dim=2).contiguous()
        match, cost, cost_m, g1, g2 = _n_d(ops, a, c, gc)
        assert same(match, want[0]) and same(cost, want[1]) and same(cost_m, want[2])
        assert same(g1[..., :3].contiguous(), want[3]) and same(g2[..., :3].contiguous(), want[4])
        assert not g1[..., 3:].any() and not g2[..., 3:].any()
    # D = 2 equals the 3-D entry on the clouds padded with z = 0
    a2, c2 = a3[..., :2].contiguous(), c3[..., :2].contiguous()
    pad = _three_d(ops, torch.cat([a2, torch.zeros(b, n, 1, device=DEV)], dim=2).contiguous(),
                   torch.cat([c2, torch.zeros(b, m, 1, device=DEV)], dim=2).contiguous(), gc)
    match, cost, cost_m, g1, g2 = _n_d(ops, a2, c2, gc)
    assert same(match, pad[0]) and same(cost, pad[1]) and same(cost_m, pad[2])
    assert same(g1, pad[3][..., :2].contiguous()) and same(g2, pad[4][..., :2].contiguous())
    assert not pad[3][..., 2].any() and not pad[4][..., 2].any()


# ---- 3. backward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 6])
@pytest.mark.parametrize("b,n,m", [(3, 100, 37), (2, 37, 700)])
def test_backward_vs_float64_closed_form(ops, b, n, m, d):
    """grad1, grad2 against the closed form in float64 from the kernel's own match:
    rtol 1e-4, atol 1e-5, the 3-D backward's bounds (tests/test_gpu_ops.py)."""
    a, c, _ = reference(b, n, m, d)
    gc = np.random.default_rng(n + m + d).random(b).astype(np.float32)
    match, _ = ops.approxmatch_cost_forward_nd(cu(a), cu(c))
    g1, g2 = ops.matchcost_backward_nd(cu(gc), cu(a), cu(c), match)
    e1, e2 = ndref.matchcost_grads(gc, a, c, np_(match))
    print(f"emd_nd_bwd D={d} {(b, n, m)}: grad1 {np.abs(np_(g1) - e1).max():.3e} of "
          f"{np.abs(e1).max():.3e}, grad2 {np.abs(np_(g2) - e2).max():.3e} of "
          f"{np.abs(e2).max():.3e}")
    assert g1.shape == (b, n, d) and g2.shape == (b, m, d)
    np.testing.assert_allclose(np_(g1), e1, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np_(g2), e2, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("d", [2, 6])
def test_earth_mover_distance_nd_under_autograd(ops, d):
    from PyTorchEMD.emd_nd import earth_mover_distance_nd
    b, n = 2, 300
    a, c, w = urand(4, b, n, d), urand(5, b, n, d), urand(6, b)
    p1, p2 = a.clone().requires_grad_(True), c.clone().requires_grad_(True)
    dist = earth_mover_distance_nd(p1, p2)
    match, cost = ops.approxmatch_cost_forward_nd(a, c)
    assert same(dist.detach(), cost / float(n))
    (dist * w).sum().backward()
    e1, e2 = ndref.matchcost_grads(np_(w) / n, np_(a), np_(c), np_(match))
    np.testing.assert_allclose(np_(p1.grad), e1, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np_(p2.grad), e2, rtol=1e-4, atol=1e-5)
    # (B, D, N) input, and a forward that needs no gradient (no match is kept)
    dt = earth_mover_distance_nd(a.transpose(1, 2), c.transpose(1, 2), transpose=True)
    assert same(dt, dist.detach()) and not dt.requires_grad
    # under autocast the inputs are cast to float32
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert same(earth_mover_distance_nd(a, c), dist.detach())


# ---- 4. the contract --------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 5, 6])
def test_two_runs_a_side_stream_and_the_batch(ops, d):
    b, n, m = 3, 130, 300
    a, c, gc = urand(7, b, n, d), urand(8, b, m, d), urand(9, b)
    first = _n_d(ops, a, c, gc)
    for x, y in zip(_n_d(ops, a, c, gc), first):
        assert same(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = _n_d(ops, a, c, gc)
    side.synchronize()
    for x, y in zip(on_side, first):
        assert same(x, y)
    # one batch element alone: the same bits as inside the batch
    alone = _n_d(ops, a[1:2].contiguous(), c[1:2].contiguous(), gc[1:2].contiguous())
    for x, y in zip(alone, first):
        assert same(x, y[1:2].contiguous())


@pytest.mark.parametrize("d", [2, 5, 6])
@pytest.mark.parametrize("b,n,m", [(2, 1, 1), (2, 1, 50), (2, 50, 1)])
def test_single_points(ops, b, n, m, d):
    a, c, ref = reference(b, n, m, d)
    match, cost = ops.approxmatch_cost_forward_nd(cu(a), cu(c))
    assert ndref.rel_err(np_(match), ref) <= BOUND
    np.testing.assert_allclose(np_(cost), ndref.matchcost(a, c, np_(match)), rtol=1e-5)
    gc = np.ones(b, np.float32)
    g1, g2 = ops.matchcost_backward_nd(cu(gc), cu(a), cu(c), match)
    e1, e2 = ndref.matchcost_grads(gc, a, c, np_(match))
    np.testing.assert_allclose(np_(g1), e1, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(np_(g2), e2, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("d", [2, 6])
def test_empty_inputs(ops, d):
    for b, n, m in ((2, 0, 5), (2, 5, 0), (2, 0, 0), (0, 5, 5)):
        a, c = torch.zeros(b, n, d, device=DEV), torch.zeros(b, m, d, device=DEV)
        match, cost = ops.approxmatch_cost_forward_nd(a, c)
        assert match.shape == (b, m, n) and cost.shape == (b,) and not cost.any()
        assert not ops.matchcost_forward_nd(a, c, match).any()
        g1, g2 = ops.matchcost_backward_nd(torch.ones(b, device=DEV), a, c, match)
        assert g1.shape == (b, n, d) and g2.shape == (b, m, d) and not g1.any() and not g2.any()


def test_refusals_leave_the_outputs_untouched(ops):
    from pcfm import _lib
    b, n, m, d = 2, 40, 30, 6
    a, c, gc = urand(10, b, n, d), urand(11, b, m, d), urand(12, b)
    need = _lib.query("pcfm_emd_nd_workspace_bytes", b, n, m, d)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    mark = 7.25
    match, cost = torch.full((b, m, n), mark, device=DEV), torch.full((b,), mark, device=DEV)
    g1, g2 = torch.full((b, n, d), mark, device=DEV), torch.full((b, m, d), mark, device=DEV)
    p = torch.Tensor.data_ptr
    for bad_d, bad_ws, text in ((4, need, "unsupported dimension"), (7, need, "unsupported"),
                                (d, need - 1, "workspace")):
        with pytest.raises(_lib.PcfmError, match=text):
            _lib.call("pcfm_emd_nd_approxmatch_cost_f32", p(a), p(c), b, n, m, bad_d, p(match),
                      p(cost), p(ws), bad_ws, 0)
        with pytest.raises(_lib.PcfmError, match=text):
            _lib.call("pcfm_emd_nd_matchcost_f32", p(a), p(c), p(match), b, n, m, bad_d, p(cost),
                      p(ws), bad_ws, 0)
        with pytest.raises(_lib.PcfmError, match=text):
            _lib.call("pcfm_emd_nd_matchcost_bwd_f32", p(gc), p(a), p(c), p(match), b, n, m, bad_d,
                      p(g1), p(g2), p(ws), bad_ws, 0)
    with pytest.raises(_lib.PcfmError, match="negative size"):
        _lib.call("pcfm_emd_nd_approxmatch_cost_f32", p(a), p(c), b, -1, m, d, p(match), p(cost),
                  p(ws), need, 0)
    with pytest.raises(_lib.PcfmError, match="cost is required"):
        _lib.call("pcfm_emd_nd_approxmatch_cost_f32", p(a), p(c), b, n, m, d, p(match), None,
                  p(ws), need, 0)
    torch.cuda.synchronize()
    for t in (match, cost, g1, g2):
        assert bool((t == mark).all())
    assert not ws.any()


def emd_nd_row(b, n, m, d):
    def build(seed):
        g = torch.Generator(device=DEV).manual_seed(830 + seed)
        return {"a": torch.rand(b, n, d, device=DEV, generator=g),
                "c": torch.rand(b, m, d, device=DEV, generator=g),
                "gc": torch.rand(b, device=DEV, generator=g)}

    def call(t):
        from pcfm import ops
        a, c = t["a"], t["c"]
        match, cost = ops.approxmatch_cost_forward_nd(a, c, True)
        _, cost2 = ops.approxmatch_cost_forward_nd(a, c, False)
        return [match, cost, cost2, ops.matchcost_forward_nd(a, c, match),
                *ops.matchcost_backward_nd(t["gc"], a, c, match)]
    return Row(f"emd-nd-d{d}-b{b}n{n}m{m}", build, call,
               ["pcfm_emd_nd_approxmatch_cost_f32", "pcfm_emd_nd_matchcost_f32",
                "pcfm_emd_nd_matchcost_bwd_f32"])


# ragged row tails (77 = 64 + 13 rows; 300 = 4 * 64 + 44) and column tails (300 and 77
# columns over 16 waves: 18-19 and 4-5 each; 300 = 9 * 32 + 12 in the match write)
ND_ROWS = [emd_nd_row(2, 77, 300, 6), emd_nd_row(2, 300, 77, 5), emd_nd_row(3, 100, 37, 2)]


@pytest.mark.parametrize("row", ND_ROWS, ids=[r.id for r in ND_ROWS])
def test_memory_contract(ops, row, report):
    """Row / run_row of tests/test_gpu_abi_contract.py: plain twice, under the guarded
    allocator (guards intact, no poison left, the plain run's bits), and with the stale
    arenas -- workspace included -- of a call on other inputs."""
    run_row(row, report)


# ---- 5. the fused PH 3 against the unfused passes ------------------------------------------------------
def test_fused_pass_matches_unfused(tmp_path):
    """PH 2 of level j and PH 0 of level j + 1 share one launch in the N-D passes too;
    PCFM_EMD_FORM=unfused runs them apart.  One fresh child process per form
    (tests/helpers/emd_nd_forms.py); match and cost equal bit for bit."""
    for form in ("rowpass", "unfused"):
        env = dict(os.environ, PCFM_EMD_FORM=form)
        subprocess.run([sys.executable, os.path.join(HERE, "helpers", "emd_nd_forms.py"),
                        str(tmp_path / f"{form}.npz")], check=True, timeout=120, env=env, cwd=REPO)
    f, u = np.load(tmp_path / "rowpass.npz"), np.load(tmp_path / "unfused.npz")
    assert len(f.files) == 14 and sorted(f.files) == sorted(u.files)
    for k in f.files:
        assert np.isfinite(f[k]).all(), k
        np.testing.assert_array_equal(f[k], u[k], err_msg=k)


# ---- 6. the metrics ---------------------------------------------------------------------------------------
def test_pairwise_emd_nd_and_generation_metrics(ops):
    from pcfm import metrics
    for d in (2, 6):
        x, y = urand(20 + d, 6, 256, d) - 0.5, urand(30 + d, 5, 256, d) - 0.5
        got = metrics.pairwise_emd_nd(x, y)
        assert got.shape == (6, 5) and got.is_cuda
        want = metrics.pairwise_emd_nd(x.cpu(), y.cpu())
        np.testing.assert_allclose(np_(got), want.numpy(), rtol=1e-4)
        # the chunking does not show, down to one pair per call
        one = metrics._emd_nd_chunk_bytes(1, 256, 256, d, x)
        seven = metrics._emd_nd_chunk_bytes(7, 256, 256, d, x)
        assert metrics._emd_pairs_per_chunk(30, 256, 256, seven, x, d) == 7
        assert same(metrics.pairwise_emd_nd(x, y, max_bytes=seven), got)
        assert same(metrics.pairwise_emd_nd(x, y, max_bytes=one), got)
    s, r = urand(41, 6, 256, 6) - 0.5, urand(42, 5, 256, 6) - 0.5
    res = metrics.generation_metrics(s, r, emd_components="all")
    base = metrics.generation_metrics(s, r)
    assert sorted(res) == sorted(base)
    assert all(v.is_cuda and bool(torch.isfinite(v)) for v in res.values())
    mxy = metrics.pairwise_emd_nd(s, r)
    for k, v in metrics.mmd_cov(mxy).items():
        assert same(res[f"{k}_emd"], v), k
    for k in base:
        if k.endswith("_cd"):
            assert same(res[k], base[k]), k
    assert same(metrics.pairwise_emd_nd(s[..., :3].contiguous(), r[..., :3].contiguous()),
                metrics.pairwise_emd(s[..., :3].contiguous(), r[..., :3].contiguous()))
    on_cpu = metrics.generation_metrics(s.cpu(), r.cpu(), emd_components="all")
    np.testing.assert_allclose(float(res["mmd_emd"]), float(on_cpu["mmd_emd"]), rtol=1e-4)


# ---- 7. timings -----------------------------------------------------------------------------------------------
def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median_ms(fn, warm=3, reps=7):
    for _ in range(warm):
        fn()
    ts = [_ms(fn) for _ in range(reps)]
    return float(np.median(ts)), (max(ts) - min(ts)) / float(np.median(ts))


def test_timings(ops, report):
    """B = 8, N = M = 2048, one process, HIP events, 3 warm-up calls, median of 7 and
    the spread (max - min over the median): the 3-D f32 entry and the N-D entry at
    D = 3, 2, 5, 6, each for the cost-only forward, forward + match and forward +
    backward; every N-D figure also as a ratio to the 3-D entry's.  No ratio is
    asserted: only that every time is finite and positive."""
    b, n = 8, 2048
    gc = urand(50, b)

    def routes(fwd, bwd, a, c):
        def both():
            match, _ = fwd(a, c, True)
            bwd(gc, a, c, match)
        return {"cost_only": lambda: fwd(a, c, False), "fwd_match": lambda: fwd(a, c, True),
                "fwd_bwd": both}

    rec = {"shape": {"b": b, "n": n, "m": n}, "warmup": 3, "reps": 7}
    a3, c3 = urand(51, b, n, 3), urand(52, b, n, 3)
    base = {}
    for name, fn in routes(ops.approxmatch_cost_forward, ops.matchcost_backward, a3, c3).items():
        ms, spread = _median_ms(fn)
        base[name] = ms
        rec[f"3d_{name}"] = {"ms": ms, "spread": spread}
    for d in (3, 2, 5, 6):
        a, c = urand(53 + d, b, n, d), urand(63 + d, b, n, d)
        for name, fn in routes(ops.approxmatch_cost_forward_nd, ops.matchcost_backward_nd,
                               a, c).items():
            ms, spread = _median_ms(fn)
            rec[f"nd{d}_{name}"] = {"ms": ms, "spread": spread, "ratio_to_3d": ms / base[name]}
    print(rec)
    report("emd_nd/timing", rec)
    times = [v["ms"] for k, v in rec.items() if k[0] in "3n" and isinstance(v, dict)]
    assert len(times) == 15 and all(np.isfinite(t) and t > 0 for t in times), rec
