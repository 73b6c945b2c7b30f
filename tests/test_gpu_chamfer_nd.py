"""GPU: the D-component Chamfer distance (csrc/chamfer_nd.hip through
include/pcfm_chamfer_nd.h, pcfm.ops.chamfer_{2,5,6}D, chamfer{2,5,6}D/) against

  * the reference's chamfer_python.distChamfer fixtures (float64; indices
    exact -- tests/golden/make_chamfer_nd_golden.py asserts the gaps that make
    that safe);
  * the oracle-checked 3-D entry (pcfm_chamfer_fwd), bit for bit, at D = 3: both
    entries launch the one D = 3 brute-force kernel;
  * the CPU backend (pcfm.cpu_ops) and the float64 gradient formula;
  * the C ABI's memory contract (the row runner of tests/test_gpu_abi_contract.py).

Every shape is a brute-force shape for the 3-D kernel too (below the session's
culling threshold of 16M pairs, tests/conftest.py), except the timing shapes."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import chamfer_nd_cases as cases  # noqa: E402

import guard_alloc  # noqa: E402,F401  (the allocator run_row places the arenas with)
from test_gpu_abi_contract import Row, run_row  # noqa: E402

from chamfer2D.dist_chamfer_2D import chamfer_2DDist  # noqa: E402
from chamfer5D.dist_chamfer_5D import chamfer_5DDist  # noqa: E402
from chamfer6D.dist_chamfer_6D import chamfer_6DDist  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
DIST = {2: chamfer_2DDist, 5: chamfer_5DDist, 6: chamfer_6DDist}
# atomics-ordered sums: the project's bar (tests/test_gpu_ops.py test_chamfer_vs_oracle)
BWD_TOL = dict(rtol=1e-5, atol=1e-5)


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


def outs(b, n, m):
    return (torch.empty(b, n, device=DEV), torch.empty(b, m, device=DEV),
            torch.empty(b, n, dtype=torch.int32, device=DEV),
            torch.empty(b, m, dtype=torch.int32, device=DEV))


def forward(ops, a, c, d=None):
    """(dist1, dist2, idx1, idx2) of the ctypes binding on HIP tensors a, c."""
    o = outs(a.shape[0], a.shape[1], c.shape[1])
    assert ops._chamfer_nd_forward(a, c, *o, d) == 1
    return o


# ---- 1. the reference's fixtures ----------------------------------------------------
@pytest.mark.parametrize("d", cases.DIMS)
def test_vs_reference_fixtures(ops, golden, report, d):
    g = golden(f"chamfer_nd_python_d{d}.npz")
    worst = 0.0
    for case in cases.CASES:
        a, c = g[f"{case}_xyz1"], g[f"{case}_xyz2"]
        d1, d2, i1, i2 = (np_(t) for t in DIST[d]()(cu(a), cu(c)))
        for got, key in ((d1, "dist1"), (d2, "dist2")):
            ref = g[f"{case}_{key}"].astype(np.float64)
            ok = ref > 1e-12                                   # exact hits have no relative error
            worst = max(worst, float(np.max(np.abs(got[ok] - ref[ok]) / ref[ok])))
        print(f"d={d} {case}: largest relative distance deviation so far {worst:.3g}")
        np.testing.assert_array_equal(i1, g[f"{case}_idx1"])
        np.testing.assert_array_equal(i2, g[f"{case}_idx2"])
        # (D + 3) * 2^-24 <= 5.4e-7 of the fp32 chain plus the golden's float cast,
        # rounded up; atol: float64 cancellation of the expanded form at exact hits
        np.testing.assert_allclose(d1, g[f"{case}_dist1"], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(d2, g[f"{case}_dist2"], rtol=1e-6, atol=1e-9)
        # the reference's own bar (unit_test.py)
        assert (np.mean((d1 - g[f"{case}_dist1"]) ** 2)
                + np.mean((d2 - g[f"{case}_dist2"]) ** 2)) < 1e-8
    report(f"chamfer_nd/d{d}_max_rel_dist_dev_vs_distChamfer", worst)


# ---- 2. D = 3: the bits of the oracle-checked 3-D entry (the same kernel) --------------
@pytest.mark.parametrize("case", list(cases.CASES))
def test_d3_is_bit_equal_to_the_3d_kernel(ops, case):
    a, c = (cu(t) for t in cases.inputs(case, 3))
    assert a.shape[1] * c.shape[1] < int(os.environ["PCFM_CHAMFER_CULL_PAIRS"])  # brute force
    got = forward(ops, a, c)
    exp = outs(a.shape[0], a.shape[1], c.shape[1])
    assert ops.chamfer_3D.forward(a, c, *exp) == 1
    for p, q in zip(got, exp):
        assert torch.equal(p, q)


# ---- 3. HIP against the CPU backend ---------------------------------------------------
@pytest.mark.parametrize("d", cases.DIMS)
@pytest.mark.parametrize("b,n,m", [(1, 1, 1), (2, 257, 129), (1, 100, 0)])
def test_vs_cpu_backend(ops, d, b, n, m):
    g = np.random.default_rng(b + n + m + d)
    a = g.standard_normal((b, n, d)).astype(np.float32)
    c = g.standard_normal((b, m, d)).astype(np.float32)
    if n and m:
        c[:, : min(n, m) // 3] = a[:, : min(n, m) // 3]  # exact hits
    got = forward(ops, cu(a), cu(c), d)
    exp = (torch.empty(b, n), torch.empty(b, m), torch.empty(b, n, dtype=torch.int32),
           torch.empty(b, m, dtype=torch.int32))
    assert getattr(ops, f"chamfer_{d}D").forward(torch.from_numpy(a), torch.from_numpy(c),
                                                 *exp) == 1
    np.testing.assert_array_equal(np_(got[2]), exp[2].numpy())
    np.testing.assert_array_equal(np_(got[3]), exp[3].numpy())
    np.testing.assert_allclose(np_(got[0]), exp[0].numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(np_(got[1]), exp[1].numpy(), rtol=1e-6, atol=0)
    if n and m:
        k = min(n, m) // 3
        assert (np_(got[0])[:, :k] == 0).all()
    else:
        assert (np_(got[0]) == 0).all() and (np_(got[2]) == 0).all()


@pytest.mark.parametrize("d", (2, 3, 5, 6))
@pytest.mark.parametrize("b,n,m", [(2, 70, 3), (1, 5, 1)])
def test_fewer_candidates_than_one_group(ops, d, b, n, m):
    """m below the candidate group (8 for D <= 3, 4 for D = 5, 6): the walk is its ragged
    tail group alone, every load clamped to the last candidate.  Exact against the CPU
    backend, which rounds the same chain the same way (pcfm.cpu_ops._sqdist_nd)."""
    g = np.random.default_rng(1000 + 10 * d + m)
    a = g.standard_normal((b, n, d)).astype(np.float32)
    c = g.standard_normal((b, m, d)).astype(np.float32)
    c[:, 0] = a[:, 1]                                     # an exact hit
    exp = (torch.empty(b, n), torch.empty(b, m), torch.empty(b, n, dtype=torch.int32),
           torch.empty(b, m, dtype=torch.int32))
    assert ops._chamfer_nd_forward(torch.from_numpy(a), torch.from_numpy(c), *exp, d) == 1
    entries = [lambda x, y, *o: ops._chamfer_nd_forward(x, y, *o, d)]
    if d == 3:
        entries.append(ops.chamfer_3D.forward)
    for entry in entries:
        got = outs(b, n, m)
        assert entry(cu(a), cu(c), *got) == 1
        for p, q in zip(got, exp):
            np.testing.assert_array_equal(np_(p), q.numpy())


# ---- 4. backward ----------------------------------------------------------------------
def grad_f64(a, c, gd1, gd2, i1, i2):
    """The float64 formula with the forward's indices (numpy in, numpy out)."""
    a, c = a.astype(np.float64), c.astype(np.float64)
    g1, g2 = np.zeros_like(a), np.zeros_like(c)
    for bb in range(a.shape[0]):
        t = 2.0 * gd1[bb].astype(np.float64)[:, None] * (a[bb] - c[bb][i1[bb]])
        g1[bb] += t
        np.add.at(g2[bb], i1[bb], -t)
        t = 2.0 * gd2[bb].astype(np.float64)[:, None] * (c[bb] - a[bb][i2[bb]])
        g2[bb] += t
        np.add.at(g1[bb], i2[bb], -t)
    return g1, g2


# d = 3 runs through both C entries: "3d" pcfm_chamfer_bwd, "3nd" pcfm_chamfer_nd_bwd
@pytest.mark.parametrize("d", cases.DIMS + ("3d", "3nd"))
@pytest.mark.parametrize("case", ["split", "ties"])
def test_backward_vs_float64(ops, d, case):
    if d == "3d":
        d, backward = 3, ops.chamfer_3D.backward
    elif d == "3nd":
        d, backward = 3, lambda *t: ops._chamfer_nd_backward(*t, d=3)
    else:
        backward = getattr(ops, f"chamfer_{d}D").backward
    a, c = cases.inputs(case, d)
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    g = np.random.default_rng(d)
    gd1, gd2 = g.random((b, n)).astype(np.float32), g.random((b, m)).astype(np.float32)
    s1 = g.standard_normal((b, n, d)).astype(np.float32)   # a non-zero start: it ACCUMULATES
    s2 = g.standard_normal((b, m, d)).astype(np.float32)
    _, _, i1, i2 = forward(ops, cu(a), cu(c), d)
    g1, g2 = cu(s1), cu(s2)
    assert backward(cu(a), cu(c), g1, g2, cu(gd1), cu(gd2), i1, i2) == 1
    e1, e2 = grad_f64(a, c, gd1, gd2, np_(i1), np_(i2))
    np.testing.assert_allclose(np_(g1), s1 + e1, **BWD_TOL)
    np.testing.assert_allclose(np_(g2), s2 + e2, **BWD_TOL)
    # an index outside the other cloud is skipped: nothing is added for it
    bad1 = i1.clone()
    bad1[:, ::2] = m
    bad2 = torch.full_like(i2, -1)
    z1, z2 = torch.zeros_like(g1), torch.zeros_like(g2)
    assert ops._chamfer_nd_backward(cu(a), cu(c), z1, z2, cu(gd1), cu(gd2), bad1, bad2) == 1
    gd1_odd = gd1.copy()
    gd1_odd[:, ::2] = 0
    e1, e2 = grad_f64(a, c, gd1_odd, np.zeros_like(gd2), np_(i1), np_(i2))
    np.testing.assert_allclose(np_(z1), e1, **BWD_TOL)
    np.testing.assert_allclose(np_(z2), e2, **BWD_TOL)


def test_autograd_6d():
    a, c = (cu(t).requires_grad_(True) for t in cases.inputs("split", 6))
    d1, d2, i1, i2 = chamfer_6DDist()(a, c)
    assert not i1.requires_grad and not i2.requires_grad
    (d1.mean() + d2.mean()).backward()
    assert a.grad.shape == a.shape and c.grad.shape == c.shape
    assert torch.isfinite(a.grad).all() and torch.isfinite(c.grad).all()
    assert a.grad.abs().sum() > 0 and c.grad.abs().sum() > 0
    # under autocast the inputs are cast to float32 (custom_fwd), as chamfer_3DFunction
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h1, _, j1, _ = chamfer_6DDist()(a.detach().bfloat16(), c.detach().bfloat16())
    assert h1.dtype == torch.float32 and j1.dtype == torch.int32


# ---- 5. behaviour -----------------------------------------------------------------------
@pytest.mark.parametrize("d", cases.DIMS)
def test_deterministic_streams_and_extension(ops, d):
    a, c = (cu(t) for t in cases.inputs("split", d))
    first, again = forward(ops, a, c, d), forward(ops, a, c, d)
    for p, q in zip(first, again):
        assert torch.equal(p, q)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = forward(ops, a, c, d)
    s.synchronize()
    for p, q in zip(first, side):
        assert torch.equal(p, q)
    # the torch extension over the same C ABI
    ext = importlib.import_module(f"chamfer{d}D.chamfer_{d}D")
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    e = outs(b, n, m)
    assert ext.forward(a, c, *e) == 1
    for p, q in zip(first, e):
        assert torch.equal(p, q)
    with torch.cuda.stream(s):
        e2 = outs(b, n, m)
        assert ext.forward(a, c, *e2) == 1
    s.synchronize()
    for p, q in zip(first, e2):
        assert torch.equal(p, q)
    g = torch.Generator(device=DEV).manual_seed(d)
    gd1, gd2 = torch.rand(b, n, device=DEV, generator=g), torch.rand(b, m, device=DEV, generator=g)
    ga, gc = (torch.zeros_like(a), torch.zeros_like(c)), (torch.zeros_like(a), torch.zeros_like(c))
    assert ext.backward(a, c, *ga, gd1, gd2, e[2], e[3]) == 1
    assert getattr(ops, f"chamfer_{d}D").backward(a, c, *gc, gd1, gd2, first[2], first[3]) == 1
    for p, q in zip(ga, gc):
        torch.testing.assert_close(p, q, **BWD_TOL)
    # HIP tensors of the wrong shape, dimension or device: 0, nothing launched
    assert ext.forward(a, c, e[0], e[1], e[2], e[3][:, :-1].contiguous()) == 0
    assert ext.forward(a, c, e[0], e[1].cpu(), e[2], e[3]) == 0
    x3 = torch.zeros(b, n, 3, device=DEV)
    assert ext.forward(x3, x3, e[0], e[0].clone(), e[2], e[2].clone()) == 0
    assert getattr(ops, f"chamfer_{d}D").forward(x3, x3, e[0], e[0].clone(), e[2],
                                                 e[2].clone()) == 0


# ---- 6. pcfm.sample.chamfer_l2 --------------------------------------------------------------
def test_chamfer_l2_6d_and_3d():
    from chamfer3D.dist_chamfer_3D import chamfer_3DDist
    from pcfm.sample import chamfer_l2
    g = torch.Generator(device=DEV).manual_seed(0)
    a = torch.randn(2, 500, 6, device=DEV, generator=g)
    c = torch.randn(2, 500, 6, device=DEV, generator=g)
    d2 = torch.cdist(a.double(), c.double()).pow(2)
    exp = d2.min(2).values.mean(1) + d2.min(1).values.mean(1)
    torch.testing.assert_close(chamfer_l2(a, c).double(), exp, rtol=1e-5, atol=1e-7)
    a3, c3 = a[:, :, :3].contiguous(), c[:, :, :3].contiguous()
    d1, d2, _, _ = chamfer_3DDist()(a3, c3)
    assert torch.equal(chamfer_l2(a3, c3), d1.mean(dim=1) + d2.mean(dim=1))


# ---- 7. the C ABI's memory contract ------------------------------------------------------------
def nd_row(d, b, n, m):
    """chamfer_row of tests/test_gpu_abi_contract.py over d components.

    run_row compares an output bit for bit unless its two plain runs differ, and
    the backward's float atomics arrive in no fixed order: an element of g1 is
    start + own term + neighbour terms.  With free float inputs the first run of
    this file's (1, 1, 1) row at d = 6 passed and the next failed at "guarded run,
    output 6 differs from the plain run (3 of 6 elements)" -- guards intact, no
    poison left, values equal to the printed digits: two plain runs had agreed
    and the third order rounded differently.  So every row draws its inputs on a
    dyadic grid (points and starts: multiples of 1/64 within +-4; grad_dist:
    multiples of 1/16 in [0, 1]): each term g * (q - p) is a multiple of 1/512
    below 16 and every partial sum of the at most 1026 addends of an element
    stays below 2^15, all exact in fp32, so the sums do not depend on the order
    and every backward output of every row is compared bit for bit as well (the
    declared tolerance is what the row may fall back to, never what it needs)."""
    def grid(t, step, lim):
        return (torch.round(t / step) * step).clamp_(-lim, lim)

    def build(seed):
        g = torch.Generator(device=DEV).manual_seed(900 + 10 * d + seed)
        a = grid(torch.randn(b, n, d, device=DEV, generator=g), 1 / 64, 4.0)
        c = grid(torch.randn(b, m, d, device=DEV, generator=g), 1 / 64, 4.0)
        if n and m:
            k = min(n, m) // 3
            c[:, :k] = a[:, :k]                              # exact hits
        return {"a": a, "c": c,
                "gd1": grid(torch.rand(b, n, device=DEV, generator=g), 1 / 16, 1.0),
                "gd2": grid(torch.rand(b, m, device=DEV, generator=g), 1 / 16, 1.0),
                # a non-zero start: the backward ACCUMULATES
                "g1": grid(torch.randn(b, n, d, device=DEV, generator=g), 1 / 64, 4.0),
                "g2": grid(torch.randn(b, m, d, device=DEV, generator=g), 1 / 64, 4.0)}

    def call(dd):
        from pcfm import ops
        t = ops.torch                 # the allocator the wrappers use (guarded when patched)
        ns = getattr(ops, f"chamfer_{d}D")
        a, c = dd["a"], dd["c"]
        d1 = t.empty((b, n), dtype=torch.float32, device=DEV)
        d2 = t.empty((b, m), dtype=torch.float32, device=DEV)
        i1 = t.empty((b, n), dtype=torch.int32, device=DEV)
        i2 = t.empty((b, m), dtype=torch.int32, device=DEV)
        assert ns.forward(a, c, d1, d2, i1, i2) == 1
        res = [d1, d2, i1, i2]
        if n and m:
            z1 = t.zeros((b, n, d), dtype=torch.float32, device=DEV)   # pre-zeroed, as the
            z2 = t.zeros((b, m, d), dtype=torch.float32, device=DEV)   # contract says
            assert ns.backward(a, c, z1, z2, dd["gd1"], dd["gd2"], i1, i2) == 1
            s1, s2 = dd["g1"].clone(), dd["g2"].clone()
            assert ns.backward(a, c, dd["g1"], dd["g2"], dd["gd1"], dd["gd2"], i1, i2) == 1
            torch.testing.assert_close(dd["g1"], s1 + z1, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(dd["g2"], s2 + z2, rtol=1e-5, atol=1e-5)
            res += [z1, z2, dd["g1"], dd["g2"]]
        return res
    return Row(f"chamfer-nd-d{d}-b{b}n{n}m{m}", build, call,
               ["pcfm_chamfer_nd_fwd"] + (["pcfm_chamfer_nd_bwd"] if n and m else []),
               tol=(1e-5, 1e-6) if n and m else None)


ND_ROWS = [nd_row(d, *s) for d in (2, 6)
           for s in ((1, 1, 1), (1, 100, 0), (2, 257, 129), (3, 777, 1025))]


@pytest.mark.parametrize("row", ND_ROWS, ids=[r.id for r in ND_ROWS])
def test_memory_contract(ops, row, report):
    run_row(row, report)


def test_every_launching_nd_entry_is_in_a_row():
    from pcfm import _lib
    launching = {n for n in _lib.ND_SIGNATURES if n.endswith(("_fwd", "_bwd"))}
    assert launching == {e for r in ND_ROWS for e in r.entries}


def test_einval_launches_and_writes_nothing(ops):
    a = torch.randn(2, 300, 6, device=DEV)
    o = outs(2, 300, 300)
    for t in o:
        t.fill_(7)
    from pcfm import _lib
    with pytest.raises(_lib.PcfmError, match="unsupported dimension"):
        _lib.call("pcfm_chamfer_nd_fwd", a.data_ptr(), a.data_ptr(), 2, 300, 300, 4,
                  *(t.data_ptr() for t in o), None, 0, None)
    torch.cuda.synchronize()
    for t in o:
        assert (t == 7).all()


# ---- timings (recorded, not asserted) ---------------------------------------------------------
def _median_ms(fn, warmup=3, reps=7):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


@pytest.mark.parametrize("b,n,m,name", [(32, 2000, 1000, "published_32x2000x1000"),
                                        (8, 20000, 20000, "c2_8x20000x20000")])
def test_timings_recorded(ops, report, b, n, m, name):
    """d = 6 forward / backward beside the 3-D entry points in the same process:
    warm-up, HIP events, median of 7.  In this session the 3-D forward takes its
    culled search from 16M pairs (tests/conftest.py), so the brute-force
    yardstick at the C2 shape is the N-D entry at D = 3 -- the kernel the 3-D
    entry launches below its culling threshold (test 2); both are recorded."""
    g = torch.Generator(device=DEV).manual_seed(1)
    rec = {}
    for d in (3, 6):
        a = torch.randn(b, n, d, device=DEV, generator=g)
        c = torch.randn(b, m, d, device=DEV, generator=g)
        o = outs(b, n, m)
        gd1, gd2 = torch.rand(b, n, device=DEV, generator=g), torch.rand(b, m, device=DEV,
                                                                         generator=g)
        g1, g2 = torch.zeros_like(a), torch.zeros_like(c)
        rec[f"nd_d{d}_fwd_ms"] = _median_ms(lambda: ops._chamfer_nd_forward(a, c, *o, d))
        rec[f"nd_d{d}_bwd_ms"] = _median_ms(
            lambda: ops._chamfer_nd_backward(a, c, g1, g2, gd1, gd2, o[2], o[3], d))
        if d == 3:
            culled = n * m >= int(os.environ["PCFM_CHAMFER_CULL_PAIRS"])
            rec["chamfer3d_fwd_path"] = "culled" if culled else "brute force"
            rec["chamfer3d_fwd_ms"] = _median_ms(lambda: ops.chamfer_3D.forward(a, c, *o))
            rec["chamfer3d_bwd_ms"] = _median_ms(
                lambda: ops.chamfer_3D.backward(a, c, g1, g2, gd1, gd2, o[2], o[3]))
    rec["d6_over_d3_fwd"] = rec["nd_d6_fwd_ms"] / rec["nd_d3_fwd_ms"]
    print(name, rec)
    report(f"chamfer_nd/timing_{name}", rec)
