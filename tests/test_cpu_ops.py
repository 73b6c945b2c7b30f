"""The product's pure-PyTorch CPU backend (pcfm.cpu_ops, BASELINE configs[0])
against the C oracle (oracle/pcfm_oracle.c) and the reference's fixtures.

Two independent restatements of the reference kernels -- sequential C with
explicit fmaf, and vectorised torch (scatter_add_ / gather / blocked argmin) --
are held to each other: integer outputs bit-exact, gathers bit-exact (same
per-element expression), scatter sums to 1e-6 relative (summation order only,
as the reference's own float atomics).  Everything goes through the reference
entry-point names on pcfm.ops with CPU tensors.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import oracle as O
from pcfm import ops

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import emd_ref  # noqa: E402

RNG = np.random.default_rng(20261016)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _close(got, exp, rtol=1e-6, atol=1e-6):
    np.testing.assert_allclose(got.numpy() if isinstance(got, torch.Tensor) else got, exp,
                               rtol=rtol, atol=atol)


VOX_CASES = [(2, 5, 300, 8), (1, 3, 1, 4), (3, 16, 1000, 1), (2, 4, 2000, 32), (1, 2, 0, 4),
             (2, 7, 513, 100)]


@pytest.mark.parametrize("b,c,n,r", VOX_CASES)
def test_avg_voxelize_fwd_bwd(b, c, n, r):
    feat = RNG.standard_normal((b, c, n)).astype(np.float32)
    vc = RNG.integers(0, r, (b, 3, n)).astype(np.int32)
    out, ind, cnt = ops.avg_voxelize_forward(_t(feat), _t(vc), r)
    e_out, e_ind, e_cnt = O.avg_voxelize_fwd(feat, vc, r)
    assert np.array_equal(ind.numpy(), e_ind) and np.array_equal(cnt.numpy(), e_cnt)
    _close(out, e_out)
    gy = RNG.standard_normal((b, c, r ** 3)).astype(np.float32)
    gx = ops.avg_voxelize_backward(_t(gy), ind, cnt)
    assert np.array_equal(gx.numpy(), O.avg_voxelize_bwd(gy, e_ind, e_cnt))  # pure gather


@pytest.mark.parametrize("b,c,n,r", VOX_CASES)
@pytest.mark.parametrize("training", [True, False])
def test_trilinear_devoxelize_fwd_bwd(b, c, n, r, training):
    pts = (RNG.random((b, 3, n)) * (r - 1)).astype(np.float32)
    if n > 4:  # integer coordinates hit the x_hi = x_lo sentinel (trilinear_devox.cu:64-75)
        pts[:, :, :4] = np.round(pts[:, :, :4])
    grid = RNG.standard_normal((b, c, r ** 3)).astype(np.float32)
    o, i, w = ops.trilinear_devoxelize_forward(r, training, _t(pts), _t(grid))
    e_o, e_i, e_w = O.trilinear_devoxelize_fwd(pts, grid, r, training)
    _close(o, e_o, rtol=2e-7, atol=1e-7)
    if not training:
        assert i.shape == (1,) and w.shape == (1,)
        return
    assert np.array_equal(i.numpy(), e_i) and np.array_equal(w.numpy(), e_w)
    gy = RNG.standard_normal((b, c, n)).astype(np.float32)
    gx = ops.trilinear_devoxelize_backward(_t(gy), i, w, r)
    _close(gx, O.trilinear_devoxelize_bwd(gy, e_i, e_w, r), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("b,m,n,radius,u", [(2, 64, 500, 0.3, 16), (1, 5, 40, 10.0, 8),
                                             (2, 33, 100, 1e-3, 4), (1, 7, 0, 0.5, 3),
                                             (3, 100, 257, 0.5, 64), (1, 10, 20, 0.8, 32)])
def test_ball_query_bit_exact(b, m, n, radius, u):
    pts = RNG.random((b, 3, n)).astype(np.float32)
    centers = RNG.random((b, 3, m)).astype(np.float32)
    if n >= m:  # centers on points: d^2 = 0 is a hit
        centers[:, :, : m // 2] = pts[:, :, : m // 2]
    idx = ops.ball_query(_t(centers), _t(pts), radius, u)
    assert np.array_equal(idx.numpy(), O.ball_query(centers, pts, radius, u))


@pytest.mark.parametrize("b,c,n,m,u", [(2, 5, 100, 30, 8), (1, 1, 7, 3, 2), (2, 3, 50, 0, 4)])
def test_grouping_fwd_bwd(b, c, n, m, u):
    feat = RNG.standard_normal((b, c, n)).astype(np.float32)
    idx = RNG.integers(0, n, (b, m, u)).astype(np.int32)
    out = ops.grouping_forward(_t(feat), _t(idx))
    assert np.array_equal(out.numpy(), O.grouping_fwd(feat, idx))
    gy = RNG.standard_normal((b, c, m, u)).astype(np.float32)
    gx = ops.grouping_backward(_t(gy), _t(idx), n)
    _close(gx, O.grouping_bwd(gy, idx, n), rtol=1e-5, atol=1e-6)


def _chamfer_cpu(a, c):
    from chamfer3D.dist_chamfer_3D import chamfer_3DDist
    x1 = _t(a).requires_grad_(True)
    x2 = _t(c).requires_grad_(True)
    d1, d2, i1, i2 = chamfer_3DDist()(x1, x2)
    return x1, x2, d1, d2, i1, i2


@pytest.mark.parametrize("case", ["unit", "wide", "small", "ties", "timing_shape"])
def test_chamfer_against_reference_fixture(golden, case):
    """chamfer_python.distChamfer outputs (the reference's own CUDA-test oracle)."""
    g = golden("chamfer_python.npz")
    a, c = g[f"{case}_xyz1"], g[f"{case}_xyz2"]
    _, _, d1, d2, i1, i2 = _chamfer_cpu(a, c)
    assert np.array_equal(i1.numpy(), g[f"{case}_idx1"])
    assert np.array_equal(i2.numpy(), g[f"{case}_idx2"])
    # unit_test.py:23-34 asserts mean squared difference < 1e-8
    assert np.mean((d1.detach().numpy() - g[f"{case}_dist1"]) ** 2) < 1e-8
    assert np.mean((d2.detach().numpy() - g[f"{case}_dist2"]) ** 2) < 1e-8


@pytest.mark.parametrize("b,n,m", [(2, 300, 200), (1, 1, 5), (3, 64, 64)])
def test_chamfer_fwd_bwd_against_oracle(b, n, m):
    a = RNG.standard_normal((b, n, 3)).astype(np.float32)
    c = RNG.standard_normal((b, m, 3)).astype(np.float32)
    c[:, :2] = a[:, :2]  # exact hits: distance 0
    x1, x2, d1, d2, i1, i2 = _chamfer_cpu(a, c)
    e = O.chamfer_fwd(a, c)
    for got, exp in zip((d1, d2, i1, i2), e):
        assert np.array_equal(got.detach().numpy(), exp)  # same fma contract: bit-exact
    gd1 = RNG.standard_normal((b, n)).astype(np.float32)
    gd2 = RNG.standard_normal((b, m)).astype(np.float32)
    torch.autograd.backward([d1, d2], [_t(gd1), _t(gd2)])
    e1, e2 = O.chamfer_bwd(a, c, gd1, gd2, e[2], e[3])
    _close(x1.grad, e1, rtol=1e-5, atol=1e-6)
    _close(x2.grad, e2, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("bad", ["dist1 (b, n + 1)", "idx2 (b, m, 1)", "gradxyz1 (b, n, 2)",
                                 "xyz2 another batch size"])
def test_chamfer_3d_refuses_mis_shaped_tensors(bad, capfd):
    """chamfer_3D checks every extent the kernels index with, as chamfer_{2,5,6}D and the
    C++ extension do: a mis-shaped tensor prints the reference's line, returns 0 and
    leaves every output as it was.  (The backward's graddist1 has dist1's shape; the
    forward takes no gradxyz1.)"""
    b, n, m = 2, 7, 5
    xyz1 = torch.rand(b, n, 3)
    xyz2 = torch.rand(b + (bad == "xyz2 another batch size"), m, 3)
    f = {"dist1": (b, n + (bad == "dist1 (b, n + 1)")), "dist2": (b, m),
         "gradxyz1": (b, n, 3 - (bad == "gradxyz1 (b, n, 2)")), "gradxyz2": (b, m, 3)}
    i = {"idx1": (b, n), "idx2": (b, m) + ((1,) if bad == "idx2 (b, m, 1)" else ())}
    t = {k: torch.full(s, 7.0) for k, s in f.items()}
    t.update({k: torch.zeros(s, dtype=torch.int32) for k, s in i.items()})
    before = {k: v.clone() for k, v in t.items()}
    if bad != "gradxyz1 (b, n, 2)":
        assert ops.chamfer_3D.forward(xyz1, xyz2, t["dist1"], t["dist2"], t["idx1"],
                                      t["idx2"]) == 0
        assert "error in nnd updateOutput: " in capfd.readouterr().out
    assert ops.chamfer_3D.backward(xyz1, xyz2, t["gradxyz1"], t["gradxyz2"], t["dist1"],
                                   t["dist2"], t["idx1"], t["idx2"]) == 0
    assert "error in nnd get grad: " in capfd.readouterr().out
    assert all(torch.equal(t[k], before[k]) for k in t)


def test_chamfer_self_distance_is_zero():
    """README.md:116-133: CD(x, x) = 0 with idx = identity for distinct points."""
    a = RNG.standard_normal((2, 2048, 3)).astype(np.float32)
    _, _, d1, d2, i1, i2 = _chamfer_cpu(a, a)
    assert float(d1.detach().abs().max()) == 0.0 and float(d2.detach().abs().max()) == 0.0
    ar = np.arange(2048)
    assert np.array_equal(i1.numpy()[0], ar) and np.array_equal(i2.numpy()[1], ar)


def test_emd_known_answer(golden):
    """PyTorchEMD/test_emd_loss.py: EMD = exact assignment (0.355 per element)."""
    from PyTorchEMD.emd import earth_mover_distance
    g = golden("emd_known.npz")
    p1 = _t(g["p1"]).requires_grad_(True)
    p2 = _t(g["p2"]).requires_grad_(True)
    d = earth_mover_distance(p1, p2, transpose=False)
    _close(d.detach(), g["gt_per_element"], rtol=1e-4, atol=1e-6)
    (d * _t(g["weights"])).sum().backward()
    # the script's ground truth weights the unnormalised pair cost: d(loss) = gt / N
    _close(p1.grad, g["gt_grad1"] / 2, rtol=1e-3, atol=1e-5)
    _close(p2.grad, g["gt_grad2"] / 2, rtol=1e-3, atol=1e-5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("b,n,m", [(2, 40, 40), (1, 30, 70), (2, 64, 16)])
def test_emd_against_oracle(dtype, b, n, m):
    a = RNG.random((b, n, 3)).astype(dtype)
    c = RNG.random((b, m, 3)).astype(dtype)
    match = ops.approxmatch_forward(_t(a), _t(c))
    e_match = O.emd_approxmatch(a, c)
    # the oracle evaluates exp in float (the reference's __expf); relative 1e-4
    _close(match, e_match, rtol=1e-3, atol=5e-5)
    cost = ops.matchcost_forward(_t(a), _t(c), match)
    _close(cost, O.emd_matchcost(a, c, e_match), rtol=1e-4, atol=1e-6)
    gc = RNG.random((b,)).astype(dtype)
    g1, g2 = ops.matchcost_backward(_t(gc), _t(a), _t(c), match)
    e1, e2 = O.emd_matchcost_bwd(gc, a, c, e_match)
    _close(g1, e1, rtol=1e-3, atol=1e-4)
    _close(g2, e2, rtol=1e-3, atol=1e-4)


# The fp64 reference of approxmatch (tests/helpers/emd_ref.py) against the two CPU
# implementations.  Each bound is four times the largest deviation measured over
# emd_ref.CPU_CASES (max |x - ref| / max ref; the deviation is a round-off walk that
# moves with seed and shape):
#   cpu_ops f32 4.212e-06, cpu_ops f64 1.708e-06 (its exp is exact, the reference's
#   is the kernels' float32 exp2), oracle f32 6.973e-06, oracle f64 4.602e-06.
EMD_REF_BOUND = {("cpu", np.float32): 4 * 4.212e-06, ("cpu", np.float64): 4 * 1.708e-06,
                 ("oracle", np.float32): 4 * 6.973e-06, ("oracle", np.float64): 4 * 4.602e-06}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("b,n,m", emd_ref.CPU_CASES)
def test_emd_fp64_reference_against_cpu_and_oracle(dtype, b, n, m):
    a, c = emd_ref.clouds(b, n, m, dtype, 1000 * n + m)
    ref = emd_ref.approxmatch(a, c)
    assert ref.shape == (b, m, n) and ref.dtype == np.float64 and (ref >= 0).all()
    # no point gives or takes more than its capacity (emd_kernel.cu:27-33)
    multi_l, multi_r = (1.0, float(n // m)) if n >= m else (float(m // n), 1.0)
    assert ref.sum(axis=1).max() <= multi_l + 1e-9 and ref.sum(axis=2).max() <= multi_r + 1e-9
    got = {"cpu": ops.approxmatch_forward(_t(a), _t(c)).numpy(), "oracle": O.emd_approxmatch(a, c)}
    for who, x in got.items():
        err = emd_ref.rel_err(x, ref)
        print(f"emd_ref {who} {np.dtype(dtype).name} {(b, n, m)}: {err:.3e}")
        assert err <= EMD_REF_BOUND[who, dtype], (who, err)
