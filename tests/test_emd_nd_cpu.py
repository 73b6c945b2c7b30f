"""CPU: the approximate EMD over D-component points (include/pcfm_emd_nd.h,
csrc/emd.hip) without a GPU -- the CPU backend against the float64 reference of
tests/helpers/emd_nd_ref.py and, at D = 3, against the existing functions bit for
bit; the autograd wrapper; pairwise_emd_nd and the emd_components keyword of
generation_metrics; the sixth ABI table, the host plan and the host-side
refusals; the resources of the shipped kernels."""
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
import emd_nd_ref as ndref  # noqa: E402
import emd_ref  # noqa: E402

from pcfm import _lib, cpu_ops, metrics, ops  # noqa: E402
from PyTorchEMD.emd import earth_mover_distance  # noqa: E402
from PyTorchEMD.emd_nd import EarthMoverDistanceNDFunction, earth_mover_distance_nd  # noqa: E402

HEADER = os.path.join(REPO, "include", "pcfm_emd_nd.h")
EMD_ND = sorted(_lib.EMD_ND_SIGNATURES)
BOUND = 1e-4        # the project's EMD bar (EMD_REF_BOUND["f32"] in tests/test_gpu_ops.py)


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# ---- 1. the CPU backend ------------------------------------------------------------------
@pytest.mark.parametrize("b,n,m,d", ndref.CASES)
def test_cpu_ops_vs_fp64_reference(b, n, m, d):
    a, c = ndref.clouds(b, n, m, d)
    ref = ndref.approxmatch(a, c)
    ta, tc = torch.from_numpy(a), torch.from_numpy(c)
    match = cpu_ops.approxmatch_forward_nd(ta, tc)
    assert match.shape == (b, m, n) and match.dtype == torch.float32
    err = ndref.rel_err(match.numpy(), ref)
    print(f"emd_nd cpu_ops D={d} {(b, n, m)}: {err:.3e}")
    assert err <= BOUND, err
    np.testing.assert_allclose(match.numpy().sum(axis=(1, 2), dtype=np.float64),
                               ref.sum(axis=(1, 2)), rtol=10 * BOUND)
    # the cost and the gradients of that match against the float64 closed forms
    cost = cpu_ops.matchcost_forward_nd(ta, tc, match)
    np.testing.assert_allclose(cost.numpy(), ndref.matchcost(a, c, match.numpy()), rtol=BOUND)
    gc = _rand(5, b)
    g1, g2 = cpu_ops.matchcost_backward_nd(gc, ta, tc, match)
    r1, r2 = ndref.matchcost_grads(gc.numpy(), a, c, match.numpy())
    np.testing.assert_allclose(g1.numpy(), r1, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(r1).max()))
    np.testing.assert_allclose(g2.numpy(), r2, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(r2).max()))


def test_reference_at_d3_is_emd_ref():
    a, c = emd_ref.clouds(3, 100, 37, np.float32, 7)
    assert np.array_equal(ndref.pair_d2(a[0], c[0]), emd_ref.pair_d2(a[0], c[0]))
    assert np.array_equal(ndref.approxmatch(a, c), emd_ref.approxmatch(a, c))
    assert emd_ref.pair_d2.__module__ == "emd_ref"      # the helper put it back


@pytest.mark.parametrize("b,n,m", [(3, 100, 37), (2, 37, 700), (4, 1, 64), (2, 5, 0), (0, 4, 4)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_d3_equals_existing_cpu_ops_in_bits(b, n, m, dtype):
    a, c, gc = (_rand(1, b, n, 3).to(dtype), _rand(2, b, m, 3).to(dtype), _rand(3, b).to(dtype))
    match = cpu_ops.approxmatch_forward(a, c)
    assert torch.equal(cpu_ops.approxmatch_forward_nd(a, c), match)
    assert torch.equal(cpu_ops.matchcost_forward_nd(a, c, match),
                       cpu_ops.matchcost_forward(a, c, match))
    for x, y in zip(cpu_ops.matchcost_backward_nd(gc, a, c, match),
                    cpu_ops.matchcost_backward(gc, a, c, match)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("d", [2, 5, 6])
def test_backward_vs_float64_autograd(d):
    b, n, m = 2, 37, 50
    a = _rand(11, b, n, d).double().requires_grad_(True)
    c = _rand(12, b, m, d).double().requires_grad_(True)
    match = cpu_ops.approxmatch_forward_nd(a.detach(), c.detach())
    gc = _rand(13, b).double()
    (cpu_ops.matchcost_forward_nd(a, c, match) * gc).sum().backward()
    g1, g2 = cpu_ops.matchcost_backward_nd(gc, a.detach(), c.detach(), match)
    torch.testing.assert_close(g1, a.grad, rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(g2, c.grad, rtol=1e-10, atol=1e-12)


# ---- 2. the ops wrappers and the autograd function on CPU tensors ------------------------------
def test_ops_wrappers_on_cpu_tensors():
    a, c = _rand(1, 2, 30, 6), _rand(2, 2, 40, 6)
    match, cost = ops.approxmatch_cost_forward_nd(a, c)
    assert torch.equal(match, cpu_ops.approxmatch_forward_nd(a, c))
    assert torch.equal(cost, cpu_ops.matchcost_forward_nd(a, c, match))
    none, cost2 = ops.approxmatch_cost_forward_nd(a, c, want_match=False)
    assert none is None and torch.equal(cost, cost2)
    assert torch.equal(ops.matchcost_forward_nd(a, c, match), cost)
    gc = _rand(3, 2)
    for x, y in zip(ops.matchcost_backward_nd(gc, a, c, match),
                    cpu_ops.matchcost_backward_nd(gc, a, c, match)):
        assert torch.equal(x, y)
    # D = 3: the 3-D wrapper's bits
    a3, c3 = a[..., :3].contiguous(), c[..., :3].contiguous()
    m3, c3cost = ops.approxmatch_cost_forward(a3, c3)
    m3n, c3ncost = ops.approxmatch_cost_forward_nd(a3, c3)
    assert torch.equal(m3, m3n) and torch.equal(c3cost, c3ncost)


def test_ops_wrapper_refusals():
    a, c = torch.zeros(2, 5, 6), torch.zeros(2, 7, 6)
    match, gc = torch.zeros(2, 7, 5), torch.zeros(2)
    bad_pairs = [(a.double(), c.double()), (a, c.double()), (a, torch.zeros(3, 7, 6)),
                 (a, torch.zeros(2, 7, 5)), (torch.zeros(2, 5, 4), torch.zeros(2, 7, 4)),
                 (torch.zeros(2, 5, 1), torch.zeros(2, 7, 1)),
                 (torch.zeros(2, 5, 7), torch.zeros(2, 7, 7)), (torch.zeros(5, 6), c),
                 (torch.zeros(5, 2, 6).transpose(0, 1), c)]
    for x, y in bad_pairs:
        with pytest.raises(RuntimeError):
            ops.approxmatch_cost_forward_nd(x, y)
    for bad in (torch.zeros(2, 5, 7), match.double(), torch.zeros(7, 2, 5).transpose(0, 1)):
        with pytest.raises(RuntimeError):
            ops.matchcost_forward_nd(a, c, bad)
        with pytest.raises(RuntimeError):
            ops.matchcost_backward_nd(gc, a, c, bad)
    with pytest.raises(RuntimeError):
        ops.matchcost_backward_nd(torch.zeros(3), a, c, match)
    for d in ops.EMD_ND_DIMS:        # empty problems: zeros of the stated shapes
        m0, c0 = ops.approxmatch_cost_forward_nd(torch.zeros(2, 0, d), torch.zeros(2, 4, d))
        assert m0.shape == (2, 4, 0) and torch.equal(c0, torch.zeros(2))


@pytest.mark.parametrize("d", [2, 5, 6])
def test_earth_mover_distance_nd_forward_and_backward(d):
    b, n, m = 2, 40, 40
    a = _rand(21, b, n, d).requires_grad_(True)
    c = _rand(22, b, m, d).requires_grad_(True)
    w = _rand(23, b)
    dist = earth_mover_distance_nd(a, c)
    match = cpu_ops.approxmatch_forward_nd(a.detach(), c.detach())
    cost = cpu_ops.matchcost_forward_nd(a.detach(), c.detach(), match)
    assert torch.equal(dist.detach(), cost / n)
    (dist * w).sum().backward()
    g1, g2 = cpu_ops.matchcost_backward_nd(w / n, a.detach(), c.detach(), match)
    torch.testing.assert_close(a.grad, g1, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(c.grad, g2, rtol=1e-6, atol=1e-7)
    # transposed input, a 2-D pair and a forward that needs no gradient
    dt = earth_mover_distance_nd(a.detach().transpose(1, 2), c.detach().transpose(1, 2),
                                 transpose=True)
    assert torch.equal(dt, dist.detach())
    one = earth_mover_distance_nd(a.detach()[0], c.detach()[0])
    assert one.shape == (1,) and torch.equal(one[0], dist.detach()[0])
    assert not EarthMoverDistanceNDFunction.apply(a.detach(), c.detach()).requires_grad


def test_earth_mover_distance_nd_at_d3_is_the_3d_function():
    a, c = _rand(31, 2, 33, 3), _rand(32, 2, 33, 3)
    assert torch.equal(earth_mover_distance_nd(a, c), earth_mover_distance(a, c, transpose=False))


# ---- 3. the metrics -----------------------------------------------------------------------------
def test_pairwise_emd_nd():
    x3, y3 = _rand(41, 3, 24, 3), _rand(42, 4, 24, 3)
    assert torch.equal(metrics.pairwise_emd_nd(x3, y3), metrics.pairwise_emd(x3, y3))
    for d in (2, 5, 6):
        x, y = _rand(43 + d, 3, 24, d), _rand(53 + d, 4, 24, d)
        full = metrics.pairwise_emd_nd(x, y)
        assert full.shape == (3, 4) and full.dtype == torch.float32
        one = metrics._emd_nd_chunk_bytes(1, 24, 24, d, x)
        # the chunking does not show.  Every chunk here holds at least two pairs: on CPU
        # tensors a call on ONE pair sends torch's einsum down its matrix-vector route,
        # whose sums round differently (the kernels have no such case:
        # tests/test_gpu_emd_nd.py holds one pair against a batch bit for bit)
        for pairs in (5, 6, 12):
            lim = metrics._emd_nd_chunk_bytes(pairs, 24, 24, d, x)
            assert metrics._emd_pairs_per_chunk(12, 24, 24, lim, x, d) == pairs
            assert metrics._emd_pairs_per_chunk(12, 24, 24, lim - 1, x, d) == pairs - 1
            assert torch.equal(metrics.pairwise_emd_nd(x, y, max_bytes=lim), full)
        with pytest.raises(ValueError, match="max_bytes"):
            metrics.pairwise_emd_nd(x, y, max_bytes=one - 1)
        # entry [i, j] is the pair's own cost over all D components, x[i] as p1
        _, cost = ops.approxmatch_cost_forward_nd(x[[2, 0]], y[[1, 3]], want_match=False)
        assert torch.equal(full[2, 1], cost[0] / 24) and torch.equal(full[0, 3], cost[1] / 24)
        # a strided view gives the contiguous copy's bits
        xt = x.transpose(0, 1).contiguous().transpose(0, 1)
        assert not xt.is_contiguous() and torch.equal(metrics.pairwise_emd_nd(xt, y), full)
    x6 = _rand(61, 3, 24, 6)
    for bad in (_rand(62, 4, 20, 6), _rand(62, 4, 24, 5), _rand(62, 24, 6)):
        with pytest.raises(ValueError):
            metrics.pairwise_emd_nd(x6, bad)
    for d in (1, 4, 7):
        with pytest.raises(ValueError):
            metrics.pairwise_emd_nd(_rand(1, 2, 8, d), _rand(2, 2, 8, d))
    assert metrics.pairwise_emd_nd(torch.zeros(0, 8, 6), torch.zeros(3, 8, 6)).shape == (0, 3)
    assert torch.equal(metrics.pairwise_emd_nd(torch.zeros(2, 0, 6), torch.zeros(3, 0, 6)),
                       torch.zeros(2, 3))
    # the 3-D function still refuses anything but D = 3
    with pytest.raises(ValueError):
        metrics.pairwise_emd(x6, x6)


def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_generation_metrics_emd_components():
    s, r = _rand(71, 5, 32, 6) - 0.5, _rand(72, 4, 32, 6) - 0.5
    base = metrics.generation_metrics(s, r)
    _same_dict(metrics.generation_metrics(s, r, emd_components="xyz"), base)
    _same_dict(metrics.generation_metrics(s, r, jsd=True, emd_components="xyz"),
               metrics.generation_metrics(s, r, jsd=True))
    got = metrics.generation_metrics(s, r, emd_components="all")
    assert sorted(got) == sorted(base)
    mxy = metrics.pairwise_emd_nd(s, r)
    want = {f"{k}_emd": v for k, v in metrics.mmd_cov(mxy).items()}
    nna = metrics.one_nna(metrics.pairwise_emd_nd(s, s), mxy, metrics.pairwise_emd_nd(r, r))
    want.update({"1nna_emd": nna["acc"], "1nna_gen_emd": nna["acc_gen"],
                 "1nna_ref_emd": nna["acc_ref"]})
    _same_dict({k: v for k, v in got.items() if k.endswith("_emd")}, want)
    _same_dict({k: v for k, v in got.items() if k.endswith("_cd")},
               {k: v for k, v in base.items() if k.endswith("_cd")})
    # colour is seen: the xyz figure is not the all-components one
    assert not torch.equal(got["mmd_emd"], base["mmd_emd"])
    # D = 2: "xyz" has no third component, "all" works
    s2, r2 = s[..., :2].contiguous(), r[..., :2].contiguous()
    with pytest.raises(ValueError):
        metrics.generation_metrics(s2, r2)
    g2 = metrics.generation_metrics(s2, r2, emd_components="all")
    assert torch.equal(g2["mmd_emd"], metrics.mmd_cov(metrics.pairwise_emd_nd(s2, r2))["mmd"])
    # with n_points both sets are subsampled first, as for "xyz"
    sub = metrics.generation_metrics(s, r, n_points=16, emd_components="all")
    assert torch.equal(sub["mmd_emd"], metrics.mmd_cov(metrics.pairwise_emd_nd(
        metrics.subsample(s, 16), metrics.subsample(r, 16)))["mmd"])
    for bad in ("rgb", "", None, "ALL"):
        with pytest.raises(ValueError, match="emd_components"):
            metrics.generation_metrics(s, r, emd_components=bad)
    with pytest.raises(ValueError):                    # unequal point counts
        metrics.generation_metrics(s, r[:, :20].contiguous(), emd_components="all")


# ---- 4. the sixth ABI table ------------------------------------------------------------------------
def test_header_and_binding_agree():
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(pcfm_[a-z0-9_]+)\s*\(", text))) == EMD_ND
    for other in (_lib.SIGNATURES, _lib.ND_SIGNATURES, _lib.CROSS_SIGNATURES,
                  _lib.FPS_SIGNATURES, _lib.OCCUPANCY_SIGNATURES):
        assert not set(_lib.EMD_ND_SIGNATURES) & set(other)
    lib = _lib.load()
    for name in EMD_ND:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EMD_ND_SIGNATURES[name][1], name  # declared by load()
        assert fn.restype == _lib.EMD_ND_SIGNATURES[name][0], name
    assert lib.pcfm_emd_nd_abi_version() == 1 == _lib.EMD_ND_ABI_VERSION
    # the five older versions are untouched by the new sibling header
    assert lib.pcfm_abi_version() == _lib.ABI_VERSION == 20
    assert lib.pcfm_chamfer_nd_abi_version() == _lib.ND_ABI_VERSION == 1
    assert lib.pcfm_chamfer_cross_abi_version() == _lib.CROSS_ABI_VERSION == 1
    assert lib.pcfm_fps_abi_version() == _lib.FPS_ABI_VERSION == 1
    assert lib.pcfm_occupancy_abi_version() == _lib.OCCUPANCY_ABI_VERSION == 1


# ---- 5. the host plan and the host-side refusals (no GPU is touched) ----------------------------------
def test_plan_and_refusals_on_the_host():
    lib = _lib.load()
    q = lib.pcfm_emd_nd_workspace_bytes

    def err():
        return lib.pcfm_last_error().decode()

    def fwd(b, n, m, d, ws_bytes=0, cost=1):
        # cost: any non-null address; a refused call dereferences nothing
        return lib.pcfm_emd_nd_approxmatch_cost_f32(None, None, b, n, m, d, None, cost, None,
                                                    ws_bytes, None)

    def cost(b, n, m, d, ws_bytes=0):
        return lib.pcfm_emd_nd_matchcost_f32(None, None, None, b, n, m, d, None, None, ws_bytes,
                                             None)

    def bwd(b, n, m, d, ws_bytes=0):
        return lib.pcfm_emd_nd_matchcost_bwd_f32(None, None, None, None, b, n, m, d, None, None,
                                                 None, ws_bytes, None)

    for d in range(-1, 10):
        assert lib.pcfm_emd_nd_supported(d) == int(d in (2, 3, 5, 6))
    for d in (2, 3, 5, 6):
        assert lib.pcfm_emd_nd_supported(d) == 1
    for d in (1, 4, 7):
        assert lib.pcfm_emd_nd_supported(d) == 0
    for entry in (fwd, cost, bwd):
        for bad in ((-1, 10, 10), (2, -10, 10), (2, 10, -1)):
            assert entry(*bad, 6, 1 << 40) == -1 and "negative size" in err()
            assert q(*bad, 6) == 0
        for d in (1, 4, 7, 0, -3):
            assert entry(2, 100, 100, d, 1 << 40) == -1 and "unsupported dimension" in err()
            assert q(2, 100, 100, d) == 0
        for d in (2, 3, 5, 6):
            need = q(2, 100, 37, d)
            assert need > 0
            assert entry(2, 100, 37, d, need - 1) == -1
            assert f"workspace {need - 1} < {need}" in err()
    assert fwd(2, 100, 37, 6, 1 << 40, cost=None) == -1 and "cost is required" in err()
    with pytest.raises(_lib.PcfmError, match="workspace"):
        _lib.call("pcfm_emd_nd_matchcost_f32", None, None, None, 2, 100, 37, 6, None, None, 0, None)
    with pytest.raises(_lib.PcfmError, match="unsupported dimension 4"):
        _lib.call("pcfm_emd_nd_matchcost_f32", None, None, None, 2, 100, 37, 4, None, None,
                  1 << 40, None)
    # the plan: D <= 3 is the 3-D entries' plan (4-float packs), D = 5, 6 has 8-float packs
    for b, n, m in ((2, 100, 37), (8, 2048, 2048), (1, 70, 2200), (3, 1, 1), (0, 5, 5), (2, 0, 5)):
        q3 = lib.pcfm_emd_workspace_bytes(b, n, m, 4)
        assert q(b, n, m, 3) == q3
        assert q(b, n, m, 2) <= q3 <= q(b, n, m, 5) <= q(b, n, m, 6)
    # B = 8, N = M = 2048.  approxmatch: packs 3 * 16384 * pack, remL 16384, levL + levR
    # 20 * 16384, the match write's partials 8 * (2048 / 32) * (2048 / 256); the gradient:
    # S = 16 splits (4 waves per SIMD over 16384 rows) of 16384 * d partials; the larger holds
    rows = 8 * 2048
    for d, pack in ((2, 4), (3, 4), (5, 8), (6, 8)):
        fwd_elems = 3 * rows * pack + rows + 20 * rows + 8 * 64 * 8
        assert q(8, 2048, 2048, d) == 4 * max(fwd_elems, 16 * rows * d), d


# ---- 6. the shipped device code ---------------------------------------------------------------------------
def test_shipped_emd_nd_kernels_have_no_scratch(tmp_path):
    """One kernel family <T, D> (row passes <T, D, PH>) serves the 3-D and the N-D
    entries: float at D = 2, 3, 5, 6 and double at D = 3, every instance once."""
    assert codeobj.available(), "ROCm LLVM tools absent"
    names, found = [], {}
    for co in codeobj.extract(_lib.LIB_PATH, str(tmp_path)):
        for name, res in codeobj.kernel_resources(co).items():
            if "emd" in name and "emd_auction" not in name:
                names.append(name)
                found[name] = res
    assert len(names) == len(set(names)), sorted(names)      # no kernel in two code objects
    insts = [("f", d) for d in (2, 3, 5, 6)] + [("d", 3)]
    for kind, count in (("rowpass_kernelI%sLi%dELi%dEE", None), ("match_cost_kernelI%sLi%dEE", 1),
                        ("cost_kernelI%sLi%dEE", 1), ("grad1_kernelI%sLi%dEE", 1),
                        ("grad2_kernelI%sLi%dEE", 1), ("pack_kernelI%sLi%dEE", 1)):
        for t, d in insts:
            pats = [kind % (t, d, ph) for ph in range(4)] if count is None else [kind % (t, d)]
            for pat in pats:
                assert sum("emd_" + pat in k for k in found) == 1, pat
    for t in "fd":                                           # cost_fin and grad1_fin: per T alone
        for kind in ("cost_fin_kernelI%sE", "grad1_fin_kernelI%sE"):
            assert sum("emd_" + kind % t in k for k in found) == 1, (kind, t)
    # nothing else carries "emd": no second kernel for any <T, D, PH>
    assert len(found) == 5 * (4 + 5) + 2 * 2, sorted(found)
    for k, res in found.items():
        assert res["scratch"] == 0, (k, res)                 # double too: the 3-D double kernels had none
        if "rowpass" in k:
            assert res["wg"] == 1024, (k, res)
