"""CPU: the assignment EMD by auction (include/pcfm_emd_auction.h,
csrc/emd_auction.hip) without a GPU -- pcfm.cpu_ops.emd_auction, the rule in pure
PyTorch, against the float64 optimum stored in tests/golden/emd_auction.npz
(tests/golden/make_emd_auction_golden.py; no test reads scipy) and against brute
force; the not-finished contract; pairwise_emd_auction and the emd_match keyword of
generation_metrics; the autograd loss; the seventh ABI table, the host-side
refusals and the resources of the shipped kernels."""
import functools
import itertools
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

from pcfm import _lib, cpu_ops, metrics, ops  # noqa: E402
from PyTorchEMD.emd_auction import earth_mover_distance_auction  # noqa: E402

HEADER = os.path.join(REPO, "include", "pcfm_emd_auction.h")
AUCTION = sorted(_lib.EMD_AUCTION_SIGNATURES)
EPS_REL = 2.0 ** -16
CAP = 65536         # max_rounds: the fixture's maker asserts every case needs at most half
FIX = np.load(os.path.join(HERE, "golden", "emd_auction.npz"), allow_pickle=False)
NAMES = [str(s) for s in FIX["names"]]
SMALL = [s for s in NAMES if FIX[f"{s}_p1"].shape[1] < 2048]     # the reference runs here
LARGE = [s for s in NAMES if s not in SMALL]                     # its results are stored


def _rand(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _clouds(name):
    return torch.from_numpy(FIX[f"{name}_p1"]), torch.from_numpy(FIX[f"{name}_p2"])


def _costs(p1, p2):
    """The rule's fp32 costs c(i, j) as float64, (b, n, n)."""
    return cpu_ops._pair_sqdist_nd(p1, p2).double().numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """cpu_ops.emd_auction on a case, once for all tests."""
    return cpu_ops.emd_auction(*_clouds(name), EPS_REL, CAP)


def _check_against_optimum(name, assignment, cost):
    p1, p2 = _clouds(name)
    b, n, _ = p1.shape
    c = _costs(p1, p2)
    for bb in range(b):
        a = assignment[bb].tolist()
        assert sorted(a) == list(range(n)), (name, bb)
        opt, cmax = float(FIX[f"{name}_opt"][bb]), float(FIX[f"{name}_cmax"][bb])
        assert cmax == c[bb].max()
        got = float(cost[bb])
        gap = got - opt
        print(f"emd_auction {name}[{bb}]: cost {got:.6g}, optimum {opt:.6g}, gap {gap:.3g} of "
              f"the bound {n * EPS_REL * cmax:.3g}")
        assert opt * (1 - 1e-6) <= got <= opt + n * EPS_REL * cmax, (name, bb, got, opt)
        # the cost is the float64 sum over the assignment, rounded once
        np.testing.assert_allclose(got, c[bb][np.arange(n), a].sum(), rtol=1e-6)


# ---- 1. the CPU backend ------------------------------------------------------------------
def test_the_fixture_has_the_issues_cases():
    shapes = {s: FIX[f"{s}_p1"].shape for s in NAMES}
    for b, n, d in ((3, 1, 3), (2, 2, 6), (2, 3, 2), (2, 63, 5), (2, 64, 3), (2, 65, 6),
                    (2, 77, 6), (2, 300, 5), (1, 300, 2)):
        assert shapes[f"uniform_{b}x{n}x{d}"] == (b, n, d)
    assert shapes["p2_one_point"][1] == 100 and shapes["both_one_point"][1] == 50
    assert shapes["lattice_shifted"] == shapes["lattice_permuted"] == (1, 64, 3)
    assert shapes["cloud_permuted"][1] == 300 and shapes["clusters"][1] == 200
    assert shapes["uniform_1x2048x6"] == (1, 2048, 6)
    assert shapes["sphere_gaussian_1x2048x3"] == (1, 2048, 3)
    assert len(NAMES) == 17 and LARGE == ["uniform_1x2048x6", "sphere_gaussian_1x2048x3"]
    for s in NAMES:
        assert FIX[f"{s}_p2"].shape == shapes[s] and FIX[f"{s}_p1"].dtype == np.float32
    assert len(np.unique(FIX["p2_one_point_p2"][0], axis=0)) == 1
    assert len(np.unique(FIX["both_one_point_p1"][0], axis=0)) == 1
    assert len(np.unique(FIX["both_one_point_p2"][0], axis=0)) == 1


@pytest.mark.parametrize("name", SMALL)
def test_permutation_and_optimality_bound(name):
    assignment, cost, rounds = reference(name)
    b, n, _ = FIX[f"{name}_p1"].shape
    assert assignment.shape == (b, n) and assignment.dtype == torch.int32
    assert cost.shape == (b,) and cost.dtype == torch.float32
    assert rounds.shape == (b,) and rounds.dtype == torch.int32
    assert bool((rounds > 0).all()) and bool((rounds <= CAP // 2).all()), rounds
    _check_against_optimum(name, assignment, cost)


@pytest.mark.parametrize("name", LARGE)
def test_the_stored_reference_of_the_large_cases(name):
    """n = 2048: the reference's results as the fixture's maker stored them (the GPU
    test compares against these) meet the same bounds."""
    assignment = torch.from_numpy(FIX[f"{name}_assignment"])
    p1, p2 = _clouds(name)
    c = _costs(p1, p2)[0]
    cost = torch.tensor([c[np.arange(2048), assignment[0].numpy()].sum()]).float()
    assert 0 < int(FIX[f"{name}_rounds"][0]) <= CAP // 2
    _check_against_optimum(name, assignment, cost)


@pytest.mark.parametrize("name", ["uniform_3x1x3", "uniform_2x2x6", "uniform_2x3x2"])
def test_against_brute_force(name):
    p1, p2 = _clouds(name)
    b, n, _ = p1.shape
    assert n <= 6
    c = _costs(p1, p2)
    _, cost, _ = reference(name)
    for bb in range(b):
        best = min(sum(c[bb][i, p[i]] for i in range(n)) for p in
                   itertools.permutations(range(n)))
        np.testing.assert_allclose(best, FIX[f"{name}_opt"][bb], rtol=1e-12)
        assert best * (1 - 1e-6) <= float(cost[bb]) <= best + n * EPS_REL * c[bb].max()


@pytest.mark.parametrize("name", SMALL)
def test_orientation(name):
    """cost(a, b) and cost(b, a) are both within n * eps_final of ONE optimum."""
    p1, p2 = _clouds(name)
    n = p1.shape[1]
    _, fwd, _ = reference(name)
    back_a, back, rounds = cpu_ops.emd_auction(p2, p1, EPS_REL, CAP)
    assert bool((rounds >= 0).all())
    for bb in range(p1.shape[0]):
        assert sorted(back_a[bb].tolist()) == list(range(n))
        bound = n * EPS_REL * float(FIX[f"{name}_cmax"][bb])
        assert abs(float(fwd[bb]) - float(back[bb])) <= bound, (name, bb)


def test_special_cases():
    # a cloud against a permutation of itself: cost exactly 0, the inverse permutation
    p1, p2 = _clouds("cloud_permuted")
    a, cost, _ = reference("cloud_permuted")
    assert float(cost[0]) == 0.0 and torch.equal(p2[0][a[0].long()], p1[0])
    a, cost, _ = reference("lattice_permuted")
    p1, p2 = _clouds("lattice_permuted")
    assert float(cost[0]) == 0.0 and torch.equal(p2[0][a[0].long()], p1[0])
    # identical clouds, every cost 0 on the diagonal only: still the identity
    x = _rand(1, 2, 40, 5)
    a, cost, rounds = cpu_ops.emd_auction(x, x.clone())
    assert torch.equal(a, torch.arange(40, dtype=torch.int32).expand(2, 40)) and not cost.any()
    # cmax == 0 (all points one point): the identity, cost 0, rounds 0
    one = _rand(2, 1, 1, 3).expand(2, 30, 3).contiguous()
    a, cost, rounds = cpu_ops.emd_auction(one, one.clone())
    assert torch.equal(a, torch.arange(30, dtype=torch.int32).expand(2, 30))
    assert not cost.any() and not rounds.any()
    # a batch's pairs are problems of their own
    p1, p2 = _clouds("uniform_2x77x6")
    whole = reference("uniform_2x77x6")
    alone = cpu_ops.emd_auction(p1[1:], p2[1:], EPS_REL, CAP)
    for w, o in zip(whole, alone):
        assert torch.equal(w[1:], o)
    # empty problems
    a, cost, rounds = ops.emd_auction(torch.zeros(2, 0, 6), torch.zeros(2, 0, 6))
    assert a.shape == (2, 0) and not cost.any() and not rounds.any() and cost.shape == (2,)
    a, cost, rounds = ops.emd_auction(torch.zeros(0, 5, 3), torch.zeros(0, 5, 3))
    assert a.shape == (0, 5) and cost.shape == (0,) and rounds.shape == (0,)


def test_not_finished_at_one_round():
    p1, p2 = _clouds("uniform_2x64x3")
    p1, p2 = p1[:1].contiguous(), p2[:1].contiguous()
    a, cost, rounds = ops.emd_auction(p1, p2, max_rounds=1)
    assert rounds.tolist() == [-1] and bool((a == -1).all()) and bool(torch.isnan(cost).all())
    none, cost, rounds = ops.emd_auction(p1, p2, max_rounds=1, want_assignment=False)
    assert none is None and rounds.tolist() == [-1] and bool(torch.isnan(cost).all())
    with pytest.raises(RuntimeError, match="1 of 1 pairs did not finish"):
        metrics.pairwise_emd_auction(p1, p2, max_rounds=1)
    with pytest.raises(RuntimeError, match="did not finish"):
        earth_mover_distance_auction(p1, p2, max_rounds=1)
    # a cap the auction stays within changes nothing, down to the exact round count
    full = reference("uniform_2x64x3")
    need = int(full[2][0])
    for got, want in zip(ops.emd_auction(p1, p2, max_rounds=need), full):
        assert torch.equal(got, want[:1])
    assert ops.emd_auction(p1, p2, max_rounds=need - 1)[2].tolist() == [-1]


def test_the_op_checks_its_arguments():
    x = _rand(3, 2, 8, 3)
    for bad in (_rand(4, 2, 9, 3), _rand(4, 3, 8, 3), _rand(4, 2, 8, 2), _rand(4, 8, 3)):
        with pytest.raises(RuntimeError, match="one shape"):
            ops.emd_auction(x, bad)
    with pytest.raises(RuntimeError, match="D = 4"):
        ops.emd_auction(_rand(5, 2, 8, 4), _rand(6, 2, 8, 4))
    with pytest.raises(RuntimeError, match="float tensor"):
        ops.emd_auction(x.double(), x.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.emd_auction(x.transpose(0, 1), x.transpose(0, 1))
    for eps in (0.0, 2.0 ** -21, 0.6, float("nan"), float("inf"), -0.1):
        with pytest.raises(RuntimeError, match="eps_rel"):
            ops.emd_auction(x, x, eps_rel=eps)
    for cap in (0, -5, 1 << 31):
        with pytest.raises(RuntimeError, match="max_rounds"):
            ops.emd_auction(x, x, max_rounds=cap)
    # the two ends of the eps range are accepted; a coarser eps needs no more rounds
    coarse = ops.emd_auction(x, x.flip(1).contiguous(), eps_rel=0.5)
    fine = ops.emd_auction(x, x.flip(1).contiguous(), eps_rel=2.0 ** -20)
    assert bool((coarse[2] > 0).all()) and bool((coarse[2] <= fine[2]).all())
    assert not fine[1].any() and torch.equal(fine[0], torch.arange(7, -1, -1).int().expand(2, 8))


# ---- 2. the metrics ----------------------------------------------------------------------
def test_pairwise_emd_auction():
    x, y = _rand(11, 4, 24, 6) - 0.5, _rand(12, 3, 24, 6) - 0.5
    full = metrics.pairwise_emd_auction(x, y)
    assert full.shape == (4, 3) and full.dtype == torch.float32
    for i in range(4):
        for j in range(3):
            _, cost, _ = cpu_ops.emd_auction(x[i:i + 1], y[j:j + 1])
            assert torch.equal(full[i, j], (cost / 24)[0])
    # the chunking does not show, down to one pair per call
    pair = 2 * 24 * 6 * 4 + 3 * 24 * 24 * 4
    for pairs in (1, 5, 12):
        assert torch.equal(metrics.pairwise_emd_auction(x, y, max_bytes=pairs * pair), full)
    with pytest.raises(ValueError, match="max_bytes"):
        metrics.pairwise_emd_auction(x, y, max_bytes=pair - 1)
    # the transpose agrees within the bound: eps_rel * cmax per entry after the division by n
    back = metrics.pairwise_emd_auction(y, x)
    for i in range(4):
        for j in range(3):
            cmax = float(cpu_ops._pair_sqdist_nd(x[i:i + 1], y[j:j + 1]).max())
            assert abs(float(full[i, j]) - float(back[j, i])) <= EPS_REL * cmax * (1 + 1e-6)
    # a set against itself: a zero diagonal, symmetric within the bound
    xx = metrics.pairwise_emd_auction(x, x)
    assert not xx.diagonal().any()
    assert float((xx - xx.t()).abs().max()) <= EPS_REL * 6.0
    xt = x.transpose(1, 2).contiguous().transpose(1, 2)         # not contiguous
    assert not xt.is_contiguous() and torch.equal(metrics.pairwise_emd_auction(xt, y), full)
    for d in (1, 4, 7):
        with pytest.raises(ValueError):
            metrics.pairwise_emd_auction(_rand(1, 2, 8, d), _rand(2, 2, 8, d))
    with pytest.raises(ValueError, match="point counts"):
        metrics.pairwise_emd_auction(x, y[:, :20].contiguous())
    with pytest.raises(ValueError):
        metrics.pairwise_emd_auction(x, y[..., :5].contiguous())
    assert metrics.pairwise_emd_auction(torch.zeros(0, 8, 6), torch.zeros(3, 8, 6)).shape == (0, 3)
    assert torch.equal(metrics.pairwise_emd_auction(torch.zeros(2, 0, 6), torch.zeros(3, 0, 6)),
                       torch.zeros(2, 3))
    assert "pairwise_emd_auction" in metrics.__all__ and "emd_auction" in cpu_ops.__all__


def _same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k


def test_generation_metrics_emd_match():
    s, r = _rand(71, 5, 32, 6) - 0.5, _rand(72, 4, 32, 6) - 0.5
    base = metrics.generation_metrics(s, r)
    _same_dict(metrics.generation_metrics(s, r, emd_match="approx"), base)
    _same_dict(metrics.generation_metrics(s, r, jsd=True, emd_components="all",
                                          emd_match="approx"),
               metrics.generation_metrics(s, r, jsd=True, emd_components="all"))
    # the default's _emd entries are the approximate match's, as before the keyword
    mxy = metrics.pairwise_emd(s[..., :3].contiguous(), r[..., :3].contiguous())
    assert torch.equal(base["mmd_emd"], metrics.mmd_cov(mxy)["mmd"])
    for comp, pick in (("xyz", lambda t: t[..., :3].contiguous()), ("all", lambda t: t)):
        got = metrics.generation_metrics(s, r, emd_components=comp, emd_match="auction")
        assert sorted(got) == sorted(base)
        a, b = pick(s), pick(r)
        mxy = metrics.pairwise_emd_auction(a, b)
        want = {f"{k}_emd": v for k, v in metrics.mmd_cov(mxy).items()}
        nna = metrics.one_nna(metrics.pairwise_emd_auction(a, a), mxy,
                              metrics.pairwise_emd_auction(b, b))
        want.update({"1nna_emd": nna["acc"], "1nna_gen_emd": nna["acc_gen"],
                     "1nna_ref_emd": nna["acc_ref"]})
        _same_dict({k: v for k, v in got.items() if k.endswith("_emd")}, want)
        _same_dict({k: v for k, v in got.items() if k.endswith("_cd")},
                   {k: v for k, v in base.items() if k.endswith("_cd")})
        assert not torch.equal(got["mmd_emd"], base["mmd_emd"])
    # emd=False never reaches the match; n_points subsamples first
    _same_dict(metrics.generation_metrics(s, r, emd=False, emd_match="auction"),
               metrics.generation_metrics(s, r, emd=False))
    sub = metrics.generation_metrics(s, r, n_points=16, emd_components="all", emd_match="auction")
    assert torch.equal(sub["mmd_emd"], metrics.mmd_cov(metrics.pairwise_emd_auction(
        metrics.subsample(s, 16), metrics.subsample(r, 16)))["mmd"])
    for bad in ("exact", "", None, "AUCTION"):
        with pytest.raises(ValueError, match="emd_match"):
            metrics.generation_metrics(s, r, emd_match=bad)
    with pytest.raises(ValueError):                    # unequal point counts
        metrics.generation_metrics(s, r[:, :20].contiguous(), emd_match="auction")
    with pytest.raises(ValueError):                    # "xyz" has no third component at D = 2
        metrics.generation_metrics(s[..., :2].contiguous(), r[..., :2].contiguous(),
                                   emd_match="auction")


# ---- 3. the loss ---------------------------------------------------------------------------
def test_the_loss_under_autograd():
    b, n, d = 2, 40, 5
    a, c, w = _rand(21, b, n, d), _rand(22, b, n, d), _rand(23, b)
    p1, p2 = a.clone().requires_grad_(True), c.clone().requires_grad_(True)
    dist = earth_mover_distance_auction(p1, p2)
    assignment, cost, _ = cpu_ops.emd_auction(a, c)
    assert dist.shape == (b,) and dist.requires_grad
    np.testing.assert_allclose(dist.detach().numpy(), (cost / n).numpy(), rtol=1e-6)
    (dist * w).sum().backward()
    # the gather's gradient, exactly as torch computes it from the constant assignment
    q1, q2 = a.clone().requires_grad_(True), c.clone().requires_grad_(True)
    idx = assignment.long()[:, :, None].expand(-1, -1, d)
    ((q1 - torch.gather(q2, 1, idx)).square().sum(dim=2).mean(dim=1) * w).sum().backward()
    assert torch.equal(p1.grad, q1.grad) and torch.equal(p2.grad, q2.grad)
    # in closed form: 2 (p1[i] - p2[a(i)]) / n at p1[i], its mirror at p2[a(i)]
    g1 = 2 * (a - torch.gather(c, 1, idx)) / n * w[:, None, None]
    np.testing.assert_allclose(p1.grad.numpy(), g1.numpy(), rtol=1e-5, atol=1e-7)
    g2 = torch.zeros_like(c).scatter_add(1, idx, -g1)
    np.testing.assert_allclose(p2.grad.numpy(), g2.numpy(), rtol=1e-5, atol=1e-7)
    # one pair without a batch dimension, and a forward that needs no gradient
    one = earth_mover_distance_auction(a[0], c[0])
    assert one.shape == (1,) and torch.equal(one, dist.detach()[:1]) and not one.requires_grad


# ---- 4. the seventh ABI table --------------------------------------------------------------
def test_header_and_binding_agree():
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(pcfm_[a-z0-9_]+)\s*\(", text))) == AUCTION
    for other in (_lib.SIGNATURES, _lib.ND_SIGNATURES, _lib.CROSS_SIGNATURES,
                  _lib.FPS_SIGNATURES, _lib.OCCUPANCY_SIGNATURES, _lib.EMD_ND_SIGNATURES):
        assert not set(_lib.EMD_AUCTION_SIGNATURES) & set(other)
    lib = _lib.load()
    for name in AUCTION:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.EMD_AUCTION_SIGNATURES[name][1], name  # declared by load()
        assert fn.restype == _lib.EMD_AUCTION_SIGNATURES[name][0], name
    assert lib.pcfm_emd_auction_abi_version() == 1 == _lib.EMD_AUCTION_ABI_VERSION
    # the six older versions are untouched by the new sibling header
    assert lib.pcfm_abi_version() == _lib.ABI_VERSION == 20
    assert lib.pcfm_chamfer_nd_abi_version() == _lib.ND_ABI_VERSION == 1
    assert lib.pcfm_chamfer_cross_abi_version() == _lib.CROSS_ABI_VERSION == 1
    assert lib.pcfm_fps_abi_version() == _lib.FPS_ABI_VERSION == 1
    assert lib.pcfm_occupancy_abi_version() == _lib.OCCUPANCY_ABI_VERSION == 1
    assert lib.pcfm_emd_nd_abi_version() == _lib.EMD_ND_ABI_VERSION == 1


# ---- 5. the host-side refusals (no GPU is touched) -------------------------------------------
def test_refusals_on_the_host():
    lib = _lib.load()

    def err():
        return lib.pcfm_last_error().decode()

    def call(b=2, n=100, d=6, eps=EPS_REL, cap=CAP, cost=1, rounds=1):
        # cost, rounds: any non-null address; a refused call dereferences nothing
        return lib.pcfm_emd_auction_f32(None, None, b, n, d, eps, cap, None, cost, rounds, None,
                                        0, None)

    for d in range(-1, 10):
        top = lib.pcfm_emd_auction_max_points(d)
        assert (top >= 2048) if d in (2, 3, 5, 6) else (top == 0), d
        assert lib.pcfm_emd_auction_workspace_bytes(2, 100, d) == 0
    assert call(b=-1) == -1 and "negative size" in err()
    assert call(n=-1) == -1 and "negative size" in err()
    for d in (1, 4, 7, 0, -3):
        assert call(d=d) == -1 and "unsupported dimension" in err()
    for d in (2, 3, 5, 6):
        top = lib.pcfm_emd_auction_max_points(d)
        assert call(n=top + 1, d=d) == -1 and f"n = {top + 1} above" in err()
    for eps in (0.0, 2.0 ** -21, 0.5000001, float("nan"), float("inf"), -1.0):
        assert call(eps=eps) == -1 and "eps_rel" in err(), eps
    for cap in (0, -1):
        assert call(cap=cap) == -1 and "max_rounds" in err()
    assert call(cost=None) == -1 and "cost and rounds are required" in err()
    assert call(rounds=None) == -1 and "cost and rounds are required" in err()
    # b == 0 does nothing, whatever the pointers
    assert call(b=0, cost=None, rounds=None) == 0
    with pytest.raises(_lib.PcfmError, match="unsupported dimension 4"):
        _lib.call("pcfm_emd_auction_f32", None, None, 2, 100, 4, EPS_REL, CAP, None, 1, 1, None,
                  0, None)


# ---- 6. the shipped device code ------------------------------------------------------------
def test_shipped_auction_kernels_fit_the_block(tmp_path):
    """One 1024-thread block per pair: at most 128 VGPRs a lane, no scratch, and a
    static LDS share that leaves the n = 2048, d = 6 state (144 KiB) inside the
    160 KiB of a CU."""
    assert codeobj.available(), "ROCm LLVM tools absent"
    found = {}
    for co in codeobj.extract(_lib.LIB_PATH, str(tmp_path)):
        for name, res in codeobj.kernel_resources(co).items():
            if "emd_auction_kernel" in name:
                found[name] = res
    for d in (2, 3, 5, 6):
        assert sum(f"emd_auction_kernelILi{d}E" in k for k in found) == 1, (d, sorted(found))
    assert len(found) == 4
    for k, res in found.items():
        print(k, res)
        assert res["scratch"] == 0 and res["wg"] == 1024 and res["vgpr"] <= 128, (k, res)
        assert res["lds"] + 2048 * (8 * 6 + 24) <= 160 * 1024, (k, res)
