"""CPU: the generation metrics (pcfm/metrics.py) and the set-against-set Chamfer
entry points behind them (include/pcfm_chamfer_cross.h, csrc/chamfer_cross.hip)
without a GPU -- the third ABI table, the host-side refusals, the reductions on
hand-written matrices, the CPU backend against float64 brute force, the EMD
matrix against one-pair calls, and what the shipped library's device code
contains."""
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

from pcfm import _lib, metrics, ops  # noqa: E402
from pcfm.sample import chamfer_l2  # noqa: E402

HEADER = os.path.join(REPO, "include", "pcfm_chamfer_cross.h")
CROSS = sorted(_lib.CROSS_SIGNATURES)
DIMS = (2, 3, 5, 6)


# ---- 1. the third ABI table -----------------------------------------------------
def test_header_and_binding_agree():
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(pcfm_[a-z0-9_]+)\s*\(", text))) == CROSS
    assert not set(_lib.CROSS_SIGNATURES) & set(_lib.SIGNATURES)
    assert not set(_lib.CROSS_SIGNATURES) & set(_lib.ND_SIGNATURES)
    lib = _lib.load()
    for name in CROSS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.CROSS_SIGNATURES[name][1], name  # declared by load()
        assert fn.restype == _lib.CROSS_SIGNATURES[name][0], name
    assert lib.pcfm_chamfer_cross_abi_version() == 1 == _lib.CROSS_ABI_VERSION
    # the other two versions are untouched by the new sibling header
    assert lib.pcfm_abi_version() == _lib.ABI_VERSION
    assert lib.pcfm_chamfer_nd_abi_version() == _lib.ND_ABI_VERSION


# ---- 2. host-side refusals (no GPU is touched) ------------------------------------
def test_refusals_on_the_host():
    lib = _lib.load()
    q = lib.pcfm_chamfer_cross_workspace_bytes

    def err():
        return lib.pcfm_last_error().decode()

    def fwd(s, r, n, m, d, ws_bytes=0):
        return lib.pcfm_chamfer_cross_fwd(None, None, s, r, n, m, d, None, None, None, ws_bytes,
                                          None)

    for bad in ((-1, 2, 10, 10), (2, -1, 10, 10), (2, 2, -10, 10), (2, 2, 10, -1)):
        assert fwd(*bad, 6) == -1 and "negative size" in err()
        assert q(*bad, 6) == 0
    for d in (4, 0, 1, 7, -3):
        assert fwd(2, 2, 10, 10, d) == -1 and f"unsupported dimension {d}" in err()
        assert q(2, 2, 3000, 10, d) == 0
    assert [lib.pcfm_chamfer_cross_supported(d) for d in range(-1, 9)] == \
        [0, 0, 0, 1, 1, 0, 1, 1, 0, 0]
    # oversize: s * r, s * n, r * m and the block count s * r * (query blocks) < 2^31
    for big in ((1 << 16, 1 << 16, 4, 4), (2, 2, 1 << 30, 4), (2, 2, 4, 1 << 30),
                (1 << 15, 1 << 15, 2049, 2049)):
        assert fwd(*big, 2, 1 << 40) == -1 and "too large" in err()
        assert q(*big, 2) == 0
    # clouds of at most 2048 points need no workspace; above, one float64 per
    # (pair, block of 2048 queries) of the direction whose clouds are that large
    assert q(1000, 1000, 2048, 2048, 6) == 0
    assert q(2, 2, 2049, 300, 3) == 2 * 2 * 2 * 8
    assert q(3, 5, 100, 4097, 5) == 3 * 5 * 3 * 8
    assert q(3, 5, 2049, 4097, 5) == 3 * 5 * (2 + 3) * 8
    assert q(0, 5, 2049, 300, 3) == 0 and q(5, 0, 2049, 300, 3) == 0
    assert q(2, 2, 2049, 0, 3) == 0
    assert fwd(2, 2, 2049, 300, 3, 63) == -1 and "workspace 63 < 64" in err()
    with pytest.raises(_lib.PcfmError, match="workspace"):
        _lib.call("pcfm_chamfer_cross_fwd", None, None, 2, 2, 2049, 300, 3, None, None, None, 0,
                  None)
    # nothing to do: no launch, no error
    assert fwd(0, 5, 10, 10, 3) == 0 and fwd(5, 0, 10, 10, 3) == 0


def test_ops_wrapper_refuses_shapes_and_dtypes():
    a = torch.zeros(2, 5, 3)
    for bad in ((a, torch.zeros(2, 5, 6)), (a, torch.zeros(5, 3)), (a.double(), a.double()),
                (torch.zeros(2, 5, 4), torch.zeros(2, 5, 4)), (a.transpose(0, 1), a)):
        with pytest.raises(RuntimeError):
            ops.chamfer_cross_forward(*bad)
    ab, ba = ops.chamfer_cross_forward(a, torch.zeros(3, 0, 3))       # an empty cloud: zeros
    assert ab.shape == ba.shape == (2, 3) and not ab.any() and not ba.any()
    ab, ba = ops.chamfer_cross_forward(torch.zeros(0, 5, 3), a)
    assert ab.shape == ba.shape == (0, 2)


# ---- 3. the reductions on hand-written matrices -------------------------------------
def test_mmd_cov_by_hand():
    # column minima 1, 2 -> mmd 1.5; row minima 1, 2, 3 -> mmd_smp 2; row argmins
    # 0, 0 (a tie 2 == 2: the lowest index; the highest would give cov 1), 0 -> cov 1/2
    out = metrics.mmd_cov(torch.tensor([[1.0, 4.0], [2.0, 2.0], [3.0, 5.0]]))
    assert sorted(out) == ["cov", "mmd", "mmd_smp"]
    assert (out["mmd"].item(), out["mmd_smp"].item(), out["cov"].item()) == (1.5, 2.0, 0.5)
    # column minima 3, 1, 0.5 -> 1.5; row minima 1, 0.5, 1 -> 2.5 / 3; row argmins
    # 1, 2, 1 -> two distinct columns of three
    out = metrics.mmd_cov(torch.tensor([[3.0, 1.0, 2.0], [3.0, 5.0, 0.5], [4.0, 1.0, 7.0]]))
    assert out["mmd"].item() == 1.5
    np.testing.assert_allclose(out["mmd_smp"].item(), 2.5 / 3, rtol=1e-7)
    np.testing.assert_allclose(out["cov"].item(), 2 / 3, rtol=1e-7)
    with pytest.raises(ValueError):
        metrics.mmd_cov(torch.zeros(0, 3))


def test_one_nna_by_hand():
    mxx = torch.tensor([[0.0, 1.0, 6.0], [1.0, 0.0, 7.0], [6.0, 7.0, 0.0]])
    mxy = torch.tensor([[5.0, 9.0], [8.0, 9.0], [2.0, 9.0]])
    myy = torch.tensor([[0.0, 3.0], [3.0, 0.0]])
    # J, labels 1 1 1 0 0 (the diagonal is replaced by +inf whatever it holds):
    #   inf  1   6   5   9
    #   1   inf  7   8   9
    #   6   7   inf  2   9
    #   5   8   2   inf  3
    #   9   9   9   3   inf
    # column argmin rows 1, 0, 3, 2, 3 -> predictions 1, 1, 0, 1, 0 against labels
    # 1, 1, 1, 0, 0: right, right, wrong | wrong, right
    out = metrics.one_nna(mxx, mxy, myy)
    assert sorted(out) == ["acc", "acc_gen", "acc_ref"]
    np.testing.assert_allclose([out["acc"].item(), out["acc_gen"].item(), out["acc_ref"].item()],
                               [3 / 5, 2 / 3, 1 / 2], rtol=1e-7)
    # a tie: myy[0, 1] = myy[1, 0] = 9 makes the last column 9 9 9 9 inf; the lowest
    # index is row 0 (label 1): wrong (the highest, row 3, would be right).  Column 3
    # becomes 5 8 2 inf 9: still row 2, wrong.
    out = metrics.one_nna(mxx, mxy, torch.tensor([[0.0, 9.0], [9.0, 0.0]]))
    np.testing.assert_allclose([out["acc"].item(), out["acc_gen"].item(), out["acc_ref"].item()],
                               [2 / 5, 2 / 3, 0.0], rtol=1e-7)
    # 3 x 3 blocks; the lower left block is mxy TRANSPOSED, so mxy[0, 2] = 0.5 sits in
    # column 5 (row 0) and in column 0 (row 5):
    mxy3 = torch.tensor([[9.0, 9.0, 0.5], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0]])
    m3 = torch.tensor([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 3.0, 0.0]])
    # columns 0..2 (generated), mxx column | mxy row: col 0 = inf 1 2 | 9 9 0.5 -> row 5,
    # wrong (with the block not transposed: 9 9 9 -> row 1, right); col 1 = 1 inf 3 | 9 9 9
    # -> row 0, right; col 2 = 2 3 inf | 9 9 9 -> row 0, right
    # columns 3..5 (reference), mxy column | myy column: col 3 = 9 9 9 | inf 1 2 -> row 4,
    # right; col 4 = 9 9 9 | 1 inf 3 -> row 3, right; col 5 = 0.5 9 9 | 2 3 inf -> row 0, wrong
    out = metrics.one_nna(m3, mxy3, m3)
    np.testing.assert_allclose([out["acc"].item(), out["acc_gen"].item(), out["acc_ref"].item()],
                               [4 / 6, 2 / 3, 2 / 3], rtol=1e-7)
    with pytest.raises(ValueError):
        metrics.one_nna(mxx, mxy, mxx)


# ---- 4. pairwise_chamfer on the CPU backend -------------------------------------------
def brute_f64(x, y):
    """(ab, ba) float64 of numpy arrays x (S, N, D), y (R, M, D)."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    ab, ba = np.zeros((len(x), len(y))), np.zeros((len(x), len(y)))
    for i in range(len(x)):
        for j in range(len(y)):
            d2 = ((x[i][:, None, :] - y[j][None, :, :]) ** 2).sum(-1)
            ab[i, j], ba[i, j] = d2.min(1).mean(), d2.min(0).mean()
    return ab, ba


@pytest.mark.parametrize("d", DIMS)
def test_cpu_pairwise_chamfer(d):
    g = np.random.default_rng(40 + d)
    x = g.standard_normal((3, 50, d)).astype(np.float32)
    y = g.standard_normal((4, 37, d)).astype(np.float32)
    y[:, :12] = x[:3, :12][[0, 1, 2, 0]]                  # exact hits
    y[2] = x[1, :37]                                       # y[2] lies inside x[1]
    xs = np.concatenate([x, np.pad(y[3:4], ((0, 0), (0, 13), (0, 0)), mode="wrap")])
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    ab, ba = ops.chamfer_cross_forward(tx, ty)
    assert ab.dtype == ba.dtype == torch.float32 and ab.shape == ba.shape == (3, 4)
    eab, eba = brute_f64(x, y)
    # (D + 4) * 2^-24 <= 6e-7: the N-D test's (D + 3) * 2^-24 for the fp32 chain
    # plus the final rounding of the mean
    np.testing.assert_allclose(ab.numpy(), eab, rtol=1e-6, atol=0)
    np.testing.assert_allclose(ba.numpy(), eba, rtol=1e-6, atol=0)
    assert ba[1, 2] == 0                                   # every point of y[2] is in x[1]
    m = metrics.pairwise_chamfer(tx, ty)
    assert torch.equal(m, ab + ba)
    # chamfer_l2's CPU path is torch.cdist in fp32, which expands |p|^2 + |q|^2 - 2 p.q:
    # each squared distance is off by up to about (D + 4) * 2^-24 * (|p| + |q|)^2 <=
    # (D + 4) * 2^-24 * 4 * max |point|^2 in ABSOLUTE terms (it does not return 0 at an
    # exact hit), and so are the two means
    atol = 2 * (d + 4) * 2.0 ** -24 * 4 * float(max((x ** 2).sum(-1).max(), (y ** 2).sum(-1).max()))
    for i in range(3):
        for j in range(4):
            np.testing.assert_allclose(m[i, j].item(), chamfer_l2(tx[i:i + 1], ty[j:j + 1]).item(),
                                       rtol=1e-6, atol=atol)
    # a cloud present in both sets: exactly 0, and a set against itself has a 0 diagonal
    txs = torch.from_numpy(xs)
    assert xs.shape[0] == 4 and metrics.pairwise_chamfer(txs, ty)[3, 3] == 0
    assert (torch.diagonal(metrics.pairwise_chamfer(txs, txs)) == 0).all()


# ---- 5. pairwise_emd on the CPU backend ------------------------------------------------
def test_cpu_pairwise_emd():
    g = torch.Generator().manual_seed(11)
    x, y = torch.rand(3, 16, 3, generator=g), torch.rand(4, 16, 3, generator=g)
    m = metrics.pairwise_emd(x, y)
    assert m.shape == (3, 4) and m.dtype == torch.float32
    for i in range(3):
        for j in range(4):
            _, c = ops.approxmatch_cost_forward(x[i:i + 1], y[j:j + 1], want_match=False)
            assert m[i, j] == c[0] / 16, (i, j)        # xyz1 = x[i], xyz2 = y[j]
    # the chunking does not show: 4 pairs per call against all 12 in one
    four = metrics._emd_chunk_bytes(4, 16, 16, x)
    assert metrics._emd_pairs_per_chunk(12, 16, 16, four, x) == 4
    assert metrics._emd_pairs_per_chunk(12, 16, 16, 1 << 30, x) == 12
    assert torch.equal(metrics.pairwise_emd(x, y, max_bytes=four), m)
    with pytest.raises(ValueError, match="max_bytes"):
        metrics.pairwise_emd(x, y, max_bytes=100)
    with pytest.raises(ValueError):
        metrics.pairwise_emd(torch.rand(2, 16, 6), torch.rand(2, 16, 6))
    with pytest.raises(ValueError, match="point counts"):
        metrics.pairwise_emd(x, torch.rand(2, 17, 3))


def test_generation_metrics_keys_and_consistency():
    g = torch.Generator().manual_seed(5)
    s, r = torch.randn(4, 32, 6, generator=g), torch.randn(3, 32, 6, generator=g)
    cd = ["mmd_cd", "mmd_smp_cd", "cov_cd", "1nna_cd", "1nna_gen_cd", "1nna_ref_cd"]
    out = metrics.generation_metrics(s, r, emd=False)
    assert sorted(out) == sorted(cd)
    both = metrics.generation_metrics(s, r)
    assert sorted(both) == sorted(cd + [k[:-2] + "emd" for k in cd])
    mxy = metrics.pairwise_chamfer(s, r)
    exp = metrics.mmd_cov(mxy)
    nna = metrics.one_nna(metrics.pairwise_chamfer(s, s), mxy, metrics.pairwise_chamfer(r, r))
    assert both["mmd_cd"] == exp["mmd"] == out["mmd_cd"] and both["cov_cd"] == exp["cov"]
    assert both["1nna_cd"] == nna["acc"] and both["1nna_ref_cd"] == nna["acc_ref"]
    # EMD runs over xyz only
    e = metrics.pairwise_emd(s[..., :3].contiguous(), r[..., :3].contiguous())
    assert both["mmd_emd"] == metrics.mmd_cov(e)["mmd"]
    with pytest.raises(ValueError):          # EMD needs equal point counts
        metrics.generation_metrics(s, r[:, :20].contiguous())
    assert "mmd_cd" in metrics.generation_metrics(s, r[:, :20].contiguous(), emd=False)


# ---- 6. the shipped device code -----------------------------------------------------
def test_shipped_cross_kernels_have_no_scratch(tmp_path):
    assert codeobj.available(), "ROCm LLVM tools absent"
    fwd, fin, brute3 = {}, {}, []
    for co in codeobj.extract(_lib.LIB_PATH, str(tmp_path)):
        for name, res in codeobj.kernel_resources(co).items():
            # the per-point search whose query load and candidate walk cross_kernel shares
            # (csrc/chamfer_search.hpp): exactly one D = 3 forward kernel in the library
            if re.search(r"\dnn_kernel(ILi3E|E)|nn_nd_kernelILi3E", name):
                brute3.append(name)
            m = re.search(r"cross_kernelILi(\d+)E", name)
            if m:
                assert int(m.group(1)) not in fwd, name
                fwd[int(m.group(1))] = res
            elif "cross_finalize_kernel" in name:
                fin[name] = res
    assert sorted(fwd) == [2, 3, 5, 6]
    assert len(fin) == 1
    assert len(brute3) == 1, brute3
    for k, res in list(fwd.items()) + list(fin.items()):
        assert res["scratch"] == 0, (k, res)
    for k, res in fwd.items():
        assert res["wg"] == 256, (k, res)
