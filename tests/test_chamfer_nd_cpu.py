"""CPU: the D-component Chamfer distance (include/pcfm_chamfer_nd.h,
csrc/chamfer_nd.hip, chamfer{2,5,6}D/) without a GPU -- the sibling ABI table,
the host-side refusals, the CPU backend against the reference's
chamfer_python.distChamfer fixtures (tests/golden/make_chamfer_nd_golden.py),
the module surface of the drop-ins and their torch extensions, and what the
shipped library's device code contains."""
import importlib
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import chamfer_nd_cases as cases  # noqa: E402
import codeobj  # noqa: E402

from chamfer2D.dist_chamfer_2D import chamfer_2DDist, chamfer_2DFunction  # noqa: E402,F401
from chamfer5D.dist_chamfer_5D import chamfer_5DDist, chamfer_5DFunction  # noqa: E402,F401
from chamfer6D.dist_chamfer_6D import chamfer_6DDist, chamfer_6DFunction  # noqa: E402,F401
from pcfm import _lib, cpu_ops  # noqa: E402

HEADER = os.path.join(REPO, "include", "pcfm_chamfer_nd.h")
DIST = {2: chamfer_2DDist, 5: chamfer_5DDist, 6: chamfer_6DDist}
ND = sorted(_lib.ND_SIGNATURES)


# ---- 1. the sibling ABI table ---------------------------------------------------
def test_header_and_binding_agree():
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(pcfm_[a-z0-9_]+)\s*\(", text))) == ND
    assert not set(_lib.ND_SIGNATURES) & set(_lib.SIGNATURES)
    lib = _lib.load()
    for name in ND:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.ND_SIGNATURES[name][1], name  # declared by load()
    assert lib.pcfm_chamfer_nd_abi_version() == 1 == _lib.ND_ABI_VERSION
    # pcfm.h's own version is untouched by the sibling header
    assert lib.pcfm_abi_version() == _lib.ABI_VERSION == 20


# ---- 2. host-side refusals (no GPU is touched) ------------------------------------
def _err(lib):
    return lib.pcfm_last_error().decode()


def test_refusals_on_the_host():
    lib = _lib.load()
    none5 = (None,) * 5

    def fwd(b, n, m, d, ws_bytes=0):
        return lib.pcfm_chamfer_nd_fwd(None, None, b, n, m, d, None, None, None, None, None,
                                       ws_bytes, None)

    def bwd(b, n, m, d):
        return lib.pcfm_chamfer_nd_bwd(None, None, b, n, m, d, None, *none5, None)

    assert fwd(1, 10, 10, 4) == -1 and "unsupported dimension 4" in _err(lib)
    assert bwd(1, 10, 10, 4) == -1 and "unsupported dimension 4" in _err(lib)
    for bad in ((-1, 10, 10), (1, -10, 10), (1, 10, -1)):
        assert fwd(*bad, 6) == -1 and "negative size" in _err(lib)
        assert bwd(*bad, 6) == -1 and "negative size" in _err(lib)
    # a shape with candidate splits needs a workspace
    need = lib.pcfm_chamfer_nd_workspace_bytes(8, 20000, 20000, 6)
    assert need == 8 * 40000 * 8
    assert fwd(8, 20000, 20000, 6, need - 1) == -1 and "workspace" in _err(lib)
    with pytest.raises(_lib.PcfmError, match="workspace"):
        _lib.call("pcfm_chamfer_nd_fwd", None, None, 8, 20000, 20000, 6, None, None, None, None,
                  None, 0, None)
    # b * max(n, m) >= 2^31
    assert fwd(2, 1 << 30, 4, 2, 1 << 40) == -1 and "too large" in _err(lib)
    assert bwd(2, 4, 1 << 30, 2) == -1 and "too large" in _err(lib)
    assert [lib.pcfm_chamfer_nd_supported(d) for d in range(-1, 9)] == \
        [0, 0, 0, 1, 1, 0, 1, 1, 0, 0]
    q = lib.pcfm_chamfer_nd_workspace_bytes
    assert q(0, 20000, 20000, 6) == 0 and q(-1, 20000, 20000, 6) == 0
    assert q(8, -1, 20000, 6) == 0 and q(8, 20000, -1, 6) == 0
    assert q(8, 20000, 20000, 4) == 0 and q(8, 20000, 20000, 0) == 0
    assert q(2, 1 << 30, 4, 2) == 0
    assert q(4, 100, 200, 6) == 0                    # one split: no workspace
    assert q(3, 777, 1025, 5) == 3 * (777 + 1025) * 8
    assert q(1, 100, 0, 2) == 0


# ---- 3. the CPU backend against the reference's fixtures ------------------------
def check_golden(out, g, case):
    """The issue's three bars on (dist1, dist2, idx1, idx2) numpy arrays."""
    d1, d2, i1, i2 = out
    np.testing.assert_array_equal(i1, g[f"{case}_idx1"])
    np.testing.assert_array_equal(i2, g[f"{case}_idx2"])
    # (D + 3) * 2^-24 <= 5.4e-7 of the fp32 chain plus the golden's float cast,
    # rounded up; atol: float64 cancellation of the expanded form at exact hits
    np.testing.assert_allclose(d1, g[f"{case}_dist1"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(d2, g[f"{case}_dist2"], rtol=1e-6, atol=1e-9)
    # the reference's own bar (unit_test.py)
    assert (np.mean((d1 - g[f"{case}_dist1"]) ** 2)
            + np.mean((d2 - g[f"{case}_dist2"]) ** 2)) < 1e-8


@pytest.mark.parametrize("d", cases.DIMS)
@pytest.mark.parametrize("case", list(cases.CASES))
def test_cpu_backend_vs_reference(golden, d, case):
    g = golden(f"chamfer_nd_python_d{d}.npz")
    a, c = cases.inputs(case, d)
    np.testing.assert_array_equal(a, g[f"{case}_xyz1"])   # the seeds reproduce the fixture
    np.testing.assert_array_equal(c, g[f"{case}_xyz2"])
    out = DIST[d]()(torch.from_numpy(a), torch.from_numpy(c))
    assert out[0].dtype == torch.float32 and out[2].dtype == torch.int32
    check_golden([t.numpy() for t in out], g, case)


def test_wrong_last_dimension_is_the_reference_assertion():
    x = torch.zeros(1, 4, 3)
    for d in cases.DIMS:
        with pytest.raises(AssertionError, match="Wrong last dimension"):
            DIST[d]()(x, x)


def test_cpu_backward_formula():
    g = torch.Generator().manual_seed(7)
    a = torch.rand(2, 40, 6, generator=g).requires_grad_(True)
    c = torch.rand(2, 30, 6, generator=g).requires_grad_(True)
    d1, d2, i1, i2 = chamfer_6DDist()(a, c)
    (d1.sum() + 2 * d2.sum()).backward()
    a64, c64 = a.detach().double(), c.detach().double()
    ea, ec = torch.zeros_like(a64), torch.zeros_like(c64)
    for bb in range(2):
        t = 2 * (a64[bb] - c64[bb][i1[bb].long()])
        ea[bb] += t
        ec[bb].index_add_(0, i1[bb].long(), -t)
        t = 4 * (c64[bb] - a64[bb][i2[bb].long()])
        ec[bb] += t
        ea[bb].index_add_(0, i2[bb].long(), -t)
    np.testing.assert_allclose(a.grad.numpy(), ea.numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(c.grad.numpy(), ec.numpy(), rtol=1e-5, atol=1e-6)


# ---- 4. D = 3 is the 3-D backend ------------------------------------------------
@pytest.mark.parametrize("case", list(cases.CASES))
def test_nd_at_d3_is_the_3d_backend(case):
    a, c = (torch.from_numpy(t) for t in cases.inputs(case, 3))
    b, n, m = a.shape[0], a.shape[1], c.shape[1]

    def outs():
        return (torch.empty(b, n), torch.empty(b, m), torch.empty(b, n, dtype=torch.int32),
                torch.empty(b, m, dtype=torch.int32))
    x, y = outs(), outs()
    cpu_ops.chamfer_nd_forward(a, c, *x)
    cpu_ops.chamfer_forward(a, c, *y)
    for p, q in zip(x, y):
        assert torch.equal(p, q)
    # and both are the 3-D formula fma(dz, dz, fma(dx, dx, dy*dy)), first minimum
    for bb in range(b):
        dd = c[bb][None, :, :] - a[bb][:, None, :]
        val, arg = cpu_ops._sqdist(dd[..., 0], dd[..., 1], dd[..., 2]).min(dim=1)
        assert torch.equal(x[0][bb], val) and torch.equal(x[2][bb], arg.int())


# ---- 5. module surface ------------------------------------------------------------
@pytest.mark.parametrize("d", cases.DIMS)
def test_module_surface(d, capfd):
    mod = importlib.import_module(f"chamfer{d}D.dist_chamfer_{d}D")
    for name in (f"chamfer_{d}DFunction", f"chamfer_{d}DDist"):
        assert isinstance(getattr(mod, name), type), name
    from pcfm import ops
    ns = getattr(ops, f"chamfer_{d}D")
    ext = importlib.import_module(f"chamfer{d}D.chamfer_{d}D")   # the torch extension
    assert sorted(n for n in dir(ext) if not n.startswith("_")) == ["backward", "forward"]
    z = torch.zeros(1, 4, d)
    f4, i4 = torch.zeros(1, 4), torch.zeros(1, 4, dtype=torch.int32)
    i5 = torch.zeros(1, 5, dtype=torch.int32)
    # the extension: HIP tensors only, status 0 after printing
    assert ext.forward(z, z, f4, f4.clone(), i4, i4.clone()) == 0
    assert ext.forward(z, z, f4, f4.clone(), i4, i5) == 0
    assert ext.backward(z, z, z.clone(), z.clone(), f4, f4.clone(), i4, i5) == 0
    # the ctypes binding runs CPU tensors, and refuses a wrong shape or dimension
    assert ns.forward(z, z, f4, f4.clone(), i4, i4.clone()) == 1
    assert ns.forward(z, z, f4, f4.clone(), i4, i5) == 0
    z3 = torch.zeros(1, 4, 3)
    assert ns.forward(z3, z3, f4, f4.clone(), i4, i4.clone()) == 0
    assert ns.backward(z, z, z.clone(), z.clone(), f4, f4.clone(), i4, i5) == 0
    assert ns.backward(z, z, z.clone(), torch.zeros(1, 4, d + 1), f4, f4.clone(), i4,
                       i4.clone()) == 0
    assert "error in nnd" in capfd.readouterr().out


def test_fscore_known_answer():
    from fscore import fscore
    d1 = torch.tensor([[0.0, 0.0005, 0.002, 0.5], [1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    d2 = torch.tensor([[0.0001, 0.3], [2.0, 3.0], [0.0, 1.0]])
    f, p1, p2 = fscore(d1, d2)
    assert torch.equal(p1, torch.tensor([0.5, 0.0, 1.0]))
    assert torch.equal(p2, torch.tensor([0.5, 0.0, 0.5]))
    # 2 * .5 * .5 / 1 = .5;  0 / 0 -> 0;  2 * 1 * .5 / 1.5 = 2/3
    torch.testing.assert_close(f, torch.tensor([0.5, 0.0, 2.0 / 3.0]))
    assert f[1] == 0 and not torch.isnan(f).any()
    f, _, _ = fscore(d1, d2, threshold=0.01)
    torch.testing.assert_close(f, torch.tensor([2 * 0.75 * 0.5 / 1.25, 0.0, 2.0 / 3.0]))


# ---- 6. the shipped device code -----------------------------------------------------
def test_shipped_kernels_have_no_scratch(tmp_path):
    assert codeobj.available(), "ROCm LLVM tools absent"
    fwd, grad = {}, {}
    for co in codeobj.extract(_lib.LIB_PATH, str(tmp_path)):
        for name, res in codeobj.kernel_resources(co).items():
            # one brute-force forward and one backward per D in the whole library: the 3-D
            # entries launch the D = 3 instantiations (csrc/chamfer_search.hpp)
            for table, kernel in ((fwd, "nn_kernel"), (grad, "nn_grad_kernel")):
                m = re.search(r"\d%sILi(\d+)E" % kernel, name)
                if m:
                    assert int(m.group(1)) not in table, name
                    table[int(m.group(1))] = res
            # no other brute-force search or gradient kernel beside them
            assert not re.search(r"nn_nd_|\d(nn_kernel|nn_grad_kernel)E", name), name
    assert sorted(fwd) == [2, 3, 5, 6]
    assert sorted(grad) == [2, 3, 5, 6]
    for k, res in list(fwd.items()) + list(grad.items()):
        assert res["scratch"] == 0, (k, res)
        assert res["wg"] == 256, (k, res)


def test_sample_chamfer_l2_keeps_the_cdist_path_on_the_cpu():
    from pcfm.sample import chamfer_l2
    g = torch.Generator().manual_seed(1)
    a, c = torch.rand(2, 50, 6, generator=g), torch.rand(2, 40, 6, generator=g)
    d2 = torch.cdist(a, c, p=2).pow(2)
    want = d2.min(dim=2).values.mean(dim=1) + d2.min(dim=1).values.mean(dim=1)
    assert torch.equal(chamfer_l2(a, c), want)
