"""What the shared point blocks (csrc/points.hpp, pcfm/chamfer_dist.py) must keep
as it was: one set of point widths behind every N-D entry, and the
chamfer{2,5,6}D packages' names, CPU results and assertion text.  Nothing here is
new behaviour; every test passes on the library from before the blocks were shared.

The refusal of d = 4 with the outputs untouched is already pinned on the GPU for
pcfm_chamfer_nd_fwd (test_gpu_chamfer_nd.py::test_einval_launches_and_writes_nothing),
pcfm_chamfer_cross_fwd (test_gpu_metrics.py, same name), the three pcfm_emd_nd
entries (test_gpu_emd_nd.py::test_refusals_leave_the_outputs_untouched),
pcfm_emd_auction_f32 (test_gpu_emd_auction.py), pcfm_fps and pcfm_occupancy_counts
(test_gpu_fps.py, test_gpu_occupancy.py::test_einval_writes_nothing, whose matches now
include the pcfm_last_error text); pcfm_chamfer_nd_bwd is the one added here."""
import ctypes
import importlib
import os
import pickle

import pytest
import torch

from pcfm import cpu_ops, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("PCFM_LIB") or os.path.join(REPO, "point-cloud-flow-matching_amd", "csrc",
                                                 "libpcfm_hip.so")
ASSERTION = "Wrong last dimension for the chamfer distance 's input! Check with .size()"


def test_one_set_of_point_widths_on_the_host():
    """ctypes alone, no launch: the four predicates and the auction's capacity agree
    for d in -1..8 and equal ops.POINT_DIMS; the occupancy grid keeps its narrower set."""
    lib = ctypes.CDLL(LIB)
    assert ops.POINT_DIMS == (2, 3, 5, 6) and ops.EMD_ND_DIMS == ops.POINT_DIMS
    for d in range(-1, 9):
        want = d in ops.POINT_DIMS
        for name in ("pcfm_chamfer_nd_supported", "pcfm_chamfer_cross_supported",
                     "pcfm_fps_supported", "pcfm_emd_nd_supported"):
            assert bool(getattr(lib, name)(d)) == want, (name, d)
        assert (lib.pcfm_emd_auction_max_points(d) > 0) == want, d
        assert bool(lib.pcfm_occupancy_supported(d, 28)) == (d in (3, 5, 6)), d


@pytest.mark.parametrize("d", (2, 5, 6))
def test_chamfer_packages_keep_names_and_cpu_results(d):
    mod = importlib.import_module(f"chamfer{d}D.dist_chamfer_{d}D")
    names = [f"chamfer_{d}D", f"chamfer_{d}DFunction", f"chamfer_{d}DDist"]
    assert mod.__all__ == names and all(hasattr(mod, n) for n in names)
    for n in names[1:]:   # pickle finds the class where the package exports it
        cls = getattr(mod, n)
        assert (cls.__module__, cls.__qualname__, cls.__name__) == (mod.__name__, n, n)
    assert type(pickle.loads(pickle.dumps(getattr(mod, names[2])()))) is getattr(mod, names[2])
    assert issubclass(getattr(mod, names[1]), torch.autograd.Function)
    assert issubclass(getattr(mod, names[2]), torch.nn.Module)

    g = torch.Generator().manual_seed(40 + d)
    a = torch.randn(2, 5, d, generator=g).requires_grad_(True)
    c = torch.randn(2, 7, d, generator=g).requires_grad_(True)
    gd1, gd2 = torch.randn(2, 5, generator=g), torch.randn(2, 7, generator=g)
    d1, d2, i1, i2 = getattr(mod, names[2])()(a, c)
    ((d1 * gd1).sum() + (d2 * gd2).sum()).backward()

    e = (torch.empty(2, 5), torch.empty(2, 7), torch.empty(2, 5, dtype=torch.int32),
         torch.empty(2, 7, dtype=torch.int32))
    cpu_ops.chamfer_forward(a.detach(), c.detach(), *e)
    for got, exp in zip((d1, d2, i1, i2), e):
        assert got.dtype == exp.dtype and torch.equal(got.detach(), exp)
    g1, g2 = torch.zeros(2, 5, d), torch.zeros(2, 7, d)
    cpu_ops.chamfer_backward(a.detach(), c.detach(), g1, g2, gd1, gd2, e[2], e[3])
    assert torch.equal(a.grad, g1) and torch.equal(c.grad, g2)

    with pytest.raises(AssertionError) as err:
        getattr(mod, names[2])()(torch.zeros(1, 4, d + 1), torch.zeros(1, 4, d + 1))
    assert str(err.value) == ASSERTION
    with pytest.raises(AssertionError) as err:
        getattr(mod, names[2])()(torch.zeros(1, 4, d), torch.zeros(1, 4, 3))
    assert str(err.value) == ASSERTION


@pytest.mark.gpu
def test_chamfer_nd_bwd_refuses_d4_and_writes_nothing():
    from pcfm import _lib
    b, n, m = 2, 300, 200
    a, c = torch.randn(b, n, 4, device="cuda"), torch.randn(b, m, 4, device="cuda")
    gd1, gd2 = torch.randn(b, n, device="cuda"), torch.randn(b, m, device="cuda")
    i1 = torch.zeros(b, n, dtype=torch.int32, device="cuda")
    i2 = torch.zeros(b, m, dtype=torch.int32, device="cuda")
    g1, g2 = torch.full((b, n, 4), 7.0, device="cuda"), torch.full((b, m, 4), 7.0, device="cuda")
    p = torch.Tensor.data_ptr
    with pytest.raises(_lib.PcfmError, match="chamfer_nd_bwd: unsupported dimension 4"):
        _lib.call("pcfm_chamfer_nd_bwd", p(a), p(c), b, n, m, 4, p(gd1), p(gd2), p(i1), p(i2),
                  p(g1), p(g2), None)
    torch.cuda.synchronize()
    assert bool((g1 == 7).all()) and bool((g2 == 7).all())
