"""The Chamfer distance packages chamfer{2,3,5,6}D, once: make(d) gives what
chamfer<d>D/dist_chamfer_<d>D.py exports (drop-ins for
third_party/ChamferDistancePytorch/chamfer<d>D/dist_chamfer_<d>D.py).

`chamfer_<d>D` is the native module (forward/backward write caller-allocated
tensors and return 1 on success, 0 after printing the error, like
chamfer_cuda.cpp:17-32); the autograd Function allocates its outputs directly on
the device instead of the reference's CPU torch.zeros + .to(device) round trip
(dist_chamfer_3D.py:53-63, :77-81).  By default the native module is the ctypes
binding (pcfm.ops.chamfer_<d>D; d = 3 over include/pcfm.h, the others over
include/pcfm_chamfer_nd.h), which also runs CPU tensors; PCFM_TORCH_BACKEND=1,
read when make() runs, selects the torch C++ extension
`chamfer<d>D/chamfer_<d>D*.so` (csrc/torch_losses.cpp) for HIP tensors, CPU
tensors still going to the ctypes binding's CPU backend.
"""
import importlib
import os

import torch
from torch import nn
from torch.autograd import Function

from pcfm import ops


def make(d):
    """(native module, run_forward, autograd Function, nn.Module) over d-component
    points; run_forward(xyz1, xyz2) -> (dist1, dist2, idx1, idx2) without autograd."""
    name = f"chamfer_{d}D"
    native = getattr(ops, name)
    if os.environ.get("PCFM_TORCH_BACKEND") == "1":
        ext = importlib.import_module(f"chamfer{d}D.{name}")  # the torch-extension module
        native = ops.host_routed(ext, native, ["forward", "backward"])

    def run_forward(xyz1, xyz2):
        b, n, d1 = xyz1.shape
        _, m, d2 = xyz2.shape
        assert d1 == d and d2 == d, \
            "Wrong last dimension for the chamfer distance 's input! Check with .size()"
        dev = xyz1.device
        out = (torch.empty(b, n, device=dev), torch.empty(b, m, device=dev),
               torch.empty(b, n, dtype=torch.int32, device=dev),
               torch.empty(b, m, dtype=torch.int32, device=dev))
        if not native.forward(xyz1, xyz2, *out):
            raise RuntimeError(f"{name}.forward failed")
        return out

    class ChamferFunction(Function):
        @staticmethod
        @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
        def forward(ctx, xyz1, xyz2):
            dist1, dist2, idx1, idx2 = run_forward(xyz1, xyz2)
            ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
            ctx.mark_non_differentiable(idx1, idx2)
            return dist1, dist2, idx1, idx2

        @staticmethod
        @torch.amp.custom_bwd(device_type="cuda")
        def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
            xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
            g1 = torch.zeros_like(xyz1)
            g2 = torch.zeros_like(xyz2)
            ok = native.backward(xyz1, xyz2, g1, g2, graddist1.contiguous(),
                                 graddist2.contiguous(), idx1, idx2)
            if not ok:
                raise RuntimeError(f"{name}.backward failed")
            return g1, g2

    class ChamferDist(nn.Module):
        def forward(self, input1, input2):
            return ChamferFunction.apply(input1.contiguous(), input2.contiguous())

    # the classes live where the package module exports them (pickle, repr)
    for cls, suffix in ((ChamferFunction, "Function"), (ChamferDist, "Dist")):
        cls.__name__ = cls.__qualname__ = name + suffix
        cls.__module__ = f"chamfer{d}D.dist_{name}"
    return native, run_forward, ChamferFunction, ChamferDist
