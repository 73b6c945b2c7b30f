"""Chamfer-5D distance (drop-in for
third_party/ChamferDistancePytorch/chamfer5D/dist_chamfer_5D.py): nearest
neighbours over 5-component points (e.g. xyz plus two attribute channels; callers
scale the extra channels themselves, as with the reference's module).

Shaped as chamfer3D/dist_chamfer_3D.py: `chamfer_5D` is the native module
(forward/backward write caller-allocated tensors and return 1 on success, 0
after printing the error); the autograd Function allocates its outputs on the
device.  By default `chamfer_5D` is the ctypes binding (pcfm.ops.chamfer_5D over
include/pcfm_chamfer_nd.h, which also runs CPU tensors); PCFM_TORCH_BACKEND=1
selects the torch C++ extension `chamfer5D/chamfer_5D*.so`
(csrc/torch_losses.cpp) for HIP tensors, CPU tensors still going to the ctypes
binding's CPU backend.
"""
import os

import torch
from torch import nn
from torch.autograd import Function

from pcfm.ops import chamfer_5D

if os.environ.get("PCFM_TORCH_BACKEND") == "1":
    from chamfer5D import chamfer_5D as _ext  # the torch-extension module
    from pcfm.ops import host_routed
    chamfer_5D = host_routed(_ext, chamfer_5D, ["forward", "backward"])

__all__ = ["chamfer_5D", "chamfer_5DFunction", "chamfer_5DDist"]


def _outputs(xyz1, xyz2):
    b, n, d1 = xyz1.shape
    _, m, d2 = xyz2.shape
    assert d1 == 5 and d2 == 5, \
        "Wrong last dimension for the chamfer distance 's input! Check with .size()"
    dev = xyz1.device
    return (torch.empty(b, n, device=dev), torch.empty(b, m, device=dev),
            torch.empty(b, n, dtype=torch.int32, device=dev),
            torch.empty(b, m, dtype=torch.int32, device=dev))


class chamfer_5DFunction(Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, xyz1, xyz2):
        dist1, dist2, idx1, idx2 = _outputs(xyz1, xyz2)
        if not chamfer_5D.forward(xyz1, xyz2, dist1, dist2, idx1, idx2):
            raise RuntimeError("chamfer_5D.forward failed")
        ctx.save_for_backward(xyz1, xyz2, idx1, idx2)
        ctx.mark_non_differentiable(idx1, idx2)
        return dist1, dist2, idx1, idx2

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, graddist1, graddist2, gradidx1, gradidx2):
        xyz1, xyz2, idx1, idx2 = ctx.saved_tensors
        g1 = torch.zeros_like(xyz1)
        g2 = torch.zeros_like(xyz2)
        ok = chamfer_5D.backward(xyz1, xyz2, g1, g2, graddist1.contiguous(),
                                 graddist2.contiguous(), idx1, idx2)
        if not ok:
            raise RuntimeError("chamfer_5D.backward failed")
        return g1, g2


class chamfer_5DDist(nn.Module):
    def forward(self, input1, input2):
        return chamfer_5DFunction.apply(input1.contiguous(), input2.contiguous())
