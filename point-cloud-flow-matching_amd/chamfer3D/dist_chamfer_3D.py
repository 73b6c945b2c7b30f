"""Chamfer-3D distance (drop-in for
third_party/ChamferDistancePytorch/chamfer3D/dist_chamfer_3D.py).
Built by pcfm/chamfer_dist.py, which says what each name is; the two noGrad
names, which only this width has in the reference, are the forward without
autograd.
"""
from torch import nn
from torch.autograd import Function

from pcfm.chamfer_dist import make

__all__ = ["chamfer_3D", "chamfer_3DFunction", "chamfer_3DDist", "chamfer_3DFunction_noGrad",
           "chamfer_3DDist_nograd"]

chamfer_3D, _run_forward, chamfer_3DFunction, chamfer_3DDist = make(3)


class chamfer_3DFunction_noGrad(Function):
    @staticmethod
    def forward(ctx, xyz1, xyz2):
        return _run_forward(xyz1, xyz2)


class chamfer_3DDist_nograd(nn.Module):
    def forward(self, input1, input2):
        return chamfer_3DFunction_noGrad.apply(input1.contiguous(), input2.contiguous())
