"""Approximate Earth Mover's Distance over D-component points, D in {2, 3, 5, 6}:
PyTorchEMD/emd.py's autograd function over include/pcfm_emd_nd.h
(csrc/emd.hip), so that the EMD can see the colour of an xyz+rgb cloud and
serve as a loss on it.  Every component enters the squared distance with the same
weight; scaling colour against position is the caller's data convention.

float32 only.  CPU tensors run the pure-PyTorch backend (pcfm.cpu_ops).  There is
no torch C++ extension for these entries: PCFM_TORCH_BACKEND does not change
this module.  At D = 3 the values are those of PyTorchEMD.emd, bit for bit.
"""
import torch

from pcfm.ops import approxmatch_cost_forward_nd, matchcost_backward_nd

__all__ = ["EarthMoverDistanceNDFunction", "earth_mover_distance_nd"]


class EarthMoverDistanceNDFunction(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, p1, p2):
        p1 = p1.contiguous()
        p2 = p2.contiguous()
        # approxmatch + matchcost in one native call; match is kept only when a
        # gradient will need it
        need = any(ctx.needs_input_grad)
        match, cost = approxmatch_cost_forward_nd(p1, p2, want_match=need)
        ctx.save_for_backward(p1, p2, match if need else None)
        return cost

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_cost):
        p1, p2, match = ctx.saved_tensors
        g1, g2 = matchcost_backward_nd(grad_cost.contiguous().to(p1.dtype), p1, p2, match)
        return g1, g2


def earth_mover_distance_nd(p1, p2, transpose=False):
    """EMD (approx) per batch element over all D components, divided by the
    number of points of p1.

    p1, p2: (B, N, D) and (B, M, D), or (B, D, N) and (B, D, M) with
    transpose=True; 2-D inputs get a batch dimension.  Returns cost (B,).
    """
    if p1.dim() == 2:
        p1 = p1.unsqueeze(0)
    if p2.dim() == 2:
        p2 = p2.unsqueeze(0)
    if transpose:
        p1 = p1.transpose(1, 2)
        p2 = p2.transpose(1, 2)
    return EarthMoverDistanceNDFunction.apply(p1, p2) / float(p1.shape[1])
