"""Earth Mover's Distance with a one-to-one match: the assignment the parallel
auction of include/pcfm_emd_auction.h (csrc/emd_auction.hip) finds, whose cost is
within n * eps_rel * (the pair's largest squared distance) of the optimal
bijection's -- the form generation and completion papers report.  Both clouds
have the same number of points; D in {2, 3, 5, 6}, every component with the same
weight.

float32 only.  CPU tensors run the pure-PyTorch backend (pcfm.cpu_ops).  The
assignment is a constant under autograd: the value is recomputed from it in
torch, so the gradient is the gather's and there is no backward kernel.
"""
import torch

from pcfm.ops import emd_auction

__all__ = ["earth_mover_distance_auction"]


def earth_mover_distance_auction(p1, p2, eps_rel=2.0 ** -16, max_rounds=1 << 20):
    """p1, p2 (B, n, D), or (n, D) for one pair -> (B,): the mean over i of
    |p1[i] - p2[a(i)]|^2 under the auction's assignment a.  The gradient is
    2 (p1[i] - p2[a(i)]) / n at p1[i] and its mirror at p2[a(i)].  Raises
    RuntimeError if a pair's auction did not finish within max_rounds rounds."""
    if p1.dim() == 2:
        p1 = p1.unsqueeze(0)
    if p2.dim() == 2:
        p2 = p2.unsqueeze(0)
    with torch.no_grad():
        assignment, _, rounds = emd_auction(p1.detach().contiguous(), p2.detach().contiguous(),
                                            eps_rel=eps_rel, max_rounds=max_rounds)
    unfinished = int((rounds < 0).sum())
    if unfinished:
        raise RuntimeError(f"earth_mover_distance_auction: {unfinished} of {rounds.numel()} "
                           "pairs did not finish their auction")
    matched = torch.gather(p2, 1, assignment.long()[:, :, None].expand(-1, -1, p2.shape[2]))
    return (p1 - matched).square().sum(dim=2).mean(dim=1)
