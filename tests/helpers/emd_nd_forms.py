"""Subprocess of tests/test_gpu_emd_nd.py::test_fused_pass_matches_unfused: runs
the N-D approxmatch on a fixed set of shapes under the PCFM_EMD_FORM the parent
set and saves the match matrices and the costs to argv[1] (.npz)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

# (d, b, n, m): n >< m, ragged row and column tails, more than one LDS chunk per
# wave (> 64 columns per wave: m or n above 1024), a single row
CASES = [(6, 2, 500, 500), (5, 3, 1000, 333), (2, 2, 77, 300), (6, 1, 70, 2200),
         (5, 1, 2100, 70), (3, 2, 300, 77), (6, 4, 1, 64)]


def main():
    from pcfm import _lib, ops
    _lib.load()
    out = {}
    for k, (d, b, n, m) in enumerate(CASES):
        g = torch.Generator(device="cuda").manual_seed(k)
        a = torch.rand(b, n, d, device="cuda", generator=g)
        c = torch.rand(b, m, d, device="cuda", generator=g)
        match, cost = ops.approxmatch_cost_forward_nd(a, c)
        out[f"match{k}"] = match.cpu().numpy()
        out[f"cost{k}"] = cost.cpu().numpy()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
