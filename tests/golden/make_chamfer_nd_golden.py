"""Generate tests/golden/chamfer_nd_python_d{2,5,6}.npz from the REFERENCE's own
code: ChamferDistancePytorch/chamfer_python.py `distChamfer` (float64
expanded-form pairwise distances, any point dimension -- what the reference's
unit_test.py asserts its CUDA kernels against).

Run where the reference tree is mounted read-only:

    python tests/golden/make_chamfer_nd_golden.py <reference checkout>

It never runs on the GPU box and nothing under tests/ reads the reference at
test time -- only these .npz files (inputs and the four outputs per case; the
cases and seeds: tests/helpers/chamfer_nd_cases.py).

Index equality needs no exclusions: for every query the maker asserts, in
float64, that the runner-up is more than 1e-5 relative beyond the winner
(bit-identical candidate rows count as one candidate -- among those the lowest
index must win), while the fp32 chain of include/pcfm_chamfer_nd.h is within
(D + 2) * 2^-24 <= 4.8e-7 relative of the exact distance.  It also asserts that
distChamfer's indices are the direct float64 lowest-index argmin (its expanded
form |x|^2 + |y|^2 - 2xy could otherwise reorder a near tie).
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True
os.environ["PYTHONDONTWRITEBYTECODE"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "helpers"))
import chamfer_nd_cases as cases  # noqa: E402

MIN_GAP = 1e-5
SIZE_CAP = 967522  # bytes: train_step_c1.npz, the largest fixture so far


def direct(q: np.ndarray, p: np.ndarray):
    """float64 direct-form nearest neighbour of each q in p (one batch element):
    (lowest-index argmin, smallest relative gap between the winner and the
    nearest candidate whose row is not bit-identical to the winner's)."""
    d = ((q[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)) ** 2).sum(-1)
    arg = d.argmin(axis=1)  # first minimum
    win = d[np.arange(len(q)), arg]
    same = (p[None, :, :] == p[arg][:, None, :]).all(-1)  # (nq, np): duplicates of the winner
    rest = np.where(same, np.inf, d)
    second = rest.min(axis=1)
    assert (second >= win).all()
    gap = (second - win) / second
    return arg, float(gap.min())


def main(ref: str) -> None:
    sys.path.insert(0, os.path.join(ref, "third_party", "ChamferDistancePytorch"))
    import chamfer_python  # reference, pure torch

    for d in cases.DIMS + (3,):
        out, worst = {}, {}
        for name in cases.CASES:
            a, c = cases.inputs(name, d)
            d1, d2, i1, i2 = chamfer_python.distChamfer(torch.from_numpy(a), torch.from_numpy(c))
            gaps = []
            for bb in range(a.shape[0]):
                for q, p, idx in ((a[bb], c[bb], i1[bb]), (c[bb], a[bb], i2[bb])):
                    arg, gap = direct(q, p)
                    assert np.array_equal(arg, idx.numpy()), (d, name, "index is not the argmin")
                    gaps.append(gap)
            worst[name] = min(gaps)
            assert worst[name] > MIN_GAP, (d, name, worst[name])
            out[f"{name}_xyz1"], out[f"{name}_xyz2"] = a, c
            out[f"{name}_dist1"], out[f"{name}_dist2"] = d1.numpy(), d2.numpy()
            out[f"{name}_idx1"], out[f"{name}_idx2"] = i1.numpy(), i2.numpy()
        print(f"d={d}: smallest relative gaps", {k: f"{v:.3g}" for k, v in worst.items()})
        if d == 3:
            continue  # checked only: the tests regenerate the d = 3 inputs from the seeds
        path = os.path.join(HERE, f"chamfer_nd_python_d{d}.npz")
        np.savez(path, **out)
        size = os.path.getsize(path)
        assert size < SIZE_CAP, (path, size)
        print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
