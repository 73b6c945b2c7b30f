"""CPU: the grouping-backward cases of tests/helpers/seg_ldsrow_cases.py reach
what they are for, and pcfm.cpu_ops' grouping backward meets on them the bound
the GPU engines are held to (tests/test_gpu_seg_ldsrow.py)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import seg_ldsrow_cases as cases  # noqa: E402


@pytest.mark.parametrize("name", list(cases.GROUP))
def test_cpu_grouping_backward_within_bound(name):
    from pcfm import cpu_ops
    gy, idx, n = cases.group_inputs(name)
    ref, bound = cases.group_reference(name)
    got = cpu_ops.grouping_backward(torch.from_numpy(gy), torch.from_numpy(idx), n).numpy()
    assert got.shape == ref.shape
    assert (np.abs(got.astype(np.float64) - ref) <= bound).all()


def test_repeat_case_is_crowded():
    """A 16-row tile of more than 256 items (kTV, kItems of csrc/segsum.hpp) whose
    repeated row alone holds more than one piece, and C no multiple of 64."""
    gy, idx, n = cases.group_inputs("repeat")
    assert gy.shape[1] % 64 != 0
    for b in range(idx.shape[0]):
        cnt = np.bincount(idx[b].reshape(-1), minlength=n)
        row = int(cnt.argmax())
        tile = cnt[row // 16 * 16: row // 16 * 16 + 16].sum()
        pieces = -(-tile // 256)
        assert tile > 256 and cnt[row] > tile / pieces, (tile, cnt[row])
