"""A/B timing of the BatchNorm / GroupNorm passes (csrc/norm.hip) at the C2
train-step shapes (dev tool): PCFM_LIB=<variant> python tools/bn_ab.py tag

One process times every call once: warm-up 3, device events around each of 7
calls, the median -> one JSON line {"tag", "ms": {call: median ms}}.  Run it in
fresh processes alternated between two libraries and compare the medians of
the per-process medians ("Measured")."""
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]
from pcfm import ops  # noqa: E402


def med7(fn):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


ms = {}
g = torch.Generator(device="cuda").manual_seed(0)


def randn(*shape):
    return torch.randn(*shape, device="cuda", generator=g)


def bn_operands(c):
    return (torch.rand(c, device="cuda", generator=g) + 0.5, randn(c) * 0.1,
            torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"))


# the contiguous passes (SharedMLP's BatchNorm1d + ReLU)
for b, c, s in ((8, 256, 20000), (8, 128, 20000), (8, 128, 32768), (8, 256, 4096)):
    x, dz = randn(b, c, s), randn(b, c, s)
    gm, bt, rm, rv = bn_operands(c)
    _, mean, invstd = ops.bn_act_forward(x, gm, bt, 1e-5, 0.0, 0.1, rm, rv)
    tag = f"B{b}C{c}S{s}"
    ms[f"bn_fwd {tag}"] = med7(lambda: ops.bn_act_forward(x, gm, bt, 1e-5, 0.0, 0.1, rm, rv))
    ms[f"bn_bwd {tag}"] = med7(lambda: ops.bn_act_backward(dz, x, gm, bt, mean, invstd, 0.0,
                                                           want_dbias_in=True))
    del x, dz

# the voxel passes (PVConv's BatchNorm3d + LeakyReLU): split, SE and row-mean forms
for b, c, r in ((8, 256, 8), (2, 128, 32)):
    x, dz = randn(b, c, r, r, r), randn(b, c, r, r, r)
    gm, bt, rm, rv = bn_operands(c)
    se_s, dmv = torch.rand(b, c, device="cuda", generator=g), randn(b, c) * 1e-3
    _, mean, invstd = ops.bn_act_forward_split(x, gm, bt, 1e-4, 0.1, 0.1, rm, rv)
    rowstats = ops.bn_se_backward_stats(dz, x, mean, invstd, gm, bt, 0.1)
    tag = f"B{b}C{c}R{r}"
    ms[f"bn_fwd_split {tag}"] = med7(
        lambda: ops.bn_act_forward_split(x, gm, bt, 1e-4, 0.1, 0.1, rm, rv))
    ms[f"bn_bwd_split {tag}"] = med7(
        lambda: ops.bn_act_backward_split(dz, x, gm, bt, mean, invstd, 0.1, want_dbias_in=True))
    ms[f"bn_fwd_rowmean {tag}"] = med7(
        lambda: ops.bn_act_forward_rowmean(x, gm, bt, 1e-4, 0.1, 0.1, rm, rv))
    ms[f"bn_se_bwd_stats {tag}"] = med7(
        lambda: ops.bn_se_backward_stats(dz, x, mean, invstd, gm, bt, 0.1))
    ms[f"bn_se_bwd_apply_split {tag}"] = med7(
        lambda: ops.bn_se_backward_apply_split(dz, x, mean, invstd, gm, bt, se_s, dmv, rowstats,
                                               0.1, want_dbias_in=True))
    del x, dz

# GroupNorm: the FiLM residual (plain, over a pre-BatchNorm tensor) and the SiLU head
b, c, n, grp = 8, 256, 20000, 32
x, dout = randn(b, c, n), randn(b, c, n)
w, bias = torch.rand(c, device="cuda", generator=g) + 0.5, randn(c) * 0.1
fg, fb = randn(b, c) * 0.1, randn(b, c) * 0.1
gm, bt, _, _ = bn_operands(c)
bm, biv = ops.bn_forward_stats(x, 1e-5, 0.1, None, None)
tag = f"B{b}C{c}N{n}"
_, mean, rstd = ops.gn_film_res_forward(x, w, bias, fg, fb, grp, 1e-5)
ms[f"gn_film_fwd {tag}"] = med7(lambda: ops.gn_film_res_forward(x, w, bias, fg, fb, grp, 1e-5))
ms[f"gn_film_bwd {tag}"] = med7(
    lambda: ops.gn_film_res_backward(dout, x, w, bias, fg, mean, rstd, grp))
_, mean, rstd = ops.gn_film_res_forward_bnin(x, bm, biv, gm, bt, 0.0, w, bias, fg, fb, grp, 1e-5)
ms[f"gn_film_bnin_fwd {tag}"] = med7(
    lambda: ops.gn_film_res_forward_bnin(x, bm, biv, gm, bt, 0.0, w, bias, fg, fb, grp, 1e-5))
ms[f"gn_film_bnin_bwd {tag}"] = med7(
    lambda: ops.gn_film_res_backward_bnin(dout, x, bm, biv, gm, bt, 0.0, w, bias, fg, mean, rstd,
                                          grp))
_, mean, rstd = ops.gn_silu_forward(x, w, bias, grp, 1e-5)
ms[f"gn_silu_fwd {tag}"] = med7(lambda: ops.gn_silu_forward(x, w, bias, grp, 1e-5))
ms[f"gn_silu_bwd {tag}"] = med7(lambda: ops.gn_silu_backward(dout, x, w, bias, mean, rstd, grp))

print(json.dumps({"tag": sys.argv[1] if len(sys.argv) > 1 else "main", "ms": ms}), flush=True)
