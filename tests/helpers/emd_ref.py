"""numpy fp64 reference of approxmatch (csrc/emd.hip; emd_kernel.cu:24-156).

It emulates what the kernels DEFINE, not how they sum:
  * d2 of fp32 points is the fp32 sqdist3 chain (pcfm_common.hpp): the
    differences, dy*dy, fma(dx, dx, .) and fma(dz, dz, .) each rounded to fp32
    (every step formed in fp64 first); d2 of fp64 points is formed in fp64;
  * the exponent argument is float32(float32(d2) * float32(level_j * log2 e)),
    e = float32(exp2(argument)) with exp2 taken in fp64, and level 0 is exactly 1;
  * everything else is fp64: the row and column sums, remain / (1e-9 + sum),
    min(., 1), max(0, .), and match accumulated in level order.
So a kernel's distance from it is the hardware exp2's error plus the round-off
walk of its fp32 (or fp64) sums, and nothing else."""
import numpy as np

LOG2E_F32 = np.float32(1.4426950408889634)
# level_j = -4^j for j = 7 .. -1, then 0 (emd_kernel.cu:44-48)
LEVELS = tuple(-(4.0 ** j) for j in range(7, -2, -1)) + (0.0,)
EPS = float(np.float32(1e-9))  # the kernels' (T)1e-9f

# (b, n, m, dtypes): the smallest shapes that reach each way the GPU kernels can
# go wrong (tests/test_gpu_ops.py::test_emd_vs_fp64_reference, tools/emd_parity.py)
GPU_CASES = (
    (2, 64, 64, ("f32",)),            # exact 64-row tiles
    (3, 100, 37, ("f32", "f64")),     # fewer columns than lanes; 2-3 columns per wave; multiR = 2
    (2, 37, 700, ("f32",)),           # multiL = 18
    (1, 513, 300, ("f32",)),          # the last row block holds one row
    (4, 1, 64, ("f32",)),             # a single row
    (1, 70, 2200, ("f32", "f64")),    # > 128 columns per wave in PH 0/2 (two LDS chunks, the
                                      # prefetch past the end), > 64 in PH 3 (three chunks)
    (1, 2100, 70, ("f32",)),          # the same for PH 1
)
# the shapes of the CPU comparison (tests/test_cpu_ops.py)
CPU_CASES = ((2, 64, 64), (2, 77, 300), (3, 1000, 333), (4, 1, 64), (2, 130, 65))


def clouds(b, n, m, dtype, seed):
    g = np.random.default_rng(seed)
    return g.random((b, n, 3)).astype(dtype), g.random((b, m, 3)).astype(dtype)


def pair_d2(p1, p2):
    """d2[k, l] of one batch element as the kernels form it -> float32 (n, m)."""
    d = p2[None, :, :].astype(np.float64) - p1[:, None, :].astype(np.float64)
    if p1.dtype == np.float32:
        r = lambda v: v.astype(np.float32).astype(np.float64)  # noqa: E731
        dx, dy, dz = r(d[..., 0]), r(d[..., 1]), r(d[..., 2])
        return r(dz * dz + r(dx * dx + r(dy * dy))).astype(np.float32)
    return (d[..., 2] * d[..., 2] + (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1])).astype(np.float32)


def approxmatch(xyz1, xyz2):
    """xyz1 (b, n, 3), xyz2 (b, m, 3), float32 or float64 -> match (b, m, n) float64."""
    b, n, m = xyz1.shape[0], xyz1.shape[1], xyz2.shape[1]
    match = np.zeros((b, n, m))
    if n == 0 or m == 0:
        return match.transpose(0, 2, 1).copy()
    multi_l = 1.0 if n >= m else float(m // n)  # emd_kernel.cu:27-33
    multi_r = float(n // m) if n >= m else 1.0
    for bb in range(b):
        d2 = pair_d2(xyz1[bb], xyz2[bb])
        rem_l, rem_r = np.full(n, multi_l), np.full(m, multi_r)
        for level in LEVELS:
            if level == 0.0:
                e = np.ones((n, m))
            else:
                arg = d2 * np.float32(np.float32(level) * LOG2E_F32)  # float32 product
                e = np.exp2(arg.astype(np.float64)).astype(np.float32).astype(np.float64)
            rat_l = rem_l / (EPS + e @ rem_r)
            sum_r = (rat_l @ e) * rem_r
            rat_r = np.minimum(rem_r / (sum_r + EPS), 1.0) * rem_r
            rem_r = np.maximum(0.0, rem_r - sum_r)
            w = (e * rat_l[:, None]) * rat_r[None, :]
            match[bb] += w
            rem_l = np.maximum(0.0, rem_l - w.sum(axis=1))
    return match.transpose(0, 2, 1).copy()


def rel_err(x, ref):
    """max |x - ref| over the largest reference entry (the cross-form measure)."""
    return float(np.abs(np.asarray(x, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)
