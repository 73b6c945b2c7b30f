"""CPU: farthest-point sampling (include/pcfm_fps.h, csrc/fps.hip) and the
subsample the generation metrics take with it (pcfm/metrics.py), without a GPU
-- the fourth ABI table, the host-side refusals, the ops wrapper's refusals, the
CPU backend against the float64 reference of tests/helpers/fps_ref.py, the
metrics' new entry points, and the resources of the shipped kernels."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "helpers"))
import codeobj  # noqa: E402
import fps_ref  # noqa: E402

from pcfm import _lib, cpu_ops, metrics, ops  # noqa: E402

HEADER = os.path.join(REPO, "include", "pcfm_fps.h")
FPS = sorted(_lib.FPS_SIGNATURES)


# ---- 1. the fourth ABI table ------------------------------------------------------
def test_header_and_binding_agree():
    text = open(HEADER).read()
    assert sorted(set(re.findall(r"\b(pcfm_[a-z0-9_]+)\s*\(", text))) == FPS
    for other in (_lib.SIGNATURES, _lib.ND_SIGNATURES, _lib.CROSS_SIGNATURES):
        assert not set(_lib.FPS_SIGNATURES) & set(other)
    lib = _lib.load()
    for name in FPS:
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.FPS_SIGNATURES[name][1], name  # declared by load()
        assert fn.restype == _lib.FPS_SIGNATURES[name][0], name
    assert lib.pcfm_fps_abi_version() == 1 == _lib.FPS_ABI_VERSION
    # the three older versions are untouched by the new sibling header
    assert lib.pcfm_abi_version() == _lib.ABI_VERSION == 20
    assert lib.pcfm_chamfer_nd_abi_version() == _lib.ND_ABI_VERSION == 1
    assert lib.pcfm_chamfer_cross_abi_version() == _lib.CROSS_ABI_VERSION == 1


# ---- 2. host-side refusals (no GPU is touched) --------------------------------------
def test_refusals_on_the_host():
    lib = _lib.load()
    q = lib.pcfm_fps_workspace_bytes

    def err():
        return lib.pcfm_last_error().decode()

    def fps(b, n, m, d, ws_bytes=0):
        return lib.pcfm_fps(None, b, n, d, m, None, None, None, None, ws_bytes, None)

    assert [lib.pcfm_fps_supported(d) for d in range(-1, 9)] == [0, 0, 0, 1, 1, 0, 1, 1, 0, 0]
    res = lib.pcfm_fps_resident_points()
    assert res >= 20000
    for bad in ((-1, 10, 4), (2, -10, 4), (2, 10, -4)):
        assert fps(*bad, 3) == -1 and "negative size" in err()
        assert q(*bad, 3) == 0
    for d in (4, 0, 1, 7, -3):
        assert fps(2, 10, 4, d) == -1 and f"unsupported dimension {d}" in err()
        assert q(2, res + 1, 4, d) == 0
    assert fps(2, 0, 4, 3) == -1 and "no point" in err()
    assert q(2, 0, 4, 3) == 0
    # b * n and b * m stay below 2^31
    for big in ((1 << 16, 1 << 15, 1), (1 << 16, 1, 1 << 15)):
        assert fps(*big, 3, 1 << 40) == -1 and "too large" in err()
        assert q(*big, 3) == 0
    # the resident form needs no workspace; the streaming form its running minima,
    # b * n floats
    assert q(300, res, 2048, 6) == 0 and q(1, 1, 1, 2) == 0
    assert q(1, res + 1, 8, 3) == (res + 1) * 4
    assert q(3, 100000, 2048, 6) == 3 * 100000 * 4
    assert q(0, res + 1, 8, 3) == 0 and q(3, res + 1, 0, 3) == 0
    need = 2 * (res + 1) * 4
    assert fps(2, res + 1, 8, 6, need - 1) == -1 and f"workspace {need - 1} < {need}" in err()
    with pytest.raises(_lib.PcfmError, match="workspace"):
        _lib.call("pcfm_fps", None, 2, res + 1, 6, 8, None, None, None, None, 0, None)
    # nothing to do: no launch, no error
    assert fps(0, 10, 4, 3) == 0 and fps(2, 10, 0, 3) == 0 and fps(2, 0, 0, 3) == 0
    assert fps(0, 0, 4, 3) == 0


def test_ops_wrapper_refusals():
    a = torch.zeros(2, 5, 3)
    ok = torch.zeros(2, dtype=torch.int32)
    for bad in (a.double(), torch.zeros(5, 3), torch.zeros(2, 5, 4), torch.zeros(2, 5, 1),
                torch.zeros(5, 2, 3).transpose(0, 1), torch.zeros(2, 0, 3)):
        with pytest.raises(RuntimeError):
            ops.farthest_point_sample(bad, 2)
    for start in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.int32),
                  ok.long(), ok.float(), torch.zeros(4, dtype=torch.int32)[::2]):
        with pytest.raises(RuntimeError):
            ops.farthest_point_sample(a, 2, start)
    with pytest.raises(RuntimeError):
        ops.farthest_point_sample(a, -1)
    if torch.cuda.is_available():          # a start on another device than the points
        with pytest.raises(RuntimeError):
            ops.farthest_point_sample(a, 2, ok.cuda())
    idx, out = ops.farthest_point_sample(a, 2, ok)
    assert idx.dtype == torch.int32 and idx.shape == (2, 2) and out.shape == (2, 2, 3)
    idx, out = ops.farthest_point_sample(a, 2, gather=False)
    assert out is None and idx.shape == (2, 2)
    idx, out = ops.farthest_point_sample(a, 0)
    assert idx.shape == (2, 0) and out.shape == (2, 0, 3)
    idx, out = ops.farthest_point_sample(torch.zeros(0, 5, 6), 3)
    assert idx.shape == (0, 3) and out.shape == (0, 3, 6)
    # the reference-named backend entry point is still outside this build
    with pytest.raises(NotImplementedError):
        ops.backend.furthest_point_sampling(a, 2)


# ---- 3. the CPU backend against the reference ---------------------------------------
def _cpu(points, m, start=None):
    st = None if start is None else torch.tensor(start, dtype=torch.int32)
    idx, out = ops.farthest_point_sample(torch.from_numpy(points), m, st)
    assert idx.dtype == torch.int32 and out.dtype == torch.float32
    idx, out = idx.numpy(), out.numpy()
    b = points.shape[0]
    # out: the rows idx names, bit for bit
    assert np.array_equal(out.view(np.uint32),
                          points[np.arange(b)[:, None], idx].view(np.uint32))
    assert idx.min(initial=0) >= 0 and idx.max(initial=0) < points.shape[1]
    return idx


GRID = [(10, 2, 1000, 37, 6), (3, 2, 1000, 64, 3), (10, 2, 64, 64, 3), (3, 1, 5, 8, 3),
        (10, 2, 300, 16, 2), (3, 2, 300, 40, 5)]


@pytest.mark.parametrize("bits,b,n,m,d", GRID)
def test_cpu_grid_clouds_exact(bits, b, n, m, d):
    pts = fps_ref.grid_cloud(bits * 1000 + n, b, n, d, bits)
    idx = _cpu(pts, m)
    assert np.array_equal(idx, fps_ref.reference(pts, m))
    if bits == 10 and m <= n:
        assert fps_ref.distinct_prefix_ok(pts, idx)
    if m == n:          # a cloud whose positions are all distinct: a permutation
        for c in range(b):
            if len(np.unique(pts[c, :, :min(d, 3)], axis=0)) == n:
                assert sorted(idx[c].tolist()) == list(range(n))


@pytest.mark.parametrize("b,n,m,d", [(2, 1000, 37, 3), (1, 20000, 64, 6), (2, 1025, 200, 2),
                                     (2, 500, 30, 5)])
def test_cpu_random_clouds_property(b, n, m, d):
    pts = fps_ref.random_cloud(n + d, b, n, d)
    idx = _cpu(pts, m)
    ratio = fps_ref.min_ratio(pts, idx)
    print("min ratio", ratio)
    assert ratio >= fps_ref.PROPERTY_BOUND
    # the reference itself satisfies its own property exactly
    assert fps_ref.min_ratio(pts, fps_ref.reference(pts, m)) == 1.0


def test_cpu_start_and_degenerate_clouds():
    n, m = 200, 12
    pts = fps_ref.grid_cloud(77, 4, n, 3, 10)
    for start in ([0, 0, 0, 0], [n - 1] * 4, [-5, n + 7, 3, 1 << 30], [n, -1, n - 1, 0]):
        idx = _cpu(pts, m, start)
        assert idx[:, 0].tolist() == np.clip(start, 0, n - 1).tolist()
        assert np.array_equal(idx, fps_ref.reference(pts, m, start))
    # m > n: every point once, then index 0 for good
    small = fps_ref.grid_cloud(78, 2, 5, 3, 10)
    idx = _cpu(small, 8, [3, 0])
    assert np.array_equal(idx, fps_ref.reference(small, 8, [3, 0]))
    if all(len(np.unique(c, axis=0)) == 5 for c in small):
        assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4] and idx[:, 5:].tolist() == [[0] * 3] * 2
    # all points identical: the start, then index 0
    same = np.repeat(fps_ref.grid_cloud(79, 2, 1, 6, 10), 9, axis=1)
    assert _cpu(same, 4, [5, 0]).tolist() == [[5, 0, 0, 0], [0, 0, 0, 0]]
    # a single point
    assert _cpu(fps_ref.random_cloud(80, 1, 1, 3), 1).tolist() == [[0]]
    # colour does not steer the sampling: the picks of xyz+rgb are those of xyz alone
    six = fps_ref.random_cloud(81, 2, 300, 6)
    assert np.array_equal(_cpu(six, 20), _cpu(np.ascontiguousarray(six[..., :3]), 20))
    # cpu_ops is what ops ran
    i2, o2 = cpu_ops.farthest_point_sample(torch.from_numpy(six), 20)
    assert np.array_equal(i2.numpy(), _cpu(six, 20))


# ---- 4. the metrics' entry points ----------------------------------------------------
def test_subsample_returns_the_rows_idx_names():
    assert "subsample" in metrics.__all__
    pts = torch.from_numpy(fps_ref.random_cloud(90, 3, 400, 6))
    idx, out = ops.farthest_point_sample(pts, 50)
    sub = metrics.subsample(pts, 50)
    assert sub.shape == (3, 50, 6) and sub.dtype == torch.float32 and not sub.requires_grad
    rows = pts[torch.arange(3)[:, None], idx.long()]
    assert torch.equal(sub.view(torch.int32), rows.view(torch.int32))
    assert torch.equal(sub.view(torch.int32), out.view(torch.int32))
    st = torch.tensor([7, 399, 0], dtype=torch.int32)
    sub = metrics.subsample(pts, 50, st)
    assert torch.equal(sub[:, 0], pts[torch.arange(3), st.long()])
    assert torch.equal(metrics.subsample(pts.requires_grad_(), 50, st), sub)
    assert metrics.subsample(pts, 400).shape == (3, 400, 6)
    with pytest.raises(ValueError):
        metrics.subsample(pts, 401)
    with pytest.raises(ValueError):
        metrics.subsample(pts[0], 10)


def _same(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_generation_metrics_n_points():
    g = torch.Generator().manual_seed(6)
    s, r = torch.randn(4, 96, 6, generator=g), torch.randn(3, 80, 6, generator=g)
    m = 24
    got = metrics.generation_metrics(s, r, n_points=m)
    exp = metrics.generation_metrics(metrics.subsample(s, m), metrics.subsample(r, m))
    assert len(got) == 12
    _same(got, exp)
    # EMD now runs on sets whose clouds differ in size; without the keyword it cannot
    with pytest.raises(ValueError):
        metrics.generation_metrics(s, r)
    _same(metrics.generation_metrics(s, r, emd=False, n_points=m),
          metrics.generation_metrics(metrics.subsample(s, m), metrics.subsample(r, m), emd=False))
    with pytest.raises(ValueError):
        metrics.generation_metrics(s, r, n_points=81)


def test_generation_metrics_without_the_keyword_is_unchanged():
    g = torch.Generator().manual_seed(5)
    s, r = torch.randn(4, 32, 6, generator=g), torch.randn(3, 32, 6, generator=g)
    out = metrics.generation_metrics(s, r)
    _same(out, metrics.generation_metrics(s, r, n_points=None))
    exp = {}
    for tag, pw, a, b in (("cd", metrics.pairwise_chamfer, s, r),
                          ("emd", metrics.pairwise_emd, s[..., :3].contiguous(),
                           r[..., :3].contiguous())):
        mxy = pw(a, b)
        exp.update({f"{k}_{tag}": v for k, v in metrics.mmd_cov(mxy).items()})
        nna = metrics.one_nna(pw(a, a), mxy, pw(b, b))
        exp.update({f"1nna_{tag}": nna["acc"], f"1nna_gen_{tag}": nna["acc_gen"],
                    f"1nna_ref_{tag}": nna["acc_ref"]})
    _same(out, exp)


# ---- 5. the shipped device code -------------------------------------------------------
def test_shipped_fps_kernels_have_no_scratch(tmp_path):
    assert codeobj.available(), "ROCm LLVM tools absent"
    resident, stream = {}, {}
    for co in codeobj.extract(_lib.LIB_PATH, str(tmp_path)):
        for name, res in codeobj.kernel_resources(co).items():
            m = re.search(r"fps_resident_kernelILi(\d+)ELi(\d+)E", name)
            if m:
                key = (int(m.group(1)), int(m.group(2)))
                assert key not in resident, name
                resident[key] = res
            m = re.search(r"fps_stream_kernelILi(\d+)E", name)
            if m:
                assert int(m.group(1)) not in stream, name
                stream[int(m.group(1))] = res
    assert sorted(stream) == [2, 3]
    assert sorted({k for k, _ in resident}) == [2, 3]
    per_thread = sorted({p for _, p in resident})
    assert sorted(resident) == [(k, p) for k in (2, 3) for p in per_thread]
    for key, res in list(resident.items()) + list(stream.items()):
        assert res["scratch"] == 0, (key, res)
        assert res["wg"] == 512, (key, res)
    # the largest instance holds every cloud the resident form takes
    assert per_thread[-1] * 512 == _lib.load().pcfm_fps_resident_points()
