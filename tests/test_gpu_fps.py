"""GPU: farthest-point sampling (include/pcfm_fps.h, csrc/fps.hip) -- the kernel's
picks against the float64 reference of tests/helpers/fps_ref.py on grid clouds
(exact: every fp32 operation of the chain is exact there, and the tie rule is
exercised constantly), the defining property on random clouds, the start /
out = NULL / stream / batch independence rules, HIP against CPU through
metrics.subsample, the memory contract by the row runner of
tests/test_gpu_abi_contract.py, and timings (recorded, not asserted, but for the
one condition that the kernel is not slower than the torch-composed loop)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import fps_ref  # noqa: E402
from test_gpu_abi_contract import Row, run_row  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def resident():
    from pcfm import _lib
    return _lib.query("pcfm_fps_resident_points")


# (b, n, m, d); "R": pcfm_fps_resident_points(), known once the library is loaded
SHAPES = [
    (1, 1, 1, 3),            # a single point
    (2, 64, 64, 3),          # m = n: a permutation, and exactly one wave
    (3, 1000, 37, 6),        # ragged tail, row stride 6
    (2, 1025, 16, 2),        # k = 2, and one thread owns a second point
    (1, 5, 8, 3),            # m > n
    (300, 200, 10, 5),       # more clouds than CUs
    (2, 20000, 64, 6),       # the C2 cloud, the largest points-per-thread instance
    (1, "R", 8, 3),          # the last resident size
    (1, "R+1", 8, 3),        # the first streaming size
    (2, "R+1", 8, 6),        # the streaming form with two clouds
]
KINDS = ("grid10", "grid3", "random")


def _shape(shape):
    b, n, m, d = shape
    if isinstance(n, str):
        n = resident() + (1 if n.endswith("+1") else 0)
    return b, n, m, d


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(points, reference idx or None), computed once per (shape, kind) and never
    written to."""
    b, n, m, d = _shape(shape)
    seed = 1000 * SHAPES.index(shape) + KINDS.index(kind)
    if kind == "random":
        pts, ref = fps_ref.random_cloud(seed, b, n, d), None
    else:
        pts = fps_ref.grid_cloud(seed, b, n, d, int(kind[4:]))
        ref = fps_ref.reference(pts, m)
        ref.setflags(write=False)
    pts.setflags(write=False)
    return pts, ref


def _run(ops, pts, m, start=None, gather=True):
    t = torch.from_numpy(np.array(pts)).to(DEV)
    st = None if start is None else torch.tensor(start, dtype=torch.int32, device=DEV)
    idx, out = ops.farthest_point_sample(t, m, st, gather=gather)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (pts.shape[0], m)
    idx = idx.cpu().numpy()
    assert idx.min(initial=0) >= 0 and idx.max(initial=0) < pts.shape[1]
    if not gather:
        assert out is None
        return idx, None
    assert out.dtype == torch.float32 and tuple(out.shape) == (pts.shape[0], m, pts.shape[2])
    return idx, out.cpu().numpy()


def _rows(pts, idx):
    return pts[np.arange(pts.shape[0])[:, None], idx]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "b{}n{}m{}d{}".format(*s))
def test_picks(ops, shape, kind):
    b, n, m, d = _shape(shape)
    pts, ref = _case(shape, kind)
    idx, out = _run(ops, pts, m)
    assert (idx[:, 0] == 0).all()
    # out is a bit copy of the rows idx names
    assert np.array_equal(out.view(np.uint32), _rows(pts, idx).view(np.uint32))
    if kind == "random":
        ratio = fps_ref.min_ratio(pts, idx)
        print("min ratio", ratio, "bound", fps_ref.PROPERTY_BOUND)
        assert ratio >= fps_ref.PROPERTY_BOUND
        return
    bad = np.argwhere(idx != ref)
    assert not len(bad), f"first of {len(bad)} differing picks (cloud, round): {bad[0]}"
    assert np.array_equal(out.view(np.uint32), _rows(pts, ref).view(np.uint32))
    if kind == "grid10" and m <= n:
        assert fps_ref.distinct_prefix_ok(pts, idx)


def test_start(ops):
    shape = (3, 1000, 37, 6)
    b, n, m, d = shape
    pts, _ = _case(shape, "grid10")
    for start in ([0, 0, 0], [n - 1] * 3, [-5, n + 7, 1 << 30], [n, -(1 << 31), 17]):
        idx, out = _run(ops, pts, m, start)
        assert idx[:, 0].tolist() == np.clip(start, 0, n - 1).tolist()
        assert np.array_equal(idx, fps_ref.reference(pts, m, start))
        assert np.array_equal(out.view(np.uint32), _rows(pts, idx).view(np.uint32))
    # the streaming form clamps as well
    shape = (2, "R+1", 8, 6)
    pts, _ = _case(shape, "grid10")
    n = pts.shape[1]
    for start in ([n - 1, -3], [n + 100, 5]):
        idx, _ = _run(ops, pts, 8, start)
        assert np.array_equal(idx, fps_ref.reference(pts, 8, start))
    # all points identical: the start, then index 0 for good
    same = np.repeat(fps_ref.grid_cloud(5, 2, 1, 6, 10), 70, axis=1)
    assert _run(ops, same, 4, [5, 0])[0].tolist() == [[5, 0, 0, 0], [0, 0, 0, 0]]


@pytest.mark.parametrize("shape", [(3, 1000, 37, 6), (2, 1025, 16, 2), (2, "R+1", 8, 6)],
                         ids=lambda s: "b{}n{}m{}d{}".format(*s))
def test_without_out_second_stream_and_alone(ops, shape):
    b, n, m, d = _shape(shape)
    pts, ref = _case(shape, "grid3")
    idx, out = _run(ops, pts, m)
    # out = NULL: the same picks
    assert np.array_equal(_run(ops, pts, m, gather=False)[0], idx)
    # a second call, on a side stream: the same bits
    t = torch.from_numpy(np.array(pts)).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        i2, o2 = ops.farthest_point_sample(t, m)
    side.synchronize()
    assert np.array_equal(i2.cpu().numpy(), idx)
    assert np.array_equal(o2.cpu().numpy().view(np.uint32), out.view(np.uint32))
    # a cloud alone (b = 1) as inside its batch; random clouds too (the same
    # arithmetic whatever the batch)
    rnd, _ = _case(shape, "random")
    full = _run(ops, rnd, m)[0]
    for c in range(b):
        assert np.array_equal(_run(ops, pts[c:c + 1], m)[0][0], idx[c])
        assert np.array_equal(_run(ops, rnd[c:c + 1], m)[0][0], full[c])


def test_non_finite_coordinates_keep_the_indices_in_range(ops):
    pts = np.array(_case((3, 1000, 37, 6), "random")[0])
    pts[0, 5, 0], pts[1, 7, 1], pts[2, 0, 2], pts[2, 9, 2] = np.nan, np.inf, -np.inf, np.nan
    idx, _ = _run(ops, pts, 37)           # _run checks the range
    assert idx.shape == (3, 37)


def test_subsample_hip_equals_cpu(ops):
    from pcfm import metrics
    for shape, kind in (((3, 1000, 37, 6), "grid10"), ((3, 1000, 37, 6), "grid3"),
                        ((2, 1025, 16, 2), "grid3")):
        pts = torch.from_numpy(np.array(_case(shape, kind)[0]))
        m = shape[2]
        st = torch.tensor([4, 999, -1][: shape[0]], dtype=torch.int32)
        cpu = metrics.subsample(pts, m, st)
        hip = metrics.subsample(pts.to(DEV), m, st.to(DEV))
        assert hip.is_cuda and tuple(hip.shape) == (shape[0], m, shape[3])
        assert torch.equal(hip.cpu().view(torch.int32), cpu.view(torch.int32))


def test_generation_metrics_n_points_on_the_device(ops):
    from pcfm import metrics
    s = torch.from_numpy(fps_ref.grid_cloud(61, 3, 300, 6, 10)).to(DEV)
    r = torch.from_numpy(fps_ref.grid_cloud(62, 4, 257, 6, 10)).to(DEV)
    got = metrics.generation_metrics(s, r, n_points=64)
    exp = metrics.generation_metrics(metrics.subsample(s, 64), metrics.subsample(r, 64))
    assert sorted(got) == sorted(exp) and len(got) == 12
    for k in got:
        assert got[k].is_cuda and torch.equal(got[k], exp[k]), k


# ---- the memory contract ------------------------------------------------------------
def fps_row(b, n, m, d):
    def build(seed):
        bb, nn, mm, dd = _shape((b, n, m, d))
        pts = fps_ref.random_cloud(900 + seed, bb, nn, dd)
        g = np.random.default_rng(seed)
        return {"pts": torch.from_numpy(pts).to(DEV),
                "start": torch.from_numpy(g.integers(-3, nn + 3, bb).astype(np.int32)).to(DEV)}

    def call(d_):
        from pcfm import ops
        mm = _shape((b, n, m, d))[2]
        i1, o1 = ops.farthest_point_sample(d_["pts"], mm, d_["start"])
        i2, _ = ops.farthest_point_sample(d_["pts"], mm, d_["start"], gather=False)
        i3, o3 = ops.farthest_point_sample(d_["pts"], mm)
        return [i1, o1, i2, i3, o3]
    return Row(f"fps-b{b}n{n}m{m}d{d}", build, call, ["pcfm_fps"])


FPS_ROWS = [fps_row(3, 1000, 37, 6), fps_row(2, 1025, 16, 2), fps_row(2, "R+1", 8, 6)]


def test_every_launching_fps_entry_is_in_a_row():
    from pcfm import _lib
    launching = {n for n in _lib.FPS_SIGNATURES
                 if not n.endswith(("_abi_version", "_supported", "_resident_points", "_bytes"))}
    assert launching == {"pcfm_fps"}
    declared = set()
    for row in FPS_ROWS:
        declared |= set(row.entries)
    assert declared == launching


@pytest.mark.parametrize("row", FPS_ROWS, ids=[r.id for r in FPS_ROWS])
def test_contract(ops, row, report):
    run_row(row, report)


def test_einval_writes_nothing(ops):
    """d = 4 is refused on the host: PCFM_EINVAL, and neither idx nor out is touched."""
    from pcfm import _lib
    b, n, m, d = 2, 100, 7, 4
    pts = torch.randn(b, n, d, device=DEV)
    idx = torch.full((b, m), -7, dtype=torch.int32, device=DEV)
    out = torch.full((b, m, d), 3.5, device=DEV)
    with pytest.raises(_lib.PcfmError, match=r"status -1\): fps: unsupported dimension 4$"):
        _lib.call("pcfm_fps", pts.data_ptr(), b, n, d, m, None, idx.data_ptr(), out.data_ptr(),
                  None, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (idx == -7).all() and (out == 3.5).all()
    with pytest.raises(RuntimeError, match="unsupported point dimension"):
        ops.farthest_point_sample(pts, m)


# ---- timings (recorded, not asserted) ------------------------------------------------
def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median_ms(fn, warm=2, reps=7):
    for _ in range(warm):
        fn()
    ts = [_ms(fn) for _ in range(reps)]
    return float(np.median(ts)), (max(ts) - min(ts)) / float(np.median(ts))


def _composed_loop(pts, m):
    """The route the tree offered before the kernel: per round one broadcast squared
    distance, torch.minimum, argmax and an index (argmax's tie rule is torch's,
    the timing does not depend on it)."""
    b, n, _ = pts.shape
    pos = pts[..., :3]
    rows = torch.arange(b, device=pts.device)
    sel = torch.zeros(b, dtype=torch.long, device=pts.device)
    dmin = torch.full((b, n), float("inf"), device=pts.device)
    idx = torch.empty((b, m), dtype=torch.long, device=pts.device)
    idx[:, 0] = sel
    for j in range(1, m):
        dist = ((pos - pos[rows, sel][:, None, :]) ** 2).sum(-1)
        dmin = torch.minimum(dmin, dist)
        sel = dmin.argmax(dim=1)
        idx[:, j] = sel
    return idx


def test_timings(ops, report):
    """HIP events, 2 warm-up calls, median of 7 for the kernel; one timed run of the
    composed loop (after 3 warm-up rounds), because it is slow."""
    m, d = 2048, 6
    g = torch.Generator(device=DEV).manual_seed(3)
    big = torch.randn(256, 20000, d, device=DEV, generator=g)
    rec = {}
    for b in (256, 64):
        x = big[:b]
        ms, spread = _median_ms(lambda: ops.farthest_point_sample(x, m))
        rec[f"resident_b{b}_n20000_m{m}_d{d}"] = {"ms": ms, "spread": spread,
                                                  "us_per_round": ms * 1e3 / m}
    x = big[:64]
    idx, _ = ops.farthest_point_sample(x, m)
    _composed_loop(x, 4)
    loop_idx = []
    loop_ms = _ms(lambda: loop_idx.append(_composed_loop(x, m)))
    rec["composed_loop_b64_n20000_m2048_d6"] = {"ms": loop_ms, "runs": 1,
                                                "us_per_round": loop_ms * 1e3 / m}
    kern = rec[f"resident_b64_n20000_m{m}_d{d}"]["ms"]
    rec["loop_over_kernel_b64"] = loop_ms / kern
    # both routes are farthest-point samplers of the same clouds: the property holds
    # for the kernel's picks at the timed size (checked on 2 clouds, 256 rounds)
    part = x[:2].cpu().numpy()
    assert fps_ref.min_ratio(part, idx[:2, :256].cpu().numpy()) >= fps_ref.PROPERTY_BOUND
    del big, x
    y = torch.randn(4, 100000, d, device=DEV, generator=g)
    ms, spread = _median_ms(lambda: ops.farthest_point_sample(y, m), warm=1, reps=7)
    rec[f"streaming_b4_n100000_m{m}_d{d}"] = {"ms": ms, "spread": spread,
                                              "us_per_round": ms * 1e3 / m}
    print(rec)
    report("fps/timing", rec)
    # the one condition: the kernel is not slower than the route it replaces
    assert kern <= loop_ms, (kern, loop_ms)
