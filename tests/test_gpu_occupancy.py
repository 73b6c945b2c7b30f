"""GPU: the occupancy counts (include/pcfm_occupancy.h, csrc/occupancy.hip) -- the
kernel against the float64 reference of tests/helpers/occupancy_ref.py on lattice
clouds (exact: every fp32 operation is exact there and ties are true ties) and
against pcfm.cpu_ops on every cloud (exact as well: one contract, integer counts),
launch independence, the refusals, the memory contract by the row runner of
tests/test_gpu_abi_contract.py, HIP against CPU through pcfm.metrics, and timings
(recorded, not asserted, but for the one condition that the kernel is not slower
than the torch-composed route)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import occupancy_ref as oref  # noqa: E402
from test_gpu_abi_contract import Row, run_row  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
THREADS, BLOCK_CAP = 1024, 256      # csrc/occupancy.hip: points per block and round, the cap


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


# (s, n, d, r)
SHAPES = [
    (1, 1, 3, 28),                          # a single point
    (2, 64, 3, 28),                         # one wave... and two clouds
    (3, 1000, 6, 28),                       # ragged tail, row stride 6
    (2, 1025, 5, 9),                        # row stride 5, a third block with two points
    (300, 200, 3, 3),                       # more clouds than blocks, the smallest grid
    (2, 20000, 6, 28),                      # the C2 cloud
    (1, 4096, 3, 32),                       # the largest LDS instance (128 KiB)
    (1, BLOCK_CAP * THREADS + 1, 3, 9),     # one round more than blocks: block 0 takes a second
    (1, 700, 3, 28),                        # less than one round: one block, 324 idle threads
]
IDS = ["s{}n{}d{}r{}".format(*s) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(points, cpu_ops' counts, the reference's counts or None), computed once per
    (shape, kind) and never written to.  The reference walks every kept node per
    branch-2 point in numpy: it is taken on the lattice clouds, where it is exact."""
    from pcfm import cpu_ops
    s, n, d, r = shape
    pts = oref.cloud(kind, 1000 * SHAPES.index(shape) + oref.KINDS.index(kind), s, n, d)
    pts.setflags(write=False)
    cpu = cpu_ops.occupancy_counts(torch.from_numpy(np.array(pts)), r).numpy()
    ref = oref.reference_counts(pts, r) if kind.startswith("lattice") else None
    for a in (cpu, ref):
        if a is not None:
            a.setflags(write=False)
    return pts, cpu, ref


def _run(ops, pts, r):
    c = ops.occupancy_counts(torch.from_numpy(np.array(pts)).to(DEV), r)
    assert c.is_cuda and c.dtype == torch.int32 and tuple(c.shape) == (r ** 3,)
    c = c.cpu().numpy()
    assert c.sum() == pts.shape[0] * pts.shape[1] and c.min() >= 0
    assert not c[~oref.kept_mask(r).reshape(-1)].any()
    return c


def _diff(got, want):
    bad = np.flatnonzero(got != want)
    return f"{len(bad)} differing nodes, the first {bad[:3]}: {got[bad[:3]]} != {want[bad[:3]]}"


@pytest.mark.parametrize("kind", oref.KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_counts(ops, shape, kind):
    pts, cpu, ref = _case(shape, kind)
    got = _run(ops, pts, shape[3])
    if ref is not None:
        assert np.array_equal(got, ref), _diff(got, ref)
    assert np.array_equal(got, cpu), _diff(got, cpu)


def test_the_host_plan_of_the_shapes():
    """The shapes above take the paths their comments name."""
    from pcfm import _lib
    q = functools.partial(_lib.query, "pcfm_occupancy_workspace_bytes")
    assert q(1, BLOCK_CAP * THREADS + 1, 3, 9) == BLOCK_CAP * 729 * 4 == q(1, BLOCK_CAP * THREADS,
                                                                           3, 9)
    assert q(1, 700, 3, 28) == 28 ** 3 * 4 and q(2, 1025, 5, 9) == 3 * 729 * 4
    assert q(300, 200, 3, 3) == 59 * 27 * 4 and q(2, 20000, 6, 28) == 40 * 28 ** 3 * 4


def test_one_lane_of_a_wave_searches(ops):
    """All points at the centre but one far outside: one point takes branch 2, is
    queued, and one wave walks the nodes for it; the other points keep their node."""
    r = 28
    for d, lane in ((3, 17), (6, 0), (5, 63)):
        pts = np.zeros((1, 64, d), np.float32)
        pts[0, lane, :3] = (3.0, 0.0, 0.0)
        got = _run(ops, pts, r)
        want = np.zeros(r ** 3, np.int32)
        want[(14 * r + 14) * r + 14] = 63          # u = 13.5: half to even
        want[(26 * r + 13) * r + 13] = 1           # four kept nodes at one distance: the lowest
        assert np.array_equal(got, want), _diff(got, want)
        assert np.array_equal(got, oref.reference_counts(pts, r))
    # the same in the second wave of a block's second round, the rest of the round idle
    pts = np.zeros((1, THREADS * BLOCK_CAP + 100, 3), np.float32)
    pts[0, -1] = (0.0, -3.0, 0.0)
    got = _run(ops, pts, r)
    assert got[(14 * r + 14) * r + 14] == pts.shape[1] - 1 and got[(13 * r + 1) * r + 13] == 1


@functools.lru_cache(maxsize=None)
def _outside_lattice_points():
    """4000 lattice points (exact, ties included) that take branch 2 at r = 28."""
    far = oref.lattice_cloud(78, 1, 5 * THREADS, 3, 48)
    far = far[:, ~oref.rint_nodes(oref.grid_coords(far, 28), 28)[1]][:, :4000]
    assert far.shape[1] == 4000
    far.setflags(write=False)
    return far


@pytest.mark.parametrize("rounds", [(64, 0, 0), (65, 0, 0), (1021, 3, 0), (1023, 3, 0),
                                    (1024, 0, 1), (700, 700, 900), (1024, 1024, 1024)],
                         ids=lambda q: "q{}-{}-{}".format(*q))
def test_the_search_queue(ops, rounds):
    """Block 0 takes three rounds (2 * 256 * 1024 + 1024 points, all at the centre but
    the `rounds` points of block 0's three rounds that lie outside the sphere).  The
    queued points end at a wave's last lane and at the next wave's first; reach one
    full pass exactly, in the second round, with nothing and with two left; fill
    the block; carry 376 entries over a pass and wrap the ring of 2048 entries."""
    r = 28
    stride = BLOCK_CAP * THREADS
    pts = np.zeros((1, 2 * stride + THREADS, 3), np.float32)
    far = _outside_lattice_points()
    g = np.random.default_rng(sum(rounds))
    used = 0
    for k, q in enumerate(rounds):
        where = k * stride + np.sort(g.permutation(THREADS)[:q])
        pts[0, where] = far[0, used:used + q]
        used += q
    want = oref.reference_counts(far[:, :used], r)
    want[(14 * r + 14) * r + 14] += pts.shape[1] - used
    got = _run(ops, pts, r)
    assert np.array_equal(got, want), _diff(got, want)


def test_no_point_gives_zeros_and_non_finite_points_are_counted(ops):
    for empty in (torch.zeros(0, 5, 3), torch.zeros(4, 0, 6)):
        c = ops.occupancy_counts(empty.to(DEV), 9)
        assert c.is_cuda and c.shape == (729,) and int(c.abs().sum()) == 0
    pts = np.array(_case((3, 1000, 6, 28), "randn")[0])
    pts[0, 5, 0], pts[1, 7, 1], pts[2, 0, 2], pts[2, 9, 2] = np.nan, np.inf, -np.inf, np.nan
    pts[1, 100, :3] = np.nan
    _run(ops, pts, 28)                     # _run checks the sum and the kept nodes


@pytest.mark.parametrize("shape", [(3, 1000, 6, 28), (2, 1025, 5, 9), (300, 200, 3, 3)],
                         ids=lambda s: "s{}n{}d{}r{}".format(*s))
def test_alone_in_a_larger_set_on_a_side_stream_and_twice(ops, shape):
    s, n, d, r = shape
    a, ca, _ = _case(shape, "randn")
    b = _case(shape, "lattice48")[0]
    got = _run(ops, a, r)
    assert np.array_equal(got, ca)
    # two runs: equal tensors
    assert np.array_equal(_run(ops, a, r), got)
    # inside a larger set: the counts add (another number of blocks, other rounds)
    both = _run(ops, np.concatenate([b, a, b]), r)
    assert np.array_equal(both, got + 2 * _run(ops, b, r))
    # cloud by cloud, and as one long cloud
    assert np.array_equal(sum(_run(ops, a[c:c + 1], r) for c in range(min(s, 3)))
                          + (_run(ops, a[3:], r) if s > 3 else 0), got)
    assert np.array_equal(_run(ops, a.reshape(1, s * n, d), r), got)
    # on a side stream
    t = torch.from_numpy(np.array(a)).to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c2 = ops.occupancy_counts(t, r)
    side.synchronize()
    assert np.array_equal(c2.cpu().numpy(), got)


def test_einval_writes_nothing(ops):
    """d = 2, d = 4, r = 2, r = 33 and a short workspace are refused on the host:
    PCFM_EINVAL, and counts is not touched."""
    from pcfm import _lib
    s, n = 2, 100
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    for d, r, ws_bytes in ((2, 28, ws.numel()), (4, 28, ws.numel()), (3, 2, ws.numel()),
                           (3, 33, ws.numel()), (3, 28, 28 ** 3 * 4 - 1), (6, 9, 0)):
        pts = torch.randn(s, n, d, device=DEV)
        counts = torch.full((max(r, 3) ** 3,), -7, dtype=torch.int32, device=DEV)
        text = (r"occupancy: workspace \d+ < \d+ bytes$" if ws_bytes < ws.numel() else
                f"occupancy: unsupported dimension {d} or resolution {r}$")
        with pytest.raises(_lib.PcfmError, match=r"status -1\): " + text):
            _lib.call("pcfm_occupancy_counts", pts.data_ptr(), s, n, d, r, counts.data_ptr(),
                      ws.data_ptr(), ws_bytes, st)
        torch.cuda.synchronize()
        assert (counts == -7).all(), (d, r, ws_bytes)
    for bad, r in ((torch.randn(s, n, 2, device=DEV), 28), (torch.randn(s, n, 4, device=DEV), 28),
                   (torch.randn(s, n, 3, device=DEV), 2), (torch.randn(s, n, 3, device=DEV), 33)):
        with pytest.raises(RuntimeError):
            ops.occupancy_counts(bad, r)


# ---- the memory contract ------------------------------------------------------------
def occ_row(s, n, d, r):
    def build(seed):
        kind = ("randn", "cube")[seed % 2]
        return {"pts": torch.from_numpy(oref.cloud(kind, 900 + seed, s, n, d)).to(DEV)}

    def call(d_):
        from pcfm import ops
        return [ops.occupancy_counts(d_["pts"], r)]
    return Row(f"occupancy-s{s}n{n}d{d}r{r}", build, call, ["pcfm_occupancy_counts"])


OCC_ROWS = [occ_row(3, 1000, 6, 28), occ_row(2, 1025, 5, 9), occ_row(1, 4096, 3, 32),
            occ_row(1, BLOCK_CAP * THREADS + 1, 3, 3)]


def test_every_launching_occupancy_entry_is_in_a_row():
    from pcfm import _lib
    launching = {n for n in _lib.OCCUPANCY_SIGNATURES
                 if not n.endswith(("_abi_version", "_supported", "_bytes"))}
    assert launching == {"pcfm_occupancy_counts"}
    declared = set()
    for row in OCC_ROWS:
        declared |= set(row.entries)
    assert declared == launching


@pytest.mark.parametrize("row", OCC_ROWS, ids=[r.id for r in OCC_ROWS])
def test_contract(ops, row, report):
    run_row(row, report)


# ---- HIP against CPU end to end -------------------------------------------------------
def test_jsd_hip_equals_cpu(ops):
    from pcfm import metrics
    a = torch.from_numpy(np.array(_case((3, 1000, 6, 28), "randn02")[0]))
    b = torch.from_numpy(np.array(_case((3, 1000, 6, 28), "cube")[0]))[:2, :777].contiguous()
    for res in (28, 9, 32):
        cpu = metrics.jsd(a, b, res)
        hip = metrics.jsd(a.to(DEV), b.to(DEV), res)
        assert hip.is_cuda and hip.dtype == torch.float64 and hip.dim() == 0
        assert 0.0 < float(cpu) < 1.0
        assert torch.equal(hip.cpu().view(torch.int64), cpu.view(torch.int64)), res
        assert torch.equal(metrics.occupancy_counts(a.to(DEV), res).cpu(),
                           metrics.occupancy_counts(a, res))
    small, ref = a[:, :96].contiguous(), b[:, :80].contiguous()
    cpu = metrics.generation_metrics(small, ref, emd=False, jsd=True)
    hip = metrics.generation_metrics(small.to(DEV), ref.to(DEV), emd=False, jsd=True)
    assert sorted(cpu) == sorted(hip) and len(hip) == 7 and hip["jsd"].is_cuda
    assert torch.equal(hip["jsd"].cpu().view(torch.int64), cpu["jsd"].view(torch.int64))
    assert torch.equal(cpu["jsd"], metrics.jsd(small, ref))
    # before the subsample, on the device as on the host
    sub = metrics.generation_metrics(small.to(DEV), ref.to(DEV), emd=False, jsd=True,
                                     n_points=32)
    assert torch.equal(sub["jsd"], hip["jsd"])
    # without the keyword: the dict of before
    base = metrics.generation_metrics(small.to(DEV), ref.to(DEV), emd=False)
    assert sorted(base) == sorted(k for k in hip if k != "jsd")
    for k in base:
        assert torch.equal(base[k], hip[k]), k


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


def _composed_nodes(pts, r):
    """The route torch offers without the kernel, branch 1 only: fma, round, clamp
    and the flat index."""
    half = torch.full((), 0.5 * (r - 1), device=pts.device)
    u = torch.addcmul(half, pts[..., :3], torch.full((), float(r - 1), device=pts.device))
    c = torch.round(u).clamp_(0, r - 1).long()
    return ((c[..., 0] * r + c[..., 1]) * r + c[..., 2]).reshape(-1)


def _composed(pts, r):
    return torch.bincount(_composed_nodes(pts, r), minlength=r ** 3)


def test_timings(ops, report):
    """HIP events, 2 warm-up calls, median of 7 and the spread (max - min over the
    median), D = 6, r = 28.  In-sphere clouds (|p| <= 0.45: rint(u) is within
    0.45 * 27 + sqrt(3) / 2 < 13.5 grid units of the centre, so no point takes
    branch 2), randn clouds (branch 2 nearly everywhere) and randn * 0.2 (a tenth of
    the points, spread over nearly every wave)."""
    d, r = 6, 28
    kept = torch.from_numpy(oref.kept_mask(r).reshape(-1)).to(DEV)
    n_kept = int(kept.sum())
    g = torch.Generator(device=DEV).manual_seed(3)
    rec = {}
    for s, n in ((1000, 2048), (256, 20000)):
        x = torch.randn(s, n, d, device=DEV, generator=g)
        inside = x / x[..., :3].norm(dim=-1, keepdim=True) \
            * (0.45 * torch.rand(s, n, 1, device=DEV, generator=g) ** (1 / 3))
        inside = inside.contiguous()
        # the composed route is valid on these clouds: no point leaves the sphere
        nodes = _composed_nodes(inside, r)
        assert bool(kept[nodes].all())
        del nodes
        read = s * n * d * 4
        ms, spread = _median_ms(lambda: ops.occupancy_counts(inside, r))
        rec[f"inside_s{s}_n{n}"] = {"ms": ms, "spread": spread, "bytes_read": read,
                                    "gb_per_s": read / ms * 1e-6}
        cms, cspread = _median_ms(lambda: _composed(inside, r))
        got, comp = ops.occupancy_counts(inside, r), _composed(inside, r)
        rec[f"composed_inside_s{s}_n{n}"] = {
            "ms": cms, "spread": cspread,
            "nodes_differing_from_kernel": int((got.long() != comp).sum())}
        assert int(got.sum()) == s * n == int(comp.sum())
        ms2, spread2 = _median_ms(lambda: ops.occupancy_counts(x, r))
        searched = int((~kept[_composed_nodes(x, r)]).sum())
        rec[f"randn_s{s}_n{n}"] = {"ms": ms2, "spread": spread2, "branch2_share": searched / (s * n),
                                   "node_evals_per_s": searched * n_kept / (ms2 * 1e-3)}
        # what clouds that only nearly fit the cube look like: a tenth of the points search
        x.mul_(0.2)
        ms3, spread3 = _median_ms(lambda: ops.occupancy_counts(x, r))
        searched = int((~kept[_composed_nodes(x, r)]).sum())
        rec[f"randn02_s{s}_n{n}"] = {"ms": ms3, "spread": spread3,
                                     "branch2_share": searched / (s * n),
                                     "node_evals_per_s": searched * n_kept / (ms3 * 1e-3)}
        del x, inside
    print(rec)
    report("occupancy/timing", rec)
    # the one condition: the kernel is not slower than the route it replaces
    kern, comp = rec["inside_s1000_n2048"]["ms"], rec["composed_inside_s1000_n2048"]["ms"]
    assert kern <= comp, (kern, comp)
