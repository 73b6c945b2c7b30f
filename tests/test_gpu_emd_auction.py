"""GPU: the assignment EMD by auction (include/pcfm_emd_auction.h,
csrc/emd_auction.hip) -- assignment and rounds bit for bit against the rule in pure
PyTorch (pcfm.cpu_ops.emd_auction; at n = 2048 against its results stored in
tests/golden/emd_auction.npz), the cost within the stated bound of the stored
float64 optimum, the contract (two runs, a side stream, the batch, no assignment,
not finished, empty sizes, the refusals, guarded and stale memory), the metrics on
top, and the timings."""
import functools
import os

import numpy as np
import pytest
import torch

from test_gpu_abi_contract import Row, run_row

pytestmark = pytest.mark.gpu
DEV = "cuda"
HERE = os.path.dirname(os.path.abspath(__file__))
EPS_REL = 2.0 ** -16
CAP = 65536         # max_rounds: the fixture's maker asserts every case needs at most half
FIX = np.load(os.path.join(HERE, "golden", "emd_auction.npz"), allow_pickle=False)
NAMES = [str(s) for s in FIX["names"]]


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def _bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int32) if t.is_floating_point() else t


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def urand(seed, *shape):
    return torch.rand(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _clouds(name):
    return torch.from_numpy(FIX[f"{name}_p1"]), torch.from_numpy(FIX[f"{name}_p2"])


@functools.lru_cache(maxsize=None)
def reference(name):
    """(assignment, rounds) of the rule on the CPU, once per case; the stored ones
    where the fixture has them (n = 2048)."""
    if f"{name}_assignment" in FIX.files:
        return torch.from_numpy(FIX[f"{name}_assignment"]), torch.from_numpy(FIX[f"{name}_rounds"])
    from pcfm import cpu_ops
    assignment, _, rounds = cpu_ops.emd_auction(*_clouds(name), EPS_REL, CAP)
    return assignment, rounds


# ---- 1. against the rule and the optimum ----------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_vs_the_rule_and_the_optimum(ops, name):
    from pcfm import cpu_ops
    p1, p2 = _clouds(name)
    b, n, _ = p1.shape
    assignment, cost, rounds = ops.emd_auction(p1.to(DEV), p2.to(DEV), EPS_REL, CAP)
    assert assignment.dtype == torch.int32 and rounds.dtype == torch.int32
    assert cost.dtype == torch.float32 and cost.shape == (b,)
    want_a, want_r = reference(name)
    print(f"emd_auction {name}: rounds {rounds.tolist()} (the rule: {want_r.tolist()})")
    assert torch.equal(rounds.cpu(), want_r)
    assert torch.equal(assignment.cpu(), want_a)
    c = cpu_ops._pair_sqdist_nd(p1, p2).double().numpy()
    for bb in range(b):
        a = assignment[bb].tolist()
        assert sorted(a) == list(range(n))
        got = float(cost[bb])
        np.testing.assert_allclose(got, c[bb][np.arange(n), a].sum(), rtol=1e-6)
        opt, cmax = float(FIX[f"{name}_opt"][bb]), float(FIX[f"{name}_cmax"][bb])
        print(f"  [{bb}] cost {got:.6g}, optimum {opt:.6g}, gap {got - opt:.3g} of the bound "
              f"{n * EPS_REL * cmax:.3g}")
        assert opt * (1 - 1e-6) <= got <= opt + n * EPS_REL * cmax


# ---- 2. the contract --------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 5, 6])
def test_two_runs_a_side_stream_and_the_batch(ops, d):
    b, n = 3, 130
    a, c = urand(7 + d, b, n, d), urand(17 + d, b, n, d)
    first = ops.emd_auction(a, c)
    assert bool((first[2] > 0).all())
    for x, y in zip(ops.emd_auction(a, c), first):
        assert same(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = ops.emd_auction(a, c)
    side.synchronize()
    for x, y in zip(on_side, first):
        assert same(x, y)
    # one pair alone: the same bits as inside the batch
    alone = ops.emd_auction(a[1:2].contiguous(), c[1:2].contiguous())
    for x, y in zip(alone, first):
        assert same(x, y[1:2].contiguous())
    # without the assignment: the same cost and rounds
    none, cost, rounds = ops.emd_auction(a, c, want_assignment=False)
    assert none is None and same(cost, first[1]) and same(rounds, first[2])


def test_not_finished_at_one_round(ops):
    p1, p2 = _clouds("uniform_2x64x3")
    p1, p2 = p1[:1].to(DEV), p2[:1].to(DEV)
    a, cost, rounds = ops.emd_auction(p1, p2, max_rounds=1)
    assert rounds.tolist() == [-1] and bool((a == -1).all()) and bool(torch.isnan(cost).all())
    none, cost, rounds = ops.emd_auction(p1, p2, max_rounds=1, want_assignment=False)
    assert none is None and rounds.tolist() == [-1] and bool(torch.isnan(cost).all())
    # the cap is exact: the rule's round count finishes, one fewer does not
    need = int(reference("uniform_2x64x3")[1][0])
    a, cost, rounds = ops.emd_auction(p1, p2, max_rounds=need)
    assert rounds.tolist() == [need] and torch.equal(a.cpu(), reference("uniform_2x64x3")[0][:1])
    assert ops.emd_auction(p1, p2, max_rounds=need - 1)[2].tolist() == [-1]
    # a pair that finishes beside one that does not: each is a problem of its own
    q1 = torch.cat([p1, p1]).contiguous()
    q2 = torch.cat([p2, p1]).contiguous()           # the second pair: a cloud against itself
    a, cost, rounds = ops.emd_auction(q1, q2, max_rounds=need - 1)
    assert rounds[0].item() == -1 and rounds[1].item() > 0 and float(cost[1]) == 0.0
    assert torch.equal(a[1].cpu(), torch.arange(64, dtype=torch.int32))


@pytest.mark.parametrize("d", [2, 6])
def test_empty_and_degenerate_inputs(ops, d):
    a, cost, rounds = ops.emd_auction(torch.zeros(2, 0, d, device=DEV),
                                      torch.zeros(2, 0, d, device=DEV))
    assert a.shape == (2, 0) and cost.tolist() == [0.0, 0.0] and rounds.tolist() == [0, 0]
    a, cost, rounds = ops.emd_auction(torch.zeros(0, 5, d, device=DEV),
                                      torch.zeros(0, 5, d, device=DEV))
    assert a.shape == (0, 5) and cost.shape == (0,) and rounds.shape == (0,)
    # cmax == 0: the identity, cost 0, rounds 0
    one = urand(3, 1, 1, d).expand(2, 70, d).contiguous()
    a, cost, rounds = ops.emd_auction(one, one.clone())
    assert torch.equal(a.cpu(), torch.arange(70, dtype=torch.int32).expand(2, 70))
    assert cost.tolist() == [0.0, 0.0] and rounds.tolist() == [0, 0]


def test_refusals_leave_the_outputs_untouched(ops):
    from pcfm import _lib
    b, n, d = 2, 40, 6
    a, c = urand(10, b, n, d), urand(11, b, n, d)
    ws = torch.zeros(64, dtype=torch.uint8, device=DEV)
    mark = 7.25
    assignment = torch.full((b, n), 77, dtype=torch.int32, device=DEV)
    rounds = torch.full((b,), 77, dtype=torch.int32, device=DEV)
    cost = torch.full((b,), mark, device=DEV)
    p = torch.Tensor.data_ptr
    top = _lib.query("pcfm_emd_auction_max_points", d)

    def call(b_=b, n_=n, d_=d, eps=EPS_REL, cap=CAP, cost_=p(cost), rounds_=p(rounds)):
        _lib.call("pcfm_emd_auction_f32", p(a), p(c), b_, n_, d_, eps, cap, p(assignment), cost_,
                  rounds_, p(ws), ws.numel(), 0)

    for kw, text in (({"d_": 4}, "unsupported dimension"), ({"d_": 7}, "unsupported"),
                     ({"n_": -1}, "negative size"), ({"b_": -1}, "negative size"),
                     ({"n_": top + 1}, "above"), ({"eps": 0.0}, "eps_rel"),
                     ({"eps": 0.75}, "eps_rel"), ({"eps": float("nan")}, "eps_rel"),
                     ({"eps": 2.0 ** -21}, "eps_rel"), ({"cap": 0}, "max_rounds"),
                     ({"cost_": None}, "required"), ({"rounds_": None}, "required")):
        with pytest.raises(_lib.PcfmError, match=text):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((assignment == 77).all()) and bool((rounds == 77).all())
    assert bool((cost == mark).all()) and not ws.any()


def auction_row(b, n, d):
    def build(seed):
        g = torch.Generator(device=DEV).manual_seed(860 + seed)
        return {"a": torch.rand(b, n, d, device=DEV, generator=g),
                "c": torch.rand(b, n, d, device=DEV, generator=g)}

    def call(t):
        from pcfm import ops
        assignment, cost, rounds = ops.emd_auction(t["a"], t["c"])
        _, cost2, rounds2 = ops.emd_auction(t["a"], t["c"], want_assignment=False)
        return [assignment, cost, rounds, cost2, rounds2]
    return Row(f"emd-auction-d{d}-b{b}n{n}", build, call, ["pcfm_emd_auction_f32"])


# ragged tails of the lanes' object scan (77 = 64 + 13, 300 = 4 * 64 + 44, 65 = 64 + 1)
# and of the staging loop (n * d elements over 1024 threads)
AUCTION_ROWS = [auction_row(2, 77, 6), auction_row(2, 300, 5), auction_row(3, 65, 2)]


@pytest.mark.parametrize("row", AUCTION_ROWS, ids=[r.id for r in AUCTION_ROWS])
def test_memory_contract(ops, row, report):
    """Row / run_row of tests/test_gpu_abi_contract.py: plain twice, under the guarded
    allocator (guards intact, no poison left, the plain run's bits), and with the stale
    arenas of a call on other inputs."""
    run_row(row, report)


# ---- 3. the metrics ---------------------------------------------------------------------------
def test_pairwise_emd_auction_and_generation_metrics(ops):
    from pcfm import metrics
    x, y = urand(41, 4, 64, 6) - 0.5, urand(42, 4, 64, 6) - 0.5
    got = metrics.pairwise_emd_auction(x, y)
    assert got.shape == (4, 4) and got.is_cuda
    want = metrics.pairwise_emd_auction(x.cpu(), y.cpu())
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-6)
    # the chunking does not show, down to one pair per call
    pair = 2 * 64 * 6 * 4
    assert same(metrics.pairwise_emd_auction(x, y, max_bytes=5 * pair), got)
    assert same(metrics.pairwise_emd_auction(x, y, max_bytes=pair), got)
    for comp in ("xyz", "all"):
        res = metrics.generation_metrics(x, y, emd_components=comp, emd_match="auction")
        on_cpu = metrics.generation_metrics(x.cpu(), y.cpu(), emd_components=comp,
                                            emd_match="auction")
        base = metrics.generation_metrics(x, y, emd_components=comp)
        assert sorted(res) == sorted(on_cpu) == sorted(base)
        assert all(v.is_cuda and bool(torch.isfinite(v)) for v in res.values())
        for k, v in res.items():
            if k.startswith(("cov", "1nna")):           # the count-based figures: equal
                assert float(v) == float(on_cpu[k]), k
            else:
                np.testing.assert_allclose(float(v), float(on_cpu[k]), rtol=1e-6, err_msg=k)
            if k.endswith("_cd"):
                assert same(v, base[k]), k
    _default = metrics.generation_metrics(x, y)
    for k, v in metrics.generation_metrics(x, y, emd_match="approx").items():
        assert same(v, _default[k]), k


# ---- 4. timings -------------------------------------------------------------------------------
def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _median_ms(fn, warm=1, reps=3):
    for _ in range(warm):
        fn()
    ts = [_ms(fn) for _ in range(reps)]
    return float(np.median(ts)), (max(ts) - min(ts)) / float(np.median(ts))


def test_timings(ops, report):
    """One process, HIP events, 1 warm-up call, median of 3 and the spread (max - min
    over the median): ops.emd_auction at B = 8, n = 2048, D = 3 and 6, uniform clouds,
    and pairwise_emd_auction at S = R = 16, n = 2048 (256 pairs, one block each), each
    beside the approximate EMD (approxmatch_cost_forward_nd / pairwise_emd_nd) at the
    same shape.  No time is a pass mark: only that every one is finite and positive
    and that every pair finished."""
    from pcfm import metrics
    b, n = 8, 2048
    rec = {"shape": {"b": b, "n": n, "pairwise": [16, 16]}, "warmup": 1, "reps": 3,
           "eps_rel": EPS_REL}
    for d in (3, 6):
        a, c = urand(50 + d, b, n, d) - 0.5, urand(60 + d, b, n, d) - 0.5
        rounds = ops.emd_auction(a, c, want_assignment=False)[2]
        assert bool((rounds > 0).all())
        ms, spread = _median_ms(lambda: ops.emd_auction(a, c, want_assignment=False))
        rec[f"auction_d{d}"] = {"ms": ms, "spread": spread, "rounds": rounds.tolist(),
                                "us_per_round": 1e3 * ms / int(rounds.max())}
        ms, spread = _median_ms(lambda: ops.approxmatch_cost_forward_nd(a, c, want_match=False))
        rec[f"approx_d{d}"] = {"ms": ms, "spread": spread}
        x, y = urand(70 + d, 16, n, d) - 0.5, urand(80 + d, 16, n, d) - 0.5
        ms, spread = _median_ms(lambda: metrics.pairwise_emd_auction(x, y))
        rec[f"pairwise_auction_d{d}"] = {"ms": ms, "spread": spread}
        ms, spread = _median_ms(lambda: metrics.pairwise_emd_nd(x, y))
        rec[f"pairwise_approx_d{d}"] = {"ms": ms, "spread": spread}
    print(rec)
    report("emd_auction/timing", rec)
    times = [v["ms"] for v in rec.values() if isinstance(v, dict) and "ms" in v]
    assert len(times) == 8 and all(np.isfinite(t) and t > 0 for t in times), rec
