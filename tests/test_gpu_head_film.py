"""The FiLM head row kernels (csrc/head_film.hip: pcfm_head_film_fwd / _bwd,
pcfm_head_silu_fwd / _bwd and the two reduce kernels behind the backward), each
output against a float64 torch.autograd reference of the formula in
include/pcfm.h (tests/helpers/head_film_ref.py), through pcfm.ops.

Bounds (e = 2^-24; the counts are derived, rounding by rounding, in the helper's
docstring; none exceeds the 1e-5 / e = 167.8 this project holds its fp32 row
kernels to in test_tgate_matches_torch):

* fp32 row outputs, per row, max |got - ref| <= k e scale_row with scale_row the
  row's largest reference magnitude: u k = 35, mean k = 13 (scale: the row's
  largest |h|, whose sum it is), rstd k = 31, dh k = 89 (scale: the row's
  largest |dy gamma| rstd -- dh is a cancelling difference of those terms),
  head_silu_bwd's dh k = 34.
* bf16 row outputs against the bf16 rounding of the float64 function of the
  kernel's own fp32 result: a within one ulp and at most 0.5 % of the elements
  different at all; dh16 exactly bf16(dh) (a pure rounding).
* column sums, per column, |got - ref| <= k_s e abs_sum: k_s = 150 for dsp1,
  dshift, dgamma, dbeta (72 roundings in the longest summand + 78 in the adds:
  64 serial rows of a wave, the 4-wave combine, the chunk and batch combines),
  k_s = 78 for dbias / dbias_b (summands exact).  abs_sum is the column's sum of
  summand magnitudes from the reference, every cancelling sum inside a summand
  (x - mean, gamma xhat + beta, dh_next + da SiLU'(u)) taken by its terms'
  magnitudes; for dbias / dbias_b the reference is the float64 sum of the
  kernel's own dh16, which isolates the reduction.  test_rows_colsum_matches_sum
  holds a pure column sum to 1e-6 = 17 e of the largest column's scale: that is
  a measured figure for a sum of exact inputs against the worst column, this one
  is a worst-case count, per column, that also carries the summands' own
  roundings (u, SiLU', the products).

Every error / bound is recorded under head_film/<shape>/<output> as
{"first": ..., "later": ...} (one figure per input form; the output layer's pair
under head_film/<shape>/silu_<output>); nothing asserts on the recorded values.
tests/test_head_film_ref_cpu.py shows on the CPU that a correct fp32 evaluation
of the kernel's expressions meets all of this on the same inputs.

One-line mutations of head_film.hip, each of which fails a test here.  Each is
argued below, was seen to fail exactly the named tests in one run on an MI355X
with the library rebuilt from the mutated source, and is applied to the CPU
emulation by test_head_film_ref_cpu.py::test_checks_reject_one_line_mutations:

* drop `- xh*m2` from dh: dh is off by rstd xhat m2, of the order of the dh
  scale itself, in every row -> test_film_backward fails on dh at every shape.
  (Scaling m2 by 0.99 instead fails the same twelve cases and none of the
  whole-trunk tests of test_gpu_head.py.)
* accumulate `d*xc` for d sp1 where the kernel accumulates `d*y`: gamma != 1 and
  beta != 0 make every column differ at O(1) relative -> test_film_backward
  fails on dsp1 at every shape.
* index sp1 with batch 0 (the forward's load): sp1 differs by a spread of 0.4
  per batch element, so u of every row of b > 0 is wrong at O(0.1) ->
  test_film_forward fails on u at every shape with b > 1; the same index in the
  backward's constant load fails test_film_backward (dh, dgamma, dbeta) there.
* start the reduce's tail loop (now ordered_sum4's, in pcfm_common.hpp, shared
  with head.hip and pointwise.hip) at `q + 4`: every reduce group drops its first
  tail partial; group 0's is chunk 0 whenever chunks < 13, so all column sums of
  test_film_backward and test_silu_pair fail from one chunk up, and at 13 and 18
  chunks one to four partials are missing.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import head_film_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(s, f) for s in R.SHAPES for f in (True, False)]
IDS = [f"{R.shape_id(s)}-{'first' if f else 'later'}" for s, f in CASES]


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    return ops


_RECORDED = {}


def _recorder(shape, form):
    """rec(report, name, v): head_film/<shape>/<name> -> {form: error / bound}."""
    def rec(report, name, v):
        key = f"head_film/{R.shape_id(shape)}/{name}"
        _RECORDED.setdefault(key, {})[form] = v
        report(key, dict(_RECORDED[key]))
    return rec


def _dev(t):
    return None if t is None else t.cuda()


def _fwd(ops, inp):
    return ops.head_film_fwd(_dev(inp["h16"]), _dev(inp["uprev"]), _dev(inp["gprev"]),
                             _dev(inp["gamma"]), _dev(inp["beta"]), _dev(inp["sp1"]),
                             _dev(inp["shift"]), inp["n"], R.EPS, hbias=_dev(inp["hbias"]))


@pytest.fixture(scope="module", params=CASES, ids=IDS)
def case(request, ops):
    """One (shape, input form): the kernels' outputs on the CPU next to the
    reference.  First block (h16 + hbias): the backward is handed the forward's u;
    later block (uprev + gprev): u = None and shift, recomputed in the kernel."""
    shape, first = request.param
    inp, ref = R.cached_case(shape, first)
    u, a, mean, rstd = _fwd(ops, inp)
    res = ops.head_film_bwd(_dev(inp["dh_next"]), _dev(inp["da16"]), u if first else None,
                            _dev(inp["h16"]), _dev(inp["uprev"]), _dev(inp["gprev"]), mean, rstd,
                            _dev(inp["gamma"]), _dev(inp["beta"]), _dev(inp["sp1"]), inp["n"],
                            want_dh=True, hbias=_dev(inp["hbias"]),
                            shift=None if first else _dev(inp["shift"]))
    assert len(res) == (8 if first else 7)
    names = ("dh", "dh16", "dsp1", "dshift", "dgamma", "dbeta", "dbias", "dbias_b")
    out = {"u": u, "a": a, "mean": mean, "rstd": rstd}
    out.update(zip(names, res))
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    return inp, ref, out, _recorder(shape, "first" if first else "later")


def test_film_forward(case, report):
    """u, mean, rstd per row against float64; a against bf16(SiLU64(kernel u))."""
    inp, ref, out, rec = case
    rows, w = inp["b"] * inp["n"], inp["w"]
    assert out["u"].shape == (rows, w) and out["u"].dtype == torch.float32
    assert out["a"].shape == (rows, w) and out["a"].dtype == torch.bfloat16
    assert out["mean"].shape == out["rstd"].shape == (rows,)
    R.check_film_forward(out, ref, lambda name, v: rec(report, name, v))


def test_film_backward(case, report):
    """dh per row, dh16 as a pure rounding of dh, and every column sum per column,
    against torch.autograd in float64."""
    inp, ref, out, rec = case
    b, w = inp["b"], inp["w"]
    assert out["dh"].shape == (b * inp["n"], w) and out["dh16"].dtype == torch.bfloat16
    assert out["dsp1"].shape == out["dshift"].shape == (b, w)
    assert out["dgamma"].shape == out["dbeta"].shape == out["dbias"].shape == (w,)
    if inp["first"]:
        assert out["dbias_b"].shape == (b, w)
    R.check_film_backward(out, ref, inp["n"], lambda name, v: rec(report, name, v))


@pytest.mark.parametrize("s", [1, 3, 4, 5, 12, 13, 16, 17, 29, 33])
def test_film_backward_reduce_loop_edges(ops, s):
    """b = 1, w = 256, n = 256 s: s chunks (asserted on the workspace), the chunk
    counts at the loop edges of the ordered reduce (ordered_sum4 in
    csrc/pcfm_common.hpp: four partials loaded at a time while q + 12 < s, then a
    stride-4 tail, in each of 4 groups) between and beyond SHAPES' 1, 2, 13 and
    18.  The first-block form, which returns every sum (dbias_b too), through
    test_film_backward's checks and bounds; two calls return equal bits."""
    from pcfm import _lib
    b, w, n = 1, 256, 256 * s
    assert _lib.query("pcfm_head_bwd_workspace_bytes", b, n, w) == (b * s * 5 + 3 * b) * w * 4
    inp = R.make_inputs(b, n, w, True)
    ref = R.film_ref(inp)
    u, _, mean, rstd = _fwd(ops, inp)

    def bwd():
        res = ops.head_film_bwd(_dev(inp["dh_next"]), _dev(inp["da16"]), u, _dev(inp["h16"]), None,
                                None, mean, rstd, _dev(inp["gamma"]), _dev(inp["beta"]),
                                _dev(inp["sp1"]), n, want_dh=True, hbias=_dev(inp["hbias"]))
        return [t.cpu() for t in res]
    r0, r1 = bwd(), bwd()
    names = ("dh", "dh16", "dsp1", "dshift", "dgamma", "dbeta", "dbias", "dbias_b")
    assert len(r0) == len(names)
    for x0, x1 in zip(r0, r1):
        assert torch.equal(x0, x1)
    R.check_film_backward(dict(zip(names, r0)), ref, n, lambda name, v: None)


@pytest.mark.parametrize("shape", R.SHAPES, ids=[R.shape_id(s) for s in R.SHAPES])
def test_silu_pair(ops, shape, report):
    """The output layer: a = bf16(SiLU(h)) and dh = da SiLU'(h), dh16, dbias."""
    inp = R.make_silu_inputs(*shape)
    ref = R.silu_ref(inp)
    up, gp, n = inp["uprev"].cuda(), inp["gprev"].cuda(), inp["n"]
    a = ops.head_silu_fwd(up, gp, n)
    dh, dh16, dbias = ops.head_silu_bwd(inp["da16"].cuda(), up, gp, n)
    out = {"a": a.cpu(), "dh": dh.cpu(), "dh16": dh16.cpu(), "dbias": dbias.cpu()}
    key = f"head_film/{R.shape_id(shape)}/"
    R.check_silu_pair(out, ref, n, lambda name, v: report(key + name, v))


@pytest.mark.parametrize("shape", [(2, 257, 512), (3, 33, 256)],
                         ids=["2x257x512", "3x33x256"])
@pytest.mark.parametrize("first", [True, False], ids=["first", "later"])
def test_forward_tiling_is_bitwise_neutral(ops, shape, first, monkeypatch):
    """A forward block's row range is only a tiling: 4 and 256 rows per block
    (PCFM_FILM_FWD_ROWS, read on every call) give bit-equal u, a, mean, rstd."""
    inp = R.make_inputs(*shape, first)
    res = []
    for rows in ("4", "256"):
        monkeypatch.setenv("PCFM_FILM_FWD_ROWS", rows)
        res.append([t.cpu() for t in _fwd(ops, inp)])
    for x4, x256 in zip(*res):
        assert torch.equal(x4, x256)
    if first:
        return
    res = []  # the output layer's forward shares the launch
    for rows in ("4", "256"):
        monkeypatch.setenv("PCFM_FILM_FWD_ROWS", rows)
        res.append(ops.head_silu_fwd(_dev(inp["uprev"]), _dev(inp["gprev"]), inp["n"]).cpu())
    assert torch.equal(res[0], res[1])


def test_dh16_without_dh_is_the_same_rounding(ops):
    """want_dh = False skips the fp32 store only: dh16 and the sums do not move."""
    inp = R.make_inputs(2, 257, 512, False)
    u, a, mean, rstd = _fwd(ops, inp)
    args = (_dev(inp["dh_next"]), _dev(inp["da16"]), u, None, _dev(inp["uprev"]),
            _dev(inp["gprev"]), mean, rstd, _dev(inp["gamma"]), _dev(inp["beta"]),
            _dev(inp["sp1"]), inp["n"])
    r0 = [t.cpu() for t in ops.head_film_bwd(*args, want_dh=True)[1:]]
    r1 = ops.head_film_bwd(*args, want_dh=False)
    assert r1[0] is None
    for x0, x1 in zip(r0, r1[1:]):
        assert torch.equal(x0, x1.cpu())
