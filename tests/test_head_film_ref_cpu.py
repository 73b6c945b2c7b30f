"""CPU: the float64 reference of the FiLM head row kernels
(tests/helpers/head_film_ref.py) against an independently composed block, and the
bounds of tests/test_gpu_head_film.py against a float32 emulation of the kernel's
own expressions on the very inputs the GPU test uses.

The emulation must stay inside every bound, and keep a factor 4 on the bf16 flip
shares: a bound a correct fp32 implementation cannot meet would be a wrong bound,
not a finding.  Where it does not, the inputs change, never the caps."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import head_film_ref as R  # noqa: E402

CASES = [(s, f) for s in R.SHAPES for f in (True, False)]
IDS = [f"{R.shape_id(s)}-{'first' if f else 'later'}" for s, f in CASES]


def test_rounding_counts_stay_below_the_cap():
    for k in (R.K_MEAN, R.K_RSTD, R.K_U, R.K_DH, R.K_SILU_DH, R.K_S, R.K_S_BIAS):
        assert 0 < k <= R.K_CAP


@pytest.mark.parametrize("shape,first", CASES, ids=IDS)
def test_reference_matches_independent_composition(shape, first):
    """mean, rstd and u against nn.LayerNorm(W).double() -> broadcast FiLM ->
    nn.SiLU, batch element by batch element (checks the helper's per-batch rows)."""
    b, n, w = shape
    inp, ref = R.cached_case(shape, first)
    ln = torch.nn.LayerNorm(w, eps=R.EPS).double()
    with torch.no_grad():
        ln.weight.copy_(inp["gamma"].double())
        ln.bias.copy_(inp["beta"].double())
        if first:
            h = torch.stack([(inp["h16"].float()[i * n:(i + 1) * n] + inp["hbias"][i]).bfloat16()
                             for i in range(b)]).double()
        else:
            h = (inp["uprev"] + inp["gprev"].float()).double().view(b, n, w)
        u = torch.stack([ln(h[i]) * inp["sp1"][i].double() + inp["shift"][i].double()
                         for i in range(b)]).view(b * n, w)
        # the statistics LayerNorm itself used
        _, mean, rstd = torch.native_layer_norm(h.view(b * n, w), (w,), ln.weight, ln.bias, R.EPS)
        a = torch.nn.SiLU()(u)
    assert (ref["mean"] - mean.view(-1)).abs().max().item() <= 1e-12
    assert (ref["rstd"] - rstd.view(-1)).abs().max().item() <= 1e-12
    assert (ref["u"] - u).abs().max().item() <= 1e-12
    assert (torch.nn.functional.silu(ref["u"]) - a).abs().max().item() <= 1e-12


def test_inputs_differ_per_batch_element_and_reach_the_tails():
    inp, ref = R.cached_case((3, 3, 512), True)
    for k in ("sp1", "shift", "hbias"):
        t = inp[k].float()
        assert (t[1] - t[0]).std().item() >= 0.3 and (t[2] - t[1]).std().item() >= 0.3
    sh = inp["shift"].float()
    assert int((sh == 20.0).sum()) == 8 * 3 and int((sh == -20.0).sum()) == 8 * 3
    assert ref["u"].max().item() > 12.0 and ref["u"].min().item() < -12.0


@pytest.mark.parametrize("shape,first", CASES, ids=IDS)
def test_fp32_emulation_stays_inside_the_gpu_bounds(shape, first, report):
    inp, ref = R.cached_case(shape, first)
    out = R.emulate_film_fp32(inp)
    key = f"head_film_cpu_emulation/{R.shape_id(shape)}/{'first' if first else 'later'}/"
    rec = lambda name, v: report(key + name, v)  # noqa: E731
    R.check_film_forward(out, ref, rec, flip_margin=4.0)
    R.check_film_backward(out, ref, shape[1], rec)


@pytest.mark.parametrize("shape", R.SHAPES, ids=[R.shape_id(s) for s in R.SHAPES])
def test_fp32_emulation_of_the_silu_pair_stays_inside_the_gpu_bounds(shape, report):
    inp = R.make_silu_inputs(*shape)
    ref = R.silu_ref(inp)
    assert ref["h"].max().item() > 12.0 and ref["h"].min().item() < -12.0
    key = f"head_film_cpu_emulation/{R.shape_id(shape)}/"
    R.check_silu_pair(R.emulate_silu_fp32(inp), ref, shape[1],
                      lambda name, v: report(key + name, v), flip_margin=4.0)


def test_kernel_order_colsum_is_a_sum():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2 * 1100, 256, generator=g)
    got = R._kernel_colsum(x, 2, 1100)
    want = x.double().view(2, 1100, 256).sum(1)
    assert ((got.double() - want).abs() / x.abs().double().view(2, 1100, 256).sum(1)).max() < 1e-6


def test_checks_reject_one_line_mutations():
    """The four one-line mutations of head_film.hip listed in
    tests/test_gpu_head_film.py's docstring, applied to the emulation's outputs:
    each must fail the check of the output it corrupts."""
    shape = (2, 257, 512)
    b, n, w = shape
    inp, ref = R.cached_case(shape, False)
    good = R.emulate_film_fp32(inp)
    nul = lambda name, v: None  # noqa: E731
    x = R.h_of(inp).float()
    xc = good["rstd"][:, None] * (x - good["mean"][:, None])
    sp = inp["sp1"].float().repeat_interleave(n, 0)
    d = inp["dh_next"] + inp["da16"].float() * R._dsilu32(good["u"])
    dxh = d * sp * inp["gamma"]
    m2 = (dxh * xc).sum(1, keepdim=True) / w
    # 1. drop "- xh*m2"
    bad = dict(good, dh=good["dh"] + good["rstd"][:, None] * xc * m2)
    bad["dh16"] = bad["dh"].bfloat16()
    with pytest.raises(AssertionError, match="'dh'"):
        R.check_film_backward(bad, ref, n, nul)
    # 2. d*xc for d sp1
    with pytest.raises(AssertionError, match="'dsp1'"):
        R.check_film_backward(dict(good, dsp1=R._kernel_colsum(d * xc, b, n)), ref, n, nul)
    # 3. sp1 of batch 0 for every batch element
    inp0 = dict(inp, sp1=inp["sp1"][:1].expand(b, w).contiguous())
    with pytest.raises(AssertionError, match="'u'"):
        R.check_film_forward(R.emulate_film_fp32(inp0), ref, nul)
    # 4. a chunk partial missed by the reduce (here: the second chunk's one row)
    miss = R._kernel_colsum((d * sp).view(b, n, w)[:, :256].reshape(b * 256, w), b, 256)
    with pytest.raises(AssertionError, match="'dbeta'"):
        R.check_film_backward(dict(good, dbeta=R._batch_sum(miss)), ref, n, nul)
