"""CPU: the float64 references of the BatchNorm / GroupNorm passes
(tests/helpers/norm_ref.py) against independently composed torch modules, and the
bounds of tests/test_gpu_norm_ref.py against a float32 emulation of the kernels'
own expression trees and summation orders on the very inputs the GPU test uses.

The emulation must stay inside every bound at every listed shape: a bound a
correct fp32 evaluation cannot meet would be a wrong bound, not a finding.  The
kink construction must leave no ambiguous pre-activation and move at most 1e-3 of
the elements (asserted by make_inputs, called here for every shape and kind).
test_checks_reject_one_line_mutations applies the mutations listed in
tests/test_gpu_norm_ref.py's docstring to the emulation: each must fail the check
named for it."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import norm_ref as R  # noqa: E402

sid = R.shape_id
BN_CASES = [(s, k) for s in R.SHAPES_BN for k in R.KINDS]
PARTS_CASES = [(s, k) for s in R.SHAPES_BN_PARTS for k in R.KINDS]
GN_CASES = [(e, s, k) for e in ("gn_film", "gn_silu", "bnin") for s in R.SHAPES_GN
            for k in R.KINDS]
ids2 = lambda cs: [f"{sid(s)}-{k}" for s, k in cs]  # noqa: E731
nul = lambda name, v: None  # noqa: E731


def test_rounding_counts_stay_below_the_cap():
    seen = set()
    for fam, shapes in (("bn", R.SHAPES_BN + R.SHAPES_SE + [s[:3] for s in R.SHAPES_BN_PARTS]),
                        ("gn", R.SHAPES_GN)):
        for s in shapes:
            for name, k in R.counts(fam, s).items():
                assert k > 0
                if R.ABOVE_CAP.get((fam, s)) == name:
                    assert k > R.K_CAP  # listed because it is above: keep the list honest
                    seen.add((fam, s))
                else:
                    assert k <= R.K_CAP, (fam, s, name, k)
    assert seen == set(R.ABOVE_CAP)


@pytest.mark.parametrize("shape,kind", BN_CASES, ids=ids2(BN_CASES))
def test_bn_reference_matches_torch_batch_norm(shape, kind):
    """The graph of bn_ref against F.batch_norm (training) + the activation in
    float64, gradients by autograd through torch's own batch_norm backward."""
    inp = R.make_inputs("bn", shape, kind)
    ref = R.bn_ref("bn", shape, kind)
    x = inp["x"].double().requires_grad_(True)
    g = inp["gamma"].double().requires_grad_(True)
    bt = inp["beta"].double().requires_grad_(True)
    rm, rv = inp["rm"].double().clone(), inp["rv"].double().clone()
    y = F.batch_norm(x, rm, rv, g, bt, True, R.MOM, inp["eps"])
    z = F.relu(y) if inp["slope"] == 0 else F.leaky_relu(y, inp["slope"])
    dx, dg, db = torch.autograd.grad((inp["dz"].double() * z).sum(), [x, g, bt])
    tol = lambda t: 1e-10 * max(1.0, float(t.abs().max()))  # noqa: E731
    assert (R._flat3(z.detach()) - ref["z"]).abs().max() <= tol(ref["z"])
    assert (R._flat3(dx) - ref["dx"]).abs().max() <= 1e-9 * max(1.0, float(ref["dx_terms"].max()))
    assert (dg - ref["dgamma"]).abs().max() <= tol(ref["dgamma"]) * 10
    assert (db - ref["dbeta"]).abs().max() <= tol(ref["dbeta"]) * 10
    if ref["n"] > 1:
        assert (rm - ref["running_mean"]).abs().max() <= 1e-12 * 50
        assert (rv - ref["running_var"]).abs().max() <= tol(ref["running_var"])
    # the conv bias gradient is analytically 0: the reference's is float64 round-off
    assert ref["dbias_in"].abs().max() <= 1e-9 * float(ref["dx_terms"].sum((0, 2)).max())


@pytest.mark.parametrize("entry,shape,kind", GN_CASES,
                         ids=[f"{e}-{sid(s)}-{k}" for e, s, k in GN_CASES])
def test_gn_reference_matches_independent_composition(entry, shape, kind):
    """out of gn_ref / bnin_ref against nn.GroupNorm(...).double() (and
    nn.BatchNorm1d + ReLU before it for the bnin form), batch element by element."""
    b, c, n, groups = shape
    inp = R.make_inputs(entry, shape, kind)
    ref = R.bnin_ref(shape, kind) if entry == "bnin" else R.gn_ref(entry, shape, kind)
    norm = torch.nn.GroupNorm(groups, c, eps=inp["eps"]).double()
    with torch.no_grad():
        norm.weight.copy_(inp["w"].double())
        norm.bias.copy_(inp["bias"].double())
        if entry == "bnin":
            bn = torch.nn.BatchNorm1d(c, eps=inp["bn_eps"]).double().train()
            bn.weight.copy_(inp["bn_gamma"].double())
            bn.bias.copy_(inp["bn_beta"].double())
            x = torch.relu(bn(inp["y"].double()))
        else:
            x = inp["x"].double()
        outs = []
        for i in range(b):
            gn = norm(x[i:i + 1])[0]
            if entry == "gn_silu":
                outs.append(torch.nn.SiLU()(gn))
            else:
                outs.append(x[i] + (gn * (1 + inp["gamma"][i].double()[:, None])
                                    + inp["beta"][i].double()[:, None]))
        out = torch.stack(outs)
    assert (out - ref["out"]).abs().max() <= 1e-9 * max(1.0, float(ref["out"].abs().max()))


def test_inputs_are_adverse():
    """offset: mean / std reaches the hundreds; first_out: A about 37 (6 sigma)
    where the channel / group is long enough to hold a 6 sigma element."""
    ref = R.bn_ref("bn", (2, 6, 4100), "first_out")
    core = ref["core"]
    assert float((core["mean"].abs() * core["invstd"]).max()) > 30.0
    assert 30.0 < float(core["A"].min()) and float(core["A"].max()) < 45.0
    assert bool((ref["inp"]["gamma"] < 0).any()) and bool((ref["inp"]["gamma"] > 0).any())
    assert 30.0 < float(R.gn_ref("gn_film", (2, 256, 2000, 32), "first_out")["core"]["A"].min())
    a = R.bnin_ref((2, 256, 2000, 32), "first_out")["core"]["A"]
    assert 25.0 < float(a.min()) and float(a.max()) < 50.0
    assert float(R.bn_ref("bn", (2, 6, 4100), "offset")["core"]["A"].max()) < 20.0


@pytest.mark.parametrize("shape,kind", BN_CASES, ids=ids2(BN_CASES))
def test_kink_construction_moves_few(shape, kind):
    inp = R.make_inputs("bn", shape, kind)  # asserts the empty set and the cap
    assert inp["moved"] <= R.MOVED_CAP
    ref = R.bn_ref("bn", shape, kind)
    margin = ref["pre_b"].amax((0, 2), keepdim=True)
    assert bool((ref["core"]["pre"].abs() >= margin).all())


@pytest.mark.parametrize("shape,kind", BN_CASES, ids=ids2(BN_CASES))
def test_bn_emulation_stays_inside_the_gpu_bounds(shape, kind, report):
    inp = R.make_inputs("bn", shape, kind)
    ref = R.bn_ref("bn", shape, kind)
    key = f"norm_ref_cpu_emulation/bn/{sid(shape)}/{kind}/"
    rec = lambda name, v: report(key + name, v)  # noqa: E731
    fwd = R.emulate_bn_forward(inp)
    R.check_bn_stats(fwd, ref, rec)
    R.check_bn_forward(fwd, ref, rec)
    bwd = R.emulate_bn_backward(inp, fwd["mean"], fwd["invstd"])
    R.check_bn_backward(bwd, ref, rec, prefix="bwd_")
    if shape in R.SHAPES_SPLIT:
        fs = R.emulate_bn_forward(inp, split=True)
        R.check_bn_forward({"y": fs["y"], "split": True}, ref, rec, prefix="split_")
        bs = R.emulate_bn_backward(inp, fwd["mean"], fwd["invstd"], split=True)
        R.check_bn_backward(bs, ref, rec, prefix="split_bwd_", split=True)


@pytest.mark.parametrize("shape", R.SHAPES_SE, ids=[sid(s) for s in R.SHAPES_SE])
@pytest.mark.parametrize("kind", R.KINDS)
def test_se_emulation_stays_inside_the_gpu_bounds(shape, kind, report):
    inp = R.make_inputs("bn", shape, kind)
    ref = R.bn_ref("bn", shape, kind)
    key = f"norm_ref_cpu_emulation/se/{sid(shape)}/{kind}/"
    rec = lambda name, v: report(key + name, v)  # noqa: E731
    st = R.emulate_bn_stats(inp["x"], inp["eps"], inp["rm"], inp["rv"])
    se = R.emulate_se(inp, st["mean"], st["invstd"])
    R.check_se_rowstats(se, ref, rec)
    R.check_bn_backward(se, ref, rec, prefix="se_", se=True, split=True)


@pytest.mark.parametrize("shape,kind", PARTS_CASES, ids=ids2(PARTS_CASES))
def test_producer_statistics_emulation_stays_inside_the_gpu_bounds(shape, kind, report):
    b, c, s, gsz = shape
    inp = R.make_inputs("bn_parts", shape, kind)
    ref = R.bn_ref("bn_parts", shape, kind, "parts")
    st = R.emulate_bn_fin_parts(R.synth_group_stats(inp["x"], gsz), b, s, gsz, inp["eps"],
                                inp["rm"], inp["rv"])
    key = f"norm_ref_cpu_emulation/bn_parts/{sid(shape)}/{kind}/"
    rec = lambda name, v: report(key + name, v)  # noqa: E731
    R.check_bn_stats(st, ref, rec)
    ch = R.BnChan(R._chan(st["mean"]), R._chan(st["invstd"]), R._chan(inp["gamma"]),
                  R._chan(inp["beta"]), inp["slope"])
    R.check_bn_forward({"y": ch.z(inp["x"])}, ref, rec)


@pytest.mark.parametrize("shape", R.BWD_PARTS_SHAPES, ids=[sid(s) for s in R.BWD_PARTS_SHAPES])
@pytest.mark.parametrize("P", R.BWD_PARTS_P)
@pytest.mark.parametrize("kind", R.KINDS)
def test_backward_on_given_partials_emulation(shape, P, kind, report):
    ref = R.bn_bwd_parts_ref(shape, kind, P)
    out = R.emulate_bn_backward(ref["inp"], ref["mean32"], ref["invstd32"], parts=ref["part"])
    key = f"norm_ref_cpu_emulation/bn_bwd_parts/{sid(shape)}/P{P}/{kind}/"
    R.check_bn_backward(out, ref, lambda name, v: report(key + name, v))


@pytest.mark.parametrize("entry,shape,kind", GN_CASES,
                         ids=[f"{e}-{sid(s)}-{k}" for e, s, k in GN_CASES])
def test_gn_emulation_stays_inside_the_gpu_bounds(entry, shape, kind, report):
    inp = R.make_inputs(entry, shape, kind)
    assert inp["moved"] <= R.MOVED_CAP
    key = f"norm_ref_cpu_emulation/{entry}/{sid(shape)}/{kind}/"
    rec = lambda name, v: report(key + name, v)  # noqa: E731
    if entry == "bnin":
        ref = R.bnin_ref(shape, kind)
        out = R.emulate_bnin(inp)
        bref = {"mean": ref["bn_mean"], "invstd": ref["bn_invstd"], "mean_b": ref["bn_mean_b"],
                "relis": ref["bn_relis"], "n": 2, "running_mean": ref["running_mean"],
                "running_mean_b": ref["running_mean_b"], "running_var": ref["running_var"],
                "running_var_b": ref["running_var_b"]}
        R.check_bn_stats(out["bn"], bref, rec, prefix="bn_")
        R.check_gn_forward(out, ref, rec)
        R.check_gn_backward(out, ref, rec, dx_key="dz")
        R.check_bnin_chain(out, ref, rec)
    else:
        ref = R.gn_ref(entry, shape, kind)
        out = R.emulate_gn(inp, entry == "gn_silu")
        R.check_gn_forward(out, ref, rec)
        R.check_gn_backward(out, ref, rec)


def test_strip_order_sum_is_a_sum():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 1094, 4, generator=g)
    got = R._strip(x)
    want = x.double().sum((1, 2))
    assert ((got.double() - want).abs() / x.abs().double().sum((1, 2))).max() < 1e-6
    assert torch.equal(R._strip(torch.zeros(2, 0, 4)), torch.zeros(2))
    p = torch.randn(5, 17, generator=g)
    assert torch.allclose(R.sum_parts2(p).double(), p.double().sum(1), atol=1e-5)


def test_checks_reject_one_line_mutations():
    """Each mutation of the list in tests/test_gpu_norm_ref.py's docstring, applied to
    the emulation, fails the check of the output it corrupts."""
    # BatchNorm at (3, 5, 36): b > 1, P = 18 (a sum_parts2 tail of two)
    shape, kind = (3, 5, 36), "first_out"
    inp, ref = R.make_inputs("bn", shape, kind), R.bn_ref("bn", shape, kind)
    good = R.emulate_bn_forward(inp)
    R.check_bn_stats(good, ref, nul)
    # 1. inv_n from s instead of b * s
    with pytest.raises(AssertionError, match="'dx'"):
        R.check_bn_backward(R.emulate_bn_backward(inp, good["mean"], good["invstd"], "inv_n_s"),
                            ref, nul)
    # 2. running_var updated with the biased variance
    with pytest.raises(AssertionError, match="'running_var'"):
        R.check_bn_stats(R.emulate_bn_forward(inp, "biased_running_var"), ref, nul)
    # 3. md * md dropped from stat_of_shifted (the variance around K)
    with pytest.raises(AssertionError, match="'invstd'"):
        R.check_bn_stats(R.emulate_bn_forward(inp, "no_md2"), ref, nul)
    # 4. the last partial left out of sum_parts2's tail: forward statistics and backward
    # sums.  At (17, 3, 8) the tail is the 17th partial, the last row ((3, 5, 36)'s last
    # partial is its empty sixth part of a row: dropping it changes nothing)
    tin, tref = R.make_inputs("bn", (17, 3, 8), "offset"), R.bn_ref("bn", (17, 3, 8), "offset")
    tgood = R.emulate_bn_forward(tin)
    with pytest.raises(AssertionError, match="'invstd'"):
        R.check_bn_stats(R.emulate_bn_forward(tin, "parts_tail"), tref, nul)
    with pytest.raises(AssertionError, match="'dbeta'"):
        R.check_bn_backward(R.emulate_bn_backward(tin, tgood["mean"], tgood["invstd"],
                                                  "parts_tail"), tref, nul)
    # 5. ragged-group count min(gsz, ...) -> gsz in the producer-statistics merge
    ps = (2, 5, 100, 64)
    pin, pref = R.make_inputs("bn_parts", ps, "offset"), R.bn_ref("bn_parts", ps, "offset", "parts")
    stats = R.synth_group_stats(pin["x"], 64)
    R.check_bn_stats(R.emulate_bn_fin_parts(stats, 2, 100, 64, pin["eps"], pin["rm"], pin["rv"]),
                     pref, nul)
    with pytest.raises(AssertionError, match="'mean'"):
        R.check_bn_stats(R.emulate_bn_fin_parts(stats, 2, 100, 64, pin["eps"], pin["rm"],
                                                pin["rv"], "ragged_count"), pref, nul)
    # 6. - xhat * mgx dropped from BnChan::dx
    with pytest.raises(AssertionError, match="'dx'"):
        R.check_bn_backward(R.emulate_bn_backward(inp, good["mean"], good["invstd"], "dx_no_mgx"),
                            ref, nul)
    # 7. GroupNorm k2 divided by N instead of cpg * N (cpg = 2)
    gs = (3, 6, 36, 3)
    gin, gref = R.make_inputs("gn_film", gs, "offset"), R.gn_ref("gn_film", gs, "offset")
    R.check_gn_backward(R.emulate_gn(gin, False), gref, nul)
    with pytest.raises(AssertionError, match="'dx'"):
        R.check_gn_backward(R.emulate_gn(gin, False, "k2_over_n"), gref, nul)
    # 8. dgamma[b, c] without the bias[c] * a2 term
    with pytest.raises(AssertionError, match="'dgamma'"):
        R.check_gn_backward(R.emulate_gn(gin, False, "dgamma_no_bias"), gref, nul)
    # 9. bnpart indexed with b and bx swapped (b = 2, nbx = 2: a permutation of the
    # channel's four partials -- only the per-slot check can see it)
    bs = (2, 8, 1028, 2)
    bin_, bref = R.make_inputs("bnin", bs, "offset"), R.bnin_ref(bs, "offset")
    R.check_bnin_chain(R.emulate_bnin(bin_), bref, nul)
    with pytest.raises(AssertionError, match="'bnpart_slot'"):
        R.check_bnin_chain(R.emulate_bnin(bin_, "bnpart_swap"), bref, nul)
    # 10. SiLU' taken at x before the affine
    sin, sref = R.make_inputs("gn_silu", gs, "offset"), R.gn_ref("gn_silu", gs, "offset")
    R.check_gn_backward(R.emulate_gn(sin, True), sref, nul)
    with pytest.raises(AssertionError, match="'dx'"):
        R.check_gn_backward(R.emulate_gn(sin, True, "dsilu_arg"), sref, nul)


@pytest.mark.parametrize("kind", R.KINDS)
def test_pair16_inputs_of_the_post_wrapper_case(kind):
    """"bnin_q" (test_post_gn_film_residual_wrapper): y is a fixed point of the bf16
    hi / lo pair, the kink set is empty on that grid, and the emulation meets the bounds."""
    shape = R.SHAPES_GN[0]
    inp, ref = R.make_inputs("bnin_q", shape, kind), R.bnin_ref(shape, kind, "bnin_q")
    assert torch.equal(R.pair16(inp["y"]), inp["y"]) and inp["moved"] <= R.MOVED_CAP
    out = R.emulate_bnin(inp)
    R.check_gn_forward(out, ref, nul)
    R.check_gn_backward(out, ref, nul, dx_key="dz")
    R.check_bnin_chain(out, ref, nul)
