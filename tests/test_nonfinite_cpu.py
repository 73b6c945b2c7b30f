"""The non-finite case table (tests/helpers/nonfinite_ref.py) proven on the CPU
before the GPU sees it: every injection of every case has a reference with a finite
and a non-finite element (assertion 3 of the contract, from the float64 reference
alone), the GEMM cases' column-wise classification equals the one from the full
float64 reference, and the float32 module path that runs where the native library
does not (modules.norm_act, modules.se, PointwiseConv1d on CPU tensors) meets
assertions 1 and 2 of the same table."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import nonfinite_ref as R  # noqa: E402

ENTRIES = R.all_entries()
IDS = [e.id for e in ENTRIES]
SMALL = 1 << 20  # elements of the largest operand up to which the module path is run


def _clean_ref(e):
    return None if e.fast_masks is not None else e.ref(e.inputs())


def test_table_covers_the_special_values_and_sites():
    assert set(R.KINDS) == {"+inf", "-inf", "nan", "nan7fffffff"}
    assert R.bits(R.special("nan7fffffff")).item() == 0x7FFFFFFF
    assert R.bits(R.special("nan")).item() == 0x7FC00000
    assert len(set(IDS)) == len(IDS)
    for e in ENTRIES:
        inj = list(e.injections())
        assert (e.opposing is None) == (e.name in R.GATHERS)  # one opposing pair per reduction
        assert len(inj) == 4 * sum(map(len, e.sites.values())) + (e.opposing is not None)
    nch = {(sh[1] + 31) // 32 for sh, (form, _) in R.PW_SHAPES.items() if form == "Stream128"}
    assert nch >= {1, 2, 3, 4, 5, 6, 7}


@pytest.mark.parametrize("e", ENTRIES, ids=IDS)
def test_reference_has_a_finite_and_a_non_finite_element(e):
    inp = e.inputs()
    for t in inp.values():
        assert bool(torch.isfinite(t).all())
    clean = _clean_ref(e)
    small = e.fast_masks is not None and max(t.numel() for t in inp.values()) <= 1 << 16
    conv8 = e.family == "conv3d" and e.shape[3] == 8  # a full float64 conv: +inf cases only
    full_clean = e.ref(inp) if small or conv8 else None
    for label, op, sk in e.injections():
        cls = e.classify(inp, op, sk, clean)
        assert R.nontrivial(cls), f"{e.id}: {label}: trivial affected set"
        if small or (conv8 and sk[0][1] == "+inf"):
            # the column-wise classification against the full reference's
            with R.poked(inp, op, sk):
                rs = e.ref(inp)
            for k, v in rs.items():
                fin = torch.isfinite(v)
                assert torch.equal(cls[k][0], ~fin), (e.id, label, k)
                assert torch.equal(cls[k][1], fin & (v != full_clean[k])), (e.id, label, k)
    for t in inp.values():  # every poke was undone
        assert bool(torch.isfinite(t).all())


# ---------------------------------------------------------------------------
# the module path on CPU tensors
# ---------------------------------------------------------------------------
def _bn_module(inp, shape):
    cls = torch.nn.BatchNorm1d if len(shape) == 3 else torch.nn.BatchNorm3d
    bn = cls(shape[1], eps=R.EPS, momentum=R.MOM).train()
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"])
        bn.bias.copy_(inp["beta"])
        bn.running_mean.copy_(inp["rm"])
        bn.running_var.copy_(inp["rv"])
    return bn


def _run_bn(e, inp):
    from modules.norm_act import bn_act
    bn = _bn_module(inp, e.shape)
    x = inp["x"].clone().requires_grad_(True)
    z = bn_act(x, bn, e.params["slope"])
    if "forward" in e.name:
        return {"y": z.detach(), "running_mean": bn.running_mean.clone(),
                "running_var": bn.running_var.clone()}
    z.backward(inp["dz"])
    return {"dx": x.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad}


def _run_gn(e, inp):
    from modules.norm_act import gn_film_residual, gn_silu
    b, c, n, groups = e.shape
    norm = torch.nn.GroupNorm(groups, c, eps=R.EPS)
    with torch.no_grad():
        norm.weight.copy_(inp["w"])
        norm.bias.copy_(inp["bias"])
    x = inp["x"].clone().requires_grad_(True)
    gamma, beta = inp["gamma"].clone().requires_grad_(True), inp["beta"].clone().requires_grad_(True)
    film = e.name.startswith("gn_film")
    out = gn_film_residual(x, norm, gamma, beta) if film else gn_silu(x, norm)
    if e.name.endswith("forward"):
        return {"out": out.detach()}
    out.backward(inp["dout"])
    res = {"dx": x.grad, "dw": norm.weight.grad, "dbias": norm.bias.grad}
    if film:
        res.update({"dgamma": gamma.grad, "dbeta": beta.grad})
    return res


def _run_se(e, inp):
    from modules.se import SE3d
    b, c, red = e.shape
    se = SE3d(c, red)
    with torch.no_grad():
        se.fc[0].weight.copy_(inp["w1"])
        se.fc[2].weight.copy_(inp["w2"])
    m = inp["m"].clone().requires_grad_(True)
    s = se.fc(m)
    if e.name.endswith("forward"):
        return {"s": s.detach()}
    s.backward(inp["ds"])
    return {"dm": m.grad, "dw1": se.fc[0].weight.grad, "dw2": se.fc[2].weight.grad}


def _run_pw(e, inp):
    from modules.shared_mlp import PointwiseConv1d
    b, cin, cout, n = e.shape
    mod = PointwiseConv1d(cin, cout, 1)
    with torch.no_grad():
        mod.weight.copy_(inp["w"])
        mod.bias.copy_(inp["bias"])
    x = inp["x"].clone().requires_grad_(True)
    y = mod(x)
    if e.name == "pointwise_forward":
        return {"y": y.detach()}
    y.backward(inp["gy"])
    return {"dx": x.grad} if e.name.endswith("data") else {"dw": mod.weight.grad[:, :, 0]}


def _runner(e):
    if e.family == "more":
        return None  # fused forms of the native library only
    if e.name in ("bn_act_forward", "bn_act_backward"):
        return _run_bn
    if e.name.startswith("gn_"):
        return _run_gn
    if e.name.startswith("se_mlp"):
        return _run_se
    if e.name in ("pointwise_forward", "pointwise_backward_data", "pointwise_backward_weight"):
        return _run_pw
    if e.family == "scatter" and not e.name.startswith("se_") and e.name not in R.GPU_ONLY:
        from pcfm import ops  # CPU tensors: pcfm.cpu_ops
        return lambda e, inp: R.run_scatter(ops, e, inp)
    return None  # no float32 path outside the native library (split forms, statistics entries)


def _largest_operand(e):
    if e.family == "pointwise":
        b, cin, cout, n = e.shape
        return b * max(cin, cout) * n
    return 0


# (the two large GEMM shapes run on the GPU only)
CPU_ENTRIES = [e for e in ENTRIES if _runner(e) is not None and _largest_operand(e) <= SMALL]


@pytest.mark.parametrize("e", CPU_ENTRIES, ids=[e.id for e in CPU_ENTRIES])
def test_module_path_meets_the_contract(e):
    inp = e.inputs()
    run = _runner(e)
    # Where the CPU path deliberately differs from the native expectation it is held
    # to its own, explicit one (Entry.cpu_ref): torch's folded BatchNorm affine (NaN at
    # gamma = +-inf) and pcfm.cpu_ops' scatter through the forward's folded indices.
    ref = e.cpu_ref if e.fast_masks is None else None
    clean_ref = None if e.fast_masks is not None else (ref or e.ref)(inp)
    out_c = run(e, inp)
    for label, op, sk in e.injections():
        cls = e.classify(inp, op, sk, clean_ref, ref)
        with R.poked(inp, op, sk):
            out_s = run(e, inp)
        R.check(f"{e.id}: {label}", out_s, out_c, cls)


def test_rows_max_cases_cover_the_issue():
    labels = {lab for lab, _ in R.rows_max_cases()}
    assert {"nan", "two_nans", "inf_beside_nan"} <= labels
    for lab, h in R.rows_max_cases():
        v, i = torch.max(h.float(), dim=1)
        assert h.shape == R.ROWS_MAX_SHAPE and h.dtype == torch.bfloat16
        nf = ~torch.isfinite(v)
        # (a -inf never is a column's maximum: that case pins that nothing is invented)
        assert bool(nf.any()) == (lab != "-inf") and not bool(nf.all()), lab
        if lab == "two_nans":
            assert int(i[0, 2]) == 64  # the lowest index wins
