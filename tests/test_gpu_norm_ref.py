"""The BatchNorm / GroupNorm passes of csrc/norm.hip (+ bn_chan.hpp), every output
of every launching entry against a float64 torch.autograd reference of the
function it computes (tests/helpers/norm_ref.py), through pcfm.ops.  The batch and
group statistics are inside the reference's graph, so BnChan::dx, the k0 / k1 / k2
coefficients of the GroupNorm backward and the bnin form (one graph: y ->
BatchNorm -> ReLU -> GroupNorm-FiLM residual) are checked against a derivative
they share no algebra with.

Bounds (e = 2^-24; every count is derived, rounding by rounding, in the helper's
docstring, and counts(...) returns them per shape; none is fitted to a measured
error, tests/test_norm_ref_cpu.py holds them to K_CAP = 1e-5 / e = 167.8 and shows
that a float32 emulation of the kernels' expression trees and summation orders
meets every one of them on the same inputs):

* statistics: mean against (adds_f + 3) e max |x| of the channel / group; invstd /
  rstd relative against (1.5 adds_f + 5) A var / (var + eps) e + 3 e with
  A = 1 + (K - mean)^2 / var the shifted-moment amplification from the reference
  (K the first element as the kernel sees it; `first_out` inputs put it 6 sigma
  out, A about 37); producer statistics with A_parts in A's place; running_mean /
  running_var: momentum times those + the update's roundings, running_var
  against var n / (n - 1) with n = B S; num_batches_tracked exact.
* element outputs (y / z, dx, GroupNorm out, dx / dz), per channel or per (b, c)
  row: max |got - ref| <= the row's largest bound, the bound a sum of k e scale
  terms with every cancelling sum taken by its terms (|x| + |mean|,
  |xhat gamma| + |beta|, |g| + |mg| + |xhat mgx|, |d| + |d k0| + |k1| + |xhat k2|);
  split operands decoded hi + lo, + 2^-16 |v|.
* sums (dgamma, dbeta, dbias_in, rowmean, the five rowstats rows, GroupNorm dw,
  dbias, dgamma[b, c], dbeta[b, c], bnpart per slot and per channel), per output
  element: |got - ref| <= k_s e abs_sum + the summands' own bounds.
* the activation kink is kept out of it by construction (no reference
  pre-activation within the kernel's own pre-activation bound of 0), never by a
  wider tolerance.

Every error / bound is recorded under norm_ref/<entry>/<shape>/<kind>/<output>;
nothing asserts on the recorded values.  The invstd error with the first element
30 sigma out (A about 900, the weak end of the shifted moments) is recorded under
norm_ref/first_30/<shape>, not asserted.

One-line mutations, each applied to the emulation by
tests/test_norm_ref_cpu.py::test_checks_reject_one_line_mutations, and the test
here that each one fails.  Each was also built into the library, one at a time, and
seen on an MI355X to fail the cases argued below, with the bnin and wrapper cases
that run the same code (in the order of the list: 44, 80, 170, 36, 12, 70, 30, 28, 4
and 14 of the 213 cases of this file):

* inv_n from s instead of b * s (bn_inv_n): mg and mgx are B times too large, dx is
  off by O(|gamma invstd| |mg|) -> 'dx' of bn_act_backward* at every shape with b > 1.
* running_var updated with the biased variance: off by var / n relative 1 / n,
  far above e at n <= 540 -> 'running_var' of every forward entry at the small shapes.
* md * md dropped from stat_of_shifted: the variance is taken around K, too large
  by (K - mean)^2, a factor A -> 'invstd' of every forward entry (`first_out`: 6x),
  'rstd' of every GroupNorm entry (stat_of_shifted is shared) and all that follows.
* the last partial left out of sum_parts2's tail: at (17, 3, 8) the 17th partial is
  the last batch row -> 'mean' / 'invstd' of the forward entries, 'dbeta' / 'dgamma'
  of bn_act_backward there, bn_act_backward_parts at P = 1, 7, 17, and the bnin
  chain at every shape (P = b * nbx is 1, 2, 3 or 4).
* ragged-group count min(gsz, ...) -> gsz in bn_fin_parts_kernel: the last group of
  a row weighs 64 / 36 too much -> 'mean' of bn_forward_stats_parts /
  bn_act_forward_parts at the ragged shapes.
* - xhat * mgx dropped from BnChan::dx: dx is off by |gamma invstd xhat mgx|, O(1)
  of its scale -> 'dx' of every BatchNorm backward entry and 'dy' of the bnin chain.
* GroupNorm k2 divided by N instead of cpg * N: k2 is cpg times too large ->
  'dx' of gn_film_res_backward / gn_silu_backward, 'dz' of the bnin form, cpg > 1.
* dgamma[b, c] without bias[c] * a2: off by |bias a2| -> 'dgamma' of
  gn_film_res_backward and gn_film_res_backward_bnin.
* bnpart indexed with b and bx swapped: a permutation of the channel's partials
  (its sum does not move) -> 'bnpart_slot' at (2, 8, 1028, 2) and
  (2, 256, 2000, 32), where b = nbx = 2.
* SiLU' at x before the affine: the wrong argument, O(1) -> 'dx', 'dw', 'dbias' of
  gn_silu_backward.
"""
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import norm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
sid = R.shape_id

BWD_PARTS = [s + (p,) for s in R.BWD_PARTS_SHAPES for p in R.BWD_PARTS_P]
# entry (the pcfm.ops function, with its variant) -> (extern "C" entries it drives, shapes)
ENTRIES = {
    "bn_act_forward": (["pcfm_bn_act_fwd"], R.SHAPES_BN),
    "bn_forward_stats": (["pcfm_bn_fwd_stats"], R.SHAPES_BN),
    "bn_forward_stats_parts": (["pcfm_bn_fwd_stats"], R.SHAPES_BN_PARTS),
    "bn_act_forward_parts": (["pcfm_bn_act_fwd_parts"], R.SHAPES_BN_PARTS),
    "bn_act_forward_split": (["pcfm_bn_act_fwd_split"], R.SHAPES_SPLIT),
    "bn_act_forward_rowmean": (["pcfm_bn_act_fwd_rowmean"], R.SHAPES_BN),
    "bn_act_backward": (["pcfm_bn_act_bwd"], R.SHAPES_BN),
    "bn_act_backward_dbias": (["pcfm_bn_act_bwd"], R.SHAPES_BN),
    "bn_act_backward_parts": (["pcfm_bn_act_bwd_apply_parts"], BWD_PARTS),
    "bn_act_backward_split": (["pcfm_bn_act_bwd_split"], R.SHAPES_SPLIT),
    "bn_se_backward_stats": (["pcfm_bn_se_bwd_stats"], R.SHAPES_SE),
    "bn_se_backward_apply_split": (["pcfm_bn_se_bwd_apply_split"], R.SHAPES_SE),
    "gn_film_res_forward": (["pcfm_gn_film_res_fwd"], R.SHAPES_GN),
    "gn_film_res_backward": (["pcfm_gn_film_res_bwd"], R.SHAPES_GN),
    "gn_silu_forward": (["pcfm_gn_silu_fwd"], R.SHAPES_GN),
    "gn_silu_backward": (["pcfm_gn_silu_bwd"], R.SHAPES_GN),
    "gn_film_res_forward_bnin": (["pcfm_gn_film_res_fwd_bnin"], R.SHAPES_GN),
    "gn_film_res_backward_bnin": (["pcfm_gn_film_res_bwd_bnin", "pcfm_bn_act_bwd_apply_parts"],
                                  R.SHAPES_GN),
}
# shape-major, so that the entries of one shape share its cached reference
CASES = sorted(((e, s, k) for e, (_, shapes) in ENTRIES.items() for s in shapes for k in R.KINDS),
               key=lambda c: (c[0][:2], c[1][:3], c[2], c[0], c[1]))
IDS = [f"{e}-{sid(s)}-{k}" for e, s, k in CASES]


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    return ops


def test_every_launching_norm_entry_is_in_a_case():
    """include/pcfm.h's pcfm_bn_* / pcfm_gn_* names that launch a kernel (all but the
    size queries) against the entries the table above drives."""
    with open(os.path.join(os.path.dirname(HERE), "include", "pcfm.h")) as f:
        names = set(re.findall(r"\b(pcfm_(?:bn|gn)_\w+)\s*\(", f.read()))
    launching = {n for n in names if not n.endswith("_bytes") and n != "pcfm_gn_bnin_parts"}
    assert len(launching) == 16
    assert launching == {n for ents, _ in ENTRIES.values() for n in ents}


def _dev(t):
    return t.cuda()


def _running(inp):
    return (_dev(inp["rm"]).clone(), _dev(inp["rv"]).clone(),
            torch.full((), R.NBT0, dtype=torch.int64, device="cuda"))


def _stats_dict(m, iv, rm, rv, nbt):
    return {"mean": m.cpu(), "invstd": iv.cpu(), "running_mean": rm.cpu(),
            "running_var": rv.cpu(), "nbt": int(nbt)}


def _kernel_stats(ops, inp):
    """mean / invstd as the modules obtain them for a backward: the statistics pass"""
    rm, rv, nbt = _running(inp)
    return ops.bn_forward_stats(_dev(inp["x"]), inp["eps"], R.MOM, rm, rv, nbt)


def _run_bn(ops, entry, shape, kind, rec):
    if entry == "bn_act_backward_parts":
        ref = R.bn_bwd_parts_ref(shape[:3], kind, shape[3])
        inp = ref["inp"]
        dx, dg, dbt, db = ops.bn_act_backward_parts(
            _dev(inp["dz"]), _dev(inp["x"]), _dev(inp["gamma"]), _dev(inp["beta"]),
            _dev(ref["mean32"]), _dev(ref["invstd32"]), _dev(ref["part"]), inp["slope"],
            want_dbias_in=True)
        R.check_bn_backward({"dx": dx.cpu(), "dgamma": dg.cpu(), "dbeta": dbt.cpu(),
                             "dbias_in": db.cpu()}, ref, rec)
        return
    parts = entry.endswith("_parts")
    inp = R.make_inputs("bn_parts" if parts else "bn", shape, kind)
    ref = R.bn_ref("bn_parts" if parts else "bn", shape, kind, "parts" if parts else "pass")
    b, c, s = inp["b"], inp["c"], inp["s"]
    x, gamma, beta = _dev(inp["x"]), _dev(inp["gamma"]), _dev(inp["beta"])
    eps, slope = inp["eps"], inp["slope"]
    if "forward" in entry:
        rm, rv, nbt = _running(inp)
        out = {}
        if entry == "bn_forward_stats":
            m, iv = ops.bn_forward_stats(x, eps, R.MOM, rm, rv, nbt)
        elif entry == "bn_forward_stats_parts":
            st = _dev(R.synth_group_stats(inp["x"], inp["gsz"]))
            m, iv = ops.bn_forward_stats(x, eps, R.MOM, rm, rv, nbt, parts=st)
        elif entry == "bn_act_forward_parts":
            st = _dev(R.synth_group_stats(inp["x"], inp["gsz"]))
            y, m, iv = ops.bn_act_forward_parts(x, st, gamma, beta, eps, slope, R.MOM, rm, rv, nbt)
            out["y"] = y.cpu()
        elif entry == "bn_act_forward":
            y, m, iv = ops.bn_act_forward(x, gamma, beta, eps, slope, R.MOM, rm, rv, nbt)
            assert y.shape == x.shape and y.dtype == torch.float32
            out["y"] = y.cpu()
        elif entry == "bn_act_forward_split":
            ys, m, iv = ops.bn_act_forward_split(x, gamma, beta, eps, slope, R.MOM, rm, rv, nbt)
            out["y"], out["split"] = R.unsplit(ys.cpu(), b, c, s), True
        else:
            rowmean, m, iv = ops.bn_act_forward_rowmean(x, gamma, beta, eps, slope, R.MOM, rm, rv,
                                                        nbt)
            assert rowmean.shape == (b, c)
            out["rowmean"] = rowmean.cpu()
        assert m.shape == iv.shape == (c,)
        R.check_bn_stats(_stats_dict(m, iv, rm, rv, nbt), ref, rec)
        R.check_bn_forward(out, ref, rec)
        return
    m, iv = _kernel_stats(ops, inp)
    dz = _dev(inp["dz"])
    if entry in ("bn_act_backward", "bn_act_backward_dbias"):
        want = entry.endswith("dbias")
        dx, dg, dbt, db = ops.bn_act_backward(dz, x, gamma, beta, m, iv, slope, want_dbias_in=want)
        assert (db is not None) == want and dx.shape == x.shape
        R.check_bn_backward({"dx": dx.cpu(), "dgamma": dg.cpu(), "dbeta": dbt.cpu(),
                             "dbias_in": db.cpu() if want else None}, ref, rec)
    elif entry == "bn_act_backward_split":
        dxs, dg, dbt, db = ops.bn_act_backward_split(dz, x, gamma, beta, m, iv, slope,
                                                     want_dbias_in=True)
        R.check_bn_backward({"dx": R.unsplit(dxs.cpu(), b, c, s), "dgamma": dg.cpu(),
                             "dbeta": dbt.cpu(), "dbias_in": db.cpu()}, ref, rec, split=True)
    else:
        rowstats = ops.bn_se_backward_stats(dz, x, m, iv, gamma, beta, slope)
        assert rowstats.shape == (5, b, c)
        if entry == "bn_se_backward_stats":
            R.check_se_rowstats({"rowstats": rowstats.cpu()}, ref, rec)
            return
        dxs, dg, dbt, db = ops.bn_se_backward_apply_split(
            dz, x, m, iv, gamma, beta, _dev(inp["se_s"]), _dev(inp["dmv"]), rowstats, slope,
            want_dbias_in=True)
        R.check_bn_backward({"dx": R.unsplit(dxs.cpu(), b, c, s), "dgamma": dg.cpu(),
                             "dbeta": dbt.cpu(), "dbias_in": db.cpu()}, ref, rec, se=True,
                            split=True)


def _bn_part_of(ref):
    """the BatchNorm statistics' reference and bounds of a bnin case, as check_bn_stats reads them"""
    return {"mean": ref["bn_mean"], "invstd": ref["bn_invstd"], "mean_b": ref["bn_mean_b"],
            "relis": ref["bn_relis"], "n": 2, "running_mean": ref["running_mean"],
            "running_mean_b": ref["running_mean_b"], "running_var": ref["running_var"],
            "running_var_b": ref["running_var_b"]}


def _run_gn(ops, entry, shape, kind, rec):
    b, c, n, groups = shape
    bnin = entry.endswith("bnin")
    fam = "bnin" if bnin else ("gn_silu" if "silu" in entry else "gn_film")
    inp = R.make_inputs(fam, shape, kind)
    ref = R.bnin_ref(shape, kind) if bnin else R.gn_ref(fam, shape, kind)
    w, bias, dout = _dev(inp["w"]), _dev(inp["bias"]), _dev(inp["dout"])
    gamma, beta, eps = _dev(inp["gamma"]), _dev(inp["beta"]), inp["eps"]
    if bnin:
        y, bg, bb = _dev(inp["y"]), _dev(inp["bn_gamma"]), _dev(inp["bn_beta"])
        rm, rv, nbt = _running(inp)
        m, iv = ops.bn_forward_stats(y, inp["bn_eps"], R.MOM, rm, rv, nbt)
        out, gm, grs = ops.gn_film_res_forward_bnin(y, m, iv, bg, bb, 0.0, w, bias, gamma, beta,
                                                    groups, eps)
        if "forward" in entry:
            R.check_bn_stats(_stats_dict(m, iv, rm, rv, nbt), _bn_part_of(ref),
                             lambda nm, v: rec("bn_" + nm, v))
            R.check_gn_forward({"out": out.cpu(), "mean": gm.cpu(), "rstd": grs.cpu()}, ref, rec)
            return
        dz, dw, dbias, dgamma, dbeta, bnpart = ops.gn_film_res_backward_bnin(
            dout, y, m, iv, bg, bb, 0.0, w, bias, gamma, gm, grs, groups)
        assert bnpart.shape == (c, b * -(-(n // 4) // 256), 2)
        dy, dgb, dbb, db = ops.bn_act_backward_parts(dz, y, bg, bb, m, iv, bnpart, 0.0,
                                                     want_dbias_in=True)
        res = {"dz": dz.cpu(), "dw": dw.cpu(), "dbias": dbias.cpu(), "dgamma": dgamma.cpu(),
               "dbeta": dbeta.cpu(), "bnpart": bnpart.cpu(), "dy": dy.cpu(), "bn_dgamma": dgb.cpu(),
               "bn_dbeta": dbb.cpu(), "dbias_in": db.cpu()}
        R.check_gn_backward(res, ref, rec, dx_key="dz")
        R.check_bnin_chain(res, ref, rec)
        return
    x = _dev(inp["x"])
    if fam == "gn_silu":
        out, gm, grs = ops.gn_silu_forward(x, w, bias, groups, eps)
    else:
        out, gm, grs = ops.gn_film_res_forward(x, w, bias, gamma, beta, groups, eps)
    assert gm.shape == grs.shape == (b, groups) and out.shape == x.shape
    if "forward" in entry:
        R.check_gn_forward({"out": out.cpu(), "mean": gm.cpu(), "rstd": grs.cpu()}, ref, rec)
    elif fam == "gn_silu":
        dx, dw, dbias = ops.gn_silu_backward(dout, x, w, bias, gm, grs, groups)
        R.check_gn_backward({"dx": dx.cpu(), "dw": dw.cpu(), "dbias": dbias.cpu()}, ref, rec)
    else:
        dx, dw, dbias, dgamma, dbeta = ops.gn_film_res_backward(dout, x, w, bias, gamma, gm, grs,
                                                                groups)
        assert dgamma.shape == dbeta.shape == (b, c)
        R.check_gn_backward({"dx": dx.cpu(), "dw": dw.cpu(), "dbias": dbias.cpu(),
                             "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu()}, ref, rec)


@pytest.mark.parametrize("entry,shape,kind", CASES, ids=IDS)
def test_entry_against_float64(ops, entry, shape, kind, report):
    key = f"norm_ref/{entry}/{sid(shape)}/{kind}/"
    rec = lambda name, v: report(key + name, v)  # noqa: E731
    (_run_bn if entry.startswith("bn_") else _run_gn)(ops, entry, shape, kind, rec)


@pytest.mark.parametrize("shape", [(2, 6, 4100), (1, 4, 70000)], ids=sid)
def test_records_invstd_with_the_first_element_30_sigma_out(ops, shape, report):
    """The known weak end of the shifted moments (A about 900): recorded, not
    asserted against a bound; the statistics must still be finite."""
    inp = R.make_inputs("bn", shape, "offset")
    core = R.bn_core(inp["x"], inp["gamma"], inp["beta"], inp["eps"], inp["slope"])
    x = inp["x"].clone()
    x[0, :, 0] = (core["mean"] + 30.0 * core["var"].sqrt()).float()
    core = R.bn_core(x, inp["gamma"], inp["beta"], inp["eps"], inp["slope"])
    rm, rv, nbt = _running(inp)
    m, iv = ops.bn_forward_stats(_dev(x), inp["eps"], R.MOM, rm, rv, nbt)
    rel = (iv.cpu().double() - core["invstd"]).abs() / core["invstd"]
    assert bool(torch.isfinite(rel).all())
    k = R.counts("bn", shape)
    report(f"norm_ref/first_30/{sid(shape)}",
           {"A": float(core["A"].max()), "invstd_rel_err": float(rel.max()),
            "bound": float((0.5 * k["k_var"] * R.E * core["A"] * core["vv"] + 3 * R.E).max())})


# ---------------------------------------------------------------------------
# the module wrappers (modules/norm_act.py) at their smallest shapes: the plumbing
# between saved tensors and kernels under the same reference
# ---------------------------------------------------------------------------
def _bn_module(inp, c, eps, gamma, beta):
    bn = torch.nn.BatchNorm1d(c, eps=eps, momentum=R.MOM).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        bn.running_mean.copy_(inp["rm"])
        bn.running_var.copy_(inp["rv"])
        bn.num_batches_tracked.fill_(R.NBT0)
    return bn


def _gn_module(inp, c, groups):
    norm = torch.nn.GroupNorm(groups, c, eps=inp["eps"]).cuda()
    with torch.no_grad():
        norm.weight.copy_(inp["w"])
        norm.bias.copy_(inp["bias"])
    return norm


@pytest.mark.parametrize("kind", R.KINDS)
def test_bn_act_wrapper(ops, kind, report):
    from modules.norm_act import _fusable, bn_act
    shape = R.SHAPES_BN[0]
    inp, ref = R.make_inputs("bn", shape, kind), R.bn_ref("bn", shape, kind)
    bn = _bn_module(inp, inp["c"], inp["eps"], inp["gamma"], inp["beta"])
    x = _dev(inp["x"]).requires_grad_(True)
    assert _fusable(x, bn)
    z = bn_act(x, bn, inp["slope"])
    z.backward(_dev(inp["dz"]))
    rec = lambda name, v: report(f"norm_ref/wrapper_bn_act/{sid(shape)}/{kind}/{name}", v)  # noqa: E731
    R.check_bn_forward({"y": z.detach().cpu()}, ref, rec)
    R.check_bn_backward({"dx": x.grad.cpu(), "dgamma": bn.weight.grad.cpu(),
                         "dbeta": bn.bias.grad.cpu()}, ref, rec)
    R.check_bn_stats({"running_mean": bn.running_mean.cpu(), "running_var": bn.running_var.cpu(),
                      "nbt": int(bn.num_batches_tracked)}, ref, rec)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("fam", ["gn_film", "gn_silu"])
def test_gn_wrappers(ops, fam, kind, report):
    from modules.norm_act import _GNFiLMRes, _GNSiLU, gn_film_residual, gn_silu
    shape = R.SHAPES_GN[0]
    b, c, n, groups = shape
    inp, ref = R.make_inputs(fam, shape, kind), R.gn_ref(fam, shape, kind)
    norm = _gn_module(inp, c, groups)
    x = _dev(inp["x"]).requires_grad_(True)
    res = {}
    if fam == "gn_silu":
        out = gn_silu(x, norm)
        assert isinstance(out.grad_fn, _GNSiLU._backward_cls)
        out.backward(_dev(inp["dout"]))
    else:
        gamma, beta = _dev(inp["gamma"]).requires_grad_(True), _dev(inp["beta"]).requires_grad_(True)
        out = gn_film_residual(x, norm, gamma, beta)
        assert isinstance(out.grad_fn, _GNFiLMRes._backward_cls)
        out.backward(_dev(inp["dout"]))
        res.update({"dgamma": gamma.grad.cpu(), "dbeta": beta.grad.cpu()})
    res.update({"dx": x.grad.cpu(), "dw": norm.weight.grad.cpu(), "dbias": norm.bias.grad.cpu()})
    rec = lambda name, v: report(f"norm_ref/wrapper_{fam}/{sid(shape)}/{kind}/{name}", v)  # noqa: E731
    R.check_gn_forward({"out": out.detach().cpu()}, ref, rec)
    R.check_gn_backward(res, ref, rec)


@pytest.mark.parametrize("kind", R.KINDS)
def test_post_gn_film_residual_wrapper(ops, kind, report):
    """The PV block's tail as one node.  The post SharedMLP's 1x1 conv carries the
    identity and the input lies on the grid a bf16 hi / lo pair holds exactly
    ("bnin_q"), so the GEMM's products 1 * hi + 1 * lo reproduce it in any summation
    order: the conv output is the reference's y.  The data gradient is the
    reference's dy through the backward GEMM's own hi / lo pair: + 2^-16 |dy|."""
    import modules.norm_act as na
    from modules.shared_mlp import SharedMLP
    shape = R.SHAPES_GN[0]
    b, c, n, groups = shape
    inp, ref = R.make_inputs("bnin_q", shape, kind), R.bnin_ref(shape, kind, "bnin_q")
    post = SharedMLP(c, [c]).cuda().train()
    conv, bn = post.layers[0], post.layers[1]
    with torch.no_grad():
        conv.weight.copy_(torch.eye(c).view_as(conv.weight))
        conv.bias.zero_()
        bn.weight.copy_(inp["bn_gamma"])
        bn.bias.copy_(inp["bn_beta"])
        bn.running_mean.copy_(inp["rm"])
        bn.running_var.copy_(inp["rv"])
        bn.num_batches_tracked.fill_(R.NBT0)
        assert bn.eps == inp["bn_eps"] and bn.momentum == R.MOM
        assert torch.equal(conv(_dev(inp["y"])), _dev(inp["y"]))
    norm = _gn_module(inp, c, groups)
    x = _dev(inp["y"]).requires_grad_(True)
    gamma, beta = _dev(inp["gamma"]).requires_grad_(True), _dev(inp["beta"]).requires_grad_(True)
    out = na.post_gn_film_residual(post, norm, x, gamma, beta)
    assert isinstance(out.grad_fn, na._PostGNFiLMRes._backward_cls)
    out.backward(_dev(inp["dout"]))
    rec = lambda name, v: report(f"norm_ref/wrapper_post_gn/{sid(shape)}/{kind}/{name}", v)  # noqa: E731
    R.check_gn_forward({"out": out.detach().cpu()}, ref, rec)
    st = {"running_mean": bn.running_mean.cpu(), "running_var": bn.running_var.cpu(),
          "nbt": int(bn.num_batches_tracked)}
    R.check_bn_stats(st, _bn_part_of(ref), lambda nm, v: rec("bn_" + nm, v))
    res = {"dw": norm.weight.grad.cpu(), "dbias": norm.bias.grad.cpu(),
           "dgamma": gamma.grad.cpu(), "dbeta": beta.grad.cpu(),
           "dy": x.grad.cpu(), "bn_dgamma": bn.weight.grad.cpu(), "bn_dbeta": bn.bias.grad.cpu(),
           "dbias_in": conv.bias.grad.cpu()}
    R.check_gn_backward(res, ref, rec, dx_key="dz")
    R.check_bnin_chain(res, ref, rec, dy_pair=True)
