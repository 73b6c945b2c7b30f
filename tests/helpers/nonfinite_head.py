"""The head's FiLM / SiLU row kernels in the non-finite table
(tests/helpers/nonfinite_ref.py): head_film_fwd / head_film_bwd as the first block
(h16, with and without hbias) and as a later block (uprev + gprev, shift recomputed),
head_silu_fwd / head_silu_bwd.  Inputs and the float64 autograd references are those
of tests/helpers/head_film_ref.py (LayerNorm per row, FiLM per cloud, SiLU)."""
import torch

import head_film_ref as H
import nonfinite_ref as R

B, N, W = 2, 500, 256  # 1000 rows: forward blocks of 32 rows, backward chunks of 256,
#                        one chunk (rows 256..511) holding rows of both clouds
FORMS = ("first_hbias", "first", "later")
_META = ("b", "n", "w", "first")


def _full(inp, form):
    """the tensor dict of a case -> head_film_ref's input dict"""
    d = {"b": B, "n": N, "w": W, "first": form != "later", "h16": None, "hbias": None,
         "uprev": None, "gprev": None}
    d.update(inp)
    return d


def _film_make(form):
    def make():
        inp = H.make_inputs(B, N, W, form != "later")
        if form == "first":
            inp["hbias"] = None
        return {k: v for k, v in inp.items() if k not in _META and v is not None}
    return make


def film_ref(inp, form, backward):
    ref = H.film_ref(_full(inp, form))
    if not backward:
        return {k: ref[k] for k in ("u", "mean", "rstd")}
    dh = ref["dh"]
    out = {k: ref[k] for k in ("dh", "dsp1", "dshift", "dgamma", "dbeta")}
    out["dbias"] = dh.sum(0)
    if form == "first_hbias":
        out["dbias_b"] = dh.view(B, N, W).sum(1)
    return out


def run_film(ops, e, d):
    form = e.params["form"]
    g = d.get
    u, a, mean, rstd = ops.head_film_fwd(g("h16"), g("uprev"), g("gprev"), d["gamma"], d["beta"],
                                         d["sp1"], d["shift"], N, H.EPS, hbias=g("hbias"))
    if e.name == "head_film_fwd":
        return {"u": u, "mean": mean, "rstd": rstd}
    first = form != "later"
    res = ops.head_film_bwd(d["dh_next"], d["da16"], u if first else None, g("h16"), g("uprev"),
                            g("gprev"), mean, rstd, d["gamma"], d["beta"], d["sp1"], N,
                            want_dh=True, hbias=g("hbias"), shift=None if first else d["shift"])
    names = ("dh", "dh16", "dsp1", "dshift", "dgamma", "dbeta", "dbias", "dbias_b")
    out = dict(zip(names, res))
    del out["dh16"]  # a rounding of dh
    return out


def _silu_make():
    inp = H.make_silu_inputs(B, N, W)
    return {k: v for k, v in inp.items() if k not in _META}


def silu_ref(inp, backward):
    ref = H.silu_ref(_full(inp, "later"))
    if not backward:
        return {"a": ref["a"]}
    return {"dh": ref["dh"], "dbias": ref["dh"].sum(0)}


def run_silu(ops, e, d):
    if e.name == "head_silu_fwd":
        return {"a.hi": ops.head_silu_fwd(d["uprev"], d["gprev"], N)}  # bf16: one plane
    dh, _, dbias = ops.head_silu_bwd(d["da16"], d["uprev"], d["gprev"], N)
    return {"dh": dh, "dbias": dbias}


def entries():
    rows = B * N
    # first / last row, each side of a forward block, of a backward chunk and of the
    # boundary between the clouds (inside one backward chunk)
    elem = [(0, 0), (rows - 1, W - 1)] + [(r, W // 2) for r in (31, 32, 255, 256, N - 1, N)]
    col, per = [(0,), (W - 1,)], [(0, 0), (B - 1, W - 1)]
    out = []
    for form in FORMS:
        x = "uprev" if form == "later" else "h16"
        fwd = {x: elem, "gamma": col, "beta": col, "sp1": per, "shift": per}
        if form == "later":
            fwd["gprev"] = elem[:2]
        if form == "first_hbias":
            fwd["hbias"] = per
        bwd = dict(fwd, dh_next=elem, da16=elem)
        del bwd["beta"]  # beta does not enter the backward (u is handed over / recomputed)
        for name, sites, back in (("head_film_fwd", fwd, False), ("head_film_bwd", bwd, True)):
            if back and form != "later":
                del sites["shift"]  # first block: the backward reads the forward's u
            out.append(R.Entry("more", name, (B, N, W), _film_make(form), sites,
                               lambda inp, form=form, back=back: film_ref(inp, form, back),
                               opposing=(x, (5, 0), (5, 1)), params={"form": form}))
    sil = {"uprev": elem, "gprev": elem[:2]}
    out.append(R.Entry("more", "head_silu_fwd", (B, N, W), _silu_make, sil,
                       lambda inp: silu_ref(inp, False)))
    out.append(R.Entry("more", "head_silu_bwd", (B, N, W), _silu_make, dict(sil, da16=elem),
                       lambda inp: silu_ref(inp, True), opposing=("uprev", (5, 0), (6, 0))))
    return out


def run(ops, e, d):
    return (run_film if "film" in e.name else run_silu)(ops, e, d)
