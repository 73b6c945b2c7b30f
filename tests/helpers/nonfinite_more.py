"""Further cases of the non-finite table (tests/helpers/nonfinite_ref.py): the
consumers of BnChan outside the plain BatchNorm passes (statistics from a producer,
the GroupNorm passes over a pre-BatchNorm tensor with the BatchNorm backward on their
partial sums, the devoxelization gather that applies act(bn(.)) while staging), the
channel-segmented pointwise GEMM, and the head's row kernels (tgate, column sums,
the bf16 weight gradient).  Each entry: clean inputs, sites, a float64 reference,
and its runner through pcfm.ops (run)."""
import torch
import torch.nn.functional as F

import nonfinite_ref as R

Entry, EPS, MOM = R.Entry, R.EPS, R.MOM


# ---------------------------------------------------------------------------
# BatchNorm from a producer's group statistics
# ---------------------------------------------------------------------------
PARTS_SHAPE, PARTS_GROUP = (2, 5, 100), 32  # P = 8, a ragged last group of 4


def _bn_parts_entries():
    out = []
    sh = PARTS_SHAPE
    opp = ("x", (0, 1, 0), (0, 1, 1))
    for slope in (0.0, 0.1):
        out.append(Entry("more", "bn_act_forward_parts", sh, R._bn_make(sh, slope),
                         R._bn_sites(sh, ("x", "gamma", "beta")),
                         lambda inp, slope=slope: R.bn_forward_ref(inp, slope), opposing=opp,
                         params={"slope": slope}))

    def stats_ref(inp):
        r = R.bn_forward_ref(inp, 0.0)
        del r["y"]
        return r
    out.append(Entry("more", "bn_forward_stats_parts", sh, R._bn_make(sh, 0.0),
                     R._bn_sites(sh, ("x",)), stats_ref, opposing=opp))
    return out


def _run_bn_parts(ops, e, d):
    x = d["x"]
    # the producer's epilogue statistics of the (special) x: float64 group mean and
    # centred sum of squares, as float32 (c, b * groups, 2)
    st = R.pw_group_stats(x.double(), PARTS_GROUP).float().contiguous()
    rm, rv = d["rm"].clone(), d["rv"].clone()
    nbt = torch.full((), R.NBT0, dtype=torch.int64, device=x.device)
    out = {}
    if e.name == "bn_act_forward_parts":
        out["y"], m, iv = ops.bn_act_forward_parts(x, st, d["gamma"], d["beta"], EPS,
                                                   e.params["slope"], MOM, rm, rv, nbt)
    else:
        m, iv = ops.bn_forward_stats(x, EPS, MOM, rm, rv, nbt, parts=st)
    out.update({"mean": m, "invstd": iv, "running_mean": rm, "running_var": rv})
    return out


# ---------------------------------------------------------------------------
# GroupNorm-FiLM residual over z = act(bn(y)), y the pre-BatchNorm tensor; its
# backward hands the BatchNorm backward its partial sums (bn_act_backward_parts)
# ---------------------------------------------------------------------------
BNIN_SHAPE = (3, 6, 36, 3)


def _bnin_make(slope):
    def make():
        b, c, n, _ = BNIN_SHAPE
        g = R._gen("bnin", BNIN_SHAPE, slope)
        return {"y": R._randn(g, b, c, n) + 0.5, "dout": R._randn(g, b, c, n),
                "bn_gamma": 1.0 + 0.25 * R._randn(g, c), "bn_beta": 0.25 * R._randn(g, c),
                "rm": 0.1 * R._randn(g, c), "rv": 1.0 + 0.1 * torch.rand(c, generator=g),
                "w": 1.0 + 0.25 * R._randn(g, c), "bias": 0.25 * R._randn(g, c),
                "gamma": 0.25 * R._randn(g, b, c), "beta": 0.25 * R._randn(g, b, c)}
    return make


def bnin_ref(inp, slope, backward):
    groups = BNIN_SHAPE[3]
    names = ("y", "bn_gamma", "bn_beta", "w", "bias", "gamma", "beta")
    t = {k: inp[k].double().requires_grad_(True) for k in names}
    y = t["y"]
    pre, mean, var, invstd = R._bn_pre(y, t["bn_gamma"], t["bn_beta"])
    z = R._act(pre, slope)
    gn = F.group_norm(z, groups, t["w"], t["bias"], EPS)
    out = z + (gn * (1.0 + t["gamma"][:, :, None]) + t["beta"][:, :, None])
    if not backward:
        n = y.numel() // y.shape[1]
        zg = z.detach().reshape(y.shape[0], groups, -1)
        return {"out": out.detach(), "mean": zg.mean(2),
                "rstd": (zg.var(2, unbiased=False) + EPS).rsqrt(),
                "bn_mean": mean.detach(), "bn_invstd": invstd.detach(),
                "running_mean": (1 - MOM) * inp["rm"].double() + MOM * mean.detach(),
                "running_var": (1 - MOM) * inp["rv"].double() + MOM * (var.detach() * n / (n - 1))}
    order = ("w", "bias", "gamma", "beta", "y", "bn_gamma", "bn_beta")
    gr = torch.autograd.grad(out, [z] + [t[k] for k in order], inp["dout"].double())
    res = dict(zip(("dz", "dw", "dbias", "dgamma", "dbeta", "dy", "bn_dgamma", "bn_dbeta"), gr))
    dy = res["dy"]
    res["dbias_in"] = dy.sum((0, 2))

    def post(cls):  # dbias_in is an analytically zero sum: see nonfinite_ref.bn_backward_ref
        nf, _, val = cls["dbias_in"]
        moved = (cls["dy"][0] | cls["dy"][1]).transpose(0, 1).flatten(1).any(1)
        mag = torch.where(torch.isfinite(dy), dy.abs(), torch.zeros_like(dy)).sum((0, 2))
        cls["dbias_in"] = (nf, ~nf & moved, val, float(mag.max()))
    res["_post"] = post
    return res


def _bnin_entries():
    b, c, n, _ = BNIN_SHAPE
    elem = [(0, 0, 0), (b - 1, c - 1, n - 1), (1, 2, 31), (1, 3, 32)]
    chan, row = [(0,), (c - 1,)], [(0, 0), (b - 1, c - 1)]
    out = []
    for slope in (0.0, 0.1):
        for backward in (False, True):
            sites = {"y": elem, "bn_gamma": chan, "bn_beta": chan, "w": chan, "bias": chan,
                     "gamma": row}
            if backward:
                sites["dout"] = elem
            else:
                sites["beta"] = row
            out.append(Entry("more", "gn_film_res_%s_bnin" % ("backward" if backward else "forward"),
                             BNIN_SHAPE, _bnin_make(slope), sites,
                             lambda inp, slope=slope, backward=backward: bnin_ref(inp, slope,
                                                                                  backward),
                             opposing=("y", (0, 2, 0), (0, 2, 1)), params={"slope": slope}))
    return out


def _run_bnin(ops, e, d):
    groups, slope = BNIN_SHAPE[3], e.params["slope"]
    y, bg, bb = d["y"], d["bn_gamma"], d["bn_beta"]
    rm, rv = d["rm"].clone(), d["rv"].clone()
    nbt = torch.full((), R.NBT0, dtype=torch.int64, device=y.device)
    m, iv = ops.bn_forward_stats(y, EPS, MOM, rm, rv, nbt)
    out, gm, grs = ops.gn_film_res_forward_bnin(y, m, iv, bg, bb, slope, d["w"], d["bias"],
                                                d["gamma"], d["beta"], groups, EPS)
    if "forward" in e.name:
        return {"out": out, "mean": gm, "rstd": grs, "bn_mean": m, "bn_invstd": iv,
                "running_mean": rm, "running_var": rv}
    dz, dw, dbias, dgamma, dbeta, bnpart = ops.gn_film_res_backward_bnin(
        d["dout"], y, m, iv, bg, bb, slope, d["w"], d["bias"], d["gamma"], gm, grs, groups)
    dy, dgb, dbb, db = ops.bn_act_backward_parts(dz, y, bg, bb, m, iv, bnpart, slope,
                                                 want_dbias_in=True)
    return {"dz": dz, "dw": dw, "dbias": dbias, "dgamma": dgamma, "dbeta": dbeta, "dy": dy,
            "bn_dgamma": dgb, "bn_dbeta": dbb, "dbias_in": db}


# ---------------------------------------------------------------------------
# Devoxelization with SE scale and the point-branch sum folded in; the BN form
# gathers act(bn(x)) (LeakyReLU 0.1) and adds act(bn(add)) (ReLU), never written
# ---------------------------------------------------------------------------
DEVOX_SHAPE = R.SCATTER_SHAPES[0]


def _devox_make(geo):
    def make():
        b, c, n, r = DEVOX_SHAPE
        g = R._gen("devox-sa", DEVOX_SHAPE)
        return {"grid": R._randn(g, b, c, r ** 3) + 0.5, "scale": torch.rand(b, c, generator=g) + 0.25,
                "add": R._randn(g, b, c, n) + 0.5, "gamma": 1.0 + 0.25 * R._randn(g, c),
                "beta": 0.25 * R._randn(g, c), "add_gamma": 1.0 + 0.25 * R._randn(g, c),
                "add_beta": 0.25 * R._randn(g, c), "pts": geo["pts"], "inds": geo["inds"].int(),
                "wgts": geo["wgts"].float()}
    return make


def devox_sa_ref(inp, bn):
    b, c, n, r = DEVOX_SHAPE
    grid, add = inp["grid"].double(), inp["add"].double()
    if bn:
        grid = R._act(R._bn_pre(grid, inp["gamma"].double(), inp["beta"].double())[0], 0.1)
        add = R._act(R._bn_pre(add, inp["add_gamma"].double(), inp["add_beta"].double())[0], 0.0)
    inds, wgts = inp["inds"].long(), inp["wgts"].double()
    dv = torch.zeros(b, c, n, dtype=torch.float64)
    for k in range(8):  # the forward reads the folded corners: 0 * inf counts
        dv = dv + wgts[:, k:k + 1] * torch.gather(grid, 2, inds[:, k:k + 1].expand(b, c, n))
    return {"outs": inp["scale"].double()[:, :, None] * dv + add}


def _devox_entries():
    b, c, n, r = DEVOX_SHAPE
    geo = R._scatter_geometry(DEVOX_SHAPE)
    inds = geo["inds"]
    pts = R._pw_elem_sites(b, c, n)
    read = [(bi, ci, int(inds[bi, 0, p])) for bi, ci, p in pts[:2]] + [
        (0, 1, int(inds[0, 0, R.INT_POINT])), (b - 1, c - 1, int(inds[b - 1, 7, R.HALF_POINT]))]
    row, chan = [(0, 0), (b - 1, c - 1)], [(0,), (c - 1,)]
    plain = {"grid": read, "scale": row, "add": pts}
    full = dict(plain, gamma=chan, beta=chan, add_gamma=chan, add_beta=chan)
    return [Entry("more", "trilinear_devoxelize_scale_add", DEVOX_SHAPE, _devox_make(geo), plain,
                  lambda inp: devox_sa_ref(inp, False)),
            Entry("more", "trilinear_devoxelize_bn_scale_add", DEVOX_SHAPE, _devox_make(geo), full,
                  lambda inp: devox_sa_ref(inp, True),
                  opposing=("grid", (0, 2, 5), (0, 2, 6)))]


def _run_devox(ops, e, d):
    b, c, n, r = DEVOX_SHAPE
    if e.name == "trilinear_devoxelize_scale_add":
        return {"outs": ops.trilinear_devoxelize_scale_add(r, True, d["pts"], d["grid"], d["scale"],
                                                           d["add"])[0]}
    m, iv = ops.bn_forward_stats(d["grid"], EPS, MOM, None, None)
    am, aiv = ops.bn_forward_stats(d["add"], EPS, MOM, None, None)
    return {"outs": ops.trilinear_devoxelize_bn_scale_add(
        r, True, d["pts"], d["grid"], m, iv, d["gamma"], d["beta"], 0.1, d["scale"], d["add"],
        add_bn=(am, aiv, d["add_gamma"], d["add_beta"], 0.0))[0]}


# ---------------------------------------------------------------------------
# Channel-segmented pointwise GEMM: y = W cat(parts) + bias without the concat
# ---------------------------------------------------------------------------
PW_PARTS_WIDTHS = (32, 32, 32, 7)
PW_PARTS_SHAPE = (2, sum(PW_PARTS_WIDTHS), 130, 65)  # (b, cin, cout, n)


def _pw_parts_entries():
    b, cin, cout, n = PW_PARTS_SHAPE
    # first; last channel of the ragged last part at the last point; each side of a part
    # boundary; the first channel of the last part at each side of the 32-point edge
    xs = [(0, 0, 0), (b - 1, cin - 1, n - 1), (1, 31, 10), (1, 32, 10), (1, 96, 31), (1, 96, 32)]
    gs = R._pw_elem_sites(b, cout, n)
    ws, bs = [(0, 0, 0), (cout - 1, cin - 1, 0), (5, 96, 0)], [(0,), (cout - 1,)]
    out = []
    for name, sites, opp in (
            ("pointwise_forward_parts", {"x": xs, "w": ws, "bias": bs}, ("x", (0, 31, 0), (0, 32, 0))),
            ("pointwise_backward_weight_parts", {"x": xs, "gy": gs}, ("x", (0, 96, 0), (0, 96, 1)))):
        out.append(Entry("more", name, PW_PARTS_SHAPE, R.pw_make(PW_PARTS_SHAPE), sites,
                         lambda inp, name=name: R.pw_full_ref(name, inp), opposing=opp,
                         masks=R.pw_masks))
    return out


def _run_pw_parts(ops, e, d):
    xs = [t.contiguous() for t in torch.split(d["x"], PW_PARTS_WIDTHS, 1)]
    if e.name == "pointwise_forward_parts":
        return {"y": ops.pointwise_forward_parts(xs, d["w"][:, :, 0].contiguous(), d["bias"])}
    return {"dw": ops.pointwise_backward_weight_parts(xs, d["gy"])}


# ---------------------------------------------------------------------------
# Head rows: the time gate, column sums, the bf16 weight gradient
# ---------------------------------------------------------------------------
TGATE_SHAPE = (2, 70, 130)  # (b, c, n): ragged 64 x 64 tiles both ways


def _tgate_make():
    b, c, n = TGATE_SHAPE
    g = R._gen("tgate")
    return {"head": R._randn(g, b, c, n), "glb": R._randn(g, b, c), "dout": R._randn(g, b, n, c),
            "alpha": torch.rand(b, generator=g) * 0.5 + 0.25}


def _tgate_entries():
    b, c, n = TGATE_SHAPE
    elem = [(0, 0, 0), (b - 1, c - 1, n - 1), (1, 63, 63), (1, 64, 64), (1, 5, 127), (1, 5, 128)]
    delem = [(bi, p, ci) for bi, ci, p in elem]

    def fwd(inp):
        a = inp["alpha"].double()[:, None, None]
        return {"out": a * inp["head"].double().transpose(1, 2)
                + (1.0 - a) * inp["glb"].double()[:, None, :]}
    return [Entry("more", "tgate_forward", TGATE_SHAPE, _tgate_make,
                  {"head": elem, "glb": [(0, 0), (b - 1, c - 1)], "alpha": [(0,), (b - 1,)]}, fwd),
            Entry("more", "tgate_backward", TGATE_SHAPE, _tgate_make,
                  {"dout": delem, "alpha": [(0,), (b - 1,)]},
                  lambda inp: {"dhead": inp["alpha"].double()[:, None, None]
                               * inp["dout"].double().transpose(1, 2)})]


COLSUM_SHAPES = [((3, 777, 6), torch.bfloat16), ((2, 1000, 64), torch.float32)]


def _colsum_entries():
    out = []
    for sh, dt in COLSUM_SHAPES:
        b, rows, c = sh

        def make(sh=sh, dt=dt):
            return {"x": R._randn(R._gen("colsum", sh), *sh).to(dt)}
        sites = [(0, 0, 0), (b - 1, rows - 1, c - 1)] + [(1, p, c // 2)
                                                        for p in R._edge_points(rows)[1:-1]]
        out.append(Entry("more", "rows_colsum", sh, make, {"x": sites},
                         lambda inp: {"out": inp["x"].double().sum(1)},
                         opposing=("x", (0, 0, 1), (0, 1, 1)),
                         params={"dtype": str(dt).split(".")[1]}))
    return out


WGRAD_SHAPES = [(63, 128, 128), (4097, 256, 384)]  # (rows, M, N)


def _wgrad_make(sh):
    def make():
        rows, m, n = sh
        g = R._gen("rows_wgrad", sh)
        return {"gy": R._randn(g, rows, m).bfloat16(), "x": R._randn(g, rows, n).bfloat16()}
    return make


def wgrad_masks(entry, inp, operand, sites_kinds):
    """dW[m, n] = sum over rows of gy[r, m] * x[r, n]: an element of gy enters row m, one
    of x column n; that row / column on the special and the clean inputs (the full
    float64 product per injection is 4e8 multiply-adds at the larger shape)"""
    rows, m, n = entry.shape
    tri = R._mask_triple((m, n))
    for s in [s for s, _ in sites_kinds]:
        j = s[1]

        def line():
            if operand == "gy":
                return inp["gy"][:, j].double() @ inp["x"].double()
            return inp["gy"].double().t() @ inp["x"][:, j].double()
        clean = line()
        with R.poked(inp, operand, sites_kinds):
            spec = line()
        R._fill(tri, (j,) if operand == "gy" else (slice(None), j), spec, clean)
    return {"dw": tri}


def _wgrad_entries():
    out = []
    for sh in WGRAD_SHAPES:
        rows, m, n = sh

        def sites(w):
            return [(0, 0), (rows - 1, w - 1)] + [(p, w // 2) for p in R._edge_points(rows)[1:-1]]
        out.append(Entry("more", "rows_wgrad_bf16", sh, _wgrad_make(sh),
                         {"gy": sites(m), "x": sites(n)},
                         lambda inp: {"dw": inp["gy"].double().t() @ inp["x"].double()},
                         opposing=("gy", (0, 1), (1, 1)), masks=wgrad_masks))
    return out


def entries():
    import nonfinite_head
    return (_bn_parts_entries() + _bnin_entries() + _devox_entries() + _pw_parts_entries()
            + _tgate_entries() + _colsum_entries() + _wgrad_entries() + nonfinite_head.entries())


def run(ops, e, d):
    """the entry through pcfm.ops on the tensors' device -> {output: tensor}"""
    if e.name.startswith("head_"):
        import nonfinite_head
        return nonfinite_head.run(ops, e, d)
    if e.name.endswith("_parts") and e.name.startswith("bn_"):
        return _run_bn_parts(ops, e, d)
    if e.name.endswith("_bnin"):
        return _run_bnin(ops, e, d)
    if e.name.startswith("trilinear_"):
        return _run_devox(ops, e, d)
    if e.name.startswith("pointwise_"):
        return _run_pw_parts(ops, e, d)
    if e.name == "tgate_forward":
        return {"out": ops.tgate_forward(d["head"], d["glb"], d["alpha"])}
    if e.name == "tgate_backward":
        return {"dhead": ops.tgate_backward(d["dout"], d["alpha"])}
    if e.name == "rows_colsum":
        return {"out": ops.rows_colsum(d["x"])}
    return {"dw": ops.rows_wgrad_bf16(d["gy"], d["x"])}
