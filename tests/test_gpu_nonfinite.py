"""GPU: non-finite propagation through the gradient-path kernels (DESIGN.md
"Parity", the non-finite contract).  Training under AMP relies on an inf / NaN
produced anywhere reaching the gradients, where the fused update's found_inf skips
the step; a kernel must neither swallow one nor smear it over outputs that do not
depend on it.

For every case of tests/helpers/nonfinite_ref.py (the table tests/test_nonfinite_cpu.py
proves on the CPU) and every injection -- +inf, -inf, NaN 0x7FC00000, NaN 0x7FFFFFFF at
the first / last element, each side of the 32 / 64 / 128 tile edges, the ragged tails,
and +inf with -inf in one reduction -- the kernel's non-finite mask equals the float64
reference's, and every output the injection does not reach has the bits of the clean
call (R.check).  One test per (entry, shape, slope) loops its injections.

Also here: the weight images (a NaN weight stays NaN; finite weights give the image
the previous rounding gave), the five Stream128 K-chunk counts no other test reaches
against fp64, rows_max_bf16 against torch.max on the same tensor, and the fused
update's skip on a NaN gradient."""
import hashlib
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "helpers"))
import nonfinite_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRIES = R.all_entries()
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    return ops


def _running(d):
    return d["rm"].clone(), d["rv"].clone(), torch.full((), R.NBT0, dtype=torch.int64, device=DEV)


def _split(buf, shape):
    b, c = shape[:2]
    hi, lo = R.split_planes(buf, b, c, torch.Size(shape[2:]).numel())
    return hi.reshape(shape), lo.reshape(shape)


def _run_bn(ops, e, d):
    slope, name = e.params.get("slope", 0.0), e.name
    x, gamma, beta = d["x"], d["gamma"], d["beta"]
    rm, rv, nbt = _running(d)
    if "forward" in name:
        out = {}
        if name == "bn_forward_stats":
            m, iv = ops.bn_forward_stats(x, R.EPS, R.MOM, rm, rv, nbt)
        elif name == "bn_act_forward":
            out["y"], m, iv = ops.bn_act_forward(x, gamma, beta, R.EPS, slope, R.MOM, rm, rv, nbt)
        elif name == "bn_act_forward_split":
            ys, m, iv = ops.bn_act_forward_split(x, gamma, beta, R.EPS, slope, R.MOM, rm, rv, nbt)
            out["y.hi"], out["y.lo"] = _split(ys, e.shape)
        else:
            out["rowmean"], m, iv = ops.bn_act_forward_rowmean(x, gamma, beta, R.EPS, slope, R.MOM,
                                                               rm, rv, nbt)
        assert int(nbt) == R.NBT0 + 1
        out.update({"mean": m, "invstd": iv, "running_mean": rm, "running_var": rv})
        return out
    m, iv = ops.bn_forward_stats(x, R.EPS, R.MOM, rm, rv, nbt)  # as the modules obtain them
    if name == "bn_act_backward":
        dx, dg, dbt, db = ops.bn_act_backward(d["dz"], x, gamma, beta, m, iv, slope,
                                              want_dbias_in=True)
        return {"dx": dx, "dgamma": dg, "dbeta": dbt, "dbias_in": db}
    if name == "bn_act_backward_split":
        dxs, dg, dbt, db = ops.bn_act_backward_split(d["dz"], x, gamma, beta, m, iv, slope,
                                                     want_dbias_in=True)
    else:
        rowstats = ops.bn_se_backward_stats(d["dz"], x, m, iv, gamma, beta, slope)
        dxs, dg, dbt, db = ops.bn_se_backward_apply_split(d["dz"], x, m, iv, gamma, beta, d["se_s"],
                                                          d["dmv"], rowstats, slope,
                                                          want_dbias_in=True)
    hi, lo = _split(dxs, e.shape)
    return {"dx.hi": hi, "dx.lo": lo, "dgamma": dg, "dbeta": dbt, "dbias_in": db}


def _run_gn(ops, e, d):
    groups = e.shape[3]
    film = e.name.startswith("gn_film")
    x, w, bias = d["x"], d["w"], d["bias"]
    if film:
        out, m, rs = ops.gn_film_res_forward(x, w, bias, d["gamma"], d["beta"], groups, R.EPS)
    else:
        out, m, rs = ops.gn_silu_forward(x, w, bias, groups, R.EPS)
    if e.name.endswith("forward"):
        return {"out": out, "mean": m, "rstd": rs}
    if film:
        r = ops.gn_film_res_backward(d["dout"], x, w, bias, d["gamma"], m, rs, groups)
        return dict(zip(["dx", "dw", "dbias", "dgamma", "dbeta"], r))
    return dict(zip(["dx", "dw", "dbias"], ops.gn_silu_backward(d["dout"], x, w, bias, m, rs, groups)))


def _run_se(ops, e, d):
    s, hid = ops.se_mlp_forward(d["m"], d["w1"], d["w2"])
    if e.name.endswith("forward"):
        return {"s": s, "hid": hid}
    return dict(zip(["dm", "dw1", "dw2"],
                    ops.se_mlp_backward(d["m"], hid, s, d["ds"], d["w1"], d["w2"])))


def _run_pw(ops, e, d):
    if e.name == "pointwise_forward":
        return {"y": ops.pointwise_forward(d["x"], d["w"], d["bias"])}
    if e.name == "pointwise_forward_bnstats":
        ys = ops.pointwise_forward_bnstats(d["x"], d["w"], d["bias"])
        assert ys is not None
        return {"y": ys[0], "stats": ys[1]}
    if e.name == "pointwise_backward_data":
        return {"dx": ops.pointwise_backward_data(d["gy"], d["w"])}
    return {"dw": ops.pointwise_backward_weight(d["x"], d["gy"])}


def _runner(e):
    if e.family == "more":
        import nonfinite_more
        return nonfinite_more.run
    if e.name.startswith("bn_"):
        return _run_bn
    if e.name.startswith("gn_"):
        return _run_gn
    if e.name.startswith("se_mlp"):
        return _run_se
    if e.name.startswith("rows_"):
        return R.run_rows
    if e.family == "conv3d":
        return R.run_conv
    if e.family == "scatter":
        return R.run_scatter
    return _run_pw


@pytest.mark.parametrize("e", ENTRIES, ids=[e.id for e in ENTRIES])
def test_nothing_swallowed_invented_or_leaked(ops, e):
    inp = e.inputs()
    dev = {k: v.to(DEV) for k, v in inp.items()}
    run = _runner(e)
    if e.family == "pointwise":  # the form this shape is in the table for
        from pcfm import _lib
        b, cin, cout, n = e.shape
        form, group = R.PW_SHAPES[e.shape]
        groups = _lib.query("pcfm_pointwise_bnstats_groups", b, cin, cout, n)
        assert groups == (b * -(-n // group) if group else 0)
        # the launcher's one decision (pointwise.hip pw_plan) on this device's CU count:
        # the library exposes the statistics group (queried above: 32 = Stream128, 64 =
        # Tile256) but no query that tells the 128-row from the 64-row tile
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        mpad = -(-cout // 256) * 256 if cout > 256 else -(-cout // 128) * 128
        big = -(-n // 128) * (mpad // 128) * b
        stream = mpad == 128 and cin <= 256 and cin % 32 == 0 and cout % 32 == 0
        want = ("Stream128" if stream else "Tile256" if mpad % 256 == 0 and big // 2 >= 2 * cus
                else "Tile128" if big >= 2 * cus else "Tile64")
        assert want == form, (want, form, cus)
    if e.family == "conv3d":  # as test_gpu_conv3d.py::test_added_cases_reach_their_forms
        from pcfm import _lib
        b, cin, cout, r = e.shape
        nb = _lib.query("pcfm_conv3d_igemm_cl_workspace_bytes", b, cin, cout, r)
        splits = 1 if nb == 1 else nb // (4 * b * cout * r ** 3)
        assert splits == R.CONV_SPLITS[e.shape]
        if r == 8:  # the window form needs its K / 32 chunks to divide by the splits
            assert ((cin // 32) % splits == 0) == (R.CONV_SHAPES[e.shape] == "window")
    clean_ref = None if e.fast_masks is not None else e.ref(inp)
    out_c = run(ops, e, dev)
    again = run(ops, e, dev)
    for k in out_c:  # deterministic: what the leak assertion stands on
        assert torch.equal(R.bits(out_c[k]), R.bits(again[k])), k
    for label, op, sk in e.injections():
        cls = e.classify(inp, op, sk, clean_ref)
        assert R.nontrivial(cls), label
        with R.poked(dev, op, sk):
            out_s = run(ops, e, dev)
        R.check(f"{e.id}: {label}", out_s, out_c, cls)


# ---------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------
def _weights():
    g = torch.Generator().manual_seed(20)
    return {"pointwise": torch.randn(130, 70, generator=g) / 8,
            "conv3d": torch.randn(128, 64, 3, 3, 3, generator=g) / 40}


# sha256 of the image bits of _weights() under the rounding bf16_bits had before it
# kept NaNs (a plain add of 0x7FFF + lsb to the bits): (not transposed, transposed)
IMAGE_SHA = {
    "pointwise": ("5659954e5bf3ae9c50c7fb905e5dbe52474e9d5edfc2002e8a1225101ea86457",
                  "62f9172385dd3445e1615c6ca04a8f5ab141e60b95a4428471cedd9982e40e8f"),
    "conv3d": ("43195974c91a43209b03b755b21a863d3a02b82b7106f2714d6794b37edf31b2",
               "8dd1a37327b8c6f7cb0924dfd829c81b90038a67bcfd8130ad639fc3146a4e48"),
}


def _image(ops, kind, w, transpose):
    """the bytes the prep kernel writes: the conv image whole; of the pointwise buffer
    (sized for the larger orientation) the [Mpad][Kpad] bf16 hi and lo images"""
    if kind == "conv3d":
        return ops.conv3d_prep_weight(w.to(DEV), transpose)
    m, k = (w.shape[1], w.shape[0]) if transpose else w.shape
    mpad = -(-m // 256) * 256 if m > 256 else -(-m // 128) * 128
    return ops.pointwise_prep_weight(w.to(DEV), transpose)[:2 * mpad * (-(-k // 32) * 32) * 2]


@pytest.mark.parametrize("kind", ["pointwise", "conv3d"])
def test_weight_image_of_finite_weights_is_unchanged(ops, kind):
    w = _weights()[kind]
    got = tuple(hashlib.sha256(_image(ops, kind, w, t).cpu().numpy().tobytes()).hexdigest()
                for t in (False, True))
    assert got == IMAGE_SHA[kind]


@pytest.mark.parametrize("kind", ["pointwise", "conv3d"])
@pytest.mark.parametrize("special", R.KINDS)
def test_weight_image_keeps_a_non_finite_weight(ops, kind, special):
    """Exactly the elements of the injected weight change in the image, and its hi
    element is non-finite: NaN 0x7FFFFFFF used to round to -0.0."""
    w = _weights()[kind]
    for site in [(0,) * w.dim(), tuple(s - 1 for s in w.shape)]:
        for transpose in (False, True):
            clean = w.clone()
            clean[site] = 1.0
            bad = clean.clone()
            bad[site] = R.special(special)
            a = _image(ops, kind, clean, transpose).view(torch.bfloat16)
            b = _image(ops, kind, bad, transpose).view(torch.bfloat16)
            moved = R.bits(a) != R.bits(b)
            assert int(moved.sum()) == 2  # the weight's hi and lo
            assert int((~torch.isfinite(b.float())).sum()) in (1, 2)
            assert bool((~torch.isfinite(b.float()))[moved].any())
            assert bool(torch.isfinite(a.float()).all())


# ---------------------------------------------------------------------------
# the Stream128 K-chunk counts 1, 2, 5, 6, 7 on clean data, the suite's fp64 bar
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.PW_NCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream128_chunk_counts_vs_fp64(ops, shape):
    from pcfm import _lib
    b, cin, cout, n = shape
    assert _lib.query("pcfm_pointwise_bnstats_groups", b, cin, cout, n) == b * -(-n // 32)
    inp = R.pw_make(shape)()
    d = {k: v.to(DEV) for k, v in inp.items()}
    ys = ops.pointwise_forward_bnstats(d["x"], d["w"], d["bias"])
    ref = R.pw_full_ref("pointwise_forward_bnstats", inp, 32)

    def rel(a, r):
        return ((a.double().cpu() - r).abs().max() / r.pow(2).mean().sqrt()).item()
    assert rel(ops.pointwise_forward(d["x"], d["w"], d["bias"]), ref["y"]) < 1e-4
    assert torch.equal(ys[0], ops.pointwise_forward(d["x"], d["w"], d["bias"]))
    # the statistics against float64 statistics of the kernel's own y, at the bounds of
    # tests/test_gpu_pointwise.py::test_pointwise_256_row_shapes
    st, scale = ys[1].double().cpu(), ref["y"].abs().max()
    own = R.pw_group_stats(ys[0].double().cpu(), 32)
    assert torch.allclose(st[..., 0], own[..., 0], rtol=1e-5, atol=1e-6 * scale)
    assert torch.allclose(st[..., 1], own[..., 1], rtol=1e-4, atol=1e-5 * scale ** 2 * 32)
    assert rel(ops.pointwise_backward_data(d["gy"], d["w"]),
               R.pw_full_ref("pointwise_backward_data", inp)["dx"]) < 1e-4
    assert rel(ops.pointwise_backward_weight(d["x"], d["gy"]),
               R.pw_full_ref("pointwise_backward_weight", inp)["dw"]) < 1e-4


# ---------------------------------------------------------------------------
# rows_max_bf16: torch.max(dim=1) on the same bf16 tensor
# ---------------------------------------------------------------------------
def test_rows_max_propagates_like_torch_max(ops):
    from pcfm.layers import max_over_points
    for label, h in R.rows_max_cases():
        h = h.to(DEV)
        val, idx = ops.rows_max_bf16(h)
        ref = torch.max(h, dim=1)
        assert torch.equal(torch.isnan(val), torch.isnan(ref.values)), label
        assert torch.equal(R.bits(val)[~torch.isnan(val)],
                           R.bits(ref.values)[~torch.isnan(val)]), label
        assert torch.equal(idx.long(), ref.indices), label
        hh = h.clone().requires_grad_(True)
        gv = torch.arange(1, val.numel() + 1, device=DEV).view_as(val).to(val.dtype)
        max_over_points(hh).backward(gv)
        exp = torch.zeros_like(h).scatter_(1, ref.indices.unsqueeze(1), gv.unsqueeze(1))
        assert torch.equal(hh.grad, exp), label


# ---------------------------------------------------------------------------
# the fused update with a scaler: a NaN gradient skips the step like an inf
# (mirrors tests/test_gpu_optim.py::test_fused_adamw_skips_on_inf_and_backs_off)
# ---------------------------------------------------------------------------
OPT_SHAPES = [(256, 128, 3, 3, 3), (7,), (3,), (513, 9), (4096,), (4097,), (64, 64), (1,)]


class _Scaler:
    """The GradScaler attributes FusedAdamWEMA.step reads and updates."""

    def __init__(self, scale):
        self._scale = torch.full((1,), float(scale), device=DEV)
        self._growth_tracker = torch.zeros(1, dtype=torch.int32, device=DEV)
        self._growth_factor, self._backoff_factor, self._growth_interval = 2.0, 0.5, 2000

    def is_enabled(self):
        return True


@pytest.mark.parametrize("where", [(3, (0, 0)), (7, (0,)), (5, (4096,))],
                         ids=["nan_513x9", "nan_1_element", "nan_4097_elements"])
def test_fused_adamw_skips_on_nan_and_backs_off(where):
    from pcfm.optim import FusedAdamWEMA
    g = torch.Generator(device=DEV).manual_seed(2)
    ps = [torch.randn(s, device=DEV, generator=g) * 0.1 for s in OPT_SHAPES]
    shadows = [p.clone() + 0.01 for p in ps]
    fused = FusedAdamWEMA([{"params": ps, "lr": 1e-3, "weight_decay": 1e-4}],
                          ema_shadows=dict(zip(ps, shadows)), ema_decay=0.9)
    scaler = _Scaler(2.0 ** 16)
    before = [p.clone() for p in ps]
    sh_before = [s.clone() for s in shadows]
    for p in ps:
        p.grad = torch.randn(p.shape, device=DEV, generator=g)
    i, site = where
    assert OPT_SHAPES[i] in ((513, 9), (1,), (4097,))
    ps[i].grad[site] = float("nan")
    fused.step(1.0, scaler)
    for a, b in zip(ps, before):
        assert torch.equal(a, b)  # update skipped
    for s, s0, p in zip(shadows, sh_before, before):  # the EMA still moves
        torch.testing.assert_close(s, s0 * 0.9 + 0.1 * p, rtol=1e-6, atol=1e-7)
    assert float(fused.steps.max()) == 0.0 and float(fused.found_inf) == 1.0
    assert float(scaler._scale) == 2.0 ** 15
    for p in ps:
        p.grad = torch.randn(p.shape, device=DEV, generator=g)
    fused.step(1.0, scaler)
    assert float(fused.steps.min()) == 1.0 and float(fused.found_inf) == 0.0
    assert not all(torch.equal(a, b) for a, b in zip(ps, before))


# ---------------------------------------------------------------------------
# the voxel convolution's occupancy forms (occ= masks, vlists= voxel lists) against
# the dense form on a voxelized grid (exact zero outside the occupied voxels, as in
# tests/test_gpu_pvconv.py::test_conv_occupancy_skipping_is_exact), a special value at
# an occupied voxel: every element bit-equal to the dense form's or non-finite in both
# ---------------------------------------------------------------------------
def _same_or_both_nonfinite(a, b):
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    return bool(torch.equal(fa, fb)) and bool(torch.equal(R.bits(a)[fa], R.bits(b)[fa]))


@pytest.mark.parametrize("cin,cout,r", [(128, 128, 32), (128, 256, 16)])
def test_conv_occupancy_forms_agree_with_the_dense_form(ops, cin, cout, r):
    b, n = 2, 3000
    g = torch.Generator(device=DEV).manual_seed(r + cin)
    vox = torch.randint(0, r, (b, 3, n), device=DEV, generator=g, dtype=torch.int32)
    grid, ind, cnt = ops.avg_voxelize_forward(torch.randn(b, cin, n, device=DEV, generator=g), vox, r)
    occ, vl = ops.conv3d_occupancy(cnt, r), ops.conv3d_vlists(cnt, r)
    assert occ is not None and vl is not None
    w = torch.randn(cout, cin, 3, 3, 3, device=DEV, generator=g) * 0.05
    bias = torch.randn(cout, device=DEV, generator=g)
    img, imgt = ops.conv3d_prep_weight(w, False), ops.conv3d_prep_weight(w, True)
    dy = torch.randn(b, cout, r ** 3, device=DEV, generator=g)
    occupied = cnt.view(b, 1, -1) > 0
    # occupied voxels: the first point's, the last point's (the other cloud)
    sites = [(0, 0, int(ind[0, 0])), (b - 1, cin - 1, int(ind[b - 1, n - 1]))]
    for kind in R.KINDS:
        for bi, ci, v in sites:
            x = grid.clone()
            x[bi, ci, v] = R.special(kind).to(DEV)
            xs = ops.conv3d_split(x.view(b, cin, r, r, r))
            y0 = ops.conv3d_igemm_split(xs, img, bias, b, cin, cout, r, "conv3d_fwd")
            assert not bool(torch.isfinite(y0).all()) and bool(torch.isfinite(y0).any())
            y1 = ops.conv3d_igemm_split(xs, img, bias, b, cin, cout, r, "conv3d_fwd", occ=occ,
                                        occ_mode=1)
            y2 = ops.conv3d_igemm_split(xs, img, bias, b, cin, cout, r, "conv3d_fwd", occ=occ,
                                        occ_mode=1, vlists=vl, cnt=cnt)
            assert _same_or_both_nonfinite(y1, y0), (kind, "occ forward")
            assert _same_or_both_nonfinite(y2, y0), (kind, "list forward")
            d = dy.clone()
            d[bi, min(ci, cout - 1), v] = R.special(kind).to(DEV)
            gys = ops.conv3d_split(d.view(b, cout, r, r, r))
            dx0 = ops.conv3d_igemm_split(gys, imgt, None, b, cout, cin, r, "conv3d_bwd_data")
            dx1 = ops.conv3d_igemm_split(gys, imgt, None, b, cout, cin, r, "conv3d_bwd_data",
                                         occ=occ, occ_mode=2)
            dx2 = ops.conv3d_igemm_split(gys, imgt, None, b, cout, cin, r, "conv3d_bwd_data",
                                         occ=occ, occ_mode=2, vlists=vl, cnt=cnt)
            m = occupied.expand(b, cin, r ** 3)  # the voxels both forms define
            for name, dx in (("occ", dx1), ("list", dx2)):
                assert _same_or_both_nonfinite(dx.view(b, cin, -1)[m], dx0.view(b, cin, -1)[m]), (
                    kind, name + " backward-data")
            # weight gradient, special in x (clean gradient): full agreement
            gyc = ops.conv3d_split(dy.view(b, cout, r, r, r))
            dw0 = ops.conv3d_wgrad_split(xs, gyc, b, cin, cout, r)
            dw1 = ops.conv3d_wgrad_split(xs, gyc, b, cin, cout, r, occ=occ)
            assert not bool(torch.isfinite(dw0).all())
            assert _same_or_both_nonfinite(dw1, dw0), (kind, "occ weight gradient, x")
            # special in the gradient (clean x): the dense form multiplies it with the
            # exact zeros of unoccupied neighbours (0 * inf = NaN), the occupancy form
            # skips those steps (DESIGN.md "Non-finite values").  Expected: nothing the
            # dense form has finite moves, the occupancy form's non-finite set is inside
            # the dense one, and no output-channel row loses its non-finite altogether.
            xc = ops.conv3d_split(grid.view(b, cin, r, r, r))
            dw0 = ops.conv3d_wgrad_split(xc, gys, b, cin, cout, r)
            dw1 = ops.conv3d_wgrad_split(xc, gys, b, cin, cout, r, occ=occ)
            f0, f1 = torch.isfinite(dw0), torch.isfinite(dw1)
            assert torch.equal(R.bits(dw1)[f0], R.bits(dw0)[f0]), (kind, "occ weight gradient, gy")
            assert bool((f1 | ~f0).all())
            assert torch.equal((~f0).flatten(1).any(1), (~f1).flatten(1).any(1))


# ---------------------------------------------------------------------------
# end to end: one PVConv block, fused path against the module path on the CPU
# (torch + pcfm.cpu_ops), with one inf in the input features; then a Trainer step
# ---------------------------------------------------------------------------
def test_pvconv_block_gradients_carry_the_inf(ops):
    import copy
    import modules.pvconv as pv
    torch.manual_seed(8)
    cin, cout, r, n = 64, 128, 8, 3000
    mod = pv.PVConv(cin, cout, 3, r, with_se=True, normalize=True).train()
    ref = copy.deepcopy(mod)
    mod = mod.to(DEV)
    feats = torch.randn(2, cin, n)
    feats[0, 3, 100] = float("inf")
    coords = torch.rand(2, 3, n) * 2 - 1  # coordinates stay finite
    gy = torch.randn(2, cout, n)
    grads = {}
    for name, m, dev in (("fused", mod, DEV), ("module", ref, "cpu")):
        f = feats.to(dev).requires_grad_(True)
        out, _ = m((f, coords.to(dev)))
        out.backward(gy.to(dev))
        grads[name] = [("input", f.grad.cpu())] + [(k, p.grad.cpu())
                                                   for k, p in m.named_parameters()]
        if name == "module":
            assert not bool(torch.isfinite(out).all())
    assert any(not bool(torch.isfinite(g).all()) for _, g in grads["module"])
    for (k, a), (_, b) in zip(grads["fused"], grads["module"]):
        missing = ~torch.isfinite(b) & torch.isfinite(a)
        assert not bool(missing.any()), (k, int(missing.sum()), int((~torch.isfinite(b)).sum()))


def test_trainer_step_with_an_inf_feature_is_skipped():
    from pcfm.train import TrainConfig, Trainer, synthetic_batch
    tr = Trainer(TrainConfig(batch_size=2, num_points=1024, steps_per_epoch=4, epochs=1,
                             tunableop=False, miopen_find=False, device_rng=False), DEV)
    tr.train_mode()
    batch = synthetic_batch(tr.cfg, DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    batch["train_rgb"][0, 5, 1] = float("inf")  # a feature; train_points (coordinates) untouched
    assert tr.cfg.amp and tr.scaler.is_enabled()
    before = [p.detach().clone() for p in tr._clip_params]
    scale = tr.scaler.get_scale()
    torch.manual_seed(5)
    tr.step(batch, epoch=201)
    for p, p0 in zip(tr._clip_params, before):
        assert torch.equal(p.detach(), p0)
    assert tr.scaler.get_scale() == scale / 2
