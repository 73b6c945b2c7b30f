"""The C ABI's memory contract (include/pcfm.h, top of file), checked by address
rather than by value: every launching entry point is run

  a. plain, twice (real allocator) -- the outputs to compare against, and
     whether the op is deterministic;
  b. under tests/guard_alloc.py -- inputs, outputs and workspaces inside
     guarded arenas, float outputs pre-filled with a NaN pattern: every guard
     intact (nothing written outside the stated extents, every
     *_workspace_bytes() large enough), no poison left in an output, outputs
     equal to the plain run's (an over-read that is used meets NaN / index 0);
  c. stale -- the arenas of a call on *another* input of the same shape handed
     to the call on the real input, workspaces and integer outputs included:
     outputs equal to the plain run's (nothing depends on prior contents).

Outputs are compared bit for bit.  An op whose two plain runs differ must
declare the tolerance tests/test_gpu_ops.py states for atomics-ordered sums:
only the Chamfer backward does (the scatters sort), every other output of every
row compares exactly.

A row's id names the kernel form its shape takes, read from the dispatch code
(plan_gather in csrc/rows.hpp, pw_plan / pw_wgrad_plan in csrc/pointwise.hip,
conv3_wgrad_splits, glds_splits and the list choice in csrc/conv3d.hip).
"""
import contextlib

import pytest
import torch

import guard_alloc as ga

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from pcfm import _lib, ops
    _lib.load()
    assert torch.cuda.is_available()
    return ops


def G(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rn(g, *s):
    return torch.randn(*s, device=DEV, generator=g)


def ru(g, *s):
    return torch.rand(*s, device=DEV, generator=g)


# --------------------------------------------------------------------------
# the row runner
# --------------------------------------------------------------------------
class Row:
    def __init__(self, rid, build, call, entries, tol=None):
        self.id, self.build, self.call, self.entries, self.tol = rid, build, call, entries, tol


def _map(d, f):
    out = {}
    for k, v in d.items():
        if isinstance(v, torch.Tensor):
            out[k] = f(v)
        elif isinstance(v, (list, tuple)) and v and all(isinstance(t, torch.Tensor) for t in v):
            out[k] = [f(t) for t in v]
        else:
            out[k] = v
    return out


def _args(inp, alloc):
    """The row's inputs as fresh copies (alloc None) or inside guarded arenas; "P"
    places an intermediate the call wants guarded as an input (identity when plain)."""
    d = _map(inp, torch.clone if alloc is None else alloc.guarded)
    d["P"] = (lambda t: t) if alloc is None else alloc.guarded
    return d


def _as_bf16(P, buf):
    """A split operand / weight image (opaque uint8 of bf16 pairs) placed as a bf16
    input: its guards are NaN, so an unmasked read before the first or after the
    last voxel row that is used poisons the answer."""
    return P(buf.view(torch.bfloat16)).view(torch.uint8)


_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    t = t.detach().contiguous()
    return t.view(_INT[t.element_size()]) if t.is_floating_point() else t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@contextlib.contextmanager
def recorder():
    """The entry points reached through pcfm._lib.call while active."""
    from pcfm import _lib
    names, real = [], _lib.call

    def call(name, *args):
        names.append(name)
        return real(name, *args)
    _lib.call = call
    try:
        yield names
    finally:
        _lib.call = real


def _outs(res):
    return [t for t in res if t is not None]


def _compare(what, row, got, plain, det):
    assert len(got) == len(plain), (row.id, what)
    for k, (a, p, d) in enumerate(zip(got, plain, det)):
        if d:
            assert _same(a, p), f"{row.id}: {what} run, output {k} differs from the plain run " \
                                f"({int((_bits(a) != _bits(p)).sum())} of {p.numel()} elements)"
        else:
            rtol, atol = row.tol
            scale = max(1.0, float(p.abs().max())) if p.numel() else 1.0
            torch.testing.assert_close(a, p, rtol=rtol, atol=atol * scale,
                                       msg=lambda m: f"{row.id}: {what} run, output {k}: {m}")


def run_row(row, report):
    inp, other = row.build(0), row.build(1)
    with recorder() as names:
        plain = _outs(row.call(_args(inp, None)))
        again = _outs(row.call(_args(inp, None)))
        det = [_same(a, b) for a, b in zip(plain, again)]
        assert all(det) or row.tol is not None, \
            f"{row.id}: two plain runs differ in outputs {[k for k, d in enumerate(det) if not d]} " \
            "and the op claims no atomics-ordered sum"
        # b. guarded
        with ga.GuardedAlloc() as g:
            got = _outs(row.call(_args(inp, g)))
        g.report.assert_guards_intact()
        left = [ga.poison_left(a, p) for a, p in zip(got, plain)]
        assert not any(left), f"{row.id}: poison left in outputs {left}\n{g.report.describe()}"
        _compare("guarded", row, got, plain, det)
        # c. stale: the arenas of a call on another input of the same shape
        with ga.GuardedAlloc() as first:
            row.call(_args(other, first))
        first.report.assert_guards_intact()
        with ga.GuardedAlloc(stale=first) as st:
            stale = _outs(row.call(_args(inp, st)))
        st.report.assert_guards_intact()
        _compare("stale", row, stale, plain, det)
    missing = set(row.entries) - set(names)
    assert not missing, f"{row.id}: declared entry points not reached: {sorted(missing)}"
    report(f"abi_contract/{row.id}", {
        "entries": sorted(set(names)), "compare": "bit-exact" if all(det) else f"tol {row.tol}",
        "arenas": len(g.report.arenas), "workspace_bytes": g.report.workspace_bytes()})


# --------------------------------------------------------------------------
# gather / scatter chain
# --------------------------------------------------------------------------
def vox_row(b, c, n, r, form):
    def build(seed):
        g = G(100 + seed)
        hi = r if seed == 0 else max(1, (r + 1) // 2)      # the other cloud: another occupancy
        return {"feat": rn(g, b, c, n),
                "coords": torch.randint(0, hi, (b, 3, n), device=DEV, generator=g,
                                        dtype=torch.int32),
                "gy": rn(g, b, c, r ** 3), "add": rn(g, b, c, n)}

    def call(d):
        from pcfm import ops
        out, ind, cnt = ops.avg_voxelize_forward(d["feat"], d["coords"], r)
        gx = ops.avg_voxelize_backward(d["gy"], ind, cnt)
        gxa = ops.avg_voxelize_backward_add(d["gy"], ind, cnt, d["add"])
        plan = ops.avg_voxelize_plan(d["coords"], r)
        outp = ops.avg_voxelize_forward_planned(d["feat"], plan)
        return out, ind, cnt, gx, gxa, plan.ind, plan.cnt, outp
    return Row(f"voxelize-b{b}c{c}n{n}r{r}-{form}", build, call,
               ["pcfm_avg_voxelize_fwd", "pcfm_avg_voxelize_bwd", "pcfm_avg_voxelize_bwd_add",
                "pcfm_avg_voxelize_plan", "pcfm_avg_voxelize_fwd_planned"])


def devox_row(b, c, n, r, form, outside=False, bn=True):
    def build(seed):
        g = G(200 + seed)
        pts = ru(g, b, 3, n) * (r - 1)
        if n >= 8:                                   # integer coordinates, the boundary r-1
            pts[:, :, : n // 8] = torch.round(pts[:, :, : n // 8])
            pts[:, :, -1] = r - 1
        if outside and n >= 8:                       # ~a quarter of the points outside the volume
            k = n // 4
            pts[:, :, n // 8: n // 8 + k] = ru(g, b, 3, k) * (r + 3) - 1.5
        return {"pts": pts.contiguous(), "grid": rn(g, b, c, r ** 3), "scale": ru(g, b, c),
                "add": rn(g, b, c, n), "gy": rn(g, b, c, n), "mean": rn(g, c) * 0.1,
                "invstd": ru(g, c) + 0.5, "w": ru(g, c) + 0.5, "bias": rn(g, c) * 0.1}

    def call(d):
        from pcfm import ops
        o, i, w = ops.trilinear_devoxelize_forward(r, True, d["pts"], d["grid"])
        oe = ops.trilinear_devoxelize_forward(r, False, d["pts"], d["grid"])[0]
        o2, i2, w2 = ops.trilinear_devoxelize_scale_add(r, True, d["pts"], d["grid"], d["scale"],
                                                       d["add"])
        res = [o, i, w, oe, o2, i2, w2]
        if bn:
            res += ops.trilinear_devoxelize_bn_scale_add(
                r, True, d["pts"], d["grid"], d["mean"], d["invstd"], d["w"], d["bias"], 0.1,
                d["scale"], d["add"],
                # (an empty add has no address: its BatchNorm operands would be refused)
                add_bn=(d["mean"], d["invstd"], d["w"], d["bias"], 0.0) if n else None)
        res.append(ops.trilinear_devoxelize_backward(d["gy"], i, w, r))
        plan = ops.trilinear_devoxelize_backward_plan(i, w, r)
        res.append(ops.trilinear_devoxelize_backward_planned(d["gy"], plan))
        return res
    ent = ["pcfm_trilinear_devoxelize_fwd", "pcfm_trilinear_devoxelize_scale_add_fwd",
           "pcfm_trilinear_devoxelize_bwd", "pcfm_trilinear_devoxelize_bwd_plan",
           "pcfm_trilinear_devoxelize_bwd_planned"]
    if bn:
        ent.append("pcfm_trilinear_devoxelize_bn_scale_add_fwd")
    return Row(f"devoxelize-b{b}c{c}n{n}r{r}-{form}", build, call, ent)


def group_row(b, m, n, u, c=5):
    def build(seed):
        g = G(300 + seed)
        pts, ctr = ru(g, b, 3, n), ru(g, b, 3, m)
        if n > 0:
            ctr[:, :, : m // 4] = pts[:, :, : m // 4]      # centers on points: d2 == 0 hits
        return {"pts": pts, "ctr": ctr, "feat": rn(g, b, c, n), "gy": rn(g, b, c, m, u)}

    def call(d):
        from pcfm import ops
        idx = ops.ball_query(d["ctr"], d["pts"], 0.3, u)
        if n == 0:
            return [idx]
        return [idx, ops.grouping_forward(d["feat"], idx), ops.grouping_backward(d["gy"], idx, n)]
    ent = ["pcfm_ball_query"] + (["pcfm_grouping_fwd", "pcfm_grouping_bwd"] if n else [])
    return Row(f"ballquery-grouping-b{b}m{m}n{n}u{u}", build, call, ent)


# --------------------------------------------------------------------------
# pointwise GEMMs
# --------------------------------------------------------------------------
def pw_row(b, cin, cout, n, form, fparts, bparts, bnstats=False):
    """fparts: the forward's input parts (all but the last % 32); bparts: the
    backward-data's output parts (all but the last % 128)."""
    def build(seed):
        g = G(400 + seed)
        return {"x": rn(g, b, cin, n), "w": rn(g, cout, cin) * 0.1, "bias": rn(g, cout),
                "gy": rn(g, b, cout, n), "bb": rn(g, b, cout), "gamma": ru(g, cout) + 0.5,
                "beta": rn(g, cout) * 0.1, "rm": rn(g, cout), "rv": ru(g, cout) + 0.5,
                "nbt": torch.zeros((), dtype=torch.int64, device=DEV)}

    def call(d):
        from pcfm import ops
        x, w, gy = d["x"], d["w"], d["gy"]
        res = [ops.pointwise_forward(x, w, d["bias"]), ops.pointwise_forward(x, w, None),
               ops.pointwise_backward_data(gy, w), ops.pointwise_backward_weight(x, gy)]
        xs = [d["P"](t.contiguous()) for t in torch.split(x, fparts, dim=1)]
        res.append(ops.pointwise_forward_parts(xs, w, d["bias"]))
        res.append(ops.pointwise_forward_parts(xs, w, d["bb"], bias_per_batch=True))
        res += ops.pointwise_backward_data_parts(gy, w, bparts)
        res.append(ops.pointwise_backward_weight_parts(xs, gy))
        st = ops.pointwise_forward_bnstats(x, w, d["bias"])
        assert (st is not None) == bnstats, "bnstats path: not what the row declares"
        if st is not None:
            y, stats = st
            assert stats.shape[0] == cout
            res += [y, stats]
        if st is not None and n % 4 == 0:       # the BatchNorm kernels need n % 4 == 0
            res += ops.bn_act_forward_parts(y, stats, d["gamma"], d["beta"], 1e-5, 0.0, 0.1,
                                            d["rm"], d["rv"], d["nbt"])
            res += ops.bn_forward_stats(y, 1e-5, 0.1, d["rm"], d["rv"], d["nbt"], parts=stats)
            res += [d["rm"], d["rv"], d["nbt"]]
        return res
    ent = ["pcfm_pointwise_prep_weight", "pcfm_pointwise_gemm", "pcfm_pointwise_wgrad",
           "pcfm_pointwise_gemm_parts", "pcfm_pointwise_wgrad_parts"]
    if bnstats:
        ent += ["pcfm_pointwise_gemm_bnstats"]
        if n % 4 == 0:
            ent += ["pcfm_bn_act_fwd_parts", "pcfm_bn_fwd_stats"]
    return Row(f"pointwise-b{b}cin{cin}cout{cout}n{n}-{form}", build, call, ent)


# --------------------------------------------------------------------------
# voxel convolutions
# --------------------------------------------------------------------------
def conv_row(b, cin, cout, r, form, fwd_only=False):
    def build(seed):
        g = G(500 + seed)
        return {"x": rn(g, b, cin, r, r, r), "w": rn(g, cout, cin, 3, 3, 3) * 0.05,
                "bias": rn(g, cout), "gy": rn(g, b, cout, r, r, r)}

    def call(d):
        from pcfm import ops
        x, w, gy = d["x"], d["w"], d["gy"]
        P = d["P"]
        xs = _as_bf16(P, ops.conv3d_split(x))
        img = _as_bf16(P, ops.conv3d_prep_weight(w, False))
        res = [xs, img, ops.conv3d_igemm_split(xs, img, d["bias"], b, cin, cout, r, "conv3d_fwd"),
               ops.conv3d_forward(x, w, d["bias"])]
        if not fwd_only:
            gys = _as_bf16(P, ops.conv3d_split(gy))
            imgt = _as_bf16(P, ops.conv3d_prep_weight(w, True))
            res += [gys, imgt,
                    ops.conv3d_igemm_split(gys, imgt, None, b, cout, cin, r, "conv3d_bwd_data"),
                    ops.conv3d_wgrad_split(xs, gys, b, cin, cout, r),
                    ops.conv3d_backward_data(gy, w), ops.conv3d_backward_weight(x, gy)]
        return res
    ent = ["pcfm_conv3d_split", "pcfm_conv3d_prep_weight", "pcfm_conv3d_igemm_cl",
           "pcfm_conv3d_igemm"]
    if not fwd_only:
        ent += ["pcfm_conv3d_wgrad_cl", "pcfm_conv3d_wgrad"]
    return Row(f"conv3d-b{b}cin{cin}cout{cout}r{r}-{form}", build, call, ent)


def _cloud_grid(ops, b, c, r, n, seed, empty=None):
    """_voxelized of tests/test_gpu_pvconv.py with another cloud per seed (seed 1:
    a spherical shell -- another occupancy pattern) and, with `empty`, one batch
    element without a single point."""
    g = G(seed)
    pts = rn(g, b, 3, n)
    if seed % 2:
        pts = pts / pts.norm(dim=1, keepdim=True)
    c0 = pts - pts.mean(2, keepdim=True)
    unit = c0 / (2 * c0.norm(dim=1, keepdim=True).max(2, keepdim=True).values + 1e-6) + 0.5
    vox = torch.round(torch.clamp(unit * r, 0, r - 1)).int().contiguous()
    grid, _, cnt = ops.avg_voxelize_forward(rn(g, b, c, n), vox, r)
    if empty is not None:
        grid[empty] = 0.0
        cnt[empty] = 0
    return grid.view(b, c, r, r, r).contiguous(), cnt


def conv_sparse_row(b, c, r, form, empty=None):
    """Occupancy and voxel-list forms over a voxelized grid.  The list form runs
    where glds_splits(b, cin, cout, r) == 1: at r = 32, 128 -> 128 channels, from
    b = 2 on (b r^3 / 256 tiles > half the CUs)."""
    def build(seed):
        from pcfm import ops
        grid, cnt = _cloud_grid(ops, b, c, r, 3000, 600 + seed, empty)
        g = G(650 + seed)
        gy = rn(g, b, c, r, r, r)
        return {"x": grid, "cnt": cnt, "w": rn(g, c, c, 3, 3, 3) * 0.05, "bias": rn(g, c),
                "gy": gy}

    def call(d):
        from pcfm import ops
        cnt = d["cnt"]
        occ = ops.conv3d_occupancy(cnt, r)
        vl = ops.conv3d_vlists(cnt, r)
        P = d["P"]
        xs, gys = _as_bf16(P, ops.conv3d_split(d["x"])), _as_bf16(P, ops.conv3d_split(d["gy"]))
        img = _as_bf16(P, ops.conv3d_prep_weight(d["w"], False))
        imgt = _as_bf16(P, ops.conv3d_prep_weight(d["w"], True))
        a = (b, c, c, r)
        y_occ = ops.conv3d_igemm_split(xs, img, d["bias"], *a, "conv3d_fwd", occ=occ, occ_mode=1)
        y_lst = ops.conv3d_igemm_split(xs, img, d["bias"], *a, "conv3d_fwd", occ_mode=1,
                                       vlists=vl, cnt=cnt)
        dx_occ = ops.conv3d_igemm_split(gys, imgt, None, *a, "conv3d_bwd_data", occ=occ,
                                        occ_mode=2)
        dx_lst = ops.conv3d_igemm_split(gys, imgt, None, *a, "conv3d_bwd_data", occ_mode=2,
                                        vlists=vl, cnt=cnt)
        dw = ops.conv3d_wgrad_split(xs, gys, *a)
        dw_occ = ops.conv3d_wgrad_split(xs, gys, *a, occ=occ)
        assert torch.equal(dw, dw_occ)      # the skipped products are exact zeros
        return [occ, y_occ, y_lst, dx_occ, dx_lst, dw, dw_occ]
    return Row(f"conv3d-sparse-b{b}c{c}r{r}-{form}", build, call,
               ["pcfm_conv3d_occupancy", "pcfm_conv3d_vlist", "pcfm_conv3d_igemm_cl_occ",
                "pcfm_conv3d_igemm_cl_list", "pcfm_conv3d_wgrad_cl_occ", "pcfm_conv3d_wgrad_cl"])


# --------------------------------------------------------------------------
# normalisation and head kernels
# --------------------------------------------------------------------------
def _bn_inputs(g, shape):
    c = shape[1]
    return {"x": rn(g, *shape) * 2.0 + 1.0, "dz": rn(g, *shape), "gamma": ru(g, c) + 0.5,
            "beta": ru(g, c) - 0.5, "rm": rn(g, c), "rv": ru(g, c) + 0.5,
            "nbt": torch.zeros((), dtype=torch.int64, device=DEV)}


def bn_row(shape, slope):
    def build(seed):
        return _bn_inputs(G(700 + seed), shape)

    def call(d):
        from pcfm import ops
        x = d["x"]
        y, mean, invstd = ops.bn_act_forward(x, d["gamma"], d["beta"], 1e-5, slope, 0.1, d["rm"],
                                             d["rv"], d["nbt"])
        m2, iv2 = ops.bn_forward_stats(x, 1e-5, 0.1, d["rm"], d["rv"], d["nbt"])
        rowmean, m3, iv3 = ops.bn_act_forward_rowmean(x, d["gamma"], d["beta"], 1e-5, slope, 0.1,
                                                      d["rm"], d["rv"], d["nbt"])
        back = ops.bn_act_backward(d["dz"], x, d["gamma"], d["beta"], mean, invstd, slope,
                                   want_dbias_in=True)
        back2 = ops.bn_act_backward(d["dz"], x, d["gamma"], d["beta"], mean, invstd, slope)
        return [y, mean, invstd, m2, iv2, rowmean, m3, iv3, *back, *back2, d["rm"], d["rv"],
                d["nbt"]]
    return Row(f"bn-{'x'.join(map(str, shape))}", build, call,
               ["pcfm_bn_act_fwd", "pcfm_bn_fwd_stats", "pcfm_bn_act_fwd_rowmean",
                "pcfm_bn_act_bwd"])


def bn_split_row(b, c, r, slope):
    """The forms that write / read conv split operands (c, r^3 multiples of 64)."""
    def build(seed):
        g = G(720 + seed)
        d = _bn_inputs(g, (b, c, r, r, r))
        d.update({"se": ru(g, b, c), "dmv": rn(g, b, c) * 1e-3})
        return d

    def call(d):
        from pcfm import ops
        x, ga_, be = d["x"], d["gamma"], d["beta"]
        ys, mean, invstd = ops.bn_act_forward_split(x, ga_, be, 1e-4, slope, 0.1, d["rm"],
                                                    d["rv"], d["nbt"])
        res = [ys, mean, invstd]
        res += ops.bn_act_backward_split(d["dz"], x, ga_, be, mean, invstd, slope,
                                         want_dbias_in=True)
        rowstats = ops.bn_se_backward_stats(d["dz"], x, mean, invstd, ga_, be, slope)
        res.append(rowstats)
        res += ops.bn_se_backward_apply_split(d["dz"], x, mean, invstd, ga_, be, d["se"],
                                              d["dmv"], rowstats, slope, want_dbias_in=True)
        return res + [d["rm"], d["rv"], d["nbt"]]
    return Row(f"bn-split-b{b}c{c}r{r}", build, call,
               ["pcfm_bn_act_fwd_split", "pcfm_bn_act_bwd_split", "pcfm_bn_se_bwd_stats",
                "pcfm_bn_se_bwd_apply_split"])


def gn_row(b, c, n, groups, bnin=True):
    def build(seed):
        g = G(740 + seed)
        return {"x": rn(g, b, c, n) * 1.5 + 2.0, "dout": rn(g, b, c, n), "w": ru(g, c) + 0.5,
                "bias": ru(g, c) - 0.5, "gamma": rn(g, b, c) * 0.3, "beta": rn(g, b, c) * 0.3,
                "bw": ru(g, c) + 0.5, "bb": ru(g, c) - 0.5}

    def call(d):
        from pcfm import ops
        x, w, bias, dout = d["x"], d["w"], d["bias"], d["dout"]
        out, mean, rstd = ops.gn_film_res_forward(x, w, bias, d["gamma"], d["beta"], groups, 1e-6)
        res = [out, mean, rstd]
        res += ops.gn_film_res_backward(dout, x, w, bias, d["gamma"], mean, rstd, groups)
        o2, m2, r2 = ops.gn_silu_forward(x, w, bias, groups, 1e-6)
        res += [o2, m2, r2, *ops.gn_silu_backward(dout, x, w, bias, m2, r2, groups)]
        if bnin:
            bm = x.mean(dim=(0, 2))
            bi = torch.rsqrt(x.var(dim=(0, 2), unbiased=False) + 1e-5)
            o3, m3, r3 = ops.gn_film_res_forward_bnin(x, bm, bi, d["bw"], d["bb"], 0.0, w, bias,
                                                      d["gamma"], d["beta"], groups, 1e-6)
            dz, dw, db, dg, dbe, part = ops.gn_film_res_backward_bnin(
                dout, x, bm, bi, d["bw"], d["bb"], 0.0, w, bias, d["gamma"], m3, r3, groups)
            res += [o3, m3, r3, dz, dw, db, dg, dbe, part]
            res += ops.bn_act_backward_parts(dz, x, d["bw"], d["bb"], bm, bi, part, 0.0,
                                             want_dbias_in=True)
        return res
    ent = ["pcfm_gn_film_res_fwd", "pcfm_gn_film_res_bwd", "pcfm_gn_silu_fwd", "pcfm_gn_silu_bwd"]
    if bnin:
        ent += ["pcfm_gn_film_res_fwd_bnin", "pcfm_gn_film_res_bwd_bnin",
                "pcfm_bn_act_bwd_apply_parts"]
    return Row(f"gn-b{b}c{c}n{n}g{groups}", build, call, ent)


def se_rows_row(b, c, h, rows, length):
    """SE3d's MLP, and the small row kernels: rows_dot, rows_affine (in place)."""
    def build(seed):
        g = G(760 + seed)
        return {"m": rn(g, b, c), "w1": rn(g, h, c), "w2": rn(g, c, h), "ds": rn(g, b, c),
                "a": rn(g, rows, length), "b2": rn(g, rows, length), "s": rn(g, rows),
                "t": rn(g, rows)}

    def call(d):
        from pcfm import ops
        s, hid = ops.se_mlp_forward(d["m"], d["w1"], d["w2"])
        res = [s, hid, *ops.se_mlp_backward(d["m"], hid, s, d["ds"], d["w1"], d["w2"], 0.5)]
        res += [ops.rows_dot(d["a"], d["b2"], 0.25), ops.rows_dot(d["a"], None)]
        res.append(ops.rows_affine_(d["a"], d["s"], d["t"]))
        res.append(ops.rows_affine_(d["b2"], d["s"], None))
        return res
    return Row(f"se-mlp-b{b}c{c}h{h}-rows{rows}x{length}", build, call,
               ["pcfm_se_mlp_fwd", "pcfm_se_mlp_bwd", "pcfm_rows_dot", "pcfm_rows_affine"])


def head_row(b, n, w):
    """The trunk's FiLM block kernels, rows = b * n (a 32-row block is ragged
    when rows % 32 != 0), and the bf16 weight gradient / column sum / row max /
    time gate over the same rows."""
    rows = b * n

    def build(seed):
        g = G(780 + seed)
        return {"gamma": 1.0 + 0.2 * rn(g, w), "beta": 0.2 * rn(g, w),
                "sp1": (1.0 + 0.1 * rn(g, b, w)).bfloat16(), "sh": (0.1 * rn(g, b, w)).bfloat16(),
                "h16": rn(g, rows, w).bfloat16(), "hb": rn(g, b, w), "uprev": rn(g, rows, w),
                "gprev": rn(g, rows, w).bfloat16(), "dhn": rn(g, rows, w),
                "da": rn(g, rows, w).bfloat16(), "x16": rn(g, rows, 6).bfloat16(),
                "h3": rn(g, b, n, 6).bfloat16(), "head": rn(g, b, 64, n), "glb": rn(g, b, 64),
                "alpha": ru(g, b), "dout": rn(g, b, n, 64)}

    def call(d):
        from pcfm import ops
        ga_, be, sp1, sh = d["gamma"], d["beta"], d["sp1"], d["sh"]
        res = []
        # first block (h16 + per-batch bias), then an inner block (uprev, gprev)
        u, a, mean, rstd = ops.head_film_fwd(d["h16"], None, None, ga_, be, sp1, sh, n, 1e-5,
                                             hbias=d["hb"])
        res += [u, a, mean, rstd]
        res += ops.head_film_bwd(d["dhn"], d["da"], None, d["h16"], None, None, mean, rstd, ga_,
                                 be, sp1, n, want_dh=False, hbias=d["hb"], shift=sh)[1:]
        u2, a2, mean2, rstd2 = ops.head_film_fwd(None, d["uprev"], d["gprev"], ga_, be, sp1, sh,
                                                 n, 1e-5)
        res += [u2, a2, mean2, rstd2]
        res += ops.head_film_bwd(d["dhn"], d["da"], u2, None, d["uprev"], d["gprev"], mean2,
                                 rstd2, ga_, be, sp1, n, want_dh=True)
        res.append(ops.head_silu_fwd(d["uprev"], d["gprev"], n))
        res += ops.head_silu_bwd(d["da"], d["uprev"], d["gprev"], n)
        res.append(ops.rows_wgrad_bf16(d["da"], d["x16"]))
        res.append(ops.rows_wgrad_bf16(d["da"], d["gprev"]))
        res += [ops.rows_colsum(d["da"]), ops.rows_colsum(d["dhn"].view(b, n, w))]
        res += ops.rows_max_bf16(d["h3"])
        res += ops.rows_max_bf16(d["gprev"].view(b, n, w))
        res.append(ops.tgate_forward(d["head"], d["glb"], d["alpha"]))
        res.append(ops.tgate_backward(d["dout"], d["alpha"]))
        return res
    return Row(f"head-b{b}n{n}w{w}", build, call,
               ["pcfm_head_film_fwd", "pcfm_head_film_bwd", "pcfm_head_silu_fwd",
                "pcfm_head_silu_bwd", "pcfm_rows_wgrad_bf16", "pcfm_rows_colsum",
                "pcfm_rows_max_bf16", "pcfm_tgate_fwd", "pcfm_tgate_bwd"])


# --------------------------------------------------------------------------
# losses
# --------------------------------------------------------------------------
def chamfer_row(b, n, m):
    def build(seed):
        g = G(800 + seed)
        a, c = rn(g, b, n, 3), rn(g, b, m, 3)
        if n and m:
            k = min(n, m) // 3
            c[:, :k] = a[:, :k]                              # exact hits
        return {"a": a, "c": c, "gd1": ru(g, b, n), "gd2": ru(g, b, m),
                "g1": rn(g, b, n, 3), "g2": rn(g, b, m, 3)}   # a non-zero start (ACCUMULATES)

    def call(d):
        from pcfm import ops
        t = ops.torch                 # the allocator the wrappers use (guarded when patched)
        a, c = d["a"], d["c"]
        d1 = t.empty((b, n), dtype=torch.float32, device=DEV)
        d2 = t.empty((b, m), dtype=torch.float32, device=DEV)
        i1 = t.empty((b, n), dtype=torch.int32, device=DEV)
        i2 = t.empty((b, m), dtype=torch.int32, device=DEV)
        assert ops.chamfer_3D.forward(a, c, d1, d2, i1, i2) == 1
        res = [d1, d2, i1, i2]
        if n and m:
            z1 = t.zeros((b, n, 3), dtype=torch.float32, device=DEV)   # pre-zeroed, as the
            z2 = t.zeros((b, m, 3), dtype=torch.float32, device=DEV)   # contract says
            assert ops.chamfer_3D.backward(a, c, z1, z2, d["gd1"], d["gd2"], i1, i2) == 1
            s1, s2 = d["g1"].clone(), d["g2"].clone()
            assert ops.chamfer_3D.backward(a, c, d["g1"], d["g2"], d["gd1"], d["gd2"], i1,
                                           i2) == 1
            # ACCUMULATES: the result is added to what the buffers held
            torch.testing.assert_close(d["g1"], s1 + z1, rtol=1e-5, atol=1e-5)
            torch.testing.assert_close(d["g2"], s2 + z2, rtol=1e-5, atol=1e-5)
            res += [z1, z2, d["g1"], d["g2"]]
        return res
    # the backward's sums are atomics-ordered (tests/test_gpu_ops.py: rtol 1e-5, atol
    # 1e-6 scaled to the magnitude); the forward's outputs still compare exactly
    return Row(f"chamfer-b{b}n{n}m{m}", build, call,
               ["pcfm_chamfer_fwd"] + (["pcfm_chamfer_bwd"] if n and m else []),
               tol=(1e-5, 1e-6) if n and m else None)


def emd_row(b, n, m, dtype):
    sfx = "f32" if dtype == torch.float32 else "f64"

    def build(seed):
        g = G(820 + seed)
        return {"a": ru(g, b, n, 3).to(dtype), "c": ru(g, b, m, 3).to(dtype),
                "gc": ru(g, b).to(dtype)}

    def call(d):
        from pcfm import ops
        a, c = d["a"], d["c"]
        match = ops.approxmatch_forward(a, c)
        cost = ops.matchcost_forward(a, c, match)
        m2, c2 = ops.approxmatch_cost_forward(a, c, True)
        _, c3 = ops.approxmatch_cost_forward(a, c, False)
        return [match, cost, m2, c2, c3, *ops.matchcost_backward(d["gc"], a, c, match)]
    return Row(f"emd-{sfx}-b{b}n{n}m{m}", build, call,
               [f"pcfm_emd_approxmatch_{sfx}", f"pcfm_emd_matchcost_{sfx}",
                f"pcfm_emd_approxmatch_cost_{sfx}", f"pcfm_emd_matchcost_bwd_{sfx}"])


# --------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------
ROWS = [
    vox_row(2, 4, 100, 2, "lds"), vox_row(2, 3, 17, 1, "r1"), vox_row(1, 7, 0, 4, "empty-cloud"),
    vox_row(1, 3, 3000, 64, "rows-beyond-lds"), vox_row(1, 2, 1025, 32, "1024-thread-1ch"),
    vox_row(256, 8, 50, 8, "cpb4"), vox_row(171, 7, 50, 8, "cpb2-short-last-group"),
    devox_row(2, 4, 100, 2, "lds"), devox_row(2, 3, 17, 1, "r1"),
    devox_row(1, 7, 0, 4, "empty-cloud"),
    devox_row(1, 3, 3000, 64, "rows-beyond-lds", bn=False),
    devox_row(1, 2, 1025, 32, "1024-thread-1ch", outside=True),
    devox_row(256, 8, 50, 8, "cpb4", outside=True),
    devox_row(171, 7, 50, 8, "cpb2-short-last-group", outside=True),
    group_row(2, 33, 100, 4), group_row(1, 300, 0, 3), group_row(1, 40, 2049, 70),
    pw_row(1, 5, 3, 7, "tile64", [5], [5]),
    pw_row(3, 264, 64, 129, "tile64-ragged-k", [256, 8], [256, 8]),
    pw_row(3, 256, 64, 129, "stream128", [128, 128], [128, 128], bnstats=True),
    pw_row(1, 96, 32, 45, "stream128-ragged-32pt-tile", [64, 32], [96], bnstats=True),
    pw_row(2, 128, 128, 64, "stream128-stats-into-bn", [64, 64], [128], bnstats=True),
    pw_row(4, 262, 128, 16385, "tile128-ragged-k-and-n", [256, 6], [256, 6]),
    pw_row(4, 72, 200, 16385, "tile256-56-pad-rows", [64, 8], [72], bnstats=True),
    pw_row(2, 256, 256, 100, "wgrad-wide-few-ksteps", [128, 128], [128, 128]),
    pw_row(2, 262, 128, 1000, "wgrad128-ragged-cin", [256, 6], [256, 6]),
    conv_row(1, 64, 128, 8, "fwd-only-cin64", fwd_only=True),
    conv_row(3, 128, 128, 8, "window-odd-batch"), conv_row(2, 128, 128, 16, "slab"),
    conv_row(1, 128, 128, 32, "slab"),
    conv_sparse_row(2, 128, 32, "list"), conv_sparse_row(3, 128, 32, "list-empty-batch-elem",
                                                         empty=1),
    bn_row((3, 64, 100), 0.0), bn_row((1, 32, 8, 8, 8), 0.1), bn_row((1, 5, 12), 0.1),
    bn_split_row(1, 64, 4, 0.0), bn_split_row(3, 128, 8, 0.1),
    gn_row(3, 64, 36, 8), gn_row(1, 6, 4, 3),
    se_rows_row(1, 7, 3, 5, 8), se_rows_row(3, 64, 8, 129, 100),
    head_row(3, 777, 256), head_row(1, 5, 512),
    chamfer_row(1, 1, 1), chamfer_row(1, 100, 0), chamfer_row(2, 257, 129),
    emd_row(3, 100, 37, torch.float32), emd_row(1, 513, 300, torch.float32),
    emd_row(3, 100, 37, torch.float64), emd_row(1, 513, 300, torch.float64),
]

# launching entry points no row reaches, each with its reason
EXEMPT = {
    "pcfm_debug_devox_verify": "diagnostic behind PCFM_DEVOX_VERIFY=1; allocates nothing per call",
    "pcfm_debug_devox_verify_bn": "diagnostic behind PCFM_DEVOX_VERIFY=1, as above",
}
OPTIM_ENTRIES = ["pcfm_adamw_grad_norm", "pcfm_adamw_ema_step"]
# the queries: they size or describe a call and launch nothing.  (Among the names
# ending in _parts only pcfm_gn_bnin_parts is one: pcfm_pointwise_gemm_parts,
# pcfm_pointwise_wgrad_parts, pcfm_bn_act_fwd_parts and pcfm_bn_act_bwd_apply_parts launch.)
_QUERY_SUFFIXES = ("_bytes", "_supported", "_groups", "_chunk_elems")
_QUERIES = ("pcfm_abi_version", "pcfm_last_error", "pcfm_gn_bnin_parts")


def launching_entries():
    from pcfm import _lib
    return {n for n in _lib.SIGNATURES if n not in _QUERIES and not n.endswith(_QUERY_SUFFIXES)}


def test_every_launching_entry_is_in_a_row():
    declared = set(OPTIM_ENTRIES)
    for row in ROWS:
        declared |= set(row.entries)
    entries = launching_entries()
    assert declared <= entries, sorted(declared - entries)
    assert len(EXEMPT) <= 6 and not (set(EXEMPT) & declared)
    assert entries - declared == set(EXEMPT), sorted((entries - declared) ^ set(EXEMPT))


@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_contract(ops, row, report):
    run_row(row, report)


def test_detector_on_device_memory(ops):
    """The checks themselves on HIP memory (tests/test_guard_alloc_cpu.py shows
    them on CPU tensors): a byte changed on either side of a wrapper's output --
    with a torch op, inside the arena's own allocation -- and an output nobody
    wrote are reported with the wrapper's name."""
    a = rn(G(1), 5, 8)
    with ga.GuardedAlloc() as g:
        out = ops.rows_dot(g.guarded(a), None)
        arena = g.arenas[0]
        assert arena.view.data_ptr() == out.data_ptr() and out.data_ptr() % 512 == 0
        arena.raw[ga.GUARD - 1] = 7
        arena.raw[ga.GUARD + arena.nbytes] = 7
        never = ops.torch.empty((3,), dtype=torch.float32, device=DEV)
    rep = g.report
    assert [(x.site, f, r) for x, f, r in rep.touched] == [("rows_dot#0:empty", 1, 1)]
    assert {x.site: n for x, n in rep.poison_left.items()} == \
        {"test_detector_on_device_memory#0:empty": 3}
    assert ga.poison_left(never, torch.zeros(3, device=DEV)) == 3
    assert ga.poison_left(out, a.sum(1)) == 0 and torch.equal(out, ops.rows_dot(a, None))


# --------------------------------------------------------------------------
# PCFM_EINVAL means nothing launched
# --------------------------------------------------------------------------
def test_einval_writes_nothing(ops):
    """trilinear_devoxelize_bn_scale_add at r = 64: the rows do not fit LDS, the
    call answers PCFM_EINVAL and no output element is written."""
    from pcfm._lib import PcfmError
    b, c, n, r = 1, 3, 3000, 64
    d = devox_row(b, c, n, r, "einval").build(0)
    with ga.GuardedAlloc() as g:
        with pytest.raises(PcfmError, match="status"):
            ops.trilinear_devoxelize_bn_scale_add(r, True, g.guarded(d["pts"]),
                                                  g.guarded(d["grid"]), d["mean"], d["invstd"],
                                                  d["w"], d["bias"], 0.1, None, None)
    g.report.assert_guards_intact()
    outs, inds, wgts = g.arenas[:3]
    assert [a.shape for a in (outs, inds, wgts)] == [(b, c, n), (b, 8, n), (b, 8, n)]
    assert int(outs.poison_mask().sum()) == outs.view.numel()
    assert int(wgts.poison_mask().sum()) == wgts.view.numel()
    assert int(inds.view.abs().sum()) == 0


# --------------------------------------------------------------------------
# the masked weight gradient where the K-slice masks do not fit LDS
# --------------------------------------------------------------------------
def test_wgrad_occ_beyond_the_lds_mask_cap(ops, report):
    """512 -> 896 channels at r = 32, b = 4, the smallest shape (in elements) whose
    masked weight gradient lists more chunks per split than the K-slice masks have
    room for: 9 * 7 * 4 = 252 tile triples fill the 256 CUs in one round, so
    conv3_wgrad_splits keeps one split (a second would double the rounds) of
    4 * 32^3 / 64 = 2048 chunks; their masks (16 bytes each) no longer fit behind
    the two 66 KiB staging buffers in the 160 KiB LDS (room for 1792).  The call
    used to launch the list kernel and then answer PCFM_EINVAL; it now runs
    without the K-slice masks.  The masked gradient is bit-identical to the
    unmasked one, as in test_conv_occupancy_skipping_is_exact, plain and under the
    guarded allocator."""
    from pcfm import _lib
    b, cin, cout, r = 4, 512, 896, 32
    # the shape does exceed the cap: splits and chunks per split from the size queries
    partial = (_lib.query("pcfm_conv3d_wgrad_workspace_bytes", b, cin, cout, r)
               - 4 * b * r ** 3 * (cin + cout))
    splits = partial // (27 * cin * cout * 4)
    lists = _lib.query("pcfm_conv3d_wgrad_occ_workspace_bytes", b, cin, cout, r) - partial
    cap = lists // (9 * splits * 4) - 1
    assert splits == 1 and cap == 2048 and 2 * 67584 + 16 * cap > 160 * 1024
    g = G(31)
    cnt = (ru(g, b, r ** 3) < 0.05).int()
    x = rn(g, b, cin, r, r, r) * (cnt.view(b, 1, r, r, r) > 0)
    xs = ops.conv3d_split(x.contiguous())
    del x
    gy = rn(g, b, cout, r, r, r)
    gys = ops.conv3d_split(gy)
    del gy
    occ = ops.conv3d_occupancy(cnt, r)
    a = (b, cin, cout, r)
    with recorder() as names:
        dw = ops.conv3d_wgrad_split(xs, gys, *a)
        dw_occ = ops.conv3d_wgrad_split(xs, gys, *a, occ=occ)
        assert torch.equal(dw, dw_occ)
        with ga.GuardedAlloc() as ga_:
            got = ops.conv3d_wgrad_split(xs, gys, *a, occ=ga_.guarded(occ))
        ga_.report.assert_guards_intact()
        assert ga.poison_left(got, dw) == 0 and torch.equal(got, dw)
    assert "pcfm_conv3d_wgrad_cl_occ" in names
    report("abi_contract/wgrad_occ_beyond_mask_cap", {"chunks_per_split": cap,
                                                      "compare": "bit-exact"})


# --------------------------------------------------------------------------
# optimiser
# --------------------------------------------------------------------------
def _optim_step(alloc, seed, steps=2):
    """FusedAdamWEMA over test_gpu_optim's SHAPES, built and stepped under `alloc`
    (None: the real allocator); parameters and shadows in guarded arenas."""
    from pcfm.optim import FusedAdamWEMA
    from test_gpu_optim import SHAPES
    g = G(900 + seed)
    place = alloc.guarded if alloc is not None else (lambda t: t)
    params = [place(rn(g, *s)) for s in SHAPES]
    shadows = {p: place(p.clone()) for p in params[::2]}
    grads = [[rn(g, *s) for s in SHAPES] for _ in range(steps)]
    opt = FusedAdamWEMA([{"params": params[:3], "lr": 1e-3, "weight_decay": 0.0},
                         {"params": params[3:], "lr": 2e-3, "weight_decay": 1e-2}],
                        ema_shadows=shadows)
    norms = []
    for gs in grads:
        for k, (p, gr) in enumerate(zip(params, gs)):
            p.grad = None if k == 1 else place(gr)      # one parameter without a gradient
        norms.append(opt.step(max_norm=1.0).clone())
    torch.cuda.synchronize()
    return (params + list(shadows.values()) + norms
            + [opt.exp_avg, opt.exp_avg_sq, opt.steps, opt.state_dev])


def test_optimizer_contract(ops, report):
    with recorder() as names:
        plain = _optim_step(None, 0)
        again = _optim_step(None, 0)
        assert all(_same(a, b) for a, b in zip(plain, again))
        with ga.GuardedAlloc() as g:
            got = _optim_step(g, 0)
        g.report.assert_guards_intact()
        assert all(_same(a, b) for a, b in zip(got, plain))
        with ga.GuardedAlloc() as first:
            _optim_step(first, 1)
        first.report.assert_guards_intact()
        with ga.GuardedAlloc(stale=first) as st:
            stale = _optim_step(st, 0)
        st.report.assert_guards_intact()
        bad = [k for k, (a, b) in enumerate(zip(stale, plain)) if not _same(a, b)]
        assert not bad, f"stale run: outputs {bad} differ"
    assert set(OPTIM_ENTRIES) <= set(names)
    report("abi_contract/optimizer", {"entries": sorted(set(names)), "compare": "bit-exact",
                                      "arenas": len(g.report.arenas)})


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------
def test_trainer_forward_backward_under_guards(ops, report):
    """Trainer.forward_backward plain and under the guarded allocator, same seeds:
    the same loss bits and parameter-gradient bits, every guard intact -- the
    wrappers at the shapes the autograd functions reach."""
    from pcfm.train import TrainConfig, Trainer, synthetic_batch
    cfg = dict(batch_size=2, num_points=1024, steps_per_epoch=4, epochs=1, tunableop=False,
               miopen_find=False, device_rng=False)

    def run(alloc):
        torch.manual_seed(0)
        tr = Trainer(TrainConfig(**cfg), DEV)
        tr.train_mode()
        batch = synthetic_batch(tr.cfg, DEV, generator=G(3))
        torch.manual_seed(5)
        with (alloc if alloc is not None else contextlib.nullcontext()):
            losses = tr.forward_backward(batch, epoch=201)
            torch.cuda.synchronize()
        loss = torch.stack([losses["loss_point"].float(), losses["loss_latent"].float()])
        grads = [p.grad.detach().clone() for p in tr._clip_params if p.grad is not None]
        return loss, grads

    with recorder() as names:
        loss0, grads0 = run(None)
        g = ga.GuardedAlloc()
        loss1, grads1 = run(g)
    g.report.assert_guards_intact()
    assert _same(loss0, loss1), (loss0, loss1)
    assert len(grads0) == len(grads1) and grads0
    bad = [k for k, (a, b) in enumerate(zip(grads0, grads1)) if not _same(a, b)]
    assert not bad, f"parameter gradients {bad} differ under the guarded allocator"
    report("abi_contract/trainer_forward_backward",
           {"entries": sorted(set(names)), "arenas": len(g.report.arenas), "compare": "bit-exact"})
