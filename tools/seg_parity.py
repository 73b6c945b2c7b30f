"""Digests of everything the segment scatter engine's entries (csrc/segsum.hip
through voxel.hip, neighbor.hip and chamfer.hip) and the row gathers (rows.hpp)
return, from fixed seeds through the C ABI, for a bit-for-bit comparison of two
builds (dev tool):

    PCFM_LIB=<library> python tools/seg_parity.py out.json [tag]         # once per build and engine (GPU)
    PCFM_LIB=<library> python tools/seg_parity.py --host out.json [tag]  # size functions, no GPU
    python tools/seg_parity.py --diff a.json b.json [report.json]  # exit 1 on a difference

One SHA-256 per returned tensor: every VOX and DEVOX and GROUP case of
tests/helpers/seg_ldsrow_cases.py and the three bench-stage shapes of
tools/scatter_ab.py, through avg_voxelize fwd / plan / fwd_planned, trilinear
devoxelize bwd / bwd_plan / bwd_planned, grouping bwd, the culled Chamfer
search (its sort is the engine's) and the gathers (avg_voxelize bwd / bwd_add,
the three devoxelization forwards, grouping fwd).  Every plan buffer is
allocated zero-filled and digested whole after the plan call: that pins each
region's offset and content, the unit list included.  The engine is chosen once
per process: run it under the default and under PCFM_SEG_LDSROW=0 (the digest
keys carry the setting).

--host queries the five scatter size functions and pcfm_chamfer_workspace_bytes
over b in 0..9, 16, 64, c in {0, 1, 3, 64, 70, 128, 256}, n in {0, 1, 255, 256,
257, 4097, 20000, 40000, 40001, 100000}, r in {1, 2, 4, 8, 16, 32}, taps in
{1, 8}."""
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd"),
                os.path.join(REPO, "tests", "helpers")]

BENCH = ((8, 128, 20000, 32), (8, 256, 20000, 16), (8, 256, 20000, 8))  # scatter_ab.py
CHAMFER = ((2, 1000, 777), (1, 4097, 4097))  # culled: n, m >= 256


def diff(a, b, out=None):
    ja, jb = json.load(open(a)), json.load(open(b))
    da, db = ja["digests"], jb["digests"]
    bad = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    rep = {"a": ja["lib"], "b": jb["lib"], "compared": len(set(da) | set(db)), "differing": bad}
    if out:
        with open(out, "w") as f:
            json.dump(rep, f, indent=1)
    print(json.dumps(rep))
    return 1 if bad or not da else 0


def host(out_path, tag="tree"):
    lib = ctypes.CDLL(os.environ.get("PCFM_LIB") or os.path.join(
        REPO, "point-cloud-flow-matching_amd", "csrc", "libpcfm_hip.so"))
    bcnr = ("pcfm_avg_voxelize_fwd_workspace_bytes", "pcfm_trilinear_devoxelize_bwd_workspace_bytes")
    names = bcnr + ("pcfm_grouping_bwd_workspace_bytes", "pcfm_seg_plan_bytes",
                    "pcfm_seg_apply_workspace_bytes", "pcfm_chamfer_workspace_bytes")
    for n in names:
        getattr(lib, n).restype = ctypes.c_size_t
    val = {}
    ns = (0, 1, 255, 256, 257, 4097, 20000, 40000, 40001, 100000)
    for b in list(range(10)) + [16, 64]:
        for n in ns:
            for m in ns:
                val[f"pcfm_chamfer_workspace_bytes/{b}/{n}/{m}"] = int(
                    lib.pcfm_chamfer_workspace_bytes(b, n, m))
            for r in (1, 2, 4, 8, 16, 32):
                for taps in (1, 8):
                    val[f"pcfm_seg_plan_bytes/{b}/{n}/{r}/{taps}"] = int(
                        lib.pcfm_seg_plan_bytes(b, n, r, taps))
                for c in (0, 1, 3, 64, 70, 128, 256):
                    for f in bcnr:
                        val[f"{f}/{b}/{c}/{n}/{r}"] = int(getattr(lib, f)(b, c, n, r))
                    for taps in (1, 8):
                        val[f"pcfm_seg_apply_workspace_bytes/{b}/{c}/{n}/{r}/{taps}"] = int(
                            lib.pcfm_seg_apply_workspace_bytes(b, c, n, r, taps))
                    m = min(n, 4097)  # grouping: n rows, m * r items
                    val[f"pcfm_grouping_bwd_workspace_bytes/{b}/{c}/{n}/{m}/{r}"] = int(
                        lib.pcfm_grouping_bwd_workspace_bytes(b, c, n, m, r))
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": val}, f)
    print(json.dumps({"values": len(val)}))
    return 0


def main(out_path, tag="tree"):
    os.environ.setdefault("PCFM_CHAMFER_CULL_PAIRS", "1")  # the culled search at every size
    import numpy as np
    import torch
    import seg_ldsrow_cases as cases
    from pcfm import _lib, ops

    engine = "ldsrow=" + os.environ.get("PCFM_SEG_LDSROW", "1")
    dig = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            raw = t.detach().contiguous().cpu().numpy().tobytes()
            dig[f"{engine}/{name}/{i}"] = hashlib.sha256(raw).hexdigest()

    cu = cases._cu
    st = torch.cuda.current_stream().cuda_stream

    def zeros(nbytes):
        return torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device="cuda")

    def f32(*shape):
        return torch.zeros(shape, dtype=torch.float32, device="cuda")

    def i32(*shape):
        return torch.zeros(shape, dtype=torch.int32, device="cuda")

    def vox(tag, feat, coords, r):
        b, c, n = feat.shape
        s = r ** 3
        out, ind, cnt = f32(b, c, s), i32(b, n), i32(b, s)
        ws = zeros(_lib.query("pcfm_avg_voxelize_fwd_workspace_bytes", b, c, n, r))
        _lib.call("pcfm_avg_voxelize_fwd", feat.data_ptr(), coords.data_ptr(), b, c, n, r,
                  out.data_ptr(), ind.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(), st)
        put(f"{tag}/avg_voxelize_fwd", out, ind, cnt)
        plan, pind, pcnt = zeros(_lib.query("pcfm_seg_plan_bytes", b, n, r, 1)), i32(b, n), i32(b, s)
        _lib.call("pcfm_avg_voxelize_plan", coords.data_ptr(), b, n, r, pind.data_ptr(),
                  pcnt.data_ptr(), plan.data_ptr(), plan.numel(), st)
        put(f"{tag}/avg_voxelize_plan", plan, pind, pcnt)
        out2 = f32(b, c, s)
        ws = zeros(_lib.query("pcfm_seg_apply_workspace_bytes", b, c, n, r, 1))
        _lib.call("pcfm_avg_voxelize_fwd_planned", feat.data_ptr(), plan.data_ptr(), b, c, n, r,
                  out2.data_ptr(), ws.data_ptr(), ws.numel(), st)
        put(f"{tag}/avg_voxelize_fwd_planned", out2)
        # the gathers back: grad of `out` to the points, alone and added to feat
        put(f"{tag}/avg_voxelize_bwd", ops.avg_voxelize_backward(out, ind, cnt),
            ops.avg_voxelize_backward_add(out, ind, cnt, feat))

    def devox(tag, gy, pts, r, grid):
        b, c, n = gy.shape
        s = r ** 3
        fwd, inds, wgts = ops.trilinear_devoxelize_forward(r, True, pts, grid)
        sc = grid[:, :, :1].reshape(b, c).contiguous()
        put(f"{tag}/devox_fwd", fwd, inds, wgts,
            ops.trilinear_devoxelize_forward(r, False, pts, grid)[0],
            ops.trilinear_devoxelize_scale_add(r, True, pts, grid, sc, gy)[0])
        if c > 0 and s <= 32768:
            mean, invstd = sc[0].contiguous(), (sc[0].abs() + 0.5).contiguous()
            put(f"{tag}/devox_fwd_bn", ops.trilinear_devoxelize_bn_scale_add(
                r, True, pts, grid, mean, invstd, invstd, mean, 0.1, sc, gy)[0])
        gx = f32(b, c, s)
        ws = zeros(_lib.query("pcfm_trilinear_devoxelize_bwd_workspace_bytes", b, c, n, r))
        _lib.call("pcfm_trilinear_devoxelize_bwd", gy.data_ptr(), inds.data_ptr(), wgts.data_ptr(),
                  b, c, n, r, gx.data_ptr(), ws.data_ptr(), ws.numel(), st)
        put(f"{tag}/devox_bwd", gx)
        plan = zeros(_lib.query("pcfm_seg_plan_bytes", b, n, r, 8))
        _lib.call("pcfm_trilinear_devoxelize_bwd_plan", inds.data_ptr(), wgts.data_ptr(), b, n, r,
                  plan.data_ptr(), plan.numel(), st)
        put(f"{tag}/devox_bwd_plan", plan)
        gx2 = f32(b, c, s)
        ws = zeros(_lib.query("pcfm_seg_apply_workspace_bytes", b, c, n, r, 8))
        _lib.call("pcfm_trilinear_devoxelize_bwd_planned", gy.data_ptr(), plan.data_ptr(), b, c, n,
                  r, gx2.data_ptr(), ws.data_ptr(), ws.numel(), st)
        put(f"{tag}/devox_bwd_planned", gx2)

    def group(tag, gy, idx, n):
        b, c, m, u = gy.shape
        gx = f32(b, c, n)
        ws = zeros(_lib.query("pcfm_grouping_bwd_workspace_bytes", b, c, n, m, u))
        _lib.call("pcfm_grouping_bwd", gy.data_ptr(), idx.data_ptr(), b, c, n, m, u, gx.data_ptr(),
                  ws.data_ptr(), ws.numel(), st)
        put(f"{tag}/grouping_bwd", gx, ops.grouping_forward(gx, idx))

    def chamfer(tag, b, n, m):
        gen = torch.Generator(device="cuda").manual_seed(17 * n + m + b)
        x1 = torch.randn(b, n, 3, device="cuda", generator=gen)
        x2 = torch.randn(b, m, 3, device="cuda", generator=gen)
        d1, d2, i1, i2 = f32(b, n), f32(b, m), i32(b, n), i32(b, m)
        ws = zeros(_lib.query("pcfm_chamfer_workspace_bytes", b, n, m))
        _lib.call("pcfm_chamfer_fwd", x1.data_ptr(), x2.data_ptr(), b, n, m, d1.data_ptr(),
                  d2.data_ptr(), i1.data_ptr(), i2.data_ptr(), ws.data_ptr(), ws.numel(), st)
        put(f"{tag}/chamfer_fwd", d1, d2, i1, i2)

    for name in cases.VOX:
        feat, coords, r = cases.vox_inputs(name)
        vox(f"vox.{name}", cu(feat), cu(coords), r)
    for name in cases.DEVOX:
        gy, pts, r = cases.devox_inputs(name)
        devox(f"devox.{name}", cu(gy), cu(pts), r, cu(cases.devox_grid(name)))
    for name in cases.GROUP:
        gy, idx, n = cases.group_inputs(name)
        group(f"group.{name}", cu(gy), cu(idx), n)
    for b, c, n, r in BENCH:
        g = np.random.default_rng([5, c, r])
        pts = np.clip(g.normal(r / 2, r / 6, (b, 3, n)), 0, r - 1).astype(np.float32)
        feat = g.standard_normal((b, c, n)).astype(np.float32)
        grid = g.standard_normal((b, c, r ** 3)).astype(np.float32)
        vox(f"bench.C{c}R{r}", cu(feat), cu(np.round(pts).astype(np.int32)), r)
        devox(f"bench.C{c}R{r}", cu(feat), cu(pts), r, cu(grid))
    for b, n, m in CHAMFER:
        chamfer(f"chamfer.{b}x{n}x{m}", b, n, m)

    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": dig}, f, indent=1)
    print(json.dumps({"lib": tag, "engine": engine, "digests": len(dig)}), flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(*sys.argv[2:5]))
    if sys.argv[1] == "--host":
        sys.exit(host(*sys.argv[2:4]))
    sys.exit(main(*sys.argv[1:3]))
