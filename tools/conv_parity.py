"""Digests of everything the voxel-convolution entries (csrc/conv3d.hip) return,
from fixed seeds, for a bit-for-bit comparison of two builds (dev tool):

    PCFM_LIB=<library> python tools/conv_parity.py out.json [tag]         # once per build (GPU)
    PCFM_LIB=<library> python tools/conv_parity.py --host out.json [tag]  # host decisions, no GPU
    python tools/conv_parity.py --diff a.json b.json [report.json]  # exit 1 on a difference
    python tools/conv_parity.py --trace-diff a_kernel_stats.csv b_kernel_stats.csv [report.json]

One SHA-256 per returned tensor, at the smallest shapes that reach each form of
the forward / backward-data GEMM and each weight-gradient kernel, over a
voxelized (mostly empty) input so that the tile-mask, list and occupancy forms
have work to skip.  The forms are bit-identical by design, so WHICH kernel ran
is shown by the kernel trace instead: run the digest pass of each build under
`rocprofv3 --kernel-trace --stats ... -- python tools/conv_parity.py out.json`
and give the two kernel_stats files to --trace-diff ((kernel, launches) lists
equal, every conv3_* kernel of the source launched).

--host queries the six size / support functions of the C ABI over b in 0..9, 16,
64, channels in {64, 128, 192, 256, 512}, r in {4, 6, 8, 12, 16, 24, 32, 64}."""
import ctypes
import csv
import hashlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]

# (b, cin, cout, r): what each is the smallest shape for
SHAPES = (
    (2, 128, 128, 32),   # slab<32> (unsplit, dense)
    (5, 128, 256, 16),   # slab<16>: 160 items forward
    (2, 256, 256, 8),    # window: 8 chunks over 8 splits, both directions
    (3, 128, 128, 8),    # split LDS-DMA without the window (4 chunks, 8 splits)
    (1, 128, 128, 16),   # split r = 16
    (1, 128, 128, 24),   # the non-power-of-two weight gradient (conv3_wgrad_cl_kernel)
    (4, 128, 128, 32),   # list form on 256-entry tiles
    (8, 256, 256, 16),   # list form on 128-entry tiles too (backward-data)
    (4, 256, 256, 8),    # no list form (split): the dense fallback
)
# the knobs tests flip in-process, off, at the shapes they decide
KNOBS_OFF = (("PCFM_CONV_SLAB", (2, 128, 128, 32)), ("PCFM_CONV_SLAB", (5, 128, 256, 16)),
             ("PCFM_CONV_WIN", (2, 256, 256, 8)), ("PCFM_LIST_VOX", (4, 128, 128, 32)),
             ("PCFM_LIST_VOX", (8, 256, 256, 16)))


def diff(a, b, out=None):
    da, db = json.load(open(a))["digests"], json.load(open(b))["digests"]
    bad = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    rep = {"a": json.load(open(a))["lib"], "b": json.load(open(b))["lib"],
           "compared": len(set(da) | set(db)), "differing": bad}
    if out:
        with open(out, "w") as f:
            json.dump(rep, f, indent=1)
    print(json.dumps(rep))
    return 1 if bad or not da else 0


def trace_diff(a, b, out=None):
    """(kernel, launches) of two rocprofv3 kernel_stats files; a template argument
    list may have shrunk between the builds, so a conv3 kernel is named by its base
    name and its LAST two template arguments."""
    def load(path):
        calls = {}
        for row in csv.DictReader(open(path)):
            name = row["Name"].split("(anonymous namespace)::")[-1]
            m = re.match(r"(conv3_\w+_kernel)(?:<([^>]*)>)?", name)
            if m:
                args = [x.strip() for x in (m.group(2) or "").split(",") if x.strip()]
                name = m.group(1) + ("<" + ", ".join(args[-2:]) + ">" if args else "")
            else:
                name = name.split("(")[0]
            calls[name] = calls.get(name, 0) + int(row["Calls"])
        return calls
    ca, cb = load(a), load(b)
    bad = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
    src = open(os.path.join(REPO, "point-cloud-flow-matching_amd", "csrc", "conv3d.hip")).read()
    want = sorted(set(re.findall(r"^\s+(conv3_\w+_kernel)\(", src, re.M)))
    missing = [k for k in want if not any(n.startswith(k) for n in cb)]
    rep = {"kernels": len(cb), "launches": cb, "differing": bad, "conv3_kernels_not_launched": missing}
    if out:
        with open(out, "w") as f:
            json.dump(rep, f, indent=1)
    print(json.dumps({"kernels": len(cb), "differing": bad, "conv3_kernels_not_launched": missing}))
    return 1 if bad or missing or not ca else 0


def host(out_path, tag="tree"):
    lib = ctypes.CDLL(os.environ.get("PCFM_LIB") or os.path.join(
        REPO, "point-cloud-flow-matching_amd", "csrc", "libpcfm_hip.so"))
    four = ("pcfm_conv3d_igemm_cl_workspace_bytes", "pcfm_conv3d_wgrad_workspace_bytes",
            "pcfm_conv3d_wgrad_occ_workspace_bytes")
    two = ("pcfm_conv3d_occupancy_bytes", "pcfm_conv3d_vlist_bytes")
    for n in four + two:
        getattr(lib, n).restype = ctypes.c_size_t
    lib.pcfm_conv3d_supported.restype = ctypes.c_int
    val = {}
    chans = (64, 128, 192, 256, 512)
    for b in list(range(10)) + [16, 64]:
        for r in (4, 6, 8, 12, 16, 24, 32, 64):
            for n in two:
                val[f"{n}/{b}/{r}"] = int(getattr(lib, n)(b, r))
            for cin in chans:
                for cout in chans:
                    k = f"{b}/{cin}/{cout}/{r}"
                    val[f"pcfm_conv3d_supported/{k}"] = int(lib.pcfm_conv3d_supported(b, cin, cout, r))
                    for n in four:
                        val[f"{n}/{k}"] = int(getattr(lib, n)(b, cin, cout, r))
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": val}, f)
    print(json.dumps({"values": len(val)}))
    return 0


def main(out_path, tag="tree"):
    import torch
    from pcfm import _lib, ops

    dig = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            raw = t.detach().contiguous().cpu().numpy().tobytes()
            dig[f"{name}/{i}"] = hashlib.sha256(raw).hexdigest()

    def zeroed(query, call, cnt, b, r):
        """A buffer-building entry run into a zero-filled buffer: the parts an entry
        leaves unwritten (padding, list tails) hash the same in every run."""
        buf = torch.zeros(_lib.query(query, b, r) // 4, dtype=torch.int32, device="cuda")
        _lib.call(call, ops._ptr(cnt), b, r, ops._ptr(buf), ops._stream(cnt))
        return buf

    def case(tag, b, cin, cout, r):
        gen = torch.Generator(device="cuda").manual_seed(1000 * r + cin + 7 * cout + b)
        # a voxelized grid: ~12 % of the voxels occupied, in clumps along z
        cnt = (torch.rand(b, r, r, r // 4, device="cuda", generator=gen) < 0.12).int()
        cnt = cnt.repeat_interleave(4, dim=3).reshape(b, r ** 3).contiguous()
        x = torch.randn(b, cin, r, r, r, device="cuda", generator=gen)
        x = (x * (cnt.view(b, 1, r, r, r) > 0)).contiguous()
        gy = torch.randn(b, cout, r, r, r, device="cuda", generator=gen)
        w = torch.randn(cout, cin, 3, 3, 3, device="cuda", generator=gen) / (27 * cin) ** 0.5
        bias = torch.randn(cout, device="cuda", generator=gen)
        occ = zeroed("pcfm_conv3d_occupancy_bytes", "pcfm_conv3d_occupancy", cnt, b, r)
        vl = zeroed("pcfm_conv3d_vlist_bytes", "pcfm_conv3d_vlist", cnt, b, r)
        put(f"{tag}/occupancy", occ, ops.conv3d_occupancy(cnt, r))
        put(f"{tag}/vlists", vl)
        xs, gys = ops.conv3d_split(x), ops.conv3d_split(gy)
        img, imgt = ops.conv3d_prep_weight(w, False), ops.conv3d_prep_weight(w, True)
        put(f"{tag}/split", xs, gys, img, imgt)
        for form, kw1, kw2 in (("dense", {}, {}),
                               ("mask", dict(occ=occ, occ_mode=1), dict(occ=occ, occ_mode=2)),
                               ("list", dict(vlists=vl, cnt=cnt, occ_mode=1),
                                dict(vlists=vl, cnt=cnt, occ_mode=2))):
            put(f"{tag}/igemm/{form}",
                ops.conv3d_igemm_split(xs, img, bias, b, cin, cout, r, "t", **kw1),
                ops.conv3d_igemm_split(gys, imgt, None, b, cout, cin, r, "t", **kw2))
        put(f"{tag}/wgrad", ops.conv3d_wgrad_split(xs, gys, b, cin, cout, r),
            ops.conv3d_wgrad_split(xs, gys, b, cin, cout, r, occ=occ))
        put(f"{tag}/fp32", ops.conv3d_forward(x, w, bias), ops.conv3d_backward_data(gy, w),
            ops.conv3d_backward_weight(x, gy))

    for s in SHAPES:
        case("x".join(map(str, s)), *s)
    for knob, s in KNOBS_OFF:
        os.environ[knob] = "0"
        case(knob + "=0/" + "x".join(map(str, s)), *s)
        del os.environ[knob]

    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": dig}, f, indent=1)
    print(json.dumps({"lib": tag, "digests": len(dig)}), flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(*sys.argv[2:5]))
    if sys.argv[1] == "--trace-diff":
        sys.exit(trace_diff(*sys.argv[2:5]))
    if sys.argv[1] == "--host":
        sys.exit(host(*sys.argv[2:4]))
    sys.exit(main(*sys.argv[1:3]))
