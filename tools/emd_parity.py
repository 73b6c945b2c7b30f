"""Digests of everything the approximate-EMD entries (csrc/emd.hip) return, from fixed seeds,
for a bit-for-bit comparison of two builds (dev tool):

    PCFM_LIB=<library> python tools/emd_parity.py out.json [tag]         # once per build (GPU)
    PCFM_LIB=<library> python tools/emd_parity.py --ref out.json [tag]   # distance from the fp64 reference (GPU)
    PCFM_LIB=<library> python tools/emd_parity.py --host out.json [tag]  # workspace sizes, no GPU
    python tools/emd_parity.py --diff a.json b.json [report.json]        # exit 1 on a difference

One SHA-256 per returned tensor: approxmatch's match, matchcost's cost, the
fused entry's match and cost, its cost-only cost, and matchcost_bwd's grad1 and
grad2, for f32 and f64, and what the three pcfm_emd_nd.h entries return at
D = 2, 5, 6 (clouds from the same seeds), at the shapes of tests/test_gpu_ops.py::
test_emd_vs_fp64_reference plus (8, 2048, 2048), in the default form and under
PCFM_EMD_FORM=unfused.

--ref gives, per dtype, the largest max|match - ref| / max(ref) of
approxmatch_forward and of approxmatch_cost_forward's match against
tests/helpers/emd_ref.py over those test shapes, under whatever PCFM_EMD_FORM is
set (the bound of the test was measured this way on the retired split form).

--host records pcfm_emd_workspace_bytes over b, n, m in {0, 1, 37, 64, 513,
2048, 20000} and checks bytes(.., 8) == 2 * bytes(.., 4), and
pcfm_emd_nd_workspace_bytes over the same sizes at d = 2, 3, 5, 6; the plan's own
layout (regions end to end, packs aligned) is a static_assert in emd_core.hpp."""
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd"), os.path.join(REPO, "tests")]
from helpers import emd_ref  # noqa: E402
from tools.conv_parity import diff  # noqa: E402

SHAPES = tuple((b, n, m) for b, n, m, _ in emd_ref.GPU_CASES) + ((8, 2048, 2048),)


def host(out_path, tag="tree"):
    lib = ctypes.CDLL(os.environ.get("PCFM_LIB") or os.path.join(
        REPO, "point-cloud-flow-matching_amd", "csrc", "libpcfm_hip.so"))
    lib.pcfm_emd_workspace_bytes.restype = ctypes.c_size_t
    lib.pcfm_emd_nd_workspace_bytes.restype = ctypes.c_size_t
    sizes = (0, 1, 37, 64, 513, 2048, 20000)
    val, bad = {}, []
    for b in sizes:
        for n in sizes:
            for m in sizes:
                w4, w8 = (int(lib.pcfm_emd_workspace_bytes(b, n, m, e)) for e in (4, 8))
                val[f"workspace_bytes/{b}/{n}/{m}"] = w4
                if w8 != 2 * w4:
                    bad.append((b, n, m))
                for d in (2, 3, 5, 6):
                    val[f"nd_workspace_bytes/{b}/{n}/{m}/{d}"] = int(
                        lib.pcfm_emd_nd_workspace_bytes(b, n, m, d))
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": val, "f64_not_twice_f32": bad}, f)
    print(json.dumps({"values": len(val), "f64_not_twice_f32": bad}))
    return 1 if bad else 0


def ref(out_path, tag="tree"):
    import torch
    from pcfm import ops
    worst, rows = {}, []
    for b, n, m, dts in emd_ref.GPU_CASES:
        for dt in dts:
            a, c = emd_ref.clouds(b, n, m, "float32" if dt == "f32" else "float64", 1000 * n + m)
            want = emd_ref.approxmatch(a, c)
            ta, tc = torch.from_numpy(a).cuda(), torch.from_numpy(c).cuda()
            e1 = emd_ref.rel_err(ops.approxmatch_forward(ta, tc).cpu().numpy(), want)
            e2 = emd_ref.rel_err(ops.approxmatch_cost_forward(ta, tc)[0].cpu().numpy(), want)
            rows.append({"shape": [b, n, m], "dtype": dt, "approxmatch": e1, "approxmatch_cost": e2})
            worst[dt] = max(worst.get(dt, 0.0), e1, e2)
    rep = {"lib": tag, "form": os.environ.get("PCFM_EMD_FORM", "default"),
           "max_rel_dev": worst, "cases": rows}
    with open(out_path, "w") as f:
        json.dump(rep, f, indent=1)
    print(json.dumps({k: rep[k] for k in ("lib", "form", "max_rel_dev")}), flush=True)
    return 0


def main(out_path, tag="tree"):
    import torch
    from pcfm import ops

    dig = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            dig[f"{name}/{i}"] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()

    for form in ("default", "unfused"):
        if form != "default":
            os.environ["PCFM_EMD_FORM"] = form
        for b, n, m in SHAPES:
            for dtype in (torch.float32, torch.float64):
                gen = torch.Generator(device="cuda").manual_seed(1000 * n + m + b)
                a = torch.rand(b, n, 3, device="cuda", generator=gen, dtype=dtype)
                c = torch.rand(b, m, 3, device="cuda", generator=gen, dtype=dtype)
                gc = torch.rand(b, device="cuda", generator=gen, dtype=dtype)
                tag_ = f"{form}/{b}x{n}x{m}/{'f32' if dtype == torch.float32 else 'f64'}"
                match = ops.approxmatch_forward(a, c)
                put(f"{tag_}/match", match)
                put(f"{tag_}/cost", ops.matchcost_forward(a, c, match))
                put(f"{tag_}/fused", *ops.approxmatch_cost_forward(a, c))
                put(f"{tag_}/cost_only", ops.approxmatch_cost_forward(a, c, want_match=False)[1])
                put(f"{tag_}/grads", *ops.matchcost_backward(gc, a, c, match))
                del match
            for d in (2, 5, 6):   # the pcfm_emd_nd.h entries; D = 3 is the f32 kernels above
                gen = torch.Generator(device="cuda").manual_seed(1000 * n + m + b)
                a = torch.rand(b, n, d, device="cuda", generator=gen)
                c = torch.rand(b, m, d, device="cuda", generator=gen)
                gc = torch.rand(b, device="cuda", generator=gen)
                tag_ = f"{form}/{b}x{n}x{m}/nd{d}"
                match, cost = ops.approxmatch_cost_forward_nd(a, c)
                put(f"{tag_}/fused", match, cost)
                put(f"{tag_}/cost_only", ops.approxmatch_cost_forward_nd(a, c, want_match=False)[1])
                put(f"{tag_}/cost", ops.matchcost_forward_nd(a, c, match))
                put(f"{tag_}/grads", *ops.matchcost_backward_nd(gc, a, c, match))
                del match
        os.environ.pop("PCFM_EMD_FORM", None)
    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": dig}, f, indent=1)
    print(json.dumps({"lib": tag, "digests": len(dig)}), flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(*sys.argv[2:5]))
    if sys.argv[1] == "--host":
        sys.exit(host(*sys.argv[2:4]))
    if sys.argv[1] == "--ref":
        sys.exit(ref(*sys.argv[2:4]))
    sys.exit(main(*sys.argv[1:3]))
