"""Digests of everything the pointwise-convolution entries (csrc/pointwise.hip)
return, from fixed seeds, for a bit-for-bit comparison of two builds (dev tool):

    PCFM_LIB=<library> python tools/pw_parity.py out.json [tag]         # once per build (GPU)
    PCFM_LIB=<library> python tools/pw_parity.py --host out.json [tag]  # host decisions, no GPU
    python tools/pw_parity.py --diff a.json b.json [report.json]  # exit 1 on a difference
    python tools/pw_parity.py --trace-diff a_kernel_stats.csv b_kernel_stats.csv [report.json]

One SHA-256 per returned tensor: forward with and without bias, forward with
statistics (y, stats), backward-data, weight gradient and the three _parts
entries (per-batch bias), at the smallest shapes that reach each form plus the
train-step shapes; the streaming shapes again with PCFM_PW_STREAM_STATS=0.
WHICH kernel ran is shown by the kernel trace: run the digest pass of each build
under `rocprofv3 --kernel-trace --stats ... -- python tools/pw_parity.py out.json`
and give the two kernel_stats files to --trace-diff ((kernel, launches) lists
equal, every pw_* kernel of the source launched).

--host queries pcfm_pointwise_weight_bytes, pcfm_pointwise_bnstats_groups and
pcfm_pointwise_wgrad_workspace_bytes over b in 0..9, 16, channels in {3, 32, 64,
96, 128, 200, 256, 262, 512, 640, 768}, n in {0, 1, 31, 64, 129, 1000, 16385,
20000}; bnstats_groups also with PCFM_PW_STREAM_STATS=0."""
import csv
import ctypes
import hashlib
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]
from tools.conv_parity import diff  # noqa: E402

# (b, cin, cout, n): what each is the smallest shape for
SHAPES = (
    (1, 5, 3, 7), (3, 264, 64, 129),                          # tile64
    (3, 256, 64, 129), (1, 96, 32, 45), (2, 128, 128, 64),    # stream128
    (4, 262, 128, 16385),                                     # tile128
    (4, 72, 200, 16385),                                      # tile256
    (2, 256, 256, 100), (1, 512, 256, 77),                    # wide weight gradient
    (8, 256, 256, 20000), (8, 128, 256, 20000), (8, 128, 128, 20000),  # train step
)
# channel-segmented calls: (b, input widths, cout, n); the last is ContextNet's head_pre
PARTS = ((2, (128, 96), 64, 333), (2, (32, 32, 32, 7), 130, 65), (8, (128, 256, 256), 256, 20000))


def trace_diff(a, b, out=None):
    """(kernel, launches) of two rocprofv3 kernel_stats files."""
    def load(path):
        calls = {}
        for row in csv.DictReader(open(path)):
            m = re.search(r"(\w+_kernel(?:<[^>]*>)?)\(", row["Name"])  # the name without its arguments
            name = m.group(1) if m else row["Name"].split("(")[0]
            calls[name] = calls.get(name, 0) + int(row["Calls"])
        return calls
    ca, cb = load(a), load(b)
    bad = sorted(k for k in set(ca) | set(cb) if ca.get(k) != cb.get(k))
    src = open(os.path.join(REPO, "point-cloud-flow-matching_amd", "csrc", "pointwise.hip")).read()
    want = sorted(set(re.findall(r"^\s+(pw_\w+_kernel)\(", src, re.M)))
    missing = [k for k in want if not any(n.startswith(k) for n in cb)]
    rep = {"kernels": len(cb), "launches": cb, "differing": bad, "pw_kernels_not_launched": missing}
    if out:
        with open(out, "w") as f:
            json.dump(rep, f, indent=1)
    print(json.dumps({"kernels": len(cb), "differing": bad, "pw_kernels_not_launched": missing}))
    return 1 if bad or missing or not ca else 0


def host(out_path, tag="tree"):
    lib = ctypes.CDLL(os.environ.get("PCFM_LIB") or os.path.join(
        REPO, "point-cloud-flow-matching_amd", "csrc", "libpcfm_hip.so"))
    lib.pcfm_pointwise_weight_bytes.restype = ctypes.c_size_t
    lib.pcfm_pointwise_wgrad_workspace_bytes.restype = ctypes.c_size_t
    lib.pcfm_pointwise_bnstats_groups.restype = ctypes.c_int
    chans = (3, 32, 64, 96, 128, 200, 256, 262, 512, 640, 768)
    val = {}
    for cin in chans:
        for cout in chans:
            val[f"weight_bytes/{cout}/{cin}"] = int(lib.pcfm_pointwise_weight_bytes(cout, cin))
            for b in list(range(10)) + [16]:
                for n in (0, 1, 31, 64, 129, 1000, 16385, 20000):
                    k = f"{b}/{cin}/{cout}/{n}"
                    val[f"wgrad_workspace_bytes/{k}"] = int(
                        lib.pcfm_pointwise_wgrad_workspace_bytes(b, cin, cout, n))
                    val[f"bnstats_groups/{k}"] = int(lib.pcfm_pointwise_bnstats_groups(b, cin, cout, n))
                    os.environ["PCFM_PW_STREAM_STATS"] = "0"
                    val[f"bnstats_groups/STREAM_STATS=0/{k}"] = int(
                        lib.pcfm_pointwise_bnstats_groups(b, cin, cout, n))
                    del os.environ["PCFM_PW_STREAM_STATS"]
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

    def case(tag, b, cin, cout, n):
        gen = torch.Generator(device="cuda").manual_seed(1000 * n + cin + 7 * cout + b)
        x = torch.randn(b, cin, n, device="cuda", generator=gen)
        w = torch.randn(cout, cin, 1, device="cuda", generator=gen) / cin ** 0.5
        bias = torch.randn(cout, device="cuda", generator=gen)
        gy = torch.randn(b, cout, n, device="cuda", generator=gen)
        fs = ops.pointwise_forward_bnstats(x, w, bias)
        dig[f"{tag}/bnstats_present"] = str(fs is not None)
        if fs is not None:
            put(f"{tag}/fwd_bnstats", *fs)
        put(f"{tag}/fwd", ops.pointwise_forward(x, w, bias), ops.pointwise_forward(x, w, None))
        put(f"{tag}/bwd_data", ops.pointwise_backward_data(gy, w))
        put(f"{tag}/wgrad", ops.pointwise_backward_weight(x, gy))

    def parts(tag, b, widths, cout, n):
        gen = torch.Generator(device="cuda").manual_seed(sum(widths) + cout + n)
        xs = [torch.randn(b, c, n, device="cuda", generator=gen) for c in widths]
        cin = sum(widths)
        w = torch.randn(cout, cin, device="cuda", generator=gen) / cin ** 0.5
        bias_b = torch.randn(b, cout, device="cuda", generator=gen)
        gy = torch.randn(b, cout, n, device="cuda", generator=gen)
        put(f"{tag}/fwd_parts", ops.pointwise_forward_parts(xs, w, bias_b, bias_per_batch=True))
        if all(v % 128 == 0 for v in widths[:-1]):
            put(f"{tag}/bwd_data_parts", *ops.pointwise_backward_data_parts(gy, w, list(widths)))
        put(f"{tag}/wgrad_parts", ops.pointwise_backward_weight_parts(xs, gy))

    for s in SHAPES:
        case("x".join(map(str, s)), *s)
    for b, widths, cout, n in PARTS:
        parts(f"parts/{b}x{'+'.join(map(str, widths))}x{cout}x{n}", b, widths, cout, n)
    groups = [_lib.query("pcfm_pointwise_bnstats_groups", *s) for s in SHAPES]
    os.environ["PCFM_PW_STREAM_STATS"] = "0"
    for s, g in zip(SHAPES, groups):  # where the switch changes pcfm_pointwise_bnstats_groups
        if _lib.query("pcfm_pointwise_bnstats_groups", *s) != g:
            case("STREAM_STATS=0/" + "x".join(map(str, s)), *s)
    del os.environ["PCFM_PW_STREAM_STATS"]

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
