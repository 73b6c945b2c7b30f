"""A/B timing of the pointwise (1x1 conv) bf16x3 GEMMs at the C2 train-step
shapes and ContextNet's head_pre parts call (dev tool).

    PCFM_LIB=<variant .so> python tools/pw_ab.py [tag]   -> one JSON line
    python tools/pw_ab.py --judge A1.jsonl [A2.jsonl ...] -> exit 1 if a call is slower

Times forward, backward-data and the weight gradient with HIP events: REPEATS
repeats of 20 launches each after 3 warm-ups; `*_ms` is the median repeat,
`repeats` holds all.  --judge is tools/conv_ab.py's: job files of alternating
lines, tags "parent..." and "new..."; a timed call passes if the new build's
median lies inside the spread of the parent's own runs in that job, or does so
in another."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]
from tools.conv_ab import REPEATS, judge  # noqa: E402


def main(tag):
    import torch
    from pcfm import ops

    def timeit(fn, it=20):
        for _ in range(3):
            fn()
        reps = []
        for _ in range(REPEATS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(it):
                fn()
            e1.record()
            torch.cuda.synchronize()
            reps.append(e0.elapsed_time(e1) / it)
        return reps

    def record(key, calls):
        reps = {k: timeit(fn) for k, fn in calls.items()}
        res[key] = dict({k + "_ms": sorted(v)[len(v) // 2] for k, v in reps.items()}, repeats=reps)

    OUT = {}
    res = {"tag": tag}
    g = torch.Generator(device="cuda").manual_seed(0)
    for b, ci, co, n in ((8, 256, 256, 20000), (8, 128, 256, 20000), (8, 128, 128, 20000)):
        x = torch.randn(b, ci, n, device="cuda", generator=g)
        w = torch.randn(co, ci, 1, device="cuda", generator=g) * ci ** -0.5
        bias = torch.randn(co, device="cuda", generator=g)
        dy = torch.randn(b, co, n, device="cuda", generator=g)
        key = f"Ci{ci}Co{co}N{n}B{b}"
        record(key, {"fwd": lambda: ops.pointwise_forward(x, w, bias),
                     "bwd_data": lambda: ops.pointwise_backward_data(dy, w),
                     "wgrad": lambda: ops.pointwise_backward_weight(x, dy)})
        OUT[key] = (ops.pointwise_forward(x, w, bias).cpu(),
                    ops.pointwise_backward_data(dy, w).cpu())
    # ContextNet head_pre as the benchmark's model calls it: the three stage
    # outputs read in place, per-cloud bias
    b, widths, co, n = 8, (128, 256, 256), 256, 20000
    xs = [torch.randn(b, c, n, device="cuda", generator=g) for c in widths]
    w = torch.randn(co, sum(widths), device="cuda", generator=g) * sum(widths) ** -0.5
    bias_b = torch.randn(b, co, device="cuda", generator=g)
    dy = torch.randn(b, co, n, device="cuda", generator=g)
    record("Chead_pre_parts", {
        "fwd": lambda: ops.pointwise_forward_parts(xs, w, bias_b, bias_per_batch=True),
        "wgrad": lambda: ops.pointwise_backward_weight_parts(xs, dy)})
    save = os.environ.get("PW_SAVE")  # outputs for a bitwise comparison across variants
    if save:
        if os.path.exists(save):
            ref = torch.load(save, weights_only=True)
            res["bit_equal_to_saved"] = all(torch.equal(a, c) for k in OUT
                                            for a, c in zip(OUT[k], ref[k]))
        else:
            torch.save(OUT, save)
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--judge":
        sys.exit(judge(sys.argv[2:]))
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("PCFM_LIB", "main")))
