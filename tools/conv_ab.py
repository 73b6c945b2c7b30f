"""A/B timing of the voxel-conv GEMMs at the C2 stage shapes (dev tool).

    PCFM_LIB=<variant .so> python tools/conv_ab.py [tag]   -> one JSON line
    python tools/conv_ab.py --judge A1.jsonl [A2.jsonl ...] -> exit 1 if a call is slower

Times conv3d fwd and bwd-data (split operands; dense, and over a voxelized input
the tile-mask and list forms) and wgrad (dense and with the occupancy masks) at
C128 R32, C256 R16 and C256 R8 (B = 8) with HIP events: REPEATS repeats of 20
launches each after 3 warm-ups; `*_ms` is the median repeat, `repeats` holds all.

--judge reads job files of alternating lines, tags "parent..." and "new...", and
passes a timed call if the new build's median lies inside the spread (min..max
over all repeats) of the parent's own runs in that job, or does so in another."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]

REPEATS = 5


def judge(paths):
    jobs = []
    for p in paths:
        rows = [json.loads(l) for l in open(p) if l.startswith("{")]
        jobs.append(([r for r in rows if r["tag"].startswith("parent")],
                     [r for r in rows if r["tag"].startswith("new")]))
    calls, out = {}, {}
    for j, (par, new) in enumerate(jobs):
        for shape in (k for k in new[0] if k.startswith("C")):
            for call, reps in new[0][shape]["repeats"].items():
                pr = [t for r in par for t in r[shape]["repeats"][call]]
                nw = sorted(t for r in new for t in r[shape]["repeats"][call])
                med = nw[len(nw) // 2]
                calls.setdefault(f"{shape}/{call}", []).append(
                    {"job": j, "parent_min": min(pr), "parent_max": max(pr), "new_median": med,
                     "inside_or_faster": med <= max(pr)})
    for k, v in calls.items():
        out[k] = {"jobs": v, "pass": any(x["inside_or_faster"] for x in v)}
    bad = sorted(k for k, v in out.items() if not v["pass"])
    print(json.dumps({"calls": out, "slower": bad}, indent=1))
    return 1 if bad or not out else 0


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

    res = {"tag": tag}
    OUT = {}
    g = torch.Generator(device="cuda").manual_seed(0)
    b = 8
    for c, r in ((128, 32), (256, 16), (256, 8)):
        x = torch.randn(b, c, r, r, r, device="cuda", generator=g)
        w = torch.randn(c, c, 3, 3, 3, device="cuda", generator=g) * (1.0 / (27 * c) ** 0.5)
        xs, gys = ops.conv3d_split(x), ops.conv3d_split(x * 0.5)
        img_f, img_b = ops.conv3d_prep_weight(w, False), ops.conv3d_prep_weight(w, True)
        # a voxelized input: ~12 % of the voxels occupied, in clumps of 4 along z
        cnt = (torch.rand(b, r, r, r // 4, device="cuda", generator=g) < 0.12).int()
        cnt = cnt.repeat_interleave(4, dim=3).reshape(b, r ** 3).contiguous()
        xv = ops.conv3d_split((x * (cnt.view(b, 1, r, r, r) > 0)).contiguous())
        occ, vl = ops.conv3d_occupancy(cnt, r), ops.conv3d_vlists(cnt, r)
        flops = 2.0 * b * r ** 3 * 27 * c * c
        calls = {
            "fwd": lambda: ops.conv3d_igemm_split(xs, img_f, None, b, c, c, r, "f"),
            "bwd": lambda: ops.conv3d_igemm_split(gys, img_b, None, b, c, c, r, "f"),
            "wgrad": lambda: ops.conv3d_wgrad_split(xs, gys, b, c, c, r),
            "fwd_mask": lambda: ops.conv3d_igemm_split(xv, img_f, None, b, c, c, r, "f", occ=occ,
                                                       occ_mode=1),
            "bwd_mask": lambda: ops.conv3d_igemm_split(gys, img_b, None, b, c, c, r, "f", occ=occ,
                                                       occ_mode=2),
            "fwd_list": lambda: ops.conv3d_igemm_split(xv, img_f, None, b, c, c, r, "f", vlists=vl,
                                                       cnt=cnt, occ_mode=1),
            "bwd_list": lambda: ops.conv3d_igemm_split(gys, img_b, None, b, c, c, r, "f", vlists=vl,
                                                       cnt=cnt, occ_mode=2),
            "wgrad_occ": lambda: ops.conv3d_wgrad_split(xv, gys, b, c, c, r, occ=occ),
        }
        reps = {k: timeit(fn) for k, fn in calls.items()}
        med = {k: sorted(v)[len(v) // 2] for k, v in reps.items()}
        # correctness guard: the variant must agree with the exact fp32 conv
        y = calls["fwd"]()
        ref = torch.nn.functional.conv3d(x, w, padding=1)
        err = float((y - ref).abs().max() / ref.abs().max())
        # the weight gradient (small) and a 1/64 sample of the forward output
        OUT[f"C{c}R{r}"] = (y.flatten()[::64].cpu(), calls["wgrad"]().cpu())
        res[f"C{c}R{r}"] = dict({k + "_ms": v for k, v in med.items()},
                                fwd_TF_fp32eq=flops / med["fwd"] / 1e9,
                                wgrad_TF_fp32eq=flops / med["wgrad"] / 1e9, fwd_rel_err=err,
                                repeats=reps)
    save = os.environ.get("CONV_SAVE")  # outputs for a bitwise comparison across variants
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
