"""Digests of everything the BatchNorm / GroupNorm entries (csrc/norm.hip) and the
BatchNorm-applying devoxelization gather return, from fixed seeds, for a
bit-for-bit comparison of two builds (dev tool):

    PCFM_LIB=<library> python tools/norm_parity.py out.json     # once per build
    python tools/norm_parity.py --diff a.json b.json            # exit 1 on a difference

One SHA-256 per returned tensor and per buffer updated in place.  The shapes are
the smallest that reach each branch of the kernels (part counts, tails, block
counts, reversed block order with an odd count)."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]


def diff(a, b):
    da, db = json.load(open(a))["digests"], json.load(open(b))["digests"]
    bad = sorted(k for k in set(da) | set(db) if da.get(k) != db.get(k))
    print(json.dumps({"compared": len(set(da) | set(db)), "differing": bad}))
    return 1 if bad or not da else 0


def main(out_path):
    import torch
    from pcfm import ops

    dig = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                raw = t.detach().contiguous().cpu().numpy().tobytes()
                dig[f"{name}/{i}"] = hashlib.sha256(raw).hexdigest()

    gen = torch.Generator(device="cuda").manual_seed(1234)

    def randn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen)

    def rand(*shape):
        return torch.rand(*shape, device="cuda", generator=gen)

    def running(c):
        return rand(c) - 0.5, rand(c) + 0.5, torch.full((), 5, dtype=torch.int64, device="cuda")

    def groups(c, b, s, gsz):  # a producer's epilogue statistics: (mean, centred m2) per group
        p = b * ((s + gsz - 1) // gsz)
        return torch.stack([randn(c, p) + 3.0, rand(c, p) * 100.0 + 1.0], dim=-1).contiguous()

    # contiguous BatchNorm entries
    for shape in ((3, 5, 36), (2, 64, 4100), (1, 4, 70000)):
        b, c, s = shape
        tag = "x".join(map(str, shape))
        x, dz = randn(*shape) * 2.0 + 3.0, randn(*shape)
        gamma, beta = rand(c) + 0.5, rand(c) - 0.5
        for slope in (0.0, 0.1):
            rm, rv, nbt = running(c)
            y, mean, invstd = ops.bn_act_forward(x, gamma, beta, 1e-5, slope, 0.1, rm, rv, nbt)
            put(f"bn_act_forward/{tag}/{slope}", y, mean, invstd, rm, rv, nbt)
            rm, rv, nbt = running(c)
            put(f"bn_act_forward_rowmean/{tag}/{slope}",
                *ops.bn_act_forward_rowmean(x, gamma, beta, 1e-5, slope, 0.1, rm, rv, nbt),
                rm, rv, nbt)
            for dbias in (False, True):
                put(f"bn_act_backward/{tag}/{slope}/{dbias}",
                    *ops.bn_act_backward(dz, x, gamma, beta, mean, invstd, slope, dbias))
                for p in (1, 8, 19):
                    part = randn(c, p, 2).contiguous()
                    put(f"bn_act_backward_parts/{tag}/{slope}/{dbias}/{p}",
                        *ops.bn_act_backward_parts(dz, x, gamma, beta, mean, invstd, part, slope,
                                                   dbias))
        rm, rv, nbt = running(c)
        put(f"bn_forward_stats/{tag}", *ops.bn_forward_stats(x, 1e-5, 0.1, rm, rv, nbt), rm, rv,
            nbt)
        put(f"bn_forward_stats/{tag}/norunning", *ops.bn_forward_stats(x, 1e-5, 0.1, None, None))
        for gsz in (64, 32):
            rm, rv, nbt = running(c)
            put(f"bn_act_forward_parts/{tag}/{gsz}",
                *ops.bn_act_forward_parts(x, groups(c, b, s, gsz), gamma, beta, 1e-5, 0.1, 0.1,
                                          rm, rv, nbt), rm, rv, nbt)

    # statistics from a producer's groups: P = 6, 12 and 819 (> 768: the 4-deep loop)
    for b, s, gsz in ((3, 100, 64), (3, 100, 32), (13, 4000, 64)):
        c = 7
        rm, rv, nbt = running(c)
        put(f"bn_forward_stats_parts/{b}x{s}/{gsz}",
            *ops.bn_forward_stats(randn(b, c, s), 1e-5, 0.1, rm, rv, nbt,
                                  parts=groups(c, b, s, gsz)), rm, rv, nbt)

    # split forms and the SE forms
    for b, c, r in ((1, 64, 4), (3, 128, 8), (2, 64, 16), (1, 64, 32)):
        tag = f"{b}x{c}x{r}"
        x, dz = randn(b, c, r, r, r) * 2.0 + 1.0, randn(b, c, r, r, r)
        gamma, beta = rand(c) + 0.5, rand(c) - 0.5
        se_s, dmv = rand(b, c), randn(b, c) * 1e-3
        for slope in (0.0, 0.1):
            rm, rv, nbt = running(c)
            ys, mean, invstd = ops.bn_act_forward_split(x, gamma, beta, 1e-4, slope, 0.1, rm, rv,
                                                        nbt)
            put(f"bn_act_forward_split/{tag}/{slope}", ys, mean, invstd, rm, rv, nbt)
            rowstats = ops.bn_se_backward_stats(dz, x, mean, invstd, gamma, beta, slope)
            put(f"bn_se_backward_stats/{tag}/{slope}", rowstats)
            for dbias in (False, True):
                put(f"bn_act_backward_split/{tag}/{slope}/{dbias}",
                    *ops.bn_act_backward_split(dz, x, gamma, beta, mean, invstd, slope, dbias))
                put(f"bn_se_backward_apply_split/{tag}/{slope}/{dbias}",
                    *ops.bn_se_backward_apply_split(dz, x, mean, invstd, gamma, beta, se_s, dmv,
                                                    rowstats, slope, dbias))

    # GroupNorm entries: plain, over a pre-BatchNorm tensor, SiLU
    for b, c, n, grp in ((3, 64, 36, 8), (2, 128, 1000, 32)):
        tag = f"{b}x{c}x{n}x{grp}"
        x, dout = randn(b, c, n) + 0.5, randn(b, c, n)
        w, bias = rand(c) + 0.5, rand(c) - 0.5
        fg, fb = randn(b, c) * 0.1, randn(b, c) * 0.1
        out, mean, rstd = ops.gn_film_res_forward(x, w, bias, fg, fb, grp, 1e-5)
        put(f"gn_film_res_forward/{tag}", out, mean, rstd)
        put(f"gn_film_res_backward/{tag}",
            *ops.gn_film_res_backward(dout, x, w, bias, fg, mean, rstd, grp))
        out, mean, rstd = ops.gn_silu_forward(x, w, bias, grp, 1e-5)
        put(f"gn_silu_forward/{tag}", out, mean, rstd)
        put(f"gn_silu_backward/{tag}", *ops.gn_silu_backward(dout, x, w, bias, mean, rstd, grp))
        bg, bb = rand(c) + 0.5, rand(c) - 0.5
        for slope in (0.0, 0.1):
            bm, biv = ops.bn_forward_stats(x, 1e-5, 0.1, None, None)
            out, mean, rstd = ops.gn_film_res_forward_bnin(x, bm, biv, bg, bb, slope, w, bias, fg,
                                                           fb, grp, 1e-5)
            put(f"gn_film_res_forward_bnin/{tag}/{slope}", out, mean, rstd)
            put(f"gn_film_res_backward_bnin/{tag}/{slope}",
                *ops.gn_film_res_backward_bnin(dout, x, bm, biv, bg, bb, slope, w, bias, fg, mean,
                                               rstd, grp))

    # the devoxelization gather that applies BatchNorm + activation while staging
    for b, c, r, n in ((2, 128, 16, 1000), (1, 64, 4, 100)):
        tag = f"{b}x{c}x{r}x{n}"
        x = randn(b, c, r, r, r) * 2.0 + 1.0
        gamma, beta = rand(c) + 0.5, rand(c) - 0.5
        mean, invstd = ops.bn_forward_stats(x, 1e-4, 0.1, None, None)
        coords = rand(b, 3, n) * (r - 1)
        sc, add = rand(b, c), randn(b, c, n)
        am, aiv = ops.bn_forward_stats(add, 1e-5, 0.1, None, None)
        add_bn = (am, aiv, rand(c) + 0.5, rand(c) - 0.5, 0.0)
        for name, abn in (("plain", None), ("add_bn", add_bn)):
            for training in (True, False):
                o, i, wt = ops.trilinear_devoxelize_bn_scale_add(r, training, coords, x, mean,
                                                                 invstd, gamma, beta, 0.1, sc,
                                                                 add, abn)
                put(f"devox_bn/{tag}/{name}/{training}", o, *((i, wt) if training else ()))

    torch.cuda.synchronize()
    lib = os.path.basename(os.environ.get("PCFM_LIB", "libpcfm_hip.so"))
    with open(out_path, "w") as f:
        json.dump({"lib": lib, "digests": dig}, f, indent=1)
    print(json.dumps({"lib": lib, "digests": len(dig)}), flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    sys.exit(main(sys.argv[1]))
