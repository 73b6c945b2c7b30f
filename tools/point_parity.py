"""Digests of what the point-cloud loss and metric entries return (csrc/chamfer.hip,
chamfer_nd.hip, chamfer_cross.hip, fps.hip, occupancy.hip, emd_auction.hip and the
optimizer's block sum in optim.hip), from fixed seeds, for a bit-for-bit comparison
of two builds (dev tool):

    PCFM_LIB=<library> python tools/point_parity.py out.json [tag]   # once per build (GPU)
    python tools/point_parity.py --diff a.json b.json [report.json]  # exit 1 on a difference

One SHA-256 per returned tensor, at the smallest sizes that take each code path:
  chamfer_nd   D = 2, 3, 5, 6: one candidate split; two (b = 1, n = m = 512: the key
               merge and unpack run); ragged n, m (no multiple of 8 or of a group),
               unsplit and split
  chamfer_3d   299 x 300 (brute force) and 300 x 300 (culled): either side of the
               culling threshold, which the tool sets to 300 * 300 pairs
               (PCFM_CHAMFER_CULL_PAIRS, read once per process)
  cross        one query block per cloud; two (n, m just above 2048); 128 x 128
               small clouds, the smallest launch with a partner tile of 2
  fps          resident at 1 and at 4 points per thread; streaming (n just above
               pcfm_fps_resident_points(), m = 5); a cloud on a 4^D grid (ties in
               every round, across lanes and waves)
  occupancy    r = 3, 28, 32 over D = 3, 5, 6, a third of the points outside the
               sphere (the nearest-kept-node search)
  auction      D = 2, 3, 5, 6 x n = 1, 2, 63, 65, 257, the last third of each cloud
               a copy of the first (equal bids)
  adamw        FusedAdamWEMA, two steps over odd-sized and multi-chunk tensors with
               clipping: norm / multiplier / flag, parameters, moments, EMA
Chamfer backward adds with float atomics and has no stable digest: its kernel is
compared in the listing (tools/isa_same.py)."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd")]
from tools.conv_parity import diff  # noqa: E402

CULL_PAIRS = 300 * 300


def main(out_path, tag="tree"):
    os.environ["PCFM_CHAMFER_CULL_PAIRS"] = str(CULL_PAIRS)
    import torch
    from pcfm import _lib, ops
    from pcfm.optim import FusedAdamWEMA

    dig = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            raw = t.detach().contiguous().cpu().numpy().tobytes()
            dig[f"{name}/{i}"] = hashlib.sha256(raw).hexdigest()

    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)

    def rand(g, *shape):
        return torch.rand(*shape, device="cuda", generator=g)

    def chamfer(entry, a, c):
        b, n, m = a.shape[0], a.shape[1], c.shape[1]
        out = (torch.empty(b, n, device="cuda"), torch.empty(b, m, device="cuda"),
               torch.empty(b, n, dtype=torch.int32, device="cuda"),
               torch.empty(b, m, dtype=torch.int32, device="cuda"))
        assert entry.forward(a, c, *out) == 1
        return out

    for d in ops.POINT_DIMS:
        nd = getattr(ops, f"chamfer_{d}D") if d != 3 else ops._chamfer_namespace(3, "_nd")
        for b, n, m in ((2, 300, 200), (1, 512, 512), (2, 37, 101), (1, 523, 777)):
            g = gen(100 * d + n)
            put(f"chamfer_nd/{d}/{b}x{n}x{m}", *chamfer(nd, rand(g, b, n, d), rand(g, b, m, d)))

    for b, n, m in ((2, 299, 300), (2, 300, 300)):
        g = gen(n)
        put(f"chamfer_3d/{b}x{n}x{m}", *chamfer(ops.chamfer_3D, rand(g, b, n, 3), rand(g, b, m, 3)))

    for d in ops.POINT_DIMS:
        for s, r, n, m in ((3, 2, 300, 200), (2, 3, 2049, 2050), (128, 128, 24, 17)):
            g = gen(1000 * d + n)
            put(f"cross/{d}/{s}x{r}x{n}x{m}", *ops.chamfer_cross_forward(rand(g, s, n, d),
                                                                         rand(g, r, m, d)))

    resident = _lib.query("pcfm_fps_resident_points")
    for d in ops.POINT_DIMS:
        for b, n, m in ((2, 500, 64), (2, 1500, 64), (1, resident + 7, 5)):
            g = gen(2000 * d + m + b)
            pts = rand(g, b, n, d)
            start = torch.tensor([n // 3] * b, dtype=torch.int32, device="cuda")
            put(f"fps/{d}/{b}x{n}x{m}", *ops.farthest_point_sample(pts, m, start))
        g = gen(3000 + d)
        grid = torch.randint(0, 4, (2, 1000, d), device="cuda", generator=g).float() / 4
        put(f"fps/{d}/grid", *ops.farthest_point_sample(grid, 64))

    for d in (3, 5, 6):
        for r in (3, 28, 32):
            g = gen(4000 + 10 * d + r)
            put(f"occupancy/{d}/{r}", ops.occupancy_counts(rand(g, 3, 1000, d) * 1.3 - 0.65, r))

    for d in ops.POINT_DIMS:
        for n in (1, 2, 63, 65, 257):
            g = gen(5000 + 10 * n + d)
            a, c = rand(g, 3, n, d), rand(g, 3, n, d)
            k = n // 3
            if k:
                a[:, n - k:] = a[:, :k]
                c[:, n - k:] = c[:, :k]
            put(f"auction/{d}/{n}", *ops.emd_auction(a, c))
            put(f"auction/{d}/{n}/cost_only", *ops.emd_auction(a, c, want_assignment=False)[1:])

    g = gen(6000)
    chunk = _lib.query("pcfm_adamw_chunk_elems")
    params = [torch.nn.Parameter(torch.randn(k, device="cuda", generator=g))
              for k in (70001, 2 * chunk + 4, 64, 3)]
    ema = {p: p.detach().clone() for p in params[:2]}
    opt = FusedAdamWEMA([{"params": params[:2], "lr": 1e-3, "weight_decay": 1e-2},
                         {"params": params[2:], "lr": 2e-3, "weight_decay": 0.0}], ema_shadows=ema)
    for step in range(2):
        for p in params[:3]:   # the last parameter has no gradient: skipped
            p.grad = torch.randn(p.shape, device="cuda", generator=g)
        opt.step(max_norm=1.0)
        put(f"adamw/{step}", opt.state_dev, opt.steps, opt.exp_avg, opt.exp_avg_sq, *params,
            *ema.values())

    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": dig}, f, indent=1)
    print(json.dumps({"lib": tag, "digests": len(dig)}), flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(*sys.argv[2:5]))
    sys.exit(main(*sys.argv[1:3]))
