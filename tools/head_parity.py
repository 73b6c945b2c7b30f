"""Digests of everything the per-point head entries (csrc/head.hip and
csrc/head_film.hip) return, from fixed seeds, for a bit-for-bit comparison of
two builds (dev tool):

    PCFM_LIB=<library> python tools/head_parity.py out.json [tag]   # once per build (GPU)
    python tools/head_parity.py --diff a.json b.json [report.json]  # exit 1 on a difference

One SHA-256 per returned tensor, plus the workspace queries as numbers:

* pcfm_rows_wgrad_bf16 over the three load modes of each operand (an odd row
  stride, an even unaligned one, an aligned multiple of 128 columns), the shapes
  of tests/test_gpu_head.py, the train-step shapes and one 128 x 128 tile at the
  partial counts REDUCE_S (the loop edges of the ordered reduce);
* pcfm_rows_colsum in bf16 and fp32, pcfm_rows_max_bf16, pcfm_tgate_fwd / _bwd;
* pcfm_head_film_fwd / _bwd and pcfm_head_silu_fwd / _bwd at widths 256 and 512:
  h16 with and without hbias and the (uprev, gprev) form, the backward with u
  given and with u recomputed, at tests/helpers/head_film_ref.py's shapes, the
  chunk counts REDUCE_S and the train-step shape.

The pointwise weight gradient shares the ordered reduce: its digests come from
tools/pw_parity.py, run beside this tool."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "point-cloud-flow-matching_amd"),
                os.path.join(REPO, "tests", "helpers")]
from tools.conv_parity import diff  # noqa: E402

REDUCE_S = (1, 3, 4, 5, 12, 13, 16, 17, 29, 33)
# (row stride, columns) per load mode of rows_wgrad_kernel's load_tile
MODES = {0: (131, 100), 1: (130, 100), 2: (256, 128)}
WGRAD = ((5000, 512, 512), (4097, 256, 384), (3001, 6, 512), (2500, 128, 6), (1000, 512, 326),
         (63, 128, 128), (1, 3, 5),
         (160000, 512, 512), (160000, 512, 384), (160000, 6, 512))       # train step
COLSUM = ((1, 160000, 128), (8, 20000, 64), (3, 777, 6), (1, 5, 512), (8, 20000, 512))
ROWSMAX = ((8, 20000, 128), (2, 777, 6), (3, 50, 384))
TGATE = ((3, 64, 1000), (2, 70, 130), (8, 64, 20000))
FILM_TRAIN = ((8, 20000, 512), (8, 20000, 256))


def main(out_path, tag="tree"):
    import head_film_ref as R
    import torch
    from pcfm import _lib, ops

    dig = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            if t is not None:
                raw = t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()
                dig[f"{name}/{i}"] = hashlib.sha256(raw).hexdigest()

    def gen(seed):
        return torch.Generator(device="cuda").manual_seed(seed)

    def wgrad(name, rows, m, n, lda=None, ldb=None):
        g = gen(rows + 3 * m + n)
        a = torch.randn(rows, lda or m, device="cuda", generator=g).bfloat16()[:, :m]
        b = torch.randn(rows, ldb or n, device="cuda", generator=g).bfloat16()[:, :n]
        dig[f"{name}/workspace"] = _lib.query("pcfm_rows_wgrad_workspace_bytes", rows, m, n)
        put(name, ops.rows_wgrad_bf16(a, b))

    for ma, (lda, m) in MODES.items():
        for mb, (ldb, n) in MODES.items():
            wgrad(f"rows_wgrad/modes{ma}{mb}", 4097, m, n, lda, ldb)
    for rows, m, n in WGRAD:
        wgrad(f"rows_wgrad/{rows}x{m}x{n}", rows, m, n)
    for s in REDUCE_S:
        wgrad(f"rows_wgrad/S{s}", 512 * s, 128, 128)

    for b, rows, c in COLSUM + tuple((1, 256 * s, 64) for s in REDUCE_S):
        for dt in (torch.bfloat16, torch.float32):
            name = f"rows_colsum/{b}x{rows}x{c}/{str(dt).split('.')[1]}"
            x = torch.randn(b, rows, c, device="cuda", generator=gen(b + rows + c)).to(dt)
            dig[f"{name}/workspace"] = _lib.query("pcfm_rows_colsum_workspace_bytes", b, rows, c)
            put(name, ops.rows_colsum(x))

    for b, n, c in ROWSMAX:
        h = torch.randn(b, n, c, device="cuda", generator=gen(n + c)).bfloat16()
        h[0, 5:9, 0] = 100.0  # a tie
        dig[f"rows_max/{b}x{n}x{c}/workspace"] = _lib.query("pcfm_rows_max_workspace_bytes", b, n, c)
        put(f"rows_max/{b}x{n}x{c}", *ops.rows_max_bf16(h))

    for b, c, n in TGATE:
        g = gen(b + c + n)
        head = torch.randn(b, c, n, device="cuda", generator=g)
        glb = torch.randn(b, c, device="cuda", generator=g)
        alpha = torch.rand(b, device="cuda", generator=g)
        dout = torch.randn(b, n, c, device="cuda", generator=g)
        put(f"tgate/{b}x{c}x{n}", ops.tgate_forward(head, glb, alpha), ops.tgate_backward(dout, alpha))

    def film(name, inp):
        """inp: CUDA tensors (or None) under make_inputs' names."""
        b, n, w = inp["b"], inp["n"], inp["w"]
        dig[f"{name}/workspace"] = _lib.query("pcfm_head_bwd_workspace_bytes", b, n, w)
        u, a, mean, rstd = ops.head_film_fwd(inp["h16"], inp["uprev"], inp["gprev"], inp["gamma"],
                                             inp["beta"], inp["sp1"], inp["shift"], n, R.EPS,
                                             hbias=inp["hbias"])
        put(f"{name}/fwd", u, a, mean, rstd)
        for form, uu, sh in (("u_given", u, None), ("u_recomputed", None, inp["shift"])):
            put(f"{name}/bwd/{form}", *ops.head_film_bwd(
                inp["dh_next"], inp["da16"], uu, inp["h16"], inp["uprev"], inp["gprev"], mean, rstd,
                inp["gamma"], inp["beta"], inp["sp1"], n, want_dh=True, hbias=inp["hbias"], shift=sh))
        if inp["uprev"] is not None:  # the output layer's pair on the same rows
            put(f"{name}/silu_fwd", ops.head_silu_fwd(inp["uprev"], inp["gprev"], n))
            put(f"{name}/silu_bwd", *ops.head_silu_bwd(inp["da16"], inp["uprev"], inp["gprev"], n))

    def forms(shape_name, make):
        """h16 + hbias, h16 alone, (uprev, gprev)."""
        first, later = make(True), make(False)
        film(f"film/{shape_name}/h16_hbias", first)
        film(f"film/{shape_name}/h16", dict(first, hbias=None))
        film(f"film/{shape_name}/uprev_gprev", later)

    def small(b, n, w):
        def make(first):
            inp = R.make_inputs(b, n, w, first)
            return {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in inp.items()}
        return make

    def train(b, n, w):
        def make(first):
            g = gen(1009 * n + w + first)
            rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
            inp = {"b": b, "n": n, "w": w, "h16": None, "hbias": None, "uprev": None, "gprev": None,
                   "gamma": 1.0 + 0.2 * rnd(w), "beta": 0.2 * rnd(w),
                   "sp1": (1.0 + 0.1 * rnd(b, w)).bfloat16(), "shift": (0.1 * rnd(b, w)).bfloat16(),
                   "dh_next": rnd(b * n, w), "da16": rnd(b * n, w).bfloat16()}
            if first:
                inp.update(h16=rnd(b * n, w).bfloat16(), hbias=rnd(b, w))
            else:
                inp.update(uprev=rnd(b * n, w), gprev=rnd(b * n, w).bfloat16())
            return inp
        return make

    for shape in R.SHAPES:
        forms(R.shape_id(shape), small(*shape))
    for s in REDUCE_S:
        for w in (256, 512):
            forms(f"S{s}x{w}", small(1, 256 * s, w))
    for shape in FILM_TRAIN:
        forms(R.shape_id(shape), train(*shape))

    torch.cuda.synchronize()
    with open(out_path, "w") as f:
        json.dump({"lib": tag, "digests": dig}, f, indent=1)
    print(json.dumps({"lib": tag, "digests": len(dig)}), flush=True)
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--diff":
        sys.exit(diff(*sys.argv[2:5]))
    sys.exit(main(*sys.argv[1:3]))
