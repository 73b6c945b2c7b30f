"""float64 autograd references, seeded adverse inputs, error bounds and a float32
emulation of the BatchNorm / GroupNorm passes of csrc/norm.hip (+ bn_chan.hpp).
Shared by tests/test_norm_ref_cpu.py (the emulation through the checks, the
mutations) and tests/test_gpu_norm_ref.py (the kernels through the same checks).

References.  Every reference is a plain forward in float64 differentiated by
torch.autograd, the batch / group statistics computed from x inside the graph:
it shares no algebra with BnChan::dx, the k0 / k1 / k2 coefficients or the bnin
form (one graph: y -> BN -> ReLU -> GroupNorm-FiLM residual).

Bounds.  e = 2^-24 is one fp32 rounding, a 1-ulp intrinsic (rsqrtf, expf) counts
2, -ffp-contract=off makes the expression trees of the source the roundings.
Every bound is a sum of terms k e scale: k roundings on a dependency chain times
the magnitude they act on, every cancelling sum taken by its terms.  K_CAP =
1e-5 / e = 167.8 is the project's cap for a chain; counts(...) returns every k
for a shape and the CPU test holds them to the cap.

  adds of one ordered sum (the shape-dependent part):
    T(L) = ceil(L / 256)   serial adds of one thread walking L float4s
                           (strip_reduce; the apply blocks' per-thread sums)
    block                  6 shuffle adds + 3 wave adds                    =  9
    P                      ordered partials (sum_parts2, gn finalize: 4)
    forward statistics (add_shifted: one add per float4 after a 2-level tree):
      adds_f = 2 + T + 9 + P          BN (1,4,70000): 2+5+9+16 = 32; (17,3,8): 29
                                      GN: P = 4, (2,256,2000,32): 2+4+9+4 = 19
    backward BN statistics (one add per element):  adds_b = 4 T + 9 + P  (<= 45)
    backward GN row sums (tree per float4):        adds_g = 2 + T + 9 + 4 (<= 16)
    SE row sums: 4 T + 9 + PS;  bnpart slot: 4 + 9

  mean   : x - K 1, adds_f, (float)(s / n) 1, K + md 1     k_mean = adds_f + 3
           (<= 35 < cap), scale max |x| of the channel / group.
  var    : q's summand (x - K)^2 carries 3 (relative, all terms positive), so
           q / n: adds_f + 4; md: adds_f + 2 relative to mean |x - K| <=
           sqrt(var + md^2); var = q/n - md md then has
             |d var| <= e (k_q + 2 k_md + 2) (var + md^2)
           i.e. k_var = 3 adds_f + 10 (<= 106 < cap) times the amplification
           A = 1 + (K - mean)^2 / var of the shifted-moment design.
  invstd : relative, k_var / 2 * A * var / (var + eps)  +  3 (+ eps, rsqrtf 2).
           k_is = 1.5 adds_f + 5 + 3 <= 56 < cap.
  producer statistics (bn_fin_parts_kernel, fp64 Chan merges): the inputs are
           fp32 roundings of group means and centred squares; mean k = 3
           (input 1, the fp64 chain 1, the cast 1); var: the between-group term
           carries 2 e |mean_g| |mean_g - mean| per value, so
           A_parts = 1 + 2 sum nb |mean_g| |d_g| / (n var) takes A's place with
           k_var = 1 * A_parts + 2.  (Inherent to fp32 group means.)
  running_mean / running_var: momentum * the bound above + 3 roundings of the
           update by its terms (+ 1 for the cast of var n / (n - 1)); the
           reference is var n / (n - 1) with n = B S: the check that n is right.
  xhat   : dxh = (mean bound + 2 e (|x| + |mean|)) invstd + rel_is |xhat|
           (k_mean + 2 <= 37 on the scale (|x| + |mean|) invstd, + the invstd term)
  pre    : |gamma| dxh + 1 e (|xhat gamma| + |beta|)  (the fma) -- this is `margin`,
           the kink construction's distance;  y / z: + 1 e |z| (the slope).
  BN sums (k_s = summand + adds): dbeta 1 + adds_b; dgamma 2 + adds_b, + sum |g| dxh
           (<= 47 < cap, then xhat's own chain 37: 84 in all < cap).
  BN dx  : |gamma is| [ (6 e + rel_is) T + d mg + |xhat| d mgx + MGX dxh ],
           T = |g| + |mg| + |xhat mgx| by terms, d mg = dbeta bound / n + 2 e MG.
           Longest chain: k_mean + 2 (xhat) + 2 + adds_b (sgx) + 2 (mgx) + 6
           = adds_f + adds_b + 15 <= 92 < cap.
  dbias_in: sum of the dx bounds (the errors of mg / mgx are common to a channel
           and add linearly) + adds of the block sums and the finalize.
  split  : hi + lo decoded; + 2^-16 |v| for the pair.
  GroupNorm forward: a = rstd w (1), s = bias - mean a (2), u = fma(x, a, s) (1):
           du = |w| dxh + 3 e (|x a| + |mean a| + |bias|); FiLM residual out:
           |1 + gamma| du + 5 e (|x| + U |1 + gamma| + |beta|); SiLU out:
           1.1 du + 6 e |SiLU(u)| (expf 2, 1 + . 1, division 1, slack 2).
  GroupNorm backward: A2 = sum d, A3 = sum d xhat per (b, c) row: adds_g (+ 3 for
           A3's product and tree) and sum |d| dxh; the SiLU head's d = dout SiLU'(u)
           carries |dout| (0.5 du + 33 e) (SiLU' as head_film_ref counts it) + 1.
           dbeta = A2; dgamma[b, c] = w A3 + bias A2: + 3; dw, dbias: + B + 2.
           k1, k2: product w g1 a 3, the cpg-long serial loop of
           gn_bwd_finalize_kernel cpg, rstd * . * inv_d 3: cpg + 6, + rel_rstd.
           dx: |d| dk0 + dk1 + |xhat| dk2 + |k2| dxh + 5 e (|d| + |d k0| + |k1| +
           |xhat k2|).  Longest chain: k_mean + 2 + 3 + adds_g + cpg + 6 + 5
           = adds_f + adds_g + cpg + 19.  At the product's grouping (cpg = 8,
           (2,256,2000,32)) that is 62; at cpg = 128 ((2,128,36,1), one group of
           128 channels, a grouping no model here uses) it is 180 > K_CAP: the
           serial group loop is the excess (a tree would be 7).  It is reported,
           not hidden: ABOVE_CAP lists the shape, the bound keeps the count.
  bnin   : the GroupNorm reads z' = z + dz_in with dz_in the BatchNorm's y bound:
           mean + max dz_in, rel_rstd + max dz_in * rstd, dxh + dz_in * rstd.
           bnpart slot (b, bx) of channel c: sum of the dz bounds + (4 + 9) e sum |g|
           (second: + 2, + sum |g| dxh_bn), checked per slot (a slot index that
           swaps b and bx only permutes a channel's partials) and reduced per
           channel; bn_act_backward_parts then adds P and goes on as BN dx with the
           input perturbation dz bound.

A count is a bound only to first order and only while the summation error is
measured against the sum of term magnitudes, which is how every scale here is
formed; tests/test_norm_ref_cpu.py runs the float32 emulation below (the
kernels' expression trees and summation orders) through the same checks on the
same inputs at every shape.  No k was set from a measured error.

Activation kink.  make_inputs moves every element whose reference
pre-activation lies within `margin` (the pre bound above, per channel) of 0 away
by 4 margin / |gamma invstd|, recomputes, repeats, and asserts that none is left
and that at most 1e-3 of the elements were moved.
"""
import functools
import zlib

import torch
import torch.nn.functional as F

E = 2.0 ** -24
K_CAP = 1e-5 / E
MOM = 0.1
NBT0 = 3
MOVED_CAP = 1e-3
SLOPE32 = float(torch.tensor(0.1, dtype=torch.float32))  # LeakyReLU's slope as the kernel sees it
K_BN_PARTS, K_APPLY_U, K_BWD_U, K_GN_PARTS = 16, 4, 2, 4  # norm.hip's constants

# BatchNorm contiguous (b, c, *spatial)
SHAPES_BN = [
    (1, 1, 4),           # one float4, 15 of 16 statistics parts empty, n = 4
    (3, 5, 36),          # P = 18, 6 parts per 9-float4 row (last empty); C % 4 != 0 in the bias finalize
    (17, 3, 8),          # b > 16: one part per row, sum_parts2 = two 8-wide rounds + a tail of one
    (2, 6, 4100),        # S4 = 1025: one-float4 second forward / third backward block, through bn_rev
    (1, 4, 70000),       # parts of 1094 float4s: strip_reduce's unrolled loop, then its tail; 18 apply blocks
    (2, 64, 4, 4, 4),    # 5-D; smallest split form: one 64-channel tile, one 64-voxel tile
    (1, 128, 8, 8, 8),   # 5-D; two channel tiles, eight voxel tiles; bias finalize block kernel nch = 8
]
SHAPES_SPLIT = SHAPES_BN[5:]
# SE forms: the split shapes + the smallest row with two statistics parts per row
SHAPES_SE = SHAPES_SPLIT + [(1, 64, 20, 20, 20)]  # S4 = 2000: se_stat_parts = 2
# BatchNorm from producer statistics (b, c, s, gsz)
SHAPES_BN_PARTS = [
    (1, 3, 64, 64),       # P = 1
    (2, 5, 100, 64),      # P = 4, ragged last group of 36
    (2, 5, 100, 32),      # P = 8, ragged last group of 4
    (3, 4, 44, 32),       # ragged last group of 12
    (2, 2, 33280, 64),    # P = 1040: one 4-at-a-time round, then the tail loop in 16 threads only
    (2, 2, 33280, 32),    # P = 2080: two 4-at-a-time rounds, then the tail in 32 threads
]
BWD_PARTS_P = (1, 7, 8, 17)  # bn_act_backward_parts: partials over a fixed partition
BWD_PARTS_SHAPES = [(3, 5, 36), (2, 6, 4100)]
# GroupNorm (b, c, n, groups), each for the FiLM residual, the SiLU head and the bnin form
SHAPES_GN = [
    (1, 4, 4, 4),         # cpg = 1, tot = 1, three of four parts empty
    (3, 6, 36, 3),        # C % 4 != 0, cpg = 2, b = 3
    (2, 128, 36, 1),      # one group of 128 channels, N4 = 9: a thread's next float4 is 28 channels on
    (2, 8, 1028, 2),      # N4 = 257: a one-float4 second apply block; bnin: nbx = 2, P = 4
    (1, 1024, 4, 32),     # C = 1024 fills gn_bwd_finalize_kernel's one block
    (2, 256, 2000, 32),   # the product's grouping at a size where the sums are long
]
KINDS = ("offset", "first_out")
# chains above K_CAP (explained in the docstring): (family, shape) -> count
ABOVE_CAP = {("gn", (2, 128, 36, 1)): "gn_dx_chain"}


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def _cdiv(a, b):
    return -(-a // b)


def bn_parts(b):
    return b * _cdiv(K_BN_PARTS, b)


def se_stat_parts(b, c, s):
    return min(max(1, _cdiv(s // 4, 1024)), max(1, _cdiv(2048, b * c)))


def strip_T(L):
    return max(1, _cdiv(L, 256))


def counts(family, shape):
    """Every rounding count of the docstring for one shape."""
    if family == "bn":
        b, c = shape[0], shape[1]
        s = 1
        for d in shape[2:]:
            s *= d
        P = bn_parts(b)
        T = strip_T(_cdiv(s // 4, P // b))
        adds_f, adds_b = 2 + T + 9 + P, 4 * T + 9 + P
        nch = _cdiv(s // 4, 256 * K_BWD_U)
        k = {"adds_f": adds_f, "adds_b": adds_b, "k_mean": adds_f + 3, "k_var": 3 * adds_f + 10,
             "k_is": 1.5 * adds_f + 8, "k_xhat": adds_f + 5, "k_dbeta": 1 + adds_b,
             "k_dgamma": 2 + adds_b + adds_f + 5, "bn_dx_chain": adds_f + adds_b + 15,
             "adds_rowmean": 2 + K_APPLY_U + 9 + _cdiv(s // 4, 256 * K_APPLY_U) + 1,
             "adds_dbias": 2 + K_BWD_U + 9 + _cdiv(b * nch, 64) + 6,
             "adds_dbias_split": 16 + 2 + b * _cdiv(max(1, s // 64), 256) + 9,
             "adds_se": 4 * strip_T(_cdiv(s // 4, se_stat_parts(b, c, s))) + 9
             + se_stat_parts(b, c, s) + b + 2}
        return k
    b, c, n, groups = shape
    cpg = c // groups
    T = strip_T(_cdiv(cpg * (n // 4), K_GN_PARTS))
    adds_f = 2 + T + 9 + K_GN_PARTS
    adds_g = 2 + strip_T(_cdiv(n // 4, K_GN_PARTS)) + 9 + K_GN_PARTS
    return {"adds_f": adds_f, "adds_g": adds_g, "k_mean": adds_f + 3, "k_var": 3 * adds_f + 10,
            "k_is": 1.5 * adds_f + 8, "k_xhat": adds_f + 5, "k_a3": adds_g + 3 + adds_f + 5,
            "k_group": cpg + 6, "k_dw": b + 2, "gn_dx_chain": adds_f + adds_g + cpg + 19,
            "k_bnpart": 4 + 9 + 2}


# ---------------------------------------------------------------------------
# float64 forward quantities (no autograd): used by the kink construction, the
# scales and the bounds
# ---------------------------------------------------------------------------
def _flat3(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


def _act(pre, slope):
    return torch.where(pre > 0, pre, pre * slope)


def bn_core(x, gamma, beta, eps, slope):
    """x (b, c, s) any float dtype -> float64 forward quantities of act(bn(x))."""
    x = _flat3(x).double()
    g, bt = gamma.double()[None, :, None], beta.double()[None, :, None]
    n = x.shape[0] * x.shape[2]
    mean = x.mean((0, 2))
    var = x.var((0, 2), unbiased=False)
    invstd = (var + eps).rsqrt()
    xhat = (x - mean[None, :, None]) * invstd[None, :, None]
    pre = xhat * g + bt
    K = x[0, :, 0]
    return {"x": x, "n": n, "mean": mean, "var": var, "invstd": invstd, "xhat": xhat, "pre": pre,
            "z": _act(pre, slope), "gamma": g, "beta": bt, "eps": eps, "slope": slope,
            "A": 1.0 + (K - mean) ** 2 / var, "vv": var / (var + eps),
            "xmax": x.abs().amax((0, 2))}


def bn_stat_bounds(core, shape3, source="pass", gsz=None):
    """(mean bound [c], relative invstd bound [c], relative var bound [c]) of the
    kernel's statistics.  source: "pass" (bn_stats_kernel), "parts" (producer
    statistics, group size gsz), "given" (fp32 roundings of the reference)."""
    b, c, s = shape3
    if source == "pass":
        k = counts("bn", shape3)
        mean_b = k["k_mean"] * E * core["xmax"]
        relvar = k["k_var"] * E * core["A"]
    elif source == "parts":
        x = core["x"]
        G = _cdiv(s, gsz)
        pad = F.pad(x, (0, G * gsz - s), value=float("nan")).view(b, c, G, gsz)
        nb = (~pad.isnan()).sum(-1).double()
        mg = pad.nansum(-1) / nb
        dg = (mg - core["mean"][None, :, None]).abs()
        a_parts = 1.0 + 2.0 * (nb * mg.abs() * dg).sum((0, 2)) / (core["n"] * core["var"])
        mean_b = 3 * E * core["xmax"]
        relvar = (a_parts + 2.0) * E
    else:
        mean_b = E * core["mean"].abs()
        relvar = torch.zeros_like(core["mean"])
        return mean_b, E * torch.ones_like(mean_b), relvar
    return mean_b, 0.5 * relvar * core["vv"] + 3 * E, relvar


def bn_elem_bounds(core, mean_b, relis, din=None):
    """dxh (the kernel's xhat error), pre_b (`margin`), y_b, elementwise (b, c, s)."""
    x, mean, invstd = core["x"], core["mean"][None, :, None], core["invstd"][None, :, None]
    din = 0.0 if din is None else din
    dxh = ((mean_b[None, :, None] + din + 2 * E * (x.abs() + mean.abs())) * invstd
           + relis[None, :, None] * core["xhat"].abs())
    pre_b = core["gamma"].abs() * dxh + E * ((core["xhat"] * core["gamma"]).abs()
                                             + core["beta"].abs())
    return dxh, pre_b, pre_b + E * core["z"].abs()


def gn_core(x, groups, eps):
    """x (b, c, n) -> float64 group statistics, broadcast per element."""
    x = x.double()
    b, c, n = x.shape
    xg = x.reshape(b, groups, -1)
    mean = xg.mean(2)
    var = xg.var(2, unbiased=False)
    rstd = (var + eps).rsqrt()
    K = xg[:, :, 0]
    cpg = c // groups
    per = lambda t: t.repeat_interleave(cpg, 1)[:, :, None]  # noqa: E731  (b, G) -> (b, c, 1)
    return {"x": x, "mean": mean, "var": var, "rstd": rstd, "cpg": cpg, "groups": groups,
            "mean_e": per(mean), "rstd_e": per(rstd), "xhat": (x - per(mean)) * per(rstd),
            "A": 1.0 + (K - mean) ** 2 / var, "vv": var / (var + eps),
            "xmax": xg.abs().amax(2), "per": per}


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def _gen(entry, shape, kind, salt):
    return torch.Generator().manual_seed(
        zlib.crc32(repr((entry, tuple(shape), kind, salt)).encode()))


def _signed(g, *s):
    """magnitudes in [0.5, 1.5], random sign"""
    mag = 0.5 + torch.rand(*s, generator=g)
    return torch.where(torch.rand(*s, generator=g) < 0.5, -mag, mag)


def _offset_data(g, b, c, s):
    mean = 100.0 * torch.rand(c, generator=g) - 50.0
    std = 0.05 + 1.95 * torch.rand(c, generator=g)
    return mean[None, :, None] + std[None, :, None] * torch.randn(b, c, s, generator=g)


def pair16(x):
    """x rounded to what a bf16 hi / lo pair holds exactly (16 significant bits)."""
    hi = x.bfloat16().float()
    return hi + (x - hi).bfloat16().float()


def _clear_kink(x, eval_fn, quant=False):
    """Move the elements of x (b, c, s) fp32 whose reference pre-activation lies
    within margin of 0 away from it.  eval_fn(x) -> (pre, margin, dpre_dx), float64,
    elementwise / broadcastable.  Returns (x, moved share).  quant: x stays on
    pair16's grid (a move is at least one step of it)."""
    moved = torch.zeros(x.shape, dtype=torch.bool)
    for _ in range(50):
        pre, margin, slope_x = eval_fn(x)
        bad = pre.abs() < margin
        if not bool(bad.any()):
            break
        step = torch.where(pre >= 0, 1.0, -1.0) * 4.0 * margin / slope_x
        if quant:
            step = torch.sign(step) * torch.maximum(step.abs(), 2.0 ** -14 * x.double().abs())
        new = (x.double() + step).float()
        x = torch.where(bad, pair16(new) if quant else new, x)
        moved |= bad
    pre, margin, _ = eval_fn(x)
    assert not bool((pre.abs() < margin).any()), "kink: ambiguous elements left"
    return x, float(moved.double().mean())


def _bn_kink_eval(gamma, beta, eps, slope, shape3, source, gsz):
    def f(x):
        core = bn_core(x, gamma, beta, eps, slope)
        mean_b, relis, _ = bn_stat_bounds(core, shape3, source, gsz)
        _, pre_b, _ = bn_elem_bounds(core, mean_b, relis)
        margin = pre_b.amax((0, 2), keepdim=True)
        return core["pre"], margin.expand_as(core["pre"]), core["gamma"] * core["invstd"][None, :, None]
    return f


@functools.lru_cache(maxsize=None)
def make_inputs(entry, shape, kind):
    """Seeded CPU inputs; treat as read-only.  entry: "bn" (shape (b, c, *spatial)),
    "bn_parts" ((b, c, s, gsz)), "gn_film", "gn_silu", "bnin" ((b, c, n, groups)),
    "bnin_q" (bnin with y on pair16's grid: a 1x1 conv carrying the identity then
    reproduces it exactly through the bf16 hi / lo GEMM).
    In a channel of a few hundred values one moved element is above the 1e-3 cap:
    the seed's salt counts up until the construction meets the cap (the inputs
    change, never the cap); the cap itself is asserted."""
    for salt in range(16):
        inp = _make_inputs(entry, shape, kind, salt)
        if inp["moved"] <= MOVED_CAP:
            break
    assert inp["moved"] <= MOVED_CAP, f"kink: moved share {inp['moved']}"
    return inp


def _make_inputs(entry, shape, kind, salt):
    assert kind in KINDS
    g = _gen(entry, shape, kind, salt)
    sig = {"offset": 0.0, "first_out": 6.0}[kind]  # the first element's distance, in sigma
    if entry in ("bn", "bn_parts"):
        gsz = shape[3] if entry == "bn_parts" else None
        full = tuple(shape[:3]) if entry == "bn_parts" else tuple(shape)
        b, c = full[0], full[1]
        s = 1
        for d in full[2:]:
            s *= d
        five_d = len(full) == 5
        eps, slope = (1e-4, SLOPE32) if five_d else (1e-5, 0.0)
        x = _offset_data(g, b, c, s)
        gamma, beta = _signed(g, c), torch.rand(c, generator=g) - 0.5
        if sig:
            flat = x.double().permute(1, 0, 2).reshape(c, -1)[:, 1:]
            sd = flat.std(1, unbiased=False) if flat.shape[1] > 1 else torch.ones(c, dtype=torch.float64)
            sign = torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0).double()
            x[0, :, 0] = (flat.mean(1) + sign * sig * sd).float()
        x, share = _clear_kink(x, _bn_kink_eval(gamma, beta, eps, slope, (b, c, s),
                                                "parts" if gsz else "pass", gsz))
        inp = {"entry": entry, "shape": full, "b": b, "c": c, "s": s, "gsz": gsz, "eps": eps,
               "slope": slope, "x": x.reshape(full).contiguous(), "gamma": gamma, "beta": beta,
               "dz": torch.randn(full, generator=g),
               "rm": 2.0 * torch.rand(c, generator=g) - 1.0, "rv": 0.5 + torch.rand(c, generator=g),
               "se_s": torch.rand(b, c, generator=g), "dmv": 1e-2 * torch.randn(b, c, generator=g),
               "moved": share}
        return inp
    b, c, n, groups = shape
    cpg = c // groups
    inp = {"entry": entry, "shape": shape, "b": b, "c": c, "n": n, "groups": groups,
           "eps": 1e-5 if entry == "gn_silu" else 1e-6,
           "w": _signed(g, c), "bias": torch.rand(c, generator=g) - 0.5,
           "gamma": 0.3 * torch.randn(b, c, generator=g), "beta": 0.3 * torch.randn(b, c, generator=g),
           "dout": torch.randn(b, c, n, generator=g), "moved": 0.0}
    x = _offset_data(g, b, c, n)
    if not entry.startswith("bnin"):
        if sig:
            xg = x.double().reshape(b, groups, -1)
            rest = xg[:, :, 1:]
            sd = rest.std(2, unbiased=False) if rest.shape[2] > 1 else torch.ones(b, groups, dtype=torch.float64)
            mu = rest.mean(2) if rest.shape[2] > 0 else xg[:, :, 0]
            sign = torch.where(torch.rand(b, groups, generator=g) < 0.5, -1.0, 1.0).double()
            x.view(b, groups, -1)[:, :, 0] = (mu + sign * sig * sd).float()
        inp["x"] = x
        return inp
    # bnin: y is the post SharedMLP's conv output; BN1d (eps 1e-5) + ReLU, then GroupNorm
    bn_gamma, bn_beta = _signed(g, c), torch.rand(c, generator=g) - 0.5
    y = x
    if sig:
        for _ in range(4):
            core = bn_core(y, bn_gamma, bn_beta, 1e-5, 0.0)
            zg = core["z"].reshape(b, groups, -1)
            rest = zg[:, :, 1:]
            sd = rest.std(2, unbiased=False) if rest.shape[2] > 1 else torch.ones(b, groups, dtype=torch.float64)
            mu = rest.mean(2) if rest.shape[2] > 0 else zg[:, :, 0]
            z0 = mu + sig * sd.clamp_min(1e-3) + 1e-3  # > 0: the ReLU passes it
            c0 = torch.arange(groups) * cpg
            xh0 = (z0 - bn_beta.double()[c0]) / bn_gamma.double()[c0]
            y0 = core["mean"][c0] + xh0 / core["invstd"][c0]
            y = y.clone()
            y[:, c0, 0] = y0.float()
    quant = entry == "bnin_q"
    if quant:
        y = pair16(y)
    y, share = _clear_kink(y, _bn_kink_eval(bn_gamma, bn_beta, 1e-5, 0.0, (b, c, n), "pass", None),
                           quant)
    inp.update({"y": y, "bn_gamma": bn_gamma, "bn_beta": bn_beta, "bn_eps": 1e-5, "slope": 0.0,
                "rm": 2.0 * torch.rand(c, generator=g) - 1.0, "rv": 0.5 + torch.rand(c, generator=g),
                "moved": share})
    return inp


def synth_group_stats(x, gsz):
    """The producer's epilogue statistics of x (b, c, s): float32 (c, P, 2) of each
    group's float64 mean and centred sum of squares, group p = b * G + j."""
    x = _flat3(x).double()
    b, c, s = x.shape
    G = _cdiv(s, gsz)
    out = torch.empty(c, b * G, 2, dtype=torch.float64)
    for j in range(G):
        seg = x[:, :, j * gsz:min(s, (j + 1) * gsz)]
        m = seg.mean(2)
        out[:, j::G, 0] = m.t()
        out[:, j::G, 1] = ((seg - m[:, :, None]) ** 2).sum(2).t()
    return out.float()


def bwd_partition(b, s, P):
    """A fixed partition of the (b, s) positions of a channel into P sets (by
    position index modulo P, scrambled): (b, s) int64 labels."""
    idx = torch.arange(b * s, dtype=torch.int64)
    return ((idx * 7 + idx // 5) % P).view(b, s)


# ---------------------------------------------------------------------------
# float64 autograd references (+ the scales and bounds the checks use)
# ---------------------------------------------------------------------------
def _bn_sums_bounds(core, dxh, gabs, ddz, adds, P_extra=0):
    """Bounds of dbeta = sum g, dgamma = sum g xhat per channel (summands: 1 / 2
    roundings; ddz: the bound of the incoming gradient's own error) and their
    term sums MG, MGX (per value)."""
    n = core["n"]
    xh = core["xhat"].abs()
    sg, sgx = gabs.sum((0, 2)), (gabs * xh).sum((0, 2))
    dbeta_b = (1 + adds + P_extra) * E * sg + ddz.sum((0, 2))
    dgamma_b = ((2 + adds + P_extra) * E * sgx + (gabs * dxh).sum((0, 2))
                + (ddz * xh).sum((0, 2)))
    return dbeta_b, dgamma_b, sg / n, sgx / n


def _bn_dx_bound(core, dxh, relis, gabs, ddz, dbeta_b, dgamma_b, MG, MGX):
    n = core["n"]
    xh = core["xhat"].abs()
    bc = lambda t: t[None, :, None]  # noqa: E731
    dmg = bc(dbeta_b / n + 2 * E * MG)
    dmgx = bc(dgamma_b / n + 2 * E * MGX)
    T = gabs + bc(MG) + xh * bc(MGX)
    gi = (core["gamma"] * bc(core["invstd"])).abs()
    return gi * ((6 * E + bc(relis)) * T + dmg + xh * dmgx + bc(MGX) * dxh + ddz), gi * T


@functools.lru_cache(maxsize=4)
def bn_ref(entry, shape, kind, source="pass"):
    """Reference of the BatchNorm forms on make_inputs(entry, shape, kind).
    source: where the kernel's statistics come from (selects the statistics bound)."""
    inp = make_inputs(entry, shape, kind)
    b, c, s, eps, slope = inp["b"], inp["c"], inp["s"], inp["eps"], inp["slope"]
    x = _flat3(inp["x"]).double().requires_grad_(True)
    gamma = inp["gamma"].double().requires_grad_(True)
    beta = inp["beta"].double().requires_grad_(True)
    bias_in = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    xe = x + bias_in[None, :, None]
    mean = xe.mean((0, 2))
    var = xe.var((0, 2), unbiased=False)
    pre = (xe - mean[None, :, None]) / (var[None, :, None] + eps).sqrt() * gamma[None, :, None] \
        + beta[None, :, None]
    z = _act(pre, slope)
    dz = _flat3(inp["dz"]).double()
    dx, dgamma, dbeta, dbias_in = torch.autograd.grad((dz * z).sum(), [x, gamma, beta, bias_in],
                                                      retain_graph=True)
    # SE composition: dz = g s[b, c] + dmv[b, c]
    dz_se = dz * inp["se_s"].double()[:, :, None] + inp["dmv"].double()[:, :, None]
    se_dx, se_dgamma, se_dbeta, se_dbias_in = torch.autograd.grad(
        (dz_se * z).sum(), [x, gamma, beta, bias_in])
    n = b * s
    core = bn_core(inp["x"], inp["gamma"], inp["beta"], eps, slope)
    mean_b, relis, relvar = bn_stat_bounds(core, (b, c, s), source, inp["gsz"])
    dxh, pre_b, y_b = bn_elem_bounds(core, mean_b, relis)
    a = torch.where(core["pre"] > 0, 1.0, slope).double()
    k = counts("bn", (b, c, s))
    rm0, rv0 = inp["rm"].double(), inp["rv"].double()
    varu = core["var"] * n / (n - 1) if n > 1 else core["var"] * float("nan")
    ref = {"core": core, "inp": inp, "k": k, "n": n, "a": a,
           "z": z.detach(), "mean": core["mean"], "invstd": core["invstd"],
           "mean_b": mean_b, "relis": relis, "dxh": dxh, "pre_b": pre_b, "y_b": y_b,
           "running_mean": (1 - MOM) * rm0 + MOM * core["mean"],
           "running_mean_b": MOM * mean_b + 3 * E * ((1 - MOM) * rm0.abs() + MOM * core["mean"].abs()),
           "running_var": (1 - MOM) * rv0 + MOM * varu,
           "running_var_b": MOM * relvar * varu + 4 * E * ((1 - MOM) * rv0.abs() + MOM * varu),
           "dx": dx, "dgamma": dgamma, "dbeta": dbeta, "dbias_in": dbias_in,
           "se_dx": se_dx, "se_dgamma": se_dgamma, "se_dbeta": se_dbeta,
           "se_dbias_in": se_dbias_in, "dz_se": dz_se}
    zabs = core["z"].abs()
    ref["rowmean"] = core["z"].mean(2)
    ref["rowmean_b"] = (y_b.sum(2) + k["adds_rowmean"] * E * zabs.sum(2)) / s
    # plain backward
    g = dz * a
    gabs = g.abs()
    zero = torch.zeros_like(gabs)
    db_b, dg_b, MG, MGX = _bn_sums_bounds(core, dxh, gabs, zero, k["adds_b"])
    ref["dbeta_b"], ref["dgamma_b"] = db_b, dg_b
    ref["dx_b"], ref["dx_terms"] = _bn_dx_bound(core, dxh, relis, gabs, zero, db_b, dg_b, MG, MGX)
    # SE row sums (5, b, c) and the composed backward
    gd, xh = dz, core["xhat"]
    rs = torch.stack([(core["z"] * gd).sum(2), (a * gd).sum(2), a.sum(2), (a * gd * xh).sum(2),
                      (a * xh).sum(2)])
    ase = k["adds_se"]
    rs_b = torch.stack([
        (gd.abs() * y_b).sum(2) + ase * E * (zabs * gd.abs()).sum(2),
        (1 + ase) * E * (a * gd.abs()).sum(2),
        ase * E * a.sum(2),
        (1 + ase) * E * (a * gd.abs() * xh.abs()).sum(2) + (a * gd.abs() * dxh).sum(2),
        ase * E * (a * xh.abs()).sum(2) + (a * dxh).sum(2)])
    ref["rowstats"], ref["rowstats_b"] = rs, rs_b
    sa, ta = inp["se_s"].double().abs()[:, :, None], inp["dmv"].double().abs()[:, :, None]
    gabs_se = a * (sa * gd.abs() + ta)
    ddz_se = a * E * (sa * gd.abs() + ta)
    xha = xh.abs()
    se_db_b = (sa[:, :, 0] * rs_b[1] + ta[:, :, 0] * rs_b[2]).sum(0) + (b + 2) * E * gabs_se.sum((0, 2))
    se_dg_b = (sa[:, :, 0] * rs_b[3] + ta[:, :, 0] * rs_b[4]).sum(0) \
        + (b + 2) * E * (gabs_se * xha).sum((0, 2))
    nn = core["n"]
    ref["se_dbeta_b"], ref["se_dgamma_b"] = se_db_b, se_dg_b
    ref["se_dx_b"], ref["se_dx_terms"] = _bn_dx_bound(
        core, dxh, relis, gabs_se, ddz_se, se_db_b, se_dg_b, gabs_se.sum((0, 2)) / nn,
        (gabs_se * xha).sum((0, 2)) / nn)
    return ref


def bn_bwd_parts_ref(shape, kind, P):
    """bn_act_backward_parts on given statistics: mean / invstd are the fp32
    roundings of the reference's, part (c, P, 2) the fp32 roundings of float64
    partial sums over bwd_partition."""
    inp = make_inputs("bn", shape, kind)
    full = bn_ref("bn", shape, kind)
    core = full["core"]
    b, c, s = inp["b"], inp["c"], inp["s"]
    mean_b, relis, _ = bn_stat_bounds(core, (b, c, s), "given")
    dxh, pre_b, _ = bn_elem_bounds(core, mean_b, relis)
    assert bool((core["pre"].abs() >= pre_b).all())  # the pass margin covers this one
    g = _flat3(inp["dz"]).double() * full["a"]
    lab = bwd_partition(b, s, P)
    part = torch.zeros(c, P, 2, dtype=torch.float64)
    for p in range(P):
        m = (lab == p)[:, None, :]
        part[:, p, 0] = (g * m).sum((0, 2))
        part[:, p, 1] = (g * core["xhat"] * m).sum((0, 2))
    gabs = g.abs()
    n = core["n"]
    sg, sgx = gabs.sum((0, 2)), (gabs * core["xhat"].abs()).sum((0, 2))
    # the partials are exact sums rounded once; the kernel adds P of them
    db_b, dg_b = (P + 1) * E * sg, (P + 1) * E * sgx
    dx_b, dx_terms = _bn_dx_bound(core, dxh, relis, gabs, torch.zeros_like(gabs), db_b, dg_b,
                                  sg / n, sgx / n)
    return {"inp": inp, "part": part.float(), "mean32": core["mean"].float(),
            "invstd32": core["invstd"].float(), "dx": full["dx"], "dgamma": full["dgamma"],
            "dbeta": full["dbeta"], "dbias_in": full["dbias_in"], "dx_b": dx_b,
            "dx_terms": dx_terms, "dbeta_b": db_b, "dgamma_b": dg_b, "k": full["k"], "core": core}


def _gn_bounds(core, inp_w, inp_bias, g1, bt, dout, k, silu, mean_b, relis, din, b):
    """Bounds of the GroupNorm forward / backward outputs (docstring)."""
    x, xh = core["x"], core["xhat"].abs()
    per = core["per"]
    rs, me = core["rstd_e"], core["mean_e"]
    w, bias = inp_w.double()[None, :, None], inp_bias.double()[None, :, None]
    cpg, n = core["cpg"], x.shape[2]
    dxh = (per(mean_b) + din + 2 * E * (x.abs() + me.abs())) * rs + per(relis) * xh
    a = rs * w
    U = (x * a).abs() + (me * a).abs() + bias.abs()
    du = w.abs() * dxh + 3 * E * U
    u = core["xhat"] * w + bias
    out = {"dxh": dxh, "du": du}
    if silu:
        out["out_b"] = 1.1 * du + 6 * E * F.silu(u).abs()
        sg = torch.sigmoid(u)
        dsilu = sg * (1 + u * (1 - sg))
        dy = dout * dsilu
        dabs = dy.abs()
        dd = dout.abs() * (0.5 * du + 33 * E) + E * dabs
    else:
        out["out_b"] = din + g1.abs() * du + 5 * E * (x.abs() + U * g1.abs() + bt.abs())
        dabs, dd = dout.abs(), torch.zeros_like(x)
    A2abs, A3abs = dabs.sum(2), (dabs * xh).sum(2)
    A2_b = dd.sum(2) + k["adds_g"] * E * A2abs
    A3_b = (dd * xh + dabs * dxh).sum(2) + (k["adds_g"] + 3) * E * A3abs
    w2, b2, g12 = w[:, :, 0].abs(), bias[:, :, 0].abs(), g1[:, :, 0].abs()
    out.update({"A2abs": A2abs, "A3abs": A3abs,
                "dbeta_b": A2_b, "dgamma_b": w2 * A3_b + b2 * A2_b + 3 * E * (w2 * A3abs + b2 * A2abs),
                "dw_b": (g12 * A3_b).sum(0) + (b + 2) * E * (g12 * A3abs).sum(0),
                "dbias_b": (g12 * A2_b).sum(0) + (b + 2) * E * (g12 * A2abs).sum(0)})
    wg = w2 * g12  # (b, c)
    grp = lambda t: per(t.reshape(b, core["groups"], cpg).sum(2))  # noqa: E731
    scale = rs / (cpg * n)
    K1abs, K2abs = scale * grp(wg * A2abs), scale * grp(wg * A3abs)
    kg = (cpg + 6) * E + per(relis)
    dk1 = scale * grp(wg * A2_b) + kg * K1abs
    dk2 = scale * grp(wg * A3_b) + kg * K2abs
    k0 = (rs * g1 * w).abs()
    dk0 = (3 * E + per(relis)) * k0
    if silu:
        out["dx_b"] = k0 * dd + dabs * dk0 + dk1 + xh * dk2 + K2abs * dxh \
            + 4 * E * (dabs * k0 + K1abs + xh * K2abs)
        out["dx_terms"] = dabs * k0 + K1abs + xh * K2abs
    else:
        out["dx_b"] = dout.abs() * dk0 + dk1 + xh * dk2 + K2abs * dxh \
            + 5 * E * (dout.abs() + dabs * k0 + K1abs + xh * K2abs)
        out["dx_terms"] = dout.abs() + dabs * k0 + K1abs + xh * K2abs
    return out


@functools.lru_cache(maxsize=4)
def gn_ref(entry, shape, kind):
    """entry "gn_film": x + GN(x)(1 + gamma) + beta; "gn_silu": SiLU(GN(x))."""
    inp = make_inputs(entry, shape, kind)
    b, c, n, groups = shape
    silu = entry == "gn_silu"
    x = inp["x"].double().requires_grad_(True)
    w = inp["w"].double().requires_grad_(True)
    bias = inp["bias"].double().requires_grad_(True)
    gamma = inp["gamma"].double().requires_grad_(True)
    beta = inp["beta"].double().requires_grad_(True)
    gn = F.group_norm(x, groups, w, bias, inp["eps"])
    out = F.silu(gn) if silu else x + (gn * (1 + gamma[:, :, None]) + beta[:, :, None])
    dout = inp["dout"].double()
    wrt = [x, w, bias] if silu else [x, w, bias, gamma, beta]
    grads = torch.autograd.grad((dout * out).sum(), wrt)
    core = gn_core(inp["x"], groups, inp["eps"])
    k = counts("gn", shape)
    mean_b = k["k_mean"] * E * core["xmax"]
    relvar = k["k_var"] * E * core["A"]
    relis = 0.5 * relvar * core["vv"] + 3 * E
    g1 = torch.ones(b, c, 1, dtype=torch.float64) if silu else 1 + inp["gamma"].double()[:, :, None]
    bt = torch.zeros(b, c, 1, dtype=torch.float64) if silu else inp["beta"].double()[:, :, None]
    bounds = _gn_bounds(core, inp["w"], inp["bias"], g1, bt, dout, k, silu, mean_b, relis, 0.0, b)
    ref = {"inp": inp, "core": core, "k": k, "out": out.detach(), "mean": core["mean"],
           "rstd": core["rstd"], "mean_b": mean_b, "relis": relis,
           "dx": grads[0], "dw": grads[1], "dbias": grads[2]}
    if not silu:
        ref["dgamma"], ref["dbeta"] = grads[3], grads[4]
    ref.update(bounds)
    return ref


@functools.lru_cache(maxsize=4)
def bnin_ref(shape, kind, entry="bnin"):
    """One graph: z = ReLU(BN(y)), out = z + GN(z)(1 + gamma) + beta; gradients with
    respect to y, both norms' affine parameters, gamma, beta and the conv bias."""
    inp = make_inputs(entry, shape, kind)
    b, c, n, groups = shape
    y = inp["y"].double().requires_grad_(True)
    bg = inp["bn_gamma"].double().requires_grad_(True)
    bb = inp["bn_beta"].double().requires_grad_(True)
    bias_in = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    w = inp["w"].double().requires_grad_(True)
    bias = inp["bias"].double().requires_grad_(True)
    gamma = inp["gamma"].double().requires_grad_(True)
    beta = inp["beta"].double().requires_grad_(True)
    ye = y + bias_in[None, :, None]
    m = ye.mean((0, 2))
    v = ye.var((0, 2), unbiased=False)
    pre = (ye - m[None, :, None]) / (v[None, :, None] + inp["bn_eps"]).sqrt() * bg[None, :, None] \
        + bb[None, :, None]
    z = torch.relu(pre)
    out = z + (F.group_norm(z, groups, w, bias, inp["eps"]) * (1 + gamma[:, :, None])
               + beta[:, :, None])
    dout = inp["dout"].double()
    gr = torch.autograd.grad((dout * out).sum(), [y, bg, bb, bias_in, w, bias, gamma, beta, z])
    bcore = bn_core(inp["y"], inp["bn_gamma"], inp["bn_beta"], inp["bn_eps"], 0.0)
    bmean_b, brelis, brelvar = bn_stat_bounds(bcore, (b, c, n), "pass")
    bdxh, bpre_b, by_b = bn_elem_bounds(bcore, bmean_b, brelis)
    a = (bcore["pre"] > 0).double()
    din = by_b * a  # the error of the z the GroupNorm reads (0 where the ReLU cuts)
    core = gn_core(bcore["z"], groups, inp["eps"])
    k = counts("gn", shape)
    dmax = din.reshape(b, groups, -1).amax(2)
    mean_b = k["k_mean"] * E * core["xmax"] + dmax
    relis = 0.5 * k["k_var"] * E * core["A"] * core["vv"] + dmax * core["rstd"] + 3 * E
    g1, bt = 1 + inp["gamma"].double()[:, :, None], inp["beta"].double()[:, :, None]
    gb = _gn_bounds(core, inp["w"], inp["bias"], g1, bt, dout, k, False, mean_b, relis, din, b)
    dz, dz_b = gr[8], gb["dx_b"]
    # the BatchNorm backward partials out of the GroupNorm apply blocks
    nbx = _cdiv(n // 4, 256)
    g = dz * a
    gabs, ddz = gb["dx_terms"] * a, dz_b * a
    xh = bcore["xhat"]
    pad = nbx * 1024 - n
    blk = lambda t: F.pad(t, (0, pad)).view(b, c, nbx, 1024).sum(3).permute(1, 0, 2).reshape(c, b * nbx)  # noqa: E731
    slot = torch.stack([blk(g), blk(g * xh)], 2)
    slot_b = torch.stack([blk(ddz) + 13 * E * blk(gabs),
                          blk(ddz * xh.abs() + gabs * bdxh) + 15 * E * blk(gabs * xh.abs())], 2)
    P = b * nbx
    nn = bcore["n"]
    db_b = slot_b[:, :, 0].sum(1) + P * E * gabs.sum((0, 2))
    dg_b = slot_b[:, :, 1].sum(1) + P * E * (gabs * xh.abs()).sum((0, 2))
    dy_b, dy_terms = _bn_dx_bound(bcore, bdxh, brelis, gabs, ddz, db_b, dg_b,
                                  gabs.sum((0, 2)) / nn, (gabs * xh.abs()).sum((0, 2)) / nn)
    rm0, rv0 = inp["rm"].double(), inp["rv"].double()
    varu = bcore["var"] * nn / (nn - 1)
    kb = counts("bn", (b, c, n))
    ref = {"inp": inp, "core": core, "bcore": bcore, "k": k, "kb": kb, "out": out.detach(),
           "mean": core["mean"], "rstd": core["rstd"], "mean_b": mean_b, "relis": relis,
           "bn_mean": bcore["mean"], "bn_invstd": bcore["invstd"], "bn_mean_b": bmean_b,
           "bn_relis": brelis,
           "running_mean": (1 - MOM) * rm0 + MOM * bcore["mean"],
           "running_mean_b": MOM * bmean_b + 3 * E * ((1 - MOM) * rm0.abs() + MOM * bcore["mean"].abs()),
           "running_var": (1 - MOM) * rv0 + MOM * varu,
           "running_var_b": MOM * brelvar * varu + 4 * E * ((1 - MOM) * rv0.abs() + MOM * varu),
           "dy": gr[0], "bn_dgamma": gr[1], "bn_dbeta": gr[2], "dbias_in": gr[3], "dw": gr[4],
           "dbias": gr[5], "dgamma": gr[6], "dbeta": gr[7], "dz": dz, "dz_b": dz_b,
           "dz_terms": gb["dx_terms"], "slot": slot, "slot_b": slot_b,
           "bn_dbeta_b": db_b, "bn_dgamma_b": dg_b, "dy_b": dy_b, "dy_terms": dy_terms}
    for key in ("out_b", "dbeta_b", "dgamma_b", "dw_b", "dbias_b"):
        ref[key] = gb[key]
    return ref


# ---------------------------------------------------------------------------
# ratios (error / bound; <= 1 passes; NaN fails)
# ---------------------------------------------------------------------------
def _ratio(got, ref, bound):
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    err = (got.double() - ref).abs()
    # a bound of 0 (a sum whose every summand the ReLU cuts) asks for the exact value
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, 0.0, float("inf")).double())
    return float(r.max()) if bool(torch.isfinite(r).all()) else float("nan")


def _row_ratio(got, ref, bound, dims):
    """max |got - ref| over dims against the bound's max over dims (k e scale_row)."""
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    err, bnd = (got.double() - ref).abs().amax(dims), bound.amax(dims)
    r = torch.where(bnd > 0, err / bnd, torch.where(err == 0, 0.0, float("inf")).double())
    return float(r.max()) if bool(torch.isfinite(r).all()) else float("nan")


class _Notes:
    def __init__(self, rec):
        self.rec, self.bad = rec, []

    def __call__(self, name, ratio, cap=1.0):
        self.rec(name, ratio)
        if not ratio <= cap:
            self.bad.append((name, ratio, cap))

    def done(self):
        assert not self.bad, self.bad


def unsplit(buf, b, c, s):
    """Decode a conv split operand (channels-last rows, [hi 32 | lo 32] bf16 per
    32-channel group) to float64 (b, c, s) = hi + lo."""
    t = buf.view(torch.bfloat16).view(b * s, c // 32, 2, 32).double()
    return (t[:, :, 0] + t[:, :, 1]).reshape(b, s, c).permute(0, 2, 1).contiguous()


def dbias_adds(k, b, c, s, split):
    return k["adds_dbias_split"] if split else k["adds_dbias"]


def check_bn_stats(out, ref, rec, prefix=""):
    """mean, invstd, the running pair and the counter."""
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    if "mean" in out:  # (a module wrapper keeps them to itself)
        note("mean", _ratio(out["mean"], ref["mean"], ref["mean_b"]))
        note("invstd", _ratio(out["invstd"], ref["invstd"], ref["relis"] * ref["invstd"]))
    if ref["n"] > 1:
        note("running_mean", _ratio(out["running_mean"], ref["running_mean"], ref["running_mean_b"]))
        note("running_var", _ratio(out["running_var"], ref["running_var"], ref["running_var_b"]))
    note("num_batches_tracked", abs(int(out["nbt"]) - (NBT0 + 1)), 0)
    note.done()


def check_bn_forward(out, ref, rec, prefix=""):
    """y (fp32, or the decoded split pair with out["split"]) and rowmean."""
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    if "y" in out:
        bound = ref["y_b"] + (2.0 ** -16 * ref["z"].abs() if out.get("split") else 0.0)
        note("y", _row_ratio(_flat3(out["y"]), ref["z"], bound, (0, 2)))
    if "rowmean" in out:
        note("rowmean", _ratio(out["rowmean"], ref["rowmean"], ref["rowmean_b"]))
    note.done()


def check_bn_backward(out, ref, rec, prefix="", se=False, split=False):
    """dx (fp32 or decoded split), dgamma, dbeta and dbias_in (when given)."""
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    p = "se_" if se else ""
    dx_b = ref[p + "dx_b"]
    bound = dx_b + (2.0 ** -16 * ref[p + "dx"].abs() if split else 0.0)
    note("dx", _row_ratio(_flat3(out["dx"]), ref[p + "dx"], bound, (0, 2)))
    note("dgamma", _ratio(out["dgamma"], ref[p + "dgamma"], ref[p + "dgamma_b"]))
    note("dbeta", _ratio(out["dbeta"], ref[p + "dbeta"], ref[p + "dbeta_b"]))
    if out.get("dbias_in") is not None:
        core = ref["core"]
        b, c, s = core["x"].shape
        adds = dbias_adds(ref["k"], b, c, s, split)
        bnd = dx_b.sum((0, 2)) + adds * E * ref[p + "dx_terms"].sum((0, 2))
        note("dbias_in", _ratio(out["dbias_in"], ref[p + "dbias_in"], bnd))
    note.done()


def check_se_rowstats(out, ref, rec, prefix=""):
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    for i, nm in enumerate(("ds", "A", "N", "AX", "NX")):
        note("rowstats_" + nm, _ratio(out["rowstats"][i], ref["rowstats"][i], ref["rowstats_b"][i]))
    note.done()


def check_gn_forward(out, ref, rec, prefix=""):
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    if "mean" in out:
        note("mean", _ratio(out["mean"], ref["mean"], ref["mean_b"]))
        note("rstd", _ratio(out["rstd"], ref["rstd"], ref["relis"] * ref["rstd"]))
    note("out", _row_ratio(out["out"], ref["out"], ref["out_b"], 2))
    note.done()


def check_gn_backward(out, ref, rec, prefix="", dx_key="dx"):
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    bkey = "dz_b" if dx_key == "dz" else "dx_b"
    if dx_key in out:
        note(dx_key, _row_ratio(out[dx_key], ref[dx_key], ref[bkey], 2))
    note("dw", _ratio(out["dw"], ref["dw"], ref["dw_b"]))
    note("dbias", _ratio(out["dbias"], ref["dbias"], ref["dbias_b"]))
    if "dgamma" in out:
        note("dgamma", _ratio(out["dgamma"], ref["dgamma"], ref["dgamma_b"]))
        note("dbeta", _ratio(out["dbeta"], ref["dbeta"], ref["dbeta_b"]))
    note.done()


def check_bnin_chain(out, ref, rec, prefix="", dy_pair=False):
    """bnpart per slot and per channel, then bn_act_backward_parts' outputs against
    the one-graph reference.  dy_pair: dy went through a bf16 hi / lo pair (+ 2^-16 |dy|)."""
    note = _Notes(lambda nm, v: rec(prefix + nm, v))
    if "bnpart" in out:
        part = out["bnpart"].double()
        assert tuple(part.shape) == tuple(ref["slot"].shape), (part.shape, ref["slot"].shape)
        note("bnpart_slot", _ratio(part, ref["slot"], ref["slot_b"]))
        note("bnpart_channel", _ratio(part.sum(1), ref["slot"].sum(1), ref["slot_b"].sum(1)))
    pair = 2.0 ** -16 * ref["dy"].abs() if dy_pair else 0.0
    note("dy", _row_ratio(out["dy"], ref["dy"], ref["dy_b"] + pair, (0, 2)))
    note("bn_dgamma", _ratio(out["bn_dgamma"], ref["bn_dgamma"], ref["bn_dgamma_b"]))
    note("bn_dbeta", _ratio(out["bn_dbeta"], ref["bn_dbeta"], ref["bn_dbeta_b"]))
    b, c, n = ref["bcore"]["x"].shape
    bnd = ref["dy_b"].sum((0, 2)) + ref["kb"]["adds_dbias"] * E * ref["dy_terms"].sum((0, 2))
    note("dbias_in", _ratio(out["dbias_in"], ref["dbias_in"], bnd))
    note.done()


# ---------------------------------------------------------------------------
# float32 emulation of the kernels' expression trees and summation orders
# ---------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    """fmaf: the product of two floats is exact in float64."""
    return (a.double() * b.double() + c.double()).float()


def _tree4(v):
    return (v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])


def _block_sum(acc):
    """block_sum2: acc (..., 256) -> (...): xor tree per wave, the 4 waves in order."""
    w = acc.reshape(*acc.shape[:-1], 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[..., :off] + w[..., off:2 * off]
    w = w[..., 0]
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _thread_items(items):
    L, e = items.shape[-2:]
    iters = max(1, _cdiv(L, 256))
    pad = F.pad(items, (0, 0, 0, iters * 256 - L))
    return pad.reshape(*items.shape[:-2], iters, 256, e), iters, e


def _strip(items):
    """strip_reduce's order: items (..., L, E); thread t adds items t, t + 256, ...
    (E per step, in order) to its accumulator; then block_sum2.  Padding adds 0."""
    v, iters, e = _thread_items(items)
    acc = torch.zeros(*v.shape[:-3], 256, dtype=torch.float32)
    for i in range(iters):
        for j in range(e):
            acc = acc + v[..., i, :, j]
    return _block_sum(acc)


def _strip_fma(a, b):
    """the same walk with acc = fmaf(a, b, acc)"""
    va, iters, e = _thread_items(a)
    vb, _, _ = _thread_items(b)
    acc = torch.zeros(*va.shape[:-3], 256, dtype=torch.float32)
    for i in range(iters):
        for j in range(e):
            acc = _fma(va[..., i, :, j], vb[..., i, :, j], acc)
    return _block_sum(acc)


def _part_range(S4, ps, PS):
    chunk = _cdiv(S4, PS)
    return min(S4, chunk * ps), min(S4, chunk * (ps + 1))


def sum_parts2(part, mut=None):
    """part (..., P) -> (...): added in p order from 0; mut "parts_tail": the tail
    loop stops one short."""
    P = part.shape[-1]
    stop = P
    if mut == "parts_tail" and P % 8 != 0:
        stop = P - 1
    s = torch.zeros(part.shape[:-1], dtype=torch.float32)
    for p in range(stop):
        s = s + part[..., p]
    return s


def stat_of_shifted(s, q, n, K, eps, mut=None):
    md = (s.double() / n).float()
    qn = (q.double() / n).float()
    var = torch.clamp_min(qn if mut == "no_md2" else qn - md * md, 0.0)
    return K + md, torch.rsqrt(var + _f32(eps)), var


def _publish(m, var, n, rm, rv, mut=None):
    mom = _f32(MOM)
    varu = var if mut == "biased_running_var" else (var.double() * n / (n - 1.0)).float()
    return (_f32(1.0) - mom) * rm + mom * m, (_f32(1.0) - mom) * rv + mom * varu


def _shifted_parts(x4, K):
    """x4 (..., L, 4), K (...,) -> the block's (sum (x - K), sum (x - K)^2)"""
    d = x4 - K[..., None, None]
    return _strip(_tree4(d)[..., None]), _strip(_tree4(d * d)[..., None])


class BnChan:
    def __init__(self, m, is_, g, bt, slope):
        self.m, self.is_, self.g, self.bt, self.slope = m, is_, g, bt, slope

    def xhat(self, v):
        return (v - self.m) * self.is_

    def pre(self, v):
        return _fma(self.xhat(v), self.g, self.bt)

    def z(self, v):
        t = self.pre(v)
        return torch.where(t > 0, t, torch.zeros_like(t) if self.slope == 0 else t * _f32(self.slope))

    def grad(self, v, dz):
        return torch.where(self.pre(v) > 0, dz, dz * _f32(self.slope))

    def dx(self, v, dz, mg, mgx, mut=None):
        t = self.grad(v, dz) - mg
        if mut != "dx_no_mgx":
            t = t - self.xhat(v) * mgx
        return (self.g * self.is_) * t


def _chan(t):
    return t[None, :, None]


def emulate_bn_stats(x, eps, rm, rv, mut=None):
    """bn_stats_kernel + BnFwdFin::get / publish -> dict(mean, invstd, running pair, nbt)."""
    x = _flat3(x)
    B, C, S = x.shape
    S4, P = S // 4, bn_parts(B)
    PS = P // B
    x4 = x.reshape(B, C, S4, 4)
    K = x[0, :, 0]
    ps_, pq_ = [], []
    for p in range(P):
        b = p // PS
        s0, s1 = _part_range(S4, p - b * PS, PS)
        s, q = _shifted_parts(x4[b, :, s0:s1], K)
        ps_.append(s)
        pq_.append(q)
    s = sum_parts2(torch.stack(ps_, 1), mut)
    q = sum_parts2(torch.stack(pq_, 1), mut)
    n = float(B) * S
    m, is_, var = stat_of_shifted(s, q, n, K, eps, mut)
    rm2, rv2 = _publish(m, var, n, rm, rv, mut) if n > 1 else (rm, rv)
    return {"mean": m, "invstd": is_, "running_mean": rm2, "running_var": rv2, "nbt": NBT0 + 1}


def _chan_merge(n, mu, m2, nb, mb, qb):
    nn = n + nb
    ok = nn > 0
    safe = torch.where(ok, nn, torch.ones_like(nn))
    d = mb - mu
    mu2 = torch.where(ok, mu + d * nb / safe, mu)
    m22 = torch.where(ok, m2 + qb + d * d * n * nb / safe, m2)
    return nn, mu2, m22


def emulate_bn_fin_parts(part, B, S, gsz, eps, rm, rv, mut=None):
    """bn_fin_parts_kernel: part float32 (C, P, 2); thread t merges groups t, t + 256,
    ... in float64, xor tree per wave, waves in order."""
    C, P, _ = part.shape
    G = _cdiv(S, gsz)
    pd = part.double()
    n = torch.zeros(C, 256, dtype=torch.float64)
    mu, m2 = torch.zeros_like(n), torch.zeros_like(n)
    t = torch.arange(256)
    for k in range(_cdiv(P, 256)):
        p = k * 256 + t
        valid = p < P
        pc = torch.where(valid, p, torch.zeros_like(p))
        cnt = torch.full_like(pc, gsz) if mut == "ragged_count" else torch.minimum(
            torch.full_like(pc, gsz), S - (pc % G) * gsz)
        nb = torch.where(valid, cnt, torch.zeros_like(cnt)).double()[None, :]
        n, mu, m2 = _chan_merge(n, mu, m2, nb.expand(C, 256), pd[:, pc, 0], pd[:, pc, 1] * valid)
    n, mu, m2 = (a.reshape(C, 4, 64) for a in (n, mu, m2))
    for off in (32, 16, 8, 4, 2, 1):
        n, mu, m2 = _chan_merge(n[..., :off], mu[..., :off], m2[..., :off], n[..., off:2 * off],
                                mu[..., off:2 * off], m2[..., off:2 * off])
    n, mu, m2 = n[..., 0], mu[..., 0], m2[..., 0]
    an, amu, am2 = n[:, 0], mu[:, 0], m2[:, 0]
    for w in range(1, 4):
        an, amu, am2 = _chan_merge(an, amu, am2, n[:, w], mu[:, w], m2[:, w])
    var = torch.clamp_min((am2 / an).float(), 0.0)
    m = amu.float()
    nn = float(an[0])
    rm2, rv2 = _publish(m, var, nn, rm, rv, mut)
    return {"mean": m, "invstd": torch.rsqrt(var + _f32(eps)), "running_mean": rm2,
            "running_var": rv2, "nbt": NBT0 + 1}


def _split_pair(f):
    hi = f.bfloat16().float()
    return hi.double() + (f - hi).bfloat16().double()


def _apply_blocks(t4, U):
    """t4 (..., S4) per-float4 values -> (..., nblk): each apply block's sum (thread:
    U serial float4s 256 apart; block_sum2)."""
    S4 = t4.shape[-1]
    per = 256 * U
    nblk = _cdiv(S4, per)
    v = F.pad(t4, (0, nblk * per - S4)).reshape(*t4.shape[:-1], nblk, U, 256)
    acc = torch.zeros(*t4.shape[:-1], nblk, 256, dtype=torch.float32)
    for u in range(U):
        acc = acc + v[..., u, :]
    return _block_sum(acc)


def emulate_bn_forward(inp, mut=None, split=False):
    """bn_act_fwd / _rowmean / _split on the pass statistics."""
    x = _flat3(inp["x"])
    B, C, S = x.shape
    st = emulate_bn_stats(x, inp["eps"], inp["rm"], inp["rv"], mut)
    ch = BnChan(_chan(st["mean"]), _chan(st["invstd"]), _chan(inp["gamma"]), _chan(inp["beta"]),
                inp["slope"])
    z = ch.z(x)
    out = dict(st)
    out["y"] = _split_pair(z) if split else z
    out["split"] = split
    rowpart = _apply_blocks(_tree4(z.reshape(B, C, S // 4, 4)), K_APPLY_U)
    rs = torch.zeros(B, C, dtype=torch.float32)
    for kk in range(rowpart.shape[-1]):
        rs = rs + rowpart[..., kk]
    out["rowmean"] = rs * _f32(1.0 / S)
    return out


def _wave_finalize(rowpart):
    """bn_bias_finalize_kernel: rowpart (B, C, nch) -> (C,): lane-strided over
    e = b * nch + k, then a xor tree."""
    B, C, nch = rowpart.shape
    flat = rowpart.permute(1, 0, 2).reshape(C, B * nch)
    it = _cdiv(B * nch, 64)
    v = F.pad(flat, (0, it * 64 - B * nch)).reshape(C, it, 64)
    acc = torch.zeros(C, 64, dtype=torch.float32)
    for i in range(it):
        acc = acc + v[:, i]
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :off] + acc[..., off:2 * off]
    return acc[..., 0]


def _block_finalize(rowpart):
    """bn_bias_finalize_block_kernel: thread-strided over k for each b in turn."""
    B, C, nch = rowpart.shape
    it = _cdiv(nch, 256)
    v = F.pad(rowpart, (0, it * 256 - nch)).reshape(B, C, it, 256)
    acc = torch.zeros(C, 256, dtype=torch.float32)
    for b in range(B):
        for i in range(it):
            acc = acc + v[b, :, i]
    return _block_sum(acc)


def _bn_bwd_apply(x, dz, ch, sg, sgx, mut=None, split=False):
    B, C, S = x.shape
    inv_n = _f32(1.0 / (S if mut == "inv_n_s" else float(B) * S))
    mg, mgx = _chan(sg * inv_n), _chan(sgx * inv_n)
    dx = ch.dx(x, dz, mg, mgx, mut)
    if split:
        t = dx.reshape(B, C, S // 64, 4, 16)
        acc = torch.zeros(B, C, S // 64, 4, dtype=torch.float32)
        for qq in range(16):
            acc = acc + t[..., qq]
        rowpart = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])
        dbias = _block_finalize(rowpart)
        return _split_pair(dx), dbias
    rowpart = _apply_blocks(_tree4(dx.reshape(B, C, S // 4, 4)), K_BWD_U)
    return dx, _wave_finalize(rowpart)


def emulate_bn_backward(inp, mean, invstd, mut=None, split=False, parts=None):
    """bn_act_bwd (bn_bwd_stats_kernel + apply) or, with parts (C, P, 2), the apply
    on given partials (bn_act_bwd_apply_parts)."""
    x, dz = _flat3(inp["x"]), _flat3(inp["dz"])
    B, C, S = x.shape
    ch = BnChan(_chan(mean), _chan(invstd), _chan(inp["gamma"]), _chan(inp["beta"]), inp["slope"])
    if parts is None:
        S4, P = S // 4, bn_parts(B)
        PS = P // B
        g = ch.grad(x, dz)
        gx = g * ch.xhat(x)
        g4, gx4 = g.reshape(B, C, S4, 4), gx.reshape(B, C, S4, 4)
        pg, pgx = [], []
        for p in range(P):
            b = p // PS
            s0, s1 = _part_range(S4, p - b * PS, PS)
            pg.append(_strip(g4[b, :, s0:s1]))
            pgx.append(_strip(gx4[b, :, s0:s1]))
        parts = torch.stack([torch.stack(pg, 1), torch.stack(pgx, 1)], 2)
    sg, sgx = sum_parts2(parts[..., 0], mut), sum_parts2(parts[..., 1], mut)
    dx, dbias = _bn_bwd_apply(x, dz, ch, sg, sgx, mut, split)
    return {"dx": dx, "dgamma": sgx, "dbeta": sg, "dbias_in": dbias}


def emulate_se(inp, mean, invstd, mut=None):
    """bn_se_bwd_stats (five row sums) and bn_se_bwd_apply_split."""
    x, g = _flat3(inp["x"]), _flat3(inp["dz"])
    B, C, S = x.shape
    S4, PS = S // 4, se_stat_parts(B, C, S)
    ch = BnChan(_chan(mean), _chan(invstd), _chan(inp["gamma"]), _chan(inp["beta"]), inp["slope"])
    xh, t = ch.xhat(x), ch.pre(x)
    a = torch.where(t > 0, _f32(1.0), _f32(inp["slope"]))
    z = ch.z(x)
    ag = a * g
    r4 = lambda v: v.reshape(B, C, S4, 4)  # noqa: E731
    acc = [torch.zeros(B, C, dtype=torch.float32) for _ in range(5)]
    for ps in range(PS):
        s0, s1 = _part_range(S4, ps, PS)
        sl = lambda v: r4(v)[:, :, s0:s1]  # noqa: E731
        vals = [_strip_fma(sl(z), sl(g)), _strip(sl(ag)), _strip(sl(a.expand_as(x))),
                _strip_fma(sl(ag), sl(xh)), _strip_fma(sl(a.expand_as(x)), sl(xh))]
        acc = [s + v for s, v in zip(acc, vals)]
    rowstats = torch.stack(acc)
    sv, tv = inp["se_s"], inp["dmv"]
    sg = torch.zeros(C, dtype=torch.float32)
    sgx = torch.zeros(C, dtype=torch.float32)
    for bb in range(B):
        sg = sg + _fma(sv[bb], rowstats[1, bb], tv[bb] * rowstats[2, bb])
        sgx = sgx + _fma(sv[bb], rowstats[3, bb], tv[bb] * rowstats[4, bb])
    dz = _fma(sv[:, :, None].expand_as(x), g, tv[:, :, None].expand_as(x))
    dx, dbias = _bn_bwd_apply(x, dz, ch, sg, sgx, mut, split=True)
    return {"rowstats": rowstats, "dx": dx, "dgamma": sgx, "dbeta": sg, "dbias_in": dbias}


def _silu32(x):
    return x / (1.0 + torch.exp(-x))


def _dsilu32(x):
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def emulate_gn(inp, silu, mut=None, bn=None):
    """gn_stats / gn_finalize / apply and gn_bwd_stats / gn_bwd_finalize / apply.
    bn = (mean, invstd) float32: the IN forms over z = BnChan::z(y); the output then
    also has bnpart (c, b * nbx, 2)."""
    B, C, N, G = inp["shape"]
    cpg, N4 = C // G, N // 4
    x = inp["x"] if bn is None else inp["y"]
    tc = None
    v = x
    if bn is not None:
        tc = BnChan(_chan(bn[0]), _chan(bn[1]), _chan(inp["bn_gamma"]), _chan(inp["bn_beta"]), 0.0)
        v = tc.z(x)
    w, bias = inp["w"], inp["bias"]
    vg = v.reshape(B, G, cpg * N4, 4)
    K = v.reshape(B, G, -1)[:, :, 0]
    tot = cpg * N4
    chunk = _cdiv(tot, K_GN_PARTS)
    s = torch.zeros(B, G, dtype=torch.float32)
    q = torch.zeros(B, G, dtype=torch.float32)
    for p in range(K_GN_PARTS):
        f0 = min(tot, p * chunk)
        f1 = min(tot, f0 + chunk)
        ps, pq = _shifted_parts(vg[:, :, f0:f1], K)
        s, q = s + ps, q + pq
    mean, rstd, _ = stat_of_shifted(s, q, float(cpg) * N, K, inp["eps"], mut)
    per = lambda t: t.repeat_interleave(cpg, 1)[:, :, None]  # noqa: E731
    m, rs = per(mean), per(rstd)
    a = rs * w[None, :, None]
    sh = bias[None, :, None] - m * a
    u = _fma(v, a.expand_as(v), sh.expand_as(v))
    out = {"mean": mean, "rstd": rstd}
    if silu:
        g1 = torch.ones(B, C, 1, dtype=torch.float32)
        out["out"] = _silu32(u)
    else:
        g1 = 1.0 + inp["gamma"][:, :, None]
        out["out"] = v + (u * g1 + inp["beta"][:, :, None])
    # backward
    d = inp["dout"]
    if silu:
        arg = u if mut != "dsilu_arg" else v
        d = d * _dsilu32(arg)
    xh = (v - m) * rs
    d4, dx4 = d.reshape(B, C, N4, 4), (d * xh).reshape(B, C, N4, 4)
    rchunk = _cdiv(N4, K_GN_PARTS)
    a2 = torch.zeros(B, C, dtype=torch.float32)
    a3 = torch.zeros(B, C, dtype=torch.float32)
    for p in range(K_GN_PARTS):
        f0 = min(N4, p * rchunk)
        f1 = min(N4, f0 + rchunk)
        a2 = a2 + _strip(_tree4(d4[:, :, f0:f1])[..., None])
        t = dx4[:, :, f0:f1]
        a3 = a3 + _strip(((t[..., 0] + t[..., 1]) + (t[..., 2] + t[..., 3]))[..., None])
    g12 = g1[:, :, 0]
    if not silu:
        out["dbeta"] = a2
        out["dgamma"] = w[None] * a3 + (0.0 if mut == "dgamma_no_bias" else bias[None] * a2)
    dws = torch.zeros(C, dtype=torch.float32)
    dbs = torch.zeros(C, dtype=torch.float32)
    for b in range(B):
        dws = dws + g12[b] * a3[b]
        dbs = dbs + g12[b] * a2[b]
    out["dw"], out["dbias"] = dws, dbs
    t1 = (w[None] * g12 * a2).reshape(B, G, cpg)
    t2 = (w[None] * g12 * a3).reshape(B, G, cpg)
    k1 = torch.zeros(B, G, dtype=torch.float32)
    k2 = torch.zeros(B, G, dtype=torch.float32)
    for j in range(cpg):
        k1, k2 = k1 + t1[:, :, j], k2 + t2[:, :, j]
    inv_d = _f32(1.0 / (float(cpg) * N))
    inv_d2 = _f32(1.0 / N) if mut == "k2_over_n" else inv_d
    kc0 = rs * g1 * w[None, :, None]
    kc1 = rs * per(k1) * inv_d
    kc2 = rs * per(k2) * inv_d2
    if silu:
        dx = (d * kc0 - kc1) - xh * kc2
    else:
        dx = d + ((d * kc0 - kc1) - xh * kc2)
    out["dz" if bn is not None else "dx"] = dx
    if bn is not None:
        nbx = _cdiv(N4, 256)
        gg = tc.grad(x, dx)
        ggx = gg * tc.xhat(x)
        pad = nbx * 256 - N4
        blk = lambda t: F.pad(t.reshape(B, C, N4, 4), (0, 0, 0, pad)).reshape(B, C, nbx, 256, 4)  # noqa: E731
        sg, sgx = _strip(blk(gg)), _strip(blk(ggx))  # (B, C, nbx)
        slot = torch.stack([sg, sgx], 3)  # (B, C, nbx, 2)
        part = torch.zeros(C, B * nbx, 2, dtype=torch.float32)
        for b in range(B):
            for bx in range(nbx):
                idx = bx * B + b if mut == "bnpart_swap" else b * nbx + bx
                part[:, idx] = slot[b, :, bx]
        out["bnpart"] = part
    return out


def emulate_bnin(inp, mut=None):
    """bn_forward_stats(y) -> gn_film_res_forward_bnin -> gn_film_res_backward_bnin ->
    bn_act_backward_parts, as _PostGNFiLMRes chains them."""
    y = inp["y"]
    st = emulate_bn_stats(y, inp["bn_eps"], inp["rm"], inp["rv"], mut)
    out = emulate_gn(inp, False, mut, bn=(st["mean"], st["invstd"]))
    bi = {"x": y, "dz": out["dz"], "gamma": inp["bn_gamma"], "beta": inp["bn_beta"], "slope": 0.0}
    bw = emulate_bn_backward(bi, st["mean"], st["invstd"], mut, parts=out["bnpart"])
    out.update({"bn": st, "dy": bw["dx"], "bn_dgamma": bw["dgamma"], "bn_dbeta": bw["dbeta"],
                "dbias_in": bw["dbias_in"]})
    return out
