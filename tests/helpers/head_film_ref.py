"""float64 autograd reference, seeded inputs and error bounds for the FiLM head
row kernels (csrc/head_film.hip; formulas in include/pcfm.h, "Trunk rows of
VelocityNetWithContext").  Shared by tests/test_head_film_ref_cpu.py (which runs
a float32 emulation of the kernel's expressions through the same checks) and
tests/test_gpu_head_film.py (which runs the kernels through them).

The reference is a plain forward in float64 differentiated by torch.autograd:
it shares no algebra with the kernel's hand-written backward.

Rounding counts.  e = 2^-24 is one fp32 rounding.  Every k below is the number
of roundings on the longest dependency chain of film_fwd_kernel /
film_bwd_kernel for that output, at W = 512 (NV = 2: 8 channels per lane), a
1-ulp intrinsic (expf, rsqrtf) counted as 2:

  mean  : 7 serial lane adds + 6 shuffle adds (x 1/W is exact)            = 13
  rstd  : mean 13, x - mean 1, 8 serial fma, 6 shuffle adds, + eps 1,
          rsqrtf 2                                                        = 31
  u     : rstd 31, rstd * (x - mean) 1, fma 1, * sp1 1, + shift 1         = 35
  SiLU' : expf 2, 1 + . 1, 1 / . 1, 1 - s 1, x * . 1, 1 + . 1, s * . 1 = 8,
          and the cancellation 1 - s: it is exact, but carries s's absolute
          error (half an ulp of 1 + exp(-x) in [1, 2) = e, half an ulp of the
          quotient in [0.5, 1) = e / 2) multiplied by x.  x (1 - s) is non-zero
          only while exp(-x) >= 2^-24, x <= 24 ln 2 = 16.6, so where SiLU' ~ 1
          it adds up to 1.5 * 16.6 = 25 roundings' worth               8 + 25 = 33
  dh    : u 35, SiLU' 33, da * . 1, du + . 1, * sp1 1, * gamma 1,
          * xc 1, s2: 7 + 6 = 13, xh * m2 1, the second subtraction 1,
          rstd * . 1                                                      = 89
  SiLU-only dh : SiLU' 33, da * . 1                                       = 34
  column-sum term (dy * xc, the longest): u 35, SiLU' 33, da * . 1,
          du + . 1, * sp1 1, * xc 1                                       = 72
  column-sum adds: 64 serial adds of one wave, 3 of the 4-wave combine,
          ceil(18 / 4) = 5 serial chunk adds of one reduce group, 3 of the
          group combine, B = 3 batch adds                                 = 78
  k_s   : 72 + 78 = 150 (dsp1, dshift, dgamma, dbeta); 78 for dbias and
          dbias_b, whose summands (the kernel's own bf16 dh) are exact.

All stay below the 1e-5 / e = 167.8 cap.  A count is a bound only while each
rounding's magnitude, carried to the output, stays below the output's scale;
with the inputs of make_inputs (|gamma * sp1| <~ 3, rstd ~ 2/3, a row's largest
|u| >= 20 from the shift tails) that holds, and the CPU emulation test checks
it on exactly these inputs.
"""
import functools

import torch
import torch.nn.functional as F

E = 2.0 ** -24
K_CAP = 1e-5 / E
K_MEAN = 13
K_RSTD = 31
K_U = 35
K_DH = 89
K_SILU_DH = 34
K_S = 150
K_S_BIAS = 78
FLIP_CAP_A = 5e-3  # share of bf16 a elements that may differ (by one ulp) at all
EPS = 1e-5
ROWS_PER_CHUNK = 256  # film_bwd_kernel's rows per block

# (b, n, w): the smallest sizes at which a distinct code path can fail
SHAPES = [
    (1, 1, 256),     # one row, three idle waves
    (3, 3, 512),     # fewer rows than waves, b > 1
    (2, 33, 256),    # a second forward block of one row (32 rows per block)
    (2, 257, 512),   # a second backward chunk of one row; 3 of 4 reduce groups empty
    (3, 3073, 256),  # chunks = 13: 4-at-a-time loop in group 0 only, tail loop elsewhere
    (2, 4357, 512),  # chunks = 18: pre-loaded loop in all groups, tails in groups 0 and 1
]


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def make_inputs(b, n, w, first):
    """Seeded CPU inputs of one FiLM block.  first: h16 + hbias (the first block);
    else uprev + gprev.  Rows carry a per-row offset (a one-pass variance fails),
    every per-batch vector is drawn per batch element, shift reaches +-20 in 8
    columns each, and no tile repeats."""
    g = torch.Generator().manual_seed(1000003 * b + 1009 * n + w + (7 if first else 0))
    rows = b * n
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    uni = lambda *s: 2.0 * torch.rand(*s, generator=g) - 1.0  # noqa: E731
    hfull = 1.5 * rnd(rows, w) + 4.0 * uni(rows, 1)
    inp = {"b": b, "n": n, "w": w, "first": first,
           "h16": None, "hbias": None, "uprev": None, "gprev": None}
    if first:
        inp["h16"] = hfull.bfloat16()
        inp["hbias"] = 0.5 * rnd(b, w)
    else:
        inp["gprev"] = (0.5 * rnd(rows, w)).bfloat16()
        inp["uprev"] = hfull - inp["gprev"].float()
    inp["gamma"] = 1.0 + 0.3 * uni(w)
    inp["beta"] = 0.3 * uni(w)
    inp["sp1"] = (1.0 + 0.4 * rnd(b, w)).bfloat16()
    shift = 0.4 * rnd(b, w)
    cols = torch.randperm(w, generator=g)[:16]
    shift[:, cols[:8]] = 20.0
    shift[:, cols[8:]] = -20.0
    inp["shift"] = shift.bfloat16()
    nz = lambda t: torch.where(t == 0, torch.ones_like(t), t)  # noqa: E731
    inp["dh_next"] = nz(rnd(rows, w))
    inp["da16"] = nz(rnd(rows, w).bfloat16())
    assert bool((inp["dh_next"] != 0).all()) and bool((inp["da16"] != 0).all())
    return inp


def make_silu_inputs(b, n, w):
    """The output layer's pair: h = uprev + gprev with +-20 tails in 8 columns each."""
    g = torch.Generator().manual_seed(1000003 * b + 1009 * n + w + 13)
    rows = b * n
    gprev = (0.5 * torch.randn(rows, w, generator=g)).bfloat16()
    uprev = 1.5 * torch.randn(rows, w, generator=g) + 4.0 * (2.0 * torch.rand(rows, 1, generator=g) - 1.0)
    cols = torch.randperm(w, generator=g)[:16]
    uprev[:, cols[:8]] += 20.0
    uprev[:, cols[8:]] -= 20.0
    da16 = torch.randn(rows, w, generator=g).bfloat16()
    return {"b": b, "n": n, "w": w, "uprev": uprev, "gprev": gprev, "da16": da16}


def h_of(inp):
    """h as the kernel forms it (fp32 add, bf16 round for the hbias form), in float64."""
    b, n, w = inp["b"], inp["n"], inp["w"]
    if inp.get("h16") is not None:
        if inp.get("hbias") is not None:
            h = (inp["h16"].float().view(b, n, w) + inp["hbias"][:, None, :]).bfloat16()
            return h.double().view(b * n, w)
        return inp["h16"].double()
    return (inp["uprev"] + inp["gprev"].float()).double()


def _per_batch(t, n):
    return t.view(t.shape[0] // n, n, -1).sum(1)


def film_ref(inp):
    """float64 forward + torch.autograd backward of one FiLM block; also the scales
    the errors are measured against."""
    b, n, w = inp["b"], inp["n"], inp["w"]
    h = h_of(inp).requires_grad_(True)
    gamma = inp["gamma"].double().requires_grad_(True)
    beta = inp["beta"].double().requires_grad_(True)
    sp1 = inp["sp1"].double().requires_grad_(True)
    shift = inp["shift"].double().requires_grad_(True)
    dhn, da = inp["dh_next"].double(), inp["da16"].double()
    y = F.layer_norm(h, (w,), gamma, beta, EPS)
    u = (y.view(b, n, w) * sp1[:, None, :] + shift[:, None, :]).view(b * n, w)
    a = F.silu(u)
    loss = (dhn * u).sum() + (da * a).sum()
    dh, dgamma, dbeta, dsp1, dshift, dy = torch.autograd.grad(
        loss, [h, gamma, beta, sp1, shift, y], retain_graph=True)
    ds, = torch.autograd.grad(a.sum(), u)  # SiLU'(u), elementwise
    hd = h.detach()
    mean = hd.mean(1)
    rstd = (hd.var(1, unbiased=False) + EPS).rsqrt()
    # Magnitudes for the scales only (the compared values all come from autograd).
    # A column sum's summand is a product of cancelling sums -- x - mean,
    # gamma xhat + beta, dh_next + da SiLU'(u) -- and each enters with the sum of
    # its terms' magnitudes: where one cancels, its error does not.
    xhat = (hd.abs() + mean.abs()[:, None]) * rstd[:, None]
    yabs = gamma.detach().abs() * xhat + beta.detach().abs()
    dabs = dhn.abs() + (da * ds).abs()
    spb = sp1.detach().abs().repeat_interleave(n, 0)
    ref = {
        "h": hd, "u": u.detach(), "mean": mean, "rstd": rstd,
        "dh": dh, "dgamma": dgamma, "dbeta": dbeta, "dsp1": dsp1, "dshift": dshift,
        "u_scale": u.detach().abs().amax(1),
        "mean_scale": hd.abs().amax(1),
        "rstd_scale": rstd,
        "dh_scale": (dy * gamma.detach()).abs().amax(1) * rstd,
        "dsp1_abs": _per_batch(dabs * yabs, n),
        "dshift_abs": _per_batch(dabs, n),
        "dgamma_abs": (dabs * spb * xhat).sum(0),
        "dbeta_abs": (dabs * spb).sum(0),
    }
    return ref


def silu_ref(inp):
    h = h_of(inp).requires_grad_(True)
    a = F.silu(h)
    dh, = torch.autograd.grad((inp["da16"].double() * a).sum(), h)
    return {"h": h.detach(), "a": a.detach(), "dh": dh, "dh_scale": dh.abs().amax(1)}


def bias_ref(dh16, n):
    """dbias / dbias_b are sums of the bf16-rounded dh: the reference is the float64
    column sum of the kernel's own dh16 (isolates the reduction from the rounding)."""
    d = dh16.double()
    return {"dbias": d.sum(0), "dbias_abs": d.abs().sum(0),
            "dbias_b": _per_batch(d, n), "dbias_b_abs": _per_batch(d.abs(), n)}


@functools.lru_cache(maxsize=2)
def cached_case(shape, first):
    """(inputs, reference) of one case, computed once and shared; treat as read-only."""
    inp = make_inputs(*shape, first)
    return inp, film_ref(inp)


# ---------------------------------------------------------------------------
# checks (each returns the largest error / bound; <= 1 passes; NaN fails)
# ---------------------------------------------------------------------------
def row_ratio(got, ref, scale_row, k):
    """Per row: max |got - ref| over the row against k e scale_row."""
    assert k <= K_CAP
    rows = ref.shape[0]
    err = (got.double() - ref).abs().reshape(rows, -1).amax(1)
    assert got.shape == ref.shape and bool((scale_row > 0).all())
    return float((err / (k * E * scale_row)).max())


def colsum_ratio(got, ref, abs_sum, k):
    """Per column: |got - ref| against k e abs_sum."""
    assert k <= K_CAP
    assert got.shape == ref.shape and bool((abs_sum > 0).all())
    return float(((got.double() - ref).abs() / (k * E * abs_sum)).max())


def _bf16_key(t):
    bits = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits < 0, -(bits & 0x7FFF), bits)


def bf16_flips(got, want):
    """(largest distance in bf16 ulps, share of elements that differ at all)."""
    assert got.dtype == want.dtype == torch.bfloat16 and got.shape == want.shape
    assert bool(torch.isfinite(got.float()).all())
    d = (_bf16_key(got) - _bf16_key(want)).abs()
    return int(d.max()), float((d != 0).double().mean())


# ---------------------------------------------------------------------------
# float32 emulation of the kernel's expressions (CPU); the column sums follow
# the kernel's order: 64 serial rows per wave, 4-wave combine, every 4th chunk
# per reduce group, group combine, serial batch sum.
# ---------------------------------------------------------------------------
def _kernel_colsum(x, b, n):
    """x f32 (b*n, w) -> per-batch (b, w) sums in film_bwd / film_bwd_reduce order."""
    w = x.shape[1]
    chunks = -(-n // ROWS_PER_CHUNK)
    pad = torch.zeros(b, chunks * ROWS_PER_CHUNK, w, dtype=torch.float32)
    pad[:, :n] = x.view(b, n, w)
    pad = pad.view(b, chunks, 64, 4, w)  # row i0 + 4 it + wave
    acc = torch.zeros(b, chunks, 4, w, dtype=torch.float32)
    for it in range(64):
        acc = acc + pad[:, :, it]
    part = ((acc[:, :, 0] + acc[:, :, 1]) + acc[:, :, 2]) + acc[:, :, 3]
    grp = []
    for g in range(4):
        s = torch.zeros(b, w, dtype=torch.float32)
        for q in range(g, chunks, 4):
            s = s + part[:, q]
        grp.append(s)
    return ((grp[0] + grp[1]) + grp[2]) + grp[3]


def _batch_sum(perb):
    s = torch.zeros_like(perb[0])
    for i in range(perb.shape[0]):
        s = s + perb[i]
    return s


def _silu32(x):
    return x / (1.0 + torch.exp(-x))


def _dsilu32(x):
    s = 1.0 / (1.0 + torch.exp(-x))
    return s * (1.0 + x * (1.0 - s))


def emulate_film_fp32(inp):
    """The kernel's expressions in float32 torch: two-pass mean / variance,
    fma(gamma, rstd (x - mean), beta) * sp1 + shift, x / (1 + exp(-x)),
    s (1 + x (1 - s)), the LayerNorm / FiLM backward and the ordered sums."""
    b, n, w = inp["b"], inp["n"], inp["w"]
    x = h_of(inp).float()  # exact: h is a bf16 value or an fp32 sum
    gm, bt = inp["gamma"], inp["beta"]
    sp = inp["sp1"].float().repeat_interleave(n, 0)
    sh = inp["shift"].float().repeat_interleave(n, 0)
    mean = x.sum(1) * (1.0 / w)
    dev = x - mean[:, None]
    rstd = ((dev * dev).sum(1) * (1.0 / w) + EPS).rsqrt()
    xc = rstd[:, None] * dev
    y = torch.addcmul(bt, gm, xc)
    u = y * sp + sh
    a = _silu32(u).bfloat16()
    d = inp["dh_next"] + inp["da16"].float() * _dsilu32(u)
    dy = d * sp
    dxh = dy * gm
    m1 = dxh.sum(1, keepdim=True) * (1.0 / w)
    m2 = (dxh * xc).sum(1, keepdim=True) * (1.0 / w)
    dh = rstd[:, None] * (dxh - m1 - xc * m2)
    dh16 = dh.bfloat16()
    perb = [_kernel_colsum(t, b, n) for t in (dy * xc, dy, dh16.float())]
    return {"u": u, "a": a, "mean": mean, "rstd": rstd, "dh": dh, "dh16": dh16,
            "dsp1": _kernel_colsum(d * y, b, n), "dshift": _kernel_colsum(d, b, n),
            "dgamma": _batch_sum(perb[0]), "dbeta": _batch_sum(perb[1]),
            "dbias": _batch_sum(perb[2]), "dbias_b": perb[2]}


def emulate_silu_fp32(inp):
    b, n = inp["b"], inp["n"]
    x = h_of(inp).float()
    dh = inp["da16"].float() * _dsilu32(x)
    dh16 = dh.bfloat16()
    return {"a": _silu32(x).bfloat16(), "dh": dh, "dh16": dh16,
            "dbias": _batch_sum(_kernel_colsum(dh16.float(), b, n))}


# ---------------------------------------------------------------------------
# the assertions of both suites: out is a dict of CPU tensors (kernel outputs or
# the emulation's); rec(name, ratio) records error / bound; flip_margin divides
# the flip caps (the CPU emulation must keep a factor to spare)
# ---------------------------------------------------------------------------
def check_film_forward(out, ref, rec, flip_margin=1.0):
    bad = []

    def note(name, ratio, cap=1.0):
        rec(name, ratio)
        if not ratio <= cap:
            bad.append((name, ratio, cap))
    note("u", row_ratio(out["u"], ref["u"], ref["u_scale"], K_U))
    note("mean", row_ratio(out["mean"], ref["mean"], ref["mean_scale"], K_MEAN))
    note("rstd", row_ratio(out["rstd"], ref["rstd"], ref["rstd_scale"], K_RSTD))
    # a: the bf16 rounding of the float64 SiLU of the kernel's own fp32 u
    ulps, share = bf16_flips(out["a"], F.silu(out["u"].double()).bfloat16())
    note("a_ulps", ulps)
    note("a_flip_share", share, FLIP_CAP_A / flip_margin)
    assert not bad, bad


def check_film_backward(out, ref, n, rec):
    bad = []

    def note(name, ratio, cap=1.0):
        rec(name, ratio)
        if not ratio <= cap:
            bad.append((name, ratio, cap))
    note("dh", row_ratio(out["dh"], ref["dh"], ref["dh_scale"], K_DH))
    # dh16 is a pure rounding of the fp32 dh written next to it: no flips at all
    ulps, share = bf16_flips(out["dh16"], out["dh"].bfloat16())
    note("dh16_ulps", ulps, 0)
    note("dh16_flip_share", share, 0.0)
    for k in ("dsp1", "dshift", "dgamma", "dbeta"):
        note(k, colsum_ratio(out[k], ref[k], ref[k + "_abs"], K_S))
    br = bias_ref(out["dh16"], n)
    note("dbias", colsum_ratio(out["dbias"], br["dbias"], br["dbias_abs"], K_S_BIAS))
    if out.get("dbias_b") is not None:
        note("dbias_b", colsum_ratio(out["dbias_b"], br["dbias_b"], br["dbias_b_abs"], K_S_BIAS))
    assert not bad, bad


def check_silu_pair(out, ref, n, rec, flip_margin=1.0):
    bad = []

    def note(name, ratio, cap=1.0):
        rec(name, ratio)
        if not ratio <= cap:
            bad.append((name, ratio, cap))
    ulps, share = bf16_flips(out["a"], ref["a"].bfloat16())
    note("silu_a_ulps", ulps)
    note("silu_a_flip_share", share, FLIP_CAP_A / flip_margin)
    note("silu_dh", row_ratio(out["dh"], ref["dh"], ref["dh_scale"], K_SILU_DH))
    ulps, share = bf16_flips(out["dh16"], out["dh"].bfloat16())
    note("silu_dh16_ulps", ulps, 0)
    note("silu_dh16_flip_share", share, 0.0)
    br = bias_ref(out["dh16"], n)
    note("silu_dbias", colsum_ratio(out["dbias"], br["dbias"], br["dbias_abs"], K_S_BIAS))
    assert not bad, bad
