"""The non-finite contract of the gradient-path kernels (DESIGN.md "Parity"): the
case table shared by tests/test_nonfinite_cpu.py and tests/test_gpu_nonfinite.py,
plain float64 torch references, and the three assertions.

A case is an Entry: one kernel entry point at one shape (and slope).  Its inputs are
finite O(1) float32 tensors with 1.0 at every injection site, so ONE `clean` call
serves every site; an injection replaces one site (the opposing case: two) by a
special value.  For each injection

1. mask:  ~isfinite(kernel output) == ~isfinite(reference), elementwise, every output.
   Masks, not kinds: a bf16x3 operand split turns inf into (hi = inf, lo = NaN).
2. leak:  where the reference is finite and EQUAL on the special and the clean
   inputs the kernel's special output has the bits of its clean output.
   Where the reference is finite on the special inputs but differs from its value on
   the clean ones the output does depend on the injected element (relu(-inf) = 0,
   the sum of dz behind a NaN ReLU unit, max(inf, NaN)): bit equality with `clean`
   cannot hold for any implementation, and the output is held to the reference at
   DEP_TOL, the suite's fp64 bar.
3. non-trivial: the affected set -- non-finite in the reference, or finite and moved
   (relu(-inf) = 0 leaves nothing non-finite) -- is neither empty nor every output
   (no case of the table is exempt: the only all-dependent operation named by the
   issue, the clip norm, is pinned by the fused-update tests, outside the table).

Only float feature / gradient / weight / affine operands are injected; indices,
coordinates, counts and plans are never touched.
"""
import contextlib
import math

import torch
import torch.nn.functional as F

DEP_TOL = 1e-4  # max |err| / max(1, max |ref|) on the dependent finite outputs
MOM, NBT0, EPS = 0.1, 3, 1e-5

_BITS = {"+inf": 0x7F800000, "-inf": 0xFF800000 - (1 << 32), "nan": 0x7FC00000,
         "nan7fffffff": 0x7FFFFFFF}
KINDS = tuple(_BITS)


def special(kind):
    """the float32 special value, as a 0-dim tensor (bit pattern kept)"""
    return torch.tensor(_BITS[kind], dtype=torch.int32).view(torch.float32)


def bits(t):
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16)
    return t


@contextlib.contextmanager
def poked(inp, operand, sites_kinds):
    """inp[operand][site] = special(kind) for the block, restored after it (in place:
    the large GEMM operands are not copied per injection)"""
    t = inp[operand]
    old = [t[s].clone() for s, _ in sites_kinds]
    for s, k in sites_kinds:
        if t.dtype == torch.bfloat16:  # the bf16 of the same kind: the high 16 bits
            t.view(torch.int16)[s] = _BITS[k] >> 16
        else:
            t.view(torch.int32)[s] = _BITS[k]
    try:
        yield inp
    finally:
        for (s, _), o in zip(sites_kinds, old):
            t[s] = o


class Entry:
    """name: the pcfm.ops function (+ variant); shape; params (slope ...);
    make(): the clean inputs; sites: operand -> [index tuples]; opposing: (operand,
    site of +inf, site of -inf) in one reduction; ref(inp) -> {output: float64 / int
    tensor}; masks(...) optional: the classification without full references"""

    def __init__(self, family, name, shape, make, sites, ref, opposing=None, params=None,
                 masks=None, cpu_ref=None):
        self.family, self.name, self.shape = family, name, tuple(shape)
        self.make, self.sites, self.ref = make, sites, ref
        self.opposing, self.params = opposing, dict(params or {})
        # fast_masks: the classification without full references (large GEMMs);
        # cpu_ref: the reference of the CPU path where it deliberately differs
        self.fast_masks, self.cpu_ref = masks, cpu_ref
        self._inp = None

    @property
    def id(self):
        p = "".join(f"-{k}{v}" for k, v in sorted(self.params.items()))
        return f"{self.name}-{'x'.join(str(s) for s in self.shape)}{p}"

    def inputs(self):
        """the clean inputs (cached; injections poke and restore them)"""
        if self._inp is None:
            inp = self.make()
            for op, sites in self.sites.items():
                for s in sites:
                    inp[op][s] = 1.0
            if self.opposing is not None:
                op, a, b = self.opposing
                inp[op][a] = 1.0
                inp[op][b] = 1.0
            self._inp = inp
        return self._inp

    def injections(self):
        """(label, operand, [(site, kind), ...])"""
        for op, sites in self.sites.items():
            for s in sites:
                for k in KINDS:
                    yield f"{op}{list(s)}={k}", op, [(s, k)]
        if self.opposing is not None:
            op, a, b = self.opposing
            yield f"{op}{list(a)}=+inf,{list(b)}=-inf", op, [(a, "+inf"), (b, "-inf")]

    def classify(self, inp, operand, sites_kinds, clean_ref, ref=None):
        """{output: (nonfinite mask, dependent mask, reference values float64)} of the
        injection; clean_ref = ref(clean inputs) (None where masks() needs none)"""
        if self.fast_masks is not None:
            return self.fast_masks(self, inp, operand, sites_kinds)
        with poked(inp, operand, sites_kinds):
            rs = (ref or self.ref)(inp)  # ref: cpu_ref, with clean_ref from it too
        out = {}
        post =rs.pop("_post", None)
        clean_ref = {k: v for k, v in clean_ref.items() if k != "_post"}
        for k, v in rs.items():
            c = clean_ref[k]
            if not v.dtype.is_floating_point:
                out[k] = (torch.zeros_like(v, dtype=torch.bool), v != c, v)
                continue
            fin = torch.isfinite(v)
            out[k] = (~fin, fin & (v != c), v)
        if post is not None:
            post(out)
        return out


def nontrivial(cls):
    """assertion 3 on a classification: the affected set (non-finite in the reference,
    or finite and moved: relu(-inf) = 0 leaves nothing non-finite) is neither empty
    nor everything"""
    aff = sum(int((m[0] | m[1]).sum()) for m in cls.values())
    tot = sum(m[0].numel() for m in cls.values())
    return 0 < aff < tot


def check(label, out_s, out_c, cls):
    """assertions 1 and 2 of one injection.  out_s / out_c: {output or output.hi /
    output.lo (the planes of a bf16 split): tensor} of the special and the clean call
    (any device); cls: Entry.classify's result."""
    for k, got in out_s.items():
        nf, dep, val, *scale = cls[k.split(".")[0]]
        clean = out_c[k]
        dev = got.device
        nf, dep = nf.to(dev), dep.to(dev)
        assert got.shape == nf.shape, (label, k, got.shape, nf.shape)
        if got.dtype.is_floating_point:
            gnf = ~torch.isfinite(got)
            if not torch.equal(gnf, nf):
                sw, inv = int((nf & ~gnf).sum()), int((gnf & ~nf).sum())
                raise AssertionError(f"{label}: {k}: non-finite mask differs from the reference: "
                                     f"{sw} swallowed, {inv} invented (of {int(nf.sum())} "
                                     f"non-finite in the reference, {nf.numel()} elements)")
        same = ~nf & ~dep
        leak = (bits(got) != bits(clean)) & same
        if bool(leak.any()):
            raise AssertionError(f"{label}: {k}: {int(leak.sum())} outputs that do not depend on "
                                 f"the injected element differ from the clean call's bits")
        if bool(dep.any()) and not k.endswith(".lo"):
            v = val.to(dev)[dep]
            if not got.dtype.is_floating_point:
                assert torch.equal(got[dep].long(), v.long()), (label, k)
                continue
            err = (got[dep].double() - v).abs().max().item()
            # (scale: the sum of magnitudes behind an output that is a cancelling sum)
            bar = DEP_TOL * max(1.0, v.abs().max().item(), *scale)
            if k.endswith(".hi"):  # the hi plane alone: + bf16's 2^-9 relative
                bar += 2.0 ** -8 * v.abs().max().item()
            assert err <= bar, f"{label}: {k}: dependent finite outputs off by {err} > {bar}"


def _gen(*key):
    """a CPU generator seeded from the key's text (the same data in every process)"""
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate("/".join(map(str, key))))
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _randn(g, *s):
    return torch.randn(*s, generator=g, dtype=torch.float32)


def _edge_points(n):
    """first, last and each side of every 32 / 64 / 128 tile edge below n"""
    return sorted({0, n - 1} | {p for p in (31, 32, 63, 64, 127, 128) if p < n})


def split_planes(buf, b, c, s):
    """a conv split operand (channels-last rows, [hi 32 | lo 32] bf16 per 32-channel
    group) -> its (b, c, s) bf16 hi and lo planes"""
    t = buf.view(torch.bfloat16).view(b * s, c // 32, 2, 32)
    pl = [t[:, :, i].reshape(b, s, c).permute(0, 2, 1).contiguous() for i in (0, 1)]
    return pl[0], pl[1]


# ---------------------------------------------------------------------------
# BatchNorm (batch statistics) + ReLU / LeakyReLU
# ---------------------------------------------------------------------------
def _act(y, slope):
    return F.relu(y) if slope == 0 else F.leaky_relu(y, slope)


def _bn_opposing(shape):
    """two neighbours of channel 1, batch element 0: one channel's reduction"""
    z = (0,) * (len(shape) - 3)
    return (0, 1) + z + (0,), (0, 1) + z + (1,)


def _bn_make(shape, slope, se=False):
    def make():
        inp = make_()
        for s in _bn_opposing(shape):  # live units: an opposing dz pair reaches the sums
            inp["x"][s] = 3.0
        return inp

    def make_():
        g = _gen("bn", shape, slope)
        b, c = shape[:2]
        inp = {"x": _randn(g, *shape) + 0.5, "dz": _randn(g, *shape),
               "gamma": 1.0 + 0.25 * _randn(g, c), "beta": 0.25 * _randn(g, c),
               "rm": 0.1 * _randn(g, c), "rv": 1.0 + 0.1 * torch.rand(c, generator=g)}
        if se:
            inp["se_s"] = torch.rand(b, c, generator=g) + 0.25
            inp["dmv"] = 0.01 * _randn(g, b, c)
        return inp
    return make


def _bn_sites(shape, operands):
    b, c = shape[:2]
    sp = shape[2:]
    s = math.prod(sp)
    pts = _edge_points(s)
    cm = c // 2

    def at(bi, ci, p):
        idx = []
        for d in reversed(sp):
            idx.append(p % d)
            p //= d
        return (bi, ci) + tuple(reversed(idx))
    elem = [at(0, 0, 0), at(b - 1, c - 1, s - 1)] + [at(b - 1, cm, p) for p in pts[1:-1]]
    if s > 4096:  # both sides of the first apply block's end
        elem += [at(0, cm, 4095), at(0, cm, 4096)]
    chan = [(0,), (c - 1,)]
    full = {"x": elem, "dz": elem, "gamma": chan, "beta": chan}
    return {k: full[k] for k in operands}


def _bn_pre(x, gamma, beta):
    """training-mode BatchNorm as its definition reads, ((x - mean) * invstd) * gamma
    + beta, statistics in the graph.  F.batch_norm's CPU kernel agrees on every
    injection but gamma = +-inf: it folds the affine into x * (gamma * invstd) +
    (beta - mean * gamma * invstd), which is inf - inf = NaN where the definition
    (and BnChan::pre) gives -inf, a finite 0 behind the ReLU (DESIGN.md "Parity")."""
    dims = [0] + list(range(2, x.dim()))
    ex = (None, slice(None)) + (None,) * (x.dim() - 2)
    mean, var = x.mean(dims), x.var(dims, unbiased=False)
    invstd = (var + EPS).rsqrt()
    return ((x - mean[ex]) * invstd[ex]) * gamma[ex] + beta[ex], mean, var, invstd


def bn_forward_ref(inp, slope, torch_affine=False):
    """BatchNorm (batch statistics) + the activation in float64; the saved statistics
    as the kernels define them (biased variance), the running ones as
    F.batch_norm(training=True) updates them (unbiased).  torch_affine: y from
    F.batch_norm itself -- the CPU module path's expectation (NaN for gamma = +-inf
    where the definition gives -inf)."""
    x = inp["x"].double()
    pre, mean, var, invstd = _bn_pre(x, inp["gamma"].double(), inp["beta"].double())
    if torch_affine:
        pre = F.batch_norm(x, None, None, inp["gamma"].double(), inp["beta"].double(), True,
                           MOM, EPS)
    n = x.numel() // x.shape[1]
    return {"y": _act(pre, slope), "mean": mean, "invstd": invstd,
            "running_mean": (1 - MOM) * inp["rm"].double() + MOM * mean,
            "running_var": (1 - MOM) * inp["rv"].double() + MOM * (var * n / (n - 1))}


def bn_backward_ref(inp, slope, se=False, torch_affine=False):
    """autograd through the same composition; se: the gradient arriving is
    dz = se_s[b, c] * g + dmv[b, c] (PVConv's SE scale and pooling gradient)"""
    x = inp["x"].double().requires_grad_(True)
    gamma = inp["gamma"].double().requires_grad_(True)
    beta = inp["beta"].double().requires_grad_(True)
    if torch_affine:
        y = _act(F.batch_norm(x, None, None, gamma, beta, True, MOM, EPS), slope)
    else:
        y = _act(_bn_pre(x, gamma, beta)[0], slope)
    dz = inp["dz"].double()
    if se:
        ex = (Ellipsis,) + (None,) * (x.dim() - 2)
        dz = inp["se_s"].double()[ex] * dz + inp["dmv"].double()[ex]
    dx, dg, db = torch.autograd.grad(y, [x, gamma, beta], dz)
    dims = [0] + list(range(2, x.dim()))

    def post(cls):
        """dbias_in = sum of dx over the channel is analytically 0 (rounding noise on
        both sides): whether it depends on the injection is read off dx, not off the
        noise comparing equal, and its error scale is the channel's sum of |dx|"""
        nf, _, val = cls["dbias_in"]
        moved = (cls["dx"][0] | cls["dx"][1]).transpose(0, 1).flatten(1).any(1)
        mag = torch.where(torch.isfinite(dx), dx.abs(), torch.zeros_like(dx)).sum(dims)
        cls["dbias_in"] = (nf, ~nf & moved, val, float(mag.max()))
    return {"dx": dx, "dgamma": dg, "dbeta": db, "dbias_in": dx.sum(dims), "_post": post}


def _bn_entries():
    out = []
    contig, split = [(3, 5, 36), (2, 6, 4100)], [(2, 64, 4, 4, 4)]
    for slope in (0.0, 0.1):
        p = {"slope": slope}
        for name, shapes in (("bn_act_forward", contig), ("bn_act_forward_split", split),
                             ("bn_act_forward_rowmean", contig[:1] + split)):
            for sh in shapes:
                def ref(inp, slope=slope, name=name):
                    r = bn_forward_ref(inp, slope)
                    if name.endswith("rowmean"):
                        r["rowmean"] = r.pop("y").flatten(2).mean(2)
                    return r
                out.append(Entry("norm", name, sh, _bn_make(sh, slope),
                                 _bn_sites(sh, ("x", "gamma", "beta")), ref,
                                 opposing=("x", (0, 1) + (0,) * (len(sh) - 2),
                                           (0, 1) + (0,) * (len(sh) - 3) + (1,)), params=p,
                                 cpu_ref=lambda inp, slope=slope: bn_forward_ref(inp, slope, True)))
        for name, shapes in (("bn_act_backward", contig), ("bn_act_backward_split", split),
                             ("bn_se_backward_apply_split", split)):
            for sh in shapes:
                se = name.startswith("bn_se")
                out.append(Entry("norm", name, sh, _bn_make(sh, slope, se),
                                 _bn_sites(sh, ("x", "dz", "gamma", "beta")),
                                 lambda inp, slope=slope, se=se: bn_backward_ref(inp, slope, se),
                                 opposing=("dz", (0, 1) + (0,) * (len(sh) - 2),
                                           (0, 1) + (0,) * (len(sh) - 3) + (1,)), params=p,
                                 cpu_ref=lambda inp, slope=slope, se=se: bn_backward_ref(
                                     inp, slope, se, True)))
    for sh in contig:  # the statistics alone (no activation: one slope)
        def ref(inp):
            r = bn_forward_ref(inp, 0.0)
            del r["y"]
            return r
        out.append(Entry("norm", "bn_forward_stats", sh, _bn_make(sh, 0.0), _bn_sites(sh, ("x",)),
                         ref, opposing=("x", (0, 1, 0), (0, 1, 1))))
    return out


# ---------------------------------------------------------------------------
# GroupNorm + SiLU, GroupNorm + FiLM + residual
# ---------------------------------------------------------------------------
def _gn_make(shape):
    def make():
        b, c, n, _ = shape
        g = _gen("gn", shape)
        return {"x": _randn(g, b, c, n) + 0.5, "dout": _randn(g, b, c, n),
                "w": 1.0 + 0.25 * _randn(g, c), "bias": 0.25 * _randn(g, c),
                "gamma": 0.25 * _randn(g, b, c), "beta": 0.25 * _randn(g, b, c)}
    return make


def gn_ref(inp, groups, film, backward):
    t = {k: inp[k].double().requires_grad_(True) for k in ("x", "w", "bias", "gamma", "beta")}
    x = t["x"]
    y = F.group_norm(x, groups, t["w"], t["bias"], EPS)
    out = x + (y * (1.0 + t["gamma"][:, :, None]) + t["beta"][:, :, None]) if film else F.silu(y)
    if not backward:
        b = x.shape[0]
        xg = x.detach().reshape(b, groups, -1)
        return {"out": out.detach(), "mean": xg.mean(2),
                "rstd": (xg.var(2, unbiased=False) + EPS).rsqrt()}
    names = ["x", "w", "bias"] + (["gamma", "beta"] if film else [])
    gr = torch.autograd.grad(out, [t[k] for k in names], inp["dout"].double())
    return dict(zip(["dx", "dw", "dbias", "dgamma", "dbeta"], gr))


def _gn_entries():
    out = []
    sh = (3, 6, 36, 3)
    b, c, n, groups = sh
    elem = [(0, 0, 0), (b - 1, c - 1, n - 1), (1, 2, 31), (1, 3, 32)]
    chan, row = [(0,), (c - 1,)], [(0, 0), (b - 1, c - 1)]
    for film in (True, False):
        fam = "gn_film_res" if film else "gn_silu"
        for backward in (False, True):
            sites = {"x": elem, "w": chan, "bias": chan}
            if film:
                sites.update({"gamma": row, "beta": row})
            if backward:
                sites["dout"] = elem
            if backward and film:
                del sites["beta"]  # beta does not enter the FiLM residual's backward
            out.append(Entry("norm", fam + ("_backward" if backward else "_forward"), sh,
                             _gn_make(sh), sites,
                             lambda inp, film=film, backward=backward: gn_ref(inp, groups, film,
                                                                             backward),
                             opposing=("x", (0, 2, 0), (0, 3, 1))))
    return out


# ---------------------------------------------------------------------------
# SE3d's channel MLP: s = sigmoid(W2 relu(W1 m))
# ---------------------------------------------------------------------------
def _se_make(shape):
    def make():
        b, c, red = shape
        g = _gen("se", shape)
        h = c // red
        return {"m": _randn(g, b, c), "w1": _randn(g, h, c) / c ** 0.5,
                "w2": _randn(g, c, h) / h ** 0.5, "ds": _randn(g, b, c)}
    return make


def se_ref(inp, backward):
    t = {k: inp[k].double().requires_grad_(True) for k in ("m", "w1", "w2")}
    hid = F.relu(t["m"] @ t["w1"].t())
    s = torch.sigmoid(hid @ t["w2"].t())
    if not backward:
        return {"s": s.detach(), "hid": hid.detach()}
    gr = torch.autograd.grad(s, [t["m"], t["w1"], t["w2"]], inp["ds"].double())
    return dict(zip(["dm", "dw1", "dw2"], gr))


def _se_entries():
    sh = (3, 64, 8)
    b, c, red = sh
    h = c // red
    sites = {"m": [(0, 0), (b - 1, c - 1), (1, 15), (1, 16)], "w1": [(0, 0), (h - 1, c - 1)],
             "w2": [(0, 0), (c - 1, h - 1)]}
    out = [Entry("scatter", "se_mlp_forward", sh, _se_make(sh), sites,
                 lambda inp: se_ref(inp, False), opposing=("m", (1, 0), (1, 1)))]
    bs = dict(sites)
    bs["ds"] = [(0, 0), (b - 1, c - 1)]
    out.append(Entry("scatter", "se_mlp_backward", sh, _se_make(sh), bs,
                     lambda inp: se_ref(inp, True), opposing=("ds", (1, 0), (1, 1))))
    return out


# ---------------------------------------------------------------------------
# Pointwise (1x1) convolution: y = W x + bias, its BatchNorm group statistics,
# backward-data, backward-weight, the weight image
# ---------------------------------------------------------------------------
# (b, cin, cout, n) -> (forward form, statistics group or 0)
PW_SHAPES = {
    (1, 96, 32, 45): ("Stream128", 32), (2, 128, 128, 64): ("Stream128", 32),
    (1, 32, 32, 45): ("Stream128", 32), (1, 64, 128, 70): ("Stream128", 32),
    (1, 160, 64, 33): ("Stream128", 32), (1, 192, 96, 40): ("Stream128", 32),
    (1, 224, 128, 65): ("Stream128", 32),
    (1, 5, 3, 7): ("Tile64", 0), (1, 512, 256, 77): ("Tile64", 0),
    (4, 262, 128, 16385): ("Tile128", 0),
    (8, 64, 256, 8200): ("Tile256", 64),
    (2, 256, 256, 100): ("Tile64", 0),  # the wide weight gradient
}
PW_NCH_SHAPES = [(1, 32, 32, 45), (1, 64, 128, 70), (1, 160, 64, 33), (1, 192, 96, 40),
                 (1, 224, 128, 65)]  # Stream128 at NCH = 1, 2, 5, 6, 7


def pw_make(shape):
    def make():
        b, cin, cout, n = shape
        g = _gen("pw", shape)
        return {"x": _randn(g, b, cin, n), "w": _randn(g, cout, cin, 1) / cin ** 0.5,
                "bias": _randn(g, cout), "gy": _randn(g, b, cout, n)}
    return make


def _pw_elem_sites(b, c, n):
    pts = _edge_points(n)
    s = [(0, 0, 0), (b - 1, c - 1, n - 1)] + [(b - 1, c // 2, p) for p in pts[1:-1]]
    if n > 8192:  # the last point of a ragged 128-point tile past many full ones
        s.append((b - 1, c - 1, n - 2))
    return s


def pw_forward_ref(inp):
    w = inp["w"].double()[:, :, 0]
    return {"y": torch.einsum("oc,bcn->bon", w, inp["x"].double())
            + inp["bias"].double()[None, :, None]}


def pw_group_stats(y, group):
    """(cout, b * ceil(n / group), 2): each group's mean and centred sum of squares"""
    b, cout, n = y.shape
    ng = -(-n // group)
    yd = F.pad(y, (0, ng * group - n)).view(b, cout, ng, group)
    dev = y.device
    cnt = torch.full((ng,), float(group), dtype=torch.float64, device=dev)
    cnt[-1] = n - (ng - 1) * group
    valid = (torch.arange(group, device=dev)[None, :]
             + group * torch.arange(ng, device=dev)[:, None]) < n
    mean = torch.where(valid, yd, torch.zeros((), dtype=y.dtype)).sum(-1) / cnt
    m2 = torch.where(valid, (yd - mean[..., None]) ** 2, torch.zeros((), dtype=y.dtype)).sum(-1)
    return torch.stack([mean, m2], -1).permute(1, 0, 2, 3).reshape(cout, b * ng, 2)


def pw_full_ref(name, inp, group=0):
    w = inp["w"].double()[:, :, 0]
    if name.startswith("pointwise_forward"):
        r = pw_forward_ref(inp)
        if name.endswith("bnstats"):
            r["stats"] = pw_group_stats(r["y"], group)
        return r
    if name.startswith("pointwise_backward_data"):
        return {"dx": torch.einsum("oc,bon->bcn", w, inp["gy"].double())}
    return {"dw": torch.einsum("bon,bcn->oc", inp["gy"].double(), inp["x"].double())}


def _mask_triple(shape):
    return (torch.zeros(shape, dtype=torch.bool), torch.zeros(shape, dtype=torch.bool),
            torch.zeros(shape, dtype=torch.float64))


def _fill(tri, index, vs, vc):
    """classify the slice `index` of an output from its special / clean reference"""
    nf, dep, val = tri
    fin = torch.isfinite(vs)
    nf[index] = ~fin
    dep[index] = fin & (vs != vc)
    val[index] = torch.where(fin, vs, torch.zeros((), dtype=torch.float64))


def pw_masks(entry, inp, operand, sites_kinds):
    """Entry.classify for the GEMM entries without a full float64 GEMM per injection:
    an injected element enters one column / row of the output, which is evaluated on
    the special and the clean inputs; every other output has the clean reference by
    construction.  tests/test_nonfinite_cpu.py holds this against the full
    reference at the small shapes."""
    name, (b, cin, cout, n) = entry.name, entry.shape
    group = entry.params.get("group", 0)
    x, gy, bias = inp["x"], inp["gy"], inp["bias"]
    w = inp["w"][:, :, 0]
    sites = [s for s, _ in sites_kinds]
    cache = entry.__dict__.setdefault("_cache", {})

    def f64(k):  # the float64 copy of an operand this injection leaves alone
        assert k != operand
        if k not in cache:
            cache[k] = inp[k].double()
        return cache[k]

    def both(key, fn):  # fn on the special and the clean inputs (clean: once per site)
        key = (operand, key)
        if key not in cache:
            cache[key] = fn()
        with poked(inp, operand, sites_kinds):
            return fn(), cache[key]

    out = {}
    if name.startswith("pointwise_forward"):
        y = _mask_triple((b, cout, n))
        st = _mask_triple((cout, b * -(-n // group), 2)) if group else None
        ng = -(-n // group) if group else 0
        if operand == "x":
            for bi, _, p in sites:
                vs, vc = both((bi, p), lambda: w.double() @ x[bi, :, p].double() + bias.double())
                _fill(y, (bi, slice(None), p), vs, vc)
                if group:
                    g0 = p // group * group
                    sl = slice(g0, min(n, g0 + group))

                    def gs():
                        yy = w.double() @ x[bi, :, sl].double() + bias.double()[:, None]
                        return pw_group_stats(yy[None], group)[:, 0]
                    vs, vc = both((bi, p, "g"), gs)
                    _fill(st, (slice(None), bi * ng + p // group), vs, vc)
        else:
            for s in sites:
                o = s[0]
                vs, vc = both(o, lambda: torch.einsum("c,bcn->bn", w[o].double(), f64("x"))
                              + bias[o].double())
                _fill(y, (slice(None), o), vs, vc)
                if group:
                    vs, vc = both((o, "g"), lambda: pw_group_stats(
                        (torch.einsum("c,bcn->bn", w[o].double(), f64("x"))
                         + bias[o].double())[:, None], group)[0])
                    _fill(st, (o,), vs, vc)
        out["y"] = y
        if group:
            out["stats"] = st
    elif name.startswith("pointwise_backward_data"):
        dx = _mask_triple((b, cin, n))
        if operand == "gy":
            for bi, _, p in sites:
                vs, vc = both((bi, p), lambda: w.double().t() @ gy[bi, :, p].double())
                _fill(dx, (bi, slice(None), p), vs, vc)
        else:  # w[o, c]: column c of every point
            for o, c, _ in sites:
                vs, vc = both(c, lambda: torch.einsum("o,bon->bn", w[:, c].double(), f64("gy")))
                _fill(dx, (slice(None), c), vs, vc)
        out["dx"] = dx
    else:
        dw = _mask_triple((cout, cin))
        for s in sites:
            if operand == "x":
                c = s[1]
                vs, vc = both(c, lambda: torch.einsum("bon,bn->o", f64("gy"), x[:, c].double()))
                _fill(dw, (slice(None), c), vs, vc)
            else:
                o = s[1]
                vs, vc = both(o, lambda: torch.einsum("bn,bcn->c", gy[:, o].double(), f64("x")))
                _fill(dw, (o,), vs, vc)
        out["dw"] = dw
    return out


def _pw_entries():
    out = []
    for sh, (form, group) in PW_SHAPES.items():
        b, cin, cout, n = sh
        wsites = [(0, 0, 0), (cout - 1, cin - 1, 0)]
        bsites = [(0,), (cout - 1,)]
        xs, gs = _pw_elem_sites(b, cin, n), _pw_elem_sites(b, cout, n)
        opp_c = ("x", (0, 0, 0), (0, 1, 0))       # one point's reduction over channels
        opp_n = ("x", (0, 0, 0), (0, 0, 1))       # one weight column's reduction over points
        names = [("pointwise_forward", {"x": xs, "w": wsites, "bias": bsites}, opp_c, {}),
                 ("pointwise_backward_data", {"gy": gs, "w": wsites},
                  ("gy", (0, 0, 0), (0, 1, 0)), {}),
                 ("pointwise_backward_weight", {"x": xs, "gy": gs}, opp_n, {})]
        if group:
            names.append(("pointwise_forward_bnstats", {"x": xs, "w": wsites, "bias": bsites},
                          opp_c, {"group": group}))
        for name, sites, opp, params in names:
            out.append(Entry("pointwise", name, sh, pw_make(sh), sites,
                             lambda inp, name=name, group=group: pw_full_ref(name, inp, group),
                             opposing=opp, params=dict(params, form=form), masks=pw_masks))
    return out


# ---------------------------------------------------------------------------
# rows_max_bf16: torch.max(dim=1) of the same bf16 tensor, values and indices
# ---------------------------------------------------------------------------
ROWS_MAX_SHAPE = (2, 777, 6)


def rows_max_cases():
    """(label, h bf16 (B, N, C)) -- a NaN, two NaNs in one column (the lowest index
    wins), +inf beside a NaN, and the infinities alone; the reference is
    torch.max(h, dim=1) itself"""
    b, n, c = ROWS_MAX_SHAPE
    g = _gen("rows_max")
    base = _randn(g, b, n, c).bfloat16()
    nan, inf = float("nan"), float("inf")
    cases = {"nan": [((0, 300, 1), nan)], "nan_first_row": [((1, 0, 0), nan)],
             "nan_last_row": [((1, n - 1, c - 1), nan)],
             "two_nans": [((0, 500, 2), nan), ((0, 64, 2), nan)],
             "inf_beside_nan": [((1, 10, 3), inf), ((1, 400, 3), nan)],
             "nan_before_inf": [((1, 10, 4), nan), ((1, 400, 4), inf)],
             "+inf": [((0, 63, 5), inf)], "-inf": [((0, 64, 0), -inf)],
             "opposing": [((1, 127, 1), inf), ((1, 128, 1), -inf)]}
    for label, pokes in cases.items():
        h = base.clone()
        for s, v in pokes:
            h[s] = v
        yield label, h


# ---------------------------------------------------------------------------
# Scatter / gather on features: voxelization, devoxelization, grouping, row ops.
# Coordinates and indices are part of the case (always finite and in range); only
# features and gradients are injected.  pcfm.ops routes CPU tensors to pcfm.cpu_ops,
# so run_scatter serves the CPU and the GPU file.
# ---------------------------------------------------------------------------
SCATTER_SHAPES = [(2, 16, 1000, 8), (2, 64, 3000, 16)]  # (b, c, n, r)
GROUP_M, GROUP_U = 64, 8
INT_POINT, HALF_POINT = 7, 8  # a point on a voxel corner (7 zero weights), one on a face


def _scatter_geometry(shape):
    """the finite part of a case: integer voxel coordinates, float coordinates in
    [0, r - 1], grouping indices -- and what they imply (voxel of each point, corner
    indices and weights in float64)"""
    b, c, n, r = shape
    g = _gen("scatter-geo", shape)
    vc = torch.randint(0, r, (b, 3, n), generator=g, dtype=torch.int32)
    vc[:, :, 1] = vc[:, :, 0]  # points 0 and 1 share a voxel: one reduction
    pts = torch.rand(b, 3, n, generator=g) * (r - 1)
    pts[:, :, 1] = pts[:, :, 0]
    pts[:, :, INT_POINT] = torch.tensor([2.0, 3.0, 1.0])[None, :]
    pts[:, :, HALF_POINT] = torch.tensor([2.0, 3.5, 1.25])[None, :]
    gidx = torch.randint(0, n, (b, GROUP_M, GROUP_U), generator=g, dtype=torch.int32)
    gidx[:, 0, 1] = gidx[:, 0, 0]  # two slots of one point
    ind = (vc[:, 0].long() * r + vc[:, 1].long()) * r + vc[:, 2].long()
    x = pts.double()
    fl = x.floor()
    f1 = x - fl
    f0 = 1.0 - f1
    base = (fl[:, 0].long() * r + fl[:, 1].long()) * r + fl[:, 2].long()
    d = [(f1[:, 0] > 0).long() * r * r, (f1[:, 1] > 0).long() * r, (f1[:, 2] > 0).long()]
    inds, wgts, ginds = [], [], []
    for k in range(8):
        kx, ky, kz = (k >> 2) & 1, (k >> 1) & 1, k & 1
        inds.append(base + kx * d[0] + ky * d[1] + kz * d[2])
        ginds.append(base + kx * r * r + ky * r + kz)  # the corner's own cell
        wgts.append((f1[:, 0] if kx else f0[:, 0]) * (f1[:, 1] if ky else f0[:, 1])
                    * (f1[:, 2] if kz else f0[:, 2]))
    ginds = torch.stack(ginds, 1)
    assert int(ginds.max()) < r ** 3  # every corner cell is inside the grid
    return {"vc": vc, "pts": pts, "gidx": gidx, "ind": ind, "inds": torch.stack(inds, 1),
            "wgts": torch.stack(wgts, 1), "ginds": ginds}


def _scatter_make(shape, geo):
    def make():
        b, c, n, r = shape
        g = _gen("scatter", shape)
        s = r ** 3
        cnt = torch.zeros(b, s, dtype=torch.int32)
        cnt.scatter_add_(1, geo["ind"], torch.ones(b, n, dtype=torch.int32))
        return {"features": _randn(g, b, c, n), "grad_n": _randn(g, b, c, n),
                "grid": _randn(g, b, c, s), "grad_s": _randn(g, b, c, s),
                "grad_g": _randn(g, b, c, GROUP_M, GROUP_U),
                "vc": geo["vc"], "pts": geo["pts"], "gidx": geo["gidx"],
                "ind": geo["ind"].int(), "cnt": cnt, "inds": geo["inds"].int(),
                "wgts": geo["wgts"].float(), "ginds": geo["ginds"].int()}
    return make


def scatter_ref(name, inp, shape, folded=False):
    b, c, n, r = shape
    s = r ** 3
    ind = inp["ind"].long()
    name = name.replace("_planned", "")
    if name.startswith("avg_voxelize"):
        cnt = inp["cnt"].double()
        w = torch.gather(1.0 / cnt.clamp_min(1.0), 1, ind)[:, None, :]
        idx = ind[:, None, :].expand(b, c, n)
        if name.endswith("forward"):
            out = torch.zeros(b, c, s, dtype=torch.float64)
            out.scatter_add_(2, idx, inp["features"].double() * w)
            return {"out": out, "ind": inp["ind"], "cnt": inp["cnt"]}
        return {"grad_x": torch.gather(inp["grad_s"].double(), 2, idx) * w}
    if name.startswith("trilinear_devoxelize"):
        inds, wgts = inp["inds"].long(), inp["wgts"].double()
        if name.endswith("forward"):
            grid = inp["grid"].double()
            out = torch.zeros(b, c, n, dtype=torch.float64)
            for k in range(8):  # 0 * inf is NaN: the zero-weight corners count
                out = out + wgts[:, k:k + 1] * torch.gather(
                    grid, 2, inds[:, k:k + 1].expand(b, c, n))
            return {"outs": out, "inds": inp["inds"], "wgts": wgts}
        # DOCUMENTED DEVIATION (DESIGN.md "Non-finite values"): where a coordinate's
        # fraction is 0 the forward's saved index folds the zero-weight corner onto the
        # low cell; the segment scatter adds that corner's w * g = 0 * g to the corner's
        # own cell ("both placements add the same zeros" -- for a finite g).  A
        # non-finite g therefore marks the point's whole geometric stencil, a superset
        # of the folded one: the expectation is the scatter over the corner cells.
        gx = torch.zeros(b, c, s, dtype=torch.float64)
        # folded: pcfm.cpu_ops scatters through the forward's folded indices
        cells = inds if folded else inp["ginds"].long()
        for k in range(8):
            gx.scatter_add_(2, cells[:, k:k + 1].expand(b, c, n),
                            wgts[:, k:k + 1] * inp["grad_n"].double())
        return {"grad_x": gx}
    gi = inp["gidx"].long().reshape(b, 1, -1).expand(b, c, GROUP_M * GROUP_U)
    if name == "grouping_forward":
        return {"out": torch.gather(inp["features"].double(), 2, gi).reshape(b, c, GROUP_M,
                                                                             GROUP_U)}
    gx = torch.zeros(b, c, n, dtype=torch.float64)
    gx.scatter_add_(2, gi, inp["grad_g"].double().reshape(b, c, -1))
    return {"grad_x": gx}


def run_scatter(ops, e, d):
    """the entry through pcfm.ops on the tensors' device -> {output: tensor}"""
    b, c, n, r = e.shape
    name = e.name
    if name == "avg_voxelize_forward":
        out, ind, cnt = ops.avg_voxelize_forward(d["features"], d["vc"], r)
        return {"out": out, "ind": ind, "cnt": cnt}
    if name == "avg_voxelize_forward_planned":
        plan = ops.avg_voxelize_plan(d["vc"], r)
        return {"out": ops.avg_voxelize_forward_planned(d["features"], plan),
                "ind": plan.ind, "cnt": plan.cnt}
    if name == "avg_voxelize_backward":
        return {"grad_x": ops.avg_voxelize_backward(d["grad_s"], d["ind"], d["cnt"])}
    if name == "trilinear_devoxelize_forward":
        outs, inds, wgts = ops.trilinear_devoxelize_forward(r, True, d["pts"], d["grid"])
        return {"outs": outs, "inds": inds, "wgts": wgts}
    if name == "trilinear_devoxelize_backward":
        return {"grad_x": ops.trilinear_devoxelize_backward(d["grad_n"], d["inds"], d["wgts"], r)}
    if name == "trilinear_devoxelize_backward_planned":
        plan = ops.trilinear_devoxelize_backward_plan(d["inds"], d["wgts"], r)
        return {"grad_x": ops.trilinear_devoxelize_backward_planned(d["grad_n"], plan)}
    if name == "grouping_forward":
        return {"out": ops.grouping_forward(d["features"], d["gidx"])}
    return {"grad_x": ops.grouping_backward(d["grad_g"], d["gidx"], n)}


# entries pcfm.ops has no CPU route for
GPU_ONLY = ("avg_voxelize_forward_planned", "trilinear_devoxelize_backward_planned", "rows_dot",
            "rows_affine_")
# gathers: no reduction, so no opposing pair
GATHERS = ("avg_voxelize_backward", "trilinear_devoxelize_forward", "grouping_forward",
           "rows_affine_", "trilinear_devoxelize_scale_add", "tgate_forward", "tgate_backward",
           "head_silu_fwd")


def _scatter_entries():
    out = []
    for sh in SCATTER_SHAPES:
        b, c, n, r = sh
        geo = _scatter_geometry(sh)
        ind, inds, gidx = geo["ind"], geo["inds"], geo["gidx"]
        pts = _pw_elem_sites(b, c, n)  # (b, c, point): first, last, the tile edges
        # occupied voxels (the gradient of an empty voxel is never read); voxels some
        # point reads: corner 0 of a few points, the corner point's voxel among them
        occ = [(bi, ci, int(ind[bi, p])) for bi, ci, p in pts]
        read = [(bi, ci, int(inds[bi, 0, p])) for bi, ci, p in pts[:2]] + [
            (0, 1, int(inds[0, 0, INT_POINT])), (b - 1, c - 1, int(inds[b - 1, 7, HALF_POINT]))]
        grp_f = [(0, 0, int(gidx[0, 0, 0])), (b - 1, c - 1, int(gidx[b - 1, -1, -1]))]
        grp_g = [(0, 0, 0, 0), (b - 1, c - 1, GROUP_M - 1, GROUP_U - 1), (b - 1, c // 2, 31, 7),
                 (b - 1, c // 2, 32, 0)]
        corner = [(0, 0, INT_POINT), (b - 1, c - 1, HALF_POINT)]
        table = [
            ("avg_voxelize_forward", {"features": pts}, ("features", (0, 0, 0), (0, 0, 1))),
            ("avg_voxelize_forward_planned", {"features": pts},
             ("features", (0, 0, 0), (0, 0, 1))),
            ("avg_voxelize_backward", {"grad_s": occ}, None),
            ("trilinear_devoxelize_forward", {"grid": read}, None),
            ("trilinear_devoxelize_backward", {"grad_n": pts + corner},
             ("grad_n", (0, 0, 0), (0, 0, 1))),
            ("trilinear_devoxelize_backward_planned", {"grad_n": pts + corner},
             ("grad_n", (0, 0, 0), (0, 0, 1))),
            ("grouping_forward", {"features": grp_f}, None),
            ("grouping_backward", {"grad_g": grp_g}, ("grad_g", (0, 0, 0, 0), (0, 0, 0, 1))),
        ]
        for name, sites, opp in table:
            out.append(Entry("scatter", name, sh, _scatter_make(sh, geo), sites,
                             lambda inp, name=name, sh=sh: scatter_ref(name, inp, sh),
                             opposing=opp,
                             cpu_ref=lambda inp, name=name, sh=sh: scatter_ref(name, inp, sh, True)))
    return out


# ---------------------------------------------------------------------------
# Voxel convolution (3 x 3 x 3, padding 1) on split operands: forward,
# backward-data (the transposed image), weight gradient.  The injected operands are
# the voxel tensors and the bias; a non-finite WEIGHT is pinned at the image
# (conv3d_prep_weight), because what an inf weight does at the grid's border is the
# padding's 0 * inf, which F.conv3d and an implicit GEMM may each decide either way.
# ---------------------------------------------------------------------------
# (b, cin, cout, r) -> the forward form tests/test_gpu_conv3d.py pins it to
CONV_SHAPES = {(3, 128, 128, 8): "split-K LDS-DMA", (2, 256, 256, 8): "window",
               (5, 128, 256, 16): "slab<16>", (2, 128, 128, 32): "slab<32>"}


# split-K launches of the forward (1: the unsplit slab forms), from the workspace query
CONV_SPLITS = {(3, 128, 128, 8): 8, (2, 256, 256, 8): 8, (5, 128, 256, 16): 1,
               (2, 128, 128, 32): 1}


def _conv_make(shape):
    def make():
        b, cin, cout, r = shape
        g = _gen("conv", shape)
        return {"x": _randn(g, b, cin, r, r, r), "gy": _randn(g, b, cout, r, r, r),
                "w": _randn(g, cout, cin, 3, 3, 3) / (27 * cin) ** 0.5, "bias": _randn(g, cout)}
    return make


def conv_full_ref(name, inp):
    x, gy, w = inp["x"].double(), inp["gy"].double(), inp["w"].double()
    if name == "conv3d_forward":
        return {"y": F.conv3d(x, w, inp["bias"].double(), padding=1)}
    if name == "conv3d_backward_data":
        return {"dx": torch.nn.grad.conv3d_input(x.shape, w, gy, padding=1)}
    return {"dw": torch.nn.grad.conv3d_weight(x, w.shape, gy, padding=1)}


def _window(t, bi, pos, r):
    """t[bi] around voxel pos, two voxels each way, zero outside the grid: (1, C, 5, 5, 5)"""
    z, y, x = pos
    p = F.pad(t[bi:bi + 1].double(), (2, 2, 2, 2, 2, 2))
    return p[:, :, z:z + 5, y:y + 5, x:x + 5]


def conv_masks(entry, inp, operand, sites_kinds):
    """Entry.classify without a full float64 convolution per injection: a voxel enters
    its 27-neighbourhood clipped to the grid (a corner voxel: 8 outputs), evaluated on
    a 5^3 window of the special and the clean inputs; a bias element its channel; in
    the weight gradient a voxel of x (of grad_y) enters the taps of its input
    channel's column (output channel's row) whose partner voxel is inside the grid.
    tests/test_nonfinite_cpu.py holds this against the full reference at r = 8."""
    name, (b, cin, cout, r) = entry.name, entry.shape
    cache = entry.__dict__.setdefault("_cache", {})
    out = {}

    def f64(k):  # the float64 copy of an operand this injection leaves alone
        assert k != operand
        if k not in cache:
            cache[k] = inp[k].double()
        return cache[k]

    def both(key, fn):  # fn on the special and the clean inputs (clean: once per site)
        key = (operand, key, tuple(s for s, _ in sites_kinds))
        if key not in cache:
            cache[key] = fn()
        with poked(inp, operand, sites_kinds):
            return fn(), cache[key]
    w64 = f64("w")

    def nbhd(pos):
        lo = [max(0, p - 1) for p in pos]
        hi = [min(r, p + 2) for p in pos]
        return tuple(slice(a, e) for a, e in zip(lo, hi)), tuple(
            slice(a - p + 1, e - p + 1) for a, e, p in zip(lo, hi, pos))

    if name in ("conv3d_forward", "conv3d_backward_data"):
        fwd = name == "conv3d_forward"
        src, key, ch = ("x", "y", cout) if fwd else ("gy", "dx", cin)
        tri = _mask_triple((b, ch, r, r, r))
        for s in [s for s, _ in sites_kinds]:
            if operand == "bias":
                o = s[0]
                if ("conv", o) not in cache:  # x and w are not injected here
                    cache[("conv", o)] = F.conv3d(f64("x"), w64[o:o + 1], padding=1)[:, 0]
                vs, vc = both(s, lambda: cache[("conv", o)] + inp["bias"][o].double())
                _fill(tri, (slice(None), o), vs, vc)
                continue
            bi, pos = s[0], s[2:]

            def local():  # the 3^3 outputs around pos from the 5^3 window
                win = _window(inp[src], bi, pos, r)
                if fwd:
                    return F.conv3d(win, w64, inp["bias"].double())[0]
                return F.conv3d(win, w64.transpose(0, 1).flip(2, 3, 4))[0]
            vs, vc = both(s, local)
            g, l = nbhd(pos)
            _fill(tri, (bi, slice(None)) + g, vs[(slice(None),) + l], vc[(slice(None),) + l])
        out[key] = tri
    else:
        # dw[o, c, tap] = sum over (b, p) of gy[b, o, p] * x[b, c, p + tap - 1]: the clean
        # column (row) once per channel, and in it the injected voxel's own 27 products
        # replaced by their special values
        tri = _mask_triple((cout, cin, 3, 3, 3))
        sites = [s for s, _ in sites_kinds]
        other = "gy" if operand == "x" else "x"
        sign = -1 if operand == "x" else 1

        def products():
            res = []
            for bi, c, z, y, xx in sites:
                t = torch.zeros((inp[other].shape[1], 3, 3, 3), dtype=torch.float64)
                for tz in range(3):
                    for ty in range(3):
                        for tx in range(3):
                            q = (z + sign * (tz - 1), y + sign * (ty - 1), xx + sign * (tx - 1))
                            v = inp[operand][bi, c, z, y, xx].double()
                            if all(0 <= i < r for i in q):
                                t[:, tz, ty, tx] = inp[other][bi, :, q[0], q[1], q[2]].double() * v
                            elif operand == "gy":
                                # x is zero-padded and the padding counts: 0 * inf is NaN,
                                # as torch.nn.grad.conv3d_weight decides it
                                t[:, tz, ty, tx] = 0.0 * v
                res.append(t)
            return res
        clean_p = products()
        with poked(inp, operand, sites_kinds):
            spec_p = products()
        for c in sorted({s[1] for s in sites}):
            key = ("dw", operand, c)
            if key not in cache:
                if operand == "x":
                    cache[key] = torch.nn.grad.conv3d_weight(
                        inp["x"][:, c:c + 1].double(), (cout, 1, 3, 3, 3), f64("gy"),
                        padding=1)[:, 0]
                else:
                    cache[key] = torch.nn.grad.conv3d_weight(
                        f64("x"), (1, cin, 3, 3, 3), inp["gy"][:, c:c + 1].double(), padding=1)[0]
            vs = cache[key].clone()
            for s, tc, ts in zip(sites, clean_p, spec_p):
                if s[1] == c:
                    vs = (vs - tc) + ts
            _fill(tri, (slice(None), c) if operand == "x" else (c,), vs, cache[key])
        out["dw"] = tri
    return out


def run_conv(ops, e, d):
    b, cin, cout, r = e.shape
    if e.name == "conv3d_forward":
        img = ops.conv3d_prep_weight(d["w"], False)
        return {"y": ops.conv3d_igemm_split(ops.conv3d_split(d["x"]), img, d["bias"], b, cin, cout,
                                            r, "conv3d_fwd")}
    if e.name == "conv3d_backward_data":
        img = ops.conv3d_prep_weight(d["w"], True)
        return {"dx": ops.conv3d_igemm_split(ops.conv3d_split(d["gy"]), img, None, b, cout, cin, r,
                                             "conv3d_bwd_data")}
    return {"dw": ops.conv3d_wgrad_split(ops.conv3d_split(d["x"]), ops.conv3d_split(d["gy"]), b,
                                         cin, cout, r)}


def _conv_entries():
    out = []
    for sh, form in CONV_SHAPES.items():
        b, cin, cout, r = sh
        m = r // 2

        def vox(c):  # a corner, a face, an interior voxel, the last voxel
            return [(0, 0, 0, 0, 0), (b - 1, c // 2, 0, m, m), (b - 1, c - 1, m, m - 1, m + 1),
                    (b - 1, c - 1, r - 1, r - 1, r - 1)]
        opp = ((0, 1, m, m, m), (0, 2, m, m, m + 1))  # two channels / voxels of one output
        bsites = [(0,), (cout - 1,)]
        for name, sites, o in (
                ("conv3d_forward", {"x": vox(cin), "bias": bsites}, ("x",) + opp),
                ("conv3d_backward_data", {"gy": vox(cout)}, ("gy",) + opp),
                ("conv3d_backward_weight", {"x": vox(cin), "gy": vox(cout)},
                 ("x", (0, 1, m, m, m), (0, 1, m, m, m + 1)))):
            out.append(Entry("conv3d", name, sh, _conv_make(sh), sites,
                             lambda inp, name=name: conv_full_ref(name, inp), opposing=o,
                             params={"form": form.replace(" ", "_")}, masks=conv_masks))
    return out


ROWS_SHAPE = (5, 1028)  # 257 float4 per row: a one-float4 second block in rows_affine_


def _rows_make():
    g = _gen("rows", ROWS_SHAPE)
    r, n = ROWS_SHAPE
    return {"a": _randn(g, r, n), "b": _randn(g, r, n), "s": _randn(g, r), "t": _randn(g, r)}


def run_rows(ops, e, d):
    if e.name == "rows_dot":
        return {"out": ops.rows_dot(d["a"], d["b"], 0.5)}
    return {"x": ops.rows_affine_(d["a"].clone(), d["s"], d["t"])}


def _rows_entries():
    r, n = ROWS_SHAPE
    elem = [(0, 0), (r - 1, n - 1), (2, 1023), (2, 1024)] + [(3, p) for p in (63, 64, 127, 128)]
    row = [(0,), (r - 1,)]
    return [
        Entry("scatter", "rows_dot", ROWS_SHAPE, _rows_make, {"a": elem, "b": elem},
              lambda inp: {"out": 0.5 * (inp["a"].double() * inp["b"].double()).sum(1)},
              opposing=("a", (1, 0), (1, 1))),
        Entry("scatter", "rows_affine_", ROWS_SHAPE, _rows_make, {"a": elem, "s": row, "t": row},
              lambda inp: {"x": inp["s"].double()[:, None] * inp["a"].double()
                           + inp["t"].double()[:, None]}),
    ]


def all_entries():
    import nonfinite_more  # (imports this module: resolved at call time)
    return (_bn_entries() + _gn_entries() + _se_entries() + _pw_entries() + _conv_entries()
            + _scatter_entries() + _rows_entries() + nonfinite_more.entries())
