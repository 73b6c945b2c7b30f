"""A guarded allocator for the C-ABI memory contract (include/pcfm.h).

While `GuardedAlloc` is active every buffer pcfm.ops and pcfm.optim allocate --
`torch.empty`, `torch.empty_like`, `torch.zeros`, `torch.zeros_like` and
`ops._workspace`, the only ways they allocate -- is a view into an *arena*: one ordinary torch allocation
of GUARD + payload + GUARD bytes.  Only the name `torch` inside those two modules
is swapped (for a proxy that forwards everything else); the global torch module
is untouched.

Fill policy -- a defect shows as a wrong answer, never as a wild address:
  * guards of an allocated buffer: the byte GUARD_BYTE, checked byte for byte;
  * float payloads of empty-style calls: a NaN bit pattern (POISON);
  * zeros-style calls: zero;
  * integer payloads and uint8 workspaces: zero on a fresh arena, and on a
    *stale* session the bytes the previous call of the same shape left there
    (a made-up integer could be used as an index);
  * `guarded(t)`: a test input with NaN guards (float) or 0 guards (integer --
    0 is a valid index everywhere in this ABI), so an over-read that is used
    changes the answer.

A stale session (`GuardedAlloc(stale=previous)`) hands the previous session's
arenas back, in allocation order, with every payload as that session left it
(zeros-style payloads are zeroed again: the wrapper asked for zeros).

Not a conftest and not a plugin: tests import it like golden_util.
"""
from __future__ import annotations

import sys

import torch

GUARD = 4096          # bytes; a multiple of the caching allocator's 512-byte alignment
GUARD_BYTE = 0xC9
# NaN bit patterns (quiet NaNs with a recognisable payload), by element size
POISON = {2: 0x7FD5, 4: 0x7FD5A5C9, 8: 0x7FF5A5C9A5C9A5C9}
_INT_OF_SIZE = {2: torch.int16, 4: torch.int32, 8: torch.int64}
_FLOATS = (torch.float32, torch.bfloat16, torch.float64, torch.float16)


def _is_float(dtype) -> bool:
    return dtype in _FLOATS


def _numel(shape) -> int:
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _shape(args, kwargs):
    if "size" in kwargs:
        args = (kwargs["size"],)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


class Arena:
    """guard | payload | guard in one allocation; `view` is the payload."""

    def __init__(self, site, kind, shape, dtype, device):
        self.site, self.kind = site, kind          # kind: empty / zeros / ws / input
        self.shape, self.dtype = tuple(shape), dtype
        self.nbytes = _numel(shape) * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.empty(2 * GUARD + self.nbytes, dtype=torch.uint8, device=device)
        self.view = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(self.shape)
        self.guard_expect = None                   # (GUARD,) uint8: what both guards hold

    # ---- fills -----------------------------------------------------------
    def _fill_nan(self, t):
        """t: a uint8 tensor whose length is a multiple of the element size."""
        es = torch.empty((), dtype=self.dtype).element_size()
        t.view(_INT_OF_SIZE[es]).fill_(POISON[es])

    def fill_guards(self, nan: bool, byte: int = 0):
        front, rear = self.raw[:GUARD], self.raw[GUARD + self.nbytes:]
        for g in (front, rear):
            if nan:
                self._fill_nan(g)
            else:
                g.fill_(byte)
        self.guard_expect = front.clone()

    def fill_payload(self, how: str):
        pay = self.raw[GUARD:GUARD + self.nbytes]
        if how == "nan":
            self._fill_nan(pay)
        else:
            pay.zero_()

    # ---- checks (device tensors; the session gathers them in one copy) -----
    def guard_damage(self):
        front, rear = self.raw[:GUARD], self.raw[GUARD + self.nbytes:]
        return torch.stack([(front != self.guard_expect).sum(),
                            (rear != self.guard_expect).sum()])

    def poison_mask(self):
        """Boolean mask, shaped like the payload, of elements still holding POISON."""
        es = self.view.element_size()
        return self.view.view(_INT_OF_SIZE[es]) == POISON[es]

    def __repr__(self):
        return f"<{self.kind} {self.site} {tuple(self.shape)} {self.dtype}>"


class Report:
    def __init__(self, arenas, damage, poison):
        self.arenas = arenas
        # [(arena, front_bytes, rear_bytes)] of the touched guards
        self.touched = [(a, f, r) for a, (f, r) in zip(arenas, damage) if f or r]
        # {arena: count} of float empty-style payload elements still holding POISON
        self.poison_left = {a: n for a, n in zip(arenas, poison) if n}

    def sites(self):
        return [a.site for a in self.arenas]

    def workspace_bytes(self):
        return [a.nbytes for a in self.arenas if a.kind == "ws"]

    def describe(self):
        out = []
        for a, f, r in self.touched:
            out.append(f"guard touched at {a}: {f} bytes before, {r} bytes after the payload")
        for a, n in self.poison_left.items():
            out.append(f"poison left at {a}: {n} elements never written")
        return "\n".join(out)

    def assert_guards_intact(self):
        assert not self.touched, self.describe()


class _Proxy:
    """Stands in for the name `torch` inside one module: forwards every attribute
    to the real module, overrides the allocation functions."""

    def __init__(self, session):
        self.__dict__["_s"] = session

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, dtype=None, device=None, **kw):
        return self._s._alloc("empty", _shape(args, kw), dtype, device)

    def zeros(self, *args, dtype=None, device=None, **kw):
        return self._s._alloc("zeros", _shape(args, kw), dtype, device)

    def empty_like(self, t, dtype=None, device=None, **kw):
        if not t.is_contiguous():
            raise AssertionError("guard_alloc: empty_like of a non-contiguous tensor")
        return self._s._alloc("empty", tuple(t.shape), dtype or t.dtype, device or t.device)

    def zeros_like(self, t, dtype=None, device=None, **kw):
        return self._s._alloc("zeros", tuple(t.shape), dtype or t.dtype, device or t.device)


def _gather(ts):
    """Host values of a list of small tensors (None -> 0): the device ones in one copy."""
    out = [0] * len(ts)
    dev = [i for i, t in enumerate(ts) if t is not None and t.is_cuda]
    if dev:
        flat = torch.stack([ts[i] for i in dev])
        for i, v in zip(dev, flat.cpu().tolist()):
            out[i] = v
    for i, t in enumerate(ts):
        if t is not None and not t.is_cuda:
            out[i] = t.tolist()
    return out


class GuardedAlloc:
    """Context manager; `modules` are the modules whose `torch` name (and
    `_workspace`, where present) are redirected -- pcfm.ops and pcfm.optim unless
    a test passes its own (the CPU self-tests use a fake module).  On exit
    `.report` holds the arenas, the touched guards and the surviving poison."""

    def __init__(self, modules=None, stale: "GuardedAlloc | None" = None):
        if modules is None:
            from pcfm import ops, optim
            modules = (ops, optim)
        self.modules = tuple(modules)
        self.arenas = []
        self.inputs = []
        self._replay = list(stale.arenas) if stale is not None else None
        self._seq = {}
        self._saved = []
        self.report = None

    # ---- allocation ------------------------------------------------------
    _OWN = ("_site", "_alloc", "_workspace", "empty", "zeros", "empty_like", "zeros_like",
            "<lambda>", "<listcomp>", "<genexpr>")

    def _site(self, kind):
        """`wrapper#k:kind`: the function that asked, and its k-th allocation."""
        f = sys._getframe(1)
        while f is not None and f.f_code.co_name in self._OWN:
            f = f.f_back
        name = f.f_code.co_name if f is not None else "?"
        k = self._seq.get(name, 0)
        self._seq[name] = k + 1
        return f"{name}#{k}:{kind}"

    def _alloc(self, kind, shape, dtype, device):
        dtype = dtype or torch.get_default_dtype()
        device = torch.device(device) if device is not None else torch.device("cpu")
        site = self._site(kind)
        if self._replay is not None:
            if not self._replay:
                raise AssertionError(f"guard_alloc: stale run allocates more than the first "
                                     f"call did (at {site})")
            a = self._replay.pop(0)
            same = (a.site, a.shape, a.dtype, a.raw.device.type) == (site, tuple(shape), dtype,
                                                                    device.type)
            if not same:
                raise AssertionError(f"guard_alloc: stale run asks for {site} {tuple(shape)} "
                                     f"{dtype}, the first call had {a}")
            if kind == "zeros":
                a.fill_payload("zero")
        else:
            a = Arena(site, kind, shape, dtype, device)
            a.fill_guards(nan=False, byte=GUARD_BYTE)
            a.fill_payload("nan" if kind == "empty" and _is_float(dtype) else "zero")
        self.arenas.append(a)
        return a.view

    def _workspace(self, nbytes, like):
        return self._alloc("ws", (max(int(nbytes), 1),), torch.uint8, like.device)

    def guarded(self, t: torch.Tensor) -> torch.Tensor:
        """A copy of the input t inside an arena whose guards are NaN (float) or 0."""
        t = t.detach()
        a = Arena(f"input#{len(self.inputs)}", "input", tuple(t.shape), t.dtype, t.device)
        a.fill_guards(nan=_is_float(t.dtype), byte=0)
        a.view.copy_(t.contiguous())
        self.inputs.append(a)
        return a.view

    # ---- the context -----------------------------------------------------
    def __enter__(self):
        proxy = _Proxy(self)
        for m in self.modules:
            self._saved.append((m, "torch", m.__dict__["torch"]))
            m.__dict__["torch"] = proxy
            if "_workspace" in m.__dict__:
                self._saved.append((m, "_workspace", m.__dict__["_workspace"]))
                m.__dict__["_workspace"] = lambda nbytes, like: self._workspace(nbytes, like)
        return self

    def __exit__(self, *exc):
        for m, name, old in reversed(self._saved):
            m.__dict__[name] = old
        self._saved = []
        if exc[0] is None:
            self.check()
        return False

    def _checks_poison(self, a) -> bool:
        return (a.kind == "empty" and _is_float(a.dtype) and a.nbytes > 0
                and self._replay is None)

    def check(self) -> Report:
        every = self.arenas + self.inputs
        if any(a.raw.is_cuda for a in every):
            torch.cuda.synchronize()
        damage = _gather([a.guard_damage() for a in every])
        poison = _gather([a.poison_mask().sum() if self._checks_poison(a) else None
                          for a in every])
        self.report = Report(every, damage, poison)
        return self.report


def poison_left(out: torch.Tensor, plain: torch.Tensor) -> int:
    """Elements of a float output that still hold POISON where the plain run's
    element is not NaN."""
    if not _is_float(out.dtype) or out.numel() == 0:
        return 0
    es = out.element_size()
    o = out.contiguous()
    mask = o.view(_INT_OF_SIZE[es]) == POISON[es]
    return int((mask & ~torch.isnan(plain.contiguous())).sum())
