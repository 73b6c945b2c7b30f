"""The guarded allocator (tests/guard_alloc.py) seen to detect: fake ops -- plain
Python on CPU tensors, allocated the way pcfm.ops allocates -- that overrun an
output, leave an element unwritten or consume stale workspace bytes are
reported, and a correct op passes.  The proxy mechanics are the same on a HIP
device, so these are the evidence that tests/test_gpu_abi_contract.py would
fail on such a kernel."""
import types

import pytest
import torch

import guard_alloc as ga

# a module that allocates like pcfm.ops: through its own name `torch` and `_workspace`
_SRC = '''
import torch


def _workspace(nbytes, like):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=like.device)


def _raw(t, extra):
    """The kernel's view of a pointer: the bytes at t's address, `extra` bytes past its end."""
    return t.new_empty(0).set_(t.untyped_storage(), t.storage_offset(), (t.numel() + extra,))


def scale_ok(x):
    out = torch.empty_like(x)
    ws = _workspace(4 * x.numel(), x)
    acc = ws.view(torch.float32)
    acc.zero_()                      # initialises the scratch it accumulates into
    acc += x.reshape(-1)
    out.copy_((2.0 * acc).view_as(x))
    return out


def scale_overrun(x):
    y = torch.empty((3,), dtype=torch.float32, device=x.device)      # bystander
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    out.copy_(2.0 * x)
    _raw(out.reshape(-1), 1)[-1] = 7.0                               # one element too far
    y.zero_()
    return out


def scale_underrun(x):
    out = torch.empty_like(x)
    out.new_empty(0).set_(out.untyped_storage(), out.storage_offset() - 1, (1,))[0] = 7.0
    out.copy_(2.0 * x)
    return out


def scale_hole(x):
    out = torch.empty_like(x)
    flat = out.reshape(-1)
    flat[:-1] = 2.0 * x.reshape(-1)[:-1]                             # last element never written
    return out


def scale_stale(x):
    out = torch.empty_like(x)
    ws = _workspace(4 * x.numel(), x)
    acc = ws.view(torch.float32)
    acc += x.reshape(-1)                                             # no initialisation
    out.copy_((2.0 * acc).view_as(x))
    return out


def count_stale(x):
    """An integer output that is incremented, not written."""
    cnt = torch.empty((4,), dtype=torch.int32, device=x.device)
    cnt += (x.reshape(-1)[:4] > 0).to(torch.int32)
    return cnt


def zeros_then_add(x):
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)  # asked for zeros
    out += x
    return out
'''


@pytest.fixture()
def fake():
    m = types.ModuleType("fake_ops")
    exec(compile(_SRC, "fake_ops.py", "exec"), m.__dict__)
    return m


def _x(seed=0, shape=(3, 5)):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def _triple(fake, op, x, other):
    """plain / guarded / stale, as the GPU contract test runs a row."""
    plain = op(x)
    with ga.GuardedAlloc(modules=(fake,)) as g:
        got = op(g.guarded(x))
    with ga.GuardedAlloc(modules=(fake,)) as first:
        op(first.guarded(other))
    with ga.GuardedAlloc(modules=(fake,), stale=first) as st:
        stale = op(st.guarded(x))
    return plain, got, g.report, stale, st.report


def test_correct_op_passes(fake):
    x = _x()
    plain, got, rep, stale, srep = _triple(fake, fake.scale_ok, x, _x(1))
    rep.assert_guards_intact()
    srep.assert_guards_intact()
    assert ga.poison_left(got, plain) == 0
    assert torch.equal(got, plain) and torch.equal(stale, plain)
    assert rep.sites() == ["scale_ok#0:empty", "scale_ok#1:ws", "input#0"]
    assert rep.workspace_bytes() == [4 * x.numel()]     # the byte count passed through
    assert fake.torch is torch and fake._workspace.__name__ == "_workspace"  # restored


def test_write_past_the_output_is_reported(fake):
    x = _x()
    with ga.GuardedAlloc(modules=(fake,)) as g:
        fake.scale_overrun(g.guarded(x))
    rep = g.report
    assert [(a.site, f, r) for a, f, r in rep.touched] == [("scale_overrun#1:empty", 0, 4)]
    with pytest.raises(AssertionError, match=r"scale_overrun#1:empty.*4 bytes after"):
        rep.assert_guards_intact()


def test_write_before_the_output_is_reported(fake):
    with ga.GuardedAlloc(modules=(fake,)) as g:
        fake.scale_underrun(g.guarded(_x()))
    assert [(a.site, f, r) for a, f, r in g.report.touched] == [("scale_underrun#0:empty", 4, 0)]


def test_unwritten_output_element_is_reported(fake):
    x = _x()
    plain = fake.scale_hole(x)
    with ga.GuardedAlloc(modules=(fake,)) as g:
        got = fake.scale_hole(g.guarded(x))
    g.report.assert_guards_intact()
    assert ga.poison_left(got, plain) == 1
    assert {a.site: n for a, n in g.report.poison_left.items()} == {"scale_hole#0:empty": 1}
    assert not torch.equal(got, plain)


def test_stale_workspace_dependence_is_caught(fake):
    x = _x()
    plain = 2.0 * x
    _, got, rep, stale, srep = _triple(fake, fake.scale_stale, x, _x(1))
    rep.assert_guards_intact()
    srep.assert_guards_intact()
    assert torch.equal(got, plain)          # a zeroed workspace hides it ...
    assert not torch.equal(stale, plain)    # ... the previous call's bytes do not


def test_stale_integer_output_dependence_is_caught(fake):
    x, other = torch.ones(3, 5), torch.ones(3, 5)
    with ga.GuardedAlloc(modules=(fake,)) as first:
        want = fake.count_stale(first.guarded(other)).clone()
    with ga.GuardedAlloc(modules=(fake,), stale=first) as st:
        got = fake.count_stale(st.guarded(x))
    assert want.tolist() == [1, 1, 1, 1] and got.tolist() == [2, 2, 2, 2]


def test_zeros_stay_zeros_in_a_stale_run(fake):
    x = _x()
    plain, got, rep, stale, _ = _triple(fake, fake.zeros_then_add, x, _x(1))
    assert torch.equal(got, plain) and torch.equal(stale, plain)


def test_payload_alignment_and_fills(fake):
    with ga.GuardedAlloc(modules=(fake,)) as g:
        f = fake.torch.empty((2, 3), dtype=torch.float32)
        h = fake.torch.empty((5,), dtype=torch.bfloat16)
        d = fake.torch.empty((2,), dtype=torch.float64)
        i = fake.torch.empty((7,), dtype=torch.int32)
        z = fake.torch.empty((0, 4), dtype=torch.float32)
        xin = g.guarded(torch.arange(6, dtype=torch.int32))
        fin = g.guarded(torch.ones(3))
    for t in (f, h, d):
        assert torch.isnan(t).all() and t.is_contiguous()
    assert i.tolist() == [0] * 7 and z.shape == (0, 4)
    for a in g.arenas + g.inputs:
        if a.nbytes == 0:       # an empty tensor's data_ptr() is 0, as for torch.empty(0)
            continue
        assert (a.view.data_ptr() - a.raw.data_ptr()) == ga.GUARD and ga.GUARD % 512 == 0
    # the input guards: zeros around integers, NaN around floats
    a_int, a_flt = g.inputs
    assert int(a_int.raw[:ga.GUARD].sum()) == 0 and xin.tolist() == list(range(6))
    assert torch.isnan(a_flt.raw[:ga.GUARD].view(torch.float32)).all()
    assert torch.isnan(a_flt.raw[ga.GUARD + 12:].view(torch.float32)).all() and fin.sum() == 3
    g.report.assert_guards_intact()


def test_stale_run_refuses_a_different_allocation_sequence(fake):
    with ga.GuardedAlloc(modules=(fake,)) as first:
        fake.scale_ok(_x())
    with pytest.raises(AssertionError, match="stale run asks for"):
        with ga.GuardedAlloc(modules=(fake,), stale=first):
            fake.scale_ok(_x(shape=(2, 2)))
    assert fake.torch is torch
