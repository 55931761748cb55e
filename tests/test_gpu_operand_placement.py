"""Every kernel entry point on operands that sit at a 4-byte but not a 16-byte boundary (tests/placement_cases.py; the host
half is tests/test_placement_host.py).

The library tests pointer alignment in many places ("Operand alignment") and no other test hands it an
operand off 16 bytes: the allocator aligns to 512. Per case: the call on aligned operands against the case's fp64
reference, then (a) every operand a caller supplies placed 1, 2 and 3 floats past a 16-byte boundary (labels 8 bytes,
byte masks 1 / 4 / 15 bytes), (b) each such operand placed alone with the others aligned - a test that ORs pointers and
forgets one shows only this way. Each run must: not raise; stay within the case's bound of the reference; for
elementwise and data-movement kernels (and Adam) equal the aligned call bit for bit; leave the guard elements around every
operand and every operand it does not write untouched. No (case, operand) pair is marked as refused: include/m2d.h asks
for a float's alignment everywhere these calls reach."""
import pytest
import torch

from tests import placement_cases as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {}   # printed by tests/conftest.py with every run


def K():
    from music2dance_amd import kernels
    return kernels.impl()


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))
    return val


def bits(t):
    """the tensor's bit patterns (a NaN - an undefined cell of a metric - equals itself)"""
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def offset(t, k):
    """placement k (1, 2, 3) in the operand's own unit"""
    if t.dtype == torch.uint8:
        return {1: 1, 2: 4, 3: 15}[k]
    return k if t.element_size() == 4 else 1   # (8-byte elements: the one residue they can have)


def run_placed(case, offs):
    """operands of `case` on the device, operand `name` placed at offs.get(name, 0) -> (results, operands, buffers)"""
    t, bufs = {}, {}
    for name, cpu in case.operands().items():
        t[name], bufs[name] = P.place(cpu, offs.get(name, 0), DEV)
    outs = tuple(case.run(K(), t))
    torch.cuda.synchronize()
    K().check_async_errors()
    return outs, t, bufs


def check(case, what, outs, t, bufs, base):
    ref = case.reference()
    assert len(outs) == len(ref), (case.name, what)
    for i, (o, r, tol) in enumerate(zip(outs, ref, case.tols(len(ref)))):
        if r is not None:
            ok, fig = P.within(o, r, tol)
            print("%s | %s | result %d: %.3e (bound %s)" % (case.name, what, i, fig, getattr(tol, "__name__", tol)))
            if not isinstance(tol, tuple) and tol is not None:
                note("placement " + "/".join(case.ops), fig)
            assert ok, (case.name, what, i, fig, tol)
        if case.exact and base is not None:
            assert torch.equal(bits(o.cpu()), bits(base[i])), (case.name, what, i, "differs from the call on aligned operands",
                                                               float((o.cpu().double() - base[i].double()).abs().nan_to_num().max()))
    if case.extra is not None:
        case.extra(outs, t)
    for name, cpu in case.operands().items():
        assert P.guards_intact(bufs[name], t[name]), (case.name, what, "guard elements around %s were written" % name)
        if name not in case.written:
            assert torch.equal(t[name].cpu(), cpu), (case.name, what, "operand %s was written" % name)


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c.name)
def test_operands_off_16_byte_alignment(case):
    ops = case.operands()
    outs, t, bufs = run_placed(case, {})
    check(case, "aligned", outs, t, bufs, None)
    base = [o.cpu() for o in outs]
    placements = [("all at %d" % k, {n: offset(ops[n], k) for n in case.place}) for k in (1, 2, 3)]
    if len(case.place) > 1:
        placements += [("%s alone" % n, {n: offset(ops[n], 1)}) for n in case.place]
    for what, offs in placements:
        outs, t, bufs = run_placed(case, offs)
        for n, off in offs.items():
            assert t[n].data_ptr() % 16 == off * ops[n].element_size()
        check(case, what, outs, t, bufs, base)
