"""Host half of the operand-placement tests (tests/placement_cases.py; the device half is tests/test_gpu_operand_placement.py):
the placement helper yields every residue it is asked for, the guard check sees a write on either side of an operand,
every case's fp64 reference agrees with the CPU stand-in of the kernel layer within the case's own bound, and every
public entry point of kernels.HipKernels that takes a tensor has a case or a stated reason for having none."""
import inspect

import pytest
import torch

from music2dance_amd import kernels
from tests import placement_cases as P
from tests.knn_cases import NumpyKnnBackend
from tests.ops_cases import OpsFakeKernels
from tests.sync_cases import NumpySyncBackend

CPU = torch.device("cpu")


@pytest.mark.parametrize("dtype,offs", [(torch.float32, range(4)), (torch.uint8, range(16)), (torch.int64, range(2)),
                                        (torch.float64, range(2))], ids=str)
def test_place_yields_every_residue(dtype, offs):
    t = (torch.arange(3 * 5 * 7) % 100).to(dtype).view(3, 5, 7)
    for off in offs:
        view, buf = P.place(t, off, CPU)
        assert view.data_ptr() % 16 == off * t.element_size() and view.is_contiguous() and view.shape == t.shape
        assert torch.equal(view, t) and buf.numel() == 2 * P.GUARD + 16 // t.element_size() + t.numel()
        assert view.data_ptr() - buf.data_ptr() == (P.GUARD + off) * t.element_size()
        assert P.guards_intact(buf, view)
    with pytest.raises(AssertionError):
        P.place(t, 16 // t.element_size(), CPU)


@pytest.mark.parametrize("where", [-1, 0, "first guard element", "last guard element"])
def test_guards_catch_a_write_beside_the_output(where):
    """a Python stand-in for a kernel that stores one element before / after its output (nothing is launched)"""
    out, buf = P.place(torch.zeros(4, 6), 1, CPU)
    start = P.GUARD + 1

    def op(dst, stray):
        dst.copy_(torch.ones(4, 6))
        if stray is not None:
            buf[stray] = 1.0
    op(out, None)
    assert P.guards_intact(buf, out) and bool((out == 1).all())
    stray = {-1: start - 1, 0: start + out.numel(), "first guard element": 0, "last guard element": buf.numel() - 1}[where]
    op(out, stray)
    assert not P.guards_intact(buf, out)
    buf[stray] = float("nan")    # a NaN is no sentinel either
    assert not P.guards_intact(buf, out)


def test_case_names_are_unique_and_every_case_places_something():
    names = [c.name for c in P.CASES]
    assert len(set(names)) == len(names)
    for c in P.CASES:
        assert c.place, c.name
        assert all(v.device == CPU for v in c.operands().values())


class StandIn(OpsFakeKernels, NumpySyncBackend, NumpyKnnBackend):
    """every CPU stand-in of the kernel layer the suite has: fake_backend.FakeKernels and the label / dropout / BCE /
    cross-entropy entries in torch ops, the metric kernels through their fp64 numpy statements"""
    name = "fake-cpu"


STOOD_IN = [c for c in P.CASES if not c.hip_only and all(hasattr(StandIn, op) for op in c.ops)]


@pytest.mark.parametrize("case", STOOD_IN, ids=lambda c: c.name)
def test_reference_agrees_with_the_cpu_stand_in(case):
    """proves the references and the shapes without a device: the stand-in restates each entry point's contract in fp32
    torch ops (tests/fake_backend.py and the host tests of the later features)"""
    fake = StandIn()
    t = {k: v.clone() for k, v in case.operands().items()}
    got = case.run(fake, t)
    ref = case.reference()
    assert len(got) == len(ref)
    for i, (g, r, tol) in enumerate(zip(got, ref, case.tols(len(ref)))):
        if r is None:
            continue
        ok, fig = P.within(g, r, tol)
        assert ok, (case.name, i, fig, tol)
    for name, v in case.operands().items():
        if name not in case.written:
            assert torch.equal(t[name], v), (case.name, name)


def test_the_stand_in_covers_all_but_the_entry_points_that_need_the_library():
    assert {c.name for c in P.CASES} - {c.name for c in STOOD_IN} == {
        "dropout seeded", "randn_frames", "adam_multi weight with live packed images", "resample_poly", "render_sticks"}


# public methods of HipKernels that take no tensor
NO_TENSOR = {"weight_cache", "check_async_errors", "fault_word", "raise_async_fault", "recover_async_fault", "prof_begin",
             "prof_dump", "prof_end", "knn_max_k", "sym_eig_max_dim", "sync_scan_max_frames"}


def test_every_tensor_entry_point_has_a_case_or_a_reason():
    """a kernel entry point added later fails here until it gets a case (or a line in EXEMPT saying why it needs none)"""
    public = {n for n, f in inspect.getmembers(kernels.HipKernels, callable) if not n.startswith("_")}
    covered = {op for c in P.CASES for op in c.ops}
    assert covered <= public, covered - public
    assert set(P.EXEMPT) <= public and NO_TENSOR <= public
    assert not (covered & set(P.EXEMPT)) and not (covered & NO_TENSOR) and not (set(P.EXEMPT) & NO_TENSOR)
    missing = public - covered - set(P.EXEMPT) - NO_TENSOR
    assert not missing, "no placement case and no exemption: %s" % sorted(missing)
    assert all(isinstance(r, str) and len(r) > 10 for r in P.EXEMPT.values())


def test_the_k4_entry_refuses_misaligned_operands_before_any_launch():
    """m2d_conv1d_fwd_k4 IS the kernel that stages x and its weight image by 16-byte LDS-DMA (include/m2d.h): a pointer off
    16 bytes comes back as M2D_ERR_ARG. The addresses are never dereferenced - the refusal is made on the host - so this
    runs without a device; aligned pointers are not tried here (that call would launch)."""
    from music2dance_amd import _lib
    h = _lib.lib()
    Cin, L, Cout, ks, s, p = 16, 512, 64, 25, 4, 11     # k4pair.a
    assert h.m2d_conv1d_k4_applicable(Cin, L, Cout, ks, s, p) == 1
    base = 0x100000
    for x, w in ((base + 4, base), (base + 8, base), (base + 12, base), (base, base + 4)):
        rc = h.m2d_conv1d_fwd_k4(x, w, None, base, None, 1, Cin, L, Cout, ks, s, p, 0, 0.0, None, None, 0.0, None, None, 0, None)
        assert rc == -1 and b"16-byte aligned" in h.m2d_last_error(), (x - base, w - base, rc)
