"""Non-finite values through the fused epilogues of the HIP kernels: every case of
tests/nonfinite_cases.py through kernels.impl(), exactly as test_gpu_kernels.py calls the kernels. Each case plants one
NaN / +inf / -inf in seeded operands and compares with plain fp64 torch CPU ops: the output's NaN set equals the
reference's (none swallowed, none leaked outside the receptive field), the infinite elements are equal, the finite rest
is within the tolerance of the corresponding parity test. The table names, per case, the source site it reaches.

The split-K cases run in both forms of test_split_k_in_one_launch_equals_the_two_launch_form: with the stream's ticket
scratch registered (the epilogue runs in the tile's last arriver) and without it (m2d_splitk_reduce_kernel applies it)."""
import contextlib

import pytest
import torch

from tests import nonfinite_cases as nf

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def K():
    from music2dance_amd import kernels
    return kernels.impl()


def _run(case):
    for label, got, ref, tol in case.run(K(), lambda t: t.to(DEV)):
        try:
            nf.check(got, ref, tol)
        except AssertionError as e:
            raise AssertionError("%s (%s): %s" % (label, case.site, e)) from None


@contextlib.contextmanager
def two_launch_split_k():
    """unregister the stream's ticket scratch (a split-K plan then runs as GEMM + m2d_splitk_reduce_kernel), register it again"""
    from music2dance_amd import _lib, kernels
    stream = kernels._stream(torch.device(DEV))  # registers the scratch
    t = kernels._STREAM_SCRATCH[(torch.device(DEV).index, stream)]
    _lib.check(_lib.lib().m2d_stream_scratch_set(stream, 0, 0), "m2d_stream_scratch_set")
    try:
        yield
        torch.cuda.synchronize()
    finally:
        _lib.check(_lib.lib().m2d_stream_scratch_set(stream, t.data_ptr(), t.numel() * 4), "m2d_stream_scratch_set")


@pytest.mark.parametrize("case", nf.CASES, ids=lambda c: c.id)
def test_non_finite_values_pass_through(case):
    _run(case)


@pytest.mark.parametrize("case", [c for c in nf.CASES if c.split_k], ids=lambda c: c.id)
def test_non_finite_values_pass_through_the_split_k_reduce_kernel(case):
    with two_launch_split_k():
        _run(case)
