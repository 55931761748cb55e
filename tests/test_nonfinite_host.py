"""The non-finite case table (tests/nonfinite_cases.py) against the CPU stand-in for the kernel layer
(tests/fake_backend.py): every case's reference has a non-finite and a finite part (check() asserts it), and the stand-in,
which restates each entry point's contract in torch ops, meets every check. So the expectations hold without the kernels,
and the stand-in keeps the NaN / inf behaviour the product has. No GPU needed."""
import pytest
import torch

from tests import nonfinite_cases as nf
from tests.fake_backend import FakeKernels


@pytest.mark.parametrize("case", nf.CASES, ids=lambda c: c.id)
def test_the_stand_in_backend_meets_every_case(case):
    for label, got, ref, tol in case.run(FakeKernels(), lambda t: t.clone()):
        try:
            nf.check(got, ref, tol)
        except AssertionError as e:
            raise AssertionError("%s (%s): %s" % (label, case.site, e)) from None


def test_the_checker_catches_a_swallowed_and_a_leaked_nan_and_a_wrong_infinity():
    ref = torch.tensor([1.0, float("nan"), float("-inf"), 2.0], dtype=torch.float64)
    nf.check(ref.float(), ref, 1e-6)
    for bad in ([1.0, 0.0, float("-inf"), 2.0],              # NaN swallowed
                [float("nan"), float("nan"), float("-inf"), 2.0],   # NaN leaked
                [1.0, float("nan"), 0.0, 2.0],                # -inf flattened
                [1.0, float("nan"), float("inf"), 2.0],       # wrong sign
                [1.0, float("nan"), float("-inf"), 2.1]):     # finite part off
        with pytest.raises(AssertionError):
            nf.check(torch.tensor(bad), ref, 1e-6)
    with pytest.raises(AssertionError, match="vacuous"):
        nf.check(torch.ones(3), torch.ones(3, dtype=torch.float64), 1e-6)
    with pytest.raises(AssertionError, match="vacuous"):
        nf.check(torch.full((3,), float("nan")), torch.full((3,), float("nan"), dtype=torch.float64), 1e-6)


def test_every_poison_and_position_of_the_contract_is_in_the_table():
    ids = [c.id for c in nf.CASES]
    for word in ("-nan-", "-pinf-", "-ninf-", "x_first", "x_last", "x_pad", "-w", "-b", "mask", "two_out", "stats", "res-act"):
        assert any(word in i for i in ids), word
    assert not any("mask" in i and ("pinf" in i or "ninf" in i) for i in ids)   # under a mask: NaN only
