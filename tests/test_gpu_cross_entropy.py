"""Softmax cross-entropy (m2d_cross_entropy_fwd / _bwd, ops.cross_entropy): loss, gradient and argmax against
F.cross_entropy / torch.argmax in fp64, extreme logits, out-of-range labels, run-to-run bit equality."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WORST = {}
DEV = "cuda"


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def case(B, C, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    logits = scale * torch.randn(B, C, generator=g)
    labels = torch.randint(0, C, (B,), generator=g)
    return logits, labels


def run(logits, labels, gout=1.0):
    from music2dance_amd import ops
    x = logits.to(DEV).requires_grad_(True)
    y = labels.to(DEV)
    loss = ops.cross_entropy(x, y)
    (loss * gout).backward()
    _, pred = ops.cross_entropy_pred(x.detach(), y)
    torch.cuda.synchronize()
    return loss.detach().cpu(), x.grad.cpu(), pred.cpu()


@pytest.mark.parametrize("C", [2, 4, 10, 1000])
@pytest.mark.parametrize("B", [1, 49, 4096])
def test_matches_torch_fp64(B, C):
    logits, labels = case(B, C, seed=B * 7 + C)
    loss, grad, pred = run(logits, labels, gout=1.7)
    x = logits.double().requires_grad_(True)
    want = F.cross_entropy(x, labels)
    (want * 1.7).backward()
    err = abs(loss.item() - want.item())
    note("ce loss B%d C%d" % (B, C), err / abs(want.item()))
    assert err <= 1e-5 * abs(want.item()) + 1e-7
    gerr = (grad.double() - x.grad).abs().max().item()
    note("ce grad B%d C%d" % (B, C), gerr / x.grad.abs().max().item())
    assert gerr <= 1e-5 * x.grad.abs().max().item()
    assert torch.equal(pred, logits.argmax(1))
    assert pred.dtype == torch.int64


def test_argmax_takes_the_first_maximum():
    from music2dance_amd import ops
    logits = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0], [-1.0, -5.0, -1.0, -1.0]] + [[0.0] * 3 + [5.0]])
    logits = torch.cat([logits, torch.zeros(4, 100)], 1)  # ties across lanes of the wave too
    logits[1, 64] = 2.0
    _, pred = ops.cross_entropy_pred(logits.to(DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
    assert pred.cpu().tolist() == logits.argmax(1).tolist() == [1, 0, 4, 3]


def test_extreme_logits_stay_finite():
    logits, labels = case(49, 10, seed=3)
    logits = torch.where(torch.rand(49, 10, generator=torch.Generator().manual_seed(4)) < 0.5, 80.0, -80.0)
    loss, grad, _ = run(logits, labels)
    assert math.isfinite(loss.item()) and torch.isfinite(grad).all()
    x = logits.double().requires_grad_(True)
    want = F.cross_entropy(x, labels)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-5 * abs(want.item()) + 1e-6
    assert (grad.double() - x.grad).abs().max().item() <= 1e-5 * x.grad.abs().max().item()


@pytest.mark.parametrize("bad", [-1, 4, 1 << 40])
def test_out_of_range_label_gives_nan(bad):
    from music2dance_amd import ops
    logits, labels = case(8, 4, seed=5)
    labels[3] = bad
    loss = ops.cross_entropy(logits.to(DEV), labels.to(DEV))
    assert math.isnan(loss.item())


def test_bit_stable_across_runs():
    logits, labels = case(4096, 1000, seed=6)
    a = run(logits, labels)
    b = run(logits, labels)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_too_many_classes_raise():
    from music2dance_amd import _lib, ops
    with pytest.raises(_lib.M2dError):
        ops.cross_entropy(torch.zeros(2, 1025, device=DEV), torch.zeros(2, dtype=torch.int64, device=DEV))
