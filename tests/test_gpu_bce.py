"""m2d_bce_logits_fwd / _bwd and ops.bce_with_logits on the MI355X against torch's BCEWithLogitsLoss in fp64: one and
two segments, constant targets 0, 1 and 0.3, ordinary and +-1e4 logits; NaN propagation, argument errors and run-to-run
bit stability."""
import pytest
import torch
import torch.nn.functional as F

from music2dance_amd import _lib, kernels, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _logits(n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    if scale == "1e4":
        x = 1e4 * torch.where(x < 0, -1.0, 1.0)
    else:
        x = scale * x
    return x.to(DEV)


def _ref(x, n0, t0, n1, t1):
    xd = x.detach().double().cpu().requires_grad_(True)
    m0 = F.binary_cross_entropy_with_logits(xd[:n0], torch.full((n0,), t0, dtype=torch.float64))
    m1 = (F.binary_cross_entropy_with_logits(xd[n0:], torch.full((n1,), t1, dtype=torch.float64)) if n1
          else xd.new_zeros(()))
    (m0 + m1).backward()
    return torch.stack((m0 + m1, m0, m1)).detach(), xd.grad


def _rel_close(got, want, rtol=1e-6):
    got = got.double().cpu()
    assert torch.all((got - want).abs() <= rtol * want.abs() + 1e-30), (got, want)


CASES = [(n0, n1, t, scale) for n0 in (1, 24, 4096) for n1 in (0, n0) for t in (0.0, 1.0, 0.3) for scale in (3.0, "1e4")]


@pytest.mark.parametrize("n0,n1,t,scale", CASES)
def test_fwd_bwd_against_fp64_torch(n0, n1, t, scale):
    k = kernels.impl()
    t1 = 0.3 if t != 0.3 else 1.0
    x = _logits(n0 + n1, scale, seed=n0 + 7 * n1 + int(10 * t))
    want, gwant = _ref(x, n0, t, n1, t1)
    out, dx = k.bce_logits_fwd(x, n0, t, n1, t1, with_dx=True)
    assert torch.isfinite(out).all() and torch.isfinite(dx).all()
    _rel_close(out, want)
    gmax = float(gwant.abs().max())
    assert float((dx.double().cpu() - gwant).abs().max()) <= 1e-6 * gmax + 1e-30
    gout = torch.tensor(2.5, device=DEV)
    dx2 = k.bce_logits_bwd(x, n0, t, n1, t1, gout)
    assert float((dx2.double().cpu() - 2.5 * gwant).abs().max()) <= 2.5e-6 * gmax + 1e-30
    out_only, none = k.bce_logits_fwd(x, n0, t, n1, t1)
    assert none is None and torch.equal(out_only, out)


@pytest.mark.parametrize("n", [1, 24, 4096])
@pytest.mark.parametrize("t", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("scale", [3.0, "1e4"])
def test_autograd_op_against_fp64_torch(n, t, scale):
    x = _logits(n, scale, seed=100 + n).view(n // 2 if n > 1 else 1, -1).requires_grad_(True)
    loss = ops.bce_with_logits(x, t)
    assert loss.dim() == 0
    (gx,) = torch.autograd.grad(3.0 * loss, x)
    xd = x.detach().double().cpu().requires_grad_(True)
    want = F.binary_cross_entropy_with_logits(xd, torch.full_like(xd, t))
    (gwant,) = torch.autograd.grad(3.0 * want, xd)
    _rel_close(loss.detach().view(1), want.detach().view(1))
    assert gx.shape == x.shape
    assert float((gx.double().cpu() - gwant).abs().max()) <= 1e-6 * float(gwant.abs().max()) + 1e-30


def test_nan_propagates():
    k = kernels.impl()
    x = _logits(48, 3.0, seed=5)
    x[30] = float("nan")
    out, dx = k.bce_logits_fwd(x, 24, 1.0, 24, 0.0, with_dx=True)
    assert torch.isnan(out[0]) and torch.isnan(out[2]) and torch.isfinite(out[1])
    assert torch.isnan(dx[30]) and torch.isfinite(dx[:30]).all() and torch.isfinite(dx[31:]).all()
    dx2 = k.bce_logits_bwd(x, 24, 1.0, 24, 0.0, torch.ones((), device=DEV))
    assert torch.isnan(dx2[30]) and torch.isfinite(dx2[:30]).all()
    xl = x.clone().requires_grad_(True)
    loss = ops.bce_with_logits(xl, 0.0)
    (g,) = torch.autograd.grad(loss, xl)
    assert torch.isnan(loss) and torch.isnan(g[30])


def test_bad_segment_sizes_raise():
    k = kernels.impl()
    x = _logits(8, 3.0, seed=6)
    with pytest.raises(_lib.M2dError):
        k.bce_logits_fwd(x, 0, 1.0, 8, 0.0)
    with pytest.raises(_lib.M2dError):
        k.bce_logits_fwd(x, 9, 1.0, -1, 0.0)
    with pytest.raises(_lib.M2dError):
        k.bce_logits_bwd(x, 0, 1.0, 8, 0.0, torch.ones((), device=DEV))
    with pytest.raises(_lib.M2dError):
        k.bce_logits_fwd(x, 4, 1.0, 3, 0.0)   # 7 logits announced, 8 given


def test_two_runs_are_bit_equal():
    k = kernels.impl()
    x = _logits(4096 + 4096, 3.0, seed=9)
    a = k.bce_logits_fwd(x, 4096, 1.0, 4096, 0.0, with_dx=True)
    b = k.bce_logits_fwd(x, 4096, 1.0, 4096, 0.0, with_dx=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
