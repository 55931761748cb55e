"""The label-conditioning and dropout kernels (m2d_label_concat, m2d_pose_pack3_label, m2d_label_embed_bwd,
m2d_dropout) on the MI355X against fp64 torch."""
import pytest
import torch

from music2dance_amd import kernels, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASES = {"mixed": [2, 0, 3, 1, 2, 2], "all-equal": [1, 1, 1, 1], "absent": [0, 3, 3, 0, 3], "B=1": [2]}


def K():
    return kernels.impl()


def _emb64(E, labels):
    return E.double()[labels]


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("layout", [0, 1])
def test_concat_and_embedding_gradient(case, layout):
    g = torch.Generator().manual_seed(3)
    labels = torch.tensor(CASES[case])
    B, T, C, L, D = labels.numel(), 120, 69, 4, 4
    E = torch.randn(L, D, generator=g)
    x = torch.randn((B, T, C) if layout == 0 else (B, C, T), generator=g)
    y = K().label_concat(x.to(DEV), E.to(DEV), labels.to(DEV), layout)
    e = _emb64(E, labels)
    want = torch.cat((x.double(), e[:, None].expand(-1, T, -1)), 2) if layout == 0 else \
        torch.cat((x.double(), e[:, :, None].expand(-1, -1, T)), 1)
    assert torch.equal(y.cpu().double(), want)
    dy = torch.randn(y.shape, generator=g)
    dE = K().label_embed_bwd(dy.to(DEV), labels.to(DEV), 0, B, C, L, D, layout)
    ref = torch.zeros(L, D, dtype=torch.float64)
    part = dy.double()[:, :, C:].sum(1) if layout == 0 else dy.double()[:, C:].sum(2)
    ref.index_add_(0, labels, part)
    torch.testing.assert_close(dE.cpu().double(), ref, rtol=0, atol=1e-5)
    if case == "absent":
        assert torch.equal(dE[1:3].cpu(), torch.zeros(2, D))
    again = [K().label_embed_bwd(dy.to(DEV), labels.to(DEV), 0, B, C, L, D, layout) for _ in range(3)]
    assert all(torch.equal(a, dE) for a in again)


def test_embedding_gradient_over_a_row_range():
    g = torch.Generator().manual_seed(4)
    B, T, C = 3, 120, 69
    dx = torch.randn(3 * B, C + 4, T, generator=g)
    lbl = torch.tensor([0, 2, 2, 3, 1, 0])
    dE = K().label_embed_bwd(dx.to(DEV), lbl.to(DEV), B, 3 * B, C, 4, 4, 1)
    ref = torch.zeros(4, 4, dtype=torch.float64).index_add_(0, lbl, dx.double()[B:, C:].sum(2))
    torch.testing.assert_close(dE.cpu().double(), ref, rtol=0, atol=1e-5)


def test_out_of_range_label_gives_nan_and_no_fault():
    B, T, C = 3, 120, 69
    E = torch.randn(4, 4, device=DEV)
    x = torch.randn(B, T, C, device=DEV)
    for bad in (4, -1, 1 << 40):
        labels = torch.tensor([1, bad, 2], device=DEV)
        y = K().label_concat(x, E, labels, 0)
        assert torch.isnan(y[1, :, C:]).all() and not torch.isnan(y[[0, 2]]).any() and torch.equal(y[1, :, :C], x[1])
        dE = K().label_embed_bwd(y, labels, 0, B, C, 4, 4, 0)
        assert torch.isnan(dE).all()
    torch.cuda.synchronize()


def test_pose_pack3_label_matches_torch():
    g = torch.Generator().manual_seed(5)
    B, T, C = 3, 120, 69
    real, fake = torch.rand(B, T, C, generator=g), torch.rand(B * T, C, generator=g)
    alpha = torch.rand(B, generator=g)
    E = torch.randn(4, 4, generator=g)
    rl, fl = torch.tensor([0, 3, 1]), torch.tensor([2, 2, 0])
    X = K().pose_pack3_label(real.to(DEV), fake.to(DEV), alpha.to(DEV), E.to(DEV), rl.to(DEV), fl.to(DEV)).cpu()
    base = K().pose_pack3(real.to(DEV), fake.to(DEV), alpha.to(DEV)).cpu()
    assert torch.equal(X[:, :C], base)
    lbl = torch.cat((rl, rl, fl))
    assert torch.equal(X[:, C:], E[lbl][:, :, None].expand(-1, -1, T))


def test_dropout_given_mask_is_exact():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(32, 128, 120, generator=g)
    m = (torch.rand(x.shape, generator=g) < 0.5).to(torch.uint8)
    y = K().dropout(x.to(DEV), m.to(DEV)).cpu()
    assert torch.equal(y, x * m.float() * 2)


def test_dropout_philox_bits():
    n = 4 * 1024 * 1024 + 3
    x = torch.randn(n, device=DEV)
    m1 = torch.empty(n, dtype=torch.uint8, device=DEV)
    m2 = torch.empty_like(m1)
    m3 = torch.empty_like(m1)
    y = K().dropout(x, m1, seed=1234, offset=7)
    K().dropout(None, m2, seed=1234, offset=7)
    K().dropout(None, m3, seed=1234, offset=8)
    assert torch.equal(m1, m2) and not torch.equal(m1, m3)
    keep = float(m1.float().mean())
    assert abs(keep - 0.5) <= 0.002, keep
    assert 0.49 < float((m1 == m3).float().mean()) < 0.51
    assert torch.equal(y, x * m1.float() * 2)
    # forward and backward use the same bits (the autograd op keeps the mask)
    xr = torch.randn(64, 256, device=DEV, requires_grad=True)
    out, mask = ops.dropout(xr, 0.5, host=False)
    gy = torch.randn_like(out)
    gx, = torch.autograd.grad(out, xr, gy)
    assert torch.equal(gx, gy * mask.float() * 2) and torch.equal(out, xr.detach() * mask.float() * 2)
