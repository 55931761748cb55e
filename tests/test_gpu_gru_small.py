"""Small-state GRU (m2d_gru_small_fwd / _bwd, ops.gru_final_state): h_n, out and every gradient against
torch.nn.GRU in fp64 on the CPU, the gru_stack fallback (M2D_GRU_SMALL=0), run-to-run bit equality, the H bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu

WORST = {}
DEV = "cuda"


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def make(B, T, H, I=8, seed=0, saturate=False):
    g = torch.Generator().manual_seed(seed)
    k = 1.0 / H ** 0.5
    x = torch.randn(B, T, I, generator=g)
    w_ih = (2 * torch.rand(3 * H, I, generator=g) - 1) * k
    w_hh = (2 * torch.rand(3 * H, H, generator=g) - 1) * k
    b_ih = (2 * torch.rand(3 * H, generator=g) - 1) * k
    b_hh = (2 * torch.rand(3 * H, generator=g) - 1) * k
    if saturate:  # |gi| around 30: gates pinned at 0 / 1, tanh at +-1
        x = 10 * torch.randn(B, T, I, generator=g)
        w_ih = torch.randn(3 * H, I, generator=g) * (3.0 / I ** 0.5)
    gh = torch.randn(B, H, generator=g)
    return [x, w_ih, w_hh, b_ih, b_hh], gh


def reference(params, gh, lengths=None):
    """fp64 nn.GRU on the CPU -> (h_n, out padded with zeros, grads of x, w_ih, w_hh, b_ih, b_hh) for L = sum(h_n * gh)"""
    x, w_ih, w_hh, b_ih, b_hh = [p.double().clone().requires_grad_(True) for p in params]
    B, T, I = x.shape
    H = w_hh.shape[1]
    rnn = torch.nn.GRU(I, H, batch_first=True).double()
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(w_ih), rnn.weight_hh_l0.copy_(w_hh), rnn.bias_ih_l0.copy_(b_ih), rnn.bias_hh_l0.copy_(b_hh)
    if lengths is None:
        out, h_n = rnn(x)
    else:
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, lengths.tolist(), batch_first=True)
        out, h_n = rnn(packed)
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=T)
    h_n = h_n[0]
    (h_n * gh.double()).sum().backward()
    grads = [x.grad] + [p.grad for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)]
    return h_n.detach(), out.detach(), grads


def run(params, gh, lengths=None):
    from music2dance_amd import ops
    ps = [p.to(DEV).requires_grad_(True) for p in params]
    ln = None if lengths is None else lengths.to(DEV, torch.int32)
    h_n = ops.gru_final_state(*ps, lengths=ln)
    (h_n * gh.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return h_n.detach().cpu(), [p.grad.cpu() for p in ps]


def close(got, want, what, tol=1e-5):
    """|got - want| <= tol * (largest |want|)"""
    want = want.double()
    err = (got.double() - want).abs().max().item()
    scale = max(want.abs().max().item(), 1e-30)
    note(what, err / scale)
    assert err <= tol * scale, "%s: max err %.3e vs %.3e * %.3e" % (what, err, tol, scale)


def sorted_lengths(B, T, seed):
    g = torch.Generator().manual_seed(seed)
    ln = torch.randint(1, T + 1, (B,), generator=g)
    ln[-1] = 1  # a length-1 row
    ln[0] = T
    return ln.sort(descending=True).values


CASES = ([(49, 120, H) for H in (1, 3, 4, 8, 16)] + [(49, T, 4) for T in (1, 2, 750)] + [(B, 120, 4) for B in (1, 200)]
         + [(200, 750, 16), (1, 1, 1)])


@pytest.mark.parametrize("B,T,H", CASES)
@pytest.mark.parametrize("with_lengths", [False, True])
def test_matches_torch_gru_fp64(B, T, H, with_lengths):
    params, gh = make(B, T, H, seed=B * 1000 + T * 10 + H)
    lengths = sorted_lengths(B, T, seed=H) if with_lengths else None
    h_n, grads = run(params, gh, lengths)
    r_h, r_out, r_grads = reference(params, gh, lengths)
    tag = "gru_small B%d T%d H%d%s" % (B, T, H, " len" if with_lengths else "")
    # a SINGLE-element state (B1 H1) has no larger element to measure against: here h_n = 5e-3 = (1 - z) * n with O(1)
    # gates, so it and everything derived from it carry the gates' rounding, about 1.2e-5 of their own size (measured:
    # h_n 1.1e-5, dx 1.15e-5). That case alone is held to 3e-5; every other case to the 1e-5 bound
    tol = 3e-5 if B * H == 1 else 1e-5
    close(h_n, r_h, tag + " h_n", tol=tol)
    for name, g, r in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), grads, r_grads):
        close(g, r, tag + " " + name, tol=tol)
    # the full output sequence of the kernel (rows past a length are 0)
    from music2dance_amd import kernels
    k = kernels.impl()
    x, w_ih, w_hh, b_ih, b_hh = [p.to(DEV) for p in params]
    gi = k.gemm(0, x.reshape(B * T, -1).contiguous(), w_ih, b_ih).view(B, T, 3 * H)
    ln = None if lengths is None else lengths.to(DEV, torch.int32)
    out, h2, saved = k.gru_small_fwd(gi, w_hh, b_hh, ln, save=False, with_out=True)
    assert saved is None
    close(out.cpu(), r_out, tag + " out", tol=tol)
    torch.cuda.synchronize()
    assert torch.equal(h2.cpu(), h_n)


@pytest.mark.parametrize("H", [1, 4, 16])
def test_saturating_inputs(H):
    params, gh = make(49, 120, H, I=3, seed=7 + H, saturate=True)
    lengths = sorted_lengths(49, 120, seed=3)
    h_n, grads = run(params, gh, lengths)
    assert torch.isfinite(h_n).all() and all(torch.isfinite(g).all() for g in grads)
    r_h, _, r_grads = reference(params, gh, lengths)
    close(h_n, r_h, "gru_small saturating H%d h_n" % H)
    for name, g, r in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), grads, r_grads):
        close(g, r, "gru_small saturating H%d %s" % (H, name))


@pytest.mark.parametrize("with_lengths", [False, True])
def test_agrees_with_the_stack_fallback(monkeypatch, with_lengths):
    params, gh = make(49, 120, 4, seed=5)
    lengths = sorted_lengths(49, 120, seed=9) if with_lengths else None
    small = run(params, gh, lengths)
    monkeypatch.setenv("M2D_GRU_SMALL", "0")
    fall = run(params, gh, lengths)
    close(small[0], fall[0], "small vs stack h_n")
    for name, a, b in zip(("dx", "dw_ih", "dw_hh", "db_ih", "db_hh"), small[1], fall[1]):
        close(a, b, "small vs stack " + name)


def test_wide_states_take_the_stack_path():
    params, gh = make(8, 30, 17, seed=17)
    h_n, grads = run(params, gh)
    r_h, _, r_grads = reference(params, gh)
    close(h_n, r_h, "gru_final_state H17 h_n")
    close(grads[2], r_grads[2], "gru_final_state H17 dw_hh")


def test_two_runs_bit_equal():
    params, gh = make(200, 120, 4, seed=11)
    lengths = sorted_lengths(200, 120, seed=2)
    a = run(params, gh, lengths)
    b = run(params, gh, lengths)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1], b[1]):
        assert torch.equal(x, y)


def test_cpu_int64_lengths_are_accepted_and_raw_kernels_check_them():
    from music2dance_amd import _lib, kernels
    params, gh = make(6, 20, 4, seed=21)
    lengths = torch.tensor([20, 17, 9, 9, 3, 1])  # what pack_padded_sequence takes: CPU int64
    h_n, grads = run(params, gh, lengths.to(torch.int32))
    from music2dance_amd import ops
    ps = [p.to(DEV) for p in params]
    assert torch.equal(ops.gru_final_state(*ps, lengths=lengths).cpu(), h_n)
    assert torch.equal(ops.gru_final_state(*ps, lengths=lengths.tolist()).cpu(), h_n)
    k = kernels.impl()
    gi = torch.zeros(6, 20, 12, device=DEV)
    for bad in (lengths, lengths.to(DEV), lengths.to(torch.int32), lengths.to(DEV, torch.int32)[:5]):
        with pytest.raises(_lib.M2dError):
            k.gru_small_fwd(gi, ps[2], ps[4], bad)


def test_h_outside_bound_raises():
    from music2dance_amd import _lib, kernels
    k = kernels.impl()
    gi = torch.zeros(2, 3, 3 * 17, device=DEV)
    w_hh = torch.zeros(3 * 17, 17, device=DEV)
    b_hh = torch.zeros(3 * 17, device=DEV)
    with pytest.raises(_lib.M2dError):
        k.gru_small_fwd(gi, w_hh, b_hh)
    out = torch.zeros(2, 3, 17, device=DEV)
    saved = torch.zeros(4, 2, 3, 17, device=DEV)
    with pytest.raises(_lib.M2dError):
        k.gru_small_bwd(None, torch.zeros(2, 17, device=DEV), out, saved, w_hh)
