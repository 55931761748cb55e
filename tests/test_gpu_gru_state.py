"""GRU stack forward with a carried state (m2d_gru_stack_fwd_state): outputs and h_n against torch.nn.GRU(..., hx) in
fp64 on the CPU, in the per-step and the persistent form, with and without lengths; h0 = NULL bit-equal to
m2d_gru_stack_fwd; a sequence split in two calls chained through h_n -> h0 bit-equal to one call."""
import itertools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}


def K():
    from music2dance_amd import kernels
    return kernels.impl()


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def make(B, T, H, L, seed=0):
    """(nn.GRU in fp64 with input size H, x (B, T, H) fp64, h0 (L, B, H) fp64, kernel arguments in fp32 on the device)"""
    g = torch.Generator().manual_seed(seed)
    rnn = torch.nn.GRU(H, H, L, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.1 if p.dim() == 1 else 1.0 / math.sqrt(p.shape[1])))
    x = torch.randn(B, T, H, generator=g, dtype=torch.float64)
    h0 = 0.5 * torch.randn(L, B, H, generator=g, dtype=torch.float64)
    gi0 = (x @ rnn.weight_ih_l0.t() + rnn.bias_ih_l0).float().to(DEV)
    w_ih_t = [None] + [getattr(rnn, "weight_ih_l%d" % l).t().contiguous().float().to(DEV) for l in range(1, L)]
    b_ih = [None] + [getattr(rnn, "bias_ih_l%d" % l).float().to(DEV) for l in range(1, L)]
    w_hh_t = [getattr(rnn, "weight_hh_l%d" % l).t().contiguous().float().to(DEV) for l in range(L)]
    b_hh = [getattr(rnn, "bias_hh_l%d" % l).float().to(DEV) for l in range(L)]
    return rnn, x, h0, (gi0, w_ih_t, b_ih, w_hh_t, b_hh)


def reference(rnn, x, h0, lengths):
    with torch.no_grad():
        if lengths is None:
            return rnn(x, h0)
        packed = torch.nn.utils.rnn.pack_padded_sequence(x, lengths, batch_first=True, enforce_sorted=False)
        out, h_n = rnn(packed, h0)
        out, _ = torch.nn.utils.rnn.pad_packed_sequence(out, batch_first=True, total_length=x.shape[1])
        return out, h_n


CASES = list(itertools.product((1, 3), (10, 240), (1, 5), (1, 2, 37, 300), (False, True), (False, True)))


@pytest.mark.parametrize("L,H,B,T,with_lengths,persistent", CASES,
                         ids=lambda v: str(v))
def test_state_matches_torch_gru_with_hx(L, H, B, T, with_lengths, persistent):
    rnn, x, h0, args = make(B, T, H, L, seed=L * 1000 + H + B + T)
    lengths = None
    if with_lengths:
        lengths = [T] + [max(1, T - 3 * i - 1) for i in range(1, B)]
    ref_out, ref_hn = reference(rnn, x, h0, lengths)
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=DEV)
    outs, _, h_n = K().gru_stack_fwd(*args, lengths=lens, save=False, persistent=persistent,
                                     h0=h0.float().to(DEV), want_state=True)
    torch.cuda.synchronize()
    K().check_async_errors()
    e_out, e_hn = rel_err(outs[-1], ref_out), rel_err(h_n, ref_hn)
    WORST["gru_state out rel"] = max(WORST.get("gru_state out rel", 0.0), e_out)
    WORST["gru_state h_n rel"] = max(WORST.get("gru_state h_n rel", 0.0), e_hn)
    assert e_out < 1e-4 and e_hn < 1e-4, (e_out, e_hn)
    if with_lengths:  # rows past a sequence's length stay zero, as without a state
        for b, n in enumerate(lengths):
            assert torch.count_nonzero(outs[-1][b, n:]) == 0


@pytest.mark.parametrize("L,H,B,T,persistent", [(3, 240, 5, 37, True), (3, 240, 1, 300, True), (1, 10, 5, 2, False),
                                                (3, 240, 5, 37, False), (1, 10, 1, 300, True)],
                         ids=lambda v: str(v))
def test_null_h0_is_bit_identical_to_the_stateless_entry_point(L, H, B, T, persistent):
    _, _, _, args = make(B, T, H, L, seed=7)
    lens = torch.tensor([T] + [max(1, T - i) for i in range(1, B)], dtype=torch.int32, device=DEV)
    for lengths in (None, lens):
        ref, ref_saved = K().gru_stack_fwd(*args, lengths=lengths, save=True, persistent=persistent)
        outs, saved, h_n = K().gru_stack_fwd(*args, lengths=lengths, save=True, persistent=persistent, want_state=True)
        torch.cuda.synchronize()
        K().check_async_errors()
        for l in range(L):
            assert torch.equal(outs[l], ref[l]), l
            assert torch.equal(saved[l], ref_saved[l]), l
        last = (torch.full((B,), T, device=DEV) if lengths is None else lengths.long()) - 1
        for l in range(L):
            assert torch.equal(h_n[l], ref[l][torch.arange(B, device=DEV), last]), l


@pytest.mark.parametrize("L,H,B,T,T1", [(3, 240, 5, 37, 13), (3, 240, 1, 300, 1), (3, 240, 5, 37, 3),
                                        (1, 10, 5, 37, 20), (3, 10, 1, 300, 150), (1, 240, 5, 2, 1)],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("persistent", [False, True])
def test_split_chained_through_h_n_is_bit_identical_to_one_call(L, H, B, T, T1, persistent):
    _, _, _, args = make(B, T, H, L, seed=11)
    gi0 = args[0]
    k = K()
    one, _ = k.gru_stack_fwd(*args, save=False, persistent=persistent)
    first, _, h1 = k.gru_stack_fwd(gi0[:, :T1].contiguous(), *args[1:], save=False, persistent=persistent,
                                   want_state=True)
    second, _, _ = k.gru_stack_fwd(gi0[:, T1:].contiguous(), *args[1:], save=False, persistent=persistent, h0=h1,
                                   want_state=True)
    torch.cuda.synchronize()
    k.check_async_errors()
    for l in range(L):
        assert torch.equal(torch.cat((first[l], second[l]), 1), one[l]), l


def test_layer_forward_with_hx_in_torch_layout():
    from music2dance_amd import layers
    B, T, I, H, L = 3, 29, 17, 40, 3
    ref = torch.nn.GRU(I, H, L, batch_first=True).double()
    mine = layers.GRU(I, H, L, batch_first=True)
    mine.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    mine.to(DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, T, I, generator=g, dtype=torch.float64)
    hx = torch.randn(L, B, H, generator=g, dtype=torch.float64)
    with torch.no_grad():
        r_out, r_hn = ref(x, hx)
        out, h_n = mine(x.float().to(DEV), None, hx.float().to(DEV))
        plain = mine(x.float().to(DEV))
    assert h_n.shape == (L, B, H)
    assert rel_err(out, r_out) < 1e-5 and rel_err(h_n, r_hn) < 1e-5
    assert plain[1] is None

