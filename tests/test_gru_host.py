"""Host path of the GRU family above the kernel layer, on the fake backend in fp64 (no GPU): the autograd glue of
ops.gru_stack / gru_layer / gru_final_state, the carried state, the lengths normaliser, and the kernel wrappers'
lengths check.

Reference: torch.nn.GRU in fp64 (pack_padded_sequence with lengths). Bound: 1e-12 relative to max |reference| - the
fake backend restates the same fp64 arithmetic in another summation order (measured: <= 6.3e-16), so three orders of
magnitude are left for that order.
"""
import functools

import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

B, T, I, H = 3, 5, 6, 5
LENGTHS = [5, 3, 1]
BOUND = 1e-12


@pytest.fixture(autouse=True)
def fake_kernels():
    from music2dance_amd import kernels
    from tests.fake_backend import FakeKernels
    prev = kernels.set_impl(FakeKernels())
    yield
    kernels.set_impl(prev)


def gen(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rel(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return ((got - ref).abs().max() / ref.abs().max()).item()


def names(L):
    return [n % l for l in range(L) for n in ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")]


@functools.lru_cache(maxsize=None)
def reference(L, hidden, with_lengths, with_hx):
    """nn.GRU in fp64 -> (rnn, x, hx, dout, dh_n, out, h_n, gradients of <out, dout> wrt x and the 4L parameters,
    gradients of <h_n[-1], dh_n> wrt the same); computed once per case and never written to"""
    torch.manual_seed(100 * L + hidden)
    rnn = torch.nn.GRU(I, hidden, L, batch_first=True).double()
    x = gen(B, T, I, seed=1).requires_grad_(True)
    hx = gen(L, B, hidden, seed=2) if with_hx else None
    dout, dh_n = gen(B, T, hidden, seed=3), gen(B, hidden, seed=4)
    if with_lengths:
        out, h_n = rnn(pack_padded_sequence(x, LENGTHS, batch_first=True), hx)
        out = pad_packed_sequence(out, batch_first=True, total_length=T)[0]
    else:
        out, h_n = rnn(x, hx)
    wrt = [x] + [getattr(rnn, n) for n in names(L)]
    g_out = torch.autograd.grad(out, wrt, dout, retain_graph=True)
    g_hn = torch.autograd.grad(h_n[-1], wrt, dh_n, allow_unused=True)
    return rnn, x.detach(), hx, dout, dh_n, out.detach(), h_n.detach(), g_out, g_hn


def leaves(rnn, L):
    return [getattr(rnn, n).detach().clone().requires_grad_(True) for n in names(L)]


@pytest.mark.parametrize("with_lengths", [False, True], ids=["dense", "lengths"])
@pytest.mark.parametrize("L", [1, 3, 5])
def test_output_and_every_gradient_against_nn_gru(L, with_lengths):
    """L = 1, 3: ops.gru_stack; L = 5: layers.GRU, which runs stacks of more than 4 layers through ops.gru_layer"""
    from music2dance_amd import layers, ops
    rnn, x, _, dout, _, ref, _, gref, _ = reference(L, H, with_lengths, False)
    lengths = LENGTHS if with_lengths else None
    xg = x.clone().requires_grad_(True)
    if L <= 4:
        params = leaves(rnn, L)
        out = ops.gru_stack(xg, params, lengths)
    else:
        mod = layers.GRU(I, H, L, batch_first=True).double()
        mod.load_state_dict(rnn.state_dict())
        params = [getattr(mod, n) for n in names(L)]
        out, none = mod(xg, lengths=lengths)
        assert none is None
    assert rel(out, ref) < BOUND
    got = torch.autograd.grad(out, [xg] + params, dout)
    for g, r, n in zip(got, gref, ["x"] + names(L)):
        assert rel(g, r) < BOUND, n


@pytest.mark.parametrize("with_lengths", [False, True], ids=["dense", "lengths"])
@pytest.mark.parametrize("L", [1, 3])
def test_carried_state_against_nn_gru(L, with_lengths):
    from music2dance_amd import ops
    rnn, x, hx, _, _, ref, ref_hn, _, _ = reference(L, H, with_lengths, True)
    params = [p.detach() for p in leaves(rnn, L)]
    with torch.no_grad():
        out, h_n = ops.gru_stack(x, params, LENGTHS if with_lengths else None, hx=hx, return_state=True)
        only_out = ops.gru_stack(x, params, LENGTHS if with_lengths else None, hx=hx)
    assert rel(out, ref) < BOUND
    assert rel(h_n, ref_hn) < BOUND
    assert torch.equal(only_out, out)


def test_a_sequence_in_two_chunks_chained_through_the_state_equals_one_call():
    from music2dance_amd import ops
    L = 3
    rnn, x, hx, _, _, _, _, _, _ = reference(L, H, False, True)
    params = [p.detach() for p in leaves(rnn, L)]
    with torch.no_grad():
        out, h_n = ops.gru_stack(x, params, hx=hx, return_state=True)
        out_a, h_a = ops.gru_stack(x[:, :2], params, hx=hx, return_state=True)
        out_b, h_b = ops.gru_stack(x[:, 2:], params, hx=h_a, return_state=True)
    assert torch.equal(torch.cat((out_a, out_b), 1), out)
    assert torch.equal(h_b, h_n)


@pytest.mark.parametrize("with_lengths", [False, True], ids=["dense", "lengths"])
@pytest.mark.parametrize("hidden", [4, 17], ids=["small-kernels", "stack-fallback"])
def test_final_state_against_nn_gru(hidden, with_lengths):
    from music2dance_amd import ops
    rnn, x, _, _, dh_n, _, ref_hn, _, gref = reference(1, hidden, with_lengths, False)
    forms = [None]
    if with_lengths:
        forms = [torch.tensor(LENGTHS, dtype=torch.int32), list(LENGTHS), torch.tensor(LENGTHS, dtype=torch.int64)]
    results = []
    for lengths in forms:
        xg = x.clone().requires_grad_(True)
        params = leaves(rnn, 1)
        h_n = ops.gru_final_state(xg, *params, lengths=lengths)
        results.append((h_n.detach(),) + torch.autograd.grad(h_n, [xg] + params, dh_n))
    assert rel(results[0][0], ref_hn[-1]) < BOUND
    for g, r, n in zip(results[0][1:], gref, ["x"] + names(1)):
        assert rel(g, r) < BOUND, n
    for other in results[1:]:  # an int32 tensor, a list and the CPU int64 tensor of pack_padded_sequence: one result
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)


def test_lengths_normaliser():
    from music2dance_amd import ops
    x = torch.zeros(B, T, I)
    ready = torch.tensor(LENGTHS, dtype=torch.int32)
    assert ops._gru_lengths(ready, x, "t") is ready          # already in the kernels' form: no copy
    assert ops._gru_lengths(None, x, "t") is None
    for form in (list(LENGTHS), torch.tensor(LENGTHS), torch.tensor([9] + LENGTHS, dtype=torch.int32)[1:]):
        got = ops._gru_lengths(form, x, "t")
        assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == LENGTHS
    for op in (lambda n: ops.gru_stack(x, [], n), lambda n: ops.gru_layer(x, None, None, None, None, n),
               lambda n: ops.gru_final_state(x, None, torch.zeros(12, 4), None, None, n)):
        with pytest.raises(ValueError, match="4 lengths for a batch of 3"):
            op([5, 3, 1, 1])


class _DeviceTensor:
    """what _chk_lengths looks at, of a tensor on a device this machine need not have"""

    def __init__(self, n, dtype=torch.int32, device=torch.device("cuda", 0), contiguous=True):
        self.n, self.dtype, self.device, self.contiguous, self.is_cuda = n, dtype, device, contiguous, True

    def numel(self):
        return self.n

    def is_contiguous(self):
        return self.contiguous


def test_the_kernel_wrappers_lengths_check_is_strict():
    from music2dance_amd._lib import M2dError
    from music2dance_amd.kernels import HipKernels
    dev = torch.device("cuda", 0)
    chk = HipKernels._chk_lengths
    assert chk(None, dev, B) is None
    assert chk(_DeviceTensor(B), dev, B) is None
    with pytest.raises(M2dError, match="contiguous int32 tensor on cuda:0"):   # a host address must never reach a kernel
        chk(torch.tensor(LENGTHS, dtype=torch.int32), dev, B)
    with pytest.raises(M2dError, match="contiguous int32 tensor on cuda:0"):
        chk(torch.tensor(LENGTHS, dtype=torch.int64), dev, B)
    for bad in (_DeviceTensor(B, dtype=torch.int64), _DeviceTensor(B, device=torch.device("cuda", 1)),
                _DeviceTensor(B, contiguous=False)):
        with pytest.raises(M2dError, match="contiguous int32 tensor on cuda:0"):
            chk(bad, dev, B)
    with pytest.raises(M2dError, match="4 entries for a batch of 3"):
        chk(_DeviceTensor(B + 1), dev, B)
