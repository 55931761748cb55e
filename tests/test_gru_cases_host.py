"""The GRU edge cases of tests/gru_cases.py on the fake backend in fp64 (no GPU): every case is well formed, its
reference is what ops.gru_stack / ops.gru_layer compute, and what test_gpu_gru_edges.py expects of padding, of dead
steps and of degenerate lengths holds for the reference arithmetic.

Bound: the 1e-12 of test_gru_host.py, relative to max |reference| - the fake backend restates nn.GRU's fp64 arithmetic
in another summation order.
"""
import pytest
import torch

from tests import gru_cases as G

BOUND = 1e-12


@pytest.fixture(autouse=True)
def fake_kernels():
    from music2dance_amd import kernels
    from tests.fake_backend import FakeKernels
    prev = kernels.set_impl(FakeKernels())
    yield
    kernels.set_impl(prev)


def K():
    from music2dance_amd import kernels
    return kernels.impl()


def same(t):
    return t


def rel(got, ref):
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not ref.any():  # dW_hh at T = 1
        assert not got.any()
        return 0.0
    return ((got - ref).abs().max() / ref.abs().max()).item()


def test_the_case_lists_are_the_ones_the_issue_names():
    shapes = lambda cases: {c[1:5] for c in cases}
    assert shapes(G.LENGTHS_CASES) == {(5, 7, 33, 2), (17, 9, 240, 3), (33, 6, 64, 1), (16, 37, 48, 3), (3, 5, 21, 4)}
    for dims in shapes(G.LENGTHS_CASES):  # each with lengths and, as its neighbour, dense
        assert sorted(c.lengths is None for c in G.LENGTHS_CASES if c[1:5] == dims) == [False, True]
    assert shapes(G.WIDE_CASES) == {(3, 5, H, L) for H in (257, 260, 272) for L in (1, 2, 3)} | {(17, 4, 260, 1)}
    assert [c[1:5] for c in G.WIDE_CASES if c.lengths] == [(3, 5, 260, 2)]
    assert shapes(G.EDGE_CASES) == {(17, 6, 256, 3), (5, 6, 256, 4), (5, 6, 252, 2), (5, 6, 250, 2), (5, 9, 16, 3),
                                    (33, 9, 12, 2), (1, 4, 240, 4)} | {(4, T, 40, 2) for T in (1, 2, 3, 4)}
    assert all(any(c[1:5] == d[1:5] and c.lengths is None for c in G.EDGE_CASES) for d in G.EDGE_CASES)  # all run dense
    assert 2 * sum(1 for c in G.EDGE_CASES if c.lengths) >= len(shapes(G.EDGE_CASES))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_case_is_well_formed(c):
    """persistent eligibility from the case's numbers, a short row in every batch tile, max |reference gradient| >= 1"""
    if c in G.PERSISTENT_CASES:
        assert c.T >= 4 and c.H <= 256 and G.persist_blocks(c) <= 192
    else:
        assert c.H > 256 or c.T < 4
    if c.lengths:
        assert len(c.lengths) == c.B and max(c.lengths) == c.T and min(c.lengths) == 1
        assert list(c.lengths) != sorted(c.lengths, reverse=True)
        for b0 in range(0, c.B, 16):
            assert min(c.lengths[b0:b0 + 16]) < c.T, b0
        if c.B == 17:
            assert c.lengths[16] < c.T
    ref = G.reference(c)
    assert ref.out.abs().max().item() <= 1.0
    for g, n in zip(ref.grads, ["x"] + G.names(c.L)):
        if c.T == 1 and n.startswith("weight_hh"):
            assert not g.any()                  # h[-1] = 0: identically zero, compared exactly
        else:
            assert g.abs().max().item() >= 1.0, n   # rel_err's floor of 1 never loosens a gradient bound
        assert torch.isfinite(g).all()


@pytest.mark.parametrize("c", G.CASES + [G.DEEP_CASE], ids=G.case_id)
def test_reference_is_what_the_ops_compute(c):
    """ops.gru_stack (L <= 4), ops.gru_layer as well (L = 1), layers.GRU's loop over ops.gru_layer (L = 5)"""
    from music2dance_amd import layers, ops
    ref = G.reference(c)
    routes = []
    if c.L <= 4:
        routes.append(lambda x, p: ops.gru_stack(x, p, ref.lengths))
    if c.L == 1:
        routes.append(lambda x, p: ops.gru_layer(x, *p, ref.lengths))
    for route in routes or [None]:
        x = ref.x.clone().requires_grad_(True)
        if route is None:
            mod = layers.GRU(G.I, c.H, c.L, batch_first=True).double()
            mod.load_state_dict(dict(zip(G.names(c.L), ref.params)))
            params = [getattr(mod, n) for n in G.names(c.L)]
            out = mod(x, lengths=ref.lengths)[0]
        else:
            params = [p.clone().requires_grad_(True) for p in ref.params]
            out = route(x, params)
        assert rel(out, ref.out) < BOUND
        got = torch.autograd.grad(out, [x] + params, ref.dout)
        for g, r, n in zip(got, ref.grads, ["x"] + G.names(c.L)):
            assert rel(g, r) < BOUND, n


WITH_LENGTHS = [c for c in G.CASES if c.lengths]


@pytest.mark.parametrize("c", WITH_LENGTHS, ids=G.case_id)
def test_dead_steps_are_exactly_zero_and_padding_is_never_read(c):
    """sections c and d of the GPU test, for the reference arithmetic"""
    ref = G.reference(c)
    zero = G.kernel_run(K(), same, ref, c.lengths, True)
    for b, n in G.dead_steps(c.lengths, c.T):
        for l in range(c.L):
            assert not zero.outs[l][b, n:].any() and not zero.dgi[l][b, n:].any() and not zero.dgh[l][b, n:].any()
        assert not zero.grads[0][b, n:].any()
    assert rel(zero.outs[-1], ref.out) < BOUND
    x, dout = G.with_garbage_padding(ref)
    assert x.abs().max() >= 1e3 and dout.isnan().any()
    dirty = G.kernel_run(K(), same, ref, c.lengths, True, x=x, dout=dout)
    assert torch.equal(dirty.outs[-1], zero.outs[-1])
    for a, b, n in zip(dirty.grads, zero.grads, ["x"] + G.names(c.L)):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("c", G.DEGENERATE_CASES, ids=G.case_id)
def test_degenerate_lengths(c):
    """section e of the GPU test: a length above T is length T; a row of length 0 leaves zeros and the parameter
    gradients of the batch without it"""
    ref = G.reference(c)
    base = G.kernel_run(K(), same, ref, c.lengths, True)
    above = G.kernel_run(K(), same, ref, [n + 3 if n == c.T else n for n in c.lengths], True)
    for a, b in zip(base.outs + base.saved + base.dgi + base.dgh + base.grads,
                    above.outs + above.saved + above.dgi + above.dgh + above.grads):
        assert torch.equal(a, b)
    row = G.EMPTY_ROW
    assert 1 < c.lengths[row] and row in ref.rows
    less = G.reference_without_row(c, row)
    for g in less.grads:
        assert g.abs().max().item() >= 1.0
    lengths = [0 if b == row else n for b, n in enumerate(c.lengths)]
    empty = G.kernel_run(K(), same, less, lengths, True)
    for l in range(c.L):
        assert not empty.outs[l][row].any() and not empty.dgi[l][row].any() and not empty.dgh[l][row].any()
    assert rel(empty.outs[-1][less.rows], less.out) < BOUND
    assert rel(empty.grads[0][less.rows], less.grads[0]) < BOUND
    for g, r, n in zip(empty.grads[1:], less.grads[1:], G.names(c.L)):
        assert rel(g, r) < BOUND, n
