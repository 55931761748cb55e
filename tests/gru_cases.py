"""GRU stack under per-sequence lengths, states wider than 256 and the edges of the persistent kernels: the case lists
and fp64 references that the GPU test (test_gpu_gru_edges.py) and the host test (test_gru_cases_host.py) share. A helper,
not a test module; it imports no GPU code, and music2dance_amd only inside the functions that run a backend.

The reference is torch.nn.GRU(I, H, L, batch_first=True) in fp64 on the CPU, over pack_padded_sequence(enforce_sorted=
False) / pad_packed_sequence(total_length=T) where a case has lengths. Weights as in test_gru_stack_fwd_bwd: normal,
1 / sqrt(fan_in) for matrices, 0.1 for biases. I = 7 throughout (the input projection is the GEMM engine's, tested
elsewhere). Every input is drawn in fp32 and widened, so the fp32 kernels and the fp64 reference start from the same
numbers.

A case is (group, B, T, H, L, lengths or None):
  lengths  ragged batches through the three backward kernels; every shape also runs dense
  wide     H > 256: the forward's gru_mac branch, the backward's K = 3H > 768, the persistent plan must decline
  edges    H = 256 / 252 / 250, L = 4, one hidden tile with several layers, T = 1..4

dout is scaled by a power of two per case until the smallest of the reference gradients has max |g| >= 1: rel_err of
test_gpu_kernels.py floors its denominator at 1, and with this the floor never loosens a gradient bound (REFERENCE
asserts it; the host test shows it for every case). The one exception is dW_hh at T = 1, which is identically 0
because h[-1] is: the tests ask for an exact 0 there.
"""
import collections
import functools
import math

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

I = 7
TILE = 16            # batch rows and hidden units of one workgroup
PERSIST_MAX_H = 256  # gru_persist_plan: H <= 256, T >= 4, at most 3/4 of the CUs (256 on the part this targets)
PERSIST_MIN_T = 4
PERSIST_MAX_BLOCKS = 192

Case = collections.namedtuple("Case", "group B T H L lengths")


def case_id(c):
    return "B%d-T%d-H%d-L%d%s" % (c.B, c.T, c.H, c.L, "-len" if c.lengths else "")


def ragged(B, T, seed):
    """B lengths in 1..T that hold T and 1, are not sorted, and leave the last row of every 16-row batch tile short
    (for B = 17 that is the lone row of the second tile)"""
    g = torch.Generator().manual_seed(seed)
    ln = torch.randint(1, T + 1, (B,), generator=g).tolist()
    ln[0], ln[1] = max(1, T // 2), T
    if B > 2:
        ln[2] = 1
    for b0 in range(0, B, TILE):
        last = min(b0 + TILE, B) - 1
        if last != 1:
            ln[last] = min(ln[last], T - 1)
    return tuple(ln)


def _both(group, B, T, H, L):
    """the shape dense and, as its neighbour, with lengths"""
    return [Case(group, B, T, H, L, None), Case(group, B, T, H, L, ragged(B, T, seed=B + T + H + L))]


LENGTHS_CASES = [c for dims in [(5, 7, 33, 2), (17, 9, 240, 3), (33, 6, 64, 1), (16, 37, 48, 3), (3, 5, 21, 4)]
                 for c in _both("lengths", *dims)]

WIDE_CASES = ([Case("wide", 3, 5, H, L, None) for H in (257, 260, 272) for L in (1, 2, 3)]
              + [Case("wide", 3, 5, 260, 2, ragged(3, 5, seed=260)), Case("wide", 17, 4, 260, 1, None)])

# half of the edge shapes also run with lengths (T = 1 leaves no room for a short row, B = 1 none for a ragged batch)
EDGE_CASES = (_both("edges", 17, 6, 256, 3) + [Case("edges", 5, 6, 256, 4, None)] + _both("edges", 5, 6, 252, 2)
              + _both("edges", 5, 6, 250, 2) + [Case("edges", 5, 9, 16, 3, None)] + _both("edges", 33, 9, 12, 2)
              + [Case("edges", 4, 1, 40, 2, None), Case("edges", 4, 2, 40, 2, None)] + _both("edges", 4, 3, 40, 2)
              + _both("edges", 4, 4, 40, 2) + [Case("edges", 1, 4, 240, 4, None)])

CASES = LENGTHS_CASES + WIDE_CASES + EDGE_CASES

# more than GRU_MAX_LAYERS layers: layers.GRU runs them one by one through ops.gru_layer (the per-step layer kernels)
DEEP_CASE = Case("deep", 3, 5, 21, 5, ragged(3, 5, seed=21))

# degenerate lengths (above T, and 0 for row EMPTY_ROW, whose own length is T // 2 >= 2): one case per recurrence form
DEGENERATE_CASES = [c for c in CASES if c.lengths and c[1:5] in ((5, 7, 33, 2), (3, 5, 260, 2))]
EMPTY_ROW = 0

# the cases that are there to run the step form: states too wide for the persistent kernels, sequences too short
STEP_ONLY = [c for c in CASES if c.group == "wide" or c.T < PERSIST_MIN_T]
PERSISTENT_CASES = [c for c in CASES if c not in STEP_ONLY]


def persist_blocks(c):
    return math.ceil(c.H / TILE) * math.ceil(c.B / TILE) * c.L


def persistent_eligible(c):
    """gru_persist_plan restated for a 256-CU part"""
    return c.T >= PERSIST_MIN_T and c.H <= PERSIST_MAX_H and persist_blocks(c) <= PERSIST_MAX_BLOCKS


def short_row_in_every_tile(c):
    return all(min(c.lengths[b0:b0 + TILE]) < c.T for b0 in range(0, c.B, TILE))


# without these a case would quietly test the step form twice, or the persistent form where the step form is meant
assert all(persistent_eligible(c) for c in PERSISTENT_CASES), [case_id(c) for c in PERSISTENT_CASES if not persistent_eligible(c)]
assert not any(persistent_eligible(c) for c in STEP_ONLY)
assert all(c.H > PERSIST_MAX_H for c in WIDE_CASES)
for _c in CASES:
    if _c.lengths:
        assert len(_c.lengths) == _c.B and max(_c.lengths) == _c.T and min(_c.lengths) == 1, case_id(_c)
        assert list(_c.lengths) != sorted(_c.lengths, reverse=True), case_id(_c)
        assert short_row_in_every_tile(_c), case_id(_c)
assert len({case_id(c) for c in CASES}) == len(CASES)
assert 2 * sum(1 for c in EDGE_CASES if c.lengths) >= len({c[:5] for c in EDGE_CASES})


def names(L):
    return [n % l for l in range(L) for n in ("weight_ih_l%d", "weight_hh_l%d", "bias_ih_l%d", "bias_hh_l%d")]


# params: the 4L parameters in names(L) order; x, dout: the whole batch (B rows); rows: the rows the reference ran on (all
# of them, but for without_row); lengths: those rows' lengths or None; out and grads[0] (dx) have len(rows) rows;
# grads = [dx] + the 4L parameter gradients of <out, dout[rows]>. All fp64 on the CPU, never written to.
Reference = collections.namedtuple("Reference", "case params x dout rows lengths out grads")


def _gen(*shape, g):
    return torch.randn(*shape, generator=g, dtype=torch.float32).double()


def build_reference(B, T, H, L, lengths, seed, drop=None, case=None):
    g = torch.Generator().manual_seed(seed)
    rnn = torch.nn.GRU(I, H, L, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_((torch.randn(p.shape, generator=g) * (0.1 if p.dim() == 1 else 1.0 / math.sqrt(p.shape[1]))).double())
    x, dout = _gen(B, T, I, g=g), _gen(B, T, H, g=g)
    rows = [b for b in range(B) if b != drop]
    lens = None if lengths is None else [lengths[b] for b in rows]
    xr = x[rows].clone().requires_grad_(True)
    if lens is None:
        out, _ = rnn(xr)
    else:
        out, _ = rnn(pack_padded_sequence(xr, lens, batch_first=True, enforce_sorted=False))
        out, _ = pad_packed_sequence(out, batch_first=True, total_length=T)
    wrt = [xr] + [getattr(rnn, n) for n in names(L)]
    grads = torch.autograd.grad(out, wrt, dout[rows])
    # gradients are linear in dout: one power of two lifts the smallest of them to max |g| >= 1
    # (at T = 1 every dW_hh is identically 0, h[-1] being 0: nothing lifts it, and the tests ask for an exact 0 there)
    tops = [gr.abs().max().item() for gr in grads]
    assert all(top > 0 or (T == 1 and n.startswith("weight_hh")) for top, n in zip(tops, ["x"] + names(L)))
    scale = 2.0 ** max(0, math.ceil(-math.log2(min(top for top in tops if top > 0))))
    grads = [gr * scale for gr in grads]
    assert all(gr.abs().max().item() >= 1.0 or not gr.any() for gr in grads)
    params = [getattr(rnn, n).detach() for n in names(L)]
    return Reference(case, params, x, dout * scale, rows, lens, out.detach(), grads)


@functools.lru_cache(maxsize=None)
def reference(c):
    return build_reference(c.B, c.T, c.H, c.L, c.lengths, seed=1000 * c.H + 10 * c.B + c.L, case=c)


@functools.lru_cache(maxsize=None)
def reference_without_row(c, row):
    """the same draw as reference(c), nn.GRU run on the batch without `row`: what a row of length 0 must leave"""
    return build_reference(c.B, c.T, c.H, c.L, c.lengths, seed=1000 * c.H + 10 * c.B + c.L, drop=row, case=c)


def lengths_tensor(lengths, like):
    """as ops._gru_lengths hands them to the kernels: int32 on the device of `like`"""
    return None if lengths is None else torch.tensor(list(lengths), dtype=torch.int32, device=like.device)


def with_garbage_padding(ref):
    """(x, dout) of a case with lengths, everything past a length replaced: x by finite garbage of magnitude ~1e3, dout
    by NaN. The packed reference never reads either."""
    c = ref.case
    g = torch.Generator().manual_seed(5)
    x, dout = ref.x.clone(), ref.dout.clone()
    for b, n in enumerate(c.lengths):
        x[b, n:] = 1e3 * (1.0 + torch.rand(c.T - n, I, generator=g)) * (1 - 2 * torch.randint(0, 2, (c.T - n, I), generator=g))
        dout[b, n:] = float("nan")
    return x, dout


Run = collections.namedtuple("Run", "outs saved dgi dgh grads")


def kernel_run(k, to, ref, lengths, persistent, x=None, dout=None, h0=None):
    """The stack at the kernel level, as ops._GRUStack runs it: layer 0's projection, k.gru_stack_fwd, k.gru_stack_bwd,
    then the engine GEMMs and channel sums of ops._gru_layer_grads. `to`: a CPU fp64 tensor on the backend's device in its
    dtype; lengths: a sequence or None (any integers: nothing here refuses 0 or more than T).
    -> Run(outs, saved, dgi, dgh of all layers, [dx] + the 4L parameter gradients)"""
    from music2dance_amd import ops
    c = ref.case
    x = to(ref.x if x is None else x)
    dout = to(ref.dout if dout is None else dout)
    p = [to(t) for t in ref.params]
    w_ih, w_hh, b_ih, b_hh = (p[i::4] for i in range(4))
    lens = lengths_tensor(lengths, x)
    gi0 = k.gemm(0, x.view(c.B * c.T, I), w_ih[0], b_ih[0]).view(c.B, c.T, 3 * c.H)
    outs, saved = k.gru_stack_fwd(gi0, [None] + [w.t().contiguous() for w in w_ih[1:]], [None] + b_ih[1:],
                                  [w.t().contiguous() for w in w_hh], b_hh, lens, True, persistent=persistent)
    dgi, dgh = k.gru_stack_bwd(dout, outs, saved, w_hh, [None] + w_ih[1:], lens, persistent=persistent)
    layers = [ops._gru_layer_grads(x if l == 0 else outs[l - 1], w_ih[l], outs[l], dgi[l], dgh[l], l == 0)
              for l in range(c.L)]
    return Run(outs, saved, dgi, dgh, [layers[0][0]] + [g for layer in layers for g in layer[1:]])


def dead_steps(lengths, T):
    """[(b, first dead step)] of the rows that end before T"""
    return [(b, max(0, n)) for b, n in enumerate(lengths) if n < T]
