"""GRU stack kernels where the dense tests do not reach (cases and references: tests/gru_cases.py): backward through
time under per-sequence lengths, states wider than 256 (the forward's gru_mac branch, K = 3H > 768 in the backward), the
edges of the register-resident persistent kernels (H = 256 / 252 / 250, L = 4, one hidden tile under several layers,
T = 1..4), each in the persistent form (the defaults) and as step launches.

Reference: torch.nn.GRU in fp64 on the CPU. Bounds: those of test_gru_stack_fwd_bwd, with rel_err of test_gpu_kernels.py
- out < 1e-5 (absolute: |out| <= 1), every gradient < 3e-5 of its largest element (every reference gradient has
max |g| >= 1, so the floor of rel_err's denominator is never in use; an identically zero one, dW_hh at T = 1, is
compared exactly). Carried state: the measure and the 1e-4 of test_gpu_gru_state.py. Everything else here is exact.

Which test reaches what:
  m2d_gru_bwd_step_kernel       a / c / d at the L = 1 cases with lengths (ops.gru_layer, k.gru_layer_bwd), a's 5-layer case
  m2d_gru_stack_bwd_kernel      a / c / d / e in the step form, b's reference side; every wide and T < 4 case in any form
  m2d_gru_persist_bwd_kernel    a / c / d / e in the default form, b's persistent side
  m2d_gru_stack_fwd_kernel, H > 256   every wide case of a - f
"""
import pytest
import torch

from tests import gru_cases as G
from tests.test_gpu_gru_state import reference as state_reference
from tests.test_gpu_gru_state import rel_err as state_err
from tests.test_gpu_kernels import DEV, K, rel_err

pytestmark = pytest.mark.gpu

WORST = {}
FORMS = ["default", "step"]
WITH_LENGTHS = [c for c in G.CASES if c.lengths]


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def to(t):
    return t.float().to(DEV)


def select(monkeypatch, form):
    """the recurrence form of ops.gru_stack, through the switches the product has"""
    from music2dance_amd.kernels import HipKernels
    if form == "step":
        monkeypatch.setenv("M2D_GRU_BWD_PERSIST", "0")
        monkeypatch.setattr(HipKernels, "persistent_gru", False)
    else:
        monkeypatch.delenv("M2D_GRU_BWD_PERSIST", raising=False)
        assert HipKernels.persistent_gru is True  # (False after a recovered time-out: the case would run the step form twice)


def settled():
    """a persistent launch that gave up leaves invalid outputs: look before comparing anything"""
    torch.cuda.synchronize()
    K().check_async_errors()


def compare(tag, out, grads, ref):
    e = rel_err(out, ref.out)
    note("gru_edges %s: out (bound 1e-5)" % tag, e)
    assert e < 1e-5, e
    for g, r, n in zip(grads, ref.grads, ["x"] + G.names(ref.case.L)):
        if not r.any():
            assert not g.any(), n
            continue
        e = rel_err(g, r)
        note("gru_edges %s: gradients (bound 3e-5)" % tag, e)
        assert e < 3e-5, (n, e)


def autograd_run(route, ref, x=None, dout=None):
    """-> (out, [dx] + the parameter gradients) of route(x, params, lengths) on the device"""
    x = to(ref.x if x is None else x).requires_grad_(True)
    params = [to(p).requires_grad_(True) for p in ref.params]
    out = route(x, params, G.lengths_tensor(ref.lengths, x))
    grads = torch.autograd.grad(out, [x] + params, to(ref.dout if dout is None else dout))
    settled()
    return out.detach(), grads


def routes(c):
    from music2dance_amd import ops
    found = [("stack", lambda x, p, n: ops.gru_stack(x, p, n))]
    if c.L == 1:  # the per-step layer kernels, which layers.GRU runs for stacks of more than 4 layers
        found.append(("layer", lambda x, p, n: ops.gru_layer(x, *p, n)))
    return found


# ------------------------------------------------------------------ a. output and every gradient against fp64
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_output_and_every_gradient_against_fp64(c, form, monkeypatch):
    select(monkeypatch, form)
    ref = G.reference(c)
    for _, route in routes(c):
        out, grads = autograd_run(route, ref)
        compare("%s, %s form" % (c.group, form), out, grads, ref)


def test_five_layers_with_lengths_against_fp64():
    """layers.GRU(7, 21, 5): more than GRU_MAX_LAYERS, so layer by layer through ops.gru_layer"""
    from music2dance_amd import layers
    c = G.DEEP_CASE
    ref = G.reference(c)
    mod = layers.GRU(G.I, c.H, c.L, batch_first=True)
    mod.load_state_dict({n: p.float() for n, p in zip(G.names(c.L), ref.params)})
    mod.to(DEV)
    x = to(ref.x).requires_grad_(True)
    out, none = mod(x, lengths=list(c.lengths))
    assert none is None
    grads = torch.autograd.grad(out, [x] + [getattr(mod, n) for n in G.names(c.L)], to(ref.dout))
    compare("five layers with lengths, layer kernels", out.detach(), grads, ref)


# ------------------------------------------------------------------ b. kernel-level form equality
@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_persistent_request_is_bit_identical_to_the_step_launches(c):
    """outs, saved gates, dgi and dgh of all layers. Where the library declines the persistent form (H > 256, T < 4) the
    request must come back right from the step launches, with no error word raised."""
    k = K()
    assert k.persistent_gru is True
    ref = G.reference(c)
    step = G.kernel_run(k, to, ref, c.lengths, False)
    pers = G.kernel_run(k, to, ref, c.lengths, True)
    settled()
    for what in ("outs", "saved", "dgi", "dgh"):
        for l, (a, b) in enumerate(zip(getattr(step, what), getattr(pers, what))):
            assert torch.equal(a, b), (what, l)
    e = rel_err(pers.outs[-1], ref.out)  # (equal to each other and wrong together is a's business; out costs nothing here)
    assert e < 1e-5, e


# ------------------------------------------------------------------ c. structure under lengths
@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("c", WITH_LENGTHS, ids=G.case_id)
def test_dead_steps_are_exactly_zero(c, persistent):
    """for every row b and every t >= lengths[b]: out, dgi and dgh of every layer, and dx. No tolerance."""
    k = K()
    ref = G.reference(c)
    run = G.kernel_run(k, to, ref, c.lengths, persistent)
    settled()
    dead = (torch.arange(c.T)[None, :] >= torch.tensor(c.lengths)[:, None]).to(DEV)
    assert dead.any()
    for l in range(c.L):
        for what, t in (("out", run.outs[l]), ("dgi", run.dgi[l]), ("dgh", run.dgh[l])):
            assert not t[dead].any(), (what, l)
    assert not run.grads[0][dead].any()
    if c.L == 1 and persistent:  # the per-step layer kernels
        x, (w_ih, w_hh, b_ih, b_hh) = to(ref.x), [to(p) for p in ref.params]
        lens = G.lengths_tensor(c.lengths, x)
        gi = k.gemm(0, x.view(c.B * c.T, G.I), w_ih, b_ih).view(c.B, c.T, 3 * c.H)
        out, saved = k.gru_layer_fwd(gi, w_hh.t().contiguous(), b_hh, lens)
        dgi, dgh = k.gru_layer_bwd(to(ref.dout), out, saved, w_hh, lens)
        torch.cuda.synchronize()
        for what, t in (("out", out), ("dgi", dgi), ("dgh", dgh)):
            assert not t[dead].any(), ("layer kernels", what)


# ------------------------------------------------------------------ d. padding is never read
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("c", WITH_LENGTHS, ids=G.case_id)
def test_padding_is_never_read(c, form, monkeypatch):
    """x past each length filled with finite garbage of magnitude ~1e3, dout past each length with NaN: out, dx and all
    4L parameter gradients equal the run with zero padding bit for bit - the reference's packed path never touches
    padding. Non-finite values in the padding of x are out of scope: the weight-gradient GEMM multiplies the (zero)
    gate gradients of dead steps by the layer's input, 0 x NaN is NaN by construction, and the project's collate pads
    with zeros."""
    select(monkeypatch, form)
    ref = G.reference(c)
    x, dout = G.with_garbage_padding(ref)
    for name, route in routes(c):
        clean_out, clean = autograd_run(route, ref)
        out, grads = autograd_run(route, ref, x=x, dout=dout)
        assert torch.equal(out, clean_out), name
        for g, r, n in zip(grads, clean, ["x"] + G.names(c.L)):
            assert torch.equal(g, r), (name, n)


# ------------------------------------------------------------------ e. degenerate lengths
@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "step"])
@pytest.mark.parametrize("c", G.DEGENERATE_CASES, ids=G.case_id)
def test_degenerate_lengths(c, persistent):
    """kernel level (torch refuses both): a length above T is length T, word for word; a row of length 0 gives exact
    zeros in out, dgi and dgh, and the parameter gradients of the batch without that row (bounds of a)"""
    k = K()
    ref = G.reference(c)
    base = G.kernel_run(k, to, ref, c.lengths, persistent)
    above = G.kernel_run(k, to, ref, [n + 3 if n == c.T else n for n in c.lengths], persistent)
    settled()
    for a, b in zip(base.outs + base.saved + base.dgi + base.dgh + base.grads,
                    above.outs + above.saved + above.dgi + above.dgh + above.grads):
        assert torch.equal(a, b)
    row = G.EMPTY_ROW
    less = G.reference_without_row(c, row)
    empty = G.kernel_run(k, to, less, [0 if b == row else n for b, n in enumerate(c.lengths)], persistent)
    settled()
    for l in range(c.L):
        for what, t in (("out", empty.outs[l]), ("dgi", empty.dgi[l]), ("dgh", empty.dgh[l])):
            assert not t[row].any(), (what, l)
    assert not empty.grads[0][row].any()
    compare("a row of length 0, %s" % ("persistent" if persistent and c.H <= 256 else "step"),
            empty.outs[-1][less.rows], [empty.grads[0][less.rows]] + empty.grads[1:], less)


# ------------------------------------------------------------------ f. carried state on the wide path
@pytest.mark.parametrize("c", [c for c in G.WIDE_CASES if c[1:5] == (3, 5, 260, 2)], ids=G.case_id)
def test_carried_state_on_the_wide_path(c):
    ref = G.reference(c)
    rnn = torch.nn.GRU(G.I, c.H, c.L, batch_first=True).double()
    rnn.load_state_dict(dict(zip(G.names(c.L), ref.params)))
    h0 = 0.5 * torch.randn(c.L, c.B, c.H, generator=torch.Generator().manual_seed(9)).double()
    want_out, want_hn = state_reference(rnn, ref.x, h0, None if c.lengths is None else list(c.lengths))
    k = K()
    x, p = to(ref.x), [to(t) for t in ref.params]
    w_ih, w_hh, b_ih, b_hh = (p[i::4] for i in range(4))
    gi0 = k.gemm(0, x.view(c.B * c.T, G.I), w_ih[0], b_ih[0]).view(c.B, c.T, 3 * c.H)
    outs, _, h_n = k.gru_stack_fwd(gi0, [None] + [w.t().contiguous() for w in w_ih[1:]], [None] + b_ih[1:],
                                   [w.t().contiguous() for w in w_hh], b_hh, G.lengths_tensor(c.lengths, x), save=False,
                                   h0=to(h0), want_state=True)
    settled()
    e_out, e_hn = state_err(outs[-1], want_out), state_err(h_n, want_hn)
    note("gru_edges wide carried state: out (bound 1e-4)", e_out)
    note("gru_edges wide carried state: h_n (bound 1e-4)", e_hn)
    assert e_out < 1e-4 and e_hn < 1e-4, (e_out, e_hn)
