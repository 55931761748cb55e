"""Every autograd Function of music2dance_amd/ops.py against an fp64 twin in plain torch ops, element by element, at
first and second order: which mask, slope and operand each Function hands to which kernel in its backward and in its
double backward. Two legs: "cpu-fake" pins the autograd wiring on the CPU stand-in, "hip" pins the same wiring on the
kernels and on the routes the library picks by shape (engine, k4, thin, TemporalBlock, sub-pixel forms), driven with the
operands a gradient-penalty pass really produces. The GRU Functions are compared with fp64 torch through ops by
tests/test_gru_host.py and tests/test_gpu_gru_edges.py.

Forms (tests/ops_cases.py): the PENALTY form for everything twice differentiable (the layer under test is never the
last parametrised layer: with a constant layer behind it autograd never asks for the d/d gy branch of the second
order), the WEIGHT-SIDE form (a graph through the weight and bias gradients: _Conv1dBwdWeight.backward,
_LinearBwdWeight.backward, _ChannelSum.backward) and the FIRST-ORDER form for the once-differentiable Functions.

Error: max|got - ref64| / max|ref64| per tensor, no floor under the denominator. Bounds, all the project's own:
  2e-5  a contraction's value and the gradients one kernel away      (test_gpu_kernels.py, test_ops_premask.py)
  3e-5  weight / bias / table gradients                               (the same files)
  1e-6  ops without a contraction                                     (test_gpu_pointwise_gaps.py)
  1e-5 / 2e-5  BatchNorm forward / backward                           (test_gpu_kernels.py::test_bn_train_fwd_bwd)
First-order error bounds add along a path: a chain of n contraction layers is held to n times the single bound (BatchNorm
behind a conv: the sum of the two). Every case asserts its kink guard on the twin first, then that its own activation
signs equal the twin's: the comparison allows no flipped ReLU."""
import pytest
import torch
import torch.nn.functional as F

from music2dance_amd import kernels, ops
from tests import ops_cases as C
from tests.ops_cases import Build, TOL_PARAM, TOL_PATH, TOL_POINT, compare, kink_guard, same_signs

WORST = {}
_TWINS = {}   # one fp64 reference per case, shared by the legs (and by the flag variants of one chain), never changed


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))
    return val


@pytest.fixture(params=[pytest.param("cpu-fake"), pytest.param("hip", marks=pytest.mark.gpu)])
def dev(request):
    if request.param == "hip":
        yield torch.device("cuda:0")
    else:
        prev = kernels.set_impl(C.OpsFakeKernels())
        try:
            yield torch.device("cpu")
        finally:
            kernels.set_impl(prev)


def _leg(dev):
    return "hip" if dev.type == "cuda" else "cpu-fake"


def _twin(key, run):
    """(twin build, its result) of case `key`, computed once; the guard is asserted on every use"""
    if key not in _TWINS:
        b = Build(torch.device("cpu"), True)
        _TWINS[key] = (b, run(b))
    kink_guard(_TWINS[key][0])
    return _TWINS[key]


def _check(dev, key, run, bounds_of, twin_key=None):
    twin, ref = _twin(twin_key or key, run)
    b = Build(dev, False)
    got = run(b)
    same_signs(b, twin)
    compare(got, ref, bounds_of(ref), note, "ops %s [%s]" % (key, _leg(dev)))
    return got, ref


def _penalty(dev, key, case, twin_key=None):
    params = {"d/d" + n for n in case["names"]}
    return _check(dev, key, lambda b: C.penalty_form(b, case["net"], case["x"], case["P"], case["names"], case["c"]),
                  lambda ref: C.path_bounds(ref, case["n"], params), twin_key)


# ------------------------------------------------------------------------------------------------ conv1d, by route
@pytest.mark.parametrize("case_id", C.conv_case_ids())
def test_conv1d_penalty_form(dev, case_id):
    case = C.conv_case(case_id)
    _, _, (B, Cin, L, Cout, k, s, p), k4, thin, _ = case["row"]
    assert kernels.HipKernels._thin(Cin, Cout, k, s) == thin
    if dev.type == "cuda":
        from music2dance_amd import _lib
        assert bool(_lib.lib().m2d_conv1d_k4_applicable(Cin, L, Cout, k, s, p)) == k4
    _penalty(dev, "conv " + case_id, case)


def test_thin_predicate_agrees_with_the_library():
    """csrc/conv1d_thin.hip thin_ok: Cin == 1 && ks == 25 && stride == 4 && Cout == 32"""
    t = kernels.HipKernels._thin
    assert t(1, 32, 25, 4)
    assert not t(1, 8, 25, 4) and not t(1, 64, 25, 4) and not t(2, 32, 25, 4) and not t(1, 32, 24, 4) and not t(1, 32, 25, 2)


@pytest.mark.gpu
def test_thin_layer_still_refuses_an_output_mask():
    """the real thin layer (1 -> 32, k25, s4) has no out_mask / residual epilogue in its backward-data kernel: refused in
    Python; its 8-channel sibling is the engine's and takes one (test_conv1d_penalty_form[thin-sibling-cout8-*-flags])"""
    from music2dance_amd import _lib
    d = torch.device("cuda:0")
    dy, w, m = torch.randn(2, 32, 64, device=d), torch.randn(32, 1, 25, device=d), torch.randn(2, 1, 256, device=d)
    with pytest.raises(_lib.M2dError, match="thin"):
        kernels.impl().conv1d_bwd_data(dy, w, 256, 4, 11, out_mask=m)
    with pytest.raises(_lib.M2dError, match="thin"):
        kernels.impl().conv1d_bwd_data(dy, w, 256, 4, 11, residual=m)


def _weight_side(dev, key, case):
    g = torch.Generator().manual_seed(5)
    c1, c2 = C.draw(g, *case["P"][0].shape), C.draw(g, *case["P"][1].shape)
    params = {"gw", "gb", "d/dW", "d/dW2"}
    return _check(dev, key, lambda b: C.weight_side_form(b, case["net"], case["x"], case["P"], case["names"], case["c"], c1, c2),
                  lambda ref: C.path_bounds(ref, case["n"], params))


@pytest.mark.parametrize("case_id", ["engine-packed-ragged-leaky", "engine-unpacked-relu"])
def test_conv1d_weight_side_form(dev, case_id):
    """a graph through dW and db: _Conv1dBwdWeight.backward with its g_b branch (bwd_data with the cotangent in the weight
    slot, conv1d_fwd of x with the cotangent as weight). dW does not depend on W: no gradient there."""
    _, ref = _weight_side(dev, "conv weight-side " + case_id, C.conv_case(case_id))
    assert ref["d/dx"].any() and ref["d/dW2"].any() and not ref["d/dW"].any()


LINEAR_SEEDS = {"id": 0, "relu": 0, "leaky": 0}


@pytest.mark.parametrize("act", ["leaky", "relu"])
def test_linear_weight_side_form(dev, act):
    """_LinearBwdWeight.backward, and _ChannelSum.backward under a mask (the bias gradient's second order)"""
    _, ref = _weight_side(dev, "linear weight-side " + act, C.linear_case((7, 33, 20), act, True, LINEAR_SEEDS[act]))
    assert ref["d/dx"].any() and ref["d/dW2"].any() and not ref["d/dW"].any()


# ------------------------------------------------------------------------------------------------ linear, tanh, ...
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["id", "relu", "leaky"])
@pytest.mark.parametrize("shape", [(7, 33, 20), (2, 5, 33, 20)], ids=["2d", "3d"])
def test_linear_penalty_form(dev, shape, act, bias):
    _penalty(dev, "linear %s %s %s" % ("x".join(map(str, shape)), act, "bias" if bias else "nobias"),
             C.linear_case(shape, act, bias, LINEAR_SEEDS[act]))


def test_tanh_penalty_form(dev):
    _penalty(dev, "tanh between linears", C.tanh_case(0))


@pytest.mark.parametrize("p", [0.5, 0.3])
def test_dropout_penalty_form(dev, p):
    _penalty(dev, "dropout p=%.1f" % p, C.dropout_case(p, 0))


@pytest.mark.parametrize("layout", [0, 1])
def test_label_concat_penalty_form(dev, layout):
    """the table gradient gE of a label that occurs twice, with its first-order part (the 0.1 mean(y^2) term) and its
    second-order part (the penalty, through the tanh behind the layer); and no gE under input_grads_only"""
    case = C.label_case(layout, 0)
    _penalty(dev, "label_concat layout %d" % layout, case)
    b = Build(dev, False)
    x, P = b.leaf(case["x"]), [b.leaf(p, p.is_floating_point()) for p in case["P"]]
    y = case["net"](b, x, P)
    with ops.input_grads_only():
        gs = C.grad(y.sum(), [x] + P[:5], allow_unused=True)
    assert gs[0] is not None and all(g is None for g in gs[1:])


def test_pointwise_ops_first_order(dev):
    """tanh, dropout and label_concat alone, value and gradient at the bound of an op without a contraction"""
    g = torch.Generator().manual_seed(0)
    x = C.draw(g, 7, 33, scale=1.5)
    keep = (torch.rand(7, 33, generator=g) >= 0.3).to(torch.uint8)
    x3, E, labels = C.draw(g, 4, 6, 5), C.draw(g, 3, 3), torch.tensor(C.LABELS)
    forms = {
        "tanh": (lambda b, x: b.tanh(x), [x], ["x"]),
        "dropout": (lambda b, x, keep: b.dropout(x, keep, 0.3), [x, keep], ["x", None]),
        "label_concat 0": (lambda b, x, E, l: b.label_concat(x, E, l, 0), [x3, E, labels], ["x", "E", None]),
        "label_concat 1": (lambda b, x, E, l: b.label_concat(x, E, l, 1), [x3, E, labels], ["x", "E", None]),
    }
    for name, (fn, inputs, names) in forms.items():
        _check(dev, "first-order " + name, lambda b: C.first_order_form(b, fn, inputs, names),
               lambda ref: {n: TOL_POINT for n in ref})


CRITIC_SEED = 0


@pytest.mark.parametrize("flags", [False, True], ids=["masked-operands", "premask-flags"])
def test_critic_shaped_chain(dev, flags):
    """both runs against the one twin (the flags change where a mask is applied, not what is computed)"""
    _penalty(dev, "critic chain " + ("flags" if flags else "plain"), C.critic_case(flags, CRITIC_SEED), twin_key="critic chain")


def test_input_grads_only_and_no_input_grad_for(dev):
    case = C.critic_case(False, CRITIC_SEED)
    b = Build(dev, False)

    def graph():
        x, P = b.leaf(case["x"]), [b.leaf(p, p.is_floating_point()) for p in case["P"]]
        return x, P[:9], (case["net"](b, x, P) * b.leaf(case["c"], False)).sum()

    x, P, s = graph()
    plain = C.grad(s, [x] + P)
    x, P, s = graph()
    with ops.input_grads_only():
        only = C.grad(s, [x] + P, allow_unused=True)
    assert torch.equal(only[0], plain[0]), "gx under input_grads_only differs from the plain gx"
    assert all(g is None for g in only[1:]), "a parameter received a gradient under input_grads_only"
    # two inputs through one conv and one linear layer each: the named input alone goes without its gradient
    g = torch.Generator().manual_seed(2)
    xs = [b.leaf(C.draw(g, 2, 3, 9)) for _ in range(2)] + [b.leaf(C.draw(g, 4, 6)) for _ in range(2)]
    w, wl = b.leaf(C.draw(g, 5, 3, 3)), b.leaf(C.draw(g, 5, 6))

    def total():
        return (ops.conv1d(xs[0], w, None, 1, 1, ops.ACT_RELU) + ops.conv1d(xs[1], w, None, 1, 1, ops.ACT_RELU)).sum() + \
            (ops.linear(xs[2], wl, None, ops.ACT_LEAKY, 0.2) * ops.linear(xs[3], wl)).sum()

    plain = C.grad(total(), xs + [w, wl])
    for dead in (0, 2):
        s = total()
        with ops.no_input_grad_for(xs[dead]):
            got = C.grad(s, xs + [w, wl], allow_unused=True)
        for i, (a, ref) in enumerate(zip(got, plain)):
            if i == dead:
                assert a is None, "input %d still received its gradient" % i
            else:
                assert a is not None and torch.equal(a, ref), "gradient %d changed under no_input_grad_for(input %d)" % (i, dead)


# ------------------------------------------------------------------------------------------------ conv1d_windows
WINDOW_CASES = {"engine": ((2, 5, 37, 101, 8, 5, 2, 1), "relu", 1), "thin": ((2, 3, 64, 256, 32, 25, 4, 0), "leaky", 0)}


@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_conv1d_windows_first_order(dev, name):
    (B, T, hop, window, Cout, k, s, p), act_name, seed = WINDOW_CASES[name]
    act, slope = C.ACTS[act_name]
    g = torch.Generator().manual_seed(seed)
    track = C.draw(g, B, (T - 1) * hop + window)
    w, bias = C.draw(g, Cout, 1, k, scale=k ** -0.5), C.draw(g, Cout, scale=0.3)

    def fn(b, track, w, bias):
        if b.twin:   # a conv on the materialised slices
            x = track.unfold(-1, window, hop)[:, :T].reshape(-1, 1, window)
            return b.conv(x, w, bias, s, p, act, slope)
        return b._seen(ops.conv1d_windows(track, T, hop, window, w, bias, s, p, act, slope), act)

    _check(dev, "conv1d_windows " + name, lambda b: C.first_order_form(b, fn, [track, w, bias], [None, "W", "b"]),
           lambda ref: {"y": TOL_PATH, "d/dW": TOL_PARAM, "d/db": TOL_PARAM})
    with pytest.raises(NotImplementedError):
        ops.conv1d_windows(track.to(dev).requires_grad_(True), T, hop, window, w.to(dev), bias.to(dev), s, p)


# ------------------------------------------------------------------------------------------------ batch norm
BN_EPS, BN_MOM = 1e-5, 0.1
BN_CASES = {   # shape, act, slope, residual, seed
    "3d id": ((6, 8, 12), 0, 0.0, False, 0), "3d relu": ((6, 8, 12), 1, 0.0, False, 0), "3d leaky": ((6, 8, 12), 2, 0.2, False, 0),
    "3d relu residual": ((6, 8, 12), 1, 0.0, True, 0), "2d leaky": ((9, 8), 2, 0.2, False, 0), "2d id residual": ((9, 8), 0, 0.0, True, 0),
}


def _bn(b, x, gamma, beta, res, rm, rv, training, act, slope, sums=None):
    """-> y; rm / rv (fp32 CPU) are cloned into the build and left, updated, in b.buffers"""
    rm, rv = b.leaf(rm, False), b.leaf(rv, False)
    b.buffers = (rm, rv)
    if b.twin:
        z = F.batch_norm(x, rm, rv, gamma, beta, training, BN_MOM, BN_EPS)
        y = b._act_twin(z, act, slope)
        return y if res is None else y + res
    y = ops.batch_norm(x, gamma, beta, rm, rv, training, BN_EPS, BN_MOM, act, slope, residual=res, sums=sums)
    b._seen(y if res is None else y - res, act)
    return y


def _bn_inputs(shape, residual, seed):
    g = torch.Generator().manual_seed(seed)
    Cn = shape[1]
    per_channel = (1, Cn) + (1,) * (len(shape) - 2)   # channels of unlike spread and offset
    x = C.draw(g, *shape) * (0.5 + torch.rand(Cn, generator=g)).view(per_channel) + C.draw(g, Cn).view(per_channel)
    gamma, beta = 0.5 + torch.rand(Cn, generator=g), C.draw(g, Cn, scale=0.3)
    res = C.draw(g, *shape) if residual else None
    rm, rv = C.draw(g, Cn, scale=0.2), 0.5 + torch.rand(Cn, generator=g)
    return x, gamma, beta, res, rm, rv


@pytest.mark.parametrize("name", list(BN_CASES))
def test_batch_norm_training_first_order(dev, name):
    shape, act, slope, residual, seed = BN_CASES[name]
    x, gamma, beta, res, rm, rv = _bn_inputs(shape, residual, seed)

    def run(b):
        def fn(b, x, gamma, beta, *r):
            return _bn(b, x, gamma, beta, r[0] if r else None, rm, rv, True, act, slope)
        out = C.first_order_form(b, fn, [x, gamma, beta] + ([res] if residual else []), ["x", "gamma", "beta"] + (["residual"] if residual else []))
        out["running_mean"], out["running_var"] = b.buffers
        return out

    _, ref = _check(dev, "batch_norm " + name, run,
                    lambda ref: {n: (C.TOL_BN_BWD if n.startswith("d/d") else C.TOL_BN_FWD) for n in ref})
    if residual:
        assert ref["d/dresidual"].any()


BN_SUMS_SEED = 0


def test_batch_norm_with_sums_from_the_conv(dev):
    """conv1d(with_stats=True) -> batch_norm(sums=...) against conv -> batch_norm; bounds add: conv 2e-5 (3e-5 for its
    weight) + BatchNorm 1e-5 forward / 2e-5 backward; gamma / beta see the conv's 2e-5 in their input. The conv has no
    bias: BatchNorm removes it, its gradient is zero up to rounding and has no scale to compare against."""
    g = torch.Generator().manual_seed(BN_SUMS_SEED)
    x, w = C.draw(g, 4, 5, 20), C.draw(g, 8, 5, 3, scale=15 ** -0.5)
    gamma, beta = 0.5 + torch.rand(8, generator=g), C.draw(g, 8, scale=0.3)
    rm, rv = torch.zeros(8), torch.ones(8)

    def fn(b, x, w, gamma, beta):
        if b.twin:
            return _bn(b, F.conv1d(x, w, None, stride=2, padding=1), gamma, beta, None, rm, rv, True, 2, 0.2)
        h, sums = ops.conv1d(x, w, None, 2, 1, with_stats=True)
        return _bn(b, h, gamma, beta, None, rm, rv, True, 2, 0.2, sums=sums)

    def run(b):
        out = C.first_order_form(b, fn, [x, w, gamma, beta], ["x", "W", "gamma", "beta"])
        out["running_mean"], out["running_var"] = b.buffers
        return out

    fwd = TOL_PATH + C.TOL_BN_FWD
    _check(dev, "batch_norm sums from conv", run,
           lambda ref: {"y": fwd, "running_mean": fwd, "running_var": fwd, "d/dx": TOL_PATH + C.TOL_BN_BWD,
                        "d/dW": TOL_PARAM + C.TOL_BN_BWD, "d/dgamma": TOL_PATH + C.TOL_BN_BWD, "d/dbeta": TOL_PATH + C.TOL_BN_BWD})



@pytest.mark.parametrize("shape", [(6, 8, 12), (9, 8)], ids=["3d", "2d"])
def test_batch_norm_eval_forward_and_no_eval_backward(dev, shape):
    x, gamma, beta, res, rm, rv = _bn_inputs(shape, True, 3)

    def run(b):
        y = _bn(b, b.leaf(x, False), b.leaf(gamma, False), b.leaf(beta, False), b.leaf(res, False), rm, rv, False, 0, 0.0)
        return {"y": y, "running_mean": b.buffers[0], "running_var": b.buffers[1]}

    got, _ = _check(dev, "batch_norm eval %dd" % len(shape), run, lambda ref: {n: C.TOL_BN_FWD for n in ref})
    assert torch.equal(got["running_mean"].cpu(), rm) and torch.equal(got["running_var"].cpu(), rv)
    b = Build(dev, False)
    y = _bn(b, b.leaf(x), b.leaf(gamma), b.leaf(beta), None, rm, rv, False, 0, 0.0)
    with pytest.raises(NotImplementedError):
        y.sum().backward()


# ------------------------------------------------------------------------------------------------ once-differentiable ops
def _point(dev, key, fn, inputs, names):
    return _check(dev, key, lambda b: C.first_order_form(b, fn, inputs, names), lambda ref: {n: TOL_POINT for n in ref})


@pytest.mark.parametrize("L", [9, 10], ids=["odd", "even"])
def test_maxpool2_first_order(dev, L):
    x = C.draw(torch.Generator().manual_seed(0), 2, 3, L)

    def fn(b, x):
        if not b.twin:
            return ops.maxpool2(x)
        n = L // 2
        b.gaps.append((x[:, :, 0:2 * n:2] - x[:, :, 1:2 * n:2]).detach())
        return F.max_pool1d(x, 2, 2)

    _point(dev, "maxpool2 L=%d" % L, fn, [x], ["x"])


def test_upsample2_linear_first_order(dev):
    x = C.draw(torch.Generator().manual_seed(0), 2, 3, 7)
    _point(dev, "upsample2_linear", lambda b, x: F.interpolate(x, scale_factor=2, mode="linear", align_corners=False)
           if b.twin else ops.upsample2_linear(x), [x], ["x"])


def test_l1_mean_first_order(dev):
    g = torch.Generator().manual_seed(0)
    a, bb = C.draw(g, 3, 5, 7), C.draw(g, 3, 5, 7)

    def fn(b, a, bb):
        if not b.twin:
            return ops.l1_mean(a, bb)
        b.gaps.append((a - bb).detach())
        return (a - bb).abs().mean()

    _, ref = _point(dev, "l1_mean", fn, [a, bb], ["a", "b"])
    assert torch.equal(ref["d/da"], -ref["d/db"])


@pytest.mark.parametrize("layout", ["dense", "permuted"])
def test_tv_and_jerk_mean(dev, layout):
    """dense (B, C, T), and the (B, C, T) view of a dense (B, T, C) tensor (the gradient goes to the storage as it lies)"""
    base = C.draw(torch.Generator().manual_seed(0), 2, 9, 5)

    def view(t):
        return t.permute(0, 2, 1) if layout == "permuted" else t

    def tv(b, t):
        v = view(t)
        if not b.twin:
            return ops.tv_mean(v)
        d = v[:, :, 1:] - v[:, :, :-1]
        b.gaps.append(d.detach())
        return d.abs().mean()

    def jerk(b, t):
        v = view(t)
        if not b.twin:
            y = ops.jerk_mean(v)
            assert not y.requires_grad
            return y
        d = v[:, :, 3:] - 3 * v[:, :, 2:-1] + 3 * v[:, :, 1:-2] - v[:, :, :-3]
        return (d ** 2).sum(dim=1).mean().detach()

    _point(dev, "tv_mean " + layout, tv, [base], ["x"])
    _check(dev, "jerk_mean " + layout, lambda b: {"y": jerk(b, b.leaf(base))}, lambda ref: {"y": TOL_POINT})


def test_cross_entropy_first_order(dev):
    g = torch.Generator().manual_seed(0)
    logits, target = C.draw(g, 6, 10, scale=2.0), torch.tensor([3, 0, 9, 3, 7, 1])
    _point(dev, "cross_entropy", lambda b, x, t: F.cross_entropy(x, t) if b.twin else ops.cross_entropy(x, t),
           [logits, target], ["logits", None])


@pytest.mark.parametrize("target", [0.0, 1.0, 0.9])
def test_bce_with_logits_first_order(dev, target):
    logits = C.draw(torch.Generator().manual_seed(0), 5, 3, scale=2.0)
    _point(dev, "bce_with_logits t=%.1f" % target,
           lambda b, x: F.binary_cross_entropy_with_logits(x, torch.full_like(x, target)) if b.twin else ops.bce_with_logits(x, target),
           [logits], ["logits"])


@pytest.mark.parametrize("lp", [False, True], ids=["gp", "lp"])
def test_gp_penalty_first_order(dev, lp):
    """rows: norm above 1, norm 0.5 (LP: no penalty, no gradient), all zero, norm above 1. The GP twin carries the 1e-12
    inside the square root that ops.gp_penalty's docstring states; the LP twin's norm is the plain one (its square root
    is taken of 1 where the row is zero, so that the clamped branch's zero gradient is not 0 * inf)."""
    g = C.draw(torch.Generator().manual_seed(0), 4, 12)
    g[1] *= 0.5 / g[1].norm()
    g[2] = 0.0

    def fn(b, g):
        if not b.twin:
            return ops.gp_penalty(g, lp)
        q = (g * g).sum(1)
        if lp:
            live = q > 0
            return ((torch.sqrt(torch.where(live, q, torch.ones_like(q))) * live - 1).clamp_min(0) ** 2).mean()
        return ((torch.sqrt(q + 1e-12) - 1) ** 2).mean()

    _, ref = _point(dev, "gp_penalty " + ("lp" if lp else "gp"), fn, [g], ["g"])
    assert not ref["d/dg"][2].any() and ref["d/dg"][0].any() and bool(ref["d/dg"][1].any()) == (not lp)


def test_gp_interpolate(dev):
    g = torch.Generator().manual_seed(0)
    real, fake, alpha = C.draw(g, 4, 30), C.draw(g, 4, 30), torch.rand(4, generator=g)

    def run(b):
        r, f, a = b.leaf(real), b.leaf(fake), b.leaf(alpha, False)
        if b.twin:
            return {"y": a.view(-1, 1) * r + (1 - a.view(-1, 1)) * f}
        y = ops.gp_interpolate(r, f, a)
        assert not y.requires_grad      # taken of detached inputs (losses.py:20 of the reference)
        return {"y": y}

    _check(dev, "gp_interpolate", run, lambda ref: {"y": TOL_POINT})
