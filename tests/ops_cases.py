"""What tests/test_ops_autograd.py is built from (a helper, not a test module): the layers of a case written twice - once
on music2dance_amd.ops, once as an fp64 twin in plain torch ops - the three forms a case is differentiated in, the
kink guard, the comparison and the case tables.

Every case draws its fp32 values on the CPU from torch.Generator().manual_seed(seed); the product build gets them as
they are (moved to its device), the twin gets them widened to fp64. The seed stands in the table: it was picked here,
on the CPU, so that no pre-activation in front of a ReLU / LeakyReLU (and no max-pool pair) of the TWIN lies within
1e-5 of the layer's largest - the kernels err by about 2e-6 of that, so both builds take the same side of every kink
and the comparison is elementwise, with no allowance for flips. Tests never search seeds.

Bounds (all the project's own, see the test module's docstring): 2e-5 per contraction layer on a path for values and
input-side gradients, 3e-5 per contraction layer for parameter gradients (weights, biases, tables), 1e-6 for ops that
hold no contraction, BatchNorm 1e-5 forward / 2e-5 backward. Error is max|got - ref64| / max|ref64| per tensor."""
import torch
import torch.nn.functional as F

from music2dance_amd import ops
from tests.test_p2_cond_host import CondFakeKernels
from tests.test_p2_gan_host import BceFakeKernels

KINK = 1e-5          # the guard: min|z| > KINK * max|z| per activation layer of the twin
TOL_PATH = 2e-5      # per contraction layer: values, input gradients
TOL_PARAM = 3e-5     # per contraction layer: weight / bias / table gradients
TOL_POINT = 1e-6     # ops without a contraction
TOL_BN_FWD, TOL_BN_BWD = 1e-5, 2e-5
grad = torch.autograd.grad


class OpsFakeKernels(CondFakeKernels, BceFakeKernels):
    """The CPU stand-in with every entry music2dance_amd.ops calls: FakeKernels + the label / dropout entries + the BCE
    pair (both restated by the host tests of the features that brought them) + the softmax cross-entropy pair."""

    def cross_entropy_fwd(self, logits, labels, with_pred=False):
        return F.cross_entropy(logits, labels), (logits.argmax(1) if with_pred else None)

    def cross_entropy_bwd(self, logits, labels, gout):
        p = torch.softmax(logits, 1)
        p[torch.arange(logits.shape[0]), labels] -= 1.0
        return p * (gout / logits.shape[0])


def draw(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ------------------------------------------------------------------------------------------------ the two builds
class Build:
    """One build of a case. twin: fp64 torch ops on the CPU, recording every pre-activation (`zs`) and pool gap
    (`gaps`); else music2dance_amd.ops on `dev`. Both record the sign pattern behind every activation (`signs`)."""

    def __init__(self, dev, twin):
        self.dev, self.twin = dev, twin
        self.dtype = torch.float64 if twin else torch.float32
        self.zs, self.gaps, self.signs = [], [], []

    def leaf(self, t, requires_grad=True):
        t = t.detach().to(device=self.dev, dtype=self.dtype if t.is_floating_point() else t.dtype).clone()
        return t.requires_grad_(True) if requires_grad else t

    # -- activations
    def _act_twin(self, z, act, slope):
        if act == ops.ACT_NONE:
            return z
        self.zs.append(z.detach())
        self.signs.append((z > 0).detach())
        return F.relu(z) if act == ops.ACT_RELU else F.leaky_relu(z, slope)

    def _seen(self, y, act):
        if act != ops.ACT_NONE:
            self.signs.append((y > 0).detach().cpu())
        return y

    # -- layers
    def conv(self, x, w, b, stride=1, pad=0, act=0, slope=0.0, in_act=None, out_pm=False):
        if self.twin:
            return self._act_twin(F.conv1d(x, w, b, stride=stride, padding=pad), act, slope)
        return self._seen(ops.conv1d(x, w, b, stride, pad, act, slope, in_act=in_act, out_pm=out_pm), act)

    def linear(self, x, w, b, act=0, slope=0.0):
        if self.twin:
            return self._act_twin(F.linear(x, w, b), act, slope)
        return self._seen(ops.linear(x, w, b, act, slope), act)

    def tanh(self, x):
        return torch.tanh(x) if self.twin else ops.tanh(x)

    def label_concat(self, x, E, labels, layout):
        if not self.twin:
            return ops.label_concat(x, E, labels, layout)
        e = E[labels]                                                   # the embedding lookup
        if layout == 0:
            return torch.cat((x, e[:, None, :].expand(-1, x.shape[1], -1)), 2)
        return torch.cat((x, e[:, :, None].expand(-1, -1, x.shape[2])), 1)

    def dropout(self, x, keep, p):
        if self.twin:
            return x * keep.to(x.dtype) / (1.0 - p)
        return ops.dropout(x, p, mask=keep)[0]


def kink_guard(b):
    """on the twin alone: every pre-activation and pool gap clear of its kink by KINK of the layer's largest"""
    assert b.twin
    for i, z in enumerate(b.zs + b.gaps):
        lo, hi = float(z.abs().min()), float(z.abs().max())
        assert lo > KINK * hi, "layer %d of the twin comes within %.1e of a kink (largest %.3g): pick another seed" % (i, lo, hi)


def same_signs(b, twin):
    assert len(b.signs) == len(twin.signs)
    for i, (s, t) in enumerate(zip(b.signs, twin.signs)):
        n = int((s != t).sum())
        assert n == 0, "activation %d: %d of %d elements on the other side of the kink than in the fp64 twin" % (i, n, t.numel())


# ------------------------------------------------------------------------------------------------ comparison
def rel_err(got, ref64):
    """max|got - ref64| / max|ref64| (no floor under the denominator)"""
    ref64 = ref64.detach().double()
    return float((got.detach().double().cpu() - ref64).abs().max() / ref64.abs().max())


def compare(got, ref, bounds, note, key):
    """got / ref: {name: tensor or None}; bounds: {name: bound}. Where the twin has no gradient (None or all zeros) the
    product has none or exact zeros. Prints every figure, notes the worst under `key`, then asserts."""
    assert set(got) == set(ref) == set(bounds), (sorted(got), sorted(ref), sorted(bounds))
    bad = []
    for name in ref:
        g, r = got[name], ref[name]
        if r is None or not bool(r.any()):
            if g is not None and bool(g.any()):
                bad.append("%s: the twin has no gradient, the product has %.3e" % (name, float(g.abs().max())))
            continue
        if g is None:
            bad.append("%s: no gradient (the twin has one)" % name)
            continue
        assert g.shape == r.shape, (name, g.shape, r.shape)
        e = rel_err(g, r)
        print("FIGURE %s %s %.3e (bound %.1e)" % (key, name, e, bounds[name]))
        note(key, e)
        if not e <= bounds[name]:
            bad.append("%s: %.3e > %.1e" % (name, e, bounds[name]))
    assert not bad, "%s: %s" % (key, "; ".join(bad))


def path_bounds(names, n_contractions, params):
    """the chain rule of the bounds: first-order error bounds add along a path"""
    return {n: (TOL_PARAM if n in params else TOL_PATH) * n_contractions for n in names}


# ------------------------------------------------------------------------------------------------ the three forms
def penalty_form(b, net, x, P, names, c):
    """y = net(x); score_b = sum(y_b * c_b); gx = d sum(score) / dx with a graph; loss = mean((|gx_b| - 1)^2) +
    0.1 mean(y^2); -> y, gx and the gradients of loss w.r.t. x and every parameter."""
    x = b.leaf(x)
    P = [b.leaf(p) if p.is_floating_point() else b.leaf(p, False) for p in P]
    y = net(b, x, P)
    B = y.shape[0]
    score = (y * b.leaf(c, False)).reshape(B, -1).sum(1)
    (gx,) = grad(score.sum(), x, create_graph=True)
    pen = ((gx.reshape(B, -1).norm(dim=1) - 1) ** 2).mean()
    loss = pen + 0.1 * (y ** 2).mean()
    leaves = [(n, p) for n, p in zip(names, P) if p.is_floating_point()]
    gs = grad(loss, [x] + [p for _, p in leaves], allow_unused=True)
    out = {"y": y.detach(), "gx": gx.detach(), "d/dx": gs[0]}
    out.update({"d/d" + n: g for (n, _), g in zip(leaves, gs[1:])})
    return out


def weight_side_form(b, net, x, P, names, c, c1, c2):
    """gw, gb = d sum(score) / d(P[0], P[1]) with a graph; -> gw, gb and the gradients of sum(gw c1) + sum(gb c2) w.r.t.
    x, the layer's own weight and the next layer's weight (P[2])."""
    x = b.leaf(x)
    P = [b.leaf(p) for p in P]
    y = net(b, x, P)
    B = y.shape[0]
    score = (y * b.leaf(c, False)).reshape(B, -1).sum(1)
    gw, gb = grad(score.sum(), (P[0], P[1]), create_graph=True)
    obj = (gw * b.leaf(c1, False)).sum() + (gb * b.leaf(c2, False)).sum()
    gs = grad(obj, [x, P[0], P[2]], allow_unused=True)
    return {"y": y.detach(), "gw": gw.detach(), "gb": gb.detach(), "d/dx": gs[0], "d/d" + names[0]: gs[1],
            "d/d" + names[2]: gs[2]}


def first_order_form(b, fn, inputs, names, c_seed=1):
    """y = fn(b, *leaves); -> y and the gradients of sum(y * c) w.r.t. every floating-point input that is named"""
    leaves = [b.leaf(t, n is not None) if t.is_floating_point() else b.leaf(t, False) for t, n in zip(inputs, names)]
    y = fn(b, *leaves)
    c = draw(torch.Generator().manual_seed(c_seed), *y.shape) if y.dim() else torch.tensor(1.3)
    want = [(n, t) for n, t in zip(names, leaves) if n is not None]
    gs = grad((y * b.leaf(c, False)).sum(), [t for _, t in want], allow_unused=True)
    out = {"y": y.detach()}
    out.update({"d/d" + n: g for (n, _), g in zip(want, gs)})
    return out


# ------------------------------------------------------------------------------------------------ conv cases
# (id, route and the condition in csrc/conv1d.hip / conv1d_thin.hip / tcn.hip that sends the shape there,
#  (B, Cin, L, Cout, k, stride, pad), m2d_conv1d_k4_applicable, HipKernels._thin, also run inside a flagged chain)
CONV_ROUTES = [
    ("engine-unpacked", "engine, unpacked operand: Cin < 16 (conv_uses_packed)", (2, 3, 17, 5, 3, 2, 1), False, False, False),
    ("engine-packed-ragged", "engine, packed, ragged 16-channel chunk: Cin 20", (2, 20, 50, 24, 5, 3, 2), False, False, False),
    ("full-length", "full-length: Lout == 1, pad == 0, L == k", (3, 20, 12, 6, 12, 1, 0), False, False, False),
    ("thin-k25s4", "thin k25/s4: thin_ok (Cin 1, Cout 32)", (2, 1, 256, 32, 25, 4, 11), False, True, False),
    ("thin-sibling-cout8", "k25/s4 with Cout 8: not thin_ok, the engine", (2, 1, 256, 8, 25, 4, 11), False, False, True),
    ("thin-long-k250s50", "thin-long forward k250/s50: Lout % 32 == 0", (2, 1, 1552, 32, 250, 50, 124), False, False, False),
    ("thin-long-k160s4", "thin-long forward k160/s4: Lout % 32 == 0", (2, 1, 128, 32, 160, 4, 79), False, False, False),
    ("k4-paired", "k4 forward, phantom-paired order: k4_paired (k25, pad 11)", (2, 16, 64, 64, 25, 4, 11), True, False, False),
    ("k4-plain", "k4 forward, plain order: k24", (2, 16, 64, 64, 24, 4, 11), True, False, False),
    ("subpixel-ci-r", "sub-pixel backward-data, (ci, r) order: 64 <= Cin * s <= 128", (2, 32, 16, 64, 4, 2, 1), False, False, False),
    ("subpixel-32x4", "sub-pixel, 32 channels x 4 phases: tall kernel on an unmasked dy, register staging on a masked one",
     (2, 32, 64, 64, 25, 4, 11), True, False, True),
    ("subpixel-phase-major", "sub-pixel phase-major: subpixel_tall (Cin 64), unmasked dy only; masked: the engine",
     (2, 64, 64, 64, 25, 4, 11), True, False, True),
    ("tcn-ragged", "TemporalBlock conv + weight-gradient kernels, ragged channel block: Cin 20, L % 60 == 0",
     (2, 20, 60, 128, 7, 1, 3), False, False, True),
    ("tcn-full", "TemporalBlock kernels, full 128 channels", (1, 128, 60, 128, 7, 1, 3), False, False, True),
]
ACTS = {"relu": (ops.ACT_RELU, 0.0), "leaky": (ops.ACT_LEAKY, 0.2)}
C_POST = 4   # output channels of the k = 1 conv behind the layer under test

# seeds that pass the kink guard, found on the CPU (key: "<route id>-<act>" or "<route id>-<act>-flags"); others: 0
CONV_SEEDS = {"tcn-ragged-relu": 1, "tcn-ragged-relu-flags": 2, "tcn-ragged-leaky": 1, "tcn-full-relu": 1,
              "tcn-full-relu-flags": 1, "tcn-full-leaky": 1, "tcn-full-leaky-flags": 1}


def conv_case_ids():
    ids = []
    for rid, _, _, _, _, chained in CONV_ROUTES:
        for act in ACTS:
            ids.append("%s-%s" % (rid, act))
            if chained:
                ids.append("%s-%s-flags" % (rid, act))
    return ids


def conv_case(case_id):
    """-> dict(route row, act, slope, flags, x, P, names, net, n_contractions)"""
    flags = case_id.endswith("-flags")
    rid, act_name = (case_id[:-6] if flags else case_id).rsplit("-", 1)
    row = next(r for r in CONV_ROUTES if r[0] == rid)
    B, Cin, L, Cout, k, s, p = row[2]
    act, slope = ACTS[act_name]
    g = torch.Generator().manual_seed(CONV_SEEDS.get(case_id, 0))
    x = draw(g, B, Cin, L)
    P, names = [], []
    if flags:   # a k = 1 layer in front, so that the layer under test has an activation to pre-mask for
        P += [draw(g, Cin, Cin, 1, scale=Cin ** -0.5), draw(g, Cin, scale=0.3)]
        names += ["W0", "b0"]
    P += [draw(g, Cout, Cin, k, scale=(Cin * k) ** -0.5), draw(g, Cout, scale=0.3),
          draw(g, C_POST, Cout, 1, scale=Cout ** -0.5), draw(g, C_POST, scale=0.3)]
    names += ["W", "b", "W2", "b2"]

    def net(b, x, P):
        if flags:
            x = b.conv(x, P[0], P[1], 1, 0, act, slope, None, True)
            P = P[2:]
        y = b.conv(x, P[0], P[1], s, p, act, slope, (act, slope) if flags else None, flags)
        return b.conv(y, P[2], P[3], 1, 0, 0, 0.0, (act, slope) if flags else None, False)

    Lout = (L + 2 * p - k) // s + 1
    return dict(row=row, act=act, slope=slope, flags=flags, x=x, P=P, names=names, net=net, n=3 if flags else 2,
                c=draw(g, B, C_POST, Lout))


# ------------------------------------------------------------------------------------------------ other chains
def linear_case(shape, act_name, bias, seed):
    """linear(act) -> linear; shape (N, in, out) or (B, T, in, out) for the 3-D input"""
    *lead, fin, fout = shape
    act, slope = ACTS.get(act_name, (ops.ACT_NONE, 0.0))
    g = torch.Generator().manual_seed(seed)
    x = draw(g, *lead, fin)
    P = [draw(g, fout, fin, scale=fin ** -0.5)] + ([draw(g, fout, scale=0.3)] if bias else []) + \
        [draw(g, 3, fout, scale=fout ** -0.5), draw(g, 3, scale=0.3)]
    names = ["W"] + (["b"] if bias else []) + ["W2", "b2"]

    def net(b, x, P):
        w, bb, w2, b2 = (P[0], P[1], P[2], P[3]) if bias else (P[0], None, P[1], P[2])
        return b.linear(b.linear(x, w, bb, act, slope), w2, b2)

    return dict(x=x, P=P, names=names, net=net, n=2, c=draw(g, *lead, 3))


def tanh_case(seed):
    g = torch.Generator().manual_seed(seed)
    x = draw(g, 7, 33)
    P = [draw(g, 20, 33, scale=33 ** -0.5), draw(g, 20, scale=0.3), draw(g, 3, 20, scale=20 ** -0.5), draw(g, 3, scale=0.3)]

    def net(b, x, P):
        return b.linear(b.tanh(b.linear(x, P[0], P[1])), P[2], P[3])

    return dict(x=x, P=P, names=["W", "b", "W2", "b2"], net=net, n=2, c=draw(g, 7, 3))


def dropout_case(p, seed):
    g = torch.Generator().manual_seed(seed)
    x = draw(g, 7, 33)
    keep = (torch.rand(7, 20, generator=g) >= p).to(torch.uint8)
    P = [draw(g, 20, 33, scale=33 ** -0.5), draw(g, 20, scale=0.3), draw(g, 3, 20, scale=20 ** -0.5), draw(g, 3, scale=0.3), keep]

    def net(b, x, P):
        return b.linear(b.dropout(b.linear(x, P[0], P[1], ops.ACT_LEAKY, 0.2), P[4], p), P[2], P[3])

    return dict(x=x, P=P, names=["W", "b", "W2", "b2", "keep"], net=net, n=2, c=draw(g, 7, 3))


LABELS = [2, 0, 2, 1]   # label 2 occurs twice in the batch; 4 rows of a 3 x D table


def label_case(layout, seed):
    """layout 0: [x | E[l]] (B, T, C + D) -> linear(leaky) -> tanh -> linear; layout 1: (B, C + D, T) -> conv(leaky) ->
    tanh -> k1 conv. The tanh gives gx a dependence on E, so that the table's gradient has a second-order part."""
    g = torch.Generator().manual_seed(seed)
    B, T, C, D = 4, 6, 5, 3
    labels = torch.tensor(LABELS)
    E = draw(g, 3, D)
    if layout == 0:
        x = draw(g, B, T, C)
        P = [E, draw(g, 9, C + D, scale=(C + D) ** -0.5), draw(g, 9, scale=0.3), draw(g, 2, 9, scale=1 / 3), draw(g, 2, scale=0.3), labels]

        def net(b, x, P):
            h = b.label_concat(x, P[0], P[5], 0)
            return b.linear(b.tanh(b.linear(h, P[1], P[2], ops.ACT_LEAKY, 0.2)), P[3], P[4])

        c = draw(g, B, T, 2)
    else:
        x = draw(g, B, C, T)
        P = [E, draw(g, 9, C + D, 3, scale=(3 * (C + D)) ** -0.5), draw(g, 9, scale=0.3), draw(g, 2, 9, 1, scale=1 / 3), draw(g, 2, scale=0.3), labels]

        def net(b, x, P):
            h = b.label_concat(x, P[0], P[5], 1)
            return b.conv(b.tanh(b.conv(h, P[1], P[2], 1, 1, ops.ACT_LEAKY, 0.2)), P[3], P[4])

        c = draw(g, B, 2, T)
    return dict(x=x, P=P, names=["E", "W", "b", "W2", "b2", "labels"], net=net, n=2, c=c)


def critic_case(flags, seed):
    """label_concat(1) -> conv(leaky) -> conv(relu, stride 2) -> full-length conv -> tanh -> linear"""
    g = torch.Generator().manual_seed(seed)
    B, T, C, D = 4, 12, 5, 3
    x = draw(g, B, C, T)
    P = [draw(g, 3, D),
         draw(g, 10, C + D, 3, scale=(3 * (C + D)) ** -0.5), draw(g, 10, scale=0.3),
         draw(g, 12, 10, 3, scale=30 ** -0.5), draw(g, 12, scale=0.3),
         draw(g, 7, 12, 6, scale=72 ** -0.5), draw(g, 7, scale=0.3),
         draw(g, 1, 7, scale=7 ** -0.5), draw(g, 1, scale=0.3), torch.tensor(LABELS)]

    def net(b, x, P):
        h = b.label_concat(x, P[0], P[9], 1)
        h = b.conv(h, P[1], P[2], 1, 1, ops.ACT_LEAKY, 0.2, None, flags)
        h = b.conv(h, P[3], P[4], 2, 1, ops.ACT_RELU, 0.0, (ops.ACT_LEAKY, 0.2) if flags else None, flags)
        h = b.conv(h, P[5], P[6], 1, 0, 0, 0.0, (ops.ACT_RELU, 0.0) if flags else None, False)
        return b.linear(b.tanh(h.reshape(B, 7)), P[7], P[8])

    return dict(x=x, P=P, names=["E", "W1", "b1", "W2", "b2", "W3", "b3", "W4", "b4", "labels"], net=net, n=4,
                c=draw(g, B, 1))
