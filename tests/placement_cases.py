"""What tests/test_placement_host.py and tests/test_gpu_operand_placement.py are built from (a helper, not a test module;
no device is needed to import it): operands placed OFF 16-byte alignment.

Every tensor a test makes comes fresh from an allocator that aligns to 512 bytes, so the unaligned arm of every pointer
test in the library ("Operand alignment") never ran. In production operands do sit at 4-byte boundaries: the
gradient views of a data-parallel bucket (dp.py lays them end to end in one flat buffer), `out=` / `sum_out=` views, a
caller's slices. Here:

  place(t_cpu, off, device)   a copy of `t_cpu` that starts `off` elements past a 16-byte boundary inside a buffer full of
                              a sentinel, with `guard` sentinel elements on either side
  guards_intact(buf, view)    nothing outside the view was written
  CASES                       one Case per entry point (and route) of kernels.HipKernels: CPU operands at the smallest
                              shape that reaches the vector arm, which of them can be placed, which the call writes, a
                              plain-torch fp64 reference and the bound of the op's family
  EXEMPT                      the public methods of HipKernels that take a tensor and have no case, each with its reason

Bounds are the suite's own, measured the same way (rel_err: max|got - ref64| / max(1, max|ref64|)): 2e-5 contractions,
3e-5 weight / bias gradients (tests/test_gpu_kernels.py, tests/test_gpu_tcn.py), BatchNorm 1e-5 forward / 2e-5 backward,
1e-6 running buffers and ops without a contraction, 1e-5 channel sums and recurrences (2e-5 their gradients), the Adam
bounds of tests/test_optim.py. Cases marked `exact` are elementwise or data movement: access width changes no
arithmetic there, and the GPU test holds every placement bit-equal to the aligned call."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

GUARD = 64
TOL_PATH, TOL_PARAM, TOL_POINT = 2e-5, 3e-5, 1e-6
TOL_BN_FWD, TOL_BN_BWD, TOL_SUMS, TOL_GRU = 1e-5, 2e-5, 1e-5, 1e-5


def sentinel(dtype):
    """finite, non-zero, exactly representable in every dtype an operand has"""
    return 1234.5 if dtype.is_floating_point else 90


def place(t_cpu, off, device, guard=GUARD):
    """-> (view, buf): `buf` is one flat buffer of guard + 16 bytes + numel + guard elements of t's dtype, filled with the
    sentinel; `view` is the contiguous view of t's shape that starts at element guard + off, holding t's data. `off`
    counts elements: floats for fp32 (residue 4 * off), bytes for uint8, 8-byte steps for int64 / fp64."""
    t = t_cpu.detach().contiguous()
    step = t.element_size()
    n = t.numel()
    buf = torch.empty(guard + 16 // step + n + guard, dtype=t.dtype, device=device)
    buf.fill_(sentinel(t.dtype))
    view = buf[guard + off:guard + off + n].view(t.shape)
    view.copy_(t)
    assert 0 <= off * step < 16 and buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == off * step, (off, step)
    return view, buf


def guards_intact(buf, view):
    """every element of `buf` outside `view` still equals the sentinel (a NaN written there differs too)"""
    start = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    s = sentinel(buf.dtype)
    return bool((buf[:start] == s).all()) and bool((buf[start + view.numel():] == s).all())


def rel_err(got, ref64):
    got, ref64 = got.detach().cpu().double(), ref64.detach().cpu().double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if got.numel() == 0:
        return 0.0
    return (got - ref64).abs().max().item() / max(1.0, ref64.abs().max().item())


def within(got, ref64, tol):
    """-> (ok, figure). tol: a rel_err bound; ("allclose", rtol, atol) as tests/test_optim.py holds parameters;
    ("max", t): relative to the reference's largest element with no floor (its moments, the loss gradients);
    ("abs", t): the largest difference itself (the scalar losses); None: equal values (indices, pixels); a callable
    (got, ref64) -> (ok, figure): a metric's own bound, restated from its GPU test."""
    if tol is None:
        return torch.equal(got.detach().cpu().double(), ref64.detach().cpu().double()), 0.0
    if callable(tol):
        return tol(got.detach().cpu().double(), ref64.detach().cpu().double())
    if isinstance(tol, tuple) and tol[0] == "allclose":
        g, r = got.detach().cpu().double(), ref64.detach().cpu().double()
        fig = ((g - r).abs() - tol[1] * r.abs()).max().item()
        return fig <= tol[2], fig
    if isinstance(tol, tuple) and tol[0] == "abs":
        fig = (got.detach().cpu().double() - ref64.detach().cpu().double()).abs().max().item()
        return fig <= tol[1], fig
    if isinstance(tol, tuple) and tol[0] == "max":
        g, r = got.detach().cpu().double(), ref64.detach().cpu().double()
        fig = (g - r).abs().max().item() / r.abs().max().item()
        return fig <= tol[1], fig
    e = rel_err(got, ref64)
    return e <= tol, e


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def mf(mask, slope):
    return torch.where(mask > 0, torch.ones_like(mask), torch.full_like(mask, slope))


def act_(y, act, slope):
    return y if act == 0 else (F.relu(y) if act == 1 else F.leaky_relu(y, slope))


class Case:
    """name: id; op: the HipKernels method(s) it covers (a name or a tuple); make() -> {operand: CPU tensor};
    run(K, t) -> tuple of result tensors from operands `t` on K's device; ref(t64) -> the same tuple in fp64 from the
    operands widened to fp64 (None: that result is held by the other checks only); place: the operands a caller
    supplies; written: those of them the call writes; tol: one bound, or one per result; exact: see the module docstring;
    hip_only: `run` needs the library itself (weight images, device random bits); extra(outs, t): what else must hold
    of the results `outs` a run on operands `t` gave (asserts)."""

    def __init__(self, name, op, make, run, ref, place, written=(), tol=TOL_PATH, exact=False, hip_only=False, extra=None):
        self.name, self.ops = name, ((op,) if isinstance(op, str) else tuple(op))
        self._make, self.run, self._ref = make, run, ref
        self.place, self.written, self.tol, self.exact, self.hip_only = tuple(place), tuple(written), tol, exact, hip_only
        self.extra = extra

    @functools.lru_cache(maxsize=None)
    def operands(self):
        t = self._make()
        assert set(self.place) <= set(t) and set(self.written) <= set(self.place), self.name
        return t

    @functools.lru_cache(maxsize=None)
    def reference(self):
        """computed once, shared by every placement"""
        t64 = {k: (v.double() if v.dtype == torch.float32 else v.clone()) for k, v in self.operands().items()}
        return tuple(self._ref(t64))

    def tols(self, n):
        return self.tol if isinstance(self.tol, list) else [self.tol] * n

    def __repr__(self):
        return self.name


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


# ------------------------------------------------------------------------------------------------------------ conv1d
# (name, B, Cin, L, Cout, ks, stride, pad): one layer per route of csrc/conv1d.hip, shapes of tests/test_gpu_kernels.py
CONV_LAYERS = {
    "unet.k3.25": (2, 128, 25, 128, 3, 1, 1),      # generic engine, packed image
    "enc.c1": (6, 32, 64, 64, 4, 2, 1),            # generic engine, 16-byte epilogue rows
    "k4pair.a": (1, 16, 512, 64, 25, 4, 11),       # tap-vectorised stride-4 forward, phantom-paired order
    "k4plain.a": (2, 32, 1024, 64, 24, 4, 11),     # ... plain order
    "subpixel": (3, 32, 384, 64, 25, 4, 11),       # sub-pixel backward-data (quad epilogue), phase-major at 32 channels
    "subpixel.ragged": (3, 64, 260, 48, 25, 4, 11),  # phase-major with ragged row ends
    "wg.l1": (3, 1, 3200, 32, 25, 4, 0),           # thin (Cin = 1) kernels, Lout = 794: 8-byte rows
    "enc.c0": (6, 1, 3200, 32, 250, 50, 124),      # thin, k250
    "tcn.3": (3, 128, 120, 128, 7, 1, 3),          # TemporalBlock kernels
    "tcn.50": (50, 128, 120, 128, 7, 1, 3),        # ... a launch of several tile rounds
    "p2.lastconv": (4, 128, 120, 1, 120, 1, 0),    # full-length kernel: a plain NT GEMM
}
THIN = ("wg.l1", "enc.c0")


def _conv_ops(layer, seed=0):
    B, Cin, L, Cout, ks, s, p = CONV_LAYERS[layer]
    Lout = (L + 2 * p - ks) // s + 1
    return {"x": gen(B, Cin, L, seed=seed + 1), "w": gen(Cout, Cin, ks, seed=seed + 2, scale=1.0 / math.sqrt(Cin * ks)),
            "bias": gen(Cout, seed=seed + 3, scale=0.1), "dy": gen(B, Cout, Lout, seed=seed + 4),
            "ymask": gen(B, Cout, Lout, seed=seed + 5), "yres": gen(B, Cout, Lout, seed=seed + 6),
            "xmask": gen(B, Cin, L, seed=seed + 7), "xres": gen(B, Cin, L, seed=seed + 8),
            "y": torch.zeros(B, Cout, Lout), "y2": torch.zeros(B, Cout, Lout), "dx": torch.zeros(B, Cin, L)}


def _pick(layer, names):
    return lambda: {k: v for k, v in _conv_ops(layer).items() if k in names}


def _conv_fwd(layer, form):
    B, Cin, L, Cout, ks, s, p = CONV_LAYERS[layer]
    conv = lambda t: F.conv1d(t["x"], t["w"], t["bias"], stride=s, padding=p)
    if form == "plain":       # bias + ReLU into a caller's view
        names = ("x", "w", "bias", "y")
        run = lambda K, t: (K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=1, out=t["y"]),)
        ref = lambda t: (F.relu(conv(t)),)
        written = ("y",)
    elif form == "full":      # leaky + out mask + residual into a caller's view
        names = ("x", "w", "bias", "yres", "ymask", "y")
        run = lambda K, t: (K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=2, slope=0.2, residual=t["yres"],
                                         out_mask=t["ymask"], out_mask_slope=0.2, out=t["y"]),)
        ref = lambda t: (F.leaky_relu(conv(t), 0.2) * mf(t["ymask"], 0.2) + t["yres"],)
        written = ("y",)
    elif form == "sum":       # two outputs: y and sum_out = y + residual
        names = ("x", "w", "bias", "yres", "y", "y2")
        run = lambda K, t: K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=1, residual=t["yres"], out=t["y"],
                                        sum_out=t["y2"])
        ref = lambda t: (F.relu(conv(t)), F.relu(conv(t)) + t["yres"])
        written = ("y", "y2")
    else:                     # epilogue statistics
        names = ("x", "w", "bias")
        run = lambda K, t: K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=2, slope=0.2, with_stats=True)

        def ref(t):
            y = F.leaky_relu(conv(t), 0.2)
            return y, torch.stack((y.sum((0, 2)), (y * y).sum((0, 2))), 1).reshape(-1)
        written = ()
    case("conv1d_fwd %s %s" % (layer, form), "conv1d_fwd", _pick(layer, names), run, ref, names, written,
         tol=[TOL_PATH, TOL_SUMS] if form == "stats" else TOL_PATH)


def _conv_bwd_data(layer, form):
    B, Cin, L, Cout, ks, s, p = CONV_LAYERS[layer]

    def gx(t, dy):
        return torch.nn.grad.conv1d_input((B, Cin, L), t["w"], dy, stride=s, padding=p)
    if form == "plain":
        names = ("dy", "w", "dx")
        run = lambda K, t: (K.conv1d_bwd_data(t["dy"], t["w"], L, s, p, out=t["dx"]),)
        ref = lambda t: (gx(t, t["dy"]),)
    elif form == "epi":       # residual, then the output mask
        names = ("dy", "w", "xmask", "xres", "dx")
        run = lambda K, t: (K.conv1d_bwd_data(t["dy"], t["w"], L, s, p, out_mask=t["xmask"], out_mask_slope=0.2,
                                              residual=t["xres"], out=t["dx"]),)
        ref = lambda t: ((gx(t, t["dy"]) + t["xres"]) * mf(t["xmask"], 0.2),)
    else:                     # ... with a masked dy
        names = ("dy", "w", "ymask", "xmask", "xres", "dx")
        run = lambda K, t: (K.conv1d_bwd_data(t["dy"], t["w"], L, s, p, dy_mask=t["ymask"], dy_mask_slope=0.2,
                                              out_mask=t["xmask"], out_mask_slope=0.2, residual=t["xres"], out=t["dx"]),)
        ref = lambda t: ((gx(t, t["dy"] * mf(t["ymask"], 0.2)) + t["xres"]) * mf(t["xmask"], 0.2),)
    case("conv1d_bwd_data %s %s" % (layer, form), "conv1d_bwd_data", _pick(layer, names), run, ref, names, ("dx",))


def _conv_bwd_weight(layer, masked):
    B, Cin, L, Cout, ks, s, p = CONV_LAYERS[layer]
    names = ("x", "dy", "ymask") if masked else ("x", "dy")

    def run(K, t):
        return K.conv1d_bwd_weight(t["x"], t["dy"], ks, s, p, dy_mask=t["ymask"] if masked else None,
                                   dy_mask_slope=0.2, with_bias=True)

    def ref(t):
        dy = t["dy"] * mf(t["ymask"], 0.2) if masked else t["dy"]
        return torch.nn.grad.conv1d_weight(t["x"], (Cout, Cin, ks), dy, stride=s, padding=p), dy.sum((0, 2))
    case("conv1d_bwd_weight %s %s" % (layer, "masked" if masked else "plain"), "conv1d_bwd_weight", _pick(layer, names),
         run, ref, names, tol=TOL_PARAM)


for _l in CONV_LAYERS:
    _conv_fwd(_l, "plain")
    if _l not in ("subpixel.ragged",):
        _conv_bwd_weight(_l, False)
    _conv_bwd_data(_l, "plain")
for _l in ("enc.c1", "tcn.3", "tcn.50", "k4pair.a", "p2.lastconv"):
    _conv_fwd(_l, "full")
for _l in ("tcn.3", "tcn.50", "enc.c1"):
    _conv_fwd(_l, "sum")
_conv_fwd("enc.c1", "stats")
for _l in ("tcn.3", "tcn.50", "subpixel", "subpixel.ragged", "enc.c1"):
    _conv_bwd_data(_l, "epi")
for _l in ("tcn.3", "tcn.50"):
    _conv_bwd_data(_l, "full")
for _l in ("tcn.3", "enc.c1", "wg.l1"):
    _conv_bwd_weight(_l, True)

# conv over the windows of a padded track: (name, B, T, hop, window, Cout, ks, stride, pad) of tests/test_gpu_kernels.py
for _name, _B, _T, _hop, _win, _Cout, _ks, _s, _p in (("wavegan.l1-thin", 3, 6, 640, 3200, 32, 25, 4, 0),
                                                     ("odd-geometry", 4, 9, 37, 101, 8, 5, 2, 1)):
    def _win_ops(B=_B, T=_T, hop=_hop, win=_win, Cout=_Cout, ks=_ks, s=_s, p=_p):
        Lout = (win + 2 * p - ks) // s + 1
        return {"track": gen(B, (T - 1) * hop + win + 3, seed=1), "w": gen(Cout, 1, ks, seed=2, scale=1.0 / math.sqrt(ks)),
                "bias": gen(Cout, seed=3, scale=0.1), "dy": gen(B * T, Cout, Lout, seed=4), "ymask": gen(B * T, Cout, Lout, seed=5)}

    def _slices(t, T=_T, hop=_hop, win=_win):
        return t["track"].unfold(-1, win, hop)[:, :T].reshape(-1, 1, win)
    case("conv1d_fwd_windows " + _name, "conv1d_fwd_windows", _win_ops,
         lambda K, t, T=_T, hop=_hop, win=_win, s=_s, p=_p: (K.conv1d_fwd_windows(t["track"], T, hop, win, t["w"], t["bias"], s, p,
                                                                                  act=2, slope=0.2),),
         lambda t, s=_s, p=_p, sl=_slices: (F.leaky_relu(F.conv1d(sl(t), t["w"], t["bias"], stride=s, padding=p), 0.2),),
         ("track", "w", "bias"))
    case("conv1d_bwd_weight_windows " + _name, "conv1d_bwd_weight_windows", _win_ops,
         lambda K, t, T=_T, hop=_hop, win=_win, ks=_ks, s=_s, p=_p: K.conv1d_bwd_weight_windows(
             t["track"], T, hop, win, t["dy"], ks, s, p, dy_mask=t["ymask"], dy_mask_slope=0.2, with_bias=True),
         lambda t, Cout=_Cout, ks=_ks, s=_s, p=_p, sl=_slices: (
             torch.nn.grad.conv1d_weight(sl(t), (Cout, 1, ks), t["dy"] * mf(t["ymask"], 0.2), stride=s, padding=p),
             (t["dy"] * mf(t["ymask"], 0.2)).sum((0, 2))),
         ("track", "dy", "ymask"), tol=TOL_PARAM)


# -------------------------------------------------------------------------------------------------------------- gemm
GM, GN, GK = 480, 256, 256


def _gemm_ops(mode):
    a = gen(GM, GK, seed=10 + mode)
    b = gen(GN, GK, seed=20 + mode, scale=1.0 / math.sqrt(GK))
    t = {"a": a if mode != 2 else a.t().contiguous(), "b": b if mode == 0 else b.t().contiguous(),
         "bias": gen(GN, seed=30, scale=0.1), "out_mask": gen(GM, GN, seed=32), "c": torch.zeros(GM, GN)}
    if mode != 2:   # (mode 2 unmasked: a masked operand would keep it off the LDS-direct kernel)
        t["a_mask"] = gen(GM, GK, seed=31)
    return t


def _gemm_ref(mode, t, masked=True):
    a = t["a"] * mf(t["a_mask"], 0.2) if masked else t["a"]
    prod = a @ t["b"].t() if mode == 0 else (a @ t["b"] if mode == 1 else a.t() @ t["b"])
    return F.leaky_relu(prod + t["bias"], 0.2) * mf(t["out_mask"], 0.2)


for _mode in (0, 1, 2):
    case("gemm mode %d" % _mode, "gemm", functools.partial(_gemm_ops, _mode),
         lambda K, t, mode=_mode: (K.gemm(mode, t["a"], t["b"], t["bias"], act=2, slope=0.2, a_mask=t.get("a_mask"), a_mask_slope=0.2,
                                          out_mask=t["out_mask"], out_mask_slope=0.2, out=t["c"]),),
         functools.partial(lambda mode, t: (_gemm_ref(mode, t, "a_mask" in t),), _mode),
         ("a", "b", "bias", "out_mask", "c") + (("a_mask",) if _mode != 2 else ()), ("c",))


def _plain_gemm_run(K, t):
    """a forced (64 rows, 3 splits) plan without the stream's tickets: GEMM + the slab reduction, two launches"""
    if K.name != "hip":
        return (K.gemm(0, t["a"], t["b"], t["bias"], act=2, slope=0.2, out=t["c"]),)
    from tests import plan_cases
    from tests.test_gpu_gemm_plans import tickets
    with tickets(False), plan_cases.forced_plan(64, 3):
        return (K.gemm(0, t["a"], t["b"], t["bias"], act=2, slope=0.2, out=t["c"]),)


case("gemm mode 0 forced two-launch split-K", "gemm", lambda: {k: v for k, v in _gemm_ops(0).items() if k in ("a", "b", "bias", "c")},
     _plain_gemm_run, lambda t: (F.leaky_relu(t["a"] @ t["b"].t() + t["bias"], 0.2),), ("a", "b", "bias", "c"), ("c",))


# one column block per operand (tests/test_gpu_kernels.py::test_gemm_on_column_blocks_of_wider_buffers, mode 0): the
# WIDE buffers are what gets placed, the call takes their blocks; the reference leaves the rest of C as it was
LM, LN, LK = 37, 100, 128


def _ld_ops():
    return {"A": gen(LM, LK + 5, seed=40), "B": gen(LN, LK + 9, seed=41, scale=1.0 / math.sqrt(LK)),
            "AM": gen(LM, LK + 5, seed=42), "C": gen(LM, LN + 60, seed=43)}


def _ld_run(K, t):
    blk = t["C"][:, 20:20 + LN]
    K.gemm_ld(0, t["A"][:, 2:2 + LK], t["B"][:, 4:4 + LK], a_mask=t["AM"][:, 2:2 + LK], a_mask_slope=0.0, out_mask=blk,
              out_mask_slope=0.0, out=blk)
    return (t["C"],)


def _ld_ref(t):
    c = t["C"].clone()
    blk = c[:, 20:20 + LN]
    prod = (t["A"][:, 2:2 + LK] * (t["AM"][:, 2:2 + LK] > 0)) @ t["B"][:, 4:4 + LK].t()
    c[:, 20:20 + LN] = prod * (blk > 0)
    return (c,)


case("gemm_ld column blocks", "gemm_ld", _ld_ops, _ld_run, _ld_ref, ("A", "B", "AM", "C"), ("C",))


# -------------------------------------------------------------------------------------------------------- batch norm
BN_SHAPES = [(4, 128, 120), (64, 100, 1), (2, 32, 794)]


def _bn_ops(shape):
    B, C, L = shape
    x = gen(B, C, L, seed=1) * 1.5 + 0.3
    res, dy = gen(B, C, L, seed=9), gen(B, C, L, seed=6)
    if L == 1:
        x, res, dy = x.view(B, C), res.view(B, C), dy.view(B, C)
    x64 = x.double()
    dims = (0,) if L == 1 else (0, 2)
    mean = x64.mean(dims)
    var = ((x64 - mean.view((1, -1) + (() if L == 1 else (1,)))) ** 2).mean(dims)
    t = {"x": x, "gamma": 1.0 + gen(C, seed=2, scale=0.1), "beta": gen(C, seed=3, scale=0.1), "rm": gen(C, seed=4, scale=0.1),
         "rv": 1.0 + gen(C, seed=5, scale=0.1).abs(), "res": res, "dy": dy,
         "sums": torch.stack((x64.sum(dims), (x64 * x64).sum(dims)), 1).reshape(-1),
         "mean": mean.float(), "invstd": (1.0 / torch.sqrt(var + 1e-5)).float()}
    if L > 1:   # (out= takes channel blocks of (B, C, L) buffers: the two-dimensional form has none)
        t["y"] = torch.zeros_like(x)
    return t


def _bn_shape(t):
    return (1, -1) if t["x"].dim() == 2 else (1, -1, 1)


def _bn_train_ref(t, act, res):
    rm, rv = t["rm"].clone(), t["rv"].clone()
    z = F.batch_norm(t["x"], rm, rv, t["gamma"], t["beta"], True, 0.1, 1e-5)
    y = act_(z, act, 0.2) + (t["res"] if res else 0.0)
    return y, t["mean"].double(), t["invstd"].double(), rm, rv


def _bn_dz(t):
    sh = _bn_shape(t)
    xh = (t["x"] - t["mean"].view(sh)) * t["invstd"].view(sh)
    return t["dy"], xh     # (act = 0 in the backward cases: no kink for fp32 noise to cross)


def _bn_bwd_ref(t):
    sh = _bn_shape(t)
    dims = (0,) if t["x"].dim() == 2 else (0, 2)
    dz, xh = _bn_dz(t)
    n = t["x"].numel() // t["x"].shape[1]
    s1, s2 = dz.sum(dims), (dz * xh).sum(dims)
    dx = t["gamma"].view(sh) * t["invstd"].view(sh) * (dz - (s1 / n).view(sh) - xh * (s2 / n).view(sh))
    return dx, s2, s1


_BN_IN = ("x", "gamma", "beta", "rm", "rv")
for _shape in BN_SHAPES:
    _tag = "x".join(map(str, _shape))
    _mk = functools.partial(_bn_ops, _shape)
    _n = _shape[0] * _shape[2]
    _y = ("y",) if _shape[2] > 1 else ()
    case("bn_fwd training " + _tag, "bn_fwd", _mk,
         lambda K, t: K.bn_fwd(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], True, 1e-5, 0.1, 2, 0.2, residual=t["res"],
                               out=t.get("y")) + (t["rm"], t["rv"]),
         lambda t: _bn_train_ref(t, 2, True), _BN_IN + ("res",) + _y, ("rm", "rv") + _y,
         tol=[TOL_BN_FWD, TOL_POINT, TOL_BN_FWD, TOL_POINT, TOL_POINT])
    case("bn_fwd eval " + _tag, "bn_fwd", _mk,
         lambda K, t: (K.bn_fwd(t["x"], t["gamma"], t["beta"], t["rm"], t["rv"], False, 1e-5, 0.1, 1, 0.0, residual=t["res"])[0],),
         lambda t: (t["res"] + F.relu(F.batch_norm(t["x"], t["rm"], t["rv"], t["gamma"], t["beta"], False, 0.1, 1e-5)),),
         _BN_IN + ("res",), tol=TOL_BN_FWD)
    case("bn_stats " + _tag, "bn_stats", _mk, lambda K, t: (K.bn_stats(t["x"]),), lambda t: (t["sums"],), ("x",), tol=TOL_SUMS)
    case("bn_fwd_sums " + _tag, "bn_fwd_sums", _mk,
         lambda K, t, n=_n: K.bn_fwd_sums(t["x"], t["sums"], float(n), t["gamma"], t["beta"], t["rm"], t["rv"], 1e-5, 0.1, 2, 0.2,
                                          residual=t["res"], out=t.get("y")) + (t["rm"], t["rv"]),
         lambda t: _bn_train_ref(t, 2, True), _BN_IN + ("sums", "res") + _y, ("rm", "rv") + _y,
         tol=[TOL_BN_FWD, TOL_POINT, TOL_BN_FWD, TOL_POINT, TOL_POINT])
    case("bn_bwd " + _tag, "bn_bwd", _mk,
         lambda K, t: K.bn_bwd(t["dy"], t["x"], t["gamma"], t["beta"], t["mean"], t["invstd"], 0, 0.0),
         _bn_bwd_ref, ("dy", "x", "gamma", "beta", "mean", "invstd"), tol=TOL_BN_BWD)

    def _halves(K, t, n=_n):
        loc = K.bn_bwd_stats(t["dy"], t["x"], t["gamma"], t["beta"], t["mean"], t["invstd"], 0, 0.0)
        return (loc,) + tuple(K.bn_bwd_sums(t["dy"], t["x"], t["gamma"], t["beta"], t["mean"], t["invstd"], loc, loc, float(n), 0, 0.0))

    def _halves_ref(t):
        dims = (0,) if t["x"].dim() == 2 else (0, 2)
        dz, xh = _bn_dz(t)
        return (torch.stack((dz.sum(dims), (dz * xh).sum(dims)), 1).reshape(-1),) + tuple(_bn_bwd_ref(t))
    case("bn_bwd_stats + bn_bwd_sums " + _tag, ("bn_bwd_stats", "bn_bwd_sums"), _mk, _halves, _halves_ref,
         ("dy", "x", "gamma", "beta", "mean", "invstd"), tol=[TOL_SUMS, TOL_BN_BWD, TOL_BN_BWD, TOL_BN_BWD])
    case("channel_sums " + _tag, "channel_sums", lambda s=_shape: {"x": gen(*s, seed=1), "mask": gen(*s, seed=2)},
         lambda K, t: (K.channel_sums(t["x"]), K.channel_sums(t["x"], t["mask"], 0.2)),
         lambda t: (t["x"].sum((0, 2)), (t["x"] * mf(t["mask"], 0.2)).sum((0, 2))), ("x", "mask"), tol=TOL_SUMS)

# the fused forms: BatchNorm from sums with the following max-pool / upsampling made in the same pass
for _shape in [(5, 8, 50), (4, 6, 25)]:
    _tag = "x".join(map(str, _shape))
    _B, _C, _L = _shape
    _mk = functools.partial(lambda s: dict(_bn_ops(s), up=torch.zeros(s[0], s[1], 2 * s[2])), _shape)
    _up = lambda y: F.interpolate(y, scale_factor=2, mode="linear", align_corners=False)
    if _L % 2 == 0:
        case("bn_fwd_sums_pool " + _tag, "bn_fwd_sums_pool", _mk,
             lambda K, t, n=_B * _L: K.bn_fwd_sums_pool(t["x"], t["sums"], float(n), t["gamma"], t["beta"], t["rm"], t["rv"], 1e-5, 0.1,
                                                        2, 0.2, out=t["y"]) + (t["rm"], t["rv"]),
             lambda t: (lambda r: (r[0], F.max_pool1d(r[0], 2, 2)) + r[1:])(_bn_train_ref(t, 2, False)),
             _BN_IN + ("sums", "y"), ("rm", "rv", "y"),
             tol=[TOL_BN_FWD, TOL_BN_FWD, TOL_POINT, TOL_BN_FWD, TOL_POINT, TOL_POINT])
    case("bn_fwd_sums_upsample2 " + _tag, "bn_fwd_sums_upsample2", _mk,
         lambda K, t, n=_B * _L: K.bn_fwd_sums_upsample2(t["x"], t["sums"], float(n), t["gamma"], t["beta"], t["rm"], t["rv"], 1e-5,
                                                         0.1, 2, 0.2, out=t["up"]) + (t["rm"], t["rv"]),
         lambda t, up=_up: (lambda r: (up(r[0]),) + r[1:])(_bn_train_ref(t, 2, False)),
         _BN_IN + ("sums", "up"), ("rm", "rv", "up"), tol=[TOL_BN_FWD, TOL_POINT, TOL_BN_FWD, TOL_POINT, TOL_POINT])

case("bn_update_running", "bn_update_running", functools.partial(_bn_ops, (5, 8, 50)),
     lambda K, t: (K.bn_update_running(t["sums"], 250.0, t["rm"], t["rv"], 1e-5, 0.1), t["rm"], t["rv"])[1:],
     lambda t: _bn_train_ref(t, 0, False)[3:], ("sums", "rm", "rv"), ("rm", "rv"), tol=TOL_POINT)


# ------------------------------------------------------------------------------------------- pool, upsample, tanh (exact)
def _pool_bwd_ref(t):
    x = t["x"].clone().requires_grad_(True)
    return torch.autograd.grad(F.max_pool1d(x, 2, 2), x, t["dy"])


def _up_bwd_ref(t):
    x = torch.zeros(t["dy"].shape[0], t["dy"].shape[1], t["dy"].shape[2] // 2, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad(F.interpolate(x, scale_factor=2, mode="linear", align_corners=False), x, t["dy"])


for _shape in [(2, 4, 200), (4, 5, 25), (2, 3, 1)]:
    _tag = "x".join(map(str, _shape))
    _B, _C, _L = _shape
    if _L >= 2:
        case("maxpool2_fwd " + _tag, "maxpool2_fwd", lambda s=_shape: {"x": gen(*s, seed=1)},
             lambda K, t: (K.maxpool2_fwd(t["x"]),), lambda t: (F.max_pool1d(t["x"], 2, 2),), ("x",), tol=TOL_POINT, exact=True)
        case("maxpool2_bwd " + _tag, "maxpool2_bwd", lambda s=_shape: {"x": gen(*s, seed=1), "dy": gen(s[0], s[1], s[2] // 2, seed=2)},
             lambda K, t: (K.maxpool2_bwd(t["x"], t["dy"]),), _pool_bwd_ref, ("x", "dy"), tol=TOL_POINT, exact=True)
    case("upsample2_fwd " + _tag, "upsample2_fwd", lambda s=_shape: {"x": gen(*s, seed=1), "up": torch.zeros(s[0], s[1], 2 * s[2])},
         lambda K, t: (K.upsample2_fwd(t["x"], out=t["up"]),),
         lambda t: (F.interpolate(t["x"], scale_factor=2, mode="linear", align_corners=False),), ("x", "up"), ("up",),
         tol=TOL_POINT, exact=True)
    case("upsample2_bwd " + _tag, "upsample2_bwd", lambda s=_shape: {"dy": gen(s[0], s[1], 2 * s[2], seed=3)},
         lambda K, t: (K.upsample2_bwd(t["dy"]),), _up_bwd_ref, ("dy",), tol=TOL_POINT, exact=True)

for _n in (257, 25000):
    _mk = lambda n=_n: {"x": gen(n, seed=1, scale=2.0), "g": gen(n, seed=2), "gy": gen(n, seed=3), "y": torch.tanh(gen(n, seed=1, scale=2.0))}
    case("tanh_fwd %d" % _n, "tanh_fwd", _mk, lambda K, t: (K.tanh_fwd(t["x"]),), lambda t: (torch.tanh(t["x"]),), ("x",),
         tol=TOL_POINT, exact=True)
    case("tanh_bwd %d" % _n, "tanh_bwd", _mk, lambda K, t: (K.tanh_bwd(t["gy"], t["y"]),),
         lambda t: (t["gy"] * (1.0 - t["y"] * t["y"]),), ("gy", "y"), tol=TOL_POINT, exact=True)
    case("tanh_bwd_bwd %d" % _n, "tanh_bwd_bwd", _mk, lambda K, t: (K.tanh_bwd_bwd(t["g"], t["gy"], t["y"]),),
         lambda t: (-2.0 * t["y"] * t["g"] * t["gy"],), ("g", "gy", "y"), tol=TOL_POINT, exact=True)


# ------------------------------------------------------------------------------------------- gradient penalty, losses
def _gp_ops(n=8280, B=6):
    scale = torch.tensor([0.2, 0.9, 1.0, 1.1, 3.0, 0.5]).view(B, 1) / math.sqrt(n)
    g = gen(B, n, seed=4) * scale
    return {"real": gen(B, n, seed=1), "fake": gen(B, n, seed=2), "alpha": torch.rand(B, generator=torch.Generator().manual_seed(3)),
            "g": g, "norms": torch.sqrt((g.double() ** 2).sum(1) + 1e-12).float(), "gout": torch.tensor(0.7), "dg": torch.zeros(B, n)}


def _gp_pen(g, lp):
    if lp:
        norms = torch.sqrt((g * g).sum(1))
        d = (norms - 1).clamp_min(0)
    else:
        norms = torch.sqrt((g * g).sum(1) + 1e-12)
        d = norms - 1
    return (d * d).mean(), norms


def _gp_bwd_ref(t, lp):
    d = t["norms"] - 1
    if lp:
        d = d.clamp_min(0)
    coef = torch.where(d == 0, torch.zeros_like(d), t["gout"] * 2 * d / (t["norms"] * t["g"].shape[0]))
    return (coef.view(-1, 1) * t["g"],)


case("gp_interpolate", "gp_interpolate", _gp_ops, lambda K, t: (K.gp_interpolate(t["real"], t["fake"], t["alpha"]),),
     lambda t: (t["alpha"].view(-1, 1) * t["real"] + (1 - t["alpha"].view(-1, 1)) * t["fake"],), ("real", "fake", "alpha"),
     tol=TOL_POINT, exact=True)
for _lp in (False, True):
    case("gp_penalty_fwd lp=%d" % _lp, "gp_penalty_fwd", _gp_ops, lambda K, t, lp=_lp: K.gp_penalty_fwd(t["g"], lp),
         lambda t, lp=_lp: _gp_pen(t["g"], lp), ("g",), tol=1e-5)
    case("gp_penalty_bwd lp=%d" % _lp, "gp_penalty_bwd", _gp_ops,
         lambda K, t, lp=_lp: (K.gp_penalty_bwd(t["g"], t["norms"], t["gout"], lp, out=t["dg"]),),
         lambda t, lp=_lp: _gp_bwd_ref(t, lp), ("g", "norms", "gout", "dg"), ("dg",), tol=("max", 1e-5))

LB, LC, LT = 5, 69, 120


def _loss_ops():
    return {"a": gen(LB, LC, LT, seed=1), "b": gen(LB, LC, LT, seed=2), "rows": gen(LB * LT, LC, seed=3), "gout": torch.tensor(1.3)}


def _tv(t):
    v = t["rows"].view(LB, LT, LC).permute(0, 2, 1)
    return (v[:, :, 1:] - v[:, :, :-1]).abs().mean()


def _tv_bwd_ref(t):
    r = dict(t, rows=t["rows"].clone().requires_grad_(True))
    return (t["gout"] * torch.autograd.grad(_tv(r), r["rows"])[0],)


def _jerk(t):
    v = t["rows"].view(LB, LT, LC).permute(0, 2, 1)
    d = v[:, :, 3:] - 3 * v[:, :, 2:-1] + 3 * v[:, :, 1:-2] - v[:, :, :-3]
    return ((d ** 2).sum(dim=1).mean(),)


case("l1_mean_fwd", "l1_mean_fwd", _loss_ops, lambda K, t: (K.l1_mean_fwd(t["a"], t["b"]),),
     lambda t: ((t["a"] - t["b"]).abs().mean(),), ("a", "b"), tol=("abs", 1e-6))
case("l1_mean_bwd", "l1_mean_bwd", _loss_ops, lambda K, t: (K.l1_mean_bwd(t["a"], t["b"], t["gout"]),),
     lambda t: (t["gout"] * torch.sign(t["a"] - t["b"]) / t["a"].numel(),), ("a", "b", "gout"), tol=TOL_POINT, exact=True)
case("tv_mean_fwd", "tv_mean_fwd", _loss_ops, lambda K, t: (K.tv_mean_fwd(t["rows"], LB, LC, LT, LT * LC, 1, LC),),
     lambda t: (_tv(t),), ("rows",), tol=("abs", 1e-6))
case("tv_mean_bwd", "tv_mean_bwd", _loss_ops, lambda K, t: (K.tv_mean_bwd(t["rows"], t["gout"], LB, LC, LT, LT * LC, 1, LC),),
     _tv_bwd_ref, ("rows", "gout"), tol=("abs", 1e-9), exact=True)
case("jerk_mean_fwd", "jerk_mean_fwd", _loss_ops, lambda K, t: (K.jerk_mean_fwd(t["rows"], LB, LC, LT, LT * LC, 1, LC),),
     _jerk, ("rows",), tol=TOL_POINT)
case("affine_cols", "affine_cols", lambda: {"x": gen(77, 69, seed=1), "scale": gen(69, seed=2), "shift": gen(69, seed=3), "y": torch.zeros(77, 69)},
     lambda K, t: (K.affine_cols(t["x"], t["scale"], t["shift"], out=t["y"]),), lambda t: (t["x"] * t["scale"] + t["shift"],),
     ("x", "scale", "shift", "y"), ("y",), tol=TOL_POINT, exact=True)


def _wgan_ref(t):
    B = t["scores"].numel() // 3
    w = t["scores"][2 * B:].mean() - t["scores"][B:2 * B].mean()
    gp = t["p0"] + t["p1"]
    return torch.stack((w + 10.0 * gp,)), torch.stack((gp, w))


case("wgan_critic_loss", "wgan_critic_loss",
     lambda: {"scores": gen(111, seed=1), "p0": torch.rand((), generator=torch.Generator().manual_seed(2)),
              "p1": torch.rand((), generator=torch.Generator().manual_seed(3))},
     lambda K, t: (lambda o: (o[:1], o[1:]))(K.wgan_critic_loss(t["scores"], 37, t["p0"], t["p1"], 10.0)), _wgan_ref,
     ("scores", "p0", "p1"), tol=[("abs", 1e-5), ("abs", 1e-6)])


# ------------------------------------------------------------------------------------------- critic pack, labels, dropout
PB, PT, PC, PL, PD = 3, 33, 69, 10, 8


def _pack_ops():
    g = torch.Generator().manual_seed(PB)
    return {"real": torch.rand(PB, PT, PC, generator=g), "fake": torch.randn(PB * PT, PC, generator=g), "alpha": torch.rand(PB, generator=g),
            "E": torch.randn(PL, PD, generator=g), "rl": torch.randint(0, PL, (PB,), generator=g),
            "fl": torch.randint(0, PL, (PB,), generator=g), "o": torch.zeros(3 * PB, PC, PT), "ol": torch.zeros(3 * PB, PC + PD, PT),
            "xt": torch.randn(PB, PT, PC, generator=g), "xc": torch.randn(PB, PC, PT, generator=g),
            "ot": torch.zeros(PB, PT, PC + PD), "oc": torch.zeros(PB, PC + PD, PT),
            "dxt": torch.randn(3 * PB, PT, PC + PD, generator=g), "dxc": torch.randn(3 * PB, PC + PD, PT, generator=g),
            "lbl2": torch.randint(0, PL, (2 * PB,), generator=g), "dE": torch.zeros(PL, PD)}


def _pack_ref(t):
    a = t["alpha"].view(PB, 1, 1)
    fake = t["fake"].view(PB, PT, PC)
    return torch.cat((a * t["real"] + (1 - a) * fake, t["real"], fake), 0).permute(0, 2, 1).contiguous()


def _pack_label_ref(t):
    e = lambda l: t["E"][l].view(PB, PD, 1).expand(PB, PD, PT)
    return (torch.cat((_pack_ref(t), torch.cat((e(t["rl"]), e(t["rl"]), e(t["fl"])), 0)), 1),)


def _embed_bwd_ref(t, layout):
    r0, r1 = PB, 3 * PB
    dx = t["dxt"] if layout == 0 else t["dxc"].permute(0, 2, 1)
    rows = dx[r0:r1, :, PC:PC + PD].sum(1)
    return (torch.zeros(PL, PD, dtype=torch.float64).index_add_(0, t["lbl2"], rows),)


case("pose_pack3", "pose_pack3", _pack_ops, lambda K, t: (K.pose_pack3(t["real"], t["fake"], t["alpha"], out=t["o"]),),
     lambda t: (_pack_ref(t),), ("real", "fake", "alpha", "o"), ("o",), tol=TOL_POINT, exact=True)
case("pose_pack3_label", "pose_pack3_label", _pack_ops,
     lambda K, t: (K.pose_pack3_label(t["real"], t["fake"], t["alpha"], t["E"], t["rl"], t["fl"], out=t["ol"]),), _pack_label_ref,
     ("real", "fake", "alpha", "E", "rl", "fl", "ol"), ("ol",), tol=TOL_POINT, exact=True)
case("label_concat layout 0", "label_concat", _pack_ops, lambda K, t: (K.label_concat(t["xt"], t["E"], t["rl"], 0, out=t["ot"]),),
     lambda t: (torch.cat((t["xt"], t["E"][t["rl"]].view(PB, 1, PD).expand(PB, PT, PD)), 2),), ("xt", "E", "rl", "ot"), ("ot",),
     tol=TOL_POINT, exact=True)
case("label_concat layout 1", "label_concat", _pack_ops, lambda K, t: (K.label_concat(t["xc"], t["E"], t["rl"], 1, out=t["oc"]),),
     lambda t: (torch.cat((t["xc"], t["E"][t["rl"]].view(PB, PD, 1).expand(PB, PD, PT)), 1),), ("xc", "E", "rl", "oc"), ("oc",),
     tol=TOL_POINT, exact=True)
for _layout in (0, 1):
    case("label_embed_bwd layout %d" % _layout, "label_embed_bwd", _pack_ops,
         lambda K, t, lo=_layout: (K.label_embed_bwd(t["dxt" if lo == 0 else "dxc"], t["lbl2"], PB, 3 * PB, PC, PL, PD, lo, out=t["dE"]),),
         functools.partial(lambda lo, t: _embed_bwd_ref(t, lo), _layout), ("dxt" if _layout == 0 else "dxc", "lbl2", "dE"), ("dE",),
         tol=("abs", 1e-5))


def _drop_ops():
    g = torch.Generator().manual_seed(5)
    return {"x": torch.randn(7, 333, generator=g), "mask": (torch.rand(7, 333, generator=g) < 0.5).to(torch.uint8), "y": torch.zeros(7, 333)}


case("dropout given mask", "dropout", _drop_ops, lambda K, t: (K.dropout(t["x"], t["mask"], 0.5, 2.0, out=t["y"]),),
     lambda t: (t["x"] * t["mask"].double() * 2.0,), ("x", "mask", "y"), ("y",), tol=TOL_POINT, exact=True)


def _drop_seeded_extra(outs, t):
    y, mask = outs
    assert set(mask.unique().tolist()) <= {0, 1} and 0.4 < float(mask.float().mean()) < 0.6
    assert torch.equal(y, t["x"] * mask.float() * 2.0)


def _drop_seeded(K, t):
    y = K.dropout(t["x"], t["mask"], 0.5, 2.0, seed=1234, offset=7, out=t["y"])
    return y, t["mask"]


# (the Philox bits have no plain-torch twin: y against x * mask * scale of the mask the call wrote; bits by `exact`)
case("dropout seeded", "dropout", _drop_ops, _drop_seeded, lambda t: (None, None), ("x", "mask", "y"), ("mask", "y"), tol=TOL_POINT,
     exact=True, hip_only=True, extra=_drop_seeded_extra)
case("randn_frames", "randn_frames", lambda: {"o": torch.zeros(3, 17, 10)},
     lambda K, t: (K.randn_frames(99, 5, 3, 17, 10, t["o"].device, out=t["o"]),), lambda t: (None,), ("o",), ("o",), exact=True,
     hip_only=True)


# ------------------------------------------------------------------------------------------- BCE on logits, cross entropy
def _bce_ops():
    return {"x": gen(24 + 49, seed=1, scale=3.0), "gout": torch.tensor(2.5)}


def _bce_ref(t):
    x = t["x"].clone().requires_grad_(True)
    l0 = F.binary_cross_entropy_with_logits(x[:24], torch.full((24,), 1.0, dtype=x.dtype))
    l1 = F.binary_cross_entropy_with_logits(x[24:], torch.full((49,), 0.3, dtype=x.dtype))
    (dx,) = torch.autograd.grad(l0 + l1, x)
    return torch.stack((l0 + l1, l0, l1)).detach(), dx


case("bce_logits_fwd", "bce_logits_fwd", _bce_ops, lambda K, t: K.bce_logits_fwd(t["x"], 24, 1.0, 49, 0.3, with_dx=True), _bce_ref,
     ("x",), tol=[("allclose", 1e-6, 1e-30), ("max", 1e-6)])
case("bce_logits_bwd", "bce_logits_bwd", _bce_ops, lambda K, t: (K.bce_logits_bwd(t["x"], 24, 1.0, 49, 0.3, t["gout"]),),
     lambda t: (2.5 * _bce_ref(t)[1],), ("x", "gout"), tol=("max", 1e-6))


def _ce_ops():
    g = torch.Generator().manual_seed(7)
    return {"logits": torch.randn(49, 10, generator=g) * 3.0, "labels": torch.randint(0, 10, (49,), generator=g), "gout": torch.tensor(0.7)}


def _ce_bwd_ref(t):
    x = t["logits"].clone().requires_grad_(True)
    return (0.7 * torch.autograd.grad(F.cross_entropy(x, t["labels"]), x)[0],)


case("cross_entropy_fwd", "cross_entropy_fwd", _ce_ops, lambda K, t: K.cross_entropy_fwd(t["logits"], t["labels"], with_pred=True),
     lambda t: (F.cross_entropy(t["logits"], t["labels"]), t["logits"].argmax(1)), ("logits", "labels"), tol=[1e-5, None])
case("cross_entropy_bwd", "cross_entropy_bwd", _ce_ops, lambda K, t: (K.cross_entropy_bwd(t["logits"], t["labels"], t["gout"]),),
     _ce_bwd_ref, ("logits", "labels", "gout"), tol=("max", 1e-5))


# -------------------------------------------------------------------------------------------------------------- Adam
ADAM = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8)
ADAM_TOL = [("allclose", 2e-6, 2e-7), ("max", 1e-6), ("max", 3e-5)]   # parameters, exp_avg, exp_avg_sq (tests/test_optim.py)
ADAM_SHAPES = [(128, 69, 25), (128,), (128, 128, 7), (128,), (100, 12800), (1, 128), (3,), (5000, 33), (64, 32, 4)]


def adam_ref(p, g, m, v, step=1, lr=ADAM["lr"]):
    """torch.optim.Adam's step in fp64 -> (p, m, v)"""
    m = m + (g - m) * (1.0 - ADAM["b1"])
    v = v * ADAM["b2"] + g * g * (1.0 - ADAM["b2"])
    bc1, bc2s = 1.0 - ADAM["b1"] ** step, math.sqrt(1.0 - ADAM["b2"] ** step)
    return p - (lr / bc1) * (m / (v.sqrt() / bc2s + ADAM["eps"])), m, v


def _adam_flat_ops():
    """the parameter list of tests/test_optim.py::_params; the gradients as dp.py lays a bucket out: ONE flat buffer, end
    to end - everything behind the (1, 128) and (3,) tensors starts off 16 bytes even when the buffer itself does not"""
    g = torch.Generator().manual_seed(0)
    ps = [torch.randn(s, generator=g) for s in ADAM_SHAPES]
    flat = torch.cat([torch.randn(p.numel(), generator=g) * 10.0 ** (i % 3 - 1) for i, p in enumerate(ps)])
    return dict({"p%d" % i: p for i, p in enumerate(ps)}, flat=flat)


def _adam_flat_run(K, t):
    from music2dance_amd import kernels
    from music2dance_amd.optim import Adam
    ps = [t["p%d" % i] for i in range(len(ADAM_SHAPES))]
    for p in ps:
        p.requires_grad_(True)
    off = 0
    for p in ps:
        p.grad = t["flat"][off:off + p.numel()].view(p.shape)
        off += p.numel()
    prev = kernels.set_impl(K)
    try:
        opt = Adam(ps, lr=ADAM["lr"])
        opt.step()
    finally:
        kernels.set_impl(prev)
    out = [p.detach() for p in ps] + [opt.state[p]["exp_avg"] for p in ps] + [opt.state[p]["exp_avg_sq"] for p in ps]
    for p in ps:
        p.grad = None
        p.requires_grad_(False)
    return tuple(out)


def _adam_flat_ref(t):
    ps = [t["p%d" % i] for i in range(len(ADAM_SHAPES))]
    res, off = [], 0
    for p in ps:
        g = t["flat"][off:off + p.numel()].view(p.shape)
        off += p.numel()
        res.append(adam_ref(p, g, torch.zeros_like(p), torch.zeros_like(p)))
    return tuple(r[0] for r in res) + tuple(r[1] for r in res) + tuple(r[2] for r in res)


_NP = len(ADAM_SHAPES)
case("adam_multi through optim.Adam, bucket-laid gradients", "adam_multi", _adam_flat_ops, _adam_flat_run, _adam_flat_ref,
     tuple("p%d" % i for i in range(_NP)) + ("flat",), tuple("p%d" % i for i in range(_NP)),
     tol=[ADAM_TOL[0]] * _NP + [ADAM_TOL[1]] * _NP + [ADAM_TOL[2]] * _NP, exact=True)


def _adam_one_ops(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return {"p": torch.randn(shape, generator=g), "g": torch.randn(shape, generator=g), "m": torch.randn(shape, generator=g) * 0.1,
            "v": torch.rand(shape, generator=g) * 0.01}


def _adam_one_run(K, t):
    K.adam_multi([t["p"]], [t["g"]], [t["m"]], [t["v"]], ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], 3)
    return t["p"], t["m"], t["v"]


case("adam_multi one tensor", "adam_multi", functools.partial(_adam_one_ops, (100, 36, 7), 3), _adam_one_run,
     lambda t: adam_ref(t["p"], t["g"], t["m"], t["v"], step=3), ("p", "g", "m", "v"), ("p", "m", "v"), tol=ADAM_TOL, exact=True)


def _adam_packed_run(K, t):
    """a conv weight with LIVE packed images: the tile mode on aligned tensors, the one-element path (images as scattered
    stores) on anything else - parameters, moments and both images"""
    with K.weight_cache():
        K.packed_weights(t["p"])
        launches = K.pack_launches
        K.adam_multi([t["p"]], [t["g"]], [t["m"]], [t["v"]], ADAM["lr"], ADAM["b1"], ADAM["b2"], ADAM["eps"], 3)
        K.invalidate_packed([t["p"]])
        wf, wb = K.packed_weights(t["p"])
        assert K.pack_launches == launches, "the step did not keep the packed images"
        return t["p"], t["m"], t["v"], wf.clone(), wb.clone()


def _adam_packed_extra(outs, t):
    p, _, _, wf, wb = outs
    assert torch.equal(wf, p.permute(1, 2, 0).contiguous()) and torch.equal(wb, p.permute(0, 2, 1).contiguous())


def _adam_packed_ref(t):
    p, m, v = adam_ref(t["p"], t["g"], t["m"], t["v"], step=3)
    return p, m, v, None, None     # (the images: the GPU test holds them equal to the permuted parameter it got)


case("adam_multi weight with live packed images", "adam_multi", functools.partial(_adam_one_ops, (64, 32, 25), 4), _adam_packed_run,
     _adam_packed_ref, ("p", "g", "m", "v"), ("p", "m", "v"), tol=ADAM_TOL + [None, None], exact=True, hip_only=True,
     extra=_adam_packed_extra)


# --------------------------------------------------------------------------------------------------------------- GRU
# (B, T, H, layers): the MFMA kernels at H = 240 (16-byte row loads) and the small-H kernel's range at H = 12
GRU_DIMS = {"h12": (5, 8, 12, 2), "h240": (3, 6, 240, 2)}


def _gru_ops(tag):
    B, T, H, L = GRU_DIMS[tag]
    sc = 1.0 / math.sqrt(H)
    t = {"gi": gen(B, T, 3 * H, seed=1), "dout": gen(B, T, H, seed=9), "dhn": gen(B, H, seed=10)}
    for l in range(L):
        t["w_hh%d" % l] = gen(3 * H, H, seed=20 + l, scale=sc)
        t["w_ih%d" % l] = gen(3 * H, H, seed=30 + l, scale=sc)
        # (the forward kernels read W^T: the caller supplies it - kernels.transposed would hand back an aligned copy)
        t["w_hht%d" % l], t["w_iht%d" % l] = t["w_hh%d" % l].t().contiguous(), t["w_ih%d" % l].t().contiguous()
        t["b_hh%d" % l] = gen(3 * H, seed=40 + l, scale=0.1)
        t["b_ih%d" % l] = gen(3 * H, seed=50 + l, scale=0.1)
        t["h0_%d" % l] = gen(B, H, seed=60 + l, scale=0.5)
    return t


def _gru_layer(gi, w_hh, b_hh, h0=None):
    """one layer in plain torch ops -> out (B, T, H); differentiable"""
    B, T, H3 = gi.shape
    H = H3 // 3
    h = gi.new_zeros(B, H) if h0 is None else h0
    outs = []
    for s in range(T):
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, s, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, s, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, s, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        outs.append(h)
    return torch.stack(outs, 1)


def _gru_grads(t, with_hn):
    """(dgi, dgh) of layer 0 alone: dgh by a zero probe added to every step's W_hh h + b_hh"""
    B, T, H3 = t["gi"].shape
    H = H3 // 3
    gi = t["gi"].clone().requires_grad_(True)
    probe = torch.zeros(B, T, H3, dtype=torch.float64, requires_grad=True)
    h = gi.new_zeros(B, H)
    outs = []
    for s in range(T):
        gh = h @ t["w_hh0"].t() + t["b_hh0"] + probe[:, s]
        r = torch.sigmoid(gi[:, s, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, s, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, s, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        outs.append(h)
    out = torch.stack(outs, 1)
    loss = (out * t["dout"]).sum() + ((h * t["dhn"]).sum() if with_hn else 0.0)
    return torch.autograd.grad(loss, (gi, probe))


for _tag in GRU_DIMS:
    _mk = functools.partial(_gru_ops, _tag)
    _L = GRU_DIMS[_tag][3]

    def _layer_fwd(K, t):
        out, saved = K.gru_layer_fwd(t["gi"], t["w_hht0"], t["b_hh0"])
        return (out,)

    def _layer_bwd(K, t):
        out, saved = K.gru_layer_fwd(t["gi"], t["w_hht0"], t["b_hh0"])
        return tuple(K.gru_layer_bwd(t["dout"], out, saved, t["w_hh0"]))
    case("gru_layer_fwd " + _tag, "gru_layer_fwd", _mk, _layer_fwd, lambda t: (_gru_layer(t["gi"], t["w_hh0"], t["b_hh0"]),),
         ("gi", "w_hht0", "b_hh0"), tol=TOL_GRU)
    case("gru_layer_bwd " + _tag, "gru_layer_bwd", _mk, _layer_bwd, lambda t: _gru_grads(t, False),
         ("gi", "w_hht0", "w_hh0", "b_hh0", "dout"), tol=2e-5)

    def _stack_args(K, t, L=_L):
        w_ih_t = [None] + [t["w_iht%d" % l] for l in range(1, L)]
        b_ih = [None] + [t["b_ih%d" % l] for l in range(1, L)]
        w_hh_t = [t["w_hht%d" % l] for l in range(L)]
        return w_ih_t, b_ih, w_hh_t, [t["b_hh%d" % l] for l in range(L)], [t["h0_%d" % l] for l in range(L)]

    def _stack_fwd(K, t, persistent):
        w_ih_t, b_ih, w_hh_t, b_hh, h0 = _stack_args(K, t)
        outs, saved, h_n = K.gru_stack_fwd(t["gi"], w_ih_t, b_ih, w_hh_t, b_hh, persistent=persistent, h0=h0, want_state=True)
        return tuple(outs) + (h_n,)

    def _stack_fwd_ref(t, L=_L):
        outs, x = [], None
        for l in range(L):
            gi = t["gi"] if l == 0 else x @ t["w_ih%d" % l].t() + t["b_ih%d" % l]
            x = _gru_layer(gi, t["w_hh%d" % l], t["b_hh%d" % l], t["h0_%d" % l])
            outs.append(x)
        return tuple(outs) + (torch.stack([o[:, -1] for o in outs], 0),)

    def _stack_bwd(K, t, persistent, L=_L):
        w_ih_t, b_ih, w_hh_t, b_hh, _ = _stack_args(K, t)
        outs, saved = K.gru_stack_fwd(t["gi"], w_ih_t, b_ih, w_hh_t, b_hh, persistent=persistent)
        dgi, dgh = K.gru_stack_bwd(t["dout"], outs, saved, [t["w_hh%d" % l] for l in range(L)],
                                   [None] + [t["w_ih%d" % l] for l in range(1, L)], persistent=persistent)
        return tuple(dgi) + tuple(dgh)

    def _stack_bwd_ref(t, L=_L):
        B, T, H3 = t["gi"].shape
        H = H3 // 3
        gi0 = t["gi"].clone().requires_grad_(True)
        probes = [torch.zeros(B, T, H3, dtype=torch.float64, requires_grad=True) for _ in range(L)]
        gis, x = [], None
        for l in range(L):
            gi = gi0 if l == 0 else x @ t["w_ih%d" % l].t() + t["b_ih%d" % l]
            gi.retain_grad() if l else None
            gis.append(gi)
            h, outs = gi.new_zeros(B, H), []
            for s in range(T):
                gh = h @ t["w_hh%d" % l].t() + t["b_hh%d" % l] + probes[l][:, s]
                r = torch.sigmoid(gi[:, s, :H] + gh[:, :H])
                z = torch.sigmoid(gi[:, s, H:2 * H] + gh[:, H:2 * H])
                n = torch.tanh(gi[:, s, 2 * H:] + r * gh[:, 2 * H:])
                h = (1 - z) * n + z * h
                outs.append(h)
            x = torch.stack(outs, 1)
        return torch.autograd.grad((x * t["dout"]).sum(), gis + probes)

    _fwd_names = ("gi",) + tuple("%s%d" % (n, l) for n in ("w_hht", "b_hh", "h0_") for l in range(_L)) + \
        tuple("%s%d" % (n, l) for n in ("w_iht", "b_ih") for l in range(1, _L))
    _bwd_names = tuple(n for n in _fwd_names if not n.startswith("h0_")) + ("dout",) + tuple("w_hh%d" % l for l in range(_L)) + \
        tuple("w_ih%d" % l for l in range(1, _L))
    for _pers in (True, False):
        _ptag = " persistent" if _pers else " step launches"
        case("gru_stack_fwd " + _tag + _ptag, "gru_stack_fwd", _mk, functools.partial(_stack_fwd, persistent=_pers), _stack_fwd_ref,
             _fwd_names, tol=TOL_GRU)
        case("gru_stack_bwd " + _tag + _ptag, "gru_stack_bwd", _mk, functools.partial(_stack_bwd, persistent=_pers), _stack_bwd_ref,
             _bwd_names, tol=2e-5)

# the one-launch layer for 1 <= H <= 16
case("gru_small_fwd h12", "gru_small_fwd", functools.partial(_gru_ops, "h12"),
     lambda K, t: K.gru_small_fwd(t["gi"], t["w_hh0"], t["b_hh0"])[:2],
     lambda t: (lambda o: (o, o[:, -1]))(_gru_layer(t["gi"], t["w_hh0"], t["b_hh0"])), ("gi", "w_hh0", "b_hh0"), tol=TOL_GRU)


def _small_bwd(K, t):
    out, h_n, saved = K.gru_small_fwd(t["gi"], t["w_hh0"], t["b_hh0"])
    return tuple(K.gru_small_bwd(t["dout"], t["dhn"], out, saved, t["w_hh0"]))


case("gru_small_bwd h12", "gru_small_bwd", functools.partial(_gru_ops, "h12"), _small_bwd, lambda t: _gru_grads(t, True),
     ("gi", "w_hh0", "b_hh0", "dout", "dhn"), tol=2e-5)


# ------------------------------------------------------------------------------------------- metrics and tools
# Each at the smallest shape of its own GPU test, against the fp64 numpy statement that test uses (tests/beat_cases.py,
# sync_cases.py, knn_cases.py, distribution_cases.py, render_rule.py) and inside that test's own bound. These kernels
# are deterministic and read their inputs a float at a time: every placement must give the aligned call's bits.
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _n(t):
    return t.detach().cpu().numpy()


def _each(bound_of_ref):
    """|got - ref| <= bound elementwise, bound a function of the reference (NaN in the same places)"""
    def tol(got, ref):
        g, r = _n(got), _n(ref)
        b = bound_of_ref(r)
        if not np.array_equal(np.isnan(g), np.isnan(r)):
            return False, float("inf")
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        bb = np.broadcast_to(b, r.shape)[ok]
        fig = float((err / np.where(bb > 0, bb, 1.0)).max()) if err.size else 0.0
        return bool((err <= bb).all()), fig
    return tol


STFT = (256, 100, 17, 20)     # n_fft, hop, frames, bands: frame 0 starts before the 1500 samples, the last ones end behind them


def _stft_ops():
    from music2dance_amd import metrics
    from tests import beat_cases as C
    n_fft, hop, T, nb = STFT
    return {"x": _t((0.5 * np.random.default_rng(11).standard_normal((2, 1500))).astype(np.float32)),
            "bands": _t(C.mel_bands(nb, n_fft, C.RATE).astype(np.float32)), "table": _t(metrics.stft_table(n_fft))}


def _stft_run(K, t):
    n_fft, hop, T, nb = STFT
    return (K.stft_bands(t["x"], T, hop, n_fft, K.stft_pack_basis(t["table"]), t["bands"]),)


def _stft_ref(t):
    from tests import beat_cases as C
    n_fft, hop, T, nb = STFT
    return (_t(C.band_energies(_n(t["x"]), T, hop, n_fft, _n(t["bands"]))),)


def _stft_tol(got, ref):
    """tests/test_gpu_beat.py: relative to the row's largest energy, min(1e-4, 32 x the error of an fp32 numpy evaluation)"""
    from tests import beat_cases as C
    n_fft, hop, T, nb = STFT
    ops = _stft_ops()
    E64 = _n(ref)
    E32 = C.band_energies(_n(ops["x"]), T, hop, n_fft, _n(ops["bands"]), dtype=np.float32).astype(np.float64)
    rowmax = E64.reshape(len(E64), -1).max(axis=1)[:, None, None]
    e32 = float((np.abs(E32 - E64) / rowmax).max())
    err = float((np.abs(_n(got) - E64) / rowmax).max())
    return e32 > 0 and err <= min(1e-4, 32.0 * e32), err


case("stft_bands", "stft_bands", _stft_ops, _stft_run, _stft_ref, ("x", "bands"), tol=_stft_tol, exact=True)


def _onset_ops():
    E = (np.random.default_rng(21).random((3, 50, 40)) * 1e4).astype(np.float32)
    E[1, 17] = 0.0
    return {"E": _t(E)}


def _curve_ops():
    from tests import beat_cases as C
    o, v = C.curves(5, 64)
    return {"o": _t(o.astype(np.float32)), "v": _t(v.astype(np.float32))}


def _smooth_tol(key, sigma, ulps):
    """tests/test_gpu_beat.py / test_gpu_sync.py: ulps x 2^-24 x (sum w |c| / sum w) per element"""
    def tol(got, ref):
        from tests import beat_cases as C
        mag = C.smooth(_n(_curve_ops()[key]).astype(np.float64), sigma)[1]
        return _each(lambda r: ulps * 2.0 ** -24 * mag)(got, ref)
    return tol


def _beat_ref(t):
    from tests import beat_cases as C
    r = C.alignment(_n(t["o"]), _n(t["v"]))
    return None, None, None, _t(r["osm"]), _t(r["vsm"])    # (scores and events: ties decide them - held by `exact`)


def _beat_extra(outs, t):
    """the scores are the formula on the device's OWN event masks (tests/test_gpu_beat.py: bound 1e-5)"""
    from tests import beat_cases as C
    scores, K_, M_ = _n(outs[0]).astype(np.float64), _n(outs[1]).astype(bool), _n(outs[2]).astype(bool)
    own = C.scores_from_masks(K_, M_, 2.0)
    assert np.array_equal(scores[:, 2], K_.sum(axis=1)) and np.array_equal(scores[:, 3], M_.sum(axis=1))
    ok = ~np.isnan(own[:, 0])
    assert np.array_equal(np.isnan(scores[:, 0]), ~ok) and (not ok.any() or np.abs(scores[ok, :2] - own[ok, :2]).max() <= 1e-5)


def _speed_ops():
    from tests import beat_cases as C
    return {"p": _t(C.dance(7, (0, 0, 0))[:, :20])}


case("onset_flux", "onset_flux", _onset_ops, lambda K, t: (K.onset_flux(t["E"], 1.0),),
     lambda t: (_t(__import__("tests.beat_cases", fromlist=["x"]).onset(_n(t["E"]), 1.0)),), ("E",), tol=("abs", 1e-5), exact=True)
case("motion_speed", "motion_speed", _speed_ops, lambda K, t: (K.motion_speed(t["p"]),),
     lambda t: (_t(__import__("tests.beat_cases", fromlist=["x"]).speed(_n(t["p"]))),), ("p",),
     tol=_each(lambda r: 1e-6 * r.max(axis=1, keepdims=True)), exact=True)
case("beat_align", "beat_align", _curve_ops, lambda K, t: K.beat_align(t["o"], t["v"], return_events=True), _beat_ref, ("o", "v"),
     tol=[None, None, None, _smooth_tol("o", 1.0, 2 * 3 + 4), _smooth_tol("v", 2.0, 2 * 6 + 4)], exact=True,
     extra=_beat_extra)
case("gauss_smooth", "gauss_smooth", _curve_ops, lambda K, t: (K.gauss_smooth(t["v"], 2.0),),
     lambda t: (_t(__import__("tests.beat_cases", fromlist=["x"]).smooth(_n(t["v"]), 2.0)[0]),), ("v",),
     tol=_smooth_tol("v", 2.0, 2.0), exact=True)

SYNC_L, SYNC_MIN = 8, 2


def _sync_ops():
    from tests import sync_cases as S
    a, b = S.uniform_curves(164, 3, 64, 40, extra=0)
    return {"a": _t(a), "b": _t(b), "na": torch.tensor([64, 62, 0], dtype=torch.int32), "nb": torch.tensor([40, 37, 40], dtype=torch.int32)}


def _sync_ref(t):
    from tests import sync_cases as S
    r, n = S.profile(_n(t["a"]), _n(t["b"]), S.FACTORS, SYNC_L, SYNC_MIN, _n(t["na"]), _n(t["nb"]))
    return _t(r), _t(n)


def _sync_tol(got, ref):
    """tests/test_gpu_sync.py: |r - r64| <= 64 (n + 8) 2^-53 per defined cell, NaN in the same cells"""
    n64 = _n(_sync_ref({k: (v.double() if v.dtype == torch.float32 else v) for k, v in _sync_ops().items()})[1])
    return _each(lambda r: 64.0 * (n64 + 8.0) * 2.0 ** -53)(got, ref)


case("sync_scan", "sync_scan", _sync_ops,
     lambda K, t: K.sync_scan(t["a"], t["b"], __import__("tests.sync_cases", fromlist=["x"]).FACTORS, SYNC_L, SYNC_MIN, t["na"], t["nb"]),
     _sync_ref, ("a", "b", "na", "nb"), tol=[_sync_tol, None], exact=True)

KNN_N, KNN_M, KNN_D, KNN_K = 40, 33, 3, 1


def _knn_ops():
    from tests import knn_cases as Kc
    R, Fq = Kc.split_case(KNN_N, KNN_M, KNN_D)
    return {"P": _t(R), "Q": _t(Fq), "r2": _t(Kc.radii(R, KNN_K).astype(np.float32))}


def _knn_eps(r):
    return (KNN_D + 4) * 2.0 ** -24 * np.abs(r)       # tests/knn_cases.py: eps(D), relative


case("knn_radii", "knn_radii", _knn_ops, lambda K, t: (K.knn_radii(t["P"], KNN_K),),
     lambda t: (_t(__import__("tests.knn_cases", fromlist=["x"]).radii(_n(t["P"]), KNN_K)),), ("P",), tol=_each(_knn_eps), exact=True)
# (count lies between the pairs decided inside and the pairs possibly inside at that bound, nn_idx is any index within the
# bound of the minimum - tests/test_gpu_knn.py; here both are held by `exact`, the minimum itself by the bound)
case("ball_query", "ball_query", _knn_ops, lambda K, t: K.ball_query(t["Q"], t["P"], t["r2"]),
     lambda t: (None, _t(__import__("tests.knn_cases", fromlist=["x"]).ball(_n(t["Q"]), _n(t["P"]))[1]), None), ("Q", "P", "r2"),
     tol=[None, _each(_knn_eps), None], exact=True)


def _dist_ops():
    from tests import distribution_cases as C
    X1, X2 = C.fd_pair((33, 17, 2, "full"))
    (m1, S1), (m2, S2) = C.moments(X1), C.moments(X2)
    return {"p": _t(C.random_walk(44, 12)), "X": _t(C.gaussian(1234, 33, 5)), "A": _t(np.stack([C.sym_matrix(5, "psd"), C.sym_matrix(5, "indefinite")])),
            "m1": _t(m1[None]), "S1": _t(S1[None]), "m2": _t(m2[None]), "S2": _t(S2[None])}


def _dc():
    from tests import distribution_cases as C
    return C


def _moments_tol(power, bound):
    def tol(got, ref):
        mx = float(np.abs(_n(_dist_ops()["X"])).max())
        return _each(lambda r: bound * mx ** power)(got, ref)
    return tol


def _eig_tol(got, ref):
    """tests/test_gpu_distribution.py: max|w - eigvalsh| / |A|_F <= 1e-11"""
    A = _n(_dist_ops()["A"])
    return _each(lambda r: 1e-11 * np.sqrt((A * A).sum(axis=(1, 2)))[:, None])(got, ref)


def _eig_extra(outs, t):
    w, V, info = (_n(o) for o in outs)
    A = _n(t["A"])
    for i in range(len(A)):
        nrm = np.sqrt((A[i] * A[i]).sum())
        assert info[i, 1] == 1.0 and np.abs(V[i].T @ V[i] - np.eye(A.shape[1])).max() <= 1e-12
        assert np.abs(A[i] @ V[i] - V[i] * w[i]).max() / nrm <= 1e-11


def _fd_ref(t):
    C = _dc()
    X1, X2 = C.fd_pair((33, 17, 2, "full"))
    fd, scale = C.fd_svd(X1, X2)
    dmu, tr = C.fd_terms(_n(t["m1"])[0], _n(t["S1"])[0], _n(t["m2"])[0], _n(t["S2"])[0])
    return (_t(np.array([[fd, dmu, tr]])),)


def _fd_tol(got, ref):
    """|fd - fd_svd| <= fd_bound x scale; the two cheap terms to 1e-13 of the scale (tests/test_gpu_distribution.py)"""
    r = _n(ref)
    scale = r[0, 1] + r[0, 2]
    return _each(lambda _: np.array([[_dc().fd_bound("full", 2), 1e-13, 1e-13]]) * scale)(got, ref)


case("kinetic_features", "kinetic_features", _dist_ops, lambda K, t: (K.kinetic_features(t["p"], 25.0, 1),),
     lambda t: (_t(_dc().kinetic(_n(t["p"]), 25.0, 1)),), ("p",), tol=_each(lambda r: 32.0 * 2.0 ** -24 * np.abs(r)), exact=True)
case("feature_moments", "feature_moments", _dist_ops, lambda K, t: K.feature_moments(t["X"]),
     lambda t: tuple(_t(a) for a in _dc().moments(_n(t["X"]))), ("X",), tol=[_moments_tol(1, 2.0 ** -50), _moments_tol(2, 1e-12)],
     exact=True)
case("sym_eig", "sym_eig", _dist_ops, lambda K, t: K.sym_eig(t["A"], vectors=True),
     lambda t: (_t(np.linalg.eigvalsh(_n(t["A"]))), None, None), ("A",), tol=[_eig_tol, None, None], exact=True,
     extra=_eig_extra)
case("frechet", "frechet", _dist_ops, lambda K, t: (K.frechet(t["m1"], t["S1"], t["m2"], t["S2"])[:, :3],), _fd_ref,
     ("m1", "S1", "m2", "S2"), tol=_fd_tol, exact=True)
case("pairwise_mean_dist", "pairwise_mean_dist", _dist_ops, lambda K, t: (K.pairwise_mean_dist(t["X"], 3),),
     lambda t: (_t(_dc().pairwise(_n(t["X"]), 3)),), ("X",), tol=_each(lambda r: (5 + 4) * 2.0 ** -24 * np.abs(r)), exact=True)

RS_UP, RS_DOWN, RS_NX, RS_TAPS = 3, 2, 300, 31


def _rs_ops():
    rng = np.random.default_rng(31)
    return {"x": _t(rng.standard_normal((2, RS_NX)).astype(np.float32)), "taps": _t((rng.standard_normal(RS_TAPS) / RS_TAPS).astype(np.float32)),
            "y": torch.zeros(2, RS_NX * RS_UP // RS_DOWN)}


def _rs_matrix(taps):
    """W[n, m] = taps[n down + half - m up] (include/m2d.h: m2d_resample_poly), zero outside the filter"""
    ny = RS_NX * RS_UP // RS_DOWN
    k = np.arange(ny)[:, None] * RS_DOWN + RS_TAPS // 2 - np.arange(RS_NX)[None, :] * RS_UP
    return np.where((k >= 0) & (k < RS_TAPS), taps[np.clip(k, 0, RS_TAPS - 1)], 0.0)


def _rs_tol(got, ref):
    """tests/test_gpu_resample.py: (P + 3) 2^-24 sum |taps| |x|, P the terms of an output"""
    ops = _rs_ops()
    R = np.abs(_n(ops["x"]).astype(np.float64)) @ np.abs(_rs_matrix(_n(ops["taps"]).astype(np.float64))).T
    return _each(lambda r: (-(-RS_TAPS // RS_UP) + 3) * 2.0 ** -24 * R)(got, ref)


case("resample_poly", "resample_poly", _rs_ops,
     lambda K, t: (K.resample_poly(t["x"], 0, t["taps"], RS_UP, RS_DOWN, 0, t["y"].shape[1], out=t["y"]),),
     lambda t: (_t(_n(t["x"]) @ _rs_matrix(_n(t["taps"])).T),), ("x", "taps", "y"), ("y",), tol=_rs_tol, exact=True, hip_only=True)


def _render_ops():
    poses = np.random.default_rng(21).uniform(-30.0, 30.0, size=(5, 23, 3)).astype(np.float32)
    return {"poses": _t(poses), "fb": torch.zeros(5, 37, 50, 3, dtype=torch.uint8)}


# (`fb` is a byte buffer: its placements are 1, 4 and 15 BYTES past a 16-byte boundary)
case("render_sticks", "render_sticks", _render_ops, lambda K, t: (K.render_sticks(t["poses"], 37, 50, out=t["fb"]),),
     lambda t: (_t(__import__("tests.render_rule", fromlist=["x"]).render(_n(t["poses"]).astype(np.float32), 37, 50)),), ("poses", "fb"),
     ("fb",), tol=None, exact=True, hip_only=True)


# ----------------------------------------------------------------------------------------------------- exemptions
EXEMPT = {
    "jpeg_encode": "uint8 frames at every byte offset: tests/test_gpu_jpeg.py::test_input_alignment",
    "fault_fetch": "one float written by one lane",
    "packed_weights": "weight-cache method: reads w a float at a time, writes images the library owns",
    "packed_k4": "weight-cache method: as packed_weights",
    "transposed": "weight-cache method: a torch transpose",
    "invalidate_packed": "weight-cache bookkeeping, no launch",
    "stft_pack_basis": "writes the library-owned basis image (its 16-byte alignment is stated in include/m2d.h); runs inside the stft_bands case",
}
