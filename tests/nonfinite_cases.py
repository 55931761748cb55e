"""Non-finite values through the fused epilogues: the case table the GPU test (test_gpu_nonfinite.py) and the host test
(test_nonfinite_host.py) share, and the one checker both use. A helper, not a test module; it imports no GPU code.

The contract: every fused activation gives what torch.nn.functional gives on the same fp32 value - a
NaN stays a NaN and +inf stays +inf for every `act`, -inf becomes 0 under ReLU and stays -inf otherwise. The sign of a
zero is not part of it (the checker compares with ==).

A case builds seeded inputs, plants ONE poison value (NaN, +inf or -inf; NaN only where a 0 / 1 mask multiplies) at one
position, and states the expectation in plain fp64 torch CPU ops: F.conv1d, @, F.batch_norm, F.relu, F.leaky_relu,
masks as `* torch.where(mask > 0, 1, slope)`, residuals as `+ res`, gradients by autograd of those ops. The positions:

  x_first / x_last   the first element of the input / the last element of the last row that a window reads (with
                     stride 4 the rows of wg.l1 end in three samples no output sees); with padding both touch it
  x_pad              element 1 of a row in a middle sample: its receptive field reaches into the zero padding (cases
                     with pad > 0 only)
  x_mid              the element one past the window of output (L / 2) / stride, in a middle sample: that output is
                     outside its receptive field, but a kernel that pads its tap count with zero weights (the phantom
                     odd tap of thin_fwd_mfma_kernel) reads exactly this element for it - "0 x inf" must not leak
  w                  one weight element: one output channel (forward), one input channel (backward-data)
  b                  one bias element: one output channel
  dy_*               backward passes: one element of the incoming gradient (under a mask: one whose mask is > 0)

Why neither half of a check is vacuous (check() asserts it; test_nonfinite_host.py shows it holds without a GPU):
  conv / TCN / thin  an input element reaches only the outputs of its sample whose window covers it - the other samples
                     (B >= 2) stay finite; a weight or bias element reaches one of >= 32 output channels
  GEMM               an `a` element reaches one row, a `b` or bias element one column of C
  BatchNorm          training statistics spread a poison over its whole channel and no further: every shape has at
                     least two channels and one is poisoned; in eval mode only the poisoned element (x) or channel
                     (gamma, beta) is non-finite
  gradients          a dy element reaches one output channel of dW / the window of one sample of dx
  A -inf in a bias (or beta) under ReLU is left out: the whole channel becomes 0 and the reference has no non-finite
  element left; -inf under ReLU is covered by the input and weight positions, whose outputs are -inf and +inf by the
  sign of the other factor.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as F

SLOPE = 0.2
POISONS = {"nan": float("nan"), "pinf": float("inf"), "ninf": float("-inf")}
# tolerances of the existing parity tests (test_gpu_kernels.py / test_gpu_tcn.py): fp32 contraction noise relative to the
# tensor's largest element; 3e-5 for weight gradients (K = batch x length); BatchNorm forward 1e-5, its dx 2e-5
TOL, TOL_DW, TOL_BN, TOL_BN_BWD = 2e-5, 3e-5, 1e-5, 2e-5

# id: unique; site: the source the case reaches; split_k: the GPU test also runs it in the two-launch split-K form;
# run(k, dev) -> [(label, got, ref64, tol)] with k a kernels backend and dev(t) the tensor on the backend's device
Case = collections.namedtuple("Case", "id site run split_k")


def gen(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def check(got, ref64, tol):
    """got carries the reference's NaN set exactly (none swallowed, none leaked), equals it where it is +-inf, and is
    within `tol` elsewhere: max |got - ref| over the finite reference elements / max(1, max |ref| over the same) - the
    rel_err of the parity tests with the non-finite elements left out of numerator and denominator. The reference must
    have both kinds of element."""
    got = got.detach().cpu().double()
    ref = ref64.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = ref.isfinite()
    assert bool(fin.any()) and not bool(fin.all()), \
        "vacuous case: %d of %d reference elements are finite" % (int(fin.sum()), ref.numel())
    gn, rn = got.isnan(), ref.isnan()
    if not torch.equal(gn, rn):
        lost, leaked = rn & ~gn, gn & ~rn
        where = (lost | leaked).nonzero()[0].tolist()
        raise AssertionError("NaN set differs: %d of the reference's %d NaNs are missing, %d NaNs outside it (first at %s: "
                             "got %r, reference %r)" % (int(lost.sum()), int(rn.sum()), int(leaked.sum()), where,
                                                        got[tuple(where)].item(), ref[tuple(where)].item()))
    inf = ref.isinf()
    if bool(inf.any()):
        bad = inf & (got != ref)
        assert not bool(bad.any()), "%d of %d infinite reference elements differ (first at %s: got %r, reference %r)" % (
            int(bad.sum()), int(inf.sum()), bad.nonzero()[0].tolist(), got[bad][0].item(), ref[bad][0].item())
    err = (got[fin] - ref[fin]).abs().max().item() / max(1.0, ref[fin].abs().max().item())
    assert err < tol, "relative error %.3g on the finite elements (bound %.3g)" % (err, tol)


def act64(z, act):
    return z if act == 0 else (F.relu(z) if act == 1 else F.leaky_relu(z, SLOPE))


def mf64(mask):
    m = mask.double()
    return torch.where(m > 0, torch.ones_like(m), torch.full_like(m, SLOPE))


def poisons(masked=False):
    return ("nan",) if masked else ("nan", "pinf", "ninf")


def conv_plants(pad, masked=False):
    """(poison, position) pairs of a forward conv case. NaN goes to every position. The infinities go where they ask
    something a NaN does not: +inf to x_last and x_mid (the operand a zero-weight phantom tap would meet: 0 x inf) and to
    the bias (a whole +inf channel); -inf to x_first and the weight (outputs of both signs: -inf -> 0 under ReLU next to
    +inf kept)."""
    out = [("nan", w) for w in conv_positions(pad)]
    if not masked:
        out += [("pinf", "x_last"), ("pinf", "x_mid"), ("pinf", "b"), ("ninf", "x_first"), ("ninf", "w")]
    return out


def dead(act, poison, where):
    """-inf added to a whole channel under ReLU: an all-zero, all-finite channel (see the module docstring)"""
    return act == 1 and poison == "ninf" and where in ("b", "bias", "beta")


# ------------------------------------------------------------------------------------------------ convolutions
def conv_positions(pad):
    return ("x_first", "x_last") + (("x_pad",) if pad > 0 else ()) + ("x_mid", "w", "b")


@functools.lru_cache(maxsize=4)
def _conv_clean(B, Cin, L, Cout, ks):
    return (gen(B, Cin, L, seed=1), gen(Cout, Cin, ks, seed=2, scale=1.0 / math.sqrt(Cin * ks)),
            gen(Cout, seed=3, scale=0.1))


@functools.lru_cache(maxsize=8)
def conv_poisoned(shape, poison, where):
    """-> (x, w, b, z64): the seeded operands with the poison planted, and the fp64 pre-activation reference
    F.conv1d(x, w, b) of exactly those operands, computed once per (shape, poison, position). Callers go through
    conv_operands(), which hands out copies: a backend that writes into an operand cannot reach the next case."""
    B, Cin, L, Cout, ks, s, p = shape
    x, w, b = (t.clone() for t in _conv_clean(B, Cin, L, Cout, ks))
    v = POISONS[poison]
    if where == "x_first":
        x[0, 0, 0] = v
    elif where == "x_last":
        x[-1, -1, min(L - 1, ((L + 2 * p - ks) // s) * s - p + ks - 1)] = v
    elif where == "x_pad":
        assert p > 0 and ks - 1 - p >= 1
        x[B // 2, Cin // 2, 1] = v
    elif where == "x_mid":
        q = ((L // 2) // s) * s - p + ks
        assert 0 < q < L - ks
        x[B // 2, Cin // 2, q] = v
    elif where == "w":
        w[Cout // 3, Cin // 2, ks // 2] = v
    elif where == "b":
        b[Cout - 1] = v
    else:
        raise KeyError(where)
    z = F.conv1d(x.double(), w.double(), b.double(), stride=s, padding=p)
    return x, w, b, z


def conv_operands(shape, poison, where):
    return tuple(t.clone() for t in conv_poisoned(shape, poison, where))


def _conv_fwd_case(tag, site, shape, epi, act, poison, where, split_k=False):
    B, Cin, L, Cout, ks, s, p = shape

    def run(k, dev):
        x, w, b, z = conv_operands(shape, poison, where)
        xd, wd, bd = dev(x), dev(w), dev(b)
        slope = SLOPE if act == 2 else 0.0
        a = act64(z, act)
        if epi == "plain":
            return [("y", k.conv1d_fwd(xd, wd, bd, s, p, act=act, slope=slope), a, TOL)]
        mask, res = gen(*z.shape, seed=5), gen(*z.shape, seed=6)
        if epi == "mask":
            y = k.conv1d_fwd(xd, wd, bd, s, p, act=act, slope=slope, out_mask=dev(mask), out_mask_slope=SLOPE)
            return [("y", y, a * mf64(mask), TOL)]
        if epi == "res":
            y = k.conv1d_fwd(xd, wd, bd, s, p, act=act, slope=slope, residual=dev(res))
            return [("y", y, a + res.double(), TOL)]
        if epi == "mask_res":      # mask BEFORE the residual (include/m2d.h)
            y = k.conv1d_fwd(xd, wd, bd, s, p, act=act, slope=slope, residual=dev(res), out_mask=dev(mask),
                             out_mask_slope=SLOPE)
            return [("y", y, a * mf64(mask) + res.double(), TOL)]
        if epi == "two_out":       # y without the residual, sum_out = y + residual
            y, so = k.conv1d_fwd(xd, wd, bd, s, p, act=act, slope=slope, residual=dev(res),
                                 sum_out=dev(torch.empty(tuple(z.shape))))
            return [("y", y, a, TOL), ("sum_out", so, a + res.double(), TOL)]
        raise KeyError(epi)
    return Case("%s-%s-act%d-%s-%s" % (tag, epi, act, poison, where), site, run, split_k)


def _conv_fwd_cases(tag, site, shape, epilogues, split_k=False):
    """epilogues: (epi, act) pairs, each with the plants of conv_plants() (NaN only under a mask)"""
    out = []
    for epi, act in epilogues:
        for poison, where in conv_plants(shape[6], masked="mask" in epi):
            if not dead(act, poison, where):
                out.append(_conv_fwd_case(tag, site, shape, epi, act, poison, where, split_k))
    return out


def _conv_stats_case(tag, site, shape, act, poison, where):
    """conv1d_fwd(with_stats): the returned sums of a channel that holds a NaN are NaN; the other channels' sums equal the
    fp64 sums of what the launch stored (1e-6, as test_conv1d_epilogue_statistics_and_bn_from_sums). The expected sums
    are the fp64 sums of the stored y with the reference's non-finite elements in their places, so a launch that swallows a
    NaN in y and in its sums alike still misses them (y is checked first, against fp64; the sums then against what was
    stored). `where` is w or b: one poisoned output channel, the others finite."""
    B, Cin, L, Cout, ks, s, p = shape

    def run(k, dev):
        x, w, b, z = conv_operands(shape, poison, where)
        a = act64(z, act)
        y, sums = k.conv1d_fwd(dev(x), dev(w), dev(b), s, p, act=act, slope=SLOPE if act == 2 else 0.0, with_stats=True)
        y64 = torch.where(a.isfinite(), y.detach().cpu().double(), a)
        want = torch.stack((y64.sum((0, 2)), (y64 * y64).sum((0, 2))), 1).reshape(-1)
        return [("y", y, a, TOL), ("sums", sums, want, 1e-6)]
    return Case("%s-stats-act%d-%s-%s" % (tag, act, poison, where), site, run, False)


def _first_kept(mask, last=False):
    """index of the first (last) element whose mask is > 0"""
    idx = (mask > 0).nonzero()
    return tuple(idx[-1 if last else 0].tolist())


def _bwd_data_case(tag, site, shape, masked, poison, where):
    """conv1d_bwd_data; `masked`: dy_mask (slope 0), out_mask (slope 0.2) and residual - dx = out_mask * (conv^T(dy *
    dy_mask) + residual), the mask_last epilogue. where: dy_first / dy_last / dy_mid (one dy element; under the mask one
    whose mask is > 0) or w."""
    B, Cin, L, Cout, ks, s, p = shape

    def run(k, dev):
        _, w, _ = (t.clone() for t in _conv_clean(B, Cin, L, Cout, ks))
        Lout = (L + 2 * p - ks) // s + 1
        dy, mask = gen(B, Cout, Lout, seed=4), gen(B, Cout, Lout, seed=5)
        v = POISONS[poison]
        if where == "w":
            w[Cout // 3, Cin // 2, ks // 2] = v
        elif masked:
            dy[_first_kept(mask, last=where == "dy_last")] = v
        else:
            dy[{"dy_first": (0, 0, 0), "dy_last": (B - 1, Cout - 1, Lout - 1), "dy_mid": (B // 2, Cout // 3, Lout // 2)}[where]] = v
        d64 = dy.double() * (mask.double() > 0).double() if masked else dy.double()
        x64 = torch.zeros(B, Cin, L, dtype=torch.float64, requires_grad=True)
        (gx,) = torch.autograd.grad(F.conv1d(x64, w.double(), None, stride=s, padding=p), x64, d64)
        if not masked:
            return [("dx", k.conv1d_bwd_data(dev(dy), dev(w), L, s, p), gx, TOL)]
        om, rs = gen(B, Cin, L, seed=7), gen(B, Cin, L, seed=8)
        dx = k.conv1d_bwd_data(dev(dy), dev(w), L, s, p, dy_mask=dev(mask), dy_mask_slope=0.0, out_mask=dev(om),
                               out_mask_slope=SLOPE, residual=dev(rs))
        return [("dx", dx, (gx + rs.double()) * mf64(om), TOL)]      # residual BEFORE the mask
    return Case("%s-bwd_data%s-%s-%s" % (tag, "-mask_last" if masked else "", poison, where), site, run, False)


def _bwd_weight_case(tag, site, shape, poison, where):
    """conv1d_bwd_weight(with_bias) with one dy element poisoned: one output channel of dW and of the bias gradient. The
    element sits mid-row: at a row's end some taps pair it with the zero padding, and whether that product (0 x NaN) is
    formed at all differs between torch's own CPU paths - not a question these cases ask."""
    B, Cin, L, Cout, ks, s, p = shape

    def run(k, dev):
        x, w, _ = (t.clone() for t in _conv_clean(B, Cin, L, Cout, ks))
        Lout = (L + 2 * p - ks) // s + 1
        dy = gen(B, Cout, Lout, seed=4)
        dy[{"dy_first": (0, 0, Lout // 2), "dy_last": (B - 1, Cout - 1, Lout // 2 + 1), "dy_mid": (B // 2, Cout // 3, Lout // 2)}[where]] = POISONS[poison]
        w64 = w.double().requires_grad_(True)
        (gw,) = torch.autograd.grad(F.conv1d(x.double(), w64, None, stride=s, padding=p), w64, dy.double())
        dw, db = k.conv1d_bwd_weight(dev(x), dev(dy), ks, s, p, with_bias=True)
        return [("dw", dw, gw, TOL_DW), ("db", db, dy.double().sum((0, 2)), TOL_DW)]
    return Case("%s-bwd_weight-%s-%s" % (tag, poison, where), site, run, False)


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_case(mode, mnk, poison, where):
    M, N, Kd = mnk

    def run(k, dev):
        a = gen(M, Kd, seed=1)
        bt = gen(N, Kd, seed=2, scale=1.0 / math.sqrt(Kd))
        bias = gen(N, seed=3)
        v = POISONS[poison]
        if where == "a_first":
            a[0, 0] = v
        elif where == "a_last":
            a[-1, -1] = v
        elif where == "b":
            bt[N // 3, Kd // 2] = v
        else:
            bias[N - 1] = v
        ref = F.relu(a.double() @ bt.double().t() + bias.double())
        if mode == 0:
            c = k.gemm(0, dev(a), dev(bt), dev(bias), act=1)
        elif mode == 1:
            c = k.gemm(1, dev(a), dev(bt.t().contiguous()), dev(bias), act=1)
        else:
            c = k.gemm(2, dev(a.t().contiguous()), dev(bt.t().contiguous()), dev(bias), act=1)
        return [("c", c, ref, TOL)]
    return Case("gemm-mode%d-%s-%s" % (mode, poison, where),
                "gemm_engine.hip m2d_tile_epilogue, fast pass, 16-byte rows (N = 128)", run, False)


# ------------------------------------------------------------------------------------------------ BatchNorm
def _bn_operands(shape, poison, where, plain=False):
    B, C, L = shape
    x = gen(B, C, L, seed=1) if plain else gen(B, C, L, seed=1) * 1.5 + 0.3
    gamma, beta = 1.0 + gen(C, seed=2, scale=0.1), gen(C, seed=3, scale=0.1)
    v = POISONS[poison]
    if where == "x_first":
        x[0, 0, 0] = v
    elif where == "x_last":
        x[-1, -1, -1] = v
    elif where == "gamma":
        gamma[C // 2] = v
    elif where == "beta":
        beta[C - 1] = v
    elif where != "dy_last":
        raise KeyError(where)
    return x, gamma, beta


def bn_plants():
    """(poison, position) pairs of a BatchNorm case: NaN at every position; +inf in the last x element and in beta (a
    whole +inf channel), -inf in the first x element and in beta (-inf kept by act 0 / 2; left out under ReLU: dead())"""
    return [("nan", w) for w in bn_positions("nan")] + [("pinf", "x_last"), ("pinf", "beta"), ("ninf", "x_first"), ("ninf", "beta")]


def bn_positions(poison):
    # an infinite gamma is left out: gamma * xhat + beta and F.batch_norm's x * (gamma * invstd) + (beta - mean * gamma *
    # invstd) are the same number only while gamma is finite (the second form is inf - inf)
    return ("x_first", "x_last", "beta") + (("gamma",) if poison == "nan" else ())


def _running(C):
    return gen(C, seed=4, scale=0.1), 1.0 + gen(C, seed=5, scale=0.1).abs()


def _bn_fwd_case(shape, training, act, with_res, poison, where):
    B, C, L = shape

    def run(k, dev):
        x, gamma, beta = _bn_operands(shape, poison, where)
        rm, rv = _running(C)
        res = gen(B, C, L, seed=9)
        z = F.batch_norm(x.double(), rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), training, 0.1, 1e-5)
        ref = act64(z, act) + (res.double() if with_res else 0.0)
        y, _, _ = k.bn_fwd(dev(x), dev(gamma), dev(beta), dev(rm), dev(rv), training, 1e-5, 0.1, act,
                           SLOPE if act == 2 else 0.0, residual=dev(res) if with_res else None)
        return [("y", y, ref, TOL_BN)]
    return Case("bn_fwd-%s-%s-act%d%s-%s-%s" % ("x".join(map(str, shape)), "train" if training else "eval", act,
                                                 "-res" if with_res else "", poison, where),
                "bn.hip:480 m2d_bn_apply_kernel (forward arm)", run, False)


def _bn_fused_case(shape, kind, poison, where):
    """bn_fwd_sums_pool / bn_fwd_sums_upsample2 with ReLU, the statistics handed in as fp64 sums of the poisoned x (the
    way test_batchnorm_pass_with_the_following_pool_or_upsampling_fused_in makes them)"""
    B, C, L = shape

    def run(k, dev):
        x, gamma, beta = _bn_operands(shape, poison, where, plain=True)
        x64 = x.double()
        sums = torch.stack((x64.sum((0, 2)), (x64 * x64).sum((0, 2))), 1).reshape(-1)
        rm, rv = torch.full((C,), 0.25), torch.full((C,), 1.5)
        y_ref = F.relu(F.batch_norm(x64, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5))
        if kind == "pool":
            y, pooled, _, _ = k.bn_fwd_sums_pool(dev(x), dev(sums), float(B * L), dev(gamma), dev(beta), dev(rm), dev(rv),
                                                 1e-5, 0.1, act=1)
            return [("y", y, y_ref, TOL_BN), ("pooled", pooled, F.max_pool1d(y_ref, 2, 2), TOL_BN)]
        up, _, _ = k.bn_fwd_sums_upsample2(dev(x), dev(sums), float(B * L), dev(gamma), dev(beta), dev(rm), dev(rv),
                                           1e-5, 0.1, act=1)
        return [("up", up, F.interpolate(y_ref, scale_factor=2, mode="linear", align_corners=False), TOL_BN)]
    site = {"pool": "bn.hip:480 m2d_bn_apply_kernel with pool_out", "upsample2": "bn.hip:578 m2d_bn_upsample2_rows_kernel (even L)",
            "upsample2-odd": "bn.hip:530 m2d_bn_upsample2_flat_kernel (odd L)"}[kind + ("-odd" if kind == "upsample2" and L % 2 else "")]
    return Case("bn_%s-%s-%s-%s" % (kind, "x".join(map(str, shape)), poison, where), site, run, False)


def _bn_bwd_case(shape, act, poison, where):
    """bn_bwd after bn_fwd of the same operands: dx carries the reference's NaN set (autograd of the fp64 ops). The
    poisoned channel's dgamma / dbeta are not part of the check."""
    B, C, L = shape

    def run(k, dev):
        x, gamma, beta = _bn_operands(shape, poison, where)
        rm, rv = _running(C)
        dy = gen(B, C, L, seed=6)
        if where == "dy_last":
            dy[-1, -1, -1] = POISONS[poison]
        x64 = x.double().requires_grad_(True)
        z = F.batch_norm(x64, rm.double().clone(), rv.double().clone(), gamma.double(), beta.double(), True, 0.1, 1e-5)
        (gx,) = torch.autograd.grad(act64(z, act), x64, dy.double())
        slope = SLOPE if act == 2 else 0.0
        xd, gd, bd = dev(x), dev(gamma), dev(beta)
        _, mean, invstd = k.bn_fwd(xd, gd, bd, dev(rm), dev(rv), True, 1e-5, 0.1, act, slope)
        dx, _, _ = k.bn_bwd(dev(dy), xd, gd, bd, mean, invstd, act, slope)
        return [("dx", dx, gx, TOL_BN_BWD)]
    return Case("bn_bwd-%s-act%d-%s-%s" % ("x".join(map(str, shape)), act, poison, where),
                "bn.hip:485 m2d_bn_apply_kernel (backward arm; unchanged by the fix)", run, False)


# ------------------------------------------------------------------------------------------------ split-K in one launch
def _split_k_one_launch_case():
    """The operands of test_split_k_in_one_launch_equals_the_two_launch_form with a NaN planted: the weight gradient (K =
    B * Lout = 15 360: always split; no activation - it pins the NaN set of one output channel) and the small-N forward
    with bias and ReLU (split; the reduce step applies the epilogue)."""
    B, Cin, L, Cout, ks, s, p = 128, 128, 120, 128, 7, 1, 3

    def run(k, dev):
        x, dy = gen(B, Cin, L, seed=1), gen(B, Cout, L, seed=2)
        w, bias = gen(Cout, Cin, ks, seed=3) / math.sqrt(Cin * ks), gen(Cout, seed=4)
        dy[B // 2, Cout // 3, L // 2] = POISONS["nan"]
        x8 = x[:8].clone()
        x8[3, 5, 60] = POISONS["nan"]
        ref_w = torch.nn.grad.conv1d_weight(x.double(), w.shape, dy.double(), stride=s, padding=p)
        ref_y = F.relu(F.conv1d(x8.double(), w.double(), bias.double(), stride=s, padding=p))
        gw = k.conv1d_bwd_weight(dev(x), dev(dy), ks, s, p)
        y = k.conv1d_fwd(dev(x8), dev(w), dev(bias), s, p, act=1)
        return [("dw", gw, ref_w, TOL), ("y", y, ref_y, TOL)]
    return Case("split_k-one_launch_operands-nan", "gemm_engine.hip m2d_splitk_reduce_kernel -> m2d_epilogue (two-launch form); "
                "the last arriver's tile epilogue (one-launch form)", run, True)


# ------------------------------------------------------------------------------------------------ the table
# (B, Cin, L, Cout, k, stride, pad) - shapes of CONV_CASES (test_gpu_kernels.py) and SHAPES (test_gpu_tcn.py), which are
# known to route as stated
ACTS = (("plain", 0), ("plain", 1), ("plain", 2))


def _build():
    c = []
    # ---- TemporalBlock k7 convs: csrc/tcn.hip m2d_tcn_conv_kernel, the epilogue after the two K halves meet (m2d_act at
    # tcn.hip:397). (3, 128, 120): 16-column tiles; (50, 128, 120): 32-column tiles.
    for tag, shape in (("tcn16", (3, 128, 120, 128, 7, 1, 3)), ("tcn32", (50, 128, 120, 128, 7, 1, 3))):
        site = "tcn.hip:397 m2d_tcn_conv_kernel epilogue (%s-column tiles)" % tag[3:]
        c += _conv_fwd_cases(tag, site, shape, ACTS + (("mask_res", 2), ("two_out", 1)))
        for where in ("dy_first", "dy_last", "w"):          # the mask_last form: the values are gradients
            c.append(_bwd_data_case(tag, site + ", mask_last", shape, True, "nan", where))
    # ---- thin forward: conv1d_thin.hip thin_fwd_mfma_kernel. The interior path (:517) needs 16-byte rows: audio_d.l1 has
    # Lout = 19 200. wg.l1's Lout is 794 (even, not a multiple of 4: every tile takes the row-end path, :541, with 8-byte
    # stores), wg.l1-odd-lout's 795 (scalar stores), wg.l1-pad-even's 798 with pad 3. +inf in the last input sample
    # (pinf-x_last) meets the phantom odd tap's zero weight ("0 x inf", the LAST_DEAD operand of the kernel).
    thin_epi = ACTS + (("mask", 1),)
    c += _conv_fwd_cases("thin19200", "conv1d_thin.hip:517 thin_fwd_mfma_kernel, interior path (16-byte rows)",
                         (2, 1, 76800, 32, 25, 4, 11), thin_epi)
    c += _conv_fwd_cases("thin794", "conv1d_thin.hip:541 thin_fwd_mfma_kernel, row-end path (8-byte rows)", (3, 1, 3200, 32, 25, 4, 0), thin_epi)
    c += _conv_fwd_cases("thin795", "conv1d_thin.hip:541 thin_fwd_mfma_kernel, row-end path (scalar rows)", (3, 1, 3204, 32, 25, 4, 0), thin_epi)
    c += _conv_fwd_cases("thin798pad", "conv1d_thin.hip:541 thin_fwd_mfma_kernel, row-end path, pad 3", (2, 1, 3210, 32, 25, 4, 3), thin_epi)
    # ---- thin_long_fwd_kernel (k250 / stride 50), conv1d_thin.hip:802
    c += _conv_fwd_cases("thinlong", "conv1d_thin.hip:802 thin_long_fwd_kernel", (6, 1, 3200, 32, 250, 50, 124), ACTS)
    # ---- engine fast pass, 16-byte rows (Lout = 32): gemm_engine.hip:600-603
    c += _conv_fwd_cases("wide", "gemm_engine.hip:600 m2d_tile_epilogue<WIDE> fast pass", (6, 32, 64, 64, 4, 2, 1), ACTS + (("mask", 1),))
    for mode in (0, 1, 2):
        for poison in poisons():
            for where in ("a_first", "a_last", "b", "bias"):
                if not dead(1, poison, where):
                    c.append(_gemm_case(mode, (64, 128, 200), poison, where))
    # ---- engine fast pass, one element per lane (Lout = 43: odd rows): gemm_engine.hip:621
    c += _conv_fwd_cases("narrow", "gemm_engine.hip:621 m2d_tile_epilogue<!WIDE> fast pass", (3, 64, 193, 128, 25, 4, 0), ACTS)
    # the same pass with epilogue statistics (Lout = 193): the row sums re-read the image at gemm_engine.hip:541-544
    for act in (0, 1):
        for poison in poisons():
            for where in ("w", "b"):
                if not dead(act, poison, where):
                    c.append(_conv_stats_case("narrow", "gemm_engine.hip:541 row statistics of the one-element fast pass",
                                              (3, 32, 794, 64, 25, 4, 0), act, poison, where))
    # ---- engine general pass (a residual): 16-byte rows gemm_engine.hip:692, one element per lane :724
    c += _conv_fwd_cases("general-wide", "gemm_engine.hip:692 m2d_tile_epilogue<WIDE> general pass",
                         (2, 128, 200, 128, 3, 1, 1), (("res", 1), ("res", 2)))
    c += _conv_fwd_cases("general-narrow", "gemm_engine.hip:724 m2d_tile_epilogue<!WIDE> general pass",
                         (3, 64, 193, 128, 25, 4, 0), (("res", 1), ("res", 2)))
    # ---- split-K plans: the reduce kernel's m2d_epilogue (gemm_engine.hip:313) in the two-launch form, the last
    # arriver's tile epilogue in the one-launch form
    for tag, shape in (("split.a", (40, 32, 100, 48, 5, 2, 2)), ("split.b", (70, 16, 33, 130, 3, 1, 1))):
        c += _conv_fwd_cases(tag, "gemm_engine.hip:313 m2d_epilogue (two-launch split-K) / tile epilogue of the last arriver",
                             shape, (("plain", 1),), split_k=True)
    c.append(_split_k_one_launch_case())
    # ---- BatchNorm: bn.hip:480 (m2d_bn_apply_kernel), :530 (upsample, flat kernel: odd L), :578 (upsample, rows kernel)
    for shape in ((4, 128, 120), (7, 5, 3)):
        for act in (0, 1, 2):
            for with_res in (False, True):
                for poison, where in bn_plants():
                    if not dead(act, poison, where):
                        c.append(_bn_fwd_case(shape, True, act, with_res, poison, where))
        for poison, where in bn_plants():   # (eval, -inf in x: one 0 among finite values - nothing non-finite left)
            if not dead(1, poison, where) and not (poison == "ninf" and where.startswith("x_")):
                c.append(_bn_fwd_case(shape, False, 1, False, poison, where))
        for act in (0, 1, 2):
            for poison, where in (("nan", "x_first"), ("pinf", "x_last"), ("ninf", "x_first"), ("nan", "dy_last"), ("nan", "gamma")):
                c.append(_bn_bwd_case(shape, act, poison, where))
    for kind, shape in (("pool", (9, 16, 200)), ("upsample2", (9, 16, 200)), ("upsample2", (7, 6, 3))):
        for poison, where in bn_plants():
            if not dead(1, poison, where):
                c.append(_bn_fused_case(shape, kind, poison, where))
    # ---- no activation: weight gradients and backward-data with a NaN in dy (they pass before the fix and pin it):
    # tcn.hip (k7) and, for k25 / stride 4 / pad 11, the sub-pixel backward-data with the quad epilogue
    # (gemm_engine.hip:1043 - bwd_data never sets an activation, so that site's ReLU cannot be reached through the C-ABI)
    for tag, shape in (("tcn16", (3, 128, 120, 128, 7, 1, 3)), ("k25s4", (2, 32, 1024, 64, 25, 4, 11))):
        for where in ("dy_first", "dy_mid", "dy_last"):
            c.append(_bwd_weight_case(tag, "weight gradient of %s" % tag, shape, "nan", where))
            c.append(_bwd_data_case(tag, "backward-data of %s" % tag, shape, False, "nan", where))
    return c


CASES = _build()
assert len({c.id for c in CASES}) == len(CASES)
