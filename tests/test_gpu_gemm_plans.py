"""The GEMM engine under forced launch plans (csrc/gemm_engine.hip: m2d_debug_force_plan, bound in tests/plan_cases.py):
every tile height (32 / 64 / 128 rows) and every split form (unsplit, split-K in one launch with the stream's tickets,
the two-launch form with m2d_splitk_reduce_kernel, a split count with empty trailing splits) of the three kernel
families, on shapes with partial tiles in both directions - against fp64 torch on the CPU and against each other.
Which plan a launch takes is otherwise the cost model's choice for the shape: the op-level cases of test_gpu_kernels.py
run the 32-row tile in almost every dense case, and cannot say which kernel they ran.

Bounds (the project's own): rel_err = max|got - ref64| / max(1, max|ref64|) < 2e-5 for contractions (test_gpu_kernels.py),
3e-5 for weight and bias gradients (test_conv1d_fwd_bwd), 1e-6 for the epilogue statistics against the sums of the y the
launch wrote (test_epilogue_statistics_with_and_without_the_streams_tickets), 2e-6 between the plans of one call
(test_split_k_in_one_launch_equals_the_two_launch_form's figure for its two forms): between any two plans of a dense
call (K = 1 283), between the two forms of one (rows, splits) of a conv pass (K up to 3 591, where an unsplit fp32 chain
alone is further than that from a 20-split sum).

Measured on an MI355X (worst over all cases; the same to three digits at 32, 64 and 128 rows - the tile height does not
change the order of a sum): dense, against fp64, unsplit 1.84e-6 / 1.65e-6 / 1.51e-6 in modes 0 / 1 / 2, 3 splits 1.2e-6
or less, 16 and 20 splits 4.4e-7 or less; between plans of a call 1.96e-6 / 1.70e-6 / 1.55e-6 - the unsplit launch
against the most-split ones, close under the 2e-6, and the same figure in every run: nothing in a plan is timed. Conv
passes against fp64: 2.2e-6 at most (unsplit stride-1 backward-data, K = 3 591), between the two forms of one plan
under 2e-6, between all plans of a pass 2.8e-6 at most (recorded, not asserted)."""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import plan_cases as C
from tests.test_gpu_kernels import DEV, K, gen, rel_err

pytestmark = pytest.mark.gpu

WORST = {}   # printed by tests/conftest.py with every run
BMS = (32, 64, 128)
# (splits, with the stream's tickets): 81 and more K chunks in 16 splits of 6 leave the last two or more splits empty, in
# 20 splits of 5 the last three or more; 20 > M2D_FUSE_MAX_SPLITS runs in two launches whatever the stream has
PLANS = ((1, True), (3, True), (16, True), (3, False), (16, False), (20, True))
FUSE_MAX = 16
GUARD = 1024   # floats behind the workspace the launch is told about


@pytest.fixture(scope="module", autouse=True)
def _no_forced_plan_is_left_behind():
    yield
    assert C.force_plan(0, 0) == 0


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def form(splits, fused):
    return "unsplit" if splits == 1 else ("%d splits, one launch" if fused else "%d splits, two launches") % splits


@contextlib.contextmanager
def tickets(on):
    """The current stream's ticket scratch, registered (on) or unregistered for the scope (the two-launch split-K)."""
    from music2dance_amd import _lib, kernels
    dev = torch.device(DEV)
    stream = kernels._stream(dev)   # (a stream's first look-up registers its scratch)
    t = kernels._STREAM_SCRATCH[(dev.index, stream)]
    if on:
        yield t
        return
    _lib.check(_lib.lib().m2d_stream_scratch_set(stream, 0, 0), "m2d_stream_scratch_set")
    try:
        yield t
    finally:
        torch.cuda.synchronize()
        _lib.check(_lib.lib().m2d_stream_scratch_set(stream, t.data_ptr(), t.numel() * 4), "m2d_stream_scratch_set")


def spread(results):
    """results: same-shaped device tensors, one per plan -> per plan, its largest difference to any other plan, relative to
    max(1, largest magnitude of any of them) - rel_err of every pair, at once."""
    r = torch.stack([x.double().reshape(-1) for x in results])
    lo, hi = r.min(0).values, r.max(0).values
    denom = max(1.0, r.abs().amax(1).min().item())
    return [max((x - lo).max().item(), (hi - x).max().item()) / denom for x in r]


# ------------------------------------------------------------------------------------------------- dense GEMMs
M, KD = 261, 1283            # row tiles 9 / 5 / 3 with a partial last one at every height; 81 chunks, the last 3 deep
NCHUNKS = -(-KD // 16)
# N, row pitch of the output's buffer, column offset of the block (operand blocks take the same offset):
WIDTHS = {"n260": (260, 284, 8),             # 16-byte epilogue rows
          "n260-odd-pitch": (260, 285, 8),   # ... declined: rows do not start on 16 bytes
          "n261": (261, 288, 3)}             # one-element rows
FAMILY = {0: "mode 0 (register staging, K-fast / K-fast)", 1: "mode 1 (register staging, K-fast / row-fast)",
          2: "mode 2 (LDS-direct)"}
DENSE_CASES = [(mode, width, "plain") for mode in (0, 1, 2) for width in WIDTHS] + [
    (0, "n261", "bias+relu"), (0, "n260", "bias+leaky"), (0, "n260", "masks"), (0, "n261", "masks"),
    (1, "n261", "bias+leaky"), (1, "n260", "masks"),
    (2, "n260", "bias+leaky"), (2, "n261", "bias+leaky"), (2, "n261", "out_mask")]
SENTINEL = -1234.5


@functools.lru_cache(maxsize=None)
def _dense(mode, width):
    """Operands of one (mode, width) as column blocks of wider device buffers, and the fp64 products (computed once)."""
    N, ldc, off = WIDTHS[width]
    g = torch.Generator().manual_seed(1000 * mode + ldc)
    rnd = lambda *s: torch.randn(*s, generator=g)
    a, bt, bias, am, om = rnd(M, KD), rnd(N, KD) / math.sqrt(KD), rnd(N), rnd(M, KD), rnd(M, N)

    def block(mat, pad, at):   # `mat` as the columns [at, at + cols) of a buffer `pad` columns wider, noise around it
        buf = rnd(mat.shape[0], mat.shape[1] + pad)
        buf[:, at:at + mat.shape[1]] = mat
        return buf.to(DEV)[:, at:at + mat.shape[1]]

    d = {"N": N, "ldc": ldc, "off": off, "bias": bias.to(DEV), "bias64": bias.double()}
    if mode == 2:
        d["a"], d["a_mask"] = block(a.t().contiguous(), 3, 1), None
    else:
        d["a"], d["a_mask"] = block(a, 5, 2), block(am, 5, 2)
    d["b"] = block(bt, 9, 4) if mode == 0 else block(bt.t().contiguous(), ldc - N, off)
    ombuf = rnd(M, ldc)
    ombuf[:, off:off + N] = om
    d["out_mask"] = ombuf.to(DEV)[:, off:off + N]
    d["om64"] = torch.where(om.double() > 0, 1.0, 0.2)
    d["prod"] = a.double() @ bt.double().t()
    d["prod_masked"] = (a.double() * (am.double() > 0)) @ bt.double().t() if mode != 2 else None
    return d


def _dense_epilogue(d, epi):
    """-> (C-ABI epilogue arguments, the pre-epilogue product, the expected output), fp64"""
    leaky = lambda v: torch.where(v < 0, 0.2 * v, v)
    if epi == "plain":
        return dict(), d["prod"], d["prod"]
    if epi == "bias+relu":
        return dict(bias=d["bias"], act=1), d["prod"], (d["prod"] + d["bias64"]).clamp_min(0)
    if epi == "bias+leaky":
        return dict(bias=d["bias"], act=2, slope=0.2), d["prod"], leaky(d["prod"] + d["bias64"])
    if epi == "masks":
        return (dict(a_mask=d["a_mask"], out_mask=d["out_mask"], out_mask_slope=0.2), d["prod_masked"],
                d["prod_masked"] * d["om64"])
    assert epi == "out_mask"
    return dict(out_mask=d["out_mask"], out_mask_slope=0.2), d["prod"], d["prod"] * d["om64"]


@pytest.mark.parametrize("mode,width,epi", DENSE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_dense_gemm_under_every_plan(mode, width, epi):
    from music2dance_amd import kernels
    from music2dance_amd.kernels import HipKernels, _ptr
    dev = torch.device(DEV)
    d = _dense(mode, width)
    N, ldc, off = d["N"], d["ldc"], d["off"]
    args, product, want = _dense_epilogue(d, epi)
    a, b = d["a"], d["b"]
    sentinel = torch.full((M, ldc), SENTINEL).view(torch.int32)
    outs, names = [], []
    for bm in BMS:
        for splits, with_tickets in PLANS:
            with C.forced_plan(bm, splits), tickets(with_tickets) as t:
                # the workspace: what the library's own query asks for under this plan, all NaN, and a guard behind it
                nws = C.gemm_ws_bytes(mode, M, N, KD)
                slab = C.slab_bytes(M, N, bm, splits)
                assert nws >= slab and nws % 4 == 0
                rc, pbm, psplits, fused = C.select_plan(C.GENERAL, M, N, NCHUNKS, 1, 1, 0.0, 0, 0, 0, nws, True,
                                                        C.TICKET_BYTES if with_tickets else 0)
                assert (rc, pbm, psplits) == (0, bm, splits)
                assert fused == int(with_tickets and 1 < splits <= FUSE_MAX)
                ws = torch.full((nws // 4 + GUARD,), float("nan"), device=DEV)
                buf = torch.full((M, ldc), SENTINEL, device=DEV)
                out = buf[:, off:off + N]
                kernels._launch("m2d_gemm_ld", dev, mode, _ptr(a), HipKernels._ld(a), _ptr(b), HipKernels._ld(b),
                                _ptr(args.get("bias")), _ptr(out), ldc, M, N, KD, args.get("act", 0),
                                args.get("slope", 0.0), _ptr(args.get("a_mask")), 0.0, _ptr(args.get("out_mask")),
                                args.get("out_mask_slope", 0.0), _ptr(ws), nws)
                torch.cuda.synchronize()
            what = "%s, %d rows, %s" % (FAMILY[mode], bm, form(splits, fused))
            # around the output block: untouched, bit for bit
            got_bits = buf.view(torch.int32).cpu()
            assert torch.equal(got_bits[:, :off], sentinel[:, :off]) and torch.equal(got_bits[:, off + N:], sentinel[:, off + N:]), what
            # the workspace: nothing behind the plan's slab, nothing at all when unsplit; two launches leave the slabs
            assert bool(ws[slab // 4:].isnan().all()), what
            if splits > 1 and not fused:
                slabs = ws[:splits * M * N].view(splits, M, N)
                assert bool(slabs.isfinite().all()), what
                e = rel_err(slabs.double().sum(0), product)
                note("dense %s: sum of the slabs vs fp64" % what, e)
                assert e < 2e-5, what
            if fused:
                # one whole-tile image per (tile, split): as many floats as this tile height and split count make
                assert bool(ws[:slab // 4].isfinite().all()), what
                assert int(t.abs().sum().item()) == 0, what   # the tickets are left zero
            e = rel_err(out, want)
            print("%-100s %-18s %-10s vs fp64 %.3e" % (what, width, epi, e))
            note("dense %s: vs fp64" % what, e)
            assert e < 2e-5, (what, e)
            outs.append(out)
            names.append(what)
    for what, e in zip(names, spread(outs)):
        print("%-100s %-18s %-10s vs the other plans %.3e" % (what, width, epi, e))
        note("dense %s: vs the other plans of the call" % what, e)
        assert e < 2e-6, (what, e)


# ------------------------------------------------------------------------------------- conv passes under forced plans
# (B, Cin, L, Cout, ks, stride, pad): packed, LDS-direct layers (Cin >= 16) with 133 output channels (two row tiles of 128
# or three of 64, the last partial; 133 % 32 != 0), 80 K chunks at least in every splittable pass, several column tiles
# with a partial last one. Stride 1: Lout = 100, 16-byte output rows; stride 2: Lout = 51, one-element rows.
LAYERS = {"s1": (12, 40, 100, 133, 27, 1, 13), "s2": (20, 72, 101, 133, 17, 2, 8)}
PASSES = ("fwd", "fwd_stats", "bwdD", "bwdW")
# a plan outside each pass's envelope: the two-launch form with statistics; elsewhere one split more than the launch's
# chunks allow (4 each) - for a strided backward-data, a launch of `stride` phases, that is any split at all
REFUSED = {"fwd_stats": (64, 20)}


def _query(conv, kind):
    """What the pass's launcher asks select_plan, by hand from csrc/conv1d.hip: (M, N, nchunks, phases, allow_split,
    small-tile penalty, plan kind, bwd_data)."""
    B, Cin, L, Cout, ks, s, p = conv
    Lout = (L + 2 * p - ks) // s + 1
    c16 = lambda n: -(-n // 16)
    if kind in ("fwd", "fwd_stats"):    # rows co, columns (n, l), K = (tap, ci)
        return Cout, B * Lout, ks * c16(Cin), 1, 1, 1.25 if s > 1 else 1.0, 0, 0
    if kind == "bwdW":                  # rows co, columns (ci, tap) + the bias column, K = (n, l)
        assert Lout >= 16
        return Cout, Cin * ks + 1, B * c16(Lout), 1, 1, 0.0, 1, 0
    if s == 1:                          # rows ci, columns (n, j), K = (tap, co)
        return Cin, B * L, ks * c16(Cout), 1, 1, 0.0, 0, 0
    nq = max((L - 1 + p - r) // s - (0 if r >= p else -(-(p - r) // s)) + 1 for r in range(s))
    return Cin, B * nq, -(-ks // s) * c16(Cout), s, 0, 0.0, 2, 1   # one launch of `s` phases: never split


@functools.lru_cache(maxsize=None)
def _layer(name):
    B, Cin, L, Cout, ks, s, p = LAYERS[name]
    x = gen(B, Cin, L, seed=11)
    w = gen(Cout, Cin, ks, seed=12, scale=1.0 / math.sqrt(Cin * ks))
    bias = gen(Cout, seed=13, scale=0.1)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y = F.conv1d(x64, w64, bias.double(), stride=s, padding=p)
    dy = gen(*y.shape, seed=14)
    gx, gw = torch.autograd.grad(y, (x64, w64), dy.double())
    return {"x": x.to(DEV), "w": w.to(DEV), "bias": bias.to(DEV), "dy": dy.to(DEV), "y": y.detach(), "gx": gx, "gw": gw,
            "gb": dy.double().sum((0, 2))}


def _run_pass(kind, d, conv):
    """-> (outputs, (error vs fp64, its bound) per check)"""
    B, Cin, L, Cout, ks, s, p = conv
    if kind == "fwd":
        y = K().conv1d_fwd(d["x"], d["w"], d["bias"], s, p)
        return [y], [(rel_err(y, d["y"]), 2e-5)]
    if kind == "fwd_stats":
        y, sums = K().conv1d_fwd(d["x"], d["w"], d["bias"], s, p, with_stats=True)
        y64 = y.double()
        return [y], [(rel_err(y, d["y"]), 2e-5), (rel_err(sums[0::2], y64.sum((0, 2))), 1e-6),
                     (rel_err(sums[1::2], (y64 * y64).sum((0, 2))), 1e-6)]
    if kind == "bwdD":
        dx = K().conv1d_bwd_data(d["dy"], d["w"], L, s, p)
        return [dx], [(rel_err(dx, d["gx"]), 2e-5)]
    dw, db = K().conv1d_bwd_weight(d["x"], d["dy"], ks, s, p, with_bias=True)
    return [dw, db], [(rel_err(dw, d["gw"]), 3e-5), (rel_err(db, d["gb"]), 3e-5)]


@pytest.mark.parametrize("kind", PASSES)
@pytest.mark.parametrize("layer", list(LAYERS))
def test_conv_pass_under_every_plan_its_envelope_admits(layer, kind):
    from music2dance_amd import _lib
    conv = LAYERS[layer]
    d = _layer(layer)
    Mq, Nq, nchunks, phases, allow_split, penalty, plan_kind, bwd_data = _query(conv, kind)
    stats = kind == "fwd_stats"
    assert Mq in (133, conv[1]) and Nq > 256 and Nq % 128 != 0
    top = C.max_splits(nchunks, phases, allow_split, plan_kind)

    def select(with_tickets):
        ws = C.launcher_ws_bytes(kind, conv, Mq, Nq)
        return C.select_plan(C.GENERAL, Mq, Nq, nchunks, phases, allow_split, penalty, plan_kind, bwd_data, stats, ws,
                             True, C.TICKET_BYTES if with_tickets else 0)

    plans = [(bm, splits, tk) for bm in BMS for splits, tk in PLANS
             if splits <= top and not (stats and splits > 1 and not (tk and splits <= FUSE_MAX))]
    if kind == "bwdD" and conv[5] > 1:
        assert top == 1 and len(plans) == 3      # a strided backward-data runs unsplit only
    else:
        assert nchunks >= 80 and top >= 20 and len(plans) == (9 if stats else 18)
    outs, names = [], []
    for bm, splits, tk in plans:
        with C.forced_plan(bm, splits), tickets(tk) as t:
            fused = int(tk and 1 < splits <= FUSE_MAX)
            assert select(tk) == (0, bm, splits, fused), (bm, splits, tk)   # the hand-made query is the launcher's
            got, errs = _run_pass(kind, d, conv)
            torch.cuda.synchronize()
        if fused:
            assert int(t.abs().sum().item()) == 0
        what = "conv %s %s, %d rows, %s" % (layer, kind, bm, form(splits, fused))
        print("%-70s %s" % (what, " ".join("%.3e" % e for e, _ in errs)))
        note("%s: vs fp64 (worst check relative to its bound)" % what, max(e / bound for e, bound in errs))
        for e, bound in errs:
            assert e < bound, (what, errs)
        outs.append(got)
        names.append(what)
    # Between plans: recorded for all of them; asserted where the project's 2e-6 applies - the two forms of one (rows,
    # splits), which add the same per-split partial tiles and differ only in the order of at most 16 additions. (An
    # unsplit chain of K = 3 591 terms is by itself 2.2e-6 from fp64 here, the 20-split sum 0.3e-6: across split counts
    # only the fp64 bound holds.)
    for i in range(len(outs[0])):
        for what, e in zip(names, spread([o[i] for o in outs])):
            note("%s: vs the other plans of the call" % what, e)
        for bm in BMS:
            for splits in (3, 16):
                pair = [o[i] for o, (pbm, ps, _) in zip(outs, plans) if (pbm, ps) == (bm, splits)]
                assert len(pair) == (0 if top == 1 else 1 if stats else 2)
                if len(pair) == 2:
                    assert spread(pair)[0] < 2e-6, (layer, kind, bm, splits, i)
    # outside the envelope: refused before any launch, and the next launch - the model's own plan - is right
    bm, splits = REFUSED.get(kind, (64, top + 1))   # (where `top` is 20, 20 splits ran above: the launcher counts chunks as _query does)
    with C.forced_plan(bm, splits):
        assert select(True)[0] != 0
        with pytest.raises(_lib.M2dError):
            _run_pass(kind, d, conv)
    natural = select(True)
    assert natural[0] == 0
    got, errs = _run_pass(kind, d, conv)
    print("conv %s %s: the model's plan %s %s" % (layer, kind, natural[1:], " ".join("%.3e" % e for e, _ in errs)))
    for e, bound in errs:
        assert e < bound, (layer, kind, "after the refused launch", errs)
