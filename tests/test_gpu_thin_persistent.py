"""The single-channel conv kernels (csrc/conv1d_thin.hip) against fp64 references at shapes where a wave walks several
tiles - the cases of tests/thin_cases.py, which tests/test_thin_schedule_host.py holds to their regimes:

  forwards   the persistent loops of thin_fwd_mfma_kernel<25,4> and thin_long_fwd_kernel<250,50> / <160,4> entered a
             second, third and fourth time: the hand-over between the two operand sets and the loop-back, a prefetch
             issued while a tile is processed, the next segment landing under the epilogue, the mask rows of every tile,
             the statistics summed over all of a wave's tiles; dense inputs and window views of a track
  backwards  the k25 backward-data and backward-weight kernels with 1 280 and 1 536 positions per block (every other op
             test runs them at 1 024), the last block of a sample partial, unmasked (two tiles in flight) and masked (one)

References: F.conv1d and its autograd in fp64 on the CPU, from the seeded inputs and the weight scaling of
tests/test_gpu_kernels.py: test_conv1d_fwd_bwd. Bounds: that file's own - err = max|got - ref64| / max(1, max|ref64|)
<= 2e-5 for the forward and backward-data, 3e-5 for backward-weight and the bias gradient, 1e-6 for the epilogue
statistics against the fp64 sums of the stored activation. The comparison itself runs on the device in fp64 (the same
quantity as rel_err; a 100 MB activation compared on the host costs more than the kernel and its reference together).

Measured on an MI355X (worst over the cases of a table; the run prints every figure under "worst errors recorded"):
  k25 forward (plain, leaky, ReLU, masked, with statistics)   2.5e-07      statistics against the stored y   1.4e-09
  k250 forward                                                7.0e-07      statistics                        1.5e-09
  k160 forward                                                5.9e-07      statistics                        1.1e-09
  window views                                   k25 2.0e-07, k250 9.1e-07, k160 5.8e-07 (bit-equal to the dense calls)
  k25 backward-data                              chunk-1536 1.8e-07, chunk-1280 2.1e-07, odd-rows 1.6e-07
  k25 backward-weight                            chunk-1536 4.3e-07 (768 000 terms), chunk-1280 3.0e-07, odd-rows 2.3e-07
  k25 bias gradient                              chunk-1536 3.3e-07, chunk-1280 3.6e-07, odd-rows 2.5e-07
  (masked backward cases: 1.3e-07 .. 2.4e-07.) Every figure is well over an order of magnitude inside its bound, the
  backward-weight over 768 000 terms included: a wave sums at most a chunk in fp32, the slabs are summed in fp64.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import thin_cases as C
from tests.test_gpu_kernels import DEV, K, gen, rel_err

pytestmark = pytest.mark.gpu

WORST = {}
FWD_TOL, BWD_DATA_TOL, BWD_WEIGHT_TOL, STATS_TOL = 2e-5, 2e-5, 3e-5, 1e-6
SLOPE = 0.2


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))
    print("%-60s %.3e" % (key, val))
    return val


def err(got, ref64):
    """rel_err of tests/test_gpu_kernels.py, evaluated where `ref64` lives (an fp64 tensor on the device)"""
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    denom = max(1.0, ref64.abs().max().item())
    return (got.double() - ref64).abs().max().item() / denom


def _layer(ks):
    w = gen(C.COUT, 1, ks, seed=2, scale=1.0 / math.sqrt(ks))
    b = gen(C.COUT, seed=3, scale=0.1)
    return w, b


def _keep(mask64, slope):
    return torch.where(mask64 > 0, torch.ones_like(mask64), torch.full_like(mask64, slope))


def _check_stats(tag, k, x, w, b, s, p, ref, y_plain):
    y, sums = k.conv1d_fwd(x, w, b, s, p, with_stats=True)
    assert sums.dtype == torch.float64 and sums.shape == (2 * C.COUT,)
    e_y = note("%s fwd+stats y" % tag, err(y, ref))
    y64 = y.double()
    e_1 = note("%s stats sum" % tag, err(sums[0::2], y64.sum((0, 2))))
    e_2 = note("%s stats sum of squares" % tag, err(sums[1::2], (y64 * y64).sum((0, 2))))
    assert e_y < FWD_TOL
    assert e_1 < STATS_TOL and e_2 < STATS_TOL
    assert torch.equal(y, y_plain), "the statistics launch stored another activation"


@pytest.mark.parametrize("case", C.K25_FWD_CASES, ids=lambda c: c[0])
def test_k25_forward_over_several_tiles_per_wave(case):
    name, B, L, ks, s, p, Lout, tiles, r = case
    tag = "k25 fwd %s" % name
    k = K()
    x = gen(B, 1, L, seed=1)
    w, b = _layer(ks)
    ref = F.conv1d(x.double(), w.double(), b.double(), stride=s, padding=p).to(DEV)
    assert tuple(ref.shape) == (B, C.COUT, Lout)
    x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)
    y_plain = k.conv1d_fwd(x, w, b, s, p)
    e = [note("%s plain" % tag, err(y_plain, ref))]
    y = k.conv1d_fwd(x, w, b, s, p, act=2, slope=SLOPE)
    e.append(note("%s leaky" % tag, err(y, F.leaky_relu(ref, SLOPE))))
    mask = gen(B, C.COUT, Lout, seed=5).to(DEV)
    keep = _keep(mask.double(), SLOPE)
    y = k.conv1d_fwd(x, w, b, s, p, act=2, slope=SLOPE, out_mask=mask, out_mask_slope=SLOPE)
    e.append(note("%s leaky+mask" % tag, err(y, F.leaky_relu(ref, SLOPE) * keep)))
    y = k.conv1d_fwd(x, w, b, s, p, act=1, out_mask=mask, out_mask_slope=SLOPE)
    e.append(note("%s relu+mask" % tag, err(y, ref.clamp_min(0) * keep)))
    y = k.conv1d_fwd(x, w, b, s, p, act=1)
    e.append(note("%s relu" % tag, err(y, ref.clamp_min(0))))
    del y, mask, keep
    assert max(e) < FWD_TOL, e
    _check_stats(tag, k, x, w, b, s, p, ref, y_plain)


@pytest.mark.parametrize("case", C.LONG_FWD_CASES, ids=lambda c: c[0])
def test_long_forward_over_several_tiles_per_wave(case):
    name, B, L, ks, s, p, Lout, tiles, r = case
    tag = "long fwd %s" % name
    k = K()
    x = gen(B, 1, L, seed=1)
    w, b = _layer(ks)
    ref = F.conv1d(x.double(), w.double(), b.double(), stride=s, padding=p).to(DEV)
    assert tuple(ref.shape) == (B, C.COUT, Lout)
    x, w, b = x.to(DEV), w.to(DEV), b.to(DEV)
    y_plain = k.conv1d_fwd(x, w, b, s, p)
    e = [note("%s plain" % tag, err(y_plain, ref))]
    y = k.conv1d_fwd(x, w, b, s, p, act=1)
    e.append(note("%s relu" % tag, err(y, ref.clamp_min(0))))
    assert max(e) < FWD_TOL, e
    _check_stats(tag, k, x, w, b, s, p, ref, y_plain)


@pytest.mark.parametrize("case", C.WINDOW_FWD_CASES, ids=lambda c: c[0])
def test_window_view_forward_over_several_tiles_per_wave(case):
    name, which, B, T, hop, window, ks, s, p, tiles, r = case
    tag = "window fwd %s" % name
    k = K()
    track = gen(B, (T - 1) * hop + window, seed=1)
    w, b = _layer(ks)
    dense = track.unfold(-1, window, hop).contiguous().view(B * T, 1, window)
    ref = F.conv1d(dense.double(), w.double(), b.double(), stride=s, padding=p).to(DEV)
    track, dense, w, b = track.to(DEV), dense.to(DEV), w.to(DEV), b.to(DEV)
    y_w = k.conv1d_fwd_windows(track, T, hop, window, w, b, s, p)
    y_d = k.conv1d_fwd(dense, w, b, s, p)
    assert torch.equal(y_w, y_d)
    assert note(tag, err(y_w, ref)) < FWD_TOL


@pytest.mark.parametrize("masked", [False, True], ids=["two-in-flight", "masked-one-in-flight"])
@pytest.mark.parametrize("case", C.BWD_CASES, ids=lambda c: c[0])
def test_k25_backward_with_a_chunk_other_than_1024(case, masked):
    name, B, L, p, Lout, chunk, blocks = case
    ks, s = 25, 4
    tag = "k25 %s %s" % (name, "masked" if masked else "unmasked")
    k = K()
    x = gen(B, 1, L, seed=1)
    w, _ = _layer(ks)
    dy = gen(B, C.COUT, Lout, seed=4)
    mask = gen(B, C.COUT, Lout, seed=5) if masked else None
    dy_eff = dy.double() * (mask.double() > 0).double() if masked else dy.double()
    x64 = x.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv1d(x64, w64, None, stride=s, padding=p), (x64, w64), dy_eff)
    gb = dy_eff.sum((0, 2))
    del x64, dy_eff
    x, w, dy = x.to(DEV), w.to(DEV), dy.to(DEV)
    kw = dict(dy_mask=mask.to(DEV), dy_mask_slope=0.0) if masked else {}
    dx = k.conv1d_bwd_data(dy, w, L, s, p, **kw)
    e_dx = note("%s bwd_data" % tag, err(dx, gx.to(DEV)))
    dw, db = k.conv1d_bwd_weight(x, dy, ks, s, p, with_bias=True, **kw)
    e_dw = note("%s bwd_weight" % tag, rel_err(dw, gw))
    e_db = note("%s bias gradient" % tag, rel_err(db, gb))
    assert e_dx < BWD_DATA_TOL
    assert e_dw < BWD_WEIGHT_TOL and e_db < BWD_WEIGHT_TOL
    if name == "chunk-1536":
        # the same samples as the windows of tracks: same kernels, same summation order -> bit-equal. A track's windows
        # overlap, so the dense x is rebuilt from the tracks (dy and the mask do not depend on x)
        Bt, T, hop = C.BWD_WINDOW
        assert Bt * T == B
        track = gen(Bt, (T - 1) * hop + L, seed=6).to(DEV)
        dense = track.unfold(-1, L, hop).contiguous().view(B, 1, L)
        dw_w, db_w = k.conv1d_bwd_weight_windows(track, T, hop, L, dy, ks, s, p, with_bias=True, **kw)
        dw_d, db_d = k.conv1d_bwd_weight(dense, dy, ks, s, p, with_bias=True, **kw)
        assert torch.equal(dw_w, dw_d) and torch.equal(db_w, db_d)
