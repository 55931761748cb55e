"""Host side of the polyphase resampler (audio.py, data.retime_sequence, prepare_data), no GPU needed:
  * design_taps is scipy's default resample_poly filter, bit for bit in fp64, over the reduced ratio;
  * StreamResampler's bookkeeping (which outputs a push completes, what the carry keeps, the flush) against an fp64
    stand-in for m2d_resample_poly that restates the header's formula: every chunking gives scipy's resample_poly;
  * retime_sequence: endpoints, halving, identity, and no read past the end when i * delta rounds off the last index;
  * prepare_data --dry-run lists the work without a device and writes nothing."""
import json

import numpy as np
import pytest
import torch

from music2dance_amd import kernels
from tests.fake_backend import FakeKernels
from tests.resample_cases import chunkings, listing, raw_folder


class ResampleFakeKernels(FakeKernels):
    """m2d_resample_poly by its definition (include/m2d.h) in fp64: y[n] = sum_m taps[n down + half - m up] X[m]"""
    def resample_poly(self, x, x0, taps, up, down, n0, ny, out=None):
        x, taps = x.double(), taps.double()
        B, nx = x.shape
        ntaps = taps.numel()
        assert ntaps % 2 == 1 and np.gcd(up, down) == 1 and x0 >= 0 and n0 >= 0 and ny >= 0
        half = (ntaps - 1) // 2
        n = torch.arange(n0, n0 + ny, dtype=torch.int64)
        t = n * down + half
        j = torch.arange(-(-ntaps // up), dtype=torch.int64)
        k = (t % up)[:, None] + j[None, :] * up                                  # tap index, (ny, P)
        m = torch.div(t, up, rounding_mode="floor")[:, None] - j[None, :] - x0   # column of x
        ok = (k < ntaps) & (m >= 0) & (m < nx)
        if nx == 0:
            return torch.zeros((B, ny), dtype=torch.float64)
        tv = taps[k.clamp(max=ntaps - 1)] * ok
        xv = x[:, m.clamp(0, nx - 1)]                                            # (B, ny, P)
        return (xv * tv[None]).sum(-1)


@pytest.fixture
def fake():
    prev = kernels.set_impl(ResampleFakeKernels())
    try:
        yield
    finally:
        kernels.set_impl(prev)


def test_design_taps_is_scipys_default_filter():
    from scipy.signal import firwin
    from music2dance_amd import audio as A
    up, down, taps = A.design_taps(16000, 44100)
    assert (up, down) == (160, 441) and taps.dtype == np.float64 and len(taps) == 2 * 10 * 441 + 1
    assert np.array_equal(taps, firwin(2 * 10 * 441 + 1, 1.0 / 441, window=("kaiser", 5.0)) * 160)
    up, down, taps = A.design_taps(4, 2)
    assert (up, down) == (2, 1) and np.array_equal(taps, firwin(41, 0.5, window=("kaiser", 5.0)) * 2)
    # the largest table among the common rates stays under the kernel's cap
    assert len(A.design_taps(16000, 11025)[2]) == 12801 <= 16384
    assert A.ratio(44100, 16000) == (160, 441) and A.out_len(30000, 160, 441) == 10885


@pytest.mark.parametrize("name", ["ones", "441s", "mixed"])
def test_stream_bookkeeping_gives_scipys_resample_poly(fake, name):
    from scipy.signal import resample_poly
    from music2dance_amd import audio as A
    B, N = 2, 30000
    g = torch.Generator().manual_seed(3)
    x = 0.3 * torch.randn(B, N, generator=g)
    rs = A.StreamResampler(44100, 16000, batch=B, device="cpu")
    up, down, half, ntaps = rs.up, rs.down, rs.half, rs.ntaps
    assert (up, down, ntaps) == (160, 441, 8821)
    want = resample_poly(x.double().numpy(), up, down, axis=1, window=rs.taps.double().numpy() / up,
                         padtype="constant")
    short = A.StreamResampler(44100, 16000, batch=B, device="cpu")
    assert tuple(short.push(x[:, :3]).shape) == (B, 0)       # a push too short to complete an output
    assert short.carry.shape[1] == 3 and short.emitted == 0
    parts, pos = [], 0
    sizes = chunkings(N)[name]
    assert sum(sizes) == N
    for n in sizes:
        y = rs.push(x[:, pos:pos + n])
        pos += n
        parts.append(y)
        # exactly the outputs whose whole window has arrived
        assert rs.emitted == max(0, (pos * up - 1 - half) // down + 1)
        assert (rs.emitted * down + half) // up > pos - 1
        # the carry starts at the next output's first sample and is shorter than one window of P = ceil(ntaps / up)
        lo = max(0, (rs.emitted * down + half - ntaps) // up + 1)
        assert rs.carry0 == min(lo, pos) and rs.carry0 + rs.carry.shape[1] == pos
        assert rs.carry.shape[1] < -(-ntaps // up)
    assert pos == N
    parts.append(rs.flush())
    got = torch.cat(parts, 1)
    assert got.shape == (B, -(-N * up // down)) == want.shape
    assert float(np.abs(got.numpy() - want).max()) <= 1e-12
    one = A.resample(x, 44100, 16000)
    assert one.shape == got.shape and float((one - got).abs().max()) <= 1e-12
    with pytest.raises(RuntimeError):
        rs.push(x[:, :1])
    with pytest.raises(RuntimeError):
        rs.flush()


def test_equal_rates_pass_through(fake):
    from music2dance_amd import audio as A
    x = torch.randn(1, 100, generator=torch.Generator().manual_seed(0))
    assert torch.equal(A.resample(x[0], 16000, 16000).float(), x)
    rs = A.StreamResampler(16000, 16000, device="cpu")
    got = torch.cat([rs.push(x[:, :37]), rs.push(x[:, 37:]), rs.flush()], 1)
    assert torch.equal(got.float(), x)


def test_retime_sequence():
    from music2dance_amd.data import retime_sequence
    rng = np.random.RandomState(0)
    x = rng.randn(11, 23, 3)
    for new_len in (2, 5, 6, 11, 12, 40):
        y = retime_sequence(x, new_len)
        assert y.shape == (new_len, 23, 3) and y.dtype == np.float64
        assert np.array_equal(y[0], x[0]) and np.array_equal(y[-1], x[-1])       # endpoints exact
    assert np.array_equal(retime_sequence(x, 6), x[::2])                         # a halving: every second frame
    assert np.array_equal(retime_sequence(x, 11), x)                             # same length: the identity
    y = retime_sequence(x, 21)                                                   # a doubling: midpoints in between
    assert np.array_equal(y[::2], x) and np.allclose(y[1::2], 0.5 * (x[:-1] + x[1:]), rtol=0, atol=1e-15)
    # the reference's recipe, element by element, where it stays inside the take
    delta = 10 / 6.0
    y = retime_sequence(x, 7)
    for i in range(6):
        k, f = int(i * delta), i * delta - int(i * delta)
        assert np.array_equal(y[i], x[k] if f < np.finfo(float).eps else x[k] + f * (x[k + 1] - x[k]))
    # lengths at which (new_len - 1) * delta does not round to len - 1 exactly: no index error, last frame kept
    hits = 0
    for n in range(2, 60):
        for new_len in range(2, 80):
            last = (new_len - 1) * ((n - 1) / float(new_len - 1))
            hits += last != n - 1
            z = np.arange(n, dtype=np.float64)
            out = retime_sequence(z, new_len)
            assert out[-1] == n - 1 and out[0] == 0 and np.all(np.diff(out) >= 0)
            assert np.allclose(out, np.linspace(0, n - 1, new_len), rtol=0, atol=1e-12)
    assert hits > 0
    assert np.array_equal(retime_sequence(x[:1], 3), np.repeat(x[:1], 3, axis=0))
    with pytest.raises(ValueError):
        retime_sequence(x, 0)


def test_prepare_data_dry_run_needs_no_device(tmp_path, capsys):
    from music2dance_amd import prepare_data
    folder = raw_folder(str(tmp_path / "raw"))
    before = listing(folder)
    rep = prepare_data.main([folder, "--dry-run", "--waltz-factor", "0.5"])
    assert json.loads(capsys.readouterr().out) == json.loads(json.dumps(rep))
    assert listing(folder) == before and rep["dry_run"] is True and rep["rate"] == 16000
    takes = {t["take"]: t for t in rep["takes"]}
    assert sorted(takes) == ["DANCE_C_1", "DANCE_R_2", "DANCE_T_3", "DANCE_W_4"]
    assert takes["DANCE_C_1"]["rate_in"] == 44100 and takes["DANCE_C_1"]["samples_in"] == 88200
    assert takes["DANCE_C_1"]["samples_out"] == 32000 and takes["DANCE_R_2"]["samples_out"] == 32000
    assert takes["DANCE_T_3"]["samples_out"] == takes["DANCE_T_3"]["samples_in"] == 32000
    assert all(t["audio"] == "would write" for t in rep["takes"])
    assert takes["DANCE_W_4"]["waltz"].startswith("would write") and "waltz" not in takes["DANCE_C_1"]
    # without the factor the waltz take is reported, not touched
    rep = prepare_data.main([folder, "--dry-run"])
    assert {t["take"]: t for t in rep["takes"]}["DANCE_W_4"]["waltz"].startswith("needs re-timing")
    with pytest.raises(SystemExit):
        prepare_data.main([str(tmp_path / "nowhere"), "--dry-run"])
