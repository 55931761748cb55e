"""Audio rate conversion on the device: a polyphase FIR resampler over m2d_resample_poly (include/m2d.h).

The reference converts its tracks to 16 kHz with `sox` (change_rate.py:6-8). Here the filter is scipy's own
`resample_poly` default (a Kaiser-windowed sinc, `design_taps`), applied by one HIP kernel. Output n of a track is a
pure function of its absolute index, so `StreamResampler` - the same conversion fed chunk by chunk at the source's own
rate - returns the bits of `resample` over the whole track, whatever the chunking.
"""
import math

import numpy as np
import torch

from . import kernels

_TAPS = {}  # (up, down, device) -> fp32 taps of the default design


def design_taps(up, down, zeros=10, beta=5.0):
    """-> (up', down', taps): the ratio reduced by its gcd and the float64 filter scipy.signal.resample_poly designs for
    it by default, firwin(2 zeros max(up', down') + 1, 1 / max(up', down'), window=('kaiser', beta)) * up'"""
    from scipy.signal import firwin
    up, down = int(up), int(down)
    if up <= 0 or down <= 0:
        raise ValueError("design_taps: up and down must be positive")
    g = math.gcd(up, down)
    up, down = up // g, down // g
    big = max(up, down)
    return up, down, firwin(2 * int(zeros) * big + 1, 1.0 / big, window=("kaiser", beta)) * up


def ratio(rate_in, rate_out):
    """(up, down) of a conversion rate_in -> rate_out, reduced"""
    rate_in, rate_out = int(rate_in), int(rate_out)
    if rate_in <= 0 or rate_out <= 0:
        raise ValueError("sample rates must be positive")
    g = math.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def out_len(n, up, down):
    """samples n samples become: ceil(n up / down)"""
    return -(-int(n) * int(up) // int(down))


def _device_taps(up, down, device, taps):
    """fp32 taps on `device`: the caller's, or the default design (made once per (up, down, device))"""
    device = torch.device(device)
    if taps is not None:
        t = torch.as_tensor(taps).detach().to(device=device, dtype=torch.float32).contiguous()
        if t.dim() != 1 or t.numel() % 2 == 0:
            raise ValueError("resampling taps: a 1-D filter of odd length expected")
        return t
    key = (up, down, str(device))
    t = _TAPS.get(key)
    if t is None:
        # equal rates: the one-tap identity (scipy's design would be a sinc cut at Nyquist; scipy copies then, too)
        design = np.ones(1) if up == down else design_taps(up, down)[2]
        t = _TAPS[key] = torch.as_tensor(design, dtype=torch.float32).to(device)
    return t


def _rows(x):
    x = torch.as_tensor(x)
    if x.dim() == 1:
        x = x.unsqueeze(0)
    if x.dim() != 2:
        raise ValueError("audio rows: (N,) or (B, N) samples expected, got %s" % (tuple(x.shape),))
    return x


def resample(x, rate_in, rate_out, taps=None):
    """x (N,) or (B, N) fp32 samples on the device at rate_in Hz -> (B, ceil(N up / down)) at rate_out Hz; zero phase,
    zeros outside the track (scipy.signal.resample_poly(x, up, down, padtype='constant') with the same window)"""
    x = _rows(x)
    up, down = ratio(rate_in, rate_out)
    t = _device_taps(up, down, x.device, taps)
    return kernels.impl().resample_poly(x, 0, t, up, down, 0, out_len(x.shape[1], up, down))


class StreamResampler:
    """`resample` for B tracks that arrive in pieces. push(chunk (B, n)) -> (B, k): every output whose whole filter
    window has been received, (n down + half) // up <= received - 1; flush() -> the rest, up to ceil(received up /
    down) outputs in all, the missing future counting as zeros. The carry holds only the samples the next output can
    still read. All pushes and the flush, concatenated, equal resample(whole track) bit for bit."""

    def __init__(self, rate_in, rate_out, batch=1, device="cuda", taps=None):
        self.up, self.down = ratio(rate_in, rate_out)
        self.batch = int(batch)
        if self.batch <= 0:
            raise ValueError("StreamResampler: batch must be positive")
        self.device = torch.device(device)
        self.taps = _device_taps(self.up, self.down, self.device, taps)
        self.ntaps = self.taps.numel()
        self.half = (self.ntaps - 1) // 2
        self.carry = torch.zeros((self.batch, 0), dtype=torch.float32, device=self.device)
        self.carry0 = 0      # absolute index of carry[:, 0]
        self.received = 0    # samples pushed so far
        self.emitted = 0     # outputs returned so far (= index of the next output)
        self.closed = False

    def _emit(self, buf, end):
        k = end - self.emitted
        if k <= 0:
            return torch.zeros((self.batch, 0), dtype=torch.float32, device=self.device), buf
        y = kernels.impl().resample_poly(buf, self.carry0, self.taps, self.up, self.down, self.emitted, k)
        self.emitted = end
        # the next output's earliest sample: the smallest m with emitted down + half - m up < ntaps
        first = max(0, (self.emitted * self.down + self.half - self.ntaps) // self.up + 1)
        drop = min(first, self.received) - self.carry0
        if drop > 0:
            buf = buf[:, drop:]
            self.carry0 += drop
        return y, buf

    def push(self, chunk):
        if self.closed:
            raise RuntimeError("StreamResampler: push after flush")
        x = _rows(chunk)
        if x.shape[0] != self.batch:
            raise ValueError("StreamResampler.push: (%d, n) samples expected, got %s" % (self.batch, tuple(x.shape)))
        x = x.to(device=self.device, dtype=torch.float32)
        buf = torch.cat((self.carry, x), 1) if self.carry.shape[1] else x
        self.received += x.shape[1]
        # output n is complete when n down + half <= received up - 1
        end = max(0, (self.received * self.up - 1 - self.half) // self.down + 1)
        y, self.carry = self._emit(buf, end)
        return y

    def flush(self):
        if self.closed:
            raise RuntimeError("StreamResampler: flushed twice")
        self.closed = True
        y, self.carry = self._emit(self.carry, out_len(self.received, self.up, self.down))
        return y
