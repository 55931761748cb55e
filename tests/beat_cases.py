"""The beat-alignment metric of music2dance_amd.metrics restated in plain numpy (fp64 unless a dtype is asked for),
written from the definition and independently of metrics.py, and the input recipes
the beat tests share. A helper, not a test module."""
import math

import numpy as np

RATE, HOP, T_CLICKS, PER = 16000, 640, 120, (10, 8, 13)


# ------------------------------------------------------------------------------------------------ the definition
def mel_bands(nb, n_fft, rate):
    mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
    lo, hi = mel(0.0), mel(rate / 2.0)
    f = [700.0 * (10.0 ** ((lo + (hi - lo) * i / (nb + 1)) / 2595.0) - 1.0) for i in range(nb + 2)]
    out = np.zeros((nb, n_fft // 2 + 1))
    for b in range(nb):
        for k in range(n_fft // 2 + 1):
            F = k * rate / n_fft
            out[b, k] = max(0.0, min((F - f[b]) / (f[b + 1] - f[b]), (f[b + 2] - F) / (f[b + 2] - f[b + 1])))
    return out


def hann(n_fft):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)


def basis(n_fft):
    """(2, nbins, n_fft) fp64: [w cos; -w sin] of 2 pi ((n k) mod n_fft) / n_fft"""
    n = np.arange(n_fft)
    k = np.arange(n_fft // 2 + 1)
    arg = 2.0 * np.pi * ((k[:, None] * n[None, :]) % n_fft) / n_fft
    w = hann(n_fft)
    return np.stack([w * np.cos(arg), -(w * np.sin(arg))])


def frames(x, T, hop, n_fft, frame0=0):
    """(B, T, n_fft): the windows of frames frame0 .. frame0 + T - 1, zeros outside the track (no window applied)"""
    x = np.atleast_2d(x)
    B, S = x.shape
    out = np.zeros((B, T, n_fft), dtype=x.dtype)
    for i in range(T):
        s = (frame0 + i) * hop + hop // 2 - n_fft // 2
        lo, hi = max(s, 0), min(s + n_fft, S)
        if hi > lo:
            out[:, i, lo - s:hi - s] = x[:, lo:hi]
    return out


def band_energies(x, T, hop, n_fft, bands, frame0=0, dtype=np.float64):
    """(B, T, nb), every operation in `dtype`"""
    fr = frames(np.asarray(x, dtype=dtype), T, hop, n_fft, frame0)
    bs = basis(n_fft).astype(dtype)
    re = fr @ bs[0].T
    im = fr @ bs[1].T
    P = re * re + im * im
    return P @ np.asarray(bands, dtype=dtype).T


def onset(E, gamma=1.0):
    L = np.log1p(gamma * np.asarray(E, dtype=np.float64))
    o = np.zeros(L.shape[:2])
    o[:, 1:] = np.maximum(0.0, L[:, 1:] - L[:, :-1]).mean(axis=2)
    return o


def speed(p):
    p = np.asarray(p, dtype=np.float64)
    p = p.reshape(p.shape[0], p.shape[1], -1, 3)
    v = np.zeros(p.shape[:2])
    v[:, 1:] = np.sqrt(((p[:, 1:] - p[:, :-1]) ** 2).sum(axis=3)).mean(axis=2)
    v[:, 0] = v[:, 1]
    return v


def smooth(c, sigma):
    """-> (g(c, sigma), sum w |c| / sum w), both (B, T)"""
    c = np.asarray(c, dtype=np.float64)
    B, T = c.shape
    R = int(math.ceil(3.0 * sigma))
    num, mag, den = np.zeros((B, T)), np.zeros((B, T)), np.zeros(T)
    for j in range(-R, R + 1):
        w = math.exp(-j * j / (2.0 * sigma * sigma))
        lo, hi = max(0, -j), min(T, T - j)      # t with 0 <= t + j < T
        if hi > lo:
            num[:, lo:hi] += w * c[:, lo + j:hi + j]
            mag[:, lo:hi] += w * np.abs(c[:, lo + j:hi + j])
            den[lo:hi] += w
    return num / den, mag / den


def events(sm, music):
    """-> (mask (B, T) bool, margin (B, T)): the events of a smoothed curve and, per frame of [1, T - 2], the smallest
    of |s[t] - s[t - 1]|, |s[t] - s[t + 1]| and (music) |s[t] - mean|, relative to the row's max |s| (inf elsewhere)"""
    B, T = sm.shape
    mask = np.zeros((B, T), dtype=bool)
    margin = np.full((B, T), np.inf)
    if T < 3:
        return mask, margin
    a, b, d = sm[:, :-2], sm[:, 1:-1], sm[:, 2:]
    m = np.minimum(np.abs(b - a), np.abs(b - d))
    if music:
        mean = sm.mean(axis=1, keepdims=True)
        mask[:, 1:-1] = (b > a) & (b >= d) & (b > mean)
        m = np.minimum(m, np.abs(b - mean))
    else:
        mask[:, 1:-1] = (b < a) & (b <= d)
    scale = np.abs(sm).max(axis=1, keepdims=True)
    margin[:, 1:-1] = m / np.where(scale > 0, scale, 1.0)
    return mask, margin


def scores_from_masks(K, M, sigma_align=2.0):
    """-> (B, 4) fp64 [beat_align, beat_cover, |K|, |M|] of event masks (B, T), by the O(|K| |M|) definition"""
    out = np.full((len(K), 4), np.nan)
    for b in range(len(K)):
        k, m = np.flatnonzero(K[b]), np.flatnonzero(M[b])
        out[b, 2:] = len(k), len(m)
        if len(k) and len(m):
            d2 = ((k[:, None] - m[None, :]) ** 2).astype(np.float64)
            out[b, 0] = np.exp(-d2.min(axis=1) / (2.0 * sigma_align ** 2)).mean()
            out[b, 1] = np.exp(-d2.min(axis=0) / (2.0 * sigma_align ** 2)).mean()
    return out


def alignment(o, v, sigma_onset=1.0, sigma_speed=2.0, sigma_align=2.0):
    """-> dict: scores (B, 4), K, M (masks), osm, vsm (smoothed), omag, vmag (sum w |c| / sum w), kmargin, mmargin"""
    osm, omag = smooth(o, sigma_onset)
    vsm, vmag = smooth(v, sigma_speed)
    M, mmargin = events(osm, True)
    K, kmargin = events(vsm, False)
    return dict(scores=scores_from_masks(K, M, sigma_align), K=K, M=M, osm=osm, vsm=vsm, omag=omag, vmag=vmag,
                kmargin=kmargin, mmargin=mmargin)


def beat_scores(x, p, hop, rate=RATE, n_fft=1024, n_bands=40, gamma=1.0, **kw):
    p = np.asarray(p)
    E = band_energies(x, p.shape[1], hop, n_fft, mel_bands(n_bands, n_fft, rate))
    return alignment(onset(E, gamma), speed(p), **kw)


# ------------------------------------------------------------------------------------------------ the inputs
def clicks(seed):
    """(3, T hop - 300) fp32 at 16 kHz: noise with a decaying burst every PER[b] frames from frame 3 on"""
    rng = np.random.default_rng(seed)
    S = T_CLICKS * HOP - 300
    x = 0.05 * rng.standard_normal((len(PER), S))
    for b, per in enumerate(PER):
        p = 3 * HOP + 100
        while p < S:
            n = min(3000, S - p)
            x[b, p:p + n] += 0.8 * np.exp(-np.arange(n) / 400.0) * rng.standard_normal(n)
            p += per * HOP
    return x.astype(np.float32)


def dance(seed, shift):
    """(3, T, 23, 3) fp32: row b moves with speed 0.6 - 0.4 cos(2 pi (t - 3 - shift[b]) / PER[b]): slowest on the
    bursts of clicks() for shift 0"""
    rng = np.random.default_rng(seed)
    t = np.arange(T_CLICKS)
    rows = []
    for b, per in enumerate(PER):
        amp = 0.6 - 0.4 * np.cos(2.0 * np.pi * (t - 3 - shift[b]) / per)
        rows.append(np.cumsum(amp[:, None, None] * (1.0 + 0.2 * rng.standard_normal((T_CLICKS, 23, 3))), axis=0))
    return np.stack(rows).astype(np.float32)


def curves(seed, T):
    """two (4, T) uniform [0, 1) fp64 arrays (an onset and a speed curve)"""
    rng = np.random.default_rng(seed)
    return rng.random((4, T)), rng.random((4, T))


# ------------------------------------------------------------------------------------------------ a host backend
class NumpyBeatBackend:
    """The five HipKernels methods metrics.py calls, on host tensors through the fp64 statement above (for the host
    tests: monkeypatch kernels.impl with `lambda: NumpyBeatBackend()`)"""

    def stft_pack_basis(self, table):
        return table

    def stft_bands(self, x, n_frames, hop, n_fft, image, bands, frame0=0):
        import torch
        E = band_energies(x.double().numpy(), n_frames, hop, n_fft, bands.double().numpy(), frame0)
        return torch.from_numpy(E).float()

    def onset_flux(self, E, gamma=1.0):
        import torch
        return torch.from_numpy(onset(E.double().numpy(), gamma)).float()

    def motion_speed(self, poses):
        import torch
        return torch.from_numpy(speed(poses.double().numpy())).float()

    def beat_align(self, onset, speed, sigma_onset=1.0, sigma_speed=2.0, sigma_align=2.0, return_events=False):
        import torch
        r = alignment(onset.double().numpy(), speed.double().numpy(), sigma_onset, sigma_speed, sigma_align)
        scores = torch.from_numpy(r["scores"]).float()
        if not return_events:
            return scores
        return (scores, torch.from_numpy(r["K"].astype(np.uint8)), torch.from_numpy(r["M"].astype(np.uint8)),
                torch.from_numpy(r["osm"]).float(), torch.from_numpy(r["vsm"]).float())
