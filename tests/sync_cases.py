"""The audio-motion synchronisation of music2dance_amd.metrics restated in plain numpy fp64,
written from the definitions and independently of metrics.py, the planted takes the sync tests share, and a host
backend for the tests that need no GPU. A helper, not a test module."""
import json
import math
import os

import numpy as np

from tests import beat_cases as C

HOP, RATE, T_AUDIO = 640, 16000, 400
FACTORS = (1.0, 0.25, 4.0, 1.02)


# ------------------------------------------------------------------------------------------------ the definition
def smooth(c, sigma):
    """g(c, sigma), rows of a 2-D array (beat_cases.smooth is the statement of g)"""
    return C.smooth(np.atleast_2d(c), sigma)[0]


def curves(audio, poses, hop=HOP, rate=RATE, sigma_onset=1.0, sigma_speed=2.0):
    """-> (a (B, ceil(S / hop)), b (B, T)) fp64 from raw audio (B, S) and poses (B, T, J, 3)"""
    x = np.atleast_2d(np.asarray(audio, dtype=np.float64))
    p = np.asarray(poses, dtype=np.float64)
    p = p[None] if p.ndim == 3 else p
    T = -(-x.shape[1] // hop)
    o = C.onset(C.band_energies(x, T, hop, 1024, C.mel_bands(40, 1024, rate)))
    return smooth(o, sigma_onset), -smooth(C.speed(p), sigma_speed)


def cell(a, b, f, l, min_overlap):
    """(r, n) of one row, one factor, one lag: a (na,), b (nb,) fp64 arrays holding fp32 values"""
    na, nb = len(a), len(b)
    if na == 0 or nb == 0:
        return float("nan"), 0
    j = np.arange(na)
    x = (j + l).astype(np.float64) / f
    ok = (x >= 0) & (x <= nb - 1)
    n = int(ok.sum())
    if n < min_overlap:
        return float("nan"), n
    x = x[ok]
    i = np.floor(x).astype(np.int64)
    fr = x - i
    bv = b[i] + fr * (b[np.minimum(i + 1, nb - 1)] - b[i])
    av = a[ok]
    da, db = av - av.mean(), bv - bv.mean()
    sab, saa, sbb = float((da * db).sum()), float((da * da).sum()), float((db * db).sum())
    if saa == 0.0 or sbb == 0.0:
        return float("nan"), n
    return sab / math.sqrt(saa * sbb), n


def profile(a, b, factors, L, min_overlap, na=None, nb=None):
    """-> (r (B, F, 2 L + 1) fp64, n int32) of curves a (B, Ta), b (B, Tb)"""
    a, b = np.atleast_2d(np.asarray(a, dtype=np.float64)), np.atleast_2d(np.asarray(b, dtype=np.float64))
    B = len(a)
    r = np.full((B, len(factors), 2 * L + 1), np.nan)
    n = np.zeros(r.shape, dtype=np.int32)
    for row in range(B):
        ar = a[row, :a.shape[1] if na is None else int(na[row])]
        br = b[row, :b.shape[1] if nb is None else int(nb[row])]
        for i, f in enumerate(factors):
            for l in range(-L, L + 1):
                r[row, i, l + L], n[row, i, l + L] = cell(ar, br, float(f), l, min_overlap)
    return r, n


def estimate(r, factors, L):
    """One row's profile r (F, 2 L + 1) -> dict (factor, lag_frames, lag, r, r_second), by plain loops: the largest
    non-NaN r, ties to the smallest |l| then the smallest factor index; r_second outside |l - l*| <= 3 on the same
    factor; the parabola through the three cells around the peak"""
    best = None
    for i in range(len(factors)):
        for k in range(2 * L + 1):
            v = r[i, k]
            if math.isnan(v):
                continue
            key = (-v, abs(k - L), i)
            if best is None or key < best[0]:
                best = (key, i, k)
    if best is None:
        return dict(factor=None, lag_frames=None, lag=None, r=None, r_second=None)
    _, i, k = best
    second = [r[i, q] for q in range(2 * L + 1) if abs(q - k) > 3 and not math.isnan(r[i, q])]
    lag = float(k - L)
    if 0 < k < 2 * L and not math.isnan(r[i, k - 1]) and not math.isnan(r[i, k + 1]):
        den = r[i, k - 1] - 2.0 * r[i, k] + r[i, k + 1]
        if den != 0.0:
            lag += 0.5 * (r[i, k - 1] - r[i, k + 1]) / den
    return dict(factor=float(factors[i]), lag_frames=k - L, lag=lag, r=float(r[i, k]),
                r_second=max(second) if second else None)


# ------------------------------------------------------------------------------------------------ the planted takes
_AUDIO = {}


def audio(T=T_AUDIO, seed=5):
    """-> (x (T hop - 300,) fp32, the click frames): 0.05 N(0, 1) noise, click frames from 3 on, 6 to 14 apart, while
    < T - 2; each click a burst 0.8 exp(-k / 400) N(0, 1) of up to 3000 samples at c hop + 100"""
    if (T, seed) not in _AUDIO:
        rng = np.random.default_rng(seed)
        S = T * HOP - 300
        x = 0.05 * rng.standard_normal(S)
        clicks, c = [], 3
        while c < T - 2:
            clicks.append(c)
            c += int(rng.integers(6, 15))
        for c in clicks:
            p = c * HOP + 100
            n = min(3000, S - p)
            x[p:p + n] += 0.8 * np.exp(-np.arange(n) / 400.0) * rng.standard_normal(n)
        _AUDIO[(T, seed)] = (x.astype(np.float32), np.asarray(clicks))
    return _AUDIO[(T, seed)]


def dance(lag, stretch=1.0, T=T_AUDIO, seed=9):
    """(round(T stretch), 23, 3) fp32: the body slows to 0.2 of its speed at the clicks of audio(T), `lag` frames late;
    recorded `stretch` times slower"""
    clicks = audio(T)[1]
    rng = np.random.default_rng(seed)
    n = int(round(T * stretch))
    t = np.arange(n) / stretch
    near = np.exp(-(t[:, None] - clicks[None, :] - lag) ** 2 / (2.0 * 1.5 ** 2)).sum(axis=1)
    amp = 0.6 - 0.4 * np.minimum(1.0, near)
    return np.cumsum(amp[:, None, None] / stretch * (1.0 + 0.2 * rng.standard_normal((n, 23, 3))), axis=0) \
        .astype(np.float32)


def uniform_curves(seed, B, Ta, Tb, extra=7):
    """(B, Ta + extra), (B, Tb + extra) uniform [0, 1) fp32 buffers: the tests cut (B, Ta) / (B, Tb) rows out of them"""
    rng = np.random.default_rng(seed)
    return rng.random((B, Ta + extra)).astype(np.float32), rng.random((B, Tb + extra)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the script cases
PLANTED = [(5, 1.0), (-9, 1.0), (0, 1.0)]      # (lag, stretch) of the three takes of planted_folder
CFG = {"audio_rate": 16000, "video_rate": 25, "seq_length": 4, "feat_size": 69}


def strict_json(text):
    def refuse(c):
        raise AssertionError("non-standard JSON constant %s" % c)
    return json.loads(text, parse_constant=refuse)


def planted_folder(tmp_path, planted=PLANTED, styles="CRT", seconds=16):
    from music2dance_amd import data as D
    return D.write_synthetic_dataset(str(tmp_path / "data"), n_takes=len(planted), seconds=seconds, styles=styles,
                                     planted=planted)


def run_prepare(argv, capsys):
    """prepare_data.main(argv) -> the printed report, parsed as strict JSON"""
    from music2dance_amd import prepare_data
    prepare_data.main(argv)
    return strict_json(capsys.readouterr().out.strip().splitlines()[-1])


def sync_files(folder):
    """{take: its sync.json} of the takes that have one"""
    out = {}
    for d in sorted(os.listdir(folder)):
        path = os.path.join(folder, d, "sync.json")
        if os.path.exists(path):
            with open(path) as f:
                out[d] = strict_json(f.read())
    return out


def slow_waltz_folder(path, planted=(4, 4.0)):
    """one waltz take recorded `planted[1]` times slower, as the download has it: skeletons.json, no new_skeletons.json"""
    from music2dance_amd import data as D
    folder = D.write_synthetic_dataset(str(path), n_takes=1, seconds=8, styles="W", planted=[planted])
    take = os.path.join(folder, "DANCE_W_1")
    os.rename(os.path.join(take, "new_skeletons.json"), os.path.join(take, "skeletons.json"))
    return folder, take


# ------------------------------------------------------------------------------------------------ a host backend
class NumpySyncBackend(C.NumpyBeatBackend):
    """NumpyBeatBackend plus the methods of the synchronisation path, on host tensors through the statement above"""
    name = "numpy"

    def gauss_smooth(self, c, sigma):
        import torch
        return torch.from_numpy(smooth(c.double().numpy(), sigma)).float()

    def sync_scan_max_frames(self):
        return 16384

    def sync_scan(self, a, b, factors, max_lag, min_overlap, na=None, nb=None):
        import torch
        r, n = profile(a.double().numpy(), b.double().numpy(), list(factors), int(max_lag), int(min_overlap),
                       None if na is None else na.numpy(), None if nb is None else nb.numpy())
        return torch.from_numpy(r), torch.from_numpy(n)
