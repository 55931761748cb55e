"""Shared cases of the augmentation tests (tests/test_augment_host.py, tests/test_gpu_augment.py): a small store -
audio_rate 1600, video_rate 25 (hop 64), seq_length 0.48 (T = 12, S = 768), three takes of 40, 23 and 61 frames with
tracks of matching length. Every value is fp32-representable, so the host's fp64 and the device's fp32 start from the same
numbers; takes 0 and 2 are filled with values around 1e3, the middle take with values around 1: a read across a take
boundary cannot hide. The scaler is fitted on the store and the poses are kept AS THEY ARE (the dataset is built without
a scaler and `pose_scaler` is set afterwards): the transform's un-scale / re-scale then runs with an honest per-column
scale and shift, and no value is re-rounded on the way into the store."""
import math

import numpy as np

from music2dance_amd import data as D

CONFIG = {"audio_rate": 1600, "video_rate": 25, "seq_length": 0.48, "feat_size": 69}
HOP, T, S = 64, 12, 768
FRAMES = (40, 23, 61)
SPEEDS = ((4, 5), (1, 1), (5, 4), (24, 25), (25, 24))
U = 2.0 ** -24


def takes(seed=7):
    """-> (poses [(L, 23, 3)], tracks [(L hop,)]) fp64 arrays of fp32-representable values"""
    rng = np.random.default_rng(seed)
    poses, tracks = [], []
    for n, L in enumerate(FRAMES):
        big = 1.0 if n == 1 else 1000.0
        p = big * (1.0 + 0.3 * rng.standard_normal((L, 23, 3))) if n != 1 else rng.standard_normal((L, 23, 3))
        a = big * (1.0 + 0.3 * rng.standard_normal(L * HOP)) if n != 1 else 0.5 * rng.standard_normal(L * HOP)
        poses.append(p.astype(np.float32).astype(np.float64))
        tracks.append(a.astype(np.float32).astype(np.float64))
    return poses, tracks


def scaler(poses):
    return D.MinMaxScaler().fit(np.concatenate(poses).reshape(-1, 69))


def dataset(augment=None, withaudio=True, crop_seed=3):
    poses, tracks = takes()
    state = {"sequences": poses, "labels": np.asarray([0, 1, 2]), "dirs": ["take_A", "take_B", "take_C"],
             "musics": tracks}
    ds = D.SequenceDataset(state, CONFIG, resume=True, withaudio=withaudio, augment=augment,
                           crop_rng=np.random.RandomState(crop_seed))
    ds.pose_scaler = scaler(poses)
    assert (ds.stick_length, ds.audio_length, ds.ratio) == (T, S, HOP)
    return ds


def params(a=1, b=1, mirror=False, deg=0.0, gain=1.0):
    th = math.radians(deg)
    return D.AugmentParams(a, b, mirror, math.cos(th), math.sin(th), gain)


def last_start(L, a, b):
    """the last admissible window start of a take of L frames: starts are drawn from [0, L - need)"""
    return L - D.frames_needed(T, a, b) - 1


def scipy_audio(track, a0, n_out, a, b, taps=None, absolute=False):
    """The audio rule through scipy.signal.resample_poly on the shifted, zero-padded take: pad in front by k a - a0,
    take the outputs from k b, k = ceil(a0 / a). absolute: |taps| over |x| (the sum the error bound is made of)."""
    from scipy.signal import resample_poly
    taps = D.speed_taps(a, b) if taps is None else taps
    x = np.asarray(track, dtype=np.float64)
    if absolute:
        taps, x = np.abs(taps), np.abs(x)
    if a == b:
        y = np.concatenate([x[a0:], np.zeros(n_out)])[:n_out]
        return y
    k = -(-a0 // a)
    padded = np.concatenate([np.zeros(k * a - a0), x, np.zeros((n_out + 2) * a + len(taps))])
    return resample_poly(padded, b, a, window=taps / b, padtype="constant")[k * b:k * b + n_out]


def audio_bound(track, a0, a, b, gain, S=S):
    """|y - y64| <= (P + 4) 2^-24 g sum |tap| |x|, P = ceil(ntaps / up): the P-term fp32 dot product of
    tests/test_gpu_resample.py (P + 3) and one more rounding for the multiply by the gain"""
    ntaps = len(D.speed_taps(a, b))
    P = -(-ntaps // b)
    return (P + 4) * U * abs(gain) * scipy_audio(track, a0, S, a, b, absolute=True)


def pose_bound(take, p0, p, sc, T=T):
    """Running-error bound of the kernel's pose value against augment_window, from the fp64 intermediates; u = 2^-24
    (times 1 + 2^-10 for the second-order terms). The kernel's roundings, each weighted by what it acts on:
      interpolation (f != 0): f = fl(r / b), d = fl(x1 - x0), v = fma(f, d, x0):   E_v = u (2 |f d| + |V|)
      identity transform: E = E_v. Otherwise, per column with T = V - shift, U = T / scale:
      un-scale: shift and scale arrive rounded to fp32, one subtraction, one (correctly rounded) division:
                                                                   E_U = (E_v + u |shift| + u |T|) / |scale| + 2 u |U|
      rotation: c and s arrive rounded to fp32, s z is rounded, fma(c, x, .) rounds once:
                              E_X' = |c| E_Ux + |s| E_Uz + u (|c X| + 2 |s Z| + |X'|), the same for Z'; E_Y' = E_Uy
      re-scale: fma(U', scale, shift) with the rounded scale and shift:
                                                          E_out = |scale| E_U' + u (|U' scale| + |shift| + |out|)
    -> (T, 23, 3) bounds."""
    u = U * (1.0 + 2.0 ** -10)
    x = np.asarray(take, dtype=np.float64).reshape(len(take), -1)
    ia = np.arange(T, dtype=np.int64) * p.a
    j, r = p0 + ia // p.b, ia % p.b
    f = (r / float(p.b))[:, None]
    nxt = np.minimum(j + 1, len(x) - 1)
    d = x[nxt] - x[j]
    V = x[j] + f * d
    Ev = np.where(f == 0.0, 0.0, u * (2.0 * np.abs(f * d) + np.abs(V)))
    if not p.mirror and p.cos == 1.0 and p.sin == 0.0:
        return Ev.reshape(T, -1, 3)
    scale, shift = (1.0, 0.0) if sc is None else (np.asarray(sc.scale_), np.asarray(sc.min_))
    Tm = V - shift
    Um = Tm / scale
    EU = ((Ev + u * np.abs(shift) + u * np.abs(Tm)) / np.abs(scale) + 2.0 * u * np.abs(Um)).reshape(T, -1, 3)
    Um = Um.reshape(T, -1, 3)
    X, Y, Z = (-Um[..., 0] if p.mirror else Um[..., 0]), Um[..., 1], Um[..., 2]
    c, s = p.cos, p.sin
    Xr, Zr = c * X + s * Z, -s * X + c * Z
    EX = abs(c) * EU[..., 0] + abs(s) * EU[..., 2] + u * (np.abs(c * X) + 2.0 * np.abs(s * Z) + np.abs(Xr))
    EZ = abs(c) * EU[..., 2] + abs(s) * EU[..., 0] + u * (np.abs(c * Z) + 2.0 * np.abs(s * X) + np.abs(Zr))
    Ur = np.stack((Xr, Y, Zr), axis=-1).reshape(T, -1)
    EUr = np.stack((EX, EU[..., 1], EZ), axis=-1).reshape(T, -1)
    out = Ur * scale + shift
    E = np.abs(scale) * EUr + u * (np.abs(Ur * scale) + np.abs(shift) + np.abs(out))
    return E.reshape(T, -1, 3)
