"""Host half of the beat-alignment metric (music2dance_amd.metrics): the mel bands and the DFT
table against the numpy statement of tests/beat_cases.py; that statement against numpy's FFT; that the shared inputs
leave few frames near a tie (so the device's event masks can be held to the fp64 ones) and separate an aligned dance
from a shifted one; and the --beat-align flags and JSON keys of the two phase-3 scripts through a host stand-in."""
import json
import math

import numpy as np
import pytest
import torch

from tests import beat_cases as C

PARAMS = [(40, 1024, 16000), (40, 2048, 16000), (20, 256, 16000)]
CURVE_T = [5, 64, 257, 4099]
_CACHE = {}


def ref(name):
    """fp64 alignment of the shared inputs, computed once"""
    if name not in _CACHE:
        if name == "clicks":
            x = C.clicks(2024)
            _CACHE[name] = C.onset(C.band_energies(x, C.T_CLICKS, C.HOP, 1024, C.mel_bands(40, 1024, C.RATE)))
        elif name in ("aligned", "shifted"):
            p = C.dance(7, (0, 0, 0) if name == "aligned" else (5, 4, 6))
            _CACHE[name] = C.alignment(ref("clicks"), C.speed(p))
    return _CACHE[name]


@pytest.mark.parametrize("nb,n_fft,rate", PARAMS)
def test_mel_bands(nb, n_fft, rate):
    from music2dance_amd import metrics
    got = metrics.mel_bands(nb, n_fft, rate)
    assert got.dtype == np.float64 and got.shape == (nb, n_fft // 2 + 1)
    assert np.abs(got - C.mel_bands(nb, n_fft, rate)).max() <= 1e-12
    assert got.min() >= 0.0 and got.max() <= 1.0
    assert got.sum(axis=1).min() > 1.0          # no empty band (the smallest row sum is 2.9)
    assert np.array_equal(metrics.mel_bands(), metrics.mel_bands(40, 1024, 16000))


@pytest.mark.parametrize("n_fft", [256, 1024, 2048])
def test_dft_table_is_the_fp32_rounding_of_the_fp64_basis(n_fft):
    from music2dance_amd import metrics
    got = metrics.stft_table(n_fft)
    assert got.dtype == np.float32 and got.shape == (2, n_fft // 2 + 1, n_fft)
    assert np.array_equal(got, C.basis(n_fft).astype(np.float32))
    for bad in (1000, 128, 4096):
        with pytest.raises(ValueError):
            metrics.stft_table(bad)


@pytest.mark.parametrize("n_fft,hop", [(256, 100), (1024, 640), (2048, 640)])
def test_helper_dft_agrees_with_numpy_fft(n_fft, hop):
    x = 0.5 * np.random.default_rng(3).standard_normal((2, 9509))
    T = 9
    fr = C.frames(x, T, hop, n_fft)
    bs = C.basis(n_fft)
    spec = np.fft.rfft(fr * C.hann(n_fft), axis=2)
    re, im = fr @ bs[0].T, fr @ bs[1].T
    scale = np.abs(spec).max()
    assert np.abs(re - spec.real).max() <= 1e-9 * scale and np.abs(im - spec.imag).max() <= 1e-9 * scale
    # frame 0 starts before the track: its head is zeros
    assert hop // 2 - n_fft // 2 < 0 and not fr[:, 0, :n_fft // 2 - hop // 2].any()


def _near_ties(margin):
    """share of the frames of [1, T - 2] whose margin is below 1e-4, per row"""
    inner = margin[:, 1:-1]
    return (inner < 1e-4).mean(axis=1) if inner.shape[1] else np.zeros(len(margin))


def test_shared_inputs_have_few_near_ties():
    worst = 0.0
    for name in ("aligned", "shifted"):
        r = ref(name)
        for m in (r["kmargin"], r["mmargin"]):
            share = _near_ties(m)
            worst = max(worst, share.max())
            assert share.max() <= 0.05, (name, share)
    for T in CURVE_T:
        o, v = C.curves(5, T)
        r = C.alignment(o, v)
        for m in (r["kmargin"], r["mmargin"]):
            share = _near_ties(m)
            worst = max(worst, share.max())
            assert share.max() <= 0.05, (T, share)
    print("largest share of near-tie frames: %.4f" % worst)


def test_aligned_and_shifted_dances_separate():
    a, s = ref("aligned")["scores"], ref("shifted")["scores"]
    print("beat_align aligned %s shifted %s" % (a[:, 0], s[:, 0]))
    assert (a[:, 2:] > 0).all() and (s[:, 2:] > 0).all()
    assert (a[:, 0] >= 0.9).all(), a
    assert (s[:, 0] <= 0.3).all(), s
    o, v = C.curves(5, 5)
    r = C.alignment(o, v)["scores"]
    # T = 5: three candidate frames; this draw has no row with both kinds of event
    assert np.isnan(r[:, :2]).all()


def test_two_scan_distances_equal_the_definition():
    """scores_from_masks is the O(|K| |M|) definition; a hand-made case pins it"""
    K = np.zeros((1, 12), dtype=bool)
    M = np.zeros((1, 12), dtype=bool)
    K[0, [2, 9]] = True
    M[0, [3, 4, 10]] = True
    s = C.scores_from_masks(K, M, 2.0)[0]
    e = lambda d: math.exp(-d * d / 8.0)
    assert s[0] == pytest.approx((e(1) + e(1)) / 2) and s[1] == pytest.approx((e(1) + e(2) + e(1)) / 3)
    assert tuple(s[2:]) == (2, 3)


# ---------------------------------------------------------------------------------------------- flags and JSON
TODAY = ["jerk_real_mean", "jerk_real_std", "jerk_fake_mean", "jerk_fake_std", "confusion", "style_agreement",
         "n_sequences"]
BEAT_KEYS = ["beat_%s_%s_%s" % (n, tag, st) for n in ("align", "cover") for tag in ("real", "fake")
             for st in ("mean", "std")] + ["beat_defined_real", "beat_defined_fake"]


def test_flags_parse():
    from music2dance_amd.phase3 import evaluate, generate
    base = ["-c", "x.yaml", "-l", "run"]
    assert evaluate.parse_args(base + ["--classifier", "w.pt"]).beat_align is False
    assert evaluate.parse_args(base + ["--classifier", "w.pt", "--beat-align"]).beat_align is True
    assert generate.parse_args(base + ["--synthetic"]).beat_align is False
    assert generate.parse_args(base + ["--synthetic", "--beat-align"]).beat_align is True


def test_summary_keys_with_and_without_the_flag(monkeypatch):
    from music2dance_amd import kernels, metrics
    from music2dance_amd.phase3 import evaluate
    jerk = np.array([1.0, 2.0, 3.0, 5.0])
    pred = np.array([0, 1, 2, 3])
    off = evaluate.summary(jerk, jerk, pred, pred)
    assert list(off) == TODAY

    monkeypatch.setattr(kernels, "impl", lambda: C.NumpyBeatBackend())
    monkeypatch.setattr(metrics, "_BASIS", {})
    monkeypatch.setattr(metrics, "_BANDS", {})
    audio = torch.from_numpy(C.clicks(2024))
    real = torch.from_numpy(C.dance(7, (0, 0, 0))).reshape(3, C.T_CLICKS, 69)
    fake = torch.from_numpy(C.dance(7, (5, 4, 6))).reshape(3, C.T_CLICKS, 69).clone()
    fake[1] = fake[1, :1]                      # a dance that stands still: no kinematic beat, its score is undefined
    beat = evaluate.beat_rows(audio, real, fake, C.HOP, C.RATE)
    assert np.isnan(beat["fake"][0][1]) and np.isnan(beat["fake"][1][1])
    on = evaluate.summary(jerk, jerk, pred, pred, beat=beat)
    assert list(on)[:len(TODAY)] == TODAY and set(on) == set(TODAY + BEAT_KEYS)
    assert {k: on[k] for k in TODAY} == off
    assert on["beat_defined_real"] == 3 and on["beat_defined_fake"] == 2
    want = ref("aligned")["scores"]
    assert on["beat_align_real_mean"] == pytest.approx(want[:, 0].mean(), abs=1e-5)
    assert on["beat_cover_real_std"] == pytest.approx(want[:, 1].std(ddof=1), abs=1e-5)
    shifted = ref("shifted")["scores"][[0, 2]]
    assert on["beat_align_fake_mean"] == pytest.approx(shifted[:, 0].mean(), abs=1e-5)
    assert on["beat_align_real_mean"] >= 0.9 and on["beat_align_fake_mean"] <= 0.3
    # one defined row: a mean, no spread; none: neither - and strict JSON either way
    one = evaluate.beat_stats([0.5, np.nan], [0.25, np.nan], "real")
    assert one == {"beat_defined_real": 1, "beat_align_real_mean": 0.5, "beat_cover_real_mean": 0.25,
                   "beat_align_real_std": pytest.approx(float("nan"), nan_ok=True),
                   "beat_cover_real_std": pytest.approx(float("nan"), nan_ok=True)}
    none = evaluate.json_safe(evaluate.beat_stats([np.nan], [np.nan], "fake"))
    assert none["beat_defined_fake"] == 0 and none["beat_align_fake_mean"] is None
    json.dumps(evaluate.json_safe(on), allow_nan=False)


def test_metrics_shapes_through_the_stand_in(monkeypatch):
    from music2dance_amd import kernels, metrics
    monkeypatch.setattr(kernels, "impl", lambda: C.NumpyBeatBackend())
    monkeypatch.setattr(metrics, "_BASIS", {})
    monkeypatch.setattr(metrics, "_BANDS", {})
    x = torch.from_numpy(C.clicks(2024))
    p = torch.from_numpy(C.dance(7, (0, 0, 0)))
    one = metrics.beat_scores(x[0], p[0], C.HOP, return_events=True)        # (N,) audio, (T, J, 3) poses: one row
    assert tuple(one["align"].shape) == (1,) and tuple(one["music_events"].shape) == (1, C.T_CLICKS)
    flat = metrics.beat_scores(x, p.reshape(3, C.T_CLICKS, 69), C.HOP)      # (B, T, 3 J)
    assert torch.equal(flat["align"][:1], one["align"]) and float(flat["align"].min()) >= 0.9
    assert int(one["n_music"][0]) == int(one["music_events"].sum())
    with pytest.raises(ValueError):
        metrics.beat_scores(x[:2], p, C.HOP)
    E = metrics.band_energies(x, 7, C.HOP, frame0=3)
    assert tuple(E.shape) == (3, 7, 40)
