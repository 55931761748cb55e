"""Host half of the audio-motion synchronisation (music2dance_amd.metrics sync_*, prepare_data --sync / --waltz-factor
auto, data.load_all(sync=True)): the estimate's rules on hand-made profiles, the planted offsets
recovered by the numpy statement of tests/sync_cases.py and by metrics.py through a host stand-in, the flags and files
of prepare_data, the loaders' trimming, and the binding table."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import sync_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
_CACHE = {}


def rule_curves(lag, stretch=1.0):
    """fp64 curves of the planted take, the values rounded to fp32 as the device holds them; computed once"""
    key = (lag, stretch)
    if key not in _CACHE:
        a, b = S.curves(S.audio()[0], S.dance(lag, stretch))
        _CACHE[key] = (a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64))
    return _CACHE[key]


@pytest.fixture
def host_backend(monkeypatch):
    from music2dance_amd import kernels, metrics, runner
    monkeypatch.setattr(kernels, "impl", lambda: S.NumpySyncBackend())
    monkeypatch.setattr(metrics, "_BASIS", {})
    monkeypatch.setattr(metrics, "_BANDS", {})
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ sync_estimate
def _est(rows, factors, L, n=None):
    from music2dance_amd import metrics
    r = np.asarray(rows, dtype=np.float64)
    n = np.full(r.shape, 100, dtype=np.int32) if n is None else np.asarray(n, dtype=np.int32)
    return metrics.sync_estimate(torch.from_numpy(r), torch.from_numpy(n), factors, L)


def test_estimate_ties_go_to_the_smallest_lag_then_the_first_factor():
    # L = 2, two factors: the top value 0.9 stands at (f0, l = +2), (f0, l = -1), (f1, l = -1) and (f1, l = +1)
    prof = [[[0.1, 0.9, 0.2, 0.3, 0.9], [0.0, 0.9, 0.1, 0.9, 0.2]]]
    n = [[[11, 12, 13, 14, 15], [21, 22, 23, 24, 25]]]
    (e,) = _est(prof, (1.0, 4.0), 2, n)
    assert (e["factor"], e["lag_frames"], e["r"], e["overlap"]) == (1.0, -1, 0.9, 12)
    # |l| decides before the factor index: (f1, l = 0) beats (f0, l = 1)
    (e,) = _est([[[0.0, 0.0, 0.1, 0.9, 0.0], [0.0, 0.0, 0.9, 0.1, 0.0]]], (1.0, 4.0), 2)
    assert (e["factor"], e["lag_frames"]) == (4.0, 0)
    # the statement of tests/sync_cases.py agrees
    want = S.estimate(np.asarray(prof[0]), (1.0, 4.0), 2)
    assert (want["factor"], want["lag_frames"]) == (1.0, -1)


def test_estimate_nan_handling_and_edges():
    # NaN cells never win; a row of NaN gives None everywhere and overlap 0
    rows = [[[NAN, 0.2, 0.5, 0.4, NAN]], [[NAN] * 5]]
    e0, e1 = _est(rows, (1.0,), 2)
    assert (e0["lag_frames"], e0["r"]) == (0, 0.5)
    assert e0["lag"] == pytest.approx(0.0 + 0.5 * (0.2 - 0.4) / (0.2 - 1.0 + 0.4))
    assert e0["r_second"] is None                      # every other defined cell lies inside |l - l*| <= 3
    assert e1 == {"factor": None, "lag_frames": None, "lag": None, "r": None, "r_second": None, "overlap": 0}
    # at the grid's edge and next to a NaN the refinement is the integer lag
    (e,) = _est([[[0.9, 0.2, 0.1, 0.0, 0.0]]], (1.0,), 2)
    assert (e["lag_frames"], e["lag"]) == (-2, -2.0)
    (e,) = _est([[[0.0, NAN, 0.9, 0.2, 0.1]]], (1.0,), 2)
    assert (e["lag_frames"], e["lag"]) == (0, 0.0)
    (e,) = _est([[[0.0, 0.5, 0.5, 0.5, 0.0]]], (1.0,), 2)      # a flat top: tie to |l| = 0, zero curvature
    assert (e["lag_frames"], e["lag"]) == (0, 0.0)
    with pytest.raises(ValueError):
        _est([[[0.0, 0.1, 0.2]]], (1.0,), 2)


def test_estimate_second_peak_window():
    L = 6
    prof = np.full((1, 2, 2 * L + 1), 0.05)
    prof[0, 0, L + 1] = 0.8            # the peak: f0, l = 1
    prof[0, 0, L + 4] = 0.7            # l = 4: inside the window, not a second peak
    prof[0, 0, L + 5] = 0.3            # l = 5: the first lag outside
    prof[0, 0, L - 3] = 0.4            # l = -3: |l - l*| = 4, outside
    prof[0, 1, L - 6] = 0.75           # another factor: not looked at
    (e,) = _est(prof, (1.0, 0.25), L)
    assert (e["factor"], e["lag_frames"], e["r"], e["r_second"]) == (1.0, 1, 0.8, 0.4)
    assert S.estimate(prof[0], (1.0, 0.25), L)["r_second"] == 0.4


# ------------------------------------------------------------------------------------------------ recovery
@pytest.mark.parametrize("lag", [0, 7, -11, 23])
def test_the_rule_recovers_planted_lags(lag):
    a, b = rule_curves(lag)
    r, n = S.profile(a, b, (1.0,), 40, 32)
    e = S.estimate(r[0], (1.0,), 40)
    print("lag %d: r %.4f r_second %.4f lag %.3f" % (lag, e["r"], e["r_second"], e["lag"]))
    assert e["lag_frames"] == lag and e["r"] - e["r_second"] >= 0.3
    assert abs(e["lag"] - lag) < 0.5
    # f = 1 pairs a[j] with b[j + l] exactly: the cell equals numpy's corrcoef of the two slices
    lo, hi = max(0, -lag), min(len(a[0]), len(b[0]) - lag)
    assert n[0, 0, lag + 40] == hi - lo
    assert r[0, 0, lag + 40] == pytest.approx(np.corrcoef(a[0, lo:hi], b[0, lo + lag:hi + lag])[0, 1], abs=1e-12)


def test_the_rule_recovers_planted_factors():
    a, b = rule_curves(7, 4.0)
    assert a.shape[1] == 400 and b.shape[1] == 1600
    r, _ = S.profile(a, b, (0.25, 4.0), 40, 32)
    e = S.estimate(r[0], (0.25, 4.0), 40)
    assert (e["factor"], e["lag_frames"]) == (0.25, 7) and np.nanmax(r[0, 1]) < 0.1 < 0.9 < e["r"]
    grid = (0.96, 0.98, 1.0, 1.02, 1.04)
    a, b = rule_curves(7, 1 / 1.02)
    r, _ = S.profile(a, b, grid, 40, 32)
    e = S.estimate(r[0], grid, 40)
    peaks = np.nanmax(r[0], axis=1)
    print("peaks over %s: %s" % (grid, peaks))
    assert (e["factor"], e["lag_frames"]) == (1.02, 7) and np.delete(peaks, 3).max() <= 0.3 < 0.7 <= peaks[3]


def test_metrics_through_the_stand_in(host_backend):
    """metrics.sync_curves / sync_profile / sync_estimate on host tensors equal the statement"""
    from music2dance_amd import metrics
    x = torch.from_numpy(S.audio()[0])
    p = torch.from_numpy(S.dance(-11))
    a, b = metrics.sync_curves(x, p, S.HOP)
    assert tuple(a.shape) == (1, 400) and tuple(b.shape) == (1, 400)
    wa, wb = rule_curves(-11)
    # (the stand-in rounds the band energies, the onset curve and the speed to fp32 on the way, as the device does)
    assert np.abs(a.double().numpy() - wa).max() <= 1e-6 * np.abs(wa).max()
    assert np.abs(b.double().numpy() - wb).max() <= 1e-6 * np.abs(wb).max()
    r, n = metrics.sync_profile(a, b, (1.0, 1.02), 40, 32)
    assert tuple(r.shape) == (1, 2, 81) and r.dtype == torch.float64 and n.dtype == torch.int32
    (e,) = metrics.sync_estimate(r, n, (1.0, 1.02), 40)
    want = S.estimate(r[0].numpy(), (1.0, 1.02), 40)
    assert {k: e[k] for k in want} == want and e["lag_frames"] == -11 and e["overlap"] == 389
    # one row given as 1-D curves, lengths as lists
    r1, _ = metrics.sync_profile(a[0], b[0], (1.0,), 40, 32, na=[400], nb=[400])
    assert torch.equal(r1[:, 0], r[:, 0])
    with pytest.raises(ValueError):
        metrics.sync_curves(x, torch.zeros(2, 10, 69), S.HOP)
    with pytest.raises(ValueError):
        metrics.sync_profile(a, b, (1.0,), 4, 2, na=[1, 2])


# ------------------------------------------------------------------------------------------------ data
def test_trimming_arithmetic_for_both_signs():
    from music2dance_amd import data as D
    assert D.sync_heads(7, 640) == (7, 0) and D.sync_heads(-11, 640) == (0, 7040) and D.sync_heads(0, 640) == (0, 0)
    take = {"skeletons": list(range(20)), "center": list(range(100, 120)), "length": 20}
    music = np.arange(20 * 4)
    t, m = D.apply_sync(take, music, {"lag_frames": 3, "hop": 4})
    assert t["skeletons"] == list(range(3, 20)) and t["center"] == list(range(103, 120)) and t["length"] == 17
    assert m is not None and np.array_equal(m, music) and take["length"] == 20 and len(take["skeletons"]) == 20
    t, m = D.apply_sync(take, music, {"lag_frames": -3, "hop": 4})
    assert t["skeletons"] == take["skeletons"] and np.array_equal(m, music[12:])


PLANTED, CFG, _folder, _run, _sync_files = S.PLANTED, S.CFG, S.planted_folder, S.run_prepare, S.sync_files


def test_default_synthetic_dataset_is_unchanged_by_the_planted_option(tmp_path):
    from music2dance_amd import data as D
    a = D.write_synthetic_dataset(str(tmp_path / "a"), n_takes=2, seconds=1)
    b = D.write_synthetic_dataset(str(tmp_path / "b"), n_takes=2, seconds=1, planted=None)
    for d in sorted(os.listdir(a)):
        for name in sorted(os.listdir(os.path.join(a, d))):
            assert open(os.path.join(a, d, name), "rb").read() == open(os.path.join(b, d, name), "rb").read()
    # (the default's bytes themselves: one take's wav is noise of 3000 rms, not clicks)
    from scipy.io import wavfile
    pcm = wavfile.read(os.path.join(a, "DANCE_C_1", "resampled_audio_extract.wav"))[1]
    assert 2500 < pcm.astype(np.float64).std() < 3500


def test_prepare_data_sync_flags_and_files(tmp_path, capsys, host_backend):
    from music2dance_amd import data as D
    from music2dance_amd import prepare_data
    opts = prepare_data.parse_args(["x"])
    assert (opts.sync, opts.max_lag, opts.min_peak, opts.waltz_factor, opts.factor_candidates) == \
        (False, 10.0, 0.0, None, (0.25, 4.0))
    assert prepare_data.parse_args(["x", "--waltz-factor", "auto"]).waltz_factor == "auto"
    assert prepare_data.parse_args(["x", "--waltz-factor", "0.5"]).waltz_factor == 0.5
    assert prepare_data.parse_args(["x", "--waltz-factor", "auto", "--factor-candidates", "0.5,2,3"]) \
        .factor_candidates == (0.5, 2.0, 3.0)
    with pytest.raises(SystemExit):
        prepare_data.parse_args(["x", "--factor-candidates", "0.5,-2"])

    folder = _folder(tmp_path)
    rep = _run([folder, "--sync", "--max-lag", "1.6", "--dry-run"], capsys)
    assert [t["sync"] for t in rep["takes"]] == ["would write"] * 3 and not _sync_files(folder)
    rep = _run([folder], capsys)
    assert all("sync" not in t for t in rep["takes"]) and not _sync_files(folder)

    rep = _run([folder, "--sync", "--max-lag", "1.6"], capsys)
    files = _sync_files(folder)
    assert sorted(files) == ["DANCE_C_1", "DANCE_R_2", "DANCE_T_3"]
    for take, (lag, _), entry in zip(sorted(files), PLANTED, rep["takes"]):
        js = files[take]
        assert set(js) == {"factor", "lag_frames", "lag", "r", "r_second", "overlap", "hop", "rate", "video_rate",
                           "max_lag_frames", "min_overlap", "accepted"}
        assert (js["lag_frames"], js["factor"], js["hop"], js["rate"], js["max_lag_frames"]) == (lag, 1.0, 640, 16000, 40)
        assert js["accepted"] is True and 200 <= js["min_overlap"] <= js["overlap"] and js["r"] - js["r_second"] >= 0.3
        assert entry["take"] == take and entry["sync"] == dict(js, file="written")

    # kept without --force, rewritten with it
    marker = os.path.join(folder, "DANCE_C_1", "sync.json")
    with open(marker, "w") as f:
        json.dump({"accepted": False, "lag_frames": 99, "hop": 640}, f)
    rep = _run([folder, "--sync", "--max-lag", "1.6"], capsys)
    assert [t["sync"] for t in rep["takes"]] == ["skipped: exists"] * 3
    assert json.load(open(marker))["lag_frames"] == 99
    # --min-peak above any margin: written, not accepted - and the loader then leaves the take alone
    rep = _run([folder, "--sync", "--max-lag", "1.6", "--force", "--min-peak", "5"], capsys)
    assert [t["sync"]["accepted"] for t in rep["takes"]] == [False] * 3
    assert [t["sync"]["lag_frames"] for t in rep["takes"]] == [5, -9, 0]
    plain = D.load_all(folder, ["C", "R", "T"])
    trimmed = D.load_all(folder, ["C", "R", "T"], sync=True)
    assert [len(t["skeletons"]) for t in plain[0]] == [len(t["skeletons"]) for t in trimmed[0]]
    assert all(np.array_equal(x, y) for x, y in zip(plain[1], trimmed[1]))


def test_dataset_trims_exactly_the_planted_heads(tmp_path, capsys, host_backend):
    from music2dance_amd import data as D
    folder = _folder(tmp_path)
    _run([folder, "--sync", "--max-lag", "1.6"], capsys)
    off = D.SequenceDataset(folder, CFG, dance_types=("C", "R", "T"), withaudio=True)
    again = D.SequenceDataset(folder, CFG, dance_types=("C", "R", "T"), withaudio=True, sync=False)
    on = D.SequenceDataset(folder, CFG, dance_types=("C", "R", "T"), withaudio=True, sync=True)
    assert off.dirs == on.dirs == again.dirs and len(off) == 3
    lags = {"DANCE_C_1": 5, "DANCE_R_2": -9, "DANCE_T_3": 0}
    for i, d in enumerate(off.dirs):
        assert np.array_equal(off.sequences[i], again.sequences[i]) and np.array_equal(off.musics[i], again.musics[i])
        frames, samples = D.sync_heads(lags[os.path.basename(d)], 640)
        assert np.array_equal(on.sequences[i], off.sequences[i][frames:])
        assert np.array_equal(on.musics[i], off.musics[i][samples:])
        assert len(on.sequences[i]) == len(off.sequences[i]) - frames
        assert len(on.musics[i]) == len(off.musics[i]) - samples
    # a take without a file is left as it is
    os.remove(os.path.join(folder, "DANCE_C_1", "sync.json"))
    on = D.SequenceDataset(folder, CFG, dance_types=("C", "R", "T"), withaudio=True, sync=True)
    i = [os.path.basename(d) for d in on.dirs].index("DANCE_C_1")
    assert np.array_equal(on.sequences[i], off.sequences[i])


def test_waltz_factor_auto_writes_what_the_given_factor_writes(tmp_path, capsys, host_backend):
    outs = {}
    for name, flag in (("auto", "auto"), ("given", "0.25")):
        folder, take = S.slow_waltz_folder(tmp_path / name)
        rep = _run([folder, "--waltz-factor", flag, "--max-lag", "1.6"], capsys)
        outs[name] = (open(os.path.join(take, "new_skeletons.json"), "rb").read(), rep["takes"][0])
    assert outs["auto"][0] == outs["given"][0]
    rep = outs["auto"][1]
    assert rep["waltz"] == outs["given"][1]["waltz"] and rep["waltz"].startswith("written ")
    auto = rep["waltz_auto"]
    assert auto["chosen"] == 0.25 and [c["factor"] for c in auto["candidates"]] == [0.25, 4.0]
    assert auto["candidates"][0]["lag_frames"] == 4 and auto["candidates"][0]["r"] > 0.5
    assert auto["candidates"][1]["r"] is None or auto["candidates"][1]["r"] < 0.3
    assert "waltz_auto" not in outs["given"][1]
    # a dry run names the candidates and needs neither the scan nor a device
    folder, take = S.slow_waltz_folder(tmp_path / "dry")
    rep = _run([folder, "--waltz-factor", "auto", "--dry-run"], capsys)
    assert rep["takes"][0]["waltz"].startswith("would choose") and not os.path.exists(os.path.join(take, "new_skeletons.json"))


# ------------------------------------------------------------------------------------------------ the binding
def test_signatures_hold_the_new_entries_in_the_headers_order():
    from music2dance_amd import _lib
    new = ["m2d_gauss_smooth", "m2d_sync_scan_max_frames", "m2d_sync_scan"]
    names = list(_lib.SIGNATURES)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m2d.h")).read(), flags=re.S)
    order = [m for m in re.findall(r"\b(m2d_[a-z0-9_]+)\s*\(", text)]
    for name in new:
        assert name in names and name in order
    i = names.index("m2d_pairwise_mean_dist")      # the section stands behind the distribution scores' in the header
    assert names[i + 1:i + 4] == new and order[order.index("m2d_pairwise_mean_dist") + 1:][:3] == new
    res, args = _lib.SIGNATURES["m2d_sync_scan"]
    assert len(args) == 16
    from music2dance_amd.kernels import HipKernels
    assert callable(HipKernels.gauss_smooth) and callable(HipKernels.sync_scan)
