"""From the published Music-to-Dance-Motion-Synthesis download to the files the loaders read (data.load_all).

    python -m music2dance_amd.prepare_data <folder> [--rate 16000] [--waltz-factor F | auto] [--sync] [--force]
                                           [--dry-run] [-d N]

For every DANCE_* folder that does not end in `bis`:
  * audio_extract.wav (any PCM or float format, any channel count: data._read_wav) is resampled ON THE DEVICE to --rate
    (audio.resample: m2d_resample_poly with scipy's default resample_poly filter) and written as
    resampled_audio_extract.wav, 16-bit mono PCM, rint(y * 32768) clipped to [-32768, 32767], no dither. The reference
    does this with `sox` (change_rate.py:6-8). A source already at --rate is written without filtering. Existing
    outputs are kept unless --force.
  * with --waltz-factor F, a waltz folder (DANCE_W_*) that has skeletons.json but no new_skeletons.json gets one:
    `skeletons` and `center` re-timed to round(len * F) frames (data.retime_sequence, the reference's
    utils.interpolate recipe), `length` updated. The factor has no default: the reference does not state it, and its
    README's "4 times slower" can be read both ways. Without the flag such folders are reported and left alone.
  * with --waltz-factor auto [--factor-candidates 0.25,4] the factor of such a folder is measured: the raw take's
    motion curve is correlated with the music's onset curve at every candidate and every lag up to --max-lag
    (metrics.sync_curves / sync_profile: m2d_sync_scan), the candidate with the largest peak is used as a given
    --waltz-factor would be, and every candidate's peak goes into the report (`waltz_auto`).
  * with --sync [--max-lag SECONDS=10] [--min-peak X=0] [--video-rate 25], after those two steps and therefore on the
    files the loaders will read, every take's audio-motion offset is estimated: the curves of
    all takes are padded into batches, one scan launch a batch at factor 1 with min_overlap = max(64, half the shorter
    curve), and <take>/sync.json is written: factor, lag_frames (> 0: the motion lags the audio), lag, r, r_second,
    overlap, hop, rate, video_rate, max_lag_frames, min_overlap and accepted = (r - r_second >= min_peak). The loaders
    use the file only when asked (data.load_all(sync=True), YAML key dataset.sync). An existing file is kept unless
    --force. The method is verified on planted offsets only; --min-peak has no tuned default.
One JSON report is printed: per take the rate in, the samples in and out, and what was written or skipped.
--dry-run writes nothing and needs no device.
"""
import argparse
import json
import os

import numpy as np

SOURCE_WAV = "audio_extract.wav"
TARGET_WAV = "resampled_audio_extract.wav"


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("folder", type=str, help="the dataset folder (holds the DANCE_* folders)")
    ap.add_argument("--rate", type=int, default=16000, help="target sample rate in Hz")
    ap.add_argument("--waltz-factor", type=_factor_or_auto, default=None,
                    help="re-time the waltz takes to round(len * F) frames (no default); 'auto': the candidate of "
                         "--factor-candidates whose motion curve correlates best with the music")
    ap.add_argument("--factor-candidates", type=_factor_list, default=(0.25, 4.0),
                    help="comma-separated factors --waltz-factor auto chooses from")
    ap.add_argument("--sync", action="store_true", help="estimate every take's audio-motion offset into sync.json")
    ap.add_argument("--max-lag", type=float, default=10.0, help="largest offset searched, in seconds")
    ap.add_argument("--min-peak", type=float, default=0.0,
                    help="accept an estimate when its peak stands this far above the second one")
    ap.add_argument("--video-rate", type=float, default=25.0, help="pose frames a second")
    ap.add_argument("--force", action="store_true", help="rewrite outputs that exist")
    ap.add_argument("--dry-run", action="store_true", help="report the work, write nothing")
    ap.add_argument("-d", "--device", type=int, default=None, help="choose gpu id")
    return ap.parse_args(argv)


def _factor_or_auto(text):
    return "auto" if text == "auto" else float(text)


def _factor_list(text):
    vals = tuple(float(t) for t in text.split(",") if t.strip())
    if not vals or not all(np.isfinite(v) and v > 0 for v in vals):
        raise argparse.ArgumentTypeError("positive factors expected, got %r" % (text,))
    return vals


def to_pcm16(y):
    """float samples in [-1, 1) -> int16: rint(y * 32768) clipped, no dither"""
    return np.clip(np.rint(np.asarray(y, dtype=np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)


def _wav_header(path):
    """(rate, samples per channel) without reading the data"""
    from scipy.io import wavfile
    rate, data = wavfile.read(path, mmap=True)
    return int(rate), int(data.shape[0])


def _audio(directory, opts, device):
    """-> the take's audio entry of the report; `device`: callable returning the torch device (asked for on first use)"""
    from scipy.io import wavfile
    from . import audio as A
    from .data import _read_wav
    src, dst = os.path.join(directory, SOURCE_WAV), os.path.join(directory, TARGET_WAV)
    if not os.path.exists(src):
        return {"audio": "missing " + SOURCE_WAV}
    rate_in, n_in = _wav_header(src)
    up, down = A.ratio(rate_in, opts.rate)
    rep = {"rate_in": rate_in, "samples_in": n_in, "samples_out": A.out_len(n_in, up, down)}
    if os.path.exists(dst) and not opts.force:
        rep["audio"] = "skipped: exists"
    elif opts.dry_run:
        rep["audio"] = "would write"
    else:
        x = _read_wav(src)
        if rate_in != opts.rate:
            import torch
            dev = device()
            y = A.resample(torch.from_numpy(np.ascontiguousarray(x)).to(dev), rate_in, opts.rate)[0]
            x = y.cpu().numpy()
        assert len(x) == rep["samples_out"], (len(x), rep)
        wavfile.write(dst, opts.rate, to_pcm16(x))
        rep["audio"] = "written" if rate_in != opts.rate else "written (rate unchanged)"
    return rep


def _hop(opts):
    return int(opts.rate / opts.video_rate)


def _lag_frames(opts):
    return int(round(opts.max_lag * opts.video_rate))


def _take_curves(audio, poses, opts, device):
    """the two curves of one take, cut to the scan's row limit -> (a (na,), b (nb,)) on the device"""
    import torch
    from . import kernels, metrics
    dev = device()
    x = torch.from_numpy(np.ascontiguousarray(audio, dtype=np.float32)).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(np.asarray(poses, dtype=np.float32))).to(dev)
    a, b = metrics.sync_curves(x, p.reshape(len(p), -1), _hop(opts), rate=opts.rate)
    limit = kernels.impl().sync_scan_max_frames()
    return a[0, :limit], b[0, :limit]


def _auto_factor(directory, take, opts, device):
    """--waltz-factor auto -> (the chosen candidate, the waltz_auto entry of the report)"""
    from . import metrics
    from .data import _read_wav
    wav = os.path.join(directory, TARGET_WAV)
    if not os.path.exists(wav):
        raise SystemExit("%s: --waltz-factor auto needs %s" % (directory, TARGET_WAV))
    a, b = _take_curves(_read_wav(wav), take["skeletons"], opts, device)
    cands = list(opts.factor_candidates)
    shortest = min([a.numel()] + [int(round(b.numel() * f)) for f in cands])
    L, overlap = _lag_frames(opts), max(64, shortest // 2)
    r, n = metrics.sync_profile(a, b, cands, L, overlap)
    peaks = []
    for f in cands:
        est = metrics.sync_estimate(r[:, len(peaks):len(peaks) + 1], n[:, len(peaks):len(peaks) + 1], [f], L)[0]
        peaks.append({"factor": f, "r": est["r"], "lag_frames": est["lag_frames"], "overlap": est["overlap"]})
    defined = [p for p in peaks if p["r"] is not None]
    if not defined:
        raise SystemExit("%s: no candidate of --factor-candidates overlaps the music by %d frames" % (directory, overlap))
    best = max(defined, key=lambda p: p["r"])   # (the first of equal peaks)
    return best["factor"], {"candidates": peaks, "chosen": best["factor"], "max_lag_frames": L, "min_overlap": overlap}


def _waltz(directory, opts, device, rep):
    """-> the waltz entry of the report (None for the other styles); --waltz-factor auto adds `waltz_auto` to rep"""
    from .data import retime_sequence
    if os.path.basename(directory)[6] != "W":
        return None
    src, dst = os.path.join(directory, "skeletons.json"), os.path.join(directory, "new_skeletons.json")
    if os.path.exists(dst) and not (opts.force and opts.waltz_factor is not None and os.path.exists(src)):
        return "skipped: exists"
    if not os.path.exists(src):
        return "missing skeletons.json"
    if opts.waltz_factor is None:
        return "needs re-timing: pass --waltz-factor"
    if opts.waltz_factor == "auto" and opts.dry_run:
        return "would choose a factor of %s and write" % (list(opts.factor_candidates),)
    with open(src) as f:
        take = json.load(f)
    factor = opts.waltz_factor
    if factor == "auto":
        factor, rep["waltz_auto"] = _auto_factor(directory, take, opts, device)
    n = len(take["skeletons"])
    new_len = int(round(n * factor))
    if new_len < 1:
        raise SystemExit("%s: --waltz-factor %g leaves no frame of %d" % (directory, factor, n))
    if opts.dry_run:
        return "would write %d -> %d frames" % (n, new_len)
    take["skeletons"] = retime_sequence(take["skeletons"], new_len).tolist()
    if "center" in take:
        take["center"] = retime_sequence(take["center"], new_len).tolist()
    take["length"] = new_len
    with open(dst, "w") as f:
        json.dump(take, f)
    return "written %d -> %d frames" % (n, new_len)


SYNC_BATCH = 64   # takes of one scan launch


def _sync(pending, opts, device):
    """--sync: `pending` = [(directory, report entry)] of the takes to estimate; curves take by take, ONE scan launch per
    SYNC_BATCH takes (rows padded, the lengths as arrays), sync.json written, the entries' `sync` key filled"""
    import torch
    from . import metrics
    from .data import SYNC_FILE, _read_wav, _skeleton_file
    from .scoring import json_safe
    L = _lag_frames(opts)
    for i0 in range(0, len(pending), SYNC_BATCH):
        batch = pending[i0:i0 + SYNC_BATCH]
        curves = []
        for directory, _ in batch:
            with open(directory + _skeleton_file(os.path.basename(directory))) as f:
                poses = json.load(f)["skeletons"]
            curves.append(_take_curves(_read_wav(os.path.join(directory, TARGET_WAV)), poses, opts, device))
        na, nb = [c[0].numel() for c in curves], [c[1].numel() for c in curves]
        dev = curves[0][0].device
        A = torch.zeros((len(batch), max(na)), dtype=torch.float32, device=dev)
        Bm = torch.zeros((len(batch), max(nb)), dtype=torch.float32, device=dev)
        for i, (a, b) in enumerate(curves):
            A[i, :na[i]], Bm[i, :nb[i]] = a, b
        overlap = [max(64, min(x, y) // 2) for x, y in zip(na, nb)]
        # one launch at the batch's smallest min_overlap; a take's own (larger) one is applied to the copied profile:
        # r does not depend on min_overlap where it is defined
        r, n = metrics.sync_profile(A, Bm, (1.0,), L, min(overlap), na, nb)
        r, n = r.cpu(), n.cpu()
        r[n < torch.tensor(overlap, dtype=torch.int32)[:, None, None]] = float("nan")
        for (directory, rep), est, mo in zip(batch, metrics.sync_estimate(r, n, (1.0,), L), overlap):
            margin = None if est["r"] is None or est["r_second"] is None else est["r"] - est["r_second"]
            est.update(hop=_hop(opts), rate=int(opts.rate), video_rate=opts.video_rate, max_lag_frames=L, min_overlap=mo,
                       accepted=bool(est["r"] is not None and (margin >= opts.min_peak if margin is not None
                                                               else opts.min_peak <= 0)))
            est = json_safe(est)
            with open(os.path.join(directory, SYNC_FILE), "w") as f:
                json.dump(est, f, allow_nan=False)
            rep["sync"] = dict(est, file="written")


def _sync_plan(directory, opts):
    """-> None when the take's offset is to be estimated, else why not (the `sync` entry of the report)"""
    from .data import SYNC_FILE, _skeleton_file
    if os.path.exists(os.path.join(directory, SYNC_FILE)) and not opts.force:
        return "skipped: exists"
    if opts.dry_run:
        return "would write"
    for name in (TARGET_WAV, _skeleton_file(os.path.basename(directory))[1:]):
        if not os.path.exists(os.path.join(directory, name)):
            return "missing " + name
    return None


def prepare(opts):
    """-> the report dict"""
    from .data import _dance_dirs
    if not os.path.isdir(opts.folder):
        raise SystemExit("dataset folder %r not found" % (opts.folder,))
    if opts.rate <= 0 or (opts.waltz_factor not in (None, "auto") and not opts.waltz_factor > 0):
        raise SystemExit("--rate and --waltz-factor must be positive")
    if not opts.video_rate > 0 or opts.max_lag < 0 or _hop(opts) < 1:
        raise SystemExit("--video-rate must be positive and at most --rate, --max-lag non-negative")
    cache = []

    def device():
        if not cache:
            from . import runner
            cache.append(runner.pick_device(opts.device))
        return cache[0]

    takes, pending = [], []
    for directory, base in sorted(_dance_dirs(opts.folder)):
        rep = {"take": base}
        rep.update(_audio(directory, opts, device))
        w = _waltz(directory, opts, device, rep)
        if w is not None:
            rep["waltz"] = w
        if opts.sync:
            rep["sync"] = _sync_plan(directory, opts)
            if rep["sync"] is None:
                pending.append((directory, rep))
        takes.append(rep)
    if pending:
        _sync(pending, opts, device)
    return {"folder": opts.folder, "rate": int(opts.rate), "waltz_factor": opts.waltz_factor,
            "dry_run": bool(opts.dry_run), "takes": takes}


def main(argv=None):
    report = prepare(parse_args(argv))
    print(json.dumps(report, allow_nan=False))
    return report


if __name__ == "__main__":
    main()
