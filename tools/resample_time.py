"""Dev tool: the polyphase resampler at the sizes a user runs. In one process, after warm-up:
  * audio.resample 44.1 -> 16 kHz of a 3-minute track and of 30 such tracks in one batch (90 minutes of audio), and
    48 -> 16 kHz of a 3-minute track: HIP events around each call (--reps calls, median / best), plus the time per
    call inside a window of 100 back-to-back calls (what a call costs once the launch queue is full);
  * the host's scipy.signal.resample (the FFT pass of generate.load_track) and scipy.signal.resample_poly on the same
    track, best and worst of 3;
  * phase3.generate --audio <the same track as a 44.1 kHz wav> --chunk-frames 25 with --resampler fft and --resampler
    poly, alternating, three runs each (random generator weights, a synthetic dataset folder for the scaler).

    python tools/resample_time.py [--reps 50] [--json PATH]"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2dance_amd import audio as A  # noqa: E402
from music2dance_amd import runner  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SECONDS = 180


def event_times(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": round(statistics.median(ms), 5), "ms_best": round(min(ms), 5), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--json", type=str, default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_time.py measures on a HIP device; none is visible")
    rng = np.random.RandomState(0)
    pcm = np.clip(rng.randn(SECONDS * 44100) * 3000.0, -32767, 32767).astype(np.int16)
    host = pcm.astype(np.float32) / 32768.0
    one = torch.from_numpy(host).to(DEV)
    res = {"seconds": SECONDS}
    res["device_3min_44k1"] = event_times(lambda: A.resample(one, 44100, 16000), opts.reps)

    def hundred():
        for _ in range(100):
            A.resample(one, 44100, 16000)

    w = event_times(hundred, 5)
    res["device_3min_44k1_per_call_of_100"] = {"ms_median": round(w["ms_median"] / 100, 5),
                                              "ms_best": round(w["ms_best"] / 100, 5)}
    batch = one.unsqueeze(0).repeat(30, 1).contiguous()
    res["device_90min_batch30_44k1"] = event_times(lambda: A.resample(batch, 44100, 16000), max(opts.reps // 2, 5))
    del batch
    other = torch.from_numpy(rng.randn(SECONDS * 48000).astype(np.float32) * 0.1).to(DEV)
    res["device_3min_48k"] = event_times(lambda: A.resample(other, 48000, 16000), opts.reps)

    from scipy.signal import resample, resample_poly
    for name, fn in (("host_scipy_resample_fft", lambda: resample(host, int(len(host) * (16000 / 44100)))),
                     ("host_scipy_resample_poly", lambda: resample_poly(host, 160, 441))):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        res[name] = {"s_best": round(min(ts), 4), "s_worst": round(max(ts), 4)}

    from scipy.io import wavfile
    from music2dance_amd.data import write_synthetic_dataset
    from music2dance_amd.phase3 import generate as G
    from music2dance_amd.phase3.archis.default import build_generator
    cfg_path = os.path.join(ROOT, "music2dance_amd", "phase3", "configs", "default.yaml")
    with tempfile.TemporaryDirectory() as tmp:
        wav = os.path.join(tmp, "song.wav")
        wavfile.write(wav, 44100, pcm)
        data = write_synthetic_dataset(os.path.join(tmp, "data"), n_takes=4, seconds=2)
        torch.manual_seed(0)
        weights = os.path.join(tmp, "gen.pt")
        torch.save(build_generator(runner.load_config(cfg_path), "cpu").state_dict(), weights)
        for how in ("fft", "poly") * 3:
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                out = G.main(["-c", cfg_path, "-l", os.path.join(tmp, how), "--gen-weights", weights, "--audio", wav,
                              "--folder", data, "--resampler", how, "--chunk-frames", "25"])
            tr = out["tracks"][0]
            res.setdefault("generate_" + how, []).append(
                {"real_time_factor": round(tr["real_time_factor"], 1), "wall_s": round(tr["wall_s"], 4),
                 "gpu_ms_per_chunk_p50": round(tr["gpu_ms_per_chunk_p50"], 4),
                 "gpu_ms_per_chunk_p99": round(tr["gpu_ms_per_chunk_p99"], 4), "chunks": tr["chunks"],
                 "main_s": round(time.perf_counter() - t0, 4)})
    print(json.dumps(res))
    if opts.json:
        os.makedirs(os.path.dirname(os.path.abspath(opts.json)), exist_ok=True)
        with open(opts.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
