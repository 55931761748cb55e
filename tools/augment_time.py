"""Dev tool: the resident gather of a training batch with and without augmentation, at the phase-3 bench shape (DESIGN.md
section 19): B = 64 windows of T = 120 frames and S = 76 800 samples out of a resident store of 61 takes (random values;
--seconds each). In one process, after warm-up, HIP events around each `SequenceDataset.sample_batch(indices, device)`
call (--reps calls, median / best) - the whole call as the loader makes it: the draws and the table on the host, the
small upload, the launch -
  * plain:      augment=None, the two index gathers of the unaugmented path;
  * augmented:  mirror 0.5, yaw 180 degrees, speeds 1/1, 24/25, 25/24, 9/10, 10/9, gain 3 dB (one m2d_crop_augment launch);
  * identity:   an `augment: {}` block: the same launch on its copy paths;
and the m2d_crop_augment launch alone, from the library's per-launch event profiler.

    python tools/augment_time.py [--reps 30] [--seconds 40] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2dance_amd import data as D  # noqa: E402
from music2dance_amd import kernels  # noqa: E402

DEV = torch.device("cuda:0")
CONFIG = {"audio_rate": 16000, "video_rate": 25, "seq_length": 4.8, "feat_size": 69}
FULL = {"mirror": 0.5, "yaw_deg": 180, "speeds": ["1/1", "24/25", "25/24", "9/10", "10/9"], "gain_db": 3, "seed": 0}
TAKES, BATCH = 61, 64


def timed(fn, reps, warmup=5):
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


def dataset(seconds, augment):
    rng = np.random.default_rng(0)
    frames = [seconds * 25 + int(rng.integers(0, 25)) for _ in range(TAKES)]
    poses = [rng.random((n, 23, 3), dtype=np.float32) for n in frames]
    state = {"sequences": poses, "labels": np.arange(TAKES) % 4, "dirs": ["take_%d" % i for i in range(TAKES)],
             "musics": [rng.random(n * 640, dtype=np.float32) - 0.5 for n in frames]}
    ds = D.SequenceDataset(state, CONFIG, resume=True, withaudio=True, augment=augment,
                           crop_rng=np.random.RandomState(1))
    ds.pose_scaler = D.MinMaxScaler().fit(np.concatenate(poses).reshape(-1, 69))
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--seconds", type=int, default=40)
    ap.add_argument("--json", type=str, default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py measures on a HIP device; none is visible")
    res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "frames": 120, "samples": 76800, "takes": TAKES,
           "take_seconds": opts.seconds}
    order = np.random.default_rng(2).integers(0, TAKES, size=(opts.reps + 16, BATCH))
    for name, block in (("plain", None), ("augmented", FULL), ("identity", {})):
        ds = dataset(opts.seconds, block)
        calls = iter(order)
        res[name] = timed(lambda: ds.sample_batch(next(calls), DEV), opts.reps)
        if block is not None:
            kernels.impl().prof_begin()
            for idx in order[:8]:
                ds.sample_batch(idx, DEV)
            torch.cuda.synchronize()
            rows = [r for r in kernels.impl().prof_dump() if r[1] == "crop_augment"]
            kernels.impl().prof_end()
            res[name]["kernel_ms_median"] = round(statistics.median(r[5] for r in rows), 5)
            res[name]["kernel_launches_per_batch"] = len(rows) / 8.0
    print(json.dumps(res))
    if opts.json:
        os.makedirs(os.path.dirname(os.path.abspath(opts.json)), exist_ok=True)
        with open(opts.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
