"""Dev tool: the lag / tempo-factor scan at the sizes prepare_data runs it. In one process,
after warm-up, HIP events around each call (--reps calls, median / best):
  * the --sync scan: 61 takes (the dataset's count) padded to 8 192 frames (5.5 minutes at 25 fps), factor 1,
    max_lag 250 frames (10 s), one m2d_sync_scan launch; and the same at the row limit, 16 384 frames;
  * the --waltz-factor auto scan: one take, 2 048 audio frames against 8 192 pose frames, candidates (0.25, 4);
  * the yardstick the issue names, "minutes of numpy for the dataset": the fp64 numpy statement of one take of the
    first case over 11 of its 501 lags, scaled to the 501 x 61 cells (host time, one thread).
The pair evaluations a call makes (2 passes x n pairs per cell, n read back from the call) over its time is printed as
G pairs / s.

    python tools/sync_time.py [--reps 20] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2dance_amd import metrics  # noqa: E402

DEV = torch.device("cuda:0")
CASES = {"sync_61x8192_L250": (61, 8192, 8192, (1.0,), 250), "sync_61x16384_L250": (61, 16384, 16384, (1.0,), 250),
         "waltz_auto_1x2048x8192_L250": (1, 2048, 8192, (0.25, 4.0), 250)}


def timed(fn, reps, warmup=2):
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


def numpy_cells(a, b, lags):
    """the fp64 two-pass correlation at factor 1 for `lags`, plain numpy"""
    out = []
    for l in lags:
        lo, hi = max(0, -l), min(len(a), len(b) - l)
        x, y = a[lo:hi], b[lo + l:hi + l]
        dx, dy = x - x.mean(), y - y.mean()
        out.append(float((dx * dy).sum() / np.sqrt((dx * dx).sum() * (dy * dy).sum())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", type=str, default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_time.py measures on a HIP device; none is visible")
    g = torch.Generator().manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0)}
    for name, (B, Ta, Tb, factors, L) in CASES.items():
        a, b = torch.rand(B, Ta, generator=g).to(DEV), torch.rand(B, Tb, generator=g).to(DEV)
        r, n = metrics.sync_profile(a, b, factors, L, 64)
        pairs = 2.0 * float(n.double().sum())
        t = timed(lambda: metrics.sync_profile(a, b, factors, L, 64), opts.reps)
        t.update(rows=B, frames=[Ta, Tb], factors=list(factors), max_lag=L, pair_evaluations=pairs,
                 gpairs_per_s=round(pairs / (t["ms_median"] * 1e6), 2), defined_cells=int((~torch.isnan(r)).sum()))
        res[name] = t
        if name == "sync_61x8192_L250":
            ah, bh = a[0].cpu().double().numpy(), b[0].cpu().double().numpy()
            lags = list(range(-250, 251, 50))
            t0 = time.perf_counter()
            want = numpy_cells(ah, bh, lags)
            dt = time.perf_counter() - t0
            got = r[0, 0, [l + L for l in lags]].cpu().numpy()
            res["numpy_one_thread"] = {"s_for_%d_cells" % len(lags): round(dt, 5),
                                       "s_scaled_to_61x501_cells": round(dt / len(lags) * 61 * 501, 2),
                                       "max_abs_difference_from_the_kernel": float(np.abs(got - np.asarray(want)).max())}
    print(json.dumps(res))
    if opts.json:
        os.makedirs(os.path.dirname(os.path.abspath(opts.json)), exist_ok=True)
        with open(opts.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
