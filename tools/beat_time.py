"""Dev tool: the beat-alignment kernels at the sizes a user runs. In one process, after
warm-up, HIP events around each call (--reps calls, median / best), the new path and the yardstick alternating:
  * metrics.band_energies (m2d_stft_bands, n_fft 1024, hop 640, 40 mel bands) at the evaluation size, 120 rows x 120
    frames, and at the dataset's size, one row of 135 000 frames (90 minutes at 25 fps);
  * the yardstick, what the library could do before m2d_stft_bands: the same spectrum as a Conv1d(1, 2 nbins, n_fft,
    stride = hop) with the windowed DFT basis as its weights through m2d_conv1d_fwd (the track padded so that the
    frames are the same), then the power and the band projection in torch ops. Its largest difference from the fused
    kernel, relative to the largest band energy, is printed with the times;
  * the whole metrics.beat_scores at both sizes. m2d_beat_align takes rows of at most 16 384 frames, so the 135 000
    frames are scored as 9 sections of 15 000 frames (9 rows of one call).

    python tools/beat_time.py [--reps 20] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from music2dance_amd import kernels, metrics  # noqa: E402

DEV = torch.device("cuda:0")
N_FFT, HOP, RATE = 1024, 640, 16000
SIZES = {"eval_120x120": (120, 120), "dataset_1x135000": (1, 135000)}


def time_pair(fns, reps, warmup=2):
    """fns: {name: callable}; the callables alternate, each timed with its own pair of events"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"ms_median": round(statistics.median(v), 5), "ms_best": round(min(v), 5), "reps": reps}
            for k, v in ms.items()}


def conv_path(x, T, table, bands, zero_bias):
    """band energies through m2d_conv1d_fwd + torch ops: x (B, S) -> (B, T, nb)"""
    B, S = x.shape
    left = N_FFT // 2 - HOP // 2
    need = (T - 1) * HOP + N_FFT
    xp = torch.zeros((B, 1, max(need, left + S)), dtype=torch.float32, device=x.device)
    xp[:, 0, left:left + S] = x
    y = kernels.impl().conv1d_fwd(xp[:, :, :need].contiguous(), table, zero_bias, HOP, 0)     # (B, 2 nbins, T)
    nbins = N_FFT // 2 + 1
    P = y[:, :nbins] * y[:, :nbins] + y[:, nbins:] * y[:, nbins:]
    return torch.matmul(bands, P).transpose(1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", type=str, default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beat_time.py measures on a HIP device; none is visible")
    g = torch.Generator().manual_seed(0)
    table = torch.from_numpy(metrics.stft_table(N_FFT)).to(DEV)
    weights = table.reshape(-1, 1, N_FFT).contiguous()
    zero_bias = torch.zeros(weights.shape[0], device=DEV)
    bands = torch.as_tensor(metrics.mel_bands(40, N_FFT, RATE), dtype=torch.float32).to(DEV)
    res = {"n_fft": N_FFT, "hop": HOP, "bands": 40}
    for name, (B, T) in SIZES.items():
        x = (0.1 * torch.randn(B, T * HOP, generator=g)).to(DEV)
        reps = opts.reps if B * T < 100000 else max(opts.reps // 4, 3)
        new = metrics.band_energies(x, T, HOP)
        old = conv_path(x, T, weights, bands, zero_bias)
        diff = float((new - old).abs().max() / new.max())
        del new, old
        r = time_pair({"stft_bands": lambda: metrics.band_energies(x, T, HOP),
                       "conv1d_fwd_then_torch": lambda: conv_path(x, T, weights, bands, zero_bias)}, reps)
        r["max_difference_over_max_energy"] = diff
        r["tflops_stft_bands"] = round(4.0 * B * T * (N_FFT // 2) * N_FFT / (r["stft_bands"]["ms_median"] * 1e9), 2)
        # the whole metric: sections of at most 16 384 frames are the rows of one call
        rows = 1 if T <= 16384 else 9
        xs = x.reshape(B * rows, -1)
        poses = torch.cumsum(torch.randn(B * rows, T // rows, 23, 3, generator=g), 1).to(DEV)
        r.update(time_pair({"beat_scores": lambda: metrics.beat_scores(xs, poses, HOP)}, reps))
        r["beat_scores_rows_x_frames"] = [B * rows, T // rows]
        res[name] = r
        del x, xs, poses
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if opts.json:
        os.makedirs(os.path.dirname(os.path.abspath(opts.json)), exist_ok=True)
        with open(opts.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
