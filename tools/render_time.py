"""Dev tool: the stick-figure renderer at the size of a 3-minute track (4 500 frames of 300 x 300, 1.215 GB of RGB).
In one process it times, with HIP events after warm-up,
  * m2d_render_sticks over the whole track in one launch (--reps launches, median and best);
  * a plain device fill (torch fill_) of the same output buffer, the bound the render launch is measured against;
  * visualize.frame_to_vid end to end, split into render, device-to-host copy, JPEG encode and mux: --pairs times
    with encoder="pil" and encoder="hip" in turn, so that both see the same clocks and neighbours;
  * m2d_jpeg_encode on one chunk of CHUNK_FRAMES rendered frames: device time per chunk, and the bytes the launches
    move (frames read once, int16 coefficients written once and read three times, streams written) per second.

    python tools/render_time.py [--frames 4500] [--reps 30] [--pairs 3] [--poses POSES.npy] [--json PATH]

Without --poses the dance is synthetic: a figure with joints spread over about 180 x 240 pixels that sways and turns
frame by frame; its segments cross more of the canvas than a generated dance's do, so fewer tiles take the
background path. Under `rocprofv3 --kernel-trace --stats -- python tools/render_time.py --reps 5` the per-kernel
table follows."""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from music2dance_amd import kernels, visualize  # noqa: E402

DEV = torch.device("cuda:0")


def synthetic_dance(n, seed=0):
    rng = np.random.default_rng(seed)
    base = np.stack([rng.uniform(-90, 90, 23), rng.uniform(-120, 120, 23), rng.uniform(-50, 50, 23)], 1)
    t = np.arange(n)[:, None] / 25.0
    phase = rng.uniform(0, 2 * np.pi, 23)[None]
    sway = 30 * np.sin(2 * np.pi * 0.5 * t)
    turn = np.cos(2 * np.pi * 0.1 * t)
    x = base[None, :, 0] * turn + sway + 6 * np.sin(2 * np.pi * 1.3 * t + phase)
    y = base[None, :, 1] + 8 * np.cos(2 * np.pi * 0.9 * t + phase)
    z = np.broadcast_to(base[None, :, 2], x.shape)
    return np.stack([x, y, z], -1).astype(np.float32)


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
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4500)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=3, help="frame_to_vid runs per encoder, alternated")
    ap.add_argument("--poses", type=str, default=None, help="a (T, 23, 3) .npy instead of the synthetic dance")
    ap.add_argument("--json", type=str, default=None)
    opts = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_time.py measures on a HIP device; none is visible")
    poses = np.load(opts.poses).astype(np.float32) if opts.poses else synthetic_dance(opts.frames)
    n = poses.shape[0]
    x = torch.from_numpy(poses.reshape(n, 69)).to(DEV)
    out = torch.empty((n, 300, 300, 3), dtype=torch.uint8, device=DEV)
    nbytes = out.numel()
    k = kernels.impl()
    res = {"frames": n, "bytes": nbytes, "reps": opts.reps}
    # alternate the two so that both see the same clocks and neighbours
    rnd, fill = [], []
    for _ in range(2):
        rnd += event_times(lambda: k.render_sticks(x, 300, 300, out=out), opts.reps // 2)
        fill += event_times(lambda: out.fill_(255), opts.reps // 2)
    k.check_async_errors()
    for name, ms in (("render", rnd), ("fill", fill)):
        med = statistics.median(ms)
        res[name + "_ms_median"] = round(med, 4)
        res[name + "_ms_best"] = round(min(ms), 4)
        res[name + "_TBps_median"] = round(nbytes / med / 1e9, 3)
    res["render_over_fill"] = round(res["render_ms_median"] / res["fill_ms_median"], 3)
    k.render_sticks(x, 300, 300, out=out)
    figure = (out[..., 0] == 0).float().mean().item()
    res["figure_pixel_share"] = round(figure, 4)
    del out
    torch.cuda.empty_cache()
    # the encode launches on one chunk of the product path
    k_frames = min(n, visualize.CHUNK_FRAMES)
    chunk = k.render_sticks(x[:k_frames], 300, 300)
    qtabs = visualize.jpeg_tables(95)[:2]
    enc = event_times(lambda: k.jpeg_encode(chunk, qtabs), opts.reps)
    k.check_async_errors()
    _, offsets = k.jpeg_encode(chunk, qtabs)
    stream_bytes = int(offsets[-1])
    coef_bytes = k_frames * 38 * 38 * 384
    moved = chunk.numel() + 4 * coef_bytes + stream_bytes   # coefficients: written once, walked three times
    med = statistics.median(enc)
    res["encode_chunk"] = {"frames": k_frames, "ms_median": round(med, 4), "ms_best": round(min(enc), 4),
                           "stream_bytes": stream_bytes, "moved_bytes": moved,
                           "moved_TBps_median": round(moved / med / 1e9, 3)}
    del chunk
    torch.cuda.empty_cache()
    runs = []
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dance.avi")
        for encoder in visualize.ENCODERS:   # warm-up: code objects, PIL
            visualize.frame_to_vid(poses[:min(n, 64)], path, 25, encoder=encoder)
        for _ in range(opts.pairs):
            for encoder in visualize.ENCODERS:
                split = visualize.frame_to_vid(poses, path, 25, encoder=encoder)
                split["file_bytes"] = os.path.getsize(path)
                runs.append({key: round(v, 4) if isinstance(v, float) else v for key, v in split.items()})
    res["frame_to_vid"] = runs
    print(json.dumps(res))
    if opts.json:
        os.makedirs(os.path.dirname(os.path.abspath(opts.json)), exist_ok=True)
        with open(opts.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
