"""Score a trained phase-1 generator (the still-pose WGAN-GP) on the HIP path.

    python -m music2dance_amd.phase1.evaluate -c music2dance_amd/phase1/configs/b1l10s128.yaml -l <logdir> \
        [--gen-weights PATH] [--samples 4096] [--k 5] [--max-real N] [--seed 0] [--sheet 25] [--synthetic]
        [--folder F] [-d N]

The reference only draws samples of a checkpoint (phase1/test.py); it has no score. This script samples `--samples`
poses from the generator (eval mode, noise from torch.randn on the device, seeded by --seed) and compares them with the
real poses - every row of StickDataset(folder, normalize="minmax"), flattened to 69, or a seeded random subset of
--max-real of them - in that MinMax-scaled space:

    precision, recall, density, coverage, nn_ratio_median, nn_fake_to_real_median, nn_real_to_real_median
        metrics.prdc(real, generated, k): k-nearest-neighbour fidelity and variety, and whether the generated poses sit
        closer to training poses than training poses sit to each other (nn_ratio_median well below 1: memorisation);
    precision_real_split, recall_real_split, density_real_split, coverage_real_split
        the same four for the even rows against the odd rows of the real set: what a perfect generator would get;
    fd_pose, fd_pose_real_split, fd_pose_converged
        the Frechet distance (metrics.feature_moments / frechet_from_moments) of the 69-D rows, standardised by the real
        set's moments, and its sampling floor on the even / odd real rows;
    div_pose_real, div_pose_fake
        the mean pairwise distance of the standardised rows (at most DIVERSITY_ROWS rows of each set, a seeded subset:
        the pairwise kernel is quadratic in fp64);
    k, n_real, n_fake, checkpoint.

The generator checkpoint defaults to the <logdir>/models/gen_<n>.pt with the largest n; with --synthetic and no
checkpoint the weights are random, and the real rows are torch.rand(4 x samples, 69), as the training script's synthetic
batches are. Writes <logdir>/evaluation.json (strict JSON, an undefined value is `null`) and prints it.

--sheet S (0: off) draws the first S generated poses (inverse-scaled, unless --synthetic) with visualize.render, tiles
them into a ceil(sqrt(S))-column grid on the device, encodes it with visualize.encode_jpeg and writes
<logdir>/samples/sheet.jpg; every generated row goes to <logdir>/samples/poses.npy.
"""
import argparse
import glob
import json
import math
import os
import re

import numpy as np
import torch

from .. import metrics, runner, visualize
from ..phase3.evaluate import json_safe
from .archis.residual import Generator

STICK_CHANNELS = 69
DIVERSITY_ROWS = 4096
SHEET_CELL = 300
SPLIT_KEYS = ("precision", "recall", "density", "coverage")
KEYS = (list(metrics.PRDC_KEYS) + ["%s_real_split" % s for s in SPLIT_KEYS]
        + ["fd_pose", "fd_pose_real_split", "fd_pose_converged", "div_pose_real", "div_pose_fake", "k", "n_real", "n_fake",
           "checkpoint"])


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, required=True, help="phase-1 config file of the generator")
    ap.add_argument("-l", "--logdir", type=str, required=True, help="run directory of the generator")
    ap.add_argument("--gen-weights", type=str, default=None, help="generator state_dict (default: latest "
                                                                    "<logdir>/models/gen_*.pt)")
    ap.add_argument("--samples", type=int, default=4096, help="poses to generate")
    ap.add_argument("--k", type=int, default=5, help="neighbours of the radii")
    ap.add_argument("--max-real", type=int, default=None, help="score against a seeded random subset of N real poses")
    ap.add_argument("--seed", type=int, default=0, help="seed of the noise and of the subsets")
    ap.add_argument("--sheet", type=int, default=25, help="poses on the contact sheet (0: none)")
    ap.add_argument("--synthetic", action="store_true", help="uniform random real poses; random weights without a checkpoint")
    ap.add_argument("--folder", type=str, default=None, help="dataset folder (overrides the YAML's `folder:`)")
    ap.add_argument("-d", "--device", type=int, default=None, help="choose gpu id")
    opts = ap.parse_args(argv)
    if opts.k < 1:
        ap.error("--k needs K >= 1")
    if opts.samples < opts.k + 1:
        ap.error("--samples must be at least k + 1")
    if opts.max_real is not None and opts.max_real < 2 * (opts.k + 1):
        ap.error("--max-real must be at least 2 (k + 1): the even / odd split needs k + 1 rows a side")
    if opts.sheet < 0:
        ap.error("--sheet must not be negative")
    return opts


def latest_checkpoint(logdir):
    """<logdir>/models/gen_<n>.pt with the largest n, or None"""
    best, best_n = None, -1
    for p in glob.glob(os.path.join(logdir, "models", "gen_*.pt")):
        m = re.search(r"gen_(\d+)\.pt$", p)
        if m and int(m.group(1)) > best_n:
            best, best_n = p, int(m.group(1))
    return best


def _subset(rows, n, seed):
    """a seeded random subset of n rows (all of them when there are no more), in their original order"""
    if n is None or rows.shape[0] <= n:
        return rows
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(rows.shape[0], generator=g)[:n].sort().values
    return rows[idx.to(rows.device)].contiguous()


def real_rows(opts, cfg, device):
    """-> (rows (N, 69) fp32 on the device, the dataset's scaler or None)"""
    if opts.synthetic:
        g = torch.Generator(device=device).manual_seed(opts.seed + 1)
        return torch.rand(4 * opts.samples, STICK_CHANNELS, generator=g, device=device), None
    from .. import data as D
    sticks = D.StickDataset(runner.dataset_folder(cfg, opts.folder), normalize="minmax")
    rows = torch.as_tensor(sticks.skeletons.reshape(len(sticks), STICK_CHANNELS), dtype=torch.float32).to(device)
    return _subset(rows, opts.max_real, opts.seed), sticks.scaler


def scores(real, fake, k, seed=0):
    """real (N, 69), fake (M, 69) fp32 on the device -> the keys of evaluation.json but `checkpoint`. Host reads: the
    final scalars only."""
    res = {key: float(val.cpu()) for key, val in metrics.prdc(real, fake, k).items()}
    split = metrics.prdc(real[0::2], real[1::2], k)
    res.update({"%s_real_split" % s: float(split[s].cpu()) for s in SPLIT_KEYS})
    mean, cov = metrics.feature_moments(real)
    Zr, Zf = metrics.standardize(real, mean, cov), metrics.standardize(fake, mean, cov)
    pairs = [(Zr, Zf), (Zr[0::2], Zr[1::2])]
    mom = [[metrics.feature_moments(x) for x in pair] for pair in pairs]
    fd = metrics.frechet_from_moments(torch.stack([m[0][0] for m in mom]), torch.stack([m[0][1] for m in mom]),
                                      torch.stack([m[1][0] for m in mom]), torch.stack([m[1][1] for m in mom]))
    vals = fd["fd"].cpu().numpy()
    res["fd_pose"], res["fd_pose_real_split"] = float(vals[0]), float(vals[1])
    res["fd_pose_converged"] = bool((fd["converged"] != 0).all().cpu())
    res["div_pose_real"] = float(metrics.mean_pairwise_distance(_subset(Zr, DIVERSITY_ROWS, seed))[0].cpu())
    res["div_pose_fake"] = float(metrics.mean_pairwise_distance(_subset(Zf, DIVERSITY_ROWS, seed))[0].cpu())
    res.update(k=int(k), n_real=int(real.shape[0]), n_fake=int(fake.shape[0]))
    return res


def sheet_grid(frames):
    """frames (S, h, w, 3) uint8 -> (1, rows h, cols w, 3): a ceil(sqrt(S))-column grid in reading order, the cells
    past the last frame white"""
    S, h, w, _ = frames.shape
    cols = int(math.ceil(math.sqrt(S)))
    rows = (S + cols - 1) // cols
    if rows * cols > S:
        pad = torch.full((rows * cols - S, h, w, 3), 255, dtype=torch.uint8, device=frames.device)
        frames = torch.cat([frames, pad])
    return frames.reshape(rows, cols, h, w, 3).permute(0, 2, 1, 3, 4).reshape(1, rows * h, cols * w, 3).contiguous()


def write_sheet(poses, path):
    """poses (S, 69) in world units on the device -> a JPEG contact sheet at `path`; -> (height, width)"""
    cols = int(math.ceil(math.sqrt(poses.shape[0])))
    cell = min(SHEET_CELL, 4096 // cols)                    # the renderer and the encoder take at most 4096 a side
    grid = sheet_grid(visualize.render(poses, cell, cell))
    with open(path, "wb") as f:
        f.write(visualize.encode_jpeg(grid)[0])
    return int(grid.shape[1]), int(grid.shape[2])


@torch.no_grad()
def evaluate(opts, cfg, device):
    gen = Generator(cfg["latent_vector_size"], cfg["size"], cfg["output_size"], cfg["nblocks_gen"]).to(device)
    path = opts.gen_weights or latest_checkpoint(opts.logdir)
    if path is not None:
        gen.load_state_dict(torch.load(path, map_location=device))
    elif not opts.synthetic:
        raise SystemExit("no generator checkpoint: pass --gen-weights or train into %s/models" % opts.logdir)
    gen.eval()
    real, scaler = real_rows(opts, cfg, device)
    if real.shape[0] < 2 * (opts.k + 1):
        raise SystemExit("%d real poses are too few for k = %d" % (real.shape[0], opts.k))
    g = torch.Generator(device=device).manual_seed(opts.seed)
    noise = torch.randn(opts.samples, cfg["latent_vector_size"], generator=g, device=device)
    fake = gen(noise).reshape(opts.samples, STICK_CHANNELS).float().contiguous()
    res = scores(real.contiguous(), fake, opts.k, opts.seed)
    res["checkpoint"] = path
    samples = os.path.join(opts.logdir, "samples")
    os.makedirs(samples, exist_ok=True)
    np.save(os.path.join(samples, "poses.npy"), fake.cpu().numpy())
    if opts.sheet:
        first = fake[:opts.sheet].contiguous()
        if scaler is not None:
            first = scaler.inverse_transform_device(first)
        write_sheet(first, os.path.join(samples, "sheet.jpg"))
    return res


def main(argv=None):
    opts = parse_args(argv)
    cfg = runner.load_config(opts.config)
    device = runner.pick_device(opts.device)
    os.makedirs(opts.logdir, exist_ok=True)
    res = evaluate(opts, cfg, device)
    with open(os.path.join(opts.logdir, "evaluation.json"), "w") as f:
        json.dump(json_safe(res), f, indent=1, allow_nan=False)
    print(json.dumps(json_safe(res), allow_nan=False))
    return res


if __name__ == "__main__":
    main()
