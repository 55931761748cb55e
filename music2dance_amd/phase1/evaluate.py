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
        the pairwise kernel is quadratic in fp64); these five are scoring.distribution_scores';
    k, n_real, n_fake, checkpoint.

The generator checkpoint defaults to the <logdir>/models/gen_<n>.pt with the largest n; with --synthetic and no
checkpoint the weights are random, and the real rows are torch.rand(4 x samples, 69), as the training script's synthetic
batches are. Writes <logdir>/evaluation.json (strict JSON, an undefined value is `null`) and prints it.

--sheet S (0: off) draws the first S generated poses (inverse-scaled, unless --synthetic) with visualize.render, tiles
them into a ceil(sqrt(S))-column grid on the device, encodes it with visualize.encode_jpeg and writes
<logdir>/samples/sheet.jpg; every generated row goes to <logdir>/samples/poses.npy.
"""
import argparse
import functools
import math
import os

import numpy as np
import torch

from .. import metrics, runner, scoring, visualize
from ..scoring import STICK_CHANNELS, json_safe, subset as _subset  # noqa: F401  (json_safe: the tests' name)
from .archis.residual import Generator

DIVERSITY_ROWS = 4096
SHEET_CELL = 300
SPLIT_KEYS = ("precision", "recall", "density", "coverage")
POSE_KEYS = ("fd_pose", "fd_pose_real_split", "fd_pose_converged", "div_pose_real", "div_pose_fake")
KEYS = (list(metrics.PRDC_KEYS) + ["%s_real_split" % s for s in SPLIT_KEYS] + list(POSE_KEYS)
        + ["k", "n_real", "n_fake", "checkpoint"])
latest_checkpoint = functools.partial(scoring.latest_checkpoint, stem="gen")


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    scoring.add_common_flags(ap, 1, "gen", "uniform random real poses; random weights without a checkpoint")
    ap.add_argument("--samples", type=int, default=4096, help="poses to generate")
    ap.add_argument("--k", type=int, default=5, help="neighbours of the radii")
    ap.add_argument("--max-real", type=int, default=None, help="score against a seeded random subset of N real poses")
    ap.add_argument("--seed", type=int, default=0, help="seed of the noise and of the subsets")
    ap.add_argument("--sheet", type=int, default=25, help="poses on the contact sheet (0: none)")
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
    dist = scoring.distribution_scores(real, fake, "pose", DIVERSITY_ROWS, seed)
    res.update({key: dist[key] for key in POSE_KEYS})
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
    path = scoring.load_generator(gen, opts, "gen")
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
    return scoring.run(parse_args, evaluate, argv, out="evaluation.json")       # no global seed: --seed is the seed


if __name__ == "__main__":
    main()
