"""Score a trained style-conditioned phase-2 generator as the reference's phase2/test.py does, on the HIP path.

    python -m music2dance_amd.phase2.evaluate -c music2dance_amd/phase2/configs/default.yaml -l <logdir> \
        --classifier logs/type2/weights.pt [--gen-weights PATH] [--samples-per-style 250] [--synthetic]

For every style, `--samples-per-style` sequences are requested from the generator of phase2/archis/conditional.py
(eval mode: BatchNorm on its running statistics, dropout off; noise from torch's generator, seeded), and the
dance-style classifier (dance_classification.archis.default.RecurrentDanceClassifier, eval mode) names the style it
sees in the scaled poses, fed channels-first as the reference feeds it. The reference draws the requested labels at
random, so a style can go unrequested; here every style gets the same number of requests. Writes
<logdir>/evaluation.json, strict JSON: the requested (row) x predicted (column) confusion matrix, row-normalised, its
counts, `style_agreement` (the trace over the total) and the jerkiness mean and unbiased std of the generated poses
(inverse-MinMax-scaled when a dataset is given, i.e. without --synthetic). The generator checkpoint defaults to the
latest <logdir>/models/gpgen_*.pt; --synthetic runs a randomly initialised generator when there is none. The common
flags, the loaders, the confusion matrix and the jerkiness statistics are scoring.py's.
"""
import argparse

import numpy as np
import torch

from .. import ops, runner, scoring
from ..scoring import N_STYLES, STICK_CHANNELS, confusion, jerk_stats
from .archis.conditional import SequenceGenerator


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    scoring.add_common_flags(ap, 2, "gpgen", "no dataset: poses are scored as generated")
    ap.add_argument("--classifier", type=str, required=True, help="RecurrentDanceClassifier state_dict")
    ap.add_argument("--samples-per-style", type=int, default=250, help="requested sequences per style")
    ap.add_argument("--chunk", type=int, default=256, help="sequences per generator call")
    return ap.parse_args(argv)


@torch.no_grad()
def evaluate(opts, cfg, device):
    ds = cfg["dataset"]
    T = int(ds["seq_length"] * ds["video_rate"])
    gen = SequenceGenerator(cfg["input_vector_size"], cfg["latent_vector_size"], cfg["size"], cfg["output_size"],
                            cfg["nblocks_gen"], cfg["n_cells"], device)
    scoring.load_generator(gen, opts)
    classifier = scoring.load_classifier(opts.classifier, device)
    scaler = None
    if not opts.synthetic:
        from .. import data as D
        scaler = D.StickDataset(runner.dataset_folder(cfg, opts.folder), normalize="minmax").scaler

    n = int(opts.samples_per_style)
    requested = torch.arange(N_STYLES, device=device).repeat_interleave(n)
    preds, jerks = [], []
    for lo in range(0, requested.numel(), opts.chunk):
        lbl = requested[lo:lo + opts.chunk].contiguous()
        m = lbl.numel()
        fake = gen(torch.randn(m, T, cfg["input_vector_size"], device=device), lbl).reshape(m, T, STICK_CHANNELS)
        _, pred = ops.cross_entropy_pred(classifier(fake.permute(0, 2, 1).contiguous()), lbl)
        preds.append(pred)
        poses = scaler.inverse_transform_device(fake.contiguous()) if scaler is not None else fake
        jerks += scoring.jerk_per_sequence(poses)
    pred = torch.cat(preds).cpu().numpy()
    cm, counts = confusion(requested.cpu().numpy(), pred, N_STYLES)
    jm, js = jerk_stats(torch.stack(jerks).cpu().numpy())
    total = int(counts.sum())
    return {"confusion": cm.tolist(), "counts": counts.tolist(),
            "style_agreement": float(np.trace(counts)) / total if total else float("nan"),
            "jerk_fake_mean": jm, "jerk_fake_std": js, "n_sequences": total, "samples_per_style": n}


def main(argv=None):
    return scoring.run(parse_args, evaluate, argv, out="evaluation.json", seed=0)


if __name__ == "__main__":
    main()
