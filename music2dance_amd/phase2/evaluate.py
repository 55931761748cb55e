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
latest <logdir>/models/gpgen_*.pt; --synthetic runs a randomly initialised generator when there is none.
"""
import argparse
import json
import os

import numpy as np
import torch

from .. import losses, ops, runner
from ..dance_classification.archis.default import RecurrentDanceClassifier
from ..phase3.evaluate import confusion, jerk_stats, json_safe, latest_checkpoint
from .archis.conditional import N_CLASSES, SequenceGenerator

STICK_CHANNELS = 69


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, required=True, help="phase-2 config file of the generator")
    ap.add_argument("-l", "--logdir", type=str, required=True, help="run directory of the generator")
    ap.add_argument("--gen-weights", type=str, default=None, help="generator state_dict (default: latest "
                                                                    "<logdir>/models/gpgen_*.pt)")
    ap.add_argument("--classifier", type=str, required=True, help="RecurrentDanceClassifier state_dict")
    ap.add_argument("--samples-per-style", type=int, default=250, help="requested sequences per style")
    ap.add_argument("--chunk", type=int, default=256, help="sequences per generator call")
    ap.add_argument("--synthetic", action="store_true", help="no dataset: poses are scored as generated")
    ap.add_argument("--folder", type=str, default=None, help="dataset folder (overrides the YAML's `folder:`)")
    ap.add_argument("-d", "--device", type=int, default=None, help="choose gpu id")
    return ap.parse_args(argv)


@torch.no_grad()
def evaluate(opts, cfg, device):
    ds = cfg["dataset"]
    T = int(ds["seq_length"] * ds["video_rate"])
    gen = SequenceGenerator(cfg["input_vector_size"], cfg["latent_vector_size"], cfg["size"], cfg["output_size"],
                            cfg["nblocks_gen"], cfg["n_cells"], device)
    path = opts.gen_weights or latest_checkpoint(opts.logdir)
    if path is not None:
        gen.load_state_dict(torch.load(path, map_location=device))
    elif not opts.synthetic:
        raise SystemExit("no generator checkpoint: pass --gen-weights or train into %s/models" % opts.logdir)
    classifier = RecurrentDanceClassifier(STICK_CHANNELS, 128, N_CLASSES).to(device)
    classifier.load_state_dict(torch.load(opts.classifier, map_location=device))
    gen.eval(), classifier.eval()
    scaler = None
    if not opts.synthetic:
        from .. import data as D
        scaler = D.StickDataset(runner.dataset_folder(cfg, opts.folder), normalize="minmax").scaler

    n = int(opts.samples_per_style)
    requested = torch.arange(N_CLASSES, device=device).repeat_interleave(n)
    preds, jerks = [], []
    for lo in range(0, requested.numel(), opts.chunk):
        lbl = requested[lo:lo + opts.chunk].contiguous()
        m = lbl.numel()
        fake = gen(torch.randn(m, T, cfg["input_vector_size"], device=device), lbl).reshape(m, T, STICK_CHANNELS)
        _, pred = ops.cross_entropy_pred(classifier(fake.permute(0, 2, 1).contiguous()), lbl)
        preds.append(pred)
        poses = scaler.inverse_transform_device(fake.contiguous()) if scaler is not None else fake
        jerks += [losses.jerkiness(poses[i:i + 1].permute(0, 2, 1)) for i in range(m)]
    pred = torch.cat(preds).cpu().numpy()
    cm, counts = confusion(requested.cpu().numpy(), pred, N_CLASSES)
    jm, js = jerk_stats(torch.stack(jerks).cpu().numpy())
    total = int(counts.sum())
    return {"confusion": cm.tolist(), "counts": counts.tolist(),
            "style_agreement": float(np.trace(counts)) / total if total else float("nan"),
            "jerk_fake_mean": jm, "jerk_fake_std": js, "n_sequences": total, "samples_per_style": n}


def main(argv=None):
    opts = parse_args(argv)
    cfg = runner.load_config(opts.config)
    device = runner.pick_device(opts.device)
    os.makedirs(opts.logdir, exist_ok=True)
    torch.manual_seed(0)
    res = evaluate(opts, cfg, device)
    with open(os.path.join(opts.logdir, "evaluation.json"), "w") as f:
        json.dump(json_safe(res), f, indent=1, allow_nan=False)
    print(json.dumps(json_safe(res), allow_nan=False))
    return res


if __name__ == "__main__":
    main()
