"""The scoring driver of the scripts that use a trained generator (phase1.evaluate, phase2.evaluate, phase3.evaluate and
phase3.generate), as runner.py is the training driver: the constants, the common flags (`add_common_flags`), the
checkpoint and classifier loaders, the shared `main` (`run`), strict JSON (`json_safe`), the validation-take lookup and
the scores more than one script computes (`confusion`, `jerk_stats`, `jerk_per_sequence`, `distribution_scores`). A
script keeps its docstring, its own flags and their checks, its networks, its seeds and the order of its result's keys.
"""
import glob
import json
import os
import re

import numpy as np
import torch

from . import losses, metrics, runner
from .dance_classification.archis.default import RecurrentDanceClassifier

STICK_CHANNELS = 69   # 23 joints x 3 coordinates
N_STYLES = 4


# ------------------------------------------------------------------------------------------- the command line
def add_common_flags(ap, phase, stem, synthetic="random inputs of the dataset's shapes", source=None):
    """The flags every scoring script takes: -c, -l, --gen-weights, --synthetic, --folder, -d, and --ema (score the
    averaged generator a run with `ema_decay` saved). `synthetic`: what that flag means to the script; `source`: the
    (mutually exclusive) group --synthetic joins instead of the parser."""
    ap.add_argument("-c", "--config", type=str, required=True, help="phase-%d config file of the generator" % phase)
    ap.add_argument("-l", "--logdir", type=str, required=True, help="run directory of the generator")
    ap.add_argument("--gen-weights", type=str, default=None,
                    help="generator state_dict (default: latest <logdir>/models/%s_*.pt)" % stem)
    (source or ap).add_argument("--synthetic", action="store_true", help=synthetic)
    ap.add_argument("--folder", type=str, default=None, help="dataset folder (overrides the YAML's `folder:`)")
    ap.add_argument("-d", "--device", type=int, default=None, help="choose gpu id")
    ap.add_argument("--ema", action="store_true",
                    help="load the averaged generator (latest <logdir>/models/%s_ema_*.pt) instead of the last iterate; "
                         "--gen-weights still wins" % stem)


def json_safe(v):
    """NaN / inf -> None (JSON null), recursively through lists and dicts"""
    if isinstance(v, dict):
        return {k: json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [json_safe(x) for x in v]
    if isinstance(v, float) and not np.isfinite(v):
        return None
    return v


def run(parse_args, body, argv=None, out=None, seed=None):
    """The `main` of a scoring script: flags, YAML, device, <logdir>, `torch.manual_seed(seed)` unless seed is None,
    res = body(opts, cfg, device), strict JSON of it into <logdir>/<out> (unless out is None) and onto stdout; -> res"""
    opts = parse_args(argv)
    cfg = runner.load_config(opts.config)
    device = runner.pick_device(opts.device)
    os.makedirs(opts.logdir, exist_ok=True)
    if seed is not None:
        torch.manual_seed(seed)
    res = body(opts, cfg, device)
    if out is not None:
        with open(os.path.join(opts.logdir, out), "w") as f:
            json.dump(json_safe(res), f, indent=1, allow_nan=False)
    print(json.dumps(json_safe(res), allow_nan=False))
    return res


# ------------------------------------------------------------------------------------------- what a run loads
def latest_checkpoint(logdir, stem="gpgen"):
    """<logdir>/models/<stem>_<n>.pt with the largest n, or None"""
    best, best_n = None, -1
    for p in glob.glob(os.path.join(logdir, "models", stem + "_*.pt")):
        m = re.search(r"%s_(\d+)\.pt$" % re.escape(stem), p)
        if m and int(m.group(1)) > best_n:
            best, best_n = p, int(m.group(1))
    return best


def load_generator(gen, opts, stem="gpgen"):
    """--gen-weights, or the latest <logdir>/models/<stem>_*.pt (with --ema: <stem>_ema_*.pt, the averaged generator of
    a run trained with `ema_decay`), into `gen`, which is left in eval mode; -> the path, None for the random weights
    --synthetic allows when there is no checkpoint"""
    ema = bool(getattr(opts, "ema", False))
    path = opts.gen_weights or latest_checkpoint(opts.logdir, stem + "_ema" if ema else stem)
    if path is None and ema and not opts.synthetic:
        raise SystemExit("--ema: no averaged-generator checkpoint %s/models/%s_ema_*.pt: train with `ema_decay` set in "
                         "the YAML, or pass --gen-weights" % (opts.logdir, stem))
    if path is not None:
        if not os.path.exists(path):
            raise SystemExit("generator checkpoint %s not found" % path)
        gen.load_state_dict(torch.load(path, map_location=next(gen.parameters()).device))
    elif not opts.synthetic:
        raise SystemExit("no generator checkpoint: pass --gen-weights or train into %s/models" % opts.logdir)
    gen.eval()
    return path


def load_classifier(path, device, n_classes=N_STYLES):
    """the dance-style classifier of a state_dict file, in eval mode"""
    classifier = RecurrentDanceClassifier(STICK_CHANNELS, 128, n_classes).to(device)
    classifier.load_state_dict(torch.load(path, map_location=device))
    return classifier.eval()


def validation_takes(opts, cfg, withaudio=True):
    """-> (val_dirs, their indices in the dataset, the SequenceDataset, the still poses' scaler): the takes listed under
    `val_samples` in <logdir>/trainvaltest_samples.json"""
    from . import data as D
    with open(os.path.join(opts.logdir, "trainvaltest_samples.json")) as f:
        val_dirs = json.load(f)["val_samples"]
    folder = runner.dataset_folder(cfg, opts.folder)
    scaler = D.StickDataset(folder, normalize="minmax").scaler
    dataset = D.SequenceDataset(folder, cfg["dataset"], dance_types=cfg["dance_types"], scaler=scaler,
                                withaudio=withaudio, sync=cfg["dataset"].get("sync", False))
    where = {d: i for i, d in enumerate(dataset.dirs)}
    missing = [d for d in val_dirs if d not in where]
    if missing:
        raise SystemExit("validation takes not in the dataset: %s" % missing[:5])
    return val_dirs, [where[d] for d in val_dirs], dataset, scaler


# ------------------------------------------------------------------------------------------- the shared scores
def confusion(real_pred, fake_pred, n_classes=N_STYLES):
    """-> (row-normalised C x C matrix of real-predicted (row) vs fake-predicted (column) labels, NaN rows where a
    real label never occurs; the raw counts)."""
    real_pred = np.asarray(real_pred, dtype=np.int64).reshape(-1)
    fake_pred = np.asarray(fake_pred, dtype=np.int64).reshape(-1)
    counts = np.zeros((n_classes, n_classes), dtype=np.int64)
    np.add.at(counts, (real_pred, fake_pred), 1)
    rows = counts.sum(axis=1, keepdims=True).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        cm = np.where(rows > 0, counts / np.where(rows > 0, rows, 1.0), np.nan)
    return cm, counts


def jerk_stats(values):
    """(mean, unbiased standard deviation) of per-sequence jerkiness values (torch.std's default; NaN for one value)"""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    return float(v.mean()), (float(v.std(ddof=1)) if v.size > 1 else float("nan"))


def jerk_per_sequence(poses):
    """poses (N, T, 69) -> [losses.jerkiness of each sequence]: one launch a sequence, since the reference scores the
    per-sequence values (phase3/test.py:76-104), not a batch mean"""
    return [losses.jerkiness(poses[i:i + 1].permute(0, 2, 1)) for i in range(poses.shape[0])]


def subset(rows, n, seed):
    """a seeded random subset of n rows (all of them when n is None or there are no more), in their original order"""
    if n is None or rows.shape[0] <= n:
        return rows
    g = torch.Generator().manual_seed(seed)
    idx = torch.randperm(rows.shape[0], generator=g)[:n].sort().values
    return rows[idx.to(rows.device)].contiguous()


def distribution_scores(real, fake, tag, max_rows=None, seed=0):
    """Features of the real rows (N, D) and of the generated rows (M, D) - or a list of generated sets, of which the
    first is scored - both standardised by the REAL set's moments -> `fd_<tag>` (Frechet distance real against
    generated), `fd_<tag>_real_split` (even against odd real rows, the sampling floor; NaN when N < 4),
    `fd_<tag>_converged`, `div_<tag>_real` and `div_<tag>_fake` (mean pairwise distance, with max_rows over a seeded
    subset of at most that many rows: the pairwise kernel is quadratic in fp64), and the standardised rows `Zr` and
    `Zf` (as `fake` came: a set or a list). N < 2: NaN scores, None for the rest, no device work. Both Frechet pairs go
    through ONE m2d_frechet call; the only host reads are the final scalars."""
    nan = float("nan")
    res = {"fd_%s" % tag: nan, "fd_%s_real_split" % tag: nan, "fd_%s_converged" % tag: None,
           "div_%s_real" % tag: nan, "div_%s_fake" % tag: nan, "Zr": None, "Zf": None}
    N = real.shape[0]
    if N < 2:
        return res
    mean, cov = metrics.feature_moments(real)
    Zr = metrics.standardize(real, mean, cov)
    sets = fake if isinstance(fake, (list, tuple)) else [fake]
    Zf = [metrics.standardize(f, mean, cov) for f in sets]
    pairs = [(Zr, Zf[0])] + ([(Zr[0::2], Zr[1::2])] if N >= 4 else [])
    mom = [[metrics.feature_moments(x) for x in pair] for pair in pairs]
    fd = metrics.frechet_from_moments(torch.stack([m[0][0] for m in mom]), torch.stack([m[0][1] for m in mom]),
                                      torch.stack([m[1][0] for m in mom]), torch.stack([m[1][1] for m in mom]))
    vals = fd["fd"].cpu().numpy()
    res["fd_%s" % tag] = float(vals[0])
    if len(pairs) > 1:
        res["fd_%s_real_split" % tag] = float(vals[1])
    res["fd_%s_converged" % tag] = bool((fd["converged"] != 0).all().cpu())
    res["div_%s_real" % tag] = float(metrics.mean_pairwise_distance(subset(Zr, max_rows, seed))[0].cpu())
    res["div_%s_fake" % tag] = float(metrics.mean_pairwise_distance(subset(Zf[0], max_rows, seed))[0].cpu())
    res.update(Zr=Zr, Zf=Zf if sets is fake else Zf[0])
    return res
