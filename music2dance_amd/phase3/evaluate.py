"""Score a trained phase-3 generator as the reference's phase3/test.py:76-140 does, on the HIP path.

    python -m music2dance_amd.phase3.evaluate -c music2dance_amd/phase3/configs/default.yaml -l <logdir> \
        --classifier logs/type2/weights.pt [--gen-weights PATH] [--repeats 20] [--synthetic] [--beat-align] \
        [--frechet [--modes K] [--prdc [K]]]

1. Jerkiness (losses.jerkiness) of every real validation take and of the dance generated from its music, on
   inverse-MinMax-scaled poses: mean and unbiased standard deviation of each.
2. Style consistency: the dance-style classifier (dance_classification.archis.default.RecurrentDanceClassifier, eval
   mode) labels each real take and its generated counterpart; the confusion matrix of real-predicted (rows) against
   fake-predicted (columns) labels, row-normalised. It is always C x C, a row without samples is NaN (sklearn's matrix
   shrinks to the labels present instead).

The validation takes are <logdir>/trainvaltest_samples.json's `val_samples`, each drawn `--repeats` times (a fresh
random crop per draw, as the reference's loader makes); all draws go through ONE eval-mode generator call (eval-mode
BatchNorm keeps the rows independent, so only the order of the noise draws differs from the reference's batch-1 loop).
The generator checkpoint defaults to the latest <logdir>/models/gpgen_*.pt. Writes <logdir>/evaluation.json, strict
JSON: an undefined value (a confusion row without samples, the spread of a single sequence) is `null`.

--beat-align adds the music-dance beat alignment (metrics.beat_scores) of every real draw and of
its generated counterpart against the draw's own audio row: `beat_align_{real,fake}_{mean,std}`,
`beat_cover_{real,fake}_{mean,std}` over the rows whose score is defined (a row without a kinematic beat or without an
onset has none) and `beat_defined_{real,fake}`, the number of such rows. Without the flag evaluation.json is what it
was.

--frechet adds the distribution scores of DESIGN.md section 14 on the kinetic features (metrics.kinetic_features at the
config's video_rate) of the inverse-scaled real and generated draws, both standardised by the REAL set's moments:
`fd_kinetic` (Frechet distance real against generated), `fd_kinetic_real_split` (even against odd real rows: the
sampling floor `fd_kinetic` is to be read against), `div_kinetic_real`, `div_kinetic_fake` (mean pairwise distance),
`fd_kinetic_converged` and `kinetic_dims`. --modes K (K >= 2, needs --frechet) runs the generator K times on the same
audio slices, fresh noise each time, and adds `multimodality_kinetic`: the mean pairwise distance among the K dances
of a slice, averaged over the slices. A value that needs more rows than there are is `null`.

--prdc [K] (default 5, needs --frechet) adds the k-nearest-neighbour scores of DESIGN.md section 15 (metrics.prdc) on the
same standardised kinetic features, real rows against generated rows: `precision_kinetic`, `recall_kinetic`,
`density_kinetic`, `coverage_kinetic`, `nn_ratio_median_kinetic`, `nn_fake_to_real_median_kinetic`,
`nn_real_to_real_median_kinetic` and `prdc_k`; `null` with fewer than K + 1 rows.
"""
import argparse
import glob
import json
import os
import re

import numpy as np
import torch

from .. import losses, ops, runner
from ..dance_classification.archis.default import RecurrentDanceClassifier
from .archis.default import SequenceGenerator

N_STYLES = 4
STICK_CHANNELS = 69


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, required=True, help="phase-3 config file of the generator")
    ap.add_argument("-l", "--logdir", type=str, required=True, help="run directory of the generator")
    ap.add_argument("--gen-weights", type=str, default=None, help="generator state_dict (default: latest "
                                                                    "<logdir>/models/gpgen_*.pt)")
    ap.add_argument("--classifier", type=str, required=True, help="RecurrentDanceClassifier state_dict")
    ap.add_argument("--repeats", type=int, default=20, help="draws of every validation take")
    ap.add_argument("--synthetic", action="store_true", help="random poses / audio / styles of the dataset's shapes")
    ap.add_argument("--folder", type=str, default=None, help="dataset folder (overrides the YAML's `folder:`)")
    ap.add_argument("-d", "--device", type=int, default=None, help="choose gpu id")
    ap.add_argument("--beat-align", action="store_true", help="also score the beat alignment of the real and the "
                                                              "generated dances with their music")
    ap.add_argument("--frechet", action="store_true", help="also score the Frechet distance and the diversity of the "
                                                           "kinetic features of the real and the generated dances")
    ap.add_argument("--modes", type=int, default=None, help="with --frechet: generate K >= 2 dances per audio slice "
                                                            "and score their multimodality")
    ap.add_argument("--prdc", type=int, nargs="?", const=5, default=None,
                    help="with --frechet: k-nearest-neighbour precision, recall, density and coverage of the kinetic "
                         "features, K neighbours (default 5)")
    opts = ap.parse_args(argv)
    if opts.modes is not None and not opts.frechet:
        ap.error("--modes requires --frechet")
    if opts.prdc is not None and not opts.frechet:
        ap.error("--prdc requires --frechet")
    if opts.prdc is not None and opts.prdc < 1:
        ap.error("--prdc needs K >= 1")
    if opts.modes is not None and opts.modes < 2:
        ap.error("--modes needs K >= 2")
    return opts


def latest_checkpoint(logdir):
    """<logdir>/models/gpgen_<iteration>.pt with the largest iteration, or None"""
    best, best_it = None, -1
    for p in glob.glob(os.path.join(logdir, "models", "gpgen_*.pt")):
        m = re.search(r"gpgen_(\d+)\.pt$", p)
        if m and int(m.group(1)) > best_it:
            best, best_it = p, int(m.group(1))
    return best


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


def beat_stats(align, cover, tag):
    """The beat-alignment keys of one side (`tag` = real / fake): mean and unbiased standard deviation of beat_align
    and beat_cover over the rows where the score is defined (both are NaN together), and how many rows those are"""
    align = np.asarray(align, dtype=np.float64).reshape(-1)
    cover = np.asarray(cover, dtype=np.float64).reshape(-1)
    ok = np.isfinite(align) & np.isfinite(cover)
    out = {"beat_defined_%s" % tag: int(ok.sum())}
    for name, v in (("align", align[ok]), ("cover", cover[ok])):
        out["beat_%s_%s_mean" % (name, tag)] = float(v.mean()) if v.size else float("nan")
        out["beat_%s_%s_std" % (name, tag)] = float(v.std(ddof=1)) if v.size > 1 else float("nan")
    return out


def beat_rows(audio, real_i, fake_i, hop, rate):
    """-> {'real': (align, cover), 'fake': (align, cover)}, numpy (N,) each: metrics.beat_scores of the inverse-scaled
    dances (N, T, 69) against the audio rows (N, S) they were drawn with. A drawn take's audio row starts at its first
    pose frame (SequenceDataset.sample_batch), so pose frame t belongs to samples [t hop, (t + 1) hop) of the row."""
    from .. import metrics
    out = {}
    for tag, poses in (("real", real_i), ("fake", fake_i)):
        s = metrics.beat_scores(audio, poses.contiguous(), hop, rate=rate)
        out[tag] = (s["align"].cpu().numpy(), s["cover"].cpu().numpy())
    return out


def kinetic_rows(real_i, fakes_i, fps, up_axis=1, prdc_k=None):
    """The keys of --frechet (and, for more than one generated set, of --modes): real_i (N, T, 69) and the list fakes_i
    of generated sets of the same shape, inverse-scaled; set k row n is the k-th dance made for the music of real row
    n. Features are standardised by the real set's moments; both Frechet pairs go through ONE m2d_frechet call. The
    only host reads are the final scalars. prdc_k (--prdc): also metrics.prdc of the standardised real rows against
    the first generated set with that many neighbours, keys suffixed `_kinetic`, and `prdc_k`."""
    from .. import metrics
    nan = float("nan")
    N = real_i.shape[0]
    Fr = metrics.kinetic_features(real_i.contiguous(), fps, up_axis)
    Ff = [metrics.kinetic_features(f.contiguous(), fps, up_axis) for f in fakes_i]
    res = {"fd_kinetic": nan, "fd_kinetic_real_split": nan, "div_kinetic_real": nan, "div_kinetic_fake": nan,
           "fd_kinetic_converged": None, "kinetic_dims": int(Fr.shape[1])}
    if len(fakes_i) > 1:
        res["multimodality_kinetic"] = nan
    if prdc_k is not None:
        res.update({"%s_kinetic" % key: nan for key in metrics.PRDC_KEYS})
        res["prdc_k"] = int(prdc_k)
    if N < 2:
        return res
    mean, cov = metrics.feature_moments(Fr)
    Zr = metrics.standardize(Fr, mean, cov)
    Zf = [metrics.standardize(f, mean, cov) for f in Ff]
    pairs = [(Zr, Zf[0])] + ([(Zr[0::2], Zr[1::2])] if N >= 4 else [])
    mom = [[metrics.feature_moments(x) for x in pair] for pair in pairs]
    fd = metrics.frechet_from_moments(torch.stack([m[0][0] for m in mom]), torch.stack([m[0][1] for m in mom]),
                                      torch.stack([m[1][0] for m in mom]), torch.stack([m[1][1] for m in mom]))
    vals = fd["fd"].cpu().numpy()
    res["fd_kinetic"] = float(vals[0])
    if len(pairs) > 1:
        res["fd_kinetic_real_split"] = float(vals[1])
    res["fd_kinetic_converged"] = bool((fd["converged"] != 0).all().cpu())
    res["div_kinetic_real"] = float(metrics.mean_pairwise_distance(Zr)[0].cpu())
    res["div_kinetic_fake"] = float(metrics.mean_pairwise_distance(Zf[0])[0].cpu())
    if len(Zf) > 1:
        Z = torch.stack(Zf, 1).reshape(N * len(Zf), -1).contiguous()       # the dances of a slice are consecutive rows
        res["multimodality_kinetic"] = float(metrics.mean_pairwise_distance(Z, groups=N).mean().cpu())
    if prdc_k is not None and N >= prdc_k + 1:
        for key, val in metrics.prdc(Zr, Zf[0], prdc_k).items():
            res["%s_kinetic" % key] = float(val.cpu())
    return res


def summary(real_jerk, fake_jerk, real_pred, fake_pred, n_classes=N_STYLES, beat=None, kinetic=None):
    """beat: beat_rows' result, or None (the keys of --beat-align are then absent); kinetic: kinetic_rows' result, or
    None (the keys of --frechet are then absent)"""
    cm, counts = confusion(real_pred, fake_pred, n_classes)
    rm, rs = jerk_stats(real_jerk)
    fm, fs = jerk_stats(fake_jerk)
    total = int(counts.sum())
    res = {"jerk_real_mean": rm, "jerk_real_std": rs, "jerk_fake_mean": fm, "jerk_fake_std": fs,
           "confusion": cm.tolist(), "style_agreement": float(np.trace(counts)) / total if total else float("nan"),
           "n_sequences": total}
    if beat is not None:
        for tag in ("real", "fake"):
            res.update(beat_stats(beat[tag][0], beat[tag][1], tag))
    if kinetic is not None:
        res.update(kinetic)
    return res


def json_safe(v):
    """NaN / inf -> None (JSON null), recursively through lists and dicts"""
    if isinstance(v, dict):
        return {k: json_safe(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [json_safe(x) for x in v]
    if isinstance(v, float) and not np.isfinite(v):
        return None
    return v


def build_generator(cfg, device):
    rate = cfg["dataset"]["audio_rate"]
    return SequenceGenerator(int(cfg["window_size"] * rate), cfg["input_vector_size"], cfg["latent_vector_size"],
                             cfg["size"], cfg["output_size"], cfg["noise_size"], cfg["nblocks_gen"], cfg["n_cells"],
                             cfg["enc_type"], cfg["activ"], device)


def _takes(opts, cfg, device):
    """-> (real poses (N, T, 69), audio tracks (N, S), labels (N,), scaler, window, hop): the validation takes,
    each drawn `repeats` times."""
    from .. import data as D
    ds = cfg["dataset"]
    window = int(cfg["window_size"] * ds["audio_rate"])
    hop = int(ds["audio_rate"] // ds["video_rate"])
    split = os.path.join(opts.logdir, "trainvaltest_samples.json")
    if opts.synthetic:
        n_val = 6
        if os.path.exists(split):
            with open(split) as f:
                n_val = max(len(json.load(f).get("val_samples", [])), 1)
        from ..engine import synthetic_phase3_batch
        T = int(ds["seq_length"] * ds["video_rate"])
        real, audio, _ = synthetic_phase3_batch(n_val * opts.repeats, T, device, seed=12345,
                                                audio_rate=ds["audio_rate"], video_rate=ds["video_rate"],
                                                window_s=cfg["window_size"])
        g = torch.Generator(device=device).manual_seed(12346)
        labels = torch.randint(0, N_STYLES, (n_val,), generator=g, device=device).repeat(opts.repeats)
        scaler = D.MinMaxScaler().fit(real.reshape(-1, STICK_CHANNELS).cpu().numpy())
        return real, audio, labels, scaler, window, hop
    with open(split) as f:
        val_dirs = json.load(f)["val_samples"]
    folder = runner.dataset_folder(cfg, opts.folder)
    sticks = D.StickDataset(folder, normalize="minmax")
    dataset = D.SequenceDataset(folder, ds, dance_types=cfg["dance_types"], scaler=sticks.scaler, withaudio=True)
    dataset.truncate()
    where = {d: i for i, d in enumerate(dataset.dirs)}
    missing = [d for d in val_dirs if d not in where]
    if missing:
        raise SystemExit("validation takes not in the dataset: %s" % missing[:5])
    idx = [where[d] for d in val_dirs]
    parts = [dataset.sample_batch(idx, device) for _ in range(opts.repeats)]
    real = torch.cat([p[0].reshape(len(idx), dataset.stick_length, STICK_CHANNELS) for p in parts]).float()
    audio = torch.cat([p[2] for p in parts]).float()
    labels = torch.cat([p[3].reshape(-1) for p in parts]).long()
    return real, audio, labels, sticks.scaler, int(cfg["window_size"] * dataset.aud_rate), dataset.ratio


@torch.no_grad()
def evaluate(opts, cfg, device):
    from ..utils import slice_audio_batch
    gen = build_generator(cfg, device)
    path = opts.gen_weights or latest_checkpoint(opts.logdir)
    if path is not None:
        gen.load_state_dict(torch.load(path, map_location=device))
    elif not opts.synthetic:
        raise SystemExit("no generator checkpoint: pass --gen-weights or train into %s/models" % opts.logdir)
    classifier = RecurrentDanceClassifier(STICK_CHANNELS, 128, N_STYLES).to(device)
    classifier.load_state_dict(torch.load(opts.classifier, map_location=device))
    gen.eval(), classifier.eval()

    real, audio, labels, scaler, window, hop = _takes(opts, cfg, device)
    N, T, _ = real.shape
    real = real.contiguous()
    slices = slice_audio_batch(audio.contiguous(), window, hop, window - hop, lazy=True)
    fake = gen(slices, [T] * N).reshape(N, T, STICK_CHANNELS)

    # jerkiness per sequence on the inverse-scaled poses (phase3/test.py:76-104)
    real_i = scaler.inverse_transform_device(real)
    fake_i = scaler.inverse_transform_device(fake.contiguous())
    real_jerk = torch.stack([losses.jerkiness(real_i[i:i + 1].permute(0, 2, 1)) for i in range(N)])
    fake_jerk = torch.stack([losses.jerkiness(fake_i[i:i + 1].permute(0, 2, 1)) for i in range(N)])

    # style classification of every real take and its generated counterpart (phase3/test.py:107-140)
    _, real_pred = ops.cross_entropy_pred(classifier(real.permute(0, 2, 1).contiguous()), labels)
    _, fake_pred = ops.cross_entropy_pred(classifier(fake.permute(0, 2, 1).contiguous()), labels)
    beat = None
    if getattr(opts, "beat_align", False):
        beat = beat_rows(audio.contiguous(), real_i, fake_i, hop, int(cfg["dataset"]["audio_rate"]))
    kinetic = None
    if getattr(opts, "frechet", False):
        # --modes K: K - 1 further generator calls on the same slices (each draws its own noise), after everything
        # the scores above are made of
        more = [scaler.inverse_transform_device(gen(slices, [T] * N).reshape(N, T, STICK_CHANNELS).contiguous())
                for _ in range((getattr(opts, "modes", None) or 1) - 1)]
        kinetic = kinetic_rows(real_i, [fake_i] + more, float(cfg["dataset"]["video_rate"]),
                               prdc_k=getattr(opts, "prdc", None))
    return summary(real_jerk.cpu().numpy(), fake_jerk.cpu().numpy(), real_pred.cpu().numpy(),
                   fake_pred.cpu().numpy(), beat=beat, kinetic=kinetic)


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
