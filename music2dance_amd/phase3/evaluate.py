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
JSON: an undefined value (a confusion row without samples, the spread of a single sequence) is `null`. What this script
shares with phase1.evaluate, phase2.evaluate and phase3.generate (flags, loaders, the take lookup, `confusion`,
`jerk_stats`, `json_safe`, the Frechet / diversity block) is scoring.py's.

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
import json
import os

import numpy as np
import torch

from .. import metrics, ops, scoring
from ..scoring import N_STYLES, STICK_CHANNELS, confusion, jerk_stats, json_safe, latest_checkpoint  # noqa: F401
from .archis.default import build_generator


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    scoring.add_common_flags(ap, 3, "gpgen", "random poses / audio / styles of the dataset's shapes")
    ap.add_argument("--classifier", type=str, required=True, help="RecurrentDanceClassifier state_dict")
    ap.add_argument("--repeats", type=int, default=20, help="draws of every validation take")
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
    out = {}
    for tag, poses in (("real", real_i), ("fake", fake_i)):
        s = metrics.beat_scores(audio, poses.contiguous(), hop, rate=rate)
        out[tag] = (s["align"].cpu().numpy(), s["cover"].cpu().numpy())
    return out


def kinetic_rows(real_i, fakes_i, fps, up_axis=1, prdc_k=None):
    """The keys of --frechet (and, for more than one generated set, of --modes): real_i (N, T, 69) and the list fakes_i
    of generated sets of the same shape, inverse-scaled; set k row n is the k-th dance made for the music of real row
    n. The Frechet and diversity keys are scoring.distribution_scores' of the kinetic features. prdc_k (--prdc): also
    metrics.prdc of the standardised real rows against the first generated set with that many neighbours, keys
    suffixed `_kinetic`, and `prdc_k`. The only host reads are the final scalars."""
    nan = float("nan")
    N = real_i.shape[0]
    Fr = metrics.kinetic_features(real_i.contiguous(), fps, up_axis)
    Ff = [metrics.kinetic_features(f.contiguous(), fps, up_axis) for f in fakes_i]
    dist = scoring.distribution_scores(Fr, Ff, "kinetic")
    res = {key: dist[key] for key in ("fd_kinetic", "fd_kinetic_real_split", "div_kinetic_real", "div_kinetic_fake",
                                      "fd_kinetic_converged")}
    res["kinetic_dims"] = int(Fr.shape[1])
    if len(fakes_i) > 1:
        res["multimodality_kinetic"] = nan
    if prdc_k is not None:
        res.update({"%s_kinetic" % key: nan for key in metrics.PRDC_KEYS})
        res["prdc_k"] = int(prdc_k)
    if N < 2:
        return res
    Zr, Zf = dist["Zr"], dist["Zf"]
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
    _, idx, dataset, scaler = scoring.validation_takes(opts, cfg)
    dataset.truncate()
    parts = [dataset.sample_batch(idx, device) for _ in range(opts.repeats)]
    real = torch.cat([p[0].reshape(len(idx), dataset.stick_length, STICK_CHANNELS) for p in parts]).float()
    audio = torch.cat([p[2] for p in parts]).float()
    labels = torch.cat([p[3].reshape(-1) for p in parts]).long()
    return real, audio, labels, scaler, int(cfg["window_size"] * dataset.aud_rate), dataset.ratio


@torch.no_grad()
def evaluate(opts, cfg, device):
    from ..utils import slice_audio_batch
    gen = build_generator(cfg, device)
    scoring.load_generator(gen, opts)
    classifier = scoring.load_classifier(opts.classifier, device)

    real, audio, labels, scaler, window, hop = _takes(opts, cfg, device)
    N, T, _ = real.shape
    real = real.contiguous()
    slices = slice_audio_batch(audio.contiguous(), window, hop, window - hop, lazy=True)
    fake = gen(slices, [T] * N).reshape(N, T, STICK_CHANNELS)

    # jerkiness per sequence on the inverse-scaled poses (phase3/test.py:76-104)
    real_i = scaler.inverse_transform_device(real)
    fake_i = scaler.inverse_transform_device(fake.contiguous())
    real_jerk = torch.stack(scoring.jerk_per_sequence(real_i))
    fake_jerk = torch.stack(scoring.jerk_per_sequence(fake_i))

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
    return scoring.run(parse_args, evaluate, argv, out="evaluation.json", seed=0)


if __name__ == "__main__":
    main()
