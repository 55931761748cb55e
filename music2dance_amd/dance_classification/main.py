"""Train the dance-style classifier on MI355X.

    python -m music2dance_amd.dance_classification.main -c music2dance_amd/dance_classification/configs/default.yaml \
        -d 0 -n type2 [--synthetic] [--epochs N]

Same flags (-c/-d/-n), YAML keys, split (numpy seed 19), class-balanced samplers, per-epoch train / validation losses
and output files (logs/<name>/trainvaltest_samples.json, logs/<name>/weights.pt) as the reference's
dance_classification/main.py; the loop body is engine.ClassifierEngine.
"""
import argparse
import json
import os

import torch

from .. import runner
from ..scoring import N_STYLES, STICK_CHANNELS
from .archis.default import RecurrentDanceClassifier
from .engine import ClassifierEngine


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, help="choose config file")
    ap.add_argument("-d", "--device", type=int, help="choose gpu id")
    ap.add_argument("-n", "--name", type=str, help="choose name of experiment")
    ap.add_argument("--synthetic", action="store_true", help="random poses / labels of the dataset's shapes")
    ap.add_argument("--epochs", type=int, default=None, help="override num_epochs")
    ap.add_argument("--folder", type=str, default=None, help="dataset folder (overrides the YAML's `folder:`)")
    ap.add_argument("--synthetic-takes", type=int, default=61, help="--synthetic: takes in the random dataset")
    return ap.parse_args(argv)


def stick_length(cfg):
    ds = cfg["dataset"]
    return int(ds["seq_length"] * ds["video_rate"])


def synthetic_takes(n, T, device, seed):
    """n random takes (poses U[0,1) of shape (n, 69, T), styles uniform in 0..3) from the device generator"""
    g = torch.Generator(device=device).manual_seed(seed)
    sticks = torch.rand(n, STICK_CHANNELS, T, generator=g, device=device)
    labels = torch.randint(0, N_STYLES, (n,), generator=g, device=device)
    return sticks, labels


def _loaders(cfg, folder, batch_size, logdir, device):
    """dance_classification/main.py:29-106: minmax-scaled sequences, the seed-19 split written to
    trainvaltest_samples.json, class-balanced samplers, validation as one batch; batches gathered in HBM."""
    from torch.utils.data import WeightedRandomSampler

    from .. import data as D
    sticks = D.StickDataset(folder, normalize="minmax")
    dataset = D.SequenceDataset(folder, cfg["dataset"], dance_types=cfg["dance_types"], scaler=sticks.scaler,
                                withaudio=False)
    dataset.truncate()
    parts = dict(zip(("train", "val", "test"), D.split_indices(len(dataset), random_seed=19)))
    with open(os.path.join(logdir, "trainvaltest_samples.json"), "w") as f:
        json.dump({k + "_samples": [dataset.dirs[i] for i in v] for k, v in parts.items()}, f)

    def loader(idx, per_batch):
        if not idx:
            return None
        sampler = WeightedRandomSampler(D.class_balanced_weights(dataset.labels, idx), len(idx))
        return D.ResidentLoader(dataset.subset(idx, withaudio=False), per_batch, sampler, device)

    return loader(parts["train"], batch_size), loader(parts["val"], len(parts["val"]))


def main(argv=None):
    opts = parse_args(argv)
    logdir = "./logs/" + str(opts.name)
    os.makedirs(logdir, exist_ok=True)
    cfg = runner.load_config(opts.config)
    device = runner.pick_device(opts.device)
    batch_size = cfg["batch_size"]
    num_epochs = cfg["num_epochs"] if opts.epochs is None else opts.epochs
    T = stick_length(cfg)

    if opts.synthetic:
        n = opts.synthetic_takes
        from .. import data as D
        parts = dict(zip(("train", "val", "test"), D.split_indices(n, random_seed=19)))
        with open(os.path.join(logdir, "trainvaltest_samples.json"), "w") as f:
            json.dump({k + "_samples": ["SYNTHETIC_%d" % i for i in v] for k, v in parts.items()}, f)
        all_sticks, all_labels = synthetic_takes(n, T, device, seed=19)
        tr = torch.as_tensor(parts["train"], device=device)
        va = torch.as_tensor(parts["val"], device=device)

        def train_batches(epoch):
            g = torch.Generator(device=device).manual_seed(1 + epoch)
            order = tr[torch.randperm(len(tr), generator=g, device=device)]
            for i in range(0, len(order), batch_size):
                yield all_sticks[order[i:i + batch_size]], all_labels[order[i:i + batch_size]]

        def val_batches():
            if len(va):
                yield all_sticks[va], all_labels[va]
    else:
        train_loader, val_loader = _loaders(cfg, runner.dataset_folder(cfg, opts.folder), batch_size, logdir, device)

        def as_batch(b):
            poses, labels = b[0], b[-2]
            B = poses.shape[0]
            return poses.reshape(B, T, STICK_CHANNELS).permute(0, 2, 1).contiguous(), labels.reshape(-1).long()

        def train_batches(epoch):
            for b in train_loader:
                yield as_batch(b)

        def val_batches():
            if val_loader is not None:
                for b in val_loader:
                    yield as_batch(b)

    model = RecurrentDanceClassifier(STICK_CHANNELS, 128, N_STYLES).to(device)
    engine = ClassifierEngine(model, cfg["lr"])
    log = runner.ScalarLog(logdir, 1)
    n_valid_steps = 1
    print("Start training..")
    for epoch in range(num_epochs):
        losses = [engine.train_step(sticks, labels) for sticks, labels in train_batches(epoch)]
        if losses:
            log.scalars({"loss_train": torch.stack(losses).mean()}, epoch, force=True)
        if epoch % n_valid_steps == 0:
            vals = [engine.evaluate(sticks, labels)[0] for sticks, labels in val_batches()]
            if vals:
                log.scalars({"loss_val": torch.stack(vals).mean()}, epoch, force=True)
    log.flush()
    torch.save(model.state_dict(), logdir + "/weights.pt")
    print("done: %d epochs, %d steps, weights in %s" % (num_epochs, engine.total_iterations, logdir + "/weights.pt"))
    return engine, log


if __name__ == "__main__":
    main()
