"""Phase 3: audio-conditioned sequence WGAN-GP on MI355X.

    python -m music2dance_amd.phase3.train -c music2dance_amd/phase3/configs/default.yaml -d 0 -n run --synthetic

Same flags (-c/-d/-n), YAML keys, seeds, scalar tags and checkpoint names as the
reference's phase3/train.py; the loop body is engine.Phase3Engine.
"""
import functools

import numpy as np
import torch

from .. import runner
from ..engine import Phase3Engine, synthetic_phase3_batch
from .archis.default import AblatedSequenceDiscriminator, SequenceDiscriminator, SequenceGenerator


LAST_LOG = None  # the ScalarLog of the most recent main() (tests and notebooks read .last)


def build(cfg, device, stick_length):
    rate = cfg["dataset"]["audio_rate"]
    window = int(cfg["window_size"] * rate)
    gen = SequenceGenerator(window, cfg["input_vector_size"], cfg["latent_vector_size"], cfg["size"],
                            cfg["output_size"], cfg["noise_size"], cfg["nblocks_gen"], cfg["n_cells"],
                            cfg["enc_type"], cfg["activ"], device)
    cls = AblatedSequenceDiscriminator if cfg["ablated"] else SequenceDiscriminator
    critic = cls(cfg["output_size"], cfg["channels"], cfg["code_size"], stick_length,
                 init_ker=cfg["init_kernel"], activ=cfg["activ"], device=device)
    return gen, critic


def parser():
    ap = runner.train_parser()
    ap.add_argument("--val-batches", type=int, default=1, help="held-out synthetic batches for l1_loss_val")
    return ap


def checkpoints(epoch, ema=False):
    """ema: the run keeps an averaged generator (YAML `ema_decay`), saved as gpgen_ema_<n>.pt beside gpgen_<n>.pt"""
    n = epoch + 1
    if n % 5000 == 0:
        return runner.with_ema([("gen", "gpgen_%d.pt" % n), ("critic", "gpcritic_%d.pt" % n)], ema)
    return runner.with_ema([("gen", "gpgen_%d.pt" % n)] if n <= 1000 and n % 100 == 0 else [], ema)


def scalars(out):
    if "loss_gen" in out:
        return {"loss_critic": -out["loss_critic"], "loss_gen": out["loss_gen"], "gp": out["gp"],
                "w_dist": -out["w_dist"], "l1_loss_train": out["l1_loss_train"]}


def main(argv=None):
    run = runner.start(parser().parse_args(argv))
    cfg, device, opts, ds = run.cfg, run.device, run.opts, run.cfg["dataset"]
    torch.manual_seed(0)
    stick_length, batch_size = runner.sequence_shape(run)
    logdir = runner.run_dir(run)  # (before the loaders: make_loaders writes the split into it)
    train_loader = val_loader = None
    if not opts.synthetic:
        # phase3/train.py:72-76,112-162: scaler fitted on all still poses, sequences + audio, seeded split,
        # class-balanced samplers
        from .. import data as D
        from ..utils import slice_audio_batch
        dataset = runner.sequence_dataset(run, withaudio=True)
        dataset.truncate()
        stick_length = dataset.stick_length
        resident = device if (device.type == "cuda" and not opts.host_loader) else None
        train_loader, val_loader, _ = D.make_loaders(dataset, batch_size, withaudio=True, logdir=logdir, device=resident)
        window, hop = int(cfg["window_size"] * dataset.aud_rate), dataset.ratio
    gen, critic = build(cfg, device, stick_length)
    engine = Phase3Engine(gen, critic, cfg, ablated=cfg["ablated"], sync_bn=opts.sync_bn)
    ema = runner.enable_ema(engine, cfg)
    # seed 0 built identical weights on every rank; the in-loop host draws (generator noise,
    # penalty alpha) must differ between ranks, as they do between samples of one global batch
    torch.manual_seed(run.rank)

    def started(log):
        global LAST_LOG
        LAST_LOG = log
        np.random.seed(14)

    def loader_batches(loader):
        # the window view of the padded track is made on the copy stream, in front of the `ready` event: the
        # generator forward that reads it runs on a stream of its own and waits for nothing but that event
        def with_slices(b):
            real, audio = b[0], b[2] if len(b) > 2 else b[1]
            return real, audio, slice_audio_batch(audio, window, hop, window - hop, lazy=True)

        if isinstance(loader, D.ResidentLoader):
            return runner.resident_batches(loader, device, derive=with_slices)
        return (runner.staged((real_h.float(), audio_h), device, derive=with_slices)
                for real_h, _, audio_h, _, _ in loader)

    def synthetic(seed, **kw):
        return synthetic_phase3_batch(batch_size, stick_length, device, seed=seed, audio_rate=ds["audio_rate"],
                                      video_rate=ds["video_rate"], window_s=cfg["window_size"], **kw)

    def batches(epoch):
        # staged on the copy stream: the engine may start this batch's generator forward while the
        # previous iteration's critic kernels are still running
        if train_loader is not None:
            return loader_batches(train_loader)
        drawn = (synthetic(seed, with_event=True) for seed in runner.synthetic_seeds(run, epoch))
        return ((b[:3], b[3]) for b in drawn)

    def val_batches():
        # the reference's validation loader serves the held-out 20 % split as one batch
        # (phase3/train.py:161); synthetic runs: fixed held-out synthetic batches, disjoint seeds from training
        if val_loader is not None:
            return ((real, slices) for (real, _, slices), _ in loader_batches(val_loader))
        return (synthetic(-(1 + v * run.world + run.rank))[::2] for v in range(opts.val_batches))

    def validate(epoch, log, done):
        # eval-mode L1 on held-out batches after every epoch (n_valid_steps = 1, phase3/train.py:168,245-261);
        # validation_l1 restores train mode
        e_val = engine.validation_l1(val_batches())
        log.scalars({"l1_loss_val": e_val}, engine.total_iterations, force=True)
        if ema:   # the averaged generator on the same held-out batches (a tag of this port's; the reference's stay)
            log.scalars({"l1_loss_val_ema": engine.validation_l1(val_batches(), gen=engine.gen_ema)},
                        engine.total_iterations, force=True)
        if (epoch + 1) % 500 == 0 and run.rank == 0 and not done:
            o = engine.last_full
            print("Iteration: {} LossG : {} LossD : {} L1 train : {} L1 val : {}".format(
                engine.total_iterations, float(o.get("loss_gen", float("nan"))), float(o["loss_critic"]),
                float(o.get("l1_loss_train", float("nan"))), float(e_val)))

    runner.train(run, logdir, engine, batches, scalars, functools.partial(checkpoints, ema=ema), started=started,
                 epoch_end=validate)
    return engine


if __name__ == "__main__":
    main()
