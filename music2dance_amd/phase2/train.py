"""Phase 2: unconditional sequence GAN on MI355X, WGAN-LP (`-f wgangp`) or vanilla (`-f gan`).

    python -m music2dance_amd.phase2.train -c music2dance_amd/phase2/configs/default.yaml -d 0 -n run -f wgangp --synthetic
    python -m music2dance_amd.phase2.train -c music2dance_amd/phase2/configs/default.yaml -d 0 -n run -f gan --synthetic

Flags -c/-d/-n/-f and YAML keys as in the reference's phase2/train.py. `wgangp` runs engine.Phase2Engine
(phase2/train.py:130-195) and logs loss_critic / loss_gen / gp / w_dist; `gan` runs engine.Phase2GanEngine
(phase2/train.py:204-268): BCEWithLogitsLoss with float labels (the reference's int64 labels are refused by current
torch), a generator step and both scheduler steps on every iteration, scalars logged as loss_D / loss_G. Both keep this
port's checkpoint schedule (gpgen_ / gpcritic_ every 5000 epochs). Any other value raises the reference's error.
"""
import functools

import torch

from .. import runner
from ..engine import Phase2Engine, Phase2GanEngine
from .archis.default import SequenceDiscriminator, SequenceGenerator


def parser():
    return runner.train_parser(framework="choose between `wgangp` and `gan`", graphs=(
        "replay each loop body from captured HIP graphs (default on a single GPU: round 6 - with the TemporalBlock kernels "
        "a loop body is 1.2 ms of GPU work and the eager loop is bound by the host's launch rate: 16.4 k vs 19.7 k "
        "sequences / s at batch 32)"))


def checkpoints(epoch, ema=False):
    """ema: the run keeps an averaged generator (YAML `ema_decay`), saved as gpgen_ema_<n>.pt beside gpgen_<n>.pt"""
    n = epoch + 1
    return runner.with_ema([("gen", "gpgen_%d.pt" % n), ("critic", "gpcritic_%d.pt" % n)] if n % 5000 == 0 else [], ema)


def wgangp_scalars(out):
    if "loss_gen" in out:
        return {"loss_critic": -out["loss_critic"], "loss_gen": out["loss_gen"], "gp": out["gp"], "w_dist": -out["w_dist"]}


def gan_scalars(out):
    return {"loss_D": out["loss_critic"], "loss_G": out["loss_gen"]}


def main(argv=None):
    opts = parser().parse_args(argv)
    if opts.framework not in ("wgangp", "gan"):
        raise ValueError("Please state existing framework")
    run = runner.start(opts)
    cfg, device = run.cfg, run.device
    torch.manual_seed(0)
    stick_length, batch_size = runner.sequence_shape(run)
    loader = None
    if not opts.synthetic:
        from torch.utils.data import DataLoader
        loader, stick_length = runner.pose_sequence_loader(run, batch_size)
    logdir = runner.run_dir(run)
    gen = SequenceGenerator(cfg["input_vector_size"], cfg["latent_vector_size"], cfg["size"], cfg["output_size"],
                            cfg["nblocks_gen"], cfg["n_cells"], device)
    critic = SequenceDiscriminator(cfg["output_size"], cfg["channels"], stick_length, cfg["init_kernel"],
                                   cfg["nblocks_critic"], device)
    if next(critic.parameters()).is_cuda:
        from .. import kernels
        kernels.set_plan_model(5)   # no second critic branch to overlap with: the launch-by-launch cost model
    gan = opts.framework == "gan"
    engine = (Phase2GanEngine if gan else Phase2Engine)(gen, critic, cfg, sync_bn=opts.sync_bn)
    torch.manual_seed(run.rank)  # identical weights (seed 0 above), rank-distinct noise / alpha draws
    engine.host_noise = False  # phase2/train.py:139-140 draws the noise on the device
    ema = runner.enable_ema(engine, cfg)
    if runner.graphs_on(run):
        engine.enable_graphs()

    def synthetic(seed):
        g = torch.Generator().manual_seed(seed)
        return (torch.rand(batch_size, stick_length, cfg["output_size"], generator=g).to(device),), None

    def batches(epoch):  # ((real,), no event) each
        if loader is None:
            return map(synthetic, runner.synthetic_seeds(run, epoch))
        if isinstance(loader, DataLoader):
            return ((runner.staged((b[0].float().reshape(b[0].size(0), stick_length, -1),), device)[0], None)
                    for b in loader)
        return (((b[0].reshape(b[0].size(0), stick_length, -1),), None)
                for b, _ in runner.resident_batches(loader, device))

    runner.train(run, logdir, engine, batches, gan_scalars if gan else wgangp_scalars,
                 functools.partial(checkpoints, ema=ema))
    return engine


if __name__ == "__main__":
    main()
