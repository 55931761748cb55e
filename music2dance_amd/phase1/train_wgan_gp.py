"""Phase 1: still-pose residual-MLP WGAN-GP on MI355X.

    python -m music2dance_amd.phase1.train_wgan_gp -c music2dance_amd/phase1/configs/b1l10s128.yaml -d 0 -n run --synthetic

Flags -d/-n as in the reference's phase1/train_wgan-gp.py plus -c for the config file (the
reference reads an undefined `file` variable, phase1/train_wgan-gp.py:31). The hyphenated
script name of the reference is not importable as a module; `train_wgan-gp.py` next to this
file forwards to it.
"""
import functools

import numpy as np
import torch

from .. import runner
from ..engine import Phase1Engine
from .archis.residual import Discriminator, Generator


def parser():
    return runner.train_parser(batch_size=False, graphs=(
        "replay each loop body from captured HIP graphs (the eager loop is bound by the host's launch rate: 2.8 -> 0.86 ms "
        "per body at batch 64); results equal the eager path's. Default on one GPU"))


def checkpoints(epoch, ema=False):
    """ema: the run keeps an averaged generator (YAML `ema_decay`), saved as gen_ema_<n>.pt beside gen_<n>.pt"""
    n = epoch + 1
    return runner.with_ema([("gen", "gen_%d.pt" % n), ("critic", "critic_%d.pt" % n)] if n % 5 == 0 else [], ema)


def scalars(out):
    if "loss_gen" in out:
        return {"loss_critic": -out["loss_critic"], "loss_gen": out["loss_gen"]}


def main(argv=None):
    run = runner.start(parser().parse_args(argv))
    cfg, device = run.cfg, run.device
    B = cfg["batch_size"]
    loader = None
    if not run.opts.synthetic:
        # phase1/train_wgan-gp.py:24-26,71-72: MinMax-scaled still poses, a random subset sampler
        from torch.utils.data import DataLoader
        from .. import data as D
        print("Loading sticks and sequences datasets...")
        dataset = D.StickDataset(runner.dataset_folder(cfg, run.opts.folder), normalize="minmax")
        loader = runner.subset_loader(run, dataset, B)
    logdir = runner.run_dir(run)
    np.random.seed(37)
    gen = Generator(cfg["latent_vector_size"], cfg["size"], cfg["output_size"], cfg["nblocks_gen"]).to(device)
    critic = Discriminator(cfg["output_size"], cfg["size"], cfg["nblocks_critic"]).to(device)
    engine = Phase1Engine(gen, critic, cfg, sync_bn=run.opts.sync_bn)
    if run.world > 1:  # identical weights must come from a common seed; the reference (single process) sets none
        for m in (gen, critic):
            for t in list(m.parameters()) + list(m.buffers()):
                torch.distributed.broadcast(t.data, 0)
        torch.manual_seed(torch.initial_seed() + run.rank)
    engine.host_noise = False  # phase1/train_wgan-gp.py:83 draws the noise on the device
    ema = runner.enable_ema(engine, cfg)   # (after the broadcast: the twin copies the common weights)
    if runner.graphs_on(run):
        engine.enable_graphs()

    def synthetic(seed):
        return (torch.rand(B, 23, 3, generator=torch.Generator().manual_seed(seed)).to(device),), None

    def batches(epoch):  # ((real,), no event) each
        if loader is None:
            return map(synthetic, runner.synthetic_seeds(run, epoch))
        if isinstance(loader, DataLoader):
            return ((runner.staged((b,), device)[0], None) for b in loader)
        return (((b,), None) for b, _ in runner.resident_batches(loader, device))

    # (the reference's phase 1 writes no model_*.txt)
    runner.train(run, logdir, engine, batches, scalars, functools.partial(checkpoints, ema=ema), architectures=False)
    return engine


if __name__ == "__main__":
    main()
