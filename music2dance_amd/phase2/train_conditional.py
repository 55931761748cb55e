"""Phase 2, style-conditioned: the label-conditioned sequence WGAN-LP on MI355X.

    python -m music2dance_amd.phase2.train_conditional -c music2dance_amd/phase2/configs/default.yaml -d 0 -n run \
        -f wgangp --synthetic

Flags -c/-d/-n/-f and YAML keys as in the reference's phase2/train_conditional.py, with the extras of phase2/train.py.
The networks are phase2/archis/conditional.py's; the loop is the script's `wgangp` branch (:109-185) as the archis force
it (engine.Phase2CondEngine): the real rows' styles come from the dataset's label column, every fake
batch draws its own, uniform over {0..3}; plain Adam, no schedulers; dropout masks and noise drawn on the device.
Logs loss_critic / loss_gen / gp / w_dist with the reference's signs and saves gpgen_ / gpcritic_ every 5000 epochs.
Only `wgangp` runs: the reference's conditional `gan` branch needs the auxiliary head the archis do not have (and
maximises its real-row BCE); any other value raises the reference's error.
"""
import functools

import torch

from .. import runner
from ..engine import Phase2CondEngine
from .archis.conditional import N_CLASSES, SequenceDiscriminator, SequenceGenerator
from .train import checkpoints, wgangp_scalars as scalars


def parser():
    return runner.train_parser(framework="`wgangp` (the only conditional framework)")


def main(argv=None):
    opts = parser().parse_args(argv)
    if opts.framework != "wgangp":
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
        kernels.set_plan_model(5)   # as phase2/train.py: one critic branch, the launch-by-launch cost model
    engine = Phase2CondEngine(gen, critic, cfg, sync_bn=opts.sync_bn)
    torch.manual_seed(run.rank)  # identical weights (seed 0 above), rank-distinct draws
    engine.host_noise = False  # labels, noise, alpha and dropout masks on the device
    ema = runner.enable_ema(engine, cfg)

    def synthetic(seed):  # random poses and random styles
        g = torch.Generator().manual_seed(seed)
        poses = torch.rand(batch_size, stick_length, cfg["output_size"], generator=g)
        labels = torch.randint(0, N_CLASSES, (batch_size,), generator=g)
        return (poses.to(device), labels.to(device)), None

    def batches(epoch):
        if loader is None:
            return map(synthetic, runner.synthetic_seeds(run, epoch))
        if isinstance(loader, DataLoader):
            return (((p.float().reshape(p.size(0), stick_length, -1), lbl), None)
                    for p, lbl in (runner.staged((b[0], b[2]), device)[0] for b in loader))
        return (((b[0].reshape(b[0].size(0), stick_length, -1), b[2]), None)
                for b, _ in runner.resident_batches(loader, device))

    runner.train(run, logdir, engine, batches, scalars, functools.partial(checkpoints, ema=ema),
                 train_mode=("gen", "critic"))
    return engine


if __name__ == "__main__":
    main()
