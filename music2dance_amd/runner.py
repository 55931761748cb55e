"""The training driver of the four GAN train scripts: their flags, run set-up, loaders and the epoch loop (`train`),
with YAML config, run folders, optional TensorBoard and checkpoints under the reference's file names.

The scripts run on `--synthetic` batches of the dataset's shapes, or - through music2dance_amd.data, the
reference's dataset pipeline (utils.py:15-194, phase3/train.py:114-162) - on a Music-to-Dance-Motion-Synthesis
folder (`folder:` of the YAML, or `--folder`).
"""
import argparse
import collections
import datetime
import os

import torch
import yaml

from . import dp


def load_config(path):
    with open(path, "r") as f:
        return yaml.safe_load(f)


def pick_device(idx):
    if not torch.cuda.is_available():
        raise RuntimeError("music2dance_amd trains on an MI355X: no HIP device is visible and there is no CPU path")
    return torch.device("cuda:" + str(0 if idx is None else idx))


def settle_garbage_collector():
    """Call once the models / engine are built: collect, then move everything alive into the permanent
    generation. A full (generation-2) collection over the module / parameter / closure graph of a training
    process takes 60-80 ms of host time (measured, tools/spike_probe.py) - five loop bodies during which the
    launch queue runs dry; afterwards a full collection only walks what the loop itself allocates."""
    import gc
    gc.collect()
    gc.freeze()


def make_run_dir(name, enabled=True):
    if not enabled:
        return None
    os.makedirs("./runs", exist_ok=True)
    logdir = "./runs/" + datetime.datetime.now().strftime("%Y%m%d-%H%M%S") + "_" + str(name)
    os.makedirs(logdir)
    os.makedirs(logdir + "/samples")
    os.makedirs(logdir + "/models")
    return logdir


class ScalarLog:
    """TensorBoard scalars under the reference's tags when tensorboard is importable; otherwise a no-op.
    The reference writes `loss.item()` every generator iteration (phase3/train.py:228-236): a host sync per scalar that
    drains the launch queue. Here a logged value is copied to pinned host memory on the stream that made it
    (non-blocking) and WRITTEN when that copy is known to have finished - on a later `scalars()` call, or in
    `flush()` at the end of the run: same tags, steps and values, no stall in the loop."""

    def __init__(self, logdir, every=1, writer=None):
        self.every = max(int(every), 1)
        self.writer = writer
        self.last = {}  # most recent value per tag (device tensors; tests and prints read it)
        self._queue = []  # (tag, step, host tensor or float, event or None)
        if logdir is not None and writer is None:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(logdir + "/logging")
            except Exception:
                self.writer = None

    def _drain(self, block=False):
        while self._queue:
            tag, step, host, ev = self._queue[0]
            if ev is not None and not block and not ev.query():
                return
            if ev is not None and block:
                ev.synchronize()
            self._queue.pop(0)
            self.writer.add_scalar(tag, float(host), step)

    def scalars(self, values, step, force=False):
        self.last.update(values)
        if self.writer is None or (step % self.every and not force):
            return
        for tag, v in values.items():
            if torch.is_tensor(v) and v.is_cuda:
                host = torch.empty((), dtype=v.dtype, pin_memory=True)
                host.copy_(v.detach().reshape(()), non_blocking=True)
                self._queue.append((tag, step, host, torch.cuda.current_stream(v.device).record_event()))
            else:
                self._queue.append((tag, step, v, None))
        self._drain()

    def flush(self):
        if self.writer is not None:
            self._drain(block=True)
            if hasattr(self.writer, "flush"):
                self.writer.flush()


def dump_architectures(logdir, gen, critic):
    if logdir is None:
        return
    with open(logdir + "/model_gen.txt", "w+") as f:
        f.write(str(gen))
    with open(logdir + "/model_critic.txt", "w+") as f:
        f.write(str(critic))


def save_state(module, path):
    torch.save(module.state_dict(), path)


def dataset_folder(cfg, override=None):
    """The dataset folder of a non-synthetic run (`--folder` or the YAML's `folder:` key); exits with the
    reference's own situation spelled out when it is absent (the data is not distributed with either repo)."""
    folder = override or cfg.get("folder")
    if not folder or not os.path.isdir(folder):
        raise SystemExit("dataset folder %r not found: pass --folder <Music-to-Dance-Motion-Synthesis-master> "
                         "(or --synthetic for random batches of the dataset's shapes)" % (folder,))
    return folder


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from _tensors(y)


def resident_batches(loader, device, derive=None):
    """Batches of a data.ResidentLoader, each gathered on the copy stream: yields (batch, event after which its tensors
    are complete) like `staged` does for host batches - the gather of batch k + 1 runs beside the kernels of loop body k,
    and `train_step(..., inputs_ready=event)` may start its generator forward as soon as the gather is done.
    `derive(batch)` (optional) runs on the copy stream too, BEFORE the event: tensors computed from the batch that the
    step's other streams read (phase 3's padded audio track) - it replaces the batch in what is yielded."""
    from .layers import copy_stream
    it = iter(loader)
    cuda = torch.device(device).type == "cuda"
    while True:
        if not cuda:
            try:
                batch = next(it)
            except StopIteration:
                return
            yield (derive(batch) if derive else batch), None
            continue
        cur = torch.cuda.current_stream(device)
        cs = copy_stream(device)
        # (no wait for `cur`: the dataset is uploaded by the first gather on this same stream and never written again,
        # and the batch lands in fresh blocks of the copy stream's own pool)
        with torch.cuda.stream(cs):
            try:
                batch = next(it)
            except StopIteration:
                return
            if derive is not None:
                batch = derive(batch)
            ready = cs.record_event()
        cur.wait_event(ready)
        for t in _tensors(batch):
            t.record_stream(cur)
        yield batch, ready


def staged(tensors, device, derive=None):
    """Host tensors of one loader batch -> device, on the copy stream; (device tensors, event after which they
    are complete): what `train_step(..., inputs_ready=)` takes. `derive(device tensors)` (optional) runs on the copy
    stream before the event and replaces them: whatever else the step's other streams read must be complete at the
    event too (phase 3's padded audio track - made on the main stream it would sit behind the previous loop body
    while the generator stream, which only waits for the event, already reads it)."""
    from .layers import copy_stream
    if torch.device(device).type != "cuda":
        out = [t.to(device) for t in tensors]
        return (derive(out) if derive else out), None
    cur = torch.cuda.current_stream(device)
    cs = copy_stream(device)
    with torch.cuda.stream(cs):
        out = [t.to(device, non_blocking=True) for t in tensors]
        if derive is not None:
            out = derive(out)
        ready = cs.record_event()
    cur.wait_event(ready)
    for t in _tensors(out):
        t.record_stream(cur)
    return out, ready


# ------------------------------------------------------------------------------------------- the training driver
def train_parser(batch_size=True, graphs=None, framework=None):
    """The flags every train script takes. Opt-in: `--batch-size`; `graphs`, the help text of `--graphs` (with it comes
    `--no-graphs`); `framework`, the help text of `-f`."""
    ap = argparse.ArgumentParser()
    ap.add_argument("-c", "--config", type=str, help="choose config file")
    ap.add_argument("-d", "--device", type=int, help="choose gpu id")
    ap.add_argument("-n", "--name", type=str, help="name experiment")
    if framework:
        ap.add_argument("-f", "--framework", type=str, default="wgangp", help=framework)
    ap.add_argument("--synthetic", action="store_true", help="random batches of the dataset's shapes")
    ap.add_argument("--folder", type=str, default=None, help="dataset folder (overrides the YAML's `folder:`)")
    ap.add_argument("--iterations", type=int, default=None, help="stop after this many loop bodies")
    if batch_size:
        ap.add_argument("--batch-size", type=int, default=None, help="override batch_size (per GPU)")
    ap.add_argument("--log-every", type=int, default=1)
    ap.add_argument("--no-run-dir", action="store_true")
    ap.add_argument("--sync-bn", action="store_true", help="data parallel: BatchNorm statistics over the global batch")
    ap.add_argument("--host-loader", action="store_true",
                    help="fetch and collate batches on the host (torch DataLoader, as the reference does) instead of "
                         "gathering them from the HBM-resident dataset; same batches either way")
    if graphs:
        ap.add_argument("--graphs", action="store_true", help=graphs)
        ap.add_argument("--no-graphs", action="store_true", help="keep the eager launch loop on a single GPU too")
    return ap


Run = collections.namedtuple("Run", "rank world device cfg opts")


def start(opts):
    rank, world, local = dp.init_from_env()
    return Run(rank, world, pick_device(local if world > 1 else opts.device), load_config(opts.config), opts)


def run_dir(run):
    return make_run_dir(run.opts.name, enabled=(run.rank == 0 and not run.opts.no_run_dir))


def sequence_shape(run):
    """(stick_length, batch_size) of a sequence phase: poses per sequence from the YAML, `--batch-size` over the YAML's."""
    ds = run.cfg["dataset"]
    return int(ds["seq_length"] * ds["video_rate"]), run.opts.batch_size or run.cfg["batch_size"]


def subset_loader(run, dataset, batch_size, collate_fn=None):
    """Full batches of a random subset of the first `num_train` items: gathered from the HBM-resident dataset on a HIP
    device, by a torch DataLoader on the host with `--host-loader` (or without a device)."""
    from torch.utils.data import DataLoader, SubsetRandomSampler
    from . import data as D
    sampler = SubsetRandomSampler(range(min(run.cfg["num_train"], len(dataset))))
    if run.device.type == "cuda" and not run.opts.host_loader:
        return D.ResidentLoader(dataset, batch_size, sampler, run.device, drop_last=True)
    return DataLoader(dataset, batch_size=batch_size, drop_last=True, sampler=sampler, collate_fn=collate_fn)


def sequence_dataset(run, withaudio):
    """MinMax-scaled pose sequences (the scaler fitted on all still poses), random crops - augmented when the YAML has
    a `dataset: augment:` block (data.Augment; phase 3's make_loaders keeps it to the train subset)."""
    from . import data as D
    folder = dataset_folder(run.cfg, run.opts.folder)
    print("Loading sticks and sequences datasets...")
    sticks = D.StickDataset(folder, normalize="minmax")
    return D.SequenceDataset(folder, run.cfg["dataset"], dance_types=run.cfg["dance_types"], scaler=sticks.scaler,
                             withaudio=withaudio, sync=run.cfg["dataset"].get("sync", False),
                             augment=run.cfg["dataset"].get("augment"))


def pose_sequence_loader(run, batch_size):
    """phase2/train.py:66-70,115-116: pose sequences without audio under a random subset sampler; also the
    dataset's stick_length."""
    from . import data as D
    dataset = sequence_dataset(run, withaudio=False)
    return subset_loader(run, dataset, batch_size, lambda b: D.collate_fn(b, withaudio=False)), dataset.stick_length


def synthetic_seeds(run, epoch):
    """Seeds of one epoch's synthetic batches, distinct per batch and rank. (The number of batches comes from the YAML's
    batch size whatever `--batch-size` says.)"""
    n = max(run.cfg["num_train"] // run.cfg["batch_size"], 1)
    return (1 + (epoch * n + b) * run.world + run.rank for b in range(n))


def graphs_on(run):
    """Captured HIP graphs by default on one GPU; data parallel the exchange stays outside the graphs, so only on request."""
    return run.device.type == "cuda" and (run.opts.graphs or (run.world == 1 and not run.opts.no_graphs))


def enable_ema(engine, cfg):
    """The YAML keys `ema_decay` (a float; absent, null or 0: off) and `ema_warmup` (default true) -> engine.enable_ema;
    -> whether the engine now keeps an averaged generator (engine.gen_ema)."""
    engine.enable_ema(cfg.get("ema_decay"), warmup=bool(cfg.get("ema_warmup", True)))
    return engine.gen_ema is not None


def with_ema(due, ema):
    """A script's due checkpoints [(module name, file name)]; with `ema`, ("gen", "<stem>_<n>.pt") is followed by
    ("gen_ema", "<stem>_ema_<n>.pt"): the averaged generator as an ordinary generator state_dict."""
    if not ema:
        return due
    out = []
    for name, file in due:
        out.append((name, file))
        if name == "gen":
            stem, n = file.rsplit("_", 1)
            out.append(("gen_ema", "%s_ema_%s" % (stem, n)))
    return out


def train(run, logdir, engine, batches, scalars, checkpoints, train_mode=("gen",), architectures=True, started=None,
          epoch_end=None):
    """The loop of a train script, from the built engine to the closing print.
    batches(epoch):       the epoch's batches, each (train_step's positional arguments, event after which they are
                          complete or None); every step is `engine.train_step(*args, inputs_ready=event)`, so an
                          engine run by this driver takes `inputs_ready` (None: nothing to wait for)
    scalars(out):         what to log of a train_step's result, tag -> value, or None on an iteration that logs nothing
    checkpoints(epoch):   [(module name, file name), ...] due after that epoch (needs a run directory)
    train_mode:           the engine's modules put into train mode at the top of every epoch
    architectures:        write model_gen.txt / model_critic.txt into the run directory
    started(log):         optional, once before the first epoch
    epoch_end(epoch, log, done): optional, after every epoch's batches - also those of the epoch in which `--iterations`
                          was reached (done), which ends the run right after: no checkpoint follows it."""
    log = ScalarLog(logdir, run.opts.log_every)
    if architectures:
        dump_architectures(logdir, engine.gen, engine.critic)
    if started is not None:
        started(log)
    modules = [getattr(engine, name) for name in train_mode]
    stop = run.opts.iterations
    settle_garbage_collector()
    print("Start training..")
    done = False
    for epoch in range(run.cfg["num_epochs"]):
        for m in modules:
            m.train()
        for args, ready in batches(epoch):
            out = engine.train_step(*args, inputs_ready=ready)
            it = engine.total_iterations
            values = scalars(out)
            if values is not None:
                log.scalars(values, it)
            if stop is not None and it >= stop:
                done = True
                break
        if epoch_end is not None:
            epoch_end(epoch, log, done)
        if done:
            break
        due = checkpoints(epoch) if logdir is not None else ()
        if any(name == "critic" for name, _ in due):
            engine.flush()  # a deferred (data-parallel) critic step must be in the checkpoint
        for name, file in due:
            save_state(getattr(engine, name), logdir + "/models/" + file)
    engine.flush()
    log.flush()
    if run.rank == 0:
        print("done: {} iterations, last {}".format(engine.total_iterations,
                                                    {k: float(v) for k, v in engine.last.items()}))
