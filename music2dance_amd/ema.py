"""An exponential moving average of the generator's weights, kept inside the generator's fused Adam launch.

Every score and every generated dance used to come from the LAST iterate of a WGAN-GP generator, the noisiest
checkpoint a run produces. `GeneratorEMA` holds a twin of the generator - same class, same state_dict keys, parameters
in storage of its own - whose parameters are the shadows `optim.Adam.track_ema` hands to m2d_adam_multi_ema: the launch
that steps a parameter p also moves its shadow, e += (1 - d) * (p - e), from the register copy of the fresh p. No second
pass over the weights, no further launches.

  decay      d of the n-th update (n = 0 for the first) is min(decay, (1 + n) / (10 + n)) with warm-up, else `decay`:
             early updates follow the live weights closely instead of averaging in the random initialisation.
  parameters a parameter that never gets a gradient (the dead fc1 / bn1 of every LinearBlock) is never stepped, so its
             shadow keeps the initial copy - which is what the live value stays, too.
  buffers    BatchNorm running_mean / running_var / num_batches_tracked are not averaged (they are statistics of the
             activations, not iterates): `sync_buffers()` copies the live generator's into the twin whenever the twin is
             handed out (`module()`).
  images     the fused step does not move tensor version counters, so the twin's cached packed conv images and GRU
             transposes (kernels.weight_cache) would go stale: `stepped()` drops them after every step that wrote
             shadows.
Data parallel: every rank's parameters are equal after the gradient exchange, so its shadows are too; nothing is
exchanged. The twin is an ordinary generator: its state_dict loads wherever the live generator's does.
"""
import copy

import torch

from . import kernels


def decay_at(n, decay, warmup=True):
    """The decay of the n-th update (n = 0 for the first)"""
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def _twin(gen):
    """A deep copy of `gen` (parameters and buffers in storage of their own); side streams a module made for itself are
    not shared - the copy makes its own when it first needs one."""
    memo = {}
    if torch.cuda.is_available():
        for m in gen.modules():
            for v in vars(m).values():
                if isinstance(v, (torch.cuda.Stream, torch.cuda.Event)):
                    memo[id(v)] = None
    return copy.deepcopy(gen, memo)


class GeneratorEMA:
    def __init__(self, gen, optimizer, decay, warmup=True):
        if not hasattr(optimizer, "track_ema"):
            raise RuntimeError("GeneratorEMA needs the fused optimizer step (music2dance_amd.optim.Adam): with "
                               "M2D_ADAM=torch there is no launch to keep the average in")
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("ema decay must lie in (0, 1), got %r" % (decay,))
        self.gen, self.decay, self.warmup = gen, decay, bool(warmup)
        self.updates = 0   # issued generator steps
        self.twin = _twin(gen)
        self.twin.requires_grad_(False)
        self.twin.eval()
        live, mine = dict(gen.named_parameters()), dict(self.twin.named_parameters())
        assert list(live) == list(mine)
        self._shadows = list(mine.values())
        optimizer.track_ema((live[k], mine[k]) for k in live)

    def next_decay(self):
        """The decay of the update about to be issued"""
        return decay_at(self.updates, self.decay, self.warmup)

    def stepped(self):
        """After a generator step that wrote shadows: count it, drop the twin's cached weight images (the fused step
        leaves version counters where they were)."""
        self.updates += 1
        kernels.impl().invalidate_packed(self._shadows)

    @torch.no_grad()
    def sync_buffers(self):
        for (k, b), (k2, mine) in zip(self.gen.named_buffers(), self.twin.named_buffers()):
            assert k == k2
            mine.copy_(b)

    def module(self):
        """The averaged generator, its buffers the live generator's as of now, in eval mode"""
        self.sync_buffers()
        return self.twin
