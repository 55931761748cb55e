"""Shared cases of the generator EMA tests (tests/test_ema_host.py, tests/test_gpu_ema.py).

The fp64 statement of the average is `e64 += (1 - d) * (p.double() - e64)`, fed with the KERNEL'S OWN fp32 parameters read
back after each step, so Adam's rounding is not charged to the EMA.

The bound after n updates is n * 8 * 2**-24 * max|e|. Per update the fp32 path rounds `omd = 1 - d`, the difference
`p - e`, the product `omd * (p - e)` and the sum, each against operands no larger than 2 * max: four roundings of half
an ulp of 2 * max each = 4 * 2**-24 * max, doubled for margin. A numpy fp32 simulation over d in {0.1, 0.5, 0.9, 0.999,
0.9999} stayed below 1 * 2**-24 * max|e| per update. max|e| is each tensor's own, of its fp64 average as it stands.
"""
import torch

# tests/test_optim.py's shapes, plus a conv weight of few output channels, one whose tile rows end inside a tile, a flat
# tensor one chunk and a ragged tail long, and one shorter than a vector
OPTIM_SHAPES = [(128, 69, 25), (128,), (128, 128, 7), (128,), (100, 12800), (1, 128), (3,), (5000, 33), (64, 32, 4)]
SHAPES = OPTIM_SHAPES + [(20, 16, 3), (100, 36, 7), (4099,), (7,)]
DECAYS = (0.1, 0.5, 0.999)
EMA_BATCH = 40   # tensors per m2d_adam_multi_ema launch (csrc/pointwise.hip: M2D_ADAM_EMA_BATCH)
ULP = 2.0 ** -24


class Ema64:
    """The fp64 average of a list of tensors, fed with the fp32 parameters read back after each step."""

    def __init__(self, shadows):
        self.e = [s.detach().cpu().double().clone() for s in shadows]
        self.n = [0] * len(self.e)

    def update(self, params, decay, which=None):
        for i, p in enumerate(params):
            if which is not None and i not in which:
                continue
            p64 = p.detach().cpu().double()
            self.e[i] += (1.0 - decay) * (p64 - self.e[i])
            self.n[i] += 1

    def bound(self, i):
        return self.n[i] * 8 * ULP * float(self.e[i].abs().max())

    def check(self, shadows, what=""):
        for i, s in enumerate(shadows):
            if s is None:
                continue
            err = float((s.detach().cpu().double() - self.e[i]).abs().max()) if s.numel() else 0.0
            print("%s tensor %d %s: updates %d, err %.3e, bound %.3e" % (what, i, tuple(s.shape), self.n[i], err, self.bound(i)))
            assert err <= self.bound(i), (what, i, tuple(s.shape), err, self.bound(i))


def tensors(shapes, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def grads(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * 10.0 ** (i % 3 - 1) for i, s in enumerate(shapes)]
