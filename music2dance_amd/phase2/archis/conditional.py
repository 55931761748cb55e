"""Phase-2 label-conditioned sequence GAN (phase2/archis/conditional.py of the reference) on HIP kernels.

Both networks embed the requested style with `embed_label = nn.Embedding(4, 4)`: the generator's GRU reads
[noise | E[label]] (input_size + 4 features per frame, ops.label_concat batch-first), the critic's conv1 reads
[poses | E[label]] channels-first (69 + 4 channels, the label channels last and constant over time). Dropout(0.5) sits
before the decoder's lastfc and before the critic's lastconv (layers.Dropout on m2d_dropout). LinearBlock, TemporalBlock
and NoiseGen are the unconditional archis' classes. Constructor RNG order (the embedding's normal init first, then the
GRU, then the rest, then initialize_weights), state_dict keys and shapes are the reference's.
"""
import torch.nn as nn

from ... import ops
from ...layers import BatchNorm1d, Conv1d, Dropout, Linear, batched_bn_counters
from ...scoring import N_STYLES as N_CLASSES
from ...utils import initialize_weights
from .default import LinearBlock, NoiseGen, TemporalBlock


def _dropout(p):
    d = Dropout(p)
    d.hip = True
    return d


class FrameDecoder(nn.Module):
    """Per-frame residual MLP with Dropout(0.5) before lastfc (conditional.py:98-117)."""

    def __init__(self, latent_size, size, output_size, nblocks):
        super().__init__()
        self.latent_size, self.size, self.output_size, self.nblocks = latent_size, size, output_size, nblocks
        self.fc1 = Linear(latent_size, size)
        self.bn1 = BatchNorm1d(size, eps=1e-5, momentum=0.1)
        self.relu = nn.ReLU(inplace=True)
        self.blocks = nn.Sequential(*[LinearBlock(size, use_bn=True) for _ in range(nblocks)])
        self.dropout = _dropout(0.5)
        self.lastfc = Linear(size, output_size)

    def forward(self, x):
        h = self.bn1(self.fc1(x), act=ops.ACT_RELU)
        return self.lastfc(self.dropout(self.blocks(h)))


class SequenceGenerator(nn.Module):
    def __init__(self, input_size, latent_size, size, output_size, n_blocks, n_cells=1, device="cpu"):
        super().__init__()
        self.input_size, self.latent_size, self.size, self.output_size = input_size, latent_size, size, output_size
        self.embed_label = nn.Embedding(N_CLASSES, 4)
        self.noise_gen = NoiseGen(input_size + 4, latent_size, n_cells)
        self.decoder = FrameDecoder(latent_size, size, output_size, n_blocks)
        initialize_weights(self)
        self.to(device)

    def forward(self, x, labels):
        """x (B, T, input_size) noise, labels (B,) styles in [0, 4) -> (B*T, output_size) pose rows"""
        with batched_bn_counters(self):
            h = self.noise_gen(ops.label_concat(x, self.embed_label.weight, labels, 0))
            return self.decoder(h.reshape(-1, self.decoder.latent_size))


class SequenceDiscriminator(nn.Module):
    """TCN critic on [poses | E[label]]: conv(k=init_ker) + ReLU, n_blocks TemporalBlocks, Dropout(0.5), full-length
    conv -> score."""

    def __init__(self, channels_in, channels_h, seqlen, init_ker=7, n_blocks=1, device="cpu"):
        super().__init__()
        self.embed_label = nn.Embedding(N_CLASSES, 4)
        self.conv1 = Conv1d(channels_in + 4, channels_h, kernel_size=init_ker, padding=int((init_ker - 1) / 2))
        self.blocks = nn.Sequential(*[TemporalBlock(channels_h, 7) for _ in range(n_blocks)])
        self.lastconv = Conv1d(channels_h, 1, seqlen)
        self.dropout = _dropout(0.5)
        self.relu = nn.ReLU(inplace=True)
        initialize_weights(self)
        self.to(device)

    def forward(self, x, labels):
        """x (B, 69, T) poses, labels (B,) -> (B,) scores"""
        h = self.blocks(self.conv1(ops.label_concat(x, self.embed_label.weight, labels, 1), act=ops.ACT_RELU))
        return self.lastconv(self.dropout(h)).squeeze(1)
