"""The dance-style classifier of the reference (dance_classification/archis/default.py:5-26) on the HIP path.

Same constructor, attribute names, state_dict keys / shapes and construction-time RNG use as the reference, so its
checkpoints load unchanged. The front is StickDiscriminator's without the full-length conv: Conv1d + ReLU (fused in the
epilogue), TemporalBlocks (csrc/tcn.hip shapes), then a GRU whose final state is the logits: nn.GRU(128, 4) runs on the
small-state kernels (one launch per direction, ops.gru_final_state)."""
import torch.nn as nn

from ... import ops
from ...layers import GRU, Conv1d
from ...phase3.archis.default import TemporalBlock
from ...utils import initialize_weights


class RecurrentDanceClassifier(nn.Module):
    def __init__(self, channels_in, channels_h, output_code, init_ker=9, n_blocks=1):
        super().__init__()
        self.conv1 = Conv1d(channels_in, channels_h, kernel_size=init_ker, padding=int((init_ker - 1) / 2))
        self.relu = nn.ReLU(inplace=True)
        self.blocks = nn.Sequential(*[TemporalBlock(channels_h, 7) for _ in range(n_blocks)])
        self.rnn = GRU(channels_h, output_code, batch_first=True)
        initialize_weights(self)

    def forward(self, x):
        """x: (B, channels_in, T) poses -> (B, output_code) logits (the GRU's h_n)."""
        h = self.blocks(self.conv1(x, act=ops.ACT_RELU))
        return self.rnn.final_state(h.permute(0, 2, 1).contiguous())
