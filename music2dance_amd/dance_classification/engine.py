"""Training step of the dance-style classifier (dance_classification/main.py:117-136): forward, mean cross-entropy,
backward and Adam, every op on the HIP kernels. Nothing synchronises with the host: losses stay on the device."""
import torch

from .. import kernels, ops, optim


class ClassifierEngine:
    def __init__(self, model, lr):
        self.model = model
        self.params = [p for p in model.parameters()]
        self.optim = optim.Adam(self.params, lr=lr)
        self.total_iterations = 0
        self.last = None

    def train_step(self, sticks, labels):
        """sticks (B, 69, T) on the device, labels (B,) int64 -> 0-dim loss (device tensor)."""
        self.model.train()
        self.total_iterations += 1
        with kernels.impl().weight_cache():
            loss = ops.cross_entropy(self.model(sticks), labels)
            self.optim.zero_grad(set_to_none=True)
            loss.backward()
            self.optim.step()
            kernels.impl().invalidate_packed(self.params)
        self.last = loss.detach()
        return self.last

    @torch.no_grad()
    def evaluate(self, sticks, labels):
        """Eval-mode forward without a graph -> (0-dim mean loss, (B,) int64 argmax of the logits)."""
        was_training = self.model.training
        self.model.eval()
        try:
            return ops.cross_entropy_pred(self.model(sticks), labels)
        finally:
            self.model.train(was_training)
