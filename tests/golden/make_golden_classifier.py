"""Fixture generator for the dance-style classifier — runs ONLY where the reference exists.

Imports the reference's RecurrentDanceClassifier (dance_classification/archis/default.py) with `librosa` stubbed, as
make_golden.py does, and stores its OUTPUTS only (never its source) in cls.npz. Inputs are regenerated from the seeds of
patterns.py on every side. Large tensors (conv weights and their gradients) are stored as their float64 checksums,
their largest magnitude and SAMPLE elements at seeded flat indices; small ones in full.

    python tests/golden/make_golden_classifier.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import patterns as P  # noqa: E402

REF = "/root/reference"
B, T, C = 49, 120, 4
CTOR_SEED, FILL_SEED, X_SEED, Y_SEED, TRACE_SEED = 123, 7000, 71, 72, 80
LR, TRACE_STEPS = 2e-4, 8
SAMPLES = 512


def import_reference():
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    return importlib.import_module("dance_classification.archis.default")


def inputs(seed_x=X_SEED, seed_y=Y_SEED):
    """(B, 69, T) poses and (B,) int64 styles of one case"""
    x = P.poses(B, T, seed=seed_x).permute(0, 2, 1).contiguous()
    y = torch.randint(0, C, (B,), generator=P._gen(seed_y))
    return x, y


def sample_index(numel, key):
    """seeded flat indices of the stored sample of a tensor with `numel` elements"""
    g = P._gen(10_000 + sum(map(ord, key)))
    return torch.randperm(numel, generator=g)[:min(SAMPLES, numel)].sort().values


def pack(prefix, named, out):
    for k, v in named.items():
        v = v.detach().double()
        out[prefix + k + ":checksum"] = np.array(P.checksum(v))
        out[prefix + k + ":absmax"] = np.array(v.abs().max().item())
        if v.numel() <= 4096:
            out[prefix + k + ":full"] = v.numpy()
        else:
            idx = sample_index(v.numel(), k)
            out[prefix + k + ":sample"] = v.reshape(-1)[idx].numpy()


def main():
    ref = import_reference()
    out = {}
    torch.manual_seed(CTOR_SEED)
    m = ref.RecurrentDanceClassifier(69, 128, C)
    sd = m.state_dict()
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
    pack("init/", sd, out)

    m.load_state_dict(P.fill_state_dict(sd, FILL_SEED))
    x, y = inputs()
    logits = m(x)
    loss = torch.nn.CrossEntropyLoss(reduction="mean")(logits, y)
    loss.backward()
    out["logits"] = logits.detach().double().numpy()
    out["loss"] = np.array(loss.item())
    pack("grad/", {k: p.grad for k, p in m.named_parameters()}, out)

    m.load_state_dict(P.fill_state_dict(sd, FILL_SEED))
    opt = torch.optim.Adam(m.parameters(), lr=LR)
    trace = []
    for s in range(TRACE_STEPS):
        xs, ys = inputs(TRACE_SEED + 2 * s, TRACE_SEED + 2 * s + 1)
        loss = torch.nn.CrossEntropyLoss(reduction="mean")(m(xs), ys)
        opt.zero_grad()
        loss.backward()
        opt.step()
        trace.append(loss.item())
    out["trace"] = np.array(trace)
    path = os.path.join(HERE, "cls.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d KB)" % (path, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()
