"""Streaming generation (phase3/generate.py) on the device: DanceStream with pushes of 1 frame, 7 frames, 1 000 samples
(not a multiple of the hop) and the whole track against generate_track; generate_track against the CPU oracle's
eval-mode generator with the same noise; a --synthetic CLI run writes arrays and JSON of the expected shapes."""
import json
import os

import numpy as np
import pytest
import torch

import oracle.m2d_oracle as O
from tests.golden import patterns as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
WINDOW, HOP, PAD, NOISE = 3200, 640, 2560, 10
T = 600


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


@pytest.fixture(scope="module", params=["default", "wavegan"])
def gen(request):
    from music2dance_amd.phase3.archis.default import SequenceGenerator
    torch.manual_seed(0)
    g = SequenceGenerator(WINDOW, 250, 250, 256, 69, NOISE, 2, 3, request.param, "id", "cpu")
    g.load_state_dict(P.fill_state_dict(g.state_dict(), 4321))
    g.enc_type = request.param
    return g.to(DEV).eval()


@pytest.fixture(scope="module")
def track():
    g = torch.Generator().manual_seed(77)
    return (0.1 * torch.randn(T * HOP, generator=g)).to(DEV)


@pytest.fixture(scope="module")
def one_shot(gen, track):
    from music2dance_amd.phase3 import generate as G
    out = G.generate_track(gen, track, seed=5)
    torch.cuda.synchronize()
    return out


def stream(gen, track, step):
    from music2dance_amd.phase3 import generate as G
    s = G.DanceStream(gen, WINDOW, HOP, PAD, seed=5)
    parts = [s.push(track[i:i + step].unsqueeze(0)) for i in range(0, track.shape[0], step)] + [s.flush()]
    assert all(p.shape[0] == 1 and p.shape[2] == 69 for p in parts)
    return torch.cat(parts, 1)[0]


@pytest.mark.parametrize("step", [HOP, 7 * HOP, 1000, T * HOP], ids=["1frame", "7frames", "1000samples", "whole"])
def test_stream_matches_one_shot(gen, track, one_shot, step):
    assert one_shot.shape == (T, 69)
    got = stream(gen, track, step)
    assert got.shape == one_shot.shape
    d = float((got - one_shot).abs().max())
    note("dance_stream |d| vs one-shot (%s)" % gen.enc_type, d)
    # launch plans that differ by row count may sum in another order: the mismatch is fp32 rounding only
    assert d < 1e-4, d


def test_stream_is_seeded_by_frame(gen, track, one_shot):
    from music2dance_amd.phase3 import generate as G
    other = G.generate_track(gen, track, seed=6)
    assert float((other - one_shot).abs().max()) > 1e-3   # the noise reaches the poses
    again = G.generate_track(gen, track, seed=5)
    assert torch.equal(again, one_shot)


def test_one_shot_matches_the_oracle(gen, track, one_shot):
    from music2dance_amd.phase3 import generate as G
    from music2dance_amd.utils import slice_audio_batch
    noise = G.frame_noise(5, 0, 1, T, NOISE, DEV).cpu().double()
    sd = {k: v.detach().cpu().double() if torch.is_floating_point(v) else v.cpu() for k, v in gen.state_dict().items()}
    slices = slice_audio_batch(track.cpu().double().unsqueeze(0), WINDOW, HOP, PAD)
    with torch.no_grad():
        ref = O.p3_generator(sd, slices, noise, gen.enc_type, "id", 3, 2, False)
    d = float((one_shot.cpu().double() - ref).abs().max())
    note("dance_stream |d| vs oracle (%s)" % gen.enc_type, d)
    assert d < 1e-4, d


def test_cli_synthetic_writes_poses_and_timings(tmp_path):
    from music2dance_amd.phase3 import generate as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = os.path.join(root, "music2dance_amd", "phase3", "configs", "default.yaml")
    res = G.main(["-c", cfg, "-l", str(tmp_path), "--synthetic", "--chunk-frames", "25", "--seed", "3"])
    arr = np.load(os.path.join(str(tmp_path), "samples", "synthetic.npy"))
    assert arr.shape == (600, 23, 3) and arr.dtype == np.float32 and np.isfinite(arr).all()
    with open(os.path.join(str(tmp_path), "samples", "generation.json")) as f:
        js = json.load(f)
    assert js == json.loads(json.dumps(res))
    (tr,) = js["tracks"]
    assert tr["frames"] == 600 and tr["seconds"] == pytest.approx(24.0) and tr["chunk_frames"] == 25
    assert tr["chunks"] == 25 and tr["wall_s"] > 0 and tr["real_time_factor"] > 0
    assert 0 < tr["gpu_ms_per_chunk_p50"] <= tr["gpu_ms_per_chunk_p99"]
    # one-shot run of the same seed: the same dance
    G.main(["-c", cfg, "-l", str(tmp_path), "--synthetic", "--chunk-frames", "0", "--seed", "3"])
    again = np.load(os.path.join(str(tmp_path), "samples", "synthetic.npy"))
    assert np.abs(again - arr).max() < 1e-3
