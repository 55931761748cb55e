"""Host side of the streaming generator (phase3/generate.py), no GPU needed:
  * DanceStream's frame arithmetic equals utils.slice_audio_batch exactly, for random track lengths, windows, hops,
    pads and push splits (a stand-in generator hands the windows it is given back as its rows);
  * the decomposition itself: a chunked fp64 generator built from the oracle's functions and torch.nn.GRU(hx),
    its GRU states carried from chunk to chunk, equals oracle.p3_generator over the whole track in eval mode;
  * the errors of the command line and the carried-state plumbing."""
import argparse
import os

import pytest
import torch

import oracle.m2d_oracle as O
from tests.golden import patterns as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class WindowEcho:
    """stands in for an eval-mode SequenceGenerator: rows = the audio windows of the chunk, state = frames seen"""
    training = False
    noise_size = 2

    def __init__(self, window):
        self.window_size = self.output_size = window
        self.calls = []

    def parameters(self):
        return iter([torch.zeros(1)])

    def step(self, x, state=None, noise=None):
        B, k, W = x.shape
        seen = 0 if state is None else state
        assert noise.shape == (B, k, self.noise_size)
        assert torch.equal(noise[..., 0], torch.arange(seen, seen + k, dtype=torch.float32).expand(B, k))
        self.calls.append(k)
        return x.reshape(B * k, W).clone(), seen + k


def frame_index_noise(frame0, B, n):
    return torch.arange(frame0, frame0 + n, dtype=torch.float32).view(1, n, 1).expand(B, n, 2).contiguous()


def test_frame_arithmetic_matches_slice_audio_batch():
    from music2dance_amd.phase3 import generate as G
    from music2dance_amd.utils import slice_audio_batch
    g = torch.Generator().manual_seed(0)
    for trial in range(300):
        hop = int(torch.randint(1, 40, (1,), generator=g))
        window = hop + int(torch.randint(0, 90, (1,), generator=g))
        pad = int(torch.randint(0, 2 * window, (1,), generator=g)) if trial % 3 else window - hop
        S = int(torch.randint(0, 700, (1,), generator=g))
        B = 1 + trial % 3
        audio = torch.randn(B, S, generator=g)
        want_T = G.n_frames(S, window, hop, pad)
        gen = WindowEcho(window)
        s = G.DanceStream(gen, window, hop, pad, seed=0, batch=B, noise_fn=frame_index_noise)
        parts, i = [], 0
        while i < S:
            n = int(torch.randint(0, 3 * hop + window, (1,), generator=g))
            parts.append(s.push(audio[:, i:i + n]))
            i += n
        parts.append(s.flush())
        got = torch.cat(parts, 1)
        if S + pad >= window:
            want = slice_audio_batch(audio, window, hop, pad)
            assert want.shape[1] == want_T == (S + pad - window) // hop + 1
            assert torch.equal(got, want), (trial, S, window, hop, pad)
        else:
            assert got.shape[1] == want_T == 0
        assert sum(gen.calls) == want_T and s.frames == want_T
        assert s.carry.shape[1] < window  # never more than the next frame's partial window is kept


def test_frames_are_emitted_as_soon_as_their_window_is_complete():
    from music2dance_amd.phase3 import generate as G
    window, hop, pad = 3200, 640, 2560
    left = pad // 2
    s = G.DanceStream(WindowEcho(window), window, hop, pad, seed=0, noise_fn=frame_index_noise)
    received = 0
    for n in (1919, 1, 639, 1, 5000, 64000):
        k = s.push(torch.zeros(1, n)).shape[1]
        before = s.frames - k
        received += n
        # frame t is ready when t hop - left + window <= received
        ready = [t for t in range(0, 1000) if t * hop - left + window <= received]
        assert s.frames == len(ready), (received, s.frames)
        assert before <= s.frames
    assert s.frames == (received - (window - left)) // hop + 1
    with pytest.raises(RuntimeError):
        s.flush(), s.push(torch.zeros(1, 3))


def _gru_from_sd(sd, prefix, n_layers):
    w = sd[prefix + "weight_ih_l0"]
    rnn = torch.nn.GRU(w.shape[1], sd[prefix + "weight_hh_l0"].shape[1], n_layers, batch_first=True).double()
    rnn.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
    return rnn


@pytest.mark.parametrize("enc", ["default", "wavegan"])
def test_chunked_generator_equals_the_one_shot_oracle(enc):
    """the decomposition DanceStream relies on: eval-mode rows are independent, the GRUs only need their state"""
    from music2dance_amd.phase3.archis.default import SequenceGenerator
    from music2dance_amd.utils import slice_audio_batch
    torch.manual_seed(0)
    gen = SequenceGenerator(3200, 250, 250, 256, 69, 10, 2, 3, enc, "id", "cpu")
    sd = {k: (v.double() if torch.is_floating_point(v) else v)
          for k, v in P.fill_state_dict(gen.state_dict(), 99).items()}
    g = torch.Generator().manual_seed(1)
    B, T = 2, 37
    audio = 0.1 * torch.randn(B, T * 640, generator=g, dtype=torch.float64)
    slices = slice_audio_batch(audio, 3200, 640, 2560)
    noise = torch.randn(B, T, 10, generator=g, dtype=torch.float64)
    with torch.no_grad():
        want = O.p3_generator(dict(sd), slices, noise, enc, "id", 3, 2, False).view(B, T, 69)
        audio_rnn, noise_rnn = _gru_from_sd(sd, "audio_rnn.rnn.", 3), _gru_from_sd(sd, "noise_gen.rnn.", 1)
        encoder = {"default": O.p3_default_encoder, "wavegan": O.p3_wavegan_encoder}[enc]
        ha, hn = torch.zeros(3, B, 240, dtype=torch.float64), torch.zeros(1, B, 10, dtype=torch.float64)
        parts, t = [], 0
        for k in (1, 7, 2, 20, 7):
            x = slices[:, t:t + k].reshape(-1, 1, 3200)
            code = encoder(sd, "audio_enc.model.", x, "id", False).reshape(B, k, -1)
            h, ha = audio_rnn(code, ha)
            n, hn = noise_rnn(noise[:, t:t + k], hn)
            lat = torch.cat((h, n), -1).reshape(B * k, -1)
            parts.append(O.frame_decoder(sd, "decoder.", lat, 2, False).view(B, k, 69))
            t += k
        assert t == T
        got = torch.cat(parts, 1)
    assert float((got - want).abs().max()) < 1e-10


def _opts(tmp_path, **kw):
    base = dict(config=os.path.join(ROOT, "music2dance_amd", "phase3", "configs", "default.yaml"),
                logdir=str(tmp_path), gen_weights=None, audio=None, val=False, synthetic=False, chunk_frames=25,
                seed=0, folder=None, device=None)
    base.update(kw)
    return argparse.Namespace(**base)


def test_cli_errors(tmp_path):
    from music2dance_amd import runner
    from music2dance_amd.phase3 import generate as G
    cfg = runner.load_config(_opts(tmp_path).config)
    # no checkpoint in <logdir>/models and none given
    with pytest.raises(SystemExit, match="no generator checkpoint"):
        G.generate(_opts(tmp_path, audio=["a.wav"]), cfg, torch.device("cpu"))
    with pytest.raises(SystemExit, match="not found"):
        G.generate(_opts(tmp_path, val=True, gen_weights=str(tmp_path / "missing.pt")), cfg, torch.device("cpu"))
    # exactly one input source
    with pytest.raises(SystemExit):
        G.parse_args(["-c", "x.yaml", "-l", str(tmp_path)])
    with pytest.raises(SystemExit):
        G.parse_args(["-c", "x.yaml", "-l", str(tmp_path), "--val", "--synthetic"])
    assert G.parse_args(["-c", "x.yaml", "-l", "d", "--audio", "a.wav", "b.wav"]).audio == ["a.wav", "b.wav"]


def test_train_mode_generator_is_refused():
    from music2dance_amd.phase3 import generate as G
    from music2dance_amd.phase3.archis.default import SequenceGenerator
    torch.manual_seed(0)
    gen = SequenceGenerator(3200, 250, 250, 256, 69, 10, 2, 3, "default", "id", "cpu")
    gen.train()
    with pytest.raises(RuntimeError, match="eval mode"):
        gen.step(torch.zeros(1, 2, 3200))
    with pytest.raises(RuntimeError, match="eval"):
        G.DanceStream(gen, 3200, 640, 2560, seed=0)
    with pytest.raises(ValueError):
        G.DanceStream(gen.eval(), 3000, 640, 2560, seed=0)   # not the generator's window


def test_carried_state_refuses_gradients():
    from music2dance_amd import layers, ops
    x = torch.zeros(2, 5, 4)
    params = [torch.zeros(24, 4), torch.zeros(24, 8), torch.zeros(24), torch.zeros(24)]
    hx = torch.zeros(1, 2, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="initial state"):
        ops.gru_stack(x, params, hx=hx)
    with pytest.raises(RuntimeError, match="no_grad"):
        ops.gru_stack(x, [p.requires_grad_() for p in params], hx=hx.detach())
    deep = layers.GRU(4, 8, 5, batch_first=True)
    with pytest.raises(NotImplementedError):
        with torch.no_grad():
            deep(x, None, torch.zeros(5, 2, 8))
