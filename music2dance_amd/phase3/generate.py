"""Generate a dance for whole music tracks with a trained phase-3 generator, streamed chunk by chunk.

    python -m music2dance_amd.phase3.generate -c music2dance_amd/phase3/configs/default.yaml -l <logdir> \
        [--gen-weights PATH] (--audio a.wav [b.wav ...] | --val | --synthetic) [--chunk-frames N] [--seed S] \
        [--folder DIR] [-d N] [--video [--encoder {pil,hip}]] [--resampler {fft,poly}] [--beat-align]

The reference generates a 30-second sample in phase3/test.py:64-72 (with a broken call) and says its generator
handles tracks of any length. Frame t of a track reads the audio window track[t hop - left, t hop - left + window)
(left = pad // 2, pad = window - hop: utils.slice_audio_batch), i.e. it needs window - left samples (120 ms by
default) past its start time t hop. After the encoder come a forward-only GRU stack and a per-frame decoder, and an
eval-mode generator keeps its rows independent (BatchNorm uses the running statistics). So a track can be generated
WHILE IT ARRIVES: `DanceStream` keeps the samples the next frame still needs and the GRU states
(SequenceGenerator.step), and a chunked run gives the frames of one whole-track call (`generate_track`). The noise is
drawn on the device per absolute frame index (m2d_randn_frames): a seed gives the same dance whatever the chunking.

Outputs: <logdir>/samples/<name>.npy, the inverse-MinMax-scaled poses (T, 23, 3) of each track (what the reference's
visualize.frame_to_vid takes), and <logdir>/samples/generation.json (strict JSON): per track the frame count, the
seconds of audio, the chunk size, the wall time, the GPU time per chunk (p50 / p99) and the real-time factor
(seconds of audio per second of wall time). With --video each saved array is also rendered to
<logdir>/samples/<name>.avi (visualize.frame_to_vid at the config's video_rate), and its track entry gains `video`,
`render_ms` (device time of the render launches) and `video_s` (wall time of the whole write). --encoder chooses the
JPEG encoder of that video (pil: on the host, the default; hip: m2d_jpeg_encode on the device); when it is given the
track entry also records `encoder`.

--resampler: how an --audio file that is not at the config's audio_rate gets there. `fft` (the default) converts the
whole file on the host with scipy.signal.resample before anything is generated, as SequenceDataset.resample_audio does.
`poly` uploads the file at its own rate and converts it on the device with the polyphase filter of audio.py
(m2d_resample_poly): in one call for --chunk-frames 0, else chunk by chunk - pushes of chunk_frames * hop * rate_in /
rate_out source samples go through an audio.StreamResampler into the DanceStream, so the track is never needed whole.
generation.json records `resampler` and, per track that comes from an --audio file, `source_rate`.

--beat-align: each track entry gains `beat_align`, `beat_cover`, `beat_motion_events` and `beat_music_events`, the beat
alignment (metrics.beat_scores) of the saved poses with the track at the model's rate - with
--resampler poly the device's own conversion of the file (the streamed pieces, concatenated, equal it bit for bit).
Tracks longer than the alignment kernel's row limit fail loudly.

The common flags, the checkpoint loading and the --val lookup are scoring.py's.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from .. import audio as A
from .. import kernels, runner, scoring
from ..scoring import STICK_CHANNELS, json_safe
from ..utils import slice_audio_batch
from .archis.default import build_generator

DEFAULT_HOP = 640  # 16 kHz audio, 25 fps video


def n_frames(S, window, hop, pad):
    """frames utils.slice_audio_batch cuts from S samples: (S + pad - window) // hop + 1 (0 when too short)"""
    return max(0, (S + pad - window) // hop + 1) if S + pad >= window else 0


def frame_noise(seed, frame0, B, n, C, device):
    """(B, n, C) standard normals of frames [frame0, frame0 + n): a pure function of (seed, row, frame, channel)"""
    return kernels.impl().randn_frames(seed, frame0, B, n, C, device)


class DanceStream:
    """Streaming generation of B tracks at once: push(samples) -> the poses of every frame whose audio window is
    complete; flush() at the end of the tracks -> the rest. Frame t is ready when t hop - left + window <= received.

    The stream keeps the padded track from the next frame's first sample on (at most window - 1 samples, the last
    window - hop after an aligned push) as the carry; the first encoder conv reads the ready windows in place from
    [carry | new samples] (a WindowView), no dense window tensor is built. The GRU states of the generator are carried
    from chunk to chunk and the noise of frame t is m2d_randn_frames(seed, frame t), so the frames equal those of
    generate_track over the whole track.

    noise_fn(frame0, B, n) -> (B, n, noise_size) replaces the device noise (a test hook)."""

    def __init__(self, gen, window, hop, pad, seed, batch=1, noise_fn=None):
        window, hop, pad, batch = int(window), int(hop), int(pad), int(batch)
        if not 0 < hop <= window or pad < 0 or batch <= 0:
            raise ValueError("DanceStream: need 0 < hop <= window, pad >= 0 and batch > 0")
        if getattr(gen, "window_size", window) != window:
            raise ValueError("DanceStream: window %d, the generator's is %d" % (window, gen.window_size))
        if getattr(gen, "training", False):
            raise RuntimeError("DanceStream needs an eval-mode generator (gen.eval())")
        self.gen, self.window, self.hop, self.pad, self.seed, self.batch = gen, window, hop, pad, int(seed), batch
        self.left = pad // 2
        try:
            self.device = next(gen.parameters()).device
        except (AttributeError, StopIteration):
            self.device = torch.device("cpu")
        self.noise_fn = noise_fn
        self.carry = torch.zeros((batch, self.left), dtype=torch.float32, device=self.device)  # the left pad
        self.received = 0     # samples of the tracks pushed so far
        self.frames = 0       # frames emitted so far (= index of the next frame)
        self.state = None
        self.closed = False

    def _noise(self, n):
        if self.noise_fn is not None:
            return self.noise_fn(self.frames, self.batch, n)
        return frame_noise(self.seed, self.frames, self.batch, n, self.gen.noise_size, self.device)

    def _consume(self, new):
        buf = torch.cat((self.carry, new), 1) if new.shape[1] else self.carry
        avail = buf.shape[1]
        k = (avail - self.window) // self.hop + 1 if avail >= self.window else 0
        if k == 0:
            self.carry = buf
            return None
        windows = buf.unfold(1, self.window, self.hop)[:, :k]   # (B, k, window) view of [carry | new]
        rows, self.state = self.gen.step(windows, self.state, self._noise(k))
        self.frames += k
        self.carry = buf[:, k * self.hop:]
        return rows.reshape(self.batch, k, -1)

    def _empty(self):
        width = getattr(self.gen, "output_size", self.window)
        return torch.zeros((self.batch, 0, width), dtype=torch.float32, device=self.device)

    def push(self, samples):
        """samples (B, n) (or (n,) for one track) -> poses (B, k, output_size) of the frames now complete (k >= 0)"""
        if self.closed:
            raise RuntimeError("DanceStream: push after flush")
        x = torch.as_tensor(samples)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2 or x.shape[0] != self.batch:
            raise ValueError("DanceStream.push: (%d, n) samples expected, got %s" % (self.batch, tuple(x.shape)))
        x = x.to(device=self.device, dtype=torch.float32)
        self.received += x.shape[1]
        out = self._consume(x)
        return self._empty() if out is None else out

    def flush(self):
        """end of the tracks: the right pad (pad - left zeros) completes the last windows -> their poses"""
        if self.closed:
            raise RuntimeError("DanceStream: flushed twice")
        self.closed = True
        out = self._consume(torch.zeros((self.batch, self.pad - self.left), dtype=torch.float32, device=self.device))
        return self._empty() if out is None else out


@torch.no_grad()
def generate_track(gen, audio, seed, hop=DEFAULT_HOP, pad=None):
    """One call over whole tracks: audio (B, S) (or (S,)) -> poses (B, T, output_size) (or (T, output_size)), T the
    frame count of slice_audio_batch, with the noise DanceStream(..., seed) draws."""
    window = gen.window_size
    pad = window - hop if pad is None else int(pad)
    one = audio.dim() == 1
    a = (audio.unsqueeze(0) if one else audio).to(device=next(gen.parameters()).device, dtype=torch.float32)
    B = a.shape[0]
    slices = slice_audio_batch(a.contiguous(), window, hop, pad, lazy=True)
    T = slices.shape[1]
    if T == 0:
        raise ValueError("generate_track: a track of %d samples holds no frame" % a.shape[1])
    rows, _ = gen.step(slices, None, frame_noise(seed, 0, B, T, gen.noise_size, a.device))
    out = rows.reshape(B, T, -1)
    return out[0] if one else out


# --------------------------------------------------------------------------------------- command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--audio", type=str, nargs="+", help="wav files to dance to")
    src.add_argument("--val", action="store_true", help="the takes listed under val_samples in "
                                                        "<logdir>/trainvaltest_samples.json")
    scoring.add_common_flags(ap, 3, "gpgen", "a random 600-frame track (random weights without a checkpoint)", src)
    ap.add_argument("--chunk-frames", type=int, default=25, help="frames of audio per push (0: one call per track)")
    ap.add_argument("--seed", type=int, default=0, help="noise seed")
    ap.add_argument("--video", action="store_true", help="also render each saved dance to <logdir>/samples/<name>.avi "
                                                         "(300 x 300 stick figures at the config's video_rate)")
    ap.add_argument("--encoder", choices=("pil", "hip"), default=None,
                    help="with --video: the JPEG encoder, pil = on the host (the default), hip = on the device")
    ap.add_argument("--resampler", choices=("fft", "poly"), default="fft",
                    help="rate conversion of --audio files: fft = scipy.signal.resample of the whole file on the host, "
                         "poly = the polyphase filter on the device, streamed with the chunks")
    ap.add_argument("--beat-align", action="store_true", help="score each dance's beat alignment with its track "
                                                              "(beat_* keys of generation.json)")
    return ap.parse_args(argv)


def load_native(path):
    """(mono float32 samples of a wav file at its own rate, that rate)"""
    from scipy.io import wavfile
    from ..data import _read_wav
    sr = int(wavfile.read(path, mmap=True)[0])
    return np.asarray(_read_wav(path), dtype=np.float32), sr


def load_track(path, rate):
    """mono float32 samples of a wav file at `rate` Hz (resampled as SequenceDataset.resample_audio does)"""
    from scipy.io import wavfile
    from ..data import _read_wav
    sr = wavfile.read(path, mmap=True)[0]
    x = _read_wav(path)
    if sr != rate:
        from scipy.signal import resample
        x = resample(x, int(len(x) * (rate / sr)))
    return np.asarray(x, dtype=np.float32)


def _tracks(opts, cfg):
    """-> ([(name, samples, rate of the samples, rate of the wav file they come from or None)], scaler)"""
    from .. import data as D
    ds = cfg["dataset"]
    if opts.synthetic:
        g = torch.Generator().manual_seed(12345)
        scaler = D.MinMaxScaler().fit(torch.rand(1000, STICK_CHANNELS, generator=g).numpy())
        T = 600
        audio = 0.1 * torch.randn(T * int(ds["audio_rate"] // ds["video_rate"]), generator=g)
        return [("synthetic", audio.numpy(), ds["audio_rate"], None)], scaler
    if opts.audio:
        from scipy.io import wavfile
        scaler = D.StickDataset(runner.dataset_folder(cfg, opts.folder), normalize="minmax").scaler
        poly = getattr(opts, "resampler", "fft") == "poly"
        out = []
        for p in opts.audio:
            name = os.path.splitext(os.path.basename(p))[0]
            if poly:
                samples, sr = load_native(p)
                out.append((name, samples, sr, sr))
            else:
                out.append((name, load_track(p, ds["audio_rate"]), ds["audio_rate"],
                            int(wavfile.read(p, mmap=True)[0])))
        return out, scaler
    val_dirs, idx, dataset, scaler = scoring.validation_takes(opts, cfg)
    return [(os.path.basename(os.path.normpath(d)), np.asarray(dataset.musics[i], dtype=np.float32),
             ds["audio_rate"], None) for d, i in zip(val_dirs, idx)], scaler


def _pctl(v, q):
    return float(np.percentile(np.asarray(v, dtype=np.float64), q)) if len(v) else float("nan")


def run_track(gen, audio, seed, window, hop, pad, chunk_frames, rates=None, track_out=None):
    """-> (poses (T, output_size) on the device, timing dict). chunk_frames 0: generate_track; else DanceStream pushes
    of chunk_frames * hop samples (the track already in device memory), then flush(). rates = (rate_in, rate_out):
    `audio` is at rate_in and is converted on the device (audio.resample for one call; else every push goes through
    an audio.StreamResampler, in pieces of chunk_frames * hop * rate_in / rate_out source samples, rounded up).
    track_out: a list that receives the track at rate_out as the generator saw it, (S,) on the device (the converted
    pieces of a streamed run, concatenated)."""
    dev = next(gen.parameters()).device
    audio = audio.to(dev)
    convert = rates is not None and int(rates[0]) != int(rates[1])
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    events = []
    if chunk_frames <= 0:
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        if convert:
            audio = A.resample(audio, rates[0], rates[1])[0]
        if track_out is not None:
            track_out.append(audio)
        out = generate_track(gen, audio, seed, hop, pad)
        e[1].record()
        events.append(e)
    else:
        stream = DanceStream(gen, window, hop, pad, seed)
        parts = []
        step = chunk_frames * hop
        if convert:
            rs = A.StreamResampler(rates[0], rates[1], 1, dev)
            step = -(-step * int(rates[0]) // int(rates[1]))
            converted = []

            def keep(y):
                if track_out is not None:
                    converted.append(y[0])
                return y

            feed = lambda p: stream.push(keep(rs.push(p)))
            tail = [lambda: stream.push(keep(rs.flush())), stream.flush]   # the outputs that waited for the future first
        else:
            feed, tail = stream.push, [stream.flush]
            if track_out is not None:
                track_out.append(audio)
        pieces = [audio[i:i + step] for i in range(0, audio.shape[0], step)]
        for call in [lambda p=p: feed(p.unsqueeze(0)) for p in pieces] + tail:
            e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            e[0].record()
            rows = call()
            e[1].record()
            if rows.shape[1]:
                events.append(e)
            parts.append(rows[0])
        out = torch.cat(parts, 0)
        if convert and track_out is not None:
            track_out.append(torch.cat(converted, 0))
    torch.cuda.synchronize(dev)
    wall = time.perf_counter() - t0
    kernels.HipKernels.check_async_errors()
    gpu_ms = [a.elapsed_time(b) for a, b in events]
    return out, {"wall_s": wall, "chunks": len(gpu_ms), "gpu_ms_per_chunk_p50": _pctl(gpu_ms, 50),
                 "gpu_ms_per_chunk_p99": _pctl(gpu_ms, 99)}


def generate(opts, cfg, device):
    """-> the generation.json dict; writes <logdir>/samples/<name>.npy"""
    ds = cfg["dataset"]
    rate = int(ds["audio_rate"])
    hop = int(ds["audio_rate"] // ds["video_rate"])
    gen = build_generator(cfg, device)
    path = scoring.load_generator(gen, opts)
    window = gen.window_size
    pad = window - hop
    tracks, scaler = _tracks(opts, cfg)
    outdir = os.path.join(opts.logdir, "samples")
    os.makedirs(outdir, exist_ok=True)
    res = {"checkpoint": path, "seed": int(opts.seed), "chunk_frames": int(opts.chunk_frames),
           "resampler": getattr(opts, "resampler", "fft"), "tracks": []}
    for name, samples, samples_rate, source_rate in tracks:
        audio = torch.as_tensor(np.ascontiguousarray(samples), dtype=torch.float32)
        T = n_frames(A.out_len(audio.shape[0], *A.ratio(samples_rate, rate)), window, hop, pad)
        if T == 0:
            raise SystemExit("track %s: %d samples hold no frame" % (name, audio.shape[0]))
        beat = getattr(opts, "beat_align", False)
        heard = [] if beat else None
        poses, timing = run_track(gen, audio, opts.seed, window, hop, pad, opts.chunk_frames, (samples_rate, rate),
                                  heard)
        assert poses.shape[0] == T, (poses.shape, T)
        arr = scaler.inverse_transform(poses.cpu().numpy().astype(np.float64)).astype(np.float32)
        saved = arr.reshape(T, STICK_CHANNELS // 3, 3)
        np.save(os.path.join(outdir, name + ".npy"), saved)
        seconds = audio.shape[0] / float(samples_rate)
        res["tracks"].append(dict(name=name, frames=T, seconds=seconds, chunk_frames=int(opts.chunk_frames),
                                  real_time_factor=seconds / timing["wall_s"] if timing["wall_s"] > 0 else None,
                                  **timing))
        if source_rate is not None:
            res["tracks"][-1]["source_rate"] = int(source_rate)
        if beat:
            from .. import metrics
            s = metrics.beat_scores(heard[0].contiguous(), torch.from_numpy(saved).to(heard[0].device), hop, rate=rate)
            res["tracks"][-1].update(beat_align=float(s["align"][0]), beat_cover=float(s["cover"][0]),
                                     beat_motion_events=int(s["n_motion"][0]), beat_music_events=int(s["n_music"][0]))
        if getattr(opts, "video", False):
            from .. import visualize
            path = os.path.join(outdir, name + ".avi")
            encoder = getattr(opts, "encoder", None)
            # the keyword only when it is not the default: frame_to_vid is the reference's three-argument call
            kw = {} if encoder in (None, "pil") else {"encoder": encoder}
            vid = visualize.frame_to_vid(saved, path, ds["video_rate"], **kw)
            res["tracks"][-1].update(video=path, render_ms=vid["render_ms"], video_s=vid["wall_s"])
            if encoder is not None:
                res["tracks"][-1].update(encoder=encoder)
    with open(os.path.join(outdir, "generation.json"), "w") as f:
        json.dump(json_safe(res), f, indent=1, allow_nan=False)
    return res


def main(argv=None):
    return scoring.run(parse_args, generate, argv, seed=0)       # generate wrote samples/generation.json itself


if __name__ == "__main__":
    main()
