"""Stick-figure videos of dances (reference visualize.py:195-255: draw, frame_to_vid).

    python -m music2dance_amd.visualize POSES.npy OUT.avi [--fps 25]

`render` draws poses into uint8 RGB frames on the device in one launch (m2d_render_sticks: the reference's skeleton,
blue on white, as its OpenCV calls draw it, but rasterised exactly by our own rule).
`AviWriter` muxes JPEG frames into an AVI 1.0 MJPG file (PIL encodes, 4:4:4 chroma; no OpenCV). `frame_to_vid` is the
reference's entry point: 300 x 300 frames, rendered in chunks of at most CHUNK_FRAMES so that host memory stays
bounded. Rendering needs a HIP device (there is no CPU path); AviWriter is host code.
"""
import argparse
import io
import os
import struct
import time
from fractions import Fraction

import numpy as np
import torch

from . import _lib, kernels

N_JOINTS = 23
CHUNK_FRAMES = 256
MAX_FILE_BYTES = 2 ** 31 - 1   # AVI 1.0 without OpenDML extensions
AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10


def render(poses, height=300, width=300, out=None):
    """poses (n, 23, 3) or (n, 69) on a HIP device (float64 is rounded to fp32 first) -> uint8 (n, height, width, 3)
    device tensor of stick figures, one launch"""
    if not torch.is_tensor(poses) or not poses.is_cuda:
        raise _lib.M2dError("render: poses must be a tensor on a HIP device; there is no CPU path")
    if poses.dim() not in (2, 3) or tuple(poses.shape[1:]) not in ((3 * N_JOINTS,), (N_JOINTS, 3)):
        raise _lib.M2dError("render: poses must be (n, 23, 3) or (n, 69), got %s" % (tuple(poses.shape),))
    x = poses.to(torch.float32).reshape(poses.shape[0], 3 * N_JOINTS).contiguous()
    return kernels.impl().render_sticks(x, height, width, out)


class AviWriter:
    """AVI 1.0 (RIFF 'AVI ') with one MJPG video stream: hdrl (avih, strl: strh, strf), movi ('00dc' chunks), idx1.
    Frames are appended as they come; counts and sizes are patched in close(). write() of any split of the frames
    gives the same bytes. Refuses to grow past MAX_FILE_BYTES."""

    def __init__(self, path, fps, height, width, quality=95):
        rate = Fraction(fps).limit_denominator(1001)
        if rate <= 0:
            raise ValueError("AviWriter: fps must be positive, got %r" % (fps,))
        if not (0 < int(height) <= 32767 and 0 < int(width) <= 32767):
            raise ValueError("AviWriter: bad frame size %r x %r" % (height, width))
        self.path, self.height, self.width, self.quality = path, int(height), int(width), int(quality)
        self.rate, self.scale = rate.numerator, rate.denominator
        self.index = []          # (offset from the 'movi' tag, payload size) per frame
        self.max_chunk = 0
        self.encode_s = 0.0      # time in the JPEG encoder
        self.mux_s = 0.0         # time writing chunks and headers
        self.f = open(path, "wb")
        self.f.write(self._headers())
        self.movi = self.f.tell() - 4   # offset of the 'movi' list type: idx1 offsets count from here
        self.closed = False

    def _headers(self):
        w, h, n = self.width, self.height, len(self.index)
        us = int(round(1e6 * self.scale / self.rate))
        buf = self.max_chunk + 8
        bps = min(self.max_chunk * self.rate // self.scale, 0xFFFFFFFF)
        avih = struct.pack("<14I", us, bps, 0, AVIF_HASINDEX, n, 0, 1, buf, w, h, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4h", b"vids", b"MJPG", 0, 0, 0, 0, self.scale, self.rate, 0, n, buf,
                           0xFFFFFFFF, 0, 0, 0, w, h)
        strf = struct.pack("<IiiHH4sIiiII", 40, w, h, 1, 24, b"MJPG", w * h * 3, 0, 0, 0, 0)
        strl = b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf)
        hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", strl)
        movi_size = 4 + sum(8 + s + (s & 1) for _, s in self.index)
        return (b"RIFF" + struct.pack("<I", 0) + b"AVI " + _chunk(b"LIST", hdrl) + b"LIST"
                + struct.pack("<I", movi_size) + b"movi")

    def encode(self, frame):
        """one (height, width, 3) uint8 RGB frame -> JPEG bytes (quality, 4:4:4)"""
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray(frame, "RGB").save(buf, "JPEG", quality=self.quality, subsampling=0)
        return buf.getvalue()

    def write(self, frames):
        """frames (k, height, width, 3) uint8 (numpy or host torch) -> appended; returns self"""
        if self.closed:
            raise ValueError("AviWriter: write after close")
        a = frames.numpy() if torch.is_tensor(frames) else np.asarray(frames)
        if a.dtype != np.uint8 or a.ndim != 4 or a.shape[1:] != (self.height, self.width, 3):
            raise ValueError("AviWriter: uint8 (k, %d, %d, 3) frames expected, got %s %s"
                             % (self.height, self.width, a.dtype, a.shape))
        for frame in a:
            t0 = time.perf_counter()
            data = self.encode(np.ascontiguousarray(frame))
            t1 = time.perf_counter()
            self._append(data)
            self.mux_s += time.perf_counter() - t1
            self.encode_s += t1 - t0
        return self

    def _append(self, data):
        n = len(data)
        pos = self.f.tell()
        end = pos + 8 + n + (n & 1) + 8 + 16 * (len(self.index) + 1)   # with this frame's idx1 entry
        if end > MAX_FILE_BYTES:
            raise OverflowError("AviWriter: %s would grow to %d bytes, past the AVI 1.0 limit of %d (OpenDML is not "
                                "supported); split the video" % (self.path, end, MAX_FILE_BYTES))
        self.f.write(b"00dc" + struct.pack("<I", n) + data + (b"\0" if n & 1 else b""))
        self.index.append((pos - self.movi, n))
        self.max_chunk = max(self.max_chunk, n)

    def close(self):
        if self.closed:
            return
        t0 = time.perf_counter()
        idx = b"".join(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, off, n) for off, n in self.index)
        self.f.write(_chunk(b"idx1", idx))
        size = self.f.tell()
        self.f.seek(0)
        head = self._headers()
        self.f.write(head[:4] + struct.pack("<I", size - 8) + head[8:])
        self.f.close()
        self.closed = True
        self.mux_s += time.perf_counter() - t0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _chunk(fourcc, data):
    return fourcc + struct.pack("<I", len(data)) + data + (b"\0" if len(data) & 1 else b"")


def _render_host(part, height, width, stats):
    """one chunk of poses (numpy or torch, host or device) -> host uint8 frames (k, height, width, 3); adds the render
    launch's device time to stats['render_ms'] and the device-to-host copy's wall time to stats['d2h_s']"""
    if torch.is_tensor(part) and part.is_cuda:
        x = part
    elif not torch.cuda.is_available():
        raise _lib.M2dError("frame_to_vid renders on a HIP device: none is visible and there is no CPU path")
    else:
        x = part if torch.is_tensor(part) else torch.from_numpy(np.ascontiguousarray(part, dtype=np.float32))
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    frames = render(x, height, width)
    b.record()
    b.synchronize()
    t0 = time.perf_counter()
    out = frames.cpu().numpy()
    stats["d2h_s"] += time.perf_counter() - t0
    stats["render_ms"] += a.elapsed_time(b)
    return out


def frame_to_vid(frames, name, fps):
    """The reference's frame_to_vid: poses (T, 23, 3) or (T, 69) (numpy or torch, host or device; not modified) ->
    a 300 x 300 MJPG AVI at `name`, `fps` frames per second, rendered CHUNK_FRAMES at a time. Returns the time split
    {frames, render_ms, d2h_s, encode_s, mux_s, wall_s}."""
    t0 = time.perf_counter()
    height = width = 300
    T = len(frames)
    stats = {"frames": T, "render_ms": 0.0, "d2h_s": 0.0, "encode_s": 0.0, "mux_s": 0.0}
    with AviWriter(name, fps, height, width) as vid:
        for i in range(0, T, CHUNK_FRAMES):
            vid.write(_render_host(frames[i:i + CHUNK_FRAMES], height, width, stats))
    stats["encode_s"], stats["mux_s"] = vid.encode_s, vid.mux_s
    stats["wall_s"] = time.perf_counter() - t0
    return stats


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="render saved poses (T, 23, 3) to a 300 x 300 stick-figure MJPG AVI")
    ap.add_argument("poses", type=str, help=".npy of poses (T, 23, 3) or (T, 69), e.g. <logdir>/samples/<name>.npy")
    ap.add_argument("out", type=str, help="output .avi")
    ap.add_argument("--fps", type=float, default=25.0, help="frames per second (default 25)")
    return ap.parse_args(argv)


def main(argv=None):
    opts = parse_args(argv)
    poses = np.load(opts.poses)
    if poses.ndim not in (2, 3) or poses.shape[1:] not in ((3 * N_JOINTS,), (N_JOINTS, 3)):
        raise SystemExit("%s: poses (T, 23, 3) or (T, 69) expected, got %s" % (opts.poses, poses.shape))
    if opts.fps <= 0:
        raise SystemExit("--fps must be positive")
    d = os.path.dirname(os.path.abspath(opts.out))
    os.makedirs(d, exist_ok=True)
    stats = frame_to_vid(poses, opts.out, opts.fps)
    print("%s: %d frames, %.1f s" % (opts.out, stats["frames"], stats["wall_s"]))
    return stats


if __name__ == "__main__":
    main()
