"""Stick-figure videos of dances (reference visualize.py:195-255: draw, frame_to_vid).

    python -m music2dance_amd.visualize POSES.npy OUT.avi [--fps 25] [--encoder {pil,hip}]

`render` draws poses into uint8 RGB frames on the device in one launch (m2d_render_sticks: the reference's skeleton,
blue on white, as its OpenCV calls draw it, but rasterised exactly by our own rule).
`AviWriter` muxes JPEG frames into an AVI 1.0 MJPG file (PIL encodes, 4:4:4 chroma; no OpenCV). `frame_to_vid` is the
reference's entry point: 300 x 300 frames, rendered in chunks of at most CHUNK_FRAMES so that host memory stays
bounded. Rendering needs a HIP device (there is no CPU path); AviWriter is host code.
With encoder="hip" the frames never leave the device: `encode_jpeg` turns a chunk into baseline JPEG streams there
(m2d_jpeg_encode: integer colour transform, DCT and quantisation, the standard's Huffman tables, one restart interval
per row of blocks), only the compressed bytes are copied, and `AviWriter.write_encoded`
appends them.
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
ENCODERS = ("pil", "hip")

# Annex K.1 of the JPEG standard: base quantisation tables, row-major
_BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
              14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
              49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# Annex K.3: the typical Huffman tables as (table class << 4 | id, code counts of lengths 1..16, symbols), in the
# order of the DHT segments (csrc/jpeg.hip holds the same constants)
HUFFMAN_SPEC = (
    (0x00, (0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x10, (0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125),
     (1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82,
      209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67,
      68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117,
      118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162,
      163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199,
      200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241,
      242, 243, 244, 245, 246, 247, 248, 249, 250)),
    (0x01, (0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12))),
    (0x11, (0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119),
     (0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51,
      82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58,
      67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116,
      117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153,
      154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
      198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234,
      242, 243, 244, 245, 246, 247, 248, 249, 250)),
)


def jpeg_tables(quality):
    """-> (luma, chroma, huffman): the two quantisation tables of `quality` (1..100; Annex K.1 scaled as libjpeg scales
    them: s = 5000 // q below 50, else 200 - 2 q; entry clamp((base s + 50) // 100, 1, 255)), 64 entries each in
    row-major order, and HUFFMAN_SPEC"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("jpeg_tables: quality must lie in [1, 100], got %r" % (quality,))
    s = 5000 // q if q < 50 else 200 - 2 * q
    luma, chroma = ([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (_BASE_LUMA, _BASE_CHROMA))
    return luma, chroma, HUFFMAN_SPEC


def _encode_device(frames, qtabs, capacity):
    """the device encoder (the seam host tests replace): -> (out uint8 (capacity,), offsets int64 (n + 1,))"""
    return kernels.impl().jpeg_encode(frames, qtabs, capacity)


def encode_jpeg(frames, quality=95, stats=None):
    """frames (n, height, width, 3) uint8 on a HIP device -> list of n JPEG streams (bytes). Two device-to-host copies:
    the offsets, then the used bytes only. The first launch gets room for the raw frame bytes; should the streams
    need more (noise at high quality), the offsets say how much and one more launch gets exactly that. `stats`
    (optional dict) gains the launches' device time in `encode_ms`, the copies' wall time in `d2h_s` and the host time
    spent waiting for the encoder in `encode_s`."""
    luma, chroma, _ = jpeg_tables(quality)
    n = int(frames.shape[0])
    cap = int(frames.numel())
    timed = stats is not None and torch.cuda.is_available()
    events, wait_s, copy_s = [], 0.0, 0.0
    for _ in range(2):
        if timed:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
        out, offsets = _encode_device(frames, (luma, chroma), cap)
        t0 = time.perf_counter()
        if timed:
            b.record()
            b.synchronize()
            events.append((a, b))
        t1 = time.perf_counter()
        off = offsets.cpu().tolist()
        wait_s, copy_s = wait_s + (t1 - t0), copy_s + (time.perf_counter() - t1)
        if off[n] <= cap:
            break
        cap = off[n]
    else:
        raise _lib.M2dError("encode_jpeg: the encoder asked for %d bytes after being given what it asked for" % off[n])
    t1 = time.perf_counter()
    data = out[:off[n]].cpu().numpy().tobytes()
    copy_s += time.perf_counter() - t1
    if stats is not None:
        stats["encode_ms"] = stats.get("encode_ms", 0.0) + sum(a.elapsed_time(b) for a, b in events)
        stats["d2h_s"] = stats.get("d2h_s", 0.0) + copy_s
        stats["encode_s"] = stats.get("encode_s", 0.0) + wait_s
    return [data[off[i]:off[i + 1]] for i in range(n)]


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

    def write_encoded(self, payloads):
        """JPEG streams that are already encoded (bytes, each from SOI to EOI) -> appended, one frame each; returns
        self. Any split of the payloads into calls gives the same file."""
        if self.closed:
            raise ValueError("AviWriter: write after close")
        payloads = list(payloads)
        for data in payloads:
            if (not isinstance(data, (bytes, bytearray, memoryview)) or len(data) < 4
                    or bytes(data[:2]) != b"\xff\xd8" or bytes(data[-2:]) != b"\xff\xd9"):
                raise ValueError("AviWriter: a payload must be a JPEG stream from SOI to EOI")
        t0 = time.perf_counter()
        for data in payloads:
            self._append(bytes(data))
        self.mux_s += time.perf_counter() - t0
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


def _device_poses(part):
    """one chunk of poses (numpy or torch, host or device) -> a tensor on the current HIP device"""
    if torch.is_tensor(part) and part.is_cuda:
        return part
    if not torch.cuda.is_available():
        raise _lib.M2dError("frame_to_vid renders on a HIP device: none is visible and there is no CPU path")
    x = part if torch.is_tensor(part) else torch.from_numpy(np.ascontiguousarray(part, dtype=np.float32))
    return x.to(torch.device("cuda", torch.cuda.current_device()))


def _render_device(part, height, width, stats):
    """one chunk of poses -> uint8 frames (k, height, width, 3) left on the device; adds the render launch's device
    time to stats['render_ms'] (the seam host tests replace on the hip path)"""
    x = _device_poses(part)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    frames = render(x, height, width)
    b.record()
    b.synchronize()
    stats["render_ms"] += a.elapsed_time(b)
    return frames


def frame_to_vid(frames, name, fps, encoder="pil"):
    """The reference's frame_to_vid: poses (T, 23, 3) or (T, 69) (numpy or torch, host or device; not modified) ->
    a 300 x 300 MJPG AVI at `name`, `fps` frames per second, rendered CHUNK_FRAMES at a time. encoder "pil": the raw
    frames are copied to the host and PIL encodes them; "hip": m2d_jpeg_encode encodes each chunk on the device and
    only the compressed bytes are copied (d2h_s: that copy; encode_s: host time waiting for the encoder). Returns the
    time split {frames, render_ms, d2h_s, encode_s, mux_s, wall_s, encoder, encode_ms}; encode_ms is the device time
    of the encode launches (0 for pil)."""
    if encoder not in ENCODERS:
        raise ValueError("frame_to_vid: encoder must be one of %s, got %r" % (ENCODERS, encoder))
    t0 = time.perf_counter()
    height = width = 300
    T = len(frames)
    stats = {"frames": T, "render_ms": 0.0, "d2h_s": 0.0, "encode_s": 0.0, "mux_s": 0.0}
    hip = {"encode_ms": 0.0, "d2h_s": 0.0, "encode_s": 0.0}
    with AviWriter(name, fps, height, width) as vid:
        for i in range(0, T, CHUNK_FRAMES):
            part = frames[i:i + CHUNK_FRAMES]
            if encoder == "hip":
                vid.write_encoded(encode_jpeg(_render_device(part, height, width, stats), vid.quality, hip))
            else:
                vid.write(_render_host(part, height, width, stats))
    stats["encode_s"], stats["mux_s"] = vid.encode_s, vid.mux_s
    if encoder == "hip":
        stats["d2h_s"], stats["encode_s"] = hip["d2h_s"], hip["encode_s"]
    stats["wall_s"] = time.perf_counter() - t0
    stats["encoder"], stats["encode_ms"] = encoder, hip["encode_ms"]
    return stats


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="render saved poses (T, 23, 3) to a 300 x 300 stick-figure MJPG AVI")
    ap.add_argument("poses", type=str, help=".npy of poses (T, 23, 3) or (T, 69), e.g. <logdir>/samples/<name>.npy")
    ap.add_argument("out", type=str, help="output .avi")
    ap.add_argument("--fps", type=float, default=25.0, help="frames per second (default 25)")
    ap.add_argument("--encoder", choices=ENCODERS, default="pil",
                    help="JPEG encoder: pil = on the host from raw frames (default), hip = on the device")
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
    kw = {} if opts.encoder == "pil" else {"encoder": opts.encoder}
    stats = frame_to_vid(poses, opts.out, opts.fps, **kw)
    print("%s: %d frames, %.1f s" % (opts.out, stats["frames"], stats["wall_s"]))
    return stats


if __name__ == "__main__":
    main()
