"""The drawing rule of m2d_render_sticks stated in numpy: the reference implementation that
tests/test_render_host.py checks and tests/test_gpu_render.py compares the kernel against, bit for bit.

Coordinates: x' = fl32(x + width // 2), y' = fl32(y + height // 2); pixel (trunc(x'), trunc(y')); a midpoint is
trunc(fl32(fl32(a' + b') * 0.5)). A joint is valid when |x'|, |y'| < 2^14 (so also finite); an invalid joint draws no
disk and cancels every segment that uses it, directly or through a midpoint. Coverage, in unflipped (column, pixel
height) coordinates, exact in int64: disks (c - px)^2 + (r - py)^2 <= 16; segments squared distance <= 1. The image
is flipped vertically (row = height - 1 - pixel height); figure pixels are (0, 0, 255), the rest white.

`parse_avi` reads an AVI 1.0 file back and checks its RIFF structure (both test files use it)."""
import struct

import numpy as np

N_JOINTS = 23
# points 23..26: midpoints of these joint pairs
MIDPOINTS = [(0, 1), (3, 12), (10, 11), (19, 20)]
# the reference's skeleton: 15 joint pairs, then 6 segments to midpoints (point indices as above)
SEGMENTS = [(0, 1), (3, 4), (4, 5), (5, 6), (12, 13), (13, 14), (14, 15), (2, 7), (7, 8), (8, 9), (10, 11), (2, 16),
            (16, 17), (17, 18), (19, 20),
            (23, 24), (3, 24), (12, 24), (2, 24), (9, 25), (18, 26)]
LIMIT = np.float32(2 ** 14)
FIGURE = (0, 0, 255)


def points(frame, height, width):
    """frame (23, >= 2) -> (px, py, valid) of the 27 points (joints, then midpoints), int64 / bool"""
    f = np.asarray(frame, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        xs = f[:, 0] + np.float32(width // 2)
        ys = f[:, 1] + np.float32(height // 2)
        ok = (np.abs(xs) < LIMIT) & (np.abs(ys) < LIMIT)
        mx = [(xs[a] + xs[b]) * np.float32(0.5) for a, b in MIDPOINTS]
        my = [(ys[a] + ys[b]) * np.float32(0.5) for a, b in MIDPOINTS]
    X = np.concatenate([xs, np.array(mx, np.float32)])
    Y = np.concatenate([ys, np.array(my, np.float32)])
    V = np.concatenate([ok, np.array([ok[a] and ok[b] for a, b in MIDPOINTS])])
    px = np.where(V, np.trunc(np.where(V, X, 0)), 0).astype(np.int64)
    py = np.where(V, np.trunc(np.where(V, Y, 0)), 0).astype(np.int64)
    return px, py, V


def cover_disk(cov, px, py):
    """mark the pixels (c, r) with (c - px)^2 + (r - py)^2 <= 16 in cov (height, width), unflipped rows"""
    H, W = cov.shape
    c0, c1, r0, r1 = max(px - 4, 0), min(px + 4, W - 1), max(py - 4, 0), min(py + 4, H - 1)
    if c0 > c1 or r0 > r1:
        return
    C, R = np.meshgrid(np.arange(c0, c1 + 1, dtype=np.int64), np.arange(r0, r1 + 1, dtype=np.int64))
    cov[r0:r1 + 1, c0:c1 + 1] |= (C - px) ** 2 + (R - py) ** 2 <= 16


def cover_segment(cov, p0, p1):
    """mark the pixels Q at squared distance <= 1 from the segment p0 - p1 (integer endpoints), exactly in int64"""
    H, W = cov.shape
    (x0, y0), (x1, y1) = p0, p1
    c0, c1 = max(min(x0, x1) - 1, 0), min(max(x0, x1) + 1, W - 1)
    r0, r1 = max(min(y0, y1) - 1, 0), min(max(y0, y1) + 1, H - 1)
    if c0 > c1 or r0 > r1:
        return
    C, R = np.meshgrid(np.arange(c0, c1 + 1, dtype=np.int64), np.arange(r0, r1 + 1, dtype=np.int64))
    dx, dy = np.int64(x1 - x0), np.int64(y1 - y0)
    L = dx * dx + dy * dy
    qx, qy = C - x0, R - y0
    t = qx * dx + qy * dy
    near0 = qx * qx + qy * qy <= 1
    near1 = (C - x1) ** 2 + (R - y1) ** 2 <= 1
    cross = qx * dy - qy * dx
    inside = cross * cross <= L
    cov[r0:r1 + 1, c0:c1 + 1] |= np.where(t <= 0, near0, np.where(t >= L, near1, inside))


def coverage(frame, height, width):
    """bool (height, width) in unflipped rows: row r is pixel height r"""
    px, py, V = points(frame, height, width)
    cov = np.zeros((height, width), dtype=bool)
    for j in range(N_JOINTS):
        if V[j]:
            cover_disk(cov, int(px[j]), int(py[j]))
    for a, b in SEGMENTS:
        if V[a] and V[b]:
            cover_segment(cov, (int(px[a]), int(py[a])), (int(px[b]), int(py[b])))
    return cov


def render(poses, height=300, width=300):
    """poses (n, 23, 3) or (n, 69), any float dtype (rounded to fp32 first) -> uint8 (n, height, width, 3)"""
    p = np.asarray(poses, dtype=np.float32).reshape(-1, N_JOINTS, 3)
    out = np.full((p.shape[0], height, width, 3), 255, dtype=np.uint8)
    for i in range(p.shape[0]):
        out[i][coverage(p[i], height, width)[::-1]] = FIGURE
    return out


def _chunks(buf, pos, end):
    """RIFF sub-chunks of buf[pos:end] -> [(fourcc, data_start, size)]; sizes must tile the range with even padding"""
    out = []
    while pos < end:
        assert pos + 8 <= end, "truncated chunk header at %d" % pos
        fourcc, size = buf[pos:pos + 4], struct.unpack("<I", buf[pos + 4:pos + 8])[0]
        assert pos + 8 + size <= end, "chunk %r at %d overruns its parent" % (fourcc, pos)
        out.append((fourcc, pos + 8, size))
        pos += 8 + size + (size & 1)
    assert pos == end, "chunks do not tile their parent (%d != %d)" % (pos, end)
    return out


def parse_avi(path):
    """-> dict(avih=..., strh=..., strf=..., frames=[payload bytes], index=[(flags, offset, size)]) after checking
    every RIFF / LIST size, the stream header fields and that each idx1 entry lands on its '00dc' chunk"""
    buf = open(path, "rb").read()
    assert buf[:4] == b"RIFF" and buf[8:12] == b"AVI ", "not an AVI file"
    assert struct.unpack("<I", buf[4:8])[0] == len(buf) - 8, "RIFF size"
    top = _chunks(buf, 12, len(buf))
    assert [c[0] for c in top] == [b"LIST", b"LIST", b"idx1"], top
    (_, hdrl, hdrl_n), (_, movi, movi_n), (_, idx, idx_n) = top
    assert buf[hdrl:hdrl + 4] == b"hdrl" and buf[movi:movi + 4] == b"movi"
    hd = _chunks(buf, hdrl + 4, hdrl + hdrl_n)
    assert [c[0] for c in hd] == [b"avih", b"LIST"] and hd[0][2] == 56
    avih = dict(zip(("us_per_frame", "max_bytes_per_sec", "padding", "flags", "total_frames", "initial_frames",
                     "streams", "suggested_buffer", "width", "height"), struct.unpack("<10I", buf[hd[0][1]:hd[0][1] + 40])))
    strl = hd[1][1]
    assert buf[strl:strl + 4] == b"strl"
    sl = _chunks(buf, strl + 4, strl + hd[1][2])
    assert [c[0] for c in sl] == [b"strh", b"strf"] and sl[0][2] == 56 and sl[1][2] == 40
    v = struct.unpack("<4s4sIHHIIIIIIII4h", buf[sl[0][1]:sl[0][1] + 56])
    strh = dict(type=v[0], handler=v[1], scale=v[6], rate=v[7], length=v[9], suggested_buffer=v[10], frame=v[13:])
    v = struct.unpack("<IiiHH4sIiiII", buf[sl[1][1]:sl[1][1] + 40])
    strf = dict(size=v[0], width=v[1], height=v[2], planes=v[3], bits=v[4], compression=v[5], image_bytes=v[6])
    frames = _chunks(buf, movi + 4, movi + movi_n)
    assert all(c[0] == b"00dc" for c in frames)
    for fourcc, start, size in frames:
        if size & 1:
            assert buf[start + size] == 0, "odd chunk not padded with a zero byte"
    assert idx_n == 16 * len(frames)
    index = []
    for k, (_, start, size) in enumerate(frames):
        ck, flags, off, n = struct.unpack("<4sIII", buf[idx + 16 * k:idx + 16 * k + 16])
        assert ck == b"00dc" and n == size, (k, ck, n, size)
        assert movi + off == start - 8, "idx1 entry %d points to %d, chunk at %d" % (k, movi + off, start - 8)
        index.append((flags, off, n))
    return dict(avih=avih, strh=strh, strf=strf, index=index, frames=[buf[s:s + n] for _, s, n in frames])
