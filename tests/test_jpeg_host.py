"""The device JPEG path on the host: the encoding rule's numpy statement (tests/jpeg_rule.py) against PIL - tables,
decodability, quality and size, the hard entropy-coding cases - then AviWriter.write_encoded, frame_to_vid with
encoder="hip" over stand-ins made of the two numpy rules, and the command lines. No GPU."""
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_rule as J
from tests import render_rule as R

NOISE_SEED = 3955   # chosen so that the 33 x 50 noise frame holds a ZRL symbol (test_noise_frame_hits_the_hard_cases)


def pil_encode(frame, quality):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(frame, "RGB").save(buf, "JPEG", quality=quality, subsampling=0)
    return buf.getvalue()


def decoded(payload, shape):
    from PIL import Image
    img = Image.open(io.BytesIO(payload))
    img.load()
    assert img.format == "JPEG" and img.mode == "RGB" and img.size == (shape[1], shape[0])
    return np.asarray(img).astype(np.int32)


def segments(data):
    """marker segments before the scan -> [(marker, body)]"""
    assert data[:2] == b"\xff\xd8"
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        n = (data[i + 2] << 8) | data[i + 3]
        out.append((data[i + 1], data[i + 4:i + 2 + n]))
        if data[i + 1] == 0xDA:
            return out
        i += 2 + n


def stick_poses(n, seed=0):
    return np.random.default_rng(seed).uniform(-120, 120, size=(n, R.N_JOINTS, 3)).astype(np.float32)


@pytest.fixture(scope="module")
def sticks():
    """two 300 x 300 stick frames and the rule's encoding of each at quality 95: made once, never modified"""
    frames = R.render(stick_poses(2), 300, 300)
    frames.setflags(write=False)
    return frames, [J.encode(f, 95) for f in frames]


def noise_frame():
    return np.random.default_rng(NOISE_SEED).integers(0, 256, (33, 50, 3), dtype=np.uint8)


def crop(frame, h, w):
    """an h x w window of a stick frame with its top-left corner two pixels up and left of the first figure pixel:
    figure and background in one small frame"""
    ys, xs = np.nonzero(frame[..., 0] == 0)
    y0, x0 = max(int(ys[0]) - 2, 0), max(int(xs[0]) - 2, 0)
    out = np.ascontiguousarray(frame[y0:y0 + h, x0:x0 + w])
    assert out.shape == (h, w, 3) and (out[..., 0] == 0).any() and (out[..., 0] == 255).any()
    return out


# ------------------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("quality", [1, 50, 75, 95, 100])
def test_tables_equal_the_ones_pil_writes(quality):
    from music2dance_amd import visualize as V
    luma, chroma, huffman = V.jpeg_tables(quality)
    segs = segments(pil_encode(np.zeros((8, 8, 3), np.uint8), quality))
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    dqt = [b for m, b in segs if m == 0xDB]
    for i, table in enumerate((luma, chroma)):
        assert dqt[i][0] == i and len(dqt[i]) == 65
        assert [table[J.ZIGZAG[k]] for k in range(64)] == list(dqt[i][1:])
    dht = [b for m, b in segs if m == 0xC4]
    assert [(b[0], tuple(b[1:17]), tuple(b[17:])) for b in dht] == [tuple(h) for h in huffman]
    # the rule carries its own copy of the same tables
    assert (list(luma), list(chroma)) == tuple(map(list, J.quant_tables(quality)))
    assert [(i, tuple(bits), tuple(vals)) for i, (bits, vals) in J.HUFFMAN] == [tuple(h) for h in huffman]
    with pytest.raises(ValueError):
        V.jpeg_tables(0)
    with pytest.raises(ValueError):
        V.jpeg_tables(101)


def test_header_is_laid_out_as_pil_lays_it_out(sticks):
    frames, enc = sticks
    mine, pil = segments(enc[0][0]), segments(pil_encode(frames[0], 95))
    assert [m for m, _ in mine] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDD, 0xDA]
    assert [s for s in mine if s[0] != 0xDD] == pil
    assert dict(mine)[0xDD] == bytes([0, 38])   # one row of 38 MCUs


# ----------------------------------------------------------------------------------------------------------- decoding
def check_against_pil(frame, data, quality, size_too):
    """PIL decodes the rule's stream; its error is within 5 % of the error of PIL's own encoding, its size too"""
    src = frame.astype(np.int32)
    pil = pil_encode(frame, quality)
    mine_err = np.abs(decoded(data, frame.shape) - src)
    pil_err = np.abs(decoded(pil, frame.shape) - src)
    print("%s q%d: mae %.4f (PIL %.4f), bytes %d (PIL %d)" % (frame.shape, quality, mine_err.mean(), pil_err.mean(),
                                                             len(data), len(pil)))
    assert mine_err.mean() <= 1.05 * pil_err.mean() + 0.02, (mine_err.mean(), pil_err.mean())
    if size_too:
        assert len(data) <= 1.05 * len(pil), (len(data), len(pil))
    return mine_err


def test_stick_frames_decode_like_pils_own(sticks):
    frames, enc = sticks
    for frame, (data, _) in zip(frames, enc):
        err = check_against_pil(frame, data, 95, size_too=True)
        assert err.mean() <= 1.0 and err.max() <= 48, (err.mean(), err.max())
        got = decoded(data, frame.shape)
        want = frame.astype(np.int32)
        assert ((want[..., 2] - want[..., 0] > 128) == (got[..., 2] - got[..., 0] > 128)).all()


@pytest.mark.parametrize("h,w", [(8, 8), (9, 17)])
def test_small_frames_decode_like_pils_own(sticks, h, w):
    frame = crop(sticks[0][0], h, w)
    data, _ = J.encode(frame, 95)
    check_against_pil(frame, data, 95, size_too=False)
    assert len(dict(segments(data))[0xDA]) == 10 and data[-2:] == b"\xff\xd9"


def test_noise_frame_decodes_like_pils_own():
    frame = noise_frame()
    data, _ = J.encode(frame, 100)
    check_against_pil(frame, data, 100, size_too=False)


def test_restart_markers_cycle(sticks):
    data = sticks[1][0][0]
    scan = data[J.header(300, 300, J.quant_tables(95)).__len__():]
    marks = [scan[i + 1] for i in range(len(scan) - 1) if scan[i] == 0xFF and scan[i + 1] != 0]
    assert marks == [0xD0 + (r & 7) for r in range(37)] + [0xD9]


# --------------------------------------------------------------------------------------------------------- hard cases
def test_noise_frame_hits_the_hard_cases():
    _, c = J.encode(noise_frame(), 100)
    assert c["zrl"] >= 1 and c["stuffed"] >= 1 and c["no_eob"] >= 1, c
    assert c["max_dc_cat"] >= 9 and c["max_ac_cat"] >= 9, c


def test_white_frame_has_no_ac_symbols():
    data, c = J.encode(np.full((24, 40, 3), 255, np.uint8), 95)
    assert c["ac_symbols"] == 0 and c["zrl"] == 0 and c["no_eob"] == 0 and c["max_ac_cat"] == 0
    assert (decoded(data, (24, 40)) == 255).all()


def test_coefficients_stay_in_their_categories():
    # the extremes of the DC: constant blocks of 0 and of 255 next to each other, quantised by 1
    frame = np.zeros((8, 16, 3), np.uint8)
    frame[:, 8:] = 255
    k = J.coefficients(frame, ([1] * 64, [1] * 64))
    assert k[0, 0, 0, 0] == -1024 and k[0, 1, 0, 0] == 1016 and not k[..., 1:].any()
    _, c = J.encode(frame, 100)
    assert c["max_dc_cat"] == 11
    # a checkerboard of 0 and 255 puts the largest magnitude an AC coefficient reaches at (7, 7)
    board = np.where((np.add.outer(np.arange(8), np.arange(8)) & 1)[..., None], 255, 0).astype(np.uint8).repeat(3, 2)
    k = J.coefficients(board, ([1] * 64, [1] * 64))
    assert 512 <= np.abs(k[0, 0, 0, 1:]).max() <= 1023


# ------------------------------------------------------------------------------------------------------ write_encoded
def test_write_encoded_equals_write(tmp_path, monkeypatch):
    from music2dance_amd import visualize as V
    rng = np.random.default_rng(2)
    payloads = [b"\xff\xd8" + rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() + b"\xff\xd9"
                for n in (5, 8, 1, 0, 300, 77, 2)]
    queue = iter(payloads)
    monkeypatch.setattr(V.AviWriter, "encode", lambda self, frame: next(queue))
    with V.AviWriter(str(tmp_path / "w.avi"), 25, 4, 4) as vid:
        vid.write(np.zeros((len(payloads), 4, 4, 3), np.uint8))
    want = open(str(tmp_path / "w.avi"), "rb").read()
    for name, splits in (("one", []), ("some", [1, 4, 6]), ("each", [1, 2, 3, 4, 5, 6]), ("empty", [0, 3, 3])):
        with V.AviWriter(str(tmp_path / (name + ".avi")), 25, 4, 4) as vid:
            for a, b in zip([0] + splits, splits + [len(payloads)]):
                assert vid.write_encoded(payloads[a:b]) is vid
        assert open(str(tmp_path / (name + ".avi")), "rb").read() == want, name
    assert R.parse_avi(str(tmp_path / "one.avi"))["frames"] == payloads


def test_write_encoded_refuses_what_is_not_a_jpeg_stream(tmp_path):
    from music2dance_amd import visualize as V
    good = b"\xff\xd8\x01\x02\xff\xd9"
    with V.AviWriter(str(tmp_path / "r.avi"), 25, 4, 4) as vid:
        for bad in (good[2:], good[:-2], b"", b"\xff\xd8", "text", None, good[:-1] + b"\xd8"):
            with pytest.raises(ValueError):
                vid.write_encoded([good, bad])
        vid.write_encoded([good])
    assert R.parse_avi(str(tmp_path / "r.avi"))["frames"] == [good]   # a refused call appends nothing
    with pytest.raises(ValueError):
        vid.write_encoded([good])                                       # closed


# ------------------------------------------------------------------------------------------- frame_to_vid on stand-ins
class StandIns:
    """the two device seams of visualize replaced by the numpy rules; the rule's encodings are kept per distinct
    frame, so a dance that alternates between two poses costs two encodings"""

    def __init__(self):
        self.render_calls, self.encode_calls, self.cache = [], [], {}

    def render(self, part, height, width, stats):
        self.render_calls.append(len(part))
        p = np.asarray(part, dtype=np.float32).reshape(len(part), -1)
        distinct, inverse = np.unique(p, axis=0, return_inverse=True)
        return torch.from_numpy(R.render(distinct, height, width)[inverse.reshape(-1)])

    def rule(self, frame, qtabs):
        key = (frame.tobytes(), frame.shape, tuple(map(tuple, qtabs)))
        if key not in self.cache:
            self.cache[key] = J.encode(frame, qtabs=[list(t) for t in qtabs])[0]
        return self.cache[key]

    def encode(self, frames, qtabs, capacity):
        self.encode_calls.append((len(frames), capacity))
        streams = [self.rule(f, qtabs) for f in frames.numpy()]
        offsets = torch.from_numpy(np.cumsum([0] + [len(s) for s in streams]).astype(np.int64))
        out = torch.full((capacity,), 0x5A, dtype=torch.uint8)
        if int(offsets[-1]) <= capacity:   # as the entry point: nothing is written when the streams do not fit
            out[:int(offsets[-1])] = torch.frombuffer(bytearray(b"".join(streams)), dtype=torch.uint8)
        return out, offsets


@pytest.fixture
def seams(monkeypatch):
    from music2dance_amd import visualize as V
    s = StandIns()
    monkeypatch.setattr(V, "_render_device", s.render)
    monkeypatch.setattr(V, "_encode_device", s.encode)
    return s


def two_pose_dance(n, seed=3):
    return stick_poses(2, seed)[np.arange(n) % 3 % 2]


def test_frame_to_vid_hip_on_the_rules(tmp_path, seams):
    from music2dance_amd import visualize as V
    poses = two_pose_dance(300)
    keep = poses.copy()
    stats = V.frame_to_vid(poses, str(tmp_path / "h.avi"), 25, encoder="hip")
    assert np.array_equal(poses, keep)
    assert seams.render_calls == [256, 44]
    assert seams.encode_calls == [(256, 256 * 270000), (44, 44 * 270000)]
    assert set(stats) == {"frames", "render_ms", "d2h_s", "encode_s", "mux_s", "wall_s", "encoder", "encode_ms"}
    assert stats["frames"] == 300 and stats["encoder"] == "hip" and stats["d2h_s"] > 0 and stats["wall_s"] > 0
    avi = R.parse_avi(str(tmp_path / "h.avi"))
    assert len(avi["frames"]) == 300 and (avi["strf"]["width"], avi["strf"]["height"]) == (300, 300)
    frames = R.render(poses[:2], 300, 300)
    want = [J.encode(f, 95)[0] for f in frames]
    assert avi["frames"] == [want[i % 3 % 2] for i in range(300)]


def test_unknown_encoder_raises_before_a_file_exists(tmp_path, seams):
    from music2dance_amd import visualize as V
    with pytest.raises(ValueError, match="nope"):
        V.frame_to_vid(two_pose_dance(3), str(tmp_path / "n.avi"), 25, encoder="nope")
    assert not os.path.exists(str(tmp_path / "n.avi")) and seams.render_calls == [] and seams.encode_calls == []


def test_default_encoder_never_reaches_the_seams(tmp_path, seams, monkeypatch):
    from music2dance_amd import visualize as V
    calls = []

    def render_host(part, height, width, stats):
        calls.append(len(part))
        return R.render(np.asarray(part), height, width)
    monkeypatch.setattr(V, "_render_host", render_host)
    stats = V.frame_to_vid(two_pose_dance(2), str(tmp_path / "p.avi"), 25)
    assert calls == [2] and seams.render_calls == [] and seams.encode_calls == []
    assert stats["encoder"] == "pil" and stats["encode_ms"] == 0.0 and stats["encode_s"] > 0
    with V.AviWriter(str(tmp_path / "w.avi"), 25, 300, 300) as vid:
        vid.write(R.render(two_pose_dance(2), 300, 300))
    assert open(str(tmp_path / "p.avi"), "rb").read() == open(str(tmp_path / "w.avi"), "rb").read()


def test_overflow_retries_once_with_the_reported_need(seams):
    from music2dance_amd import visualize as V
    frames = np.random.default_rng(8).integers(0, 256, (2, 33, 50, 3), dtype=np.uint8)
    stats = {}
    got = V.encode_jpeg(torch.from_numpy(frames), 100, stats)
    want = [J.encode(f, 100)[0] for f in frames]
    need = sum(len(w) for w in want)
    assert need > frames.size                                   # noise at quality 100 outgrows its raw bytes
    assert seams.encode_calls == [(2, frames.size), (2, need)]
    assert got == want and set(stats) == {"encode_ms", "d2h_s", "encode_s"}
    # streams that fit take one call
    seams.encode_calls.clear()
    flat = np.full((3, 9, 17, 3), 200, np.uint8)
    big = np.concatenate([flat] * 8, axis=1)
    assert V.encode_jpeg(torch.from_numpy(big), 95) == [J.encode(f, 95)[0] for f in big]
    assert seams.encode_calls == [(3, big.size)]


# ------------------------------------------------------------------------------------------------------ command lines
def test_visualize_cli_reaches_the_hip_encoder(tmp_path, seams):
    from music2dance_amd import visualize as V
    np.save(str(tmp_path / "p.npy"), two_pose_dance(5))
    stats = V.main([str(tmp_path / "p.npy"), str(tmp_path / "p.avi"), "--encoder", "hip"])
    assert stats["encoder"] == "hip" and seams.render_calls == [5] and [n for n, _ in seams.encode_calls] == [5]
    assert len(R.parse_avi(str(tmp_path / "p.avi"))["frames"]) == 5
    assert V.parse_args(["a.npy", "a.avi"]).encoder == "pil"
    with pytest.raises(SystemExit):
        V.parse_args(["a.npy", "a.avi", "--encoder", "cv2"])


def test_generate_cli_parses_the_encoder():
    from music2dance_amd.phase3 import generate as G
    base = ["-c", "x.yaml", "-l", "logs", "--synthetic", "--video"]
    assert G.parse_args(base).encoder is None
    assert G.parse_args(base + ["--encoder", "hip"]).encoder == "hip"
    assert G.parse_args(base + ["--encoder", "pil"]).encoder == "pil"
    with pytest.raises(SystemExit):
        G.parse_args(base + ["--encoder", "cv2"])
