"""m2d_jpeg_encode on the device against the numpy statement of the encoding rule (tests/jpeg_rule.py), byte for byte:
block edges, the capacity retry, input alignment, canaries behind the offsets and the streams, determinism, stream
ordering, argument checks, and frame_to_vid / `phase3.generate --video` with encoder="hip" end to end."""
import io
import json
import os

import numpy as np
import pytest
import torch

from tests import jpeg_rule as J
from tests import render_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NOISE_SEED = 3955   # tests/test_jpeg_host.py asserts what this seed's 33 x 50 frame exercises


def kern():
    from music2dance_amd import kernels
    return kernels.impl()


def settle():
    torch.cuda.synchronize()
    kern().check_async_errors()


def random_poses(n, spread, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, size=(n, R.N_JOINTS, 3)).astype(np.float32)


def noise(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def device_encode(frames, quality):
    from music2dance_amd import visualize as V
    got = V.encode_jpeg(torch.from_numpy(np.array(frames)).to(DEV), quality)
    settle()
    return got


def assert_streams(got, frames, quality, what):
    assert len(got) == len(frames), (what, len(got), len(frames))
    for i, (g, f) in enumerate(zip(got, frames)):
        want = J.encode(f, quality)[0]
        if g != want:
            first = next((k for k, (a, b) in enumerate(zip(g, want)) if a != b), min(len(g), len(want)))
            raise AssertionError("%s: frame %d differs from the rule at byte %d (%d bytes, rule %d)"
                                 % (what, i, first, len(g), len(want)))


@pytest.fixture(scope="module")
def sticks300():
    """five 300 x 300 stick frames (numpy rule), shared and never modified"""
    frames = R.render(random_poses(5, 120, seed=0), 300, 300)
    frames.setflags(write=False)
    return frames


@pytest.mark.parametrize("n,h,w,quality", [(3, 8, 8, 95), (2, 9, 17, 95), (2, 16, 24, 50), (1, 1, 1, 95)])
def test_small_shapes_bit_exact(n, h, w, quality):
    frames = noise(n, h, w, seed=100 * h + w)
    assert_streams(device_encode(frames, quality), frames, quality, "noise %dx%d" % (h, w))
    flat = np.full((n, h, w, 3), 255, np.uint8)   # every block takes the one-colour path
    flat[-1] = (12, 200, 77)
    assert_streams(device_encode(flat, quality), flat, quality, "flat %dx%d" % (h, w))


def test_noise_at_quality_100_takes_the_capacity_retry(monkeypatch):
    from music2dance_amd import visualize as V
    # the first frame is the host test's: ZRL, stuffing, blocks without EOB
    frames = np.concatenate([noise(1, 33, 50, NOISE_SEED), noise(1, 33, 50, NOISE_SEED + 1)])
    caps = []
    real = V._encode_device

    def counting(fr, qtabs, capacity):
        caps.append(capacity)
        return real(fr, qtabs, capacity)
    monkeypatch.setattr(V, "_encode_device", counting)
    got = device_encode(frames, 100)
    assert_streams(got, frames, 100, "noise 33x50")
    assert caps == [frames.size, sum(len(g) for g in got)] and caps[1] > caps[0]


@pytest.mark.parametrize("n,h,w,quality", [
    (1, 16, 300, 100),    # 38 blocks a row, one wave a row: each row's stream passes through the LDS buffer in pieces
    (2, 8, 520, 95),      # 65 blocks a row: the wide workgroup
    (1, 9, 2056, 100),    # 257 blocks a row: two blocks a thread, several pieces
    (1, 2056, 9, 95),     # 257 rows of blocks: two rows a thread in the row-offset scan
])
def test_long_rows_and_many_rows_bit_exact(n, h, w, quality):
    frames = noise(n, h, w, seed=h + w)
    assert_streams(device_encode(frames, quality), frames, quality, "noise %dx%d" % (h, w))


def test_stick_frames_bit_exact(sticks300):
    assert_streams(device_encode(sticks300, 95), sticks300, 95, "sticks 300x300")


def test_more_frames_than_a_workgroup_has_lanes():
    n = 300
    frames = R.render(random_poses(n, 14, seed=7), 32, 32)
    got = device_encode(frames, 95)
    assert_streams(got, frames, 95, "300 frames of 32x32")


def test_no_frames():
    from music2dance_amd import visualize as V
    assert V.encode_jpeg(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=DEV)) == []
    out, offsets = kern().jpeg_encode(torch.empty((0, 300, 300, 3), dtype=torch.uint8, device=DEV), J.quant_tables(95))
    settle()
    assert out.numel() == 0 and offsets.tolist() == [0]


@pytest.mark.parametrize("offset", [1, 4, 15])
def test_input_alignment(offset):
    n, h, w = 3, 16, 24   # the middle frame's rows all lie inside the input: every block takes the dword loads
    frames = noise(n, h, w, seed=offset)
    total = frames.size
    buf = torch.zeros((64 + total + 64,), dtype=torch.uint8, device=DEV)
    view = buf[offset:offset + total].view(n, h, w, 3)
    view.copy_(torch.from_numpy(frames).to(DEV))
    assert view.data_ptr() % 16 == offset
    from music2dance_amd import visualize as V
    got = V.encode_jpeg(view, 95)
    settle()
    assert_streams(got, frames, 95, "input at +%d" % offset)


def raw_encode(frames, quality, capacity, guard=64):
    """the entry point itself on buffers with canaries -> (rc, out bytes incl. guard, offsets incl. guard)"""
    from music2dance_amd import _lib
    h = _lib.lib()
    n, H, W = frames.shape[:3]
    x = torch.from_numpy(frames).to(DEV)
    out = torch.full((capacity + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    offsets = torch.full((n + 1 + 8,), -77, dtype=torch.int64, device=DEV)
    nws = h.m2d_jpeg_workspace_bytes(n, H, W)
    ws = torch.empty((nws + 3) // 4, dtype=torch.float32, device=DEV)
    q = bytes(v for t in J.quant_tables(quality) for v in t)
    rc = h.m2d_jpeg_encode(x.data_ptr(), n, H, W, q, out.data_ptr(), capacity, offsets.data_ptr(), ws.data_ptr(),
                           ws.numel() * 4, torch.cuda.current_stream().cuda_stream)
    settle()
    return rc, out.cpu().numpy(), offsets.cpu().numpy()


def test_canaries_and_capacity():
    frames = noise(3, 17, 26, seed=5)
    want = [J.encode(f, 90)[0] for f in frames]
    need = sum(len(w) for w in want)
    for capacity in (need + 100, need):
        rc, out, off = raw_encode(frames, 90, capacity)
        assert rc == 0
        assert off[:4].tolist() == np.cumsum([0] + [len(w) for w in want]).tolist() and (off[4:] == -77).all()
        assert out[:need].tobytes() == b"".join(want)
        assert (out[need:] == 0x5A).all()      # nothing behind offsets[n], nothing behind the capacity
    for capacity in (need - 1, 700, 0):        # too small: the need is reported, no byte is written
        rc, out, off = raw_encode(frames, 90, capacity)
        assert rc == 0 and off[3] == need and (off[4:] == -77).all()
        assert (out == 0x5A).all()


def test_two_runs_give_the_same_bytes(sticks300):
    x = torch.from_numpy(np.concatenate([sticks300[:2], noise(1, 300, 300, 9)])).to(DEV)
    q = J.quant_tables(95)
    a_out, a_off = kern().jpeg_encode(x, q)
    b_out, b_off = kern().jpeg_encode(x, q)
    settle()
    assert torch.equal(a_off, b_off)
    used = int(a_off[-1])
    assert used <= a_out.numel() and torch.equal(a_out[:used], b_out[:used])


def test_side_stream_after_the_render_event():
    n = 64
    base = torch.from_numpy(random_poses(n, 140, seed=31)).to(DEV)
    q = J.quant_tables(95)
    frames = kern().render_sticks((base * 0.5).contiguous().reshape(n, 69), 300, 300)
    w_out, w_off = kern().jpeg_encode(frames, q)
    settle()
    used = int(w_off[-1])
    side = torch.cuda.Stream()
    main = torch.cuda.current_stream()
    for _ in range(3):
        torch.cuda._sleep(2_000_000)   # keep the producer behind the host
        frames = kern().render_sticks((base * 0.5).reshape(n, 69), 300, 300)   # rendered on the main stream
        done = torch.cuda.Event()
        done.record(main)
        with torch.cuda.stream(side):
            side.wait_event(done)
            out, off = kern().jpeg_encode(frames, q)
        main.wait_stream(side)
        frames.record_stream(side)
        out.record_stream(main)
        off.record_stream(main)
        assert torch.equal(off, w_off) and torch.equal(out[:used], w_out[:used])
    settle()


def test_captured_launches_replay_on_new_frames():
    first, second = noise(2, 16, 24, seed=61), noise(2, 16, 24, seed=62)
    x = torch.from_numpy(first).to(DEV)
    q = J.quant_tables(75)
    cap = 4 * first.size
    kern().jpeg_encode(x, q, cap)   # outside the capture: the stream's first launch
    settle()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, off = kern().jpeg_encode(x, q, cap)
    for frames in (first, second):
        x.copy_(torch.from_numpy(frames).to(DEV))
        graph.replay()
        settle()
        o, data = off.tolist(), out.cpu().numpy().tobytes()
        assert_streams([data[o[i]:o[i + 1]] for i in range(2)], frames, 75, "replayed graph")


def test_arguments_are_checked():
    from music2dance_amd import _lib
    k = kern()
    q = J.quant_tables(95)
    x = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(x.cpu(), q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(x.float(), q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device=DEV)[:, :, ::2], q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(torch.zeros((2, 8, 8, 4), dtype=torch.uint8, device=DEV), q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(torch.zeros((1, 4097, 1, 3), dtype=torch.uint8, device=DEV), q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(torch.zeros((1, 1, 4097, 3), dtype=torch.uint8, device=DEV), q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(torch.zeros((1, 0, 8, 3), dtype=torch.uint8, device=DEV), q)
    with pytest.raises(_lib.M2dError):
        k.jpeg_encode(x, ([0] * 64, [1] * 64))
    h = _lib.lib()
    qb = bytes(v for t in q for v in t)
    o = torch.zeros(8, dtype=torch.int64, device=DEV)
    ws = torch.zeros(4096, dtype=torch.float32, device=DEV)
    p = x.data_ptr()
    assert 2 * 384 <= h.m2d_jpeg_workspace_bytes(2, 8, 8) <= 2 * 384 + 256   # the coefficients and a few small arrays
    assert h.m2d_jpeg_workspace_bytes(2, 0, 8) == 0 and h.m2d_jpeg_workspace_bytes(2, 8, 4097) == 0
    assert h.m2d_jpeg_encode(p, -1, 8, 8, qb, p, 10, o.data_ptr(), ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(p, 2, 0, 8, qb, p, 10, o.data_ptr(), ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(p, 2, 8, 4097, qb, p, 10, o.data_ptr(), ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(p, 2, 8, 8, qb, p, -1, o.data_ptr(), ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(0, 2, 8, 8, qb, p, 10, o.data_ptr(), ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(p, 2, 8, 8, qb, p, 10, 0, ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(p, 2, 8, 8, bytes(128), p, 10, o.data_ptr(), ws.data_ptr(), 16384, None) == -1
    assert h.m2d_jpeg_encode(p, 2, 8, 8, qb, p, 10, o.data_ptr(), ws.data_ptr(), 100, None) == -3
    assert h.m2d_jpeg_encode(0, 0, 8, 8, None, 0, 0, 0, 0, 0, None) == 0
    settle()
    assert (x == 0).all() and (o == 0).all()


def decoded(payload):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(payload)).convert("RGB")).astype(np.int32)


def test_frame_to_vid_hip_end_to_end(tmp_path):
    from music2dance_amd import visualize as V
    T = 300
    poses = random_poses(T, 110, seed=41)
    stats = V.frame_to_vid(poses, str(tmp_path / "h.avi"), 25, encoder="hip")
    settle()
    assert stats["frames"] == T and stats["encoder"] == "hip"
    assert stats["render_ms"] > 0 and stats["encode_ms"] > 0 and stats["d2h_s"] > 0
    avi = R.parse_avi(str(tmp_path / "h.avi"))
    assert len(avi["frames"]) == T and avi["avih"]["total_frames"] == T
    # every payload equals the device encoding of the device rendering; the rule is Python loops, so it is applied
    # to a sample that holds both ends of both chunks
    frames = V.render(torch.from_numpy(poses).to(DEV), 300, 300)
    assert V.encode_jpeg(frames, 95) == avi["frames"]
    idx = [0, 1, 131, 255, 256, 299]
    want = R.render(poses[idx], 300, 300)
    assert_streams([avi["frames"][i] for i in idx], want, 95, "frame_to_vid payloads")
    ref = frames.cpu().numpy().astype(np.int32)
    worst_mae = worst_max = 0
    for f, payload in zip(ref, avi["frames"]):
        got = decoded(payload)
        err = np.abs(got - f)
        worst_mae, worst_max = max(worst_mae, err.mean()), max(worst_max, err.max())
        assert ((f[..., 2] - f[..., 0] > 128) == (got[..., 2] - got[..., 0] > 128)).all()
    assert worst_mae <= 1.0 and worst_max <= 48, (worst_mae, worst_max)


def test_default_encoder_keeps_its_bytes(tmp_path):
    from music2dance_amd import visualize as V
    T = 40
    poses = random_poses(T, 110, seed=43)
    stats = V.frame_to_vid(poses, str(tmp_path / "p.avi"), 25)
    assert stats["encoder"] == "pil" and stats["encode_ms"] == 0.0 and stats["encode_s"] > 0
    frames = V.render(torch.from_numpy(poses).to(DEV), 300, 300).cpu().numpy()
    with V.AviWriter(str(tmp_path / "w.avi"), 25, 300, 300) as vid:
        vid.write(frames)
    assert open(str(tmp_path / "p.avi"), "rb").read() == open(str(tmp_path / "w.avi"), "rb").read()


def test_generate_video_with_the_hip_encoder(tmp_path):
    from music2dance_amd.phase3 import generate as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = os.path.join(root, "music2dance_amd", "phase3", "configs", "default.yaml")
    G.main(["-c", cfg, "-l", str(tmp_path), "--synthetic", "--seed", "3", "--video", "--encoder", "hip"])
    settle()
    with open(str(tmp_path / "samples" / "generation.json")) as f:
        (v,) = json.load(f)["tracks"]
    assert v["encoder"] == "hip" and v["video"] == str(tmp_path / "samples" / "synthetic.avi")
    saved = np.load(str(tmp_path / "samples" / "synthetic.npy"))
    avi = R.parse_avi(v["video"])
    assert len(avi["frames"]) == saved.shape[0] == v["frames"]
    assert_streams(avi["frames"][:1], R.render(saved[:1], 300, 300), 95, "generate --encoder hip")
