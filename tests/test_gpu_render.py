"""m2d_render_sticks on the device against the numpy statement of the drawing rule (tests/render_rule.py), bit for bit;
that it writes exactly its output bytes; stream ordering; frame_to_vid end to end and `phase3.generate --video`."""
import json
import os

import numpy as np
import pytest
import torch

from tests import render_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def kern():
    from music2dance_amd import kernels
    return kernels.impl()


def random_poses(n, spread=160.0, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-spread, spread, size=(n, R.N_JOINTS, 3)).astype(np.float32)


def device_render(poses, h, w):
    from music2dance_amd import visualize as V
    out = V.render(torch.from_numpy(np.ascontiguousarray(poses)).to(DEV), h, w)
    torch.cuda.synchronize()
    kern().check_async_errors()
    return out.cpu().numpy()


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((got != want).any(-1))
    assert len(bad) == 0, "%s: %d pixels differ, first (frame, row, col) %s" % (what, len(bad), bad[:5].tolist())


@pytest.mark.parametrize("h,w", [(300, 300), (64, 200), (200, 64), (1, 1)])
def test_random_poses_bit_exact(h, w):
    poses = random_poses(64, spread=0.6 * max(h, w), seed=h * 1000 + w)
    assert_same(device_render(poses, h, w), R.render(poses, h, w), "random %dx%d" % (h, w))


@pytest.mark.parametrize("n", [1, 7])
def test_edge_cases_bit_exact(n):
    H = W = 300
    cases = []
    # joints on the borders and corners (x' = 0, W-1; y' = 0, H-1) and segments leaving the canvas
    f = random_poses(1, 100, seed=1)[0]
    f[0, :2] = (-150, -150)
    f[1, :2] = (149, 149)
    f[2, :2] = (-150, 149)
    f[3, :2] = (149.99, -150)
    f[4, :2] = (400, 20)
    f[12, :2] = (-20, -700)
    cases.append(f)
    # coincident endpoints: every joint in one place, and pairs of joints on top of each other
    f = np.zeros((R.N_JOINTS, 3), np.float32)
    cases.append(f)
    f = random_poses(1, 60, seed=2)[0]
    f[1], f[13], f[20] = f[0], f[12], f[19]
    cases.append(f)
    # negative fractional coordinates near the canvas origin
    f = random_poses(1, 2.0, seed=3)[0] - np.float32(150.0)
    cases.append(f)
    # NaN and +-inf joints: only their own primitives vanish
    f = random_poses(1, 120, seed=4)[0]
    f[3, 0], f[10, 1], f[19, 0], f[7, 1] = np.nan, np.inf, -np.inf, np.nan
    cases.append(f)
    # coordinates beyond +-2^14 and just inside
    f = random_poses(1, 120, seed=5)[0]
    f[5, 0], f[12, 1], f[8, 0], f[16, 1] = 2.0 ** 14, -3e9, 16000.0, -16200.0
    f[9, :2] = (-16100.0, f[8, 1] + 3.3)   # segment (8, 9) spans 32 000 pixels across the canvas: the int64 test
    cases.append(f)
    # fractional values within an ulp of integers
    f = np.round(random_poses(1, 140, seed=6)[0]) - np.float32(1e-5)
    cases.append(f)
    assert len(cases) == 7
    for i in range(0, len(cases), n):   # n = 1: each case alone; n = 7: all in one launch
        batch = np.stack(cases[i:i + n])
        assert_same(device_render(batch, H, W), R.render(batch, H, W), "edge cases %d..%d" % (i, i + n))


def test_4500_frames_in_one_launch():
    n = 4500
    poses = random_poses(n, 140, seed=9)
    x = torch.from_numpy(poses).to(DEV)
    out = kern().render_sticks(x.reshape(n, 69), 300, 300)
    torch.cuda.synchronize()
    kern().check_async_errors()
    idx = np.sort(np.random.default_rng(10).choice(n, 32, replace=False))
    idx[-1] = n - 1
    got = out[torch.from_numpy(idx).to(DEV)].cpu().numpy()
    assert_same(got, R.render(poses[idx], 300, 300), "4500-frame launch")


@pytest.mark.parametrize("h,w,offset", [(300, 300, 0), (7, 5, 3), (1, 1, 1), (64, 200, 5)])
def test_writes_exactly_its_bytes(h, w, offset):
    n, guard = 9, 64
    poses = random_poses(n, 0.6 * max(h, w), seed=21)
    total = n * h * w * 3
    buf = torch.full((guard + offset + total + guard,), 0x5A, dtype=torch.uint8, device=DEV)
    out = buf[guard + offset:guard + offset + total].view(n, h, w, 3)   # misaligned for offset != 0
    kern().render_sticks(torch.from_numpy(poses).to(DEV), h, w, out=out)
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert (b[:guard + offset] == 0x5A).all() and (b[guard + offset + total:] == 0x5A).all()
    img = b[guard + offset:guard + offset + total].reshape(n, h, w, 3)
    assert set(np.unique(img).tolist()) <= {0, 255}
    assert_same(img, R.render(poses, h, w), "sentinel %dx%d+%d" % (h, w, offset))


def test_arguments_are_checked():
    from music2dance_amd import _lib
    k = kern()
    x = torch.zeros(2, 69, device=DEV)
    for h, w in ((0, 10), (10, 0), (4097, 10), (10, 4097)):
        with pytest.raises(_lib.M2dError):
            k.render_sticks(x, h, w)
    with pytest.raises(_lib.M2dError):
        k.render_sticks(x.double(), 10, 10)
    with pytest.raises(_lib.M2dError):
        k.render_sticks(torch.zeros(2, 68, device=DEV), 10, 10)
    with pytest.raises(_lib.M2dError):
        k.render_sticks(x, 10, 10, out=torch.empty(2, 10, 10, 3, dtype=torch.uint8))
    h = _lib.lib()
    assert h.m2d_render_sticks(x.data_ptr(), -1, 10, 10, x.data_ptr(), None) == -1
    assert h.m2d_render_sticks(0, 2, 10, 10, x.data_ptr(), None) == -1
    assert h.m2d_render_sticks(x.data_ptr(), 2, 10, 10, 0, None) == -1
    assert h.m2d_render_sticks(0, 0, 10, 10, 0, None) == 0
    assert tuple(k.render_sticks(torch.zeros(0, 23, 3, device=DEV), 10, 10).shape) == (0, 10, 10, 3)


def test_side_stream_after_the_producer_event():
    n = 300
    base = torch.from_numpy(random_poses(n, 140, seed=31)).to(DEV)
    want = kern().render_sticks((base * 0.5).contiguous(), 300, 300)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    main = torch.cuda.current_stream()
    for _ in range(3):
        torch.cuda._sleep(2_000_000)   # keep the producer behind the host
        poses = base * 0.5             # produced on the main stream
        done = torch.cuda.Event()
        done.record(main)
        with torch.cuda.stream(side):
            side.wait_event(done)
            got = kern().render_sticks(poses, 300, 300)
        main.wait_stream(side)
        poses.record_stream(side)
        got.record_stream(main)
        assert torch.equal(got, want)


def decoded(payload):
    import io
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(payload)).convert("RGB")).astype(np.int32)


def test_frame_to_vid_end_to_end(tmp_path):
    from music2dance_amd import visualize as V
    T = 300
    poses = random_poses(T, 110, seed=41).astype(np.float64)
    keep = poses.copy()
    stats = V.frame_to_vid(poses, str(tmp_path / "v.avi"), 25)
    assert np.array_equal(poses, keep)
    assert stats["frames"] == T and stats["render_ms"] > 0 and stats["encode_s"] > 0
    avi = R.parse_avi(str(tmp_path / "v.avi"))
    assert len(avi["frames"]) == T and avi["avih"]["total_frames"] == T
    assert (avi["strh"]["rate"], avi["strh"]["scale"]) == (25, 1)
    ref = device_render(poses.astype(np.float32), 300, 300)
    assert_same(ref, R.render(poses, 300, 300), "frame_to_vid frames")
    worst_mae = worst_max = 0
    for want, payload in zip(ref, avi["frames"]):
        got = decoded(payload)
        err = np.abs(got - want)
        worst_mae, worst_max = max(worst_mae, err.mean()), max(worst_max, err.max())
        assert ((want[..., 2] - want[..., 0] > 128) == (got[..., 2] - got[..., 0] > 128)).all()
    assert worst_mae <= 1.0 and worst_max <= 48, (worst_mae, worst_max)
    # device input, (T, 69): the same bytes
    V.frame_to_vid(torch.from_numpy(poses).to(DEV).reshape(T, 69), str(tmp_path / "d.avi"), 25)
    assert open(str(tmp_path / "d.avi"), "rb").read() == open(str(tmp_path / "v.avi"), "rb").read()


def test_generate_video(tmp_path):
    from music2dance_amd import visualize as V
    from music2dance_amd.phase3 import generate as G
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = os.path.join(root, "music2dance_amd", "phase3", "configs", "default.yaml")
    plain, vid = tmp_path / "plain", tmp_path / "vid"
    G.main(["-c", cfg, "-l", str(plain), "--synthetic", "--seed", "3"])
    res = G.main(["-c", cfg, "-l", str(vid), "--synthetic", "--seed", "3", "--video"])
    assert not os.path.exists(str(plain / "samples" / "synthetic.avi"))
    with open(str(plain / "samples" / "generation.json")) as f:
        (p,) = json.load(f)["tracks"]
    with open(str(vid / "samples" / "generation.json")) as f:
        (v,) = json.load(f)["tracks"]
    assert set(p) == {"name", "frames", "seconds", "chunk_frames", "real_time_factor", "wall_s", "chunks",
                      "gpu_ms_per_chunk_p50", "gpu_ms_per_chunk_p99"}
    assert set(v) == set(p) | {"video", "render_ms", "video_s"}
    assert v["video"] == str(vid / "samples" / "synthetic.avi") and v["render_ms"] > 0 and v["video_s"] > 0
    assert res["tracks"][0]["video"] == v["video"]
    saved = np.load(str(vid / "samples" / "synthetic.npy"))
    T = saved.shape[0]
    avi = R.parse_avi(v["video"])
    assert len(avi["frames"]) == T == v["frames"]
    again = str(tmp_path / "again.avi")
    V.frame_to_vid(saved, again, 25)
    assert R.parse_avi(again)["frames"] == avi["frames"]
