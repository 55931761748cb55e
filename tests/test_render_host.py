"""Stick-figure videos on the host: the drawing rule's numpy statement (tests/render_rule.py) on cases counted by hand,
the AVI 1.0 MJPG writer (structure, padding, chunked writes, empty files, the 2 GiB refusal, decodable payloads) and
the command line with a stand-in renderer. No GPU."""
import io
import os

import numpy as np
import pytest
import torch

from tests import render_rule as R


def lone(x, y, joint=0):
    f = np.full((R.N_JOINTS, 3), np.nan, dtype=np.float32)
    f[joint] = (x, y, 0.0)
    return f


def test_a_lone_valid_joint_covers_49_pixels():
    cov = R.coverage(lone(0.3, -2.7, joint=5), 300, 300)
    assert cov.sum() == 49
    # its centre: x' = 150.3 -> 150, y' = 147.3 -> 147
    assert cov[147, 150] and cov[147, 154] and not cov[147, 155] and cov[151, 150] and not cov[151, 151]


def test_segment_counts():
    cov = np.zeros((50, 50), dtype=bool)
    R.cover_segment(cov, (10, 20), (20, 20))
    assert cov.sum() == 35   # 11 x 3 along the segment + one cap pixel at each end
    cov[:] = False
    R.cover_segment(cov, (7, 7), (7, 7))
    assert cov.sum() == 5
    cov[:] = False
    R.cover_segment(cov, (20, 10), (20, 20))   # vertical: the same count
    assert cov.sum() == 35


def test_negative_fractional_coordinates_truncate_toward_zero():
    px, py, v = R.points(lone(-150.5, -150.25), 300, 300)   # x' = -0.5, y' = -0.25
    assert v[0] and px[0] == 0 and py[0] == 0                # trunc, not floor (-1)
    px, py, v = R.points(lone(-151.5, 10.0), 300, 300)
    assert px[0] == -1 and py[0] == 160
    img = R.render(lone(-150.5, -150.25)[None], 300, 300)[0]
    # the disk around (0, 0), flipped: pixel height 0..4 are image rows 299..295
    assert (img[299, 0] == (0, 0, 255)).all() and (img[295, 0] == (0, 0, 255)).all() and (img[294, 0] == 255).all()


def test_invalid_joints_cancel_their_segments_and_midpoints():
    f = np.zeros((R.N_JOINTS, 3), dtype=np.float32)
    f[:, 0] = np.linspace(-100, 100, R.N_JOINTS)
    f[:, 1] = np.linspace(-80, 90, R.N_JOINTS)
    full = R.coverage(f, 300, 300)
    g = f.copy()
    g[3, 0] = np.inf                       # joint 3: its disk, (3, 4) and every segment to mid(3, 12) go
    _, _, v = R.points(g, 300, 300)
    assert not v[3] and not v[24] and v[23] and v[25]
    part = R.coverage(g, 300, 300)
    assert part.sum() < full.sum() and not (part & ~full).any()
    h = f.copy()
    h[7, 1] = 2.0 ** 14                    # beyond the limit: invalid as well
    assert not R.points(h, 300, 300)[2][7]


def test_float64_poses_are_rounded_to_fp32_first():
    f = lone(0.0, 0.0).astype(np.float64)
    f[0, 0] = 0.99999999                   # rounds to 1.0 in fp32: pixel 151, not 150
    assert R.points(f, 300, 300)[0][0] == 151


# ---------------------------------------------------------------------------------------------------------- AVI writer
def stick_frames(n, h=300, w=300, seed=0):
    rng = np.random.default_rng(seed)
    poses = rng.uniform(-120, 120, size=(n, R.N_JOINTS, 3)).astype(np.float32)
    return R.render(poses, h, w)


def write(path, frames, fps=25, splits=None, h=300, w=300, **kw):
    from music2dance_amd import visualize as V
    with V.AviWriter(str(path), fps, h, w, **kw) as vid:
        if splits is None:
            vid.write(frames)
        else:
            for a, b in zip([0] + splits, splits + [len(frames)]):
                vid.write(frames[a:b])
    return open(str(path), "rb").read()


@pytest.mark.parametrize("fps,rate,scale", [(25, 25, 1), (29.97, 2997, 100)])
def test_avi_structure(tmp_path, fps, rate, scale):
    frames = stick_frames(5, 96, 128)
    write(tmp_path / "a.avi", frames, fps, h=96, w=128)
    avi = R.parse_avi(str(tmp_path / "a.avi"))
    a, s, f = avi["avih"], avi["strh"], avi["strf"]
    assert a["total_frames"] == 5 and a["streams"] == 1 and a["flags"] & 0x10
    assert a["width"] == 128 and a["height"] == 96
    assert a["us_per_frame"] == round(1e6 * scale / rate)
    biggest = max(len(p) for p in avi["frames"])
    assert a["suggested_buffer"] == s["suggested_buffer"] == biggest + 8
    assert s["type"] == b"vids" and s["handler"] == b"MJPG" and (s["rate"], s["scale"]) == (rate, scale)
    assert s["length"] == 5 and s["frame"] == (0, 0, 128, 96)
    assert f["size"] == 40 and (f["width"], f["height"]) == (128, 96) and f["planes"] == 1 and f["bits"] == 24
    assert f["compression"] == b"MJPG" and f["image_bytes"] == 128 * 96 * 3
    assert len(avi["frames"]) == 5 and all(fl == 0x10 for fl, _, _ in avi["index"])
    assert all(p[:2] == b"\xff\xd8" and p[-2:] == b"\xff\xd9" for p in avi["frames"])


def test_odd_payloads_are_padded(tmp_path, monkeypatch):
    from music2dance_amd import visualize as V
    sizes = iter([7, 10, 1])
    monkeypatch.setattr(V.AviWriter, "encode", lambda self, fr: b"\xab" * next(sizes))
    write(tmp_path / "o.avi", np.zeros((3, 4, 4, 3), np.uint8), h=4, w=4)
    avi = R.parse_avi(str(tmp_path / "o.avi"))   # checks the zero pad bytes and that idx1 still lands
    assert [len(p) for p in avi["frames"]] == [7, 10, 1]
    assert [n for _, _, n in avi["index"]] == [7, 10, 1]
    assert [off for _, off, _ in avi["index"]] == [4, 4 + 8 + 8, 4 + 16 + 18]


def test_chunked_writes_give_the_same_bytes(tmp_path):
    frames = stick_frames(7, 64, 80, seed=3)
    one = write(tmp_path / "one.avi", frames, h=64, w=80)
    assert write(tmp_path / "split.avi", frames, splits=[1, 4, 6], h=64, w=80) == one
    assert write(tmp_path / "each.avi", frames, splits=[1, 2, 3, 4, 5, 6], h=64, w=80) == one
    assert write(tmp_path / "torch.avi", torch.from_numpy(frames), h=64, w=80) == one


def test_zero_frames_give_a_valid_file(tmp_path):
    write(tmp_path / "z.avi", np.zeros((0, 300, 300, 3), np.uint8))
    avi = R.parse_avi(str(tmp_path / "z.avi"))
    assert avi["frames"] == [] and avi["avih"]["total_frames"] == 0 and avi["strh"]["length"] == 0


def test_refuses_to_grow_past_the_limit(tmp_path, monkeypatch):
    from music2dance_amd import visualize as V
    frames = stick_frames(4, 64, 64)
    size = len(write(tmp_path / "full.avi", frames, h=64, w=64))
    monkeypatch.setattr(V, "MAX_FILE_BYTES", size - 1)
    with pytest.raises(OverflowError, match="AVI 1.0"):
        write(tmp_path / "big.avi", frames, h=64, w=64)
    monkeypatch.setattr(V, "MAX_FILE_BYTES", size)
    assert len(write(tmp_path / "fits.avi", frames, h=64, w=64)) == size


def test_writer_rejects_bad_frames(tmp_path):
    from music2dance_amd import visualize as V
    with V.AviWriter(str(tmp_path / "x.avi"), 25, 8, 8) as vid:
        with pytest.raises(ValueError):
            vid.write(np.zeros((1, 8, 9, 3), np.uint8))
        with pytest.raises(ValueError):
            vid.write(np.zeros((1, 8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        V.AviWriter(str(tmp_path / "y.avi"), 0, 8, 8)


def test_payloads_decode_to_the_frames(tmp_path):
    from PIL import Image
    frames = stick_frames(6, seed=11)
    write(tmp_path / "d.avi", frames)
    avi = R.parse_avi(str(tmp_path / "d.avi"))
    for want, payload in zip(frames, avi["frames"]):
        got = np.asarray(Image.open(io.BytesIO(payload)).convert("RGB")).astype(np.int32)
        err = np.abs(got - want.astype(np.int32))
        assert err.mean() <= 1.0 and err.max() <= 48, (err.mean(), err.max())
        fig_want = want[..., 2].astype(np.int32) - want[..., 0] > 128
        fig_got = got[..., 2] - got[..., 0] > 128
        assert (fig_want == fig_got).all()


# -------------------------------------------------------------------------------------------------------- command line
@pytest.fixture
def stand_in(monkeypatch):
    """frame_to_vid with the numpy rule in place of the device renderer"""
    from music2dance_amd import visualize as V
    calls = []

    def render_host(part, height, width, stats):
        calls.append(len(part))
        return R.render(np.asarray(part), height, width)
    monkeypatch.setattr(V, "_render_host", render_host)
    return calls


def test_cli_renders_a_saved_file(tmp_path, stand_in):
    from music2dance_amd import visualize as V
    rng = np.random.default_rng(5)
    poses = rng.uniform(-100, 100, size=(300, R.N_JOINTS, 3)).astype(np.float32)
    np.save(str(tmp_path / "p.npy"), poses)
    keep = poses.copy()
    out = tmp_path / "sub" / "p.avi"
    stats = V.main([str(tmp_path / "p.npy"), str(out), "--fps", "29.97"])
    assert stand_in == [256, 44] and stats["frames"] == 300
    avi = R.parse_avi(str(out))
    assert len(avi["frames"]) == 300 and (avi["strh"]["rate"], avi["strh"]["scale"]) == (2997, 100)
    assert (avi["strf"]["width"], avi["strf"]["height"]) == (300, 300)
    # the default rate, and (T, 69) input
    np.save(str(tmp_path / "q.npy"), poses[:3].reshape(3, 69))
    V.main([str(tmp_path / "q.npy"), str(tmp_path / "q.avi")])
    avi = R.parse_avi(str(tmp_path / "q.avi"))
    assert len(avi["frames"]) == 3 and (avi["strh"]["rate"], avi["strh"]["scale"]) == (25, 1)
    assert np.array_equal(np.load(str(tmp_path / "p.npy")), keep)


def test_cli_rejects_bad_arguments(tmp_path, stand_in):
    from music2dance_amd import visualize as V
    with pytest.raises(SystemExit):
        V.parse_args([])
    with pytest.raises(SystemExit):
        V.parse_args(["only.npy"])
    np.save(str(tmp_path / "bad.npy"), np.zeros((4, 22, 3), np.float32))
    with pytest.raises(SystemExit):
        V.main([str(tmp_path / "bad.npy"), str(tmp_path / "bad.avi")])
    np.save(str(tmp_path / "ok.npy"), np.zeros((4, 23, 3), np.float32))
    with pytest.raises(SystemExit):
        V.main([str(tmp_path / "ok.npy"), str(tmp_path / "ok.avi"), "--fps", "0"])
    assert stand_in == [] and not os.path.exists(str(tmp_path / "bad.avi"))


def test_frame_to_vid_leaves_its_input_alone(tmp_path, stand_in):
    from music2dance_amd import visualize as V
    frames = torch.linspace(-50, 50, 10 * 69).reshape(10, 23, 3).double()
    keep = frames.clone()
    V.frame_to_vid(frames, str(tmp_path / "t.avi"), 25)
    assert torch.equal(frames, keep) and stand_in == [10]


def test_rendering_without_a_device_fails_loudly(tmp_path, monkeypatch):
    from music2dance_amd import _lib
    from music2dance_amd import visualize as V
    with pytest.raises(_lib.M2dError):
        V.render(torch.zeros(2, 23, 3))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(_lib.M2dError):
        V.frame_to_vid(np.zeros((2, 23, 3), np.float32), str(tmp_path / "n.avi"), 25)
