"""Host half of the on-device augmentation (data.Augment, data.augment_window, SequenceDataset(augment=); DESIGN.md
section 19; the device half is tests/test_gpu_augment.py): the fp64 rule against scipy.signal.resample_poly and
retime_sequence, its invariants (mirror twice, yaw keeps lengths and heights), the draws, the errors, and that nothing
changes with augment=None."""
import math
import re

import numpy as np
import pytest
import torch

from music2dance_amd import data as D
from tests import augment_cases as A

ROOT = A.__file__.rsplit("/tests/", 1)[0]


@pytest.fixture(scope="module")
def store():
    poses, tracks = A.takes()
    return poses, tracks, A.scaler(poses)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("speed", A.SPEEDS, ids=lambda s: "%dover%d" % s)
@pytest.mark.parametrize("where", ["first", "last"])
def test_audio_is_scipys_resample_poly_on_the_shifted_padded_take(store, speed, where):
    """windows at the first and the last admissible start of the middle take: the last one runs past the take's end
    at a speed above 1 only through the filter's tail - and reads zeros there, not take 2"""
    from scipy.signal import resample_poly  # noqa: F401 (the comparison needs scipy)
    poses, tracks, sc = store
    a, b = speed
    p0 = 0 if where == "first" else A.last_start(A.FRAMES[1], a, b)
    got = D.augment_window(poses[1], tracks[1], p0, A.T, A.S, A.HOP, A.params(a, b, gain=0.7), sc)[1]
    want = 0.7 * A.scipy_audio(tracks[1], p0 * A.HOP, A.S, a, b)
    # two fp64 dot products of P terms each, and the gain
    P = -(-len(D.speed_taps(a, b)) // b)
    bound = 2 * (P + 3) * 2.0 ** -53 * 0.7 * A.scipy_audio(tracks[1], p0 * A.HOP, A.S, a, b, absolute=True)
    assert got.shape == (A.S,) and np.all(np.abs(got - want) <= bound)
    assert np.abs(got).max() < 10.0     # nothing of the neighbours (values around 1e3) came in


def test_audio_outside_the_take_is_zero(store):
    poses, tracks, sc = store
    short = tracks[1][:A.HOP * 10]      # a track shorter than its poses: the window's tail is silence
    y = D.augment_window(poses[1], short, 5, A.T, A.S, A.HOP, A.params(), sc)[1]
    assert np.array_equal(y[:5 * A.HOP], short[5 * A.HOP:]) and not y[5 * A.HOP:].any()


def test_a_mirror_applied_twice_is_the_identity(store):
    poses, _, sc = store
    x = poses[2][:A.T]
    once = D.augment_window(x, None, 0, A.T, 0, A.HOP, A.params(mirror=True), sc)[0]
    twice = D.augment_window(once, None, 0, A.T, 0, A.HOP, A.params(mirror=True), sc)[0]
    # per pass: un-scale (2 roundings), re-scale (2) on values of size |v| + |shift|
    tol = 16 * 2.0 ** -53 * (np.abs(x).reshape(A.T, -1) + 2 * np.abs(sc.min_)).reshape(x.shape)
    assert np.all(np.abs(twice - x) <= tol) and not np.allclose(once, x)
    raw = sc.inverse_transform(x.reshape(A.T, -1)).reshape(x.shape)
    raw1 = sc.inverse_transform(once.reshape(A.T, -1)).reshape(x.shape)
    np.testing.assert_allclose(raw1[..., 0], -raw[..., 0], rtol=1e-12)
    np.testing.assert_allclose(raw1[..., 1:], raw[..., 1:], rtol=1e-12)


@pytest.mark.parametrize("deg", [37.0, -180.0, 90.0])
def test_a_yaw_keeps_every_joints_horizontal_radius_and_height(store, deg):
    poses, _, sc = store
    x = poses[0][3:3 + A.T]
    y = D.augment_window(poses[0], None, 3, A.T, 0, A.HOP, A.params(deg=deg), sc)[0]
    raw = sc.inverse_transform(x.reshape(A.T, -1)).reshape(x.shape)
    rot = sc.inverse_transform(y.reshape(A.T, -1)).reshape(x.shape)
    r2 = raw[..., 0] ** 2 + raw[..., 2] ** 2
    np.testing.assert_allclose(rot[..., 0] ** 2 + rot[..., 2] ** 2, r2, rtol=1e-12, atol=1e-12 * r2.max())
    np.testing.assert_allclose(rot[..., 1], raw[..., 1], rtol=1e-12, atol=1e-12 * np.abs(raw).max())
    th = math.radians(deg)   # x' = c x + s z, z' = -s x + c z
    np.testing.assert_allclose(rot[..., 0], math.cos(th) * raw[..., 0] + math.sin(th) * raw[..., 2], rtol=1e-11,
                               atol=1e-11 * np.abs(raw).max())


@pytest.mark.parametrize("speed", [(1, 1), (2, 1), (3, 11), (12, 11)], ids=lambda s: "%dover%d" % s)
def test_poses_equal_retime_sequence_where_the_recipes_coincide(store, speed):
    """(T - 1) a divisible by b: the window's last frame sits on a source frame, and retime_sequence over exactly the
    frames the window needs has the same positions i a / b"""
    poses, _, sc = store
    a, b = speed
    assert (A.T - 1) * a % b == 0
    need = D.frames_needed(A.T, a, b)
    assert need == (A.T - 1) * a // b + 1
    got = D.augment_window(poses[2], None, 4, A.T, 0, A.HOP, A.params(a, b), sc)[0]
    want = D.retime_sequence(poses[2][4:4 + need], A.T)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    if b == 1:
        assert np.array_equal(got, poses[2][4:4 + need:a])


def test_identity_parameters_return_the_window_itself(store):
    poses, tracks, sc = store
    p, y = D.augment_window(poses[1], tracks[1], 2, A.T, A.S, A.HOP, D.IDENTITY, sc)
    assert np.array_equal(p, poses[1][2:2 + A.T]) and np.array_equal(y, tracks[1][2 * A.HOP:2 * A.HOP + A.S])
    with pytest.raises(ValueError, match="do not fit"):
        D.augment_window(poses[1], None, 12, A.T, 0, A.HOP, D.IDENTITY, sc)


# ------------------------------------------------------------------------------------------------ the draws
FULL = {"mirror": 0.5, "yaw_deg": 180, "speeds": ["1/1", "24/25", "25/24", "9/10", "10/9"], "gain_db": 3, "seed": 5}


def test_draws_are_reproducible_and_take_four_uniforms_a_row_whatever_is_off():
    one, two = D.Augment(FULL).draw(6), D.Augment(FULL).draw(6)
    assert one == two and len({(p.a, p.b) for p in one}) > 1 and any(p.mirror for p in one)
    assert one != D.Augment(dict(FULL, seed=6)).draw(6)
    for p in one:
        assert abs(p.cos ** 2 + p.sin ** 2 - 1) < 1e-15 and 10 ** (-3 / 20) <= p.gain <= 10 ** (3 / 20)
    # draw(n) is n draws of one row
    aug = D.Augment(FULL)
    assert [aug.draw(1)[0] for _ in range(6)] == one
    # a configuration with everything off consumes the same stream and gives identity rows
    off = D.Augment({"seed": 5})
    assert off.draw(6) == [D.IDENTITY] * 6
    ref = np.random.Generator(np.random.PCG64(5))
    ref.random(24)
    assert off.rng.random() == ref.random()
    # ... and what stays on draws what it drew with the others on
    only_yaw = D.Augment({"yaw_deg": 180, "seed": 5}).draw(6)
    assert [(p.cos, p.sin) for p in only_yaw] == [(p.cos, p.sin) for p in one]
    assert all((p.a, p.b, p.mirror, p.gain) == (1, 1, False, 1.0) for p in only_yaw)


@pytest.mark.parametrize("cfg,match", [({"flip": 0.5}, "unknown key"), ({"speeds": ["2/4"]}, "not reduced"),
                                       ({"speeds": ["65/64"]}, r"\[1, 64\]"), ({"speeds": ["0/1"]}, r"\[1, 64\]"),
                                       ({"speeds": ["fast"]}, "a/b"), ({"mirror": -0.1}, "probability"),
                                       ({"mirror": 1.5}, "probability"), ({"yaw_deg": -1}, "yaw_deg"),
                                       ({"gain_db": -3}, "gain_db")], ids=str)
def test_bad_configurations_raise(cfg, match):
    with pytest.raises(ValueError, match=match):
        D.Augment(cfg)


def test_a_take_that_is_too_short_raises_and_names_it():
    ds = A.dataset(augment={"speeds": ["2/1"]})       # 12 frames at 2/1 need 23: take_B has exactly 23
    ds[0], ds[2]
    with pytest.raises(ValueError, match="take_B"):
        ds[1]
    with pytest.raises(ValueError, match="take_B"):
        ds.sample_batch([0, 1])


# ------------------------------------------------------------------------------------------------ the dataset
def test_without_augment_nothing_changes():
    """augment=None: the windows are the plain slices at the starts the crop generator gives, drawn as before"""
    poses, tracks = A.takes()
    order = [0, 2, 1, 0, 1]
    rng = np.random.RandomState(3)
    firsts = [int(rng.randint(0, A.FRAMES[i] - A.T)) for i in order]
    ds = A.dataset(augment=None)
    got = ds.sample_batch(order)
    assert len(got) == 5 and got[0].dtype == torch.float32
    want_p = np.stack([poses[i][f:f + A.T] for i, f in zip(order, firsts)])
    want_a = np.stack([tracks[i][f * A.HOP:f * A.HOP + A.S] for i, f in zip(order, firsts)])
    assert np.array_equal(got[0].numpy(), want_p.astype(np.float32)) and np.array_equal(got[2].numpy(), want_a.astype(np.float32))
    ds = A.dataset(augment=None)
    for i, f in zip(order, firsts):
        p, a, label, name = ds[i]
        assert np.array_equal(p.numpy(), poses[i][f:f + A.T]) and p.dtype == torch.float64
        assert np.array_equal(a.numpy(), tracks[i][f * A.HOP:f * A.HOP + A.S].astype(np.float32))
    # an augmentation with everything off is the identity on the same starts (1/1 draws from [0, L - T) too)
    ident = A.dataset(augment={}).sample_batch(order)
    assert torch.equal(ident[0], got[0]) and torch.equal(ident[2], got[2]) and ident[1] == got[1]
    assert torch.equal(ident[3], got[3]) and ident[4] == got[4]
    assert A.dataset(augment=None, withaudio=False).sample_batch(order)[0].shape == (5, A.T, 23, 3)


def test_host_sample_batch_and_getitem_follow_the_rule():
    cfg = dict(FULL, speeds=["4/5", "5/4", "1/1"])
    order = [2, 0, 1, 2]
    batch = A.dataset(augment=cfg).sample_batch(order)
    ds = A.dataset(augment=cfg)
    items = [ds[i] for i in order]          # the same draws, item by item (what --host-loader sees)
    assert torch.equal(batch[0], torch.stack([it[0] for it in items]).float())
    assert torch.equal(batch[2], torch.stack([it[1] for it in items]))
    # and they are augment_window under the drawn parameters
    params = D.Augment(cfg).draw(4)
    rng = np.random.RandomState(3)
    poses, tracks = A.takes()
    for r, (i, p) in enumerate(zip(order, params)):
        first = int(rng.randint(0, A.FRAMES[i] - D.frames_needed(A.T, p.a, p.b)))
        wp, wa = D.augment_window(poses[i], tracks[i], first, A.T, A.S, A.HOP, p, ds.pose_scaler)
        assert np.array_equal(items[r][0].numpy(), wp) and np.array_equal(items[r][1].numpy(), wa.astype(np.float32))
    none = A.dataset(augment=cfg, withaudio=False)
    assert len(none[0]) == 3 and len(none.sample_batch([0, 1])) == 4


def test_subsets_drop_the_augmentation_and_only_the_train_loader_gets_it():
    ds = A.dataset(augment=FULL)
    assert ds.subset([0, 1]).augment is None and ds.subset([0, 1]).pose_scaler is ds.pose_scaler
    assert ds.subset([0], augment=ds.augment).augment is ds.augment
    poses, tracks = A.takes()
    state = {"sequences": poses * 3, "labels": np.arange(9) % 4, "dirs": ["t%d" % i for i in range(9)],
             "musics": tracks * 3}
    big = D.SequenceDataset(state, A.CONFIG, resume=True, withaudio=True, augment=dict(FULL, speeds=["1/1", "4/5"]))
    train, val, parts = D.make_loaders(big, 2)
    assert train.dataset.augment is big.augment and val.dataset.augment is None
    assert len(train.dataset) == len(parts[0]) and len(val.dataset) == len(parts[1]) > 0
    poses_b, lengths, audio_b, labels, dirs = next(iter(train))
    assert poses_b.shape == (2, A.T, 23, 3) and audio_b.shape == (2, A.S) and poses_b.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ the wiring
def test_the_yaml_key_reaches_the_dataset(tmp_path):
    import collections
    from music2dance_amd import runner
    folder = D.write_synthetic_dataset(str(tmp_path / "ds"), n_takes=2, seconds=1, audio_rate=1600, seed=1)
    Opts = collections.namedtuple("Opts", "folder")
    for block, kind in ((None, type(None)), ({"mirror": 0.5, "speeds": ["24/25"]}, D.Augment)):
        cfg = {"dataset": dict(A.CONFIG, augment=block), "dance_types": ["W", "C", "R", "T"], "folder": folder}
        if block is None:
            del cfg["dataset"]["augment"]
        run = runner.Run(0, 1, torch.device("cpu"), cfg, Opts(None))
        ds = runner.sequence_dataset(run, withaudio=False)
        assert isinstance(ds.augment, kind) and ds.pose_scaler is ds.scaler is not None
    assert ds.augment.speeds == ((24, 25),) and ds[0][0].shape == (A.T, 23, 3)


def test_synthetic_argument_handling_is_untouched():
    from music2dance_amd.phase3 import train as T3
    opts = T3.parser().parse_args(["-c", "x.yaml", "-d", "0", "-n", "r", "--synthetic"])
    assert opts.synthetic and not opts.host_loader and opts.folder is None
    assert "augment" not in " ".join(T3.parser()._option_string_actions)


def test_the_binding_is_in_the_headers_order():
    from music2dance_amd import _lib, build, kernels
    names = list(_lib.SIGNATURES)
    assert names[names.index("m2d_resample_poly") + 1] == "m2d_crop_augment" and "augment.hip" in build.SOURCES
    header = open(ROOT + "/include/m2d.h").read()
    order = re.findall(r"\b(m2d_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert order[order.index("m2d_resample_poly") + 1] == "m2d_crop_augment"
    assert len(_lib.SIGNATURES["m2d_crop_augment"][1]) == 16 and callable(kernels.crop_augment)
    # the numpy record is struct M2dAugmentRow, field for field
    body = re.search(r"typedef struct M2dAugmentRow \{(.*?)\}", header, flags=re.S).group(1)
    fields = [n.strip() for line in body.split(";") if line.strip() for n in line.split(None, 1)[1].replace("long ", "").split(",")]
    assert fields == list(kernels.AUGMENT_ROW.names) and kernels.AUGMENT_ROW.itemsize == 80


def test_the_wrapper_needs_device_tensors():
    from music2dance_amd import _lib, kernels
    table = np.zeros(1, dtype=kernels.AUGMENT_ROW)
    with pytest.raises(_lib.M2dError, match="no CPU path"):
        kernels.crop_augment(torch.zeros(4, 69), None, table, torch.ones(69), torch.zeros(69), None, 2, 0)


def test_the_train_scripts_run_augmented_on_the_host(tmp_path, monkeypatch):
    """without a device the scripts' loaders run the rule itself (DataLoader -> __getitem__ -> augment_window): phase 3
    augments its train subset only, phase 2 its audio-less loader; the first batch is the rule under the seeded draws"""
    import yaml
    from music2dance_amd import kernels, runner
    from music2dance_amd.phase2 import train as T2
    from music2dance_amd.phase3 import train as T3
    from tests.fake_backend import FakeKernels
    prev = kernels.set_impl(FakeKernels())
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    monkeypatch.chdir(tmp_path)
    block = {"mirror": 0.5, "yaw_deg": 180, "speeds": ["1/1", "24/25", "25/24"], "gain_db": 3, "seed": 0}
    pkg = ROOT + "/music2dance_amd/"
    try:
        folder = D.write_synthetic_dataset(str(tmp_path / "ds"), n_takes=10, seconds=6, seed=1)
        for script, src, extra in ((T3, "phase3/configs/ablated.yaml", []), (T2, "phase2/configs/default.yaml", ["-f", "wgangp"])):
            cfg = yaml.safe_load(open(pkg + src))
            cfg.update(batch_size=2, num_train=6, num_epochs=1, n_critic_steps=2, folder=folder)
            cfg["dataset"]["augment"] = block
            (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
            seen, calls = [], []
            collate, window = D.collate_fn, D.augment_window
            with monkeypatch.context() as m:
                m.setattr(D, "collate_fn", lambda *a, **k: (seen.append(collate(*a, **k)), seen[-1])[1])
                m.setattr(D, "augment_window", lambda *a: (calls.append(a), window(*a))[1])
                eng = script.main(["-c", str(tmp_path / "cfg.yaml"), "-d", "0", "-n", "h", "--no-run-dir", "--iterations", "2"] + extra)
            assert eng.total_iterations == 2 and all(np.isfinite(float(v)) for v in eng.last_full.values())
            audio = script is T3
            # every call belongs to a train batch (two rows each): the validation batch of phase 3 is not augmented
            assert len(calls) == 4 and all((c[1] is not None) == audio for c in calls)
            params = D.Augment(block).draw(4)
            assert [c[6] for c in calls] == params and len({(p.a, p.b) for p in params}) > 1
            for r, c in enumerate(calls[:2]):
                wp, wa = D.augment_window(*c)
                assert np.array_equal(seen[0][0][r].numpy(), wp.astype(np.float32))
                if audio:
                    assert np.array_equal(seen[0][2][r].numpy(), wa.astype(np.float32))
    finally:
        kernels.set_impl(prev)
