"""The crop + augment gather on the device (m2d_crop_augment, kernels.crop_augment, SequenceDataset(augment=); DESIGN.md
section 19) on the small store of tests/augment_cases.py: parity with the host rule (data.augment_window, fp64) inside
derived bounds; identity parameters give the bits of the plain gather; the audio leg is m2d_resample_poly bit for bit,
take boundaries included; a row's output does not depend on the batch around it nor on where the store puts its take
(one case past 2^31 samples); the audio-less form; the argument and table errors; and the train scripts end to end."""
import os

import numpy as np
import pytest
import torch
import yaml

from music2dance_amd import data as D
from tests import augment_cases as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music2dance_amd")


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def K():
    from music2dance_amd import kernels
    return kernels.impl()


_DS = {}


def dataset(withaudio=True):
    """one resident dataset per form, shared by the tests (nothing writes to it)"""
    if withaudio not in _DS:
        _DS[withaudio] = A.dataset(withaudio=withaudio)
    return _DS[withaudio]


def edge_rows(a, b):
    """(take, start) pairs: both ends of every take - for the middle take the windows that touch its neighbours"""
    return [(i, f) for i, L in enumerate(A.FRAMES) for f in (0, A.last_start(L, a, b))]


def _ratio(err, bound):
    """worst err / bound; a zero bound admits a zero error only"""
    assert np.all(err[bound == 0] == 0)
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("speed", A.SPEEDS, ids=lambda s: "%dover%d" % s)
def test_parity_with_the_host_rule(speed):
    """every {mirror, no mirror} x {0, 37, -180 degrees} x {gain 1, 0.7} of one speed as the rows of one launch, the
    rows walking over both ends of all three takes. Audio: |y - y64| <= (P + 4) 2^-24 g sum |tap| |x|
    (augment_cases.audio_bound). Poses: the running-error bound of augment_cases.pose_bound, which follows the kernel's
    roundings through the fp64 intermediates: with u = 2^-24 (1 + 2^-10),
      E_v = u (2 |f d| + |V|) for the interpolation (0 when f == 0); identity transform: E = E_v; otherwise
      E_U = (E_v + u |shift| + u |V - shift|) / |scale| + 2 u |U|,
      E_X' = |c| E_Ux + |s| E_Uz + u (|c X| + 2 |s Z| + |X'|) (Z' alike, Y' = E_Uy),
      E_out = |scale| E_U' + u (|U' scale| + |shift| + |out|).
    Neither bound is tuned: a ratio above 1 is a failure."""
    a, b = speed
    ds = dataset()
    combos = [A.params(a, b, m, deg, g) for m in (False, True) for deg in (0.0, 37.0, -180.0) for g in (1.0, 0.7)]
    where = edge_rows(a, b)
    idx = [where[r % len(where)][0] for r in range(len(combos))]
    firsts = [where[r % len(where)][1] for r in range(len(combos))]
    poses, audio = ds.gather_augmented(idx, firsts, combos, DEV)
    poses, audio = poses.cpu().double().numpy(), audio.cpu().double().numpy()
    takes, tracks = A.takes()
    worst_p = worst_a = 0.0
    for r, (i, f, p) in enumerate(zip(idx, firsts, combos)):
        wp, wa = D.augment_window(takes[i], tracks[i], f, A.T, A.S, A.HOP, p, ds.pose_scaler)
        worst_p = max(worst_p, _ratio(np.abs(poses[r] - wp), A.pose_bound(takes[i], f, p, ds.pose_scaler)))
        worst_a = max(worst_a, _ratio(np.abs(audio[r] - wa), A.audio_bound(tracks[i], f * A.HOP, a, b, p.gain)))
    print("crop_augment %d/%d: worst pose error / bound = %.3e, worst audio error / bound = %.3e" % (a, b, worst_p, worst_a))
    note("crop_augment pose |v - v64| / running-error bound  %d/%d" % speed, worst_p)
    note("crop_augment audio |y - y64| / ((P + 4) 2^-24 g sum|h||x|)  %d/%d" % speed, worst_a)
    assert worst_p <= 1.0 and worst_a <= 1.0, (worst_p, worst_a)


# ------------------------------------------------------------------------------------------------ 2. identity
def test_identity_parameters_are_todays_gather():
    order = [0, 2, 1, 0, 1, 2, 2]
    plain = A.dataset(augment=None).sample_batch(order, DEV)
    rng = np.random.RandomState(3)
    firsts = [int(rng.randint(0, A.FRAMES[i] - A.T)) for i in order]
    poses, audio = dataset().gather_augmented(order, firsts, [D.IDENTITY] * len(order), DEV)
    assert torch.equal(poses, plain[0]) and torch.equal(audio, plain[2])
    off = A.dataset(augment={"seed": 9}).sample_batch(order, DEV)     # everything off: the same starts, the same bits
    assert torch.equal(off[0], plain[0]) and torch.equal(off[2], plain[2]) and torch.equal(off[3], plain[3])
    assert off[1] == plain[1] and off[4] == plain[4]


# ------------------------------------------------------------------------------------------------ 3. the resampler
@pytest.mark.parametrize("speed", A.SPEEDS, ids=lambda s: "%dover%d" % s)
def test_the_audio_leg_is_the_resampler(speed):
    """gain 1: every row is m2d_resample_poly on its take ALONE, declared at x0 = k a - a0 and read from output k b,
    k = ceil(a0 / a) - also for the windows at both ends of the middle take, whose filters reach past it: a read outside
    the take would bring in the neighbours' 1e3"""
    a, b = speed
    ds = dataset()
    where = edge_rows(a, b) + [(1, 3), (2, 17)]
    idx, firsts = [w[0] for w in where], [w[1] for w in where]
    audio = ds.gather_augmented(idx, firsts, [A.params(a, b, True, 37.0, 1.0)] * len(where), DEV)[1]
    taps = torch.as_tensor(D.speed_taps(a, b), dtype=torch.float32).to(DEV)
    store = ds._tracks.device(DEV)
    for r, (i, f) in enumerate(where):
        take = store[int(ds._tracks.starts[i]):int(ds._tracks.starts[i + 1])].clone()[None]
        a0 = f * A.HOP
        k = -(-a0 // a)
        want = K().resample_poly(take, k * a - a0, taps, b, a, k * b, A.S)
        assert torch.equal(audio[r:r + 1], want), (i, f, float((audio[r] - want[0]).abs().max()))
        if i == 1:
            assert float(audio[r].abs().max()) < 10.0


# ------------------------------------------------------------------------------------------------ 4. pure function
def test_a_row_does_not_depend_on_the_batch_around_it():
    ds = dataset()
    row = (2, 7, A.params(25, 24, True, 37.0, 0.7))
    alone = ds.gather_augmented([row[0]], [row[1]], [row[2]], DEV)
    others = [(i % 3, 1 + i, A.params(*A.SPEEDS[i % 5], bool(i % 2), 10.0 * i, 1.0 + 0.1 * i)) for i in range(7)]
    others[5] = row
    seven = ds.gather_augmented(*zip(*others), DEV)
    many = ds.gather_augmented([row[0]] * 64, [row[1]] * 64, [row[2]] * 64, DEV)
    for got in (seven[0][5:6], many[0][:1], many[0][63:]):
        assert torch.equal(got, alone[0])
    for got in (seven[1][5:6], many[1][:1], many[1][63:]):
        assert torch.equal(got, alone[1])
    assert torch.equal(many[0], alone[0].expand_as(many[0])) and torch.equal(many[1], alone[1].expand_as(many[1]))


def _hand_table(kernels, B, pose, audio, p, slot):
    t = np.zeros(B, dtype=kernels.AUGMENT_ROW)
    t["pose_start"], t["pose_first"], t["pose_last"] = pose
    t["audio_start"], t["audio_first"], t["audio_last"] = audio
    t["a"], t["b"], t["mirror"], t["cos_yaw"], t["sin_yaw"], t["gain"] = p.a, p.b, p.mirror, p.cos, p.sin, p.gain
    t["tap_offset"], t["ntaps"] = slot
    return t


def test_a_take_past_two_to_the_31_samples():
    """the same take at the front of a small store and behind 2^31 samples of a long one (about 8.6 GB of fp32), its
    neighbours filled with 1e3: the same bits"""
    from music2dance_amd import kernels
    takes, tracks = A.takes()
    p = A.params(25, 24, False, 37.0, 0.7)
    take = torch.as_tensor(tracks[2], dtype=torch.float32)
    n, off, f = take.numel(), 2 ** 31 + 1001, A.last_start(A.FRAMES[2], 25, 24)
    try:
        far = torch.full((off + n + 4096,), 1000.0, dtype=torch.float32, device=DEV)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for a store of 2^31 samples (8.6 GB) on this device")
    far[off:off + n] = take.to(DEV)
    near = torch.full((n + 4096,), 1000.0, dtype=torch.float32, device=DEV)
    near[:n] = take.to(DEV)
    poses = torch.as_tensor(takes[2], dtype=torch.float32).reshape(-1, 69).to(DEV)
    sc = A.scaler(takes)._coeffs(torch.device(DEV), False)
    taps = torch.as_tensor(D.speed_taps(25, 24), dtype=torch.float32).to(DEV)
    pose = (f, 0, A.FRAMES[2] - 1)
    got_far = kernels.crop_augment(poses, far, _hand_table(kernels, 2, pose, (off + f * A.HOP, off, off + n - 1), p,
                                                            (0, taps.numel())), *sc, taps, A.T, A.S)
    got_near = kernels.crop_augment(poses, near, _hand_table(kernels, 2, pose, (f * A.HOP, 0, n - 1), p,
                                                              (0, taps.numel())), *sc, taps, A.T, A.S)
    assert torch.equal(got_far[1], got_near[1]) and torch.equal(got_far[0], got_near[0])
    want = D.augment_window(takes[2], tracks[2], f, A.T, A.S, A.HOP, p, A.scaler(takes))[1]
    err = np.abs(got_far[1][0].cpu().double().numpy() - want)
    assert np.all(err <= A.audio_bound(tracks[2], f * A.HOP, 25, 24, p.gain))
    del far


# ------------------------------------------------------------------------------------------------ 5. audio-less
def test_the_audio_less_form_gives_the_same_poses():
    rows = [(i % 3, 2 + i, A.params(*A.SPEEDS[i % 5], bool(i % 2), 25.0 * i, 0.7)) for i in range(6)]
    with_audio = dataset().gather_augmented(*zip(*rows), DEV)
    without = dataset(withaudio=False).gather_augmented(*zip(*rows), DEV)
    assert without[1] is None and torch.equal(without[0], with_audio[0])
    batch = A.dataset(augment={"mirror": 0.5, "yaw_deg": 90, "speeds": ["4/5", "5/4"], "gain_db": 6},
                      withaudio=False).sample_batch([0, 1, 2, 1], DEV)
    assert len(batch) == 4 and batch[0].shape == (4, A.T, 23, 3) and bool(torch.isfinite(batch[0]).all())


def test_operands_off_16_byte_alignment():
    """every pointer of the call one float into its buffer: the same bits (the kernel loads and stores 4 bytes wide)"""
    from music2dance_amd import kernels
    ds = dataset()
    rows = [(i % 3, 1 + i, A.params(*A.SPEEDS[(i + 2) % 5], bool(i % 2), 33.0 * i, 0.7)) for i in range(5)]
    want = ds.gather_augmented(*zip(*rows), DEV)

    def off(t):
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
        buf[1:] = t.reshape(-1)
        return buf[1:].view(t.shape)

    captured = {}
    orig = kernels.crop_augment

    def shifted(poses, track, table, scale, shift, taps, T, S):
        captured["n"] = captured.get("n", 0) + 1
        args = [off(t) for t in (poses, track, scale, shift, taps)]
        assert all(t.data_ptr() % 16 == 4 for t in args)
        return orig(args[0], args[1], table, args[2], args[3], args[4], T, S)

    kernels.crop_augment = shifted
    try:
        got = ds.gather_augmented(*zip(*rows), DEV)
    finally:
        kernels.crop_augment = orig
    assert captured["n"] == 1 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 6. errors
def test_argument_errors_name_the_entry_point_and_launch_nothing():
    from music2dance_amd import _lib, kernels
    dev = torch.device(DEV)
    poses = torch.zeros(8, 69, device=DEV)
    track = torch.zeros(8 * A.HOP, device=DEV)
    one = torch.ones(69, device=DEV)
    taps = torch.ones(1, device=DEV)
    rows = torch.from_numpy(_hand_table(kernels, 1, (0, 0, 7), (0, 0, 8 * A.HOP - 1), D.IDENTITY, (0, 1)).view(np.uint8)).to(DEV)
    out = torch.full((1, 2, 69), 7.0, device=DEV)
    aud = torch.full((1, 16), 7.0, device=DEV)
    P = kernels._ptr

    def call(poses=P(poses), frames=8, C=69, track=P(track), samples=8 * A.HOP, rows=P(rows), scale=P(one), shift=P(one),
             taps=P(taps), ntaps=1, out=P(out), aud=P(aud), B=1, T=2, S=16):
        kernels._launch("m2d_crop_augment", dev, poses, frames, C, track, samples, rows, scale, shift, taps, ntaps, out,
                        aud, B, T, S)

    bad = [dict(B=0), dict(T=0), dict(C=0), dict(S=-1), dict(C=68), dict(poses=0), dict(rows=0), dict(scale=0),
           dict(shift=0), dict(out=0), dict(frames=0), dict(track=0), dict(taps=0), dict(aud=0), dict(samples=0)]
    for kw in bad:
        with pytest.raises(_lib.M2dError, match="m2d_crop_augment"):
            call(**kw)
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((aud == 7).all())
    call(track=0, taps=0, aud=0, samples=0, ntaps=0, S=0)       # the audio-less form is no error
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((aud == 7).all())


def test_the_wrapper_rejects_bad_tables_before_any_launch(monkeypatch):
    from music2dance_amd import _lib, kernels
    launched = []
    monkeypatch.setattr(kernels, "_launch", lambda *a: launched.append(a))
    poses = torch.zeros(40, 69, device=DEV)
    track = torch.zeros(40 * A.HOP, device=DEV)
    one = torch.ones(69, device=DEV)
    taps = torch.ones(101, device=DEV)
    last = 40 * A.HOP - 1

    def call(p=A.params(5, 4), pose=(3, 0, 39), audio=(3 * A.HOP, 0, last), slot=(0, 101), track=track, taps=taps, S=A.S):
        return kernels.crop_augment(poses, track, _hand_table(kernels, 2, pose, audio, p, slot), one, one, taps, A.T, S)

    call()
    assert len(launched) == 1
    bad = [dict(p=A.params(2, 4)), dict(p=A.params(65, 64)), dict(p=A.params(0, 1)), dict(slot=(0, 100)),
           dict(slot=(1, 101)), dict(slot=(-1, 101)), dict(slot=(0, 1283)), dict(pose=(26, 0, 39)), dict(pose=(3, 4, 39)),
           dict(pose=(3, 0, 40)), dict(pose=(3, -1, 39)), dict(audio=(0, 0, last + 1)), dict(audio=(0, -1, last)),
           dict(audio=(last + 1, 0, last)), dict(p=A.params(5, 4, gain=float("nan"))), dict(track=None), dict(taps=None)]
    for kw in bad:
        with pytest.raises(_lib.M2dError, match="crop_augment"):
            call(**kw)
    with pytest.raises(_lib.M2dError, match="AUGMENT_ROW"):
        kernels.crop_augment(poses, track, np.zeros((2, 20)), one, one, taps, A.T, A.S)
    assert len(launched) == 1
    call(slot=(0, 100), p=A.params(1, 1))       # the taps of a 1/1 row are not read
    call(track=None, taps=None, S=0)
    assert len(launched) == 3


# ------------------------------------------------------------------------------------------------ 7. end to end
def _cfg(tmp_path, src, **over):
    cfg = yaml.safe_load(open(os.path.join(PKG, src)))
    dataset_over = over.pop("dataset", {})
    cfg.update(over)
    cfg["dataset"].update(dataset_over)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


AUGMENT = {"mirror": 0.5, "yaw_deg": 180, "speeds": ["1/1", "24/25", "25/24"], "gain_db": 3, "seed": 0}


def _first_batches(monkeypatch, main, argv):
    """run a train script and keep the first batch its loader made, and the arguments of the host rule's calls"""
    seen, calls = [], []
    sample, collate, window = D.SequenceDataset.sample_batch, D.collate_fn, D.augment_window
    with monkeypatch.context() as m:
        m.setattr(D.SequenceDataset, "sample_batch", lambda self, *a, **k: (seen.append(sample(self, *a, **k)), seen[-1])[1])
        m.setattr(D, "collate_fn", lambda *a, **k: (seen.append(collate(*a, **k)), seen[-1])[1])
        m.setattr(D, "augment_window", lambda *a: (calls.append(a), window(*a))[1])
        eng = main(argv)
    return eng, seen[0], calls


def _within_the_bounds(resident, host, calls, audio):
    B = resident[0].shape[0]
    assert len(calls) >= B and host[0].shape == resident[0].shape
    worst = 0.0
    for r, (take, track, p0, T, S, hop, p, sc) in enumerate(calls[:B]):
        wp, wa = D.augment_window(take, track, p0, T, S, hop, p, sc)
        # (the host loader's batch is the fp64 rule rounded to fp32)
        assert np.array_equal(host[0][r].cpu().numpy(), wp.astype(np.float32))
        # the resident store holds the scaled poses rounded to fp32 (the host loader rounds after the transform): the
        # kernel is held to the rule on the values it reads
        take = np.asarray(take).astype(np.float32).astype(np.float64)
        w32 = D.augment_window(take, None, p0, T, 0, hop, p, sc)[0]
        err = np.abs(resident[0][r].cpu().double().numpy() - w32)
        worst = max(worst, _ratio(err, A.pose_bound(take, p0, p, sc, T=T)))
        if audio:
            err = np.abs(resident[2][r].cpu().double().numpy() - wa)
            worst = max(worst, _ratio(err, A.audio_bound(track, p0 * hop, p.a, p.b, p.gain, S=S)))
    return worst


def test_the_train_scripts_run_augmented_and_both_loaders_see_the_same_batches(tmp_path, monkeypatch):
    from music2dance_amd import _lib, kernels
    from music2dance_amd.phase2 import train as T2
    from music2dance_amd.phase3 import train as T3
    monkeypatch.chdir(tmp_path)
    folder = D.write_synthetic_dataset(str(tmp_path / "ds"), n_takes=12, seconds=6, seed=2)
    small = dict(batch_size=4, num_epochs=4, n_critic_steps=2)
    first = {}
    # the phase-2 script sets the GEMM engine's PROCESS-WIDE plan model (kernels.set_plan_model): put it back, the
    # tests that run after this one in the same process hold their kernels to the default model's summation orders
    model = _lib.lib().m2d_plan_model_get()
    try:
        _run_the_scripts(monkeypatch, tmp_path, folder, small, first, T2, T3)
    finally:
        kernels.set_plan_model(model)
    _compare_the_first_batches(first)


def _run_the_scripts(monkeypatch, tmp_path, folder, small, first, T2, T3):
    for aug in (AUGMENT, None):
        for extra in ([], ["--host-loader"]):
            c3 = _cfg(tmp_path, "phase3/configs/ablated.yaml", folder=folder, dataset={"augment": aug}, **small)
            n = 4 if aug and not extra else 1
            e3, batch, calls = _first_batches(monkeypatch, T3.main, ["-c", c3, "-d", "0", "-n", "a3", "--no-run-dir",
                                                                     "--iterations", str(n)] + extra)
            assert e3.total_iterations == n and all(np.isfinite(float(v)) for v in e3.last_full.values())
            first[(3, bool(aug), bool(extra))] = (batch, calls)
            if aug is None and extra:
                continue        # (phase 2 without augmentation on the host: the loaders' own test covers it)
            c2 = _cfg(tmp_path, "phase2/configs/default.yaml", num_train=10, dataset={"augment": aug}, **small)
            np.random.seed(5)   # phase 2 crops from numpy's global generator as the run finds it (phase 3 seeds it)
            e2, batch, calls = _first_batches(monkeypatch, T2.main, ["-c", c2, "-d", "0", "-n", "a2", "--no-run-dir", "-f", "wgangp",
                                                                     "--folder", folder, "--iterations", str(n)] + extra)
            assert e2.total_iterations == n and all(np.isfinite(float(v)) for v in e2.last_full.values())
            first[(2, bool(aug), bool(extra))] = (batch, calls)


def _compare_the_first_batches(first):
    # augmented: the resident loader's first batch is the host loader's, inside the bounds of the parity test
    for phase, audio in ((3, True), (2, False)):
        resident, host = first[(phase, True, False)][0], first[(phase, True, True)][0]
        assert not first[(phase, True, False)][1]                      # the resident path never ran the host rule
        worst = _within_the_bounds(resident, host, first[(phase, True, True)][1], audio)
        print("phase %d, first batch: worst resident-loader error / bound = %.3e" % (phase, worst))
        note("crop_augment end to end, phase %d: error / bound" % phase, worst)
        assert worst <= 1.0
        assert torch.equal(resident[-2].cpu(), host[-2].cpu()) and tuple(resident[-1]) == tuple(host[-1])
    # no `augment` key: the bits of the plain gather, which are the host loader's
    plain, host = first[(3, False, False)][0], first[(3, False, True)][0]
    assert torch.equal(plain[0].cpu(), host[0].float()) and torch.equal(plain[2].cpu(), host[2])
    assert not first[(3, False, True)][1] and not torch.equal(plain[0], first[(3, True, False)][0][0])
