"""Host half of the k-nearest-neighbour scores (music2dance_amd.metrics.prdc), through the numpy
stand-in of tests/knn_cases.py: worked cases by hand (five points on a line with a duplicate: every score, k = 1 and 2,
the inclusive tie, self-exclusion by index), metrics.prdc against the numpy statement, the flags and JSON keys of
phase3.evaluate --prdc, phase1.evaluate --synthetic end to end, and the ctypes table."""
import json
import math
import os

import numpy as np
import pytest
import torch
import yaml

from tests import knn_cases as K
from tests.fake_backend import FakeKernels
from tests.test_distribution_host import FD_KEYS, TODAY, _sets

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "music2dance_amd")
R5 = np.array([[0.0], [1.0], [1.0], [3.0], [6.0]], dtype=np.float32)        # rows 1 and 2 are duplicates
F4 = np.array([[1.0], [2.0], [5.0], [10.0]], dtype=np.float32)
KINETIC_PRDC = ["%s_kinetic" % k for k in K.PRDC_KEYS] + ["prdc_k"]
P1_KEYS = (K.PRDC_KEYS + ["precision_real_split", "recall_real_split", "density_real_split", "coverage_real_split",
                          "fd_pose", "fd_pose_real_split", "fd_pose_converged", "div_pose_real", "div_pose_fake", "k",
                          "n_real", "n_fake", "checkpoint"])


class KnnFakeKernels(K.NumpyKnnBackend, FakeKernels):
    """the stand-in of the script tests: FakeKernels for the networks, the fp64 statements for the scores"""


@pytest.fixture
def stand_in(monkeypatch):
    from music2dance_amd import kernels
    monkeypatch.setattr(kernels, "impl", lambda: K.NumpyKnnBackend())


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def test_radii_by_hand(stand_in):
    from music2dance_amd import metrics
    # row 1: its duplicate (row 2) is at distance 0 and counts; the row itself does not, although it is at 0 too
    assert metrics.knn_radii(t(R5), 1).tolist() == [1.0, 0.0, 0.0, 4.0, 9.0]
    assert metrics.knn_radii(t(R5), 2).tolist() == [1.0, 1.0, 1.0, 4.0, 25.0]
    assert metrics.knn_radii(t(F4), 1).tolist() == [1.0, 1.0, 9.0, 25.0]
    assert metrics.knn_radii(t(F4), 2).tolist() == [16.0, 9.0, 16.0, 64.0]
    assert K.radii(R5, 1).tolist() == [1.0, 0.0, 0.0, 4.0, 9.0] and K.radii(F4, 2).tolist() == [16.0, 9.0, 16.0, 64.0]


def test_ball_query_by_hand(stand_in):
    from music2dance_amd import metrics
    r2 = metrics.knn_radii(t(R5), 1)
    count, nn_d2, nn_idx = metrics.ball_query(t(F4), t(R5), r2)
    # F = 1 lies ON the spheres of R = 0 (1 <= 1) and R = 3 (4 <= 4): inclusive
    assert count.tolist() == [4, 1, 2, 0] and count.dtype == torch.int32
    assert nn_d2.tolist() == [0.0, 1.0, 1.0, 16.0] and nn_d2.dtype == torch.float32
    assert nn_idx.tolist() == [1, 1, 4, 4]                   # F = 1: rows 1 and 2 tie at 0; F = 2: rows 1, 2, 3 tie at 1
    none, nn2, idx2 = metrics.ball_query(t(F4), t(R5))
    assert none is None and torch.equal(nn2, nn_d2) and torch.equal(idx2, nn_idx)


def test_scores_by_hand(stand_in):
    from music2dance_amd import metrics
    one = metrics.prdc(t(R5), t(F4), 1)
    assert list(one) == K.PRDC_KEYS == list(metrics.PRDC_KEYS)
    for v in one.values():
        assert v.dtype == torch.float64 and v.dim() == 0
    got = {k: float(v) for k, v in one.items()}
    assert got == {"precision": 0.75, "recall": 1.0, "density": 7.0 / 4.0, "coverage": 1.0, "nn_ratio_median": 1.0,
                   "nn_fake_to_real_median": 1.0, "nn_real_to_real_median": 1.0}
    two = {k: float(v) for k, v in metrics.prdc(t(R5), t(F4), 2).items()}
    assert two["precision"] == 1.0 and two["density"] == 12.0 / 8.0 and two["recall"] == 1.0 and two["coverage"] == 1.0
    assert two["nn_real_to_real_median"] == 1.0               # always the k = 1 radii
    # without F = 1 the real rows 0, 1, 2 have no generated row inside their k = 1 ball
    three = {k: float(v) for k, v in metrics.prdc(t(R5), t(F4[1:]), 1).items()}
    assert three["coverage"] == 2.0 / 5.0 and three["precision"] == 2.0 / 3.0 and three["density"] == 1.0
    assert three["recall"] == 1.0
    # a far real row is not recalled
    far = R5.copy()
    far[4] = 20.0
    assert float(metrics.prdc(t(far), t(F4), 1)["recall"]) == 4.0 / 5.0
    # more than half of the real rows duplicated: the median real-to-real distance is 0, the ratio undefined
    dup = np.array([[0.0], [0.0], [2.0], [2.0], [5.0]], dtype=np.float32)
    r = metrics.prdc(t(dup), t(F4), 1)
    assert float(r["nn_real_to_real_median"]) == 0.0 and math.isnan(float(r["nn_ratio_median"]))


def test_nearest_stats():
    from music2dance_amd import metrics
    s = metrics.nearest_stats(torch.tensor([16.0, 0.0, 4.0, 1.0]))
    assert {k: float(v) for k, v in s.items()} == {"median": 1.5, "mean": 7.0 / 4.0, "min": 0.0}
    assert all(v.dtype == torch.float64 and v.dim() == 0 for v in s.values())
    assert float(metrics.nearest_stats(torch.tensor([9.0, 1.0, 4.0]))["median"]) == 2.0


@pytest.mark.parametrize("k", [1, 3])
def test_prdc_through_the_stand_in_equals_the_numpy_statement(stand_in, k):
    from music2dance_amd import metrics
    R, F = K.lattice()
    want = K.prdc(R, F, k)
    got = {key: float(v) for key, v in metrics.prdc(t(R), t(F), k).items()}
    assert got == pytest.approx(want, abs=1e-15, nan_ok=True)
    assert 0 < want["precision"] < 1 and 0 < want["coverage"] < 1 and want["density"] > 0
    ties = int((K.d2_matrix(F, R) == K.radii(R, k)[None, :]).sum())
    assert ties >= 40                                         # pairs exactly on a sphere


def test_the_recipes():
    R, F = K.split_case(257, 300, 69, 0.5)
    assert R.shape == (257, 69) and F.shape == (300, 69) and R.dtype == F.dtype == np.float32
    R0, F0 = K.split_case(257, 300, 69, 0.0)
    assert np.array_equal(R0, R) and np.array_equal(F0 + np.float32(0.5), F)
    L, G = K.lattice()
    assert L.shape == (203, 6) and G.shape == (150, 6) and np.array_equal(L[100:120], L[0:20])
    assert np.all(K.radii(L, 1)[100:120] == 0.0)
    assert K.eps(69) == 73 * 2.0 ** -24


def test_flags_parse(capsys):
    from music2dance_amd.phase1 import evaluate as E1
    from music2dance_amd.phase3 import evaluate as E3
    base = ["-c", "x.yaml", "-l", "run", "--classifier", "w.pt"]
    assert E3.parse_args(base).prdc is None and E3.parse_args(base + ["--frechet"]).prdc is None
    assert E3.parse_args(base + ["--frechet", "--prdc"]).prdc == 5
    assert E3.parse_args(base + ["--frechet", "--prdc", "3", "--modes", "2"]).prdc == 3
    for bad in (["--prdc"], ["--prdc", "3"], ["--frechet", "--prdc", "0"]):
        with pytest.raises(SystemExit):
            E3.parse_args(base + bad)
    o = E1.parse_args(["-c", "x.yaml", "-l", "run"])
    assert (o.samples, o.k, o.max_real, o.seed, o.sheet, o.synthetic, o.gen_weights) == (4096, 5, None, 0, 25, False, None)
    o = E1.parse_args(["-c", "x.yaml", "-l", "run", "--samples", "64", "--k", "3", "--max-real", "100", "--seed", "4",
                       "--sheet", "0", "--synthetic", "--folder", "f", "-d", "1", "--gen-weights", "g.pt"])
    assert (o.samples, o.k, o.max_real, o.seed, o.sheet, o.synthetic, o.folder, o.device) == (64, 3, 100, 4, 0, True, "f", 1)
    for bad in (["--k", "0"], ["--samples", "3", "--k", "3"], ["--max-real", "5"], ["--sheet", "-1"]):
        with pytest.raises(SystemExit):
            E1.parse_args(["-c", "x.yaml", "-l", "run"] + bad)
    capsys.readouterr()


def test_the_ctypes_table_has_the_entry_points():
    from music2dance_amd import _lib
    names = list(_lib.SIGNATURES)
    new = ["m2d_knn_max_k", "m2d_knn_radii_workspace_bytes", "m2d_knn_radii", "m2d_ball_query_workspace_bytes",
           "m2d_ball_query"]
    assert names[-5:] == new                                  # appended after the last declaration, in the header's order
    assert len(_lib.SIGNATURES["m2d_knn_radii"][1]) == 9 and len(_lib.SIGNATURES["m2d_ball_query"][1]) == 14
    from music2dance_amd import build
    assert "knn.hip" in build.SOURCES


def test_phase3_summary_keys_with_and_without_prdc(stand_in):
    from music2dance_amd.phase3 import evaluate
    jerk = np.array([1.0, 2.0, 3.0, 5.0])
    pred = np.array([0, 1, 2, 3])
    real, fakes = _sets(12, 2)
    off = evaluate.summary(jerk, jerk, pred, pred, kinetic=evaluate.kinetic_rows(real, fakes[:1], 25.0))
    assert list(off) == TODAY + FD_KEYS
    on = evaluate.summary(jerk, jerk, pred, pred, kinetic=evaluate.kinetic_rows(real, fakes[:1], 25.0, prdc_k=3))
    assert list(on) == TODAY + FD_KEYS + KINETIC_PRDC
    assert {k: on[k] for k in TODAY + FD_KEYS} == off and on["prdc_k"] == 3 and isinstance(on["prdc_k"], int)
    for k in KINETIC_PRDC[:-1]:
        assert isinstance(on[k], float) and math.isfinite(on[k]), k
    assert 0.0 <= on["precision_kinetic"] <= 1.0 and 0.0 <= on["coverage_kinetic"] <= 1.0
    both = evaluate.summary(jerk, jerk, pred, pred, kinetic=evaluate.kinetic_rows(real, fakes, 25.0, prdc_k=3))
    assert list(both) == TODAY + FD_KEYS + ["multimodality_kinetic"] + KINETIC_PRDC
    assert {k: both[k] for k in KINETIC_PRDC} == {k: on[k] for k in KINETIC_PRDC}
    json.dumps(evaluate.json_safe(both), allow_nan=False)
    # the values are the numpy statement's on the standardised features
    from tests import distribution_cases as C
    Fr = C.kinetic(real.numpy().reshape(12, 30, 23, 3)).astype(np.float32)
    Ff = C.kinetic(fakes[0].numpy().reshape(12, 30, 23, 3)).astype(np.float32)
    m, S = C.moments(Fr)
    Zr, Zf = ((Fr - m) / np.sqrt(np.diag(S))).astype(np.float32), ((Ff - m) / np.sqrt(np.diag(S))).astype(np.float32)
    want = K.prdc(Zr, Zf, 3)
    assert {k: on["%s_kinetic" % k] for k in K.PRDC_KEYS} == pytest.approx(want, rel=1e-6)
    # fewer rows than k + 1: null
    few = evaluate.json_safe(evaluate.kinetic_rows(real[:3], [fakes[0][:3]], 25.0, prdc_k=3))
    assert [few[k] for k in KINETIC_PRDC[:-1]] == [None] * 7 and few["prdc_k"] == 3
    json.dumps(few, allow_nan=False)


def test_phase1_evaluate_synthetic_end_to_end(tmp_path, monkeypatch, capsys):
    from music2dance_amd import kernels, runner, visualize
    from music2dance_amd.phase1 import evaluate as E1
    assert list(E1.KEYS) == P1_KEYS
    cfg = yaml.safe_load(open(os.path.join(PKG, "phase1/configs/b1l10s32.yaml")))
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    seen = {}

    def render(poses, height=300, width=300, out=None):     # no device: white frames of the asked size
        seen["poses"] = tuple(poses.shape)
        return torch.full((poses.shape[0], height, width, 3), 255, dtype=torch.uint8)

    def encode(frames, qtabs, capacity):
        seen["frames"] = tuple(frames.shape)
        data = b"\xff\xd8stub\xff\xd9"
        return torch.tensor(list(data), dtype=torch.uint8), torch.tensor([0, len(data)], dtype=torch.int64)

    prev = kernels.set_impl(KnnFakeKernels())
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    monkeypatch.setattr(visualize, "render", render)
    monkeypatch.setattr(visualize, "_encode_device", encode)
    try:
        logdir = tmp_path / "run"
        argv = ["-c", str(path), "-l", str(logdir), "--synthetic", "--samples", "48", "--k", "3", "--sheet", "7"]
        res = E1.main(argv)
        again = E1.main(argv)
    finally:
        kernels.set_impl(prev)
    printed = capsys.readouterr().out.strip().splitlines()
    strict = lambda s: json.loads(s, parse_constant=lambda c: pytest.fail("not strict JSON: %s" % c))
    on_disk = strict((logdir / "evaluation.json").read_text())
    assert list(on_disk) == P1_KEYS and strict(printed[-1]) == on_disk
    assert list(res) == P1_KEYS and E1.json_safe(again) == on_disk            # seeded: the same run twice
    assert on_disk["k"] == 3 and on_disk["n_fake"] == 48 and on_disk["n_real"] == 4 * 48 and on_disk["checkpoint"] is None
    assert on_disk["fd_pose_converged"] is True and on_disk["fd_pose"] > on_disk["fd_pose_real_split"]
    for key in P1_KEYS[:11]:
        assert on_disk[key] is None or isinstance(on_disk[key], float), key
    for s in ("precision", "recall", "density", "coverage"):
        assert 0.0 < on_disk["%s_real_split" % s] <= 1.5, s
    poses = np.load(logdir / "samples" / "poses.npy")
    assert poses.shape == (48, 69) and poses.dtype == np.float32
    assert seen["poses"] == (7, 69) and seen["frames"] == (1, 3 * 300, 3 * 300, 3)    # 7 poses: 3 columns, 3 rows
    assert (logdir / "samples" / "sheet.jpg").read_bytes() == b"\xff\xd8stub\xff\xd9"
    # the scores are the numpy statement's of the rows the script saved
    g = torch.Generator().manual_seed(1)
    real = torch.rand(4 * 48, 69, generator=g).numpy()
    want = K.prdc(real, poses, 3)
    assert {k: on_disk[k] for k in K.PRDC_KEYS} == pytest.approx(want, rel=1e-6, nan_ok=True)


def test_sheet_grid_is_in_reading_order():
    from music2dance_amd.phase1 import evaluate as E1
    frames = torch.arange(5, dtype=torch.uint8).reshape(5, 1, 1, 1).expand(5, 2, 4, 3).contiguous()
    grid = E1.sheet_grid(frames)
    assert tuple(grid.shape) == (1, 4, 12, 3) and grid.is_contiguous()
    assert grid[0, :2, :, 0].tolist() == [[0] * 4 + [1] * 4 + [2] * 4] * 2
    assert grid[0, 2:, :, 0].tolist() == [[3] * 4 + [4] * 4 + [255] * 4] * 2


def test_a_checkpoint_is_needed_without_synthetic(tmp_path):
    from music2dance_amd.phase1 import evaluate as E1
    (tmp_path / "models").mkdir()
    for n in (5, 20, 10):
        (tmp_path / "models" / ("gen_%d.pt" % n)).write_bytes(b"")
    (tmp_path / "models" / "critic_25.pt").write_bytes(b"")
    assert E1.latest_checkpoint(str(tmp_path)).endswith("gen_20.pt")
    assert E1.latest_checkpoint(str(tmp_path / "models")) is None
