"""Host half of the distribution scores (music2dance_amd.metrics), through the numpy stand-in of
tests/distribution_cases.py: the --frechet / --modes flags and JSON keys of phase3.evaluate, standardize, worked cases
by hand, and that the two fp64 formulations of the Frechet distance (the SVD reference and the eigen-solver form the
device uses) stay inside the bounds the device is held to."""
import json
import math

import numpy as np
import pytest
import torch

from tests import beat_cases
from tests import distribution_cases as C

TODAY = ["jerk_real_mean", "jerk_real_std", "jerk_fake_mean", "jerk_fake_std", "confusion", "style_agreement",
         "n_sequences"]
FD_KEYS = ["fd_kinetic", "fd_kinetic_real_split", "div_kinetic_real", "div_kinetic_fake", "fd_kinetic_converged",
           "kinetic_dims"]


@pytest.fixture
def stand_in(monkeypatch):
    from music2dance_amd import kernels
    monkeypatch.setattr(kernels, "impl", lambda: C.NumpyDistributionBackend())


def test_flags_parse(capsys):
    from music2dance_amd.phase3 import evaluate
    base = ["-c", "x.yaml", "-l", "run", "--classifier", "w.pt"]
    o = evaluate.parse_args(base)
    assert o.frechet is False and o.modes is None
    o = evaluate.parse_args(base + ["--frechet"])
    assert o.frechet is True and o.modes is None
    o = evaluate.parse_args(base + ["--frechet", "--modes", "3"])
    assert o.frechet is True and o.modes == 3
    for bad in (["--modes", "3"], ["--frechet", "--modes", "1"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(base + bad)
    capsys.readouterr()


def test_the_ctypes_table_has_the_entry_points():
    from music2dance_amd import _lib
    for name in ("m2d_kinetic_features", "m2d_feature_moments", "m2d_sym_eig", "m2d_sym_eig_max_dim",
                 "m2d_sym_eig_workspace_bytes", "m2d_frechet", "m2d_frechet_workspace_bytes",
                 "m2d_pairwise_mean_dist", "m2d_pairwise_mean_dist_workspace_bytes"):
        assert name in _lib.SIGNATURES
    names = list(_lib.SIGNATURES)
    assert names.index("m2d_kinetic_features") == names.index("m2d_beat_align") + 1      # the header's position


def _sets(N, K):
    """real (N, T, 69) and K generated sets, as evaluate hands them to kinetic_rows"""
    rng = np.random.default_rng(4)
    real = torch.from_numpy(np.cumsum(rng.standard_normal((N, 30, 69)), axis=1).astype(np.float32))
    fakes = [torch.from_numpy(np.cumsum(1.5 * rng.standard_normal((N, 30, 69)), axis=1).astype(np.float32))
             for _ in range(K)]
    return real, fakes


def test_summary_keys_with_and_without_the_flags(stand_in):
    from music2dance_amd.phase3 import evaluate
    jerk = np.array([1.0, 2.0, 3.0, 5.0])
    pred = np.array([0, 1, 2, 3])
    off = evaluate.summary(jerk, jerk, pred, pred)
    assert list(off) == TODAY

    real, fakes = _sets(12, 3)
    kin = evaluate.kinetic_rows(real, fakes[:1], 25.0)
    on = evaluate.summary(jerk, jerk, pred, pred, kinetic=kin)
    assert list(on) == TODAY + FD_KEYS and {k: on[k] for k in TODAY} == off
    assert on["kinetic_dims"] == 69 and on["fd_kinetic_converged"] is True
    assert isinstance(on["kinetic_dims"], int) and isinstance(on["fd_kinetic_converged"], bool)
    for k in FD_KEYS[:4]:
        assert isinstance(on[k], float) and math.isfinite(on[k]), k
    assert on["div_kinetic_real"] > 0 and on["div_kinetic_fake"] > 0
    assert on["fd_kinetic"] > on["fd_kinetic_real_split"]          # wider steps against the sampling floor
    # the values are the fp64 statement's on the standardised features
    Fr, Ff = C.kinetic(real.numpy().reshape(12, 30, 23, 3)), C.kinetic(fakes[0].numpy().reshape(12, 30, 23, 3))
    m, S = C.moments(Fr.astype(np.float32))
    Zr = ((Fr.astype(np.float32) - m) / np.sqrt(np.diag(S))).astype(np.float32)
    Zf = ((Ff.astype(np.float32) - m) / np.sqrt(np.diag(S))).astype(np.float32)
    assert on["fd_kinetic"] == pytest.approx(C.fd_eigh(*C.moments(Zr), *C.moments(Zf))[0], rel=1e-9)
    assert on["fd_kinetic_real_split"] == pytest.approx(C.fd_eigh(*C.moments(Zr[0::2]), *C.moments(Zr[1::2]))[0], rel=1e-9)
    assert on["div_kinetic_fake"] == pytest.approx(C.pairwise(Zf)[0], rel=1e-12)

    modes = evaluate.summary(jerk, jerk, pred, pred, kinetic=evaluate.kinetic_rows(real, fakes, 25.0))
    assert list(modes) == TODAY + FD_KEYS + ["multimodality_kinetic"]
    assert {k: modes[k] for k in TODAY + FD_KEYS} == on and modes["multimodality_kinetic"] > 0
    json.dumps(evaluate.json_safe(modes), allow_nan=False)


def test_undefined_values_are_null(stand_in):
    from music2dance_amd.phase3 import evaluate
    real, fakes = _sets(3, 2)
    few = evaluate.json_safe(evaluate.kinetic_rows(real, fakes, 25.0))          # 3 rows: no even / odd split
    assert few["fd_kinetic_real_split"] is None and few["fd_kinetic"] is not None
    assert few["multimodality_kinetic"] is not None and few["fd_kinetic_converged"] is True
    one = evaluate.json_safe(evaluate.kinetic_rows(real[:1], [f[:1] for f in fakes], 25.0))
    assert [one[k] for k in FD_KEYS[:5]] == [None] * 5 and one["kinetic_dims"] == 69
    assert one["multimodality_kinetic"] is None
    json.dumps(one, allow_nan=False)


def test_standardize_with_a_zero_variance_column():
    from music2dance_amd import metrics
    X = torch.tensor([[1.0, 5.0, 2.0], [3.0, 5.0, 6.0], [5.0, 5.0, 10.0]])
    mean = torch.tensor([3.0, 5.0, 6.0], dtype=torch.float64)
    cov = torch.diag(torch.tensor([4.0, 0.0, 16.0], dtype=torch.float64))
    Z = metrics.standardize(X, mean, cov)
    assert Z.dtype == torch.float32 and Z.is_contiguous()
    assert torch.equal(Z, torch.tensor([[-1.0, 0.0, -1.0], [0.0, 0.0, 0.0], [1.0, 0.0, 1.0]]))
    other = metrics.standardize(torch.tensor([[3.0, 7.0, 6.0]]), mean, cov)      # divided by 1, not by 0
    assert torch.equal(other, torch.tensor([[0.0, 2.0, 0.0]]))


def test_frechet_of_diagonal_covariances_by_hand(stand_in):
    from music2dance_amd import metrics
    m1, m2 = torch.tensor([1.0, 2.0], dtype=torch.float64), torch.tensor([0.0, 0.0], dtype=torch.float64)
    S1 = torch.diag(torch.tensor([4.0, 9.0], dtype=torch.float64))
    S2 = torch.diag(torch.tensor([1.0, 16.0], dtype=torch.float64))
    r = metrics.frechet_from_moments(m1, S1, m2, S2)
    # |dm|^2 + sum (sqrt a_i - sqrt b_i)^2 = 5 + (2 - 1)^2 + (3 - 4)^2
    assert float(r["fd"]) == pytest.approx(7.0, abs=1e-12) and r["fd"].dim() == 0
    assert float(r["mean_term"]) == 5.0 and float(r["trace_term"]) == 30.0
    assert float(r["sqrt_term"]) == pytest.approx(2.0 + 12.0, abs=1e-12) and float(r["converged"]) == 1.0
    both = metrics.frechet_from_moments(torch.stack([m1, m2]), torch.stack([S1, S2]), torch.stack([m2, m2]),
                                        torch.stack([S2, S2]))
    assert tuple(both["fd"].shape) == (2,) and float(both["fd"][0]) == pytest.approx(7.0, abs=1e-12)
    assert float(both["fd"][1]) == pytest.approx(0.0, abs=1e-12)


def test_diversity_of_three_points_by_hand(stand_in):
    from music2dance_amd import metrics
    X = torch.tensor([[0.0, 0.0], [3.0, 4.0], [0.0, 8.0]])
    d = metrics.mean_pairwise_distance(X)                  # distances 5, 8, 5
    assert tuple(d.shape) == (1,) and d.dtype == torch.float64 and float(d[0]) == pytest.approx(6.0, abs=1e-14)
    g = metrics.mean_pairwise_distance(torch.cat([X, X[:1], X[2:], X[:1]]), groups=2)
    assert float(g[0]) == pytest.approx(6.0, abs=1e-14) and float(g[1]) == pytest.approx(16.0 / 3.0, abs=1e-14)
    assert math.isnan(float(metrics.mean_pairwise_distance(X, groups=3)[0]))       # K = 1


def test_sym_eig_shapes_through_the_stand_in(stand_in):
    from music2dance_amd import metrics
    A = torch.tensor([[2.0, 1.0], [1.0, 2.0]], dtype=torch.float64)
    one = metrics.sym_eig(A, vectors=True)
    assert one["values"].tolist() == pytest.approx([1.0, 3.0]) and tuple(one["vectors"].shape) == (2, 2)
    assert one["sweeps"].dim() == 0 and float(one["converged"]) == 1.0
    assert torch.allclose(A @ one["vectors"], one["vectors"] * one["values"])          # eigenvectors are columns
    two = metrics.sym_eig(torch.stack([A, 2.0 * A]))
    assert set(two) == {"values", "sweeps", "converged"} and tuple(two["values"].shape) == (2, 2)
    assert two["values"][1].tolist() == pytest.approx([2.0, 6.0]) and tuple(two["converged"].shape) == (2,)


def test_kinetic_features_of_a_uniform_motion_by_hand(stand_in):
    from music2dance_amd import metrics
    t = np.arange(5, dtype=np.float32)
    p = np.zeros((1, 5, 2, 3), dtype=np.float32)
    p[0, :, 0] = t[:, None] * np.array([0.25, 0.5, 0.0], dtype=np.float32)       # constant velocity
    p[0, :, 1, 1] = 0.125 * t * t                                                 # constant vertical acceleration
    F = metrics.kinetic_features(torch.from_numpy(p), fps=4.0, up_axis=1)
    assert tuple(F.shape) == (1, 6) and F.dtype == torch.float32
    # [h_0, h_1 | v_0, v_1 | e_0, e_1]: speeds (1, 2, 0) and vertical speeds 0.5 (2 t - 1), acceleration 0.25 * 16
    assert F[0].tolist() == pytest.approx([1.0, 0.0, 4.0, (0.25 + 2.25 + 6.25 + 12.25) / 4, 0.0, 4.0])
    flat = metrics.kinetic_features(torch.from_numpy(p).reshape(5, 6), fps=4.0)   # one dance, (T, 3 J)
    assert torch.equal(flat, F)
    side = metrics.kinetic_features(torch.from_numpy(p), fps=4.0, up_axis=0)
    assert side[0].tolist() == pytest.approx([4.0, (0.25 + 2.25 + 6.25 + 12.25) / 4, 1.0, 0.0, 0.0, 4.0])
    assert beat_cases.dance(7, (0, 0, 0)).shape == (3, 120, 23, 3)                # the dance the GPU test shares


CASES = C.FD_CASES + [C.FD_EQUAL]


@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d-%s" % c for c in CASES])
def test_the_two_fp64_formulations_agree_inside_the_device_bounds(stand_in, case):
    """metrics.frechet_distance through the stand-in is the eigen-solver formulation in fp64 numpy; C.fd_svd is the
    reference. The reference alone has to pass what the device is held to."""
    from music2dance_amd import metrics
    X1, X2 = C.fd_pair(case)
    if case is C.FD_EQUAL:
        X2 = X1
    ref, scale = C.fd_svd(X1, X2)
    r = metrics.frechet_distance(torch.from_numpy(X1), torch.from_numpy(X2))
    err = abs(float(r["fd"]) - ref) / scale
    bound = C.fd_bound(case[3], case[2])
    print("fd %s: svd %.9g, eigh form %.9g, |diff| / scale %.3e (bound %.3e)" % (case, ref, float(r["fd"]), err, bound))
    assert float(r["mean_term"]) + float(r["trace_term"]) == pytest.approx(scale, rel=1e-13)
    assert err <= bound
    rank = min(case[0], case[1]) - 1
    assert (rank < case[2]) == (case[3] == "deficient")
    if case is C.FD_EQUAL:
        assert float(r["mean_term"]) == 0.0 and abs(ref) <= bound * scale
