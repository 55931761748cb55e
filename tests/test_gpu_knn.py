"""The nearest-neighbour kernels on the device (m2d_knn_radii, m2d_ball_query, metrics.prdc, phase1.evaluate,
phase3.evaluate --prdc) against the fp64 numpy statement of tests/knn_cases.py: radii inside (D + 4) 2^-24 of fp64 for
every row; counts between the pairs decided inside and the pairs possibly inside at that bound, with the device's own
radii on both sides; an integer lattice where everything is exact, ties at the radius and duplicated rows included;
the scores end to end; bit-level symmetry, independence of the other queries and of a row's position, repeatability;
the argument errors; and the two scripts. Every measured figure is recorded with `note` and printed in the terminal summary
of a run."""
import json
import math
import os
import struct

import numpy as np
import pytest
import torch

from tests import knn_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
_CACHE = {}


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def M():
    from music2dance_amd import metrics
    return metrics


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def ball_inputs(case):
    """(R, F) on the host and the fp64 distances [j][i] of F rows to R rows: made once per case"""
    if case not in _CACHE:
        R, F = K.split_case(*case)
        _CACHE[case] = (R, F, K.d2_matrix(F, R))
    return _CACHE[case]


# ------------------------------------------------------------------------------------------------ radii
@pytest.mark.parametrize("case", K.RADII_CASES, ids=["%dx%d-k%d" % c for c in K.RADII_CASES])
def test_radii_against_fp64(case):
    N, D, k = case
    X = K.radii_input(N, D)
    ref = K.radii(X, k)
    if case == K.RADII_CASES[0]:                      # a column block of a wider buffer, taken in place
        wide = torch.full((N, D + 11), float("nan"), device=DEV)
        wide[:, 3:3 + D] = dev(X)
        Xd = wide[:, 3:3 + D]
        assert Xd.stride(0) == D + 11 and not Xd.is_contiguous()
    else:
        Xd = dev(X)
    r2 = M().knn_radii(Xd, k)
    assert r2.dtype == torch.float32 and tuple(r2.shape) == (N,)
    got = r2.cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(got - ref) / ref))
    print("radii %s: max |r2 - ref| / ref = %.3e (bound %.3e)" % (case, err, K.eps(D)))
    note("radii max |r2 - ref| / ref (bound %.2e)  N %d D %d k %d" % ((K.eps(D),) + case), err)
    assert np.all(np.abs(got - ref) <= K.eps(D) * ref)


def test_the_1500_row_case_splits_the_reference_range():
    """the workspace of the (1500, 69, 3) case holds more than one partial list per row: the merge launch is exercised"""
    from music2dance_amd._lib import lib
    assert lib().m2d_knn_radii_workspace_bytes(1500, 3) > 1500 * lib().m2d_knn_max_k() * 4
    assert lib().m2d_ball_query_workspace_bytes(64, 1500) > 64 * 12
    assert lib().m2d_knn_max_k() >= 10 and K.MAX_K == lib().m2d_knn_max_k()


# ------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize("case", K.BALL_CASES, ids=["%dx%dx%d+%g" % c for c in K.BALL_CASES])
def test_ball_query_against_fp64(case):
    N, Mq, D, _ = case
    R, F, d = ball_inputs(case)
    Rd, Fd = dev(R), dev(F)
    r2 = M().knn_radii(Rd, 5)
    count, nn_d2, nn_idx = M().ball_query(Fd, Rd, r2)
    assert count.dtype == torch.int32 and nn_idx.dtype == torch.int32 and nn_d2.dtype == torch.float32
    assert tuple(count.shape) == tuple(nn_d2.shape) == tuple(nn_idx.shape) == (Mq,)
    e = K.eps(D)
    r64 = r2.cpu().numpy().astype(np.float64)
    lo = (d <= (r64 * (1.0 - e))[None, :]).sum(axis=1)
    hi = (d <= (r64 * (1.0 + e))[None, :]).sum(axis=1)
    undecided = int((lo != hi).sum())
    print("ball %s: %d of %d queries undecided at eps %.2e" % (case, undecided, Mq, e))
    assert undecided <= 0.01 * Mq                     # a condition on the inputs, not a tolerance
    c = count.cpu().numpy()
    assert np.all(lo <= c) and np.all(c <= hi)
    mn = d.min(axis=1)
    got = nn_d2.cpu().numpy().astype(np.float64)
    err = float(np.max(np.abs(got - mn) / mn))
    note("ball max |nn_d2 - min| / min (bound %.2e)  N %d M %d D %d shift %g" % ((e,) + case), err)
    assert np.all(np.abs(got - mn) <= e * mn)
    idx = nn_idx.cpu().numpy()
    assert np.all((idx >= 0) & (idx < N))
    assert np.all(d[np.arange(Mq), idx] <= mn * (1.0 + e))
    # without radii: no counts, the same nearest rows
    none, nn2, idx2 = M().ball_query(Fd, Rd)
    assert none is None and torch.equal(nn2, nn_d2) and torch.equal(idx2, nn_idx)


# ------------------------------------------------------------------------------------------------ lattice: exact
@pytest.mark.parametrize("k", [1, 3])
def test_lattice_is_exact(k):
    R, F = K.lattice()
    Rd, Fd = dev(R), dev(F)
    ref_r = K.radii(R, k)
    r2 = M().knn_radii(Rd, k)
    assert torch.equal(r2.cpu(), torch.from_numpy(ref_r.astype(np.float32)))
    if k == 1:
        assert np.all(ref_r[:20] == 0.0) and np.all(ref_r[100:120] == 0.0)      # the duplicated rows
    ties = int((K.d2_matrix(F, R) == ref_r[None, :]).sum())
    assert ties >= 40, ties                          # pairs exactly at the radius: the comparison is inclusive
    for Q, P, rr in ((F, R, ref_r), (R, F, K.radii(F, k)), (R, R, ref_r)):
        cnt, nn, idx = K.ball(Q, P, rr)
        c, n, i = M().ball_query(dev(Q), dev(P), dev(rr.astype(np.float32)))
        assert torch.equal(c.cpu(), torch.from_numpy(cnt.astype(np.int32)))
        assert torch.equal(n.cpu(), torch.from_numpy(nn.astype(np.float32)))
        assert torch.equal(i.cpu(), torch.from_numpy(idx.astype(np.int32)))    # the smallest index of a tie
    want = K.prdc(R, F, k)
    got = M().prdc(Rd, Fd, k)
    assert list(got) == K.PRDC_KEYS
    for key in K.PRDC_KEYS:
        assert got[key].dtype == torch.float64 and got[key].dim() == 0 and got[key].is_cuda
    for key in ("precision", "recall", "density", "coverage"):
        assert abs(float(got[key]) - want[key]) <= 1e-15, (key, float(got[key]), want[key])
    for key in K.PRDC_KEYS[4:]:
        a, b = float(got[key]), want[key]
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-15 * max(1.0, abs(b)), (key, a, b)
    print("lattice k %d: P %.3f R %.3f D %.3f C %.3f, %d ties" % (k, want["precision"], want["recall"],
                                                                 want["density"], want["coverage"], ties))


# ------------------------------------------------------------------------------------------------ scores end to end
@pytest.mark.parametrize("case,k", [((257, 300, 69, 0.0), 5), ((257, 300, 69, 0.5), 5), ((40, 33, 3, 0.0), 2)],
                         ids=["shift0", "shift0.5", "tiny"])
def test_prdc_equals_the_numpy_statement(case, k):
    N, Mq, D, _ = case
    R, F, d = ball_inputs(case)
    want = K.prdc(R, F, k)
    got = {key: float(v) for key, v in M().prdc(dev(R), dev(F), k).items()}
    # a pair whose decision fp32 may take the other way: d2 / r2 inside [(1 - e) / (1 + e), (1 + e) / (1 - e)]
    e = K.eps(D)
    lo_f, hi_f = (1.0 - e) / (1.0 + e), (1.0 + e) / (1.0 - e)
    rR, rF = K.radii(R, k), K.radii(F, k)
    band_R = (d >= lo_f * rR[None, :]) & (d <= hi_f * rR[None, :])           # [j][i] against the real radii
    band_F = (d >= lo_f * rF[:, None]) & (d <= hi_f * rF[:, None])
    mn = d.min(axis=0)
    slack = {"precision": band_R.any(axis=1).sum() / Mq, "density": band_R.sum() / (k * Mq),
             "recall": band_F.any(axis=0).sum() / N,
             "coverage": ((mn >= lo_f * rR) & (mn <= hi_f * rR)).sum() / N}
    print("prdc %s k %d: P %.3f R %.3f D %.3f C %.3f ratio %.3f; undecided shares %s"
          % (case, k, want["precision"], want["recall"], want["density"], want["coverage"], want["nn_ratio_median"],
             {s: float(v) for s, v in slack.items()}))
    for key, s in slack.items():
        if s == 0:
            assert got[key] == want[key], (key, got[key], want[key])
        else:
            assert abs(got[key] - want[key]) <= s + 1e-15, (key, got[key], want[key], s)
    for key in ("nn_fake_to_real_median", "nn_real_to_real_median"):         # an order statistic of values each within e / 2
        assert abs(got[key] - want[key]) <= e * want[key], (key, got[key], want[key])
    assert abs(got["nn_ratio_median"] - want["nn_ratio_median"]) <= 2.0 * e * want["nn_ratio_median"]


def test_identical_sets():
    R, _, _ = ball_inputs(K.BALL_CASES[0])
    got = M().prdc(dev(R), dev(R), 5)
    assert float(got["precision"]) == 1.0 and float(got["recall"]) == 1.0 and float(got["coverage"]) == 1.0
    assert float(got["nn_fake_to_real_median"]) == 0.0 and float(got["nn_ratio_median"]) == 0.0
    assert float(got["density"]) >= 1.0               # every row lies in its own ball and in k others' on average


# ------------------------------------------------------------------------------------------------ bits
def test_symmetry_of_the_distance():
    X = dev(K.radii_input(257, 69))
    for i in range(8):
        a, b = X[i:i + 1], X[100 + i:101 + i]
        ab, ba = M().ball_query(a, b)[1], M().ball_query(b, a)[1]
        assert torch.equal(ab, ba) and float(ab) > 0


def test_a_query_row_does_not_depend_on_the_other_queries():
    R, F, _ = ball_inputs((1500, 64, 69, 0.0))        # 24 reference tiles: the range is split
    Rd, Fd = dev(R), dev(F)
    r2 = M().knn_radii(Rd, 3)
    full = M().ball_query(Fd, Rd, r2)
    part = M().ball_query(Fd[10:20], Rd, r2)
    again = M().ball_query(Fd, Rd, r2)
    for f, p, a in zip(full, part, again):
        assert torch.equal(f[10:20], p) and torch.equal(f, a)
    # the other regime (many query tiles, one share of the references each) gives the same bits
    big = M().ball_query(torch.cat([Fd] * 130), Rd, r2)
    for f, b in zip(full, big):
        assert torch.equal(b[:64], f) and torch.equal(b[-64:], f)


def test_a_radius_does_not_depend_on_the_position_of_its_row():
    X = dev(K.radii_input(1500, 69))
    r2 = M().knn_radii(X, 3)
    assert torch.equal(M().knn_radii(X, 3), r2)       # two runs, the same bits
    rolled = torch.roll(X, 777, dims=0).contiguous()
    assert torch.equal(M().knn_radii(rolled, 3), torch.roll(r2, 777))
    # k = 1 is the nearest other row: the query of rows [10:20] alone against the set without that row
    r1 = M().knn_radii(X, 1)
    for i in range(10, 20):
        others = torch.cat([X[:i], X[i + 1:]])
        assert torch.equal(M().ball_query(X[i:i + 1], others)[1], r1[i:i + 1])


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    from music2dance_amd import _lib
    X = dev(K.radii_input(40, 3))
    for bad in (lambda: M().knn_radii(X, 0), lambda: M().knn_radii(X, K.MAX_K + 1), lambda: M().knn_radii(X[:5], 5),
                lambda: M().knn_radii(torch.zeros(20, 129, device=DEV), 2),
                lambda: M().ball_query(torch.zeros(20, 129, device=DEV), torch.zeros(20, 129, device=DEV)),
                lambda: M().knn_radii(X.cpu(), 2), lambda: M().ball_query(X.cpu(), X),
                lambda: M().ball_query(X, X.cpu()), lambda: M().ball_query(X, X[:, :2].contiguous()),
                lambda: M().ball_query(X, X, torch.zeros(39, device=DEV))):
        with pytest.raises(_lib.M2dError):
            bad()
    torch.cuda.synchronize()


def test_a_short_workspace_is_refused_through_the_c_abi():
    """arguments only: the library returns before it launches anything"""
    from music2dance_amd import _lib
    h = _lib.lib()
    X = dev(K.radii_input(300, 69))
    out = torch.empty(300, device=DEV)
    idx = torch.empty(300, dtype=torch.int32, device=DEV)
    need = h.m2d_knn_radii_workspace_bytes(300, 5)
    ws = torch.empty(need // 4 + 1, device=DEV)
    rc = h.m2d_knn_radii(X.data_ptr(), 69, 300, 69, 5, out.data_ptr(), ws.data_ptr(), need - 1, None)
    assert rc == -3 and b"m2d_knn_radii" in h.m2d_last_error()
    rc = h.m2d_knn_radii(X.data_ptr(), 69, 300, 69, 5, out.data_ptr(), None, 0, None)
    assert rc == -3
    need = h.m2d_ball_query_workspace_bytes(300, 300)
    rc = h.m2d_ball_query(X.data_ptr(), 69, 300, X.data_ptr(), 69, 300, 69, None, None, out.data_ptr(), idx.data_ptr(),
                          ws.data_ptr(), need - 1, None)
    assert rc == -3 and b"m2d_ball_query" in h.m2d_last_error()
    rc = h.m2d_ball_query(X.data_ptr(), 69, 300, X.data_ptr(), 69, 300, 69, out.data_ptr(), None, out.data_ptr(),
                          idx.data_ptr(), ws.data_ptr(), need, None)
    assert rc == -1                                   # r2 without count
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the scripts
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P1_KEYS = (K.PRDC_KEYS + ["precision_real_split", "recall_real_split", "density_real_split", "coverage_real_split",
                          "fd_pose", "fd_pose_real_split", "fd_pose_converged", "div_pose_real", "div_pose_fake", "k",
                          "n_real", "n_fake", "checkpoint"])


def strict_json(text):
    return json.loads(text, parse_constant=lambda c: pytest.fail("non-standard JSON constant %s" % c))


def sof0_size(jpeg):
    """(height, width) of the baseline frame header (marker FFC0: length, precision, height, width)"""
    at = jpeg.index(b"\xff\xc0")
    return struct.unpack(">HH", jpeg[at + 5:at + 9])


def test_phase1_evaluate_synthetic(tmp_path):
    from music2dance_amd.phase1 import evaluate
    cfg = os.path.join(ROOT, "music2dance_amd", "phase1", "configs", "b1l10s128.yaml")
    logdir = tmp_path / "run"
    torch.manual_seed(5)                              # the randomly initialised generator
    res = evaluate.main(["-c", cfg, "-l", str(logdir), "--synthetic", "--samples", "512", "--sheet", "9"])
    out = strict_json((logdir / "evaluation.json").read_text())
    assert list(out) == P1_KEYS and list(res) == P1_KEYS
    assert out["k"] == 5 and out["n_fake"] == 512 and out["n_real"] == 2048 and out["checkpoint"] is None
    for s in ("precision", "recall", "density", "coverage"):
        v = out["%s_real_split" % s]
        note("phase1.evaluate %s_real_split (uniform rows in 69-D; in (0, 1.5])" % s, v)
        assert 0.0 < v <= 1.5, (s, v)
        assert out[s] is not None and 0.0 <= out[s], (s, out[s])
    assert out["fd_pose_converged"] is True and out["fd_pose"] > out["fd_pose_real_split"]
    assert out["div_pose_real"] > 0 and out["div_pose_fake"] >= 0
    sheet = (logdir / "samples" / "sheet.jpg").read_bytes()
    assert sheet[:2] == b"\xff\xd8" and sheet[-2:] == b"\xff\xd9" and sof0_size(sheet) == (900, 900)
    poses = np.load(logdir / "samples" / "poses.npy")
    assert poses.shape == (512, 69) and poses.dtype == np.float32 and np.isfinite(poses).all()


def test_phase3_evaluate_with_and_without_prdc(tmp_path):
    from music2dance_amd.dance_classification.archis.default import RecurrentDanceClassifier
    from music2dance_amd.phase3 import evaluate
    torch.manual_seed(3)
    cls_path = str(tmp_path / "cls.pt")
    torch.save(RecurrentDanceClassifier(69, 128, 4).state_dict(), cls_path)
    cfg = os.path.join(ROOT, "music2dance_amd", "phase3", "configs", "default.yaml")
    out, text = {}, {}
    for name, extra in (("frechet", ["--frechet"]), ("again", ["--frechet"]), ("prdc", ["--frechet", "--prdc", "3"])):
        logdir = tmp_path / name
        logdir.mkdir()
        evaluate.main(["-c", cfg, "-l", str(logdir), "--classifier", cls_path, "--repeats", "2", "--synthetic"] + extra)
        text[name] = (logdir / "evaluation.json").read_text()
        out[name] = strict_json(text[name])
    assert text["again"] == text["frechet"]           # the file without the flag, byte for byte
    new = ["%s_kinetic" % k for k in K.PRDC_KEYS] + ["prdc_k"]
    assert not [k for k in out["frechet"] if k in new]
    assert list(out["prdc"]) == list(out["frechet"]) + new
    assert {k: out["prdc"][k] for k in out["frechet"]} == out["frechet"]
    assert out["prdc"]["prdc_k"] == 3
    for k in new[:4]:
        assert out["prdc"][k] is not None and 0.0 <= out["prdc"][k], k
    assert out["prdc"]["precision_kinetic"] <= 1.0 and out["prdc"]["recall_kinetic"] <= 1.0
