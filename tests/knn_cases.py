"""The k-nearest-neighbour scores of music2dance_amd.metrics (radii, ball query, precision / recall / density /
coverage, nearest-row distances) restated in plain fp64 numpy, written from the definitions and
independently of metrics.py; the input recipes the k-NN tests share; and a numpy stand-in for the kernels. A helper,
not a test module."""
import numpy as np

from tests import distribution_cases as C

MAX_K = 10
MAX_D = 128
PRDC_KEYS = ["precision", "recall", "density", "coverage", "nn_ratio_median", "nn_fake_to_real_median",
             "nn_real_to_real_median"]


# ------------------------------------------------------------------------------------------------ the definitions
def d2_matrix(A, B):
    """(len A, len B) fp64: sum_d (a_d - b_d)^2, the differences taken directly"""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    out = np.empty((A.shape[0], B.shape[0]))
    for i in range(A.shape[0]):
        diff = B - A[i]
        out[i] = (diff * diff).sum(axis=1)
    return out


def radii(X, k):
    """r2[i] = the k-th smallest of d2(X_i, X_j) over j != i: the row itself leaves by index, a duplicate of it stays"""
    d = d2_matrix(X, X)
    n = d.shape[0]
    out = np.empty(n)
    for i in range(n):
        others = np.delete(d[i], i)
        out[i] = np.sort(others)[k - 1]
    return out


def ball(Qm, Pm, r2=None):
    """-> (count or None, nn_d2, nn_idx): count[j] = #{i : d2(Q_j, P_i) <= r2[i]}, the minimum over i and the smallest
    index that attains it"""
    d = d2_matrix(Qm, Pm)
    count = None if r2 is None else (d <= np.asarray(r2, dtype=np.float64)[None, :]).sum(axis=1)
    return count, d.min(axis=1), d.argmin(axis=1)            # (argmin returns the first minimum)


def prdc(R, F, k):
    """the seven scores of metrics.prdc from the definitions"""
    R, F = np.asarray(R, dtype=np.float64), np.asarray(F, dtype=np.float64)
    rR, rF = radii(R, k), radii(F, k)
    d = d2_matrix(F, R)                                      # [j][i]
    inside = d <= rR[None, :]
    f2r = np.sqrt(d.min(axis=1))
    r2r = np.sqrt(radii(R, 1))
    den = float(np.median(r2r))
    return {"precision": float(inside.any(axis=1).mean()),
            "recall": float((d <= rF[:, None]).any(axis=0).mean()),
            "density": float(inside.sum()) / (k * F.shape[0]),
            "coverage": float((d.min(axis=0) <= rR).mean()),
            "nn_ratio_median": float(np.median(f2r)) / den if den > 0 else float("nan"),
            "nn_fake_to_real_median": float(np.median(f2r)),
            "nn_real_to_real_median": den}


def eps(D):
    """first-order bound on the relative error of an fp32 chain of D squared fp32 differences against fp64: 2u from the
    square, D u from the chain of non-negative terms, 2u of slack; u = 2^-24"""
    return (D + 4) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the inputs
def split(seed, N, M, D, shift=0.0):
    """one gaussian(seed, N + M, D) draw: the first N rows are real, the rest plus `shift` are generated"""
    X = C.gaussian(seed, N + M, D)
    return X[:N].copy(), (X[N:] + np.float32(shift)).astype(np.float32)


def split_case(N, M, D, shift=0.0):
    return split(3000 + N + M + D, N, M, D, shift)


def lattice():
    """integer coordinates in -3..3, D = 6: every d2 is a small integer (fp32 and fp64 agree exactly), ties at the radius
    are plentiful, and rows 100..119 of R repeat rows 0..19 (radius 0 at k = 1)"""
    rng = np.random.default_rng(7)
    R = rng.integers(-3, 4, (203, 6)).astype(np.float32)
    R[100:120] = R[0:20]
    F = rng.integers(-3, 4, (150, 6)).astype(np.float32)
    return R, F


# (N, D, k) of the radii cases; (N, M, D, shift) of the ball-query cases
RADII_CASES = [(257, 69, 5), (1500, 69, 3), (300, 128, MAX_K), (97, 1, 2), (40, 3, 1), (6, 69, 5)]
BALL_CASES = [(257, 300, 69, 0.0), (257, 300, 69, 0.5), (1500, 64, 69, 0.0), (40, 33, 3, 0.0), (97, 130, 1, 0.0),
              (2100, 520, 16, 0.25), (300, 257, 128, 0.0)]


def radii_input(N, D):
    return C.gaussian(3000 + N + D, N, D)


# ------------------------------------------------------------------------------------------------ a host backend
class NumpyKnnBackend(C.NumpyDistributionBackend):
    """The HipKernels methods metrics.py calls for the distribution AND the k-NN scores, on host tensors through the
    fp64 statements (monkeypatch kernels.impl with `lambda: NumpyKnnBackend()`)"""

    def knn_max_k(self):
        return MAX_K

    def knn_radii(self, X, k):
        import torch
        if not 1 <= k <= MAX_K or X.shape[0] <= k or not 1 <= X.shape[1] <= MAX_D:
            raise ValueError("knn_radii: bad arguments")
        return torch.from_numpy(radii(X.numpy(), k).astype(np.float32))

    def ball_query(self, Qm, Pm, r2=None):
        import torch
        cnt, nn, idx = ball(Qm.numpy(), Pm.numpy(), None if r2 is None else r2.numpy())
        return (None if cnt is None else torch.from_numpy(cnt.astype(np.int32)),
                torch.from_numpy(nn.astype(np.float32)), torch.from_numpy(idx.astype(np.int32)))
