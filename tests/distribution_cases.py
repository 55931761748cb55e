"""The distribution scores of music2dance_amd.metrics (kinetic features, moments, Frechet distance, mean pairwise
distance) restated in plain fp64 numpy, written from the definitions and independently of
metrics.py; the input recipes and bounds the distribution tests share; and a numpy stand-in for the kernels. A helper,
not a test module."""
import numpy as np

MAX_DIM = 128
SWEEP_CAP = 30


# ------------------------------------------------------------------------------------------------ the definitions
def kinetic(p, fps=25.0, up_axis=1):
    """poses (B, T, J, 3) -> (B, 3 J) fp64: [mean squared horizontal speed | mean squared vertical speed | mean
    absolute acceleration] per joint, v[t] = (p[t] - p[t - 1]) fps, a[t] = (p[t + 1] - 2 p[t] + p[t - 1]) fps^2"""
    p = np.asarray(p, dtype=np.float64)
    p = p.reshape(p.shape[0], p.shape[1], -1, 3)
    v = (p[:, 1:] - p[:, :-1]) * fps
    a = (p[:, 2:] - 2.0 * p[:, 1:-1] + p[:, :-2]) * fps * fps
    hor = [c for c in range(3) if c != up_axis]
    h = (v[..., hor] ** 2).sum(axis=3).mean(axis=1)
    u = (v[..., up_axis] ** 2).mean(axis=1)
    e = np.sqrt((a ** 2).sum(axis=3)).mean(axis=1)
    return np.concatenate([h, u, e], axis=1)


def moments(X):
    """-> (mean (D), unbiased covariance (D, D)), fp64, two passes"""
    X = np.asarray(X, dtype=np.float64)
    m = X.mean(axis=0)
    Xc = X - m
    return m, Xc.T @ Xc / (X.shape[0] - 1)


def fd_terms(m1, S1, m2, S2):
    """-> (|m1 - m2|^2, tr S1 + tr S2); their sum is the `scale` the bounds are relative to"""
    d = np.asarray(m1, dtype=np.float64) - np.asarray(m2, dtype=np.float64)
    return float(d @ d), float(np.trace(S1) + np.trace(S2))


def fd_svd(X1, X2):
    """THE reference: tr (S1 S2)^1/2 is the nuclear norm of A B^T, A = X1c / sqrt(n1 - 1), B = X2c / sqrt(n2 - 1)
    (numpy.linalg.svd, fp64); no square root of a near-zero eigenvalue is taken. -> (fd, scale)"""
    X1, X2 = np.asarray(X1, dtype=np.float64), np.asarray(X2, dtype=np.float64)
    m1, S1 = moments(X1)
    m2, S2 = moments(X2)
    A = (X1 - m1) / np.sqrt(X1.shape[0] - 1.0)
    B = (X2 - m2) / np.sqrt(X2.shape[0] - 1.0)
    nuc = np.linalg.svd(A @ B.T, compute_uv=False).sum()
    dmu, tr = fd_terms(m1, S1, m2, S2)
    return dmu + tr - 2.0 * nuc, dmu + tr


def sqrt_term_eigh(S1, S2):
    """tr (S1 S2)^1/2 as the sum of sqrt(max(l, 0)) over the eigenvalues of S1^1/2 S2 S1^1/2 (numpy.linalg.eigh)"""
    w, V = np.linalg.eigh(S1)
    R = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = R @ S2 @ R
    return float(np.sqrt(np.maximum(np.linalg.eigvalsh(0.5 * (M + M.T)), 0.0)).sum())


def fd_eigh(m1, S1, m2, S2):
    """the eigen-solver formulation the device uses, in fp64 numpy -> (fd, |dm|^2, tr S1 + tr S2, tr (S1 S2)^1/2)"""
    dmu, tr = fd_terms(m1, S1, m2, S2)
    rt = sqrt_term_eigh(np.asarray(S1, dtype=np.float64), np.asarray(S2, dtype=np.float64))
    return dmu + tr - 2.0 * rt, dmu, tr, rt


def pairwise(X, groups=1):
    """-> (G,) fp64: the mean of |x_i - x_j| over the pairs i < j of each group of K consecutive rows; NaN for K < 2"""
    X = np.asarray(X, dtype=np.float64)
    K = X.shape[0] // groups
    out = np.full(groups, np.nan)
    for g in range(groups):
        Y = X[g * K:(g + 1) * K]
        if K >= 2:
            i, j = np.triu_indices(K, 1)
            out[g] = np.sqrt(((Y[i] - Y[j]) ** 2).sum(axis=1)).mean()
    return out


def fd_bound(kind, D):
    """the bound on |fd - fd_svd| / scale: 1e-10 where both covariances have full rank, D 2^-26 otherwise (up to D zero
    eigenvalues, each off by sqrt(eps))"""
    return 1e-10 if kind == "full" else D * 2.0 ** -26


# ------------------------------------------------------------------------------------------------ the inputs
def gaussian(seed, N, D):
    """(N, D) fp32: N(0, 1) rows through a random D x D mixing matrix (entries N(0, 1 / D)) plus a mean N(0, 1)"""
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((D, D)) / np.sqrt(D)
    mean = rng.standard_normal(D)
    return (rng.standard_normal((N, D)) @ mix + mean).astype(np.float32)


# (N1, N2, D, kind): full rank with an odd D (the tournament has a bye); the limit, even D; rank-deficient; tiny ones
FD_CASES = [(300, 257, 69, "full"), (200, 150, 128, "full"), (40, 50, 69, "deficient"), (33, 17, 2, "full"),
            (9, 9, 1, "full")]
FD_EQUAL = (100, 100, 69, "full")     # X2 = X1


def fd_pair(case):
    N1, N2, D = case[:3]
    return gaussian(1000 + N1 + D, N1, D), gaussian(2000 + N2 + D, N2, D)


def sym_matrix(D, kind, seed=5):
    """(D, D) fp64: M M^T ('psd') or M + M^T ('indefinite') of a standard normal M"""
    M = np.random.default_rng(seed + D).standard_normal((D, D))
    return M @ M.T if kind == "psd" else M + M.T


def random_walk(seed, T, B=2, J=23):
    """(B, T, J, 3) fp32: a random walk with N(0, 0.05^2) steps"""
    rng = np.random.default_rng(seed)
    return np.cumsum(0.05 * rng.standard_normal((B, T, J, 3)), axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ a host backend
class NumpyDistributionBackend:
    """The HipKernels methods the distribution half of metrics.py calls, on host tensors through the fp64 statement
    above (for the host tests: monkeypatch kernels.impl with `lambda: NumpyDistributionBackend()`)"""

    def sym_eig_max_dim(self):
        return MAX_DIM

    def kinetic_features(self, poses, fps=25.0, up_axis=1):
        import torch
        return torch.from_numpy(kinetic(poses.numpy(), fps, up_axis)).float()

    def feature_moments(self, X):
        import torch
        m, S = moments(X.numpy())
        return torch.from_numpy(m), torch.from_numpy(S)

    def sym_eig(self, A, vectors=False):
        import torch
        w, V = np.linalg.eigh(A.numpy())
        info = torch.tensor([[1.0, 1.0]] * A.shape[0], dtype=torch.float64)
        return torch.from_numpy(w), (torch.from_numpy(V) if vectors else None), info

    def frechet(self, mean1, cov1, mean2, cov2):
        import torch
        rows = [list(fd_eigh(mean1[p].numpy(), cov1[p].numpy(), mean2[p].numpy(), cov2[p].numpy())) + [1.0, 1.0]
                for p in range(mean1.shape[0])]
        return torch.tensor(rows, dtype=torch.float64)

    def pairwise_mean_dist(self, X, groups=1):
        import torch
        return torch.from_numpy(pairwise(X.numpy(), groups))
