"""m2d_randn_frames: standard normals indexed by (seed, row, absolute frame, channel) - the same draws whatever
chunks the frames are asked for in, different seeds differ, and the moments are those of N(0, 1)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def K():
    from music2dance_amd import kernels
    return kernels.impl()


@pytest.mark.parametrize("C", [10, 3, 4, 1])
def test_draws_do_not_depend_on_the_chunking(C):
    B, T, seed = 3, 257, 1234
    whole = K().randn_frames(seed, 0, B, T, C, DEV)
    for split in ([1] * 40 + [T - 40], [7] * 36 + [5], [100, 157], [256, 1]):
        parts, f = [], 0
        for n in split:
            parts.append(K().randn_frames(seed, f, B, n, C, DEV))
            f += n
        assert f == T
        assert torch.equal(torch.cat(parts, 1), whole), split
    # a late window alone (a stream resumed at frame 10 000)
    late = K().randn_frames(seed, 10000, B, 5, C, DEV)
    assert torch.equal(late, K().randn_frames(seed, 0, B, 10005, C, DEV)[:, 10000:])


def test_seeds_and_rows_differ():
    a = K().randn_frames(1, 0, 2, 50, 10, DEV)
    b = K().randn_frames(2, 0, 2, 50, 10, DEV)
    assert not torch.equal(a, b)
    assert (a != b).float().mean() > 0.99
    assert (a[0] != a[1]).float().mean() > 0.99
    assert torch.equal(a, K().randn_frames(1, 0, 2, 50, 10, DEV))   # deterministic
    big = K().randn_frames((1 << 40) + 1, 0, 1, 50, 10, DEV)         # the seed's high word is used
    assert not torch.equal(big, K().randn_frames(1, 0, 1, 50, 10, DEV))


def test_moments_over_a_million_draws():
    x = K().randn_frames(99, 0, 4, 25000, 10, DEV).double()
    n = x.numel()
    assert n == 10 ** 6
    assert torch.isfinite(x).all()
    mean, std = float(x.mean()), float(x.std())
    # 5 sigma sampling bounds: mean ~ N(0, 1/n), std ~ N(1, 1/(2n))
    assert abs(mean) < 5 / math.sqrt(n), mean
    assert abs(std - 1.0) < 5 / math.sqrt(2 * n), std
    # tails: P(|z| > 3) = 0.0027
    frac = float((x.abs() > 3).double().mean())
    assert abs(frac - 0.0027) < 5 * math.sqrt(0.0027 / n), frac
    print("\nrandn_frames over 1e6 draws: mean %.2e std %.6f P(|z|>3) %.5f" % (mean, std, frac))
