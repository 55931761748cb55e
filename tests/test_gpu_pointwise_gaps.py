"""Op-level tests of the C-ABI entries no other GPU test calls directly: m2d_tanh_fwd / _bwd / _bwd_bwd (and ops.tanh
under a double backward), m2d_jerk_mean_fwd, m2d_affine_cols, m2d_bn_update_running. References are plain fp64 torch
expressions on the CPU; the bound is the "1e-6-level for elementwise kernels" of tests/test_gpu_kernels.py
(err = max|got - ref64| / max(1, max|ref64|) < 1e-6) unless a test says otherwise. The kernels hold no contraction: an
fp32 result a few roundings away from the fp64 one is 1e-7-level, 1e-6 leaves room for the 2-ulp tanhf only."""
import pytest
import torch

from tests.test_gpu_kernels import DEV, K, gen, rel_err

pytestmark = pytest.mark.gpu

WORST = {}
TOL = 1e-6
DENORMAL = 1e-40
SPECIALS = [0.0, 1e-8, -1e-8, 20.0, -20.0, DENORMAL, -DENORMAL, 0.5, -9.0, 88.0]


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))
    return val


def _tanh_input(n):
    """seeded values over tanh's whole bend, the special inputs in front as far as they fit, zero first"""
    x = gen(n, seed=1, scale=3.0)
    m = min(n, len(SPECIALS))
    x[:m] = torch.tensor(SPECIALS[:m])
    return x


# ----------------------------------------------------------------------------------------------------------- tanh heads
@pytest.mark.parametrize("n", [1, 255, 257, 25000, 1920000])
def test_tanh_fwd(n):
    x = _tanh_input(n)
    y = K().tanh_fwd(x.to(DEV))
    ref = torch.tanh(x.double())
    assert y.shape == x.shape and y.dtype == torch.float32
    assert note("tanh_fwd", rel_err(y, ref)) < TOL
    assert float(y[0]) == 0.0


def test_tanh_fwd_special_inputs_one_by_one():
    """0 -> 0; +-1e-8 -> themselves to 1e-6 of their own size (not of 1.0); +-20 and 88 saturate to +-1 without a NaN; a
    denormal comes back as itself or, flushed, as zero"""
    x = torch.tensor(SPECIALS)
    y = K().tanh_fwd(x.to(DEV)).cpu().double()
    ref = torch.tanh(x.double())
    assert torch.isfinite(y).all()
    assert ((y - ref).abs() <= TOL * ref.abs() + 1e-37).all(), (y, ref)
    assert y[3] == 1.0 and y[4] == -1.0 and y[9] == 1.0


@pytest.mark.parametrize("n", [1, 255, 257, 25000, 1920000])
def test_tanh_bwd_and_bwd_bwd(n):
    """gx = gy (1 - y^2) and g_y = -2 y g gy, both evaluated in fp64 on the fp32 y the forward stored"""
    k = K()
    y = k.tanh_fwd(_tanh_input(n).to(DEV))
    gy, g = gen(n, seed=2), gen(n, seed=3)
    y64 = y.cpu().double()
    gx = k.tanh_bwd(gy.to(DEV), y)
    assert note("tanh_bwd", rel_err(gx, gy.double() * (1.0 - y64 * y64))) < TOL
    g_y = k.tanh_bwd_bwd(g.to(DEV), gy.to(DEV), y)
    assert note("tanh_bwd_bwd", rel_err(g_y, -2.0 * y64 * g.double() * gy.double())) < TOL


@pytest.mark.parametrize("shape", [(7, 33), (300, 100)], ids=str)
def test_ops_tanh_under_a_double_backward(shape):
    """the gradient penalty's use of a tanh head: d/dx sum (d(y . c)/dx)^2 against fp64 autograd of torch.tanh"""
    from music2dance_amd import ops
    x, c = gen(*shape, seed=1, scale=1.5), gen(*shape, seed=2)

    def second_order(tanh, x, c):
        x = x.requires_grad_(True)
        (gx,) = torch.autograd.grad((tanh(x) * c).sum(), x, create_graph=True)
        (g2,) = torch.autograd.grad(gx.pow(2).sum(), x)
        return gx.detach(), g2

    gx, g2 = second_order(ops.tanh, x.to(DEV), c.to(DEV))
    gx64, g264 = second_order(torch.tanh, x.double(), c.double())
    assert note("ops.tanh first order", rel_err(gx, gx64)) < 1e-5
    assert note("ops.tanh second order", rel_err(g2, g264)) < 1e-5


# ----------------------------------------------------------------------------------------------------------- jerkiness
def _jerk_ref(x_bct):
    x = x_bct.double()
    d = x[:, :, 3:] - 3.0 * x[:, :, 2:-1] + 3.0 * x[:, :, 1:-2] - x[:, :, :-3]
    return (d * d).sum(1).mean()


@pytest.mark.parametrize("shape", [(3, 69, 4), (2, 5, 5), (3, 69, 120), (64, 69, 120)], ids=str)
def test_jerk_mean_fwd_in_both_layouts(shape):
    from music2dance_amd import ops
    B, C, T = shape
    k = K()
    x = gen(B, C, T, seed=1)
    ref = _jerk_ref(x)
    got = k.jerk_mean_fwd(x.to(DEV), B, C, T, C * T, T, 1)
    assert got.dim() == 0
    assert note("jerk_mean_fwd (B, C, T)", rel_err(got, ref)) < TOL
    # the generator's native layout: dense (B, T, C) storage seen as (B, C, T)
    base = gen(B, T, C, seed=2)
    ref = _jerk_ref(base.permute(0, 2, 1))
    got = k.jerk_mean_fwd(base.to(DEV), B, C, T, T * C, 1, C)
    assert note("jerk_mean_fwd (B, T, C)", rel_err(got, ref)) < TOL
    assert torch.equal(ops.jerk_mean(base.to(DEV).permute(0, 2, 1)), got)
    assert torch.equal(ops.jerk_mean(x.to(DEV)), k.jerk_mean_fwd(x.to(DEV), B, C, T, C * T, T, 1))


def test_jerk_mean_fwd_refuses_three_frames_before_any_launch():
    from music2dance_amd import _lib
    h = _lib.lib()
    x = gen(2, 5, 3, seed=1).to(DEV)
    out = torch.full((), -7.0, device=DEV)
    nws = h.m2d_reduce_workspace_bytes()
    ws = torch.full((nws // 4,), -7.0, device=DEV)
    rc = h.m2d_jerk_mean_fwd(x.data_ptr(), out.data_ptr(), 2, 5, 3, 15, 3, 1, ws.data_ptr(), nws,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == -1, h.m2d_last_error()   # M2D_ERR_ARG
    torch.cuda.synchronize()
    assert float(out) == -7.0 and bool((ws == -7.0).all())   # neither the partials nor the result were written
    with pytest.raises(_lib.M2dError, match=r"\(-1\)"):
        K().jerk_mean_fwd(x, 2, 5, 3, 15, 3, 1)


# ----------------------------------------------------------------------------------------------------------- MinMax scaling
@pytest.mark.parametrize("rows", [0, 1, 7680])
@pytest.mark.parametrize("cols", [1, 69, 250])
def test_affine_cols_is_two_separately_rounded_operations(rows, cols):
    x = gen(rows, cols, seed=1, scale=3.0)
    scale, shift = gen(cols, seed=2).abs().add(0.37), gen(cols, seed=3)
    want = x * scale          # rounded to fp32 ...
    want = want + shift       # ... before the sum: no fused multiply-add
    k = K()
    xd = x.to(DEV)
    y = k.affine_cols(xd, scale.to(DEV), shift.to(DEV))
    assert y.shape == x.shape and y is not xd
    assert torch.equal(y.cpu(), want)
    assert torch.equal(xd.cpu(), x)
    y2 = k.affine_cols(xd, scale.to(DEV), shift.to(DEV), out=xd)
    assert y2 is xd and torch.equal(xd.cpu(), want)


# ----------------------------------------------------------------------------------------------------------- BatchNorm buffers
@pytest.mark.parametrize("C", [3, 256, 1024])
def test_bn_update_running_replays_a_second_forward(C):
    """After bn_fwd_sums on a batch, m2d_bn_update_running with the same sums leaves the running buffers bit-equal to a
    second bn_fwd_sums of that batch; and both equal the fp64 recurrence (momentum 0.1, unbiased variance)."""
    B, L, eps, mom = 6, 5, 1e-5, 0.1
    k = K()
    x = (gen(B, C, L, seed=1) * 1.5 + 0.3).to(DEV)
    g, bt = gen(C, seed=2).abs().add(0.5).to(DEV), gen(C, seed=3, scale=0.2).to(DEV)
    rm0, rv0 = gen(C, seed=4, scale=0.1), 1.0 + gen(C, seed=5, scale=0.1).abs()
    n = B * L
    sums = k.bn_stats(x)
    rm_a, rv_a = rm0.to(DEV), rv0.to(DEV)
    k.bn_fwd_sums(x, sums, n, g, bt, rm_a, rv_a, eps, mom)
    rm_b, rv_b = rm_a.clone(), rv_a.clone()
    k.bn_update_running(sums, n, rm_a, rv_a, eps, mom)
    k.bn_fwd_sums(x, sums, n, g, bt, rm_b, rv_b, eps, mom)
    assert torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b)
    x64 = x.cpu().double()
    mean, var = x64.mean((0, 2)), x64.var((0, 2), unbiased=True)
    rm64, rv64 = rm0.double(), rv0.double()
    for _ in range(2):
        rm64 = (1 - mom) * rm64 + mom * mean
        rv64 = (1 - mom) * rv64 + mom * var
    assert not torch.equal(rm_a.cpu(), rm0)
    assert note("bn_update_running mean", rel_err(rm_a, rm64)) < TOL
    assert note("bn_update_running var", rel_err(rv_a, rv64)) < TOL
