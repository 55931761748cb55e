"""The phase-2 `gan` framework (-f gan) without a GPU: the C-ABI surface of the BCE-on-logits entries, the engine's
loop against an fp64 re-enactment of phase2/train.py:204-240 built from the oracle's phase-2 networks and torch's BCE
(draw order, per-iteration generator and scheduler steps, no n_critic gating), the hand-scheduled critic iteration
against the autograd one, a world-size-2 gloo run and the script surface. Kernels are the CPU stand-in of
tests/fake_backend.py, extended here by the two BCE entries."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from music2dance_amd import kernels, runner
from tests.fake_backend import FakeKernels
from tests.test_dp_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("m2d_bce_logits_fwd", "m2d_bce_logits_bwd")


class BceFakeKernels(FakeKernels):
    """FakeKernels + the BCE-on-logits pair, in torch (same contract as kernels.HipKernels)."""

    @staticmethod
    def _targets(x, n0, t0, n1, t1):
        assert x.numel() == n0 + n1
        return torch.cat((torch.full((n0,), float(t0)), torch.full((n1,), float(t1)))).to(x)

    def bce_logits_fwd(self, x, n0, t0, n1=0, t1=0.0, with_dx=False):
        t = self._targets(x, n0, t0, n1, t1)
        xs = x.reshape(-1)
        m0 = F.binary_cross_entropy_with_logits(xs[:n0], t[:n0])
        m1 = F.binary_cross_entropy_with_logits(xs[n0:], t[n0:]) if n1 else xs.new_zeros(())
        dx = None
        if with_dx:
            n = torch.cat((torch.full((n0,), float(n0)), torch.full((n1,), float(max(n1, 1))))).to(x)
            dx = ((torch.sigmoid(xs) - t) / n).view_as(x)
        return torch.stack((m0 + m1, m0, m1)), dx

    def bce_logits_bwd(self, x, n0, t0, n1, t1, gout):
        t = self._targets(x, n0, t0, n1, t1)
        n = torch.cat((torch.full((n0,), float(n0)), torch.full((n1,), float(max(n1, 1))))).to(x)
        return (gout * (torch.sigmoid(x.reshape(-1)) - t) / n).view_as(x)


@pytest.fixture
def fake():
    prev = kernels.set_impl(BceFakeKernels())
    try:
        yield
    finally:
        kernels.set_impl(prev)


def test_header_and_ctypes_table_carry_the_new_entries():
    from music2dance_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m2d.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"m2d_bce_logits_fwd\(const float\* x, int n0, float t0, int n1, float t1, float\* out, float\* dx",
                     text)
    assert _lib.SIGNATURES["m2d_bce_logits_fwd"][1][2] is _lib._f


def test_bce_op_matches_torch_on_the_stand_in(fake):
    from music2dance_amd import losses
    x = (3 * torch.randn(7, generator=torch.Generator().manual_seed(1))).requires_grad_(True)
    for t in (0.0, 1.0, 0.3):
        got = losses.bce_with_logits(x, t)
        ref = F.binary_cross_entropy_with_logits(x, torch.full_like(x, t))
        (gx,) = torch.autograd.grad(got, x)
        (rx,) = torch.autograd.grad(ref, x)
        assert torch.allclose(got, ref, atol=1e-6) and torch.allclose(gx, rx, atol=1e-7)
    with pytest.raises(TypeError):
        losses.bce_with_logits(x, torch.ones(7))


# --------------------------------------------------------------------------------------------- small networks
NZ, B, T = 8, 4, 24
CFG = {"lr_gen": 1e-3, "lr_critic": 1e-3, "n_critic_steps": 5, "gamma": 10, "eta": 50, "input_vector_size": NZ}


def _make_p2(seed=0):
    from music2dance_amd.phase2.archis.default import SequenceDiscriminator, SequenceGenerator
    torch.manual_seed(seed)
    gen = SequenceGenerator(NZ, NZ, 16, 69, 1, 1, "cpu")
    critic = SequenceDiscriminator(69, 8, T, 5, 1, "cpu")
    return gen, critic


def _reenact(gsd, dsd, real, steps, seed, lr, eta):
    """fp64 phase2/train.py:204-240 with float labels: every iteration a critic step (noise, BCE(real, 1) +
    BCE(fake, 0)), then a generator step (fresh noise, BCE(critic(fake), 1) + eta * TV)."""
    from oracle import m2d_oracle as O
    torch.manual_seed(seed)
    g_params, g_buf = O.split_state({k: v.double() if v.is_floating_point() else v for k, v in gsd.items()})
    d_params, _ = O.split_state({k: v.double() for k, v in dsd.items()})
    opt_d, opt_g = O.Adam(lr), O.Adam(lr)
    real_c = real.double().view(B, T, 69).permute(0, 2, 1).contiguous()

    def gen_forward():
        sd = dict(g_params)
        sd.update(g_buf)
        out = O.p2_generator(sd, torch.randn(B, T, NZ).double(), 1, 1, True)
        for k in g_buf:
            g_buf[k] = sd[k]
        return out.view(B, T, 69).permute(0, 2, 1)

    def bce(s, t):
        return F.binary_cross_entropy_with_logits(s, torch.full_like(s, t))

    trace = {"loss_critic": [], "err_real": [], "err_fake": [], "loss_gen": []}
    for _ in range(steps):
        critic = lambda x: O.p2_critic(d_params, x, 1, 5)  # noqa: E731
        fake = gen_forward().contiguous().detach()
        err_real, err_fake = bce(critic(real_c), 1.0), bce(critic(fake), 0.0)
        err_critic = err_real + err_fake
        grads = O.grads_of(err_critic, d_params)
        for k, v in (("loss_critic", err_critic), ("err_real", err_real), ("err_fake", err_fake)):
            trace[k].append(v.item())
        new = opt_d.step({k: v.detach() for k, v in d_params.items()}, grads)
        d_params = {k: v.detach().clone().requires_grad_(True) for k, v in new.items()}
        critic = lambda x: O.p2_critic(d_params, x, 1, 5)  # noqa: E731
        fake = gen_forward()
        err_gen = bce(critic(fake), 1.0) + eta * O.tv_loss(fake)
        grads = O.grads_of(err_gen, g_params)
        trace["loss_gen"].append(err_gen.item())
        new = opt_g.step({k: v.detach() for k, v in g_params.items()}, grads)
        g_params = {k: v.detach().clone().requires_grad_(True) for k, v in new.items()}
    return trace, {k: v.detach() for k, v in d_params.items()}, {k: v.detach() for k, v in g_params.items()}


@pytest.mark.parametrize("manual", [True, False], ids=["manual-critic", "autograd-critic"])
def test_engine_trace_matches_fp64_reenactment(fake, monkeypatch, manual):
    from music2dance_amd.critic_step import GanCriticStep
    from music2dance_amd.engine import Phase2GanEngine
    monkeypatch.setenv("M2D_MANUAL_CRITIC", "1" if manual else "0")
    gen, critic = _make_p2()
    gsd = {k: v.clone() for k, v in gen.state_dict().items()}
    dsd = {k: v.clone() for k, v in critic.state_dict().items()}
    real = torch.rand(B, T, 69, generator=torch.Generator().manual_seed(3))
    eng = Phase2GanEngine(gen, critic, CFG, data_parallel=False)
    assert isinstance(eng.manual_critic, GanCriticStep) == manual
    assert eng.n_critic_steps == 1
    steps, seed = 4, 8
    torch.manual_seed(seed)
    tr = {"loss_critic": [], "err_real": [], "err_fake": [], "loss_gen": []}
    for _ in range(steps):
        out = eng.train_step(real)
        assert set(out) == set(tr) and all(v.dim() == 0 for v in out.values())
        for k in tr:
            tr[k].append(out[k].item())
    eng.flush()
    after = torch.rand(5)
    # the host draws: the critic iteration's noise, then the generator iteration's, and nothing else
    torch.manual_seed(seed)
    for _ in range(2 * steps):
        torch.randn(B, T, NZ)
    assert torch.equal(torch.rand(5), after)
    want, d_final, g_final = _reenact(gsd, dsd, real, steps, seed, CFG["lr_critic"], CFG["eta"])
    for k in tr:
        np.testing.assert_allclose(tr[k][:1], want[k][:1], rtol=1e-5, atol=1e-6, err_msg=k)
        np.testing.assert_allclose(tr[k], want[k], rtol=2e-4, atol=1e-5, err_msg=k)
    for n, p in critic.named_parameters():
        assert torch.allclose(p.detach().double(), d_final[n], atol=2e-5), n
    for n, p in gen.named_parameters():
        if n in g_final and not n.endswith(("fc1.bias", "fc2.bias")):   # (biases in front of a BatchNorm: zero gradient)
            assert torch.allclose(p.detach().double(), g_final[n], atol=2e-5), n
    for sch in (eng.scheduler_critic, eng.scheduler_gen):
        assert sch.last_epoch == steps
    assert all(int(s["step"]) == steps for s in eng.optim_gen.state.values())
    assert all(int(s["step"]) == steps for s in eng.optim_critic.state.values())


def test_manual_and_autograd_critic_iterations_agree(fake, monkeypatch):
    from music2dance_amd.engine import Phase2GanEngine
    real = torch.rand(B, T, 69, generator=torch.Generator().manual_seed(4))
    noise = torch.randn(B, T, NZ, generator=torch.Generator().manual_seed(5))
    grads = {}
    for manual in ("1", "0"):
        monkeypatch.setenv("M2D_MANUAL_CRITIC", manual)
        gen, critic = _make_p2()
        eng = Phase2GanEngine(gen, critic, CFG, data_parallel=False)
        eng._noise = lambda b, t, d: noise
        out = eng._critic_body(real, None, None)
        grads[manual] = ({k: float(v) for k, v in out.items()}, {n: p.grad.clone() for n, p in critic.named_parameters()})
    (l1, g1), (l0, g0) = grads["1"], grads["0"]
    assert l1.keys() == l0.keys() == {"loss_critic", "err_real", "err_fake"}
    for k in l1:
        assert abs(l1[k] - l0[k]) <= 1e-6 * max(1.0, abs(l0[k])), k
    for n in g0:
        tol = 1e-5 * float(g0[n].abs().max())
        assert float((g1[n] - g0[n]).abs().max()) <= tol, n


# --------------------------------------------------------------------------------------------- data parallel
def _dp_worker(rank, world, port, q, noises, real, steps):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    kernels.set_impl(BceFakeKernels())
    from music2dance_amd.engine import Phase2GanEngine
    gen, critic = _make_p2()
    eng = Phase2GanEngine(gen, critic, CFG, data_parallel=True)
    lo, hi = rank * B // 2, (rank + 1) * B // 2
    it = {"i": 0}
    eng._noise = lambda b, t, d: noises[it["i"]][rank]
    for i in range(steps):
        it["i"] = 2 * i
        eng.train_step(real[lo:hi])   # (critic noise: index 2i; the generator iteration's: 2i + 1)
    eng.flush()
    q.put((rank, [p.detach().numpy().copy() for p in list(gen.parameters()) + list(critic.parameters())],
           eng.scheduler_gen.last_epoch))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_parameters():
    import torch.multiprocessing as mp
    steps = 3
    g = torch.Generator().manual_seed(21)
    noises = [[torch.randn(B // 2, T, NZ, generator=g) for _ in range(2)] for _ in range(2 * steps)]
    real = torch.rand(B, T, 69, generator=g)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, noises, real, steps)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    [p.join(60) for p in procs]
    init = [p.detach() for m in _make_p2() for p in m.parameters()]
    assert res[0][2] == res[1][2] == steps
    assert max(float((torch.from_numpy(a) - b).abs().max()) for a, b in zip(res[0][1], init)) > 1e-4
    for a, b in zip(res[0][1], res[1][1]):
        assert (a == b).all()


# --------------------------------------------------------------------------------------------- the script
def test_phase2_script_gan_framework(fake, tmp_path, monkeypatch):
    import yaml
    from music2dance_amd.engine import Phase2GanEngine
    from music2dance_amd.phase2 import train as TR
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    monkeypatch.chdir(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "music2dance_amd", "phase2", "configs", "default.yaml")))
    cfg.update(batch_size=2, num_train=4, num_epochs=1, n_critic_steps=8, channels=8, size=16)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    seen = []
    orig = runner.ScalarLog.scalars
    monkeypatch.setattr(runner.ScalarLog, "scalars", lambda self, d, step: (seen.append((sorted(d), step)),
                                                                           orig(self, d, step))[1])
    eng = TR.main(["-c", str(path), "-d", "0", "-n", "g", "-f", "gan", "--synthetic", "--no-run-dir"])
    assert isinstance(eng, Phase2GanEngine) and eng.total_iterations == 2
    assert seen == [(["loss_D", "loss_G"], 1), (["loss_D", "loss_G"], 2)]
    assert eng.scheduler_critic.last_epoch == eng.scheduler_gen.last_epoch == 2
    with pytest.raises(ValueError, match="Please state existing framework"):
        TR.main(["-c", str(path), "-d", "0", "-n", "g", "-f", "nope", "--synthetic"])
