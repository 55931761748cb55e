"""The phase-2 `gan` framework (-f gan) on the MI355X: Phase2GanEngine's K-step trace against the reference's own
(tests/golden/p2_gan.npz, made by make_golden_p2gan.py) with the hand-scheduled critic, the autograd critic and captured
graphs; single-pass values; the hand-scheduled critic iteration against the autograd one; the script."""
import os

import numpy as np
import pytest
import torch
import yaml

from music2dance_amd import kernels, losses, runner
from music2dance_amd.critic_step import GanCriticStep
from music2dance_amd.engine import Phase2GanEngine
from music2dance_amd.phase2.archis import default as p2
from tests.golden import patterns as P
from tests.test_product_parity import TRACE_RTOL, close, fill, grad_norms, load, norms_close, sums_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 2, 120
KEYS = {"loss_critic": "err_critic", "err_real": "err_real", "err_fake": "err_fake", "loss_gen": "err_gen"}


def _nets():
    fx = load("p2")
    gen = fill(p2.SequenceGenerator(50, 50, 256, 69, 2, 3, "cpu"), fx, "gen", 3000).to(DEV)
    critic = fill(p2.SequenceDiscriminator(69, 128, T, 25, 3, "cpu"), fx, "critic", 4000).to(DEV)
    return gen, critic


def _cfg(lr):
    return {"lr_gen": lr, "lr_critic": lr, "n_critic_steps": 8, "gamma": 10, "eta": 50, "input_vector_size": 50}


@pytest.mark.parametrize("mode", ["manual", "autograd", "graphs"])
def test_trace_matches_reference(mode, monkeypatch):
    fx = load("p2_gan")
    monkeypatch.setenv("M2D_MANUAL_CRITIC", "0" if mode == "autograd" else "1")
    gen, critic = _nets()
    real = P.poses(B, T, seed=32).to(DEV)
    lr = float(fx["trace_lr"])   # 5e-5: see make_golden_p2gan.py
    eng = Phase2GanEngine(gen, critic, _cfg(lr))
    assert (eng.manual_critic is None) == (mode == "autograd")
    if mode == "graphs":
        eng.enable_graphs()
    torch.manual_seed(8)
    K = len(fx["trace_err_critic"])
    tr = {k: [] for k in KEYS}
    for _ in range(K):
        out = eng.train_step(real)
        assert set(out) == set(KEYS)
        for k in KEYS:
            tr[k].append(out[k].item())
    eng.flush()
    for k, fk in KEYS.items():
        close(np.array(tr[k][:1]), fx["trace_" + fk][:1], 1e-4)
        close(np.array(tr[k]), fx["trace_" + fk], 1e-3, TRACE_RTOL)
    assert eng.scheduler_critic.last_epoch == eng.scheduler_gen.last_epoch == K
    sums_close(gen.state_dict(), fx["gen_final_sum"], adam_lr=lr, adam_steps=K, bn_biases=True)
    sums_close(critic.state_dict(), fx["critic_final_sum"], adam_lr=lr, adam_steps=K)


def test_single_pass_values():
    fx = load("p2_gan")
    gen, critic = _nets()
    noise, real = P.noise(B, T, 50, seed=31).to(DEV), P.poses(B, T, seed=32).to(DEV)
    gen.train()
    with torch.no_grad():
        rows = gen(noise, [T] * B)
    fake = rows.view(B, T, 69).permute(0, 2, 1).contiguous()
    real_c = real.permute(0, 2, 1).contiguous()
    with torch.no_grad():
        close(critic(real_c).view(-1), fx["score_real"]), close(critic(fake).view(-1), fx["score_fake"])
    out = GanCriticStep(critic).run(real, rows)
    close(out["err_real"], fx["err_real"]), close(out["err_fake"], fx["err_fake"])
    close(out["loss_critic"], fx["err_critic"])
    norms_close(grad_norms(critic), fx["critic_grad_norms"])
    critic.zero_grad(set_to_none=True)
    gen2, _ = _nets()
    gen2.train()
    fake_g = gen2(noise, [T] * B).view(B, T, 69).permute(0, 2, 1)
    for p in critic.parameters():
        p.requires_grad_(False)
    err_gen = losses.bce_with_logits(critic(fake_g), 1.0) + 50 * losses.tv_loss(fake_g)
    err_gen.backward()
    close(err_gen, fx["err_gen"])
    norms_close(grad_norms(gen2), fx["gen_grad_norms"])


def test_manual_critic_matches_autograd_critic(monkeypatch):
    real = P.poses(B, T, seed=32).to(DEV)
    noise = P.noise(B, T, 50, seed=31).to(DEV)
    res = {}
    for manual in ("1", "0"):
        monkeypatch.setenv("M2D_MANUAL_CRITIC", manual)
        gen, critic = _nets()
        eng = Phase2GanEngine(gen, critic, _cfg(5e-4))
        out = eng._critic_body(real, noise, None)
        torch.cuda.synchronize()
        res[manual] = ({k: float(v) for k, v in out.items()}, {n: p.grad.clone() for n, p in critic.named_parameters()})
    (l1, g1), (l0, g0) = res["1"], res["0"]
    for k in l0:
        assert abs(l1[k] - l0[k]) <= 1e-5 * max(1.0, abs(l0[k])), (k, l1[k], l0[k])
    for n in g0:
        tol = 1e-5 * float(g0[n].abs().max())
        assert float((g1[n] - g0[n]).abs().max()) <= tol, n


@pytest.mark.parametrize("graphs", [True, False], ids=["graphs", "no-graphs"])
def test_script_gan_framework(graphs, tmp_path, monkeypatch):
    from music2dance_amd.phase2 import train as TR
    monkeypatch.chdir(tmp_path)
    cfg = yaml.safe_load(open(os.path.join(ROOT, "music2dance_amd", "phase2", "configs", "default.yaml")))
    cfg.update(batch_size=4, num_train=40, num_epochs=1)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    outs = []
    orig = Phase2GanEngine.train_step

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        outs.append(sorted(out))
        return out

    monkeypatch.setattr(Phase2GanEngine, "train_step", spy)
    argv = ["-c", str(path), "-d", "0", "-n", "g", "-f", "gan", "--synthetic", "--no-run-dir", "--iterations", "3"]
    eng = TR.main(argv + ([] if graphs else ["--no-graphs"]))
    assert isinstance(eng, Phase2GanEngine) and eng.total_iterations == 3
    assert bool(getattr(eng, "_use_graphs", False)) == graphs
    assert outs == [sorted(KEYS)] * 3
    assert eng.scheduler_critic.last_epoch == eng.scheduler_gen.last_epoch == 3
    assert all(np.isfinite(float(v)) for v in eng.last.values())
    with pytest.raises(ValueError, match="Please state existing framework"):
        TR.main(["-c", str(path), "-d", "0", "-n", "g", "-f", "nope", "--synthetic"])
