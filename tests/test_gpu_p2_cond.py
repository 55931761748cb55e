"""The style-conditioned phase-2 WGAN-LP on the MI355X: one pass and the 4-step trace of Phase2CondEngine against the
reference's networks (tests/golden/p2_cond.npz, made by make_golden_p2cond.py), the hand-scheduled critic iteration
against the autograd one, device-drawn training, and the two scripts."""
import json
import os

import numpy as np
import pytest
import torch
import yaml

from music2dance_amd import runner
from music2dance_amd.critic_step import CondCriticStep
from music2dance_amd.engine import Phase2CondEngine
from music2dance_amd.phase2.archis import conditional as pc
from tests.golden import patterns as P
from tests.test_product_parity import TRACE_RTOL, close, grad_norms, load, norms_close

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = 2, 120
REAL_LABELS = [1, 3]


def _nets():
    gen = pc.SequenceGenerator(50, 50, 256, 69, 2, 3)
    critic = pc.SequenceDiscriminator(69, 128, T, 25, 3)
    gen.load_state_dict(P.fill_state_dict(gen.state_dict(), 3000))
    critic.load_state_dict(P.fill_state_dict(critic.state_dict(), 4000))
    return gen.to(DEV), critic.to(DEV)


def _cfg(lr, n_critic=2):
    return {"lr_gen": lr, "lr_critic": lr, "n_critic_steps": n_critic, "gamma": 10, "eta": 50, "input_vector_size": 50}


@pytest.mark.parametrize("mode", ["manual", "autograd"])
def test_one_pass_matches_reference(mode, monkeypatch):
    fx = load("p2_cond")
    monkeypatch.setenv("M2D_MANUAL_CRITIC", "0" if mode == "autograd" else "1")
    gen, critic = _nets()
    eng = Phase2CondEngine(gen, critic, _cfg(1e-5))
    assert isinstance(eng.manual_critic, CondCriticStep) == (mode == "manual")
    real = P.poses(B, T, seed=32).to(DEV)
    lbl = torch.tensor(REAL_LABELS, device=DEV)
    torch.manual_seed(21)
    out = eng._critic_body(real, lbl)
    torch.cuda.synchronize()
    close(out["loss_critic"], fx["err_critic"], 1e-4)
    close(out["gp"], fx["gp"], 1e-4)
    close(out["w_dist"], fx["w_dist"], 1e-4)
    norms_close(grad_norms(critic), fx["critic_grad_norms"])
    gen2, critic2 = _nets()
    eng2 = Phase2CondEngine(gen2, critic2, _cfg(1e-5))
    torch.manual_seed(22)
    g = eng2._generator_body(real, lbl)
    close(g["loss_gen"], fx["err_gen"], 1e-4, 1e-5)
    # (the recurrent layers and the BatchNorm-fronted biases: 2.0e-3 seen against the reference's CPU fp32)
    norms_close(grad_norms(gen2), fx["gen_grad_norms"], rtol=5e-3, what="generator gradient norms")


@pytest.mark.parametrize("mode", ["manual", "autograd"])
def test_trace_matches_reference(mode, monkeypatch):
    fx = load("p2_cond")
    monkeypatch.setenv("M2D_MANUAL_CRITIC", "0" if mode == "autograd" else "1")
    gen, critic = _nets()
    eng = Phase2CondEngine(gen, critic, _cfg(float(fx["trace_lr"])))
    real = P.poses(B, T, seed=32).to(DEV)
    lbl = torch.tensor(REAL_LABELS, device=DEV)
    torch.manual_seed(8)
    tr = {"loss_critic": [], "gp": [], "w_dist": [], "loss_gen": []}
    for _ in range(len(fx["trace_err_critic"])):
        out = eng.train_step(real, lbl)
        for k, v in out.items():
            tr[k].append(v.item())
    eng.flush()
    for k, fk in (("loss_critic", "err_critic"), ("gp", "gp"), ("w_dist", "w_dist"), ("loss_gen", "err_gen")):
        close(np.array(tr[k][:1]), fx["trace_" + fk][:1], 1e-4, 1e-5)
        close(np.array(tr[k]), fx["trace_" + fk], 1e-3, TRACE_RTOL)


def test_manual_and_autograd_gradients_agree(monkeypatch):
    real = P.poses(4, T, seed=40).to(DEV)
    lbl = torch.tensor([0, 1, 2, 3], device=DEV)
    res = {}
    for manual in ("1", "0"):
        monkeypatch.setenv("M2D_MANUAL_CRITIC", manual)
        gen, critic = _nets()
        eng = Phase2CondEngine(gen, critic, _cfg(1e-5))
        torch.manual_seed(5)
        out = eng._critic_body(real, lbl)
        res[manual] = ({k: float(v) for k, v in out.items()}, {n: p.grad.clone() for n, p in critic.named_parameters()})
    (l1, g1), (l0, g0) = res["1"], res["0"]
    for k in l1:
        assert abs(l1[k] - l0[k]) <= 1e-4 * max(1.0, abs(l0[k])), (k, l1[k], l0[k])
    assert set(g1) == set(g0)
    for n in g0:
        tol = 1e-4 * float(g0[n].abs().max()) + 1e-7
        assert float((g1[n] - g0[n]).abs().max()) <= tol, n


def test_device_draws_train_finite():
    gen, critic = _nets()
    eng = Phase2CondEngine(gen, critic, _cfg(5e-4, 8))
    eng.host_noise = False
    assert all(not m.host_rng for m in list(gen.modules()) + list(critic.modules()) if hasattr(m, "host_rng"))
    real = P.poses(32, T, seed=41).to(DEV)
    lbl = torch.randint(0, 4, (32,), device=DEV)
    for _ in range(16):
        out = eng.train_step(real, lbl)
    eng.flush()
    assert all(np.isfinite(float(v)) for v in eng.last_full.values())
    with pytest.raises(NotImplementedError):
        eng.enable_graphs()


def _small_cfg(tmp_path):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "music2dance_amd", "phase2", "configs", "default.yaml")))
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def test_scripts(tmp_path, monkeypatch):
    from music2dance_amd.dance_classification.archis.default import RecurrentDanceClassifier
    from music2dance_amd.phase2 import evaluate as EV
    from music2dance_amd.phase2 import train_conditional as TC
    monkeypatch.chdir(tmp_path)
    path = _small_cfg(tmp_path)
    eng = TC.main(["-c", str(path), "-d", "0", "-n", "c", "-f", "wgangp", "--synthetic", "--iterations", "16",
                   "--no-run-dir"])
    assert eng.total_iterations == 16
    assert all(np.isfinite(float(v)) for v in eng.last_full.values())
    fx = load("p2_cond")
    for name, m in (("gen", eng.gen), ("critic", eng.critic)):
        sd = m.state_dict()
        assert list(sd.keys()) == list(fx[name + "_keys"])
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(fx[name + "_shapes"])
    logdir = tmp_path / "run"
    os.makedirs(logdir / "models")
    runner.save_state(eng.gen, str(logdir / "models" / "gpgen_5000.pt"))
    torch.manual_seed(1)
    clf = tmp_path / "clf.pt"
    torch.save(RecurrentDanceClassifier(69, 128, 4).state_dict(), str(clf))
    EV.main(["-c", str(path), "-l", str(logdir), "--classifier", str(clf), "--synthetic", "--samples-per-style", "40",
             "--chunk", "64", "-d", "0"])
    res = json.loads((logdir / "evaluation.json").read_text())
    counts = np.array(res["counts"])
    assert counts.sum() == 160 and counts.sum(1).tolist() == [40] * 4
    np.testing.assert_allclose(np.array(res["confusion"]).sum(1), 1.0, atol=1e-12)
    assert res["jerk_fake_mean"] is not None and res["jerk_fake_std"] is not None
