"""The style-conditioned phase-2 WGAN-LP without a GPU: the C-ABI surface of the label / dropout entries, the seeded
constructors and state_dict layout against the reference's (p2_cond.npz), the engine's loop against the reference's
loop (the fixture's trace and an fp64 re-enactment), the hand-scheduled critic iteration against the autograd one, a
world-size-2 gloo run and the script surface. Kernels are the CPU stand-in of tests/fake_backend.py, extended here by
the four new entries."""
import copy
import os
import re

import numpy as np
import pytest
import torch

from music2dance_amd import kernels, runner
from tests.fake_backend import FakeKernels
from tests.golden import patterns as P
from tests.test_dp_gloo import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("m2d_label_concat", "m2d_pose_pack3_label", "m2d_label_embed_bwd", "m2d_dropout")
FIX = os.path.join(ROOT, "tests", "golden", "p2_cond.npz")


def _emb(E, labels):
    ok = (labels >= 0) & (labels < E.shape[0])
    rows = E[labels.clamp(0, E.shape[0] - 1)]
    return torch.where(ok[:, None], rows, torch.full_like(rows, float("nan")))


class CondFakeKernels(FakeKernels):
    """FakeKernels + label concatenation, labelled pose packing, the embedding gradient and dropout, in torch (same
    contract as kernels.HipKernels; the device-made dropout bits are a CPU generator's, seeded by (seed, offset))."""

    def label_concat(self, x, E, labels, layout, out=None):
        e = _emb(E, labels)
        if layout == 0:
            y = torch.cat((x, e[:, None, :].expand(-1, x.shape[1], -1)), 2)
        else:
            y = torch.cat((x, e[:, :, None].expand(-1, -1, x.shape[2])), 1)
        return self._into(out, y)

    def pose_pack3_label(self, real, fake_rows, alpha, E, real_lbl, fake_lbl, out=None):
        B, T, C = real.shape
        a = alpha.reshape(B, 1, 1)
        f = fake_rows.reshape(B, T, C)
        rows = torch.cat((a * real + (1 - a) * f, real, f)).transpose(1, 2)
        lbl = torch.cat((real_lbl, real_lbl, fake_lbl))
        return self._into(out, self.label_concat(rows.contiguous(), E, lbl, 1))

    def label_embed_bwd(self, dx, labels, r0, r1, c0, L, D, layout, out=None):
        g = dx[r0:r1, :, c0:c0 + D].sum(1) if layout == 0 else dx[r0:r1, c0:c0 + D].sum(2)
        dE = torch.zeros(L, D, dtype=torch.float64)
        if ((labels < 0) | (labels >= L)).any():
            dE.fill_(float("nan"))
        else:
            dE.index_add_(0, labels, g.double())
        return self._into(out, dE.float())

    def dropout(self, x, mask, p_keep=0.5, scale=2.0, seed=None, offset=0, out=None):
        if seed is not None:
            g = torch.Generator().manual_seed((int(seed) * 1000003 + int(offset)) & 0x7FFFFFFFFFFFFFFF)
            shape = x.shape if x is not None else mask.shape
            bits = (torch.rand(tuple(shape), generator=g) < p_keep).to(torch.uint8)
            if mask is not None:
                mask.copy_(bits)
            else:
                mask = bits
        if x is None:
            return mask
        return self._into(out, x * mask.to(x.dtype) * scale)


@pytest.fixture
def fake():
    prev = kernels.set_impl(CondFakeKernels())
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
    assert re.search(r"m2d_dropout\(const float\* x, float\* y, unsigned char\* mask, long long n, float p_keep", text)
    assert _lib.SIGNATURES["m2d_dropout"][1][3] is _lib._c.c_longlong
    assert _lib.SIGNATURES["m2d_dropout"][1][6] is _lib._c.c_ulonglong


def test_seeded_constructors_match_the_reference():
    from music2dance_amd.phase2.archis.conditional import SequenceDiscriminator, SequenceGenerator
    fx = np.load(FIX)
    torch.manual_seed(0)
    gen = SequenceGenerator(50, 50, 256, 69, 2, 3)
    critic = SequenceDiscriminator(69, 128, 120, 25, 3)
    for name, m in (("gen", gen), ("critic", critic)):
        sd = m.state_dict()
        assert list(sd.keys()) == list(fx[name + "_keys"]), name
        assert [",".join(str(d) for d in v.shape) for v in sd.values()] == list(fx[name + "_shapes"]), name
        np.testing.assert_allclose(P.sd_checksums(sd), fx["init_%s_sum" % name], rtol=1e-6, atol=1e-6, err_msg=name)


# --------------------------------------------------------------------------------------------- the fixture's networks
CFG = {"lr_gen": 1e-5, "lr_critic": 1e-5, "n_critic_steps": 2, "gamma": 10, "eta": 50, "input_vector_size": 50}
B, T = 2, 120


def _fixture_nets():
    from music2dance_amd.phase2.archis.conditional import SequenceDiscriminator, SequenceGenerator
    gen = SequenceGenerator(50, 50, 256, 69, 2, 3)
    critic = SequenceDiscriminator(69, 128, T, 25, 3)
    gen.load_state_dict(P.fill_state_dict(gen.state_dict(), 3000))
    critic.load_state_dict(P.fill_state_dict(critic.state_dict(), 4000))
    return gen, critic


@pytest.mark.parametrize("manual", [True, False], ids=["manual-critic", "autograd-critic"])
def test_engine_trace_matches_the_reference_loop(fake, monkeypatch, manual):
    from music2dance_amd.critic_step import CondCriticStep
    from music2dance_amd.engine import Phase2CondEngine
    torch.set_num_threads(8)
    monkeypatch.setenv("M2D_MANUAL_CRITIC", "1" if manual else "0")
    fx = np.load(FIX)
    gen, critic = _fixture_nets()
    eng = Phase2CondEngine(gen, critic, CFG, data_parallel=False)
    assert isinstance(eng.manual_critic, CondCriticStep) == manual
    assert eng.host_noise and eng.host_rng
    real = P.poses(B, T, seed=32)
    labels = torch.tensor([1, 3])
    torch.manual_seed(8)
    tr = {"loss_critic": [], "gp": [], "w_dist": [], "loss_gen": []}
    for _ in range(4):
        out = eng.train_step(real, labels)
        for k in out:
            tr[k].append(out[k].item())
    eng.flush()
    for k, fk in (("loss_critic", "err_critic"), ("gp", "gp"), ("w_dist", "w_dist"), ("loss_gen", "err_gen")):
        np.testing.assert_allclose(tr[k], fx["trace_" + fk], rtol=2e-4, atol=2e-4, err_msg=k)
    # (biases in front of a BatchNorm get zero-sum gradients: Adam turns their rounding into steps of lr; rtol 2e-3)
    np.testing.assert_allclose(P.sd_checksums(gen.state_dict()), fx["gen_final_sum"], rtol=2e-3, atol=1e-3)
    np.testing.assert_allclose(P.sd_checksums(critic.state_dict()), fx["critic_final_sum"], rtol=1e-4, atol=1e-4)
    # no schedulers: the learning rate never moves
    assert eng.scheduler_gen.last_epoch == 0 and eng.optim_gen.param_groups[0]["lr"] == CFG["lr_gen"]


def test_engine_matches_fp64_reenactment_of_one_body(fake):
    """the reference's loop body in fp64 torch (nn.Embedding, F.conv1d, nn.GRU ...: the reference's networks rebuilt
    from the same state_dicts) against one engine body, draw for draw"""
    from music2dance_amd.engine import Phase2CondEngine
    gen, critic = _fixture_nets()
    gsd = copy.deepcopy(gen.state_dict())
    dsd = copy.deepcopy(critic.state_dict())
    eng = Phase2CondEngine(gen, critic, dict(CFG, n_critic_steps=1), data_parallel=False)
    real = P.poses(B, T, seed=32)
    labels = torch.tensor([2, 0])
    torch.manual_seed(5)
    out = {k: v.item() for k, v in eng.train_step(real, labels).items()}
    want = _reenact_body(gsd, dsd, real, labels, 5)
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, out[k], v)


def _reenact_body(gsd, dsd, real, labels, seed):
    import torch.nn as nn
    import torch.nn.functional as F
    g = {k: v.double() if v.is_floating_point() else v for k, v in gsd.items()}
    d = {k: v.double().requires_grad_(True) for k, v in dsd.items()}

    rnn = nn.GRU(54, 50, 3, batch_first=True).double()   # (built before the seed: its constructor draws)
    rnn.load_state_dict({k[len("noise_gen.rnn."):]: v for k, v in g.items() if k.startswith("noise_gen.rnn.")})

    def gen(noise, lbl):
        x = torch.cat((noise, g["embed_label.weight"][lbl][:, None].expand(-1, T, -1)), 2)
        h = rnn(x)[0].reshape(-1, 50)

        def bn(x, p):
            return F.batch_norm(x, None, None, g[p + ".weight"], g[p + ".bias"], True, 0.1, 1e-5)

        def lin(x, p):
            return F.linear(x, g[p + ".weight"], g[p + ".bias"])

        h = F.relu(bn(lin(h, "decoder.fc1"), "decoder.bn1"))
        for i in range(2):
            h = h + F.relu(bn(lin(h, "decoder.blocks.%d.fc2" % i), "decoder.blocks.%d.bn2" % i))
        keep = torch.empty(h.shape[0], 256).bernoulli_(0.5).double()
        return lin(h * keep * 2, "decoder.lastfc")

    def critic(x, lbl):
        x = torch.cat((x, d["embed_label.weight"][lbl][:, :, None].expand(-1, -1, T)), 1)
        h = F.relu(F.conv1d(x, d["conv1.weight"], d["conv1.bias"], padding=12))
        for i in range(3):
            p = "blocks.%d." % i
            u = F.relu(F.conv1d(h, d[p + "conv1.weight"], d[p + "conv1.bias"], padding=3))
            h = h + F.relu(F.conv1d(u, d[p + "conv2.weight"], d[p + "conv2.bias"], padding=3))
        keep = torch.empty(h.shape).bernoulli_(0.5).double()
        return F.conv1d(h * keep * 2, d["lastconv.weight"], d["lastconv.bias"]).squeeze(1)

    torch.manual_seed(seed)
    real_c = real.double().view(B, T, 69).permute(0, 2, 1)
    fl = torch.randint(0, 4, (B,))
    fake = gen(torch.randn(B, T, 50).double(), fl).view(B, T, 69).permute(0, 2, 1).detach()
    a = torch.rand(B, 1).double().view(B, 1, 1)
    interp = (a * real_c + (1 - a) * fake).requires_grad_(True)
    s = critic(interp, labels)
    gr, = torch.autograd.grad(s.sum(), interp, create_graph=True)
    gp = (torch.clamp(gr.reshape(B, -1).norm(dim=1) - 1, min=0) ** 2).mean()
    s_real = critic(real_c, labels)   # (the critic masks: interpolated, real, fake)
    w = critic(fake, fl).mean() - s_real.mean()
    out = {"loss_critic": (w + 10 * gp).item(), "gp": gp.item(), "w_dist": w.item()}
    # (the generator iteration runs on the critic after its Adam step: only the critic iteration's terms are compared)
    return out


def test_manual_and_autograd_critic_iterations_agree(fake, monkeypatch):
    from music2dance_amd.engine import Phase2CondEngine
    from music2dance_amd.phase2.archis.conditional import SequenceDiscriminator, SequenceGenerator
    real = torch.rand(3, 24, 69, generator=torch.Generator().manual_seed(4))
    labels = torch.tensor([0, 3, 3])
    grads = {}
    for manual in ("1", "0"):
        monkeypatch.setenv("M2D_MANUAL_CRITIC", manual)
        torch.manual_seed(0)
        gen = SequenceGenerator(8, 8, 16, 69, 1, 1)
        critic = SequenceDiscriminator(69, 8, 24, 5, 1)
        eng = Phase2CondEngine(gen, critic, dict(CFG, input_vector_size=8), data_parallel=False)
        torch.manual_seed(11)
        out = eng._critic_body(real, labels)
        grads[manual] = ({k: float(v) for k, v in out.items()}, {n: p.grad.clone() for n, p in critic.named_parameters()})
    (l1, g1), (l0, g0) = grads["1"], grads["0"]
    for k in l1:
        assert abs(l1[k] - l0[k]) <= 1e-5 * max(1.0, abs(l0[k])), k
    assert set(g1) == set(g0) and "embed_label.weight" in g1
    for n in g0:
        tol = 1e-5 * float(g0[n].abs().max()) + 1e-9
        assert float((g1[n] - g0[n]).abs().max()) <= tol, n


def test_penalty_has_no_embedding_term(fake, monkeypatch):
    """E reaches the penalty through ReLU masks only: d gp / d E is exactly zero (autograd path, double backward)"""
    from music2dance_amd import losses
    from music2dance_amd.phase2.archis.conditional import SequenceDiscriminator
    torch.manual_seed(0)
    critic = SequenceDiscriminator(69, 8, 24, 5, 1)
    real, fake_ = torch.rand(2, 69, 24), torch.rand(2, 69, 24)
    gp = losses.gradient_penalty(critic, 2, real, fake_, is_seq=True, lp=True, alpha=torch.full((2, 1), 0.3),
                                 labels=torch.tensor([1, 2]))
    gp = gp + 0 * critic.embed_label.weight.sum()
    gE, = torch.autograd.grad(gp, critic.embed_label.weight)
    assert float(gp.detach()) > 0 and torch.equal(gE, torch.zeros_like(gE))


def test_enable_graphs_raises(fake):
    from music2dance_amd.engine import Phase2CondEngine
    gen, critic = _fixture_nets()
    eng = Phase2CondEngine(gen, critic, CFG, data_parallel=False)
    with pytest.raises(NotImplementedError):
        eng.enable_graphs()
    eng.enable_graphs(False)


# --------------------------------------------------------------------------------------------- data parallel
def _dp_worker(rank, world, port, q, real, labels, steps):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    kernels.set_impl(CondFakeKernels())
    from music2dance_amd.engine import Phase2CondEngine
    from music2dance_amd.phase2.archis.conditional import SequenceDiscriminator, SequenceGenerator
    torch.manual_seed(0)
    gen = SequenceGenerator(8, 8, 16, 69, 1, 1)
    critic = SequenceDiscriminator(69, 8, 24, 5, 1)
    eng = Phase2CondEngine(gen, critic, dict(CFG, input_vector_size=8, lr_gen=1e-3, lr_critic=1e-3, n_critic_steps=2),
                           data_parallel=True)
    torch.manual_seed(100 + rank)   # rank-distinct draws
    lo, hi = rank * 2, (rank + 1) * 2
    for _ in range(steps):
        eng.train_step(real[lo:hi], labels[lo:hi])
    eng.flush()
    q.put((rank, [p.detach().numpy().copy() for p in list(gen.parameters()) + list(critic.parameters())]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_hold_identical_parameters():
    import torch.multiprocessing as mp
    g = torch.Generator().manual_seed(21)
    real = torch.rand(4, 24, 69, generator=g)
    labels = torch.tensor([0, 1, 2, 3])
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, real, labels, 4)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=300) for _ in range(2)], key=lambda r: r[0])
    [p.join(60) for p in procs]
    for a, b in zip(res[0][1], res[1][1]):
        assert (a == b).all()


# --------------------------------------------------------------------------------------------- the scripts
def _small_cfg(tmp_path):
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "music2dance_amd", "phase2", "configs", "default.yaml")))
    cfg.update(batch_size=2, num_train=4, num_epochs=2, n_critic_steps=2, channels=8, size=16)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def test_conditional_script_frameworks(fake, tmp_path, monkeypatch):
    from music2dance_amd.engine import Phase2CondEngine
    from music2dance_amd.phase2 import train_conditional as TC
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    monkeypatch.chdir(tmp_path)
    path = _small_cfg(tmp_path)
    seen = []
    orig = runner.ScalarLog.scalars
    monkeypatch.setattr(runner.ScalarLog, "scalars", lambda self, d, step: (seen.append((sorted(d), step)),
                                                                           orig(self, d, step))[1])
    eng = TC.main(["-c", str(path), "-d", "0", "-n", "c", "-f", "wgangp", "--synthetic", "--no-run-dir",
                   "--iterations", "4"])
    assert isinstance(eng, Phase2CondEngine) and eng.total_iterations == 4 and not eng.host_noise
    assert seen == [(["gp", "loss_critic", "loss_gen", "w_dist"], 2), (["gp", "loss_critic", "loss_gen", "w_dist"], 4)]
    assert all(np.isfinite(float(v)) for v in eng.last_full.values())
    for fw in ("gan", "nope"):
        with pytest.raises(ValueError, match="Please state existing framework"):
            TC.main(["-c", str(path), "-d", "0", "-n", "c", "-f", fw, "--synthetic", "--no-run-dir"])


def test_evaluate_script_synthetic(fake, tmp_path, monkeypatch):
    import json
    from music2dance_amd.dance_classification.archis.default import RecurrentDanceClassifier
    from music2dance_amd.phase2 import evaluate as EV
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    monkeypatch.setattr(EV.ops, "cross_entropy_pred", lambda logits, t: (None, logits.argmax(1)))
    path = _small_cfg(tmp_path)
    torch.manual_seed(1)
    clf = tmp_path / "clf.pt"
    torch.save(RecurrentDanceClassifier(69, 128, 4).state_dict(), str(clf))
    monkeypatch.setattr(RecurrentDanceClassifier, "forward", lambda self, x: x.mean(2)[:, :4])
    logdir = tmp_path / "run"
    EV.main(["-c", str(path), "-l", str(logdir), "--classifier", str(clf), "--synthetic", "--samples-per-style", "3",
             "--chunk", "5"])
    res = json.loads((logdir / "evaluation.json").read_text())
    assert np.array(res["counts"]).sum() == 12 and np.array(res["counts"]).sum(1).tolist() == [3, 3, 3, 3]
    np.testing.assert_allclose(np.array(res["confusion"]).sum(1), 1.0)
    assert 0.0 <= res["style_agreement"] <= 1.0 and res["jerk_fake_mean"] >= 0.0
