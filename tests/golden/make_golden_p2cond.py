"""Fixture generator for the conditional phase-2 WGAN-LP (phase2/archis/conditional.py, train_conditional.py) — runs
ONLY where the reference exists.

train_conditional.py cannot run against archis/conditional.py (7 constructor arguments for a critic that takes 5,
`critic(x)` expected to return (score, aux), `gen(noise, lengths)` for a generator that takes labels, a one-hot written
into the noise on top of the embeddings). The archis are the runnable, checkpointable part, so they are the contract;
the loop is the script's `wgangp` branch (:109-185), changed only where the archis force it. Decisions:

  1. networks: the reference's archis as they are (imported here); nn.Embedding(4, 4) in both, the generator's GRU
     reads [noise | E[label]], the critic's conv1 [poses | E[label]] channels-first, Dropout(0.5) before lastfc and
     before lastconv.
  2. critic loss: mean(D(fake, fake_lbl)) - mean(D(real, real_lbl)) + gamma * LP, LP = mean max(0, ||g|| - 1)^2 (no
     eps), the interpolates scored with the REAL labels; the err_ac terms are dropped (no auxiliary head).
  3. generator loss: mean(D(real, real_lbl)) - mean(D(fake, fake_lbl)) + eta * tv_loss(fake), every n_critic-th body;
     plain Adam, no schedulers (:80-81).
  4. draws per body on the host generator: critic iteration - fake labels randint(0, 4, (B,)), noise randn(B, T, nz),
     the decoder's dropout mask, alpha rand(B, 1), the critic's masks for interpolated, real, fake rows; generator
     iteration - labels, noise, the decoder's mask, the critic's mask for real, then for fake.
  5. `-f gan` is out of scope.

Stores OUTPUTS only in p2_cond.npz:

  * the seeded constructor checksums (torch.manual_seed(0), generator then critic) and the state_dict key / shape list;
  * one pass (weights load_filled(gen, 3000) / load_filled(critic, 4000), poses seed 32, real labels [1, 3]): a critic
    iteration from host seed 21 (scores, gp, loss terms, critic gradient norms) and, from the same weights, a generator
    iteration from host seed 22 (err_gen, generator gradient norms); both embeddings included;
  * a K = 4 iteration trace from host seed 8 with n_critic 2, its loss terms and the final parameter checksums.

The trace runs at lr 1e-5: at 5e-5 the fp32 and fp64 runs of this script part by 4.7e-4 (relative) at step 3; at 1e-5
they agree within 4e-6. The script checks that they agree within 1e-4 and stops otherwise.

    python tests/golden/make_golden_p2cond.py
"""
import copy
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import patterns as P  # noqa: E402

B, T, NZ, GAMMA, ETA = 2, 120, 50, 10.0, 50.0
REAL_LABELS = [1, 3]
PASS_SEEDS = (21, 22)
TRACE_SEED, TRACE_STEPS, N_CRITIC, LR = 8, 4, 2, 1e-5


def networks(C):
    gen = C.SequenceGenerator(NZ, NZ, 256, 69, 2, 3)
    critic = C.SequenceDiscriminator(69, 128, T, 25, 3)
    return gen, critic


def lp_penalty(critic, real_c, fake_c, labels, dtype):
    alpha = torch.rand(B, 1).to(dtype)
    r2, f2 = real_c.reshape(B, -1), fake_c.reshape(B, -1)
    a = alpha.expand(r2.size())
    interp = (a * r2.detach() + (1 - a) * f2.detach()).view(B, 69, -1).requires_grad_(True)
    score = critic(interp, labels)
    g, = torch.autograd.grad(score, interp, torch.ones_like(score), create_graph=True, retain_graph=True)
    norms = g.reshape(B, -1).norm(2, dim=1)
    return (torch.clamp(norms - 1, min=0) ** 2).mean(), score


def critic_iteration(gen, critic, real_c, real_lbl, dtype):
    fake_lbl = torch.randint(0, 4, (B,))
    noise = torch.randn(B, T, NZ).to(dtype)
    fake = gen(noise, fake_lbl).view(B, T, 69).permute(0, 2, 1).contiguous()
    gp, s_int = lp_penalty(critic, real_c, fake, real_lbl, dtype)
    s_real = critic(real_c, real_lbl)
    s_fake = critic(fake.detach(), fake_lbl)
    err_real, err_fake = s_real.mean(), s_fake.mean()
    err_critic = err_fake - err_real + GAMMA * gp
    err_critic.backward()
    return {"err_critic": err_critic, "gp": gp, "w_dist": err_fake - err_real}, (s_int, s_real, s_fake)


def generator_iteration(gen, critic, real_c, real_lbl, dtype, tv_loss):
    lbl = torch.randint(0, 4, (B,))
    noise = torch.randn(B, T, NZ).to(dtype)
    fake = gen(noise, lbl).view(B, T, 69).permute(0, 2, 1)
    err_real = critic(real_c, real_lbl).mean()
    err_fake = critic(fake, lbl).mean()
    err_gen = err_real - err_fake + ETA * tv_loss(fake)
    err_gen.backward()
    return err_gen


def trace(R, gen, critic, real, dtype):
    gen, critic = copy.deepcopy(gen).to(dtype), copy.deepcopy(critic).to(dtype)
    real_c = real.to(dtype).view(B, T, 69).permute(0, 2, 1).contiguous()
    real_lbl = torch.tensor(REAL_LABELS)
    opt_d = torch.optim.Adam(critic.parameters(), lr=LR)
    opt_g = torch.optim.Adam(gen.parameters(), lr=LR)
    gen.train()
    critic.train()
    torch.manual_seed(TRACE_SEED)
    tr = {"err_critic": [], "gp": [], "w_dist": [], "err_gen": []}
    for it in range(1, TRACE_STEPS + 1):
        opt_d.zero_grad()
        out, _ = critic_iteration(gen, critic, real_c, real_lbl, dtype)
        opt_d.step()
        for k in ("err_critic", "gp", "w_dist"):
            tr[k].append(out[k].item())
        if it % N_CRITIC:
            continue
        opt_g.zero_grad()
        tr["err_gen"].append(generator_iteration(gen, critic, real_c, real_lbl, dtype, R["losses"].tv_loss).item())
        opt_g.step()
    return tr, gen, critic


def main():
    torch.set_num_threads(8)
    R = G.import_reference()
    C = importlib.import_module("phase2.archis.conditional")
    out = {}
    torch.manual_seed(0)
    gen0, critic0 = networks(C)
    out["init_gen_sum"] = P.sd_checksums(gen0.state_dict())
    out["init_critic_sum"] = P.sd_checksums(critic0.state_dict())
    for name, m in (("gen", gen0), ("critic", critic0)):
        sd = m.state_dict()
        out[name + "_keys"] = np.array(list(sd.keys()))
        out[name + "_shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])

    gen, critic = networks(C)
    G.load_filled(gen, 3000)
    G.load_filled(critic, 4000)
    real = P.poses(B, T, seed=32)
    real_c = real.view(B, T, 69).permute(0, 2, 1).contiguous()
    real_lbl = torch.tensor(REAL_LABELS)
    g1, c1 = copy.deepcopy(gen), copy.deepcopy(critic)
    g1.train()
    c1.train()
    torch.manual_seed(PASS_SEEDS[0])
    res, (s_int, s_real, s_fake) = critic_iteration(g1, c1, real_c, real_lbl, torch.float32)
    out.update(score_interp=G.npf(s_int), score_real=G.npf(s_real), score_fake=G.npf(s_fake),
               err_critic=res["err_critic"].item(), gp=res["gp"].item(), w_dist=res["w_dist"].item(),
               critic_grad_norms=G.grad_norms(c1))
    g2, c2 = copy.deepcopy(gen), copy.deepcopy(critic)
    g2.train()
    c2.train()
    for p in c2.parameters():
        p.requires_grad_(False)
    torch.manual_seed(PASS_SEEDS[1])
    err_gen = generator_iteration(g2, c2, real_c, real_lbl, torch.float32, R["losses"].tv_loss)
    out.update(err_gen=err_gen.item(), gen_grad_norms=G.grad_norms(g2))

    tr32, gen32, critic32 = trace(R, gen, critic, real, torch.float32)
    tr64, _, _ = trace(R, gen, critic, real, torch.float64)
    worst = max(abs(a - b) / max(1.0, abs(b)) for k in tr32 for a, b in zip(tr32[k], tr64[k]))
    print("fp32 against fp64 over the trace: %.3g (relative)" % worst)
    assert worst <= 1e-4, "the trace at lr %g is not reproducible in fp32: lower it" % LR
    out["trace_lr"] = LR
    out["trace_fp64_worst"] = worst
    for k, v in tr32.items():
        out["trace_" + k] = np.array(v)
    out["gen_final_sum"] = P.sd_checksums(gen32.state_dict())
    out["critic_final_sum"] = P.sd_checksums(critic32.state_dict())
    G.save("p2_cond", **out)


if __name__ == "__main__":
    main()
