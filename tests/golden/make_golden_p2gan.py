"""Fixture generator for the phase-2 `gan` framework (phase2/train.py:204-240, `-f gan`) — runs ONLY where the
reference exists.

Imports the reference's phase-2 networks (phase2/archis/default.py) with `librosa` stubbed, as make_golden.py does,
and torch.nn.BCEWithLogitsLoss; the loop is written here afresh around them, with FLOAT labels (the reference's
torch.full((B,), 1) is int64, which BCEWithLogitsLoss refuses on current torch). Stores OUTPUTS only in p2_gan.npz:

  * one pass (weights load_filled(gen, 3000) / load_filled(critic, 4000), noise seed 31, poses seed 32 - case_p2's):
    the scores, err_real / err_fake / err_critic, err_gen, the critic's and the generator's gradient norms;
  * a K = 4 iteration trace from host seed 8 (per iteration: critic noise, then generator noise): err_critic,
    err_real, err_fake, err_gen, and the final parameter / BatchNorm-buffer checksums of both networks.

The trace runs at lr 5e-5, not the config's 5e-4: at 5e-4 the critic drives the fake scores to saturation within the
four iterations (err_fake 0.01 -> 13.8 -> 0.23) and the reference's own fp32 run then sits 2.4e-3 from its fp64 run at
step 3 (3e-3 on err_gen at step 4) - fp32 rounding amplified, not a property of any implementation. At 5e-5 the two
agree within 3.1e-5; the script checks that they agree within 1e-4 and stops otherwise.

    python tests/golden/make_golden_p2gan.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402
import patterns as P  # noqa: E402

B, T, NZ, ETA = 2, 120, 50, 50.0
TRACE_SEED, TRACE_STEPS, LR = 8, 4, 5e-5


def build(R):
    gen = R["p2"].SequenceGenerator(NZ, NZ, 256, 69, 2, 3, "cpu")
    critic = R["p2"].SequenceDiscriminator(69, 128, T, 25, 3, "cpu")
    G.load_filled(gen, 3000)
    G.load_filled(critic, 4000)
    return gen, critic


def trace(R, gen, critic, real, dtype):
    gen, critic = copy.deepcopy(gen).to(dtype), copy.deepcopy(critic).to(dtype)
    crit = torch.nn.BCEWithLogitsLoss(reduction="mean")
    ones, zeros = torch.ones(B, dtype=dtype), torch.zeros(B, dtype=dtype)
    real_c = real.to(dtype).view(B, T, 69).permute(0, 2, 1).contiguous()
    opt_d = torch.optim.Adam(critic.parameters(), lr=LR)
    opt_g = torch.optim.Adam(gen.parameters(), lr=LR)
    gen.train()
    torch.manual_seed(TRACE_SEED)
    tr = {"err_critic": [], "err_real": [], "err_fake": [], "err_gen": []}
    for _ in range(TRACE_STEPS):
        opt_d.zero_grad()
        fake = gen(torch.randn(B, T, NZ).to(dtype), [T] * B).view(B, T, 69).permute(0, 2, 1).contiguous()
        err_real = crit(critic(real_c).squeeze(1), ones)
        err_fake = crit(critic(fake.detach()).squeeze(1), zeros)
        err_critic = err_real + err_fake
        err_critic.backward()
        opt_d.step()
        opt_g.zero_grad()
        fake = gen(torch.randn(B, T, NZ).to(dtype), [T] * B).view(B, T, 69).permute(0, 2, 1)
        err_gen = crit(critic(fake).squeeze(1), ones) + ETA * R["losses"].tv_loss(fake)
        err_gen.backward()
        opt_g.step()
        for k, v in (("err_critic", err_critic), ("err_real", err_real), ("err_fake", err_fake), ("err_gen", err_gen)):
            tr[k].append(v.item())
    return tr, gen, critic


def main():
    torch.set_num_threads(8)
    R = G.import_reference()
    gen, critic = build(R)
    out = {}
    noise, real = P.noise(B, T, NZ, seed=31), P.poses(B, T, seed=32)
    real_c = real.view(B, T, 69).permute(0, 2, 1).contiguous()
    crit = torch.nn.BCEWithLogitsLoss(reduction="mean")
    g1, c1 = copy.deepcopy(gen), copy.deepcopy(critic)
    g1.train()
    fake = g1(noise, [T] * B).view(B, T, 69).permute(0, 2, 1).contiguous()
    s_real, s_fake = c1(real_c).squeeze(1), c1(fake.detach()).squeeze(1)
    err_real, err_fake = crit(s_real, torch.ones(B)), crit(s_fake, torch.zeros(B))
    (err_real + err_fake).backward()
    out.update(score_real=G.npf(s_real), score_fake=G.npf(s_fake), err_real=err_real.item(),
               err_fake=err_fake.item(), err_critic=(err_real + err_fake).item(), critic_grad_norms=G.grad_norms(c1))
    c1.zero_grad()
    g2 = copy.deepcopy(gen)
    g2.train()
    fake_g = g2(noise, [T] * B).view(B, T, 69).permute(0, 2, 1)
    err_gen = crit(c1(fake_g).squeeze(1), torch.ones(B)) + ETA * R["losses"].tv_loss(fake_g)
    err_gen.backward()
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
    G.save("p2_gan", **out)


if __name__ == "__main__":
    main()
