"""Dev tool: the dance classifier's recurrence on the small-state kernels (M2D_GRU_SMALL=1) against the gru_stack
fallback (=0), alternated in one process. Times, with HIP events,
  * the recurrence alone: forward + backward through time of nn.GRU(128, 4) at B = 49, T = 120 (gi given);
  * the same through ops.gru_final_state (input projection, recurrence, weight / input gradients);
  * the whole classifier train step (forward, cross-entropy, backward, Adam).

    python tools/classifier_time.py [--rounds 5] [--iters 50] [--json PATH]

Under `rocprofv3 --kernel-trace --stats -- python tools/classifier_time.py --rounds 1` the per-kernel table follows."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from music2dance_amd import kernels, ops  # noqa: E402

B, T, I, H = 49, 120, 128, 4
DEV = torch.device("cuda:0")


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / iters  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", type=str, default=None)
    opts = ap.parse_args()
    k = kernels.impl()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, I, generator=g).to(DEV)
    w_ih = (0.1 * torch.randn(3 * H, I, generator=g)).to(DEV).requires_grad_(True)
    w_hh = (0.5 * torch.randn(3 * H, H, generator=g)).to(DEV).requires_grad_(True)
    b_ih = (0.1 * torch.randn(3 * H, generator=g)).to(DEV).requires_grad_(True)
    b_hh = (0.1 * torch.randn(3 * H, generator=g)).to(DEV).requires_grad_(True)
    xg = x.clone().requires_grad_(True)
    gi = k.gemm(0, x.view(B * T, I), w_ih.detach(), b_ih.detach()).view(B, T, 3 * H)
    dh_n = torch.randn(B, H, generator=g).to(DEV)
    dout_full = torch.zeros(B, T, H, device=DEV)
    dout_full[:, -1] = dh_n
    w_hh_d, b_hh_d = w_hh.detach(), b_hh.detach()
    w_hh_t = k.transposed(w_hh_d)

    def rec_small():
        out, _, saved = k.gru_small_fwd(gi, w_hh_d, b_hh_d, None, save=True)
        k.gru_small_bwd(None, dh_n, out, saved, w_hh_d)

    def rec_stack():
        outs, saved = k.gru_stack_fwd(gi, [None], [None], [w_hh_t], [b_hh_d], None, True)
        k.gru_stack_bwd(dout_full, outs, saved, [w_hh_d], [None], None)

    def op_fb():
        h = ops.gru_final_state(xg, w_ih, w_hh, b_ih, b_hh)
        h.backward(dh_n)

    from music2dance_amd.dance_classification.archis.default import RecurrentDanceClassifier
    from music2dance_amd.dance_classification.engine import ClassifierEngine
    torch.manual_seed(0)
    eng = ClassifierEngine(RecurrentDanceClassifier(69, 128, 4).to(DEV), 2e-4)
    sticks = torch.rand(B, 69, T, generator=g).to(DEV)
    labels = torch.randint(0, 4, (B,), generator=g).to(DEV)

    def step():
        eng.train_step(sticks, labels)

    res = {"small": {}, "fallback": {}}
    for r in range(opts.rounds):
        for mode in ("small", "fallback"):
            os.environ["M2D_GRU_SMALL"] = "1" if mode == "small" else "0"
            rec = timed(rec_small if mode == "small" else rec_stack, opts.iters)
            op = timed(op_fb, opts.iters)
            st = timed(step, opts.iters)
            for key, v in (("recurrence_fwd_bwd_us", rec), ("gru_final_state_fwd_bwd_us", op), ("train_step_us", st)):
                res[mode].setdefault(key, []).append(round(v, 2))
            print("round %d %-8s recurrence fwd+bwd %8.1f us   gru_final_state fwd+bwd %8.1f us   train step %8.1f us"
                  % (r, mode, rec, op, st), flush=True)
    k.check_async_errors()
    summ = {m: {key: min(v) for key, v in d.items()} for m, d in res.items()}
    s, f = summ["small"], summ["fallback"]
    summ["small_us_per_step"] = round(s["recurrence_fwd_bwd_us"] / (2 * T), 3)
    summ["train_step_share_removed"] = round((f["train_step_us"] - s["train_step_us"]) / f["train_step_us"], 4)
    summ["rounds"] = res
    print(json.dumps(summ))
    if opts.json:
        os.makedirs(os.path.dirname(os.path.abspath(opts.json)), exist_ok=True)
        with open(opts.json, "w") as fh:
            json.dump(summ, fh, indent=1)


if __name__ == "__main__":
    main()
