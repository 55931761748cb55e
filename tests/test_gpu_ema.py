"""The generator EMA on the GPU (include/m2d.h: m2d_adam_multi_ema; music2dance_amd/ema.py): every arm of the kernel with
parameters, moments and packed images bit-equal to the untracked step and shadows within tests/ema_cases.py's bound of
the fp64 average; shadows / all operands off 16-byte alignment; more tensors than a launch carries; the skip word; the
phase-2 engine eager and from captured graphs; the phase-3 engine's twin after consecutive steps (the stale-image case);
the phase-2 train script with `ema_decay` set."""
import pytest
import torch
import yaml

from music2dance_amd import kernels
from music2dance_amd.optim import Adam
from tests import ema_cases as C
from tests.placement_cases import guards_intact, place

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def K():
    k = kernels.impl()
    assert k.name == "hip"
    return k


def _put(t, off):
    """-> (tensor on the device holding t, its guard buffer or None): off floats past 16-byte alignment"""
    if off == 0:
        return t.to(DEV), None
    return place(t, off, DEV)


def _adam_with_state(ps, off, lr):
    """optim.Adam whose moments lie `off` floats past 16-byte alignment too (off 0: the optimizer makes them itself)"""
    opt = Adam(ps, lr=lr)
    if off:
        for p in ps:
            opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": place(torch.zeros(p.shape), off, DEV)[0],
                            "exp_avg_sq": place(torch.zeros(p.shape), off, DEV)[0]}
    return opt


# ------------------------------------------------------------------------------------------------ 1, 2: the arms
@pytest.mark.parametrize("shadow_off,operand_off", [(0, 0), (1, 0), (1, 1)],
                         ids=["aligned", "shadows-off-16", "every-operand-off-16"])
def test_every_arm_steps_like_the_untracked_kernel_and_averages(shadow_off, operand_off):
    k = K()
    init = C.tensors(C.SHAPES, seed=0)
    tracked = [_put(t, operand_off)[0].requires_grad_(True) for t in init]
    plain = [t.to(DEV).requires_grad_(True) for t in init]
    placed = [_put(t, shadow_off) for t in init]
    shadows = [s for s, _ in placed]
    opt, opt0 = _adam_with_state(tracked, operand_off, 1e-3), Adam(plain, lr=1e-3)
    opt.track_ema(zip(tracked, shadows))
    ref = C.Ema64(shadows)
    convs = [i for i, s in enumerate(C.SHAPES) if len(s) == 3]
    with k.weight_cache():
        for i in convs:                                   # live packed images: the step rewrites them
            k.packed_weights(tracked[i]), k.packed_weights(plain[i])
        for step, decay in enumerate(C.DECAYS):
            for a, b, g in zip(tracked, plain, C.grads(C.SHAPES, seed=20 + step)):
                a.grad, b.grad = _put(g, operand_off)[0], g.to(DEV)
            opt.ema_decay = decay
            opt.step()
            opt0.step()
            k.invalidate_packed(tracked + plain)             # what the engines call: the step's images stay
            ref.update(tracked, decay)
            launches = k.pack_launches
            for i, (a, b) in enumerate(zip(tracked, plain)):
                assert torch.equal(a.detach(), b.detach()), (step, i)
                for key in ("exp_avg", "exp_avg_sq"):
                    assert torch.equal(opt.state[a][key], opt0.state[b][key]), (step, i, key)
            for i in convs:
                (wf, wb), (wf0, wb0) = k.packed_weights(tracked[i]), k.packed_weights(plain[i])
                assert torch.equal(wf, wf0) and torch.equal(wb, wb0), (step, i)
                assert torch.equal(wf, tracked[i].detach().permute(1, 2, 0).contiguous()), (step, i)
                assert torch.equal(wb, tracked[i].detach().permute(0, 2, 1).contiguous()), (step, i)
            assert k.pack_launches == launches                   # the images were the step's, not fresh packs
    ref.check(shadows, "arms %d/%d" % (shadow_off, operand_off))
    assert all(not torch.equal(s, p.detach()) for s, p in zip(shadows, tracked))
    for s, buf in placed:
        assert buf is None or guards_intact(buf, s)


# ------------------------------------------------------------------------------------------------ 3: batches
def test_more_tensors_than_one_launch_carries():
    k = K()
    n = 2 * C.EMA_BATCH + 3
    sizes = [1 + (i * 7) % 50 for i in range(n)]
    assert min(sizes) == 1 and max(sizes) == 50
    g = torch.Generator().manual_seed(5)
    total = sum(sizes)

    def laid_out(flat):
        """the tensors end to end in one buffer: every residue of 16 bytes occurs"""
        flat, out, at = flat.to(DEV), [], 0
        for s in sizes:
            out.append(flat[at:at + s])
            at += s
        return out

    p_h, g_h = torch.randn(total, generator=g), torch.randn(total, generator=g)
    m_h, v_h = torch.randn(total, generator=g) * 0.1, torch.rand(total, generator=g) * 0.01
    e_h = p_h.clone()                                           # shadows start as copies, as the twin's do
    sets = [[laid_out(t.clone()) for t in (p_h, g_h, m_h, v_h)] for _ in range(2)]
    shadows = laid_out(e_h.clone())
    ema = [None if i % 3 == 2 else s for i, s in enumerate(shadows)]
    ref = C.Ema64(shadows)
    k.adam_multi(*sets[0], 2e-4, 0.9, 0.999, 1e-8, 3, ema=ema, ema_decay=0.9)
    k.adam_multi(*sets[1], 2e-4, 0.9, 0.999, 1e-8, 3)
    for a, b in zip(sets[0], sets[1]):
        for i, (x, y) in enumerate(zip(a, b)):
            assert torch.equal(x, y), i
    assert not torch.equal(sets[0][0][0], p_h[:1].to(DEV))
    tracked = {i for i in range(n) if i % 3 != 2}
    ref.update(sets[0][0], 0.9, which=tracked)
    ref.check(shadows, "batches")
    at = 0
    for i, s in enumerate(sizes):                               # a tensor without a shadow: nothing near it is written
        if i not in tracked:
            assert torch.equal(shadows[i].cpu(), e_h[at:at + s]), i
        elif s >= 8:
            assert not torch.equal(shadows[i].cpu(), e_h[at:at + s]), i
        at += s
    with pytest.raises(Exception, match="ema"):
        k.adam_multi(*sets[0], 2e-4, 0.9, 0.999, 1e-8, 4, ema=ema[:-1], ema_decay=0.9)
    with pytest.raises(Exception, match="ema"):
        k.adam_multi(*sets[0], 2e-4, 0.9, 0.999, 1e-8, 4, ema=ema)


def test_c_abi_refuses_a_missing_shadow_table():
    import ctypes
    from music2dance_amd import _lib
    h = _lib.lib()
    t = [torch.zeros(8, device=DEV) for _ in range(4)]
    items = (_lib.AdamItem * 1)()
    items[0].param, items[0].grad, items[0].exp_avg, items[0].exp_avg_sq, items[0].numel = (*[x.data_ptr() for x in t], 8)
    rc = h.m2d_adam_multi_ema(ctypes.addressof(items), None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.5, None, None)
    assert rc == h.m2d_adam_multi_ema(None, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.5, None, None) != 0
    assert h.m2d_adam_multi_ema(None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.03, 0.5, None, None) == 0
    torch.cuda.synchronize()
    assert all(float(x.abs().sum()) == 0.0 for x in t)


# ------------------------------------------------------------------------------------------------ 4: skip
def test_a_raised_skip_word_voids_parameters_and_shadows():
    k = K()
    shapes = [(20, 16, 3), (4099,), (7,), (33, 5)]
    ps = [t.to(DEV) for t in C.tensors(shapes, seed=2)]
    gs = [t.to(DEV) for t in C.grads(shapes, seed=3)]
    ms, vs = [torch.zeros_like(p) for p in ps], [torch.zeros_like(p) for p in ps]
    shadows = [p.clone() for p in ps]
    held = [[t.clone() for t in ts] for ts in (ps, ms, vs, shadows)]
    skip = torch.ones((), device=DEV)
    k.adam_multi(ps, gs, ms, vs, 1e-3, 0.9, 0.999, 1e-8, 1, skip=skip, ema=shadows, ema_decay=0.5)
    torch.cuda.synchronize()
    for before, now in zip(held, (ps, ms, vs, shadows)):
        assert all(torch.equal(a, b) for a, b in zip(before, now))
    ref = C.Ema64(shadows)
    skip.zero_()
    k.adam_multi(ps, gs, ms, vs, 1e-3, 0.9, 0.999, 1e-8, 1, skip=skip, ema=shadows, ema_decay=0.5)
    assert all(not torch.equal(a, b) for a, b in zip(held[0], ps))
    assert all(not torch.equal(a, b) for a, b in zip(held[3], shadows))
    ref.update(ps, 0.5)
    ref.check(shadows, "skip cleared")


# ------------------------------------------------------------------------------------------------ 5: phase 2
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_phase2_engine_shadows_follow_the_fp64_average(graphs):
    from music2dance_amd.engine import Phase2Engine
    from music2dance_amd.phase2.archis import default as p2
    K()
    cfg = {"lr_gen": 5e-4, "lr_critic": 5e-4, "n_critic_steps": 2, "gamma": 10, "eta": 50, "input_vector_size": 50}
    real = torch.rand(8, 120, 69, generator=torch.Generator().manual_seed(4)).to(DEV)
    torch.manual_seed(0)
    gen = p2.SequenceGenerator(50, 50, 256, 69, 2, 3, DEV)
    critic = p2.SequenceDiscriminator(69, 128, 120, 25, 3, DEV)
    eng = Phase2Engine(gen, critic, cfg, data_parallel=False)
    if graphs:
        eng.enable_graphs()
    eng.enable_ema(0.999)
    twin = eng.gen_ema
    assert list(twin.state_dict()) == list(gen.state_dict()) and not twin.training
    ref = C.Ema64(list(twin.parameters()))
    torch.manual_seed(21)
    gen_steps = 0
    for body in range(8):
        before = [p.clone() for p in twin.parameters()] if body % 2 == 0 else None
        out = eng.train_step(real)
        if "loss_gen" in out:
            stepped = {i for i, p in enumerate(gen.parameters()) if p in eng.optim_gen.state}
            ref.update(list(gen.parameters()), min(0.999, (1 + gen_steps) / (10 + gen_steps)), which=stepped)
            gen_steps += 1
        else:
            assert all(torch.equal(a, b) for a, b in zip(before, twin.parameters()))    # a critic-only body
    eng.flush()
    assert gen_steps == 4 and eng._ema.updates == 4
    ref.check(list(twin.parameters()), "phase 2 graphs=%s" % graphs)
    live = dict(gen.named_parameters())
    dead = {k for k, p in live.items() if p not in eng.optim_gen.state}
    for name, p in twin.named_parameters():
        assert torch.equal(p, live[name].detach()) == (name in dead), name
    handed = eng.gen_ema
    for (name, b), (_, b0) in zip(handed.named_buffers(), gen.named_buffers()):
        assert torch.equal(b, b0), name


# ------------------------------------------------------------------------------------------------ 6: phase 3
def test_phase3_twin_forward_reads_fresh_weight_images_after_every_step():
    """The stale-image case: the default encoder's convs (>= 16 input channels) and the GRUs keep packed images /
    transposes of the twin's weights in the weight cache; the fused step rewrites the weights without moving their
    version counters. A forward through engine.gen_ema after step k and again after step k + 1 must equal the forward of
    a fresh generator loaded from its state_dict."""
    import bench
    from music2dance_amd.engine import Phase3Engine, synthetic_phase3_batch
    k = K()
    gen, critic = bench.build_models(DEV, 120)
    eng = Phase3Engine(gen, critic, dict(bench.P3_DEFAULT, n_critic_steps=1), data_parallel=False)
    eng.enable_ema(0.5, warmup=False)
    fresh, _ = bench.build_models(DEV, 120)
    fresh.eval()
    real, audio, slices = synthetic_phase3_batch(4, 120, DEV, seed=3)
    _, _, probe = synthetic_phase3_batch(2, 120, DEV, seed=9)
    outs = []
    for step in range(2):
        out = eng.train_step(real, audio, slices)
        assert "loss_gen" in out and eng._ema.updates == step + 1
        twin = eng.gen_ema
        noise = torch.randn(2, 120, gen.noise_size, generator=torch.Generator().manual_seed(7)).to(DEV)
        with torch.no_grad():
            with k.weight_cache(keep=True):          # as the engine's own scopes: images survive between the steps
                launches = k.pack_launches
                got = twin(probe, [120] * 2, noise=noise)
                assert k.pack_launches > launches    # the twin's images were dropped by the step: packed afresh
                again = twin(probe, [120] * 2, noise=noise)
            fresh.load_state_dict(twin.state_dict(), strict=True)
            with k.weight_cache():
                want = fresh(probe, [120] * 2, noise=noise)
        assert torch.isfinite(got).all() and torch.equal(got, again) and torch.equal(got, want), step
        outs.append(got)
    eng.flush()
    assert not torch.equal(outs[0], outs[1])
    assert any(not torch.equal(a, b.detach()) for a, b in zip(eng.gen_ema.parameters(), gen.parameters()))


# ------------------------------------------------------------------------------------------------ 7: the script
def test_phase2_train_script_with_ema_decay(tmp_path, monkeypatch):
    import os
    from music2dance_amd.phase2 import train as T
    K()
    monkeypatch.chdir(tmp_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = yaml.safe_load(open(os.path.join(root, "music2dance_amd", "phase2", "configs", "default.yaml")))
    cfg.update(batch_size=4, num_train=8, num_epochs=4, n_critic_steps=2, ema_decay=0.999)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    # the phase-2 script sets the GEMM engine's PROCESS-WIDE plan model (kernels.set_plan_model): put it back, the
    # tests that run after this one expect the default
    from music2dance_amd import _lib
    model = _lib.lib().m2d_plan_model_get()
    try:
        eng = T.main(["-c", str(path), "-d", "0", "-n", "e", "-f", "wgangp", "--synthetic", "--no-run-dir",
                      "--iterations", "6"])
    finally:
        kernels.set_plan_model(model)
    assert eng.total_iterations == 6 and eng._ema.updates == 3
    twin = eng.gen_ema
    assert twin is not None and twin is not eng.gen and not twin.training
    sd, live = twin.state_dict(), eng.gen.state_dict()
    assert list(sd) == list(live) and all(torch.isfinite(v).all() for v in sd.values())
    assert any(not torch.equal(sd[k], live[k]) for k in sd)
