"""The generator EMA above the kernel layer, no GPU: the decay schedule, optim.Adam with shadows against optim.Adam
without (parameters and moments equal, shadows within tests/ema_cases.py's bound of the fp64 average), parameters
without / with late gradients, the optimizer's state_dict, a tiny Phase2Engine (update count, critic-only bodies, the
twin's keys and buffers), the scripts' checkpoint lists, and the scoring driver's --ema. Kernels are the CPU stand-in of
tests/fake_backend.py, extended here by the `ema=` form of adam_multi."""
import argparse
import glob
import os

import pytest
import torch
import yaml

from music2dance_amd import kernels, runner
from music2dance_amd.optim import Adam
from tests import ema_cases as C
from tests.fake_backend import FakeKernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class FakeEmaKernels(FakeKernels):
    """FakeKernels whose adam_multi understands `ema=` (m2d_adam_multi_ema in torch ops: the shadow moves in fp32 towards
    the fresh parameter; a raised skip voids it with the step)."""

    name = "fake-cpu-ema"

    def __init__(self):
        self.ema_calls = 0
        self.invalidated = []

    def invalidate_packed(self, tensors=None):
        self.invalidated.append(None if tensors is None else [id(t) for t in tensors])

    def adam_multi(self, params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, step, skip=None, repack=True,
                   ema=None, ema_decay=None):
        super().adam_multi(params, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, step, skip=skip, repack=repack)
        if ema is None or (skip is not None and float(skip) != 0.0):
            return
        assert ema_decay is not None and len(ema) == len(params)
        self.ema_calls += 1
        omd = torch.tensor(1.0 - float(ema_decay), dtype=torch.float32)
        with torch.no_grad():
            for p, e in zip(params, ema):
                if e is not None:
                    e.add_(omd * (p - e))


@pytest.fixture
def fake(monkeypatch):
    k = FakeEmaKernels()
    prev = kernels.set_impl(k)
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    try:
        yield k
    finally:
        kernels.set_impl(prev)


# ------------------------------------------------------------------------------------------------ the schedule
def test_decay_schedule():
    from music2dance_amd.ema import decay_at
    assert [decay_at(n, 0.999) for n in (0, 1, 10)] == [1 / 10, 2 / 11, 11 / 20]
    assert decay_at(8990, 0.999) == 8991 / 9000 and decay_at(8991, 0.999) == 0.999 and decay_at(10 ** 6, 0.999) == 0.999
    assert decay_at(0, 0.05) == 0.05                                          # a decay below the ramp is itself
    assert [decay_at(n, 0.999, warmup=False) for n in (0, 1, 10 ** 6)] == [0.999] * 3
    steps = [decay_at(n, 0.9) for n in range(200)]
    assert steps == sorted(steps) and steps[-1] == 0.9


def test_generator_ema_counts_and_hands_out_the_schedule(fake):
    from music2dance_amd.ema import GeneratorEMA
    gen = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    opt = Adam(gen.parameters(), lr=1e-3)
    ema = GeneratorEMA(gen, opt, 0.999)
    assert ema.updates == 0 and ema.next_decay() == 0.1
    ema.stepped()
    assert ema.updates == 1 and ema.next_decay() == 2 / 11
    assert fake.invalidated[-1] == [id(p) for p in ema.twin.parameters()]
    assert GeneratorEMA(gen, Adam(gen.parameters()), 0.5, warmup=False).next_decay() == 0.5
    with pytest.raises(RuntimeError, match="M2D_ADAM=torch"):
        GeneratorEMA(gen, torch.optim.Adam(gen.parameters()), 0.999)
    for bad in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            GeneratorEMA(gen, Adam(gen.parameters()), bad)


# ------------------------------------------------------------------------------------------------ the optimizer
SHAPES = [(6, 5, 3), (16,), (33, 7), (3,), (1, 9)]
DEAD, LATE = 3, 1   # never a gradient; first gradient at step 2


def _run(track, steps=6, decays=(0.1, 0.5, 0.9, 0.999, 0.9999, 0.5)):
    ps = [p.requires_grad_(True) for p in C.tensors(SHAPES, seed=0)]
    opt = Adam(ps, lr=2e-3)
    shadows = [p.detach().clone() for p in ps]
    ref = C.Ema64(shadows)
    if track:
        opt.track_ema(zip(ps, shadows))
    for step in range(steps):
        gs = C.grads(SHAPES, seed=10 + step)
        stepped = set()
        for i, p in enumerate(ps):
            p.grad = None if (i == DEAD or (i == LATE and step < 2)) else gs[i]
            if p.grad is not None:
                stepped.add(i)
        opt.ema_decay = decays[step]
        opt.step()
        ref.update(ps, decays[step], which=stepped)
    return ps, opt, shadows, ref


def test_tracked_adam_equals_untracked_adam_and_the_fp64_average(fake):
    ps0, opt0, untouched, _ = _run(track=False)
    assert fake.ema_calls == 0
    ps, opt, shadows, ref = _run(track=True)
    assert fake.ema_calls == 2 + 4 * 2              # from step 2 on the late parameter's step-count group is a call of its own
    for a, b in zip(ps, ps0):
        assert torch.equal(a, b)
    for a, b in zip(ps, ps0):
        assert (a in opt.state) == (b in opt0.state)
        if a in opt.state:
            for key in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(opt.state[a][key], opt0.state[b][key]), key
    ref.check(shadows, "tracked")
    assert ref.n == [6, 4, 6, 0, 6]
    # the parameter without a gradient is not stepped: no state, the shadow is still the initial copy = the live value
    assert ps[DEAD] not in opt.state and torch.equal(shadows[DEAD], ps[DEAD].detach())
    assert float(opt.state[ps[LATE]]["step"]) == 4.0 and float(opt.state[ps[0]]["step"]) == 6.0
    for i in (0, 1, 2, 4):
        assert not torch.equal(shadows[i], ps[i].detach()) and not torch.equal(shadows[i], untouched[i])
    for a, b in zip(untouched, C.tensors(SHAPES, seed=0)):   # untracked: nobody writes the would-be shadows
        assert torch.equal(a, b)


def test_ema_decay_unset_leaves_the_shadows_alone(fake):
    ps = [p.requires_grad_(True) for p in C.tensors(SHAPES[:2], seed=1)]
    shadows = [p.detach().clone() for p in ps]
    opt = Adam(ps, lr=1e-2)
    opt.track_ema(zip(ps, shadows))
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [s.clone() for s in shadows]
    opt.step()                                          # ema_decay is None: today's call
    assert fake.ema_calls == 0 and all(torch.equal(a, b) for a, b in zip(before, shadows))
    opt.ema_decay, opt.skip_flag = 0.5, torch.ones(())  # a raised skip voids parameters and shadows
    held = [p.detach().clone() for p in ps]
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, shadows))
    assert all(torch.equal(a, b.detach()) for a, b in zip(held, ps))
    opt.skip_flag = torch.zeros(())
    opt.step()
    assert not any(torch.equal(a, b) for a, b in zip(before, shadows))


def test_track_ema_refuses_what_cannot_be_a_shadow(fake):
    ps = [p.requires_grad_(True) for p in C.tensors(SHAPES[:2], seed=1)]
    opt = Adam(ps, lr=1e-2)
    with pytest.raises(ValueError, match="not a parameter"):
        opt.track_ema([(torch.zeros(3, requires_grad=True), torch.zeros(3))])
    with pytest.raises(ValueError, match="shape"):
        opt.track_ema([(ps[0], torch.zeros(4))])
    with pytest.raises(ValueError, match="storage of its own"):
        opt.track_ema([(ps[0], ps[0].detach())])
    opt.track_ema([(ps[0], ps[0].detach().clone())])
    opt.ema_decay = 1.5
    ps[0].grad = torch.ones_like(ps[0])
    with pytest.raises(ValueError, match="ema_decay"):
        opt.step()


def test_state_dict_keeps_its_layout_and_loads_into_torch_adam(fake):
    ps, opt, shadows, _ = _run(track=True, steps=3)
    ps0, opt0, _, _ = _run(track=False, steps=3)
    sd, sd0 = opt.state_dict(), opt0.state_dict()
    assert sorted(sd) == sorted(sd0) == ["param_groups", "state"]
    assert sd["param_groups"] == sd0["param_groups"] and sorted(sd["state"]) == sorted(sd0["state"])
    for k in sd["state"]:
        assert sorted(sd["state"][k]) == ["exp_avg", "exp_avg_sq", "step"]
        for key in sd["state"][k]:
            assert torch.equal(sd["state"][k][key], sd0["state"][k][key])
    again = torch.optim.Adam([p.detach().clone().requires_grad_(True) for p in ps], lr=2e-3)
    again.load_state_dict(sd)
    assert len(again.state_dict()["state"]) == len(SHAPES) - 1


# ------------------------------------------------------------------------------------------------ the engine
NZ, B, T = 8, 4, 24
CFG = {"lr_gen": 1e-3, "lr_critic": 1e-3, "n_critic_steps": 2, "gamma": 10, "eta": 50, "input_vector_size": NZ}


def _engine(seed=0):
    from music2dance_amd.engine import Phase2Engine
    from music2dance_amd.phase2.archis.default import SequenceDiscriminator, SequenceGenerator
    torch.manual_seed(seed)
    gen = SequenceGenerator(NZ, NZ, 16, 69, 1, 1, "cpu")
    critic = SequenceDiscriminator(69, 8, T, 5, 1, "cpu")
    return Phase2Engine(gen, critic, CFG, data_parallel=False)


def test_phase2_engine_keeps_the_average(fake):
    eng = _engine()
    assert eng.gen_ema is None and eng.enable_ema(None).gen_ema is None and eng.enable_ema(0).gen_ema is None
    eng.enable_ema(0.999)
    state = eng._ema
    assert eng.enable_ema(0.999)._ema is state                                # idempotent
    twin = eng.gen_ema
    assert type(twin) is type(eng.gen) and twin is not eng.gen and not twin.training
    assert list(twin.state_dict()) == list(eng.gen.state_dict())
    live = dict(eng.gen.named_parameters())
    for k, p in twin.named_parameters():
        assert not p.requires_grad and torch.equal(p, live[k].detach()) and p.data_ptr() != live[k].data_ptr()
    ref = C.Ema64(list(twin.parameters()))
    real = torch.rand(B, T, 69, generator=torch.Generator().manual_seed(3))
    gen_steps = 0
    for body in range(1, 7):
        before = [p.clone() for p in twin.parameters()]
        had_grad = None
        out = eng.train_step(real)
        if body % 2:
            # a critic-only body: no generator step, the shadows are what they were
            assert "loss_gen" not in out and state.updates == gen_steps
            assert all(torch.equal(a, b) for a, b in zip(before, twin.parameters()))
        else:
            d = min(0.999, (1 + gen_steps) / (10 + gen_steps))
            assert eng.optim_gen.ema_decay == d
            had_grad = {i for i, p in enumerate(eng.gen.parameters()) if p in eng.optim_gen.state}
            ref.update(list(eng.gen.parameters()), d, which=had_grad)
            gen_steps += 1
            assert "loss_gen" in out and state.updates == gen_steps
            assert fake.invalidated[-1] == [id(p) for p in twin.parameters()]
    assert gen_steps == 3 and fake.ema_calls == 3
    ref.check(list(twin.parameters()), "phase 2")
    # parameters that never get a gradient (the dead fc1 / bn1 of every LinearBlock) keep the live value
    dead = [k for k, p in eng.gen.named_parameters() if p not in eng.optim_gen.state]
    assert dead and all(torch.equal(dict(twin.named_parameters())[k], live[k].detach()) for k in dead)
    moved = [k for k, p in twin.named_parameters() if not torch.equal(p, live[k].detach())]
    assert len(moved) == len(live) - len(dead)
    # buffers are not averaged: handing the twin out copies the live ones
    bufs = dict(eng.gen.named_buffers())
    assert bufs and any(not torch.equal(b, dict(twin.named_buffers())[k]) for k, b in bufs.items())
    handed = eng.gen_ema
    assert handed is twin and not handed.training
    for k, b in handed.named_buffers():
        assert torch.equal(b, bufs[k]) and b.data_ptr() != bufs[k].data_ptr()
    # the file is an ordinary generator state_dict
    fresh = _engine(seed=5).gen
    fresh.load_state_dict(handed.state_dict(), strict=True)
    eng.enable_ema(0)
    assert eng.gen_ema is None


def test_ema_needs_the_fused_step(fake, monkeypatch):
    monkeypatch.setenv("M2D_ADAM", "torch")
    eng = _engine()
    assert type(eng.optim_gen) is torch.optim.Adam
    assert eng.enable_ema(None).gen_ema is None
    with pytest.raises(RuntimeError, match="M2D_ADAM=torch"):
        eng.enable_ema(0.999)


# ------------------------------------------------------------------------------------------------ the scripts
_DUE = {"phase1.train_wgan_gp": (5, [("gen", "gen_5.pt"), ("gen_ema", "gen_ema_5.pt"), ("critic", "critic_5.pt")]),
        "phase2.train": (5000, [("gen", "gpgen_5000.pt"), ("gen_ema", "gpgen_ema_5000.pt"), ("critic", "gpcritic_5000.pt")]),
        "phase2.train_conditional": (5000, [("gen", "gpgen_5000.pt"), ("gen_ema", "gpgen_ema_5000.pt"),
                                            ("critic", "gpcritic_5000.pt")]),
        "phase3.train": (5000, [("gen", "gpgen_5000.pt"), ("gen_ema", "gpgen_ema_5000.pt"), ("critic", "gpcritic_5000.pt")])}


@pytest.mark.parametrize("name", sorted(_DUE))
def test_checkpoint_lists_with_and_without_ema(name):
    import importlib
    schedule = importlib.import_module("music2dance_amd." + name).checkpoints
    n, due = _DUE[name]
    assert list(schedule(n - 1, ema=True)) == due
    assert list(schedule(n - 1, ema=False)) == list(schedule(n - 1)) == [d for d in due if d[0] != "gen_ema"]
    assert list(schedule(n, ema=True)) == list(schedule(n)) == []
    if name == "phase3.train":
        assert schedule(99, ema=True) == [("gen", "gpgen_100.pt"), ("gen_ema", "gpgen_ema_100.pt")]
        assert schedule(99) == [("gen", "gpgen_100.pt")]


def _cfg(tmp_path, src, **over):
    cfg = yaml.safe_load(open(os.path.join(ROOT, "music2dance_amd", src)))
    cfg.update(over)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path), cfg


def test_shipped_configs_leave_ema_off():
    for path in glob.glob(os.path.join(ROOT, "music2dance_amd", "phase*", "configs", "*.yaml")):
        cfg = yaml.safe_load(open(path))
        assert "ema_decay" not in cfg and "ema_warmup" not in cfg, path
        if os.path.basename(path) == "default.yaml":
            assert "# ema_decay:" in open(path).read(), path


def test_a_run_with_ema_decay_writes_the_averaged_generator(fake, tmp_path, monkeypatch):
    """Six one-batch epochs of phase 1 (n_critic_steps = 5: one generator step) with a run directory: gen_ema_5.pt
    beside gen_5.pt, an ordinary generator state_dict that the scoring driver's --ema finds."""
    from music2dance_amd import scoring
    from music2dance_amd.phase1 import train_wgan_gp as T
    from music2dance_amd.phase1.archis.residual import Generator
    monkeypatch.chdir(tmp_path)
    path, cfg = _cfg(tmp_path, "phase1/configs/b2l50s32.yaml", batch_size=8, num_train=8, num_epochs=6, ema_decay=0.999)
    eng = T.main(["-c", path, "-d", "0", "-n", "ck", "--synthetic"])
    assert eng.total_iterations == 6 and eng._ema.updates == 1 and eng._ema.warmup
    run = glob.glob(str(tmp_path / "runs" / "*_ck"))[0]
    assert sorted(os.listdir(run + "/models")) == ["critic_5.pt", "gen_5.pt", "gen_ema_5.pt"]
    last, avg = (torch.load(run + "/models/" + f, map_location="cpu") for f in ("gen_5.pt", "gen_ema_5.pt"))
    assert list(last) == list(avg) and any(not torch.equal(last[k], avg[k]) for k in last)
    for k in last:   # buffers are the live generator's
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(last[k], avg[k]), k
    gen = Generator(cfg["latent_vector_size"], cfg["size"], cfg["output_size"], cfg["nblocks_gen"])
    opts = argparse.Namespace(logdir=run, gen_weights=None, synthetic=False, ema=True)
    assert scoring.load_generator(gen, opts, "gen").endswith("models/gen_ema_5.pt")
    assert all(torch.equal(v, avg[k]) for k, v in gen.state_dict().items())
    # ema_warmup: false, and ema_decay: null / 0 / absent = off
    path, _ = _cfg(tmp_path, "phase1/configs/b2l50s32.yaml", batch_size=8, num_train=8, num_epochs=1, ema_decay=0.9,
                   ema_warmup=False)
    eng = T.main(["-c", path, "-d", "0", "-n", "w", "--synthetic", "--no-run-dir"])
    assert not eng._ema.warmup and eng._ema.decay == 0.9
    for off in ({"ema_decay": None}, {"ema_decay": 0}, {}):
        path, _ = _cfg(tmp_path, "phase1/configs/b2l50s32.yaml", batch_size=8, num_train=8, num_epochs=1, **off)
        assert T.main(["-c", path, "-d", "0", "-n", "o", "--synthetic", "--no-run-dir"]).gen_ema is None


def test_phase3_validation_logs_the_twin(fake, tmp_path, monkeypatch):
    from music2dance_amd.phase3 import train as T3
    monkeypatch.chdir(tmp_path)
    seen = []
    orig = runner.ScalarLog.scalars
    monkeypatch.setattr(runner.ScalarLog, "scalars", lambda self, d, step, **kw: (seen.append((sorted(d), step)),
                                                                                 orig(self, d, step, **kw))[1])
    small = dict(batch_size=2, num_train=4, num_epochs=1, n_critic_steps=2)
    argv = ["-d", "0", "-n", "s", "--synthetic", "--no-run-dir"]
    path, _ = _cfg(tmp_path, "phase3/configs/ablated.yaml", ema_decay=0.5, **small)
    eng = T3.main(["-c", path] + argv)
    assert eng._ema.updates == 1 and eng.gen.training and not eng.gen_ema.training
    assert [t for t, _ in seen if t[0].startswith("l1_loss_val")] == [["l1_loss_val"], ["l1_loss_val_ema"]]
    assert torch.isfinite(T3.LAST_LOG.last["l1_loss_val_ema"])
    assert float(T3.LAST_LOG.last["l1_loss_val_ema"]) != float(T3.LAST_LOG.last["l1_loss_val"])
    del seen[:]
    path, _ = _cfg(tmp_path, "phase3/configs/ablated.yaml", **small)
    T3.main(["-c", path] + argv)
    assert [t for t, _ in seen if t[0].startswith("l1_loss_val")] == [["l1_loss_val"]]


# ------------------------------------------------------------------------------------------------ scoring
def test_latest_checkpoint_and_load_generator_with_both_kinds_of_file(tmp_path):
    from music2dance_amd import scoring
    (tmp_path / "models").mkdir()
    for name, fill in (("gpgen_100", 1.0), ("gpgen_300", 3.0), ("gpgen_ema_100", 10.0), ("gpgen_ema_200", 20.0),
                       ("gen_5", 5.0)):
        torch.save({"weight": torch.full((2, 2), fill), "bias": torch.full((2,), fill)},
                   str(tmp_path / "models" / (name + ".pt")))
    assert scoring.latest_checkpoint(str(tmp_path), "gpgen").endswith("models/gpgen_300.pt")       # not gpgen_ema_*
    assert scoring.latest_checkpoint(str(tmp_path), "gpgen_ema").endswith("models/gpgen_ema_200.pt")
    assert scoring.latest_checkpoint(str(tmp_path), "gen").endswith("models/gen_5.pt")
    assert scoring.latest_checkpoint(str(tmp_path), "gen_ema") is None
    gen = torch.nn.Linear(2, 2)
    opts = argparse.Namespace(logdir=str(tmp_path), gen_weights=None, synthetic=False, ema=True)
    assert scoring.load_generator(gen.train(), opts).endswith("gpgen_ema_200.pt")
    assert float(gen.weight.detach()[0, 0]) == 20.0 and not gen.training
    opts.ema = False
    assert scoring.load_generator(gen, opts).endswith("gpgen_300.pt") and float(gen.bias.detach()[0]) == 3.0
    opts.ema, opts.gen_weights = True, str(tmp_path / "models" / "gpgen_100.pt")                   # --gen-weights wins
    assert scoring.load_generator(gen, opts) == opts.gen_weights and float(gen.bias.detach()[0]) == 1.0
    # --ema with no averaged checkpoint: exits saying so, unless --synthetic allows random weights
    opts = argparse.Namespace(logdir=str(tmp_path), gen_weights=None, synthetic=False, ema=True)
    with pytest.raises(SystemExit, match=r"--ema: no averaged-generator checkpoint .*gen_ema_\*\.pt"):
        scoring.load_generator(gen, opts, "gen")
    opts.synthetic = True
    assert scoring.load_generator(gen, opts, "gen") is None


def test_the_four_scoring_parsers_take_ema():
    from music2dance_amd.phase1 import evaluate as E1
    from music2dance_amd.phase2 import evaluate as E2
    from music2dance_amd.phase3 import evaluate as E3
    from music2dance_amd.phase3 import generate as G
    base = ["-c", "x.yaml", "-l", "run"]
    for m, own in ((E1, []), (E2, ["--classifier", "w.pt"]), (E3, ["--classifier", "w.pt"]), (G, ["--val"])):
        assert m.parse_args(base + own).ema is False and m.parse_args(base + own + ["--ema"]).ema is True
