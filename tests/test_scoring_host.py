"""The scoring driver (music2dance_amd.scoring) that phase1.evaluate, phase2.evaluate, phase3.evaluate and
phase3.generate share, no GPU: the checkpoint lookup with both stems, load_generator's three ends, the six common flags
of the four parsers, run()'s JSON, seed and return value, and distribution_scores through the numpy stand-in of
tests/distribution_cases.py (the five keys for both tags, the small-N values, the capped seeded diversity subset)."""
import argparse
import json
import math

import numpy as np
import pytest
import torch

from tests import distribution_cases as C

COMMON = ("config", "logdir", "gen_weights", "synthetic", "folder", "device")


@pytest.fixture
def stand_in(monkeypatch):
    from music2dance_amd import kernels
    monkeypatch.setattr(kernels, "impl", lambda: C.NumpyDistributionBackend())


def _rows(N, D=6, seed=9, scale=1.0):
    return torch.from_numpy((scale * np.random.default_rng(seed).standard_normal((N, D))).astype(np.float32))


def test_latest_checkpoint_with_both_stems(tmp_path):
    from music2dance_amd import scoring
    from music2dance_amd.phase1 import evaluate as E1
    from music2dance_amd.phase3 import evaluate as E3
    assert scoring.latest_checkpoint(str(tmp_path)) is None and scoring.latest_checkpoint(str(tmp_path), "gen") is None
    (tmp_path / "models").mkdir()
    for name in ("gen_5", "gen_20", "gpgen_7", "critic_25"):
        (tmp_path / "models" / (name + ".pt")).write_bytes(b"")
    assert scoring.latest_checkpoint(str(tmp_path), "gen").endswith("models/gen_20.pt")      # not gpgen_7, not critic_25
    assert scoring.latest_checkpoint(str(tmp_path), "gpgen").endswith("models/gpgen_7.pt")
    assert scoring.latest_checkpoint(str(tmp_path)).endswith("models/gpgen_7.pt")            # the default stem
    assert scoring.latest_checkpoint(str(tmp_path), "critic").endswith("models/critic_25.pt")
    assert E1.latest_checkpoint(str(tmp_path)).endswith("gen_20.pt")
    assert E3.latest_checkpoint(str(tmp_path)).endswith("gpgen_7.pt")
    assert scoring.latest_checkpoint(str(tmp_path / "models"), "gen") is None


def test_load_generator(tmp_path):
    from music2dance_amd import scoring
    gen = torch.nn.Linear(2, 2).train()
    opts = argparse.Namespace(logdir=str(tmp_path), gen_weights=str(tmp_path / "missing.pt"), synthetic=True)
    with pytest.raises(SystemExit, match="generator checkpoint .*missing.pt not found"):      # --synthetic or not
        scoring.load_generator(gen, opts, "gen")
    opts = argparse.Namespace(logdir=str(tmp_path), gen_weights=None, synthetic=False)
    with pytest.raises(SystemExit, match="no generator checkpoint: pass --gen-weights or train into %s/models"
                                         % str(tmp_path)):
        scoring.load_generator(gen, opts, "gen")
    assert gen.training
    opts.synthetic = True
    assert scoring.load_generator(gen, opts, "gen") is None and not gen.training
    # the latest checkpoint of the stem, and a named file over it
    (tmp_path / "models").mkdir()
    for name, fill in (("gen_5", 5.0), ("gen_20", 20.0), ("gpgen_30", 30.0)):
        torch.save({"weight": torch.full((2, 2), fill), "bias": torch.full((2,), fill)},
                   str(tmp_path / "models" / (name + ".pt")))
    opts.synthetic = False
    path = scoring.load_generator(gen.train(), opts, "gen")
    assert path.endswith("gen_20.pt") and float(gen.weight.detach()[0, 0]) == 20.0 and not gen.training
    assert scoring.load_generator(gen, opts).endswith("gpgen_30.pt") and float(gen.bias.detach()[1]) == 30.0
    opts.gen_weights = str(tmp_path / "models" / "gen_5.pt")
    assert scoring.load_generator(gen, opts, "gen") == opts.gen_weights and float(gen.weight.detach()[1, 1]) == 5.0


def test_the_four_parsers_share_the_six_flags(capsys):
    from music2dance_amd.phase1 import evaluate as E1
    from music2dance_amd.phase2 import evaluate as E2
    from music2dance_amd.phase3 import evaluate as E3
    from music2dance_amd.phase3 import generate as G
    base = ["-c", "x.yaml", "-l", "run"]
    parsers = [(E1, []), (E2, ["--classifier", "w.pt"]), (E3, ["--classifier", "w.pt"])]
    plain = [m.parse_args(base + own) for m, own in parsers] + [G.parse_args(base + ["--val"])]
    for o in plain:
        assert {d: getattr(o, d) for d in COMMON} == {"config": "x.yaml", "logdir": "run", "gen_weights": None,
                                                      "synthetic": False, "folder": None, "device": None}
    given = ["--config", "y.yaml", "--logdir", "r2", "--gen-weights", "g.pt", "--synthetic", "--folder", "f",
             "--device", "1"]
    for m, own in parsers + [(G, [])]:
        o = m.parse_args(given + own)
        assert [getattr(o, d) for d in COMMON] == ["y.yaml", "r2", "g.pt", True, "f", 1]
        for missing in (["-l", "run"], ["-c", "x.yaml"]):                 # -c and -l are required everywhere
            with pytest.raises(SystemExit):
                m.parse_args(missing + own + ["--synthetic"])
    with pytest.raises(SystemExit):                                       # generate: --synthetic is one of the sources
        G.parse_args(base + ["--synthetic", "--val"])
    capsys.readouterr()


def test_run_writes_prints_seeds_and_returns(tmp_path, monkeypatch, capsys):
    from music2dance_amd import runner, scoring
    monkeypatch.setattr(runner, "pick_device", lambda idx: torch.device("cpu"))
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("size: 7\n")
    logdir = tmp_path / "a" / "run"                                       # made by run()
    seen = []
    result = {"x": float("nan"), "y": [1.5, float("inf")], "z": {"n": 3, "t": True}, "s": None}

    def parse(argv):
        seen.append(("argv", argv))
        return argparse.Namespace(config=str(cfg), logdir=str(logdir), device=None)

    def body(opts, cfg, device):
        seen.append((opts.logdir, cfg, device, torch.initial_seed()))
        return result

    strict = lambda s: json.loads(s, parse_constant=lambda c: pytest.fail("not strict JSON: %s" % c))
    want = {"x": None, "y": [1.5, None], "z": {"n": 3, "t": True}, "s": None}
    torch.manual_seed(1234)
    assert scoring.run(parse, body, ["-q"], out="evaluation.json") is result
    assert torch.initial_seed() == 1234                                   # seed=None: the generator is left alone
    assert seen == [("argv", ["-q"]), (str(logdir), {"size": 7}, torch.device("cpu"), 1234)]
    text = (logdir / "evaluation.json").read_text()
    assert strict(text) == want and list(strict(text)) == list(result) and text == json.dumps(want, indent=1)
    printed = capsys.readouterr().out.strip().splitlines()
    assert len(printed) == 1 and strict(printed[0]) == want
    # seed=0: seeded before the body; out=None: printed only
    (logdir / "evaluation.json").unlink()
    assert scoring.run(parse, body, None, seed=0) is result
    assert seen[-1][-1] == 0 and torch.initial_seed() == 0 and not (logdir / "evaluation.json").exists()
    assert strict(capsys.readouterr().out.strip()) == want


@pytest.mark.parametrize("tag", ["pose", "kinetic"])
def test_distribution_scores_at_12_rows(stand_in, monkeypatch, tag):
    from music2dance_amd import metrics, scoring
    keys = ["fd_%s" % tag, "fd_%s_real_split" % tag, "fd_%s_converged" % tag, "div_%s_real" % tag, "div_%s_fake" % tag]
    real, fake = _rows(12), _rows(12, seed=10, scale=1.5)
    calls = []
    frechet = metrics.frechet_from_moments
    monkeypatch.setattr(metrics, "frechet_from_moments", lambda *a: (calls.append(tuple(a[0].shape)), frechet(*a))[1])
    d = scoring.distribution_scores(real, fake, tag)
    assert list(d) == keys + ["Zr", "Zf"] and calls == [(2, 6)]           # both pairs in ONE Frechet call
    assert d[keys[2]] is True and all(isinstance(d[k], float) and math.isfinite(d[k]) for k in keys[:2] + keys[3:])
    # the values are the fp64 statement's on the rows standardised by the REAL set's moments
    m, S = C.moments(real.numpy())
    Zr = ((real.numpy() - m) / np.sqrt(np.diag(S))).astype(np.float32)
    Zf = ((fake.numpy() - m) / np.sqrt(np.diag(S))).astype(np.float32)
    np.testing.assert_allclose(d["Zr"].numpy(), Zr, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(d["Zf"].numpy(), Zf, rtol=1e-6, atol=1e-7)
    Zr, Zf = d["Zr"].numpy(), d["Zf"].numpy()
    assert d[keys[0]] == pytest.approx(C.fd_eigh(*C.moments(Zr), *C.moments(Zf))[0], rel=1e-9)
    assert d[keys[1]] == pytest.approx(C.fd_eigh(*C.moments(Zr[0::2]), *C.moments(Zr[1::2]))[0], rel=1e-9)
    assert d[keys[3]] == pytest.approx(C.pairwise(Zr)[0], rel=1e-12)
    assert d[keys[4]] == pytest.approx(C.pairwise(Zf)[0], rel=1e-12)
    # a list of generated sets: the first is scored, every set comes back standardised
    many = scoring.distribution_scores(real, [fake, real], tag)
    assert {k: many[k] for k in keys} == {k: d[k] for k in keys} and len(many["Zf"]) == 2
    assert torch.equal(many["Zf"][0], d["Zf"]) and torch.equal(many["Zf"][1], d["Zr"]) and len(calls) == 2


def test_distribution_scores_with_too_few_rows(stand_in):
    from music2dance_amd import scoring
    keys = ["fd_pose", "fd_pose_real_split", "fd_pose_converged", "div_pose_real", "div_pose_fake"]
    real, fake = _rows(3), _rows(3, seed=10)
    few = scoring.distribution_scores(real, fake, "pose")                 # 3 rows: no even / odd split
    assert math.isnan(few["fd_pose_real_split"]) and scoring.json_safe(few["fd_pose_real_split"]) is None
    assert math.isfinite(few["fd_pose"]) and few["fd_pose_converged"] is True and few["div_pose_real"] > 0
    assert tuple(few["Zr"].shape) == (3, 6)
    one = scoring.distribution_scores(real[:1], fake[:1], "pose")         # 1 row: nothing is defined
    assert all(math.isnan(one[k]) for k in keys[:2] + keys[3:]) and one["fd_pose_converged"] is None
    assert one["Zr"] is None and one["Zf"] is None
    assert scoring.json_safe({k: one[k] for k in keys}) == dict.fromkeys(keys)


def test_distribution_scores_caps_the_diversity_rows(stand_in):
    from music2dance_amd import metrics, scoring
    from music2dance_amd.phase1 import evaluate as E1
    real, fake = _rows(40), _rows(33, seed=10, scale=1.5)
    full = scoring.distribution_scores(real, fake, "pose")
    cap = scoring.distribution_scores(real, fake, "pose", max_rows=16, seed=3)
    assert cap["fd_pose"] == full["fd_pose"] and cap["fd_pose_real_split"] == full["fd_pose_real_split"]
    assert torch.equal(cap["Zr"], full["Zr"]) and torch.equal(cap["Zf"], full["Zf"])        # all rows come back
    for side, Z in (("real", full["Zr"]), ("fake", full["Zf"])):
        sub = E1._subset(Z, 16, 3)
        idx = torch.randperm(Z.shape[0], generator=torch.Generator().manual_seed(3))[:16].sort().values
        assert torch.equal(sub, Z[idx]) and sub.shape[0] == 16
        assert cap["div_pose_%s" % side] == float(metrics.mean_pairwise_distance(sub)[0])
        assert cap["div_pose_%s" % side] == pytest.approx(C.pairwise(Z[idx].numpy())[0], rel=1e-12)
        assert cap["div_pose_%s" % side] != full["div_pose_%s" % side]
    other = scoring.distribution_scores(real, fake, "pose", max_rows=16, seed=4)
    assert other["div_pose_real"] != cap["div_pose_real"]
    roomy = scoring.distribution_scores(real, fake, "pose", max_rows=40, seed=3)            # no more rows than the cap
    assert roomy["div_pose_real"] == full["div_pose_real"] and roomy["div_pose_fake"] == full["div_pose_fake"]
