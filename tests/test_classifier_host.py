"""Dance-style classifier and phase-3 evaluation: everything that needs no GPU.

Constructor surface and seeded-construction parity against tests/golden/cls.npz (made from the reference's own
module by tests/golden/make_golden_classifier.py), reference checkpoint round trip, the new C-ABI entries, the host
logic of the evaluation (confusion matrix, jerkiness statistics) and both command lines."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cls.npz")
NEW_SYMBOLS = ("m2d_gru_small_fwd", "m2d_gru_small_bwd", "m2d_cross_entropy_workspace_bytes", "m2d_cross_entropy_fwd",
               "m2d_cross_entropy_bwd")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _classifier():
    from music2dance_amd.dance_classification.archis.default import RecurrentDanceClassifier
    return RecurrentDanceClassifier


def test_constructor_surface_keys_and_shapes(gold):
    m = _classifier()(69, 128, 4)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold["keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in gold["shapes"]]
    assert m.conv1.kernel_size == (9,) and m.conv1.padding == (4,)
    assert len(m.blocks) == 1 and m.blocks[0].ksize == 7
    assert m.rnn.hidden_size == 4 and m.rnn.num_layers == 1 and m.rnn.batch_first
    two = _classifier()(69, 32, 4, init_ker=5, n_blocks=2)
    assert "blocks.1.conv2.weight" in two.state_dict() and two.conv1.padding == (2,)


def test_seeded_construction_matches_reference(gold):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_classifier as G
    torch.manual_seed(G.CTOR_SEED)
    sd = _classifier()(69, 128, 4).state_dict()
    for k, v in sd.items():
        v = v.double()
        ref = gold["init/%s:checksum" % k]
        np.testing.assert_allclose([v.sum().item(), v.abs().sum().item()], ref, rtol=1e-9, atol=1e-9, err_msg=k)
        if "init/%s:full" % k in gold:
            np.testing.assert_array_equal(v.numpy(), gold["init/%s:full" % k], err_msg=k)
        else:
            idx = G.sample_index(v.numel(), k)
            np.testing.assert_array_equal(v.reshape(-1)[idx].numpy(), gold["init/%s:sample" % k], err_msg=k)


def test_reference_state_dict_round_trip(gold, tmp_path):
    from tests.golden import patterns as P
    ref_sd = P.fill_state_dict(P.template(gold["keys"], gold["shapes"]), 42)
    path = tmp_path / "weights.pt"
    torch.save(ref_sd, path)
    m = _classifier()(69, 128, 4)
    m.load_state_dict(torch.load(path))  # strict: same keys, same shapes
    back = m.state_dict()
    assert list(back) == list(ref_sd)
    for k in ref_sd:
        assert torch.equal(back[k], ref_sd[k]), k


def test_header_and_ctypes_table_carry_the_new_entries():
    from music2dance_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "m2d.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"m2d_cross_entropy_fwd\([^;]*const long long\* labels[^;]*long long\* pred", text, flags=re.S)
    assert _lib.SIGNATURES["m2d_cross_entropy_workspace_bytes"][0] is _lib._S


def test_confusion_matrix_is_square_row_normalised_with_nan_rows():
    from music2dance_amd.phase3.evaluate import confusion, summary
    real = [0, 0, 0, 1, 1, 3]
    fake = [0, 2, 2, 1, 3, 3]
    cm, counts = confusion(real, fake, 4)
    assert cm.shape == (4, 4) and counts.sum() == 6
    np.testing.assert_allclose(cm[0], [1 / 3, 0, 2 / 3, 0])
    np.testing.assert_allclose(cm[1], [0, 0.5, 0, 0.5])
    assert np.isnan(cm[2]).all()  # style 2 never predicted for a real take
    np.testing.assert_allclose(cm[3], [0, 0, 0, 1])
    s = summary([1.0, 2.0, 3.0], [2.0, 2.0, 2.0], real, fake)
    assert s["n_sequences"] == 6
    assert s["style_agreement"] == pytest.approx(3 / 6)
    assert len(s["confusion"]) == 4 and all(len(r) == 4 for r in s["confusion"])


def test_evaluation_json_is_strict():
    import json

    from music2dance_amd.phase3.evaluate import json_safe, summary
    s = summary([1.0], [2.0], [0], [1])  # one sequence: no spread, three empty confusion rows
    text = json.dumps(json_safe(s), allow_nan=False)
    back = json.loads(text)
    assert back["jerk_real_std"] is None and back["confusion"][1] == [None] * 4
    assert back["confusion"][0] == [0.0, 1.0, 0.0, 0.0]


def test_jerk_statistics_are_mean_and_unbiased_std():
    from music2dance_amd.phase3.evaluate import jerk_stats
    v = [0.5, 1.5, 2.0, 4.0]
    m, s = jerk_stats(v)
    t = torch.tensor(v, dtype=torch.float64)
    assert m == pytest.approx(t.mean().item()) and s == pytest.approx(t.std().item())
    assert np.isnan(jerk_stats([1.0])[1])


def test_latest_generator_checkpoint(tmp_path):
    from music2dance_amd.phase3.evaluate import latest_checkpoint
    assert latest_checkpoint(str(tmp_path)) is None
    (tmp_path / "models").mkdir()
    for it in (100, 900, 5000, 1000):
        (tmp_path / "models" / ("gpgen_%d.pt" % it)).write_bytes(b"")
    (tmp_path / "models" / "gpcritic_90000.pt").write_bytes(b"")
    assert latest_checkpoint(str(tmp_path)).endswith("gpgen_5000.pt")


def test_classifier_cli(capsys):
    from music2dance_amd.dance_classification import main
    with pytest.raises(SystemExit) as e:
        main.parse_args(["--help"])
    assert e.value.code == 0
    assert "-c CONFIG" in capsys.readouterr().out
    o = main.parse_args(["-c", "x.yaml", "-d", "1", "-n", "type2", "--synthetic", "--epochs", "2"])
    assert (o.config, o.device, o.name, o.synthetic, o.epochs) == ("x.yaml", 1, "type2", True, 2)


def test_evaluate_cli(capsys):
    from music2dance_amd.phase3 import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.parse_args(["--help"])
    assert e.value.code == 0
    assert "--classifier" in capsys.readouterr().out
    o = evaluate.parse_args(["-c", "a.yaml", "-l", "run", "--classifier", "w.pt"])
    assert (o.repeats, o.gen_weights, o.synthetic) == (20, None, False)
    with pytest.raises(SystemExit):
        evaluate.parse_args(["-c", "a.yaml", "-l", "run"])  # the classifier is required


def test_configs_carry_the_reference_keys():
    import yaml
    cfg = yaml.safe_load(open(os.path.join(ROOT, "music2dance_amd", "dance_classification", "configs",
                                           "default.yaml")))
    assert (cfg["batch_size"], cfg["lr"]) == (49, 2e-4)
    assert set(cfg) >= {"num_epochs", "batch_size", "seq_length", "lr", "dance_types", "dataset", "folder"}
    from music2dance_amd.dance_classification.main import stick_length
    assert stick_length(cfg) == 120


@pytest.mark.parametrize("stem,kernels", [("gru", ("m2d_gru_small_fwd_kernel", "m2d_gru_small_bwd_kernel")),
                                          ("pointwise", ("m2d_ce_fwd_rows_kernel", "m2d_ce_bwd_kernel"))])
def test_new_kernels_have_no_scratch(stem, kernels):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_info
    obj = os.path.join(ROOT, "music2dance_amd", "lib", "obj", stem + ".o")
    if not os.path.exists(obj):
        from music2dance_amd import build
        build.build(verbose=False)
    if isa_info._tool("llvm-readelf") is None:
        pytest.skip("llvm-readelf not installed")
    import shutil
    co = isa_info.code_object(stem)
    try:
        tab = isa_info.kernel_table(co)
    finally:
        shutil.rmtree(os.path.dirname(co), ignore_errors=True)
    for k in kernels:
        rows = [r for n, r in tab.items() if n.startswith(k + "(")]
        assert rows, k
        for r in rows:
            assert r["scratch"] == 0 and r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0, (k, r)
