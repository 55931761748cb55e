"""Every kernel-path lever of DESIGN.md section 16 in its other position (tests/lever_cases.py: ARMS), one test per arm.

The library reads a switch once per process (a function-local `static const`), so an arm's work runs in a fresh child
process with the arm's environment - the pattern of tests/test_gpu_kernels.py:
test_from_sums_forwards_with_the_separate_finalize_launch. The child runs the arm's work items in order - cases of
tests/placement_cases.py and tests/lever_cases.py against their own fp64 references and bounds, existing GPU test
functions that assert against fp64 torch or the reference's golden files - and saves its results, its figures and the
ROUTES the library took (csrc/m2d_common.h: one host-side counter per kernel form). The parent asserts: the child ended
well; every route the arm must reach ran and every route it must leave did not (so an arm whose shape does not qualify
for the switched path fails instead of passing on the default path); every figure is inside its case's bound. Then the
parent runs the arm's cases in its own process, without the environment - the default arm - and asserts ITS routes: what
the comments of placement_cases.py say about which kernel a layer reaches ("phase-major at 32 channels", "phantom-paired
order", the TemporalBlock and single-channel kernels) is held here. The largest difference between the two arms is noted
per arm (WORST) and asserted only where lever_cases.py says, with its reason, that no sum changes its order (same_bits).

If a child dies (a signal, an abort, the time limit) nothing more is started: every later arm fails at once. A test that
merely fails does not stop the others. At most the parent and one child hold the device at a time.
"""
import os
import subprocess
import sys

import pytest
import torch

from tests import lever_cases as L
from tests import placement_cases as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORST = {}   # printed by tests/conftest.py with every run
DIED = []    # the arm whose child died, once one has


def note(key, val):
    WORST[key] = max(WORST.get(key, 0.0), float(val))


def run_child(arm, out):
    code = ("import sys; sys.path.insert(0, %r); from tests import lever_cases as L; L.run_arm(%r, %r)" % (ROOT, arm.name, out))
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **arm.env), cwd=ROOT, capture_output=True,
                           text=True, timeout=120)
    except subprocess.TimeoutExpired:
        DIED.append(arm.name)
        pytest.fail("the child of arm %s did not end within 120 s" % arm.name)
    if r.returncode < 0 or r.returncode in (134, 137, 139):
        DIED.append(arm.name)
    assert r.returncode == 0, "child of arm %s ended with %d\n%s" % (arm.name, r.returncode, r.stderr[-3000:])
    return torch.load(out)


@pytest.fixture
def default_plan_model():
    """the process-wide plan model is the default one while the parent plays the default arm (a train script run earlier in
    the same process may have left the other one: kernels.set_plan_model)"""
    from music2dance_amd import _lib, kernels
    model = _lib.lib().m2d_plan_model_get()
    kernels.set_plan_model(4)
    yield
    kernels.set_plan_model(model)


@pytest.mark.parametrize("arm", list(L.ARMS.values()), ids=lambda a: a.name)
def test_lever_arm(arm, tmp_path, default_plan_model):
    if DIED:
        pytest.fail("not started: an earlier arm died (%s)" % DIED[0])
    theirs = run_child(arm, str(tmp_path / "arm.pt"))
    print("arm %s: %.1f s of work in the child; routes %s" % (arm.name, theirs["seconds"],
                                                              {k: v for k, v in theirs["routes"].items() if v}))
    note("lever arm %s: seconds of work in the child" % arm.name, theirs["seconds"])
    # every figure against its bound, from the saved figures: a failure names the case
    for name, rows in theirs["figures"].items():
        for i, (fig, bound, ok) in enumerate(rows):
            print("arm %s | %s | result %d: %.3e (bound %s)" % (arm.name, name, i, fig, bound))
            assert ok, (arm.name, name, i, fig, bound)
    assert theirs["error"] is None, "arm %s:\n%s" % (arm.name, theirs["error"])
    bad = L.route_misses(theirs["routes"], arm.hit, arm.miss)
    assert not bad, "arm %s: %s; routes %s" % (arm.name, "; ".join(bad), {k: v for k, v in theirs["routes"].items() if v})
    if arm.thin_wg is not None:
        assert theirs["thin_wg"] == arm.thin_wg, (arm.name, theirs["thin_wg"])
    for move in arm.plan_moves:   # the levers that only move a plan: the plan of a pass the arm ran is another one
        there, here = tuple(theirs["plans"]["%s %s" % move]), L.plan_of(*move)
        print("arm %s | plan of %s %s: %s, by default %s" % (arm.name, move[0], move[1], there[1:], here[1:]))
        assert there[0] == 0 and here[0] == 0 and there != here, (arm.name, move, there, here)

    # the default arm: the same cases in this process
    items = arm.case_items()
    if not items:
        return
    from music2dance_amd import kernels
    before = L.routes()
    mine, figures = {}, {}
    L.run_items(items, mine, figures)
    seen = L.routes_since(before)
    print("default arm of %s: routes %s" % (arm.name, {k: v for k, v in seen.items() if v}))
    bad = L.route_misses(seen, arm.default_hit, arm.default_miss)
    assert not bad, "default arm of %s: %s; routes %s" % (arm.name, "; ".join(bad), {k: v for k, v in seen.items() if v})
    if arm.thin_wg is not None:
        assert L.thin_wg_per_cu() == 4
    assert sorted(mine) == sorted(theirs["results"])
    worst = 0.0
    for key, outs in mine.items():
        for i, (a, b) in enumerate(zip(outs, theirs["results"][key])):
            if not a.is_floating_point():
                assert torch.equal(a, b), (arm.name, key, i)
                continue
            d = P.rel_err(b, a.double())
            worst = max(worst, d)
            if key in arm.same_bits:
                assert torch.equal(a, b), (arm.name, key, i, "differs from the default arm", d)
    note("lever arm %s: largest difference to the default arm" % arm.name, worst)
    assert kernels.impl().name == "hip"
