"""Host half of the lever tests (tests/lever_cases.py; the device half is tests/test_gpu_levers.py): the route witness of
the library answers in a process that never touched a GPU, every route name an arm asserts is one the library counts,
every work item names something that exists, the cases added for the levers agree with their own fp64 references on the
CPU stand-in of the kernel layer, and what lever_cases.py says about the plans of its statistics cases is what the
library's plan selection gives."""
import pytest
import torch

from tests import lever_cases as L
from tests import plan_cases as C
from tests.fake_backend import FakeKernels


def test_the_route_witness_answers_without_a_device():
    names = L.route_names()
    assert len(names) > 40 and len(set(names)) == len(names) and all(n and n == n.strip() and " " not in n for n in names)
    r = L.routes()
    assert list(r) == names and all(isinstance(v, int) and v >= 0 for v in r.values())
    # a short buffer gets its share and the full count comes back
    import ctypes
    buf = (ctypes.c_ulonglong * 3)(7, 7, 7)
    assert L._handle().m2d_debug_routes(buf, 2) == len(names) and buf[2] == 7
    assert L._handle().m2d_debug_routes(None, 0) == len(names)
    assert L.thin_wg_per_cu() == 0   # (no launch in this process)


def test_route_misses_reads_hit_miss_and_any_of():
    seen = dict.fromkeys(L.route_names(), 0)
    seen["k4_plain"], seen["epi_one"] = 2, 1
    assert L.route_misses(seen, ("k4_plain", ("k4_paired", "epi_one")), ("k4_paired", ("epi_wide", "gemm_dl8"))) == []
    assert L.route_misses(seen, ("k4_paired",), ()) == ["never ran: k4_paired"]
    assert L.route_misses(seen, (("k4_paired", "epi_wide"),), ("epi_one",)) == ["never ran: k4_paired / epi_wide", "ran 1 times: epi_one"]


@pytest.mark.parametrize("arm", list(L.ARMS.values()), ids=lambda a: a.name)
def test_an_arm_names_routes_and_work_that_exist(arm):
    names = set(L.route_names())
    for group in (arm.hit, arm.miss, arm.default_hit, arm.default_miss):
        for entry in group:
            for n in ((entry,) if isinstance(entry, str) else entry):
                assert n in names, (arm.name, n)
    assert arm.env and arm.work
    for item in arm.work:
        what = L.resolve(item)   # raises where the case or the function does not exist
        assert isinstance(what, L.Case) or callable(what[0]), item
    for n in arm.same_bits:
        assert (n,) in arm.work, (arm.name, n)
    names_run = {item[0] for item in arm.case_items()}
    for layer, kind in arm.plan_moves:   # a pass whose plan must move is a pass the arm runs, and its plan can be asked here
        assert "%s %s plain" % ({"fwd": "conv1d_fwd", "bwdD": "conv1d_bwd_data", "bwdW": "conv1d_bwd_weight"}[kind], layer) in names_run
        assert L.plan_of(layer, kind)[0] == 0
    if not (arm.hit or arm.miss or arm.thin_wg or arm.plan_moves):
        assert L.is_function(arm.work[0]) and arm.work[0][0].endswith(":engine_trace"), "an arm without a witness: " + arm.name
    # what must run in one position must not be demanded of the other as well, unless both positions share it on purpose
    assert not (set(arm.hit) & set(arm.miss)) and not (set(arm.default_hit) & set(arm.default_miss)), arm.name
    # an arm with routes to leave says which route its default position takes instead (or has no cases to run there)
    if arm.miss and arm.case_items():
        assert arm.default_hit, arm.name


def test_case_names_are_unique_across_both_tables():
    assert len(L.case_table()) == len(L.P.CASES) + len(L.CASES)


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_reference_agrees_with_the_cpu_stand_in(case):
    """as tests/test_placement_host.py does for the placement cases: shapes and references proven without a device"""
    figures = {}
    L.run_case(case, FakeKernels(), "cpu", figures=figures)
    assert figures[case.name] and all(ok for _, _, ok in figures[case.name])
    for name, v in case.operands().items():
        assert v.device == torch.device("cpu")


def _stats_plan(conv):
    """the plan of the layer's forward with epilogue statistics, as csrc/conv1d.hip asks for it: rows = output channels,
    columns = (sample, position), K chunks = taps x 16-channel blocks, the 1.25 small-tile penalty of strided forwards"""
    B, Cin, L_, Cout, ks, s, p = conv
    M, N = Cout, B * ((L_ + 2 * p - ks) // s + 1)
    ws = C.launcher_ws_bytes("fwd_stats", conv, M, N)
    plain = C.select_plan(C.GENERAL, M, N, ks * -(-Cin // 16), 1, 1, 1.0 if s == 1 else 1.25, 0, 0, 0, ws, True, C.TICKET_BYTES)
    stats = C.select_plan(C.GENERAL, M, N, ks * -(-Cin // 16), 1, 1, 1.0 if s == 1 else 1.25, 0, 0, 1, ws, True, C.TICKET_BYTES)
    return plain, stats


def test_which_statistics_case_splits_k():
    """lever_cases.LAYERS: at K = 3200 the model wants more splits than one launch finishes (and more still with more
    channels), so the statistics launch stays whole; at K = 384 it splits in one launch - the case the M2D_STATS_SPLIT arm
    stands on."""
    for cin in range(128, 1025, 128):
        plain, stats = _stats_plan((4, cin, 25, 128, 25, 1, 12))
        assert plain[0] == 0 and plain[2] > 16 and plain[3] == 0, (cin, plain)
        assert stats[0] == 0 and stats[2] == 1, (cin, stats)
    assert L.LAYERS["stats.k3200"] == (4, 128, 25, 128, 25, 1, 12)
    plain, stats = _stats_plan(L.LAYERS["stats.k384"])
    assert stats[0] == 0 and 1 < stats[2] <= 16 and stats[3] == 1, stats
    for name in ("stats.n125",):
        _, stats = _stats_plan(L.LAYERS[name])
        assert stats[:3] == (0, 32, 1) or stats[2] == 1, stats
    B, Cin, L_, Cout, ks, s, p = L.LAYERS["stats.n125"]
    assert (B * ((L_ + 2 * p - ks) // s + 1)) % 4 != 0   # rows of the output not on 16 bytes
