"""The GEMM engine's plan selection (csrc/gemm_engine.hip: select_plan), on the CPU: the library loads without a GPU and
the selection is host arithmetic. The recorded table of tests/plan_cases.py pins the plan of every layer shape to what the
launchers chose before selection became one function; the grid checks what must hold for any shape."""
import itertools

import pytest

from tests import plan_cases as C

ERR_WORKSPACE = -3
AMPLE = 1 << 40   # workspace bytes no slab of the grid comes near
GRID = list(itertools.product((32, 64, 128, 250), (8, 128, 7680), (1, 8, 56, 1200), (0, 1)))   # M, N, nchunks, statistics
LAUNCHERS = (C.GENERAL, C.K4)


@pytest.mark.parametrize("kind", ["fwd", "bwdD", "bwdW", "fwd_stats"])
def test_recorded_plans(kind):
    """Every recorded launch of this pass gets the (bm, splits, fused) the parent's launcher gave it on the MI355X."""
    rows = [r for r in C.RECORDED if r[1] == kind]
    assert len(rows) >= (7 if kind == "fwd_stats" else 20)
    wrong = []
    for name, _, conv, launcher, M, N, nchunks, phases, allow_split, pen100, plan_kind, bwd_data, tall, want in rows:
        stats = kind == "fwd_stats"
        got = C.select_plan(launcher, M, N, nchunks, phases, allow_split, pen100 / 100.0, plan_kind, bwd_data, stats,
                            C.launcher_ws_bytes(kind, conv, M, N), True, C.TICKET_BYTES, tall)
        if got != (0,) + want:
            wrong.append((name, got, want))
    assert not wrong, wrong


def test_the_k4_launches_of_the_table_are_recorded():
    assert sum(1 for r in C.RECORDED if r[3] == C.K4) >= 6


def test_statistics_split_only_in_one_launch():
    """With statistics a split plan is always the one-launch form - with everything available and with each of the three
    things the one-launch form needs taken away."""
    split = 0
    for launcher, (M, N, nchunks, stats) in itertools.product(LAUNCHERS, GRID):
        if not stats:
            continue
        for ws, aligned, tickets in ((AMPLE, True, C.TICKET_BYTES), (AMPLE, True, 0), (AMPLE, False, C.TICKET_BYTES),
                                     (0, True, C.TICKET_BYTES)):
            rc, bm, splits, fused = C.select_plan(launcher, M, N, nchunks, 1, 1, 1.0, 0, 0, 1, ws, aligned, tickets)
            assert rc == 0 and splits >= 1
            assert splits == 1 or fused == 1, (launcher, M, N, nchunks, ws, aligned, tickets)
            split += splits > 1
    assert split > 0   # (the grid does hold shapes that split)


def test_statistics_without_tickets_alignment_or_slab_do_not_split():
    """No ticket bytes, or a workspace off 16-byte alignment: a statistics launch runs unsplit. A workspace one byte short
    of the chosen plan's m2d_slab_bytes: that plan is not taken again; what is taken instead either is unsplit or is a
    smaller one-launch split whose slab does fit (the model's next candidate - the launchers have always fallen through
    the candidates in order), and taking the byte from each in turn ends at an unsplit launch."""
    chains = 0
    for launcher, (M, N, nchunks, stats) in itertools.product(LAUNCHERS, GRID):
        if not stats:
            continue
        q = (launcher, M, N, nchunks, 1, 1, 1.0, 0, 0, 1)
        assert C.select_plan(*q, AMPLE, True, 0)[2] == 1
        assert C.select_plan(*q, AMPLE, False, C.TICKET_BYTES)[2] == 1
        rc, bm, splits, fused = C.select_plan(*q, AMPLE, True, C.TICKET_BYTES)
        for _ in range(8):
            assert rc == 0
            if splits == 1:
                break
            ws = C.slab_bytes(M, N, bm, splits) - 1
            prev = (bm, splits)
            rc, bm, splits, fused = C.select_plan(*q, ws, True, C.TICKET_BYTES)
            assert (bm, splits) != prev and (splits == 1 or (fused == 1 and C.slab_bytes(M, N, bm, splits) <= ws))
            chains += 1
        assert splits == 1, (launcher, M, N, nchunks)
    assert chains > 0


def test_the_k4_launcher_keeps_64_rows_at_least():
    for (M, N, nchunks, stats), (ws, aligned, tickets) in itertools.product(
            GRID, ((AMPLE, True, C.TICKET_BYTES), (AMPLE, False, 0), (0, True, C.TICKET_BYTES))):
        rc, bm, splits, fused = C.select_plan(C.K4, M, N, nchunks, 1, 1, 1.0, 0, 0, stats, ws, aligned, tickets)
        assert rc == 0 and bm in (64, 128)


def test_without_workspace_the_general_launcher_fails_and_the_k4_launcher_runs_unsplit():
    """Where every candidate of the model splits K (one output tile, a K of 1 200 chunks: an unsplit launch is an order of
    magnitude beyond the model's 1.5 x cut) and there is no workspace: M2D_ERR_WORKSPACE from the general launcher, the
    unsplit 128-row plan from the k4 launcher. Where the general launcher does find a plan, it is unsplit."""
    assert C.select_plan(C.GENERAL, 64, 128, 1200, 1, 1, 1.0, 0, 0, 0, 0, True, C.TICKET_BYTES)[0] == ERR_WORKSPACE
    failed = 0
    for M, N, nchunks, stats in GRID:
        if stats:   # (a statistics launch plans again without splitting)
            continue
        q = (M, N, nchunks, 1, 1, 1.0, 0, 0, 0, 0, True, C.TICKET_BYTES)
        rc, bm, splits, fused = C.select_plan(C.GENERAL, *q)
        if rc == 0:
            assert splits == 1
            continue
        assert rc == ERR_WORKSPACE
        assert C.select_plan(C.GENERAL, M, N, nchunks, 1, 1, 1.0, 0, 0, 0, AMPLE, True, C.TICKET_BYTES)[2] > 1
        assert C.select_plan(C.K4, *q) == (0, 128, 1, 0)
        failed += 1
    assert failed > 0


def test_backward_data_is_never_fused():
    for launcher, (M, N, nchunks, stats), phases in itertools.product(LAUNCHERS, GRID, (1, 4)):
        rc, bm, splits, fused = C.select_plan(launcher, M, N, nchunks, phases, 1, 1.0, 0, 1, stats, AMPLE, True,
                                              C.TICKET_BYTES)
        assert rc == 0 and fused == 0
        assert not (stats and splits > 1)
