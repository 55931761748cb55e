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


# ---------------------------------------------------------------------------- the forced plan (m2d_debug_force_plan)
ERR_ARG = -1
FORCED = [(bm, splits) for bm in (32, 64, 128) for splits in (1, 2, 3, 14, 16, 20, 128, 256)]


@pytest.fixture(scope="module", autouse=True)
def _no_forced_plan_is_left_behind():
    yield
    assert C.force_plan(0, 0) == 0


def _admits(launcher, nchunks, phases, allow_split, plan_kind, stats, tall, bm, splits, M, N, ws, aligned, tickets):
    """What the envelope says, written out independently of the library: -> None (admitted) or the rc of the refusal."""
    if tall:
        return None if (bm, splits) == (128, 1) else ERR_ARG
    if launcher == C.K4 and bm == 32:
        return ERR_ARG
    if splits == 1:
        return None
    if splits > C.max_splits(nchunks, phases, allow_split, plan_kind):
        return ERR_ARG
    slab = C.slab_bytes(M, N, bm, splits)
    if ws < slab:
        return ERR_WORKSPACE
    one_launch = (splits <= 16 and aligned and slab < 0x7fffffff and
                  tickets >= 4 * (-(-M // bm)) * (-(-N // 128)))
    return ERR_ARG if stats and not one_launch else None


def test_force_plan_takes_the_three_tile_heights_and_1_to_256_splits_only():
    try:
        for bm, splits in ((0, 1), (16, 1), (48, 2), (256, 1), (64, 0), (64, -1), (64, 257), (0, 3), (32, 0)):
            assert C.force_plan(bm, splits) == ERR_ARG, (bm, splits)
            # a refused setting leaves the selection as it was: the model's
            assert C.select_plan(C.GENERAL, 64, 128, 1200, 1, 1, 1.0, 0, 0, 0, AMPLE, True, C.TICKET_BYTES)[2] > 1
        for bm, splits in FORCED:
            assert C.force_plan(bm, splits) == 0
    finally:
        assert C.force_plan(0, 0) == 0


@pytest.mark.parametrize("forced", FORCED, ids=lambda f: "%dx%d" % f)
def test_a_forced_plan_is_taken_exactly_or_refused(forced):
    """Over the grid, both launchers, every plan kind, phased and unsplittable launches, with and without tickets, an
    aligned and a misaligned workspace: inside the envelope select_plan returns exactly the forced (bm, splits) - in
    one launch exactly where decide_fused's conditions hold - and outside it the refusal's error code, never another
    plan."""
    bm, splits = forced
    taken = refused = 0
    with C.forced_plan(bm, splits):
        for launcher, (M, N, nchunks, stats), (phases, allow_split, kind), (aligned, tickets) in itertools.product(
                LAUNCHERS, GRID, ((1, 1, 0), (1, 1, 1), (1, 1, 2), (4, 1, 2), (1, 0, 0)),
                ((True, C.TICKET_BYTES), (True, 0), (False, C.TICKET_BYTES))):
            got = C.select_plan(launcher, M, N, nchunks, phases, allow_split, 1.0, kind, 0, stats, AMPLE, aligned, tickets)
            want = _admits(launcher, nchunks, phases, allow_split, kind, stats, 0, bm, splits, M, N, AMPLE, aligned, tickets)
            what = (launcher, M, N, nchunks, stats, phases, allow_split, kind, aligned, tickets)
            if want is None:
                assert got[:3] == (0, bm, splits), (what, got)
                one_launch = splits > 1 and splits <= 16 and aligned and tickets > 0
                assert got[3] == int(one_launch), (what, got)
                taken += 1
            else:
                assert got[0] == want, (what, got)
                refused += 1
    assert taken > 0 and (refused > 0 or (bm, splits) in ((64, 1), (128, 1)))


def test_each_rule_of_the_envelope_refuses():
    q = dict(M=128, N=7680, nchunks=56, phases=1, allow_split=1, penalty=1.0, plan_kind=0, bwd_data=0, stats=0,
             ws_bytes=AMPLE, ws_aligned=True, ticket_bytes=C.TICKET_BYTES)
    sel = lambda launcher, **kw: C.select_plan(launcher, **dict(q, **kw))
    with C.forced_plan(32, 1):     # 32 rows on the k4 launcher
        assert sel(C.GENERAL) == (0, 32, 1, 0)
        assert sel(C.K4)[0] == ERR_ARG
    with C.forced_plan(64, 14):    # 56 chunks: 14 splits of 4 chunks at most
        assert sel(C.GENERAL) == (0, 64, 14, 1) and sel(C.K4) == (0, 64, 14, 1)
    with C.forced_plan(64, 15):
        assert sel(C.GENERAL)[0] == ERR_ARG and sel(C.K4)[0] == ERR_ARG
    with C.forced_plan(64, 2):
        assert sel(C.GENERAL, nchunks=7)[0] == ERR_ARG      # fewer than 8 chunks
        assert sel(C.GENERAL, nchunks=8) == (0, 64, 2, 1)
        assert sel(C.GENERAL, allow_split=0)[0] == ERR_ARG   # the launcher forbids the split
        assert sel(C.GENERAL, phases=4, plan_kind=2, bwd_data=1)[0] == ERR_ARG   # a phased backward-data launch
        assert sel(C.GENERAL, phases=4, plan_kind=2, bwd_data=1, allow_split=0)[0] == ERR_ARG
        # statistics: the one-launch form or nothing
        assert sel(C.GENERAL, stats=1) == (0, 64, 2, 1)
        assert sel(C.GENERAL, stats=1, ticket_bytes=0)[0] == ERR_ARG
        assert sel(C.GENERAL, stats=1, ws_aligned=False)[0] == ERR_ARG
        assert sel(C.GENERAL, stats=1, ticket_bytes=4 * 2 * 60 - 4)[0] == ERR_ARG   # one ticket short of the 2 x 60 tiles
        assert sel(C.GENERAL, stats=1, ticket_bytes=4 * 2 * 60) == (0, 64, 2, 1)
        # the workspace holds the slab - whole tiles - or the launch is refused
        slab = C.slab_bytes(120, 7000, 64, 2)
        assert slab > 2 * 120 * 7000 * 4
        assert sel(C.GENERAL, M=120, N=7000, ws_bytes=slab) == (0, 64, 2, 1)
        assert sel(C.GENERAL, M=120, N=7000, ws_bytes=slab - 1)[0] == ERR_WORKSPACE
        assert sel(C.GENERAL, M=120, N=7000, ws_bytes=0)[0] == ERR_WORKSPACE
        assert sel(C.K4, M=120, N=7000, ws_bytes=slab - 1)[0] == ERR_WORKSPACE   # (no quiet (128, 1) either)
    with C.forced_plan(128, 129):  # 128 splits at most under the general model, 256 under the rounds model's kinds
        assert sel(C.GENERAL, nchunks=1200)[0] == ERR_ARG
        assert sel(C.GENERAL, nchunks=1200, plan_kind=1) == (0, 128, 129, 0)
    with C.forced_plan(64, 1):     # the phase-major sub-pixel launch: whole 128-row tiles, whole K
        assert sel(C.GENERAL, tall_last_rb=1, allow_split=0, plan_kind=2)[0] == ERR_ARG
    with C.forced_plan(128, 2):
        assert sel(C.GENERAL, tall_last_rb=1, plan_kind=2)[0] == ERR_ARG
    with C.forced_plan(128, 1):
        assert sel(C.GENERAL, tall_last_rb=1, allow_split=0, plan_kind=2) == (0, 128, 1, 0)
        assert sel(C.K4) == (0, 128, 1, 0)


@pytest.mark.parametrize("mnk", [(261, 260, 1283), (37, 100, 400), (250, 720, 7680), (7680, 720, 250), (33, 69, 0)], ids=str)
def test_the_size_query_covers_a_forced_split(mnk):
    """m2d_gemm_workspace_bytes under a forced plan the shape admits: the slab at least; a select_plan with exactly that
    many bytes takes the plan. Under one it does not admit, and after clearing: what the model alone asks for."""
    M, N, Kd = mnk
    nchunks = -(-Kd // 16)
    natural = C.gemm_ws_bytes(0, M, N, Kd)
    for bm, splits in FORCED:
        with C.forced_plan(bm, splits):
            ws = C.gemm_ws_bytes(0, M, N, Kd)
            got = C.select_plan(C.GENERAL, M, N, nchunks, 1, 1, 0.0, 0, 0, 0, ws, True, C.TICKET_BYTES)
        if splits <= C.max_splits(nchunks, 1, 1, 0):
            assert ws >= C.slab_bytes(M, N, bm, splits) and ws >= natural
            assert got[:3] == (0, bm, splits)
        else:
            assert ws == natural and got[0] == ERR_ARG
    assert C.gemm_ws_bytes(0, M, N, Kd) == natural


@pytest.mark.parametrize("kind", ["fwd", "bwdD", "bwdW", "fwd_stats"])
def test_recorded_plans_hold_again_after_a_force_and_clear(kind):
    """Forced, the recorded launches take the forced plan or are refused (the table's own plans are gone); cleared, the
    table holds again in the same process, workspace sizes included."""
    rows = [r for r in C.RECORDED if r[1] == kind]
    with C.forced_plan(32, 2):
        for name, _, conv, launcher, M, N, nchunks, phases, allow_split, pen100, plan_kind, bwd_data, tall, want in rows:
            got = C.select_plan(launcher, M, N, nchunks, phases, allow_split, pen100 / 100.0, plan_kind, bwd_data,
                                kind == "fwd_stats", C.launcher_ws_bytes(kind, conv, M, N), True, C.TICKET_BYTES, tall)
            assert got[0] != 0 or got[1:3] == (32, 2), (name, got)
            assert got != (0,) + want
    test_recorded_plans(kind)
