"""Launch plans of the GEMM engine: the recorded table tests/test_plan_host.py pins, and the ctypes binding of the
test-only export it (and the ticket test of test_gpu_kernels.py) asks. A helper, not a test module; it needs no GPU.

RECORDED holds, for the 28 layer shapes of tools/plan_sweep.py: CASES and the passes forward, backward-data,
backward-weight and - for the layers a BatchNorm follows - forward with epilogue statistics, what the engine's launcher
was asked and what it chose. It was recorded on an MI355X from a -DM2D_TUNING build (tools/build_variant.sh tune
-DM2D_TUNING) of the commit BEFORE plan selection became one function (select_plan): each conv ran once through
kernels.impl() and m2d_debug_last_plan was read back - for the k4 forwards, for `fused` (the launch has tickets:
split-K in one launch) and for tall_last_rb (the phase-major sub-pixel backward-data launch) from the same build with
those fields added to the record, in m2d_conv_k4_launch too.
A pass that never reaches the engine (the thin and TCN kernels) has no row. The expectations are therefore never the
output of the code under test. Regenerate the table ONLY when the cost model (plan_candidates, rounds_cost) or a
launcher's feasibility rule is changed on purpose - and then from the commit before that change plus the reviewed
differences, not by copying what the new code prints.

A row: (layer, pass, (B, Cin, L, Cout, k, stride, pad), launcher, M, N, nchunks, phases, allow_split,
        small-tile penalty x 100, plan kind, bwd_data, tall_last_rb, (bm, splits, fused)).
The workspace of a row is what the library's own m2d_conv1d_workspace_bytes asks for the conv (less the statistics
partials, which the conv entry point takes off the front before it calls the launcher), the tickets are the 64 KB every
stream gets (kernels._TICKET_WORDS), the workspace is 16-byte aligned.
"""
import contextlib
import ctypes

from music2dance_amd import _lib, kernels
from music2dance_amd.kernels import _TICKET_WORDS

GENERAL, K4 = 0, 1          # m2d_gemm_launch, m2d_conv_k4_launch
TICKET_BYTES = 4 * _TICKET_WORDS
_WHICH = {"fwd": 0, "fwd_stats": 0, "bwdD": 1, "bwdW": 2}
_h = None


def _handle():
    global _h
    if _h is None:
        _h = ctypes.CDLL(_lib.LIB_PATH)
        i, z = ctypes.c_int, ctypes.c_size_t
        _h.m2d_debug_select_plan.restype = None
        _h.m2d_debug_select_plan.argtypes = [i, i, i, i, i, i, ctypes.c_double, i, i, i, z, i, z, i, ctypes.POINTER(i)]
        _h.m2d_conv1d_workspace_bytes.restype = z
        _h.m2d_conv1d_workspace_bytes.argtypes = [i] * 8
        _h.m2d_gemm_workspace_bytes.restype = z
        _h.m2d_gemm_workspace_bytes.argtypes = [i] * 4
        _h.m2d_debug_force_plan.restype = i
        _h.m2d_debug_force_plan.argtypes = [i, i]
    return _h


def force_plan(bm, splits):
    """csrc/gemm_engine.hip: m2d_debug_force_plan -> rc. (0, 0) clears. The binding's cached workspace sizes follow the
    plans (kernels._ws_bytes): dropped with every change."""
    kernels._WS_BYTES.clear()
    return _handle().m2d_debug_force_plan(bm, splits)


@contextlib.contextmanager
def forced_plan(bm, splits):
    """Every engine launch inside the scope takes the plan (bm, splits) or is refused (M2dError); cleared on the way out."""
    try:
        rc = force_plan(bm, splits)
        assert rc == 0, (bm, splits, rc)
        yield
    finally:
        force_plan(0, 0)


def gemm_ws_bytes(mode, M, N, K):
    """include/m2d.h: m2d_gemm_workspace_bytes, uncached"""
    return _handle().m2d_gemm_workspace_bytes(mode, M, N, K)


def max_splits(nchunks, phases, allow_split, plan_kind):
    """The largest split factor a plan of this query may have under the default cost model (written out from DESIGN.md's
    plan-selection rules, not read from the library): 4 chunks per split at least, 128 splits (256 for the rounds-model
    kinds 1 and 2) at most, none for phased launches and under 8 chunks."""
    if not allow_split or phases > 1 or nchunks < 8:
        return 1
    return min(256 if plan_kind in (1, 2) else 128, nchunks // 4)


def select_plan(launcher, M, N, nchunks, phases, allow_split, penalty, plan_kind, bwd_data, stats, ws_bytes, ws_aligned,
                ticket_bytes, tall_last_rb=0):
    """-> (rc, bm, splits, fused) of csrc/gemm_engine.hip: select_plan (through m2d_debug_select_plan)"""
    out = (ctypes.c_int * 4)()
    _handle().m2d_debug_select_plan(launcher, M, N, nchunks, phases, int(allow_split), penalty, plan_kind, int(bwd_data),
                                    int(stats), ws_bytes, int(ws_aligned), ticket_bytes, tall_last_rb, out)
    return tuple(out)


def slab_bytes(M, N, bm, splits):
    """csrc/gemm_engine.h: m2d_slab_bytes - whole tiles"""
    return 0 if splits <= 1 else splits * (-(-M // bm) * bm) * (-(-N // 128) * 128) * 4


def rowstats_bytes(M, N):
    """csrc/gemm_engine.h: m2d_rowstats_bytes - the statistics partials in front of a statistics launch's workspace"""
    return ((-(-N // 128) * 4 * M * 2 * 4 + 15) & ~15) + 256 * M * 2 * 8


def launcher_ws_bytes(kind, conv, M, N):
    ws = _handle().m2d_conv1d_workspace_bytes(_WHICH[kind], *conv)
    return ws - rowstats_bytes(M, N) if kind == "fwd_stats" else ws


RECORDED = [
    ('stick.conv1 B64', 'fwd', (64, 69, 120, 128, 25, 1, 12), GENERAL, 128, 7680, 125, 1, 1, 100, 0, 0, 0, (64, 4, 1)),
    ('stick.conv1 B64', 'bwdD', (64, 69, 120, 128, 25, 1, 12), GENERAL, 69, 7680, 200, 1, 1, 0, 0, 0, 0, (32, 4, 1)),
    ('stick.conv1 B64', 'bwdW', (64, 69, 120, 128, 25, 1, 12), GENERAL, 128, 1725, 512, 1, 1, 0, 1, 0, 0, (128, 36, 0)),
    ('audio_d.l2', 'fwd', (64, 32, 19200, 64, 25, 4, 11), K4, 64, 307200, 56, 1, 1, 100, 0, 0, 0, (64, 1, 0)),
    ('audio_d.l2', 'bwdD', (64, 32, 19200, 64, 25, 4, 11), GENERAL, 128, 307264, 28, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('audio_d.l2', 'bwdW', (64, 32, 19200, 64, 25, 4, 11), GENERAL, 64, 800, 19200, 1, 1, 0, 1, 0, 0, (64, 256, 0)),
    ('audio_d.l3', 'fwd', (64, 64, 4800, 128, 25, 4, 11), K4, 128, 76800, 112, 1, 1, 100, 0, 0, 0, (64, 1, 0)),
    ('audio_d.l3', 'bwdD', (64, 64, 4800, 128, 25, 4, 11), GENERAL, 256, 76864, 56, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('audio_d.l3', 'bwdW', (64, 64, 4800, 128, 25, 4, 11), GENERAL, 128, 1600, 4800, 1, 1, 0, 1, 0, 0, (128, 78, 0)),
    ('audio_d.l4', 'fwd', (64, 128, 1200, 256, 25, 4, 11), GENERAL, 256, 19200, 200, 1, 1, 125, 0, 0, 0, (128, 4, 1)),
    ('audio_d.l4', 'bwdD', (64, 128, 1200, 256, 25, 4, 11), GENERAL, 128, 19200, 112, 4, 0, 0, 2, 1, 0, (64, 1, 0)),
    ('audio_d.l4', 'bwdW', (64, 128, 1200, 256, 25, 4, 11), GENERAL, 256, 3200, 1216, 1, 1, 0, 1, 0, 0, (128, 20, 0)),
    ('audio_d.l5', 'fwd', (64, 256, 300, 512, 25, 4, 11), GENERAL, 512, 4800, 400, 1, 1, 125, 0, 0, 0, (128, 5, 1)),
    ('audio_d.l5', 'bwdD', (64, 256, 300, 512, 25, 4, 11), GENERAL, 256, 4800, 224, 4, 0, 0, 2, 1, 0, (32, 1, 0)),
    ('audio_d.l5', 'bwdW', (64, 256, 300, 512, 25, 4, 11), GENERAL, 512, 6400, 320, 1, 1, 0, 1, 0, 0, (128, 5, 1)),
    ('audio_d2B.l2', 'fwd', (128, 32, 19200, 64, 25, 4, 11), K4, 64, 614400, 56, 1, 1, 100, 0, 0, 0, (64, 1, 0)),
    ('audio_d2B.l2', 'bwdD', (128, 32, 19200, 64, 25, 4, 11), GENERAL, 128, 614528, 28, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('audio_d2B.l2', 'bwdW', (128, 32, 19200, 64, 25, 4, 11), GENERAL, 64, 800, 38400, 1, 1, 0, 1, 0, 0, (64, 256, 0)),
    ('audio_d2B.l3', 'fwd', (128, 64, 4800, 128, 25, 4, 11), K4, 128, 153600, 112, 1, 1, 100, 0, 0, 0, (128, 1, 0)),
    ('audio_d2B.l3', 'bwdD', (128, 64, 4800, 128, 25, 4, 11), GENERAL, 256, 153728, 56, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('audio_d2B.l3', 'bwdW', (128, 64, 4800, 128, 25, 4, 11), GENERAL, 128, 1600, 9600, 1, 1, 0, 1, 0, 0, (128, 78, 0)),
    ('audio_d2B.l4', 'fwd', (128, 128, 1200, 256, 25, 4, 11), GENERAL, 256, 38400, 200, 1, 1, 125, 0, 0, 0, (128, 2, 1)),
    ('audio_d2B.l4', 'bwdD', (128, 128, 1200, 256, 25, 4, 11), GENERAL, 128, 38400, 112, 4, 0, 0, 2, 1, 0, (64, 1, 0)),
    ('audio_d2B.l4', 'bwdW', (128, 128, 1200, 256, 25, 4, 11), GENERAL, 256, 3200, 2432, 1, 1, 0, 1, 0, 0, (128, 20, 0)),
    ('audio_d2B.l5', 'fwd', (128, 256, 300, 512, 25, 4, 11), GENERAL, 512, 9600, 400, 1, 1, 125, 0, 0, 0, (128, 5, 1)),
    ('audio_d2B.l5', 'bwdD', (128, 256, 300, 512, 25, 4, 11), GENERAL, 256, 9600, 224, 4, 0, 0, 2, 1, 0, (64, 1, 0)),
    ('audio_d2B.l5', 'bwdW', (128, 256, 300, 512, 25, 4, 11), GENERAL, 512, 6400, 640, 1, 1, 0, 1, 0, 0, (128, 5, 1)),
    ('audio_dh.l2', 'fwd', (32, 32, 19200, 64, 25, 4, 11), K4, 64, 153600, 56, 1, 1, 100, 0, 0, 0, (64, 1, 0)),
    ('audio_dh.l2', 'bwdD', (32, 32, 19200, 64, 25, 4, 11), GENERAL, 128, 153632, 28, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('audio_dh.l2', 'bwdW', (32, 32, 19200, 64, 25, 4, 11), GENERAL, 64, 800, 9600, 1, 1, 0, 1, 0, 0, (64, 219, 0)),
    ('audio_dh.l3', 'fwd', (32, 64, 4800, 128, 25, 4, 11), K4, 128, 38400, 112, 1, 1, 100, 0, 0, 0, (64, 2, 1)),
    ('audio_dh.l3', 'bwdD', (32, 64, 4800, 128, 25, 4, 11), GENERAL, 256, 38432, 56, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('audio_dh.l3', 'bwdW', (32, 64, 4800, 128, 25, 4, 11), GENERAL, 128, 1600, 2400, 1, 1, 0, 1, 0, 0, (128, 78, 0)),
    ('audio_dh.l4', 'fwd', (32, 128, 1200, 256, 25, 4, 11), GENERAL, 256, 9600, 200, 1, 1, 125, 0, 0, 0, (128, 5, 1)),
    ('audio_dh.l4', 'bwdD', (32, 128, 1200, 256, 25, 4, 11), GENERAL, 128, 9600, 112, 4, 0, 0, 2, 1, 0, (32, 1, 0)),
    ('audio_dh.l4', 'bwdW', (32, 128, 1200, 256, 25, 4, 11), GENERAL, 256, 3200, 608, 1, 1, 0, 1, 0, 0, (128, 15, 1)),
    ('audio_dh.l5', 'fwd', (32, 256, 300, 512, 25, 4, 11), GENERAL, 512, 2400, 400, 1, 1, 125, 0, 0, 0, (128, 10, 1)),
    ('audio_dh.l5', 'bwdD', (32, 256, 300, 512, 25, 4, 11), GENERAL, 256, 2400, 224, 4, 0, 0, 2, 1, 0, (32, 1, 0)),
    ('audio_dh.l5', 'bwdW', (32, 256, 300, 512, 25, 4, 11), GENERAL, 512, 6400, 160, 1, 1, 0, 1, 0, 0, (128, 5, 1)),
    ('wavegan.l4', 'fwd', (3840, 128, 43, 256, 25, 4, 0), GENERAL, 256, 19200, 200, 1, 1, 125, 0, 0, 0, (128, 4, 1)),
    ('wavegan.l4', 'bwdD', (3840, 128, 43, 256, 25, 4, 0), GENERAL, 128, 42240, 112, 4, 0, 0, 2, 1, 0, (64, 1, 0)),
    ('wavegan.l4', 'bwdW', (3840, 128, 43, 256, 25, 4, 0), GENERAL, 256, 3200, 1200, 1, 1, 0, 0, 0, 0, (128, 10, 1)),
    ('wavegan.l4', 'fwd_stats', (3840, 128, 43, 256, 25, 4, 0), GENERAL, 256, 19200, 200, 1, 1, 125, 0, 0, 0, (128, 4, 1)),
    ('wavegan.l3', 'fwd', (3840, 64, 193, 128, 25, 4, 0), GENERAL, 128, 165120, 100, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('wavegan.l3', 'bwdD', (3840, 64, 193, 128, 25, 4, 0), GENERAL, 256, 188160, 56, 1, 0, 0, 2, 0, 1, (128, 1, 0)),
    ('wavegan.l3', 'bwdW', (3840, 64, 193, 128, 25, 4, 0), GENERAL, 128, 1600, 11520, 1, 1, 0, 1, 0, 0, (128, 78, 0)),
    ('wavegan.l3', 'fwd_stats', (3840, 64, 193, 128, 25, 4, 0), GENERAL, 128, 165120, 100, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c1', 'fwd', (7680, 32, 64, 64, 4, 2, 1), GENERAL, 64, 245760, 8, 1, 1, 125, 0, 0, 0, (64, 1, 0)),
    ('enc.c1', 'bwdD', (7680, 32, 64, 64, 4, 2, 1), GENERAL, 64, 253440, 8, 1, 0, 0, 2, 0, 0, (64, 1, 0)),
    ('enc.c1', 'bwdW', (7680, 32, 64, 64, 4, 2, 1), GENERAL, 64, 128, 15360, 1, 1, 0, 1, 0, 0, (32, 256, 0)),
    ('enc.c1', 'fwd_stats', (7680, 32, 64, 64, 4, 2, 1), GENERAL, 64, 245760, 8, 1, 1, 125, 0, 0, 0, (64, 1, 0)),
    ('enc.c2', 'fwd', (7680, 64, 32, 128, 4, 2, 1), GENERAL, 128, 122880, 16, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c2', 'bwdD', (7680, 64, 32, 128, 4, 2, 1), GENERAL, 128, 130560, 16, 1, 0, 0, 2, 0, 0, (128, 1, 0)),
    ('enc.c2', 'bwdW', (7680, 64, 32, 128, 4, 2, 1), GENERAL, 128, 256, 7680, 1, 1, 0, 1, 0, 0, (128, 256, 0)),
    ('enc.c2', 'fwd_stats', (7680, 64, 32, 128, 4, 2, 1), GENERAL, 128, 122880, 16, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c3', 'fwd', (7680, 128, 16, 256, 4, 2, 1), GENERAL, 256, 61440, 32, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c3', 'bwdD', (7680, 128, 16, 256, 4, 2, 1), GENERAL, 128, 61440, 32, 2, 0, 0, 2, 1, 0, (128, 1, 0)),
    ('enc.c3', 'bwdW', (7680, 128, 16, 256, 4, 2, 1), GENERAL, 256, 512, 3840, 1, 1, 0, 0, 0, 0, (128, 64, 0)),
    ('enc.c3', 'fwd_stats', (7680, 128, 16, 256, 4, 2, 1), GENERAL, 256, 61440, 32, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c4', 'fwd', (7680, 256, 8, 512, 4, 2, 1), GENERAL, 512, 30720, 64, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c4', 'bwdD', (7680, 256, 8, 512, 4, 2, 1), GENERAL, 256, 30720, 64, 2, 0, 0, 2, 1, 0, (128, 1, 0)),
    ('enc.c4', 'bwdW', (7680, 256, 8, 512, 4, 2, 1), GENERAL, 512, 1024, 1920, 1, 1, 0, 0, 0, 0, (128, 16, 1)),
    ('enc.c4', 'fwd_stats', (7680, 256, 8, 512, 4, 2, 1), GENERAL, 512, 30720, 64, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c5', 'fwd', (7680, 512, 4, 1024, 4, 2, 1), GENERAL, 1024, 15360, 128, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c5', 'bwdD', (7680, 512, 4, 1024, 4, 2, 1), GENERAL, 512, 15360, 128, 2, 0, 0, 2, 1, 0, (128, 1, 0)),
    ('enc.c5', 'bwdW', (7680, 512, 4, 1024, 4, 2, 1), GENERAL, 1024, 2048, 960, 1, 1, 0, 0, 0, 0, (128, 4, 1)),
    ('enc.c5', 'fwd_stats', (7680, 512, 4, 1024, 4, 2, 1), GENERAL, 1024, 15360, 128, 1, 1, 125, 0, 0, 0, (128, 1, 0)),
    ('enc.c6', 'fwd', (7680, 1024, 2, 250, 2, 1, 0), GENERAL, 250, 7680, 128, 1, 1, 0, 0, 0, 0, (128, 4, 1)),
    ('enc.c6', 'bwdD', (7680, 1024, 2, 250, 2, 1, 0), GENERAL, 7680, 2048, 16, 1, 1, 0, 0, 0, 0, (128, 1, 0)),
    ('enc.c6', 'bwdW', (7680, 1024, 2, 250, 2, 1, 0), GENERAL, 250, 2048, 480, 1, 1, 0, 0, 0, 0, (128, 16, 1)),
]
