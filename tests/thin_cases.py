"""The single-channel (Cin = 1, Cout = 32) conv kernels of csrc/conv1d_thin.hip at shapes where a wave walks several
tiles: the case tables tests/test_thin_schedule_host.py and tests/test_gpu_thin_persistent.py share, and the ctypes
binding of the test-only export both ask. A helper, not a test module; it needs no GPU.

The three forwards are persistent: a fixed grid of G waves, wave g walks the tiles g, g + G, g + 2G, ... (a tile = 32
channels x 32 positions of one sample) with the next tile's operands prefetched under the current one. A case's `r` is
ceil(tiles / G): some waves then run r tiles and some r - 1, so every exit of the loop is taken. The backward kernels
share a sample's positions out in blocks of `chunk` positions (thin_bw_chunk: 1 024 for B * Lout <= 524 288).
The expectations (tiles, r, chunk, blocks) are worked out by hand from the shapes and the grids the kernels' comments
state - 4 096 waves for k25 and k160, 2 048 for k250; the host test compares them with what the launchers' own
functions say, so the GPU tests cannot silently stop reaching the loop when a grid is retuned.
"""
import ctypes

from music2dance_amd import _lib

K25_FWD, LONG_FWD, BWD_WEIGHT, BWD_DATA = 0, 1, 2, 3
COUT = 32
_h = None


def _handle():
    global _h
    if _h is None:
        _h = ctypes.CDLL(_lib.LIB_PATH)
        i = ctypes.c_int
        _h.m2d_debug_thin_schedule.restype = None
        _h.m2d_debug_thin_schedule.argtypes = [i, i, i, i, i, i, ctypes.POINTER(i)]
    return _h


def schedule(which, B, L, ks, stride, pad):
    """csrc/conv1d_thin.hip: m2d_debug_thin_schedule -> forward (total tiles, waves of the grid, 0),
    backward (positions per sample, chunk, blocks per sample); (-1, -1, -1) where the pass has no such kernel"""
    out = (ctypes.c_int * 3)()
    _handle().m2d_debug_thin_schedule(which, B, L, ks, stride, pad, out)
    return tuple(out)


def out_len(L, ks, stride, pad):
    return (L + 2 * pad - ks) // stride + 1


# ---- dense forwards: (name, B, L, ks, stride, pad, Lout, tiles, r)
K25_FWD_CASES = [
    ("two-tiles", 15, 51200, 25, 4, 11, 12800, 6000, 2),       # exit after the first tile / at t2
    ("three-tiles", 25, 51200, 25, 4, 11, 12800, 10000, 3),    # exit at the t3 test
    ("loop-back", 33, 51200, 25, 4, 11, 12800, 13200, 4),      # tile = t3, second trip
    ("row-tail-16B", 33, 51216, 25, 4, 11, 12804, 13233, 4),   # 4-position last tile of 16-byte rows
    ("rows-8B", 350, 3200, 25, 4, 0, 794, 8750, 3),            # valign == 2 on every tile
    ("rows-4B", 350, 3204, 25, 4, 0, 795, 8750, 3),            # scalar path
]
LONG_FWD_CASES = [
    ("k250-two-tiles", 100, 51200, 250, 50, 124, 1024, 3200, 2),
    ("k250-three-tiles", 140, 51200, 250, 50, 124, 1024, 4480, 3),
    ("k160-two-tiles", 200, 3200, 160, 4, 79, 800, 5000, 2),
    ("k160-three-tiles", 330, 3200, 160, 4, 79, 800, 8250, 3),
]
# ---- window views (conv1d_fwd_windows): (name, which, B, T, hop, window, ks, stride, pad, tiles, r)
WINDOW_FWD_CASES = [
    ("k25-windows", K25_FWD, 5, 120, 640, 3200, 25, 4, 0, 15000, 4),
    ("k250-windows", LONG_FWD, 18, 120, 640, 3200, 250, 50, 124, 4320, 3),
    ("k160-windows", LONG_FWD, 3, 120, 640, 3200, 160, 4, 79, 9000, 3),
]
# ---- k25 backward: (name, B, L, pad, Lout, chunk, blocks per sample) - the same chunk and blocks in backward-weight
# (over Lout positions) and backward-data (over nq = (L - 1 + pad) / 4 + 1 positions)
BWD_CASES = [
    ("chunk-1536", 40, 76800, 11, 19200, 1536, 13),
    ("chunk-1280", 64, 38400, 11, 9600, 1280, 8),
    ("odd-rows", 700, 3204, 0, 795, 1280, 1),    # chunk > Lout: one partial block, scalar loads
]
# chunk-1536 through conv1d_bwd_weight_windows: (B, T) tracks x windows with B * T = 40, window 76 800, hop 640
BWD_WINDOW = (5, 8, 640)
