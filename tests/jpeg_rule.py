"""The encoding rule of m2d_jpeg_encode stated in numpy and plain integers: the reference
that tests/test_jpeg_host.py checks against PIL and tests/test_gpu_jpeg.py compares the kernels with, byte for byte.
No floating point enters any value.

Format: baseline sequential JFIF, 8 bits, 3 components at 1 x 1 (4:4:4), one interleaved scan. Segments in the order
PIL writes them: SOI, APP0 (JFIF 1.1, density 1:1 without unit), DQT 0, DQT 1, SOF0, DHT DC0, DHT AC0, DHT DC1,
DHT AC1, DRI, SOS, entropy data, EOI.

Tables: the Huffman tables are the standard's typical ones (Annex K.3); the quantisation tables are Annex K.1 scaled
by quality q in [1, 100]: s = 5000 // q below 50, else 200 - 2 q; entry = clamp((base * s + 50) // 100, 1, 255).

Colour (R, G, B in 0..255, >> arithmetic):
    Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
    Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
    Cr = ( 32768 R - 27439 G -  5329 B + (128 << 16) + 32767) >> 16
All three lie in 0..255 without a clamp (the coefficient rows sum to 65536, 0 and 0).

Blocks: the frame is extended to multiples of 8 by repeating its last row and column; samples are shifted by -128.

DCT: C[u][x] = rint(2^14 * 0.5 * c(u) * cos((2x + 1) u pi / 16)), the 64 literals of DCT below.
    rows:    t[y][u] = (sum_x C[u][x] p[y][x] + 2^10) >> 11        |sum| <= 128 * 45990 < 2^23
    columns: c[v][u] = (sum_y C[v][y] t[y][u] + 2^16) >> 17        |sum| <= 2875 * 45990 < 2^28

Quantisation: k = sign(c) * ((|c| + Q // 2) // Q), Q the table entry. A DC value lies in [-1024, 1016] (a constant
block of -128 and of 127 through the two passes above, Q = 1), so a DC difference lies within +-2040 and fits
category 11. The exact DCT bounds an AC value by 128 * 8 * (5.126 / 8)^2 < 1023, but the bound is not proved for the
rounded passes, so AC values are clamped to [-1023, 1023], category 10: the clamp is part of the rule.

Entropy coding: DC as the difference from the previous block of the same component; AC as (run, size) symbols with
ZRL (0xF0) for runs above 15, EOB (0x00) unless coefficient 63 is non-zero; a value v of category n is followed by
its n low bits, v + 2^n - 1 for negative v. A zero byte follows every 0xFF data byte.

Restart intervals: DRI = one MCU row (ceil(width / 8) MCUs), always written. Every MCU row starts with the DC
predictors at 0, ends padded with 1-bits to a whole byte and - except the last - is followed by RSTm, m = row mod 8.
Rows are therefore independent of each other.

`encode(frame, quality)` -> (bytes, counters); counters: zrl, stuffed, no_eob (blocks of a component without EOB),
max_dc_cat, max_ac_cat, ac_symbols (AC symbols other than EOB)."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
          61, 54, 47, 55, 62, 63]
BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
               47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193,
            21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55,
            56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104,
            105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
            149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183,
            184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
            225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193,
              9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42,
              53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102,
              103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138,
              146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180,
              181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215,
              216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])
# (table class << 4 | id, spec) in the order the DHT segments are written
HUFFMAN = [(0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)]
DCT = np.array([[5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793],
                [8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035],
                [7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568],
                [6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811],
                [5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793],
                [4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551],
                [3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135],
                [1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598]], dtype=np.int64)


def quant_tables(quality):
    """-> (luma, chroma): two lists of 64 entries in natural (row-major) order"""
    q = int(quality)
    assert 1 <= q <= 100, quality
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple([min(max((b * s + 50) // 100, 1), 255) for b in base] for base in (BASE_LUMA, BASE_CHROMA))


def huffman_codes(spec):
    """(bits, values) of a DHT segment -> {symbol: (code, length)} (Annex C)"""
    bits, vals = spec
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def header(height, width, qtabs):
    """every byte before the entropy data"""
    def seg(marker, body):
        return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)
    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    for i, t in enumerate(qtabs):
        out += seg(0xDB, [i] + [int(t[ZIGZAG[k]]) for k in range(64)])
    out += seg(0xC0, [8, height >> 8, height & 255, width >> 8, width & 255, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])
    for tc_th, (bits, vals) in HUFFMAN:
        out += seg(0xC4, [tc_th] + bits + vals)
    mcus = (width + 7) // 8
    out += seg(0xDD, [mcus >> 8, mcus & 255])
    return out + seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])


def ycc(frame):
    """(H, W, 3) uint8 RGB -> (3, H, W) int64 Y, Cb, Cr in 0..255"""
    r, g, b = (frame[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr])


def coefficients(frame, qtabs):
    """(H, W, 3) uint8 -> (rows, cols, 3, 64) int64 quantised coefficients in zigzag order, AC clamped to +-1023"""
    H, W = frame.shape[:2]
    by, bx = (H + 7) // 8, (W + 7) // 8
    p = np.pad(ycc(frame), ((0, 0), (0, 8 * by - H), (0, 8 * bx - W)), mode="edge") - 128
    p = p.reshape(3, by, 8, bx, 8).transpose(1, 3, 0, 2, 4)               # (by, bx, comp, y, x)
    t = (np.einsum("ux,...yx->...yu", DCT, p) + (1 << 10)) >> 11
    c = (np.einsum("vy,...yu->...vu", DCT, t) + (1 << 16)) >> 17
    q = np.array([qtabs[0], qtabs[1], qtabs[1]], dtype=np.int64).reshape(3, 8, 8)
    k = np.sign(c) * ((np.abs(c) + q // 2) // q)
    k = k.reshape(by, bx, 3, 64)[..., ZIGZAG]
    k[..., 1:] = np.clip(k[..., 1:], -1023, 1023)
    return k


class _Bits:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code
        self.n += length

    def flush(self, counters):
        """pad with 1-bits to a whole byte, stuff a zero after every 0xFF -> bytes"""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        raw = self.acc.to_bytes(self.n // 8, "big") if self.n else b""
        counters["stuffed"] += raw.count(b"\xff")
        return raw.replace(b"\xff", b"\xff\x00")


def _value(bits, v, code, length, cat):
    bits.put((code << cat) | ((v if v >= 0 else v + (1 << cat) - 1) & ((1 << cat) - 1)), length + cat)


def encode(frame, quality=95, qtabs=None):
    """(H, W, 3) uint8 RGB -> (JPEG bytes, counters); `qtabs` (two lists of 64, natural order) overrides `quality`"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3, (frame.dtype, frame.shape)
    H, W = frame.shape[:2]
    assert 1 <= H <= 4096 and 1 <= W <= 4096
    qtabs = quant_tables(quality) if qtabs is None else qtabs
    dc = [huffman_codes(DC_LUMA), huffman_codes(DC_CHROMA), huffman_codes(DC_CHROMA)]
    ac = [huffman_codes(AC_LUMA), huffman_codes(AC_CHROMA), huffman_codes(AC_CHROMA)]
    coef = coefficients(frame, qtabs).tolist()
    cnt = dict(zrl=0, stuffed=0, no_eob=0, max_dc_cat=0, max_ac_cat=0, ac_symbols=0)
    out = [header(H, W, qtabs)]
    for row, blocks in enumerate(coef):
        bits, pred = _Bits(), [0, 0, 0]
        for block in blocks:
            for c in range(3):
                k = block[c]
                d, pred[c] = k[0] - pred[c], k[0]
                cat = abs(d).bit_length()
                assert cat <= 11
                cnt["max_dc_cat"] = max(cnt["max_dc_cat"], cat)
                _value(bits, d, *dc[c][cat], cat)
                run = 0
                if any(k[1:]):
                    for v in k[1:]:
                        if v == 0:
                            run += 1
                            continue
                        while run > 15:
                            bits.put(*ac[c][0xF0])
                            run -= 16
                            cnt["zrl"] += 1
                            cnt["ac_symbols"] += 1
                        cat = abs(v).bit_length()
                        cnt["max_ac_cat"] = max(cnt["max_ac_cat"], cat)
                        cnt["ac_symbols"] += 1
                        _value(bits, v, *ac[c][(run << 4) | cat], cat)
                        run = 0
                else:
                    run = 63
                if run:
                    bits.put(*ac[c][0x00])
                else:
                    cnt["no_eob"] += 1
        out.append(bits.flush(cnt))
        out.append(b"\xff\xd9" if row == len(coef) - 1 else bytes([0xFF, 0xD0 + (row & 7)]))
    return b"".join(out), cnt
