// Baseline JPEG encoder for the stick-figure frames (MJPG payloads of visualize.AviWriter), defined in integers so that
// a numpy statement of the rule (tests/jpeg_rule.py) matches it byte for byte. DESIGN.md section 11.6.
//
// Stream: JFIF, 8 bits, 3 components at 1 x 1, one interleaved scan, the standard's typical Huffman tables, a restart
// interval of one MCU row: every row of 8 x 8 blocks starts with DC predictors 0, ends on a byte boundary and is
// followed by RSTm (EOI after the last), so rows are coded independently of each other.
//
// Four stages (five launches) on the caller's stream, no host synchronisation, no atomics on global memory:
//   1. transform: one lane per block. 8 rows of 24 bytes (dword loads where the row's 4-byte aligned window lies
//      inside the input, byte loads with edge replication otherwise), colour transform, 8 x 8 DCT, quantisation; the int16
//      zigzag coefficients of the three components go to the workspace. A block of one colour (almost every block of a
//      stick-figure frame) skips the DCT: its only non-zero coefficient is the DC, from the same two rounding steps.
//   2. measure: one workgroup per (frame, MCU row), one lane per block (64 threads for rows of up to 64 blocks, 256
//      for up to 512). Bit lengths of the row's blocks (kept for stage 4), exclusive scan in LDS, the row's bits
//      assembled in LDS (atomic OR of words: order-independent), 0xFF bytes counted -> bytes of the row.
//   3. scans: row offsets inside each frame (LDS scan per frame), then the frames' offsets (one workgroup walks the
//      frames 256 at a time with a carry) -> offsets[0..n] as int64.
//   4. write: stage 2's assembly again, now storing header, stuffed bytes and markers at their offsets - unless
//      offsets[n] exceeds the capacity, in which case nothing is written and the offsets report the need.
#include "m2d_common.h"

namespace {

constexpr int JP_HDR = 629;            // bytes before the entropy data
constexpr int JP_THREADS = 256;
constexpr int JP_NARROW = 64;          // threads of a coding workgroup when a row has at most 64 blocks (width <= 512)
constexpr int JP_CHUNK_WORDS = 16;     // LDS bit buffer: 64 bytes of a row's stream per thread at a time
constexpr int JP_OFF_Q0 = 25, JP_OFF_Q1 = 94, JP_OFF_SIZE = 163, JP_OFF_DRI = 613;

struct JpQuant {
  unsigned char q[2][64];  // luminance, chrominance; natural (row-major) order
};

constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the JPEG standard's typical Huffman tables (Annex K.3): code counts per length 1..16, then the symbols
constexpr unsigned char kBitsDcL[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char kBitsDcC[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char kValsDc[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char kBitsAcL[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr unsigned char kValsAcL[162] = {
    1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161,
    8,   35,  66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,
    39,  40,  41,  42,  52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,
    87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
    134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
    178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214,
    215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249,
    250};
constexpr unsigned char kBitsAcC[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr unsigned char kValsAcC[162] = {
    0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,
    145, 161, 177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,
    26,  38,  39,  40,  41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,
    86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
    132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168,
    169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
    213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249,
    250};

// symbol -> code | length << 16 for the tables DC luminance, AC luminance, DC chrominance, AC chrominance
struct JpHuff {
  unsigned e[4][256];
};
struct JpHeader {
  unsigned char b[JP_HDR];
};
struct JpZigzag {
  unsigned char z[64];
};

constexpr void jp_assign(unsigned (&e)[256], const unsigned char (&bits)[16], const unsigned char* vals) {
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i) e[vals[k++]] = code++ | ((unsigned)len << 16);
    code <<= 1;
  }
}

constexpr JpHuff jp_make_huff() {
  JpHuff h{};
  jp_assign(h.e[0], kBitsDcL, kValsDc);
  jp_assign(h.e[1], kBitsAcL, kValsAcL);
  jp_assign(h.e[2], kBitsDcC, kValsDc);
  jp_assign(h.e[3], kBitsAcC, kValsAcC);
  return h;
}

constexpr void jp_seg(JpHeader& h, int& n, int marker, int body) {
  h.b[n++] = 0xFF, h.b[n++] = (unsigned char)marker, h.b[n++] = (unsigned char)((body + 2) >> 8),
  h.b[n++] = (unsigned char)((body + 2) & 255);
}

constexpr void jp_dht(JpHeader& h, int& n, int id, const unsigned char (&bits)[16], const unsigned char* vals, int nv) {
  jp_seg(h, n, 0xC4, 17 + nv);
  h.b[n++] = (unsigned char)id;
  for (int i = 0; i < 16; ++i) h.b[n++] = bits[i];
  for (int i = 0; i < nv; ++i) h.b[n++] = vals[i];
}

// the header with zeros where the quantisation tables, the frame size and the restart interval go
constexpr JpHeader jp_make_header() {
  JpHeader h{};
  int n = 0;
  h.b[n++] = 0xFF, h.b[n++] = 0xD8;
  jp_seg(h, n, 0xE0, 14);
  const unsigned char app0[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (int i = 0; i < 14; ++i) h.b[n++] = app0[i];
  for (int t = 0; t < 2; ++t) {
    jp_seg(h, n, 0xDB, 65);
    h.b[n++] = (unsigned char)t;
    n += 64;
  }
  jp_seg(h, n, 0xC0, 15);
  const unsigned char sof[15] = {8, 0, 0, 0, 0, 3, 1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1};
  for (int i = 0; i < 15; ++i) h.b[n++] = sof[i];
  jp_dht(h, n, 0x00, kBitsDcL, kValsDc, 12);
  jp_dht(h, n, 0x10, kBitsAcL, kValsAcL, 162);
  jp_dht(h, n, 0x01, kBitsDcC, kValsDc, 12);
  jp_dht(h, n, 0x11, kBitsAcC, kValsAcC, 162);
  jp_seg(h, n, 0xDD, 2);
  n += 2;
  jp_seg(h, n, 0xDA, 10);
  const unsigned char sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
  for (int i = 0; i < 10; ++i) h.b[n++] = sos[i];
  if (n != JP_HDR) h.b[JP_HDR + n] = 0;  // not a constant expression: the build fails if the layout drifts
  return h;
}

constexpr JpZigzag jp_make_zigzag() {
  JpZigzag z{};
  for (int i = 0; i < 64; ++i) z.z[i] = kZigzag[i];
  return z;
}

__constant__ JpHuff kJpHuff = jp_make_huff();
__constant__ JpHeader kJpHeader = jp_make_header();
__constant__ JpZigzag kJpZigzag = jp_make_zigzag();

constexpr int jp_zz(int k) {
  constexpr unsigned char z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k];
}

// ---- stage 1: colour, DCT, quantisation ------------------------------------------------------------------------------

// o[u] = sum_x C[u][x] p[x] for C[u][x] = rint(2^14 * 0.5 * c(u) * cos((2x + 1) u pi / 16)): the rows of C are
// symmetric (even u) or antisymmetric (odd u), so the sums are formed from p[x] +- p[7 - x]; integer arithmetic, the
// same value as the plain sum
__device__ __forceinline__ void jp_dct8(int p0, int p1, int p2, int p3, int p4, int p5, int p6, int p7, int (&o)[8]) {
  const int s0 = p0 + p7, s1 = p1 + p6, s2 = p2 + p5, s3 = p3 + p4;
  const int d0 = p0 - p7, d1 = p1 - p6, d2 = p2 - p5, d3 = p3 - p4;
  o[0] = 5793 * (s0 + s1 + s2 + s3);
  o[4] = 5793 * (s0 - s1 - s2 + s3);
  o[2] = 7568 * (s0 - s3) + 3135 * (s1 - s2);
  o[6] = 3135 * (s0 - s3) - 7568 * (s1 - s2);
  o[1] = 8035 * d0 + 6811 * d1 + 4551 * d2 + 1598 * d3;
  o[3] = 6811 * d0 - 1598 * d1 - 8035 * d2 - 4551 * d3;
  o[5] = 4551 * d0 - 8035 * d1 + 1598 * d2 + 6811 * d3;
  o[7] = 1598 * d0 - 4551 * d1 + 6811 * d2 - 8035 * d3;
}

template <int COMP>
__device__ __forceinline__ int jp_colour(int r, int g, int b) {
  if (COMP == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (COMP == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// k = sign(c) (|c| + Q / 2) / Q; AC values are clamped to category 10
template <bool AC>
__device__ __forceinline__ int jp_quant(int c, unsigned q) {
  const unsigned a = (unsigned)(c < 0 ? -c : c);
  unsigned k = (a + (q >> 1)) / q;
  if (AC) k = min(k, 1023u);
  return c < 0 ? -(int)k : (int)k;
}

__device__ __forceinline__ unsigned jp_byte(const unsigned (&d)[48], int y, int j) {
  return (d[y * 6 + (j >> 2)] >> (8 * (j & 3))) & 255u;
}

// one component of one block: d holds the block's 8 rows of 24 RGB bytes; dst its 64 int16 zigzag coefficients
template <int COMP>
__device__ __forceinline__ void jp_component(const unsigned (&d)[48], bool flat, const JpQuant& qt, uint4* dst) {
  const unsigned char* q = qt.q[COMP ? 1 : 0];
  unsigned w[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = 0;
  if (flat) {
    const int p = jp_colour<COMP>((int)jp_byte(d, 0, 0), (int)jp_byte(d, 0, 1), (int)jp_byte(d, 0, 2)) - 128;
    const int t = (8 * 5793 * p + (1 << 10)) >> 11;
    const int c = (8 * 5793 * t + (1 << 16)) >> 17;
    w[0] = (unsigned)jp_quant<false>(c, q[0]) & 0xFFFFu;
  } else {
    int t[64];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      int p[8], o[8];
#pragma unroll
      for (int x = 0; x < 8; ++x)
        p[x] = jp_colour<COMP>((int)jp_byte(d, y, 3 * x), (int)jp_byte(d, y, 3 * x + 1), (int)jp_byte(d, y, 3 * x + 2)) - 128;
      jp_dct8(p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], o);
#pragma unroll
      for (int u = 0; u < 8; ++u) t[y * 8 + u] = (o[u] + (1 << 10)) >> 11;
    }
    int c[64];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int o[8];
      jp_dct8(t[u], t[8 + u], t[16 + u], t[24 + u], t[32 + u], t[40 + u], t[48 + u], t[56 + u], o);
#pragma unroll
      for (int v = 0; v < 8; ++v) c[v * 8 + u] = (o[v] + (1 << 16)) >> 17;
    }
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const int z = jp_zz(k);
      const int v = k == 0 ? jp_quant<false>(c[z], q[z]) : jp_quant<true>(c[z], q[z]);
      w[k >> 1] |= ((unsigned)v & 0xFFFFu) << (16 * (k & 1));
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) dst[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
}

__global__ void __launch_bounds__(JP_THREADS) m2d_jpeg_transform_kernel(const unsigned char* __restrict__ frames,
                                                                        long long n_blocks, long long n_frames, int H, int W,
                                                                        int nbx, int nby, JpQuant qt,
                                                                        short* __restrict__ coef) {
  const long long g = (long long)blockIdx.x * JP_THREADS + threadIdx.x;
  if (g >= n_blocks) return;
  const int bx = (int)(g % nbx);
  const long long r = g / nbx;
  const int by = (int)(r % nby);
  const long long f = r / nby;
  const size_t frame_bytes = (size_t)H * W * 3;
  const unsigned char* fb = frames + (size_t)f * frame_bytes;
  const unsigned char* lo = frames;
  const unsigned char* hi = frames + (size_t)n_frames * frame_bytes;
  const bool full = bx * 8 + 8 <= W && by * 8 + 8 <= H;

  unsigned d[48];
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const int yy = min(by * 8 + y, H - 1);
    const unsigned char* row = fb + (size_t)yy * W * 3;
    const unsigned char* p = row + bx * 24;
    const unsigned m = (unsigned)((uintptr_t)p & 3);
    const unsigned char* a = p - m;  // the row's 24 bytes lie inside the 28 bytes from this 4-byte boundary
    if (full && a >= lo && a + 28 <= hi) {
      const unsigned* s = reinterpret_cast<const unsigned*>(a);
      unsigned v[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) v[i] = s[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) d[y * 6 + i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], m);
    } else {  // edge blocks repeat the last column and row; the first and last rows of the input stay inside it
#pragma unroll
      for (int i = 0; i < 6; ++i) d[y * 6 + i] = 0;
#pragma unroll
      for (int x = 0; x < 8; ++x) {
        const unsigned char* px = row + 3 * min(bx * 8 + x, W - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int j = 3 * x + c;
          d[y * 6 + (j >> 2)] |= (unsigned)px[c] << (8 * (j & 3));
        }
      }
    }
  }

  // one colour: every row is the 12-byte pattern of its first pixel
  const unsigned cr = d[0] & 255u, cg = (d[0] >> 8) & 255u, cb = (d[0] >> 16) & 255u;
  const unsigned e0 = cr | (cg << 8) | (cb << 16) | (cr << 24);
  const unsigned e1 = cg | (cb << 8) | (cr << 16) | (cg << 24);
  const unsigned e2 = cb | (cr << 8) | (cg << 16) | (cb << 24);
  unsigned diff = 0;
#pragma unroll
  for (int y = 0; y < 8; ++y)
    diff |= (d[y * 6] ^ e0) | (d[y * 6 + 1] ^ e1) | (d[y * 6 + 2] ^ e2) | (d[y * 6 + 3] ^ e0) | (d[y * 6 + 4] ^ e1) |
            (d[y * 6 + 5] ^ e2);
  const bool flat = diff == 0;

  uint4* dst = reinterpret_cast<uint4*>(coef + g * 192);
  jp_component<0>(d, flat, qt, dst);
  jp_component<1>(d, flat, qt, dst + 8);
  jp_component<2>(d, flat, qt, dst + 16);
}

// ---- stages 2 and 4: entropy coding of one MCU row --------------------------------------------------------------------

// exclusive scan of v over the workgroup's THREADS threads; `total` is the sum. s: THREADS entries of LDS.
template <int THREADS, typename T>
__device__ __forceinline__ T jp_scan(T v, T* s, T& total) {
  const int t = threadIdx.x;
  s[t] = v;
  __syncthreads();
  for (int off = 1; off < THREADS; off <<= 1) {
    const T x = t >= off ? s[t - off] : (T)0;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
  total = s[THREADS - 1];
  const T r = s[t] - v;
  __syncthreads();
  return r;
}

// `len` (1..27) bits at bit `pos` of the row's stream into the words [w0, w0 + nw) held in buf; bits outside are dropped
__device__ __forceinline__ void jp_put(unsigned* buf, unsigned w0, unsigned nw, unsigned pos, unsigned bits, int len) {
  const unsigned o = pos & 31u, r = (pos >> 5) - w0;  // r wraps below w0: out of range, except r + 1 == 0
  const unsigned long long v = (unsigned long long)bits << (64 - (int)o - len);
  const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
  if (hi && r < nw) atomicOr(buf + r, hi);
  if (lo && r + 1u < nw) atomicOr(buf + r + 1u, lo);
}

// the code of one block (three components) from bit `pos` on -> its length in bits. cf: the block's 192 coefficients;
// first: the row's first block (DC predictors 0, otherwise the block before). EMIT false: the length only.
template <bool EMIT>
__device__ __forceinline__ unsigned jp_block(const short* __restrict__ cf, bool first, const unsigned* huff, unsigned pos,
                                             unsigned* buf, unsigned w0, unsigned nw) {
  const unsigned start = pos;
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const uint4* q = reinterpret_cast<const uint4*>(cf + c * 64);
    const unsigned* hdc = huff + (c ? 512 : 0);
    const unsigned* hac = hdc + 256;
    const int pred = first ? 0 : (int)cf[c * 64 - 192];
    uint4 all[8];  // the component's 64 coefficients in one round of loads: the walk below waits for memory once
#pragma unroll
    for (int i = 0; i < 8; ++i) all[i] = q[i];
    {
      const int dc = (int)(short)(all[0].x & 0xFFFFu) - pred;
      const unsigned a = (unsigned)(dc < 0 ? -dc : dc);
      const int cat = a ? 32 - __builtin_clz(a) : 0;
      const unsigned h = hdc[cat];
      const int n = (int)(h >> 16) + cat;
      if (EMIT) jp_put(buf, w0, nw, pos, ((h & 0xFFFFu) << cat) | ((unsigned)(dc < 0 ? dc - 1 : dc) & ((1u << cat) - 1u)), n);
      pos += n;
      all[0].x &= 0xFFFF0000u;
    }
    int run = -1;  // the DC slot is cleared above and counts as one zero
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint4 v = all[i];
      if ((v.x | v.y | v.z | v.w) == 0u) {
        run += 8;
        continue;
      }
      const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int val = (int)(short)((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
        if (val == 0) {
          ++run;
          continue;
        }
        while (run > 15) {  // ZRL
          const unsigned h = hac[0xF0];
          if (EMIT) jp_put(buf, w0, nw, pos, h & 0xFFFFu, (int)(h >> 16));
          pos += h >> 16;
          run -= 16;
        }
        const unsigned a = (unsigned)(val < 0 ? -val : val);
        const int cat = 32 - __builtin_clz(a);
        const unsigned h = hac[(run << 4) | cat];
        const int n = (int)(h >> 16) + cat;
        if (EMIT) jp_put(buf, w0, nw, pos, ((h & 0xFFFFu) << cat) | ((unsigned)(val < 0 ? val - 1 : val) & ((1u << cat) - 1u)), n);
        pos += n;
        run = 0;
      }
    }
    if (run > 0) {  // EOB, unless coefficient 63 is non-zero
      const unsigned h = hac[0];
      if (EMIT) jp_put(buf, w0, nw, pos, h & 0xFFFFu, (int)(h >> 16));
      pos += h >> 16;
    }
  }
  return pos - start;
}

__device__ __forceinline__ unsigned jp_stream_byte(const unsigned* buf, unsigned k) {
  return (buf[k >> 2] >> (24u - 8u * (k & 3u))) & 255u;
}

// WRITE false (stage 2): block_bits[block] = bits of the block's code; row_info[row] = bytes of the row's entropy data,
// stuffing and marker included. WRITE true (stage 4): block_bits is read; row_info[row] is the row's offset behind its
// frame's header; the bytes are stored. THREADS: JP_NARROW or JP_THREADS, at least half the blocks of a row.
template <bool WRITE, int THREADS>
__global__ void __launch_bounds__(THREADS) m2d_jpeg_code_kernel(const short* __restrict__ coef, int nbx, int nby,
                                                                long long n_frames, int H, int W, JpQuant qt,
                                                                unsigned short* __restrict__ block_bits,
                                                                int* __restrict__ row_info,
                                                                const long long* __restrict__ offsets,
                                                                unsigned char* __restrict__ out, long long capacity) {
  constexpr unsigned CHUNK = THREADS * JP_CHUNK_WORDS;
  __shared__ unsigned s_huff[1024];
  __shared__ unsigned s_buf[CHUNK];
  __shared__ unsigned s_scan[THREADS];
  const int t = threadIdx.x;
  const long long row = blockIdx.x;  // frame * nby + by
  const long long f = row / nby;
  const int by = (int)(row - f * nby);
  unsigned char* dst = nullptr;
  if (WRITE) {
    if (offsets[n_frames] > capacity) return;  // the streams do not fit: nothing is written, the offsets say how much
    dst = out + offsets[f];
    if (by == 0) {
      for (int i = t; i < JP_HDR; i += THREADS) {
        unsigned b = kJpHeader.b[i];
        if (i >= JP_OFF_Q0 && i < JP_OFF_Q0 + 64) b = qt.q[0][kJpZigzag.z[i - JP_OFF_Q0]];
        if (i >= JP_OFF_Q1 && i < JP_OFF_Q1 + 64) b = qt.q[1][kJpZigzag.z[i - JP_OFF_Q1]];
        if (i == JP_OFF_SIZE) b = (unsigned)H >> 8;
        if (i == JP_OFF_SIZE + 1) b = (unsigned)H & 255u;
        if (i == JP_OFF_SIZE + 2) b = (unsigned)W >> 8;
        if (i == JP_OFF_SIZE + 3) b = (unsigned)W & 255u;
        if (i == JP_OFF_DRI) b = (unsigned)nbx >> 8;
        if (i == JP_OFF_DRI + 1) b = (unsigned)nbx & 255u;
        dst[i] = (unsigned char)b;
      }
    }
    dst += JP_HDR + row_info[row];
  }
  for (int i = t; i < 1024; i += THREADS) s_huff[i] = kJpHuff.e[i >> 8][i & 255];
  __syncthreads();

  // each thread owns `per` (1 or 2) consecutive blocks of the row
  const int per = (nbx + THREADS - 1) / THREADS;
  const short* cf = coef + row * (long long)nbx * 192;
  unsigned short* bits = block_bits + row * (long long)nbx;
  const int b0 = t * per;
  unsigned len[2] = {0u, 0u};
  for (int i = 0; i < per; ++i) {
    if (b0 + i >= nbx) break;
    if (WRITE) {
      len[i] = bits[b0 + i];
    } else {  // at most 3 * (11 + 11 + 63 * 26) bits: fits 16
      len[i] = jp_block<false>(cf + (b0 + i) * 192, b0 + i == 0, s_huff, 0u, nullptr, 0u, 0u);
      bits[b0 + i] = (unsigned short)len[i];
    }
  }
  unsigned total_bits;
  unsigned bit0[2];
  bit0[0] = jp_scan<THREADS, unsigned>(len[0] + len[1], s_scan, total_bits);
  bit0[1] = bit0[0] + len[0];
  const unsigned pad = (0u - total_bits) & 7u;
  const unsigned n_bytes = (total_bits + pad) >> 3;

  unsigned stuffed = 0;  // 0xFF bytes before the current chunk (uniform)
  for (unsigned w0 = 0; 4u * w0 < n_bytes; w0 += CHUNK) {
    const unsigned nb = min(4u * CHUNK, n_bytes - 4u * w0), nw = (nb + 3u) >> 2;
    for (unsigned i = t; i < nw; i += THREADS) s_buf[i] = 0u;
    __syncthreads();
    const unsigned lo = 32u * w0, hi = lo + 32u * nw;
    for (int i = 0; i < per; ++i)
      if (len[i] && bit0[i] < hi && bit0[i] + len[i] > lo)
        jp_block<true>(cf + (b0 + i) * 192, b0 + i == 0, s_huff, bit0[i], s_buf, w0, nw);
    if (t == 0 && pad) jp_put(s_buf, w0, nw, total_bits, (1u << pad) - 1u, (int)pad);
    __syncthreads();
    const unsigned span = (nb + THREADS - 1) / THREADS;
    const unsigned k0 = min(t * span, nb), k1 = min(k0 + span, nb);
    unsigned ff = 0;
    for (unsigned k = k0; k < k1; ++k) ff += jp_stream_byte(s_buf, k) == 255u;
    unsigned ff_total;
    const unsigned before = jp_scan<THREADS, unsigned>(ff, s_scan, ff_total);  // ends on a barrier: s_buf may be cleared again
    if (WRITE) {
      unsigned char* p = dst + 4u * w0 + stuffed + k0 + before;
      for (unsigned k = k0; k < k1; ++k) {
        const unsigned b = jp_stream_byte(s_buf, k);
        *p++ = (unsigned char)b;
        if (b == 255u) *p++ = 0;
      }
    }
    stuffed += ff_total;
    __syncthreads();
  }
  if (t == 0) {
    if (WRITE) {
      dst[n_bytes + stuffed] = 0xFF;
      dst[n_bytes + stuffed + 1] = by == nby - 1 ? 0xD9 : (unsigned char)(0xD0 + (by & 7));
    } else {
      row_info[row] = (int)(n_bytes + stuffed + 2u);
    }
  }
}

// ---- stage 3: offsets -------------------------------------------------------------------------------------------------

// one workgroup per frame: row_info (bytes per row) -> exclusive scan in place; frame_bytes[f] = header + rows
__global__ void __launch_bounds__(JP_THREADS) m2d_jpeg_rows_kernel(int* __restrict__ row_info, int nby,
                                                                   long long* __restrict__ frame_bytes) {
  __shared__ unsigned s_scan[JP_THREADS];
  const int t = threadIdx.x;
  int* rows = row_info + (long long)blockIdx.x * nby;
  const int per = (nby + JP_THREADS - 1) / JP_THREADS;  // 1 or 2
  const int r0 = t * per;
  unsigned v[2] = {0u, 0u};
  for (int i = 0; i < per; ++i)
    if (r0 + i < nby) v[i] = (unsigned)rows[r0 + i];
  unsigned total;
  const unsigned e = jp_scan<JP_THREADS, unsigned>(v[0] + v[1], s_scan, total);
  if (r0 < nby) rows[r0] = (int)e;
  if (per > 1 && r0 + 1 < nby) rows[r0 + 1] = (int)(e + v[0]);
  if (t == 0) frame_bytes[blockIdx.x] = (long long)JP_HDR + total;
}

// one workgroup: offsets[0..n] = exclusive scan of frame_bytes, JP_THREADS frames at a time with a carry
__global__ void __launch_bounds__(JP_THREADS) m2d_jpeg_frames_kernel(const long long* __restrict__ frame_bytes,
                                                                     long long n_frames, long long* __restrict__ offsets) {
  __shared__ unsigned long long s_scan[JP_THREADS];
  const int t = threadIdx.x;
  unsigned long long carry = 0;
  for (long long base = 0; base < n_frames; base += JP_THREADS) {
    const long long i = base + t;
    const unsigned long long v = i < n_frames ? (unsigned long long)frame_bytes[i] : 0ull;
    unsigned long long total;
    const unsigned long long e = jp_scan<JP_THREADS, unsigned long long>(v, s_scan, total);
    if (i < n_frames) offsets[i] = (long long)(carry + e);
    carry += total;
  }
  if (t == 0) offsets[n_frames] = (long long)carry;
}

struct JpLayout {
  int nbx, nby;
  long long blocks, rows;
  size_t coef_bytes, bits_bytes, row_bytes, total;
};

JpLayout jp_layout(long n, int H, int W) {
  JpLayout l;
  l.nbx = (W + 7) / 8, l.nby = (H + 7) / 8;
  l.rows = (long long)n * l.nby;
  l.blocks = l.rows * l.nbx;
  l.coef_bytes = (size_t)l.blocks * 384;                            // 3 x 64 int16 per block: a multiple of 16
  l.bits_bytes = (((size_t)l.blocks * 2) + 15) & ~(size_t)15;       // uint16 per block: the bits of its code
  l.row_bytes = (((size_t)l.rows * 4) + 15) & ~(size_t)15;          // int32 per MCU row
  l.total = l.coef_bytes + l.bits_bytes + l.row_bytes + (size_t)n * 8;   // + int64 per frame
  return l;
}

}  // namespace

extern "C" {

size_t m2d_jpeg_workspace_bytes(long n_frames, int height, int width) {
  if (n_frames <= 0 || height < 1 || height > 4096 || width < 1 || width > 4096) return 0;
  return jp_layout(n_frames, height, width).total;
}

int m2d_jpeg_encode(const unsigned char* frames, long n_frames, int height, int width, const unsigned char* qtabs,
                    unsigned char* out, long long capacity, long long* offsets, void* workspace, size_t workspace_bytes,
                    void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_frames < 0 || height < 1 || height > 4096 || width < 1 || width > 4096 || capacity < 0)
    M2D_FAIL(M2D_ERR_ARG, "m2d_jpeg_encode: bad arguments (n_frames %ld, %d x %d, capacity %lld)", n_frames, height,
             width, capacity);
  if (n_frames == 0) return M2D_OK;
  if (!frames || !qtabs || !offsets || !workspace || (!out && capacity > 0))
    M2D_FAIL(M2D_ERR_ARG, "m2d_jpeg_encode: null pointer");
  JpQuant qt;
  for (int i = 0; i < 128; ++i) {
    if (qtabs[i] == 0) M2D_FAIL(M2D_ERR_ARG, "m2d_jpeg_encode: quantisation entry %d is zero", i);
    qt.q[i >> 6][i & 63] = qtabs[i];
  }
  const JpLayout l = jp_layout(n_frames, height, width);
  if (((uintptr_t)workspace & 15) != 0) M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_jpeg_encode: the workspace must be 16-byte aligned");
  if (workspace_bytes < l.total)
    M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_jpeg_encode: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
  const long long tgrid = m2d_ceil_div64(l.blocks, JP_THREADS);
  if (tgrid > 0x7fffffffLL || l.rows > 0x7fffffffLL)
    M2D_FAIL(M2D_ERR_RANGE, "m2d_jpeg_encode: %ld frames are too many for one launch", n_frames);
  short* coef = (short*)workspace;
  unsigned short* block_bits = (unsigned short*)((char*)workspace + l.coef_bytes);
  int* row_info = (int*)((char*)workspace + l.coef_bytes + l.bits_bytes);
  long long* frame_bytes = (long long*)((char*)workspace + l.coef_bytes + l.bits_bytes + l.row_bytes);
  const bool narrow = l.nbx <= JP_NARROW;
  const double raw = (double)n_frames * height * width * 3.0;
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, raw + 4.0 * (double)l.coef_bytes, "jpeg_encode", height, width);
  hipLaunchKernelGGL(m2d_jpeg_transform_kernel, dim3((unsigned)tgrid), dim3(JP_THREADS), 0, stream, frames, l.blocks,
                     (long long)n_frames, height, width, l.nbx, l.nby, qt, coef);
  M2D_CHECK_LAUNCH("m2d_jpeg_encode (transform)");
  if (narrow)
    hipLaunchKernelGGL((m2d_jpeg_code_kernel<false, JP_NARROW>), dim3((unsigned)l.rows), dim3(JP_NARROW), 0, stream, coef,
                       l.nbx, l.nby, (long long)n_frames, height, width, qt, block_bits, row_info,
                       (const long long*)nullptr, (unsigned char*)nullptr, 0LL);
  else
    hipLaunchKernelGGL((m2d_jpeg_code_kernel<false, JP_THREADS>), dim3((unsigned)l.rows), dim3(JP_THREADS), 0, stream,
                       coef, l.nbx, l.nby, (long long)n_frames, height, width, qt, block_bits, row_info,
                       (const long long*)nullptr, (unsigned char*)nullptr, 0LL);
  M2D_CHECK_LAUNCH("m2d_jpeg_encode (measure)");
  hipLaunchKernelGGL(m2d_jpeg_rows_kernel, dim3((unsigned)n_frames), dim3(JP_THREADS), 0, stream, row_info, l.nby,
                     frame_bytes);
  M2D_CHECK_LAUNCH("m2d_jpeg_encode (row offsets)");
  hipLaunchKernelGGL(m2d_jpeg_frames_kernel, dim3(1), dim3(JP_THREADS), 0, stream, frame_bytes, (long long)n_frames,
                     offsets);
  M2D_CHECK_LAUNCH("m2d_jpeg_encode (frame offsets)");
  if (narrow)
    hipLaunchKernelGGL((m2d_jpeg_code_kernel<true, JP_NARROW>), dim3((unsigned)l.rows), dim3(JP_NARROW), 0, stream, coef,
                       l.nbx, l.nby, (long long)n_frames, height, width, qt, block_bits, row_info, offsets, out,
                       capacity);
  else
    hipLaunchKernelGGL((m2d_jpeg_code_kernel<true, JP_THREADS>), dim3((unsigned)l.rows), dim3(JP_THREADS), 0, stream,
                       coef, l.nbx, l.nby, (long long)n_frames, height, width, qt, block_bits, row_info, offsets, out,
                       capacity);
  M2D_CHECK_LAUNCH("m2d_jpeg_encode (write)");
  return M2D_OK;
}

}  // extern "C"
