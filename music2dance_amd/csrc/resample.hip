// Polyphase FIR resampling of audio rows by a rational factor up / down (m2d_resample_poly, include/m2d.h): what the
// reference's change_rate.py leaves to `sox`, and what phase3/generate.py needs to take a stream at the file's own rate.
//
// Output n of a row is defined per ABSOLUTE index, like the frames of m2d_randn_frames:
//   t = n down + half, half = (ntaps - 1) / 2, y[n] = sum over m with 0 <= t - m up < ntaps of taps[t - m up] X[m].
// With phi = t mod up and q = t / up the taps of one output are taps[phi + j up] and its samples X[q - j],
// j = 0 .. P_phi - 1, P_phi = ceil((ntaps - phi) / up): one fp32 accumulator, fmaf in ascending j. Nothing else enters the
// value - not the call's first output, the declared window, the tile or the row count - so the chunks of a stream equal the
// whole-track call bit for bit.
//
// The work is cut into (tile of outputs, row) items; a workgroup stages the tap table once and then walks items
// blockIdx.x, blockIdx.x + gridDim.x, ... (as many workgroups as the device holds at once: re-staging 36 KB of taps per
// tile cost as much as the tile's arithmetic). LDS holds
//   * the tap table phase-major, tp[phi * S + j] = taps[phi + j up] for the min(up, ntaps) phases that have a tap;
//     S = P | 1 with P = ceil(ntaps / up): neighbouring lanes' phases advance by down mod up, an odd row stride keeps
//     their ds_read_b32 (32 banks per half wave) apart whenever that step is odd; slots past P_phi are never read;
//   * the tile's input span X[q_first - (P - 1) .. q_last], zeros outside the declared window [x0, x0 + nx).
// The host sizes the tile so that both fit: 44.1 -> 16 kHz at the default design is 36 KB of taps + 23 KB of samples
// for 2048 outputs (two workgroups of 16 waves per CU: the accumulation is one dependent chain of LDS reads and fmaf per
// lane, so it is the wave count that hides the LDS latency); a 16 383-tap filter or a huge `down` shrinks the tile
// instead of failing.
#include "m2d_common.h"

#include <limits.h>

#include <numeric>

#define M2D_RS_THREADS 1024
#define M2D_RS_MAX_TAPS 16384
#define M2D_RS_LDS_MAX (160 * 1024)
#define M2D_RS_LDS_SOFT (64 * 1024)

namespace {

__global__ void __launch_bounds__(M2D_RS_THREADS) m2d_resample_poly_kernel(
    const float* __restrict__ x, long long x0, int nx, long long ldx, const float* __restrict__ taps, int ntaps, int up,
    int down, float* __restrict__ y, long long n0, int ny, long long ldy, int tile, int tiles, int work, int P, int S,
    int rows, int narrow) {
  extern __shared__ float sh[];
  float* tp = sh;                       // [rows][S]
  float* xs = sh + (size_t)rows * S;    // the tile's input span
  const long long half = (ntaps - 1) / 2;
  for (int k = threadIdx.x; k < ntaps; k += M2D_RS_THREADS) {
    const int j = k / up;
    tp[(size_t)(k - j * up) * S + j] = taps[k];
  }
  for (long long w = blockIdx.x; w < work; w += gridDim.x) {
    const int b = (int)(w / tiles);
    const int i0 = (int)(w - (long long)b * tiles) * tile;   // < ny
    const int cnt = min(tile, ny - i0);
    const long long tA = (n0 + i0) * (long long)down + half;
    const long long qA = tA / up;
    const long long rA = tA - qA * up;                // phase of the tile's first output
    const long long q_last = (rA + (long long)(cnt - 1) * down) / up;
    const long long span = q_last + P;                // host: fits the LDS behind the tap table
    const long long mlo = qA - (P - 1);               // absolute index of xs[0]
    const float* xrow = x + (long long)b * ldx;
    __syncthreads();                                  // the previous item's reads of xs are done
    for (long long s = threadIdx.x; s < span; s += M2D_RS_THREADS) {
      const long long idx = mlo + s - x0;
      xs[s] = (idx >= 0 && idx < nx) ? xrow[idx] : 0.f;
    }
    __syncthreads();                                  // (the first time: the tap table, too)

    float* yrow = y + (long long)b * ldy + i0;
    for (int i = threadIdx.x; i < cnt; i += M2D_RS_THREADS) {
      long long q, phi;
      if (narrow) {  // rA + i down < 2^31: one 32-bit division per output
        const unsigned l = (unsigned)rA + (unsigned)i * (unsigned)down;
        const unsigned qq = l / (unsigned)up;
        q = qq;
        phi = l - qq * (unsigned)up;
      } else {
        const long long l = rA + (long long)i * down;
        q = l / up;
        phi = l - q * up;
      }
      float acc = 0.f;
      if (phi < ntaps) {
        const int np = (int)((ntaps - phi + up - 1) / up);   // taps of this phase, 1 .. P
        const float* t = tp + (size_t)phi * S;
        const float* s = xs + (q + (P - 1));
        for (int j = 0; j < np; ++j) acc = fmaf(t[j], s[-j], acc);
      }
      yrow[i] = acc;
    }
  }
}

}  // namespace

extern "C" {

int m2d_resample_poly(const float* x, long long x0, int nx, long long ldx, const float* taps, int ntaps, int up,
                      int down, float* y, long long n0, int ny, long long ldy, int B, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (up <= 0 || down <= 0 || B <= 0 || nx < 0 || ny < 0)
    M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: up, down and B must be positive, nx and ny non-negative");
  if (x0 < 0 || n0 < 0) M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: x0 and n0 must be non-negative");
  if (ntaps <= 0 || ntaps % 2 == 0) M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: ntaps must be odd (got %d)", ntaps);
  if (ntaps > M2D_RS_MAX_TAPS)
    M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: at most %d taps (got %d)", M2D_RS_MAX_TAPS, ntaps);
  if (ldx < nx || ldy < ny) M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: ldx < nx or ldy < ny");
  if (std::gcd(up, down) != 1)
    M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: up / down = %d / %d is not reduced by its gcd", up, down);
  if (!taps || (!x && nx > 0) || (!y && ny > 0)) M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: null pointer");
  const long long half = (ntaps - 1) / 2;
  if (n0 > LLONG_MAX - ny || x0 > LLONG_MAX - nx || n0 + ny > (LLONG_MAX - half) / down)
    M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: n * down + half leaves 63 bits");
  if (ny == 0) return M2D_OK;

  const int P = (ntaps + up - 1) / up;
  const int S = P | 1;
  const int rows = up < ntaps ? up : ntaps;
  const long long tap_bytes = (long long)rows * S * 4;
  auto span_of = [&](int t) { return ((long long)(t - 1) * down + (up - 1)) / up + P; };
  int tile = 2048;
  while (tile > 1 && (tap_bytes + 4 * span_of(tile < ny ? tile : ny) > M2D_RS_LDS_MAX ||
                      (tile > 256 && tap_bytes + 4 * span_of(tile < ny ? tile : ny) > M2D_RS_LDS_SOFT)))
    tile >>= 1;
  const long long lds = tap_bytes + 4 * span_of(tile < ny ? tile : ny);
  if (lds > M2D_RS_LDS_MAX) M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: %lld bytes of LDS needed", lds);
  const int tiles = m2d_ceil_div(ny, tile);
  if ((long long)tiles * B > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_resample_poly: too many tiles");
  const int narrow = (long long)(tile - 1) * down + up < (1ll << 31);

  static bool attr_set = false;
  static int cus = 0;
  if (!attr_set) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      M2D_FAIL(M2D_ERR_HIP, "m2d_resample_poly: cannot read the device's CU count");
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&m2d_resample_poly_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, M2D_RS_LDS_MAX) != hipSuccess)
      M2D_FAIL(M2D_ERR_HIP, "m2d_resample_poly: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 2.0 * (double)B * ny * P,
                    4.0 * (double)B * ((double)ny + (double)ny * down / up) + (double)tiles * B * tap_bytes,
                    "resample_poly", up, down, ntaps);
  // resident workgroups: 2048 threads and 160 KB of LDS per CU
  const int per_cu = lds * 2 <= M2D_RS_LDS_MAX ? 2 : 1;
  const int work = tiles * B;
  const int grid = work < cus * per_cu ? work : cus * per_cu;
  hipLaunchKernelGGL(m2d_resample_poly_kernel, dim3((unsigned)grid), dim3(M2D_RS_THREADS), (size_t)lds, stream, x, x0,
                     nx, ldx, taps, ntaps, up, down, y, n0, ny, ldy, tile, tiles, work, P, S, rows, narrow);
  M2D_CHECK_LAUNCH("m2d_resample_poly");
  return M2D_OK;
}

}  // extern "C"
