// The music-dance beat-alignment score (metrics.py; include/m2d.h "beat alignment"):
//   m2d_stft_bands    band energies of STFT frames, the DFT as an fp32-MFMA contraction with the band projection fused;
//   m2d_onset_flux    log-compressed, half-wave rectified spectral flux of the band energies;
//   m2d_motion_speed  mean joint speed of a dance;
//   m2d_beat_align    smoothing, event detection, nearest-event distances and the two scores, one workgroup per row;
//   m2d_gauss_smooth  that smoothing alone, for curves of any length;
//   m2d_sync_scan     Pearson correlation of two curves over a grid of lags and time-scale factors.
//
// m2d_stft_bands. A workgroup owns one row and a tile of F <= 32 consecutive frames. Their windows overlap, so the
// tile's samples are staged ONCE in LDS as one span of (F - 1) hop + n_fft floats (32 frames at hop 640, n_fft 1024:
// 20 864 samples, 83 KB), zeros outside [0, S); nothing of shape (B, T, n_fft) exists anywhere. The contraction runs
// transposed, C[bin][frame] = sum_k basis[bin][k] x[s_frame + k] on v_mfma_f32_32x32x2_f32: A = the windowed basis (one
// float per lane: bin = lane & 31, k = 2 step + (lane >> 5)), B = the samples (frame = lane & 31, the same k). The
// cosine and the sine accumulator of a tile of 32 bins share the B operand and the C layout (column = frame, row = bin
// (r & 3) + 8 (r >> 2) + 4 (lane >> 5)), so re^2 + im^2 is elementwise in registers - and register r of that power tile
// IS the B operand of a second MFMA whose k pair is the bins (r & 3) + 8 (r >> 2) and + 4: E^T[band][frame] +=
// bands[band][bin] P[bin][frame] needs no shuffle, no LDS and no HBM. The (T, 2 nbins) spectrum is never written.
//   * Lanes that differ in their frame read LDS addresses hop apart; hop = 640 would put all 32 on one bank. The span
//     is stored with `pad` floats of air after every hop samples, pad = (2 - hop) mod 4: the frame stride hop + pad is
//     twice an odd number, the 32 frames of the lower half wave fall on 32 different even banks and the upper half
//     wave (k + 1) on the odd ones. off[k] = k + (k / hop) pad, a table in LDS, is the address of sample k of frame 0.
//   * bins 0 .. n_fft/2 - 1 are n_fft / 64 tiles of 32, dealt to the 8 waves round robin. DC's sine is identically
//     zero, so its slot in the image carries the Nyquist bin's cosine: tile 0 yields both real bins, and the band
//     projection of tile 0 takes one extra MFMA step for bands[:, n_fft/2].
//   * The basis is n_fft^2 floats (4 MiB at 1024) and every workgroup walks all of it: it is served by L2 / Infinity
//     Cache. A wave's bins are its own - no other wave of the workgroup reads them - so a pass through LDS would buy no
//     reuse; the packed image (m2d_stft_pack_basis) holds, per (tile, chunk of 32 k), each lane's 16 cosine and 16 sine
//     operands as 8 x 16 bytes, read with global_load_dwordx4 one chunk ahead of the MFMAs that use them.
//   * The 8 partial E^T of a workgroup are added in LDS in wave order (fixed), then written (frame, band) row-major.
// Frame t's value depends on t, its samples, the basis and the bands only: the tile size F is a function of (hop, n_fft,
// nb), the lane a frame lands in changes no operation. No atomics.
#include "m2d_common.h"
#include "m2d_device.h"
#include "m2d_reduce.h"

#include <limits.h>
#include <math.h>

#define M2D_SP_THREADS 512
#define M2D_SP_WAVES 8
#define M2D_SP_LDS_MAX (160 * 1024)
#define M2D_SP_MAX_BANDS 128
#define M2D_SP_RED_LD 33
#define M2D_BA_THREADS 1024
#define M2D_BA_MAX_T 16384
#define M2D_BA_MAX_R 64
#define M2D_GS_THREADS 256
#define M2D_SS_THREADS 1024
#define M2D_SS_WAVES 16
#define M2D_SS_LAGS 64      // lags of one (row, factor) a workgroup takes: 4 a wave
#define M2D_SS_MAX_T 16384
#define M2D_SS_MAX_F 32     // factors of one launch (a kernel argument); more go in further launches

namespace {

// table (2, nbins, n) -> image: element (((tile nc + chunk) 8 + v) 64 + lane) 4 + e, v = 4 comp + q, is
// table[comp][32 tile + (lane & 31)][32 chunk + 2 (4 q + e) + (lane >> 5)]; DC's sine slot holds Nyquist's cosine
__global__ void m2d_stft_pack_kernel(const float* __restrict__ table, int n, float* __restrict__ image) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n * n) return;
  const int e = (int)(idx & 3), l = (int)(idx >> 2) & 63, v = (int)(idx >> 8) & 7;
  const int tc = (int)(idx >> 11), nc = n >> 5, nbins = n / 2 + 1;
  const int tb = tc / nc, c = tc - tb * nc;
  const int comp = v >> 2, s = 4 * (v & 3) + e;
  const int k = 32 * c + 2 * s + (l >> 5), bin = 32 * tb + (l & 31);
  image[idx] = (comp == 1 && bin == 0) ? table[(size_t)(nbins - 1) * n + k]
                                       : table[((size_t)comp * nbins + bin) * n + k];
}

__global__ void __launch_bounds__(M2D_SP_THREADS) m2d_stft_bands_kernel(
    const float* __restrict__ x, long long ldx, int S, long long frame0, int T, int hop, int n,
    const float* __restrict__ image, const float* __restrict__ bands, int nb, float* __restrict__ E, int F, int tiles,
    int pad, int xs_floats) {
  extern __shared__ float sh[];
  float* xs = sh;                          // the tile's span, `pad` floats of air after every hop samples
  int* off = (int*)(sh + xs_floats);       // [n]
  float* red = sh + xs_floats + n;         // [32 nbt][33]: E^T of the tile
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const int i0 = tile * F;
  const int nfr = min(F, T - i0);
  const long long g0 = (frame0 + i0) * (long long)hop + hop / 2 - n / 2;
  const int span = (F - 1) * hop + n;
  const int nbt = (nb + 31) >> 5;
  const float* xrow = x + (long long)row * ldx;
  for (int p = tid; p < span; p += M2D_SP_THREADS) {
    const long long g = g0 + p;
    xs[p + (int)((unsigned)p / (unsigned)hop) * pad] = (g >= 0 && g < S) ? xrow[g] : 0.f;
  }
  for (int k = tid; k < n; k += M2D_SP_THREADS) off[k] = k + (int)((unsigned)k / (unsigned)hop) * pad;
  for (int i = tid; i < nbt * 32 * M2D_SP_RED_LD; i += M2D_SP_THREADS) red[i] = 0.f;
  __syncthreads();

  const float* xl = xs + (l31 < F ? l31 : 0) * (hop + pad);   // lanes past the tile recompute frame 0 (not stored)
  const int NT = n >> 6, NC = n >> 5, nbins = n / 2 + 1;
  f32x16 eacc[4];
#pragma unroll
  for (int bt = 0; bt < 4; ++bt)
#pragma unroll
    for (int r = 0; r < 16; ++r) eacc[bt][r] = 0.f;

  for (int tb = w; tb < NT; tb += M2D_SP_WAVES) {
    f32x16 re, im;
#pragma unroll
    for (int r = 0; r < 16; ++r) re[r] = im[r] = 0.f;
    const m2d_f32x4* img = reinterpret_cast<const m2d_f32x4*>(image) + (size_t)tb * NC * 512 + lane;
    m2d_f32x4 cur[8], nxt[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) nxt[v] = cur[v] = img[v * 64];
    for (int c = 0; c < NC; ++c) {
      if (c + 1 < NC) {
#pragma unroll
        for (int v = 0; v < 8; ++v) nxt[v] = img[((c + 1) * 8 + v) * 64];
      }
      const int* oc = off + 32 * c + h;
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const float xv = xl[oc[2 * s]];
        re = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[s >> 2][s & 3], xv, re, 0, 0, 0);
        im = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[4 + (s >> 2)][s & 3], xv, im, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 8; ++v) cur[v] = nxt[v];
    }
    // power, in the accumulators' layout: P[r] = |X[bin (r & 3) + 8 (r >> 2) + 4 h][frame l31]|^2
    float P[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) P[r] = re[r] * re[r] + im[r] * im[r];
    float pny = 0.f;
    if (tb == 0) {   // row 0 (r = 0, h = 0): `re` is DC, `im` the Nyquist bin - two real bins
      const float dc = re[0] * re[0], ny = im[0] * im[0];
      if (h == 0) {
        P[0] = dc;
        pny = ny;
      }
    }
#pragma unroll
    for (int bt = 0; bt < 4; ++bt) {
      if (bt < nbt) {
        const int band = 32 * bt + l31;
        const bool ok = band < nb;
        const float* brow = bands + (size_t)(ok ? band : nb - 1) * nbins;
        const float* bt0 = brow + 32 * tb + 4 * h;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float a = bt0[(r & 3) + 8 * (r >> 2)];
          eacc[bt] = __builtin_amdgcn_mfma_f32_32x32x2f32(ok ? a : 0.f, P[r], eacc[bt], 0, 0, 0);
        }
        if (tb == 0) {
          const float a = brow[nbins - 1];
          eacc[bt] = __builtin_amdgcn_mfma_f32_32x32x2f32((ok && h == 0) ? a : 0.f, pny, eacc[bt], 0, 0, 0);
        }
      }
    }
  }
  // the waves' partial E^T, added in wave order
  for (int ww = 0; ww < M2D_SP_WAVES; ++ww) {
    if (w == ww) {
#pragma unroll
      for (int bt = 0; bt < 4; ++bt)
        if (bt < nbt) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            red[(32 * bt + (r & 3) + 8 * (r >> 2) + 4 * h) * M2D_SP_RED_LD + l31] += eacc[bt][r];
        }
    }
    __syncthreads();
  }
  float* Et = E + ((size_t)row * T + i0) * nb;
  for (int i = tid; i < nfr * nb; i += M2D_SP_THREADS) {
    const int f = i / nb, b = i - f * nb;
    Et[i] = red[b * M2D_SP_RED_LD + f];
  }
}

__global__ void m2d_onset_flux_kernel(const float* __restrict__ E, long long rows, int T, int nb, float gamma,
                                      float* __restrict__ o) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // (b, t)
  if (i >= rows) return;
  const int t = (int)(i % T);
  float acc = 0.f;
  if (t > 0) {
    const float* cur = E + i * nb;
    const float* prev = cur - nb;
    for (int b = 0; b < nb; ++b) acc += fmaxf(0.f, log1pf(gamma * cur[b]) - log1pf(gamma * prev[b]));
    acc = acc / (float)nb;
  }
  o[i] = acc;
}

__global__ void m2d_motion_speed_kernel(const float* __restrict__ p, long long rows, int T, int J,
                                        float* __restrict__ v) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;   // (b, t)
  if (i >= rows) return;
  const int t = (int)(i % T);
  const float* cur = p + (i + (t == 0 ? 1 : 0)) * J * 3;           // v[0] = v[1]: the same operations
  const float* prev = cur - (size_t)J * 3;
  float acc = 0.f;
  for (int j = 0; j < J; ++j) {
    const float dx = cur[3 * j] - prev[3 * j], dy = cur[3 * j + 1] - prev[3 * j + 1],
                dz = cur[3 * j + 2] - prev[3 * j + 2];
    acc += sqrtf(dx * dx + dy * dy + dz * dz);
  }
  v[i] = acc / (float)J;
}

// ---- m2d_beat_align: one workgroup per row ------------------------------------------------------------------------
#define BA_NEG (-(1 << 30))
#define BA_BIG (1 << 20)

__device__ void ba_scan_max(int* sc) {   // inclusive, over the M2D_BA_THREADS entries; callers sync before writing sc
  const int tid = threadIdx.x;
  __syncthreads();
  for (int d = 1; d < M2D_BA_THREADS; d <<= 1) {
    const int a = sc[tid], b = tid >= d ? sc[tid - d] : BA_NEG;
    __syncthreads();
    sc[tid] = a > b ? a : b;
    __syncthreads();
  }
}

// The smoothing g(c, sigma) of m2d_beat_align and m2d_gauss_smooth, stated once. ba_weights: wt[j + R] = w_j for j in
// [-R, R], by the first `threads` threads of the workgroup (the caller syncs afterwards). ba_smooth_at: g(c, sigma)[t],
// fp64 sums in ascending j, one rounding to fp32.
__device__ __forceinline__ void ba_weights(double* wt, double sigma, int R, int threads) {
  for (int j = threadIdx.x; j <= 2 * R; j += threads)
    wt[j] = exp(-(double)((j - R) * (j - R)) / (2.0 * sigma * sigma));
}

__device__ __forceinline__ float ba_smooth_at(const float* __restrict__ c, int T, int t, int R, const double* wt) {
  double num = 0.0, den = 0.0;
  for (int j = -R; j <= R; ++j) {
    const int u = t + j;
    if (u >= 0 && u < T) {
      num += wt[j + R] * (double)c[u];
      den += wt[j + R];
    }
  }
  return (float)(num / den);
}

// sm[t] = g(c, sigma)[t]; mask[t] = event; -> the number of events
__device__ int ba_curve(const float* __restrict__ c, int T, double sigma, int R, bool music, float* sm,
                        unsigned char* mask, double* wt, double* redd, float* out_sm, unsigned char* out_mask, int lo,
                        int hi) {
  const int tid = threadIdx.x;
  __syncthreads();
  ba_weights(wt, sigma, R, M2D_BA_THREADS);
  __syncthreads();
  for (int t = tid; t < T; t += M2D_BA_THREADS) {
    const float r = ba_smooth_at(c, T, t, R, wt);
    sm[t] = r;
    if (out_sm) out_sm[t] = r;
  }
  __syncthreads();
  double mean = 0.0;
  if (music) {
    double part = 0.0;
    for (int t = lo; t < hi; ++t) part += (double)sm[t];
    mean = m2d_block_sum<M2D_BA_THREADS>(part, redd) / (double)T;
  }
  int n = 0;
  for (int t = lo; t < hi; ++t) {
    bool ev = false;
    if (t >= 1 && t <= T - 2) {
      const float a = sm[t - 1], b = sm[t], d = sm[t + 1];
      ev = music ? (b > a && b >= d && (double)b > mean) : (b < a && b <= d);
    }
    mask[t] = ev ? 1 : 0;
    if (out_mask) out_mask[t] = ev ? 1 : 0;
    n += ev ? 1 : 0;
  }
  return (int)(m2d_block_sum<M2D_BA_THREADS>((double)n, redd) + 0.5);
}

// sum over the events t of Y of exp(-d(t)^2 / (2 sa^2)), d(t) the distance to the nearest event of X (X not empty)
__device__ double ba_nearest(const unsigned char* X, const unsigned char* Y, int* dist, int* sc, double* redd, float sa,
                             int lo, int hi) {
  const int tid = threadIdx.x;
  int last = BA_NEG;
  for (int t = lo; t < hi; ++t)
    if (X[t]) last = t;
  __syncthreads();
  sc[tid] = last;
  ba_scan_max(sc);
  int c = tid > 0 ? sc[tid - 1] : BA_NEG;
  for (int t = lo; t < hi; ++t) {
    if (X[t]) c = t;
    dist[t] = c == BA_NEG ? BA_BIG : t - c;
  }
  int first = BA_NEG;   // -(index of the segment's first event)
  for (int t = hi - 1; t >= lo; --t)
    if (X[t]) first = -t;
  __syncthreads();
  sc[M2D_BA_THREADS - 1 - tid] = first;
  ba_scan_max(sc);
  c = tid < M2D_BA_THREADS - 1 ? sc[M2D_BA_THREADS - 2 - tid] : BA_NEG;
  double sum = 0.0;
  const float den = 2.f * sa * sa;
  for (int t = hi - 1; t >= lo; --t) {
    if (X[t]) c = -t;
    if (Y[t]) {
      const int dn = c == BA_NEG ? BA_BIG : -c - t;
      const float d = (float)(dist[t] < dn ? dist[t] : dn);
      sum += (double)expf(-(d * d) / den);
    }
  }
  return m2d_block_sum<M2D_BA_THREADS>(sum, redd);
}

__global__ void __launch_bounds__(M2D_BA_THREADS) m2d_beat_align_kernel(
    const float* __restrict__ o, const float* __restrict__ v, int T, int Tpad, double so, int Ro, double sv, int Rv,
    float sa, float* __restrict__ scores, unsigned char* motion_events, unsigned char* music_events,
    float* onset_smooth, float* speed_smooth) {
  extern __shared__ unsigned char shb[];
  float* sm = reinterpret_cast<float*>(shb);   // the smoothed curve; afterwards the distances
  int* dist = reinterpret_cast<int*>(shb);
  unsigned char* maskM = shb + 4 * (size_t)Tpad;
  unsigned char* maskK = maskM + Tpad;
  double* redd = reinterpret_cast<double*>(maskK + Tpad);
  double* wt = redd + M2D_BA_THREADS;
  int* sc = reinterpret_cast<int*>(wt + 2 * M2D_BA_MAX_R + 2);
  const int tid = threadIdx.x;
  const size_t r0 = (size_t)blockIdx.x * T;
  const int seg = (T + M2D_BA_THREADS - 1) / M2D_BA_THREADS;
  const int lo = min(T, tid * seg), hi = min(T, lo + seg);
  const int nM = ba_curve(o + r0, T, so, Ro, true, sm, maskM, wt, redd, onset_smooth ? onset_smooth + r0 : nullptr,
                          music_events ? music_events + r0 : nullptr, lo, hi);
  const int nK = ba_curve(v + r0, T, sv, Rv, false, sm, maskK, wt, redd, speed_smooth ? speed_smooth + r0 : nullptr,
                          motion_events ? motion_events + r0 : nullptr, lo, hi);
  float align = nanf(""), cover = nanf("");
  if (nM > 0 && nK > 0) {   // uniform over the workgroup
    align = (float)(ba_nearest(maskM, maskK, dist, sc, redd, sa, lo, hi) / (double)nK);
    cover = (float)(ba_nearest(maskK, maskM, dist, sc, redd, sa, lo, hi) / (double)nM);
  }
  if (tid < 4) scores[(size_t)blockIdx.x * 4 + tid] = tid == 0 ? align : tid == 1 ? cover : tid == 2 ? (float)nK : (float)nM;
}

// ---- m2d_gauss_smooth: g(c, sigma) row by row, the expression of ba_curve --------------------------------------------
__global__ void __launch_bounds__(M2D_GS_THREADS) m2d_gauss_smooth_kernel(const float* __restrict__ c, int T, int tiles,
                                                                          double sigma, int R, float* __restrict__ out) {
  __shared__ double wt[2 * M2D_BA_MAX_R + 2];
  const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  ba_weights(wt, sigma, R, M2D_GS_THREADS);
  __syncthreads();
  const int t = tile * M2D_GS_THREADS + threadIdx.x;
  if (t < T) out[(size_t)row * T + t] = ba_smooth_at(c + (size_t)row * T, T, t, R, wt);
}

// ---- m2d_sync_scan: the lag / tempo-factor profile of two curves -------------------------------
// A workgroup owns one row, one factor and M2D_SS_LAGS consecutive lags; it stages the row's a and b in LDS once and its
// 16 waves take the lags in turn. ONE wave computes a cell: lane k owns the residue class j = k (mod 64), walks it in
// ascending j with fp64 accumulators, and the 64 partials are added by the xor butterfly 32, 16, 8, 4, 2, 1 (every lane
// ends with the same bits). Pass 1: n and the two sums; pass 2: the three centred sums, the pairs rebuilt by the same
// operations. Which wave or workgroup a cell lands in changes no operation: r and n are functions of the row's values,
// na, nb, f, l and min_overlap alone.
struct SsFactors {
  double f[M2D_SS_MAX_F];
};

__device__ __forceinline__ double ss_wave_sum(double v) {
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s);
  return v;
}

// the pair of a[j]: x = (j + l) / f; false once x has left [0, nb - 1] (x grows with j; the callers start at j + l >= 0)
__device__ __forceinline__ bool ss_pair(const float* bs, int nb, double f, long long jl, double& bv) {
  const double x = (double)jl / f;
  if (!(x <= (double)(nb - 1))) return false;
  const int i = (int)x;
  const double fr = x - (double)i;
  const double b0 = (double)bs[i], b1 = (double)bs[i + 1 < nb ? i + 1 : nb - 1];
  bv = b0 + fr * (b1 - b0);
  return true;
}

__global__ void __launch_bounds__(M2D_SS_THREADS) m2d_sync_scan_kernel(
    const float* __restrict__ a, long long lda, const int* __restrict__ na_rows, const float* __restrict__ b,
    long long ldb, const int* __restrict__ nb_rows, int Ta, int Tb, SsFactors fac, int f0, int F, int L, int chunks,
    int min_overlap, double* __restrict__ r, int* __restrict__ n) {
  extern __shared__ float ssh[];
  float* as = ssh;
  float* bs = ssh + ((Ta + 3) & ~3);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks, fi = blockIdx.y;
  int na = na_rows ? na_rows[row] : Ta, nb = nb_rows ? nb_rows[row] : Tb;
  if (na < 0 || na > Ta || nb < 0 || nb > Tb) na = nb = 0;   // (refused on the host; under a capture: an empty row)
  const float* arow = a + (long long)row * lda;
  const float* brow = b + (long long)row * ldb;
  for (int i = tid; i < na; i += M2D_SS_THREADS) as[i] = arow[i];
  for (int i = tid; i < nb; i += M2D_SS_THREADS) bs[i] = brow[i];
  __syncthreads();
  const double f = fac.f[fi];
  const long long cells = 2LL * L + 1;
  const size_t out0 = ((size_t)row * F + f0 + fi) * (size_t)cells;
  for (int c = w; c < M2D_SS_LAGS; c += M2D_SS_WAVES) {
    const long long li = (long long)chunk * M2D_SS_LAGS + c;
    if (li >= cells) break;
    const long long l = li - L;
    // lane's first j: the smallest j = lane (mod 64) with j + l >= 0
    long long j0 = lane;
    if (-l > j0) j0 += ((-l - j0 + 63) / 64) * 64;
    int cnt = 0;
    double sa = 0.0, sb = 0.0;
    if (nb > 0) {
      for (long long j = j0; j < na; j += 64) {
        double bv;
        if (!ss_pair(bs, nb, f, j + l, bv)) break;
        sa += (double)as[j];
        sb += bv;
        ++cnt;
      }
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
    sa = ss_wave_sum(sa);
    sb = ss_wave_sum(sb);
    double rv = nan("");
    if (cnt >= min_overlap) {   // uniform over the wave
      const double ma = sa / (double)cnt, mb = sb / (double)cnt;
      double sab = 0.0, saa = 0.0, sbb = 0.0;
      for (long long j = j0; j < na; j += 64) {
        double bv;
        if (!ss_pair(bs, nb, f, j + l, bv)) break;
        const double da = (double)as[j] - ma, db = bv - mb;
        sab += da * db;
        saa += da * da;
        sbb += db * db;
      }
      sab = ss_wave_sum(sab);
      saa = ss_wave_sum(saa);
      sbb = ss_wave_sum(sbb);
      if (saa != 0.0 && sbb != 0.0) rv = sab / sqrt(saa * sbb);
    }
    if (lane == 0) {
      r[out0 + li] = rv;
      n[out0 + li] = cnt;
    }
  }
}

int sp_nfft_ok(int n) { return n >= 256 && n <= 2048 && (n & (n - 1)) == 0; }

}  // namespace

extern "C" {

size_t m2d_stft_image_elems(int n_fft) { return sp_nfft_ok(n_fft) ? (size_t)n_fft * n_fft : 0; }

int m2d_stft_pack_basis(const float* table, int n_fft, float* image, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sp_nfft_ok(n_fft)) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_pack_basis: n_fft must be a power of two in [256, 2048] (got %d)", n_fft);
  if (!table || !image) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_pack_basis: null pointer");
  const long long total = (long long)n_fft * n_fft;
  hipLaunchKernelGGL(m2d_stft_pack_kernel, dim3((unsigned)(total / 256)), dim3(256), 0, stream, table, n_fft, image);
  M2D_CHECK_LAUNCH("m2d_stft_pack_basis");
  return M2D_OK;
}

int m2d_stft_bands(const float* x, long long ldx, int S, int B, long long frame0, int T, int hop, int n_fft,
                   const float* image, const float* bands, int nb, float* E, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!sp_nfft_ok(n_fft)) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: n_fft must be a power of two in [256, 2048] (got %d)", n_fft);
  if (nb <= 0 || nb > M2D_SP_MAX_BANDS) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: 1 to %d bands (got %d)", M2D_SP_MAX_BANDS, nb);
  if (hop <= 0 || B <= 0 || T < 0 || S < 0 || frame0 < 0)
    M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: hop and B must be positive, T, S and frame0 non-negative");
  if (ldx < S) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: ldx < S");
  if (!image || !bands || (!x && S > 0) || (!E && T > 0)) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: null pointer");
  if (((uintptr_t)image & 15) != 0) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: the basis image must be 16-byte aligned");
  if (frame0 > LLONG_MAX - T || frame0 + T > (LLONG_MAX - 2 * (long long)n_fft) / hop - 64)
    M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: frame * hop leaves 63 bits");
  if (T == 0) return M2D_OK;

  const int pad = (6 - hop % 4) % 4;   // hop + pad = 2 (mod 4)
  const int nbt = (nb + 31) / 32;
  const long long fixed = n_fft + (long long)nbt * 32 * M2D_SP_RED_LD;
  auto xs_need = [&](int f) {
    const long long span = (long long)(f - 1) * hop + n_fft;
    return (span + (span / hop) * pad + 4) & ~3ll;
  };
  int F = 32;   // a function of (hop, n_fft, nb) alone
  while (F > 1 && 4 * (xs_need(F) + fixed) > M2D_SP_LDS_MAX) --F;
  const long long xs_floats = xs_need(F);
  const long long lds = 4 * (xs_floats + fixed);
  if (lds > M2D_SP_LDS_MAX) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: %lld bytes of LDS needed", lds);
  const long long tiles = m2d_ceil_div64(T, F);
  if (tiles * B > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_stft_bands: too many tiles");

  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&m2d_stft_bands_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, M2D_SP_LDS_MAX) != hipSuccess)
      M2D_FAIL(M2D_ERR_HIP, "m2d_stft_bands: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  M2dProfScope prof(M2D_FAM_GEMM, stream, 4.0 * (double)B * T * (n_fft / 2) * n_fft,
                    4.0 * ((double)tiles * B * n_fft * n_fft + (double)B * T * (hop + nb)), "stft_bands", n_fft, hop,
                    nb);
  hipLaunchKernelGGL(m2d_stft_bands_kernel, dim3((unsigned)(tiles * B)), dim3(M2D_SP_THREADS), (size_t)lds, stream, x,
                     ldx, S, frame0, T, hop, n_fft, image, bands, nb, E, F, (int)tiles, pad, (int)xs_floats);
  M2D_CHECK_LAUNCH("m2d_stft_bands");
  return M2D_OK;
}

int m2d_onset_flux(const float* E, int B, int T, int nb, float gamma, float* o, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T < 0 || nb <= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_onset_flux: B and nb must be positive, T non-negative");
  if (!(gamma >= 0.f)) M2D_FAIL(M2D_ERR_ARG, "m2d_onset_flux: gamma must be non-negative");
  if (T == 0) return M2D_OK;
  if (!E || !o) M2D_FAIL(M2D_ERR_ARG, "m2d_onset_flux: null pointer");
  const long long rows = (long long)B * T;
  const long long grid = m2d_ceil_div64(rows, 256);
  if (grid > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_onset_flux: too many frames");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 4.0 * (double)rows * nb, 4.0 * (double)rows * (nb + 1), "onset_flux",
                    T, nb, 0);
  hipLaunchKernelGGL(m2d_onset_flux_kernel, dim3((unsigned)grid), dim3(256), 0, stream, E, rows, T, nb, gamma, o);
  M2D_CHECK_LAUNCH("m2d_onset_flux");
  return M2D_OK;
}

int m2d_motion_speed(const float* poses, int B, int T, int J, float* v, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T < 2 || J <= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_motion_speed: B and J must be positive, T at least 2");
  if (!poses || !v) M2D_FAIL(M2D_ERR_ARG, "m2d_motion_speed: null pointer");
  const long long rows = (long long)B * T;
  const long long grid = m2d_ceil_div64(rows, 256);
  if (grid > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_motion_speed: too many frames");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 9.0 * (double)rows * J, 4.0 * (double)rows * (3 * J + 1),
                    "motion_speed", T, J, 0);
  hipLaunchKernelGGL(m2d_motion_speed_kernel, dim3((unsigned)grid), dim3(256), 0, stream, poses, rows, T, J, v);
  M2D_CHECK_LAUNCH("m2d_motion_speed");
  return M2D_OK;
}

int m2d_beat_align_max_frames(void) { return M2D_BA_MAX_T; }

int m2d_beat_align(const float* onset, const float* speed, int B, int T, double sigma_onset, double sigma_speed,
                   double sigma_align, float* scores, unsigned char* motion_events, unsigned char* music_events,
                   float* onset_smooth, float* speed_smooth, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T < 0) M2D_FAIL(M2D_ERR_ARG, "m2d_beat_align: B must be positive, T non-negative");
  if (T > M2D_BA_MAX_T) M2D_FAIL(M2D_ERR_ARG, "m2d_beat_align: at most %d frames a row (got %d)", M2D_BA_MAX_T, T);
  if (!(sigma_onset > 0.0) || !(sigma_speed > 0.0) || !(sigma_align > 0.0))
    M2D_FAIL(M2D_ERR_ARG, "m2d_beat_align: the three sigmas must be positive");
  if (3.0 * sigma_onset > M2D_BA_MAX_R || 3.0 * sigma_speed > M2D_BA_MAX_R)
    M2D_FAIL(M2D_ERR_ARG, "m2d_beat_align: a smoothing radius ceil(3 sigma) above %d", M2D_BA_MAX_R);
  if (!scores || (T > 0 && (!onset || !speed))) M2D_FAIL(M2D_ERR_ARG, "m2d_beat_align: null pointer");
  const int Ro = (int)ceil(3.0 * sigma_onset), Rv = (int)ceil(3.0 * sigma_speed);
  const int Tpad = (T + 15) & ~15;
  const size_t lds = 6 * (size_t)Tpad + 8 * (M2D_BA_THREADS + 2 * M2D_BA_MAX_R + 2) + 4 * M2D_BA_THREADS;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&m2d_beat_align_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, M2D_SP_LDS_MAX) != hipSuccess)
      M2D_FAIL(M2D_ERR_HIP, "m2d_beat_align: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 4.0 * (double)B * T * (Ro + Rv + 2), 8.0 * (double)B * T, "beat_align", T,
                    Ro, Rv);
  hipLaunchKernelGGL(m2d_beat_align_kernel, dim3((unsigned)B), dim3(M2D_BA_THREADS), lds, stream, onset, speed, T, Tpad,
                     sigma_onset, Ro, sigma_speed, Rv, (float)sigma_align, scores, motion_events, music_events,
                     onset_smooth, speed_smooth);
  M2D_CHECK_LAUNCH("m2d_beat_align");
  return M2D_OK;
}

int m2d_gauss_smooth(const float* c, int B, int T, double sigma, float* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T < 0) M2D_FAIL(M2D_ERR_ARG, "m2d_gauss_smooth: B must be positive, T non-negative");
  if (!(sigma > 0.0)) M2D_FAIL(M2D_ERR_ARG, "m2d_gauss_smooth: sigma must be positive");
  if (3.0 * sigma > M2D_BA_MAX_R)
    M2D_FAIL(M2D_ERR_ARG, "m2d_gauss_smooth: a smoothing radius ceil(3 sigma) above %d", M2D_BA_MAX_R);
  if (T == 0) return M2D_OK;
  if (!c || !out) M2D_FAIL(M2D_ERR_ARG, "m2d_gauss_smooth: null pointer");
  const int R = (int)ceil(3.0 * sigma);
  const long long tiles = m2d_ceil_div64(T, M2D_GS_THREADS);
  if (tiles * B > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_gauss_smooth: too many frames");
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 4.0 * (double)B * T * (R + 1), 8.0 * (double)B * T, "gauss_smooth", T, R, 0);
  hipLaunchKernelGGL(m2d_gauss_smooth_kernel, dim3((unsigned)(tiles * B)), dim3(M2D_GS_THREADS), 0, stream, c, T,
                     (int)tiles, sigma, R, out);
  M2D_CHECK_LAUNCH("m2d_gauss_smooth");
  return M2D_OK;
}

int m2d_sync_scan_max_frames(void) { return M2D_SS_MAX_T; }

// the per-row lengths live on the device: one small copy tells the host whether any leaves [0, T]. Not inside a stream
// capture (a copy to the host would end it): there the kernel treats such a row as empty.
static int ss_check_lengths(const int* rows, int B, int T, const char* what, hipStream_t stream) {
  if (!rows) return M2D_OK;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cap) != hipSuccess) M2D_FAIL(M2D_ERR_HIP, "m2d_sync_scan: cannot query the stream");
  if (cap != hipStreamCaptureStatusNone) return M2D_OK;
  int* host = (int*)malloc(sizeof(int) * (size_t)B);
  if (!host) M2D_FAIL(M2D_ERR_HIP, "m2d_sync_scan: out of host memory");
  hipError_t e = hipMemcpyAsync(host, rows, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  int bad = -1;
  if (e == hipSuccess)
    for (int i = 0; i < B && bad < 0; ++i)
      if (host[i] < 0 || host[i] > T) bad = i;
  const int len = bad >= 0 ? host[bad] : 0;
  free(host);
  if (e != hipSuccess) M2D_FAIL(M2D_ERR_HIP, "m2d_sync_scan: reading %s failed: %s", what, hipGetErrorString(e));
  if (bad >= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: %s[%d] = %d lies outside [0, %d]", what, bad, len, T);
  return M2D_OK;
}

int m2d_sync_scan(const float* a, long long lda, const int* na_rows, const float* b, long long ldb, const int* nb_rows,
                  int B, int Ta, int Tb, const double* factors, int F, int L, int min_overlap, double* r, int* n,
                  void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || F <= 0 || L < 0) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: B and F must be positive, L non-negative");
  if (Ta < 0 || Tb < 0) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: Ta and Tb must be non-negative");
  if (Ta > M2D_SS_MAX_T || Tb > M2D_SS_MAX_T)
    M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: at most %d frames a row (got %d and %d)", M2D_SS_MAX_T, Ta, Tb);
  if (min_overlap < 2) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: min_overlap must be at least 2 (got %d)", min_overlap);
  if (lda < Ta || ldb < Tb) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: lda < Ta or ldb < Tb");
  if (!factors || !r || !n || (!a && Ta > 0) || (!b && Tb > 0)) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: null pointer");
  if (((uintptr_t)a & 3) || ((uintptr_t)b & 3) || ((uintptr_t)na_rows & 3) || ((uintptr_t)nb_rows & 3) ||
      ((uintptr_t)r & 7) || ((uintptr_t)n & 3))
    M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: a misaligned pointer");
  for (int i = 0; i < F; ++i)
    if (!(factors[i] > 0.0) || !isfinite(factors[i]))
      M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: factor %d must be positive and finite (got %g)", i, factors[i]);
  const long long chunks = m2d_ceil_div64(2LL * L + 1, M2D_SS_LAGS);
  if (chunks * B > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_sync_scan: too many lags");
  int rc = ss_check_lengths(na_rows, B, Ta, "na_rows", stream);
  if (rc == M2D_OK) rc = ss_check_lengths(nb_rows, B, Tb, "nb_rows", stream);
  if (rc != M2D_OK) return rc;

  const size_t lds = 4 * ((size_t)((Ta + 3) & ~3) + (size_t)Tb);
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&m2d_sync_scan_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, M2D_SP_LDS_MAX) != hipSuccess)
      M2D_FAIL(M2D_ERR_HIP, "m2d_sync_scan: cannot raise the dynamic LDS limit");
    attr_set = true;
  }
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 16.0 * (double)B * F * (2.0 * L + 1) * Ta,
                    4.0 * (double)B * ((double)Ta + Tb) + 12.0 * (double)B * F * (2.0 * L + 1), "sync_scan", Ta, Tb, L);
  for (int f0 = 0; f0 < F; f0 += M2D_SS_MAX_F) {
    const int Fc = F - f0 < M2D_SS_MAX_F ? F - f0 : M2D_SS_MAX_F;
    SsFactors fac;
    for (int i = 0; i < M2D_SS_MAX_F; ++i) fac.f[i] = i < Fc ? factors[f0 + i] : 1.0;
    hipLaunchKernelGGL(m2d_sync_scan_kernel, dim3((unsigned)(chunks * B), (unsigned)Fc), dim3(M2D_SS_THREADS), lds,
                       stream, a, lda, na_rows, b, ldb, nb_rows, Ta, Tb, fac, f0, F, L, (int)chunks, min_overlap, r, n);
    M2D_CHECK_LAUNCH("m2d_sync_scan");
  }
  return M2D_OK;
}

}  // extern "C"
