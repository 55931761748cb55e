// Label conditioning and dropout of the conditional phase-2 networks (phase2/archis/conditional.py):
//   * [x | E[label]] concatenation, batch-first for the generator's GRU input and channels-first for the critic
//   * m2d_pose_pack3 and its labelled variant: the critic's [interpolated | real | fake] rows, with their label channels
//   * the embedding-table gradient: a fixed-order fp64 sum, one workgroup per (class, column), no atomics
//   * dropout y = x * keep * scale from a caller's byte mask or from Philox4x32-10 bits made on the device
//   * standard normals indexed by absolute frame (the streaming generator's noise, phase3/generate.py)
// Labels are int64 (torch's default index type). A label outside [0, L) never indexes the table: the features it would
// have selected (forward) or the whole table gradient (backward) become NaN, so the loss shows it.
#include "m2d_common.h"
#include "m2d_reduce.h"

namespace {

__device__ __forceinline__ float label_feature(const float* E, const long long* labels, int b, int d, int L, int D) {
  const long long l = labels[b];
  return (l >= 0 && l < L) ? E[l * D + d] : __int_as_float(0x7fc00000);
}

// one thread per output element; layout 0: out (B, T, C + D), layout 1: out (B, C + D, T)
__global__ void __launch_bounds__(256) m2d_label_concat_kernel(const float* __restrict__ x, const float* __restrict__ E,
                                                               const long long* __restrict__ labels,
                                                               float* __restrict__ out, int B, int T, int C, int L,
                                                               int D, int layout) {
  const int Ct = C + D;
  const long long n = (long long)B * T * Ct;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int b, t, c;
  if (layout == 0) {
    c = (int)(i % Ct);
    const long long bt = i / Ct;
    t = (int)(bt % T);
    b = (int)(bt / T);
    out[i] = c < C ? x[bt * C + c] : label_feature(E, labels, b, c - C, L, D);
  } else {
    t = (int)(i % T);
    const long long bc = i / T;
    c = (int)(bc % Ct);
    b = (int)(bc / Ct);
    out[i] = c < C ? x[((long long)b * C + c) * T + t] : label_feature(E, labels, b, c - C, L, D);
  }
}

// ---------------------------------------------------------------- critic-iteration input pack
// The critic iteration's three pose batches in ONE channels-first buffer (3B, C + D, T) - [interpolated | real | fake] -
// from the loader's real poses (B, T, C) and the generator's rows (B*T, C) (phase3/train.py:196-199 permute +
// contiguous, losses.py:13-25 interpolate): a (32 frames x C joints) tile is read as one contiguous run, staged in
// LDS, and leaves as 128-byte runs along time per joint row. The interpolation is the reference's expression,
// three separately rounded fp32 operations. LABELS: D label channels E[label] follow the C pose channels of every row
// (the interpolated rows carry the real labels); without them D = 0 and the struct is empty.
#define M2D_PACK_TT 32
template <bool LABELS>
struct PackLabels {};
template <>
struct PackLabels<true> {
  const float* E;
  const long long* real_lbl;
  const long long* fake_lbl;
  int L, D;
};

template <bool LABELS>
__global__ void __launch_bounds__(256) m2d_pose_pack3_kernel(const float* __restrict__ real,
                                                             const float* __restrict__ fake,
                                                             const float* __restrict__ alpha, float* __restrict__ out,
                                                             int B, int T, int C, PackLabels<LABELS> lab) {
  extern __shared__ float sh[];  // [2][TT][C + 1]
  const int b = blockIdx.y, t0 = blockIdx.x * M2D_PACK_TT;
  const int nt = min(M2D_PACK_TT, T - t0);
  const int ld = C + 1;
  float* sr = sh;
  float* sf = sh + M2D_PACK_TT * ld;
  const size_t base = ((size_t)b * T + t0) * C;
  for (int i = threadIdx.x; i < nt * C; i += 256) {
    const int t = i / C, c = i - t * C;
    sr[t * ld + c] = real[base + i];
    sf[t * ld + c] = fake[base + i];
  }
  __syncthreads();
  const float a = alpha[b];
  const float na = __fsub_rn(1.f, a);
  int Ct = C;
  if constexpr (LABELS) Ct = C + lab.D;
  const size_t plane = (size_t)Ct * T;
  float* oi = out + (size_t)b * plane + t0;
  float* orl = out + ((size_t)B + b) * plane + t0;
  float* of = out + ((size_t)2 * B + b) * plane + t0;
  for (int i = threadIdx.x; i < C * M2D_PACK_TT; i += 256) {
    const int c = i / M2D_PACK_TT, t = i - c * M2D_PACK_TT;
    if (t < nt) {
      const float r = sr[t * ld + c], f = sf[t * ld + c];
      oi[(size_t)c * T + t] = __fadd_rn(__fmul_rn(a, r), __fmul_rn(na, f));
      orl[(size_t)c * T + t] = r;
      of[(size_t)c * T + t] = f;
    }
  }
  if constexpr (LABELS) {
    for (int i = threadIdx.x; i < lab.D * M2D_PACK_TT; i += 256) {
      const int d = i / M2D_PACK_TT, t = i - d * M2D_PACK_TT;
      if (t < nt) {
        const float er = label_feature(lab.E, lab.real_lbl, b, d, lab.L, lab.D);
        const float ef = label_feature(lab.E, lab.fake_lbl, b, d, lab.L, lab.D);
        oi[(size_t)(C + d) * T + t] = er;
        orl[(size_t)(C + d) * T + t] = er;
        of[(size_t)(C + d) * T + t] = ef;
      }
    }
  }
}

// one workgroup per (l, d) = blockIdx.x: rows in order, each row's T values split over the threads in a fixed pattern,
// fp64 partials, one tree sum at the end - the same bits on every run
__global__ void __launch_bounds__(256) m2d_label_embed_bwd_kernel(const float* __restrict__ dx,
                                                                  const long long* __restrict__ labels,
                                                                  float* __restrict__ dE, int r0, int r1, int T,
                                                                  int Ctot, int c0, int L, int D, int layout) {
  __shared__ double sh[256];
  __shared__ int bad;
  const int l = blockIdx.x / D, d = blockIdx.x - l * D;
  if (threadIdx.x == 0) bad = 0;
  __syncthreads();
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    const long long v = labels[r - r0];
    if (v < 0 || v >= L) bad = 1;
  }
  __syncthreads();
  if (bad) {
    if (threadIdx.x == 0) dE[blockIdx.x] = __int_as_float(0x7fc00000);
    return;
  }
  double acc = 0.0;
  const int c = c0 + d;
  for (int r = r0; r < r1; ++r) {
    if (labels[r - r0] != l) continue;
    const size_t row = (size_t)r * Ctot * T;
    for (int t = threadIdx.x; t < T; t += 256)
      acc += (double)(layout == 0 ? dx[row + (size_t)t * Ctot + c] : dx[row + (size_t)c * T + t]);
  }
  acc = m2d_block_sum<256>(acc, sh);
  if (threadIdx.x == 0) dE[blockIdx.x] = (float)acc;
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011)
__device__ __forceinline__ uint4 philox4x32_10(uint4 ctr, uint2 key) {
  const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    const unsigned hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += W0;
    key.y += W1;
  }
  return ctr;
}

// four elements per thread: counter (i / 4 as 64 bits, offset as 64 bits), key = seed; element i takes word i % 4,
// uniform = (word >> 8) * 2^-24, kept when below p_keep
__global__ void __launch_bounds__(256) m2d_dropout_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          unsigned char* __restrict__ mask, long long n, float p_keep,
                                                          float scale, unsigned long long seed,
                                                          unsigned long long offset, int gen) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long i0 = q * 4;
  if (i0 >= n) return;
  unsigned w[4];
  if (gen) {
    const uint4 r = philox4x32_10(make_uint4((unsigned)q, (unsigned)((unsigned long long)q >> 32), (unsigned)offset,
                                             (unsigned)(offset >> 32)),
                                  make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    w[0] = r.x, w[1] = r.y, w[2] = r.z, w[3] = r.w;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long i = i0 + j;
    if (i < n) {
      float keep;
      if (gen) {
        keep = (float)(w[j] >> 8) * 5.9604644775390625e-8f < p_keep ? 1.f : 0.f;
        if (mask) mask[i] = (unsigned char)keep;
      } else {
        keep = mask[i] ? 1.f : 0.f;
      }
      if (x) y[i] = __fmul_rn(__fmul_rn(x[i], keep), scale);
    }
  }
}

// Standard normals indexed by (seed, batch row, ABSOLUTE frame, channel): one Philox4x32-10 call per (b, frame, group
// of four channels), counter = (c / 4, frame low, frame high, b), key = seed; Box-Muller turns words (0, 1) and (2, 3)
// into channels 4 j + 0, 1 and 4 j + 2, 3: u1 = ((w >> 8) + 1) 2^-24 in (0, 1], u2 = (w >> 8) 2^-24 in [0, 1),
// z = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2). A chunk of frames [frame0, frame0 + n) gets the values a whole-track
// call gives those frames, whatever the chunking.
__device__ __forceinline__ void randn_box_muller(unsigned w1, unsigned w2, float& z0, float& z1) {
  const float u1 = (float)((w1 >> 8) + 1u) * 5.9604644775390625e-8f;
  const float u2 = (float)(w2 >> 8) * 5.9604644775390625e-8f;
  const float r = sqrtf(-2.f * logf(u1));
  float sn, cs;
  sincosf(6.283185307179586f * u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

__global__ void __launch_bounds__(256) m2d_randn_frames_kernel(float* __restrict__ out, unsigned long long seed,
                                                               long long frame0, int B, int n, int C) {
  const int C4 = (C + 3) / 4;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)B * n * C4) return;
  const int j = (int)(q % C4);
  const long long bi = q / C4;  // b * n + i
  const int i = (int)(bi % n);
  const int b = (int)(bi / n);
  const unsigned long long f = (unsigned long long)(frame0 + i);
  const uint4 w = philox4x32_10(make_uint4((unsigned)j, (unsigned)f, (unsigned)(f >> 32), (unsigned)b),
                                make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
  float z[4];
  randn_box_muller(w.x, w.y, z[0], z[1]);
  randn_box_muller(w.z, w.w, z[2], z[3]);
  float* o = out + bi * C;
#pragma unroll
  for (int m = 0; m < 4; ++m)
    if (4 * j + m < C) o[4 * j + m] = z[m];
}

}  // namespace

extern "C" {

int m2d_label_concat(const float* x, const float* E, const long long* labels, float* out, int B, int T, int C, int L,
                     int D, int layout, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T <= 0 || C < 0 || L <= 0 || D <= 0 || (layout != 0 && layout != 1) || !x || !E || !labels || !out)
    M2D_FAIL(M2D_ERR_ARG, "m2d_label_concat: bad arguments");
  const long long n = (long long)B * T * (C + D);
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, 8.0 * (double)n, "label_concat");
  hipLaunchKernelGGL(m2d_label_concat_kernel, dim3((unsigned)m2d_ceil_div64(n, 256)), dim3(256), 0, stream, x, E,
                     labels, out, B, T, C, L, D, layout);
  M2D_CHECK_LAUNCH("m2d_label_concat");
  return M2D_OK;
}

// [interpolated | real | fake] poses channels-first (3B, C, T) from real (B, T, C), fake rows (B*T, C), alpha (B,):
// replaces permute(0,2,1).contiguous() x2 (phase3/train.py:196-199), the interpolation (losses.py:13-25) and the
// concatenation of the batches the critic scores in one pass.
int m2d_pose_pack3(const float* real, const float* fake, const float* alpha, float* out, int B, int T, int C,
                   void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T <= 0 || C <= 0 || C > 1024) M2D_FAIL(M2D_ERR_ARG, "m2d_pose_pack3: bad shape");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, 20.0 * (double)B * T * C, "pose_pack3");
  const size_t lds = 2 * (size_t)M2D_PACK_TT * (C + 1) * sizeof(float);
  hipLaunchKernelGGL(m2d_pose_pack3_kernel<false>, dim3(m2d_ceil_div(T, M2D_PACK_TT), B), dim3(256), lds, stream, real,
                     fake, alpha, out, B, T, C, PackLabels<false>{});
  M2D_CHECK_LAUNCH("m2d_pose_pack3");
  return M2D_OK;
}

int m2d_pose_pack3_label(const float* real, const float* fake, const float* alpha, const float* E,
                         const long long* real_lbl, const long long* fake_lbl, float* out, int B, int T, int C, int L,
                         int D, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T <= 0 || C <= 0 || C > 1024 || L <= 0 || D <= 0 || !real || !fake || !alpha || !E || !real_lbl ||
      !fake_lbl || !out)
    M2D_FAIL(M2D_ERR_ARG, "m2d_pose_pack3_label: bad arguments");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, 4.0 * (double)B * T * (5 * C + 3 * D), "pose_pack3_label");
  const size_t lds = 2 * (size_t)M2D_PACK_TT * (C + 1) * sizeof(float);
  hipLaunchKernelGGL(m2d_pose_pack3_kernel<true>, dim3(m2d_ceil_div(T, M2D_PACK_TT), B), dim3(256), lds, stream, real,
                     fake, alpha, out, B, T, C, PackLabels<true>{E, real_lbl, fake_lbl, L, D});
  M2D_CHECK_LAUNCH("m2d_pose_pack3_label");
  return M2D_OK;
}

int m2d_label_embed_bwd(const float* dx, const long long* labels, float* dE, int r0, int r1, int T, int Ctot, int c0,
                        int L, int D, int layout, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (r0 < 0 || r1 <= r0 || T <= 0 || L <= 0 || D <= 0 || c0 < 0 || c0 + D > Ctot || (layout != 0 && layout != 1) ||
      !dx || !labels || !dE)
    M2D_FAIL(M2D_ERR_ARG, "m2d_label_embed_bwd: bad arguments");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, 4.0 * (double)(r1 - r0) * T * D * L, "label_embed_bwd");
  hipLaunchKernelGGL(m2d_label_embed_bwd_kernel, dim3(L * D), dim3(256), 0, stream, dx, labels, dE, r0, r1, T, Ctot,
                     c0, L, D, layout);
  M2D_CHECK_LAUNCH("m2d_label_embed_bwd");
  return M2D_OK;
}

int m2d_dropout(const float* x, float* y, unsigned char* mask, long long n, float p_keep, float scale,
                unsigned long long seed, unsigned long long offset, int gen, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n <= 0 || (gen != 0 && gen != 1) || (!mask && !gen) || (x && !y) || (!x && !mask))
    M2D_FAIL(M2D_ERR_ARG, "m2d_dropout: bad arguments");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, (x ? 9.0 : 1.0) * (double)n, "dropout");
  hipLaunchKernelGGL(m2d_dropout_kernel, dim3((unsigned)m2d_ceil_div64(n, 1024)), dim3(256), 0, stream, x, y, mask, n,
                     p_keep, scale, seed, offset, gen);
  M2D_CHECK_LAUNCH("m2d_dropout");
  return M2D_OK;
}

int m2d_randn_frames(float* out, unsigned long long seed, long long frame0, int B, int n, int C, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!out || B <= 0 || n <= 0 || C <= 0 || frame0 < 0 || frame0 > (1ll << 62))
    M2D_FAIL(M2D_ERR_ARG, "m2d_randn_frames: bad arguments");
  const long long threads = (long long)B * n * ((C + 3) / 4);
  if (m2d_ceil_div64(threads, 256) > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_randn_frames: too many draws");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, 4.0 * (double)B * n * C, "randn_frames");
  hipLaunchKernelGGL(m2d_randn_frames_kernel, dim3((unsigned)m2d_ceil_div64(threads, 256)), dim3(256), 0, stream, out,
                     seed, frame0, B, n, C);
  M2D_CHECK_LAUNCH("m2d_randn_frames");
  return M2D_OK;
}

}  // extern "C"
