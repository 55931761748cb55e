// Crop + augment gather of a training batch out of the HBM-resident dataset (m2d_crop_augment, include/m2d.h): the
// windows of data.SequenceDataset.sample_batch with a playback speed a / b, a mirror, a yaw about the vertical axis and
// an audio gain per row, in ONE launch. The rule is stated in fp64 by data.augment_window; DESIGN.md section 19.
//
// A workgroup belongs to one row of the batch, so every per-row decision (speed 1/1, identity pose path, no audio) is
// uniform over its waves. Per row the grid holds ceil(S / 2048) audio workgroups followed by ceil(T (C / 3) / 256) pose
// workgroups.
//
// Audio. Output n sits at source time n a / b after the window start: m2d_resample_poly's formula with up = b,
// down = a, restated here (resample.hip keeps its own copy: the two kernels share a definition, not code) -
//   t = n a + half, phi = t mod b, q = t / b, y[n] = g * sum_j taps[phi + j b] X[q - j], j = 0 .. P_phi - 1,
// one fp32 accumulator, fmaf in ascending j, then one multiply by g. X[m] is sample start + m of the flat store where
// that lies inside the row's own take and zero elsewhere (the product with the zero is still accumulated, as the
// resampler does with its zero padding). The row's taps (at most 1 281 floats) are staged in LDS phase-major with an
// odd row stride, as in resample.hip; the samples come straight from global memory: neighbouring lanes read
// neighbouring samples and every sample is re-read by about P lanes of the same wave, which the vector L1 absorbs.
// Speed 1/1 copies: y[n] = g X[n].
//
// Poses. Output frame i shows source position i a / b: j = (i a) div b, r = (i a) mod b, both exact integers;
//   v = x[j] when r == 0, else fmaf(fl(r / b), x[j + 1] - x[j], x[j])
// with j + 1 clamped to the take's last row and read only when r != 0. The identity transform (no mirror, c == 1,
// s == 0) stores v: a row at 1/1 with the identity parameters is the bits of the plain gather. Otherwise, per joint,
//   u = (v - shift) / scale (per column), ux = -ux under the mirror,
//   x' = fmaf(c, ux, s uz), z' = fmaf(c, uz, -(s ux)), y' = uy, out = fmaf(u', scale, shift).
// A thread owns one (frame, joint). Nothing is accumulated across threads, no atomics, no workspace: an output element
// is a pure function of its row's table entry and its index.
#include "m2d_common.h"

#define M2D_AUG_THREADS 256
#define M2D_AUG_TILE 2048          // audio outputs per workgroup
#define M2D_AUG_MAX_TAPS 1281      // 20 * 64 + 1: the default design at max(a, b) = 64
#define M2D_AUG_MAX_RATIO 64
#define M2D_AUG_TAP_LDS 1536       // >= rows * (P | 1) <= ntaps + 2 b for every admissible (ntaps, b)

namespace {

// v into [lo, hi], and into [0, hi] should a broken table say lo > hi (hi < frames, frames >= 1)
__device__ __forceinline__ long long m2d_aug_clamp(long long v, long long lo, long long hi) {
  v = v < lo ? lo : v;
  v = v > hi ? hi : v;
  return v < 0 ? 0 : v;
}

__global__ void __launch_bounds__(M2D_AUG_THREADS) m2d_crop_augment_kernel(
    const float* __restrict__ poses, long long frames, int C, const float* __restrict__ track, long long samples,
    const M2dAugmentRow* __restrict__ table, const float* __restrict__ scale, const float* __restrict__ shift,
    const float* __restrict__ taps, int taps_total, float* __restrict__ out_poses, float* __restrict__ out_audio, int T,
    int S, int tiles_a, int tiles_p) {
  __shared__ float tp[M2D_AUG_TAP_LDS];
  const int per_row = tiles_a + tiles_p;
  const int row = blockIdx.x / per_row;
  const int k = blockIdx.x - row * per_row;
  const M2dAugmentRow R = table[row];     // uniform over the workgroup: scalar loads
  const bool ratio_ok = R.a >= 1 && R.b >= 1 && R.a <= M2D_AUG_MAX_RATIO && R.b <= M2D_AUG_MAX_RATIO;

  if (k < tiles_a) {
    // ------------------------------------------------------------------------------------------------ audio
    const int i0 = k * M2D_AUG_TILE;
    const int cnt = min(M2D_AUG_TILE, S - i0);
    float* y = out_audio + (long long)row * S + i0;
    // the take, cut to the store: a table the wrapper did not check still reads nothing outside the store
    const long long lo = R.audio_first < 0 ? 0 : R.audio_first;
    const long long hi = R.audio_last > samples - 1 ? samples - 1 : R.audio_last;
    const float g = R.gain;
    const bool taps_ok = R.ntaps >= 1 && R.ntaps <= M2D_AUG_MAX_TAPS && (R.ntaps & 1) && R.tap_offset >= 0 &&
                         (long long)R.tap_offset + R.ntaps <= taps_total;
    if (!ratio_ok || (R.a != R.b && !taps_ok)) {   // never through the Python wrapper
      for (int i = threadIdx.x; i < cnt; i += M2D_AUG_THREADS) y[i] = __builtin_nanf("");
      return;
    }
    if (R.a == R.b) {   // speed 1/1: the plain gather, times g
      for (int i = threadIdx.x; i < cnt; i += M2D_AUG_THREADS) {
        const long long idx = R.audio_start + i0 + i;
        y[i] = (idx >= lo && idx <= hi ? track[idx] : 0.f) * g;
      }
      return;
    }
    const int up = R.b, down = R.a, ntaps = R.ntaps;
    const int P = (ntaps + up - 1) / up;
    const int Sd = P | 1;
    const float* h = taps + R.tap_offset;
    for (int t = threadIdx.x; t < ntaps; t += M2D_AUG_THREADS) {
      const int j = t / up;
      tp[(t - j * up) * Sd + j] = h[t];
    }
    __syncthreads();
    const long long half = (ntaps - 1) / 2;
    const long long tA = (long long)i0 * down + half;
    const long long qA = tA / up;
    const unsigned rA = (unsigned)(tA - qA * up);
    const long long src0 = R.audio_start + qA;          // absolute store index of X[qA]
#pragma unroll 1
    for (int i = threadIdx.x; i < cnt; i += M2D_AUG_THREADS) {
      const unsigned l = rA + (unsigned)i * (unsigned)down;   // < 64 + 2048 * 64
      const unsigned qq = l / (unsigned)up;
      const int phi = (int)(l - qq * (unsigned)up);
      float acc = 0.f;
      if (phi < ntaps) {
        const int np = (ntaps - phi + up - 1) / up;           // taps of this phase, 1 .. P
        const float* t = tp + phi * Sd;
        const long long src = src0 + qq;
#pragma unroll 4
        for (int j = 0; j < np; ++j) {
          const long long idx = src - j;
          const float x = (idx >= lo && idx <= hi) ? track[idx] : 0.f;
          acc = fmaf(t[j], x, acc);
        }
      }
      y[i] = acc * g;
    }
    return;
  }

  // -------------------------------------------------------------------------------------------------- poses
  const int J = C / 3;
  const int e = (k - tiles_a) * M2D_AUG_THREADS + threadIdx.x;   // (frame, joint) of this thread
  if (e >= T * J) return;
  const int i = e / J;
  const int jt = e - i * J;
  float* o = out_poses + ((long long)row * T + i) * C + 3 * jt;
  if (!ratio_ok) {
    o[0] = o[1] = o[2] = __builtin_nanf("");
    return;
  }
  const long long first = R.pose_first < 0 ? 0 : R.pose_first;
  const long long last = R.pose_last > frames - 1 ? frames - 1 : (R.pose_last < 0 ? 0 : R.pose_last);
  const long long ia = (long long)i * R.a;
  const long long j = ia / R.b;
  const int r = (int)(ia - j * R.b);
  const long long r0 = m2d_aug_clamp(R.pose_start + j, first, last);
  const float* p0 = poses + r0 * C + 3 * jt;
  float v[3] = {p0[0], p0[1], p0[2]};
  if (r != 0) {
    const float* p1 = poses + (r0 < last ? r0 + 1 : last) * C + 3 * jt;
    const float f = (float)r / (float)R.b;
#pragma unroll
    for (int d = 0; d < 3; ++d) v[d] = fmaf(f, p1[d] - v[d], v[d]);
  }
  const float c = R.cos_yaw, s = R.sin_yaw;
  if (R.mirror != 0 || c != 1.f || s != 0.f) {
    const float* sc = scale + 3 * jt;
    const float* sh = shift + 3 * jt;
    float ux = (v[0] - sh[0]) / sc[0];
    const float uy = (v[1] - sh[1]) / sc[1];
    const float uz = (v[2] - sh[2]) / sc[2];
    if (R.mirror != 0) ux = -ux;
    const float xr = fmaf(c, ux, s * uz);
    const float zr = fmaf(c, uz, -(s * ux));
    v[0] = fmaf(xr, sc[0], sh[0]);
    v[1] = fmaf(uy, sc[1], sh[1]);
    v[2] = fmaf(zr, sc[2], sh[2]);
  }
  o[0] = v[0];
  o[1] = v[1];
  o[2] = v[2];
}

}  // namespace

extern "C" {

int m2d_crop_augment(const float* poses, long long frames, int C, const float* track, long long samples,
                     const M2dAugmentRow* rows, const float* scale, const float* shift, const float* taps,
                     int taps_total, float* out_poses, float* out_audio, int B, int T, int S, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || T <= 0 || C <= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_crop_augment: B, T and C must be positive");
  if (S < 0) M2D_FAIL(M2D_ERR_ARG, "m2d_crop_augment: S must be non-negative");
  if (C % 3 != 0) M2D_FAIL(M2D_ERR_ARG, "m2d_crop_augment: C = %d is not a multiple of 3", C);
  if (!poses || !rows || !scale || !shift || !out_poses || frames <= 0)
    M2D_FAIL(M2D_ERR_ARG, "m2d_crop_augment: null pose store, table, scale, shift or output, or an empty store");
  if (S > 0 && (!track || !taps || !out_audio || samples <= 0 || taps_total <= 0))
    M2D_FAIL(M2D_ERR_ARG, "m2d_crop_augment: S > 0 needs a track store, taps and an audio output");
  const int tiles_a = m2d_ceil_div(S, M2D_AUG_TILE);
  const long long triples = (long long)T * (C / 3);
  const long long tiles_p = m2d_ceil_div64(triples, M2D_AUG_THREADS);
  if (triples > 0x7fffffffLL || (tiles_a + tiles_p) * B > 0x7fffffffLL)
    M2D_FAIL(M2D_ERR_ARG, "m2d_crop_augment: too many workgroups");
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 2.0 * (double)B * S * 21 + 20.0 * (double)B * T * C,
                    8.0 * (double)B * ((double)S + (double)T * C), "crop_augment", B, T, S);
  hipLaunchKernelGGL(m2d_crop_augment_kernel, dim3((unsigned)((tiles_a + tiles_p) * B)), dim3(M2D_AUG_THREADS), 0,
                     stream, poses, frames, C, track, samples, rows, scale, shift, taps, taps_total, out_poses,
                     out_audio, T, S, tiles_a, (int)tiles_p);
  M2D_CHECK_LAUNCH("m2d_crop_augment");
  return M2D_OK;
}

}  // extern "C"
