// Stick-figure rasteriser: the geometry of the reference's visualize.draw (visualize.py:195-244), drawn exactly in
// integers so that a numpy statement of the rule (tests/render_rule.py) matches it bit for bit. DESIGN.md section 11.
//
// One wave owns a contiguous span of RS_SPAN bytes of one frame's RGB image. It builds the frame's 44 primitives in
// its own lanes (lane k holds primitive k: integer endpoints and a bounding box grown by the radius), so there is no
// LDS and no barrier. Each 1 KiB step of the span (64 lanes x 16 bytes) ballots the primitives whose boxes meet the
// step's rows: with none left the step is a plain white store, otherwise every lane tests the six pixels its 16 bytes
// touch against the surviving primitives, read with readlane (uniform). Stores are 16-byte vector stores; the bytes
// before the first and after the last 16-byte boundary of the span (frame tails when a frame is not a multiple of
// 16 bytes) are written one per lane.
#include "m2d_common.h"

namespace {

constexpr int RS_JOINTS = 23;        // points 0..22: joints; 23..26: midpoints
constexpr int RS_POINTS = 27;
constexpr int RS_PRIMS = 44;         // 23 disks (lanes 0..22), 21 segments (lanes 23..43)
constexpr int RS_WAVES = 4;          // waves per workgroup, each on its own span
constexpr unsigned RS_STEP = 1024u;  // bytes per wave step: 64 lanes x 16
constexpr unsigned RS_SPAN = 8u * RS_STEP;
constexpr float RS_LIMIT = 16384.f;  // |x'|, |y'| < 2^14: the exact tests stay inside int64

// the reference's skeleton (visualize.py:200-203 and the six midpoint lines after it), as point indices
__constant__ unsigned char kRsMid[4][2] = {{0, 1}, {3, 12}, {10, 11}, {19, 20}};
__constant__ unsigned char kRsSeg[21][2] = {{0, 1},   {3, 4},   {4, 5},   {5, 6},   {12, 13}, {13, 14}, {14, 15},
                                            {2, 7},   {7, 8},   {8, 9},   {10, 11}, {2, 16},  {16, 17}, {17, 18},
                                            {19, 20}, {23, 24}, {3, 24},  {12, 24}, {2, 24},  {9, 25},  {18, 26}};

// bit i of the result: pixel (cx[i], cy[i]) (column, unflipped height) lies on a primitive of `mask`. Primitive k is
// lane k's, with endpoints (X0, Y0) - (X1, Y1); `mask` is wave-uniform.
template <int NPIX>
__device__ __forceinline__ unsigned rs_cover(unsigned long long mask, const int (&cx)[NPIX], const int (&cy)[NPIX],
                                             int X0, int Y0, int X1, int Y1) {
  unsigned bits = 0;
  while (mask) {
    const int k = __builtin_ctzll(mask);
    mask &= mask - 1;
    const int x0 = __builtin_amdgcn_readlane(X0, k), y0 = __builtin_amdgcn_readlane(Y0, k);
    if (k < RS_JOINTS) {  // disk of radius 4: |dx|, |dy| < 20480 here, the squares fit int32
#pragma unroll
      for (int i = 0; i < NPIX; ++i) {
        const int dx = cx[i] - x0, dy = cy[i] - y0;
        if (dx * dx + dy * dy <= 16) bits |= 1u << i;
      }
      continue;
    }
    const int x1 = __builtin_amdgcn_readlane(X1, k), y1 = __builtin_amdgcn_readlane(Y1, k);
    const int xlo = min(x0, x1) - 1, xhi = max(x0, x1) + 1, ylo = min(y0, y1) - 1, yhi = max(y0, y1) + 1;
    const long long dx = x1 - x0, dy = y1 - y0, L = dx * dx + dy * dy;
#pragma unroll
    for (int i = 0; i < NPIX; ++i) {
      if (cx[i] < xlo || cx[i] > xhi || cy[i] < ylo || cy[i] > yhi) continue;
      const long long qx = cx[i] - x0, qy = cy[i] - y0, t = qx * dx + qy * dy;
      bool hit;
      if (t <= 0) {  // also L == 0
        hit = qx * qx + qy * qy <= 1;
      } else if (t >= L) {
        const long long rx = cx[i] - x1, ry = cy[i] - y1;
        hit = rx * rx + ry * ry <= 1;
      } else {
        const long long c = qx * dy - qy * dx;
        hit = c * c <= L;
      }
      if (hit) bits |= 1u << i;
    }
  }
  return bits;
}

// 16 bytes of RGB starting at byte c (0..2) of a pixel: six pixels, bit i of `bits` = pixel i is figure (0, 0, 255),
// otherwise white
__device__ __forceinline__ uint4 rs_pack(unsigned bits, unsigned c) {
  unsigned w[5] = {~0u, ~0u, ~0u, ~0u, ~0u};
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const unsigned on = 0u - ((bits >> i) & 1u);
#pragma unroll
    for (int b = 3 * i; b < 3 * i + 2; ++b) w[b >> 2] &= ~(on & (0xFFu << (8 * (b & 3))));
  }
  const unsigned s = 8 * c;
  uint4 r;
  r.x = (unsigned)((((unsigned long long)w[1] << 32) | w[0]) >> s);
  r.y = (unsigned)((((unsigned long long)w[2] << 32) | w[1]) >> s);
  r.z = (unsigned)((((unsigned long long)w[3] << 32) | w[2]) >> s);
  r.w = (unsigned)((((unsigned long long)w[4] << 32) | w[3]) >> s);
  return r;
}

__global__ void __launch_bounds__(256) m2d_render_sticks_kernel(const float* __restrict__ poses, long long n_frames,
                                                                int h, int w, unsigned char* __restrict__ out,
                                                                unsigned frame_bytes, unsigned spans_per_frame) {
  const int lane = threadIdx.x & 63;
  const long long g = (long long)blockIdx.x * RS_WAVES + (threadIdx.x >> 6);
  if (g >= n_frames * spans_per_frame) return;  // whole waves
  const long long f = g / spans_per_frame;
  const unsigned span = (unsigned)(g - f * spans_per_frame);

  // points: x' = fl32(x + w/2), y' = fl32(y + h/2); a midpoint is fl32(fl32(a' + b') * 0.5)
  float xs = 0.f, ys = 0.f;
  if (lane < RS_JOINTS) {
    const float* p = poses + f * (3 * RS_JOINTS) + 3 * lane;
    xs = p[0] + (float)(w / 2);
    ys = p[1] + (float)(h / 2);
  }
  const int ok = fabsf(xs) < RS_LIMIT && fabsf(ys) < RS_LIMIT;  // false for NaN and inf
  int a = lane, b = lane;
  if (lane >= RS_JOINTS && lane < RS_POINTS) a = kRsMid[lane - RS_JOINTS][0], b = kRsMid[lane - RS_JOINTS][1];
  const float xa = __shfl(xs, a), xb = __shfl(xs, b), ya = __shfl(ys, a), yb = __shfl(ys, b);
  const int oka = __shfl(ok, a), okb = __shfl(ok, b);
  const bool mid = lane >= RS_JOINTS;
  const float mx = mid ? (xa + xb) * 0.5f : xs, my = mid ? (ya + yb) * 0.5f : ys;
  const int pv = mid ? (oka & okb) : ok;
  const int ptx = pv ? (int)mx : 0, pty = pv ? (int)my : 0;  // C++ conversion truncates toward zero

  // primitives: lane k < 23 the disk at joint k, lane 23 + s segment s
  int pa = lane, pb = lane;
  if (lane >= RS_JOINTS && lane < RS_PRIMS) pa = kRsSeg[lane - RS_JOINTS][0], pb = kRsSeg[lane - RS_JOINTS][1];
  const int X0 = __shfl(ptx, pa), Y0 = __shfl(pty, pa), X1 = __shfl(ptx, pb), Y1 = __shfl(pty, pb);
  const int V = __shfl(pv, pa) & __shfl(pv, pb);
  const int r = lane < RS_JOINTS ? 4 : 1;
  const int ylo = min(Y0, Y1) - r, yhi = max(Y0, Y1) + r;
  const bool live = lane < RS_PRIMS && V && max(X0, X1) + r >= 0 && min(X0, X1) - r < w && yhi >= 0 && ylo < h;

  // the span [e0, e1) of the frame's bytes; [b0, b1) its 16-byte aligned body (empty when the span holds no aligned
  // 16 bytes; `back` may exceed e1 itself in frames of fewer than 16 bytes, so it is compared, never subtracted blindly)
  unsigned char* fb = out + f * (long long)frame_bytes;
  const unsigned e0 = span * RS_SPAN, e1 = min(e0 + RS_SPAN, frame_bytes);
  const unsigned b0 = min(e0 + (unsigned)((16 - ((uintptr_t)(fb + e0) & 15)) & 15), e1);
  const unsigned back = (unsigned)((uintptr_t)(fb + e1) & 15);
  const unsigned b1 = e1 - b0 >= back ? e1 - back : b0;

  for (unsigned step = b0; step < b1; step += RS_STEP) {
    const unsigned hi = min(step + RS_STEP, b1);
    const int rlo = (int)(step / 3 / (unsigned)w), rhi = (int)((hi - 1) / 3 / (unsigned)w);  // image rows
    const unsigned long long m = __ballot(live && ylo <= h - 1 - rlo && yhi >= h - 1 - rhi);
    const unsigned e = step + 16 * lane;
    uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);
    if (m) {
      const unsigned p0 = e / 3, c = e - 3 * p0;
      int row = (int)(p0 / (unsigned)w), col = (int)(p0 - (unsigned)row * w);
      int cx[6], cy[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        cx[i] = col, cy[i] = h - 1 - row;
        if (++col == w) col = 0, ++row;
      }
      const unsigned bits = rs_cover<6>(m, cx, cy, X0, Y0, X1, Y1);
      if (bits) v = rs_pack(bits, c);
    }
    if (e < hi) *reinterpret_cast<uint4*>(fb + e) = v;
  }

  if (b0 > e0 || e1 > b1) {  // head [e0, b0) on lanes 0..15, tail [b1, e1) on lanes 16..31: < 16 bytes each
    const unsigned e = lane < 16 ? e0 + lane : b1 + (lane - 16);
    const bool act = lane < 16 ? e < b0 : (lane < 32 && e < e1);
    const unsigned p = e / 3;
    const int row = (int)(p / (unsigned)w);
    const int cx[1] = {(int)(p - (unsigned)row * w)}, cy[1] = {h - 1 - row};
    const unsigned bits = rs_cover<1>(__ballot(live), cx, cy, X0, Y0, X1, Y1);
    if (act) fb[e] = (e - 3 * p == 2 || !bits) ? 255 : 0;
  }
}

}  // namespace

extern "C" {

int m2d_render_sticks(const float* poses, long n_frames, int height, int width, unsigned char* out, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (n_frames < 0 || height < 1 || height > 4096 || width < 1 || width > 4096)
    M2D_FAIL(M2D_ERR_ARG, "m2d_render_sticks: bad arguments (n_frames %ld, %d x %d)", n_frames, height, width);
  if (n_frames == 0) return M2D_OK;
  if (!poses || !out) M2D_FAIL(M2D_ERR_ARG, "m2d_render_sticks: null pointer");
  const unsigned frame_bytes = 3u * (unsigned)height * (unsigned)width;
  const unsigned spans = (frame_bytes + RS_SPAN - 1) / RS_SPAN;
  const long long blocks = m2d_ceil_div64((long long)n_frames * spans, RS_WAVES);
  if (blocks > 0x7fffffffLL)
    M2D_FAIL(M2D_ERR_RANGE, "m2d_render_sticks: %ld frames are too many for one launch", n_frames);
  M2dProfScope prof(M2D_FAM_POINTWISE, stream, 0.0, (double)n_frames * (frame_bytes + 8.0 * RS_JOINTS),
                    "render_sticks", height, width);
  hipLaunchKernelGGL(m2d_render_sticks_kernel, dim3((unsigned)blocks), dim3(64 * RS_WAVES), 0, stream, poses,
                     (long long)n_frames, height, width, out, frame_bytes, spans);
  M2D_CHECK_LAUNCH("m2d_render_sticks");
  return M2D_OK;
}

}  // extern "C"
