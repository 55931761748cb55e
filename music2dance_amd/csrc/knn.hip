// Exact nearest-neighbour queries between two sets of fp32 rows (metrics.py; include/m2d.h "nearest-neighbour queries";
// DESIGN.md section 15):
//   m2d_knn_radii    r2[i] = the k-th smallest squared distance of row i of X to the OTHER rows of X;
//   m2d_ball_query   per query row: how many reference rows hold it inside their radius, and its nearest reference row.
// d2(x, y) = sum_d (x_d - y_d)^2 in the direct-difference form: the difference in fp32, then one fmaf chain over d
// ascending from 0. (x - y) = -(y - x) exactly, so d2(x, y) and d2(y, x) are the same bits, and a pair's value depends on
// nothing but the two rows. Everything after the distances is selection (minimum, k smallest, integer counts): the
// results do not depend on tile shapes, on the split of the reference range or on the other queries of the call.
//
// One tile kernel serves both entry points. A workgroup of 256 threads owns 128 query rows, staged once in LDS, and walks
// reference tiles of 64 rows. Both tiles lie TRANSPOSED in LDS, [d][row], rows of the image 132 / 68 floats apart, D
// padded to a multiple of 4 with zeros (a zero lane adds fmaf(0, 0, acc) = acc exactly). Thread (tq, tr) = (tid / 16,
// tid % 16) holds the 8 x 4 accumulators of queries 8 tq .. 8 tq + 7 against references 4 tr .. 4 tr + 3: per d it reads
// two 16-byte words of the query image (the 16 lanes of a ds_read_b128 group see two addresses 32 bytes apart: a
// broadcast) and one of the reference image (16 lanes x 16 bytes = 256 consecutive bytes, the 64 banks once), and issues
// 32 subtractions and 32 fmas, written on float2 so that the compiler emits v_pk_add_f32 / v_pk_fma_f32 over the pairs
// of references: 32 VALU instructions for 3 LDS reads, the kernel is VALU-bound. The next reference tile is fetched
// into registers (at most 32 a thread) before the current one is computed and stored to LDS after it; a wave reads 16
// consecutive floats of 4 rows per instruction and stores them to banks 4 c + r, a 2-way conflict, which a ds_write_b32
// does not pay for.
//
// Selection. Radii: a thread keeps, per query, the M2D_KNN_MAX_K smallest distances it has met as a sorted list in
// registers; a candidate below the list's last entry is inserted by a fully unrolled compare-and-shift (no loop whose
// bound comes from the data: a NaN compares false and is never inserted). The lists of the 16 lanes that share a query
// are merged by a 4-step butterfly (lane ^ 1, 2, 4, 8), always in that order. Ball query: per query a count of the
// references i with d2 <= r2[i], the minimum and the smallest index that attains it (strict < while the indices ascend;
// (d2, index) lexicographic between lanes).
//
// Both regimes fill the chip: the grid is (query tiles, S), split s walks reference tiles [s tps, (s + 1) tps) and
// writes its partial result into the workspace; S is chosen from the shape alone so that about 512 workgroups exist. A
// second launch merges the S partials of a query in ascending s. No atomics anywhere.
//
// Non-finite inputs: no loop or exit depends on the data, so they cannot hang; what they give is unspecified (a NaN
// distance is never counted, never a minimum, never in a list).
#include "m2d_common.h"

#include <math.h>

#define M2D_KNN_MAX_K 10
#define M2D_KNN_MAX_D 128
#define M2D_KNN_THREADS 256
#define M2D_KNN_TQ 128                     // query rows of a workgroup
#define M2D_KNN_TR 64                      // reference rows of a tile
#define M2D_KNN_QLD (M2D_KNN_TQ + 4)       // floats between two d-rows of the query image (16-byte multiple)
#define M2D_KNN_RLD (M2D_KNN_TR + 4)
#define M2D_KNN_PF 32                      // registers of the reference prefetch: (128 / 16) * 16 * 64 / 256
#define M2D_KNN_TARGET_WGS 512             // workgroups wanted on the chip (256 CUs, two resident each at D = 69)
#define M2D_KNN_MAX_SPLIT 512
#define M2D_KNN_MAX_ROWS 0x7fffff00        // row indices (and the tile arithmetic on them) stay inside an int

namespace {

typedef float knn_f2 __attribute__((ext_vector_type(2)));

enum { KNN_RADII = 0, KNN_NEAREST = 1, KNN_BALL = 2 };

// v into the ascending list, the largest entry drops out; the caller has checked v < list[last]
__device__ __forceinline__ void knn_insert(float (&list)[M2D_KNN_MAX_K], float v) {
#pragma unroll
  for (int i = 0; i < M2D_KNN_MAX_K; ++i) {
    const float a = list[i];
    const bool lt = v < a;
    list[i] = lt ? v : a;
    v = lt ? a : v;
  }
}

// MODE KNN_RADII:   Q == P (the set against itself, pair (i, i) skipped by index) -> part_f (S, M, MAX_K) sorted lists
// MODE KNN_NEAREST: -> part_f (S, M) minimum, part_i (S, M) its smallest index
// MODE KNN_BALL:    the same and part_c (S, M) = #{i : d2 <= r2[i]}
template <int MODE>
__global__ void __launch_bounds__(M2D_KNN_THREADS)
m2d_knn_tile_kernel(const float* __restrict__ Q, long long ldq, int M, const float* __restrict__ P, long long ldp, int N,
                    int D, int Dp, int tps, int rtiles, const float* __restrict__ r2, float* __restrict__ part_f,
                    int* __restrict__ part_i, int* __restrict__ part_c) {
  extern __shared__ __attribute__((aligned(16))) float knn_lds[];
  float* Qs = knn_lds;                               // [Dp][QLD]
  float* Ps = Qs + (size_t)Dp * M2D_KNN_QLD;         // [Dp][RLD]
  float* Rs = Ps + (size_t)Dp * M2D_KNN_RLD;         // [TR] radii of the tile (KNN_BALL)
  const int tid = threadIdx.x;
  const int tq = tid >> 4, tr = tid & 15;
  const int q0 = blockIdx.x * M2D_KNN_TQ;
  const int t_begin = blockIdx.y * tps;
  const int t_end = t_begin + tps < rtiles ? t_begin + tps : rtiles;   // the launcher leaves no split empty
  const int c_lo = tid & 15, r_lo = tid >> 4;        // staging: a wave takes 16 consecutive floats of 4 rows

  // the query tile, once
  for (int c0 = 0; c0 < Dp; c0 += 16) {
    const int c = c0 + c_lo;
#pragma unroll
    for (int u = 0; u < M2D_KNN_TQ / 16; ++u) {
      const int r = u * 16 + r_lo;
      if (c < Dp) Qs[c * M2D_KNN_QLD + r] = (c < D && q0 + r < M) ? Q[(size_t)(q0 + r) * ldq + c] : 0.f;
    }
  }

  float pf[M2D_KNN_PF];
  float rpf = 0.f;
  // slot u of the prefetch: columns 16 (u / 4) .., rows 16 (u % 4) .. of the tile
  auto fetch = [&](int t) {
    const int r0 = t * M2D_KNN_TR;
#pragma unroll
    for (int u = 0; u < M2D_KNN_PF; ++u) {
      const int c = (u >> 2) * 16 + c_lo, r = (u & 3) * 16 + r_lo;
      pf[u] = (c < D && r0 + r < N) ? P[(size_t)(r0 + r) * ldp + c] : 0.f;
    }
    if (MODE == KNN_BALL) rpf = (tid < M2D_KNN_TR && r0 + tid < N) ? r2[r0 + tid] : 0.f;
  };
  auto stage = [&]() {
#pragma unroll
    for (int u = 0; u < M2D_KNN_PF; ++u) {
      const int c = (u >> 2) * 16 + c_lo, r = (u & 3) * 16 + r_lo;
      if (c < Dp) Ps[c * M2D_KNN_RLD + r] = pf[u];
    }
    if (MODE == KNN_BALL && tid < M2D_KNN_TR) Rs[tid] = rpf;
  };

  float list[MODE == KNN_RADII ? 8 : 1][M2D_KNN_MAX_K];
  float best[8];
  int bidx[8], cnt[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    best[q] = INFINITY, bidx[q] = 0x7fffffff, cnt[q] = 0;
    if (MODE == KNN_RADII) {
#pragma unroll
      for (int i = 0; i < M2D_KNN_MAX_K; ++i) list[q][i] = INFINITY;
    }
  }

  fetch(t_begin);
  for (int t = t_begin; t < t_end; ++t) {            // (bounds from the shape alone)
    __syncthreads();                                 // the previous tile has been read by every wave
    stage();
    __syncthreads();
    if (t + 1 < t_end) fetch(t + 1);

    knn_f2 acc[8][2];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q][0] = acc[q][1] = (knn_f2){0.f, 0.f};
    const float* qp = Qs + tq * 8;
    const float* pp = Ps + tr * 4;
    // the three reads of d + 1 are issued before the arithmetic of d (the last step re-reads its own row): their
    // latency hides behind 32 VALU instructions instead of standing in front of them
    float4 nqa = *reinterpret_cast<const float4*>(qp);
    float4 nqb = *reinterpret_cast<const float4*>(qp + 4);
    float4 npv = *reinterpret_cast<const float4*>(pp);
#pragma unroll 4
    for (int d = 0; d < Dp; ++d) {
      const float4 qa = nqa, qb = nqb, pv = npv;
      const int dn = d + 1 < Dp ? d + 1 : d;
      nqa = *reinterpret_cast<const float4*>(qp + dn * M2D_KNN_QLD);
      nqb = *reinterpret_cast<const float4*>(qp + dn * M2D_KNN_QLD + 4);
      npv = *reinterpret_cast<const float4*>(pp + dn * M2D_KNN_RLD);
      const float qv[8] = {qa.x, qa.y, qa.z, qa.w, qb.x, qb.y, qb.z, qb.w};
      const knn_f2 p01 = {pv.x, pv.y}, p23 = {pv.z, pv.w};
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const knn_f2 qq = {qv[q], qv[q]};
        const knn_f2 d01 = qq - p01, d23 = qq - p23;
        acc[q][0] = __builtin_elementwise_fma(d01, d01, acc[q][0]);
        acc[q][1] = __builtin_elementwise_fma(d23, d23, acc[q][1]);
      }
    }

    const int gr0 = t * M2D_KNN_TR + tr * 4;
    float rr[4] = {0.f, 0.f, 0.f, 0.f};
    if (MODE == KNN_BALL) {
      const float4 rv = *reinterpret_cast<const float4*>(Rs + tr * 4);
      rr[0] = rv.x, rr[1] = rv.y, rr[2] = rv.z, rr[3] = rv.w;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int gq = q0 + tq * 8 + q;
      const float v4[4] = {acc[q][0].x, acc[q][0].y, acc[q][1].x, acc[q][1].y};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int gr = gr0 + j;
        const float v = v4[j];
        if (MODE == KNN_RADII) {
          if (gr < N && gr != gq && v < list[q][M2D_KNN_MAX_K - 1]) knn_insert(list[q], v);
        } else {
          const bool in = gr < N;
          if (MODE == KNN_BALL) cnt[q] += (in && v <= rr[j]) ? 1 : 0;
          const bool lt = in && v < best[q];         // indices ascend along a thread's walk: the first minimum stays
          best[q] = lt ? v : best[q];
          bidx[q] = lt ? gr : bidx[q];
        }
      }
    }
  }

  // the 16 lanes of a query: lanes 16 (tq % 4) .. + 15 of the wave, butterfly over lane ^ 1, 2, 4, 8
#pragma unroll
  for (int q = 0; q < 8; ++q) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) {
      if (MODE == KNN_RADII) {
        float other[M2D_KNN_MAX_K];
#pragma unroll
        for (int i = 0; i < M2D_KNN_MAX_K; ++i) other[i] = __shfl_xor(list[q][i], m);
#pragma unroll
        for (int i = 0; i < M2D_KNN_MAX_K; ++i)
          if (other[i] < list[q][M2D_KNN_MAX_K - 1]) knn_insert(list[q], other[i]);
      } else {
        const float ob = __shfl_xor(best[q], m);
        const int oi = __shfl_xor(bidx[q], m);
        const bool lt = ob < best[q] || (ob == best[q] && oi < bidx[q]);
        best[q] = lt ? ob : best[q];
        bidx[q] = lt ? oi : bidx[q];
        if (MODE == KNN_BALL) cnt[q] += __shfl_xor(cnt[q], m);
      }
    }
    const int gq = q0 + tq * 8 + q;
    if (tr == 0 && gq < M) {
      const size_t row = (size_t)blockIdx.y * M + gq;
      if (MODE == KNN_RADII) {
#pragma unroll
        for (int i = 0; i < M2D_KNN_MAX_K; ++i) part_f[row * M2D_KNN_MAX_K + i] = list[q][i];
      } else {
        part_f[row] = best[q];
        part_i[row] = bidx[q];
        if (MODE == KNN_BALL) part_c[row] = cnt[q];
      }
    }
  }
}

// the S partial lists of a row, merged in ascending s -> its k-th smallest
__global__ void __launch_bounds__(M2D_KNN_THREADS)
m2d_knn_radii_merge_kernel(const float* __restrict__ part, int N, int S, int k, float* __restrict__ r2) {
  const int i = blockIdx.x * M2D_KNN_THREADS + threadIdx.x;
  if (i >= N) return;
  float list[M2D_KNN_MAX_K];
#pragma unroll
  for (int j = 0; j < M2D_KNN_MAX_K; ++j) list[j] = INFINITY;
  for (int s = 0; s < S; ++s) {
    const float* src = part + ((size_t)s * N + i) * M2D_KNN_MAX_K;
#pragma unroll
    for (int j = 0; j < M2D_KNN_MAX_K; ++j) {
      const float v = src[j];
      if (v < list[M2D_KNN_MAX_K - 1]) knn_insert(list, v);
    }
  }
  float out = list[0];
#pragma unroll
  for (int j = 1; j < M2D_KNN_MAX_K; ++j) out = (j == k - 1) ? list[j] : out;
  r2[i] = out;
}

// the S partials of a query in ascending s (= ascending reference index): strict < keeps the smallest index
__global__ void __launch_bounds__(M2D_KNN_THREADS)
m2d_ball_merge_kernel(const float* __restrict__ part_f, const int* __restrict__ part_i, const int* __restrict__ part_c,
                      int M, int N, int S, int* __restrict__ count, float* __restrict__ nn_d2, int* __restrict__ nn_idx) {
  const int j = blockIdx.x * M2D_KNN_THREADS + threadIdx.x;
  if (j >= M) return;
  float best = INFINITY;
  int bidx = 0x7fffffff, cnt = 0;
  for (int s = 0; s < S; ++s) {
    const size_t row = (size_t)s * M + j;
    const float v = part_f[row];
    const int vi = part_i[row];
    if (part_c) cnt += part_c[row];
    const bool lt = v < best;
    best = lt ? v : best;
    bidx = lt ? vi : bidx;
  }
  nn_d2[j] = best;
  nn_idx[j] = (bidx >= 0 && bidx < N) ? bidx : 0;    // (no distance below +inf: non-finite input, unspecified)
  if (count) count[j] = cnt;
}

// a pointer the device can be handed: known to the runtime and not host memory (as distrib.hip's check)
bool knn_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type != hipMemoryTypeHost && at.type != hipMemoryTypeUnregistered;
}

struct KnnPlan {
  int qtiles, rtiles, tps, S;
};

// a function of the two row counts alone: about M2D_KNN_TARGET_WGS workgroups, no empty split
KnnPlan knn_plan(int M, int N) {
  KnnPlan p;
  p.qtiles = m2d_ceil_div(M, M2D_KNN_TQ);
  p.rtiles = m2d_ceil_div(N, M2D_KNN_TR);
  int want = m2d_ceil_div(M2D_KNN_TARGET_WGS, p.qtiles);
  if (want > M2D_KNN_MAX_SPLIT) want = M2D_KNN_MAX_SPLIT;
  if (want > p.rtiles) want = p.rtiles;
  p.tps = m2d_ceil_div(p.rtiles, want);
  p.S = m2d_ceil_div(p.rtiles, p.tps);
  return p;
}

bool knn_rows_ok(int n) { return n > 0 && n <= M2D_KNN_MAX_ROWS; }

template <int MODE>
int knn_launch_tiles(const char* what, const float* Q, long long ldq, int M, const float* P, long long ldp, int N, int D,
                     const KnnPlan& p, const float* r2, float* part_f, int* part_i, int* part_c, hipStream_t stream) {
  const int Dp = (D + 3) & ~3;
  const size_t lds = ((size_t)Dp * (M2D_KNN_QLD + M2D_KNN_RLD) + M2D_KNN_TR) * sizeof(float);
  static bool attr_set = false;
  if (!attr_set) {
    const size_t lds_max = ((size_t)M2D_KNN_MAX_D * (M2D_KNN_QLD + M2D_KNN_RLD) + M2D_KNN_TR) * sizeof(float);
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&m2d_knn_tile_kernel<MODE>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max) != hipSuccess)
      M2D_FAIL(M2D_ERR_HIP, "%s: cannot raise the dynamic LDS limit", what);
    attr_set = true;
  }
  hipLaunchKernelGGL(m2d_knn_tile_kernel<MODE>, dim3((unsigned)p.qtiles, (unsigned)p.S), dim3(M2D_KNN_THREADS), lds,
                     stream, Q, ldq, M, P, ldp, N, D, Dp, p.tps, p.rtiles, r2, part_f, part_i, part_c);
  M2D_CHECK_LAUNCH(what);
  return M2D_OK;
}

}  // namespace

extern "C" {

int m2d_knn_max_k(void) { return M2D_KNN_MAX_K; }

size_t m2d_knn_radii_workspace_bytes(int N, int k) {
  if (!knn_rows_ok(N) || k < 1 || k > M2D_KNN_MAX_K) return 0;
  const KnnPlan p = knn_plan(N, N);
  return (size_t)p.S * N * M2D_KNN_MAX_K * sizeof(float);
}

int m2d_knn_radii(const float* X, long long ldx, int N, int D, int k, float* r2, void* ws, size_t ws_bytes,
                  void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (k < 1 || k > M2D_KNN_MAX_K) M2D_FAIL(M2D_ERR_ARG, "m2d_knn_radii: k must be in [1, %d] (got %d)", M2D_KNN_MAX_K, k);
  if (N <= k) M2D_FAIL(M2D_ERR_ARG, "m2d_knn_radii: at least k + 1 = %d rows are needed (got %d)", k + 1, N);
  if (!knn_rows_ok(N)) M2D_FAIL(M2D_ERR_ARG, "m2d_knn_radii: too many rows");
  if (D <= 0 || D > M2D_KNN_MAX_D) M2D_FAIL(M2D_ERR_ARG, "m2d_knn_radii: D must be in [1, %d] (got %d)", M2D_KNN_MAX_D, D);
  if (ldx < D) M2D_FAIL(M2D_ERR_ARG, "m2d_knn_radii: row stride below D");
  if (!knn_device_ptr(X) || !knn_device_ptr(r2)) M2D_FAIL(M2D_ERR_ARG, "m2d_knn_radii: null or host pointer");
  const size_t need = m2d_knn_radii_workspace_bytes(N, k);
  if (!ws || ws_bytes < need) M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_knn_radii: workspace of %zu bytes needed", need);
  const KnnPlan p = knn_plan(N, N);
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 3.0 * (double)N * N * D, 4.0 * (double)p.qtiles * N * D, "knn_radii", N, D, k);
  const int rc = knn_launch_tiles<KNN_RADII>("m2d_knn_radii", X, ldx, N, X, ldx, N, D, p, nullptr, (float*)ws, nullptr,
                                             nullptr, stream);
  if (rc != M2D_OK) return rc;
  hipLaunchKernelGGL(m2d_knn_radii_merge_kernel, dim3((unsigned)m2d_ceil_div(N, M2D_KNN_THREADS)),
                     dim3(M2D_KNN_THREADS), 0, stream, (const float*)ws, N, p.S, k, r2);
  M2D_CHECK_LAUNCH("m2d_knn_radii");
  return M2D_OK;
}

size_t m2d_ball_query_workspace_bytes(int M, int N) {
  if (!knn_rows_ok(M) || !knn_rows_ok(N)) return 0;
  const KnnPlan p = knn_plan(M, N);
  return (size_t)p.S * M * 3 * sizeof(float);
}

int m2d_ball_query(const float* Q, long long ldq, int M, const float* P, long long ldp, int N, int D, const float* r2,
                   int* count, float* nn_d2, int* nn_idx, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!knn_rows_ok(M) || !knn_rows_ok(N)) M2D_FAIL(M2D_ERR_ARG, "m2d_ball_query: M and N must be in [1, %d]", M2D_KNN_MAX_ROWS);
  if (D <= 0 || D > M2D_KNN_MAX_D) M2D_FAIL(M2D_ERR_ARG, "m2d_ball_query: D must be in [1, %d] (got %d)", M2D_KNN_MAX_D, D);
  if (ldq < D || ldp < D) M2D_FAIL(M2D_ERR_ARG, "m2d_ball_query: row stride below D");
  if ((r2 == nullptr) != (count == nullptr)) M2D_FAIL(M2D_ERR_ARG, "m2d_ball_query: r2 and count go together");
  if (!knn_device_ptr(Q) || !knn_device_ptr(P) || !knn_device_ptr(nn_d2) || !knn_device_ptr(nn_idx) ||
      (r2 && (!knn_device_ptr(r2) || !knn_device_ptr(count))))
    M2D_FAIL(M2D_ERR_ARG, "m2d_ball_query: null or host pointer");
  const size_t need = m2d_ball_query_workspace_bytes(M, N);
  if (!ws || ws_bytes < need) M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_ball_query: workspace of %zu bytes needed", need);
  const KnnPlan p = knn_plan(M, N);
  const size_t sm = (size_t)p.S * M;
  float* part_f = (float*)ws;
  int* part_i = (int*)ws + sm;
  int* part_c = r2 ? (int*)ws + 2 * sm : nullptr;
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 3.0 * (double)M * N * D, 4.0 * ((double)p.qtiles * N + M) * D, "ball_query", M,
                    N, D);
  const int rc = r2 ? knn_launch_tiles<KNN_BALL>("m2d_ball_query", Q, ldq, M, P, ldp, N, D, p, r2, part_f, part_i, part_c,
                                                 stream)
                    : knn_launch_tiles<KNN_NEAREST>("m2d_ball_query", Q, ldq, M, P, ldp, N, D, p, nullptr, part_f, part_i,
                                                    nullptr, stream);
  if (rc != M2D_OK) return rc;
  hipLaunchKernelGGL(m2d_ball_merge_kernel, dim3((unsigned)m2d_ceil_div(M, M2D_KNN_THREADS)), dim3(M2D_KNN_THREADS), 0,
                     stream, (const float*)part_f, (const int*)part_i, (const int*)part_c, M, N, p.S, count, nn_d2,
                     nn_idx);
  M2D_CHECK_LAUNCH("m2d_ball_query");
  return M2D_OK;
}

}  // extern "C"
