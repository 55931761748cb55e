// Distribution scores of a set of dances (metrics.py; include/m2d.h "distribution scores"):
//   m2d_kinetic_features    per-joint kinetic features of a dance (horizontal / vertical kinetic energy, energy expenditure);
//   m2d_feature_moments     fp64 mean and unbiased covariance of a set of fp32 feature rows;
//   m2d_sym_eig             eigenvalues (and vectors) of a batch of symmetric fp64 matrices, D <= 128: cyclic Jacobi;
//   m2d_frechet             Frechet distance of pairs of Gaussians given by their moments;
//   m2d_pairwise_mean_dist  mean pairwise Euclidean distance inside groups of rows (diversity, multimodality).
// Everything past the fp32 differences is plain fp64 arithmetic (v_fma_f64 / v_mul_f64 / v_add_f64, no MFMA: the largest
// product here is 128^3) and every sum has a fixed order: no atomics, bit-identical results from run to run.
//
// m2d_sym_eig. Two-sided cyclic Jacobi, one workgroup of 1024 threads per matrix. The matrix (padded by a zero row and
// column to an even order n when D is odd) lives in LDS for the whole solve, rows n + 1 doubles apart: 128 x 129 x 8 =
// 132 096 bytes of the CU's 160 KiB; the accumulated rotations V^T (only when the caller wants vectors) stay in global memory,
// where a 128 KiB matrix is L2-resident and every access is a coalesced row. A sweep is n - 1 steps of a round-robin
// tournament: step s pairs (n - 1, s) and ((s + k) mod (n - 1), (s - k) mod (n - 1)) for k = 1 .. n / 2 - 1, n / 2
// disjoint pairs that cover every index. A step is two phases with one barrier each:
//   1. thread k < n / 2 forms the rotation (c, s, t) that annihilates a[p][q] of its pair (Rutishauser's formulas) and adds
//      a[p][q]^2 to its own register;
//   2. the matrix is cut into (n / 2)^2 blocks of 2 x 2, block (k, l) = rows of pair k x columns of pair l; the blocks are
//      disjoint, block (k, l) becomes J_k^T B J_l with no other block read: one phase updates rows and columns at once.
//      A diagonal block becomes diag(a_pp - t a_pq, a_qq + t a_pq) exactly. The same phase rotates rows p, q of V^T.
// After a sweep the n / 2 registers are added in LDS in ascending k; the solve has converged when twice that sum - the
// squared off-diagonal norm the sweep met - is at most (2^-50 ||A||_F)^2. The sweep loop runs at most M2D_EIG_SWEEPS (30)
// times whatever the data: a NaN compares false, such a matrix runs to the cap and comes out as NaN with converged = 0.
#include "m2d_common.h"
#include "m2d_reduce.h"

#include <math.h>

#define M2D_EIG_MAX_D 128
#define M2D_EIG_LD (M2D_EIG_MAX_D + 1)
#define M2D_EIG_THREADS 1024
#define M2D_EIG_SWEEPS 30
#define M2D_DS_THREADS 256
#define M2D_DBL_MAX 1.79769313486231570e308

namespace {

// ---- m2d_kinetic_features: one workgroup per (dance, joint) ----------------------------------------------------------
__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_kinetic_kernel(const float* __restrict__ poses, int T, int J, double fps, int up, float* __restrict__ F) {
  __shared__ double red[M2D_DS_THREADS];
  const int b = blockIdx.x / J, j = blockIdx.x - b * J;
  const int o1 = up == 0 ? 1 : 0, o2 = up == 2 ? 1 : 2;       // the two horizontal axes, ascending
  const size_t st = (size_t)J * 3;
  const float* p = poses + (size_t)b * T * st + (size_t)j * 3;
  double h = 0.0, v = 0.0, e = 0.0;
  for (int t = 1 + threadIdx.x; t < T; t += M2D_DS_THREADS) {
    const float* c = p + (size_t)t * st;
    float d0[3], d1[3];
    for (int a = 0; a < 3; ++a) d0[a] = c[a] - c[(ptrdiff_t)a - (ptrdiff_t)st];            // fp32 differences
    const double v1 = (double)d0[o1] * fps, v2 = (double)d0[o2] * fps, vu = (double)d0[up] * fps;
    h += v1 * v1 + v2 * v2;
    v += vu * vu;
    if (t + 1 < T) {
      for (int a = 0; a < 3; ++a) d1[a] = c[st + a] - c[a];
      const double f2 = fps * fps;
      const double a1 = (double)(d1[o1] - d0[o1]) * f2, a2 = (double)(d1[o2] - d0[o2]) * f2,
                   au = (double)(d1[up] - d0[up]) * f2;
      e += sqrt((a1 * a1 + a2 * a2) + au * au);
    }
  }
  h = m2d_block_sum<M2D_DS_THREADS>(h, red);
  v = m2d_block_sum<M2D_DS_THREADS>(v, red);
  e = m2d_block_sum<M2D_DS_THREADS>(e, red);
  if (threadIdx.x == 0) {
    float* out = F + (size_t)b * 3 * J;
    out[j] = (float)(h / (double)(T - 1));
    out[J + j] = (float)(v / (double)(T - 1));
    out[2 * J + j] = (float)(e / (double)(T - 2));
  }
}

// ---- m2d_feature_moments -------------------------------------------------------------------------------------------
// mean: one workgroup per column; thread i adds rows i, i + 256, .. in ascending order, then the tree
__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_moments_mean_kernel(const float* __restrict__ X, long long ldx, int N, double* __restrict__ mean) {
  __shared__ double red[M2D_DS_THREADS];
  const int d = blockIdx.x;
  double acc = 0.0;
  for (int n = threadIdx.x; n < N; n += M2D_DS_THREADS) acc += (double)X[(size_t)n * ldx + d];
  acc = m2d_block_sum<M2D_DS_THREADS>(acc, red);
  if (threadIdx.x == 0) mean[d] = acc / (double)N;
}

// cov: a workgroup owns a 16 x 16 tile of the matrix; 64 centred rows of both column blocks are staged in LDS at a time,
// thread (i, j) adds its products in ascending row order. (x_i - m_i)(x_j - m_j) commutes, so cov is exactly symmetric.
__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_moments_cov_kernel(const float* __restrict__ X, long long ldx, int N, int D, const double* __restrict__ mean,
                       double* __restrict__ cov) {
  __shared__ double a[64][17], bt[64][17];
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
  const int i0 = blockIdx.y * 16, j0 = blockIdx.x * 16;
  double acc = 0.0;
  for (int n0 = 0; n0 < N; n0 += 64) {
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 16; e += M2D_DS_THREADS) {
      const int r = e >> 4, c = e & 15, n = n0 + r;
      const bool in = n < N;
      a[r][c] = (in && i0 + c < D) ? (double)X[(size_t)n * ldx + i0 + c] - mean[i0 + c] : 0.0;
      bt[r][c] = (in && j0 + c < D) ? (double)X[(size_t)n * ldx + j0 + c] - mean[j0 + c] : 0.0;
    }
    __syncthreads();
    const int nr = N - n0 < 64 ? N - n0 : 64;
    for (int r = 0; r < nr; ++r) acc = fma(a[r][ti], bt[r][tj], acc);
  }
  if (i0 + ti < D && j0 + tj < D) cov[(size_t)(i0 + ti) * D + j0 + tj] = acc / (double)(N - 1);
}

// ---- m2d_sym_eig ---------------------------------------------------------------------------------------------------
struct EigShared {
  double a[M2D_EIG_MAX_D * M2D_EIG_LD];
  double red[M2D_EIG_THREADS];
  double c[M2D_EIG_MAX_D / 2], s[M2D_EIG_MAX_D / 2], t[M2D_EIG_MAX_D / 2];
  int p[M2D_EIG_MAX_D / 2], q[M2D_EIG_MAX_D / 2];
  int flag;
};

// A (P, D, D) -> w (P, D) ascending, vecs (P, D, D) columns (or null), info (P, 2) doubles [sweeps, converged];
// vt: (P, n, n) scratch for V^T when vecs is wanted
__global__ void __launch_bounds__(M2D_EIG_THREADS)
m2d_sym_eig_kernel(const double* __restrict__ A, int D, double* __restrict__ w, double* __restrict__ vecs,
                   double* __restrict__ vt, double* __restrict__ info) {
  __shared__ EigShared sh;
  const int tid = threadIdx.x;
  const int n = D + (D & 1), half = n >> 1, m = n - 1;
  const double* Ag = A + (size_t)blockIdx.x * D * D;
  double* V = vecs ? vt + (size_t)blockIdx.x * n * n : nullptr;

  double fro = 0.0;
  for (int e = tid; e < n * n; e += M2D_EIG_THREADS) {
    const int r = e / n, c = e - r * n;
    const double x = (r < D && c < D) ? Ag[(size_t)r * D + c] : 0.0;
    sh.a[r * M2D_EIG_LD + c] = x;
    fro += x * x;
    if (V) V[e] = r == c ? 1.0 : 0.0;
  }
  fro = m2d_block_sum<M2D_EIG_THREADS>(fro, sh.red);
  const double tol2 = fro * (0x1p-50 * 0x1p-50);

  int sweeps = 0, converged = 0;
  for (int sweep = 0; sweep < M2D_EIG_SWEEPS; ++sweep) {     // the cap: no exit of this loop depends on the data alone
    double off = 0.0;
    for (int step = 0; step < m; ++step) {
      if (tid < half) {
        int p, q;
        if (tid == 0) {
          p = step, q = m;
        } else {
          p = (step + tid) % m, q = (step - tid + m) % m;
        }
        const double app = sh.a[p * M2D_EIG_LD + p], aqq = sh.a[q * M2D_EIG_LD + q], apq = sh.a[p * M2D_EIG_LD + q];
        double c = 1.0, s = 0.0, t = 0.0;
        if (apq != 0.0) {                                    // (a NaN is != 0 and makes NaN rotations)
          const double tau = (aqq - app) / (2.0 * apq);
          t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
          c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
        }
        off += apq * apq;
        sh.p[tid] = p, sh.q[tid] = q, sh.c[tid] = c, sh.s[tid] = s, sh.t[tid] = t;
      }
      __syncthreads();
      for (int e = tid; e < half * half; e += M2D_EIG_THREADS) {
        const int k = e / half, l = e - k * half;
        const int p = sh.p[k], q = sh.q[k], u = sh.p[l], v = sh.q[l];
        double* rp = sh.a + p * M2D_EIG_LD;
        double* rq = sh.a + q * M2D_EIG_LD;
        if (k == l) {
          const double d = sh.t[k] * rp[q];
          rp[p] -= d, rq[q] += d;
          rp[q] = 0.0, rq[p] = 0.0;
        } else {
          const double ck = sh.c[k], sk = sh.s[k], cl = sh.c[l], sl = sh.s[l];
          const double b00 = rp[u], b01 = rp[v], b10 = rq[u], b11 = rq[v];
          const double t00 = b00 * cl - b01 * sl, t01 = b00 * sl + b01 * cl;
          const double t10 = b10 * cl - b11 * sl, t11 = b10 * sl + b11 * cl;
          rp[u] = ck * t00 - sk * t10, rp[v] = ck * t01 - sk * t11;
          rq[u] = sk * t00 + ck * t10, rq[v] = sk * t01 + ck * t11;
        }
      }
      if (V) {
        for (int e = tid; e < half * n; e += M2D_EIG_THREADS) {
          const int k = e / n, r = e - k * n;
          double* vp = V + (size_t)sh.p[k] * n + r;
          double* vq = V + (size_t)sh.q[k] * n + r;
          const double c = sh.c[k], s = sh.s[k], x = *vp, y = *vq;
          *vp = c * x - s * y, *vq = s * x + c * y;
        }
      }
      __syncthreads();
    }
    // the squared off-diagonal norm this sweep met, added in ascending pair order
    if (tid < half) sh.red[tid] = off;
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int k = 0; k < half; ++k) tot += sh.red[k];
      sh.flag = (2.0 * tot <= tol2 && fro <= M2D_DBL_MAX) ? 1 : 0;   // false for a NaN or an infinity anywhere
    }
    __syncthreads();
    sweeps = sweep + 1;
    converged = sh.flag;
    __syncthreads();
    if (converged) break;
  }

  // ascending order by rank; a matrix that did not come out finite is NaN throughout
  if (tid == 0) sh.flag = 0;
  __syncthreads();
  if (tid < D) {
    const double x = sh.a[tid * M2D_EIG_LD + tid];
    sh.red[tid] = x;
    if (!(fabs(x) <= M2D_DBL_MAX)) sh.flag = 1;              // (every writer stores the same value)
  }
  __syncthreads();
  const int bad = sh.flag;
  if (bad) converged = 0;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (tid < D) {
    const double x = sh.red[tid];
    int rank = 0;
    for (int j = 0; j < D; ++j) {
      const double y = sh.red[j];
      rank += (y < x || (y == x && j < tid)) ? 1 : 0;
    }
    w[(size_t)blockIdx.x * D + (bad ? tid : rank)] = bad ? nan : x;
    sh.red[M2D_EIG_MAX_D + tid] = (double)rank;
  }
  __syncthreads();
  if (vecs) {
    double* out = vecs + (size_t)blockIdx.x * D * D;
    for (int e = tid; e < D * D; e += M2D_EIG_THREADS) {
      const int i = e / D, r = e - i * D;                    // eigenvector i (a row of V^T), component r
      const int col = bad ? i : (int)sh.red[M2D_EIG_MAX_D + i];
      out[(size_t)r * D + col] = bad ? nan : V[(size_t)i * n + r];
    }
  }
  if (tid == 0) {
    info[2 * blockIdx.x] = (double)sweeps;
    info[2 * blockIdx.x + 1] = (double)converged;
  }
}

// ---- m2d_frechet ---------------------------------------------------------------------------------------------------
// Tm = S2 V (V: eigenvectors of S1 as columns)
__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_frechet_sv_kernel(const double* __restrict__ S2, const double* __restrict__ V, int D, double* __restrict__ Tm) {
  const size_t base = (size_t)blockIdx.y * D * D;
  const int e = blockIdx.x * M2D_DS_THREADS + threadIdx.x;
  if (e >= D * D) return;
  const int i = e / D, j = e - i * D;
  double acc = 0.0;
  for (int k = 0; k < D; ++k) acc = fma(S2[base + (size_t)i * D + k], V[base + (size_t)k * D + j], acc);
  Tm[base + e] = acc;
}

// M = L^1/2 (V^T Tm) L^1/2 for i <= j, mirrored: exactly symmetric. L = max(w1, 0).
__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_frechet_vtv_kernel(const double* __restrict__ V, const double* __restrict__ Tm, const double* __restrict__ w1, int D,
                       double* __restrict__ M) {
  const size_t base = (size_t)blockIdx.y * D * D;
  const int e = blockIdx.x * M2D_DS_THREADS + threadIdx.x;
  if (e >= D * D) return;
  const int i = e / D, j = e - i * D;
  if (i > j) return;
  double acc = 0.0;
  for (int k = 0; k < D; ++k) acc = fma(V[base + (size_t)k * D + i], Tm[base + (size_t)k * D + j], acc);
  const double li = w1[(size_t)blockIdx.y * D + i], lj = w1[(size_t)blockIdx.y * D + j];
  // (x > 0 ? x : 0 would drop a NaN; this form hands it on)
  const double si = sqrt(li < 0.0 ? 0.0 : li), sj = sqrt(lj < 0.0 ? 0.0 : lj);
  const double val = (si * sj) * acc;
  M[base + (size_t)i * D + j] = val;
  M[base + (size_t)j * D + i] = val;
}

__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_frechet_final_kernel(const double* __restrict__ mean1, const double* __restrict__ cov1,
                         const double* __restrict__ mean2, const double* __restrict__ cov2,
                         const double* __restrict__ w2, const double* __restrict__ info1,
                         const double* __restrict__ info2, int D, double* __restrict__ out) {
  __shared__ double red[M2D_DS_THREADS];
  const int pr = blockIdx.x, tid = threadIdx.x;
  double dmu = 0.0, tr = 0.0, rt = 0.0;
  if (tid < D) {      // D <= 128 < 256: one term a thread, the tree fixes the order
    const double d = mean1[(size_t)pr * D + tid] - mean2[(size_t)pr * D + tid];
    dmu = d * d;
    tr = cov1[((size_t)pr * D + tid) * D + tid] + cov2[((size_t)pr * D + tid) * D + tid];
    const double l = w2[(size_t)pr * D + tid];
    rt = sqrt(l < 0.0 ? 0.0 : l);
  }
  dmu = m2d_block_sum<M2D_DS_THREADS>(dmu, red);
  tr = m2d_block_sum<M2D_DS_THREADS>(tr, red);
  rt = m2d_block_sum<M2D_DS_THREADS>(rt, red);
  if (tid == 0) {
    double* o = out + (size_t)pr * 6;
    o[0] = (dmu + tr) - 2.0 * rt;
    o[1] = dmu;
    o[2] = tr;
    o[3] = rt;
    o[4] = fmax(info1[2 * pr], info2[2 * pr]);
    o[5] = (info1[2 * pr + 1] != 0.0 && info2[2 * pr + 1] != 0.0) ? 1.0 : 0.0;
  }
}

// ---- m2d_pairwise_mean_dist ----------------------------------------------------------------------------------------
// workgroup (i, g): the distances of row i of group g to the rows j > i of the group -> part[g K + i]
__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_pairwise_rows_kernel(const float* __restrict__ X, long long ldx, int K, int D, double* __restrict__ part) {
  __shared__ double red[M2D_DS_THREADS];
  const int i = blockIdx.x, g = blockIdx.y;
  const float* xi = X + ((size_t)g * K + i) * ldx;
  double acc = 0.0;
  for (int j = i + 1 + threadIdx.x; j < K; j += M2D_DS_THREADS) {
    const float* xj = X + ((size_t)g * K + j) * ldx;
    double ss = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (double)(xi[d] - xj[d]);               // the difference in fp32, directly
      ss = fma(df, df, ss);
    }
    acc += sqrt(ss);
  }
  acc = m2d_block_sum<M2D_DS_THREADS>(acc, red);
  if (threadIdx.x == 0) part[(size_t)g * K + i] = acc;
}

__global__ void __launch_bounds__(M2D_DS_THREADS)
m2d_pairwise_final_kernel(const double* __restrict__ part, int K, double* __restrict__ out) {
  __shared__ double red[M2D_DS_THREADS];
  const int g = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < K; i += M2D_DS_THREADS) acc += part[(size_t)g * K + i];
  acc = m2d_block_sum<M2D_DS_THREADS>(acc, red);
  if (threadIdx.x == 0)
    out[g] = K < 2 ? __longlong_as_double(0x7ff8000000000000LL) : acc / (0.5 * (double)K * (double)(K - 1));
}

// a pointer the device can be handed: known to the runtime and not host memory
bool ds_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t at;
  memset(&at, 0, sizeof(at));
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return at.type != hipMemoryTypeHost && at.type != hipMemoryTypeUnregistered;
}

size_t eig_ws_bytes(int P, int D, int vectors) {
  if (P <= 0 || D <= 0 || D > M2D_EIG_MAX_D || !vectors) return 0;
  const size_t n = (size_t)D + (D & 1);
  return (size_t)P * n * n * sizeof(double);
}

int eig_launch(const double* A, int P, int D, double* w, double* vecs, double* info, double* vt, hipStream_t stream) {
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 0.0, 8.0 * (double)P * D * D * (vecs ? 3 : 1), "sym_eig", P, D, vecs ? 1 : 0);
  hipLaunchKernelGGL(m2d_sym_eig_kernel, dim3((unsigned)P), dim3(M2D_EIG_THREADS), 0, stream, A, D, w, vecs, vt, info);
  M2D_CHECK_LAUNCH("m2d_sym_eig");
  return M2D_OK;
}

}  // namespace

extern "C" {

int m2d_kinetic_features(const float* poses, int B, int T, int J, double fps, int up_axis, float* F, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || J <= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_kinetic_features: B and J must be positive");
  if (T < 3) M2D_FAIL(M2D_ERR_ARG, "m2d_kinetic_features: at least 3 frames are needed (got %d)", T);
  if (up_axis < 0 || up_axis > 2) M2D_FAIL(M2D_ERR_ARG, "m2d_kinetic_features: up_axis must be 0, 1 or 2 (got %d)", up_axis);
  if (!(fps > 0.0)) M2D_FAIL(M2D_ERR_ARG, "m2d_kinetic_features: fps must be positive");
  if ((long long)B * J > 0x7fffffffLL) M2D_FAIL(M2D_ERR_ARG, "m2d_kinetic_features: too many rows");
  if (!ds_device_ptr(poses) || !ds_device_ptr(F)) M2D_FAIL(M2D_ERR_ARG, "m2d_kinetic_features: null or host pointer");
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 30.0 * (double)B * T * J, 12.0 * (double)B * T * J, "kinetic", T, J, up_axis);
  hipLaunchKernelGGL(m2d_kinetic_kernel, dim3((unsigned)(B * J)), dim3(M2D_DS_THREADS), 0, stream, poses, T, J,
                     fps, up_axis, F);
  M2D_CHECK_LAUNCH("m2d_kinetic_features");
  return M2D_OK;
}

int m2d_sym_eig_max_dim(void) { return M2D_EIG_MAX_D; }
int m2d_sym_eig_max_sweeps(void) { return M2D_EIG_SWEEPS; }

int m2d_feature_moments(const float* X, long long ldx, int N, int D, double* mean, double* cov, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (N < 2) M2D_FAIL(M2D_ERR_ARG, "m2d_feature_moments: at least 2 rows are needed (got %d)", N);
  if (D <= 0 || D > M2D_EIG_MAX_D)
    M2D_FAIL(M2D_ERR_ARG, "m2d_feature_moments: D must be in [1, %d] (got %d)", M2D_EIG_MAX_D, D);
  if (ldx < D) M2D_FAIL(M2D_ERR_ARG, "m2d_feature_moments: row stride below D");
  if (!ds_device_ptr(X) || !ds_device_ptr(mean) || !ds_device_ptr(cov))
    M2D_FAIL(M2D_ERR_ARG, "m2d_feature_moments: null or host pointer");
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 2.0 * (double)N * D * D, 4.0 * (double)N * D, "moments", N, D, 0);
  hipLaunchKernelGGL(m2d_moments_mean_kernel, dim3((unsigned)D), dim3(M2D_DS_THREADS), 0, stream, X, ldx, N, mean);
  M2D_CHECK_LAUNCH("m2d_feature_moments");
  const unsigned tiles = (unsigned)m2d_ceil_div(D, 16);
  hipLaunchKernelGGL(m2d_moments_cov_kernel, dim3(tiles, tiles), dim3(M2D_DS_THREADS), 0, stream, X, ldx, N, D,
                     (const double*)mean, cov);
  M2D_CHECK_LAUNCH("m2d_feature_moments");
  return M2D_OK;
}

size_t m2d_sym_eig_workspace_bytes(int P, int D, int vectors) { return eig_ws_bytes(P, D, vectors); }

int m2d_sym_eig(const double* A, int P, int D, double* w, double* vecs, double* info, void* ws, size_t ws_bytes,
                void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (P <= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_sym_eig: P must be positive");
  if (D <= 0 || D > M2D_EIG_MAX_D) M2D_FAIL(M2D_ERR_ARG, "m2d_sym_eig: D must be in [1, %d] (got %d)", M2D_EIG_MAX_D, D);
  if (!ds_device_ptr(A) || !ds_device_ptr(w) || !ds_device_ptr(info) || (vecs && !ds_device_ptr(vecs)))
    M2D_FAIL(M2D_ERR_ARG, "m2d_sym_eig: null or host pointer");
  const size_t need = eig_ws_bytes(P, D, vecs != nullptr);
  if (need && (!ws || ws_bytes < need)) M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_sym_eig: workspace of %zu bytes needed", need);
  return eig_launch(A, P, D, w, vecs, info, (double*)ws, stream);
}

// workspace of m2d_frechet, in doubles: w1, w2 (P D each), info1, info2 (2 P each), V, Tm, M (P D D each), V^T scratch
size_t m2d_frechet_workspace_bytes(int P, int D) {
  if (P <= 0 || D <= 0 || D > M2D_EIG_MAX_D) return 0;
  const size_t pd = (size_t)P * D, pdd = pd * D;
  return (2 * pd + 4 * (size_t)P + 3 * pdd) * sizeof(double) + eig_ws_bytes(P, D, 1);
}

int m2d_frechet(const double* mean1, const double* cov1, const double* mean2, const double* cov2, int P, int D,
                double* out, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (P <= 0 || P > 65535) M2D_FAIL(M2D_ERR_ARG, "m2d_frechet: P must be in [1, 65535]");
  if (D <= 0 || D > M2D_EIG_MAX_D) M2D_FAIL(M2D_ERR_ARG, "m2d_frechet: D must be in [1, %d] (got %d)", M2D_EIG_MAX_D, D);
  if (!ds_device_ptr(mean1) || !ds_device_ptr(cov1) || !ds_device_ptr(mean2) || !ds_device_ptr(cov2) ||
      !ds_device_ptr(out))
    M2D_FAIL(M2D_ERR_ARG, "m2d_frechet: null or host pointer");
  const size_t need = m2d_frechet_workspace_bytes(P, D);
  if (!ws || ws_bytes < need) M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_frechet: workspace of %zu bytes needed", need);
  const size_t pd = (size_t)P * D, pdd = pd * D;
  double* w1 = (double*)ws;
  double* w2 = w1 + pd;
  double* info1 = w2 + pd;
  double* info2 = info1 + 2 * (size_t)P;
  double* V = info2 + 2 * (size_t)P;
  double* Tm = V + pdd;
  double* M = Tm + pdd;
  double* vt = M + pdd;
  int rc = eig_launch(cov1, P, D, w1, V, info1, vt, stream);
  if (rc != M2D_OK) return rc;
  {
    M2dProfScope prof(M2D_FAM_REDUCE, stream, 4.0 * (double)pdd * D, 8.0 * 5.0 * (double)pdd, "frechet_mm", P, D, 0);
    const dim3 grid((unsigned)m2d_ceil_div(D * D, M2D_DS_THREADS), (unsigned)P);
    hipLaunchKernelGGL(m2d_frechet_sv_kernel, grid, dim3(M2D_DS_THREADS), 0, stream, cov2, (const double*)V, D, Tm);
    M2D_CHECK_LAUNCH("m2d_frechet");
    hipLaunchKernelGGL(m2d_frechet_vtv_kernel, grid, dim3(M2D_DS_THREADS), 0, stream, (const double*)V,
                       (const double*)Tm, (const double*)w1, D, M);
    M2D_CHECK_LAUNCH("m2d_frechet");
  }
  rc = eig_launch(M, P, D, w2, nullptr, info2, nullptr, stream);
  if (rc != M2D_OK) return rc;
  hipLaunchKernelGGL(m2d_frechet_final_kernel, dim3((unsigned)P), dim3(M2D_DS_THREADS), 0, stream, mean1, cov1, mean2,
                     cov2, (const double*)w2, (const double*)info1, (const double*)info2, D, out);
  M2D_CHECK_LAUNCH("m2d_frechet");
  return M2D_OK;
}

size_t m2d_pairwise_mean_dist_workspace_bytes(int G, int K) {
  if (G <= 0 || K <= 0) return 0;
  return (size_t)G * K * sizeof(double);
}

int m2d_pairwise_mean_dist(const float* X, long long ldx, int G, int K, int D, double* out, void* ws, size_t ws_bytes,
                           void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (G <= 0 || K <= 0 || D <= 0) M2D_FAIL(M2D_ERR_ARG, "m2d_pairwise_mean_dist: G, K and D must be positive");
  if (G > 65535) M2D_FAIL(M2D_ERR_ARG, "m2d_pairwise_mean_dist: at most 65535 groups");
  if (ldx < D) M2D_FAIL(M2D_ERR_ARG, "m2d_pairwise_mean_dist: row stride below D");
  if (!ds_device_ptr(X) || !ds_device_ptr(out)) M2D_FAIL(M2D_ERR_ARG, "m2d_pairwise_mean_dist: null or host pointer");
  const size_t need = m2d_pairwise_mean_dist_workspace_bytes(G, K);
  if (!ws || ws_bytes < need) M2D_FAIL(M2D_ERR_WORKSPACE, "m2d_pairwise_mean_dist: workspace of %zu bytes needed", need);
  M2dProfScope prof(M2D_FAM_REDUCE, stream, 1.5 * (double)G * K * K * D, 4.0 * (double)G * K * D, "pairwise", G, K, D);
  hipLaunchKernelGGL(m2d_pairwise_rows_kernel, dim3((unsigned)K, (unsigned)G), dim3(M2D_DS_THREADS), 0, stream, X, ldx,
                     K, D, (double*)ws);
  M2D_CHECK_LAUNCH("m2d_pairwise_mean_dist");
  hipLaunchKernelGGL(m2d_pairwise_final_kernel, dim3((unsigned)G), dim3(M2D_DS_THREADS), 0, stream, (const double*)ws,
                     K, out);
  M2D_CHECK_LAUNCH("m2d_pairwise_mean_dist");
  return M2D_OK;
}

}  // extern "C"
