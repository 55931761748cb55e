// Shared plumbing for the m2d HIP library (gfx950 only): error reporting across the
// C-ABI, launch checking, and the optional per-kernel-family event profiler that
// bench.py uses for its roofline line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>

// the public C-ABI (error codes, struct M2dAdamItem, every entry point): each extern "C" definition is compiled against
// its declaration, so one that disagrees with the header is a "conflicting types" error
#include "../../include/m2d.h"

void m2d_set_error(const char* fmt, ...);

#define M2D_FAIL(code, ...)      \
  do {                           \
    m2d_set_error(__VA_ARGS__);  \
    return (code);               \
  } while (0)

#define M2D_CHECK_LAUNCH(name)                                            \
  do {                                                                    \
    hipError_t e__ = hipGetLastError();                                   \
    if (e__ != hipSuccess)                                                \
      M2D_FAIL(M2D_ERR_HIP, "%s: launch failed: %s", name, hipGetErrorString(e__)); \
  } while (0)

// ---- profiler: kernel families ------------------------------------------------
enum M2dFamily {
  M2D_FAM_GEMM = 0,   // implicit-GEMM engine (conv1d fwd/bwd_data/bwd_weight, linear)
  M2D_FAM_BN = 1,     // batch-norm statistics / apply / backward
  M2D_FAM_GRU = 2,    // recurrent step kernels
  M2D_FAM_POINTWISE = 3,
  M2D_FAM_REDUCE = 4,
  M2D_FAM_COUNT = 5
};

struct M2dProfScope {
  int fam;
  hipStream_t stream;
  int slot;
  M2dProfScope(int family, hipStream_t s, double flops, double bytes, const char* tag = nullptr, int d0 = 0,
               int d1 = 0, int d2 = 0);
  ~M2dProfScope();
};

// The fused activation of every epilogue (act: 0 none, 1 ReLU, 2 leaky with `slope`). It gives what
// torch.nn.functional gives on the same fp32 value: NaN -> NaN and +inf -> +inf for every act, -inf -> 0 under ReLU and
// -inf otherwise (non-finite values pass through). One select on `v < 0` - a NaN compares false and is
// handed on untouched - over v times 1 / 0 / slope, formed with v_mul_legacy_f32, whose 0 x anything is 0: -inf x 0 is 0
// under ReLU, not NaN, and the multiplicand is never a NaN (it is < 0). No fmax / fmin: on gfx9 they return the operand
// that is not a NaN. `act` is uniform per launch, so the factor is a scalar formed once: three VALU per element.
extern "C" __device__ float m2d_fmul_legacy(float, float) __asm("llvm.amdgcn.fmul.legacy");

__device__ __forceinline__ float m2d_act(float v, int act, float slope) {
  const float s = act == 0 ? 1.f : (act == 1 ? 0.f : slope);
  return v < 0.f ? m2d_fmul_legacy(v, s) : v;
}

// The same function without the multiply under ReLU, as two selects: for the one-element engine epilogue and
// conv1d_thin.hip, whose kernels sit at a register ceiling and spill SGPRs or VGPRs with the form above.
__device__ __forceinline__ float m2d_act_sel(float v, int act, float slope) {
  const float neg = act == 1 ? 0.f : v * slope;
  return (act != 0 && v < 0.f) ? neg : v;
}

// ---- environment levers (host code; DESIGN.md "Levers" lists every name) -------------------------------------------
// A switch is on unless its value begins with '0'; a number is its default when the name is unset. Call sites keep the
// result in a function-local `static const`, so a lever is read once per process, at first use.
static inline const char* m2d_env_raw(const char* name) { return getenv(name); }   // for a site with a parse of its own
static inline bool m2d_env_on(const char* name) {
  const char* e = m2d_env_raw(name);
  return !(e && e[0] == '0');
}
static inline int m2d_env_int(const char* name, int dflt) {
  const char* e = m2d_env_raw(name);
  return e ? atoi(e) : dflt;
}
static inline double m2d_env_double(const char* name, double dflt) {
  const char* e = m2d_env_raw(name);
  return e ? atof(e) : dflt;
}

// ---- route witness (host code; tests only) --------------------------------------------------------------------------
// One process-wide counter per kernel form a launcher can choose, bumped on the host where the choice is made: the
// suite asks them which kernel a call ran (tests/lever_cases.py, tests/test_gpu_levers.py). A relaxed increment per
// launch, no lock, nothing on the device. m2d_debug_routes / m2d_debug_route_names (m2d_runtime.hip) read them; the
// names are this list, in this order.
#define M2D_ROUTES(X)                                                                                                  \
  /* gemm_engine.hip, launch_maps: the kernel a tile launch runs */                                                    \
  X(gemm_dl_tall) X(gemm_dl8) X(gemm_dl4_128) X(gemm_dl_small)                                                         \
  X(gemm_reg_rr) X(gemm_reg_rr_masked) X(gemm_reg_kr) X(gemm_reg_kr_masked) X(gemm_reg_kk) X(gemm_reg_kk_masked)       \
  /* plan_and_launch (both launchers): epilogue, split-K form, tile order, statistics */                               \
  X(epi_wide) X(epi_one) X(splitk_one_launch) X(splitk_two_launch) X(tile_map_off)                            \
  X(stats_general) X(stats_split) X(k4_paired) X(k4_plain)                                                             \
  /* conv1d.hip: backward-data forms and the handovers to the dedicated kernels */                                     \
  X(bwd_subpixel_tall) X(bwd_subpixel_cir) X(bwd_polyphase)                                                            \
  X(conv_to_tcn_fwd) X(conv_to_tcn_bwd_data) X(conv_to_tcn_wgrad) X(conv_to_thin_long)                                 \
  /* tcn.hip */                                                                                                        \
  X(tcn_ns4) X(tcn_ns8) X(tcn_nt96) X(tcn_nt64) X(tcn_nt48) X(tcn_nt32) X(tcn_nt16) X(tcn_wgrad)                       \
  /* conv1d_thin.hip */                                                                                                \
  X(thin_long) X(thin_persistent)                                                                                      \
  /* bn.hip */                                                                                                         \
  X(bn_reduce_vec) X(bn_reduce_scalar) X(bn_fin_in_apply) X(bn_fin_launch)                                             \
  /* pointwise.hip */                                                                                                  \
  X(up_fwd_flat) X(up_fwd_vec) X(up_fwd_row) X(up_fwd_plain) X(up_bwd_flat) X(up_bwd_plain)                            \
  /* gru.hip */                                                                                                        \
  X(gru_fwd_persistent) X(gru_fwd_steps) X(gru_bwd_persistent) X(gru_bwd_steps) X(gru_small)

enum M2dRoute {
#define M2D_ROUTE_ENUM(name) M2D_RT_##name,
  M2D_ROUTES(M2D_ROUTE_ENUM)
#undef M2D_ROUTE_ENUM
  M2D_RT_COUNT
};

extern std::atomic<unsigned long long> g_m2d_routes[M2D_RT_COUNT];   // m2d_runtime.hip
static inline void m2d_route_hit(int route) { g_m2d_routes[route].fetch_add(1, std::memory_order_relaxed); }

static inline int m2d_ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline long long m2d_ceil_div64(long long a, long long b) { return (a + b - 1) / b; }
