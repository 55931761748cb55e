// Device primitives shared by the kernel files (gfx950 only): the vector types, raw buffer loads / stores / LDS-DMA
// with their range-check contract, LDS addresses, and the fp32-exact divmod. A kernel file includes this header instead
// of re-typing the block under a prefix of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x16 __attribute__((ext_vector_type(16)));      // one 32 x 32 MFMA accumulator tile per lane
typedef float m2d_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned m2d_u32x4 __attribute__((__vector_size__(16)));   // (the type the 16-byte builtins take and return)
typedef __attribute__((address_space(3))) float m2d_lds_f;      // a float in LDS

// Global accesses that may fall on padding, a tail or a missing row are raw buffer operations: such an element gets
// the byte offset M2D_OOB, which the hardware range check (num_records = the extent of the tensor in bytes, < 2^31)
// rejects whatever scalar offset is added - a load returns 0.0f, an LDS-DMA writes 0.0f, a store is dropped. No select
// on the data, no divergent branch, nothing that forces a wait on the load before its consumer.
// M2D_BAD is the same idea one step earlier: a window position so large that `(unsigned)(pos + p) < lim` fails for
// every p a kernel adds.
#define M2D_OOB 0x80000000u
#define M2D_BAD 0x40000000

// descriptor over [p, p + nbytes): word 3 = 0x00020000 is DATA_FORMAT 32 with every other field 0 - untyped raw
// addressing (offset = voff + soff in bytes, no stride, no swizzle), range-checked against nbytes. nbytes = 0: every
// load reads 0.0f and every store is dropped (an absent optional tensor).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t m2d_rsrc(const void* p, unsigned nbytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)p, (short)0, (int)nbytes, 0x00020000);
}

// Cache policy of a raw buffer access (the builtins' last argument, a compile-time constant): 0 = default, M2D_SC1 =
// device scope - a load that sees what another workgroup wrote, a store written through to where it will look.
#define M2D_SC1 16

// voff: per-lane byte offset (range-checked), soff: wave-uniform byte offset (SGPR)
template <int CP = 0>
__device__ __forceinline__ float m2d_bload(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff = 0) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, soff, CP));
}
// (the stores take their arguments in the builtins' order: value, descriptor, offset)
template <int CP = 0>
__device__ __forceinline__ void m2d_bstore1(float v, __amdgpu_buffer_rsrc_t r, unsigned voff) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)voff, 0, CP);
}
// 16 bytes. (Whole-vector bit casts: an element-wise __builtin_bit_cast(float, v[i]) on the load builtin's result is
// narrowed to ONE dword load by hipcc 7.2 - every element then reads as the first.)
template <int CP = 0>
__device__ __forceinline__ m2d_f32x4 m2d_bload16(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff = 0) {
  return __builtin_bit_cast(m2d_f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, soff, CP));
}
template <int CP = 0>
__device__ __forceinline__ void m2d_bstore16(m2d_f32x4 v, __amdgpu_buffer_rsrc_t r, unsigned voff) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(m2d_u32x4, v), r, (int)voff, 0, CP);
}

// the same load with the LDS as its destination, no register stop: lane l of the wave writes BYTES bytes at
// dst + l * BYTES (M0 = dst, wave-uniform); lanes whose offset fails the range check write 0.0f (measured on gfx950),
// so padding needs no separate store. BYTES: 4 or 16.
template <int BYTES>
__device__ __forceinline__ void m2d_bload_lds(__amdgpu_buffer_rsrc_t r, float* dst, unsigned voff, int soff) {
  static_assert(BYTES == 4 || BYTES == 16, "LDS-DMA moves 4 or 16 bytes per lane");
  // (the builtin checks its size when the template is parsed: it has to be a literal)
  if constexpr (BYTES == 16) __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (m2d_lds_f*)dst, 16, (int)voff, soff, 0, 0);
  else __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (m2d_lds_f*)dst, 4, (int)voff, soff, 0, 0);
}

// LDS byte address of a pointer into a __shared__ array (what inline-assembly ds_read helpers take)
__device__ __forceinline__ unsigned m2d_lds_addr(const float* p) {
  return (unsigned)(uintptr_t)(__attribute__((address_space(3))) const float*)p;
}

// n / d and n % d for 0 <= n < 2^24 (exact in fp32; the launchers reject larger extents), inv = 1 / d. Branch-free.
// (bn.hip keeps a form of its own, bn_divmod: its kernels compile to different code with this one, unmeasured.)
__device__ __forceinline__ void m2d_divmod(int n, int d, float inv, int& q, int& r) {
  q = (int)((float)n * inv);
  r = n - q * d;
  const int adj = (r < 0 ? -1 : 0) + (r >= d ? 1 : 0);
  q += adj;
  r -= adj * d;
}
