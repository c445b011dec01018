// Shared helpers of the matrix-core GEMMs (gemm3.hip, gemmx3.hip, gemmh2.hip)
// and of the sampler's LDS-DMA ring: vector types of the MFMA operands, the
// hand-counted LDS DMA, the bare barrier, the exact bf16 split and the
// swizzle of the transposed LDS reads.
#pragma once
#include "common.hpp"

namespace nts_hip {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;  // ds_read_b64_tr_b16's operand
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// the 32-bit LDS address of a __shared__ object
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(lds_ptr_t)p;
}

// 16 bytes per lane from `src` to LDS (wave-uniform base `lds`) + 16 * lane.
// Inline asm: hipcc cannot tell the stages of one LDS array apart and, for a
// compiler-visible LDS DMA, waits vmcnt(0) before the next ds_read of ANY
// stage (draining the pipeline).  Completion is counted by hand (s_waitcnt
// vmcnt(N)) by the caller.
__device__ __forceinline__ void glds16(const void* src, uint32_t lds) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(lds)
      : "memory");
}

// s_barrier between two compiler fences, and nothing else: unlike
// __syncthreads() it emits no s_waitcnt, so the LDS DMAs in flight stay in
// flight.  It therefore does NOT wait for the calling wave's outstanding LDS
// stores either: a caller that wrote LDS for other waves to read must issue
// its own s_waitcnt lgkmcnt(0) before calling it.
__device__ __forceinline__ void raw_barrier() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// The exact three-piece bf16 split x -> (x0, x1, x2): x0 = bf16(x), x1 =
// bf16(x - x0), x2 = bf16(x - x0 - x1), RNE each, so x0 + x1 + x2 == x for
// every finite fp32.  Element-wise over one lane's 8 fragment values.
__device__ __forceinline__ void split3(const float (&x)[8], bf16x8& h0, bf16x8& h1, bf16x8& h2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 a0 = (__bf16)x[j];
    const float r1 = x[j] - (float)a0;
    const __bf16 a1 = (__bf16)r1;
    const float r2 = r1 - (float)a1;
    h0[j] = a0;
    h1[j] = a1;
    h2[j] = (__bf16)r2;
  }
}

// the same split of two fp32 values into three packed bf16 pairs (the
// pairwise form, so the pieces can be scheduled pair by pair)
__device__ __forceinline__ void split3_pair(float x0, float x1, uint32_t& p0, uint32_t& p1, uint32_t& p2) {
  const bf16x2 h = __builtin_convertvector((f32x2){x0, x1}, bf16x2);
  const f32x2 hf = __builtin_convertvector(h, f32x2);
  const float r0 = x0 - hf[0], r1 = x1 - hf[1];
  const bf16x2 m = __builtin_convertvector((f32x2){r0, r1}, bf16x2);
  const f32x2 mf = __builtin_convertvector(m, f32x2);
  const bf16x2 l = __builtin_convertvector((f32x2){r0 - mf[0], r1 - mf[1]}, bf16x2);
  p0 = __builtin_bit_cast(uint32_t, h);
  p1 = __builtin_bit_cast(uint32_t, m);
  p2 = __builtin_bit_cast(uint32_t, l);
}

// byte offset of 16-byte chunk `ch` (0..15) of row `row` in an image of
// 256-byte rows whose chunks are XOR-swizzled for ds_read_b64_tr_b16
// (one swizzle for the bf16 and the f16 TN kernels)
__device__ __forceinline__ int tr_off(int row, int ch) {
  return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
}

}  // namespace nts_hip
