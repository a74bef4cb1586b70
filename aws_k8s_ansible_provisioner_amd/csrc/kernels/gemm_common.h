// Device helpers shared by the GEMM kernels (gemm / dgemm / gdgemm / kgemm / wgemm / qgemm /
// q4gemm / pgemm, and through moe_gemm_common.h moe_dgemm / moe_qgemm / moe_q4gemm): LDS swizzle
// and LDS-DMA staging, counted waits, the epilogue arithmetic whose rounding order is a contract
// with the CPU reference, and the split-K ticket step.
#pragma once

#include "common.h"
#include "kernels.h"

namespace akap {

constexpr int kSc1 = 16;  // buffer op cache bits: sc1 (write-through stores, L1-bypass loads)

// LDS tile rows of 64 bf16 = 8 chunks of 16 B: chunk' = chunk ^ (row & 7), so the 16 lanes of a
// ds_read_b128 lane group (16 consecutive rows, one chunk) hit 16 distinct 16-B bank positions.
// Returns the 16-B unit index.
__device__ __forceinline__ int swz8(int row, int chunk) { return row * 8 + (chunk ^ (row & 7)); }

// LDS rows of 64 B = 4 chunks of 16 B (64 fp8 or 128 packed e2m1 codes: qgemm.hip, q4gemm.hip,
// moe_q4gemm.hip): chunk c stored at c ^ g((row >> 2) & 3), g = {0, 2, 3, 1} (wgemm.hip ww_swz).
// Returns the 16-B unit index.
__device__ __forceinline__ int swz4_g(int row) { return (0x1320 >> (4 * ((row >> 2) & 3))) & 3; }
__device__ __forceinline__ int swz4_w(int row, int c) { return row * 4 + (c ^ swz4_g(row)); }

// LDS-DMA: 16 B per lane from g to lds_wave_base + 16 * lane.  AUX = kAuxNT is the non-temporal
// policy: for once-read weights only (MI355X_MICROARCH.md nt-weights), never for the
// activation rows every column tile re-reads.
constexpr int kAuxNT = 2;
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0,
                                   AUX);
}

// LDS-DMA, 4 B per lane from g to lds_wave_base + 4 * lane
__device__ __forceinline__ void glds4(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}

// at most N_ of this wave's vector memory operations still outstanding (the counter holds 63)
template <int N_>
__device__ __forceinline__ void wait_vm() {
  if constexpr (N_ >= 63) asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N_) : "memory");
}

__device__ __forceinline__ float silu_bf(float g) { return bf2f(f2bf(g / (1.f + __expf(-g)))); }

// ---- MXFP4 weights: q4gemm.hip, moe_q4gemm.hip ------------------------------------------------
// 8 e2m1 codes (element e in bits [4e, 4e + 4)) times `scale` (a power of two) -> 8 bf16, exact
__device__ __forceinline__ bf16x8 fp4x8_to_bf16x8(uint32_t v, float scale) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(v, scale, 3);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
// e8m0 code (2..252) -> 2^(code - 127)
__device__ __forceinline__ float e8m0_to_f32(uint32_t code) { return __uint_as_float(code << 23); }

// ---- per-channel scaled (FP8-weight) epilogues ----------------------------------------------
// The rounding order of moe_qgemm.hip's and qgemm.hip's scaled epilogues stands next to the
// grouped kernels' tile epilogue in moe_gemm_common.h.

// ---- EPI_RESNORM arithmetic -----------------------------------------------------------------
// The fused residual / next-norm rounding order, a contract with the CPU reference and
// custom_allreduce.hip:  s = bf16(bf16(y * scale) + residual),  a = bf16(s * ln),  returns s^2
// for the row's sum of squares.  (gdgemm.hip's tile epilogue still spells it out:
// profiles/gemm_common_refactor.md.)
__device__ __forceinline__ float resnorm1(float y, float scale, bf16 old, bf16 ln, bf16& o,
                                          bf16& a) {
  o = f2bf(bf2f(f2bf(y * scale)) + bf2f(old));
  const float f = bf2f(o);
  a = f2bf(f * bf2f(ln));
  return f * f;
}
// 4 consecutive columns of one row; returns ss + their sum of squares, added element by element
// (ss: the running sum of a thread that handles several groups of one row)
__device__ __forceinline__ float resnorm4(f32x4 y, float scale, bf16x4 old, bf16x4 ln, bf16x4& o,
                                          bf16x4& a, float ss = 0.f) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16 oj, aj;
    ss += resnorm1(y[j], scale, old[j], ln[j], oj, aj);
    o[j] = oj;
    a[j] = aj;
  }
  return ss;
}

// ---- in-launch split-K combine: the last-arriver ticket ---------------------------------------
// Call after issuing this slice's write-through (sc1) slab stores.  Every storing wave drains
// its stores, the workgroup barrier, then thread 0 takes an agent-scope ticket on the tile's
// counter; the slice that draws S-1 re-arms the ticket for the next launch.  Returns, to every
// thread of the workgroup, whether this slice is that last arriver (it then combines the S
// slabs).  flag: one int of LDS.
template <int S>
__device__ __forceinline__ bool splitk_last_arriver(int* ticket, int* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave drains its stores
  __syncthreads();
  if (threadIdx.x == 0) {
    const int prev = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == S - 1;
    if (last) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *flag = last;
  }
  __syncthreads();
  return *flag != 0;
}

}  // namespace akap
