// What the two weight-streaming decode GEMMs over quantized weights share (qgemm.hip FP8,
// q4gemm.hip MXFP4): a 4-wave workgroup owns a BM x BN output tile, wave w takes the BK-deep
// k-steps w, w + 4, ... through a private NS-slot LDS-DMA ring with no barrier in the K loop,
// and the four partial tiles are summed through LDS -- no workspace, tickets or atomics.  Here
// are the tile prologue, the per-lane DMA source pointers, the accumulators, the ring's prime
// and per-step advance, the combine, the row-segment epilogue and the dequantizers' grid.  Each
// kernel file keeps its slot layout, its `issue`, its fragment reads and widening, its MFMA
// order and its NS table.  (kgemm.hip shares the idea but not the text.)
// Most pieces are macros expanded in the kernel: every piece here compiles to the instructions
// the kernels had before it was shared, and as functions those pieces did not
// (profiles/quant_format_refactor.md; moe_gemm_common.h explains why).
#pragma once

#include "gemm_common.h"

namespace akap {

// The tile prologue: the workgroup's tile (m0, n0), this lane's place in it (tid, lane, w, the
// MFMA fragment row fr and lane group fg) and n, this wave's steps: k0 = (w + 4 s) * BK.  Plain
// statements expanded in the kernel (which has BM, BN and p): returned in a struct by a function,
// every kernel's code changes.
#define QGEMM_TILE_PROLOGUE(BK)                                                             \
  const int tiles_m = (p.M + BM - 1) / BM;                                                  \
  const int tiles_n = (p.N + BN - 1) / BN;                                                  \
  const int lt = xcd_remap(blockIdx.x, tiles_m * tiles_n);                                  \
  const int tn = lt / tiles_m, tm = lt % tiles_m; /* a column tile's row tiles share an XCD */ \
  const int m0 = tm * BM, n0 = tn * BN;                                                     \
  const int tid = threadIdx.x, lane = tid & 63;                                             \
  /* the wave index in a scalar register: the step count and the ring base are wave-uniform */ \
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);                                   \
  const int fr = lane & 15, fg = lane >> 4;                                                 \
  const int nk = p.K / (BK);                                                                \
  const int n = w < nk ? (nk - w + 3) / 4 : 0;

// Per-lane DMA sources of wave w's step 0.  Rows past M / N re-read row 0 (never stored).
// X: the source of the instruction that moves 8 rows x 128 B from row0 on, lane -> row L / 8, LDS chunk L % 8 holding
// logical chunk (L % 8) ^ (L / 8).
template <int BK>
__device__ __forceinline__ const bf16* qgemm_x_src(const bf16* X, int row0, int M, int ldx, int w,
                                                   int lane) {
  const int lr = lane >> 3, lc = (lane & 7) ^ lr;
  const int row = row0 + lr;
  return X + (size_t)(row < M ? row : 0) * ldx + w * BK + lc * 8;
}
// Wq: one instruction = 16 rows x 64 B, lane -> row L / 4, LDS chunk L % 4 holding logical chunk
// (L % 4) ^ g.  row_bytes: a weight row in memory; step_bytes: a k-step of it.  Fills the
// kernel's wsrc[GW] from Wq, n0, lane, w and p.N; a macro because either function form (one
// pointer returned, the array filled) reschedules q4gemm's prologue.
#define QGEMM_W_SRC(row_bytes, step_bytes)                                                   \
  {                                                                                          \
    const int wr = lane >> 2, wc = (lane & 3) ^ swz4_g(wr);                                  \
    _Pragma("unroll") for (int j = 0; j < GW; ++j) {                                         \
      const int v = n0 + j * 16 + wr;                                                        \
      wsrc[j] = Wq + (size_t)(v < p.N ? v : 0) * (row_bytes) + w * (step_bytes) + wc * 16;   \
    }                                                                                        \
  }

// The kernel's MI x NJ fp32 accumulator tiles, cleared (as a function over the array one
// kernel's register assignment changes)
#define QGEMM_ACC(acc)                                 \
  f32x4 acc[MI][NJ];                                   \
  _Pragma("unroll") for (int i = 0; i < MI; ++i)       \
  _Pragma("unroll") for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}

// The wave-private ring.  issue(s) stages step s with G DMA instructions into slot s % NS.
// Prime NS - 1 steps; then, at the head of step t of the kernel's K loop: retire this wave's
// DMAs of step t (steps t+1 .. t+NS-2 stay in flight when they exist), wait until step t-1's
// fragment reads have returned, so that its slot can be refilled, and refill it.  The reads
// that follow are of this wave's own DMAs, so no barrier is needed.
// Macros for the reason MOE_RING is one: as function templates over the closure they change
// the code of every kernel.
#define QGEMM_RING_PRIME(NS, n, issue) \
  _Pragma("unroll") for (int s = 0; s < NS - 1; ++s) if (s < (n)) issue(s)
#define QGEMM_RING_ADVANCE(NS, G, t, n, issue)                    \
  if ((t) + NS - 2 < (n)) wait_vm<G * (NS - 2)>();                \
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           \
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");              \
  if ((t) + NS - 1 < (n)) issue((t) + NS - 1)

// The 4 waves' partial tiles to LDS as part[w][row][PB] fp32 (over the rings: no wave reads or
// fills its ring any more).  PB = BN + 4: the fg groups on distinct banks.
template <int MI, int NJ>
__device__ __forceinline__ void qgemm_combine(float* part, const f32x4 (&acc)[MI][NJ], int w,
                                              int fr, int fg) {
  constexpr int BM = 16 * MI, PB = 16 * NJ + 4;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        part[(w * BM + i * 16 + fg * 4 + r) * PB + j * 16 + fr] = acc[i][j][r];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// The row-segment epilogue: the sum of the four partials, bf16, 16-byte stores (N % 8 == 0: a
// segment is inside N or outside).  SCALED (FP8): the sum times scale[n] before the rounding,
// the order of moe_gemm_common.h's scaled epilogue; MXFP4 applied its block scales in the K loop.
// A macro for the reason MOE_TILE_EPILOGUE is one: as a function template it reorders the address
// arithmetic of the kernels.  Expanded at the end of the kernel, it uses the kernel's part, p,
// m0, n0, tid and BM / BN / PB.
#define QGEMM_STORE_EPILOGUE(SCALED)                                                       \
  bf16* Y = static_cast<bf16*>(p.Y);                                                       \
  constexpr int CPR = BN / 8;                                                              \
  for (int e = tid; e < BM * CPR; e += 256) {                                              \
    const int rr = e / CPR, cc = e % CPR;                                                  \
    const int row = m0 + rr, col = n0 + cc * 8;                                            \
    if (row >= p.M || col >= p.N) continue;                                                \
    f32x4 lo = *reinterpret_cast<const f32x4*>(&part[rr * PB + cc * 8]);                   \
    f32x4 hi = *reinterpret_cast<const f32x4*>(&part[rr * PB + cc * 8 + 4]);               \
    _Pragma("unroll") for (int ww = 1; ww < 4; ++ww) {                                     \
      lo += *reinterpret_cast<const f32x4*>(&part[(ww * BM + rr) * PB + cc * 8]);          \
      hi += *reinterpret_cast<const f32x4*>(&part[(ww * BM + rr) * PB + cc * 8 + 4]);      \
    }                                                                                      \
    if constexpr (SCALED) {                                                                \
      lo *= *reinterpret_cast<const f32x4*>(static_cast<const float*>(p.scale) + col);     \
      hi *= *reinterpret_cast<const f32x4*>(static_cast<const float*>(p.scale) + col + 4); \
    }                                                                                      \
    bf16x8 o;                                                                              \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                        \
      o[q] = f2bf(lo[q]);                                                                  \
      o[4 + q] = f2bf(hi[q]);                                                              \
    }                                                                                      \
    *reinterpret_cast<bf16x8*>(Y + (size_t)row * p.ldy + col) = o;                         \
  }

// Grid of a grid-stride dequantizer over `items` units, one per thread
inline int dequant_grid(long items) {
  const long blocks = (items + 255) / 256;
  return (int)(blocks < 8192 ? blocks : 8192);
}

}  // namespace akap
