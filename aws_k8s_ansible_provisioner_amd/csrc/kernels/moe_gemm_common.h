// What the grouped expert GEMMs for MoE decode share (moe_dgemm.hip bf16, moe_qgemm.hip FP8,
// moe_q4gemm.hip MXFP4 weights): the tile geometry, the gate/up interleave map, the GATHER row
// pointers, the compile-time load ring, the LDS store of the 128-deep steps' two A k-tiles, the
// tile epilogue and the host dispatch over the compiled variants.  Each kernel file keeps its
// weight and scale staging, its LDS layout and its fragment order.
// The ring and the epilogue are macros: shared as function templates they compile to other code
// than the text they replace (below), and every shared piece here compiles to the instructions
// the kernels had before it was shared (profiles/moe_gemm_common_refactor.md).
#pragma once

#include "gemm_common.h"

namespace akap {

constexpr int MOE_BN = 128;  // tile columns

// BM = rows per tile (32 or 64): 4 waves as WM (= BM/32) x WN (= 4/WM), each owning a
// 32-row x (128/WN)-col sub-tile = 2 x JN 16x16 MFMA tiles.  AR: A rows staged per thread.
template <int BM>
struct MoeTile {
  static constexpr int WM = BM / 32, WN = 4 / WM, WCOLS = MOE_BN / WN, JN = WCOLS / 16;
  static constexpr int AR = BM / 32;
};

// The weight row a virtual tile column v reads (columns past N read row 0).  SILU: W = [gate; up]
// is read gate/up-interleaved in 16-row groups (dgemm.hip EPI_SILU).
template <bool SILU>
__device__ __forceinline__ int moe_wrow(int v, int N) {
  int wrow = v < N ? v : 0;
  if constexpr (SILU) wrow = v < N ? ((v >> 4) & 1) * (N >> 1) + (v >> 5) * 16 + (v & 15) : 0;
  return wrow;
}

// The activation row a thread stages for tile row arow.  GATHER: through sorted_ids to the
// hidden-state row; padding rows read row 0 and their outputs are never combined.
template <bool GATHER>
__device__ __forceinline__ const bf16* moe_a_row(const bf16* A, const int32_t* sorted_ids,
                                                 int arow, int n_flat, int topk, int lda) {
  if constexpr (GATHER) {
    const int sid = sorted_ids[arow];
    arow = sid < n_flat ? sid / topk : 0;
  }
  return A + (size_t)arow * lda;
}

// The compile-time load ring (dgemm.hip's): PF steps of loads in flight in registers, an LDS
// double buffer.  gload(q, k0) loads the step at k0 into ring slot q, sstore(q, buf) writes slot
// q to LDS buffer buf, mfma(buf, last) multiplies it; last marks the slice's final step (a half
// step in the 128-deep kernels).  nk steps of STEP from kbeg; the host keeps nk % PF == 0.
// A macro, not a function template over the three callables: the compiler optimizes a helper
// on its own before it inlines it, so the q loops are unrolled while the ring registers still
// sit behind the closures' pointers, and every kernel's code changes (the k offsets of the
// priming loads no longer fold into the instructions; the FP8 kernels reach 246 VGPRs from
// 240).  Expanded in the kernel, the loops are unrolled where they always were.
#define MOE_RING(PF, STEP, nk, kbeg, gload, sstore, mfma)                               \
  do {                                                                                  \
    _Pragma("unroll") for (int q = 0; q < PF; ++q) gload(q, (kbeg) + q * (STEP));       \
    int t = 0;                                                                          \
    for (; t + PF < (nk); t += PF) {                                                    \
      _Pragma("unroll") for (int q = 0; q < PF; ++q) {                                  \
        const int buf = (t + q) & 1;                                                    \
        sstore(q, buf);                                                                 \
        __syncthreads();                                                                \
        gload(q, (kbeg) + (t + q + PF) * (STEP));                                       \
        __builtin_amdgcn_sched_barrier(0);  /* keep the refill here (see dgemm.hip) */  \
        mfma(buf, false);                                                               \
      }                                                                                 \
    }                                                                                   \
    _Pragma("unroll") for (int q = 0; q < PF; ++q) {                                    \
      const int buf = (t + q) & 1;                                                      \
      sstore(q, buf);                                                                   \
      __syncthreads();                                                                  \
      mfma(buf, q == PF - 1);                                                           \
    }                                                                                   \
  } while (0)

// A staging of a 128-deep step (moe_qgemm.hip, moe_q4gemm.hip): two 64-deep k-tiles per row,
// sa[PF][2][AR] in registers (each kernel's gload fills them: the second k-tile of a half step
// is not loaded, the registers hold zeros), stored to LDS as [k-tile 0: BM rows | k-tile 1: BM
// rows] x 8 chunks at buf.
template <int BM, int AR>
__device__ __forceinline__ void moe_sstore_a2(u32x4* buf, const u32x4 (&sa)[2][AR], int s_r,
                                              int s_ch) {
#pragma unroll
  for (int h = 0; h < 2; ++h)
#pragma unroll
    for (int c = 0; c < AR; ++c) buf[h * BM * 8 + swz8(s_r + 32 * c, s_ch)] = sa[h][c];
}

// ---- the tile epilogue ---------------------------------------------------------------------
// Lane holds rows wm*32 + i*16 + fg*4 + r, column fr of each 16-col sub-tile j.
//   store   Y[r, n] = bf16(acc)
//   SILU    sub-tiles 2jj / 2jj+1 = gate / up:  Y[r, f] = bf16(bf16(silu(bf16(g))) * bf16(u)),
//           Y is [rows, N/2]
//   SPLIT   P[z, r, n] = acc_z   (fp32, ldy = N; moe_combine_split sums the slices)
// Per-channel scaled (FP8-weight) form, sc[j] the scale of the weight row sub-tile j's column
// fr was read from.  The rounding order is a contract with the CPU reference (ops/quant.py):
// the scale multiplies the fp32 accumulator BEFORE the first rounding.
//   store   y    = bf16(scale[e, n] * acc)
//   SILU    g    = bf16(s_gate * acc_gate),  u = bf16(s_up * acc_up),  y = bf16(silu_bf(g) * u)
//           with s_gate / s_up the scales of the weight rows the gate/up interleave read
//   split   P[z] = scale[e, n] * acc_z
// qgemm.hip's store epilogue follows the same rule with scale[n].
// A macro for the reason MOE_RING is one (as a function template it reorders the address
// arithmetic of every kernel that stores bf16).  Expanded at the end of the kernel, it uses the
// kernel's acc[2][JN], Y, P, m0, n0, wm, wn, fr, fg, N, ldy, rows and SILU / SPLIT / WCOLS / JN.
// scaled(j, x): what sub-tile j makes of accumulator x before the first rounding.
#define MOE_NO_SCALE(j, x) (x)  /* bf16 and MXFP4 weights: no accumulator multiply */
#define MOE_TILE_EPILOGUE(scaled)                                                          \
  _Pragma("unroll") for (int i = 0; i < 2; ++i)                                            \
  _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                          \
    const int row = m0 + wm * 32 + i * 16 + fg * 4 + r;                                   \
    if constexpr (SILU) {                                                                  \
      _Pragma("unroll") for (int jj = 0; jj < JN / 2; ++jj) {                              \
        const int vb = n0 + wn * WCOLS + 32 * jj;                                          \
        if (vb + 16 + fr < N) {                                                            \
          const float g = bf2f(f2bf(scaled(2 * jj, acc[i][2 * jj][r])));                   \
          const float u = bf2f(f2bf(scaled(2 * jj + 1, acc[i][2 * jj + 1][r])));           \
          Y[(size_t)row * ldy + (vb >> 1) + fr] = f2bf(silu_bf(g) * u);                    \
        }                                                                                  \
      }                                                                                    \
    } else if constexpr (SPLIT) {                                                          \
      float* pz = P + ((size_t)blockIdx.z * rows + row) * N;                               \
      _Pragma("unroll") for (int j = 0; j < JN; ++j) {                                     \
        const int col = n0 + wn * WCOLS + j * 16 + fr;                                     \
        if (col < N) pz[col] = scaled(j, acc[i][j][r]);                                    \
      }                                                                                    \
    } else {                                                                               \
      _Pragma("unroll") for (int j = 0; j < JN; ++j) {                                     \
        const int col = n0 + wn * WCOLS + j * 16 + fr;                                     \
        if (col < N) Y[(size_t)row * ldy + col] = f2bf(scaled(j, acc[i][j][r]));           \
      }                                                                                    \
    }                                                                                      \
  }

// ---- host dispatch ---------------------------------------------------------------------------
// Runtime (bm, gather, silu, split, pf, ntw) -> the compiled variant of kernel family F:
// BM 32 | 64 x six (GATHER, SILU, SPLIT) forms (SILU never splits) x (PF, NTW) in {(1, 0),
// (2, 0), (2, 1), (4, 0), (4, 1)}; pf = 1 ignores ntw.  F::launch<BM, G, S, PF, SPL, NT>(grid,
// stream, args...) launches its kernel; the families differ by the scale pointer in args.
template <typename F, int BM, bool G, bool S, bool SPL, typename... Args>
static void moe_launch_pf(int pf, bool ntw, dim3 grid, hipStream_t s, Args... a) {
  switch (pf) {
    case 4:
      if (ntw) F::template launch<BM, G, S, 4, SPL, true>(grid, s, a...);
      else F::template launch<BM, G, S, 4, SPL, false>(grid, s, a...);
      break;
    case 2:
      if (ntw) F::template launch<BM, G, S, 2, SPL, true>(grid, s, a...);
      else F::template launch<BM, G, S, 2, SPL, false>(grid, s, a...);
      break;
    default: F::template launch<BM, G, S, 1, SPL, false>(grid, s, a...);
  }
}

template <typename F, int BM, typename... Args>
static void moe_launch_form(bool gather, bool silu, int pf, bool ntw, dim3 grid, hipStream_t s,
                            Args... a) {
  const bool spl = grid.z > 1;
  if (gather && silu) moe_launch_pf<F, BM, true, true, false>(pf, ntw, grid, s, a...);
  else if (silu) moe_launch_pf<F, BM, false, true, false>(pf, ntw, grid, s, a...);
  else if (gather && spl) moe_launch_pf<F, BM, true, false, true>(pf, ntw, grid, s, a...);
  else if (gather) moe_launch_pf<F, BM, true, false, false>(pf, ntw, grid, s, a...);
  else if (spl) moe_launch_pf<F, BM, false, false, true>(pf, ntw, grid, s, a...);
  else moe_launch_pf<F, BM, false, false, false>(pf, ntw, grid, s, a...);
}

// grid = (max_tiles, column tiles, splitk); the kernels take rows = max_tiles * bm last
template <typename F, typename... Args>
static void moe_launch(int max_tiles, int N, int splitk, int bm, int gather, int silu, int pf,
                       bool ntw, hipStream_t s, Args... a) {
  if (max_tiles == 0) return;
  const dim3 grid(max_tiles, (N + MOE_BN - 1) / MOE_BN, splitk);
  const int rows = max_tiles * bm;
  if (bm == 64) moe_launch_form<F, 64>(gather, silu, pf, ntw, grid, s, a..., rows);
  else moe_launch_form<F, 32>(gather, silu, pf, ntw, grid, s, a..., rows);
}

}  // namespace akap
