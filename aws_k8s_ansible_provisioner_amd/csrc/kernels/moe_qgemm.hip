// Grouped expert GEMM for MoE decode with FP8 (OCP e4m3fn) expert weights on gfx950: the
// 1-byte-weight form of moe_dgemm.hip (W8A16).
//
//   Y[r] = bf16( scale[e, :] * (A[row(r)] . float(Wq[e])^T) )     e = tile_expert[tile(r)]
//
// Wq uint8 [E, N, K] holds e4m3fn codes, scale fp32 [E, N] one value per expert and output
// channel.  Everything moe_dgemm.hip fixes is kept: one expert per BM x 128 tile (BM 32 | 64),
// the uniform exit for tiles past the padded rows, GATHER through sorted_ids (padding rows
// read row 0), the gate/up-interleaved SILU epilogue, SPLIT over gridDim.z into fp32 partials
// for moe_combine_split, the compile-time load ring, no workspace and no cross-workgroup
// state (graph-capturable, bit-reproducible).
//
// What the 1-byte weights change:
//   * a k-step is 128 deep.  A weight row of a step is then 128 B = one cache line, staged
//     as in moe_dgemm.hip by 8 lanes x 16 B; the activation rows of the step are two 64-deep
//     k-tiles (two 128-B lines per row).  A thread issues the same four 16-B weight loads per
//     step as the bf16 kernel, so a ring of PF steps keeps the same weight bytes in flight
//     and covers twice the K.
//   * a slice whose depth is an odd multiple of 64 ends in a half step: its second k-tile
//     is not loaded (the registers hold zeros) and not multiplied.  The weight lanes of
//     that half (chunks 4..7) are idle, so the last request of such a row is 64 B.
//   * the weights stay 1 byte through HBM, L2 AND LDS and are widened to bf16 at the
//     fragment read (fp8x8_to_bf16x8, exact), as qgemm.hip does: a W tile in LDS is 128 rows
//     x 8 chunks of 16 B, the geometry (and swz8 swizzle) of the bf16 kernel's 64-deep tile.
//     Widening before the LDS store instead would double the LDS bytes of W (the 64-row
//     variant would no longer fit two workgroups' double buffers in 64 KB of static LDS);
//     that form was not built, so the choice rests on the LDS budget, not on an A/B timing
//     (profiles/moe_fp8_weights.md).
//   * fragment k-order: lane group fg of MFMA pair ks owns k in [64 ks + 16 fg, +16): ONE
//     ds_read_b128 of the fp8 row feeds both MFMAs (low 8 bytes, high 8 bytes); the A
//     operands are chunks 2 fg and 2 fg + 1 of k-tile ks.  A and B agree on the order.
//   * the scale multiplies the fp32 accumulator before the first rounding (moe_gemm_common.h).
#include "moe_gemm_common.h"

namespace akap {

template <int BM, bool GATHER, bool SILU, int PF, bool SPLIT, bool NTW = false>
__global__ __launch_bounds__(256, 2) void moe_qgemm_kernel(const bf16* __restrict__ A,
                                                           const uint8_t* __restrict__ W,
                                                           const float* __restrict__ scale,
                                                           bf16* __restrict__ Y,
                                                           float* __restrict__ P,
                                                           const int32_t* __restrict__ sorted_ids,
                                                           const int32_t* __restrict__ tile_expert,
                                                           int n_flat, int topk, int N, int K,
                                                           int lda, int ldy, int rows) {
  using T = MoeTile<BM>;
  constexpr int WN = T::WN, WCOLS = T::WCOLS, JN = T::JN, AR = T::AR;  // AR: per k-tile
  // one __shared__ object: [buf 2][A k-tile 0: BM rows | A k-tile 1: BM rows | W 128 rows]
  // [8 chunks of 16 B]
  constexpr int BUF = (2 * BM + MOE_BN) * 8;
  __shared__ u32x4 lds[2 * BUF];
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0) return;  // past the padded row count (graph-safe fixed grid); uniform exit
  const int m0 = tile * BM, n0 = blockIdx.y * MOE_BN;
  // host: kps % 64 == 0 and ceil(kps / 128) % PF == 0
  const int kps = K / gridDim.z, kbeg = blockIdx.z * kps, kend = kbeg + kps;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w / WN, wn = w % WN;
  const int fr = lane & 15, fg = lane >> 4;
  const int s_ch = tid & 7, s_r = tid >> 3;  // staging chunk / row (0..31)

  const bf16* xa[AR];
#pragma unroll
  for (int c = 0; c < AR; ++c)
    xa[c] = moe_a_row<GATHER>(A, sorted_ids, m0 + s_r + 32 * c, n_flat, topk, lda);
  const uint8_t* wb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int wrow = moe_wrow<SILU>(n0 + s_r + 32 * c, N);
    wb[c] = W + ((size_t)e * N + wrow) * K;
  }

  u32x4 sa[PF][2][AR], sb[PF][4];
  // k0 < kend always; the step's second k-tile exists unless the slice ends in a half step
  auto gload = [&](int q, int k0) {
    const bool full = k0 + 64 < kend;
#pragma unroll
    for (int c = 0; c < AR; ++c) {
      sa[q][0][c] = *reinterpret_cast<const u32x4*>(xa[c] + k0 + s_ch * 8);
      sa[q][1][c] = u32x4{0u, 0u, 0u, 0u};
      if (full) sa[q][1][c] = *reinterpret_cast<const u32x4*>(xa[c] + k0 + 64 + s_ch * 8);
    }
    const bool wl = full || s_ch < 4;  // lanes 4..7 of a row hold the second k-tile's bytes
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const u32x4* src = reinterpret_cast<const u32x4*>(wb[c] + k0 + s_ch * 16);
      sb[q][c] = u32x4{0u, 0u, 0u, 0u};
      if (wl) sb[q][c] = NTW ? __builtin_nontemporal_load(src) : *src;
    }
  };
  auto sstore = [&](int q, int buf) {
    moe_sstore_a2<BM>(&lds[buf * BUF], sa[q], s_r, s_ch);
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[buf * BUF + 2 * BM * 8 + swz8(s_r + 32 * c, s_ch)] = sb[q][c];
  };
  f32x4 acc[2][JN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // nks: k-tiles of the step to multiply (2, or 1 for the half step that ends a slice)
  auto mfma = [&](int buf, bool last) {
    const int nks = last && (kps & 127) ? 1 : 2;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks < nks) {
        bf16x8 a0[2], a1[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int row = wm * 32 + i * 16 + fr;
          a0[i] = __builtin_bit_cast(bf16x8, lds[buf * BUF + ks * BM * 8 + swz8(row, 2 * fg)]);
          a1[i] = __builtin_bit_cast(bf16x8, lds[buf * BUF + ks * BM * 8 + swz8(row, 2 * fg + 1)]);
        }
#pragma unroll
        for (int j = 0; j < JN; ++j) {
          const u32x4 q8 = lds[buf * BUF + 2 * BM * 8 + swz8(wn * WCOLS + j * 16 + fr, ks * 4 + fg)];
          const bf16x8 b0 = fp8x8_to_bf16x8(q8[0], q8[1]);
          const bf16x8 b1 = fp8x8_to_bf16x8(q8[2], q8[3]);
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0, acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1, acc[i][j], 0, 0, 0);
          }
        }
      }
    }
  };

  const int nk = (kps + 127) / 128;  // steps of this slice, the last maybe half
  MOE_RING(PF, 128, nk, kbeg, gload, sstore, mfma);

  // sc[j]: the scale of the weight row sub-tile j's column fr was read from (SILU: the
  // interleave maps sub-tile 2jj to gate row vb/2 + fr and 2jj+1 to up row N/2 + vb/2 + fr)
  const float* se = scale + (size_t)e * N;
  float sc[JN];
#pragma unroll
  for (int j = 0; j < JN; ++j) {
    const int v = n0 + wn * WCOLS + j * 16 + fr;  // virtual column
    sc[j] = v < N ? se[moe_wrow<SILU>(v, N)] : 0.f;
  }
#define MOEQ_SCALED(j, x) (sc[j] * (x))  // the scale before the first rounding
  MOE_TILE_EPILOGUE(MOEQ_SCALED)
#undef MOEQ_SCALED
}

struct MoeQgemmFamily {
  template <int BM, bool G, bool S, int PF, bool SPL, bool NT, typename... Args>
  static void launch(dim3 grid, hipStream_t s, Args... a) {
    moe_qgemm_kernel<BM, G, S, PF, SPL, NT><<<grid, 256, 0, s>>>(a...);
  }
};

void launch_moe_qgemm(const void* A, const void* Wq, const float* scale, void* Y,
                      const int32_t* sorted_ids, const int32_t* tile_expert, int max_tiles,
                      int n_flat, int topk, int N, int K, int lda, int ldy, int gather, int silu,
                      int pf, int bm, int splitk, float* partials, bool ntw, hipStream_t s) {
  moe_launch<MoeQgemmFamily>(max_tiles, N, splitk, bm, gather, silu, pf, ntw, s, (const bf16*)A,
                             (const uint8_t*)Wq, scale, (bf16*)Y, partials, sorted_ids,
                             tile_expert, n_flat, topk, N, K, lda, ldy);
}

}  // namespace akap
