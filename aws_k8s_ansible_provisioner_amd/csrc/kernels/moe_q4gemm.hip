// Grouped expert GEMM for MoE decode with MXFP4 (OCP e2m1 + e8m0) expert weights on gfx950:
// the 4-bit-weight form of moe_dgemm.hip (W4A16), q4gemm.hip's arithmetic inside
// moe_qgemm.hip's structure.
//
//   Y[r, n] = bf16( sum_k A[row(r), k] * e2m1(Wq[e, n, k]) * 2^(scale[e, n, k/32] - 127) )
//   e = tile_expert[tile(r)]
//
// Wq uint8 [E, N, K/2] packs two e2m1 codes per byte (element 2j in the low nibble), scale uint8
// [E, N, K/32] holds one e8m0 code (2..252) per 32 elements along K.  Everything moe_dgemm.hip
// and moe_qgemm.hip fix is kept: one expert per BM x 128 tile (BM 32 | 64), the uniform exit
// for tiles past the padded rows, GATHER through sorted_ids (padding rows read row 0), the
// gate/up-interleaved SILU epilogue, SPLIT over gridDim.z into fp32 partials for
// moe_combine_split, the compile-time load ring, no workspace and no cross-workgroup state
// (graph-capturable, bit-reproducible).
//
// What the 4-bit weights change:
//   * a k-step stays 128 deep.  A weight row of a step is then 64 B, staged by 4 lanes x 16 B;
//     the W tile in LDS is 128 rows x 4 chunks of 16 B (q4gemm.hip's 64-B-row swizzle) and
//     stays packed through HBM, L2 and LDS.  The activation rows of the step are two 64-deep
//     k-tiles as in moe_qgemm.hip.  (A 256-deep step would stage four A k-tiles: 96 KB of
//     double buffer at BM = 64, which does not fit two workgroups per CU.)
//   * a thread issues TWO 16-B weight loads per step, not four: at equal ring depth half the
//     weight bytes are in flight.  Ring depths 1, 2 and 4 are compiled.  Depth 8 is not: at
//     __launch_bounds__(256, 2) its 64-row variants spill 178 VGPRs (the ring alone is 200
//     registers).  The resource usage of each variant is in profiles/moe_mxfp4_weights.md.
//   * a slice whose depth is an odd multiple of 64 ends in a half step: the second k-tile and
//     the weight chunks 2..3 are not loaded (the registers hold zeros).  Unlike moe_qgemm.hip
//     the half step still runs all four MFMAs of a sub-tile, because each MFMA spans the whole
//     step (fragment order below): lane groups 2 and 3 multiply zeros by zeros, which adds +0.
//   * the scale codes ride the ring.  A step needs 4 codes per weight row and a half step 2.
//     DEVIATION from one 4-byte word per row: every thread loads ONE 2-byte pair (thread t:
//     tile row t / 2, pair t % 2; the odd threads idle in a half step).  A slice may begin at
//     an odd multiple of 64 (K = 384 split 2: byte 6 of a scale row), where a 4-byte load
//     would be misaligned; a pair is always 2-byte aligned (slices begin at multiples of 64)
//     and, K % 128 == 0, never runs past its row.  A code s becomes a float by s << 23.
//   * fragment k-order: lane group fg owns k in [32 fg, 32 fg + 32) of the step -- exactly one
//     scale block.  ONE ds_read_b128 of the packed row gives the B operands of four MFMAs
//     (word c = k 32 fg + 8 c .. + 8), all scaled by byte fg of the row's 4 codes; the A
//     operands are chunks 4 (fg & 1) + c of k-tile fg >> 1.  A and B agree on the order.
//   * the block scale is applied at the widening (v_cvt_scalef32_pk_bf16_fp4, exact): there is
//     no per-channel scale and no accumulator multiply; the epilogues are moe_dgemm.hip's.
#include "moe_gemm_common.h"

namespace akap {

template <int BM, bool GATHER, bool SILU, int PF, bool SPLIT, bool NTW = false>
__global__ __launch_bounds__(256, 2) void moe_q4gemm_kernel(const bf16* __restrict__ A,
                                                            const uint8_t* __restrict__ W,
                                                            const uint8_t* __restrict__ scale,
                                                            bf16* __restrict__ Y,
                                                            float* __restrict__ P,
                                                            const int32_t* __restrict__ sorted_ids,
                                                            const int32_t* __restrict__ tile_expert,
                                                            int n_flat, int topk, int N, int K,
                                                            int lda, int ldy, int rows) {
  using T = MoeTile<BM>;
  constexpr int WN = T::WN, WCOLS = T::WCOLS, JN = T::JN, AR = T::AR;  // AR: per k-tile
  // one __shared__ object, in 16-B units: [buf 2][A k-tile 0: BM rows x 8 | A k-tile 1: BM rows
  // x 8 | W: 128 rows x 4 | scale: 128 rows x 4 B = 32]
  constexpr int WOFF = 2 * BM * 8, SOFF = WOFF + MOE_BN * 4;
  constexpr int BUF = SOFF + MOE_BN / 4;
  __shared__ u32x4 lds[2 * BUF];
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0) return;  // past the padded row count (graph-safe fixed grid); uniform exit
  const int m0 = tile * BM, n0 = blockIdx.y * MOE_BN;
  // host: K % 128 == 0, kps % 64 == 0 and ceil(kps / 128) % PF == 0
  const int kps = K / gridDim.z, kbeg = blockIdx.z * kps, kend = kbeg + kps;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w / WN, wn = w % WN;
  const int fr = lane & 15, fg = lane >> 4;
  const int s_ch = tid & 7, s_r = tid >> 3;    // A staging chunk / row (0..31)
  const int w_ch = tid & 3, w_r = tid >> 2;    // W staging chunk / row (0..63)
  const int c_h = tid & 1, c_r = tid >> 1;     // scale staging pair / row (0..127)

  const bf16* xa[AR];
#pragma unroll
  for (int c = 0; c < AR; ++c)
    xa[c] = moe_a_row<GATHER>(A, sorted_ids, m0 + s_r + 32 * c, n_flat, topk, lda);
  const uint8_t* wb[2];
#pragma unroll
  for (int c = 0; c < 2; ++c)
    wb[c] = W + ((size_t)e * N + moe_wrow<SILU>(n0 + w_r + 64 * c, N)) * (K >> 1) + w_ch * 16;
  const uint8_t* cb = scale + ((size_t)e * N + moe_wrow<SILU>(n0 + c_r, N)) * (K >> 5) + c_h * 2;

  u32x4 sa[PF][2][AR], sb[PF][2];
  uint32_t sc[PF];
  // k0 < kend always; the step's second half exists unless the slice ends in a half step
  auto gload = [&](int q, int k0) {
    const bool full = k0 + 64 < kend;
#pragma unroll
    for (int c = 0; c < AR; ++c) {
      sa[q][0][c] = *reinterpret_cast<const u32x4*>(xa[c] + k0 + s_ch * 8);
      sa[q][1][c] = u32x4{0u, 0u, 0u, 0u};
      if (full) sa[q][1][c] = *reinterpret_cast<const u32x4*>(xa[c] + k0 + 64 + s_ch * 8);
    }
    const bool wl = full || w_ch < 2;  // chunks 2..3 of a row hold the second half's codes
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const u32x4* src = reinterpret_cast<const u32x4*>(wb[c] + (k0 >> 1));
      sb[q][c] = u32x4{0u, 0u, 0u, 0u};
      if (wl) sb[q][c] = NTW ? __builtin_nontemporal_load(src) : *src;
    }
    sc[q] = 0x7f7fu;  // idle pair: 2^0 for the zero codes of a half step
    if (full || c_h == 0) sc[q] = *reinterpret_cast<const uint16_t*>(cb + (k0 >> 5));
  };
  auto sstore = [&](int q, int buf) {
    moe_sstore_a2<BM>(&lds[buf * BUF], sa[q], s_r, s_ch);
#pragma unroll
    for (int c = 0; c < 2; ++c) lds[buf * BUF + WOFF + swz4_w(w_r + 64 * c, w_ch)] = sb[q][c];
    reinterpret_cast<uint16_t*>(&lds[buf * BUF + SOFF])[tid] = (uint16_t)sc[q];
  };
  f32x4 acc[2][JN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mfma = [&](int buf, bool) {
    const u32x4* xh = &lds[buf * BUF + (fg >> 1) * BM * 8];  // this lane group's k-tile
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(&lds[buf * BUF + SOFF]);
    bf16x8 a[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < 2; ++i)
        a[c][i] = __builtin_bit_cast(bf16x8, xh[swz8(wm * 32 + i * 16 + fr, 4 * (fg & 1) + c)]);
#pragma unroll
    for (int j = 0; j < JN; ++j) {
      const int wr = wn * WCOLS + j * 16 + fr;
      const u32x4 q4 = lds[buf * BUF + WOFF + swz4_w(wr, fg)];
      const float s = e8m0_to_f32((sw[wr] >> (8 * fg)) & 0xffu);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 b = fp4x8_to_bf16x8(q4[c], s);
#pragma unroll
        for (int i = 0; i < 2; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c][i], b, acc[i][j], 0, 0, 0);
      }
    }
  };

  const int nk = (kps + 127) / 128;  // steps of this slice, the last maybe half
  MOE_RING(PF, 128, nk, kbeg, gload, sstore, mfma);
  MOE_TILE_EPILOGUE(MOE_NO_SCALE)
}

struct MoeQ4gemmFamily {
  template <int BM, bool G, bool S, int PF, bool SPL, bool NT, typename... Args>
  static void launch(dim3 grid, hipStream_t s, Args... a) {
    moe_q4gemm_kernel<BM, G, S, PF, SPL, NT><<<grid, 256, 0, s>>>(a...);
  }
};

void launch_moe_q4gemm(const void* A, const void* Wq, const void* scale, void* Y,
                       const int32_t* sorted_ids, const int32_t* tile_expert, int max_tiles,
                       int n_flat, int topk, int N, int K, int lda, int ldy, int gather, int silu,
                       int pf, int bm, int splitk, float* partials, bool ntw, hipStream_t s) {
  moe_launch<MoeQ4gemmFamily>(max_tiles, N, splitk, bm, gather, silu, pf, ntw, s, (const bf16*)A,
                              (const uint8_t*)Wq, (const uint8_t*)scale, (bf16*)Y, partials,
                              sorted_ids, tile_expert, n_flat, topk, N, K, lda, ldy);
}

}  // namespace akap
