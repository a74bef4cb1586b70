// Grouped expert GEMM for MoE decode on gfx950 (Mixtral 8x7B: every expert's weights are
// streamed every step, ~2.8 GB per layer, so the kernel must run at the HBM rate).
//
//   Y[r] = A[row(r)] . W[e(tile(r))]^T     r over the expert-sorted, block-padded rows
//
// Tile = BM (32 | 64) rows x 128 columns, one expert per tile; the host picks BM from the
// expected rows per expert (T*top_k/E) so one tile usually covers an expert: a second tile
// of the same expert re-streams its weights, a half-empty tile wastes MFMA work only.  The
// wide N tile keeps the re-read activation traffic at 1/4 of the weight bytes (a 64x64 tile
// reads as many activation bytes as weight bytes through each CU's load path).  4 waves as
// WM x WN (moe_gemm_common.h MoeTile), BK = 64, full-line staging (8 lanes per 128-B row),
// PF k-tiles of loads in flight in registers (the compile-time ring of dgemm.hip,
// MOE_RING), XOR-swizzled LDS double buffer.
//
//   GATHER   row(r) = sorted_ids[r] / top_k (hidden-state rows; padding rows read row 0 and
//            their outputs are never combined), else row(r) = r
//   SILU     W = [gate; up] (N = 2F) read gate/up-interleaved in 16-row groups (dgemm.hip
//            EPI_SILU): Y[r, f] = bf16(bf16(silu(g)) * u), Y is [rows, F] -- the SwiGLU of
//            the expert FFN happens in the w13 GEMM's epilogue.
#include "moe_gemm_common.h"

namespace akap {

// SPLIT: K is split over gridDim.z; each slice writes fp32 partials P[z, row, col] (ldy = N)
// that moe_combine_split_kernel sums while combining (no extra launch).
template <int BM, bool GATHER, bool SILU, int PF, bool SPLIT, bool NTW = false>
__global__ __launch_bounds__(256, 2) void moe_dgemm_kernel(const bf16* __restrict__ A,
                                                           const bf16* __restrict__ W,
                                                           bf16* __restrict__ Y,
                                                           float* __restrict__ P,
                                                           const int32_t* __restrict__ sorted_ids,
                                                           const int32_t* __restrict__ tile_expert,
                                                           int n_flat, int topk, int N, int K,
                                                           int lda, int ldy, int rows) {
  using T = MoeTile<BM>;
  constexpr int WN = T::WN, WCOLS = T::WCOLS, JN = T::JN, AR = T::AR;
  // one __shared__ object: [buf 2][A BM rows | W 128 rows][8 chunks] bf16x8
  __shared__ bf16x8 lds[2 * (BM + MOE_BN) * 8];
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0) return;  // past the padded row count (graph-safe fixed grid); uniform exit
  const int m0 = tile * BM, n0 = blockIdx.y * MOE_BN;
  const int kps = K / gridDim.z, kbeg = blockIdx.z * kps;  // host: kps % (MBK * PF) == 0
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wm = w / WN, wn = w % WN;
  const int fr = lane & 15, fg = lane >> 4;
  const int s_ch = tid & 7, s_r = tid >> 3;  // staging chunk / row (0..31)

  const bf16* xa[AR];
#pragma unroll
  for (int c = 0; c < AR; ++c)
    xa[c] = moe_a_row<GATHER>(A, sorted_ids, m0 + s_r + 32 * c, n_flat, topk, lda);
  const bf16* wb[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int wrow = moe_wrow<SILU>(n0 + s_r + 32 * c, N);
    wb[c] = W + ((size_t)e * N + wrow) * K;
  }

  bf16x8 sa[PF][AR], sb[PF][4];
  auto gload = [&](int q, int k0) {
    const int kk = k0 + s_ch * 8;
#pragma unroll
    for (int c = 0; c < AR; ++c) sa[q][c] = *reinterpret_cast<const bf16x8*>(xa[c] + kk);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bf16x8* src = reinterpret_cast<const bf16x8*>(wb[c] + kk);
      sb[q][c] = NTW ? __builtin_nontemporal_load(src) : *src;
    }
  };
  constexpr int BUF = (BM + MOE_BN) * 8;
  auto sstore = [&](int q, int buf) {
#pragma unroll
    for (int c = 0; c < AR; ++c) lds[buf * BUF + swz8(s_r + 32 * c, s_ch)] = sa[q][c];
#pragma unroll
    for (int c = 0; c < 4; ++c) lds[buf * BUF + BM * 8 + swz8(s_r + 32 * c, s_ch)] = sb[q][c];
  };
  f32x4 acc[2][JN];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < JN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto mfma = [&](int buf, bool) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[2], bfr[JN];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = lds[buf * BUF + swz8(wm * 32 + i * 16 + fr, ks * 4 + fg)];
#pragma unroll
      for (int j = 0; j < JN; ++j)
        bfr[j] = lds[buf * BUF + BM * 8 + swz8(wn * WCOLS + j * 16 + fr, ks * 4 + fg)];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < JN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  };
  const int nk = kps / MBK;
  MOE_RING(PF, MBK, nk, kbeg, gload, sstore, mfma);
  MOE_TILE_EPILOGUE(MOE_NO_SCALE)
}

// out[t] = sum_k w[t,k] * sum_z P[z, inv[t*K+k]]  (fp32 partial slices of the down GEMM)
__global__ __launch_bounds__(256) void moe_combine_split_kernel(const float* __restrict__ P,
                                                                const float* __restrict__ wts,
                                                                const int32_t* __restrict__ inv,
                                                                bf16* __restrict__ out, int T,
                                                                int topk, int d, int S,
                                                                int rows) {
  const int vpr = d / 8;
  const long total = (long)T * vpr;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    int t, c;  // 32-bit split when it fits (no 64-bit division per element)
    if (total < (1L << 30)) {
      t = (int)i / vpr;
      c = ((int)i - t * vpr) * 8;
    } else {
      t = (int)(i / vpr);
      c = (int)(i % vpr) * 8;
    }
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < topk; ++k) {
      const int pos = inv[(size_t)t * topk + k];
      if (pos < 0) continue;  // skipped (expert-parallel padding) row
      const float wk = wts[(size_t)t * topk + k];
      const size_t r = (size_t)pos;
      for (int z = 0; z < S; ++z) {
        const f32x4* p = reinterpret_cast<const f32x4*>(P + ((size_t)z * rows + r) * d + c);
        const f32x4 a = p[0], b = p[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j] += wk * a[j];
          acc[4 + j] += wk * b[j];
        }
      }
    }
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(acc[j]);
    *reinterpret_cast<bf16x8*>(out + (size_t)t * d + c) = o;
  }
}

void launch_moe_combine_split(const float* P, const float* wts, const int32_t* inv, void* out,
                              int T, int topk, int d, int S, int rows, hipStream_t s) {
  if (T == 0) return;
  long blocks = ((long)T * (d / 8) + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  moe_combine_split_kernel<<<(int)blocks, 256, 0, s>>>(P, wts, inv, (bf16*)out, T, topk, d, S,
                                                       rows);
}

struct MoeDgemmFamily {
  template <int BM, bool G, bool S, int PF, bool SPL, bool NT, typename... Args>
  static void launch(dim3 grid, hipStream_t s, Args... a) {
    moe_dgemm_kernel<BM, G, S, PF, SPL, NT><<<grid, 256, 0, s>>>(a...);
  }
};

void launch_moe_dgemm(const void* A, const void* W, void* Y, const int32_t* sorted_ids,
                      const int32_t* tile_expert, int max_tiles, int n_flat, int topk, int N,
                      int K, int lda, int ldy, int gather, int silu, int pf, int bm, int splitk,
                      float* partials, bool ntw, hipStream_t s) {
  moe_launch<MoeDgemmFamily>(max_tiles, N, splitk, bm, gather, silu, pf, ntw, s, (const bf16*)A,
                             (const bf16*)W, (bf16*)Y, partials, sorted_ids, tile_expert, n_flat,
                             topk, N, K, lda, ldy);
}

}  // namespace akap
