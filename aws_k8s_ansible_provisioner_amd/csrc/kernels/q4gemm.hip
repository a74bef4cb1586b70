// MXFP4-weight decode GEMM for gfx950 (W4A16):
//   Y[M,N] = bf16( sum_k X[M,K] (bf16) * e2m1(Wq[N,K]) * 2^(scale[N,K/32] - 127) ),  M <= 256,
// and the dequantizer the prefill path uses (out[n,k] = bf16(e2m1(q[n,k]) * 2^(scale - 127))).
//
// Wq packs two OCP e2m1 codes per byte (element 2j in the low nibble of byte j), scale holds one
// e8m0 code per 32 elements along K, 2 <= code <= 252.  In that range every dequantized value
// is a normal bf16 number, so -- as in qgemm.hip -- the weights stay narrow where bytes cost
// (HBM, L2, LDS) and are widened in registers right before v_mfma_f32_16x16x32_bf16:
// v_cvt_scalef32_pk_bf16_fp4 turns one byte into two bf16 and multiplies by the block scale,
// whose fp32 operand is simply code << 23.  The scale is per 32-deep block, so it is applied
// HERE, inside the K loop; the epilogue only rounds the fp32 sums to bf16.
//
// Geometry and staging are qgemm.hip's: a 4-wave workgroup owns a BM x BN output tile, wave w
// takes the k-steps w, w + 4, ... through a private NS-slot LDS-DMA ring with no barrier in the
// K loop, and the four partial tiles are summed through LDS -- no workspace, tickets or
// atomics.  What differs is the k-step: 128 deep, so that a weight row in a slot is 64 B and
// one DMA instruction moves 16 rows x 64 B exactly as in qgemm (a 64-deep step would be a 32-B
// row: twice the DMA instructions per byte, and DMA instructions in flight per CU are what
// bound the fp8 kernel, profiles/fp8_weights.md).  A slot holds
//   X:     2 halves x BM rows x 128 B (k 0..63 | 64..127), each half laid out and swizzled
//          (swz8) as qgemm's X slot, 8 rows per DMA instruction;
//   Wq:    BN rows x 64 B, 16 rows per instruction, qgemm's 64-B-row swizzle;
//   scale: 64 x 4 B, ONE 4-byte-per-lane DMA instruction: lane r brings the step's 4 codes
//          of tile row r (lanes past BN or N re-read row 0).
// The codes ride the ring, so the K loop has no ordinary load whose use would make the
// compiler drain vmcnt(0) under the DMAs in flight.
//
// Fragment k-order: lane group fg of a 128-deep step owns k in [32 fg, 32 fg + 32) -- exactly
// one scale block.  ONE ds_read_b128 of the fp4 row gives the B operands of four MFMAs (word c
// = k 32 fg + 8 c .. + 8), all scaled by byte fg of the row's scale word; the A operands are
// the X chunks 4 fg + c, i.e. chunks 4 (fg & 1) + c of half fg >> 1.  A and B agree on the
// order, which is all an MFMA needs.
#include "qgemm_common.h"

namespace akap {

template <int MI, int NJ, int NS>
__global__ __launch_bounds__(256, 1) void q4gemm_kernel(Q4GemmArgs p) {
  constexpr int BM = 16 * MI, BN = 16 * NJ;
  constexpr int GH = BM / 8;             // X DMA instructions per 64-deep half
  constexpr int GA = 2 * GH;             // X DMA instructions per step
  constexpr int GW = BN / 16;            // Wq DMA instructions per step
  constexpr int G = GA + GW + 1;         // + the scale words
  constexpr int XU = BM * 16, WU = BN * 4;  // 16-B units of a slot's X and Wq parts
  constexpr int SU = XU + WU + 16;       // + 64 scale words
  constexpr int PB = BN + 4;             // combine row pitch (fp32): fg groups on distinct banks
  static_assert(4 * BM * PB * 4 <= 4 * NS * SU * 16, "combine buffer fits in the rings");
  static_assert(4 * NS * SU * 16 <= 160 * 1024, "rings fit in LDS");
  static_assert(NS >= 2 && G * (NS - 1) < 63, "vmcnt counts every DMA in flight");
  __shared__ bf16x8 lds[4 * NS * SU];

  QGEMM_TILE_PROLOGUE(Q4BK)
  const bf16* X = static_cast<const bf16*>(p.X);
  const uint8_t* Wq = static_cast<const uint8_t*>(p.Wq);
  const uint8_t* Sc = static_cast<const uint8_t*>(p.scale);
  bf16x8* ring = lds + w * NS * SU;

  // per-lane DMA sources (qgemm_common.h); the X sources are of one 64-deep half.  Scale: lane
  // -> tile row L (lanes past BN or N re-read row 0)
  const bf16* asrc[GH];
  const uint8_t* wsrc[GW];
  const uint8_t* ssrc;
  {
#pragma unroll
    for (int i = 0; i < GH; ++i) asrc[i] = qgemm_x_src<Q4BK>(X, m0 + i * 8, p.M, p.ldx, w, lane);
    QGEMM_W_SRC(p.K / 2, Q4BK / 2)
    const int sv = n0 + lane;
    ssrc = Sc + (size_t)(lane < BN && sv < p.N ? sv : 0) * (p.K / MXBLK) + w * (Q4BK / MXBLK);
  }
  auto issue = [&](int s) {
    bf16x8* slot = ring + (s % NS) * SU;
    const int k0 = s * 4 * Q4BK;
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int i = 0; i < GH; ++i) glds16(asrc[i] + k0 + h * 64, slot + (h * GH + i) * 64);
    // every weight byte is read by one workgroup per row tile: non-temporal, as wgemm.hip
#pragma unroll
    for (int j = 0; j < GW; ++j) glds16<kAuxNT>(wsrc[j] + k0 / 2, slot + XU + j * 64);
    glds4(ssrc + k0 / MXBLK, slot + XU + WU);
  };

  QGEMM_ACC(acc);
  QGEMM_RING_PRIME(NS, n, issue);
  for (int t = 0; t < n; ++t) {
    QGEMM_RING_ADVANCE(NS, G, t, n, issue);
    const bf16x8* slot = ring + (t % NS) * SU;
    const bf16x8* xh = slot + (fg >> 1) * (BM * 8);     // this lane group's 64-deep half
    const u32x4* wslot = reinterpret_cast<const u32x4*>(slot + XU);
    const uint32_t* sslot = reinterpret_cast<const uint32_t*>(slot + XU + WU);
    bf16x8 a[4][MI];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int i = 0; i < MI; ++i) a[c][i] = xh[swz8(i * 16 + fr, 4 * (fg & 1) + c)];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const u32x4 q = wslot[swz4_w(j * 16 + fr, fg)];
      const float sc = e8m0_to_f32((sslot[j * 16 + fr] >> (8 * fg)) & 0xffu);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 b = fp4x8_to_bf16x8(q[c], sc);
#pragma unroll
        for (int i = 0; i < MI; ++i)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[c][i], b, acc[i][j], 0, 0, 0);
      }
    }
  }

  float* part = reinterpret_cast<float*>(lds);
  qgemm_combine(part, acc, w, fr, fg);
  QGEMM_STORE_EPILOGUE(false)  // the block scales were applied in the K loop
}

void launch_q4gemm(const Q4GemmArgs& p, hipStream_t st) {
  if (p.M == 0 || p.N == 0) return;
  const QGemmGeom g = q4gemm_geometry(p.M, p.N, p.K);
  // ring depth: as many slots as LDS holds -- a 16-row tile is a pure weight stream, bound by
  // the bytes its DMAs keep in flight; 64-row tiles are left with a double buffer
#define AKAP_Q4GEMM_CASE(MI_, NJ_, NS_) \
  q4gemm_kernel<MI_, NJ_, NS_><<<g.grid, 256, 0, st>>>(p)
  if (g.bm == 16) {
    if (g.bn == 16) AKAP_Q4GEMM_CASE(1, 1, 7);
    else if (g.bn == 32) AKAP_Q4GEMM_CASE(1, 2, 6);
    else AKAP_Q4GEMM_CASE(1, 4, 4);
  } else if (g.bm == 32) {
    if (g.bn == 32) AKAP_Q4GEMM_CASE(2, 2, 3);
    else AKAP_Q4GEMM_CASE(2, 4, 3);
  } else {
    AKAP_Q4GEMM_CASE(4, 2, 2);  // 64-row tiles are 32 columns wide (q4gemm_geometry)
  }
#undef AKAP_Q4GEMM_CASE
}

// ---- dequantizer: out[n, k] = bf16(e2m1(q[n, k]) * 2^(scale[n, k/32] - 127)) ----------------
// One thread per scale block: a 16-byte load of 32 codes, one scale byte, four 16-byte stores.
__global__ __launch_bounds__(256) void dequant_mxfp4_kernel(const uint8_t* __restrict__ q,
                                                            const uint8_t* __restrict__ scale,
                                                            bf16* __restrict__ out, long blocks) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < blocks; e += stride) {
    const float s = e8m0_to_f32(scale[e]);
    const u32x4 v = ld_nt(reinterpret_cast<const u32x4*>(q) + e);
    bf16x8* dst = reinterpret_cast<bf16x8*>(out) + 4 * e;
#pragma unroll
    for (int c = 0; c < 4; ++c) dst[c] = fp4x8_to_bf16x8(v[c], s);
  }
}

void launch_dequant_mxfp4(const void* q, const void* scale, void* out, long N, int K,
                          hipStream_t st) {
  const long blocks = N * (K / MXBLK);
  if (blocks == 0) return;
  dequant_mxfp4_kernel<<<dequant_grid(blocks), 256, 0, st>>>(static_cast<const uint8_t*>(q),
                                             static_cast<const uint8_t*>(scale),
                                             static_cast<bf16*>(out), blocks);
}

}  // namespace akap
