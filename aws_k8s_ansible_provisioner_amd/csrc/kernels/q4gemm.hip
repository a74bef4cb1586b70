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
#include "gemm_common.h"

namespace akap {

// LDS-DMA, 4 B per lane from g to lds_wave_base + 4 * lane
__device__ __forceinline__ void glds4(const void* g, void* lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)lds_wave_base, 4, 0, 0);
}

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

  const int tiles_m = (p.M + BM - 1) / BM;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int lt = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tn = lt / tiles_m, tm = lt % tiles_m;  // a column tile's row tiles share an XCD
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  // the wave index in a scalar register: the step count and the ring base are wave-uniform
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nk = p.K / Q4BK;
  const int n = w < nk ? (nk - w + 3) / 4 : 0;  // this wave's steps: k0 = (w + 4 s) * 128
  const bf16* X = static_cast<const bf16*>(p.X);
  const uint8_t* Wq = static_cast<const uint8_t*>(p.Wq);
  const uint8_t* Sc = static_cast<const uint8_t*>(p.scale);
  bf16x8* ring = lds + w * NS * SU;

  // per-lane DMA sources.  X: one instruction = 8 rows x 128 B of one half, lane -> row L / 8,
  // LDS chunk L % 8 holding logical chunk (L % 8) ^ (L / 8).  Wq: one instruction = 16 rows x
  // 64 B, lane -> row L / 4, LDS chunk L % 4 holding logical chunk (L % 4) ^ g.  Scale: lane ->
  // tile row L.  Rows past M / N re-read row 0 (never stored).
  const bf16* asrc[GH];
  const uint8_t* wsrc[GW];
  const uint8_t* ssrc;
  {
    const int lr = lane >> 3, lc = (lane & 7) ^ lr;
#pragma unroll
    for (int i = 0; i < GH; ++i) {
      const int row = m0 + i * 8 + lr;
      asrc[i] = X + (size_t)(row < p.M ? row : 0) * p.ldx + w * Q4BK + lc * 8;
    }
    const int wr = lane >> 2, wc = (lane & 3) ^ q4swz_g(wr);
#pragma unroll
    for (int j = 0; j < GW; ++j) {
      const int v = n0 + j * 16 + wr;
      wsrc[j] = Wq + (size_t)(v < p.N ? v : 0) * (p.K / 2) + w * (Q4BK / 2) + wc * 16;
    }
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

  f32x4 acc[MI][NJ];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < n) issue(s);
  for (int t = 0; t < n; ++t) {
    // retire this wave's DMAs of step t (steps t+1 .. t+NS-2 stay in flight when they exist);
    // the reads below are of this wave's own DMAs, so no barrier is needed
    if (t + NS - 2 < n) wait_vm<G * (NS - 2)>();
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // step t-1's fragment reads returned
    if (t + NS - 1 < n) issue(t + NS - 1);              // ... so its slot can be refilled
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
      const u32x4 q = wslot[q4swz_w(j * 16 + fr, fg)];
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

  // ---- sum the 4 waves' partial tiles through LDS: part[w][row][PB] fp32 ----
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // no wave reads or fills its ring any more
  float* part = reinterpret_cast<float*>(lds);
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        part[(w * BM + i * 16 + fg * 4 + r) * PB + j * 16 + fr] = acc[i][j][r];
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  // bf16 + 16-byte row-segment stores (N % 8 == 0: a segment is inside N or outside)
  bf16* Y = static_cast<bf16*>(p.Y);
  constexpr int CPR = BN / 8;
  for (int e = tid; e < BM * CPR; e += 256) {
    const int rr = e / CPR, cc = e % CPR;
    const int row = m0 + rr, col = n0 + cc * 8;
    if (row >= p.M || col >= p.N) continue;
    f32x4 lo = *reinterpret_cast<const f32x4*>(&part[rr * PB + cc * 8]);
    f32x4 hi = *reinterpret_cast<const f32x4*>(&part[rr * PB + cc * 8 + 4]);
#pragma unroll
    for (int ww = 1; ww < 4; ++ww) {
      lo += *reinterpret_cast<const f32x4*>(&part[(ww * BM + rr) * PB + cc * 8]);
      hi += *reinterpret_cast<const f32x4*>(&part[(ww * BM + rr) * PB + cc * 8 + 4]);
    }
    bf16x8 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[q] = f2bf(lo[q]);
      o[4 + q] = f2bf(hi[q]);
    }
    *reinterpret_cast<bf16x8*>(Y + (size_t)row * p.ldy + col) = o;
  }
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
  const long wgs = (blocks + 255) / 256;
  const int grid = (int)(wgs < 8192 ? wgs : 8192);
  dequant_mxfp4_kernel<<<grid, 256, 0, st>>>(static_cast<const uint8_t*>(q),
                                             static_cast<const uint8_t*>(scale),
                                             static_cast<bf16*>(out), blocks);
}

}  // namespace akap
