// FP8-weight decode GEMM for gfx950 (W8A16):
//   Y[M,N] = bf16( scale[n] * sum_k X[M,K] (bf16) * Wq[N,K] (OCP e4m3fn bytes) ),  M <= 256,
// and the dequantizer the prefill path uses (out[n,k] = bf16(float(q[n,k]) * scale[n])).
//
// Non-scaled fp8 MFMA runs at the bf16 rate on gfx950 and every e4m3 value is exact in bf16,
// so the weights stay 1 byte only where it pays -- HBM, L2 and LDS -- and are widened to bf16
// in registers (fp8x8_to_bf16x8) right before v_mfma_f32_16x16x32_bf16.  The per-channel
// scale multiplies the fp32 accumulators in the epilogue.
//
// Geometry: a workgroup of 4 waves owns a BM x BN output tile (BM = 16 | 32 | 64 rows,
// BN = 16 | 32 | 64 columns) and the K dimension is split INSIDE the workgroup as in kgemm.hip:
// wave w takes the 64-deep k-steps w, w + 4, w + 8, ...  and the four partial tiles are
// summed through LDS at the end -- no global partials, tickets, atomics or workspace, so a
// launch is graph-capturable and bit-reproducible.  Small column tiles keep the chip full on
// the narrow projections (N = 1,024 at M = 256: 128 workgroups; N = 4,096 at M <= 16: 256).
//
// Staging: each wave stages ITS OWN k-steps by global_load_lds into a private NS-slot ring
// (X: BM rows x 128 B, 8 rows per DMA instruction, chunk ^ (row & 7) as wgemm.hip; Wq: BN rows
// x 64 B, 16 rows per instruction, the 64-B-row swizzle of wgemm_wide_kernel; both on the
// per-lane SOURCE address and on the fragment reads, cdna_hip_programming.md rule 21).  A
// wave reads only what it staged, so its own counted `s_waitcnt vmcnt` orders the reads and
// the K loop has no barrier at all: the four waves are independent streams.
//
// Fragment k-order: the lane group fg of a 64-deep k-step owns k in [16 fg, 16 fg + 16): ONE
// ds_read_b128 of the fp8 row gives the B operands of both MFMAs (low 8 bytes, high 8 bytes)
// and the A operands are X chunks 2 fg and 2 fg + 1.  A and B agree on the order, which is all
// an MFMA needs.
#include "qgemm_common.h"

namespace akap {

// X rows (128 B) use swz8, W rows of 64 B swz4_w (gemm_common.h)
template <int MI, int NJ, int NS>
__global__ __launch_bounds__(256, 1) void qgemm_kernel(QGemmArgs p) {
  constexpr int BM = 16 * MI, BN = 16 * NJ;
  constexpr int GA = BM / 8;             // X DMA instructions per step
  constexpr int GW = BN / 16;            // Wq DMA instructions per step
  constexpr int G = GA + GW;
  constexpr int SU = BM * 8 + BN * 4;    // 16-B units per ring slot
  constexpr int PB = BN + 4;             // combine row pitch (fp32): fg groups on distinct banks
  static_assert(4 * BM * PB * 4 <= 4 * NS * SU * 16, "combine buffer fits in the rings");
  static_assert(NS >= 3, "two steps in flight");
  __shared__ bf16x8 lds[4 * NS * SU];

  QGEMM_TILE_PROLOGUE(QBK)
  const bf16* X = static_cast<const bf16*>(p.X);
  const uint8_t* Wq = static_cast<const uint8_t*>(p.Wq);
  bf16x8* ring = lds + w * NS * SU;

  const bf16* asrc[GA];  // per-lane DMA sources (qgemm_common.h)
  const uint8_t* wsrc[GW];
#pragma unroll
  for (int i = 0; i < GA; ++i) asrc[i] = qgemm_x_src<QBK>(X, m0 + i * 8, p.M, p.ldx, w, lane);
  QGEMM_W_SRC(p.K, QBK)
  auto issue = [&](int s) {
    bf16x8* slot = ring + (s % NS) * SU;
    const int k0 = s * 4 * QBK;
#pragma unroll
    for (int i = 0; i < GA; ++i) glds16(asrc[i] + k0, slot + i * 64);
    // every weight byte is read by one workgroup per row tile: non-temporal, as wgemm.hip
#pragma unroll
    for (int j = 0; j < GW; ++j) glds16<kAuxNT>(wsrc[j] + k0, slot + BM * 8 + j * 64);
  };

  QGEMM_ACC(acc);
  QGEMM_RING_PRIME(NS, n, issue);
  for (int t = 0; t < n; ++t) {
    QGEMM_RING_ADVANCE(NS, G, t, n, issue);
    const bf16x8* slot = ring + (t % NS) * SU;
    const u32x4* wslot = reinterpret_cast<const u32x4*>(slot + BM * 8);
    bf16x8 a0[MI], a1[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      a0[i] = slot[swz8(i * 16 + fr, 2 * fg)];
      a1[i] = slot[swz8(i * 16 + fr, 2 * fg + 1)];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const u32x4 q = wslot[swz4_w(j * 16 + fr, fg)];
      const bf16x8 b0 = fp8x8_to_bf16x8(q[0], q[1]);
      const bf16x8 b1 = fp8x8_to_bf16x8(q[2], q[3]);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1, acc[i][j], 0, 0, 0);
      }
    }
  }

  float* part = reinterpret_cast<float*>(lds);
  qgemm_combine(part, acc, w, fr, fg);
  QGEMM_STORE_EPILOGUE(true)
}

void launch_qgemm(const QGemmArgs& p, hipStream_t st) {
  if (p.M == 0 || p.N == 0) return;
  const QGemmGeom g = qgemm_geometry(p.M, p.N, p.K);
  // ring depth: 4 slots (three steps in flight) up to 32 rows, 3 slots for 64-row tiles (LDS)
#define AKAP_QGEMM_CASE(MI_, NJ_, NS_) \
  qgemm_kernel<MI_, NJ_, NS_><<<g.grid, 256, 0, st>>>(p)
  if (g.bn == 16) {
    AKAP_QGEMM_CASE(1, 1, 4);  // 16-row tiles only (qgemm_geometry)
  } else if (g.bn == 32) {
    if (g.bm == 16) AKAP_QGEMM_CASE(1, 2, 4);
    else if (g.bm == 32) AKAP_QGEMM_CASE(2, 2, 4);
    else AKAP_QGEMM_CASE(4, 2, 3);
  } else {
    if (g.bm == 16) AKAP_QGEMM_CASE(1, 4, 4);
    else if (g.bm == 32) AKAP_QGEMM_CASE(2, 4, 4);
    else AKAP_QGEMM_CASE(4, 4, 3);
  }
#undef AKAP_QGEMM_CASE
}

// ---- dequantizer: out[n, k] = bf16(float(q[n, k]) * scale[n]) -------------------------------
// One thread per 16 weights: a 16-byte load, one fp32 multiply per element, the bf16 cast
// (round to nearest even) and two 16-byte stores.
__global__ __launch_bounds__(256) void dequant_fp8_kernel(const uint8_t* __restrict__ q,
                                                          const float* __restrict__ scale,
                                                          bf16* __restrict__ out, long chunks,
                                                          int cpr) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < chunks; e += stride) {
    const float s = scale[e / cpr];
    const u32x4 v = ld_nt(reinterpret_cast<const u32x4*>(q) + e);
    const bf16x8 a = fp8x8_to_bf16x8(v[0], v[1]);
    const bf16x8 b = fp8x8_to_bf16x8(v[2], v[3]);
    bf16x8 oa, ob;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      oa[i] = f2bf(bf2f(a[i]) * s);
      ob[i] = f2bf(bf2f(b[i]) * s);
    }
    bf16x8* dst = reinterpret_cast<bf16x8*>(out) + 2 * e;
    dst[0] = oa;
    dst[1] = ob;
  }
}

void launch_dequant_fp8(const void* q, const float* scale, void* out, long N, int K,
                        hipStream_t st) {
  const long chunks = N * (K / 16);
  if (chunks == 0) return;
  dequant_fp8_kernel<<<dequant_grid(chunks), 256, 0, st>>>(static_cast<const uint8_t*>(q), scale,
                                           static_cast<bf16*>(out), chunks, K / 16);
}

}  // namespace akap
