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
#include "gemm_common.h"

namespace akap {

// X rows (128 B) use swz8.  W rows of 64 B: chunk c stored at c ^ g((row >> 2) & 3),
// g = {0, 2, 3, 1} (wgemm.hip ww_swz)
__device__ __forceinline__ int qswz_g(int row) { return (0x1320 >> (4 * ((row >> 2) & 3))) & 3; }
__device__ __forceinline__ int qswz_w(int row, int c) { return row * 4 + (c ^ qswz_g(row)); }

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

  const int tiles_m = (p.M + BM - 1) / BM;
  const int tiles_n = (p.N + BN - 1) / BN;
  const int lt = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  const int tn = lt / tiles_m, tm = lt % tiles_m;  // a column tile's row tiles share an XCD
  const int m0 = tm * BM, n0 = tn * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  // the wave index in a scalar register: the step count and the ring base are wave-uniform
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const int nk = p.K / QBK;
  const int n = w < nk ? (nk - w + 3) / 4 : 0;  // this wave's steps: k0 = (w + 4 s) * 64
  const bf16* X = static_cast<const bf16*>(p.X);
  const uint8_t* Wq = static_cast<const uint8_t*>(p.Wq);
  bf16x8* ring = lds + w * NS * SU;

  // per-lane DMA sources.  X: one instruction = 8 rows x 128 B, lane -> row L / 8, LDS chunk
  // L % 8 holding logical chunk (L % 8) ^ (L / 8).  Wq: one instruction = 16 rows x 64 B, lane
  // -> row L / 4, LDS chunk L % 4 holding logical chunk (L % 4) ^ g.  Rows past M / N re-read
  // row 0 (never stored).
  const bf16* asrc[GA];
  const uint8_t* wsrc[GW];
  {
    const int lr = lane >> 3, lc = (lane & 7) ^ lr;
#pragma unroll
    for (int i = 0; i < GA; ++i) {
      const int row = m0 + i * 8 + lr;
      asrc[i] = X + (size_t)(row < p.M ? row : 0) * p.ldx + w * QBK + lc * 8;
    }
    const int wr = lane >> 2, wc = (lane & 3) ^ qswz_g(wr);
#pragma unroll
    for (int j = 0; j < GW; ++j) {
      const int v = n0 + j * 16 + wr;
      wsrc[j] = Wq + (size_t)(v < p.N ? v : 0) * p.K + w * QBK + wc * 16;
    }
  }
  auto issue = [&](int s) {
    bf16x8* slot = ring + (s % NS) * SU;
    const int k0 = s * 4 * QBK;
#pragma unroll
    for (int i = 0; i < GA; ++i) glds16(asrc[i] + k0, slot + i * 64);
    // every weight byte is read by one workgroup per row tile: non-temporal, as wgemm.hip
#pragma unroll
    for (int j = 0; j < GW; ++j) glds16<kAuxNT>(wsrc[j] + k0, slot + BM * 8 + j * 64);
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
    const u32x4* wslot = reinterpret_cast<const u32x4*>(slot + BM * 8);
    bf16x8 a0[MI], a1[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      a0[i] = slot[swz8(i * 16 + fr, 2 * fg)];
      a1[i] = slot[swz8(i * 16 + fr, 2 * fg + 1)];
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const u32x4 q = wslot[qswz_w(j * 16 + fr, fg)];
      const bf16x8 b0 = fp8x8_to_bf16x8(q[0], q[1]);
      const bf16x8 b1 = fp8x8_to_bf16x8(q[2], q[3]);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0[i], b0, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1[i], b1, acc[i][j], 0, 0, 0);
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

  // scale + bf16 + 16-byte row-segment stores (N % 8 == 0: a segment is inside N or outside)
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
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(p.scale + col);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(p.scale + col + 4);
    bf16x8 o;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      o[q] = f2bf(lo[q] * s0[q]);
      o[4 + q] = f2bf(hi[q] * s1[q]);
    }
    *reinterpret_cast<bf16x8*>(Y + (size_t)row * p.ldy + col) = o;
  }
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
  const long blocks = (chunks + 255) / 256;
  const int grid = (int)(blocks < 8192 ? blocks : 8192);
  dequant_fp8_kernel<<<grid, 256, 0, st>>>(static_cast<const uint8_t*>(q), scale,
                                           static_cast<bf16*>(out), chunks, K / 16);
}

}  // namespace akap
