// The host-side contract of the kernels: which shapes and variants a launch accepts, how large
// its fp32 workspace and ticket array must be, and the layout constants both sides of a launch
// agree on.  Plain C++17 (no HIP, no torch): kernels.h includes it for the kernels and ops.cpp,
// and csrc/runtime/bindings.cpp exposes it to Python (`_runtime.contract`), so the bindings'
// checks, the tuner's enumeration, the engine's workspace sizing and the tests ask one function.
#pragma once

#include <stddef.h>

namespace akap {

// Ints per in-launch ticket counter: each counter on its own 128-B L2 line.  Atomics (and the
// relaxed polls of a spinning combine) on one line serialise at one L2 channel -- 1024 row
// tickets packed 32 to a line cost the sampler ~18 us at B = 16 (tools/sample_bench.py, s5c).
constexpr int kCtrStride = 32;
// the shared GEMM counter array (ops.gemm_counters): its size and the combine-timeout flag
constexpr int kCtrInts = 1 << 18;
constexpr int kCtrErr = kCtrInts - 1;

// longest decode split-KV partition: 64 wave steps of 128 tokens, one cache block id per step
constexpr int kDecodeMaxPart = 8192;

enum { PRO_PLAIN = 0, PRO_ADDNORM = 1, PRO_SILU = 2 };
enum { EPI_STORE = 0, EPI_RESNORM = 1, EPI_SILU = 2 };

// ---- tile constants the predicates below share with their kernels ----
constexpr int GBM = 64, GBN = 64, GBK = 64;  // gemm.hip tiles; gdgemm.hip k-step
constexpr int DBM = 64, DBN = 64, DBK = 64;  // dgemm.hip
constexpr int KBN = 32;                      // kgemm.hip: output columns per workgroup
constexpr int KST = 256;                     // kgemm.hip: K per stage (4 waves x 64)
constexpr int MBK = 64;                      // moe_dgemm.hip k-step
constexpr int PG_T = 256;                    // pgemm.hip: tile rows / cols
constexpr int PG_BK = 64;                    // pgemm.hip: K tile
constexpr int QBK = 64;                      // qgemm.hip: k per wave step
constexpr int QGEMM_MAX_M = 256;             // rows one qgemm launch covers
constexpr int Q4BK = 128;                    // q4gemm.hip: k per wave step (a 64-B fp4 row)
constexpr int MXBLK = 32;                    // MXFP4: elements along K per e8m0 scale
constexpr int Q4GEMM_MAX_M = 256;            // rows one q4gemm launch covers
constexpr int WBK = 64;                      // wgemm.hip k-step
constexpr int kRouterMaxE = 16;              // moe.hip fused router: experts

// ---- sampling.hip ----
constexpr int kMaxChunks = 64;  // chunks (workgroups) per row
constexpr int kSelWords = 16;   // per-row state of the filter passes (32-bit words)
// per-row histogram area of the filter passes, in float2: kMaxChunks x 512 pairs (pass B
// publishes two 256-bin sets per chunk)
constexpr int kHistRow = kMaxChunks * 512;
constexpr int kMaxTiles = 64;   // 2048-element tiles per chunk: chunk <= 131072 elements
// longest row the sampler covers: kMaxChunks chunks x kMaxTiles tiles x 2048 elements
constexpr long kSampleMaxVocab = 64L * 64 * 2048;

// fp32 workspace floats of a sampler launch: partial records, selection states, per-row
// histograms (kMaxChunks x 512 float2), the draw rows' tile masses (kMaxChunks x kMaxTiles)
inline long sample_ws_floats(int B) {
  return (long)B * (kMaxChunks * 8 + kSelWords + 2 * kHistRow + kMaxChunks * kMaxTiles);
}

// ---- gemm.hip ----
// split-K factor: enough 64 x 64 tiles x slices to cover 256 CUs, each slice >= 256 of K
inline int gemm_splitk_choice(int M, int N, int K) {
  const int tiles = ((M + GBM - 1) / GBM) * ((N + GBN - 1) / GBN);
  int s = 1;
  while (tiles * s < 256 && K / (s * 2) >= 256) s *= 2;
  return s;
}

// ---- dgemm.hip / gdgemm.hip ----
// split-K factors with a compiled reduce (1, 2, 4, 8, 16)
inline bool dgemm_splitk_ok(int splitk) {
  return splitk == 1 || splitk == 2 || splitk == 4 || splitk == 8 || splitk == 16;
}

inline bool dgemm_supported(int M, int N, int K, int splitk, int pf) {
  if (M <= 0 || N <= 0 || K <= 0 || !dgemm_splitk_ok(splitk) || N % 4) return false;
  if (pf != 1 && pf != 2 && pf != 4 && pf != 8) return false;
  if (K % splitk) return false;
  const int kps = K / splitk;
  return kps % (DBK * pf) == 0;
}

// epilogues of a launch whose K slices meet in the separate reduce pass (or that has one slice)
inline bool dgemm_epi_supported(int N, int epi, int splitk) {
  if (epi == EPI_SILU) return splitk == 1 && N % 32 == 0;
  if (epi == EPI_RESNORM) return splitk == 1 || N % 256 == 0;
  return true;
}

inline bool gdgemm_supported(int M, int N, int K, int splitk, int bn, int bm = 64) {
  if (bn != 64 && bn != 128) return false;
  if (bm != 64 && !(bm == 128 && bn == 128) && bm != 256) return false;
  if (M <= 0 || N <= 0 || K <= 0 || !dgemm_splitk_ok(splitk) || N % 4 || K % splitk) return false;
  const int kps = K / splitk;
  return kps % GBK == 0 && kps >= GBK;
}

// fp32 workspace floats of a split-K launch that combines in the launch (tile-padded slabs)
inline long gdgemm_ws_floats(int M, int N, int splitk, int bn, int bm = 64) {
  if (bn <= 0 || bm <= 0) return 0;
  const long tm = (M + bm - 1) / bm, tn = (N + bn - 1) / bn;
  const long slabs = (long)splitk * tm * tn * bm * bn;
  const long dense = (long)splitk * M * N;
  return slabs > dense ? slabs : dense;
}

// ---- kgemm.hip: plain prologue, EPI_STORE / EPI_RESNORM ----
inline bool kgemm_supported(int M, int N, int K, int bm, int epi = EPI_STORE) {
  return M > 0 && (bm == 16 || bm == 32) && N % KBN == 0 && K >= KST && K % KST == 0 &&
         (epi == EPI_STORE || epi == EPI_RESNORM);
}

// ---- pgemm.hip ----
// ldx: row stride of X in elements.  The DMA addresses X and one group's W through buffer
// descriptors with 32-bit offsets, so both stay below 2 GiB.
inline bool pgemm_supported(int M, int N, int K, long ldx) {
  return M > 0 && N > 0 && N % PG_T == 0 && K >= PG_BK && K % PG_BK == 0 &&
         (long)M * ldx * 2 < (1L << 31) && (long)N * K * 2 < (1L << 31);
}

// the decode split-K form: grid = tiles * splits <= the CU count (all slices resident), two
// tickets per tile below the error word
inline bool pgemm_sk_supported(int M, int N, int K, int splits, int cus) {
  const int nk = K / PG_BK;
  const long grid = (long)((M + PG_T - 1) / PG_T) * (N / PG_T) * splits;
  return M > 0 && N % PG_T == 0 && K % PG_BK == 0 && splits >= 1 && splits <= 32 &&
         nk >= splits && grid <= cus &&
         (N / PG_T) * ((M + PG_T - 1) / PG_T) * 2 * kCtrStride < kCtrErr;
}

inline long pgemm_sk_ws_floats(int M, int N, int splits) {
  if (splits <= 1) return 0;
  return (long)((M + PG_T - 1) / PG_T) * (N / PG_T) * splits * PG_T * PG_T;
}

// ---- wgemm.hip ----
inline bool wgemm_supported(int M, int N, int K, int ldx, int ldw, int ldy) {
  return M > 0 && N > 0 && K >= WBK && K % WBK == 0 && ldx % 8 == 0 && ldw % 8 == 0 &&
         ldy % 8 == 0;
}

// ---- qgemm.hip ----
struct QGemmGeom {
  int bm, bn;  // output tile of one 4-wave workgroup (K is split over its waves)
  int grid;
};

// The one place the geometry is chosen.  Rows: the smallest tile that holds M (64-row tiles
// above 32 rows).  Columns: 64 when that still gives every CU a workgroup ("wide N": half the
// X re-reads per weight byte), else 32 ("narrow N": more workgroups for the o / down
// projections), and 16 for the 16-row tile when 32 columns would leave half the CUs or more
// without a workgroup (N <= 4,096 at M <= 16: a pure weight stream, so the number of
// workgroups with DMAs in flight is what bounds it).
inline QGemmGeom qgemm_geometry(int M, int N, int K) {
  (void)K;
  constexpr int kCus = 256;
  QGemmGeom g;
  g.bm = M <= 16 ? 16 : (M <= 32 ? 32 : 64);
  const int tiles_m = (M + g.bm - 1) / g.bm;
  if (((N + 63) / 64) * tiles_m >= kCus) g.bn = 64;
  else if (g.bm == 16 && (N + 31) / 32 <= kCus / 2) g.bn = 16;
  else g.bn = 32;
  g.grid = tiles_m * ((N + g.bn - 1) / g.bn);
  return g;
}

// What qgemm.hip and q4gemm.hip take (qgemm_common.h): at most max_m rows, whole bk-deep wave
// steps, 16-byte row segments of Y and 16-byte aligned rows of X and Y
inline bool quant_gemm_supported(int M, int N, int K, int ldx, int ldy, int max_m, int bk) {
  return M > 0 && M <= max_m && N > 0 && N % 8 == 0 && K >= bk && K % bk == 0 && ldx % 8 == 0 &&
         ldy % 8 == 0;
}

inline bool qgemm_supported(int M, int N, int K, int ldx, int ldy) {
  return quant_gemm_supported(M, N, K, ldx, ldy, QGEMM_MAX_M, QBK);
}

// ---- q4gemm.hip ----
// Rows and columns as qgemm_geometry, except that a 64-row tile is always 32 columns wide: at a
// 128-deep k-step a 64-row X slot is 16 KB per wave, and two such slots per wave with a
// 64-column weight slot do not fit the CU's 160 KB of LDS.
inline QGemmGeom q4gemm_geometry(int M, int N, int K) {
  QGemmGeom g = qgemm_geometry(M, N, K);
  if (g.bm == 64) {
    g.bn = 32;
    g.grid = ((M + 63) / 64) * ((N + 31) / 32);
  }
  return g;
}

// K % 128: a wave step is 128 deep, and it makes a row of scale codes (K / 32 bytes) a whole
// number of the 4-byte words the scale DMA moves
inline bool q4gemm_supported(int M, int N, int K, int ldx, int ldy) {
  return quant_gemm_supported(M, N, K, ldx, ldy, Q4GEMM_MAX_M, Q4BK);
}

// ---- moe_dgemm.hip / moe_qgemm.hip / moe_q4gemm.hip (moe_gemm_common.h) ----
// What the three grouped kernels agree on: the compiled ring depths, K split evenly, no SILU
// epilogue on fp32 partials, whole gate/up interleave groups (SILU) or 16-byte output rows.
// Each adds its own depth rule.  N > 0 and K > 0 are not part of it: the bf16 predicate has
// never tested them (an empty launch is a no-op there).
inline bool moe_gemm_common_supported(int N, int K, int pf, int silu, int splitk) {
  if (pf != 1 && pf != 2 && pf != 4) return false;
  if (splitk < 1 || K % splitk) return false;
  if (silu && splitk > 1) return false;
  return silu ? N % 32 == 0 : N % 8 == 0;
}

// bf16 weights: a ring step is MBK deep and a slice is whole ring turns
inline bool moe_dgemm_supported(int N, int K, int pf, int silu, int splitk) {
  return moe_gemm_common_supported(N, K, pf, silu, splitk) && (K / splitk) % (MBK * pf) == 0;
}

// FP8 weights: a ring step is MQBK deep, and a slice whose depth is an odd multiple of MBK ends
// in a half step, so pf = 1 takes every (N, K, silu, splitk) that moe_dgemm_supported takes
// for some pf
constexpr int MQBK = 128;
inline bool moe_qgemm_supported(int N, int K, int pf, int silu, int splitk) {
  if (N <= 0 || K <= 0 || !moe_gemm_common_supported(N, K, pf, silu, splitk)) return false;
  return (K / splitk) % MBK == 0 && ((K / splitk + MQBK - 1) / MQBK) % pf == 0;
}

// MXFP4 weights: moe_qgemm's ring step and half step.  A scale row is K / 32 bytes and a step
// reads 4 of them (a half step 2), so K % MQBK == 0; with that, pf = 1 takes every (N, K, silu,
// splitk) that moe_dgemm_supported takes for some pf
inline bool moe_q4gemm_supported(int N, int K, int pf, int silu, int splitk) {
  return K % MQBK == 0 && moe_qgemm_supported(N, K, pf, silu, splitk);
}

inline bool moe_router_topk_supported(int E, int d) {
  return E >= 1 && E <= kRouterMaxE && d % 8 == 0;
}

// ---- the dgemm op's launch contract (torch.ops.akap.dgemm: dgemm.hip, gdgemm.hip and the
// pgemm.hip split-K body behind one binding) ----
enum { DG_RING = 0, DG_LDS = 1, DG_PGEMM_SK = 2 };
struct DGemmContract {
  bool supported;    // the binding accepts the launch
  int family;        // DG_RING (bn = 0) | DG_LDS (bn 64 | 128) | DG_PGEMM_SK (bn = 256)
  bool inlaunch;     // the K slices are combined through tile tickets, no separate reduce pass
  long ws_floats;    // fp32 workspace the launch needs (0: none)
  long ticket_ints;  // zeroed int32 tickets it needs (0: none)
};

// inlaunch: the caller asks for (offers tickets for) the in-launch combine.  Every LDS-DMA
// variant takes it; the register ring only with the plain prologue and 2 | 4 | 8 slices, and
// otherwise runs its separate reduce pass; the 256 x 256 body always combines in the launch.
// cus: the device's compute units (the 256 x 256 body needs every slice resident).  ns (the
// LDS ring depth) is any value: the launcher maps it to a compiled depth.
inline DGemmContract dgemm_contract(int M, int N, int K, int pro, int epi, int splitk, int pf,
                                    int bn, int ns, int bm, bool inlaunch, int cus) {
  (void)ns;
  DGemmContract c{};
  const bool sk = bn == 256;
  c.family = sk ? DG_PGEMM_SK : bn > 0 ? DG_LDS : DG_RING;
  c.inlaunch = splitk > 1 && (sk || (inlaunch && (bn > 0 || (pro == PRO_PLAIN &&
                                                             (splitk == 2 || splitk == 4 ||
                                                              splitk == 8)))));
  c.supported =
      pro >= PRO_PLAIN && pro <= PRO_SILU && epi >= EPI_STORE && epi <= EPI_SILU &&
      (epi == EPI_STORE || pro == PRO_PLAIN) &&  // epilogues need the plain prologue,
      (bn == 0 || pro == PRO_PLAIN) &&           // and so do the LDS-DMA variants
      (bm == 64 || bn > 0) &&                    // taller tiles are LDS-DMA variants
      (sk ? pgemm_sk_supported(M, N, K, splitk, cus)
          : bn > 0 ? gdgemm_supported(M, N, K, splitk, bn, bm)
                   : dgemm_supported(M, N, K, splitk, pf)) &&
      (c.inlaunch ? (epi != EPI_SILU || N % 32 == 0) : dgemm_epi_supported(N, epi, splitk)) &&
      (long)N * K * 2 >= (long)M * 4;  // W at least M floats
  // the sizes follow from M, N and the variant alone (any K, any epilogue)
  const int tile_n = bn > 0 ? bn : DBN, tile_m = bn > 0 ? bm : DBM;
  if (splitk > 1 && tile_m > 0) {
    c.ws_floats = sk ? pgemm_sk_ws_floats(M, N, splitk)
                  : c.inlaunch ? gdgemm_ws_floats(M, N, splitk, tile_n, tile_m)
                               : (long)splitk * M * N + (pro == PRO_ADDNORM ? (long)splitk * M : 0);
    if (c.inlaunch)
      c.ticket_ints = sk ? (long)kCtrInts
                         : (long)((M + tile_m - 1) / tile_m) * ((N + tile_n - 1) / tile_n) *
                               kCtrStride;
  }
  return c;
}

// ---- paged KV cache layout ----
// The one definition of where a (block, kv head, token, dim) element of the paged caches lives;
// every kernel, ops.cpp and Python (`_runtime.contract`) take it from here.  Offsets are in
// elements (bf16, or bytes of an fp8 cache).  Chosen so the attention kernels issue 16-byte
// MFMA-operand loads with no transpose, 1 KiB contiguous per load instruction:
//   K cache: [num_blocks, Hkv, BS, D] shape, BS % 32 == 0.  Within one (block, kv head) each
//            32-token chunk is stored as [tile tt (2)][k-step cc (4)][row r (16)][32 dims]: the
//            exact operand order of the attention kernels' S^T = K.Q^T MFMA tiles, whose row r
//            of tile tt is chunk token 8*(r>>2) + 4*tt + (r&3).  That row order makes a lane
//            group hold 8 contiguous tokens, which is what lets V^T come straight from:
//   V cache: [num_blocks, Hkv, BS/8, D, 8] (8-token groups, dim-major inside a group): the
//            attention kernel's V^T operand (one dim, 8 consecutive tokens) is one 16-byte
//            load, and a token's 128 dims land in 16-byte-strided slots of one 2 KiB group
//            (4x fewer cache lines touched per written token than [D][BS]).
//   V tail:  [tail slots, Hkv, 8, D] bf16, token-major: a sequence's still-partial last V
//            group, so decode steps write no partial cache lines.
constexpr int kKvD = 128, kKvChunk = 32;       // head dim; tokens per K chunk
constexpr int kKvGroup = 8, kVTailRows = 8;    // tokens per V group; V-tail rows per kv head

// First element of a (block, kv head) in the K and in the V cache, the 8-token V group of token
// `off` within it, and row 0 of a (tail slot, kv head) of the V tail.  These four also exist as
// macros: a kernel whose tuned code changes when the arithmetic arrives through an inlined
// function (rope_cache.hip, the prefill staging of attention.hip) expands the same text in place.
#define AKAP_K_HEAD_BASE(blk, Hkv, h, BS) (((size_t)(blk) * (Hkv) + (h)) * (BS) * akap::kKvD)
#define AKAP_V_HEAD_BASE(blk, Hkv, h, BS) (((size_t)(blk) * (Hkv) + (h)) * akap::kKvD * (BS))
#define AKAP_V_GROUP_OFFSET(off) (((off) >> 3) * akap::kKvD * akap::kKvGroup)
#define AKAP_V_TAIL_BASE(tsl, Hkv, h) \
  (((size_t)(tsl) * (Hkv) + (h)) * akap::kVTailRows * akap::kKvD)
constexpr size_t k_head_base(size_t blk, int Hkv, int h, int BS) {
  return AKAP_K_HEAD_BASE(blk, Hkv, h, BS);
}
constexpr size_t v_head_base(size_t blk, int Hkv, int h, int BS) {
  return AKAP_V_HEAD_BASE(blk, Hkv, h, BS);
}
// K: (token `off` of the block, dim 0) within the block-head; dim d is k_dim_offset(d) further
constexpr int k_token_offset(int off) {
  const int o = off & (kKvChunk - 1);
  const int tt = (o >> 2) & 1;
  const int r = ((o >> 3) << 2) | (o & 3);
  return (off >> 5) * kKvChunk * kKvD + tt * 16 * kKvD + r * 32;
}
constexpr int k_dim_offset(int d) { return (d >> 5) * 512 + (d & 31); }
// V: the 8-token group of token `off`, and its element (token off, dim d), within the block-head
constexpr int v_group_offset(int off) { return AKAP_V_GROUP_OFFSET(off); }
constexpr int v_elem_offset(int off, int d) { return v_group_offset(off) + d * 8 + (off & 7); }
// V tail: dim 0 of row `row` (token row of the partial group) of a (tail slot, kv head)
constexpr size_t v_tail_row_offset(size_t tsl, int Hkv, int h, int row) {
  return AKAP_V_TAIL_BASE(tsl, Hkv, h) + (size_t)row * kKvD;
}

// ---- K/V rider workgroups of the gate|up decode GEMM launch (kv_write.h) ----
// Workgroups of one dgemm.hip / gdgemm.hip variant a CU holds at once: the register ring is
// __launch_bounds__(256, 2); the LDS ring holds two only in its shallow 64-row form (the deep
// ring and the 128 / 256-row tiles fill a CU's LDS with one).
inline int dgemm_wgs_per_cu(int bn, int ns, int bm) {
  if (bn == 0) return 2;
  if (bm == 128 || bm == 256) return 1;
  return ns >= 6 ? 1 : 2;
}

constexpr int kKvRiderRows = 16;  // (sequence, kv head, K | V) rows one rider covers per pass

// Rider workgroups to append to the launch, 0 when it may carry none.  Legal: the SwiGLU
// epilogue with one K slice on the register-ring or LDS-ring family, and the kernel's resident
// capacity (cus x workgroups per CU) covers the tiles and at least one rider, so no rider waits
// for a tile to finish; the model side: bf16 KV cache with a V tail, tp = 1, a dense layer, no
// weight quantization.  Each rider loops over its share of the ceil(B * Hkv * 2 / 16) passes.
inline int kv_rider_blocks(int M, int N, int epi, int splitk, int bn, int ns, int bm, int cus,
                           int B, int Hkv, bool kv_bf16_tail, int tp, bool dense,
                           bool quantized) {
  if (epi != EPI_SILU || splitk != 1 || bn == 256 || bn < 0) return 0;
  if (!kv_bf16_tail || tp != 1 || !dense || quantized) return 0;
  if (M <= 0 || N <= 0 || B <= 0 || Hkv <= 0 || cus <= 0) return 0;
  const int tile_n = bn > 0 ? bn : DBN, tile_m = bn > 0 ? bm : DBM;
  if (tile_m <= 0) return 0;
  const long tiles = (long)((M + tile_m - 1) / tile_m) * ((N + tile_n - 1) / tile_n);
  const long room = (long)cus * dgemm_wgs_per_cu(bn, ns, bm) - tiles;
  const long need = ((long)B * Hkv * 2 + kKvRiderRows - 1) / kKvRiderRows;
  const long n = need < room ? need : room;
  return n > 0 ? (int)n : 0;
}

}  // namespace akap
