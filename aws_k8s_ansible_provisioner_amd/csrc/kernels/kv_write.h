// The decode step's new-token K / V write, once: per-head K RMSNorm (bf16-rounded) + NeoX RoPE
// and the stores into the paged caches and the V tail.  One head row (D = 128) is held by 16
// lanes x 8 dims (lane j = dims [8j, 8j + 8)); rotary pairs (d, d + 64) sit in lanes j and j ^ 8.
//
// Two callers, one lane layout, so the bytes written are identical:
//   * attention.hip's fused decode prologue (rows G = key head, G + 1 = value head of its
//     work item): head_norm_rope on the q and k rows, then kv_store_k / kv_store_v_tail_row /
//     kv_store_v_group -- in its serving form from the LDS images, at the end of the work item;
//   * the rider workgroups of the gate|up decode GEMM (kv_rider_block below, dgemm.hip /
//     gdgemm.hip): kv_write_row, which is the same arithmetic followed by the same stores.
#pragma once

#include "common.h"
#include "kernels.h"

namespace akap {

// 16 lanes (j = dims [8j, 8j+8)) hold an 8-token group token-major (rows[i] = token i) and
// turn it into the cache's [D][8] group image (dim-major, 16 B per dim): u[k] = dim 8j + k
__device__ __forceinline__ void group_units(const bf16x8 (&rows)[8], bf16x8 (&u)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k)
#pragma unroll
    for (int i = 0; i < 8; ++i) u[k][i] = rows[i][k];
}

// x: this lane's 8 dims of a raw q / k head row.  norm: per-head RMSNorm with weight w8, the
// result rounded to bf16 like the standalone kernel's; then NeoX RoPE with the cos (c0, c1) and
// sin (s0, s1) of dims 8 (j & 7) .. + 7.  The 16 lanes of the row run this together.
__device__ __forceinline__ void head_norm_rope(float (&x)[8], bool norm, const bf16x8& w8,
                                               const f32x4& c0, const f32x4& c1, const f32x4& s0,
                                               const f32x4& s1, float eps, int j) {
  if (norm) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) ss += x[i] * x[i];
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 16);
    const float inv = rsqrtf(ss / (float)kKvD + eps);
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = bf2f(f2bf(x[i] * inv * bf2f(w8[i])));
  }
  const float cv[8] = {c0[0], c0[1], c0[2], c0[3], c1[0], c1[1], c1[2], c1[3]};
  const float sv[8] = {s0[0], s0[1], s0[2], s0[3], s1[0], s1[1], s1[2], s1[3]};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float other = __shfl_xor(x[i], 8, 16);
    x[i] = j < 8 ? x[i] * cv[i] - other * sv[i] : x[i] * cv[i] + other * sv[i];
  }
}

// 8 consecutive cache elements at element `e` <- bf16x8: one 16-B store, or (fp8 cache) the pack
// of the bf16-rounded values and one 8-B store.  The counterpart of ld_kv8.
template <bool F8>
__device__ __forceinline__ void st_kv8(void* cache, size_t e, const bf16x8& v) {
  if constexpr (F8) {
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    u32x2 w;
    w[0] = f32x4_to_fp8x4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
    w[1] = f32x4_to_fp8x4((float)v[4], (float)v[5], (float)v[6], (float)v[7]);
    *reinterpret_cast<u32x2*>(reinterpret_cast<uint8_t*>(cache) + e) = w;
  } else {
    *reinterpret_cast<bf16x8*>(reinterpret_cast<bf16*>(cache) + e) = v;
  }
}
template <bool F8>
__device__ __forceinline__ void st_kv1(void* cache, size_t e, bf16 v) {
  if constexpr (F8) reinterpret_cast<uint8_t*>(cache)[e] = f32_to_fp8((float)v);
  else reinterpret_cast<bf16*>(cache)[e] = v;
}

// The V stores here and in rope_cache.hip add the element step to the group themselves; it is the
// layout's: dim d of token off sits 8 d + off % 8 past AKAP_V_GROUP_OFFSET(off).
constexpr bool v_steps_match_layout() {
  bool ok = true;
  for (int i = 0; i < 64 * kKvD; ++i)  // (off, d) = (i / D, i % D)
    ok = ok && v_elem_offset(i / kKvD, i % kKvD) ==
                   AKAP_V_GROUP_OFFSET(i / kKvD) + (i % kKvD) * 8 + ((i / kKvD) & 7);
  return ok;
}
static_assert(v_steps_match_layout());

// The stores take a cache slot as (blk, off) = (slot / BS, slot % BS): 64-bit divisions, done
// once by a caller with several stores; the bases in their macro form (host_contract.h), which
// keeps the callers' tuned code.  The K row of token off of block blk, dims [8j, 8j+8):
template <bool F8 = false>
__device__ __forceinline__ void kv_store_k(void* k_cache, int Hkv, int BS, int kvh, int64_t blk,
                                           int off, int j, const bf16x8& k8) {
  st_kv8<F8>(k_cache,
             AKAP_K_HEAD_BASE(blk, Hkv, kvh, BS) + k_token_offset(off) + k_dim_offset(8 * j), k8);
}

// a still-partial V group: the token's row (dims [8j, 8j+8)) goes to row i0 of the sequence's tail
__device__ __forceinline__ void kv_store_v_tail_row(bf16* v_tail, int Hkv, int kvh, int tsl,
                                                    int i0, int j, const bf16x8& v8) {
  // row 0, then the row step (rows are kKvD apart): as one sum the rider GEMMs take a VGPR more
  bf16* tb = v_tail + AKAP_V_TAIL_BASE(tsl, Hkv, kvh) + 8 * j;
  *reinterpret_cast<bf16x8*>(tb + (size_t)i0 * kKvD) = v8;
}

// a completed V group: its [D][8] image (u[k] = dim 8j + k, 8 tokens) goes to the cache
template <bool F8 = false>
__device__ __forceinline__ void kv_store_v_group(void* v_cache, int Hkv, int BS, int kvh,
                                                 int64_t blk, int off, int j,
                                                 const bf16x8 (&u)[8]) {
  const size_t e =
      AKAP_V_HEAD_BASE(blk, Hkv, kvh, BS) + AKAP_V_GROUP_OFFSET(off) + (size_t)(8 * j) * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) st_kv8<F8>(v_cache, e + 8 * k, u[k]);
}

// one token of a V group: its dims [8j, 8j+8) go to the group's token column, 8 elements apart
template <bool F8 = false>
__device__ __forceinline__ void kv_store_v_token(void* v_cache, int Hkv, int BS, int kvh,
                                                 int64_t blk, int off, int j, const bf16x8& v8) {
  const size_t e = AKAP_V_HEAD_BASE(blk, Hkv, kvh, BS) + AKAP_V_GROUP_OFFSET(off) + (off & 7) +
                   (size_t)(8 * j) * 8;
#pragma unroll
  for (int k = 0; k < 8; ++k) st_kv1<F8>(v_cache, e + 8 * k, v8[k]);
}

// Operands of one (sequence, kv head, K | V) row, loaded up front by 16 lanes.
struct KvRowOps {
  bf16x8 raw, w8;
  f32x4 c0, c1, s0, s1;
  bf16x8 trow[8];  // V rows: the sequence's 8 tail rows
  int64_t slot;
  int tsl;
};

// One row's write from preloaded operands.  is_v is uniform over the row's 16 lanes (the norm's
// and the rotation's lane swaps stay inside one branch).  Rows with slot < 0 (graph padding) or
// tsl < 0 (no tail) write nothing.
__device__ __forceinline__ void kv_write_row(const KvWriteArgs& a, int kvh, bool is_v, bool live,
                                             int j, const KvRowOps& r) {
  const bool wr = live && r.slot >= 0 && r.tsl >= 0;
  // slot / BS and slot % BS stay inside the K and the V branch: hoisted above them the rider GEMMs
  // are ~350 lines shorter but take 3 to 8 VGPRs more (profiles/kv_layout_refactor.md)
  bf16* kc = static_cast<bf16*>(a.k_cache);
  bf16* vc = static_cast<bf16*>(a.v_cache);
  bf16* vt = static_cast<bf16*>(a.v_tail);
  if (!is_v) {
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = bf2f(r.raw[i]);
    head_norm_rope(x, a.k_w != nullptr, r.w8, r.c0, r.c1, r.s0, r.s1, a.eps, j);
    bf16x8 o8;
#pragma unroll
    for (int i = 0; i < 8; ++i) o8[i] = f2bf(x[i]);
    if (wr) kv_store_k(kc, a.Hkv, a.BS, kvh, r.slot / a.BS, (int)(r.slot % a.BS), j, o8);
  } else if (wr) {
    const int i0 = (int)(r.slot % a.BS) & 7;
    if (i0 == 7) {  // rows 0..6 from the tail, row 7 = the new token
      bf16x8 rows[8], u[8];
#pragma unroll
      for (int i = 0; i < 7; ++i) rows[i] = r.trow[i];
      rows[7] = r.raw;
      group_units(rows, u);
      kv_store_v_group(vc, a.Hkv, a.BS, kvh, r.slot / a.BS, (int)(r.slot % a.BS), j, u);
    } else {
      kv_store_v_tail_row(vt, a.Hkv, kvh, r.tsl, i0, j, r.raw);
    }
  }
}

// A rider workgroup (256 threads) of a GEMM launch: 16 rows per pass, 16 lanes per row.  A
// pass covers 8 consecutive (sequence, kv head) pairs: waves 0-1 their K rows, waves 2-3 their
// V rows (wave-uniform K | V).  Rider `rider` of `nriders` takes passes rider, rider + nriders,
// ...  No LDS, no barrier, no atomics.  Every load of a pass is issued before its first
// dependent use and reads a valid address on every lane (lanes past the last pair re-read the
// last pair; a K row's "tail rows" and a V row's norm weight read the qkv row), so the waits
// are counted; only the stores are predicated.
__device__ __forceinline__ void kv_rider_block(const KvWriteArgs& a, int rider, int nriders) {
  if (threadIdx.x >= 256) return;  // the 8-wave tiles: waves 4-7 have no rows
  const int rr = threadIdx.x >> 4;
  const int j = threadIdx.x & 15;
  const bool is_v = rr >= 8;
  const int pairs = a.B * a.Hkv;
  const int passes = (pairs + 7) >> 3;
  const bf16* qkv = static_cast<const bf16*>(a.qkv);
  const bf16* kw = static_cast<const bf16*>(a.k_w);
  const bf16* vt = static_cast<const bf16*>(a.v_tail);
  // two passes per trip: a pass is two dependent round trips (row indices, then operands), so a
  // rider's share costs half as many of them; a pass index past the end is a dead row
  constexpr int U = 2;
  for (int ps = rider; ps < passes; ps += U * nriders) {
    KvRowOps r[U];
    int seq[U], kvh[U];
    int64_t pos[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p0 = (ps + u * nriders) * 8 + (rr & 7);
      live[u] = ps + u * nriders < passes && p0 < pairs;
      const int pr = live[u] ? p0 : pairs - 1;
      seq[u] = pr / a.Hkv;
      kvh[u] = pr % a.Hkv;
      r[u].slot = a.slots[seq[u]];
      r[u].tsl = a.tail_slot[seq[u]];
      pos[u] = a.positions[seq[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bf16* row = qkv + (size_t)seq[u] * a.qkv_stride;
      const int head = a.Hq + (is_v ? a.Hkv : 0) + kvh[u];
      r[u].raw = *reinterpret_cast<const bf16x8*>(row + head * kKvD + 8 * j);
      r[u].w8 = *reinterpret_cast<const bf16x8*>(!is_v && kw != nullptr ? kw + 8 * j : row);
      const float* cs = a.cos_sin + (size_t)pos[u] * kKvD;
      const int i0 = is_v ? 0 : 8 * (j & 7);
      r[u].c0 = *reinterpret_cast<const f32x4*>(cs + i0);
      r[u].c1 = *reinterpret_cast<const f32x4*>(cs + i0 + 4);
      r[u].s0 = *reinterpret_cast<const f32x4*>(cs + 64 + i0);
      r[u].s1 = *reinterpret_cast<const f32x4*>(cs + 64 + i0 + 4);
      const bf16* tb =
          is_v ? vt + AKAP_V_TAIL_BASE(max(r[u].tsl, 0), a.Hkv, kvh[u]) + 8 * j : row;
      const int ts = is_v ? kKvD : 0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        r[u].trow[i] = *reinterpret_cast<const bf16x8*>(tb + (size_t)i * ts);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) kv_write_row(a, kvh[u], is_v, live[u], j, r[u]);
  }
}

}  // namespace akap
