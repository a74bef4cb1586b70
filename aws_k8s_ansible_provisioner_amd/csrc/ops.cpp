// torch custom-op registrations (namespace `akap`) for the gfx950 kernels.
//
// Every op launches on the caller's current HIP stream, allocates nothing and
// never synchronises, so all of them are hipGraph-capturable (engine decode path).
// PyTorch on ROCm names the GPU dispatch key "CUDA"; kernels are HIP/CDNA4 only.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include "kernels/kernels.h"
#include "op_args.h"

// `data_ptr` appears in this file only in the functions below; every other pointer that
// reaches a launch comes from an akap::OpArgs accessor (op_args.h).  tests/test_op_args.py
// audits this list:
//   h2d_stage        the source is pinned HOST memory, mapped with hipHostGetDevicePointer
//   car_ipc_handles  fills a host byte blob with the two IPC handles
//   car_open         reads the gathered host blob of IPC handles
//   ipc_export       asks the runtime for the allocation around the address; fills a host blob
//   ipc_open         reads a host blob (IPC handle + offset)

namespace {

using at::Tensor;
using akap::OpArgs, akap::kAlign16, akap::kContig, akap::kLastContig, akap::kKvD;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

// The accessor (and device guard) of op `op`, anchored on its tensor `t`, which must be on a GPU
OpArgs on_gpu(const char* op, const Tensor& t, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda(), op, ": ", name, " must be a GPU tensor");
  return OpArgs(op, t.device());
}

void rmsnorm(Tensor out, Tensor x, Tensor w, double eps) {
  const OpArgs a = on_gpu("rmsnorm", x, "x");
  const int d = x.size(-1);
  TORCH_CHECK(d % 8 == 0, "rmsnorm: hidden size must be a multiple of 8");
  const int rows = x.numel() / d;
  akap::launch_rmsnorm(a.bf16(out, "out", (int64_t)rows * d, kLastContig),
                       a.bf16(x, "x", 0, kLastContig), a.bf16(w, "w", d), rows, d,
                       x.dim() > 1 ? x.stride(-2) : d, out.dim() > 1 ? out.stride(-2) : d,
                       (float)eps, cur_stream());
}

void fused_add_rmsnorm(Tensor out, Tensor residual, Tensor x, Tensor w, double eps) {
  const OpArgs a = on_gpu("fused_add_rmsnorm", x, "x");
  const int d = x.size(-1);
  TORCH_CHECK(d % 8 == 0, "fused_add_rmsnorm: hidden size must be a multiple of 8");
  const int rows = x.numel() / d;
  akap::launch_fused_add_rmsnorm(a.bf16(out, "out", (int64_t)rows * d, kLastContig),
                                 a.bf16(residual, "residual", (int64_t)rows * d),
                                 a.bf16(x, "x", 0, kLastContig), a.bf16(w, "w", d), rows, d,
                                 x.dim() > 1 ? x.stride(-2) : d,
                                 out.dim() > 1 ? out.stride(-2) : d, (float)eps, cur_stream());
}

// The paged KV cache of one layer (layout: host_contract.h): K [NB, Hkv, BS, 128] and
// V [NB, Hkv, BS/8, 128, 8] (8-token groups), both contiguous and both bf16, or both uint8
// holding OCP e4m3fn bytes (--kv-cache-dtype fp8); BS a multiple of 32 (K cache chunk layout).
struct KVCache { int fp8, Hkv, BS; void *k, *v; };
KVCache kv_cache_of(const OpArgs& a, const Tensor& k_cache, const Tensor& v_cache) {
  KVCache c{};
  c.k = a.ptr(k_cache, "k_cache", {at::kBFloat16, at::kByte});
  c.v = a.ptr(v_cache, "v_cache", {k_cache.scalar_type()});
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(3) == kKvD, a.op(),
              ": k_cache must be [NB,Hkv,BS,128] (head_dim 128)");
  c.fp8 = k_cache.scalar_type() == at::kByte;
  c.Hkv = k_cache.size(1);
  c.BS = k_cache.size(2);
  TORCH_CHECK(c.BS % akap::kKvChunk == 0, a.op(),
              ": k_cache block size must be a multiple of 32 (K cache chunk layout)");
  TORCH_CHECK(v_cache.dim() == 5 && v_cache.size(0) == k_cache.size(0) &&
                  v_cache.size(1) == c.Hkv && v_cache.size(2) * akap::kKvGroup == c.BS &&
                  v_cache.size(3) == kKvD && v_cache.size(4) == akap::kKvGroup,
              a.op(), ": v_cache must be [NB,Hkv,BS/8,128,8] beside k_cache [NB,Hkv,BS,128]");
  return c;
}

// The V tail: v_tail contiguous bf16 [slots, Hkv, 8, 128] (a bf16 cache only) with tail_slot,
// int32 with at least `rows` entries; both null when v_tail is absent
struct VTail { void* v_tail; const int* tail_slot; };
VTail v_tail_of(const OpArgs& a, const KVCache& kv, const std::optional<Tensor>& v_tail,
                const std::optional<Tensor>& tail_slot, int rows) {
  if (!v_tail) return {nullptr, nullptr};
  TORCH_CHECK(!kv.fp8, a.op(), ": v_tail needs a bf16 KV cache");
  TORCH_CHECK(tail_slot.has_value(), a.op(), ": tail_slot must come with v_tail");
  VTail t{a.bf16(*v_tail, "v_tail"), a.ptr<int>(*tail_slot, "tail_slot", rows)};
  TORCH_CHECK(v_tail->dim() == 4 && v_tail->size(1) == kv.Hkv &&
                  v_tail->size(2) == akap::kVTailRows && v_tail->size(3) == kKvD,
              a.op(), ": v_tail must be contiguous bf16 [slots, Hkv, 8, 128]");
  return t;
}

void qk_norm_rope_cache(Tensor qkv, Tensor q_out, Tensor k_cache, Tensor v_cache,
                        Tensor positions, Tensor slots, Tensor cos_sin,
                        std::optional<Tensor> q_w, std::optional<Tensor> k_w, int64_t Hq,
                        int64_t Hkv, double eps, bool apply_rope, bool decode,
                        std::optional<Tensor> v_tail, std::optional<Tensor> tail_slot,
                        int64_t num_decode, int64_t q_rows) {
  const OpArgs a = on_gpu("qk_norm_rope_cache", qkv, "qkv");
  const KVCache kv = kv_cache_of(a, k_cache, v_cache);
  TORCH_CHECK(qkv.dim() == 2 && Hq >= 0 && Hkv == kv.Hkv, a.op(),
              ": qkv must be 2-D and Hkv the cache's");
  const int T = qkv.size(0);
  TORCH_CHECK(q_rows >= -1 && q_rows <= T, a.op(), ": q_rows out of range");
  TORCH_CHECK(qkv.size(1) >= (Hq + 2 * Hkv) * kKvD, a.op(), ": qkv too narrow");
  TORCH_CHECK(!v_tail || !decode, a.op(),
              ": v_tail is written by the span (prefill / mixed) role only");
  TORCH_CHECK(!v_tail || (num_decode >= 0 && num_decode <= T), a.op(),
              ": num_decode out of range");
  const VTail vt = v_tail_of(a, kv, v_tail, tail_slot, T);
  akap::launch_qk_norm_rope_cache(
      a.bf16(qkv, "qkv", 0, kLastContig), qkv.stride(0),
      a.bf16(q_out, "q_out", (q_rows < 0 ? T : q_rows) * Hq * kKvD), kv.k, kv.v,
      a.ptr<int64_t>(positions, "positions", T), a.ptr<int64_t>(slots, "slots", T),
      a.ptr<float>(cos_sin, "cos_sin", apply_rope ? kKvD : 0), a.bf16(q_w, "q_w", kKvD),
      a.bf16(k_w, "k_w", kKvD), T, Hq, Hkv, kKvD, kv.BS, (float)eps, apply_rope ? 1 : 0,
      cur_stream(), kv.fp8, decode ? 1 : 0, vt.v_tail, vt.tail_slot, (int)num_decode,
      (int)q_rows);
}

void reshape_and_cache(Tensor k, Tensor v, Tensor k_cache, Tensor v_cache, Tensor slots) {
  const OpArgs a = on_gpu("reshape_and_cache", k, "k");
  const KVCache kv = kv_cache_of(a, k_cache, v_cache);
  TORCH_CHECK(k.dim() == 3 && k.size(1) == kv.Hkv && k.size(2) == kKvD, a.op(),
              ": k must be [T, Hkv, 128] with the cache's Hkv");
  const int T = k.size(0);
  akap::launch_reshape_and_cache(a.bf16(k, "k"), a.bf16(v, "v", k.numel()), kv.k, kv.v,
                                 a.ptr<int64_t>(slots, "slots", T), T, kv.Hkv, kKvD, kv.BS,
                                 cur_stream(), kv.fp8);
}

void silu_and_mul(Tensor out, Tensor x) {
  const OpArgs a = on_gpu("silu_and_mul", x, "x");
  const int F = x.size(-1) / 2;
  TORCH_CHECK(F % 8 == 0, "silu_and_mul: ffn size must be a multiple of 8");
  const long T = x.numel() / x.size(-1);
  akap::launch_silu_and_mul(a.bf16(out, "out", T * F), a.bf16(x, "x", 0, kLastContig), T, F,
                            x.dim() > 1 ? x.stride(-2) : 2 * F, cur_stream());
}

// What the four attention ops share: `q` is the q-shaped tensor [T, Hq, 128] (the ops that
// read raw QKV rows pass `out`, same shape, and clear p.q), `rows` the q / out rows the launch
// certainly touches (0: known to the device only), B the number of sequences.
akap::AttnParams attn_params(const OpArgs& a, const KVCache& kv, Tensor& out, Tensor& q,
                             Tensor& block_tables, Tensor& seq_lens, int64_t rows, int64_t G,
                             double scale) {
  TORCH_CHECK(q.dim() == 3 && q.size(2) == kKvD, a.op(), ": q / out must be [T, Hq, 128]");
  const int B = seq_lens.numel();
  akap::AttnParams p{};
  p.Hq = q.size(1);
  p.Hkv = kv.Hkv;
  p.G = G;
  p.BS = kv.BS;
  TORCH_CHECK(p.Hq == p.Hkv * G, a.op(), ": Hq must equal Hkv * G");
  p.q = (const __bf16*)a.bf16(q, "q", rows * p.Hq * kKvD);
  p.out = (__bf16*)a.bf16(out, "out", q.numel());
  p.kv_fp8 = kv.fp8;
  p.k_cache = kv.k;
  p.v_cache = kv.v;
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) >= B, a.op(),
              ": block_tables must be [B, max_blocks], one row per sequence");
  p.block_tables = a.ptr<int>(block_tables, "block_tables", 0, kLastContig);
  p.bt_stride = block_tables.stride(0);
  p.seq_lens = a.ptr<int>(seq_lens, "seq_lens");
  p.scale_log2 = (float)(scale * 1.4426950408889634);
  return p;
}

// The prefill tile map: q_start [B+1] and the per-tile sequence / first-row maps, int32;
// tile_rows 128 | 256 (256: bf16 cache).  Returns the number of tiles.
int set_prefill_tiles(const OpArgs& a, akap::AttnParams& p, const Tensor& block_tables,
                      const Tensor& seq_lens, const Tensor& q_start, const Tensor& tile_seq,
                      const Tensor& tile_row, int64_t tile_rows) {
  TORCH_CHECK(tile_rows == 128 || tile_rows == 256, a.op(), ": tile_rows must be 128 or 256");
  TORCH_CHECK(tile_rows != 256 || !p.kv_fp8, a.op(), ": tile_rows=256 needs a bf16 KV cache");
  // the flash-style kernel caches a sequence's block ids in LDS: <= 32768 keys
  TORCH_CHECK(block_tables.size(1) * p.BS <= 32768, a.op(),
              ": prefill attention supports contexts up to 32768 tokens");
  const int num_tiles = tile_seq.numel();
  p.q_start = a.ptr<int>(q_start, "q_start", seq_lens.numel() + 1);
  p.tile_seq = a.ptr<int>(tile_seq, "tile_seq");
  p.tile_row = a.ptr<int>(tile_row, "tile_row", num_tiles);
  return num_tiles;
}

// The raw-QKV source of the ops whose kernel applies the per-head RMSNorm + RoPE itself: qkv
// bf16 [>= rows, >= (Hq + 2 Hkv) * 128] in 16-byte aligned rows (the kernels load 16-byte
// vectors from them), positions int64, cos_sin contiguous fp32 [P, 128], q_w / k_w contiguous
// bf16 [128] or absent.
void set_raw_qkv(const OpArgs& a, akap::AttnParams& p, const Tensor& qkv, int64_t rows,
                 const Tensor& positions, const Tensor& cos_sin,
                 const std::optional<Tensor>& q_w, const std::optional<Tensor>& k_w,
                 double eps) {
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) >= rows &&
                  qkv.size(1) >= (p.Hq + 2 * p.Hkv) * kKvD,
              a.op(), ": qkv must be [rows, >= (Hq + 2 Hkv) * 128]");
  TORCH_CHECK(qkv.stride(0) % 8 == 0, a.op(), ": qkv rows must be 16-byte aligned");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == kKvD, a.op(),
              ": cos_sin must be contiguous fp32 [max_pos, 128]");
  TORCH_CHECK((!q_w || q_w->numel() == kKvD) && (!k_w || k_w->numel() == kKvD), a.op(),
              ": q_w / k_w must be contiguous bf16 [128]");
  p.q = nullptr;
  p.qkv = (const __bf16*)a.bf16(qkv, "qkv", 0, kLastContig | kAlign16);
  p.qkv_stride = qkv.stride(0);
  p.positions = a.ptr<int64_t>(positions, "positions", rows);
  p.cos_sin = a.ptr<float>(cos_sin, "cos_sin");
  p.q_w = (const __bf16*)a.bf16(q_w, "q_w");
  p.k_w = (const __bf16*)a.bf16(k_w, "k_w");
  p.eps = (float)eps;
}

// The decode ops' split-KV fields: part_size, and with more than one part the fp32 partial
// max / sum / output workspaces
void set_split_kv(const OpArgs& a, akap::AttnParams& p, const Tensor& part_m,
                  const Tensor& part_l, const Tensor& part_o, int64_t num_parts,
                  int64_t part_size, int B) {
  TORCH_CHECK(part_size % 128 == 0 && part_size > 0 && part_size <= akap::kDecodeMaxPart,
              a.op(), ": part_size must be a multiple of 128, at most ", akap::kDecodeMaxPart);
  p.num_parts = num_parts;
  p.part_size = part_size;
  if (num_parts <= 1) return;
  const int64_t n = (int64_t)B * p.Hkv * num_parts * p.G;
  p.part_m = a.ptr<float>(part_m, "part_m", n);
  p.part_l = a.ptr<float>(part_l, "part_l", n);
  p.part_o = a.ptr<float>(part_o, "part_o", n * kKvD);
}

void paged_attention_prefill(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache,
                             Tensor block_tables, Tensor seq_lens, Tensor q_start,
                             Tensor tile_seq, Tensor tile_row, int64_t G, double scale,
                             int64_t tile_rows) {
  const OpArgs a = on_gpu("paged_attention_prefill", q, "q");
  const KVCache kv = kv_cache_of(a, k_cache, v_cache);
  auto p = attn_params(a, kv, out, q, block_tables, seq_lens, 0, G, scale);
  const int num_tiles =
      set_prefill_tiles(a, p, block_tables, seq_lens, q_start, tile_seq, tile_row, tile_rows);
  akap::launch_paged_attn_prefill(p, num_tiles, (int)tile_rows, cur_stream());
}

// Prefill attention that reads its q rows raw from the QKV projection and applies the per-head
// q RMSNorm (q_w, optional) and NeoX RoPE itself (attention.hip, prefill kernel prologue): the
// standalone qk_norm_rope_cache pass then writes q only for the decode rows of a mixed step
// (q_rows = num_decode), saving the q write and re-read of every prefill token.
// The rotary row of a q token is its key index kv_len - q_len + i: the same invariant the
// kernel's causal mask relies on, and what the engine's positions hold for every prefill
// token.  `positions` is shape-checked and passed through but not read by the kernel.
void paged_attention_prefill_qprep(Tensor out, Tensor qkv, Tensor k_cache, Tensor v_cache,
                                   Tensor block_tables, Tensor seq_lens, Tensor q_start,
                                   Tensor tile_seq, Tensor tile_row, Tensor positions,
                                   Tensor cos_sin, std::optional<Tensor> q_w, int64_t G,
                                   double scale, double eps, int64_t tile_rows) {
  const OpArgs a = on_gpu("paged_attention_prefill_qprep", qkv, "qkv");
  const KVCache kv = kv_cache_of(a, k_cache, v_cache);
  // `out` doubles as the q-shaped tensor for the shared parameter checks (same [T, Hq, D])
  auto p = attn_params(a, kv, out, out, block_tables, seq_lens, 0, G, scale);
  TORCH_CHECK(qkv.dim() == 2 && qkv.size(0) == out.size(0), a.op(),
              ": qkv / out token counts differ");
  set_raw_qkv(a, p, qkv, out.size(0), positions, cos_sin, q_w, std::nullopt, eps);
  const int num_tiles =
      set_prefill_tiles(a, p, block_tables, seq_lens, q_start, tile_seq, tile_row, tile_rows);
  akap::launch_paged_attn_prefill(p, num_tiles, (int)tile_rows, cur_stream());
}

void paged_attention_decode(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache,
                            Tensor block_tables, Tensor seq_lens, std::optional<Tensor> q_start,
                            Tensor part_m, Tensor part_l, Tensor part_o, int64_t num_parts,
                            int64_t part_size, int64_t G, double scale,
                            std::optional<Tensor> v_tail, std::optional<Tensor> tail_slot) {
  const OpArgs a = on_gpu("paged_attention_decode", q, "q");
  const KVCache kv = kv_cache_of(a, k_cache, v_cache);
  const int B = seq_lens.numel();
  // one q row per sequence unless q_start maps several to it
  auto p = attn_params(a, kv, out, q, block_tables, seq_lens, q_start ? 0 : B, G, scale);
  TORCH_CHECK(G <= 16, a.op(), ": the decode kernel supports up to 16 q heads per kv head");
  const VTail vt = v_tail_of(a, kv, v_tail, tail_slot, B);
  p.v_tail = (__bf16*)vt.v_tail;
  p.tail_slot = vt.tail_slot;
  p.q_start = a.ptr<int>(q_start, "q_start", B + 1);
  set_split_kv(a, p, part_m, part_l, part_o, num_parts, part_size, B);
  akap::launch_paged_attn_decode(p, B, cur_stream());
}

// Decode attention fused with the per-head q/k RMSNorm + RoPE + new-token K/V cache write:
// reads the raw QKV projection rows, so the standalone qk_norm_rope_cache launch (and its
// q round trip) disappears from every decode layer.
void paged_attention_decode_fused(Tensor out, Tensor qkv, Tensor k_cache, Tensor v_cache,
                                  Tensor block_tables, Tensor seq_lens, Tensor positions,
                                  Tensor slots, Tensor cos_sin, std::optional<Tensor> q_w,
                                  std::optional<Tensor> k_w, Tensor part_m, Tensor part_l,
                                  Tensor part_o, int64_t num_parts, int64_t part_size, int64_t G,
                                  double scale, double eps, std::optional<Tensor> v_tail,
                                  std::optional<Tensor> tail_slot, bool write_kv) {
  const OpArgs a = on_gpu("paged_attention_decode_fused", qkv, "qkv");
  const KVCache kv = kv_cache_of(a, k_cache, v_cache);
  const int B = seq_lens.numel();
  // `out` doubles as the q-shaped tensor, as in the q-prep prefill
  auto p = attn_params(a, kv, out, out, block_tables, seq_lens, B, G, scale);
  TORCH_CHECK(G + 2 <= 16, a.op(), ": fused decode supports up to 14 q heads per kv head");
  const VTail vt = v_tail_of(a, kv, v_tail, tail_slot, B);
  p.v_tail = (__bf16*)vt.v_tail;
  p.tail_slot = vt.tail_slot;
  set_raw_qkv(a, p, qkv, B, positions, cos_sin, q_w, k_w, eps);
  p.slots = a.ptr<int64_t>(slots, "slots", B);
  p.q_start = nullptr;
  if (!write_kv) {
    // the caller writes the new token's K / V (dgemm kv_write): the V-tail form only
    TORCH_CHECK(!kv.fp8 && vt.v_tail != nullptr, a.op(),
                ": write_kv=False needs a bf16 KV cache and a V tail");
    p.flags |= akap::kAttnCallerWritesKv;
  }
  set_split_kv(a, p, part_m, part_l, part_o, num_parts, part_size, B);
  akap::launch_paged_attn_decode(p, B, cur_stream());
}

// the tensors may have any dtype: the kernel only touches their bytes
void l2_prefetch(std::vector<Tensor> ts, Tensor sink) {
  TORCH_CHECK(ts.size() <= 8, "l2_prefetch: at most 8 tensors");
  const OpArgs a = on_gpu("l2_prefetch", sink, "sink");
  akap::PrefetchList L{};
  for (size_t i = 0; i < ts.size(); ++i) {
    L.ptr[i] = a.ptr(ts[i], "ts[i]", {ts[i].scalar_type()});
    L.bytes[i] = (long)ts[i].numel() * ts[i].element_size();
  }
  L.n = ts.size();
  akap::launch_l2_prefetch(L, reinterpret_cast<uint32_t*>(a.ptr<int>(sink, "sink", 1)),
                           cur_stream());
}

int64_t gemm_splitk(int64_t M, int64_t N, int64_t K) {
  return akap::gemm_splitk_choice(M, N, K);
}

void gemm(Tensor out, Tensor x, Tensor w, Tensor ws, int64_t splitk,
          std::optional<Tensor> counters) {
  const OpArgs a = on_gpu("gemm", x, "x");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && out.dim() == 2, "gemm: 2-D tensors");
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && out.size(0) == M && out.size(1) == N, "gemm: shape mismatch");
  TORCH_CHECK(K % 8 == 0 && N % 4 == 0, "gemm: K % 8, N % 4");
  TORCH_CHECK(x.stride(0) % 8 == 0 && w.stride(0) % 8 == 0, "gemm: 16-byte aligned rows");
  // split-K: fp32 workspace of splitk*M*N; counters: one L2 line (kCtrStride ints) per 64x64 tile
  float* wsp = splitk > 1 ? a.ptr<float>(ws, "workspace", splitk * M * N) : nullptr;
  int* cnt = splitk > 1 ? a.ptr<int>(counters, "counters",
                                     (int64_t)((M + 63) / 64) * ((N + 63) / 64) * akap::kCtrStride)
                        : nullptr;
  akap::launch_gemm_bf16(a.bf16(x, "x", 0, kLastContig), a.bf16(w, "w", 0, kLastContig),
                         a.bf16(out, "out", 0, kLastContig), wsp, M, N, K, x.stride(0),
                         w.stride(0), out.stride(0), splitk, cur_stream(), cnt);
}

// Fused decode GEMM: out = prologue(x, ...) @ w^T, then an epilogue.
// pro 0 plain (optional ss_in row scale), 1 residual-add + RMSNorm (r = residual in,
// rout = x + r out, ln = norm weight), 2 SiLU(gate) * up over x = [gate|up].
// epi 0 store, 1 residual/next-norm (out = residual in/out, aout = bf16(out * ln_out),
// ss_out += row sums of squares), 2 SwiGLU over gate/up-interleaved rows (out [M, N/2]).
// Compute units of a device (cached): the persistent / in-launch-combine GEMM grids must fit.
static int device_cus(int dev) {
  static int cached[16] = {0};
  if (dev < 0 || dev >= 16) dev = 0;
  if (cached[dev] == 0) {
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cached[dev] = n;
  }
  return cached[dev];
}

// The checks and DGemmArgs fields dgemm() and kgemm() share: bf16 GPU operands with aligned rows,
// out / x / w pointers, sizes and strides, eps, the epilogue, the process-default weight policy
// and K stagger, the optional ss_in row scale and the EPI_RESNORM operands.
static akap::DGemmArgs dgemm_args(const OpArgs& o, const Tensor& out, const Tensor& x,
                                  const Tensor& w, double eps, int64_t epi,
                                  const std::optional<Tensor>& ss_in,
                                  const std::optional<Tensor>& ss_out,
                                  const std::optional<Tensor>& aout,
                                  const std::optional<Tensor>& ln_out) {
  const char* op = o.op();
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && out.dim() == 2, op, ": 2-D tensors");
  const int M = x.size(0), N = w.size(0), K = w.size(1);
  TORCH_CHECK(x.stride(0) % 8 == 0 && w.stride(0) % 8 == 0 && out.stride(0) % 4 == 0,
              op, ": 16-byte aligned rows");
  akap::DGemmArgs a{};
  a.ntw = akap::weight_nt_default();
  a.stag = akap::gemm_stagger_default();
  a.X = o.bf16(x, "x", 0, kLastContig);
  a.W = o.bf16(w, "w", 0, kLastContig);
  a.Y = o.bf16(out, "out", 0, kLastContig);
  a.M = M; a.N = N; a.K = K;
  a.ldx = x.stride(0); a.ldw = w.stride(0); a.ldy = out.stride(0);
  a.eps = (float)eps;
  a.epi = (int)epi;
  a.ss_in = o.ptr<float>(ss_in, "ss_in", M);
  if (epi == akap::EPI_RESNORM) {
    TORCH_CHECK(ss_out && aout && ln_out, op, ": resnorm epilogue needs ss_out, aout, ln_out");
    TORCH_CHECK(aout->numel() == (int64_t)M * N && ln_out->numel() == N,
                op, ": resnorm aout [M, N], ln_out [N]");
    TORCH_CHECK(out.stride(0) == N, op, ": resnorm residual must be dense");
    a.ss_out = o.ptr<float>(*ss_out, "ss_out", M);
    a.Aout = o.bf16(*aout, "aout");
    a.ln_out = o.bf16(*ln_out, "ln_out", N);
  }
  return a;
}

// kv_write of dgemm(): [qkv, positions, slots, cos_sin, k_w (no elements: no k norm), k_cache,
// v_cache, v_tail, tail_slot] of the decode step whose new-token K / V rows rider workgroups of
// this launch write (kernels/kv_write.h), one row of each per sequence: B = positions.numel().
// blocks > 0 caps the riders (1: one rider loops over every row).  The launch must be one the
// riders are legal on (kv_rider_blocks of host_contract.h): asking otherwise is an error, not a
// launch that quietly leaves the cache unwritten.
static akap::KvWriteArgs kv_write_args(const OpArgs& o, const std::vector<Tensor>& t, int64_t Hq,
                                       int64_t blocks, double eps, int M, int N, int pro, int epi,
                                       int splitk, int bn, int ns, int bm, int cus) {
  TORCH_CHECK(t.size() == 9, o.op(), ": kv_write takes 9 tensors");
  const Tensor &qkv = t[0], &positions = t[1], &slots = t[2], &cos_sin = t[3], &k_w = t[4];
  const KVCache kv = kv_cache_of(o, t[5], t[6]);
  const int B = positions.numel();
  const VTail vt = v_tail_of(o, kv, t[7], t[8], B);
  TORCH_CHECK(!kv.fp8 && t[7].size(0) >= 1, o.op(), ": kv_write needs a bf16 KV cache");
  TORCH_CHECK(Hq > 0 && qkv.dim() == 2 && qkv.size(0) >= B &&
                  qkv.size(1) >= (Hq + 2 * kv.Hkv) * kKvD && qkv.stride(0) % 8 == 0,
              o.op(), ": kv_write qkv must be [>= B, >= (Hq + 2 Hkv) * 128] in 16-byte rows");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == kKvD, o.op(),
              ": kv_write cos_sin must be contiguous fp32 [max_pos, 128]");
  TORCH_CHECK(k_w.numel() == 0 || k_w.numel() == kKvD, o.op(),
              ": kv_write k_w must be bf16 [128]");
  const int room = pro == akap::PRO_PLAIN
                       ? akap::kv_rider_blocks(M, N, epi, splitk, bn, ns, bm, cus, B, kv.Hkv, true,
                                               1, true, false)
                       : 0;
  TORCH_CHECK(room > 0, o.op(), ": this launch cannot carry K/V riders (kv_rider_blocks)");
  akap::KvWriteArgs k{};
  k.qkv = o.bf16(qkv, "kv_write qkv", 0, kLastContig | kAlign16);
  k.qkv_stride = qkv.stride(0);
  k.positions = o.ptr<int64_t>(positions, "kv_write positions", B);
  k.slots = o.ptr<int64_t>(slots, "kv_write slots", B);
  k.cos_sin = o.ptr<float>(cos_sin, "kv_write cos_sin");
  k.k_w = k_w.numel() ? o.bf16(k_w, "kv_write k_w", kKvD) : nullptr;
  k.eps = (float)eps;
  k.k_cache = kv.k;
  k.v_cache = kv.v;
  k.v_tail = vt.v_tail;
  k.tail_slot = vt.tail_slot;
  k.Hq = (int)Hq;
  k.Hkv = kv.Hkv;
  k.BS = kv.BS;
  k.B = B;
  k.n_blocks = blocks > 0 && blocks < room ? (int)blocks : room;
  return k;
}

void dgemm(Tensor out, Tensor x, Tensor w, Tensor ws, int64_t pro, int64_t splitk, int64_t pf,
           std::optional<Tensor> r, std::optional<Tensor> rout, std::optional<Tensor> ln,
           double eps, int64_t epi, std::optional<Tensor> ss_in, std::optional<Tensor> ss_out,
           std::optional<Tensor> aout, std::optional<Tensor> ln_out, int64_t bn, int64_t ns,
           std::optional<Tensor> counters, int64_t bm,
           std::optional<std::vector<Tensor>> kv_write,
           int64_t kv_hq, int64_t kv_blocks, double kv_eps) {
  TORCH_CHECK(pro >= 0 && pro <= 2, "dgemm: prologue 0|1|2");
  TORCH_CHECK(epi >= 0 && epi <= 2, "dgemm: epilogue 0|1|2");
  const OpArgs o = on_gpu("dgemm", x, "x");
  // the ss_in row scale belongs to the plain prologue (the others have their own)
  akap::DGemmArgs a = dgemm_args(o, out, x, w, eps, epi,
                                 pro == akap::PRO_PLAIN ? ss_in : std::nullopt, ss_out, aout,
                                 ln_out);
  const int M = a.M, N = a.N, K = a.K;
  TORCH_CHECK(x.size(1) == (pro == akap::PRO_SILU ? 2 * K : K), "dgemm: x width");
  TORCH_CHECK(out.size(0) == M && out.size(1) == (epi == akap::EPI_SILU ? N / 2 : N),
              "dgemm: out shape");
  // what the launch accepts and needs: host_contract.h (offering counters asks for the
  // in-launch combine)
  const akap::DGemmContract c =
      akap::dgemm_contract(M, N, K, (int)pro, (int)epi, (int)splitk, (int)pf, (int)bn, (int)ns,
                           (int)bm, counters.has_value(), device_cus(x.device().index()));
  TORCH_CHECK(c.supported, "dgemm: unsupported M/N/K/pro/epi/splitk/pf/bn/bm");
  if (splitk > 1) {
    // fp32 workspace of splitk*M*N (+ splitk*M for the norm)
    a.ws = o.ptr<float>(ws, "workspace", c.ws_floats);
    TORCH_CHECK(out.stride(0) == N || c.inlaunch,
                "dgemm: split-K output must be dense (separate reduce pass)");
  }
  a.bn = (int)bn;
  a.ns = (int)ns;
  a.bm = (int)bm;
  if (c.ticket_ints > 0) {
    // in-launch split-K combine: one zeroed int32 ticket per output tile, each on its own L2
    // line (bn=256: 2 per tile, the kCtrInts array)
    TORCH_CHECK(counters.has_value(), "dgemm: counters needed by the in-launch split-K combine");
    a.counters = o.ptr<int>(*counters, "counters", c.ticket_ints);
  }
  if (pro == akap::PRO_ADDNORM) {
    TORCH_CHECK(r && rout && ln, "dgemm: addnorm needs residual, residual-out and norm weight");
    TORCH_CHECK(r->numel() == (int64_t)M * K && rout->numel() == (int64_t)M * K &&
                ln->numel() == K, "dgemm: addnorm residual [M, K], norm weight [K]");
    a.R = o.bf16(*r, "r");
    a.Rout = o.bf16(*rout, "rout");
    a.ln = o.bf16(*ln, "ln");
    TORCH_CHECK(a.R != a.Rout, "dgemm: rout must not alias r");
  }
  if (kv_write.has_value())
    a.kv = kv_write_args(o, *kv_write, kv_hq, kv_blocks, kv_eps, M, N, (int)pro, (int)epi,
                         (int)splitk, (int)bn, (int)ns, (int)bm,
                         device_cus(x.device().index()));
  if (c.family == akap::DG_PGEMM_SK) {
    akap::launch_pgemm_sk(a, (int)splitk, cur_stream());
    return;
  }
  akap::launch_dgemm(a, (int)pro, (int)splitk, (int)pf, cur_stream());
}

// Wide-row weight-streaming GEMM (LM head): out[M, N] = x[M, K] @ w[N, K]^T, one workgroup
// per column tile holding all (<= 256) rows, so the weights cross HBM -> CU once.
void wgemm(Tensor out, Tensor x, Tensor w) {
  const OpArgs o = on_gpu("wgemm", x, "x");
  TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && out.dim() == 2, "wgemm: 2-D tensors");
  const int M = x.size(0), N = w.size(0), K = w.size(1);
  TORCH_CHECK(x.size(1) == K && out.size(0) == M && out.size(1) == N, "wgemm: shapes");
  TORCH_CHECK(akap::wgemm_supported(M, N, K, x.stride(0), w.stride(0), out.stride(0)),
              "wgemm: K % 64 == 0 and 16-byte aligned rows");
  akap::WGemmArgs a{o.bf16(x, "x", 0, kLastContig), o.bf16(w, "w", 0, kLastContig),
                    o.bf16(out, "out", 0, kLastContig), M, N, K,
                    (int)x.stride(0), (int)w.stride(0), (int)out.stride(0)};
  akap::launch_wgemm(a, cur_stream());
}

// What qgemm and q4gemm share: x [M, K] and out [M, N] bf16 with 16-byte aligned rows.  The
// caller has checked the dimension counts, read (N, K) from its weight and checked its scale's
// shape; it passes its *_supported predicate and what that needs, and fills Wq and scale.
static akap::QGemmArgs qgemm_args(const OpArgs& o, const Tensor& out, const Tensor& x, int N,
                                  int K, bool (*supported)(int, int, int, int, int),
                                  const char* needs) {
  const char* op = o.op();
  const int M = x.size(0);
  TORCH_CHECK(x.size(1) == K && out.size(0) == M && out.size(1) == N, op, ": shapes");
  TORCH_CHECK(M == 0 || supported(M, N, K, x.stride(0), out.stride(0)), op, ": needs ", needs);
  akap::QGemmArgs a{};
  a.X = o.bf16(x, "x", 0, kLastContig | kAlign16);
  a.Y = o.bf16(out, "out", 0, kLastContig | kAlign16);
  a.M = M; a.N = N; a.K = K;
  a.ldx = x.stride(0); a.ldy = out.stride(0);
  return a;
}

// FP8-weight decode GEMM (csrc/kernels/qgemm.hip): out[M, N] = bf16(scale[n] * x[M, K] @
// float(wq[N, K])^T), wq = OCP e4m3fn bytes (uint8 or float8_e4m3fn), scale fp32 per channel.
void qgemm(Tensor out, Tensor x, Tensor wq, Tensor scale) {
  const OpArgs o = on_gpu("qgemm", x, "x");
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 2 && out.dim() == 2 && scale.dim() == 1,
              "qgemm: x, wq, out 2-D and scale 1-D");
  const int N = wq.size(0), K = wq.size(1);
  TORCH_CHECK(scale.size(0) == N, "qgemm: shapes");
  akap::QGemmArgs a = qgemm_args(o, out, x, N, K, akap::qgemm_supported,
                                 "M <= 256, K % 64 == 0, N % 8 == 0 and 16-byte aligned rows");
  a.Wq = o.ptr(wq, "wq", {at::kByte, at::kFloat8_e4m3fn}, 0, kContig | kAlign16);
  a.scale = o.ptr<float>(scale, "scale", N, kContig | kAlign16);
  akap::launch_qgemm(a, cur_stream());
}

// out[N, K] bf16 = bf16(float(wq) * scale[:, None]) (one fp32 multiply, RNE cast)
void dequant_fp8(Tensor out, Tensor wq, Tensor scale) {
  const OpArgs o = on_gpu("dequant_fp8", wq, "wq");
  TORCH_CHECK(wq.dim() == 2 && out.dim() == 2 && scale.dim() == 1, "dequant_fp8: dims");
  const int64_t N = wq.size(0), K = wq.size(1);
  TORCH_CHECK(out.size(0) == N && out.size(1) == K && scale.size(0) == N, "dequant_fp8: shapes");
  TORCH_CHECK(K % 16 == 0, "dequant_fp8: K % 16 == 0");
  const unsigned vec = kContig | kAlign16;
  akap::launch_dequant_fp8(o.ptr(wq, "wq", {at::kByte, at::kFloat8_e4m3fn}, 0, vec),
                           o.ptr<float>(scale, "scale", N), o.bf16(out, "out", 0, vec), N, (int)K,
                           cur_stream());
}

// MXFP4-weight decode GEMM (csrc/kernels/q4gemm.hip): out[M, N] = bf16(x[M, K] @ deq(wq)^T),
// wq = packed e2m1 codes uint8 [N, K/2], scale = e8m0 codes uint8 [N, K/32].
void q4gemm(Tensor out, Tensor x, Tensor wq, Tensor scale) {
  const OpArgs o = on_gpu("q4gemm", x, "x");
  TORCH_CHECK(x.dim() == 2 && wq.dim() == 2 && out.dim() == 2 && scale.dim() == 2,
              "q4gemm: x, wq, scale and out 2-D");
  const int N = wq.size(0), K = 2 * wq.size(1);
  TORCH_CHECK(K % akap::MXBLK == 0 && scale.size(0) == N && scale.size(1) == K / akap::MXBLK,
              "q4gemm: scale must be [N, K/32]");
  akap::Q4GemmArgs a{qgemm_args(o, out, x, N, K, akap::q4gemm_supported,
                                "M <= 256, K >= 128, K % 128 == 0, N % 8 == 0 and 16-byte "
                                "aligned rows")};
  a.Wq = o.ptr<uint8_t>(wq, "wq", (int64_t)N * (K / 2), kContig | kAlign16);
  a.scale = o.ptr<uint8_t>(scale, "scale", (int64_t)N * (K / akap::MXBLK), kContig | kAlign16);
  akap::launch_q4gemm(a, cur_stream());
}

// out[N, K] bf16 = e2m1(wq) * 2^(scale - 127), exact
void dequant_mxfp4(Tensor out, Tensor wq, Tensor scale) {
  const OpArgs o = on_gpu("dequant_mxfp4", wq, "wq");
  TORCH_CHECK(wq.dim() == 2 && out.dim() == 2 && scale.dim() == 2, "dequant_mxfp4: dims");
  const int64_t N = wq.size(0), K = 2 * wq.size(1);
  TORCH_CHECK(K % akap::MXBLK == 0, "dequant_mxfp4: K % 32 == 0");
  TORCH_CHECK(out.size(0) == N && out.size(1) == K && scale.size(0) == N &&
                  scale.size(1) == K / akap::MXBLK, "dequant_mxfp4: shapes");
  const unsigned vec = kContig | kAlign16;
  akap::launch_dequant_mxfp4(o.ptr<uint8_t>(wq, "wq", N * (K / 2), vec),
                             o.ptr<uint8_t>(scale, "scale", N * (K / akap::MXBLK)),
                             o.bf16(out, "out", N * K, vec), N, (int)K, cur_stream());
}

// Narrow-output decode GEMM with the K split inside the workgroup (csrc/kernels/kgemm.hip):
// out = x @ w^T (rows scaled by rsqrt(ss_in / K + eps) when ss_in is given), epi 0 store,
// 1 residual/next-norm (out = residual in/out, aout = bf16(out * ln_out), ss_out += row sums).
void kgemm(Tensor out, Tensor x, Tensor w, int64_t bm, int64_t epi, double eps,
           std::optional<Tensor> ss_in, std::optional<Tensor> ss_out, std::optional<Tensor> aout,
           std::optional<Tensor> ln_out) {
  TORCH_CHECK(epi == 0 || epi == 1, "kgemm: epilogue 0|1");
  const OpArgs o = on_gpu("kgemm", x, "x");
  const akap::DGemmArgs a = dgemm_args(o, out, x, w, eps, epi, ss_in, ss_out, aout, ln_out);
  const int M = a.M, N = a.N, K = a.K;
  TORCH_CHECK(x.size(1) == K && out.size(0) == M && out.size(1) == N, "kgemm: shapes");
  TORCH_CHECK(akap::kgemm_supported(M, N, K, (int)bm, (int)epi), "kgemm: bm 16|32, N % 32, K % 256");
  akap::launch_kgemm(a, (int)bm, cur_stream());
}

// fp32 or bf16 logits [B, V] with unit last stride
void* logits_of(const OpArgs& a, const Tensor& logits) {
  TORCH_CHECK(logits.dim() == 2, a.op(), ": logits must be [B, V]");
  return a.ptr(logits, "logits", {at::kFloat, at::kBFloat16}, 0, kLastContig);
}

void sample(Tensor logits, Tensor temperature, Tensor top_k, Tensor top_p, Tensor seeds,
            Tensor steps, Tensor out_tokens, Tensor out_logprobs, bool greedy_logprobs,
            Tensor ws, Tensor tickets, bool filtered) {
  const OpArgs a = on_gpu("sample", logits, "logits");
  akap::SampleParams p{};
  p.logits = logits_of(a, logits);
  const int B = logits.size(0);
  TORCH_CHECK(logits.size(1) >= 1 && logits.size(1) <= akap::kSampleMaxVocab,
              "sample: logits rows of 1 .. ", akap::kSampleMaxVocab, " entries");
  p.is_bf16 = logits.scalar_type() == at::kBFloat16;
  p.ld = logits.stride(0);
  p.V = logits.size(1);
  // one parameter / output entry per row
  p.temperature = a.ptr<float>(temperature, "temperature", B);
  p.top_k = a.ptr<int>(top_k, "top_k", B);
  p.top_p = a.ptr<float>(top_p, "top_p", B);
  p.seeds = a.ptr<int64_t>(seeds, "seeds", B);
  p.steps = a.ptr<int>(steps, "steps", B);
  p.out_tokens = a.ptr<int64_t>(out_tokens, "out_tokens", B);
  p.out_logprobs = a.ptr_unless_empty<float>(out_logprobs, "out_logprobs", B);
  p.greedy_logprobs = greedy_logprobs ? 1 : 0;
  // workspace: per-(row, chunk) 32-byte partial records + filter-pass states / histograms, and
  // one ticket per row, each on its own L2 line (ops.sample keeps both persistent; the tickets
  // are zeroed once and re-armed by each row's last chunk)
  akap::launch_sample(p, B, a.ptr<float>(ws, "workspace", (int64_t)akap::sample_ws_floats(B)),
                      a.ptr<int>(tickets, "tickets", (int64_t)B * akap::kCtrStride),
                      filtered ? 1 : 0, cur_stream());
}

// presence / frequency / repetition are indexed by the row numbers in `rows`, which only the
// device knows: the engine sizes them by its sampled rows, so the host can only ask that the
// three are equally long
void apply_penalties(Tensor logits, Tensor rows, Tensor toks, Tensor counts, Tensor presence,
                     Tensor frequency, Tensor repetition) {
  const OpArgs a = on_gpu("apply_penalties", logits, "logits");
  const int n = rows.numel();
  TORCH_CHECK(toks.numel() == n && counts.numel() == n, "apply_penalties: COO length mismatch");
  const int64_t np = n ? std::max<int64_t>(presence.numel(), 1) : 0;
  akap::launch_apply_penalties(logits_of(a, logits), logits.stride(0),
                               logits.scalar_type() == at::kBFloat16, a.ptr<int>(rows, "rows"),
                               a.ptr<int>(toks, "toks", n), a.ptr<int>(counts, "counts", n),
                               a.ptr<float>(presence, "presence", np),
                               a.ptr<float>(frequency, "frequency", np),
                               a.ptr<float>(repetition, "repetition", np), n, cur_stream());
}

void argmax(Tensor logits, Tensor out) {
  const OpArgs a = on_gpu("argmax", logits, "logits");
  akap::launch_argmax(logits_of(a, logits), logits.stride(0), logits.size(1),
                      logits.scalar_type() == at::kBFloat16,
                      a.ptr<int64_t>(out, "out", logits.size(0)), logits.size(0), cur_stream());
}

void moe_topk_softmax(Tensor logits, Tensor topk_w, Tensor topk_ids, bool renorm) {
  const OpArgs a = on_gpu("moe_topk_softmax", logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) <= 256, "moe_topk_softmax: at most 256 experts");
  TORCH_CHECK(topk_w.size(1) >= 1 && topk_w.size(1) <= 8 && topk_w.size(1) <= logits.size(1),
              "moe_topk_softmax: top-k in 1..min(8, E)");
  TORCH_CHECK(topk_ids.sizes() == topk_w.sizes() && topk_w.size(0) == logits.size(0),
              "moe_topk_softmax: topk_w / topk_ids [T, K]");
  akap::launch_moe_topk_softmax(a.bf16(logits, "logits", 0, kLastContig), logits.stride(0),
                                logits.size(1), topk_w.size(1), a.ptr<float>(topk_w, "topk_w"),
                                a.ptr<int32_t>(topk_ids, "topk_ids"), logits.size(0),
                                renorm ? 1 : 0, cur_stream());
}

void moe_router_topk(Tensor h, Tensor router, Tensor topk_w, Tensor topk_ids, bool renorm) {
  const OpArgs a = on_gpu("moe_router_topk", h, "h");
  TORCH_CHECK(h.dim() == 2 && router.dim() == 2 && topk_w.dim() == 2, "moe_router_topk: 2-D");
  const int T = h.size(0), d = h.size(1), E = router.size(0), K = topk_w.size(1);
  TORCH_CHECK(router.size(1) == d, "moe_router_topk: router shape");
  TORCH_CHECK(akap::moe_router_topk_supported(E, d),
              "moe_router_topk: the fused router supports <= 16 experts, d % 8 == 0");
  TORCH_CHECK(topk_w.size(0) >= T && topk_ids.size(0) >= T, "moe_router_topk: outputs too small");
  TORCH_CHECK(h.stride(0) % 8 == 0, "moe_router_topk: h rows must be 16-byte aligned");
  akap::launch_moe_router_topk(a.bf16(h, "h", 0, kLastContig | kAlign16), h.stride(0),
                               a.bf16(router, "router"), d, E, K,
                               a.ptr<float>(topk_w, "topk_w", (int64_t)T * K),
                               a.ptr<int32_t>(topk_ids, "topk_ids", (int64_t)T * K), T,
                               renorm ? 1 : 0, cur_stream());
}

void moe_align(Tensor topk_ids, int64_t E, int64_t block, Tensor sorted_ids, Tensor offsets,
               Tensor num_padded, Tensor inv, Tensor tile_expert) {
  const OpArgs a = on_gpu("moe_align", topk_ids, "topk_ids");
  const int n = topk_ids.numel();
  const int max_tiles = tile_expert.numel();
  TORCH_CHECK(max_tiles == 0 || (int64_t)max_tiles * block >= sorted_ids.numel(),
              "moe_align: tile_expert must cover sorted_ids");
  akap::launch_moe_align(a.ptr<int32_t>(topk_ids, "topk_ids"), n, E, block,
                         a.ptr<int32_t>(sorted_ids, "sorted_ids", n + E * (block - 1)),
                         a.ptr<int32_t>(offsets, "offsets", E + 1),
                         a.ptr<int32_t>(num_padded, "num_padded", 1),
                         a.ptr_unless_empty<int32_t>(inv, "inv", n),
                         a.ptr_unless_empty<int32_t>(tile_expert, "tile_expert"), max_tiles,
                         cur_stream());
}

void moe_gemm(Tensor out, Tensor a, Tensor w, Tensor sorted_ids, Tensor tile_expert,
              int64_t n_flat, int64_t topk, bool gather) {
  const OpArgs o = on_gpu("moe_gemm", a, "a");
  TORCH_CHECK(w.dim() == 3 && a.dim() == 2 && out.dim() == 2, "moe_gemm: expert weights [E, N, K]");
  const int N = w.size(1), K = w.size(2);
  TORCH_CHECK(a.size(1) == K && out.size(1) == N, "moe_gemm: shape mismatch");
  TORCH_CHECK(K % 8 == 0, "moe_gemm: K % 8");
  const int max_tiles = tile_expert.numel();
  const int64_t rows = (int64_t)max_tiles * 64;
  TORCH_CHECK(out.size(0) >= rows, "moe_gemm: out rows must cover all tiles");
  TORCH_CHECK(gather || a.size(0) >= rows, "moe_gemm: a rows must cover all tiles");
  akap::launch_moe_gemm(o.bf16(a, "a", 0, kLastContig), o.bf16(w, "w"), o.bf16(out, "out"),
                        o.ptr<int32_t>(sorted_ids, "sorted_ids"),  // read for live tiles only
                        o.ptr<int32_t>(tile_expert, "tile_expert"), max_tiles, n_flat, topk, N, K,
                        a.stride(0), gather ? 1 : 0, cur_stream());
}

// What moe_dgemm / moe_qgemm / moe_q4gemm hand to their launchers besides the weights.
struct MoeGemmArgs {
  const void* a;
  void* y;          // bf16 [rows, out width], or null with splitk > 1
  float* partials;  // splitk > 1: fp32 [splitk, rows, N]
  const int32_t* sorted_ids;
  const int32_t* tile_expert;
  int max_tiles, n_flat, topk, lda, ldy, gather, silu, pf, bm, splitk;
  bool ntw;
};

// The checks and arguments the three grouped expert GEMMs share.  The caller has checked its
// weight and scale shapes (E experts of [N, K]) and passes its *_supported predicate's answer.
// out: bf16 [rows, N] (or [rows, N/2] with silu); splitk > 1: out is an fp32 partials buffer
// [splitk, rows, N] consumed by moe_combine_split.
static MoeGemmArgs moe_gemm_args(const OpArgs& o, const Tensor& out, const Tensor& a,
                                 const Tensor& sorted_ids, const Tensor& tile_expert, int64_t E,
                                 int N, int K, bool supported, int64_t n_flat, int64_t topk,
                                 bool gather, bool silu, int64_t pf, int64_t bm, int64_t splitk) {
  const char* op = o.op();
  TORCH_CHECK(a.size(1) == K, op, ": a width != K");
  TORCH_CHECK(supported, op, ": unsupported N/K/pf/split");
  TORCH_CHECK(a.stride(0) % 8 == 0, op, ": 16-byte aligned rows");
  TORCH_CHECK(bm == 32 || bm == 64, op, ": tile rows 32 | 64");
  TORCH_CHECK(topk >= 1 && n_flat >= 0, op, ": topk >= 1, n_flat >= 0");
  MoeGemmArgs g{};
  g.max_tiles = tile_expert.numel();
  const int64_t rows = (int64_t)g.max_tiles * bm;
  g.partials = splitk > 1 ? o.ptr<float>(out, "out", splitk * rows * N) : nullptr;
  g.y = splitk > 1 ? nullptr : o.bf16(out, "out");
  TORCH_CHECK(splitk > 1 || (out.dim() == 2 && out.size(1) == (silu ? N / 2 : N)),
              op, ": out width");
  TORCH_CHECK(splitk > 1 || out.size(0) >= rows, op, ": out rows must cover all tiles");
  TORCH_CHECK(gather ? a.size(0) * topk >= n_flat : a.size(0) >= rows,
              op, ": a rows must cover all tiles (gather: all n_flat / topk tokens)");
  // Non-temporal expert-weight loads when each expert's weights are streamed by one row tile
  // (64-row tiles, <= 40 rows per expert on average): measured on MI355X, Mixtral T=128,
  // w13 345 -> 319 us, w2 (split 4) 226 -> 215 us; with 32-row tiles an expert's second tile
  // re-reads its weights and nt loses (bench/moe_gemm_micro.py, profiles/r2_moe_nt.log).
  // AKAP_MOE_NT=0|1 overrides.
  static const int nt_env = [] {
    const char* e = std::getenv("AKAP_MOE_NT");
    return e ? std::atoi(e) : -1;
  }();
  g.ntw = nt_env >= 0 ? nt_env != 0 : (bm == 64 && n_flat <= 40 * E);
  g.a = o.bf16(a, "a", 0, kLastContig | kAlign16);
  g.sorted_ids = o.ptr<int32_t>(sorted_ids, "sorted_ids", rows);
  g.tile_expert = o.ptr<int32_t>(tile_expert, "tile_expert");
  g.n_flat = n_flat; g.topk = topk;
  g.lda = a.stride(0); g.ldy = splitk > 1 ? N : out.stride(0);
  g.gather = gather ? 1 : 0; g.silu = silu ? 1 : 0;
  g.pf = (int)pf; g.bm = (int)bm; g.splitk = (int)splitk;
  return g;
}

void moe_dgemm(Tensor out, Tensor a, Tensor w, Tensor sorted_ids, Tensor tile_expert,
               int64_t n_flat, int64_t topk, bool gather, bool silu, int64_t pf, int64_t bm,
               int64_t splitk) {
  const OpArgs o = on_gpu("moe_dgemm", a, "a");
  TORCH_CHECK(w.dim() == 3 && a.dim() == 2, "moe_dgemm: a [rows, K], expert weights [E, N, K]");
  const int N = w.size(1), K = w.size(2);
  const MoeGemmArgs g = moe_gemm_args(o, out, a, sorted_ids, tile_expert, w.size(0), N, K,
                                      akap::moe_dgemm_supported(N, K, pf, silu, splitk), n_flat,
                                      topk, gather, silu, pf, bm, splitk);
  akap::launch_moe_dgemm(g.a, o.bf16(w, "w"), g.y, g.sorted_ids, g.tile_expert, g.max_tiles,
                         g.n_flat, g.topk, N, K, g.lda, g.ldy, g.gather, g.silu, g.pf, g.bm,
                         g.splitk, g.partials, g.ntw, cur_stream());
}

// moe_dgemm over FP8 expert weights (csrc/kernels/moe_qgemm.hip): wq uint8 / float8_e4m3fn
// [E, N, K] e4m3fn codes, scale fp32 [E, N]; out as moe_dgemm's.
void moe_qgemm(Tensor out, Tensor a, Tensor wq, Tensor scale, Tensor sorted_ids,
               Tensor tile_expert, int64_t n_flat, int64_t topk, bool gather, bool silu,
               int64_t pf, int64_t bm, int64_t splitk) {
  const OpArgs o = on_gpu("moe_qgemm", a, "a");
  TORCH_CHECK(wq.dim() == 3 && a.dim() == 2,
              "moe_qgemm: a [rows, K], expert weights wq [E, N, K]");
  const int64_t E = wq.size(0);
  const int N = wq.size(1), K = wq.size(2);
  TORCH_CHECK(scale.dim() == 2 && scale.size(0) == E && scale.size(1) == N,
              "moe_qgemm: scale must be [E, N]");
  const MoeGemmArgs g = moe_gemm_args(o, out, a, sorted_ids, tile_expert, E, N, K,
                                      akap::moe_qgemm_supported(N, K, pf, silu, splitk), n_flat,
                                      topk, gather, silu, pf, bm, splitk);
  akap::launch_moe_qgemm(g.a,
                         o.ptr(wq, "wq", {at::kByte, at::kFloat8_e4m3fn}, 0, kContig | kAlign16),
                         o.ptr<float>(scale, "scale", E * N), g.y, g.sorted_ids, g.tile_expert,
                         g.max_tiles, g.n_flat, g.topk, N, K, g.lda, g.ldy, g.gather, g.silu,
                         g.pf, g.bm, g.splitk, g.partials, g.ntw, cur_stream());
}

// moe_dgemm over MXFP4 expert weights (csrc/kernels/moe_q4gemm.hip): wq uint8 [E, N, K/2] packed
// e2m1 codes, scale uint8 [E, N, K/32] e8m0 codes; out as moe_dgemm's.
void moe_q4gemm(Tensor out, Tensor a, Tensor wq, Tensor scale, Tensor sorted_ids,
                Tensor tile_expert, int64_t n_flat, int64_t topk, bool gather, bool silu,
                int64_t pf, int64_t bm, int64_t splitk) {
  const OpArgs o = on_gpu("moe_q4gemm", a, "a");
  TORCH_CHECK(wq.dim() == 3 && a.dim() == 2,
              "moe_q4gemm: a [rows, K], expert weights wq [E, N, K/2]");
  const int64_t E = wq.size(0);
  const int N = wq.size(1), K = 2 * wq.size(2);
  TORCH_CHECK(K % akap::MXBLK == 0 && scale.dim() == 3 && scale.size(0) == E &&
                  scale.size(1) == N && scale.size(2) == K / akap::MXBLK,
              "moe_q4gemm: scale must be [E, N, K/32]");
  const MoeGemmArgs g = moe_gemm_args(o, out, a, sorted_ids, tile_expert, E, N, K,
                                      akap::moe_q4gemm_supported(N, K, pf, silu, splitk), n_flat,
                                      topk, gather, silu, pf, bm, splitk);
  akap::launch_moe_q4gemm(g.a, o.ptr<uint8_t>(wq, "wq", E * N * (K / 2), kContig | kAlign16),
                          o.ptr<uint8_t>(scale, "scale", E * N * (K / akap::MXBLK),
                                         kContig | kAlign16),
                          g.y, g.sorted_ids, g.tile_expert, g.max_tiles, g.n_flat, g.topk, N, K,
                          g.lda, g.ldy, g.gather, g.silu, g.pf, g.bm, g.splitk, g.partials, g.ntw,
                          cur_stream());
}

void moe_combine_split(Tensor partials, Tensor wts, Tensor inv, Tensor out, int64_t splitk,
                       int64_t rows) {
  const OpArgs a = on_gpu("moe_combine_split", partials, "partials");
  TORCH_CHECK(out.dim() == 2 && wts.dim() == 2, "moe_combine_split: out [T, d], wts [T, topk]");
  const int T = out.size(0), d = out.size(1), topk = wts.size(1);
  TORCH_CHECK(d % 8 == 0, "moe_combine_split: d % 8");
  akap::launch_moe_combine_split(a.ptr<float>(partials, "partials", splitk * rows * d),
                                 a.ptr<float>(wts, "wts", (int64_t)T * topk),
                                 a.ptr<int32_t>(inv, "inv", (int64_t)T * topk),
                                 a.bf16(out, "out"), T, topk, d, (int)splitk, (int)rows,
                                 cur_stream());
}

void moe_combine(Tensor y, Tensor wts, Tensor inv, Tensor out) {
  const OpArgs a = on_gpu("moe_combine", y, "y");
  TORCH_CHECK(out.dim() == 2 && wts.dim() == 2, "moe_combine: out [T, d], wts [T, topk]");
  const int T = out.size(0), d = out.size(1), topk = wts.size(1);
  TORCH_CHECK(d % 8 == 0, "moe_combine: d % 8");
  akap::launch_moe_combine(a.bf16(y, "y"), a.ptr<float>(wts, "wts", (int64_t)T * topk),
                           a.ptr<int32_t>(inv, "inv", (int64_t)T * topk), a.bf16(out, "out"), T,
                           topk, d, cur_stream());
}

// cache: [planes, NB, ...block...]; out / buf: [planes, nblk, block].  The blocks move as raw
// 16-byte vectors, so no dtype is asked of either.
void kv_gather(Tensor cache, Tensor block_ids, Tensor out) {
  const OpArgs a = on_gpu("kv_gather", cache, "cache");
  const int planes = cache.size(0), nblk = block_ids.numel();
  const int block_elems = cache.stride(1);
  TORCH_CHECK(block_elems % 8 == 0, "kv_gather: a block must be a multiple of 16 bytes");
  akap::launch_kv_gather(a.ptr(cache, "cache", {cache.scalar_type()}), cache.stride(0), planes,
                         block_elems, cache.size(1), a.ptr<int>(block_ids, "block_ids"), nblk,
                         a.ptr(out, "out", {out.scalar_type()},
                               (int64_t)planes * nblk * block_elems),
                         cur_stream());
}

void kv_scatter(Tensor buf, Tensor cache, Tensor block_ids) {
  const OpArgs a = on_gpu("kv_scatter", cache, "cache");
  const int planes = cache.size(0), nblk = block_ids.numel();
  akap::launch_kv_scatter(a.ptr(buf, "buf", {buf.scalar_type()},
                                (int64_t)planes * nblk * cache.stride(1)),
                          a.ptr(cache, "cache", {cache.scalar_type()}), cache.stride(0), planes,
                          cache.stride(1), cache.size(1), a.ptr<int>(block_ids, "block_ids"),
                          nblk, cur_stream());
}

// hipIpc KV pull (see kv_transfer.hip).  src_planes / dst_planes: int64 device tables of
// per-plane base addresses (a peer's planes as mapped by ipc_open -- or this engine's own for a
// tail-only fill -- and this engine's planes); every plane is [NB, block_elems] bf16 (an fp8
// cache moves as bf16 pairs).  Index ranges are validated by the caller
// (ops.kv_pull) before upload: the kernel trusts pairs / tail_jobs.
void kv_pull(Tensor src_planes, Tensor dst_planes, int64_t block_elems, Tensor pairs,
             std::optional<Tensor> tail, std::optional<Tensor> tail_jobs, int64_t Hkv,
             int64_t BS, int64_t D) {
  const OpArgs o = on_gpu("kv_pull", dst_planes, "dst_planes");
  TORCH_CHECK(src_planes.numel() == dst_planes.numel() && src_planes.numel() % 2 == 0,
              "kv_pull: plane tables int64 [2L], same length");
  TORCH_CHECK(pairs.numel() % 2 == 0, "kv_pull: pairs [n, 2]");
  akap::KVPullArgs a{};
  a.src_planes = o.ptr<int64_t>(src_planes, "src_planes");
  a.dst_planes = o.ptr<int64_t>(dst_planes, "dst_planes");
  a.planes = src_planes.numel();
  a.block_elems = (int)block_elems;
  // bf16 cache: block = Hkv*BS*D; an fp8 (byte) cache is moved as bf16 pairs, block =
  // Hkv*BS*D/2 -- the copy jobs are dtype-agnostic 16-byte moves; V tails exist only for bf16
  const bool byte_cache = (int64_t)a.block_elems * 2 == Hkv * BS * D;
  TORCH_CHECK(a.block_elems % 8 == 0 && (a.block_elems == Hkv * BS * D || byte_cache),
              "block = Hkv*BS*D (bf16) or Hkv*BS*D/2 (fp8 bytes viewed as bf16)");
  a.pairs = o.ptr<int>(pairs, "pairs");
  a.nblk = pairs.numel() / 2;
  a.Hkv = Hkv; a.BS = BS; a.D = D;
  a.layers = a.planes / 2;
  if (tail && tail_jobs && tail_jobs->numel()) {
    TORCH_CHECK(!byte_cache, "kv_pull: V-tail jobs need a bf16 cache");
    TORCH_CHECK(tail->dim() == 5 && tail->size(0) == a.layers && tail->size(2) == Hkv &&
                tail->size(3) == 8 && tail->size(4) == D, "kv_pull: tail [L, slots, Hkv, 8, D]");
    TORCH_CHECK(tail_jobs->numel() % 4 == 0, "kv_pull: tail_jobs [m, 4]");
    TORCH_CHECK(BS % 8 == 0, "kv_pull: block size % 8");
    a.tail = reinterpret_cast<__bf16*>(o.bf16(*tail, "tail"));
    a.tail_slots = tail->size(1);
    a.tail_jobs = o.ptr<int>(*tail_jobs, "tail_jobs");
    a.ntail = tail_jobs->numel() / 4;
  }
  akap::launch_kv_pull(a, cur_stream());
}

// Prefill / large-M GEMM (pgemm.hip): out = x . w^T (epi 0) or silu(gate) * up over the
// [gate; up] halves of w (epi 2, out [M, N/2]).  offs (int32 [G], device) -> expert-grouped:
// rows of x sorted by group, w [G, N, K].
void pgemm(Tensor out, Tensor x, Tensor w, int64_t epi, std::optional<Tensor> offs) {
  const OpArgs o = on_gpu("pgemm", x, "x");
  TORCH_CHECK(x.dim() == 2 && out.dim() == 2, "pgemm: x, out must be 2-D");
  TORCH_CHECK(epi == akap::EPI_STORE || epi == akap::EPI_SILU, "pgemm: epilogue store | silu");
  akap::PGemmArgs a{};
  a.M = x.size(0);
  a.K = x.size(1);
  a.N = w.size(-2);
  TORCH_CHECK(w.size(-1) == a.K, "pgemm: w [.., N, K] must match x [M, K]");
  TORCH_CHECK(akap::pgemm_supported(a.M, a.N, a.K, x.stride(0)),
              "pgemm: N % 256 == 0 and K % 64 == 0 needed, X and each weight matrix below 2 GiB");
  TORCH_CHECK(out.size(0) == a.M && out.size(1) == (epi == akap::EPI_SILU ? a.N / 2 : a.N),
              "pgemm: out shape");
  // grouped: w [G, N, K] with offs int32 [G]; dense: w [N, K]
  TORCH_CHECK(w.dim() == (offs ? 3 : 2) && (!offs || offs->numel() == w.size(0)),
              "pgemm: w [N, K], or w [G, N, K] with offs [G]");
  a.offs = o.ptr<int>(offs, "offs");
  a.groups = offs ? offs->numel() : 0;
  a.X = o.bf16(x, "x", 0, kLastContig);
  a.W = o.bf16(w, "w");
  a.Y = o.bf16(out, "out", 0, kLastContig);
  a.ldx = x.stride(0);
  a.ldy = out.stride(0);
  TORCH_CHECK(a.ldx % 8 == 0 && a.ldy % 4 == 0,
              "pgemm: row strides must keep 16-B / 8-B alignment");
  akap::launch_pgemm(a, (int)epi, cur_stream());
}

// dst (device) <- src (pinned host) by a kernel that reads the device mapping of the host
// buffer (no hipMemcpyAsync): the caller keeps src untouched until the stream passes it
void h2d_stage(Tensor dst, Tensor src) {
  const OpArgs a = on_gpu("h2d_stage", dst, "dst");
  TORCH_CHECK(src.defined() && !src.is_cuda() && src.is_pinned() && src.is_contiguous(),
              "h2d_stage: src must be contiguous pinned host memory");
  TORCH_CHECK(src.nbytes() == dst.nbytes(), "h2d_stage: size mismatch");
  void* dev_src = nullptr;
  TORCH_CHECK(hipHostGetDevicePointer(&dev_src, src.data_ptr(), 0) == hipSuccess,
              "h2d_stage: the pinned buffer has no device mapping");
  akap::launch_h2d_stage(dev_src, a.ptr(dst, "dst", {dst.scalar_type()}), (long)dst.nbytes(),
                         cur_stream());
}

void embedding(Tensor ids, Tensor table, Tensor out, int64_t vocab_start, int64_t vocab_end) {
  const OpArgs a = on_gpu("embedding", ids, "ids");
  TORCH_CHECK(table.dim() == 2 && table.size(1) % 8 == 0,
              "embedding: table [V, d] with d a multiple of 8");
  const int T = ids.numel(), d = table.size(1);
  akap::launch_embedding(a.ptr<int64_t>(ids, "ids"), a.bf16(table, "table"),
                         a.bf16(out, "out", (int64_t)T * d), T, d, vocab_start, vocab_end,
                         cur_stream());
}

void embedding_prep(Tensor ids, Tensor table, Tensor ln, Tensor residual, Tensor a_out,
                    Tensor ss_out, Tensor zbuf, int64_t vocab_start, int64_t vocab_end) {
  const OpArgs a = on_gpu("embedding_prep", ids, "ids");
  TORCH_CHECK(table.dim() == 2, "embedding_prep: table [V, d]");
  const int T = ids.numel(), d = table.size(1);
  TORCH_CHECK(d % 8 == 0 && ln.numel() == d,
              "embedding_prep: embedding dim multiple of 8, ln of length d");
  TORCH_CHECK(residual.numel() == (int64_t)T * d && a_out.numel() == (int64_t)T * d,
              "embedding_prep: residual / a_out [T, d]");
  akap::launch_embedding_prep(a.ptr<int64_t>(ids, "ids"), a.bf16(table, "table"),
                              a.bf16(ln, "ln"), a.bf16(residual, "residual"),
                              a.bf16(a_out, "a_out"), a.ptr<float>(ss_out, "ss_out", T),
                              a.ptr<float>(zbuf, "zbuf"), zbuf.numel(), T, d, vocab_start,
                              vocab_end, cur_stream());
}

}  // namespace


// ---------------------------------------------------------------- custom all-reduce (K13)
// Per-communicator state lives here (C++), indexed by a small integer handle that the
// Python wrapper (parallel/custom_allreduce.py) keeps.  IPC handles are exchanged by the
// caller over torch.distributed.
namespace {
struct CarComm {
  int device = 0;
  akap::CarArgs args{};
  void* buf = nullptr;
  void* sig = nullptr;
  std::vector<void*> opened;
};
std::vector<CarComm*>& car_table() {
  static std::vector<CarComm*> t;
  return t;
}
CarComm* car_get(int64_t h) {
  auto& t = car_table();
  TORCH_CHECK(h >= 0 && h < (int64_t)t.size() && t[h] != nullptr, "bad custom all-reduce handle");
  return t[h];
}
#define HIP_OK(x)                                                                     \
  do {                                                                                \
    hipError_t e_ = (x);                                                              \
    TORCH_CHECK(e_ == hipSuccess, #x " failed: ", hipGetErrorString(e_));             \
  } while (0)
}  // namespace

int64_t car_create(int64_t device, int64_t rank, int64_t world, int64_t max_elems,
                   int64_t blocks) {
  TORCH_CHECK(world >= 1 && world <= 8 && rank >= 0 && rank < world, "world must be 1..8");
  TORCH_CHECK(blocks >= 1 && blocks <= 128, "car blocks must be 1..128");
  TORCH_CHECK(max_elems % 8 == 0, "max_elems % 8");
  const c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (int)device));
  auto* c = new CarComm();
  c->device = (int)device;
  const size_t buf_bytes = (size_t)4 * max_elems * sizeof(uint16_t);
  const size_t sig_bytes = akap::custom_allreduce_signal_bytes();
  HIP_OK(hipExtMallocWithFlags(&c->buf, buf_bytes, hipDeviceMallocUncached));
  HIP_OK(hipExtMallocWithFlags(&c->sig, sig_bytes, hipDeviceMallocUncached));
  HIP_OK(hipMemset(c->sig, 0, sig_bytes));
  void* local = nullptr;
  HIP_OK(hipMalloc(&local, 4096));
  HIP_OK(hipMemset(local, 0, 4096));
  HIP_OK(hipDeviceSynchronize());
  c->args.counter = reinterpret_cast<uint32_t*>(local);
  c->args.err = reinterpret_cast<uint32_t*>(local) + 1023;
  c->args.rank = (int)rank;
  c->args.world = (int)world;
  c->args.half_elems = (size_t)max_elems;
  c->args.blocks = (int)blocks;
  for (int p = 0; p < 8; ++p) { c->args.bufs[p] = nullptr; c->args.sigs[p] = nullptr; }
  c->args.bufs[rank] = reinterpret_cast<__bf16*>(c->buf);
  c->args.sigs[rank] = reinterpret_cast<uint32_t*>(c->sig);
  car_table().push_back(c);
  return (int64_t)car_table().size() - 1;
}

Tensor car_ipc_handles(int64_t h) {
  CarComm* c = car_get(h);
  const c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, c->device));
  auto out = at::empty({2, (int64_t)sizeof(hipIpcMemHandle_t)}, at::kByte);
  hipIpcMemHandle_t hb, hs;
  HIP_OK(hipIpcGetMemHandle(&hb, c->buf));
  HIP_OK(hipIpcGetMemHandle(&hs, c->sig));
  std::memcpy(out.data_ptr<uint8_t>(), &hb, sizeof(hb));
  std::memcpy(out.data_ptr<uint8_t>() + sizeof(hb), &hs, sizeof(hs));
  return out;
}

void car_open(int64_t h, Tensor all_handles) {
  CarComm* c = car_get(h);
  TORCH_CHECK(all_handles.device().is_cpu() && all_handles.scalar_type() == at::kByte, "cpu uint8");
  TORCH_CHECK(all_handles.size(0) == c->args.world, "one handle pair per rank");
  const c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, c->device));
  auto hc = all_handles.contiguous();
  const uint8_t* base = hc.data_ptr<uint8_t>();
  const size_t hs = sizeof(hipIpcMemHandle_t);
  for (int p = 0; p < c->args.world; ++p) {
    if (p == c->args.rank) continue;
    hipIpcMemHandle_t hb, hg;
    std::memcpy(&hb, base + (size_t)p * 2 * hs, hs);
    std::memcpy(&hg, base + (size_t)p * 2 * hs + hs, hs);
    void* pb = nullptr;
    void* pg = nullptr;
    HIP_OK(hipIpcOpenMemHandle(&pb, hb, hipIpcMemLazyEnablePeerAccess));
    HIP_OK(hipIpcOpenMemHandle(&pg, hg, hipIpcMemLazyEnablePeerAccess));
    c->opened.push_back(pb);
    c->opened.push_back(pg);
    c->args.bufs[p] = reinterpret_cast<__bf16*>(pb);
    c->args.sigs[p] = reinterpret_cast<uint32_t*>(pg);
  }
}

// The collectives' user tensors: contiguous, and 16-byte aligned (the IPC kernels move bf16x8
// vectors on them)
constexpr unsigned kCarVec = akap::kContig | akap::kAlign16;

// every peer's buffers are mapped and the message fits one staging half
static void car_check_ready(const CarComm* c, size_t elems) {
  TORCH_CHECK(elems <= c->args.half_elems, "message larger than the buffer");
  for (int p = 0; p < c->args.world; ++p)
    TORCH_CHECK(c->args.bufs[p] != nullptr, "peer buffers not opened (call car_open)");
}

void car_all_reduce(int64_t h, Tensor inp, Tensor out, bool two_shot) {
  CarComm* c = car_get(h);
  const OpArgs a = on_gpu("car_all_reduce", inp, "inp");
  TORCH_CHECK(inp.numel() == out.numel(), "car_all_reduce: size mismatch");
  TORCH_CHECK(inp.numel() % 8 == 0, "car_all_reduce: numel % 8");
  car_check_ready(c, inp.numel());
  akap::launch_custom_allreduce(c->args, a.bf16(inp, "inp", 0, kCarVec),
                                a.bf16(out, "out", inp.numel(), kCarVec), inp.numel(),
                                two_shot ? 1 : 0, cur_stream());
}

static akap::CarEpi car_epi_of(const OpArgs& a, Tensor& residual, Tensor& ln, Tensor& aout,
                               Tensor& ss, int64_t n) {
  const int64_t d = ln.numel();
  TORCH_CHECK(d > 0 && d % 512 == 0, a.op(), ": resnorm row width must be a multiple of 512");
  TORCH_CHECK(residual.numel() == n && aout.numel() == n && n % d == 0, a.op(),
              ": resnorm residual / aout [M, d] like the message");
  akap::CarEpi e{};
  e.residual = (__bf16*)a.bf16(residual, "residual", 0, kCarVec);
  e.ln = (const __bf16*)a.bf16(ln, "ln", 0, kCarVec);
  e.aout = (__bf16*)a.bf16(aout, "aout", 0, kCarVec);
  e.ss = a.ptr<float>(ss, "ss", n / d);
  e.d = (int)d;
  return e;
}

// All-reduce of row-parallel partial sums fused with the decode chain's residual add and the
// elementwise half of the next RMSNorm (see CarEpi): residual += sum; aout = residual * ln;
// ss += row sums of residual^2.  `inp` is consumed (staged), nothing else is written.
void car_all_reduce_resnorm(int64_t h, Tensor inp, Tensor residual, Tensor ln, Tensor aout,
                            Tensor ss, bool two_shot) {
  CarComm* c = car_get(h);
  const OpArgs a = on_gpu("car_all_reduce_resnorm", inp, "inp");
  car_check_ready(c, inp.numel());
  const akap::CarEpi e = car_epi_of(a, residual, ln, aout, ss, inp.numel());
  akap::launch_custom_allreduce(c->args, a.bf16(inp, "inp", 0, kCarVec), nullptr, inp.numel(),
                                two_shot ? 1 : 0, cur_stream(), &e);
}

// Test hook: wire communicators created in THIS process (one per simulated rank, all on
// one GPU) to each other without IPC, so the kernel protocol can be exercised on 1 GPU.
void car_link_local(int64_t h, std::vector<int64_t> peers) {
  CarComm* c = car_get(h);
  TORCH_CHECK((int)peers.size() == c->args.world, "one handle per rank");
  for (int p = 0; p < c->args.world; ++p) {
    CarComm* o = car_get(peers[p]);
    c->args.bufs[p] = reinterpret_cast<__bf16*>(o->buf);
    c->args.sigs[p] = reinterpret_cast<uint32_t*>(o->sig);
  }
}

// Test hook: run the all-reduce of every simulated rank (communicators linked with
// car_link_local) in ONE grid, blockIdx.y = rank, so all ranks are co-resident regardless
// of how streams map to hardware queues.
void car_all_reduce_multi(std::vector<int64_t> hs, std::vector<Tensor> ins,
                          std::vector<Tensor> outs, bool two_shot,
                          std::optional<std::vector<Tensor>> epi, bool warm) {
  const int W = hs.size();
  TORCH_CHECK(W >= 1 && W <= 8 && (int)ins.size() == W && (int)outs.size() == W, "W ranks");
  akap::CarMulti m{};
  m.warm = warm ? 1 : 0;
  const OpArgs a = on_gpu("car_all_reduce_multi", ins[0], "ins[0]");
  const int64_t n = ins[0].numel();
  for (int r = 0; r < W; ++r) {
    CarComm* c = car_get(hs[r]);
    TORCH_CHECK(c->args.world == W && c->args.rank == r, "handles must be ranks 0..W-1");
    TORCH_CHECK(ins[r].numel() == n && outs[r].numel() == n && n % 8 == 0, "sizes");
    TORCH_CHECK((size_t)n <= c->args.half_elems, "message larger than the buffer");
    m.args[r] = c->args;
    m.in[r] = a.bf16(ins[r], "ins[r]");
    m.out[r] = a.bf16(outs[r], "outs[r]");
    if (epi) {  // 4 tensors per rank: residual, ln, aout, ss
      TORCH_CHECK((int)epi->size() == 4 * W, "epi: residual, ln, aout, ss per rank");
      m.epi[r] = car_epi_of(a, (*epi)[4 * r], (*epi)[4 * r + 1], (*epi)[4 * r + 2],
                            (*epi)[4 * r + 3], n);
      m.use_epi = 1;
    }
  }
  akap::launch_custom_allreduce_multi(m, W, n, two_shot ? 1 : 0, cur_stream());
}

int64_t car_error(int64_t h) {
  CarComm* c = car_get(h);
  const c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, c->device));
  uint32_t v = 0;
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(&v, c->args.err, sizeof(v), hipMemcpyDeviceToHost));
  return (int64_t)v;
}

// The communicator's device error word as a 1-element int32 tensor (no copy): a replayed
// decode graph enqueues an async copy of it to pinned host memory after its last collective,
// and the host checks it before the step's tokens are emitted (ModelRunner._err_probe).
Tensor car_error_word(int64_t h) {
  CarComm* c = car_get(h);
  return at::from_blob(c->args.err, {1},
                       at::TensorOptions().dtype(at::kInt).device(
                           c10::Device(c10::DeviceType::CUDA, c->device)));
}

// Rank-major all-gather of the vocab-parallel logits shard inp [R, n] -> out [R, W*n].
void car_all_gather(int64_t h, Tensor inp, Tensor out) {
  CarComm* c = car_get(h);
  const OpArgs a = on_gpu("car_all_gather", inp, "inp");
  const int64_t n = inp.size(-1);
  const int64_t rows = inp.numel() / n;
  TORCH_CHECK(n % 8 == 0, "car_all_gather: shard width % 8");
  TORCH_CHECK(out.numel() == inp.numel() * c->args.world, "car_all_gather: out [R, W*n]");
  car_check_ready(c, inp.numel());
  akap::launch_custom_allgather(c->args, a.bf16(inp, "inp", 0, kCarVec),
                                a.bf16(out, "out", 0, kCarVec), rows, (int)n, cur_stream());
}

// Equal-segment all-to-all: inp/out [world * seg] bf16, segment d of inp goes to rank d and
// segment p of out comes from rank p.
void car_all_to_all(int64_t h, Tensor inp, Tensor out) {
  CarComm* c = car_get(h);
  const OpArgs a = on_gpu("car_all_to_all", inp, "inp");
  const int64_t W = c->args.world;
  TORCH_CHECK(inp.numel() == out.numel() && inp.numel() % (W * 8) == 0,
              "car_all_to_all: inp/out [world * seg] with seg % 8 == 0");
  car_check_ready(c, inp.numel());
  const void* src = a.bf16(inp, "inp", 0, kCarVec);
  void* dst = a.bf16(out, "out", 0, kCarVec);
  TORCH_CHECK(src != dst, "car_all_to_all: out of place only");
  akap::launch_custom_alltoall(c->args, src, dst, inp.numel() / W, cur_stream());
}

// In-place broadcast of buf (any dtype, nbytes % 16 == 0) from group rank `root`.
void car_broadcast(int64_t h, Tensor buf, int64_t root) {
  CarComm* c = car_get(h);
  const OpArgs a = on_gpu("car_broadcast", buf, "buf");
  const int64_t bytes = buf.numel() * buf.element_size();
  TORCH_CHECK(bytes % 16 == 0, "car_broadcast: bytes % 16");
  TORCH_CHECK(root >= 0 && root < c->args.world, "car_broadcast: root rank");
  car_check_ready(c, (size_t)(bytes + 1) / 2);
  akap::launch_custom_broadcast(c->args, a.ptr(buf, "buf", {buf.scalar_type()}, 0, kCarVec),
                                bytes, (int)root, cur_stream());
}

// ---------------------------------------------------------------- hipIpc of a whole tensor
// (the P/D KV pull): export -> [handle | offset of data_ptr in its allocation | bytes]
namespace {
std::vector<std::pair<int64_t, void*>>& ipc_opened() {
  static std::vector<std::pair<int64_t, void*>> t;
  return t;
}
}  // namespace

Tensor ipc_export(Tensor t) {
  TORCH_CHECK(t.defined() && t.is_cuda(), "ipc_export: t must be a GPU tensor");
  const c10::DeviceGuard g(t.device());
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  HIP_OK(hipMemGetAddressRange(&base, &size, t.data_ptr()));
  // ROCm 7.0.x runtimes (the one PyTorch bundles) hang in the PEER's hipIpcOpenMemHandle when
  // bit 31 of the allocation size is set (size mod 4 GiB >= 2 GiB; 7.2 maps them):
  // bench/ipc_import_repro.cpp, profiles/r6_ipc_import_sweep.md.  Refuse here instead of
  // letting the importer hang; KV segments are sized by models.transformer.ipc_safe_alloc_bytes
  int rt = 0;
  HIP_OK(hipRuntimeGetVersion(&rt));
  TORCH_CHECK(rt >= 70200000 || (size & (size_t(1) << 31)) == 0,
              "ipc_export: allocation of ", size, " bytes has bit 31 set; a peer's "
              "hipIpcOpenMemHandle of it hangs on this HIP runtime (", rt,
              "): pad it to a multiple of 4 GiB (ipc_safe_alloc_bytes)");
  hipIpcMemHandle_t hd;
  HIP_OK(hipIpcGetMemHandle(&hd, base));
  const int64_t off = (int64_t)((char*)t.data_ptr() - (char*)base);
  const int64_t nbytes = t.numel() * t.element_size();
  TORCH_CHECK(off >= 0 && (size_t)(off + nbytes) <= size, "tensor outside its allocation");
  auto out = at::empty({(int64_t)sizeof(hd) + 16}, at::kByte);
  std::memcpy(out.data_ptr<uint8_t>(), &hd, sizeof(hd));
  std::memcpy(out.data_ptr<uint8_t>() + sizeof(hd), &off, 8);
  std::memcpy(out.data_ptr<uint8_t>() + sizeof(hd) + 8, &nbytes, 8);
  return out;
}

// Map a peer's exported tensor; returns its device address (valid on `device` until
// ipc_close).  The same GPU (two processes) or a peer GPU over xGMI.
int64_t ipc_open(Tensor blob, int64_t device) {
  TORCH_CHECK(blob.device().is_cpu() && blob.scalar_type() == at::kByte &&
              blob.numel() == (int64_t)sizeof(hipIpcMemHandle_t) + 16, "ipc_export blob");
  const c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, (int)device));
  auto b = blob.contiguous();
  hipIpcMemHandle_t hd;
  int64_t off = 0;
  std::memcpy(&hd, b.data_ptr<uint8_t>(), sizeof(hd));
  std::memcpy(&off, b.data_ptr<uint8_t>() + sizeof(hd), 8);
  void* p = nullptr;
  HIP_OK(hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess));
  const int64_t addr = (int64_t)((char*)p + off);
  ipc_opened().emplace_back(addr, p);
  return addr;
}

void ipc_close(int64_t addr) {
  auto& t = ipc_opened();
  for (size_t i = 0; i < t.size(); ++i)
    if (t[i].first == addr) {
      (void)hipIpcCloseMemHandle(t[i].second);
      t.erase(t.begin() + i);
      return;
    }
}

void car_destroy(int64_t h) {
  CarComm* c = car_get(h);
  const c10::DeviceGuard g(c10::Device(c10::DeviceType::CUDA, c->device));
  (void)hipDeviceSynchronize();
  for (void* p : c->opened) (void)hipIpcCloseMemHandle(p);
  (void)hipFree(c->buf);
  (void)hipFree(c->sig);
  (void)hipFree(c->args.counter);
  delete c;
  car_table()[h] = nullptr;
}

TORCH_LIBRARY(akap, m) {
  m.def("rmsnorm(Tensor(a!) out, Tensor x, Tensor w, float eps) -> ()");
  m.def("fused_add_rmsnorm(Tensor(a!) out, Tensor(b!) residual, Tensor x, Tensor w, float eps) -> ()");
  m.def(
      "qk_norm_rope_cache(Tensor qkv, Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, "
      "Tensor positions, Tensor slots, Tensor cos_sin, Tensor? q_w, Tensor? k_w, int Hq, int Hkv, "
      "float eps, bool apply_rope, bool decode=False, Tensor(d!)? v_tail=None, "
      "Tensor? tail_slot=None, int num_decode=0, int q_rows=-1) -> ()");
  m.def("reshape_and_cache(Tensor k, Tensor v, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor slots) -> ()");
  m.def("silu_and_mul(Tensor(a!) out, Tensor x) -> ()");
  m.def(
      "paged_attention_prefill(Tensor(a!) out, Tensor q, Tensor k_cache, Tensor v_cache, "
      "Tensor block_tables, Tensor seq_lens, Tensor q_start, Tensor tile_seq, Tensor tile_row, "
      "int G, float scale, int tile_rows=128) -> ()");
  m.def(
      "paged_attention_prefill_qprep(Tensor(a!) out, Tensor qkv, Tensor k_cache, Tensor v_cache, "
      "Tensor block_tables, Tensor seq_lens, Tensor q_start, Tensor tile_seq, Tensor tile_row, "
      "Tensor positions, Tensor cos_sin, Tensor? q_w, int G, float scale, float eps, "
      "int tile_rows=128) -> ()");
  m.def(
      "paged_attention_decode(Tensor(a!) out, Tensor q, Tensor k_cache, Tensor v_cache, "
      "Tensor block_tables, Tensor seq_lens, Tensor? q_start, Tensor(b!) part_m, Tensor(c!) part_l, "
      "Tensor(d!) part_o, int num_parts, int part_size, int G, float scale, "
      "Tensor? v_tail=None, Tensor? tail_slot=None) -> ()");
  m.def(
      "paged_attention_decode_fused(Tensor(a!) out, Tensor qkv, Tensor(b!) k_cache, "
      "Tensor(c!) v_cache, Tensor block_tables, Tensor seq_lens, Tensor positions, Tensor slots, "
      "Tensor cos_sin, Tensor? q_w, Tensor? k_w, Tensor(d!) part_m, Tensor(e!) part_l, "
      "Tensor(f!) part_o, int num_parts, int part_size, int G, float scale, float eps, "
      "Tensor(g!)? v_tail=None, Tensor? tail_slot=None, bool write_kv=True) -> ()");
  m.def(
      "sample(Tensor logits, Tensor temperature, Tensor top_k, Tensor top_p, Tensor seeds, "
      "Tensor steps, Tensor(a!) out_tokens, Tensor(b!) out_logprobs, "
      "bool greedy_logprobs, Tensor(c!) ws, Tensor(d!) tickets, bool filtered=True) -> ()");
  m.def(
      "apply_penalties(Tensor(a!) logits, Tensor rows, Tensor toks, Tensor counts, "
      "Tensor presence, Tensor frequency, Tensor repetition) -> ()");
  m.def("argmax(Tensor logits, Tensor(a!) out) -> ()");
  m.def(
      "gemm(Tensor(a!) out, Tensor x, Tensor w, Tensor(b!) ws, int splitk, "
      "Tensor(c!)? counters=None) -> ()");
  m.def("gemm_splitk(int M, int N, int K) -> int");
  m.def(
      "dgemm(Tensor(a!) out, Tensor x, Tensor w, Tensor(b!) ws, int pro, int splitk, int pf, "
      "Tensor? r=None, Tensor(c!)? rout=None, Tensor? ln=None, float eps=1e-6, int epi=0, "
      "Tensor? ss_in=None, Tensor(d!)? ss_out=None, Tensor(e!)? aout=None, "
      "Tensor? ln_out=None, int bn=0, int ns=0, Tensor(f!)? counters=None, int bm=64, "
      "Tensor[]? kv_write=None, int kv_hq=0, int kv_blocks=0, float kv_eps=1e-6) -> ()");
  m.def("wgemm(Tensor(a!) out, Tensor x, Tensor w) -> ()");
  m.def("qgemm(Tensor(a!) out, Tensor x, Tensor wq, Tensor scale) -> ()");
  m.def("dequant_fp8(Tensor(a!) out, Tensor wq, Tensor scale) -> ()");
  m.def("q4gemm(Tensor(a!) out, Tensor x, Tensor wq, Tensor scale) -> ()");
  m.def("dequant_mxfp4(Tensor(a!) out, Tensor wq, Tensor scale) -> ()");
  m.def("pgemm(Tensor(a!) out, Tensor x, Tensor w, int epi=0, Tensor? offs=None) -> ()");
  m.def("kgemm(Tensor(a!) out, Tensor x, Tensor w, int bm, int epi, float eps, Tensor? ss_in, "
        "Tensor(b!)? ss_out, Tensor(c!)? aout, Tensor? ln_out) -> ()");
  m.def("l2_prefetch(Tensor[] ts, Tensor(a!) sink) -> ()");
  m.def("car_create(int device, int rank, int world, int max_elems, int blocks=128) -> int");
  m.def("car_ipc_handles(int h) -> Tensor");
  m.def("car_open(int h, Tensor handles) -> ()");
  m.def("car_all_reduce(int h, Tensor inp, Tensor(a!) out, bool two_shot) -> ()");
  m.def("car_error(int h) -> int");
  m.def("car_error_word(int h) -> Tensor");
  m.def("car_link_local(int h, int[] peers) -> ()");
  m.def("car_all_reduce_multi(int[] hs, Tensor[] ins, Tensor(a!)[] outs, bool two_shot, "
        "Tensor(b!)[]? epi=None, bool warm=False) -> ()");
  m.def("car_all_reduce_resnorm(int h, Tensor inp, Tensor(a!) residual, Tensor ln, "
        "Tensor(b!) aout, Tensor(c!) ss, bool two_shot) -> ()");
  m.def("car_destroy(int h) -> ()");
  m.def("car_all_gather(int h, Tensor inp, Tensor(a!) out) -> ()");
  m.def("car_broadcast(int h, Tensor(a!) buf, int root) -> ()");
  m.def("car_all_to_all(int h, Tensor inp, Tensor(a!) out) -> ()");
  m.def("h2d_stage(Tensor(a!) dst, Tensor src) -> ()");
  m.def("ipc_export(Tensor t) -> Tensor");
  m.def("ipc_open(Tensor blob, int device) -> int");
  m.def("ipc_close(int addr) -> ()");
  m.def(
      "kv_pull(Tensor src_planes, Tensor dst_planes, int block_elems, Tensor pairs, "
      "Tensor(a!)? tail, Tensor? tail_jobs, int Hkv, int BS, int D) -> ()");
  m.def("moe_topk_softmax(Tensor logits, Tensor(a!) topk_w, Tensor(b!) topk_ids, bool renorm) -> ()");
  m.def("moe_router_topk(Tensor h, Tensor router, Tensor(a!) topk_w, Tensor(b!) topk_ids, bool renorm) -> ()");
  m.def(
      "moe_align(Tensor topk_ids, int E, int block, Tensor(a!) sorted_ids, Tensor(b!) offsets, "
      "Tensor(c!) num_padded, Tensor(d!) inv, Tensor(e!) tile_expert) -> ()");
  m.def(
      "moe_gemm(Tensor(a!) out, Tensor a, Tensor w, Tensor sorted_ids, Tensor tile_expert, "
      "int n_flat, int topk, bool gather) -> ()");
  m.def("moe_combine(Tensor y, Tensor wts, Tensor inv, Tensor(a!) out) -> ()");
  m.def(
      "moe_dgemm(Tensor(a!) out, Tensor a, Tensor w, Tensor sorted_ids, Tensor tile_expert, "
      "int n_flat, int topk, bool gather, bool silu, int pf, int bm=32, int splitk=1) -> ()");
  m.def(
      "moe_qgemm(Tensor(a!) out, Tensor a, Tensor wq, Tensor scale, Tensor sorted_ids, "
      "Tensor tile_expert, int n_flat, int topk, bool gather, bool silu, int pf, int bm=32, "
      "int splitk=1) -> ()");
  m.def(
      "moe_q4gemm(Tensor(a!) out, Tensor a, Tensor wq, Tensor scale, Tensor sorted_ids, "
      "Tensor tile_expert, int n_flat, int topk, bool gather, bool silu, int pf, int bm=32, "
      "int splitk=1) -> ()");
  m.def(
      "moe_combine_split(Tensor partials, Tensor wts, Tensor inv, Tensor(a!) out, int splitk, "
      "int rows) -> ()");
  m.def("kv_gather(Tensor cache, Tensor block_ids, Tensor(a!) out) -> ()");
  m.def("kv_scatter(Tensor buf, Tensor(a!) cache, Tensor block_ids) -> ()");
  m.def("embedding(Tensor ids, Tensor table, Tensor(a!) out, int vocab_start, int vocab_end) -> ()");
  m.def("embedding_prep(Tensor ids, Tensor table, Tensor ln, Tensor(a!) residual, "
        "Tensor(b!) a_out, Tensor(c!) ss_out, Tensor(d!) zbuf, int vocab_start, "
        "int vocab_end) -> ()");
}

TORCH_LIBRARY_IMPL(akap, CompositeExplicitAutograd, m) {
  m.impl("gemm_splitk", &gemm_splitk);
  m.impl("car_create", &car_create);
  m.impl("car_ipc_handles", &car_ipc_handles);
  m.impl("car_open", &car_open);
  m.impl("car_error", &car_error);
  m.impl("car_error_word", &car_error_word);
  m.impl("car_link_local", &car_link_local);
  m.impl("car_destroy", &car_destroy);
  m.impl("ipc_open", &ipc_open);
  m.impl("ipc_close", &ipc_close);
  m.impl("h2d_stage", &h2d_stage);  // pinned CPU source + device destination
}

TORCH_LIBRARY_IMPL(akap, CUDA, m) {
  m.impl("rmsnorm", &rmsnorm);
  m.impl("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.impl("qk_norm_rope_cache", &qk_norm_rope_cache);
  m.impl("reshape_and_cache", &reshape_and_cache);
  m.impl("silu_and_mul", &silu_and_mul);
  m.impl("paged_attention_prefill", &paged_attention_prefill);
  m.impl("paged_attention_prefill_qprep", &paged_attention_prefill_qprep);
  m.impl("paged_attention_decode", &paged_attention_decode);
  m.impl("paged_attention_decode_fused", &paged_attention_decode_fused);
  m.impl("sample", &sample);
  m.impl("apply_penalties", &apply_penalties);
  m.impl("argmax", &argmax);
  m.impl("gemm", &gemm);
  m.impl("dgemm", &dgemm);
  m.impl("wgemm", &wgemm);
  m.impl("qgemm", &qgemm);
  m.impl("dequant_fp8", &dequant_fp8);
  m.impl("q4gemm", &q4gemm);
  m.impl("dequant_mxfp4", &dequant_mxfp4);
  m.impl("pgemm", &pgemm);
  m.impl("kgemm", &kgemm);
  m.impl("moe_topk_softmax", &moe_topk_softmax);
  m.impl("moe_router_topk", &moe_router_topk);
  m.impl("moe_align", &moe_align);
  m.impl("moe_gemm", &moe_gemm);
  m.impl("moe_combine", &moe_combine);
  m.impl("moe_dgemm", &moe_dgemm);
  m.impl("moe_qgemm", &moe_qgemm);
  m.impl("moe_q4gemm", &moe_q4gemm);
  m.impl("moe_combine_split", &moe_combine_split);
  m.impl("car_all_reduce", &car_all_reduce);
  m.impl("l2_prefetch", &l2_prefetch);
  m.impl("car_all_reduce_multi", &car_all_reduce_multi);
  m.impl("car_all_reduce_resnorm", &car_all_reduce_resnorm);
  m.impl("kv_gather", &kv_gather);
  m.impl("kv_scatter", &kv_scatter);
  m.impl("kv_pull", &kv_pull);
  m.impl("car_all_gather", &car_all_gather);
  m.impl("car_broadcast", &car_broadcast);
  m.impl("car_all_to_all", &car_all_to_all);
  m.impl("ipc_export", &ipc_export);
  m.impl("embedding", &embedding);
  m.impl("embedding_prep", &embedding_prep);
}
