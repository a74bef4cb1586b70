// Stand-alone test of csrc/op_args.h with CPU tensors and the CPU device as the anchor:
// every accessor form on a valid tensor, and every refusal with the op and tensor name in its
// message.  Built and run by tests/test_op_args.py (g++ against torch's own headers).
#include <cstdio>
#include <functional>
#include <optional>
#include <string>

#include "op_args.h"

using akap::OpArgs;
using at::Tensor;

static int failures = 0;

#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

// f must throw a c10::Error whose text starts "<op>: <name> " and mentions `word`
static void expect_refused(const char* what, const std::function<void()>& f,
                           const std::string& prefix, const std::string& word) {
  try {
    f();
  } catch (const c10::Error& e) {
    const std::string msg = e.what_without_backtrace();
    if (msg.rfind(prefix, 0) != 0 || msg.find(word) == std::string::npos) {
      std::printf("FAIL %s: message '%s' (wanted '%s...%s')\n", what, msg.c_str(), prefix.c_str(),
                  word.c_str());
      ++failures;
    }
    return;
  }
  std::printf("FAIL %s: accepted\n", what);
  ++failures;
}

int main() {
  const c10::Device cpu(c10::DeviceType::CPU);
  const OpArgs a("testop", cpu);
  const auto f32 = at::TensorOptions().dtype(at::kFloat);
  const Tensor f = at::zeros({4, 8}, f32);
  const Tensor i32 = at::zeros({6}, f32.dtype(at::kInt));
  const Tensor i64 = at::zeros({6}, f32.dtype(at::kLong));
  const Tensor bf = at::zeros({4, 8}, f32.dtype(at::kBFloat16));
  const Tensor u8 = at::zeros({16}, f32.dtype(at::kByte));
  const Tensor f8 = at::zeros({16}, f32.dtype(at::kFloat8_e4m3fn));

  // every form on a valid tensor returns data_ptr()
  EXPECT(a.ptr<float>(f, "f") == f.data_ptr<float>());
  EXPECT(a.ptr<int>(i32, "i32", 6) == i32.data_ptr<int>());
  EXPECT(a.ptr<int64_t>(i64, "i64", 6) == i64.data_ptr<int64_t>());
  EXPECT(a.bf16(bf, "bf", 32, akap::kContig | akap::kAlign16) == bf.data_ptr());
  EXPECT(a.ptr(f, "f", {at::kFloat, at::kBFloat16}) == f.data_ptr());
  EXPECT(a.ptr<float>(std::optional<Tensor>(f), "f") == f.data_ptr<float>());
  EXPECT(a.ptr_unless_empty<float>(f, "f", 32) == f.data_ptr<float>());
  EXPECT(std::string(a.op()) == "testop");

  // undefined
  expect_refused("undefined", [&] { a.ptr<float>(Tensor(), "t"); }, "testop: t ", "undefined");
  expect_refused("undefined (empty form)", [&] { a.ptr_unless_empty<float>(Tensor(), "t"); },
                 "testop: t ", "undefined");
  // dtype
  expect_refused("dtype", [&] { a.ptr<float>(i32, "temperature"); }, "testop: temperature ",
                 "Float");
  expect_refused("bf16 dtype", [&] { a.bf16(f, "x"); }, "testop: x ", "BFloat16");
  // device: a meta tensor, and a second anchor that the CPU tensor is not on
  const Tensor meta = at::empty({4}, f32.device(c10::DeviceType::Meta));
  expect_refused("meta device", [&] { a.ptr<float>(meta, "seeds"); }, "testop: seeds ", "cpu");
  const OpArgs on_meta("metaop", c10::Device(c10::DeviceType::Meta));
  expect_refused("other anchor", [&] { on_meta.ptr<float>(f, "w"); }, "metaop: w ", "meta");
  // layout
  const Tensor cols = f.slice(1, 0, 4);  // rows strided, unit last stride
  const Tensor tr = f.t();               // non-unit last stride
  expect_refused("non-contiguous", [&] { a.ptr<float>(cols, "cols"); }, "testop: cols ",
                 "contiguous");
  EXPECT(a.ptr<float>(cols, "cols", 16, akap::kLastContig) == cols.data_ptr<float>());
  EXPECT(a.ptr<float>(cols, "cols", 16, akap::kStrided) == cols.data_ptr<float>());
  expect_refused("last stride", [&] { a.ptr<float>(tr, "tr", 0, akap::kLastContig); },
                 "testop: tr ", "unit last stride");
  // length: one short is refused, exactly min_numel is taken
  expect_refused("too short", [&] { a.ptr<int>(i32, "top_k", 7); }, "testop: top_k ", "7");
  EXPECT(a.ptr<int>(i32.slice(0, 0, 5), "top_k", 5) == i32.data_ptr<int>());
  expect_refused("one short", [&] { a.ptr<int>(i32.slice(0, 0, 5), "top_k", 6); },
                 "testop: top_k ", "too short");
  // alignment: a view offset by one element
  const Tensor off1 = bf.view({32}).slice(0, 1, 17);
  EXPECT(a.bf16(off1, "qkv") == off1.data_ptr());
  expect_refused("misaligned", [&] { a.bf16(off1, "qkv", 0, akap::kContig | akap::kAlign16); },
                 "testop: qkv ", "16-byte aligned");
  // optional forms: nullptr when absent, checked when present
  const std::optional<Tensor> none;
  EXPECT(a.ptr<float>(none, "q_start") == nullptr);
  EXPECT(a.bf16(none, "q_w") == nullptr);
  expect_refused("optional dtype", [&] { a.bf16(std::optional<Tensor>(f), "q_w"); },
                 "testop: q_w ", "BFloat16");
  // empty form: nullptr when empty, checked otherwise
  EXPECT(a.ptr_unless_empty<float>(at::zeros({0}, f32), "out_logprobs", 4) == nullptr);
  expect_refused("empty form short",
                 [&] { a.ptr_unless_empty<float>(at::zeros({3}, f32), "out_logprobs", 4); },
                 "testop: out_logprobs ", "too short");
  // dtype-set form: each allowed dtype, and another refused
  EXPECT(a.ptr(u8, "wq", {at::kByte, at::kFloat8_e4m3fn}) == u8.data_ptr());
  EXPECT(a.ptr(f8, "wq", {at::kByte, at::kFloat8_e4m3fn}) == f8.data_ptr());
  expect_refused("dtype set", [&] { a.ptr(i32, "wq", {at::kByte, at::kFloat8_e4m3fn}); },
                 "testop: wq ", "Byte or Float8_e4m3fn");

  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("op_args_test: ok\n");
  return 0;
}
