// The one way a tensor of an op becomes a raw pointer for a kernel launch.
//
// An OpArgs is bound to the op's name and its anchor device, and holds the launch's device
// guard.  Every accessor checks that the tensor is defined, on that device, of an allowed
// dtype, laid out as asked and at least `min_numel` long, and only then returns its data
// pointer; a failure is a c10::Error starting "<op>: <name> ".  ATen / c10 only (no HIP
// header): a plain host compiler builds it (tests/cpp/op_args_test.cpp, CPU tensors).
#pragma once

#include <cstdint>
#include <initializer_list>
#include <optional>
#include <string>
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

namespace akap {

// layout flags of an accessor call
enum : unsigned {
  kStrided = 0,     // any strides (the op checks what it needs itself)
  kContig = 1,      // fully contiguous
  kLastContig = 2,  // unit last stride (rows may be strided)
  kAlign16 = 4,     // 16-byte aligned base address
};

class OpArgs {
 public:
  OpArgs(const char* op, c10::Device device) : op_(op), device_(device), guard_(device) {}
  const char* op() const { return op_; }

  // dtype-set form: `t` may have any of `dtypes`
  void* ptr(const at::Tensor& t, const char* name, std::initializer_list<at::ScalarType> dtypes,
            int64_t min_numel = 0, unsigned flags = kContig) const {
    TORCH_CHECK(t.defined(), op_, ": ", name, " is undefined");
    TORCH_CHECK(t.device() == device_, op_, ": ", name, " must be on ", device_, ", is on ",
                t.device());
    bool dtype_ok = false;
    for (at::ScalarType d : dtypes) dtype_ok |= t.scalar_type() == d;
    if (!dtype_ok) {
      std::string want;
      for (at::ScalarType d : dtypes) want += std::string(want.empty() ? "" : " or ") + c10::toString(d);
      TORCH_CHECK(false, op_, ": ", name, " must be ", want, ", is ", t.scalar_type());
    }
    TORCH_CHECK(!(flags & kContig) || t.is_contiguous(), op_, ": ", name, " must be contiguous");
    TORCH_CHECK(!(flags & kLastContig) || (t.dim() >= 1 && t.stride(-1) == 1), op_, ": ", name,
                " must have unit last stride");
    TORCH_CHECK(t.numel() >= min_numel, op_, ": ", name, " too short: ", t.numel(),
                " elements, the launch needs ", min_numel);
    void* p = t.data_ptr();
    TORCH_CHECK(!(flags & kAlign16) || reinterpret_cast<uintptr_t>(p) % 16 == 0, op_, ": ", name,
                " must be 16-byte aligned");
    return p;
  }
  // typed form: the dtype is T's
  template <typename T>
  T* ptr(const at::Tensor& t, const char* name, int64_t min_numel = 0,
         unsigned flags = kContig) const {
    return static_cast<T*>(ptr(t, name, {c10::CppTypeToScalarType<T>::value}, min_numel, flags));
  }
  // bf16 tensors travel as void* (the launchers' headers stay free of device types)
  void* bf16(const at::Tensor& t, const char* name, int64_t min_numel = 0,
             unsigned flags = kContig) const {
    return ptr(t, name, {at::kBFloat16}, min_numel, flags);
  }

  // optional forms: nullptr when the tensor is absent
  template <typename T>
  T* ptr(const std::optional<at::Tensor>& t, const char* name, int64_t min_numel = 0,
         unsigned flags = kContig) const {
    return t ? ptr<T>(*t, name, min_numel, flags) : nullptr;
  }
  void* bf16(const std::optional<at::Tensor>& t, const char* name, int64_t min_numel = 0,
             unsigned flags = kContig) const {
    return t ? bf16(*t, name, min_numel, flags) : nullptr;
  }

  // "empty means absent" form: nullptr for a tensor of no elements
  template <typename T>
  T* ptr_unless_empty(const at::Tensor& t, const char* name, int64_t min_numel = 0,
                      unsigned flags = kContig) const {
    TORCH_CHECK(t.defined(), op_, ": ", name, " is undefined");
    return t.numel() ? ptr<T>(t, name, min_numel, flags) : nullptr;
  }

 private:
  const char* op_;
  c10::Device device_;
  c10::DeviceGuard guard_;
};

}  // namespace akap
