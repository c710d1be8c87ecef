// Argument checks of the torch bindings (csrc/bindings.cpp), host only. The rule: no pointer reaches a launcher
// without passing one of the helpers below, so data_ptr appears in this file and nowhere in bindings.cpp.
//
//   Op a("op", first, "first");     the call's context: the op's name and the device of its first tensor (a GPU)
//   a.dense<T>(t, "t", n, dims, al) a device array read through a raw pointer: T's dtype, a's device, contiguous,
//                                   numel >= n, optionally dims (exact, ANY or ge(n) each) and al-byte base alignment
//   a.rows<T>(t, "t", r, c)         a 2-D row matrix with unit column stride: pointer and row stride
//   a.dense_opt / a.rows_opt        the same for an optional tensor (c10::optional or numel() == 0): null if absent
//   a.i32(v)                        a tensor-derived size narrowed to int
//   LAUNCH(launch_x(...))           the die::launch_* call and its error check
#pragma once

#include <climits>
#include <cstdint>
#include <initializer_list>
#include <sstream>
#include <type_traits>

#include <torch/extension.h>

#include "kernels/launchers.h"

namespace chk {

using torch::Tensor;

// Check-only mode (_C.check_only): every check runs, nothing is launched, and the first tensor only has to define
// the device. It lets the checks be tested on host tensors; nothing else consults it.
inline bool g_check_only = false;

#define HIP_OK(call)                                                                 \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    TORCH_CHECK(e_ == hipSuccess, "HIP launch failed: ", hipGetErrorString(e_), " (", \
                #call, ")");                                                          \
  } while (0)
#define LAUNCH(call)              \
  do {                            \
    if (chk::g_check_only) break; \
    HIP_OK(die::call);            \
  } while (0)

// The dtype a pointer type stands for. die::bf16_t is uint16_t; the int16 state table that a kernel reads as
// uint16_t is asked for by the tag u16_of_i16, an int32 tensor read as unsigned words by uint32_t, bytes of any
// dtype by void.
struct u16_of_i16 {};
template <class T> struct Elem;
#define CHK_ELEM(T, C, D)                          \
  template <> struct Elem<T> {                     \
    using type = C;                                \
    static constexpr at::ScalarType dtype = at::D; \
  };
CHK_ELEM(die::bf16_t, die::bf16_t, kBFloat16)
CHK_ELEM(u16_of_i16, uint16_t, kShort)
CHK_ELEM(int16_t, int16_t, kShort)
CHK_ELEM(uint8_t, uint8_t, kByte)
CHK_ELEM(int, int, kInt)
CHK_ELEM(uint32_t, uint32_t, kInt)
CHK_ELEM(int64_t, int64_t, kLong)
CHK_ELEM(float, float, kFloat)
CHK_ELEM(void, void, ScalarType::Undefined)
#undef CHK_ELEM

// a dim of a shape: an exact size, ANY, or ge(n) for "at least n"
constexpr int64_t ANY = -1;
inline int64_t ge(int64_t n) { return -n - 1; }
using Dims = std::initializer_list<int64_t>;

inline bool dims_ok(const Tensor& t, Dims dims) {
  if (dims.size() == 0) return true;
  if ((size_t)t.dim() != dims.size()) return false;
  int64_t i = 0;
  for (int64_t d : dims) {
    const int64_t s = t.size(i++);
    if (d >= 0 ? s != d : s < -d - 1) return false;
  }
  return true;
}

inline std::string dims_str(Dims dims) {
  std::ostringstream o;
  o << "[";
  for (int64_t d : dims) {
    if (d == ANY) o << " *";
    else if (d < 0) o << " >=" << -d - 1;
    else o << " " << d;
  }
  o << " ]";
  return o.str();
}

template <class T> struct Rows {
  T* p = nullptr;
  int64_t ld = 0;  // row stride in elements
};

inline const Tensor* present(const Tensor& t) { return t.numel() ? &t : nullptr; }
inline const Tensor* present(const c10::optional<Tensor>& t) { return t.has_value() ? &*t : nullptr; }

struct Op {
  const char* op;
  c10::Device dev;

  Op(const char* op_, const Tensor& first, const char* arg) : op(op_), dev(first.device()) {
    TORCH_CHECK(first.is_cuda() || g_check_only, op, ": ", arg, " must be a GPU tensor");
  }

  template <class T>
  typename Elem<T>::type* dense(const Tensor& t, const char* arg, int64_t n, Dims dims = {}, int align = 0) const {
    TORCH_CHECK(t.device() == dev && (std::is_void<T>::value || t.scalar_type() == Elem<T>::dtype) &&
                    t.is_contiguous() && t.numel() >= n && dims_ok(t, dims) &&
                    (align == 0 || reinterpret_cast<uintptr_t>(t.data_ptr()) % align == 0),
                op, ": ", arg, " must be a contiguous ", Elem<T>::dtype, " array of >= ", n, " elements",
                dims.size() ? " shaped " + dims_str(dims) : std::string(),
                align ? ", " + std::to_string(align) + "-byte aligned," : std::string(), " on ", dev, "; got ",
                t.scalar_type(), " ", t.sizes(), " strides ", t.strides(), " on ", t.device());
    return static_cast<typename Elem<T>::type*>(t.data_ptr());
  }

  // aligned (the bf16 matrices the kernels read in 16-byte groups): row stride % 8 == 0, 16-byte aligned base
  template <class T = die::bf16_t>
  Rows<typename Elem<T>::type> rows(const Tensor& t, const char* arg, int64_t r = ANY, int64_t c = ANY,
                                    bool aligned = true) const {
    TORCH_CHECK(t.device() == dev && t.scalar_type() == Elem<T>::dtype && dims_ok(t, {r, c}), op, ": ", arg,
                " must be ", Elem<T>::dtype, " ", dims_str({r, c}), " on ", dev, "; got ", t.scalar_type(), " ",
                t.sizes(), " on ", t.device());
    TORCH_CHECK(t.stride(1) == 1, op, ": ", arg, " rows must be contiguous");
    TORCH_CHECK(!aligned || t.stride(0) % 8 == 0, op, ": ", arg, " row stride must be a multiple of 8 elements");
    TORCH_CHECK(!aligned || reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, op, ": ", arg,
                " must be 16-byte aligned");
    return {static_cast<typename Elem<T>::type*>(t.data_ptr()), t.stride(0)};
  }

  // An absent tensor may live anywhere and have any dtype: callers pass one shared empty tensor.
  template <class T, class Opt>
  typename Elem<T>::type* dense_opt(const Opt& t, const char* arg, int64_t n, Dims dims = {}, int align = 0) const {
    const Tensor* p = present(t);
    return p ? dense<T>(*p, arg, n, dims, align) : nullptr;
  }
  template <class T = die::bf16_t, class Opt>
  Rows<typename Elem<T>::type> rows_opt(const Opt& t, const char* arg, int64_t r = ANY, int64_t c = ANY) const {
    const Tensor* p = present(t);
    return p ? rows<T>(*p, arg, r, c) : Rows<typename Elem<T>::type>{};
  }

  int i32(int64_t v) const {
    TORCH_CHECK(v >= INT_MIN && v <= INT_MAX, op, ": size ", v, " does not fit an int");
    return (int)v;
  }
};

}  // namespace chk
