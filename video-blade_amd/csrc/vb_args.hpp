// Host-side argument checks and kernel dispatch shared by the attention entry points (forward,
// backward, multi-level). Host only: nothing here is called from a kernel.
#pragma once
#include <cmath>
#include <type_traits>

#include "vb_common.hpp"

namespace vb {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// every stride of a [B,H,L,D] view is a multiple of 8 elements (16-byte chunks stay whole)
inline bool strides_mul8(const int64_t* s) { return ((s[0] | s[1] | s[2]) & 7) == 0; }
// one (b,h) slice of L rows at `row_stride` 16-bit elements must be addressable by a 32-bit buffer
// offset (the tile DMAs address rows through buffer descriptors)
inline bool slice_fits32(int64_t L, int64_t row_stride, int D) {
  return (L - 1) * 2 * row_stride + 2 * D < (int64_t(1) << 31);
}
// workspace regions start at multiples of 256 bytes
inline uint64_t round_up256(uint64_t x) { return (x + 255) & ~uint64_t(255); }
// the softmax scale of an entry point: the caller's if positive, else 1/sqrt(D)
inline float scale_or_default(float scale, int D) { return scale > 0.f ? scale : (float)(1.0 / sqrt((double)D)); }

inline bool head_dim_ok(int D) { return D == 64 || D == 128; }
inline bool dtype_ok(int dtype) { return dtype == VB_DTYPE_BF16 || dtype == VB_DTYPE_F16; }

template <int V>
using Int = std::integral_constant<int, V>;

// f(cs..., std::bool_constant<b>...): run-time bools become trailing compile-time arguments
template <class F>
int with_bools(F&& f) { return f(); }
template <class F, class... Rest>
int with_bools(F&& f, bool b, Rest... rest) {
  auto next = [&](auto B) { return with_bools([&](auto... cs) { return f(B, cs...); }, rest...); };
  return b ? next(std::true_type{}) : next(std::false_type{});
}

// (D, dtype, bools...) -> f(Int<D>{}, T{}, std::bool_constant<b>{}...), T = BF16 or F16: the one
// place a run-time head shape picks template arguments, e.g.
//   dispatch_head(D, dtype, [&](auto d, auto t, auto pool) {
//     hipLaunchKernelGGL((kernel<d(), decltype(t), pool()>), ...); return check_launch("kernel"); }, pooled);
// The entry points validate D and dtype first, with their own messages and in their own order.
template <class F, class... Bools>
int dispatch_head(int D, int dtype, F&& f, Bools... bools) {
  if (!head_dim_ok(D) || !dtype_ok(dtype)) return fail(VB_ERR_INVALID, "dispatch_head: head_dim or dtype not validated");
  return with_bools(
      [&](auto... bs) {
        if (dtype == VB_DTYPE_BF16) return D == 64 ? f(Int<64>{}, BF16{}, bs...) : f(Int<128>{}, BF16{}, bs...);
        return D == 64 ? f(Int<64>{}, F16{}, bs...) : f(Int<128>{}, F16{}, bs...);
      },
      bools...);
}

}  // namespace vb
