// Device helpers shared by the q/k prologue's forward (vb_qk_prologue.hip) and backward
// (vb_qk_prologue_bwd.hip): the lane-to-element mapping both keep (one lane owns 8 consecutive
// elements of a token row), the RoPE table row of a lane, and the in-wave sums.
#pragma once
#include "vb_common.hpp"

namespace vb {
namespace qk {

constexpr int kMaxWaves = 16;

template <class T>
__device__ __forceinline__ void unpack8(const u32x4 r, float (&f)[8]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[2 * e] = T::bits_to_f32(r[e] & 0xffff);
    f[2 * e + 1] = T::bits_to_f32(r[e] >> 16);
  }
}

// element i of a weight or bias (storage dtype or fp32); `fill` when the array is absent
template <class T>
__device__ __forceinline__ float affine_at(const void* p, int f32, int i, float fill) {
  if (!p) return fill;
  return f32 ? reinterpret_cast<const float*>(p)[i] : T::bits_to_f32(reinterpret_cast<const uint16_t*>(p)[i]);
}

__device__ __forceinline__ void lds8(const float* p, float (&f)[8]) {
  const f32x4 a = reinterpret_cast<const f32x4*>(p)[0], b = reinterpret_cast<const f32x4*>(p)[1];
#pragma unroll
  for (int e = 0; e < 4; ++e) { f[e] = a[e]; f[4 + e] = b[e]; }
}

// the RoPE table entries of one lane's 8 elements: (cos, sin) per element, or (re, im) per pair
struct RopeTab {
  float c[8], s[8];
  double zr[4], zi[4];
};

// the launch's one RoPE table, as vb_qk_prologue_args names it
struct RopeSrc {
  int rope_start;
  const float* cos; const float* sin;
  const void* freqs; int freqs_f64;
};

template <int ROPE>
__device__ __forceinline__ void load_tab(const RopeSrc& t, int l, int D, int d0, RopeTab& tab) {
  if (ROPE == VB_QK_ROPE_REAL) {
    // rows below rope_start load the table's first row and ignore it: the load never waits for a branch
    const int64_t at = (int64_t)(l > t.rope_start ? l - t.rope_start : 0) * D + d0;
    const f32x4* c = reinterpret_cast<const f32x4*>(t.cos + at);
    const f32x4* s = reinterpret_cast<const f32x4*>(t.sin + at);
    const f32x4 c0 = c[0], c1 = c[1], s0 = s[0], s1 = s[1];
#pragma unroll
    for (int e = 0; e < 4; ++e) { tab.c[e] = c0[e]; tab.c[4 + e] = c1[e]; tab.s[e] = s0[e]; tab.s[4 + e] = s1[e]; }
  } else {
    const int64_t at = (int64_t)l * D + d0;   // pair p of row l is scalars 2*(l*D/2 + p), +1
    if (t.freqs_f64) {
      typedef double f64x2 __attribute__((ext_vector_type(2)));
      const f64x2* z = reinterpret_cast<const f64x2*>(reinterpret_cast<const double*>(t.freqs) + at);
#pragma unroll
      for (int p = 0; p < 4; ++p) { const f64x2 v = z[p]; tab.zr[p] = v[0]; tab.zi[p] = v[1]; }
    } else {
      const f32x4* z = reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(t.freqs) + at);
      const f32x4 a = z[0], b = z[1];
      tab.zr[0] = a[0]; tab.zi[0] = a[1]; tab.zr[1] = a[2]; tab.zi[1] = a[3];
      tab.zr[2] = b[0]; tab.zi[2] = b[1]; tab.zr[3] = b[2]; tab.zi[3] = b[3];
    }
  }
}

// sum over the `lanes` (8, 16 or 64) neighbouring lanes that hold one head / one wave; every lane
// of the wave takes part
__device__ __forceinline__ float group_sum(float v, int lanes) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  if (lanes > 8) v += __shfl_xor(v, 8);
  if (lanes > 16) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
  }
  return v;
}

__device__ __forceinline__ float sum8(const float (&f)[8]) {
  return ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
}

}  // namespace qk
}  // namespace vb
