// The attention processors' q/k prologue for gfx950: q/k norm + RoPE in one HBM pass
// (vb_qk_prologue, include/vblade.h). Replaces the eager chains of
//   cogvideox/train/modify_cogvideo.py:54-64  per-head LayerNorm, apply_rotary_emb on the video rows
//   wanx/train/modify_wan.py:99-116           RMSNorm over the projection row, float64 complex RoPE
// with the same rounding points: norm -> storage dtype -> RoPE -> storage dtype.
//
// One lane owns 8 consecutive elements of a token row (one 16-byte load and store), so RoPE pairs
// are lane-local and a head is 8 (D=64) or 16 (D=128) neighbouring lanes. A workgroup of H*D/8 lanes
// (rounded up to whole waves) owns a whole token row of q and of k: the per-head LayerNorm is a
// butterfly over the head's lanes, the row-wide RMS one LDS reduction, and the RoPE table row is
// read once per token. Workgroups stride over the B*L rows.
//
// A row costs one memory round trip: its q, k and table loads are all issued before the first is
// used (none sits behind a branch on a nullable pointer or on the row index), and the weights and
// biases wait in LDS as fp32, staged once per workgroup with 1 and 0 standing in for absent ones.
//
// The real RoPE's two products and its sum are three separately rounded fp32 operations, as the three
// eager kernels compute them: they go through mul_rn / add_rn below, which no compiler flag can
// contract. The unit is also built with -ffp-contract=off (Makefile), and the fused multiply-adds of
// the norm are written out as fmaf, so the listing holds exactly the FMAs the source names.
#include <cmath>

#include "vb_qk_prologue.hpp"

namespace vb {
namespace {
using namespace qk;

struct QkTensor {
  const uint8_t* x; uint8_t* out;
  int64_t xs[2], os[2];
  const void* w; const void* b;
  int affine_f32; float eps;
  int norm_on, rope_on;   // this tensor takes the launch's norm / RoPE
};
struct QkTask {
  QkTensor t[2];
  int nt;            // 1: q alone, 2: q and k
  RopeSrc rope;      // the launch's one RoPE table: both tensors read the row once
  int B, L, H, D;
};

// One rounded operation each, whatever -ffp-contract says (this HIP release declares no __fmul_rn /
// __fadd_rn, and the device library's *_rte entry points still fuse under -ffp-contract=fast): the
// product passes through an empty asm statement, so the compiler cannot see a multiply feeding the
// sum that follows it and has nothing to contract. No instruction is emitted for it.
template <class F>
__device__ __forceinline__ F mul_rn(F a, F b) {
#pragma clang fp contract(off)
  F p = a * b;
  asm("" : "+v"(p));
  return p;
}
template <class F>
__device__ __forceinline__ F add_rn(F a, F b) {
#pragma clang fp contract(off)
  return a + b;
}

// x.float()*cos + rot(x).float()*sin, each operation rounded to fp32 on its own; then the storage dtype
template <class T>
__device__ __forceinline__ void rope_real(float (&f)[8], const RopeTab& tab) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = f[2 * p], b = f[2 * p + 1];
    f[2 * p] = round_to<T>(add_rn(mul_rn(a, tab.c[2 * p]), mul_rn(-b, tab.s[2 * p])));
    f[2 * p + 1] = round_to<T>(add_rn(mul_rn(b, tab.c[2 * p + 1]), mul_rn(a, tab.s[2 * p + 1])));
  }
}

// view_as_complex(x.double()) * freqs, then double -> float -> storage dtype
template <class T>
__device__ __forceinline__ void rope_complex(float (&f)[8], const RopeTab& tab) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const double a = f[2 * p], b = f[2 * p + 1];
    f[2 * p] = round_to<T>(static_cast<float>(add_rn(mul_rn(a, tab.zr[p]), -mul_rn(b, tab.zi[p]))));
    f[2 * p + 1] = round_to<T>(static_cast<float>(add_rn(mul_rn(a, tab.zi[p]), mul_rn(b, tab.zr[p]))));
  }
}

constexpr int kRedFloats = 2 * 2 * kMaxWaves;   // [row parity][tensor][wave]: the RMS partial sums

// dynamic LDS of a launch: the partial sums, then the fp32 weights (and biases) of both tensors
size_t lds_bytes(int norm, int H, int D) {
  const size_t affine = norm == VB_QK_NORM_LAYER_HEAD ? 4 * (size_t)D : norm == VB_QK_NORM_RMS_ROW ? 2 * (size_t)H * D : 0;
  return (kRedFloats + affine) * sizeof(float);
}

// NORM / ROPE: the launch's norm and RoPE modes; a tensor whose own mode is NONE skips that step
template <class T, int NORM, int ROPE>
__global__ void __launch_bounds__(1024) qk_prologue_kernel(const QkTask task) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* red = lds;
  float* aff = lds + kRedFloats;   // LayerNorm: [tensor][weight | bias][D]; RMSNorm: [tensor][H*D]
  const int D = task.D, W = task.H * task.D;
  const int c0 = (int)threadIdx.x * 8;     // this lane's first column of the H*D row
  const bool active = c0 < W;
  const int d0 = c0 & (D - 1);
  const int wave = (int)threadIdx.x >> 6, nwaves = ((int)blockDim.x + 63) >> 6;
  if (NORM == VB_QK_NORM_LAYER_HEAD) {
    for (int i = threadIdx.x; i < 4 * D; i += blockDim.x) {
      const int t = i / (2 * D), bias = (i / D) & 1, d = i & (D - 1);
      aff[i] = bias ? affine_at<T>(task.t[t].b, task.t[t].affine_f32, d, 0.f)
                    : affine_at<T>(task.t[t].w, task.t[t].affine_f32, d, 1.f);
    }
    __syncthreads();
  } else if (NORM == VB_QK_NORM_RMS_ROW) {
    for (int i = threadIdx.x; i < 2 * W; i += blockDim.x) {
      const int t = i >= W;
      aff[i] = affine_at<T>(task.t[t].w, task.t[t].affine_f32, i - t * W, 1.f);
    }
    __syncthreads();
  }
  const int64_t rows = (int64_t)task.B * task.L;
  int par = 0;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x, par ^= 1) {
    const int b = (int)(row / task.L), l = (int)(row - (int64_t)b * task.L);
    // every load of the row is issued before any is used
    u32x4 raw[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    RopeTab tab;
    if (active) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (t < task.nt)
          raw[t] = __builtin_nontemporal_load(   // read once: leave the caches to the table and the output
              reinterpret_cast<const u32x4*>(task.t[t].x + (b * task.t[t].xs[0] + l * task.t[t].xs[1] + c0) * 2));
      if (ROPE != VB_QK_ROPE_NONE) load_tab<ROPE>(task.rope, l, D, d0, tab);
    }
    float f[2][8];
#pragma unroll
    for (int t = 0; t < 2; ++t) unpack8<T>(raw[t], f[t]);

    float row_ms[2] = {0.f, 0.f};   // RMSNorm: the row's mean square
    if (NORM == VB_QK_NORM_RMS_ROW) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float sq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) sq[e] = f[t][e] * f[t][e];
        const float ss = group_sum(sum8(sq), 64);
        if ((threadIdx.x & 63) == 0) red[(par * 2 + t) * kMaxWaves + wave] = ss;
      }
      __syncthreads();   // one barrier per row: the next row writes the other parity
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float tot = 0.f;
        for (int w = 0; w < nwaves; ++w) tot += red[(par * 2 + t) * kMaxWaves + w];
        row_ms[t] = tot / (float)W;
      }
    }

#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t >= task.nt) break;
      const QkTensor& A = task.t[t];
      float (&x)[8] = f[t];
      if (NORM == VB_QK_NORM_LAYER_HEAD && A.norm_on) {
        const float mean = group_sum(sum8(x), D / 8) / (float)D;
        float dev[8], sq[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { dev[e] = x[e] - mean; sq[e] = dev[e] * dev[e]; }
        const float var = group_sum(sum8(sq), D / 8) / (float)D;
        const float rstd = rsqrtf(var + A.eps);
        float wv[8], bv[8];
        lds8(aff + t * 2 * D + d0, wv);
        lds8(aff + t * 2 * D + D + d0, bv);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = round_to<T>(fmaf(wv[e], rstd * dev[e], bv[e]));
      } else if (NORM == VB_QK_NORM_RMS_ROW && A.norm_on) {
        const float rstd = rsqrtf(row_ms[t] + A.eps);
        float wv[8];
        lds8(aff + t * W + (active ? c0 : 0), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = round_to<T>(wv[e] * (rstd * x[e]));
      }
      if (active) {
        if (ROPE != VB_QK_ROPE_NONE && A.rope_on && l >= task.rope.rope_start) {
          if (ROPE == VB_QK_ROPE_REAL) rope_real<T>(x, tab);
          else rope_complex<T>(x, tab);
        }
        u32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = pack2<T>(x[2 * e], x[2 * e + 1]);
        *reinterpret_cast<u32x4*>(A.out + (b * A.os[0] + l * A.os[1] + c0) * 2) = y;
      }
    }
  }
}

int check_tensor(const char* who, const vb_qk_prologue_args* a, QkTensor& t) {
  const std::string p = std::string("vb_qk_prologue: ") + who + ": ";
  if (!a->x || !a->out) return fail(VB_ERR_INVALID, p + "null x or out");
  if (a->B <= 0 || a->L <= 0 || a->H <= 0) return fail(VB_ERR_INVALID, p + "B, L and H must be positive");
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, p + "head_dim must be 64 or 128");
  if ((int64_t)a->H * a->D > 8192) return fail(VB_ERR_UNSUPPORTED, p + "rows wider than 8192 elements (H*D)");
  if (a->norm == VB_QK_NORM_RMS_ROW && lds_bytes(a->norm, a->H, a->D) > 65536)   // both tensors' fp32 weights in LDS
    return fail(VB_ERR_UNSUPPORTED, p + "RMSNorm rows wider than 8128 elements (H*D)");
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, p + "unknown dtype");
  const int64_t W = (int64_t)a->H * a->D;
  for (int i = 0; i < 2; ++i)
    if (((a->x_stride[i] | a->out_stride[i]) & 7) || a->x_stride[i] < 0 || a->out_stride[i] < 0)
      return fail(VB_ERR_INVALID, p + "strides must be non-negative multiples of 8 elements");
  if (a->x_stride[1] < W || a->out_stride[1] < W) return fail(VB_ERR_INVALID, p + "row stride below H*D");
  if (a->B > 1 && a->out_stride[0] < (int64_t)a->L * a->out_stride[1])
    return fail(VB_ERR_INVALID, p + "output batches overlap");
  if (((uintptr_t)a->x | (uintptr_t)a->out) & 15) return fail(VB_ERR_INVALID, p + "x and out must be 16-byte aligned");
  if (a->norm != VB_QK_NORM_NONE && a->norm != VB_QK_NORM_LAYER_HEAD && a->norm != VB_QK_NORM_RMS_ROW)
    return fail(VB_ERR_INVALID, p + "unknown norm mode");
  if (a->norm != VB_QK_NORM_NONE && !(a->eps >= 0.f && std::isfinite(a->eps)))
    return fail(VB_ERR_INVALID, p + "eps must be finite and non-negative");
  if (a->norm != VB_QK_NORM_LAYER_HEAD && a->bias) return fail(VB_ERR_INVALID, p + "bias needs the LayerNorm mode");
  if (a->norm == VB_QK_NORM_NONE && a->weight) return fail(VB_ERR_INVALID, p + "weight without a norm mode");
  if (((uintptr_t)a->weight | (uintptr_t)a->bias) & 15)
    return fail(VB_ERR_INVALID, p + "weight and bias must be 16-byte aligned");
  if (a->rope != VB_QK_ROPE_NONE && a->rope != VB_QK_ROPE_REAL && a->rope != VB_QK_ROPE_COMPLEX)
    return fail(VB_ERR_INVALID, p + "unknown rope mode");
  if (a->rope_start < 0 || a->rope_start > a->L) return fail(VB_ERR_INVALID, p + "rope_start outside [0, L]");
  if (a->rope == VB_QK_ROPE_REAL && (!a->cos || !a->sin))
    return fail(VB_ERR_INVALID, p + "real RoPE needs the cos and sin tables");
  if (a->rope == VB_QK_ROPE_COMPLEX && !a->freqs) return fail(VB_ERR_INVALID, p + "complex RoPE needs the freqs table");
  if (a->rope == VB_QK_ROPE_COMPLEX && a->rope_start != 0)
    return fail(VB_ERR_INVALID, p + "complex RoPE covers every row (rope_start must be 0)");
  if (a->rope == VB_QK_ROPE_REAL && (((uintptr_t)a->cos | (uintptr_t)a->sin) & 15))
    return fail(VB_ERR_INVALID, p + "cos and sin must be 16-byte aligned");
  if (a->rope == VB_QK_ROPE_COMPLEX && ((uintptr_t)a->freqs & 15))
    return fail(VB_ERR_INVALID, p + "freqs must be 16-byte aligned");
  t.x = reinterpret_cast<const uint8_t*>(a->x);
  t.out = reinterpret_cast<uint8_t*>(a->out);
  for (int i = 0; i < 2; ++i) { t.xs[i] = a->x_stride[i]; t.os[i] = a->out_stride[i]; }
  t.w = a->weight; t.b = a->bias; t.affine_f32 = a->affine_f32; t.eps = a->eps;
  t.norm_on = a->norm != VB_QK_NORM_NONE;
  t.rope_on = a->rope != VB_QK_ROPE_NONE && a->rope_start < a->L;   // rope_start == L: no row takes it
  return VB_OK;
}

template <class T, int NORM>
const void* pick_rope(int rope) {
  switch (rope) {
    case VB_QK_ROPE_REAL: return reinterpret_cast<const void*>(qk_prologue_kernel<T, NORM, VB_QK_ROPE_REAL>);
    case VB_QK_ROPE_COMPLEX: return reinterpret_cast<const void*>(qk_prologue_kernel<T, NORM, VB_QK_ROPE_COMPLEX>);
    default: return reinterpret_cast<const void*>(qk_prologue_kernel<T, NORM, VB_QK_ROPE_NONE>);
  }
}
template <class T>
const void* pick_kernel(int norm, int rope) {
  switch (norm) {
    case VB_QK_NORM_LAYER_HEAD: return pick_rope<T, VB_QK_NORM_LAYER_HEAD>(rope);
    case VB_QK_NORM_RMS_ROW: return pick_rope<T, VB_QK_NORM_RMS_ROW>(rope);
    default: return pick_rope<T, VB_QK_NORM_NONE>(rope);
  }
}

// the tensors that take RoPE name one table, one form and one first row
bool same_rope(const vb_qk_prologue_args* a, const vb_qk_prologue_args* b) {
  if (a->rope != b->rope || a->rope_start != b->rope_start) return false;
  return a->rope == VB_QK_ROPE_REAL ? (a->cos == b->cos && a->sin == b->sin)
                                    : (a->freqs == b->freqs && !a->freqs_f64 == !b->freqs_f64);
}

// one launch: `n` tensors that share the norm mode and the RoPE table of whichever of them has one,
// in the instantiation of those modes, on a resident-sized grid
int launch(const vb_qk_prologue_args* const* a, const QkTensor* t, int n, hipStream_t s) {
  QkTask task{};
  task.nt = n;
  int norm = VB_QK_NORM_NONE, rope = VB_QK_ROPE_NONE;
  for (int i = 0; i < n; ++i) {
    task.t[i] = t[i];
    if (t[i].norm_on) norm = a[i]->norm;
    if (t[i].rope_on && rope == VB_QK_ROPE_NONE) {
      rope = a[i]->rope;
      task.rope = RopeSrc{a[i]->rope_start, a[i]->cos, a[i]->sin, a[i]->freqs, a[i]->freqs_f64};
    }
  }
  task.B = a[0]->B; task.L = a[0]->L; task.H = a[0]->H; task.D = a[0]->D;
  const void* kernel = a[0]->dtype == VB_DTYPE_BF16 ? pick_kernel<BF16>(norm, rope) : pick_kernel<F16>(norm, rope);
  const int threads = (task.H * task.D / 8 + 63) / 64 * 64;   // <= 1024 (H*D <= 8192)
  const size_t smem = lds_bytes(norm, task.H, task.D);       // <= 64 KiB (check_tensor)
  const int64_t rows = (int64_t)task.B * task.L;
  const int64_t cap = resident_grid(kernel, threads, smem);
  const dim3 grid((unsigned)(rows < cap ? rows : cap));
  void* params[] = {&task};
  (void)hipLaunchKernel(kernel, grid, dim3(threads), params, smem, s);
  return check_launch("qk_prologue_kernel");
}

}  // namespace
}  // namespace vb

extern "C" int vb_qk_prologue(const vb_qk_prologue_args* q, const vb_qk_prologue_args* k, void* stream) {
  using namespace vb;
  if (!q) return fail(VB_ERR_INVALID, "vb_qk_prologue: null q arguments");
  QkTensor t[2] = {};
  if (int rc = check_tensor("q", q, t[0])) return rc;
  if (k) {
    if (int rc = check_tensor("k", k, t[1])) return rc;
    if (k->B != q->B || k->L != q->L || k->H != q->H || k->D != q->D || k->dtype != q->dtype)
      return fail(VB_ERR_INVALID, "vb_qk_prologue: k must have q's B, L, H, D and dtype");
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const vb_qk_prologue_args* a[2] = {q, k};
  // one launch serves both tensors unless they name two different norms or two different RoPE tables
  // (no processor does): then each gets its own launch on `stream`
  const bool split = k && ((t[0].norm_on && t[1].norm_on && q->norm != k->norm) ||
                           (t[0].rope_on && t[1].rope_on && !same_rope(q, k)));
  if (!split) return launch(a, t, k ? 2 : 1, s);
  if (int rc = launch(a, t, 1, s)) return rc;
  return launch(a + 1, t + 1, 1, s);
}
