// The q/k prologue's backward for gfx950 (vb_qk_prologue_bwd, include/vblade.h): the transposes of
// RoPE and of the q/k norm in one HBM pass, for training through the processors' fused prologue.
//
// The forward's lane-to-element mapping (vb_qk_prologue.hpp): one lane owns 8 consecutive elements
// of a token row, a workgroup of H*D/8 lanes owns a token row of q and of k, the RoPE table row is
// read once for both, and workgroups stride over the B*L rows. A row costs one memory round trip:
// x and g of both tensors and the table row are all issued before the first is used. The
// statistics are recomputed from x as the forward computes them; between loading g and storing dx
// nothing is rounded to the storage dtype.
//
// LayerNorm: one butterfly round for the mean, one for sum(dev^2), sum(a) and sum(a*dev) together.
// RMSNorm: sum(x^2) and sum(a*x) do not depend on rstd (mean(a*xhat) = rstd*mean(a*x)), so both go
// through the same LDS reduction: one barrier per row.
//
// Weight and bias gradients, without atomics: each lane accumulates fp32 partials over the rows its
// workgroup visits; after the row loop the workgroup reduces across heads (LayerNorm) through LDS
// in head order and writes its partial vector to the workspace; wgrad_reduce_kernel then adds the
// workgroups' partials in a fixed order. The order depends on the shape and the grid alone.
#include <cmath>

#include "vb_qk_prologue.hpp"

namespace vb {
namespace {
using namespace qk;

struct BwdTensor {
  const uint8_t* x; const uint8_t* g; uint8_t* dx;
  int64_t xs[2], gs[3], ds[2];
  const void* w;
  int affine_f32; float eps;
  int norm_on, rope_on;   // this tensor takes the launch's norm / RoPE
  float* part_w;          // [grid][D or H*D] partial sums in the workspace; null: not requested
  float* part_b;          // [grid][D]
};
struct BwdTask {
  BwdTensor t[2];
  int nt;            // tensors of this launch: q and k, or one of them
  RopeSrc rope;      // the launch's one RoPE table
  int B, L, H, D;
};

constexpr int kRedFloats = 2 * 2 * 2 * kMaxWaves;   // [row parity][tensor][sum(x^2) | sum(a*x)][wave]

// dynamic LDS of a launch: the RMS partial sums, the fp32 weights of both tensors, and for the
// LayerNorm one H*D row for the cross-head reduction of the weight gradients
size_t lds_bytes(int norm, int H, int D) {
  const size_t W = (size_t)H * D;
  const size_t extra = norm == VB_QK_NORM_LAYER_HEAD ? 2 * (size_t)D + W : norm == VB_QK_NORM_RMS_ROW ? 2 * W : 0;
  return (kRedFloats + extra) * sizeof(float);
}

// gy = RoPE^T g, in place
__device__ __forceinline__ void rope_real_t(float (&g)[8], const RopeTab& tab) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const float a = g[2 * p], b = g[2 * p + 1];
    g[2 * p] = a * tab.c[2 * p] + b * tab.s[2 * p + 1];
    g[2 * p + 1] = b * tab.c[2 * p + 1] - a * tab.s[2 * p];
  }
}
__device__ __forceinline__ void rope_complex_t(float (&g)[8], const RopeTab& tab) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const double a = g[2 * p], b = g[2 * p + 1];
    g[2 * p] = static_cast<float>(a * tab.zr[p] + b * tab.zi[p]);
    g[2 * p + 1] = static_cast<float>(b * tab.zr[p] - a * tab.zi[p]);
  }
}

__device__ __forceinline__ void store8(float* p, const float (&f)[8]) {
  reinterpret_cast<f32x4*>(p)[0] = f32x4{f[0], f[1], f[2], f[3]};
  reinterpret_cast<f32x4*>(p)[1] = f32x4{f[4], f[5], f[6], f[7]};
}

// NORM / ROPE: the launch's norm and RoPE modes; a tensor whose own mode is NONE skips that step
template <class T, int NORM, int ROPE>
__global__ void __launch_bounds__(1024) qk_prologue_bwd_kernel(const BwdTask task) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* red = lds;
  float* aff = lds + kRedFloats;   // LayerNorm: [tensor][D] then the [H*D] reduction row; RMSNorm: [tensor][H*D]
  const int D = task.D, W = task.H * task.D;
  const int c0 = (int)threadIdx.x * 8;     // this lane's first column of the H*D row
  const bool active = c0 < W;              // heads are whole groups of lanes: active or not as one
  const int d0 = c0 & (D - 1), h0 = c0 / D;
  const int wave = (int)threadIdx.x >> 6, nwaves = ((int)blockDim.x + 63) >> 6;
  // the weights wait in LDS as fp32, 1 standing in for an absent one (t is unrolled: the kernel
  // arguments are never indexed by a run-time value)
  if (NORM != VB_QK_NORM_NONE) {
    const int n = NORM == VB_QK_NORM_LAYER_HEAD ? D : W;
#pragma unroll
    for (int t = 0; t < 2; ++t)
      for (int i = threadIdx.x; i < n; i += blockDim.x)
        aff[t * n + i] = affine_at<T>(task.t[t].w, task.t[t].affine_f32, i, 1.f);
    __syncthreads();
  }
  float accw[2][8], accb[2][8];   // sum over this workgroup's rows of gy*xhat and of gy
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) accw[t][e] = accb[t][e] = 0.f;

  const int64_t rows = (int64_t)task.B * task.L;
  int par = 0;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x, par ^= 1) {
    const int b = (int)(row / task.L), l = (int)(row - (int64_t)b * task.L);
    // every load of the row is issued before any is used; inactive lanes hold zeros
    u32x4 raw_x[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, raw_g[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    RopeTab tab;
    if (active) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
        if (t < task.nt) {
          const BwdTensor& A = task.t[t];
          raw_x[t] = __builtin_nontemporal_load(
              reinterpret_cast<const u32x4*>(A.x + (b * A.xs[0] + l * A.xs[1] + c0) * 2));
          raw_g[t] = __builtin_nontemporal_load(
              reinterpret_cast<const u32x4*>(A.g + (b * A.gs[0] + l * A.gs[1] + h0 * A.gs[2] + d0) * 2));
        }
      if (ROPE != VB_QK_ROPE_NONE) load_tab<ROPE>(task.rope, l, D, d0, tab);
    }
    float x[2][8], gy[2][8];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      unpack8<T>(raw_x[t], x[t]);
      unpack8<T>(raw_g[t], gy[t]);
      if (ROPE != VB_QK_ROPE_NONE && active && t < task.nt && task.t[t].rope_on && l >= task.rope.rope_start) {
        if (ROPE == VB_QK_ROPE_REAL) rope_real_t(gy[t], tab);
        else rope_complex_t(gy[t], tab);
      }
    }

    float a[2][8];                   // gy * weight
    float row_sq[2] = {0.f, 0.f};    // RMSNorm: the row's sum(x^2) and sum(a*x)
    float row_ax[2] = {0.f, 0.f};
    if (NORM == VB_QK_NORM_RMS_ROW) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float wv[8], sq[8], ax[8];
        lds8(aff + t * W + (active ? c0 : 0), wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          a[t][e] = gy[t][e] * wv[e];
          sq[e] = x[t][e] * x[t][e];
          ax[e] = a[t][e] * x[t][e];
        }
        const float ss = group_sum(sum8(sq), 64), sa = group_sum(sum8(ax), 64);
        if ((threadIdx.x & 63) == 0) {
          red[((par * 2 + t) * 2 + 0) * kMaxWaves + wave] = ss;
          red[((par * 2 + t) * 2 + 1) * kMaxWaves + wave] = sa;
        }
      }
      __syncthreads();   // one barrier per row: the next row writes the other parity
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float ss = 0.f, sa = 0.f;
        for (int w = 0; w < nwaves; ++w) {
          ss += red[((par * 2 + t) * 2 + 0) * kMaxWaves + w];
          sa += red[((par * 2 + t) * 2 + 1) * kMaxWaves + w];
        }
        row_sq[t] = ss;
        row_ax[t] = sa;
      }
    }

#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t >= task.nt) break;
      const BwdTensor& A = task.t[t];
      float dx[8];
      if (NORM == VB_QK_NORM_LAYER_HEAD && A.norm_on) {
        const float mean = group_sum(sum8(x[t]), D / 8) / (float)D;
        float wv[8], dev[8], sq[8], ad[8];
        lds8(aff + t * D + d0, wv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          dev[e] = x[t][e] - mean;
          sq[e] = dev[e] * dev[e];
          a[t][e] = gy[t][e] * wv[e];
          ad[e] = a[t][e] * dev[e];
        }
        const float s_sq = group_sum(sum8(sq), D / 8);
        const float s_a = group_sum(sum8(a[t]), D / 8);
        const float s_ad = group_sum(sum8(ad), D / 8);
        const float rstd = rsqrtf(s_sq / (float)D + A.eps);
        const float mean_a = s_a / (float)D;
        const float mean_ax = rstd * (s_ad / (float)D);   // mean_D(a * xhat)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xhat = dev[e] * rstd;
          dx[e] = rstd * ((a[t][e] - mean_a) - xhat * mean_ax);
          if (active) {
            if (A.part_w) accw[t][e] += gy[t][e] * xhat;
            if (A.part_b) accb[t][e] += gy[t][e];
          }
        }
      } else if (NORM == VB_QK_NORM_RMS_ROW && A.norm_on) {
        const float rstd = rsqrtf(row_sq[t] / (float)W + A.eps);
        const float mean_ax = rstd * (row_ax[t] / (float)W);   // mean_W(a * xhat)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float xhat = x[t][e] * rstd;
          dx[e] = rstd * (a[t][e] - xhat * mean_ax);
          if (active && A.part_w) accw[t][e] += gy[t][e] * xhat;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) dx[e] = gy[t][e];
      }
      if (active) {
        u32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = pack2<T>(dx[2 * e], dx[2 * e + 1]);
        *reinterpret_cast<u32x4*>(A.dx + (b * A.ds[0] + l * A.ds[1] + c0) * 2) = y;
      }
    }
  }

  // this workgroup's partial sums -> workspace row blockIdx.x
  if (NORM == VB_QK_NORM_RMS_ROW) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (t < task.nt && task.t[t].part_w && active) store8(task.t[t].part_w + (int64_t)blockIdx.x * W + c0, accw[t]);
  } else if (NORM == VB_QK_NORM_LAYER_HEAD) {
    float* across = aff + 2 * D;   // [H][D]: summed over the heads in head order
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t >= task.nt) break;
#pragma unroll
      for (int which = 0; which < 2; ++which) {
        float* part = which ? task.t[t].part_b : task.t[t].part_w;
        if (!part) continue;   // the same for every lane of the workgroup
        __syncthreads();
        if (active) store8(across + c0, which ? accb[t] : accw[t]);
        __syncthreads();
        for (int d = threadIdx.x; d < D; d += blockDim.x) {   // D = 128 with H <= 4: 64 lanes only
          float s = 0.f;
          for (int h = 0; h < task.H; ++h) s += across[h * D + d];
          part[(int64_t)blockIdx.x * D + d] = s;
        }
      }
    }
  }
}

// out[job][c] = sum over the G workgroups' partial vectors, in a fixed order: 16 slices of
// consecutive workgroups summed in order, then the 16 slice sums in order
struct ReduceJobs {
  const float* part[4]; float* out[4];
  int n[4], G[4];
};
constexpr int kSlices = 16;
__global__ void __launch_bounds__(64 * kSlices) wgrad_reduce_kernel(const ReduceJobs jobs) {
  __shared__ float sm[kSlices][64];
  const int job = blockIdx.y, n = jobs.n[job], G = jobs.G[job];
  if ((int)blockIdx.x * 64 >= n) return;   // n is a multiple of 64: whole blocks
  const int col = blockIdx.x * 64 + threadIdx.x, slice = threadIdx.y;
  const int per = (G + kSlices - 1) / kSlices;
  const int g0 = slice * per, g1 = g0 + per < G ? g0 + per : G;
  const float* p = jobs.part[job] + col;
  float s = 0.f;
#pragma unroll 8
  for (int g = g0; g < g1; ++g) s += p[(int64_t)g * n];
  sm[slice][threadIdx.x] = s;
  __syncthreads();
  if (slice == 0) {
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kSlices; ++i) tot += sm[i][threadIdx.x];
    jobs.out[job][col] = tot;
  }
}

typedef vb_qk_prologue_bwd_args Args;

bool overlap(const void* a, int64_t a_elems, const void* b, int64_t b_elems) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)b_elems * 2 && b0 < a0 + (uintptr_t)a_elems * 2;
}

int check_tensor(const char* who, const Args* a, BwdTensor& t) {
  const std::string p = std::string("vb_qk_prologue_bwd: ") + who + ": ";
  if (!a->x || !a->g || !a->dx) return fail(VB_ERR_INVALID, p + "null x, g or dx");
  if (a->B <= 0 || a->L <= 0 || a->H <= 0) return fail(VB_ERR_INVALID, p + "B, L and H must be positive");
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, p + "head_dim must be 64 or 128");
  if ((int64_t)a->H * a->D > 8192) return fail(VB_ERR_UNSUPPORTED, p + "rows wider than 8192 elements (H*D)");
  if (a->norm == VB_QK_NORM_RMS_ROW && lds_bytes(a->norm, a->H, a->D) > 65536)   // both tensors' fp32 weights in LDS
    return fail(VB_ERR_UNSUPPORTED, p + "RMSNorm rows wider than 8128 elements (H*D)");
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, p + "unknown dtype");
  const int64_t W = (int64_t)a->H * a->D;
  for (int i = 0; i < 2; ++i)
    if (((a->x_stride[i] | a->dx_stride[i]) & 7) || a->x_stride[i] < 0 || a->dx_stride[i] < 0)
      return fail(VB_ERR_INVALID, p + "strides must be non-negative multiples of 8 elements");
  for (int i = 0; i < 3; ++i)
    if ((a->g_stride[i] & 7) || a->g_stride[i] < 0)
      return fail(VB_ERR_INVALID, p + "g strides must be non-negative multiples of 8 elements");
  if (a->x_stride[1] < W || a->dx_stride[1] < W) return fail(VB_ERR_INVALID, p + "row stride below H*D");
  if (a->H > 1 && a->g_stride[2] < a->D) return fail(VB_ERR_INVALID, p + "g head stride below D");
  if (a->B > 1 && a->dx_stride[0] < (int64_t)a->L * a->dx_stride[1])
    return fail(VB_ERR_INVALID, p + "dx batches overlap");
  if (((uintptr_t)a->x | (uintptr_t)a->g | (uintptr_t)a->dx) & 15)
    return fail(VB_ERR_INVALID, p + "x, g and dx must be 16-byte aligned");
  const int64_t x_elems = (a->B - 1) * a->x_stride[0] + (a->L - 1) * a->x_stride[1] + W;
  const int64_t d_elems = (a->B - 1) * a->dx_stride[0] + (a->L - 1) * a->dx_stride[1] + W;
  const int64_t g_elems = (a->B - 1) * a->g_stride[0] + (a->L - 1) * a->g_stride[1] + (a->H - 1) * a->g_stride[2] + a->D;
  if (overlap(a->dx, d_elems, a->x, x_elems) || overlap(a->dx, d_elems, a->g, g_elems))
    return fail(VB_ERR_INVALID, p + "dx must not alias x or g");
  if (a->norm != VB_QK_NORM_NONE && a->norm != VB_QK_NORM_LAYER_HEAD && a->norm != VB_QK_NORM_RMS_ROW)
    return fail(VB_ERR_INVALID, p + "unknown norm mode");
  if (a->norm != VB_QK_NORM_NONE && !(a->eps >= 0.f && std::isfinite(a->eps)))
    return fail(VB_ERR_INVALID, p + "eps must be finite and non-negative");
  if (a->norm != VB_QK_NORM_LAYER_HEAD && a->bias) return fail(VB_ERR_INVALID, p + "bias needs the LayerNorm mode");
  if (a->norm == VB_QK_NORM_NONE && a->weight) return fail(VB_ERR_INVALID, p + "weight without a norm mode");
  if (a->norm != VB_QK_NORM_LAYER_HEAD && a->dbias) return fail(VB_ERR_INVALID, p + "dbias needs the LayerNorm mode");
  if (a->norm == VB_QK_NORM_NONE && a->dweight) return fail(VB_ERR_INVALID, p + "dweight without a norm mode");
  if (((uintptr_t)a->weight | (uintptr_t)a->bias | (uintptr_t)a->dweight | (uintptr_t)a->dbias) & 15)
    return fail(VB_ERR_INVALID, p + "weight, bias, dweight and dbias must be 16-byte aligned");
  if (a->grid_limit < 0) return fail(VB_ERR_INVALID, p + "grid_limit must not be negative");
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
  t.g = reinterpret_cast<const uint8_t*>(a->g);
  t.dx = reinterpret_cast<uint8_t*>(a->dx);
  for (int i = 0; i < 2; ++i) { t.xs[i] = a->x_stride[i]; t.ds[i] = a->dx_stride[i]; }
  for (int i = 0; i < 3; ++i) t.gs[i] = a->g_stride[i];
  t.w = a->weight; t.affine_f32 = a->affine_f32; t.eps = a->eps;
  t.norm_on = a->norm != VB_QK_NORM_NONE;
  t.rope_on = a->rope != VB_QK_ROPE_NONE && a->rope_start < a->L;   // rope_start == L: no row takes it
  return VB_OK;
}

// the most workgroups a launch for `a` can have: what the workspace is sized for
int64_t grid_bound(const Args* a) {
  const int64_t rows = (int64_t)a->B * a->L;
  const int64_t cap = a->grid_limit > 0 ? a->grid_limit : VB_QK_BWD_MAX_GRID;
  return rows < cap ? rows : cap;
}
uint64_t workspace_floats(const Args* a) {
  if (!a || a->B <= 0 || a->L <= 0 || a->H <= 0 || a->D <= 0) return 0;
  const uint64_t G = (uint64_t)grid_bound(a);
  const uint64_t n = a->norm == VB_QK_NORM_LAYER_HEAD ? (uint64_t)a->D : (uint64_t)a->H * a->D;
  return (a->dweight ? G * n : 0) + (a->dbias ? G * (uint64_t)a->D : 0);
}

template <class T, int NORM>
const void* pick_rope(int rope) {
  switch (rope) {
    case VB_QK_ROPE_REAL: return reinterpret_cast<const void*>(qk_prologue_bwd_kernel<T, NORM, VB_QK_ROPE_REAL>);
    case VB_QK_ROPE_COMPLEX: return reinterpret_cast<const void*>(qk_prologue_bwd_kernel<T, NORM, VB_QK_ROPE_COMPLEX>);
    default: return reinterpret_cast<const void*>(qk_prologue_bwd_kernel<T, NORM, VB_QK_ROPE_NONE>);
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
bool same_rope(const Args* a, const Args* b) {
  if (a->rope != b->rope || a->rope_start != b->rope_start) return false;
  return a->rope == VB_QK_ROPE_REAL ? (a->cos == b->cos && a->sin == b->sin)
                                    : (a->freqs == b->freqs && !a->freqs_f64 == !b->freqs_f64);
}

// one launch: `n` tensors that share the norm mode and the RoPE table of whichever of them has one;
// *grid is the number of workgroups it ran, i.e. of partial vectors it left in the workspace
int launch(const Args* const* a, const BwdTensor* t, int n, hipStream_t s, int* grid) {
  BwdTask task{};
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
  int64_t cap = a[0]->grid_limit;
  if (cap <= 0) {
    cap = resident_grid(kernel, threads, smem);
    if (cap > VB_QK_BWD_MAX_GRID) cap = VB_QK_BWD_MAX_GRID;
  }
  *grid = (int)(rows < cap ? rows : cap);   // <= grid_bound(a[i]) for every tensor of the launch
  void* params[] = {&task};
  (void)hipLaunchKernel(kernel, dim3((unsigned)*grid), dim3(threads), params, smem, s);
  return check_launch("qk_prologue_bwd_kernel");
}

}  // namespace
}  // namespace vb

extern "C" uint64_t vb_qk_prologue_bwd_workspace_size(const vb_qk_prologue_bwd_args* q,
                                                      const vb_qk_prologue_bwd_args* k) {
  return (vb::workspace_floats(q) + vb::workspace_floats(k)) * sizeof(float);
}

extern "C" int vb_qk_prologue_bwd(const vb_qk_prologue_bwd_args* q, const vb_qk_prologue_bwd_args* k, void* stream) {
  using namespace vb;
  if (!q && !k) return fail(VB_ERR_INVALID, "vb_qk_prologue_bwd: null q and k arguments");
  const Args* a[2] = {q ? q : k, q ? k : nullptr};
  const int n = q && k ? 2 : 1;
  BwdTensor t[2] = {};
  if (int rc = check_tensor(q ? "q" : "k", a[0], t[0])) return rc;
  if (n == 2) {
    if (int rc = check_tensor("k", k, t[1])) return rc;
    if (k->B != q->B || k->L != q->L || k->H != q->H || k->D != q->D || k->dtype != q->dtype ||
        k->grid_limit != q->grid_limit)
      return fail(VB_ERR_INVALID, "vb_qk_prologue_bwd: k must have q's B, L, H, D, dtype and grid_limit");
  }
  // the workspace: per tensor, its dweight partials [grid][D or H*D] and then its dbias partials [grid][D]
  const uint64_t need = vb_qk_prologue_bwd_workspace_size(q, k);
  if (need) {
    if (!a[0]->workspace || ((uintptr_t)a[0]->workspace & 15) || a[0]->workspace_bytes < need)
      return fail(VB_ERR_INVALID, "vb_qk_prologue_bwd: workspace null, not 16-byte aligned or smaller than "
                                  "vb_qk_prologue_bwd_workspace_size (" + std::to_string(need) + " bytes)");
    float* ws = reinterpret_cast<float*>(a[0]->workspace);
    for (int i = 0; i < n; ++i) {
      const int64_t G = grid_bound(a[i]);
      const int64_t nw = a[i]->norm == VB_QK_NORM_LAYER_HEAD ? a[i]->D : (int64_t)a[i]->H * a[i]->D;
      if (a[i]->dweight) { t[i].part_w = ws; ws += G * nw; }
      if (a[i]->dbias) { t[i].part_b = ws; ws += G * a[i]->D; }
    }
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // one launch serves both tensors unless they name two different norms or two different RoPE tables
  // (no processor does): then each gets its own launch on `stream`
  const bool split = n == 2 && ((t[0].norm_on && t[1].norm_on && q->norm != k->norm) ||
                                (t[0].rope_on && t[1].rope_on && !same_rope(q, k)));
  int grid[2] = {0, 0};
  if (!split) {
    if (int rc = launch(a, t, n, s, &grid[0])) return rc;
    grid[1] = grid[0];
  } else {
    if (int rc = launch(a, t, 1, s, &grid[0])) return rc;
    if (int rc = launch(a + 1, t + 1, 1, s, &grid[1])) return rc;
  }
  if (!need) return VB_OK;
  ReduceJobs jobs{};
  int nj = 0, widest = 0;
  for (int i = 0; i < n; ++i) {
    const int nw = a[i]->norm == VB_QK_NORM_LAYER_HEAD ? a[i]->D : a[i]->H * a[i]->D;
    if (t[i].part_w) { jobs.part[nj] = t[i].part_w; jobs.out[nj] = a[i]->dweight; jobs.n[nj] = nw; jobs.G[nj++] = grid[i]; }
    if (t[i].part_b) { jobs.part[nj] = t[i].part_b; jobs.out[nj] = a[i]->dbias; jobs.n[nj] = a[i]->D; jobs.G[nj++] = grid[i]; }
  }
  for (int j = 0; j < nj; ++j) widest = jobs.n[j] > widest ? jobs.n[j] : widest;
  void* params[] = {&jobs};
  (void)hipLaunchKernel(reinterpret_cast<const void*>(wgrad_reduce_kernel), dim3(widest / 64, nj), dim3(64, kSlices),
                        params, 0, s);
  return check_launch("qk_prologue_bwd wgrad_reduce_kernel");
}
