// Mean pooling of K/V (fused with the Gilbert-ordered K/V copies) and the reference-faithful LSE
// combine for gfx950: the two HBM-bound element passes of the adaptive path.
//   simple_pooling (cogvideox/train/special_attentions_local/TrainRelated/cogvideo_blocksparseattn.py:83-88)
//   + the rearrange gathers (:148-150); the bf16 combine of adaptive_block_sparse_attn (:374-393).
#include <cstdlib>

#include "vb_pool.hpp"

namespace vb {

// simple_pooling of K and V (+ the Gilbert-ordered copies): pool_kv_span (vb_pool.hpp), grid-strided
template <class T>
__global__ void __launch_bounds__(256) pool_kv_kernel(const PoolTask t) {
  pool_kv_span<T>(t, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// Workgroups of an HBM-bound pass that runs beside the predictor's score kernel on another stream:
// a capped, grid-strided launch leaves most CUs to the MFMA-bound kernel instead of flooding the
// dispatcher (kPoolWgsDefault; 0 = one workgroup per 256 chunks).
unsigned pool_grid(int64_t work_items) {
  constexpr int cap = kPoolWgsDefault;
  const int64_t n = (work_items + 255) / 256;
  return (unsigned)((cap > 0 && n > cap) ? cap : n);
}

// adaptive_block_sparse_attn's combine (cogvideo_blocksparseattn.py:374-393), eager-op rounding. The
// arithmetic of a row (its weights) and of a 16-byte chunk is written once, for the contiguous and the
// strided kernel: the two differ in addressing only.
template <class T>
__device__ __forceinline__ void lse_combine_weights(float lse1, float lse2, float gap, float& a, float& b) {
  const float l1 = round_to<T>(lse1);
  const float l2 = round_to<T>(lse2);
  const float log_g = round_to<T>(logf(round_to<T>(gap)));
  const float w2 = round_to<T>(l2 + log_g);
  const float mx = fmaxf(l1, w2);
  const float e1 = round_to<T>(expf(round_to<T>(l1 - mx)));
  const float e2 = round_to<T>(expf(round_to<T>(w2 - mx)));
  a = round_to<T>(e1 / round_to<T>(e1 + e2));
  b = round_to<T>(1.0f - a);
}

// No contraction here: with fp16 the compiler narrows the three rounded fp32 operations to half
// arithmetic (the same values) and, contracting, fused v1 * a into the addition (v_pk_fma_f16), which
// drops the rounding of that product the reference makes (tests/test_gpu_lse_combine.py, check (c)).
template <class T>
__device__ __forceinline__ u32x4 lse_combine_chunk(const u32x4& x1, const u32x4& x2, float a, float b) {
#pragma clang fp contract(off)
  u32x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float r[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const float v1 = T::bits_to_f32((x1[e] >> (16 * s)) & 0xffff);
      const float v2 = T::bits_to_f32((x2[e] >> (16 * s)) & 0xffff);
      r[s] = round_to<T>(round_to<T>(v1 * a) + round_to<T>(v2 * b));
    }
    y[e] = pack2<T>(r[0], r[1]);
  }
  return y;
}

template <class T>
__global__ void __launch_bounds__(256) lse_combine_kernel(const uint8_t* out1, const float* lse1, const uint8_t* out2,
                                                          const float* lse2, int64_t rows, int D, float gap,
                                                          uint8_t* out, float* alpha_out) {
  const int CH = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= rows * CH) return;
  const int64_t row = idx / CH;
  const int ch = idx % CH;
  float a, b;
  lse_combine_weights<T>(lse1[row], lse2[row], gap, a, b);
  if (alpha_out && ch == 0) alpha_out[row] = a;
  const u32x4 x1 = *reinterpret_cast<const u32x4*>(out1 + (row * D + ch * 8) * 2);
  const u32x4 x2 = *reinterpret_cast<const u32x4*>(out2 + (row * D + ch * 8) * 2);
  *reinterpret_cast<u32x4*>(out + (row * D + ch * 8) * 2) = lse_combine_chunk<T>(x1, x2, a, b);
}

// The same combine on [B,H,L,D] tensors addressed through (batch, head, row) element strides. One
// 16-byte chunk per lane, D/8 = 8 or 16 consecutive lanes per row: a wave covers 8 or 4 whole rows, so
// a row's D*2 contiguous bytes leave (and arrive) as full 128-byte lines whatever the row stride is.
// grid (ceil(L*D/8 / 256), H, B): no division by a runtime L or H in the address.
struct CombineStrides { int64_t o1[3], o2[3], o[3]; };

template <class T, int D>
__global__ void __launch_bounds__(256) lse_combine_strided_kernel(const uint8_t* out1, const float* lse1,
                                                                  const uint8_t* out2, const float* lse2,
                                                                  const CombineStrides st, int L, float gap,
                                                                  uint8_t* out, float* alpha_out) {
  constexpr int CH = D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t l = idx / CH;
  if (l >= L) return;
  const int ch = (int)(idx % CH);
  const int64_t h = blockIdx.y, b = blockIdx.z;
  const int64_t row = (b * gridDim.y + h) * L + l;   // lse1, lse2, alpha: contiguous [B,H,L]
  float wa, wb;
  lse_combine_weights<T>(lse1[row], lse2[row], gap, wa, wb);
  if (alpha_out && ch == 0) alpha_out[row] = wa;
  const u32x4 x1 = *reinterpret_cast<const u32x4*>(out1 + 2 * (b * st.o1[0] + h * st.o1[1] + l * st.o1[2] + ch * 8));
  const u32x4 x2 = *reinterpret_cast<const u32x4*>(out2 + 2 * (b * st.o2[0] + h * st.o2[1] + l * st.o2[2] + ch * 8));
  *reinterpret_cast<u32x4*>(out + 2 * (b * st.o[0] + h * st.o[1] + l * st.o[2] + ch * 8)) =
      lse_combine_chunk<T>(x1, x2, wa, wb);
}

}  // namespace vb

extern "C" int vb_pool_kv(const void* k, const void* v, const int64_t* k_stride, const int64_t* v_stride,
                          const int32_t* rows, int B, int H, int L, int D, int gap, int dtype, void* kp, void* vp,
                          void* k_r, void* v_r, void* stream) {
  using namespace vb;
  if (!k || !v || !k_stride || !v_stride || !kp || !vp) return fail(VB_ERR_INVALID, "vb_pool_kv: null argument");
  if ((k_r == nullptr) != (v_r == nullptr)) return fail(VB_ERR_INVALID, "vb_pool_kv: give both k_r and v_r or neither");
  if (B <= 0 || H <= 0 || L <= 0 || gap <= 0 || D % 8) return fail(VB_ERR_INVALID, "vb_pool_kv: bad sizes");
  for (int i = 0; i < 3; ++i)
    if ((k_stride[i] | v_stride[i]) & 7) return fail(VB_ERR_INVALID, "vb_pool_kv: strides must be multiples of 8");
  PoolTask t{};
  t.k = reinterpret_cast<const uint8_t*>(k); t.v = reinterpret_cast<const uint8_t*>(v);
  for (int i = 0; i < 3; ++i) { t.ks[i] = k_stride[i]; t.vs[i] = v_stride[i]; }
  t.rows = rows; t.B = B; t.H = H; t.L = L; t.D = D; t.gap = gap; t.Lp = (L + gap - 1) / gap;
  t.kp = reinterpret_cast<uint8_t*>(kp); t.vp = reinterpret_cast<uint8_t*>(vp);
  t.k_r = reinterpret_cast<uint8_t*>(k_r); t.v_r = reinterpret_cast<uint8_t*>(v_r);
  const dim3 grid(pool_grid((int64_t)B * H * t.Lp * (D / 8)));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (dtype == VB_DTYPE_BF16)
    hipLaunchKernelGGL(pool_kv_kernel<BF16>, grid, dim3(256), 0, s, t);
  else if (dtype == VB_DTYPE_F16)
    hipLaunchKernelGGL(pool_kv_kernel<F16>, grid, dim3(256), 0, s, t);
  else
    return fail(VB_ERR_INVALID, "vb_pool_kv: unknown dtype");
  return check_launch("pool_kv_kernel");
}

extern "C" int vb_lse_combine(const void* out1, const float* lse1, const void* out2, const float* lse2, int B, int H,
                              int L, int D, float gap, int dtype, void* out, float* alpha, void* stream) {
  using namespace vb;
  if (!out1 || !lse1 || !out2 || !lse2 || !out) return fail(VB_ERR_INVALID, "vb_lse_combine: null argument");
  if (B <= 0 || H <= 0 || L <= 0 || D % 8) return fail(VB_ERR_INVALID, "vb_lse_combine: bad sizes");
  const int64_t rows = (int64_t)B * H * L;
  const dim3 grid((unsigned)((rows * (D / 8) + 255) / 256));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto* o1 = reinterpret_cast<const uint8_t*>(out1);
  auto* o2 = reinterpret_cast<const uint8_t*>(out2);
  auto* o = reinterpret_cast<uint8_t*>(out);
  if (dtype == VB_DTYPE_BF16)
    hipLaunchKernelGGL(lse_combine_kernel<BF16>, grid, dim3(256), 0, s, o1, lse1, o2, lse2, rows, D, gap, o, alpha);
  else if (dtype == VB_DTYPE_F16)
    hipLaunchKernelGGL(lse_combine_kernel<F16>, grid, dim3(256), 0, s, o1, lse1, o2, lse2, rows, D, gap, o, alpha);
  else
    return fail(VB_ERR_INVALID, "vb_lse_combine: unknown dtype");
  return check_launch("lse_combine_kernel");
}

extern "C" int vb_lse_combine_strided(const void* out1, const int64_t* out1_stride, const float* lse1, const void* out2,
                                      const int64_t* out2_stride, const float* lse2, int B, int H, int L, int D,
                                      float gap, int dtype, void* out, const int64_t* out_stride, float* alpha,
                                      void* stream) {
  using namespace vb;
  if (!out1 || !out1_stride || !lse1 || !out2 || !out2_stride || !lse2 || !out || !out_stride)
    return fail(VB_ERR_INVALID, "vb_lse_combine_strided: null argument");
  // H and B are grid dimensions y and z
  if (B <= 0 || H <= 0 || L <= 0 || B > 65535 || H > 65535 || (D != 64 && D != 128))
    return fail(VB_ERR_INVALID, "vb_lse_combine_strided: bad sizes (D must be 64 or 128; B, H <= 65535)");
  if (dtype != VB_DTYPE_BF16 && dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, "vb_lse_combine_strided: unknown dtype");
  const int extent[3] = {B, H, L};
  for (int i = 0; i < 3; ++i) {
    if (out1_stride[i] < 0 || out2_stride[i] < 0 || out_stride[i] < 0 ||
        ((out1_stride[i] | out2_stride[i] | out_stride[i]) & 7))
      return fail(VB_ERR_INVALID, "vb_lse_combine_strided: strides must be non-negative multiples of 8 elements");
    // a zero stride repeats an input; on the output it would make two rows one
    if (extent[i] > 1 && out_stride[i] == 0)
      return fail(VB_ERR_INVALID, "vb_lse_combine_strided: out's rows must be distinct (a stride of 0)");
  }
  if (((uintptr_t)out1 | (uintptr_t)out2 | (uintptr_t)out) & 15)
    return fail(VB_ERR_INVALID, "vb_lse_combine_strided: tensors must be 16-byte aligned");
  if (out == out1 || out == out2) return fail(VB_ERR_INVALID, "vb_lse_combine_strided: out may not overlap the inputs");
  CombineStrides st;
  for (int i = 0; i < 3; ++i) { st.o1[i] = out1_stride[i]; st.o2[i] = out2_stride[i]; st.o[i] = out_stride[i]; }
  const dim3 grid((unsigned)(((int64_t)L * (D / 8) + 255) / 256), (unsigned)H, (unsigned)B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  auto* o1 = reinterpret_cast<const uint8_t*>(out1);
  auto* o2 = reinterpret_cast<const uint8_t*>(out2);
  auto* o = reinterpret_cast<uint8_t*>(out);
#define VB_COMBINE_STRIDED(T, DD) \
  hipLaunchKernelGGL((lse_combine_strided_kernel<T, DD>), grid, dim3(256), 0, s, o1, lse1, o2, lse2, st, L, gap, o, alpha)
  if (dtype == VB_DTYPE_BF16) {
    if (D == 64) VB_COMBINE_STRIDED(BF16, 64); else VB_COMBINE_STRIDED(BF16, 128);
  } else {
    if (D == 64) VB_COMBINE_STRIDED(F16, 64); else VB_COMBINE_STRIDED(F16, 128);
  }
#undef VB_COMBINE_STRIDED
  return check_launch("lse_combine_strided_kernel");
}
