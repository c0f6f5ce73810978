// Mask predictor, second block score: the sampled softmax mass per (q-block, key-block) pair
// (include/vblade.h, vb_mask_scores_mass), beside the max proxy of vb_predict.hip. The sampled streams
// are the max predictor's; only the score differs.
//
//   mass_gather_kernel   the sampled q and k rows (32 per 128-token block, through `rows`, the
//                        replicate pad as a clamp) copied into two contiguous workspace streams
//                        [B*H][nb*32][D], 16 bytes per thread, so the score loop streams 32-row tiles.
//   mass_score_kernel    one wave per PAIR of q-blocks (2 x 32 sampled queries); it walks the 32-key
//                        tiles, one key block each, twice. S^T = K * Q^T (v_mfma_f32_32x32x16): a lane
//                        owns one query per q-block and 16 of the tile's 32 keys, its partner lane ^ 32
//                        the other 16, so a per-query reduction is in-lane plus one permlane32_swap.
//                        Pass 1: per lane the running maximum and the sum of exp2 relative to it over
//                        its half of every tile; the halves are joined once, after the last tile. A
//                        score minus the maximum is ONE v_fma_f32 of the accumulator, qk_scale and -M
//                        (the kernel is bound by vector issue: 16 exp2 and ~45 plain operations per
//                        32x32 tile against four or eight MFMAs).
//                        Pass 2: the tile again, exp2(s - M_r), the lane's 16 values, the partner's,
//                        one product with 1/l_r, the 32 queries by four v_add_f32_dpp and one
//                        v_permlane16_swap; lane j % 64 keeps tile j's total and the wave stores 64
//                        block masses at a time.
//                        The four waves of a workgroup (eight q-blocks) share every K tile through
//                        LDS, copied one tile ahead; one barrier per tile.
//   mass_norm_kernel     one wave per row of mass: the row sum (per lane over j = lane, lane + 64, ...,
//                        then a butterfly over the 64 lanes) and po = storage(mass / sum).
//
// No launch allocates or synchronises; no floating-point atomics; three launches on the caller's stream.
#include <cmath>
#include <string>

#include "vb_common.hpp"

namespace vb {
namespace {

constexpr int kBlock = 128;        // tokens per mask block
constexpr int kKeep = 32;          // sampled tokens per block: one MFMA tile
constexpr int kMaxBlocks = 1024;   // L <= 131072
constexpr int kQT = 2;             // q-blocks per wave
constexpr int kScoreWaves = 4;
constexpr int kNormWaves = 4;
constexpr int kGatherThreads = 256;

struct MassParams {
  const void* q; const void* k;
  int64_t qs[3], ks[3];
  const int32_t* rows; const int32_t* q_off; const int32_t* k_off;
  int B, H, L, D, nb;
  float c;          // fp32(scale) * fp32(1.44269504)
  void* qstream;    // workspace [B*H][nb*32][D] storage dtype
  void* kstream;
  float* mass;      // [B*H][nb][nb]: the caller's, or the workspace's
  void* po;
};

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// x + the value of the lane a DPP control pairs this lane with (one v_add_f32_dpp, no LDS)
template <int kCtrl>
__device__ __forceinline__ float add_dpp(float x) {
  const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), kCtrl, 0xf, 0xf, false);
  return x + __int_as_float(y);
}
// the sum over the 32 lanes of a half-wave, the same bits in each of them: pairs (quad_perm [1,0,3,2]),
// quads ([2,3,0,1]), the two quads of eight lanes (row_half_mirror: every lane of a quad already holds
// the quad's sum), the two eights of a row (row_mirror), the two rows (v_permlane16_swap). Each step
// adds two values in either order, so the order of the sum is fixed by the lane numbers alone.
__device__ __forceinline__ float sum_half(float x) {
  x = add_dpp<0xB1>(x);
  x = add_dpp<0x4E>(x);
  x = add_dpp<0x141>(x);
  x = add_dpp<0x140>(x);
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ------------------------------------------------------------------------------------------ gather
// grid (chunks of a head's stream / 256, B*H, 2): z = 0 the queries, 1 the keys
__global__ void __launch_bounds__(kGatherThreads) mass_gather_kernel(const MassParams p) {
  const int per_row = p.D / 8;                 // 16-byte chunks per row
  const int n = p.nb * kKeep * per_row;        // <= 1024 * 32 * 16
  const int idx = blockIdx.x * kGatherThreads + threadIdx.x;
  if (idx >= n) return;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const bool keys = blockIdx.z != 0;
  const int srow = idx / per_row, ch = idx - srow * per_row;
  const int blk = srow / kKeep, t = srow - blk * kKeep;
  const int off = clampi((keys ? p.k_off : p.q_off)[(int64_t)bh * kKeep + t], 0, kBlock - 1);
  int pos = blk * kBlock + off;
  pos = pos < p.L - 1 ? pos : p.L - 1;         // replicate padding
  if (p.rows) pos = clampi(p.rows[pos], 0, p.L - 1);
  const int64_t* st = keys ? p.ks : p.qs;
  const uint16_t* src = reinterpret_cast<const uint16_t*>(keys ? p.k : p.q) + b * st[0] + h * st[1] +
                        (int64_t)pos * st[2] + 8 * ch;
  uint16_t* dst = reinterpret_cast<uint16_t*>(keys ? p.kstream : p.qstream) +
                  ((int64_t)bh * p.nb * kKeep + srow) * p.D + 8 * ch;
  *reinterpret_cast<u32x4*>(dst) = *reinterpret_cast<const u32x4*>(src);
}

// ------------------------------------------------------------------------------------------ scores
// One workgroup = kScoreWaves waves = kScoreWaves * kQT consecutive q-blocks of one head. The waves share
// every 32-key tile through LDS (two buffers, rows padded by 16 bytes): each thread copies 16 or 32
// bytes of the next tile global -> registers -> LDS while the workgroup computes on the current one, one
// barrier per tile. Read straight from L2 by every wave the K stream bounds the kernel (every wave of a
// head reads the whole stream: 3.8 GB per CogVideoX call); shared, it is read once per workgroup.
template <class T, int D>
__global__ void __launch_bounds__(64 * kScoreWaves) mass_score_kernel(const MassParams p) {
  using vec8 = typename T::vec8;
  using raw = typename T::raw;
  constexpr int kSteps = D / 16;
  constexpr int kRowB = D * 2 + 16;                                   // padded LDS row, bytes
  constexpr int kChunks = kKeep * (D / 8) / (64 * kScoreWaves);       // 16-byte chunks per thread and tile
  static_assert(kKeep * (D / 8) % (64 * kScoreWaves) == 0, "a tile divides over the workgroup");
  __shared__ __attribute__((aligned(16))) uint8_t tile[2][kKeep * kRowB];
  const int bh = blockIdx.y;
  const int tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
  const int r32 = lane & 31, half = lane >> 5;
  const int nb = p.nb;
  const int i0 = (blockIdx.x * kScoreWaves + wave) * kQT;   // the wave's first q-block; may lie past the
                                                            // last: the wave then computes on the last
                                                            // q-block and stores nothing (it still
                                                            // copies its share of every tile)
  const int64_t head = (int64_t)bh * nb * kKeep * D;
  const raw* qb = reinterpret_cast<const raw*>(p.qstream) + head;
  const raw* kb = reinterpret_cast<const raw*>(p.kstream) + head;

  // the queries as MFMA B operands: lane (r32, half) holds query r32 of q-block i0 + t, d = 16*step +
  // 8*half ..+7. A q-block past the last repeats the last (computed, never stored).
  vec8 qf[kQT][kSteps];
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
    const int i = i0 + t < nb ? i0 + t : nb - 1;
    const raw* src = qb + ((int64_t)i * kKeep + r32) * D + 8 * half;
#pragma unroll
    for (int st = 0; st < kSteps; ++st) qf[t][st] = *reinterpret_cast<const vec8*>(src + 16 * st);
  }
  // this thread's chunks of a tile: chunk c = tid + 256 * u is row c / (D/8), 16-byte column c % (D/8);
  // a tile is kKeep * D contiguous elements of the stream, so chunk c lies at element 8 * c
  u32x4 stage[kChunks];
  auto fetch = [&](int j) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kChunks; ++u)
      stage[u] = *reinterpret_cast<const u32x4*>(kb + (int64_t)j * kKeep * D + 8 * (tid + 64 * kScoreWaves * u));
  };
  auto put = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < kChunks; ++u) {
      const int c = tid + 64 * kScoreWaves * u;
      *reinterpret_cast<u32x4*>(&tile[buf][(c / (D / 8)) * kRowB + (c % (D / 8)) * 16]) = stage[u];
    }
  };
  // the keys as MFMA A operands: lane (r32, half) reads key r32 of the tile, d = 16*step + 8*half ..+7
  const int frag = r32 * kRowB + 16 * half;
  auto keys = [&](int buf, vec8* kf) __attribute__((always_inline)) {
#pragma unroll
    for (int st = 0; st < kSteps; ++st) kf[st] = *reinterpret_cast<const vec8*>(&tile[buf][frag + 32 * st]);
  };

  // C layout of K * Q^T: column (query) = lane & 31, row (key) = (reg & 3) + 8 * (reg >> 2) + 4 * half
  // ---- pass 1: per lane, over its 16 keys of every tile, the running maximum and the sum relative to it
  float M[kQT], l[kQT];
#pragma unroll
  for (int t = 0; t < kQT; ++t) { M[t] = -INFINITY; l[t] = 0.f; }
  fetch(0);
  put(0);
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    if (j + 1 < nb) fetch(j + 1);   // uniform
    vec8 kf[kSteps];
    keys(j & 1, kf);
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
      f32x16 acc = {};
#pragma unroll
      for (int st = 0; st < kSteps; ++st) acc = T::mfma32(kf[st], qf[t][st], acc);
      // qk_scale > 0 and rounding is monotonic: the maximum of the products is the product of the maximum
      float m = acc[0];
#pragma unroll
      for (int reg = 1; reg < 16; ++reg) m = fmaxf(m, acc[reg]);
      m = fmaxf(m * p.c, M[t]);
      float e = exp2_fast(fmaf(acc[0], p.c, -m));
#pragma unroll
      for (int reg = 1; reg < 16; ++reg) e += exp2_fast(fmaf(acc[reg], p.c, -m));
      l[t] = l[t] * exp2_fast(M[t] - m) + e;   // the first tile: 0 * exp2(-inf) = 0
      M[t] = m;
    }
    // the other buffer was last read before the previous barrier; this one is read until the next
    if (j + 1 < nb) put((j + 1) & 1);
    __syncthreads();
  }
  // the two halves of each query joined: a symmetric combine, both lanes hold the same bits
  float inv_l[kQT];
#pragma unroll
  for (int t = 0; t < kQT; ++t) {
    const float m = max_xor32(M[t]);
    const float lt = add_xor32(l[t] * exp2_fast(M[t] - m));
    M[t] = m;
    inv_l[t] = 1.0f / lt;   // lt is 1 or more up to rounding: the row's largest term is exp2(~0)
  }

  // ---- pass 2: the block masses. Lane j % 64 keeps tile j's total; 64 of them leave in one store.
  float keep[kQT];
#pragma unroll
  for (int t = 0; t < kQT; ++t) keep[t] = 0.f;
  const int irow = i0 < nb ? i0 : nb - 1;
  float* mrow = p.mass + ((int64_t)bh * nb + irow) * nb;   // row i0; row i0 + 1 follows at + nb
  fetch(0);
  put(0);   // every wave passed pass 1's last barrier after its last read of either buffer
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    if (j + 1 < nb) fetch(j + 1);
    vec8 kf[kSteps];
    keys(j & 1, kf);
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
      f32x16 acc = {};
#pragma unroll
      for (int st = 0; st < kSteps; ++st) acc = T::mfma32(kf[st], qf[t][st], acc);
      float e = exp2_fast(fmaf(acc[0], p.c, -M[t]));
#pragma unroll
      for (int reg = 1; reg < 16; ++reg) e += exp2_fast(fmaf(acc[reg], p.c, -M[t]));
      e = add_xor32(e) * inv_l[t];   // query r32's share of key block j
      e = sum_half(e);               // over the 32 queries: both halves hold them all
      if (lane == (j & 63)) keep[t] = e;
    }
    if ((j & 63) == 63 || j == nb - 1) {
      const int c = (j & ~63) + lane;
#pragma unroll
      for (int t = 0; t < kQT; ++t)
        if (c <= j && i0 + t < nb) mrow[(int64_t)t * nb + c] = keep[t];
    }
    if (j + 1 < nb) put((j + 1) & 1);
    __syncthreads();
  }
}

// -------------------------------------------------------------------------------------------- norm
template <class T>
__global__ void __launch_bounds__(64 * kNormWaves) mass_norm_kernel(const MassParams p) {
  const int row = blockIdx.x * kNormWaves + (threadIdx.x >> 6);   // row of one head's [nb][nb]
  const int bh = blockIdx.y, lane = lane_id();
  if (row >= p.nb) return;
  const int64_t base = ((int64_t)bh * p.nb + row) * p.nb;
  const float* m = p.mass + base;
  float s = 0.f;
  for (int c = lane; c < p.nb; c += 64) s += m[c];
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
  typename T::raw* out = reinterpret_cast<typename T::raw*>(p.po) + base;
  for (int c = lane; c < p.nb; c += 64) out[c] = T::from_f32(m[c] / s);
}

int blocks_of(const vb_mass_scores_args* a) { return (a->L + kBlock - 1) / kBlock; }

// bytes of one gathered stream (all heads), a multiple of 16
uint64_t stream_bytes(const vb_mass_scores_args* a) {
  return (uint64_t)a->B * a->H * (uint64_t)blocks_of(a) * kKeep * (uint64_t)a->D * 2;
}

template <class T>
const void* score_kernel(int D) {
  return D == 64 ? reinterpret_cast<const void*>(mass_score_kernel<T, 64>)
                 : reinterpret_cast<const void*>(mass_score_kernel<T, 128>);
}

}  // namespace
}  // namespace vb

extern "C" uint64_t vb_mask_scores_mass_workspace_size(const vb_mass_scores_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->L <= 0 || a->D <= 0) return 0;
  const uint64_t nb = (uint64_t)vb::blocks_of(a);
  const uint64_t bytes = 2 * vb::stream_bytes(a) + (uint64_t)a->B * a->H * nb * nb * 4;
  return (bytes + 15) & ~uint64_t(15);
}

extern "C" int vb_mask_scores_mass(const vb_mass_scores_args* a, void* stream) {
  using namespace vb;
  const std::string fn = "vb_mask_scores_mass: ";
  if (!a || !a->q || !a->k || !a->q_off || !a->k_off || !a->po) return fail(VB_ERR_INVALID, fn + "null argument");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (a->block != kBlock || a->num_keep != kKeep)
    return fail(VB_ERR_UNSUPPORTED, fn + "block must be 128 and num_keep 32: the mass score is built for 32 sampled "
                                         "tokens per block only, 16 and 64 are vb_mask_predict's (got block " +
                                        std::to_string(a->block) + ", num_keep " + std::to_string(a->num_keep) + ")");
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, fn + "unknown dtype");
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, fn + "head_dim must be 64 or 128");
  const int nb = blocks_of(a);
  if (nb > kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, fn + "sequence too long (L <= 131072)");
  for (int i = 0; i < 3; ++i)
    if (((a->q_stride[i] | a->k_stride[i]) & 7) || a->q_stride[i] < 0 || a->k_stride[i] < 0)
      return fail(VB_ERR_INVALID, fn + "q/k strides must be non-negative multiples of 8");
  if ((int64_t)(a->L - 1) * a->q_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31) ||
      (int64_t)(a->L - 1) * a->k_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31))
    return fail(VB_ERR_UNSUPPORTED, fn + "a q/k (b,h) slice spans >= 2 GiB");
  if ((reinterpret_cast<uintptr_t>(a->q) | reinterpret_cast<uintptr_t>(a->k)) & 15)
    return fail(VB_ERR_INVALID, fn + "q and k must be 16-byte aligned");
  if ((int64_t)a->B * a->H > 65535) return fail(VB_ERR_UNSUPPORTED, fn + "B*H must be <= 65535");
  const uint64_t need = vb_mask_scores_mass_workspace_size(a);
  if (!a->workspace || a->workspace_bytes < need || (reinterpret_cast<uintptr_t>(a->workspace) & 15))
    return fail(VB_ERR_INVALID, fn + "workspace missing or smaller than vb_mask_scores_mass_workspace_size() (" +
                                    std::to_string(need) + " bytes)");
  MassParams p{};
  p.q = a->q; p.k = a->k;
  for (int i = 0; i < 3; ++i) { p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; }
  p.rows = a->rows; p.q_off = a->q_off; p.k_off = a->k_off;
  p.B = a->B; p.H = a->H; p.L = a->L; p.D = a->D; p.nb = nb;
  const float scale = a->scale > 0.f ? a->scale : (float)(1.0 / sqrt((double)a->D));
  p.c = scale * 1.44269504f;
  uint8_t* ws = reinterpret_cast<uint8_t*>(a->workspace);
  p.qstream = ws;
  p.kstream = ws + stream_bytes(a);
  p.mass = a->mass ? a->mass : reinterpret_cast<float*>(ws + 2 * stream_bytes(a));
  p.po = a->po;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  void* params[] = {&p};
  const unsigned bh = (unsigned)(a->B * a->H);
  const unsigned chunks = (unsigned)(nb * kKeep * (a->D / 8));
  (void)hipLaunchKernel(reinterpret_cast<const void*>(mass_gather_kernel),
                        dim3((chunks + kGatherThreads - 1) / kGatherThreads, bh, 2), dim3(kGatherThreads), params, 0, s);
  if (int rc = check_launch("mass_gather_kernel")) return rc;
  const unsigned waves = (unsigned)((nb + kQT - 1) / kQT);
  const void* score = a->dtype == VB_DTYPE_BF16 ? score_kernel<BF16>(a->D) : score_kernel<F16>(a->D);
  (void)hipLaunchKernel(score, dim3((waves + kScoreWaves - 1) / kScoreWaves, bh), dim3(64 * kScoreWaves), params, 0, s);
  if (int rc = check_launch("mass_score_kernel")) return rc;
  const void* norm = a->dtype == VB_DTYPE_BF16 ? reinterpret_cast<const void*>(mass_norm_kernel<BF16>)
                                               : reinterpret_cast<const void*>(mass_norm_kernel<F16>);
  (void)hipLaunchKernel(norm, dim3((unsigned)((nb + kNormWaves - 1) / kNormWaves), bh), dim3(64 * kNormWaves), params, 0, s);
  return check_launch("mass_norm_kernel");
}
