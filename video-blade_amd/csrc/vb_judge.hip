// Head-adaptive retain budgets: the judge_sparsity estimator (cogvideox/train/special_attentions_local/
// TrainRelated/blocksparseattn.py:147-160) and the budget rule of the reference's commented-out lines
// (cogvideo_blocksparseattn.py:344-348), on the device.
//
//   judge_score_kernel   S sampled query rows (padded to the 32-row MFMA tile) against every
//                        key_stride-th key: scale*log2(e)*<q,k> in fp32, staged in the workspace as
//                        [B*H][S][n padded to 4]. One wave per 32-key tile, operands read in place from the
//                        strided tensors (16 bytes per lane and k-step), no LDS.
//   judge_select_kernel  one workgroup per staged row: row maximum, then the top_n-th largest
//                        e_j = exp2(t_j - max) by a radix-256 selection over the fp32 bit patterns
//                        (order-preserving for e >= 0; integer LDS histograms, so no
//                        floating-point atomics), then
//                        mass = (sum(e > t) + (top_n - #(e > t)) * t) / sum(e). The row is re-read
//                        from the workspace (L2) by each of the six passes, 16 bytes per thread
//                        and load, and e recomputed (the same bits each time). Every sum runs in
//                        an order fixed by n alone. The workgroup that finishes a (b,h)'s last row
//                        (an integer ticket in the workspace) sums the S masses in row order.
//   head_budget_kernel   sparsity [B,H] -> max_keep [B,H]: one workgroup, float64.
//
// No launch allocates or synchronises; three launches for the two entries together.
#include <cmath>
#include <string>

#include "vb_common.hpp"

namespace vb {
namespace {

constexpr int kKeyTile = 32;        // keys per MFMA tile (one wave)
constexpr int kScoreWaves = 4;
constexpr int kTilesPerWave = 4;
constexpr int kKeyChunk = kKeyTile * kScoreWaves * kTilesPerWave;   // keys per score workgroup: 512
constexpr int kMaxSamples = 64;
constexpr int kSelectWaves = 4;

struct JudgeParams {
  const void* q; const void* k;
  int64_t qs[3], ks[3];
  const int32_t* rows;
  int B, H, L, D, S, key_stride, n, top_n;
  int n_pad;            // row stride of the staged scores: n rounded up to four floats
  float c;              // scale * log2(e)
  float* scores;        // workspace [B*H][S][n_pad]
  float* mass;          // workspace [B*H][S]: the rows' masses, for the last workgroup of a (b,h)
  int* ticket;          // workspace [B*H]: finished rows per (b,h); zeroed by the score launch
  float* sparsity; float* row_mass;
};

// ------------------------------------------------------------------------------------------ scores
template <class T, int D>
__global__ void __launch_bounds__(64 * kScoreWaves) judge_score_kernel(const JudgeParams p) {
  using vec8 = typename T::vec8;
  constexpr int kSteps = D / 16;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int r32 = lane & 31, half = lane >> 5;
  const typename T::raw* qb = reinterpret_cast<const typename T::raw*>(p.q) + b * p.qs[0] + h * p.qs[1];
  const typename T::raw* kb = reinterpret_cast<const typename T::raw*>(p.k) + b * p.ks[0] + h * p.ks[1];
  const bool two = p.S > 32;   // uniform: a second 32-row tile of samples

  // the sampled q rows as MFMA A operands: lane (r32, half) holds row r32 (+32), d = 16*step + 8*half ..+7.
  // Rows past S repeat row S-1 (their scores are never stored); row numbers are clamped to [0, L-1].
  vec8 qa[2][kSteps];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    if (t == 1 && !two) break;
    int s = r32 + 32 * t;
    s = s < p.S ? s : p.S - 1;
    int row = p.rows[s];
    row = row < 0 ? 0 : (row > p.L - 1 ? p.L - 1 : row);
    const typename T::raw* src = qb + (int64_t)row * p.qs[2] + 8 * half;
#pragma unroll
    for (int st = 0; st < kSteps; ++st) qa[t][st] = *reinterpret_cast<const vec8*>(src + 16 * st);
  }

  if (blockIdx.x == 0 && threadIdx.x == 0) p.ticket[bh] = 0;   // for the select launch behind this one
  const int first = blockIdx.x * (kScoreWaves * kTilesPerWave);
  float* out = p.scores + (int64_t)bh * p.S * p.n_pad;
#pragma unroll 1
  for (int i = 0; i < kTilesPerWave; ++i) {
    const int j0 = (first + wave + kScoreWaves * i) * kKeyTile;
    if (j0 >= p.n) break;   // uniform per wave
    int j = j0 + r32;
    const bool live = j < p.n;
    j = live ? j : p.n - 1;   // j * key_stride <= L - 1 for every j < n = ceil(L / key_stride)
    const typename T::raw* src = kb + (int64_t)j * p.key_stride * p.ks[2] + 8 * half;
    vec8 kf[kSteps];
#pragma unroll
    for (int st = 0; st < kSteps; ++st) kf[st] = *reinterpret_cast<const vec8*>(src + 16 * st);
    f32x16 acc0 = {}, acc1 = {};
#pragma unroll
    for (int st = 0; st < kSteps; ++st) acc0 = T::mfma32(qa[0][st], kf[st], acc0);
    if (two) {
#pragma unroll
      for (int st = 0; st < kSteps; ++st) acc1 = T::mfma32(qa[1][st], kf[st], acc1);
    }
    // C layout: column (key) = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    if (live) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int s = (reg & 3) + 8 * (reg >> 2) + 4 * half;
        if (s < p.S) out[(int64_t)s * p.n_pad + j] = acc0[reg] * p.c;
        if (two && s + 32 < p.S) out[(int64_t)(s + 32) * p.n_pad + j] = acc1[reg] * p.c;
      }
    }
  }
}

// --------------------------------------------------------------------------------------- selection
// fixed-order wave reductions (xor butterflies: every lane ends with the same bits)
__device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m, 64));
  return x;
}
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
  return x;
}

// every element of a staged row, four per load (rows start 16-byte aligned and are padded to a
// multiple of four floats; the padding is never written, so it is masked by index): thread t visits
// vectors t, t + 256, ... and the four elements of each in order, the same order in every pass
template <class F>
__device__ __forceinline__ void for_row(const float* t, int n, F f) {
  const f32x4* t4 = reinterpret_cast<const f32x4*>(t);
  const int n4 = (n + 3) >> 2;
#pragma unroll 2
  for (int i = threadIdx.x; i < n4; i += 64 * kSelectWaves) {
    const f32x4 x = t4[i];
    const int j = 4 * i;
    f(x[0]);
    if (j + 1 < n) f(x[1]);
    if (j + 2 < n) f(x[2]);
    if (j + 3 < n) f(x[3]);
  }
}

// the waves' partial results combined in wave order (every thread gets the same bits); `slot` is
// one of two LDS arrays used in turn, so one barrier per call is enough
__device__ __forceinline__ float block_sum(float x, float* slot, int wave, int lane) {
  x = wave_sum(x);
  if (lane == 0) slot[wave] = x;
  __syncthreads();
  float s = slot[0];
  for (int w = 1; w < kSelectWaves; ++w) s += slot[w];
  return s;
}

// One workgroup per staged row. The workgroup that finishes a (b,h)'s last row (a ticket counter,
// zeroed by the score launch) adds the S row masses up in row order: which workgroup that is never
// changes the bits.
__global__ void __launch_bounds__(64 * kSelectWaves) judge_select_kernel(const JudgeParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t hist[256];
  __shared__ float part[2][kSelectWaves];
  __shared__ int parti[kSelectWaves];
  const int r = blockIdx.x, bh = blockIdx.y;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int n = p.n, top_n = p.top_n;
  const float* t = p.scores + ((int64_t)bh * p.S + r) * p.n_pad;

  float m = -INFINITY;
  for_row(t, n, [&](float x) { m = fmaxf(m, x); });
  m = wave_max(m);
  if (lane == 0) part[0][wave] = m;
  __syncthreads();
  m = part[0][0];
  for (int w = 1; w < kSelectWaves; ++w) m = fmaxf(m, part[0][w]);

  // the top_n-th largest e, eight bits of its pattern per pass, most significant first; the
  // first pass also sums e
  float sum = 0.f;
  uint32_t prefix = 0;
  int need = top_n;
#pragma unroll 1
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[threadIdx.x] = 0;
    __syncthreads();
    // a thread adds a run of equal bins at once: a softmax row puts most of its elements in very
    // few bins (the underflowed tail in bin 0 of every pass), and many lanes adding 1 to one LDS
    // address serialise
    int cur = 0, run = 0;
    auto count = [&](int b) {
      if (b != cur) {
        if (run) atomicAdd(&hist[cur], (uint32_t)run);
        cur = b;
        run = 0;
      }
      ++run;
    };
    if (shift == 24) {
      for_row(t, n, [&](float x) {
        const float e = exp2_fast(x - m);
        sum += e;
        count((int)(__float_as_uint(e) >> 24));
      });
    } else {
      const uint32_t hi = prefix >> (shift + 8);
      for_row(t, n, [&](float x) {
        const uint32_t u = __float_as_uint(exp2_fast(x - m));
        if ((u >> (shift + 8)) == hi) count((int)((u >> shift) & 255u));
      });
    }
    if (run) atomicAdd(&hist[cur], (uint32_t)run);
    __syncthreads();
    // the bin that holds the need-th largest: lane l takes bins 4l .. 4l+3, a suffix sum over the
    // lanes finds the lane, that lane walks its four bins from the top (every wave does the same)
    const u32x4 c4 = *reinterpret_cast<const u32x4*>(&hist[4 * lane]);
    const int own = (int)(c4[0] + c4[1] + c4[2] + c4[3]);
    int suffix = own;   // bins of lanes >= l
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_down(suffix, d, 64);
      if (lane + d < 64) suffix += v;
    }
    int above = suffix - own, bin = 0;
    const bool mine = above < need && need <= suffix;
    if (mine) {
      bin = 4 * lane + 3;
      for (int k = 3; k > 0; --k) {
        if (above + (int)c4[k] >= need) break;
        above += (int)c4[k];
        --bin;
      }
    }
    const int src = __ffsll((unsigned long long)__ballot(mine)) - 1;   // exactly one lane
    bin = __shfl(bin, src, 64);
    above = __shfl(above, src, 64);
    need -= above;
    prefix |= (uint32_t)bin << shift;
    __syncthreads();
  }
  sum = block_sum(sum, part[1], wave, lane);
  const float thr = __uint_as_float(prefix);
  float gs = 0.f;
  int gc = 0;
  for_row(t, n, [&](float x) {
    const float e = exp2_fast(x - m);
    if (e > thr) { gs += e; ++gc; }
  });
  gs = block_sum(gs, part[0], wave, lane);
  gc = wave_sum(gc);
  if (lane == 0) parti[wave] = gc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  gc = 0;
  for (int w = 0; w < kSelectWaves; ++w) gc += parti[w];
  const float v = (gs + (float)(top_n - gc) * thr) / sum;
  if (p.row_mass) p.row_mass[(int64_t)bh * p.S + r] = v;
  // publish the row's mass, then draw a ticket; the drawer of the last one sums the S masses
  float* mass = p.mass + (int64_t)bh * p.S;
  __hip_atomic_store(&mass[r], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const int ticket = __hip_atomic_fetch_add(&p.ticket[bh], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ticket != p.S - 1) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float s = 0.f;
  for (int i = 0; i < p.S; ++i) s += __hip_atomic_load(&mass[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  p.sparsity[bh] = s / (float)p.S;
}

// ------------------------------------------------------------------------------------------ budget
struct BudgetParams {
  const float* sparsity;
  int count, nb, arith;
  double base, lo, hi;
  int32_t* max_keep; float* ratio;
};

__global__ void __launch_bounds__(256) head_budget_kernel(const BudgetParams p) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < p.count; i += 256) s += (double)p.sparsity[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  const double mean = part[0] / (double)p.count;
  for (int i = threadIdx.x; i < p.count; i += 256) {
    double ratio = p.base * ((double)p.sparsity[i] / mean);
    ratio = ratio > p.lo ? ratio : p.lo;
    ratio = ratio < p.hi ? ratio : p.hi;
    int c = p.arith == 0 ? (int)((float)p.nb * (float)ratio) : (int)((double)p.nb * ratio);
    p.max_keep[i] = c > 1 ? c : 1;
    if (p.ratio) p.ratio[i] = (float)ratio;
  }
}

int keys_of(const vb_judge_args* a) { return (a->L + a->key_stride - 1) / a->key_stride; }
int padded(int n) { return (n + 3) & ~3; }

}  // namespace
}  // namespace vb

extern "C" uint64_t vb_judge_sparsity_workspace_size(const vb_judge_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->L <= 0 || a->S <= 0 || a->key_stride <= 0) return 0;
  // the staged scores, the row masses, the ticket counters
  const uint64_t bh = (uint64_t)a->B * a->H;
  const uint64_t words = bh * a->S * (uint64_t)vb::padded(vb::keys_of(a)) + bh * a->S + bh;
  return (words * 4 + 15) & ~uint64_t(15);
}

extern "C" int vb_judge_sparsity(const vb_judge_args* a, void* stream) {
  using namespace vb;
  const std::string fn = "vb_judge_sparsity: ";
  if (!a || !a->q || !a->k || !a->rows || !a->sparsity) return fail(VB_ERR_INVALID, fn + "null argument");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (a->L > 131072) return fail(VB_ERR_UNSUPPORTED, fn + "sequence too long (L <= 131072)");
  if (a->S < 1 || a->S > kMaxSamples) return fail(VB_ERR_INVALID, fn + "S must be in [1, 64]");
  if (a->key_stride < 1) return fail(VB_ERR_INVALID, fn + "key_stride must be >= 1");
  const int n = keys_of(a);
  if (a->top_n < 1 || a->top_n > n)
    return fail(VB_ERR_INVALID, fn + "top_n must be in [1, n = " + std::to_string(n) + "]");
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, fn + "unknown dtype");
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, fn + "head_dim must be 64 or 128");
  if ((int64_t)(a->L - 1) * a->q_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31) ||
      (int64_t)(a->L - 1) * a->k_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31))
    return fail(VB_ERR_UNSUPPORTED, fn + "a q/k (b,h) slice spans >= 2 GiB");
  for (int i = 0; i < 3; ++i)
    if (((a->q_stride[i] | a->k_stride[i]) & 7) || a->q_stride[i] < 0 || a->k_stride[i] < 0)
      return fail(VB_ERR_INVALID, fn + "strides must be non-negative multiples of 8");
  if ((reinterpret_cast<uintptr_t>(a->q) | reinterpret_cast<uintptr_t>(a->k)) & 15)
    return fail(VB_ERR_INVALID, fn + "q and k must be 16-byte aligned");
  const uint64_t need = vb_judge_sparsity_workspace_size(a);
  if (!a->workspace || a->workspace_bytes < need || (reinterpret_cast<uintptr_t>(a->workspace) & 15))
    return fail(VB_ERR_INVALID, fn + "workspace missing or smaller than vb_judge_sparsity_workspace_size() (" +
                                    std::to_string(need) + " bytes)");
  JudgeParams p{};
  p.q = a->q; p.k = a->k;
  for (int i = 0; i < 3; ++i) { p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; }
  p.rows = a->rows;
  p.B = a->B; p.H = a->H; p.L = a->L; p.D = a->D; p.S = a->S;
  p.key_stride = a->key_stride; p.n = n; p.top_n = a->top_n; p.n_pad = padded(n);
  const float scale = a->scale > 0.f ? a->scale : (float)(1.0 / sqrt((double)a->D));
  p.c = scale * kLog2e;
  p.scores = reinterpret_cast<float*>(a->workspace);
  p.mass = p.scores + (int64_t)a->B * a->H * a->S * p.n_pad;
  p.ticket = reinterpret_cast<int*>(p.mass + (int64_t)a->B * a->H * a->S);
  p.sparsity = a->sparsity; p.row_mass = a->row_mass;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const void* kernel =
      a->dtype == VB_DTYPE_BF16
          ? (a->D == 64 ? reinterpret_cast<const void*>(judge_score_kernel<BF16, 64>)
                        : reinterpret_cast<const void*>(judge_score_kernel<BF16, 128>))
          : (a->D == 64 ? reinterpret_cast<const void*>(judge_score_kernel<F16, 64>)
                        : reinterpret_cast<const void*>(judge_score_kernel<F16, 128>));
  void* params[] = {&p};
  const unsigned chunks = (unsigned)((n + kKeyChunk - 1) / kKeyChunk);
  (void)hipLaunchKernel(kernel, dim3(chunks, (unsigned)(a->B * a->H)), dim3(64 * kScoreWaves), params, 0, s);
  if (int rc = check_launch("judge_score_kernel")) return rc;
  (void)hipLaunchKernel(reinterpret_cast<const void*>(judge_select_kernel), dim3((unsigned)a->S, (unsigned)(a->B * a->H)),
                        dim3(64 * kSelectWaves), params, 0, s);
  return check_launch("judge_select_kernel");
}

extern "C" int vb_head_budget(const float* sparsity, int B, int H, int nb, double base, double lo, double hi,
                              int arith, int32_t* max_keep, float* ratio, void* stream) {
  using namespace vb;
  const std::string fn = "vb_head_budget: ";
  if (!sparsity || !max_keep) return fail(VB_ERR_INVALID, fn + "null argument");
  if (B <= 0 || H <= 0 || nb < 1) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (!(base > 0.0) || !std::isfinite(base)) return fail(VB_ERR_INVALID, fn + "base must be positive and finite");
  if (!(lo <= hi) || !std::isfinite(lo) || !std::isfinite(hi))
    return fail(VB_ERR_INVALID, fn + "the clamp needs finite lo <= hi");
  if (arith != 0 && arith != 1) return fail(VB_ERR_INVALID, fn + "arith must be 0 (cog) or 1 (wan)");
  if ((int64_t)B * H > (int64_t(1) << 24)) return fail(VB_ERR_UNSUPPORTED, fn + "more than 2^24 heads");
  BudgetParams p{sparsity, B * H, nb, arith, base, lo, hi, max_keep, ratio};
  void* params[] = {&p};
  (void)hipLaunchKernel(reinterpret_cast<const void*>(head_budget_kernel), dim3(1), dim3(256), params, 0,
                        reinterpret_cast<hipStream_t>(stream));
  return check_launch("head_budget_kernel");
}
