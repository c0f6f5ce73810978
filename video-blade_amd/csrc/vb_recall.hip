// Attention-recall probe: the exact softmax mass a block mask keeps, for a handful of probe queries
// per head, and the best mass any mask with as many blocks could have kept (include/vblade.h,
// vb_mask_recall). The sibling of the judge_sparsity estimator (vb_judge.hip): the same MFMA score pass
// over keys read in place, but reduced inside the wave, so a call stages two floats per (row, key
// block) instead of every score.
//
//   recall_score_kernel   one wave per 128-key block of the reordered sequence: its four 32-key MFMA
//                         tiles against the S probe rows (padded to one or two 32-row tiles; keys and
//                         queries gathered through `rows`, 16 bytes per lane and k-step, no LDS). The
//                         wave keeps all four tiles' accumulators, takes each row's block maximum m_c of
//                         t_j = scale*log2(e)*<q,k_j> (lane-local over the tiles, then an xor butterfly
//                         over the 32 lanes that hold the row) and sum_c = sum_j exp2(t_j - m_c) the same
//                         way; keys past L count as -inf. Staged: [B*H][S][nb][2] fp32 (m_c, sum_c).
//   recall_reduce_kernel  one workgroup per staged row: the row maximum M, E_c = sum_c * exp2(m_c - M)
//                         in LDS, the mask row's kept flags and their count n; every block's rank by
//                         counting (value descending, then index ascending); then T, K and the oracle's
//                         sum, each by ONE thread walking the blocks in ascending order, so an all-ones
//                         mask gives K == T in bits and a mask that holds the n heaviest blocks gives
//                         the oracle's bits.
//   recall_mean_kernel    one thread per (b,h): the fp32 means over the S rows, summed in row order.
//
// No launch allocates or synchronises; no floating-point atomics; three launches on the caller's stream.
#include <cmath>
#include <string>

#include "vb_common.hpp"

namespace vb {
namespace {

constexpr int kBlockKeys = 128;     // keys per mask block
constexpr int kKeyTile = 32;        // keys per MFMA tile
constexpr int kTiles = kBlockKeys / kKeyTile;
constexpr int kScoreWaves = 4;      // key blocks per score workgroup
constexpr int kMaxSamples = 64;
constexpr int kMaxBlocks = 1024;    // L <= 131072
constexpr int kReduceThreads = 256;
constexpr int kMeanThreads = 64;

struct RecallParams {
  const void* q; const void* k;
  int64_t qs[3], ks[3];
  const int32_t* rows; const int32_t* probe_pos;
  const uint8_t* mask; int64_t ms[3];
  int B, H, L, D, S, nb;
  float c;              // scale * log2(e)
  float* pairs;         // workspace [B*H][S][nb][2]: block maximum, sum of exp2 relative to it
  float* rowv;          // workspace [B*H][S][2]: the rows' recall and oracle recall, for the mean launch
  float* recall; float* oracle; float* row_recall; float* row_oracle; int32_t* row_kept;
};

__device__ __forceinline__ int clamp_pos(int x, int L) { return x < 0 ? 0 : (x > L - 1 ? L - 1 : x); }

// ------------------------------------------------------------------------------------------ scores
// QT: 32-row tiles of probe rows (1: S <= 32, 2: S <= 64)
template <class T, int D, int QT>
__global__ void __launch_bounds__(64 * kScoreWaves) recall_score_kernel(const RecallParams p) {
  using vec8 = typename T::vec8;
  constexpr int kSteps = D / 16;
  const int bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int wave = threadIdx.x >> 6, lane = lane_id();
  const int r32 = lane & 31, half = lane >> 5;
  const int blk = blockIdx.x * kScoreWaves + wave;
  if (blk >= p.nb) return;   // uniform per wave; the kernel has no barrier
  const typename T::raw* qb = reinterpret_cast<const typename T::raw*>(p.q) + b * p.qs[0] + h * p.qs[1];
  const typename T::raw* kb = reinterpret_cast<const typename T::raw*>(p.k) + b * p.ks[0] + h * p.ks[1];

  // the probe rows as MFMA A operands: lane (r32, half) holds row r32 (+32), d = 16*step + 8*half ..+7.
  // Rows past S repeat row S-1 (never stored); positions and row numbers are clamped to [0, L-1].
  vec8 qa[QT][kSteps];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    int s = r32 + 32 * t;
    s = s < p.S ? s : p.S - 1;
    int row = clamp_pos(p.probe_pos[s], p.L);
    if (p.rows) row = clamp_pos(p.rows[row], p.L);
    const typename T::raw* src = qb + (int64_t)row * p.qs[2] + 8 * half;
#pragma unroll
    for (int st = 0; st < kSteps; ++st) qa[t][st] = *reinterpret_cast<const vec8*>(src + 16 * st);
  }

  // C layout: column (key) = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  f32x16 x[QT][kTiles];
#pragma unroll
  for (int i = 0; i < kTiles; ++i) {
    const int j = blk * kBlockKeys + i * kKeyTile + r32;
    const bool live = j < p.L;
    int row = live ? j : p.L - 1;
    if (p.rows) row = clamp_pos(p.rows[row], p.L);
    const typename T::raw* src = kb + (int64_t)row * p.ks[2] + 8 * half;
    vec8 kf[kSteps];
#pragma unroll
    for (int st = 0; st < kSteps; ++st) kf[st] = *reinterpret_cast<const vec8*>(src + 16 * st);
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      f32x16 acc = {};
#pragma unroll
      for (int st = 0; st < kSteps; ++st) acc = T::mfma32(qa[t][st], kf[st], acc);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) x[t][i][reg] = live ? acc[reg] * p.c : -INFINITY;
    }
  }

  // per row: block maximum and the sum of exp2 relative to it, over this lane's four keys in tile
  // order, then over the 32 lanes of the half (xor butterflies: a fixed order, every lane the same
  // bits). Every block holds at least one real key, so the maximum is finite.
  float* out = p.pairs + (int64_t)bh * p.S * p.nb * 2;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    float pm = 0.f, ps = 0.f;   // the pair of the row this lane stores: reg == r32
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      float m = fmaxf(fmaxf(x[t][0][reg], x[t][1][reg]), fmaxf(x[t][2][reg], x[t][3][reg]));
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
      float s = exp2_fast(x[t][0][reg] - m);
      s += exp2_fast(x[t][1][reg] - m);
      s += exp2_fast(x[t][2][reg] - m);
      s += exp2_fast(x[t][3][reg] - m);
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
      if (r32 == reg) { pm = m; ps = s; }
    }
    const int s = (r32 & 3) + 8 * (r32 >> 2) + 4 * half + 32 * t;
    if (r32 < 16 && s < p.S) {
      float* dst = out + ((int64_t)s * p.nb + blk) * 2;
      dst[0] = pm;
      dst[1] = ps;
    }
  }
}

// ------------------------------------------------------------------------------------------ reduce
__global__ void __launch_bounds__(kReduceThreads) recall_reduce_kernel(const RecallParams p) {
  __shared__ float E[kMaxBlocks];
  __shared__ uint8_t kept[kMaxBlocks], best[kMaxBlocks];
  __shared__ float partf[kReduceThreads / 64];
  __shared__ int parti[kReduceThreads / 64];
  __shared__ float sums[3];
  const int r = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int tid = threadIdx.x, wave = tid >> 6, lane = lane_id();
  const int nb = p.nb;
  const int i = clamp_pos(p.probe_pos[r], p.L) / kBlockKeys;
  const float* pr = p.pairs + ((int64_t)bh * p.S + r) * nb * 2;
  const uint8_t* mrow = p.mask + b * p.ms[0] + h * p.ms[1] + i * p.ms[2];

  // the row maximum (a maximum does not depend on its order) and the kept count (an integer sum)
  float m = -INFINITY;
  int n = 0;
  for (int c = tid; c < nb; c += kReduceThreads) {
    m = fmaxf(m, pr[2 * c]);
    const uint8_t f = mrow[c] != 0;
    kept[c] = f;
    n += f;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    m = fmaxf(m, __shfl_xor(m, d, 64));
    n += __shfl_xor(n, d, 64);
  }
  if (lane == 0) { partf[wave] = m; parti[wave] = n; }
  __syncthreads();
  m = partf[0];
  n = parti[0];
  for (int w = 1; w < kReduceThreads / 64; ++w) { m = fmaxf(m, partf[w]); n += parti[w]; }

  for (int c = tid; c < nb; c += kReduceThreads) E[c] = pr[2 * c + 1] * exp2_fast(pr[2 * c] - m);
  __syncthreads();

  // the n heaviest blocks by counting: block c's rank is the number of blocks ahead of it in the
  // order (mass descending, index ascending)
  for (int c = tid; c < nb; c += kReduceThreads) {
    const float e = E[c];
    int rank = 0;
    for (int o = 0; o < nb; ++o) {
      const float eo = E[o];
      rank += (eo > e || (eo == e && o < c)) ? 1 : 0;
    }
    best[c] = rank < n;
  }
  __syncthreads();

  // three serial sums over the blocks in ascending order, one thread of three different waves each;
  // a block left out adds +0, which changes no bit of a non-negative sum
  if (lane == 0 && wave < 3) {
    const uint8_t* flag = wave == 1 ? kept : best;
    float s = 0.f;
    if (wave == 0) {
      for (int c = 0; c < nb; ++c) s += E[c];
    } else {
      for (int c = 0; c < nb; ++c) s += flag[c] ? E[c] : 0.f;
    }
    sums[wave] = s;
  }
  __syncthreads();
  if (tid != 0) return;
  const float total = sums[0];   // >= 1: the row's largest e is exp2(0)
  const float rec = sums[1] / total, ora = sums[2] / total;
  const int64_t o = (int64_t)bh * p.S + r;
  p.rowv[2 * o] = rec;
  p.rowv[2 * o + 1] = ora;
  if (p.row_recall) p.row_recall[o] = rec;
  if (p.row_oracle) p.row_oracle[o] = ora;
  if (p.row_kept) p.row_kept[o] = n;
}

// -------------------------------------------------------------------------------------------- mean
__global__ void __launch_bounds__(kMeanThreads) recall_mean_kernel(const RecallParams p) {
  const int bh = blockIdx.x * kMeanThreads + threadIdx.x;
  if (bh >= p.B * p.H) return;
  const float* v = p.rowv + (int64_t)bh * p.S * 2;
  float rec = 0.f, ora = 0.f;
  for (int r = 0; r < p.S; ++r) {
    rec += v[2 * r];
    ora += v[2 * r + 1];
  }
  p.recall[bh] = rec / (float)p.S;
  if (p.oracle) p.oracle[bh] = ora / (float)p.S;
}

int blocks_of(const vb_recall_args* a) { return (a->L + kBlockKeys - 1) / kBlockKeys; }

template <class T>
const void* score_kernel(int D, bool two) {
  if (D == 64)
    return two ? reinterpret_cast<const void*>(recall_score_kernel<T, 64, 2>)
               : reinterpret_cast<const void*>(recall_score_kernel<T, 64, 1>);
  return two ? reinterpret_cast<const void*>(recall_score_kernel<T, 128, 2>)
             : reinterpret_cast<const void*>(recall_score_kernel<T, 128, 1>);
}

}  // namespace
}  // namespace vb

extern "C" uint64_t vb_mask_recall_workspace_size(const vb_recall_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->L <= 0 || a->S <= 0) return 0;
  // the staged (maximum, sum) pairs and the rows' two results
  const uint64_t rows = (uint64_t)a->B * a->H * a->S;
  const uint64_t words = rows * (uint64_t)vb::blocks_of(a) * 2 + rows * 2;
  return (words * 4 + 15) & ~uint64_t(15);
}

extern "C" int vb_mask_recall(const vb_recall_args* a, void* stream) {
  using namespace vb;
  const std::string fn = "vb_mask_recall: ";
  if (!a || !a->q || !a->k || !a->probe_pos || !a->block_mask || !a->recall)
    return fail(VB_ERR_INVALID, fn + "null argument");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (a->L > kMaxBlocks * kBlockKeys) return fail(VB_ERR_UNSUPPORTED, fn + "sequence too long (L <= 131072)");
  if (a->S < 1 || a->S > kMaxSamples) return fail(VB_ERR_INVALID, fn + "S must be in [1, 64]");
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, fn + "unknown dtype");
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, fn + "head_dim must be 64 or 128");
  if ((int64_t)(a->L - 1) * a->q_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31) ||
      (int64_t)(a->L - 1) * a->k_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31))
    return fail(VB_ERR_UNSUPPORTED, fn + "a q/k (b,h) slice spans >= 2 GiB");
  for (int i = 0; i < 3; ++i)
    if (((a->q_stride[i] | a->k_stride[i]) & 7) || a->q_stride[i] < 0 || a->k_stride[i] < 0)
      return fail(VB_ERR_INVALID, fn + "q/k strides must be non-negative multiples of 8");
  for (int i = 0; i < 3; ++i)
    if (a->mask_stride[i] < 0) return fail(VB_ERR_INVALID, fn + "mask strides must be non-negative");
  if ((reinterpret_cast<uintptr_t>(a->q) | reinterpret_cast<uintptr_t>(a->k)) & 15)
    return fail(VB_ERR_INVALID, fn + "q and k must be 16-byte aligned");
  const uint64_t need = vb_mask_recall_workspace_size(a);
  if (!a->workspace || a->workspace_bytes < need || (reinterpret_cast<uintptr_t>(a->workspace) & 15))
    return fail(VB_ERR_INVALID, fn + "workspace missing or smaller than vb_mask_recall_workspace_size() (" +
                                    std::to_string(need) + " bytes)");
  RecallParams p{};
  p.q = a->q; p.k = a->k;
  for (int i = 0; i < 3; ++i) { p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; p.ms[i] = a->mask_stride[i]; }
  p.rows = a->rows; p.probe_pos = a->probe_pos; p.mask = a->block_mask;
  p.B = a->B; p.H = a->H; p.L = a->L; p.D = a->D; p.S = a->S; p.nb = blocks_of(a);
  const float scale = a->scale > 0.f ? a->scale : (float)(1.0 / sqrt((double)a->D));
  p.c = scale * kLog2e;
  p.pairs = reinterpret_cast<float*>(a->workspace);
  p.rowv = p.pairs + (int64_t)a->B * a->H * a->S * p.nb * 2;
  p.recall = a->recall; p.oracle = a->oracle_recall;
  p.row_recall = a->row_recall; p.row_oracle = a->row_oracle; p.row_kept = a->row_kept;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool two = a->S > 32;
  const void* kernel = a->dtype == VB_DTYPE_BF16 ? score_kernel<BF16>(a->D, two) : score_kernel<F16>(a->D, two);
  void* params[] = {&p};
  const unsigned bh = (unsigned)(a->B * a->H);
  (void)hipLaunchKernel(kernel, dim3((unsigned)((p.nb + kScoreWaves - 1) / kScoreWaves), bh), dim3(64 * kScoreWaves),
                        params, 0, s);
  if (int rc = check_launch("recall_score_kernel")) return rc;
  (void)hipLaunchKernel(reinterpret_cast<const void*>(recall_reduce_kernel), dim3((unsigned)a->S, bh),
                        dim3(kReduceThreads), params, 0, s);
  if (int rc = check_launch("recall_reduce_kernel")) return rc;
  (void)hipLaunchKernel(reinterpret_cast<const void*>(recall_mean_kernel), dim3((bh + kMeanThreads - 1) / kMeanThreads),
                        dim3(kMeanThreads), params, 0, s);
  return check_launch("recall_mean_kernel");
}
