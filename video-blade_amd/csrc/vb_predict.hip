// Mask predictor for gfx950 (sampled pooled scores + energy top-k).
//
// vb_mask_predict fuses, per (b, h) and group of four 32-row sampled q-blocks:
//   * efficient_attn_with_pooling: replicate pad + per-block token sampling
//     (cogvideox/train/special_attentions_local/TrainRelated/cogvideo_blocksparseattn.py:20-82),
//     done as row-index arithmetic on the caller's (un-reordered) q/k through the Gilbert rows;
//   * the Triton pooled-score kernel (TrainRelated/attn_pooling_kernel.py:17-255): per sampled row
//     the max logit of every 32-key sampled block (MFMA 32x32x16, query on the lane), rounded to the
//     storage dtype (R), the running fp32 row max m, then Po[i,j] = max_rows exp2(R - m) and the
//     storage-dtype row normalisation; the kernel's tile size is num_keep, the sampled tokens per
//     block: 32 by default, 16 and 64 as further instantiations (mask_predict_kernel's kKeep);
//   * transfer_attn_to_mask(mode="energy") (:177-249; wanx_blocksparseattn.py:162-233): stable
//     descending rank, fp32-accumulated cumsum rounded to the storage dtype per prefix, the first
//     crossing of storage(total * thr), clamp to [min_keep, max_keep], forced tail rows/cols.
//     vb_mask_predict_rule runs the rule's other forms in the same place (kRule instantiations):
//     the energy rule with bounds and threshold per (b,h), and mode="topk" (:205-225).
// Nothing but Po and the mask reaches HBM (R stays in LDS).
//
// This unit: the C entries with their validation and set-up, the stand-alone mask and offset kernels,
// and the 16 score kernels of vb_mask_predict / vb_mask_predict_long. The score kernel itself is
// vb_predict_kernel.hpp, the per-row rules vb_mask_rows.hpp, the 12 rule kernels vb_predict_rule.hip.
#include <cstdlib>

#include "vb_trace.hpp"

// Diagnostic builds only: the device globals behind -DVB_PRED_TRACE=1 (tools/diag/pred_trace.py) and
// -DVB_PRED_STAMPS=1 (tools/diag/pred_stamps.py), and the hooks through which this unit's score
// kernels write them (vb_predict_kernel.hpp; the rule unit's kernels are never instrumented).
#ifndef VB_PRED_TRACE
#define VB_PRED_TRACE 0
#endif
#ifndef VB_PRED_STAMPS
#define VB_PRED_STAMPS 0
#endif
#if VB_PRED_TRACE
namespace vb { __device__ TraceBuf g_pred_trace; }
#define VB_TRACE_START(k) trace_start(g_pred_trace, k)
#define VB_TRACE_END() trace_end(g_pred_trace)
#endif
#if VB_PRED_STAMPS
namespace vb { __device__ unsigned long long g_pred_stamp[8]; }
#define VB_PRED_KERNEL_STAMPS 1
#endif

#include "vb_predict_kernel.hpp"

namespace vb {

// random_sample_tokens' topk (cogvideo_blocksparseattn.py:45-46): for every row of `n` uniform draws,
// the indices of the `keep` largest values in descending order of value (ties -> lower index
// first). One wave per row; blockIdx.y selects the q or the k draws.
__global__ void __launch_bounds__(256) topk_offsets_kernel(const float* rq, const float* rk, int rows, int n,
                                                           int keep, int32_t* oq, int32_t* ok) {
  __shared__ alignas(16) float buf[4][256];
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows || n > 256) return;
  topk_wave((blockIdx.y ? rk : rq) + (int64_t)row * n, n, keep, (blockIdx.y ? ok : oq) + (int64_t)row * keep, buf[wave]);
}

// LDS floats per row buffer of energy_mask_kernel (val and keys each; keys padded to 16)
__host__ __device__ inline int energy_row_floats(int nc) { return nc <= kMaxNb ? kEnergyRow : ((nc + 15) & ~15); }
static size_t energy_smem_bytes(int nc) { return (size_t)4 * 2 * energy_row_floats(nc) * 4; }

template <class T>
__global__ void __launch_bounds__(256) energy_mask_kernel(const void* po, int rows_total, int nc, float thr,
                                                          int min_keep, int max_keep, int force_tail, int nr,
                                                          uint8_t* mask, unsigned long long* count) {
  // [4 waves][val | keys], energy_row_floats(nc) floats each (dynamic: rows of up to kMaxNb columns
  // keep the 10.5 KiB the static buffer took)
  extern __shared__ __attribute__((aligned(16))) float energy_buf[];
  const int erow = energy_row_floats(nc);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows_total) return;
  const typename T::raw* src = reinterpret_cast<const typename T::raw*>(po) + (int64_t)row * nc;
  float* val = energy_buf + wave * 2 * erow;
  for (int j = lane; j < nc; j += 64) val[j] = T::to_f32(src[j]);
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int i = row % nr;
  const bool force_all = force_tail > 0 && i >= nr - force_tail;
  const int kept = energy_row<T, true>(val, reinterpret_cast<uint32_t*>(val + erow), mask + (int64_t)row * nc, nc,
                                       thr, min_keep, max_keep, force_tail, force_all);
  if (count && lane == 0) atomicAdd(count, (unsigned long long)kept);
}

// vb_block_mask_rule: energy_mask_kernel with rule_row in place of energy_row (one wave per row; the
// row's head is row / nr). `grow` of the top-k updates is the row count nr.
template <class T>
__global__ void __launch_bounds__(256) rule_mask_kernel(const void* po, int rows_total, int nc, const RuleParams rule,
                                                        float thr, int min_keep, int max_keep, int force_tail, int nr,
                                                        uint8_t* mask, unsigned long long* count, int32_t* rows_kept) {
  extern __shared__ __attribute__((aligned(16))) float energy_buf[];
  const int erow = energy_row_floats(nc);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + wave;
  if (row >= rows_total) return;
  const typename T::raw* src = reinterpret_cast<const typename T::raw*>(po) + (int64_t)row * nc;
  float* val = energy_buf + wave * 2 * erow;
  for (int j = lane; j < nc; j += 64) val[j] = T::to_f32(src[j]);
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int i = row % nr;
  const bool force_all = force_tail > 0 && i >= nr - force_tail;
  const int kept = rule_row<T>(rule, row / nr, val, reinterpret_cast<uint32_t*>(val + erow), mask + (int64_t)row * nc,
                               nc, nr, thr, min_keep, max_keep, force_tail, force_all);
  if (count && lane == 0) atomicAdd(count, (unsigned long long)kept);
  if (rows_kept && lane == 0) rows_kept[row] = kept;
}

// vb_mask_rule -> RuleParams; nc = the row width a scalar init_k is checked against
static int resolve_rule(const vb_mask_rule* r, int nc, int min_keep, int max_keep, const std::string& fn, RuleParams* out) {
  if (r->mode != VB_RULE_ENERGY && r->mode != VB_RULE_TOPK)
    return fail(VB_ERR_INVALID, fn + "unknown rule mode " + std::to_string(r->mode));
  RuleParams p{};
  p.mode = r->mode;
  if (r->mode == VB_RULE_TOPK) {
    if (!r->init_k_bh && (r->init_k < 1 || r->init_k > nc))
      return fail(VB_ERR_INVALID, fn + "init_k must be in [1, " + std::to_string(nc) + "], got " + std::to_string(r->init_k));
    p.k0 = r->init_k; p.k0_bh = r->init_k_bh;
    p.lo = r->grow_below > 0.f ? r->grow_below : 0.6f;
    p.hi = r->shrink_below > 0.f ? r->shrink_below : 0.9f;
  } else {
    if ((!r->min_keep && min_keep < 1) || (!r->max_keep && max_keep < 1))
      return fail(VB_ERR_INVALID, fn + "keep counts must be >= 1");
    p.min_keep = r->min_keep; p.max_keep = r->max_keep; p.thr = r->energy_threshold;
  }
  *out = p;
  return 0;
}

// workspace: the sampled k rows' int32 byte offsets | R; both scale with the sampling density `keep`
// (rows per block)
static uint64_t predict_rows_bytes(int B, int H, int L, int keep) {
  const int nb = (L + 127) / 128;
  return (uint64_t)B * H * nb * keep * 4;
}
static uint64_t predict_ws_bytes(int B, int H, int L, int keep) {
  const uint64_t nb = (L + 127) / 128;
  return predict_rows_bytes(B, H, L, keep) + (uint64_t)B * H * nb * nb * keep * 2;
}

// B*H*block bound of the in-kernel Philox draws (see vb_mask_predict), per device, cached
static int64_t philox_x_only_numel() {
  static int64_t cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 0;
  if (dev < 64 && cache[dev] > 0) return cache[dev];
  int cus = 0, thr = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipDeviceGetAttribute(&thr, hipDeviceAttributeMaxThreadsPerMultiProcessor, dev) != hipSuccess)
    return 0;
  const int64_t n = (int64_t)cus * thr;
  if (dev < 64) cache[dev] = n;
  return n;
}

// (head dim, dtype, kLong, density, rule) -> launch_predict<...>; the caller has checked every value.
// This unit's 16 instantiations: per head dim and dtype the short and the long kernel at density 32,
// and densities 16 and 64 in the long form only (it writes the short one's bits for nb <= kMaxNb; the
// entry's own row limit is checked before). The 12 rule kernels are vb_predict_rule.hip's.
template <int D, class T, bool kLong>
static int dispatch_keep(const PredParams& p, int keep, hipStream_t s, hipEvent_t ev) {
  if (keep == 16) return launch_predict<D, T, true, 16>(p, s, ev);
  if (keep == 64) return launch_predict<D, T, true, 64>(p, s, ev);
  return launch_predict<D, T, kLong>(p, s, ev);
}
template <bool kLong>
static int dispatch_predict(const PredParams& p, int dtype, int keep, bool rule, hipStream_t s, hipEvent_t ev) {
  if (rule) return launch_predict_rule(p, dtype, keep, s, ev);
  const bool bf = dtype == VB_DTYPE_BF16;
  if (p.D == 64) return bf ? dispatch_keep<64, BF16, kLong>(p, keep, s, ev) : dispatch_keep<64, F16, kLong>(p, keep, s, ev);
  return bf ? dispatch_keep<128, BF16, kLong>(p, keep, s, ev) : dispatch_keep<128, F16, kLong>(p, keep, s, ev);
}

// What the two passes that can ride in the score kernel's launch (pooled K/V, KV pyramid) share: the
// pool_v stride check, the task's source fields, and the launch's workgroups for the pass: one per 256
// of its 16-byte items (`rows_out` output rows of D/8 chunks per (b,h)), capped per head dim.
template <class Task>
static int fused_pass_setup(const vb_predict_args* a, const std::string& fn, int rows_out, Task& t, int* n_pool) {
  for (int i = 0; i < 3; ++i)
    if (a->pool_v_stride[i] & 7) return fail(VB_ERR_INVALID, fn + "pool_v strides must be multiples of 8");
  t.k = reinterpret_cast<const uint8_t*>(a->k); t.v = reinterpret_cast<const uint8_t*>(a->pool_v);
  for (int i = 0; i < 3; ++i) { t.ks[i] = a->k_stride[i]; t.vs[i] = a->pool_v_stride[i]; }
  t.rows = a->rows; t.B = a->B; t.H = a->H; t.L = a->L;
  const int64_t items = (int64_t)a->B * a->H * rows_out * (a->D / 8);
  int n = (int)((items + 255) / 256);
  const int cap = a->D == 64 ? kFusedPoolWgs64 : kFusedPoolWgs;
  n = n < cap ? n : cap;
  *n_pool = (n + 7) / 8 * 8;   // keeps blockIdx % 8 of the score workgroups (their XCD)
  return 0;
}

}  // namespace vb

#if VB_PRED_TRACE
VB_TRACE_GETTER(vb_debug_pred_trace, vb::g_pred_trace)
#endif
#if VB_PRED_STAMPS
// diagnostic builds only: read and clear the score kernel's phase sums
extern "C" int vb_debug_pred_stamps(unsigned long long* out) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vb::g_pred_stamp), 8 * sizeof(unsigned long long)) != hipSuccess) return -1;
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  return hipMemcpyToSymbol(HIP_SYMBOL(vb::g_pred_stamp), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" uint64_t vb_mask_predict_workspace_size(const vb_predict_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->L <= 0 || a->D <= 0 || a->num_keep <= 0) return 0;
  return vb::predict_ws_bytes(a->B, a->H, a->L, a->num_keep);
}

// vb_mask_predict, vb_mask_predict_long and vb_mask_predict_rule: one validation and parameter
// set-up, `fn` names the entry in the messages, kLong selects the row limit and the kernel
// instantiation. `rule` (vb_mask_predict_rule only, kLong) selects the rule instantiations.
template <bool kLong>
static int mask_predict_entry(const vb_predict_args* a, void* stream, const vb_mask_rule* rule = nullptr) {
  using namespace vb;
  const std::string fn = rule ? "vb_mask_predict_rule: " : kLong ? "vb_mask_predict_long: " : "vb_mask_predict: ";
  if (!a || !a->q || !a->k || !a->q_off || !a->k_off || !a->po)
    return fail(VB_ERR_INVALID, fn + "null argument");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (a->block != 128 || (a->num_keep != 16 && a->num_keep != 32 && a->num_keep != 64))
    return fail(VB_ERR_UNSUPPORTED, fn + "block must be 128 and num_keep 16, 32 or 64 (got block " +
                                        std::to_string(a->block) + ", num_keep " + std::to_string(a->num_keep) + ")");
  const int nb = (a->L + a->block - 1) / a->block;
  if (nb > (kLong ? kMaxNbLong : kMaxNb)) return fail(VB_ERR_UNSUPPORTED, fn + "sequence too long");
  // The short entry's L < 65536 guard came with the packed sort keys. Audit of every 16-bit quantity
  // on this path: the sort key's low 16 bits hold 0xFFFF - (block index <= 1023) and its high 16 the
  // score's storage bits; R holds storage bits; the buffer descriptors' 16-bit field is the (zero)
  // stride. Token positions are int32 throughout (sampled_row, the int32 byte-offset table, the
  // descriptors' byte counts, checked < 2^31 below), so the long entry has no such guard.
  if (!kLong && a->L > 65535) return fail(VB_ERR_UNSUPPORTED, fn + "L must be < 65536");
  PredParams p{};
  if (rule) {
    if (a->mask_level) return fail(VB_ERR_INVALID, fn + "mask_level and a rule are exclusive");
    if (int rc = resolve_rule(rule, nb, a->min_keep, a->max_keep, fn, &p.rule)) return rc;
  } else if (a->min_keep < 1 || a->max_keep < 1) {
    return fail(VB_ERR_INVALID, fn + "keep counts must be >= 1");
  }
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, fn + "head_dim must be 64 or 128");
  const uint64_t ws = predict_ws_bytes(a->B, a->H, a->L, a->num_keep);
  if (!a->workspace || a->workspace_bytes < ws || (reinterpret_cast<uintptr_t>(a->workspace) & 15))
    return fail(VB_ERR_INVALID, fn + "workspace missing or smaller than vb_mask_predict_workspace_size()");
  const uint64_t rows_b = predict_rows_bytes(a->B, a->H, a->L, a->num_keep);
  if (rows_b / a->B / a->H >= (uint64_t(1) << 31)) return fail(VB_ERR_UNSUPPORTED, fn + "sampled stream too large");
  if ((int64_t)(a->L - 1) * a->k_stride[2] * 2 + 2 * a->D >= (int64_t(1) << 31))
    return fail(VB_ERR_UNSUPPORTED, fn + "a k (b,h) slice spans >= 2 GiB");
  for (int i = 0; i < 3; ++i)
    if ((a->q_stride[i] | a->k_stride[i]) & 7) return fail(VB_ERR_INVALID, fn + "strides must be multiples of 8");
  p.q = a->q; p.k = a->k;
  for (int i = 0; i < 3; ++i) { p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; }
  p.rows = a->rows; p.q_off = a->q_off; p.k_off = a->k_off;
  p.B = a->B; p.H = a->H; p.L = a->L; p.D = a->D; p.block = a->block; p.nb = nb;
  const float scale = a->scale > 0.f ? a->scale : (float)(1.0 / sqrt((double)a->D));
  p.c = scale * 1.44269504f;
  p.thr = a->energy_threshold;
  p.min_keep = a->min_keep; p.max_keep = a->max_keep; p.force_tail = a->force_tail;
  p.po = a->po; p.mask = a->mask; p.count = a->mask_count;
  // the kept counts come from the energy rule of the fused epilogue: refused where it does not run
  if (a->mask_rows_kept && (a->mask_level || !a->mask))
    return fail(VB_ERR_INVALID, fn + "mask_rows_kept needs the energy mask (mask set, mask_level 0)");
  p.rows_kept = a->mask_rows_kept;
  p.k_row_off = reinterpret_cast<int32_t*>(a->workspace);
  p.rbuf = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(a->workspace) + rows_b);
  if ((a->rand_q == nullptr) != (a->rand_k == nullptr))
    return fail(VB_ERR_INVALID, fn + "give both rand_q and rand_k or neither");
  p.rand_q = a->rand_q; p.rand_k = a->rand_k;
  if (a->level_bands < 0 || a->level_bands > 8 ||
      (a->level_bands > 0 && (!a->level_band_value || !a->level_band_start || !a->level_band_end)))
    return fail(VB_ERR_INVALID, fn + "0..8 level bands with value/start/end arrays");
  if (a->mask_level) {
    if (!a->mask) return fail(VB_ERR_INVALID, fn + "mask_level needs a mask output");
    p.level = 1;
    p.lv.n = a->level_bands;
    for (int i = 0; i < a->level_bands; ++i) {
      const int val = a->level_band_value[i];
      if (val != 0 && val != 1 && val != 2 && val != 4 && val != 8)
        return fail(VB_ERR_INVALID, fn + "band values must be 0, 1, 2, 4 or 8");
      // max(0, int(nb * start)), min(nb, int(nb * end)) in double, as vb_level_mask
      const int ia = (int)((double)nb * a->level_band_start[i]), ib = (int)((double)nb * a->level_band_end[i]);
      p.lv.value[i] = val;
      p.lv.start[i] = ia < 0 ? 0 : ia;
      p.lv.end[i] = ib > nb ? nb : ib;
    }
  }
  if (a->philox) {
    if (a->rand_q || a->rand_k) return fail(VB_ERR_INVALID, fn + "philox and rand_q/rand_k are exclusive");
    // torch.rand's grid-stride launch gives element i the x value of thread i only while every
    // element has a thread of its own: numel <= CUs * max threads per CU of THIS device (524288 on
    // an unpartitioned MI355X; fewer in a CPX partition)
    const int64_t one_pass = philox_x_only_numel();
    if (one_pass <= 0) return fail(VB_ERR_LAUNCH, fn + "cannot query the device's CU count");
    if ((int64_t)a->B * a->H * a->block > one_pass)
      return fail(VB_ERR_UNSUPPORTED, fn + "philox draws need B*H*block <= " + std::to_string(one_pass) +
                                          " (CUs x max threads per CU of this device)");
    p.philox = 1; p.philox_seed = a->philox_seed; p.philox_offset = a->philox_offset;
  }
  if (a->pool_kp) {   // the pooled K/V pass rides in the score kernel's launch
    if (!a->pool_v || !a->pool_vp || a->pool_gap <= 0 || ((a->pool_k_r == nullptr) != (a->pool_v_r == nullptr)))
      return fail(VB_ERR_INVALID, fn + "pool_v, pool_vp, pool_gap > 0 and both or neither of pool_k_r/pool_v_r");
    PoolTask& t = p.pool;
    t.D = a->D; t.gap = a->pool_gap;
    t.Lp = (a->L + a->pool_gap - 1) / a->pool_gap;
    if (int rc = fused_pass_setup(a, fn, t.Lp, t, &p.n_pool)) return rc;
    t.kp = reinterpret_cast<uint8_t*>(a->pool_kp); t.vp = reinterpret_cast<uint8_t*>(a->pool_vp);
    t.k_r = reinterpret_cast<uint8_t*>(a->pool_k_r); t.v_r = reinterpret_cast<uint8_t*>(a->pool_v_r);
  }
  if (a->pyr_k) {   // the KV pyramid pass rides in the score kernel's launch
    if (a->pool_kp) return fail(VB_ERR_INVALID, fn + "pool_* and pyr_* are exclusive");
    if (!a->pyr_v || !a->pool_v) return fail(VB_ERR_INVALID, fn + "pyr_k needs pyr_v and pool_v");
    PyrTask& t = p.pyr;
    t.Lpad = nb * 128;
    if (int rc = fused_pass_setup(a, fn, t.Lpad / 8, t, &p.n_pool)) return rc;
    if (((reinterpret_cast<uintptr_t>(a->k) | reinterpret_cast<uintptr_t>(a->pool_v) |
          reinterpret_cast<uintptr_t>(a->pyr_k) | reinterpret_cast<uintptr_t>(a->pyr_v)) & 15) != 0)
      return fail(VB_ERR_INVALID, fn + "pyramid tensors must be 16-byte aligned");
    t.kpyr = reinterpret_cast<uint8_t*>(a->pyr_k); t.vpyr = reinterpret_cast<uint8_t*>(a->pyr_v);
    p.pool_kind = 2;
  }
#if VB_DIAG
  if (const char* d = getenv("VB_DEBUG_PRED")) p.dbg = atoi(d);
#endif
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipEvent_t ev = reinterpret_cast<hipEvent_t>(a->staged_event);
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, fn + "unknown dtype");
  return dispatch_predict<kLong>(p, a->dtype, a->num_keep, rule != nullptr, s, ev);
}

extern "C" int vb_mask_predict(const vb_predict_args* a, void* stream) { return mask_predict_entry<false>(a, stream); }

extern "C" int vb_mask_predict_long(const vb_predict_args* a, void* stream) {
  return mask_predict_entry<true>(a, stream);
}

extern "C" int vb_mask_predict_rule(const vb_predict_args* a, const vb_mask_rule* rule, void* stream) {
  if (rule) return mask_predict_entry<true>(a, stream, rule);
  // no rule: the call (and the bits) of the entry that serves this row count
  if (a && a->block > 0 && a->L > 0 && (a->L + a->block - 1) / a->block > vb::kMaxNb) return mask_predict_entry<true>(a, stream);
  return mask_predict_entry<false>(a, stream);
}

extern "C" int vb_block_mask_rule(const void* po, int B, int H, int nr, int nc, const vb_mask_rule* rule,
                                  float energy_threshold, int min_keep, int max_keep, int force_tail, int dtype,
                                  uint8_t* mask, unsigned long long* mask_count, int32_t* rows_kept, void* stream) {
  using namespace vb;
  const std::string fn = "vb_block_mask_rule: ";
  if (!po || !mask) return fail(VB_ERR_INVALID, fn + "null argument");
  if (B <= 0 || H <= 0 || nr <= 0 || nc <= 0) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (nc > kMaxNbLong) return fail(VB_ERR_UNSUPPORTED, fn + "too many columns");
  if (force_tail < 0) return fail(VB_ERR_INVALID, fn + "force_tail must be >= 0");
  RuleParams rp{};   // no rule: energy mode with the call's scalars (vb_energy_mask's rule)
  vb_mask_rule none{};
  if (int rc = resolve_rule(rule ? rule : &none, nc, min_keep, max_keep, fn, &rp)) return rc;
  if (dtype != VB_DTYPE_BF16 && dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, fn + "unknown dtype");
  const int rows = B * H * nr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((rows + 3) / 4);
  if (dtype == VB_DTYPE_BF16)
    hipLaunchKernelGGL(rule_mask_kernel<BF16>, grid, dim3(256), energy_smem_bytes(nc), s, po, rows, nc, rp, energy_threshold,
                       min_keep, max_keep, force_tail, nr, mask, mask_count, rows_kept);
  else
    hipLaunchKernelGGL(rule_mask_kernel<F16>, grid, dim3(256), energy_smem_bytes(nc), s, po, rows, nc, rp, energy_threshold,
                       min_keep, max_keep, force_tail, nr, mask, mask_count, rows_kept);
  return check_launch("rule_mask_kernel");
}

extern "C" int vb_energy_mask(const void* po, int B, int H, int nr, int nc, float energy_threshold, int min_keep,
                              int max_keep, int force_tail, int dtype, uint8_t* mask,
                              unsigned long long* mask_count, void* stream) {
  using namespace vb;
  if (!po || !mask) return fail(VB_ERR_INVALID, "vb_energy_mask: null argument");
  if (B <= 0 || H <= 0 || nr <= 0 || nc <= 0) return fail(VB_ERR_INVALID, "vb_energy_mask: bad sizes");
  if (nc > kMaxNbLong) return fail(VB_ERR_UNSUPPORTED, "vb_energy_mask: too many columns");
  if (min_keep < 1 || max_keep < 1) return fail(VB_ERR_INVALID, "vb_energy_mask: keep counts must be >= 1");
  const int rows = B * H * nr;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((rows + 3) / 4);
  if (dtype == VB_DTYPE_BF16)
    hipLaunchKernelGGL(energy_mask_kernel<BF16>, grid, dim3(256), energy_smem_bytes(nc), s, po, rows, nc, energy_threshold, min_keep,
                       max_keep, force_tail, nr, mask, mask_count);
  else if (dtype == VB_DTYPE_F16)
    hipLaunchKernelGGL(energy_mask_kernel<F16>, grid, dim3(256), energy_smem_bytes(nc), s, po, rows, nc, energy_threshold, min_keep,
                       max_keep, force_tail, nr, mask, mask_count);
  else
    return fail(VB_ERR_INVALID, "vb_energy_mask: unknown dtype");
  return check_launch("energy_mask_kernel");
}

extern "C" int vb_sample_offsets(const float* rand_q, const float* rand_k, int rows, int n, int keep,
                                 int32_t* q_off, int32_t* k_off, void* stream) {
  using namespace vb;
  if (!rand_q || !rand_k || !q_off || !k_off) return fail(VB_ERR_INVALID, "vb_sample_offsets: null argument");
  if (rows <= 0 || n <= 0 || keep <= 0 || keep > n) return fail(VB_ERR_INVALID, "vb_sample_offsets: bad sizes");
  if (n > 256) return fail(VB_ERR_UNSUPPORTED, "vb_sample_offsets: at most 256 draws per row");
  hipLaunchKernelGGL(topk_offsets_kernel, dim3((rows + 3) / 4, 2), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     rand_q, rand_k, rows, n, keep, q_off, k_off);
  return check_launch("topk_offsets_kernel");
}
