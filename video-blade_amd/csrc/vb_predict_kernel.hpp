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
// This header holds the score kernel, its sampling launch and launch_predict<...>. Two translation
// units instantiate it side by side (the kernel's device compile is the build's critical path):
// vb_predict.hip the 16 kernels of vb_mask_predict / vb_mask_predict_long, vb_predict_rule.hip the 12
// kRule kernels behind launch_predict_rule.
#pragma once
#include <type_traits>

#include <rocrand/rocrand_kernel.h>

#include "vb_tiles.hpp"
#include "vb_pool.hpp"
#include "vb_pyr.hpp"
#include "vb_mask_rows.hpp"

namespace vb {

// The shape of the score kernel. Each of these was a build knob while it was being tuned; the values
// below are the ones that won, the others' code is gone.
constexpr int kPWaves = 4;   // sampled q-blocks (one per wave) sharing one K stream through LDS
constexpr int kPThreads = 64 * kPWaves;
constexpr int kPMinWg = 2;   // __launch_bounds__' workgroups per CU (no further register budget)
// keys per LDS tile: D=64 streams four 32-key sampled blocks per barrier (16 MFMAs per wave),
// D=128 two (also 16 MFMAs); 16 KiB tiles in a 2-deep ring at D=64 (36.5 KiB with the row-offset
// ring: four workgroups per CU) and a 3-deep ring at D=128 (52.5 KiB: three per CU).
// (Two q-blocks per wave at D=64, each K fragment read feeding two MFMAs, halved the LDS reads per
// FLOP and measured 0.975x alone, 0.962x per call: profiles/archive/r04_fwd1_experiments.md.)
template <int D> constexpr int kKeysPerTile = (D == 64) ? 128 : 64;
// K ring slots. D=64: a 2-slot ring (36.5 KiB of LDS, four workgroups per CU), see kFusedPoolWgs64
template <int D> constexpr int kPBufs = D == 64 ? 2 : 3;
// (No constant for it: K rows are gathered by the score kernel's own DMA from the caller's k, the
// sampling launch writes their byte offsets only. The sampled-row copy that it replaced made 27 MB
// per CogVideoX call, profiles/archive/r03_experiments.md.)

constexpr int kPSched = 4;   // K-fragment reads issued this many MFMAs ahead of their MFMA
constexpr int kPRCols = 3;   // R-readback columns per lane per pass in the epilogue
typedef int i32x4 __attribute__((ext_vector_type(4)));
// pooling workgroups after the score workgroups: D=128 (Wan) only. Round 5, with the pipelined pass:
// Wan call 1.004-1.006x (launch span 246 -> 232 us), CogVideoX 0.945x (its pass outlasts the score
// kernel's last round); before the pipelining it measured 1-4 % slower on both
// (profiles/archive/r05_pool_pipeline_ab.log)
template <int D> constexpr bool kPoolLast = D == 128;
// workgroups of the predictor's launch that run the pooled K/V pass (D=128, Wan). Round 5: with the
// pass pipelined (vb_pool.hpp) 512 measured 0.995x per Wan call against the serial pass, 320 0.999x,
// 192 0.995x, 128 0.981x (profiles/archive/r05_pool_pipeline_ab.log)
constexpr int kFusedPoolWgs = 320;
// D=64 (CogVideoX): with four score workgroups per CU, 384 pooling workgroups leave more slots to the
// score workgroups while the pass runs (per call 1.006x against the 3-slot ring with 512; 512 with
// the 2-slot ring 0.97x, 256 0.99x; Wan keeps the 3-slot ring and 512: 0.98x with 2 slots + 384)
constexpr int kFusedPoolWgs64 = 384;

struct PredParams {
  const void* q; const void* k;
  int64_t qs[3], ks[3];
  // never read or written (once the sampled q rows). It keeps its 8 bytes: without them the fields
  // behind move, hipcc merges the kernels' scalar argument loads differently (a dwordx8 for two
  // dwordx4) and the instruction streams change, which wants a timed A/B, not a clean-up.
  void* reserved;
  int32_t* k_row_off;   // byte offsets of the sampled k rows in their (b,h) slice of k [B,H,nb*keep] (workspace)
  uint16_t* rbuf;       // R [B,H,nb(q-block),nb(key block),keep rows] storage bits (workspace)
  const int32_t* rows;
  int32_t* q_off; int32_t* k_off;   // inputs, or outputs when rand_q/rand_k are given
  const float* rand_q; const float* rand_k;   // [B,H,block] uniforms (nullable): offsets drawn here
  int philox; unsigned long long philox_seed, philox_offset;   // or the uniforms generated here
  PoolTask pool;                    // pooled K/V pass run by the first n_pool workgroups (fused launch)
  PyrTask pyr;                      // or the multi-level KV pyramid pass (pool_kind 2)
  int n_pool, pool_kind;
  int level;        // 1: the epilogue writes the multi-level rank-band mask (bands lv), not the energy mask
  PredBands lv;
  int B, H, L, D, block, nb;
  float c;             // fp32(scale) * fp32(1.44269504), as the Triton kernel forms qk_scale
  float thr;
  int min_keep, max_keep, force_tail;
  void* po;
  uint8_t* mask;
  unsigned long long* count;
  int32_t* rows_kept;   // [B,H,nb] kept blocks per mask row (nullable)
  int dbg;   // diagnostic builds only (VB_DEBUG_PRED): 1 = skip epilogue, 2 = skip main loop, 4 = no MFMA, 8 = no energy rule
  RuleParams rule;   // kRule instantiations only
};

#ifndef VB_DIAG
#define VB_DIAG 0
#endif
// Diagnostic builds only (-DVB_PRED_TRACE=1: per-workgroup start/end times, tools/diag/pred_trace.py;
// -DVB_PRED_STAMPS=1: per-phase s_memtime sums, tools/diag/pred_stamps.py). The device globals they
// write live in vb_predict.hip, which defines VB_TRACE_START/VB_TRACE_END and VB_PRED_KERNEL_STAMPS
// before it includes this header: only that unit's kernels are instrumented, whatever the flags say.
#ifndef VB_TRACE_START
#define VB_TRACE_START(k)
#define VB_TRACE_END()
#endif
#ifndef VB_PRED_KERNEL_STAMPS
#define VB_PRED_KERNEL_STAMPS 0
#endif
#if VB_PRED_KERNEL_STAMPS
__device__ __forceinline__ unsigned long long pred_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define VB_PST(var) const unsigned long long var = pred_stamp()
#define VB_PST_SUM(i, cycles) pst[i] += (cycles)
#else
#define VB_PST(var)
#define VB_PST_SUM(i, cycles)
#endif

// caller row holding reordered-padded position `pos` of a (b,h) stream
__device__ __forceinline__ int sampled_row(int blk, int off, int block, int L, const int32_t* rows) {
  int pos = blk * block + off;
  pos = min(pos, L - 1);  // replicate padding (F.pad mode='replicate')
  return rows ? rows[pos] : pos;
}

// random_sample_tokens' topk (cogvideo_blocksparseattn.py:45-46) by one wave: the indices of the
// `keep` largest of n <= 256 uniforms r (global), in descending order of value, ties -> lower index
// first, written to dst[rank] (LDS or global). `sv` is LDS scratch for n floats.
__device__ __forceinline__ void topk_wave_lds(int n, int keep, int32_t* dst, const float* sv);
__device__ __forceinline__ void topk_wave(const float* r, int n, int keep, int32_t* dst, float* sv) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; i < n; i += 64) sv[i] = r[i];
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  topk_wave_lds(n, keep, dst, sv);
}

// torch.rand(B,H,1,block) on a device generator at Philox state (seed, offset), element base + t of
// the draw for t < n (PyTorch's uniform_: distribution_elementwise_grid_stride_kernel with one
// grid-stride pass, hiprand_init(seed, element, offset), the x of hiprand_uniform4, 1.0 -> 0.0),
// written to LDS sv[t] by one wave.
__device__ __forceinline__ void philox_draw_wave(unsigned long long seed, unsigned long long offset,
                                                 long long base, int n, float* sv) {
  const int lane = threadIdx.x & 63;
  for (int t = lane; t < n; t += 64) {
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, (unsigned long long)(base + t), offset, &st);
    const float u = rocrand_uniform4(&st).x;
    sv[t] = u == 1.0f ? 0.0f : u;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
}

// the rank loop of topk_wave on draws already in LDS sv[0..n)
__device__ __forceinline__ void topk_wave_lds(int n, int keep, int32_t* dst, const float* sv) {
  const int lane = threadIdx.x & 63;
  // the rank loop reads 4 draws per 16-byte LDS broadcast, 8 reads in flight: a one-float loop was
  // LDS-latency bound (~6 us of sample_rows_kernel's 10 us at the CogVideoX shape)
  const float4* s4 = reinterpret_cast<const float4*>(sv);
  const int n4 = n >> 2;
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    const float v = i < n ? sv[i] : 0.f;
    int rank = 0;
#pragma unroll 8
    for (int j4 = 0; j4 < n4; ++j4) {
      const float4 w = s4[j4];
      const int j = 4 * j4;
      rank += (w.x > v || (w.x == v && j < i)) ? 1 : 0;
      rank += (w.y > v || (w.y == v && j + 1 < i)) ? 1 : 0;
      rank += (w.z > v || (w.z == v && j + 2 < i)) ? 1 : 0;
      rank += (w.w > v || (w.w == v && j + 3 < i)) ? 1 : 0;
    }
    for (int j = 4 * n4; j < n; ++j) {
      const float w = sv[j];
      rank += (w > v || (w == v && j < i)) ? 1 : 0;
    }
    if (i < n && rank < keep) dst[rank] = i;
  }
}

// The sampled rows of k as a table of byte offsets, int32 [B,H,nb*keep], within the (b,h) slice of k
// (the score kernel gathers the rows themselves by LDS-DMA, and its prologue the q fragments, one row
// per lane); keep = kKeep sampled tokens per block: row j*keep + t of (b,h) = reordered position
// min(j*block + off[b,h,t], L-1) (replicate padding), at the caller's row rows[pos].
// grid (row chunks, B*H), one thread per sampled row. With rand_q/rand_k the offsets are drawn here first (topk_wave: one launch
// instead of two) and the first chunk of every (b,h) writes them out for the score kernel.
template <class T, int kKeep = 32>
__global__ void __launch_bounds__(256) sample_rows_kernel(const PredParams p) {
  __shared__ alignas(16) float sv[2][256];
  __shared__ int32_t koff_s[kKeep];
  const int bh = blockIdx.y;
  const int wave = threadIdx.x >> 6;
  const int32_t* koff = p.k_off + (int64_t)bh * kKeep;
  if (p.philox) {   // the two torch.rand draws generated here: q at offset, k at offset + 4
    if (wave == 0) {
      philox_draw_wave(p.philox_seed, p.philox_offset + 4, (long long)bh * p.block, p.block, sv[0]);
      topk_wave_lds(p.block, kKeep, koff_s, sv[0]);
    }
    if (blockIdx.x == 0 && wave == 1) {
      philox_draw_wave(p.philox_seed, p.philox_offset, (long long)bh * p.block, p.block, sv[1]);
      topk_wave_lds(p.block, kKeep, p.q_off + (int64_t)bh * kKeep, sv[1]);
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < kKeep) p.k_off[(int64_t)bh * kKeep + threadIdx.x] = koff_s[threadIdx.x];
    koff = koff_s;
  } else if (p.rand_k) {
    if (wave == 0) topk_wave(p.rand_k + (int64_t)bh * p.block, p.block, kKeep, koff_s, sv[0]);
    if (blockIdx.x == 0 && wave == 1)
      topk_wave(p.rand_q + (int64_t)bh * p.block, p.block, kKeep, p.q_off + (int64_t)bh * kKeep, sv[1]);
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x < kKeep) p.k_off[(int64_t)bh * kKeep + threadIdx.x] = koff_s[threadIdx.x];
    koff = koff_s;
  }
  const int jt = blockIdx.x * blockDim.x + threadIdx.x;
  if (jt >= p.nb * kKeep) return;
  constexpr int kKeepLog2 = kKeep == 16 ? 4 : kKeep == 32 ? 5 : 6;
  static_assert(kKeep == 1 << kKeepLog2, "sampling densities: 16, 32 or 64 tokens per block");
  int pos = min((jt >> kKeepLog2) * p.block + koff[jt & (kKeep - 1)], p.L - 1);
  if (p.rows) pos = p.rows[pos];
  p.k_row_off[(int64_t)bh * p.nb * kKeep + jt] =(int32_t)((int64_t)pos * p.ks[2] * 2);
}

// kLong: the instantiation behind vb_mask_predict_long. Only the epilogue differs: the per-wave row
// scratch holds kEnergyRowLong entries and the rank/cumsum code covers up to 16 values per lane.
//
// kKeep: sampled tokens per 128-token block (16, 32 or 64; the reference's num_keep). The sampled
// streams have nb*kKeep rows and the score loop runs over them in the same 32x32 MFMA tiles; what
// changes is which tile rows and lanes belong to one (q-block, key block) pair:
//   * 32: a wave's 32 query lanes are one q-block, a 32-key tile one key block.
//   * 64: a q-block is two 32-row groups (two neighbouring waves), a key block two 32-key tiles. The
//     block's row maximum is the maximum over both tiles (every lane ends up holding it); R is
//     [q-block][key block][64 rows], each wave storing its 32 rows; the even wave of a pair runs the
//     epilogue over both groups' rows and row maxima.
//   * 16: a 32x32 tile is two q-blocks (lanes 0-15 / 16-31 of each half) by two key blocks
//     (accumulator registers 0-7 / 8-15). One permlane32_swap of the two 8-register maxima gives
//     lanes 0-31 the first key block's row maximum and lanes 32-63 the second's; R is
//     [q-block][key block][16 rows]; a wave runs the epilogue of its two q-blocks in turn.
// The wave's unit of work is therefore a 32-row *group* of the sampled q stream (`qbs`, `ng` of them).
// kRule: the instantiations behind vb_mask_predict_rule (long ones). Only the last step of the epilogue
// differs: rule_row (per-head bounds, top-k mode) instead of energy_row with the call's scalars.
template <int D, class T, bool kLong = false, int kKeep = 32, bool kRule = false>
__global__ void __launch_bounds__(kPThreads, kPMinWg) mask_predict_kernel(const PredParams p) {
  static_assert(!kRule || kLong, "the rule instantiations are long ones");
  static_assert(kKeep == 16 || kKeep == 32 || kKeep == 64, "sampling densities: 16, 32 or 64 tokens per block");
  constexpr int KS = D / 16;
  constexpr int kRowB = D * 2;                        // bytes per key row
  constexpr int kKT = kKeysPerTile<D> / 32;          // sampled key blocks per tile
  constexpr int kTileBytes = kKeysPerTile<D> * kRowB;
  constexpr int kRowsPerInst = 1024 / kRowB;          // rows one 1-KiB LDS-DMA wave-instruction fills
  constexpr int kInstPerWave = kTileBytes / 1024 / kPWaves;
  constexpr int kBufs = kPBufs<D>;                    // tile t read, the younger ones in flight
  // 32-row groups of the sampled q stream per wave: one. The loops over KQ below have a single trip
  // and date from a build with two groups per wave; they stay because hipcc's code depends on them:
  // taking out any of six of the nine changes the kernel's instruction stream (the one round the
  // epilogue call by 2900 lines at kKeep 32), and the refactor that fixed the knobs was held to an
  // unchanged listing (tools/diag/listing_diff.py). Remove them together with a timed A/B.
  constexpr int KQ = 1;
  // R stores per wave and LDS tile: one per pair of 32-key tiles; at 16 one per 32-key tile
  constexpr int kSt = kKeep == 16 ? kKT : KQ * (kKT / 2);
  // LDS: m [4][32] f32 | K tiles x kBufs | row-offset ring (after the main loop: per-wave row
  // scratch). The per-row block maxima R go to a global scratch in [key block][32 rows] order (as the
  // Triton kernel keeps R in HBM): a tile's two columns are one contiguous 128-byte store, and the
  // LDS stays small enough for 3 workgroups per CU at any nb.
  // The first n_pool workgroups of the launch run the pooled K/V pass (HBM-bound) beside the score
  // workgroups (MFMA-bound): one launch, no second stream or events. n_pool is a multiple of 8, so
  // the score workgroups keep their XCD (blockIdx % 8).
  // kPoolLast<D>: the pooling workgroups come after the score workgroups instead, where they fill the
  // score kernel's partial last round.
  const bool pool_wg = kPoolLast<D> ? (int)blockIdx.x >= (int)gridDim.x - p.n_pool : (int)blockIdx.x < p.n_pool;
  if (pool_wg) {
    VB_TRACE_START(1);
    const int pw = kPoolLast<D> ? (int)blockIdx.x - ((int)gridDim.x - p.n_pool) : (int)blockIdx.x;
    const int64_t i0 = (int64_t)pw * blockDim.x + threadIdx.x, st = (int64_t)p.n_pool * blockDim.x;
    if (p.pool_kind == 2) kv_pyramid_span<D, T>(p.pyr, i0, st);
    else pool_kv_span<T>(p.pool, i0, st);
    VB_TRACE_END();
    return;
  }
  VB_TRACE_START(0);
  const int wg = kPoolLast<D> ? (int)blockIdx.x : (int)blockIdx.x - p.n_pool;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int nb = p.nb;
  float* mrow_s = reinterpret_cast<float*>(smem);
  uint8_t* ktile = smem + kPWaves * KQ * 32 * 4;
  float* rowbuf = reinterpret_cast<float*>(ktile);  // [4][2][kERow<kLong>], reused after the loop
  // the row scratch overlays the K ring and the row-offset ring behind it (36 KiB at D=64, 52 KiB at
  // D=128); both are idle after the main loop's final vmcnt(0) and barrier
  static_assert(kPWaves * 2 * kERow<kLong> * 4 <= kBufs * kTileBytes + 4 * kPWaves * 256,
                "the per-wave row scratch must fit in the K-tile ring it overlays");

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;
  // XCD-aware order: give each XCD a contiguous range of (head, q-group) work, so a head's sampled
  // keys are re-read from that XCD's own L2. Placement only affects speed.
  const int ng = kKeep == 64 ? 2 * nb : kKeep == 16 ? (nb + 1) >> 1 : nb;   // 32-row groups of the q stream
  const int nqg = (ng + kPWaves * KQ - 1) / (kPWaves * KQ);
  const int lin = xcd_linear(wg, nqg * p.B * p.H);
  const int bh = lin / nqg;
  int qbs[KQ];   // this wave's 32-row group of the sampled q stream (at kKeep 32: its q-block)
#pragma unroll
  for (int e = 0; e < KQ; ++e) qbs[e] = (lin % nqg) * kPWaves * KQ + wave * KQ + e;

  // Q fragment of this lane's sampled row (B operand of S^T = K_s . Q_s^T), gathered straight from
  // the caller's q: reordered-padded position qb*block + q_off[l32] (replicate padding) at row rows[pos]
  typename T::vec8 qf[KQ][KS];
#pragma unroll
  for (int e = 0; e < KQ; ++e) {
    const int b = bh / p.H, h = bh % p.H;
    // the lane's row of the sampled q stream is qbs[e]*32 + l32: q-block and token of that row
    const int qb_l = kKeep == 64 ? qbs[e] >> 1 : kKeep == 16 ? 2 * qbs[e] + (l32 >> 4) : qbs[e];
    const int qt_l = kKeep == 64 ? (qbs[e] & 1) * 32 + l32 : kKeep == 16 ? (l32 & 15) : l32;
    const int qrow = sampled_row(qb_l < nb ? qb_l : 0, p.q_off[(int64_t)bh * kKeep + qt_l], p.block, p.L, p.rows);
    const uint8_t* qp = reinterpret_cast<const uint8_t*>(p.q) + 2 * (b * p.qs[0] + h * p.qs[1] + (int64_t)qrow * p.qs[2]);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[e][s] = *reinterpret_cast<const typename T::vec8*>(qp + (16 * s + 8 * half) * 2);
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(qf[e][s]));  // see vb_attn_fwd.hip
  }
  // K tiles by LDS-DMA, gathered straight from the caller's k: the sampling launch wrote only the
  // byte offsets of the sampled rows within the (b,h) slice of k (int32 table [bh][nb*kKeep]). A
  // buffer descriptor per (b,h) slice; per tile each wave DMAs the offsets of its own rows into a
  // small LDS ring two tiles ahead (one 4-byte lane each, ordered so that lane L's four rows are 16
  // contiguous bytes), reads them back and issues the row DMAs with per-lane voffsets. Offsets past
  // the table (a partial last tile) read as 0: row 0, never used. 27 MB of row copies per CogVideoX
  // call are not made.
  static_assert(kBufs == 2 || kBufs == 3, "the gather pipeline's vmcnt counts assume a 2- or 3-slot K ring");
  constexpr int kChunks = kRowB / 16;
  const uint8_t* kslice = reinterpret_cast<const uint8_t*>(p.k) + 2 * ((bh / p.H) * p.ks[0] + (bh % p.H) * p.ks[1]);
  const srd_t ksrd = make_srd(kslice, (int)((int64_t)(p.L - 1) * p.ks[2] * 2 + kRowB));
  const srd_t isrd = make_srd(p.k_row_off + (int64_t)bh * nb * kKeep, nb * kKeep * 4);
  uint8_t* ibuf = ktile + kBufs * kTileBytes + wave * 256;   // [4 tiles][4 waves][64 dwords]
  int cv[kInstPerWave];   // the lane's swizzled chunk within its row, per DMA instruction
#pragma unroll
  for (int i = 0; i < kInstPerWave; ++i) {
    const int r = (wave * kInstPerWave + i) * kRowsPerInst + lane / kChunks;
    const int sw = (D == 64) ? ((r >> 1) & 7) : (r & 15);
    cv[i] = 16 * ((lane % kChunks) ^ sw);
  }
  // offset-DMA lane 4j + i fetches row (wave*kIPW + i)*kRowsPerInst + j of the tile (lanes past the
  // wave's rows repeat the last one)
  const int ivoff = 4 * ((wave * kInstPerWave + (lane & 3)) * kRowsPerInst + min(lane >> 2, kRowsPerInst - 1));
  float m[KQ];
#pragma unroll
  for (int e = 0; e < KQ; ++e) m[e] = -INFINITY;
  __syncthreads();   // all plain global loads retired before the DMA pipeline

  // LDS tiles of the nb*kKeep-row sampled K stream (kKT 32-key tiles each)
  const int nkt = kKeep == 64 ? 2 * nb : kKeep == 16 ? (nb + 1) >> 1 : nb;
  const int ntiles = (VB_DIAG && (p.dbg & 2)) ? 0 : (nkt + kKT - 1) / kKT;
  // K tile t by LDS-DMA (global_load_lds_dwordx4): the LDS image is written linearly (1 KiB per
  // wave-instruction), so the 16-byte-chunk XOR swizzle of the image is applied to each lane's
  // SOURCE address: LDS slot `sl` of row r holds chunk sl ^ sw(r).
  // offsets of tile t's rows -> LDS ring slot t & 3 (one instruction per wave; past the table: 0).
  // Four slots: the prologue has I0..I2 in flight at once, a body reads I(t+2) while I(t+3) lands.
  auto issue_idx = [&](int t) __attribute__((always_inline)) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(isrd.base), (short)0, isrd.bytes, 0x00020000),
        (__attribute__((address_space(3))) void*)(ibuf + (t & 3) * (kPWaves * 256)), 4, ivoff,
        __builtin_amdgcn_readfirstlane(t * kKeysPerTile<D> * 4), 0, 0);
  };
  // rows of tile t (offsets already in LDS) -> K ring slot t % kBufs
  auto issue = [&](int t) __attribute__((always_inline)) {
    uint8_t* dst = ktile + (t % kBufs) * kTileBytes;
    const i32x4 o = *reinterpret_cast<const i32x4*>(ibuf + (t & 3) * (kPWaves * 256) + 16 * (lane / kChunks));
#pragma unroll
    for (int i = 0; i < kInstPerWave; ++i) dma16(ksrd, dst + (wave * kInstPerWave + i) * 1024, o[i] + cv[i], 0);
  };
  // loop-invariant lane addresses of the K fragment reads (the swizzle depends on the lane's row
  // bits only), so every read of every slot is base + compile-time immediate
  int k_lane[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int sw = (D == 64) ? ((l32 >> 1) & 7) : (l32 & 15);
    k_lane[ks] = l32 * kRowB + 16 * ((2 * ks + half) ^ sw);
  }
  uint16_t* Rqs[KQ];   // this wave's group's R slice
  srd_t rsrd[KQ];
#pragma unroll
  for (int e = 0; e < KQ; ++e) {
    if constexpr (kKeep == 32) {
      Rqs[e] = p.rbuf + ((int64_t)bh * nb + (qbs[e] < nb ? qbs[e] : 0)) * nb * 32;
      rsrd[e] = make_srd(Rqs[e], qbs[e] < nb ? nb * 64 : 0);
    } else {
      // the slice of the group's first q-block; at 16 the descriptor spans the group's two q-blocks
      // (one when nb is odd and the group is the last: the lanes of the missing one fall outside)
      const int qb0 = kKeep == 64 ? qbs[e] >> 1 : 2 * qbs[e];
      const int nqb = kKeep == 64 ? 1 : min(2, nb - qb0);
      Rqs[e] = p.rbuf + ((int64_t)bh * nb + (qbs[e] < ng ? qb0 : 0)) * nb * kKeep;
      rsrd[e] = make_srd(Rqs[e], qbs[e] < ng ? nqb * nb * kKeep * 2 : 0);
    }
  }
  // the lane's byte offset within a key block's column of R (plus, at 16, its q-block's slice); lanes
  // that must not store get kNoStore, outside any descriptor whatever the tile's offset adds
  [[maybe_unused]] constexpr int kNoStore = 0x40000000;
  [[maybe_unused]] const int rv = kKeep == 64 ? ((qbs[0] & 1) * 32 + l32) * 2
               : kKeep == 16 ? ((l32 >> 4) * nb * 16 + half * 16 + (l32 & 15)) * 2 : lane * 2;
  // Issue order: I0 I1 I2 K0 K1, then per body t: I(t+3) K(t+2) [compute] S(t) — every DMA is
  // issued, past the last tile too (offsets past the table read 0: row 0 into a slot no tile reads
  // any more), so the counts below are constant. Body t needs K(t) and I(t+2); younger than I(t+2)
  // are K(t+1) and S(t-1) (for t = 0: only K1), so K(t+1) stays in flight.
  // 2-slot ring (36 KiB of LDS: four workgroups per CU): I0 I1 K0, then per body t: I(t+2) K(t+1)
  // [compute] S(t); K(t+1) can only go after the barrier that frees its slot, so a body waits for
  // its own K(t) with only S(t-1) younger.
  if (ntiles > 0) {
    if constexpr (kBufs == 2) {
      issue_idx(0);
      issue_idx(1);
      VB_WAIT_VMCNT(1);
      asm volatile("" ::: "memory");
      issue(0);
    } else {
      issue_idx(0);
      issue_idx(1);
      issue_idx(2);
      VB_WAIT_VMCNT(2);
      asm volatile("" ::: "memory");   // the offsets' LDS reads stay behind the wait
      issue(0);
      VB_WAIT_VMCNT(1 + kInstPerWave);
      asm volatile("" ::: "memory");
      issue(1);
    }
  }
#if VB_PRED_KERNEL_STAMPS
  unsigned long long pst[4] = {0, 0, 0, 0};
#endif
  auto halfmax = [&](const f32x16& a) __attribute__((always_inline)) -> float {
    float y = fmaxf(fmaxf(a[0], a[1]), a[2]);
#pragma unroll
    for (int r = 3; r < 15; r += 2) y = fmaxf(fmaxf(y, a[r]), a[r + 1]);
    return fmaxf(y, a[15]);
  };
  auto body = [&](int t, auto U) __attribute__((always_inline)) {
    constexpr int u = decltype(U)::value;
    VB_PST(b0);
    // vmcnt counts the R stores too, in issue order: every body issues exactly kSt of them
    if constexpr (kBufs == 2) {
      if (t == 0) VB_WAIT_VMCNT(0);
      else VB_WAIT_VMCNT(kSt);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      issue_idx(t + 2);
      issue(t + 1);
    } else {
      if (t == 0) VB_WAIT_VMCNT(kInstPerWave);
      else VB_WAIT_VMCNT(kInstPerWave + kSt);
      VB_PST(b1);
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      VB_PST(b2);
      issue_idx(t + 3);
      issue(t + 2);
      VB_PST(b3);
      VB_PST_SUM(0, b1 - b0);
      VB_PST_SUM(1, b2 - b1);
      VB_PST_SUM(2, b3 - b2);
    }
    const uint8_t* kl = ktile + u * kTileBytes;
    if (VB_DIAG && (p.dbg & 4)) return;   // diagnostic: stream the K tiles only
    // one accumulator per 32-key block: the MFMAs of block kt+1 do not wait for the row-max
    // reads of block kt (a shared accumulator serialises MFMA -> s_nop -> VALU -> MFMA)
    f32x16 sc[KQ][kKT];
#pragma unroll
    for (int kt = 0; kt < kKT; ++kt) {
      typename T::vec8 kf[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        kf[ks] = *reinterpret_cast<const typename T::vec8*>(kl + kt * 32 * kRowB + k_lane[ks]);
#pragma unroll
      for (int e = 0; e < KQ; ++e)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[e][kt][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int e = 0; e < KQ; ++e) sc[e][kt] = T::mfma32(kf[ks], qf[e][ks], sc[e][kt]);
    }
    // Pin the issue order: each K-fragment read kPSched MFMAs ahead of the MFMA that consumes
    // it (left alone, hipcc reuses one fragment register and serialises read -> wait -> MFMA).
#pragma unroll
    for (int i = 0; i < kPSched; ++i) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#pragma unroll
    for (int i = 0; i < kKT * KS; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x8, KQ, 0);
      if (i + kPSched < kKT * KS) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    // row maxima, two 32-key blocks per v_permlane32_swap: after the swap lanes 0-31 hold block
    // 2pr's full row max and lanes 32-63 block 2pr+1's (the halves of each block's C tile meet)
    const int j0 = kKT * t;
    constexpr int kPairs = kKT / 2;
    if constexpr (kKeep == 64) {
      // a key block is the pair of tiles 2pr, 2pr+1: the maximum over both tiles' registers, then
      // over the two lane halves, so every lane holds its query row's maximum over the block's 64 keys
#pragma unroll
      for (int pr = 0; pr < kPairs; ++pr) {
        const float x = fmaxf(halfmax(sc[0][2 * pr]), halfmax(sc[0][2 * pr + 1]));
        float mx = max_xor32(x) * p.c;
        const int jb = kPairs * t + pr;   // wave-uniform
        if (jb >= nb) mx = -INFINITY;     // partial last tile (D=64, odd nb)
        m[0] = fmaxf(m[0], mx);
        // R[jb][64 rows]: the wave's 32 rows (both halves store the same value to the same bytes).
        // One store per pair, issued unconditionally as below.
        store16(rsrd[0], (uint16_t)storage_bits<T>(mx), jb < nb ? rv : kNoStore, jb * 128);
      }
    } else if constexpr (kKeep == 16) {
      // a 32-key tile is two key blocks: accumulator registers 0-7 are key rows 0-15 of the tile (of
      // both halves), 8-15 rows 16-31. After the swap lanes 0-31 hold the first block's row maximum
      // and lanes 32-63 the second's, for query l32 (q-block 2g + (l32 >> 4), row l32 & 15).
#pragma unroll
      for (int kt = 0; kt < kKT; ++kt) {
        const f32x16& a = sc[0][kt];
        const float lo = fmaxf(fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3])), fmaxf(fmaxf(a[4], a[5]), fmaxf(a[6], a[7])));
        const float hi = fmaxf(fmaxf(fmaxf(a[8], a[9]), fmaxf(a[10], a[11])), fmaxf(fmaxf(a[12], a[13]), fmaxf(a[14], a[15])));
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo), __float_as_uint(hi), false, false);
        float mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * p.c;
        const int jb = 2 * (j0 + kt) + half;
        if (jb >= nb) mx = -INFINITY;   // half a tile of keys past an odd nb, and whole tiles past it
        m[0] = fmaxf(m[0], mx);         // this half's key blocks; halves meet below
        // R[q-block][jb][16 rows]: kKT stores per body, issued unconditionally; a lane whose key block
        // is past nb stores nowhere, one whose q-block is past nb falls outside the descriptor
        store16(rsrd[0], (uint16_t)storage_bits<T>(mx), jb < nb ? rv : kNoStore, (j0 + kt) * 64);
      }
    } else {
#pragma unroll
      for (int q = 0; q < KQ; ++q) {
        float mxp[kPairs];
#pragma unroll
        for (int pr = 0; pr < kPairs; ++pr) {
          const float x0 = halfmax(sc[q][2 * pr]), x1 = halfmax(sc[q][2 * pr + 1]);
          const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x0), __float_as_uint(x1), false, false);
          mxp[pr] = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])) * p.c;   // tl.max(qk, 1) * qk_scale
        }
        if (j0 + kKT > nb) {   // partial last tile: blocks past nb take no part (their rows are zeros)
          asm volatile("");
#pragma unroll
          for (int pr = 0; pr < kPairs; ++pr)
            if (j0 + 2 * pr + half >= nb) mxp[pr] = -INFINITY;
        }
#pragma unroll
        for (int pr = 0; pr < kPairs; ++pr) m[q] = fmaxf(m[q], mxp[pr]);   // this half's blocks; halves meet below
        // R[j][row]: lane (half, row) stores block j0 + 2pr + half, so one store writes 128 contiguous
        // bytes. Issued unconditionally (kSt per body, the vmcnt counts above rely on it): blocks past
        // nb fall outside the descriptor and an inactive q-block's descriptor is empty, so the hardware
        // drops those lanes.
#pragma unroll
        for (int pr = 0; pr < kPairs; ++pr) store16(rsrd[q], (uint16_t)storage_bits<T>(mxp[pr]), lane * 2, (j0 + 2 * pr) * 64);
      }
    }
    VB_PST(b4);
    VB_PST_SUM(3, b4 - b0);
  };
  // the loop body is instantiated once per ring slot
  for (int t0 = 0; t0 < ntiles; t0 += kBufs) {
    body(t0, std::integral_constant<int, 0>{});
    if (t0 + 1 < ntiles) body(t0 + 1, std::integral_constant<int, 1>{});
    if constexpr (kBufs == 3)
      if (t0 + 2 < ntiles) body(t0 + 2, std::integral_constant<int, 2>{});
  }

  VB_WAIT_VMCNT(0);   // the DMAs issued past the last tile land before the epilogue reuses the LDS
  VB_PST(e0);
#pragma unroll
  for (int e = 0; e < KQ; ++e) {
    m[e] = max_xor32(m[e]);   // the two halves saw alternate key blocks
    if (half == 0) mrow_s[(wave * KQ + e) * 32 + l32] = m[e];
  }
  __syncthreads();
  if (VB_DIAG && (p.dbg & 1)) return;

  // Po[qb, j] = storage(max_r exp2(R[r][j] - m_r)) = storage(exp2(max_r (R[r][j] - m_r)))
  // (exp2 and the rounding are monotone), then the storage-dtype row normalisation; one q-block
  // after the other (the wave's row scratch is reused)
  float* val = rowbuf + wave * 2 * (kERow<kLong>);
  uint32_t* keys = reinterpret_cast<uint32_t*>(val + kERow<kLong>);
  auto epilogue = [&](const int qb, const uint16_t* Rq, const float* mw) __attribute__((always_inline)) {
    // this wave's R columns were stored by its own lanes: wait for them and drop any stale L1 line
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    // the q-block's kKeep rows in sweeps of kER: at 64 the first sweep leaves max_r (R - m_r) over
    // rows 0-31 in val[], the second joins rows 32-63 (the other wave's, behind the barrier above)
    constexpr int kER = kKeep == 16 ? 16 : 32;
    float part = 0.f;
#pragma unroll
    for (int sw = 0; sw < kKeep / kER; ++sw) {
      float mreg[kER];
#pragma unroll
      for (int r = 0; r < kER; r += 4) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(mw + kER * sw + r);
#pragma unroll
        for (int e = 0; e < 4; ++e) mreg[r + e] = x[e];
      }
      // kPRCols columns per lane per pass (4 loads each in flight): the block's 32 row maxima
      // are 64 contiguous bytes
      constexpr int kRC = kPRCols;
      for (int j0 = 0; j0 < nb; j0 += 64 * kRC) {
        u32x4 w[kRC][kER / 8];
#pragma unroll
        for (int h = 0; h < kRC; ++h) {
          const int jj = min(j0 + 64 * h + lane, nb - 1);
#pragma unroll
          for (int c = 0; c < kER / 8; ++c) w[h][c] = reinterpret_cast<const u32x4*>(Rq + jj * kKeep + kER * sw)[c];
        }
#pragma unroll
        for (int h = 0; h < kRC; ++h) {
          const int j = j0 + 64 * h + lane;
          float cm = -INFINITY;
#pragma unroll
          for (int c = 0; c < kER / 8; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = 8 * c + 2 * e;
              cm = max3f(cm, T::bits_to_f32((uint16_t)(w[h][c][e] & 0xFFFF)) - mreg[r],
                         T::bits_to_f32((uint16_t)(w[h][c][e] >> 16)) - mreg[r + 1]);
            }
          if constexpr (kKeep == 64) {
            if (sw == 0) {
              if (j < nb) val[j] = cm;
              continue;
            }
            if (j < nb) cm = fmaxf(cm, val[j]);
          }
          cm = round_to<T>(exp2_fast(cm));
          if (j < nb) {
            val[j] = cm;
            part += cm;
          }
        }
      }
    }
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    const float tot = round_to<T>(part);
    typename T::raw* po = reinterpret_cast<typename T::raw*>(p.po) + ((int64_t)bh * nb + qb) * nb;
    for (int j = lane; j < nb; j += 64) {
      const float v = round_to<T>(val[j] / tot);
      val[j] = v;
      po[j] = T::from_f32(v);
    }
#if VB_PRED_KERNEL_STAMPS
    {
      VB_PST(e1);
      if (lane == 0) {
        for (int i = 0; i < 4; ++i) atomicAdd(&g_pred_stamp[i], pst[i]);
        atomicAdd(&g_pred_stamp[4], e1 - e0);
        atomicAdd(&g_pred_stamp[5], 1ull);
      }
    }
#endif
    if (p.mask == nullptr) return;   // scores only
    if (VB_DIAG && (p.dbg & 8)) return;   // diagnostic: no energy rule (Po written)
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    uint8_t* mrow = p.mask + ((int64_t)bh * nb + qb) * nb;
    if (p.level) {   // the multi-level path's rank bands instead of the energy rule
      level_row<T, kLong>(val, keys, mrow, nb, qb, p.lv);
      return;
    }
    const bool force_all = p.force_tail > 0 && qb >= nb - p.force_tail;
    int kept;
    if constexpr (kRule)
      kept = rule_row<T>(p.rule, bh, val, keys, mrow, nb, nb, p.thr, p.min_keep, p.max_keep, p.force_tail, force_all);
    else
      kept = energy_row<T, kLong>(val, keys, mrow, nb, p.thr, p.min_keep, p.max_keep, p.force_tail, force_all);
    if (p.count && lane == 0) atomicAdd(p.count, (unsigned long long)kept);
    if (p.rows_kept && lane == 0) p.rows_kept[(int64_t)bh * nb + qb] = kept;
  };
  if constexpr (kKeep == 64) {
    // the even wave of a pair holds the q-block's rows 0-31, its neighbour rows 32-63 (ng is even, so
    // both are live); their row maxima are 64 consecutive floats of mrow_s. The neighbour's R stores
    // were retired (vmcnt(0)) before the barrier above.
    if (qbs[0] < ng && !(wave & 1)) epilogue(qbs[0] >> 1, Rqs[0], mrow_s + wave * 32);
  } else if constexpr (kKeep == 16) {
    for (int s = 0; s < 2; ++s)   // the group's two q-blocks: rows 16s.. of the tile
      if (2 * qbs[0] + s < nb) epilogue(2 * qbs[0] + s, Rqs[0] + s * nb * 16, mrow_s + wave * 32 + 16 * s);
  } else {
#pragma unroll
    for (int e = 0; e < KQ; ++e)
      if (qbs[e] < nb) epilogue(qbs[e], Rqs[e], mrow_s + (wave * KQ + e) * 32);
  }
  VB_TRACE_END();
}

// dynamic LDS of the score kernel: the row maxima, then the K ring with the row-offset ring behind
// it or, where that is larger, the epilogue's row scratch that overlays both
static size_t predict_smem_bytes(int D, bool long_rows) {
  const size_t tiles = D == 64 ? (size_t)kPBufs<64> * kKeysPerTile<64> * 64 * 2
                               : (size_t)kPBufs<128> * kKeysPerTile<128> * 128 * 2;
  const size_t scratch = (size_t)kPWaves * 2 * (long_rows ? kEnergyRowLong : kEnergyRow) * 4;
  const size_t ring = 4 * kPWaves * 256;
  const size_t mrow = (size_t)kPWaves * 32 * 4;
  return mrow + (tiles + ring > scratch ? tiles + ring : scratch);
}

// the sampling launch, `staged` (nullable) recorded behind it, then the score kernel
template <int D, class T, bool kLong, int kKeep = 32, bool kRule = false>
static int launch_predict(const PredParams& p, hipStream_t stream, hipEvent_t staged) {
  const size_t smem = predict_smem_bytes(D, kLong);
  auto kern = mask_predict_kernel<D, T, kLong, kKeep, kRule>;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)smem) != hipSuccess)
    return fail(VB_ERR_LAUNCH, "mask_predict: cannot reserve LDS");
  hipLaunchKernelGGL((sample_rows_kernel<T, kKeep>), dim3((unsigned)((p.nb * kKeep + 255) / 256), (unsigned)(p.B * p.H)),
                     dim3(256), 0, stream, p);
  if (int rc = check_launch("sample_rows_kernel")) return rc;
  if (staged && hipEventRecord(staged, stream) != hipSuccess) return fail(VB_ERR_LAUNCH, "vb_mask_predict: hipEventRecord failed");
  const int ng = (p.nb * kKeep + 31) / 32;   // 32-row groups of the sampled q stream, one per wave
  const dim3 grid(((ng + kPWaves - 1) / kPWaves) * p.B * p.H + p.n_pool);
  hipLaunchKernelGGL(kern, grid, dim3(kPThreads), smem, stream, p);
  return check_launch("mask_predict_kernel");
}

// the rule instantiations (long kernels, every head dim, dtype and sampling density): vb_predict_rule.hip
int launch_predict_rule(const PredParams& p, int dtype, int keep, hipStream_t s, hipEvent_t ev);

}  // namespace vb

