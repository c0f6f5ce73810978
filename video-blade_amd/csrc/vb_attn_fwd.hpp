// Parameter block, build constants, LDS images, work-item decode and launchers shared by the
// block-sparse attention forward: the kernels (vb_attn_fwd.hip) and the host layer that validates,
// fills the parameters and sequences the launches (vb_attn_fwd_host.cpp).
#pragma once
#include "vb_tiles.hpp"

namespace vb {

struct FwdParams {
  const void* q; const void* k; const void* v;
  int64_t qs[3], ks[3], vs[3];
  const int32_t* q_rows; const int32_t* kv_rows;
  const int32_t* cu_q; const int32_t* cu_k;   // varlen row offsets (reference API), nullable
  const int32_t* head_mask_type;              // reference API, nullable
  int hm_mode;                                // VB_MASK_HEAD_PER_HEAD / VB_MASK_HEAD_SHARED0
  int use_main;
  const uint8_t* mask; int64_t ms[3];
  const void* kp; const void* vp; int64_t kps[3], vps[3];
  int Lkp; float pool_bias_l2;                 // bias in the exp2 domain (log2 gap)
  void* out; int64_t os[3];
  float* lse; int64_t lse_s[2];               // row stride 1
  int B, H, Lq, Lk, nbq, nbk;
  float c;                                    // softmax scale * log2(e)
  int heavy_rows;                             // last q-block rows known to be dense (scheduling hint)
  const int32_t* q_order;                     // phase-2 dispatch order (attn_order_kernel), or NULL
  const int32_t* q_len;                       // kept key blocks per mask row (ordering input), or NULL
  int order_window;                           // re-order only the last N items of each XCD range (0: all)
  // multi-level mode (vb_ml_attn_fwd): k/v are the KV pyramids [B,H,15*Lpad/8,D]
  int Lpad;                                   // level-1 rows (ceil(L/128)*128)
  int ref_tail;                               // 1: level-1 tail keys >= L take part (zero rows)
  int* work_queue;                            // persistent dispatch: per-XCD queue heads, or NULL
  int n_items;                                // work items (nbq * B * H) behind the queue
};

constexpr int kThreads = 256;
constexpr int kQBlk = 128;   // rows per workgroup (4 waves x 32)
constexpr int kKT = 64;      // keys per LDS tile
constexpr int kMaxBlocks = 1024;  // keys <= 131072

// ---- build constants of the forward kernel, each with the measurement that fixed it ----------------
namespace fwd {
// V^T k-steps prefetched before the softmax (D=64); 4 under the iterative-ilp scheduler (attention
// kernel 1.016-1.030x on three boxes, bit-identical; 3 was best before it)
constexpr int kVPre64 = 4;
// the same for the launches that gather K/V rows through the Gilbert index: 4 spills a DMA offset
// into their tile-issue blocks (tests/test_codegen.py)
constexpr int kVPre64Rows = 3;
// Split P.V: the P.V of a tile's first 32 keys is issued before the exp of its second 32. D=64 only:
// measured +0.8 % at D=64 (VALU-issue-bound loop) and -1.4 % at D=128.
constexpr bool split_pv(int D) { return D == 64; }
// Inference loop: s_setprio 1 around parts of the tile (bit 0: the S MFMA chain, bit 1: each P.V
// k-step's MFMAs, bit 2: the exp/pack of a half-tile); 0 = never. `tools/ab.py --what attn`, r02: the
// LSE-returning D=128 loop with 1 / 3 / 7 measured 1.00x / 0.97x / 0.98x (it has none)
constexpr int kPrio64 = 0;    // measured (CogVideoX, 3 waves per SIMD): 1 -2.6 %, 2 -0.6 %, 4 -4.1 %, 5 -6.2 %
constexpr int kPrio128 = 3;   // measured (Wan, 2 waves per SIMD): 3 +4.1/+4.5 %, 1 +2.5/+5.6 %, 7 +4.2 %, 2 -2.6 %, 4 +0.0 %
// the Q fragment loaded after the ring's first DMAs (their round trips overlap), per launch form.
// Measured (tools/ab.py, r06, profiles/r06_qlate_ab.log, against the first item-loop build): D=64
// attention 1.044-1.048x, its LSE launch 1.058x; D=128 LSE launch 1.047-1.049x, the inference launch
// on gathered K/V (Wan's module path) 1.001-1.003x per call, on Gilbert copies 0.98x (kept off
// there). On the final tree the CogVideoX call runs 1.002x with it (profiles/r06_fwd_retune_ab.log)
constexpr bool kQLate64 = true;
constexpr bool kQLate128 = true;
constexpr bool kQLate128Lazy = false;   // D=128 inference launch on contiguous (copied) K/V
constexpr int kWavesD64 = 3;            // waves per SIMD the D=64 kernel is register-budgeted for
constexpr float kRescaleSlack = 4.0f;   // log2 units: P <= 16 between rescales of the training loop
}  // namespace fwd
// lazy-max mode: a half-tile row sum (>= each of its P) above this raises m. bf16 P: with
// P <= 2^32, O and l stay below 2^32 * Lk * max|V| (Lk <= 2^17): no overflow for any |V| < 2^78.
// f16 P (max 65504): P <= 2^8, so P keeps the same normal range below it as P <= 1 does.
constexpr float kLazyBoundBF16 = 4294967296.0f;
constexpr float kLazyBoundF16 = 256.0f;

// ---- LDS images --------------------------------------------------------------------------------
// K: [64 rows][D] with 16-byte chunks XOR-swizzled so a ds_read_b128 column slice (32 rows, one
//    chunk) hits 16 distinct bank slots per lane group (guide T2).
template <int D>
__device__ __forceinline__ int k_off(int row, int ch) {
  constexpr int kRowBytes = D * 2;
  const int sw = (D == 64) ? ((row >> 1) & 7) : (row & 15);
  return row * kRowBytes + 16 * (ch ^ sw);
}
// V: [64 rows][D] row-major, 64-byte granules XOR-swizzled so the 4-row x 64-byte footprint of
//    a half-wave's ds_read_b64_tr_b16 covers a full 256-byte bank row.
template <int D>
__device__ __forceinline__ int v_off_bytes(int row, int col) {
  constexpr int kRowBytes = D * 2;
  const int g = col >> 5;
  const int sw = (D == 64) ? ((row >> 1) & 1) : (row & 3);
  return row * kRowBytes + 64 * (g ^ sw) + (col & 31) * 2;
}

// Describes where tile t's keys come from.
struct TileSrc {
  int pooled;   // 0 = main (block-masked) keys, 1 = pooled keys
  int kstart;   // first key (reordered index for main, pooled index otherwise)
  int klen;     // valid keys in this tile (1..64)
};

// Multi-level tile: 64 pyramid rows of one level. The rows this wave's LDS-DMA fills (its half of
// the tile, 32 rows) come as two 16-row quarters starting at pyramid rows srcA and srcB: a level-8
// block is 16 rows, a level-4 block 32, levels 1/2 are contiguous.
struct MlTileSrc {
  int srcA, srcB;   // pyramid rows of this wave's first and second 16-row quarter
  int klen;         // valid keys in this tile (1..64); the rest are masked
  int lvl;          // log2 of the level: the logit bias in the exp2 domain
};

// ---- work-item decode ------------------------------------------------------------------------------
// Work order (placement only affects speed, never results). Workgroups are dealt round-robin over
// the 8 XCDs (blockIdx % 8 share one XCD and its 4 MiB L2).
//  phase 1: the `heavy_rows` last q-block rows of every head (CogVideoX's dense text rows, the
//           longest workgroups) go first, spread over all XCDs;
//  phase 2: every XCD takes a contiguous, head-major range of the remaining (head, q-block) work
//           (xcd_linear), so the pooled K/V and the kept K/V blocks of the one or two heads an XCD
//           is working on are re-read from its own L2 instead of the Infinity Cache / HBM.
// Phase-2 linear index -> (b*H + h, q-block): head-major, a head's q-blocks in descending order
__device__ __forceinline__ void fwd_phase2_item(int lin, int rows_left, int& bh, int& qblk) {
  bh = lin / rows_left;
  qblk = rows_left - 1 - lin % rows_left;
}
// work item `vblk` (a blockIdx, or a work-queue item) -> (b*H + h, q-block)
__device__ __forceinline__ void fwd_item_decode(const FwdParams& p, int vblk, int& bh, int& qblk) {
  const int BH = p.B * p.H;
  const int hr = min(p.heavy_rows, p.nbq);
  const int n_heavy = hr * BH;
  if (vblk < n_heavy) {
    qblk = p.nbq - 1 - vblk / BH;
    bh = vblk % BH;
  } else {
    const int rows_left = p.nbq - hr;
    int lin = xcd_linear(vblk - n_heavy, rows_left * BH);
    if (p.q_order) lin = __builtin_amdgcn_readfirstlane(p.q_order[lin]);   // longest first (attn_order_kernel)
    fwd_phase2_item(lin, rows_left, bh, qblk);
  }
}

// ---- launchers (vb_attn_fwd.hip): each returns 0 or a VB_ERR code; D and dtype already validated ----
// the block-sparse forward (pooled branch with `pool`; the inference kernel when p.lse is NULL)
int launch_fwd(const FwdParams& p, int D, int dtype, bool pool, hipStream_t stream);
// its multi-level form (k/v = the KV pyramids, mask = the level mask)
int launch_ml_fwd(const FwdParams& p, int D, int dtype, hipStream_t stream);
// the longest-first dispatch order of phase 2 into order[rows_left * B * H]
int launch_attn_order(const FwdParams& p, int32_t* order, hipStream_t stream);

}  // namespace vb
