// Parameter blocks, build constants, work-item decode and launchers shared by the block-sparse FMHA
// backward: the kernels (vb_attn_bwd.hip, vb_attn_bwd_kv.hip) and the host layer that validates,
// lays out the workspace and sequences the launches (vb_attn_bwd_host.cpp). See vb_attn_bwd.hip for
// the algorithm.
#pragma once
#include "vb_tiles.hpp"

namespace vb {

namespace bwd {
constexpr int kThreads = 256;
constexpr int kBlk = 128;       // mask block (rows and keys)
constexpr int kT = 64;          // rows (dkdv) / keys (dq) per LDS tile
constexpr int kMaxBlocks = 1024;
constexpr float kBigL = 1.0e30f;  // L' of rows that must contribute nothing (exp2(s - 1e30) = 0)

// ---- register budgets and priorities of the compiler-scheduled kernels (vb_attn_bwd.hip) ----------
// s_setprio 1 around the MFMA chains of the dK/dV kernel (bit 0: S and dP, bit 1: the dV/dK steps)
constexpr int kDkdvPrio64 = 1;    // measured (cog backward): 1 1.013x, 3 1.009x
constexpr int kDkdvPrio128 = 0;   // one wave per SIMD at D=128: nothing to arbitrate
constexpr int kDkdvWavesD64 = 2;  // waves per SIMD the D=64 dK/dV kernel is register-budgeted for
// waves per multi-level pooled dK/dV workgroup at D=64: 2 = 64-row items on a 2-slot ring, four
// workgroups per CU (vb_ml_attn_bwd 1.15x over 4 = 128-row items, dk bit-identical;
// profiles/archive/r05_ml_bwd_pyr2_ab.log). D=128 keeps 4 (two waves spill there).
constexpr int kMlPyrWaves = 2;
// dQ, D=128: two waves per SIMD with a 2-slot ring (over one wave on a 3-slot ring: Wan backward
// 1.014-1.018x)
constexpr int kDqWavesD128 = 2;
constexpr int kDqWavesD64 = 2;    // waves per SIMD the D=64 dQ kernel is register-budgeted for
// s_setprio 1 around the MFMA chains of the dQ kernel (bit 0: S and dP, bit 1: the dQ steps)
constexpr int kDqPrio64 = 0;      // measured (cog backward): 1 0.990x, 3 0.990x
constexpr int kDqPrio128 = 1;     // measured (Wan backward, two waves per SIMD): 1 1.096x, 3 1.094x
// ---- the hand-placed streams (vb_attn_bwd_kv.hip) ------------------------------------------------
constexpr int kKv64Waves = 1;     // waves per SIMD the D=64 stream kernels are register-budgeted for (2 spills)
constexpr int kKvLA = 4;          // operand lookahead in MFMAs (dK/dV, and the 4-slot dQ)
constexpr int kDq2LA = 2;         // operand lookahead of the 2-slot dQ pipeline
constexpr int kDq64R2Wgs = 2;     // workgroups per CU the D=64 2-slot dQ is register-budgeted for (3: 1.005x)
}  // namespace bwd

struct PrepParams {
  const void* q; const void* dout; const void* out; const void* out2;
  int64_t qs[3], dos[3], os[3], o2s[3];
  const float* lse; const float* lse2; const float* alpha;  // [B,H,Lq] at the caller's row
  const int32_t* q_rows; const int32_t* cu_q;
  void* q_r; void* do_r;  // [B,H,Lq,D] contiguous reordered copies (written when q_rows != NULL)
  float* stats;           // [B*H][ntile][4][64]: L'1, -Delta1, L'2, -Delta2
  int B, H, Lq, D, ntile;
  // vb_attn_bwd_joint: out / lse are those of the ONE softmax over kept keys and biased pooled keys,
  // pool_log_bias its bias (out2, lse2 and alpha are NULL and never read)
  float pool_log_bias;
};

struct BwdParams {
  const void* q; const void* dout; int64_t qs[3], dos[3];  // row g of (b,h) at qrow0 + g
  const void* k; const void* v; int64_t ks[3], vs[3];
  const void* kp; const void* vp; int64_t kps[3], vps[3];
  int Lkp;
  const int32_t* cu_q; const int32_t* cu_k; const int32_t* head_mask_type;
  int hm_mode;   // VB_MASK_HEAD_PER_HEAD / VB_MASK_HEAD_SHARED0 (head_mask_base)
  const uint8_t* mask; int64_t ms[3];
  const float* stats; int ntile;
  void* dq; int64_t dqs[3]; const int32_t* q_rows;
  void* dk; void* dv; int64_t dks[3], dvs[3]; const int32_t* kv_rows;
  float* dkp; float* dvp;  // [B,H,Lkp,D] fp32 pooled-key grads
  int psplit;              // pooled-key workgroups split the q-blocks in psplit ranges...
  float* dkp_part; float* dvp_part;  // ...into [psplit][B,H,Lkp,D] partials (== dkp/dvp if 1)
  int gap;
  int B, H, Lq, Lk, nbq, nbk, nbkp;
  float c;      // scale * log2(e)
  float scale;
  int heavy_rows;
  // multi-level mode (vb_ml_attn_bwd): k/v are the KV pyramids [B,H,15*Lpad/8,D] (contiguous),
  // mask the level mask; the pooled levels' pyramid-row grads go to dkpyr/dvpyr fp32
  // [B,H,7*Lpad/8,D] (level 2 rows, then level 4, then level 8)
  int Lpad;
  int ref_tail;
  float* dkpyr; float* dvpyr;
};

// multi-level geometry shared by the backward kernels: pyramid level regions (rows) and the
// pooled-level work items of the dK/dV pass (one 128-row pyramid block each)
struct MlGeom {
  int nb, Lpad, off[4];   // level-1/2/4/8 region starts in the pyramid
  int nblk[4];            // 128-row pyramid blocks per level: ceil(nb / p)
  __device__ __forceinline__ MlGeom(int Lpad_) {
    Lpad = Lpad_;
    nb = Lpad / 128;
    off[0] = 0; off[1] = Lpad; off[2] = Lpad + Lpad / 2; off[3] = off[2] + Lpad / 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) nblk[e] = (nb + (1 << e) - 1) >> e;
  }
};

// ---- work-item decode shared by the round-3 kernels and the hand-placed streams -------------------
// a varlen batch entry's own lengths and first rows (cu_q / cu_k), else the padded ones
__device__ __forceinline__ void seq_bounds(const BwdParams& p, int b, int& Lq, int& Lk, int64_t& qrow0,
                                           int64_t& krow0) {
  Lq = p.Lq; Lk = p.Lk;
  qrow0 = 0; krow0 = 0;
  if (p.cu_q) {
    qrow0 = p.cu_q[b]; Lq = p.cu_q[b + 1] - p.cu_q[b];
    krow0 = p.cu_k[b]; Lk = p.cu_k[b + 1] - p.cu_k[b];
  }
}
// dK/dV workgroup -> (b*H + h, key block) over nkb key blocks per head.
// Pooled-key blocks see every q-block: their work is split into psplit q-block ranges (split
// innermost, so a key block's workgroups run together).
// Main blocks: the `heavy_rows` last key blocks of every head (CogVideoX's forced dense text
// columns, kept by every q-block: ~8x the average column's tiles) go first over all XCDs, then
// each XCD takes a contiguous head-major range with key blocks in descending order. Ascending
// order put every head's two heavy columns at the end of its range, so the last head of each
// XCD's range left a long tail (measured: 1.26 waves per SIMD on average at 2 possible).
template <bool kPooled, bool kML>
__device__ __forceinline__ void dkdv_item(const BwdParams& p, int BH, int nkb, int& bh, int& kblk) {
  if (kPooled) {
    const int lin = (int)blockIdx.x / p.psplit;
    bh = lin / nkb;
    kblk = lin % nkb;
  } else {
    const int hr = kML ? 0 : min(p.heavy_rows, nkb);
    const int n_heavy = hr * BH;
    if ((int)blockIdx.x < n_heavy) {
      kblk = nkb - 1 - (int)(blockIdx.x / BH);
      bh = blockIdx.x % BH;
    } else {
      const int cols_left = nkb - hr;
      const int lin = xcd_linear(blockIdx.x - n_heavy, cols_left * BH);
      bh = lin / cols_left;
      kblk = cols_left - 1 - lin % cols_left;
    }
  }
}
// dQ workgroup -> (b*H + h, q-block): heavy-first, then XCD-contiguous head-major (as the forward)
__device__ __forceinline__ void dq_item(const BwdParams& p, int BH, int& bh, int& qblk) {
  const int hr = min(p.heavy_rows, p.nbq);
  const int n_heavy = hr * BH;
  if ((int)blockIdx.x < n_heavy) {
    qblk = p.nbq - 1 - (int)(blockIdx.x / BH);
    bh = blockIdx.x % BH;
  } else {
    const int rows_left = p.nbq - hr;
    const int lin = xcd_linear(blockIdx.x - n_heavy, rows_left * BH);
    bh = lin / rows_left;
    qblk = rows_left - 1 - lin % rows_left;
  }
}

// ---- launchers: each returns 0 or a VB_ERR code; dtype is VB_DTYPE_BF16 / VB_DTYPE_F16 -------------
// vb_attn_bwd.hip (compiler-scheduled)
// joint: the statistics of vb_attn_bwd_joint (PrepParams::pool_log_bias) instead of the two-branch ones
int launch_prep(const PrepParams& pp, int dtype, bool joint, hipStream_t s);
// the round-3 dK/dV: pooled-key pass (grid nbkp * B*H * psplit) or full-resolution (grid nbk * B*H)
int launch_dkdv_round3(const BwdParams& p, int D, int dtype, bool pooled, hipStream_t s);
// the multi-level level-1 dK/dV on the round-3 kernel
int launch_ml_dkdv_round3(const BwdParams& p, int D, int dtype, hipStream_t s);
// the round-3 dQ (grid nbq * B*H), and its multi-level form
int launch_dq_round3(const BwdParams& p, int D, int dtype, bool pool, hipStream_t s);
int launch_ml_dq_round3(const BwdParams& p, int D, int dtype, hipStream_t s);
// dkp/dvp = the sum of the psplit pooled-key partials
int launch_pool_grad_reduce(const BwdParams& p, int D, hipStream_t s);
// the multi-level pyramid pass: the pooled levels' dK/dV into dkpyr/dvpyr
int launch_ml_pyramid(const BwdParams& p, int D, int dtype, hipStream_t s);
// vb_attn_bwd_kv.hip (hand-placed streams): dK/dV, `pooled` as above
int launch_dkdv_pipe(const BwdParams& p, int D, int dtype, bool pooled, hipStream_t s);
// dQ on the 2-slot ring, or the 4-slot one (VB_BWD_SEL_DQ_RING4)
int launch_dq_pipe(const BwdParams& p, int D, int dtype, bool pool, bool ring4, hipStream_t s);
// the multi-level dQ on the 2-slot pipeline (vb_ml_attn_bwd)
int launch_ml_dq_pipe(const BwdParams& p, int D, int dtype, hipStream_t s);
// the multi-level level-1 dK/dV on the pipeline kernel
int launch_ml_dkdv_pipe(const BwdParams& p, int D, int dtype, hipStream_t s);

}  // namespace vb
