// Host layer of the block-sparse FMHA backward: argument validation, workspace layout, parameter
// fill and launch sequencing of vb_attn_bwd, vb_attn_bwd_joint, vb_block_sparse_attn_bwd and vb_ml_attn_bwd. The
// kernels and their launchers are in vb_attn_bwd.hip (compiler-scheduled) and vb_attn_bwd_kv.hip
// (hand-placed streams); nothing here is compiled with their per-file flags.
#include <map>
#include <mutex>

#include "vb_args.hpp"
#include "vb_attn_bwd.hpp"

namespace vb {
namespace {

// dQ depends only on the prep kernel's row statistics; the dK/dV chain (pooled keys, their reduce,
// main keys) never reads dQ. So dQ is launched on a per-device side stream that waits for the
// caller's stream at the fork and is joined back (an event) before the call returns: the two
// launches fill each other's last rounds and the chain's small launches. Work and results are
// unchanged (no atomics, disjoint outputs). Graph capture: the side stream joins the caller's
// capture through the event wait. The mutex keeps one call's record/wait pairs together.
// Measured (tools/ab.py, profiles/r06_bwd_fork_ab.log): Wan backward 1.016-1.019x, CogVideoX
// 0.998-1.000x, the multi-level backward 0.987-0.990x, so only the D=128 main backward forks.
struct BwdFork {
  hipStream_t side = nullptr;
  hipEvent_t forked = nullptr, joined = nullptr;
};
class ForkScope {
 public:
  ForkScope(hipStream_t s, bool enable) : s_(s), lock_(mu(), std::defer_lock) {
    if (!enable) return;
    lock_.lock();
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return;
    BwdFork& f = forks()[dev];
    if (!f.side) {
      if (hipStreamCreateWithFlags(&f.side, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&f.forked, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&f.joined, hipEventDisableTiming) != hipSuccess) {
        f = BwdFork{};
        return;   // no side stream: everything stays on the caller's stream
      }
    }
    if (hipEventRecord(f.forked, s) != hipSuccess || hipStreamWaitEvent(f.side, f.forked, 0) != hipSuccess) return;
    f_ = &f;
  }
  ~ForkScope() {
    if (f_ && hipEventRecord(f_->joined, f_->side) == hipSuccess) (void)hipStreamWaitEvent(s_, f_->joined, 0);
  }
  hipStream_t dq_stream() const { return f_ ? f_->side : s_; }
  bool forked() const { return f_ != nullptr; }

 private:
  static std::mutex& mu() {
    static std::mutex m;
    return m;
  }
  static std::map<int, BwdFork>& forks() {
    static std::map<int, BwdFork> m;
    return m;
  }
  hipStream_t s_;
  std::unique_lock<std::mutex> lock_;   // held from the fork to the join (the destructor's event wait)
  BwdFork* f_ = nullptr;
};

// ---- workspace: 256-byte aligned regions, in this order ---------------------------------------------
//   stats [B*H][ntile64][4][64] f32 | q_r, do_r [B,H,Lq,D] (reordered copies, with q_rows) |
//   main backward, pooled: dkp, dvp [B,H,Lkp,D] f32, then (psplit > 1) their [psplit] partials |
//   multi-level: dkpyr, dvpyr [B,H,7*Lpad/8,D] f32
struct WsLayout {
  uint64_t stats, q_r, do_r, dkp, dvp, dkp_part, dvp_part, dkpyr, dvpyr, total;
  int psplit;
};
struct WsCursor {
  uint64_t off = 0;
  uint64_t take(uint64_t bytes) {
    const uint64_t at = off;
    off = round_up256(off + bytes);
    return at;
  }
};
// the regions every backward starts with
WsCursor ws_head(WsLayout& w, int B, int H, int Lq, int D, bool copies) {
  WsCursor c;
  w = WsLayout{};
  w.psplit = 1;
  w.stats = c.take((uint64_t)B * H * ((Lq + 63) / 64) * 256 * 4);
  if (copies) {
    w.q_r = c.take((uint64_t)B * H * Lq * D * 2);
    w.do_r = c.take((uint64_t)B * H * Lq * D * 2);
  }
  return c;
}
// pooled-key q-range split: aim at ~3k workgroups per sample for the pooled dK/dV pass. The split
// sets the order of the partial sums, so it does not depend on B: a sample's gradients are the
// same bits in any batch (the B=5 training-batch test).
int pool_split(int H, int Lq, int Lkp) {
  if (Lkp <= 0) return 1;
  const int nbkp = (Lkp + 127) / 128, nbq = (Lq + 127) / 128;
  const int wg = nbkp * H;
  const int s = (3072 + wg / 2) / wg;
  return s < 1 ? 1 : (s > nbq ? nbq : s);
}
WsLayout ws_layout(int B, int H, int Lq, int D, bool copies, int Lkp) {
  WsLayout w;
  WsCursor c = ws_head(w, B, H, Lq, D, copies);
  w.psplit = pool_split(H, Lq, Lkp);
  if (Lkp > 0) {
    const uint64_t grads = (uint64_t)B * H * Lkp * D * 4;
    w.dkp_part = w.dkp = c.take(grads);
    w.dvp_part = w.dvp = c.take(grads);
    if (w.psplit > 1) {
      w.dkp_part = c.take(w.psplit * grads);
      w.dvp_part = c.take(w.psplit * grads);
    }
  }
  w.total = c.off;
  return w;
}
WsLayout ml_ws_layout(int B, int H, int L, int D, bool copies) {
  WsLayout w;
  WsCursor c = ws_head(w, B, H, L, D, copies);
  const uint64_t lpad = (uint64_t)(L + 127) / 128 * 128;
  w.dkpyr = c.take((uint64_t)B * H * (7 * lpad / 8) * D * 4);
  w.dvpyr = c.take((uint64_t)B * H * (7 * lpad / 8) * D * 4);
  w.total = c.off;
  return w;
}

// ---- parameter fill shared by the entries -----------------------------------------------------------
void copy3(int64_t* dst, const int64_t* src) {
  for (int i = 0; i < 3; ++i) dst[i] = src[i];
}
// The prep kernel's inputs and the q / dO the gradient kernels read: with q_rows the prep kernel
// writes reordered contiguous copies into the workspace (one gather pass instead of one per key
// block that reads them) and the gradient kernels read those.
void fill_q_side(PrepParams& pp, BwdParams& p, uint8_t* ws, const WsLayout& w, const void* q, const int64_t* q_stride,
                 const void* dout, const int64_t* dout_stride, const int32_t* q_rows, int B, int H, int Lq, int D) {
  pp.q = q; pp.dout = dout;
  copy3(pp.qs, q_stride); copy3(pp.dos, dout_stride);
  pp.q_rows = q_rows;
  pp.stats = reinterpret_cast<float*>(ws + w.stats);
  pp.B = B; pp.H = H; pp.Lq = Lq; pp.D = D; pp.ntile = (Lq + 63) / 64;
  if (q_rows) {
    pp.q_r = ws + w.q_r; pp.do_r = ws + w.do_r;
    p.q = pp.q_r; p.dout = pp.do_r;
    p.qs[0] = p.dos[0] = (int64_t)H * Lq * D;
    p.qs[1] = p.dos[1] = (int64_t)Lq * D;
    p.qs[2] = p.dos[2] = D;
  } else {
    p.q = q; p.dout = dout;
    copy3(p.qs, q_stride); copy3(p.dos, dout_stride);
  }
  p.stats = pp.stats; p.ntile = pp.ntile;
  p.q_rows = q_rows;
  p.B = B; p.H = H; p.Lq = Lq;
}
void fill_scale(BwdParams& p, float scale, int D) {
  p.scale = scale_or_default(scale, D);
  p.c = p.scale * kLog2e;
}

// ---- launch sequencing: kernel choice is kernel_select (VB_BWD_SEL_* bits); `ran` collects the
// VB_BWD_RAN_* bits of what was launched -------------------------------------------------------------
int launch_dq(const BwdParams& p, int D, int dtype, bool pool, hipStream_t s, int sel, int& ran) {
  if (sel & VB_BWD_SEL_DQ_ROUND3) {
    ran |= VB_BWD_RAN_DQ_ROUND3;
    return launch_dq_round3(p, D, dtype, pool, s);
  }
  const bool ring4 = sel & VB_BWD_SEL_DQ_RING4;
  ran |= ring4 ? VB_BWD_RAN_DQ_PIPE_RING4 : VB_BWD_RAN_DQ_PIPE_RING2;
  return launch_dq_pipe(p, D, dtype, pool, ring4, s);
}
int launch_dkdv(const BwdParams& p, int D, int dtype, bool pooled, bool pipe, hipStream_t s) {
  return pipe ? launch_dkdv_pipe(p, D, dtype, pooled, s) : launch_dkdv_round3(p, D, dtype, pooled, s);
}

// joint: the prep launch writes vb_attn_bwd_joint's statistics; the gradient launches are the same
int launch_grads(const PrepParams& pp, const BwdParams& p, int D, int dtype, bool pool, hipStream_t s, int sel,
                 int& ran, bool joint = false) {
  if (int rc = launch_prep(pp, dtype, joint, s)) return rc;
  const bool pipe = !(sel & VB_BWD_SEL_DKDV_ROUND3);
  if ((pool && p.dkp) || p.k) ran |= pipe ? VB_BWD_RAN_DKDV_PIPE : VB_BWD_RAN_DKDV_ROUND3;
  ForkScope fork(s, D == 128);
  if (fork.forked())   // dQ first, on the side stream
    if (int rc = launch_dq(p, D, dtype, pool, fork.dq_stream(), sel, ran)) return rc;
  if (pool && p.dkp) {
    if (int rc = launch_dkdv(p, D, dtype, true, pipe, s)) return rc;
    if (p.psplit > 1)
      if (int rc = launch_pool_grad_reduce(p, D, s)) return rc;
  }
  if (p.k)
    if (int rc = launch_dkdv(p, D, dtype, false, pipe, s)) return rc;
  return fork.forked() ? 0 : launch_dq(p, D, dtype, pool, s, sel, ran);
}

int launch_ml_grads(const PrepParams& pp, const BwdParams& p, int D, int dtype, hipStream_t s, int sel, int& ran) {
  if (int rc = launch_prep(pp, dtype, false, s)) return rc;
  ran |= VB_BWD_RAN_ML_PYRAMID;
  // dQ stays last on the caller's stream: forked beside the pyramid and level-1 passes it measured
  // 0.987-0.990x (ForkScope)
  if (int rc = launch_ml_pyramid(p, D, dtype, s)) return rc;
  if (!(sel & VB_BWD_SEL_DKDV_ROUND3)) {
    ran |= VB_BWD_RAN_DKDV_PIPE;
    if (int rc = launch_ml_dkdv_pipe(p, D, dtype, s)) return rc;
  } else {
    ran |= VB_BWD_RAN_DKDV_ROUND3;
    if (int rc = launch_ml_dkdv_round3(p, D, dtype, s)) return rc;
  }
  if (!(sel & VB_BWD_SEL_DQ_ROUND3)) {
    ran |= VB_BWD_RAN_DQ_PIPE_RING2;
    return launch_ml_dq_pipe(p, D, dtype, s);
  }
  ran |= VB_BWD_RAN_DQ_ROUND3;
  return launch_ml_dq_round3(p, D, dtype, s);
}

}  // namespace
}  // namespace vb

extern "C" uint64_t vb_attn_bwd_workspace_size(const vb_attn_bwd_args* a) {
  if (!a) return 0;
  return vb::ws_layout(a->B, a->H, a->Lq, a->D, a->q_rows != nullptr, a->kp ? a->Lkp : 0).total;
}

namespace vb {
namespace {
// vb_attn_bwd (joint = false) and vb_attn_bwd_joint: `entry` names the call in the messages
int attn_bwd(const vb_attn_bwd_args* a, bool joint, float pool_log_bias, void* stream, const std::string& entry) {
  if (!a) return fail(VB_ERR_INVALID, entry + ": null args");
  if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->Lk <= 0 || a->D <= 0)
    return fail(VB_ERR_INVALID, entry + ": B, H, Lq, Lk, D must be positive");
  if (!head_dim_ok(a->D))
    return fail(VB_ERR_UNSUPPORTED, entry + ": head_dim must be 64 or 128, got " + std::to_string(a->D));
  if (!dtype_ok(a->dtype)) return fail(VB_ERR_INVALID, entry + ": unknown dtype");
  if (!a->q || !a->k || !a->v || !a->out || !a->lse || !a->dout || !a->dq || !a->dk || !a->dv)
    return fail(VB_ERR_INVALID, entry + ": missing tensor");
  if (a->kernel_select & ~(VB_BWD_SEL_DKDV_ROUND3 | VB_BWD_SEL_DQ_ROUND3 | VB_BWD_SEL_DQ_RING4))
    return fail(VB_ERR_INVALID, entry + ": unknown kernel_select bits");
  const bool pool = a->kp != nullptr;
  if (joint) {
    if (!pool || !a->vp || a->Lkp <= 0 || a->pool_gap <= 0)
      return fail(VB_ERR_INVALID, entry + ": needs the pooled keys kp, vp, Lkp > 0 and pool_gap > 0");
    if (a->out2 || a->lse2 || a->alpha)
      return fail(VB_ERR_INVALID, entry + ": out2, lse2 and alpha must be NULL (one softmax has one output and one LSE)");
  } else if (pool && (!a->vp || a->Lkp <= 0 || !a->out2 || !a->lse2 || a->pool_gap <= 0))
    return fail(VB_ERR_INVALID, entry + ": pooled branch needs vp, Lkp, out2, lse2 and pool_gap");
  if (pool && (int64_t)a->Lkp * a->pool_gap < a->Lk)
    return fail(VB_ERR_INVALID, entry + ": Lkp * pool_gap must cover Lk");
  const int nbk = (a->Lk + 127) / 128;
  const int nbq = (a->Lq + 127) / 128;
  if (nbk > bwd::kMaxBlocks || nbq > bwd::kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, entry + ": sequence too long");
  const int64_t* strides[] = {a->q_stride, a->k_stride, a->v_stride, a->out_stride, a->dout_stride,
                              a->dq_stride, a->dk_stride, a->dv_stride};
  for (const int64_t* s : strides)
    if (!strides_mul8(s)) return fail(VB_ERR_INVALID, entry + ": strides must be multiples of 8 elements");
  if (pool && (!strides_mul8(a->kp_stride) || !strides_mul8(a->vp_stride) ||
               (!joint && !strides_mul8(a->out2_stride))))
    return fail(VB_ERR_INVALID, entry + ": strides must be multiples of 8 elements");
  const void* ptrs[] = {a->q, a->k, a->v, a->out, a->dout, a->dq, a->dk, a->dv};
  for (const void* q : ptrs)
    if (!aligned16(q)) return fail(VB_ERR_INVALID, entry + ": tensors must be 16-byte aligned");
  if (pool && (!aligned16(a->kp) || !aligned16(a->vp) || !aligned16(a->out2)))
    return fail(VB_ERR_INVALID, entry + ": tensors must be 16-byte aligned");
  const WsLayout w = ws_layout(a->B, a->H, a->Lq, a->D, a->q_rows != nullptr, pool ? a->Lkp : 0);
  if (!a->workspace || a->workspace_bytes < w.total || !aligned16(a->workspace))
    return fail(VB_ERR_INVALID, entry + ": workspace missing or smaller than vb_attn_bwd_workspace_size()");
  if (!a->q_rows && (!slice_fits32(a->Lq, a->q_stride[2], a->D) || !slice_fits32(a->Lq, a->dout_stride[2], a->D)))
    return fail(VB_ERR_UNSUPPORTED, entry + ": a q/dout (b,h) slice spans >= 2 GiB");
  if (!slice_fits32(a->Lk, a->k_stride[2], a->D) || !slice_fits32(a->Lk, a->v_stride[2], a->D) ||
      (pool && (!slice_fits32(a->Lkp, a->kp_stride[2], a->D) || !slice_fits32(a->Lkp, a->vp_stride[2], a->D))))
    return fail(VB_ERR_UNSUPPORTED, entry + ": a k/v/kp/vp (b,h) slice spans >= 2 GiB");
  uint8_t* ws = reinterpret_cast<uint8_t*>(a->workspace);

  PrepParams pp{};
  BwdParams p{};
  fill_q_side(pp, p, ws, w, a->q, a->q_stride, a->dout, a->dout_stride, a->q_rows, a->B, a->H, a->Lq, a->D);
  pp.out = a->out; copy3(pp.os, a->out_stride);
  pp.lse = a->lse; pp.alpha = a->alpha;
  pp.pool_log_bias = pool_log_bias;
  p.k = a->k; p.v = a->v;
  copy3(p.ks, a->k_stride); copy3(p.vs, a->v_stride);
  copy3(p.ms, a->mask_stride);
  copy3(p.dqs, a->dq_stride); copy3(p.dks, a->dk_stride); copy3(p.dvs, a->dv_stride);
  p.mask = a->block_mask;
  p.dq = a->dq; p.dk = a->dk; p.dv = a->dv; p.kv_rows = a->kv_rows;
  p.psplit = 1;
  p.gap = 1;
  if (pool) {
    if (!joint) {
      pp.out2 = a->out2; copy3(pp.o2s, a->out2_stride);
      pp.lse2 = a->lse2;
    }
    p.kp = a->kp; p.vp = a->vp; p.Lkp = a->Lkp;
    copy3(p.kps, a->kp_stride); copy3(p.vps, a->vp_stride);
    p.dkp = reinterpret_cast<float*>(ws + w.dkp); p.dvp = reinterpret_cast<float*>(ws + w.dvp);
    p.psplit = w.psplit;
    p.dkp_part = reinterpret_cast<float*>(ws + w.dkp_part); p.dvp_part = reinterpret_cast<float*>(ws + w.dvp_part);
    p.gap = a->pool_gap;
    p.nbkp = (a->Lkp + 127) / 128;
  }
  p.Lk = a->Lk; p.nbq = nbq; p.nbk = nbk;
  fill_scale(p, a->scale, a->D);
  p.heavy_rows = a->heavy_rows;
  int ran = 0;
  const int rc = launch_grads(pp, p, a->D, a->dtype, pool, reinterpret_cast<hipStream_t>(stream), a->kernel_select, ran,
                              joint);
  if (a->kernels_ran) *a->kernels_ran = ran;
  return rc;
}
}  // namespace
}  // namespace vb

extern "C" int vb_attn_bwd(const vb_attn_bwd_args* a, void* stream) {
  return vb::attn_bwd(a, false, 0.f, stream, "vb_attn_bwd");
}

extern "C" int vb_attn_bwd_joint(const vb_attn_bwd_args* a, float pool_log_bias, void* stream) {
  return vb::attn_bwd(a, true, pool_log_bias, stream, "vb_attn_bwd_joint");
}

extern "C" uint64_t vb_block_sparse_attn_bwd_workspace_size(int batch, int num_heads, int max_seqlen_q) {
  if (batch <= 0 || num_heads <= 0 || max_seqlen_q <= 0) return 0;
  return vb::ws_layout(batch, num_heads, max_seqlen_q, 64, false, 0).total;
}

extern "C" int vb_block_sparse_attn_bwd(const void* dout, const void* q_unpad, const void* k_unpad,
                                        const void* v_unpad, const void* out_unpad, const float* softmax_lse,
                                        const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                                        const int32_t* head_mask_type, const int32_t* streaming_info,
                                        const uint8_t* base_blockmask, int batch, int num_heads, int head_dim,
                                        int max_seqlen_q, int max_seqlen_k, float p_dropout, float softmax_scale,
                                        int is_causal, int exact_streaming, int deterministic, int dtype,
                                        void* dq, void* dk, void* dv, void* workspace, uint64_t workspace_bytes,
                                        int mask_head_mode, void* stream) {
  using namespace vb;
  (void)streaming_info;
  (void)deterministic;  // always deterministic (no atomics)
  if (p_dropout != 0.f) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_bwd: p_dropout must be 0");
  if (is_causal || exact_streaming) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_bwd: causal/streaming not supported");
  if (mask_head_mode != VB_MASK_HEAD_PER_HEAD && mask_head_mode != VB_MASK_HEAD_SHARED0)
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_bwd: unknown mask_head_mode");
  if (!dout || !q_unpad || !k_unpad || !v_unpad || !out_unpad || !softmax_lse || !cu_seqlens_q || !cu_seqlens_k ||
      !dq || !dk || !dv)
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_bwd: null tensor");
  if (batch <= 0 || num_heads <= 0 || max_seqlen_q <= 0 || max_seqlen_k <= 0)
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_bwd: bad sizes");
  if (!head_dim_ok(head_dim)) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_bwd: head_dim must be 64 or 128");
  if (!dtype_ok(dtype)) return fail(VB_ERR_INVALID, "vb_block_sparse_attn_bwd: unknown dtype");
  const int nbq = (max_seqlen_q + 127) / 128;
  const int nbk = (max_seqlen_k + 127) / 128;
  if (nbk > bwd::kMaxBlocks || nbq > bwd::kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_bwd: sequence too long");
  const WsLayout w = ws_layout(batch, num_heads, max_seqlen_q, head_dim, false, 0);
  if (!workspace || workspace_bytes < w.total || !aligned16(workspace))
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_bwd: workspace missing or too small");
  const int64_t row = (int64_t)num_heads * head_dim;
  if (!slice_fits32(max_seqlen_q, row, head_dim))
    return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_bwd: a sequence's q/dout span >= 2 GiB");
  if (!slice_fits32(max_seqlen_k, row, head_dim))
    return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_bwd: a sequence's k/v span >= 2 GiB");
  const void* ptrs[] = {dout, q_unpad, k_unpad, v_unpad, out_unpad, dq, dk, dv};
  for (const void* q : ptrs)
    if (!aligned16(q)) return fail(VB_ERR_INVALID, "vb_block_sparse_attn_bwd: tensors must be 16-byte aligned");
  const int64_t s3[3] = {0, head_dim, row};   // unpadded [tokens, H, D]: a batch entry starts at its cu_seqlens row

  PrepParams pp{};
  BwdParams p{};
  fill_q_side(pp, p, reinterpret_cast<uint8_t*>(workspace), w, q_unpad, s3, dout, s3, nullptr, batch, num_heads,
              max_seqlen_q, head_dim);
  pp.out = out_unpad; copy3(pp.os, s3);
  pp.lse = softmax_lse;
  pp.cu_q = cu_seqlens_q;
  p.k = k_unpad; p.v = v_unpad;
  copy3(p.ks, s3); copy3(p.vs, s3); copy3(p.dqs, s3); copy3(p.dks, s3); copy3(p.dvs, s3);
  p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k; p.head_mask_type = head_mask_type;
  p.hm_mode = mask_head_mode;
  p.mask = base_blockmask;
  p.ms[0] = head_mask_type ? -1 : (int64_t)num_heads * nbq * nbk;
  p.ms[1] = (int64_t)nbq * nbk; p.ms[2] = nbk;
  p.dq = dq; p.dk = dk; p.dv = dv;
  p.gap = 1;
  p.psplit = 1;
  p.Lk = max_seqlen_k; p.nbq = nbq; p.nbk = nbk;
  fill_scale(p, softmax_scale, head_dim);
  int ran = 0;
  return launch_grads(pp, p, head_dim, dtype, false, reinterpret_cast<hipStream_t>(stream), 0, ran);
}

// ------------------------------------------------------------------------------------------------
// multi-level backward (kernels/block_sparse_attn_kernel_with_backward_9_10.py _backward :1375-1576)
// ------------------------------------------------------------------------------------------------
extern "C" uint64_t vb_ml_attn_bwd_workspace_size(const vb_ml_attn_bwd_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->L <= 0 || a->D <= 0) return 0;
  return vb::ml_ws_layout(a->B, a->H, a->L, a->D, a->rows != nullptr).total;
}

extern "C" int vb_ml_attn_bwd(const vb_ml_attn_bwd_args* a, void* stream) {
  using namespace vb;
  if (!a) return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: null args");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: B, H, L must be positive");
  if (!head_dim_ok(a->D))
    return fail(VB_ERR_UNSUPPORTED, "vb_ml_attn_bwd: head_dim must be 64 or 128, got " + std::to_string(a->D));
  if (!dtype_ok(a->dtype)) return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: unknown dtype");
  if (!a->q || !a->kpyr || !a->vpyr || !a->level_mask || !a->out || !a->lse || !a->dout || !a->dq || !a->dk || !a->dv)
    return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: missing tensor");
  if (a->kernel_select & ~(VB_BWD_SEL_DKDV_ROUND3 | VB_BWD_SEL_DQ_ROUND3))
    return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: unsupported kernel_select bits (the multi-level dQ has one ring)");
  const int nb = (a->L + 127) / 128;
  if (nb > bwd::kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, "vb_ml_attn_bwd: sequence too long");
  const int64_t* strides[] = {a->q_stride, a->out_stride, a->dout_stride, a->dq_stride, a->dk_stride, a->dv_stride};
  for (const int64_t* st : strides)
    if (!strides_mul8(st)) return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: strides must be multiples of 8 elements");
  const void* ptrs[] = {a->q, a->kpyr, a->vpyr, a->out, a->dout, a->dq, a->dk, a->dv};
  for (const void* q : ptrs)
    if (!aligned16(q)) return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: tensors must be 16-byte aligned");
  const WsLayout w = ml_ws_layout(a->B, a->H, a->L, a->D, a->rows != nullptr);
  if (!a->workspace || a->workspace_bytes < w.total || !aligned16(a->workspace))
    return fail(VB_ERR_INVALID, "vb_ml_attn_bwd: workspace missing or smaller than vb_ml_attn_bwd_workspace_size()");
  if (!a->rows && (!slice_fits32(a->L, a->q_stride[2], a->D) || !slice_fits32(a->L, a->dout_stride[2], a->D)))
    return fail(VB_ERR_UNSUPPORTED, "vb_ml_attn_bwd: a q/dout (b,h) slice spans >= 2 GiB");
  if ((int64_t)vb_kv_pyramid_rows(a->L) * 2 * a->D >= (int64_t(1) << 31))
    return fail(VB_ERR_UNSUPPORTED, "vb_ml_attn_bwd: a pyramid (b,h) slice spans >= 2 GiB");
  uint8_t* ws = reinterpret_cast<uint8_t*>(a->workspace);
  const int Lpad = nb * 128;
  const int R = 15 * (Lpad / 8);

  PrepParams pp{};
  BwdParams p{};
  fill_q_side(pp, p, ws, w, a->q, a->q_stride, a->dout, a->dout_stride, a->rows, a->B, a->H, a->L, a->D);
  pp.out = a->out; copy3(pp.os, a->out_stride);
  pp.lse = a->lse;
  p.k = a->kpyr; p.v = a->vpyr;
  p.ks[0] = p.vs[0] = (int64_t)a->H * R * a->D;
  p.ks[1] = p.vs[1] = (int64_t)R * a->D;
  p.ks[2] = p.vs[2] = a->D;
  copy3(p.ms, a->mask_stride);
  copy3(p.dqs, a->dq_stride); copy3(p.dks, a->dk_stride); copy3(p.dvs, a->dv_stride);
  p.mask = a->level_mask;
  p.dq = a->dq; p.dk = a->dk; p.dv = a->dv; p.kv_rows = a->rows;
  p.psplit = 1;
  p.gap = 1;
  p.Lk = a->L; p.nbq = nb; p.nbk = nb;
  p.nbkp = (nb + 1) / 2 + (nb + 3) / 4 + (nb + 7) / 8;
  p.Lpad = Lpad;
  p.ref_tail = a->ref_tail ? 1 : 0;
  p.dkpyr = reinterpret_cast<float*>(ws + w.dkpyr);
  p.dvpyr = reinterpret_cast<float*>(ws + w.dvpyr);
  fill_scale(p, a->scale, a->D);
  p.heavy_rows = a->heavy_rows;
  int ran = 0;
  const int rc = launch_ml_grads(pp, p, a->D, a->dtype, reinterpret_cast<hipStream_t>(stream), a->kernel_select, ran);
  if (a->kernels_ran) *a->kernels_ran = ran;
  return rc;
}
