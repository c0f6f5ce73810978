// Host layer of the block-sparse FMHA forward: argument validation, parameter fill and launch
// sequencing of vb_attn_fwd, vb_ml_attn_fwd and vb_block_sparse_attn_fwd. The kernels and their
// launchers are in vb_attn_fwd.hip; nothing here is compiled with that file's flags.
#include "vb_args.hpp"
#include "vb_attn_fwd.hpp"

namespace vb {
namespace {

void copy3(int64_t* dst, const int64_t* src) {
  for (int i = 0; i < 3; ++i) dst[i] = src[i];
}
// what every entry fills the same way: sizes, the [B,H,Lq] LSE output and the softmax scale
void fill_shape(FwdParams& p, int B, int H, int Lq, int Lk, int nbq, int nbk, int D, float scale, float* lse) {
  p.B = B; p.H = H; p.Lq = Lq; p.Lk = Lk; p.nbq = nbq; p.nbk = nbk;
  p.lse = lse;
  p.lse_s[0] = (int64_t)H * Lq; p.lse_s[1] = Lq;
  p.c = scale_or_default(scale, D) * kLog2e;
}
// vb_attn_fwd and vb_block_sparse_attn_fwd: dtype, then head_dim, then the launch
int check_and_launch(const FwdParams& p, int D, int dtype, bool pool, hipStream_t stream) {
  if (!dtype_ok(dtype)) return fail(VB_ERR_INVALID, "attn: unknown dtype");
  if (!head_dim_ok(D)) return fail(VB_ERR_UNSUPPORTED, "attn: head_dim must be 64 or 128, got " + std::to_string(D));
  return launch_fwd(p, D, dtype, pool, stream);
}

}  // namespace
}  // namespace vb

extern "C" int vb_attn_fwd(const vb_attn_args* a, void* stream) {
  using namespace vb;
  if (!a) return fail(VB_ERR_INVALID, "vb_attn_fwd: null args");
  if (a->B <= 0 || a->H <= 0 || a->Lq <= 0 || a->D <= 0)
    return fail(VB_ERR_INVALID, "vb_attn_fwd: B, H, Lq, D must be positive");
  if (!a->q || !a->out || (a->use_main && (!a->k || !a->v || a->Lk <= 0)))
    return fail(VB_ERR_INVALID, "vb_attn_fwd: missing q/k/v/out");
  const bool pool = a->kp != nullptr;
  if (!a->use_main && !pool) return fail(VB_ERR_INVALID, "vb_attn_fwd: nothing to attend to");
  if (pool && (!a->vp || a->Lkp <= 0)) return fail(VB_ERR_INVALID, "vb_attn_fwd: pooled branch needs vp and Lkp > 0");
  const int nbq = (a->Lq + kQBlk - 1) / kQBlk;
  const int nbk = a->use_main ? (a->Lk + kQBlk - 1) / kQBlk : 0;
  if (nbk > kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, "vb_attn_fwd: Lk too long");
  for (int i = 0; i < 3; ++i) {
    if ((a->q_stride[i] | a->out_stride[i]) & 7) return fail(VB_ERR_INVALID, "vb_attn_fwd: q/out strides must be multiples of 8 elements");
    if (a->use_main && ((a->k_stride[i] | a->v_stride[i]) & 7)) return fail(VB_ERR_INVALID, "vb_attn_fwd: k/v strides must be multiples of 8 elements");
    if (pool && ((a->kp_stride[i] | a->vp_stride[i]) & 7)) return fail(VB_ERR_INVALID, "vb_attn_fwd: kp/vp strides must be multiples of 8 elements");
  }
  // reachable only without the main branch (with it, "Lk too long" already refused such an Lk)
  if (a->kv_rows && a->Lk >= (1 << 24))
    return fail(VB_ERR_UNSUPPORTED, "vb_attn_fwd: kv_rows needs Lk < 2^24");
  // the tile DMA offsets use 24-bit multiplies: row strides below 2^24 bytes (16 MiB per row)
  if ((a->use_main && (a->k_stride[2] * 2 >= (1 << 24) || a->v_stride[2] * 2 >= (1 << 24))) ||
      (pool && (a->kp_stride[2] * 2 >= (1 << 24) || a->vp_stride[2] * 2 >= (1 << 24))))
    return fail(VB_ERR_UNSUPPORTED, "vb_attn_fwd: k/v/kp/vp row strides must be < 2^24 bytes");
  if (a->use_main && (!slice_fits32(a->Lk, a->k_stride[2], a->D) || !slice_fits32(a->Lk, a->v_stride[2], a->D)))
    return fail(VB_ERR_UNSUPPORTED, "vb_attn_fwd: a k/v (b,h) slice spans >= 2 GiB");
  if (pool && (!slice_fits32(a->Lkp, a->kp_stride[2], a->D) || !slice_fits32(a->Lkp, a->vp_stride[2], a->D)))
    return fail(VB_ERR_UNSUPPORTED, "vb_attn_fwd: a kp/vp (b,h) slice spans >= 2 GiB");
  if (!aligned16(a->q) || !aligned16(a->out) || (a->use_main && (!aligned16(a->k) || !aligned16(a->v))) ||
      (pool && (!aligned16(a->kp) || !aligned16(a->vp))))
    return fail(VB_ERR_INVALID, "vb_attn_fwd: tensors must be 16-byte aligned");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  FwdParams p{};
  p.q = a->q; p.k = a->k; p.v = a->v; p.out = a->out;
  copy3(p.qs, a->q_stride); copy3(p.ks, a->k_stride); copy3(p.vs, a->v_stride); copy3(p.os, a->out_stride);
  copy3(p.ms, a->mask_stride); copy3(p.kps, a->kp_stride); copy3(p.vps, a->vp_stride);
  p.q_rows = a->q_rows; p.kv_rows = a->kv_rows;
  p.use_main = a->use_main;
  p.mask = a->block_mask;
  p.kp = a->kp; p.vp = a->vp; p.Lkp = a->Lkp;
  p.pool_bias_l2 = a->kp_log_bias * kLog2e;
  fill_shape(p, a->B, a->H, a->Lq, a->use_main ? a->Lk : 1, nbq, nbk, a->D, a->scale, a->lse);
  p.heavy_rows = a->heavy_rows;
  p.q_len = a->q_lengths;
  p.order_window = a->order_window;
  p.work_queue = a->work_queue;
  if (a->q_order && p.use_main && p.mask) {   // longest-first dispatch order (scheduling only)
    if (int rc = launch_attn_order(p, a->q_order, st)) return rc;
    p.q_order = a->q_order;
  }
  return check_and_launch(p, a->D, a->dtype, pool, st);
}

extern "C" int vb_kv_pyramid_rows(int L) {
  const int lpad = (L + vb::kQBlk - 1) / vb::kQBlk * vb::kQBlk;
  return 15 * (lpad / 8);
}

extern "C" int vb_ml_attn_fwd(const vb_ml_attn_args* a, void* stream) {
  using namespace vb;
  if (!a) return fail(VB_ERR_INVALID, "vb_ml_attn_fwd: null args");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, "vb_ml_attn_fwd: B, H, L must be positive");
  if (!a->q || !a->kpyr || !a->vpyr || !a->level_mask || !a->out)
    return fail(VB_ERR_INVALID, "vb_ml_attn_fwd: missing q/kpyr/vpyr/level_mask/out");
  if (!head_dim_ok(a->D))
    return fail(VB_ERR_UNSUPPORTED, "vb_ml_attn_fwd: head_dim must be 64 or 128, got " + std::to_string(a->D));
  const int nb = (a->L + kQBlk - 1) / kQBlk;
  if (nb > kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, "vb_ml_attn_fwd: L too long");
  for (int i = 0; i < 3; ++i)
    if ((a->q_stride[i] | a->out_stride[i]) & 7) return fail(VB_ERR_INVALID, "vb_ml_attn_fwd: q/out strides must be multiples of 8 elements");
  // a pyramid (b,h) slice always fits a 32-bit buffer offset: at most 15 * 1024 * 16 rows of 256 bytes
  const int R = vb_kv_pyramid_rows(a->L);
  if (!aligned16(a->q) || !aligned16(a->out) || !aligned16(a->kpyr) || !aligned16(a->vpyr))
    return fail(VB_ERR_INVALID, "vb_ml_attn_fwd: tensors must be 16-byte aligned");
  FwdParams p{};
  p.q = a->q; p.k = a->kpyr; p.v = a->vpyr; p.out = a->out;
  copy3(p.qs, a->q_stride); copy3(p.os, a->out_stride); copy3(p.ms, a->mask_stride);
  p.ks[0] = p.vs[0] = (int64_t)a->H * R * a->D;
  p.ks[1] = p.vs[1] = (int64_t)R * a->D;
  p.ks[2] = p.vs[2] = a->D;
  p.q_rows = a->q_rows;
  p.use_main = 1;
  p.mask = a->level_mask;
  fill_shape(p, a->B, a->H, a->L, a->L, nb, nb, a->D, a->scale, a->lse);
  p.Lpad = nb * kQBlk;
  p.ref_tail = a->ref_tail ? 1 : 0;
  p.heavy_rows = a->heavy_rows;
  p.work_queue = a->work_queue;
  if (!dtype_ok(a->dtype)) return fail(VB_ERR_INVALID, "vb_ml_attn_fwd: unknown dtype");
  return launch_ml_fwd(p, a->D, a->dtype, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int vb_block_sparse_attn_fwd(const void* q_unpad, const void* k_unpad, const void* v_unpad,
                                        const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                                        const int32_t* head_mask_type, const int32_t* streaming_info,
                                        const uint8_t* base_blockmask, int batch, int num_heads, int head_dim,
                                        int max_seqlen_q, int max_seqlen_k, float p_dropout, int deterministic,
                                        float softmax_scale, int is_causal, int exact_streaming, int dtype,
                                        void* out_unpad, float* softmax_lse, int mask_head_mode, void* stream) {
  using namespace vb;
  (void)streaming_info;
  (void)deterministic;
  if (p_dropout != 0.f) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_fwd: p_dropout must be 0");
  if (is_causal || exact_streaming) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_fwd: causal/streaming not supported");
  if (mask_head_mode != VB_MASK_HEAD_PER_HEAD && mask_head_mode != VB_MASK_HEAD_SHARED0)
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_fwd: unknown mask_head_mode");
  if (!q_unpad || !k_unpad || !v_unpad || !cu_seqlens_q || !cu_seqlens_k || !out_unpad)
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_fwd: null tensor");
  if (batch <= 0 || num_heads <= 0 || max_seqlen_q <= 0 || max_seqlen_k <= 0)
    return fail(VB_ERR_INVALID, "vb_block_sparse_attn_fwd: bad sizes");
  const int nbq = (max_seqlen_q + kQBlk - 1) / kQBlk;
  const int nbk = (max_seqlen_k + kQBlk - 1) / kQBlk;
  if (nbk > kMaxBlocks) return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_fwd: max_seqlen_k too long");
  const int64_t row = (int64_t)num_heads * head_dim;
  if (!slice_fits32(max_seqlen_k, row, head_dim))
    return fail(VB_ERR_UNSUPPORTED, "vb_block_sparse_attn_fwd: a sequence's k/v span >= 2 GiB");
  const int64_t s3[3] = {0, head_dim, row};   // unpadded [tokens, H, D]: a batch entry starts at its cu_seqlens row
  FwdParams p{};
  p.q = q_unpad; p.k = k_unpad; p.v = v_unpad; p.out = out_unpad;
  copy3(p.qs, s3); copy3(p.ks, s3); copy3(p.vs, s3); copy3(p.os, s3);
  p.cu_q = cu_seqlens_q; p.cu_k = cu_seqlens_k;
  p.head_mask_type = head_mask_type;
  p.hm_mode = mask_head_mode;
  p.use_main = 1;
  p.mask = base_blockmask;  // may be NULL: dense
  // base_blockmask [batch, n_sparse, nbq, nbk]: n_sparse (= number of heads whose mask id is 1) is
  // counted on the device from head_mask_type (no host read of device memory, no sync).
  p.ms[0] = head_mask_type ? -1 : (int64_t)num_heads * nbq * nbk;
  p.ms[1] = (int64_t)nbq * nbk; p.ms[2] = nbk;
  fill_shape(p, batch, num_heads, max_seqlen_q, max_seqlen_k, nbq, nbk, head_dim, softmax_scale, softmax_lse);
  return check_and_launch(p, head_dim, dtype, false, reinterpret_cast<hipStream_t>(stream));
}
