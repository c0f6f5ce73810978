/*
 * vblade.h — C ABI of libvblade_hip.so, the MI355X (gfx950) block-sparse attention path of
 * Video-BLADE. Plain pointers, sizes and strides; no framework types. Every device pointer is
 * a HIP device address; `stream` is a hipStream_t (NULL = the null stream).
 *
 * Contract:
 *   - the caller owns every buffer (inputs read-only, outputs fully overwritten); the library
 *     never allocates, frees or synchronises, so every entry point is hipGraph-capturable;
 *   - return 0 on success, a negative VB_ERR_* code otherwise; vb_last_error() holds the message
 *     of the last failure on the calling thread; no C++ exception crosses the ABI;
 *   - stateless and reentrant; all work is enqueued on `stream`.
 *
 * Tensor convention: "[B,H,L,D] strided" = element (b,h,l,d) at base + b*s[0] + h*s[1] + l*s[2] + d,
 * strides in ELEMENTS, innermost (d) stride 1. Row-index arrays ("rows") map a position of the
 * reordered (Gilbert) sequence to the row of the caller's tensor that holds it; NULL = identity.
 */
#ifndef VBLADE_H_
#define VBLADE_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VB_ABI_VERSION 4   /* 2: mask_head_mode argument of vb_block_sparse_attn_fwd/bwd; 3: vb_attn_args.q_order;
                              4: work_queue (persistent forward), kernel_select/kernels_ran (backward) */

/* Work queue of the persistent forward launches (vb_attn_args / vb_ml_attn_args.work_queue): device
 * int32[VB_WORK_QUEUE_INTS], ALL ZERO before its first use; every launch leaves it zero again. One
 * queue serves one launch at a time (launches that may overlap, e.g. on two streams, need one each). */
#define VB_WORK_QUEUE_INTS 288

enum vb_status {
  VB_OK = 0,
  VB_ERR_INVALID = -1,     /* bad argument / shape */
  VB_ERR_UNSUPPORTED = -2, /* valid for the reference op but not implemented (dropout, causal, streaming, head dim,
                              a predictor num_keep other than 16, 32 or 64) */
  VB_ERR_LAUNCH = -3       /* the HIP launch failed */
};

enum vb_dtype { VB_DTYPE_BF16 = 0, VB_DTYPE_F16 = 1 };
/* reading of head_mask_type = ones(H) (see vb_block_sparse_attn_fwd) */
enum vb_mask_head_mode { VB_MASK_HEAD_PER_HEAD = 0, VB_MASK_HEAD_SHARED0 = 1 };

/* Message of the last failing call on this thread ("" if none). */
const char* vb_last_error(void);
int vb_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Gilbert 3-D curve permutation (host). Replaces GilbertRearranger.__init__ /
 * _gilbert3d_with_index + utils/gilbert3d.py:6-167
 * (cogvideox/train/special_attentions_local/TrainRelated/cogvideo_blocksparseattn.py:112-140).
 * perm_out[g] = x + width*(y + height*z) of the g-th curve point (length width*height*depth).
 * ------------------------------------------------------------------------------------------ */
int vb_gilbert3d_perm(int width, int height, int depth, int32_t* perm_out);

/* ------------------------------------------------------------------------------------------
 * Drop-in for block_sparse_attn_func forward (mit-han-lab/Block-Sparse-Attention) exactly as the
 * reference calls it: cogvideo_blocksparseattn.py:316-320 (also :106-109 for the dense pooled
 * call; wanx_blocksparseattn.py:301-305).
 *   q/k/v_unpad   [total, H, D] contiguous, dtype `dtype`
 *   cu_seqlens_*  int32 [batch+1] (device)
 *   head_mask_type int32 [H] (device): 0 dense; m>0 block-sparse with base_blockmask head m-1;
 *                 m<0 (streaming) -> that head's output is NaN. How the reference's
 *                 head_mask_type = ones(H) (cog :313) reads is open offline:
 *                 mask_head_mode VB_MASK_HEAD_PER_HEAD (0, default) first renumbers every 1 to
 *                 1,2,3,... in head order (Block-Sparse-Attention's replace_ones_with_count: one
 *                 predicted mask per head); VB_MASK_HEAD_SHARED0 (1) reads m literally, so ones(H)
 *                 gives every head base_blockmask head 0.
 *   streaming_info ignored (only used by streaming heads)
 *   base_blockmask uint8/bool [batch, n_sparse, ceil(max_q/128), ceil(max_k/128)] contiguous
 *   out_unpad     [total_q, H, D]; softmax_lse fp32 [batch, H, max_seqlen_q] (natural log).
 *                 A query row with no kept key block gets a zero output row and lse = +inf,
 *                 FlashAttention-2's convention for an empty softmax (its normalize_softmax_lse);
 *                 the native entry vb_attn_fwd reports -inf for such rows instead.
 *   p_dropout must be 0, is_causal/exact_streaming must be 0 (the reference's call) else
 *   VB_ERR_UNSUPPORTED. softmax_scale <= 0 means head_dim^-1/2. `deterministic` is accepted
 *   and ignored (the forward is deterministic).
 * ------------------------------------------------------------------------------------------ */
int vb_block_sparse_attn_fwd(const void* q_unpad, const void* k_unpad, const void* v_unpad,
                             const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                             const int32_t* head_mask_type, const int32_t* streaming_info,
                             const uint8_t* base_blockmask, int batch, int num_heads, int head_dim,
                             int max_seqlen_q, int max_seqlen_k, float p_dropout, int deterministic,
                             float softmax_scale, int is_causal, int exact_streaming, int dtype,
                             void* out_unpad, float* softmax_lse, int mask_head_mode, void* stream);

/* ------------------------------------------------------------------------------------------
 * Native strided block-sparse attention forward (the adaptive module's hot kernel). One softmax
 * over the union of
 *   (a) full-resolution keys of the 128x128 blocks kept by `block_mask` (NULL = all kept), and
 *   (b) optionally, `Lkp` pooled keys kp/vp carrying an additive score bias `kp_log_bias`
 *       (= ln sample_gap: the LSE combine of cogvideo_blocksparseattn.py:374-393 fused as one
 *       softmax).
 * Setting use_main=0 attends only to (b) (the reference's standard_attn, :106-109).
 * q rows are read at q_rows[g] and out/lse written at q_rows[g] (g = reordered position), so
 * the Gilbert reorder and its inverse (:141-161) cost no separate pass; k/v rows read at kv_rows[g].
 * ------------------------------------------------------------------------------------------ */
typedef struct vb_attn_args {
  const void* q; const void* k; const void* v;
  int64_t q_stride[3]; int64_t k_stride[3]; int64_t v_stride[3];
  const int32_t* q_rows;  /* [Lq] or NULL */
  const int32_t* kv_rows; /* [Lk] or NULL */
  int use_main;           /* attend to the block-masked full-resolution keys */
  const uint8_t* block_mask; int64_t mask_stride[3]; /* [B,H,ceil(Lq/128),ceil(Lk/128)] or NULL */
  const void* kp; const void* vp;                     /* pooled keys [B,H,Lkp,D] strided or NULL */
  int64_t kp_stride[3]; int64_t vp_stride[3];
  int Lkp; float kp_log_bias;
  void* out; int64_t out_stride[3];
  float* lse;             /* [B,H,Lq] fp32 natural-log LSE (written at q_rows) or NULL */
  int B, H, Lq, Lk, D;
  float scale;            /* <= 0 -> D^-1/2 */
  int dtype;
  int heavy_rows;         /* scheduling hint: the last N q-block rows keep (almost) every key
                             block (CogVideoX's forced text rows: 2); 0 = none. Never affects results. */
  int32_t* q_order;       /* scheduling workspace [B*H*ceil(Lq/128)] int32, or NULL (ABI 3): with a
                             block mask, each XCD's q-blocks are dispatched head by head, longest
                             (most kept key blocks) first, so its last workgroups are the short ones.
                             Written by a small launch before the attention kernel. Never affects results. */
  const int32_t* q_lengths; /* [B,H,ceil(Lq/128)] kept key blocks per mask row (vb_predict_args.
                             mask_rows_kept), or NULL: the ordering launch counts them from the mask */
  int order_window;       /* > 0: only the last order_window q-blocks of each XCD range are re-ordered
                             (the tail; the rest keeps the kernel's head-major, Gilbert-neighbour
                             order and its L2 reuse); 0: the whole range */
  int32_t* work_queue;    /* ABI 4, nullable: persistent dispatch — a resident-sized grid whose workgroups
                             pull q-blocks from per-XCD queues (in the order above) and, once their own
                             XCD's queue is empty, from the others'. NULL: one workgroup per q-block.
                             Never affects results. See VB_WORK_QUEUE_INTS. */
} vb_attn_args;
int vb_attn_fwd(const vb_attn_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused mask predictor (a3+a4+a5): efficient_attn_with_pooling + attn_with_pooling (Triton,
 * attn_pooling_kernel.py:17-255) + transfer_attn_to_mask(mode="energy")
 * (cogvideo_blocksparseattn.py:57-82, 177-249; wanx_blocksparseattn.py:162-233).
 * For each (b,h): the reordered sequence (rows, replicate-padded to a multiple of `block`) is
 * sampled at the `num_keep` offsets q_off[b,h,:] / k_off[b,h,:] of every block; pooled scores
 * Po [nb,nb] (storage dtype, row-normalised) are written to `po` and the energy rule
 * (threshold, min/max kept blocks, last `force_tail` rows/cols forced) writes `mask` [B,H,nb,nb].
 * Ties between equal Po values are kept lowest-block-first. `mask_count` (nullable) receives
 * an atomic add of the number of kept blocks (device-side sparsity statistic, no host sync).
 * ------------------------------------------------------------------------------------------ */
typedef struct vb_predict_args {
  const void* q; const void* k;
  int64_t q_stride[3]; int64_t k_stride[3];
  const int32_t* rows;     /* [L] reordered -> caller row, or NULL */
  int32_t* q_off;          /* [B,H,num_keep] int32 in [0,block): input, or output with rand_q/rand_k */
  int32_t* k_off;
  int B, H, L, D, block, num_keep; /* block = 128. num_keep = 16, 32 or 64 sampled tokens per block (the
                              reference's default is 32; 16 does a quarter of the score work, 64 four
                              times), otherwise VB_ERR_UNSUPPORTED before any launch. The sampled streams
                              have nb*num_keep rows: row j*num_keep + t of (b,h) is reordered position
                              min(j*block + off[b,h,t], L-1). */
  float scale;             /* <= 0 -> D^-1/2 */
  float energy_threshold;
  int min_keep, max_keep, force_tail;
  void* po;                /* [B,H,nb,nb] storage dtype, contiguous */
  uint8_t* mask;           /* [B,H,nb,nb] contiguous, or NULL: scores only (no energy rule) */
  unsigned long long* mask_count; /* nullable */
  int dtype;
  void* workspace;         /* device, 16-byte aligned, >= vb_mask_predict_workspace_size(args) bytes:
                              the sampled k rows' offsets and the per-row block maxima,
                              B*H*(nb*num_keep*4 + nb*nb*num_keep*2) bytes; smaller: VB_ERR_INVALID */
  uint64_t workspace_bytes;
  void* staged_event;      /* nullable hipEvent_t, recorded on `stream` once the sampled rows are
                              staged (before the score kernel): independent work on another stream
                              can start then and overlap the score kernel */
  /* Optional fusions (NULL = off):
   * rand_q/rand_k: [B,H,block] fp32 uniforms, the q then k torch.rand draws of
   *   random_sample_tokens (:45-46); the topk(num_keep) offsets are drawn in the sampling launch
   *   (as vb_sample_offsets) and WRITTEN to q_off/k_off.
   * pool_*: the pooled K/V pass of vb_pool_kv (on this call's k and pool_v, same rows) run by
   *   extra workgroups of the score kernel's own launch, beside it on `stream`: no second stream
   *   and no events. pool_kp/pool_vp [B,H,ceil(L/pool_gap),D]; pool_k_r/pool_v_r [B,H,L,D] or NULL. */
  const float* rand_q;
  const float* rand_k;
  const void* pool_v;
  int64_t pool_v_stride[3];
  int pool_gap;
  void* pool_kp; void* pool_vp;
  void* pool_k_r; void* pool_v_r;
  /* pyr_k/pyr_v: the multi-level path's KV pyramid pass of vb_kv_pyramid (this call's k and
   * pool_v, same rows; [B,H,vb_kv_pyramid_rows(L),D] each) run by extra workgroups of the score
   * kernel's launch, like pool_* (which it excludes): no second stream and no events. */
  void* pyr_k; void* pyr_v;
  /* philox != 0: the two torch.rand(B,H,1,block) draws of random_sample_tokens are generated inside
   * the sampling launch instead of read from rand_q/rand_k — PyTorch's uniform_ on a device
   * generator at state (philox_seed, philox_offset): element i of a draw = the x value of the first
   * hiprand_uniform4 of Philox4x32-10 subsequence i (1.0 mapped to 0.0), the q draw at
   * philox_offset and the k draw at philox_offset + 4 (each torch.rand call advances the offset by
   * 4 per call). Element i takes the x of thread i only while every element has a thread of its own
   * in torch.rand's grid-stride launch: B*H*block <= CUs x max threads per CU of the device (524288
   * on an unpartitioned MI355X); past that the call fails with VB_ERR_UNSUPPORTED. The offsets are WRITTEN
   * to q_off/k_off; the caller advances its generator by 8. */
  int philox;
  uint64_t philox_seed;
  uint64_t philox_offset;
  /* mask_level != 0: `mask` receives the multi-level rank-band mask instead of the energy mask —
   * vb_level_mask's rule (bands level_band_value / [level_band_start, level_band_end) as fractions
   * of nb, 0..8 of them; the last two rows and columns forced to level 1) applied by the score
   * kernel's epilogue to the normalised scores it has just written to po: no second launch and no
   * re-read of po. Replaces the vb_level_mask launch of the multi-level path
   * (Triton/cogvideo_newattn.py:154-207). */
  int mask_level;
  int level_bands;
  const int32_t* level_band_value;
  const double* level_band_start;
  const double* level_band_end;
  /* mask_rows_kept (ABI 3, nullable): [B,H,nb] int32, the number of key blocks the energy rule kept
   * in each mask row (the attention kernel's per-q-block work, for vb_attn_args.q_lengths). */
  int32_t* mask_rows_kept;
} vb_predict_args;
uint64_t vb_mask_predict_workspace_size(const vb_predict_args* args);
int vb_mask_predict(const vb_predict_args* args, void* stream);   /* nb <= 320 (L <= 40960) */
/* vb_mask_predict for rows of up to 1024 blocks (L <= 131072, the attention kernels' own limit).
 * Same arguments, outputs, options and workspace (vb_mask_predict_workspace_size) as
 * vb_mask_predict; accepts any nb in [1, 1024] and fails with VB_ERR_UNSUPPORTED past that. A second
 * instantiation of the same score kernel whose epilogue ranks up to 16 values per lane: for
 * nb <= 320 it writes the bits vb_mask_predict writes (num_keep 16 and 64 run this instantiation
 * from either entry; each entry keeps its own nb limit). Workspace per (b,h):
 * nb*num_keep*4 + nb*nb*num_keep*2 bytes, nearly all of it the block maxima: at num_keep 32, 22 MB
 * at 591 blocks (Wan 720p) and 67 MB at 1024; at 1024 blocks 34 MB with num_keep 16 and 134 MB
 * with num_keep 64. */
int vb_mask_predict_long(const vb_predict_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * The whole mask rule of transfer_attn_to_mask (cogvideo_blocksparseattn.py:177-249;
 * wanx_blocksparseattn.py:162-233): mode="energy" with bounds and threshold per (batch, head) (the
 * CogVideoX copy's [B,H] max_retain_ratio / min_retain_ratio tensors, :230-231), and mode="topk"
 * (:205-225). Per q-block row of nc scores, rounded to the storage dtype T and ranked in descending
 * order (ties: lower column first); cum[i] = the fp32 running sum of the sorted values, each prefix
 * rounded to T; total = cum[nc-1].
 *   VB_RULE_ENERGY  the rule of vb_mask_predict / vb_energy_mask with min_keep[b,h], max_keep[b,h]
 *                   and energy_threshold[b,h]; a NULL array takes the scalar of the call.
 *   VB_RULE_TOPK    k0 = init_k_bh[b,h] (or the scalar init_k); e = cum[k0-1];
 *                   c_lo = e >= T(total * grow_below), c_hi = e >= T(total * shrink_below);
 *                   k = k0; if (!c_lo && k0 < nr) k = min(3k, nr);
 *                   if (!c_hi && k0 < nr) k = min(k/3*2, nr)  (on the updated k, integer division);
 *                   the k best columns are kept (k may be 0), then the forced tail as in energy
 *                   mode. In vb_block_mask_rule k is also capped at nc. min_keep, max_keep and
 *                   energy_threshold are unused.
 * A scalar init_k outside [1, nc] is VB_ERR_INVALID before any launch. Values read from DEVICE
 * arrays (init_k_bh, min_keep, max_keep) cannot be checked on the host without a synchronisation:
 * the kernel clamps each to [1, nc] before any use as an index or a bound (for the energy rule the
 * clamp never changes the mask a scalar call with the same value writes).
 * ------------------------------------------------------------------------------------------ */
enum vb_rule_mode { VB_RULE_ENERGY = 0, VB_RULE_TOPK = 1 };
typedef struct vb_mask_rule {
  int mode;
  const int32_t* min_keep;          /* device [B,H] or NULL: the scalar of the call */
  const int32_t* max_keep;
  const float*   energy_threshold;
  int            init_k;            /* top-k: scalar k0 ... */
  const int32_t* init_k_bh;         /* ... or device [B,H] (wins when non-NULL) */
  float          grow_below, shrink_below;   /* <= 0: 0.6 / 0.9, the reference's constants */
} vb_mask_rule;

/* vb_mask_predict with the rule above applied by the score kernel's epilogue (no second launch, no
 * re-read of po); any nb in [1, 1024]; every other option of the call works as without a rule, and
 * po and the pooled / pyramid outputs are the same bits. mask_count and mask_rows_kept count the
 * kept blocks (forced ones included) in both modes. rule == NULL: the call and the bits of
 * vb_mask_predict (nb <= 320) / vb_mask_predict_long. mask_level != 0 with a rule: VB_ERR_INVALID. */
int vb_mask_predict_rule(const vb_predict_args* args, const vb_mask_rule* rule, void* stream);

/* The rule alone on given scores (vb_energy_mask's sibling): po [B,H,nr,nc] contiguous storage dtype
 * -> mask [B,H,nr,nc], nc <= 1024. energy_threshold / min_keep / max_keep are the scalars that NULL
 * arrays of an energy-mode rule fall back to. rows_kept (nullable): int32 [B,H,nr], kept blocks per
 * mask row. rule == NULL: vb_energy_mask. */
int vb_block_mask_rule(const void* po, int B, int H, int nr, int nc, const vb_mask_rule* rule,
                       float energy_threshold, int min_keep, int max_keep, int force_tail, int dtype,
                       uint8_t* mask, unsigned long long* mask_count, int32_t* rows_kept, void* stream);

/* random_sample_tokens' index draw (cogvideo_blocksparseattn.py:45-46): the caller draws the
 * uniforms (torch.rand(B,H,1,block), q first then k, so the RNG stream is the reference's); this
 * replaces the two topk(num_keep) calls: rand_q/rand_k fp32 [rows, n] -> q_off/k_off int32
 * [rows, keep], indices of the `keep` largest values in descending order (ties: lower index first). */
int vb_sample_offsets(const float* rand_q, const float* rand_k, int rows, int n, int keep,
                      int32_t* q_off, int32_t* k_off, void* stream);

/* Energy rule alone on given scores (transfer_attn_to_mask, mode="energy"):
 * po [B,H,nr,nc] contiguous storage dtype -> mask [B,H,nr,nc], nc <= 1024. */
int vb_energy_mask(const void* po, int B, int H, int nr, int nc, float energy_threshold,
                   int min_keep, int max_keep, int force_tail, int dtype, uint8_t* mask,
                   unsigned long long* mask_count, void* stream);

/* ------------------------------------------------------------------------------------------
 * Mean pooling of K and V over `gap` consecutive reordered tokens with replicate padding
 * (simple_pooling, cogvideo_blocksparseattn.py:83-88): kp/vp [B,H,ceil(L/gap),D] contiguous.
 * Optionally (k_r, v_r non-NULL) also writes the reordered copies k_r/v_r [B,H,L,D] contiguous
 * (the reference's index_select, :148-150) in the same pass: every row is read once.
 * ------------------------------------------------------------------------------------------ */
int vb_pool_kv(const void* k, const void* v, const int64_t* k_stride, const int64_t* v_stride,
               const int32_t* rows, int B, int H, int L, int D, int gap, int dtype, void* kp,
               void* vp, void* k_r, void* v_r, void* stream);

/* ------------------------------------------------------------------------------------------
 * Reference-faithful LSE combine (cogvideo_blocksparseattn.py:374-393, each eager op rounded to
 * the storage dtype): out = out1*a + out2*(1-a), a = e1/(e1+e2) from lse1 and lse2 + ln(gap).
 * All tensors [B,H,L,(D)] contiguous; alpha (nullable) receives a as fp32 [B,H,L].
 * ------------------------------------------------------------------------------------------ */
int vb_lse_combine(const void* out1, const float* lse1, const void* out2, const float* lse2,
                   int B, int H, int L, int D, float gap, int dtype, void* out, float* alpha,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * vb_lse_combine on strided tensors: the same arithmetic, element for element and with the same
 * rounding points, so out and alpha are the bits vb_lse_combine writes on contiguous copies of the
 * inputs. out1, out2 and out are each [B,H,L,D] addressed through three element strides (batch,
 * head, row; unit d-stride; non-negative multiples of 8; bases 16-byte aligned), e.g. the
 * [B,H,L,D] view of [B,L,H*D] projection-layout memory. lse1, lse2 and alpha (nullable) stay
 * contiguous fp32 [B,H,L]. D is 64 or 128; B and H at most 65535 (grid dimensions). out may not
 * overlap out1 or out2, and its rows must be distinct (no zero stride over an extent above 1).
 * Null arguments, bad sizes, an unknown dtype, bad strides or alignment: VB_ERR_INVALID before any
 * launch. Allocates nothing, never synchronises; one launch on `stream` (16 bytes per lane, a wave
 * covers whole rows: a row's D*2 contiguous bytes move as full cache lines at any row stride).
 * ------------------------------------------------------------------------------------------ */
int vb_lse_combine_strided(const void* out1, const int64_t* out1_stride, const float* lse1,
                           const void* out2, const int64_t* out2_stride, const float* lse2,
                           int B, int H, int L, int D, float gap, int dtype, void* out,
                           const int64_t* out_stride, float* alpha, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward (FlashAttention-2 semantics, deterministic: no atomics) of the block-sparse attention
 * and of the adaptive module's two-branch form, as the reference's autograd computes it
 * (cogvideo_blocksparseattn.py:316-320 + :366-393):
 *   main branch   keys k/v [B,H,Lk,D] in REORDERED order (row g = reordered key g), block_mask
 *                 [B,H,ceil(Lq/128),ceil(Lk/128)] (NULL = dense), its output `out` and LSE `lse`
 *   pooled branch (kp != NULL) kp/vp [B,H,Lkp,D], its output out2 and LSE lse2 (no bias), the
 *                 combine weight alpha (fp32 [B,H,Lq], as vb_lse_combine writes it) — LSEs and alpha
 *                 are constants: dO1 = alpha*dO, dO2 = storage(1-alpha)*dO; the pooled K/V grads
 *                 are folded back through the mean pool over `pool_gap` reordered keys (replicate
 *                 padding onto the last key)
 * q/out/out2/dout/lse/lse2/alpha/dq rows are addressed through q_rows[g] like vb_attn_fwd; dk/dv of
 * reordered key g are written at row kv_rows[g] (NULL = g). dq/dk/dv are fully overwritten.
 * `workspace` (device, 16-byte aligned) of at least vb_attn_bwd_workspace_size(args) bytes.
 * The workspace grows linearly with B: besides the per-row statistics and the reordered q/dO
 * copies it holds the pooled-key dK/dV partials, psplit * B * H * Lkp * D fp32 values twice, with
 * psplit chosen from H and L only (never B) so that a sample's gradients are the same bits alone
 * or inside a micro-batch. At B=5 that is ~0.86 GB for CogVideoX (psplit 6) and ~1.9 GB for Wan
 * (psplit 14) — small against 288 GB of HBM, so no cap is applied.
 * ------------------------------------------------------------------------------------------ */
typedef struct vb_attn_bwd_args {
  const void* q; int64_t q_stride[3];
  const void* k; const void* v; int64_t k_stride[3]; int64_t v_stride[3];
  const int32_t* q_rows;    /* [Lq] or NULL */
  const int32_t* kv_rows;   /* [Lk] or NULL */
  const uint8_t* block_mask; int64_t mask_stride[3];
  const void* out; int64_t out_stride[3];
  const float* lse;         /* [B,H,Lq] natural log */
  const void* kp; const void* vp; int64_t kp_stride[3]; int64_t vp_stride[3];
  int Lkp;
  const void* out2; int64_t out2_stride[3];
  const float* lse2;        /* [B,H,Lq] */
  const float* alpha;       /* [B,H,Lq] or NULL (= 1: no pooled branch) */
  int pool_gap;
  const void* dout; int64_t dout_stride[3];
  void* dq; int64_t dq_stride[3];
  void* dk; void* dv; int64_t dk_stride[3]; int64_t dv_stride[3];
  void* workspace; uint64_t workspace_bytes;
  int B, H, Lq, Lk, D;
  float scale;              /* <= 0 -> D^-1/2 */
  int dtype;
  int heavy_rows;           /* scheduling hint as in vb_attn_args */
  int kernel_select;        /* ABI 4: VB_BWD_SEL_* bits, 0 = the default kernels (same results up to the
                               fp32 summation order; for A/B tests) */
  int32_t* kernels_ran;     /* ABI 4, HOST memory, nullable: receives the VB_BWD_RAN_* bits of the
                               kernels this call launched */
} vb_attn_bwd_args;
/* kernel_select bits: the earlier kernels each default replaced */
#define VB_BWD_SEL_DKDV_ROUND3 1   /* dK/dV (main and pooled keys; multi-level: level 1) on bwd_dkdv_kernel
                                      instead of the hand-placed stream bwd_dkdv_pipe_kernel */
#define VB_BWD_SEL_DQ_ROUND3 2     /* dQ on bwd_dq_kernel instead of the pipeline bwd_dq_pipe_kernel */
#define VB_BWD_SEL_DQ_RING4 4      /* D=128 pipeline dQ on the 4-slot ring (one workgroup per CU) */
/* kernels_ran bits */
#define VB_BWD_RAN_DKDV_PIPE 1
#define VB_BWD_RAN_DKDV_ROUND3 2
#define VB_BWD_RAN_DQ_PIPE_RING2 4
#define VB_BWD_RAN_DQ_PIPE_RING4 8
#define VB_BWD_RAN_DQ_ROUND3 16
#define VB_BWD_RAN_ML_PYRAMID 32   /* the multi-level pooled-level dK/dV pass */
uint64_t vb_attn_bwd_workspace_size(const vb_attn_bwd_args* args);
int vb_attn_bwd(const vb_attn_bwd_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Exact backward of the ONE-softmax form vb_attn_fwd evaluates with kp/vp/kp_log_bias (the
 * inference call, and the training forward of grad_combine="joint"). The function differentiated is
 *   out[i] = sum_j P[i,j] v[j] + sum_m Pp[i,m] vp[m],
 *   P[i,j]  = exp(scale q[i].k[j]            - lse[i])   over the keys j of blocks block_mask keeps,
 *   Pp[i,m] = exp(scale q[i].kp[m] + beta    - lse[i])   over all Lkp pooled keys,
 *   lse[i]  = log(sum_j exp(scale q[i].k[j]) + sum_m exp(scale q[i].kp[m] + beta)),
 * with beta = pool_log_bias, the block mask a constant, and kp/vp the mean pool of k/v over
 * `pool_gap` consecutive REORDERED keys (replicate padding onto the last key), so dk/dv receive the
 * pooled keys' gradients folded back through that pool. The gradient is exact: one LSE and one
 * Delta = rowsum(dO * out) serve both key sets. vb_attn_bwd's two-branch form instead holds both
 * branch LSEs and the combine weight alpha constant (the reference's autograd), which drops the
 * term (out1 - out2) * d alpha; dq and dk of the two therefore differ, dv does not.
 * Same struct and conventions as vb_attn_bwd: `out` and `lse` are the joint forward's (vb_attn_fwd
 * with need of the LSE, the same kp_log_bias); kp, vp, Lkp > 0 and pool_gap > 0 are required; out2,
 * lse2 and alpha must be NULL. Workspace: vb_attn_bwd_workspace_size(args). kernel_select and
 * kernels_ran keep their meaning (only the per-row statistics pass differs). No atomics: results
 * are bit-reproducible, and a sample's gradients are the same bits alone or inside a batch.
 * ------------------------------------------------------------------------------------------ */
int vb_attn_bwd_joint(const vb_attn_bwd_args* args, float pool_log_bias, void* stream);

/* Drop-in for the block_sparse_attn_func backward (same tensor conventions as
 * vb_block_sparse_attn_fwd): dq/dk/dv [total, H, D]; softmax_lse as the forward wrote it.
 * workspace >= vb_block_sparse_attn_bwd_workspace_size(batch, num_heads, max_seqlen_q) bytes. */
uint64_t vb_block_sparse_attn_bwd_workspace_size(int batch, int num_heads, int max_seqlen_q);
int vb_block_sparse_attn_bwd(const void* dout, const void* q_unpad, const void* k_unpad,
                             const void* v_unpad, const void* out_unpad, const float* softmax_lse,
                             const int32_t* cu_seqlens_q, const int32_t* cu_seqlens_k,
                             const int32_t* head_mask_type, const int32_t* streaming_info,
                             const uint8_t* base_blockmask, int batch, int num_heads, int head_dim,
                             int max_seqlen_q, int max_seqlen_k, float p_dropout, float softmax_scale,
                             int is_causal, int exact_streaming, int deterministic, int dtype,
                             void* dq, void* dk, void* dv, void* workspace, uint64_t workspace_bytes,
                             int mask_head_mode, void* stream);

/* ==========================================================================================
 * Multi-level block-sparse attention: the VBench sampler's op (cogvideox/sample_evaluate/
 * modify_cogvideo.py:9 -> Triton/cogvideo_newattn.py:210-234, kernel Triton/kernels/
 * block_sparse_attn_kernel_with_backward_9_10.py). Every (query block i, key block j) pair has a
 * level p in {0, 1, 2, 4, 8}: 0 skips the block, p > 0 attends to the block's 128/p keys of K/V
 * mean-pooled by p, each with logit q.k*scale + ln p.
 * ========================================================================================== */

/* Rows of the KV pyramid of an L-row sequence: 15*Lpad/8 with Lpad = ceil(L/128)*128. */
int vb_kv_pyramid_rows(int L);

/* The KV pyramid (the _forward wrapper's pad_to_multiple + pooling x3, :1239-1270, :1311-1320):
 * k/v [B,H,L,D] with strides k_stride/v_stride (elements; batch, head, row), rows gathered through
 * `rows` (reordered row g = caller row rows[g]; NULL = g) -> kpyr/vpyr [B,H,R,D] contiguous:
 *   rows [0, Lpad)              level 1: the reordered rows, rows >= L ZERO (the kernel's masked
 *                               loads of the tail block, :111, :126)
 *   [Lpad, 3Lpad/2)             level 2: mean of reordered row pairs, rows >= L replicate row L-1
 *   [3Lpad/2, 7Lpad/4)          level 4: mean of level-2 pairs, rounded per level like torch.mean
 *   [7Lpad/4, 15Lpad/8)         level 8
 * One pass reads every row once. */
int vb_kv_pyramid(const void* k, const void* v, const int64_t* k_stride, const int64_t* v_stride,
                  const int32_t* rows, int B, int H, int L, int D, int dtype, void* kpyr, void* vpyr,
                  void* stream);

/* transfer_attn_to_mask (Triton/cogvideo_newattn.py:154-207): po [B,H,nr,nc] contiguous storage
 * dtype -> mask [B,H,nr,nc] uint8. Per row, the entry ranked r in descending order (ties: lower
 * column first; the reference's torch.sort is unstable) gets band_value[b] of the LAST band b with
 * floor(nc*band_start[b]) <= r < floor(nc*band_end[b]) (bounds computed in double, as Python does),
 * else 0; then the last two columns and the last two rows are set to 1. n_bands <= 8, values in
 * {0,1,2,4,8}; band arrays are HOST memory. nc <= 4096. */
int vb_level_mask(const void* po, int B, int H, int nr, int nc, int n_bands, const int32_t* band_value,
                  const double* band_start, const double* band_end, int dtype, uint8_t* mask,
                  void* stream);

/* Multi-level attention forward (_fwd_kernel, :338-692): queries q [B,H,L,D] (rows through q_rows as
 * in vb_attn_fwd), keys/values the pyramids of vb_kv_pyramid, level_mask [B,H,nb,nb] (nb =
 * ceil(L/128); entries other than 1,2,4,8 skip). out [B,H,L,D] written at q_rows[g]; lse (nullable,
 * fp32 [B,H,L] at the caller's row q_rows[g], as vb_attn_fwd) = m + ln(l) of the reference's (l, m).
 * ref_tail = 1 reproduces the reference on L % 128 != 0: a level-1 tail block's keys >= L are
 * zero vectors that still take part (logit 0, value 0); ref_tail = 0 masks them. */
typedef struct vb_ml_attn_args {
  const void* q; int64_t q_stride[3];
  const int32_t* q_rows;       /* [L] or NULL */
  const void* kpyr; const void* vpyr;   /* [B,H,vb_kv_pyramid_rows(L),D] contiguous */
  const uint8_t* level_mask; int64_t mask_stride[3];
  void* out; int64_t out_stride[3];
  float* lse;
  int B, H, L, D;
  float scale;                 /* <= 0 -> D^-1/2 */
  int ref_tail;
  int dtype;
  int heavy_rows;              /* last q-block rows known to be dense (the forced rows): dispatched first */
  int32_t* work_queue;         /* ABI 4, nullable: persistent dispatch as vb_attn_args.work_queue */
} vb_ml_attn_args;
int vb_ml_attn_fwd(const vb_ml_attn_args* args, void* stream);

/* Multi-level attention backward (_backward + the per-level kernels, :696-1237, :1375-1576),
 * FlashAttention-2 semantics from the forward's out and lse, deterministic (no atomics):
 *   dQ over every kept block's keys at its level (+ln p bias);
 *   dK/dV of each pyramid row, the pooled levels' folded back through the means:
 *   dk[r] = dK1[r] + dK2[r/2]/2 + dK4[r/4]/4 + dK8[r/8]/8 for r < L (gradient reaching the
 *   replicate-padded rows is dropped, as the reference does).
 * `rows` (nullable) is the reorder of the forward (pyramid rows and q_rows): q/out/dout/dq rows are
 * addressed through it, and dk/dv of reordered key g are written at caller row rows[g].
 * dq/dk/dv are fully overwritten. workspace >= vb_ml_attn_bwd_workspace_size(args) bytes. */
typedef struct vb_ml_attn_bwd_args {
  const void* q; int64_t q_stride[3];
  const int32_t* rows;         /* [L] or NULL */
  const void* kpyr; const void* vpyr;
  const uint8_t* level_mask; int64_t mask_stride[3];
  const void* out; int64_t out_stride[3];
  const float* lse;            /* as vb_ml_attn_fwd wrote it */
  const void* dout; int64_t dout_stride[3];
  void* dq; int64_t dq_stride[3];
  void* dk; void* dv; int64_t dk_stride[3]; int64_t dv_stride[3];
  void* workspace; uint64_t workspace_bytes;
  int B, H, L, D;
  float scale;                 /* <= 0 -> D^-1/2 */
  int ref_tail;
  int dtype;
  int heavy_rows;
  int kernel_select;           /* ABI 4: as vb_attn_bwd_args (DKDV_ROUND3: the level-1 pass) */
  int32_t* kernels_ran;        /* ABI 4, HOST memory, nullable: as vb_attn_bwd_args */
} vb_ml_attn_bwd_args;
uint64_t vb_ml_attn_bwd_workspace_size(const vb_ml_attn_bwd_args* args);
int vb_ml_attn_bwd(const vb_ml_attn_bwd_args* args, void* stream);

/* ==========================================================================================
 * The attention processors' q/k prologue in one pass: the q/k norm and RoPE that sit between the
 * projections and inner_attention (cogvideox/train/modify_cogvideo.py:54-64, a per-head LayerNorm
 * then apply_rotary_emb on the video rows; wanx/train/modify_wan.py:99-116, an RMSNorm over the
 * projection row then the float64 complex RoPE). Every element is read once and written once.
 *
 * A tensor is [B,L,H,D] as the projection wrote it: element (b,l,h,d) at base + b*stride[0] +
 * l*stride[1] + h*D + d (strides in ELEMENTS, multiples of 8, row stride >= H*D; 16-byte aligned
 * bases) — the memory whose [B,H,L,D] view the attention kernels take through their strides.
 * `out` may equal `x` (in place); any other overlap is undefined. D = 64 or 128, H*D <= 8192
 * (8128 with the RMSNorm).
 *
 * Per row, in the eager chain's order and with its rounding points:
 *   norm  VB_QK_NORM_LAYER_HEAD  LayerNorm over each head's D elements: fp32 mean, then fp32 mean of
 *                                the squared deviations (two-pass), (x-mean)*rsqrt(var+eps)*weight+bias
 *         VB_QK_NORM_RMS_ROW     RMSNorm over the H*D row: x*rsqrt(mean(x^2)+eps)*weight
 *         weight (nullable = 1) and bias (nullable = 0; LayerNorm only) hold D (LayerNorm) or H*D
 *         (RMSNorm) values of the storage dtype or, with affine_f32 != 0, fp32. The result is
 *         rounded to the storage dtype; RoPE works on the rounded value.
 *   rope  VB_QK_ROPE_REAL        rows l >= rope_start: y = x*cos[l-rope_start] + rot(x)*sin[l-rope_start]
 *                                with rot(x)[2i] = -x[2i+1], rot(x)[2i+1] = x[2i]; cos/sin fp32
 *                                [L-rope_start, D]; two fp32 products and one fp32 sum, each rounded
 *                                (never fused), then the storage dtype. Rows below rope_start get
 *                                the norm alone.
 *         VB_QK_ROPE_COMPLEX     every row (rope_start must be 0): pairs (a,b) = (x[2i], x[2i+1])
 *                                times freqs[l][i] = (c,s) in fp64, (a*c - b*s, a*s + b*c), rounded
 *                                double -> float -> storage dtype; freqs [L, D/2] (re,im) pairs of
 *                                fp32 or, with freqs_f64 != 0, fp64.
 * No trigonometry runs on the device: the tables are the caller's.
 * ========================================================================================== */
enum vb_qk_norm { VB_QK_NORM_NONE = 0, VB_QK_NORM_LAYER_HEAD = 1, VB_QK_NORM_RMS_ROW = 2 };
enum vb_qk_rope { VB_QK_ROPE_NONE = 0, VB_QK_ROPE_REAL = 1, VB_QK_ROPE_COMPLEX = 2 };
typedef struct vb_qk_prologue_args {
  const void* x; void* out;
  int64_t x_stride[2]; int64_t out_stride[2];   /* batch, row */
  int B, L, H, D;
  int dtype;
  int norm;                 /* vb_qk_norm */
  const void* weight; const void* bias;
  int affine_f32;           /* weight and bias are fp32 (else the storage dtype) */
  float eps;
  int rope;                 /* vb_qk_rope */
  int rope_start;
  const float* cos; const float* sin;
  const void* freqs; int freqs_f64;
} vb_qk_prologue_args;
/* q and, when k != NULL, k (same B, L, H, D and dtype as q; its own modes and buffers) in ONE launch:
 * a workgroup takes whole token rows of both, so tensors that name the same RoPE table with the same
 * mode and rope_start read each table row once. */
int vb_qk_prologue(const vb_qk_prologue_args* q, const vb_qk_prologue_args* k, void* stream);

/* The prologue's backward, for training: dx (and the norm's parameter gradients) from the forward's
 * input x, its modes and parameters, and g, the gradient w.r.t. the forward's output. Nothing else
 * is saved from the forward: the statistics are recomputed from x as the forward computes them.
 * The forward's two roundings to the storage dtype are the identity for the gradient (as autograd
 * treats them); between loading g and storing dx everything stays in fp32 (fp64 for the complex
 * RoPE's products), with ONE rounding to the storage dtype at the store.
 *   RoPE^T  real     rows l >= rope_start: p = g*cos, s = g*sin, gy[2i] = p[2i] + s[2i+1],
 *                    gy[2i+1] = p[2i+1] - s[2i]; rows below rope_start: gy = g
 *           complex  gy = g * conj(freqs): (g_a*c + g_b*s, g_b*c - g_a*s)
 *   norm^T  LAYER_HEAD  xhat = (x-mean)*rstd, a = gy*w: dx = rstd*(a - mean_D(a) - xhat*mean_D(a*xhat));
 *                       dweight[d] = sum_{b,l,h} gy*xhat, dbias[d] = sum_{b,l,h} gy
 *           RMS_ROW     xhat = x*rstd, a = gy*w: dx = rstd*(a - xhat*mean_W(a*xhat));
 *                       dweight[c] = sum_{b,l} gy*xhat
 *           NONE        dx = gy
 * x: as vb_qk_prologue_args.x. g: element (b,l,h,d) at g + b*g_stride[0] + l*g_stride[1] +
 * h*g_stride[2] + d (strides in ELEMENTS, non-negative multiples of 8, 16-byte aligned base), so
 * [B,H,L,D]-contiguous gradients and [B,L,H,D] memory are both read where they lie. dx: storage
 * dtype, batch and row strides like x, fully overwritten; it must not overlap x or g.
 * dweight / dbias (each nullable): fp32 whatever the parameters' dtype, D (LAYER_HEAD) or H*D
 * (RMS_ROW) values, fully overwritten, summed without atomics in an order that depends only on the
 * shape and the number of workgroups: every workgroup writes its partial sums to `workspace` and a
 * second small launch on `stream` adds them up. Both NULL (for every tensor of the call): no
 * accumulation, no second launch, no workspace.
 * grid_limit: 0 = the resident grid, capped at VB_QK_BWD_MAX_GRID; > 0 caps the number of
 * workgroups. It never changes dx; equal grid_limit gives equal dweight/dbias bits.
 * workspace: >= vb_qk_prologue_bwd_workspace_size(q, k) bytes (host arithmetic; 0 when no parameter
 * gradient is requested), 16-byte aligned, named by the FIRST non-NULL of q and k for the whole
 * call. The library allocates nothing and never synchronises; the call is graph-capturable. */
#define VB_QK_BWD_MAX_GRID 1024
typedef struct vb_qk_prologue_bwd_args {
  const void* x; int64_t x_stride[2];           /* batch, row */
  const void* g; int64_t g_stride[3];           /* batch, row, head */
  void* dx; int64_t dx_stride[2];               /* batch, row */
  float* dweight; float* dbias;
  void* workspace; uint64_t workspace_bytes;
  int B, L, H, D;
  int dtype;
  int norm;                 /* vb_qk_norm */
  const void* weight; const void* bias;         /* bias: accepted as the forward's, never read */
  int affine_f32;
  float eps;
  int rope;                 /* vb_qk_rope */
  int rope_start;
  const float* cos; const float* sin;
  const void* freqs; int freqs_f64;
  int grid_limit;
} vb_qk_prologue_bwd_args;
uint64_t vb_qk_prologue_bwd_workspace_size(const vb_qk_prologue_bwd_args* q, const vb_qk_prologue_bwd_args* k);
/* Either of q and k may be NULL (a k-only backward), not both. With both, k has q's B, L, H, D,
 * dtype and grid_limit, and one launch serves both tensors (each table row read once) unless they
 * name two different norms or two different RoPE tables. */
int vb_qk_prologue_bwd(const vb_qk_prologue_bwd_args* q, const vb_qk_prologue_bwd_args* k, void* stream);

/* ==========================================================================================
 * Head-adaptive retain budgets: the reference's judge_sparsity estimator (cogvideox/train/
 * special_attentions_local/TrainRelated/blocksparseattn.py:147-160) and the budget rule of its
 * commented-out call sites (cogvideo_blocksparseattn.py:344-348; wanx_blocksparseattn.py:328-330),
 * on the device. Additive to ABI 4.
 *
 * vb_judge_sparsity: for every (b,h) and every sampled row r < S, over the n = ceil(L / key_stride)
 * keys j*key_stride (j = 0 .. n-1):
 *   s_j    = scale * <q[b,h,rows[r],:], k[b,h,j*key_stride,:]>, MFMA with fp32 accumulation
 *   p      = softmax(s) over the n keys, max-subtracted, fp32 (exp2 on scale*log2(e)-scaled scores)
 *   mass_r = the sum of the top_n largest p_j: with t the top_n-th largest value, found by a radix
 *            selection over the fp32 bit patterns (no sort), sum(p > t) + (top_n - #(p > t)) * t, so
 *            ties at the boundary count the same whichever of them is taken
 *   sparsity[b,h] = the fp32 mean of mass_r over r, summed serially in r order
 * which is the reference's sort-descending / mean-by-rank / sum of the first top_n ranks: the mean
 * over rows of each row's top-n mass. The Python side passes top_n = int(n * 0.2).
 * q, k: [B,H,L,D] strided (unit d-stride, strides multiples of 8 elements, 16-byte aligned bases),
 * read in place; D = 64 or 128, L <= 131072, every (b,h) slice < 2 GiB (else VB_ERR_UNSUPPORTED).
 * rows: DEVICE int32 [S], caller row numbers shared by all (b,h), S in [1, 64]. They cannot be
 * checked on the host without a synchronisation: the kernel clamps each to [0, L-1] before it is
 * used as an address. top_n in [1, n]. Null pointers, S, top_n or key_stride out of range and a
 * short workspace are VB_ERR_INVALID before any launch.
 * sparsity: fp32 [B,H]; row_mass (nullable): fp32 [B,H,S], mass_r.
 * workspace: device, 16-byte aligned, >= vb_judge_sparsity_workspace_size(args) bytes (host
 * arithmetic: B*H*S rows of n fp32 scores, each padded to a multiple of four, staged between the
 * two launches of the call, plus B*H*S row masses and B*H counters).
 * Deterministic: no floating-point atomics, every sum in an order fixed by the shape; two calls
 * give the same bits. Two launches on `stream`.
 * ========================================================================================== */
typedef struct vb_judge_args {
  const void* q; const void* k;
  int64_t q_stride[3]; int64_t k_stride[3];
  const int32_t* rows;      /* device [S] */
  int B, H, L, D, S;
  int key_stride;           /* >= 1; the reference's k[:, :, ::3] is 3 */
  int top_n;
  float scale;              /* <= 0 -> D^-1/2 */
  int dtype;
  float* sparsity;          /* [B,H] */
  float* row_mass;          /* [B,H,S] or NULL */
  void* workspace; uint64_t workspace_bytes;
} vb_judge_args;
uint64_t vb_judge_sparsity_workspace_size(const vb_judge_args* args);
int vb_judge_sparsity(const vb_judge_args* args, void* stream);

/* The budget rule on the device: sparsity fp32 [B,H] -> max_keep int32 [B,H] (the array
 * vb_mask_rule.max_keep takes) and, when non-NULL, ratio fp32 [B,H]. In float64:
 *   m     = (sum of all B*H values) / (B*H)       (batch and heads together, the reference's .mean())
 *   ratio = min(max(base * (sparsity[b,h] / m), lo), hi)
 *   count = max(1, int(float(nb) * float(ratio)))  arith 0 (cog: an fp32 product)
 *           max(1, int(nb * ratio))                arith 1 (wan: float64)
 * the two arithmetics of the per-head retain counts elsewhere in this library's Python layer. One
 * launch on `stream`. base > 0, finite lo <= hi, nb >= 1, arith 0 or 1, else VB_ERR_INVALID. */
int vb_head_budget(const float* sparsity, int B, int H, int nb, double base, double lo, double hi,
                   int arith, int32_t* max_keep, float* ratio, void* stream);

/* ==========================================================================================
 * Attention-recall probe: what a block mask keeps of the true attention, measured on a call's own
 * q, k and mask for S probe queries per head. Additive to ABI 4.
 *
 * The energy rule steers one quantity through a sampled, pooled proxy: the share of a query's
 * softmax mass that falls inside the key blocks its mask row keeps. vb_mask_recall computes that
 * share exactly (recall), and the best share any mask with the same number of blocks could have kept
 * for that query (oracle recall). Both low: the budget is too small. Recall well below the oracle:
 * the predictor picked the wrong blocks.
 *
 * All arithmetic fp32 unless stated. For every (b,h) and probe r < S:
 *   g = clamp(probe_pos[r], 0, L-1), a REORDERED position; i = g / 128 its mask row
 *   the query is caller row rows[g]; key j of the reordered sequence is caller row rows[j],
 *   j = 0 .. L-1 (rows NULL: the identity). Only the L real keys take part: the last block holds
 *   L - 128*(nb-1) keys, no replicate padding.
 *   s_j = scale * <q, k_j>, MFMA with fp32 accumulation; e_j = exp2((s_j - max_j s_j) * log2(e))
 *   (evaluated per block relative to the block's maximum and rescaled to the row's)
 *   E_c = sum of e_j over the keys of block c (an order fixed by the shape)
 *   T = sum_c E_c;  K = sum of E_c over the c with mask[b,h,i,c] != 0: BOTH summed over c in
 *   ascending block order, so an all-ones mask row gives K == T in bits and recall exactly 1.0f
 *   row_recall = K / T;  row_kept = n_i = #{c < nb : mask[b,h,i,c] != 0}
 *   row_oracle = (the sum of the n_i largest E_c) / T: ties take the lower block index first, the
 *   selected set is summed in ascending block order; a mask row that already holds the n_i heaviest
 *   blocks gives row_oracle == row_recall in bits; n_i = 0 gives 0 for both
 *   recall[b,h], oracle_recall[b,h] = the fp32 means over r, summed serially in r order
 * q, k: as vb_judge_args. rows: the array vb_attn_args.q_rows / kv_rows take (a permutation of
 * [0, L); the kernel clamps what it reads to [0, L-1] before it is used as an address). probe_pos:
 * DEVICE int32 [S], shared by all (b,h), S in [1, 64]; clamped to [0, L-1] by the kernel before any
 * use. block_mask: uint8 [B,H,nb,nb] in reordered order, nb = ceil(L/128), unit stride along the key
 * blocks, the other three strides in mask_stride (a head stride of 0 is the shared_head0 view).
 * Null q, k, probe_pos, block_mask or recall, bad sizes, S outside [1, 64], an unknown dtype, q/k
 * bases not 16-byte aligned or strides that are not non-negative multiples of 8, negative mask
 * strides and a short or missing workspace are VB_ERR_INVALID before any launch; D not 64 or 128,
 * L > 131072 and a (b,h) slice of 2 GiB or more are VB_ERR_UNSUPPORTED.
 * workspace: device, 16-byte aligned, >= vb_mask_recall_workspace_size(args) bytes (host arithmetic:
 * B*H*S*nb pairs of fp32, a block's maximum and its sum relative to it, staged between the launches,
 * plus B*H*S pairs of row results: at most 512 KiB + 512 bytes per head).
 * Deterministic: no floating-point atomics, every sum in an order fixed by the shape; two calls give
 * the same bits. Three launches on `stream`; nothing is allocated, nothing synchronises.
 * ========================================================================================== */
typedef struct vb_recall_args {
  const void* q; const void* k;
  int64_t q_stride[3]; int64_t k_stride[3];
  const int32_t* rows;       /* device [L]: reordered position -> caller row, or NULL = identity */
  const int32_t* probe_pos;  /* device [S]: reordered positions of the probe queries */
  const uint8_t* block_mask; int64_t mask_stride[3];
  int B, H, L, D, S;
  float scale;               /* <= 0 -> D^-1/2 */
  int dtype;
  float* recall;             /* [B,H] */
  float* oracle_recall;      /* [B,H] or NULL */
  float* row_recall;         /* [B,H,S] or NULL */
  float* row_oracle;         /* [B,H,S] or NULL */
  int32_t* row_kept;         /* [B,H,S] or NULL: kept blocks in the probe row's mask row */
  void* workspace; uint64_t workspace_bytes;
} vb_recall_args;
uint64_t vb_mask_recall_workspace_size(const vb_recall_args* args);
int vb_mask_recall(const vb_recall_args* args, void* stream);

/* ==========================================================================================
 * Mask predictor, second block score: the sampled softmax MASS of a (q-block, key-block) pair, beside
 * the max proxy of vb_mask_predict (the largest single-key probability ratio of the block). The
 * sampling, the mask rule (vb_block_mask_rule on `po`) and everything downstream are the existing
 * ones; only the score differs. Additive to ABI 4.
 *
 * Sampled streams: those of vb_mask_predict. Per (b,h), block i < nb = ceil(L/128) and t < num_keep
 * the reordered position is g = min(128*i + off[b,h,t], L-1) (the clamp is the replicate pad) and the
 * caller's row is rows[g] (rows NULL: the identity). q_off gives the sampled queries qs, k_off the
 * sampled keys ks, nb*num_keep rows each; row i*num_keep + t belongs to block i. The kernel clamps
 * each offset to [0, 127] and each row number to [0, L-1] before it is used as an address.
 *
 * All arithmetic fp32 unless stated. For sampled query r and sampled key c of one (b,h):
 *   s[r,c]    = <qs_r, ks_c> (MFMA, fp32 accumulation) * qk_scale;
 *               qk_scale = fp32(scale) * fp32(1.44269504) as vb_mask_predict forms it, scale <= 0 ->
 *               D^-1/2
 *   M_r       = max_c s[r,c] (the rounded product of the largest dot product: qk_scale > 0);
 *               l_r = sum_c exp2(s[r,c] - M_r), every s - M one fused multiply-add of the dot product,
 *               qk_scale and -M (the product is not rounded before the subtraction), evaluated online
 *               over the key blocks in ascending order, per half of each 32-key tile, the two halves
 *               joined at the end
 *   mass[i,j] = sum over the queries r of q-block i of (1/l_r) * sum over the keys c of key block j
 *               of exp2(s[r,c] - M_r): per query the 16 keys of each half-tile in a fixed order, the
 *               two halves, one product with 1/l_r, then the 32 queries by a butterfly. Every row of
 *               mass sums to num_keep up to rounding.
 *   po[i,j]   = storage(mass[i,j] / sum_j mass[i,j]): row-normalised in the storage dtype, the form
 *               vb_block_mask_rule expects; the row sum runs per lane over j = lane, lane+64, ... and
 *               then over the 64 lanes by a butterfly.
 * Everything is taken relative to M_r, so scores of magnitude in the hundreds do not overflow.
 * Deterministic: no floating-point atomics, every sum in an order fixed by the shape; two calls give
 * the same bits. Three launches on `stream` (gather of the sampled rows, scores, row normalisation);
 * nothing is allocated, nothing synchronises.
 *
 * q, k: [B,H,L,D] bf16/fp16, unit stride along D, the other strides (elements) in q_stride/k_stride:
 * non-negative multiples of 8, bases 16-byte aligned; D = 64 or 128; nb <= 1024 (L <= 131072); every
 * (b,h) slice of q and of k < 2 GiB. block must be 128. num_keep must be 32: 16 and 64 (which
 * vb_mask_predict serves) are VB_ERR_UNSUPPORTED here, as are another D, nb > 1024 and a slice of
 * 2 GiB or more. Null q, k, q_off, k_off or po, bad sizes, an unknown dtype, bad strides or alignment
 * and a short or missing workspace are VB_ERR_INVALID. Every refusal happens before the first launch.
 * workspace: device, 16-byte aligned, >= vb_mask_scores_mass_workspace_size(args) bytes (host
 * arithmetic): the two gathered streams, B*H*2*nb*32*D elements, and B*H*nb*nb fp32 block masses.
 * ========================================================================================== */
typedef struct vb_mass_scores_args {
  const void* q; const void* k;
  int64_t q_stride[3]; int64_t k_stride[3];
  const int32_t* rows;       /* device [L]: reordered position -> caller row, or NULL = identity */
  const int32_t* q_off;      /* device [B,H,num_keep] int32 in [0, block): explicit offsets only */
  const int32_t* k_off;
  int B, H, L, D, block, num_keep;
  float scale;               /* <= 0 -> D^-1/2 */
  int dtype;
  void* po;                  /* [B,H,nb,nb] storage dtype, contiguous */
  float* mass;               /* [B,H,nb,nb] fp32 contiguous, or NULL (tests and calibration) */
  void* workspace; uint64_t workspace_bytes;
} vb_mass_scores_args;
uint64_t vb_mask_scores_mass_workspace_size(const vb_mass_scores_args* args);
int vb_mask_scores_mass(const vb_mass_scores_args* args, void* stream);

/* ==========================================================================================
 * Output-fidelity probe: the error of an attention output against exact dense attention, measured
 * on a call's own q, k, v and out for S probe queries per head. Additive to ABI 4.
 *
 * The recall probe (vb_mask_recall) looks at the scores alone: it ignores V and the pooled branch
 * and has no meaning for a graded (multi-level) mask. vb_attn_fidelity needs neither a mask nor an
 * order (a softmax over all keys does not depend on the keys' order): it recomputes the dense output
 * rows of the probe queries and compares `out` with them, whichever module or option produced `out`.
 *
 * All arithmetic fp32 unless stated. For every (b,h) and probe r < S:
 *   g = clamp(probe_rows[r], 0, L-1), a CALLER row of q and out
 *   t_j = <q_g, k_j> * qk_scale, j = 0 .. L-1 in caller order: MFMA with fp32 accumulation, the
 *   product with qk_scale rounded once; qk_scale = fp32(scale) * fp32(1.44269504) as
 *   vb_mask_scores_mass forms it, scale <= 0 -> D^-1/2. Only the L real rows take part: no padding.
 *   The keys are cut into chunks of VB_FIDELITY_CHUNK = 512 consecutive keys, nc = ceil(L/512) of
 *   them (the last holds L - 512*(nc-1)): a rule of L alone, never of the device, B or H.
 *   Per chunk c: m_c = max t_j; e_j = exp2(t_j - m_c); l_c = sum e_j (per MFMA column over the
 *   chunk's 32-key tiles in ascending order, then a butterfly over the 32 columns);
 *   acc_c[d] = sum_j e_j * v_j[d], one fmaf per key in ascending key order, e_j never rounded below
 *   fp32. (m_c, l_c, acc_c) are staged in the workspace.
 *   Join, chunks in ascending order: m = max_c m_c; w_c = exp2(m_c - m); l = fmaf(l_c, w_c, l);
 *   a[d] = fmaf(acc_c[d], w_c, a[d]); ref[d] = a[d] / l. Everything is relative to a maximum, so
 *   scores of magnitude in the hundreds do not overflow.
 *   row_err = sum_d (float(out[g,d]) - ref[d])^2 and row_sig = sum_d ref[d]^2: one fmaf per d, in
 *   ascending d.  row_lse = ln(l) + m * ln 2 (the natural-log LSE of scale * <q,k>).
 *   err[b,h], sig[b,h] = the sums of row_err, row_sig over r, added serially in r order;
 *   peak[b,h] = max over r and d of |ref[d]|.
 * SNR = 10 log10(sig / err) per head is the figure to log; peak^2 * S * D / err gives a sampled PSNR.
 *
 * q, k, v, out: [B,H,L,D] bf16/fp16, unit stride along D, the other strides (elements) in
 * q_stride/k_stride/v_stride/out_stride: non-negative multiples of 8, bases 16-byte aligned; D = 64
 * or 128; L <= 131072; every (b,h) slice < 2 GiB. probe_rows: DEVICE int32 [S], shared by all (b,h),
 * S in [1, 64]; clamped to [0, L-1] by the kernel before any use. The kernels read no byte outside
 * the L rows of each (b,h) slice.
 * Outputs: err, sig fp32 [B,H] (required); peak fp32 [B,H], row_err, row_sig, row_lse fp32 [B,H,S]
 * and ref fp32 [B,H,S,D] contiguous (each nullable).
 * A null q, k, v, out, probe_rows, err or sig, bad sizes, S outside [1, 64], an unknown dtype, bases
 * not 16-byte aligned or strides that are not non-negative multiples of 8 and a short or missing
 * workspace are VB_ERR_INVALID before any launch; D not 64 or 128, L > 131072 and a (b,h) slice of
 * 2 GiB or more are VB_ERR_UNSUPPORTED.
 * workspace: device, 16-byte aligned, >= vb_attn_fidelity_workspace_size(args) bytes (host
 * arithmetic): 4 * (B*H*S*nc*(D+2) + 3*B*H*S) rounded up to 16: the chunks' (m, l), their acc rows,
 * and three results per row for the last launch.
 * Deterministic: no floating-point atomics, every sum in an order fixed by the shape; two calls give
 * the same bits, and a sample's results are the same bits alone or inside a larger batch. Three
 * launches on `stream` (chunk partials, join, per-head sums); nothing is allocated, nothing
 * synchronises.
 * ========================================================================================== */
#define VB_FIDELITY_MAX_SAMPLES 64
#define VB_FIDELITY_CHUNK 512
typedef struct vb_fidelity_args {
  const void* q; const void* k; const void* v; const void* out;
  int64_t q_stride[3]; int64_t k_stride[3]; int64_t v_stride[3]; int64_t out_stride[3];
  const int32_t* probe_rows; /* device [S]: caller rows of the probe queries */
  int B, H, L, D, S;
  float scale;               /* <= 0 -> D^-1/2 */
  int dtype;
  float* err;                /* [B,H] */
  float* sig;                /* [B,H] */
  float* peak;               /* [B,H] or NULL */
  float* row_err;            /* [B,H,S] or NULL */
  float* row_sig;            /* [B,H,S] or NULL */
  float* row_lse;            /* [B,H,S] or NULL */
  float* ref;                /* [B,H,S,D] or NULL */
  void* workspace; uint64_t workspace_bytes;
} vb_fidelity_args;
uint64_t vb_attn_fidelity_workspace_size(const vb_fidelity_args* args);
int vb_attn_fidelity(const vb_fidelity_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VBLADE_H_ */
