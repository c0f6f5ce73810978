"""TEST INFRASTRUCTURE ONLY — CPU restatement (oracle) of Video-BLADE's adaptive block-sparse
attention path.

Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline`` leg may import
this module, and only as the checker / CPU baseline. The product path is the HIP library
``libvblade_hip.so`` (``video-blade_amd/csrc``); it never calls into this file.

Every function cites the reference file:line it restates. Paths are relative to the reference
repo root; ``TR/`` = ``cogvideox/train/special_attentions_local/TrainRelated/`` (the Wan copy
under ``wanx/train/...`` differs only where noted).

Pinning:
  * gilbert permutation, sampled offsets, pooled scores (fp32 and fp16 storage), energy masks,
    simple pooling, the LSE combine and the whole adaptive glue are pinned against the
    reference's own Python/Triton code run in this container (``tests/golden/make_golden.py``,
    Triton interpreter) — fixtures in ``tests/golden/``.
  * the external CUDA op ``block_sparse_attn_func`` (mit-han-lab/Block-Sparse-Attention, an
    un-vendored FlashAttention-2 fork; no version pinned by the reference, README.md:52-61) is
    absent: its restatement here (masked softmax with natural-log LSE) is pinned only by the
    identity with dense SDPA for an all-ones mask and by masked-softmax semantics
    -> "parity unpinned" for that single op, as recorded in DESIGN.md.
"""
from __future__ import annotations

import math

import numpy as np
import torch

LOG2E = 1.44269504  # the literal used by attn_pooling_kernel.py:169


# ----------------------------------------------------------------------------------------------
# rounding helpers
# ----------------------------------------------------------------------------------------------
def rnd(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Round an fp32/fp64 tensor to ``dtype`` storage and back to fp32 (no-op for fp32)."""
    return x.to(dtype).to(torch.float32)


# ----------------------------------------------------------------------------------------------
# a3: padding and token sampling for the mask predictor
# ----------------------------------------------------------------------------------------------
def pad_replicate(x: torch.Tensor, multiple: int) -> torch.Tensor:
    """TR/cogvideo_blocksparseattn.py:20-31 — replicate-pad dim -2 up to a multiple."""
    L = x.shape[-2]
    rem = L % multiple
    if rem == 0:
        return x
    tail = x[..., L - 1:L, :].expand(*x.shape[:-2], multiple - rem, x.shape[-1])
    return torch.cat([x, tail], dim=-2)


def draw_sample_offsets(B: int, H: int, block: int = 128, num_keep: int = 32,
                        generator: torch.Generator | None = None, device="cpu") -> torch.Tensor:
    """TR/cogvideo_blocksparseattn.py:45-46 — rand(B,H,1,block) then topk(num_keep) -> [B,H,num_keep]."""
    r = torch.rand(B, H, 1, block, generator=generator, device=device)
    return torch.topk(r, num_keep, dim=3).indices[:, :, 0, :]


def sample_tokens(x_padded: torch.Tensor, offsets: torch.Tensor, block: int = 128) -> torch.Tensor:
    """TR/cogvideo_blocksparseattn.py:32-55 — the same ``num_keep`` offsets in every block of a (b,h)."""
    B, H, L, D = x_padded.shape
    nb = L // block
    xb = x_padded.reshape(B, H, nb, block, D)
    idx = offsets[:, :, None, :, None].expand(B, H, nb, offsets.shape[-1], D)
    return torch.gather(xb, 3, idx).reshape(B, H, nb * offsets.shape[-1], D)


# ----------------------------------------------------------------------------------------------
# a4: pooled scores (restates the Triton kernel attn_pooling_kernel.py:17-84, 87-199, 201-253)
# ----------------------------------------------------------------------------------------------
def pooled_scores(qs: torch.Tensor, ks: torch.Tensor, sm_scale: float, block: int = 32,
                  store_dtype: torch.dtype | None = None) -> torch.Tensor:
    """Po[b,h,i,j] = max_{r in q-block i} exp2(R[r,j] - m_r), row-normalised in ``store_dtype``.

    * qk_scale = fp32(sm_scale) * fp32(1.44269504)                     (:168-169)
    * rowmax_blk = max over the block's keys of fp32 dot products, times qk_scale (:46,52)
    * R = rowmax_blk rounded to the storage dtype (q.dtype)             (:55, R alloc :219)
    * m_r = running max of the UNROUNDED fp32 rowmax_blk                 (:53,56)
    * Po[i,j] = storage(max_r exp2(float(R[r,j]) - m_r))  (l_i == 1)    (:73-82)
    * Po /= Po.sum(-1) in the storage dtype (fp32 accumulation)         (:250-251)
    """
    store_dtype = store_dtype or qs.dtype
    B, H, Ls, D = qs.shape
    n = Ls // block
    qk_scale = float(np.float32(sm_scale) * np.float32(LOG2E))
    S = torch.matmul(qs.float(), ks.float().transpose(-1, -2))             # [B,H,Ls,Ls] fp32
    rowblk = S.reshape(B, H, Ls, n, block).amax(-1) * np.float32(qk_scale)  # fp32
    m = rowblk.amax(-1, keepdim=True)
    R = rnd(rowblk, store_dtype)
    w = torch.exp2(R - m)
    po = rnd(w.reshape(B, H, n, block, n).amax(3), store_dtype)
    tot = rnd(po.sum(-1, keepdim=True), store_dtype)
    return rnd(po / tot, store_dtype)


# ----------------------------------------------------------------------------------------------
# a5: energy rule -> block mask
# ----------------------------------------------------------------------------------------------
def retain_counts(nb: int, min_ratio: float, max_ratio: float, variant: str) -> tuple[int, int]:
    """min/max kept blocks per row.

    cog: clamp((seq * fp32 ratio tensor).to(int), min=1)   (TR/cogvideo_blocksparseattn.py:230-231, 347-348)
    wan: max(1, int(seq * ratio)) in Python floats          (wanx_blocksparseattn.py:215-216)"""
    if variant == "cog":
        lo = int(np.float32(nb) * np.float32(min_ratio))
        hi = int(np.float32(nb) * np.float32(max_ratio))
    else:
        lo = int(nb * min_ratio)
        hi = int(nb * max_ratio)
    return max(1, lo), max(1, hi)


def energy_keep_count(po_row_sorted: np.ndarray, thr: float, store_dtype=torch.bfloat16) -> int:
    """Number of leading sorted blocks kept before clamping (TR/cogvideo_blocksparseattn.py:232-238).

    cumsum accumulates in fp32 and rounds each prefix to the storage dtype (torch CPU cumsum);
    k = first index with cum >= storage(total*fp32(thr)); the crossing block itself is NOT kept;
    never crossing -> k = nb."""
    # torch CPU cumsum for bf16/fp16 accumulates in float: a sequential fp32 running sum,
    # each prefix rounded to the storage dtype
    cums = np.cumsum(po_row_sorted.astype(np.float32), dtype=np.float32)
    cum = rnd(torch.from_numpy(cums), store_dtype)
    total = cum[-1]
    th = rnd(total * np.float32(thr), store_dtype)
    hit = torch.nonzero(cum >= th)
    return int(hit[0]) if hit.numel() else int(cum.numel())


def energy_keep_counts(po: torch.Tensor, min_keep: int, max_keep: int, thr: float = 0.95,
                       store_dtype=torch.bfloat16) -> torch.Tensor:
    """Clamped kept-block count k per row [B,H,nr] (TR/cogvideo_blocksparseattn.py:232-239).
    k depends only on the sorted VALUES, so it is independent of how ties are ordered."""
    p = po.float().cpu().numpy()
    k = np.zeros(p.shape[:3], dtype=np.int64)
    for idx in np.ndindex(*p.shape[:3]):
        row = p[idx]
        kk = energy_keep_count(-np.sort(-row), thr, store_dtype)
        k[idx] = min(max(kk, min_keep), max_keep)
    return torch.from_numpy(k)


def energy_mask(po: torch.Tensor, min_keep: int, max_keep: int, thr: float = 0.95,
                force_tail: int = 0, store_dtype=torch.bfloat16) -> torch.Tensor:
    """transfer_attn_to_mask(mode="energy") (TR/cogvideo_blocksparseattn.py:177-249;
    wanx_blocksparseattn.py:162-233). Ties are broken by LOWER block index first (stable
    descending sort); the reference's torch.sort is unstable, so which of several EQUAL
    boundary blocks it keeps is implementation-defined (``mask_is_valid_topk`` accepts any
    such choice). ``force_tail`` = 2 for CogVideoX (:247-248: last 2 rows and columns forced
    True), 0 for Wan."""
    B, H, nr, nc = po.shape
    p = po.float().cpu().numpy()
    kk = energy_keep_counts(po, min_keep, max_keep, thr, store_dtype).numpy()
    mask = np.zeros((B, H, nr, nc), dtype=bool)
    for idx in np.ndindex(B, H, nr):
        order = np.argsort(-p[idx], kind="stable")
        mask[idx][order[:kk[idx]]] = True
    if force_tail:
        mask[..., -force_tail:] = True
        mask[..., -force_tail:, :] = True
    return torch.from_numpy(mask)


def mask_is_valid_topk(mask: torch.Tensor, po: torch.Tensor, k: torch.Tensor,
                       force_tail: int = 0) -> bool:
    """True when every row of ``mask`` equals T ∪ F for SOME top-k selection T of that row
    (any tie order) and F = the forced tail columns; forced rows must be all True."""
    m = mask.bool().cpu().numpy()
    p = po.float().cpu().numpy()
    kk = k.cpu().numpy()
    nr, nc = m.shape[2], m.shape[3]
    forced = np.zeros(nc, dtype=bool)
    if force_tail:
        forced[-force_tail:] = True
    for idx in np.ndindex(*m.shape[:3]):
        row, val, kr = m[idx], p[idx], int(kk[idx])
        if force_tail and idx[2] >= nr - force_tail:
            if not row.all():
                return False
            continue
        if not row[forced].all():
            return False
        vk = np.sort(val)[::-1][kr - 1]
        required = val > vk
        ties = val == vk
        body = row & ~forced
        if not row[required].all():
            return False
        if (body & ~(required | ties)).any():
            return False
        need = kr - int(required.sum())
        if not (int((body & ties).sum()) <= need <= int((row & ties).sum())):
            return False
    return True


# ----------------------------------------------------------------------------------------------
# a7: block-sparse attention (external block_sparse_attn_func; restated, parity unpinned)
# ----------------------------------------------------------------------------------------------
def block_sparse_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                           block_mask: torch.Tensor | None, sm_scale: float | None = None,
                           block: int = 128, key_bias: float = 0.0,
                           acc_dtype=torch.float64):
    """out[b,h,r] = softmax over keys c of the kept (row-block, col-block) pairs of
    (q_r . k_c) * scale, times v; lse = natural-log log-sum-exp of the kept scaled scores.

    Replaces block_sparse_attn_func as called at TR/cogvideo_blocksparseattn.py:316-320
    (non-causal, p_dropout 0, softmax_scale None -> D^-1/2, 128x128 blocks, LSE fp32 [B,H,Lq]).
    ``block_mask`` None = dense. Computed per 128-row block in ``acc_dtype``.
    Returns (out fp32 [B,H,Lq,D], lse fp32 [B,H,Lq])."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(D)
    qf, kf, vf = q.to(acc_dtype), k.to(acc_dtype), v.to(acc_dtype)
    out = torch.zeros(B, H, Lq, D, dtype=torch.float32)
    lse = torch.full((B, H, Lq), float("-inf"), dtype=torch.float32)
    nbq = (Lq + block - 1) // block
    keycol_block = torch.arange(Lk) // block
    for i in range(nbq):
        r0, r1 = i * block, min(Lq, (i + 1) * block)
        s = torch.matmul(qf[:, :, r0:r1], kf.transpose(-1, -2)) * scale + key_bias  # [B,H,m,Lk]
        if block_mask is not None:
            keep = block_mask[:, :, i, :].bool()[:, :, keycol_block]                   # [B,H,Lk]
            s = s.masked_fill(~keep[:, :, None, :], float("-inf"))
        mx = s.amax(-1, keepdim=True)
        mx_safe = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
        p = torch.exp(s - mx_safe)
        l = p.sum(-1, keepdim=True)
        o = torch.matmul(p, vf) / torch.where(l > 0, l, torch.ones_like(l))
        out[:, :, r0:r1] = o.float()
        lse[:, :, r0:r1] = (mx_safe + torch.log(l)).squeeze(-1).float()
    return out, lse


def union_keys(q, k, v, block_mask, kp=None, vp=None, kp_log_bias=0.0, use_main=True, block=128):
    """The one key set the fused forward's softmax runs over: the main keys a row's mask row keeps
    (``block_mask`` None = all of them; ``use_main`` False = none) followed by the pooled keys.
    Returns (K [B,H,n,D], V [B,H,n,D], visible bool [B,H,Lq,n], bias fp64 [n] in natural-log
    units: 0 for main keys, ``kp_log_bias`` for pooled ones), K/V in the inputs' dtype."""
    B, H, Lq, D = q.shape
    nbq = (Lq + block - 1) // block
    Ks, Vs, vis, bias = [], [], [], []
    if use_main:
        Lk = k.shape[2]
        if block_mask is None:
            keep = torch.ones(B, H, Lq, Lk, dtype=torch.bool)
        else:
            nbk = (Lk + block - 1) // block
            m = block_mask.bool().expand(B, H, *block_mask.shape[2:])[:, :, :nbq, :nbk]
            keep = m[:, :, torch.arange(Lq) // block][:, :, :, torch.arange(Lk) // block]
        Ks.append(k), Vs.append(v), vis.append(keep), bias.append(torch.zeros(Lk, dtype=torch.float64))
    if kp is not None:
        Lkp = kp.shape[2]
        Ks.append(kp), Vs.append(vp), vis.append(torch.ones(B, H, Lq, Lkp, dtype=torch.bool))
        bias.append(torch.full((Lkp,), float(kp_log_bias), dtype=torch.float64))
    return torch.cat(Ks, 2), torch.cat(Vs, 2), torch.cat(vis, 3), torch.cat(bias)


def softmax_over_visible(q, K, V, visible, bias, scale):
    """fp64 softmax attention of q over the keys K with per-(row, key) visibility and a per-key
    additive logit bias (natural-log units). Rows that see no key give a zero output and -inf LSE.
    Returns fp64 (out [B,H,Lq,D], lse [B,H,Lq])."""
    s = torch.matmul(q.double(), K.double().transpose(-1, -2)) * scale + bias.double()
    s = s.masked_fill(~visible, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
    p = torch.exp(s - mx)
    l = p.sum(-1, keepdim=True)
    out = torch.matmul(p, V.double()) / torch.where(l > 0, l, torch.ones_like(l))
    return out, (mx + torch.log(l)).squeeze(-1)


def joint_attention(q, k, v, mask, kp=None, vp=None, bias=0.0, sm_scale=None, use_main=True, block=128):
    """fp64 reference of the fused forward (vb_attn_fwd): ONE softmax over the union of the kept
    full-resolution keys and the pooled keys, the latter carrying the logit bias ``bias`` (the a9
    identity, see adaptive_attention_joint; no intermediate rounding). ``mask`` None = dense,
    ``kp`` None = main branch alone, ``use_main`` False = pooled keys alone (k, v ignored).
    Returns fp64 (out [B,H,Lq,D], lse [B,H,Lq], natural log; -inf for a row with no key)."""
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(q.shape[-1])
    K, V, vis, b = union_keys(q, k, v, mask, kp, vp, bias, use_main, block)
    return softmax_over_visible(q, K, V, vis, b, scale)


LOG2E_F32 = np.float32(1.4426950408889634)   # kLog2e (csrc/vb_common.hpp)
LN2_F32 = np.float32(0.6931471805599453)     # kLn2


def attention_fwd_emulated(q, k, v, block_mask, *, kp=None, vp=None, kp_log_bias=0.0, use_main=True,
                           sm_scale=None, store_dtype, prescale_q=False, block=128, m_lag=None):
    """vb_attn_fwd (csrc/vb_attn_fwd.hip) restated in fp32 with its roundings, for deriving test
    bounds (per_row_bound): what the kernel rounds, this rounds; what it only reorders (tile order,
    the deferred and lazy rescales, fp32 summation order) is not emulated.

      * c = fp32(scale) * fp32(log2 e); pooled keys carry fp32(kp_log_bias) * fp32(log2 e) (host).
      * training form (launches that return the LSE): scores are fp32 dot products of the storage
        operands; the exp2 argument is fma(s, c, bias - m), one rounding.
      * inference form (``prescale_q``; kCBias): q := storage(fp32(q) * c), and the dot product,
        seeded with bias - m, is the exp2 argument itself.
      * P = exp2(.) in fp32; l = sum of the fp32 P; P is rounded to the storage type as the P.V
        operand; O accumulates in fp32; out = storage(O * (1 / l)); lse = (m + log2 l) * fp32(ln 2).
      * m is the row's exact maximum (exp2 domain) minus ``m_lag`` (log2 units, broadcastable to
        [B,H,Lq,1]; None = 0). The kernels' m is the maximum of the first tile processed, raised
        later only past kRescaleSlack = 4 (training) or log2 kLazyBound (inference) log2 units, so
        it lags the exact maximum by a data-dependent amount. The lag scales P and l alike, but it
        decides how P rounds: with the exact maximum a row's largest P is exactly 1 and rounds
        without error, so a row that one key owns shows the output rounding alone, while the
        kernels round that P = 2^-lag like any other (up to 2^-9 bf16 / 2^-12 f16 of the whole row).
        Bounds for the kernels are therefore derived with a lag whose fractional part is spread
        over [0, 1) across the rows; which tile raises m when is not emulated.
    Rows that see no key: zero output, -inf LSE. Returns fp32 (out, lse)."""
    D = q.shape[-1]
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(D)
    K, V, vis, b = union_keys(q, k, v, block_mask, kp, vp, 0.0, use_main, block)
    bias2 = b.float()   # exp2 domain
    if kp is not None:
        bias2[-kp.shape[2]:] = float(np.float32(kp_log_bias) * LOG2E_F32)
    return fwd_emulated_over_visible(q, K, V, vis, bias2, scale, store_dtype, prescale_q, m_lag)


def fwd_emulated_over_visible(q, K, V, vis, bias2, scale, store_dtype, prescale_q=False, m_lag=None):
    """The roundings of attention_fwd_emulated over any union of keys: K, V [B,H,n,D] in the storage
    dtype, ``vis`` bool [B,H,Lq,n], ``bias2`` fp32 [n] the per-key logit bias in the EXP2 domain (what
    the kernel adds: fp32(kp_log_bias) * fp32(log2 e) for pooled keys, exactly 0, 1, 2, 3 for the
    multi-level forward's levels). Returns fp32 (out, lse)."""
    c = np.float32(scale) * LOG2E_F32
    ninf = float("-inf")
    if prescale_q:
        qs = rnd(q.float() * float(c), store_dtype)
        x = (torch.matmul(qs, K.float().transpose(-1, -2)) + bias2).masked_fill(~vis, ninf)
        m = x.amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        if m_lag is not None:
            m = m - m_lag
        x = x - m
    else:
        s = torch.matmul(q.float(), K.float().transpose(-1, -2))
        m = (s * float(c) + bias2).masked_fill(~vis, ninf).amax(-1, keepdim=True)
        m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
        if m_lag is not None:
            m = m - m_lag
        # fma(s, c, bias - m): the product is exact in fp64, so one rounding to fp32
        x = (s.double() * float(c) + (bias2 - m).double()).float().masked_fill(~vis, ninf)
    p = torch.exp2(x)
    l = p.sum(-1, keepdim=True)
    o = torch.matmul(rnd(p, store_dtype), V.float())
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    out = rnd(o * inv, store_dtype)
    lse = ((m + torch.log2(l)) * float(LN2_F32)).squeeze(-1)
    return out, lse


def block_sparse_attention_bwd(q, k, v, out, lse, dout, block_mask, sm_scale=None, block=128,
                               key_bias: float = 0.0, acc_dtype=torch.float64):
    """FlashAttention-2 backward semantics for a7 (LSE treated as a constant, no LSE gradient):
    P = exp(S*scale + bias - lse), Delta = rowsum(dO*O), dS = P*(dO V^T - Delta),
    dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO. Returns fp32 (dq, dk, dv)."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(D)
    qf, kf, vf = q.to(acc_dtype), k.to(acc_dtype), v.to(acc_dtype)
    of, dof = out.to(acc_dtype), dout.to(acc_dtype)
    dq = torch.zeros(B, H, Lq, D, dtype=acc_dtype)
    dk = torch.zeros(B, H, Lk, D, dtype=acc_dtype)
    dv = torch.zeros(B, H, Lk, D, dtype=acc_dtype)
    nbq = (Lq + block - 1) // block
    keycol_block = torch.arange(Lk) // block
    for i in range(nbq):
        r0, r1 = i * block, min(Lq, (i + 1) * block)
        s = torch.matmul(qf[:, :, r0:r1], kf.transpose(-1, -2)) * scale + key_bias
        if block_mask is not None:
            keep = block_mask[:, :, i, :].bool()[:, :, keycol_block]
            s = s.masked_fill(~keep[:, :, None, :], float("-inf"))
        p = torch.exp(s - lse[:, :, r0:r1, None].to(acc_dtype))
        do = dof[:, :, r0:r1]
        delta = (do * of[:, :, r0:r1]).sum(-1, keepdim=True)
        dp = torch.matmul(do, vf.transpose(-1, -2))
        ds = p * (dp - delta)
        dq[:, :, r0:r1] = torch.matmul(ds, kf) * scale
        dk += torch.matmul(ds.transpose(-1, -2), qf[:, :, r0:r1]) * scale
        dv += torch.matmul(p.transpose(-1, -2), do)
    return dq.float(), dk.float(), dv.float()


# ----------------------------------------------------------------------------------------------
# a8: mean pooling of K/V; a9: LSE combine
# ----------------------------------------------------------------------------------------------
def simple_pooling(x: torch.Tensor, gap: int, store_dtype=None) -> torch.Tensor:
    """TR/cogvideo_blocksparseattn.py:83-88 — replicate-pad to a multiple of ``gap`` and mean
    groups of ``gap`` consecutive (reordered) tokens; fp32 accumulate, stored in x.dtype."""
    store_dtype = store_dtype or x.dtype
    xp = pad_replicate(x.float(), gap)
    B, H, L, D = xp.shape
    return xp.reshape(B, H, L // gap, gap, D).mean(-2).to(store_dtype)


def simple_pooling_bwd(dxp: torch.Tensor, L: int, gap: int) -> torch.Tensor:
    """Adjoint of simple_pooling: each pooled row's gradient / gap to its ``gap`` sources;
    replicate-padded rows fold onto the last token (F.pad replicate backward)."""
    B, H, Lp, D = dxp.shape
    g = (dxp.float() / gap).repeat_interleave(gap, dim=2)       # [B,H,Lp*gap,D]
    dx = g[:, :, :L].clone()
    if Lp * gap > L:
        dx[:, :, L - 1] += g[:, :, L:].sum(2)
    return dx


def combine_reference(out1: torch.Tensor, lse1: torch.Tensor, out2: torch.Tensor,
                      lse2: torch.Tensor, gap: int, dtype=torch.bfloat16):
    """TR/cogvideo_blocksparseattn.py:374-393 executed op-by-op in ``dtype`` (each eager op
    computes in fp32 and rounds to ``dtype``); lse1/lse2 are first cast to ``dtype`` (:324).
    Returns (out [B,H,L,D] in fp32 holding ``dtype`` values, alpha)."""
    R = lambda t: rnd(t, dtype)  # noqa: E731
    l1 = R(lse1.float())[..., None]
    l2 = R(lse2.float())[..., None]
    log_g = R(torch.log(R(torch.tensor(float(gap)))))
    w2 = R(l2 + log_g)
    mx = torch.maximum(l1, w2)
    e1 = R(torch.exp(R(l1 - mx)))
    e2 = R(torch.exp(R(w2 - mx)))
    alpha = R(e1 / R(e1 + e2))
    o = R(R(R(out1.float()) * alpha) + R(R(out2.float()) * R(1.0 - alpha)))
    return o, alpha


# ----------------------------------------------------------------------------------------------
# whole adaptive path (a1-a9)
# ----------------------------------------------------------------------------------------------
class AdaptiveConfig:
    """Reference module-level globals (TR/cogvideo_blocksparseattn.py:9-16; wanx :9-16)."""

    def __init__(self, variant="cog", width=45, height=30, depth=13, text_length=226,
                 sample_gap=15, min_retain_ratio=0.05, max_retain_ratio=0.1,
                 energy_threshold=0.95, block=128, num_keep=32, use_rearrange=True):
        self.variant = variant
        self.width, self.height, self.depth = width, height, depth
        self.text_length = text_length
        self.sample_gap = sample_gap
        self.min_retain_ratio, self.max_retain_ratio = min_retain_ratio, max_retain_ratio
        self.energy_threshold = energy_threshold
        self.block, self.num_keep = block, num_keep
        self.use_rearrange = use_rearrange

    @property
    def force_tail(self):
        return 2 if self.variant == "cog" else 0

    @staticmethod
    def cogvideox(**kw):
        return AdaptiveConfig(**{**dict(variant="cog"), **kw})

    @staticmethod
    def wan(**kw):
        base = dict(variant="wan", width=52, height=30, depth=21, text_length=0, sample_gap=30,
                    min_retain_ratio=0.05, max_retain_ratio=0.17)
        return AdaptiveConfig(**{**base, **kw})


def predict_mask(q_r, k_r, cfg: AdaptiveConfig, q_off, k_off, store_dtype=torch.bfloat16):
    """efficient_attn_with_pooling + transfer_attn_to_mask (TR/cogvideo_blocksparseattn.py:57-82,
    343-358) on already-reordered q, k. Returns (po, mask)."""
    D = q_r.shape[-1]
    qs = sample_tokens(pad_replicate(q_r, cfg.block), q_off, cfg.block)
    ks = sample_tokens(pad_replicate(k_r, cfg.block), k_off, cfg.block)
    po = pooled_scores(qs, ks, 1.0 / (D ** 0.5), cfg.num_keep, store_dtype)
    nb = po.shape[-1]
    lo, hi = retain_counts(nb, cfg.min_retain_ratio, cfg.max_retain_ratio, cfg.variant)
    mask = energy_mask(po, lo, hi, cfg.energy_threshold, cfg.force_tail, store_dtype)
    return po, mask


def adaptive_attention(q, k, v, cfg: AdaptiveConfig, q_off, k_off, mask=None,
                       store_dtype=torch.bfloat16):
    """AdaptiveBlockSparseAttnTrain.forward (TR/cogvideo_blocksparseattn.py:405-427) +
    adaptive_block_sparse_attn (:327-394), reference-faithful rounding (out1/out2 rounded to the
    storage dtype, bf16 combine). Returns dict with out (original order, fp32 values),
    mask, po, sparsity, and the intermediate branch results."""
    from gilbert_oracle import full_sequence_perm  # local import: oracle dir is on sys.path
    B, H, L, D = q.shape
    if cfg.use_rearrange:
        P = torch.from_numpy(full_sequence_perm(cfg.width, cfg.height, cfg.depth, cfg.text_length))
    else:
        P = torch.arange(L)
    assert P.numel() == L
    q_r, k_r, v_r = q[:, :, P], k[:, :, P], v[:, :, P]
    po = None
    if mask is None:
        po, mask = predict_mask(q_r, k_r, cfg, q_off, k_off, store_dtype)
    out1, lse1 = block_sparse_attention(q_r, k_r, v_r, mask, block=cfg.block)
    kp = simple_pooling(k_r, cfg.sample_gap, store_dtype)
    vp = simple_pooling(v_r, cfg.sample_gap, store_dtype)
    out2, lse2 = block_sparse_attention(q_r, kp, vp, None, block=cfg.block)
    out_r, alpha = combine_reference(rnd(out1, store_dtype), lse1, rnd(out2, store_dtype), lse2,
                                     cfg.sample_gap, store_dtype)
    inv = torch.empty_like(P)
    inv[P] = torch.arange(L)
    sparsity = 1.0 - mask.float().mean().item() - 1.0 / cfg.sample_gap
    return dict(out=out_r[:, :, inv], out_r=out_r, mask=mask, po=po, perm=P, out1=out1, lse1=lse1,
                out2=out2, lse2=lse2, kp=kp, vp=vp, alpha=alpha, sparsity=sparsity)


def adaptive_attention_joint(q, k, v, cfg: AdaptiveConfig, mask):
    """The single-softmax identity of a9 (no intermediate rounding): softmax over the kept
    full-resolution keys united with the pooled keys carrying a +ln(gap) bias. Equal to
    ``adaptive_attention`` up to the reference's bf16 rounding of out1/out2/lse/alpha."""
    from gilbert_oracle import full_sequence_perm
    B, H, L, D = q.shape
    P = (torch.from_numpy(full_sequence_perm(cfg.width, cfg.height, cfg.depth, cfg.text_length))
         if cfg.use_rearrange else torch.arange(L))
    q_r, k_r, v_r = q[:, :, P], k[:, :, P], v[:, :, P]
    out1, lse1 = block_sparse_attention(q_r, k_r, v_r, mask, block=cfg.block)
    kp = simple_pooling(k_r, cfg.sample_gap)
    vp = simple_pooling(v_r, cfg.sample_gap)
    out2, lse2 = block_sparse_attention(q_r, kp, vp, None, block=cfg.block,
                                        key_bias=math.log(cfg.sample_gap))
    lse = torch.logaddexp(lse1, lse2)
    a = torch.exp(lse1 - lse)[..., None]
    out_r = out1 * a + out2 * (1 - a)
    inv = torch.empty_like(P)
    inv[P] = torch.arange(L)
    return out_r[:, :, inv], lse


def joint_from_branches(fwd: dict, log_gap: float) -> torch.Tensor:
    """Exact (fp64) single-softmax combine of ``adaptive_attention``'s unrounded branch results
    (out1/lse1, out2/lse2): the a9 identity with no bf16 rounding of lse, alpha or the branch
    outputs, the pooled keys carrying the bias ``log_gap`` (the reference's combine uses the bf16
    value of ln g, :375-376). Returns the output in the original token order (fp64)."""
    l1 = fwd["lse1"].double()
    l2 = fwd["lse2"].double() + log_gap
    lse = torch.logaddexp(l1, l2)
    a = torch.exp(l1 - lse)[..., None]
    out_r = fwd["out1"].double() * a + fwd["out2"].double() * (1 - a)
    P = fwd["perm"]
    inv = torch.empty_like(P)
    inv[P] = torch.arange(P.numel())
    return out_r[:, :, inv]


def bf16_ulp_distance(got: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """Checker utility: |bf16(got) - bf16(ref)| in bf16 units in the last place at the reference's
    magnitude, with magnitudes below the tensor's RMS binade measured in that binade's ULP (an
    output near zero from cancellation is judged at the scale of the tensor, not in ULPs of its
    own tiny value). bf16 keeps 8 significant bits: ULP(x) = 2^(floor(log2|x|) - 7). int64."""
    g = got.float().to(torch.bfloat16).double()
    r = ref.float().to(torch.bfloat16).double()
    rms = float(r.pow(2).mean().sqrt())
    floor = 2.0 ** math.floor(math.log2(rms)) if rms > 0 else 2.0 ** -126
    mag = torch.clamp(r.abs(), min=floor)
    ulp = torch.exp2(torch.floor(torch.log2(mag)) - 7)
    return torch.round((g - r).abs() / ulp).to(torch.int64)


ULP_BUCKETS = ((0, 0), (1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, None))


def bf16_ulp_histogram(got: torch.Tensor, ref: torch.Tensor) -> dict:
    """Fractions of elements per bf16-ULP distance bucket (0, 1, 2, 3-4, 5-8, 9-16, >16; see
    bf16_ulp_distance), plus the maximum distance (SURVEY §8d Quality)."""
    d = bf16_ulp_distance(got, ref).flatten()
    n = d.numel()
    hist = {}
    for lo, hi in ULP_BUCKETS:
        sel = (d >= lo) if hi is None else ((d >= lo) & (d <= hi))
        key = f">{lo - 1}" if hi is None else (str(lo) if lo == hi else f"{lo}-{hi}")
        hist[key] = round(int(sel.sum()) / n, 6)
    return {"ulp_hist": hist, "max_ulp": int(d.max()), "n": n,
            "ulp_unit": "bf16 ULP at |ref|, floored at the RMS binade of ref"}


def adaptive_attention_bwd(q, k, v, dout, cfg: AdaptiveConfig, fwd: dict):
    """Gradient of adaptive_attention w.r.t. q, k, v under the reference's autograd semantics
    (a10): mask under no_grad; LSEs carry no gradient (FA2 convention) so alpha is a constant;
    dO1 = alpha dO, dO2 = (1-alpha) dO; each branch's backward uses its own output and LSE;
    pooled-branch K/V grads flow back through the mean pool; the Gilbert gather transposes.
    fp32/fp64 arithmetic (no bf16 emulation of the backward)."""
    P = fwd["perm"]
    L = q.shape[2]
    q_r, k_r, v_r = q[:, :, P], k[:, :, P], v[:, :, P]
    do_r = dout.float()[:, :, P]
    a = fwd["alpha"]
    do1, do2 = do_r * a, do_r * (1 - a)
    dq1, dk1, dv1 = block_sparse_attention_bwd(q_r, k_r, v_r, fwd["out1"], fwd["lse1"], do1,
                                               fwd["mask"], block=cfg.block)
    dq2, dkp, dvp = block_sparse_attention_bwd(q_r, fwd["kp"], fwd["vp"], fwd["out2"], fwd["lse2"],
                                               do2, None, block=cfg.block)
    dq_r = dq1 + dq2
    dk_r = dk1 + simple_pooling_bwd(dkp, L, cfg.sample_gap)
    dv_r = dv1 + simple_pooling_bwd(dvp, L, cfg.sample_gap)
    inv = torch.empty_like(P)
    inv[P] = torch.arange(L)
    return dq_r[:, :, inv], dk_r[:, :, inv], dv_r[:, :, inv]


def _branch_bwd(q, k, v, out, lse, dout, w, block_mask, scale, block, rdtype):
    """One branch of two_branch_attention_bwd in fp64: the probabilities carry the row weight ``w``
    (w*P = w*exp(S*scale - lse)); rows with lse = +-inf or w = 0 contribute nothing. ``rdtype`` not
    None: w*P and dS are rounded to that storage dtype before the three products, as the kernels
    feed them to the MFMAs (dS itself is formed from the unrounded w*P). Returns fp64 (dq, dk, dv)."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    R = (lambda t: t) if rdtype is None else (lambda t: t.to(rdtype).double())
    qf, kf, vf, of, dof = (t.double() for t in (q, k, v, out, dout))
    lse, w = lse.double(), w.double()
    live = torch.isfinite(lse) & (w > 0)
    lse_s = torch.where(live, lse, torch.zeros_like(lse))
    w_s = torch.where(live, w, torch.zeros_like(w))
    dq = torch.zeros(B, H, Lq, D, dtype=torch.float64)
    dk = torch.zeros(B, H, Lk, D, dtype=torch.float64)
    dv = torch.zeros(B, H, Lk, D, dtype=torch.float64)
    keycol_block = torch.arange(Lk) // block
    for i in range((Lq + block - 1) // block):
        r0, r1 = i * block, min(Lq, (i + 1) * block)
        s = torch.matmul(qf[:, :, r0:r1], kf.transpose(-1, -2)) * scale
        if block_mask is not None:
            keep = block_mask[:, :, i, :].bool()[:, :, keycol_block]
            s = s.masked_fill(~keep[:, :, None, :], float("-inf"))
        p = torch.exp(s - lse_s[:, :, r0:r1, None]) * w_s[:, :, r0:r1, None]
        do = dof[:, :, r0:r1]
        delta = (do * of[:, :, r0:r1]).sum(-1, keepdim=True)
        ds = R(p * (torch.matmul(do, vf.transpose(-1, -2)) - delta))
        p = R(p)
        dq[:, :, r0:r1] = torch.matmul(ds, kf) * scale
        dk += torch.matmul(ds.transpose(-1, -2), qf[:, :, r0:r1]) * scale
        dv += torch.matmul(p.transpose(-1, -2), do)
    return dq, dk, dv


def kept_key_rows(mask_row, Lk, block=128):
    """The key rows one q-block's mask row [>= ceil(Lk/block)] keeps, ascending, as the kernels' lists
    hold them. A bool row keeps a block once; an integer row keeps block j ``mask_row[j]`` times (a
    deliberately wrong list for testing the error metric: an entry counted twice)."""
    nbk = (Lk + block - 1) // block
    m = mask_row[:nbk]
    blocks = torch.nonzero(m).flatten()
    if m.dtype != torch.bool:
        blocks = blocks.repeat_interleave(m[blocks].long())
    rows = (blocks[:, None] * block + torch.arange(block)).flatten()
    return rows[rows < Lk]


def gathered_attention(q, k, v, block_mask, *, kp=None, vp=None, bias=0.0, use_main=True, sm_scale=None,
                       block=128, emulate=None):
    """joint_attention (``emulate`` None; fp64) or attention_fwd_emulated (``emulate`` = its keyword
    arguments store_dtype, prescale_q, m_lag; fp32) for long sequences: per (b, h, q-block) the kept
    key blocks are gathered, followed by the pooled keys, and the same arithmetic runs on them with
    everything visible, so the work follows the mask's density instead of Lq x Lk. ``block_mask``
    None = dense. A q-block without a key gives zero rows and -inf LSE. ``m_lag`` is [B,H,Lq,1] or
    None. Returns (out, lse) as the dense form does."""
    B, H, Lq, D = q.shape
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(D)
    Lk = k.shape[2] if use_main else 0
    Lkp = 0 if kp is None else kp.shape[2]
    nbq = (Lq + block - 1) // block
    dt = torch.float64 if emulate is None else torch.float32
    out = torch.zeros(B, H, Lq, D, dtype=dt)
    lse = torch.full((B, H, Lq), float("-inf"), dtype=dt)
    every = torch.arange(Lk)
    m = None if block_mask is None else block_mask.expand(B, H, *block_mask.shape[2:])
    if emulate is not None:
        emulate = dict(emulate)
        lag = emulate.pop("m_lag", None)
        pooled_bias2 = float(np.float32(bias) * LOG2E_F32)
    for b in range(B):
        for h in range(H):
            pk = () if kp is None else (kp[b:b + 1, h:h + 1],)
            pv = () if kp is None else (vp[b:b + 1, h:h + 1],)
            for i in range(nbq):
                r0, r1 = i * block, min(Lq, (i + 1) * block)
                rows = every if m is None else kept_key_rows(m[b, h, i], Lk, block)
                n = rows.numel() * bool(use_main)
                if n + Lkp == 0:
                    continue
                K = torch.cat(((k[b:b + 1, h:h + 1, rows],) if n else ()) + pk, 2)
                V = torch.cat(((v[b:b + 1, h:h + 1, rows],) if n else ()) + pv, 2)
                vis = torch.ones(1, 1, r1 - r0, n + Lkp, dtype=torch.bool)
                qb = q[b:b + 1, h:h + 1, r0:r1]
                if emulate is None:
                    kb = torch.cat((torch.zeros(n, dtype=torch.float64), torch.full((Lkp,), float(bias), dtype=torch.float64)))
                    o, l = softmax_over_visible(qb, K, V, vis, kb, scale)
                else:
                    kb = torch.cat((torch.zeros(n), torch.full((Lkp,), pooled_bias2)))
                    o, l = fwd_emulated_over_visible(qb, K, V, vis, kb, scale, m_lag=None if lag is None else lag[b:b + 1, h:h + 1, r0:r1],
                                                     **emulate)
                out[b, h, r0:r1], lse[b, h, r0:r1] = o[0, 0], l[0, 0]
    return out, lse


def _branch_bwd_gathered(q, k, v, out, lse, dout, w, block_mask, scale, block, rdtype, kv_mask=None, full_tail=False):
    """_branch_bwd for long sequences: per (b, h, q-block) the kept key blocks are gathered, the same
    arithmetic with the same ``rdtype`` rounding points runs on them, and dk/dv are scatter-added.

    Two deliberately wrong forms, for testing the error metric against the lists the kernels build:
      * ``kv_mask`` (bool or integer counts, as kept_key_rows): the dK/dV side takes its (q-block,
        key block) pairs from it while dQ keeps ``block_mask``'s, as a dK/dV kernel with a wrong
        q-list would; an integer ``block_mask`` counts a key-list entry more than once in dQ.
      * ``full_tail``: a last block of at most block/2 rows is treated as if its second half-tile held
        block/2 more copies of the last row (the kernels skip that half-tile, ``ntiles -= 1``; their
        loads clamp to the last row): the last key block's copies enter dQ, the last q-block's dK/dV."""
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    R = (lambda t: t) if rdtype is None else (lambda t: t.to(rdtype).double())
    qf, kf, vf, of, dof = (t.double() for t in (q, k, v, out, dout))
    lse, w = lse.double(), w.double()
    live = torch.isfinite(lse) & (w > 0)
    lse_s = torch.where(live, lse, torch.zeros_like(lse))
    w_s = torch.where(live, w, torch.zeros_like(w))
    delta = (dof * of).sum(-1, keepdim=True)
    dq = torch.zeros(B, H, Lq, D, dtype=torch.float64)
    dk = torch.zeros(B, H, Lk, D, dtype=torch.float64)
    dv = torch.zeros(B, H, Lk, D, dtype=torch.float64)
    nbq = (Lq + block - 1) // block
    half = block // 2
    q_extra = full_tail and Lq - (nbq - 1) * block <= half
    k_extra = full_tail and Lk - (Lk - 1) // block * block <= half
    if block_mask is None:
        block_mask = torch.ones(1, 1, nbq, (Lk + block - 1) // block, dtype=torch.bool)
    m = block_mask.expand(B, H, *block_mask.shape[2:])
    mkv = None if kv_mask is None else kv_mask.expand(B, H, *kv_mask.shape[2:])

    def products(b, h, qrows, krows):
        """(dS, w*P, K rows, V rows) of the query rows ``qrows`` against the key rows ``krows``."""
        Kg, Vg = kf[b, h, krows], vf[b, h, krows]
        s = torch.matmul(qf[b, h, qrows], Kg.transpose(-1, -2)) * scale
        p = torch.exp(s - lse_s[b, h, qrows, None]) * w_s[b, h, qrows, None]
        ds = R(p * (torch.matmul(dof[b, h, qrows], Vg.transpose(-1, -2)) - delta[b, h, qrows]))
        return ds, R(p), Kg

    for b in range(B):
        for h in range(H):
            for i in range(nbq):
                qrows = torch.arange(i * block, min(Lq, (i + 1) * block))
                krows = kept_key_rows(m[b, h, i], Lk, block)
                split = mkv is not None and not torch.equal(mkv[b, h, i].long(), m[b, h, i].long())
                if krows.numel():
                    kq = krows
                    if k_extra and int(krows[-1]) == Lk - 1:
                        kq = torch.cat((krows, torch.full((half,), Lk - 1)))
                    ds, p, Kg = products(b, h, qrows, kq)
                    dq[b, h, qrows] = torch.matmul(ds, Kg) * scale
                last_q = q_extra and i == nbq - 1
                if split or last_q or (krows.numel() and kq is not krows):
                    krows = kept_key_rows(mkv[b, h, i], Lk, block) if split else krows
                    if last_q:
                        qrows = torch.cat((qrows, torch.full((half,), Lq - 1)))
                    if krows.numel():
                        ds, p, _ = products(b, h, qrows, krows)
                if krows.numel():
                    dk[b, h].index_add_(0, krows, torch.matmul(ds.transpose(-1, -2), qf[b, h, qrows]) * scale)
                    dv[b, h].index_add_(0, krows, torch.matmul(p.transpose(-1, -2), dof[b, h, qrows]))
    return dq, dk, dv


def two_branch_attention_bwd(q_r, k_r, v_r, kp, vp, out1, lse1, out2, lse2, alpha, dout, mask, gap,
                             sm_scale=None, store_dtype=torch.bfloat16, emulate_rounding=False,
                             block=128, replicate_fold=True, gathered=False, kv_mask=None, full_tail=False):
    """Op-level statement of vb_attn_bwd (include/vblade.h), every tensor in REORDERED row order:
    the gradient w.r.t. q_r [B,H,Lq,D], k_r, v_r [B,H,Lk,D] of
        alpha * BSA(q_r, k_r, v_r; mask)  +  storage(1 - alpha) * SDPA(q_r, pool(k_r), pool(v_r))
    with both LSEs and alpha constants (a10; cogvideo_blocksparseattn.py:366-393): dO1 = alpha dO,
    dO2 = storage(1-alpha) dO, each branch through block_sparse_attention_bwd's semantics with its
    own output and LSE (out1/lse1, out2/lse2 as the forward wrote them), the pooled K/V gradients
    folded back through simple_pooling_bwd. ``alpha`` [B,H,Lq] is any constant in [0,1] per row.
    kp None: the main branch alone (alpha None = 1). Rows with lse = +-inf contribute nothing.
    Lq != Lk (mask [B,H,ceil(Lq/block),ceil(Lk/block)]) and ``sm_scale`` are honoured.

    ``emulate_rounding``: the same in fp64 but rounded to ``store_dtype`` exactly where the kernels
    round (csrc/vb_attn_bwd.hip): the weighted probabilities w*P and dS of each branch (the MFMA
    operands), and the three results (dq of both branches, dk/dv after the pool fold, summed in the
    accumulator and rounded once). ``replicate_fold=False`` drops the replicate-padding term of the
    mean-pool adjoint: a deliberately wrong reference for testing the error metric.
    ``gathered``: the main branch through _branch_bwd_gathered (long sequences under a sparse mask: the
    same arithmetic on each q-block's kept key blocks; equal to the dense form up to fp64 summation
    order); the pooled branch stays dense (Lkp is small). ``kv_mask`` and ``full_tail`` are that
    function's deliberately wrong lists.
    Returns fp32 (dq_r, dk_r, dv_r)."""
    D = q_r.shape[-1]
    Lk = k_r.shape[2]
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(D)
    rd = store_dtype if emulate_rounding else None
    w1 = torch.ones(q_r.shape[:3]) if alpha is None else alpha.float()
    if gathered:
        dq, dk, dv = _branch_bwd_gathered(q_r, k_r, v_r, out1, lse1, dout, w1, mask, scale, block, rd, kv_mask, full_tail)
    else:
        assert kv_mask is None and not full_tail
        dq, dk, dv = _branch_bwd(q_r, k_r, v_r, out1, lse1, dout, w1, mask, scale, block, rd)
    if kp is not None:
        w2 = rnd(1.0 - w1, store_dtype)
        dq2, dkp, dvp = _branch_bwd(q_r, kp, vp, out2, lse2, dout, w2, None, scale, block, rd)
        dq = dq + dq2
        for g, gp in ((dk, dkp), (dv, dvp)):
            e = (gp / gap).repeat_interleave(gap, dim=2)
            g += e[:, :, :Lk]
            if replicate_fold and e.shape[2] > Lk:
                g[:, :, Lk - 1] += e[:, :, Lk:].sum(2)
    if emulate_rounding:
        dq, dk, dv = (t.to(store_dtype) for t in (dq, dk, dv))
    return dq.float(), dk.float(), dv.float()


def per_row_errors(g: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """err[b,h,r] = ||g[b,h,r] - ref[b,h,r]|| / max(||ref[b,h,r]||, rms), rms = the root-mean-square
    row norm of ``ref`` (rows whose reference is near zero are judged at the tensor's scale); a NaN
    counts as inf. fp64 [B,H,L]."""
    g, ref = g.detach().double().cpu(), ref.detach().double().cpu()
    rn = ref.norm(dim=-1)
    rms = rn.pow(2).mean().sqrt().clamp_min(1e-300)
    err = (g - ref).norm(dim=-1) / torch.maximum(rn, rms)
    return torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)


def per_row_error(g: torch.Tensor, ref: torch.Tensor):
    """Checker metric that a single wrong row cannot hide in: the worst of per_row_errors.
    Returns (worst error, (b, h, r) of that row)."""
    err = per_row_errors(g, ref)
    i = int(err.argmax())
    return float(err.flatten()[i]), tuple(int(x) for x in np.unravel_index(i, err.shape))


# the most a derived per-row bound may be: ~2.4x / ~3x the worst row the emulation shows (3.3-4.2e-3
# bf16, 3.8-5.1e-4 f16 on the backward tests' shapes), so a loose emulation cannot loosen the tests
PER_ROW_CAP = {torch.bfloat16: 1e-2, torch.float16: 1.5e-3}


def per_row_bound(emu: torch.Tensor, ref: torch.Tensor, store_dtype) -> float:
    """The backward tests' per-row bound for one gradient: 2x the worst per-row error of the rounding
    emulation against the unrounded reference on the same inputs (the factor covers the spread of a
    maximum over rows and the kernels' fp32 summation order, not kernel error), which must itself
    stay under PER_ROW_CAP."""
    bound = 2.0 * per_row_error(emu, ref)[0]
    assert 0 < bound <= PER_ROW_CAP[store_dtype], (bound, PER_ROW_CAP[store_dtype])
    return bound


def block_mask_from_density(B, H, nbq, nbk, density, seed=3):
    """BASELINE.md §3 synthetic mask: (rand < density) | eye, at least one block per row."""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(B, H, nbq, nbk, generator=g) < density
    eye = torch.zeros(nbq, nbk, dtype=torch.bool)
    d = min(nbq, nbk)
    eye[torch.arange(d), torch.arange(d)] = True
    return m | eye
