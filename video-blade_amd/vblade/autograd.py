"""autograd.Function wrappers with the reference's gradient semantics.

* ``block_sparse_attn_func`` — drop-in for mit-han-lab/Block-Sparse-Attention's function of the
  same name as called at cogvideo_blocksparseattn.py:316-320 (differentiable in q, k, v; the
  returned LSE carries no gradient, FlashAttention-2 convention).
* ``adaptive_split_attention`` — adaptive_block_sparse_attn's two-branch form (:366-393): block-
  sparse branch + pooled dense branch + bf16 LSE combine. Under autograd alpha is a constant
  (both LSEs are detached), so dO1 = alpha*dO, dO2 = (1-alpha)*dO and each branch back-propagates
  with its own output and LSE; pooled-branch K/V gradients flow back through the mean pool.
* ``adaptive_joint_attention`` — the one-softmax form the inference call evaluates, with its exact
  gradient (nothing held constant but the block mask): one attention launch forward, one
  ``ops.attention_bwd_joint`` call backward. Opt-in (``grad_combine="joint"``); it is not the
  reference's gradient, which drops the term (out1 - out2)·d alpha.
"""
from __future__ import annotations

import torch

from . import ops

# The training forward's pooled-only branch (every query against the pooled keys) on a side stream
# beside the block-sparse branch: the two launches share only their inputs, so they can fill each
# other's last rounds. Scheduling only: the same bits (tools/ab.py --what trainfwd,
# profiles/r06_trainfwd_fork_ab.log): Wan (D=128) 1.031-1.034x, CogVideoX 0.989-0.992x, so D=128 only.
FORK_POOLED_BRANCH = True
_SIDE_STREAMS = {}


def _dout(dout: torch.Tensor, io_layout: str) -> torch.Tensor:
    """The incoming gradient as the backward ops take it: a contiguous copy on the default path, as it
    comes with io_layout "blhd" (the ops read it through its strides and copy only what misses the
    16-byte rule)."""
    return dout if io_layout == "blhd" else dout.contiguous()


def _side_stream(dev: torch.device) -> torch.cuda.Stream:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    st = _SIDE_STREAMS.get(idx)
    if st is None:
        st = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=idx)
    return st


class _BlockSparseAttnFunc(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_q, cu_k, head_mask_type, streaming_info, base_blockmask,
                max_q, max_k, p_dropout, deterministic, softmax_scale, is_causal, exact_streaming,
                mask_head_mode):
        out, lse = ops.block_sparse_attn_fwd(q, k, v, cu_q, cu_k, head_mask_type, streaming_info,
                                             base_blockmask, max_q, max_k, p_dropout,
                                             deterministic, softmax_scale, is_causal,
                                             exact_streaming, mask_head_mode=mask_head_mode)
        ctx.save_for_backward(q, k, v, out, lse, cu_q, cu_k, head_mask_type, base_blockmask)
        ctx.meta = (max_q, max_k, softmax_scale, mask_head_mode)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, cu_q, cu_k, hmt, mask = ctx.saved_tensors
        max_q, max_k, scale, mode = ctx.meta
        dq, dk, dv = ops.block_sparse_attn_bwd(dout, q, k, v, out, lse, cu_q, cu_k, hmt, None,
                                               mask, max_q, max_k, softmax_scale=scale,
                                               mask_head_mode=mode)
        return (dq, dk, dv) + (None,) * 13


def block_sparse_attn_func(q_unpad, k_unpad, v_unpad, cu_seqlens_q, cu_seqlens_k, head_mask_type,
                           streaming_info, base_blockmask, max_seqlen_q_, max_seqlen_k_, p_dropout,
                           deterministic=False, softmax_scale=None, is_causal=False,
                           exact_streaming=False, return_attn_probs=False, mask_head_mode="per_head"):
    """Same signature and return convention as the reference's external op. ``mask_head_mode``
    (keyword, not in the reference's signature): the reading of head_mask_type's ones that SURVEY
    Appendix B leaves open offline ("per_head" default, "shared_head0")."""
    out, lse = _BlockSparseAttnFunc.apply(q_unpad, k_unpad, v_unpad, cu_seqlens_q, cu_seqlens_k,
                                          head_mask_type, streaming_info, base_blockmask,
                                          max_seqlen_q_, max_seqlen_k_, p_dropout, deterministic,
                                          softmax_scale, is_causal, exact_streaming, mask_head_mode)
    if return_attn_probs:
        return out, lse, None
    return out


class _AdaptiveSplitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, mask, rows, gap, heavy_rows, io_layout="bhld"):
        kp, vp, k_r, v_r = ops.pool_kv(k, v, gap, rows, reordered=True)
        # the persistent (work-queue) launch at D=128: Wan's LSE forward 1.024-1.030x, CogVideoX's
        # 0.98x (profiles/r06_persist_unscoped_ab.log); bit-identical either way. Captured into a graph
        # on a stream that has no queue yet, the launch is per q-block (ops.work_queue makes none there)
        fork = FORK_POOLED_BRANCH and q.is_cuda and q.shape[-1] == 128
        if fork:
            cur = torch.cuda.current_stream(q.device)
            side = _side_stream(q.device)
            side.wait_stream(cur)   # kp/vp and q are ready
            with torch.cuda.stream(side):
                out2, lse2 = ops.attention_fwd(q, None, None, use_main=False, q_rows=rows, kp=kp,
                                               vp=vp, need_lse=True)
        else:
            out2, lse2 = ops.attention_fwd(q, None, None, use_main=False, q_rows=rows, kp=kp, vp=vp,
                                           need_lse=True)
        out1, lse1 = ops.attention_fwd(q, k_r, v_r, block_mask=mask, q_rows=rows, need_lse=True,
                                       heavy_rows=heavy_rows, persistent=q.shape[-1] == 128)
        if fork:
            cur.wait_stream(side)
            for t in (q, kp, vp, rows):   # read on the side stream: not reused before it is done
                if t is not None:
                    t.record_stream(side)
            out2.record_stream(cur)
            lse2.record_stream(cur)
        # io_layout "blhd": the combine (the call's last pass) stores the output in projection layout
        # through its strides; the two branch outputs stay contiguous, they never leave this function
        out, alpha = ops.lse_combine(out1, lse1, out2, lse2, gap, out_layout=io_layout)
        ctx.save_for_backward(q, k_r, v_r, mask, rows, out1, lse1, out2, lse2, alpha, kp, vp)
        ctx.gap = gap
        ctx.heavy_rows = heavy_rows
        ctx.io_layout = io_layout
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k_r, v_r, mask, rows, out1, lse1, out2, lse2, alpha, kp, vp = ctx.saved_tensors
        # per-branch FA2 backward with dO1 = alpha*dO, dO2 = (1-alpha)*dO; pooled-branch K/V grads
        # through the mean pool and the Gilbert gather, returned in the caller's row order
        dq, dk, dv = ops.attention_bwd(_dout(dout, ctx.io_layout), q, k_r, v_r, out1, lse1, block_mask=mask,
                                       q_rows=rows, kv_rows=rows, kp=kp, vp=vp, out2=out2,
                                       lse2=lse2, alpha=alpha, gap=ctx.gap, heavy_rows=ctx.heavy_rows,
                                       grad_layout=ctx.io_layout)
        return dq, dk, dv, None, None, None, None, None


def adaptive_split_attention(q, k, v, mask, rows, gap, heavy_rows=2, io_layout="bhld"):
    """heavy_rows: forced-dense tail rows dispatched first (CogVideoX 2, Wan 0); scheduling only.
    io_layout: "bhld" (default) or "blhd": the output and dq, dk, dv are the [B,H,L,D] views of
    [B,L,H,D] memory (the projections' layout) and the incoming gradient is read through its strides
    (a copy only when it misses the kernels' 16-byte rule). The same values either way."""
    return _AdaptiveSplitFn.apply(q, k, v, mask, rows, gap, heavy_rows, ops.io_layout_code("io_layout", io_layout))


class _AdaptiveJointFn(torch.autograd.Function):
    """The inference call under autograd: ONE attention launch (kept keys ∪ biased pooled keys, LSE
    stored) forward, ops.attention_bwd_joint backward. k_r/v_r/kp/vp come from the detached k/v; the
    backward folds the pooled keys' gradients through the mean pool and scatters to the caller's rows."""

    @staticmethod
    def forward(ctx, q, k, v, mask, rows, gap, kp_log_bias, heavy_rows, pooled, io_layout="bhld"):
        kp, vp, k_r, v_r = pooled if pooled is not None else ops.pool_kv(k, v, gap, rows, reordered=True)
        out, lse = ops.attention_fwd(q, k_r, v_r, block_mask=mask, q_rows=rows, kp=kp, vp=vp,
                                     kp_log_bias=kp_log_bias, need_lse=True, heavy_rows=heavy_rows,
                                     persistent=q.shape[-1] == 128, out_layout=io_layout)
        ctx.save_for_backward(q, k_r, v_r, kp, vp, out, lse, mask, rows)
        ctx.gap = gap
        ctx.io_layout = io_layout
        ctx.kp_log_bias = kp_log_bias
        ctx.heavy_rows = heavy_rows
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k_r, v_r, kp, vp, out, lse, mask, rows = ctx.saved_tensors
        dq, dk, dv = ops.attention_bwd_joint(_dout(dout, ctx.io_layout), q, k_r, v_r, out, lse, block_mask=mask,
                                             q_rows=rows, kv_rows=rows, kp=kp, vp=vp, gap=ctx.gap,
                                             kp_log_bias=ctx.kp_log_bias, heavy_rows=ctx.heavy_rows,
                                             grad_layout=ctx.io_layout)
        return dq, dk, dv, None, None, None, None, None, None, None


def adaptive_joint_attention(q, k, v, mask, rows, gap, kp_log_bias, heavy_rows=2, pooled=None, io_layout="bhld"):
    """The one-softmax form the inference call evaluates (block-masked keys ∪ pooled keys with the
    logit bias ``kp_log_bias``), differentiable in q, k, v with its exact gradient: the mask is a
    constant, the pooled keys are the mean pool of the reordered k/v. ``pooled``: (kp, vp, k_r, v_r)
    already computed from the detached k/v (ops.pool_kv(..., reordered=True), or the predictor's
    pool= outputs), or None to run ops.pool_kv here. One attention launch forward, one
    ops.attention_bwd_joint call backward; saves q, k_r, v_r, kp, vp, out, lse, mask, rows.
    ``io_layout``: as adaptive_split_attention."""
    return _AdaptiveJointFn.apply(q, k, v, mask, rows, gap, kp_log_bias, heavy_rows, pooled,
                                  ops.io_layout_code("io_layout", io_layout))


class _QkPrologueFn(torch.autograd.Function):
    """ops.qk_prologue out of place forward, ops.qk_prologue_bwd backward. Nothing but the inputs is
    saved: the backward recomputes the norm's statistics."""

    @staticmethod
    def forward(ctx, q_proj, k_proj, q_weight, q_bias, k_weight, k_bias, kw):
        ctx.set_materialize_grads(False)   # a None output gradient leaves that tensor out of the launch
        ctx.kw = kw
        ctx.save_for_backward(q_proj, k_proj, q_weight, q_bias, k_weight, k_bias)
        return ops.qk_prologue(q_proj, k_proj, q_weight=q_weight, q_bias=q_bias, k_weight=k_weight,
                               k_bias=k_bias, **kw)

    @staticmethod
    def backward(ctx, gq, gk=None):
        q_proj, k_proj, q_weight, q_bias, k_weight, k_bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        use_q = gq is not None and (need[0] or need[2] or need[3])
        use_k = gk is not None and (need[1] or need[4] or need[5])
        if not (use_q or use_k):
            return (None,) * 7
        dq, dk, dqw, dqb, dkw, dkb = ops.qk_prologue_bwd(
            q_proj if use_q else None, k_proj if use_k else None, gq=gq if use_q else None,
            gk=gk if use_k else None, q_weight=q_weight, q_bias=q_bias, k_weight=k_weight, k_bias=k_bias,
            need_wgrad=(use_q and need[2], use_q and need[3], use_k and need[4], use_k and need[5]), **ctx.kw)

        def like(grad, param):   # the op sums in fp32; the gradient has the parameter's dtype and shape
            return None if grad is None else grad.to(param.dtype).view(param.shape)

        return (dq if need[0] else None, dk if need[1] else None, like(dqw, q_weight), like(dqb, q_bias),
                like(dkw, k_weight), like(dkb, k_bias), None)


def qk_prologue(q_proj, k_proj=None, *, heads, norm="none", q_weight=None, q_bias=None, q_eps=1e-5,
                k_weight=None, k_bias=None, k_eps=None, rope="none", rope_start=0, cos=None, sin=None,
                freqs=None):
    """``ops.qk_prologue`` (out of place; there is no ``inplace`` here: the backward reads the
    forward's input) differentiable in q_proj, k_proj and the norms' weights and biases, through
    ``ops.qk_prologue_bwd``. Returns the same [B,heads,L,D] view(s). The RoPE tables are constants:
    one that requires grad is refused. Parameter gradients are computed only where autograd asks
    for them and come back in the parameter's dtype."""
    for name, t in (("cos", cos), ("sin", sin), ("freqs", freqs)):
        if t is not None and t.requires_grad:
            raise ValueError(f"autograd.qk_prologue: {name} requires grad, but the RoPE tables get no gradient")
    kw = dict(heads=heads, norm=norm, q_eps=q_eps, k_eps=k_eps, rope=rope, rope_start=rope_start,
              cos=cos, sin=sin, freqs=freqs)
    return _QkPrologueFn.apply(q_proj, k_proj, q_weight, q_bias, k_weight, k_bias, kw)
