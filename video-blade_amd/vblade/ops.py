"""Torch-facing wrappers over the C ABI (include/vblade.h).

PyTorch supplies device memory and the current HIP stream only; every byte of the hot path is
computed by libvblade_hip.so. Calls on CPU tensors raise (there is no CPU fallback).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math
import os
from typing import Optional, Union

import numpy as np
import torch

from . import _lib
from ._lib import AttnArgs, BwdArgs, MlAttnArgs, MlBwdArgs, PredictArgs, check

BLOCK = 128
NUM_KEEP_VALUES = (16, 32, 64)   # sampled tokens per block the predictor is built for (default 32)
MAX_BLOCKS = 320         # vb_mask_predict's rows (L <= 40960)
MAX_BLOCKS_LONG = 1024   # vb_mask_predict_long's, the attention kernels' own limit (L <= 131072)


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return _lib.VB_DTYPE_BF16
    if t.dtype == torch.float16:
        return _lib.VB_DTYPE_F16
    raise TypeError(f"vblade: unsupported dtype {t.dtype} (bf16/fp16 only)")


def _require_gpu(*ts: Optional[torch.Tensor]):
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("vblade: tensors must live on a HIP (cuda) device; there is no CPU path")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("vblade: tensors on different devices")
    return dev


def _stream(dev) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _s3(t: torch.Tensor):
    """(batch, head, row) element strides of a [B,H,L,D] tensor with unit d-stride."""
    if t.stride(-1) != 1:
        raise ValueError("vblade: last dimension must be contiguous")
    return (ctypes.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def _aligned_bhld(t: torch.Tensor) -> torch.Tensor:
    """Return t if its strides/pointer satisfy the kernels' 16-byte rules, else a contiguous copy."""
    if (t.stride(-1) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0):
        return t
    return t.contiguous()


IO_LAYOUTS = ("bhld", "blhd")   # memory order of a [B,H,L,D] tensor the library allocates


def io_layout_code(name: str, layout: str) -> str:
    if layout not in IO_LAYOUTS:
        raise ValueError(f"{name} must be one of {list(IO_LAYOUTS)}, got {layout!r}")
    return layout


def _empty_bhld(B: int, H: int, L: int, D: int, dev, dtype, layout: str = "bhld") -> torch.Tensor:
    """An uninitialised [B,H,L,D] tensor: contiguous ("bhld"), or the [B,H,L,D] view of [B,L,H,D]
    memory ("blhd", the projections' [B,L,H*D] layout: transpose(1, 2).reshape(B, L, H*D) of it is a
    view). The kernels address either through its strides."""
    if layout == "blhd":
        return torch.empty(B, L, H, D, device=dev, dtype=dtype).transpose(1, 2)
    return torch.empty(B, H, L, D, device=dev, dtype=dtype)


_WORK_QUEUES = {}


def work_queue(dev) -> Optional[torch.Tensor]:
    """The persistent forward's work queue (include/vblade.h VB_WORK_QUEUE_INTS) for ``dev``'s current
    stream: int32, zero when allocated, and left zero by every launch that uses it. One per (device,
    stream), since two launches that may overlap must not share one.

    No queue is ever created while the stream is being captured into a graph: the zero-fill would
    become a graph node that has not run when another graph captured on the same stream finds the
    cached queue and is replayed first, and the memory would belong to the graph's private pool. With
    no queue for (device, stream) yet and a capture under way this returns None, allocates nothing
    and caches nothing; the callers then launch the one-workgroup-per-q-block form. A queue created
    eagerly beforehand (the warm-up calls torch asks for before a capture) is returned as always."""
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, _stream(dev))
    wq = _WORK_QUEUES.get(key)
    if wq is None:
        if torch.cuda.is_current_stream_capturing():
            return None
        wq = _WORK_QUEUES[key] = torch.zeros(_lib.VB_WORK_QUEUE_INTS, device=dev, dtype=torch.int32)
    return wq


def _work_queue_ptr(dev, persistent: bool):
    """vb_attn_args.work_queue of a launch: the stream's queue when ``persistent`` is asked for and a
    queue may be used (work_queue), else None, the one-workgroup-per-q-block form (the same bits)."""
    wq = work_queue(dev) if persistent else None
    return None if wq is None else wq.data_ptr()


def _check_dev(name: str, t: torch.Tensor, dev):
    """A pointer handed to a kernel must live on the launch's device (a CPU or other-GPU tensor
    would be a device fault or a write to the wrong memory, not a Python error)."""
    if t.device != dev:
        raise ValueError(f"{name} must be on {dev}, got {t.device}")


# ----------------------------------------------------------------------------------------------
# Gilbert permutation
# ----------------------------------------------------------------------------------------------
def gilbert_perm(width: int, height: int, depth: int) -> np.ndarray:
    """perm[g] = x + W*(y + H*z) of the g-th Gilbert point (vb_gilbert3d_perm, host C++)."""
    n = width * height * depth
    out = np.empty(n, dtype=np.int32)
    check(_lib.load().vb_gilbert3d_perm(width, height, depth, out.ctypes.data), "vb_gilbert3d_perm")
    return out


def sequence_rows(width: int, height: int, depth: int, text_length: int) -> np.ndarray:
    """Reordered position -> caller row: [video[perm] (+text offset), text] (CogVideoX puts the
    text tail last, cogvideo_blocksparseattn.py:141-154; Wan has text_length 0)."""
    perm = gilbert_perm(width, height, depth).astype(np.int64) + text_length
    return np.concatenate([perm, np.arange(text_length)]).astype(np.int32)


# ----------------------------------------------------------------------------------------------
# attention forward
# ----------------------------------------------------------------------------------------------
def attention_fwd(q: torch.Tensor, k: Optional[torch.Tensor], v: Optional[torch.Tensor], *,
                  block_mask: Optional[torch.Tensor] = None, q_rows: Optional[torch.Tensor] = None,
                  kv_rows: Optional[torch.Tensor] = None, kp: Optional[torch.Tensor] = None,
                  vp: Optional[torch.Tensor] = None, kp_log_bias: float = 0.0, use_main: bool = True,
                  scale: Optional[float] = None, need_lse: bool = False,
                  out: Optional[torch.Tensor] = None, heavy_rows: int = 0, order: bool = False,
                  q_lengths: Optional[torch.Tensor] = None, order_window: int = 0,
                  q_order_out: Optional[torch.Tensor] = None, persistent: bool = False,
                  out_layout: str = "bhld"):
    """vb_attn_fwd: softmax over (block-masked keys of k/v) ∪ (pooled keys kp/vp + bias).
    q,k,v [B,H,L,D]; block_mask [B,H,ceil(Lq/128),ceil(Lk/128)] bool/uint8; rows int32.
    ``order``: dispatch each XCD's q-blocks longest first (scheduling only; ``q_lengths`` [B,H,nbq]
    int32 kept blocks per mask row from mask_predict(rows_kept=...), else counted on the device;
    ``order_window`` > 0 re-orders only the last that many q-blocks of each XCD's range;
    ``q_order_out``: int32 [B*H*ceil(Lq/128)] to receive the dispatch permutation, for tests).
    ``persistent``: a resident-sized launch whose workgroups pull q-blocks from per-XCD queues
    (work_queue(); scheduling only, the same outputs). While the current stream is being captured into
    a graph and has no queue yet (no eager persistent call was made on it before the capture), the
    call launches the one-workgroup-per-q-block form instead and creates no queue: the same bits.
    ``out_layout``: the memory order of the output allocated here: "bhld" (contiguous) or "blhd" (the
    [B,H,Lq,D] view of [B,Lq,H,D] memory, the projections' layout; the same values, stored through
    other strides). ``out``: a caller's [B,H,Lq,D] buffer instead, of any layout with unit d-stride,
    the other strides multiples of 8 elements and a 16-byte aligned base; it is written in place.
    Returns out [B,H,Lq,D] (and lse fp32 [B,H,Lq] when need_lse)."""
    io_layout_code("out_layout", out_layout)
    dev = _require_gpu(q, k, v, block_mask, q_rows, kv_rows, kp, vp, q_lengths, q_order_out)
    q = _aligned_bhld(q)
    B, H, Lq, D = q.shape
    if use_main:
        k, v = _aligned_bhld(k), _aligned_bhld(v)
        Lk = k.shape[2]
    else:
        Lk = 0
    if kp is not None:
        kp, vp = _aligned_bhld(kp), _aligned_bhld(vp)
    if out is None:
        out = _empty_bhld(B, H, Lq, D, dev, q.dtype, out_layout)
    lse = torch.empty(B, H, Lq, device=dev, dtype=torch.float32) if need_lse else None
    a = AttnArgs()
    a.q = q.data_ptr()
    a.q_stride = _s3(q)
    if use_main:
        a.k, a.v = k.data_ptr(), v.data_ptr()
        a.k_stride, a.v_stride = _s3(k), _s3(v)
    a.q_rows, a.kv_rows = _ptr(q_rows), _ptr(kv_rows)
    a.use_main = 1 if use_main else 0
    if block_mask is not None:
        if block_mask.dtype == torch.bool:
            block_mask = block_mask.view(torch.uint8)
        nbq, nbk = (Lq + BLOCK - 1) // BLOCK, (Lk + BLOCK - 1) // BLOCK
        if block_mask.shape[2] < nbq or block_mask.shape[3] < nbk:
            raise ValueError(f"block_mask {tuple(block_mask.shape)} too small for {nbq}x{nbk} blocks")
        if block_mask.stride(3) != 1:
            block_mask = block_mask.contiguous()
        a.block_mask = block_mask.data_ptr()
        a.mask_stride = (ctypes.c_int64 * 3)(block_mask.stride(0), block_mask.stride(1),
                                             block_mask.stride(2))
    if kp is not None:
        a.kp, a.vp = kp.data_ptr(), vp.data_ptr()
        a.kp_stride, a.vp_stride = _s3(kp), _s3(vp)
        a.Lkp = kp.shape[2]
        a.kp_log_bias = float(kp_log_bias)
    a.out = out.data_ptr()
    a.out_stride = _s3(out)
    a.lse = _ptr(lse)
    a.B, a.H, a.Lq, a.Lk, a.D = B, H, Lq, Lk, D
    a.scale = float(scale) if scale else 0.0
    a.dtype = _dtype_code(q)
    a.heavy_rows = int(heavy_rows)
    a.work_queue = _work_queue_ptr(dev, persistent)
    if order and block_mask is not None and use_main:
        nbq = (Lq + BLOCK - 1) // BLOCK
        q_order = q_order_out if q_order_out is not None else torch.empty(B * H * nbq, device=dev, dtype=torch.int32)
        if q_order.dtype != torch.int32 or q_order.numel() < B * H * nbq or not q_order.is_contiguous() or q_order.device != dev:
            raise ValueError("attention_fwd: q_order_out must be a contiguous int32 tensor of B*H*ceil(Lq/128) on q's device")
        a.q_order = q_order.data_ptr()
        a.order_window = int(order_window)
        if q_lengths is not None:
            if q_lengths.dtype != torch.int32 or q_lengths.numel() != B * H * nbq or not q_lengths.is_contiguous():
                raise ValueError("attention_fwd: q_lengths must be contiguous int32 [B,H,ceil(Lq/128)]")
            _check_dev("attention_fwd: q_lengths", q_lengths, dev)
            a.q_lengths = q_lengths.data_ptr()
    check(_lib.load().vb_attn_fwd(ctypes.byref(a), _stream(dev)), "vb_attn_fwd")
    return (out, lse) if need_lse else out


MASK_HEAD_MODES = {"per_head": 0, "shared_head0": 1}   # vb_mask_head_mode


def mask_head_mode_code(mode: str) -> int:
    if mode not in MASK_HEAD_MODES:
        raise ValueError(f"mask_head_mode must be one of {sorted(MASK_HEAD_MODES)}, got {mode!r}")
    return MASK_HEAD_MODES[mode]


def block_sparse_attn_fwd(q_unpad, k_unpad, v_unpad, cu_seqlens_q, cu_seqlens_k, head_mask_type,
                          streaming_info, base_blockmask, max_seqlen_q, max_seqlen_k,
                          p_dropout=0.0, deterministic=False, softmax_scale=None,
                          is_causal=False, exact_streaming=False, mask_head_mode="per_head"):
    """Forward of block_sparse_attn_func through vb_block_sparse_attn_fwd (varlen layout).
    Returns (out_unpad [total_q,H,D], softmax_lse fp32 [B,H,max_seqlen_q]). ``mask_head_mode``:
    how head_mask_type's ones address base_blockmask's heads ("per_head": renumbered 1..H, one
    mask per head; "shared_head0": read literally, every such head uses mask head 0)."""
    mode = mask_head_mode_code(mask_head_mode)
    dev = _require_gpu(q_unpad, k_unpad, v_unpad, cu_seqlens_q, cu_seqlens_k, base_blockmask)
    q_unpad, k_unpad, v_unpad = q_unpad.contiguous(), k_unpad.contiguous(), v_unpad.contiguous()
    B = cu_seqlens_q.numel() - 1
    H, D = q_unpad.shape[1], q_unpad.shape[2]
    nbq = (max_seqlen_q + BLOCK - 1) // BLOCK
    nbk = (max_seqlen_k + BLOCK - 1) // BLOCK
    mask = None
    if base_blockmask is not None:
        mask = base_blockmask[:, :, :nbq, :nbk]
        if mask.dtype == torch.bool:
            mask = mask.contiguous().view(torch.uint8)
        mask = mask.to(torch.uint8).contiguous()
    hmt = head_mask_type.to(device=dev, dtype=torch.int32).contiguous() if head_mask_type is not None else None
    out = torch.empty_like(q_unpad)
    lse = torch.empty(B, H, max_seqlen_q, device=dev, dtype=torch.float32)
    check(_lib.load().vb_block_sparse_attn_fwd(
        q_unpad.data_ptr(), k_unpad.data_ptr(), v_unpad.data_ptr(),
        cu_seqlens_q.to(torch.int32).contiguous().data_ptr(),
        cu_seqlens_k.to(torch.int32).contiguous().data_ptr(),
        _ptr(hmt), _ptr(streaming_info), _ptr(mask), B, H, D, int(max_seqlen_q),
        int(max_seqlen_k), float(p_dropout), int(bool(deterministic)),
        float(softmax_scale) if softmax_scale else 0.0, int(bool(is_causal)),
        int(bool(exact_streaming)), _dtype_code(q_unpad), out.data_ptr(), lse.data_ptr(),
        mode, _stream(dev)), "vb_block_sparse_attn_fwd")
    return out, lse


# ----------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------
def _mask_u8(block_mask, Lq, Lk):
    if block_mask is None:
        return None
    if block_mask.dtype == torch.bool:
        block_mask = block_mask.view(torch.uint8)
    nbq, nbk = (Lq + BLOCK - 1) // BLOCK, (Lk + BLOCK - 1) // BLOCK
    if block_mask.shape[2] < nbq or block_mask.shape[3] < nbk:
        raise ValueError(f"block_mask {tuple(block_mask.shape)} too small for {nbq}x{nbk} blocks")
    if block_mask.stride(3) != 1:
        block_mask = block_mask.contiguous()
    return block_mask


def attention_bwd(dout, q, k, v, out, lse, *, block_mask=None, q_rows=None, kv_rows=None,
                  kp=None, vp=None, out2=None, lse2=None, alpha=None, gap: int = 0,
                  scale: Optional[float] = None, heavy_rows: int = 0, dk_rows: Optional[int] = None,
                  kernel_select: int = 0, kernels_ran: Optional[list] = None,
                  workspace_bytes: Optional[list] = None, grad_layout: str = "bhld", grads=None):
    """vb_attn_bwd: gradients (dq, dk, dv) of the block-sparse attention, optionally of the
    adaptive two-branch form (kp/vp/out2/lse2/alpha/gap: alpha detached, pooled grads folded back
    through the mean pool). k/v hold keys in reordered order; dk/dv rows are written at
    kv_rows[g] (dk_rows = number of rows of dk/dv, default Lk). Returns bf16/fp16 tensors.
    ``kernel_select``: _lib.VB_BWD_SEL_* bits (0: the default kernels); ``kernels_ran`` (a list)
    receives the _lib.VB_BWD_RAN_* bits of the kernels the call launched; ``workspace_bytes`` (a
    list) the size vb_attn_bwd_workspace_size reported for the call (it holds psplit copies of the
    pooled-key partials, so tests read the pooled-key split from it).
    ``dout`` is read through its strides (a transposed view of [B,L,H*D] memory as it comes; copied
    only when its strides or base miss the 16-byte rule). ``grad_layout``: the memory order of dq, dk
    and dv, "bhld" (contiguous) or "blhd" (the [B,H,L,D] views of [B,L,H,D] memory). ``grads``: (dq,
    dk, dv) buffers of the caller instead, as ml_attention_bwd's."""
    return _attention_bwd(dout, q, k, v, out, lse, block_mask, q_rows, kv_rows, kp, vp, out2, lse2, alpha, gap,
                          scale, heavy_rows, dk_rows, kernel_select, kernels_ran, workspace_bytes, None,
                          grad_layout, grads)


def attention_bwd_joint(dout, q, k, v, out, lse, *, block_mask, q_rows, kv_rows, kp, vp, gap: int,
                        kp_log_bias: float, scale: Optional[float] = None, heavy_rows: int = 0,
                        dk_rows: Optional[int] = None, kernel_select: int = 0,
                        kernels_ran: Optional[list] = None, workspace_bytes: Optional[list] = None,
                        grad_layout: str = "bhld", grads=None):
    """vb_attn_bwd_joint: the exact gradients (dq, dk, dv) of the one softmax attention_fwd evaluates
    with kp/vp/kp_log_bias: ``out`` and ``lse`` are that call's (need_lse=True, the same kp_log_bias),
    the block mask is a constant, and kp/vp are the mean pool of the reordered k/v over ``gap`` keys, so
    the pooled keys' gradients are folded back into dk/dv. Unlike attention_bwd's two-branch form no
    LSE or combine weight is held constant. The other arguments as attention_bwd."""
    if kp is None or vp is None:
        raise ValueError("attention_bwd_joint: the joint softmax needs the pooled keys kp and vp")
    return _attention_bwd(dout, q, k, v, out, lse, block_mask, q_rows, kv_rows, kp, vp, None, None, None, gap,
                          scale, heavy_rows, dk_rows, kernel_select, kernels_ran, workspace_bytes,
                          float(kp_log_bias), grad_layout, grads)


def _attention_bwd(dout, q, k, v, out, lse, block_mask, q_rows, kv_rows, kp, vp, out2, lse2, alpha, gap,
                   scale, heavy_rows, dk_rows, kernel_select, kernels_ran, workspace_bytes, joint_bias,
                   grad_layout="bhld", grads=None):
    """attention_bwd (``joint_bias`` None) and attention_bwd_joint (the pooled keys' logit bias)."""
    io_layout_code("grad_layout", grad_layout)
    dev = _require_gpu(dout, q, k, v, out, lse, block_mask, q_rows, kv_rows, kp, vp, out2, lse2,
                       alpha)
    q, k, v, out, dout = (_aligned_bhld(t) for t in (q, k, v, out, dout))
    B, H, Lq, D = q.shape
    Lk = k.shape[2]
    nrows = Lk if dk_rows is None else int(dk_rows)
    if grads is None:
        dq = _empty_bhld(B, H, Lq, D, dev, q.dtype, grad_layout)
        dk = _empty_bhld(B, H, nrows, D, dev, q.dtype, grad_layout)
        dv = _empty_bhld(B, H, nrows, D, dev, q.dtype, grad_layout)
    else:
        dq, dk, dv = grads
        for name, t, n in (("dq", dq, Lq), ("dk", dk, nrows), ("dv", dv, nrows)):
            _check_dev(f"attention_bwd: grads {name}", t, dev)
            if tuple(t.shape) != (B, H, n, D) or t.dtype != q.dtype:
                raise ValueError(f"attention_bwd: grads {name} must be [{B},{H},{n},{D}] {q.dtype}, got "
                                 f"{tuple(t.shape)} {t.dtype}")
    a = BwdArgs()
    a.q, a.q_stride = q.data_ptr(), _s3(q)
    a.k, a.v, a.k_stride, a.v_stride = k.data_ptr(), v.data_ptr(), _s3(k), _s3(v)
    a.q_rows, a.kv_rows = _ptr(q_rows), _ptr(kv_rows)
    m = _mask_u8(block_mask, Lq, Lk)
    if m is not None:
        a.block_mask = m.data_ptr()
        a.mask_stride = (ctypes.c_int64 * 3)(m.stride(0), m.stride(1), m.stride(2))
    a.out, a.out_stride = out.data_ptr(), _s3(out)
    lse = lse.float().contiguous()
    a.lse = lse.data_ptr()
    if kp is not None:
        kp, vp = _aligned_bhld(kp), _aligned_bhld(vp)
        a.kp, a.vp, a.kp_stride, a.vp_stride = kp.data_ptr(), vp.data_ptr(), _s3(kp), _s3(vp)
        a.Lkp = kp.shape[2]
        if joint_bias is None:
            out2 = _aligned_bhld(out2)
            lse2 = lse2.float().contiguous()
            alpha = alpha.float().contiguous()
            a.out2, a.out2_stride = out2.data_ptr(), _s3(out2)
            a.lse2, a.alpha = lse2.data_ptr(), alpha.data_ptr()
        a.pool_gap = int(gap)
    a.dout, a.dout_stride = dout.data_ptr(), _s3(dout)
    a.dq, a.dq_stride = dq.data_ptr(), _s3(dq)
    a.dk, a.dv, a.dk_stride, a.dv_stride = dk.data_ptr(), dv.data_ptr(), _s3(dk), _s3(dv)
    a.B, a.H, a.Lq, a.Lk, a.D = B, H, Lq, Lk, D
    a.scale = float(scale) if scale else 0.0
    a.dtype = _dtype_code(q)
    a.heavy_rows = int(heavy_rows)
    a.kernel_select = int(kernel_select)
    ran = ctypes.c_int32(0)
    a.kernels_ran = ctypes.pointer(ran)
    lib = _lib.load()
    nbytes = int(lib.vb_attn_bwd_workspace_size(ctypes.byref(a)))
    if workspace_bytes is not None:
        workspace_bytes.append(nbytes)
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    if joint_bias is None:
        check(lib.vb_attn_bwd(ctypes.byref(a), _stream(dev)), "vb_attn_bwd")
    else:
        check(lib.vb_attn_bwd_joint(ctypes.byref(a), joint_bias, _stream(dev)), "vb_attn_bwd_joint")
    if kernels_ran is not None:
        kernels_ran.append(ran.value)
    return dq, dk, dv


def block_sparse_attn_bwd(dout, q_unpad, k_unpad, v_unpad, out_unpad, softmax_lse, cu_seqlens_q,
                          cu_seqlens_k, head_mask_type, streaming_info, base_blockmask,
                          max_seqlen_q, max_seqlen_k, p_dropout=0.0, softmax_scale=None,
                          is_causal=False, exact_streaming=False, deterministic=True,
                          mask_head_mode="per_head"):
    """Backward of block_sparse_attn_func (vb_block_sparse_attn_bwd, varlen layout).
    Returns (dq, dk, dv) [total, H, D]. ``mask_head_mode`` as block_sparse_attn_fwd."""
    mode = mask_head_mode_code(mask_head_mode)
    dev = _require_gpu(dout, q_unpad, k_unpad, v_unpad, out_unpad, softmax_lse, base_blockmask)
    dout, q_unpad, k_unpad, v_unpad, out_unpad = (t.contiguous() for t in
                                                  (dout, q_unpad, k_unpad, v_unpad, out_unpad))
    B = cu_seqlens_q.numel() - 1
    H, D = q_unpad.shape[1], q_unpad.shape[2]
    nbq = (max_seqlen_q + BLOCK - 1) // BLOCK
    nbk = (max_seqlen_k + BLOCK - 1) // BLOCK
    mask = None
    if base_blockmask is not None:
        mask = base_blockmask[:, :, :nbq, :nbk]
        if mask.dtype == torch.bool:
            mask = mask.contiguous().view(torch.uint8)
        mask = mask.to(torch.uint8).contiguous()
    hmt = head_mask_type.to(device=dev, dtype=torch.int32).contiguous() if head_mask_type is not None else None
    cu_q = cu_seqlens_q.to(torch.int32).contiguous()
    cu_k = cu_seqlens_k.to(torch.int32).contiguous()
    lse = softmax_lse.float().contiguous()
    dq, dk, dv = torch.empty_like(q_unpad), torch.empty_like(k_unpad), torch.empty_like(v_unpad)
    lib = _lib.load()
    nbytes = int(lib.vb_block_sparse_attn_bwd_workspace_size(B, H, int(max_seqlen_q)))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    check(lib.vb_block_sparse_attn_bwd(
        dout.data_ptr(), q_unpad.data_ptr(), k_unpad.data_ptr(), v_unpad.data_ptr(),
        out_unpad.data_ptr(), lse.data_ptr(), cu_q.data_ptr(), cu_k.data_ptr(), _ptr(hmt),
        _ptr(streaming_info), _ptr(mask), B, H, D, int(max_seqlen_q), int(max_seqlen_k),
        float(p_dropout), float(softmax_scale) if softmax_scale else 0.0, int(bool(is_causal)),
        int(bool(exact_streaming)), int(bool(deterministic)), _dtype_code(q_unpad),
        dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), nbytes, mode, _stream(dev)),
        "vb_block_sparse_attn_bwd")
    return dq, dk, dv


# ----------------------------------------------------------------------------------------------
# mask predictor, energy rule, pooling, combine
# ----------------------------------------------------------------------------------------------
RULE_MODES = {"energy": _lib.VB_RULE_ENERGY, "topk": _lib.VB_RULE_TOPK}


@dataclasses.dataclass
class MaskRule:
    """vb_mask_rule: the mask rule of a mask_predict / block_mask_rule call.

    mode "energy": ``min_keep``, ``max_keep`` (kept-block counts) and ``energy_threshold`` each an
    int / float, an int32 / float32 device tensor [B,H] (one value per head), or None (the call's
    own scalar argument). mode "topk": ``init_k`` is the starting count k0, an int in [1, nc] or an
    int32 device tensor [B,H]; ``grow_below`` / ``shrink_below`` are the energy fractions (0 = the
    reference's 0.6 / 0.9) below which a row's budget triples / shrinks to k/3*2. Values in device
    tensors are clamped to [1, nc] by the kernel (they cannot be checked without a sync)."""
    mode: str = "energy"
    init_k: Union[int, torch.Tensor, None] = None
    min_keep: Union[int, torch.Tensor, None] = None
    max_keep: Union[int, torch.Tensor, None] = None
    energy_threshold: Union[float, torch.Tensor, None] = None
    grow_below: float = 0.0
    shrink_below: float = 0.0


def _rule_args(rule, B, H, dev, energy_threshold, min_keep, max_keep):
    """(ctypes MaskRule, tensors to keep alive, energy_threshold, min_keep, max_keep scalars)."""
    if isinstance(rule, dict):
        rule = MaskRule(**rule)
    if rule.mode not in RULE_MODES:
        raise ValueError(f"mask rule mode must be one of {list(RULE_MODES)}, got {rule.mode!r}")
    r = _lib.MaskRule()
    r.mode = RULE_MODES[rule.mode]
    keep = []

    def per_head(name, v, dtype):
        if v.numel() != B * H or tuple(v.shape) != (B, H):
            raise ValueError(f"mask rule: {name} must be a [B,H] = [{B},{H}] tensor, got {tuple(v.shape)}")
        _check_dev(f"mask rule: {name}", v, dev)
        v = v.to(dtype).contiguous()
        keep.append(v)
        return v.data_ptr()

    if rule.mode == "topk":
        if rule.init_k is None:
            raise ValueError("mask rule: mode 'topk' needs init_k")
        if isinstance(rule.init_k, torch.Tensor):
            r.init_k_bh = per_head("init_k", rule.init_k, torch.int32)
        else:
            r.init_k = int(rule.init_k)
        r.grow_below, r.shrink_below = float(rule.grow_below), float(rule.shrink_below)
    else:
        if isinstance(rule.min_keep, torch.Tensor):
            r.min_keep = per_head("min_keep", rule.min_keep, torch.int32)
        elif rule.min_keep is not None:
            min_keep = rule.min_keep
        if isinstance(rule.max_keep, torch.Tensor):
            r.max_keep = per_head("max_keep", rule.max_keep, torch.int32)
        elif rule.max_keep is not None:
            max_keep = rule.max_keep
        if isinstance(rule.energy_threshold, torch.Tensor):
            r.energy_threshold = per_head("energy_threshold", rule.energy_threshold, torch.float32)
        elif rule.energy_threshold is not None:
            energy_threshold = rule.energy_threshold
    return r, keep, float(energy_threshold), int(min_keep), int(max_keep)


def mask_predict(q, k, q_off=None, k_off=None, *, rows=None, energy_threshold=0.95, min_keep=1,
                 max_keep=1, force_tail=0, scale=None, mask_count=None, want_mask=True,
                 staged_event=None, rand=None, philox=None, pool=None, pyr=None, level=None,
                 rows_kept=None, long_rows=False, num_keep=None, rule=None):
    """vb_mask_predict. q,k [B,H,L,D]; q_off/k_off int32 [B,H,num_keep]. Returns (po, mask) with
    po [B,H,nb,nb] in q.dtype and mask uint8 [B,H,nb,nb] (None with want_mask=False: the scores
    only, no energy rule). ``staged_event`` (a torch.cuda.Event) is recorded once the sampled
    rows are staged, before the score kernel: work waiting on it overlaps the score kernel.

    ``rand=(rand_q, rand_k)``: the fp32 uniforms [B,H,1,block] of random_sample_tokens instead of
    q_off/k_off; the topk offsets are drawn inside the sampling launch.
    ``philox=(seed, offset)`` (from claim_rand_draws): those two draws generated inside the
    sampling launch too, equal to the values torch.rand would return at that generator state.
    ``pool=(v, gap, outs)``: the pooled K/V pass (vb_pool_kv of k, v through ``rows``) run by extra
    workgroups of the score kernel's launch on the current stream; ``outs`` = pool_kv_outputs(k,
    gap, reordered) receives kp, vp[, k_r, v_r].
    ``pyr=(v, outs)``: the multi-level KV pyramid pass (vb_kv_pyramid of k, v through ``rows``)
    run the same way; ``outs`` = kv_pyramid_outputs(k). Excludes ``pool``.
    ``level=mask_ratios``: the returned mask is the multi-level rank-band mask (level_mask's rule
    on the scores, computed by the score kernel's epilogue) instead of the energy mask.
    ``rows_kept``: int32 [B,H,nb] receiving the energy rule's kept-block count per mask row.
    ``long_rows``: call vb_mask_predict_long (up to MAX_BLOCKS_LONG = 1024 blocks, L <= 131072; the
    same outputs) instead of vb_mask_predict (up to MAX_BLOCKS = 320 blocks, L <= 40960).
    ``num_keep``: sampled tokens per 128-token block, one of NUM_KEEP_VALUES = (16, 32, 64): a quarter
    / four times the score work of the default 32 (the reference's value). With ``rand=`` or
    ``philox=`` it is the width of the offsets drawn (default 32; the draws stay [B,H,1,block]);
    with given offsets the width is read from q_off.shape[-1], which k_off and an explicit
    ``num_keep`` must match (ValueError otherwise). The library refuses other widths
    (VB_ERR_UNSUPPORTED).
    ``rule``: a MaskRule (or a dict of its fields): the call goes to vb_mask_predict_rule, whose
    epilogue applies that rule (per-head energy bounds, or the top-k mode) instead of the scalar
    energy rule; any nb up to MAX_BLOCKS_LONG, ``long_rows`` is not needed. None: the calls made
    without it."""
    try:
        return _mask_predict(q, k, q_off, k_off, rows=rows, energy_threshold=energy_threshold,
                             min_keep=min_keep, max_keep=max_keep, force_tail=force_tail, scale=scale,
                             mask_count=mask_count, want_mask=want_mask, staged_event=staged_event,
                             rand=rand, philox=philox, pool=pool, pyr=pyr, level=level,
                             rows_kept=rows_kept, long_rows=long_rows, num_keep=num_keep, rule=rule)
    except Exception as e:
        # the claimed draws go back to the generator only when nothing was launched: a Python-side
        # error (validation, or a host-side VBladeError such as the library failing to load, code
        # None), or the library refusing the call (VB_ERR_INVALID / _UNSUPPORTED, returned before
        # any launch). After a VB_ERR_LAUNCH the sampling launch may already have consumed them, and
        # rewinding would make the next torch.rand repeat those Philox values.
        launched = isinstance(e, _lib.VBladeError) and e.code not in (None, _lib.VB_ERR_INVALID,
                                                                      _lib.VB_ERR_UNSUPPORTED)
        if philox is not None and not launched:
            release_rand_draws(q.device, philox)
        raise


def _offset_width(q_off, k_off, num_keep, drawn: bool) -> int:
    """The sampling density of a mask_predict call: ``num_keep`` (default 32) when the offsets are
    drawn in the launch, else the given offsets' common width. Which widths exist is the library's
    decision (NUM_KEEP_VALUES; VB_ERR_UNSUPPORTED otherwise)."""
    if drawn:
        keep = 32 if num_keep is None else int(num_keep)
        if keep <= 0:
            raise ValueError(f"mask_predict: num_keep must be one of {NUM_KEEP_VALUES}, got {num_keep}")
        return keep
    if q_off is None or k_off is None:
        raise ValueError("mask_predict: give q_off and k_off, or rand= or philox=")
    if q_off.shape[-1] != k_off.shape[-1]:
        raise ValueError(f"mask_predict: q_off and k_off must have the same width, got "
                         f"{q_off.shape[-1]} and {k_off.shape[-1]}")
    if num_keep is not None and int(num_keep) != q_off.shape[-1]:
        raise ValueError(f"mask_predict: the offsets are {q_off.shape[-1]} wide, num_keep={num_keep}")
    return int(q_off.shape[-1])


def _mask_predict(q, k, q_off, k_off, *, rows, energy_threshold, min_keep, max_keep, force_tail,
                  scale, mask_count, want_mask, staged_event, rand, philox, pool, pyr, level, rows_kept,
                  long_rows=False, num_keep=None, rule=None):
    keep = _offset_width(q_off, k_off, num_keep, drawn=rand is not None or philox is not None)
    if k.shape != q.shape:
        raise ValueError(f"mask_predict: k and v must have q's shape {tuple(q.shape)}, "
                         f"got k {tuple(k.shape)}")
    dev = _require_gpu(q, k, q_off, k_off, rows, rows_kept)
    q, k = _aligned_bhld(q), _aligned_bhld(k)
    B, H, L, D = q.shape
    nb = (L + BLOCK - 1) // BLOCK
    if rows_kept is not None and (level is not None or not want_mask):
        raise ValueError("mask_predict: rows_kept is written by the energy rule only (not with level= "
                         "or want_mask=False)")
    po = torch.empty(B, H, nb, nb, device=dev, dtype=q.dtype)
    mask = torch.empty(B, H, nb, nb, device=dev, dtype=torch.uint8) if want_mask else None
    if rand is not None and philox is not None:
        raise ValueError("mask_predict: rand and philox are exclusive")
    if rand is not None or philox is not None:
        if rand is not None:
            rand_q, rand_k = (r.float().contiguous() for r in rand)
        q_off = torch.empty(B, H, keep, device=dev, dtype=torch.int32)
        k_off = torch.empty(B, H, keep, device=dev, dtype=torch.int32)
    q_off = q_off.to(torch.int32).contiguous()
    k_off = k_off.to(torch.int32).contiguous()
    rule_c = None
    if rule is not None:
        if level is not None:
            raise ValueError("mask_predict: rule and level are exclusive")
        rule_c, rule_keep, energy_threshold, min_keep, max_keep = _rule_args(
            rule, B, H, dev, energy_threshold, min_keep, max_keep)
    a = PredictArgs()
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_stride, a.k_stride = _s3(q), _s3(k)
    a.rows, a.q_off, a.k_off = _ptr(rows), q_off.data_ptr(), k_off.data_ptr()
    a.B, a.H, a.L, a.D, a.block, a.num_keep = B, H, L, D, BLOCK, q_off.shape[-1]
    a.scale = float(scale) if scale else 0.0
    a.energy_threshold = float(energy_threshold)
    a.min_keep, a.max_keep, a.force_tail = int(min_keep), int(max_keep), int(force_tail)
    a.po, a.mask, a.mask_count = po.data_ptr(), _ptr(mask), _ptr(mask_count)
    a.dtype = _dtype_code(q)
    lib = _lib.load()
    nbytes = int(lib.vb_mask_predict_workspace_size(ctypes.byref(a)))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.staged_event = staged_event.cuda_event if staged_event is not None else None
    if rand is not None:
        if rand_q.shape[-1] != BLOCK or rand_q.numel() != B * H * BLOCK or rand_k.numel() != B * H * BLOCK:
            raise ValueError("mask_predict: rand draws must be [B,H,1,block]")
        a.rand_q, a.rand_k = rand_q.data_ptr(), rand_k.data_ptr()
    if philox is not None:
        a.philox, a.philox_seed, a.philox_offset = 1, int(philox[0]), int(philox[1])
    if pool is not None:
        v, gap, outs = pool
        v = _aligned_bhld(v)
        if v.shape != k.shape:
            raise ValueError(f"mask_predict: k and v must have q's shape {tuple(q.shape)}, "
                             f"got v {tuple(v.shape)}")
        if outs[0].shape != (B, H, (L + int(gap) - 1) // int(gap), D):
            raise ValueError("mask_predict: pool outputs must come from pool_kv_outputs(k, gap)")
        a.pool_v, a.pool_v_stride, a.pool_gap = v.data_ptr(), _s3(v), int(gap)
        a.pool_kp, a.pool_vp = outs[0].data_ptr(), outs[1].data_ptr()
        if len(outs) > 2:
            a.pool_k_r, a.pool_v_r = outs[2].data_ptr(), outs[3].data_ptr()
    if pyr is not None:
        if pool is not None:
            raise ValueError("mask_predict: pool and pyr are exclusive")
        v, outs = pyr
        v = _aligned_bhld(v)
        if v.shape != k.shape:
            raise ValueError(f"mask_predict: k and v must have q's shape {tuple(q.shape)}, "
                             f"got v {tuple(v.shape)}")
        if outs[0].shape != (B, H, kv_pyramid_rows(L), D) or outs[1].shape != outs[0].shape:
            raise ValueError("mask_predict: pyramid outputs must come from kv_pyramid_outputs(k)")
        a.pool_v, a.pool_v_stride = v.data_ptr(), _s3(v)
        a.pyr_k, a.pyr_v = outs[0].data_ptr(), outs[1].data_ptr()
    if level is not None:
        if mask is None:
            raise ValueError("mask_predict: level needs want_mask=True")
        vals, st, en = _level_bands(level)
        a.mask_level, a.level_bands = 1, len(vals)
        a.level_band_value, a.level_band_start, a.level_band_end = (
            vals.ctypes.data, st.ctypes.data, en.ctypes.data)
    if rows_kept is not None:
        if rows_kept.dtype != torch.int32 or rows_kept.numel() != B * H * nb or not rows_kept.is_contiguous():
            raise ValueError("mask_predict: rows_kept must be contiguous int32 [B,H,nb]")
        _check_dev("mask_predict: rows_kept", rows_kept, dev)
        a.mask_rows_kept = rows_kept.data_ptr()
    if rule_c is not None:
        check(lib.vb_mask_predict_rule(ctypes.byref(a), ctypes.byref(rule_c), _stream(dev)),
              "vb_mask_predict_rule")
    elif long_rows:
        check(lib.vb_mask_predict_long(ctypes.byref(a), _stream(dev)), "vb_mask_predict_long")
    else:
        check(lib.vb_mask_predict(ctypes.byref(a), _stream(dev)), "vb_mask_predict")
    return po, mask


# torch.rand's launch on ROCm (ATen/native/hip/DistributionTemplates.h, calc_execution_policy and
# distribution_elementwise_grid_stride_kernel): 256-thread blocks, grid = min(ceil(numel / 256),
# CUs * maxThreadsPerMultiProcessor / 256); thread i draws one hiprand_uniform4 per pass and element
# li = i + pass_stride * c takes component c. Element i is the x component of thread i exactly while
# numel <= CUs * maxThreadsPerMultiProcessor (every element has a thread of its own; 524288 on an
# unpartitioned MI355X, fewer on a partitioned device or a smaller GPU). Each call then advances the
# generator's Philox offset by 4.
RAND_ONE_PASS_NUMEL = 524288   # the MI355X value; rand_one_pass_numel(device) is the per-device bound
PHILOX_DRAWS = os.environ.get("VB_PHILOX_DRAWS", "1") != "0"   # off: the callers use torch.rand
_ONE_PASS = {}


def rand_one_pass_numel(device) -> int:
    """Largest torch.rand numel whose element i is the x of Philox subsequence i on ``device``."""
    if not torch.cuda.is_available():
        return 0
    dev = torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    n = _ONE_PASS.get(idx)
    if n is None:
        pr = torch.cuda.get_device_properties(idx)
        n = _ONE_PASS[idx] = int(pr.multi_processor_count) * int(pr.max_threads_per_multi_processor)
    return n


def claim_rand_draws(device, numel: int, draws: int = 2):
    """Reserve ``draws`` consecutive torch.rand(numel) calls on ``device``'s default generator for
    a kernel that generates them itself: returns (seed, offset) and advances the generator's offset
    as those calls would, or None when the draw is too large for one x-only pass on this device or
    the stream is being captured into a graph (then call torch.rand). mask_predict gives the draws
    back (release_rand_draws) when it raises before its launch."""
    if not PHILOX_DRAWS or numel > rand_one_pass_numel(device):
        return None
    # under HIP-graph capture torch.rand draws from a per-replay offset; a seed/offset read here
    # would be baked into the graph, so captured calls keep torch.rand
    if torch.cuda.is_current_stream_capturing():
        return None
    dev = torch.device(device)
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    seed, off = gen.initial_seed(), gen.get_offset()
    gen.set_offset(off + 4 * draws)
    return seed, off


def release_rand_draws(device, philox, draws: int = 2):
    """Undo claim_rand_draws when the launch it was made for did not run: the generator's offset
    goes back to the claimed one if nothing has drawn from it since."""
    dev = torch.device(device)
    gen = torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()]
    if gen.initial_seed() == philox[0] and gen.get_offset() == philox[1] + 4 * draws:
        gen.set_offset(philox[1])


def sample_offsets(rand_q, rand_k, keep: int = 32):
    """vb_sample_offsets: topk(keep) indices (descending value, ties lower index first) of each
    row of the uniform draws rand_q/rand_k [..., n] -> int32 [..., keep] (q, k)."""
    dev = _require_gpu(rand_q, rand_k)
    rand_q, rand_k = rand_q.float().contiguous(), rand_k.float().contiguous()
    n = rand_q.shape[-1]
    rows = rand_q.numel() // n
    shape = tuple(rand_q.shape[:-1]) + (keep,)
    oq = torch.empty(shape, device=dev, dtype=torch.int32)
    ok = torch.empty(shape, device=dev, dtype=torch.int32)
    check(_lib.load().vb_sample_offsets(rand_q.data_ptr(), rand_k.data_ptr(), rows, n, keep,
                                        oq.data_ptr(), ok.data_ptr(), _stream(dev)),
          "vb_sample_offsets")
    return oq, ok


def energy_mask(po, *, energy_threshold=0.95, min_keep=1, max_keep=1, force_tail=0, mask_count=None):
    """vb_energy_mask on scores po [B,H,nr,nc] (bf16/fp16) -> uint8 mask."""
    dev = _require_gpu(po)
    po = po.contiguous()
    B, H, nr, nc = po.shape
    mask = torch.empty(B, H, nr, nc, device=dev, dtype=torch.uint8)
    check(_lib.load().vb_energy_mask(po.data_ptr(), B, H, nr, nc, float(energy_threshold),
                                     int(min_keep), int(max_keep), int(force_tail),
                                     _dtype_code(po), mask.data_ptr(), _ptr(mask_count),
                                     _stream(dev)), "vb_energy_mask")
    return mask


def block_mask_rule(po, rule=None, *, energy_threshold=0.95, min_keep=1, max_keep=1, force_tail=0,
                    mask_count=None, rows_kept=None):
    """vb_block_mask_rule: a MaskRule (or a dict of its fields; None = the scalar energy rule) alone
    on scores po [B,H,nr,nc] (bf16/fp16, nc <= 1024) -> uint8 mask. ``rows_kept`` (contiguous int32
    [B,H,nr]) receives the kept blocks per mask row, ``mask_count`` an atomic add of their sum."""
    dev = _require_gpu(po, rows_kept, mask_count)
    po = po.contiguous()
    B, H, nr, nc = po.shape
    rule_c = None
    if rule is not None:
        rule_c, rule_keep, energy_threshold, min_keep, max_keep = _rule_args(
            rule, B, H, dev, energy_threshold, min_keep, max_keep)
    if rows_kept is not None and (rows_kept.dtype != torch.int32 or rows_kept.numel() != B * H * nr
                                  or not rows_kept.is_contiguous()):
        raise ValueError("block_mask_rule: rows_kept must be contiguous int32 [B,H,nr]")
    mask = torch.empty(B, H, nr, nc, device=dev, dtype=torch.uint8)
    check(_lib.load().vb_block_mask_rule(po.data_ptr(), B, H, nr, nc,
                                         ctypes.byref(rule_c) if rule_c is not None else None,
                                         float(energy_threshold), int(min_keep), int(max_keep),
                                         int(force_tail), _dtype_code(po), mask.data_ptr(),
                                         _ptr(mask_count), _ptr(rows_kept), _stream(dev)),
          "vb_block_mask_rule")
    return mask


# ----------------------------------------------------------------------------------------------
# head-adaptive retain budgets
# ----------------------------------------------------------------------------------------------
JUDGE_MAX_SAMPLES = _lib.VB_JUDGE_MAX_SAMPLES
BUDGET_ARITH = {"cog": 0, "wan": 1}   # attention.retain_counts' two arithmetics


def judge_rows(rows, L: int, dev) -> torch.Tensor:
    """The probe rows of judge_sparsity as a device int32 [S] tensor. A host-side ``rows`` (list,
    tuple or numpy array) is range-checked against [0, L) here; a device tensor cannot be checked
    without a synchronisation and is clamped to [0, L-1] by the kernel instead."""
    if isinstance(rows, torch.Tensor):
        if rows.dim() != 1:
            raise ValueError(f"judge_sparsity: rows must be one-dimensional, got {tuple(rows.shape)}")
        if rows.is_cuda:
            _check_dev("judge_sparsity: rows", rows, dev)
            return rows.to(torch.int32).contiguous()
        rows = rows.numpy()
    r = np.asarray(rows)
    if r.ndim != 1 or r.size == 0 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("judge_sparsity: rows must be a non-empty one-dimensional list of integers")
    if r.min() < 0 or r.max() >= L:
        raise ValueError(f"judge_sparsity: rows must lie in [0, {L}), got [{r.min()}, {r.max()}]")
    return torch.from_numpy(r.astype(np.int32)).to(dev)


def judge_sparsity(q, k, rows, *, key_stride: int = 3, top: float = 0.2, scale=None, want_rows: bool = False):
    """vb_judge_sparsity: the reference's judge_sparsity(q, k) on the device. q,k [B,H,L,D] (strided
    views are read in place); ``rows`` the S <= 64 sampled query rows (a device int32 tensor, or a
    host list / numpy array, which is range-checked), shared by every (b,h). Per sampled row: the
    softmax over every ``key_stride``-th key, and the mass of its top_n = int(n * top) largest
    entries (n = ceil(L / key_stride)); the result is the mean over the rows, fp32 [B,H]. With
    ``want_rows`` also the per-row masses, fp32 [B,H,S]."""
    if k.shape != q.shape or q.dim() != 4:
        raise ValueError(f"judge_sparsity: q and k must share a [B,H,L,D] shape, got {tuple(q.shape)} "
                         f"and {tuple(k.shape)}")
    dev = _require_gpu(q, k)
    B, H, L, D = q.shape
    key_stride = int(key_stride)
    if key_stride < 1:
        raise ValueError(f"judge_sparsity: key_stride must be >= 1, got {key_stride}")
    n = (L + key_stride - 1) // key_stride
    top_n = int(n * top)
    if not 1 <= top_n <= n:
        raise ValueError(f"judge_sparsity: int(n * top) = {top_n} must lie in [1, n = {n}]")
    rows = judge_rows(rows, L, dev)
    S = rows.numel()
    if not 1 <= S <= JUDGE_MAX_SAMPLES:
        raise ValueError(f"judge_sparsity: 1 to {JUDGE_MAX_SAMPLES} sampled rows, got {S}")
    a = _lib.JudgeArgs()
    a.B, a.H, a.L, a.D, a.S = B, H, L, D, S
    a.key_stride, a.top_n = key_stride, top_n
    a.scale = float(scale) if scale else 0.0
    a.dtype = _dtype_code(q)
    lib = _lib.load()
    nbytes = int(lib.vb_judge_sparsity_workspace_size(ctypes.byref(a)))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    q, k = _aligned_bhld(q), _aligned_bhld(k)
    sparsity = torch.empty(B, H, device=dev, dtype=torch.float32)
    row_mass = torch.empty(B, H, S, device=dev, dtype=torch.float32) if want_rows else None
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_stride, a.k_stride = _s3(q), _s3(k)
    a.rows = rows.data_ptr()
    a.sparsity, a.row_mass = sparsity.data_ptr(), _ptr(row_mass)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.vb_judge_sparsity(ctypes.byref(a), _stream(dev)), "vb_judge_sparsity")
    return (sparsity, row_mass) if want_rows else sparsity


def head_budget(sparsity, nb: int, base: float, clamp=(0.05, 0.9), variant: str = "cog", want_ratio: bool = False):
    """vb_head_budget: judge_sparsity's fp32 [B,H] -> kept-block counts int32 [B,H] (a MaskRule's
    ``max_keep``): ratio = clamp(base * sparsity / sparsity.mean(), *clamp) in float64, the mean over
    batch and heads together, and count = max(1, int(nb * ratio)) in ``variant``'s arithmetic
    (attention.retain_counts). With ``want_ratio`` also the ratios, fp32 [B,H]."""
    if variant not in BUDGET_ARITH:
        raise ValueError(f"head_budget: variant must be one of {list(BUDGET_ARITH)}, got {variant!r}")
    lo, hi = float(clamp[0]), float(clamp[1])
    if not lo <= hi:
        raise ValueError(f"head_budget: clamp needs lo <= hi, got ({lo}, {hi})")
    dev = _require_gpu(sparsity)
    if sparsity.dim() != 2 or sparsity.dtype != torch.float32:
        raise ValueError(f"head_budget: sparsity must be fp32 [B,H], got {sparsity.dtype} {tuple(sparsity.shape)}")
    sparsity = sparsity.contiguous()
    B, H = sparsity.shape
    keep = torch.empty(B, H, device=dev, dtype=torch.int32)
    ratio = torch.empty(B, H, device=dev, dtype=torch.float32) if want_ratio else None
    check(_lib.load().vb_head_budget(sparsity.data_ptr(), B, H, int(nb), float(base), lo, hi,
                                     BUDGET_ARITH[variant], keep.data_ptr(), _ptr(ratio), _stream(dev)),
          "vb_head_budget")
    return (keep, ratio) if want_ratio else keep


# ----------------------------------------------------------------------------------------------
# attention-recall probe
# ----------------------------------------------------------------------------------------------
RECALL_MAX_SAMPLES = _lib.VB_RECALL_MAX_SAMPLES


def recall_probe_pos(probe_pos, L: int, dev) -> torch.Tensor:
    """The probe positions of mask_recall as a device int32 [S] tensor. A host-side ``probe_pos``
    (list, tuple or numpy array) is range-checked against [0, L) here; a device tensor cannot be
    checked without a synchronisation and is clamped to [0, L-1] by the kernel instead."""
    if isinstance(probe_pos, torch.Tensor):
        if probe_pos.dim() != 1:
            raise ValueError(f"mask_recall: probe_pos must be one-dimensional, got {tuple(probe_pos.shape)}")
        if probe_pos.is_cuda:
            _check_dev("mask_recall: probe_pos", probe_pos, dev)
            return probe_pos.to(torch.int32).contiguous()
        probe_pos = probe_pos.numpy()
    r = np.asarray(probe_pos)
    if r.ndim != 1 or r.size == 0 or not np.issubdtype(r.dtype, np.integer):
        raise ValueError("mask_recall: probe_pos must be a non-empty one-dimensional list of integers")
    if r.min() < 0 or r.max() >= L:
        raise ValueError(f"mask_recall: probe_pos must lie in [0, {L}), got [{r.min()}, {r.max()}]")
    return torch.from_numpy(r.astype(np.int32)).to(dev)


def mask_recall(q, k, block_mask, probe_pos, *, rows=None, scale=None, want_rows: bool = False):
    """vb_mask_recall: the exact softmax mass ``block_mask`` keeps for S <= 64 probe queries per head,
    and the best mass a mask with as many blocks could have kept. q,k [B,H,L,D] (strided views are
    read in place); block_mask [B,H,nb,nb] uint8 or bool in reordered order (a head-stride-0 view is
    read as it is); ``probe_pos`` the REORDERED positions of the probe queries (a device int32
    tensor, or a host list / numpy array, which is range-checked), shared by every (b,h); ``rows``
    the reordered position -> caller row index the attention launch takes (None: identity). Returns
    (recall, oracle_recall), fp32 [B,H]: the means over the probes; with ``want_rows`` also
    (row_recall, row_oracle, row_kept), fp32 / fp32 / int32 [B,H,S]."""
    if k.shape != q.shape or q.dim() != 4:
        raise ValueError(f"mask_recall: q and k must share a [B,H,L,D] shape, got {tuple(q.shape)} "
                         f"and {tuple(k.shape)}")
    dev = _require_gpu(q, k, block_mask)
    B, H, L, D = q.shape
    nb = (L + BLOCK - 1) // BLOCK
    if block_mask.dim() != 4 or block_mask.shape[0] != B or block_mask.shape[1] != H:
        raise ValueError(f"mask_recall: block_mask must be [B,H,nb,nb] = [{B},{H},{nb},{nb}], "
                         f"got {tuple(block_mask.shape)}")
    if block_mask.dtype not in (torch.uint8, torch.bool):
        raise TypeError(f"mask_recall: block_mask must be uint8 or bool, got {block_mask.dtype}")
    m = _mask_u8(block_mask, L, L)
    probe_pos = recall_probe_pos(probe_pos, L, dev)
    S = probe_pos.numel()
    if not 1 <= S <= RECALL_MAX_SAMPLES:
        raise ValueError(f"mask_recall: 1 to {RECALL_MAX_SAMPLES} probe positions, got {S}")
    if rows is not None:
        _check_dev("mask_recall: rows", rows, dev)
        if rows.dtype != torch.int32 or rows.numel() != L:
            raise ValueError(f"mask_recall: rows must be int32 [{L}], got {rows.dtype} {tuple(rows.shape)}")
        rows = rows.contiguous()
    a = _lib.RecallArgs()
    a.B, a.H, a.L, a.D, a.S = B, H, L, D, S
    a.scale = float(scale) if scale else 0.0
    a.dtype = _dtype_code(q)
    lib = _lib.load()
    nbytes = int(lib.vb_mask_recall_workspace_size(ctypes.byref(a)))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    q, k = _aligned_bhld(q), _aligned_bhld(k)
    recall = torch.empty(B, H, device=dev, dtype=torch.float32)
    oracle = torch.empty(B, H, device=dev, dtype=torch.float32)
    row_recall = row_oracle = row_kept = None
    if want_rows:
        row_recall = torch.empty(B, H, S, device=dev, dtype=torch.float32)
        row_oracle = torch.empty(B, H, S, device=dev, dtype=torch.float32)
        row_kept = torch.empty(B, H, S, device=dev, dtype=torch.int32)
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_stride, a.k_stride = _s3(q), _s3(k)
    a.rows, a.probe_pos = _ptr(rows), probe_pos.data_ptr()
    a.block_mask = m.data_ptr()
    a.mask_stride = (ctypes.c_int64 * 3)(m.stride(0), m.stride(1), m.stride(2))
    a.recall, a.oracle_recall = recall.data_ptr(), oracle.data_ptr()
    a.row_recall, a.row_oracle, a.row_kept = _ptr(row_recall), _ptr(row_oracle), _ptr(row_kept)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.vb_mask_recall(ctypes.byref(a), _stream(dev)), "vb_mask_recall")
    return (recall, oracle, row_recall, row_oracle, row_kept) if want_rows else (recall, oracle)


# ----------------------------------------------------------------------------------------------
# output-fidelity probe
# ----------------------------------------------------------------------------------------------
FIDELITY_MAX_SAMPLES = _lib.VB_FIDELITY_MAX_SAMPLES
FIDELITY_CHUNK = _lib.VB_FIDELITY_CHUNK


def attn_fidelity(q, k, v, out, probe_rows, *, scale=None, want_rows: bool = False, want_ref: bool = False):
    """vb_attn_fidelity: the error of ``out`` against exact dense attention for S <= 64 probe queries
    per head. q, k, v, out [B,H,L,D] (strided views are read in place); ``probe_rows`` the CALLER rows
    of the probe queries, shared by every (b,h): a device int32 [S] tensor (clamped to [0, L-1] by the
    kernel) or a host list / numpy array, which is range-checked. Needs no mask and no order: whichever
    module or option produced ``out``. Returns (err, sig, peak), fp32 [B,H]: the squared error and the
    squared reference summed over the probe rows, and max |ref|; then (row_err, row_sig, row_lse), fp32
    [B,H,S], when ``want_rows``; then ref, fp32 [B,H,S,D], when ``want_ref``."""
    if q.dim() != 4 or k.shape != q.shape or v.shape != q.shape or out.shape != q.shape:
        raise ValueError(f"attn_fidelity: q, k, v and out must share a [B,H,L,D] shape, got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(v.shape)} and {tuple(out.shape)}")
    dev = _require_gpu(q, k, v, out)
    if not (q.dtype == k.dtype == v.dtype == out.dtype):
        raise TypeError(f"attn_fidelity: q, k, v and out must share a dtype, got {q.dtype}, {k.dtype}, "
                        f"{v.dtype} and {out.dtype}")
    B, H, L, D = q.shape
    if isinstance(probe_rows, torch.Tensor) and probe_rows.is_cuda:
        if probe_rows.dim() != 1:
            raise ValueError(f"attn_fidelity: probe_rows must be one-dimensional, got {tuple(probe_rows.shape)}")
        _check_dev("attn_fidelity: probe_rows", probe_rows, dev)
        probe_rows = probe_rows.to(torch.int32).contiguous()
    else:
        r = np.asarray(probe_rows.numpy() if isinstance(probe_rows, torch.Tensor) else probe_rows)
        if r.ndim != 1 or r.size == 0 or not np.issubdtype(r.dtype, np.integer):
            raise ValueError("attn_fidelity: probe_rows must be a non-empty one-dimensional list of integers")
        if r.min() < 0 or r.max() >= L:
            raise ValueError(f"attn_fidelity: probe_rows must lie in [0, {L}), got [{r.min()}, {r.max()}]")
        probe_rows = torch.from_numpy(r.astype(np.int32)).to(dev)
    S = probe_rows.numel()
    if not 1 <= S <= FIDELITY_MAX_SAMPLES:
        raise ValueError(f"attn_fidelity: 1 to {FIDELITY_MAX_SAMPLES} probe rows, got {S}")
    a = _lib.FidelityArgs()
    a.B, a.H, a.L, a.D, a.S = B, H, L, D, S
    a.scale = float(scale) if scale else 0.0
    a.dtype = _dtype_code(q)
    lib = _lib.load()
    nbytes = int(lib.vb_attn_fidelity_workspace_size(ctypes.byref(a)))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    q, k, v, out = _aligned_bhld(q), _aligned_bhld(k), _aligned_bhld(v), _aligned_bhld(out)
    err = torch.empty(B, H, device=dev, dtype=torch.float32)
    sig = torch.empty(B, H, device=dev, dtype=torch.float32)
    peak = torch.empty(B, H, device=dev, dtype=torch.float32)
    row_err = row_sig = row_lse = ref = None
    if want_rows:
        row_err = torch.empty(B, H, S, device=dev, dtype=torch.float32)
        row_sig = torch.empty(B, H, S, device=dev, dtype=torch.float32)
        row_lse = torch.empty(B, H, S, device=dev, dtype=torch.float32)
    if want_ref:
        ref = torch.empty(B, H, S, D, device=dev, dtype=torch.float32)
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.q_stride, a.k_stride, a.v_stride, a.out_stride = _s3(q), _s3(k), _s3(v), _s3(out)
    a.probe_rows = probe_rows.data_ptr()
    a.err, a.sig, a.peak = err.data_ptr(), sig.data_ptr(), peak.data_ptr()
    a.row_err, a.row_sig, a.row_lse, a.ref = _ptr(row_err), _ptr(row_sig), _ptr(row_lse), _ptr(ref)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.vb_attn_fidelity(ctypes.byref(a), _stream(dev)), "vb_attn_fidelity")
    res = (err, sig, peak)
    if want_rows:
        res += (row_err, row_sig, row_lse)
    if want_ref:
        res += (ref,)
    return res


def fidelity_snr_db(err: torch.Tensor, sig: torch.Tensor) -> torch.Tensor:
    """10 log10(sig / err) per head, +inf where err == 0."""
    e, s = err.double(), sig.double()
    snr = 10.0 * torch.log10(s / e)
    return torch.where(e == 0, torch.full_like(snr, float("inf")), snr)


# ----------------------------------------------------------------------------------------------
# mask predictor: the softmax-mass block score
# ----------------------------------------------------------------------------------------------
MASS_NUM_KEEP = 32   # the only sampling density vb_mask_scores_mass is built for


def mask_scores_mass(q, k, q_off, k_off, *, rows=None, scale=None, want_mass: bool = False):
    """vb_mask_scores_mass: the sampled softmax mass per (q-block, key-block) pair, row-normalised in
    q.dtype: the score mask_predict's max proxy stands in for, in the form block_mask_rule takes.
    q,k [B,H,L,D] (strided views are read in place); q_off/k_off int32 [B,H,32], the sampled offsets
    of every 128-token block (sample_offsets' outputs); ``rows`` the reordered position -> caller row
    index (None: identity). Returns po [B,H,nb,nb], or (po, mass) with ``want_mass``: the fp32 block
    masses before the normalisation, each row summing to 32."""
    if k.shape != q.shape or q.dim() != 4:
        raise ValueError(f"mask_scores_mass: q and k must share a [B,H,L,D] shape, got {tuple(q.shape)} "
                         f"and {tuple(k.shape)}")
    dev = _require_gpu(q, k, q_off, k_off, rows)
    B, H, L, D = q.shape
    for name, off in (("q_off", q_off), ("k_off", k_off)):
        if off.dim() != 3 or off.shape[0] != B or off.shape[1] != H:
            raise ValueError(f"mask_scores_mass: {name} must be [B,H,{MASS_NUM_KEEP}] = [{B},{H},{MASS_NUM_KEEP}], "
                             f"got {tuple(off.shape)}")
        if off.shape[-1] != MASS_NUM_KEEP:
            raise ValueError(f"mask_scores_mass: the mass score samples {MASS_NUM_KEEP} tokens per block only "
                             f"(16 and 64 are mask_predict's), {name} is {off.shape[-1]} wide")
    if rows is not None:
        if rows.dtype != torch.int32 or rows.numel() != L:
            raise ValueError(f"mask_scores_mass: rows must be int32 [{L}], got {rows.dtype} {tuple(rows.shape)}")
        rows = rows.contiguous()
    nb = (L + BLOCK - 1) // BLOCK
    q_off = q_off.to(torch.int32).contiguous()
    k_off = k_off.to(torch.int32).contiguous()
    q, k = _aligned_bhld(q), _aligned_bhld(k)
    a = _lib.MassScoresArgs()
    a.B, a.H, a.L, a.D, a.block, a.num_keep = B, H, L, D, BLOCK, MASS_NUM_KEEP
    a.scale = float(scale) if scale else 0.0
    a.dtype = _dtype_code(q)
    lib = _lib.load()
    nbytes = int(lib.vb_mask_scores_mass_workspace_size(ctypes.byref(a)))
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    po = torch.empty(B, H, nb, nb, device=dev, dtype=q.dtype)
    mass = torch.empty(B, H, nb, nb, device=dev, dtype=torch.float32) if want_mass else None
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_stride, a.k_stride = _s3(q), _s3(k)
    a.rows, a.q_off, a.k_off = _ptr(rows), q_off.data_ptr(), k_off.data_ptr()
    a.po, a.mass = po.data_ptr(), _ptr(mass)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.vb_mask_scores_mass(ctypes.byref(a), _stream(dev)), "vb_mask_scores_mass")
    return (po, mass) if want_mass else po


def pool_kv_outputs(k, gap: int, reordered: bool = False):
    """Allocate pool_kv's outputs (kp, vp[, k_r, v_r]) on the current stream. A caller that launches
    pool_kv on a side stream allocates them BEFORE enqueueing other work whose temporaries could
    otherwise be recycled into them while that work still runs."""
    B, H, L, D = k.shape
    Lp = (L + gap - 1) // gap
    kw = dict(device=k.device, dtype=k.dtype)
    outs = [torch.empty(B, H, Lp, D, **kw), torch.empty(B, H, Lp, D, **kw)]
    if reordered:
        outs += [torch.empty(B, H, L, D, **kw), torch.empty(B, H, L, D, **kw)]
    return tuple(outs)


def pool_kv(k, v, gap: int, rows=None, reordered: bool = False, stream=None, out=None):
    """vb_pool_kv: mean over `gap` consecutive reordered tokens (replicate pad) -> kp, vp; with
    reordered=True also returns the Gilbert-ordered contiguous copies (k_r, v_r) written in the
    same pass. ``stream`` (a torch.cuda.Stream) launches there instead of the current stream; the
    outputs are still allocated on the current stream, which must wait for ``stream`` before
    using them."""
    if v.shape != k.shape:
        raise ValueError(f"pool_kv: k and v must have the same shape, got {tuple(k.shape)} and "
                         f"{tuple(v.shape)}")
    if rows is not None and rows.numel() != k.shape[2]:
        raise ValueError(f"pool_kv: rows has {rows.numel()} entries for {k.shape[2]} keys")
    dev = _require_gpu(k, v, rows)
    k, v = _aligned_bhld(k), _aligned_bhld(v)
    if stream is not None:   # read (and written) on the side stream: no reuse before it is done
        for t in (k, v, rows) + tuple(out or ()):
            if t is not None:
                t.record_stream(stream)
    B, H, L, D = k.shape
    if out is None:
        out = pool_kv_outputs(k, gap, reordered)
    kp, vp = out[0], out[1]
    k_r, v_r = (out[2], out[3]) if reordered else (None, None)
    check(_lib.load().vb_pool_kv(k.data_ptr(), v.data_ptr(), ctypes.cast(_s3(k), ctypes.c_void_p),
                                 ctypes.cast(_s3(v), ctypes.c_void_p), _ptr(rows), B, H, L, D,
                                 int(gap), _dtype_code(k), kp.data_ptr(), vp.data_ptr(),
                                 _ptr(k_r), _ptr(v_r),
                                 stream.cuda_stream if stream is not None else _stream(dev)), "vb_pool_kv")
    if reordered:
        return kp, vp, k_r, v_r
    return kp, vp


def lse_combine(out1, lse1, out2, lse2, gap: float, *, out_layout: str = "bhld", out=None):
    """vb_lse_combine (reference-faithful eager rounding). Returns (out, alpha fp32 [B,H,L]).
    ``out_layout``: the memory order of the output allocated here ("bhld" contiguous, "blhd" the
    [B,H,L,D] view of [B,L,H,D] memory); ``out``: a caller's [B,H,L,D] buffer instead (unit d-stride,
    the other strides multiples of 8 elements, 16-byte aligned base, no overlap with the inputs). When
    out1, out2 or the output is not contiguous and D is 64 or 128 the call goes to
    vb_lse_combine_strided, which reads and writes through the strides: the same bits, no copies."""
    io_layout_code("out_layout", out_layout)
    dev = _require_gpu(out1, lse1, out2, lse2, out)
    B, H, L, D = out1.shape
    if out is not None and (tuple(out.shape) != (B, H, L, D) or out.dtype != out1.dtype):
        raise ValueError(f"lse_combine: out must be [{B},{H},{L},{D}] {out1.dtype}, got {tuple(out.shape)} {out.dtype}")
    if out is not None and out.data_ptr() in (out1.data_ptr(), out2.data_ptr()):
        raise ValueError("lse_combine: out may not overlap the inputs")
    lse1, lse2 = lse1.float().contiguous(), lse2.float().contiguous()
    alpha = torch.empty(B, H, L, device=dev, dtype=torch.float32)
    if D in (64, 128):
        out1, out2 = _aligned_bhld(out1), _aligned_bhld(out2)
        if out is None:
            out = _empty_bhld(B, H, L, D, dev, out1.dtype, out_layout)
        if not (out1.is_contiguous() and out2.is_contiguous() and out.is_contiguous()):
            cast = lambda t: ctypes.cast(_s3(t), ctypes.c_void_p)
            check(_lib.load().vb_lse_combine_strided(
                out1.data_ptr(), cast(out1), lse1.data_ptr(), out2.data_ptr(), cast(out2), lse2.data_ptr(),
                B, H, L, D, float(gap), _dtype_code(out1), out.data_ptr(), cast(out), alpha.data_ptr(),
                _stream(dev)), "vb_lse_combine_strided")
            return out, alpha
    elif out_layout != "bhld" or (out is not None and not out.is_contiguous()):
        raise ValueError(f"lse_combine: a strided output needs D = 64 or 128, got {D}")
    out1, out2 = out1.contiguous(), out2.contiguous()
    if out is None:
        out = torch.empty_like(out1)
    check(_lib.load().vb_lse_combine(out1.data_ptr(), lse1.data_ptr(), out2.data_ptr(),
                                     lse2.data_ptr(), B, H, L, D, float(gap), _dtype_code(out1),
                                     out.data_ptr(), alpha.data_ptr(), _stream(dev)),
          "vb_lse_combine")
    return out, alpha


# ----------------------------------------------------------------------------------------------
# q/k prologue: the processors' q/k norm + RoPE in one pass (vb_qk_prologue)
# ----------------------------------------------------------------------------------------------
QK_NORMS = {"none": _lib.VB_QK_NORM_NONE, "layer": _lib.VB_QK_NORM_LAYER_HEAD, "rms": _lib.VB_QK_NORM_RMS_ROW}
QK_ROPES = {"none": _lib.VB_QK_ROPE_NONE, "real": _lib.VB_QK_ROPE_REAL, "complex": _lib.VB_QK_ROPE_COMPLEX}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _qk_affine(name, t, n, x, dev):
    """A weight or bias of n values: the storage dtype or fp32, contiguous, 16-byte aligned."""
    if t is None:
        return None
    if t.dtype not in (x.dtype, torch.float32):
        raise TypeError(f"qk_prologue: {name} must be {x.dtype} or float32, got {t.dtype}")
    if t.numel() != n:
        raise ValueError(f"qk_prologue: {name} has {t.numel()} values, the norm takes {n}")
    _check_dev(f"qk_prologue: {name}", t, dev)
    t = t.detach().reshape(n).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _qk_table(name, t, shape, dev):
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"qk_prologue: {name} must be {tuple(shape)}, got {tuple(t.shape)}")
    t = t.detach().to(dev).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _qk_modes(q_proj, k_proj, heads, norm, rope, rope_start, cos, sin, freqs):
    """The checks qk_prologue and qk_prologue_bwd share: the per-tensor modes, the shape, and the RoPE
    tables made ready for the launch. Returns (norms, ropes, dev, B, L, W, D, table)."""
    norms, ropes = _pair(norm), _pair(rope)
    for m in norms:
        if m not in QK_NORMS:
            raise ValueError(f"qk_prologue: norm must be one of {sorted(QK_NORMS)}, got {m!r}")
    for m in ropes:
        if m not in QK_ROPES:
            raise ValueError(f"qk_prologue: rope must be one of {sorted(QK_ROPES)}, got {m!r}")
    W = q_proj.shape[-1] if q_proj.dim() == 3 else heads * q_proj.shape[-1]
    if q_proj.dim() not in (3, 4) or W % heads or (q_proj.dim() == 4 and q_proj.shape[2] != heads):
        raise ValueError(f"qk_prologue: expected [B,L,{heads}*D] or [B,L,{heads},D], got {tuple(q_proj.shape)}")
    dev = _require_gpu(q_proj, k_proj)
    if k_proj is not None and (k_proj.shape != q_proj.shape or k_proj.dtype != q_proj.dtype):
        raise ValueError("qk_prologue: k_proj must have q_proj's shape and dtype")
    B, L = q_proj.shape[:2]
    D = W // heads
    table = {}
    if "real" in ropes:
        if cos is None or sin is None:
            raise ValueError("qk_prologue: rope='real' needs cos and sin")
        if cos.dtype != torch.float32 or sin.dtype != torch.float32:
            raise TypeError("qk_prologue: cos and sin must be float32")
        if not 0 <= rope_start <= L:
            raise ValueError(f"qk_prologue: rope_start {rope_start} outside [0, {L}]")
        table["cos"] = _qk_table("cos", cos, (L - rope_start, D), dev)
        table["sin"] = _qk_table("sin", sin, (L - rope_start, D), dev)
        if rope_start == L:   # no row takes it, and an empty table has no address to hand over
            ropes = tuple("none" if m == "real" else m for m in ropes)
    if "complex" in ropes:
        if freqs is None or not freqs.is_complex() or freqs.dtype not in (torch.complex64, torch.complex128):
            raise TypeError("qk_prologue: rope='complex' needs freqs as a complex64 or complex128 tensor")
        if freqs.numel() != L * (D // 2) or freqs.shape[-1] != D // 2:
            raise ValueError(f"qk_prologue: freqs must hold [{L}, {D // 2}] values, got {tuple(freqs.shape)}")
        table["freqs"] = _qk_table("freqs", torch.view_as_real(freqs.reshape(L, D // 2)), (L, D // 2, 2), dev)

    return norms, ropes, dev, B, L, W, D, table


def qk_prologue(q_proj: torch.Tensor, k_proj: Optional[torch.Tensor] = None, *, heads: int,
                norm="none", q_weight=None, q_bias=None, q_eps: float = 1e-5,
                k_weight=None, k_bias=None, k_eps: Optional[float] = None,
                rope="none", rope_start: int = 0, cos=None, sin=None, freqs=None,
                inplace: bool = False):
    """vb_qk_prologue: the attention processors' q/k norm and RoPE in one pass over q and k.

    q_proj / k_proj: the projections' outputs, [B,L,heads*D] or [B,L,heads,D] (rows contiguous).
    ``norm``: "none", "layer" (LayerNorm over each head's D values; weight/bias of D values) or "rms"
    (RMSNorm over the heads*D row; weight of heads*D values); ``rope``: "none", "real" (cos/sin fp32
    [L-rope_start, D] on the rows from ``rope_start``) or "complex" (``freqs``: a complex64/128
    tensor of L*D/2 values, every row). A (q, k) pair gives each tensor its own mode, e.g.
    ``rope=("real", "none")`` for cross attention. Weights are the storage dtype or fp32.
    ``inplace`` overwrites the projections. Returns the [B,heads,L,D] view(s) the attention kernels
    take — no transpose copy — as q or (q, k). Rounding points: include/vblade.h."""
    norms, ropes, dev, B, L, W, D, table = _qk_modes(q_proj, k_proj, heads, norm, rope, rope_start, cos, sin, freqs)

    keep = []   # tensors the launch reads stay alive until it is enqueued

    def fill(x, mode, rmode, w, b, eps):
        x3 = x.reshape(B, L, W) if x.dim() == 4 else x   # a view for rows-contiguous inputs
        ok = (x3.stride(2) == 1 and (B == 1 or x3.stride(0) % 8 == 0) and x3.stride(1) % 8 == 0 and x3.stride(1) >= W
              and x3.data_ptr() % 16 == 0)
        if inplace:
            if not ok or x3.data_ptr() != x.data_ptr():
                raise ValueError("qk_prologue: inplace needs 16-byte aligned rows with strides that are multiples of 8")
            out = x3
        else:
            if not ok:
                x3 = x3.contiguous()
            out = torch.empty(B, L, W, device=dev, dtype=x.dtype)
        a = _lib.QkPrologueArgs()
        a.x, a.out = x3.data_ptr(), out.data_ptr()
        a.x_stride = (ctypes.c_int64 * 2)(x3.stride(0) if B > 1 else 0, x3.stride(1))
        a.out_stride = (ctypes.c_int64 * 2)(out.stride(0) if B > 1 else 0, out.stride(1))
        a.B, a.L, a.H, a.D = B, L, heads, D
        a.dtype = _dtype_code(x)
        a.norm = QK_NORMS[mode]
        if mode == "none" and (w is not None or b is not None):
            raise ValueError("qk_prologue: weight/bias given without a norm")
        if mode == "rms" and b is not None:
            raise ValueError("qk_prologue: the RMSNorm takes no bias")
        n = D if mode == "layer" else W
        w, b = _qk_affine("weight", w, n, x, dev), _qk_affine("bias", b, n, x, dev)
        if w is not None and b is not None and w.dtype != b.dtype:
            raise TypeError("qk_prologue: weight and bias must share a dtype")
        a.weight, a.bias = _ptr(w), _ptr(b)
        a.affine_f32 = int(any(t is not None and t.dtype == torch.float32 for t in (w, b)))
        a.eps = float(eps)
        a.rope = QK_ROPES[rmode]
        if rmode == "real":
            a.rope_start = int(rope_start)
            a.cos, a.sin = table["cos"].data_ptr(), table["sin"].data_ptr()
        elif rmode == "complex":
            a.freqs = table["freqs"].data_ptr()
            a.freqs_f64 = int(table["freqs"].dtype == torch.float64)
        keep.extend((x3, w, b))
        return a, out

    qa, q_out = fill(q_proj, norms[0], ropes[0], q_weight, q_bias, q_eps)
    ka = k_out = None
    if k_proj is not None:
        ka, k_out = fill(k_proj, norms[1], ropes[1], k_weight, k_bias, q_eps if k_eps is None else k_eps)
    check(_lib.load().vb_qk_prologue(ctypes.byref(qa), ctypes.byref(ka) if ka is not None else None,
                                     _stream(dev)), "vb_qk_prologue")
    del keep
    q_view = q_out.view(B, L, heads, D).transpose(1, 2)
    if k_proj is None:
        return q_view
    return q_view, k_out.view(B, L, heads, D).transpose(1, 2)


def qk_prologue_bwd(q_proj: Optional[torch.Tensor] = None, k_proj: Optional[torch.Tensor] = None, *,
                    gq: Optional[torch.Tensor] = None, gk: Optional[torch.Tensor] = None, heads: int,
                    norm="none", q_weight=None, q_bias=None, q_eps: float = 1e-5,
                    k_weight=None, k_bias=None, k_eps: Optional[float] = None,
                    rope="none", rope_start: int = 0, cos=None, sin=None, freqs=None,
                    need_wgrad=(False, False, False, False), grid_limit: int = 0):
    """vb_qk_prologue_bwd: the backward of ``qk_prologue`` in one pass over q and k.

    The forward's inputs and keywords (without ``inplace``), plus ``gq`` / ``gk``: the gradients
    w.r.t. the [B,heads,L,D] views the forward returned, in any memory whose strides are multiples
    of 8 ([B,H,L,D]-contiguous or the transposed view of [B,L,H,D] memory; anything else is copied).
    A tensor whose gradient is None is left out of the launch. ``need_wgrad`` = (q_w, q_b, k_w, k_b)
    asks for the norm parameters' gradients (fp32, summed in an order fixed by the shape and
    ``grid_limit``; 0 = the library's own grid). Returns (dq_proj, dk_proj, dq_w, dq_b, dk_w, dk_b)
    with None where not requested; dq_proj / dk_proj have the projections' shape and dtype."""
    if gq is None and gk is None:
        raise ValueError("qk_prologue_bwd: gq and gk are both None")
    if (gq is not None and q_proj is None) or (gk is not None and k_proj is None):
        raise ValueError("qk_prologue_bwd: a gradient needs the forward's input of its tensor")
    first = q_proj if q_proj is not None else k_proj
    norms, ropes, dev, B, L, W, D, table = _qk_modes(first, k_proj if q_proj is not None else None, heads, norm, rope,
                                                     rope_start, cos, sin, freqs)
    keep = []   # tensors the launch reads stay alive until it is enqueued
    outs = []

    def fill(x, g, mode, rmode, w, b, eps, want_w, want_b):
        if tuple(g.shape) != (B, heads, L, D) or g.dtype != x.dtype:
            raise ValueError(f"qk_prologue_bwd: a gradient must be [{B},{heads},{L},{D}] {x.dtype}, got "
                             f"{tuple(g.shape)} {g.dtype}")
        _check_dev("qk_prologue_bwd: gradient", g, dev)
        x3 = x.detach().reshape(B, L, W) if x.dim() == 4 else x.detach()
        if not (x3.stride(2) == 1 and (B == 1 or x3.stride(0) % 8 == 0) and x3.stride(1) % 8 == 0
                and x3.stride(1) >= W and x3.data_ptr() % 16 == 0):
            x3 = x3.contiguous()
        g = g.detach()
        if not (g.stride(3) == 1 and (B == 1 or g.stride(0) % 8 == 0) and g.stride(1) % 8 == 0 and g.stride(2) % 8 == 0
                and (heads == 1 or g.stride(1) >= D) and g.data_ptr() % 16 == 0):
            g = g.contiguous()
        dx = torch.empty(B, L, W, device=dev, dtype=x.dtype)
        a = _lib.QkPrologueBwdArgs()
        a.x, a.g, a.dx = x3.data_ptr(), g.data_ptr(), dx.data_ptr()
        a.x_stride = (ctypes.c_int64 * 2)(x3.stride(0) if B > 1 else 0, x3.stride(1))
        a.g_stride = (ctypes.c_int64 * 3)(g.stride(0) if B > 1 else 0, g.stride(2), g.stride(1) if heads > 1 else D)
        a.dx_stride = (ctypes.c_int64 * 2)(dx.stride(0) if B > 1 else 0, dx.stride(1))
        a.B, a.L, a.H, a.D = B, L, heads, D
        a.dtype = _dtype_code(x)
        a.norm = QK_NORMS[mode]
        if mode == "none" and (w is not None or b is not None):
            raise ValueError("qk_prologue_bwd: weight/bias given without a norm")
        if mode == "rms" and b is not None:
            raise ValueError("qk_prologue_bwd: the RMSNorm takes no bias")
        if (want_w and w is None) or (want_b and b is None):
            raise ValueError("qk_prologue_bwd: need_wgrad asks for the gradient of a parameter that was not given")
        n = D if mode == "layer" else W
        w, b = _qk_affine("weight", w, n, x, dev), _qk_affine("bias", b, n, x, dev)
        if w is not None and b is not None and w.dtype != b.dtype:
            raise TypeError("qk_prologue_bwd: weight and bias must share a dtype")
        a.weight, a.bias = _ptr(w), _ptr(b)
        a.affine_f32 = int(any(t is not None and t.dtype == torch.float32 for t in (w, b)))
        a.eps = float(eps)
        a.rope = QK_ROPES[rmode]
        if rmode == "real":
            a.rope_start = int(rope_start)
            a.cos, a.sin = table["cos"].data_ptr(), table["sin"].data_ptr()
        elif rmode == "complex":
            a.freqs = table["freqs"].data_ptr()
            a.freqs_f64 = int(table["freqs"].dtype == torch.float64)
        a.grid_limit = int(grid_limit)
        dw = torch.empty(n, device=dev, dtype=torch.float32) if want_w else None
        db = torch.empty(n, device=dev, dtype=torch.float32) if want_b else None
        a.dweight, a.dbias = _ptr(dw), _ptr(db)
        keep.extend((x3, g, w, b))
        outs.append((dx.view(x.shape), dw, db))
        return a

    want = [bool(v) for v in need_wgrad]
    qa = ka = None
    if gq is not None:
        qa = fill(q_proj, gq, norms[0], ropes[0], q_weight, q_bias, q_eps, want[0], want[1])
    else:
        outs.append((None, None, None))
    if gk is not None:
        ka = fill(k_proj, gk, norms[1], ropes[1], k_weight, k_bias, q_eps if k_eps is None else k_eps, want[2], want[3])
    else:
        outs.append((None, None, None))
    lib = _lib.load()
    refs = [ctypes.byref(a) if a is not None else None for a in (qa, ka)]
    nbytes = lib.vb_qk_prologue_bwd_workspace_size(*refs)
    if nbytes:
        ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        head = qa if qa is not None else ka     # the first tensor of the call names the workspace
        head.workspace, head.workspace_bytes = ws.data_ptr(), nbytes
        keep.append(ws)
    check(lib.vb_qk_prologue_bwd(*refs, _stream(dev)), "vb_qk_prologue_bwd")
    del keep
    (dq, dqw, dqb), (dk, dkw, dkb) = outs
    return dq, dk, dqw, dqb, dkw, dkb


# ----------------------------------------------------------------------------------------------
# multi-level path (Triton/cogvideo_newattn.py + kernels/block_sparse_attn_kernel_with_backward_9_10.py)
# ----------------------------------------------------------------------------------------------
# Triton/cogvideo_newattn.py:12-18
ML_MASK_RATIOS = {1: (0.0, 0.05), 2: (0.05, 0.15), 4: (0.15, 0.25), 8: (0.25, 0.5), 0: (0.5, 1.0)}


def kv_pyramid_rows(L: int) -> int:
    return int(_lib.load().vb_kv_pyramid_rows(int(L)))


def kv_pyramid_outputs(k):
    """Allocate kv_pyramid's outputs on the current stream (see pool_kv_outputs)."""
    B, H, L, D = k.shape
    R = kv_pyramid_rows(L)
    return (torch.empty(B, H, R, D, device=k.device, dtype=k.dtype),
            torch.empty(B, H, R, D, device=k.device, dtype=k.dtype))


def kv_pyramid(k, v, rows=None, stream=None, out=None):
    """vb_kv_pyramid: K/V [B,H,L,D] (reordered through `rows`) -> pyramids [B,H,15*Lpad/8,D]:
    level-1 rows (zero beyond L), then the 2x, 4x, 8x mean-pooled rows (replicate padding).
    ``stream``: as pool_kv."""
    if v.shape != k.shape:
        raise ValueError(f"kv_pyramid: k and v must have the same shape, got {tuple(k.shape)} and "
                         f"{tuple(v.shape)}")
    if rows is not None and rows.numel() != k.shape[2]:
        raise ValueError(f"kv_pyramid: rows has {rows.numel()} entries for {k.shape[2]} keys")
    dev = _require_gpu(k, v, rows)
    k, v = _aligned_bhld(k), _aligned_bhld(v)
    if stream is not None:   # see pool_kv
        for t in (k, v, rows) + tuple(out or ()):
            if t is not None:
                t.record_stream(stream)
    B, H, L, D = k.shape
    kpyr, vpyr = out if out is not None else kv_pyramid_outputs(k)
    check(_lib.load().vb_kv_pyramid(k.data_ptr(), v.data_ptr(), ctypes.cast(_s3(k), ctypes.c_void_p),
                                    ctypes.cast(_s3(v), ctypes.c_void_p), _ptr(rows), B, H, L, D,
                                    _dtype_code(k), kpyr.data_ptr(), vpyr.data_ptr(),
                                    stream.cuda_stream if stream is not None else _stream(dev)),
          "vb_kv_pyramid")
    return kpyr, vpyr


def pyramid_levels(pyr: torch.Tensor, L: int):
    """Views [level1, level2, level4, level8] of a pyramid tensor (for tests and the backward)."""
    Lpad = (L + BLOCK - 1) // BLOCK * BLOCK
    offs = [0, Lpad, Lpad + Lpad // 2, Lpad + Lpad // 2 + Lpad // 4, 15 * Lpad // 8]
    return [pyr[:, :, offs[i]:offs[i + 1]] for i in range(4)]


def _level_bands(ratios):
    """mask_ratios {level: (start, end)} -> (int32 values, float64 starts, float64 ends), dict order."""
    ratios = ML_MASK_RATIOS if ratios is None else ratios
    vals = np.array([int(v) for v in ratios], dtype=np.int32)
    st = np.array([float(r[0]) for r in ratios.values()], dtype=np.float64)
    en = np.array([float(r[1]) for r in ratios.values()], dtype=np.float64)
    if len(vals) > 8:
        raise ValueError("level mask: at most 8 bands")
    return vals, st, en


def level_mask(po, ratios=None):
    """vb_level_mask: transfer_attn_to_mask (Triton/cogvideo_newattn.py:154-207) on scores po
    [B,H,nr,nc] -> uint8 levels (ties: lower column first)."""
    dev = _require_gpu(po)
    po = po.contiguous()
    B, H, nr, nc = po.shape
    vals, st, en = _level_bands(ratios)
    mask = torch.empty(B, H, nr, nc, device=dev, dtype=torch.uint8)
    check(_lib.load().vb_level_mask(po.data_ptr(), B, H, nr, nc, len(vals), vals.ctypes.data,
                                    st.ctypes.data, en.ctypes.data, _dtype_code(po), mask.data_ptr(),
                                    _stream(dev)), "vb_level_mask")
    return mask


def ml_attention_fwd(q, kpyr, vpyr, level_mask_u8, *, q_rows=None, scale=None, ref_tail=True,
                     want_lse=False, heavy_rows=2, out=None, persistent: bool = False,
                     out_layout: str = "bhld"):
    """vb_ml_attn_fwd: multi-level attention of q [B,H,L,D] over the KV pyramids. Returns out
    (rows through q_rows) and, if want_lse, the fp32 natural-log LSE [B,H,L] (at the caller's rows
    q_rows[g], like out: include/vblade.h).
    ``persistent``: as attention_fwd: the work-queue launch, or, while the current stream is being
    captured into a graph and has no queue yet, the one-workgroup-per-q-block form (the same bits; no
    queue is created inside a capture).
    ``out_layout`` / ``out``: as attention_fwd."""
    io_layout_code("out_layout", out_layout)
    dev = _require_gpu(q, kpyr, vpyr, level_mask_u8, q_rows)
    q = _aligned_bhld(q)
    B, H, L, D = q.shape
    nb = (L + BLOCK - 1) // BLOCK
    if tuple(level_mask_u8.shape) != (B, H, nb, nb) or level_mask_u8.dtype != torch.uint8:
        raise ValueError(f"vblade: level mask must be uint8 [B,H,{nb},{nb}]")
    R = kv_pyramid_rows(L)
    for t in (kpyr, vpyr):
        if tuple(t.shape) != (B, H, R, D) or not t.is_contiguous() or t.dtype != q.dtype:
            raise ValueError(f"vblade: pyramids must be contiguous [B,H,{R},D] in q's dtype")
    m = level_mask_u8
    if m.stride(-1) != 1:
        m = m.contiguous()
    if out is None:
        if out_layout == "blhd":
            out = _empty_bhld(B, H, L, D, dev, q.dtype, out_layout)
        else:
            out = torch.empty_like(q) if q.is_contiguous() else torch.empty(B, H, L, D, device=dev, dtype=q.dtype)
    lse = torch.empty(B, H, L, device=dev, dtype=torch.float32) if want_lse else None
    a = MlAttnArgs()
    a.q, a.q_stride, a.q_rows = q.data_ptr(), _s3(q), _ptr(q_rows)
    a.kpyr, a.vpyr = kpyr.data_ptr(), vpyr.data_ptr()
    a.level_mask = m.data_ptr()
    a.mask_stride = (ctypes.c_int64 * 3)(m.stride(0), m.stride(1), m.stride(2))
    a.out, a.out_stride, a.lse = out.data_ptr(), _s3(out), _ptr(lse)
    a.B, a.H, a.L, a.D = B, H, L, D
    a.scale = float(scale) if scale else 0.0
    a.ref_tail = 1 if ref_tail else 0
    a.dtype = _dtype_code(q)
    a.heavy_rows = int(heavy_rows)
    a.work_queue = _work_queue_ptr(dev, persistent)
    check(_lib.load().vb_ml_attn_fwd(ctypes.byref(a), _stream(dev)), "vb_ml_attn_fwd")
    return (out, lse) if want_lse else out


def ml_attention_bwd(dout, q, kpyr, vpyr, level_mask_u8, out, lse, *, rows=None, scale=None,
                     ref_tail=True, heavy_rows=2, kernel_select: int = 0, kernels_ran: Optional[list] = None,
                     grads=None, workspace_bytes: Optional[list] = None, grad_layout: str = "bhld"):
    """vb_ml_attn_bwd: gradients of the multi-level attention. q/out/dout [B,H,L,D] (rows through
    ``rows``), pyramids and mask as the forward; lse as ml_attention_fwd(want_lse=True) wrote it.
    Returns (dq, dk, dv) [B,H,L,D] in q's dtype (dk/dv at the caller's rows). ``kernel_select`` /
    ``kernels_ran`` as attention_bwd (VB_BWD_SEL_DQ_RING4 is refused here). ``grads``: (dq, dk, dv)
    buffers of the caller, [B,H,L,D] in q's dtype on q's device, any strides the kernels accept
    (unit d-stride, the others multiples of 8 elements, 16-byte aligned); they are fully
    overwritten and returned. ``workspace_bytes`` (a list) receives the size
    vb_ml_attn_bwd_workspace_size reported for the call. ``dout`` is read through its strides (copied
    only when it misses the 16-byte rule); ``grad_layout``: the memory order of the dq, dk, dv
    allocated here (without ``grads``), "bhld" or "blhd" as attention_bwd."""
    io_layout_code("grad_layout", grad_layout)
    dev = _require_gpu(dout, q, kpyr, vpyr, level_mask_u8, out, lse, rows)
    q, out, dout = _aligned_bhld(q), _aligned_bhld(out), _aligned_bhld(dout)
    B, H, L, D = q.shape
    m = level_mask_u8 if level_mask_u8.stride(-1) == 1 else level_mask_u8.contiguous()
    lse = lse.float().contiguous()
    if grads is None:
        dq, dk, dv = (_empty_bhld(B, H, L, D, dev, q.dtype, grad_layout) for _ in range(3))
    else:
        dq, dk, dv = grads
        for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
            _check_dev(f"ml_attention_bwd: grads {name}", t, dev)
            if tuple(t.shape) != (B, H, L, D) or t.dtype != q.dtype:
                raise ValueError(f"ml_attention_bwd: grads {name} must be [{B},{H},{L},{D}] {q.dtype}, got "
                                 f"{tuple(t.shape)} {t.dtype}")
    a = MlBwdArgs()
    a.q, a.q_stride, a.rows = q.data_ptr(), _s3(q), _ptr(rows)
    a.kpyr, a.vpyr = kpyr.data_ptr(), vpyr.data_ptr()
    a.level_mask = m.data_ptr()
    a.mask_stride = (ctypes.c_int64 * 3)(m.stride(0), m.stride(1), m.stride(2))
    a.out, a.out_stride, a.lse = out.data_ptr(), _s3(out), lse.data_ptr()
    a.dout, a.dout_stride = dout.data_ptr(), _s3(dout)
    a.dq, a.dq_stride = dq.data_ptr(), _s3(dq)
    a.dk, a.dv, a.dk_stride, a.dv_stride = dk.data_ptr(), dv.data_ptr(), _s3(dk), _s3(dv)
    a.B, a.H, a.L, a.D = B, H, L, D
    a.scale = float(scale) if scale else 0.0
    a.ref_tail = 1 if ref_tail else 0
    a.dtype = _dtype_code(q)
    a.heavy_rows = int(heavy_rows)
    a.kernel_select = int(kernel_select)
    ran = ctypes.c_int32(0)
    a.kernels_ran = ctypes.pointer(ran)
    lib = _lib.load()
    nbytes = int(lib.vb_ml_attn_bwd_workspace_size(ctypes.byref(a)))
    if workspace_bytes is not None:
        workspace_bytes.append(nbytes)
    ws = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    check(lib.vb_ml_attn_bwd(ctypes.byref(a), _stream(dev)), "vb_ml_attn_bwd")
    if kernels_ran is not None:
        kernels_ran.append(ran.value)
    return dq, dk, dv


def default_scale(D: int) -> float:
    return 1.0 / math.sqrt(D)
