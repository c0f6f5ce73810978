"""Monkey-patch surface: attention processors and the two setter functions.

Mirrors cogvideox/train/modify_cogvideo.py:11-91 and wanx/train/modify_wan.py:75-168. The
processors are the callers of the hot path (the QKV projections stay in PyTorch; so do the norms
and RoPE unless ``fused_qk=True`` hands them to the library's one-pass prologue, ops.qk_prologue,
and with ``fused_qk_backward=True`` also under autograd, through autograd.qk_prologue);
``attn.inner_attention(q, k, v)`` is the vblade module. diffusers is imported lazily and only
for its RoPE helper; nothing here needs it at import time.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import autograd, ops
from .attention import AdaptiveBlockSparseAttn


def _apply_rotary_emb_real(x: torch.Tensor, freqs_cis) -> torch.Tensor:
    """diffusers.models.embeddings.apply_rotary_emb with use_real=True, unbind_dim=-1 (the form
    CogVideoX's processor uses): x * cos + rotate_half(x) * sin over interleaved pairs."""
    try:  # prefer the library's own implementation when present
        from diffusers.models.embeddings import apply_rotary_emb
        return apply_rotary_emb(x, freqs_cis)
    except Exception:  # noqa: BLE001 - diffusers absent in this image
        cos, sin = freqs_cis
        cos, sin = cos[None, None].to(x.device), sin[None, None].to(x.device)
        x_real, x_imag = x.reshape(*x.shape[:-1], -1, 2).unbind(-1)
        x_rot = torch.stack([-x_imag, x_real], dim=-1).flatten(3)
        return (x.float() * cos + x_rot.float() * sin).to(x.dtype)


# ---------------------------------------------------------------------------------------------
# fused_qk: which calls the one-pass prologue (ops.qk_prologue) may take. Anything it cannot
# identify exactly keeps the eager chain, silently and completely.
# ---------------------------------------------------------------------------------------------
def _records_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def _prologue_inputs_ok(query, key, value, heads, head_dim, *params, backward: bool = False) -> bool:
    """HIP tensors of one 16-bit dtype and one shape, a head size the kernel has, and no autograd
    recording unless ``backward`` (fused_qk_backward) lets the call take autograd.qk_prologue."""
    if not (query.is_cuda and key.is_cuda and query.dtype in (torch.bfloat16, torch.float16)):
        return False
    if key.dtype != query.dtype or value.dtype != query.dtype or key.shape != query.shape:
        return False
    if head_dim not in (64, 128) or heads * head_dim > 8192:
        return False
    if not backward and _records_grad(query, key, *params):
        return False
    return True


def _shares_storage(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Whether a is a view of b's memory (no copy was made between them)."""
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def _norm_params(norm):
    return [] if norm is None else [getattr(norm, "weight", None), getattr(norm, "bias", None)]


def _layer_norm_spec(norm, head_dim, dtype):
    """("layer", weight, bias, eps) for exactly torch.nn.LayerNorm over (head_dim,) with parameters
    of the tensors' dtype, ("none", ...) for no norm, None for anything else."""
    if norm is None:
        return "none", None, None, 0.0
    if type(norm) is not torch.nn.LayerNorm or tuple(norm.normalized_shape) != (head_dim,):
        return None
    w, b = norm.weight, norm.bias
    if any(t is not None and t.dtype != dtype for t in (w, b)):   # the eager chain's own dtype rule
        return None
    return "layer", w, b, float(norm.eps)


def _rms_norm_spec(norm, width, dtype):
    """The same for exactly torch.nn.RMSNorm over (width,) with a weight of the tensors' dtype (a
    wider weight would promote the eager result)."""
    if norm is None:
        return "none", None, None, 0.0
    rms = getattr(torch.nn, "RMSNorm", None)
    if rms is None or type(norm) is not rms or tuple(norm.normalized_shape) != (width,):
        return None
    w = norm.weight
    if w is not None and w.dtype != dtype:
        return None
    eps = norm.eps if norm.eps is not None else torch.finfo(dtype).eps   # torch.rms_norm's default
    return "rms", w, None, float(eps)


class CogVideoXBlockSparseAttnProcessor:
    """SageAttnCogVideoXAttnProcessor (modify_cogvideo.py:11-76): joint text+video self-attention
    whose inner attention is ``attn.inner_attention``. Text tokens come FIRST in the sequence.
    ``fused_qk``: norm_q/norm_k and RoPE in one library pass where the call allows it (see
    ``_fused_qk``); ``last_path`` tells which chain the last call took, "fused" or "eager".
    ``fused_qk_backward`` (with ``fused_qk``): a call that records autograd takes the fused pass too,
    through autograd.qk_prologue, instead of keeping the eager chain.
    ``projection_layout``: the setter's flag (the shared module then returns its output in the
    projections' [B,L,H*D] memory, io_layout="blhd"), kept here for inspection; ``last_out_is_view``
    tells whether the tensor the last call gave to ``to_out[0]`` shared storage with what
    ``inner_attention`` returned (True: the reshape below was a view) or was a copy of it."""

    def __init__(self, idx: int = 0, fused_qk: bool = False, fused_qk_backward: bool = False,
                 projection_layout: bool = False):
        self.idx = idx
        self.fused_qk = fused_qk
        self.fused_qk_backward = fused_qk_backward
        self.projection_layout = projection_layout
        self.last_path = None
        self.last_out_is_view = None

    def _fused_qk(self, attn, query, key, value, head_dim, text_seq_length, image_rotary_emb):
        """(q, k) [B,H,L,D] from the [B,L,H*D] projections through ops.qk_prologue, or None when this
        call keeps the eager chain: CPU or fp32 tensors, autograd recording without
        ``fused_qk_backward``, a norm that is not exactly nn.LayerNorm((head_dim,)), or rotary tables
        that are not a (cos, sin) pair of fp32 [video rows, head_dim]."""
        norm_q, norm_k = getattr(attn, "norm_q", None), getattr(attn, "norm_k", None)
        params = (*_norm_params(norm_q), *_norm_params(norm_k))
        if not _prologue_inputs_ok(query, key, value, attn.heads, head_dim, *params,
                                   backward=self.fused_qk_backward):
            return None
        nq = _layer_norm_spec(norm_q, head_dim, query.dtype)
        nk = _layer_norm_spec(norm_k, head_dim, query.dtype)
        if nq is None or nk is None:
            return None
        rope, cos, sin = "none", None, None
        if image_rotary_emb is not None and query.shape[1] > text_seq_length:   # else no row takes RoPE
            if not (isinstance(image_rotary_emb, (tuple, list)) and len(image_rotary_emb) == 2):
                return None
            cos, sin = image_rotary_emb
            shape = (query.shape[1] - text_seq_length, head_dim)
            if not all(torch.is_tensor(t) and t.dtype == torch.float32 and tuple(t.shape) == shape
                       and not t.requires_grad for t in (cos, sin)):
                return None
            rope = "real"
        k_rope = "none" if getattr(attn, "is_cross_attention", False) else rope
        op = autograd.qk_prologue if _records_grad(query, key, *params) else ops.qk_prologue
        return op(query, key, heads=attn.heads, norm=(nq[0], nk[0]),
                  q_weight=nq[1], q_bias=nq[2], q_eps=nq[3], k_weight=nk[1], k_bias=nk[2], k_eps=nk[3],
                  rope=(rope, k_rope), rope_start=text_seq_length, cos=cos, sin=sin)

    def __call__(self, attn, hidden_states, encoder_hidden_states, attention_mask=None,
                 image_rotary_emb=None):
        assert attention_mask is None, "Attention mask is not supported"
        text_seq_length = encoder_hidden_states.size(1)
        hidden_states = torch.cat([encoder_hidden_states, hidden_states], dim=1)
        batch_size = encoder_hidden_states.shape[0]
        query = attn.to_q(hidden_states)
        key = attn.to_k(hidden_states)
        value = attn.to_v(hidden_states)
        head_dim = key.shape[-1] // attn.heads
        fused = self._fused_qk(attn, query, key, value, head_dim, text_seq_length,
                               image_rotary_emb) if self.fused_qk else None
        self.last_path = "eager" if fused is None else "fused"
        value = value.view(batch_size, -1, attn.heads, head_dim).transpose(1, 2)
        if fused is not None:
            # the attention kernels read the [B,H,L,D] views through their strides: no copy of v either
            query, key = fused
        else:
            query = query.view(batch_size, -1, attn.heads, head_dim).transpose(1, 2)
            key = key.view(batch_size, -1, attn.heads, head_dim).transpose(1, 2)
            if getattr(attn, "norm_q", None) is not None:
                query = attn.norm_q(query).to(dtype=value.dtype)
            if getattr(attn, "norm_k", None) is not None:
                key = attn.norm_k(key).to(dtype=value.dtype)
            if image_rotary_emb is not None:
                query[:, :, text_seq_length:] = _apply_rotary_emb_real(query[:, :, text_seq_length:], image_rotary_emb)
                if not getattr(attn, "is_cross_attention", False):
                    key[:, :, text_seq_length:] = _apply_rotary_emb_real(key[:, :, text_seq_length:], image_rotary_emb)
            value = value.contiguous()
        hidden_states = attn.inner_attention(query, key, value)
        attn_out = hidden_states
        hidden_states = hidden_states.transpose(1, 2).reshape(batch_size, -1, attn.heads * head_dim)
        self.last_out_is_view = _shares_storage(hidden_states, attn_out)
        hidden_states = attn.to_out[0](hidden_states)
        hidden_states = attn.to_out[1](hidden_states)
        encoder_hidden_states, hidden_states = hidden_states.split(
            [text_seq_length, hidden_states.size(1) - text_seq_length], dim=1)
        return hidden_states, encoder_hidden_states


def _projection_layout(attn_kwargs) -> bool:
    """Pop the setters' ``projection_layout`` flag; True selects the module's io_layout="blhd"."""
    flag = bool(attn_kwargs.pop("projection_layout", False))
    if flag:
        if attn_kwargs.get("io_layout", "blhd") != "blhd":
            raise ValueError("projection_layout=True is io_layout='blhd'; got io_layout="
                             f"{attn_kwargs['io_layout']!r} as well")
        attn_kwargs["io_layout"] = "blhd"
    return flag


def set_block_sparse_attn_cogvideox(model, verbose: bool = False, **attn_kwargs):
    """modify_cogvideo.py:79-91: ONE shared inner-attention module on every transformer block's
    attn1, processor swapped, the original kept as ``origin_processor``. Returns the module.
    ``fused_qk=True`` (default False) gives every processor the one-pass q/k norm + RoPE;
    ``fused_qk_backward=True`` (default False) keeps it under autograd as well (training).
    ``projection_layout=True`` (default False) sets the shared module's io_layout="blhd": its output
    (and under autograd dq, dk, dv) live in the projections' [B,L,H*D] memory, so the processors'
    reshape before ``to_out[0]`` is a view, not a copy (measured: DESIGN.md §3.8)."""
    fused_qk = bool(attn_kwargs.pop("fused_qk", False))
    fused_qk_backward = bool(attn_kwargs.pop("fused_qk_backward", False))
    projection_layout = _projection_layout(attn_kwargs)
    inner_attn = AdaptiveBlockSparseAttn("cog", **attn_kwargs)
    for idx, block in enumerate(model.transformer_blocks):
        block.attn1.verbose = verbose
        block.attn1.inner_attention = inner_attn
        origin = block.attn1.get_processor() if hasattr(block.attn1, "get_processor") else None
        block.attn1.set_processor(CogVideoXBlockSparseAttnProcessor(
            idx, fused_qk=fused_qk, fused_qk_backward=fused_qk_backward, projection_layout=projection_layout))
        if not hasattr(block.attn1, "origin_processor"):
            block.attn1.origin_processor = origin
    return inner_attn


class WanBlockSparseAttnProcessor:
    """WanAttnProcessor2_0 (modify_wan.py:75-148): video self-attention (attn1) with the
    complex-valued RoPE in float64; the I2V image branch also goes through inner_attention.
    ``fused_qk`` / ``fused_qk_backward`` / ``last_path`` / ``projection_layout`` / ``last_out_is_view``: as
    CogVideoXBlockSparseAttnProcessor."""

    def __init__(self, fused_qk: bool = False, fused_qk_backward: bool = False, projection_layout: bool = False):
        self.fused_qk = fused_qk
        self.fused_qk_backward = fused_qk_backward
        self.projection_layout = projection_layout
        self.last_path = None
        self.last_out_is_view = None

    def _fused_qk(self, attn, query, key, value, rotary_emb):
        """(q, k) [B,H,L,D] through ops.qk_prologue, or None when this call keeps the eager chain: the
        I2V image branch, k of another length than q, CPU or fp32 tensors, autograd recording without
        ``fused_qk_backward``, a norm that is not exactly nn.RMSNorm((heads*head_dim,)), or a rotary
        table that is not a complex [1,1,L,head_dim/2] tensor."""
        if getattr(attn, "add_k_proj", None) is not None or query.dim() != 3:
            return None
        width = query.shape[-1]
        if width % attn.heads:
            return None
        head_dim = width // attn.heads
        norm_q, norm_k = getattr(attn, "norm_q", None), getattr(attn, "norm_k", None)
        params = (*_norm_params(norm_q), *_norm_params(norm_k))
        if not _prologue_inputs_ok(query, key, value, attn.heads, head_dim, *params,
                                   backward=self.fused_qk_backward):
            return None
        nq = _rms_norm_spec(norm_q, width, query.dtype)
        nk = _rms_norm_spec(norm_k, width, query.dtype)
        if nq is None or nk is None:
            return None
        rope = "none"
        if rotary_emb is not None:
            if not (torch.is_tensor(rotary_emb) and rotary_emb.dtype in (torch.complex64, torch.complex128)
                    and tuple(rotary_emb.shape) == (1, 1, query.shape[1], head_dim // 2)
                    and not rotary_emb.requires_grad):
                return None
            rope = "complex"
        op = autograd.qk_prologue if _records_grad(query, key, *params) else ops.qk_prologue
        return op(query, key, heads=attn.heads, norm=(nq[0], nk[0]),
                  q_weight=nq[1], q_eps=nq[3], k_weight=nk[1], k_eps=nk[3], rope=rope, freqs=rotary_emb)

    def __call__(self, attn, hidden_states, encoder_hidden_states=None, attention_mask=None,
                 rotary_emb: Optional[torch.Tensor] = None):
        encoder_hidden_states_img = None
        if getattr(attn, "add_k_proj", None) is not None:
            encoder_hidden_states_img = encoder_hidden_states[:, :257]
            encoder_hidden_states = encoder_hidden_states[:, 257:]
        if encoder_hidden_states is None:
            encoder_hidden_states = hidden_states
        query = attn.to_q(hidden_states)
        key = attn.to_k(encoder_hidden_states)
        value = attn.to_v(encoder_hidden_states)
        fused = self._fused_qk(attn, query, key, value, rotary_emb) if self.fused_qk else None
        self.last_path = "eager" if fused is None else "fused"
        value = value.unflatten(2, (attn.heads, -1)).transpose(1, 2)
        if fused is not None:
            query, key = fused
        else:
            if getattr(attn, "norm_q", None) is not None:
                query = attn.norm_q(query)
            if getattr(attn, "norm_k", None) is not None:
                key = attn.norm_k(key)
            query = query.unflatten(2, (attn.heads, -1)).transpose(1, 2)
            key = key.unflatten(2, (attn.heads, -1)).transpose(1, 2)
            if rotary_emb is not None:
                def apply_rotary_emb(hs, freqs):
                    x_rotated = torch.view_as_complex(hs.to(torch.float64).unflatten(3, (-1, 2)))
                    return torch.view_as_real(x_rotated * freqs).flatten(3, 4).type_as(hs)
                query = apply_rotary_emb(query, rotary_emb)
                key = apply_rotary_emb(key, rotary_emb)
        hidden_states_img = None
        if encoder_hidden_states_img is not None:
            key_img = attn.norm_added_k(attn.add_k_proj(encoder_hidden_states_img))
            value_img = attn.add_v_proj(encoder_hidden_states_img)
            key_img = key_img.unflatten(2, (attn.heads, -1)).transpose(1, 2)
            value_img = value_img.unflatten(2, (attn.heads, -1)).transpose(1, 2)
            hidden_states_img = attn.inner_attention(query, key_img, value_img)
            hidden_states_img = hidden_states_img.transpose(1, 2).flatten(2, 3).type_as(query)
        hidden_states = attn.inner_attention(query, key, value)
        attn_out = hidden_states
        hidden_states = hidden_states.transpose(1, 2).flatten(2, 3).type_as(query)
        self.last_out_is_view = _shares_storage(hidden_states, attn_out)
        if hidden_states_img is not None:
            hidden_states = hidden_states + hidden_states_img
        hidden_states = attn.to_out[0](hidden_states)
        hidden_states = attn.to_out[1](hidden_states)
        return hidden_states


def set_adaptive_block_sparse_attn_wanx(model, verbose: bool = False, **attn_kwargs):
    """modify_wan.py:150-168: patch attn1 (self-attention) of every block; attn2 (cross-attention
    to the T5 tokens) keeps stock SDPA. Returns the shared module.
    ``fused_qk=True`` (default False) gives every processor the one-pass q/k norm + RoPE;
    ``fused_qk_backward=True`` (default False) keeps it under autograd as well (training).
    ``projection_layout=True`` (default False): as set_block_sparse_attn_cogvideox."""
    fused_qk = bool(attn_kwargs.pop("fused_qk", False))
    fused_qk_backward = bool(attn_kwargs.pop("fused_qk_backward", False))
    projection_layout = _projection_layout(attn_kwargs)
    inner_attn = AdaptiveBlockSparseAttn("wan", **attn_kwargs)
    for block in model.blocks:
        block.attn1.verbose = verbose
        block.attn1.inner_attention = inner_attn
        origin = block.attn1.get_processor() if hasattr(block.attn1, "get_processor") else None
        block.attn1.set_processor(WanBlockSparseAttnProcessor(fused_qk=fused_qk,
                                                               fused_qk_backward=fused_qk_backward,
                                                               projection_layout=projection_layout))
        if not hasattr(block.attn1, "origin_processor"):
            block.attn1.origin_processor = origin
    return inner_attn
