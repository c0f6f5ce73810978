"""Reference of the one-softmax ("joint") attention and its exact gradient, for the tests of
vb_attn_bwd_joint / grad_combine="joint". Everything here is in REORDERED row order, on the CPU.

The function (include/vblade.h, vb_attn_bwd_joint): with kp, vp = the mean pool of k, v over ``gap``
consecutive keys (replicate padding onto the last key),

    lse[i] = log( sum_{j kept by the block mask} exp(scale q_i.k_j) + sum_m exp(scale q_i.kp_m + beta) )
    out[i] = sum_j exp(scale q_i.k_j - lse_i) v_j + sum_m exp(scale q_i.kp_m + beta - lse_i) vp_m

``joint_forward`` states it in differentiable fp64 torch (mean pool, block mask expanded to keys, bias
on the pooled logits, logsumexp); ``joint_autograd`` differentiates that statement.

``joint_oracle_bwd`` gets the same gradient from oracle/bsa_oracle.py::two_branch_attention_bwd, with
or without its rounding emulation, by a substitution in which every factor of 2 is exact:

    out1 = out2 = out,  lse1 = lse,  lse2 = lse - beta,  alpha = 0.5,  dout -> 2 dout

Each branch then carries the weight 0.5 (storage(1 - 0.5) = 0.5 in every dtype), the doubled dO
restores P (dP - Delta) with Delta = rowsum(dO * out), and the pooled branch's scores, which carry no
bias in the oracle, get it through lse2. ``alpha_constant_bwd`` is the two-branch form the default
training path differentiates (both LSEs and alpha held constant), on the branch statistics of the same
fp64 forward: the gradient grad_combine="reference" keeps.
"""
import math

import torch

import bsa_oracle as O


def mean_pool(x, gap):
    """[B,H,L,D] -> [B,H,ceil(L/gap),D]: mean over ``gap`` consecutive rows, the last group replicate-padded
    with the last row. Differentiable, in x's dtype."""
    B, H, L, D = x.shape
    pad = (-L) % gap
    if pad:
        x = torch.cat([x, x[:, :, L - 1:L].expand(B, H, pad, D)], dim=2)
    return x.reshape(B, H, (L + pad) // gap, gap, D).mean(3)


def expand_mask(mask, Lq, Lk, block=128):
    """Block mask [B,H,nbq,nbk] -> bool [B,H,Lq,Lk] over keys."""
    m = mask.bool()
    return m[:, :, torch.arange(Lq) // block][:, :, :, torch.arange(Lk) // block]


def joint_forward(q, k, v, mask, gap, beta, sm_scale=None, block=128, pooled=None):
    """fp64 (out [B,H,Lq,D], lse [B,H,Lq]) of the function above, differentiable in q, k, v.
    ``pooled``: (kp, vp) to use in place of the mean pool of k, v (e.g. the device's rounded ones; then
    no gradient reaches k, v through them)."""
    q, k, v = q.double(), k.double(), v.double()
    Lq, Lk, D = q.shape[2], k.shape[2], q.shape[3]
    scale = sm_scale if sm_scale is not None else 1.0 / math.sqrt(D)
    kp, vp = (mean_pool(k, gap), mean_pool(v, gap)) if pooled is None else (t.double() for t in pooled)
    s_main = torch.matmul(q, k.transpose(-1, -2)) * scale
    s_main = s_main.masked_fill(~expand_mask(mask, Lq, Lk, block), float("-inf"))
    s_pool = torch.matmul(q, kp.transpose(-1, -2)) * scale + beta
    s = torch.cat([s_main, s_pool], dim=-1)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse[..., None])
    return torch.matmul(p, torch.cat([v, vp], dim=2)), lse


def joint_autograd(q, k, v, dout, mask, gap, beta, sm_scale=None):
    """(dq, dk, dv, out, lse) in fp64: torch autograd of joint_forward, the pool included."""
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    out, lse = joint_forward(q, k, v, mask, gap, beta, sm_scale)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout.double())
    return dq, dk, dv, out.detach(), lse.detach()


def joint_oracle_bwd(q, k, v, kp, vp, out, lse, dout, mask, gap, beta, sm_scale=None,
                     store_dtype=torch.bfloat16, emulate_rounding=False):
    """The joint gradient (dq, dk, dv fp32) by the substitution of the module docstring. ``out`` and
    ``lse`` are the joint forward's, ``kp``/``vp`` the pooled keys it used."""
    lse = lse.double()
    half = torch.full(tuple(q.shape[:3]), 0.5)
    return O.two_branch_attention_bwd(q, k, v, kp, vp, out, lse, out, lse - beta, half, 2.0 * dout.double(),
                                      mask, gap, sm_scale=sm_scale, store_dtype=store_dtype,
                                      emulate_rounding=emulate_rounding)


def alpha_constant_bwd(q, k, v, dout, mask, gap, beta, sm_scale=None):
    """(dq, dk, dv fp32) of the two-branch form with both LSEs and alpha constants, on the exact fp64
    branch statistics of the same function: out = alpha out1 + (1 - alpha) out2 with alpha =
    exp(lse1 - lse). Every row must keep at least one block (lse1 finite)."""
    q, k, v = q.double(), k.double(), v.double()
    kp, vp = mean_pool(k, gap), mean_pool(v, gap)
    out1, lse1 = O.joint_attention(q, k, v, mask, sm_scale=sm_scale)
    out2, lse2 = O.joint_attention(q, None, None, None, kp, vp, use_main=False, sm_scale=sm_scale)
    lse = torch.logaddexp(lse1, lse2 + beta)
    alpha = torch.exp(lse1 - lse)
    return O.two_branch_attention_bwd(q, k, v, kp, vp, out1, lse1, out2, lse2, alpha, dout.double(), mask, gap,
                                      sm_scale=sm_scale, store_dtype=torch.float32)


def rel(x, ref):
    ref = ref.double()
    return ((x.double() - ref).norm() / ref.norm().clamp_min(1e-300)).item()
