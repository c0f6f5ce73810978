"""Test helper: plain-torch restatement of the softmax-mass block score (include/vblade.h,
vb_mask_scores_mass), written from the header's semantics and independently of the kernel, on the
oracle's own sampled streams (O.pad_replicate + O.sample_tokens): a dense score matrix of the sampled
queries against the sampled keys, one softmax per query, block masses by a reshape. ``dtype`` float64
is the yardstick, float32 the eager evaluation whose own error against float64 sizes the tests' bound."""
import math

import numpy as np
import torch

import bsa_oracle as O

BLOCK = 128
KEEP = 32
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def sampled_streams(q, k, q_off, k_off, rows=None):
    """(qs, ks) [B,H,nb*keep,D]: q, k CPU tensors [B,H,L,D] reordered through ``rows`` (reordered
    position -> caller row, None: identity), replicate-padded to a multiple of 128 and sampled at the
    offsets q_off / k_off [B,H,keep] of every block."""
    if rows is not None:
        r = torch.as_tensor(np.asarray(rows), dtype=torch.long)
        q, k = q[:, :, r], k[:, :, r]
    qs = O.sample_tokens(O.pad_replicate(q, BLOCK), torch.as_tensor(q_off).long(), BLOCK)
    ks = O.sample_tokens(O.pad_replicate(k, BLOCK), torch.as_tensor(k_off).long(), BLOCK)
    return qs, ks


def qk_scale(D, scale=None):
    """fp32(scale) * fp32(1.44269504), as the max kernel forms it; scale None or <= 0 -> D^-1/2."""
    if scale is None or scale <= 0:
        scale = np.float32(1.0 / math.sqrt(D))
    return float(np.float32(scale) * np.float32(O.LOG2E))


def probabilities(qs, ks, scale=None, dtype=torch.float64):
    """The softmax of every sampled query over the sampled keys, [B,H,R,C], in base 2 on scaled scores."""
    s = torch.matmul(qs.to(dtype), ks.to(dtype).transpose(-1, -2)) * qk_scale(qs.shape[-1], scale)
    e = torch.exp2(s - s.amax(dim=-1, keepdim=True))
    return e, e.sum(dim=-1, keepdim=True)


def block_mass(qs, ks, scale=None, keep=KEEP, dtype=torch.float64):
    """mass [B,H,nq,nb]: sum over the queries of q-block i of (1/l_r) * the sum over the keys of key
    block j of exp2(s - M_r). ``qs`` may hold the sampled queries of a subset of the q-blocks (a query's
    softmax does not depend on the other queries): nq = qs rows / keep, nb = ks rows / keep."""
    B, H, R, _ = qs.shape
    nq, nb = R // keep, ks.shape[2] // keep
    e, l = probabilities(qs, ks, scale, dtype)
    per_query = e.view(B, H, R, nb, keep).sum(dim=-1) * (1.0 / l)          # [B,H,R,nb]
    return per_query.view(B, H, nq, keep, nb).sum(dim=3)


def po_of(mass, store_dtype):
    """mass / its row sum, rounded to the storage dtype."""
    return (mass / mass.sum(dim=-1, keepdim=True)).to(store_dtype)


def mass_scores(q, k, q_off, k_off, rows=None, scale=None, dtype=torch.float64):
    """(po in q.dtype, mass in ``dtype``) of caller tensors q, k [B,H,L,D]."""
    qs, ks = sampled_streams(q, k, q_off, k_off, rows)
    mass = block_mass(qs, ks, scale, q_off.shape[-1], dtype)
    return po_of(mass, q.dtype), mass


def brute_force_mass(qs, ks, scale=None, keep=KEEP):
    """The same quantity by torch.softmax over natural-log scores in float64, with explicit loops over
    the blocks: the check of block_mass itself."""
    B, H, R, D = qs.shape
    nb = R // keep
    # the fp32 qk_scale is part of the semantics; exp2(x) = exp(x * ln 2)
    sc = qk_scale(D, scale) * math.log(2.0)
    p = torch.softmax(torch.matmul(qs.double(), ks.double().transpose(-1, -2)) * sc, dim=-1)
    out = torch.zeros(B, H, nb, nb, dtype=torch.float64)
    for i in range(nb):
        for j in range(nb):
            out[:, :, i, j] = p[:, :, i * keep:(i + 1) * keep, j * keep:(j + 1) * keep].sum(dim=(-1, -2))
    return out


def small_grid_case(H=4, D=64, grid=(32, 20, 10), seed=0, probes=30):
    """The inputs of the motivating comparison: bench.local_qkv's generator on a small latent grid (CPU
    generators), the Gilbert order of that grid, one draw of q and k offsets and ``probes`` probe
    positions. Returns (q, k, rows, q_off, k_off, pos) with q, k bf16 [1,H,L,D] in caller order."""
    import bench
    import gilbert_oracle as G
    W, Hh, T = grid
    had = bench.LATENT_GRID.get("small")
    bench.LATENT_GRID["small"] = (W, Hh, T, 0)
    try:
        q, k, _ = bench.local_qkv("small", H, D, seed, "cpu")
    finally:
        if had is None:
            del bench.LATENT_GRID["small"]
        else:
            bench.LATENT_GRID["small"] = had
    rows = G.full_sequence_perm(W, Hh, T, 0)
    g = torch.Generator().manual_seed(seed)
    q_off = O.draw_sample_offsets(1, H, generator=g)
    k_off = O.draw_sample_offsets(1, H, generator=g)
    pos = torch.randperm(W * Hh * T, generator=g)[:probes].numpy()
    return q, k, rows, q_off, k_off, pos


def topk_mask(po, n):
    """bool [..., nb]: the n largest entries of each row (ties to the lower index)."""
    order = po.double().sort(dim=-1, descending=True, stable=True)[1]
    out = torch.zeros(po.shape, dtype=torch.bool)
    out.scatter_(-1, order[..., :n], True)
    return out
