"""Test helper: plain-torch restatement of the attention-recall probe (include/vblade.h,
vb_mask_recall), written from the header's semantics and independently of the kernel: a dense score
matrix of the probe queries against the reordered keys, one softmax numerator per key, block masses
by a reshape, the oracle by a stable descending sort. ``dtype`` float64 is the yardstick, float32 the
eager evaluation whose own error against float64 sizes the tests' bound."""
import math

import numpy as np
import torch

BLOCK = 128
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def block_masses(q, k, probe_pos, rows=None, scale=None, dtype=torch.float64):
    """E [B,H,S,nb]: per probe query the softmax numerators exp(s_j - max_j s_j), summed per block of
    128 reordered keys. q,k CPU tensors [B,H,L,D]; probe_pos reordered positions (clamped to
    [0, L-1]); rows the reordered position -> caller row index, or None."""
    q, k = q.to(dtype), k.to(dtype)
    B, H, L, D = q.shape
    nb = (L + BLOCK - 1) // BLOCK
    g = torch.as_tensor(np.asarray(probe_pos), dtype=torch.long).clamp(0, L - 1)
    r = torch.arange(L) if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.long)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    s = torch.matmul(q[:, :, r[g]], k[:, :, r].transpose(-2, -1)) * scale          # [B,H,S,L]
    e = torch.exp2((s - s.max(dim=-1, keepdim=True)[0]) * math.log2(math.e))
    e = torch.nn.functional.pad(e, (0, nb * BLOCK - L))                           # absent keys hold no mass
    return e.view(B, H, g.numel(), nb, BLOCK).sum(dim=-1)


def from_masses(E, mask, probe_pos, L):
    """dict of numpy arrays from block masses E [B,H,S,nb] and a mask [B,H,>=nb,>=nb]: row_recall,
    row_oracle [B,H,S] and recall, oracle [B,H] in E's dtype; row_kept [B,H,S] int32."""
    B, H, S, nb = E.shape
    g = torch.as_tensor(np.asarray(probe_pos), dtype=torch.long).clamp(0, L - 1)
    mrow = torch.as_tensor(mask)[:, :, g // BLOCK, :nb] != 0                      # [B,H,S,nb]
    mrow = mrow.expand(B, H, S, nb)
    T = E.sum(dim=-1)
    K = (E * mrow.to(E.dtype)).sum(dim=-1)
    n = mrow.sum(dim=-1)
    # the n heaviest blocks (stable descending sort: ties to the lower index), summed where they lie
    order = E.sort(dim=-1, descending=True, stable=True)[1]
    rank = order.argsort(dim=-1)
    O = (E * (rank < n.unsqueeze(-1)).to(E.dtype)).sum(dim=-1)
    rr, ro = K / T, O / T
    return dict(row_recall=rr.numpy(), row_oracle=ro.numpy(), row_kept=n.to(torch.int32).numpy(),
                recall=rr.mean(dim=-1).numpy(), oracle=ro.mean(dim=-1).numpy())


def recall(q, k, mask, probe_pos, rows=None, scale=None, dtype=torch.float64):
    E = block_masses(q, k, probe_pos, rows, scale, dtype)
    return from_masses(E, mask, probe_pos, q.shape[2])


def top_mask_row(E, n):
    """bool [..., nb]: the n heaviest blocks of each row of E (ties to the lower index)."""
    order = E.sort(dim=-1, descending=True, stable=True)[1]
    out = torch.zeros(E.shape, dtype=torch.bool)
    out.scatter_(-1, order[..., :n], True)
    return out
