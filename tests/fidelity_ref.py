"""Test helper: plain-torch restatement of the output-fidelity probe (include/vblade.h,
vb_attn_fidelity), written from the header's semantics and independently of the kernel: one dense
score matrix of the probe queries against every key in caller order, one softmax, one product with
V, no chunks. ``dtype`` float64 is the yardstick, float32 the eager evaluation whose own error
against float64 sizes the tests' bounds."""
import math

import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
CHUNK = 512   # VB_FIDELITY_CHUNK: only the workspace formula needs it here


def qk_scale(D, scale=None):
    """fp32(scale) * fp32(1.44269504), the factor the kernel multiplies a dot product with."""
    s = np.float32(1.0 / math.sqrt(D)) if scale is None or scale <= 0 else np.float32(scale)
    return float(s * np.float32(1.44269504))


def workspace_bytes(B, H, L, D, S):
    nc = (L + CHUNK - 1) // CHUNK
    return (4 * (B * H * S * nc * (D + 2) + 3 * B * H * S) + 15) // 16 * 16


def dense_rows(q, k, v, probe_rows, scale=None, dtype=torch.float64):
    """(ref [B,H,S,D], row_lse [B,H,S]) in ``dtype``: dense attention of the probe rows (clamped to
    [0, L-1]) over all L keys; row_lse = ln(l) + m ln 2 with m the row's largest base-2 score."""
    B, H, L, D = q.shape
    g = torch.as_tensor(np.asarray(probe_rows), dtype=torch.long).clamp(0, L - 1)
    t = torch.matmul(q[:, :, g].to(dtype), k.to(dtype).transpose(-2, -1)) * qk_scale(D, scale)   # [B,H,S,L]
    m = t.max(dim=-1, keepdim=True)[0]
    e = torch.exp2(t - m)
    l = e.sum(dim=-1, keepdim=True)
    ref = torch.matmul(e, v.to(dtype)) / l
    return ref, (torch.log(l) + m * math.log(2.0)).squeeze(-1)


def _serial_sum(x):
    acc = torch.zeros(x.shape[:-1], dtype=x.dtype)
    for r in range(x.shape[-1]):
        acc = acc + x[..., r]
    return acc


def fidelity(q, k, v, out, probe_rows, scale=None, dtype=torch.float64):
    """dict of numpy arrays in ``dtype``: ref [B,H,S,D]; row_err, row_sig, row_lse [B,H,S]; err, sig,
    peak [B,H]. q, k, v, out CPU tensors [B,H,L,D]."""
    L = q.shape[2]
    g = torch.as_tensor(np.asarray(probe_rows), dtype=torch.long).clamp(0, L - 1)
    ref, lse = dense_rows(q, k, v, probe_rows, scale, dtype)
    diff = out[:, :, g].to(dtype) - ref
    row_err, row_sig = (diff * diff).sum(dim=-1), (ref * ref).sum(dim=-1)
    return dict(ref=ref.numpy(), row_lse=lse.numpy(), row_err=row_err.numpy(), row_sig=row_sig.numpy(),
                err=_serial_sum(row_err).numpy(), sig=_serial_sum(row_sig).numpy(),
                peak=ref.abs().amax(dim=(-2, -1)).numpy())
