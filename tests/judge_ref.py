"""Test helper: torch/numpy restatement of the head-budget path (include/vblade.h, vb_judge_sparsity
and vb_head_budget).

``judge`` is the reference's judge_sparsity (TrainRelated/blocksparseattn.py:147-160) with the index
draw, the key stride and the top fraction as arguments, evaluated in a chosen dtype: the tensors' own
(every eager op rounds to bf16/fp16, as the reference runs it) or float64 (the yardstick). It also
returns each row's top-n mass; averaged by rank and then summed (the reference) equals the mean over
rows of those masses. ``head_budget`` is the budget rule in the exact arithmetic the header states,
so the kernel can be compared bit for bit."""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def to_bits(x: torch.Tensor) -> np.ndarray:
    """bf16/fp16 tensor -> its 16-bit patterns."""
    return x.contiguous().view(torch.int16).numpy().view(np.uint16)


def from_bits(bits: np.ndarray, dt: str) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(DTYPES[dt])


def top_n_of(L: int, key_stride: int = 3, top: float = 0.2):
    n = (L + key_stride - 1) // key_stride
    return n, int(n * top)


def judge(q, k, rows, key_stride=3, top=0.2, dtype=None, scale=None):
    """(sparsity [B,H], row_mass [B,H,S]) as float64 numpy arrays; q,k CPU tensors [B,H,L,D]; ``dtype``
    None evaluates in q's own dtype, the reference's chain of eager ops."""
    if dtype is not None:
        q, k = q.to(dtype), k.to(dtype)
    idx = torch.as_tensor(np.asarray(rows), dtype=torch.long)
    scale = 1.0 / (q.size(-1) ** 0.5) if scale is None else scale
    qs = q[:, :, idx]
    ks = k[:, :, ::key_stride]
    out = torch.matmul(qs, ks.transpose(-2, -1)) * scale
    out = out - out.max(dim=-1, keepdim=True)[0]
    attn = torch.softmax(out, dim=-1)
    srt = attn.sort(dim=-1, descending=True)[0]
    top_n = int(ks.size(-2) * top)
    sparsity = srt.mean(dim=-2)[:, :, :top_n].sum(dim=-1)
    row_mass = srt[..., :top_n].sum(dim=-1)
    return sparsity.double().numpy(), row_mass.double().numpy()


def head_budget(sparsity, nb, base, clamp=(0.05, 0.9), variant="cog"):
    """(max_keep int32 [B,H], ratio float64 [B,H]) from fp32 sparsity [B,H]."""
    s = np.asarray(sparsity, dtype=np.float32).astype(np.float64)
    m = s.sum() / s.size
    ratio = np.minimum(np.maximum(np.float64(base) * (s / m), np.float64(clamp[0])), np.float64(clamp[1]))
    if variant == "cog":
        cnt = (np.float32(nb) * ratio.astype(np.float32)).astype(np.int32)
    else:
        cnt = (np.float64(nb) * ratio).astype(np.int32)
    return np.maximum(cnt, 1).astype(np.int32), ratio
