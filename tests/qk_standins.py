"""Stand-in attention modules for the q/k prologue tests (CPU and GPU files): the attributes the
processors of vblade/patch.py read from diffusers' Attention, with the real models' norms."""
import torch
import torch.nn as nn
import torch.nn.functional as F

SDPA = F.scaled_dot_product_attention


class StandInAttention(nn.Module):
    """The attributes the processors read from diffusers' Attention, with the real models' norms:
    nn.LayerNorm(head_dim) per head (CogVideoX) or nn.RMSNorm(dim) over the projection (Wan).
    inner_attention is SDPA and keeps the q/k it was handed."""

    def __init__(self, dim, heads, kind, i2v=False, norm_cls=None, seed=0):
        super().__init__()
        torch.manual_seed(seed)
        self.heads = heads
        self.to_q, self.to_k, self.to_v = (nn.Linear(dim, dim) for _ in range(3))
        if kind == "cog":
            cls = norm_cls or nn.LayerNorm
            self.norm_q, self.norm_k = cls(dim // heads, eps=1e-6), cls(dim // heads, eps=1e-6)
        else:
            cls = norm_cls or nn.RMSNorm
            self.norm_q, self.norm_k = cls(dim, eps=1e-6), cls(dim, eps=1e-6)
        with torch.no_grad():
            for n in (self.norm_q, self.norm_k):
                n.weight.add_(0.1 * torch.randn_like(n.weight))
                if getattr(n, "bias", None) is not None:
                    n.bias.add_(0.1 * torch.randn_like(n.bias))
        self.to_out = nn.ModuleList([nn.Linear(dim, dim), nn.Dropout(0.0)])
        self.is_cross_attention = False
        self.add_k_proj = nn.Linear(dim, dim) if i2v else None
        self.add_v_proj = nn.Linear(dim, dim) if i2v else None
        self.norm_added_k = nn.RMSNorm(dim) if i2v else None
        self.seen = []
        self.inner_attention = self._sdpa
        self.processor = "stock"

    def get_processor(self):
        return self.processor

    def set_processor(self, p):
        self.processor = p

    def _sdpa(self, q, k, v):
        self.seen.append((q.clone(), k.clone()))
        return SDPA(q, k, v)


class OtherLayerNorm(nn.LayerNorm):
    """A norm the processors cannot identify exactly."""


class OtherRMSNorm(nn.RMSNorm):
    pass
