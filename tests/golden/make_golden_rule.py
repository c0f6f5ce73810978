"""Generate tests/golden/mask_rule.npz: the REFERENCE's transfer_attn_to_mask in mode="topk" (both
reference modules, bf16 and fp16) and in mode="energy" with non-uniform [B,H] ratio tensors (the
CogVideoX module), on given scores. Run from the repo root:

    python tests/golden/make_golden_rule.py

Reads the reference checkout like make_golden.py (present only in the build container); the fixture
holds arrays only: scores as 16-bit patterns of their storage dtype, the reference masks, the ratio
tensors. Key scheme (tests/test_mask_rule.py reads it back from the key list):
    topk_<dtype>_<nb>_<k0>_{po,mask_cog,mask_wan}       tie-free rows, B=2, H=3
    topkties_<dtype>_<nb>_<k0>_{po,mask_cog,mask_wan}   tie-heavy rows (gen_energy_masks' mixture)
    energy_<dtype>_<nb>_{po,min_ratio,max_ratio,mask_cog}
The generator asserts its own conditions: finite values, strictly distinct values in every tie-free
row, and each outcome of the top-k rule (stay, grow, shrink, k = 0) somewhere in the fixture."""
import os
import sys

import numpy as np
import torch

import make_golden as MG  # same directory: the reference import helpers

sys.path.insert(0, os.path.dirname(MG.HERE))
import rule_ref as R  # noqa: E402  (tests/rule_ref.py: the numpy restatement)

TOPK_CASES = [(3, 2), (5, 1), (20, 5), (20, 8), (67, 13), (65, 64)]   # (nb, k0)
TIE_CASE = (139, 13)
B, H = 2, 3


def _fresh(mod):
    # the reference caches a weight map sized by its first call
    if hasattr(mod.transfer_attn_to_mask, "fix_weight"):
        del mod.transfer_attn_to_mask.fix_weight


def _normalise(po, dt):
    po = po.to(dt)
    return (po.float() / po.float().sum(-1, keepdim=True).to(dt).float()).to(dt)


def tie_free(nb, seed, dtn):
    """Rows that are a random permutation of r**i with a per-row r, normalised like the predictor's
    rows. fp16 underflows to equal zeros for small r on long rows: the lower end of r keeps the
    smallest value r**(nb-1) * (1-r) a normal fp16 number."""
    dt = R.DTYPES[dtn]
    g = torch.Generator().manual_seed(seed)
    r_lo = 0.3 if dtn == "bf16" else max(0.3, 1e-3 ** (1.0 / max(nb - 1, 1)))
    r = r_lo + (0.97 - r_lo) * torch.rand(B, H, nb, 1, generator=g)
    base = r ** torch.arange(nb).view(1, 1, 1, nb)
    perm = torch.rand(B, H, nb, nb, generator=g).argsort(-1)
    po = _normalise(base.gather(-1, perm), dt)
    srt = po.float().sort(-1).values
    assert torch.isfinite(po.float()).all(), (dtn, nb)
    assert (srt[..., 1:] > srt[..., :-1]).all(), f"ties in a tie-free case ({dtn}, nb={nb})"
    return po


def tie_heavy(b, h, nb, seed, dtn):
    """gen_energy_masks' mixture: smooth random rows and rows with many equal maxima."""
    dt = R.DTYPES[dtn]
    g = torch.Generator().manual_seed(seed)
    po = torch.rand(b, h, nb, nb, generator=g) ** 4
    ties = (torch.rand(b, h, nb, nb, generator=g) < 0.15).float()
    po = torch.where(torch.rand(b, h, nb, 1, generator=g) < 0.5, po, torch.maximum(po, ties))
    po = _normalise(po, dt)
    assert torch.isfinite(po.float()).all()
    return po


def main():
    MG._install_block_sparse_stub()
    cog, _ = MG._import_ref(MG.COG_TRAIN, "cogvideo_blocksparseattn")
    wan, _ = MG._import_ref(MG.WAN_TRAIN, "wanx_blocksparseattn")
    res = {}
    seen = dict(stay=0, grow=0, shrink=0, zero=0)

    def topk_case(tag, po, k0, dtn):
        res[tag + "_po"] = R.to_bits(po.float().numpy(), dtn)
        for name, mod in (("cog", cog), ("wan", wan)):
            _fresh(mod)
            m = mod.transfer_attn_to_mask(po.clone(), mode="topk", init_k=k0)
            res[f"{tag}_mask_{name}"] = m.numpy()
        kk = R.topk_counts(po.float().numpy(), k0, dtn)
        seen["stay"] += int((kk == k0).sum())
        seen["grow"] += int((kk > k0).sum())
        seen["shrink"] += int(((kk < k0) & (kk > 0)).sum())
        seen["zero"] += int((kk == 0).sum())
        print(tag, tuple(po.shape), "k:", sorted(set(kk.flatten().tolist())))

    for dtn in R.DTYPES:
        for nb, k0 in TOPK_CASES:
            topk_case(f"topk_{dtn}_{nb}_{k0}", tie_free(nb, nb * 10 + k0, dtn), k0, dtn)
    nb, k0 = TIE_CASE
    topk_case(f"topkties_bf16_{nb}_{k0}", tie_heavy(1, 2, nb, 17, "bf16"), k0, "bf16")
    assert all(seen.values()), f"an outcome of the top-k rule is missing from the fixture: {seen}"

    # energy mode, ratios per (batch, head) (cogvideo_blocksparseattn.py:230-231)
    mx = torch.tensor([[0.7, 0.5, 0.3, 0.9], [0.2, 0.7, 0.05, 0.6]])
    mn = torch.tensor([[0.1, 0.2, 0.05, 0.5], [0.1, 0.0, 0.02, 0.3]])
    for dtn, dt in R.DTYPES.items():
        g = torch.Generator().manual_seed(7)
        sharp = torch.tensor([1.0, 4.0, 12.0, 40.0]).view(1, 4, 1, 1)
        po = _normalise(torch.rand(2, 4, 67, 67, generator=g) ** sharp, dt)
        assert torch.isfinite(po.float()).all()
        _fresh(cog)
        m = cog.transfer_attn_to_mask(po.clone(), mode="energy", max_retain_ratio=mx,
                                      min_retain_ratio=mn, energy_threshold=0.95)
        tag = f"energy_{dtn}_67"
        res[tag + "_po"] = R.to_bits(po.float().numpy(), dtn)
        res[tag + "_min_ratio"], res[tag + "_max_ratio"] = mn.numpy(), mx.numpy()
        res[tag + "_mask_cog"] = m.numpy()
        print(tag, tuple(po.shape))
    out = os.path.join(MG.HERE, "mask_rule.npz")
    np.savez_compressed(out, **res)
    size = os.path.getsize(out)
    assert size < 1 << 20, f"{out}: {size} bytes"
    print(out, size, "bytes; outcomes", seen)


if __name__ == "__main__":
    main()
