"""Generate tests/golden/judge_sparsity.npz: the REFERENCE's own judge_sparsity
(TrainRelated/blocksparseattn.py:147-160) on small inputs. Run from the repo root:

    python tests/golden/make_golden_judge.py

Reads the reference checkout like make_golden.py (present only in the build container). Before each
call the module globals width, height, text_length and sample_num are set and the generator is
re-seeded, so the function's torch.randperm draw can be replayed and stored. The fixture holds arrays
only, per case <tag>:
    <tag>_q, <tag>_k      [B,H,L,D] as 16-bit patterns of the storage dtype
    <tag>_idx             the sampled rows (randperm(width*height)[:sample_num] + text_length)
    <tag>_ref16/32/64     the reference's result [B,H] on the 16-bit inputs, on their fp32 copies and
                          on their float64 copies
<tag> = <dtype>_<width>x<height>x<depth>_<text>_<D>_<sample_num>."""
import os
import sys

import numpy as np
import torch

import make_golden as MG  # same directory: the reference import helpers

sys.path.insert(0, os.path.dirname(MG.HERE))
import judge_ref as J  # noqa: E402  (tests/judge_ref.py)

# (dtype, width, height, depth, text_length, B, H, D, sample_num, seed)
CASES = [
    ("bf16", 12, 9, 4, 3, 1, 2, 64, 30, 11),
    ("fp16", 10, 8, 3, 0, 1, 2, 128, 7, 12),
    ("bf16", 16, 12, 2, 26, 1, 2, 64, 30, 13),
]


def main():
    MG._install_block_sparse_stub()
    ref, _ = MG._import_ref(MG.COG_TRAIN, "blocksparseattn")
    res = {}
    for dtn, w, h, d, text, B, H, D, S, seed in CASES:
        L = w * h * d + text
        g = torch.Generator().manual_seed(seed)
        temp = torch.linspace(0.7, 3.0, H).view(1, H, 1, 1)   # heads of different concentration
        q = (torch.randn(B, H, L, D, generator=g) * temp).to(J.DTYPES[dtn])
        k = torch.randn(B, H, L, D, generator=g).to(J.DTYPES[dtn])
        ref.width, ref.height, ref.text_length, ref.sample_num = w, h, text, S
        out = {}
        for name, cast in (("ref16", lambda x: x), ("ref32", torch.Tensor.float), ("ref64", torch.Tensor.double)):
            torch.manual_seed(seed)
            out[name] = ref.judge_sparsity(cast(q), cast(k)).double().numpy()
        torch.manual_seed(seed)
        idx = torch.randperm(w * h)[:S] + text
        tag = f"{dtn}_{w}x{h}x{d}_{text}_{D}_{S}"
        res[tag + "_q"], res[tag + "_k"] = J.to_bits(q), J.to_bits(k)
        res[tag + "_idx"] = idx.numpy().astype(np.int32)
        for name, v in out.items():
            res[f"{tag}_{name}"] = v
        # the replayed draw is the one the function used
        mine, _ = J.judge(q, k, idx.numpy(), dtype=torch.float64)
        assert np.abs(mine - out["ref64"]).max() < 1e-12, tag
        print(tag, "L", L, "ref64", out["ref64"].round(4).tolist(),
              "|ref32-ref64|", np.abs(out["ref32"] - out["ref64"]).max(),
              "|ref16-ref64|", np.abs(out["ref16"] - out["ref64"]).max())
    path = os.path.join(MG.HERE, "judge_sparsity.npz")
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    assert size < 1 << 20, f"{path}: {size} bytes"
    print(path, size, "bytes")


if __name__ == "__main__":
    main()
