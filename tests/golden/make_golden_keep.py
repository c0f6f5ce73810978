"""Generate tests/golden/pooled_scores_keep.npz: the REFERENCE's Triton pooled-score kernel run at
tile sizes 16 and 64 (the predictor's num_keep) under the Triton interpreter, as
make_golden.py's gen_pooled_scores does at tile 32. Run from the repo root:

    TRITON_INTERPRET=1 python tests/golden/make_golden_keep.py

Reads the reference checkout like make_golden.py (present only in the build container); the fixture
holds arrays only (inputs, expected scores, the dtype's name)."""
import os

os.environ.setdefault("TRITON_INTERPRET", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import make_golden as MG  # noqa: E402  (same directory: the reference import helpers)

KEEPS = (16, 64)
# (name, dtype, B, H, nb, D): D = 64 and 128, fp32 and fp16, nb of 5 and 11. One (b,h) each and the
# inputs stored as fp16 (the fp32 cases' inputs are rounded to fp16 values first, then computed in
# fp32): random inputs do not compress, and the fixture has to stay a small file.
CASES = [("f32_d64", torch.float32, 1, 1, 11, 64), ("f16_d64", torch.float16, 1, 1, 5, 64),
         ("f32_d128", torch.float32, 1, 1, 5, 128), ("f16_d128", torch.float16, 1, 1, 5, 128)]


def gen_pooled_scores_keep(out, apk):
    res = {}
    for keep in KEEPS:
        for name, dt, B, H, nb, D in CASES:
            tag = f"k{keep}_{name}"
            g = torch.Generator().manual_seed(sum(map(ord, tag)))
            # block-structured scores so the rows are not all ties
            qs = torch.randn(B, H, nb * keep, D, generator=g)
            ks = torch.randn(B, H, nb * keep, D, generator=g)
            cent = torch.randn(B, H, nb, D, generator=g) * 1.5
            qs = (qs + cent.repeat_interleave(keep, 2)).half().to(dt)
            ks = (ks + cent.repeat_interleave(keep, 2)).half().to(dt)
            v = torch.zeros_like(qs)
            _, po = apk.attn_with_pooling(qs, ks, v, False, 1.0 / (D ** 0.5), keep)
            res[tag + "_q"] = qs.numpy().astype(np.float16)
            res[tag + "_k"] = ks.numpy().astype(np.float16)
            res[tag + "_po"] = po.float().numpy()
            res[tag + "_dtype"] = np.array(str(dt))
            print(tag, tuple(po.shape))
    np.savez_compressed(os.path.join(out, "pooled_scores_keep.npz"), **res)


def main():
    MG._install_block_sparse_stub()
    _, apk = MG._import_ref(MG.COG_TRAIN, "cogvideo_blocksparseattn")
    gen_pooled_scores_keep(MG.HERE, apk)


if __name__ == "__main__":
    main()
