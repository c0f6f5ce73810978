#!/usr/bin/env python3
"""The joint backward against the two-branch backward on EQUAL data.

ops.attention_bwd_joint runs the gradient kernels ops.attention_bwd runs, yet tools/ab.py --what bwd
measures it ~2 % slower on bench.py's inputs. The two-branch form's combine weight alpha is rounded to
the storage dtype: where a row's pooled mass is below 2^-9 it is exactly 1, storage(1 - alpha) is 0, and
that row's pooled probabilities are exactly 0 (L'2 = kBigL). The joint form keeps them.

usage: python tools/diag/joint_bwd_alpha.py cog|wan
Prints the share of rows with alpha == 1, and interleaved medians of: the two-branch backward, the same
with alpha capped below 1 (the pooled branch live on every row, as in the joint form; timing only, not a
gradient anyone wants), the joint backward, and the two-branch backward again (the run-to-run spread)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "video-blade_amd"))
sys.path.insert(0, ROOT)
import vblade  # noqa: E402
from vblade import ops  # noqa: E402
from bench import realistic_qkv  # noqa: E402


def main():
    variant = sys.argv[1]
    dev = torch.device("cuda")
    H, D = (48, 64) if variant == "cog" else (12, 128)
    m = vblade.AdaptiveBlockSparseAttn(variant, log_every=0)
    L = m.gilbert_rearranger.seq_len
    q, k, v = realistic_qkv(H, L, D, 0, dev)
    rows = m._rows(dev)
    qo, ko = vblade.draw_sample_offsets(1, H, dev), vblade.draw_sample_offsets(1, H, dev)
    with torch.no_grad():
        _, mask = m.predict_mask(q, k, qo, ko)
        kp, vp, k_r, v_r = ops.pool_kv(k, v, m.sample_gap, rows, reordered=True)
        do = torch.randn_like(q)
        gap, beta = m.sample_gap, m._log_gap(q.dtype)
        out1, lse1 = ops.attention_fwd(q, k_r, v_r, block_mask=mask, q_rows=rows, need_lse=True,
                                       heavy_rows=m.force_tail)
        out2, lse2 = ops.attention_fwd(q, None, None, use_main=False, q_rows=rows, kp=kp, vp=vp, need_lse=True)
        _, alpha = ops.lse_combine(out1, lse1, out2, lse2, gap)
        outj, lsej = ops.attention_fwd(q, k_r, v_r, block_mask=mask, q_rows=rows, kp=kp, vp=vp, kp_log_bias=beta,
                                       need_lse=True, heavy_rows=m.force_tail)
        print(variant, "rows with alpha == 1 (pooled branch dead in the two-branch backward):",
              float((alpha == 1).float().mean()))
        capped = alpha.clamp(max=1 - 2.0 ** -7)

        def two(a):
            return lambda: ops.attention_bwd(do, q, k_r, v_r, out1, lse1, block_mask=mask, q_rows=rows,
                                             kv_rows=rows, kp=kp, vp=vp, out2=out2, lse2=lse2, alpha=a, gap=gap,
                                             heavy_rows=m.force_tail)

        fns = {"two-branch": two(alpha), "two-branch alpha<1": two(capped),
               "joint": lambda: ops.attention_bwd_joint(do, q, k_r, v_r, outj, lsej, block_mask=mask, q_rows=rows,
                                                        kv_rows=rows, kp=kp, vp=vp, gap=gap, kp_log_bias=beta,
                                                        heavy_rows=m.force_tail),
               "two-branch again": two(alpha)}
        times = {n: [] for n in fns}
        for f in fns.values():
            f()
        torch.cuda.synchronize()
        for _ in range(15):
            for n, f in fns.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(5):
                    f()
                e1.record()
                torch.cuda.synchronize()
                times[n].append(e0.elapsed_time(e1) / 5)
    for n, t in times.items():
        print(f"{variant} {n}: median {statistics.median(t):.4f} ms (min {min(t):.4f})", flush=True)


if __name__ == "__main__":
    main()
