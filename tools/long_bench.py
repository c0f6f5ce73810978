#!/usr/bin/env python3
"""Timings of the adaptive module past 320 blocks (vb_mask_predict_long), device events on one GPU.
usage: python tools/long_bench.py [--width 80 --height 45 --depth 21] [--heads 12] [--reps 10]
Default: Wan2.1 at 720p (80x45x21 latents, L = 75600, 591 blocks), H = 12, D = 128, bf16.
Prints, per line: the predictor launch as the module issues it (pooled K/V pass riding, kept counts),
the predictor with and without its energy rule (the difference is the rank + cumulative-sum
epilogue), the attention launch, the whole inner_attention call and dense bf16 SDPA on the same
inputs."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-blade_amd"))
sys.path.insert(0, ROOT)
import vblade  # noqa: E402
from vblade import ops  # noqa: E402
from vblade.attention import retain_counts  # noqa: E402
from bench import attn_flops, realistic_qkv  # noqa: E402


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=80)
    ap.add_argument("--height", type=int, default=45)
    ap.add_argument("--depth", type=int, default=21)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3, help="times the whole set is measured (spread)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    m = vblade.AdaptiveBlockSparseAttn("wan", width=a.width, height=a.height, depth=a.depth, log_every=0)
    H, D, L = a.heads, 128, m.gilbert_rearranger.seq_len
    nb = (L + 127) // 128
    q, k, v = realistic_qkv(H, L, D, 0, dev)
    rows = m._rows(dev)
    qo = vblade.draw_sample_offsets(1, H, dev)
    ko = vblade.draw_sample_offsets(1, H, dev)
    lo, hi = retain_counts(nb, m.min_retain_ratio, m.max_retain_ratio, "wan")
    kw = dict(rows=rows, min_keep=lo, max_keep=hi, force_tail=0, long_rows=nb > ops.MAX_BLOCKS)
    print(f"L={L} nb={nb} H={H} D={D} keep=[{lo},{hi}]", flush=True)
    with torch.no_grad():
        kept = torch.empty(1, H, nb, device=dev, dtype=torch.int32)
        _, mask = ops.mask_predict(q, k, qo, ko, rows_kept=kept, **kw)
        kp, vp = ops.pool_kv(k, v, m.sample_gap, rows)
        outs = ops.pool_kv_outputs(k, m.sample_gap)
        fl = attn_flops(mask, L, D, kp.shape[2])
        print(f"mask density {mask.float().mean().item():.4f}", flush=True)
        for it in range(a.repeat):
            t_mod = timeit(lambda: ops.mask_predict(q, k, qo, ko, pool=(v, m.sample_gap, outs), rows_kept=kept, **kw), a.reps)
            t_mask = timeit(lambda: ops.mask_predict(q, k, qo, ko, **kw), a.reps)
            t_score = timeit(lambda: ops.mask_predict(q, k, qo, ko, want_mask=False, **kw), a.reps)
            t_attn = timeit(lambda: ops.attention_fwd(q, k, v, block_mask=mask, q_rows=rows, kv_rows=rows, kp=kp, vp=vp,
                                                      kp_log_bias=m._log_gap(q.dtype), order=m.order,
                                                      q_lengths=kept), a.reps)
            t_call = timeit(lambda: m(q, k, v), a.reps)
            t_dense = timeit(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v), 3)
            print(f"run {it}: predictor (module form) {t_mod:.3f} ms | predictor scores+mask {t_mask:.3f} ms, "
                  f"scores only {t_score:.3f} ms, energy rule {t_mask - t_score:.3f} ms "
                  f"({100 * (t_mask - t_score) / t_mask:.1f} % of the launch) | attention {t_attn:.3f} ms "
                  f"({fl / t_attn / 1e9:.0f} TF/s) | call {t_call:.3f} ms (predictor share "
                  f"{100 * t_mod / t_call:.1f} %) | dense SDPA {t_dense:.3f} ms ({t_dense / t_call:.2f}x the call)",
                  flush=True)


if __name__ == "__main__":
    main()
