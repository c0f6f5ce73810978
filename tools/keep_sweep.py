#!/usr/bin/env python3
"""Sampling-density sweep of the mask predictor: num_keep 16 / 32 / 64 on the CogVideoX and Wan
headline shapes, in ONE process on ONE GPU, on bench.py's locality-faithful inputs (local_qkv).
Timing as tools/ab.py: the densities interleaved round by round (16, 32, 64, 16, ...), 5 calls
between an event pair, the median over the rounds; a second keep-32 module gives the A/A spread.

Per density: the predictor's launches as the module issues them (sampling + score launch with the
pooled K/V pass riding in it) and without the pooled pass, the whole module call and its ratio to
keep 32, the kept-block fraction, the share of mask entries equal to the keep-32 mask under the same
seed (the same 128 uniforms per (b,h): the top 16 are a prefix of the top 32), and the PSNR of the
module output against dense SDPA on the same inputs.

--recall appends, per density, the attention recall of its mask and the oracle recall of its budget
(ops.mask_recall on the same q, k and mask: 30 probe queries per head, the module option's own
positions; mean and smallest head), and one more module, keep 32 with probe="recall", whose call time
against keep 32 is what the option costs. The other columns are computed as without the flag.

--fidelity appends, per density, what ops.attn_fidelity measures on its own output (30 probe queries per
head, the module option's own rows): the SNR against exact dense rows over all heads (and the smallest
head's) and a sampled PSNR, 10 log10(peak^2 S D H / sum err), to be read against the full-tensor PSNR
column; and two more modules: keep 32 with probe="fidelity", whose call time against keep 32 is what the
option costs, and the multi-level (VBench) module at keep 32 (no predictor-only columns).

usage: python tools/keep_sweep.py [--variant cog|wan|both] [--rounds 15] [--recall] [--fidelity] [--out FILE.json]"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-blade_amd"))
sys.path.insert(0, ROOT)
import vblade  # noqa: E402
from vblade import multilevel, ops  # noqa: E402
from vblade.attention import VARIANT_DEFAULTS  # noqa: E402
from bench import local_qkv  # noqa: E402

KEEPS = (16, 32, 64)
SEED = 1234


def psnr(x, ref):
    mse = torch.mean((x.double() - ref.double()) ** 2).item()
    peak = ref.double().abs().max().item()
    return 99.0 if mse == 0 else 10 * math.log10(peak * peak / mse)


def timed(fn, reps=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def recall_of(m, q, k, pos):
    """Recall and oracle recall of the module's last mask as its attention launch read it."""
    mask = m.last_mask
    if m.mask_head_mode == "shared_head0":
        mask = mask[:, :1].expand_as(mask)
    rec, ora = ops.mask_recall(q, k, mask, pos, rows=m._rows(q.device))
    return {"recall_mean": rec.mean().item(), "recall_min_head": rec.min().item(),
            "oracle_recall_mean": ora.mean().item(), "oracle_recall_min_head": ora.min().item()}


def fidelity_of(q, k, v, out, prows):
    """SNR (all heads, smallest head) and the sampled PSNR of an output, from ops.attn_fidelity."""
    err, sig, peak = (t.double() for t in ops.attn_fidelity(q, k, v, out, prows))
    S, D = prows.numel(), q.shape[-1]
    snr = ops.fidelity_snr_db(err, sig)
    return {"fidelity_snr_db": 10 * math.log10(sig.sum().item() / max(err.sum().item(), 1e-300)),
            "fidelity_snr_min_head_db": snr.min().item(),
            "fidelity_sampled_psnr_db": 10 * math.log10(peak.max().item() ** 2 * S * D * err.numel()
                                                        / max(err.sum().item(), 1e-300))}


MULTILEVEL = "ml/32"


def sweep(variant, rounds, dev, recall=False, fidelity=False):
    H, D = (48, 64) if variant == "cog" else (12, 128)
    q, k, v = local_qkv(variant, H, D, 0, dev)
    L = q.shape[2]
    # labels: the three densities and a second keep-32 module (the A/A spread of every column)
    mods = {str(kp): vblade.AdaptiveBlockSparseAttn(variant, log_every=0, num_keep=kp) for kp in KEEPS}
    mods["32#aa"] = vblade.AdaptiveBlockSparseAttn(variant, log_every=0, num_keep=32)
    pos = None
    if recall:
        mods["32+probe"] = vblade.AdaptiveBlockSparseAttn(variant, log_every=0, num_keep=32, probe="recall")
        pos = mods["32+probe"].probe_pos.to(dev)
    prows = None
    if fidelity:
        mods["32+fid"] = vblade.AdaptiveBlockSparseAttn(variant, log_every=0, num_keep=32, probe="fidelity")
        prows = mods["32+fid"].probe_rows.to(dev)
        grid = {n: VARIANT_DEFAULTS[variant][n] for n in ("width", "height", "depth", "text_length")}
        mods[MULTILEVEL] = multilevel.AdaptiveBlockSparseAttnTrain(log_every=0, num_keep=32, **grid)
    dense = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    res, masks = {}, {}

    def fns(m):
        if isinstance(m, multilevel.AdaptiveBlockSparseAttnTrain):
            def ml_call():
                torch.cuda.manual_seed(SEED)
                return m(q, k, v)
            return {"call_ms": ml_call}
        copies = not (m._gather(D) and m._rows(dev) is not None)
        outs = ops.pool_kv_outputs(k, m.sample_gap, reordered=copies)

        def pred_fused():
            torch.cuda.manual_seed(SEED)
            return m.predict_mask(q, k, pool=(v, m.sample_gap, outs))

        def pred_scores():
            torch.cuda.manual_seed(SEED)
            return m.predict_mask(q, k)

        def call():
            torch.cuda.manual_seed(SEED)
            return m(q, k, v)
        return {"pred_fused_ms": pred_fused, "pred_scores_ms": pred_scores, "call_ms": call}

    with torch.no_grad():
        work = {lab: fns(m) for lab, m in mods.items()}
        for lab, m in mods.items():   # warm up; quality figures from this call
            out = work[lab]["call_ms"]()
            torch.cuda.synchronize()
            mask = m.last_mask.clone()
            masks[lab] = mask
            kept = multilevel.density(m.mask_ratios) if lab == MULTILEVEL else mask.float().mean().item()
            res[lab] = {"num_keep": m.num_keep, "kept_fraction": kept,
                        "psnr_vs_dense_db": psnr(out, dense)}
            if recall and lab != MULTILEVEL:
                res[lab].update(recall_of(m, q, k, pos))
            if fidelity:
                res[lab].update(fidelity_of(q, k, v, out, prows))
            for f in ("pred_fused_ms", "pred_scores_ms"):
                if f in work[lab]:
                    work[lab][f]()
        times = {lab: {f: [] for f in work[lab]} for lab in mods}
        for _ in range(rounds):
            for f in ("pred_fused_ms", "pred_scores_ms", "call_ms"):
                for lab in mods:
                    if f in work[lab]:
                        times[lab][f].append(timed(work[lab][f]))
    for lab in mods:
        for f, ts in times[lab].items():
            res[lab][f] = statistics.median(ts)
            res[lab][f + "_min"] = min(ts)
        if lab != MULTILEVEL:   # a level mask is graded 0/1/2/4/8: not comparable entry by entry
            res[lab]["mask_equal_to_keep32"] = (masks[lab] == masks["32"]).float().mean().item()
    for lab in mods:
        for f in ("pred_fused_ms", "pred_scores_ms", "call_ms"):
            if f in res[lab]:
                res[lab][f.replace("_ms", "_vs_keep32")] = res[lab][f] / res["32"][f]
    return {"variant": variant, "B": 1, "H": H, "L": L, "D": D, "nb": (L + 127) // 128,
            "inputs": "bench.local_qkv(seed 0)", "rounds": rounds, "calls_per_round": 5, "densities": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="both")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--fidelity", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    out = {"device": torch.cuda.get_device_name(0), "results": []}
    for variant in (["cog", "wan"] if a.variant == "both" else [a.variant]):
        r = sweep(variant, a.rounds, dev, a.recall, a.fidelity)
        out["results"].append(r)
        print(f"{variant}: H={r['H']} L={r['L']} D={r['D']} ({r['nb']} blocks)")
        print("  keep | fused pred ms (x32) | scores-only ms (x32) | call ms (x32) | kept | == keep32 | PSNR dB"
              + (" | recall mean (min head) | oracle recall mean (min head)" if a.recall else "")
              + (" | fidelity SNR dB (min head) | sampled PSNR dB" if a.fidelity else ""))
        for lab, d in r["densities"].items():
            extra = ""
            if a.recall:
                extra = (f" | {d['recall_mean']:.4f} ({d['recall_min_head']:.4f}) | "
                         f"{d['oracle_recall_mean']:.4f} ({d['oracle_recall_min_head']:.4f})"
                         if "recall_mean" in d else " | - | -")
            if a.fidelity:
                extra += (f" | {d['fidelity_snr_db']:.2f} ({d['fidelity_snr_min_head_db']:.2f}) | "
                          f"{d['fidelity_sampled_psnr_db']:.2f}")
            pred = (f"{d['pred_fused_ms']:.4f} ({d['pred_fused_vs_keep32']:.3f}) | "
                    f"{d['pred_scores_ms']:.4f} ({d['pred_scores_vs_keep32']:.3f})" if "pred_fused_ms" in d else "- | -")
            same = f"{d['mask_equal_to_keep32']:.4f}" if "mask_equal_to_keep32" in d else "-"
            print(f"  {lab:>6} | {pred} | "
                  f"{d['call_ms']:.4f} ({d['call_vs_keep32']:.3f}) | {d['kept_fraction']:.4f} | "
                  f"{same} | {d['psnr_vs_dense_db']:.2f}{extra}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
