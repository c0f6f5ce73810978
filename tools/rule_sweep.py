#!/usr/bin/env python3
"""Mask-rule sweep of the adaptive module on the CogVideoX and Wan headline shapes, in ONE process on
ONE GPU, on bench.py's locality-faithful inputs (local_qkv). Timing as tools/keep_sweep.py: the
settings interleaved round by round, 5 calls between an event pair, the median over the rounds; a
second default module gives the A/A spread.

Settings: the default energy rule (scalar bounds: vb_mask_predict), the same rule with its bounds as
uniform per-head arrays (vb_mask_predict_rule: what the rule instantiation itself costs), top-k mode
at init_k 0.05 / 0.1 / 0.2, and one per-head budget set (the odd heads at half the default
max_retain_ratio), and the head-adaptive budget: `judge` (head_budget="judge": the estimator and
the budget rule before the predictor, every call) and `judge/clamp(r,r)` with r the default
max_retain_ratio, whose masks are those of `energy/uniform[H]`, so their difference in call time is
the estimator's pure overhead (call_vs_uniform). bench.local_qkv's heads are statistically alike, so
the estimator has nothing to find there: --head-temps LO HI scales q per head (linspace over the
heads), which gives the heads different concentrations. Per setting: the predictor's launches as the module issues them (pooled K/V pass
riding), the whole module call and its ratio to the default, the kept-block fraction, and the PSNR
of the module output against dense SDPA on the same inputs.

score=mass settings (ops.mask_scores_mass, the sampled softmax mass instead of the max proxy): `mass/energy`
(the default rule on the new score; its fused-predictor column is its three launches plus the pooled K/V
pass as a launch of its own, which is how the module runs it) and, at a budget EQUAL to the `energy`
run's, `max/top-n@energy` and `mass/top-n@energy`: the n best blocks of every row of either score's po
(n = the energy run's mean kept blocks per row, forced tail added), built with torch.topk and handed to
the module as block_mask=. Their time columns include that torch code and are not a product path; their
quality columns are what the score alone buys.

--recall appends, per setting, the attention recall of its mask and the oracle recall of its budget
(ops.mask_recall on the same q, k and mask: 30 probe queries per head, the module option's own
positions; mean and smallest head), and one more setting, `energy/probe=recall`, whose call time
against `energy` is what the option costs, beside `judge`'s. The other columns are computed as
without the flag.

--fidelity appends, per setting, what ops.attn_fidelity measures on the setting's own output (30 probe
queries per head, the module option's own rows): the SNR against exact dense rows over all heads (and the
smallest head's) and a sampled PSNR, 10 log10(peak^2 S D H / sum err) with the probe's own peak, to be read
against the full-tensor "PSNR dB" column; and two more settings: `energy/probe=fidelity`, whose call time
against `energy` is what the option costs (beside `energy/probe=recall` with --recall), and `multilevel`,
the multi-level (VBench) module on the same inputs (its predictor column is predict_level_mask with the
pyramid pass riding, its kept column the reported density).

usage: python tools/rule_sweep.py [--variant cog|wan|both] [--rounds 15] [--head-temps LO HI] [--recall] [--fidelity] [--out FILE.json]
       rocprofv3 --kernel-trace --stats -d DIR -o run --output-format csv -- python tools/rule_sweep.py --variant cog --one-call SETTING
       (four module calls of one setting and nothing else: a kernel trace then shows its launches
       per call, tools/kstats.py DIR)"""
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

SEED = 1234
INIT_KS = (0.05, 0.1, 0.2)


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


def settings(variant, H, recall=False, fidelity=False):
    d = VARIANT_DEFAULTS[variant]
    mk = lambda **kw: vblade.AdaptiveBlockSparseAttn(variant, log_every=0, **kw)  # noqa: E731
    mods = {"energy": mk(), "energy#aa": mk()}
    mods["energy/uniform[H]"] = mk(max_retain_ratio=torch.full((H,), d["max_retain_ratio"]),
                                   min_retain_ratio=torch.full((H,), d["min_retain_ratio"]),
                                   energy_threshold=torch.full((H,), 0.95))
    for ik in INIT_KS:
        mods[f"topk/{ik}"] = mk(mask_mode="topk", init_k=ik)
    half = torch.full((H,), d["max_retain_ratio"])
    half[1::2] *= 0.5
    mods["energy/odd heads at half max"] = mk(max_retain_ratio=half)
    mods["judge"] = mk(head_budget="judge")
    r = d["max_retain_ratio"]
    mods["judge/clamp(r,r)"] = mk(head_budget="judge", judge_clamp=(r, r))
    if recall:
        mods["energy/probe=recall"] = mk(probe="recall")
    if fidelity:
        mods["energy/probe=fidelity"] = mk(probe="fidelity")
        grid = {n: d[n] for n in ("width", "height", "depth", "text_length")}
        mods[MULTILEVEL] = multilevel.AdaptiveBlockSparseAttnTrain(log_every=0, **grid)
    mods["mass/energy"] = mk(score="mass")
    mods["mass/energy#aa"] = mk(score="mass")
    for lab, score in EQUAL_BUDGET.items():
        mods[lab] = mk(score=score)
    return mods


MULTILEVEL = "multilevel"
EQUAL_BUDGET = {"max/top-n@energy": "max", "mass/top-n@energy": "mass"}


def top_n_mask(m, q, k, n):
    """The n best blocks per row of the module's score (its own draws and sampled tokens), plus the forced tail."""
    B, H, L, _ = q.shape
    rows = m._rows(q.device)
    rq = torch.rand(B, H, 1, m.block, device=q.device)
    rk = torch.rand(B, H, 1, m.block, device=q.device)
    qo, ko = ops.sample_offsets(rq, rk, m.num_keep)
    qo, ko = qo[:, :, 0], ko[:, :, 0]
    if m.score == "mass":
        po = ops.mask_scores_mass(q, k, qo, ko, rows=rows)
    else:
        po = ops.mask_predict(q, k, qo, ko, rows=rows, want_mask=False,
                              long_rows=(L + 127) // 128 > ops.MAX_BLOCKS)[0]
    mask = torch.zeros(po.shape, device=q.device, dtype=torch.uint8)
    mask.scatter_(-1, torch.topk(po.float(), n, dim=-1).indices, 1)
    if m.force_tail:
        mask[..., -m.force_tail:] = 1
        mask[..., -m.force_tail:, :] = 1
    return mask


def inputs(variant, H, D, dev, temps):
    q, k, v = local_qkv(variant, H, D, 0, dev)
    if temps is not None:
        t = torch.linspace(temps[0], temps[1], H, device=dev).view(1, H, 1, 1)
        q = (q.float() * t).to(q.dtype)
    return q, k, v


def sweep(variant, rounds, dev, temps=None, recall=False, fidelity=False):
    H, D = (48, 64) if variant == "cog" else (12, 128)
    q, k, v = inputs(variant, H, D, dev, temps)
    L = q.shape[2]
    mods = settings(variant, H, recall, fidelity)
    pos = mods["energy/probe=recall"].probe_pos.to(dev) if recall else None
    prows = mods["energy/probe=fidelity"].probe_rows.to(dev) if fidelity else None
    dense = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    res = {}

    def ml_fns(m):
        outs = ops.kv_pyramid_outputs(k)

        def pred():
            torch.cuda.manual_seed(SEED)
            return multilevel.predict_level_mask(q, k, rows=m._rows(dev), mask_ratios=m.mask_ratios, pyr=(v, outs))

        def call():
            torch.cuda.manual_seed(SEED)
            return m(q, k, v)
        return {"pred_fused_ms": pred, "call_ms": call}

    def fns(lab, m):
        if lab == MULTILEVEL:
            return ml_fns(m)
        copies = not (m._gather(D) and m._rows(dev) is not None)
        outs = ops.pool_kv_outputs(k, m.sample_gap, reordered=copies)

        def pred():
            torch.cuda.manual_seed(SEED)
            if lab in EQUAL_BUDGET:
                return top_n_mask(m, q, k, n_eq)
            if m.score == "mass":   # the pooled pass is a launch of its own beside this score
                r = m.predict_mask(q, k)
                ops.pool_kv(k, v, m.sample_gap, m._rows(dev), reordered=copies)
                return r
            return m.predict_mask(q, k, pool=(v, m.sample_gap, outs))

        def call():
            torch.cuda.manual_seed(SEED)
            if lab in EQUAL_BUDGET:
                return m(q, k, v, block_mask=top_n_mask(m, q, k, n_eq))
            return m(q, k, v)
        return {"pred_fused_ms": pred, "call_ms": call}

    with torch.no_grad():
        torch.cuda.manual_seed(SEED)
        mods["energy"](q, k, v)
        # the energy run's mean kept blocks per row outside the forced tail rows, less the forced columns
        # top_n_mask adds again; the kept column shows how close the budgets came out
        ft = mods["energy"].force_tail
        body = mods["energy"].last_mask[:, :, :mods["energy"].last_mask.shape[2] - ft]
        n_eq = max(1, round(body.float().sum(-1).mean().item()) - ft)
        work = {lab: fns(lab, m) for lab, m in mods.items()}
        for lab, m in mods.items():   # warm up; quality figures from this call
            out = work[lab]["call_ms"]()
            torch.cuda.synchronize()
            kept = multilevel.density(m.mask_ratios) if lab == MULTILEVEL else m.last_mask.float().mean().item()
            res[lab] = {"kept_fraction": kept, "psnr_vs_dense_db": psnr(out, dense)}
            if recall and lab != MULTILEVEL:
                res[lab].update(recall_of(m, q, k, pos))
            if fidelity:
                res[lab].update(fidelity_of(q, k, v, out, prows))
            if lab != MULTILEVEL and m.head_budget == "judge":
                b = m.last_head_budget.flatten().tolist()
                sp = m.last_head_sparsity.flatten().tolist()
                res[lab].update(head_budget_min=min(b), head_budget_max=max(b), head_budget_mean=sum(b) / len(b),
                                head_sparsity_min=min(sp), head_sparsity_max=max(sp))
            work[lab]["pred_fused_ms"]()
        times = {lab: {f: [] for f in work[lab]} for lab in mods}
        for _ in range(rounds):
            for f in ("pred_fused_ms", "call_ms"):
                for lab in mods:
                    times[lab][f].append(timed(work[lab][f]))
    for lab in mods:
        for f, ts in times[lab].items():
            res[lab][f] = statistics.median(ts)
            res[lab][f + "_min"] = min(ts)
            res[lab][f.replace("_ms", "_vs_energy")] = res[lab][f] / statistics.median(times["energy"][f])
            res[lab][f.replace("_ms", "_vs_uniform")] = res[lab][f] / statistics.median(times["energy/uniform[H]"][f])
    same = torch.equal(mods["judge/clamp(r,r)"].last_mask, mods["energy/uniform[H]"].last_mask)
    return {"variant": variant, "B": 1, "H": H, "L": L, "D": D, "nb": (L + 127) // 128,
            "inputs": "bench.local_qkv(seed 0)" + ("" if temps is None else f", q scaled per head {temps[0]}..{temps[1]}"),
            "rounds": rounds, "calls_per_round": 5, "clamp_rr_mask_equals_uniform": same,
            "equal_budget_blocks_per_row": n_eq, "settings": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="both")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", default=None, metavar="SETTING")
    ap.add_argument("--head-temps", type=float, nargs=2, default=None, metavar=("LO", "HI"))
    ap.add_argument("--recall", action="store_true")
    ap.add_argument("--fidelity", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.one_call:
        variant = "cog" if a.variant == "both" else a.variant
        H, D = (48, 64) if variant == "cog" else (12, 128)
        m = settings(variant, H, a.recall, a.fidelity)[a.one_call]
        q, k, v = inputs(variant, H, D, dev, a.head_temps)
        with torch.no_grad():
            for _ in range(4):
                m(q, k, v)
        torch.cuda.synchronize()
        print(f"{variant} {a.one_call}: 4 calls, kept {m.last_mask.float().mean().item():.4f}"
              + (f", fidelity SNR dB per head {[round(x, 2) for x in m.fidelity.flatten().tolist()]}"
                 if getattr(m, "fidelity", None) is not None else ""))
        return
    out = {"device": torch.cuda.get_device_name(0), "results": []}
    for variant in (["cog", "wan"] if a.variant == "both" else [a.variant]):
        r = sweep(variant, a.rounds, dev, a.head_temps, a.recall, a.fidelity)
        out["results"].append(r)
        print(f"{variant}: H={r['H']} L={r['L']} D={r['D']} ({r['nb']} blocks), inputs {r['inputs']}; "
              f"judge/clamp(r,r) mask == energy/uniform[H] mask: {r['clamp_rr_mask_equals_uniform']}; "
              f"top-n@energy: n = {r['equal_budget_blocks_per_row']} blocks per row")
        print("  setting                      | fused pred ms (x energy) | call ms (x energy, x uniform[H]) | kept   | PSNR dB"
              + (" | recall mean (min head) | oracle recall mean (min head)" if a.recall else "")
              + (" | fidelity SNR dB (min head) | sampled PSNR dB" if a.fidelity else ""))
        for lab, d in r["settings"].items():
            extra = ""
            if a.recall:
                extra = (f" | {d['recall_mean']:.4f} ({d['recall_min_head']:.4f}) | "
                         f"{d['oracle_recall_mean']:.4f} ({d['oracle_recall_min_head']:.4f})"
                         if "recall_mean" in d else " | - | -")
            if a.fidelity:
                extra += (f" | {d['fidelity_snr_db']:.2f} ({d['fidelity_snr_min_head_db']:.2f}) | "
                          f"{d['fidelity_sampled_psnr_db']:.2f}")
            if "head_budget_min" in d:
                extra += (f" | budgets {d['head_budget_min']}..{d['head_budget_max']} (mean {d['head_budget_mean']:.2f}), "
                         f"sparsity {d['head_sparsity_min']:.3f}..{d['head_sparsity_max']:.3f}")
            print(f"  {lab:<28} | {d['pred_fused_ms']:.4f} ({d['pred_fused_vs_energy']:.3f}) | "
                  f"{d['call_ms']:.4f} ({d['call_vs_energy']:.3f}, {d['call_vs_uniform']:.3f}) | {d['kept_fraction']:.4f} | "
                  f"{d['psnr_vs_dense_db']:.2f}{extra}", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
