#!/usr/bin/env python3
"""A/B timing of the projection-layout option (io_layout="blhd") against the default path
(io_layout="bhld") in ONE process on ONE GPU, in the style of tools/ab.py: the same inputs (bench.py's
generators), launches interleaved A,B,A,B,... so clock and device drift cancel, outputs cross-checked
bit for bit before anything is timed.
usage: python tools/io_layout_ab.py [--variant cog|wan|both] [--what attn,proc,train] [--rounds N]
  attn   the fused attention launch alone (ops.attention_fwd on a predicted mask): contiguous output
         against projection-layout output: what the strided store itself costs
  proc   processor-level inference: inner_attention(q, k, v) plus the processors' reshape, up to the
         [B,L,H*D] tensor to_out[0] would read (a copy on the default path, a view with the option)
  train  one train.StandInAttentionBlock forward + backward (LoRA projections around the module under
         autograd), for both grad_combine forms; the option also drops the block's v.contiguous()"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-blade_amd"))
sys.path.insert(0, ROOT)
import vblade  # noqa: E402
from vblade import ops, train  # noqa: E402
from bench import realistic_qkv  # noqa: E402

TAGS = ("bhld", "blhd")
REPS = 5


def interleaved(fns, rounds):
    """Median and minimum ms per call of each function, timed in turn: REPS calls between two events."""
    times = {t: [] for t in fns}
    for _ in range(rounds):
        for t, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[t].append(e0.elapsed_time(e1) / REPS)
    return {t: (statistics.median(v), min(v)) for t, v in times.items()}


def report(label, res, note=""):
    base = res[TAGS[0]][0]
    for t in TAGS:
        md, mn = res[t]
        print(f"{label} {t}: median {md:.4f} ms (min {mn:.4f})  x{base / md:.3f} vs {TAGS[0]}", flush=True)
    d = (res[TAGS[0]][0] - res[TAGS[1]][0]) * 1e3
    print(f"{label}: {TAGS[1]} saves {d:+.1f} us per call (median){note}", flush=True)


def same(label, a, b):
    a = a if isinstance(a, (tuple, list)) else (a,)
    b = b if isinstance(b, (tuple, list)) else (b,)
    ok = all(torch.equal(x, y) for x, y in zip(a, b))
    print(f"  {label}: {TAGS[1]} bit-identical to {TAGS[0]} over {len(a)} tensor(s): {ok}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="both")
    ap.add_argument("--what", default="attn,proc,train")
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    what = a.what.split(",")
    dev = torch.device("cuda")
    for variant in (["cog", "wan"] if a.variant == "both" else [a.variant]):
        H, D = (48, 64) if variant == "cog" else (12, 128)
        mods = {t: vblade.AdaptiveBlockSparseAttn(variant, log_every=0, io_layout=t).to(dev) for t in TAGS}
        m = mods[TAGS[0]]
        L = m.gilbert_rearranger.seq_len
        q, k, v = realistic_qkv(H, L, D, 0, dev)
        rows = m._rows(dev)
        nbytes = H * L * D * 2
        print(f"{variant}: H={H} L={L} D={D}; one [1,H,L,D] tensor is {nbytes / 1e6:.1f} MB "
              f"(a copy reads and writes it: {2 * nbytes / 1e6:.1f} MB of traffic)", flush=True)
        with torch.no_grad():
            if "attn" in what:
                qo, ko = vblade.draw_sample_offsets(1, H, dev), vblade.draw_sample_offsets(1, H, dev)
                _, mask = m.predict_mask(q, k, qo, ko)
                gather = m._gather(D)
                pooled = ops.pool_kv(k, v, m.sample_gap, rows, reordered=not gather)
                kp, vp = pooled[0], pooled[1]
                k_src, v_src, kv_rows = (k, v, rows) if gather else (pooled[2], pooled[3], None)
                qlen = (mask != 0).sum(-1).to(torch.int32).contiguous()

                def attn(layout):   # the module's inference launch, as AdaptiveBlockSparseAttn.forward makes it
                    return ops.attention_fwd(q, k_src, v_src, block_mask=mask, q_rows=rows, kv_rows=kv_rows, kp=kp,
                                             vp=vp, kp_log_bias=m._log_gap(q.dtype), heavy_rows=m.force_tail,
                                             order=m.order, q_lengths=qlen if m.order else None,
                                             persistent=m.persistent, out_layout=layout)

                fns = {t: (lambda t=t: attn(t)) for t in TAGS}
                same(f"{variant} attn", *(fn() for fn in fns.values()))
                report(f"{variant} attn", interleaved(fns, a.rounds))
                # the copy the option removes, alone: contiguous [1,H,L,D] -> [1,L,H*D]
                o = attn("bhld")
                cp = interleaved({t: (lambda: o.transpose(1, 2).reshape(1, L, H * D)) for t in TAGS}, a.rounds)
                print(f"{variant} reshape copy alone: median {cp[TAGS[0]][0]:.4f} ms (min {cp[TAGS[0]][1]:.4f})", flush=True)
            if "proc" in what:
                def proc(t):
                    out = mods[t](q, k, v)
                    return out.transpose(1, 2).reshape(1, L, H * D)

                outs = []
                for t in TAGS:
                    torch.cuda.manual_seed(1234)   # the module draws its sampling offsets per call
                    out = mods[t](q, k, v)
                    flat = out.transpose(1, 2).reshape(1, L, H * D)
                    view = flat.untyped_storage().data_ptr() == out.untyped_storage().data_ptr()
                    print(f"  {variant} proc {t}: the reshape is a {'view' if view else 'copy'}", flush=True)
                    outs.append(flat)
                same(f"{variant} proc", *outs)
                report(f"{variant} proc", interleaved({t: (lambda t=t: proc(t)) for t in TAGS}, a.rounds))
        if "train" in what:
            x = q.transpose(1, 2).reshape(1, L, H * D).contiguous()
            for gc in ("reference", "joint"):
                blocks = {}
                for t in TAGS:
                    inner = vblade.AdaptiveBlockSparseAttn(variant, log_every=0, io_layout=t, grad_combine=gc).to(dev)
                    blocks[t] = train.StandInAttentionBlock(H * D, H, 64, 64.0, inner, device=dev,
                                                            generator=torch.Generator().manual_seed(0),
                                                            projection_layout=t == "blhd")
                    with torch.no_grad():   # LoRA B starts at zero: give every adapter a gradient path
                        gb = torch.Generator().manual_seed(1)
                        for n, p in blocks[t].named_parameters():
                            if n.endswith("lora_B"):
                                p.copy_(0.02 * torch.randn(p.shape, generator=gb))
                params = {t: [p for p in blocks[t].parameters() if p.requires_grad] for t in TAGS}

                def step(t):
                    for p in params[t]:
                        p.grad = None
                    loss = blocks[t](x).float().square().mean()
                    loss.backward()
                    return loss.detach()

                res = []
                for t in TAGS:
                    torch.cuda.manual_seed(1234)
                    loss = step(t)
                    res.append([loss] + [p.grad.clone() for p in params[t]])
                torch.cuda.synchronize()
                same(f"{variant} train {gc} (loss and LoRA gradients)", *res)
                report(f"{variant} train {gc}", interleaved({t: (lambda t=t: step(t)) for t in TAGS}, a.rounds))
                del blocks, params


if __name__ == "__main__":
    main()
