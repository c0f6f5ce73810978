#!/usr/bin/env python3
"""A/B of the processors' q/k prologue: the eager chain of vblade/patch.py against the one-pass
library call (ops.qk_prologue), in one process, at the two real shapes:

  cog  [1, 17776, 48x64]   per-head LayerNorm + real-pairs RoPE on the 17550 video rows (226 text rows)
  wan  [1, 32760, 12x128]  RMSNorm over the 1536-wide row + complex128 RoPE on every row

Both sides start from the projections' outputs q_proj/k_proj [B,L,H*D] and end with the [B,H,L,D]
q and k that inner_attention receives. Device events around `--reps` back-to-back calls of one side
(inside a model the device always has queued work, so a call's host-side preparation hides behind
the previous kernel; one isolated call would time the Python wrapper as much as the pass), the two
sides alternating inside one loop after a warm-up of both; the median per-call time of the timed
windows is reported, with the fastest and slowest. Successive calls take the next of `--sets`
resident q_proj/k_proj pairs and write fresh outputs, so a call finds neither its input nor its
output in the 256 MB Infinity Cache (three sets: 0.65 GB of inputs between two uses of one).
"GB/s" is compulsory bytes over per-call time: q and k read once and written once plus one read of
the RoPE table, what a single pass has to move, for either side. It is a per-call figure (launch
gaps and the wrapper's allocations included), not a kernel trace. The CogVideoX eager
processor also copies v (value.contiguous()), which the fused path hands over as a view; that copy
is timed on its own line and is NOT part of the ratio.

  python tools/prologue_bench.py [--iters 20] [--reps 50] [--sets 3] [--warmup 5] [--out profiles/qk_prologue_ab.log]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "video-blade_amd"))

HBM_PEAK = 8.0e12   # bytes/s, the MI355X figure DESIGN.md §3 uses

SHAPES = {
    "cog": dict(B=1, L=17776, H=48, D=64, text=226),
    "wan": dict(B=1, L=32760, H=12, D=128, text=0),
}


def build(name, dev, dtype, sets=3):
    from vblade import ops, patch
    s = SHAPES[name]
    B, L, H, D, T = s["B"], s["L"], s["H"], s["D"], s["text"]
    g = torch.Generator(device=dev).manual_seed(0)
    qs, ks, vp = ([(torch.randn(B, L, H * D, generator=g, device=dev) * 1.3 + 0.2).to(dtype) for _ in range(n)]
                  for n in (sets, sets, 1))
    vp = vp[0]
    turn = {"eager": 0, "fused": 0}

    def inputs(side):
        turn[side] += 1
        return qs[turn[side] % sets], ks[turn[side] % sets]
    ang = torch.rand(L - T, D // 2, generator=g, device=dev, dtype=torch.float64) * 6.28
    if name == "cog":
        nq, nk = (torch.nn.LayerNorm(D, eps=1e-6).to(dev, dtype) for _ in range(2))
        ang2 = ang.repeat_interleave(2, -1)
        cos, sin = ang2.cos().float(), ang2.sin().float()
        table_bytes = 2 * cos.numel() * 4

        def eager():
            qp, kp = inputs("eager")
            q = qp.view(B, -1, H, D).transpose(1, 2)
            k = kp.view(B, -1, H, D).transpose(1, 2)
            q = nq(q).to(dtype=dtype)
            k = nk(k).to(dtype=dtype)
            q[:, :, T:] = patch._apply_rotary_emb_real(q[:, :, T:], (cos, sin))
            k[:, :, T:] = patch._apply_rotary_emb_real(k[:, :, T:], (cos, sin))
            return q, k

        def fused():
            qp, kp = inputs("fused")
            return ops.qk_prologue(qp, kp, heads=H, norm="layer", q_weight=nq.weight, q_bias=nq.bias, q_eps=nq.eps,
                                   k_weight=nk.weight, k_bias=nk.bias, k_eps=nk.eps, rope="real", rope_start=T,
                                   cos=cos, sin=sin)

        def v_copy():
            return vp.view(B, -1, H, D).transpose(1, 2).contiguous()
    else:
        nq, nk = (torch.nn.RMSNorm(H * D, eps=1e-6).to(dev, dtype) for _ in range(2))
        freqs = torch.polar(torch.ones_like(ang), ang)[None, None]       # complex128 [1,1,L,D/2]
        table_bytes = freqs.numel() * 16

        def rope(hs):
            x_rotated = torch.view_as_complex(hs.to(torch.float64).unflatten(3, (-1, 2)))
            return torch.view_as_real(x_rotated * freqs).flatten(3, 4).type_as(hs)

        def eager():
            qp, kp = inputs("eager")
            q, k = nq(qp), nk(kp)
            q = q.unflatten(2, (H, -1)).transpose(1, 2)
            k = k.unflatten(2, (H, -1)).transpose(1, 2)
            return rope(q), rope(k)

        def fused():
            qp, kp = inputs("fused")
            return ops.qk_prologue(qp, kp, heads=H, norm="rms", q_weight=nq.weight, q_eps=nq.eps,
                                   k_weight=nk.weight, k_eps=nk.eps, rope="complex", freqs=freqs)

        v_copy = None
    with torch.no_grad():
        for n in (nq, nk):
            n.weight.add_(0.1 * torch.randn_like(n.weight))
    nbytes = 4 * B * L * H * D * vp.element_size() + table_bytes
    return eager, fused, v_copy, nbytes


def timed(fn, reps):
    """ms per call over `reps` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--sets", type=int, default=3, help="resident input pairs the calls rotate through")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--shapes", nargs="+", choices=sorted(SHAPES), default=sorted(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qk_prologue_ab.log"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prologue_bench: needs a GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    lines = [f"# tools/prologue_bench.py --iters {args.iters} --reps {args.reps} --sets {args.sets} --warmup {args.warmup} --dtype {args.dtype}",
             f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ms per call, median [min, max] of "
             f"{args.iters} windows of {args.reps} back-to-back calls over {args.sets} input sets, eager and fused "
             f"alternating; per-call figures, not a kernel trace; "
             f"HBM peak {HBM_PEAK / 1e12:.1f} TB/s"]
    with torch.no_grad():
        for name in args.shapes:
            eager, fused, v_copy, nbytes = build(name, dev, dtype, args.sets)
            for _ in range(args.warmup * args.sets):   # both sides on the same set each time
                e, f = eager(), fused()
            torch.cuda.synchronize()
            share = [(a != b).float().mean().item() for a, b in zip(e, f)]
            del e, f
            t = {"eager": [], "fused": [], "v_copy": []}
            for _ in range(args.iters):
                t["eager"].append(timed(eager, args.reps))
                t["fused"].append(timed(fused, args.reps))
                if v_copy is not None:
                    t["v_copy"].append(timed(v_copy, args.reps))
            s = SHAPES[name]
            lines.append(f"{name}: q,k [{s['B']},{s['L']},{s['H']}x{s['D']}] {args.dtype}, compulsory bytes "
                         f"{nbytes / 1e6:.1f} MB; elements fused != eager: q {share[0]:.2e}, k {share[1]:.2e}")
            med = {}
            for side in ("eager", "fused"):
                med[side] = statistics.median(t[side])
                rate = nbytes / (med[side] * 1e-3)
                lines.append(f"  {side:6s} {med[side]:8.3f} ms [{min(t[side]):.3f}, {max(t[side]):.3f}]  "
                             f"{rate / 1e9:8.1f} GB/s  {rate / HBM_PEAK:.3f} of HBM peak")
            lines.append(f"  ratio eager/fused {med['eager'] / med['fused']:.2f}x")
            if t["v_copy"]:
                lines.append(f"  (eager processor only) value.contiguous() {statistics.median(t['v_copy']):.3f} ms")
            del eager, fused, v_copy
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
