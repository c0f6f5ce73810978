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

--backward times training instead: forward + backward of the eager chain under autograd against
autograd.qk_prologue (ops.qk_prologue forward, ops.qk_prologue_bwd backward), same method, with the
norm parameters frozen (the LoRA case: no parameter gradients) and trainable. The upstream gradients
are [B,H,L,D]-contiguous, as ops.attention_bwd returns them, and rotate with the input sets. "GB/s"
of the forward + backward lines is over the compulsory bytes of both passes: the forward's (above)
plus the backward's, x and g read and dx written for q and k plus one read of the table. A third
line times the fused backward alone (ops.qk_prologue_bwd, reduction launch included) over the
backward's compulsory bytes: the figure to hold against the forward's fraction of the HBM peak.
Peak memory is torch.cuda.max_memory_allocated over one call, above what was allocated before it.
The log goes to profiles/qk_prologue_bwd_ab.log.
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


def build(name, dev, dtype, sets=3, backward=False):
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

        def eager_chain(qp, kp):
            q = qp.view(B, -1, H, D).transpose(1, 2)
            k = kp.view(B, -1, H, D).transpose(1, 2)
            q = nq(q).to(dtype=dtype)
            k = nk(k).to(dtype=dtype)
            q[:, :, T:] = patch._apply_rotary_emb_real(q[:, :, T:], (cos, sin))
            k[:, :, T:] = patch._apply_rotary_emb_real(k[:, :, T:], (cos, sin))
            return q, k

        fused_kw = dict(heads=H, norm="layer", q_weight=nq.weight, q_bias=nq.bias, q_eps=nq.eps,
                        k_weight=nk.weight, k_bias=nk.bias, k_eps=nk.eps, rope="real", rope_start=T, cos=cos, sin=sin)

        def v_copy():
            return vp.view(B, -1, H, D).transpose(1, 2).contiguous()
    else:
        nq, nk = (torch.nn.RMSNorm(H * D, eps=1e-6).to(dev, dtype) for _ in range(2))
        freqs = torch.polar(torch.ones_like(ang), ang)[None, None]       # complex128 [1,1,L,D/2]
        table_bytes = freqs.numel() * 16

        def rope(hs):
            x_rotated = torch.view_as_complex(hs.to(torch.float64).unflatten(3, (-1, 2)))
            return torch.view_as_real(x_rotated * freqs).flatten(3, 4).type_as(hs)

        def eager_chain(qp, kp):
            q, k = nq(qp), nk(kp)
            q = q.unflatten(2, (H, -1)).transpose(1, 2)
            k = k.unflatten(2, (H, -1)).transpose(1, 2)
            return rope(q), rope(k)

        fused_kw = dict(heads=H, norm="rms", q_weight=nq.weight, q_eps=nq.eps, k_weight=nk.weight, k_eps=nk.eps,
                        rope="complex", freqs=freqs)
        v_copy = None

    def eager():
        return eager_chain(*inputs("eager"))

    def fused():
        return ops.qk_prologue(*inputs("fused"), **fused_kw)
    with torch.no_grad():
        for n in (nq, nk):
            n.weight.add_(0.1 * torch.randn_like(n.weight))
    nbytes = 4 * B * L * H * D * vp.element_size() + table_bytes
    if not backward:
        return eager, fused, v_copy, nbytes

    # training: the same chains under autograd, each call on the next input set and its upstream gradients
    from vblade import autograd
    gs = [tuple((torch.randn(B, H, L, D, generator=g, device=dev)).to(dtype) for _ in range(2)) for _ in range(sets)]
    for t in qs + ks:
        t.requires_grad_()
    params = [p for n in (nq, nk) for p in n.parameters()]
    bwd_bytes = 6 * B * L * H * D * vp.element_size() + table_bytes

    def set_wgrad(on):
        for p in params:
            p.requires_grad_(on)

    def step(side, chain):
        turn[side] += 1
        i = turn[side] % sets
        leaves = [qs[i], ks[i]] + [p for p in params if p.requires_grad]
        return torch.autograd.grad(list(chain(qs[i], ks[i])), leaves, list(gs[i]))

    def eager_fb():
        return step("eager", eager_chain)

    def fused_fb():
        return step("fused", lambda qp, kp: autograd.qk_prologue(qp, kp, **fused_kw))

    def fused_b():
        turn["bwd"] = turn.get("bwd", 0) + 1
        i = turn["bwd"] % sets
        w = params[0].requires_grad
        need = (w, w and name == "cog", w, w and name == "cog")
        return ops.qk_prologue_bwd(qs[i], ks[i], gq=gs[i][0], gk=gs[i][1], need_wgrad=need, **fused_kw)

    return eager_fb, fused_fb, fused_b, set_wgrad, nbytes + bwd_bytes, bwd_bytes


def timed(fn, reps):
    """ms per call over `reps` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def peak_above(fn):
    """Bytes torch.cuda.max_memory_allocated rises above the current allocation over one call of fn."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    del out
    return torch.cuda.max_memory_allocated() - base


def backward_lines(args, dev, dtype):
    lines = []
    for name in args.shapes:
        eager_fb, fused_fb, fused_b, set_wgrad, nbytes, bwd_bytes = build(name, dev, dtype, args.sets, backward=True)
        s = SHAPES[name]
        lines.append(f"{name}: q,k [{s['B']},{s['L']},{s['H']}x{s['D']}] {args.dtype}, compulsory bytes forward + backward "
                     f"{nbytes / 1e6:.1f} MB, backward alone {bwd_bytes / 1e6:.1f} MB")
        for wgrad in (False, True):
            set_wgrad(wgrad)
            for _ in range(args.warmup * args.sets):
                e, f = eager_fb(), fused_fb()
                fused_b()
            torch.cuda.synchronize()
            rel = [((a.double() - b.double()).norm() / a.double().norm()).item() for a, b in zip(e, f)]
            del e, f
            t = {"eager": [], "fused": [], "bwd": []}
            for _ in range(args.iters):
                t["eager"].append(timed(eager_fb, args.reps))
                t["fused"].append(timed(fused_fb, args.reps))
                t["bwd"].append(timed(fused_b, args.reps))
            peak = {"eager": peak_above(eager_fb), "fused": peak_above(fused_fb), "bwd": peak_above(fused_b)}
            lines.append(f" parameter gradients {'on' if wgrad else 'off (frozen norms, the LoRA case)'}; "
                         f"||fused - eager|| / ||eager|| per gradient: " + ", ".join(f"{r:.2e}" for r in rel))
            med = {side: statistics.median(v) for side, v in t.items()}
            for side, label, nb in (("eager", "eager fwd+bwd", nbytes), ("fused", "fused fwd+bwd", nbytes),
                                    ("bwd", "fused bwd alone", bwd_bytes)):
                rate = nb / (med[side] * 1e-3)
                lines.append(f"  {label:15s} {med[side]:8.3f} ms [{min(t[side]):.3f}, {max(t[side]):.3f}]  "
                             f"{rate / 1e9:8.1f} GB/s  {rate / HBM_PEAK:.3f} of HBM peak  peak memory "
                             f"{peak[side] / 1e6:8.1f} MB")
            lines.append(f"  ratio eager/fused (fwd+bwd) {med['eager'] / med['fused']:.2f}x")
        del eager_fb, fused_fb, fused_b, set_wgrad
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=50, help="back-to-back calls per timed window")
    ap.add_argument("--sets", type=int, default=3, help="resident input pairs the calls rotate through")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=["bf16", "fp16"], default="bf16")
    ap.add_argument("--shapes", nargs="+", choices=sorted(SHAPES), default=sorted(SHAPES))
    ap.add_argument("--backward", action="store_true", help="time forward + backward under autograd (training)")
    ap.add_argument("--out", default=None, help="default profiles/qk_prologue_ab.log, with --backward "
                                                "profiles/qk_prologue_bwd_ab.log")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "qk_prologue_bwd_ab.log" if args.backward else "qk_prologue_ab.log")
    if not torch.cuda.is_available():
        sys.exit("prologue_bench: needs a GPU (a CPU run says nothing about these times)")
    dev = torch.device("cuda", 0)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    lines = [f"# tools/prologue_bench.py{' --backward' if args.backward else ''} --iters {args.iters} --reps {args.reps} --sets {args.sets} --warmup {args.warmup} --dtype {args.dtype}",
             f"# device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ms per call, median [min, max] of "
             f"{args.iters} windows of {args.reps} back-to-back calls over {args.sets} input sets, eager and fused "
             f"alternating; per-call figures, not a kernel trace; "
             f"HBM peak {HBM_PEAK / 1e12:.1f} TB/s"]
    if args.backward:
        lines += backward_lines(args, dev, dtype)
    with torch.no_grad():
        for name in ([] if args.backward else args.shapes):
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
