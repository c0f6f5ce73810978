"""Adaptive block-sparse attention module — the ``attn.inner_attention(q, k, v)`` surface.

Mirrors ``AdaptiveBlockSparseAttnTrain`` (cogvideox/train/special_attentions_local/TrainRelated/
cogvideo_blocksparseattn.py:398-427; wanx_blocksparseattn.py:375-409) and its helpers
(``adaptive_block_sparse_attn`` :327-394, ``GilbertRearranger`` :110-161,
``transfer_attn_to_mask`` :177-249, ``simple_pooling`` :83-88), with the module-level globals
(:9-16) as constructor arguments. Every tensor op of the hot path runs in libvblade_hip.so:

  forward (inference, the 8-step samplers):
    1. vb_mask_predict  — sampled pooled scores + energy top-k -> block mask (Gilbert order); the
                          pooled K/V pass (mean over `sample_gap` reordered tokens) runs in the
                          same launch as extra workgroups (one stream, no events)
    2. vb_attn_fwd      — ONE softmax over kept full-res keys ∪ pooled keys (+ln gap bias):
                          the reference's two attention calls + LSE combine, fused; q/k/v rows
                          gathered and out rows scattered through the Gilbert index (no copies)
  training (grad required) keeps the reference's two-branch structure so the backward has the
  reference's semantics (LSE/alpha detached): see ``autograd.adaptive_split_attention``. With
  grad_combine="joint" the call under autograd is the inference call (steps 1 and 2, the LSE
  stored) and the backward is the exact gradient of that one softmax:
  ``autograd.adaptive_joint_attention``.

Only the tiny RNG draw of the sampling offsets (torch.rand + topk over [B,H,1,128], exactly as
cogvideo_blocksparseattn.py:45-46 so the RNG stream matches the reference) stays in PyTorch.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops

VARIANT_DEFAULTS = {
    # cogvideo_blocksparseattn.py:9-16
    "cog": dict(use_rearrange=True, max_retain_ratio=0.1, min_retain_ratio=0.05, width=45,
                height=30, depth=13, sample_gap=15, text_length=226, force_tail=2, log_every=800),
    # wanx_blocksparseattn.py:9-16 (+ no forced rows/cols, print every 200 calls :400)
    "wan": dict(use_rearrange=True, max_retain_ratio=0.17, min_retain_ratio=0.05, width=52,
                height=30, depth=21, sample_gap=30, text_length=0, force_tail=0, log_every=200),
}


# longest-first dispatch of the attention launch (one small ordering launch before it), per
# variant. Measured (tools/ab.py, round 5, profiles/archive/r05_attn_order_ab.log): Wan 1.047-1.054x per
# attention launch; CogVideoX 0.98x over the whole range and 0.976-0.989x with only the last
# 64-256 q-blocks of each XCD range re-ordered (its q-blocks differ little in length, and the
# Gilbert-neighbour order's L2 reuse and the extra launch cost more than the tail)
ORDER_DEFAULT = {"cog": False, "wan": True}

# persistent attention launch (resident-sized grid, per-XCD work queues; ops.attention_fwd
# persistent=True), per variant. Measured (tools/ab.py, profiles/r06_persist_*_ab.log): the
# CogVideoX attention launch alone 1.005-1.009x, but the whole call 0.99-1.00x (r06_persist_call_ab.log);
# Wan's inference launch (gathered K/V) 0.98x per call. Off for both; the training path's D=128 LSE
# launch runs persistent (autograd.py, 1.024-1.030x).
PERSISTENT_DEFAULT = {"cog": False, "wan": False}


def retain_counts(nb: int, min_ratio: float, max_ratio: float, variant: str):
    """Kept-block clamp bounds. cog: (seq * fp32 ratio tensor).to(int) clamped >= 1
    (cogvideo_blocksparseattn.py:230-231, 347-348); wan: max(1, int(seq * ratio)) (wanx :215-216)."""
    if variant == "cog":
        lo = int(np.float32(nb) * np.float32(min_ratio))
        hi = int(np.float32(nb) * np.float32(max_ratio))
    else:
        lo, hi = int(nb * min_ratio), int(nb * max_ratio)
    return max(1, lo), max(1, hi)


def draw_sample_offsets(B: int, H: int, device, block: int = 128, num_keep: int = 32,
                        generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """rand(B,H,1,block) -> topk(num_keep) offsets, shared by all blocks of a (b,h)
    (random_sample_tokens, cogvideo_blocksparseattn.py:45-46). int32 [B,H,num_keep]."""
    r = torch.rand(B, H, 1, block, device=device, generator=generator)
    return torch.topk(r, num_keep, dim=3).indices[:, :, 0, :].to(torch.int32)


def draw_sample_offsets_qk(B: int, H: int, device, block: int = 128, num_keep: int = 32,
                           generator: Optional[torch.Generator] = None):
    """The q and k draws of efficient_attn_with_pooling (:77-78): two torch.rand calls in the
    reference's order (the same RNG stream), the two topk selections in one HIP launch
    (vb_sample_offsets; same indices as torch.topk for distinct values)."""
    rq = torch.rand(B, H, 1, block, device=device, generator=generator)
    rk = torch.rand(B, H, 1, block, device=device, generator=generator)
    q_off, k_off = ops.sample_offsets(rq, rk, num_keep)
    return q_off[:, :, 0, :], k_off[:, :, 0, :]


class GilbertRearranger(nn.Module):
    """Index maps of the Gilbert reorder (cogvideo_blocksparseattn.py:110-161; wanx :102-159).

    ``rows[g]`` = caller row holding reordered position g. The attention kernels consume
    ``rows`` directly; ``rearrange``/``reversed_rearrange`` are provided for API parity and
    debugging (they materialise copies the fused path never makes)."""

    def __init__(self, width: int, height: int, depth: int, text_length: int = 0):
        super().__init__()
        self.width, self.height, self.depth, self.text_length = width, height, depth, text_length
        perm = ops.gilbert_perm(width, height, depth).astype(np.int64)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(perm.size)
        self.register_buffer("original_order2gilbert_order", torch.from_numpy(perm), persistent=False)
        self.register_buffer("gilbert_order2original_order", torch.from_numpy(inv), persistent=False)
        rows = np.concatenate([perm + text_length, np.arange(text_length)]).astype(np.int32)
        self.register_buffer("rows", torch.from_numpy(rows), persistent=False)

    @property
    def seq_len(self) -> int:
        return self.width * self.height * self.depth + self.text_length

    def rearrange(self, q, k, v):
        r = self.rows.to(q.device).long()
        return q[..., r, :], k[..., r, :], v[..., r, :]

    def reversed_rearrange(self, out):
        r = self.rows.to(out.device).long()
        res = torch.empty_like(out)
        res[..., r, :] = out
        return res


def parse_probe(probe, allowed):
    """The ``probe`` option as a tuple of names: None, one of ``allowed``, or a tuple or list of distinct
    ones. Anything else raises ValueError."""
    if probe is None:
        return ()
    names = (probe,) if isinstance(probe, str) else probe
    if (not isinstance(names, (tuple, list)) or not names or len(set(names)) != len(names)
            or any(not isinstance(n, str) or n not in allowed for n in names)):
        forms = " or ".join(repr(n) for n in allowed)
        raise ValueError(f"probe must be None, {forms}" + (", or a tuple of both" if len(allowed) > 1 else "")
                         + f", got {probe!r}")
    return tuple(names)


def probe_fidelity(module, q, k, v, out):
    """One fidelity measurement of a module call (the adaptive and the multi-level module share it):
    ops.attn_fidelity under no_grad on the detached tensors, ``last_fidelity_*`` and the running sums
    on the device."""
    rows = module.probe_rows
    if rows.device != q.device or rows.dtype != torch.int32:
        rows = rows.to(device=q.device, dtype=torch.int32)
        module.probe_rows = rows
    with torch.no_grad():
        err, sig, peak = ops.attn_fidelity(q.detach(), k.detach(), v.detach(), out.detach(), rows)
        sums = module._fidelity_sums
        if sums is None or sums.shape[1:] != err.shape or sums.device != err.device:
            sums = module._fidelity_sums = torch.zeros(2, *err.shape, device=err.device, dtype=torch.float32)
            module._fidelity_count = 0
        sums[0].add_(err)
        sums[1].add_(sig)
    module._fidelity_count += 1
    module.last_fidelity_err, module.last_fidelity_sig, module.last_fidelity_peak = err, sig, peak


def fidelity_snr(module):
    if module._fidelity_sums is None or module._fidelity_count == 0:
        return None
    sums = module._fidelity_sums.cpu()
    return ops.fidelity_snr_db(sums[0], sums[1]).float()


class AdaptiveBlockSparseAttn(nn.Module):
    """``inner_attention(q, k, v) -> out`` with q,k,v,out [B,H,L,D] bf16/fp16 on a HIP device.

    variant: "cog" (CogVideoX-5B: text tail, forced last 2 block rows/cols) or "wan"
    (Wan2.1-1.3B). Keyword arguments override the reference's module globals.
    num_keep: tokens the mask predictor samples per 128-token block, 16, 32 (default, the
    reference's) or 64: a quarter / four times the predictor's score work. Given q_off/k_off must
    be [B,H,num_keep].
    combine: "fused" (one softmax, inference default) or "reference" (two attention calls + the
    reference's bf16 LSE combine, bit-for-bit structure of :366-393; used under autograd unless grad_combine="joint").
    grad_combine: what a call that records gradients differentiates: "reference" (default: the two-branch
    form above, both LSEs and the combine weight constants, the reference's gradient) or "joint" (the
    one softmax the inference call evaluates, with the same rounded ln(gap) bias, and its exact
    gradient: one attention launch forward, the pooled pass riding in the predictor's launch as at
    inference, ops.attention_bwd_joint backward; dq and dk differ from the reference's by the dropped
    (out1 - out2)·d alpha term). Inference calls are the same in both.
    mask_head_mode: how the reference's head_mask_type = ones(H) (:313) reads the predicted
    [B,H,nb,nb] mask, which SURVEY Appendix B leaves open offline: "per_head" (default: each head
    its own predicted mask, Block-Sparse-Attention's renumbering of the ones) or "shared_head0"
    (every head attends with head 0's mask). The sparsity statistic counts the predicted mask in
    both modes, as the reference's (:394) does.
    mask_mode: transfer_attn_to_mask's ``mode``: "energy" (default) or "topk" (:205-225): every row
    starts from the budget ``init_k`` (a ratio of the row's blocks below 1, int(nb * init_k), or a
    block count, as the reference reads it) and triples it / shrinks it to k/3*2 when those blocks
    hold less than 0.6 / 0.9 of the row's energy; the retain ratios and the threshold are unused.
    min_retain_ratio, max_retain_ratio, energy_threshold: a float, or a tensor [H] or [B,H] with one
    value per head (the CogVideoX reference's [B,H] ratio tensors, :230-231, :347-348). Tensor
    ratios become per-head block counts on the device (``retain_counts``' arithmetic per variant),
    once per (tensor, B, H, nb, device); a steady-state call launches nothing extra and never
    synchronises. Either option runs the mask rule in the predictor's own launch
    (vb_mask_predict_rule); without them the module makes the calls it always made.
    head_budget: None (default) or "judge": every call estimates each head's concentration from its own
    q and k (ops.judge_sparsity: ``judge_samples`` probe rows against every ``judge_key_stride``-th
    key, the softmax mass of the top ``judge_top`` of the keys) and gives head (b,h) the budget
    clamp(max_retain_ratio * sparsity / sparsity.mean(), *judge_clamp) (ops.head_budget; the
    reference's commented-out lines, cogvideo_blocksparseattn.py:344-348) as its energy rule's
    max_keep. max_retain_ratio must then be a float and mask_mode "energy". The probe rows are drawn
    once, at construction, from a CPU generator seeded with ``judge_seed`` (distinct video rows; the
    non-persistent buffer ``judge_rows``, which may be overwritten; ``forward(judge_rows=...)``
    overrides it for one call), so a call consumes no random numbers. ``last_head_sparsity`` (fp32
    [B,H]) and ``last_head_budget`` (int32 [B,H]) stay on the device.
    probe: None (default) or "recall": every ``probe_every``-th call measures, on its own q, k and the
    mask its attention launch uses (predicted or given, the shared_head0 view included), the exact
    share of the softmax mass the mask keeps for ``probe_samples`` probe queries per head, and the
    best share a mask with as many blocks could have kept (ops.mask_recall). ``last_recall`` and
    ``last_oracle_recall`` (fp32 [B,H]) stay on the device; ``recall`` reads the running means. The
    probe positions are drawn once, at construction, from a CPU generator seeded with ``probe_seed``
    (distinct reordered positions of the video part; the non-persistent buffer ``probe_pos``, which
    may be overwritten). Output, mask and random stream are those of a module without the option.
    probe "fidelity" (alone, or with "recall" as a tuple or list of both): every ``probe_every``-th call
    measures, after its output exists, the error of that output against exact dense attention on its own
    q, k and v for the same ``probe_samples`` queries (ops.attn_fidelity: V, the pooled branch and the
    combine included, which recall leaves out). The positions are the recall probe's draw, mapped once
    through the rearranger's ``rows`` into caller rows (the non-persistent buffer ``probe_rows``, which
    may be overwritten; without the reorder a position is its own caller row). ``last_fidelity_err``,
    ``last_fidelity_sig`` and ``last_fidelity_peak`` (fp32 [B,H]) stay on the device; ``fidelity`` reads
    the per-head SNR in dB over the probed calls. Inference and autograd calls are probed alike, under
    no_grad on detached tensors.
    score: the block score the mask rule reads: "max" (default: the reference kernel's proxy, the largest
    single-key probability ratio of a block, ops.mask_predict; the code path, launches and random stream
    of a module without the option) or "mass" (the sampled softmax mass of the block, the sum-pooled
    attention map the reference's docstring describes: ops.sample_offsets -> ops.mask_scores_mass ->
    ops.block_mask_rule, the pooled K/V pass as its own launch). The same seed samples the same tokens
    in both modes; every mask option above works with either. "mass" needs num_keep=32.
    io_layout: the memory order of what the module returns: "bhld" (default: contiguous [B,H,L,D]) or
    "blhd": the output lives in [B,L,H,D] memory, the projections' layout, and is returned as its
    [B,H,L,D] view, so the processors' ``transpose(1, 2).reshape(B, L, H*D)`` is a view instead of a
    full-tensor copy. Under autograd (both grad_combine forms) the incoming gradient, a transposed view
    of [B,L,H*D] memory, is read through its strides, and dq, dk and dv come back in that layout too.
    The kernels store through other strides, nothing else: output values, masks, probe figures and the
    random stream are bit for bit those of the default.
    """

    def __init__(self, variant: str = "cog", *, combine: str = "fused", **overrides):
        super().__init__()
        if variant not in VARIANT_DEFAULTS:
            raise ValueError(f"variant must be one of {list(VARIANT_DEFAULTS)}")
        cfg = dict(VARIANT_DEFAULTS[variant])
        unknown = set(overrides) - set(cfg) - {"energy_threshold", "block", "num_keep", "overlap", "gather_kv",
                                               "mask_head_mode", "order", "order_window", "persistent",
                                               "mask_mode", "init_k", "head_budget", "judge_samples",
                                               "judge_key_stride", "judge_top", "judge_clamp", "judge_seed",
                                               "probe", "probe_samples", "probe_seed", "probe_every", "score",
                                               "grad_combine", "io_layout"}
        if unknown:
            raise TypeError(f"unknown options {sorted(unknown)}")
        cfg.update(overrides)
        self.variant = variant
        self.combine = combine
        self.grad_combine = cfg.get("grad_combine", "reference")
        if self.grad_combine not in ("reference", "joint"):
            raise ValueError(f"grad_combine must be 'reference' or 'joint', got {self.grad_combine!r}")
        self.io_layout = ops.io_layout_code("io_layout", cfg.get("io_layout", "bhld"))
        self.use_rearrange = cfg["use_rearrange"]
        self.max_retain_ratio = cfg["max_retain_ratio"]
        self.min_retain_ratio = cfg["min_retain_ratio"]
        self.sample_gap = int(cfg["sample_gap"])
        self.text_length = int(cfg["text_length"])
        self.force_tail = int(cfg["force_tail"])
        thr = cfg.get("energy_threshold", 0.95)
        self.energy_threshold = thr if isinstance(thr, torch.Tensor) else float(thr)
        self.mask_mode = cfg.get("mask_mode", "energy")
        if self.mask_mode not in ops.RULE_MODES:
            raise ValueError(f"mask_mode must be one of {list(ops.RULE_MODES)}, got {self.mask_mode!r}")
        self.init_k = cfg.get("init_k")
        if self.mask_mode == "topk" and (self.init_k is None or not self.init_k > 0):
            raise ValueError("mask_mode='topk' needs init_k > 0 (a ratio below 1 or a block count)")
        self._per_head_cache = {}
        self.head_budget = cfg.get("head_budget")
        self.judge_samples = int(cfg.get("judge_samples", 30))
        self.judge_key_stride = int(cfg.get("judge_key_stride", 3))
        self.judge_top = float(cfg.get("judge_top", 0.2))
        self.judge_clamp = tuple(float(c) for c in cfg.get("judge_clamp", (0.05, 0.9)))
        self.judge_seed = int(cfg.get("judge_seed", 0))
        self.last_head_sparsity: Optional[torch.Tensor] = None
        self.last_head_budget: Optional[torch.Tensor] = None
        if self.head_budget not in (None, "judge"):
            raise ValueError(f"head_budget must be None or 'judge', got {self.head_budget!r}")
        if self.head_budget == "judge":
            if self.mask_mode != "energy":
                raise ValueError("head_budget='judge' sets the energy rule's max_keep: mask_mode must be 'energy'")
            if isinstance(self.max_retain_ratio, torch.Tensor):
                raise ValueError("head_budget='judge' scales a float max_retain_ratio per head; a tensor "
                                 "max_retain_ratio already is a per-head budget")
            if not 1 <= self.judge_samples <= ops.JUDGE_MAX_SAMPLES:
                raise ValueError(f"judge_samples must be in [1, {ops.JUDGE_MAX_SAMPLES}], got {self.judge_samples}")
            if len(self.judge_clamp) != 2 or not self.judge_clamp[0] <= self.judge_clamp[1]:
                raise ValueError(f"judge_clamp must be (lo, hi) with lo <= hi, got {self.judge_clamp}")
            if self.judge_key_stride < 1 or not 0.0 < self.judge_top <= 1.0:
                raise ValueError("judge_key_stride must be >= 1 and judge_top in (0, 1]")
            video = int(cfg["width"]) * int(cfg["height"]) * int(cfg["depth"])
            if self.judge_samples > video:
                raise ValueError(f"judge_samples {self.judge_samples} exceeds the {video} video tokens")
            # the probe: judge_samples distinct video rows, drawn ONCE from a CPU generator (the
            # reference's randperm(width*height)[:sample_num] + text_length draws anew per call and from
            # the first frame only; assign such rows to the buffer to get that). A fixed probe keeps
            # the call free of RNG use, identical under checkpoint recompute, and capturable.
            gen = torch.Generator(device="cpu")
            gen.manual_seed(self.judge_seed)
            probe = self.text_length + torch.randperm(video, generator=gen)[:self.judge_samples]
            self.register_buffer("judge_rows", probe.to(torch.int32), persistent=False)
        self.probe = cfg.get("probe")
        self.probe_samples = int(cfg.get("probe_samples", 30))
        self.probe_seed = int(cfg.get("probe_seed", 0))
        self.probe_every = int(cfg.get("probe_every", 1))
        self.last_recall: Optional[torch.Tensor] = None
        self.last_oracle_recall: Optional[torch.Tensor] = None
        self._probe_calls = 0      # host counter of forward calls, probed or not
        self._recall_sums = None   # fp32 [2,B,H] on the device: recall and oracle recall, summed over the probed calls
        self._recall_count = 0
        self.last_fidelity_err: Optional[torch.Tensor] = None
        self.last_fidelity_sig: Optional[torch.Tensor] = None
        self.last_fidelity_peak: Optional[torch.Tensor] = None
        self._fidelity_sums = None   # fp32 [2,B,H] on the device: err and sig, summed over the probed calls
        self._fidelity_count = 0
        self._probes = parse_probe(self.probe, ("recall", "fidelity"))
        if self._probes:
            if not 1 <= self.probe_samples <= ops.RECALL_MAX_SAMPLES:
                raise ValueError(f"probe_samples must be in [1, {ops.RECALL_MAX_SAMPLES}], got {self.probe_samples}")
            if self.probe_every < 1:
                raise ValueError(f"probe_every must be >= 1, got {self.probe_every}")
            video = int(cfg["width"]) * int(cfg["height"]) * int(cfg["depth"])
            if self.probe_samples > video:
                raise ValueError(f"probe_samples {self.probe_samples} exceeds the {video} video tokens")
            # probe_samples distinct REORDERED positions of the video part (the reordered sequence is
            # [video in Gilbert order, text]), drawn ONCE from a CPU generator, as the judge's rows are:
            # a call consumes no random numbers and can be captured
            gen = torch.Generator(device="cpu")
            gen.manual_seed(self.probe_seed)
            pos = torch.randperm(video, generator=gen)[:self.probe_samples]
            if "recall" in self._probes:
                self.register_buffer("probe_pos", pos.to(torch.int32), persistent=False)
        self.block = int(cfg.get("block", 128))
        self.num_keep = int(cfg.get("num_keep", 32))
        if self.block != 128 or self.num_keep not in ops.NUM_KEEP_VALUES:
            raise ValueError(f"block must be 128 (the reference's only value) and num_keep one of "
                             f"{ops.NUM_KEEP_VALUES} (the reference's default is 32)")
        self.score = cfg.get("score", "max")
        if self.score not in ("max", "mass"):
            raise ValueError(f"score must be 'max' or 'mass', got {self.score!r}")
        if self.score == "mass" and self.num_keep != ops.MASS_NUM_KEEP:
            raise ValueError(f"score='mass' samples {ops.MASS_NUM_KEEP} tokens per block only, got num_keep="
                             f"{self.num_keep}")
        self.log_every = int(cfg["log_every"])
        self.mask_head_mode = cfg.get("mask_head_mode", "per_head")
        ops.mask_head_mode_code(self.mask_head_mode)   # validates
        self.gilbert_rearranger = GilbertRearranger(cfg["width"], cfg["height"], cfg["depth"],
                                                    self.text_length)
        if "fidelity" in self._probes:
            # the same queries as caller rows: the fidelity probe takes no order
            prow = self.gilbert_rearranger.rows[pos.long()] if self.use_rearrange else pos
            self.register_buffer("probe_rows", prow.to(torch.int32).clone(), persistent=False)
        # running sparsity statistic kept on the device (the reference's .item() per call, :415,
        # is replaced by a device counter; read it through .sparsity)
        self.sparsity_counter = 0
        self._kept_slots = None
        self._slot_totals = []
        self.last_mask: Optional[torch.Tensor] = None
        # optional list: when set, every `attn_event_every`-th fused attention launch is bracketed
        # by a pair of HIP events on the launch stream (bench.py's live kernel timing; each pair is
        # two marker packets that cost the stream a few us, so the bench samples); None = no events
        self.attn_events: Optional[list] = None
        self.attn_event_every = 1
        self._attn_launches = 0
        # run the pooled K/V pass inside the predictor's launch (extra workgroups beside the score
        # workgroups, one stream) instead of as its own launch after it (inference only)
        self.overlap = bool(cfg.get("overlap", True))
        # The attention kernel gathers K/V rows through the Gilbert index (True) or streams the
        # Gilbert-ordered contiguous copies the pooled pass writes (False: 2·L·D·2 bytes more per
        # head, written beside the predictor). "auto" (default): what measured faster per head dim
        # (tools/diag/overlap_ab.py --opt gather_kv): gather at D=128 (Wan, +2.4 % per call), copies at
        # D=64 (CogVideoX, +0.9 %).
        self.gather_kv = cfg.get("gather_kv", "auto")
        # Dispatch each XCD's q-blocks of the attention launch longest first (the predictor writes
        # every mask row's kept-block count; a small launch sorts the XCD ranges before the kernel):
        # the kernel's tail is its last workgroups. Scheduling only: outputs are bit-identical.
        # order_window > 0 re-orders only each XCD range's last q-blocks (the tail), keeping the
        # head-major Gilbert-neighbour order elsewhere for its L2 reuse.
        self.order = bool(cfg.get("order", ORDER_DEFAULT[variant]))
        self.order_window = int(cfg.get("order_window", 0))
        # The fused attention launch is resident-sized (as many workgroups as fit on the device at
        # once) and its workgroups pull q-blocks from per-XCD queues in the order above, then help
        # the other XCDs: no per-workgroup launch gaps, no XCD left idle at the end. Scheduling
        # only: outputs are bit-identical.
        self.persistent = bool(cfg.get("persistent", PERSISTENT_DEFAULT[variant]))

    # -------------------------------------------------------------------------------- helpers
    def _rows(self, device):
        if not self.use_rearrange:
            return None
        r = self.gilbert_rearranger.rows
        if r.device != device:
            r = r.to(device)
            self.gilbert_rearranger.rows = r
        return r

    def _gather(self, D: int) -> bool:
        if self.gather_kv != "auto":
            return bool(self.gather_kv)
        return D == 128

    def _count_slot(self, device):
        if self._kept_slots is None or self._kept_slots.device != device:
            self._kept_slots = torch.zeros(4096, dtype=torch.int64, device=device)
            self._slot_totals = []
        i = len(self._slot_totals) % self._kept_slots.numel()
        if i == 0 and self._slot_totals:
            self._fold_slots()
            i = 0
        return self._kept_slots[i:i + 1]

    def _fold_slots(self):
        kept = self._kept_slots[:len(self._slot_totals)].double().cpu().numpy()
        tot = np.asarray(self._slot_totals, dtype=np.float64)
        self._folded = getattr(self, "_folded", 0.0) + float(np.sum(1.0 - kept / tot - 1.0 / self.sample_gap))
        self._kept_slots.zero_()
        self._slot_totals = []

    @property
    def sparsity(self) -> float:
        """Average reported sparsity 1 - mean(mask) - 1/sample_gap over all calls (:394, :415).
        Reading it synchronises once; the forward never does."""
        if self.sparsity_counter == 0:
            return 0.0
        if self._slot_totals:
            self._fold_slots()
        return getattr(self, "_folded", 0.0) / self.sparsity_counter

    def _log_gap(self, dtype) -> float:
        """ln(gap) as the reference computes it: torch.log of a tensor in the LSE's storage
        dtype (lse is cast to q.dtype at :324, the log taken in it at :375-376), i.e. 2.703125
        for g=15 in bf16. The training path's combine rounds it the same way (vb_pool.hip)."""
        return float(torch.log(torch.tensor(float(self.sample_gap), dtype=dtype)).item())

    def _per_head(self, name, value, B, H, nb, device):
        """[B,H] device tensor of a per-head option given as a tensor [H] or [B,H]: kept-block
        counts (int32) of a retain ratio, by ``retain_counts``' arithmetic on the device (cog:
        clamp((nb * fp32 ratio).to(int32), min=1), cogvideo_blocksparseattn.py:230-231; wan: the
        same in float64, the Python float of wanx :215-216), or the fp32 thresholds. Built once per
        (tensor, B, H, nb, device) and cached, so a steady-state call launches nothing for it."""
        key = (name, B, H, nb, str(device))
        hit = self._per_head_cache.get(key)
        if hit is not None and hit[0] is value and hit[1] == value._version:
            return hit[2]
        if value.dim() not in (1, 2) or value.shape[-1] != H or (value.dim() == 2 and value.shape[0] != B):
            raise ValueError(f"{name} must be a float or a tensor [H] or [B,H] = [{B},{H}], "
                             f"got {tuple(value.shape)}")
        v = value.detach().to(device)
        if name == "energy_threshold":
            out = v.float()
        else:
            v = v.float() if self.variant == "cog" else v.double()
            out = torch.clamp((nb * v).to(torch.int32), min=1)
        out = out.expand(B, H).contiguous()
        self._per_head_cache[key] = (value, value._version, out)
        return out

    def _judge_rows(self, device):
        r = self.judge_rows
        if r.device != device or r.dtype != torch.int32:
            r = r.to(device=device, dtype=torch.int32)
            self.judge_rows = r
        return r

    def _judge_budget(self, q, k, nb, judge_rows=None):
        """head_budget="judge": this call's per-head max_keep counts, int32 [B,H] on the device, from
        the estimator on the q and k received (caller row order). Two launches for the estimator and
        one for the budget rule, all on the current stream, before the predictor's."""
        rows = self._judge_rows(q.device) if judge_rows is None else judge_rows
        sparsity = ops.judge_sparsity(q, k, rows, key_stride=self.judge_key_stride, top=self.judge_top)
        budget = ops.head_budget(sparsity, nb, self.max_retain_ratio, self.judge_clamp, self.variant)
        self.last_head_sparsity, self.last_head_budget = sparsity, budget
        return budget

    def _probe_recall(self, q, k, mask, rows):
        """probe="recall": ops.mask_recall on this call's q, k and the mask its attention launch uses.
        Three launches on the current stream; the results stay on the device."""
        pos = self.probe_pos
        if pos.device != q.device or pos.dtype != torch.int32:
            pos = pos.to(device=q.device, dtype=torch.int32)
            self.probe_pos = pos
        with torch.no_grad():
            rec, ora = ops.mask_recall(q.detach(), k.detach(), mask, pos, rows=rows)
            if self._recall_sums is None or self._recall_sums.shape[1:] != rec.shape \
                    or self._recall_sums.device != rec.device:
                self._recall_sums = torch.zeros(2, *rec.shape, device=rec.device, dtype=torch.float32)
                self._recall_count = 0
            self._recall_sums[0].add_(rec)
            self._recall_sums[1].add_(ora)
        self._recall_count += 1
        self.last_recall, self.last_oracle_recall = rec, ora

    @property
    def recall(self):
        """(recall, oracle recall): fp32 [B,H] means over the probed calls, or None before the first.
        Reading it synchronises once; the forward never does."""
        if self._recall_sums is None or self._recall_count == 0:
            return None
        mean = (self._recall_sums / self._recall_count).cpu()
        return mean[0], mean[1]

    def _probe_fidelity(self, q, k, v, out):
        """probe="fidelity": ops.attn_fidelity on this call's q, k, v and the output it returns. Three
        launches on the current stream; the results stay on the device."""
        probe_fidelity(self, q, k, v, out)

    @property
    def fidelity(self):
        """Per-head SNR in dB of the output against dense attention, fp32 [B,H], from the sums of sig and
        err over the probed calls, or None before the first. Reading it synchronises once; the forward
        never does."""
        return fidelity_snr(self)

    def _mask_rule(self, B, H, nb, device, max_keep=None):
        """The ops.MaskRule of a call, or None when the options are the scalar energy rule's.
        ``max_keep``: the judge's int32 [B,H] counts, in place of max_retain_ratio's."""
        if self.mask_mode == "topk":
            k0 = int(nb * self.init_k) if self.init_k < 1 else int(self.init_k)
            return ops.MaskRule(mode="topk", init_k=k0)
        per_head = {n: v for n, v in (("min_keep", self.min_retain_ratio), ("max_keep", self.max_retain_ratio),
                                      ("energy_threshold", self.energy_threshold))
                    if isinstance(v, torch.Tensor)}
        if not per_head and max_keep is None:
            return None
        names = {"min_keep": "min_retain_ratio", "max_keep": "max_retain_ratio",
                 "energy_threshold": "energy_threshold"}
        fields = {n: self._per_head(names[n], v, B, H, nb, device) for n, v in per_head.items()}
        if max_keep is not None:
            fields["max_keep"] = max_keep
        return ops.MaskRule(mode="energy", **fields)

    # -------------------------------------------------------------------------------- forward
    def predict_mask(self, q, k, q_off=None, k_off=None, count=None, staged_event=None, pool=None,
                     rows_kept=None, judge_rows=None):
        """Block mask [B,H,nb,nb] (uint8, Gilbert order) and normalised pooled scores. ``pool``
        (v, gap, outs) runs the pooled K/V pass inside the score kernel's launch. ``judge_rows``
        overrides the module's probe rows for this call (head_budget="judge")."""
        B, H, L, D = q.shape
        # the judge's workspace is allocated (and its launches enqueued) before the predictor's
        # temporaries exist
        budget = None
        if self.head_budget == "judge":
            budget = self._judge_budget(q, k, (L + self.block - 1) // self.block, judge_rows)
        if self.score == "mass":
            if pool is not None or staged_event is not None:
                raise ValueError("score='mass': the pooled K/V pass is its own launch (ops.pool_kv); "
                                 "pool= and staged_event= belong to the max predictor's launch")
            return self._predict_mask_mass(q, k, q_off, k_off, count, rows_kept, budget)
        rand = philox = None
        if q_off is None and k_off is None:
            # the reference's two draws (:77-78, q first), generated and ranked inside the sampling
            # launch at the device generator's Philox state (the values torch.rand would return)
            philox = ops.claim_rand_draws(q.device, B * H * self.block)
            if philox is None:
                rand = (torch.rand(B, H, 1, self.block, device=q.device),
                        torch.rand(B, H, 1, self.block, device=q.device))
        elif q_off is None:
            q_off = draw_sample_offsets(B, H, q.device, self.block, self.num_keep)
        elif k_off is None:
            k_off = draw_sample_offsets(B, H, q.device, self.block, self.num_keep)
        nb = (L + self.block - 1) // self.block
        rule = self._mask_rule(B, H, nb, q.device, budget)
        if rule is not None:
            # scalars of the options given as tensors are placeholders the rule's arrays replace
            thr = 0.95 if isinstance(self.energy_threshold, torch.Tensor) else self.energy_threshold
            lo, hi = retain_counts(nb, 1.0 if isinstance(self.min_retain_ratio, torch.Tensor) else self.min_retain_ratio,
                                   1.0 if isinstance(self.max_retain_ratio, torch.Tensor) else self.max_retain_ratio,
                                   self.variant)
            return ops.mask_predict(q, k, q_off, k_off, rows=self._rows(q.device), energy_threshold=thr,
                                    min_keep=lo, max_keep=hi, force_tail=self.force_tail, mask_count=count,
                                    staged_event=staged_event, rand=rand, philox=philox, pool=pool,
                                    rows_kept=rows_kept, num_keep=self.num_keep, rule=rule)
        lo, hi = retain_counts(nb, self.min_retain_ratio, self.max_retain_ratio, self.variant)
        po, mask = ops.mask_predict(q, k, q_off, k_off, rows=self._rows(q.device),
                                    energy_threshold=self.energy_threshold, min_keep=lo,
                                    max_keep=hi, force_tail=self.force_tail, mask_count=count,
                                    staged_event=staged_event, rand=rand, philox=philox,
                                    pool=pool, rows_kept=rows_kept, long_rows=nb > ops.MAX_BLOCKS,
                                    num_keep=self.num_keep)
        return po, mask

    def _predict_mask_mass(self, q, k, q_off, k_off, count, rows_kept, budget):
        """score="mass": the reference's two draws by torch.rand (q first: the values and the generator
        state of the default path), then ops.sample_offsets -> ops.mask_scores_mass ->
        ops.block_mask_rule with the call's rule."""
        B, H, L, D = q.shape
        nb = (L + self.block - 1) // self.block
        if q_off is None and k_off is None:
            q_off, k_off = draw_sample_offsets_qk(B, H, q.device, self.block, self.num_keep)
        elif q_off is None:
            q_off = draw_sample_offsets(B, H, q.device, self.block, self.num_keep)
        elif k_off is None:
            k_off = draw_sample_offsets(B, H, q.device, self.block, self.num_keep)
        po = ops.mask_scores_mass(q, k, q_off, k_off, rows=self._rows(q.device))
        rule = self._mask_rule(B, H, nb, q.device, budget)
        thr, lo_r, hi_r = self.energy_threshold, self.min_retain_ratio, self.max_retain_ratio
        if rule is not None:
            # scalars of the options given as tensors are placeholders the rule's arrays replace
            thr = 0.95 if isinstance(thr, torch.Tensor) else thr
            lo_r = 1.0 if isinstance(lo_r, torch.Tensor) else lo_r
            hi_r = 1.0 if isinstance(hi_r, torch.Tensor) else hi_r
        lo, hi = retain_counts(nb, lo_r, hi_r, self.variant)
        mask = ops.block_mask_rule(po, rule, energy_threshold=thr, min_keep=lo, max_keep=hi,
                                   force_tail=self.force_tail, mask_count=count, rows_kept=rows_kept)
        return po, mask

    def forward(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, *,
                q_off: Optional[torch.Tensor] = None, k_off: Optional[torch.Tensor] = None,
                block_mask: Optional[torch.Tensor] = None,
                judge_rows=None) -> torch.Tensor:
        B, H, L, D = q.shape
        if k.shape != q.shape or v.shape != q.shape:
            # the reference's index_select over the Gilbert index fails on a shorter k/v (e.g. the
            # Wan I2V image keys); every launch below assumes q's [B,H,L,D] for k and v
            raise ValueError(f"k and v must have q's shape {tuple(q.shape)}, got "
                             f"{tuple(k.shape)} and {tuple(v.shape)}")
        if self.use_rearrange and L != self.gilbert_rearranger.seq_len:
            raise ValueError(f"sequence length {L} != {self.gilbert_rearranger.seq_len} expected "
                             f"by the Gilbert grid (width/height/depth/text_length)")
        rows = self._rows(q.device)
        nb = (L + self.block - 1) // self.block
        count = self._count_slot(q.device)
        grad = torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad)
        fused = not grad and self.combine != "reference"
        # grad_combine="joint": the inference call under autograd (one softmax, its exact gradient)
        joint = grad and self.grad_combine == "joint"
        pooled = None
        rows_kept = None
        if block_mask is None:
            # inference: the pooled K/V pass (one pass over K/V: pooled K/V + the Gilbert-ordered
            # contiguous copies the attention kernel streams by LDS-DMA; HBM-bound) runs inside the
            # predictor's score-kernel launch, beside the MFMA-bound score workgroups (overlap=True),
            # or after it (overlap=False)
            ride = (fused or joint) and self.overlap and self.score == "max"
            gather = self._gather(D)
            # the joint backward reads k/v in reordered order: its copies are always taken
            copies = joint or not (gather and rows is not None)
            outs = ops.pool_kv_outputs(k, self.sample_gap, reordered=copies) if ride else None
            if fused and self.order and self.mask_head_mode == "per_head":
                rows_kept = torch.empty(B, H, nb, device=q.device, dtype=torch.int32)
            with torch.no_grad():
                _, mask = self.predict_mask(q.detach(), k.detach(), q_off, k_off, count,
                                            pool=(v, self.sample_gap, outs) if ride else None,
                                            rows_kept=rows_kept, judge_rows=judge_rows)
            if ride:
                pooled = outs
            elif fused or joint:
                pooled = ops.pool_kv(k, v, self.sample_gap, rows, reordered=copies)
        else:
            mask = block_mask.to(torch.uint8)
            count.add_(mask.sum())
            if joint:
                pooled = ops.pool_kv(k, v, self.sample_gap, rows, reordered=True)
            elif fused:
                gather = self._gather(D)
                pooled = ops.pool_kv(k, v, self.sample_gap, rows, reordered=not (gather and rows is not None))
        self._slot_totals.append(B * H * nb * nb)
        self.sparsity_counter += 1
        self.last_mask = mask
        if self.mask_head_mode == "shared_head0":
            # head_mask_type's ones read literally: every head uses base_blockmask head 0 (a
            # head-stride-0 view; the kernels index the mask through its strides)
            mask = mask[:, :1].expand(B, H, mask.shape[2], mask.shape[3])
        probing = False
        if self._probes:
            probing = self._probe_calls % self.probe_every == 0
            if probing and "recall" in self._probes:
                self._probe_recall(q, k, mask, rows)
            self._probe_calls += 1
        if joint:
            from .autograd import adaptive_joint_attention
            out = adaptive_joint_attention(q, k, v, mask, rows, self.sample_gap, self._log_gap(q.dtype),
                                           heavy_rows=self.force_tail, pooled=pooled, io_layout=self.io_layout)
        elif not fused:
            from .autograd import adaptive_split_attention
            out = adaptive_split_attention(q, k, v, mask, rows, self.sample_gap,
                                           heavy_rows=self.force_tail, io_layout=self.io_layout)
        else:
            # q rows gathered and out rows scattered inside the attention kernel
            if len(pooled) == 4:   # Gilbert-ordered copies: streamed contiguously
                kp, vp, k_src, v_src = pooled
                kv_rows = None
            else:                  # the caller's k/v, rows gathered through the Gilbert index
                kp, vp = pooled
                k_src, v_src, kv_rows = k, v, rows
            ev = self.attn_events
            if ev is not None:
                self._attn_launches += 1
                if (self._attn_launches - 1) % self.attn_event_every:
                    ev = None
            if ev is not None:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            out = ops.attention_fwd(q, k_src, v_src, block_mask=mask, q_rows=rows, kv_rows=kv_rows,
                                    kp=kp, vp=vp, kp_log_bias=self._log_gap(q.dtype),
                                    heavy_rows=self.force_tail, order=self.order, q_lengths=rows_kept,
                                    order_window=self.order_window, persistent=self.persistent,
                                    out_layout=self.io_layout)
            if ev is not None:
                e1 = torch.cuda.Event(enable_timing=True)
                e1.record()
                ev.append((e0, e1))
        if probing and "fidelity" in self._probes:
            self._probe_fidelity(q, k, v, out)
        if self.log_every and self.sparsity_counter % self.log_every == 0:
            print(f"sparsity: {self.sparsity}")
        return out


# reference-named alias (the patch functions install one shared instance on every block)
AdaptiveBlockSparseAttnTrain = AdaptiveBlockSparseAttn
