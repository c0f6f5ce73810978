"""The multi-level forward's row-parity case table, shared by test_ml_oracle_forward.py (CPU: the
bounds' own checks) and test_gpu_ml_forward_rows.py (GPU: vb_ml_attn_fwd against those bounds). Not
a test module; the twin of fwd_cases.py, whose constants, bound rules and reseed rule it reuses.

A case is a frozen ``Case``; ``build(case)`` draws its inputs (CPU tensors in LOGICAL, i.e.
reordered, row order; the GPU file scatters q, k, v to caller order through the one row table the
multi-level op takes) and ``reference(case)`` adds the fp64 reference
(ml_oracle.multilevel_attention_fp64), both rounding emulations
(ml_oracle.multilevel_attention_fwd_emulated) and the bounds derived from them. Both are cached.

Groups (the kML arm of attn_fwd_item, csrc/vb_attn_fwd.hip):
  a  every instantiation: D x dtype, LSE-returning and inference, plain and persistent
  b  tile packing: n4 in 1..5 and n8 in 1..7, 9, 10, alone and beside other levels (PACK tables)
  c  tails: L = 256 + r with the last column at every level, both tail rules; one-block lengths
  d  the I/O surface: out= view, strided q, out_layout, stride-0 and strided masks
  e  values: scale=, non-level mask bytes, an all-skip row
  f  late maxima: an owning key in a later level-1, a level-2, a packed level-4 and level-8 tile
  g  key lists longer than one 64-lane ballot pass (67 blocks), three q-blocks referenced
"""
import dataclasses
import functools
import math
import types

import torch

import bsa_oracle as O
import fwd_cases as F
import ml_oracle as ML
from fwd_cases import BF16, DTYPES, F16, HUGE, LSE_CAP, LSE_FACTOR, MILD, SLACK, TWO   # noqa: F401
from test_gpu_ml_backward import MIX, _random_levels

BLOCK = ML.BLOCK
TAILS = (1, 3, 63, 64, 65, 69, 96, 127)        # L = 256 + r
ONE_BLOCK = (1, 40, 64, 65, 127)               # nb = 1
LONG_L = 8500                                  # 67 blocks: the ballot loops take a second pass
LONG_QBLOCKS = (0, 33, 66)

# b. One configuration per q-block of L = 1280 (10 key blocks). PACK_ALONE: a row holds one level
# only; PACK_BESIDE: level-4 and level-8 lists beside each other and beside levels 1 and 2. The kept
# blocks sit first, last and scattered, so both (wave & 1) halves of a packed tile and the
# min(e, n - 1) clamps of a short last tile read real and clamped list entries.
PACK = {
    "alone1": (
        (4, 0, 0, 0, 0, 0, 0, 0, 0, 0),     # n4 = 1, first
        (0, 0, 0, 0, 0, 0, 0, 0, 4, 4),     # n4 = 2, last
        (4, 0, 0, 4, 0, 0, 0, 4, 0, 0),     # n4 = 3, scattered
        (4, 4, 4, 4, 0, 0, 0, 0, 0, 0),     # n4 = 4, first
        (0, 4, 0, 4, 4, 0, 4, 0, 0, 4),     # n4 = 5, scattered and last
        (0, 0, 0, 0, 0, 0, 0, 0, 0, 8),     # n8 = 1: a single level-8 block (16 keys), last
        (8, 8, 0, 0, 0, 0, 0, 0, 0, 0),     # n8 = 2, first
        (0, 8, 0, 0, 8, 0, 0, 0, 8, 0),     # n8 = 3, scattered
        (0, 0, 0, 0, 0, 0, 8, 8, 8, 8),     # n8 = 4, last
        (8, 0, 8, 0, 8, 0, 8, 0, 8, 0),     # n8 = 5, scattered
    ),
    "alone2": (
        (8, 8, 8, 8, 8, 8, 0, 0, 0, 0),     # n8 = 6, first
        (0, 0, 0, 8, 8, 8, 8, 8, 8, 8),     # n8 = 7, last
        (8, 8, 8, 8, 0, 8, 8, 8, 8, 8),     # n8 = 9
        (8, 8, 8, 8, 8, 8, 8, 8, 8, 8),     # n8 = 10
        (0, 0, 0, 0, 0, 1, 0, 0, 0, 0),     # a single level-1 block
        (0, 0, 2, 0, 0, 0, 0, 0, 0, 0),     # a single level-2 block
        (8, 0, 0, 0, 0, 0, 0, 0, 0, 0),     # a single level-8 block, first
        (0, 0, 0, 0, 0, 0, 4, 0, 0, 0),     # n4 = 1, in the middle
        (4, 4, 0, 0, 0, 0, 0, 0, 0, 0),     # n4 = 2, first
        (0, 0, 0, 0, 0, 0, 0, 4, 4, 4),     # n4 = 3, last
    ),
    "beside": (
        (8, 8, 8, 8, 4, 8, 8, 8, 8, 8),     # n4 = 1, n8 = 9
        (4, 8, 8, 8, 1, 8, 8, 8, 8, 4),     # n4 = 2, n8 = 7, one level-1
        (8, 4, 8, 2, 8, 4, 8, 8, 4, 8),     # n4 = 3, n8 = 6, one level-2
        (4, 4, 8, 8, 0, 8, 8, 8, 4, 4),     # n4 = 4, n8 = 5
        (8, 4, 4, 4, 1, 4, 4, 8, 8, 8),     # n4 = 5, n8 = 4, one level-1
        (1, 2, 4, 8, 4, 8, 4, 8, 4, 4),     # n4 = 5, n8 = 3, levels 1 and 2
        (8, 1, 4, 2, 4, 0, 2, 4, 1, 8),     # n4 = 3, n8 = 2, two of level 1 and of level 2
        (0, 0, 2, 0, 0, 8, 0, 0, 0, 4),     # n4 = 1, n8 = 1, one level-2
        (2, 4, 4, 0, 0, 0, 0, 0, 8, 1),     # n4 = 2, n8 = 1, levels 2 and 1
        (1, 0, 8, 8, 0, 4, 4, 4, 4, 2),     # n4 = 4, n8 = 2, levels 1 and 2
    ),
}

# f. Every q-block's mask row: level-1 blocks 0, 1 (tiles 0..3), the level-2 block 2 (tile 4), the
# level-4 blocks 3, 4 (packed into tile 5) and the level-8 blocks 5..8 (packed into tile 6).
LATE_ROW = (1, 1, 2, 4, 4, 8, 8, 8, 8, 0)
# (query row, level p, first of the p aligned level-1 keys set to the spike): the pooled row of
# level p over those keys equals the spike exactly (a mean of equal storage values)
LATE = {
    "l1-later-tile": (5, 1, 128 + 64 + 40),
    "l2-tile": (6, 2, 2 * 128 + 40),
    "l4-second-block": (7, 4, 4 * 128 + 40),
    "l8-third-block": (8, 8, 7 * 128 + 40),
}


@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    name: str
    D: int
    dtype: torch.dtype
    B: int
    H: int
    L: int
    mask: str                 # mix | tailcol | one | alone1 | alone2 | beside | h_expanded | nonlevel | late | long
    ref_tail: bool = True
    scale: float = None
    q_rows: bool = False      # a row permutation (q, out and the pyramids' source rows)
    spikes: tuple = ()        # ((query row, level, first key of the aligned run, target log2 score), ...)
    io: str = ""              # out_view | q_strided | blhd | mask_h_expanded | mask_strided
    persistent: bool = False  # every launch is repeated with persistent=True (bit-identical)
    q_blocks: tuple = ()      # the q-blocks that get a reference (empty: all); the rest: finite only
    seed: int = 0

    @property
    def id(self):
        return f"{self.group}-{self.name}-D{self.D}-{'bf16' if self.dtype == BF16 else 'f16'}"

    @property
    def unit(self):
        """Scores of unit deviation (fwd_cases.Case.unit): no spike, the default scale."""
        return not (self.spikes or self.scale is not None)

    @property
    def nb(self):
        return (self.L + BLOCK - 1) // BLOCK


def _cases():
    out = []
    for D, dt in DTYPES:
        # a. 9 blocks, a 76-row tail, the backward file's level mix; ref_tail False on half the grid
        out.append(Case("a", "L1100", D, dt, 2, 2, 1100, "mix", ref_tail=(D == 64) == (dt == BF16), q_rows=True,
                        persistent=True, seed=1000))
    for D, dt in TWO:
        for name in PACK:
            out.append(Case("b", name, D, dt, 1, 1, 1280, name, seed=2000))
        for ref_tail in (True, False):
            tag = "ref" if ref_tail else "masked"
            for r in TAILS:
                out.append(Case("c", f"L{256 + r}-{tag}", D, dt, 2, 2, 256 + r, "tailcol", ref_tail=ref_tail,
                                seed=3000 + r))
            for L in ONE_BLOCK:
                out.append(Case("c", f"L{L}-{tag}", D, dt, 2, 2, L, "one", ref_tail=ref_tail, seed=3500 + L))
        for i, io in enumerate(("out_view", "q_strided", "blhd", "mask_h_expanded", "mask_strided")):
            out.append(Case("d", io.replace("_", "-"), D, dt, 2, 3, 300, "h_expanded" if io == "mask_h_expanded" else "mix",
                            q_rows=io in ("out_view", "blhd"), io=io, seed=4000 + i))
        out.append(Case("e", "scale0.2", D, dt, 1, 2, 600, "mix", scale=0.2, seed=5000))
        out.append(Case("e", "scale0.05", D, dt, 1, 2, 600, "mix", scale=0.05, ref_tail=False, seed=5001))
        out.append(Case("e", "nonlevel-bytes", D, dt, 1, 2, 600, "nonlevel", seed=5002))
        out.append(Case("g", "L8500", D, dt, 1, 1, LONG_L, "long", ref_tail=dt == BF16, q_blocks=LONG_QBLOCKS, seed=7000))
    for D, dt in DTYPES:
        for place, (row, p, j0) in LATE.items():
            for tag, T in (("mild", MILD), ("huge", HUGE[dt])):
                out.append(Case("f", f"{place}-{tag}", D, dt, 1, 2, 1280, "late", spikes=((row, p, j0, T),), seed=6000))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


CASES = _cases()

# The fwd_cases.RESEED rule: a unit-score case whose draw puts the inference emulation's worst row
# above half of PER_ROW_CAP against the true reference (the bound, twice that, must hold the cap)
# draws again, from seed + 100000 n: id -> the first n at which it does not. The bf16 inference
# emulation's worst row is 4.2e-3 .. 7.1e-3 at these shapes, around half the cap of 1e-2 itself, so
# a second draw is over it about as often as the first and some cases take several (the tails at
# D=64: about 1200 rows, many of them over 16 .. 64 pooled keys). A condition on the inputs, found
# and asserted on the CPU emulation (test_ml_oracle_forward.py: every earlier draw is over half the
# cap, the listed one is not); no kernel result enters it, no case is dropped and no bound widened.
RESEED = {
    "a-L1100-D128-bf16": 1,
    "c-L257-ref-D64-bf16": 1, "c-L259-ref-D64-bf16": 2, "c-L319-ref-D64-bf16": 7, "c-L320-ref-D64-bf16": 4,
    "c-L325-ref-D64-bf16": 11, "c-L352-ref-D64-bf16": 4,
    "c-L257-masked-D64-bf16": 1, "c-L259-masked-D64-bf16": 2, "c-L319-masked-D64-bf16": 7,
    "c-L320-masked-D64-bf16": 4, "c-L325-masked-D64-bf16": 11, "c-L352-masked-D64-bf16": 4,
    "d-out-view-D64-bf16": 1, "d-blhd-D64-bf16": 3, "d-mask-strided-D64-bf16": 1,
    "e-nonlevel-bytes-D64-bf16": 1, "g-L8500-D64-bf16": 1,
}


def by_group(group):
    return [c for c in CASES if c.group == group]


def _mask(c, seed):
    """int32 levels [B,H,nb,nb] (an expanded view of one head for h_expanded)."""
    nb = c.nb
    if c.mask == "mix":
        return _random_levels(c.B, c.H, nb, seed + 4, MIX)
    if c.mask == "h_expanded":
        return _random_levels(c.B, 1, nb, seed + 4, MIX).expand(-1, c.H, -1, -1)
    if c.mask == "tailcol":     # as test_gpu_ml_backward's case c: every level reaches the tail column
        m = _random_levels(c.B, c.H, nb, seed + 4, MIX)
        for b in range(c.B):
            for h in range(c.H):
                for i in range(nb):
                    m[b, h, i, -1] = ML.LEVELS[(i + 2 * h + b) % 4]
        return m
    if c.mask == "one":
        assert nb == 1 and c.B * c.H == 4
        return torch.tensor(ML.LEVELS, dtype=torch.int32).reshape(c.H, c.B).t().reshape(c.B, c.H, 1, 1).contiguous()
    if c.mask in PACK:
        return torch.tensor(PACK[c.mask], dtype=torch.int32).expand(c.B, c.H, nb, nb).contiguous()
    if c.mask == "late":
        return torch.tensor(LATE_ROW, dtype=torch.int32).expand(c.B, c.H, nb, nb).contiguous()
    if c.mask == "nonlevel":    # bytes that name no level keep nothing; q-block 4 of head 0 holds only such
        m = _random_levels(c.B, c.H, nb, seed + 4, MIX)
        m[:, :, 0, 1], m[:, :, 1, 2], m[:, :, 2, 0], m[:, :, 3, 3] = 3, 5, 16, 255
        m[:, 0, 4, :] = torch.tensor([3, 5, 16, 255, 0], dtype=torch.int32)
        return m
    if c.mask == "long":
        # ~70 % skips; in the referenced q-blocks columns 60..66 are all kept: every level's list has
        # entries below column 64 (asserted in test_ml_oracle_forward.py) and, over the three
        # q-blocks, at least two entries at or past it, the tail block at levels 1, 4 and 8
        m = _random_levels(c.B, c.H, nb, seed + 4, (0.075, 0.075, 0.075, 0.075, 0.7))
        hi = {0: (8, 4, 1), 33: (2, 8, 4), 66: (1, 2, 8)}
        for n, (qb, lv) in enumerate(hi.items()):
            m[:, :, qb, 60:64] = torch.tensor(ML.LEVELS[n:] + ML.LEVELS[:n], dtype=torch.int32)
            m[:, :, qb, 64:67] = torch.tensor(lv, dtype=torch.int32)
        return m
    raise ValueError(c.mask)


@functools.lru_cache(maxsize=None)
def build(c, draw=None):
    """Inputs of a case in logical row order: q, k, v [B,H,L,D], mask int32 [B,H,nb,nb], the softmax
    scale, the row table (logical position -> caller row; None without one) and ``sel``, the logical
    positions of the rows that get a reference (None: all). ``draw``: that draw instead of RESEED's."""
    seed = c.seed + 100000 * (RESEED.get(c.id, 0) if draw is None else draw)
    d = types.SimpleNamespace(case=c)
    d.scale = c.scale if c.scale is not None else 1.0 / math.sqrt(c.D)
    d.q, d.k, d.v = (F._rand(c.B, c.H, c.L, c.D, dtype=c.dtype, seed=seed + s) for s in range(3))
    for r, p, j0, target in c.spikes:
        assert j0 % p == 0
        qr = d.q[:, :, r].float()
        mult = target * math.log(2.0) / (d.scale * qr.pow(2).sum(-1, keepdim=True))
        d.k[:, :, j0:j0 + p] = (qr * mult).to(c.dtype)[:, :, None]
    d.mask = _mask(c, seed)
    d.P = F._perm(c.L, seed + 10) if c.q_rows else None
    d.sel = None
    if c.q_blocks:
        d.sel = torch.cat([torch.arange(i * BLOCK, min(c.L, (i + 1) * BLOCK)) for i in c.q_blocks])
    return d


def rows_that_can_lag(qs, d, form):
    """fwd_cases.rows_that_can_lag for the multi-level forward. "Fed more than one tile":
    2 n1 (- 1 under the tail rule) + n2 + ceil(n4 / 2) + ceil(n8 / 4) > 1 (ml_oracle.ml_tiles_fed)."""
    c = d.case
    K, _, vis, b, _, _ = ML.ml_union_keys(qs, d.k, d.v, d.mask, c.ref_tail, d.sel)
    pos = torch.arange(c.L) if d.sel is None else d.sel
    tiles = ML.ml_tiles_fed(d.mask, c.L, c.ref_tail)[:, :, pos // BLOCK] > 1
    return F.lagging_rows_over_visible(qs, K, vis, b, d.scale, tiles, form, c.dtype)


@functools.lru_cache(maxsize=None)
def reference(c, draw=None):
    """fp64 reference, the emulations and the bounds of a case, over its referenced rows (``d.sel``),
    with fwd_cases.reference's fields and rules: ``ref_i`` is the true reference for every unit-score
    case; a spiked or scaled case whose inference emulation trips PER_ROW_CAP against it is judged on
    the pre-scaled query (sm_scale = ln 2). With ``draw`` (an earlier draw of a reseeded case) only the
    reference, the emulations and ``emu_i_err`` are computed."""
    d = build(c, draw)
    r = types.SimpleNamespace(d=d)
    qs = d.q if d.sel is None else d.q[:, :, d.sel]
    kw = dict(ref_tail=c.ref_tail, q_pos=d.sel)

    def emu(**x):
        return ML.multilevel_attention_fwd_emulated(qs, d.k, d.v, d.mask, sm_scale=d.scale, store_dtype=c.dtype, **kw, **x)

    r.ref, r.ref_lse = ML.multilevel_attention_fp64(qs, d.k, d.v, d.mask, sm_scale=d.scale, **kw)
    r.emu_t, r.emu_t_lse = emu()
    r.emu_i, _ = emu(prescale_q=True)
    r.emu_i_err = O.per_row_error(r.emu_i, r.ref)[0]
    if draw is not None:
        return r
    r.prescaled = not c.unit and 2.0 * r.emu_i_err > O.PER_ROW_CAP[c.dtype]
    if r.prescaled:
        r.ref_i, _ = ML.multilevel_attention_fp64(F.prescaled_query(qs, d.scale), d.k, d.v, d.mask,
                                                  sm_scale=math.log(2.0), **kw)
    else:
        r.ref_i = r.ref
    r.emu_t_err, r.emu_i_ref_err = O.per_row_error(r.emu_t, r.ref)[0], O.per_row_error(r.emu_i, r.ref_i)[0]
    r.can_t = rows_that_can_lag(qs, d, "training")
    r.can_i = rows_that_can_lag(qs, d, "inference")
    r.bounds_t, r.bound_t, r.whole_t = F.row_bounds(r.emu_t, r.ref, c.dtype, r.can_t, lambda lag: emu(m_lag=lag)[0])
    r.bounds_i, r.bound_i, r.whole_i = F.row_bounds(r.emu_i, r.ref_i, c.dtype, r.can_i,
                                                    lambda lag: emu(prescale_q=True, m_lag=lag)[0])
    r.lse_bound, r.lse_emu_err = F.lse_bound(r.emu_t_lse, r.ref_lse)
    return r
