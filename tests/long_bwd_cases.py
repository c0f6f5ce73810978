"""The case table of the backward past 256 blocks, shared by test_long_bwd_ref.py (CPU: the gathered
reference against the dense one, the mutations the per-row bound must see, the reseed conditions)
and test_gpu_long_backward.py (GPU: vb_attn_fwd's training launch and vb_attn_bwd against the
gathered fp64 reference). Not a test module.

Past 256 blocks the default dK/dV and dQ kernels (csrc/vb_attn_bwd_kv.hip) build their block lists
in more than one round: wave w ballots the 64-block chunks w, w + 4, w + 8, w + 12 and places each
chunk's entries after the counts of the chunks before it. Shapes, the smallest that reach each regime:
  S1  L = 257 * 128 + 17 = 32913   258 blocks: chunk 4 (wave 0's second round) holds two blocks; the
                                    last block has 17 rows, so its second half-tile is skipped
  S2  L = 75600                     591 blocks (Wan 720p), a last block of 80 rows: both half-tiles run
  S3  L = 131072                    1024 blocks, the limit: every wave runs four full rounds

Masks (long_mask): every row keeps its diagonal block and 3 random blocks; on top, the designed
lists of ``designed_lists`` stand exactly, as mask rows (the dQ kernels' key lists) in head 0 and as
mask columns (the dK/dV kernels' q-lists) in head 1, so that no designed row crosses a designed
column. With H = 1 both go into the one head: columns are written over rows, the full row again,
then the empty row and the unkept column are cleared, so a crossing list there differs from its
design in those entries (the full lists hold every block but one).
"""
import dataclasses
import functools
import math
import types

import numpy as np
import torch

import bsa_oracle as O

BF16, F16 = torch.bfloat16, torch.float16
S1, S2, S3 = 257 * 128 + 17, 75600, 131072
LIST_NAMES = ("lanes", "ends", "last", "full", "from256", "random30", "empty")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    L: int
    D: int
    dtype: torch.dtype = BF16
    H: int = 2
    gap: int = 0              # > 0: the two-branch form with this pooling gap
    rows: bool = False        # random q_rows / kv_rows tables
    heads: tuple = None       # the heads the reference runs on (None: all); inputs drawn on the device
    run: bool = True          # False: kept in the table, not run (DESIGN.md §4 says why)
    seed: int = 0

    @property
    def id(self):
        return f"{self.name}-D{self.D}-{'bf16' if self.dtype == BF16 else 'f16'}"

    @property
    def nb(self):
        return (self.L + 127) // 128


MAIN = (
    Case("S1", S1, 64, BF16, seed=8103),
    Case("S1", S1, 128, BF16, seed=8110),
    Case("S1", S1, 64, F16, seed=8120),
    Case("S1", S1, 128, F16, seed=8130),
    Case("S2", S2, 128, BF16, seed=8200),
    Case("S3", S3, 64, BF16, seed=8300),
)
ROWS = Case("S1-rows", S1, 64, BF16, rows=True, seed=8400)
TWO_BRANCH = Case("S1-gap15", S1, 64, BF16, H=1, gap=15, seed=8500)
# one pooled q-range of 258 blocks: pool_split (csrc/vb_attn_bwd_host.cpp) gives psplit = 1 from
# nbkp * H >= 2049; Lkp = ceil(32913 / 7) = 4702, nbkp = 37, 37 * 56 = 2072
POOLED_ONE_RANGE = Case("S1-gap7-H56", S1, 64, BF16, H=56, gap=7, heads=(0, 28, 55), seed=8600)
CASES = MAIN + (ROWS, TWO_BRANCH, POOLED_ONE_RANGE)

# Cases whose first draw puts the rounding emulation's worst row above half of O.PER_ROW_CAP (a
# condition on the CPU emulation alone, as fwd_cases.RESEED): they draw from seed + 100000 instead.
# test_long_bwd_ref.py asserts the listed draws under the cap. None needed it.
RESEED = {}


def designed_lists(nb, seed):
    """name -> sorted block indices in [0, nb): the lists the four-wave ballot can get wrong.
      lanes     lane 0 and lane 63 of every chunk (64c, 64c + 63)
      ends      entries only in chunk 0 and in the last chunk (its first block and the last block among them)
      last      the last block alone
      full      every block
      from256   every block from 256 up (chunks 0-3, every wave's first round, are empty)
      random30  a random 30 %
      empty     nothing"""
    g = torch.Generator().manual_seed(seed)
    last_chunk = (nb - 1) // 64
    lanes = sorted({x for c in range(last_chunk + 1) for x in (64 * c, 64 * c + 63) if x < nb})
    lo = torch.nonzero(torch.rand(64, generator=g) < 0.2).flatten().tolist()
    tail = list(range(64 * last_chunk, nb))
    hi = [tail[i] for i in torch.nonzero(torch.rand(len(tail), generator=g) < 0.5).flatten().tolist()] + [tail[0], tail[-1]]
    return dict(lanes=lanes, ends=sorted(set(lo or [0]) | set(hi)), last=[nb - 1], full=list(range(nb)),
                from256=list(range(256, nb)), random30=torch.nonzero(torch.rand(nb, generator=g) < 0.3).flatten().tolist(),
                empty=[])


def designed_at(nb):
    """name -> the mask row (and the mask column) that carries the list: spread over the chunks, none
    of them the last block (the last row and column keep their diagonal for the half-tile rule)."""
    step = (nb - 2) // len(LIST_NAMES)
    return {n: 1 + i * step for i, n in enumerate(LIST_NAMES)}


@functools.lru_cache(maxsize=None)
def long_mask(nb, H, seed, layout="split"):
    """bool [1, H, nb, nb]. ``layout``: "split" (H >= 2: designed rows in head 0, designed columns in
    head 1, both exact), "one" (H = 1, see the module docstring) or "spread" (H >= 3: rows in the
    first head, columns in the middle one, the last head keeps the random base alone)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.zeros(1, H, nb, nb, dtype=torch.bool)
    m.scatter_(3, torch.randint(0, nb, (1, H, nb, 3), generator=g), True)
    m |= torch.eye(nb, dtype=torch.bool)
    lists, at = designed_lists(nb, seed + 1), designed_at(nb)
    row_head, col_head = {"split": (0, 1), "one": (0, 0), "spread": (0, H // 2)}[layout]

    def line(name):
        x = torch.zeros(nb, dtype=torch.bool)
        x[lists[name]] = True
        return x

    for n in LIST_NAMES:
        m[0, row_head, at[n], :] = line(n)
    for n in LIST_NAMES:
        m[0, col_head, :, at[n]] = line(n)
    if row_head == col_head:
        m[0, row_head, at["full"], :] = True
        m[0, row_head, at["empty"], :] = False
        m[0, col_head, :, at["empty"]] = False
    return m


def mask_of(c):
    layout = "one" if c.H == 1 else "split" if c.H == 2 else "spread"
    return long_mask(c.nb, c.H, c.seed + 4, layout)


def _rand(*shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


@functools.lru_cache(maxsize=4)
def build(c):
    """Unit-normal q, k, v, dO [1,H,L,D] in the storage dtype (LOGICAL row order, the order the oracle
    works in), the mask, alpha (two-branch: a random constant in [0.01, 0.99] per row) and the row
    tables (logical position -> caller row). Cases with ``heads`` draw on the device instead (the GPU
    file does), so they have no CPU build."""
    assert c.heads is None
    seed = c.seed + 100000 * RESEED.get(c.id, 0)
    d = types.SimpleNamespace(case=c, mask=mask_of(c), scale=1.0 / math.sqrt(c.D), alpha=None, Pq=None, Pk=None)
    d.q, d.k, d.v, d.do = (_rand(1, c.H, c.L, c.D, dtype=c.dtype, seed=seed + s) for s in range(4))
    if c.gap:
        d.alpha = torch.rand(1, c.H, c.L, generator=torch.Generator().manual_seed(seed + 5)) * 0.98 + 0.01
    if c.rows:
        d.Pq = torch.randperm(c.L, generator=torch.Generator().manual_seed(seed + 10))
        d.Pk = torch.randperm(c.L, generator=torch.Generator().manual_seed(seed + 11))
    return d


# ----------------------------------------------------------------------------------------------
# forward: the rule of tests/fwd_cases.py, per q-block on gathered keys
# ----------------------------------------------------------------------------------------------
LSE_CAP, LSE_FACTOR = 2e-5, 8.0      # fwd_cases.LSE_CAP, LSE_FACTOR


def forward_reference(q, k, v, mask, dtype, *, inference=False):
    """fp64 reference, the rounding emulation of the launch (training: the LSE-returning form;
    ``inference``: the pre-scaled-query form) and the bounds of test_gpu_forward_rows.py: every row
    within 2 x the emulation's worst row (O.per_row_bound, capped), the whole tensor within 2 x the
    emulation's Frobenius error, the LSE within 8 x the fp32 emulation's error and at most 2e-5.
    Unit-normal inputs at the default scale: no row is owned by one key, so no row gets the lagging
    rows' wider bound (fwd_cases.row_bounds).

    The inference form rounds q * scale * log2(e) to the storage type before the scores. Over the
    262144 rows of S3, most of them with 512 keys, that rounding alone puts 41 .. 58 rows of every
    draw above half of O.PER_ROW_CAP against the true reference (worst row 6.8e-3 .. 8.6e-3 bf16 in four
    draws), so no reseed can bring 2 x the worst row under the cap. Such a launch (``r.prescaled``) is
    judged per row against the fp64 reference on the pre-scaled query (sm_scale = ln 2), the
    forward's rule for launches whose pre-scale rounding alone takes more than half the cap
    (fwd_cases.reference), where the emulation's worst row is 3.5e-3; its whole tensor is still
    held to 2 x the emulation's Frobenius error against the TRUE reference (``r.whole_true``)."""
    r = types.SimpleNamespace(prescaled=False)
    r.ref, r.ref_lse = O.gathered_attention(q, k, v, mask)
    r.emu, r.emu_lse = O.gathered_attention(q, k, v, mask, emulate=dict(store_dtype=dtype, prescale_q=inference))
    r.true_ref, r.whole_true = r.ref, frob(r.emu, r.ref)
    r.emu_err = O.per_row_error(r.emu, r.ref)[0]
    if inference and 2.0 * r.emu_err > O.PER_ROW_CAP[dtype]:
        D = q.shape[-1]
        qs = (q.float() * float(np.float32(1.0 / math.sqrt(D)) * O.LOG2E_F32)).to(q.dtype)   # fwd_cases.prescaled_query
        r.prescaled = True
        r.ref, _ = O.gathered_attention(qs, k, v, mask, sm_scale=math.log(2.0))
        r.emu_err = O.per_row_error(r.emu, r.ref)[0]
    r.row_bound = O.per_row_bound(r.emu, r.ref, dtype)
    r.whole_emu = frob(r.emu, r.ref)
    fin = torch.isfinite(r.ref_lse)
    assert torch.equal(fin, torch.isfinite(r.emu_lse))
    r.lse_emu_err = float((r.emu_lse.double() - r.ref_lse)[fin].abs().max())
    assert r.lse_emu_err > 0
    r.lse_bound = min(LSE_FACTOR * r.lse_emu_err, LSE_CAP)
    return r


def cpu_statistics(d):
    """Stand-ins for the device forward's out and lse on a CPU-only box: the training launch's
    rounding emulation (out in the storage dtype, lse fp32)."""
    out, lse = O.gathered_attention(d.q, d.k, d.v, d.mask, emulate=dict(store_dtype=d.case.dtype))
    return out.to(d.case.dtype), lse


def backward_reference(q, k, v, do, out, lse, mask, dtype, *, kp=None, vp=None, out2=None, lse2=None, alpha=None, gap=0):
    """(ref, emu): two_branch_attention_bwd's gathered form, unrounded and with the kernels' roundings."""
    args = (q, k, v, kp, vp, out, lse, out2, lse2, alpha, do, mask, gap)
    ref = O.two_branch_attention_bwd(*args, store_dtype=dtype, gathered=True)
    emu = O.two_branch_attention_bwd(*args, store_dtype=dtype, gathered=True, emulate_rounding=True)
    return ref, emu


def frob(x, ref):
    ref = ref.double()
    return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-300))
