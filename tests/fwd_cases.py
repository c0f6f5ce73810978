"""The forward row-parity case table, shared by test_oracle_forward.py (CPU: the bounds' own checks)
and test_gpu_forward_rows.py (GPU: the kernels against those bounds). Not a test module.

A case is a frozen ``Case``; ``build(case)`` draws its inputs (CPU tensors in LOGICAL row order, the
order the oracle works in; the GPU file scatters them to caller order for q_rows / kv_rows) and
``reference(case)`` adds the fp64 reference, both rounding emulations and the bounds derived from
them. Both are cached, so the two files and every test of a case share one computation.

Every row of every case sees at most 600 keys (test_oracle_forward.py asserts it): below that a
dropped key moves every row's LSE by several times the LSE bound (pooled keys weigh 15 keys each;
test_oracle_forward.py says where that takes a case past the limit).
"""
import dataclasses
import functools
import math
import types

import numpy as np
import torch

import bsa_oracle as O

BF16, F16 = torch.bfloat16, torch.float16
DTYPES = ((64, BF16), (64, F16), (128, BF16), (128, F16))
TWO = ((64, BF16), (128, F16))                 # the groups that do not need the full D x dtype cross
LSE_CAP = 2e-5                                 # a hundredth of test_gpu_forward.py's 2e-3
LSE_FACTOR = 8.0
LOG15 = math.log(15.0)

KEY_TAILS = (1, 3, 63, 64, 65, 69, 96, 127, 129, 133, 192, 193, 255, 257)
QUERY_TAILS = (1, 31, 32, 33, 127, 128, 129, 161)
POOLED_TAILS = (1, 5, 31, 32, 33, 63, 64, 65, 100)

# spike targets: the spiked score in the exp2 domain (log2 units). The lazy bound is 2^32 (bf16) or
# 2^8 (f16) on P = exp2(score - m); the deferred rescale's slack is 4 log2 units.
HUGE = {BF16: 80.0, F16: 14.0}
MILD = 9.5


@dataclasses.dataclass(frozen=True)
class Case:
    group: str
    name: str
    D: int
    dtype: torch.dtype
    B: int
    H: int
    Lq: int
    Lk: int
    mask: str = "dense"       # dense | last | density | empty_row | b_expanded | h_expanded | oversized
    density: float = 0.5
    Lkp: int = 0              # pooled keys (0: no pooled branch)
    use_main: bool = True
    scale: float = None
    q_rows: bool = False
    kv_rows: bool = False
    peaked: bool = False      # q and k scaled by 2: a few keys dominate each row
    spikes: tuple = ()        # (("k" | "kp", query row, key index, target log2 score), ...)
    strided: bool = False     # q/k/v views of [B,L,H,D] storage
    out_view: bool = False    # out= a view of a larger NaN-filled buffer
    heavy_rows: int = 0
    seed: int = 0

    @property
    def id(self):
        return f"{self.group}-{self.name}-D{self.D}-{'bf16' if self.dtype == BF16 else 'f16'}"

    @property
    def spiked(self):
        return bool(self.spikes)

    @property
    def unit(self):
        """Scores of unit deviation: unit-normal q and k at the default scale, no spike (scale 0.2
        gives deviations of 1.6 at D=64 and 2.3 at D=128, much like the peaked variants)."""
        return not (self.peaked or self.spikes or self.scale is not None)


def _rand(*shape, dtype=BF16, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def _perm(L, seed):
    return torch.randperm(L, generator=torch.Generator().manual_seed(seed))


def _cases():
    out = []
    # 1. key tails: every 4-, 8-, 32- and 64-key boundary of the tail mask and the dropped-half rule
    for D, dt in DTYPES:
        for mask in ("dense", "last"):
            for gather in (False, True):
                for Lk in KEY_TAILS:
                    out.append(Case("keytail", f"Lk{Lk}-{mask}{'-gather' if gather else ''}", D, dt, 1, 2, 130, Lk,
                                    mask=mask, kv_rows=gather, seed=1000 + Lk))
        out.append(Case("keytail", "Lk193-peaked", D, dt, 1, 2, 130, 193, peaked=True, seed=1900))
    # 2. query tails, out= into a padded view
    for D, dt in DTYPES:
        for rows in (False, True):
            for Lq in QUERY_TAILS:
                out.append(Case("qtail", f"Lq{Lq}{'-rows' if rows else ''}", D, dt, 2, 3, Lq, 200, mask="density",
                                density=0.6, q_rows=rows, out_view=True, seed=2000 + Lq))
        out.append(Case("qtail", "Lq161-peaked", D, dt, 1, 2, 161, 200, mask="density", density=0.6, peaked=True,
                        out_view=True, seed=2900))
    # 3. pooled tails: (a) with a masked main branch that has a tail of its own, (b) with an empty
    #    mask row, (c) pooled keys alone
    for D, dt in DTYPES:
        for Lkp in POOLED_TAILS:
            out.append(Case("pooltail", f"Lkp{Lkp}-main", D, dt, 1, 2, 333, 333, mask="last", Lkp=Lkp, seed=3000 + Lkp))
            out.append(Case("pooltail", f"Lkp{Lkp}-emptyrow", D, dt, 1, 2, 333, 333, mask="empty_row", Lkp=Lkp,
                            seed=3200 + Lkp))
            out.append(Case("pooltail", f"Lkp{Lkp}-only", D, dt, 1, 2, 333, 0, Lkp=Lkp, use_main=False,
                            seed=3400 + Lkp))
        out.append(Case("pooltail", "Lkp33-main-peaked", D, dt, 1, 2, 333, 333, mask="last", Lkp=33, peaked=True,
                        seed=3900))
    # 4. the instantiation matrix (each case runs the inference and the training kernel)
    for D, dt in DTYPES:
        for pooled in (False, True):
            for gather in (False, True):
                out.append(Case("matrix", f"{'pool' if pooled else 'main'}{'-gather' if gather else ''}", D, dt, 2, 3,
                                300, 333, mask="density", density=0.4, Lkp=23 if pooled else 0, q_rows=True,
                                kv_rows=gather, heavy_rows=1, seed=4000))
        out.append(Case("matrix", "pool-gather-peaked", D, dt, 2, 3, 300, 333, mask="density", density=0.4, Lkp=23,
                        q_rows=True, kv_rows=True, heavy_rows=1, peaked=True, seed=4900))
    # 5. arguments the forward was never checked with
    for D, dt in TWO:
        out.append(Case("args", "scale0.2", D, dt, 1, 2, 130, 200, scale=0.2, seed=5000))
        out.append(Case("args", "mask-b-expanded", D, dt, 2, 2, 200, 300, mask="b_expanded", seed=5001))
        out.append(Case("args", "mask-h-expanded", D, dt, 2, 2, 200, 300, mask="h_expanded", seed=5002))
        out.append(Case("args", "mask-oversized", D, dt, 2, 2, 200, 300, mask="oversized", seed=5003))
        out.append(Case("args", "strided-tail", D, dt, 2, 3, 130, 197, strided=True, seed=5004))
        out.append(Case("args", "empty-row", D, dt, 1, 2, 300, 300, mask="empty_row", seed=5005))
        out.append(Case("args", "scale0.2-peaked", D, dt, 1, 2, 130, 200, scale=0.2, peaked=True, seed=5900))
    # 6. lazy and rescale paths. Lk = 333: key blocks of 128, 128 and 77 keys (tiles of 64 and 13).
    #    q-block 0 processes blocks 0, 1, 2; q-block 1 (rows 128, 129) its diagonal block 1 first.
    for D, dt in DTYPES:
        T = HUGE[dt]
        sp = dict(firsthalf=(("k", 5, 128 + 10, T),), secondhalf=(("k", 6, 192 + 40, T),),
                  tailtile=(("k", 7, 256 + 64 + 5, T),), pooled=(("kp", 8, 37, T),),
                  firsttile=(("k", 129, 128 + 3, T),), mild=(("k", 9, 256 + 20, MILD),))
        for name, spikes in sp.items():
            out.append(Case("spike", name, D, dt, 2, 2, 130, 333, Lkp=40 if name == "pooled" else 0, spikes=spikes,
                            seed=6000))
        out.append(Case("spike", "secondhalf-peaked", D, dt, 2, 2, 130, 333, spikes=sp["secondhalf"], peaked=True,
                        seed=6900))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids)
    return tuple(out)


CASES = _cases()

# Unit-score cases whose first draw puts the inference emulation's worst row above half of
# PER_ROW_CAP against the true reference (4.0e-3 .. 6.2e-3 bf16 with these few keys and rows; the
# bound, twice that, must hold the cap): they draw from seed + 100000 instead, where it does not.
# A condition on the inputs, found and asserted on the CPU emulation (test_oracle_forward.py);
# no kernel result enters it.
RESEED = dict.fromkeys((
    "keytail-Lk63-dense-D64-bf16", "keytail-Lk65-dense-D64-bf16", "keytail-Lk129-dense-D64-bf16",
    "keytail-Lk63-dense-gather-D64-bf16", "keytail-Lk65-dense-gather-D64-bf16",
    "keytail-Lk129-dense-gather-D64-bf16", "keytail-Lk63-last-D64-bf16", "keytail-Lk65-last-D64-bf16",
    "keytail-Lk129-last-D64-bf16", "keytail-Lk63-last-gather-D64-bf16", "keytail-Lk65-last-gather-D64-bf16",
    "keytail-Lk129-last-gather-D64-bf16", "keytail-Lk257-dense-D128-bf16", "keytail-Lk257-dense-gather-D128-bf16",
    "qtail-Lq161-D64-bf16", "qtail-Lq161-rows-D64-bf16", "qtail-Lq161-D128-bf16", "qtail-Lq161-rows-D128-bf16",
    "pooltail-Lkp5-main-D64-bf16", "pooltail-Lkp31-emptyrow-D64-bf16", "pooltail-Lkp31-only-D64-bf16",
    "pooltail-Lkp32-only-D64-bf16", "pooltail-Lkp63-main-D64-bf16", "pooltail-Lkp63-emptyrow-D64-bf16",
    "pooltail-Lkp63-only-D64-bf16", "pooltail-Lkp65-only-D64-bf16", "pooltail-Lkp100-main-D64-bf16",
    "pooltail-Lkp100-only-D64-bf16", "pooltail-Lkp32-emptyrow-D64-f16", "pooltail-Lkp5-main-D128-bf16",
    "pooltail-Lkp31-only-D128-bf16", "args-mask-b-expanded-D64-bf16", "args-mask-h-expanded-D64-bf16",
), 1)


def by_group(group):
    return [c for c in CASES if c.group == group]


def _mask(c, seed):
    if c.mask == "dense" or not c.use_main:
        return None
    nbq, nbk = (c.Lq + 127) // 128, (c.Lk + 127) // 128
    if c.mask == "last":
        m = O.block_mask_from_density(c.B, c.H, nbq, nbk, c.density, seed=seed + 4)
        m[..., -1] = True
    elif c.mask == "density":
        m = O.block_mask_from_density(c.B, c.H, nbq, nbk, c.density, seed=seed + 4)
    elif c.mask == "empty_row":
        m = O.block_mask_from_density(c.B, c.H, nbq, nbk, 0.6, seed=seed + 4)
        m[:, -1, 1, :] = False
    elif c.mask == "b_expanded":
        m = O.block_mask_from_density(1, c.H, nbq, nbk, c.density, seed=seed + 4).expand(c.B, -1, -1, -1)
    elif c.mask == "h_expanded":
        m = O.block_mask_from_density(c.B, 1, nbq, nbk, c.density, seed=seed + 4).expand(-1, c.H, -1, -1)
    elif c.mask == "oversized":
        m = torch.ones(c.B, c.H, nbq + 2, nbk + 2, dtype=torch.bool)
        m[:, :, :nbq, :nbk] = O.block_mask_from_density(c.B, c.H, nbq, nbk, c.density, seed=seed + 4)
    else:
        raise ValueError(c.mask)
    return m


def prescaled_query(q, scale):
    """The inference kernel's query: storage(fp32(q) * fp32(scale * log2 e))."""
    return (q.float() * float(np.float32(scale) * O.LOG2E_F32)).to(q.dtype)


@functools.lru_cache(maxsize=None)
def build(c):
    """Inputs of a case in logical row order: q [B,H,Lq,D], k/v [B,H,Lk,D] (None without a main
    branch), kp/vp (None without a pooled branch), mask (None = dense), the softmax scale, and the
    row tables (logical position -> caller row) the GPU file scatters by."""
    s = 2.0 if c.peaked else 1.0
    seed = c.seed + 100000 * RESEED.get(c.id, 0)
    d = types.SimpleNamespace(case=c, k=None, v=None, kp=None, vp=None, bias=0.0)
    d.scale = c.scale if c.scale is not None else 1.0 / math.sqrt(c.D)
    d.q = _rand(c.B, c.H, c.Lq, c.D, dtype=c.dtype, seed=seed, scale=s)
    if c.use_main:
        d.k = _rand(c.B, c.H, c.Lk, c.D, dtype=c.dtype, seed=seed + 1, scale=s)
        d.v = _rand(c.B, c.H, c.Lk, c.D, dtype=c.dtype, seed=seed + 2)
    if c.Lkp:
        d.kp = _rand(c.B, c.H, c.Lkp, c.D, dtype=c.dtype, seed=seed + 5, scale=s)
        d.vp = _rand(c.B, c.H, c.Lkp, c.D, dtype=c.dtype, seed=seed + 6)
        d.bias = LOG15
    for which, r, j, target in c.spikes:
        qr = d.q[:, :, r].float()
        mult = target * math.log(2.0) / (d.scale * qr.pow(2).sum(-1, keepdim=True))
        (d.k if which == "k" else d.kp)[:, :, j] = (qr * mult).to(c.dtype)
    d.mask = _mask(c, seed)
    d.Pq = _perm(c.Lq, seed + 10) if c.q_rows else None
    d.Pk = _perm(c.Lk, seed + 11) if c.kv_rows else None
    return d


def lse_bound(emu_lse, ref_lse):
    """LSE_FACTOR x the worst error of the fp32 emulation's LSE against fp64 on the same inputs (the
    factor covers what the CPU emulation lacks: the hardware exp2/log2 approximations, the * ln 2 and
    summation order), never more than LSE_CAP."""
    fin = torch.isfinite(ref_lse)
    assert torch.equal(fin, torch.isfinite(emu_lse))
    err = float((emu_lse.double() - ref_lse)[fin].abs().max())
    assert err > 0
    return min(LSE_FACTOR * err, LSE_CAP), err


# Half a unit in the last place of a storage value just above 1: the largest relative error one
# rounding of P can make.
HALF_ULP = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
OWNED = 0.9                                   # a row is owned by a key whose softmax weight exceeds this
SLACK = {"training": {BF16: 4.0, F16: 4.0},   # kRescaleSlack, log2 kLazyBoundBF16, log2 kLazyBoundF16
         "inference": {BF16: 32.0, F16: 8.0}}


def late_max_lag(dtype):
    """The m_lag (log2 units) at which a row's largest P is 1 + 0.98 half-ulps and so rounds to 1
    with nearly the largest error a rounding can make."""
    return math.log2(1.0 + 0.98 * HALF_ULP[dtype])


def rows_that_can_lag(q, k, v, mask, kp, vp, bias, scale, use_main, form, dtype):
    """bool [B,H,Lq]: the rows in which the kernel's running maximum can stand below the row's exact
    maximum when the owning key's P is rounded, and that rounding matters. All of:
      * one key owns the row (softmax weight > OWNED);
      * the row is fed more than one 64-key tile (the first tile sets the exact maximum:
        vb_attn_fwd.hip, `first`): more than 64 kept main keys, main and pooled keys, or more than
        64 pooled keys;
      * the owning score stands above the runner-up by no more than the form's slack (log2 units).
        m is some earlier score of the row, so a wider gap is also a wider step from m: the
        training form then raises m to the tile's exact maximum (kRescaleSlack), the inference
        form's half-tile sum exceeds kLazyBound and it does the same; P is exactly 1 either way."""
    K, V, vis, b = O.union_keys(q, k, v, mask, kp, vp, bias, use_main)
    Lkp = 0 if kp is None else kp.shape[2]
    n_main = vis[..., :vis.shape[-1] - Lkp].sum(-1)
    tiles = (n_main > 64) | ((n_main > 0) & (Lkp > 0)) | (Lkp > 64)
    return lagging_rows_over_visible(q, K, vis, b, scale, tiles, form, dtype)


def lagging_rows_over_visible(q, K, vis, b, scale, tiles, form, dtype):
    """rows_that_can_lag over any union of keys (K [B,H,n,D], ``vis`` bool [B,H,Lq,n], ``b`` the
    per-key bias in natural-log units); ``tiles`` bool [B,H,Lq]: the row is fed more than one tile."""
    s = (torch.matmul(q.double(), K.double().transpose(-1, -2)) * scale + b).masked_fill(~vis, float("-inf"))
    w = torch.softmax(s, -1)
    owned = torch.where(torch.isnan(w), torch.zeros_like(w), w).amax(-1) > OWNED
    if s.shape[-1] < 2:
        return torch.zeros_like(owned)
    top = s.topk(2, -1).values * math.log2(math.e)
    return owned & tiles & (top[..., 0] - top[..., 1] <= SLACK[form][dtype])


def row_bounds(emu, ref, dtype, can_lag, emulate_late):
    """Per-row bounds [B,H,Lq] of one launch, the scalar they start from, and the emulation's
    whole-tensor error.

    Every row: O.per_row_bound(emu, ref, dtype), 2 x the worst row of the emulation ``emu`` of the
    kernel that ran (asserted under PER_ROW_CAP there). An emulation that is exact (one visible key:
    P = 1, l = 1, out = v; in the kernels too) gives 0.

    The rows ``can_lag`` (rows_that_can_lag) get more. The emulation takes each row's exact maximum,
    so the owning key's P is exactly 1 and rounds without error. In the kernels that P is
    2^(score - m) with m lagging, and its rounding, up to 2^-8 bf16 / 2^-11 f16, goes into O whole
    while l sums the unrounded P: measured 4.8e-3 on such rows against an emulated 2.2e-3, which no
    factor of 2 covers. ``emulate_late(m_lag)`` is the same emulation with the maximum of exactly
    these rows lagging so that the P rounds worst. Their bound is its worst row among them (the
    owning P's rounding at its largest, with that row's other roundings) plus the plain emulation's
    worst row (another draw of the other roundings, as in the 2 x rule), never less than the other
    rows' bound, and asserted under PER_ROW_CAP like it."""
    worst = O.per_row_error(emu, ref)[0]
    base = 0.0 if worst == 0.0 else O.per_row_bound(emu, ref, dtype)
    bounds = torch.full(ref.shape[:3], base, dtype=torch.float64)
    if bool(can_lag.any()):
        lag = torch.where(can_lag, late_max_lag(dtype), 0.0)[..., None].float()
        late = float(O.per_row_errors(emulate_late(lag), ref)[can_lag].max())
        owned = worst + late
        assert owned <= O.PER_ROW_CAP[dtype], (owned, O.PER_ROW_CAP[dtype])
        bounds[can_lag] = max(base, owned)
    return bounds, base, frob(emu, ref)


@functools.lru_cache(maxsize=None)
def reference(c):
    """fp64 reference, the emulations and the bounds of a case. ``ref_i`` is what the inference
    launch is judged against: the reference itself, or, for a spiked, peaked or scale = 0.2 case
    (Case.unit False) whose inference emulation trips PER_ROW_CAP against it (scores that large make the rounding of q * c
    alone move a row by more than half the cap), the fp64 oracle on the pre-scaled query
    (sm_scale = ln 2), as test_huge_late_scores_rescale_both_kernels does. Every other case keeps
    the true reference (test_oracle_forward.py asserts it)."""
    d = build(c)
    kw = dict(kp=d.kp, vp=d.vp, use_main=c.use_main, kp_log_bias=d.bias, sm_scale=d.scale, store_dtype=c.dtype)
    jw = dict(kp=d.kp, vp=d.vp, use_main=c.use_main, bias=d.bias)
    r = types.SimpleNamespace(d=d)
    r.ref, r.ref_lse = O.joint_attention(d.q, d.k, d.v, d.mask, sm_scale=d.scale, **jw)
    r.emu_t, r.emu_t_lse = O.attention_fwd_emulated(d.q, d.k, d.v, d.mask, **kw)
    r.emu_i, _ = O.attention_fwd_emulated(d.q, d.k, d.v, d.mask, prescale_q=True, **kw)
    r.emu_i_err = O.per_row_error(r.emu_i, r.ref)[0]
    r.prescaled = not c.unit and 2.0 * r.emu_i_err > O.PER_ROW_CAP[c.dtype]
    if r.prescaled:
        r.ref_i, _ = O.joint_attention(prescaled_query(d.q, d.scale), d.k, d.v, d.mask, sm_scale=math.log(2.0), **jw)
    else:
        r.ref_i = r.ref
    r.emu_t_err, r.emu_i_ref_err = O.per_row_error(r.emu_t, r.ref)[0], O.per_row_error(r.emu_i, r.ref_i)[0]
    own = (d.q, d.k, d.v, d.mask, d.kp, d.vp, d.bias, d.scale, c.use_main)
    r.can_t = rows_that_can_lag(*own, "training", c.dtype)
    r.can_i = rows_that_can_lag(*own, "inference", c.dtype)
    r.bounds_t, r.bound_t, r.whole_t = row_bounds(
        r.emu_t, r.ref, c.dtype, r.can_t, lambda lag: O.attention_fwd_emulated(d.q, d.k, d.v, d.mask, m_lag=lag, **kw)[0])
    r.bounds_i, r.bound_i, r.whole_i = row_bounds(
        r.emu_i, r.ref_i, c.dtype, r.can_i,
        lambda lag: O.attention_fwd_emulated(d.q, d.k, d.v, d.mask, prescale_q=True, m_lag=lag, **kw)[0])
    r.lse_bound, r.lse_emu_err = lse_bound(r.emu_t_lse, r.ref_lse)
    return r


def frob(x, ref):
    ref = ref.double()
    return float((x.double() - ref).norm() / ref.norm().clamp_min(1e-300))
