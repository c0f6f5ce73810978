"""CPU checks of the forward row-parity bounds themselves (tests/fwd_cases.py; no kernel involved).

1. The emulation is tight: on every case of the table, mask and spike placement included, the
   per-row bound 2 x (emulation against fp64) stays under PER_ROW_CAP for the training and for the
   inference emulation, against the true reference for every unit-score case. A peaked, spiked or
   scale = 0.2 case whose inference emulation trips the cap is judged on the pre-scaled query.
   Worst rows of the emulation here (against what it is judged by):
     bf16  training 1.5e-3 .. 3.4e-3   inference 1.6e-3 .. 4.9e-3 (true reference), 1.9e-3 .. 2.8e-3 (pre-scaled)
     f16   training 1.9e-4 .. 4.4e-4   inference 2.4e-4 .. 7.4e-4 (true reference), 2.5e-4 .. 3.2e-4 (pre-scaled)
   Rows in which the kernel's maximum can lag under an owning key (fwd_cases.row_bounds) have a
   bound of their own, 5.8e-3 .. 8.6e-3 bf16 and 7.9e-4 .. 9.5e-4 f16, under the cap; no unit-score
   case has such a row.
   The LSE of the fp32 emulation is within 1.9e-7 .. 1.4e-6 of fp64 on the unit-score cases (up to
   1.5e-5 on the others), so the LSE bound (8 x, capped at 2e-5) is 1.6e-6 .. 2e-5.

2. The bounds can see the faults they are for: each mutation of the fp64 reference (a dropped or
   doubled last key, a dropped last pooled key, a lost pooled bias, the default scale in place of the
   custom one, a tail row with its neighbour's result, a kept block dropped at a list's end) moves
   the worst row by at least 4 x the case's per-row bound and the LSE of EVERY affected row by at
   least 2 x the LSE bound. The LSE condition is asserted on the unit-normal cases: with peaked or
   spiked inputs (or scale = 0.2: score deviations of 1.6 and 2.3) one key can own a row, and a key
   whose weight is e^-30 moves no LSE; those cases assert the output condition, and the LSE
   condition for the mutations that move every row's LSE by construction. A single full-resolution
   key (dropped or doubled) is claimed only while the softmax mass, main keys + 15 x pooled keys,
   is at most 600 keys: the pooled tails put up to 1500 on top of their 333 keys, where one main
   key is too light for either condition. Smallest margins here: worst row 5.7 x the bound (the
   last key of 200 behind a 0.6-density mask, counted twice), LSE shift 5.2 x its bound.
"""
import math

import pytest
import torch

import bsa_oracle as O
import fwd_cases as F
from conftest import record


def test_the_table_covers_what_it_claims():
    """Every tail length of the three groups, all 32 instantiations (16 cases x two launches), and no
    row with more than 600 visible keys."""
    for group, field, want in (("keytail", "Lk", F.KEY_TAILS), ("qtail", "Lq", F.QUERY_TAILS),
                               ("pooltail", "Lkp", F.POOLED_TAILS)):
        for D, dt in F.DTYPES:
            got = {getattr(c, field) for c in F.by_group(group) if (c.D, c.dtype) == (D, dt)}
            assert got == set(want), (group, D, dt)
    forms = {(c.D, c.dtype, c.Lkp > 0, c.kv_rows) for c in F.by_group("matrix") if not c.peaked}
    assert len(forms) == 16
    for c in F.CASES:
        assert c.B <= 2 and c.H <= 3 and max(c.Lq, c.Lk) <= 520
        assert c.Lk * c.use_main + c.Lkp <= 600, c.id


def test_emulation_is_exact_where_the_arithmetic_is():
    """One visible key: P = 1, l = 1, out = v in both forms, LSE = the score. And the emulation of
    an all-ones mask equals the dense one bit for bit."""
    c = next(c for c in F.CASES if c.Lk == 1 and c.mask == "dense")
    r = F.reference(c)
    assert r.bound_t == 0.0 and r.bound_i == 0.0
    assert torch.equal(r.emu_t, r.d.v.float().expand_as(r.emu_t))
    d = F.build(next(c for c in F.CASES if c.group == "args" and c.name == "scale0.2"))
    ones = torch.ones(d.q.shape[0], d.q.shape[1], 2, 2, dtype=torch.bool)
    a = O.attention_fwd_emulated(d.q, d.k, d.v, None, sm_scale=0.2, store_dtype=d.q.dtype)
    b = O.attention_fwd_emulated(d.q, d.k, d.v, ones, sm_scale=0.2, store_dtype=d.q.dtype)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_joint_attention_equals_the_two_branch_combine():
    """joint_attention against test_fused_pooled_branch_equals_joint_softmax's hand-built reference
    (two block_sparse_attention calls combined through their LSEs)."""
    d = F.build(next(c for c in F.CASES if c.group == "pooltail" and c.name == "Lkp33-main"))
    out, lse = O.joint_attention(d.q, d.k, d.v, d.mask, d.kp, d.vp, d.bias)
    o1, l1 = O.block_sparse_attention(d.q, d.k, d.v, d.mask)
    o2, l2 = O.block_sparse_attention(d.q, d.kp, d.vp, None, key_bias=d.bias)
    lj = torch.logaddexp(l1, l2)
    a = torch.exp(l1 - lj)[..., None]
    assert (out - (o1 * a + o2 * (1 - a))).abs().max() <= 2e-6
    assert (lse - lj).abs().max() <= 4e-6
    # an empty mask row sees the pooled keys alone
    e = F.build(next(c for c in F.CASES if c.group == "pooltail" and c.name == "Lkp33-emptyrow"))
    out, lse = O.joint_attention(e.q, e.k, e.v, e.mask, e.kp, e.vp, e.bias)
    po, pl = O.joint_attention(e.q, None, None, None, e.kp, e.vp, e.bias, use_main=False)
    assert (out[:, -1, 128:256] - po[:, -1, 128:256]).abs().max() <= 1e-12
    assert (lse[:, -1, 128:256] - pl[:, -1, 128:256]).abs().max() <= 1e-12
    assert (out[:, 0, 128:256] - po[:, 0, 128:256]).abs().max() > 1e-3     # the other head's rows do not


def test_emulations_stay_under_the_cap():
    """reference() asserts PER_ROW_CAP for every bound it derives (O.per_row_bound, and the lagging
    rows' bound in F.row_bounds); here the ranges are recorded, the LSE emulation is checked, and:
      * every unit-score case is judged against the true reference in both launches, with the
        issue's bound, 2 x the emulation's worst row, on every row (no lagging rows);
      * the lagging-maximum term reaches only rows of peaked, spiked or scale = 0.2 cases, and
        widens those rows' bound by less than 2 x, under the cap;
      * only such cases are judged on the pre-scaled query."""
    rng = {}
    n_pre = 0
    for c in F.CASES:
        r = F.reference(c)
        cap = O.PER_ROW_CAP[c.dtype]
        assert r.lse_emu_err <= 1.5e-5, (c.id, r.lse_emu_err)   # a few fp32 ulps of an LSE of 3 .. 60
        for base, bounds, can, emu_err in ((r.bound_t, r.bounds_t, r.can_t, r.emu_t_err),
                                           (r.bound_i, r.bounds_i, r.can_i, r.emu_i_ref_err)):
            assert base == 2.0 * emu_err and 0.0 <= base <= cap, c.id
            assert bool((bounds[~can] == base).all()) and float(bounds.max()) <= min(cap, 2.0 * base), c.id
            if c.unit:
                assert not bool(can.any()), c.id
        if c.unit:
            assert not r.prescaled and r.ref_i is r.ref, c.id
        n_pre += r.prescaled
        kind = "unit" if c.unit else "peaked/spiked/scaled"
        for key, val in ((("t", c.dtype), r.emu_t_err), (("i-pre" if r.prescaled else "i", c.dtype), r.emu_i_ref_err),
                         (("t lagging rows' bound", c.dtype), float(r.bounds_t.max()) if r.can_t.any() else 0.0),
                         (("i lagging rows' bound", c.dtype), float(r.bounds_i.max()) if r.can_i.any() else 0.0),
                         (("lse-" + kind, None), r.lse_emu_err)):
            if val > 0:
                lo, hi = rng.get(key, (val, val))
                rng[key] = (min(lo, val), max(hi, val))
    record("forward emulation worst rows (t training, i inference, i-pre inference on the pre-scaled query)",
           {f"{k[0]} {k[1]}": f"{lo:.2e}..{hi:.2e}" for k, (lo, hi) in rng.items()})
    record("forward cases judged on the pre-scaled query", n_pre)
    assert set(F.RESEED) <= {c.id for c in F.CASES if c.unit}


def test_spikes_cross_the_thresholds_they_are_for():
    """A spiked row's score stands above the maximum of the first tile its q-block processes by more
    than the lazy bound (2^32 bf16, 2^8 f16) for the huge spikes, and between the rescale slack
    (4 log2 units) and the f16 lazy bound (8) for the mild one. The first-tile spike IS that tile's
    maximum."""
    for c in F.by_group("spike"):
        if c.peaked:
            continue
        d = F.build(c)
        for which, row, j, target in c.spikes:
            K = d.k if which == "k" else d.kp
            s = (d.q[0, 0, row].double() @ K[0, 0].double().T) * d.scale * math.log2(math.e)
            assert abs(float(s[j]) - target) <= 0.01 * target    # the storage rounding of the spiked key
            if which == "kp":
                s = s + d.bias * math.log2(math.e)
            if c.name == "firsttile":
                first = slice(128, 192)               # q-block 1: its diagonal block comes first
                sm = (d.q[0, 0, row].double() @ d.k[0, 0, first].double().T) * d.scale * math.log2(math.e)
                assert int(sm.argmax()) == j - 128
                continue
            m0 = float(((d.q[0, 0, row].double() @ d.k[0, 0, :64].double().T) * d.scale * math.log2(math.e)).max())
            over = float(s[j]) - m0
            if c.name == "mild":
                assert 4.0 < over < 8.0, (c.id, over)
            else:
                assert over > (32.0 if c.dtype == F.BF16 else 8.0), (c.id, over)


# ----------------------------------------------------------------------------------------------
# 2. mutations
# ----------------------------------------------------------------------------------------------
def mutations(c):
    """(name, out, lse, affected rows [B,H,Lq] bool, when) for every mutation that applies to the
    case. ``when``: the inputs on which the mutation moves the LSE of EVERY affected row by 2 x the
    LSE bound: "always" (it rewrites the row or every score), "unit" (unit-variance scores: no key's
    weight vanishes in any row), "light" (a single full-resolution key: unit-variance scores and a
    softmax mass, main keys + e^bias x pooled keys, of at most MASS_LIMIT keys; the pooled tails
    carry 15 x Lkp on top of their 333 keys, and past the limit one main key is too light for the
    output condition as well, so neither is asserted there)."""
    d, r = F.build(c), F.reference(c)
    K, V, vis, b = O.union_keys(d.q, d.k, d.v, d.mask, d.kp, d.vp, d.bias, c.use_main)
    every = torch.ones(c.B, c.H, c.Lq, dtype=torch.bool)

    def run(vis=vis, b=b, scale=d.scale):
        return O.softmax_over_visible(d.q, K, V, vis, b, scale)

    if c.use_main and c.Lk >= 2:
        last = c.Lk - 1
        v2 = vis.clone()
        v2[..., last] = False
        yield ("last key dropped",) + run(vis=v2) + (vis[..., last], "light")
        b2 = b.clone()
        b2[last] += math.log(2.0)
        yield ("last key twice",) + run(b=b2) + (vis[..., last], "light")
    if c.Lkp:
        v2 = vis.clone()
        v2[..., -1] = False
        yield ("last pooled key dropped",) + run(vis=v2) + (every, "unit")
        if c.use_main:
            yield ("pooled bias 0",) + run(b=torch.zeros_like(b)) + (every, "unit")
    if c.scale is not None:
        yield ("default scale",) + run(scale=c.D ** -0.5) + (every, "always")
    if c.Lq >= 2:
        out, lse = r.ref.clone(), r.ref_lse.clone()
        out[:, :, -1], lse[:, :, -1] = r.ref[:, :, -2], r.ref_lse[:, :, -2]
        only = torch.zeros_like(every)
        only[:, :, -1] = True
        yield ("tail row takes its neighbour's", out, lse, only, "always")
    if c.use_main and d.mask is not None:
        nbk = (c.Lk + 127) // 128
        m = d.mask.clone()[:, :, :, :nbk]
        for bi in range(c.B):
            for h in range(c.H):
                kept = torch.nonzero(m[bi, h, 0])
                if kept.numel():
                    m[bi, h, 0, int(kept[-1])] = False
        Km, Vm, vm, bm = O.union_keys(d.q, d.k, d.v, m, d.kp, d.vp, d.bias, True)
        rows = torch.zeros_like(every)
        rows[:, :, :128] = True
        yield ("kept block at a list's end dropped",) + O.softmax_over_visible(d.q, Km, Vm, vm, bm, d.scale) + (rows, "unit")


MASS_LIMIT = 600


@pytest.mark.parametrize("group", ["keytail", "qtail", "pooltail", "matrix", "args", "spike"])
def test_bounds_see_the_faults_they_are_for(group):
    n = 0
    low = {}
    for c in F.by_group(group):
        r = F.reference(c)
        unit = c.unit
        mass = c.Lk * c.use_main + math.exp(r.d.bias) * c.Lkp
        bound = max(float(r.bounds_t.max()), float(r.bounds_i.max()))
        for name, out, lse, rows, when in mutations(c):
            worst = O.per_row_error(out, r.ref)[0]
            if when != "light" or mass <= MASS_LIMIT:
                assert worst >= 4.0 * bound, (c.id, name, worst, bound)
            shift = (lse - r.ref_lse).abs()
            shift = torch.where(torch.isnan(shift), torch.zeros_like(shift), shift)[rows]   # -inf - -inf: no change
            assert shift.numel() > 0, (c.id, name)
            claimed = when == "always" or (unit and (when == "unit" or mass <= MASS_LIMIT))
            if claimed:
                assert float(shift.min()) >= 2.0 * r.lse_bound, (c.id, name, float(shift.min()), r.lse_bound)
                lo = low.get(name, (math.inf, math.inf))
                low[name] = (min(lo[0], worst / bound if bound > 0 else math.inf),
                             min(lo[1], float(shift.min()) / r.lse_bound))
            n += 1
    assert n > 0
    record(f"forward mutations, {group}: smallest (worst row / bound, LSE shift / LSE bound)",
           {k: f"{a:.1f}x, {b:.1f}x" for k, (a, b) in low.items()})
