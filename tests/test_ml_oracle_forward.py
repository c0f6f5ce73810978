"""CPU checks of the multi-level forward's row-parity reference and bounds (tests/ml_fwd_cases.py;
no kernel involved). The twin of test_oracle_forward.py.

1. The reference: ml_oracle.multilevel_attention_fp64 (one softmax over the union of the pyramid's
   keys) agrees with the per-block restatement ml_oracle.multilevel_attention on fp32 inputs within
   1e-5 (measured 2e-7 .. 1.2e-6), under both tail rules, and with the reference kernel's own out, m
   and l in tests/golden/multilevel.npz at test_ml_oracle_golden.py's bounds.

2. The cap: every case's bound, 2 x (emulation against fp64), stays under PER_ROW_CAP for both
   emulations, against the true reference for every unit-score case, and the reseed rule holds
   (ml_fwd_cases.RESEED: every earlier draw of a listed case is over half the cap, every unit-score
   case's final draw is not). Worst rows of the emulation here:
     bf16  training 2.3e-3 .. 4.4e-3   inference 3.0e-3 .. 5.0e-3 (true reference), 2.3e-3 .. 3.4e-3 (pre-scaled)
     f16   training 3.0e-4 .. 5.6e-4   inference 3.8e-4 .. 7.5e-4 (true reference), 3.2e-4 (pre-scaled)
   (the one-row cases, whose arithmetic is exact or nearly so, left out of the lower ends).
   The fp32 emulation's LSE is within 3.0e-7 .. 1.7e-6 of fp64 on the unit-score cases, up to 1.1e-5
   on the spiked and scaled ones.

3. Mutations of the fp64 reference, each on the cases built for it, move the worst row by at least
   4 x the case's per-row bound and, on unit-score cases, the LSE of every affected row by at least
   2 x the LSE bound (test_oracle_forward.py's criterion): the last block of a partial level-4 or
   level-8 tile dropped, the last pyramid row of a partial tile lost (on the whole q-block and on 32
   of its rows), level-8 bias ln 4, level-2 bias lost, ref_tail ignored in both directions, the last
   real key dropped, a tail row with its neighbour's result, a kept block past column 64 dropped.
   "ref_tail ignored" is claimed where at least a quarter of the tail block is padding: a single
   zero key among 128 or more weighs under 1 % of a row, below 4 x a bf16 bound of 9e-3.
"""
import math
import os

import numpy as np
import pytest
import torch

import bsa_oracle as O
import ml_fwd_cases as M
import ml_oracle as ML
from conftest import GOLDEN, record

BLOCK = ML.BLOCK


# ----------------------------------------------------------------------------------------------
# 1. the reference
# ----------------------------------------------------------------------------------------------
def _stats(q, k, v, mask, ref_tail=True):
    """out, m (row max of the biased logits, natural log) and l = exp(lse - m) of the fp64 reference."""
    out, lse = ML.multilevel_attention_fp64(q, k, v, mask, ref_tail=ref_tail)
    K, _, vis, bias, _, _ = ML.ml_union_keys(q, k, v, mask, ref_tail)
    s = torch.matmul(q.double(), K.double().transpose(-1, -2)) * q.shape[-1] ** -0.5 + bias
    m = s.masked_fill(~vis, float("-inf")).amax(-1)
    return out, m, torch.exp(lse - m), lse


@pytest.mark.parametrize("ref_tail", [True, False])
@pytest.mark.parametrize("L,D", [(300, 64), (1000, 128), (129, 64), (256, 128), (40, 64)])
def test_fp64_reference_equals_the_per_block_restatement(L, D, ref_tail):
    B, H = 2, 2
    g = torch.Generator().manual_seed(L + D)
    q, k, v = (torch.randn(B, H, L, D, generator=g) for _ in range(3))
    nb = (L + BLOCK - 1) // BLOCK
    mask = M._random_levels(B, H, nb, L + 7 * D, M.MIX)
    mask[0, 0, 0, :] = torch.tensor([3, 5, 16, 255, 0, 0, 0, 0][:nb], dtype=torch.int32)   # keeps nothing
    for i in range(nb):
        mask[1, 1, i, -1] = ML.LEVELS[i % 4]
    r = ML.multilevel_attention(q, k, v, mask, ref_tail=ref_tail)
    out, lse = ML.multilevel_attention_fp64(q, k, v, mask, ref_tail=ref_tail)
    empty = torch.isneginf(lse)
    assert bool(empty[0, 0, :min(L, BLOCK)].all()) and bool((out[empty] == 0).all())
    assert not bool(empty[1].any())
    err = float((out - r["out"]).abs().max())
    err_lse = float((lse - r["lse"])[~empty].abs().max())
    record("multi-level fp64 reference against multilevel_attention (out, lse)", f"L={L} D={D} {err:.1e} {err_lse:.1e}")
    assert err <= 1e-5 and err_lse <= 1e-5


@pytest.mark.parametrize("case", ["f32_d64", "f16_d64", "f32_d128", "f16_d128_b2"])
def test_fp64_reference_matches_reference_kernel(case):
    z = np.load(os.path.join(GOLDEN, "multilevel.npz"))
    g = lambda s: torch.from_numpy(z[f"k_{case}_{s}"])   # noqa: E731
    dt = {"torch.float32": torch.float32, "torch.float16": torch.float16}[str(z[f"k_{case}_dtype"])]
    q, k, v = (g(s).to(dt) for s in ("q", "k", "v"))
    out, m, l, _ = _stats(q, k, v, g("mask"))
    assert (out - g("out")).abs().max() < (1e-5 if dt == torch.float32 else 2e-3)
    assert ((l - g("l")) / g("l")).abs().max() < 1e-5
    assert (m - g("m")).abs().max() < 1e-5


def test_union_keys_layout():
    """The pyramid rows, their levels, blocks and biases; the zeroed level-1 tail and its visibility
    under the two tail rules; q_pos selects rows."""
    L, D = 300, 64
    q, k, v = (M.F._rand(1, 1, L, D, seed=s) for s in range(3))
    mask = torch.tensor([[1, 2, 8], [0, 4, 1], [8, 8, 2]], dtype=torch.int32)[None, None]
    K, V, vis, bias, lvl, blk = ML.ml_union_keys(q, k, v, mask, True)
    assert K.shape == (1, 1, 15 * 384 // 8, D) and K.dtype == q.dtype
    assert bool((K[:, :, L:384] == 0).all()) and bool((V[:, :, L:384] == 0).all())
    pyr = ML.kv_pyramid(k)
    assert torch.equal(K[:, :, 384:384 + 192], pyr[1]) and torch.equal(K[:, :, 384 + 192 + 96:], pyr[3])
    assert torch.equal(bias, lvl.double().log()) and lvl.tolist() == [1] * 384 + [2] * 192 + [4] * 96 + [8] * 48
    assert blk[384:384 + 192].tolist() == [j for j in range(3) for _ in range(64)]
    # q-block 1 keeps block 1 at level 4 and block 2 at level 1 (pads included under ref_tail)
    want = torch.zeros(720, dtype=torch.bool)
    want[256:384] = True
    want[384 + 192 + 32:384 + 192 + 64] = True
    assert torch.equal(vis[0, 0, 130], want)
    _, _, vis2, _, _, _ = ML.ml_union_keys(q, k, v, mask, False)
    want[L:384] = False
    assert torch.equal(vis2[0, 0, 130], want)
    sel = torch.tensor([5, 130, 299])
    _, _, vis3, _, _, _ = ML.ml_union_keys(q[:, :, sel], k, v, mask, False, q_pos=sel)
    assert torch.equal(vis3, vis2[:, :, sel])
    a = ML.multilevel_attention_fp64(q[:, :, sel], k, v, mask, q_pos=sel)
    b = ML.multilevel_attention_fp64(q, k, v, mask)
    assert torch.equal(a[0], b[0][:, :, sel]) and torch.equal(a[1], b[1][:, :, sel])
    # tiles fed: q-block 0: 2 + 1 + 1; q-block 1: 1 + 2 (- 1 without ref_tail: 256 + 64 >= 300); q-block 2: 1 + 1
    assert ML.ml_tiles_fed(mask, L, True)[0, 0].tolist() == [4, 3, 2]
    assert ML.ml_tiles_fed(mask, L, False)[0, 0].tolist() == [4, 2, 2]
    assert ML.ml_tiles_fed(mask, 330, False)[0, 0].tolist() == [4, 3, 2]


def test_emulation_is_exact_where_the_arithmetic_is():
    """One visible key (L = 1, level 1, pads hidden) and sixteen equal keys (L = 1 at level 8: the
    replicate-padded pyramid row): out = v in both forms."""
    c = next(c for c in M.CASES if c.group == "c" and c.L == 1 and not c.ref_tail)
    r = M.reference(c)
    assert r.bound_t == 0.0 and r.bound_i == 0.0
    assert torch.equal(r.emu_t, r.d.v.float()) and torch.equal(r.emu_i, r.d.v.float())


# ----------------------------------------------------------------------------------------------
# 2. the table and the cap
# ----------------------------------------------------------------------------------------------
def _counts(row):
    return tuple(sum(1 for x in row if x == p) for p in ML.LEVELS)


def test_the_table_covers_what_it_claims():
    for c in M.CASES:
        assert c.B <= 2 and c.H <= 3 and (c.L <= 1280 or c.q_blocks), c.id
    # a: the eight instantiations, each plain and persistent, 9 blocks and a 76-row tail
    a = M.by_group("a")
    assert {(c.D, c.dtype) for c in a} == set(M.DTYPES) and all(c.persistent and c.L == 1100 and c.q_rows for c in a)
    assert {c.ref_tail for c in a} == {True, False}
    # b: every count alone and beside other levels; the singles; first, last and scattered placements
    alone4, alone8, beside4, beside8, singles = set(), set(), set(), set(), set()
    for name, table in M.PACK.items():
        assert len(table) == 10 and all(len(r) == 10 for r in table)
        for row in table:
            n1, n2, n4, n8 = _counts(row)
            kinds = sum(1 for n in (n1, n2, n4, n8) if n)
            if kinds == 1:
                alone4.update({n4} - {0}), alone8.update({n8} - {0})
                if n1 + n2 + n4 + n8 == 1:
                    singles.add(max(row))
            else:
                beside4.update({n4} - {0}), beside8.update({n8} - {0})
    assert alone4 == {1, 2, 3, 4, 5} and alone8 == {1, 2, 3, 4, 5, 6, 7, 9, 10}
    assert beside4 == {1, 2, 3, 4, 5} and beside8 == {1, 2, 3, 4, 5, 6, 7, 9}     # 10 of 10 blocks leave no room
    assert singles >= {1, 2, 8}
    for p in (4, 8):
        rows = [r for t in M.PACK.values() for r in t if p in r]
        assert any(r[0] == p for r in rows) and any(r[-1] == p for r in rows)
        assert any(r[0] != p and r[-1] != p for r in rows)
    assert {(c.D, c.dtype, c.mask) for c in M.by_group("b")} == {(D, dt, n) for D, dt in M.TWO for n in M.PACK}
    # c: every tail under both rules with every level in the last column; level 1 there on both
    # sides of (nb - 1) * 128 + 64 >= L; the one-block lengths at each level
    for D, dt in M.TWO:
        for ref_tail in (True, False):
            cs = [c for c in M.by_group("c") if (c.D, c.dtype, c.ref_tail) == (D, dt, ref_tail)]
            assert {c.L for c in cs} == {256 + r for r in M.TAILS} | set(M.ONE_BLOCK)
            for c in cs:
                m = M.build(c).mask
                assert set(m[..., -1].flatten().tolist()) == set(ML.LEVELS), c.id
    assert any(r <= 64 for r in M.TAILS) and any(r > 64 for r in M.TAILS)
    # d, e
    assert {c.io for c in M.by_group("d")} == {"out_view", "q_strided", "blhd", "mask_h_expanded", "mask_strided"}
    assert all(c.B == 2 for c in M.by_group("d")) and all(c.L % 32 for c in M.by_group("d") if c.io == "out_view")
    assert {c.scale for c in M.by_group("e")} == {0.2, 0.05, None}
    for c in M.by_group("e"):
        if c.mask == "nonlevel":
            r = M.reference(c)
            m = r.d.mask
            assert {3, 5, 16, 255} <= set(m.flatten().tolist())
            assert bool(torch.isneginf(r.ref_lse[:, 0, 4 * BLOCK:]).all()) and bool((r.ref[:, 0, 4 * BLOCK:] == 0).all())
            assert bool(torch.isfinite(r.ref_lse[:, 0, :4 * BLOCK]).all()) and bool(torch.isfinite(r.ref_lse[:, 1]).all())
    # g: 67 blocks; in every referenced q-block each level has entries below column 64, and over
    # them at least two at or past it
    for c in M.by_group("g"):
        m = M.build(c).mask
        assert c.nb == 67 and c.q_blocks == M.LONG_QBLOCKS
        past = {p: 0 for p in ML.LEVELS}
        for qb in c.q_blocks:
            row = m[0, 0, qb]
            for p in ML.LEVELS:
                assert bool((row[:64] == p).any()), (c.id, qb, p)
                past[p] += int((row[64:] == p).sum())
            assert bool((row[60:67] > 0).all())
        assert min(past.values()) >= 2
    assert {(c.D, c.dtype) for c in M.by_group("g")} == set(M.TWO)


def test_late_maxima_arrive_where_they_are_meant_to():
    """f: the spiked key's pooled row equals the spike, sits in the tile kind the case names, after
    ordinary tiles, and stands above the first tile's maximum by more than the lazy bound (huge) or
    by more than the rescale slack and, its level's bias apart, less than the f16 lazy bound (mild)."""
    assert M.LATE_ROW == (1, 1, 2, 4, 4, 8, 8, 8, 8, 0)
    for c in M.by_group("f"):
        d = M.build(c)
        (row, p, j0, target), = c.spikes
        blk = j0 // BLOCK
        assert M.LATE_ROW[blk] == p and row < BLOCK
        kept = [j for j, x in enumerate(M.LATE_ROW) if x == p]
        place = c.name.rsplit("-", 1)[0]
        assert kept.index(blk) == {"l1-later-tile": 1, "l2-tile": 0, "l4-second-block": 1, "l8-third-block": 2}[place], c.id
        assert p > 1 or j0 % BLOCK >= 64          # the level-1 block's second tile
        lv = ML.LEVELS.index(p)
        pooled = ML.kv_pyramid(d.k)[lv][:, :, j0 // p]
        assert torch.equal(pooled, d.k[:, :, j0]) and torch.equal(d.k[:, :, j0 + p - 1], d.k[:, :, j0])
        log2e = math.log2(math.e)
        s = float((d.q[0, 0, row].double() @ pooled[0, 0].double()) * d.scale * log2e)
        assert abs(s - target) <= 0.01 * target
        m0 = float(((d.q[0, 0, row].double() @ d.k[0, 0, :64].double().T) * d.scale * log2e).max())
        over = s + math.log2(p) - m0
        if c.name.endswith("mild"):
            assert target == M.MILD and 4.0 < over < 8.0 + math.log2(p), (c.id, over)
        else:
            assert over > (32.0 if c.dtype == M.BF16 else 8.0), (c.id, over)


def test_emulations_stay_under_the_cap():
    """reference() asserts PER_ROW_CAP for every bound it derives; here, as test_oracle_forward.py:
    every unit-score case is judged against the true reference in both launches with 2 x the
    emulation's worst row on every row (no lagging rows); lagging rows and the pre-scaled reference
    occur in spiked or scaled cases only; the reseed rule holds."""
    rng = {}
    n_pre = 0
    for c in M.CASES:
        r = M.reference(c)
        cap = O.PER_ROW_CAP[c.dtype]
        assert r.lse_emu_err <= 1.5e-5, (c.id, r.lse_emu_err)
        for base, bounds, can, emu_err in ((r.bound_t, r.bounds_t, r.can_t, r.emu_t_err),
                                           (r.bound_i, r.bounds_i, r.can_i, r.emu_i_ref_err)):
            assert base == 2.0 * emu_err and 0.0 <= base <= cap, c.id
            assert bool((bounds[~can] == base).all()) and float(bounds.max()) <= min(cap, 2.0 * base), c.id
            if c.unit:
                assert not bool(can.any()), c.id
        if c.unit:
            assert not r.prescaled and r.ref_i is r.ref, c.id
            assert r.emu_i_err <= cap / 2, (c.id, r.emu_i_err)
        assert (c.id in M.RESEED) <= c.unit
        for draw in range(M.RESEED.get(c.id, 0)):
            assert M.reference(c, draw).emu_i_err > cap / 2, (c.id, draw)
        n_pre += r.prescaled
        for key, val in ((("t", c.dtype), r.emu_t_err), (("i-pre" if r.prescaled else "i", c.dtype), r.emu_i_ref_err),
                         (("t lagging rows' bound", c.dtype), float(r.bounds_t.max()) if r.can_t.any() else 0.0),
                         (("i lagging rows' bound", c.dtype), float(r.bounds_i.max()) if r.can_i.any() else 0.0),
                         (("lse-" + ("unit" if c.unit else "spiked/scaled"), None), r.lse_emu_err)):
            if val > 1e-4 or (key[0].startswith("lse") and val > 0):   # the one-row cases are (nearly) exact
                lo, hi = rng.get(key, (val, val))
                rng[key] = (min(lo, val), max(hi, val))
    record("multi-level forward emulation worst rows (t training, i inference, i-pre on the pre-scaled query)",
           {f"{k[0]} {k[1]}": f"{lo:.2e}..{hi:.2e}" for k, (lo, hi) in rng.items()})
    record("multi-level forward cases judged on the pre-scaled query", n_pre)
    assert set(M.RESEED) <= {c.id for c in M.CASES}


# ----------------------------------------------------------------------------------------------
# 3. mutations
# ----------------------------------------------------------------------------------------------
def _level_offsets(Lpad):
    return {1: 0, 2: Lpad, 4: Lpad + Lpad // 2, 8: Lpad + Lpad // 2 + Lpad // 4}


def mutations(c):
    """(name, out, lse, affected rows bool [B,H,rows]) for every mutation that applies to the case,
    over the case's referenced rows."""
    d, r = M.build(c), M.reference(c)
    qs = d.q if d.sel is None else d.q[:, :, d.sel]
    pos = torch.arange(c.L) if d.sel is None else d.sel
    K, V, vis, bias, lvl, blk = ML.ml_union_keys(qs, d.k, d.v, d.mask, c.ref_tail, d.sel)
    off = _level_offsets(c.nb * BLOCK)
    qblk = pos // BLOCK
    none = torch.zeros(c.B, c.H, pos.numel(), dtype=torch.bool)

    def run(vis=vis, bias=bias):
        return O.softmax_over_visible(qs, K, V, vis, bias, d.scale)

    def q_blocks():
        for b in range(c.B):
            for h in range(c.H):
                for i in (c.q_blocks or range(c.nb)):
                    yield b, h, i, (qblk == i)

    def kept(b, h, i, p):
        return torch.nonzero(d.mask[b, h, i] == p).flatten().tolist()

    def keys_of(p, j):
        n = BLOCK // p
        return slice(off[p] + j * n, off[p] + (j + 1) * n)

    if c.group == "b":
        for p, per_tile in ((4, 2), (8, 4)):
            v2, rows = vis.clone(), none.clone()
            for b, h, i, rr in q_blocks():
                cols = kept(b, h, i, p)
                if len(cols) % per_tile:
                    v2[b, h, rr, keys_of(p, cols[-1])] = False
                    rows[b, h] |= rr
            if rows.any():
                yield (f"last block of a partial level-{p} tile dropped",) + run(vis=v2) + (rows,)
        for part in ("q-block", "32 rows"):
            v2, rows = vis.clone(), none.clone()
            for b, h, i, rr in q_blocks():
                if part == "32 rows":
                    rr = rr & (pos % BLOCK >= 32) & (pos % BLOCK < 64)
                for p, per_tile in ((4, 2), (8, 4)):
                    cols = kept(b, h, i, p)
                    if len(cols) % per_tile:
                        v2[b, h, rr, keys_of(p, cols[-1]).stop - 1] = False
                        rows[b, h] |= rr
            if rows.any():
                yield (f"last pyramid row of a partial tile lost ({part})",) + run(vis=v2) + (rows,)
        for name, p, new in (("level-8 bias ln 4", 8, math.log(4.0)), ("level-2 bias lost", 2, 0.0)):
            b2 = bias.clone()
            b2[lvl == p] = new
            rows, mixed = none.clone(), False
            for b, h, i, rr in q_blocks():
                n = _counts(d.mask[b, h, i].tolist())
                if n[ML.LEVELS.index(p)]:
                    rows[b, h] |= rr
                    mixed |= sum(1 for x in n if x) > 1
            if mixed:     # a row of one level alone: the bias moves its LSE, not its output
                yield (name,) + run(bias=b2) + (rows,)
    if c.group == "c" and c.L % BLOCK:
        rows = none.clone()
        for b, h, i, rr in q_blocks():
            if int(d.mask[b, h, i, -1]) == 1:
                rows[b, h] |= rr
        pads = c.nb * BLOCK - c.L
        if pads >= BLOCK // 4:
            out, lse = ML.multilevel_attention_fp64(qs, d.k, d.v, d.mask, sm_scale=d.scale, ref_tail=not c.ref_tail)
            yield ("ref_tail ignored", out, lse, rows)
        if c.L >= 2:
            v2 = vis.clone()
            v2[..., c.L - 1] = False
            yield ("last real key dropped",) + run(vis=v2) + (rows,)
    if pos.numel() >= 2 and int(qblk[-1]) == int(qblk[-2]):
        out, lse = r.ref.clone(), r.ref_lse.clone()
        out[:, :, -1], lse[:, :, -1] = r.ref[:, :, -2], r.ref_lse[:, :, -2]
        only = none.clone()
        only[:, :, -1] = True
        yield ("tail row takes its neighbour's", out, lse, only)
    if c.group == "g":
        for p in ML.LEVELS:
            v2, rows = vis.clone(), none.clone()
            for b, h, i, rr in q_blocks():
                cols = kept(b, h, i, p)
                if cols and cols[-1] >= 64:
                    v2[b, h, rr, keys_of(p, cols[-1])] = False
                    rows[b, h] |= rr
            assert rows.any()
            yield (f"kept level-{p} block past column 64 dropped",) + run(vis=v2) + (rows,)


@pytest.mark.parametrize("group", ["b", "c", "g"])
def test_bounds_see_the_faults_they_are_for(group):
    low = {}
    for c in M.by_group(group):
        r = M.reference(c)
        bound = max(float(r.bounds_t.max()), float(r.bounds_i.max()))
        for name, out, lse, rows in mutations(c):
            worst = O.per_row_error(out, r.ref)[0]
            assert worst >= 4.0 * bound, (c.id, name, worst, bound)
            shift = (lse - r.ref_lse).abs()
            shift = torch.where(torch.isnan(shift), torch.zeros_like(shift), shift)[rows]   # -inf - -inf: no change
            assert shift.numel() > 0, (c.id, name)
            assert c.unit
            assert float(shift.min()) >= 2.0 * r.lse_bound, (c.id, name, float(shift.min()), r.lse_bound)
            lo = low.get(name, (math.inf, math.inf))
            low[name] = (min(lo[0], worst / bound if bound > 0 else math.inf), min(lo[1], float(shift.min()) / r.lse_bound))
    want = {"b": 6, "c": 3, "g": 5}[group]
    assert len(low) >= want, sorted(low)
    record(f"multi-level forward mutations, {group}: smallest (worst row / bound, LSE shift / LSE bound)",
           {k: f"{a:.1f}x, {b:.1f}x" for k, (a, b) in low.items()})
