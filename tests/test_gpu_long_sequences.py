"""Sequences past 40960 tokens: vb_mask_predict_long (rows of up to 1024 blocks, L <= 131072), the
energy rule on rows of up to 1024 columns, and the adaptive module at the Wan 720p grid
(80x45x21 latents, L = 75600, 591 blocks).

The long entry is a second instantiation of the score kernel: its epilogue's semantics are the
short one's (stable descending rank, one sequential fp32 cumulative chain rounded per prefix to the
storage dtype, clamp, forced tail), so every mask here is checked exactly against the oracle's energy
rule on the GPU's own scores, and the scores with the short path's own criteria (quarter-integer
inputs make every fp32 dot product exact: exact share >= 0.999, max |diff| <= 2^-7)."""
import ctypes
import time

import numpy as np
import pytest
import torch

import bsa_oracle as O

gpu = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()
    from vblade import ops
    return ops


def _rand(*shape, dtype=BF16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _exact_inputs(B, H, L, D, seed):
    """bf16 values with few mantissa bits (test_gpu_forward._exact_inputs): every fp32 partial dot
    product is exact, so GPU and CPU pooled scores agree regardless of summation order."""
    g = torch.Generator().manual_seed(seed)
    cent = torch.randint(-2, 3, (B, H, L // 64 + 1, D), generator=g).repeat_interleave(64, 2)[:, :, :L]
    x = torch.randint(-2, 3, (B, H, L, D), generator=g) + cent
    return (x.float() / 4).to(BF16)


def _offsets(seed, B=1, H=1):
    g = torch.Generator().manual_seed(seed)
    qo = torch.topk(torch.rand(B, H, 1, 128, generator=g), 32, dim=3).indices[:, :, 0]
    ko = torch.topk(torch.rand(B, H, 1, 128, generator=g), 32, dim=3).indices[:, :, 0]
    return qo, ko, g


def _retain(nb, variant):
    from vblade.attention import retain_counts
    lo, hi = retain_counts(nb, 0.05, 0.1 if variant == "cog" else 0.17, variant)
    return lo, hi, (2 if variant == "cog" else 0)


def _pooled_rows(q, k, perm, qo, ko, qblocks, store=BF16):
    """bsa_oracle.pooled_scores' steps (replicate pad, per-block sampling, block row maxima rounded
    to the storage dtype, the unrounded running row max, exp2, the storage-dtype normalisation) for
    the sampled q-blocks ``qblocks`` only, against all keys; B = H = 1. Returns [1,1,len(qblocks),nb]."""
    L, D = q.shape[2], q.shape[3]
    nb = (L + 127) // 128

    def sample(x, off, blocks):
        pos = (torch.as_tensor(list(blocks))[:, None] * 128 + off[None, :].long()).clamp(max=L - 1)
        return x[:, :, perm[pos.reshape(-1)]]

    qs, ks = sample(q, qo[0, 0], qblocks), sample(k, ko[0, 0], range(nb))
    nq = len(qblocks)
    qk_scale = float(np.float32(1.0 / D ** 0.5) * np.float32(O.LOG2E))
    S = torch.matmul(qs.float(), ks.float().transpose(-1, -2))
    rowblk = S.reshape(1, 1, nq * 32, nb, 32).amax(-1) * np.float32(qk_scale)
    m = rowblk.amax(-1, keepdim=True)
    w = torch.exp2(O.rnd(rowblk, store) - m)
    po = O.rnd(w.reshape(1, 1, nq, 32, nb).amax(3), store)
    tot = O.rnd(po.sum(-1, keepdim=True), store)
    return O.rnd(po / tot, store)


def _check_scores(po_rows, ref_rows):
    exact = (po_rows == ref_rows).float().mean().item()
    worst = (po_rows - ref_rows).abs().max().item()
    print(f"scores: exact share {exact:.5f}, max |diff| {worst:.3g}")
    assert exact >= 0.999, exact
    assert worst <= 2 ** -7, worst


# ------------------------------------------------------------------ 1. long entry == short entry
@gpu
@pytest.mark.parametrize("L,D,ft", [(17776, 64, 2), (40960, 128, 0)])
def test_long_entry_writes_the_short_entrys_bits(ops, L, D, ft):
    """Up to 320 blocks both entries accept the call: scores, mask, kept counts are bit-identical."""
    q, k = _exact_inputs(1, 1, L, D, 1).to(DEV), _exact_inputs(1, 1, L, D, 2).to(DEV)
    qo, ko, g = _offsets(7)
    perm = torch.randperm(L, generator=g).int().to(DEV)
    nb = (L + 127) // 128
    got = []
    for long_rows in (False, True):
        cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
        kept = torch.full((1, 1, nb), -1, dtype=torch.int32, device=DEV)
        po, mask = ops.mask_predict(q, k, qo.int().to(DEV), ko.int().to(DEV), rows=perm, min_keep=nb // 20,
                                    max_keep=nb // 6, force_tail=ft, mask_count=cnt, rows_kept=kept,
                                    long_rows=long_rows)
        got.append((po, mask, cnt, kept))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert torch.equal(got[1][3].long().sum(), got[1][2][0]) and int(got[1][2]) == int(got[1][1].sum())


# ------------------------------------------------------------------ 2. energy rule on long rows
@gpu
@pytest.mark.parametrize("variant", ["wan", "cog"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("nc", [321, 384, 385, 591, 1023, 1024])
def test_energy_mask_on_rows_past_320_columns(ops, nc, dtype, variant):
    """Row-normalised random rows this wide are full of equal storage values, so the stable tie order
    decides the boundary. Row 0 holds all-equal values, row 1 more than the threshold in its first
    entry (rows 6, 7 are the forced tail rows of "cog")."""
    nr = 8
    g = torch.Generator().manual_seed(nc)
    p = torch.rand(1, 1, nr, nc, generator=g)
    p[0, 0, 0] = 1.0
    p[0, 0, 1] = 0.03 / (nc - 1)
    p[0, 0, 1, 0] = 0.97
    po = (p / p.sum(-1, keepdim=True)).to(dtype)
    lo, hi, ft = _retain(nc, variant)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    m = ops.energy_mask(po.to(DEV), min_keep=lo, max_keep=hi, force_tail=ft, mask_count=cnt).bool().cpu()
    t0 = time.perf_counter()
    ref = O.energy_mask(po, lo, hi, 0.95, ft, store_dtype=dtype)
    assert time.perf_counter() - t0 < 0.5   # the oracle stays cheap at these widths
    assert torch.equal(m, ref), (m != ref).nonzero()[:8]
    assert cnt.item() == int(ref.sum())


# ------------------------------------------------------------------ 3. first width past the old cap
@gpu
def test_long_predictor_matches_oracle_at_321_blocks(ops):
    """321 blocks with a replicate-padded tail (L = 321*128 - 47), D = 64, rows through a random
    permutation, forced tail 2: the full oracle."""
    L, D = 321 * 128 - 47, 64
    q, k = _exact_inputs(1, 1, L, D, 1), _exact_inputs(1, 1, L, D, 2)
    qo, ko, g = _offsets(7)
    perm = torch.randperm(L, generator=g)
    nb = 321
    lo, hi, ft = _retain(nb, "cog")
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    po, mask = ops.mask_predict(q.to(DEV), k.to(DEV), qo.int().to(DEV), ko.int().to(DEV),
                                rows=perm.int().to(DEV), min_keep=lo, max_keep=hi, force_tail=ft,
                                mask_count=cnt, long_rows=True)
    qs = O.sample_tokens(O.pad_replicate(q[:, :, perm], 128), qo)
    ks = O.sample_tokens(O.pad_replicate(k[:, :, perm], 128), ko)
    ref_po = O.pooled_scores(qs, ks, 1.0 / D ** 0.5, 32, BF16)
    po_c = po.float().cpu()
    _check_scores(po_c, ref_po)
    ref_mask = O.energy_mask(po_c, lo, hi, 0.95, ft)
    assert torch.equal(mask.bool().cpu(), ref_mask)
    assert cnt.item() == int(ref_mask.sum())


# ------------------------------------------------------------------ 4. Wan 720p and the maximum
def _assert_subset_oracle_equals_the_full_oracle():
    """The q-block subset helper reproduces bsa_oracle.pooled_scores on 1000 tokens."""
    L, D = 1000, 64
    q, k = _exact_inputs(1, 1, L, D, 1), _exact_inputs(1, 1, L, D, 2)
    qo, ko, g = _offsets(7)
    perm = torch.randperm(L, generator=g)
    qs = O.sample_tokens(O.pad_replicate(q[:, :, perm], 128), qo)
    ks = O.sample_tokens(O.pad_replicate(k[:, :, perm], 128), ko)
    full = O.pooled_scores(qs, ks, 1.0 / D ** 0.5, 32, BF16)
    assert torch.equal(_pooled_rows(q, k, perm, qo, ko, range(8)), full)
    assert torch.equal(_pooled_rows(q, k, perm, qo, ko, [0, 5, 7]), full[:, :, [0, 5, 7]])


@gpu
@pytest.mark.parametrize("L,D,variant", [(75600, 128, "wan"), (131072, 64, "cog"), (1023 * 128 + 1, 64, "wan")])
def test_long_predictor_at_wan_720p_and_the_maximum(ops, L, D, variant):
    """591 blocks (Wan 720p), 1024 (the limit) and 1024 whose last block holds one real row. The full
    sampled-score matrix is too large for the CPU, so the scores of q-blocks {0, 1, nb/2, nb-2, nb-1}
    are checked against the subset oracle (itself first checked against the full one on 1000 tokens);
    the mask on every row, exactly."""
    _assert_subset_oracle_equals_the_full_oracle()
    q, k = _exact_inputs(1, 1, L, D, 1), _exact_inputs(1, 1, L, D, 2)
    qo, ko, g = _offsets(7)
    perm = torch.randperm(L, generator=g)
    nb = (L + 127) // 128
    lo, hi, ft = _retain(nb, variant)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    po, mask = ops.mask_predict(q.to(DEV), k.to(DEV), qo.int().to(DEV), ko.int().to(DEV),
                                rows=perm.int().to(DEV), min_keep=lo, max_keep=hi, force_tail=ft,
                                mask_count=cnt, long_rows=True)
    po_c = po.float().cpu()
    blocks = [0, 1, nb // 2, nb - 2, nb - 1]
    _check_scores(po_c[:, :, blocks], _pooled_rows(q, k, perm, qo, ko, blocks))
    ref_mask = O.energy_mask(po_c, lo, hi, 0.95, ft)
    assert torch.equal(mask.bool().cpu(), ref_mask)
    assert cnt.item() == int(ref_mask.sum())


# ------------------------------------------------------------------ 5. fused options
@gpu
def test_long_entry_fused_pool_level_and_philox(ops):
    """L = 41000 (321 blocks), D = 128: the pooled K/V pass in the launch, the rank-band level mask
    from the epilogue, and the in-launch Philox draws behave as on the short path."""
    L, D = 41000, 128
    q, k, v = (_rand(1, 1, L, D, seed=s).to(DEV) for s in (1, 2, 3))
    qo, ko, g = _offsets(7)
    qo, ko = qo.int().to(DEV), ko.int().to(DEV)
    rows = torch.randperm(L, generator=g).int().to(DEV)
    nb = (L + 127) // 128
    kw = dict(rows=rows, min_keep=nb // 20, max_keep=nb // 6, long_rows=True)

    po0, mask0 = ops.mask_predict(q, k, qo, ko, **kw)
    outs = ops.pool_kv_outputs(k, 30, reordered=True)
    po1, mask1 = ops.mask_predict(q, k, qo, ko, pool=(v, 30, outs), **kw)
    assert torch.equal(po1, po0) and torch.equal(mask1, mask0)
    for got, ref in zip(outs, ops.pool_kv(k, v, 30, rows, reordered=True)):
        assert torch.equal(got, ref)

    po2, lmask = ops.mask_predict(q, k, qo, ko, rows=rows, level=ops.ML_MASK_RATIOS, long_rows=True)
    assert torch.equal(po2, po0)
    assert torch.equal(lmask, ops.level_mask(po2))

    torch.manual_seed(41)
    torch.rand(3000, device=DEV)
    rq = torch.rand(1, 1, 1, 128, device=DEV)
    rk = torch.rand(1, 1, 1, 128, device=DEV)
    after_ref = torch.rand(7, device=DEV)
    q_off = torch.topk(rq, 32, dim=3).indices[:, :, 0].to(torch.int32)
    k_off = torch.topk(rk, 32, dim=3).indices[:, :, 0].to(torch.int32)
    po_ref, mask_ref = ops.mask_predict(q, k, q_off, k_off, **kw)
    torch.manual_seed(41)
    torch.rand(3000, device=DEV)
    philox = ops.claim_rand_draws(DEV, 128)
    assert philox is not None
    po3, mask3 = ops.mask_predict(q, k, philox=philox, **kw)
    assert torch.equal(torch.rand(7, device=DEV), after_ref)
    assert torch.equal(po3, po_ref) and torch.equal(mask3, mask_ref)


# ------------------------------------------------------------------ 6. the module
@gpu
def test_module_runs_at_the_wan_720p_grid(ops):
    """AdaptiveBlockSparseAttn("wan") on the 80x45x21 grid (L = 75600): the module's mask is the
    stand-alone long predictor's, and the output rows of q-blocks {0, 300, 590} (Gilbert order)
    match the oracle's two-branch attention + reference combine computed from their own mask rows."""
    import vblade
    from vblade.attention import retain_counts
    m = vblade.AdaptiveBlockSparseAttn("wan", width=80, height=45, depth=21, log_every=0)
    L, D, gap = 75600, 128, m.sample_gap
    assert m.gilbert_rearranger.seq_len == L
    q, k, v = (_rand(1, 1, L, D, seed=60 + s) for s in range(3))
    qo, ko, _ = _offsets(9)
    qo, ko = qo.int().to(DEV), ko.int().to(DEV)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    with torch.no_grad():
        out = m(qd, kd, vd, q_off=qo, k_off=ko)
    nb = (L + 127) // 128
    assert nb == 591 and tuple(m.last_mask.shape) == (1, 1, nb, nb)
    lo, hi = retain_counts(nb, m.min_retain_ratio, m.max_retain_ratio, "wan")
    _, mask = ops.mask_predict(qd, kd, qo, ko, rows=m._rows(qd.device), min_keep=lo, max_keep=hi,
                               force_tail=0, long_rows=True)
    assert torch.equal(m.last_mask, mask)
    mask_c = mask.bool().cpu()
    kept = mask_c.sum(-1)
    assert int(kept.min()) >= lo and int(kept.max()) <= hi

    P = m.gilbert_rearranger.rows.long().cpu()
    q_r, k_r, v_r = q[:, :, P], k[:, :, P], v[:, :, P]
    kp, vp = O.simple_pooling(k_r, gap, BF16), O.simple_pooling(v_r, gap, BF16)
    out_c = out.float().cpu()
    for i in (0, 300, 590):
        rows = slice(i * 128, min(L, (i + 1) * 128))
        o1, l1 = O.block_sparse_attention(q_r[:, :, rows], k_r, v_r, mask_c[:, :, i:i + 1])
        o2, l2 = O.block_sparse_attention(q_r[:, :, rows], kp, vp, None)
        ref, _ = O.combine_reference(O.rnd(o1, BF16), l1, O.rnd(o2, BF16), l2, gap, BF16)
        err = (out_c[:, :, P[rows]] - ref).abs().max().item()
        print(f"q-block {i}: max |err| {err:.3g}")
        assert err <= 2.5e-2   # test_gpu_forward._tol(bfloat16)


@gpu
def test_module_under_autograd_past_320_blocks(ops):
    """321 blocks under autograd (the two-branch path): dq/dk/dv of the run that predicts its mask
    equal, bit for bit, those of the run handed that mask through block_mask=, and hold the per-row
    bound (2 x the rounding emulation's worst row) against the gathered fp64 two-branch reference."""
    import vblade
    L, D = 41000, 64
    m = vblade.AdaptiveBlockSparseAttn("cog", width=58, height=37, depth=19, log_every=0)   # + 226 text rows
    assert m.gilbert_rearranger.seq_len == L
    qo, ko, _ = _offsets(11)
    qo, ko = qo.int().to(DEV), ko.int().to(DEV)
    base = [_rand(1, 1, L, D, seed=70 + s).to(DEV) for s in range(4)]

    def run(**kw):
        q, k, v = (t.clone().requires_grad_(True) for t in base[:3])
        out = m(q, k, v, **kw)
        out.backward(base[3])
        return out.detach(), q.grad, k.grad, v.grad

    first = run(q_off=qo, k_off=ko)
    mask = m.last_mask
    assert tuple(mask.shape) == (1, 1, 321, 321) and bool(mask[0, 0, -2:].all()) and not bool(mask.all())
    second = run(block_mask=mask)
    for a, b in zip(first, second):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)

    # both runs launch the same kernels, so a wrong block list would agree with itself: the gradients
    # per row against the gathered two-branch reference (tests/long_bwd_cases.py), which gets the
    # reordered inputs, the module's mask and the device's own out/lse/alpha, recomputed here by
    # _AdaptiveSplitFn.forward's calls and tied to the module's run by the combined output's bits
    import long_bwd_cases as C
    from conftest import record
    rows, gap = m._rows(base[0].device), m.sample_gap
    q, k, v, do = base
    kp, vp, k_r, v_r = ops.pool_kv(k, v, gap, rows, reordered=True)
    out2, lse2 = ops.attention_fwd(q, None, None, use_main=False, q_rows=rows, kp=kp, vp=vp, need_lse=True)
    out1, lse1 = ops.attention_fwd(q, k_r, v_r, block_mask=mask, q_rows=rows, need_lse=True, heavy_rows=m.force_tail)
    out, alpha = ops.lse_combine(out1, lse1, out2, lse2, gap)
    assert torch.equal(out, first[0])
    P = rows.long().cpu()
    lq = lambda t: t.cpu()[:, :, P]  # noqa: E731
    ref, emu = C.backward_reference(lq(q), k_r.cpu(), v_r.cpu(), lq(do), lq(out1), lq(lse1), mask.bool().cpu(), BF16,
                                    kp=kp.cpu(), vp=vp.cpu(), out2=lq(out2), lse2=lq(lse2), alpha=lq(alpha), gap=gap)
    facts = []
    for name, g, r, e in zip(("dq", "dk", "dv"), first[1:], ref, emu):
        bound = O.per_row_bound(e, r, BF16)
        worst, where = O.per_row_error(lq(g.float()), r)
        facts.append(f"{name} {worst:.2e}/{bound / 2:.2e}")
        assert worst <= bound, (name, worst, where, bound)
    record("module under autograd at 321 blocks, worst row: gpu/emulation (bound: 2x emulation)", " ".join(facts))


# ------------------------------------------------------------------ 7. CPU: the entry's validation
def test_long_entry_argument_checks_without_gpu():
    from vblade import _lib
    lib = _lib.load()

    def args(L, H=1):
        p = _lib.PredictArgs()
        p.q = p.k = p.q_off = p.k_off = p.po = p.mask = 1 << 20
        p.B, p.H, p.L, p.D, p.block, p.num_keep = 1, H, L, 64, 128, 32
        p.q_stride = p.k_stride = (H * L * 64, L * 64, 64)
        p.min_keep = p.max_keep = 1
        p.workspace = 1 << 24
        p.workspace_bytes = lib.vb_mask_predict_workspace_size(ctypes.byref(p))
        return p

    assert lib.vb_mask_predict_long(None, None) == _lib.VB_ERR_INVALID
    p = args(1000)
    p.po = None
    assert lib.vb_mask_predict_long(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert b"vb_mask_predict_long" in lib.vb_last_error() and b"null" in lib.vb_last_error()
    p = args(1024 * 128 + 1)   # 1025 blocks
    assert lib.vb_mask_predict_long(ctypes.byref(p), None) == _lib.VB_ERR_UNSUPPORTED
    assert b"too long" in lib.vb_last_error()
    # 1024 blocks (L = 131072 > 65535) pass the length checks: the next refusal is a later check's
    p = args(1024 * 128)
    p.min_keep = 0
    assert lib.vb_mask_predict_long(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert b"keep counts" in lib.vb_last_error()
    # the short entry keeps its limit
    p = args(321 * 128)
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_UNSUPPORTED
    assert b"too long" in lib.vb_last_error()
    # vb_energy_mask: 1025 columns are refused
    assert lib.vb_energy_mask(1 << 20, 1, 1, 1, 1025, 0.95, 1, 1, 0, 0, 1 << 20, None, None) == _lib.VB_ERR_UNSUPPORTED
