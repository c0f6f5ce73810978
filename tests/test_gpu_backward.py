"""GPU parity of the backward kernels (vb_attn_bwd / vb_block_sparse_attn_bwd, through the C ABI)
against the oracle's FlashAttention-2-semantics backward (oracle/bsa_oracle.py, fp64) on the same
inputs and the same forward statistics (out, lse).

Tolerance: relative Frobenius error ||g - g_ref|| / ||g_ref|| <= 2e-2 per gradient. The kernels
feed P and dS to the MFMAs in the storage dtype (as the reference library's backward does) and
accumulate in fp32; the oracle keeps everything in fp64 — bf16 rounding of P/dS alone gives
errors of ~4e-3 relative. The two op-level oracle tests also hold every row to the per-row bound of
tests/test_gpu_backward_branches.py (2x the rounding emulation's worst row on the same inputs).
"""
import math

import numpy as np
import pytest
import torch

import bsa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _rand(*shape, dtype=torch.bfloat16, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype)


def rel(x, ref):
    ref = ref.double()
    return ((x.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _ops():
    from vblade import ops
    return ops


def _main_branch_emulation(q, k, v, out, lse, do, mask, dtype):
    """The oracle's storage-rounding emulation of the main-branch backward on a test's own inputs:
    O.per_row_bound turns its worst row into the per-row bound (tests/test_gpu_backward_branches.py)."""
    return O.two_branch_attention_bwd(q, k, v, None, None, out.cpu(), lse.cpu(), None, None, None, do, mask, 0,
                                      store_dtype=dtype, emulate_rounding=True)


@pytest.mark.parametrize("L,D,dtype,density", [(300, 64, torch.bfloat16, 0.5),
                                               (256, 128, torch.bfloat16, 1.0),
                                               (517, 64, torch.float16, 0.3),
                                               (260, 128, torch.bfloat16, 0.6),
                                               (1000, 64, torch.bfloat16, 0.25),
                                               (333, 128, torch.float16, 0.4),
                                               (40, 128, torch.bfloat16, 1.0),    # one partial tile
                                               (40, 64, torch.float16, 1.0)])
def test_block_sparse_bwd_matches_oracle(L, D, dtype, density):
    B, H = 1, 2
    q, k, v, do = (_rand(B, H, L, D, dtype=dtype, seed=s) for s in range(4))
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, density, seed=7)
    ops = _ops()
    out, lse = ops.attention_fwd(q.to(DEV), k.to(DEV), v.to(DEV), block_mask=mask.to(DEV),
                                 need_lse=True)
    dq, dk, dv = ops.attention_bwd(do.to(DEV), q.to(DEV), k.to(DEV), v.to(DEV), out, lse,
                                   block_mask=mask.to(DEV))
    rq, rk, rv = O.block_sparse_attention_bwd(q, k, v, out.cpu(), lse.cpu(), do, mask)
    emu = _main_branch_emulation(q, k, v, out, lse, do, mask, dtype)
    for name, g, r, e in (("dq", dq, rq, emu[0]), ("dk", dk, rk, emu[1]), ("dv", dv, rv, emu[2])):
        assert torch.isfinite(g).all(), name
        assert rel(g, r) <= TOL, (name, rel(g, r))
        assert O.per_row_error(g, r)[0] <= O.per_row_bound(e, r, dtype), (name, O.per_row_error(g, r))


@pytest.mark.parametrize("L,D,dtype,density", [(1000, 64, torch.bfloat16, 0.25), (1000, 128, torch.bfloat16, 0.25),
                                               (517, 64, torch.float16, 0.3), (700, 128, torch.float16, 0.4),
                                               (300, 64, torch.bfloat16, 0.5), (260, 128, torch.bfloat16, 0.6)])
def test_default_backward_kernels_at_the_rounding_floor(L, D, dtype, density):
    """The default kernels (hand-placed dK/dV stream, 2-slot dQ) against the fp64 oracle at a bound
    near their storage-rounding floor instead of TOL: measured 2.3-2.4e-3 (bf16) and 2.9-3.0e-4
    (f16) relative per gradient (tools/diag/bwd_parity_err.py, gpurun_out r05_c27), bound ~1.7x."""
    B, H = 1, 2
    q, k, v, do = (_rand(B, H, L, D, dtype=dtype, seed=s) for s in range(4))
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, density, seed=7)
    ops = _ops()
    out, lse = ops.attention_fwd(q.to(DEV), k.to(DEV), v.to(DEV), block_mask=mask.to(DEV), need_lse=True)
    dq, dk, dv = ops.attention_bwd(do.to(DEV), q.to(DEV), k.to(DEV), v.to(DEV), out, lse, block_mask=mask.to(DEV))
    rq, rk, rv = O.block_sparse_attention_bwd(q, k, v, out.cpu(), lse.cpu(), do, mask)
    tight = 4e-3 if dtype == torch.bfloat16 else 6e-4
    emu = _main_branch_emulation(q, k, v, out, lse, do, mask, dtype)
    for name, g, r, e in (("dq", dq, rq, emu[0]), ("dk", dk, rk, emu[1]), ("dv", dv, rv, emu[2])):
        assert rel(g, r) <= tight, (name, rel(g, r))
        assert O.per_row_error(g, r)[0] <= O.per_row_bound(e, r, dtype), (name, O.per_row_error(g, r))


def _lib_bits():
    from vblade import _lib
    return _lib


@pytest.mark.parametrize("D", [64, 128])
def test_default_backward_reports_the_pipeline_kernels(D):
    """kernel_select = 0 launches the hand-placed dK/dV stream and the 2-slot pipeline dQ, and the
    call says so (vb_attn_bwd_args.kernels_ran): the tests below compare kernels that really ran."""
    L = 300
    q, k, v, do = (_rand(1, 2, L, D, seed=40 + s) for s in range(4))
    mask = O.block_mask_from_density(1, 2, 3, 3, 0.6, seed=1)
    ops, lib = _ops(), _lib_bits()
    qd, kd, vd, dod, md = (t.to(DEV) for t in (q, k, v, do, mask))
    out, lse = ops.attention_fwd(qd, kd, vd, block_mask=md, need_lse=True)
    ran = []
    ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md, kernels_ran=ran)
    assert ran == [lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_PIPE_RING2]


@pytest.mark.parametrize("D", [64, 128])
def test_pipeline_dkdv_agrees_with_round3_kernel(D):
    """The hand-scheduled dK/dV kernels (vb_attn_bwd_kv.hip, default) against the round-3
    bwd_dkdv_kernel (kernel_select VB_BWD_SEL_DKDV_ROUND3) on the same inputs, each launch's kernels
    asserted from kernels_ran: bit-identical at D=64 (the same -Delta seeding and summation order),
    within bf16 rounding at D=128 (the pipeline seeds dP with -Delta, the round-3 D=128 kernel added it
    after the chain). dQ is the same kernel in both runs. Both against the fp64 oracle too."""
    B, H, L = 1, 2, 700
    q, k, v, do = (_rand(B, H, L, D, seed=20 + s) for s in range(4))
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, 0.5, seed=3)
    ops, lib = _ops(), _lib_bits()
    qd, kd, vd, dod, md = (t.to(DEV) for t in (q, k, v, do, mask))
    out, lse = ops.attention_fwd(qd, kd, vd, block_mask=md, need_lse=True)
    ran_new, ran_old = [], []
    new = ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md, kernels_ran=ran_new)
    old = ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md,
                            kernel_select=lib.VB_BWD_SEL_DKDV_ROUND3, kernels_ran=ran_old)
    assert ran_new == [lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_PIPE_RING2]
    assert ran_old == [lib.VB_BWD_RAN_DKDV_ROUND3 | lib.VB_BWD_RAN_DQ_PIPE_RING2]
    assert torch.equal(new[0], old[0])                      # dq
    for a, b in zip(new[1:], old[1:]):
        if D == 64:
            assert torch.equal(a, b)
        else:
            assert rel(a.float().cpu(), b.float().cpu()) <= 5e-3
    rq, rk, rv = O.block_sparse_attention_bwd(q, k, v, out.cpu(), lse.cpu(), do, mask)
    for g, r in zip(old, (rq, rk, rv)):
        assert rel(g, r) <= 4e-3


@pytest.mark.parametrize("D,sel", [(64, "round3"), (128, "round3"), (64, "ring4"), (128, "ring4")])
def test_pipeline_dq_agrees_with_selected_kernels(D, sel):
    """The default dQ (2-slot pipeline) against the round-3 bwd_dq_kernel (VB_BWD_SEL_DQ_ROUND3) and
    the 4-slot pipeline (VB_BWD_SEL_DQ_RING4) on a ragged length with a partial last key tile: each
    launch's kernels asserted from kernels_ran, dk/dv identical (the same dK/dV kernel), dq within
    bf16 rounding of the default and at the oracle's rounding floor."""
    B, H, L = 1, 2, 517
    q, k, v, do = (_rand(B, H, L, D, seed=30 + s) for s in range(4))
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, 0.5, seed=4)
    ops, lib = _ops(), _lib_bits()
    qd, kd, vd, dod, md = (t.to(DEV) for t in (q, k, v, do, mask))
    out, lse = ops.attention_fwd(qd, kd, vd, block_mask=md, need_lse=True)
    bit = lib.VB_BWD_SEL_DQ_ROUND3 if sel == "round3" else lib.VB_BWD_SEL_DQ_RING4
    ran_bit = lib.VB_BWD_RAN_DQ_ROUND3 if sel == "round3" else lib.VB_BWD_RAN_DQ_PIPE_RING4
    ran_new, ran_old = [], []
    new = ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md, kernels_ran=ran_new)
    old = ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md, kernel_select=bit, kernels_ran=ran_old)
    assert ran_new == [lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_PIPE_RING2]
    assert ran_old == [lib.VB_BWD_RAN_DKDV_PIPE | ran_bit]
    assert torch.isfinite(old[0]).all()
    assert rel(new[0].float().cpu(), old[0].float().cpu()) <= 5e-3
    assert torch.equal(new[1], old[1]) and torch.equal(new[2], old[2])
    rq, _, _ = O.block_sparse_attention_bwd(q, k, v, out.cpu(), lse.cpu(), do, mask)
    assert rel(old[0], rq) <= 4e-3


def test_kernel_select_rejects_unknown_bits():
    L, D = 128, 64
    q, k, v, do = (_rand(1, 1, L, D, seed=s).to(DEV) for s in range(4))
    ops = _ops()
    from vblade import _lib
    out, lse = ops.attention_fwd(q, k, v, need_lse=True)
    with pytest.raises(_lib.VBladeError):
        ops.attention_bwd(do, q, k, v, out, lse, kernel_select=8)


def test_bwd_empty_rows_and_columns_and_determinism():
    """A q-block row with no kept block (lse = -inf, out = 0) gets dq = 0 and contributes nothing;
    a key block kept by no row gets dk = dv = 0. Two runs are bitwise identical (no atomics)."""
    B, H, L, D = 1, 2, 384, 64
    q, k, v, do = (_rand(B, H, L, D, seed=10 + s) for s in range(4))
    mask = O.block_mask_from_density(B, H, 3, 3, 0.6, seed=2)
    mask[:, 0, 1, :] = False      # head 0: q-block 1 keeps nothing
    mask[:, 1, :, 2] = False      # head 1: key block 2 kept by nobody
    ops = _ops()
    qd, kd, vd, dod, md = (t.to(DEV) for t in (q, k, v, do, mask))
    out, lse = ops.attention_fwd(qd, kd, vd, block_mask=md, need_lse=True)
    g1 = ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md)
    g2 = ops.attention_bwd(dod, qd, kd, vd, out, lse, block_mask=md)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)
    dq, dk, dv = (t.float().cpu() for t in g1)
    assert torch.isfinite(dq).all() and torch.isfinite(dk).all() and torch.isfinite(dv).all()
    assert dq[0, 0, 128:256].abs().max() == 0
    assert dk[0, 1, 256:].abs().max() == 0 and dv[0, 1, 256:].abs().max() == 0
    lse_c = lse.cpu().clone()
    lse_c[torch.isinf(lse_c)] = float("inf")   # oracle: P = exp(-inf - inf) = 0 on empty rows
    rq, rk, rv = O.block_sparse_attention_bwd(q, k, v, out.cpu(), lse_c, do, mask)
    for g, r in ((dq, rq), (dk, rk), (dv, rv)):
        assert rel(g, r) <= TOL


@pytest.mark.parametrize("lens", [[300, 170], [300, 0, 170]])   # the second with an empty sequence
def test_block_sparse_attn_func_autograd_varlen(lens):
    """Reference-API drop-in (block_sparse_attn_func, varlen layout, head_mask_type = ones ->
    per-head masks) differentiated by torch.autograd, per sequence against the oracle."""
    import vblade
    H, D = 2, 64
    tot = sum(lens)
    q, k, v, do = (_rand(tot, H, D, seed=20 + s) for s in range(4))
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32)
    nb = (max(lens) + 127) // 128
    mask = O.block_mask_from_density(len(lens), H, nb, nb, 0.5, seed=4)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = vblade.block_sparse_attn_func(qd, kd, vd, cu.to(DEV), cu.to(DEV),
                                        torch.ones(H, dtype=torch.int32, device=DEV), None,
                                        mask.to(DEV), max(lens), max(lens), 0.0,
                                        deterministic=True)
    out.backward(do.to(DEV))
    for bi, Lb in enumerate(lens):
        if Lb == 0:
            continue
        s0 = int(cu[bi])
        sl = lambda t: t[s0:s0 + Lb].permute(1, 0, 2)[None].float()  # noqa: E731
        nbb = (Lb + 127) // 128
        mb = mask[bi:bi + 1, :, :nbb, :nbb]
        ro, rlse = O.block_sparse_attention(sl(q), sl(k), sl(v), mb)
        rq, rk, rv = O.block_sparse_attention_bwd(sl(q), sl(k), sl(v), sl(out.detach().cpu()),
                                                  rlse, sl(do), mb)
        assert rel(sl(out.detach().cpu()), ro) <= TOL
        for g, r in ((qd.grad, rq), (kd.grad, rk), (vd.grad, rv)):
            assert rel(sl(g.cpu()), r) <= TOL


def _small_module(variant):
    import vblade
    if variant == "cog":
        kw = dict(width=12, height=8, depth=5, text_length=40, sample_gap=15,
                  min_retain_ratio=0.4, max_retain_ratio=0.6)
        cfg = O.AdaptiveConfig.cogvideox(width=12, height=8, depth=5, text_length=40,
                                         sample_gap=15, min_retain_ratio=0.4, max_retain_ratio=0.6)
    else:
        kw = dict(width=10, height=6, depth=6, sample_gap=30, min_retain_ratio=0.3,
                  max_retain_ratio=0.6)
        cfg = O.AdaptiveConfig.wan(width=10, height=6, depth=6, sample_gap=30,
                                   min_retain_ratio=0.3, max_retain_ratio=0.6)
    return vblade.AdaptiveBlockSparseAttn(variant, log_every=0, **kw), cfg


def _realistic(B, H, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(B, H, L // 128 + 1, D, generator=g).repeat_interleave(128, 2)[:, :, :L]
    q = (torch.randn(B, H, L, D, generator=g) + 2 * cent).to(torch.bfloat16)
    k = (torch.randn(B, H, L, D, generator=g) + 2 * cent).to(torch.bfloat16)
    v = torch.randn(B, H, L, D, generator=g).to(torch.bfloat16)
    do = torch.randn(B, H, L, D, generator=g).to(torch.bfloat16)
    return q, k, v, do


def _check_adaptive_grads(m, cfg, q, k, v, do, tight=None):
    tight = tight or {}
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = m(qd, kd, vd)
    out.backward(do.to(DEV))
    mask = m.last_mask.bool().cpu()
    fwd = O.adaptive_attention(q, k, v, cfg, None, None, mask=mask)
    assert rel(out.detach().float().cpu(), fwd["out"]) <= tight.get("out", TOL)
    rq, rk, rv = O.adaptive_attention_bwd(q, k, v, do, cfg, fwd)
    for name, g, r in (("dq", qd.grad, rq), ("dk", kd.grad, rk), ("dv", vd.grad, rv)):
        assert torch.isfinite(g).all(), name
        assert rel(g, r) <= tight.get(name, TOL), (name, rel(g, r))


@pytest.mark.parametrize("variant,H,D", [("cog", 2, 64), ("wan", 2, 128)])
def test_adaptive_module_backward_matches_oracle(variant, H, D):
    """Training path (grad enabled): the reference's two-branch autograd — alpha detached,
    pooled-branch K/V grads through the mean pool, Gilbert gather transposed. Besides TOL, a bound
    near the measured errors (r05_c27: out 2.0e-3 / 1.7e-3, dq 8.0e-3 / 7.9e-3 — the bf16 combine
    weight and both branches' dS — dk 3.1e-3 / 2.5e-3, dv 2.5e-3 / 2.3e-3)."""
    m, cfg = _small_module(variant)
    L = m.gilbert_rearranger.seq_len
    q, k, v, do = _realistic(1, H, L, D, seed=3)
    _check_adaptive_grads(m, cfg, q, k, v, do, tight=dict(out=3e-3, dq=1.2e-2, dk=5e-3, dv=4e-3))


@pytest.mark.parametrize("variant,D", [("cog", 64), ("wan", 128)])
def test_full_size_adaptive_backward_one_head(variant, D):
    """Full CogVideoX (L=17776) / Wan (L=32760) sequence, one head, reference retain ratios."""
    import vblade
    m = vblade.AdaptiveBlockSparseAttn(variant, log_every=0)
    cfg = O.AdaptiveConfig.cogvideox() if variant == "cog" else O.AdaptiveConfig.wan()
    L = m.gilbert_rearranger.seq_len
    q, k, v, do = _realistic(1, 1, L, D, seed=5)
    _check_adaptive_grads(m, cfg, q, k, v, do)


@pytest.mark.parametrize("B", [2, 5])
def test_training_batch_matches_per_sample(B):
    """B=5 is the reference's TDM micro-batch (train_tdm_1.sh:14): each sample's grads equal the
    B=1 grads."""
    m, cfg = _small_module("cog")
    L = m.gilbert_rearranger.seq_len
    q, k, v, do = _realistic(B, 2, L, 64, seed=8)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = m(qd, kd, vd)
    out.backward(do.to(DEV))
    mask_model = m.last_mask
    for b in range(B):
        qb, kb, vb = (t[b:b + 1].to(DEV).requires_grad_(True) for t in (q, k, v))
        ob = m(qb, kb, vb, block_mask=mask_model[b:b + 1])
        ob.backward(do[b:b + 1].to(DEV))
        assert math.isclose(rel(qb.grad, qd.grad[b:b + 1].cpu()), 0.0, abs_tol=1e-6)
        assert math.isclose(rel(kb.grad, kd.grad[b:b + 1].cpu()), 0.0, abs_tol=1e-6)
        assert math.isclose(rel(vb.grad, vd.grad[b:b + 1].cpu()), 0.0, abs_tol=1e-6)


def test_full_size_b5_training_batch_one_head():
    """BASELINE config 5's micro-batch at the full CogVideoX sequence: q,k,v [5,1,17776,64] with
    grad. Every sample's dq/dk/dv equals its own B=1 run, and sample 0 matches the oracle's
    reference-semantics backward."""
    import vblade
    m = vblade.AdaptiveBlockSparseAttn("cog", log_every=0)
    cfg = O.AdaptiveConfig.cogvideox()
    L = m.gilbert_rearranger.seq_len
    q, k, v, do = _realistic(5, 1, L, 64, seed=11)
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out = m(qd, kd, vd)
    out.backward(do.to(DEV))
    mask = m.last_mask
    for b in range(5):
        qb, kb, vb = (t[b:b + 1].to(DEV).requires_grad_(True) for t in (q, k, v))
        ob = m(qb, kb, vb, block_mask=mask[b:b + 1])
        ob.backward(do[b:b + 1].to(DEV))
        assert torch.equal(ob, out[b:b + 1])
        for g1, g5 in ((qb.grad, qd.grad), (kb.grad, kd.grad), (vb.grad, vd.grad)):
            assert torch.equal(g1, g5[b:b + 1])
    fwd = O.adaptive_attention(q[:1], k[:1], v[:1], cfg, None, None, mask=mask[:1].bool().cpu())
    assert rel(out[:1].detach().float().cpu(), fwd["out"]) <= TOL
    rq, rk, rv = O.adaptive_attention_bwd(q[:1], k[:1], v[:1], do[:1], cfg, fwd)
    for name, g, r in (("dq", qd.grad[:1], rq), ("dk", kd.grad[:1], rk), ("dv", vd.grad[:1], rv)):
        assert rel(g, r) <= TOL, (name, rel(g, r))


def test_d128_backward_dq_side_stream_is_joined():
    """Round 6: at D=128 the backward launches dQ on a library-owned side stream beside the dK/dV
    chain (ForkScope, vb_attn_bwd.hip) and joins it back with an event before returning. Work on
    the caller's stream right after the call must see the finished dQ: a reduction queued on the
    caller's (non-default) stream without any synchronisation equals the one taken after a device
    synchronize, over repeated calls, and the gradients are the same bits every time."""
    B, H, L, D = 1, 4, 1000, 128
    q, k, v, do = (_rand(B, H, L, D, seed=40 + s).to(DEV) for s in range(4))
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, 0.5, seed=41).to(DEV)
    ops = _ops()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        out, lse = ops.attention_fwd(q, k, v, block_mask=mask, need_lse=True)
        ref = ops.attention_bwd(do, q, k, v, out, lse, block_mask=mask)
        sums = []
        for _ in range(4):
            dq, dk, dv = ops.attention_bwd(do, q, k, v, out, lse, block_mask=mask)
            sums.append(dq.float().sum())   # queued on st right behind the call, no sync
            assert torch.equal(dq, ref[0]) and torch.equal(dk, ref[1]) and torch.equal(dv, ref[2])
    torch.cuda.synchronize()
    want = ref[0].float().sum()
    assert all(torch.equal(s_, want) for s_ in sums)


def test_wan_training_path_forks_are_bit_identical_to_one_stream():
    """Round 6: at D=128 the training forward runs its pooled-only LSE branch on a side stream
    (autograd.FORK_POOLED_BRANCH; the backward forks its dQ in both runs, vb_attn_bwd's ForkScope).
    The module's output and all three gradients equal, bit for bit, those of the one-stream
    training forward, on a caller-created stream, twice in a row."""
    from vblade import autograd as va
    m, _ = _small_module("wan")
    L = m.gilbert_rearranger.seq_len
    q, k, v, do = _realistic(1, 2, L, 128, seed=21)

    def run(fork):
        va.FORK_POOLED_BRANCH = fork
        qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
        torch.cuda.manual_seed(5)
        out = m(qd, kd, vd)
        out.backward(do.to(DEV))
        return out.detach(), qd.grad, kd.grad, vd.grad

    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            ref = run(False)
            got = [run(True) for _ in range(2)]
        torch.cuda.synchronize()
    finally:
        va.FORK_POOLED_BRANCH = True
    for g in got:
        assert all(torch.equal(a, b) for a, b in zip(g, ref))
