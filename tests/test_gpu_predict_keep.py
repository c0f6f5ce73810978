"""GPU: the mask predictor at sampling densities of 16 and 64 tokens per block (num_keep).

The semantics are the oracle's pooled_scores(qs, ks, scale, keep) followed by the unchanged energy /
level epilogue. The acceptance criteria of the score test are those of
test_gpu_forward.test_mask_predict_matches_oracle (exact inputs: every fp32 partial dot product is
exact, so the scores agree to the bit whatever the summation order), on the smallest shapes at which
each mechanism of the new instantiations can break."""
import ctypes
import math

import pytest
import torch

import bsa_oracle as O
import ml_oracle as ML

pytestmark = pytest.mark.gpu
DEV = "cuda"
KEEPS = [16, 64]

# case -> (variant, L, D, H, long entry)
CASES = {
    "a": ("cog", 100, 64, 1, False),     # one partial block, replicate padding; at 16 half a tile is empty
    "b": ("cog", 600, 64, 3, False),     # odd nb, a partial K tile, several heads, force_tail = 2
    "c": ("wan", 1100, 128, 2, False),   # the D = 128 tile; nb odd and above 8
    "d": ("wan", 41000, 128, 1, True),   # nb = 321: the long entry
    "e": ("cog", 1000, 64, 3, False),    # the shape of the existing 1000-token test
}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _ops():
    from vblade import ops
    return ops


def psnr(x, ref):
    mse = torch.mean((x.double() - ref.double()) ** 2).item()
    peak = ref.double().abs().max().item()
    return 99.0 if mse == 0 else 10 * math.log10(peak * peak / mse)


def _exact_inputs(B, H, L, D, seed):
    """bf16 values with few mantissa bits (multiples of 1/4 in [-1, 1], exact in fp16 too): every
    fp32 partial dot product is exact, so GPU and CPU pooled scores agree to the bit regardless of
    summation order. As tests/test_gpu_forward.py."""
    g = torch.Generator().manual_seed(seed)
    cent = torch.randint(-2, 3, (B, H, L // 64 + 1, D), generator=g).repeat_interleave(64, 2)[:, :, :L]
    x = torch.randint(-2, 3, (B, H, L, D), generator=g) + cent
    return (x.float() / 4).to(torch.bfloat16)


def _offsets(B, H, keep, g):
    qo = torch.topk(torch.rand(B, H, 1, 128, generator=g), keep, dim=3).indices[:, :, 0]
    ko = torch.topk(torch.rand(B, H, 1, 128, generator=g), keep, dim=3).indices[:, :, 0]
    return qo, ko


def _pooled_scores_chunked(qs, ks, sm_scale, keep, dtype, qblocks=32):
    """O.pooled_scores evaluated `qblocks` q-blocks at a time (a q-block's row of Po depends on its
    own sampled rows and all keys only), so that the fp32 score matrix of a long case stays small.
    The per-chunk statements are the oracle's; the short cases check the two against each other."""
    B, H, Ls, D = qs.shape
    n = Ls // keep
    qk_scale = float(O.np.float32(sm_scale) * O.np.float32(O.LOG2E))
    out = []
    for i0 in range(0, n, qblocks):
        qc = qs[:, :, i0 * keep:(i0 + qblocks) * keep]
        nq = qc.shape[2] // keep
        S = torch.matmul(qc.float(), ks.float().transpose(-1, -2))
        rowblk = S.reshape(B, H, nq * keep, n, keep).amax(-1) * O.np.float32(qk_scale)
        m = rowblk.amax(-1, keepdim=True)
        R = O.rnd(rowblk, dtype)
        w = torch.exp2(R - m)
        po = O.rnd(w.reshape(B, H, nq, keep, n).amax(3), dtype)
        tot = O.rnd(po.sum(-1, keepdim=True), dtype)
        out.append(O.rnd(po / tot, dtype))
    return torch.cat(out, 2)


def _case_setup(case, keep, dtype=torch.bfloat16):
    from vblade.attention import retain_counts
    variant, L, D, H, long_rows = CASES[case]
    B = 1
    q = _exact_inputs(B, H, L, D, 1).to(dtype)
    k = _exact_inputs(B, H, L, D, 2).to(dtype)
    g = torch.Generator().manual_seed(7)
    qo, ko = _offsets(B, H, keep, g)
    nb = (L + 127) // 128
    mn, mx = (0.05, 0.1) if variant == "cog" else (0.05, 0.17)
    lo, hi = retain_counts(nb, mn, mx, variant)
    ft = 2 if variant == "cog" else 0
    perm = torch.randperm(L, generator=g)
    return dict(q=q, k=k, qo=qo, ko=ko, nb=nb, lo=lo, hi=hi, ft=ft, perm=perm, long_rows=long_rows,
                B=B, H=H, L=L, D=D)


# ------------------------------------------------------------------------- 1. scores and mask
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case,dtype", [("a", torch.bfloat16), ("b", torch.bfloat16), ("c", torch.bfloat16),
                                        ("d", torch.bfloat16), ("e", torch.bfloat16), ("e", torch.float16)])
def test_mask_predict_matches_oracle_at_density(case, dtype, keep):
    s = _case_setup(case, keep, dtype)
    q, k, qo, ko, perm, D = s["q"], s["k"], s["qo"], s["ko"], s["perm"], s["D"]
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    po, mask = _ops().mask_predict(q.to(DEV), k.to(DEV), qo.int().to(DEV), ko.int().to(DEV),
                                   rows=perm.int().to(DEV), min_keep=s["lo"], max_keep=s["hi"],
                                   force_tail=s["ft"], mask_count=cnt, long_rows=s["long_rows"])
    qr, kr = q[:, :, perm], k[:, :, perm]
    qs = O.sample_tokens(O.pad_replicate(qr, 128), qo)
    ks = O.sample_tokens(O.pad_replicate(kr, 128), ko)
    assert qs.shape[2] == s["nb"] * keep
    if s["nb"] > 64:
        ref_po = _pooled_scores_chunked(qs, ks, 1.0 / D ** 0.5, keep, dtype)
    else:
        ref_po = O.pooled_scores(qs, ks, 1.0 / D ** 0.5, keep, dtype)
        assert torch.equal(_pooled_scores_chunked(qs, ks, 1.0 / D ** 0.5, keep, dtype, qblocks=3), ref_po)
    po_c = po.float().cpu()
    exact = (po_c == ref_po).float().mean().item()
    print(f"case {case} keep {keep} {dtype}: exact share {exact:.6f}, "
          f"max|diff| {(po_c - ref_po).abs().max().item():.3e}")
    assert exact >= 0.999, exact
    assert (po_c - ref_po).abs().max().item() <= 2 ** -7
    # the energy rule applied by the oracle to the GPU's own scores reproduces the GPU mask exactly
    ref_mask = O.energy_mask(po_c, s["lo"], s["hi"], 0.95, s["ft"], dtype)
    assert torch.equal(mask.bool().cpu(), ref_mask)
    assert cnt.item() == int(ref_mask.sum())


# (D, dtype, keep, rule): the score-kernel instantiations (16 of vb_mask_predict / _long, 12 of
# vb_mask_predict_rule) that no other GPU test launches; rule=False cases go through the long entry
_OTHERWISE_UNLAUNCHED = [
    (64, torch.float16, 32, False), (128, torch.float16, 32, False),
    (128, torch.float16, 16, False), (128, torch.float16, 64, False),
    (64, torch.float16, 16, True), (64, torch.float16, 32, True), (64, torch.float16, 64, True),
    (128, torch.bfloat16, 16, True), (128, torch.bfloat16, 64, True),
    (128, torch.float16, 16, True), (128, torch.float16, 64, True),
]


@pytest.mark.parametrize("D,dtype,keep,rule", _OTHERWISE_UNLAUNCHED)
def test_remaining_score_kernel_instantiations(D, dtype, keep, rule):
    """B=1, H=2, L=300: three blocks (an odd count), the last one partial. Scores and mask bit for bit
    against the oracle; at density 32 also against the short entry's call."""
    ops = _ops()
    B, H, L = 1, 2, 300
    q = _exact_inputs(B, H, L, D, 1).to(dtype)
    k = _exact_inputs(B, H, L, D, 2).to(dtype)
    g = torch.Generator().manual_seed(7)
    qo, ko = _offsets(B, H, keep, g)
    perm = torch.randperm(L, generator=g)
    lo, hi, ft = 1, 2, 1
    kw = dict(rows=perm.int().to(DEV), min_keep=lo, max_keep=hi, force_tail=ft)
    args = (q.to(DEV), k.to(DEV), qo.int().to(DEV), ko.int().to(DEV))
    if rule:   # the energy rule's scalars given through a rule: the rule instantiation
        po, mask = ops.mask_predict(*args, rule=ops.MaskRule(), **kw)
    else:
        po, mask = ops.mask_predict(*args, long_rows=True, **kw)
    qs = O.sample_tokens(O.pad_replicate(q[:, :, perm], 128), qo)
    ks = O.sample_tokens(O.pad_replicate(k[:, :, perm], 128), ko)
    ref_po = O.pooled_scores(qs, ks, 1.0 / D ** 0.5, keep, dtype)
    po_c = po.float().cpu()
    print(f"D {D} {dtype} keep {keep} rule {rule}: exact share {(po_c == ref_po).float().mean().item():.6f}")
    assert torch.equal(po_c, ref_po)
    assert torch.equal(mask.bool().cpu(), O.energy_mask(po_c, lo, hi, 0.95, ft, dtype))
    if keep == 32:
        po_s, mask_s = ops.mask_predict(*args, **kw)
        assert torch.equal(po, po_s) and torch.equal(mask, mask_s)


# ------------------------------------------------------------------------- 2. in-launch offsets
def _case_b_gpu(keep, seed=11):
    variant, L, D, H, _ = CASES["b"]
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(1, H, L, D, generator=g).to(torch.bfloat16).to(DEV)
    k = torch.randn(1, H, L, D, generator=g).to(torch.bfloat16).to(DEV)
    v = torch.randn(1, H, L, D, generator=g).to(torch.bfloat16).to(DEV)
    rows = torch.randperm(L, generator=g).int().to(DEV)
    return q, k, v, rows, (1, H, L, D)


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("how", ["rand", "philox"])
def test_offsets_drawn_in_the_sampling_launch_equal_torch_topk(how, keep):
    """With rand= and with philox= the launch ranks topk(keep) of the 128 uniforms per (b,h) (q
    first, then k): scores and mask equal those of the same launch given
    torch.topk(torch.rand(B,H,1,128), keep) offsets, and the device generator ends advanced by 8."""
    ops = _ops()
    q, k, _, rows, (B, H, L, D) = _case_b_gpu(keep)
    kw = dict(rows=rows, energy_threshold=0.9, min_keep=1, max_keep=3, force_tail=2)
    torch.manual_seed(41)
    torch.rand(17, device=DEV)
    rq = torch.rand(B, H, 1, 128, device=DEV)
    rk = torch.rand(B, H, 1, 128, device=DEV)
    after_ref = torch.rand(7, device=DEV)
    q_off = torch.topk(rq, keep, dim=3).indices[:, :, 0].to(torch.int32)
    k_off = torch.topk(rk, keep, dim=3).indices[:, :, 0].to(torch.int32)
    po_ref, mask_ref = ops.mask_predict(q, k, q_off, k_off, **kw)
    if how == "rand":
        po, mask = ops.mask_predict(q, k, rand=(rq, rk), num_keep=keep, **kw)
    else:
        torch.manual_seed(41)
        torch.rand(17, device=DEV)
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        off0 = gen.get_offset()
        philox = ops.claim_rand_draws(DEV, B * H * 128)
        assert philox is not None
        po, mask = ops.mask_predict(q, k, philox=philox, num_keep=keep, **kw)
        assert gen.get_offset() == off0 + 8
        assert torch.equal(torch.rand(7, device=DEV), after_ref)
    assert torch.equal(po, po_ref) and torch.equal(mask, mask_ref)


# ------------------------------------------------------------------------- 3. fused passes
@pytest.mark.parametrize("keep,kind", [(16, "pool"), (16, "pyr"), (64, "pool")])
def test_fused_pool_and_pyramid_passes_at_density(keep, kind):
    """The pooled K/V pass and the KV pyramid pass riding in the score kernel's launch write the
    bits of the stand-alone ops.pool_kv / ops.kv_pyramid, and leave scores and mask unchanged."""
    ops = _ops()
    q, k, v, rows, (B, H, L, D) = _case_b_gpu(keep, seed=12)
    g = torch.Generator(device=DEV).manual_seed(5)
    rq = torch.rand(B, H, 1, 128, device=DEV, generator=g)
    rk = torch.rand(B, H, 1, 128, device=DEV, generator=g)
    kw = dict(rows=rows, min_keep=1, max_keep=3, force_tail=2, rand=(rq, rk), num_keep=keep)
    po_r, mask_r = ops.mask_predict(q, k, **kw)
    if kind == "pool":
        for copies in (True, False):
            outs = ops.pool_kv_outputs(k, 15, reordered=copies)
            po_p, mask_p = ops.mask_predict(q, k, pool=(v, 15, outs), **kw)
            ref = ops.pool_kv(k, v, 15, rows, reordered=copies)
            torch.cuda.synchronize()
            assert torch.equal(po_p, po_r) and torch.equal(mask_p, mask_r)
            assert len(outs) == len(ref) == (4 if copies else 2)
            for a, b in zip(outs, ref):
                assert torch.equal(a, b)
    else:
        outs = ops.kv_pyramid_outputs(k)
        po_p, mask_p = ops.mask_predict(q, k, pyr=(v, outs), **kw)
        ref = ops.kv_pyramid(k, v, rows)
        torch.cuda.synchronize()
        assert torch.equal(po_p, po_r) and torch.equal(mask_p, mask_r)
        for a, b in zip(outs, ref):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------- 4. epilogue options
@pytest.mark.parametrize("keep", KEEPS)
def test_epilogue_options_at_density(keep):
    ops = _ops()
    q, k, _, rows, (B, H, L, D) = _case_b_gpu(keep, seed=13)
    q, k = q * 0.05, k * 0.05          # low-entropy scores: many exactly tied bf16 values
    nb = (L + 127) // 128
    g = torch.Generator(device=DEV).manual_seed(6)
    rq = torch.rand(B, H, 1, 128, device=DEV, generator=g)
    rk = torch.rand(B, H, 1, 128, device=DEV, generator=g)
    kept = torch.full((B, H, nb), -1, device=DEV, dtype=torch.int32)
    po, mask = ops.mask_predict(q, k, rows=rows, min_keep=1, max_keep=3, force_tail=2, rand=(rq, rk),
                                num_keep=keep, rows_kept=kept)
    assert torch.equal(kept.long(), mask.long().sum(-1))
    po2, none = ops.mask_predict(q, k, rows=rows, want_mask=False, rand=(rq, rk), num_keep=keep)
    assert none is None and torch.equal(po2, po)
    for r in (None, {8: (0.0, 0.3), 2: (0.2, 0.6), 0: (0.6, 1.0)}):
        po3, lmask = ops.mask_predict(q, k, rows=rows, rand=(rq, rk), num_keep=keep,
                                      level=ops.ML_MASK_RATIOS if r is None else r)
        assert torch.equal(po3, po)
        assert torch.equal(lmask, ops.level_mask(po3, r))
        assert torch.equal(lmask.cpu().to(torch.int32), ML.level_mask(po3.cpu(), r))


# ------------------------------------------------------------------------- 5. modules end to end
def _clustered_qkv(B, H, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    cent = torch.randn(B, H, L // 16 + 1, D, generator=g).repeat_interleave(16, 2)[:, :, :L]
    q = (torch.randn(B, H, L, D, generator=g) + 1.5 * cent).bfloat16()
    k = (torch.randn(B, H, L, D, generator=g) + 1.5 * cent).bfloat16()
    v = torch.randn(B, H, L, D, generator=g).bfloat16()
    return q, k, v, g


@pytest.mark.parametrize("keep", KEEPS)
def test_adaptive_module_end_to_end_at_density(keep):
    """AdaptiveBlockSparseAttn(num_keep=keep) with given offsets (L = 226, two blocks): the mask obeys
    the retain counts, and the oracle's adaptive path with AdaptiveConfig(num_keep=keep) on the
    module's own mask agrees to PSNR >= 40 dB (the criterion of
    test_gpu_module.test_patched_processor_end_to_end_through_hip_module)."""
    import vblade
    from vblade.attention import retain_counts
    geo = dict(width=8, height=6, depth=4, text_length=34)
    m = vblade.AdaptiveBlockSparseAttn("cog", num_keep=keep, log_every=0, **geo)
    B, H, L, D = 1, 2, m.gilbert_rearranger.seq_len, 64
    assert L == 226 and m.num_keep == keep
    q, k, v, g = _clustered_qkv(B, H, L, D, 60 + keep)
    qo, ko = _offsets(B, H, keep, g)
    with torch.no_grad():
        out = m(q.to(DEV), k.to(DEV), v.to(DEV), q_off=qo.int().to(DEV), k_off=ko.int().to(DEV))
    mask = m.last_mask.bool().cpu()
    assert mask.shape == (B, H, 2, 2)
    assert mask.all()                         # force_tail = 2 forces both block rows
    cfg = O.AdaptiveConfig.cogvideox(num_keep=keep, **geo)
    ref = O.adaptive_attention(q, k, v, cfg, qo, ko, mask=mask, store_dtype=torch.bfloat16)
    assert psnr(out.float().cpu(), ref["out"]) >= 40
    # the predictor itself through the module, without the forced tail: its mask is the energy rule
    # on its own scores, and the oracle's prediction from the same offsets is the same mask
    m2 = vblade.AdaptiveBlockSparseAttn("wan", num_keep=keep, log_every=0, width=8, height=6, depth=10,
                                        min_retain_ratio=0.3, max_retain_ratio=0.6)
    L2 = m2.gilbert_rearranger.seq_len       # 480: four blocks, the last partial
    q2, k2 = _exact_inputs(B, H, L2, D, 3), _exact_inputs(B, H, L2, D, 4)
    with torch.no_grad():
        po, pm = m2.predict_mask(q2.to(DEV), k2.to(DEV), qo.int().to(DEV), ko.int().to(DEV))
    lo, hi = retain_counts(4, 0.3, 0.6, "wan")
    assert torch.equal(pm.bool().cpu(), O.energy_mask(po.float().cpu(), lo, hi, 0.95, 0))
    rows = m2.gilbert_rearranger.rows.long().cpu()
    cfg2 = O.AdaptiveConfig.wan(num_keep=keep, width=8, height=6, depth=10, min_retain_ratio=0.3,
                                max_retain_ratio=0.6)
    ref_po, _ = O.predict_mask(q2[:, :, rows], k2[:, :, rows], cfg2, qo, ko)
    assert (po.float().cpu() == ref_po).float().mean().item() >= 0.999
    with pytest.raises(ValueError, match="wide"):
        m(q.to(DEV), k.to(DEV), v.to(DEV), q_off=torch.zeros(B, H, 32, dtype=torch.int32, device=DEV),
          k_off=torch.zeros(B, H, 32, dtype=torch.int32, device=DEV))


@pytest.mark.parametrize("keep", KEEPS)
def test_multilevel_module_end_to_end_at_density(keep):
    """vblade.multilevel's module with num_keep=keep against oracle/ml_oracle.py (which takes the
    density from the offsets' width), in the form of
    test_gpu_multilevel.test_sampler_module_with_gilbert_reorder_matches_oracle."""
    from vblade import multilevel
    w, h, d, text = 14, 10, 6, 26
    L = w * h * d + text
    B, H, D = 1, 2, 64
    q, k, v, g = _clustered_qkv(B, H, L, D, 50 + keep)
    mod = multilevel.AdaptiveBlockSparseAttnTrain(width=w, height=h, depth=d, text_length=text,
                                                  num_keep=keep).to(DEV)
    qo, ko = _offsets(B, H, keep, g)
    out = mod(q.to(DEV), k.to(DEV), v.to(DEV), q_off=qo.int().to(DEV), k_off=ko.int().to(DEV))
    rows = mod.gilbert_rearranger.rows.long().cpu()
    r = ML.adaptive_multilevel_attention(q[:, :, rows], k[:, :, rows], v[:, :, rows], qo.long(), ko.long())
    mask = mod.last_mask.cpu().to(torch.int32)
    assert ML.level_mask_is_valid(mask, r["po"])
    ref = ML.multilevel_attention(q[:, :, rows], k[:, :, rows], v[:, :, rows], mask)["out"]
    want = torch.empty_like(ref)
    want[:, :, rows] = ref
    assert (out.float().cpu() - want).abs().max() <= 2.5e-2


# ------------------------------------------------------------------------- 6. refusals
def _raw_args(q, k, q_off, k_off, po, mask, keep):
    from vblade import _lib
    B, H, L, D = q.shape
    a = _lib.PredictArgs()
    a.q, a.k = q.data_ptr(), k.data_ptr()
    a.q_stride = a.k_stride = (H * L * D, L * D, D)
    a.q_off, a.k_off = q_off.data_ptr(), k_off.data_ptr()
    a.B, a.H, a.L, a.D, a.block, a.num_keep = B, H, L, D, 128, keep
    a.energy_threshold, a.min_keep, a.max_keep = 0.95, 1, 2
    a.po, a.mask = po.data_ptr(), mask.data_ptr()
    a.dtype = _lib.VB_DTYPE_BF16
    return a


@pytest.mark.parametrize("keep", [8, 24, 128])
def test_other_densities_are_refused_before_any_launch(keep):
    from vblade import _lib, ops
    lib = _lib.load()
    B, H, L, D = 1, 2, 600, 64
    q = torch.zeros(B, H, L, D, dtype=torch.bfloat16, device=DEV)
    off = torch.zeros(B, H, keep, dtype=torch.int32, device=DEV)
    po = torch.full((B, H, 5, 5), 7.0, dtype=torch.bfloat16, device=DEV)
    mask = torch.full((B, H, 5, 5), 9, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    a = _raw_args(q, q, off, off, po, mask, keep)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    for entry in (lib.vb_mask_predict, lib.vb_mask_predict_long):
        assert entry(ctypes.byref(a), None) == _lib.VB_ERR_UNSUPPORTED
        assert b"16, 32 or 64" in lib.vb_last_error()
    torch.cuda.synchronize()
    assert bool((po == 7.0).all()) and bool((mask == 9).all())
    # through ops: the error carries the code, and the claimed Philox draws go back to the generator
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    off0 = gen.get_offset()
    philox = ops.claim_rand_draws(DEV, B * H * 128)
    assert philox is not None and gen.get_offset() == off0 + 8
    with pytest.raises(_lib.VBladeError) as e:
        ops.mask_predict(q, q, philox=philox, num_keep=keep)
    assert e.value.code == _lib.VB_ERR_UNSUPPORTED
    assert gen.get_offset() == off0


@pytest.mark.parametrize("keep", KEEPS)
def test_short_workspace_and_row_limit_at_density(keep):
    from vblade import _lib
    lib = _lib.load()
    B, H, L, D = 1, 2, 600, 64
    q = torch.zeros(B, H, L, D, dtype=torch.bfloat16, device=DEV)
    off = torch.zeros(B, H, keep, dtype=torch.int32, device=DEV)
    po = torch.full((B, H, 5, 5), 7.0, dtype=torch.bfloat16, device=DEV)
    mask = torch.full((B, H, 5, 5), 9, dtype=torch.uint8, device=DEV)
    a = _raw_args(q, q, off, off, po, mask, keep)
    need = int(lib.vb_mask_predict_workspace_size(ctypes.byref(a)))
    assert need == B * H * (5 * keep * 4 + 5 * 5 * keep * 2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert lib.vb_mask_predict(ctypes.byref(a), None) == _lib.VB_ERR_INVALID
    assert b"workspace" in lib.vb_last_error()
    torch.cuda.synchronize()
    assert bool((po == 7.0).all()) and bool((mask == 9).all())
    if keep == 16:   # the short entry keeps its 320-block limit at the new densities
        Lbig = 321 * 128
        qb = torch.zeros(1, 1, Lbig, D, dtype=torch.bfloat16, device=DEV)
        o16 = torch.arange(16, dtype=torch.int32, device=DEV).view(1, 1, 16)
        with pytest.raises(RuntimeError, match="too long"):
            _ops().mask_predict(qb, qb, o16, o16, min_keep=1, max_keep=4)
