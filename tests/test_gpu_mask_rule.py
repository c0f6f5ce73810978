"""GPU: the whole mask rule (vb_mask_rule: top-k mode, per-head energy bounds) — alone on given
scores (vb_block_mask_rule) against the reference fixture and the numpy restatement, fused into the
predictor's epilogue (vb_mask_predict_rule) against the stand-alone entry, and through the module."""
import os

import numpy as np
import pytest
import torch

import rule_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORCE_TAIL = {"cog": 2, "wan": 0}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "mask_rule.npz"))


def _ops():
    from vblade import ops
    return ops


def _cases(kind):
    z = np.load(os.path.join(GOLDEN, "mask_rule.npz"))
    return sorted("_".join(k.split("_")[:-1]) for k in z.files if k.split("_")[0] == kind and k.endswith("_po"))


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _rule_on(po_np, dt, rule, force_tail, **kw):
    """ops.block_mask_rule on float32 scores (exact in dt) -> (mask bool numpy, rows_kept, count)."""
    ops = _ops()
    B, H, nr, _ = po_np.shape
    kept = torch.full((B, H, nr), -1, device=DEV, dtype=torch.int32)
    count = torch.zeros(1, device=DEV, dtype=torch.int64)
    mask = ops.block_mask_rule(R.to_torch(po_np, dt).to(DEV), rule, force_tail=force_tail,
                               rows_kept=kept, mask_count=count, **kw)
    return mask.bool().cpu().numpy(), kept.cpu().numpy(), int(count.item())


# ------------------------------------------------------------------ 1. fixture replay
@pytest.mark.parametrize("tag", _cases("topk"))
def test_topk_fixture_replay_is_bit_equal_to_the_reference(fixture, tag):
    ops = _ops()
    _, dt, nb, k0 = tag.split("_")
    po = R.from_bits(fixture[tag + "_po"], dt)
    for variant, ft in FORCE_TAIL.items():
        mask, kept, count = _rule_on(po, dt, ops.MaskRule(mode="topk", init_k=int(k0)), ft)
        assert np.array_equal(mask, fixture[f"{tag}_mask_{variant}"]), (tag, variant)
        assert np.array_equal(kept, mask.sum(-1)) and count == int(mask.sum())


@pytest.mark.parametrize("tag", _cases("topkties"))
def test_topk_fixture_replay_on_tie_heavy_rows(fixture, tag):
    ops = _ops()
    _, dt, nb, k0 = tag.split("_")
    po = R.from_bits(fixture[tag + "_po"], dt)
    kk = R.topk_counts(po, int(k0), dt)
    for variant, ft in FORCE_TAIL.items():
        mask, kept, count = _rule_on(po, dt, ops.MaskRule(mode="topk", init_k=int(k0)), ft)
        assert np.array_equal(mask, R.mask_from_counts(po, kk, ft)), variant   # lower column first
        assert R.mask_is_valid_selection(mask, po, kk, ft)
        ref = fixture[f"{tag}_mask_{variant}"]
        assert R.mask_is_valid_selection(ref, po, kk, ft)
        if ft == 0:   # with forced columns the sums depend on which members of a tie were chosen
            assert np.array_equal(mask.sum(-1), ref.sum(-1))
        assert np.array_equal(kept, mask.sum(-1)) and count == int(mask.sum())


@pytest.mark.parametrize("tag", _cases("energy"))
def test_per_head_energy_fixture_replay(fixture, tag):
    from vblade.attention import retain_counts
    ops = _ops()
    _, dt, nb = tag.split("_")
    nb = int(nb)
    po = R.from_bits(fixture[tag + "_po"], dt)
    mn, mx = fixture[tag + "_min_ratio"], fixture[tag + "_max_ratio"]
    lo, hi = np.zeros(mn.shape, np.int64), np.zeros(mn.shape, np.int64)
    for b, h in np.ndindex(*mn.shape):
        lo[b, h], hi[b, h] = retain_counts(nb, float(mn[b, h]), float(mx[b, h]), "cog")
    kk = R.energy_counts(po, lo, hi, 0.95, dt)
    rule = ops.MaskRule(mode="energy", min_keep=_i32(lo), max_keep=_i32(hi))
    for ft in (0, 2):
        mask, kept, count = _rule_on(po, dt, rule, ft, energy_threshold=0.95)
        assert np.array_equal(mask, R.mask_from_counts(po, kk, ft))
        assert np.array_equal(kept, mask.sum(-1)) and count == int(mask.sum())
    ref = fixture[tag + "_mask_cog"]   # the reference's forced tail is 2
    assert R.mask_is_valid_selection(ref, po, kk, 2)


# ------------------------------------------------------------------ 2. row widths
def _tie_heavy(B, H, nr, nc, seed, dt):
    g = torch.Generator().manual_seed(seed)
    po = torch.rand(B, H, nr, nc, generator=g) ** 4
    ties = (torch.rand(B, H, nr, nc, generator=g) < 0.15).float()
    po = torch.where(torch.rand(B, H, nr, 1, generator=g) < 0.5, po, torch.maximum(po, ties))
    tdt = R.DTYPES[dt]
    po = po.to(tdt)
    po = (po.float() / po.float().sum(-1, keepdim=True).to(tdt).float()).to(tdt)
    return po.float().numpy()


WIDTHS = [1, 2, 63, 64, 65, 128, 129, 320, 321, 1024]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("nc", WIDTHS)
def test_rule_at_the_row_width_edges(nc, dt):
    """nr = 4 rows of nc columns, B = 2, H = 3, tie-heavy scores: top-k with init_k per head spread
    over [1, nc], and the energy rule with per-head bounds, both bit-equal to the restatement."""
    ops = _ops()
    B, H, nr = 2, 3, 4
    po = _tie_heavy(B, H, nr, nc, nc, dt)
    k0 = np.unique(np.linspace(1, nc, B * H).round().astype(np.int64))
    k0 = np.resize(k0, B * H).reshape(B, H)
    assert k0.min() == 1 and k0.max() == nc
    for ft in (0, 2):
        kk = R.topk_counts(po, k0, dt)
        mask, kept, count = _rule_on(po, dt, ops.MaskRule(mode="topk", init_k=_i32(k0)), ft)
        assert np.array_equal(mask, R.mask_from_counts(po, kk, ft)), (nc, ft)
        assert np.array_equal(kept, mask.sum(-1)) and count == int(mask.sum())
    # a scalar k0 below nr lets the two updates run on these short columns of rows
    for ks in {1, min(2, nc), min(3, nc)}:
        kk = R.topk_counts(po, ks, dt)
        mask, kept, _ = _rule_on(po, dt, ops.MaskRule(mode="topk", init_k=ks), 0)
        assert np.array_equal(mask, R.mask_from_counts(po, kk, 0)) and np.array_equal(kept, kk)
    lo = np.resize(np.array([1, 2, 5, 1, 40, 3]), B * H).reshape(B, H)
    hi = np.clip(k0[::-1, ::-1] + 1, 1, None)
    thr = np.linspace(0.5, 0.99, B * H).astype(np.float32).reshape(B, H)
    kk = R.energy_counts(po, lo, hi, thr, dt)
    rule = ops.MaskRule(mode="energy", min_keep=_i32(lo), max_keep=_i32(hi),
                        energy_threshold=torch.from_numpy(thr).to(DEV))
    mask, kept, count = _rule_on(po, dt, rule, 2)
    assert np.array_equal(mask, R.mask_from_counts(po, kk, 2))
    assert np.array_equal(kept, mask.sum(-1)) and count == int(mask.sum())


# ------------------------------------------------------------------ 3. per-head energy
def test_per_head_energy_equals_the_scalar_rule_head_by_head():
    ops = _ops()
    B, H, nb = 2, 3, 67
    po = R.to_torch(_tie_heavy(B, H, nb, nb, 5, "bf16"), "bf16").to(DEV)
    lo = torch.tensor([[1, 4, 2], [7, 1, 3]], dtype=torch.int32)
    hi = torch.tensor([[6, 30, 2], [40, 9, 67]], dtype=torch.int32)
    thr = torch.tensor([[0.95, 0.5, 0.99], [0.8, 0.9, 0.7]], dtype=torch.float32)
    rule = ops.MaskRule(mode="energy", min_keep=lo.to(DEV), max_keep=hi.to(DEV), energy_threshold=thr.to(DEV))
    got = ops.block_mask_rule(po, rule, force_tail=2)
    assert len({got[b, h].sum().item() for b in range(B) for h in range(H)}) > 1
    for b in range(B):
        for h in range(H):
            want = ops.energy_mask(po[b:b + 1, h:h + 1], energy_threshold=float(thr[b, h]),
                                   min_keep=int(lo[b, h]), max_keep=int(hi[b, h]), force_tail=2)
            assert torch.equal(got[b:b + 1, h:h + 1], want), (b, h)
    # uniform arrays, and a rule that leaves everything to the scalars: the scalar call's bits
    want = ops.energy_mask(po, energy_threshold=0.9, min_keep=3, max_keep=11, force_tail=2)
    ones = torch.ones(B, H, device=DEV)
    uni = ops.MaskRule(mode="energy", min_keep=(3 * ones).int(), max_keep=(11 * ones).int(),
                       energy_threshold=0.9 * ones)
    assert torch.equal(ops.block_mask_rule(po, uni, force_tail=2), want)
    assert torch.equal(ops.block_mask_rule(po, uni, force_tail=2, energy_threshold=0.1, min_keep=50,
                                           max_keep=60), want)
    assert torch.equal(ops.block_mask_rule(po, ops.MaskRule(), energy_threshold=0.9, min_keep=3,
                                           max_keep=11, force_tail=2), want)
    assert torch.equal(ops.block_mask_rule(po, None, energy_threshold=0.9, min_keep=3, max_keep=11,
                                           force_tail=2), want)
    assert torch.equal(ops.block_mask_rule(po, {"mode": "energy", "max_keep": 11, "min_keep": 3},
                                           energy_threshold=0.9, force_tail=2), want)


# ------------------------------------------------------------------ 4. clamping
@pytest.mark.parametrize("nc", [5, 67, 321])
def test_device_array_values_are_clamped_to_the_row(nc):
    ops = _ops()
    B, H, nr = 2, 3, 4
    po_np = _tie_heavy(B, H, nr, nc, 100 + nc, "bf16")
    po = R.to_torch(po_np, "bf16").to(DEV)
    raw = np.array([[0, -5, nc + 7], [1, nc, 2 ** 31 - 1]], dtype=np.int64)
    clamped = np.clip(raw, 1, nc)
    for ft in (0, 2):
        got = ops.block_mask_rule(po, ops.MaskRule(mode="topk", init_k=_i32(raw)), force_tail=ft)
        want = ops.block_mask_rule(po, ops.MaskRule(mode="topk", init_k=_i32(clamped)), force_tail=ft)
        assert torch.equal(got, want)
        assert np.array_equal(got.bool().cpu().numpy(),
                              R.mask_from_counts(po_np, R.topk_counts(po_np, clamped, "bf16"), ft))
        for name in ("min_keep", "max_keep"):
            other = {"min_keep": "max_keep", "max_keep": "min_keep"}[name]
            base = {other: _i32(np.full((B, H), 3 if name == "max_keep" else nc))}
            got = ops.block_mask_rule(po, ops.MaskRule(mode="energy", **{name: _i32(raw)}, **base), force_tail=ft)
            want = ops.block_mask_rule(po, ops.MaskRule(mode="energy", **{name: _i32(clamped)}, **base), force_tail=ft)
            assert torch.equal(got, want), name


# ------------------------------------------------------------------ 5. the fused path
def _qk(B, H, L, D, seed, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    nb = (L + 127) // 128
    cent = torch.randn(B, H, nb, D, generator=g).repeat_interleave(128, 2)[:, :, :L] * 1.2
    q = (torch.randn(B, H, L, D, generator=g) + cent).to(dtype).to(DEV)
    k = (torch.randn(B, H, L, D, generator=g) + cent).to(dtype).to(DEV)
    v = torch.randn(B, H, L, D, generator=g).to(dtype).to(DEV)
    return q, k, v


def _offsets(B, H, keep, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 128, (B, H, keep), generator=g, dtype=torch.int32).to(DEV),
            torch.randint(0, 128, (B, H, keep), generator=g, dtype=torch.int32).to(DEV))


def _rules(ops, B, H, nb):
    g = torch.Generator().manual_seed(nb)
    k0 = torch.randint(1, max(2, nb // 3 + 1), (B, H), generator=g, dtype=torch.int32)
    lo = torch.randint(1, max(2, nb // 10 + 1), (B, H), generator=g, dtype=torch.int32)
    hi = lo + torch.randint(0, max(1, nb // 2), (B, H), generator=g, dtype=torch.int32)
    thr = 0.6 + 0.39 * torch.rand(B, H, generator=g)
    return {"topk": ops.MaskRule(mode="topk", init_k=k0.to(DEV)),
            "topk_scalar": ops.MaskRule(mode="topk", init_k=max(1, nb // 5)),
            "energy": ops.MaskRule(mode="energy", min_keep=lo.to(DEV), max_keep=hi.to(DEV),
                                   energy_threshold=thr.to(DEV))}


def _check_fused(q, k, v, qo, ko, rule, *, rows=None, pool_gap=None, force_tail=2):
    ops = _ops()
    B, H, L, D = q.shape
    nb = (L + 127) // 128
    kw = dict(rows=rows, force_tail=force_tail, energy_threshold=0.9, min_keep=1, max_keep=max(1, nb // 4))
    outs0 = ops.pool_kv_outputs(k, pool_gap, reordered=True) if pool_gap else None
    outs1 = ops.pool_kv_outputs(k, pool_gap, reordered=True) if pool_gap else None
    po0, _ = ops.mask_predict(q, k, qo, ko, long_rows=nb > ops.MAX_BLOCKS,
                              pool=(v, pool_gap, outs0) if pool_gap else None, **kw)
    kept = torch.full((B, H, nb), -1, device=DEV, dtype=torch.int32)
    count = torch.zeros(1, device=DEV, dtype=torch.int64)
    po1, mask = ops.mask_predict(q, k, qo, ko, rule=rule, rows_kept=kept, mask_count=count,
                                 pool=(v, pool_gap, outs1) if pool_gap else None, **kw)
    assert torch.equal(po0, po1)
    if pool_gap:
        for a, b in zip(outs0, outs1):
            assert torch.equal(a, b)
    want = ops.block_mask_rule(po1, rule, force_tail=force_tail, energy_threshold=0.9, min_keep=1,
                               max_keep=max(1, nb // 4))
    assert torch.equal(mask, want)
    assert torch.equal(kept.long(), mask.long().sum(-1)) and int(count.item()) == int(mask.sum().item())
    return po1, mask


@pytest.mark.parametrize("mode", ["topk", "topk_scalar", "energy"])
@pytest.mark.parametrize("shape", ["L100", "L640", "L41000"])
def test_fused_rule_equals_the_stand_alone_rule_on_the_same_scores(shape, mode):
    ops = _ops()
    B, H, L, D = {"L100": (1, 1, 100, 64), "L640": (2, 3, 640, 128), "L41000": (1, 1, 41000, 64)}[shape]
    q, k, v = _qk(B, H, L, D, L)
    qo, ko = _offsets(B, H, 32, L)
    rows = pool_gap = None
    if shape == "L640":   # a random row permutation, the pooled pass riding in the launch
        rows = torch.randperm(L, generator=torch.Generator().manual_seed(3)).to(torch.int32).to(DEV)
        pool_gap = 15
    nb = (L + 127) // 128
    _, mask = _check_fused(q, k, v, qo, ko, _rules(ops, B, H, nb)[mode], rows=rows, pool_gap=pool_gap)
    assert mask.shape == (B, H, nb, nb)


@pytest.mark.parametrize("mode", ["topk", "energy"])
@pytest.mark.parametrize("keep", [16, 32, 64])
def test_fused_rule_at_every_sampling_density(keep, mode):
    ops = _ops()
    B, H, L, D = 1, 2, 8500, 64
    q, k, v = _qk(B, H, L, D, keep)
    qo, ko = _offsets(B, H, keep, keep)
    _check_fused(q, k, v, qo, ko, _rules(ops, B, H, 67)[mode])


def test_fused_rule_fp16_and_no_forced_tail():
    ops = _ops()
    B, H, L, D = 2, 3, 640, 128
    q, k, v = _qk(B, H, L, D, 9, torch.float16)
    qo, ko = _offsets(B, H, 32, 9)
    for mode in ("topk", "energy"):
        _check_fused(q, k, v, qo, ko, _rules(ops, B, H, 5)[mode], force_tail=0)


def test_fused_rule_with_philox_draws():
    """The offsets are drawn inside the sampling launch from (seed, offset): the rule call draws the
    offsets of the call without a rule (its scores are the same bits), and applies its rule."""
    ops = _ops()
    B, H, L, D = 1, 2, 8500, 64
    q, k, v = _qk(B, H, L, D, 21)
    rule = _rules(ops, B, H, 67)["topk"]
    kw = dict(force_tail=2, energy_threshold=0.9, min_keep=1, max_keep=9)
    po0, _ = ops.mask_predict(q, k, philox=(1234, 40), **kw)
    po1, mask = ops.mask_predict(q, k, philox=(1234, 40), rule=rule, **kw)
    po2, _ = ops.mask_predict(q, k, philox=(1234, 48), rule=rule, **kw)
    assert torch.equal(po0, po1) and not torch.equal(po1, po2)
    assert torch.equal(mask, ops.block_mask_rule(po1, rule, force_tail=2))


def test_no_rule_call_makes_the_existing_entries_calls():
    from vblade import _lib
    ops = _ops()
    lib = _lib.load()
    B, H, L, D = 1, 2, 8500, 64
    q, k, v = _qk(B, H, L, D, 2)
    qo, ko = _offsets(B, H, 32, 2)
    kw = dict(force_tail=2, energy_threshold=0.9, min_keep=2, max_keep=9)
    po0, mask0 = ops.mask_predict(q, k, qo, ko, **kw)
    # the energy rule's scalars given through a rule: the same bits from the rule instantiation
    po1, mask1 = ops.mask_predict(q, k, qo, ko, rule=ops.MaskRule(), **kw)
    assert torch.equal(po0, po1) and torch.equal(mask0, mask1)
    # rule == NULL at the C entry
    orig = lib.vb_mask_predict
    try:
        lib.vb_mask_predict = lambda a, s: lib.vb_mask_predict_rule(a, None, s)
        po2, mask2 = ops.mask_predict(q, k, qo, ko, **kw)
    finally:
        lib.vb_mask_predict = orig
    assert torch.equal(po0, po2) and torch.equal(mask0, mask2)


# ------------------------------------------------------------------ 6. the module
def _cog(**kw):
    import vblade
    return vblade.AdaptiveBlockSparseAttn("cog", width=16, height=12, depth=5, text_length=226,
                                          log_every=0, **kw)


@pytest.fixture(scope="module")
def module_inputs():
    L = 16 * 12 * 5 + 226
    q, k, v = _qk(1, 2, L, 64, 77)
    qo, ko = _offsets(1, 2, 32, 77)
    return q, k, v, qo, ko


def test_module_topk_mode(module_inputs):
    ops = _ops()
    q, k, v, qo, ko = module_inputs
    m = _cog(mask_mode="topk", init_k=0.3)
    nb = (q.shape[2] + 127) // 128
    with torch.no_grad():
        po, _ = m.predict_mask(q, k, qo, ko)
        out = m(q, k, v, q_off=qo, k_off=ko)
        want = ops.block_mask_rule(po, ops.MaskRule(mode="topk", init_k=int(nb * 0.3)), force_tail=2)
        assert torch.equal(m.last_mask, want)
        assert 0 < int(want.sum()) < want.numel()
        ref = _cog()(q, k, v, q_off=qo, k_off=ko, block_mask=m.last_mask)
    assert torch.equal(out, ref)
    assert abs(m.sparsity - (1 - want.float().mean().item() - 1 / 15)) < 1e-6
    # init_k as a count
    m2 = _cog(mask_mode="topk", init_k=3)
    with torch.no_grad():
        m2(q, k, v, q_off=qo, k_off=ko)
    assert torch.equal(m2.last_mask, ops.block_mask_rule(po, ops.MaskRule(mode="topk", init_k=3), force_tail=2))


def test_module_per_head_ratios(module_inputs):
    q, k, v, qo, ko = module_inputs
    ratio = torch.tensor([0.3, 0.7])
    m = _cog(max_retain_ratio=ratio)
    with torch.no_grad():
        m(q, k, v, q_off=qo, k_off=ko)
        mask = m.last_mask.clone()
        for h in range(2):
            s = _cog(max_retain_ratio=float(ratio[h]))
            s(q, k, v, q_off=qo, k_off=ko)
            assert torch.equal(mask[:, h], s.last_mask[:, h]), h
        assert not torch.equal(mask[:, 0], mask[:, 1])
        # [B,H] tensors for all three options; the second call neither launches the conversion
        # again nor synchronises
        m3 = _cog(max_retain_ratio=ratio.view(1, 2).to(DEV), min_retain_ratio=torch.tensor([0.05, 0.1]),
                  energy_threshold=torch.tensor([[0.95, 0.8]]))
        out_a = m3(q, k, v, q_off=qo, k_off=ko)
        torch.cuda.synchronize()
        cached = dict(m3._per_head_cache)
        torch.cuda.set_sync_debug_mode("error")
        try:
            out_b = m3(q, k, v, q_off=qo, k_off=ko)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert all(m3._per_head_cache[key][2] is val[2] for key, val in cached.items()) and len(cached) == 3
        assert torch.equal(out_a, out_b)


def test_module_topk_mode_autograd_step(module_inputs):
    q, k, v, qo, ko = module_inputs
    grads = []
    mask = None
    for given in (False, True):
        m = _cog(mask_mode="topk", init_k=0.3) if not given else _cog()
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = m(qq, kk, vv, q_off=qo, k_off=ko, block_mask=mask)
        out.float().square().sum().backward()
        grads.append((out.detach(), qq.grad, kk.grad, vv.grad))
        mask = m.last_mask.clone()
    for a, b in zip(*grads):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


# ------------------------------------------------------------------ 7. capture
def test_topk_module_call_captures_into_a_hip_graph(module_inputs):
    ops = _ops()
    q, k, v, _, _ = module_inputs
    m = _cog(mask_mode="topk", init_k=0.3)
    B, H = q.shape[:2]
    with torch.no_grad():
        m(q, k, v)                                   # warm up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                assert ops.claim_rand_draws(DEV, B * H * 128) is None
                out = m(q, k, v)
        torch.cuda.current_stream().wait_stream(s)
        captured_mask = m.last_mask
        # the replay draws torch.rand at the generator's state: the same state, eagerly, gives the
        # draws (and so the offsets) the replay used
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        state = gen.get_state()
        graph.replay()
        torch.cuda.synchronize()
        replayed = captured_mask.clone()
        out_replayed = out.clone()
        gen.set_state(state)
        rq = torch.rand(B, H, 1, 128, device=DEV)
        rk = torch.rand(B, H, 1, 128, device=DEV)
        qo, ko = ops.sample_offsets(rq, rk, 32)
        eager = m(q, k, v, q_off=qo[:, :, 0], k_off=ko[:, :, 0])
        torch.cuda.synchronize()
        assert torch.equal(m.last_mask, replayed)
        assert torch.equal(eager, out_replayed)
        assert 0 < int(replayed.sum()) < replayed.numel()
