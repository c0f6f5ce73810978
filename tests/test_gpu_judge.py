"""GPU: vb_judge_sparsity / vb_head_budget and the module's head_budget="judge" option.

The estimator kernel is an fp32 evaluation, so against the float64 restatement (tests/judge_ref.py)
it must sit well inside the reference's own 16-bit rounding: its error is at most ONE EIGHTH of the
16-bit evaluation's error on the same inputs (fixture replay: of the reference's own ref16). The
budget rule is compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import judge_ref as J
from conftest import GOLDEN, record

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vblade import ops
    return ops


def _qk(B, H, L, D, dt, seed, temps=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, D, generator=g)
    k = torch.randn(B, H, L, D, generator=g)
    if temps is not None:
        q = q * torch.as_tensor(temps, dtype=torch.float32).view(1, H, 1, 1)
    return q.to(J.DTYPES[dt]), k.to(J.DTYPES[dt])


def _rows(L, S, seed):
    return np.sort(np.random.default_rng(seed).permutation(L)[:S]).astype(np.int32)


def _run(q, k, rows, **kw):
    s, rm = _ops().judge_sparsity(q.to(DEV), k.to(DEV), rows, want_rows=True, **kw)
    return s.cpu().numpy(), rm.cpu().numpy()


def _fp32_mean(rm):
    acc = np.zeros(rm.shape[:-1], dtype=np.float32)
    for r in range(rm.shape[-1]):
        acc = acc + rm[..., r]
    return acc / np.float32(rm.shape[-1])


def _check_eighth(tag, q, k, rows, **kw):
    """kernel vs float64 within one eighth of the 16-bit evaluation's error, for the statistic and
    for the per-row masses; sparsity is the fp32 mean of row_mass in row order."""
    s, rm = _run(q, k, rows, **kw)
    s64, rm64 = J.judge(q, k, rows, dtype=torch.float64, **kw)
    s16, rm16 = J.judge(q, k, rows, **kw)
    err, bound = np.abs(s - s64).max(), np.abs(s16 - s64).max() / 8
    err_r, bound_r = np.abs(rm - rm64).max(), np.abs(rm16 - rm64).max() / 8
    print(f"{tag}: kernel err {err:.3e} (bound {bound:.3e}); rows {err_r:.3e} (bound {bound_r:.3e})")
    assert np.isfinite(s).all() and np.isfinite(rm).all()
    assert err <= bound, (tag, err, bound)
    assert err_r <= bound_r, (tag, err_r, bound_r)
    assert np.array_equal(_fp32_mean(rm), s), tag
    return s, rm


# ------------------------------------------------------------------ 1. the reference's own results
def _golden():
    z = np.load(os.path.join(GOLDEN, "judge_sparsity.npz"))
    return z, sorted(k[:-len("_ref64")] for k in z.files if k.endswith("_ref64"))


@pytest.mark.parametrize("tag", _golden()[1])
def test_fixture_replay_sits_inside_the_reference_rounding(tag):
    z, _ = _golden()
    dt = tag.split("_")[0]
    q, k = J.from_bits(z[tag + "_q"], dt), J.from_bits(z[tag + "_k"], dt)
    s, _ = _run(q, k, z[tag + "_idx"])
    ref64 = z[tag + "_ref64"]
    err = np.abs(s - ref64).max()
    e16 = np.abs(z[tag + "_ref16"] - ref64).max()
    e32 = np.abs(z[tag + "_ref32"] - ref64).max()
    print(f"{tag}: kernel {err:.3e}, ref32 {e32:.3e}, ref16 {e16:.3e}")
    record("judge_sparsity kernel error / reference-fp32 error vs float64", (tag, float(err / e32)))
    assert err <= e16 / 8, (tag, err, e16)


# ------------------------------------------------------------------ 2. edges
# key tile 32, score workgroup chunk 512 keys (vb_judge.hip); n = ceil(L / key_stride)
EDGES = [
    # id, B, H, L, D, dtype, S, key_stride
    ("S1", 2, 3, 1000, 64, "bf16", 1, 3),
    ("S7", 2, 3, 1000, 64, "bf16", 7, 3),
    ("S30", 2, 3, 1000, 64, "bf16", 30, 3),
    ("S64", 2, 3, 1000, 64, "bf16", 64, 3),
    ("S33_D128", 2, 3, 1000, 128, "bf16", 33, 3),
    ("n_below_tile", 2, 3, 50, 64, "bf16", 30, 3),              # n = 17
    ("n_tile_multiple", 2, 3, 192, 64, "fp16", 30, 3),          # n = 64
    ("n_tile_plus_one", 2, 3, 193, 128, "bf16", 30, 3),         # n = 65
    ("n_chunk_plus_one", 2, 3, 1537, 64, "bf16", 30, 3),        # n = 513
    ("n_chunk_exact", 2, 3, 1536, 128, "fp16", 30, 3),          # n = 512
    ("tail_L_mod3_2", 2, 3, 1001, 64, "fp16", 30, 3),
    ("stride1", 2, 3, 700, 64, "bf16", 30, 1),
    ("stride5", 2, 3, 1003, 128, "fp16", 30, 5),
    ("fp16_D128", 2, 3, 1000, 128, "fp16", 30, 3),
]


@pytest.mark.parametrize("case", EDGES, ids=[c[0] for c in EDGES])
def test_edges_against_float64(case):
    tag, B, H, L, D, dt, S, ks = case
    q, k = _qk(B, H, L, D, dt, seed=len(tag) * 7 + L, temps=np.linspace(0.5, 2.5, H))
    rows = _rows(L, S, seed=L + S)
    if S > 1:
        rows[0], rows[-1] = 0, L - 1
    _check_eighth(tag, q, k, rows, key_stride=ks)


def test_one_long_row():
    L = 131067
    q, k = _qk(1, 1, L, 128, "bf16", seed=3, temps=[1.5])
    rows = _rows(L, 30, seed=4)
    rows[-1] = L - 1
    _check_eighth("long", q, k, rows)


def test_strided_views_are_read_in_place_and_bit_equal():
    ops = _ops()
    B, H, L, D = 2, 3, 1000, 64
    g = torch.Generator().manual_seed(21)
    rows = _rows(L, 30, 5)
    for dt in ("bf16", "fp16"):
        qm = torch.randn(B, L, H, D, generator=g).to(DEV, J.DTYPES[dt])
        km = torch.randn(B, L, H, D, generator=g).to(DEV, J.DTYPES[dt])
        q, k = qm.transpose(1, 2), km.transpose(1, 2)
        assert not q.is_contiguous() and ops._aligned_bhld(q) is q
        a = ops.judge_sparsity(q, k, rows, want_rows=True)
        b = ops.judge_sparsity(q.contiguous(), k.contiguous(), rows, want_rows=True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------ 3. exact and analytic cases
def test_zero_keys_give_top_n_over_n():
    """k = 0: every p = 1/n, so each row's mass is top_n/n (one correctly rounded fp32 division) and
    the mean of S equal values is off by at most S roundings of the serial sum: 64 * 2^-24 < 4e-6."""
    for L, ks in ((1000, 3), (193, 1)):
        q, _ = _qk(2, 3, L, 64, "bf16", seed=1)
        s, rm = _run(q, torch.zeros_like(q), _rows(L, 30, 2), key_stride=ks)
        n, top_n = J.top_n_of(L, ks)
        assert (rm == np.float32(top_n) / np.float32(n)).all()
        assert np.abs(s / (top_n / n) - 1).max() <= 4e-6


def test_ties_straddling_the_boundary():
    """Five distinct key rows repeated along the sequence: p takes five values, each n/5 times, and
    the top_n boundary falls inside a run of equal values."""
    B, H, L, D = 2, 3, 1000, 64
    q, kd = _qk(B, H, L, D, "bf16", seed=8, temps=[0.5, 1.0, 2.0])
    k = kd[:, :, torch.arange(L) % 5]
    n, top_n = J.top_n_of(L, 3, 0.3)
    assert 1 < top_n % (n // 5) < n // 5 - 1
    _check_eighth("ties", q, k, _rows(L, 30, 9), top=0.3)


@pytest.mark.parametrize("gap", [80, 120])
def test_one_dominating_key(gap):
    """Key 0 scores `gap` above the rest (all zero): its p is 1 in fp32 and the rest is e^-80 ~ 2e-35
    each (or underflows to 0 at e^-120), so every mass and the statistic are exactly 1."""
    B, H, L, D = 2, 3, 1000, 64
    q = torch.full((B, H, L, D), 2.0, dtype=torch.bfloat16)
    k = torch.zeros(B, H, L, D, dtype=torch.bfloat16)
    k[:, :, 0] = gap / 16.0            # 64 * 2 * gap/16 / sqrt(64) = gap
    s, rm = _run(q, k, _rows(L, 30, 3))
    assert (rm == 1.0).all() and (s == 1.0).all()


def test_large_scores_need_the_max_subtraction():
    """fp16 scores of 200 +- 1: exp(200) overflows fp32, the max-subtracted softmax does not. The
    16-bit evaluation is no yardstick here (its scores round to multiples of 0.125), so the bound
    comes from fp32: a score of magnitude <= 512 in log2 units carries up to 2^-15 of rounding, a
    relative 2.1e-5 in its e; a mass is a ratio of two sums of e, so <= 4.3e-5; the bound is 1e-4."""
    B, H, L, D = 2, 3, 1000, 64
    g = torch.Generator().manual_seed(31)
    q = torch.full((B, H, L, D), 5.0).to(torch.float16)
    k = (5.0 + 0.2 * torch.randn(B, H, L, D, generator=g)).to(torch.float16)
    rows = _rows(L, 30, 6)
    s, rm = _run(q, k, rows)
    s64, rm64 = J.judge(q, k, rows, dtype=torch.float64)
    assert np.isfinite(rm).all() and 0.3 < s64.min() and s64.max() < 0.99
    assert np.abs(rm - rm64).max() <= 1e-4 and np.abs(s - s64).max() <= 1e-4
    assert np.array_equal(_fp32_mean(rm), s)


def test_two_runs_are_bit_equal():
    ops = _ops()
    q, k = _qk(2, 3, 1537, 128, "bf16", seed=12, temps=[0.5, 1.0, 2.0])
    q, k = q.to(DEV), k.to(DEV)
    rows = torch.from_numpy(_rows(1537, 30, 1)).to(DEV)
    a = ops.judge_sparsity(q, k, rows, want_rows=True)
    b = ops.judge_sparsity(q, k, rows, want_rows=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.judge_sparsity(q, k, rows), a[0])       # row_mass = NULL: the same statistic


# ------------------------------------------------------------------ 4. the budget rule
@pytest.mark.parametrize("variant", ["cog", "wan"])
@pytest.mark.parametrize("nb", [3, 139, 256, 1024])
def test_head_budget_is_bit_equal_to_the_restatement(variant, nb):
    ops = _ops()
    g = np.random.default_rng(nb)
    for shape, base, clamp in (((2, 24), 0.1, (1e-3, 10.0)),       # no clamp binds
                               ((2, 24), 0.5, (0.45, 0.6)),        # both bind
                               ((2, 12), 0.17, (0.05, 0.9)),
                               ((1, 40), 0.1, (0.25, 0.25)),       # lo = hi
                               ((1, 1), 0.3, (0.05, 0.9))):        # B*H = 1: ratio = base
        s = g.uniform(0.2, 0.99, size=shape).astype(np.float32)
        keep, ratio = ops.head_budget(torch.from_numpy(s).to(DEV), nb, base, clamp, variant, want_ratio=True)
        want, want_ratio = J.head_budget(s, nb, base, clamp, variant)
        assert keep.dtype == torch.int32 and np.array_equal(keep.cpu().numpy(), want), (shape, base, clamp)
        assert np.array_equal(ratio.cpu().numpy(), want_ratio.astype(np.float32))
        if clamp == (0.45, 0.6):
            assert (want_ratio == 0.45).any() and (want_ratio == 0.6).any()
        assert torch.equal(ops.head_budget(torch.from_numpy(s).to(DEV), nb, base, clamp, variant), keep)


# ------------------------------------------------------------------ 5. the module
# max_retain_ratio = 0.5 in these tests: at 10-12 blocks the variants' 0.1 / 0.17 give every head one block
GRIDS = {"cog": dict(width=16, height=12, depth=6, text_length=26),     # L = 1178, 10 blocks
         "wan": dict(width=16, height=12, depth=8, text_length=0)}      # L = 1536, 12 blocks
HEAD_DIM = {"cog": 64, "wan": 128}
HEADS = 4


def _module(variant, **kw):
    import vblade
    return vblade.AdaptiveBlockSparseAttn(variant, log_every=0, **GRIDS[variant], **kw)


_INPUTS = {}


def _inputs(variant):
    if variant not in _INPUTS:
        gd = GRIDS[variant]
        L = gd["width"] * gd["height"] * gd["depth"] + gd["text_length"]
        g = torch.Generator().manual_seed(40)
        q, k = _qk(1, HEADS, L, HEAD_DIM[variant], "bf16", seed=41, temps=np.linspace(0.2, 3.0, HEADS))
        v = torch.randn(1, HEADS, L, HEAD_DIM[variant], generator=g).to(torch.bfloat16)
        from vblade import attention
        go = torch.Generator(device=DEV).manual_seed(42)
        qo, ko = attention.draw_sample_offsets_qk(1, HEADS, DEV, generator=go)
        _INPUTS[variant] = (q.to(DEV), k.to(DEV), v.to(DEV), qo.contiguous(), ko.contiguous())
    return _INPUTS[variant]


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_module_budget_and_mask(variant):
    ops = _ops()
    from vblade.attention import retain_counts
    q, k, v, qo, ko = _inputs(variant)
    m = _module(variant, head_budget="judge", max_retain_ratio=0.5)
    with torch.no_grad():
        out = m(q, k, v, q_off=qo, k_off=ko)
    nb = (q.shape[2] + 127) // 128
    sp, budget = m.last_head_sparsity, m.last_head_budget
    assert sp.dtype == torch.float32 and sp.shape == (1, HEADS) and budget.dtype == torch.int32
    want, _ = J.head_budget(sp.cpu().numpy(), nb, m.max_retain_ratio, m.judge_clamp, variant)
    assert np.array_equal(budget.cpu().numpy(), want)
    assert torch.equal(sp, ops.judge_sparsity(q, k, m.judge_rows))
    # q scaled 0.2 ... 3 per head: concentration, and so the budget, grows with the temperature
    assert (sp[0, 1:] > sp[0, :-1]).all() and len(set(want.flatten().tolist())) > 1
    lo, _ = retain_counts(nb, m.min_retain_ratio, 1.0, variant)
    _, mask = ops.mask_predict(q, k, qo, ko, rows=m._rows(q.device), energy_threshold=m.energy_threshold,
                               min_keep=lo, max_keep=nb, force_tail=m.force_tail,
                               rule=ops.MaskRule(max_keep=budget))
    assert torch.equal(m.last_mask, mask)
    with torch.no_grad():
        ref = _module(variant)(q, k, v, q_off=qo, k_off=ko, block_mask=mask)
    assert torch.equal(out, ref)
    # judge_rows overrides the probe for one call
    other = torch.arange(5, 25, dtype=torch.int32, device=DEV) + GRIDS[variant]["text_length"]
    with torch.no_grad():
        m(q, k, v, q_off=qo, k_off=ko, judge_rows=other)
    assert torch.equal(m.last_head_sparsity, ops.judge_sparsity(q, k, other))


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_module_flat_clamp_equals_uniform_per_head_ratio_and_draws_no_rng(variant):
    """judge_clamp = (r, r) gives every head the ratio r: mask and output are those of a module given
    max_retain_ratio = full((H,), r) under the same seed, so the option consumed no random numbers
    (the sampling offsets are drawn inside the call)."""
    q, k, v, _, _ = _inputs(variant)
    r = 0.3
    res = []
    for kw in (dict(head_budget="judge", judge_clamp=(r, r)),
               dict(max_retain_ratio=torch.full((HEADS,), r))):
        m = _module(variant, **kw)
        torch.manual_seed(5)
        with torch.no_grad():
            out = m(q, k, v)
        res.append((m.last_mask.clone(), out, torch.rand(4, device=DEV)))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2])              # the generator is where the plain call leaves it
    assert 0 < int(res[0][0].sum()) < res[0][0].numel()


def test_module_steady_state_call_does_not_synchronise():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog", head_budget="judge", max_retain_ratio=0.5)
    with torch.no_grad():
        a = m(q, k, v, q_off=qo, k_off=ko)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            b = m(q, k, v, q_off=qo, k_off=ko)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, b)


def test_module_call_captures_into_a_hip_graph():
    ops = _ops()
    q, k, v, _, _ = _inputs("cog")
    m = _module("cog", head_budget="judge", max_retain_ratio=0.5)
    B, H = q.shape[:2]
    with torch.no_grad():
        m(q, k, v)                                   # warm up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                out = m(q, k, v)
        torch.cuda.current_stream().wait_stream(s)
        captured_mask, captured_budget = m.last_mask, m.last_head_budget
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        state = gen.get_state()
        graph.replay()
        torch.cuda.synchronize()
        replayed = (captured_mask.clone(), captured_budget.clone(), out.clone())
        # the same generator state, eagerly, gives the draws (and so the offsets) the replay used
        gen.set_state(state)
        rq = torch.rand(B, H, 1, 128, device=DEV)
        rk = torch.rand(B, H, 1, 128, device=DEV)
        qo, ko = ops.sample_offsets(rq, rk, 32)
        eager = m(q, k, v, q_off=qo[:, :, 0], k_off=ko[:, :, 0])
        torch.cuda.synchronize()
    assert torch.equal(m.last_head_budget, replayed[1])
    assert torch.equal(m.last_mask, replayed[0])
    assert torch.equal(eager, replayed[2])


def test_module_under_autograd_predicts_the_same_mask():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog", head_budget="judge", max_retain_ratio=0.5)
    with torch.no_grad():
        m(q, k, v, q_off=qo, k_off=ko)
    mask, budget = m.last_mask.clone(), m.last_head_budget.clone()
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = m(qq, kk, vv, q_off=qo, k_off=ko)
    assert torch.equal(m.last_mask, mask) and torch.equal(m.last_head_budget, budget)
    out.float().square().sum().backward()
    for t in (qq, kk, vv):
        assert t.grad is not None and torch.isfinite(t.grad.float()).all()


def test_fused_qk_processor_feeds_its_strided_views():
    """A fused_qk=True CogVideoX processor hands inner_attention [B,L,H,D].transpose(1,2) views: the
    estimator reads them where they lie and gives the bits it gives on contiguous copies."""
    ops = _ops()
    from vblade import attention, patch
    from qk_standins import StandInAttention
    heads, hd, T = 2, 64, 26
    m = _module("cog", head_budget="judge", max_retain_ratio=0.5)
    N = 16 * 12 * 6
    attn = StandInAttention(heads * hd, heads, "cog").to(DEV, torch.bfloat16)
    go = torch.Generator(device=DEV).manual_seed(3)
    q_off, k_off = attention.draw_sample_offsets_qk(1, heads, DEV, generator=go)
    seen = []

    def inner(q, k, v):
        seen.append((q, k))
        return m(q, k, v, q_off=q_off, k_off=k_off)

    attn.inner_attention = inner
    g = torch.Generator().manual_seed(60)
    hidden = torch.randn(1, N, heads * hd, generator=g).to(DEV, torch.bfloat16)
    text = torch.randn(1, T, heads * hd, generator=g).to(DEV, torch.bfloat16)
    ang = (torch.rand(N, hd // 2, generator=g, dtype=torch.float64) * 6.28).repeat_interleave(2, -1)
    rope = (ang.cos().float().to(DEV), ang.sin().float().to(DEV))
    proc = patch.CogVideoXBlockSparseAttnProcessor(0, fused_qk=True)
    with torch.no_grad():
        proc(attn, hidden, text, image_rotary_emb=rope)
    assert proc.last_path == "fused"
    q, k = seen[0]
    assert not q.is_contiguous() and ops._aligned_bhld(q) is q and ops._aligned_bhld(k) is k
    assert torch.equal(m.last_head_sparsity, ops.judge_sparsity(q.contiguous(), k.contiguous(), m.judge_rows))
    want, _ = J.head_budget(m.last_head_sparsity.cpu().numpy(), 10, m.max_retain_ratio, m.judge_clamp, "cog")
    assert np.array_equal(m.last_head_budget.cpu().numpy(), want)
