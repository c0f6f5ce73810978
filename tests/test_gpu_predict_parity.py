"""GPU: the max-proxy score kernel (csrc/vb_predict_kernel.hpp, behind vb_mask_predict, _long and _rule) on
INEXACT inputs, against the float64 interval reference of tests/predict_ref.py.

The other score tests feed multiples of 1/4, on which every fp32 partial product is exact and bit equality
with the oracle is possible; logits stay within a few units and every row maximum is positive. Here the
inputs are realistic (six regimes: predict_ref.input_regime, plus `underflow`, which reaches the range where
v_exp_f32 flushes), so the kernel's summation order shows and a tolerance cannot separate a reordering from
a change of function (a flip of R at |R| ~ 32 in bf16 is a factor 2^0.25). The assertion is
lo <= po <= hi at every element, [lo, hi] holding every result a correct fp32 evaluation can produce;
tests/test_predict_ref.py shows on the CPU that the intervals contain the oracle, are mostly within two
storage ulps, and reject eight changed functions.

Every test prints its figures before it asserts. References are computed once per case and shared.

Measured on an MI355X (profiles/predict_parity_pytest_gpu.log): no element outside its interval in any
case. The kernel's scores differ from the fp32 oracle's only in a handful of places: where v_exp_f32 flushes
(the `underflow` regime in bf16: every element whose lower end is 0 comes back as 0, up to 8 of 75 at
L = 600, keep 64, where the oracle keeps a subnormal), on 1 of 162 elements of `outlier` bf16 at L = 1100,
keep 16, and on 1e-4 of the 103041 elements of the nb = 321 case; all inside their intervals."""
import numpy as np
import pytest
import torch

import bsa_oracle as O
import predict_ref as P
import rule_ref as R
from test_gpu_predict_keep import _pooled_scores_chunked

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}

# (L, D, H): one partial block with replicate padding; odd nb, a partial K tile, force_tail 2; the D = 128 tile
SHAPES = {"L100": (100, 64, 1), "L600": (600, 64, 3), "L1100": (1100, 128, 2)}
KEEPS = (16, 32, 64)
BF16_REGIMES = P.REGIMES + P.EXTRA_REGIMES
FP16_REGIMES = ("randn", "wide", "negative") + P.EXTRA_REGIMES
# the rule's scalars on the L600 shape (nb = 5): room between the bounds, CogVideoX's forced tail
LO, HI, FT, THR = 1, 3, 2, 0.95


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _ops():
    from vblade import ops
    return ops


_REF = {}


def _case(regime, shape, keep, dt, B=1):
    """The case's inputs with its interval and the fp32 oracle's scores, computed once."""
    key = (regime, shape, keep, dt, B)
    if key not in _REF:
        L, D, H = SHAPES[shape] if isinstance(shape, str) else shape
        s = P.case_inputs(regime, L, D, H, keep, DT[dt], B=B)
        _with_reference(s)
        _REF[key] = s
    return _REF[key]


def _with_reference(s):
    s["lo"], s["hi"] = P.score_interval(s["qs"], s["ks"], s["scale"], s["keep"], s["dtype"])
    if s["nb"] <= 64:
        s["ref"] = O.pooled_scores(s["qs"], s["ks"], s["scale"], s["keep"], s["dtype"])
    else:   # the oracle's statements a few q-blocks at a time
        s["ref"] = _pooled_scores_chunked(s["qs"], s["ks"], s["scale"], s["keep"], s["dtype"])
    return s


def _predict(s, q=None, k=None, **kw):
    """ops.mask_predict on the case's inputs (q, k: other layouts of the same values)."""
    q = s["q"].to(DEV) if q is None else q
    k = s["k"].to(DEV) if k is None else k
    if "rand" not in kw and "philox" not in kw:
        kw.update(q_off=s["qo"].int().to(DEV), k_off=s["ko"].int().to(DEV))
    return _ops().mask_predict(q, k, rows=s["rows"].int().to(DEV), **kw)


def _assert_inside(tag, po, s):
    """lo <= po <= hi everywhere; prints the worst position within an interval (|1| = an end) and the
    share of elements that differ from the fp32 oracle."""
    po = po.float().cpu().double()
    lo, hi = s["lo"], s["hi"]
    assert po.shape == lo.shape, (po.shape, lo.shape)
    out = P.outside(po, lo, hi)
    open_ = hi > lo
    worst = float(P.position(po, lo, hi)[open_].abs().max()) if open_.any() else 0.0
    diff = float((po != s["ref"].double()).double().mean())
    flushed = (lo == 0) & (hi > 0)
    print(f"{tag}: outside {int(out.sum())} of {out.numel()}; worst position {worst:.3f} over {int(open_.sum())} open "
          f"intervals; differs from the fp32 oracle on {diff:.4f}; wider than two storage ulps "
          f"{P.wide_share(lo, hi, s['dtype']):.4f}; lower end flushed on {int(flushed.sum())}, of which the kernel "
          f"returns 0 on {int((flushed & (po == 0)).sum())}")
    if out.any():
        i = tuple(int(x) for x in out.nonzero()[0])
        print(f"  first outside at {i}: po {float(po[i]):.9g}, lo {float(lo[i]):.9g}, hi {float(hi[i]):.9g}")
    assert not out.any(), tag


# ------------------------------------------------------------------ 1. interval parity
_PARITY = ([(r, "bf16") for r in BF16_REGIMES] + [(r, "fp16") for r in FP16_REGIMES])


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("regime,dt", _PARITY, ids=[f"{r}-{d}" for r, d in _PARITY])
def test_scores_lie_inside_the_float64_interval(regime, dt, shape, keep):
    s = _case(regime, shape, keep, dt)
    po, _ = _predict(s, want_mask=False)
    assert po.dtype == s["dtype"] and torch.isfinite(po.float()).all()
    _assert_inside(f"{regime} {dt} {shape} keep {keep}", po, s)


# ------------------------------------------------------------------ 2. every entry
@pytest.mark.parametrize("regime", ["randn", "wide"])
@pytest.mark.parametrize("entry", ["long", "rule"])
def test_long_and_rule_entries_inside_the_interval_and_equal_to_the_short_entry(entry, regime):
    """At keep 32 the long and the rule instantiations return the short entry's bits (as
    test_remaining_score_kernel_instantiations establishes on exact inputs)."""
    s = _case(regime, "L600", 32, "bf16")
    kw = dict(min_keep=LO, max_keep=HI, force_tail=FT)
    po_s, mask_s = _predict(s, **kw)
    extra = dict(long_rows=True) if entry == "long" else dict(rule=_ops().MaskRule())
    po, mask = _predict(s, **kw, **extra)
    _assert_inside(f"{entry} entry, {regime}", po, s)
    assert torch.equal(po.view(torch.int16), po_s.view(torch.int16)) and torch.equal(mask, mask_s)


@pytest.mark.parametrize("regime", ["randn", "wide"])
@pytest.mark.parametrize("how", ["rand", "philox"])
def test_offsets_drawn_in_the_launch_inside_the_interval(how, regime):
    """The fused-draw path: the reference uses torch.topk of the same uniforms, which the launch ranks
    (test_offsets_drawn_in_the_sampling_launch_equal_torch_topk); the scores equal those of given offsets."""
    ops = _ops()
    L, D, H = SHAPES["L600"]
    s = dict(P.case_inputs(regime, L, D, H, 32, torch.bfloat16))
    torch.manual_seed(43)
    rq = torch.rand(1, H, 1, 128, device=DEV)
    rk = torch.rand(1, H, 1, 128, device=DEV)
    s["qo"] = torch.topk(rq, 32, dim=3).indices[:, :, 0].cpu()
    s["ko"] = torch.topk(rk, 32, dim=3).indices[:, :, 0].cpu()
    s["qs"], s["ks"] = P.sampled_streams(s["q"], s["k"], s["qo"], s["ko"], s["rows"])
    _with_reference(s)
    if how == "rand":
        po, _ = _predict(s, rand=(rq, rk), num_keep=32, want_mask=False)
    else:
        torch.manual_seed(43)
        philox = ops.claim_rand_draws(DEV, H * 128)
        assert philox is not None
        po, _ = _predict(s, philox=philox, num_keep=32, want_mask=False)
    _assert_inside(f"{how} draw, {regime}", po, s)
    po_given, _ = _predict(s, want_mask=False)
    assert torch.equal(po.view(torch.int16), po_given.view(torch.int16))


# ------------------------------------------------------------------ 3. the long kernel proper
def test_long_kernel_past_the_short_row_limit():
    """nb = 321 (above the short entry's 320 blocks), D = 128, keep 16, `wide`, bf16: the chunked reference."""
    s = _case("wide", (41000, 128, 1), 16, "bf16")
    assert s["nb"] == 321
    po, _ = _predict(s, want_mask=False, long_rows=True)
    _assert_inside("long kernel nb 321", po, s)


# ------------------------------------------------------------------ 4. batch and layout
def test_batch_and_transposed_views():
    """B = 2, q and k given as transposed views of [B,L,H,D] storage: the bits of the contiguous call and of
    the two per-sample calls, inside the interval."""
    s = _case("wide", "L600", 32, "bf16", B=2)
    qd, kd = s["q"].to(DEV), s["k"].to(DEV)
    qv = qd.transpose(1, 2).contiguous().transpose(1, 2)
    kv = kd.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qv.is_contiguous() and qv.stride(2) == 3 * 64 and torch.equal(qv, qd)
    kw = dict(min_keep=LO, max_keep=HI, force_tail=FT)
    po_v, mask_v = _predict(s, q=qv, k=kv, **kw)
    po_c, mask_c = _predict(s, **kw)
    _assert_inside("B = 2, [B,L,H,D] views", po_v, s)
    assert torch.equal(po_v.view(torch.int16), po_c.view(torch.int16)) and torch.equal(mask_v, mask_c)
    for b in range(2):
        po_b, mask_b = _ops().mask_predict(qv[b:b + 1], kv[b:b + 1], s["qo"][b:b + 1].int().to(DEV),
                                           s["ko"][b:b + 1].int().to(DEV), rows=s["rows"].int().to(DEV), **kw)
        assert torch.equal(po_b.view(torch.int16), po_v[b:b + 1].view(torch.int16)), b
        assert torch.equal(mask_b, mask_v[b:b + 1]), b


# ------------------------------------------------------------------ 5. the mask on inexact scores
@pytest.mark.parametrize("regime", BF16_REGIMES)
def test_mask_is_the_energy_rule_on_the_kernels_own_scores(regime):
    s = _case(regime, "L600", 32, "bf16")
    nb, dtype = s["nb"], s["dtype"]
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    po, mask = _predict(s, min_keep=LO, max_keep=HI, force_tail=FT, energy_threshold=THR, mask_count=cnt)
    po_c, mask_c = po.float().cpu(), mask.bool().cpu()
    ref_mask = O.energy_mask(po_c, LO, HI, THR, FT, dtype)
    kk = O.energy_keep_counts(po_c, LO, HI, THR, dtype)
    print(f"{regime}: kept per row {mask_c.sum(-1).flatten().tolist()}, rule counts {kk.flatten().tolist()}")
    assert torch.equal(mask_c, ref_mask)
    assert cnt.item() == int(ref_mask.sum())
    assert O.mask_is_valid_topk(mask_c, po_c, kk, FT)
    if regime == "flat":
        # the zeroed q-block's scores are all equal: the stable order keeps the lowest indices, plus the tail
        i = P.FLAT_BLOCK
        assert (po_c[:, :, i] == po_c[:, :, i, :1]).all() and i < nb - FT
        for h in range(s["H"]):
            want = torch.zeros(nb, dtype=torch.bool)
            want[:int(kk[0, h, i])] = True
            want[-FT:] = True
            assert torch.equal(mask_c[0, h, i], want), h
    if regime == "onehot":
        # the reference alone says that the dominant block is every free row's best: its lower end is
        # above every other block's upper end. Then a mask that keeps at least one block keeps it.
        j = P.dominant_block(nb)
        others = torch.arange(nb) != j
        assert (s["lo"][:, :, :nb - FT, j] > s["hi"][:, :, :nb - FT][..., others].amax(-1)).all()
        assert mask_c[:, :, :nb - FT, j].all()


# ------------------------------------------------------------------ 6. the top-k rule
@pytest.mark.parametrize("shape", ["L600", "L1100"])
def test_topk_rule_on_wide_scores(shape):
    """mode="topk" in the score kernel's epilogue, against tests/rule_ref.py applied to the kernel's own
    scores: nb = 5 and nb = 9 (a second workgroup per head)."""
    ops = _ops()
    s = _case("wide", shape, 32, "bf16")
    nb = s["nb"]
    assert nb == {"L600": 5, "L1100": 9}[shape]
    for k0, ft in ((2, 0), (max(1, nb // 3), 2)):
        kept = torch.full((1, s["H"], nb), -1, dtype=torch.int32, device=DEV)
        po, mask = _predict(s, rule=ops.MaskRule(mode="topk", init_k=k0), force_tail=ft, rows_kept=kept)
        _assert_inside(f"topk rule {shape} k0 {k0}", po, s)
        po_np = po.float().cpu().numpy()
        kk = R.topk_counts(po_np, k0, "bf16")
        want = R.mask_from_counts(po_np, kk, ft)
        print(f"  counts {kk.flatten().tolist()}")
        assert np.array_equal(mask.bool().cpu().numpy(), want), (k0, ft)
        assert np.array_equal(kept.cpu().numpy(), want.sum(-1))
