"""CPU: the inputs and bounds of tests/test_gpu_lse_combine.py, checked with the reference alone
(tests/combine_cases.py): every row class is present and is what its name says, the 99 % condition on
alpha has a margin that does not depend on the kernel, a one-ulp nudge of alpha stays inside the output
bound, and the checks themselves fail for two deliberately wrong combines."""
import pytest
import torch

import combine_cases as C
from combine_cases import CASES, CLS, IDS, make_case

ALL = range(len(CASES))


def _rows(case, name):
    return case.cls == CLS[name]


@pytest.mark.parametrize("idx", ALL, ids=IDS)
def test_every_class_is_present_as_intended(idx):
    c = make_case(idx)
    B, H, L, D = c.shape
    w = C.weights(c.lse1, c.lse2, c.gap, c.dtype)
    # the op-by-op restatement with float32 exp/log IS the reference (the same torch calls)
    assert torch.equal(w.alpha, c.ref_alpha)
    assert torch.equal(C.blend(c.out1, c.out2, w.alpha, c.dtype), c.ref_out)
    if B * H * L == 1:
        assert int(c.cls.view(-1)[0]) == CLS[C.ONE_ROW_CLASS[c.gap]]
    else:
        counts = torch.bincount(c.cls.view(-1), minlength=len(C.CLASSES))
        assert int(counts.min()) >= C.MIN_ROWS, counts.tolist()
    small = torch.minimum(w.e1, w.e2)
    dd = w.l1 - w.w2                                   # d as the op sees it, after the LSEs' rounding
    r = _rows(c, "half")
    # |d| < 2^-6 drawn; the LSEs here are below 8 in magnitude, so the roundings of l1, l2 and w2 move d
    # by at most 2.5 half-ulps of bf16's [4, 8), 2^-6 each: |d| <= 3.5 * 2^-6 as the op sees it, and
    # alpha = 1 / (1 + e^-d) is within |d| / 4 < 2^-6 of 1/2, plus its own rounding (2^-9)
    assert bool(((c.d[r]).abs() < 2.0 ** -6).all())
    assert bool((torch.maximum(w.l1[r].abs(), w.w2[r].abs()) < 8).all())
    assert bool((w.alpha[r] - 0.5).abs().le(2.0 ** -6 + 2.0 ** -9).all())
    r = _rows(c, "band")
    assert bool(((c.d[r].abs() >= C.BAND[0]) & (c.d[r].abs() <= C.BAND[1])).all())
    if c.dtype == torch.float16:
        # the band's point: the smaller exponential is a nonzero fp16 subnormal after its rounding
        assert bool(((small[r] > 0) & (small[r] < 2.0 ** -14)).all())
        assert bool((small[r] / 2.0 ** -24 == torch.round(small[r] / 2.0 ** -24)).all())
    r = _rows(c, "d40")
    assert bool((c.d[r].abs() == 40).all())
    r = _rows(c, "d200")
    assert bool((small[r] == 0).all()) and bool(((w.alpha[r] == 0) | (w.alpha[r] == 1)).all())
    assert bool((w.alpha[r] == (c.d[r] > 0).float()).all())
    r = _rows(c, "near250")
    assert bool(((c.lse1[r] - 250).abs() < 30).all() and ((c.lse2[r] - 250).abs() < 15).all())
    if c.dtype == torch.bfloat16:
        # bf16 has 8 significand bits: in [128, 256) every value is a whole number, so d is one
        assert bool((dd[r] == torch.round(dd[r])).all())
    r = _rows(c, "lse2_ninf")
    assert bool(torch.isneginf(c.lse2[r]).all()) and bool((c.ref_alpha[r] == 1).all())
    assert torch.equal(c.ref_out[r], c.out1[r])
    r = _rows(c, "lse1_ninf")
    assert bool(torch.isneginf(c.lse1[r]).all()) and bool((c.out1[r] == 0).all())
    assert bool((c.ref_alpha[r] == 0).all()) and torch.equal(c.ref_out[r], c.out2[r])
    assert bool(torch.isfinite(c.ref_out.float()).all()) and bool(torch.isfinite(c.ref_alpha).all())


@pytest.mark.parametrize("idx", ALL, ids=IDS)
def test_float64_and_float32_transcendentals_agree_on_alpha(idx):
    """exp and log in float64 (rounded to float32) against the reference's float32 ones: alpha's bits
    differ on at most 0.25 % of a case's rows, a quarter of what check (b) allows a kernel whose expf and
    logf are as good. A case that fails this is reseeded (combine_cases.SEEDS)."""
    c = make_case(idx)
    w64 = C.weights(c.lse1, c.lse2, c.gap, c.dtype, exp=C.exp64, log=C.log64)
    differ = (w64.alpha.view(torch.int32) != c.ref_alpha.view(torch.int32)).float().mean().item()
    assert differ <= 0.0025, differ
    # and that evaluation passes every check, as a correct kernel must
    C.assert_combine(c, C.blend(c.out1, c.out2, w64.alpha, c.dtype), w64.alpha)


@pytest.mark.parametrize("idx", ALL, ids=IDS)
def test_one_ulp_of_alpha_stays_inside_the_output_bound(idx):
    """alpha moved one ulp of T up and down (kept in [0, 1]): the output stays within bound (d) of the
    reference's on every row, so a kernel whose alpha flips one rounding cannot miss (d)."""
    c = make_case(idx)
    v1, v2, ref = c.out1.double(), c.out2.double(), c.ref_out.double()
    bound = 2 * C.U[c.dtype] * (v1.abs() + v2.abs()) + C.ulp(ref, c.dtype)
    bits = c.ref_alpha.to(c.dtype).view(torch.int16)    # alpha >= 0: its neighbours in T are bits +- 1
    for step in (1, -1):
        a = (bits + step).clamp_min(0).view(c.dtype).float().clamp(0, 1)
        moved = (a - c.ref_alpha).abs()
        assert bool((moved > 0).any()) or moved.numel() == 1
        assert bool((moved <= C.ulp(torch.maximum(a, c.ref_alpha), c.dtype)).all())
        out = C.blend(c.out1, c.out2, a, c.dtype).double()
        assert bool(((out - ref).abs() <= bound).all()), ((out - ref).abs() / bound).max().item()


def test_the_reference_itself_passes_every_check():
    for idx in ALL:
        c = make_case(idx)
        f = C.assert_combine(c, c.ref_out, c.ref_alpha)
        assert f["alpha_equal_share"] == 1.0


def _b_equals_a(c):
    """1 - alpha replaced by alpha."""
    return C.blend(c.out1, c.out2, c.ref_alpha, c.dtype, b=c.ref_alpha), c.ref_alpha


def _e1_unrounded(c):
    """e1 not rounded to storage before the sum and the division."""
    a = C.weights(c.lse1, c.lse2, c.gap, c.dtype, round_e1=False).alpha
    return C.blend(c.out1, c.out2, a, c.dtype), a


def _subnormals_flushed(c):
    """Rounding to storage flushes subnormal results to zero (fp16: the band rows' smaller exponential)."""
    a = C.weights(c.lse1, c.lse2, c.gap, c.dtype, flush=True).alpha
    return C.blend(c.out1, c.out2, a, c.dtype), a


WRONG = {"b_equals_a": _b_equals_a, "e1_unrounded": _e1_unrounded}
MANY_ROWS = [i for i in ALL if CASES[i][0][2] > 1]


@pytest.mark.parametrize("bug", sorted(WRONG))
@pytest.mark.parametrize("idx", MANY_ROWS, ids=[IDS[i] for i in MANY_ROWS])
def test_the_checks_reject_a_wrong_combine(idx, bug):
    """The two mistakes the GPU test must catch, made in the restatement instead of the kernel: the checks
    fail for each, in every case with more than one row."""
    c = make_case(idx)
    out, alpha = WRONG[bug](c)
    with pytest.raises(AssertionError):
        C.assert_combine(c, out, alpha)


FP16_MANY = [i for i in MANY_ROWS if CASES[i][0][4] == torch.float16]


@pytest.mark.parametrize("idx", FP16_MANY, ids=[IDS[i] for i in FP16_MANY])
def test_the_checks_reject_flushed_fp16_subnormals(idx):
    """What the band rows are for: a combine whose storage rounding flushes fp16 subnormals gives alpha = 0
    where the reference keeps a subnormal weight, many ulps away, and check (b) fails."""
    c = make_case(idx)
    out, alpha = _subnormals_flushed(c)
    f = C.combine_figures(c, out, alpha)
    assert f["alpha_rest_worst_ulps"] > 1.0, f
    with pytest.raises(AssertionError):
        C.assert_combine(c, out, alpha)
