"""Cases, bounds and checks of the LSE-combine parity tests (tests/test_lse_combine_ref.py on the CPU,
tests/test_gpu_lse_combine.py on the GPU).

The operation is adaptive_block_sparse_attn's combine, every eager op rounded to the storage dtype T
(bsa_oracle.combine_reference, which is the reference here):

    l1 = T(lse1), w2 = T(T(lse2) + T(ln T(gap))), mx = max(l1, w2)
    e1 = T(exp(T(l1 - mx))), e2 = T(exp(T(w2 - mx))), alpha = T(e1 / T(e1 + e2))
    out = T(T(out1 * alpha) + T(out2 * T(1 - alpha)))

A case is a shape, a dtype and a gap; its rows are dealt into classes by d = lse1 - (lse2 + ln gap), the
difference the weights depend on (CLASSES). What the checks demand (``combine_figures`` /
``assert_combine``) comes from that arithmetic alone:

(a) lse2 = -inf gives alpha == 1 and out == out1; lse1 = -inf with a zero out1 row gives alpha == 0 and
    out == out2, bit for bit; every value is finite.
(b) The only inexact fp32 operations are logf, expf and one division, each then rounded to T: a
    different last fp32 bit can flip a rounding to T, not more. So alpha's bits equal the reference's
    on at least 99 % of the rows, and differ by at most one ulp of T at max(alpha, alpha_ref) elsewhere.
    The CPU file holds the reference with exp and log evaluated in float64 against the same in float32
    to at most 0.25 % disagreeing rows per case, so the 99 % leave a fourfold margin that does not
    depend on the kernel.
(c) Where alpha's bits match, out matches bit for bit in every element: what is left is a conversion,
    two products of two T values (exact in fp32), 1 - alpha (exact in fp32) and one fp32 addition, each
    rounded to T the IEEE way on both sides.
(d) On the other rows |out - ref| <= 2 u (|out1| + |out2|) + ulp_T(ref), u = 2^-8 (bf16) or 2^-11 (fp16):
    one ulp of alpha (at most u, since alpha <= 1), the same for 1 - alpha, the products' roundings, and
    one rounding of the result.
"""
import functools
import math
import types

import torch

import bsa_oracle as O

BF16, F16 = torch.bfloat16, torch.float16

SHAPES = [(2, 3, 333, 64, BF16), (1, 2, 129, 128, BF16), (1, 2, 129, 64, F16), (2, 2, 37, 128, F16),
          (1, 1, 1, 64, F16)]
GAPS = (15, 30, 1)   # ln 1 = 0
CASES = [(s, g) for s in SHAPES for g in GAPS]
IDS = [f"{B}x{H}x{L}x{D}-{'bf16' if t == BF16 else 'fp16'}-gap{g}" for (B, H, L, D, t), g in CASES]

# row classes, by d = lse1 - (lse2 + ln gap)
CLASSES = ("normal",      # d ~ N(0, 3)
           "half",        # |d| < 2^-6: alpha near 1/2
           "band",        # |d| uniform in [9.7, 17.3]: the smaller exponential is an fp16 subnormal
           "d40",         # d = +-40
           "d200",        # d = +-200: the smaller exponential underflows, alpha is exactly 0 or 1
           "near250",     # both LSEs near 250: rounding them to bf16 moves d by whole units
           "lse2_ninf",   # lse2 = -inf
           "lse1_ninf")   # lse1 = -inf and a zero out1 row: the native forward's empty mask row
CLS = {name: i for i, name in enumerate(CLASSES)}
ONE_ROW_CLASS = {15: "band", 30: "lse2_ninf", 1: "lse1_ninf"}   # the L = 1 shape: one class per gap
MIN_ROWS = 8           # rows per class, in every shape with more than one row

U = {BF16: 2.0 ** -8, F16: 2.0 ** -11}      # half an ulp of T at 1: the relative rounding error
MANT = {BF16: 7, F16: 10}                   # stored significand bits
EMIN = {BF16: -126, F16: -14}               # exponent of the smallest normal
BAND = (9.7, 17.3)
SEEDS = {}             # case index -> seed, for a case that had to be reseeded (test_lse_combine_ref.py)


def rnd(t, dtype):
    return O.rnd(t, dtype)


def ulp(x, dtype):
    """Spacing of ``dtype`` at |x| (float64): 2^(floor(log2 |x|) - MANT), the subnormal spacing below
    the smallest normal and at 0."""
    x = x.double().abs()
    e = torch.frexp(x).exponent.to(torch.int64) - 1    # x = m 2^(e+1), m in [0.5, 1)
    e = torch.where(x == 0, torch.full_like(e, EMIN[dtype]), e).clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(x), e - MANT[dtype])


def exp32(t):
    return torch.exp(t)


def exp64(t):
    """exp in float64, rounded to float32: a correctly rounded float32 exp but for double rounding."""
    return torch.exp(t.double()).float()


def log32(t):
    return torch.log(t)


def log64(t):
    return torch.log(t.double()).float()


def weights(lse1, lse2, gap, dtype, exp=exp32, log=log32, round_e1=True, flush=False):
    """The combine's weights, op by op as combine_reference takes them, with the two transcendental
    functions pluggable. ``round_e1=False`` (e1 kept in fp32) and ``flush=True`` (every rounding to storage
    flushes subnormal results to zero) are deliberately wrong variants the CPU file uses to show that the
    checks catch them. Returns a namespace of [B,H,L] float32 tensors."""
    def R(t):
        t = rnd(t, dtype)
        return torch.where(t.abs() < 2.0 ** EMIN[dtype], torch.zeros_like(t), t) if flush else t

    l1, l2 = R(lse1.float()), R(lse2.float())
    log_g = R(log(R(torch.tensor(float(gap)))))
    w2 = R(l2 + log_g)
    mx = torch.maximum(l1, w2)
    e1 = exp(R(l1 - mx))
    if round_e1:
        e1 = R(e1)
    e2 = R(exp(R(w2 - mx)))
    alpha = R(e1 / R(e1 + e2))
    return types.SimpleNamespace(l1=l1, w2=w2, e1=e1, e2=e2, alpha=alpha, log_g=log_g)


def blend(out1, out2, alpha, dtype, b=None):
    """out from the weights: T(T(out1 * alpha) + T(out2 * b)), b = T(1 - alpha) unless given. Returns a
    tensor of ``dtype``."""
    R = lambda t: rnd(t, dtype)  # noqa: E731
    a = alpha[..., None]
    b = R(1.0 - a) if b is None else b[..., None]
    return R(R(out1.float() * a) + R(out2.float() * b)).to(dtype)


def _band_is_subnormal(case_lse1, lse2, gap, dtype, rows):
    w = weights(case_lse1, lse2, gap, dtype)
    small = torch.minimum(w.e1, w.e2)
    return ((small > 0) & (small < 2.0 ** -14)) | ~rows


@functools.lru_cache(maxsize=None)
def make_case(idx):
    """Inputs, row classes and the reference's results of CASES[idx], built once and shared; nothing
    that uses them writes to them."""
    (B, H, L, D, dtype), gap = CASES[idx]
    g = torch.Generator().manual_seed(SEEDS.get(idx, 4200 + idx))
    N = B * H * L
    if N == 1:
        cls = torch.tensor([CLS[ONE_ROW_CLASS[gap]]])
    else:
        cls = torch.randperm(N, generator=g) % len(CLASSES)
    cls = cls.view(B, H, L)
    is_ = lambda name: cls == CLS[name]  # noqa: E731
    rand = lambda: torch.rand(B, H, L, generator=g)  # noqa: E731
    randn = lambda: torch.randn(B, H, L, generator=g)  # noqa: E731
    sign = torch.where(rand() < 0.5, -1.0, 1.0)
    log_g = float(rnd(torch.log(rnd(torch.tensor(float(gap)), dtype)), dtype))   # ln gap as the op takes it

    lse2 = randn() * 3 + 3
    d = randn() * 3
    lse2 = torch.where(is_("half"), randn(), lse2)       # small LSEs: their rounding stays below 2^-5
    d = torch.where(is_("half"), (rand() * 2 - 1) * 2.0 ** -6, d)
    d = torch.where(is_("band"), sign * (BAND[0] + rand() * (BAND[1] - BAND[0])), d)
    d = torch.where(is_("d40"), sign * 40.0, d)
    d = torch.where(is_("d200"), sign * 200.0, d)
    lse2 = torch.where(is_("near250"), 250.0 + randn() * 2, lse2)
    lse1 = lse2 + log_g + d
    if dtype == F16:
        # the band is where the smaller exponential is a nonzero fp16 subnormal AFTER the LSEs' own
        # rounding (which moves d by up to an ulp of the LSE): redraw the few rows at the band's edges
        # that the rounding pushed out
        for _ in range(64):
            bad = ~_band_is_subnormal(lse1, lse2, gap, dtype, is_("band"))
            if not bool(bad.any()):
                break
            redo = sign * (BAND[0] + rand() * (BAND[1] - BAND[0]))
            d = torch.where(bad, redo, d)
            lse1 = torch.where(bad, lse2 + log_g + redo, lse1)
    ninf = torch.full_like(lse1, -math.inf)
    lse2 = torch.where(is_("lse2_ninf"), ninf, lse2)
    lse1 = torch.where(is_("lse1_ninf"), ninf, lse1)
    out1 = torch.randn(B, H, L, D, generator=g)
    out2 = torch.randn(B, H, L, D, generator=g)
    out1 = torch.where(is_("lse1_ninf")[..., None], torch.zeros_like(out1), out1).to(dtype)
    out2 = out2.to(dtype)
    ref_out, ref_alpha = O.combine_reference(out1, lse1, out2, lse2, gap, dtype)
    return types.SimpleNamespace(idx=idx, shape=(B, H, L, D), dtype=dtype, gap=gap, cls=cls, d=d,
                                 out1=out1, out2=out2, lse1=lse1, lse2=lse2,
                                 ref_out=ref_out.to(dtype), ref_alpha=ref_alpha[..., 0].contiguous())


def _bits16(t):
    return t.contiguous().view(torch.int16)


def combine_figures(case, out, alpha):
    """What a combine's (out [B,H,L,D] in the case's dtype, alpha float32 [B,H,L]; CPU tensors) looks
    like against the case's reference: the figures assert_combine judges."""
    dtype = case.dtype
    ra = case.ref_alpha
    alpha = alpha.float().contiguous()
    got, ref = out.float(), case.ref_out.float()
    v1, v2 = case.out1.float(), case.out2.float()
    s2, s1 = case.cls == CLS["lse2_ninf"], case.cls == CLS["lse1_ninf"]
    same = alpha.view(torch.int32) == ra.view(torch.int32)
    rest = ~same
    out_same = (_bits16(out) == _bits16(case.ref_out)).all(-1)
    a_err = (alpha.double() - ra.double()).abs() / ulp(torch.maximum(alpha, ra), dtype)
    bound = 2 * U[dtype] * (v1.double().abs() + v2.double().abs()) + ulp(ref, dtype)
    o_err = ((got.double() - ref.double()).abs() / bound).amax(-1)
    worst = lambda t, m: float(t[m].max()) if bool(m.any()) else 0.0  # noqa: E731
    return dict(
        rows=alpha.numel(),
        finite=bool(torch.isfinite(got).all() and torch.isfinite(alpha).all()),
        lse2_ninf_ok=bool((alpha[s2] == 1).all() and (_bits16(out)[s2] == _bits16(case.out1)[s2]).all()),
        lse1_ninf_ok=bool((alpha[s1] == 0).all() and (_bits16(out)[s1] == _bits16(case.out2)[s1]).all()),
        alpha_equal_share=float(same.float().mean()),
        alpha_rest_worst_ulps=worst(a_err, rest),
        out_rows_differing_where_alpha_equal=int((same & ~out_same).sum()),
        out_rest_worst_over_bound=worst(o_err, rest))


def assert_combine(case, out, alpha):
    f = combine_figures(case, out, alpha)
    print(f"[combine {IDS[case.idx]}] {f}")
    assert f["finite"], f
    assert f["lse2_ninf_ok"] and f["lse1_ninf_ok"], f                # (a)
    assert f["alpha_equal_share"] >= 0.99, f                          # (b)
    assert f["alpha_rest_worst_ulps"] <= 1.0, f
    assert f["out_rows_differing_where_alpha_equal"] == 0, f          # (c)
    assert f["out_rest_worst_over_bound"] <= 1.0, f                   # (d)
    return f
