"""GPU: the q/k prologue's backward (vb_qk_prologue_bwd / ops.qk_prologue_bwd / autograd.qk_prologue /
the processors' fused_qk_backward) against an fp64 ideal: the fp64 autograd gradient of an fp64
statement of norm -> RoPE with no intermediate rounding (written below), evaluated on the
storage-dtype x, g and parameters.

Bounds: half a storage ulp of the final rounding plus 2^-18 (64 fp32 ulps) of evaluation slack,
the slack taken relative to the magnitudes BEFORE cancellation:

    dx       |got - ideal| <= 1/2 ulp_T(max(|ideal|, |got|)) + 2^-18 * S, S per reduction row:
             LayerNorm  S = rstd * (max|a| + mean|a| + max|xhat| * mean|a*xhat|)  over the head
             RMSNorm    S = rstd * (max|a| + max|xhat| * mean|a*xhat|)            over the H*D row
             no norm    S = |g_a| + |g_b| of the element's RoPE pair
    dweight  |got - ideal| <= 2^-18 * sum_i |gy_i| * max_row(i)|xhat| + N * 2^-24 * sum_i |t_i|
    dbias    the same with max|xhat| read as 1 and t = gy

with a = gy*w, gy = RoPE^T g, t_i the N summed terms (N * 2^-24: the worst case of any fp32
summation order). Through autograd the parameter gradients are cast to the parameter's dtype: one
more rounding, so half a storage ulp is added to their bound there.
"""
import copy

import pytest
import torch
from torch.utils.checkpoint import checkpoint

from conftest import record
from qk_standins import StandInAttention

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK = 2.0 ** -18
BF16, F16 = torch.bfloat16, torch.float16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------
# the fp64 ideal and the bounds
# ------------------------------------------------------------------------------------------------
def ulp(mag, dtype):
    """Spacing of `dtype` at magnitude `mag` (fp64 tensor): 2^(floor(log2 mag) - p), subnormals flat."""
    p, emin = (7, -126) if dtype == BF16 else (10, -14)
    return torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** emin))) - p)


def rope64(y, rope, start, cos, sin, freqs):
    """fp64 RoPE on y [B,L,H,D]: the real form on the rows from `start`, or the complex product."""
    if rope == "real":
        c, s = cos.double()[None, :, None, :], sin.double()[None, :, None, :]
        v = y[:, start:]
        rot = torch.stack([-v[..., 1::2], v[..., 0::2]], -1).flatten(-2)
        return torch.cat([y[:, :start], v * c + rot * s], 1)
    if rope == "complex":
        L, D = y.shape[1], y.shape[3]
        f = freqs.reshape(L, D // 2).to(torch.complex128)[None, :, None, :]
        z = torch.view_as_complex(y.unflatten(-1, (-1, 2)).contiguous()) * f
        return torch.view_as_real(z).flatten(-2)
    return y


def ideal_bwd(x, g, H, norm="none", w=None, b=None, eps=0.0, rope="none", start=0, cos=None, sin=None, freqs=None):
    """fp64 autograd through norm -> RoPE at x [B,L,H*D] and g [B,H,L,D] (storage-dtype values).
    Returns dx [B,L,H,D], dw, db, and the bounds' slack terms S (like dx), slack_w, slack_b."""
    B, L, W = x.shape
    D = W // H
    x64 = x.detach().double().reshape(B, L, H, D).requires_grad_()
    g64 = g.detach().double().transpose(1, 2)
    w64 = None if w is None else w.detach().double().requires_grad_()
    b64 = None if b is None else b.detach().double().requires_grad_()
    one = torch.ones((), device=x.device, dtype=torch.float64)
    if norm == "layer":
        dev = x64 - x64.mean(-1, keepdim=True)
        rstd = torch.rsqrt((dev * dev).mean(-1, keepdim=True) + eps)
        xhat = dev * rstd
        y = xhat * (one if w64 is None else w64)
        y = y if b64 is None else y + b64
    elif norm == "rms":
        xr = x64.reshape(B, L, W)
        rstd = torch.rsqrt((xr * xr).mean(-1, keepdim=True) + eps)
        xhat = xr * rstd
        y = (xhat * (one if w64 is None else w64)).reshape(B, L, H, D)
    else:
        y = x64 * one
    params = [p for p in (w64, b64) if p is not None]
    grads = list(torch.autograd.grad(rope64(y, rope, start, cos, sin, freqs), [x64] + params, g64))
    dx = grads.pop(0)
    dw = grads.pop(0) if w64 is not None else None
    db = grads.pop(0) if b64 is not None else None
    y0 = torch.zeros_like(g64).requires_grad_()     # RoPE is linear: its transpose at g
    gy = g64 if rope == "none" else torch.autograd.grad(rope64(y0, rope, start, cos, sin, freqs), y0, g64)[0]
    slack_w = slack_b = None
    with torch.no_grad():
        wv = one if w64 is None else w64
        if norm == "layer":
            a = gy * wv
            xmax = xhat.abs().amax(-1, keepdim=True)
            S = rstd * (a.abs().amax(-1, keepdim=True) + a.abs().mean(-1, keepdim=True)
                        + xmax * (a * xhat).abs().mean(-1, keepdim=True))
            S = S.expand_as(dx)
            N = B * L * H
            slack_w = SLACK * (gy.abs() * xmax).sum((0, 1, 2)) + N * 2.0 ** -24 * (gy * xhat).abs().sum((0, 1, 2))
            slack_b = SLACK * gy.abs().sum((0, 1, 2)) + N * 2.0 ** -24 * gy.abs().sum((0, 1, 2))
        elif norm == "rms":
            gyr = gy.reshape(B, L, W)
            a = gyr * wv
            xmax = xhat.abs().amax(-1, keepdim=True)
            S = rstd * (a.abs().amax(-1, keepdim=True) + xmax * (a * xhat).abs().mean(-1, keepdim=True))
            S = S.expand(B, L, W).reshape(B, L, H, D)
            slack_w = SLACK * (gyr.abs() * xmax).sum((0, 1)) + B * L * 2.0 ** -24 * (gyr * xhat).abs().sum((0, 1))
        else:
            pair = g64.abs().unflatten(-1, (-1, 2)).sum(-1, keepdim=True)
            S = pair.expand(B, L, H, D // 2, 2).flatten(-2)
    return dict(dx=dx.detach(), dw=dw, db=db, S=S, slack_w=slack_w, slack_b=slack_b)


def dx_ratio(got, ref, dtype, extra=0.0):
    """Worst |got - ideal| / bound over dx (<= 1 passes); got [B,L,H*D] or [B,L,H,D]. `extra` widens
    the slack on S for a result whose input was rounded on the way (the two-step form only)."""
    got = got.double().reshape(ref["dx"].shape)
    bound = 0.5 * ulp(torch.maximum(ref["dx"].abs(), got.abs()), dtype) + (SLACK + extra) * ref["S"]
    return ((got - ref["dx"]).abs() / bound).max().item()


def w_ratio(got, ideal, slack, cast=None):
    """Worst |got - ideal| / bound over a parameter gradient; `cast`: the dtype it was rounded to."""
    got = got.double().reshape(ideal.shape)
    bound = slack if cast is None else slack + 0.5 * ulp(torch.maximum(ideal.abs(), got.abs()), cast)
    return ((got - ideal).abs() / bound).max().item()


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
def randn(*shape, seed, dtype=BF16, mean=0.0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std + mean).to(DEV, dtype)


def rope_tables(S, hd, seed=3):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * 6.28
    ang2 = ang.repeat_interleave(2, -1)
    return ((ang2.cos().float().to(DEV), ang2.sin().float().to(DEV)),
            torch.polar(torch.ones_like(ang), ang)[None, None].to(DEV))


def make_case(norm, rope, B, L, H, D, dtype, *, start=0, affine=None, table=torch.complex128, seed=0,
              x_mean=0.2, x_std=1.3, eps=(1e-5, 1e-6)):
    """q and k inputs as batch slices of larger buffers; q's gradient [B,H,L,D]-contiguous, k's the
    transposed view of [B,L,H,D] memory. Returns (tensors, keywords of the op)."""
    W = H * D
    xq, xk = (randn(B, L + 7, W, seed=seed + s, dtype=dtype, mean=x_mean, std=x_std)[:, 3:3 + L] for s in (1, 2))
    gq = randn(B, H, L, D, seed=seed + 3, dtype=dtype)
    gk = randn(B, L, H, D, seed=seed + 4, dtype=dtype).transpose(1, 2)
    kw = dict(heads=H, norm=norm, rope=rope, q_eps=eps[0], k_eps=eps[1])
    if norm != "none":
        n = D if norm == "layer" else W
        wdt = torch.float32 if affine == "fp32" else dtype
        g = torch.Generator().manual_seed(seed + 5)
        for name in ("q_weight", "k_weight"):
            kw[name] = (1 + 0.1 * torch.randn(n, generator=g)).to(DEV, wdt)
        if norm == "layer":
            for name in ("q_bias", "k_bias"):
                kw[name] = (0.1 * torch.randn(n, generator=g)).to(DEV, wdt)
    if rope == "real":
        (cos, sin), _ = rope_tables(L - start, D, seed=seed + 6)
        kw.update(rope_start=start, cos=cos, sin=sin)
    elif rope == "complex":
        kw["freqs"] = rope_tables(L, D, seed=seed + 6)[1].to(table)
    return (xq, xk, gq, gk), kw


def ideal_of(x, g, kw, which):
    """ideal_bwd for the q or the k tensor of a make_case keyword set."""
    norm = kw["norm"] if isinstance(kw["norm"], str) else kw["norm"]["qk".index(which)]
    rope = kw["rope"] if isinstance(kw["rope"], str) else kw["rope"]["qk".index(which)]
    return ideal_bwd(x, g, kw["heads"], norm, kw.get(which + "_weight"), kw.get(which + "_bias"), kw[which + "_eps"],
                     rope, kw.get("rope_start", 0), kw.get("cos"), kw.get("sin"), kw.get("freqs"))


def check_case(label, tensors, kw, dtype, wgrad):
    """The op at grid_limit 3 and 0, each twice: every dx and parameter gradient within its bound, dx
    bit-equal between the grid limits, parameter gradients bit-equal across the two calls of one
    grid limit. Returns the worst ratios (dx, parameters)."""
    from vblade import ops
    xq, xk, gq, gk = tensors
    refs = [ideal_of(xq, gq, kw, "q"), ideal_of(xk, gk, kw, "k")]
    worst_dx = worst_w = 0.0
    first = None
    for limit in (3, 0):
        runs = [ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, need_wgrad=wgrad, grid_limit=limit, **kw) for _ in range(2)]
        out = runs[0]
        for a, b in zip(*runs):
            assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"{label}: not reproducible"
        for t, (x, ref) in enumerate(zip((xq, xk), refs)):
            dx, dw, db = out[t], out[2 + 2 * t], out[3 + 2 * t]
            assert dx.shape == x.shape and dx.dtype == dtype and dx.is_contiguous()
            worst_dx = max(worst_dx, dx_ratio(dx, ref, dtype))
            assert (dw is not None) == bool(wgrad[2 * t]) and (db is not None) == bool(wgrad[2 * t + 1])
            if dw is not None:
                assert dw.dtype == torch.float32
                worst_w = max(worst_w, w_ratio(dw, ref["dw"], ref["slack_w"]))
            if db is not None:
                assert db.dtype == torch.float32
                worst_w = max(worst_w, w_ratio(db, ref["db"], ref["slack_b"]))
        if first is None:
            first = out
        else:
            assert torch.equal(first[0], out[0]) and torch.equal(first[1], out[1]), f"{label}: grid_limit changed dx"
    print(f"{label}: worst |err|/bound dx {worst_dx:.3f}, parameters {worst_w:.2e}")
    record("qk_prologue_bwd: worst |err|/bound (dx, parameter gradients)", f"{label}: {worst_dx:.3f}, {worst_w:.2e}")
    return worst_dx, worst_w


# ------------------------------------------------------------------------------------------------
# the two real chains, at the smallest shapes where each mechanism can go wrong
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", ["storage", "fp32"])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H,L", [(3, 82), (48, 20)])
def test_layer_norm_real_rope_within_bounds(H, L, dtype, affine):
    """B=2, D=64, rope_start=5. H=3: 24 lanes, one partial wave with inactive lanes, 164 rows that
    grid_limit=3 deals 55/55/54; H=48: six waves and a cross-head reduction over 48 heads."""
    tensors, kw = make_case("layer", "real", 2, L, H, 64, dtype, start=5, affine=affine, seed=100 + H)
    worst_dx, worst_w = check_case(f"layer+real H={H} L={L} {dtype} {affine}", tensors, kw, dtype, (1, 1, 1, 1))
    assert worst_dx <= 1.0 and worst_w <= 1.0


@pytest.mark.parametrize("H", [1, 2, 4, 5, 12])
def test_layer_norm_head_dim_128_parameter_gradients(H):
    """LayerNorm at D=128 with every parameter gradient: H <= 4 launches one wave of 64 lanes, fewer
    than the D columns of a workgroup's partial vector (H=1: 16 active lanes); H=5 is the first
    two-wave row, H=12 three waves. B=2, L=41, rope_start=5."""
    tensors, kw = make_case("layer", "real", 2, 41, H, 128, BF16, start=5, seed=150 + H)
    worst_dx, worst_w = check_case(f"layer+real D=128 H={H}", tensors, kw, BF16, (1, 1, 1, 1))
    assert worst_dx <= 1.0 and worst_w <= 1.0


@pytest.mark.parametrize("table", [torch.complex128, torch.complex64])
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("H", [2, 12])
def test_rms_norm_complex_rope_within_bounds(H, dtype, table):
    """B=2, D=128, L=82. H=2: half a wave; H=12: three waves, the cross-wave LDS reduction."""
    tensors, kw = make_case("rms", "complex", 2, 82, H, 128, dtype, table=table, seed=200 + H)
    worst_dx, worst_w = check_case(f"rms+complex H={H} {dtype} {table}", tensors, kw, dtype, (1, 0, 1, 0))
    assert worst_dx <= 1.0 and worst_w <= 1.0


@pytest.mark.parametrize("rope", ["real", "complex"])
def test_rope_alone_within_bounds_and_text_rows_pass_through(rope):
    """No norm: S = |g_a| + |g_b|. Real RoPE: the rows below rope_start have dx == g bit for bit."""
    from vblade import ops
    B, L, H, D, T = 2, 82, 3, 64 if rope == "real" else 128, 5 if rope == "real" else 0
    tensors, kw = make_case("none", rope, B, L, H, D, BF16, start=T, seed=300)
    worst_dx, _ = check_case(f"{rope} rope alone", tensors, kw, BF16, (0, 0, 0, 0))
    assert worst_dx <= 1.0
    xq, xk, gq, gk = tensors
    dq, dk = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **kw)[:2]
    for dx, g in ((dq, gq), (dk, gk)):
        g_blw = g.transpose(1, 2).reshape(B, L, H * D)
        assert torch.equal(dx[:, :T], g_blw[:, :T])
        assert not torch.equal(dx[:, T:], g_blw[:, T:])


# ------------------------------------------------------------------------------------------------
# bit-for-bit properties
# ------------------------------------------------------------------------------------------------
def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


@pytest.mark.parametrize("name", ["cog", "wan"])
def test_call_forms_agree_bit_for_bit(name):
    """q alone == the q half of a q+k call; k alone (no gradient for q) == the k half; a sample at
    B=1 == its slice of the B=2 call; need_wgrad off gives the same dx."""
    from vblade import ops
    if name == "cog":
        tensors, kw = make_case("layer", "real", 2, 82, 3, 64, BF16, start=5, seed=400)
        wgrad = (1, 1, 1, 1)
    else:
        tensors, kw = make_case("rms", "complex", 2, 82, 12, 128, BF16, seed=410)
        wgrad = (1, 0, 1, 0)
    xq, xk, gq, gk = tensors
    both = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, need_wgrad=wgrad, grid_limit=3, **kw)
    q_kw = {a: v for a, v in kw.items() if not a.startswith("k_")}
    q_only = ops.qk_prologue_bwd(xq, gq=gq, need_wgrad=wgrad[:2] + (0, 0), grid_limit=3, **q_kw)
    assert _same(q_only[0], both[0]) and _same(q_only[2], both[2]) and _same(q_only[3], both[3])
    assert q_only[1] is None and q_only[4] is None and q_only[5] is None
    k_only = ops.qk_prologue_bwd(xq, xk, gq=None, gk=gk, need_wgrad=wgrad, grid_limit=3, **kw)
    assert _same(k_only[1], both[1]) and _same(k_only[4], both[4]) and _same(k_only[5], both[5])
    assert k_only[0] is None and k_only[2] is None and k_only[3] is None
    k_alone = ops.qk_prologue_bwd(None, xk, gk=gk, need_wgrad=(0, 0) + wgrad[2:], grid_limit=3, **kw)
    assert _same(k_alone[1], both[1]) and _same(k_alone[4], both[4]) and _same(k_alone[5], both[5])
    no_w = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **kw)
    assert torch.equal(no_w[0], both[0]) and torch.equal(no_w[1], both[1]) and no_w[2:] == (None,) * 4
    one = ops.qk_prologue_bwd(xq[1:], xk[1:], gq=gq[1:], gk=gk[1:], **kw)
    assert torch.equal(one[0], both[0][1:]) and torch.equal(one[1], both[1][1:])


def test_per_tensor_modes_and_the_two_step_form():
    """rope=("real", "none"), the cross-attention case: q as with RoPE on both, k as the norm alone.
    Norm + RoPE in one call against the RoPE backward followed by the norm backward: the fused form
    does not round in between, so the two differ in some elements and only bounds are asserted. The
    one-call form holds the plain bound. The two-step form's intermediate gy is rounded to bf16:
    |delta gy_i| <= 1/2 ulp(gy_i) <= 2^-8 |gy_i|, so |delta a_i| <= 2^-8 |a_i|, and through
    dx = rstd (a - mean a - xhat mean(a xhat)) that moves dx by at most
    2^-8 rstd (|a_i| + mean|a| + |xhat_i| mean|a xhat|) <= 2^-8 S: its bound is the plain one with
    2^-8 S added. The share of elements that differ between the two forms is printed."""
    from vblade import ops
    tensors, kw = make_case("layer", "real", 2, 82, 3, 64, BF16, start=5, seed=500)
    xq, xk, gq, gk = tensors
    both = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **kw)
    cross = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **{**kw, "rope": ("real", "none")})
    norm_kw = {a: v for a, v in kw.items() if a not in ("rope", "rope_start", "cos", "sin")}
    plain = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **norm_kw)
    assert torch.equal(cross[0], both[0]) and torch.equal(cross[1], plain[1])
    assert not torch.equal(cross[1], both[1])
    assert dx_ratio(cross[1], ideal_of(xk, gk, {**kw, "rope": "none"}, "k"), BF16) <= 1.0
    rope_kw = dict(heads=3, rope="real", rope_start=5, cos=kw["cos"], sin=kw["sin"])
    B, L, H, D = gq.shape[0], gq.shape[2], 3, 64
    step1 = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **rope_kw)[:2]
    step2 = ops.qk_prologue_bwd(xq, xk, gq=step1[0].view(B, L, H, D).transpose(1, 2),
                                gk=step1[1].view(B, L, H, D).transpose(1, 2), **norm_kw)
    share = max((step2[t] != both[t]).float().mean().item() for t in (0, 1))
    print(f"two-step vs one call: share of dx elements that differ {share:.3e}")
    record("qk_prologue_bwd: share of dx elements, RoPE-then-norm in two calls != one call", f"{share:.3e}")
    for t, (x, g) in enumerate(((xq, gq), (xk, gk))):
        ref = ideal_of(x, g, kw, "qk"[t])
        two = dx_ratio(step2[t], ref, BF16, extra=2.0 ** -8)
        print(f"two-step {'qk'[t]}: |err| / (bound + 2^-8 S) {two:.3f}; against the plain bound "
              f"{dx_ratio(step2[t], ref, BF16):.2f}")
        assert dx_ratio(both[t], ref, BF16) <= 1.0
        assert two <= 1.0


def test_weight_and_bias_of_two_dtypes_are_refused():
    """The backward reads the weight alone, in the precision the pair names: a bf16 weight beside an
    fp32 bias is refused as the forward refuses it, before any launch."""
    from vblade import ops
    tensors, kw = make_case("layer", "real", 2, 41, 3, 64, BF16, start=5, seed=550)
    xq, xk, gq, gk = tensors
    with pytest.raises(TypeError, match="share a dtype"):
        ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **{**kw, "q_bias": kw["q_bias"].float()})


def test_graph_capture_replays_bit_for_bit():
    """vb_qk_prologue_bwd and its reduction launch inside torch.cuda.graph: the replay writes what the
    direct call writes, parameter gradients included."""
    from vblade import ops
    tensors, kw = make_case("layer", "real", 2, 40, 5, 64, BF16, start=6, seed=600)
    xq, xk, gq, gk = (t.contiguous() for t in tensors)
    direct = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, need_wgrad=(1, 1, 1, 1), **kw)
    stat = [torch.zeros_like(t) for t in (xq, xk, gq, gk)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.qk_prologue_bwd(stat[0], stat[1], gq=stat[2], gk=stat[3], need_wgrad=(1, 1, 1, 1), **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.qk_prologue_bwd(stat[0], stat[1], gq=stat[2], gk=stat[3], need_wgrad=(1, 1, 1, 1), **kw)
    for s, t in zip(stat, (xq, xk, gq, gk)):
        s.copy_(t)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, direct):
        assert torch.equal(a, b)


@pytest.mark.parametrize("norm,H,D", [("layer", 3, 64), ("layer", 12, 128), ("rms", 2, 128), ("rms", 48, 64)])
def test_both_eps_values_are_really_used(norm, H, D):
    """Rows of N(0, 0.003^2): the variance / mean square (about 9e-6) is of the order of eps, and q and
    k take different eps values (1e-5, 2e-6). Each tensor holds its bound against the ideal with its
    own eps and violates it against the ideal with the other tensor's."""
    from vblade import ops
    eps = (1e-5, 2e-6)
    tensors, kw = make_case(norm, "none", 1, 9, H, D, BF16, seed=700 + H, x_mean=0.0, x_std=0.003, eps=eps)
    xq, xk, gq, gk = tensors
    out = ops.qk_prologue_bwd(xq, xk, gq=gq, gk=gk, **kw)
    swapped = {**kw, "q_eps": eps[1], "k_eps": eps[0]}
    for t, (x, g) in enumerate(((xq, gq), (xk, gk))):
        right = dx_ratio(out[t], ideal_of(x, g, kw, "qk"[t]), BF16)
        wrong = dx_ratio(out[t], ideal_of(x, g, swapped, "qk"[t]), BF16)
        print(f"eps test {norm} H={H} D={D} {'qk'[t]}: |err|/bound {right:.3f}; against the other eps {wrong:.1f}")
        assert right <= 1.0
        assert wrong > 1.0


# ------------------------------------------------------------------------------------------------
# autograd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", ["storage", "fp32"])
@pytest.mark.parametrize("name", ["cog", "wan"])
def test_autograd_function_holds_the_bounds(name, affine):
    """torch.autograd.grad through autograd.qk_prologue: the op's bounds (parameter gradients: plus
    the half ulp of their cast to a bf16 parameter's dtype; fp32 parameters take the fp32 sums as
    they are and hold the op's bound unchanged), gradient dtypes are the inputs' and the
    parameters', a None output gradient leaves that tensor out, and under
    checkpoint(use_reentrant=False) the gradients are the un-checkpointed ones bit for bit."""
    import vblade
    from vblade import autograd
    if name == "cog":
        tensors, kw = make_case("layer", "real", 2, 82, 3, 64, BF16, start=5, affine=affine, seed=800)
    else:
        tensors, kw = make_case("rms", "complex", 2, 82, 12, 128, BF16, affine=affine, seed=810)
    xq, xk, gq, gk = tensors
    xq, xk = xq.clone().requires_grad_(), xk.clone().requires_grad_()
    names = [n for n in ("q_weight", "q_bias", "k_weight", "k_bias") if n in kw]
    for n in names:
        kw[n] = kw[n].clone().requires_grad_()
    leaves = [xq, xk] + [kw[n] for n in names]

    def fn(a, b):
        return autograd.qk_prologue(a, b, **kw)

    q, k = fn(xq, xk)
    assert q.shape == gq.shape and q.stride(2) == gq.shape[1] * gq.shape[3]      # the [B,H,L,D] view
    with torch.no_grad():
        from vblade import ops
        ref_q, ref_k = ops.qk_prologue(xq, xk, **{n: (v.detach() if torch.is_tensor(v) else v) for n, v in kw.items()})
    assert torch.equal(q, ref_q) and torch.equal(k, ref_k)
    grads = torch.autograd.grad([q, k], leaves, [gq, gk])
    for t, gr in zip(leaves, grads):
        assert gr.dtype == t.dtype and gr.shape == t.shape
    refs = {"q": ideal_of(xq, gq, kw, "q"), "k": ideal_of(xk, gk, kw, "k")}
    assert dx_ratio(grads[0], refs["q"], BF16) <= 1.0 and dx_ratio(grads[1], refs["k"], BF16) <= 1.0
    for n, gr in zip(names, grads[2:]):
        ref = refs[n[0]]
        ideal, slack = (ref["dw"], ref["slack_w"]) if n.endswith("weight") else (ref["db"], ref["slack_b"])
        assert gr.dtype == (torch.float32 if affine == "fp32" else BF16)
        ratio = w_ratio(gr, ideal, slack, cast=None if affine == "fp32" else BF16)
        print(f"autograd {name} {affine} {n}: |err|/bound {ratio:.3e}")
        assert ratio <= 1.0
    only_q = torch.autograd.grad(fn(xq, xk)[0], [xq], gq)[0]            # k's output gradient is None
    assert torch.equal(only_q, grads[0])
    again = torch.autograd.grad(list(checkpoint(fn, xq, xk, use_reentrant=False)), leaves, [gq, gk])
    for a, b in zip(again, grads):
        assert torch.equal(a, b)
    with pytest.raises(TypeError, match="inplace"):
        autograd.qk_prologue(xq, xk, inplace=True, **kw)
    table = "cos" if name == "cog" else "freqs"
    with pytest.raises(ValueError, match="requires grad"):
        autograd.qk_prologue(xq, xk, **{**kw, table: kw[table].clone().requires_grad_()})
    assert vblade.qk_prologue is autograd.qk_prologue


# ------------------------------------------------------------------------------------------------
# processors
# ------------------------------------------------------------------------------------------------
def _proc_grads(kind, attn, flags, hidden, extra, upstream):
    """One processor call that records autograd; returns (last_path, gradients by name, q/k seen)."""
    from vblade import patch
    hidden = hidden.detach().clone().requires_grad_()
    attn.seen.clear()
    if kind == "cog":
        proc = patch.CogVideoXBlockSparseAttnProcessor(0, **flags)
        out = proc(attn, hidden, extra["text"], image_rotary_emb=extra["rope"])[0]
    else:
        proc = patch.WanBlockSparseAttnProcessor(**flags)
        out = proc(attn, hidden, None, rotary_emb=extra["freqs"])
    leaves = {"hidden_states": hidden, "to_q.weight": attn.to_q.weight, "to_k.weight": attn.to_k.weight,
              "norm_q.weight": attn.norm_q.weight, "norm_k.weight": attn.norm_k.weight}
    if getattr(attn.norm_q, "bias", None) is not None:
        leaves.update({"norm_q.bias": attn.norm_q.bias, "norm_k.bias": attn.norm_k.bias})
    grads = torch.autograd.grad(out, list(leaves.values()), upstream.to(out.dtype))
    return proc.last_path, dict(zip(leaves, (g.detach() for g in grads))), list(attn.seen)


def _ratio_rule(label, fused, eager, ideal):
    """||fused - ideal||_F <= 1.5 ||eager - ideal||_F for every gradient; returns the ratios."""
    ratios = {}
    for n in ideal:
        ef = (fused[n].double() - ideal[n]).norm().item()
        ee = (eager[n].double() - ideal[n]).norm().item()
        ratios[n] = ef / ee
        print(f"{label} {n}: ||fused - ideal|| {ef:.4e}, ||eager - ideal|| {ee:.4e}, ratio {ratios[n]:.3f}")
    record("qk_prologue_bwd processors: ||fused - ideal||_F / ||eager - ideal||_F",
           f"{label}: " + ", ".join(f"{n} {r:.3f}" for n, r in ratios.items()))
    return ratios


@pytest.mark.parametrize("kind", ["cog", "wan"])
def test_processor_gradients_against_the_eager_chain(kind):
    """cog 4x64 and wan 2x128, N=40, T=7, B=2, bf16. With grad enabled fused_qk + fused_qk_backward
    reports "fused" and fused_qk alone "eager"; every gradient of the fused path is as close to the
    fp64 stand-in's as the eager chain's on the same device, within a factor 1.5."""
    heads, hd = (4, 64) if kind == "cog" else (2, 128)
    dim, N, T, B = heads * hd, 40, 7, 2
    attn = StandInAttention(dim, heads, kind).to(DEV, BF16)
    hidden = randn(B, N, dim, seed=50)
    cos_sin, freqs = rope_tables(N, hd, seed=9)
    extra = {"text": randn(B, T, dim, seed=51), "rope": cos_sin, "freqs": freqs}
    upstream = randn(B, N, dim, seed=52)
    path_e, eager, _ = _proc_grads(kind, attn, dict(fused_qk=True), hidden, extra, upstream)
    path_f, fused, _ = _proc_grads(kind, attn, dict(fused_qk=True, fused_qk_backward=True), hidden, extra, upstream)
    path_n, _, _ = _proc_grads(kind, attn, dict(fused_qk_backward=True), hidden, extra, upstream)
    assert (path_e, path_f, path_n) == ("eager", "fused", "eager")
    attn.seen.clear()                                  # clones that carry autograd history: not copyable
    attn64 = copy.deepcopy(attn).double()
    extra64 = {"text": extra["text"].double(), "rope": cos_sin, "freqs": freqs}
    _, ideal, _ = _proc_grads(kind, attn64, dict(fused_qk=False), hidden.double(), extra64, upstream.double())
    for n in ideal:
        assert fused[n].dtype == eager[n].dtype == BF16
    ratios = _ratio_rule(kind, fused, eager, ideal)
    assert max(ratios.values()) <= 1.5, ratios


class _OracleInner(torch.autograd.Function):
    """The adaptive attention's CPU oracle (forward and backward) as the fp64 stand-in's inner attention."""

    @staticmethod
    def forward(ctx, q, k, v, mask, cfg):
        import bsa_oracle as O
        qc, kc, vc = (t.detach().cpu() for t in (q, k, v))
        fwd = O.adaptive_attention(qc, kc, vc, cfg, None, None, mask=mask.cpu().bool())
        ctx.saved = (qc, kc, vc, cfg, fwd)
        return fwd["out"].to(q.dtype).to(q.device)

    @staticmethod
    def backward(ctx, dout):
        import bsa_oracle as O
        qc, kc, vc, cfg, fwd = ctx.saved
        grads = O.adaptive_attention_bwd(qc, kc, vc, dout.cpu(), cfg, fwd)
        return (*(g.to(dout.dtype).to(dout.device) for g in grads), None, None)


def test_real_module_small_grid_backward():
    """Once through AdaptiveBlockSparseAttn on the 12x8x6 Gilbert grid + 26 text tokens (602 rows) with
    given sampling offsets, recording autograd: the fused-backward path's hidden_states gradient holds
    the ratio rule against the eager chain's (ideal: the fp64 stand-in around the adaptive attention's
    CPU oracle with the GPU's mask), and the masks are equal where the forward q/k are bit-equal."""
    import bsa_oracle as O
    import vblade
    from vblade import attention
    heads, hd, T = 2, 64, 26
    m = vblade.AdaptiveBlockSparseAttn("cog", width=12, height=8, depth=6, text_length=T, log_every=0)
    N = 12 * 8 * 6
    attn = StandInAttention(heads * hd, heads, "cog").to(DEV, BF16)
    g = torch.Generator(device=DEV).manual_seed(3)
    q_off, k_off = attention.draw_sample_offsets_qk(1, heads, DEV, generator=g)
    masks = []

    def inner(q, k, v):
        attn.seen.append((q.detach().clone(), k.detach().clone()))
        out = m(q, k, v, q_off=q_off, k_off=k_off)
        masks.append(m.last_mask.clone())
        return out

    attn.inner_attention = inner
    hidden = randn(1, N, heads * hd, seed=60)
    cos_sin, _ = rope_tables(N, hd, seed=11)
    extra = {"text": randn(1, T, heads * hd, seed=61), "rope": cos_sin}
    upstream = randn(1, N, heads * hd, seed=62)
    path_e, eager, seen_e = _proc_grads("cog", attn, dict(fused_qk=True), hidden, extra, upstream)
    path_f, fused, seen_f = _proc_grads("cog", attn, dict(fused_qk=True, fused_qk_backward=True), hidden, extra, upstream)
    assert (path_e, path_f) == ("eager", "fused")
    same = all(torch.equal(f, e) for f, e in zip(seen_f[0], seen_e[0]))
    record("qk_prologue_bwd real module: fused q/k bit-equal to eager", same)
    if same:
        assert torch.equal(masks[0], masks[1])
    attn.inner_attention = None
    attn.seen.clear()
    attn64 = copy.deepcopy(attn).double()
    cfg = O.AdaptiveConfig.cogvideox(width=12, height=8, depth=6, text_length=T)
    attn64.inner_attention = lambda q, k, v: _OracleInner.apply(q, k, v, masks[0], cfg)
    extra64 = {"text": extra["text"].double(), "rope": cos_sin}
    _, ideal, _ = _proc_grads("cog", attn64, dict(fused_qk=False), hidden.double(), extra64, upstream.double())
    ratios = _ratio_rule("real module", {"hidden_states": fused["hidden_states"]},
                         {"hidden_states": eager["hidden_states"]}, {"hidden_states": ideal["hidden_states"]})
    assert ratios["hidden_states"] <= 1.5
