"""GPU: the fused q/k prologue (vb_qk_prologue / ops.qk_prologue / the processors' fused_qk) against
the eager chains the processors of vblade/patch.py run on the same device.

What is derivable is asserted bit for bit: RoPE has no reduction and the kernel performs the eager
kernels' own fp32 / fp64 operations, so RoPE-only results equal the eager chain exactly. A norm
reduces, so its result is checked against an fp64 statement of the chain (written below) with

    |fused - ideal| <= 1/2 ulp(max(|ideal|, |fused|)) + 2^-18 * max_row |ideal|

(half a storage-dtype ulp of rounding plus fp32 evaluation slack; `row` is the norm's own reduction
row: a head's D values for the LayerNorm, the H*D token row for the RMSNorm), and the share of
elements that differ from the GPU's eager result must stay within 1e-3, for the norms alone and
for the q/k the processors hand on.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import record
from qk_standins import OtherLayerNorm, OtherRMSNorm, StandInAttention

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK = 2.0 ** -18


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def ulp(mag, dtype):
    """Spacing of `dtype` at magnitude `mag` (fp64 tensor): 2^(floor(log2 mag) - p), subnormals flat."""
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    return torch.exp2(torch.floor(torch.log2(mag.clamp_min(2.0 ** emin))) - p)


def norm_bound(got, ideal, row_max, dtype, slack=SLACK):
    """Worst |got - ideal| / bound over all elements (<= 1 passes)."""
    got = got.double()
    bound = 0.5 * ulp(torch.maximum(ideal.abs(), got.abs()), dtype) + slack * row_max
    return ((got - ideal).abs() / bound).max().item()


def ideal_layer_norm(x_blhd, w, b, eps):
    """fp64 LayerNorm over each head's D values; returns (ideal, max |ideal| per head row)."""
    x = x_blhd.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps)
    if w is not None:
        y = y * w.double()
    if b is not None:
        y = y + b.double()
    return y, y.abs().amax(-1, keepdim=True)


def ideal_rms_norm(x_blw, w, eps):
    """fp64 RMSNorm over the H*D row; returns (ideal, max |ideal| per row)."""
    x = x_blw.double()
    y = x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    if w is not None:
        y = y * w.double()
    return y, y.abs().amax(-1, keepdim=True)


def eager_rope_real(x_bhld, cos, sin, start):
    """The CogVideoX processor's slice assignment (patch.py, eager chain)."""
    from vblade import patch
    x = x_bhld.clone()
    x[:, :, start:] = patch._apply_rotary_emb_real(x[:, :, start:], (cos, sin))
    return x


def eager_rope_complex(hs, freqs):
    """The Wan processor's float64 complex product (patch.py, eager chain)."""
    x_rotated = torch.view_as_complex(hs.to(torch.float64).unflatten(3, (-1, 2)))
    return torch.view_as_real(x_rotated * freqs).flatten(3, 4).type_as(hs)


def rope_tables(S, hd, seed=3):
    g = torch.Generator().manual_seed(seed)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * 6.28
    ang2 = ang.repeat_interleave(2, -1)
    return ((ang2.cos().float().to(DEV), ang2.sin().float().to(DEV)),
            torch.polar(torch.ones_like(ang), ang)[None, None].to(DEV))


def randn(*shape, seed, dtype=torch.bfloat16, mean=0.2, std=1.3):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std + mean).to(DEV, dtype)


_MIXED_LN = []


def _mixed_layer_norm():
    """Does this torch build have a GPU LayerNorm for bf16 input with fp32 weight and bias?"""
    if not _MIXED_LN:
        x = torch.zeros(2, 64, device=DEV, dtype=torch.bfloat16)
        w = torch.ones(64, device=DEV)
        try:
            F.layer_norm(x, (64,), w, w, 1e-5)
            _MIXED_LN.append(True)
        except RuntimeError:
            _MIXED_LN.append(False)
    return _MIXED_LN[0]


def bhld(x_blw, H):
    B, L, W = x_blw.shape
    return x_blw.view(B, L, H, W // H).transpose(1, 2)


# ------------------------------------------------------------------------------------------------
# RoPE only: bit-equal to the eager chain
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_real_rope_is_bit_equal_to_eager(dtype):
    """B=2, H=3, D=64, L=82, rope_start=5: a boundary that is a multiple of nothing, text rows
    untouched bit for bit, inputs that are slices of a larger buffer (batch stride != L*H*D)."""
    from vblade import ops
    B, H, D, L, T = 2, 3, 64, 82, 5
    bigq, bigk = (randn(B, L + 7, H * D, seed=s, dtype=dtype) for s in (1, 2))
    xq, xk = bigq[:, 3:3 + L], bigk[:, 3:3 + L]
    assert not xq.is_contiguous()
    (cos, sin), _ = rope_tables(L - T, D)
    q, k = ops.qk_prologue(xq, xk, heads=H, rope="real", rope_start=T, cos=cos, sin=sin)
    assert q.shape == (B, H, L, D) and q.stride(2) == H * D      # the [B,H,L,D] view, no transpose copy
    for got, x in ((q, xq), (k, xk)):
        ref = eager_rope_real(bhld(x, H), cos, sin, T)
        assert torch.equal(got[:, :, :T], bhld(x, H)[:, :, :T])
        assert not torch.equal(got[:, :, T:], bhld(x, H)[:, :, T:])
        assert torch.equal(got, ref)
    # cross attention: k keeps its rows as they are
    q2, k2 = ops.qk_prologue(xq, xk, heads=H, rope=("real", "none"), rope_start=T, cos=cos, sin=sin)
    assert torch.equal(q2, q) and torch.equal(k2, bhld(xk, H))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_complex_rope_is_bit_equal_to_eager(dtype):
    """B=1, H=3, D=128, L=37 with complex128 and complex64 tables, each against its eager counterpart."""
    from vblade import ops
    B, H, D, L = 1, 3, 128, 37
    xq, xk = (randn(B, L, H * D, seed=s, dtype=dtype) for s in (3, 4))
    _, freqs = rope_tables(L, D)
    for fr in (freqs, freqs.to(torch.complex64)):
        q, k = ops.qk_prologue(xq, xk, heads=H, rope="complex", freqs=fr)
        assert torch.equal(q, eager_rope_complex(bhld(xq, H), fr))
        assert torch.equal(k, eager_rope_complex(bhld(xk, H), fr))


# ------------------------------------------------------------------------------------------------
# norm only: the fp64 bound, and the share of elements that differ from the GPU's eager norm
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("affine", ["bf16", "bf16-nobias", "fp32", "fp32-nobias", "none"])
@pytest.mark.parametrize("norm,H,D", [("layer", 48, 64), ("rms", 12, 128), ("layer", 12, 128), ("rms", 48, 64)])
def test_norm_within_half_ulp_of_fp64(norm, H, D, affine):
    from vblade import ops
    B, L, W, eps, dtype = 2, 9, H * D, 1e-5, torch.bfloat16
    x = randn(B, L, W, seed=10 + H)
    n = D if norm == "layer" else W
    g = torch.Generator().manual_seed(20 + D)
    wdt = torch.float32 if affine.startswith("fp32") else dtype
    w = None if affine == "none" else (1 + 0.1 * torch.randn(n, generator=g)).to(DEV, wdt)
    b = (0.1 * torch.randn(n, generator=g)).to(DEV, wdt) if affine in ("bf16", "fp32") and norm == "layer" else None
    got = ops.qk_prologue(x, heads=H, norm=norm, q_weight=w, q_bias=b, q_eps=eps)      # [B,H,L,D]
    if norm == "layer":
        ideal, row_max = ideal_layer_norm(x.view(B, L, H, D), w, b, eps)
        worst = norm_bound(got.transpose(1, 2), ideal, row_max, dtype)
    else:
        ideal, row_max = ideal_rms_norm(x, w, eps)
        worst = norm_bound(got.transpose(1, 2).reshape(B, L, W), ideal, row_max, dtype)
    # The GPU's eager norm on the same input: always for parameters of the storage dtype (the
    # processors' own case); for the LayerNorm with fp32 parameters where this torch build has that
    # kernel (an explicit probe); for the RMSNorm with an fp32 weight, which torch returns as fp32,
    # after one .to(dtype). The eager result's own ratio against the fp64 bound is printed beside it.
    mixed = wdt != dtype and w is not None
    eager = None
    if norm == "layer":
        if not mixed or _mixed_layer_norm():
            eager = F.layer_norm(bhld(x, H), (D,), w, b, eps).to(dtype)
    else:
        eager = bhld(F.rms_norm(x, (W,), w, eps).to(dtype), H)
    share = eager_worst = None
    if eager is not None:
        assert eager.shape == got.shape and eager.dtype == got.dtype
        share = (eager != got).float().mean().item()
        e_blhd = eager.transpose(1, 2)
        eager_worst = norm_bound(e_blhd if norm == "layer" else e_blhd.reshape(B, L, W), ideal, row_max, dtype)
    print(f"norm={norm} H={H} D={D} affine={affine}: worst |err|/bound {worst:.3f}, share != eager {share}, "
          f"eager's own |err|/bound {eager_worst}")
    record("qk_prologue norm: worst |err|/bound, share of elements != GPU eager",
           f"{norm} H={H} D={D} {affine}: {worst:.3f}, {share}")
    assert got.shape == (B, H, L, D) and got.dtype == dtype
    assert worst <= 1.0
    if eager is not None:
        assert share <= 1e-3


@pytest.mark.parametrize("H,D", [(48, 64), (12, 128)])
def test_layer_norm_eps_is_really_used(H, D):
    """Rows of 1.0 with about 10 % of the elements one bf16 step higher: the variance (up to 1.2e-5)
    is of the order of eps, so a dropped or misplaced eps is far outside the bound (the same formula
    with 32x the fp32 slack: the deviations x - mean themselves carry the mean's rounding)."""
    from vblade import ops
    B, L, eps = 1, 9, 1e-5
    g = torch.Generator().manual_seed(7)
    x = (1.0 + (torch.rand(B, L, H * D, generator=g) < 0.1) * 2.0 ** -7).to(DEV, torch.bfloat16)
    got = ops.qk_prologue(x, heads=H, norm="layer", q_eps=eps)
    ideal, row_max = ideal_layer_norm(x.view(B, L, H, D), None, None, eps)
    worst = norm_bound(got.transpose(1, 2), ideal, row_max, torch.bfloat16, slack=32 * SLACK)
    off = [norm_bound(got.transpose(1, 2), *ideal_layer_norm(x.view(B, L, H, D), None, None, e),
                      torch.bfloat16, slack=32 * SLACK) for e in (eps * 10, eps / 10)]
    print(f"eps test H={H} D={D}: worst |err|/bound {worst:.3f}; against eps x10, /10: {off}")
    assert worst <= 1.0
    assert min(off) > 10.0                     # the bound tells a tenfold eps apart
    other = ops.qk_prologue(x, heads=H, norm="layer", q_eps=1e-6)
    assert not torch.equal(other, got)


@pytest.mark.parametrize("H,D", [(48, 64), (12, 128)])
def test_rms_norm_eps_is_really_used(H, D):
    """Rows of N(0, 0.003^2): the mean square (about 1e-5) is of the order of eps, so a dropped or
    misplaced RMSNorm eps is far outside the plain bound (x itself enters exactly; only the fp32 sum
    of squares carries rounding, so no extra slack is needed)."""
    from vblade import ops
    B, L, W, eps = 1, 9, H * D, 1e-5
    x = randn(B, L, W, seed=70 + H, mean=0.0, std=0.003)
    g = torch.Generator().manual_seed(71)
    w = (1 + 0.1 * torch.randn(W, generator=g)).to(DEV, torch.bfloat16)
    got = ops.qk_prologue(x, heads=H, norm="rms", q_weight=w, q_eps=eps).transpose(1, 2).reshape(B, L, W)
    worst = norm_bound(got, *ideal_rms_norm(x, w, eps), torch.bfloat16)
    off = [norm_bound(got, *ideal_rms_norm(x, w, e), torch.bfloat16) for e in (eps * 10, eps / 10)]
    print(f"rms eps test H={H} D={D}: worst |err|/bound {worst:.3f}; against eps x10, /10: {off}")
    assert worst <= 1.0
    assert min(off) > 10.0
    other = ops.qk_prologue(x, heads=H, norm="rms", q_weight=w, q_eps=1e-6).transpose(1, 2).reshape(B, L, W)
    assert not torch.equal(other, got)


def test_no_row_takes_rope_when_rope_start_is_L():
    """rope_start == L (a call with no video rows; the tables are empty): the norm alone."""
    from vblade import ops
    B, L, H, D = 1, 7, 3, 64
    x = randn(B, L, H * D, seed=80)
    empty = torch.empty(0, D, device=DEV)
    got = ops.qk_prologue(x, heads=H, rope="real", rope_start=L, cos=empty, sin=empty)
    assert torch.equal(got, bhld(x, H))
    got = ops.qk_prologue(x, heads=H, norm="layer", rope="real", rope_start=L, cos=empty, sin=empty)
    assert torch.equal(got, ops.qk_prologue(x, heads=H, norm="layer"))


# ------------------------------------------------------------------------------------------------
# combined modes
# ------------------------------------------------------------------------------------------------
def _configs():
    (cos, sin), _ = rope_tables(40 - 6, 64, seed=5)
    _, freqs = rope_tables(23, 128, seed=6)
    g = torch.Generator().manual_seed(8)
    wl, bl = ((1 + 0.1 * torch.randn(64, generator=g)).to(DEV, torch.bfloat16),
              (0.1 * torch.randn(64, generator=g)).to(DEV, torch.bfloat16))
    wr = (1 + 0.1 * torch.randn(3 * 128, generator=g)).to(DEV, torch.bfloat16)
    return {
        "cog": (dict(B=2, L=40, H=5, D=64), dict(norm="layer", q_weight=wl, q_bias=bl, k_weight=bl + 1, k_bias=wl - 1),
                dict(rope="real", rope_start=6, cos=cos, sin=sin)),
        "wan": (dict(B=1, L=23, H=3, D=128), dict(norm="rms", q_weight=wr, k_weight=wr * wr, q_eps=1e-6),
                dict(rope="complex", freqs=freqs)),
    }


@pytest.mark.parametrize("name", ["cog", "wan"])
def test_combined_modes(name):
    """norm+rope in one call == rope(norm(x)) in two (the rounding point after the norm is real);
    in place == out of place; q alone == the q half of a q+k call."""
    from vblade import ops
    shape, norm_kw, rope_kw = _configs()[name]
    B, L, H, D = (shape[s] for s in "BLHD")
    xq, xk = (randn(B, L, H * D, seed=s) for s in (30, 31))
    q, k = ops.qk_prologue(xq, xk, heads=H, **norm_kw, **rope_kw)
    assert q.dtype == xq.dtype and q.shape == (B, H, L, D)
    nq, nk = ops.qk_prologue(xq, xk, heads=H, **norm_kw)
    unview = lambda t: t.transpose(1, 2).reshape(B, L, H * D)        # noqa: E731
    q2, k2 = ops.qk_prologue(unview(nq), unview(nk), heads=H, **rope_kw)
    assert torch.equal(q2, q) and torch.equal(k2, k)
    assert not torch.equal(nq, q)
    q_alone = ops.qk_prologue(xq, heads=H, **{a: v for a, v in norm_kw.items() if not a.startswith("k_")}, **rope_kw)
    assert torch.equal(q_alone, q)
    yq, yk = xq.clone(), xk.clone()
    qi, ki = ops.qk_prologue(yq, yk, heads=H, inplace=True, **norm_kw, **rope_kw)
    assert qi.data_ptr() == yq.data_ptr()
    assert torch.equal(qi, q) and torch.equal(ki, k)
    assert torch.equal(unview(q), yq)


def test_graph_capture_replays_bit_for_bit():
    """vb_qk_prologue on one stream inside torch.cuda.graph: the replay writes what the direct call
    writes."""
    from vblade import ops
    shape, norm_kw, rope_kw = _configs()["cog"]
    B, L, H, D = (shape[s] for s in "BLHD")
    xq, xk = (randn(B, L, H * D, seed=s) for s in (40, 41))
    q, k = ops.qk_prologue(xq, xk, heads=H, **norm_kw, **rope_kw)
    sq, sk = torch.zeros_like(xq), torch.zeros_like(xk)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.qk_prologue(sq, sk, heads=H, **norm_kw, **rope_kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gq, gk = ops.qk_prologue(sq, sk, heads=H, **norm_kw, **rope_kw)
    sq.copy_(xq)
    sk.copy_(xk)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(gq, q) and torch.equal(gk, k)


# ------------------------------------------------------------------------------------------------
# processors
# ------------------------------------------------------------------------------------------------
def _run(kind, attn, fused, hidden, extra, grad=False):
    from vblade import patch
    if kind == "cog":
        proc = patch.CogVideoXBlockSparseAttnProcessor(0, fused_qk=fused)
        call = lambda: proc(attn, hidden, extra["text"], image_rotary_emb=extra["rope"])[0]   # noqa: E731
    else:
        proc = patch.WanBlockSparseAttnProcessor(fused_qk=fused)
        call = lambda: proc(attn, hidden, extra.get("enc"), rotary_emb=extra["freqs"])        # noqa: E731
    attn.seen.clear()
    if grad:
        out = call()
    else:
        with torch.no_grad():
            out = call()
    return proc.last_path, out.detach(), list(attn.seen)


def _case(kind, i2v=False, norm_cls=None):
    heads, hd = (4, 64) if kind == "cog" else (2, 128)
    dim, N, T, B = heads * hd, 40, 7, 2
    attn = StandInAttention(dim, heads, kind, i2v=i2v, norm_cls=norm_cls).to(DEV, torch.bfloat16)
    hidden = randn(B, N, dim, seed=50, mean=0.0, std=1.0)
    cos_sin, freqs = rope_tables(N, hd, seed=9)
    extra = {"text": randn(B, T, dim, seed=51, mean=0.0, std=1.0), "rope": cos_sin, "freqs": freqs}
    if i2v:
        extra["enc"] = randn(B, 257 + N, dim, seed=52, mean=0.0, std=1.0)
    return attn, hidden, extra


@pytest.mark.parametrize("kind", ["cog", "wan"])
def test_processor_fused_path_matches_eager(kind):
    """fused_qk=True takes the fused path, and the q/k it hands inner_attention hold the norm tests'
    condition against the eager chain's: at most 1e-3 of the elements differ. Where one differs it is
    by what one storage ulp of a norm output can do to its own RoPE pair: with r the length of the
    eager pair (y0, y1) (the rotation keeps it, so |x| <= r for both norm outputs of the pair), the
    inputs move an output by at most ulp(r)(|cos| + |sin|) <= sqrt2 ulp(r), and the two roundings to
    the storage dtype (of the fused and of the eager output, both of magnitude <= r) add half an
    ulp(r) each: |diff| <= (sqrt2 + 1) ulp(r) < 2.5 ulp(r). r is taken 2^-7 larger, since the eager
    outputs it is computed from are themselves rounded."""
    attn, hidden, extra = _case(kind)
    path_e, out_e, seen_e = _run(kind, attn, False, hidden, extra)
    path_f, out_f, seen_f = _run(kind, attn, True, hidden, extra)
    assert (path_e, path_f) == ("eager", "fused")
    for name, f, e in zip("qk", seen_f[0], seen_e[0]):
        assert f.shape == e.shape and f.dtype == e.dtype
        share = (f != e).float().mean().item()
        pair = e.double().unflatten(-1, (-1, 2))
        r = pair.pow(2).sum(-1, keepdim=True).sqrt().expand_as(pair).flatten(-2) * (1 + 2.0 ** -7)
        worst = ((f.double() - e.double()).abs() / (2.5 * ulp(r, e.dtype))).max().item()
        print(f"{kind} processor {name}: share != eager {share:.2e}, worst |diff| / (2.5 ulp(r)) {worst:.3f}")
        record("qk_prologue processors: share of q/k elements != eager", f"{kind} {name}: {share:.2e}")
        assert share <= 1e-3
        assert worst <= 1.0
    torch.testing.assert_close(out_f, out_e, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("kind,why", [("cog", "norm"), ("wan", "norm"), ("cog", "grad"), ("wan", "grad"), ("wan", "i2v")])
def test_processor_keeps_the_eager_chain_when_it_must(kind, why):
    """An unknown norm class, autograd recording and the Wan I2V branch report "eager" and return
    the bits fused_qk=False returns."""
    other = {"cog": OtherLayerNorm, "wan": OtherRMSNorm}[kind]
    attn, hidden, extra = _case(kind, i2v=why == "i2v", norm_cls=other if why == "norm" else None)
    grad = why == "grad"
    path_e, out_e, seen_e = _run(kind, attn, False, hidden, extra, grad=grad)
    path_f, out_f, seen_f = _run(kind, attn, True, hidden, extra, grad=grad)
    assert (path_e, path_f) == ("eager", "eager")
    assert torch.equal(out_f, out_e)
    for f, e in zip(seen_f, seen_e):
        assert torch.equal(f[0], e[0]) and torch.equal(f[1], e[1])


def test_real_module_small_grid():
    """Once through AdaptiveBlockSparseAttn on the 12x8x6 Gilbert grid + 26 text tokens of the module
    tests (602 rows: five blocks, the last one partial; D=64, H=2) with given sampling offsets: where the fused q and k equal the eager ones bit for bit, so do the mask
    and the output; otherwise the output holds the module tests' tolerance (PSNR >= 40 dB)."""
    import math
    import vblade
    from vblade import attention
    heads, hd, T = 2, 64, 26
    m = vblade.AdaptiveBlockSparseAttn("cog", width=12, height=8, depth=6, text_length=T, log_every=0)
    N = 12 * 8 * 6
    attn = StandInAttention(heads * hd, heads, "cog").to(DEV, torch.bfloat16)
    g = torch.Generator(device=DEV).manual_seed(3)
    q_off, k_off = attention.draw_sample_offsets_qk(1, heads, DEV, generator=g)
    masks = []

    def inner(q, k, v):
        attn.seen.append((q.clone(), k.clone()))
        out = m(q, k, v, q_off=q_off, k_off=k_off)
        masks.append(m.last_mask.clone())
        return out

    attn.inner_attention = inner
    hidden = randn(1, N, heads * hd, seed=60, mean=0.0, std=1.0)
    cos_sin, _ = rope_tables(N, hd, seed=11)
    extra = {"text": randn(1, T, heads * hd, seed=61, mean=0.0, std=1.0), "rope": cos_sin}
    path_e, out_e, seen_e = _run("cog", attn, False, hidden, extra)
    path_f, out_f, seen_f = _run("cog", attn, True, hidden, extra)
    assert (path_e, path_f) == ("eager", "fused")
    same = all(torch.equal(f, e) for f, e in zip(seen_f[0], seen_e[0]))
    record("qk_prologue real module: fused q/k bit-equal to eager", same)
    if same:
        assert torch.equal(masks[0], masks[1]) and torch.equal(out_f, out_e)
    else:
        mse = torch.mean((out_f.double() - out_e.double()) ** 2).item()
        peak = out_e.double().abs().max().item()
        assert mse == 0 or 10 * math.log10(peak * peak / mse) >= 40
