"""GPU: projection-layout I/O ([B,L,H,D] memory behind the [B,H,L,D] tensors) changes where bytes
land and nothing else. Every comparison below is bit for bit against the default (contiguous) path of
the same build on the same inputs:

  * forward ops: out_layout="blhd" writes the same values, and the caller's transpose + reshape to
    [B,L,H*D] is a view of them;
  * sentinel: out (and dq/dk/dv) as views into a wider [B,L,H*D+64] buffer leave every padding
    element untouched, so no store runs past a row;
  * vb_lse_combine_strided against vb_lse_combine on contiguous copies, with rows whose weight rounds
    to exactly 1 and a row with lse2 = -inf;
  * the autograd functions, both modules, both processors and the stand-in training block.

Shapes: B=2, H=3, L=300 (three blocks, a 44-row tail) and one case at L=129 (a 1-row tail), D 64 and
128, bf16 and fp16, a random row permutation, a 0.4-density block mask with no empty row, gap 7
(pooled keys straddle block edges: 128 = 18*7 + 2)."""
import functools
import math

import pytest
import torch
import torch.nn as nn

import bsa_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H, L, GAP = 2, 3, 300, 7
CASES = [(64, torch.bfloat16), (64, torch.float16), (128, torch.bfloat16), (128, torch.float16)]
IDS = ["d64-bf16", "d64-fp16", "d128-bf16", "d128-fp16"]
SENTINEL = 0x5A5A
GEOM = {"cog": dict(width=12, height=8, depth=6, text_length=26),    # L = 602, D = 64, forced tail
        "wan": dict(width=13, height=6, depth=7)}                    # L = 546, D = 128
HEAD = {"cog": (64, torch.bfloat16), "wan": (128, torch.float16)}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _ops():
    from vblade import ops
    return ops


def _blhd_strides(t):
    b, h, l, d = t.shape
    return t.stride() == (l * h * d, d, h * d, 1)


def _assert_projection_view(t):
    """transpose + reshape to [B,L,H*D] is a view of t: same pointer, same storage, nothing allocated."""
    b, h, l, d = t.shape
    before = torch.cuda.memory_allocated()
    flat = t.transpose(1, 2).reshape(b, l, h * d)
    assert torch.cuda.memory_allocated() == before
    assert flat.data_ptr() == t.data_ptr() and flat.is_contiguous()
    assert flat.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def _problem(D, dtype, Lq=L):
    """Inputs (q, k, v, dO as views of projection-layout memory), the row permutation, the block mask,
    the pooled keys and the default path's forward results. Computed once per case and never modified."""
    ops = _ops()
    pr = Problem()
    g = torch.Generator().manual_seed(1000 + D + Lq)
    proj = lambda: (torch.randn(B, Lq, H * D, generator=g).to(dtype).to(DEV).view(B, Lq, H, D).transpose(1, 2))  # noqa: E731
    pr.q, pr.k, pr.v, pr.do = proj(), proj(), proj(), proj()
    assert _blhd_strides(pr.do) and not pr.do.is_contiguous()
    pr.rows = torch.randperm(Lq, generator=g).int().to(DEV)
    nb = (Lq + 127) // 128
    pr.mask = O.block_mask_from_density(B, H, nb, nb, 0.4, seed=D + Lq).to(DEV)
    assert pr.mask.any(-1).all()
    pr.bias = float(torch.log(torch.tensor(float(GAP), dtype=dtype)).item())
    pr.kp, pr.vp, pr.k_r, pr.v_r = ops.pool_kv(pr.k, pr.v, GAP, pr.rows, reordered=True)
    pr.fwd = {
        "fused": dict(args=(pr.q, pr.k_r, pr.v_r), kw=dict(block_mask=pr.mask, q_rows=pr.rows, kp=pr.kp, vp=pr.vp,
                                                           kp_log_bias=pr.bias, heavy_rows=2)),
        "fused_lse": dict(args=(pr.q, pr.k_r, pr.v_r), kw=dict(block_mask=pr.mask, q_rows=pr.rows, kp=pr.kp, vp=pr.vp,
                                                               kp_log_bias=pr.bias, need_lse=True)),
        "need_lse": dict(args=(pr.q, pr.k_r, pr.v_r), kw=dict(block_mask=pr.mask, q_rows=pr.rows, need_lse=True)),
        "pooled_only": dict(args=(pr.q, None, None), kw=dict(use_main=False, q_rows=pr.rows, kp=pr.kp, vp=pr.vp,
                                                            need_lse=True)),
    }
    for c in pr.fwd.values():
        c["want"] = ops.attention_fwd(*c["args"], **c["kw"])
    return pr


def _levels(nb, seed):
    """A random level mask (1, 2, 4, 8 and skips), the last column level 1 so no row is empty."""
    g = torch.Generator().manual_seed(seed)
    lv = torch.tensor([1, 2, 4, 8, 0], dtype=torch.uint8)
    m = lv[torch.randint(0, 5, (B, H, nb, nb), generator=g)]
    m[..., -1] = 1
    return m.to(DEV)


# ----------------------------------------------------------------------------------------------
# forward ops
# ----------------------------------------------------------------------------------------------
def _check_forward(pr):
    ops = _ops()
    for name, c in pr.fwd.items():
        got = ops.attention_fwd(*c["args"], **c["kw"], out_layout="blhd")
        want = c["want"]
        if c["kw"].get("need_lse"):
            assert torch.equal(got[1], want[1]), f"{name}: lse"
            got, want = got[0], want[0]
        assert want.is_contiguous() and _blhd_strides(got), name
        assert torch.isfinite(want.float()).all(), name
        assert torch.equal(got, want), name
        _assert_projection_view(got)


@pytest.mark.parametrize("D,dtype", CASES, ids=IDS)
def test_attention_fwd_projection_layout_output_is_the_default_output(D, dtype):
    _check_forward(_problem(D, dtype))


def test_attention_fwd_projection_layout_one_row_tail():
    _check_forward(_problem(64, torch.bfloat16, 129))
    _check_forward(_problem(128, torch.float16, 129))


@pytest.mark.parametrize("D,dtype", CASES, ids=IDS)
def test_ml_attention_fwd_projection_layout_output_is_the_default_output(D, dtype):
    ops = _ops()
    pr = _problem(D, dtype)
    kpyr, vpyr = ops.kv_pyramid(pr.k, pr.v, pr.rows)
    mask = _levels(3, seed=D)
    want, lse = ops.ml_attention_fwd(pr.q, kpyr, vpyr, mask, q_rows=pr.rows, want_lse=True)
    got, lse2 = ops.ml_attention_fwd(pr.q, kpyr, vpyr, mask, q_rows=pr.rows, want_lse=True, out_layout="blhd")
    assert want.is_contiguous() and _blhd_strides(got)
    assert torch.equal(got, want) and torch.equal(lse, lse2)
    _assert_projection_view(got)


# ----------------------------------------------------------------------------------------------
# sentinel: views into a wider buffer
# ----------------------------------------------------------------------------------------------
def _padded(Lr, D, dtype):
    """(buffer [B,Lr,H*D+64] prefilled with SENTINEL, its [B,H,Lr,D] view over the first H*D columns)."""
    buf = torch.empty(B, Lr, H * D + 64, device=DEV, dtype=dtype)
    buf.view(torch.int16).fill_(SENTINEL)
    view = buf[:, :, :H * D].unflatten(2, (H, D)).transpose(1, 2)
    assert view.shape == (B, H, Lr, D) and view.stride() == (Lr * (H * D + 64), D, H * D + 64, 1)
    return buf, view


def _padding_untouched(buf, D):
    return bool((buf[:, :, H * D:].contiguous().view(torch.int16) == SENTINEL).all())


@pytest.mark.parametrize("D,dtype", CASES, ids=IDS)
def test_forward_into_a_wider_buffer_leaves_the_padding(D, dtype):
    ops = _ops()
    pr = _problem(D, dtype)
    for name in ("fused", "pooled_only"):
        c = pr.fwd[name]
        buf, view = _padded(L, D, dtype)
        got = ops.attention_fwd(*c["args"], **c["kw"], out=view)
        got = got[0] if c["kw"].get("need_lse") else got
        want = c["want"][0] if c["kw"].get("need_lse") else c["want"]
        assert got.data_ptr() == view.data_ptr()
        assert torch.equal(view, want), name
        assert _padding_untouched(buf, D), name
    kpyr, vpyr = ops.kv_pyramid(pr.k, pr.v, pr.rows)
    mask = _levels(3, seed=D)
    buf, view = _padded(L, D, dtype)
    ops.ml_attention_fwd(pr.q, kpyr, vpyr, mask, q_rows=pr.rows, out=view)
    assert torch.equal(view, ops.ml_attention_fwd(pr.q, kpyr, vpyr, mask, q_rows=pr.rows))
    assert _padding_untouched(buf, D)


@pytest.mark.parametrize("D,dtype", CASES, ids=IDS)
def test_backward_into_wider_buffers_leaves_the_padding(D, dtype):
    """dq/dk/dv of the joint, the two-branch and the multi-level backward as views into wider buffers:
    the default call's bits inside, the sentinel outside."""
    ops = _ops()
    pr = _problem(D, dtype)
    out, lse = pr.fwd["fused_lse"]["want"]
    kw = dict(block_mask=pr.mask, q_rows=pr.rows, kv_rows=pr.rows, kp=pr.kp, vp=pr.vp, gap=GAP, heavy_rows=2)
    out1, lse1 = pr.fwd["need_lse"]["want"]
    out2, lse2 = pr.fwd["pooled_only"]["want"]
    _, alpha = ops.lse_combine(out1, lse1, out2, lse2, GAP)
    kpyr, vpyr = ops.kv_pyramid(pr.k, pr.v, pr.rows)
    lmask = _levels(3, seed=D)
    mout, mlse = ops.ml_attention_fwd(pr.q, kpyr, vpyr, lmask, q_rows=pr.rows, want_lse=True)
    calls = {
        "joint": lambda **g: ops.attention_bwd_joint(pr.do, pr.q, pr.k_r, pr.v_r, out, lse, kp_log_bias=pr.bias,
                                                     **kw, **g),
        "split": lambda **g: ops.attention_bwd(pr.do, pr.q, pr.k_r, pr.v_r, out1, lse1, out2=out2, lse2=lse2,
                                               alpha=alpha, **kw, **g),
        "multilevel": lambda **g: ops.ml_attention_bwd(pr.do, pr.q, kpyr, vpyr, lmask, mout, mlse, rows=pr.rows, **g),
    }
    for name, call in calls.items():
        want = call()
        bufs, views = zip(*(_padded(L, D, dtype) for _ in range(3)))
        got = call(grads=views)
        for n, g, w, buf in zip(("dq", "dk", "dv"), got, want, bufs):
            assert w.is_contiguous() and torch.isfinite(w.float()).all(), f"{name} {n}"
            assert torch.equal(g, w), f"{name} {n}"
            assert _padding_untouched(buf, D), f"{name} {n}"
        # and allocated by the op: projection-layout memory, the same bits
        for n, g, w in zip(("dq", "dk", "dv"), call(grad_layout="blhd"), want):
            assert _blhd_strides(g) and torch.equal(g, w), f"{name} {n} blhd"
            _assert_projection_view(g)


# ----------------------------------------------------------------------------------------------
# vb_lse_combine_strided
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", CASES, ids=IDS)
def test_strided_lse_combine_is_the_contiguous_entry_bit_for_bit(D, dtype):
    ops = _ops()
    g = torch.Generator().manual_seed(7 + D)
    blhd = lambda: torch.randn(B, L, H, D, generator=g).to(dtype).to(DEV).transpose(1, 2)  # noqa: E731
    out1, out2 = blhd(), blhd()
    lse1 = 3 * torch.randn(B, H, L, generator=g)
    lse2 = lse1 + 2 * torch.randn(B, H, L, generator=g) - math.log(GAP)
    lse2[:, :, 10:20] = lse1[:, :, 10:20] - 40.0      # the pooled branch far below: alpha rounds to exactly 1
    lse2[:, :, 20:30] = lse1[:, :, 20:30] + 200.0     # and so far above that exp underflows: alpha is 0
    lse2[0, 1, 7] = float("-inf")                     # a query with no pooled mass
    lse1, lse2 = lse1.to(DEV), lse2.to(DEV)
    want, walpha = ops.lse_combine(out1.contiguous(), lse1, out2.contiguous(), lse2, GAP)
    assert (walpha[:, :, 10:20] == 1).all() and walpha[0, 1, 7] == 1 and (walpha[:, :, 20:30] == 0).all()
    assert ((walpha > 0) & (walpha < 1)).any() and torch.isfinite(want.float()).all()
    # projection-layout inputs and output
    got, alpha = ops.lse_combine(out1, lse1, out2, lse2, GAP, out_layout="blhd")
    assert _blhd_strides(got) and torch.equal(got, want) and torch.equal(alpha, walpha)
    # projection-layout inputs, contiguous output; contiguous inputs, projection-layout output
    got, alpha = ops.lse_combine(out1, lse1, out2, lse2, GAP)
    assert got.is_contiguous() and torch.equal(got, want) and torch.equal(alpha, walpha)
    got, alpha = ops.lse_combine(out1.contiguous(), lse1, out2, lse2, GAP, out_layout="blhd")
    assert _blhd_strides(got) and torch.equal(got, want) and torch.equal(alpha, walpha)
    # into a wider buffer: nothing past a row
    buf, view = _padded(L, D, dtype)
    got, alpha = ops.lse_combine(out1, lse1, out2, lse2, GAP, out=view)
    assert got.data_ptr() == view.data_ptr() and torch.equal(view, want) and torch.equal(alpha, walpha)
    assert _padding_untouched(buf, D)


def test_strided_lse_combine_one_row_tail_and_refusal():
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    for Lr in (1, 129):
        out1, out2 = (torch.randn(B, Lr, H, 64, generator=g).bfloat16().to(DEV).transpose(1, 2) for _ in range(2))
        lse1, lse2 = (torch.randn(B, H, Lr, generator=g).to(DEV) for _ in range(2))
        want, walpha = ops.lse_combine(out1.contiguous(), lse1, out2.contiguous(), lse2, GAP)
        got, alpha = ops.lse_combine(out1, lse1, out2, lse2, GAP, out_layout="blhd")
        assert torch.equal(got, want) and torch.equal(alpha, walpha)
    with pytest.raises(ValueError, match="overlap"):
        ops.lse_combine(out1, lse1, out2, lse2, GAP, out=out1)


# ----------------------------------------------------------------------------------------------
# autograd functions
# ----------------------------------------------------------------------------------------------
def _grads(fn, pr):
    q, k, v = (t.detach().requires_grad_(True) for t in (pr.q, pr.k, pr.v))
    out = fn(q, k, v)
    return out.detach(), torch.autograd.grad(out, (q, k, v), pr.do)


def _check_autograd(pr, fn):
    """fn(io_layout) -> a function of (q, k, v). The upstream gradient pr.do is a transposed view of a
    [B,L,H*D] tensor in both runs."""
    want, wg = _grads(fn("bhld"), pr)
    got, gg = _grads(fn("blhd"), pr)
    assert want.is_contiguous() and _blhd_strides(got)
    assert torch.isfinite(want.float()).all() and torch.equal(got, want)
    _assert_projection_view(got)
    for n, g, w in zip(("dq", "dk", "dv"), gg, wg):
        assert torch.isfinite(w.float()).all() and w.float().abs().max() > 0, n
        assert torch.equal(g, w), n
        assert _blhd_strides(g), f"{n} strides {g.stride()}"


@pytest.mark.parametrize("D,dtype", CASES, ids=IDS)
def test_autograd_functions_projection_layout_gradients_are_the_default_gradients(D, dtype):
    from vblade import autograd, multilevel
    pr = _problem(D, dtype)
    _check_autograd(pr, lambda lay: lambda q, k, v: autograd.adaptive_split_attention(
        q, k, v, pr.mask, pr.rows, GAP, heavy_rows=2, io_layout=lay))
    _check_autograd(pr, lambda lay: lambda q, k, v: autograd.adaptive_joint_attention(
        q, k, v, pr.mask, pr.rows, GAP, pr.bias, heavy_rows=2, io_layout=lay))
    lmask = _levels(3, seed=D)
    _check_autograd(pr, lambda lay: lambda q, k, v: multilevel._SparseAttention.apply(
        q, k, v, lmask, D ** -0.5, True, pr.rows, lay))


# ----------------------------------------------------------------------------------------------
# modules
# ----------------------------------------------------------------------------------------------
def _module(variant, **kw):
    import vblade
    return vblade.AdaptiveBlockSparseAttn(variant, sample_gap=GAP, min_retain_ratio=0.2, max_retain_ratio=0.5,
                                          log_every=0, **GEOM[variant], **kw).to(DEV)


@functools.lru_cache(maxsize=None)
def _module_inputs(variant):
    D, dtype = HEAD[variant]
    Lm = _module(variant).gilbert_rearranger.seq_len
    g = torch.Generator().manual_seed(50 + D)
    proj = lambda: torch.randn(2, Lm, 2 * D, generator=g).to(dtype).to(DEV).view(2, Lm, 2, D).transpose(1, 2)  # noqa: E731
    q, k, v, do = proj(), proj(), proj(), proj()
    off = lambda: torch.stack([torch.randperm(128, generator=g)[:32] for _ in range(4)]).view(2, 2, 32).int().to(DEV)  # noqa: E731
    return q, k, v, do, dict(q_off=off(), k_off=off())


def _module_run(m, variant, grad):
    q, k, v, do, off = _module_inputs(variant)
    if not grad:
        with torch.no_grad():
            return m(q, k, v, **off), None
    q, k, v = (t.detach().requires_grad_(True) for t in (q, k, v))
    out = m(q, k, v, **off)
    return out.detach(), torch.autograd.grad(out, (q, k, v), do)


@pytest.mark.parametrize("variant", ["cog", "wan"])
@pytest.mark.parametrize("mode", ["inference", "reference", "joint"])
def test_adaptive_module_projection_layout_changes_no_bit(variant, mode):
    kw = dict(probe="fidelity", probe_samples=8)
    if mode != "inference":
        kw["grad_combine"] = mode
    base, proj = _module(variant, **kw), _module(variant, io_layout="blhd", **kw)
    want, wg = _module_run(base, variant, mode != "inference")
    got, gg = _module_run(proj, variant, mode != "inference")
    assert want.is_contiguous() and _blhd_strides(got)
    assert torch.isfinite(want.float()).all() and torch.equal(got, want)
    _assert_projection_view(got)
    assert torch.equal(base.last_mask, proj.last_mask)
    for name in ("last_fidelity_err", "last_fidelity_sig", "last_fidelity_peak"):
        assert torch.equal(getattr(base, name), getattr(proj, name)), name
    assert torch.equal(base.fidelity, proj.fidelity)
    if wg is not None:
        for n, g, w in zip(("dq", "dk", "dv"), gg, wg):
            assert w.float().abs().max() > 0 and torch.equal(g, w), n
            assert _blhd_strides(g), n


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_adaptive_module_projection_layout_given_mask_and_drawn_offsets(variant):
    """The block_mask= path, and the module's own draws: the same generator state gives the same offsets,
    so the random stream is the default's."""
    q, k, v, _, _ = _module_inputs(variant)
    base, proj = _module(variant), _module(variant, io_layout="blhd")
    nb = (q.shape[2] + 127) // 128
    given = O.block_mask_from_density(2, 2, nb, nb, 0.4, seed=9).to(DEV)
    with torch.no_grad():
        assert torch.equal(proj(q, k, v, block_mask=given), base(q, k, v, block_mask=given))
        torch.manual_seed(11)
        want = base(q, k, v)
        state = torch.cuda.get_rng_state()
        torch.manual_seed(11)
        got = proj(q, k, v)
        assert torch.equal(torch.cuda.get_rng_state(), state)
    assert torch.equal(got, want) and torch.equal(base.last_mask, proj.last_mask) and _blhd_strides(got)


@pytest.mark.parametrize("grad", [False, True], ids=["inference", "autograd"])
def test_multilevel_module_projection_layout_changes_no_bit(grad):
    from vblade import multilevel
    q, k, v, do, off = _module_inputs("cog")
    kw = dict(log_every=0, probe="fidelity", probe_samples=8, **GEOM["cog"])
    base = multilevel.AdaptiveBlockSparseAttnTrain(**kw).to(DEV)
    proj = multilevel.AdaptiveBlockSparseAttnTrain(io_layout="blhd", **kw).to(DEV)
    res = []
    for m in (base, proj):
        if grad:
            a, b, c = (t.detach().requires_grad_(True) for t in (q, k, v))
            out = m(a, b, c, **off)
            res.append((out.detach(), torch.autograd.grad(out, (a, b, c), do)))
        else:
            with torch.no_grad():
                res.append((m(q, k, v, **off), ()))
    (want, wg), (got, gg) = res
    assert want.is_contiguous() and _blhd_strides(got) and torch.equal(got, want)
    assert torch.equal(base.last_mask, proj.last_mask)
    assert torch.equal(base.last_fidelity_err, proj.last_fidelity_err)
    assert torch.equal(base.last_fidelity_sig, proj.last_fidelity_sig)
    for n, g, w in zip(("dq", "dk", "dv"), gg, wg):
        assert w.float().abs().max() > 0 and torch.equal(g, w) and _blhd_strides(g), n


# ----------------------------------------------------------------------------------------------
# processors and the stand-in training block
# ----------------------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, attn):
        super().__init__()
        self.attn1 = attn


class _Model(nn.Module):
    def __init__(self, attn):
        super().__init__()
        self.transformer_blocks = nn.ModuleList([_Block(attn)])
        self.blocks = self.transformer_blocks


@pytest.mark.parametrize("fused_qk", [False, True], ids=["eager_qk", "fused_qk"])
@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_processors_projection_layout_output_is_the_default_output(variant, fused_qk):
    import vblade
    from qk_standins import StandInAttention
    D, dtype = HEAD[variant]
    heads, text = 2, GEOM[variant].get("text_length", 0)
    Lm = _module(variant).gilbert_rearranger.seq_len
    g = torch.Generator().manual_seed(21)
    hidden = torch.randn(2, Lm - text, heads * D, generator=g).to(dtype).to(DEV)
    enc = torch.randn(2, text, heads * D, generator=g).to(dtype).to(DEV)
    setter = vblade.set_block_sparse_attn_cogvideox if variant == "cog" else vblade.set_adaptive_block_sparse_attn_wanx
    res = {}
    for flag in (False, True):
        attn = StandInAttention(heads * D, heads, variant).to(DEV, dtype)
        model = _Model(attn)
        inner = setter(model, projection_layout=flag, fused_qk=fused_qk, sample_gap=GAP, min_retain_ratio=0.2,
                       max_retain_ratio=0.5, log_every=0, **GEOM[variant]).to(DEV)
        assert inner.io_layout == ("blhd" if flag else "bhld")
        proc = attn.processor
        torch.manual_seed(5)      # the module draws its sampling offsets from the device generator
        with torch.no_grad():
            out = proc(attn, hidden, enc) if variant == "cog" else proc(attn, hidden)
        out = out[0] if variant == "cog" else out
        assert proc.last_path == ("fused" if fused_qk else "eager")
        assert proc.last_out_is_view is flag
        res[flag] = (out, inner.last_mask)
    assert torch.isfinite(res[False][0].float()).all()
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])


@pytest.mark.parametrize("grad_combine", ["reference", "joint"])
def test_stand_in_block_projection_layout_loss_and_lora_gradients(grad_combine):
    from vblade import train
    D, dtype = HEAD["cog"]
    heads = 2
    Lm = _module("cog").gilbert_rearranger.seq_len
    g = torch.Generator().manual_seed(31)
    x = torch.randn(1, Lm, heads * D, generator=g).to(dtype).to(DEV)
    target = torch.randn(1, Lm, heads * D, generator=g).to(dtype).to(DEV)
    res = {}
    for flag in (False, True):
        inner = _module("cog", grad_combine=grad_combine, **(dict(io_layout="blhd") if flag else {}))
        model = train.StandInTransformer(1, heads * D, heads, 4, 4.0, inner, gradient_checkpointing=False,
                                         dtype=dtype, device=DEV, seed=2, projection_layout=flag)
        with torch.no_grad():     # LoRA B starts at zero, which would leave every A gradient zero
            gb = torch.Generator().manual_seed(4)
            for n, p in model.named_parameters():
                if n.endswith("lora_B"):
                    p.copy_(0.05 * torch.randn(p.shape, generator=gb))
        torch.manual_seed(6)
        loss = train.pseudo_huber(model(x), target, 1e-3)
        loss.backward()
        res[flag] = (loss.detach(), {n: p.grad for n, p in model.named_parameters() if p.requires_grad})
    assert torch.isfinite(res[False][0]) and torch.equal(res[True][0], res[False][0])
    assert len(res[False][1]) == 8
    for n, w in res[False][1].items():
        assert w is not None and w.abs().max() > 0, n
        assert torch.equal(res[True][1][n], w), n
