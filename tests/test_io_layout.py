"""CPU: the projection-layout option's surface. The library exports vb_lse_combine_strided beside an
unchanged ABI version and refuses bad calls on the host, before any launch (the fake pointers below
are never dereferenced); both modules, both setters and the stand-in blocks take the option."""
import ctypes

import pytest
import torch
import torch.nn as nn

import vblade
from vblade import _lib, ops, patch, train

_PTR = 1 << 20
_B, _H, _L, _D = 2, 3, 300, 64


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _s3(*v):
    return (ctypes.c_int64 * 3)(*v)


def _blhd(L=_L, H=_H, D=_D):
    return _s3(L * H * D, D, H * D)


def _combine_args(**kw):
    """A call the host checks accept: projection-layout out1/out, contiguous out2."""
    a = dict(out1=_PTR, out1_stride=_blhd(), lse1=_PTR, out2=2 * _PTR, out2_stride=_s3(_H * _L * _D, _L * _D, _D),
             lse2=_PTR, B=_B, H=_H, L=_L, D=_D, gap=7.0, dtype=_lib.VB_DTYPE_BF16, out=3 * _PTR,
             out_stride=_blhd(), alpha=_PTR, stream=None)
    a.update(kw)
    return a


_ORDER = ("out1", "out1_stride", "lse1", "out2", "out2_stride", "lse2", "B", "H", "L", "D", "gap", "dtype", "out",
          "out_stride", "alpha", "stream")


def _call(lib, **kw):
    a = _combine_args(**kw)
    rc = lib.vb_lse_combine_strided(*(a[n] for n in _ORDER))
    return rc, lib.vb_last_error().decode()


def test_strided_combine_is_exported_and_bound_and_the_abi_version_stays(lib):
    assert hasattr(lib, "vb_lse_combine_strided")
    assert "vb_lse_combine_strided" in _lib.SIGNATURES
    restype, argtypes = _lib.SIGNATURES["vb_lse_combine_strided"]
    assert restype is ctypes.c_int and len(argtypes) == len(_ORDER)
    assert lib.vb_abi_version() == _lib.ABI_VERSION == 4


@pytest.mark.parametrize("fault,kw,message", [
    ("null out1", dict(out1=None), "null argument"),
    ("null out", dict(out=None), "null argument"),
    ("null lse2", dict(lse2=None), "null argument"),
    ("null out_stride", dict(out_stride=None), "null argument"),
    ("D=96", dict(D=96), "bad sizes"),
    ("L=0", dict(L=0), "bad sizes"),
    ("H past a grid dimension", dict(H=65536), "bad sizes"),
    ("dtype 7", dict(dtype=7), "unknown dtype"),
    ("stride of 4", dict(out_stride=_s3(_L * _H * _D, _D, 4)), "multiples of 8"),
    ("input stride of 4", dict(out1_stride=_s3(4, 4, 4)), "multiples of 8"),
    ("negative stride", dict(out2_stride=_s3(_H * _L * _D, _L * _D, -_D)), "non-negative"),
    ("zero out stride", dict(out_stride=_s3(_L * _H * _D, 0, _H * _D)), "distinct"),
    ("misaligned base", dict(out=3 * _PTR + 8), "16-byte aligned"),
    ("misaligned input", dict(out2=2 * _PTR + 2), "16-byte aligned"),
    ("out is out1", dict(out=_PTR), "overlap"),
], ids=lambda v: v.replace(" ", "_") if isinstance(v, str) and len(v) < 28 else None)
def test_strided_combine_refuses_before_any_launch(lib, fault, kw, message):
    rc, err = _call(lib, **kw)
    print(f"{fault}: {rc} {err!r}")
    assert rc == _lib.VB_ERR_INVALID
    assert err.startswith("vb_lse_combine_strided:") and message in err


def test_layout_names_are_checked_by_every_wrapper():
    with pytest.raises(ValueError, match="out_layout"):
        ops.attention_fwd(None, None, None, out_layout="hbld")
    with pytest.raises(ValueError, match="out_layout"):
        ops.ml_attention_fwd(None, None, None, None, out_layout="hbld")
    with pytest.raises(ValueError, match="out_layout"):
        ops.lse_combine(None, None, None, None, 7, out_layout="hbld")
    with pytest.raises(ValueError, match="grad_layout"):
        ops.attention_bwd(*[None] * 6, grad_layout="hbld")
    with pytest.raises(ValueError, match="grad_layout"):
        ops.ml_attention_bwd(*[None] * 7, grad_layout="hbld")
    t = ops._empty_bhld(2, 3, 5, 8, "cpu", torch.bfloat16, "blhd")
    assert t.shape == (2, 3, 5, 8) and t.stride() == (120, 8, 24, 1)
    assert t.transpose(1, 2).reshape(2, 5, 24).data_ptr() == t.data_ptr()
    assert ops._empty_bhld(2, 3, 5, 8, "cpu", torch.bfloat16).is_contiguous()


def test_modules_take_io_layout():
    geom = dict(width=12, height=8, depth=6, text_length=26)
    assert vblade.AdaptiveBlockSparseAttn("cog", **geom).io_layout == "bhld"
    for variant in ("cog", "wan"):
        assert vblade.AdaptiveBlockSparseAttn(variant, io_layout="blhd", **geom).io_layout == "blhd"
        with pytest.raises(ValueError, match="io_layout"):
            vblade.AdaptiveBlockSparseAttn(variant, io_layout="hbld", **geom)
    from vblade import multilevel
    assert multilevel.AdaptiveBlockSparseAttnTrain(**geom).io_layout == "bhld"
    assert multilevel.AdaptiveBlockSparseAttnTrain(io_layout="blhd", **geom).io_layout == "blhd"
    with pytest.raises(ValueError, match="io_layout"):
        multilevel.AdaptiveBlockSparseAttnTrain(io_layout="hbld", **geom)
    with pytest.raises(ValueError, match="io_layout"):
        multilevel.sparse_attention_factory(io_layout="hbld")


class _Attn(nn.Module):
    def __init__(self):
        super().__init__()
        self.processor = "stock"

    def get_processor(self):
        return self.processor

    def set_processor(self, p):
        self.processor = p


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.attn1 = _Attn()


class _Model(nn.Module):
    def __init__(self, n=3):
        super().__init__()
        self.transformer_blocks = nn.ModuleList([_Block() for _ in range(n)])
        self.blocks = self.transformer_blocks


@pytest.mark.parametrize("setter,blocks", [("set_block_sparse_attn_cogvideox", "transformer_blocks"),
                                           ("set_adaptive_block_sparse_attn_wanx", "blocks")])
def test_setters_take_projection_layout(setter, blocks):
    fn = getattr(vblade, setter)
    m = _Model()
    inner = fn(m, projection_layout=True, fused_qk=True)
    assert inner.io_layout == "blhd"
    for b in getattr(m, blocks):
        assert b.attn1.inner_attention is inner
        assert b.attn1.processor.projection_layout is True and b.attn1.processor.fused_qk is True
        assert b.attn1.processor.last_out_is_view is None
    m = _Model()
    inner = fn(m)
    assert inner.io_layout == "bhld"
    assert all(b.attn1.processor.projection_layout is False for b in getattr(m, blocks))
    with pytest.raises(ValueError, match="projection_layout"):
        fn(_Model(), projection_layout=True, io_layout="bhld")


class _LayoutAttention(nn.Module):
    """SDPA as ``inner_attention``, its output in the asked memory order (what the module's io_layout
    does on the device)."""

    def __init__(self, blhd):
        super().__init__()
        self.blhd = blhd

    def forward(self, q, k, v):
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v)
        return o.transpose(1, 2).contiguous().transpose(1, 2) if self.blhd else o.contiguous()


@torch.no_grad()
def test_processors_record_whether_the_reshape_was_a_view():
    from qk_standins import StandInAttention
    g = torch.Generator().manual_seed(5)
    hidden, text = torch.randn(2, 40, 64, generator=g), torch.randn(2, 7, 64, generator=g)
    got = {"cog": [], "wan": []}
    for blhd in (False, True):
        attn = StandInAttention(64, 4, "cog")
        attn.inner_attention = _LayoutAttention(blhd)
        proc = patch.CogVideoXBlockSparseAttnProcessor(0, projection_layout=blhd)
        got["cog"].append(proc(attn, hidden, text)[0])
        assert proc.last_out_is_view is blhd
        attn = StandInAttention(64, 4, "wan")
        attn.inner_attention = _LayoutAttention(blhd)
        proc = patch.WanBlockSparseAttnProcessor(projection_layout=blhd)
        got["wan"].append(proc(attn, hidden))
        assert proc.last_out_is_view is blhd
    assert torch.equal(*got["cog"]) and torch.equal(*got["wan"])


def test_stand_in_blocks_take_projection_layout():
    seen = []

    class Spy(nn.Module):
        def forward(self, q, k, v):
            seen.append(v)
            return torch.nn.functional.scaled_dot_product_attention(q, k, v)

    x = torch.randn(1, 12, 32, generator=torch.Generator().manual_seed(0))
    outs = []
    for flag in (False, True):
        model = train.StandInTransformer(2, 32, 4, 2, 2.0, Spy(), gradient_checkpointing=False, dtype=torch.float32,
                                         projection_layout=flag)
        assert all(b.projection_layout is flag for b in model.transformer_blocks)
        outs.append(model(x))
        assert seen[-1].is_contiguous() is (not flag)       # the flag hands v over as a view
    assert torch.equal(outs[0], outs[1])
