"""CPU: the q/k prologue's host side — the header declares vb_qk_prologue and compiles as C, the
ctypes mirror matches it, argument validation returns the documented codes before any launch, the
setters take ``fused_qk`` without handing it to the module, and on CPU tensors the processors with
``fused_qk=True`` keep the eager chain and return exactly what ``fused_qk=False`` returns."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch
import torch.nn as nn

import vblade
from conftest import ROOT
from qk_standins import StandInAttention
from vblade import _lib, patch

HEADER = os.path.join(ROOT, "include", "vblade.h")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_compiles_as_c_and_struct_layout_matches():
    """gcc -std=c99 takes the header, the declaration has the documented type, and sizeof/offsetof
    of vb_qk_prologue_args equal the ctypes mirror's."""
    fields = [f[0] for f in _lib.QkPrologueArgs._fields_]
    decl = ['#include <stddef.h>', f'#include "{HEADER}"',
            "int (*entry)(const vb_qk_prologue_args*, const vb_qk_prologue_args*, void*) = vb_qk_prologue;"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vb_qk_prologue_args));',
             'printf("modes %d %d %d %d\\n", VB_QK_NORM_LAYER_HEAD, VB_QK_NORM_RMS_ROW, VB_QK_ROPE_REAL, VB_QK_ROPE_COMPLEX);']
    lines += [f'printf("{f} %zu\\n", offsetof(vb_qk_prologue_args, {f}));' for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        for name, src in (("decl.c", decl), ("layout.c", lines)):
            with open(os.path.join(d, name), "w") as fh:
                fh.write("\n".join(src) + "\n")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", os.path.join(d, "decl.c"),
                               "-o", os.path.join(d, "decl.o")])
        exe = os.path.join(d, "layout")
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", os.path.join(d, "layout.c"), "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = {line.split()[0]: line.split()[1:] for line in out if line}
    assert int(got["size"][0]) == ctypes.sizeof(_lib.QkPrologueArgs)
    assert [int(v) for v in got["modes"]] == [_lib.VB_QK_NORM_LAYER_HEAD, _lib.VB_QK_NORM_RMS_ROW,
                                              _lib.VB_QK_ROPE_REAL, _lib.VB_QK_ROPE_COMPLEX]
    for f in fields:
        assert int(got[f][0]) == getattr(_lib.QkPrologueArgs, f).offset, f


def test_prototype_is_bound_and_abi_is_still_4(lib):
    assert "vb_qk_prologue" in _lib.SIGNATURES and hasattr(lib, "vb_qk_prologue")
    assert lib.vb_abi_version() == _lib.ABI_VERSION == 4


def _args(**kw):
    a = _lib.QkPrologueArgs()
    a.x = a.out = 1 << 20
    a.B, a.L, a.H, a.D = 2, 40, 3, 64
    a.x_stride = a.out_stride = (40 * 192, 192)
    a.dtype = _lib.VB_DTYPE_BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,code,word", [
    (dict(D=96), _lib.VB_ERR_UNSUPPORTED, b"head_dim"),
    (dict(H=129), _lib.VB_ERR_UNSUPPORTED, b"8192"),
    (dict(x_stride=(40 * 192, 193)), _lib.VB_ERR_INVALID, b"strides"),
    (dict(out_stride=(40 * 192 + 4, 192)), _lib.VB_ERR_INVALID, b"strides"),
    (dict(x_stride=(40 * 192, 128)), _lib.VB_ERR_INVALID, b"row stride"),
    (dict(x=(1 << 20) + 2), _lib.VB_ERR_INVALID, b"aligned"),
    (dict(out=None), _lib.VB_ERR_INVALID, b"null"),
    (dict(dtype=7), _lib.VB_ERR_INVALID, b"dtype"),
    (dict(norm=3), _lib.VB_ERR_INVALID, b"norm mode"),
    (dict(norm=_lib.VB_QK_NORM_RMS_ROW, bias=1 << 20), _lib.VB_ERR_INVALID, b"bias"),
    (dict(norm=_lib.VB_QK_NORM_LAYER_HEAD, eps=-1.0), _lib.VB_ERR_INVALID, b"eps"),
    (dict(rope=_lib.VB_QK_ROPE_REAL, cos=1 << 20, sin=1 << 20, rope_start=41), _lib.VB_ERR_INVALID, b"rope_start"),
    (dict(rope=_lib.VB_QK_ROPE_REAL, cos=1 << 20), _lib.VB_ERR_INVALID, b"cos and sin"),
    (dict(rope=_lib.VB_QK_ROPE_COMPLEX), _lib.VB_ERR_INVALID, b"freqs"),
    (dict(rope=_lib.VB_QK_ROPE_COMPLEX, freqs=1 << 20, rope_start=3), _lib.VB_ERR_INVALID, b"every row"),
    (dict(rope=4), _lib.VB_ERR_INVALID, b"rope mode"),
])
def test_argument_validation_returns_before_any_launch(lib, kw, code, word):
    """No GPU is touched: each bad argument is refused on the host, for q and for k alike."""
    assert lib.vb_qk_prologue(ctypes.byref(_args(**kw)), None, None) == code
    assert word in lib.vb_last_error() and b"q:" in lib.vb_last_error()
    assert lib.vb_qk_prologue(ctypes.byref(_args()), ctypes.byref(_args(**kw)), None) == code
    assert word in lib.vb_last_error() and b"k:" in lib.vb_last_error()


def test_null_q_and_mismatched_k(lib):
    assert lib.vb_qk_prologue(None, None, None) == _lib.VB_ERR_INVALID
    assert b"null q" in lib.vb_last_error()
    assert lib.vb_qk_prologue(ctypes.byref(_args()), ctypes.byref(_args(L=39)), None) == _lib.VB_ERR_INVALID
    assert b"k must have q's" in lib.vb_last_error()


def test_ops_wrapper_checks_and_refuses_cpu_tensors():
    from vblade import ops
    x = torch.zeros(1, 8, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="norm must be"):
        ops.qk_prologue(x, heads=2, norm="group")
    with pytest.raises(ValueError, match="rope must be"):
        ops.qk_prologue(x, heads=2, rope="yarn")
    with pytest.raises(RuntimeError, match="HIP"):
        ops.qk_prologue(x, heads=2, norm="layer")
    with pytest.raises(ValueError, match=r"expected \[B,L"):
        ops.qk_prologue(x[0], heads=2)
    with pytest.raises(ValueError, match=r"expected \[B,L"):
        ops.qk_prologue(x, heads=3)


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.attn1 = StandInAttention(128, 2, "cog")


@pytest.mark.parametrize("fused", [None, False, True])
def test_setters_take_fused_qk_and_keep_it_from_the_module(fused):
    kw = {} if fused is None else {"fused_qk": fused}
    cog = nn.Module()
    cog.transformer_blocks = nn.ModuleList([_Block(), _Block()])
    inner = vblade.set_block_sparse_attn_cogvideox(cog, **kw)      # the module rejects unknown options
    assert inner.variant == "cog" and not hasattr(inner, "fused_qk")
    assert [b.attn1.processor.fused_qk for b in cog.transformer_blocks] == [bool(fused)] * 2
    assert [b.attn1.processor.idx for b in cog.transformer_blocks] == [0, 1]
    wan = nn.Module()
    wan.blocks = nn.ModuleList([_Block()])
    inner = vblade.set_adaptive_block_sparse_attn_wanx(wan, **kw)
    assert inner.variant == "wan" and wan.blocks[0].attn1.processor.fused_qk is bool(fused)
    with pytest.raises(TypeError, match="unknown options"):
        vblade.set_block_sparse_attn_cogvideox(cog, fused_kq=True)
    assert patch.CogVideoXBlockSparseAttnProcessor().fused_qk is False
    assert patch.WanBlockSparseAttnProcessor().fused_qk is False


def _rope(S, hd):
    g = torch.Generator().manual_seed(3)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * 6.28
    ang2 = ang.repeat_interleave(2, -1)
    return (ang2.cos().float(), ang2.sin().float()), torch.polar(torch.ones_like(ang), ang)[None, None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["cog", "wan"])
@torch.no_grad()
def test_cpu_tensors_keep_the_eager_chain(kind, dtype):
    """fused_qk=True on CPU tensors: last_path is "eager" and the output is fused_qk=False's, bit for bit."""
    heads, hd = (2, 64) if kind == "cog" else (2, 128)
    dim, N, T, B = heads * hd, 24, 5, 2
    attn = StandInAttention(dim, heads, kind).to(dtype)
    g = torch.Generator().manual_seed(1)
    hidden = torch.randn(B, N, dim, generator=g).to(dtype)
    text = torch.randn(B, T, dim, generator=g).to(dtype)
    cos_sin, freqs = _rope(N, hd)
    outs = []
    for fused in (False, True):
        if kind == "cog":
            proc = patch.CogVideoXBlockSparseAttnProcessor(0, fused_qk=fused)
            assert proc.last_path is None
            out = proc(attn, hidden, text, image_rotary_emb=cos_sin)
        else:
            proc = patch.WanBlockSparseAttnProcessor(fused_qk=fused)
            out = (proc(attn, hidden, None, rotary_emb=freqs),)
        assert proc.last_path == "eager"
        outs.append(out)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
