"""CPU: the q/k prologue backward's host side — the header declares vb_qk_prologue_bwd and its
workspace query and compiles as C, the ctypes mirror matches it, every argument rule returns its
code before any launch, the workspace size is host arithmetic, the setters take
``fused_qk_backward`` without handing it to the module, and on CPU tensors the processors keep the
eager chain with grad enabled and return exactly what ``fused_qk=False`` returns."""
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
Args = _lib.QkPrologueBwdArgs if hasattr(_lib, "QkPrologueBwdArgs") else None


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_compiles_as_c_and_struct_layout_matches():
    """gcc -std=c99 takes the header, both declarations have the documented types, and
    sizeof/offsetof of vb_qk_prologue_bwd_args equal the ctypes mirror's."""
    fields = [f[0] for f in Args._fields_]
    decl = ['#include <stddef.h>', f'#include "{HEADER}"',
            "int (*entry)(const vb_qk_prologue_bwd_args*, const vb_qk_prologue_bwd_args*, void*) = vb_qk_prologue_bwd;",
            "uint64_t (*size)(const vb_qk_prologue_bwd_args*, const vb_qk_prologue_bwd_args*) = "
            "vb_qk_prologue_bwd_workspace_size;"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vb_qk_prologue_bwd_args));',
             'printf("maxgrid %d\\n", VB_QK_BWD_MAX_GRID);']
    lines += [f'printf("{f} %zu\\n", offsetof(vb_qk_prologue_bwd_args, {f}));' for f in fields]
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
    assert int(got["size"][0]) == ctypes.sizeof(Args)
    assert int(got["maxgrid"][0]) == _lib.VB_QK_BWD_MAX_GRID
    for f in fields:
        assert int(got[f][0]) == getattr(Args, f).offset, f


def test_symbols_are_bound_and_abi_is_still_4(lib):
    for name in ("vb_qk_prologue_bwd", "vb_qk_prologue_bwd_workspace_size"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.vb_abi_version() == _lib.ABI_VERSION == 4


X, G, DX, P = 1 << 20, 2 << 20, 3 << 20, 4 << 20     # addresses far enough apart not to overlap


def _args(**kw):
    a = Args()
    a.x, a.g, a.dx = X, G, DX
    a.B, a.L, a.H, a.D = 2, 40, 3, 64
    a.x_stride = a.dx_stride = (40 * 192, 192)
    a.g_stride = (3 * 40 * 64, 64, 40 * 64)      # [B,H,L,D] contiguous
    a.dtype = _lib.VB_DTYPE_BF16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


LAYER, RMS = _lib.VB_QK_NORM_LAYER_HEAD, _lib.VB_QK_NORM_RMS_ROW


@pytest.mark.parametrize("kw,code,word", [
    (dict(D=96), _lib.VB_ERR_UNSUPPORTED, b"head_dim"),
    (dict(H=129), _lib.VB_ERR_UNSUPPORTED, b"8192"),
    (dict(x_stride=(40 * 192, 193)), _lib.VB_ERR_INVALID, b"strides"),
    (dict(dx_stride=(40 * 192 + 4, 192)), _lib.VB_ERR_INVALID, b"strides"),
    (dict(x_stride=(40 * 192, 128)), _lib.VB_ERR_INVALID, b"row stride"),
    (dict(x=X + 2), _lib.VB_ERR_INVALID, b"aligned"),
    (dict(g=G + 8), _lib.VB_ERR_INVALID, b"aligned"),
    (dict(g=None), _lib.VB_ERR_INVALID, b"null"),
    (dict(dx=None), _lib.VB_ERR_INVALID, b"null"),
    (dict(g_stride=(3 * 40 * 64, 68, 40 * 64)), _lib.VB_ERR_INVALID, b"g strides"),
    (dict(g_stride=(3 * 40 * 64 + 4, 64, 40 * 64)), _lib.VB_ERR_INVALID, b"g strides"),
    (dict(g_stride=(3 * 40 * 64, 64, 40 * 64 + 2)), _lib.VB_ERR_INVALID, b"g strides"),
    (dict(dx=X), _lib.VB_ERR_INVALID, b"alias"),
    (dict(dx=G), _lib.VB_ERR_INVALID, b"alias"),
    (dict(dx=X + 192 * 2), _lib.VB_ERR_INVALID, b"alias"),            # one row into x: still an overlap
    (dict(dtype=7), _lib.VB_ERR_INVALID, b"dtype"),
    (dict(norm=3), _lib.VB_ERR_INVALID, b"norm mode"),
    (dict(norm=RMS, bias=P), _lib.VB_ERR_INVALID, b"bias"),
    (dict(norm=RMS, dbias=P), _lib.VB_ERR_INVALID, b"dbias"),
    (dict(dbias=P), _lib.VB_ERR_INVALID, b"dbias"),
    (dict(dweight=P), _lib.VB_ERR_INVALID, b"dweight"),
    (dict(norm=LAYER, eps=-1.0), _lib.VB_ERR_INVALID, b"eps"),
    (dict(grid_limit=-1), _lib.VB_ERR_INVALID, b"grid_limit"),
    (dict(rope=_lib.VB_QK_ROPE_REAL, cos=P, sin=P, rope_start=41), _lib.VB_ERR_INVALID, b"rope_start"),
    (dict(rope=_lib.VB_QK_ROPE_REAL, cos=P), _lib.VB_ERR_INVALID, b"cos and sin"),
    (dict(rope=_lib.VB_QK_ROPE_COMPLEX), _lib.VB_ERR_INVALID, b"freqs"),
    (dict(rope=_lib.VB_QK_ROPE_COMPLEX, freqs=P, rope_start=3), _lib.VB_ERR_INVALID, b"every row"),
    (dict(rope=4), _lib.VB_ERR_INVALID, b"rope mode"),
])
def test_argument_validation_returns_before_any_launch(lib, kw, code, word):
    """No GPU is touched: each bad argument is refused on the host, for q, for k beside q, and for k alone."""
    assert lib.vb_qk_prologue_bwd(ctypes.byref(_args(**kw)), None, None) == code
    err = lib.vb_last_error()
    assert word in err and b"vb_qk_prologue_bwd: q:" in err
    assert lib.vb_qk_prologue_bwd(ctypes.byref(_args()), ctypes.byref(_args(**kw)), None) == code
    err = lib.vb_last_error()
    assert word in err and b"vb_qk_prologue_bwd: k:" in err
    assert lib.vb_qk_prologue_bwd(None, ctypes.byref(_args(**kw)), None) == code
    err = lib.vb_last_error()
    assert word in err and b"vb_qk_prologue_bwd: k:" in err


def test_null_arguments_and_mismatched_k(lib):
    assert lib.vb_qk_prologue_bwd(None, None, None) == _lib.VB_ERR_INVALID
    assert b"null q and k" in lib.vb_last_error()
    for kw in (dict(L=39), dict(grid_limit=3)):
        assert lib.vb_qk_prologue_bwd(ctypes.byref(_args()), ctypes.byref(_args(**kw)), None) == _lib.VB_ERR_INVALID
        assert b"k must have q's" in lib.vb_last_error()


def test_workspace_size_is_host_arithmetic(lib):
    """0 without parameter gradients; otherwise one partial vector per workgroup the launch can have:
    min(B*L, grid_limit or VB_QK_BWD_MAX_GRID) times D (LayerNorm weight, bias) or H*D (RMSNorm weight)
    fp32 values, for q and k together."""
    size = lib.vb_qk_prologue_bwd_workspace_size
    ref = ctypes.byref
    assert size(ref(_args()), None) == 0
    assert size(ref(_args(norm=LAYER)), ref(_args(norm=LAYER))) == 0
    assert size(None, None) == 0
    rows = 2 * 40
    assert size(ref(_args(norm=LAYER, dweight=P)), None) == rows * 64 * 4          # 80 rows < 1024 workgroups
    assert size(ref(_args(norm=LAYER, dweight=P, dbias=P)), None) == 2 * rows * 64 * 4
    assert size(ref(_args(norm=RMS, dweight=P)), None) == rows * 192 * 4
    sizes = [size(ref(_args(norm=LAYER, dweight=P, grid_limit=g)), None) for g in (1, 3, 7, 80, 200)]
    assert sizes == [g * 64 * 4 for g in (1, 3, 7, 80, 80)]                          # grows, then rows bound it
    big = dict(B=5, L=4000, x_stride=(4000 * 192, 192), dx_stride=(4000 * 192, 192), g_stride=(3 * 4000 * 64, 64, 4000 * 64))
    assert size(ref(_args(norm=RMS, dweight=P, **big)), None) == _lib.VB_QK_BWD_MAX_GRID * 192 * 4
    assert size(ref(_args(norm=RMS, dweight=P, grid_limit=2000, **big)), None) == 2000 * 192 * 4
    both = size(ref(_args(norm=LAYER, dweight=P, grid_limit=3)), ref(_args(norm=LAYER, dbias=P, grid_limit=3)))
    assert both == 2 * 3 * 64 * 4
    assert size(None, ref(_args(norm=LAYER, dbias=P, grid_limit=3))) == 3 * 64 * 4


def test_a_missing_or_small_workspace_is_refused_before_any_launch(lib):
    for kw in (dict(), dict(workspace=P), dict(workspace=P, workspace_bytes=80 * 64 * 4 - 1),
               dict(workspace=P + 4, workspace_bytes=1 << 20)):
        a = _args(norm=LAYER, dweight=5 << 20, **kw)
        assert lib.vb_qk_prologue_bwd(ctypes.byref(a), None, None) == _lib.VB_ERR_INVALID
        assert b"workspace" in lib.vb_last_error()
    # k's gradients beside a q that asks for none: the first tensor's struct still names the workspace
    q, k = _args(norm=LAYER), _args(norm=LAYER, dbias=5 << 20, workspace=P, workspace_bytes=1 << 20)
    assert lib.vb_qk_prologue_bwd(ctypes.byref(q), ctypes.byref(k), None) == _lib.VB_ERR_INVALID
    assert b"workspace" in lib.vb_last_error()


def test_ops_wrapper_checks_and_refuses_cpu_tensors():
    from vblade import autograd, ops
    x = torch.zeros(1, 8, 128, dtype=torch.bfloat16)
    g = torch.zeros(1, 2, 8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="both None"):
        ops.qk_prologue_bwd(x, heads=2)
    with pytest.raises(ValueError, match="norm must be"):
        ops.qk_prologue_bwd(x, gq=g, heads=2, norm="group")
    with pytest.raises(RuntimeError, match="HIP"):
        ops.qk_prologue_bwd(x, gq=g, heads=2, norm="layer")
    with pytest.raises(ValueError, match="forward's input"):
        ops.qk_prologue_bwd(x, gq=g, gk=g, heads=2)
    with pytest.raises(TypeError, match="inplace"):
        autograd.qk_prologue(x, heads=2, inplace=True)
    cos = torch.zeros(8, 64, requires_grad=True)
    with pytest.raises(ValueError, match="requires grad"):
        autograd.qk_prologue(x, heads=2, rope="real", cos=cos, sin=cos.detach())
    assert vblade.qk_prologue is autograd.qk_prologue


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.attn1 = StandInAttention(128, 2, "cog")


@pytest.mark.parametrize("fused,backward", [(None, None), (True, None), (True, False), (True, True), (False, True)])
def test_setters_take_fused_qk_backward_and_keep_it_from_the_module(fused, backward):
    kw = {k: v for k, v in (("fused_qk", fused), ("fused_qk_backward", backward)) if v is not None}
    cog = nn.Module()
    cog.transformer_blocks = nn.ModuleList([_Block(), _Block()])
    inner = vblade.set_block_sparse_attn_cogvideox(cog, **kw)      # the module rejects unknown options
    assert inner.variant == "cog" and not hasattr(inner, "fused_qk_backward")
    assert [b.attn1.processor.fused_qk_backward for b in cog.transformer_blocks] == [bool(backward)] * 2
    assert [b.attn1.processor.fused_qk for b in cog.transformer_blocks] == [bool(fused)] * 2
    wan = nn.Module()
    wan.blocks = nn.ModuleList([_Block()])
    inner = vblade.set_adaptive_block_sparse_attn_wanx(wan, **kw)
    assert inner.variant == "wan" and wan.blocks[0].attn1.processor.fused_qk_backward is bool(backward)
    assert wan.blocks[0].attn1.processor.fused_qk is bool(fused)
    with pytest.raises(TypeError, match="unknown options"):
        vblade.set_block_sparse_attn_cogvideox(cog, fused_qk_backwards=True)
    assert patch.CogVideoXBlockSparseAttnProcessor().fused_qk_backward is False
    assert patch.WanBlockSparseAttnProcessor().fused_qk_backward is False


def _rope(S, hd):
    g = torch.Generator().manual_seed(3)
    ang = torch.rand(S, hd // 2, generator=g, dtype=torch.float64) * 6.28
    ang2 = ang.repeat_interleave(2, -1)
    return (ang2.cos().float(), ang2.sin().float()), torch.polar(torch.ones_like(ang), ang)[None, None]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["cog", "wan"])
def test_cpu_tensors_keep_the_eager_chain_with_grad_enabled(kind, dtype):
    """fused_qk=True, fused_qk_backward=True on CPU tensors that record autograd: last_path is
    "eager", and the output and the gradients are fused_qk=False's, bit for bit."""
    heads, hd = (2, 64) if kind == "cog" else (2, 128)
    dim, N, T, B = heads * hd, 24, 5, 2
    attn = StandInAttention(dim, heads, kind).to(dtype)
    g = torch.Generator().manual_seed(1)
    hidden = torch.randn(B, N, dim, generator=g).to(dtype).requires_grad_()
    text = torch.randn(B, T, dim, generator=g).to(dtype)
    cos_sin, freqs = _rope(N, hd)
    results = []
    for flags in (dict(fused_qk=False), dict(fused_qk=True, fused_qk_backward=True), dict(fused_qk_backward=True)):
        if kind == "cog":
            proc = patch.CogVideoXBlockSparseAttnProcessor(0, **flags)
            out = proc(attn, hidden, text, image_rotary_emb=cos_sin)[0]
        else:
            proc = patch.WanBlockSparseAttnProcessor(**flags)
            out = proc(attn, hidden, None, rotary_emb=freqs)
        assert proc.last_path == "eager" and out.requires_grad
        params = [hidden, attn.norm_q.weight, attn.to_k.weight]
        grads = torch.autograd.grad(out.float().square().sum(), params)
        results.append([out.detach(), *grads])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert torch.equal(a, b)
