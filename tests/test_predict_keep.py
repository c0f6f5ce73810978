"""CPU: the predictor's sampling density (num_keep 16 / 32 / 64) at the Python and C ABI level, and
the reference pin of the oracle's pooled_scores at tiles 16 and 64
(tests/golden/pooled_scores_keep.npz, written by tests/golden/make_golden_keep.py from the
reference's Triton kernel under the interpreter)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bsa_oracle as O
from conftest import GOLDEN

DT = {"torch.float32": torch.float32, "torch.float16": torch.float16}


# ------------------------------------------------------------------ 7. Python-level acceptance
@pytest.mark.parametrize("keep", [16, 32, 64])
def test_modules_accept_the_three_densities(keep):
    import vblade
    from vblade import multilevel
    m = vblade.AdaptiveBlockSparseAttn("cog", num_keep=keep, width=8, height=6, depth=4, text_length=34)
    assert m.num_keep == keep and m.block == 128
    w = vblade.AdaptiveBlockSparseAttn("wan", num_keep=keep)
    assert w.num_keep == keep
    t = multilevel.AdaptiveBlockSparseAttnTrain(num_keep=keep, width=8, height=6, depth=4, text_length=34)
    assert t.num_keep == keep


def test_default_density_is_32():
    import vblade
    from vblade import multilevel, ops
    assert vblade.AdaptiveBlockSparseAttn("cog").num_keep == 32
    assert multilevel.AdaptiveBlockSparseAttnTrain().num_keep == 32
    assert ops.NUM_KEEP_VALUES == (16, 32, 64)
    assert ops._offset_width(None, None, None, drawn=True) == 32


@pytest.mark.parametrize("keep", [0, 8, 24, 33, 128])
def test_modules_reject_other_densities(keep):
    import vblade
    from vblade import multilevel
    with pytest.raises(ValueError, match="num_keep"):
        vblade.AdaptiveBlockSparseAttn("cog", num_keep=keep)
    with pytest.raises(ValueError, match="num_keep"):
        multilevel.AdaptiveBlockSparseAttnTrain(num_keep=keep)


def test_setters_forward_the_density():
    import torch.nn as nn
    import vblade
    from test_patch import FakeAttention

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn1 = FakeAttention(128, 2, qk_norm="head")

    model = nn.Module()
    model.transformer_blocks = nn.ModuleList([Block()])
    inner = vblade.set_block_sparse_attn_cogvideox(model, num_keep=16, width=8, height=6, depth=4,
                                                   text_length=34)
    assert inner.num_keep == 16
    model = nn.Module()
    model.blocks = nn.ModuleList([Block()])
    assert vblade.set_adaptive_block_sparse_attn_wanx(model, num_keep=64).num_keep == 64


def test_ops_mask_predict_offset_widths():
    """Given offsets set the density by their width; q_off and k_off must agree with each other and
    with an explicit num_keep. The checks run before anything touches a device."""
    from vblade import ops
    q = torch.zeros(1, 2, 600, 64, dtype=torch.bfloat16)

    def off(n):
        return torch.zeros(1, 2, n, dtype=torch.int32)

    with pytest.raises(ValueError, match="same width"):
        ops.mask_predict(q, q, off(16), off(32))
    with pytest.raises(ValueError, match="wide"):
        ops.mask_predict(q, q, off(16), off(16), num_keep=64)
    with pytest.raises(ValueError, match="wide"):
        ops.mask_predict(q, q, off(32), off(32), num_keep=16)
    with pytest.raises(ValueError, match="num_keep"):
        ops.mask_predict(q, q, rand=(torch.zeros(1, 2, 1, 128), torch.zeros(1, 2, 1, 128)), num_keep=0)
    for keep in (16, 32, 64):       # accepted: the call goes on to the device check (no CPU path)
        with pytest.raises(RuntimeError, match="HIP"):
            ops.mask_predict(q, q, off(keep), off(keep), num_keep=keep)
        with pytest.raises(RuntimeError, match="HIP"):
            ops.mask_predict(q, q, off(keep), off(keep))
        assert ops._offset_width(off(keep), off(keep), None, drawn=False) == keep
        assert ops._offset_width(None, None, keep, drawn=True) == keep


# ------------------------------------------------------------------ 8. workspace size through ctypes
@pytest.fixture(scope="module")
def lib():
    from vblade import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libvblade_hip.so is not built")
    return _lib.load()


def _args(lib, B, H, L, D, keep):
    from vblade import _lib
    p = _lib.PredictArgs()
    p.q = p.k = p.q_off = p.k_off = p.po = p.mask = 1 << 20
    p.B, p.H, p.L, p.D, p.block, p.num_keep = B, H, L, D, 128, keep
    p.q_stride = p.k_stride = (H * L * D, L * D, D)
    p.min_keep = p.max_keep = 1
    p.workspace = 1 << 24
    p.workspace_bytes = lib.vb_mask_predict_workspace_size(ctypes.byref(p))
    return p


@pytest.mark.parametrize("keep", [16, 32, 64])
@pytest.mark.parametrize("B,H,L,D", [(1, 2, 1000, 64), (2, 3, 17776, 64), (1, 1, 131072, 128)])
def test_workspace_size_follows_the_documented_formula(lib, B, H, L, D, keep):
    """include/vblade.h: B*H*(nb*num_keep*4 + nb*nb*num_keep*2) bytes."""
    nb = (L + 127) // 128
    p = _args(lib, B, H, L, D, keep)
    assert p.workspace_bytes == B * H * (nb * keep * 4 + nb * nb * keep * 2)
    if (B, H, L) == (1, 1, 131072):   # the header's extremes: R alone per (b,h) at 1024 blocks
        assert nb * nb * keep * 2 == {16: 33554432, 32: 67108864, 64: 134217728}[keep]


@pytest.mark.parametrize("keep", [8, 24, 128, 0, -32])
def test_library_refuses_other_densities_without_gpu(lib, keep):
    from vblade import _lib
    p = _args(lib, 1, 2, 1000, 64, keep)
    p.workspace_bytes = 1 << 30
    for entry in (lib.vb_mask_predict, lib.vb_mask_predict_long):
        assert entry(ctypes.byref(p), None) == _lib.VB_ERR_UNSUPPORTED
        assert b"16, 32 or 64" in lib.vb_last_error()


@pytest.mark.parametrize("keep", [16, 64])
def test_library_checks_run_at_the_new_densities_without_gpu(lib, keep):
    """The argument checks behind the density check: an undersized workspace is VB_ERR_INVALID, and
    each entry keeps its row limit (320 / 1024 blocks)."""
    from vblade import _lib
    p = _args(lib, 1, 2, 1000, 64, keep)
    p.workspace_bytes -= 1
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert b"workspace" in lib.vb_last_error()
    p = _args(lib, 1, 1, 321 * 128, 64, keep)
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_UNSUPPORTED
    assert b"too long" in lib.vb_last_error()
    p = _args(lib, 1, 1, 1025 * 128, 64, keep)
    assert lib.vb_mask_predict_long(ctypes.byref(p), None) == _lib.VB_ERR_UNSUPPORTED
    assert b"too long" in lib.vb_last_error()


# ------------------------------------------------------------------ 9. reference pin at tiles 16, 64
@pytest.mark.parametrize("keep", [16, 64])
@pytest.mark.parametrize("case", ["f32_d64", "f16_d64", "f32_d128", "f16_d128"])
def test_pooled_scores_match_reference_triton_at_density(case, keep):
    """The criterion of test_oracle_golden.test_pooled_scores_match_reference_triton."""
    z = np.load(os.path.join(GOLDEN, "pooled_scores_keep.npz"))
    tag = f"k{keep}_{case}"
    dt = DT[str(z[tag + "_dtype"])]
    q = torch.from_numpy(z[tag + "_q"]).to(dt)
    k = torch.from_numpy(z[tag + "_k"]).to(dt)
    assert q.shape[2] % keep == 0 and q.shape[2] // keep in (5, 11)
    po = O.pooled_scores(q, k, 1.0 / q.shape[-1] ** 0.5, keep, dt)
    ref = torch.from_numpy(z[tag + "_po"])
    if dt == torch.float16:
        assert torch.equal(po, ref)          # storage rounding emulated bit-exactly
    else:
        assert torch.allclose(po, ref, rtol=0, atol=1e-7)  # fp32: summation order only
