"""CPU: the C ABI library loads, exports every symbol include/vblade.h declares, its ctypes
struct layouts match the C header (compiled with gcc), host-side entry points behave, and the
argument validation returns the documented error codes without touching a GPU."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "vblade.h")


def _declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vb_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from vblade import _lib
    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(lib):
    from vblade import _lib
    names = _declared_functions()
    assert names, "no functions parsed from vblade.h"
    for n in names:
        assert hasattr(lib, n), f"{n} missing from libvblade_hip.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert set(_lib.SIGNATURES) == set(names)


def test_abi_version(lib):
    from vblade import _lib
    assert lib.vb_abi_version() == _lib.ABI_VERSION == 4


def test_struct_layouts_match_header():
    """sizeof/offsetof of vb_attn_args and vb_predict_args from gcc == the ctypes mirrors."""
    from vblade._lib import AttnArgs, BwdArgs, MlAttnArgs, MlBwdArgs, PredictArgs
    structs = (("vb_attn_args", AttnArgs), ("vb_predict_args", PredictArgs),
               ("vb_attn_bwd_args", BwdArgs), ("vb_ml_attn_args", MlAttnArgs),
               ("vb_ml_attn_bwd_args", MlBwdArgs))
    fields = {st: [f[0] for f in cls._fields_] for st, cls in structs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){"]
    for st, fl in fields.items():
        lines.append(f'printf("{st} %zu\\n", sizeof({st}));')
        for f in fl:
            lines.append(f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "l")
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    got = dict(line.split() for line in out if line)
    for st, cls in structs:
        assert int(got[st]) == ctypes.sizeof(cls), st
        for f in fields[st]:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, f"{st}.{f}"


def test_gilbert_perm_host_entry_matches_reference_fixture(lib):
    from vblade import ops
    z = np.load(os.path.join(GOLDEN, "gilbert_perms.npz"))
    for key in z.files:
        w, h, d = map(int, key.split("_")[1].split("x"))
        assert np.array_equal(ops.gilbert_perm(w, h, d), z[key]), key


def test_invalid_arguments_return_codes_without_gpu(lib):
    from vblade import _lib
    buf = np.zeros(8, dtype=np.int32)
    assert lib.vb_gilbert3d_perm(0, 2, 2, buf.ctypes.data) == _lib.VB_ERR_INVALID
    assert b"positive" in lib.vb_last_error()
    # dropout is rejected before any device work
    rc = lib.vb_block_sparse_attn_fwd(1, 1, 1, 1, 1, None, None, None, 1, 1, 64, 128, 128,
                                      0.1, 1, 0.0, 0, 0, 0, 1, 1, 0, None)
    assert rc == _lib.VB_ERR_UNSUPPORTED and b"dropout" in lib.vb_last_error()
    rc = lib.vb_block_sparse_attn_fwd(1, 1, 1, 1, 1, None, None, None, 1, 1, 64, 128, 128,
                                      0.0, 1, 0.0, 1, 0, 0, 1, 1, 0, None)
    assert rc == _lib.VB_ERR_UNSUPPORTED
    # SURVEY Appendix B's mask_head_mode: per_head (0) and shared_head0 (1) only
    rc = lib.vb_block_sparse_attn_fwd(1, 1, 1, 1, 1, None, None, None, 1, 1, 64, 128, 128,
                                      0.0, 1, 0.0, 0, 0, 0, 1, 1, 2, None)
    assert rc == _lib.VB_ERR_INVALID and b"mask_head_mode" in lib.vb_last_error()
    a = _lib.AttnArgs()
    assert lib.vb_attn_fwd(ctypes.byref(a), None) == _lib.VB_ERR_INVALID
    p = _lib.PredictArgs()
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert lib.vb_energy_mask(None, 1, 1, 1, 1, 0.95, 1, 1, 0, 0, None, None, None) == _lib.VB_ERR_INVALID
    assert lib.vb_pool_kv(None, None, None, None, None, 1, 1, 1, 64, 15, 0, None, None, None, None, None) == _lib.VB_ERR_INVALID
    assert lib.vb_lse_combine(None, None, None, None, 1, 1, 1, 64, 15.0, 0, None, None, None) == _lib.VB_ERR_INVALID
    b = _lib.BwdArgs()
    assert lib.vb_attn_bwd(ctypes.byref(b), None) == _lib.VB_ERR_INVALID
    b.B = b.H = 1
    b.Lq = b.Lk = 128
    b.D = 96
    assert lib.vb_attn_bwd(ctypes.byref(b), None) == _lib.VB_ERR_UNSUPPORTED
    assert b"head_dim" in lib.vb_last_error()
    # kernel_select: unknown bits refused before any launch (ABI 4)
    b.D = 64
    b.q = b.k = b.v = b.out = b.lse = b.dout = b.dq = b.dk = b.dv = 1 << 20
    b.kernel_select = 8
    assert lib.vb_attn_bwd(ctypes.byref(b), None) == _lib.VB_ERR_INVALID
    assert b"kernel_select" in lib.vb_last_error()
    b.kernel_select = 0
    # workspace sizing is pure host arithmetic
    assert lib.vb_attn_bwd_workspace_size(ctypes.byref(b)) >= 2 * 64 * 4 * 4
    assert lib.vb_block_sparse_attn_bwd_workspace_size(1, 1, 128) > 0
    rc = lib.vb_block_sparse_attn_bwd(*([None] * 11), 1, 1, 64, 128, 128, 0.1, 0.0, 0, 0, 1, 0,
                                      None, None, None, None, 0, 0, None)
    assert rc == _lib.VB_ERR_UNSUPPORTED and b"dropout" in lib.vb_last_error()
    rc = lib.vb_block_sparse_attn_bwd(*([None] * 11), 1, 1, 64, 128, 128, 0.0, 0.0, 0, 0, 1, 0,
                                      None, None, None, None, 0, 5, None)
    assert rc == _lib.VB_ERR_INVALID and b"mask_head_mode" in lib.vb_last_error()
    # multi-level entry points
    assert lib.vb_kv_pyramid_rows(17776) == 15 * 17792 // 8
    assert lib.vb_kv_pyramid_rows(128) == 240
    m = _lib.MlAttnArgs()
    assert lib.vb_ml_attn_fwd(ctypes.byref(m), None) == _lib.VB_ERR_INVALID
    m.B = m.H = 1
    m.L = 300
    m.D = 80
    m.q = m.kpyr = m.vpyr = m.level_mask = m.out = 16
    assert lib.vb_ml_attn_fwd(ctypes.byref(m), None) == _lib.VB_ERR_UNSUPPORTED
    mb = _lib.MlBwdArgs()
    assert lib.vb_ml_attn_bwd(ctypes.byref(mb), None) == _lib.VB_ERR_INVALID
    mb.B = mb.H = 1
    mb.L, mb.D = 300, 64
    assert lib.vb_ml_attn_bwd_workspace_size(ctypes.byref(mb)) > 7 * 384 // 8 * 64 * 4 * 2
    mb.q = mb.kpyr = mb.vpyr = mb.level_mask = mb.out = mb.lse = mb.dout = mb.dq = mb.dk = mb.dv = 1 << 20
    mb.kernel_select = _lib.VB_BWD_SEL_DQ_RING4     # the multi-level dQ has one ring
    assert lib.vb_ml_attn_bwd(ctypes.byref(mb), None) == _lib.VB_ERR_INVALID
    assert b"kernel_select" in lib.vb_last_error()
    assert lib.vb_kv_pyramid(None, None, None, None, None, 1, 1, 1, 64, 0, None, None, None) == _lib.VB_ERR_INVALID
    vals = np.array([3], dtype=np.int32)
    se = np.array([0.0, 1.0], dtype=np.float64)
    rc = lib.vb_level_mask(16, 1, 1, 4, 4, 1, vals.ctypes.data, se[:1].ctypes.data, se[1:].ctypes.data,
                           0, 16, None)
    assert rc == _lib.VB_ERR_INVALID and b"band values" in lib.vb_last_error()


def test_mask_predict_option_checks_without_gpu(lib):
    """vb_mask_predict's host-side checks of the round-3 options run before any launch: Philox
    draws exclusive with rand_q/rand_k and limited to one torch.rand grid-stride pass, level bands
    validated and needing a mask output."""
    from vblade import _lib
    def args(B=1, H=2, L=1000):
        p = _lib.PredictArgs()
        p.q = p.k = p.q_off = p.k_off = p.po = p.mask = 1 << 20
        p.B, p.H, p.L, p.D, p.block, p.num_keep = B, H, L, 64, 128, 32
        p.q_stride = p.k_stride = (H * L * 64, L * 64, 64)
        p.min_keep = p.max_keep = 1
        p.workspace = 1 << 24
        p.workspace_bytes = lib.vb_mask_predict_workspace_size(ctypes.byref(p))
        return p
    p = args()
    p.philox, p.rand_q, p.rand_k = 1, 1 << 20, 1 << 20
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert b"exclusive" in lib.vb_last_error()
    p = args(B=2, H=2049)                         # 2*2049*128 > 524288 (CUs x threads per CU)
    p.philox = 1
    rc = lib.vb_mask_predict(ctypes.byref(p), None)
    import torch
    if torch.cuda.is_available():   # the bound is the device's own CUs x max threads per CU
        pr = torch.cuda.get_device_properties(0)
        assert rc == _lib.VB_ERR_UNSUPPORTED
        assert str(pr.multi_processor_count * pr.max_threads_per_multi_processor).encode() in lib.vb_last_error()
    else:                           # no device to query: refused before any launch
        assert rc == _lib.VB_ERR_LAUNCH and b"CU count" in lib.vb_last_error()
    vals = np.array([3], dtype=np.int32)
    se = np.array([0.0, 1.0], dtype=np.float64)
    p = args()
    p.mask_level, p.level_bands = 1, 1
    p.level_band_value, p.level_band_start, p.level_band_end = vals.ctypes.data, se[:1].ctypes.data, se[1:].ctypes.data
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert b"band values" in lib.vb_last_error()
    p = args()
    p.mask_level, p.level_bands, p.level_band_value = 1, 9, vals.ctypes.data
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    p = args()
    p.mask, p.mask_level = None, 1
    assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
    assert b"mask output" in lib.vb_last_error()
    # the kept counts come from the energy rule only: refused with the level mask or scores only
    for level, mask in ((1, 1 << 20), (0, None)):
        p = args()
        p.mask_rows_kept = 1 << 20
        p.mask = mask
        if level:
            p.mask_level, p.level_bands = 1, 1
            p.level_band_value, p.level_band_start, p.level_band_end = (
                np.array([1], dtype=np.int32).ctypes.data, se[:1].ctypes.data, se[1:].ctypes.data)
        assert lib.vb_mask_predict(ctypes.byref(p), None) == _lib.VB_ERR_INVALID
        assert b"mask_rows_kept" in lib.vb_last_error()


def test_level_bands_follow_mask_ratio_dict_order():
    from vblade import ops
    vals, st, en = ops._level_bands({8: (0.25, 0.5), 1: (0.0, 0.05)})
    assert vals.tolist() == [8, 1] and st.tolist() == [0.25, 0.0] and en.tolist() == [0.5, 0.05]
    vals, _, _ = ops._level_bands(None)
    assert vals.tolist() == [int(v) for v in ops.ML_MASK_RATIOS]
    assert ops.claim_rand_draws("cuda", ops.RAND_ONE_PASS_NUMEL + 1) is None   # past one pass: torch.rand


def test_ops_refuse_cpu_tensors():
    """The product path has no CPU fallback: CPU tensors raise."""
    import torch
    from vblade import ops
    q = torch.zeros(1, 1, 128, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.attention_fwd(q, q, q)
    lse = torch.zeros(1, 1, 128)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.attention_bwd(q, q, q, q, q, lse)


def test_module_config_and_retain_counts():
    import vblade
    from vblade.attention import retain_counts
    m = vblade.AdaptiveBlockSparseAttn("cog")
    assert m.gilbert_rearranger.seq_len == 17776 and m.force_tail == 2 and m.sample_gap == 15
    w = vblade.AdaptiveBlockSparseAttn("wan")
    assert w.gilbert_rearranger.seq_len == 32760 and w.force_tail == 0 and w.sample_gap == 30
    assert retain_counts(139, 0.05, 0.1, "cog") == (6, 13)
    assert retain_counts(256, 0.05, 0.17, "wan") == (12, 43)
    rows = m.gilbert_rearranger.rows.long()
    assert sorted(rows.tolist()) == list(range(17776))
    assert rows[-226:].tolist() == list(range(226))  # text tail, in order


def test_gilbert_rearranger_round_trip_cpu():
    import torch
    import vblade
    g = vblade.GilbertRearranger(8, 6, 4, text_length=10)
    x = torch.randn(2, 3, 8 * 6 * 4 + 10, 16)
    q, k, v = g.rearrange(x, x, x)
    assert torch.equal(q[..., -10:, :], x[..., :10, :])
    assert torch.equal(g.reversed_rearrange(q), x)


# ---------------------------------------------------------------------------------------------
# The attention entries' argument validation and workspace arithmetic, pinned value by value. Every
# case below is refused by a host check, so nothing is launched and the fake (non-null, 16-byte
# aligned) pointers are never dereferenced. The literals were recorded from the library before the
# backward's host layer moved into a unit of its own, and the forward entries' (vb_attn_fwd,
# vb_ml_attn_fwd, vb_block_sparse_attn_fwd) before the forward's did: a refactor of either layer must
# reproduce them.
# ---------------------------------------------------------------------------------------------
_PTR, _WS = 1 << 20, 1 << 24
_B, _H, _L, _LK, _LKP, _GAP, _D = 1, 2, 200, 330, 42, 8, 64
_BIG = 1 << 62


def _st(L, D=_D, H=_H):
    return (H * L * D, L * D, D)


def _fwd_args():
    from vblade import _lib
    a = _lib.AttnArgs()
    a.q = a.k = a.v = a.out = a.kp = a.vp = _PTR
    a.q_stride = a.out_stride = _st(_L)
    a.k_stride = a.v_stride = _st(_LK)
    a.kp_stride = a.vp_stride = _st(_LKP)
    a.use_main, a.Lkp = 1, _LKP
    a.B, a.H, a.Lq, a.Lk, a.D = _B, _H, _L, _LK, _D
    return a


def _ml_fwd_args():
    from vblade import _lib
    a = _lib.MlAttnArgs()
    a.q = a.kpyr = a.vpyr = a.level_mask = a.out = _PTR
    a.q_stride = a.out_stride = _st(_L)
    a.B, a.H, a.L, a.D = _B, _H, _L, _D
    return a


def _bwd_args():
    from vblade import _lib
    a = _lib.BwdArgs()
    a.q = a.k = a.v = a.out = a.lse = a.dout = a.dq = a.dk = a.dv = _PTR
    a.kp = a.vp = a.out2 = a.lse2 = _PTR
    a.q_stride = a.out_stride = a.out2_stride = a.dout_stride = a.dq_stride = _st(_L)
    a.k_stride = a.v_stride = a.dk_stride = a.dv_stride = _st(_LK)
    a.kp_stride = a.vp_stride = _st(_LKP)
    a.Lkp, a.pool_gap = _LKP, _GAP
    a.B, a.H, a.Lq, a.Lk, a.D = _B, _H, _L, _LK, _D
    a.workspace, a.workspace_bytes = _WS, _BIG
    return a


def _ml_bwd_args():
    from vblade import _lib
    a = _lib.MlBwdArgs()
    a.q = a.kpyr = a.vpyr = a.level_mask = a.out = a.lse = a.dout = a.dq = a.dk = a.dv = _PTR
    a.q_stride = a.out_stride = a.dout_stride = a.dq_stride = a.dk_stride = a.dv_stride = _st(_L)
    a.B, a.H, a.L, a.D = _B, _H, _L, _D
    a.workspace, a.workspace_bytes = _WS, _BIG
    return a


# vb_block_sparse_attn_bwd's positional arguments, by name
_BS_NAMES = ("dout", "q", "k", "v", "out", "lse", "cu_q", "cu_k", "head_mask_type", "streaming_info",
             "mask", "batch", "num_heads", "head_dim", "max_seqlen_q", "max_seqlen_k", "p_dropout",
             "softmax_scale", "is_causal", "exact_streaming", "deterministic", "dtype", "dq", "dk", "dv",
             "workspace", "workspace_bytes", "mask_head_mode", "stream")


def _bs_bwd_args():
    a = dict.fromkeys(_BS_NAMES, None)
    for n in ("dout", "q", "k", "v", "out", "lse", "cu_q", "cu_k", "dq", "dk", "dv"):
        a[n] = _PTR
    a.update(batch=_B, num_heads=_H, head_dim=_D, max_seqlen_q=_L, max_seqlen_k=_LK, p_dropout=0.0,
             softmax_scale=0.0, is_causal=0, exact_streaming=0, deterministic=1, dtype=0,
             workspace=_WS, workspace_bytes=_BIG, mask_head_mode=0)
    return a


# vb_block_sparse_attn_fwd's positional arguments, by name
_BSF_NAMES = ("q", "k", "v", "cu_q", "cu_k", "head_mask_type", "streaming_info", "mask", "batch", "num_heads",
              "head_dim", "max_seqlen_q", "max_seqlen_k", "p_dropout", "deterministic", "softmax_scale",
              "is_causal", "exact_streaming", "dtype", "out", "lse", "mask_head_mode", "stream")


def _bs_fwd_args():
    a = dict.fromkeys(_BSF_NAMES, None)
    for n in ("q", "k", "v", "cu_q", "cu_k", "out", "lse"):
        a[n] = _PTR
    a.update(batch=_B, num_heads=_H, head_dim=_D, max_seqlen_q=_L, max_seqlen_k=_LK, p_dropout=0.0,
             deterministic=1, softmax_scale=0.0, is_causal=0, exact_streaming=0, dtype=0, mask_head_mode=0)
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            if isinstance(a, dict):
                a[k] = v
            else:
                setattr(a, k, v)
    return f


def _row_stride(field, value):
    def f(a):
        s = list(getattr(a, field))
        s[2] = value
        setattr(a, field, tuple(s))
    return f


def _both(*fs):
    def f(a):
        for g in fs:
            g(a)
    return f


def _short_ws(size_fn):
    """One byte less than the entry's own size function asks for (never a guessed figure: a size that
    passed the check would launch on the fake pointers)."""
    def f(a):
        from vblade import _lib
        fn = getattr(_lib.load(), size_fn)
        if isinstance(a, dict):
            a["workspace_bytes"] = fn(a["batch"], a["num_heads"], a["max_seqlen_q"]) - 1
        else:
            a.workspace_bytes = fn(ctypes.byref(a)) - 1
    return f


_INV, _UNS = -1, -2
_TOO_LONG = 1025 * 128
# (entry, fault, mutation, return code, vb_last_error())
_REJECTIONS = [
    ("vb_attn_fwd", "null tensor", _set(out=None), _INV, "vb_attn_fwd: missing q/k/v/out"),
    ("vb_attn_fwd", "D=96", _set(D=96), _UNS, "attn: head_dim must be 64 or 128, got 96"),
    ("vb_attn_fwd", "dtype 7", _set(dtype=7), _INV, "attn: unknown dtype"),
    ("vb_attn_fwd", "stride of 4", _set(k_stride=(4, 4, 4)), _INV,
     "vb_attn_fwd: k/v strides must be multiples of 8 elements"),
    ("vb_attn_fwd", "pointer off by 8", _set(v=_PTR + 8), _INV, "vb_attn_fwd: tensors must be 16-byte aligned"),
    ("vb_attn_fwd", "row stride 2^24", _row_stride("k_stride", 1 << 23), _UNS,
     "vb_attn_fwd: k/v/kp/vp row strides must be < 2^24 bytes"),
    ("vb_attn_fwd", "slice >= 2 GiB", _row_stride("v_stride", 1 << 22), _UNS,
     "vb_attn_fwd: a k/v (b,h) slice spans >= 2 GiB"),
    ("vb_attn_fwd", "pooled slice >= 2 GiB", _both(_set(Lkp=330), _row_stride("kp_stride", 1 << 22)), _UNS,
     "vb_attn_fwd: a kp/vp (b,h) slice spans >= 2 GiB"),
    ("vb_attn_fwd", "1025 blocks", _set(Lk=_TOO_LONG), _UNS, "vb_attn_fwd: Lk too long"),
    ("vb_attn_fwd", "pooled without vp", _set(vp=None), _INV, "vb_attn_fwd: pooled branch needs vp and Lkp > 0"),
    ("vb_attn_fwd", "D=96 and dtype 7", _set(D=96, dtype=7), _INV, "attn: unknown dtype"),
    ("vb_attn_fwd", "B=0", _set(B=0), _INV, "vb_attn_fwd: B, H, Lq, D must be positive"),
    ("vb_attn_fwd", "neither branch", _set(use_main=0, kp=None), _INV, "vb_attn_fwd: nothing to attend to"),
    ("vb_attn_fwd", "q stride of 4", _set(q_stride=(4, 4, 4)), _INV,
     "vb_attn_fwd: q/out strides must be multiples of 8 elements"),
    ("vb_attn_fwd", "out stride of 4", _set(out_stride=(4, 4, 4)), _INV,
     "vb_attn_fwd: q/out strides must be multiples of 8 elements"),
    ("vb_attn_fwd", "pooled stride of 4", _set(vp_stride=(4, 4, 4)), _INV,
     "vb_attn_fwd: kp/vp strides must be multiples of 8 elements"),
    ("vb_attn_fwd", "pooled row stride 2^24", _row_stride("kp_stride", 1 << 23), _UNS,
     "vb_attn_fwd: k/v/kp/vp row strides must be < 2^24 bytes"),
    ("vb_attn_fwd", "stride of 4 and pointer off by 8", _set(k_stride=(4, 4, 4), k=_PTR + 8), _INV,
     "vb_attn_fwd: k/v strides must be multiples of 8 elements"),
    # reachable only without the main branch: with it, such an Lk is "too long" first
    ("vb_attn_fwd", "kv_rows with Lk 2^24 pooled only", _set(use_main=0, kv_rows=_PTR, Lk=1 << 24), _UNS,
     "vb_attn_fwd: kv_rows needs Lk < 2^24"),

    ("vb_ml_attn_fwd", "null tensor", _set(level_mask=None), _INV,
     "vb_ml_attn_fwd: missing q/kpyr/vpyr/level_mask/out"),
    ("vb_ml_attn_fwd", "D=96", _set(D=96), _UNS, "vb_ml_attn_fwd: head_dim must be 64 or 128, got 96"),
    ("vb_ml_attn_fwd", "dtype 7", _set(dtype=7), _INV, "vb_ml_attn_fwd: unknown dtype"),
    ("vb_ml_attn_fwd", "stride of 4", _set(out_stride=(4, 4, 4)), _INV,
     "vb_ml_attn_fwd: q/out strides must be multiples of 8 elements"),
    ("vb_ml_attn_fwd", "pointer off by 8", _set(kpyr=_PTR + 8), _INV,
     "vb_ml_attn_fwd: tensors must be 16-byte aligned"),
    ("vb_ml_attn_fwd", "1025 blocks", _set(L=_TOO_LONG), _UNS, "vb_ml_attn_fwd: L too long"),
    ("vb_ml_attn_fwd", "L=0", _set(L=0), _INV, "vb_ml_attn_fwd: B, H, L must be positive"),
    # head_dim before dtype here, the other way round in vb_attn_fwd: both orders are pinned
    ("vb_ml_attn_fwd", "D=96 and dtype 7", _set(D=96, dtype=7), _UNS,
     "vb_ml_attn_fwd: head_dim must be 64 or 128, got 96"),

    ("vb_block_sparse_attn_fwd", "p_dropout=0.1", _set(p_dropout=0.1), _UNS,
     "vb_block_sparse_attn_fwd: p_dropout must be 0"),
    ("vb_block_sparse_attn_fwd", "is_causal=1", _set(is_causal=1), _UNS,
     "vb_block_sparse_attn_fwd: causal/streaming not supported"),
    ("vb_block_sparse_attn_fwd", "mask_head_mode=7", _set(mask_head_mode=7), _INV,
     "vb_block_sparse_attn_fwd: unknown mask_head_mode"),
    ("vb_block_sparse_attn_fwd", "null tensor", _set(cu_k=None), _INV, "vb_block_sparse_attn_fwd: null tensor"),
    ("vb_block_sparse_attn_fwd", "batch=0", _set(batch=0), _INV, "vb_block_sparse_attn_fwd: bad sizes"),
    ("vb_block_sparse_attn_fwd", "1025 blocks", _set(max_seqlen_k=_TOO_LONG), _UNS,
     "vb_block_sparse_attn_fwd: max_seqlen_k too long"),
    ("vb_block_sparse_attn_fwd", "D=96", _set(head_dim=96), _UNS, "attn: head_dim must be 64 or 128, got 96"),
    ("vb_block_sparse_attn_fwd", "dtype 7", _set(dtype=7), _INV, "attn: unknown dtype"),
    ("vb_block_sparse_attn_fwd", "k slice >= 2 GiB", _set(num_heads=1 << 16), _UNS,
     "vb_block_sparse_attn_fwd: a sequence's k/v span >= 2 GiB"),

    ("vb_attn_bwd", "null tensor", _set(dv=None), _INV, "vb_attn_bwd: missing tensor"),
    ("vb_attn_bwd", "D=96", _set(D=96), _UNS, "vb_attn_bwd: head_dim must be 64 or 128, got 96"),
    ("vb_attn_bwd", "dtype 7", _set(dtype=7), _INV, "vb_attn_bwd: unknown dtype"),
    ("vb_attn_bwd", "stride of 4", _set(dk_stride=(4, 4, 4)), _INV,
     "vb_attn_bwd: strides must be multiples of 8 elements"),
    ("vb_attn_bwd", "pooled stride of 4", _set(out2_stride=(4, 4, 4)), _INV,
     "vb_attn_bwd: strides must be multiples of 8 elements"),
    ("vb_attn_bwd", "pointer off by 8", _set(dout=_PTR + 8), _INV, "vb_attn_bwd: tensors must be 16-byte aligned"),
    ("vb_attn_bwd", "pooled pointer off by 8", _set(vp=_PTR + 8), _INV,
     "vb_attn_bwd: tensors must be 16-byte aligned"),
    ("vb_attn_bwd", "row stride 2^24", _row_stride("k_stride", 1 << 24), _UNS,
     "vb_attn_bwd: a k/v/kp/vp (b,h) slice spans >= 2 GiB"),
    ("vb_attn_bwd", "q slice >= 2 GiB", _row_stride("dout_stride", 1 << 23), _UNS,
     "vb_attn_bwd: a q/dout (b,h) slice spans >= 2 GiB"),
    ("vb_attn_bwd", "k slice >= 2 GiB", _row_stride("v_stride", 1 << 22), _UNS,
     "vb_attn_bwd: a k/v/kp/vp (b,h) slice spans >= 2 GiB"),
    ("vb_attn_bwd", "1025 blocks", _set(Lq=_TOO_LONG), _UNS, "vb_attn_bwd: sequence too long"),
    ("vb_attn_bwd", "unknown kernel_select bit", _set(kernel_select=8), _INV,
     "vb_attn_bwd: unknown kernel_select bits"),
    ("vb_attn_bwd", "missing workspace", _set(workspace=None), _INV,
     "vb_attn_bwd: workspace missing or smaller than vb_attn_bwd_workspace_size()"),
    ("vb_attn_bwd", "short workspace", _short_ws("vb_attn_bwd_workspace_size"), _INV,
     "vb_attn_bwd: workspace missing or smaller than vb_attn_bwd_workspace_size()"),
    ("vb_attn_bwd", "pooled without vp", _set(vp=None), _INV,
     "vb_attn_bwd: pooled branch needs vp, Lkp, out2, lse2 and pool_gap"),
    ("vb_attn_bwd", "Lkp * gap < Lk", _set(pool_gap=7), _INV, "vb_attn_bwd: Lkp * pool_gap must cover Lk"),
    ("vb_attn_bwd", "D=96 and dtype 7", _set(D=96, dtype=7), _UNS,
     "vb_attn_bwd: head_dim must be 64 or 128, got 96"),
    ("vb_attn_bwd", "stride of 4 and pointer off by 8", _set(q_stride=(4, 4, 4), q=_PTR + 8), _INV,
     "vb_attn_bwd: strides must be multiples of 8 elements"),
    ("vb_attn_bwd", "short workspace and slice >= 2 GiB",
     _both(_short_ws("vb_attn_bwd_workspace_size"), _row_stride("k_stride", 1 << 22)), _INV,
     "vb_attn_bwd: workspace missing or smaller than vb_attn_bwd_workspace_size()"),

    ("vb_block_sparse_attn_bwd", "null tensor", _set(cu_k=None), _INV, "vb_block_sparse_attn_bwd: null tensor"),
    ("vb_block_sparse_attn_bwd", "D=96", _set(head_dim=96), _UNS,
     "vb_block_sparse_attn_bwd: head_dim must be 64 or 128"),
    ("vb_block_sparse_attn_bwd", "dtype 7", _set(dtype=7), _INV, "vb_block_sparse_attn_bwd: unknown dtype"),
    ("vb_block_sparse_attn_bwd", "pointer off by 8", _set(dk=_PTR + 8), _INV,
     "vb_block_sparse_attn_bwd: tensors must be 16-byte aligned"),
    ("vb_block_sparse_attn_bwd", "q slice >= 2 GiB", _set(num_heads=1 << 17), _UNS,
     "vb_block_sparse_attn_bwd: a sequence's q/dout span >= 2 GiB"),
    ("vb_block_sparse_attn_bwd", "k slice >= 2 GiB", _set(num_heads=1 << 16), _UNS,
     "vb_block_sparse_attn_bwd: a sequence's k/v span >= 2 GiB"),
    ("vb_block_sparse_attn_bwd", "1025 blocks", _set(max_seqlen_k=_TOO_LONG), _UNS,
     "vb_block_sparse_attn_bwd: sequence too long"),
    ("vb_block_sparse_attn_bwd", "missing workspace", _set(workspace=None), _INV,
     "vb_block_sparse_attn_bwd: workspace missing or too small"),
    ("vb_block_sparse_attn_bwd", "short workspace", _short_ws("vb_block_sparse_attn_bwd_workspace_size"), _INV,
     "vb_block_sparse_attn_bwd: workspace missing or too small"),

    ("vb_ml_attn_bwd", "null tensor", _set(lse=None), _INV, "vb_ml_attn_bwd: missing tensor"),
    ("vb_ml_attn_bwd", "D=96", _set(D=96), _UNS, "vb_ml_attn_bwd: head_dim must be 64 or 128, got 96"),
    ("vb_ml_attn_bwd", "dtype 7", _set(dtype=7), _INV, "vb_ml_attn_bwd: unknown dtype"),
    ("vb_ml_attn_bwd", "stride of 4", _set(dq_stride=(4, 4, 4)), _INV,
     "vb_ml_attn_bwd: strides must be multiples of 8 elements"),
    ("vb_ml_attn_bwd", "pointer off by 8", _set(vpyr=_PTR + 8), _INV,
     "vb_ml_attn_bwd: tensors must be 16-byte aligned"),
    ("vb_ml_attn_bwd", "slice >= 2 GiB", _row_stride("q_stride", 1 << 23), _UNS,
     "vb_ml_attn_bwd: a q/dout (b,h) slice spans >= 2 GiB"),
    ("vb_ml_attn_bwd", "1025 blocks", _set(L=_TOO_LONG), _UNS, "vb_ml_attn_bwd: sequence too long"),
    ("vb_ml_attn_bwd", "unknown kernel_select bit", _set(kernel_select=8), _INV,
     "vb_ml_attn_bwd: unsupported kernel_select bits (the multi-level dQ has one ring)"),
    ("vb_ml_attn_bwd", "VB_BWD_SEL_DQ_RING4", _set(kernel_select=4), _INV,
     "vb_ml_attn_bwd: unsupported kernel_select bits (the multi-level dQ has one ring)"),
    ("vb_ml_attn_bwd", "missing workspace", _set(workspace=None), _INV,
     "vb_ml_attn_bwd: workspace missing or smaller than vb_ml_attn_bwd_workspace_size()"),
    ("vb_ml_attn_bwd", "short workspace", _short_ws("vb_ml_attn_bwd_workspace_size"), _INV,
     "vb_ml_attn_bwd: workspace missing or smaller than vb_ml_attn_bwd_workspace_size()"),
]
_VALID = {"vb_attn_fwd": _fwd_args, "vb_ml_attn_fwd": _ml_fwd_args, "vb_attn_bwd": _bwd_args,
          "vb_block_sparse_attn_fwd": _bs_fwd_args, "vb_block_sparse_attn_bwd": _bs_bwd_args,
          "vb_ml_attn_bwd": _ml_bwd_args}
_POSITIONAL = {"vb_block_sparse_attn_fwd": _BSF_NAMES, "vb_block_sparse_attn_bwd": _BS_NAMES}


def _call(lib, entry, a):
    if isinstance(a, dict):
        return getattr(lib, entry)(*(a[n] for n in _POSITIONAL[entry]))
    return getattr(lib, entry)(ctypes.byref(a), None)


@pytest.mark.parametrize("entry,fault,mutate,code,message", _REJECTIONS,
                         ids=[f"{e}-{f}".replace(" ", "_") for e, f, *_ in _REJECTIONS])
def test_attention_entries_reject_one_fault_at_a_time(lib, entry, fault, mutate, code, message):
    a = _VALID[entry]()
    mutate(a)
    rc = _call(lib, entry, a)
    got = lib.vb_last_error().decode()
    print(f"{entry} [{fault}]: {rc} {got!r}")
    assert (rc, got) == (code, message)


def test_forward_entries_reject_null_args(lib):
    """A NULL args struct is refused by the first check of either struct-taking forward entry."""
    for entry in ("vb_attn_fwd", "vb_ml_attn_fwd"):
        rc = getattr(lib, entry)(None, None)
        got = lib.vb_last_error().decode()
        print(f"{entry} [null args]: {rc} {got!r}")
        assert (rc, got) == (_INV, f"{entry}: null args")


# vb_attn_bwd_workspace_size at B=1, H=2: (Lq, Lk, D, q_rows, pooled) -> bytes; pooled Lkp = ceil(Lk / 8)
_BWD_WS = {
    (128, 128, 64, False, False): 4096,
    (128, 128, 64, False, True): 20480,
    (128, 128, 64, True, False): 69632,
    (128, 128, 64, True, True): 86016,
    (128, 128, 128, False, False): 4096,
    (128, 128, 128, False, True): 36864,
    (128, 128, 128, True, False): 135168,
    (128, 128, 128, True, True): 167936,
    (200, 330, 64, False, False): 8192,
    (200, 330, 64, False, True): 137216,
    (200, 330, 64, True, False): 110592,
    (200, 330, 64, True, True): 239616,
    (200, 330, 128, False, False): 8192,
    (200, 330, 128, False, True): 266240,
    (200, 330, 128, True, False): 212992,
    (200, 330, 128, True, True): 471040,
    (1000, 1000, 64, False, False): 32768,
    (1000, 1000, 64, False, True): 1184768,
    (1000, 1000, 64, True, False): 544768,
    (1000, 1000, 64, True, True): 1696768,
    (1000, 1000, 128, False, False): 32768,
    (1000, 1000, 128, False, True): 2336768,
    (1000, 1000, 128, True, False): 1056768,
    (1000, 1000, 128, True, True): 3360768,
}
_BS_BWD_WS = 24576   # vb_block_sparse_attn_bwd_workspace_size(2, 3, 200)
# vb_ml_attn_bwd_workspace_size at B=1, H=2: (L, D, rows) -> bytes
_ML_BWD_WS = {
    (200, 64, False): 237568,
    (200, 64, True): 339968,
    (200, 128, False): 466944,
    (200, 128, True): 671744,
    (384, 64, False): 356352,
    (384, 64, True): 552960,
    (384, 128, False): 700416,
    (384, 128, True): 1093632,
}


def _bwd_ws_cases():
    return [(lq, lk, d, rows, pooled) for lq, lk in ((128, 128), (200, 330), (1000, 1000))
            for d in (64, 128) for rows in (False, True) for pooled in (False, True)]


def _ml_bwd_ws_cases():
    return [(L, d, rows) for L in (200, 384) for d in (64, 128) for rows in (False, True)]


def _bwd_ws(lib, lq, lk, d, rows, pooled):
    from vblade import _lib
    a = _lib.BwdArgs()
    a.B, a.H, a.Lq, a.Lk, a.D = _B, _H, lq, lk, d
    a.q_rows = _PTR if rows else None
    if pooled:
        a.kp, a.Lkp = _PTR, (lk + 7) // 8
    return lib.vb_attn_bwd_workspace_size(ctypes.byref(a))


def _ml_bwd_ws(lib, L, d, rows):
    from vblade import _lib
    a = _lib.MlBwdArgs()
    a.B, a.H, a.L, a.D = _B, _H, L, d
    a.rows = _PTR if rows else None
    return lib.vb_ml_attn_bwd_workspace_size(ctypes.byref(a))


def test_backward_workspace_sizes_are_pinned(lib):
    """psplit = 1 at Lq = 128 (one q-block) and > 1 at the longer ones (2 and 8 q-range partials)."""
    assert set(_BWD_WS) == set(_bwd_ws_cases()) and set(_ML_BWD_WS) == set(_ml_bwd_ws_cases())
    got = {c: _bwd_ws(lib, *c) for c in _bwd_ws_cases()}
    print(got)
    assert got == _BWD_WS
    assert lib.vb_block_sparse_attn_bwd_workspace_size(2, 3, 200) == _BS_BWD_WS
    got = {c: _ml_bwd_ws(lib, *c) for c in _ml_bwd_ws_cases()}
    print(got)
    assert got == _ML_BWD_WS
