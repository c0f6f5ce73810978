"""CPU: the surface of the joint training path. The module option grad_combine (default "reference",
"joint" accepted, anything else refused, both setters forward it), and vb_attn_bwd_joint's symbol and
argument validation: every case below is refused by a host check, so nothing is launched and the fake
(non-null, 16-byte aligned) pointers are never dereferenced."""
import ctypes
import os
import re

import pytest
import torch.nn as nn

import vblade
from conftest import ROOT
from test_patch import _CogModel, _WanModel

SMALL = dict(width=12, height=8, depth=6, text_length=26, log_every=0)


# ---------------------------------------------------------------------------------------------
# the module option
# ---------------------------------------------------------------------------------------------
def test_grad_combine_defaults_to_the_reference_gradient():
    assert vblade.AdaptiveBlockSparseAttn("cog", **SMALL).grad_combine == "reference"
    assert vblade.AdaptiveBlockSparseAttn("wan").grad_combine == "reference"


def test_grad_combine_joint_is_accepted_and_other_values_are_refused():
    assert vblade.AdaptiveBlockSparseAttn("cog", grad_combine="joint", **SMALL).grad_combine == "joint"
    assert vblade.AdaptiveBlockSparseAttn("cog", grad_combine="reference", **SMALL).grad_combine == "reference"
    for bad in ("fused", "exact", None, 1):
        with pytest.raises(ValueError, match="grad_combine"):
            vblade.AdaptiveBlockSparseAttn("cog", grad_combine=bad, **SMALL)


def test_both_setters_forward_grad_combine():
    inner = vblade.set_block_sparse_attn_cogvideox(_CogModel(), grad_combine="joint")
    assert inner.variant == "cog" and inner.grad_combine == "joint"
    inner = vblade.set_adaptive_block_sparse_attn_wanx(_WanModel(), grad_combine="joint")
    assert inner.variant == "wan" and inner.grad_combine == "joint"
    assert vblade.set_block_sparse_attn_cogvideox(_CogModel()).grad_combine == "reference"
    with pytest.raises(ValueError, match="grad_combine"):
        vblade.set_adaptive_block_sparse_attn_wanx(_WanModel(), grad_combine="both")


def test_autograd_and_ops_expose_the_joint_calls():
    from vblade import autograd, ops
    assert callable(autograd.adaptive_joint_attention) and callable(ops.attention_bwd_joint)
    assert isinstance(vblade.AdaptiveBlockSparseAttn("cog", **SMALL), nn.Module)


# ---------------------------------------------------------------------------------------------
# vb_attn_bwd_joint
# ---------------------------------------------------------------------------------------------
_PTR, _WS = 1 << 20, 1 << 24
_B, _H, _L, _LK, _LKP, _GAP, _D = 1, 2, 200, 330, 42, 8, 64
_INV, _UNS = -1, -2
ENTRY = "vb_attn_bwd_joint"


@pytest.fixture(scope="module")
def lib():
    from vblade import _lib
    return _lib.load()


def _st(L, D=_D, H=_H):
    return (H * L * D, L * D, D)


def _args():
    from vblade import _lib
    a = _lib.BwdArgs()
    a.q = a.k = a.v = a.out = a.lse = a.dout = a.dq = a.dk = a.dv = _PTR
    a.kp = a.vp = _PTR
    a.q_stride = a.out_stride = a.dout_stride = a.dq_stride = _st(_L)
    a.k_stride = a.v_stride = a.dk_stride = a.dv_stride = _st(_LK)
    a.kp_stride = a.vp_stride = _st(_LKP)
    a.Lkp, a.pool_gap = _LKP, _GAP
    a.B, a.H, a.Lq, a.Lk, a.D = _B, _H, _L, _LK, _D
    a.workspace, a.workspace_bytes = _WS, 1 << 62
    return a


def test_symbol_is_declared_exported_and_bound(lib):
    from vblade import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vblade.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+vb_attn_bwd_joint\s*\(\s*const\s+vb_attn_bwd_args\s*\*\s*args\s*,\s*float\s+"
                     r"pool_log_bias\s*,\s*void\s*\*\s*stream\s*\)\s*;", header)
    assert hasattr(lib, ENTRY)
    restype, argtypes = _lib.SIGNATURES[ENTRY]
    assert restype is ctypes.c_int
    assert argtypes == [ctypes.POINTER(_lib.BwdArgs), ctypes.c_float, ctypes.c_void_p]
    assert lib.vb_abi_version() == 4           # the entry takes the struct unchanged


def test_null_args_are_refused(lib):
    assert lib.vb_attn_bwd_joint(None, 0.0, None) == _INV
    assert lib.vb_last_error().decode() == "vb_attn_bwd_joint: null args"


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _short_ws(a):
    from vblade import _lib
    a.workspace_bytes = _lib.load().vb_attn_bwd_workspace_size(ctypes.byref(a)) - 1


_POOL = "vb_attn_bwd_joint: needs the pooled keys kp, vp, Lkp > 0 and pool_gap > 0"
_NULLS = "vb_attn_bwd_joint: out2, lse2 and alpha must be NULL (one softmax has one output and one LSE)"
_WSMSG = "vb_attn_bwd_joint: workspace missing or smaller than vb_attn_bwd_workspace_size()"
REJECTIONS = [
    ("missing kp", _set(kp=None), _INV, _POOL),
    ("missing vp", _set(vp=None), _INV, _POOL),
    ("Lkp 0", _set(Lkp=0), _INV, _POOL),
    ("pool_gap 0", _set(pool_gap=0), _INV, _POOL),
    ("out2 given", _set(out2=_PTR), _INV, _NULLS),
    ("lse2 given", _set(lse2=_PTR), _INV, _NULLS),
    ("alpha given", _set(alpha=_PTR), _INV, _NULLS),
    ("short workspace", _short_ws, _INV, _WSMSG),
    ("missing workspace", _set(workspace=None), _INV, _WSMSG),
    ("D=96", _set(D=96), _UNS, "vb_attn_bwd_joint: head_dim must be 64 or 128, got 96"),
    # vb_attn_bwd's order: the shape and tensor checks come before the pooled ones
    ("D=96 and missing kp", _set(D=96, kp=None), _UNS, "vb_attn_bwd_joint: head_dim must be 64 or 128, got 96"),
    ("null tensor and out2 given", _set(dv=None, out2=_PTR), _INV, "vb_attn_bwd_joint: missing tensor"),
    ("Lkp * gap < Lk", _set(pool_gap=7), _INV, "vb_attn_bwd_joint: Lkp * pool_gap must cover Lk"),
    ("unknown kernel_select bit", _set(kernel_select=8), _INV, "vb_attn_bwd_joint: unknown kernel_select bits"),
]


@pytest.mark.parametrize("fault,mutate,code,message", REJECTIONS, ids=[r[0].replace(" ", "_") for r in REJECTIONS])
def test_joint_entry_rejects_one_fault_at_a_time(lib, fault, mutate, code, message):
    a = _args()
    mutate(a)
    rc = lib.vb_attn_bwd_joint(ctypes.byref(a), 2.0, None)
    got = lib.vb_last_error().decode()
    print(f"{ENTRY} [{fault}]: {rc} {got!r}")
    assert (rc, got) == (code, message)


def test_workspace_size_serves_both_entries(lib):
    """vb_attn_bwd_workspace_size reads kp and Lkp, never out2: the joint call's struct (out2 NULL) asks
    for what the two-branch call's does."""
    a = _args()
    joint = lib.vb_attn_bwd_workspace_size(ctypes.byref(a))
    a.out2 = a.lse2 = a.alpha = _PTR
    assert lib.vb_attn_bwd_workspace_size(ctypes.byref(a)) == joint == 137216   # test_abi's pinned (200, 330, 64, False, True)
