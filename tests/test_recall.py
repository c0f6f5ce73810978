"""CPU: the attention-recall probe without a GPU — the ctypes mirror of vb_recall_args matches the
header, every host check of vb_mask_recall returns its code and message (each call below carries a
fault, so nothing is ever launched on the fake pointers), ops.mask_recall range-checks host probe
positions, the module's options validate, and the restatement (tests/recall_ref.py) keeps its own
invariants."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import recall_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vblade.h")
_PTR, _WS = 1 << 20, 1 << 24


def test_recall_args_layout_matches_header():
    from vblade._lib import RecallArgs
    fields = [f[0] for f in RecallArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vb_recall_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(vb_recall_args, {f}));' for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "l")
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == ctypes.sizeof(RecallArgs)
    for f in fields:
        assert int(got[f]) == getattr(RecallArgs, f).offset, f


def _args(lib, B=2, H=3, L=1000, D=64, S=30):
    from vblade import _lib
    a = _lib.RecallArgs()
    a.q = a.k = a.rows = a.probe_pos = a.block_mask = a.recall = a.oracle_recall = _PTR
    a.B, a.H, a.L, a.D, a.S = B, H, L, D, S
    a.q_stride = a.k_stride = (H * L * D, L * D, D)
    nb = (L + 127) // 128
    a.mask_stride = (H * nb * nb, nb * nb, nb)
    a.workspace = _WS
    a.workspace_bytes = lib.vb_mask_recall_workspace_size(ctypes.byref(a))
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _short_ws(a):
    a.workspace_bytes -= 1


_INV, _UNS = -1, -2
# (fault, constructor arguments, mutation, return code, text vb_last_error() must hold)
_REJECTIONS = [
    ("null q", {}, _set(q=None), _INV, "vb_mask_recall: null argument"),
    ("null k", {}, _set(k=None), _INV, "vb_mask_recall: null argument"),
    ("null probe_pos", {}, _set(probe_pos=None), _INV, "vb_mask_recall: null argument"),
    ("null block_mask", {}, _set(block_mask=None), _INV, "vb_mask_recall: null argument"),
    ("null recall", {}, _set(recall=None), _INV, "vb_mask_recall: null argument"),
    ("B = 0", {}, _set(B=0), _INV, "vb_mask_recall: bad sizes"),
    ("H < 0", {}, _set(H=-1), _INV, "vb_mask_recall: bad sizes"),
    ("L = 0", {}, _set(L=0), _INV, "vb_mask_recall: bad sizes"),
    ("S = 0", {}, _set(S=0), _INV, "vb_mask_recall: S must be in [1, 64]"),
    ("S = 65", dict(S=65), None, _INV, "vb_mask_recall: S must be in [1, 64]"),
    ("dtype 7", {}, _set(dtype=7), _INV, "vb_mask_recall: unknown dtype"),
    ("q stride of 4", {}, _set(q_stride=(4, 4, 4)), _INV,
     "vb_mask_recall: q/k strides must be non-negative multiples of 8"),
    ("negative k stride", {}, _set(k_stride=(-64, 64, 64)), _INV,
     "vb_mask_recall: q/k strides must be non-negative multiples of 8"),
    ("negative mask stride", {}, _set(mask_stride=(64, -64, 8)), _INV,
     "vb_mask_recall: mask strides must be non-negative"),
    ("q off by 8", {}, _set(q=_PTR + 8), _INV, "vb_mask_recall: q and k must be 16-byte aligned"),
    ("k off by 2", {}, _set(k=_PTR + 2), _INV, "vb_mask_recall: q and k must be 16-byte aligned"),
    ("missing workspace", {}, _set(workspace=None), _INV,
     "vb_mask_recall: workspace missing or smaller than vb_mask_recall_workspace_size() (12960 bytes)"),
    ("short workspace", {}, _short_ws, _INV,
     "vb_mask_recall: workspace missing or smaller than vb_mask_recall_workspace_size() (12960 bytes)"),
    ("workspace off by 8", {}, _set(workspace=_WS + 8), _INV,
     "vb_mask_recall: workspace missing or smaller than vb_mask_recall_workspace_size() (12960 bytes)"),
    ("D = 96", dict(D=96), None, _UNS, "vb_mask_recall: head_dim must be 64 or 128"),
    ("L = 131073", dict(B=1, H=1, L=131073), None, _UNS, "vb_mask_recall: sequence too long (L <= 131072)"),
    # (L-1) * 16384 elements * 2 bytes >= 2 GiB
    ("k slice >= 2 GiB", dict(B=1, H=1, L=131072, D=128), _set(k_stride=(1 << 40, 1 << 34, 1 << 14)), _UNS,
     "vb_mask_recall: a q/k (b,h) slice spans >= 2 GiB"),
    ("q slice >= 2 GiB", dict(B=1, H=1, L=131072, D=128), _set(q_stride=(1 << 40, 1 << 34, 1 << 14)), _UNS,
     "vb_mask_recall: a q/k (b,h) slice spans >= 2 GiB"),
]


@pytest.mark.parametrize("fault,kw,mutate,code,message", _REJECTIONS, ids=[r[0].replace(" ", "_") for r in _REJECTIONS])
def test_host_checks_reject_one_fault_at_a_time(fault, kw, mutate, code, message):
    from vblade import _lib
    lib = _lib.load()
    a = _args(lib, **kw)
    if mutate is not None:
        mutate(a)
    rc = lib.vb_mask_recall(ctypes.byref(a), None)
    got = lib.vb_last_error().decode()
    print(f"[{fault}]: {rc} {got!r}")
    assert (rc, got) == (code, message)


def test_null_args_and_workspace_arithmetic():
    from vblade import _lib
    lib = _lib.load()
    assert lib.vb_mask_recall(None, None) == _lib.VB_ERR_INVALID
    assert lib.vb_mask_recall_workspace_size(None) == 0
    # B*H*S rows of nb (maximum, sum) pairs, then the rows' two results; a multiple of 16 bytes
    assert _args(lib).workspace_bytes == (6 * 30 * 8 * 2 + 6 * 30 * 2) * 4 == 12960
    assert _args(lib, B=1, H=1, L=129, S=1).workspace_bytes == 32        # (2*2 + 2) * 4 = 24 -> 32
    # at most 512 KiB of pairs per head
    assert _args(lib, B=1, H=1, L=131072, S=64).workspace_bytes == 64 * 1024 * 8 + 64 * 8
    a = _args(lib)
    a.S = 0
    assert lib.vb_mask_recall_workspace_size(ctypes.byref(a)) == 0


def test_ops_refuse_cpu_tensors_and_bad_probe_positions():
    from vblade import ops
    q = torch.zeros(1, 1, 300, 64, dtype=torch.bfloat16)
    mask = torch.ones(1, 1, 3, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.mask_recall(q, q, mask, [0, 5])
    with pytest.raises(ValueError, match="shape"):
        ops.mask_recall(q, q[:, :, :200], mask, [0, 5])
    for pos in ([0, 300], [-1, 4], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError, match="probe_pos"):
            ops.recall_probe_pos(pos, 300, "cpu")
    with pytest.raises(ValueError, match="one-dimensional"):
        ops.recall_probe_pos(torch.zeros(2, 2, dtype=torch.int32), 300, "cpu")
    got = ops.recall_probe_pos(np.array([0, 299]), 300, "cpu")
    assert got.dtype == torch.int32 and got.tolist() == [0, 299]
    assert ops.recall_probe_pos(torch.tensor([5, 7]), 300, "cpu").dtype == torch.int32


def test_module_option_validation():
    import vblade
    small = dict(width=16, height=12, depth=6, text_length=26)
    video = 16 * 12 * 6
    m = vblade.AdaptiveBlockSparseAttn("cog", probe="recall", **small)
    p = m.probe_pos
    assert p.dtype == torch.int32 and p.numel() == 30 and len(set(p.tolist())) == 30
    assert int(p.min()) >= 0 and int(p.max()) < video                 # reordered positions of the video part
    assert "probe_pos" not in m.state_dict()
    assert m.last_recall is None and m.last_oracle_recall is None and m.recall is None
    again = vblade.AdaptiveBlockSparseAttn("cog", probe="recall", **small)
    assert torch.equal(again.probe_pos, p)                             # drawn from the seed, not the global RNG
    gen = torch.Generator().manual_seed(0)
    assert torch.equal(p.long(), torch.randperm(video, generator=gen)[:30])
    other = vblade.AdaptiveBlockSparseAttn("cog", probe="recall", probe_seed=1, probe_samples=64, **small)
    assert other.probe_pos.numel() == 64 and not torch.equal(other.probe_pos[:30], p)
    plain = vblade.AdaptiveBlockSparseAttn("cog", **small)
    assert plain.probe is None and plain.last_recall is None and not hasattr(plain, "probe_pos")
    assert vblade.AdaptiveBlockSparseAttn("wan", probe="recall", probe_every=3).probe_every == 3
    for bad in (dict(probe="mass"), dict(probe="recall", probe_samples=0), dict(probe="recall", probe_samples=65),
                dict(probe="recall", probe_every=0), dict(probe="recall", probe_every=-2)):
        with pytest.raises(ValueError):
            vblade.AdaptiveBlockSparseAttn("cog", **small, **bad)
    with pytest.raises(ValueError, match="video tokens"):
        vblade.AdaptiveBlockSparseAttn("cog", probe="recall", probe_samples=40, width=3, height=3, depth=3,
                                       text_length=26)
    with pytest.raises(TypeError):
        vblade.AdaptiveBlockSparseAttn("cog", probe_sample=3)


def _case(L, D=64, B=2, H=3, seed=0):
    from vblade import ops
    S = ops.RECALL_MAX_SAMPLES                      # the largest probe count the library takes
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, D, generator=g) * torch.linspace(0.5, 2.5, H).view(1, H, 1, 1)
    k = torch.randn(B, H, L, D, generator=g)
    pos = torch.randint(0, L, (S,), generator=g).numpy()
    nb = (L + 127) // 128
    mask = (torch.rand(B, H, nb, nb, generator=g) < 0.4).to(torch.uint8)
    return q.bfloat16(), k.bfloat16(), mask, pos, nb


@pytest.mark.parametrize("L", [128, 129, 1000])
def test_restatement_invariants(L):
    q, k, mask, pos, nb = _case(L)
    rows = torch.randperm(L, generator=torch.Generator().manual_seed(1)).numpy()
    for dtype in (torch.float64, torch.float32):
        for r in (None, rows):
            got = R.recall(q, k, mask, pos, rows=r, dtype=dtype)
            assert (got["row_recall"] <= got["row_oracle"] * (1 + 1e-6)).all()
            assert (got["row_oracle"] <= 1 + 1e-6).all() and (got["row_recall"] >= 0).all()
            assert np.array_equal(got["row_kept"], mask[:, :, pos // 128].sum(-1).numpy())
            ones = R.recall(q, k, torch.ones_like(mask), pos, rows=r, dtype=dtype)
            assert (ones["row_recall"] == 1).all() and (ones["row_oracle"] == 1).all() and (ones["recall"] == 1).all()
            assert (ones["row_kept"] == nb).all()
            empty = mask.clone()
            empty[1, 2, pos[0] // 128] = 0
            e = R.recall(q, k, empty, pos, rows=r, dtype=dtype)
            assert e["row_recall"][1, 2, 0] == 0 and e["row_oracle"][1, 2, 0] == 0 and e["row_kept"][1, 2, 0] == 0
    # the oracle of a mask that holds the heaviest blocks is its recall; out-of-range positions clamp
    E = R.block_masses(q, k, pos)
    top = R.top_mask_row(E, min(3, nb))
    full = torch.zeros(2, 3, nb, nb, dtype=torch.bool)
    full[:, :, pos[0] // 128] = top[:, :, 0]
    t = R.recall(q, k, full, pos[:1])
    assert np.allclose(t["row_recall"], t["row_oracle"], rtol=1e-14, atol=0)
    assert (t["row_kept"] == min(3, nb)).all()
    a, b = R.recall(q, k, mask, [-5, L + 7]), R.recall(q, k, mask, [0, L - 1])
    assert np.array_equal(a["row_recall"], b["row_recall"])
    # a permutation of the keys inside the blocks leaves the block masses alone only when the blocks
    # keep their keys: the identity rows and None agree
    same = R.recall(q, k, mask, pos, rows=np.arange(L))
    assert np.array_equal(same["row_recall"], R.recall(q, k, mask, pos)["row_recall"])
