"""CPU: the output-fidelity probe without a GPU — the ctypes mirror of vb_fidelity_args matches the
header, every host check of vb_attn_fidelity returns its code and message (each call below carries a
fault, so nothing is ever launched on the fake pointers), the workspace size is the header's formula,
ops.attn_fidelity refuses CPU tensors, both modules' options validate, and the restatement
(tests/fidelity_ref.py) keeps its own invariants."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import fidelity_ref as F
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vblade.h")
_PTR, _WS = 1 << 20, 1 << 24


def test_fidelity_args_layout_matches_header():
    from vblade._lib import FidelityArgs
    fields = [f[0] for f in FidelityArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vb_fidelity_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(vb_fidelity_args, {f}));' for f in fields]
    lines.append('printf("max %d\\nchunk %d\\n", VB_FIDELITY_MAX_SAMPLES, VB_FIDELITY_CHUNK);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "l")
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == ctypes.sizeof(FidelityArgs)
    for f in fields:
        assert int(got[f]) == getattr(FidelityArgs, f).offset, f
    from vblade import _lib, ops
    assert int(got["max"]) == _lib.VB_FIDELITY_MAX_SAMPLES == ops.FIDELITY_MAX_SAMPLES == 64
    assert int(got["chunk"]) == _lib.VB_FIDELITY_CHUNK == F.CHUNK


def _args(lib, B=2, H=3, L=1000, D=64, S=30):
    from vblade import _lib
    a = _lib.FidelityArgs()
    a.q = a.k = a.v = a.out = a.probe_rows = a.err = a.sig = a.peak = _PTR
    a.B, a.H, a.L, a.D, a.S = B, H, L, D, S
    a.q_stride = a.k_stride = a.v_stride = a.out_stride = (H * L * D, L * D, D)
    a.workspace = _WS
    a.workspace_bytes = lib.vb_attn_fidelity_workspace_size(ctypes.byref(a))
    return a


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _short_ws(a):
    a.workspace_bytes -= 1


_INV, _UNS = -1, -2
_NULL = "vb_attn_fidelity: null argument"
_STRIDE = "vb_attn_fidelity: q/k/v/out strides must be non-negative multiples of 8"
_ALIGN = "vb_attn_fidelity: q, k, v and out must be 16-byte aligned"
_WSMSG = "vb_attn_fidelity: workspace missing or smaller than vb_attn_fidelity_workspace_size() (97200 bytes)"
_SLICE = "vb_attn_fidelity: a q/k/v/out (b,h) slice spans >= 2 GiB"
_BIGROW = (1 << 40, 1 << 34, 1 << 14)    # (L-1) * 16384 elements * 2 bytes >= 2 GiB at L = 131072
# (fault, constructor arguments, mutation, return code, text vb_last_error() must hold)
_REJECTIONS = (
    [(f"null {n}", {}, _set(**{n: None}), _INV, _NULL) for n in ("q", "k", "v", "out", "probe_rows", "err", "sig")] + [
        ("B = 0", {}, _set(B=0), _INV, "vb_attn_fidelity: bad sizes"),
        ("H < 0", {}, _set(H=-1), _INV, "vb_attn_fidelity: bad sizes"),
        ("L = 0", {}, _set(L=0), _INV, "vb_attn_fidelity: bad sizes"),
        ("S = 0", {}, _set(S=0), _INV, "vb_attn_fidelity: S must be in [1, 64]"),
        ("S = 65", dict(S=65), None, _INV, "vb_attn_fidelity: S must be in [1, 64]"),
        ("dtype 7", {}, _set(dtype=7), _INV, "vb_attn_fidelity: unknown dtype"),
        ("q stride of 4", {}, _set(q_stride=(4, 4, 4)), _INV, _STRIDE),
        ("negative k stride", {}, _set(k_stride=(-64, 64, 64)), _INV, _STRIDE),
        ("v row stride of 12", {}, _set(v_stride=(3 * 1000 * 64, 1000 * 64, 12)), _INV, _STRIDE),
        ("negative out stride", {}, _set(out_stride=(64, -64, 64)), _INV, _STRIDE),
        ("q off by 8", {}, _set(q=_PTR + 8), _INV, _ALIGN),
        ("k off by 2", {}, _set(k=_PTR + 2), _INV, _ALIGN),
        ("v off by 4", {}, _set(v=_PTR + 4), _INV, _ALIGN),
        ("out off by 8", {}, _set(out=_PTR + 8), _INV, _ALIGN),
        ("missing workspace", {}, _set(workspace=None), _INV, _WSMSG),
        ("short workspace", {}, _short_ws, _INV, _WSMSG),
        ("workspace off by 8", {}, _set(workspace=_WS + 8), _INV, _WSMSG),
        ("D = 96", dict(D=96), None, _UNS, "vb_attn_fidelity: head_dim must be 64 or 128"),
        ("L = 131073", dict(B=1, H=1, L=131073), None, _UNS, "vb_attn_fidelity: sequence too long (L <= 131072)"),
    ] + [(f"{n} slice >= 2 GiB", dict(B=1, H=1, L=131072, D=128), _set(**{f"{n}_stride": _BIGROW}), _UNS, _SLICE)
         for n in ("q", "k", "v", "out")])


@pytest.mark.parametrize("fault,kw,mutate,code,message", _REJECTIONS, ids=[r[0].replace(" ", "_") for r in _REJECTIONS])
def test_host_checks_reject_one_fault_at_a_time(fault, kw, mutate, code, message):
    from vblade import _lib
    lib = _lib.load()
    a = _args(lib, **kw)
    if mutate is not None:
        mutate(a)
    rc = lib.vb_attn_fidelity(ctypes.byref(a), None)
    got = lib.vb_last_error().decode()
    print(f"[{fault}]: {rc} {got!r}")
    assert (rc, got) == (code, message)


def test_null_args_and_workspace_arithmetic():
    from vblade import _lib
    lib = _lib.load()
    assert lib.vb_attn_fidelity(None, None) == _lib.VB_ERR_INVALID
    assert lib.vb_attn_fidelity_workspace_size(None) == 0
    # 4 * (B*H*S*nc*(D+2) + 3*B*H*S) rounded up to 16, nc = ceil(L / 512)
    assert _args(lib).workspace_bytes == 4 * (6 * 30 * 2 * 66 + 3 * 6 * 30) == 97200
    assert _args(lib, B=1, H=1, L=1, S=1).workspace_bytes == 288          # 4 * (66 + 3) = 276 -> 288
    for B, H, L, D, S in ((1, 1, 512, 64, 1), (1, 1, 513, 64, 1), (2, 3, 5000, 128, 33), (1, 2, 131072, 128, 64),
                          (3, 1, 1024, 64, 64), (1, 1, 1025, 128, 7)):
        assert _args(lib, B=B, H=H, L=L, D=D, S=S).workspace_bytes == F.workspace_bytes(B, H, L, D, S), (B, H, L, D, S)
    # the chunk count is a rule of L alone
    assert _args(lib, B=1, H=1, L=513, S=1).workspace_bytes > _args(lib, B=1, H=1, L=512, S=1).workspace_bytes
    a = _args(lib)
    a.S = 0
    assert lib.vb_attn_fidelity_workspace_size(ctypes.byref(a)) == 0


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from vblade import ops
    q = torch.zeros(1, 1, 300, 64, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.attn_fidelity(q, q, q, q, [0, 5])
    with pytest.raises(ValueError, match="shape"):
        ops.attn_fidelity(q, q[:, :, :200], q, q, [0, 5])
    with pytest.raises(ValueError, match="shape"):
        ops.attn_fidelity(q, q, q, q[..., :32], [0, 5])
    e, s = torch.tensor([[0.0, 1e-4, 2.0]]), torch.tensor([[1.0, 1.0, 2.0]])
    snr = ops.fidelity_snr_db(e, s)
    assert snr.shape == e.shape and torch.isinf(snr[0, 0]) and snr[0, 0] > 0
    assert abs(float(snr[0, 1]) - 40.0) < 1e-4 and float(snr[0, 2]) == 0.0


SMALL = dict(width=16, height=12, depth=6, text_length=26)
VIDEO = 16 * 12 * 6


def test_adaptive_module_option_validation_and_probe_rows():
    import vblade
    m = vblade.AdaptiveBlockSparseAttn("cog", probe="fidelity", **SMALL)
    rows = m.gilbert_rearranger.rows
    gen = torch.Generator().manual_seed(0)
    pos = torch.randperm(VIDEO, generator=gen)[:30]
    pr = m.probe_rows
    assert pr.dtype == torch.int32 and pr.numel() == 30 and len(set(pr.tolist())) == 30
    assert torch.equal(pr, rows[pos])                                   # caller rows of the reordered positions
    assert int(pr.min()) >= SMALL["text_length"]                        # video rows: after the text for the caller
    assert "probe_rows" not in m.state_dict() and not hasattr(m, "probe_pos")
    assert m.last_fidelity_err is None and m.last_fidelity_sig is None and m.last_fidelity_peak is None
    assert m.fidelity is None
    for probe in (("recall", "fidelity"), ["fidelity", "recall"]):
        both = vblade.AdaptiveBlockSparseAttn("cog", probe=probe, probe_seed=3, probe_samples=64, **SMALL)
        assert both.probe_pos.numel() == 64
        assert torch.equal(both.probe_rows, rows[both.probe_pos.long()])  # the two probes look at the same queries
        assert not torch.equal(both.probe_rows[:30], pr)
    ident = vblade.AdaptiveBlockSparseAttn("cog", probe="fidelity", use_rearrange=False, **SMALL)
    assert torch.equal(ident.probe_rows.long(), pos)                    # no reorder: a position is its own row
    recall_only = vblade.AdaptiveBlockSparseAttn("cog", probe="recall", **SMALL)
    assert not hasattr(recall_only, "probe_rows") and recall_only.fidelity is None
    plain = vblade.AdaptiveBlockSparseAttn("cog", **SMALL)
    assert plain.probe is None and not hasattr(plain, "probe_rows") and plain.fidelity is None
    assert vblade.AdaptiveBlockSparseAttn("wan", probe="fidelity", probe_every=3).probe_every == 3
    for bad in (dict(probe="mass"), dict(probe=()), dict(probe=("fidelity", "fidelity")), dict(probe=("recall", "psnr")),
                dict(probe=7), dict(probe=("fidelity", 3)),
                dict(probe="fidelity", probe_samples=0), dict(probe="fidelity", probe_samples=65),
                dict(probe=("recall", "fidelity"), probe_samples=65),
                dict(probe="fidelity", probe_every=0), dict(probe="fidelity", probe_every=-2)):
        with pytest.raises(ValueError):
            vblade.AdaptiveBlockSparseAttn("cog", **SMALL, **bad)
    with pytest.raises(ValueError, match="video tokens"):
        vblade.AdaptiveBlockSparseAttn("cog", probe="fidelity", probe_samples=40, width=3, height=3, depth=3,
                                       text_length=26)


def test_multilevel_module_option_validation_and_probe_rows():
    from vblade import multilevel
    m = multilevel.AdaptiveBlockSparseAttnTrain(probe="fidelity", log_every=0, **SMALL)
    gen = torch.Generator().manual_seed(0)
    pos = torch.randperm(VIDEO, generator=gen)[:30]
    assert m.probe_rows.dtype == torch.int32 and torch.equal(m.probe_rows, m.gilbert_rearranger.rows[pos])
    assert "probe_rows" not in m.state_dict()
    assert m.last_fidelity_err is None and m.last_fidelity_sig is None and m.last_fidelity_peak is None
    assert m.fidelity is None
    other = multilevel.AdaptiveBlockSparseAttnTrain(probe="fidelity", probe_seed=1, probe_samples=64, probe_every=4,
                                                    **SMALL)
    assert other.probe_rows.numel() == 64 and other.probe_every == 4
    assert not torch.equal(other.probe_rows[:30], m.probe_rows)
    ident = multilevel.AdaptiveBlockSparseAttnTrain(probe="fidelity", use_rearrange=False, **SMALL)
    assert torch.equal(ident.probe_rows.long(), pos)
    plain = multilevel.AdaptiveBlockSparseAttnTrain(**SMALL)
    assert plain.probe is None and not hasattr(plain, "probe_rows") and plain.fidelity is None
    for bad in (dict(probe="recall"), dict(probe=("recall", "fidelity")), dict(probe="mass"), dict(probe=()),
                dict(probe="fidelity", probe_samples=0), dict(probe="fidelity", probe_samples=65),
                dict(probe="fidelity", probe_every=0)):
        with pytest.raises(ValueError):
            multilevel.AdaptiveBlockSparseAttnTrain(**SMALL, **bad)
    with pytest.raises(ValueError, match="video tokens"):
        multilevel.AdaptiveBlockSparseAttnTrain(probe="fidelity", probe_samples=40, width=3, height=3, depth=3,
                                                text_length=26)


def _case(L, D=64, B=2, H=3, S=33, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, D, generator=g) * torch.linspace(0.5, 2.5, H).view(1, H, 1, 1)
    k = torch.randn(B, H, L, D, generator=g)
    v = torch.randn(B, H, L, D, generator=g)
    rows = torch.randint(0, L, (S,), generator=g).numpy()
    return q.bfloat16(), k.bfloat16(), v.bfloat16(), rows


@pytest.mark.parametrize("L", [1, 129, 1000])
def test_restatement_invariants(L):
    q, k, v, rows = _case(L)
    B, H, _, D = q.shape
    ref, lse = F.dense_rows(q, k, v, rows)
    # out = ref gives err exactly 0 (a float64 out: the storage dtype could not hold ref)
    out = torch.zeros(B, H, L, D, dtype=torch.float64)
    out[:, :, torch.as_tensor(rows).clamp(0, L - 1)] = ref
    got = F.fidelity(q, k, v, out, rows)
    assert (got["row_err"] == 0).all() and (got["err"] == 0).all()
    assert (got["sig"] > 0).all() and np.array_equal(got["peak"], np.abs(got["ref"]).max(axis=(-2, -1)))
    # the natural-log LSE of the scaled scores, and torch's own attention (the scale as the header forms
    # it: fp32(scale) * fp32(log2 e), within 1e-8 of scale / ln 2)
    assert abs(F.qk_scale(D) * np.log(2.0) * np.sqrt(D) - 1) < 1e-7
    s = torch.matmul(q[:, :, rows].double(), k.double().transpose(-2, -1)) * (F.qk_scale(D) * np.log(2.0))
    assert np.abs(torch.logsumexp(s, dim=-1).numpy() - got["row_lse"]).max() < 1e-9
    assert np.abs((torch.softmax(s, dim=-1) @ v.double()).numpy() - got["ref"]).max() < 1e-9
    # a softmax over all keys does not depend on their order
    perm = torch.randperm(L, generator=torch.Generator().manual_seed(1))
    noise = torch.randn(B, H, L, D, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    outn = (out + 0.05 * noise).bfloat16()
    a = F.fidelity(q, k, v, outn, rows)
    b = F.fidelity(q, k[:, :, perm], v[:, :, perm], outn, rows)
    for f in ("ref", "row_lse", "row_err", "row_sig", "err", "sig", "peak"):
        assert np.abs(a[f] - b[f]).max() <= 1e-12, f
    assert (a["err"] > 0).all()
    # out-of-range rows clamp; float32 is the same computation at lower precision
    c, d = F.fidelity(q, k, v, outn, [-5, L + 7]), F.fidelity(q, k, v, outn, [0, L - 1])
    assert all(np.array_equal(c[f], d[f]) for f in c)
    e32 = F.fidelity(q, k, v, outn, rows, dtype=torch.float32)
    assert e32["ref"].dtype == np.float32 and np.abs(e32["ref"] - a["ref"]).max() < 1e-5
