"""GPU: vb_attn_fidelity and the modules' probe="fidelity" option.

The kernels evaluate in fp32, so against the float64 restatement (tests/fidelity_ref.py) `ref` and
`row_lse` must each stay within 8 x the error of the restatement's own fp32 eager evaluation on the same
inputs (per case and field, the worst edge case's value as the floor for every case). With delta the
bound of `ref`, row_err and row_sig follow by Cauchy-Schwarz:
|row_err - row_err64| <= 2 delta sqrt(D row_err64) + D delta^2 + D 2^-23 row_err64. The bounds are
measured against the restatement, never against the kernel. err, sig and peak are exact functions of
the rows' outputs and are compared in bits.

Measured on an MI355X (the figures every test prints before it asserts): the floors, 8 x the worst fp32
eager error over the 44 edge cases, are 3.16e-5 for ref (L=128, D=128, fp16, S=32: 3.96e-6) and 2.38e-5
for row_lse (L=300, D=64, fp16, S=32: 2.97e-6). The worst kernel error of ref is 2.47e-6, 0.078 of its
bound (L=513, D=64, bf16, S=33); of row_lse 1.34e-5, 0.125 of its bound (the scores of 433, where the fp32
eager evaluation has the same error); row_err stays within 0.009 and row_sig within 0.014 of their bounds.
Against 8 x each case's OWN fp32 eager error, without the floor, the worst ratio is 0.346 for ref (the
L=513 case) and 0.235 for row_lse (L=1, D=128, bf16)."""
import numpy as np
import pytest
import torch

import fidelity_ref as F
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAMES = ("err", "sig", "peak", "row_err", "row_sig", "row_lse", "ref")


def _ops():
    from vblade import ops
    return ops


def _run(q, k, v, out, rows, **kw):
    got = _ops().attn_fidelity(q.to(DEV), k.to(DEV), v.to(DEV), out.to(DEV), rows, want_rows=True, want_ref=True, **kw)
    return dict(zip(NAMES, (t.cpu().numpy() for t in got)))


def _qkv(B, H, L, D, dt, seed, temps=None, strided=False):
    """bf16/fp16 q, k, v [B,H,L,D]; ``strided``: non-contiguous views of [B,L,H,D] storage."""
    g = torch.Generator().manual_seed(seed)
    shape = (B, L, H, D) if strided else (B, H, L, D)
    q, k, v = (torch.randn(shape, generator=g) for _ in range(3))
    if strided:
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))
    if temps is not None:
        q = q * torch.as_tensor(temps, dtype=torch.float32).view(1, H, 1, 1)
    return tuple(t.to(F.DTYPES[dt]) for t in (q, k, v))


def _perturbed_out(q, k, v, rows, seed, strided=False, amp=0.02):
    """An `out` whose probe rows are the storage-rounded float64 dense rows plus noise of ``amp`` (so
    err is neither 0 nor huge) and whose other rows are random."""
    B, H, L, D = q.shape
    g = torch.Generator().manual_seed(seed)
    ref, _ = F.dense_rows(q, k, v, rows)
    out = torch.randn((B, L, H, D) if strided else (B, H, L, D), generator=g, dtype=torch.float64)
    if strided:
        out = out.transpose(1, 2)
    gi = torch.as_tensor(np.asarray(rows), dtype=torch.long).clamp(0, L - 1)
    out[:, :, gi] = ref + amp * torch.randn(ref.shape, generator=g, dtype=torch.float64)
    return out.to(q.dtype)


def _refs(q, k, v, out, rows, scale=None):
    """(ref64, {field: fp32 eager error}) of one case."""
    r64 = F.fidelity(q, k, v, out, rows, scale, dtype=torch.float64)
    r32 = F.fidelity(q, k, v, out, rows, scale, dtype=torch.float32)
    e32 = {f: float(np.abs(r32[f].astype(np.float64) - r64[f]).max()) for f in ("ref", "row_lse")}
    return r64, e32


# ------------------------------------------------------------------ the edge cases and their references
B, H = 2, 3
SAMPLES = (1, 32, 33, 64)          # one 32-row MFMA tile of probes, its edges, two tiles
# the issue's lengths, and those at which the chunk count (ceil(L / 512)) changes with one past each
LENGTHS = (1, 127, 128, 129, 300, 512, 513, 1000, 1024, 1025, 5000)
EDGES = [(L, D, dt) for L in LENGTHS for D in (64, 128) for dt in ("bf16", "fp16")]


def _edge_setup(case):
    L, D, dt = case
    li, di, ti = LENGTHS.index(L), (64, 128).index(D), ("bf16", "fp16").index(dt)
    S = SAMPLES[(2 * di + ti + li) % 4]
    strided = bool((li + di + ti) % 2)
    g = np.random.default_rng(1000 * li + 10 * di + ti)
    q, k, v = _qkv(B, H, L, D, dt, seed=L + D + ti, temps=np.linspace(0.5, 2.5, H), strided=strided)
    rows = g.integers(0, L, size=S).astype(np.int32)
    if S > 1:
        rows[0], rows[-1] = 0, L - 1
        rows[S // 2] = rows[S // 2 - 1]                      # one duplicate
    else:
        rows[0] = (L - 1) * ((li + di) % 2)
    out = _perturbed_out(q, k, v, rows, seed=7 + li, strided=strided)
    return q, k, v, out, rows, strided


_REFS = {}


def _edge_refs(case):
    """(inputs, ref64, fp32 eager errors) of an edge case, computed once and shared."""
    if case not in _REFS:
        q, k, v, out, rows, strided = _edge_setup(case)
        _REFS[case] = ((q, k, v, out, rows, strided),) + _refs(q, k, v, out, rows)
    return _REFS[case]


_FLOOR = {}


def _floor():
    """Per field, 8 x the worst fp32-eager error over every edge case: the bounds' floors."""
    if not _FLOOR:
        seen = {(len(_edge_refs(c)[0][4]), _edge_refs(c)[0][5]) for c in EDGES}
        assert seen == {(s, p) for s in SAMPLES for p in (False, True)}    # every S strided and contiguous
        for f in ("ref", "row_lse"):
            _FLOOR[f] = 8 * max(_edge_refs(c)[2][f] for c in EDGES)
        print(f"bound floors: {_FLOOR}")
    return _FLOOR


def _bounds(D, r64, e32):
    d_ref = max(8 * e32["ref"], _floor()["ref"])
    d_lse = max(8 * e32["row_lse"], _floor()["row_lse"])
    quad = {f: 2 * d_ref * np.sqrt(D * r64[f]) + D * d_ref ** 2 + D * 2.0 ** -23 * r64[f] for f in ("row_err", "row_sig")}
    return dict(ref=d_ref, row_lse=d_lse, **quad)


def _serial32(x):
    acc = np.zeros(x.shape[:-1], dtype=np.float32)
    for r in range(x.shape[-1]):
        acc = acc + x[..., r]
    return acc


def _check(tag, got, r64, e32):
    D = got["ref"].shape[-1]
    bounds = _bounds(D, r64, e32)
    worst, worst_own = 0.0, 0.0
    errs = {}
    for f in ("ref", "row_lse", "row_err", "row_sig"):
        assert np.isfinite(got[f]).all(), (tag, f)
        errs[f] = np.abs(got[f].astype(np.float64) - r64[f])
        ratio = float((errs[f] / bounds[f]).max())
        own = float(errs[f].max() / (8 * e32[f])) if f in e32 and e32[f] > 0 else 0.0
        print(f"{tag} {f}: kernel err {errs[f].max():.3e}, bound {np.max(bounds[f]):.3e}, err/bound {ratio:.3f}"
              + (f", fp32 eager err {e32[f]:.3e}, err / (8 x own eager) {own:.3f}" if f in e32 else ""))
        worst, worst_own = max(worst, ratio), max(worst_own, own)
    record("attn_fidelity kernel error / bound vs float64 (and / 8 x own eager)", (tag, round(worst, 3), round(worst_own, 3)))
    for f in ("ref", "row_lse", "row_err", "row_sig"):
        assert (errs[f] <= bounds[f]).all(), (tag, f, float(errs[f].max()))
    # the head's figures are exact functions of the rows': serial fp32 sums in r order, and a maximum
    assert np.array_equal(_serial32(got["row_err"]), got["err"]), tag
    assert np.array_equal(_serial32(got["row_sig"]), got["sig"]), tag
    assert np.array_equal(np.abs(got["ref"]).max(axis=(-2, -1)), got["peak"]), tag


@pytest.mark.parametrize("case", EDGES, ids=[f"L{L}_D{D}_{dt}" for L, D, dt in EDGES])
def test_edges_against_float64(case):
    (q, k, v, out, rows, strided), r64, e32 = _edge_refs(case)
    L = case[0]
    assert rows.min() == 0 or rows.max() == L - 1
    assert (r64["row_err"] > 0).all() and (r64["row_err"] < 1).all()     # neither 0 nor huge
    if strided and L > 1:                                              # one row: every layout is contiguous
        assert not q.is_contiguous() and not out.is_contiguous()
    got = _run(q, k, v, out, rows)
    _check(f"L{L}_D{case[1]}_{case[2]}_S{len(rows)}_{'strided' if strided else 'contig'}", got, r64, e32)


def test_large_scores_need_the_max_subtraction():
    """One head's base-2 scores are 433 +- 2: exp2 of them overflows fp32, the max-subtracted ones do not."""
    L, D = 1000, 64
    g = torch.Generator().manual_seed(31)
    q, k, v = _qkv(B, H, L, D, "fp16", seed=30, temps=np.linspace(0.5, 2.5, H))
    q[:, 0] = 6.0
    k[:, 0] = (6.25 + 0.2 * torch.randn(B, L, D, generator=g)).to(torch.float16)
    t = (q[0, 0, :1].double() @ k[0, 0].double().T) * F.qk_scale(D)
    print(f"large scores: base-2 scores of head 0 in [{t.min():.1f}, {t.max():.1f}]")
    assert 300 < t.min() and t.max() < 500
    rows = np.random.default_rng(6).integers(0, L, size=30).astype(np.int32)
    out = _perturbed_out(q, k, v, rows, seed=32)
    r64, e32 = _refs(q, k, v, out, rows)
    assert np.isfinite(r64["ref"]).all() and r64["row_lse"][:, 0].min() > 200
    _check("large", _run(q, k, v, out, rows), r64, e32)


def test_one_long_row():
    L = 131072
    q, k, v = _qkv(1, 1, L, 64, "bf16", seed=3, temps=[1.5])
    rows = np.array([777, 0, L - 1, 70000], dtype=np.int32)
    out = _perturbed_out(q, k, v, rows, seed=4)
    r64, e32 = _refs(q, k, v, out, rows)
    _check("long", _run(q, k, v, out, rows), r64, e32)


# ------------------------------------------------------------------ addressing and determinism
POISON = 3e4


def _inside(t, fill):
    """``t`` [B,H,L,D] as a view inside a larger allocation: every (b,h) slice is followed by 64 rows of
    ``fill`` and the whole tensor by 8192 more elements, so a kernel that reads past the L rows of a slice
    or past the tensor changes a value instead of leaving the buffer."""
    Bq, Hq, L, D = t.shape
    pad = 64
    buf = torch.full((Bq * Hq * (L + pad) * D + 8192,), fill, dtype=t.dtype, device=DEV)
    view = buf[:Bq * Hq * (L + pad) * D].view(Bq, Hq, L + pad, D)[:, :, :L]
    view.copy_(t.to(DEV))
    assert view.data_ptr() % 16 == 0 and not view.is_contiguous()
    return view


@pytest.mark.parametrize("L,D,dt", [(129, 64, "bf16"), (300, 128, "fp16"), (300, 64, "fp16"), (129, 128, "bf16")])
def test_nothing_is_read_past_the_rows_of_a_slice(L, D, dt):
    ops = _ops()
    q, k, v = _qkv(B, H, L, D, dt, seed=L + D)
    rows = np.array([0, L - 1, L // 2, 5, 5] + list(range(1, 29)), dtype=np.int32) % L
    out = _perturbed_out(q, k, v, rows, seed=9)
    rd = torch.from_numpy(rows).to(DEV)
    plain = ops.attn_fidelity(*(t.to(DEV) for t in (q, k, v, out)), rd, want_rows=True, want_ref=True)
    clean = ops.attn_fidelity(*(_inside(t, 0.0) for t in (q, k, v, out)), rd, want_rows=True, want_ref=True)
    dirty = ops.attn_fidelity(*(_inside(t, POISON) for t in (q, k, v, out)), rd, want_rows=True, want_ref=True)
    for name, a, b, c in zip(NAMES, plain, clean, dirty):
        assert torch.isfinite(c).all(), name
        assert torch.equal(a, b) and torch.equal(a, c), name


def test_two_runs_a_batch_slice_and_null_outputs_are_bit_equal():
    ops = _ops()
    L = 5000
    q, k, v = (t.to(DEV) for t in _qkv(B, H, L, 128, "bf16", seed=12, temps=[0.5, 1.0, 2.0]))
    out = torch.randn(B, H, L, 128, generator=torch.Generator().manual_seed(1)).to(DEV, torch.bfloat16)
    rows = torch.from_numpy(np.random.default_rng(1).integers(0, L, size=64).astype(np.int32)).to(DEV)
    a = ops.attn_fidelity(q, k, v, out, rows, want_rows=True, want_ref=True)
    b = ops.attn_fidelity(q, k, v, out, rows, want_rows=True, want_ref=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # sample 1 alone gives the bits it has inside the batch
    one = ops.attn_fidelity(q[1:], k[1:], v[1:], out[1:], rows, want_rows=True, want_ref=True)
    assert all(torch.equal(x[1:], y) for x, y in zip(a, one))
    # the nullable outputs change nothing
    c = ops.attn_fidelity(q, k, v, out, rows)
    assert len(c) == 3 and all(torch.equal(x, y) for x, y in zip(a, c))
    d = ops.attn_fidelity(q, k, v, out, rows, want_ref=True)
    assert len(d) == 4 and torch.equal(d[3], a[6])
    # out-of-range device rows are clamped by the kernel
    wild = torch.tensor([-5, L + 7], dtype=torch.int32, device=DEV)
    edge = torch.tensor([0, L - 1], dtype=torch.int32, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(ops.attn_fidelity(q, k, v, out, wild, want_rows=True, want_ref=True),
                                                 ops.attn_fidelity(q, k, v, out, edge, want_rows=True, want_ref=True)))
    # a given scale: the default is D^-1/2
    e = ops.attn_fidelity(q, k, v, out, rows, scale=128 ** -0.5, want_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:6], e))
    f = ops.attn_fidelity(q, k, v, out, rows, scale=0.05, want_rows=True)
    assert not torch.equal(f[5], a[5])


def test_the_call_captures_into_a_hip_graph_and_does_not_synchronise():
    ops = _ops()
    L = 1000
    q, k, v = (t.to(DEV) for t in _qkv(B, H, L, 64, "bf16", seed=15))
    out = torch.randn(B, H, L, 64, generator=torch.Generator().manual_seed(2)).to(DEV, torch.bfloat16)
    rows = torch.from_numpy(np.random.default_rng(3).integers(0, L, size=30).astype(np.int32)).to(DEV)
    eager = ops.attn_fidelity(q, k, v, out, rows, want_rows=True, want_ref=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = ops.attn_fidelity(q, k, v, out, rows, want_rows=True, want_ref=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(x, y) for x, y in zip(eager, again))
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            captured = ops.attn_fidelity(q, k, v, out, rows, want_rows=True, want_ref=True)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(eager, captured))


def test_a_sparser_mask_has_the_larger_error():
    """No threshold: the all-ones block mask is dense attention up to the forward kernel's own rounding,
    a random 30 % mask drops keys. Each Σerr equals the restatement on that same out within the bound."""
    ops = _ops()
    L, D, Hs = 1024, 64, 3                                              # nb = 8
    q, k, v = _qkv(1, Hs, L, D, "bf16", seed=50, temps=[0.5, 1.0, 2.0])
    rng = np.random.default_rng(51)
    rows = rng.choice(L, size=30, replace=False).astype(np.int32)
    full = torch.ones(1, Hs, 8, 8, dtype=torch.uint8)
    sparse = torch.from_numpy((rng.random((1, Hs, 8, 8)) < 0.3).astype(np.uint8))
    sparse |= torch.eye(8, dtype=torch.uint8)                           # no empty mask row
    assert sparse.float().mean() < 0.5
    tot = []
    for name, mask in (("all ones", full), ("random 30 %", sparse)):
        out = ops.attention_fwd(q.to(DEV), k.to(DEV), v.to(DEV), block_mask=mask.to(DEV)).cpu()
        got = _run(q, k, v, out, rows)
        r64, e32 = _refs(q, k, v, out, rows)
        _check(f"sanity {name}", got, r64, e32)
        snr = ops.fidelity_snr_db(torch.from_numpy(got["err"]), torch.from_numpy(got["sig"]))
        print(f"sanity {name}: sum err {got['err'].sum():.4e} (restatement {r64['err'].sum():.4e}), SNR dB {snr.tolist()}")
        tot.append(float(got["err"].sum()))
    assert tot[0] < tot[1]


# ------------------------------------------------------------------ the modules
GRID = dict(width=16, height=12, depth=6, text_length=26)                # L = 1178, 10 blocks
HEADS, HEAD_DIM = 4, 64


def _module(**kw):
    import vblade
    return vblade.AdaptiveBlockSparseAttn("cog", log_every=0, max_retain_ratio=0.5, **GRID, **kw)


def _ml_module(**kw):
    from vblade import multilevel
    return multilevel.AdaptiveBlockSparseAttnTrain(log_every=0, **GRID, **kw).to(DEV)


_INPUTS = []


def _inputs():
    if not _INPUTS:
        L = GRID["width"] * GRID["height"] * GRID["depth"] + GRID["text_length"]
        q, k, v = _qkv(1, HEADS, L, HEAD_DIM, "bf16", seed=41, temps=np.linspace(0.2, 3.0, HEADS))
        from vblade import attention
        go = torch.Generator(device=DEV).manual_seed(42)
        qo, ko = attention.draw_sample_offsets_qk(1, HEADS, DEV, generator=go)
        _INPUTS.extend((q.to(DEV), k.to(DEV), v.to(DEV), qo.contiguous(), ko.contiguous()))
    return _INPUTS


def _equals_the_op(m, q, k, v, out):
    want = _ops().attn_fidelity(q, k, v, out, m.probe_rows)
    for got, w in zip((m.last_fidelity_err, m.last_fidelity_sig, m.last_fidelity_peak), want):
        assert got.dtype == torch.float32 and got.shape == (1, HEADS) and got.is_cuda and not got.requires_grad
        assert torch.equal(got, w)
    return want


@pytest.mark.parametrize("make", [_module, _ml_module], ids=["adaptive", "multilevel"])
def test_module_probe_changes_nothing_and_equals_the_op(make):
    q, k, v, _, _ = _inputs()
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    res = []
    for kw in (dict(probe="fidelity"), dict()):
        m = make(**kw)
        torch.manual_seed(5)
        with torch.no_grad():
            out = m(q, k, v)                                   # the sampling offsets are drawn inside the call
        res.append((m, m.last_mask.clone(), out, gen.get_state().clone(), torch.rand(4, device=DEV)))
    (m, mask, out, state, draw), (plain, mask0, out0, state0, draw0) = res
    assert torch.equal(mask, mask0) and torch.equal(out, out0)
    assert torch.equal(state, state0) and torch.equal(draw, draw0)    # the generator's offset advanced identically
    assert plain.last_fidelity_err is None and plain.fidelity is None and not hasattr(plain, "probe_rows")
    err, sig, peak = _equals_the_op(m, q, k, v, out)
    snr = m.fidelity
    print(f"{make.__name__}: SNR dB per head {snr.tolist()}, peak {peak.tolist()}")
    assert snr.shape == (1, HEADS) and torch.isfinite(snr).all()       # random q, k: some heads lie below 0 dB
    assert torch.equal(snr, _ops().fidelity_snr_db(err.cpu(), sig.cpu()).float())   # one probed call so far
    # and the figures are the restatement's on the module's own output
    r64, e32 = _refs(q.cpu(), k.cpu(), v.cpu(), out.cpu(), m.probe_rows.cpu().numpy())
    _check(f"module {make.__name__}", _run(q, k, v, out, m.probe_rows), r64, e32)


def test_module_probe_every_third_call():
    q, k, v, qo, ko = _inputs()
    m = _module(probe="fidelity", probe_every=3)
    probed = []
    with torch.no_grad():
        for i in range(7):
            m.last_fidelity_err = None
            m(q, k, v, q_off=qo, k_off=ko)
            probed.append(m.last_fidelity_err is not None)
            if probed[-1]:
                first = (m.last_fidelity_err.clone(), m.last_fidelity_sig.clone())
    assert probed == [True, False, False, True, False, False, True]
    assert m._fidelity_count == 3
    # the same inputs three times: sums of three equal terms
    assert torch.equal(m.fidelity, _ops().fidelity_snr_db((first[0] * 3).cpu(), (first[1] * 3).cpu()).float())


def test_module_both_probes_give_the_recall_of_a_recall_only_module():
    q, k, v, qo, ko = _inputs()
    both, rec, fid = _module(probe=("recall", "fidelity")), _module(probe="recall"), _module(probe="fidelity")
    with torch.no_grad():
        outs = [m(q, k, v, q_off=qo, k_off=ko) for m in (both, rec, fid)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert torch.equal(both.last_recall, rec.last_recall) and torch.equal(both.last_oracle_recall, rec.last_oracle_recall)
    assert torch.equal(both.last_fidelity_err, fid.last_fidelity_err) and torch.equal(both.last_fidelity_sig, fid.last_fidelity_sig)
    assert torch.equal(both.probe_rows, both._rows(q.device)[both.probe_pos.long()])
    assert rec.last_fidelity_err is None and fid.last_recall is None


@pytest.mark.parametrize("make", [_module, _ml_module], ids=["adaptive", "multilevel"])
def test_module_under_autograd_probes_and_still_backpropagates(make):
    q, k, v, _, _ = _inputs()
    m = make(probe="fidelity")
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    torch.manual_seed(5)
    out = m(qq, kk, vv)
    _equals_the_op(m, q, k, v, out.detach())
    assert torch.isfinite(m.fidelity).all()
    out.float().square().sum().backward()
    for t in (qq, kk, vv):
        assert t.grad is not None and torch.isfinite(t.grad.float()).all()


def test_module_call_captures_into_a_hip_graph():
    ops = _ops()
    q, k, v, _, _ = _inputs()
    m = _module(probe="fidelity")
    Bq, Hq = q.shape[:2]
    with torch.no_grad():
        m(q, k, v)                                   # warm up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with torch.cuda.graph(graph, stream=s):
                out = m(q, k, v)
        torch.cuda.current_stream().wait_stream(s)
        captured = (m.last_mask, m.last_fidelity_err, m.last_fidelity_sig, m.last_fidelity_peak)
        gen = torch.cuda.default_generators[torch.cuda.current_device()]
        state = gen.get_state()
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in captured] + [out.clone()]
        # the same generator state, eagerly, gives the draws (and so the offsets) the replay used
        gen.set_state(state)
        rq = torch.rand(Bq, Hq, 1, 128, device=DEV)
        rk = torch.rand(Bq, Hq, 1, 128, device=DEV)
        qo, ko = ops.sample_offsets(rq, rk, 32)
        eager = m(q, k, v, q_off=qo[:, :, 0], k_off=ko[:, :, 0])
        torch.cuda.synchronize()
    assert torch.equal(m.last_mask, replayed[0]) and torch.equal(eager, replayed[4])
    assert torch.equal(m.last_fidelity_err, replayed[1]) and torch.equal(m.last_fidelity_sig, replayed[2])
    assert torch.equal(m.last_fidelity_peak, replayed[3])
