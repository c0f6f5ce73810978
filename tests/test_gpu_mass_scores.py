"""GPU: vb_mask_scores_mass (ops.mask_scores_mass) and the module's score="mass" option.

The kernel evaluates in fp32, so against the float64 restatement (tests/mass_ref.py) its fp32 block
masses must stay within 8 x the error of the restatement's own fp32 eager evaluation of the same case,
with 8 x the worst edge case's error as the floor for every case (the rule of tests/test_gpu_recall.py):
the order of the fp32 sums differs, nothing else. po is checked to one unit in the last place of the
storage dtype against the rounded float64 value: an fp32 error of 1e-6 can only flip a rounding boundary.
Every test prints its figures before it asserts.

Measured on an MI355X: the floor, 8 x the worst fp32 eager error over the edge cases, is 1.17e-4 (the
cases with scores of magnitude 450-520: a block mass near 32 carries an fp32 eager error of 1.5e-5); the
worst kernel error is 1.6e-5 (L=640, D=128, bf16, scores ~520), 0.14 of its bound. Against 8 x each
case's OWN fp32 eager error, without the floor, the worst ratio is 0.15 (the same case), then 0.12; po is
0 ulp from the rounded float64 value in every case; row sums lie within 4.8e-6 of 32."""
import ctypes

import numpy as np
import pytest
import torch

import bsa_oracle as O
import mass_ref as M
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ops():
    from vblade import ops
    return ops


# ------------------------------------------------------------------ the edge cases and their references
# (L, D, dtype, rows permuted, [B,L,H,D] transposed views, q multiplier). Each L is the smallest that
# reaches one edge: one ragged block; one full block; three blocks, the last ragged (an odd count: the
# wave that owns q-blocks 2 and 3 has only one); nb = 5, no multiple of the 4 waves x 2 q-blocks of a
# workgroup; a one-token tail block whose sampled rows are all clamps; nb = 9, the first count at which a
# second workgroup per head exists. The conditions are covered pairwise, not as a product. A multiplier
# of 70 gives scores (in the exponent's base-2 units) of magnitude in the hundreds (450-520 here).
EDGES = [
    (100, 64, "bf16", False, True, 1.0),
    (128, 128, "fp16", True, False, 1.0),
    (300, 128, "bf16", True, True, 1.0),
    (300, 64, "fp16", False, False, 70.0),
    (640, 64, "fp16", False, True, 1.0),
    (640, 128, "bf16", True, False, 70.0),
    (513, 64, "bf16", True, False, 1.0),
    (513, 128, "fp16", False, True, 1.0),
    (1100, 64, "bf16", True, True, 1.0),
]
B, H = 2, 3
LONG_L = 41100                       # nb = 322, past the short predictor's 320
LONG_BLOCKS = (0, 1, 160, 320, 321)  # the q-blocks of the long case that are compared


def _inputs(L, D, dt, perm, seed, mult=1.0, b=B, h=H):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(b, L, h, D, generator=g) * mult).to(M.DTYPES[dt]).transpose(1, 2)   # [B,H,L,D] views
    k = torch.randn(b, L, h, D, generator=g).to(M.DTYPES[dt]).transpose(1, 2)
    rows = torch.randperm(L, generator=g).to(torch.int32) if perm else None
    q_off = O.draw_sample_offsets(b, h, generator=g).to(torch.int32)
    k_off = O.draw_sample_offsets(b, h, generator=g).to(torch.int32)
    assert not torch.equal(q_off, k_off)
    return q, k, rows, q_off, k_off


def _run(q, k, rows, q_off, k_off, transposed, **kw):
    ops = _ops()
    qd, kd = q.to(DEV), k.to(DEV)          # .to keeps the strides of the transposed view
    if not transposed:
        qd, kd = qd.contiguous(), kd.contiguous()
    else:
        assert not qd.is_contiguous()
    r = None if rows is None else rows.to(DEV)
    po, mass = ops.mask_scores_mass(qd, kd, q_off.to(DEV), k_off.to(DEV), rows=r, want_mass=True, **kw)
    return po.cpu(), mass.cpu()


_REFS = {}


def _edge_refs(case):
    """(inputs, mass64, po of mass64 in the storage dtype, fp32 eager error), computed once and shared."""
    if case not in _REFS:
        L, D, dt, perm, _, mult = case
        inp = _inputs(L, D, dt, perm, seed=L + D + int(mult), mult=mult)
        q, k, rows, q_off, k_off = inp
        qs, ks = M.sampled_streams(q, k, q_off, k_off, rows)
        m64 = M.block_mass(qs, ks, dtype=torch.float64)
        m32 = M.block_mass(qs, ks, dtype=torch.float32)
        _REFS[case] = (inp, m64, M.po_of(m64, q.dtype), float((m32.double() - m64).abs().max()))
    return _REFS[case]


_FLOOR = []


def _floor():
    """8 x the worst fp32-eager error over the edge cases: the bound's floor."""
    if not _FLOOR:
        _FLOOR.append(8 * max(_edge_refs(c)[3] for c in EDGES))
        print(f"bound floor: {_FLOOR[0]:.3e}")
    return _FLOOR[0]


def _ulps(got, ref):
    """Distance in units of the last place between two non-negative tensors of one 16-bit dtype."""
    assert got.dtype == ref.dtype and (got.float() >= 0).all() and (ref.float() >= 0).all()
    return (got.view(torch.int16).int() - ref.view(torch.int16).int()).abs()


def _check(tag, po, mass, m64, po64, err32):
    bound = max(8 * err32, _floor())
    assert torch.isfinite(mass).all() and torch.isfinite(po.float()).all(), tag
    err = float((mass.double() - m64).abs().max())
    ulps = int(_ulps(po, po64).max())
    rowsum = float((mass.double().sum(-1) - M.KEEP).abs().max())
    print(f"{tag}: mass err {err:.3e}, fp32 eager err {err32:.3e}, bound {bound:.3e}, ratio to 8 x own eager "
          f"{err / max(8 * err32, 1e-300):.3f}; po worst {ulps} ulp; |row sum - 32| {rowsum:.3e}")
    record("mask_scores_mass kernel error / bound vs float64", (tag, round(err / bound, 3)))
    assert err <= bound, tag
    assert ulps <= 1, tag
    assert rowsum <= 32 * 1e-5, tag   # every sampled query spreads a mass of one


def _tag(case):
    L, D, dt, perm, tr, mult = case
    return f"L{L}_D{D}_{dt}_{'perm' if perm else 'id'}_{'bhld-view' if tr else 'contig'}_x{int(mult)}"


@pytest.mark.parametrize("case", EDGES, ids=[_tag(c) for c in EDGES])
def test_edges_against_float64(case):
    (q, k, rows, q_off, k_off), m64, po64, err32 = _edge_refs(case)
    po, mass = _run(q, k, rows, q_off, k_off, transposed=case[4])
    if case[5] > 1:
        s = torch.matmul(q[0, 0].double(), k[0, 0].double().T) * M.qk_scale(case[1])
        print(f"largest |score| (base-2 units): {float(s.abs().max()):.0f}")
        assert s.abs().max() > 200
    _check(_tag(case), po, mass, m64, po64, err32)


def test_past_the_short_predictors_row_limit():
    """nb = 322: the rows of five q-blocks (first, last, the pair around 160) against the restatement."""
    L, D, dt = LONG_L, 64, "bf16"
    q, k, rows, q_off, k_off = _inputs(L, D, dt, True, seed=5, b=1, h=1)
    po, mass = _run(q, k, rows, q_off, k_off, transposed=False)
    qs, ks = M.sampled_streams(q, k, q_off, k_off, rows)
    sel = torch.cat([torch.arange(32 * i, 32 * i + 32) for i in LONG_BLOCKS])
    m64 = M.block_mass(qs[:, :, sel], ks, dtype=torch.float64)
    m32 = M.block_mass(qs[:, :, sel], ks, dtype=torch.float32)
    err32 = float((m32.double() - m64).abs().max())
    idx = torch.tensor(LONG_BLOCKS)
    _check("long", po[:, :, idx], mass[:, :, idx], m64, M.po_of(m64, q.dtype), err32)
    assert mass.shape[-1] == 322
    # the rows that were not compared are whole too
    assert float((mass.double().sum(-1) - M.KEEP).abs().max()) <= 32 * 1e-5


def test_scale_argument():
    case = EDGES[2]
    (q, k, rows, q_off, k_off), _, _, _ = _edge_refs(case)
    qs, ks = M.sampled_streams(q, k, q_off, k_off, rows)
    m64 = M.block_mass(qs, ks, scale=0.31, dtype=torch.float64)
    err32 = float((M.block_mass(qs, ks, scale=0.31, dtype=torch.float32).double() - m64).abs().max())
    po, mass = _run(q, k, rows, q_off, k_off, transposed=True, scale=0.31)
    _check("scale0.31", po, mass, m64, M.po_of(m64, q.dtype), err32)


def test_two_calls_give_equal_bits_and_po_alone_equals_po_with_mass():
    ops = _ops()
    for case in (EDGES[4], EDGES[5]):
        (q, k, rows, q_off, k_off), _, _, _ = _edge_refs(case)
        a = _run(q, k, rows, q_off, k_off, transposed=case[4])
        b = _run(q, k, rows, q_off, k_off, transposed=case[4])
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        r = None if rows is None else rows.to(DEV)
        po = ops.mask_scores_mass(q.to(DEV).contiguous(), k.to(DEV).contiguous(), q_off.to(DEV), k_off.to(DEV), rows=r)
        assert torch.equal(po.cpu().view(torch.int16), a[0].view(torch.int16))


# ------------------------------------------------------------------ a case on which the two scores disagree
def _disagreement(D, dt):
    """Every query is u (entries +-1); a key is u * v / sqrt(D), so its natural-log score is v. Key block 0
    holds ONE sampled key with v = 2 and opposed keys (v = -2) elsewhere; key block 1 holds mildly aligned
    keys (v = 1) throughout; key block 2 is opposed. The largest single probability is in block 0
    (e^2 > e^1), the mass in block 1 (32 e^1 > e^2 + 31 e^-2)."""
    g = torch.Generator().manual_seed(D)
    b, h, nb = 1, 2, 3
    L = nb * 128
    u = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).float()
    q_off = O.draw_sample_offsets(b, h, generator=g).to(torch.int32)
    k_off = O.draw_sample_offsets(b, h, generator=g).to(torch.int32)
    v = torch.full((b, h, L), -2.0)
    v[:, :, 128:256] = 1.0
    for hh in range(h):
        v[0, hh, int(k_off[0, hh, 5])] = 2.0
    q = u.expand(b, h, L, D).to(M.DTYPES[dt]).contiguous()
    k = (u * (v / D ** 0.5).unsqueeze(-1)).to(M.DTYPES[dt])
    return q, k, q_off, k_off


@pytest.mark.parametrize("D,dt", [(64, "bf16"), (128, "fp16")])
def test_mass_and_max_proxy_rank_a_constructed_pair_differently(D, dt):
    ops = _ops()
    q, k, q_off, k_off = _disagreement(D, dt)
    qs, ks = M.sampled_streams(q, k, q_off, k_off)
    po_max_ref = O.pooled_scores(qs, ks, D ** -0.5, block=M.KEEP, store_dtype=q.dtype)
    po_mass_ref = M.po_of(M.block_mass(qs, ks), q.dtype).float()
    print("oracle max proxy row 0:", po_max_ref[0, 0, 0].tolist(), "restated mass row 0:", po_mass_ref[0, 0, 0].tolist())
    assert (po_max_ref[..., 0] > po_max_ref[..., 1]).all() and (po_mass_ref[..., 1] > po_mass_ref[..., 0]).all()
    po_mass = ops.mask_scores_mass(q.to(DEV), k.to(DEV), q_off.to(DEV), k_off.to(DEV)).float().cpu()
    po_max, _ = ops.mask_predict(q.to(DEV), k.to(DEV), q_off.to(DEV), k_off.to(DEV), want_mask=False)
    po_max = po_max.float().cpu()
    print("kernel max proxy row 0:", po_max[0, 0, 0].tolist(), "kernel mass row 0:", po_mass[0, 0, 0].tolist())
    assert (po_mass[..., 1] > po_mass[..., 0]).all() and (po_mass[..., 0] > po_mass[..., 2]).all()
    assert (po_max[..., 0] > po_max[..., 1]).all()


# ------------------------------------------------------------------ refusals
def test_refusals_return_before_any_launch():
    from vblade import _lib
    ops = _ops()
    lib = _lib.load()
    L, D = 300, 64
    q = torch.randn(1, 2, L, D, device=DEV).bfloat16()
    off = torch.zeros(1, 2, 32, device=DEV, dtype=torch.int32)
    po = torch.full((1, 2, 3, 3), 7.0, device=DEV, dtype=torch.bfloat16)
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)

    def call(**kw):
        a = _lib.MassScoresArgs()
        a.q = a.k = q.data_ptr()
        a.q_stride = a.k_stride = (ctypes.c_int64 * 3)(*q.stride()[:3])
        a.q_off = a.k_off = off.data_ptr()
        a.B, a.H, a.L, a.D, a.block, a.num_keep = 1, 2, L, D, 128, 32
        a.dtype = _lib.VB_DTYPE_BF16
        a.po, a.workspace, a.workspace_bytes = po.data_ptr(), ws.data_ptr(), ws.numel()
        for n, v in kw.items():
            setattr(a, n, v)
        _lib.check(lib.vb_mask_scores_mass(ctypes.byref(a), torch.cuda.current_stream().cuda_stream),
                   "vb_mask_scores_mass")

    for kw, code, word in ((dict(num_keep=16), _lib.VB_ERR_UNSUPPORTED, "num_keep 32"),
                           (dict(num_keep=64), _lib.VB_ERR_UNSUPPORTED, "num_keep 32"),
                           (dict(D=96), _lib.VB_ERR_UNSUPPORTED, "head_dim must be 64 or 128"),
                           (dict(L=128 * 1024 + 1), _lib.VB_ERR_UNSUPPORTED, "sequence too long"),
                           (dict(po=None), _lib.VB_ERR_INVALID, "null argument")):
        with pytest.raises(_lib.VBladeError, match=word) as e:
            call(**kw)
        assert e.value.code == code, kw
    torch.cuda.synchronize()
    assert (po == 7.0).all()        # nothing was launched
    call()                          # the same arguments without a fault run
    torch.cuda.synchronize()
    assert not (po == 7.0).any()
    for width in (16, 64):
        o = torch.zeros(1, 2, width, device=DEV, dtype=torch.int32)
        with pytest.raises(ValueError, match="32 tokens per block"):
            ops.mask_scores_mass(q, q, o, o)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mask_scores_mass(q.cpu(), q.cpu(), off.cpu(), off.cpu())


# ------------------------------------------------------------------ the module option
GRID = dict(width=16, height=8, depth=5, text_length=0)   # L = 640, nb = 5


def _module(**kw):
    import vblade
    opts = dict(GRID, min_retain_ratio=0.2, max_retain_ratio=0.6, log_every=0)
    opts.update(kw)
    return vblade.AdaptiveBlockSparseAttn("wan", **opts).to(DEV)


def _qkv(D=64, dt=torch.bfloat16, heads=3, batch=2):
    g = torch.Generator().manual_seed(11)
    return tuple(torch.randn(batch, heads, 640, D, generator=g).to(dt).to(DEV) for _ in range(3))


def _gen_state():
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    return gen.initial_seed(), gen.get_offset()


def test_module_mass_mask_equals_the_hand_made_chain():
    from vblade.attention import retain_counts
    ops = _ops()
    q, k, v = _qkv()
    m = _module(score="mass")
    torch.cuda.manual_seed(77)
    with torch.no_grad():
        out = m(q, k, v)
    state_mass = _gen_state()
    torch.cuda.manual_seed(77)
    rq = torch.rand(2, 3, 1, 128, device=DEV)
    rk = torch.rand(2, 3, 1, 128, device=DEV)
    q_off, k_off = ops.sample_offsets(rq, rk, 32)
    po = ops.mask_scores_mass(q, k, q_off[:, :, 0], k_off[:, :, 0], rows=m._rows(q.device))
    lo, hi = retain_counts(5, 0.2, 0.6, "wan")
    mask = ops.block_mask_rule(po, None, energy_threshold=0.95, min_keep=lo, max_keep=hi, force_tail=0)
    assert torch.equal(m.last_mask, mask)
    assert 0 < int(mask.sum()) < mask.numel()
    assert torch.isfinite(out.float()).all()
    # both modes sample the same tokens under one seed and leave the generator in the same state
    mx = _module(score="max")
    torch.cuda.manual_seed(77)
    with torch.no_grad():
        mx(q, k, v)
    assert _gen_state() == state_mass


def test_module_max_is_the_module_without_the_option():
    q, k, v = _qkv(D=128, dt=torch.float16)
    res = []
    for kw in (dict(), dict(score="max")):
        m = _module(**kw)
        torch.cuda.manual_seed(5)
        with torch.no_grad():
            out = m(q, k, v)
        res.append((out, m.last_mask, _gen_state()))
    assert torch.equal(res[0][0].view(torch.int16), res[1][0].view(torch.int16))
    assert torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


@pytest.mark.parametrize("extra", [dict(mask_mode="topk", init_k=2), dict(head_budget="judge"), dict(probe="recall")],
                         ids=["topk", "judge", "recall"])
def test_module_mass_beside_the_other_mask_options(extra):
    q, k, v = _qkv()
    m = _module(score="mass", **extra)
    torch.cuda.manual_seed(3)
    with torch.no_grad():
        out = m(q, k, v)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and m.last_mask.shape == (2, 3, 5, 5)
    assert (m.last_mask.sum(-1) >= 1).all()
    if "probe" in extra:
        rec = m.last_recall.cpu()
        assert rec.shape == (2, 3) and ((rec > 0) & (rec <= 1)).all()
    if "head_budget" in extra:
        assert m.last_head_budget.shape == (2, 3)


# ------------------------------------------------------------------ end to end
def test_mass_mask_recall_beats_the_max_proxy_mask_on_the_small_grid():
    """Equal-budget masks (the 5 best of 50 blocks per row) from the two kernels' po on the 6400-token grid
    of tests/test_mass_scores.py: ops.mask_recall of the mass mask is above that of the max mask, after the
    CPU restatement of the same inputs has shown the same sign."""
    import recall_ref as R
    ops = _ops()
    D, budget = 64, 5
    q, k, rows, q_off, k_off, pos = M.small_grid_case(H=4, D=D)
    L = q.shape[2]
    qs, ks = M.sampled_streams(q, k, q_off, k_off, rows)
    E = R.block_masses(q, k, pos, rows)
    cpu = {"max": O.pooled_scores(qs, ks, D ** -0.5, block=M.KEEP, store_dtype=torch.bfloat16),
           "mass": M.po_of(M.block_mass(qs, ks), torch.bfloat16)}
    cpu = {n: float(R.from_masses(E, M.topk_mask(po, budget), pos, L)["recall"].mean()) for n, po in cpu.items()}
    print(f"restatement: max proxy {cpu['max']:.4f}, sampled mass {cpu['mass']:.4f}")
    assert cpu["mass"] > cpu["max"]
    qd, kd = q.to(DEV), k.to(DEV)
    rd = torch.as_tensor(rows, dtype=torch.int32).to(DEV)
    qo, ko = q_off.to(torch.int32).to(DEV), k_off.to(torch.int32).to(DEV)
    po = {"max": ops.mask_predict(qd, kd, qo, ko, rows=rd, want_mask=False)[0],
          "mass": ops.mask_scores_mass(qd, kd, qo, ko, rows=rd)}
    got = {}
    for n, p in po.items():
        mask = torch.zeros(p.shape, device=DEV, dtype=torch.uint8)
        mask.scatter_(-1, torch.topk(p.float(), budget, dim=-1).indices, 1)
        assert (mask.sum(-1) == budget).all()
        got[n] = float(ops.mask_recall(qd, kd, mask, pos.astype(np.int32), rows=rd)[0].mean())
    print(f"kernels: max proxy {got['max']:.4f}, sampled mass {got['mass']:.4f}")
    record("recall at 5 of 50 blocks, max proxy vs sampled mass", (round(got["max"], 4), round(got["mass"], 4)))
    assert got["mass"] > got["max"]
