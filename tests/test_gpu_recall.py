"""GPU: vb_mask_recall and the module's probe="recall" option.

The kernels evaluate in fp32, so against the float64 restatement (tests/recall_ref.py) they must stay
within 8 x the error of the restatement's own fp32 eager evaluation on the same inputs (per case, the
worst edge case's value as the floor for every case): MFMA accumulation order and v_exp_f32 (<= 1 ulp)
differ from the CPU's fp32 by a few ulps of values <= 1. The bound is measured against the
restatement, never against the kernel.

Measured on an MI355X (the figures every test prints before it asserts): the floor, 8 x the worst fp32
eager error over the edge cases, is 6.36e-6 (L=300, D=128, fp16, S=32: 7.9e-7); the worst kernel
error is 4.2e-7 (row_oracle of the scores-of-300 case), 0.065 of its bound. Against 8 x each case's
OWN fp32 eager error, without the floor, the worst ratio is 0.77 (the same case), then 0.52 (the
L=131072 row) and 0.33 or less on the edge cases."""
import numpy as np
import pytest
import torch

import recall_ref as R
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("recall", "oracle", "row_recall", "row_oracle")


def _ops():
    from vblade import ops
    return ops


def _qk(B, H, L, D, dt, seed, temps=None):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, L, D, generator=g)
    k = torch.randn(B, H, L, D, generator=g)
    if temps is not None:
        q = q * torch.as_tensor(temps, dtype=torch.float32).view(1, H, 1, 1)
    return q.to(R.DTYPES[dt]), k.to(R.DTYPES[dt])


def _run(q, k, mask, pos, rows=None, **kw):
    ops = _ops()
    r = None if rows is None else torch.as_tensor(np.asarray(rows), dtype=torch.int32).to(DEV)
    got = ops.mask_recall(q.to(DEV), k.to(DEV), mask.to(DEV), pos, rows=r, want_rows=True, **kw)
    names = FIELDS + ("row_kept",)
    return dict(zip(names, (t.cpu().numpy() for t in got)))


def _fp32_mean(rm):
    acc = np.zeros(rm.shape[:-1], dtype=np.float32)
    for r in range(rm.shape[-1]):
        acc = acc + rm[..., r]
    return acc / np.float32(rm.shape[-1])


def _err32(ref32, ref64):
    return max(float(np.abs(ref32[f].astype(np.float64) - ref64[f]).max()) for f in FIELDS)


# ------------------------------------------------------------------ the edge cases and their references
B, H = 2, 3
SAMPLES = (1, 32, 33, 64)          # one 32-row MFMA tile of probes, its edges, two tiles
EDGES = [(L, D, dt) for L in (128, 129, 300, 1000, 5000) for D in (64, 128) for dt in ("bf16", "fp16")]
MASKS = ("random", "one_per_row", "empty_row")


def _edge_setup(case):
    """Inputs of one edge case (seeded from the case alone): S and the permutation cycle over the cases."""
    L, D, dt = case
    li, di, ti = (128, 129, 300, 1000, 5000).index(L), (64, 128).index(D), ("bf16", "fp16").index(dt)
    S = SAMPLES[(2 * di + ti + li) % 4]
    g = np.random.default_rng(1000 * li + 10 * di + ti)
    q, k = _qk(B, H, L, D, dt, seed=L + D + ti, temps=np.linspace(0.5, 2.5, H))
    pos = g.integers(0, L, size=S).astype(np.int32)
    if S > 1:
        pos[0], pos[-1] = 0, L - 1
    else:
        pos[0] = (L - 1) * ((li + di) % 2)
    rows = g.permutation(L).astype(np.int32) if (li + di) % 2 else None
    nb = (L + 127) // 128
    masks = {"random": torch.from_numpy((g.random((B, H, nb, nb)) < 0.4).astype(np.uint8))}
    one = torch.zeros(B, H, nb, nb, dtype=torch.uint8)
    one.scatter_(3, torch.from_numpy(g.integers(0, nb, size=(B, H, nb, 1))), 1)
    masks["one_per_row"] = one
    empty = masks["random"].clone()
    empty[1, 2, pos[0] // 128] = 0
    masks["empty_row"] = empty
    return q, k, pos, rows, masks


_REFS = {}


def _edge_refs(case):
    """(inputs, {mask kind: (ref64, fp32 eager error)}) of an edge case, computed once and shared."""
    if case not in _REFS:
        q, k, pos, rows, masks = _edge_setup(case)
        E64 = R.block_masses(q, k, pos, rows, dtype=torch.float64)
        E32 = R.block_masses(q, k, pos, rows, dtype=torch.float32)
        refs = {}
        for kind, m in masks.items():
            r64 = R.from_masses(E64, m, pos, case[0])
            refs[kind] = (r64, _err32(R.from_masses(E32, m, pos, case[0]), r64))
        _REFS[case] = ((q, k, pos, rows, masks), refs)
    return _REFS[case]


_FLOOR = []


def _floor():
    """8 x the worst fp32-eager error over every edge case and mask kind: the bound's floor."""
    if not _FLOOR:
        # the cases cover every probe count with and without a row permutation
        seen = {(len(_edge_refs(c)[0][2]), _edge_refs(c)[0][3] is not None) for c in EDGES}
        assert seen == {(s, p) for s in SAMPLES for p in (False, True)}
        _FLOOR.append(8 * max(e for case in EDGES for _, e in _edge_refs(case)[1].values()))
        print(f"bound floor: {_FLOOR[0]:.3e}")
    return _FLOOR[0]


def _check(tag, got, ref64, err32):
    bound = max(8 * err32, _floor())
    worst = 0.0
    for f in FIELDS:
        assert np.isfinite(got[f]).all(), (tag, f)
        err = float(np.abs(got[f].astype(np.float64) - ref64[f]).max())
        print(f"{tag} {f}: kernel err {err:.3e}, fp32 eager err {err32:.3e}, bound {bound:.3e}")
        worst = max(worst, err / bound)
    record("mask_recall kernel error / bound vs float64", (tag, round(worst, 3)))
    for f in FIELDS:
        assert np.abs(got[f].astype(np.float64) - ref64[f]).max() <= bound, (tag, f)
    assert np.array_equal(got["row_kept"], ref64["row_kept"]), tag
    # the head's figures are the fp32 means of the rows', summed in row order
    assert np.array_equal(_fp32_mean(got["row_recall"]), got["recall"]), tag
    assert np.array_equal(_fp32_mean(got["row_oracle"]), got["oracle"]), tag


@pytest.mark.parametrize("case", EDGES, ids=[f"L{L}_D{D}_{dt}" for L, D, dt in EDGES])
def test_edges_against_float64(case):
    (q, k, pos, rows, masks), refs = _edge_refs(case)
    assert pos.min() == 0 or pos.max() == case[0] - 1
    for kind in MASKS:
        got = _run(q, k, masks[kind], pos, rows)
        tag = f"L{case[0]}_D{case[1]}_{case[2]}_S{len(pos)}_{'perm' if rows is not None else 'id'}_{kind}"
        _check(tag, got, *refs[kind])
        if kind == "one_per_row":
            assert (got["row_kept"] == 1).all()
        if kind == "empty_row":
            assert got["row_kept"][1, 2, 0] == 0 and got["row_recall"][1, 2, 0] == 0 and got["row_oracle"][1, 2, 0] == 0


def test_one_long_row():
    L = 131072
    q, k = _qk(1, 1, L, 64, "bf16", seed=3, temps=[1.5])
    g = np.random.default_rng(9)
    pos = np.array([777, L - 1], dtype=np.int32)
    rows = g.permutation(L).astype(np.int32)
    mask = torch.from_numpy((g.random((1, 1, 1024, 1024)) < 0.1).astype(np.uint8))
    ref64 = R.recall(q, k, mask, pos, rows, dtype=torch.float64)
    err32 = _err32(R.recall(q, k, mask, pos, rows, dtype=torch.float32), ref64)
    _check("long", _run(q, k, mask, pos, rows), ref64, err32)


# ------------------------------------------------------------------ exact cases
def test_all_ones_mask_is_exactly_one():
    for L, D, dt in ((129, 64, "fp16"), (1000, 128, "bf16"), (5000, 64, "bf16")):
        q, k = _qk(B, H, L, D, dt, seed=L, temps=np.linspace(0.5, 2.5, H))
        nb = (L + 127) // 128
        pos = np.random.default_rng(L).integers(0, L, size=33).astype(np.int32)
        got = _run(q, k, torch.ones(B, H, nb, nb, dtype=torch.uint8), pos)
        for f in FIELDS:
            assert (got[f] == np.float32(1.0)).all(), (L, f)
        assert (got["row_kept"] == nb).all()


def _ranked_blocks(nb, D, dt, seed):
    """q = u + noise, the keys of block c = u * v_c / sqrt(D) + noise with u of +-1 entries: every score
    of block c is v_c +- 0.1, v_c = 1.5 * (a permutation of the ranks), so neighbouring block masses
    differ by a factor of e^1.3 or more, far above any rounding."""
    g = torch.Generator().manual_seed(seed)
    L = nb * 128
    u = (torch.randint(0, 2, (D,), generator=g) * 2 - 1).float()
    v = 1.5 * torch.stack([torch.randperm(nb, generator=g) for _ in range(B * H)]).view(B, H, nb).float()
    q = u + 0.01 * torch.randn(B, H, L, D, generator=g)
    k = u * (v / D ** 0.5).repeat_interleave(128, dim=2).unsqueeze(-1) + 0.01 * torch.randn(B, H, L, D, generator=g)
    return q.to(R.DTYPES[dt]), k.to(R.DTYPES[dt]), L


@pytest.mark.parametrize("D,dt", [(64, "bf16"), (128, "fp16")])
def test_mask_of_the_heaviest_blocks_gives_the_oracle_bit_for_bit(D, dt):
    nb = 10
    q, k, L = _ranked_blocks(nb, D, dt, seed=D)
    pos = np.array([0, 5 * 128 + 3, L - 1], dtype=np.int32)           # three different mask rows
    E = R.block_masses(q, k, pos)
    srt = E.sort(dim=-1, descending=True)[0]
    assert (srt[..., :-1] / srt[..., 1:]).min() > 3.0                  # well separated
    keep = [3, 1, nb]                                                   # kept blocks per head
    mask = torch.zeros(B, H, nb, nb, dtype=torch.uint8)
    for h in range(H):
        top = R.top_mask_row(E[:, h], keep[h])                         # [B,S,nb]
        for s, g in enumerate(pos):
            mask[:, h, g // 128] = top[:, s].to(torch.uint8)
    got = _run(q, k, mask, pos)
    assert np.array_equal(got["row_recall"], got["row_oracle"])
    assert np.array_equal(got["recall"], got["oracle"])
    assert (got["row_kept"] == np.array(keep).reshape(1, H, 1)).all()
    assert (got["row_recall"][:, 2] == 1.0).all() and (got["row_recall"][:, 1] < 1.0).all()
    ref64 = R.recall(q, k, mask, pos)
    _check("ranked", got, ref64, _err32(R.recall(q, k, mask, pos, dtype=torch.float32), ref64))
    # the same budget on the LIGHTEST blocks: the oracle stays, the recall falls
    low = torch.zeros_like(mask)
    for s, g in enumerate(pos):
        low[:, 0, g // 128] = R.top_mask_row(-E[:, 0], 3)[:, s].to(torch.uint8)
    got_low = _run(q, k, low, pos)
    assert np.array_equal(got_low["row_oracle"][:, 0], got["row_oracle"][:, 0])
    assert (got_low["row_recall"][:, 0] < 0.01).all()


def test_equal_block_masses_the_oracle_ignores_which_tied_block_is_taken():
    """Eight identical key blocks: every E_c holds the same bits, so any n kept blocks give the oracle's
    sum bit for bit, and both are n/8 within the bound."""
    nb, D = 8, 64
    L = nb * 128
    q, kd = _qk(B, H, L, D, "bf16", seed=8, temps=[0.5, 1.0, 2.0])
    k = kd[:, :, :128].repeat(1, 1, nb, 1)
    g = np.random.default_rng(5)
    mask = torch.from_numpy((g.random((B, H, nb, nb)) < 0.5).astype(np.uint8))
    pos = g.integers(0, L, size=30).astype(np.int32)
    got = _run(q, k, mask, pos)
    assert np.array_equal(got["row_recall"], got["row_oracle"])
    assert len(np.unique(got["row_kept"])) > 2
    ref64 = R.recall(q, k, mask, pos)
    assert np.abs(ref64["row_recall"] - ref64["row_kept"] / nb).max() < 1e-12
    _check("ties", got, ref64, _err32(R.recall(q, k, mask, pos, dtype=torch.float32), ref64))


def test_large_scores_need_the_max_subtraction():
    """fp16 scores of 300 +- 1.2: exp(300) overflows fp32, the max-subtracted numerators do not."""
    L, D = 1000, 64
    g = torch.Generator().manual_seed(31)
    q = torch.full((B, H, L, D), 6.0).to(torch.float16)
    k = (6.25 + 0.2 * torch.randn(B, H, L, D, generator=g)).to(torch.float16)
    rng = np.random.default_rng(6)
    pos = rng.integers(0, L, size=30).astype(np.int32)
    mask = torch.from_numpy((rng.random((B, H, 8, 8)) < 0.4).astype(np.uint8))
    s = (q[0, 0, :1].double() @ k[0, 0].double().T) / 8
    assert 290 < s.min() and s.max() < 310
    ref64 = R.recall(q, k, mask, pos)
    assert 0.05 < ref64["recall"].min() and ref64["recall"].max() < 0.95
    _check("large", _run(q, k, mask, pos), ref64, _err32(R.recall(q, k, mask, pos, dtype=torch.float32), ref64))


# ------------------------------------------------------------------ addressing and determinism
def test_strided_views_are_read_in_place_and_bit_equal():
    ops = _ops()
    L, D = 1000, 64
    g = torch.Generator().manual_seed(21)
    rng = np.random.default_rng(2)
    pos = rng.integers(0, L, size=30).astype(np.int32)
    rows = torch.from_numpy(rng.permutation(L).astype(np.int32)).to(DEV)
    mask = torch.from_numpy((rng.random((B, H, 8, 8)) < 0.4)).to(DEV)          # a bool mask: viewed as uint8
    for dt in ("bf16", "fp16"):
        qm = torch.randn(B, L, H, D, generator=g).to(DEV, R.DTYPES[dt])
        km = torch.randn(B, L, H, D, generator=g).to(DEV, R.DTYPES[dt])
        q, k = qm.transpose(1, 2), km.transpose(1, 2)
        assert not q.is_contiguous() and ops._aligned_bhld(q) is q
        a = ops.mask_recall(q, k, mask, pos, rows=rows, want_rows=True)
        b = ops.mask_recall(q.contiguous(), k.contiguous(), mask.to(torch.uint8), pos, rows=rows, want_rows=True)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_head_stride_zero_mask_equals_its_expanded_copy():
    ops = _ops()
    L = 1000
    q, k = _qk(B, H, L, 128, "bf16", seed=4, temps=[0.5, 1.0, 2.0])
    q, k = q.to(DEV), k.to(DEV)
    rng = np.random.default_rng(3)
    pos = rng.integers(0, L, size=30).astype(np.int32)
    base = torch.from_numpy((rng.random((B, H, 8, 8)) < 0.4).astype(np.uint8)).to(DEV)
    view = base[:, :1].expand(B, H, 8, 8)
    assert view.stride(1) == 0
    a = ops.mask_recall(q, k, view, pos, want_rows=True)
    b = ops.mask_recall(q, k, view.contiguous(), pos, want_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = ops.mask_recall(q, k, base, pos, want_rows=True)
    assert torch.equal(a[4][:, 0], c[4][:, 0]) and not torch.equal(a[4], c[4])


def test_two_runs_are_bit_equal():
    ops = _ops()
    L = 5000
    q, k = _qk(B, H, L, 128, "bf16", seed=12, temps=[0.5, 1.0, 2.0])
    q, k = q.to(DEV), k.to(DEV)
    rng = np.random.default_rng(1)
    pos = torch.from_numpy(rng.integers(0, L, size=64).astype(np.int32)).to(DEV)
    mask = torch.from_numpy((rng.random((B, H, 40, 40)) < 0.4).astype(np.uint8)).to(DEV)
    a = ops.mask_recall(q, k, mask, pos, want_rows=True)
    b = ops.mask_recall(q, k, mask, pos, want_rows=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = ops.mask_recall(q, k, mask, pos)                               # row outputs NULL: the same statistics
    assert len(c) == 2 and torch.equal(c[0], a[0]) and torch.equal(c[1], a[1])
    # out-of-range device positions are clamped by the kernel
    wild = torch.tensor([-7, L + 100], dtype=torch.int32, device=DEV)
    edge = torch.tensor([0, L - 1], dtype=torch.int32, device=DEV)
    assert all(torch.equal(x, y) for x, y in zip(ops.mask_recall(q, k, mask, wild, want_rows=True),
                                                 ops.mask_recall(q, k, mask, edge, want_rows=True)))


# ------------------------------------------------------------------ the module
# the grids of the judge's module tests; max_retain_ratio = 0.5: at 10-12 blocks the variants' 0.1 / 0.17
# give every row one block
GRIDS = {"cog": dict(width=16, height=12, depth=6, text_length=26),     # L = 1178, 10 blocks
         "wan": dict(width=16, height=12, depth=8, text_length=0)}      # L = 1536, 12 blocks
HEAD_DIM = {"cog": 64, "wan": 128}
HEADS = 4


def _module(variant, **kw):
    import vblade
    return vblade.AdaptiveBlockSparseAttn(variant, log_every=0, max_retain_ratio=0.5, **GRIDS[variant], **kw)


_INPUTS = {}


def _inputs(variant):
    if variant not in _INPUTS:
        gd = GRIDS[variant]
        L = gd["width"] * gd["height"] * gd["depth"] + gd["text_length"]
        g = torch.Generator().manual_seed(40)
        q, k = _qk(1, HEADS, L, HEAD_DIM[variant], "bf16", seed=41, temps=np.linspace(0.2, 3.0, HEADS))
        v = torch.randn(1, HEADS, L, HEAD_DIM[variant], generator=g).to(torch.bfloat16)
        from vblade import attention
        go = torch.Generator(device=DEV).manual_seed(42)
        qo, ko = attention.draw_sample_offsets_qk(1, HEADS, DEV, generator=go)
        _INPUTS[variant] = (q.to(DEV), k.to(DEV), v.to(DEV), qo.contiguous(), ko.contiguous())
    return _INPUTS[variant]


def _module_ref(m, q, k, mask):
    """(ref64, fp32 eager error) of the module's probe on `mask`."""
    rows = m._rows(q.device).cpu().numpy()
    args = (q.cpu(), k.cpu(), mask.cpu(), m.probe_pos.cpu().numpy(), rows)
    ref64 = R.recall(*args, dtype=torch.float64)
    return ref64, _err32(R.recall(*args, dtype=torch.float32), ref64)


def _check_module(tag, m, ref64, err32):
    bound = max(8 * err32, _floor())
    assert m.last_recall.dtype == torch.float32 and m.last_recall.shape == (1, HEADS) and m.last_recall.is_cuda
    for name, got in (("recall", m.last_recall), ("oracle", m.last_oracle_recall)):
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - ref64[name]).max())
        print(f"{tag} {name}: kernel err {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (tag, name, err, bound)


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_module_probe_changes_nothing_and_measures_the_mask_it_used(variant):
    q, k, v, _, _ = _inputs(variant)
    gen = torch.cuda.default_generators[torch.cuda.current_device()]
    res = []
    for kw in (dict(probe="recall"), dict()):
        m = _module(variant, **kw)
        torch.manual_seed(5)
        with torch.no_grad():
            out = m(q, k, v)                                   # the sampling offsets are drawn inside the call
        res.append((m, m.last_mask.clone(), out, gen.get_state().clone(), torch.rand(4, device=DEV)))
    (m, mask, out, state, draw), (plain, mask0, out0, state0, draw0) = res
    assert torch.equal(mask, mask0) and torch.equal(out, out0)
    assert torch.equal(state, state0) and torch.equal(draw, draw0)    # the generator's offset advanced identically
    assert 0 < int(mask.sum()) < mask.numel()
    assert plain.last_recall is None and plain.last_oracle_recall is None and plain.recall is None
    _check_module(variant, m, *_module_ref(m, q, k, mask))
    rec, ora = m.last_recall.cpu(), m.last_oracle_recall.cpu()
    assert (rec <= ora).all() and (ora <= 1).all() and (rec > 0).all() and (rec < 1).any()
    mean = m.recall
    assert torch.equal(mean[0], rec) and torch.equal(mean[1], ora)    # one probed call so far
    # a given block_mask= is probed as well: all ones keep everything
    with torch.no_grad():
        m(q, k, v, block_mask=torch.ones_like(mask))
    assert (m.last_recall == 1).all() and (m.last_oracle_recall == 1).all()
    assert torch.equal(m.recall[0], (rec + 1) / 2)


def test_module_shared_head0_probe_sees_the_view_the_attention_uses():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog", probe="recall", mask_head_mode="shared_head0")
    with torch.no_grad():
        m(q, k, v, q_off=qo, k_off=ko)
    mask = m.last_mask
    used = mask[:, :1].expand_as(mask)
    assert not torch.equal(used.contiguous(), mask)
    _check_module("shared_head0", m, *_module_ref(m, q, k, used))
    own = _ops().mask_recall(q, k, mask, m.probe_pos, rows=m._rows(q.device))
    assert torch.equal(own[0][:, 0], m.last_recall[:, 0]) and not torch.equal(own[0], m.last_recall)


def test_module_probe_every_third_call():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog", probe="recall", probe_every=3)
    probed = []
    with torch.no_grad():
        for i in range(5):
            m.last_recall = None
            m(q, k, v, q_off=qo, k_off=ko)
            probed.append(m.last_recall is not None)
            if probed[-1]:
                first = m.last_recall.clone()
    assert probed == [True, False, False, True, False]
    assert m._recall_count == 2 and torch.equal(m.recall[0], first.cpu())   # the same inputs twice


def test_module_steady_state_call_does_not_synchronise():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog", probe="recall")
    with torch.no_grad():
        a = m(q, k, v, q_off=qo, k_off=ko)
        first = m.last_recall.clone()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            b = m(q, k, v, q_off=qo, k_off=ko)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(a, b) and torch.equal(m.last_recall, first)


def test_module_call_captures_into_a_hip_graph():
    ops = _ops()
    q, k, v, _, _ = _inputs("cog")
    m = _module("cog", probe="recall")
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
        captured = (m.last_mask, m.last_recall, m.last_oracle_recall)
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
    assert torch.equal(m.last_mask, replayed[0])
    assert torch.equal(m.last_recall, replayed[1]) and torch.equal(m.last_oracle_recall, replayed[2])
    assert torch.equal(eager, replayed[3])


def test_module_under_autograd_probes_the_same_mask():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog", probe="recall")
    with torch.no_grad():
        m(q, k, v, q_off=qo, k_off=ko)
    mask, rec, ora = m.last_mask.clone(), m.last_recall.clone(), m.last_oracle_recall.clone()
    qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = m(qq, kk, vv, q_off=qo, k_off=ko)
    assert torch.equal(m.last_mask, mask)
    assert torch.equal(m.last_recall, rec) and torch.equal(m.last_oracle_recall, ora)
    assert not m.last_recall.requires_grad
    out.float().square().sum().backward()
    for t in (qq, kk, vv):
        assert t.grad is not None and torch.isfinite(t.grad.float()).all()


def test_module_without_the_option_has_no_probe():
    q, k, v, qo, ko = _inputs("cog")
    m = _module("cog")
    with torch.no_grad():
        m(q, k, v, q_off=qo, k_off=ko)
    assert m.probe is None and m.last_recall is None and m.last_oracle_recall is None and m.recall is None
