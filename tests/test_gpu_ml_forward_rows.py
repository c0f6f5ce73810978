"""Per-row parity of vb_ml_attn_fwd (the kML arm of attn_fwd_item, csrc/vb_attn_fwd.hip) at its tile
and tail edges, against the fp64 reference oracle/ml_oracle.py::multilevel_attention_fp64. The
cases, their references and their bounds come from tests/ml_fwd_cases.py; tests/
test_ml_oracle_forward.py checks the reference and the bounds themselves on the CPU. Only
ops.kv_pyramid and ops.ml_attention_fwd are called.

Every case launches ops.ml_attention_fwd with want_lse=True (the LSE-returning kernel) and without
(the inference kernel: kCBias, lazy maximum); the cases of group a launch each form again with
persistent=True, which must give the plain launch's bits. Per launch, all derived on the CPU from
the emulation (ml_oracle.multilevel_attention_fwd_emulated), never from the kernel:
  * per row: every row's O.per_row_errors(out, ref) <= fwd_cases.row_bounds: 2 x the emulation's
    worst row, asserted <= 1e-2 bf16 / 1.5e-3 f16; rows one key owns while the kernel's running
    maximum can lag get the wider bound of the m_lag emulation, under the same cap. Every unit-score
    case is judged against the true reference in both forms; the inference launch of a spiked or
    scaled case whose pre-scale rounding alone takes more than half the cap is judged against the
    fp64 reference on the pre-scaled query.
  * whole tensor: relative Frobenius error <= 2 x the emulation's.
  * LSE (want_lse launches): max |lse - ref| <= 8 x the fp32 emulation's error, at most 2e-5, and
    the same -inf pattern as the reference; all-skip rows give exact zeros.
  * with out= a view of a NaN-filled buffer every element outside the view is still NaN; group g's
    rows outside the three referenced q-blocks are checked finite.

Worst rows per group from one MI355X run of the whole suite with this file as committed (min .. max
over the group's launches; the module records its own through conftest.record; the one-row cases of
group c, exact or nearly so, left out of the ranges; bound = 2 x emulation, per case):
  group dtype kernel                 emulation            GPU worst row        GPU/emulation  whole tensor (GPU)
  a     bf16  training               2.96e-3 .. 3.10e-3   3.16e-3 .. 3.60e-3   1.07 .. 1.16   2.29e-3 .. 2.30e-3
  a     f16   training               3.70e-4 .. 3.91e-4   3.97e-4 .. 4.58e-4   1.07 .. 1.17   2.85e-4 .. 2.86e-4
  b     bf16  training               3.12e-3 .. 3.43e-3   3.12e-3 .. 3.37e-3   0.93 .. 1.00   2.24e-3 .. 2.31e-3
  b     f16   training               3.46e-4 .. 3.71e-4   3.46e-4 .. 4.33e-4   1.00 .. 1.24   2.79e-4 .. 2.86e-4
  c     bf16  training               2.80e-3 .. 4.38e-3   3.15e-3 .. 4.52e-3   1.00 .. 1.16   1.41e-3 .. 2.29e-3
  c     f16   training               3.32e-4 .. 5.63e-4   3.75e-4 .. 5.63e-4   0.94 .. 1.19   2.45e-4 .. 2.85e-4
  d     bf16  training               2.90e-3 .. 3.17e-3   3.40e-3 .. 3.79e-3   1.14 .. 1.30   2.18e-3 .. 2.23e-3
  d     f16   training               3.45e-4 .. 4.03e-4   3.68e-4 .. 4.30e-4   1.00 .. 1.16   2.74e-4 .. 2.78e-4
  e     bf16  training               2.67e-3 .. 3.05e-3   2.86e-3 .. 3.97e-3   0.98 .. 1.49   2.09e-3 .. 2.26e-3
  e     f16   training               3.04e-4 .. 3.54e-4   3.53e-4 .. 4.49e-4   1.00 .. 1.48   2.43e-4 .. 2.94e-4
  f     bf16  training               2.27e-3 .. 3.21e-3   2.27e-3 .. 3.95e-3   1.00 .. 1.35   1.48e-3 .. 2.32e-3
  f     f16   training               3.25e-4 .. 3.95e-4   4.07e-4 .. 4.74e-4   1.03 .. 1.34   2.65e-4 .. 2.91e-4
  g     bf16  training               3.83e-3              3.79e-3              0.99           2.17e-3
  g     f16   training               5.45e-4              4.55e-4              0.83           2.88e-4
  a     bf16  inference              4.31e-3 .. 4.69e-3   5.14e-3 .. 5.60e-3   1.19           2.69e-3 .. 2.70e-3
  a     f16   inference              5.47e-4 .. 6.56e-4   6.75e-4 .. 8.88e-4   1.23 .. 1.35   3.38e-4
  b     bf16  inference              3.19e-3 .. 4.47e-3   3.19e-3 .. 4.47e-3   1.00 .. 1.03   2.37e-3 .. 2.59e-3
  b     f16   inference              3.83e-4 .. 4.91e-4   3.83e-4 .. 6.04e-4   0.98 .. 1.23   2.92e-4 .. 3.19e-4
  c     bf16  inference              4.01e-3 .. 5.00e-3   3.66e-3 .. 6.13e-3   0.84 .. 1.28   1.55e-3 .. 2.71e-3
  c     f16   inference              4.50e-4 .. 7.49e-4   4.56e-4 .. 7.48e-4   0.88 .. 1.20   2.58e-4 .. 3.38e-4
  d     bf16  inference              4.70e-3 .. 5.00e-3   4.70e-3 .. 5.98e-3   1.00 .. 1.25   2.64e-3 .. 2.72e-3
  d     f16   inference              4.78e-4 .. 5.87e-4   4.87e-4 .. 6.08e-4   0.91 .. 1.07   3.26e-4 .. 3.36e-4
  e     bf16  inference              3.02e-3 .. 4.26e-3   2.98e-3 .. 4.45e-3   0.99 .. 1.04   2.29e-3 .. 2.70e-3
  e     f16   inference              3.92e-4 .. 5.74e-4   4.01e-4 .. 5.33e-4   0.93 .. 1.02   3.12e-4 .. 3.43e-4
  f     bf16  inference              4.23e-3 .. 4.93e-3   5.31e-3 .. 6.52e-3   1.16 .. 1.43   2.70e-3 .. 2.78e-3
  f     f16   inference              4.96e-4 .. 7.13e-4   6.26e-4 .. 1.04e-3   1.09 .. 1.53   3.05e-4 .. 3.50e-4
  g     bf16  inference              4.23e-3              6.41e-3              1.52           2.62e-3
  g     f16   inference              5.67e-4              7.08e-4              1.25           3.38e-4
  e     bf16  inference, pre-scaled  2.79e-3              3.92e-3              1.41           2.14e-3
  e     f16   inference, pre-scaled  3.15e-4              5.47e-4              1.73           2.66e-4
  f     bf16  inference, pre-scaled  2.26e-3 .. 3.36e-3   3.47e-3 .. 5.00e-3   1.03 .. 2.16   2.08e-3 .. 2.37e-3
  lagging rows only                  their bound          GPU worst among them
  e     f16   inference, pre-scaled  8.78e-4              3.18e-4
  f     bf16  inference, pre-scaled  7.71e-3 .. 8.69e-3   3.99e-3 .. 5.00e-3
  LSE (want_lse launches): emulation 3.0e-7 .. 1.1e-5 (above 1.7e-6 only in the spiked and scaled cases),
  GPU 3.0e-7 .. 1.1e-5, GPU/emulation 0.45 .. 1.73 against the factor of 8.
Every launch landed inside its derived bounds: the new cases exposed no kernel error, and the
emulation needed no rounding step added. As in the plain forward (test_gpu_forward_rows.py), the
inference kernel lands furthest above the emulation's worst row, 2.16 x, in rows one key owns (the
huge late maxima): the owning key's P is 2^(score - m) with a lagging m and rounds like any other,
which the lagging rows' bound is for. The persistent launches of group a gave the plain launches'
bits in all eight instantiations.
"""
import pytest
import torch

import bsa_oracle as O
import fwd_cases as F
import ml_fwd_cases as M
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (group, dtype, what) -> [min, max] over the launches of this run, recorded at the module's end
RANGES = {}
ROW_RECORD = "multi-level forward rows, per launch: gpu worst row / emulation worst row = ratio"


def _note(c, what, val):
    key = (c.group, "bf16" if c.dtype == M.BF16 else "f16", what)
    lo, hi = RANGES.get(key, (val, val))
    RANGES[key] = (min(lo, val), max(hi, val))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()
    yield
    record("multi-level forward rows, min..max over the launches run",
           {" ".join(k): f"{lo:.2e}..{hi:.2e}" for k, (lo, hi) in sorted(RANGES.items())})


def _ops():
    from vblade import ops
    return ops


def _scatter(x, P):
    """Logical row order -> the caller's (row P[i] of the result is logical row i)."""
    if P is None:
        return x
    y = torch.empty_like(x)
    y[:, :, P] = x
    return y


def _device_inputs(c, d):
    """q, the pyramids (ops.kv_pyramid of k, v in the caller's row order through the row table), the
    uint8 mask and the row table on the device, in the form the case's ``io`` asks for."""
    q, k, v = (_scatter(t, d.P) for t in (d.q, d.k, d.v))
    if c.io == "q_strided":          # [B,L,H,D] storage viewed [B,H,L,D]
        qd = q.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
        assert not qd.is_contiguous()
    else:
        qd = q.to(DEV)
    rows = None if d.P is None else d.P.int().to(DEV)
    kp, vp = _ops().kv_pyramid(k.to(DEV), v.to(DEV), rows)
    m8 = d.mask.clamp(0, 255).to(torch.uint8)
    if c.io == "mask_h_expanded":
        md = m8[:, :1].contiguous().to(DEV).expand(-1, c.H, -1, -1)
        assert md.stride(1) == 0
    elif c.io == "mask_strided":     # every second byte of a wider buffer: last-dim stride 2
        wide = torch.full((c.B, c.H, c.nb, 2 * c.nb), 1, dtype=torch.uint8, device=DEV)
        wide[..., ::2] = m8.to(DEV)
        md = wide[..., ::2]
        assert md.stride(-1) == 2
    else:
        md = m8.contiguous().to(DEV)
    return dict(q=qd, kp=kp, vp=vp, mask=md, rows=rows)


def _launch(c, dev, want_lse, persistent=False):
    """One ops.ml_attention_fwd call; returns the device tensors (out, lse or None). With out_view the
    output goes into a view of a NaN-filled buffer with padded row and head strides, and everything
    outside the view must still be NaN afterwards."""
    kw = dict(q_rows=dev["rows"], scale=c.scale, ref_tail=c.ref_tail, want_lse=want_lse, persistent=persistent)
    buf = None
    if c.io == "out_view":
        buf = torch.full((c.B, c.H, c.L + 2, c.D + 8), float("nan"), dtype=c.dtype, device=DEV)
        kw["out"] = buf[:, :, 1:c.L + 1, 8:]
    if c.io == "blhd":
        kw["out_layout"] = "blhd"
    res = _ops().ml_attention_fwd(dev["q"], dev["kp"], dev["vp"], dev["mask"], **kw)
    out, lse = res if want_lse else (res, None)
    assert tuple(out.shape) == (c.B, c.H, c.L, c.D) and out.dtype == c.dtype
    if buf is not None:
        assert out.data_ptr() == kw["out"].data_ptr()
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
        inside[:, :, 1:c.L + 1, 8:] = True
        assert bool(torch.isnan(buf[~inside]).all()), (c.id, "a store outside the out= view")
    if c.io == "blhd":
        assert out.transpose(1, 2).is_contiguous()
    return out, lse


def _logical(c, d, out, lse):
    """Device results -> the CPU, logical row order, the case's referenced rows. The rows that get no
    reference (group g) are checked finite here."""
    out = out.float().cpu()
    lse = None if lse is None else lse.cpu()
    if d.P is not None:      # out and lse are both written at the caller's rows
        out = out[:, :, d.P]
        lse = None if lse is None else lse[:, :, d.P]
    assert torch.isfinite(out).all(), c.id
    if d.sel is not None:
        if lse is not None:
            assert not torch.isnan(lse).any() and not torch.isposinf(lse).any(), c.id
            lse = lse[:, :, d.sel]
        out = out[:, :, d.sel]
    return out, lse


def _check_rows(c, kernel, out, ref, emu_err, bounds, base, whole_emu):
    """``emu_err``: the emulation's worst row; ``bounds`` per row, ``base`` (every row's bound but the
    lagging ones') and ``whole_emu`` from fwd_cases.row_bounds."""
    errs = O.per_row_errors(out, ref)
    worst, where = O.per_row_error(out, ref)
    whole = F.frob(out, ref)
    ratio = worst / emu_err if emu_err > 0 else 1.0
    if emu_err > 1e-4:      # the one-row cases (exact or nearly so) would only blur the ranges
        _note(c, f"{kernel} rows: emulation", emu_err)
        _note(c, f"{kernel} rows: gpu", worst)
        _note(c, f"{kernel} rows: gpu/emulation", ratio)
        _note(c, f"{kernel} whole: gpu", whole)
    lagging = bounds > base
    if bool(lagging.any()):
        _note(c, f"{kernel} lagging rows: bound", float(bounds.max()))
        _note(c, f"{kernel} lagging rows: gpu", float(errs[lagging].max()))
    record(ROW_RECORD, f"{c.id} {kernel} {worst:.2e}/{emu_err:.2e}={ratio:.2f}")
    over = errs > bounds
    assert not bool(over.any()), (c.id, kernel, worst, where, base, float(bounds.max()), int(over.sum()))
    assert whole <= 2.0 * whole_emu, (c.id, kernel, whole, whole_emu)


def _run(c):
    d, r = M.build(c), M.reference(c)
    dev = _device_inputs(c, d)
    empty = torch.isneginf(r.ref_lse)
    # the LSE-returning kernel
    out_t, lse_t = _launch(c, dev, True)
    out, lse = _logical(c, d, out_t, lse_t)
    assert torch.equal(torch.isneginf(lse), empty) and not torch.isnan(lse).any() and not torch.isposinf(lse).any(), c.id
    assert bool((out[empty] == 0).all()), c.id
    _check_rows(c, "training", out, r.ref, r.emu_t_err, r.bounds_t, r.bound_t, r.whole_t)
    err = float((lse.double() - r.ref_lse)[~empty].abs().max())
    _note(c, "lse: emulation", r.lse_emu_err)
    _note(c, "lse: gpu", err)
    _note(c, "lse: gpu/emulation", err / r.lse_emu_err)
    assert err <= r.lse_bound, (c.id, "lse", err, r.lse_bound, r.lse_emu_err)
    # the inference kernel
    out_i, _ = _launch(c, dev, False)
    out, _ = _logical(c, d, out_i, None)
    assert bool((out[empty] == 0).all()), c.id
    _check_rows(c, "inference (pre-scaled ref)" if r.prescaled else "inference", out, r.ref_i, r.emu_i_ref_err,
                r.bounds_i, r.bound_i, r.whole_i)
    if c.persistent:
        out_p, lse_p = _launch(c, dev, True, persistent=True)
        assert torch.equal(out_p, out_t) and torch.equal(lse_p, lse_t), (c.id, "persistent, LSE-returning")
        out_p, _ = _launch(c, dev, False, persistent=True)
        assert torch.equal(out_p, out_i), (c.id, "persistent, inference")
        assert int(_ops().work_queue(out_p.device).abs().sum()) == 0


def _ids(c):
    return c.id


@pytest.mark.parametrize("c", M.by_group("a"), ids=_ids)
def test_every_instantiation(c):
    """D x dtype, LSE-returning and inference, plain and persistent (16 launches): B=2, H=2, L=1100
    (9 blocks, a 76-row tail), the backward file's random level mix, a row permutation; the
    persistent launches give the plain launches' bits."""
    _run(c)


@pytest.mark.parametrize("c", M.by_group("b"), ids=_ids)
def test_tile_packing(c):
    """One mask row per q-block: n4 in 1..5 and n8 in 1..7, 9, 10, each alone and beside other levels,
    kept blocks first, last and scattered (both (wave & 1) halves, the min(e, n - 1) clamps, klen of a
    short last tile); a single level-1, level-2 and level-8 block."""
    _run(c)


@pytest.mark.parametrize("c", M.by_group("c"), ids=_ids)
def test_tails(c):
    """L = 256 + r, r across the 64-key half and the `ntm -= 1` boundary, under both tail rules, with
    the last column at every level (pooled levels read replicate-padded pyramid rows); L of one
    block, 1 .. 127 rows, at each level."""
    _run(c)


@pytest.mark.parametrize("c", M.by_group("d"), ids=_ids)
def test_io_surface(c):
    """B=2: out= a view of a NaN-filled buffer with a query tail, q strided out of [B,L,H,D] storage,
    out_layout="blhd", a mask expanded over the heads (stride 0), a mask with last-dim stride 2."""
    _run(c)


@pytest.mark.parametrize("c", M.by_group("e"), ids=_ids)
def test_values(c):
    """scale = 0.2 and 0.05; mask bytes 3, 5, 16, 255 keep nothing; an all-skip row (made of such
    bytes) gives exact zeros and a -inf LSE."""
    _run(c)


@pytest.mark.parametrize("c", M.by_group("f"), ids=_ids)
def test_late_maxima(c):
    """One key = mult x a query (an aligned run of p keys, so the level-p pooled row equals it) in a
    later level-1 tile, the level-2 tile, the second block of the packed level-4 tile or the third of
    the packed level-8 tile: past the rescale slack only (mild) or past the lazy bound (huge)."""
    _run(c)


@pytest.mark.parametrize("c", M.by_group("g"), ids=_ids)
def test_lists_longer_than_one_ballot_pass(c):
    """L = 8500, 67 key blocks: both passes of the list-building ballots carry counts and positions
    over column 64. q-blocks 0, 33 and 66 at the bounds, every other row finite."""
    _run(c)
