"""Per-row parity of vb_attn_fwd (csrc/vb_attn_fwd.hip) at its tile and tail edges, against the fp64
reference oracle/bsa_oracle.py::joint_attention. The cases, their references and their bounds come
from tests/fwd_cases.py; tests/test_oracle_forward.py checks the bounds themselves on the CPU.

Every case calls ops.attention_fwd twice: with need_lse=True (the training kernel) and without (the
inference kernel: kCBias, kLazy). Per launch:
  * per row: every row's O.per_row_errors(out, ref) <= O.per_row_bound(emu, ref, dtype), 2 x the worst
    per-row error of the rounding emulation of THAT kernel (O.attention_fwd_emulated, prescale_q for
    the inference form) on the same inputs, itself asserted <= 1e-2 bf16 / 1.5e-3 f16. A case with
    one visible key has the bound 0. Every unit-score case is judged this way, against the true
    reference, in both launches.
    Only the rows in which the kernel's running maximum can lag while one key owns the row (weight
    > 0.9, more than one tile, the owning score within the form's slack of the runner-up; they occur
    in peaked, spiked and scale = 0.2 cases only) get a wider bound, from a second emulation whose
    maximum lags in exactly those rows (fwd_cases.row_bounds), also asserted under the cap.
    The inference launch of a peaked, spiked or scale = 0.2 case whose pre-scale rounding alone takes
    more than half the cap is judged against the fp64 oracle on the pre-scaled query instead.
  * whole tensor: relative Frobenius error <= 2 x the emulation's own.
  * LSE (training launch): max |lse - ref| <= 8 x the worst error of the fp32 emulation's LSE against
    fp64 on the same inputs, capped at 2e-5. Each case's worst is recorded (conftest.record).
  * finite outputs; rows of an empty mask row exactly 0 with -inf LSE; with out= a view of a
    NaN-filled buffer, every element outside the view still NaN.

Worst rows over all cases of this file, one MI355X run (the module records its own ranges through
conftest.record; cases with one visible key, where everything is exactly 0, left out of the lower
ends; "bound" = 2 x emulation, per case):
  dtype kernel                 emulation            bound                GPU worst row       GPU/emulation  whole tensor (GPU)
  bf16  training               1.50e-3 .. 3.41e-3   3.00e-3 .. 6.82e-3   up to 3.80e-3       0.95 .. 1.48   up to 2.30e-3
  bf16  inference              1.57e-3 .. 4.92e-3   3.14e-3 .. 9.85e-3   up to 7.41e-3       0.95 .. 1.58   up to 3.07e-3
  bf16  inference, pre-scaled  1.93e-3 .. 2.75e-3   3.85e-3 .. 5.51e-3   3.11e-3 .. 4.82e-3  1.24 .. 2.42   1.94e-3 .. 2.34e-3
  f16   training               1.94e-4 .. 4.38e-4   3.88e-4 .. 8.77e-4   up to 5.12e-4       0.96 .. 1.72   up to 3.11e-4
  f16   inference              2.35e-4 .. 7.43e-4   4.70e-4 .. 1.49e-3   up to 9.59e-4       0.93 .. 1.56   up to 3.69e-4
  f16   inference, pre-scaled  2.49e-4 .. 3.24e-4   4.98e-4 .. 6.49e-4   3.16e-4 .. 5.51e-4  1.13 .. 1.85   2.06e-4 .. 2.70e-4
  lagging rows only            their bound          GPU worst among them
  bf16  training               5.76e-3 .. 7.16e-3   1.54e-3 .. 1.84e-3
  bf16  inference, pre-scaled  6.67e-3 .. 8.56e-3   2.89e-3 .. 4.82e-3
  f16   training               7.94e-4 .. 9.50e-4   1.75e-4 .. 2.28e-4
  f16   inference, pre-scaled  7.98e-4 .. 9.46e-4   2.51e-4 .. 4.93e-4
  LSE (training launch): emulation 2.1e-7 .. 1.5e-5 (above 1.4e-6 only on peaked, spiked or scaled inputs),
  GPU 2.3e-7 .. 1.1e-5, GPU/emulation 0.26 .. 1.80 against the factor of 8: the hardware exp2/log2 and the
  summation order cost less than one more fp32 rounding of an LSE of 3 .. 60. No case came near its bound.
Finding: unlike the backward kernels (0.998 .. 1.003 of their emulation), the forward lands up to
2.4 x above the emulation's worst row, in rows that one key owns (spikes, inference kernel: 4.8e-3
against 2.2e-3 emulated). Cause, read from vb_attn_fwd.hip and reproduced on the CPU by sweeping
the emulation's m_lag: with the exact maximum the owning key's P is exactly 1; the kernels' m is
the first tile's maximum (raised later only past kRescaleSlack or kLazyBound), so that P is
2^(score - m) with a fractional exponent and its rounding to the storage type, up to 2^-8 bf16
of the whole row, goes into O while l sums the unrounded P. That is rounding, not a fault; the
wider bound of the lagging rows is for it and for nothing else.
"""
import numpy as np
import pytest
import torch

import bsa_oracle as O
import fwd_cases as F
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (dtype, what) -> [min, max] over the cases of this run, recorded once at the module's end
RANGES = {}
LSE_RECORD = "forward LSE, worst error per case: gpu / fp32 emulation / bound"


def _note(dtype, what, val):
    key = ("bf16" if dtype == F.BF16 else "f16", what)
    lo, hi = RANGES.get(key, (val, val))
    RANGES[key] = (min(lo, val), max(hi, val))


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()
    yield
    record("forward rows, min..max over the cases run",
           {f"{k[0]} {k[1]}": f"{lo:.2e}..{hi:.2e}" for k, (lo, hi) in sorted(RANGES.items())})


def _ops():
    from vblade import ops
    return ops


def _scatter(x, P):
    """Logical row order -> the caller's (row P[i] of the result is logical row i)."""
    if x is None or P is None:
        return x
    y = torch.empty_like(x)
    y[:, :, P] = x
    return y


def _to_dev(x, strided):
    if x is None:
        return None
    if strided:      # [B,L,H,D] storage viewed [B,H,L,D]
        x = x.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
        assert not x.is_contiguous()
        return x
    return x.to(DEV)


def _mask_to_dev(c, m):
    if m is None:
        return None
    if c.mask == "b_expanded":
        md = m[:1].to(DEV).expand(c.B, -1, -1, -1)
        assert md.stride(0) == 0
    elif c.mask == "h_expanded":
        md = m[:, :1].to(DEV).expand(-1, c.H, -1, -1)
        assert md.stride(1) == 0
    else:
        md = m.contiguous().to(DEV)
    return md


def _launch(c, d, dev, need_lse):
    """One ops.attention_fwd call of the case; returns (out, lse or None) in LOGICAL row order on
    the CPU. With out_view the output goes into a view of a NaN-filled buffer with padded row and
    head strides, and everything outside the view must still be NaN afterwards."""
    kw = dict(block_mask=dev["mask"], q_rows=dev["q_rows"], kv_rows=dev["kv_rows"], kp=dev["kp"], vp=dev["vp"],
              kp_log_bias=d.bias, use_main=c.use_main, scale=c.scale, heavy_rows=c.heavy_rows, need_lse=need_lse)
    buf = None
    if c.out_view:
        buf = torch.full((c.B, c.H, c.Lq + 2, c.D + 8), float("nan"), dtype=c.dtype, device=DEV)
        kw["out"] = buf[:, :, 1:c.Lq + 1, 8:]
    res = _ops().attention_fwd(dev["q"], dev["k"], dev["v"], **kw)
    out, lse = res if need_lse else (res, None)
    if buf is not None:
        assert out.data_ptr() == kw["out"].data_ptr()
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=DEV)
        inside[:, :, 1:c.Lq + 1, 8:] = True
        assert bool(torch.isnan(buf[~inside]).all()), (c.id, "a store outside the out= view")
    out = out.float().cpu()
    lse = lse.cpu() if need_lse else None
    if d.Pq is not None:
        out = out[:, :, d.Pq]
        lse = lse[:, :, d.Pq] if need_lse else None
    return out, lse


def _check_rows(label, dtype, kernel, out, ref, emu_err, bounds, base, whole_emu):
    """``emu_err``: the emulation's worst row; ``bounds`` [B,H,L] per row, ``base`` (every row's bound
    but the lagging ones') and ``whole_emu`` from F.row_bounds."""
    assert torch.isfinite(out).all(), (label, kernel)
    errs = O.per_row_errors(out, ref)
    worst, where = O.per_row_error(out, ref)
    whole = F.frob(out, ref)
    _note(dtype, f"{kernel} rows: emulation", emu_err)
    _note(dtype, f"{kernel} rows: bound", base)
    _note(dtype, f"{kernel} rows: gpu", worst)
    _note(dtype, f"{kernel} rows: gpu/emulation", worst / emu_err if emu_err > 0 else 1.0)
    lagging = bounds > base
    if bool(lagging.any()):
        _note(dtype, f"{kernel} lagging rows: bound", float(bounds.max()))
        _note(dtype, f"{kernel} lagging rows: gpu", float(errs[lagging].max()))
    _note(dtype, f"{kernel} whole: gpu", whole)
    _note(dtype, f"{kernel} whole: gpu/emulation", whole / whole_emu if whole_emu > 0 else 1.0)
    over = errs > bounds
    assert not bool(over.any()), (label, kernel, worst, where, base, float(bounds.max()), int(over.sum()))
    assert whole <= 2.0 * whole_emu, (label, kernel, whole, whole_emu)


def _run(c):
    d, r = F.build(c), F.reference(c)
    dev = dict(q=_to_dev(_scatter(d.q, d.Pq), c.strided), k=_to_dev(_scatter(d.k, d.Pk), c.strided),
               v=_to_dev(_scatter(d.v, d.Pk), c.strided), kp=_to_dev(d.kp, False), vp=_to_dev(d.vp, False),
               mask=_mask_to_dev(c, d.mask),
               q_rows=None if d.Pq is None else d.Pq.int().to(DEV),
               kv_rows=None if d.Pk is None else d.Pk.int().to(DEV))
    empty = torch.isneginf(r.ref_lse)
    # training kernel
    out, lse = _launch(c, d, dev, True)
    assert torch.equal(torch.isneginf(lse), empty) and not torch.isnan(lse).any() and not torch.isposinf(lse).any(), c.id
    assert bool((out[empty] == 0).all()), c.id
    _check_rows(c.id, c.dtype, "training", out, r.ref, r.emu_t_err, r.bounds_t, r.bound_t, r.whole_t)
    err = float((lse.double() - r.ref_lse)[~empty].abs().max())
    _note(c.dtype, "lse: emulation", r.lse_emu_err)
    _note(c.dtype, "lse: gpu", err)
    _note(c.dtype, f"lse, {c.group} cases: gpu", err)
    _note(c.dtype, "lse: gpu/emulation", err / r.lse_emu_err)
    record(LSE_RECORD, f"{c.id} {err:.2e}/{r.lse_emu_err:.2e}/{r.lse_bound:.2e}")
    assert err <= r.lse_bound, (c.id, "lse", err, r.lse_bound, r.lse_emu_err)
    # inference kernel
    out, _ = _launch(c, d, dev, False)
    assert bool((out[empty] == 0).all()), c.id
    _check_rows(c.id, c.dtype, "inference (pre-scaled ref)" if r.prescaled else "inference", out, r.ref_i,
                r.emu_i_ref_err, r.bounds_i, r.bound_i, r.whole_i)


def _ids(c):
    return c.id


@pytest.mark.parametrize("c", F.by_group("keytail"), ids=_ids)
def test_key_tails(c):
    """Lk across every 4-, 8-, 32- and 64-key boundary of the tail mask and of the dropped second
    half, Lk < 64 (the first tile is the tail tile), Lq = 130 != Lk; dense and masked; contiguous and
    through kv_rows (the gathered kernel clamps tail rows to the last valid key)."""
    _run(c)


@pytest.mark.parametrize("c", F.by_group("qtail"), ids=_ids)
def test_query_tails_into_a_padded_out_view(c):
    """Lq around the 32-row wave and the 128-row q-block, with and without q_rows, out= a view of a
    NaN-filled buffer: the 16-byte stores of invalid rows or past a row's end would clear a NaN."""
    _run(c)


@pytest.mark.parametrize("c", F.by_group("pooltail"), ids=_ids)
def test_pooled_tails(c):
    """Lkp around the 32- and 64-key edges with kp_log_bias = ln 15: beside a masked main branch with
    a tail tile of its own, beside an empty mask row (the pooled-only result) and alone."""
    _run(c)


@pytest.mark.parametrize("c", F.by_group("matrix"), ids=_ids)
def test_every_instantiation(c):
    """D x dtype x pooled x gathered K/V, each through the inference and the training kernel: the 32
    non-persistent forms, on one ragged batched shape with heavy_rows = 1 and a q_rows table."""
    _run(c)


@pytest.mark.parametrize("c", F.by_group("args"), ids=_ids)
def test_arguments(c):
    """scale=, a mask expanded over the batch or the heads (stride 0), a mask larger than nbq x nbk,
    q/k/v strided out of [B,L,H,D] storage with a key tail, an empty mask row without a pooled branch."""
    _run(c)


@pytest.mark.parametrize("c", F.by_group("spike"), ids=_ids)
def test_lazy_and_rescale_paths(c):
    """One key = mult x a query, so that row's score jumps past the lazy bound (or, mild, past the
    rescale slack only) in the first or second half of a tile, in the tail tile, in a pooled tile,
    or already in the first tile processed (test_oracle_forward.py checks the placements)."""
    _run(c)


@pytest.mark.parametrize("D,dtype", F.TWO, ids=["64-bf16", "128-f16"])
def test_varlen_entry_with_different_q_and_k_lengths(D, dtype):
    """block_sparse_attn_func with cu_seqlens_q != cu_seqlens_k: q lengths (130, 65) against k lengths
    (193, 64), per row per sequence at the training kernel's bounds (the entry returns the LSE)."""
    import vblade
    H = 2
    lq, lk = [130, 65], [193, 64]
    q = F._rand(sum(lq), H, D, dtype=dtype, seed=7000 + D)
    k, v = (F._rand(sum(lk), H, D, dtype=dtype, seed=7001 + D + s) for s in range(2))
    cu_q = torch.tensor([0] + list(np.cumsum(lq)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(np.cumsum(lk)), dtype=torch.int32)
    mask = O.block_mask_from_density(2, H, 2, 2, 0.5, seed=7003)
    mask[..., -1] = True
    mask[1, :, 0, 0] = True
    out, lse, _ = vblade.block_sparse_attn_func(
        q.to(DEV), k.to(DEV), v.to(DEV), cu_q.to(DEV), cu_k.to(DEV), torch.ones(H, dtype=torch.int32, device=DEV),
        None, mask.to(DEV), max(lq), max(lk), 0.0, deterministic=True, return_attn_probs=True)
    out, lse = out.float().cpu(), lse.cpu()
    assert lse.shape == (2, H, max(lq))
    for bi in range(2):
        sq = q[int(cu_q[bi]):int(cu_q[bi + 1])].permute(1, 0, 2)[None]
        sk, sv = (t[int(cu_k[bi]):int(cu_k[bi + 1])].permute(1, 0, 2)[None] for t in (k, v))
        mb = mask[bi:bi + 1, :, :(lq[bi] + 127) // 128, :(lk[bi] + 127) // 128]
        ref, ref_lse = O.joint_attention(sq, sk, sv, mb)
        emu, emu_lse = O.attention_fwd_emulated(sq, sk, sv, mb, store_dtype=dtype)
        got = out[int(cu_q[bi]):int(cu_q[bi + 1])].permute(1, 0, 2)[None]
        label = f"varlen D={D} seq {bi}"
        can = F.rows_that_can_lag(sq, sk, sv, mb, None, None, 0.0, D ** -0.5, True, "training", dtype)
        assert not bool(can.any())      # unit-normal inputs: no row is owned by one key
        _check_rows(label, dtype, "training", got, ref, O.per_row_error(emu, ref)[0],
                    *F.row_bounds(emu, ref, dtype, can, None))
        bound, emu_err = F.lse_bound(emu_lse, ref_lse)
        err = float((lse[bi, :, :lq[bi]].double() - ref_lse[0]).abs().max())
        _note(dtype, "lse: gpu/emulation", err / emu_err)
        record(LSE_RECORD, f"{label} {err:.2e}/{emu_err:.2e}/{bound:.2e}")
        assert err <= bound, (label, err, bound)
