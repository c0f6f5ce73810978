"""Per-row parity of vb_attn_bwd past 256 blocks, where the default dK/dV and dQ kernels
(csrc/vb_attn_bwd_kv.hip) build their block lists in more than one ballot round per wave, against
the gathered fp64 reference (oracle/bsa_oracle.py::two_branch_attention_bwd(gathered=True)). Shapes,
masks and references come from tests/long_bwd_cases.py; tests/test_long_bwd_ref.py checks on the CPU
that the reference equals the dense one and that a lost, doubled or mis-tailed list entry at these
shapes exceeds the bounds used here.

The forward statistics come from the device, so the device forward is judged first, at every shape:
the LSE-returning launch's out per row within 2 x its rounding emulation's worst row, the whole
tensor within 2 x the emulation's Frobenius error, the LSE within 8 x the fp32 emulation's error and
at most 2e-5, the same -inf pattern (the rule of test_gpu_forward_rows.py, on gathered keys).

Gradients: per row O.per_row_error(g, ref) <= O.per_row_bound(emu, ref, dtype) (2 x the emulation's
worst row, capped at 1e-2 bf16 / 1.5e-3 f16); whole tensor <= 4e-3 bf16 / 6e-4 f16 (the bounds of
test_gpu_backward_joint.py); the empty mask row's dq and the unkept key column's dk and dv exactly 0.
Every case records its worst rows through conftest.record.

One MI355X run: backward GPU/emulation worst row 1.000 in every case and gradient (bf16 emulation
3.84e-3 .. 4.70e-3, f16 4.90e-4 .. 5.54e-4; whole tensors 2.33e-3 .. 2.37e-3 bf16, 2.92e-4 .. 2.97e-4
f16); forward training launch 1.12 .. 1.35 x its emulation's worst row, LSE 1.2 .. 1.8 x against the
factor of 8; the inference launch at 1024 blocks 1.20 x on the pre-scaled query. No defect found.
With the ballot rounds past the first ignored in a scratch build, the S1 cases fail at a worst row
of 1.0 and the serial-list kernel's dk, dv differ from the default's.
"""
import functools
import types

import pytest
import torch

import bsa_oracle as O
import long_bwd_cases as C
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = {torch.bfloat16: 4e-3, torch.float16: 6e-4}
NAMES = ("dq", "dk", "dv")
BWD_RECORD = "backward past 256 blocks, worst row: gpu/emulation (bound: 2x emulation)"
FWD_RECORD = "forward past 256 blocks: rows gpu/emulation, whole gpu/emulation, lse gpu/emulation/bound"


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()
    yield
    problem.cache_clear()


def _ops():
    from vblade import ops
    return ops


def _bits():
    from vblade import _lib
    return _lib


def _sel(name):
    lib = _bits()
    return {"default": 0, "dkdv_round3": lib.VB_BWD_SEL_DKDV_ROUND3, "dq_round3": lib.VB_BWD_SEL_DQ_ROUND3,
            "dq_ring4": lib.VB_BWD_SEL_DQ_RING4}[name]


def _ran(name):
    lib = _bits()
    return {"default": lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_PIPE_RING2,
            "dkdv_round3": lib.VB_BWD_RAN_DKDV_ROUND3 | lib.VB_BWD_RAN_DQ_PIPE_RING2,
            "dq_round3": lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_ROUND3,
            "dq_ring4": lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_PIPE_RING4}[name]


def _scatter(x, P):
    """Logical row order -> the caller's (row P[i] of the result is logical row i)."""
    if P is None:
        return x
    y = torch.empty_like(x)
    y[:, :, P] = x
    return y


class Problem:
    """One case on the device: inputs in the caller's row order, the forward's statistics, and (on
    first use) the CPU references in LOGICAL order on the heads ``heads``."""

    def __init__(self, c):
        ops = _ops()
        self.c, self.dtype = c, c.dtype
        self.heads = list(range(c.H)) if c.heads is None else list(c.heads)
        self.mask = C.mask_of(c)
        self.Pq = self.Pk = self.alpha = self.kp = self.vp = self.out2 = self.lse2 = None
        if c.heads is None:
            d = C.build(c)
            self.Pq, self.Pk, self.alpha = d.Pq, d.Pk, d.alpha
            self.q, self.do = _scatter(d.q, d.Pq).to(DEV), _scatter(d.do, d.Pq).to(DEV)
            self.k, self.v = d.k.to(DEV), d.v.to(DEV)                 # keys in reordered (logical) order
        else:   # wide H: drawn on the device, only the reference's heads come back
            g = torch.Generator(device=DEV).manual_seed(c.seed)
            self.q, self.k, self.v, self.do = (torch.randn(1, c.H, c.L, c.D, generator=g, device=DEV).to(c.dtype) for _ in range(4))
            self.alpha = torch.rand(1, c.H, c.L, generator=torch.Generator().manual_seed(c.seed + 5)) * 0.98 + 0.01
        self.mask_dev = self.mask.to(DEV)
        self.q_rows = None if self.Pq is None else self.Pq.int().to(DEV)
        self.kv_rows = None if self.Pk is None else self.Pk.int().to(DEV)
        self.out, self.lse = ops.attention_fwd(self.q, self.k, self.v, block_mask=self.mask_dev, q_rows=self.q_rows, need_lse=True)
        if c.gap:
            self.kp, self.vp = ops.pool_kv(self.k, self.v, c.gap)
            self.out2, self.lse2 = ops.attention_fwd(self.q, None, None, use_main=False, kp=self.kp, vp=self.vp, need_lse=True)
        torch.cuda.synchronize()

    def logical_q(self, t):
        """A [1,H,Lq,...] tensor in the caller's q-row order -> the reference's heads, logical rows, CPU."""
        t = t[:, self.heads].cpu()
        return t if self.Pq is None else t[:, :, self.Pq]

    def logical_k(self, t):
        t = t[:, self.heads].cpu()
        return t if self.Pk is None else t[:, :, self.Pk]

    @functools.cached_property
    def cpu(self):
        hs = self.heads
        x = types.SimpleNamespace(q=self.logical_q(self.q), do=self.logical_q(self.do), k=self.k[:, hs].cpu(), v=self.v[:, hs].cpu(),
                                  mask=self.mask[:, hs], out=self.logical_q(self.out), lse=self.logical_q(self.lse), kw={})
        if self.c.gap:
            x.kw = dict(kp=self.kp[:, hs].cpu(), vp=self.vp[:, hs].cpu(), out2=self.logical_q(self.out2),
                        lse2=self.logical_q(self.lse2), alpha=self.alpha[:, hs], gap=self.c.gap)
        return x

    @functools.cached_property
    def fwd(self):
        x = self.cpu
        return C.forward_reference(x.q, x.k, x.v, x.mask, self.dtype)

    @functools.cached_property
    def bwd(self):
        x = self.cpu
        return C.backward_reference(x.q, x.k, x.v, x.do, x.out, x.lse, x.mask, self.dtype, **x.kw)

    def backward(self, sel=0, ran=None, ws=None, heavy_rows=0):
        kw = {}
        if self.c.gap:
            kw = dict(kp=self.kp, vp=self.vp, out2=self.out2, lse2=self.lse2, alpha=self.alpha.to(DEV), gap=self.c.gap)
        return _ops().attention_bwd(self.do, self.q, self.k, self.v, self.out, self.lse, block_mask=self.mask_dev,
                                    q_rows=self.q_rows, kv_rows=self.kv_rows, heavy_rows=heavy_rows, kernel_select=sel,
                                    kernels_ran=ran, workspace_bytes=ws, **kw)

    @functools.cached_property
    def default(self):
        ran, self.ws = [], []
        grads = self.backward(0, ran, self.ws)
        torch.cuda.synchronize()
        assert ran == [_ran("default")]
        return grads

    def logical(self, grads):
        return self.logical_q(grads[0].float()), self.logical_k(grads[1].float()), self.logical_k(grads[2].float())


@functools.lru_cache(maxsize=None)
def problem(c):
    return Problem(c)


def _check_forward(label, dtype, kernel, out, lse, r):
    assert torch.isfinite(out).all(), (label, kernel)
    errs = O.per_row_errors(out, r.ref)
    worst, where = O.per_row_error(out, r.ref)
    whole = C.frob(out, r.ref)
    facts = f"{label} {kernel}: rows {worst:.2e}/{r.emu_err:.2e} whole {whole:.2e}/{r.whole_emu:.2e}"
    empty = torch.isneginf(r.ref_lse)
    assert bool((out[empty] == 0).all()), label
    err = None
    if lse is not None:
        assert torch.equal(torch.isneginf(lse), empty) and not torch.isnan(lse).any() and not torch.isposinf(lse).any(), label
        err = float((lse.double() - r.ref_lse)[~empty].abs().max())
        facts += f" lse {err:.2e}/{r.lse_emu_err:.2e}/{r.lse_bound:.2e}"
    print(facts)
    record(FWD_RECORD, facts)
    over = errs > r.row_bound
    assert not bool(over.any()), (label, kernel, worst, where, r.row_bound, int(over.sum()))
    assert whole <= 2.0 * r.whole_emu, (label, kernel, whole, r.whole_emu)
    if r.prescaled:
        whole_true = C.frob(out, r.true_ref)
        record(FWD_RECORD, f"{label} {kernel}, true reference: whole {whole_true:.2e}/{r.whole_true:.2e}")
        assert whole_true <= 2.0 * r.whole_true, (label, kernel, whole_true, r.whole_true)
    if lse is not None:
        assert err <= r.lse_bound, (label, "lse", err, r.lse_bound, r.lse_emu_err)


def _check_backward(label, dtype, grads, ref, emu):
    """grads, ref, emu: (dq, dk, dv) in logical row order. Both bounds of the module docstring."""
    rows, facts = [], []
    for name, g, r, e in zip(NAMES, grads, ref, emu):
        assert torch.isfinite(g).all(), (label, name)
        bound = O.per_row_bound(e, r, dtype)
        worst, where = O.per_row_error(g, r)
        rows.append((name, worst, where, bound, C.frob(g, r)))
        facts.append(f"{name} {worst:.2e}/{bound / 2:.2e}")
    print(f"{label}: " + " ".join(facts) + " whole " + " ".join(f"{w:.2e}" for *_, w in rows))
    record(BWD_RECORD, f"{label}: " + " ".join(facts))
    for name, worst, where, bound, whole in rows:
        assert worst <= bound, (label, name, worst, where, bound)
        assert whole <= TIGHT[dtype], (label, name, whole)


def _ids(c):
    return c.id


RUN = [c for c in C.CASES if c.run]


# ----------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RUN, ids=_ids)
def test_training_forward_supplies_sound_statistics(c):
    """The LSE-returning launch at every shape: out and lse of the main branch, which every
    backward case below takes from the device."""
    pr = problem(c)
    _check_forward(c.id, c.dtype, "training", pr.cpu.out.float(), pr.cpu.lse, pr.fwd)


def test_inference_forward_at_the_limit():
    """The inference launch (pre-scaled query, lazy rescale) at 1024 blocks: per row against the fp64
    reference on the pre-scaled query, the whole tensor also against the true reference
    (long_bwd_cases.forward_reference says why the per-row rule cannot hold the cap against the true
    reference over 262144 rows)."""
    c = C.MAIN[-1]
    assert c.nb == 1024
    pr = problem(c)
    out = _ops().attention_fwd(pr.q, pr.k, pr.v, block_mask=pr.mask_dev, q_rows=pr.q_rows)
    x = pr.cpu
    r = C.forward_reference(x.q, x.k, x.v, x.mask, c.dtype, inference=True)
    assert r.prescaled
    _check_forward(c.id, c.dtype, "inference (pre-scaled ref)", pr.logical_q(out).float(), None, r)


# ----------------------------------------------------------------------------------------------
# gradients
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RUN, ids=_ids)
def test_default_kernels_per_row(c):
    """bwd_dkdv_pipe_kernel and bwd_dq_pipe_kernel (ring 2) at 258, 591 and 1024 blocks, with row
    tables at L > 32768, and the two-branch form: per-row and whole-tensor bounds; dq of the empty
    mask row and dk, dv of the key column nobody keeps are exactly 0 (main branch alone)."""
    pr = problem(c)
    grads = pr.logical(pr.default)
    _check_backward(c.id, c.dtype, grads, *pr.bwd)
    if c.gap:
        Lkp = pr.kp.shape[2]
        assert Lkp == (c.L + c.gap - 1) // c.gap
        from test_gpu_backward_branches import psplit_of
        psplit = psplit_of(pr.ws[0], 1, c.H, c.L, c.D, Lkp, copies=False)
        assert (psplit == 1) == (c is C.POOLED_ONE_RANGE), psplit
        return
    at = C.designed_at(c.nb)["empty"]
    e = slice(at * 128, at * 128 + 128)
    assert not bool(pr.mask[0, 0, at].any()) and not bool(pr.mask[0, 1, :, at].any())
    assert grads[0][0, 0, e].abs().max() == 0 and grads[1][0, 1, e].abs().max() == 0 and grads[2][0, 1, e].abs().max() == 0


@pytest.mark.parametrize("sel", ["dkdv_round3", "dq_round3", "dq_ring4"])
def test_selected_kernels_at_591_blocks(sel):
    """The kernel_select variants at S2 (D=128, where no variant shares the default's summation
    order): the launch asserted from kernels_ran, the gradients the selection does not touch the
    default's bits, the ones it does within bf16 rounding of the default's (relative Frobenius
    <= 5e-3), and everything at the per-row bounds. The round-3 kernels build their lists with a
    serial loop."""
    c = C.MAIN[4]
    assert c.nb == 591 and c.D == 128
    pr = problem(c)
    ran = []
    grads = pr.backward(_sel(sel), ran)
    assert ran == [_ran(sel)]
    touched = (1, 2) if sel == "dkdv_round3" else (0,)
    for i in range(3):
        if i in touched:
            assert C.frob(grads[i].float().cpu(), pr.default[i].float().cpu()) <= 5e-3, (sel, NAMES[i])
        else:
            assert torch.equal(grads[i], pr.default[i]), (sel, NAMES[i])
    _check_backward(f"{c.id} {sel}", c.dtype, pr.logical(grads), *pr.bwd)


def test_serial_list_kernel_gives_the_default_bits_at_258_blocks():
    """D=64: the round-3 dK/dV kernel sums in the default's order, and builds its q-lists with a
    serial loop instead of the four-wave ballot: dk and dv bit for bit."""
    pr = problem(C.MAIN[0])
    ran = []
    grads = pr.backward(_sel("dkdv_round3"), ran)
    assert ran == [_ran("dkdv_round3")]
    for a, b in zip(grads, pr.default):
        assert torch.equal(a, b)


def test_heavy_rows_is_scheduling_only_at_258_blocks():
    pr = problem(C.MAIN[0])
    for a, b in zip(pr.backward(heavy_rows=2), pr.default):
        assert torch.equal(a, b)
