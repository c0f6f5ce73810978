"""Op-level parity of vb_attn_bwd's two-branch form and of the arguments the module never sets
(kernel_select with a pooled branch, f16 pooled kernels, scale, Lq != Lk, strided inputs, alpha and
LSE edge values, every pooled-key split regime) and of the varlen backward with
cu_seqlens_q != cu_seqlens_k, against oracle/bsa_oracle.py::two_branch_attention_bwd (fp64).

Forward statistics (out1/lse1, out2/lse2) come from ops.attention_fwd(need_lse=True) on the device,
kp/vp from ops.pool_kv; alpha is an explicit constant per row.

Bounds, per gradient:
  * per row: per_row_error(g, ref) <= 2 x the worst per-row error of the oracle's storage-rounding
    emulation against the unrounded reference on the same inputs (O.per_row_bound; computed on the
    CPU each run, never from the kernels; asserted <= 1e-2 bf16 / 1.5e-3 f16). One wrong row — a bad
    pool fold, a wrong tail row, a mis-scattered kv_rows row — fails it; a whole-tensor norm hides it
    behind 1/sqrt(L).
  * whole tensor: relative Frobenius error <= 4e-3 (bf16) / 6e-4 (f16), the existing tight bounds.

Worst-row errors over all cases and gradients of this file, one MI355X run (each case records its
own through conftest.record):
  dtype   CPU emulation          2x bound               measured on the GPU    whole tensor (GPU)
  bf16    3.09e-3 .. 4.66e-3     6.18e-3 .. 9.32e-3     3.09e-3 .. 4.66e-3     2.25e-3 .. 2.46e-3
  f16     4.39e-4 .. 5.72e-4     8.79e-4 .. 1.14e-3     4.39e-4 .. 5.72e-4     2.84e-4 .. 3.05e-4
The kernels land within 0.3 % of the emulation's worst row in every case (ratio 0.998 .. 1.003): the
emulation rounds where they round, so the two differ only where fp32 summation order flips a
rounding. No case needed a rounding step added to the emulation.
"""
import functools
import math
import types

import numpy as np
import pytest
import torch

import bsa_oracle as O
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2
TIGHT = {torch.bfloat16: 4e-3, torch.float16: 6e-4}
NAMES = ("dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _rand(*shape, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _perm(L, seed):
    return torch.randperm(L, generator=torch.Generator().manual_seed(seed))


def rel(x, ref):
    ref = ref.double()
    return ((x.double().cpu() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


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


def _check(label, dtype, grads, ref, emu):
    """grads, ref, emu: (dq, dk, dv) in the same row order. Both bounds of the module docstring."""
    rows, facts = [], []
    for name, g, r, e in zip(NAMES, grads, ref, emu):
        g = g.float().cpu()
        assert torch.isfinite(g).all(), (label, name)
        bound = O.per_row_bound(e, r, dtype)
        worst, where = O.per_row_error(g, r)
        rows.append((name, worst, where, bound, rel(g, r)))
        facts.append(f"{name} {worst:.2e}/{bound / 2:.2e}")
    record("backward worst-row error, gpu/emulation (bound: 2x emulation)", f"{label}: " + " ".join(facts))
    for name, worst, where, bound, whole in rows:
        assert worst <= bound, (label, name, worst, where, bound)
        assert whole <= TIGHT[dtype], (label, name, whole)


class TwoBranch:
    """One two-branch problem: inputs in the caller's row order, the device forward's statistics,
    and the fp64 reference / emulation in REORDERED order (on the heads ``heads`` only)."""

    def __init__(self, B, H, Lq, Lk, D, dtype, gap, density, seed, scale=None, heads=None, alpha=None,
                 edit_mask=None, on_device=False):
        ops = _ops()
        self.dtype, self.gap, self.scale, self.Lq, self.Lk = dtype, gap, scale, Lq, Lk
        self.Pq, self.Pk = _perm(Lq, seed + 10), _perm(Lk, seed + 11)
        if Lq == Lk:
            self.Pk = self.Pq
        if on_device:   # wide-H cases: draw on the device, only the oracle's heads come back
            g = torch.Generator(device=DEV).manual_seed(seed)
            self.q, self.do = (torch.randn(B, H, Lq, D, generator=g, device=DEV).to(dtype) for _ in range(2))
            self.k, self.v = (torch.randn(B, H, Lk, D, generator=g, device=DEV).to(dtype) for _ in range(2))
        else:
            self.q, self.do = _rand(B, H, Lq, D, dtype=dtype, seed=seed).to(DEV), _rand(B, H, Lq, D, dtype=dtype, seed=seed + 3).to(DEV)
            self.k, self.v = _rand(B, H, Lk, D, dtype=dtype, seed=seed + 1).to(DEV), _rand(B, H, Lk, D, dtype=dtype, seed=seed + 2).to(DEV)
        self.mask = O.block_mask_from_density(B, H, (Lq + 127) // 128, (Lk + 127) // 128, density, seed=seed + 4)
        if edit_mask is not None:
            edit_mask(self.mask)
        if alpha is None:
            alpha = torch.rand(B, H, Lq, generator=torch.Generator().manual_seed(seed + 5)) * 0.98 + 0.01
        self.alpha = alpha                                   # caller order, fp32
        self.q_rows, self.kv_rows = self.Pq.int().to(DEV), self.Pk.int().to(DEV)
        self.kp, self.vp, self.k_r, self.v_r = ops.pool_kv(self.k, self.v, gap, self.kv_rows, reordered=True)
        self.out2, self.lse2 = ops.attention_fwd(self.q, None, None, use_main=False, q_rows=self.q_rows,
                                                 kp=self.kp, vp=self.vp, need_lse=True, scale=scale)
        self.out1, self.lse1 = ops.attention_fwd(self.q, self.k_r, self.v_r, block_mask=self.mask.to(DEV),
                                                 q_rows=self.q_rows, need_lse=True, scale=scale)
        self.heads = list(range(H)) if heads is None else heads
        hs = self.heads
        c = lambda t: t[:, hs].cpu()  # noqa: E731
        args = (c(self.q)[:, :, self.Pq], c(self.k)[:, :, self.Pk], c(self.v)[:, :, self.Pk], c(self.kp), c(self.vp),
                c(self.out1)[:, :, self.Pq], c(self.lse1)[:, :, self.Pq], c(self.out2)[:, :, self.Pq],
                c(self.lse2)[:, :, self.Pq], self.alpha[:, hs][:, :, self.Pq], c(self.do)[:, :, self.Pq],
                self.mask[:, hs], gap)
        assert torch.equal(c(self.k_r), args[1])             # pool_kv's reordered copy is the gather
        kw = dict(sm_scale=scale, store_dtype=dtype)
        self.ref = O.two_branch_attention_bwd(*args, **kw)
        self.emu = O.two_branch_attention_bwd(*args, **kw, emulate_rounding=True)

    def backward(self, sel=0, ran=None, ws=None):
        return _ops().attention_bwd(self.do, self.q, self.k_r, self.v_r, self.out1, self.lse1,
                                    block_mask=self.mask.to(DEV), q_rows=self.q_rows, kv_rows=self.kv_rows,
                                    kp=self.kp, vp=self.vp, out2=self.out2, lse2=self.lse2, alpha=self.alpha.to(DEV),
                                    gap=self.gap, scale=self.scale, heavy_rows=2, kernel_select=sel,
                                    kernels_ran=ran, workspace_bytes=ws)

    def reordered(self, grads):
        """(dq, dk, dv) as the call returns them (caller rows) -> the oracle's heads, reordered rows."""
        dq, dk, dv = (g[:, self.heads].float().cpu() for g in grads)
        return dq[:, :, self.Pq], dk[:, :, self.Pk], dv[:, :, self.Pk]


def psplit_of(nbytes, B, H, Lq, D, Lkp, copies=True):
    """The pooled-key split a call used, from the workspace size it asked for (ws_layout in
    csrc/vb_attn_bwd.hip: row statistics, the reordered q/dO copies, the pooled totals, and — only
    for psplit > 1 — psplit copies of them as partials, every region rounded up to 256 bytes)."""
    up = lambda x: (x + 255) & ~255  # noqa: E731
    unit = B * H * Lkp * D * 4
    rest = nbytes - up(B * H * ((Lq + 63) // 64) * 1024) - (2 * up(B * H * Lq * D * 2) if copies else 0) - 2 * up(unit)
    if rest == 0:
        return 1
    s = round(rest / 2 / unit)
    assert s > 1 and 2 * up(s * unit) == rest, (nbytes, rest, unit)
    return s


# ----------------------------------------------------------------------------------------------
# a. every pooled kernel
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_a(D, dtype):
    """B=2, H=3, L=1000, gap=7: Lkp = 143 (two pooled key blocks, the second partial; 143*7 = 1001:
    one replicate-padded row), random row permutation, random alpha. With the default kernels' run."""
    pr = TwoBranch(2, 3, 1000, 1000, D, dtype, gap=7, density=0.3, seed=100 + D)
    ran, ws = [], []
    pr.default = pr.backward(0, ran, ws)
    assert ran == [_ran("default")]
    assert pr.kp.shape[2] == 143
    pr.psplit = psplit_of(ws[0], 2, 3, 1000, D, 143)
    return pr


@pytest.mark.parametrize("sel", ["default", "dkdv_round3", "dq_round3", "dq_ring4"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
def test_every_pooled_kernel_at_the_per_row_bound(D, dtype, sel):
    """bwd_dkdv_pipe_kernel<D,T,true>, bwd_dq_pipe_kernel<D,T,true,2|4>, bwd_dkdv_kernel<D,T,true> and
    bwd_dq_kernel<D,T,true> in both dtypes: each launch asserted from kernels_ran, each result at the
    per-row and whole-tensor bounds; the gradients a selection does not touch are the default's bits.
    psplit clamps to nbq = 8 here (the third split regime, with the two of the next test)."""
    pr = _case_a(D, dtype)
    assert pr.psplit == 8
    if sel == "default":
        grads = pr.default
    else:
        ran = []
        grads = pr.backward(_sel(sel), ran)
        assert ran == [_ran(sel)]
        if sel == "dkdv_round3":
            assert torch.equal(grads[0], pr.default[0])
        else:
            assert torch.equal(grads[1], pr.default[1]) and torch.equal(grads[2], pr.default[2])
    _check(f"a D={D} {dtype} {sel}", dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# b. pooled-key split regimes
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,L,gap,Lkp,want", [(2100, 256, 2, 128, 1), (256, 1700, 15, 114, 12)])
def test_pooled_key_split_regimes(H, L, gap, Lkp, want):
    """psplit = 1 (no reduce launch, the partials alias the totals) and 1 < psplit < nbq with uneven
    q-block ranges (14 q-blocks over 12 splits: ranges of one and two). The regime is read back
    from the workspace size, so a change of the heuristic cannot move a case unnoticed. The oracle
    runs on the first, middle and last head (heads are independent)."""
    D, dtype = 64, torch.bfloat16
    pr = TwoBranch(1, H, L, L, D, dtype, gap=gap, density=0.3, seed=200 + H, heads=[0, H // 2, H - 1],
                   on_device=True)
    assert pr.kp.shape[2] == Lkp
    ran, ws = [], []
    grads = pr.backward(0, ran, ws)
    assert ran == [_ran("default")]
    nbq = (L + 127) // 128
    assert psplit_of(ws[0], 1, H, L, D, Lkp) == want and (want == 1 or 1 < want < nbq)
    if want > 1:
        sizes = {(s + 1) * nbq // want - s * nbq // want for s in range(want)}
        assert sizes == {1, 2}
    _check(f"b H={H} L={L} psplit={want}", dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# c. alpha and LSE edges
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_alpha_and_lse_edges(D):
    """alpha exactly 0 (main branch off) and exactly 1 (storage(1 - alpha) = 0: pooled branch off)
    among random values; head 1's q-block 1 keeps no key block, so the device forward gives
    lse1 = -inf and out1 = 0 there, with alpha 0 and the pooled branch live. The last five rows of
    that block carry alpha = 1 instead: both weights 0, the only rows whose dq must be exactly 0."""
    B, H, L, gap, dtype = 1, 2, 384, 15, torch.bfloat16
    P = _perm(L, 300 + D + 10)                      # TwoBranch's q permutation for this seed
    alpha = torch.rand(B, H, L, generator=torch.Generator().manual_seed(7)) * 0.98 + 0.01
    alpha[0, 0, P[10:20]] = 0.0
    alpha[0, 0, P[20:30]] = 1.0
    alpha[0, 0, P[200:203]] = 1.0
    alpha[0, 1, P[300:310]] = 1.0
    alpha[0, 1, P[128:251]] = 0.0
    alpha[0, 1, P[251:256]] = 1.0

    def empty_row(m):
        m[:, 1, 1, :] = False

    pr = TwoBranch(B, H, L, L, D, dtype, gap=gap, density=0.6, seed=300 + D, alpha=alpha, edit_mask=empty_row)
    assert torch.equal(pr.Pq, P)
    lse1 = pr.lse1.cpu()
    assert torch.isneginf(lse1[0, 1, P[128:256]]).all() and torch.isfinite(lse1[0, 0]).all()
    assert pr.out1[0, 1].cpu()[P[128:256]].abs().max() == 0
    assert torch.isfinite(pr.lse2).all()
    grads = pr.backward()
    _check(f"c D={D}", dtype, pr.reordered(grads), pr.ref, pr.emu)
    w1_dead = ~torch.isfinite(lse1) | (alpha == 0)
    w2_dead = O.rnd(1.0 - alpha, dtype) == 0
    dq_zero = grads[0].float().cpu().abs().amax(-1) == 0
    assert int((w1_dead & w2_dead).sum()) == 5
    assert torch.equal(dq_zero, w1_dead & w2_dead)


# ----------------------------------------------------------------------------------------------
# d. scale, rectangular, strided, batched
# ----------------------------------------------------------------------------------------------
RECT = dict(B=2, H=3, Lq=300, Lk=700, scale=0.2)


@functools.lru_cache(maxsize=None)
def _case_d(D):
    """Main branch only, Lq=300 against Lk=700 (mask 3x6), scale 0.2, q/k/v/dO as [B,L,H,D] storage
    viewed [B,H,L,D] with no row tables: the kernels address the caller's strides directly."""
    B, H, Lq, Lk, scale = (RECT[n] for n in ("B", "H", "Lq", "Lk", "scale"))
    dtype = torch.bfloat16
    qs, dos = _rand(B, Lq, H, D, seed=400 + D), _rand(B, Lq, H, D, seed=403 + D)
    ks, vs = _rand(B, Lk, H, D, seed=401 + D), _rand(B, Lk, H, D, seed=402 + D)
    mask = O.block_mask_from_density(B, H, 3, 6, 0.4, seed=404 + D)
    pr = types.SimpleNamespace()
    pr.cpu = tuple(t.transpose(1, 2) for t in (qs, ks, vs, dos))
    pr.dev = tuple(t.to(DEV).transpose(1, 2) for t in (qs, ks, vs, dos))
    assert not any(t.is_contiguous() for t in pr.dev)
    pr.mask, pr.scale, pr.dtype = mask, scale, dtype
    q, k, v, do = pr.dev
    pr.out, pr.lse = _ops().attention_fwd(q, k, v, block_mask=mask.to(DEV), scale=scale, need_lse=True)
    args = pr.cpu[:3] + (None, None, pr.out.cpu(), pr.lse.cpu(), None, None, None, pr.cpu[3], mask, 0)
    pr.ref = O.two_branch_attention_bwd(*args, sm_scale=scale, store_dtype=dtype)
    pr.emu = O.two_branch_attention_bwd(*args, sm_scale=scale, store_dtype=dtype, emulate_rounding=True)
    return pr


@pytest.mark.parametrize("D", [64, 128])
def test_scaled_rectangular_strided_forwards(D):
    """Both forwards of case d against block_sparse_attention(..., sm_scale=0.2) at the forward tests'
    tolerances: the training kernel (need_lse=True) exactly, the inference kernel (Q pre-scaled by
    scale*log2(e) and rounded to bf16) against the oracle on that pre-scaled query."""
    pr = _case_d(D)
    q, k, v, _ = pr.cpu
    ref, ref_lse = O.block_sparse_attention(q, k, v, pr.mask, sm_scale=pr.scale)
    assert (pr.out.float().cpu() - ref).abs().max() <= 2.5e-2
    assert (pr.lse.cpu() - ref_lse).abs().max() <= 2e-3
    qd, kd, vd, _ = pr.dev
    out = _ops().attention_fwd(qd, kd, vd, block_mask=pr.mask.to(DEV), scale=pr.scale).float().cpu()
    qs = (q.float() * (pr.scale * 1.4426950408889634)).to(q.dtype)
    ref_s, _ = O.block_sparse_attention(qs, k, v, pr.mask, sm_scale=math.log(2.0))
    assert (out - ref_s).abs().max() <= 2.5e-2


@pytest.mark.parametrize("sel", ["default", "dkdv_round3", "dq_round3"])
@pytest.mark.parametrize("D", [64, 128])
def test_scaled_rectangular_strided_backward(D, sel):
    pr = _case_d(D)
    q, k, v, do = pr.dev
    ran = []
    grads = _ops().attention_bwd(do, q, k, v, pr.out, pr.lse, block_mask=pr.mask.to(DEV), scale=pr.scale,
                                 kernel_select=_sel(sel), kernels_ran=ran)
    assert ran == [_ran(sel)]
    assert grads[0].shape[2] == RECT["Lq"] and grads[1].shape[2] == RECT["Lk"]
    _check(f"d D={D} {sel}", pr.dtype, grads, pr.ref, pr.emu)


def test_two_branch_rectangular():
    """Both branches at Lq=300 against Lk=700, gap=15 (Lkp = 47, five replicate-padded rows), scale 0.2,
    separate row permutations for queries and keys."""
    pr = TwoBranch(RECT["B"], RECT["H"], 300, 700, 64, torch.bfloat16, gap=15, density=0.4, seed=500,
                   scale=RECT["scale"])
    assert pr.kp.shape[2] == 47 and not torch.equal(pr.Pq, pr.Pk[:300])
    ran = []
    grads = pr.backward(0, ran)
    assert ran == [_ran("default")]
    _check("d two-branch 300x700", pr.dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# e. varlen backward
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", [(128, torch.float16), (64, torch.bfloat16)], ids=["128-f16", "64-bf16"])
def test_varlen_backward_with_different_q_and_k_lengths(D, dtype):
    """block_sparse_attn_func under autograd with cu_seqlens_q != cu_seqlens_k (q lengths [300, 170]
    against k lengths [200, 420]), softmax_scale 0.2, and an empty q-block row in sequence 0, head 1:
    its forward LSE is +inf (the FlashAttention-2 convention), its dq exactly 0, everything finite.
    Per sequence against the oracle at the per-row bound of the main-branch emulation."""
    import vblade
    H, scale = 2, 0.2
    lq, lk = [300, 170], [200, 420]
    q, do = _rand(sum(lq), H, D, dtype=dtype, seed=600 + D), _rand(sum(lq), H, D, dtype=dtype, seed=603 + D)
    k, v = _rand(sum(lk), H, D, dtype=dtype, seed=601 + D), _rand(sum(lk), H, D, dtype=dtype, seed=602 + D)
    cu_q = torch.tensor([0] + list(np.cumsum(lq)), dtype=torch.int32)
    cu_k = torch.tensor([0] + list(np.cumsum(lk)), dtype=torch.int32)
    mask = O.block_mask_from_density(2, H, 3, 4, 0.5, seed=604)
    mask[0, 1, 1, :] = False
    qd, kd, vd = (t.to(DEV).requires_grad_(True) for t in (q, k, v))
    out, lse, _ = vblade.block_sparse_attn_func(qd, kd, vd, cu_q.to(DEV), cu_k.to(DEV),
                                                torch.ones(H, dtype=torch.int32, device=DEV), None, mask.to(DEV),
                                                max(lq), max(lk), 0.0, deterministic=True, softmax_scale=scale,
                                                return_attn_probs=True)
    out.backward(do.to(DEV))
    lse, out = lse.cpu(), out.detach().cpu()
    assert torch.isposinf(lse[0, 1, 128:256]).all()
    assert qd.grad[128:256, 1].abs().max() == 0
    for bi in range(2):
        sq = lambda t: t[int(cu_q[bi]):int(cu_q[bi + 1])].permute(1, 0, 2)[None]  # noqa: E731
        sk = lambda t: t[int(cu_k[bi]):int(cu_k[bi + 1])].permute(1, 0, 2)[None]  # noqa: E731
        mb = mask[bi:bi + 1, :, :(lq[bi] + 127) // 128, :(lk[bi] + 127) // 128]
        ro, _ = O.block_sparse_attention(sq(q), sk(k), sk(v), mb, sm_scale=scale)
        assert rel(sq(out), ro) <= TOL
        args = (sq(q), sk(k), sk(v), None, None, sq(out), lse[bi:bi + 1, :, :lq[bi]], None, None, None, sq(do), mb, 0)
        ref = O.two_branch_attention_bwd(*args, sm_scale=scale, store_dtype=dtype)
        emu = O.two_branch_attention_bwd(*args, sm_scale=scale, store_dtype=dtype, emulate_rounding=True)
        grads = (sq(qd.grad.cpu()), sk(kd.grad.cpu()), sk(vd.grad.cpu()))
        _check(f"e D={D} {dtype} seq {bi}", dtype, grads, ref, emu)


def test_varlen_sequence_with_keys_but_no_queries_gets_zero_dk_dv():
    """cu_seqlens_q != cu_seqlens_k allows a sequence that has keys and no query (q lengths [300, 0]
    against k lengths [200, 150]). Nothing attends to its keys: their dk/dv are exactly 0, not what
    the output buffers held before the call (they are pre-filled with NaN here). The other sequence
    is unaffected: its gradients at the usual bounds."""
    ops = _ops()
    H, D, dtype = 2, 64, torch.bfloat16
    lq, lk = [300, 0], [200, 150]
    q, do = _rand(sum(lq), H, D, seed=700), _rand(sum(lq), H, D, seed=703)
    k, v = _rand(sum(lk), H, D, seed=701), _rand(sum(lk), H, D, seed=702)
    cu_q = torch.tensor([0, 300, 300], dtype=torch.int32, device=DEV)
    cu_k = torch.tensor([0, 200, 350], dtype=torch.int32, device=DEV)
    mask = O.block_mask_from_density(2, H, 3, 2, 0.6, seed=704)
    hmt = torch.ones(H, dtype=torch.int32, device=DEV)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, do))
    out, lse = ops.block_sparse_attn_fwd(qd, kd, vd, cu_q, cu_k, hmt, None, mask.to(DEV), 300, 200)
    # the caching allocator hands the freed NaN blocks to the call's dq/dk/dv
    junk = [torch.full_like(kd, float("nan")) for _ in range(4)]
    torch.cuda.synchronize()
    del junk
    dq, dk, dv = ops.block_sparse_attn_bwd(dod, qd, kd, vd, out, lse, cu_q, cu_k, hmt, None, mask.to(DEV), 300, 200)
    for g in (dq, dk, dv):
        assert torch.isfinite(g).all()
    assert dk[200:].abs().max() == 0 and dv[200:].abs().max() == 0
    t = lambda x, n: x[:n].permute(1, 0, 2)[None]  # noqa: E731
    args = (t(q, 300), t(k, 200), t(v, 200), None, None, t(out.cpu(), 300), lse.cpu()[:1], None, None, None,
            t(do, 300), mask[:1], 0)
    ref = O.two_branch_attention_bwd(*args, store_dtype=dtype)
    emu = O.two_branch_attention_bwd(*args, store_dtype=dtype, emulate_rounding=True)
    _check("e no-query sequence, seq 0", dtype, (t(dq.cpu(), 300), t(dk.cpu(), 200), t(dv.cpu(), 200)), ref, emu)
