"""Op-level parity of vb_ml_attn_bwd (the multi-level backward) at the edges of its own logic: the
pooled dK/dV items' union q-lists and block bitmaps, the dQ kernels' packed level-4 / level-8 tiles
with partial last tiles, the level-1 tail rule, the 1/2, 1/4, 1/8 fold, all-skip rows and columns,
lists longer than one 64-lane ballot pass, and the arguments the module never sets; against
oracle/ml_oracle.py::multilevel_attention_bwd_lse (fp64).

The forward's out and lse come from ops.ml_attention_fwd(want_lse=True) on the device, the pyramids
from ops.kv_pyramid; the reference and its rounding emulation are computed on the CPU from them.

Bounds, per gradient (as tests/test_gpu_backward_branches.py):
  * per row: per_row_error(g, ref) <= 2 x the worst per-row error of the oracle's storage-rounding
    emulation against the unrounded reference on the same inputs (O.per_row_bound; computed on the
    CPU each run, never from the kernels; asserted <= 1e-2 bf16 / 1.5e-3 f16). One dropped
    (q-block, key-block) pair of any level or a wrong fold weight exceeds it several times over
    (tests/test_ml_oracle_backward.py); the whole-tensor norm at 2e-2 lets a level-8 pair through.
  * whole tensor: relative Frobenius error <= 4e-3 (bf16) / 6e-4 (f16), the existing tight bounds.

Worst-row errors over the gradients and kernel selections of each case, from one MI355X run of the
whole suite with this file as committed (each case records its own through conftest.record):
  case  dtype  CPU emulation        2x bound             measured on the GPU  gpu/emulation  whole tensor (GPU)
  a     bf16   3.53e-3 .. 4.28e-3   7.06e-3 .. 8.56e-3   3.53e-3 .. 4.28e-3   1.000          2.35e-3 .. 2.37e-3
  a     f16    4.39e-4 .. 5.02e-4   8.78e-4 .. 1.00e-3   4.39e-4 .. 5.02e-4   1.000          2.92e-4 .. 2.96e-4
  b     bf16   3.11e-3 .. 3.99e-3   6.22e-3 .. 7.98e-3   3.11e-3 .. 3.99e-3   1.000          2.34e-3 .. 2.38e-3
  c     bf16   3.29e-3 .. 4.80e-3   6.58e-3 .. 9.60e-3   3.29e-3 .. 4.80e-3   1.000          2.20e-3 .. 2.50e-3
  c     f16    2.03e-4 .. 5.79e-4   4.06e-4 .. 1.16e-3   2.03e-4 .. 5.79e-4   0.998 .. 1.002 2.00e-4 .. 2.98e-4
  d     bf16   3.38e-3 .. 4.08e-3   6.76e-3 .. 8.16e-3   3.38e-3 .. 4.08e-3   1.000          2.34e-3 .. 2.36e-3
  e     bf16   4.04e-3 .. 4.36e-3   8.08e-3 .. 8.72e-3   4.04e-3 .. 4.36e-3   1.000          2.34e-3 .. 2.41e-3
  f     bf16   3.30e-3 .. 3.88e-3   6.60e-3 .. 7.76e-3   3.30e-3 .. 3.88e-3   1.000          2.36e-3 .. 2.39e-3
The kernels land within 0.2 % of the emulation's worst row in every case: the emulation rounds where
they round (P and dS as MFMA operands, dq/dk/dv once after the fp32 fold), so the two differ only
where fp32 summation order flips a rounding. No case needed a rounding step added to the emulation,
and no case exposed a kernel error.
"""
import functools

import pytest
import torch

import bsa_oracle as O
import ml_oracle as ML
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = {torch.bfloat16: 4e-3, torch.float16: 6e-4}
NAMES = ("dq", "dk", "dv")
SELS = ["default", "dkdv_round3", "dq_round3"]
MIX = (0.15, 0.15, 0.15, 0.25, 0.3)


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _rand(*shape, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _random_levels(B, H, nb, seed, p=MIX):
    """Random level masks (values 1,2,4,8,0 with probabilities p) plus the forced last column."""
    g = torch.Generator().manual_seed(seed)
    lv = torch.tensor([1, 2, 4, 8, 0], dtype=torch.int32)
    idx = torch.multinomial(torch.tensor(p), B * H * nb * nb, replacement=True, generator=g)
    m = lv[idx].reshape(B, H, nb, nb)
    m[..., -1] = 1
    return m


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
    return {"default": 0, "dkdv_round3": lib.VB_BWD_SEL_DKDV_ROUND3, "dq_round3": lib.VB_BWD_SEL_DQ_ROUND3}[name]


def _ran(name):
    lib = _bits()
    dkdv = lib.VB_BWD_RAN_DKDV_ROUND3 if name == "dkdv_round3" else lib.VB_BWD_RAN_DKDV_PIPE
    dq = lib.VB_BWD_RAN_DQ_ROUND3 if name == "dq_round3" else lib.VB_BWD_RAN_DQ_PIPE_RING2
    return lib.VB_BWD_RAN_ML_PYRAMID | dkdv | dq


def _check(label, dtype, grads, ref, emu):
    """grads, ref, emu: (dq, dk, dv) in the same row order. Both bounds of the module docstring."""
    rows, facts = [], []
    for name, g, r, e in zip(NAMES, grads, ref, emu):
        g = g.float().cpu()
        assert torch.isfinite(g).all(), (label, name)
        bound = O.per_row_bound(e, r, dtype)
        worst, where = O.per_row_error(g, r)
        whole = rel(g, r)
        rows.append((name, worst, where, bound, whole))
        facts.append(f"{name} {worst:.2e}/{bound / 2:.2e}={worst / (bound / 2):.3f} whole {whole:.2e}")
    record("multi-level backward worst-row error, gpu/emulation (bound: 2x emulation)", f"{label}: " + " ".join(facts))
    for name, worst, where, bound, whole in rows:
        assert worst <= bound, (label, name, worst, where, bound)
        assert whole <= TIGHT[dtype], (label, name, whole)


class Problem:
    """One multi-level problem: inputs in the caller's row order, the device's pyramids and forward
    (out, lse), and the fp64 reference / emulation in REORDERED row order. ``mask`` int [B,H|1,nb,nb]
    (one head: expanded over the heads with stride 0); ``strided``: q/out/dout are [B,L,H,D] storage
    viewed [B,H,L,D]."""

    def __init__(self, B, H, L, D, dtype, mask, seed, perm=True, ref_tail=True, scale=None, strided=False):
        ops = _ops()
        self.dtype, self.L, self.ref_tail, self.scale = dtype, L, ref_tail, scale
        shape = (B, L, H, D) if strided else (B, H, L, D)
        view = (lambda t: t.transpose(1, 2)) if strided else (lambda t: t)
        q, k, v, do = (_rand(*shape, dtype=dtype, seed=seed + s) for s in range(4))
        self.cpu = tuple(view(t) for t in (q, k, v, do))
        self.q, self.k, self.v, self.do = (view(t.to(DEV)) for t in (q, k, v, do))
        self.P = torch.randperm(L, generator=torch.Generator().manual_seed(seed + 9)) if perm else None
        self.rows = self.P.int().to(DEV) if perm else None
        self.mask = mask.expand(B, H, -1, -1)
        self.md = mask.clamp(0, 255).to(torch.uint8).to(DEV).expand(B, H, -1, -1)
        self.kp, self.vp = ops.kv_pyramid(self.k, self.v, self.rows)
        out = view(torch.empty(*shape, device=DEV, dtype=dtype)) if strided else None
        self.out, self.lse = ops.ml_attention_fwd(self.q, self.kp, self.vp, self.md, q_rows=self.rows, scale=scale,
                                                  ref_tail=ref_tail, want_lse=True, out=out)
        assert self.out.is_contiguous() != strided
        r = self.reordered
        qr, kr, vr, dor = r(self.cpu)
        out_r, lse_r = r((self.out, self.lse))     # both at the caller's rows
        args = (qr, kr, vr, self.mask, out_r, lse_r, dor)
        kw = dict(sm_scale=scale, ref_tail=ref_tail, store_dtype=dtype)
        self.ref = ML.multilevel_attention_bwd_lse(*args, **kw)
        self.emu = ML.multilevel_attention_bwd_lse(*args, **kw, emulate_rounding=True)

    def backward(self, sel=0, ran=None, ws=None, grads=None, heavy_rows=2, sample=None):
        s = slice(None) if sample is None else slice(sample, sample + 1)
        return _ops().ml_attention_bwd(self.do[s], self.q[s], self.kp[s], self.vp[s], self.md[s], self.out[s],
                                       self.lse[s], rows=self.rows, scale=self.scale, ref_tail=self.ref_tail,
                                       heavy_rows=heavy_rows, kernel_select=sel, kernels_ran=ran,
                                       grads=grads, workspace_bytes=ws)

    def reordered(self, ts):
        """[B,H,L,*] tensors in the caller's row order -> on the CPU in reordered row order."""
        ts = tuple(t.cpu() for t in ts)
        return ts if self.P is None else tuple(t[:, :, self.P] for t in ts)

    def run_sel(self, sel, default):
        """The gradients of selection ``sel`` with the launches asserted from kernels_ran; the gradients
        a selection does not touch are the default launch's bits."""
        if sel == "default":
            return default
        ran = []
        grads = self.backward(_sel(sel), ran)
        assert ran == [_ran(sel)]
        if sel == "dkdv_round3":
            assert torch.equal(grads[0], default[0])
        else:
            assert torch.equal(grads[1], default[1]) and torch.equal(grads[2], default[2])
        return grads


def _default(pr):
    ran = []
    grads = pr.backward(0, ran)
    assert ran == [_ran("default")]
    return grads


def ml_workspace_bytes(B, H, L, D, copies):
    """ml_ws_layout of csrc/vb_attn_bwd.hip: the row statistics, the reordered q/dO copies (only with
    a row table), the fp32 level-2/4/8 pyramid partials of dK and dV; regions rounded up to 256 B."""
    up = lambda x: (x + 255) & ~255  # noqa: E731
    lpad = (L + 127) // 128 * 128
    n = up(B * H * ((L + 63) // 64) * 1024)
    if copies:
        n += 2 * up(B * H * L * D * 2)
    return n + 2 * up(B * H * (7 * lpad // 8) * D * 4)


# ----------------------------------------------------------------------------------------------
# a. every kernel
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_a(D, dtype):
    """B=2, H=2, L=1100: 9 key blocks, so the last level-8 item is partial at both D (D=64 items cover
    4 blocks, D=128 items 8), as are the last level-4 and level-2 items at D=128; a 76-row tail
    block; random row permutation; the random level mix with skips. ref_tail False on half the grid."""
    ref_tail = (D == 64) == (dtype == torch.bfloat16)
    pr = Problem(2, 2, 1100, D, dtype, _random_levels(2, 2, 9, seed=1100 + 7 * D), seed=100 + D, ref_tail=ref_tail)
    ran, ws = [], []
    pr.default = pr.backward(0, ran, ws)
    assert ran == [_ran("default")]
    assert ws == [ml_workspace_bytes(2, 2, 1100, D, True)]
    return pr


@pytest.mark.parametrize("sel", SELS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
def test_every_kernel_at_the_per_row_bound(D, dtype, sel):
    """bwd_dkdv_kernel<D,T,true,true,kW> (the pooled levels), bwd_dkdv_pipe / bwd_dkdv_kernel<kML>
    (level 1 and the fold), bwd_dq_pipe_kernel<kML> / bwd_dq_kernel<kML> in both dtypes: each launch
    asserted from kernels_ran, each result at the per-row and whole-tensor bounds."""
    pr = _case_a(D, dtype)
    grads = pr.run_sel(sel, pr.default)
    _check(f"a D={D} {str(dtype)[6:]} {sel}", dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# b. level coverage and partial tiles
# ----------------------------------------------------------------------------------------------
def _coverage_rows():
    """The ten mask rows of test_ml_forward_level_coverage_and_partial_tiles."""
    m = torch.zeros(10, 10, dtype=torch.int32)
    m[0, :] = 8                      # 10 level-8 blocks -> dQ tiles of 4, 4, 2
    m[1, :3] = 4                     # 3 level-4 blocks -> dQ tiles of 2, 1
    m[2, ::3] = 2
    m[3, 5] = 1
    m[4, :] = torch.tensor([1, 2, 4, 8, 0, 8, 4, 2, 1, 8], dtype=torch.int32)
    m[5, :] = torch.tensor([8, 8, 8, 8, 8, 4, 0, 0, 0, 0], dtype=torch.int32)
    m[6, :] = 1
    m[7, 9] = 8
    m[8, :] = torch.tensor([3, 5, 16, 1, 0, 0, 0, 0, 0, 0], dtype=torch.int32)  # non-levels skip
    return m                         # row 9 stays all zero


@functools.lru_cache(maxsize=None)
def _case_b(D):
    """L=1280 (nb=10), H=2, no row table: head 0 takes the forward test's ten rows (q-block 9 keeps
    nothing), head 1 their transpose, so key columns see those patterns in their q-lists (key block
    9 is kept by no q-block)."""
    m = _coverage_rows()
    mask = torch.stack([m, m.t().contiguous()])[None]
    pr = Problem(1, 2, 1280, D, torch.bfloat16, mask, seed=200 + D, perm=False)
    pr.default = _default(pr)
    return pr


@pytest.mark.parametrize("sel", SELS)
@pytest.mark.parametrize("D", [64, 128])
def test_level_coverage_and_partial_tiles(D, sel):
    """The backward twin of the forward's structured test. dq of the all-skip q-block (lse = -inf in
    the prep kernel) and dk/dv of the never-kept key block are exactly zero, written over NaN-filled
    caller buffers (dq/dk/dv are fully overwritten); everything else at the per-row bounds."""
    pr = _case_b(D)
    assert torch.isinf(pr.lse[0, 0, 9 * 128:]).all() and torch.isfinite(pr.lse[0, 1]).all()
    grads = pr.run_sel(sel, pr.default)
    bufs = tuple(torch.full_like(pr.q, float("nan")) for _ in range(3))
    ran = []
    got = pr.backward(_sel(sel), ran, grads=bufs)
    assert ran == [_ran(sel)]
    for a, b, c in zip(got, bufs, grads):
        assert a is b and torch.equal(a, c)
    _check(f"b D={D} {sel}", pr.dtype, pr.reordered(got), pr.ref, pr.emu)
    dq, dk, dv = got
    assert dq[0, 0, 9 * 128:].abs().max() == 0
    assert dk[0, 1, 9 * 128:].abs().max() == 0 and dv[0, 1, 9 * 128:].abs().max() == 0
    # nothing else is zero: every other q-block and key block takes part
    assert bool((dq[0, 0, :9 * 128].float().abs().amax(-1) > 0).all()) and bool((dq[0, 1].float().abs().amax(-1) > 0).all())
    assert bool((dk[0, 0].float().abs().amax(-1) > 0).all()) and bool((dk[0, 1, :9 * 128].float().abs().amax(-1) > 0).all())


# ----------------------------------------------------------------------------------------------
# c. tails and the fold at odd lengths
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_c(L, ref_tail, D, dtype):
    """B=2, H=2, random levels and row permutation; the last key column is forced to level
    (1, 2, 4, 8)[(i + 2h + b) % 4] in q-block i: every level reaches the tail block (and the
    replicate-padded pyramid rows behind it) in some (b, h) even with one q-block."""
    nb = (L + 127) // 128
    mask = _random_levels(2, 2, nb, seed=3 * L + D)
    for b in range(2):
        for h in range(2):
            for i in range(nb):
                mask[b, h, i, -1] = ML.LEVELS[(i + 2 * h + b) % 4]
    pr = Problem(2, 2, L, D, dtype, mask, seed=300 + L + D, ref_tail=ref_tail)
    pr.default = _default(pr)
    return pr


@pytest.mark.parametrize("sel", ["default", "dq_round3"])
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)], ids=["64-bf16", "128-f16"])
@pytest.mark.parametrize("ref_tail", [True, False])
@pytest.mark.parametrize("L", [100, 129, 448, 449, 513])
def test_tails_and_fold_at_odd_lengths(L, ref_tail, D, dtype, sel):
    """L = 100 (one block), 129 (a one-row tail block), 448 = 3*128 + 64 (the
    (nbk-1)*kBlk + kT >= Lk boundary of the `ntm -= 1` rule), 449 (one past it and odd: the last
    level-2 pair is half replicate padding), 513 (a one-row tail block behind four full ones)."""
    pr = _case_c(L, ref_tail, D, dtype)
    grads = pr.run_sel(sel, pr.default)
    _check(f"c L={L} ref_tail={ref_tail} D={D} {sel}", dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# d. more than 64 blocks
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_d(D):
    """L = 65*128 + 17 = 8337 (66 blocks): the ballot loops that build the q-lists and key lists
    take a second pass. ~70 % skips, key column 8 at level 8 and key column 3 at level 1 in EVERY
    q-block (q-lists of 66 entries), q-block 40 keeping every key block at levels 8, 4, 2, 1 in
    turn (a key list of 66 entries, n8 = 17: a partial last level-8 tile)."""
    nb = 66
    mask = _random_levels(1, 1, nb, seed=8337 + D, p=(0.075, 0.075, 0.075, 0.075, 0.7))
    mask[0, 0, 40, :] = torch.tensor([8, 4, 2, 1], dtype=torch.int32).repeat(17)[:nb]
    mask[0, 0, :, 8] = 8
    mask[0, 0, :, 3] = 1
    assert int((mask[0, 0, 40] == 8).sum()) == 17 and bool((mask[0, 0, 40] > 0).all())
    pr = Problem(1, 1, 8337, D, torch.bfloat16, mask, seed=400 + D)
    pr.default = _default(pr)
    return pr


@pytest.mark.parametrize("sel", SELS)
@pytest.mark.parametrize("D", [64, 128])
def test_more_than_64_blocks(D, sel):
    pr = _case_d(D)
    grads = pr.run_sel(sel, pr.default)
    _check(f"d D={D} {sel}", pr.dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# e. arguments the module never sets
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_e(D):
    """L=700, B=2, H=3, scale 0.2, q/out/dout as [B,L,H,D] storage viewed [B,H,L,D] with no row table
    (the kernels address the caller's strides directly), one mask per sample expanded over the heads
    (head stride 0)."""
    mask = _random_levels(2, 1, 6, seed=700 + D)
    pr = Problem(2, 3, 700, D, torch.bfloat16, mask, seed=500 + D, perm=False, scale=0.2, strided=True)
    assert pr.md.stride(1) == 0 and not pr.q.is_contiguous() and not pr.do.is_contiguous()
    ran, ws = [], []
    pr.default = pr.backward(0, ran, ws)
    assert ran == [_ran("default")]
    assert ws == [ml_workspace_bytes(2, 3, 700, D, False)]
    return pr


@pytest.mark.parametrize("sel", SELS)
@pytest.mark.parametrize("D", [64, 128])
def test_scale_strides_and_broadcast_mask(D, sel):
    """scale, strided q/out/dout, a head-broadcast mask, and dq/dk/dv written into strided buffers of
    the caller ([B,L,H,D] storage): the same bits as the contiguous results, at the bounds."""
    pr = _case_e(D)
    grads = pr.run_sel(sel, pr.default)
    B, H, L = 2, 3, 700
    bufs = tuple(torch.full((B, L, H, D), float("nan"), device=DEV, dtype=pr.dtype).transpose(1, 2) for _ in range(3))
    got = pr.backward(_sel(sel), grads=bufs)
    for a, b, c in zip(got, bufs, grads):
        assert a is b and not a.is_contiguous() and c.is_contiguous() and torch.equal(a, c)
    _check(f"e D={D} {sel}", pr.dtype, pr.reordered(got), pr.ref, pr.emu)


@pytest.mark.parametrize("D", [64, 128])
def test_heavy_rows_hint_and_batch_independence(D):
    """heavy_rows only orders the dQ workgroups (0, the default 2, and 50 > nbq): identical bits. Each
    sample of the B=2 call equals, bit for bit, the same sample run alone."""
    pr = _case_e(D)
    for hr in (0, 50):
        for a, b in zip(pr.backward(heavy_rows=hr), pr.default):
            assert torch.equal(a, b), hr
    for s in range(2):
        for a, b in zip(pr.backward(sample=s), pr.default):
            assert torch.equal(a[0], b[s]), s


# ----------------------------------------------------------------------------------------------
# f. the module's autograd path
# ----------------------------------------------------------------------------------------------
def test_module_autograd_matches_oracle():
    """AdaptiveBlockSparseAttnTrain under autograd (Gilbert row table inside the op, the predictor's
    own level mask, a non-contiguous dO): q.grad / k.grad / v.grad at the bounds, against the oracle
    on the statistics the op's forward saved (recomputed here: the same launch, the same bits)."""
    from vblade import multilevel
    w, h, d, text = 14, 10, 6, 26
    B, H, D, dtype = 1, 2, 64, torch.bfloat16
    L = w * h * d + text
    mod = multilevel.AdaptiveBlockSparseAttnTrain(width=w, height=h, depth=d, text_length=text, log_every=0).to(DEV)
    q, k, v = (_rand(B, H, L, D, seed=s).to(DEV).requires_grad_() for s in (600, 601, 602))
    do = _rand(B, L, H, D, seed=603).to(DEV).transpose(1, 2)
    torch.cuda.manual_seed(7)
    out = mod(q, k, v)
    out.backward(do)
    rows = mod.gilbert_rearranger.rows
    mask = mod.last_mask
    assert rows.numel() == L and tuple(mask.shape) == (B, H, 7, 7)
    with torch.no_grad():
        kp, vp = _ops().kv_pyramid(k, v, rows)
        out2, lse = _ops().ml_attention_fwd(q, kp, vp, mask, q_rows=rows, want_lse=True)
    assert torch.equal(out2, out.detach())
    P = rows.long().cpu()
    r = lambda t: t.detach().cpu()[:, :, P]  # noqa: E731
    args = (r(q), r(k), r(v), mask.cpu().to(torch.int32), r(out), r(lse), r(do))
    ref = ML.multilevel_attention_bwd_lse(*args, store_dtype=dtype)
    emu = ML.multilevel_attention_bwd_lse(*args, store_dtype=dtype, emulate_rounding=True)
    _check("f module autograd", dtype, (r(q.grad), r(k.grad), r(v.grad)), ref, emu)
