"""Op-level parity of vb_attn_bwd_joint (ops.attention_bwd_joint): the exact gradient of the one softmax
over the kept full-resolution keys and the biased pooled keys, against the substituted two-branch oracle
of tests/joint_ref.py (fp64; tests/test_joint_ref.py shows it is the autograd gradient of the function).

Forward statistics (out, lse) come from ops.attention_fwd(kp=, vp=, kp_log_bias=, need_lse=True) on the
device, kp/vp and the reordered k/v from ops.pool_kv; the row permutations are random, as in
test_gpu_backward_branches.py, whose bounds these are:
  * per row: per_row_error(g, ref) <= O.per_row_bound(emu, ref, dtype) = 2 x the worst row of the
    oracle's storage-rounding emulation, computed on the CPU each run, never from the kernels, and
    asserted <= 1e-2 (bf16) / 1.5e-3 (f16) by per_row_bound itself;
  * whole tensor: relative Frobenius error <= 4e-3 (bf16) / 6e-4 (f16).
Each case records its worst rows through conftest.record.
"""
import functools

import pytest
import torch

import bsa_oracle as O
import joint_ref as J
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = {torch.bfloat16: 4e-3, torch.float16: 6e-4}
NAMES = ("dq", "dk", "dv")


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _ops():
    from vblade import ops
    return ops


def _bits():
    from vblade import _lib
    return _lib


def _rand(*shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _perm(L, seed):
    return torch.randperm(L, generator=torch.Generator().manual_seed(seed))


def _sel(name):
    lib = _bits()
    return {"default": 0, "dkdv_round3": lib.VB_BWD_SEL_DKDV_ROUND3, "dq_round3": lib.VB_BWD_SEL_DQ_ROUND3}[name]


def _ran(name):
    lib = _bits()
    return {"default": lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_PIPE_RING2,
            "dkdv_round3": lib.VB_BWD_RAN_DKDV_ROUND3 | lib.VB_BWD_RAN_DQ_PIPE_RING2,
            "dq_round3": lib.VB_BWD_RAN_DKDV_PIPE | lib.VB_BWD_RAN_DQ_ROUND3}[name]


def log_gap(gap, dtype):
    """ln(gap) rounded as the module rounds it (AdaptiveBlockSparseAttn._log_gap)."""
    return float(torch.log(torch.tensor(float(gap), dtype=dtype)).item())


def _check(label, dtype, grads, ref, emu):
    """grads, ref, emu: (dq, dk, dv) in the same row order. Both bounds of the module docstring."""
    rows, facts = [], []
    for name, g, r, e in zip(NAMES, grads, ref, emu):
        g = g.float().cpu()
        assert torch.isfinite(g).all(), (label, name)
        bound = O.per_row_bound(e, r, dtype)
        worst, where = O.per_row_error(g, r)
        rows.append((name, worst, where, bound, J.rel(g, r)))
        facts.append(f"{name} {worst:.2e}/{bound / 2:.2e}")
    print(label, rows)
    record("joint backward worst-row error, gpu/emulation (bound: 2x emulation)", f"{label}: " + " ".join(facts))
    for name, worst, where, bound, whole in rows:
        assert worst <= bound, (label, name, worst, where, bound)
        assert whole <= TIGHT[dtype], (label, name, whole)


class Joint:
    """One joint problem: inputs in the caller's row order, the device forward's out and LSE, and the
    fp64 reference / emulation in REORDERED order. ``blhd``: q/k/v/dO are [B,L,H,D] storage viewed
    [B,H,L,D], addressed through their strides."""

    def __init__(self, B, H, Lq, Lk, D, dtype, gap, density, seed, scale=None, edit_mask=None, blhd=False):
        ops = _ops()
        self.dtype, self.gap, self.scale, self.B = dtype, gap, scale, B
        self.beta = log_gap(gap, dtype)
        self.Pq, self.Pk = _perm(Lq, seed + 10), _perm(Lk, seed + 11)
        if Lq == Lk:
            self.Pk = self.Pq

        def make(L, s):
            if blhd:
                return _rand(B, L, H, D, dtype=dtype, seed=s).to(DEV).transpose(1, 2)
            return _rand(B, H, L, D, dtype=dtype, seed=s).to(DEV)

        self.q, self.do = make(Lq, seed), make(Lq, seed + 3)
        self.k, self.v = make(Lk, seed + 1), make(Lk, seed + 2)
        assert blhd != self.q.is_contiguous()
        self.mask = O.block_mask_from_density(B, H, (Lq + 127) // 128, (Lk + 127) // 128, density, seed=seed + 4)
        if edit_mask is not None:
            edit_mask(self.mask)
        self.mask_dev = self.mask.to(DEV)
        self.q_rows, self.kv_rows = self.Pq.int().to(DEV), self.Pk.int().to(DEV)
        self.kp, self.vp, self.k_r, self.v_r = ops.pool_kv(self.k, self.v, gap, self.kv_rows, reordered=True)
        self.out, self.lse = ops.attention_fwd(self.q, self.k_r, self.v_r, block_mask=self.mask_dev,
                                               q_rows=self.q_rows, kp=self.kp, vp=self.vp,
                                               kp_log_bias=self.beta, need_lse=True, scale=scale)
        c = lambda t: t.cpu()  # noqa: E731
        args = (c(self.q)[:, :, self.Pq], c(self.k)[:, :, self.Pk], c(self.v)[:, :, self.Pk], c(self.kp), c(self.vp),
                c(self.out)[:, :, self.Pq], c(self.lse)[:, :, self.Pq], c(self.do)[:, :, self.Pq], self.mask, gap,
                self.beta)
        assert torch.equal(c(self.k_r), args[1])             # pool_kv's reordered copy is the gather
        kw = dict(sm_scale=scale, store_dtype=dtype)
        self.ref = J.joint_oracle_bwd(*args, **kw)
        self.emu = J.joint_oracle_bwd(*args, **kw, emulate_rounding=True)

    def backward(self, sel=0, ran=None, b=None):
        """The whole batch, or sample ``b`` alone (a B=1 call on views of the same tensors)."""
        s = slice(None) if b is None else slice(b, b + 1)
        return _ops().attention_bwd_joint(self.do[s], self.q[s], self.k_r[s], self.v_r[s], self.out[s], self.lse[s],
                                          block_mask=self.mask_dev[s], q_rows=self.q_rows, kv_rows=self.kv_rows,
                                          kp=self.kp[s], vp=self.vp[s], gap=self.gap, kp_log_bias=self.beta,
                                          scale=self.scale, heavy_rows=2, kernel_select=sel, kernels_ran=ran)

    def reordered(self, grads):
        dq, dk, dv = (g.float().cpu() for g in grads)
        return dq[:, :, self.Pq], dk[:, :, self.Pk], dv[:, :, self.Pk]


# ----------------------------------------------------------------------------------------------
# A. main case
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_a(D, dtype):
    """B=2, H=3, L=1000, gap 7: Lkp = 143 (two pooled key blocks, the second partial; 143*7 = 1001: one
    replicate-padded source row), random row permutation. With the default kernels' run."""
    pr = Joint(2, 3, 1000, 1000, D, dtype, gap=7, density=0.3, seed=100 + D)
    assert pr.kp.shape[2] == 143
    ran = []
    pr.default = pr.backward(0, ran)
    assert ran == [_ran("default")]
    return pr


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("D", [64, 128])
def test_joint_backward_at_the_per_row_bound(D, dtype):
    pr = _case_a(D, dtype)
    assert torch.isfinite(pr.lse).all()
    _check(f"A D={D} {dtype} default", dtype, pr.reordered(pr.default), pr.ref, pr.emu)


@pytest.mark.parametrize("D,dtype,sel", [(64, torch.bfloat16, "dkdv_round3"), (128, torch.float16, "dq_round3")],
                         ids=["64-bf16-dkdv_round3", "128-f16-dq_round3"])
def test_joint_statistics_feed_the_round3_kernels(D, dtype, sel):
    """bwd_dkdv_kernel and bwd_dq_kernel read the same statistics: each launch asserted from kernels_ran,
    each result at the bounds; the gradients a selection does not touch are the default's bits."""
    pr = _case_a(D, dtype)
    ran = []
    grads = pr.backward(_sel(sel), ran)
    assert ran == [_ran(sel)]
    if sel == "dkdv_round3":
        assert torch.equal(grads[0], pr.default[0])
    else:
        assert torch.equal(grads[1], pr.default[1]) and torch.equal(grads[2], pr.default[2])
    _check(f"A D={D} {dtype} {sel}", dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# B. edges
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
def test_cleared_and_full_mask_rows(D):
    """Head 1's q-block 2 keeps no key block: its queries see the pooled keys only, yet their LSE is
    finite and their dq live. Head 0's q-block 5 keeps every block. Key block 6 is kept by no row of
    head 1: its dk/dv are the pooled fold alone, and nonzero."""
    dtype = torch.bfloat16

    def edit(m):
        m[:, 1, 2, :] = False
        m[:, 0, 5, :] = True
        m[:, 1, :, 6] = False

    pr = Joint(1, 2, 1000, 1000, D, dtype, gap=7, density=0.3, seed=300 + D, edit_mask=edit)
    assert not pr.mask[0, 1, 2].any() and pr.mask[0, 0, 5].all() and not pr.mask[0, 1, :, 6].any()
    assert torch.isfinite(pr.lse).all()
    grads = pr.backward()
    _check(f"B cleared/full D={D}", dtype, pr.reordered(grads), pr.ref, pr.emu)
    dq, dk, dv = pr.reordered(grads)
    assert (dq[0, 1, 256:384].abs().amax(-1) > 0).all()
    assert (dk[0, 1, 768:896].abs().amax(-1) > 0).all() and (dv[0, 1, 768:896].abs().amax(-1) > 0).all()


def test_gap_4_with_160_pooled_keys():
    """L=640, gap 4: Lkp = 160, no padded row, the second pooled key block a quarter full."""
    pr = Joint(1, 1, 640, 640, 64, torch.bfloat16, gap=4, density=0.3, seed=400)
    assert pr.kp.shape[2] == 160
    _check("B L=640 gap=4", pr.dtype, pr.reordered(pr.backward()), pr.ref, pr.emu)


def test_rectangular_scaled_strided():
    """Lq=300 against Lk=700, gap 15 (Lkp = 47, five replicate-padded rows), scale 0.2, q/k/v/dO as
    [B,L,H,D] storage, separate row permutations for queries and keys: the entry takes vb_attn_bwd's
    struct, so the same liberties apply."""
    pr = Joint(2, 3, 300, 700, 64, torch.bfloat16, gap=15, density=0.4, seed=500, scale=0.2, blhd=True)
    assert pr.kp.shape[2] == 47 and not torch.equal(pr.Pq, pr.Pk[:300])
    ran = []
    grads = pr.backward(0, ran)
    assert ran == [_ran("default")]
    assert grads[0].shape[2] == 300 and grads[1].shape[2] == 700
    _check("B 300x700 scale 0.2 blhd", pr.dtype, pr.reordered(grads), pr.ref, pr.emu)


# ----------------------------------------------------------------------------------------------
# C. determinism
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", [(64, torch.bfloat16), (128, torch.float16)], ids=["64-bf16", "128-f16"])
def test_bit_reproducible_and_batch_invariant(D, dtype):
    """Two calls give equal bits, and each sample of the B=2 call equals its own B=1 call (the pooled-key
    split never depends on B)."""
    pr = _case_a(D, dtype)
    again = pr.backward()
    for name, a, b in zip(NAMES, pr.default, again):
        assert torch.equal(a, b), name
    for s in range(pr.B):
        alone = pr.backward(b=s)
        for name, a, b in zip(NAMES, pr.default, alone):
            assert torch.equal(a[s:s + 1], b), (name, s)
