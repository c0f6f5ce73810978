"""CPU checks of the backward reference itself (oracle/bsa_oracle.py): two_branch_attention_bwd, its
storage-rounding emulation and the per-row error metric that tests/test_gpu_backward_branches.py
derives its bounds from. No GPU: the forward statistics come from the oracle's own forward."""
import math

import pytest
import torch

import bsa_oracle as O


def _rand(*shape, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def rel(x, ref):
    ref = ref.double()
    return ((x.double() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def _two_branch_problem(B, H, Lq, Lk, D, gap, dtype, density, seed, sm_scale=None):
    """Inputs of vb_attn_bwd's two-branch form with the oracle's forward statistics, the branch
    outputs stored in ``dtype`` as the kernels read them, and a random constant alpha in (0,1)."""
    q, do = _rand(B, H, Lq, D, dtype=dtype, seed=seed), _rand(B, H, Lq, D, dtype=dtype, seed=seed + 3)
    k, v = _rand(B, H, Lk, D, dtype=dtype, seed=seed + 1), _rand(B, H, Lk, D, dtype=dtype, seed=seed + 2)
    mask = O.block_mask_from_density(B, H, (Lq + 127) // 128, (Lk + 127) // 128, density, seed=seed + 4)
    kp, vp = O.simple_pooling(k, gap), O.simple_pooling(v, gap)
    out1, lse1 = O.block_sparse_attention(q, k, v, mask, sm_scale=sm_scale)
    out2, lse2 = O.block_sparse_attention(q, kp, vp, None, sm_scale=sm_scale)
    alpha = torch.rand(B, H, Lq, generator=torch.Generator().manual_seed(seed + 5)) * 0.98 + 0.01
    return dict(q_r=q, k_r=k, v_r=v, kp=kp, vp=vp, out1=out1.to(dtype), lse1=lse1, out2=out2.to(dtype),
                lse2=lse2, alpha=alpha, dout=do, mask=mask, gap=gap, sm_scale=sm_scale, store_dtype=dtype)


def test_two_branch_bwd_equals_autograd_of_the_fp64_forward():
    """The unrounded reference against torch.autograd on an fp64 restatement of the two-branch forward
    (alpha a constant, so neither LSE enters the graph): rectangular Lq != Lk, three replicate-padded
    pool rows (29 * 7 = 203 > 200), a non-default scale, a sparse mask. Independent of
    adaptive_attention_bwd and of block_sparse_attention_bwd."""
    B, H, Lq, Lk, D, gap, scale = 1, 2, 150, 200, 16, 7, 0.3
    g = torch.Generator().manual_seed(11)
    q = torch.randn(B, H, Lq, D, generator=g, dtype=torch.float64, requires_grad=True)
    k = torch.randn(B, H, Lk, D, generator=g, dtype=torch.float64, requires_grad=True)
    v = torch.randn(B, H, Lk, D, generator=g, dtype=torch.float64, requires_grad=True)
    do = torch.randn(B, H, Lq, D, generator=g, dtype=torch.float64)
    alpha = torch.rand(B, H, Lq, generator=g)
    mask = torch.tensor([[[[1, 0], [1, 1]], [[0, 1], [1, 0]]]], dtype=torch.bool)
    keep = mask.repeat_interleave(128, 2)[:, :, :Lq].repeat_interleave(128, 3)[..., :Lk]

    def pool(x):
        return O.pad_replicate(x, gap).reshape(B, H, -1, gap, D).mean(-2)

    s1 = (q @ k.transpose(-1, -2) * scale).masked_fill(~keep, float("-inf"))
    out1, lse1 = torch.softmax(s1, -1) @ v, torch.logsumexp(s1, -1)
    kp, vp = pool(k), pool(v)
    s2 = q @ kp.transpose(-1, -2) * scale
    out2, lse2 = torch.softmax(s2, -1) @ vp, torch.logsumexp(s2, -1)
    w2 = O.rnd(1.0 - alpha, torch.bfloat16)
    out = alpha[..., None].double() * out1 + w2[..., None].double() * out2
    out.backward(do)
    got = O.two_branch_attention_bwd(q.detach(), k.detach(), v.detach(), kp.detach(), vp.detach(),
                                     out1.detach(), lse1.detach(), out2.detach(), lse2.detach(), alpha, do,
                                     mask, gap, sm_scale=scale, store_dtype=torch.bfloat16)
    assert kp.shape[2] * gap - Lk == 3
    for name, a, r in zip(("dq", "dk", "dv"), got, (q.grad, k.grad, v.grad)):
        assert rel(a, r) <= 1e-6, (name, rel(a, r))
        assert O.per_row_error(a, r)[0] <= 1e-6, name


def test_two_branch_bwd_equals_adaptive_attention_bwd_at_the_identity_permutation():
    """With no Gilbert reorder the op-level reference is the module-level adaptive_attention_bwd on
    the module's own alpha. store_dtype fp32: that oracle uses the unrounded 1 - alpha."""
    B, H, L, D, gap = 1, 2, 300, 32, 7
    q, k, v, do = (_rand(B, H, L, D, seed=50 + s) for s in range(4))
    cfg = O.AdaptiveConfig.cogvideox(sample_gap=gap, use_rearrange=False)
    mask = O.block_mask_from_density(B, H, 3, 3, 0.5, seed=5)
    fwd = O.adaptive_attention(q, k, v, cfg, None, None, mask=mask)
    want = O.adaptive_attention_bwd(q, k, v, do, cfg, fwd)
    got = O.two_branch_attention_bwd(q, k, v, fwd["kp"], fwd["vp"], fwd["out1"], fwd["lse1"], fwd["out2"],
                                     fwd["lse2"], fwd["alpha"][..., 0], do, mask, gap,
                                     store_dtype=torch.float32)
    for name, a, r in zip(("dq", "dk", "dv"), got, want):
        assert rel(a, r) <= 1e-6, (name, rel(a, r))


# the GPU floor recorded in test_gpu_backward.py::test_default_backward_kernels_at_the_rounding_floor
MEASURED_FLOOR = {torch.bfloat16: (2.3e-3, 2.4e-3), torch.float16: (2.9e-4, 3.0e-4)}


@pytest.mark.parametrize("L,D,dtype,density", [(300, 64, torch.bfloat16, 0.5), (1000, 128, torch.bfloat16, 0.25),
                                               (517, 64, torch.float16, 0.3)])
def test_rounding_emulation_reproduces_the_measured_gpu_floor(L, D, dtype, density):
    """The emulation (w*P, dS and the results rounded to the storage dtype, everything else fp64) on
    the floor test's own inputs gives the whole-tensor error the default kernels were measured at on
    the GPU, within +-20 %: the per-row bounds derived from it cannot drift loose."""
    q, k, v, do = (_rand(1, 2, L, D, dtype=dtype, seed=s) for s in range(4))
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(1, 2, nb, nb, density, seed=7)
    out, lse = O.block_sparse_attention(q, k, v, mask)
    args = (q, k, v, None, None, out.to(dtype), lse, None, None, None, do, mask, 0)
    ref = O.two_branch_attention_bwd(*args, store_dtype=dtype)
    emu = O.two_branch_attention_bwd(*args, store_dtype=dtype, emulate_rounding=True)
    lo, hi = MEASURED_FLOOR[dtype]
    for name, e, r in zip(("dq", "dk", "dv"), emu, ref):
        err = rel(e, r)
        print(f"{name} L={L} D={D} {dtype}: emulated whole-tensor {err:.3e}, worst row {O.per_row_error(e, r)[0]:.3e}")
        assert 0.8 * lo <= err <= 1.2 * hi, (name, err)
    # and the unrounded main-branch form is block_sparse_attention_bwd
    for a, r in zip(ref, O.block_sparse_attention_bwd(q, k, v, out.to(dtype), lse, do, mask)):
        assert rel(a, r) <= 1e-6


def test_per_row_metric_sees_a_dropped_replicate_fold_the_whole_tensor_bound_misses():
    """L=1000, gap=7: 143 pooled rows, the last holding one replicate-padded copy of key 999. A
    reference without the fold of that copy (dk/dv of key 999 lose half their pooled share) passes
    the old whole-tensor 2e-2 check and fails the per-row bound: 2x the emulation's worst row, which
    itself stays under the 1e-2 cap."""
    pr = _two_branch_problem(1, 2, 1000, 1000, 64, 7, torch.bfloat16, 0.3, seed=60)
    ref = O.two_branch_attention_bwd(**pr)
    emu = O.two_branch_attention_bwd(**pr, emulate_rounding=True)
    bad = O.two_branch_attention_bwd(**pr, replicate_fold=False)
    assert torch.equal(bad[0], ref[0])
    for name, b, e, r in zip(("dk", "dv"), bad[1:], emu[1:], ref[1:]):
        bound = 2 * O.per_row_error(e, r)[0]
        worst, where = O.per_row_error(b, r)
        print(f"{name}: dropped fold whole-tensor {rel(b, r):.2e}, worst row {worst:.2e} at {where}, bound {bound:.2e}")
        assert bound <= 1e-2
        assert rel(b, r) <= 2e-2
        assert worst > 1e-2 and where[2] == 999
        assert O.per_row_error(b[:, :, :999], r[:, :, :999])[0] == 0


def test_dead_rows_contribute_nothing():
    """lse = -inf (the native forward's empty row), +inf (the FlashAttention-2 convention) and
    alpha = 0 / 1 all switch a branch off for that row without producing a NaN."""
    pr = _two_branch_problem(1, 1, 256, 256, 32, 15, torch.bfloat16, 1.0, seed=70)
    pr["lse1"][0, 0, :5] = float("-inf")
    pr["lse1"][0, 0, 5:10] = float("inf")
    pr["alpha"][0, 0, :10] = 1.0          # pooled weight 0 too: rows 0..9 are dead in both branches
    pr["alpha"][0, 0, 10:20] = 0.0
    for emulate in (False, True):
        dq, dk, dv = O.two_branch_attention_bwd(**pr, emulate_rounding=emulate)
        assert all(torch.isfinite(t).all() for t in (dq, dk, dv))
        assert dq[0, 0, :10].abs().max() == 0
        assert (dq[0, 0, 10:].abs().amax(-1) > 0).all()
    assert math.isinf(pr["lse1"][0, 0, 0].item())
