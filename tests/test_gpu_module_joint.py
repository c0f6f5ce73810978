"""GPU: AdaptiveBlockSparseAttn(grad_combine="joint") — the inference call under autograd.

The output under grad is, bit for bit, ops.attention_fwd on the module's own mask (kept keys and the
biased pooled keys in one softmax, LSE stored); the gradients, in the caller's row order, meet the
per-row bound of test_gpu_backward_joint.py against the substituted oracle of tests/joint_ref.py with
that mask; overlap, a given block_mask= and torch.utils.checkpoint change no bit. The default module
("reference") still is autograd.adaptive_split_attention, bit for bit. One LoRA step through a stand-in
block gives the gradients of the same step with a torch statement of the joint function as attention.
"""
import functools

import pytest
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

import bsa_oracle as O
import joint_ref as J
from conftest import record

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIGHT = {torch.bfloat16: 4e-3, torch.float16: 6e-4}
GEOM = {"cog": dict(width=12, height=8, depth=6, text_length=26),    # L = 602, D = 64, forced tail
        "wan": dict(width=13, height=6, depth=7)}                    # L = 546, D = 128
HEAD = {"cog": (64, torch.bfloat16), "wan": (128, torch.float16)}
GAP = 4                                                              # 151 / 137 pooled keys: two blocks
B, H = 2, 2


@pytest.fixture(scope="module", autouse=True)
def _lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import vblade
    vblade.load_library()


def _module(variant, **kw):
    import vblade
    return vblade.AdaptiveBlockSparseAttn(variant, sample_gap=GAP, min_retain_ratio=0.2, max_retain_ratio=0.5,
                                          log_every=0, **GEOM[variant], **kw).to(DEV)


def _run(m, pr, wrap=None, **fw):
    """One forward and backward of module ``m`` on the problem's inputs -> (out, (dq, dk, dv))."""
    q, k, v = (t.clone().requires_grad_(True) for t in (pr.q, pr.k, pr.v))
    call = lambda a, b, c: m(a, b, c, **fw)  # noqa: E731
    out = call(q, k, v) if wrap is None else wrap(call, q, k, v)
    out.backward(pr.do)
    return out.detach(), (q.grad, k.grad, v.grad)


class Problem:
    pass


@functools.lru_cache(maxsize=None)
def _case(variant):
    D, dtype = HEAD[variant]
    pr = Problem()
    pr.variant, pr.dtype = variant, dtype
    pr.m = _module(variant, grad_combine="joint")
    L = pr.m.gilbert_rearranger.seq_len
    assert L == {"cog": 602, "wan": 546}[variant]
    g = torch.Generator().manual_seed(40 + D)
    pr.q, pr.k, pr.v, pr.do = (torch.randn(B, H, L, D, generator=g).to(dtype).to(DEV) for _ in range(4))
    off = lambda: torch.stack([torch.randperm(128, generator=g)[:32] for _ in range(B * H)]).view(B, H, 32).int().to(DEV)  # noqa: E731
    pr.off = dict(q_off=off(), k_off=off())
    pr.out, pr.grads = _run(pr.m, pr, **pr.off)
    pr.mask = pr.m.last_mask.clone()
    pr.rows = pr.m.gilbert_rearranger.rows
    assert pr.rows.device.type == "cuda" and pr.rows.dtype == torch.int32
    return pr


def _same(a, b):
    assert torch.equal(a[0], b[0]), "out"
    for n, x, y in zip(("dq", "dk", "dv"), a[1], b[1]):
        assert torch.equal(x, y), n


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_output_under_grad_is_the_inference_launch(variant):
    from vblade import ops
    pr = _case(variant)
    m = pr.m
    kp, vp, k_r, v_r = ops.pool_kv(pr.k, pr.v, GAP, pr.rows, reordered=True)
    assert kp.shape[2] > 128
    want, lse = ops.attention_fwd(pr.q, k_r, v_r, block_mask=pr.mask, q_rows=pr.rows, kp=kp, vp=vp,
                                  kp_log_bias=m._log_gap(pr.dtype), need_lse=True, heavy_rows=m.force_tail)
    assert torch.isfinite(lse).all()
    assert torch.equal(pr.out, want)
    calls = m.sparsity_counter
    with torch.no_grad():
        inf = m(pr.q, pr.k, pr.v, **pr.off)
    assert torch.equal(m.last_mask, pr.mask) and m.sparsity_counter == calls + 1
    diff = (pr.out.float() - inf.float()).abs().max().item()
    print(variant, "under grad vs no_grad, max abs", diff)
    assert diff <= 2.5e-2


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_gradients_meet_the_per_row_bound_against_the_oracle(variant):
    from vblade import ops
    pr = _case(variant)
    m = pr.m
    P = pr.rows.long().cpu()
    kp, vp, k_r, v_r = ops.pool_kv(pr.k, pr.v, GAP, pr.rows, reordered=True)
    beta = m._log_gap(pr.dtype)
    _, lse = ops.attention_fwd(pr.q, k_r, v_r, block_mask=pr.mask, q_rows=pr.rows, kp=kp, vp=vp,
                               kp_log_bias=beta, need_lse=True, heavy_rows=m.force_tail)
    c = lambda t: t.cpu()[:, :, P]  # noqa: E731
    args = (c(pr.q), c(pr.k), c(pr.v), kp.cpu(), vp.cpu(), c(pr.out), c(lse), c(pr.do), pr.mask.cpu().bool(), GAP, beta)
    ref = J.joint_oracle_bwd(*args, store_dtype=pr.dtype)
    emu = J.joint_oracle_bwd(*args, store_dtype=pr.dtype, emulate_rounding=True)
    facts = []
    for name, g, r, e in zip(("dq", "dk", "dv"), pr.grads, ref, emu):
        g = c(g.float())
        assert torch.isfinite(g).all(), name
        bound = O.per_row_bound(e, r, pr.dtype)
        worst, where = O.per_row_error(g, r)
        whole = J.rel(g, r)
        facts.append(f"{name} {worst:.2e}/{bound / 2:.2e}")
        print(variant, name, worst, where, bound, whole)
        assert worst <= bound, (name, worst, where, bound)
        assert whole <= TIGHT[pr.dtype], (name, whole)
    record("joint module worst-row error, gpu/emulation (bound: 2x emulation)", f"{variant}: " + " ".join(facts))


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_overlap_given_mask_and_checkpoint_change_no_bit(variant):
    pr = _case(variant)
    base = (pr.out, pr.grads)
    # the pooled pass as its own launch instead of inside the predictor's
    _same(_run(_module(variant, grad_combine="joint", overlap=False), pr, **pr.off), base)
    # the predicted mask passed back in
    _same(_run(pr.m, pr, block_mask=pr.mask), base)
    # recomputed forward
    ck = lambda call, q, k, v: checkpoint(call, q, k, v, use_reentrant=False)  # noqa: E731
    _same(_run(pr.m, pr, wrap=ck, **pr.off), base)


def test_shared_head0_reads_head_0s_mask_on_the_joint_path():
    from vblade import ops
    pr = _case("cog")
    m = _module("cog", grad_combine="joint", mask_head_mode="shared_head0")
    out, grads = _run(m, pr, **pr.off)
    assert torch.equal(m.last_mask, pr.mask)
    shared = pr.mask[:, :1].expand(-1, H, -1, -1)
    kp, vp, k_r, v_r = ops.pool_kv(pr.k, pr.v, GAP, pr.rows, reordered=True)
    want = ops.attention_fwd(pr.q, k_r, v_r, block_mask=shared, q_rows=pr.rows, kp=kp, vp=vp,
                             kp_log_bias=m._log_gap(pr.dtype), need_lse=True, heavy_rows=m.force_tail)[0]
    assert torch.equal(out, want)
    assert all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("variant", ["cog", "wan"])
def test_default_module_is_the_two_branch_form(variant):
    """grad_combine defaults to "reference": under grad the module returns the output and gradients of
    autograd.adaptive_split_attention on the same mask, bit for bit."""
    from vblade import autograd
    pr = _case(variant)
    m = _module(variant)
    assert m.grad_combine == "reference"
    got = _run(m, pr, **pr.off)
    assert torch.equal(m.last_mask, pr.mask)

    def split(q, k, v):
        return autograd.adaptive_split_attention(q, k, v, pr.mask, pr.rows, GAP, heavy_rows=m.force_tail)

    _same(got, _run(split, pr))
    # and it is not the joint gradient: the option changes dq
    assert not torch.equal(got[1][0], pr.grads[0])


# ----------------------------------------------------------------------------------------------
# one LoRA step
# ----------------------------------------------------------------------------------------------
class TorchJointAttention(nn.Module):
    """A torch statement of the joint function as attention: joint_ref.joint_forward in fp64 on the CPU,
    in the caller's row order, differentiated by torch autograd (the pooled keys rounded to the storage
    dtype as the device stores them, straight through)."""

    def __init__(self, mask, rows, gap, beta):
        super().__init__()
        self.mask, self.rows, self.gap, self.beta = mask.cpu().bool(), rows.long().cpu(), gap, beta

    def forward(self, q, k, v):
        qc, kc, vc = (t.double().cpu()[:, :, self.rows] for t in (q, k, v))
        st = lambda t: t + (t.to(q.dtype).double() - t).detach()  # noqa: E731
        pooled = (st(J.mean_pool(kc, self.gap)), st(J.mean_pool(vc, self.gap)))
        out, _ = J.joint_forward(qc, kc, vc, self.mask, self.gap, self.beta, pooled=pooled)
        inv = torch.empty_like(self.rows)
        inv[self.rows] = torch.arange(self.rows.numel())
        return out[:, :, inv].to(q.dtype).to(q.device)


class FixedMaskJoint(nn.Module):
    def __init__(self, mask):
        super().__init__()
        self.m = _module("cog", grad_combine="joint")
        self.mask = mask

    def forward(self, q, k, v):
        return self.m(q, k, v, block_mask=self.mask)


def test_lora_step_through_the_joint_module_matches_the_torch_statement():
    """test_gpu_train.py's LoRA-gradient check (one layer, hidden 128, 2 heads, pinned mask, tolerance
    3e-2 per LoRA tensor) with the joint module against the torch statement of the joint function."""
    from vblade import train as T
    heads, hidden, rank = 2, 128, 8
    L = 12 * 8 * 6 + 26
    nb = (L + 127) // 128
    g = torch.Generator().manual_seed(5)
    mask = torch.rand(1, heads, nb, nb, generator=g) < 0.5
    mask[..., -2:] = True
    mask[..., -2:, :] = True
    mask = mask.to(torch.uint8).to(DEV)
    fixed = FixedMaskJoint(mask)
    torch_attn = TorchJointAttention(mask, fixed.m.gilbert_rearranger.rows, GAP, fixed.m._log_gap(torch.bfloat16))
    g = torch.Generator().manual_seed(6)
    x = torch.randn(1, L, hidden, generator=g).bfloat16().to(DEV)
    y = torch.randn(1, L, hidden, generator=g).bfloat16().to(DEV)
    grads = []
    for attn in (fixed, torch_attn):
        mdl = T.StandInTransformer(1, hidden, heads, rank, float(rank), attn, dtype=torch.bfloat16, device=DEV, seed=0)
        gb = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for n, p in mdl.named_parameters():
                if n.endswith("lora_B"):
                    p.copy_((torch.randn(p.shape, generator=gb) * 0.05).to(DEV))
        T.pseudo_huber(mdl(x), y, 1e-3).backward()
        grads.append([p.grad.float().cpu() for p in mdl.lora_parameters()])
    assert grads[0]
    for a, b in zip(*grads):
        rel = ((a - b).norm() / b.norm().clamp_min(1e-12)).item()
        print("lora grad rel", rel)
        assert rel <= 3e-2, rel
