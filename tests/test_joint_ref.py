"""CPU: the reference the joint-gradient tests use (tests/joint_ref.py) is the gradient of the function.

torch autograd of the fp64 statement of the one-softmax function (mean pool with replicate padding, block
mask expanded to keys, bias on the pooled logits, logsumexp) against the substituted two-branch oracle
(out1 = out2 = out, lse1 = lse, lse2 = lse - beta, alpha = 0.5, dout -> 2 dout): relative Frobenius
error <= 1e-6 per gradient (the oracle returns fp32, so ~2.5e-8 is the floor). And the option changes the
gradient: the alpha-constant two-branch form has the same dv, but its dq and dk differ by more than 1e-2
(5e-2 to 8e-2 on these N(0,1) inputs; nobody has measured real activations).
"""
import math

import pytest
import torch

import bsa_oracle as O
import joint_ref as J


def _inputs(B, H, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, H, L, D, generator=g, dtype=torch.float64) for _ in range(4))


def _clear_row2(mask):
    mask[:, :, 2, :] = False


CASES = {
    "L1000-gap7": dict(B=1, H=2, L=1000, D=64, gap=7, density=0.3, edit=None),
    "L1000-gap7-row2-cleared": dict(B=1, H=2, L=1000, D=64, gap=7, density=0.3, edit=_clear_row2),
    "L640-gap4": dict(B=1, H=1, L=640, D=64, gap=4, density=0.3, edit=None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_substituted_oracle_is_the_autograd_gradient(name):
    c = CASES[name]
    B, H, L, D, gap = c["B"], c["H"], c["L"], c["D"], c["gap"]
    q, k, v, do = _inputs(B, H, L, D, seed=11)
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, c["density"], seed=12)
    if c["edit"]:
        c["edit"](mask)
    beta = math.log(gap)
    dq, dk, dv, out, lse = J.joint_autograd(q, k, v, do, mask, gap, beta)
    assert torch.isfinite(lse).all()           # a row with no kept block still sees the pooled keys
    kp, vp = J.mean_pool(k, gap), J.mean_pool(v, gap)
    assert kp.shape[2] == (L + gap - 1) // gap
    got = J.joint_oracle_bwd(q, k, v, kp, vp, out, lse, do, mask, gap, beta)
    errs = {n: J.rel(g, r) for n, g, r in zip(("dq", "dk", "dv"), got, (dq, dk, dv))}
    print(name, errs)
    for n, e in errs.items():
        assert e <= 1e-6, (name, n, e)


def test_alpha_constant_form_has_the_joint_dv_but_not_its_dq_dk():
    c = CASES["L1000-gap7"]
    B, H, L, D, gap = c["B"], c["H"], c["L"], c["D"], c["gap"]
    q, k, v, do = _inputs(B, H, L, D, seed=11)
    nb = (L + 127) // 128
    mask = O.block_mask_from_density(B, H, nb, nb, c["density"], seed=12)
    beta = math.log(gap)
    dq, dk, dv, _, _ = J.joint_autograd(q, k, v, do, mask, gap, beta)
    aq, ak, av = J.alpha_constant_bwd(q, k, v, do, mask, gap, beta)
    diffs = {"dq": J.rel(aq, dq), "dk": J.rel(ak, dk), "dv": J.rel(av, dv)}
    print(diffs)
    assert diffs["dv"] <= 1e-6, diffs
    assert diffs["dq"] > 1e-2 and diffs["dk"] > 1e-2, diffs
