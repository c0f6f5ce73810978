"""CPU: the fp64 op-level statement of the multi-level backward (oracle/ml_oracle.py::
multilevel_attention_bwd_lse, the reference of tests/test_gpu_ml_backward.py) against the oracle's
own Triton-form backward and the reference kernel's fixtures, and mutation checks of the per-row
metric: one wrong (q-block, key-block) pair of any level, or a wrong fold weight, must exceed the
bound the GPU tests use, while the whole-tensor norm at the old 2e-2 lets a level-8 pair through."""
import functools
import os

import numpy as np
import pytest
import torch

import bsa_oracle as O
import ml_oracle as ML
from conftest import GOLDEN

NAMES = ("dq", "dk", "dv")


def _rand(*shape, dtype=torch.bfloat16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


def _random_levels(B, H, nb, seed, p=(0.15, 0.15, 0.15, 0.25, 0.3)):
    """The GPU backward tests' level mix: values 1, 2, 4, 8, 0 with probabilities p, last column 1."""
    g = torch.Generator().manual_seed(seed)
    lv = torch.tensor([1, 2, 4, 8, 0], dtype=torch.int32)
    idx = torch.multinomial(torch.tensor(p), B * H * nb * nb, replacement=True, generator=g)
    m = lv[idx].reshape(B, H, nb, nb)
    m[..., -1] = 1
    return m


def _rel(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


@pytest.mark.parametrize("L,D,ref_tail", [(600, 64, True), (600, 64, False), (385, 128, True), (256, 64, False)])
def test_fp64_statement_agrees_with_the_triton_form(L, D, ref_tail):
    """With out, l, m of multilevel_attention (lse = m + ln l) the FlashAttention-2 form in fp64 is
    the Triton form (dO/l, m) of multilevel_attention_bwd in fp32: per-row error <= 1e-5. Head 0 has
    an all-skip q-block (lse = -inf) and a key column nobody keeps; L % 128 != 0 in three cases."""
    B, H = 1, 2
    q, k, v, do = (_rand(B, H, L, D, seed=s) for s in (1, 2, 3, 4))
    nb = (L + 127) // 128
    mask = _random_levels(B, H, nb, seed=L + D)
    mask[0, 0, 1, :] = 0
    mask[0, 0, :, 0] = 0
    fwd = ML.multilevel_attention(q, k, v, mask, ref_tail=ref_tail)
    assert torch.isneginf(fwd["lse"][0, 0, 128:256]).all()
    ref = ML.multilevel_attention_bwd(q, k, v, mask, fwd["out"], fwd["l"], fwd["m"], do)
    got = ML.multilevel_attention_bwd_lse(q, k, v, mask, fwd["out"], fwd["lse"], do, ref_tail=ref_tail)
    for name, a, r in zip(NAMES, got, ref):
        assert torch.isfinite(a).all(), name
        worst, where = O.per_row_error(a, r)
        assert worst <= 1e-5, (name, worst, where)
    assert got[0][0, 0, 128:256].abs().max() == 0
    assert got[1][0, 0, :128].abs().max() == 0 and got[2][0, 0, :128].abs().max() == 0


@pytest.mark.parametrize("case", ["f16_d64", "f16_d128_b2"])
def test_fp64_statement_matches_reference_kernel_fixture(case):
    z = np.load(os.path.join(GOLDEN, "multilevel.npz"))
    g = lambda s: torch.from_numpy(z[f"k_{case}_{s}"])  # noqa: E731
    q, k, v, do = (g(s).half() for s in ("q", "k", "v", "do"))
    lse = g("m") + torch.log(g("l"))
    got = ML.multilevel_attention_bwd_lse(q, k, v, g("mask"), g("out").half(), lse, do,
                                          store_dtype=torch.float16)
    for name, a in zip(NAMES, got):
        assert _rel(a, g(name)) <= 5e-3, name


@functools.lru_cache(maxsize=None)
def _mutation_problem():
    """L = 1280 (nb = 10), D = 64, bf16, H = 2, the random level mix: inputs, the forward's out (as
    stored) and lse, the reference, and the per-row bounds the GPU tests derive from the emulation."""
    B, H, L, D, dtype = 1, 2, 1280, 64, torch.bfloat16
    q, k, v, do = (_rand(B, H, L, D, dtype=dtype, seed=s) for s in (60, 61, 62, 63))
    mask = _random_levels(B, H, 10, seed=1280 + 7 * 64)
    fwd = ML.multilevel_attention(q, k, v, mask)
    args = (q, k, v, mask, fwd["out"].to(dtype), fwd["lse"], do)
    ref = ML.multilevel_attention_bwd_lse(*args, store_dtype=dtype)
    emu = ML.multilevel_attention_bwd_lse(*args, store_dtype=dtype, emulate_rounding=True)
    bounds = [O.per_row_bound(e, r, dtype) for e, r in zip(emu, ref)]
    return args, ref, emu, bounds


def test_rounding_emulation_is_within_the_project_bounds():
    """The emulation's own errors sit where the issue's CPU experiment put them: worst row under the
    cap (asserted by per_row_bound), whole tensor under the tight 4e-3."""
    _, ref, emu, bounds = _mutation_problem()
    for name, e, r, b in zip(NAMES, emu, ref, bounds):
        assert 2e-3 <= b <= O.PER_ROW_CAP[torch.bfloat16], (name, b)
        assert _rel(e, r) <= 4e-3, name


@pytest.mark.parametrize("level", [1, 2, 4, 8])
def test_one_dropped_pair_exceeds_the_per_row_bound(level):
    """Zero one (q-block, key-block) entry of the given level: in head 0, off the forced last column,
    in the q-block that keeps the most keys (where one pair weighs least, the hardest to see). dq,
    dk and dv all exceed the per-row bound. For level 8 the same mutant's whole-tensor dq error
    stays under the old 2e-2: the whole-tensor bound does not see it."""
    args, ref, _, bounds = _mutation_problem()
    mask = args[3]
    m0 = mask[0, 0]
    nkeys = torch.where(m0 > 0, 128 // m0.clamp_min(1), torch.zeros_like(m0)).sum(1)
    where = (m0[:, :-1] == level).nonzero().tolist()
    assert where
    i, j = max(where, key=lambda ij: (int(nkeys[ij[0]]), -ij[0], -ij[1]))
    bad = mask.clone()
    bad[0, 0, i, j] = 0
    mut = ML.multilevel_attention_bwd_lse(args[0], args[1], args[2], bad, *args[4:])
    for name, m, r, b in zip(NAMES, mut, ref, bounds):
        worst, _ = O.per_row_error(m, r)
        assert worst > b, (level, name, worst, b)
    if level == 8:
        assert _rel(mut[0], ref[0]) < 2e-2


def test_wrong_fold_weight_exceeds_the_per_row_bound():
    """The level-8 fold at 1/4 instead of 1/8: dk and dv exceed the per-row bound, dq is untouched."""
    args, ref, _, bounds = _mutation_problem()
    mut = ML.multilevel_attention_bwd_lse(*args, fold_weights=(1.0, 0.5, 0.25, 0.25))
    assert torch.equal(mut[0], ref[0])
    for name, m, r, b in list(zip(NAMES, mut, ref, bounds))[1:]:
        worst, _ = O.per_row_error(m, r)
        assert worst > b, (name, worst, b)
