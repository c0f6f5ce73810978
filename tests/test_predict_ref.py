"""CPU: the interval reference of the max-proxy pooled scores (tests/predict_ref.py) is judged here,
before it judges the kernel (tests/test_gpu_predict_parity.py):

  * containment: the fp32 oracle (bsa_oracle.pooled_scores, one admissible evaluation) lies inside
    [lo, hi] at every element of every regime, dtype and shape: the intervals are never too tight;
  * not vacuous: per case at most 10 % of the elements have an interval wider than two storage ulps of
    its upper end (a condition on the reference alone). Elements whose lower end is 0 because v_exp_f32
    flushes ("parity on inexact inputs") are a semantic difference, not looseness, and are
    not counted; only the `underflow` regime, built to reach them, has any;
  * discriminating: each of eight CPU mutants of pooled_scores (a changed function, not a changed
    order) falls outside the interval on at least 1 % of the elements of at least one regime.

Every test prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import bsa_oracle as O
import predict_ref as P

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
# (L, D, keep): one partial block; nb = 5 with a partial last block at two densities; three blocks at
# 64 tokens per block; the D = 128 tile with nb = 9
SHAPES = [(100, 64, 32), (600, 64, 32), (600, 64, 16), (300, 64, 64), (1100, 128, 16)]
H = 3
WIDE_CAP = 0.10

_CASES = {}


def _case(regime, dt, shape):
    key = (regime, dt, shape)
    if key not in _CASES:
        L, D, keep = shape
        s = P.case_inputs(regime, L, D, H, keep, DTYPES[dt])
        s["lo"], s["hi"] = P.score_interval(s["qs"], s["ks"], s["scale"], keep, s["dtype"])
        s["po"] = O.pooled_scores(s["qs"], s["ks"], s["scale"], keep, s["dtype"])
        _CASES[key] = s
    return _CASES[key]


_PARAMS = [(r, dt, sh) for sh in SHAPES for dt in DTYPES for r in P.REGIMES + P.EXTRA_REGIMES]
_IDS = [f"{r}-{dt}-L{sh[0]}_D{sh[1]}_k{sh[2]}" for r, dt, sh in _PARAMS]


@pytest.mark.parametrize("regime,dt,shape", _PARAMS, ids=_IDS)
def test_the_fp32_oracle_lies_inside_its_interval(regime, dt, shape):
    s = _case(regime, dt, shape)
    lo, hi, po = s["lo"], s["hi"], s["po"]
    assert lo.shape == hi.shape == po.shape == (1, H, s["nb"], s["nb"])
    assert (lo <= hi).all() and (lo >= 0).all() and torch.isfinite(hi).all()
    out = P.outside(po, lo, hi)
    pos = P.position(po, lo, hi)[hi > lo]
    print(f"{regime} {dt} {shape}: outside {int(out.sum())} of {out.numel()}, worst position "
          f"{float(pos.abs().max()) if pos.numel() else 0.0:.3f}, lo == hi on {float((lo == hi).double().mean()):.3f}")
    assert not out.any()


@pytest.mark.parametrize("regime,dt,shape", _PARAMS, ids=_IDS)
def test_the_intervals_are_not_vacuous(regime, dt, shape):
    s = _case(regime, dt, shape)
    flushed = (s["lo"] == 0) & (s["hi"] > 0)
    wide = (s["hi"] - s["lo"]) > 2 * P.storage_ulp(s["hi"], s["dtype"])
    share = float((wide & ~flushed).double().mean())
    print(f"{regime} {dt} {shape}: wider than two storage ulps {share:.4f} (not counted: lower end flushed to 0, "
          f"{float(flushed.double().mean()):.4f})")
    if regime not in P.EXTRA_REGIMES:
        assert not flushed.any()   # the issue's six regimes stay clear of the flush: nothing is left uncounted
    assert share <= WIDE_CAP


def test_chunked_evaluation_equals_the_whole():
    s = _case("wide", "bf16", (1100, 128, 16))
    lo, hi = P.score_interval(s["qs"], s["ks"], s["scale"], 16, s["dtype"], qblocks=2)
    assert torch.equal(lo, s["lo"]) and torch.equal(hi, s["hi"])


# ------------------------------------------------------------------ mutants
MUTANTS = ("m_from_rounded_R", "R_unrounded", "S_rounded_before_scale", "tot_unrounded", "blockmax_clamped_at_0",
           "exp_for_exp2", "zero_padding", "head0_offsets")


def _zero_pad(x, multiple):
    rem = x.shape[-2] % multiple
    if rem == 0:
        return x
    return torch.cat([x, x.new_zeros(*x.shape[:-2], multiple - rem, x.shape[-1])], dim=-2)


def mutant_scores(mutant, s):
    """bsa_oracle.pooled_scores on the case ``s`` with one statement changed (None: unchanged)."""
    assert mutant is None or mutant in MUTANTS
    dtype, keep = s["dtype"], s["keep"]
    q, k, qo, ko = s["q"][:, :, s["rows"]], s["k"][:, :, s["rows"]], s["qo"], s["ko"]
    if mutant == "head0_offsets":
        qo, ko = qo[:, :1].expand_as(qo), ko[:, :1].expand_as(ko)
    pad = _zero_pad if mutant == "zero_padding" else O.pad_replicate
    qs, ks = O.sample_tokens(pad(q, P.BLOCK), qo), O.sample_tokens(pad(k, P.BLOCK), ko)
    B, Hh, Ls, D = qs.shape
    n = Ls // keep
    c = np.float32(np.float32(s["scale"]) * np.float32(O.LOG2E))
    bm = torch.matmul(qs.float(), ks.float().transpose(-1, -2)).reshape(B, Hh, Ls, n, keep).amax(-1)
    if mutant == "S_rounded_before_scale":
        bm = O.rnd(bm, dtype)
    if mutant == "blockmax_clamped_at_0":
        bm = bm.clamp_min(0.0)
    rowblk = bm * c
    R = rowblk if mutant == "R_unrounded" else O.rnd(rowblk, dtype)
    m = (R if mutant == "m_from_rounded_R" else rowblk).amax(-1, keepdim=True)
    w = torch.exp(R - m) if mutant == "exp_for_exp2" else torch.exp2(R - m)
    po = O.rnd(w.reshape(B, Hh, n, keep, n).amax(3), dtype)
    tot = po.sum(-1, keepdim=True)
    if mutant != "tot_unrounded":
        tot = O.rnd(tot, dtype)
    return O.rnd(po / tot, dtype)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_the_mutant_harness_unchanged_is_the_oracle(dt):
    for regime in P.REGIMES:
        s = _case(regime, dt, (600, 64, 32))
        assert torch.equal(mutant_scores(None, s), s["po"]), regime


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_leaves_the_interval(mutant):
    """At L = 600, D = 64, keep 32 (nb = 5, H = 3) in bf16 and fp16: the share of elements outside, per regime."""
    best = 0.0
    for dt in DTYPES:
        shares = {}
        for regime in P.REGIMES:
            s = _case(regime, dt, (600, 64, 32))
            shares[regime] = float(P.outside(mutant_scores(mutant, s), s["lo"], s["hi"]).double().mean())
        print(f"{mutant} {dt}: " + ", ".join(f"{r} {v:.3f}" for r, v in shares.items()))
        best = max(best, max(shares.values()))
    assert best >= 0.01
