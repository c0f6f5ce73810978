"""Test helper (CPU, float64, torch only): an INTERVAL reference for the max-proxy pooled scores of the
mask predictor (csrc/vb_predict_kernel.hpp; oracle/bsa_oracle.pooled_scores), and the input regimes
its tests run on.

On inputs whose fp32 partial products are inexact the kernel cannot be compared with the oracle by a
tolerance: R is the fp32 block maximum rounded to the storage dtype, so one fp32 ulp of summation-order
difference next to a rounding tie moves R by a storage ulp (0.25 at |R| ~ 32 in bf16, a factor 2^0.25 in
exp2(R - m)). ``score_interval`` therefore restates pooled_scores stage by stage in float64 and carries,
per element, a pair [lo, hi] that contains the result of EVERY implementation that evaluates the same
function in fp32 with the kernel's roundings, whatever its summation order. Every stage is monotone in
its inputs (maxima, roundings, exp2, sums of non-negative terms, a quotient of non-negative terms), so
the ends are propagated by evaluating the stage at the ends.

What the kernel does, stage by stage (vb_predict_kernel.hpp, vb_common.hpp), and the width it is given:

  1. s = q . k accumulated in fp32 by MFMAs (any order): |s - S| <= (D+2) 2^-24 (|q| . |k|).
  2. x = fp32(blockmax(s) * c), c = fp32(scale) * fp32(1.44269504): one fp32 rounding.
  3. m = rowmax(x), unrounded.
  4. R = storage(x) (round_to<T>: a static_cast, round to nearest even).
  5. a = fp32(R - m), one fp32 rounding (relative 2^-24 of |a|); w = exp2_fast(a), which is
     __builtin_amdgcn_exp2f, the bare v_exp_f32 instruction: documented to 1 ulp (AMD CDNA3/CDNA4 ISA
     guide, V_EXP_F32), here given EXP2_ULPS = 4 ulps (of 2^-23 relative) so that a libm exp2 on the CPU
     fits too. The instruction does not produce denormal results: a result below 2^-126 is flushed to
     zero (the compiler's own exp2f scales its argument for that reason; the builtin does not). So
     where the upper end of w is below 2^-126 the lower end is 0. The upper end stays: the oracle's
     exp2 keeps the subnormal. This is the one semantic difference from the oracle that the interval
     absorbs; it is recorded in DESIGN.md 3.2, "Parity on inexact inputs".
  6. Po = storage(max over the q-block's keep rows of w). round_to<T> keeps subnormals of the storage
     dtype (f16 denormals are always enabled on gfx9): nothing is widened for them.
  7. tot = storage(fp32 sum of Po over the row, any order): relative nb 2^-24 for non-negative terms.
  8. storage(fp32(Po / tot)): an IEEE division (no fast-math in the unit's flags), relative 2^-24.

The kernel takes max_r (R - m_r) before the one exp2 and the oracle the exp2 of every row before the
maximum: exp2 and the rounding are monotone, so the two are the same function."""
import numpy as np
import torch

import bsa_oracle as O

U32 = 2.0 ** -24         # unit roundoff of fp32
TINY = 2.0 ** -149       # the smallest fp32 subnormal: absolute slack where a result may be subnormal
FLUSH = 2.0 ** -126      # below this v_exp_f32 returns zero
EXP2_ULPS = 4            # width given to exp2, in fp32 ulps (2^-23 relative); v_exp_f32 is documented to 1

REGIMES = ("randn", "wide", "outlier", "negative", "onehot", "flat")
EXTRA_REGIMES = ("underflow",)
# `underflow`: the dominating logit gain |q|^2 c, in log2 units at |q|^2 = D, chosen so that the rest of a
# dominated row lands around the storage dtype's subnormal range: 2^-126 (bf16: where v_exp_f32 flushes) and
# 2^-14 .. 2^-24 (f16). The block maximum over the q-block's rows picks the rows of smallest |q|^2.
UNDERFLOW_LOG2 = {(torch.bfloat16, 64): 187.0, (torch.bfloat16, 128): 162.0,
                  (torch.float16, 64): 28.0, (torch.float16, 128): 24.0}
BLOCK = 128


def _rs(x, dtype):
    """float64 -> fp32 -> storage dtype -> float64: monotone, and on fp32 values the kernel's round_to<T>."""
    return x.float().to(dtype).double()


def storage_ulp(x, dtype):
    """The unit in the last place of the storage dtype at |x| (float64 tensor), subnormal range included."""
    bits, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -200))).clamp_min(emin)
    return torch.exp2(e - bits)


def score_interval(qs, ks, sm_scale, keep, store_dtype, qblocks=32):
    """(lo, hi), float64 [B,H,n,n]: the bounds of pooled_scores(qs, ks, sm_scale, keep, store_dtype) over
    every fp32 evaluation order (module docstring). qs, ks [B,H,n*keep,D] are the sampled streams.
    Evaluated ``qblocks`` q-blocks at a time, so that nb = 321 fits in memory."""
    B, H, Ls, D = qs.shape
    n = Ls // keep
    c = float(np.float32(sm_scale) * np.float32(O.LOG2E))
    assert c > 0
    q64 = qs.double()
    kT = ks.double().transpose(-1, -2)
    kTa = kT.abs()
    e2 = EXP2_ULPS * 2.0 ** -23
    los, his = [], []
    for i0 in range(0, n, qblocks):
        qc = q64[:, :, i0 * keep:(i0 + qblocks) * keep]
        nq = qc.shape[2] // keep
        # 1. exact scores and the fp32 accumulation bound
        S = torch.matmul(qc, kT)
        dS = (D + 2) * U32 * torch.matmul(qc.abs(), kTa)
        # 2. block maxima times c, one fp32 rounding
        x_lo = (S - dS).reshape(B, H, nq * keep, n, keep).amax(-1) * c
        x_hi = (S + dS).reshape(B, H, nq * keep, n, keep).amax(-1) * c
        del S, dS
        x_lo = x_lo - x_lo.abs() * U32 - TINY
        x_hi = x_hi + x_hi.abs() * U32 + TINY
        # 3. row maxima, 4. R
        m_lo, m_hi = x_lo.amax(-1, keepdim=True), x_hi.amax(-1, keepdim=True)
        R_lo, R_hi = _rs(x_lo, store_dtype), _rs(x_hi, store_dtype)
        # 5. the exponent (one fp32 rounding of the difference) and exp2
        a_lo, a_hi = R_lo - m_hi, R_hi - m_lo
        a_lo = a_lo - a_lo.abs() * U32
        a_hi = a_hi + a_hi.abs() * U32
        w_hi = torch.exp2(a_hi) * (1 + e2) + TINY
        w_lo = (torch.exp2(a_lo) * (1 - e2) - TINY).clamp_min(0.0)
        w_lo = torch.where(w_hi < FLUSH, torch.zeros_like(w_lo), w_lo)   # v_exp_f32 flushes its result
        # 6. the q-block's maximum, rounded
        po_lo = _rs(w_lo.reshape(B, H, nq, keep, n).amax(3), store_dtype)
        po_hi = _rs(w_hi.reshape(B, H, nq, keep, n).amax(3), store_dtype)
        # 7. the row sum in fp32 (any order), rounded
        tot_lo = _rs(po_lo.sum(-1, keepdim=True) * (1 - n * U32), store_dtype)
        tot_hi = _rs(po_hi.sum(-1, keepdim=True) * (1 + n * U32), store_dtype)
        # 8. the quotient, rounded
        los.append(_rs((po_lo / tot_hi * (1 - U32) - TINY).clamp_min(0.0), store_dtype))
        his.append(_rs(po_hi / tot_lo * (1 + U32) + TINY, store_dtype))
    return torch.cat(los, 2), torch.cat(his, 2)


def sampled_streams(q, k, q_off, k_off, rows=None):
    """The predictor's sampled q and k streams [B,H,nb*keep,D]: rows gathered through ``rows`` (the
    reordered position -> caller row table, None = identity), replicate padding, the offsets of every block."""
    if rows is not None:
        q, k = q[:, :, rows.long()], k[:, :, rows.long()]
    return (O.sample_tokens(O.pad_replicate(q, BLOCK), q_off.long(), BLOCK),
            O.sample_tokens(O.pad_replicate(k, BLOCK), k_off.long(), BLOCK))


def case_inputs(regime, L, D, H, keep, dtype, B=1, seed=1, permute=True):
    """One test case: offsets and the rows permutation drawn as tests/test_gpu_predict_keep._case_setup
    draws them (one generator seeded 7: q offsets, k offsets, then the permutation), q and k of the regime,
    and their sampled streams. All on the CPU."""
    g = torch.Generator().manual_seed(7)
    qo = torch.topk(torch.rand(B, H, 1, BLOCK, generator=g), keep, dim=3).indices[:, :, 0]
    ko = torch.topk(torch.rand(B, H, 1, BLOCK, generator=g), keep, dim=3).indices[:, :, 0]
    perm = torch.randperm(L, generator=g)
    rows = perm if permute else None
    q, k = input_regime(regime, B, H, L, D, dtype, seed, rows=rows, q_off=qo, k_off=ko)
    qs, ks = sampled_streams(q, k, qo, ko, rows)
    return dict(q=q, k=k, qo=qo, ko=ko, rows=rows, qs=qs, ks=ks, nb=(L + BLOCK - 1) // BLOCK,
                B=B, H=H, L=L, D=D, keep=keep, dtype=dtype, scale=1.0 / D ** 0.5)


def position(x, lo, hi):
    """Where x lies within [lo, hi], in storage-independent units: (x - mid) / max(half width, tiny);
    |position| <= 1 inside. For printing the worst position of a result."""
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    return (x.double() - mid) / half.clamp_min(1e-300)


def outside(x, lo, hi):
    x = x.double()
    return (x < lo) | (x > hi) | torch.isnan(x)


def wide_share(lo, hi, dtype):
    """Share of elements whose interval is wider than two storage ulps of its upper end."""
    return float(((hi - lo) > 2 * storage_ulp(hi, dtype)).double().mean())


# The gain of each regime: the multiplier of N(0,1) (randn, wide, flat), of the outlier channel, of the
# dominant block's keys (onehot). GAIN_F16[(regime, D)]: lower gains in f16 at the head dims where the
# default leaves more than 10 % of a case's intervals wider than two storage ulps
# (tests/test_predict_ref.py measures the share per case). f16 resolves 2^-11: the uncertainty of m alone,
# (D+2) 2^-24 (|q|.|k|) c ln 2, is a quarter of an f16 ulp for N(0,1) at D = 128, and it grows with the
# square of the gain, as the logits' span does: the cap bounds how wide an f16 regime can be.
GAIN = {"randn": 1.0, "wide": 3.0, "outlier": 20.0, "negative": 1.0, "onehot": 4.0, "flat": 1.0}
GAIN_F16 = {("randn", 128): 0.7, ("flat", 128): 0.7, ("wide", 64): 1.25, ("wide", 128): 0.7,
            ("outlier", 64): 6.0, ("outlier", 128): 3.0, ("onehot", 64): 3.0, ("onehot", 128): 2.0}


def regime_gain(name, dtype, D):
    if name == "underflow":
        return UNDERFLOW_LOG2[dtype, D] / (O.LOG2E * D ** 0.5 * regime_gain("randn", dtype, D) ** 2)
    if dtype == torch.float16:
        return GAIN_F16.get((name, D), GAIN_F16.get(name, GAIN[name]))
    return GAIN[name]


def dominant_block(nb):
    """The key block the `onehot` regime makes dominant: 1, outside a forced tail of two at nb >= 4."""
    return min(1, nb - 1)


FLAT_BLOCK = 0   # the q-block whose rows the `flat` regime zeroes


def input_regime(name, B, H, L, D, dtype, seed, rows=None, q_off=None, k_off=None, gain=None):
    """q, k [B,H,L,D] in ``dtype`` for one regime:
      randn     N(0,1)
      wide      N(0,1) * 3: logits span tens of units, a flip of R is large
      outlier   N(0,1), one channel of q and of k (the same one) times 20, as DiT activations have
      negative  q = |x|, k = -0.3 |y|: every score and every row maximum is negative
      onehot    key block dominant_block(nb): its sampled rows are 4 x the sampled q rows of the same
                block (token t of k_off <- token t of q_off; without offsets, every token of the block)
      flat      the rows of q-block FLAT_BLOCK are zero: a uniform row of scores, exact ties
      underflow onehot with the gain of UNDERFLOW_LOG2: the rest of the dominated rows around the flush
    (the multipliers are GAIN's, in f16 GAIN_F16's; ``gain`` overrides them).
    ``rows`` (reordered position -> caller row, None = identity) says which caller rows form a block."""
    assert name in REGIMES + EXTRA_REGIMES, name
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, L, D, generator=g)
    y = torch.randn(B, H, L, D, generator=g)
    r = torch.arange(L) if rows is None else rows.long()
    gain = regime_gain(name, dtype, D) if gain is None else gain
    if name in ("randn", "wide", "flat"):
        x, y = x * gain, y * gain
    elif name == "underflow":
        x, y = x * regime_gain("randn", dtype, D), y * regime_gain("randn", dtype, D)
    elif name == "outlier":
        ch = int(torch.randint(0, D, (1,), generator=g))
        x[..., ch] *= gain
        y[..., ch] *= gain
    elif name == "negative":
        x, y = x.abs(), -0.3 * y.abs()
    if name == "flat":
        x[:, :, r[FLAT_BLOCK * BLOCK:min(L, (FLAT_BLOCK + 1) * BLOCK)]] = 0
    q = x.to(dtype)
    k = y.to(dtype)
    if name in ("onehot", "underflow"):
        nb = (L + BLOCK - 1) // BLOCK
        j = dominant_block(nb)
        pos = torch.arange(j * BLOCK, (j + 1) * BLOCK).clamp_max(L - 1)   # replicate padding
        for b in range(B):
            for h in range(H):
                src = pos if q_off is None else pos[q_off[b, h].long()]
                dst = pos if k_off is None else pos[k_off[b, h].long()]
                # (in a partial block the padding makes several tokens one row: the last written stays)
                for s, d in zip(src.tolist(), dst.tolist()):
                    k[b, h, r[d]] = (gain * q[b, h, r[s]].float()).to(dtype)
    return q, k
