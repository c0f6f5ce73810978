"""CPU: the softmax-mass block score's restatement (tests/mass_ref.py) against a brute-force softmax,
the property that motivates the score (at equal budget its mask keeps more of the true attention than
the max proxy's), and the ctypes mirror of vb_mass_scores_args against the header."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import bsa_oracle as O
import mass_ref as M
import recall_ref as R
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "vblade.h")


def _streams(B, H, nb, D, seed, keep=M.KEEP):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, nb * keep, D, generator=g), torch.randn(B, H, nb * keep, D, generator=g)


@pytest.mark.parametrize("nb,D,scale", [(1, 64, None), (3, 64, None), (5, 128, 0.2), (4, 64, 3.0)])
def test_restatement_matches_brute_force_softmax(nb, D, scale):
    qs, ks = _streams(2, 2, nb, D, seed=nb + D)
    mass = M.block_mass(qs, ks, scale)
    ref = M.brute_force_mass(qs, ks, scale)
    assert mass.shape == (2, 2, nb, nb)
    assert torch.allclose(mass, ref, rtol=1e-12, atol=1e-13)
    # every sampled query spreads a mass of one over the key blocks
    assert torch.allclose(mass.sum(-1), torch.full((2, 2, nb), float(M.KEEP), dtype=torch.float64), rtol=1e-12)
    po = M.po_of(mass, torch.bfloat16)
    assert po.dtype == torch.bfloat16 and torch.allclose(po.float().sum(-1), torch.ones(2, 2, nb), atol=0.02)


def test_permuting_key_blocks_permutes_columns():
    nb, D = 6, 64
    qs, ks = _streams(1, 2, nb, D, seed=7)
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(1))
    ksp = ks.view(1, 2, nb, M.KEEP, D)[:, :, perm].reshape(1, 2, nb * M.KEEP, D)
    a, b = M.block_mass(qs, ks), M.block_mass(qs, ksp)
    assert torch.allclose(a[..., perm], b, rtol=1e-12, atol=1e-14)


def test_uniform_keys_give_uniform_scores():
    nb, D = 5, 64
    qs, _ = _streams(1, 1, nb, D, seed=3)
    ks = torch.randn(1, 1, 1, D, generator=torch.Generator().manual_seed(4)).expand(1, 1, nb * M.KEEP, D)
    mass = M.block_mass(qs, ks)
    assert torch.allclose(mass, torch.full_like(mass, M.KEEP / nb), rtol=1e-12)
    assert torch.equal(M.po_of(mass, torch.float16), torch.full((1, 1, nb, nb), 1.0 / nb).half())


def test_streams_follow_rows_and_the_replicate_pad():
    B, H, L, D = 1, 2, 300, 64
    g = torch.Generator().manual_seed(0)
    q, k = torch.randn(B, H, L, D, generator=g), torch.randn(B, H, L, D, generator=g)
    rows = torch.randperm(L, generator=g).numpy()
    q_off = O.draw_sample_offsets(B, H, generator=g)
    k_off = O.draw_sample_offsets(B, H, generator=g)
    qs, ks = M.sampled_streams(q, k, q_off, k_off, rows)
    for h in range(H):
        for i in range(3):
            for t in (0, 31):
                gq = min(128 * i + int(q_off[0, h, t]), L - 1)
                gk = min(128 * i + int(k_off[0, h, t]), L - 1)
                assert torch.equal(qs[0, h, 32 * i + t], q[0, h, rows[gq]])
                assert torch.equal(ks[0, h, 32 * i + t], k[0, h, rows[gk]])


def test_mass_mask_keeps_more_attention_than_the_max_proxy_mask():
    """The motivating property, pinned on the restatement: bench.local_qkv's generator on a 32x20x10
    grid (L = 6400, 50 blocks) in Gilbert order, H=4, D=64, the same 32 sampled tokens per block and
    the same budget of 5 blocks per row for both scores; recall of 30 probe queries per head by
    tests/recall_ref.py. The assertion is the sign only."""
    D, budget = 64, 5
    q, k, rows, q_off, k_off, pos = M.small_grid_case(H=4, D=D)
    L = q.shape[2]
    assert L == 6400
    qs, ks = M.sampled_streams(q, k, q_off, k_off, rows)
    po_max = O.pooled_scores(qs, ks, D ** -0.5, block=M.KEEP, store_dtype=torch.bfloat16)
    po_mass = M.po_of(M.block_mass(qs, ks), torch.bfloat16)
    E = R.block_masses(q, k, pos, rows)
    rec = {name: float(R.from_masses(E, M.topk_mask(po, budget), pos, L)["recall"].mean())
           for name, po in (("max", po_max), ("mass", po_mass))}
    print(f"recall at {budget} of {L // 128} blocks: max proxy {rec['max']:.4f}, sampled mass {rec['mass']:.4f}")
    assert rec["mass"] > rec["max"]


def test_ctypes_mirror_matches_header():
    from vblade._lib import MassScoresArgs
    st = "vb_mass_scores_args"
    fields = [f[0] for f in MassScoresArgs._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             f'printf("{st} %zu\\n", sizeof({st}));']
    lines += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "l")
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got[st]) == ctypes.sizeof(MassScoresArgs)
    for f in fields:
        assert int(got[f"{st}.{f}"]) == getattr(MassScoresArgs, f).offset, f


def test_refusals_without_a_gpu():
    """Every refusal happens before the first launch: the codes and messages come back on a CPU box."""
    from vblade import _lib
    lib = _lib.load()

    def args(**kw):
        a = _lib.MassScoresArgs()
        a.q = a.k = a.q_off = a.k_off = a.po = a.workspace = 4096
        a.B, a.H, a.L, a.D, a.block, a.num_keep = 1, 2, 300, 64, 128, 32
        a.q_stride = a.k_stride = (ctypes.c_int64 * 3)(2 * 300 * 64, 300 * 64, 64)
        a.dtype = _lib.VB_DTYPE_BF16
        a.workspace_bytes = 1 << 40
        for n, v in kw.items():
            setattr(a, n, v)
        return a

    cases = [(dict(num_keep=16), _lib.VB_ERR_UNSUPPORTED, "num_keep 32"),
             (dict(num_keep=64), _lib.VB_ERR_UNSUPPORTED, "num_keep 32"),
             (dict(D=96), _lib.VB_ERR_UNSUPPORTED, "head_dim"),
             (dict(L=128 * 1024 + 1), _lib.VB_ERR_UNSUPPORTED, "too long"),
             (dict(po=None), _lib.VB_ERR_INVALID, "null"),
             (dict(dtype=7), _lib.VB_ERR_INVALID, "dtype"),
             (dict(workspace_bytes=16), _lib.VB_ERR_INVALID, "workspace"),
             (dict(q=4104), _lib.VB_ERR_INVALID, "aligned"),
             (dict(q_stride=(ctypes.c_int64 * 3)(0, 0, 1 << 24)), _lib.VB_ERR_UNSUPPORTED, "2 GiB")]
    for kw, code, word in cases:
        rc = lib.vb_mask_scores_mass(ctypes.byref(args(**kw)), None)
        assert rc == code, (kw, rc)
        assert word in lib.vb_last_error().decode(), (kw, lib.vb_last_error())
    a = args()
    nb = 3
    assert lib.vb_mask_scores_mass_workspace_size(ctypes.byref(a)) == 2 * (2 * nb * 32 * 64 * 2) + 2 * nb * nb * 4 + 8
    with pytest.raises(_lib.VBladeError, match="num_keep 32"):
        _lib.check(lib.vb_mask_scores_mass(ctypes.byref(args(num_keep=16)), None), "vb_mask_scores_mass")


def test_module_option_is_validated_at_construction():
    import vblade
    kw = dict(width=4, height=4, depth=8, text_length=0, log_every=0)
    assert vblade.AdaptiveBlockSparseAttn("wan", **kw).score == "max"
    assert vblade.AdaptiveBlockSparseAttn("wan", score="mass", **kw).score == "mass"
    with pytest.raises(ValueError, match="score"):
        vblade.AdaptiveBlockSparseAttn("wan", score="sum", **kw)
    for keep in (16, 64):
        with pytest.raises(ValueError, match="32"):
            vblade.AdaptiveBlockSparseAttn("wan", score="mass", num_keep=keep, **kw)
