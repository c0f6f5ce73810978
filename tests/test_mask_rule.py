"""CPU: the mask rule's numpy restatement (tests/rule_ref.py) reproduces the reference fixture
(tests/golden/mask_rule.npz: transfer_attn_to_mask in mode="topk" and in mode="energy" with [B,H]
ratio tensors), vb_mask_rule's layout matches its ctypes mirror, and the two rule entry points
validate their arguments before any launch."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import rule_ref as R
from conftest import GOLDEN, ROOT

HEADER = os.path.join(ROOT, "include", "vblade.h")
FORCE_TAIL = {"cog": 2, "wan": 0}   # the CogVideoX copy forces the last two rows and columns


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "mask_rule.npz"))


def cases(z, kind):
    """(tag, dtype name, nb, k0) of the fixture's cases of one kind, from its key list."""
    out = []
    for key in z.files:
        p = key.split("_")
        if p[0] == kind and key.endswith("_po"):
            out.append(("_".join(p[:-1]), p[1], int(p[2]), int(p[3]) if kind != "energy" else None))
    return out


def test_fixture_holds_the_cases_the_rule_is_stated_on(fixture):
    got = {(dt, nb, k0) for _, dt, nb, k0 in cases(fixture, "topk")}
    want = {(dt, nb, k0) for dt in ("bf16", "fp16")
            for nb, k0 in ((3, 2), (5, 1), (20, 5), (20, 8), (67, 13), (65, 64))}
    assert got == want
    assert [(dt, nb) for _, dt, nb, _ in cases(fixture, "topkties")] == [("bf16", 139)]
    assert {dt for _, dt, _, _ in cases(fixture, "energy")} == {"bf16", "fp16"}
    outcomes = set()
    for tag, dt, nb, k0 in cases(fixture, "topk"):
        po = R.from_bits(fixture[tag + "_po"], dt)
        assert po.shape == (2, 3, nb, nb) and np.isfinite(po).all()
        srt = np.sort(po, axis=-1)
        assert (srt[..., 1:] > srt[..., :-1]).all(), tag   # tie-free
        kk = R.topk_counts(po, k0, dt)
        outcomes |= {"zero" if k == 0 else "stay" if k == k0 else "grow" if k > k0 else "shrink"
                     for k in kk.flatten().tolist()}
    assert outcomes == {"zero", "stay", "grow", "shrink"}


def test_topk_restatement_is_bit_equal_on_tie_free_rows(fixture):
    n = 0
    for tag, dt, nb, k0 in cases(fixture, "topk"):
        po = R.from_bits(fixture[tag + "_po"], dt)
        kk = R.topk_counts(po, k0, dt)
        for variant, ft in FORCE_TAIL.items():
            ref = fixture[f"{tag}_mask_{variant}"]
            assert np.array_equal(R.mask_from_counts(po, kk, ft), ref), (tag, variant)
            n += 1
    assert n == 24


def test_topk_restatement_on_tie_heavy_rows(fixture):
    (tag, dt, nb, k0), = cases(fixture, "topkties")
    po = R.from_bits(fixture[tag + "_po"], dt)
    srt = np.sort(po, axis=-1)
    assert (srt[..., 1:] == srt[..., :-1]).any()   # the case does hold ties
    kk = R.topk_counts(po, k0, dt)
    # the Wan module forces nothing: its rows keep exactly k
    assert np.array_equal(fixture[tag + "_mask_wan"].sum(-1), kk)
    for variant, ft in FORCE_TAIL.items():
        assert R.mask_is_valid_selection(fixture[f"{tag}_mask_{variant}"], po, kk, ft), variant
        assert R.mask_is_valid_selection(R.mask_from_counts(po, kk, ft), po, kk, ft)
    # the validator refuses a wrong count and a kept column outside the selection
    assert not R.mask_is_valid_selection(fixture[tag + "_mask_wan"], po, kk + 1, 0)
    bad = R.mask_from_counts(po, kk, 0)
    i = int(np.argmin(po[0, 0, 0]))
    assert not bad[0, 0, 0, i]
    bad[0, 0, 0, i] = True
    assert not R.mask_is_valid_selection(bad, po, kk, 0)


def test_validator_accepts_rows_that_keep_nothing():
    po = np.array([[[[0.5, 0.25, 0.25], [0.25, 0.5, 0.25], [0.25, 0.25, 0.5]]]], dtype=np.float32)
    kk = np.zeros((1, 1, 3), dtype=np.int64)
    assert R.mask_is_valid_selection(np.zeros((1, 1, 3, 3), bool), po, kk, 0)
    m = R.mask_from_counts(po, kk, 2)
    assert m[0, 0, 0].tolist() == [False, True, True] and m[0, 0, 1:].all()
    assert R.mask_is_valid_selection(m, po, kk, 2)
    m[0, 0, 0, 0] = True
    assert not R.mask_is_valid_selection(m, po, kk, 2)


def test_per_head_energy_restatement_is_a_valid_selection_per_head(fixture):
    from vblade.attention import retain_counts
    for tag, dt, nb, _ in cases(fixture, "energy"):
        po = R.from_bits(fixture[tag + "_po"], dt)
        mn, mx = fixture[tag + "_min_ratio"], fixture[tag + "_max_ratio"]
        assert mn.shape == mx.shape == po.shape[:2] and len(set(mx.flatten().tolist())) > 1
        lo = np.zeros(mn.shape, dtype=np.int64)
        hi = np.zeros(mn.shape, dtype=np.int64)
        for b, h in np.ndindex(*mn.shape):
            lo[b, h], hi[b, h] = retain_counts(nb, float(mn[b, h]), float(mx[b, h]), "cog")
        kk = R.energy_counts(po, lo, hi, 0.95, dt)
        ref = fixture[tag + "_mask_cog"]
        for b, h in np.ndindex(*mn.shape):
            s = (slice(b, b + 1), slice(h, h + 1))
            assert R.mask_is_valid_selection(ref[s], po[s], kk[s], 2), (tag, b, h)
            # each head on its own, with its own scalars, is the same rule
            assert np.array_equal(kk[s], R.energy_counts(po[s], int(lo[b, h]), int(hi[b, h]), 0.95, dt))
        assert R.mask_is_valid_selection(R.mask_from_counts(po, kk, 2), po, kk, 2)


def test_mask_rule_layout_matches_header():
    """sizeof/offsetof of vb_mask_rule from gcc == the ctypes mirror; the enum values too."""
    from vblade import _lib
    fields = [f[0] for f in _lib.MaskRule._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void){",
             'printf("size %zu\\n", sizeof(vb_mask_rule));',
             'printf("energy %d\\n", (int)VB_RULE_ENERGY);', 'printf("topk %d\\n", (int)VB_RULE_TOPK);',
             'printf("abi %d\\n", VB_ABI_VERSION);']
    lines += [f'printf("{f} %zu\\n", offsetof(vb_mask_rule, {f}));' for f in fields]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "l.c")
        open(c, "w").write("\n".join(lines))
        exe = os.path.join(d, "l")
        subprocess.check_call(["gcc", "-std=c99", c, "-o", exe])
        got = dict(line.split() for line in subprocess.check_output([exe]).decode().split("\n") if line)
    assert int(got["size"]) == ctypes.sizeof(_lib.MaskRule)
    for f in fields:
        assert int(got[f]) == getattr(_lib.MaskRule, f).offset, f
    assert (int(got["energy"]), int(got["topk"])) == (_lib.VB_RULE_ENERGY, _lib.VB_RULE_TOPK)
    assert int(got["abi"]) == _lib.ABI_VERSION == 4


def test_rule_entries_validate_arguments_without_gpu():
    from vblade import _lib
    lib = _lib.load()
    fake = 1 << 20

    def block_rule(rule, po=fake, mask=fake, nc=8, min_keep=1, max_keep=1):
        return lib.vb_block_mask_rule(po, 1, 2, 4, nc, ctypes.byref(rule) if rule is not None else None,
                                      0.95, min_keep, max_keep, 0, 0, mask, None, None, None)

    def topk(k0, bh=None):
        r = _lib.MaskRule()
        r.mode, r.init_k, r.init_k_bh = _lib.VB_RULE_TOPK, k0, bh
        return r

    assert block_rule(topk(3), po=None) == _lib.VB_ERR_INVALID and b"null" in lib.vb_last_error()
    assert block_rule(topk(3), mask=None) == _lib.VB_ERR_INVALID and b"null" in lib.vb_last_error()
    for k0 in (0, 9, -1):   # nc = 8: scalar init_k outside [1, nc]
        assert block_rule(topk(k0)) == _lib.VB_ERR_INVALID and b"init_k" in lib.vb_last_error()
    r = _lib.MaskRule()
    r.mode = 2
    assert block_rule(r) == _lib.VB_ERR_INVALID and b"mode" in lib.vb_last_error()
    assert block_rule(_lib.MaskRule(), min_keep=0) == _lib.VB_ERR_INVALID and b"keep counts" in lib.vb_last_error()
    assert block_rule(None, max_keep=0) == _lib.VB_ERR_INVALID
    assert block_rule(topk(3), nc=1025) == _lib.VB_ERR_UNSUPPORTED

    def args(L=1000, H=2):
        p = _lib.PredictArgs()
        p.q = p.k = p.q_off = p.k_off = p.po = p.mask = fake
        p.B, p.H, p.L, p.D, p.block, p.num_keep = 1, H, L, 64, 128, 32
        p.q_stride = p.k_stride = (H * L * 64, L * 64, 64)
        p.min_keep = p.max_keep = 1
        p.workspace = 1 << 24
        p.workspace_bytes = lib.vb_mask_predict_workspace_size(ctypes.byref(p))
        return p

    def predict_rule(p, rule):
        return lib.vb_mask_predict_rule(ctypes.byref(p), ctypes.byref(rule), None)

    assert lib.vb_mask_predict_rule(None, ctypes.byref(topk(3)), None) == _lib.VB_ERR_INVALID
    p = args()
    p.po = None
    assert predict_rule(p, topk(3)) == _lib.VB_ERR_INVALID and b"null" in lib.vb_last_error()
    for k0 in (0, 9):   # L = 1000: nb = 8
        assert predict_rule(args(), topk(k0)) == _lib.VB_ERR_INVALID and b"init_k" in lib.vb_last_error()
    r = _lib.MaskRule()
    r.mode = -1
    assert predict_rule(args(), r) == _lib.VB_ERR_INVALID and b"mode" in lib.vb_last_error()
    p = args()
    p.mask_level = 1
    assert predict_rule(p, topk(3)) == _lib.VB_ERR_INVALID and b"mask_level" in lib.vb_last_error()
    p = args()
    p.min_keep = 0   # energy mode without a min_keep array reads the scalar
    assert predict_rule(p, _lib.MaskRule()) == _lib.VB_ERR_INVALID and b"keep counts" in lib.vb_last_error()
    assert predict_rule(args(L=131073), topk(3)) == _lib.VB_ERR_UNSUPPORTED
    # no rule: vb_mask_predict's own checks
    p = args()
    p.min_keep = 0
    assert lib.vb_mask_predict_rule(ctypes.byref(p), None, None) == _lib.VB_ERR_INVALID
    assert b"vb_mask_predict:" in lib.vb_last_error()


def test_ops_rule_arguments_are_checked_on_the_host():
    import torch
    from vblade import ops
    with pytest.raises(ValueError, match="mode"):
        ops._rule_args(ops.MaskRule(mode="best"), 1, 2, torch.device("cpu"), 0.95, 1, 1)
    with pytest.raises(ValueError, match="init_k"):
        ops._rule_args(ops.MaskRule(mode="topk"), 1, 2, torch.device("cpu"), 0.95, 1, 1)
    with pytest.raises(ValueError, match=r"\[B,H\]"):
        ops._rule_args({"max_keep": torch.ones(3, dtype=torch.int32)}, 1, 2, torch.device("cpu"), 0.95, 1, 1)
    r, keep, thr, lo, hi = ops._rule_args({"mode": "energy", "min_keep": 3, "energy_threshold": 0.9}, 1, 2,
                                          torch.device("cpu"), 0.95, 1, 7)
    assert (r.mode, lo, hi) == (0, 3, 7) and abs(thr - 0.9) < 1e-12 and not keep
    with pytest.raises(ValueError, match="mask_mode"):
        import vblade
        vblade.AdaptiveBlockSparseAttn("cog", mask_mode="best")
    with pytest.raises(ValueError, match="init_k"):
        vblade.AdaptiveBlockSparseAttn("cog", mask_mode="topk")
