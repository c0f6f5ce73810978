"""CPU checks of the long-sequence (gathered-key) reference in oracle/bsa_oracle.py and of the cases of
tests/long_bwd_cases.py, which test_gpu_long_backward.py holds vb_attn_bwd to past 256 blocks:

  * the gathered forms equal the dense ones (1e-12 in fp64) at small shapes with Lq != Lk, ragged
    tails, an empty mask row, a key column nobody keeps and the pooled branch with gap 7;
  * the masks carry the designed lists exactly;
  * at S1 (258 blocks) a list that loses, doubles or mis-tails one entry moves the touched rows to at
    least 2 x the per-row bound, while the whole tensor of a lost entry stays under the 2e-2 of the
    full-size tests (tests/test_gpu_backward.py): a lost second chunk passes a whole-tensor check;
  * the draws listed in long_bwd_cases.RESEED hold O.per_row_bound's cap.

Measured at S1, D=64, bf16 (emulation worst rows dq 4.07e-3, dk 4.03e-3, dv 3.95e-3; bounds twice
that), touched rows' worst error as a multiple of the bound, and the mutated whole tensor's error:
  mutation                                  touched rows            whole tensor
  q-list {256,257} loses 256 / 257          dk 82x / 38x, dv 72x / 35x     1.3e-2 / 4.7e-3
  q-list lanes (9 entries) loses 256        dk 86x, dv 49x                 1.2e-2
  q-list ends loses 256                     dk 42x, dv 34x                 1.0e-2
  q-list full (258 entries) loses 256 / 257 dk 14x / 5.0x, dv 8.4x / 5.3x  1.2e-2 / 4.9e-3
  key list {256,257} loses 256 / 257        dq 126x / 103x                 7.9e-2 / 2.7e-2 (seen: see the test)
  key list lanes loses 256                  dq 56x                         1.1e-2
  key list ends loses 256                   dq 28x                         5.5e-3
  key list full loses 256                   dq 2.3x                        2.4e-3
  an entry counted twice                    49x .. 126x
  the 17-row last block's half-tile full    dq 30x .. 5800x, dk/dv 36x .. 2000x
One entry of a list of n moves the list's rows by about 1/sqrt(n): 6 % at 258 entries, 3 % at 1024,
against bounds of 0.8 %. One key block lost from a full key list shows at 2.3 x the bound at S1 and
would not reach 2 x at S3; block 257's 17 keys lost from a full key list do not show at all (0.9 x).
The sparse designed lists are what make a lost entry unmistakable.
"""
import functools
import math
import types

import pytest
import torch

import bsa_oracle as O
import long_bwd_cases as C

BF16 = torch.bfloat16
NAMES = ("dq", "dk", "dv")


def _rand(*shape, dtype=BF16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype)


# ----------------------------------------------------------------------------------------------
# gathered = dense
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small(Lq, Lk, gap):
    """B=2, H=2, D=32: q-block 1 of head 1 keeps nothing, key block 2 is kept by nobody."""
    B, H, D = 2, 2, 32
    s = types.SimpleNamespace(gap=gap, kp=None, vp=None)
    s.q, s.do = _rand(B, H, Lq, D, seed=1), _rand(B, H, Lq, D, seed=4)
    s.k, s.v = _rand(B, H, Lk, D, seed=2), _rand(B, H, Lk, D, seed=3)
    s.mask = O.block_mask_from_density(B, H, (Lq + 127) // 128, (Lk + 127) // 128, 0.5, seed=5)
    s.mask[:, 1, 1, :] = False
    s.mask[:, :, :, 2] = False
    if gap:
        s.kp, s.vp = O.simple_pooling(s.k, gap), O.simple_pooling(s.v, gap)
    return s


SMALL = [(300, 700, 0), (700, 300, 0), (333, 333, 7), (513, 385, 7)]


@pytest.mark.parametrize("Lq,Lk,gap", SMALL)
def test_gathered_forward_equals_the_dense_one(Lq, Lk, gap):
    s = _small(Lq, Lk, gap)
    bias = math.log(gap) if gap else 0.0
    for use_main in ((True, False) if gap else (True,)):
        ref, lse = O.joint_attention(s.q, s.k, s.v, s.mask, s.kp, s.vp, bias, use_main=use_main)
        got, got_lse = O.gathered_attention(s.q, s.k, s.v, s.mask, kp=s.kp, vp=s.vp, bias=bias, use_main=use_main)
        empty = torch.isneginf(lse)
        assert torch.equal(empty, torch.isneginf(got_lse)) and bool(empty.any()) == (gap == 0)
        assert float((got - ref).abs().max()) <= 1e-12
        assert float((got_lse - lse)[~empty].abs().max()) <= 1e-12
        # the fp32 emulation: the same roundings on another summation order, so a result may land on
        # the neighbouring storage value (one unit in the last place), rarely
        for pre in (False, True):
            kw = dict(kp=s.kp, vp=s.vp, use_main=use_main, store_dtype=BF16, prescale_q=pre)
            emu, emu_lse = O.attention_fwd_emulated(s.q, s.k, s.v, s.mask, kp_log_bias=bias, **kw)
            gemu, gemu_lse = O.gathered_attention(s.q, s.k, s.v, s.mask, kp=s.kp, vp=s.vp, bias=bias, use_main=use_main,
                                                  emulate=dict(store_dtype=BF16, prescale_q=pre))
            assert float((gemu_lse - emu_lse)[~empty].abs().max()) <= 4e-6
            diff = (gemu - emu).abs()
            assert bool((diff <= 2.0 ** -7 * emu.abs()).all()) and float((diff > 0).float().mean()) <= 1e-3


@pytest.mark.parametrize("rdtype", [None, BF16, torch.float16], ids=["fp64", "bf16", "f16"])
@pytest.mark.parametrize("Lq,Lk,gap", SMALL)
def test_gathered_backward_equals_the_dense_one(Lq, Lk, gap, rdtype):
    s = _small(Lq, Lk, gap)
    out, lse = O.joint_attention(s.q, s.k, s.v, s.mask)
    w = torch.rand(s.q.shape[:3], generator=torch.Generator().manual_seed(6))
    args = (s.q, s.k, s.v, out, lse, s.do, w, s.mask, 0.2, 128, rdtype)
    for a, b in zip(O._branch_bwd(*args), O._branch_bwd_gathered(*args)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max()))
    # dq of the empty row and dk, dv of the unkept column are exactly zero in both
    dq, dk, dv = O._branch_bwd_gathered(*args)
    assert dq[:, 1, 128:256].abs().max() == 0 and dk[:, :, 256:384].abs().max() == 0 and dv[:, :, 256:384].abs().max() == 0
    if gap and rdtype is not torch.float16:
        out2, lse2 = O.joint_attention(s.q, None, None, None, s.kp, s.vp, use_main=False)
        full = (s.q, s.k, s.v, s.kp, s.vp, out, lse, out2, lse2, w, s.do, s.mask, gap)
        kw = dict(sm_scale=0.2, emulate_rounding=rdtype is not None)
        dense = O.two_branch_attention_bwd(*full, **kw)
        for a, b in zip(dense, O.two_branch_attention_bwd(*full, **kw, gathered=True)):
            if rdtype is None:
                assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())   # fp32 results of 1e-12-equal fp64
            else:
                assert torch.equal(a, b)


def test_existing_entry_points_return_the_same_bits():
    """The dense forms' defaults did not move: two_branch_attention_bwd without ``gathered`` is
    _branch_bwd's arithmetic (the golden fixtures of test_oracle_backward.py pin its values)."""
    s = _small(333, 333, 7)
    out, lse = O.joint_attention(s.q, s.k, s.v, s.mask)
    args = (s.q, s.k, s.v, None, None, out, lse, None, None, None, s.do, s.mask, 0)
    dq, dk, dv = O._branch_bwd(s.q, s.k, s.v, out, lse, s.do, torch.ones(s.q.shape[:3]), s.mask, 32 ** -0.5, 128, None)
    for a, b in zip(O.two_branch_attention_bwd(*args), (dq, dk, dv)):
        assert torch.equal(a, b.float())


# ----------------------------------------------------------------------------------------------
# the masks
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [258, 591, 1024])
def test_masks_carry_the_designed_lists(nb):
    m = C.long_mask(nb, 2, 11, "split")
    lists, at = C.designed_lists(nb, 12), C.designed_at(nb)
    assert len(set(at.values())) == len(C.LIST_NAMES) and nb - 1 not in at.values()
    for n in C.LIST_NAMES:
        assert torch.nonzero(m[0, 0, at[n]]).flatten().tolist() == lists[n]
        assert torch.nonzero(m[0, 1, :, at[n]]).flatten().tolist() == lists[n]
    assert lists["lanes"][:4] == [0, 63, 64, 127] and lists["full"] == list(range(nb))
    assert all(x < 64 or x >= 64 * ((nb - 1) // 64) for x in lists["ends"])
    assert min(lists["ends"]) < 64 and max(lists["ends"]) >= 64 * ((nb - 1) // 64)
    assert lists["from256"][0] == 256 and lists["last"] == [nb - 1] and 0.2 * nb < len(lists["random30"]) < 0.4 * nb
    # the half-tile rule both ways: the last block closes the last row's and another row's key list
    # (head 0) and the last column's and another column's q-list (head 1); other lists end earlier
    for h, mm in ((0, m[0, 0]), (1, m[0, 1].T)):
        ends_last = torch.nonzero(mm[:, nb - 1]).flatten().tolist()
        assert nb - 1 in ends_last and len(ends_last) >= 2 and len(ends_last) < nb
    # every other row keeps 4 blocks or fewer besides what the designed lines of the other axis add
    assert int(m[0, 1].sum(-1).max()) <= 4 + len(C.LIST_NAMES) and int(m[0, 0].sum(-2).max()) <= 30 + len(C.LIST_NAMES)
    one = C.long_mask(nb, 1, 11, "one")
    assert not bool(one[0, 0, at["empty"]].any()) and not bool(one[0, 0, :, at["empty"]].any())
    assert int(one[0, 0, at["full"]].sum()) == nb - 1 and int(one[0, 0, :, at["full"]].sum()) == nb - 1


def test_case_table():
    ids = [c.id for c in C.CASES]
    assert len(set(ids)) == len(ids)
    assert [c.nb for c in C.MAIN] == [258, 258, 258, 258, 591, 1024]
    assert C.S1 % 128 == 17 and C.S2 % 128 == 80 and C.S3 == 1024 * 128
    c = C.POOLED_ONE_RANGE
    Lkp = (c.L + c.gap - 1) // c.gap
    assert Lkp == 4702 and (Lkp + 127) // 128 * c.H >= 2049 and c.nb > 256


# ----------------------------------------------------------------------------------------------
# mutations at S1
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _s1():
    c = C.MAIN[0]
    assert c.id == "S1-D64-bf16"
    d = C.build(c)
    s = types.SimpleNamespace(c=c, d=d, nb=c.nb)
    out, lse = C.cpu_statistics(d)
    w = torch.ones(d.q.shape[:3])
    s.G = lambda mask, rd, **kw: O._branch_bwd_gathered(d.q, d.k, d.v, out, lse, d.do, w, mask, d.scale, 128, rd, **kw)  # noqa: E731
    s.ref = tuple(t.float() for t in s.G(d.mask, None))
    s.base = s.G(d.mask, BF16)
    s.emu = tuple(t.to(BF16).float() for t in s.base)
    s.bound = tuple(O.per_row_bound(e, r, BF16) for e, r in zip(s.emu, s.ref))
    return s


def _mutated(s, head, qblocks, edit_keys=None, edit_kv=None, full_tail=False):
    """The emulation's gradients with the contributions of head ``head``'s q-blocks ``qblocks``
    replaced by those of wrong lists: ``edit_keys(counts)`` edits the integer mask the dQ side reads,
    ``edit_kv(counts)`` the one the dK/dV side reads. Every product is linear in the (q-block, key
    block) pairs, so only those q-blocks are recomputed."""
    only = torch.zeros(s.d.mask.shape, dtype=torch.int64)
    only[0, head, qblocks] = s.d.mask[0, head, qblocks].long()
    keys, kv = only.clone(), only.clone()
    if edit_keys:
        edit_keys(keys[0, head])
    if edit_kv:
        edit_kv(kv[0, head])
    true = s.G(only, BF16)
    wrong = s.G(keys, BF16, kv_mask=kv, full_tail=full_tail)
    return tuple((b - t + w).to(BF16).float() for b, t, w in zip(s.base, true, wrong))


def _touched(s, mut, which, head, block):
    """Worst per-row error of gradient ``which`` over the rows of ``block`` in ``head``, over its bound."""
    rows = slice(block * 128, min(s.c.L, (block + 1) * 128))
    return float(O.per_row_errors(mut[which], s.ref[which])[0, head, rows].max()) / s.bound[which]


def _edit(i, j, to):
    def f(counts):
        assert counts[i, j] == 1
        counts[i, j] = to
    return f


# (designed list, the entry it loses): 256 is the first entry of chunk 4 (wave 0's second round), 257 the
# last block (17 rows). S1 has 258 blocks, so "the last block" and "index 257" are one place here.
DROPS = [("from256", 256), ("from256", 257), ("lanes", 256), ("ends", 256), ("full", 256), ("full", 257)]


def test_the_lists_hold_the_entries_the_mutations_drop():
    lists = C.designed_lists(258, C.MAIN[0].seed + 5)
    for name, entry in DROPS:
        assert entry in lists[name], (name, entry)
    assert len(lists["from256"]) == 2 and len(lists["lanes"]) == 9


@pytest.mark.parametrize("name,entry", DROPS)
def test_a_q_list_that_loses_an_entry_shows_in_its_key_rows(name, entry):
    """Column ``name`` of head 1 (the dK/dV kernel's q-list of that key block) loses q-block 256 or
    257: that key block's dk and dv rows move to at least 2 x the bound, while both whole tensors
    stay under the full-size tests' 2e-2."""
    s = _s1()
    j = C.designed_at(s.nb)[name]
    mut = _mutated(s, 1, [entry], edit_kv=_edit(entry, j, 0))
    assert torch.equal(mut[0], s.emu[0])
    for which in (1, 2):
        ratio = _touched(s, mut, which, 1, j)
        whole = C.frob(mut[which], s.ref[which])
        print(f"q-list {name} loses {entry}: {NAMES[which]} touched rows {ratio:.1f} x bound, whole tensor {whole:.2e}")
        assert ratio >= 2.0 and whole < 2e-2


@pytest.mark.parametrize("name,entry", DROPS[:-1])
def test_a_key_list_that_loses_an_entry_shows_in_its_query_rows(name, entry):
    """Row ``name`` of head 0 (the dQ kernel's key list of that q-block) loses key block 256 or 257:
    that q-block's dq rows move to at least 2 x the bound. The whole tensor stays under 2e-2 except
    for the two-entry list: a q-block left with 17 or 128 of its 145 keys has dq rows several times
    the tensor's typical row, and a whole-tensor check does see that one. Not claimed: the full list
    losing block 257, whose 17 keys are 0.05 % of the row's (measured 0.9 x the bound)."""
    s = _s1()
    i = C.designed_at(s.nb)[name]
    mut = _mutated(s, 0, [i], edit_keys=_edit(i, entry, 0))
    assert torch.equal(mut[1], s.emu[1]) and torch.equal(mut[2], s.emu[2])
    ratio, whole = _touched(s, mut, 0, 0, i), C.frob(mut[0], s.ref[0])
    print(f"key list {name} loses {entry}: dq touched rows {ratio:.1f} x bound, whole tensor {whole:.2e}")
    assert ratio >= 2.0 and (whole < 2e-2 or name == "from256")


@pytest.mark.parametrize("name", ["from256", "lanes"])
def test_an_entry_counted_twice_shows(name):
    s = _s1()
    at = C.designed_at(s.nb)[name]
    mut = _mutated(s, 1, [256], edit_kv=_edit(256, at, 2))
    r = [_touched(s, mut, 1, 1, at), _touched(s, mut, 2, 1, at)]
    mut = _mutated(s, 0, [at], edit_keys=_edit(at, 256, 2))
    r.append(_touched(s, mut, 0, 0, at))
    print(f"{name} counts 256 twice: dk {r[0]:.1f} dv {r[1]:.1f} dq {r[2]:.1f} x bound")
    assert min(r) >= 2.0


def test_a_short_last_block_taken_as_two_half_tiles_shows():
    """S1's last block has 17 rows, so the kernels drop its second half-tile (ntiles -= 1). Taken as
    full, its 64 clamped copies of the last row enter dq of every q-block that keeps the last key
    block, and dk/dv of every key block the last q-block keeps."""
    s = _s1()
    nb, m = s.nb, s.d.mask
    for head in (0, 1):
        keepers = torch.nonzero(m[0, head, :, nb - 1]).flatten().tolist()
        assert nb - 1 in keepers and len(keepers) >= 2
        mut = _mutated(s, head, sorted(set(keepers) | {nb - 1}), full_tail=True)
        rq = [_touched(s, mut, 0, head, i) for i in keepers]
        rk = [_touched(s, mut, w, head, j) for j in torch.nonzero(m[0, head, nb - 1]).flatten().tolist() for w in (1, 2)]
        print(f"half-tile taken as full, head {head}: dq {min(rq):.1f}..{max(rq):.1f}, dk/dv {min(rk):.1f}..{max(rk):.1f} x bound")
        assert min(rq) >= 2.0 and min(rk) >= 2.0


def test_unmutated_recomputation_is_the_emulation():
    """_mutated without an edit gives the emulation back (the linearity it relies on), and the empty
    row's dq and the unkept column's dk, dv are exactly zero in the reference."""
    s = _s1()
    at = C.designed_at(s.nb)
    mut = _mutated(s, 0, [at["full"], 256])
    for a, b in zip(mut, s.emu):
        assert float((a - b).abs().max()) <= 2.0 ** -7 * float(b.abs().max()) and float((a != b).float().mean()) <= 1e-6
    e = slice(at["empty"] * 128, at["empty"] * 128 + 128)
    assert s.ref[0][0, 0, e].abs().max() == 0 and s.ref[1][0, 1, e].abs().max() == 0 and s.ref[2][0, 1, e].abs().max() == 0


# ----------------------------------------------------------------------------------------------
# reseeded draws
# ----------------------------------------------------------------------------------------------
def test_reseeded_draws_hold_the_cap():
    """Every case listed in RESEED is a case of the table and its listed draw holds per_row_bound's
    cap on the CPU emulation (the CPU forward emulation standing in for the device's statistics)."""
    by_id = {c.id: c for c in C.CASES}
    for cid in C.RESEED:
        c = by_id[cid]
        d = C.build(c)
        out, lse = C.cpu_statistics(d)
        ref, emu = C.backward_reference(d.q, d.k, d.v, d.do, out, lse, d.mask, c.dtype)
        for e, r in zip(emu, ref):
            O.per_row_bound(e, r, c.dtype)
