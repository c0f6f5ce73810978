"""Test helper: numpy restatement of the whole mask rule (include/vblade.h, vb_mask_rule) —
transfer_attn_to_mask's mode="topk" (cogvideo_blocksparseattn.py:205-225) and mode="energy" with
bounds per (batch, head) (:227-243) — plus a validator for selections whose tie order is free.

Per row of nc scores in the storage dtype T: stable descending order (ties: lower column first),
cum[i] = the sequential fp32 running sum of the sorted values with each prefix rounded to T,
total = cum[nc-1].
  top-k:  e = cum[k0-1]; c_lo = e >= T(total*0.6); c_hi = e >= T(total*0.9); k = k0;
          if !c_lo and k0 < nr: k = min(3k, nr); if !c_hi and k0 < nr: k = min(k//3*2, nr)   (on the
          updated k); k = min(k, nc)
  energy: k = first i with cum[i] >= T(total*thr) (nc if none), clamped to [min_keep, max_keep]
The k best columns are kept; force_tail forces the last columns and rows."""
import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def rnd(x, dt):
    """x (float32 array or scalar) rounded to the storage dtype, as float32."""
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(DTYPES[dt]).float().numpy()


def to_bits(po, dt):
    """float32 values that are exact in the storage dtype -> their 16-bit patterns."""
    po = np.ascontiguousarray(po, dtype=np.float32)
    if dt == "fp16":
        return po.astype(np.float16).view(np.uint16)
    return (po.view(np.uint32) >> 16).astype(np.uint16)


def from_bits(bits, dt):
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dt == "fp16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def to_torch(po, dt):
    return torch.from_numpy(np.asarray(po, dtype=np.float32)).to(DTYPES[dt])


def _per_head(v, B, H, dtype):
    return np.broadcast_to(np.asarray(v, dtype=dtype), (B, H))


def _cum(row_sorted, dt):
    return rnd(np.cumsum(row_sorted.astype(np.float32), dtype=np.float32), dt)


def topk_counts(po, k0, dt, lo=0.6, hi=0.9):
    """k per row [B,H,nr]; po float32 [B,H,nr,nc] (values exact in dt); k0 an int or [B,H] (values
    outside [1, nc] are clamped, as the kernel clamps device arrays)."""
    B, H, nr, nc = po.shape
    k0 = np.clip(_per_head(k0, B, H, np.int64), 1, nc)
    out = np.zeros((B, H, nr), dtype=np.int64)
    for b, h, i in np.ndindex(B, H, nr):
        cum = _cum(-np.sort(-po[b, h, i]), dt)
        tot, k, e = cum[-1], int(k0[b, h]), cum[int(k0[b, h]) - 1]
        c_lo = e >= rnd(np.float32(tot) * np.float32(lo), dt)
        c_hi = e >= rnd(np.float32(tot) * np.float32(hi), dt)
        if not c_lo and k0[b, h] < nr:
            k = min(3 * k, nr)
        if not c_hi and k0[b, h] < nr:
            k = min(k // 3 * 2, nr)
        out[b, h, i] = min(k, nc)
    return out


def energy_counts(po, min_keep, max_keep, thr, dt):
    """Clamped k per row [B,H,nr]; min_keep / max_keep / thr scalars or [B,H] (counts clamped to
    [1, nc] like device arrays; for the energy rule the clamp never changes the mask)."""
    B, H, nr, nc = po.shape
    lo = np.clip(_per_head(min_keep, B, H, np.int64), 1, nc)
    hi = np.clip(_per_head(max_keep, B, H, np.int64), 1, nc)
    th = _per_head(thr, B, H, np.float32)
    out = np.zeros((B, H, nr), dtype=np.int64)
    for b, h, i in np.ndindex(B, H, nr):
        cum = _cum(-np.sort(-po[b, h, i]), dt)
        hit = np.nonzero(cum >= rnd(np.float32(cum[-1]) * np.float32(th[b, h]), dt))[0]
        k = int(hit[0]) if hit.size else nc
        out[b, h, i] = min(max(k, lo[b, h]), hi[b, h])
    return out


def mask_from_counts(po, counts, force_tail=0):
    """The mask that keeps each row's counts[b,h,i] best columns, ties to the lower column."""
    B, H, nr, nc = po.shape
    mask = np.zeros((B, H, nr, nc), dtype=bool)
    for idx in np.ndindex(B, H, nr):
        order = np.argsort(-po[idx], kind="stable")
        mask[idx][order[:counts[idx]]] = True
    if force_tail:
        mask[..., -force_tail:] = True
        mask[..., -force_tail:, :] = True
    return mask


def mask_is_valid_selection(mask, po, counts, force_tail=0):
    """True when every row of ``mask`` is T ∪ F for SOME selection T of that row's counts[b,h,i] best
    columns (any order among equal values; counts of 0 select nothing) and F the forced tail
    columns; forced rows must be all True."""
    m = np.asarray(mask).astype(bool)
    B, H, nr, nc = m.shape
    forced = np.zeros(nc, dtype=bool)
    if force_tail:
        forced[-force_tail:] = True
    for idx in np.ndindex(B, H, nr):
        row, val, kr = m[idx], po[idx], int(counts[idx])
        if force_tail and idx[2] >= nr - force_tail:
            if not row.all():
                return False
            continue
        if not row[forced].all():
            return False
        body = row & ~forced
        if kr == 0:
            if body.any():
                return False
            continue
        vk = np.sort(val)[::-1][kr - 1]
        required, ties = val > vk, val == vk
        if not row[required].all() or (body & ~(required | ties)).any():
            return False
        need = kr - int(required.sum())
        if not (int((body & ties).sum()) <= need <= int((row & ties).sum())):
            return False
    return True
