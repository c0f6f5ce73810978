// Per-row mask rules of the mask predictor (gfx950): one wave turns a row of normalised pooled scores
// in LDS into a row of the block mask. Shared by the score kernel's epilogue (vb_predict_kernel.hpp)
// and the stand-alone mask kernels (energy_mask_kernel, rule_mask_kernel in vb_predict.hip).
#pragma once
#include "vb_common.hpp"

namespace vb {

constexpr int kMaxNb = 320;        // sampled blocks per side (L <= 40960 at block 128)
constexpr int kEnergyRow = kMaxNb + 16;   // LDS floats per energy-rule row buffer (keys padded to 16)
// the long instantiation (vb_mask_predict_long, vb_energy_mask past kMaxNb columns): rows of up to
// 1024 blocks, the attention kernels' own limit (L <= 131072)
constexpr int kMaxNbLong = 1024;
constexpr int kEnergyRowLong = kMaxNbLong + 16;
template <bool kLong> constexpr int kERow = kLong ? kEnergyRowLong : kEnergyRow;

// multi-level rank bands (value, [start, end) in ranks) for the fused level-mask epilogue
struct PredBands {
  int n;
  int value[8], start[8], end[8];
};

// vb_mask_rule resolved by the host (vb_mask_predict_rule / vb_block_mask_rule). Read only by the
// kRule instantiations; it sits at the END of PredParams so every other field keeps its offset.
struct RuleParams {
  int mode;                    // VB_RULE_ENERGY / VB_RULE_TOPK
  int k0;                      // top-k: scalar init_k (checked on the host)
  const int32_t* min_keep;     // device [B,H] or NULL: PredParams' scalar
  const int32_t* max_keep;
  const float* thr;
  const int32_t* k0_bh;        // device [B,H] or NULL: k0
  float lo, hi;                // top-k: grow below lo * total, shrink below hi * total
};

// storage bits of a value already rounded to T (non-negative): orders like the value
template <class T>
__device__ __forceinline__ uint32_t storage_bits(float v) {
  const typename T::raw r = T::from_f32(v);
  uint16_t u;
  __builtin_memcpy(&u, &r, 2);
  return u;
}

// Energy rule on one row of nc normalised scores held (storage-rounded, as f32) in LDS `val`
// (room for kEnergyRow floats); `keys` is LDS scratch for kEnergyRow uint32. One full wave.
// Sort key = (storage bits << 16) | (0xFFFF - index): larger value first, ties -> lower index
// first (a stable descending sort), one unsigned compare per pair. The fp32-accumulated
// cumulative sum over the sorted values runs sequentially (bit-identical to torch's CPU cumsum)
// as one uniform chain; lane t keeps the prefix at its own position where the clamp can see it.
// The stable descending rank of each of the lane's U values (columns lane + 64u), by one wave.
template <class T, int U>
__device__ __forceinline__ void row_ranks(const float* val, uint32_t* keys, int nc, int (&rank)[U]) {
  const int lane = threadIdx.x & 63;
  uint32_t mykey[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    mykey[u] = (j < nc) ? ((storage_bits<T>(val[j]) << 16) | (0xFFFFu - j)) : 0u;
    if (j < nc) keys[j] = mykey[u];
    rank[u] = 0;
  }
  const int nc16 = (nc + 15) & ~15;
  if (nc + lane < nc16) keys[nc + lane] = 0u;  // pad to 16: never greater than a real key
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // 16 keys (four 16-byte broadcasts) per step: four LDS reads in flight
#pragma unroll 1
  for (int t16 = 0; t16 < nc16; t16 += 16) {
    u32x4 kk[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) kk[c] = *reinterpret_cast<const u32x4*>(keys + t16 + 4 * c);
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int u = 0; u < U; ++u) rank[u] += (kk[c][e] > mykey[u]) ? 1 : 0;
  }
}

template <class T, int U>
__device__ __forceinline__ int energy_row_u(const float* val, uint32_t* keys, uint8_t* mrow, int nc, float thr,
                            int min_keep, int max_keep, int force_cols, bool force_all) {
  const int lane = threadIdx.x & 63;
  int rank[U];
  row_ranks<T, U>(val, keys, nc, rank);
  const int nc16 = (nc + 15) & ~15;
  // scatter values into sorted order (reuse `keys` as float storage after a wave barrier)
  __builtin_amdgcn_wave_barrier();
  float* sorted = reinterpret_cast<float*>(keys);
  float vals[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    vals[u] = (j < nc) ? val[j] : 0.f;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (lane + 64 * u < nc) sorted[rank[u]] = vals[u];
  if (nc + lane < nc16) sorted[nc + lane] = 0.f;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // fp32 sequential cumulative sum (torch's CPU cumsum) as ONE chain, identical in every lane,
  // over the sorted values read by 16-byte LDS broadcasts. The clamped count k only depends on the
  // first min(nc, max_keep) prefixes (cum is non-decreasing, k = #prefixes below the threshold,
  // then clamped to max_keep), so lane t records the prefix at position t + 64u only there; the
  // total is the chain's end.
  const int need = min(nc, max_keep);
  float acc = 0.f;
  float pre[U];
  const float4* s4 = reinterpret_cast<const float4*>(sorted);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    pre[u] = 0.f;
    if (64 * u >= nc16) break;
    if (64 * u < need) {
#pragma unroll 4
      for (int i4 = 0; i4 < 16; ++i4) {
        if (64 * u + 4 * i4 >= nc16) break;
        const float4 w = s4[16 * u + i4];
        const int i = 4 * i4;
        acc += w.x; pre[u] = (lane == i) ? acc : pre[u];
        acc += w.y; pre[u] = (lane == i + 1) ? acc : pre[u];
        acc += w.z; pre[u] = (lane == i + 2) ? acc : pre[u];
        acc += w.w; pre[u] = (lane == i + 3) ? acc : pre[u];
      }
    } else {
#pragma unroll 4
      for (int i4 = 0; i4 < 16; ++i4) {
        if (64 * u + 4 * i4 >= nc16) break;
        const float4 w = s4[16 * u + i4];
        acc += w.x; acc += w.y; acc += w.z; acc += w.w;   // padding past nc adds zeros
      }
    }
  }
  const float total = round_to<T>(acc);   // cum_energy[..., -1]
  const float th = round_to<T>(total * thr);
  int k = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = lane + 64 * u;
    k += __popcll(__ballot(t < need && round_to<T>(pre[u]) < th));
  }
  // all `need` prefixes below the threshold: the crossing is at or past need (k = need, which the
  // clamp maps like the reference's first crossing / nc)
  k = min(max(k, min_keep), max_keep);
  int kept = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    if (j < nc) {
      const bool keep = force_all || rank[u] < k || j >= nc - force_cols;
      mrow[j] = keep ? 1 : 0;
      kept += keep;
    }
  }
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  return kept;
}
// U = values per lane, the smallest that covers the row (ranks cost nc * U compares per lane).
// kLong: rows of up to kMaxNbLong columns (U up to 16, even past 8); rows of up to kMaxNb columns
// run the same energy_row_u<T, U> either way.
template <class T, bool kLong = false>
__device__ __forceinline__ int energy_row(const float* val, uint32_t* keys, uint8_t* mrow, int nc, float thr,
                          int min_keep, int max_keep, int force_cols, bool force_all) {
  switch ((nc + 63) >> 6) {
    case 1: return energy_row_u<T, 1>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
    case 2: return energy_row_u<T, 2>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
    case 3: return energy_row_u<T, 3>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
    case 4: return energy_row_u<T, 4>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
    default: break;
  }
  if constexpr (kLong) {
    switch ((nc + 63) >> 6) {
      case 5: break;
      case 6: return energy_row_u<T, 6>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
      case 7: return energy_row_u<T, 7>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
      case 8: return energy_row_u<T, 8>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
      case 9: case 10: return energy_row_u<T, 10>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
      case 11: case 12: return energy_row_u<T, 12>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
      case 13: case 14: return energy_row_u<T, 14>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
      default: return energy_row_u<T, (kMaxNbLong + 63) / 64>(val, keys, mrow, nc, thr, min_keep, max_keep,
                                                               force_cols, force_all);
    }
  }
  return energy_row_u<T, (kMaxNb + 63) / 64>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
}

// transfer_attn_to_mask(mode="topk") (cogvideo_blocksparseattn.py:205-225) on one row, as energy_row_u:
// the same ranks and the same sequential fp32 chain over the sorted values. The rule needs the prefix
// at position k0 - 1, anywhere in [0, nc), and the total: the chain is uniform across the wave, so
// every lane picks the one prefix up as the chain passes it. Both conditions are evaluated at k0; the
// second update reads the first one's result (:218-221). k0 in [1, nc] (clamped by the caller), `grow`
// = the reference's `seq` bound of the updates (the row count), k capped at nc. Returns the kept count.
template <class T, int U>
__device__ __forceinline__ int topk_row_u(const float* val, uint32_t* keys, uint8_t* mrow, int nc, int k0,
                                          int grow, float lo, float hi, int force_cols, bool force_all) {
  const int lane = threadIdx.x & 63;
  int rank[U];
  row_ranks<T, U>(val, keys, nc, rank);
  const int nc16 = (nc + 15) & ~15;
  __builtin_amdgcn_wave_barrier();
  float* sorted = reinterpret_cast<float*>(keys);
  float vals[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    vals[u] = (j < nc) ? val[j] : 0.f;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < U; ++u)
    if (lane + 64 * u < nc) sorted[rank[u]] = vals[u];
  if (nc + lane < nc16) sorted[nc + lane] = 0.f;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const float4* s4 = reinterpret_cast<const float4*>(sorted);
  const int at = k0 - 1;
  float acc = 0.f, e = 0.f;
#pragma unroll 4
  for (int i4 = 0; i4 < nc16 / 4; ++i4) {
    const float4 w = s4[i4];
    const int i = 4 * i4;
    acc += w.x; e = (i == at) ? acc : e;
    acc += w.y; e = (i + 1 == at) ? acc : e;
    acc += w.z; e = (i + 2 == at) ? acc : e;
    acc += w.w; e = (i + 3 == at) ? acc : e;   // padding past nc adds zeros
  }
  const float total = round_to<T>(acc);   // cum_energy[..., -1]
  e = round_to<T>(e);                     // cum_energy[..., k0 - 1]
  const bool c_lo = e >= round_to<T>(total * lo), c_hi = e >= round_to<T>(total * hi);
  int k = k0;
  if (!c_lo && k0 < grow) k = min(3 * k, grow);
  if (!c_hi && k0 < grow) k = min((k / 3) * 2, grow);
  k = min(k, nc);
  int kept = 0;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    if (j < nc) {
      const bool keep = force_all || rank[u] < k || j >= nc - force_cols;
      mrow[j] = keep ? 1 : 0;
      kept += keep;
    }
  }
  for (int o = 32; o > 0; o >>= 1) kept += __shfl_xor(kept, o);
  return kept;
}
// rows of up to kMaxNbLong columns (the rule instantiations are long ones)
template <class T>
__device__ __forceinline__ int topk_row(const float* val, uint32_t* keys, uint8_t* mrow, int nc, int k0, int grow,
                                        float lo, float hi, int force_cols, bool force_all) {
  switch ((nc + 63) >> 6) {
    case 1: return topk_row_u<T, 1>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 2: return topk_row_u<T, 2>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 3: return topk_row_u<T, 3>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 4: return topk_row_u<T, 4>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 5: return topk_row_u<T, 5>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 6: return topk_row_u<T, 6>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 7: return topk_row_u<T, 7>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 8: return topk_row_u<T, 8>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 9: case 10: return topk_row_u<T, 10>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 11: case 12: return topk_row_u<T, 12>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    case 13: case 14: return topk_row_u<T, 14>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
    default: return topk_row_u<T, (kMaxNbLong + 63) / 64>(val, keys, mrow, nc, k0, grow, lo, hi, force_cols, force_all);
  }
}

// One row under a vb_mask_rule: head bh's values are read here, once per row (bh is uniform, so these
// are scalar loads), and every value that comes from a device array is clamped to [1, nc] before it
// is used as an index or a bound. The scalars were checked on the host.
template <class T>
__device__ __forceinline__ int rule_row(const RuleParams& r, int bh, const float* val, uint32_t* keys, uint8_t* mrow,
                                        int nc, int grow, float thr, int min_keep, int max_keep, int force_cols,
                                        bool force_all) {
  if (r.mode == VB_RULE_TOPK) {
    const int k0 = r.k0_bh ? min(max(r.k0_bh[bh], 1), nc) : r.k0;
    return topk_row<T>(val, keys, mrow, nc, k0, grow, r.lo, r.hi, force_cols, force_all);
  }
  if (r.min_keep) min_keep = min(max(r.min_keep[bh], 1), nc);
  if (r.max_keep) max_keep = min(max(r.max_keep[bh], 1), nc);
  if (r.thr) thr = r.thr[bh];
  return energy_row<T, true>(val, keys, mrow, nc, thr, min_keep, max_keep, force_cols, force_all);
}

// Multi-level rank bands (transfer_attn_to_mask, Triton/cogvideo_newattn.py:154-207; vb_level_mask's
// rule, vb_ml.hip) on one row of normalised scores in LDS `val`: the column of stable descending rank
// r gets the value of the last band whose [start, end) holds r (0 if none); the last two rows and
// columns are forced to level 1. Ranks as the energy rule's (same keys), so ties go to the lower column.
template <class T, int U>
__device__ __forceinline__ void level_row_u(const float* val, uint32_t* keys, uint8_t* mrow, int nc, int row,
                                            const PredBands& lv) {
  const int lane = threadIdx.x & 63;
  int rank[U];
  row_ranks<T, U>(val, keys, nc, rank);
  if constexpr (U > (kMaxNb + 63) / 64) {
    // long rows: bands outermost, so each band's bounds are read once, not once per value (the same
    // result: the last band that holds the rank wins). Unrolled per value, the reads of `lv` in
    // all the long instantiations pass the compiler's limit for keeping a kernel argument out of
    // a private copy (scratch).
    int l[U];
#pragma unroll
    for (int u = 0; u < U; ++u) l[u] = 0;
    for (int b = 0; b < lv.n; ++b) {
      const int s = lv.start[b], e = lv.end[b], v = lv.value[b];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (rank[u] >= s && rank[u] < e) l[u] = v;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = lane + 64 * u;
      if (j < nc) mrow[j] = (uint8_t)((j >= nc - 2 || row >= nc - 2) ? 1 : l[u]);
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = lane + 64 * u;
    int l = 0;
    for (int b = 0; b < lv.n; ++b)
      if (rank[u] >= lv.start[b] && rank[u] < lv.end[b]) l = lv.value[b];
    if (j >= nc - 2 || row >= nc - 2) l = 1;
    if (j < nc) mrow[j] = (uint8_t)l;
  }
}
template <class T, bool kLong = false>
__device__ __forceinline__ void level_row(const float* val, uint32_t* keys, uint8_t* mrow, int nc, int row,
                                          const PredBands& lv) {
  switch ((nc + 63) >> 6) {
    case 1: return level_row_u<T, 1>(val, keys, mrow, nc, row, lv);
    case 2: return level_row_u<T, 2>(val, keys, mrow, nc, row, lv);
    case 3: return level_row_u<T, 3>(val, keys, mrow, nc, row, lv);
    case 4: return level_row_u<T, 4>(val, keys, mrow, nc, row, lv);
    default: break;
  }
  if constexpr (kLong) {
    switch ((nc + 63) >> 6) {
      case 5: break;
      case 6: return level_row_u<T, 6>(val, keys, mrow, nc, row, lv);
      case 7: return level_row_u<T, 7>(val, keys, mrow, nc, row, lv);
      case 8: return level_row_u<T, 8>(val, keys, mrow, nc, row, lv);
      case 9: case 10: return level_row_u<T, 10>(val, keys, mrow, nc, row, lv);
      case 11: case 12: return level_row_u<T, 12>(val, keys, mrow, nc, row, lv);
      case 13: case 14: return level_row_u<T, 14>(val, keys, mrow, nc, row, lv);
      default: return level_row_u<T, (kMaxNbLong + 63) / 64>(val, keys, mrow, nc, row, lv);
    }
  }
  return level_row_u<T, (kMaxNb + 63) / 64>(val, keys, mrow, nc, row, lv);
}

}  // namespace vb
