// Block-sparse FMHA backward for gfx950 (MI355X): FlashAttention-2 gradient semantics, deterministic.
//
// Replaces the backward of the external block_sparse_attn_func (mit-han-lab/Block-Sparse-Attention)
// as the reference's autograd reaches it (cogvideox/train/special_attentions_local/TrainRelated/
// cogvideo_blocksparseattn.py:316-320 sparse call, :106-109 dense pooled call) together with the
// autograd of the surrounding adaptive_block_sparse_attn ops (:366-393):
//   * the softmax LSE is a constant (the library's backward ignores its gradient), hence the combine
//     weight a = exp(lse1 - M)/(...) is a constant too: dO1 = a*dO, dO2 = (1-a)*dO;
//   * each branch back-propagates with its own output and LSE;
//   * pooled-branch K/V gradients flow back through the mean pool (replicate padding folds onto the
//     last token) and the Gilbert gather (a scatter to the caller's rows).
// The branch weight is folded into the row statistic: a*P1 = exp2(S*c - (lse1*log2e - log2 a)),
// so dO itself is used unscaled and Delta = rowsum(dO * O_branch) (FA2's D_i) per branch.
//
// Kernels (all 256 threads = 4 waves, v_mfma_f32_32x32x16, operand maps in vb_tiles.hpp):
//   bwd_prep_kernel   per row: -Delta1/2, L'1/2 -> stats [B*H][ntile64][4][64] fp32 (Delta negated:
//                     it seeds the dP accumulators, see below); optional
//                     reordered contiguous copies of q and dO (one gather pass instead of one per
//                     key block that reads them). Its kJoint form (vb_attn_bwd_joint) writes the
//                     statistics of the exact gradient of the one-softmax function instead: one
//                     LSE and one Delta, L'2 = (lse - beta) log2e; the kernels below are the same
//   bwd_dkdv_kernel   one workgroup per (b, h, 128-key block); wave = 32 keys held in registers;
//                     streams the 64-row Q / dO tiles of every q-block that keeps this key block
//                     (mask column; all q-blocks for pooled keys) through LDS by LDS-DMA:
//                       S = Q.K^T, dP = dO.V^T         (C: lane = key, registers = q rows)
//                       P = exp2(S c - L'), dS = P (dP - Delta)
//                       dV^T += dO^T.P, dK^T += Q^T.dS (A = ds_read_b64_tr_b16 of the Q/dO tiles)
//                     pooled keys -> fp32 workspace; full-resolution keys -> dk/dv rows (kv_rows),
//                     adding the mean-pool adjoint of the pooled grads
//   bwd_dq_kernel     one workgroup per (b, h, 128-row q-block), the forward's geometry: streams the
//                     kept K/V tiles then the pooled ones:
//                       S^T = K.Q^T, dP^T = V.dO^T      (C: lane = query, registers = keys)
//                       dQ^T += K^T.dS^T                (A = transposed read of the K tile)
// No atomics: every gradient element is written by exactly one workgroup, so results are
// bit-reproducible run to run (the reference's deterministic=True).
#include <type_traits>

#include "vb_args.hpp"
#include "vb_attn_bwd.hpp"

namespace vb {

// ------------------------------------------------------------------------------------------------
// prep: one thread per 16-byte chunk of a row
// ------------------------------------------------------------------------------------------------
// kJoint (vb_attn_bwd_joint): out / lse belong to one softmax over the kept keys and the pooled keys
// with the logit bias beta = pool_log_bias. Its exact gradient has one Delta = rowsum(dO * O) for both
// key sets, P = exp(S c - lse) on the kept keys and P = exp(S c + beta - lse) on the pooled ones,
// whose scores carry no bias in the gradient kernels: L'2 = (lse - beta) log2e. out2, lse2 and alpha
// are never read.
template <class T, bool kJoint = false>
__global__ void __launch_bounds__(256) bwd_prep_kernel(const PrepParams p) {
  const int CH = p.D / 8;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t rows_per_bh = (int64_t)p.ntile * 64;
  const int64_t total = (int64_t)p.B * p.H * rows_per_bh * CH;
  if (idx >= total) return;  // CH divides 64: whole row groups leave together
  const int ch = idx % CH;
  const int64_t rid = idx / CH;
  const int g = rid % rows_per_bh;
  const int bh = rid / rows_per_bh;
  const int b = bh / p.H, h = bh % p.H;
  int Lq = p.Lq, qrow0 = 0;
  if (p.cu_q) { qrow0 = p.cu_q[b]; Lq = p.cu_q[b + 1] - qrow0; }
  const bool valid = g < Lq;
  const int row = valid ? (p.q_rows ? p.q_rows[g] : g) : 0;
  float d1 = 0.f, d2 = 0.f;
  if (valid) {
    const int64_t r = qrow0 + row;
    const u32x4 dov = *reinterpret_cast<const u32x4*>(
        reinterpret_cast<const uint8_t*>(p.dout) + 2 * (b * p.dos[0] + h * p.dos[1] + r * p.dos[2] + ch * 8));
    const u32x4 ov = *reinterpret_cast<const u32x4*>(
        reinterpret_cast<const uint8_t*>(p.out) + 2 * (b * p.os[0] + h * p.os[1] + r * p.os[2] + ch * 8));
    u32x4 o2v = {0, 0, 0, 0};
    if (!kJoint && p.out2)
      o2v = *reinterpret_cast<const u32x4*>(
          reinterpret_cast<const uint8_t*>(p.out2) + 2 * (b * p.o2s[0] + h * p.o2s[1] + r * p.o2s[2] + ch * 8));
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const float x = T::bits_to_f32((dov[e] >> (16 * s)) & 0xffff);
        d1 += x * T::bits_to_f32((ov[e] >> (16 * s)) & 0xffff);
        if (!kJoint) d2 += x * T::bits_to_f32((o2v[e] >> (16 * s)) & 0xffff);
      }
    if (p.q_r) {
      const u32x4 qv = *reinterpret_cast<const u32x4*>(
          reinterpret_cast<const uint8_t*>(p.q) + 2 * (b * p.qs[0] + h * p.qs[1] + r * p.qs[2] + ch * 8));
      const int64_t dst = 2 * (((int64_t)bh * p.Lq + g) * p.D + ch * 8);
      *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(p.q_r) + dst) = qv;
      *reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(p.do_r) + dst) = dov;
    }
  }
  // reduce over the CH consecutive lanes of this row (CH in {8, 16}, aligned groups)
  for (int o = 1; o < CH; o <<= 1) {
    d1 += __shfl_xor(d1, o);
    if (!kJoint) d2 += __shfl_xor(d2, o);
  }
  if (ch != 0) return;
  float l1 = bwd::kBigL, l2 = bwd::kBigL;
  if (valid) {
    const int64_t li = (int64_t)bh * p.Lq + row;
    const float lse1 = p.lse[li];
    if (kJoint) {
      // one LSE and one Delta for both key sets; the pooled scores get their bias through L'2
      if (lse1 > -INFINITY) {
        l1 = fminf(lse1 * kLog2e, bwd::kBigL);
        l2 = fminf((lse1 - p.pool_log_bias) * kLog2e, bwd::kBigL);
      }
      d2 = d1;
    } else {
      const float a = p.alpha ? p.alpha[li] : 1.f;
      // a * P1 = exp2(S c - (lse1 log2e - log2 a)); rows with no kept key (lse = -inf) or a = 0
      // contribute nothing
      if (lse1 > -INFINITY && a > 0.f) l1 = fminf(lse1 * kLog2e - __log2f(a), bwd::kBigL);
      if (p.lse2) {
        const float w2 = round_to<T>(1.f - a);  // the reference's bf16 (1 - alpha), :393
        const float lse2 = p.lse2[li];
        if (lse2 > -INFINITY && w2 > 0.f) l2 = fminf(lse2 * kLog2e - __log2f(w2), bwd::kBigL);
      }
    }
  } else {
    d1 = d2 = 0.f;
  }
  float* st = p.stats + ((int64_t)bh * p.ntile + g / 64) * 256 + (g & 63);
  st[0] = l1;
  st[64] = -d1;
  st[128] = l2;
  st[192] = -d2;
}

// ------------------------------------------------------------------------------------------------
// dK / dV: one workgroup per (b, h, 128-key block)
// ------------------------------------------------------------------------------------------------
// kW: waves per workgroup (4, or 2 for the multi-level pooled items: an item is 32 kW pyramid rows,
// so a level-2 item covers one key block and walks its own q-list instead of a union, and a level-4
// or level-8 item half as many blocks; the union walk leaves fewer waves idle).
template <int D, class T, bool kPooled, bool kML = false, int kW = 4>
__global__ void __launch_bounds__(kW * 64, D == 128 ? 1 : bwd::kDkdvWavesD64) bwd_dkdv_kernel(const BwdParams p) {
  using namespace bwd;
  static_assert(kW == 4 || (kML && kPooled), "2-wave workgroups: the multi-level pooled items only");
  constexpr int kRows = 32 * kW;             // keys (pyramid rows) per work item
  constexpr int kPrioKV = D == 128 ? kDkdvPrio128 : kDkdvPrio64;
  constexpr int KS = D / 16;
  constexpr int DT = D / 32;
  constexpr int RB = D * 2;                 // bytes per row
  constexpr int kTileBytes = kT * RB;       // one 64-row Q (or dO) tile
  constexpr int kInstTile = kTileBytes / 1024;
  constexpr int kRowsPerInst = 1024 / RB;
  constexpr int kCh = RB / 16;
  constexpr int kInst = 2 * kInstTile + 1;  // Q, dO, stats (1 KiB)
  constexpr int kBufBytes = 2 * kTileBytes + 1024;
  // LDS ring: tile t read, t+1 in flight, t+2 being issued; kW = 2: a 2-slot ring (38 KiB with the
  // lists), so four 2-wave workgroups fit a CU (two waves per SIMD, as the 4-wave form)
  constexpr int kBufs = kW == 2 ? 2 : 3;
  __shared__ __attribute__((aligned(16))) uint8_t smem[kBufs * kBufBytes + kMaxBlocks * 3 + 16];
  uint16_t* list = reinterpret_cast<uint16_t*>(smem + kBufs * kBufBytes);
  int* list_n = reinterpret_cast<int*>(smem + kBufs * kBufBytes + kMaxBlocks * 2);
  uint8_t* list_bits = smem + kBufs * kBufBytes + kMaxBlocks * 2 + 16;   // multi-level: active blocks

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;

  const int BH = p.B * p.H;
  const int nkb = kPooled ? p.nbkp : p.nbk;
  const int split = kPooled ? (int)blockIdx.x % p.psplit : 0;
  int bh, kblk;
  int ml_e = 0, ml_m = 0;   // multi-level pooled items: level exponent and pyramid block
  if (kML && kPooled) {
    // longest items first: a level-8 block's q-list is the union over 8 key blocks (≈4x a level-2
    // item's tiles), so level 8, then 4, then 2, each spread over the heads (consecutive
    // workgroups = different heads, so different XCDs); placement only, the results are the same
    int lin = (int)blockIdx.x;
    ml_e = 3;
    auto nit = [&](int e) { return ((p.Lpad >> e) + kRows - 1) / kRows; };   // items of level e
    while (ml_e > 1 && lin >= nit(ml_e) * BH) { lin -= nit(ml_e) * BH; --ml_e; }
    bh = lin % BH;
    ml_m = lin / BH;
    kblk = 0;
  } else {
    dkdv_item<kPooled, kML>(p, BH, nkb, bh, kblk);
  }
  const int b = bh / p.H, h = bh % p.H;

  int Lq, Lk;
  int64_t qrow0, krow0;
  seq_bounds(p, b, Lq, Lk, qrow0, krow0);
  int Lkey = kPooled ? p.Lkp : Lk;
  int k0 = kblk * kBlk;
  // multi-level: level e (p = 2^e) of this work item, its pyramid region start and row count
  int ml_row0 = 0;
  if (!(kML && kPooled)) ml_m = kblk;
  if (kML) {
    const MlGeom gm(p.Lpad);
    ml_row0 = gm.off[ml_e];
    Lkey = kPooled ? p.Lpad >> ml_e : Lk;
    k0 = ml_m * (kPooled ? kRows : kBlk);
  }
  if (k0 >= Lkey) return;
  // a varlen sequence with keys and no query (Lq = 0): an empty q-list, and the epilogue writes the
  // zero dk/dv rows (as for a key block that no mask row keeps)
  const int nbq = Lq > 0 ? (Lq + kBlk - 1) / kBlk : 0;

  bool nan_head = false;
  const uint8_t* mcol = nullptr;
  if (!kPooled || kML) {
    const uint8_t* mh = head_mask_base(p.mask, p.ms, p.head_mask_type, p.H, b, h, nan_head, p.hm_mode);
    if (mh) mcol = mh + (kML ? ((k0 << ml_e) >> 7) : kblk);   // the item's first key block
  }
  const int qlo = (kPooled && !kML) ? split * nbq / p.psplit : 0;
  const int qhi = (kPooled && !kML) ? (split + 1) * nbq / p.psplit : nbq;
  if (kML) {
    // q-blocks where any of this item's 2^e key blocks has level 2^e; bit e' = block ml_m*2^e + e'
    if (threadIdx.x < 64) {
      const int pl = 1 << ml_e;
      const int nblk_here = min((kRows << ml_e) >> 7, p.nbk - ((k0 << ml_e) >> 7));
      int n = 0;
      for (int i0 = 0; i0 < nbq; i0 += 64) {
        const int i = i0 + lane;
        int bits = 0;
        if (i < nbq)
          for (int e = 0; e < nblk_here; ++e) bits |= (mcol[(int64_t)i * p.ms[2] + e] == pl) << e;
        const unsigned long long bal = __ballot(bits != 0);
        if (bits) {
          const int pos = n + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
          list[pos] = (uint16_t)i;
          list_bits[pos] = (uint8_t)bits;
        }
        n += __popcll(bal);
      }
      if (lane == 0) *list_n = n;
    }
  } else if (threadIdx.x < 64) {
    int n = 0;
    for (int i0 = qlo; i0 < qhi; i0 += 64) {
      const int i = i0 + lane;
      const bool keep = (i < qhi) && (mcol == nullptr || mcol[(int64_t)i * p.ms[2]] != 0);
      const unsigned long long bal = __ballot(keep);
      if (keep) {
        const int pos = n + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
        list[pos] = (uint16_t)i;
      }
      n += __popcll(bal);
    }
    if (lane == 0) *list_n = n;
  }

  // this wave's 32 keys as B operands (lane = key, d = 16 ks + 8 half + 0..7)
  const int key = k0 + wave * 32 + l32;
  const bool kvalid = key < Lkey;
  const int keyc = kvalid ? key : Lkey - 1;
  const uint8_t* kb = (kPooled && !kML)
      ? reinterpret_cast<const uint8_t*>(p.kp) + 2 * (b * p.kps[0] + h * p.kps[1] + (int64_t)keyc * p.kps[2])
      : reinterpret_cast<const uint8_t*>(p.k) + 2 * (b * p.ks[0] + h * p.ks[1] + (krow0 + ml_row0 + keyc) * p.ks[2]);
  const uint8_t* vb_ = (kPooled && !kML)
      ? reinterpret_cast<const uint8_t*>(p.vp) + 2 * (b * p.vps[0] + h * p.vps[1] + (int64_t)keyc * p.vps[2])
      : reinterpret_cast<const uint8_t*>(p.v) + 2 * (b * p.vs[0] + h * p.vs[1] + (krow0 + ml_row0 + keyc) * p.vs[2]);
  // multi-level: which of the item's key blocks this lane's key belongs to, and the logit bias
  const int my_blk_bit = kML ? (wave * 32 + l32) / (kBlk >> ml_e) : 0;
  const float lvl_bias = (float)ml_e;
  typename T::vec8 kf[KS], vf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kf[s] = *reinterpret_cast<const typename T::vec8*>(kb + (16 * s + 8 * half) * 2);
    vf[s] = *reinterpret_cast<const typename T::vec8*>(vb_ + (16 * s + 8 * half) * 2);
  }
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    asm volatile("" : "+v"(kf[s]));
    asm volatile("" : "+v"(vf[s]));
  }
  __syncthreads();
  const int nlist = __builtin_amdgcn_readfirstlane(*list_n);
  int ntiles = 2 * nlist;
  if (nlist > 0 && list[nlist - 1] == nbq - 1 && (nbq - 1) * kBlk + kT >= Lq) ntiles -= 1;

  const uint8_t* qsrc = reinterpret_cast<const uint8_t*>(p.q) + 2 * (b * p.qs[0] + h * p.qs[1] + qrow0 * p.qs[2]);
  const uint8_t* dosrc = reinterpret_cast<const uint8_t*>(p.dout) + 2 * (b * p.dos[0] + h * p.dos[1] + qrow0 * p.dos[2]);
  const int qrowb = 2 * (int)p.qs[2], dorowb = 2 * (int)p.dos[2];   // host: every slice < 2 GiB
  const float* stsrc = p.stats + (int64_t)bh * p.ntile * 256;

  // Tile t (64 q rows) -> ring slot t % kBufs by LDS-DMA through buffer descriptors: this wave
  // issues instructions i = wave + 4k (i < kInstTile: Q, then dO, then the stats KiB). A lane's
  // part of each instruction (row within the tile, swizzled chunk) is a fixed voffset; the tile's
  // first row is the scalar soffset. Rows past Lq read as zeros (their stats make P = 0).
  constexpr int kHi = (kInst + kW - 1) / kW, kLo = kInst / kW;  // DMA instructions per wave and tile
  const bool many = wave < (kInst % kW);
  const srd_t q_srd = make_srd(qsrc, (int)((int64_t)(Lq - 1) * qrowb + RB));
  const srd_t do_srd = make_srd(dosrc, (int)((int64_t)(Lq - 1) * dorowb + RB));
  const srd_t st_srd = make_srd(stsrc, p.ntile * 1024);
  int voff[kHi];
#pragma unroll
  for (int k = 0; k < kHi; ++k) {
    const int i = wave + kW * k;
    voff[k] = lane * 16;
    if (i < 2 * kInstTile) {
      const int ii = i < kInstTile ? i : i - kInstTile;
      const int r = ii * kRowsPerInst + lane / kCh;
      const int c = (lane % kCh) ^ dual_swz<D>(r);
      voff[k] = r * (i < kInstTile ? qrowb : dorowb) + c * 16;
    }
  }
  auto issue = [&](int t, int slot) __attribute__((always_inline)) {
    const int qb = __builtin_amdgcn_readfirstlane(list[t >> 1]);
    const int row0 = qb * kBlk + (t & 1) * kT;
    uint8_t* buf = smem + slot * kBufBytes;
#pragma unroll
    for (int k = 0; k < kHi; ++k) {
      const int i = wave + kW * k;
      if (i >= kInst) break;
      if (i < kInstTile) dma16(q_srd, buf + i * 1024, voff[k], row0 * qrowb);
      else if (i < 2 * kInstTile) dma16(do_srd, buf + i * 1024, voff[k], row0 * dorowb);
      else dma16(st_srd, buf + i * 1024, voff[k], (row0 / 64) * 1024);
    }
  };

  f32x16 dk[DT], dv[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dk[i][r] = dv[i][r] = 0.f;

  const int trr = tr_row(lane), trc = tr_col(lane);
  constexpr int fL = (kPooled && !kML) ? 2 : 0;  // stats fields of this branch
  constexpr bool kSeed = D == 64;   // D=128: dP seeded with -Delta too measured 6 % slower on Wan's dK/dV

  if (ntiles > 0) issue(0, 0);
  if (kBufs == 3 && ntiles > 1) issue(1, 1);
  // The loop body is instantiated once per ring slot: every LDS address is a compile-time offset.
  auto body = [&](int t, auto U) __attribute__((always_inline)) {
    constexpr int u_slot = decltype(U)::value;
    // retire this wave's DMAs of tile t (tile t+1 stays in flight); the barrier makes every wave's
    // part visible and proves slot (t-1) % kBufs is no longer being read
    if (kBufs == 3 && t + 1 < ntiles) {
      if (many) VB_WAIT_VMCNT(kHi);
      else VB_WAIT_VMCNT(kLo);
    } else {
      VB_WAIT_VMCNT(0);
    }
    __builtin_amdgcn_s_barrier();
    if constexpr (kBufs == 3) {
      if (t + 2 < ntiles) issue(t + 2, (u_slot + 2) % kBufs);
    } else {
      if (t + 1 < ntiles) issue(t + 1, (u_slot + 1) % kBufs);   // into slot (t-1) % 2, free after the barrier
    }
    const uint8_t* qt = smem + u_slot * kBufBytes;
    const uint8_t* dot = qt + kTileBytes;
    const float* st = reinterpret_cast<const float*>(qt + 2 * kTileBytes);
    // multi-level pooled items: keys of blocks without level 2^e for this q-block take no part
    bool act = true;
    if (kML && kPooled) {
      act = (list_bits[t >> 1] >> my_blk_bit) & 1;
      // The item's q-block list is the union over its 2^e key blocks; a wave whose own key
      // blocks are not at level 2^e for this q-block has nothing to add (P = 0 for all its keys)
      // and skips the tile's MFMAs, leaving its SIMD to the co-resident waves. A wave holds one
      // block's keys at levels 2 and 4, two blocks' at level 8. Its tile would add exact zeros,
      // so the sums are unchanged.
      if (!__any(act)) return;
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      // dP's accumulator starts at -Delta of its row (register r = row 4j+e of this u half; the
      // stats hold -Delta, read straight into the accumulator), so dS = P * (dO.V^T - Delta) needs
      // no subtraction per score
      f32x16 s, dp;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 Dv = *reinterpret_cast<const f32x4*>(st + (fL + 1) * 64 + 32 * u + 8 * j + 4 * half);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[4 * j + e] = 0.f;
          dp[4 * j + e] = kSeed ? Dv[e] : 0.f;
        }
      }
      if constexpr (kPrioKV & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        s = T::mfma32(lds_b128<T>(qt, dual_off<D>(32 * u + l32, 2 * ks + half)), kf[ks], s);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        dp = T::mfma32(lds_b128<T>(dot, dual_off<D>(32 * u + l32, 2 * ks + half)), vf[ks], dp);
      if constexpr (kPrioKV & 1) __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 Lv = *reinterpret_cast<const f32x4*>(st + fL * 64 + 32 * u + 8 * j + 4 * half);
        f32x4 Dv2 = {0.f, 0.f, 0.f, 0.f};
        if (!kSeed) Dv2 = *reinterpret_cast<const f32x4*>(st + (fL + 1) * 64 + 32 * u + 8 * j + 4 * half);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * j + e;
          float pr;
          if (kML) pr = act ? exp2_fast(fmaf(s[r], p.c, lvl_bias - Lv[e])) : 0.f;
          else pr = exp2_fast(fmaf(s[r], p.c, -Lv[e]));
          s[r] = pr;
          dp[r] = pr * (kSeed ? dp[r] : dp[r] + Dv2[e]);
        }
      }
      // dV^T += dO^T.P and dK^T += Q^T.dS over (16-row half sb, 32-wide d tile dt) steps; the four
      // transposed reads of step j+1 are issued before step j's MFMAs and waited for with
      // lgkmcnt(4), so each wait only covers reads issued one step earlier
      typename T::vec8 pp[2], pd[2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) {
        pp[sb] = pack8<T>(s, 8 * sb);
        pd[sb] = pack8<T>(dp, 8 * sb);
      }
      constexpr int NST = 2 * DT;
      s16x4 rdo[2][2], rq[2][2];   // [ring][lo/hi]
      auto rd = [&](int j, int slot) __attribute__((always_inline)) {
        const int rr = 32 * u + 16 * (j / DT) + trr;
        const int cc = 32 * (j % DT) + trc;
        rdo[slot][0] = lds_tr4_asm_at(dot, dual_off_col<D>(rr, cc));
        rdo[slot][1] = lds_tr4_asm_at(dot, dual_off_col<D>(rr + 8, cc));
        rq[slot][0] = lds_tr4_asm_at(qt, dual_off_col<D>(rr, cc));
        rq[slot][1] = lds_tr4_asm_at(qt, dual_off_col<D>(rr + 8, cc));
      };
      rd(0, 0);
      if constexpr (kPrioKV & 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        const int sl = j & 1;
        if (j + 1 < NST) {
          rd(j + 1, sl ^ 1);
          asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(rdo[sl][0]), "+v"(rdo[sl][1]), "+v"(rq[sl][0]), "+v"(rq[sl][1]));
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rdo[sl][0]), "+v"(rdo[sl][1]), "+v"(rq[sl][0]), "+v"(rq[sl][1]));
        }
        const int sb = j / DT, dt = j % DT;
        dv[dt] = T::mfma32(join8<T>(rdo[sl][0], rdo[sl][1]), pp[sb], dv[dt]);
        dk[dt] = T::mfma32(join8<T>(rq[sl][0], rq[sl][1]), pd[sb], dk[dt]);
      }
      if constexpr (kPrioKV & 2) __builtin_amdgcn_s_setprio(0);
    }
  };
  for (int t0 = 0; t0 < ntiles; t0 += kBufs) {
    body(t0, std::integral_constant<int, 0>{});
    if (t0 + 1 < ntiles) body(t0 + 1, std::integral_constant<int, 1>{});
    if constexpr (kBufs == 3) {
      if (t0 + 2 < ntiles) body(t0 + 2, std::integral_constant<int, 2>{});
    }
  }

  // ---- epilogue: lane = key, registers = d ---------------------------------------------------------
  if (!kvalid) return;
  const float nanf_ = __builtin_nanf("");
  if (kML && kPooled) {   // pooled pyramid rows: fp32 grads, summed into dk/dv by the level-1 pass
    const int64_t po = (int64_t)bh * (7 * (p.Lpad / 8)) + (ml_row0 - p.Lpad) + key;
    float* dkr = p.dkpyr + po * D;
    float* dvr = p.dvpyr + po * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = dt * 32 + 8 * g4 + 4 * half;
        f32x4 a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = dk[dt][4 * g4 + e] * p.scale;
          c[e] = dv[dt][4 * g4 + e];
        }
        *reinterpret_cast<f32x4*>(dkr + d) = a;
        *reinterpret_cast<f32x4*>(dvr + d) = c;
      }
    return;
  }
  if (kML) {   // level-1 key (< L): + the mean-pool adjoints of its level-2/4/8 rows (KML:1494-1563)
    const int64_t rb = (int64_t)bh * (7 * (p.Lpad / 8));
    const float* pk[3];
    const float* pv[3];
#pragma unroll
    for (int e = 1; e < 4; ++e) {
      const int64_t row = rb + (MlGeom(p.Lpad).off[e] - p.Lpad) + (key >> e);
      pk[e - 1] = p.dkpyr + row * D;
      pv[e - 1] = p.dvpyr + row * D;
    }
    const int64_t orow = p.kv_rows ? p.kv_rows[key] : krow0 + key;
    uint8_t* dkr = reinterpret_cast<uint8_t*>(p.dk) + 2 * (b * p.dks[0] + h * p.dks[1] + orow * p.dks[2]);
    uint8_t* dvr = reinterpret_cast<uint8_t*>(p.dv) + 2 * (b * p.dvs[0] + h * p.dvs[1] + orow * p.dvs[2]);
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = dt * 32 + 8 * g4 + 4 * half;
        float a[4], c[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = dk[dt][4 * g4 + e] * p.scale;
          c[e] = dv[dt][4 * g4 + e];
        }
#pragma unroll
        for (int lv = 0; lv < 3; ++lv) {
          const float w = 1.0f / (float)(2 << lv);
          const f32x4 x = *reinterpret_cast<const f32x4*>(pk[lv] + d);
          const f32x4 y = *reinterpret_cast<const f32x4*>(pv[lv] + d);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            a[e] = fmaf(x[e], w, a[e]);
            c[e] = fmaf(y[e], w, c[e]);
          }
        }
        u32x2 w2, z;
        w2[0] = pack2<T>(a[0], a[1]); w2[1] = pack2<T>(a[2], a[3]);
        z[0] = pack2<T>(c[0], c[1]); z[1] = pack2<T>(c[2], c[3]);
        *reinterpret_cast<u32x2*>(dkr + d * 2) = w2;
        *reinterpret_cast<u32x2*>(dvr + d * 2) = z;
      }
    return;
  }
  if (kPooled) {
    const int64_t po = ((int64_t)split * BH + bh) * p.Lkp + key;
    float* dkr = p.dkp_part + po * D;
    float* dvr = p.dvp_part + po * D;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = dt * 32 + 8 * g4 + 4 * half;
        f32x4 a, c;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = dk[dt][4 * g4 + e] * p.scale;
          c[e] = dv[dt][4 * g4 + e];
        }
        *reinterpret_cast<f32x4*>(dkr + d) = a;
        *reinterpret_cast<f32x4*>(dvr + d) = c;
      }
    return;
  }
  // full-resolution key: + mean-pool adjoint of the pooled grads (replicate padding folds onto
  // the last token), written at the caller's row
  const float* pk = nullptr;
  const float* pv = nullptr;
  float pw = 0.f;
  if (p.dkp) {
    const int gp = key / p.gap;
    pk = p.dkp + ((int64_t)bh * p.Lkp + gp) * D;
    pv = p.dvp + ((int64_t)bh * p.Lkp + gp) * D;
    const int extra = (key == Lk - 1) ? p.Lkp * p.gap - Lk : 0;
    pw = (float)(1 + extra) / (float)p.gap;
  }
  const int64_t orow = p.kv_rows ? p.kv_rows[key] : krow0 + key;
  uint8_t* dkr = reinterpret_cast<uint8_t*>(p.dk) + 2 * (b * p.dks[0] + h * p.dks[1] + orow * p.dks[2]);
  uint8_t* dvr = reinterpret_cast<uint8_t*>(p.dv) + 2 * (b * p.dvs[0] + h * p.dvs[1] + orow * p.dvs[2]);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = dt * 32 + 8 * g4 + 4 * half;
      float a[4], c[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = dk[dt][4 * g4 + e] * p.scale;
        c[e] = dv[dt][4 * g4 + e];
      }
      if (pk) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(pk + d);
        const f32x4 y = *reinterpret_cast<const f32x4*>(pv + d);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] = fmaf(x[e], pw, a[e]);
          c[e] = fmaf(y[e], pw, c[e]);
        }
      }
      if (nan_head) {
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = c[e] = nanf_;
      }
      u32x2 w, z;
      w[0] = pack2<T>(a[0], a[1]); w[1] = pack2<T>(a[2], a[3]);
      z[0] = pack2<T>(c[0], c[1]); z[1] = pack2<T>(c[2], c[3]);
      *reinterpret_cast<u32x2*>(dkr + d * 2) = w;
      *reinterpret_cast<u32x2*>(dvr + d * 2) = z;
    }
}

// ------------------------------------------------------------------------------------------------
// dQ: one workgroup per (b, h, 128-row q-block); kept full-resolution tiles then pooled tiles
// ------------------------------------------------------------------------------------------------
template <int D, class T, bool kPool, bool kML = false>
__global__ void __launch_bounds__(bwd::kThreads, D == 128 ? bwd::kDqWavesD128 : bwd::kDqWavesD64) bwd_dq_kernel(const BwdParams p) {
  using namespace bwd;
  constexpr int KS = D / 16;
  constexpr int DT = D / 32;
  constexpr int RB = D * 2;
  constexpr int kTileBytes = kT * RB;       // one 64-key K (or V) tile
  constexpr int kInstTile = kTileBytes / 1024;
  constexpr int kRowsPerInst = 1024 / RB;
  constexpr int kCh = RB / 16;
  constexpr int kInst = 2 * kInstTile;
  constexpr int kBufBytes = 2 * kTileBytes;
  // 2-slot K/V ring with a second barrier per tile (D=128 at two waves per SIMD: 68 KiB)
  constexpr int kRing = 2;
  __shared__ __attribute__((aligned(16))) uint8_t smem[kRing * kBufBytes + kMaxBlocks * 2 + 16];
  uint16_t* list = reinterpret_cast<uint16_t*>(smem + kRing * kBufBytes);
  int* list_n = reinterpret_cast<int*>(smem + kRing * kBufBytes + kMaxBlocks * 2);

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = lane >> 5;
  const int l32 = lane & 31;

  const int BH = p.B * p.H;
  int qblk, bh;
  dq_item(p, BH, bh, qblk);
  const int b = bh / p.H, h = bh % p.H;
  int Lq, Lk;
  int64_t qrow0, krow0;
  seq_bounds(p, b, Lq, Lk, qrow0, krow0);
  const int q0 = qblk * kBlk;
  if (q0 >= Lq) return;
  const int nbk = (Lk + kBlk - 1) / kBlk;

  bool nan_head = false;
  const uint8_t* mrow = nullptr;
  const bool use_main = p.k != nullptr;
  if (use_main) {
    const uint8_t* mh = head_mask_base(p.mask, p.ms, p.head_mask_type, p.H, b, h, nan_head, p.hm_mode);
    if (mh) mrow = mh + (int64_t)qblk * p.ms[2];
  }
  if (kML) {
    // per-level key-block lists (levels 1, 2, 4, 8 in that order; as the forward)
    if (threadIdx.x < 64) {
      int cnt[4] = {0, 0, 0, 0};
      for (int j0 = 0; j0 < nbk; j0 += 64) {
        const int j = j0 + lane;
        const int lv = j < nbk ? mrow[j] : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) cnt[e] += __popcll(__ballot(lv == (1 << e)));
      }
      int pos[4] = {0, cnt[0], cnt[0] + cnt[1], cnt[0] + cnt[1] + cnt[2]};
      for (int j0 = 0; j0 < nbk; j0 += 64) {
        const int j = j0 + lane;
        const int lv = j < nbk ? mrow[j] : 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const unsigned long long bal = __ballot(lv == (1 << e));
          if (lv == (1 << e))
            list[pos[e] + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u))] = (uint16_t)j;
          pos[e] += __popcll(bal);
        }
      }
      if (lane < 4) list_n[lane] = lane == 0 ? cnt[0] : lane == 1 ? cnt[1] : lane == 2 ? cnt[2] : cnt[3];
    }
  } else if (threadIdx.x < 64) {
    int n = 0;
    if (use_main) {
      for (int j0 = 0; j0 < nbk; j0 += 64) {
        const int j = j0 + lane;
        const bool keep = (j < nbk) && (mrow == nullptr || mrow[j] != 0);
        const unsigned long long bal = __ballot(keep);
        if (keep) {
          const int pos = n + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32),
                                                        __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
          list[pos] = (uint16_t)j;
        }
        n += __popcll(bal);
      }
    }
    if (lane == 0) *list_n = n;
  }

  // this wave's 32 query rows: Q and dO as B operands (lane = query)
  const int g = q0 + wave * 32 + l32;
  const bool qvalid = g < Lq;
  const int gc = qvalid ? g : Lq - 1;
  typename T::vec8 qf[KS], df[KS];
  {
    const uint8_t* qp = reinterpret_cast<const uint8_t*>(p.q) +
                        2 * (b * p.qs[0] + h * p.qs[1] + (qrow0 + gc) * p.qs[2]);
    const uint8_t* dp_ = reinterpret_cast<const uint8_t*>(p.dout) +
                         2 * (b * p.dos[0] + h * p.dos[1] + (qrow0 + gc) * p.dos[2]);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = *reinterpret_cast<const typename T::vec8*>(qp + (16 * s + 8 * half) * 2);
      df[s] = *reinterpret_cast<const typename T::vec8*>(dp_ + (16 * s + 8 * half) * 2);
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      asm volatile("" : "+v"(qf[s]));
      asm volatile("" : "+v"(df[s]));
    }
  }
  // the clamped row's statistics, as the Q/dO loads (padding rows are never stored)
  const float* st = p.stats + ((int64_t)bh * p.ntile + gc / 64) * 256 + (gc & 63);
  float L1 = st[0], D1 = st[64], L2 = st[128], D2 = st[192];   // D1, D2 = -Delta
  asm volatile("" : "+v"(L1), "+v"(D1), "+v"(L2), "+v"(D2));

  __syncthreads();
  const int nkept = __builtin_amdgcn_readfirstlane(*list_n);
  int ntm = 2 * nkept;
  if (nkept > 0 && list[nkept - 1] == nbk - 1 && (nbk - 1) * kBlk + kT >= Lk && !(kML && p.ref_tail)) ntm -= 1;
  const int ntp = kPool ? (p.Lkp + kT - 1) / kT : 0;
  // multi-level tiles (as the forward): level 1 (2 per block), one per level-2 block, two level-4
  // blocks and four level-8 blocks per tile
  int n2 = 0, n4 = 0, n8 = 0, T12 = 0, T124 = 0;
  if (kML) {
    n2 = __builtin_amdgcn_readfirstlane(list_n[1]);
    n4 = __builtin_amdgcn_readfirstlane(list_n[2]);
    n8 = __builtin_amdgcn_readfirstlane(list_n[3]);
    T12 = ntm + n2;
    T124 = T12 + (n4 + 1) / 2;
  }
  const int ntiles = kML ? T124 + (n8 + 3) / 4 : ntm + ntp;
  // multi-level tile t: pyramid row of 16-row quarter qd, valid keys, level exponent
  const int off4 = p.Lpad + p.Lpad / 2, off8 = off4 + p.Lpad / 4;
  auto ml_quarter = [&](int t, int qd) __attribute__((always_inline)) -> int {
    if (t < ntm) return (int)list[t >> 1] * kBlk + (t & 1) * kT + 16 * qd;
    if (t < T12) return p.Lpad + (int)list[nkept + t - ntm] * 64 + 16 * qd;
    if (t < T124) {
      const int e = min(2 * (t - T12) + (qd >> 1), n4 - 1);
      return off4 + (int)list[nkept + n2 + e] * 32 + 16 * (qd & 1);
    }
    const int e = min(4 * (t - T124) + qd, n8 - 1);
    return off8 + (int)list[nkept + n2 + n4 + e] * 16;
  };
  auto ml_klen = [&](int t) __attribute__((always_inline)) -> int {
    if (t < ntm) return p.ref_tail ? kT : min(kT, Lk - ((int)list[t >> 1] * kBlk + (t & 1) * kT));
    if (t < T12) return kT;
    if (t < T124) return min(kT, (n4 - 2 * (t - T12)) * 32);
    return min(kT, (n8 - 4 * (t - T124)) * 16);
  };
  auto ml_lvl = [&](int t) __attribute__((always_inline)) -> int {
    return t < ntm ? 0 : t < T12 ? 1 : t < T124 ? 2 : 3;
  };

  const uint8_t* kbase = use_main ? reinterpret_cast<const uint8_t*>(p.k) + 2 * (b * p.ks[0] + h * p.ks[1] + krow0 * p.ks[2]) : nullptr;
  const uint8_t* vbase = use_main ? reinterpret_cast<const uint8_t*>(p.v) + 2 * (b * p.vs[0] + h * p.vs[1] + krow0 * p.vs[2]) : nullptr;
  const uint8_t* kpbase = kPool ? reinterpret_cast<const uint8_t*>(p.kp) + 2 * (b * p.kps[0] + h * p.kps[1]) : nullptr;
  const uint8_t* vpbase = kPool ? reinterpret_cast<const uint8_t*>(p.vp) + 2 * (b * p.vps[0] + h * p.vps[1]) : nullptr;

  auto tile_keys = [&](int t, int& kstart, int& klen) __attribute__((always_inline)) {
    if (t < ntm) {
      const int blk = __builtin_amdgcn_readfirstlane(list[t >> 1]);
      kstart = blk * kBlk + (t & 1) * kT;
      klen = min(kT, Lk - kstart);
    } else {
      kstart = (t - ntm) * kT;
      klen = min(kT, p.Lkp - kstart);
    }
  };
  // Tile t -> ring slot by LDS-DMA through buffer descriptors (as the dK/dV kernel): this wave
  // issues instructions i = wave + 4k (K tile first, then V). A lane's part of each instruction
  // (row within the tile, swizzled chunk) is a fixed 32-bit voffset per key source; the tile's first
  // key is the scalar soffset, so no per-lane 64-bit address math runs per tile. The host checks
  // that every (b,h) slice spans < 2 GiB.
  static_assert(kInst % 4 == 0, "every wave issues the same number of DMA instructions");
  constexpr int kPer = kInst / 4;
  const int krowb = 2 * (int)p.ks[2], vrowb = 2 * (int)p.vs[2];
  const int kprowb = kPool ? 2 * (int)p.kps[2] : 0, vprowb = kPool ? 2 * (int)p.vps[2] : 0;
  const int src_rows = kML ? 15 * (p.Lpad / 8) : Lk;
  const srd_t k_srd = make_srd(use_main ? kbase : nullptr, use_main ? (int)((int64_t)(src_rows - 1) * krowb + RB) : 0);
  const srd_t v_srd = make_srd(use_main ? vbase : nullptr, use_main ? (int)((int64_t)(src_rows - 1) * vrowb + RB) : 0);
  const srd_t kp_srd = make_srd(kPool ? kpbase : nullptr, kPool ? (int)((int64_t)(p.Lkp - 1) * kprowb + RB) : 0);
  const srd_t vp_srd = make_srd(kPool ? vpbase : nullptr, kPool ? (int)((int64_t)(p.Lkp - 1) * vprowb + RB) : 0);
  int dr[kPer], dc16[kPer], voff_m[kPer], voff_p[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = wave + 4 * k;
    const bool isv = k >= kPer / 2;   // i >= kInstTile exactly when k >= kPer / 2
    const int ii = isv ? i - kInstTile : i;
    dr[k] = ii * kRowsPerInst + lane / kCh;
    dc16[k] = 16 * ((lane % kCh) ^ dual_swz<D>(dr[k]));
    const int rr = kML ? (dr[k] & 15) : dr[k];   // multi-level: row within the 16-row quarter
    voff_m[k] = rr * (isv ? vrowb : krowb) + dc16[k];
    voff_p[k] = dr[k] * (isv ? vprowb : kprowb) + dc16[k];
  }
  auto issue = [&](int t, auto SLOT) __attribute__((always_inline)) {
    constexpr int slot = decltype(SLOT)::value;
    uint8_t* buf = smem + slot * kBufBytes;
    if constexpr (kML) {
      int qsrc[4];
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) qsrc[qd] = __builtin_amdgcn_readfirstlane(ml_quarter(t, qd));
#pragma unroll
      for (int k = 0; k < kPer; ++k) {
        const bool isv = k >= kPer / 2;
        const int i = wave + 4 * k;
        const int ii = isv ? i - kInstTile : i;
        const int qd = (ii * kRowsPerInst) >> 4;   // wave-uniform: kRowsPerInst divides 16
        const int q = qd == 0 ? qsrc[0] : qd == 1 ? qsrc[1] : qd == 2 ? qsrc[2] : qsrc[3];
        dma16(isv ? v_srd : k_srd, buf + i * 1024, voff_m[k],
              __builtin_amdgcn_readfirstlane(q * (isv ? vrowb : krowb)));
      }
      return;
    }
    int kstart, klen;
    tile_keys(t, kstart, klen);
    const bool pooled = kPool && t >= ntm;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const bool isv = k >= kPer / 2;
      const int i = wave + 4 * k;
      const int rowb = pooled ? (isv ? vprowb : kprowb) : (isv ? vrowb : krowb);
      const srd_t sd = pooled ? (isv ? vp_srd : kp_srd) : (isv ? v_srd : k_srd);
      int voff = pooled ? voff_p[k] : voff_m[k];
      if (klen < kT) voff = min(dr[k], klen - 1) * rowb + dc16[k];   // tail: replicate the last key
      dma16(sd, buf + i * 1024, voff, __builtin_amdgcn_readfirstlane(kstart * rowb));
    }
  };

  f32x16 dq[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) dq[i][r] = 0.f;
  const int trr = tr_row(lane), trc = tr_col(lane);
  constexpr int kHi = (kInst + 3) / 4, kLo = kInst / 4;  // DMA instructions per wave and tile
  const bool many = wave < (kInst & 3);

  constexpr bool kSeedQ = D == 64;
  constexpr int kPrioQ = D == 128 ? kDqPrio128 : kDqPrio64;
  f32x16 cD, zero;
#pragma unroll
  for (int r = 0; r < 16; ++r) cD[r] = zero[r] = 0.f;
  int cur_cls = -1;
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  if (ntiles > 0) issue(0, I0{});
  // The body is instantiated once per ring slot, so every LDS address is an immediate offset.
  auto body = [&](int t, auto U) __attribute__((always_inline)) {
    constexpr int u_slot = decltype(U)::value;
    if (t + 1 < ntiles) issue(t + 1, std::integral_constant<int, (u_slot + 1) % kRing>{});
    // retire this wave's part of tile t (tile t+1's stays in flight), then the barrier
    if (t + 1 < ntiles) {
      if (many) VB_WAIT_VMCNT(kHi);
      else VB_WAIT_VMCNT(kLo);
    } else {
      VB_WAIT_VMCNT(0);
    }
    __builtin_amdgcn_s_barrier();
    int kstart, klen;
    float nL;
    bool pooled;
    int cls;   // tile class (wave-uniform): main/pooled, or the multi-level level
    if (kML) {
      klen = ml_klen(t);
      pooled = false;
      cls = ml_lvl(t);
      nL = (float)cls - L1;   // + log2(level): the +ln p logit bias in the exp2 domain
    } else {
      tile_keys(t, kstart, klen);
      pooled = kPool && t >= ntm;
      cls = pooled;
      nL = -(pooled ? L2 : L1);
    }
    const float Dr = pooled ? D2 : D1;
    if (kSeedQ && cls != cur_cls) {   // only where the key source changes: refresh the persistent seeds
      asm volatile("");
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        cD[r] = kSeedQ ? Dr : 0.f;
      }
      cur_cls = cls;
    }
    const uint8_t* kt_ = smem + u_slot * kBufBytes;
    const uint8_t* vt_ = kt_ + kTileBytes;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {   // 32-key halves: S^T, dP^T -> dS^T -> dQ^T
      // dP^T's chain starts from cD = -Delta of the lane's row (dS = P * (dO.V^T - Delta) with no
      // subtraction per score); the seeds are persistent registers read as the MFMA's C operand
      f32x16 s, dp;
      if constexpr (kPrioQ & 1) __builtin_amdgcn_s_setprio(1);
      s = T::mfma32(lds_b128<T>(kt_, dual_off<D>(kt * 32 + l32, half)), qf[0], zero);
#pragma unroll
      for (int ks = 1; ks < KS; ++ks)
        s = T::mfma32(lds_b128<T>(kt_, dual_off<D>(kt * 32 + l32, 2 * ks + half)), qf[ks], s);
      dp = T::mfma32(lds_b128<T>(vt_, dual_off<D>(kt * 32 + l32, half)), df[0], kSeedQ ? cD : zero);
#pragma unroll
      for (int ks = 1; ks < KS; ++ks)
        dp = T::mfma32(lds_b128<T>(vt_, dual_off<D>(kt * 32 + l32, 2 * ks + half)), df[ks], dp);
      if constexpr (kPrioQ & 1) __builtin_amdgcn_s_setprio(0);
      if (klen < kT) {
        asm volatile("");
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool ok = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half < klen;
          const float pr = ok ? exp2_fast(fmaf(s[r], p.c, nL)) : 0.f;
          dp[r] = pr * (kSeedQ ? dp[r] : dp[r] + Dr);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pr = exp2_fast(fmaf(s[r], p.c, nL));
          dp[r] = pr * (kSeedQ ? dp[r] : dp[r] + Dr);
        }
      }
      // dQ^T += K^T.dS^T over (16-key half sb, d tile dt) steps, reads one step ahead (lgkmcnt(2))
      typename T::vec8 pdv[2];
#pragma unroll
      for (int sb = 0; sb < 2; ++sb) pdv[sb] = pack8<T>(dp, 8 * sb);
      constexpr int NST = 2 * DT;
      s16x4 rk[2][2];
      auto rd = [&](int j, int slot) __attribute__((always_inline)) {
        const int rr = kt * 32 + 16 * (j / DT) + trr;
        const int cc = 32 * (j % DT) + trc;
        rk[slot][0] = lds_tr4_asm_at(kt_, dual_off_col<D>(rr, cc));
        rk[slot][1] = lds_tr4_asm_at(kt_, dual_off_col<D>(rr + 8, cc));
      };
      rd(0, 0);
      if constexpr (kPrioQ & 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        const int sl = j & 1;
        if (j + 1 < NST) {
          rd(j + 1, sl ^ 1);
          asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(rk[sl][0]), "+v"(rk[sl][1]));
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(rk[sl][0]), "+v"(rk[sl][1]));
        }
        dq[j % DT] = T::mfma32(join8<T>(rk[sl][0], rk[sl][1]), pdv[j / DT], dq[j % DT]);
      }
      if constexpr (kPrioQ & 2) __builtin_amdgcn_s_setprio(0);
    }
    __builtin_amdgcn_s_barrier();   // slot t % 2 is refilled by the next issue
  };
  for (int t0 = 0; t0 < ntiles; t0 += kRing) {
    body(t0, I0{});
    if (t0 + 1 < ntiles) body(t0 + 1, I1{});
  }

  if (!qvalid) return;
  const float mul = nan_head ? __builtin_nanf("") : p.scale;
  const int64_t orow = p.q_rows ? p.q_rows[g] : qrow0 + g;
  uint8_t* ob = reinterpret_cast<uint8_t*>(p.dq) + 2 * (b * p.dqs[0] + h * p.dqs[1] + orow * p.dqs[2]);
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int d = dt * 32 + 8 * g4 + 4 * half;
      u32x2 w;
      w[0] = pack2<T>(dq[dt][4 * g4 + 0] * mul, dq[dt][4 * g4 + 1] * mul);
      w[1] = pack2<T>(dq[dt][4 * g4 + 2] * mul, dq[dt][4 * g4 + 3] * mul);
      *reinterpret_cast<u32x2*>(ob + d * 2) = w;
    }
}

// sum of the pooled-key gradient partials: dkp = sum_s part[s] (fixed order: deterministic)
__global__ void __launch_bounds__(256) pool_grad_reduce_kernel(const float* pk, const float* pv, int64_t n4, int nsplit,
                                                               float* dk, float* dv) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n4) return;
  f32x4 a = reinterpret_cast<const f32x4*>(pk)[i];
  f32x4 c = reinterpret_cast<const f32x4*>(pv)[i];
  for (int s = 1; s < nsplit; ++s) {
    a += reinterpret_cast<const f32x4*>(pk)[s * n4 + i];
    c += reinterpret_cast<const f32x4*>(pv)[s * n4 + i];
  }
  reinterpret_cast<f32x4*>(dk)[i] = a;
  reinterpret_cast<f32x4*>(dv)[i] = c;
}

// ------------------------------------------------------------------------------------------------
// launchers (vb_attn_bwd.hpp); the host layer is vb_attn_bwd_host.cpp
// ------------------------------------------------------------------------------------------------
int launch_prep(const PrepParams& pp, int dtype, bool joint, hipStream_t s) {
  const int64_t threads = (int64_t)pp.B * pp.H * pp.ntile * 64 * (pp.D / 8);
  const dim3 grid((unsigned)((threads + 255) / 256));
  if (joint) {
    if (dtype == VB_DTYPE_BF16) hipLaunchKernelGGL((bwd_prep_kernel<BF16, true>), grid, dim3(256), 0, s, pp);
    else hipLaunchKernelGGL((bwd_prep_kernel<F16, true>), grid, dim3(256), 0, s, pp);
  } else if (dtype == VB_DTYPE_BF16) hipLaunchKernelGGL(bwd_prep_kernel<BF16>, grid, dim3(256), 0, s, pp);
  else hipLaunchKernelGGL(bwd_prep_kernel<F16>, grid, dim3(256), 0, s, pp);
  return check_launch("bwd_prep_kernel");
}

int launch_dkdv_round3(const BwdParams& p, int D, int dtype, bool pooled, hipStream_t s) {
  const int BH = p.B * p.H;
  const dim3 grid(pooled ? p.nbkp * BH * p.psplit : p.nbk * BH);
  return dispatch_head(D, dtype, [&](auto d, auto t, auto pl) {
    hipLaunchKernelGGL((bwd_dkdv_kernel<d(), decltype(t), pl()>), grid, dim3(bwd::kThreads), 0, s, p);
    return check_launch(pl() ? "bwd_dkdv_kernel<pooled>" : "bwd_dkdv_kernel");
  }, pooled);
}

int launch_ml_dkdv_round3(const BwdParams& p, int D, int dtype, hipStream_t s) {
  return dispatch_head(D, dtype, [&](auto d, auto t) {
    hipLaunchKernelGGL((bwd_dkdv_kernel<d(), decltype(t), false, true>), dim3(p.nbk * p.B * p.H), dim3(bwd::kThreads), 0, s, p);
    return check_launch("bwd_dkdv_kernel<multi-level>");
  });
}

int launch_dq_round3(const BwdParams& p, int D, int dtype, bool pool, hipStream_t s) {
  return dispatch_head(D, dtype, [&](auto d, auto t, auto pl) {
    hipLaunchKernelGGL((bwd_dq_kernel<d(), decltype(t), pl()>), dim3(p.nbq * p.B * p.H), dim3(bwd::kThreads), 0, s, p);
    return check_launch("bwd_dq_kernel");
  }, pool);
}

int launch_ml_dq_round3(const BwdParams& p, int D, int dtype, hipStream_t s) {
  return dispatch_head(D, dtype, [&](auto d, auto t) {
    hipLaunchKernelGGL((bwd_dq_kernel<d(), decltype(t), false, true>), dim3(p.nbq * p.B * p.H), dim3(bwd::kThreads), 0, s, p);
    return check_launch("bwd_dq_kernel<multi-level>");
  });
}

int launch_pool_grad_reduce(const BwdParams& p, int D, hipStream_t s) {
  const int64_t n4 = (int64_t)p.B * p.H * p.Lkp * D / 4;
  hipLaunchKernelGGL(pool_grad_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, p.dkp_part,
                     p.dvp_part, n4, p.psplit, p.dkp, p.dvp);
  return check_launch("pool_grad_reduce_kernel");
}

int launch_ml_pyramid(const BwdParams& p, int D, int dtype, hipStream_t s) {
  return dispatch_head(D, dtype, [&](auto d, auto t) {
    constexpr int kW = d() == 64 ? bwd::kMlPyrWaves : 4, kRows = 32 * kW;   // items of kRows pyramid rows
    int items = 0;
    for (int e = 1; e < 4; ++e) items += ((p.Lpad >> e) + kRows - 1) / kRows;
    hipLaunchKernelGGL((bwd_dkdv_kernel<d(), decltype(t), true, true, kW>), dim3(items * p.B * p.H), dim3(kW * 64), 0, s, p);
    return check_launch("bwd_dkdv_kernel<multi-level pooled>");
  });
}

}  // namespace vb
