// Block-sparse FMHA forward for gfx950 (MI355X), bf16/f16 in, fp32 softmax/accumulate.
//
// Replaces the external block_sparse_attn_func forward (mit-han-lab/Block-Sparse-Attention) as the
// reference calls it (cogvideox/train/special_attentions_local/TrainRelated/cogvideo_blocksparseattn.py:
// 293-324, 106-109) and fuses the pooled-KV branch + LSE combine (:367-393) into the same softmax.
//
// Geometry: one 256-thread workgroup (4 waves) per (b, h, 128-row q-block); each wave owns 32
// query rows. Keys stream through an LDS ring of 64-key tiles (two per kept 128-key mask block,
// then the pooled keys): 2 slots at D=128, 3 at D=64, filled by LDS-DMA (global_load_lds_dwordx4)
// one or two tiles ahead of the tile being read, one barrier per tile.
//
// Per wave and tile:
//   S^T (64 keys x 32 q) = K . Q^T       v_mfma_f32_32x32x16: A = K rows (ds_read_b128 of an
//                                        XOR-swizzled image), B = Q fragment held in VGPRs
//   online softmax in the exp2 domain    query on the lane: row max = in-lane fmax over 32
//                                        values + one v_permlane32_swap
//   O^T (D x 32 q) += V^T . P^T          A = V^T via ds_read_b64_tr_b16 (hardware transpose of the
//                                        row-major, granule-swizzled V image), B = P packed from
//                                        the S^T accumulator registers (no LDS round trip)
// Gilbert reorder: q/k/v rows are gathered through q_rows / kv_rows and O/LSE scattered through
// q_rows, so the reference's index_select + cat + reverse (:141-161) cost no pass of their own.
//
// Layout: the work-item decode and the build constants (namespace fwd) are in vb_attn_fwd.hpp, the
// entry points and their validation in vb_attn_fwd_host.cpp. Here the kept-block list builder and
// the register-only softmax helpers are free functions; attn_fwd_item holds what indexes the LDS ring,
// under the headings "how a tile's source is chosen", "how a tile is issued", "one tile, inference",
// "one tile, training" and "epilogue". Every piece that is still inline there changed some kernel's
// instructions when it was moved out (forward layout).
#include <type_traits>

#include "vb_args.hpp"
#include "vb_attn_fwd.hpp"
#include "vb_trace.hpp"

#ifndef VB_ATTN_TRACE
#define VB_ATTN_TRACE 0   // diagnostic builds only (tools/diag/attn_trace.py): per-workgroup timeline
#endif
#if VB_ATTN_TRACE
namespace vb { __device__ TraceBuf g_attn_trace; }
#define VB_ATRACE_START(k) trace_start(g_attn_trace, k, (unsigned)vblk)
#define VB_ATRACE_END() trace_end(g_attn_trace, (unsigned)vblk)
#else
#define VB_ATRACE_START(k)
#define VB_ATRACE_END()
#endif

namespace vb {

#ifndef VB_LAZY_COUNT
#define VB_LAZY_COUNT 0   // diagnostic builds: count lazy-max slow paths (g_vb_stamp[10]) per tile half ([11])
#endif
#if VB_LAZY_COUNT
__device__ unsigned long long g_vb_stamp[16];
#define VB_LAZY_ADD(slot, n) if (lane == 0) atomicAdd(&g_vb_stamp[slot], n)
#else
#define VB_LAZY_ADD(slot, n)
#endif

// LDS of one attention workgroup: the K/V ring, the kept-block list and its count, and (gathered
// K/V) the kv_rows entry ring
template <int D, bool kKvRows>
constexpr int fwd_smem_bytes() {
  return ((D == 64) ? 3 : 2) * 2 * kKT * D * 2 + kMaxBlocks * 2 + 16 + (kKvRows ? 4 * 512 : 0);
}

// ---- which key blocks a q-block keeps (wave 0; list / list_n in LDS) ---------------------------------
// position of this lane's set bit among the set bits of a wave ballot
__device__ __forceinline__ int ballot_rank(unsigned long long bal) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}
// the kept key blocks of mask row `mrow` (all nbk if dense; none without the main branch), ascending
__device__ __forceinline__ void build_kept_list(const uint8_t* mrow, bool dense, bool use_main, int nbk, int qblk,
                                                int lane, uint16_t* list, int* list_n) {
  int n = 0;
  int dpos = -1;   // list position of the diagonal block (key block qblk), if kept
  if (use_main) {
    for (int j0 = 0; j0 < nbk; j0 += 64) {
      const int j = j0 + lane;
      const bool keep = (j < nbk) && (dense || mrow[j] != 0);
      const unsigned long long bal = __ballot(keep);
      if (keep) {
        const int pos = n + ballot_rank(bal);
        list[pos] = (uint16_t)j;
        if (j == qblk) dpos = pos;
      }
      n += __popcll(bal);
    }
    // Diagonal block first: in the Gilbert order a q-block's own key block usually holds its
    // largest scores, so the running max is set once on the first tile (fewer rescales; the
    // lazy-max launches rarely leave their fast path). Placement only: same sum, other order.
    // The last key block keeps its place (a half-empty tail tile must stay the last tile).
    const unsigned long long db = __ballot(dpos > 0);
    if (db != 0 && qblk != nbk - 1) {
      const int dp = __builtin_amdgcn_readlane(dpos, (int)__builtin_ctzll(db));
      if (lane == 0) {
        const uint16_t t = list[0];
        list[0] = (uint16_t)qblk;
        list[dp] = t;
      }
    }
  }
  if (lane == 0) *list_n = n;
}

// ---- softmax helpers on one 32-key half of S^T (this lane's 16 values; registers only) --------------
// row max: 7 v_max3 + 1 v_max
__device__ __forceinline__ float half_max(const f32x16& x) {
  const float a = max3f(max3f(max3f(x[0], x[1], x[2]), x[3], x[4]), x[5], x[6]);
  const float c = max3f(max3f(max3f(x[8], x[9], x[10]), x[11], x[12]), x[13], x[14]);
  return max3f(a, c, fmaxf(x[7], x[15]));
}
// P = exp2(S) packed to the storage type (the PV operands of k-steps 2kt, 2kt+1) WITHOUT
// overwriting S; returns the lane's fp32 sum (four independent chains)
template <class T, int kPrio>
__device__ __forceinline__ float exp_pack(const f32x16& x, typename T::vec8& p0, typename T::vec8& p1) {
  float e[16];
  float h4[4];
  if constexpr (kPrio & 4) __builtin_amdgcn_s_setprio(1);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    e[r] = exp2_fast(x[r]);
    h4[r & 3] = r < 4 ? e[r] : h4[r & 3] + e[r];   // chains start at their first value (no 0 + e)
  }
  u32x4 u0, u1;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    u0[w] = pack2<T>(e[2 * w], e[2 * w + 1]);
    u1[w] = pack2<T>(e[8 + 2 * w], e[8 + 2 * w + 1]);
  }
  p0 = __builtin_bit_cast(typename T::vec8, u0);
  p1 = __builtin_bit_cast(typename T::vec8, u1);
  if constexpr (kPrio & 4) __builtin_amdgcn_s_setprio(0);
  return (h4[0] + h4[1]) + (h4[2] + h4[3]);
}

// Persistent dispatch (vb_attn_args.work_queue; vb_common.hpp): the launch is resident-sized and
// every workgroup pulls work items from per-XCD queue heads. Item v (a "virtual blockIdx" in [0,
// total)) belongs to queue v % 8, in increasing v: the same items, in the same per-XCD order, as one
// workgroup per item dealt round-robin over the XCDs. A workgroup drains its own XCD's queue (w % 8
// shares an XCD, like blockIdx % 8 of the one-per-item grid), then takes the remaining items of the
// other queues, so no XCD idles while another still has work.

// One work item: the (b, h, 128-row q-block) of virtual blockIdx `vblk`. With a work queue, lane 0
// of wave 0 claims the workgroup's next item after the tile loop (`next`), so the claim's round
// trip overlaps the epilogue.
// kCBias selects the tile body. true = inference launches (no LSE output): the S accumulator starts
// at (bias - m) instead of 0 and Q is pre-scaled by scale*log2(e), so every score leaves the MFMA as
// the exp2 argument itself (no per-score v_fma before the v_exp: the D=64 loop is VALU-issue-bound),
// and the running max is lazy ("one tile, inference"). The extra rounding of q*scale to 16 bits stays
// within the stated tolerance. false = launches that return the LSE for a backward: they keep the
// unscaled Q, so forward and backward see the same scores, and take every tile's row max ("one tile,
// training").
template <int D, class T, bool kPool, bool kKvRows, bool kML, bool kCBias, bool kWQ>
__device__ __forceinline__ void attn_fwd_item(const FwdParams& p, const int vblk, int& next) {
  constexpr int KS = D / 16;                   // k-steps of the QK^T product
  constexpr int DT = D / 32;                   // 32-wide d tiles of the output
  constexpr bool kSplitPV = fwd::split_pv(D);
  // s_setprio around the MFMA chains of the inference loop: with two waves per SIMD (D=128) the wave
  // in its MFMA phase keeps the matrix pipe fed while the other runs its softmax VALU (Wan +4 %);
  // the LSE-returning loop and the 3-wave D=64 kernel measured slower with it
  constexpr int kPrio = !kCBias ? 0 : D == 64 ? fwd::kPrio64 : fwd::kPrio128;
  constexpr float kLazyBound = std::is_same<T, BF16>::value ? kLazyBoundBF16 : kLazyBoundF16;
  constexpr int kRowB = D * 2;                 // bytes per key row
  constexpr int kMatBytes = kKT * kRowB;       // one 64-key K (or V) tile
  constexpr int kBufBytes = 2 * kMatBytes;     // K image then V image
  constexpr int kBufs = (D == 64) ? 3 : 2;     // LDS ring: tile t read, t+1 (and t+2) in flight
  constexpr int kChunks = kRowB / 16;          // 16-byte chunks per row
  constexpr int kRowsPerInst = 1024 / kRowB;   // rows one 1-KiB LDS-DMA wave-instruction fills
  constexpr int kInstPerMat = kMatBytes / 1024;
  constexpr int kInstPerWave = 2 * kInstPerMat / 4;
  // declared here, not passed in from the kernel: hipcc's waitcnt pass then still sees which LDS
  // bytes each LDS-DMA writes and each read reads (through a pointer parameter it puts a vmcnt wait,
  // draining the ring, in front of every LDS read of the loop)
  __shared__ __attribute__((aligned(16))) uint8_t smem[fwd_smem_bytes<D, kKvRows>()];
  static_assert(fwd_smem_bytes<D, kKvRows>() == kBufs * kBufBytes + kMaxBlocks * 2 + 16 + (kKvRows ? 4 * 512 : 0), "LDS layout");
  static_assert(!(kML && (kPool || kKvRows)), "multi-level mode reads the KV pyramids only");
  uint16_t* list = reinterpret_cast<uint16_t*>(smem + kBufs * kBufBytes);
  int* list_n = reinterpret_cast<int*>(smem + kBufs * kBufBytes + kMaxBlocks * 2);

  // Persistent launches (kWQ) launder the thread id per item: otherwise the item loop hoists the
  // lane-derived addresses (DMA chunks, LDS fragment bases) out of it and spills them across it.
  // The mask keeps its range known (0..255), so hipcc's waitcnt pass still separates a ring slot's
  // LDS-DMA from the reads of another slot.
  int tid = threadIdx.x;
  if constexpr (kWQ) {
    asm volatile("" : "+v"(tid));
    tid &= kThreads - 1;
  }
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int half = lane >> 5;
  const int l32 = lane & 31;

  VB_ATRACE_START(0);
  int qblk, bh;
  fwd_item_decode(p, vblk, bh, qblk);
  const int b = bh / p.H, h = bh % p.H;

  int Lq = p.Lq, Lk = p.Lk;
  int64_t qrow0 = 0, krow0 = 0;
  if (p.cu_q) {
    qrow0 = p.cu_q[b];
    Lq = p.cu_q[b + 1] - p.cu_q[b];
    krow0 = p.cu_k[b];
    Lk = p.cu_k[b + 1] - p.cu_k[b];
  }
  const int q0 = qblk * kQBlk;
  if (q0 >= Lq) return;
  const int nbk = (Lk + kQBlk - 1) / kQBlk;

  // ---- which key blocks this q-block keeps ------------------------------------------------------
  const uint8_t* mrow = nullptr;
  bool dense = true;
  bool nan_head = false;
  if (p.use_main) {
    const uint8_t* mh = head_mask_base(p.mask, p.ms, p.head_mask_type, p.H, b, h, nan_head, p.hm_mode);
    if (mh) {
      dense = false;
      mrow = mh + (int64_t)qblk * p.ms[2];
    }
  }
  if (kML) {
    // multi-level: per-level lists of key blocks (levels 1, 2, 4, 8, in that order), built in two
    // passes over the mask row (counts, then positions) so they share the one kMaxBlocks array.
    if (tid < 64) {
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
      if (lane < 4) list_n[lane] = cnt[0] * (lane == 0) + cnt[1] * (lane == 1) + cnt[2] * (lane == 2) + cnt[3] * (lane == 3);
    }
  } else if (tid < 64) {
    build_kept_list(mrow, dense, p.use_main, nbk, qblk, lane, list, list_n);
  }

  // ---- Q fragment (B operand of S^T = K.Q^T): row l32 of this wave, d = 16s + 8*half + j --------
  const int qg = q0 + wave * 32 + l32;               // reordered query position
  const bool qvalid = qg < Lq;
  int qrow = qvalid ? qg : Lq - 1;
  if (p.q_rows) qrow = p.q_rows[qrow];
  const uint8_t* qbase = reinterpret_cast<const uint8_t*>(p.q) + 2 * (b * p.qs[0] + h * p.qs[1] + qrow0 * p.qs[2]);
  typename T::vec8 qf[KS];
  auto load_q = [&]() __attribute__((always_inline)) {
    const uint8_t* qp = qbase + (int64_t)qrow * 2 * p.qs[2];
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[s] = *reinterpret_cast<const typename T::vec8*>(qp + (16 * s + 8 * half) * 2);
    if constexpr (kCBias) {
      // scores in the exp2 domain straight out of the MFMA: Q carries the softmax scale * log2(e)
      // (one extra rounding of q to the storage type; the stated tolerance covers it)
#pragma unroll
      for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[s][e] = T::from_f32(T::to_f32(qf[s][e]) * p.c);
    }
    // Launder the Q fragment through an empty asm: the loop's MFMAs then depend on the asm, not
    // on the global loads, so hipcc's waitcnt pass does not count them against the DMA ring.
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(qf[s]));
  };
  // kQLate: the Q fragment is loaded after the ring's first DMAs are issued (below), so its round
  // trip and theirs overlap; only the q_rows entry (issued above) and the mask row precede the
  // barrier. Otherwise Q is loaded first and retired before the DMA ring starts.
  constexpr bool kQLate = D == 64 ? fwd::kQLate64 : (kCBias && !kKvRows) ? fwd::kQLate128Lazy : fwd::kQLate128;
  if constexpr (kQLate) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // wave 0's list writes
    __builtin_amdgcn_s_barrier();                           // kept-block list visible
    asm volatile("" ::: "memory");
  } else {
    load_q();
    __syncthreads();
  }
  const int nkept = __builtin_amdgcn_readfirstlane(*list_n);
  // main tiles: two 64-key halves per kept block, minus an empty second half of the last block
  int ntm = 2 * nkept;
  if (nkept > 0 && list[nkept - 1] == nbk - 1 && (nbk - 1) * kQBlk + kKT >= Lk && !(kML && p.ref_tail)) ntm -= 1;
  const int ntp = kPool ? (p.Lkp + kKT - 1) / kKT : 0;
  // multi-level tiles (64 pyramid rows, one level each): level 1 as above, one tile per level-2
  // block, two level-4 blocks and four level-8 blocks per tile (a short last tile is masked)
  int n2 = 0, n4 = 0, n8 = 0, T12 = 0, T124 = 0;
  if (kML) {
    n2 = __builtin_amdgcn_readfirstlane(list_n[1]);
    n4 = __builtin_amdgcn_readfirstlane(list_n[2]);
    n8 = __builtin_amdgcn_readfirstlane(list_n[3]);
    T12 = ntm + n2;
    T124 = T12 + (n4 + 1) / 2;
  }
  const int ntiles = kML ? T124 + (n8 + 3) / 4 : ntm + ntp;

  const uint8_t* kbase = reinterpret_cast<const uint8_t*>(p.k) + 2 * (b * p.ks[0] + h * p.ks[1] + krow0 * p.ks[2]);
  const uint8_t* vbase = reinterpret_cast<const uint8_t*>(p.v) + 2 * (b * p.vs[0] + h * p.vs[1] + krow0 * p.vs[2]);
  const uint8_t* kpbase = nullptr;
  const uint8_t* vpbase = nullptr;
  if (kPool) {
    kpbase = reinterpret_cast<const uint8_t*>(p.kp) + 2 * (b * p.kps[0] + h * p.kps[1]);
    vpbase = reinterpret_cast<const uint8_t*>(p.vp) + 2 * (b * p.vps[0] + h * p.vps[1]);
  }

  // ---- how a tile's source is chosen --------------------------------------------------------------
  // where tile t's keys come from; `blk_raw` = list[t >> 1] (read ahead by the caller)
  auto tile_src = [&](int t, int blk_raw) __attribute__((always_inline)) -> TileSrc {
    TileSrc s;
    if (t < ntm) {
      const int blk = __builtin_amdgcn_readfirstlane(blk_raw);  // provably wave-uniform
      s.pooled = 0;
      s.kstart = blk * kQBlk + (t & 1) * kKT;
      s.klen = min(kKT, Lk - s.kstart);
    } else {
      s.pooled = 1;
      s.kstart = (t - ntm) * kKT;
      s.klen = min(kKT, p.Lkp - s.kstart);
    }
    return s;
  };

  // multi-level: pyramid rows of tile t's two quarters for this wave's half (packed block ids `raw`
  // from ml_list_at, read one tile ahead like list_at)
  const int off4 = p.Lpad + p.Lpad / 2, off8 = off4 + p.Lpad / 4;
  const int my_half = (wave & 1) * 32;
  auto ml_tile_src = [&](int t, int raw) __attribute__((always_inline)) -> MlTileSrc {
    MlTileSrc s;
    const int a = __builtin_amdgcn_readfirstlane(raw & 0xFFFF);
    const int c = __builtin_amdgcn_readfirstlane(raw >> 16);
    if (t < ntm) {
      const int kstart = a * kQBlk + (t & 1) * kKT;
      s.srcA = kstart + my_half;
      s.klen = p.ref_tail ? kKT : min(kKT, Lk - kstart);
      s.lvl = 0;
    } else if (t < T12) {
      s.srcA = p.Lpad + a * 64 + my_half;
      s.klen = kKT;
      s.lvl = 1;
    } else if (t < T124) {
      s.srcA = off4 + a * 32;
      s.klen = min(kKT, (n4 - 2 * (t - T12)) * 32);
      s.lvl = 2;
    } else {
      s.srcA = off8 + a * 16;
      s.klen = min(kKT, (n8 - 4 * (t - T124)) * 16);
      s.lvl = 3;
    }
    s.srcB = (t >= T124) ? off8 + c * 16 : s.srcA + 16;
    return s;
  };
  auto ml_list_at = [&](int t) __attribute__((always_inline)) -> int {
    int e0, e1;
    if (t < ntm) {
      e0 = e1 = t >> 1;
    } else if (t < T12) {
      e0 = e1 = nkept + (t - ntm);
    } else if (t < T124) {
      e0 = e1 = nkept + n2 + min(2 * (t - T12) + (wave & 1), n4 - 1);
    } else {
      const int e = 4 * (t - T124) + 2 * (wave & 1);
      e0 = nkept + n2 + n4 + min(e, n8 - 1);
      e1 = nkept + n2 + n4 + min(e + 1, n8 - 1);
    }
    e0 = min(max(e0, 0), kMaxBlocks - 1);
    e1 = min(max(e1, 0), kMaxBlocks - 1);
    return (int)list[e0] | ((int)list[e1] << 16);
  };

  // ---- how a tile is issued -------------------------------------------------------------------------
  // Tile t -> LDS ring slot t % kBufs by LDS-DMA (global_load_lds_dwordx4, 1 KiB per
  // wave-instruction, written linearly). The images' XOR swizzles (k_off / v_off_bytes) are
  // applied to each lane's SOURCE chunk instead: LDS slot `sl` of row r holds the chunk that
  // k_off / v_off_bytes would have placed there. Every wave fills ONE matrix: waves 0-1 -> K,
  // waves 2-3 -> V (kInstPerWave*2 == kInstPerMat).
  static_assert(2 * kInstPerWave == kInstPerMat, "DMA split assumes two waves per matrix");
  const int my_mat = wave >> 1;
  const uint8_t* my_base = my_mat == 0 ? kbase : vbase;
  const int64_t my_stride = 2 * (my_mat == 0 ? p.ks[2] : p.vs[2]);
  const uint8_t* my_pbase = my_mat == 0 ? kpbase : vpbase;
  const int64_t my_pstride = kPool ? 2 * (my_mat == 0 ? p.kps[2] : p.vps[2]) : 0;
  // source chunk of every DMA lane (fixed: the image row of lane L is a function of L only)
  int my_chunk[kInstPerWave];
  int my_row[kInstPerWave];
#pragma unroll
  for (int i = 0; i < kInstPerWave; ++i) {
    const int mi = (wave & 1) * kInstPerWave + i;
    const int r = mi * kRowsPerInst + lane / kChunks;
    const int sl = lane % kChunks;
    my_row[i] = r;
    if (my_mat == 0) {
      my_chunk[i] = sl ^ ((D == 64) ? ((r >> 1) & 7) : (r & 15));
    } else {
      const int vsw = (D == 64) ? ((r >> 1) & 1) : (r & 3);
      my_chunk[i] = (((sl >> 2) ^ vsw) << 2) | (sl & 3);
    }
  }
  // Buffer descriptors of this wave's matrix for the (b,h) slice (main and pooled keys): the DMA
  // then needs no 64-bit per-lane address math — the lane's fixed part (row within the tile,
  // source chunk) is a precomputed 32-bit voffset and the tile's first key a scalar soffset.
  // The host guarantees every slice spans < 2^31 bytes.
  const int my_rowb = (int)my_stride;
  const int my_prowb = (int)my_pstride;
  const int src_rows = kML ? 15 * (p.Lpad / 8) : Lk;   // pyramid rows in multi-level mode
  const srd_t my_rsrc = make_srd(my_base, p.use_main ? (int)((int64_t)(src_rows - 1) * my_stride + kRowB) : 0);
  const srd_t my_prsrc = make_srd(kPool ? my_pbase : my_base, kPool ? (int)((int64_t)(p.Lkp - 1) * my_pstride + kRowB) : 0);
  // multi-level: per-lane voffsets, rows relative to the instruction's 16-row quarter (its start
  // is the soffset). Otherwise only the swizzled chunk is kept per instruction: instruction i's
  // row is my_row0 + i*kRowsPerInst, so its voffset is my_row0*rowb + chunk (one VALU per tile and
  // instruction) and the i*kRowsPerInst*rowb part goes to the scalar soffset. Fewer live VGPRs
  // than one offset per instruction and key source (a spilled one stalled the D=128 DMA ring).
  int my_voff[kInstPerWave];
  int my_rc[kInstPerWave];
  const int my_row0 = my_row[0];
#pragma unroll
  for (int i = 0; i < kInstPerWave; ++i) {
    my_rc[i] = my_chunk[i] * 16;
    if constexpr (kML) my_voff[i] = (my_row[i] & 15) * my_rowb + my_chunk[i] * 16;
  }
  // Persistent launches (kWQ) issue every K/V DMA through dma16_unscoped: the DMAs stay invisible to
  // hipcc's LDS-DMA waits across the item loop (persistent dispatch)
  auto ml_issue = [&](const MlTileSrc src, int slot) __attribute__((always_inline)) {
    uint8_t* dst = smem + slot * kBufBytes + my_mat * kMatBytes + (wave & 1) * kInstPerWave * 1024;
    const int soffA = __builtin_amdgcn_readfirstlane(src.srcA * my_rowb);
    const int soffB = __builtin_amdgcn_readfirstlane(src.srcB * my_rowb);
#pragma unroll
    for (int i = 0; i < kInstPerWave; ++i)
      if constexpr (kWQ) dma16_unscoped(my_rsrc, dst + i * 1024, my_voff[i], (i * kRowsPerInst >= 16) ? soffB : soffA);
      else dma16(my_rsrc, dst + i * 1024, my_voff[i], (i * kRowsPerInst >= 16) ? soffB : soffA);
  };
  // Gathered K/V rows (kv_rows: reordered key -> caller row; the module's path on the caller's own
  // k/v). Per tile every wave DMAs the kv_rows entries of its own 32 rows into a 4-slot LDS ring
  // one DMA stage ahead of the rows themselves (lane 32 lanes, entry j*kIPW + i = the row of DMA
  // instruction i for lanes with row j), reads its kIPW entries back with one or two ds_read_b128
  // and issues the row DMAs with per-lane voffsets row * stride + chunk (v_mad_u32_u24). Every
  // body issues one offset DMA and kIPW row DMAs, past the last tile too, so the vmcnt counts are
  // constants (see the body).
  const int gather_key = ((wave & 1) * kInstPerWave + (lane % kInstPerWave)) * kRowsPerInst + lane / kInstPerWave;
  const srd_t rows_srd = make_srd(kKvRows ? p.kv_rows : nullptr, kKvRows ? Lk * 4 : 0);
  uint8_t* const ibase = smem + kBufs * kBufBytes + kMaxBlocks * 2 + 16 + wave * 128;   // [4][4 waves][32]
  auto issue_idx = [&](int t, int blk_raw) __attribute__((always_inline)) {
    int voff = 0;   // pooled tiles and tiles past the end: a harmless entry
    if (t < ntm) {
      const int kstart = __builtin_amdgcn_readfirstlane(blk_raw) * kQBlk + (t & 1) * kKT;
      voff = 4 * (kstart + min(gather_key, min(kKT, Lk - kstart) - 1));
    }
    if (lane < 32) {
      uint8_t* dst = ibase + (t & 3) * 512;
      if constexpr (kWQ) {   // as dma16_unscoped
        uint32_t a = __builtin_amdgcn_readfirstlane(
            static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)dst)));
        asm("" : "+s"(a));
        dst = (uint8_t*)(__attribute__((address_space(3))) uint8_t*)(uintptr_t)a;
      }
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(rows_srd.base), (short)0, rows_srd.bytes, 0x00020000),
          (__attribute__((address_space(3))) void*)dst, 4, voff, 0, 0, 0);
    }
  };
  auto issue = [&](const TileSrc src, int slot, int t = 0) __attribute__((always_inline)) {
    uint8_t* dst = smem + slot * kBufBytes + my_mat * kMatBytes + (wave & 1) * kInstPerWave * 1024;
    // this wave's i-th 1 KiB piece of the tile
    auto piece = [&](int i, srd_t sd, int voff, int soff) __attribute__((always_inline)) {
      if constexpr (kWQ) dma16_unscoped(sd, dst + i * 1024, voff, soff);
      else dma16(sd, dst + i * 1024, voff, soff);
    };
    const bool pooled = kPool && src.pooled;
    if (kKvRows && !pooled) {
      typedef int i32x4 __attribute__((ext_vector_type(4)));
      int o[kInstPerWave];
      const uint8_t* ib = ibase + (t & 3) * 512 + 4 * kInstPerWave * (lane / kChunks);
#pragma unroll
      for (int c = 0; c < kInstPerWave; c += 4) {
        const i32x4 w = *reinterpret_cast<const i32x4*>(ib + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[c + e] = w[e];
      }
#pragma unroll
      for (int i = 0; i < kInstPerWave; ++i) {
        int voff;   // row * stride + chunk: rows < 2^24 and strides < 2^24 bytes (host-checked)
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(voff) : "v"(o[i]), "s"(my_rowb), "v"(my_chunk[i] * 16));
        piece(i, my_rsrc, voff, 0);
      }
      return;
    }
    const int rowb = pooled ? my_prowb : my_rowb;
    const int soff = __builtin_amdgcn_readfirstlane(src.kstart * rowb);
    if (src.klen == kKT) {
      // 24-bit multiply (full rate; v_mul_lo_u32 is a quarter-rate op on every tile): the row is
      // < 64 and the host rejects row strides of 2^24 bytes or more
      const int vb0 = (int)__umul24((unsigned)my_row0, (unsigned)rowb);
#pragma unroll
      for (int i = 0; i < kInstPerWave; ++i)
        piece(i, pooled ? my_prsrc : my_rsrc, vb0 + my_rc[i], __builtin_amdgcn_readfirstlane(soff + i * kRowsPerInst * rowb));
    } else {   // tail tile: clamp rows to the last valid key (replicated rows are masked later)
#pragma unroll
      for (int i = 0; i < kInstPerWave; ++i) {
        const int r = min(my_row0 + i * kRowsPerInst, src.klen - 1);
        piece(i, pooled ? my_prsrc : my_rsrc, r * rowb + my_rc[i], soff);
      }
    }
  };

  // ---- running state of this lane's query row -------------------------------------------------------
  f32x16 o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[i][r] = 0.f;
  float m = kCBias ? 0.f : -INFINITY;  // running max (exp2 domain)
  float l = 0.f;        // running partial row sum (this half's keys)
  // inference only: cb = cur_bias - m in every register (the first QK^T MFMA's C operand); `first`
  // makes the first tile set m from its own maximum
  f32x16 cb;
#pragma unroll
  for (int r = 0; r < 16; ++r) cb[r] = 0.f;
  int cur_bias_bits = 0;   // bit pattern of the bias folded into cb (0.0f)
  bool first = true;

  const int vrow = 4 * half + (lane & 15) / 4;
  const int vcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  // Loop-invariant per-lane LDS addresses: the images' XOR swizzles depend only on the lane's own
  // row bits (K: row l32 [+32 kt]; V: row vrow [+16 k + 8]), so every K/V fragment read of every
  // tile and ring slot is one of these bases plus a compile-time immediate offset.
  int k_lane[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) k_lane[ks] = k_off<D>(l32, 2 * ks + half);
  uint32_t v_lane[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt)
    v_lane[dt] = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(
                     (__attribute__((address_space(3))) const uint8_t*)smem)) +
                 v_off_bytes<D>(vrow, dt * 32 + vcol);

  // One 64-key tile in ring slot U: S^T = K.Q^T, online softmax, O^T += V^T.P^T.
  // bias_bits: the tile's logit bias (exp2 domain) as a bit pattern, chosen by the caller with scalar
  // selects (a float select would be a v_cndmask + v_readfirstlane on every tile)
  auto tile_step = [&](auto U, int bias_bits, int klen) __attribute__((always_inline)) {
    constexpr int kSlot = decltype(U)::value;
    const uint8_t* kl = smem + kSlot * kBufBytes;
    const float bias = __int_as_float(bias_bits);
    f32x16 s[2];
    // V^T fragments (ds_read_b64_tr_b16) for the first VPRE k-steps, issued before the softmax
    // VALU so they land while it runs; the rest are fetched one k-step ahead inside the PV loop.
    constexpr int VPRE = D == 64 ? (kKvRows ? fwd::kVPre64Rows : fwd::kVPre64) : 2;
    s16x4 vlo[4][DT], vhi[4][DT];
    auto read_v = [&](int kk) __attribute__((always_inline)) {
      const int row0 = (kk >> 1) * 32 + 16 * (kk & 1);   // + vrow (in v_lane)
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        vlo[kk][dt] = lds_tr4_asm(v_lane[dt], kSlot * kBufBytes + kMatBytes + row0 * kRowB);
        vhi[kk][dt] = lds_tr4_asm(v_lane[dt], kSlot * kBufBytes + kMatBytes + (row0 + 8) * kRowB);
      }
    };
    auto wait_v = [&](int kk) __attribute__((always_inline)) {
#pragma unroll
      for (int dt = 0; dt < DT; ++dt)
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vlo[kk][dt]), "+v"(vhi[kk][dt]));
    };
    // k-step kk (16 keys) of O^T += V^T . P^T: its V^T fragments have landed and those VPRE k-steps
    // ahead are fetched (next_v), then its MFMAs on the packed P (pv)
    auto next_v = [&](int kk) __attribute__((always_inline)) {
      wait_v(kk);
      if (kk + VPRE < 4) read_v(kk + VPRE);
    };
    auto pv = [&](int kk, const typename T::vec8& pf) __attribute__((always_inline)) {
      if constexpr (kPrio & 2) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) o[dt] = T::mfma32(join8<T>(vlo[kk][dt], vhi[kk][dt]), pf, o[dt]);
      if constexpr (kPrio & 2) __builtin_amdgcn_s_setprio(0);
    };
    // keys of half kt at or past klen -> -inf (tail tiles)
    auto mask_tail = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half >= klen) s[kt][r] = -INFINITY;
    };
    // S^T = seed + K.Q^T of both halves
    auto scores = [&](const f32x16& seed) __attribute__((always_inline)) {
      if constexpr (kPrio & 1) __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) {
        typename T::vec8 kf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) kf[ks] = lds_b128<T>(kl + kt * 32 * kRowB, k_lane[ks]);
        s[kt] = T::mfma32(kf[0], qf[0], seed);
#pragma unroll
        for (int ks = 1; ks < KS; ++ks) s[kt] = T::mfma32(kf[ks], qf[ks], s[kt]);
      }
      if constexpr (kPrio & 1) __builtin_amdgcn_s_setprio(0);
    };

    // ---- one tile, inference (kCBias): lazy running max ---------------------------------------------
    // The first tile takes its exact row max; after that no per-tile max is computed: P = exp2(S - m)
    // uses the standing m, and the row sum of each half-tile (>= each of its P) is checked against
    // kLazyBound. A passing check bounds every P, and so O and l, far from overflow. P is packed into
    // separate registers, so S survives the exp: a failing check (rare, wave-uniform) raises m to the
    // rows' max of that S, rescales O and l, and redoes the exp. m never exceeds the true running
    // max, so l >= 1 after the first tile, and P's bf16 rounding is relative: the result equals the
    // exact-max form up to rounding.
    if constexpr (kCBias) {
      // wave-uniform; only where the tile source changes (pooled, levels). Compared as bit patterns
      // in SGPRs (a scalar compare; a float compare would run on the VALU every tile)
      if (bias_bits != cur_bias_bits) {
        asm volatile("");
        const float db = bias - __int_as_float(cur_bias_bits);
#pragma unroll
        for (int r = 0; r < 16; ++r) cb[r] += db;
        cur_bias_bits = bias_bits;
      }
      // raise m by the rows' max mt of S (if > 0), rescaling O, l, the C seed and the S halves >= kt0
      // (a half whose P is already in O is dead: touching it would keep it live)
      auto raise_m = [&](float mt, auto KT0) __attribute__((always_inline)) {
        constexpr int kt0 = decltype(KT0)::value;
        const float delta = fmaxf(max_xor32(mt), 0.f);
        const float alpha = exp2_fast(-delta);
        m += delta;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          cb[r] -= delta;
          if (kt0 == 0) s[0][r] -= delta;
          s[1][r] -= delta;
        }
      };
      scores(cb);
#pragma unroll
      for (int kk = 0; kk < VPRE; ++kk) read_v(kk);
      if (klen < kKT) {   // tail tile only; the volatile asm keeps it a real (wave-uniform) branch
        asm volatile("");
        mask_tail(0);
        mask_tail(1);
      }
      if (first) {
        asm volatile("");
        const float mt = max_xor32(fmaxf(half_max(s[0]), half_max(s[1])));
        m += mt;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[0][r] -= mt;
          s[1][r] -= mt;
          cb[r] -= mt;
        }
        first = false;
      }
      typename T::vec8 pf[4];
      if constexpr (kSplitPV) {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
          float hs = exp_pack<T, kPrio>(s[kt], pf[2 * kt], pf[2 * kt + 1]);
          if (!__all(hs <= kLazyBound)) {
            asm volatile("");
            VB_LAZY_ADD(10, 1ull);
            // O and l already hold the first half's P when kt = 1: they are rescaled with the rest
            if (kt == 0) raise_m(half_max(s[0]), std::integral_constant<int, 0>{});
            else raise_m(half_max(s[1]), std::integral_constant<int, 1>{});
            hs = exp_pack<T, kPrio>(s[kt], pf[2 * kt], pf[2 * kt + 1]);
          }
          l += hs;
#pragma unroll
          for (int kk = 2 * kt; kk < 2 * kt + 2; ++kk) {
            next_v(kk);
            pv(kk, pf[kk]);
          }
        }
      } else {
        float h0 = exp_pack<T, kPrio>(s[0], pf[0], pf[1]);
        float h1 = exp_pack<T, kPrio>(s[1], pf[2], pf[3]);
        if (!__all(fmaxf(h0, h1) <= kLazyBound)) {
          asm volatile("");
          VB_LAZY_ADD(10, 1ull);
          raise_m(fmaxf(half_max(s[0]), half_max(s[1])), std::integral_constant<int, 0>{});
          h0 = exp_pack<T, kPrio>(s[0], pf[0], pf[1]);
          h1 = exp_pack<T, kPrio>(s[1], pf[2], pf[3]);
        }
        l += h0 + h1;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          next_v(kk);
          pv(kk, pf[kk]);
        }
      }
      VB_LAZY_ADD(11, kSplitPV ? 2ull : 1ull);
    }

    // ---- one tile, training (!kCBias: the launch returns the LSE): every tile's row max -------------
    // S holds the raw scores (unscaled Q, accumulator from 0); P = exp2(S * c + bias - m).
    if constexpr (!kCBias) {
      f32x16 zero;
#pragma unroll
      for (int r = 0; r < 16; ++r) zero[r] = 0.f;
      scores(zero);
#pragma unroll
      for (int kk = 0; kk < VPRE; ++kk) read_v(kk);
      if (klen < kKT) {   // tail tile, as above; written out (through mask_tail the listing changes)
        asm volatile("");
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half >= klen) s[kt][r] = -INFINITY;
      }
      // row max: four independent chains (short dependency chains, max3-friendly)
      float mq[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) {   // 16 v_max3 for 32 values (the minimum), depth 6
        const f32x16& x = s[c >> 1];
        const int o = 8 * (c & 1);
        mq[c] = max3f(max3f(max3f(x[o], x[o + 1], x[o + 2]), x[o + 3], x[o + 4]), x[o + 5], x[o + 6]);
      }
      const float f1 = max3f(mq[0], mq[1], s[0][7]);
      const float f2 = max3f(mq[2], mq[3], s[0][15]);
      float mt = max3f(max3f(f1, f2, s[1][7]), s[1][15], s[1][15]);
      mt = max_xor32(mt) * p.c + bias;       // tile row max, exp2 domain
      // Deferred rescale (guide T13): the running max m is raised only when some row's tile max
      // exceeds it by more than kRescaleSlack (log2 units), so P = exp2(s - m) <= 2^kRescaleSlack.
      // O and l always share the same m, so the result is exact up to rounding; without the slack
      // nearly every tile of a 32-row wave rescales (some row's max grows), a 40-VALU O-wide pass.
      // The empty volatile asm keeps hipcc from if-converting this block into every iteration.
      if (!__all(mt <= m + fwd::kRescaleSlack)) {
        asm volatile("");
        const float mn = fmaxf(m, mt);
        const float alpha = exp2_fast(m - mn);
        m = mn;
        l *= alpha;
#pragma unroll
        for (int i = 0; i < DT; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[i][r] *= alpha;
      }
      const float nbias = bias - m;
      float lq[4] = {0.f, 0.f, 0.f, 0.f};   // four independent partial sums
      if constexpr (kSplitPV) {
        // exp of the first 32 keys, their P.V k-steps, then the second 32: the PV MFMAs of the first
        // half overlap the second half's exp VALU (same sums, same order: bit-identical results)
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float e = exp2_fast(fmaf(s[kt][r], p.c, nbias));
            s[kt][r] = e;
            lq[(2 * kt + r) & 3] = (kt == 0 && r < 4) ? e : lq[(2 * kt + r) & 3] + e;   // no 0 + e
          }
#pragma unroll
          for (int kk = 2 * kt; kk < 2 * kt + 2; ++kk) {
            wait_v(kk);
            if (kk + VPRE < 4) read_v(kk + VPRE);
            const typename T::vec8 pf = pack8<T>(s[kk >> 1], 8 * (kk & 1));
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = T::mfma32(join8<T>(vlo[kk][dt], vhi[kk][dt]), pf, o[dt]);
          }
        }
        l += (lq[0] + lq[1]) + (lq[2] + lq[3]);
      } else {
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float e = exp2_fast(fmaf(s[kt][r], p.c, nbias));
            s[kt][r] = e;
            lq[(2 * kt + r) & 3] = (kt == 0 && r < 4) ? e : lq[(2 * kt + r) & 3] + e;
          }
        l += (lq[0] + lq[1]) + (lq[2] + lq[3]);
        // O^T += V^T . P^T : 4 k-steps of 16 keys
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          wait_v(kk);
          if (kk + VPRE < 4) read_v(kk + VPRE);
          const typename T::vec8 pf = pack8<T>(s[kk >> 1], 8 * (kk & 1));
#pragma unroll
          for (int dt = 0; dt < DT; ++dt) o[dt] = T::mfma32(join8<T>(vlo[kk][dt], vhi[kk][dt]), pf, o[dt]);
        }
      }
    }
  };

  // Each ring slot remembers its tile's source (SGPRs, written when the tile is issued), and the
  // kept-block index of the next tile to issue is read from LDS one tile ahead, so no LDS round
  // trip sits between a barrier and the tile's first MFMA.
  auto list_at = [&](int t) __attribute__((always_inline)) -> int {
    return t < ntm ? (int)list[min(t >> 1, kMaxBlocks - 1)] : 0;
  };
  using Src = std::conditional_t<kML, MlTileSrc, TileSrc>;
  auto any_list_at = [&](int t) __attribute__((always_inline)) -> int {
    if constexpr (kML) return ml_list_at(t);
    else return list_at(t);
  };
  auto any_tile_src = [&](int t, int raw) __attribute__((always_inline)) -> Src {
    if constexpr (kML) return ml_tile_src(t, raw);
    else return tile_src(t, raw);
  };
  auto any_issue = [&](const Src src, int slot) __attribute__((always_inline)) {
    if constexpr (kML) ml_issue(src, slot);
    else issue(src, slot);
  };
  Src slot_src[kBufs];
  const int pool_bias_bits = __builtin_amdgcn_readfirstlane(__float_as_int(p.pool_bias_l2));
  int next_blk, idx_blk = 0;
  if constexpr (kKvRows) {
    // I0 .. I(kBufs-1), then the rows of tiles 0 .. kBufs-2, each once its offsets have landed
    // (younger than I(s): I(s+1) .. I(kBufs-1) and the s row stages already issued)
#pragma unroll
    for (int s0 = 0; s0 < kBufs; ++s0) issue_idx(s0, list_at(s0));
    slot_src[0] = tile_src(0, list_at(0));
    VB_WAIT_VMCNT(kBufs - 1);
    asm volatile("" ::: "memory");
    issue(slot_src[0], 0, 0);
    if constexpr (kBufs > 2) {
      slot_src[1] = tile_src(1, list_at(1));
      VB_WAIT_VMCNT(kBufs - 2 + kInstPerWave);
      asm volatile("" ::: "memory");
      issue(slot_src[1], 1, 1);
    }
    next_blk = list_at(kBufs - 1);
    idx_blk = list_at(kBufs);
  } else {
    slot_src[0] = any_tile_src(0, any_list_at(0));
    if (ntiles > 0) any_issue(slot_src[0], 0);
    if constexpr (kBufs > 2) {
      slot_src[1] = any_tile_src(1, any_list_at(1));
      if (ntiles > 1) any_issue(slot_src[1], 1);
    }
    next_blk = any_list_at(kBufs - 1);
  }
  if constexpr (kQLate) load_q();   // its wait (vmcnt 0) also lands the ring's first tiles
  // The loop body is instantiated once per ring slot (compile-time U), so every LDS address is a
  // loop-invariant lane base + immediate offset: no address VALU inside the loop.
  auto body = [&](int t, auto U) __attribute__((always_inline)) {
    constexpr int u = decltype(U)::value;
    constexpr int un = (u + kBufs - 1) % kBufs;   // slot of the tile issued during this one
    // retire this wave's DMAs of tile t (younger tiles stay in flight); the barrier then makes
    // every wave's part visible and proves slot (t-1) % kBufs is no longer being read
    const int ti = t + kBufs - 1;
    if constexpr (kKvRows) {
      // per body: I(t+kBufs) then the rows of tile t+kBufs-1, always (past the end too). Body t
      // needs K/V(t) and I(t+kBufs-1); only the rows of tile t+1 (3-slot ring) are younger.
      if constexpr (kBufs == 3) VB_WAIT_VMCNT(kInstPerWave);
      else VB_WAIT_VMCNT(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      issue_idx(t + kBufs, idx_blk);
      slot_src[un] = tile_src(ti, next_blk);
      issue(slot_src[un], un, ti);
      next_blk = idx_blk;
      idx_blk = list_at(t + kBufs + 1);   // in flight during this tile's compute
    } else {
      const int younger = min(ntiles - 1 - t, kBufs - 2);
      if (younger >= 2) VB_WAIT_VMCNT(2 * kInstPerWave);
      else if (younger == 1) VB_WAIT_VMCNT(kInstPerWave);
      else VB_WAIT_VMCNT(0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      if (ti < ntiles) {
        slot_src[un] = any_tile_src(ti, next_blk);
        any_issue(slot_src[un], un);
        next_blk = any_list_at(ti + 1);   // in flight during this tile's compute
      }
    }
    const Src src = slot_src[u];
    int bias_bits;
    if constexpr (kML) {   // + ln(p) in the exp2 domain: log2(p) in {0, 1, 2, 3}
      bias_bits = src.lvl == 0 ? 0 : src.lvl == 1 ? 0x3F800000 : src.lvl == 2 ? 0x40000000 : 0x40400000;
    } else {
      bias_bits = (kPool && src.pooled) ? pool_bias_bits : 0;
    }
    bias_bits = __builtin_amdgcn_readfirstlane(bias_bits);
    tile_step(U, bias_bits, src.klen);
  };
  for (int t0 = 0; t0 < ntiles; t0 += kBufs) {
    body(t0, std::integral_constant<int, 0>{});
    if (t0 + 1 < ntiles) body(t0 + 1, std::integral_constant<int, 1>{});
    if constexpr (kBufs > 2)
      if (t0 + 2 < ntiles) body(t0 + 2, std::integral_constant<int, 2>{});
  }
  // the stages issued past the last tile land before exit; persistent launches always wait here (a
  // no-op at run time: every tile has landed): across the item loop's back edge hipcc's waitcnt pass
  // would otherwise count LDS-DMA as possibly in flight and wait (drain the ring) before the next
  // item's LDS reads
  if constexpr (kKvRows || kWQ) VB_WAIT_VMCNT(0);
  // The next item is claimed here, after the tile loop and before the epilogue's arithmetic and
  // stores, so its round trip overlaps them. Not inside the loop: the claim's wait for its own
  // result (and the waits hipcc then places after the branch) would drain the DMA ring every round.
  if (kWQ && tid == 0) next = wq_fetch(p.work_queue, blockIdx.x & 7, p.n_items);

  // ---- epilogue: O / l in the storage type to the caller's row, and the row's LSE ------------------
  const float lt = add_xor32(l);
  const float inv = (lt > 0.f) ? 1.0f / lt : 0.f;
  // streaming heads (unsupported) are flagged with NaN outputs written as bit patterns: this
  // translation unit is compiled with -fno-honor-nans, so no float arithmetic may produce them
  constexpr uint32_t kNaN2 = std::is_same<T, BF16>::value ? 0x7FC07FC0u : 0x7E007E00u;
  if (qvalid) {
    uint8_t* obase = reinterpret_cast<uint8_t*>(p.out) +
                     2 * (b * p.os[0] + h * p.os[1] + (qrow0 + qrow) * p.os[2]);
    // Each lane holds half of its row's 8-column groups (lane l: columns 8g..8g+3, lane l+32:
    // 8g+4..8g+7). One v_permlane32_swap per dword pairs groups 2p and 2p+1 so every lane owns 16
    // contiguous bytes: half the store instructions of the 8-byte form (guide T21).
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        u32x2 a, c;
        a[0] = pack2<T>(o[dt][8 * pr + 0] * inv, o[dt][8 * pr + 1] * inv);
        a[1] = pack2<T>(o[dt][8 * pr + 2] * inv, o[dt][8 * pr + 3] * inv);
        c[0] = pack2<T>(o[dt][8 * pr + 4] * inv, o[dt][8 * pr + 5] * inv);
        c[1] = pack2<T>(o[dt][8 * pr + 6] * inv, o[dt][8 * pr + 7] * inv);
        if (nan_head) a[0] = a[1] = c[0] = c[1] = kNaN2;
        const auto sx = __builtin_amdgcn_permlane32_swap(a[0], c[0], false, false);
        const auto sy = __builtin_amdgcn_permlane32_swap(a[1], c[1], false, false);
        const u32x4 w = {sx[0], sy[0], sx[1], sy[1]};
        *reinterpret_cast<u32x4*>(obase + (dt * 32 + 16 * pr + 8 * half) * 2) = w;
      }
    if (p.lse && half == 0) {
      const float v = (m + __log2f(lt)) * kLn2;
      float* dst = p.lse + b * p.lse_s[0] + h * p.lse_s[1] + (p.cu_q ? qg : qrow);
      if (nan_head) *reinterpret_cast<uint32_t*>(dst) = 0x7FC00000u;
      // a row with no kept key: -inf on the module path; +inf on the reference-signature entry
      // (cu_q set), FlashAttention-2's convention for an empty softmax (normalize_softmax_lse)
      else *dst = (p.cu_q && !(lt > 0.f)) ? INFINITY : v;
    }
  }
  VB_ATRACE_END();
}

template <int D, class T, bool kPool, bool kKvRows, bool kML = false, bool kCBias = false, bool kPersist = false>
__global__ void __launch_bounds__(kThreads, (D == 64 ? fwd::kWavesD64 : 2)) attn_fwd_kernel(const FwdParams p) {
  if constexpr (!kPersist) {   // one workgroup per item
    int next;
    attn_fwd_item<D, T, kPool, kKvRows, kML, kCBias, false>(p, blockIdx.x, next);
  } else {
    // persistent: a resident-sized grid, every item (the first one too) from the work queue
    __shared__ int next_s;
    int* const wq = p.work_queue;
    if (threadIdx.x == 0) next_s = wq_fetch(wq, blockIdx.x & 7, p.n_items);
    __syncthreads();
    int item = next_s;
    while (item >= 0) {
      int next = -2;   // -2: not claimed during the item (it returned before its tile loop)
      attn_fwd_item<D, T, kPool, kKvRows, kML, kCBias, true>(p, item, next);
      // every wave is done with this item's LDS (ring, list) before the next item's prologue writes it
      if (threadIdx.x == 0) next_s = next == -2 ? wq_fetch(wq, blockIdx.x & 7, p.n_items) : next;
      __syncthreads();
      item = next_s;
      __syncthreads();   // next_s is read by every wave before lane 0 may overwrite it
    }
    if (threadIdx.x == 0) wq_finish(wq);   // the last workgroup re-zeroes the queue
  }
}

// Dispatch order of the attention kernel's phase 2 (longest-processing-time first, per XCD): the
// kernel deals workgroups round-robin over the 8 XCDs and gives XCD x the contiguous range of
// linear work items xcd_linear assigns it (head-major). Each XCD drains its range in order, so its
// last workgroups set the kernel's tail. One workgroup per XCD range re-sorts the range by (head,
// kept key blocks descending): the head-major grouping (the L2 reuse of a head's K/V) stays, and
// within every head the longest q-blocks go first and the shortest last. Counting sort over
// (head, length) bins in LDS; the order inside a bin follows the atomics (placement only: every
// q-block's output is the same whatever the order). order[start + rank] = item.
constexpr int kOrderBins = 8192;
__global__ void __launch_bounds__(1024) attn_order_kernel(const FwdParams p, int32_t* order) {
  __shared__ int bins[kOrderBins];
  const int BH = p.B * p.H;
  const int hr = min(p.heavy_rows, p.nbq);
  const int rows_left = p.nbq - hr;
  // XCD x's range of the linear index: the inverse of xcd_linear (vb_tiles.hpp), whose slot 0 is `start`
  const int nwg = rows_left * BH;
  const int x = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7;
  int start = x < r8 ? x * (q8 + 1) : r8 * (q8 + 1) + (x - r8) * q8;
  const int count_x = q8 + (x < r8 ? 1 : 0);
  if (count_x <= 0) return;
  // only the range's last `order_window` items are re-ordered (the rest keep their place)
  const int skip = (p.order_window > 0 && p.order_window < count_x) ? count_x - p.order_window : 0;
  for (int i = threadIdx.x; i < skip; i += blockDim.x) order[start + i] = start + i;
  start += skip;
  const int count = count_x - skip;
  const int bh0 = start / rows_left;
  const int nh = (start + count - 1) / rows_left - bh0 + 1;
  const int nl = p.nbk + 1;   // kept counts 0..nbk
  // (head, length) bins; a range spanning more heads than LDS has bins for sorts by length alone
  // (longest first over the whole range: the tail is still the shortest items, the head-major
  // grouping is given up). nl <= kMaxBlocks + 1 < kOrderBins always fits.
  const bool by_head = (int64_t)nh * nl <= kOrderBins;
  const int nbins = by_head ? nh * nl : nl;
  for (int i = threadIdx.x; i < nbins; i += blockDim.x) bins[i] = 0;
  __syncthreads();
  auto key_of = [&](int lin) -> int {
    int bh, qblk;
    fwd_phase2_item(lin, rows_left, bh, qblk);
    bool nan_head = false;
    const uint8_t* mh = head_mask_base(p.mask, p.ms, p.head_mask_type, p.H, bh / p.H, bh % p.H, nan_head, p.hm_mode);
    int kept = p.nbk;
    if (p.q_len) {
      kept = min(max(p.q_len[(int64_t)bh * p.nbq + qblk], 0), p.nbk);
    } else if (mh) {
      const uint8_t* mrow = mh + (int64_t)qblk * p.ms[2];
      kept = 0;
      for (int j = 0; j < p.nbk; ++j) kept += mrow[j] != 0;
    }
    return (by_head ? (bh - bh0) * nl : 0) + (p.nbk - kept);   // head ascending, kept count descending
  };
  for (int i = threadIdx.x; i < count; i += blockDim.x) atomicAdd(&bins[key_of(start + i)], 1);
  __syncthreads();
  {   // exclusive prefix over the bins: every thread a run of C bins, a scan of the runs' sums
    __shared__ int wsum[16];
    const int C = (nbins + 1023) / 1024;
    const int b0 = threadIdx.x * C;
    int run = 0;
    for (int i = 0; i < C; ++i) run += (b0 + i < nbins) ? bins[b0 + i] : 0;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = run;   // inclusive scan within the wave
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int wbase = 0;
    for (int i = 0; i < w; ++i) wbase += wsum[i];
    int pos = wbase + incl - run;   // exclusive prefix of this thread's run
    for (int i = 0; i < C; ++i) {
      if (b0 + i < nbins) {
        const int c = bins[b0 + i];
        bins[b0 + i] = pos;
        pos += c;
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < count; i += blockDim.x) {
    const int lin = start + i;
    order[start + atomicAdd(&bins[key_of(lin)], 1)] = lin;
  }
}

// ---- launchers (declared in vb_attn_fwd.hpp; here because resident_grid needs the kernel symbol) ---
// Grid of one launch: one workgroup per item, or (persistent instantiation, with a work queue) as
// many as are resident at once — the occupancy of that instantiation times the device's CUs (host
// queries, cached per kernel and device; no device synchronisation), a multiple of 8 so every XCD
// gets the same number.
template <auto Kern, auto KernP>
static int launch_one(FwdParams p, hipStream_t stream, const char* what) {
  const unsigned items = (unsigned)(p.nbq * p.B * p.H);
  p.n_items = (int)items;
  if (p.work_queue) {
    const unsigned slots = (unsigned)resident_grid(reinterpret_cast<const void*>(KernP), kThreads, 0);
    hipLaunchKernelGGL(KernP, dim3(slots < items ? slots : items), dim3(kThreads), 0, stream, p);
  } else {
    hipLaunchKernelGGL(Kern, dim3(items), dim3(kThreads), 0, stream, p);
  }
  return check_launch(what);
}

// one forward kernel: its plain and its persistent instantiation (launch_one picks by p.work_queue)
template <int D, class T, bool kPool, bool kKvRows, bool kML, bool kCBias>
static int launch_attn(const FwdParams& p, hipStream_t stream, const char* what) {
  return launch_one<attn_fwd_kernel<D, T, kPool, kKvRows, kML, kCBias, false>,
                    attn_fwd_kernel<D, T, kPool, kKvRows, kML, kCBias, true>>(p, stream, what);
}

// inference launches (no LSE output) take the kCBias kernel
int launch_fwd(const FwdParams& p, int D, int dtype, bool pool, hipStream_t stream) {
  return dispatch_head(D, dtype, [&](auto d, auto t, auto pl, auto rows, auto cb) {
    return launch_attn<d(), decltype(t), pl(), rows(), false, cb()>(p, stream, "attn_fwd_kernel");
  }, pool, p.kv_rows != nullptr, p.lse == nullptr);
}

int launch_ml_fwd(const FwdParams& p, int D, int dtype, hipStream_t stream) {
  return dispatch_head(D, dtype, [&](auto d, auto t, auto cb) {
    return launch_attn<d(), decltype(t), false, false, true, cb()>(p, stream, "attn_fwd_kernel (multi-level)");
  }, p.lse == nullptr);
}

int launch_attn_order(const FwdParams& p, int32_t* order, hipStream_t stream) {
  hipLaunchKernelGGL(attn_order_kernel, dim3(8), dim3(1024), 0, stream, p, order);
  return check_launch("attn_order_kernel");
}

}  // namespace vb

#if VB_LAZY_COUNT
extern "C" int vb_diag_stamps(unsigned long long* host16, int reset) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(host16, HIP_SYMBOL(vb::g_vb_stamp), sizeof(unsigned long long) * 16);
  if (reset) {
    unsigned long long z[16] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(vb::g_vb_stamp), z, sizeof(z));
  }
  return 0;
}
#endif

#if VB_ATTN_TRACE
VB_TRACE_GETTER(vb_debug_attn_trace, vb::g_attn_trace)
#endif
