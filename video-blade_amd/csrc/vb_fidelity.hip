// Output-fidelity probe: exact dense attention rows for a handful of probe queries per head, and the
// error of a call's `out` against them (include/vblade.h, vb_attn_fidelity). The sibling of the recall
// probe (vb_recall.hip): the same MFMA score pass, but over keys in caller order (a softmax over all
// keys does not depend on their order, so K and V stream contiguously, no gather), and carried through
// V. The shape is flash-decoding:
//
//   fidelity_partial_kernel  one wave per chunk of 512 consecutive keys and (b,h). The S probe rows are
//                            MFMA A operands (one or two 32-row tiles), the keys B operands, 32 per
//                            tile, 16 bytes per lane and k-step. Pass 1 takes each row's chunk maximum
//                            m_c of t_j = qk_scale * <q,k_j> (lane-local over the tiles, one butterfly
//                            over the 32 key columns at the end). Pass 2 forms the same t_j again (K
//                            comes from L2 the second time), e_j = exp2(t_j - m_c), adds e_j into the
//                            lane's column sum and hands the tile's e to the V product through LDS as
//                            fp32 [key][row]; the tile's 32 rows of V go through LDS as well (16-byte
//                            loads; at D = 64 and S <= 32 keys and values are loaded one tile ahead). The V product runs on the vector ALU with
//                            lane = d (two d per lane at D = 128): per key one element of V per d and,
//                            per four probe rows, one broadcast 16-byte LDS read and four fmaf. e_j is
//                            never rounded below fp32. Staged: (m_c, l_c) and acc_c[D] per (b,h), chunk and row.
//   fidelity_join_kernel     one wave per (b,h,r): the row maximum, then the chunks in ascending order,
//                            l = fmaf(l_c, w_c, l) and a[d] = fmaf(acc_c[d], w_c, a[d]) with
//                            w_c = exp2(m_c - m); ref = a / l; one lane walks d in ascending order for
//                            row_err, row_sig and the row's peak.
//   fidelity_sum_kernel      one thread per (b,h): err and sig summed serially in r order, peak.
//
// No launch allocates or synchronises; no floating-point atomics; three launches on the caller's stream.
#include <cmath>
#include <string>

#include "vb_common.hpp"

namespace vb {
namespace {

constexpr int kChunkKeys = VB_FIDELITY_CHUNK;   // keys per partial workgroup: a rule of L alone
constexpr int kKeyTile = 32;                    // keys per MFMA tile
constexpr int kMaxSamples = VB_FIDELITY_MAX_SAMPLES;
constexpr int kMaxKeys = 131072;
constexpr int kSumThreads = 64;

struct FidelityParams {
  const void* q; const void* k; const void* v; const void* out;
  int64_t qs[3], ks[3], vs[3], os[3];
  const int32_t* probe_rows;
  int B, H, L, D, S, nc;
  float c;              // scale * log2(e)
  float* ml;            // workspace [B*H][nc][S][2]: chunk maximum, sum of exp2 relative to it
  float* acc;           // workspace [B*H][nc][S][D]: sum of e_j * v_j relative to the chunk maximum
  float* rowv;          // workspace [B*H][S][3]: row_err, row_sig, row peak, for the last launch
  float* err; float* sig; float* peak;
  float* row_err; float* row_sig; float* row_lse; float* ref;
};

__device__ __forceinline__ int clamp_row(int x, int L) { return x < 0 ? 0 : (x > L - 1 ? L - 1 : x); }

// ----------------------------------------------------------------------------------------- partial
// QT: 32-row tiles of probe rows (1: S <= 32, 2: S <= 64)
// A lane holds QT * D / 2 accumulators beside 32 * QT maxima and column sums in the MFMA C layout and the
// probe rows' operands: 2 waves per SIMD with one row tile, 1 with two. At (QT, D) = (1, 64) the registers
// also hold the next tile's keys and values, loaded one tile ahead (kAhead); the other instantiations have
// no room for them at their occupancy and load a tile where they use it.
template <class T, int D, int QT>
__global__ void __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(QT == 1 ? 2 : 1, QT == 1 ? 2 : 1)))
fidelity_partial_kernel(const FidelityParams p) {
  using vec8 = typename T::vec8;
  using raw = typename T::raw;
  constexpr int kSteps = D / 16;
  constexpr int kDpl = D / 64;             // d per lane in the V product
  constexpr int kRows = 32 * QT;
  constexpr int kPStride = kRows + 4;      // floats; keeps 16-byte alignment, spreads the banks
  constexpr bool kAhead = QT == 1 && D == 64;
  __shared__ __attribute__((aligned(16))) float P[kKeyTile * kPStride];
  __shared__ __attribute__((aligned(16))) raw Vs[kKeyTile * D];   // the tile's rows of V

  const int chunk = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int lane = lane_id();
  const int r32 = lane & 31, half = lane >> 5;
  const raw* qb = reinterpret_cast<const raw*>(p.q) + b * p.qs[0] + h * p.qs[1];
  const raw* kb = reinterpret_cast<const raw*>(p.k) + b * p.ks[0] + h * p.ks[1];
  const raw* vb_ = reinterpret_cast<const raw*>(p.v) + b * p.vs[0] + h * p.vs[1];
  const int key0 = chunk * kChunkKeys;
  const int nkeys = min(kChunkKeys, p.L - key0);       // >= 1: the grid holds ceil(L / chunk) chunks
  const int ntiles = (nkeys + kKeyTile - 1) / kKeyTile;

  // the probe rows as MFMA A operands: lane (r32, half) holds row r32 (+32), d = 16*step + 8*half ..+7.
  // Rows past S repeat row S-1 (never stored); row numbers are clamped to [0, L-1].
  vec8 qa[QT][kSteps];
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    int s = r32 + 32 * t;
    s = s < p.S ? s : p.S - 1;
    const int row = clamp_row(p.probe_rows[s], p.L);
    const raw* src = qb + (int64_t)row * p.qs[2] + 8 * half;
#pragma unroll
    for (int st = 0; st < kSteps; ++st) qa[t][st] = *reinterpret_cast<const vec8*>(src + 16 * st);
  }

  // one tile's keys as MFMA B operands (a key past L reads row L-1) and its scores. C layout: column
  // (key) = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * half. A key past L scores -inf.
  auto load_keys = [&](int tile, vec8 (&kf)[kSteps]) {
    const int j = min(key0 + tile * kKeyTile + r32, p.L - 1);
    const raw* src = kb + (int64_t)j * p.ks[2] + 8 * half;
#pragma unroll
    for (int st = 0; st < kSteps; ++st) kf[st] = *reinterpret_cast<const vec8*>(src + 16 * st);
  };
  auto scores = [&](int tile, const vec8 (&kf)[kSteps], f32x16 (&x)[QT]) {
    const bool live = key0 + tile * kKeyTile + r32 < p.L;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      f32x16 a = {};
#pragma unroll
      for (int st = 0; st < kSteps; ++st) a = T::mfma32(qa[t][st], kf[st], a);
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) x[t][reg] = live ? a[reg] * p.c : -INFINITY;
    }
  };

  // pass 1: the chunk maximum of every row (a maximum does not depend on its order)
  f32x16 mx[QT];
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) mx[t][reg] = -INFINITY;
  // (few registers are live here: four tiles' key loads are in flight at once)
#pragma unroll 4
  for (int tile = 0; tile < ntiles; ++tile) {
    vec8 kf[kSteps];
    load_keys(tile, kf);
    f32x16 x[QT];
    scores(tile, kf, x);
#pragma unroll
    for (int t = 0; t < QT; ++t)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) mx[t][reg] = fmaxf(mx[t][reg], x[t][reg]);
  }
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) mx[t][reg] = fmaxf(mx[t][reg], __shfl_xor(mx[t][reg], d, 64));

  // pass 2: e = exp2(t - m), column sums, and the V product with lane = d
  f32x16 ls[QT];
  float acc[kRows][kDpl];
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) ls[t][reg] = 0.f;
#pragma unroll
  for (int r = 0; r < kRows; ++r)
#pragma unroll
    for (int dd = 0; dd < kDpl; ++dd) acc[r][dd] = 0.f;

  // a tile's 32 rows of V, 16 bytes per lane and load. A key past L reads row L-1 against e = 0: it adds
  // +0 or -0 to a sum, which changes no bit of it unless v holds an infinity or a NaN, and then the row's
  // ref is not finite either way
  auto load_values = [&](int tile, vec8 (&vt)[kSteps]) {
#pragma unroll
    for (int i = 0; i < kSteps; ++i) {
      const int cidx = 64 * i + lane;   // 16-byte piece of the tile: row cidx / (D/8), pieces along d
      const int j = min(key0 + tile * kKeyTile + cidx / (D / 8), p.L - 1);
      vt[i] = *reinterpret_cast<const vec8*>(vb_ + (int64_t)j * p.vs[2] + 8 * (cidx % (D / 8)));
    }
  };
  // The workgroup is one wave, whose LDS operations execute in program order: between the LDS stores of
  // a tile and the reads of its V product (and back) the compiler only has to keep that order, so the
  // loop holds scheduling barriers, no s_barrier and no fence that would drain the loads in flight.
  vec8 kn[kSteps], vn[kSteps];   // kAhead: the next tile's keys and values
  if constexpr (kAhead) {
    load_keys(0, kn);
    load_values(0, vn);
  }
#pragma unroll 1
  for (int tile = 0; tile < ntiles; ++tile) {
    vec8 kf[kSteps], vt[kSteps];
    if constexpr (kAhead) {
#pragma unroll
      for (int i = 0; i < kSteps; ++i) { kf[i] = kn[i]; vt[i] = vn[i]; }
      const int ahead = min(tile + 1, ntiles - 1);
      load_keys(ahead, kn);
      load_values(ahead, vn);
    } else {
      load_values(tile, vt);
      load_keys(tile, kf);
    }
    f32x16 x[QT];
    scores(tile, kf, x);
    __builtin_amdgcn_wave_barrier();   // the V product of the tile before has read P and Vs
#pragma unroll
    for (int i = 0; i < kSteps; ++i) *reinterpret_cast<vec8*>(&Vs[8 * (64 * i + lane)]) = vt[i];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        x[t][reg] = exp2_fast(x[t][reg] - mx[t][reg]);   // exp2(-inf) = 0 for a key past L
        ls[t][reg] += x[t][reg];
      }
      // regs 4g .. 4g+3 are rows 8g + 4*half + 0..3 (+32t): one 16-byte store per g
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 e4 = {x[t][4 * g], x[t][4 * g + 1], x[t][4 * g + 2], x[t][4 * g + 3]};
        *reinterpret_cast<f32x4*>(&P[r32 * kPStride + 32 * t + 8 * g + 4 * half]) = e4;
      }
    }
    __builtin_amdgcn_wave_barrier();
    // one key per step, in ascending order: its row of V (lane = d) against the probe rows' e, four
    // rows per broadcast LDS read
#pragma unroll 2
    for (int j = 0; j < kKeyTile; ++j) {
      float vf[kDpl];
#pragma unroll
      for (int dd = 0; dd < kDpl; ++dd) vf[dd] = T::to_f32(Vs[j * D + kDpl * lane + dd]);
      const float* pr = &P[j * kPStride];
#pragma unroll
      for (int r4 = 0; r4 < kRows / 4; ++r4) {
        const f32x4 e4 = *reinterpret_cast<const f32x4*>(pr + 4 * r4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int dd = 0; dd < kDpl; ++dd) acc[4 * r4 + i][dd] = fmaf(e4[i], vf[dd], acc[4 * r4 + i][dd]);
      }
    }
  }

  // column sums -> row sums: a butterfly over the 32 key columns (a fixed order, every lane the same bits)
#pragma unroll
  for (int t = 0; t < QT; ++t)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
#pragma unroll
      for (int d = 16; d >= 1; d >>= 1) ls[t][reg] += __shfl_xor(ls[t][reg], d, 64);

  const int64_t slot = ((int64_t)bh * p.nc + chunk) * p.S;
  float* ml = p.ml + slot * 2;
#pragma unroll
  for (int t = 0; t < QT; ++t) {
    float pm = 0.f, pl = 0.f;   // the pair of the row this lane stores: reg == r32
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
      if (r32 == reg) { pm = mx[t][reg]; pl = ls[t][reg]; }
    const int s = (r32 & 3) + 8 * (r32 >> 2) + 4 * half + 32 * t;
    if (r32 < 16 && s < p.S) {
      ml[2 * s] = pm;
      ml[2 * s + 1] = pl;
    }
  }
  float* ao = p.acc + slot * D + kDpl * lane;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    if (r < p.S) {
#pragma unroll
      for (int dd = 0; dd < kDpl; ++dd) ao[(int64_t)r * D + dd] = acc[r][dd];
    }
  }
}

// -------------------------------------------------------------------------------------------- join
template <class T, int D>
__global__ void __launch_bounds__(64) fidelity_join_kernel(const FidelityParams p) {
  using raw = typename T::raw;
  constexpr int kDpl = D / 64;
  __shared__ float refs[D], outs[D];
  const int r = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
  const int lane = lane_id();
  const int64_t cstride = (int64_t)p.S;   // rows per chunk slot
  const float* ml = p.ml + ((int64_t)bh * p.nc * cstride + r) * 2;
  const float* acc = p.acc + ((int64_t)bh * p.nc * cstride + r) * D + lane;

  float m = -INFINITY;
  for (int c = 0; c < p.nc; ++c) m = fmaxf(m, ml[(int64_t)c * cstride * 2]);
  float l = 0.f, a[kDpl];
#pragma unroll
  for (int dd = 0; dd < kDpl; ++dd) a[dd] = 0.f;
  for (int c = 0; c < p.nc; ++c) {
    const float w = exp2_fast(ml[(int64_t)c * cstride * 2] - m);
    l = fmaf(ml[(int64_t)c * cstride * 2 + 1], w, l);
#pragma unroll
    for (int dd = 0; dd < kDpl; ++dd) a[dd] = fmaf(acc[(int64_t)c * cstride * D + 64 * dd], w, a[dd]);
  }
  const int g = clamp_row(p.probe_rows[r], p.L);
  const raw* ob = reinterpret_cast<const raw*>(p.out) + b * p.os[0] + h * p.os[1] + (int64_t)g * p.os[2];
  const int64_t o = (int64_t)bh * p.S + r;
#pragma unroll
  for (int dd = 0; dd < kDpl; ++dd) {
    const int d = lane + 64 * dd;
    const float x = a[dd] / l;
    refs[d] = x;
    outs[d] = T::to_f32(ob[d]);
    if (p.ref) p.ref[o * D + d] = x;
  }
  __syncthreads();
  if (lane != 0) return;
  float e = 0.f, s = 0.f, pk = 0.f;
  for (int d = 0; d < D; ++d) {
    const float x = refs[d], df = outs[d] - x;
    e = fmaf(df, df, e);
    s = fmaf(x, x, s);
    pk = fmaxf(pk, fabsf(x));
  }
  p.rowv[3 * o] = e;
  p.rowv[3 * o + 1] = s;
  p.rowv[3 * o + 2] = pk;
  if (p.row_err) p.row_err[o] = e;
  if (p.row_sig) p.row_sig[o] = s;
  if (p.row_lse) p.row_lse[o] = logf(l) + m * kLn2;
}

// --------------------------------------------------------------------------------------------- sum
__global__ void __launch_bounds__(kSumThreads) fidelity_sum_kernel(const FidelityParams p) {
  const int bh = blockIdx.x * kSumThreads + threadIdx.x;
  if (bh >= p.B * p.H) return;
  const float* v = p.rowv + (int64_t)bh * p.S * 3;
  float e = 0.f, s = 0.f, pk = 0.f;
  for (int r = 0; r < p.S; ++r) {
    e += v[3 * r];
    s += v[3 * r + 1];
    pk = fmaxf(pk, v[3 * r + 2]);
  }
  p.err[bh] = e;
  p.sig[bh] = s;
  if (p.peak) p.peak[bh] = pk;
}

int chunks_of(const vb_fidelity_args* a) { return (a->L + kChunkKeys - 1) / kChunkKeys; }

template <class T>
const void* partial_kernel(int D, bool two) {
  if (D == 64)
    return two ? reinterpret_cast<const void*>(fidelity_partial_kernel<T, 64, 2>)
               : reinterpret_cast<const void*>(fidelity_partial_kernel<T, 64, 1>);
  return two ? reinterpret_cast<const void*>(fidelity_partial_kernel<T, 128, 2>)
             : reinterpret_cast<const void*>(fidelity_partial_kernel<T, 128, 1>);
}

template <class T>
const void* join_kernel(int D) {
  return D == 64 ? reinterpret_cast<const void*>(fidelity_join_kernel<T, 64>)
                 : reinterpret_cast<const void*>(fidelity_join_kernel<T, 128>);
}

}  // namespace
}  // namespace vb

extern "C" uint64_t vb_attn_fidelity_workspace_size(const vb_fidelity_args* a) {
  if (!a || a->B <= 0 || a->H <= 0 || a->L <= 0 || a->S <= 0 || a->D <= 0) return 0;
  // per (b,h), chunk and row: (m, l) and the D partial sums; per (b,h) and row: three results
  const uint64_t rows = (uint64_t)a->B * a->H * a->S;
  const uint64_t words = rows * (uint64_t)vb::chunks_of(a) * (uint64_t)(a->D + 2) + rows * 3;
  return (words * 4 + 15) & ~uint64_t(15);
}

extern "C" int vb_attn_fidelity(const vb_fidelity_args* a, void* stream) {
  using namespace vb;
  const std::string fn = "vb_attn_fidelity: ";
  if (!a || !a->q || !a->k || !a->v || !a->out || !a->probe_rows || !a->err || !a->sig)
    return fail(VB_ERR_INVALID, fn + "null argument");
  if (a->B <= 0 || a->H <= 0 || a->L <= 0) return fail(VB_ERR_INVALID, fn + "bad sizes");
  if (a->L > kMaxKeys) return fail(VB_ERR_UNSUPPORTED, fn + "sequence too long (L <= 131072)");
  if (a->S < 1 || a->S > kMaxSamples) return fail(VB_ERR_INVALID, fn + "S must be in [1, 64]");
  if (a->dtype != VB_DTYPE_BF16 && a->dtype != VB_DTYPE_F16) return fail(VB_ERR_INVALID, fn + "unknown dtype");
  if (a->D != 64 && a->D != 128) return fail(VB_ERR_UNSUPPORTED, fn + "head_dim must be 64 or 128");
  const int64_t* strides[4] = {a->q_stride, a->k_stride, a->v_stride, a->out_stride};
  for (const int64_t* st : strides)
    for (int i = 0; i < 3; ++i)
      if ((st[i] & 7) || st[i] < 0)
        return fail(VB_ERR_INVALID, fn + "q/k/v/out strides must be non-negative multiples of 8");
  for (const int64_t* st : strides)
    if ((int64_t)(a->L - 1) * st[2] * 2 + 2 * a->D >= (int64_t(1) << 31))
      return fail(VB_ERR_UNSUPPORTED, fn + "a q/k/v/out (b,h) slice spans >= 2 GiB");
  if ((reinterpret_cast<uintptr_t>(a->q) | reinterpret_cast<uintptr_t>(a->k) | reinterpret_cast<uintptr_t>(a->v) |
       reinterpret_cast<uintptr_t>(a->out)) & 15)
    return fail(VB_ERR_INVALID, fn + "q, k, v and out must be 16-byte aligned");
  const uint64_t need = vb_attn_fidelity_workspace_size(a);
  if (!a->workspace || a->workspace_bytes < need || (reinterpret_cast<uintptr_t>(a->workspace) & 15))
    return fail(VB_ERR_INVALID, fn + "workspace missing or smaller than vb_attn_fidelity_workspace_size() (" +
                                    std::to_string(need) + " bytes)");
  FidelityParams p{};
  p.q = a->q; p.k = a->k; p.v = a->v; p.out = a->out;
  for (int i = 0; i < 3; ++i) {
    p.qs[i] = a->q_stride[i]; p.ks[i] = a->k_stride[i]; p.vs[i] = a->v_stride[i]; p.os[i] = a->out_stride[i];
  }
  p.probe_rows = a->probe_rows;
  p.B = a->B; p.H = a->H; p.L = a->L; p.D = a->D; p.S = a->S; p.nc = chunks_of(a);
  const float scale = a->scale > 0.f ? a->scale : (float)(1.0 / sqrt((double)a->D));
  p.c = scale * kLog2e;
  const int64_t rows = (int64_t)a->B * a->H * a->S;
  p.ml = reinterpret_cast<float*>(a->workspace);
  p.acc = p.ml + rows * p.nc * 2;
  p.rowv = p.acc + rows * p.nc * a->D;
  p.err = a->err; p.sig = a->sig; p.peak = a->peak;
  p.row_err = a->row_err; p.row_sig = a->row_sig; p.row_lse = a->row_lse; p.ref = a->ref;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const bool two = a->S > 32;
  const bool bf = a->dtype == VB_DTYPE_BF16;
  void* params[] = {&p};
  const unsigned bh = (unsigned)(a->B * a->H);
  (void)hipLaunchKernel(bf ? partial_kernel<BF16>(a->D, two) : partial_kernel<F16>(a->D, two),
                        dim3((unsigned)p.nc, bh), dim3(64), params, 0, s);
  if (int rc = check_launch("fidelity_partial_kernel")) return rc;
  (void)hipLaunchKernel(bf ? join_kernel<BF16>(a->D) : join_kernel<F16>(a->D), dim3((unsigned)a->S, bh), dim3(64),
                        params, 0, s);
  if (int rc = check_launch("fidelity_join_kernel")) return rc;
  (void)hipLaunchKernel(reinterpret_cast<const void*>(fidelity_sum_kernel), dim3((bh + kSumThreads - 1) / kSumThreads),
                        dim3(kSumThreads), params, 0, s);
  return check_launch("fidelity_sum_kernel");
}
