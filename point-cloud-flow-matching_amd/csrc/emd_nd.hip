// Approximate EMD over D-component points, D in {2, 3, 5, 6}, float32
// (include/pcfm_emd_nd.h): csrc/emd.hip's design with a wider point.
//
// What is shared with emd.hip is in emd_core.hpp and exists once: the level
// table, emd_exp2, the three finalize expressions, row_at, block_sum, the host
// plan, the prologue and the launch sequence (PH 2 of level j fused with PH 0 of
// level j + 1, PCFM_EMD_FORM=unfused running them apart).  d2 is sqdist_nd<D> of
// chamfer_search.hpp, at D = 3 the chain of sqdist3, and every sum below is
// taken in the order emd.hip takes it, so D = 3 returns emd.hip's bits.
//
// What is new is the point width:
//   * a pack is the point's D coordinates and the coefficient it carries into a
//     pass, in 16-byte slots: {c0, c1, c2 | 0, coef} for D <= 3 and
//     {c0, c1, c2, c3} {c4, c5 | 0, 0, coef} for D = 5, 6 (the pads are written 0
//     by the pack kernel: nothing depends on what the workspace held);
//   * a row keeps its D coordinates in registers;
//   * a wave's LDS chunk stays 128 slots (2 KiB, 32 KiB per block): 128 columns
//     of one slot (64 + 64 in PH 3: the column and, for its coefficient, the
//     same column of packL0), or 64 columns of two slots.  In PH 3 a two-slot
//     column's second coefficient goes to a 64-float side array (4 KiB per
//     block), loaded as one float per lane instead of a third 16-byte slot.
//     With the 4 + 4 KiB of wave sums a block holds at most 44 KiB of LDS, one
//     1024-thread block per CU;
//   * a column is read from LDS as one or two broadcast ds_read_b128.
#include "chamfer_search.hpp"
#include "emd_core.hpp"

#include "../../include/pcfm_emd_nd.h"

namespace pcfm {
namespace {

template <int D>
constexpr int kPack = emd_pack_elems(D);  // floats per pack
template <int D>
constexpr int kSlots = kPack<D> / 4;  // 16-byte slots per pack

// packK[b, k] = {p1, ratL};  packL0[b, l] = {p2, remR};  packL1[b, l] = {p2, ratR}
struct NdRowState {
  float* packK;
  float* packL0;
  float* packL1;
  float* remL;
  float* levL;  // [kLevels][b * n]
  float* levR;  // [kLevels][b * m]
};

// A pack's slots (hi is not looked at for D <= 3) -> the point and its coefficient.
template <int D>
__device__ __forceinline__ void unpack(const float4& lo, const float4& hi, float (&x)[D],
                                       float& coef) {
  x[0] = lo.x;
  x[1] = lo.y;
  if constexpr (D >= 3) x[2] = lo.z;
  if constexpr (D <= 3) {
    coef = lo.w;
  } else {
    x[3] = lo.w;
    x[4] = hi.x;
    if constexpr (D == 6) x[5] = hi.y;
    coef = hi.w;
  }
}

template <int D>
__device__ __forceinline__ void write_pack(float* pack, const float* __restrict__ p, float coef) {
  float v[kPack<D>] = {};
#pragma unroll
  for (int e = 0; e < D; ++e) v[e] = p[e];
  v[kPack<D> - 1] = coef;
  float4* o = reinterpret_cast<float4*>(pack);
#pragma unroll
  for (int h = 0; h < kSlots<D>; ++h)
    o[h] = float4(v[4 * h], v[4 * h + 1], v[4 * h + 2], v[4 * h + 3]);
}

template <int D>
__global__ void emd_nd_pack_kernel(const float* __restrict__ p1, size_t bn, float multiL,
                                   const float* __restrict__ p2, size_t bm, float multiR,
                                   NdRowState s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < bn) {
    write_pack<D>(s.packK + i * kPack<D>, p1 + i * D, 0.0f);
    s.remL[i] = multiL;
  }
  if (i < bm) {
    write_pack<D>(s.packL0 + i * kPack<D>, p2 + i * D, multiR);
    write_pack<D>(s.packL1 + i * kPack<D>, p2 + i * D, 0.0f);
  }
}

// Column c of a wave's chunk: slot c, and for a two-slot pack slot 64 + c.
template <int D>
__device__ __forceinline__ void chunk_col(const float4* __restrict__ st, int c, float (&q)[D],
                                          float& coef) {
  const float4 lo = st[c];
  if constexpr (kSlots<D> == 2) {
    unpack<D>(lo, st[64 + c], q, coef);
  } else {
    unpack<D>(lo, lo, q, coef);
  }
}

// One chunk of a pass over `cnt` staged columns: emd.hip's rowpass_chunk (PH 0,
// 1, 2) and rowpass_pair (PH 3), the same expressions in the same order.  PH 3's
// second coefficient remR_{j+1} of column c is side[c] for a two-slot pack and
// st[64 + c].w for a one-slot pack.
template <int D, int PH>
__device__ __forceinline__ void nd_chunk(const float4* __restrict__ st,
                                         const float* __restrict__ side, int cnt,
                                         const float (&x)[D], float rl, float lvl2, float lvl2b,
                                         float& acc, float& acc2) {
  if constexpr (PH != 3) {
    if (lvl2 == 0.0f) {  // level 0: exp(0 * d2) = 1 exactly
#pragma unroll 8
      for (int c = 0; c < cnt; ++c) {
        const float coef = kSlots<D> == 2 ? st[64 + c].w : st[c].w;
        acc = __builtin_fmaf(PH == 2 ? rl : 1.0f, coef, acc);
      }
      return;
    }
  }
#pragma unroll 8
  for (int c = 0; c < cnt; ++c) {
    float q[D], coef;
    chunk_col<D>(st, c, q, coef);
    const float d2 = sqdist_nd<D>(q, x);
    if constexpr (PH == 3) {
      const float rr = kSlots<D> == 2 ? side[c] : st[64 + c].w;
      const float e2 = emd_exp2<float>(d2, lvl2);
      const float e0 = emd_exp2<float>(d2, lvl2b);
      acc2 = __builtin_fmaf(e2 * rl, coef, acc2);
      acc = __builtin_fmaf(e0, rr, acc);
    } else if constexpr (PH == 2) {
      acc = __builtin_fmaf(emd_exp2<float>(d2, lvl2) * rl, coef, acc);
    } else {
      acc = __builtin_fmaf(emd_exp2<float>(d2, lvl2), coef, acc);
    }
  }
}

// The passes of emd.hip's emd_rowpass_kernel over packs of kSlots<D> slots:
// PH 0: rows k (packK), cols packL0 (coef remR);  suml -> ratL
// PH 1: rows l (packL0), cols packK (coef ratL);  sumr -> ratR, levR[lvl], remR
// PH 2: rows k (packK, row scale ratL), cols packL1 (coef ratR);  -> remL, levL[lvl]
// PH 3: PH 2 of level lvl then PH 0 of level lvl + 1 (lvl2b) in one launch.
// grid = (ceil(nr / 64), b), 1024 threads; a wave stages its column slice through
// its own LDS chunk, the next chunk's loads in flight while this one is used.
template <int D, int PH>
__global__ void __launch_bounds__(64 * kRowWaves)
    emd_nd_rowpass_kernel(int nr, int ncol, float lvl2, float lvl2b, int lvl, NdRowState s) {
  constexpr int P = kPack<D>, W = kSlots<D>;
  constexpr bool kSide = PH == 3 && W == 2;
  constexpr int CH = (W == 2 || PH == 3) ? 64 : kColChunk;  // columns per chunk
  __shared__ float red[kRowWaves][64];
  __shared__ float red2[PH == 3 ? kRowWaves : 1][64];
  __shared__ float4 stage[kRowWaves][kColChunk];
  __shared__ float side[kSide ? kRowWaves : 1][64];
  float* rows = PH == 1 ? s.packL0 : s.packK;
  const float* __restrict__ cols = PH == 0 ? s.packL0 : (PH == 1 ? s.packK : s.packL1);
  const int bb = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * 64 + lane;
  float x[D], rl;  // the row and its coefficient (PH 2 / 3: ratL; PH 1: remR)
  {
    const float4* rp = reinterpret_cast<const float4*>(rows) + row_at(bb, nr, i) * W;
    unpack<D>(rp[0], rp[W - 1], x, rl);
  }
  const int c0 = (int)(((long long)ncol * w) / kRowWaves);
  const int c1 = (int)(((long long)ncol * (w + 1)) / kRowWaves);
  const float4* __restrict__ cb = reinterpret_cast<const float4*>(cols) + (size_t)bb * ncol * W;
  const float* __restrict__ cb2 = s.packL0 + (size_t)bb * ncol * P;  // PH 3's remR_{lvl+1}
  float4* st = stage[w];
  float* sd = side[kSide ? w : 0];
  float acc = 0, acc2 = 0;
  // unconditional loads (index clamped to the batch element's last column; the
  // extra columns are never read): no branch around a load in flight
  const int cl = ncol - 1;
  float4 n0, n1;
  float nside = 0;
  auto fetch = [&](int base) {
    const int c = min(base + lane, cl);
    if constexpr (W == 2) {
      n0 = cb[2 * c];
      n1 = cb[2 * c + 1];
      if constexpr (kSide) nside = cb2[(size_t)c * P + (P - 1)];
    } else {
      n0 = cb[c];
      n1 = PH == 3 ? reinterpret_cast<const float4*>(cb2)[c] : cb[min(base + 64 + lane, cl)];
    }
  };
  fetch(c0);
  for (int base = c0; base < c1; base += CH) {
    st[lane] = n0;
    st[64 + lane] = n1;
    if constexpr (kSide) sd[lane] = nside;
    fetch(base + CH);
    nd_chunk<D, PH>(st, sd, min(CH, c1 - base), x, rl, lvl2, lvl2b, acc, acc2);
  }
  red[w][lane] = acc;
  if constexpr (PH == 3) red2[w][lane] = acc2;
  __syncthreads();
  if (w != 0 || i >= nr) return;
  float t = 0, t2 = 0;
#pragma unroll
  for (int q = 0; q < kRowWaves; ++q) {
    t += red[q][lane];
    if constexpr (PH == 3) t2 += red2[q][lane];
  }
  const size_t idx = (size_t)bb * nr + i;
  const size_t lv = (size_t)lvl * gridDim.y * nr + idx;
  float* rcoef = rows + idx * P + (P - 1);
  if constexpr (PH == 0) {
    *rcoef = emd_ratio_l(s.remL[idx], t);
  } else if constexpr (PH == 1) {
    const float r = rl;
    const float sumr = t * r;  // sumr *= remainR
    const float rat = emd_ratio_r(r, sumr);
    s.packL1[idx * P + (P - 1)] = rat;
    s.levR[lv] = rat;
    *rcoef = emd_remain(r, sumr);
  } else {  // PH 2, and PH 3: level lvl's remainL, then level lvl+1's ratioL
    const float rem = emd_remain(s.remL[idx], PH == 3 ? t2 : t);
    s.remL[idx] = rem;
    s.levL[lv] = rl;
    if constexpr (PH == 3) *rcoef = emd_ratio_l(rem, t);
  }
}

// This thread's row k of p1 (clamped: row_at) in registers.
template <int D>
__device__ __forceinline__ void load_row(const float* __restrict__ p1, int bb, int n, int k,
                                         float (&x)[D]) {
  const float* p = p1 + row_at(bb, n, k) * D;
#pragma unroll
  for (int e = 0; e < D; ++e) x[e] = p[e];
}

// The match write with matchcost fused: emd.hip's emd_match_cost_kernel with D
// coordinates staged per column l.
template <int D>
__global__ void __launch_bounds__(kEmdThreads)
    emd_nd_match_cost_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int b,
                             int n, int m, const float* __restrict__ levL,
                             const float* __restrict__ levR, float* __restrict__ match,
                             float* __restrict__ part) {
  constexpr int kW = kLevels + D;  // per l: ratioR_0..9, the D coordinates
  __shared__ float sl[kMatchL * kW];
  __shared__ float red[kEmdThreads / 64];
  const int bb = blockIdx.z, kb = blockIdx.x, lb = blockIdx.y;
  const int k = kb * kEmdThreads + threadIdx.x;
  const int l0 = lb * kMatchL, nl = min(kMatchL, m - l0);
  for (int e = threadIdx.x; e < nl * kW; e += kEmdThreads) {
    const int li = e / kW, q = e - li * kW;
    sl[e] = q < kLevels ? levR[(size_t)q * b * m + (size_t)bb * m + l0 + li]
                        : p2[((size_t)bb * m + l0 + li) * D + (q - kLevels)];
  }
  float x[D];
  load_row<D>(p1, bb, n, k, x);
  float rl[kLevels];
#pragma unroll
  for (int j = 0; j < kLevels; ++j) rl[j] = levL[(size_t)j * b * n + row_at(bb, n, k)];
  __syncthreads();
  float csum = 0;
  float* mrow = match != nullptr ? match + ((size_t)bb * m + l0) * n + k : nullptr;
  for (int li = 0; li < nl; ++li) {
    const float* q = sl + li * kW;
    const float d2 = sqdist_nd<D>(q + kLevels, x);
    float acc = 0;
#pragma unroll
    for (int j = 0; j < kLevels; ++j) {
      const float e = j == kLevels - 1 ? 1.0f : emd_exp2<float>(d2, level_log2e(j));  // level 0: 1
      acc += (e * rl[j]) * q[j];
    }
    if (mrow != nullptr && k < n) mrow[(size_t)li * n] = acc;
    csum = __builtin_fmaf(d2, acc, csum);
  }
  const float t = block_sum(k < n ? csum : 0.0f, red);
  if (threadIdx.x == 0) part[((size_t)bb * gridDim.y + lb) * gridDim.x + kb] = t;
}

// cost partials: grid = (k blocks, S, b); part[(bb*S + s)*kblocks + kb].
template <int D>
__global__ void __launch_bounds__(kEmdThreads)
    emd_nd_cost_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                       const float* __restrict__ match, int b, int n, int m, int S,
                       float* __restrict__ part) {
  __shared__ float red[kEmdThreads / 64];
  const int bb = blockIdx.z, s = blockIdx.y;
  const int k = blockIdx.x * kEmdThreads + threadIdx.x;
  float x[D];
  load_row<D>(p1, bb, n, k, x);
  const int l0 = (int)(((long long)m * s) / S), l1 = (int)(((long long)m * (s + 1)) / S);
  const float* __restrict__ cb = p2 + (size_t)bb * m * D;
  float sub = 0;
  if (k < n) {
    for (int l = l0; l < l1; ++l) {
      const float d = sqdist_nd<D>(cb + (size_t)D * l, x);
      sub = __builtin_fmaf(d, match[((size_t)bb * m + l) * n + k], sub);
    }
  }
  const float t = block_sum(sub, red);
  if (threadIdx.x == 0) part[((size_t)bb * S + s) * gridDim.x + blockIdx.x] = t;
}

__global__ void __launch_bounds__(64)
    emd_nd_cost_fin_kernel(const float* __restrict__ part, int per_b, float* __restrict__ cost) {
  emd_cost_fin<float>(part, per_b, cost);
}

// grad1 partials: lanes over k, l split S ways: part[s][(bb*n + k)*D + c].
template <int D>
__global__ void __launch_bounds__(kEmdThreads)
    emd_nd_grad1_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                        const float* __restrict__ match, int b, int n, int m, int S,
                        float* __restrict__ part) {
  const int bb = blockIdx.z, s = blockIdx.y;
  const int k = blockIdx.x * kEmdThreads + threadIdx.x;
  if (k >= n) return;
  float x[D];
  load_row<D>(p1, bb, n, k, x);
  const int l0 = (int)(((long long)m * s) / S), l1 = (int)(((long long)m * (s + 1)) / S);
  const float* __restrict__ cb = p2 + (size_t)bb * m * D;
  float g[D] = {};
  for (int l = l0; l < l1; ++l) {
    const float d = match[((size_t)bb * m + l) * n + k] * 2.0f;
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] = __builtin_fmaf(x[c] - cb[(size_t)D * l + c], d, g[c]);
  }
  float* o = part + (size_t)s * b * n * D + ((size_t)bb * n + k) * D;
#pragma unroll
  for (int c = 0; c < D; ++c) o[c] = g[c];
}

// grad1[i] = (the S partials of entry i, in order) * grad_cost[bb]; nd = n * D
__global__ void emd_nd_grad1_fin_kernel(const float* __restrict__ part, int S, int b, size_t nd,
                                        const float* __restrict__ gcost,
                                        float* __restrict__ grad1) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)b * nd;
  if (i >= total) return;
  grad1[i] = sum_parts(part, S, total, i) * gcost[i / nd];
}

// grad2: one block per (l, b); lanes stride over k, one block reduce per component.
template <int D>
__global__ void __launch_bounds__(kEmdThreads)
    emd_nd_grad2_kernel(const float* __restrict__ p1, const float* __restrict__ p2,
                        const float* __restrict__ match, const float* __restrict__ gcost, int n,
                        int m, float* __restrict__ grad2) {
  __shared__ float red[kEmdThreads / 64];
  const int l = blockIdx.x, bb = blockIdx.y;
  float y[D];
#pragma unroll
  for (int c = 0; c < D; ++c) y[c] = p2[((size_t)bb * m + l) * D + c];
  const float* __restrict__ row = match + ((size_t)bb * m + l) * n;
  const float* __restrict__ pb = p1 + (size_t)bb * n * D;
  float sum[D] = {};
  for (int k = threadIdx.x; k < n; k += kEmdThreads) {
    const float d = row[k] * 2.0f;
#pragma unroll
    for (int c = 0; c < D; ++c) sum[c] = __builtin_fmaf(y[c] - pb[(size_t)D * k + c], d, sum[c]);
  }
  float t[D];
#pragma unroll
  for (int c = 0; c < D; ++c) t[c] = block_sum(sum[c], red);
  if (threadIdx.x == 0) {
    const float g = gcost[bb];
    float* o = grad2 + ((size_t)bb * m + l) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = t[c] * g;
  }
}

// ---------------------------------------------------------------------------
// Host side: emd_core.hpp's plan, prologue and launch sequence, per D.
// ---------------------------------------------------------------------------
template <int D>
void launch_approxmatch_nd(const float* p1, const float* p2, int b, int n, int m, float* match,
                           float* cost, const EmdPlan& p, float* ws, hipStream_t st) {
  const NdRowState s{ws + p.packK, ws + p.packL0, ws + p.packL1,
                     ws + p.remL,  ws + p.levL,   ws + p.levR};
  const float multiL = n >= m ? 1.0f : (float)(m / n);  // integer ratio of the cloud sizes
  const float multiR = n >= m ? (float)(n / m) : 1.0f;
  hipLaunchKernelGGL(emd_nd_pack_kernel<D>, grid1d(std::max(p.bn, p.bm)), dim3(256), 0, st, p1,
                     p.bn, multiL, p2, p.bm, multiR, s);
  const dim3 gL(ceil_div(n, 64), b), gR(ceil_div(m, 64), b), blk(64 * kRowWaves);
  emd_run_levels([&](auto ph, int j, int jn) {
    constexpr int PH = decltype(ph)::value;
    constexpr bool rows_k = PH != 1;  // PH 1's rows are the l points
    hipLaunchKernelGGL((emd_nd_rowpass_kernel<D, PH>), rows_k ? gL : gR, blk, 0, st,
                       rows_k ? n : m, rows_k ? m : n, level_log2e(j),
                       PH == 3 ? level_log2e(jn) : 0.0f, j, s);
  });
  const dim3 gm(ceil_div(n, kEmdThreads), ceil_div(m, kMatchL), b);
  hipLaunchKernelGGL(emd_nd_match_cost_kernel<D>, gm, dim3(kEmdThreads), 0, st, p1, p2, b, n, m,
                     (const float*)s.levL, (const float*)s.levR, match, ws + p.mpart);
  hipLaunchKernelGGL(emd_nd_cost_fin_kernel, dim3(b), dim3(64), 0, st,
                     (const float*)(ws + p.mpart), (int)(gm.x * gm.y), cost);
}

template <int D>
void launch_matchcost_nd(const float* p1, const float* p2, const float* match, int b, int n,
                         int m, float* cost, const EmdPlan& p, float* ws, hipStream_t st) {
  const dim3 g(ceil_div(n, kEmdThreads), p.S, b);
  hipLaunchKernelGGL(emd_nd_cost_kernel<D>, g, dim3(kEmdThreads), 0, st, p1, p2, match, b, n, m,
                     p.S, ws + p.part);
  hipLaunchKernelGGL(emd_nd_cost_fin_kernel, dim3(b), dim3(64), 0, st,
                     (const float*)(ws + p.part), p.S * (int)g.x, cost);
}

template <int D>
void launch_matchcost_bwd_nd(const float* gcost, const float* p1, const float* p2,
                             const float* match, int b, int n, int m, float* grad1, float* grad2,
                             const EmdPlan& p, float* ws, hipStream_t st) {
  hipLaunchKernelGGL(emd_nd_grad1_kernel<D>, dim3(ceil_div(n, kEmdThreads), p.S, b),
                     dim3(kEmdThreads), 0, st, p1, p2, match, b, n, m, p.S, ws + p.part);
  hipLaunchKernelGGL(emd_nd_grad1_fin_kernel, grid1d(p.bn * D), dim3(256), 0, st,
                     (const float*)(ws + p.part), p.S, b, (size_t)n * D, gcost, grad1);
  hipLaunchKernelGGL(emd_nd_grad2_kernel<D>, dim3(m, b), dim3(kEmdThreads), 0, st, p1, p2, match,
                     gcost, n, m, grad2);
}

// f(integral_constant<int, d>) for a d that emd_entry has accepted
template <class F>
void with_dim(int d, F&& f) {
  switch (d) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 6>{}); break;
  }
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_emd_nd_abi_version(void) { return PCFM_EMD_ND_ABI_VERSION; }

extern "C" int pcfm_emd_nd_supported(int d) { return emd_dim_ok(d) ? 1 : 0; }

extern "C" size_t pcfm_emd_nd_workspace_bytes(int b, int n, int m, int d) {
  if (b < 0 || n < 0 || m < 0 || !emd_dim_ok(d)) return 0;
  return EmdPlan(b, n, m, d, sizeof(float)).bytes;
}

extern "C" int pcfm_emd_nd_approxmatch_cost_f32(const float* p1, const float* p2, int b, int n,
                                                int m, int d, float* match, float* cost,
                                                void* ws, size_t ws_bytes, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  PCFM_CHECK_ARG(cost != nullptr || b == 0, "emd_nd_approxmatch_cost: cost is required");
  return emd_entry<float>("emd_nd_approxmatch_cost", b, n, m, d, ws, ws_bytes, st,
                          {{cost, (size_t)b}}, [&](const EmdPlan& p, float* w) {
                            with_dim(d, [&](auto dc) {
                              launch_approxmatch_nd<decltype(dc)::value>(p1, p2, b, n, m, match,
                                                                         cost, p, w, st);
                            });
                          });
}

extern "C" int pcfm_emd_nd_matchcost_f32(const float* p1, const float* p2, const float* match,
                                         int b, int n, int m, int d, float* cost, void* ws,
                                         size_t ws_bytes, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  return emd_entry<float>("emd_nd_matchcost", b, n, m, d, ws, ws_bytes, st, {{cost, (size_t)b}},
                          [&](const EmdPlan& p, float* w) {
                            with_dim(d, [&](auto dc) {
                              launch_matchcost_nd<decltype(dc)::value>(p1, p2, match, b, n, m,
                                                                       cost, p, w, st);
                            });
                          });
}

extern "C" int pcfm_emd_nd_matchcost_bwd_f32(const float* grad_cost, const float* p1,
                                             const float* p2, const float* match, int b, int n,
                                             int m, int d, float* grad1, float* grad2, void* ws,
                                             size_t ws_bytes, void* stream) {
  const hipStream_t st = (hipStream_t)stream;
  return emd_entry<float>(
      "emd_nd_matchcost_bwd", b, n, m, d, ws, ws_bytes, st,
      {{grad1, (size_t)b * n * d}, {grad2, (size_t)b * m * d}}, [&](const EmdPlan& p, float* w) {
        with_dim(d, [&](auto dc) {
          launch_matchcost_bwd_nd<decltype(dc)::value>(grad_cost, p1, p2, match, b, n, m, grad1,
                                                       grad2, p, w, st);
        });
      });
}
