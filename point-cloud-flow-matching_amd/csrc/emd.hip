// Approximate EMD: approxmatch, matchcost and its gradient (include/pcfm.h).
//
// Reference: third_party/PyTorchEMD/cuda/emd_kernel.cu.  The reference runs
// the whole 10-level x 3-pass auction inside one block per batch element
// (<<<32,512>>>, emd_kernel.cu:186) and read-modify-writes the dense
// match[b, m, n] matrix once per level (:144).
//
// MI355X design:
//   * every pass of every level is a full-chip launch with its finalize
//     included: a block owns 64 rows (lanes), its 16 waves split the column
//     range (wave-uniform, so the column points arrive through scalar loads),
//     the wave sums of a row are added in a fixed order in LDS and the row's
//     finalize runs in the same block; a level's third pass and the next
//     level's first share one launch (21 launches per approxmatch);
//   * match is NOT accumulated level by level.  Each level only needs the
//     vectors ratioL (n) and ratioR (m), which are kept per level (10 x (n+m));
//     match is written once at the end as
//         match[l, k] = sum_j (exp(level_j * d2) * ratioL_j[k]) * ratioR_j[l]
//     summed in the reference's level order -- the same per-entry expression
//     and order as the reference's `match += w` (:143-144), with 1/10th of the
//     HBM traffic.
//   * exp is the hardware exp2 on x*log2(e): the reference is built with
//     --use_fast_math (__expf, backend.py:20), so EMD parity is tolerance-based
//     (tests/helpers/emd_ref.py is the fp64 reference of what is defined here).
//
// Measured history (B = 8, N = 2048, MI355X): the round-3 split form (6 launches
// per level, S-way partials reduced by separate finalize kernels; it can be
// built at the commit before this file lost it) 0.67 ms; a form with the
// finalizes folded into the next pass, each block re-reducing the S partials
// of its columns, 0.80 ms (the serial partial reads sat in front of every
// pass); the round-3 cooperative one-launch form with cooperative_groups grid
// barriers 4.45 ms (a grid.sync() costs ~0.1 us per block on ROCm 7.2, ~100 us
// at 1024 blocks, against ~1.7 us for a kernel boundary); the row passes as 30
// separate launches with scalar-loaded columns 0.51 ms, with LDS-staged columns
// and the fused cost 0.39 ms.
//
// The level table, emd_exp2, the finalize expressions, row_at, block_sum, the
// host plan, the prologue and the launch sequence are emd_core.hpp's, shared
// with the D-component kernels of emd_nd.hip.
#include "emd_core.hpp"

namespace pcfm {
namespace {

// cost partials: grid = (k blocks, S, b); part[(bb*S + s)*kblocks + kb].
template <typename T>
__global__ void __launch_bounds__(kEmdThreads)
    emd_cost_kernel(const T* __restrict__ xyz1, const T* __restrict__ xyz2,
                    const T* __restrict__ match, int b, int n, int m, int S,
                    T* __restrict__ part) {
  __shared__ T red[kEmdThreads / 64];
  const int bb = blockIdx.z, s = blockIdx.y;
  const int k = blockIdx.x * kEmdThreads + threadIdx.x;
  const T* p1 = xyz1 + row_at(bb, n, k) * 3;
  const T x1 = p1[0], y1 = p1[1], z1 = p1[2];
  const int l0 = (int)(((long long)m * s) / S), l1 = (int)(((long long)m * (s + 1)) / S);
  const T* __restrict__ cb = xyz2 + (size_t)bb * m * 3;
  T sub = 0;
  if (k < n) {
    for (int l = l0; l < l1; ++l) {
      const T d = sqdist3(cb[3 * l] - x1, cb[3 * l + 1] - y1, cb[3 * l + 2] - z1);
      sub = fmaT<T>(d, match[((size_t)bb * m + l) * n + k], sub);
    }
  }
  const T t = block_sum(sub, red);
  if (threadIdx.x == 0) part[((size_t)bb * S + s) * gridDim.x + blockIdx.x] = t;
}

// cost[bb] = sum of the batch element's per_b block partials (emd_cost_fin).
template <typename T>
__global__ void __launch_bounds__(64)
    emd_cost_fin_kernel(const T* __restrict__ part, int per_b, T* __restrict__ cost) {
  emd_cost_fin<T>(part, per_b, cost);
}

// The match write with matchcost fused (the fused forward, pcfm_emd_approxmatch_cost_*):
// match[b, l, k] = sum_j (exp(level_j * d2(k,l)) * ratioL_j[k]) * ratioR_j[l]
// in level order (skipped when match == nullptr), and per
// block the partial sum over its entries of d2 * match -- matchcost's terms
// (emd_kernel.cu:199-241) -- to part[(bb * lblocks + lb) * kblocks + kb], so
// the 4-byte-per-entry match matrix is not read back for the cost.  A block
// = 256 k (lanes, coalesced rows) x kMatchL l, the l points and their 10
// ratioR values staged in LDS.
template <typename T>
__global__ void __launch_bounds__(kEmdThreads)
    emd_match_cost_kernel(const T* __restrict__ xyz1, const T* __restrict__ xyz2, int b, int n,
                          int m, const T* __restrict__ levL, const T* __restrict__ levR,
                          T* __restrict__ match, T* __restrict__ part) {
  constexpr int kW = kLevels + 3;  // per l: ratioR_0..9, x, y, z
  __shared__ T sl[kMatchL * kW];
  __shared__ T red[kEmdThreads / 64];
  const int bb = blockIdx.z, kb = blockIdx.x, lb = blockIdx.y;
  const int k = kb * kEmdThreads + threadIdx.x;
  const int l0 = lb * kMatchL, nl = min(kMatchL, m - l0);
  for (int e = threadIdx.x; e < nl * kW; e += kEmdThreads) {
    const int li = e / kW, q = e - li * kW;
    sl[e] = q < kLevels ? levR[(size_t)q * b * m + (size_t)bb * m + l0 + li]
                        : xyz2[((size_t)bb * m + l0 + li) * 3 + (q - kLevels)];
  }
  const T* p1 = xyz1 + row_at(bb, n, k) * 3;
  const T x1 = p1[0], y1 = p1[1], z1 = p1[2];
  T rl[kLevels];
#pragma unroll
  for (int j = 0; j < kLevels; ++j) rl[j] = levL[(size_t)j * b * n + row_at(bb, n, k)];
  __syncthreads();
  T csum = 0;
  T* mrow = match != nullptr ? match + ((size_t)bb * m + l0) * n + k : nullptr;
  for (int li = 0; li < nl; ++li) {
    const T* q = sl + li * kW;
    const T d2 = sqdist3(q[kLevels] - x1, q[kLevels + 1] - y1, q[kLevels + 2] - z1);
    T acc = 0;
#pragma unroll
    for (int j = 0; j < kLevels; ++j) {
      const T e = j == kLevels - 1 ? (T)1 : emd_exp2<T>(d2, (T)level_log2e(j));  // level 0: 1
      acc += (e * rl[j]) * q[j];
    }
    if (mrow != nullptr && k < n) mrow[(size_t)li * n] = acc;
    csum = fmaT<T>(d2, acc, csum);
  }
  const T t = block_sum(k < n ? csum : (T)0, red);
  if (threadIdx.x == 0) part[((size_t)bb * gridDim.y + lb) * gridDim.x + kb] = t;
}

// grad1 partials: lanes over k, l split S ways: part[s][(bb*n + k)*3 + x].
template <typename T>
__global__ void __launch_bounds__(kEmdThreads)
    emd_grad1_kernel(const T* __restrict__ xyz1, const T* __restrict__ xyz2,
                     const T* __restrict__ match, int b, int n, int m, int S,
                     T* __restrict__ part) {
  const int bb = blockIdx.z, s = blockIdx.y;
  const int k = blockIdx.x * kEmdThreads + threadIdx.x;
  if (k >= n) return;
  const T* p1 = xyz1 + row_at(bb, n, k) * 3;
  const T x1 = p1[0], y1 = p1[1], z1 = p1[2];
  const int l0 = (int)(((long long)m * s) / S), l1 = (int)(((long long)m * (s + 1)) / S);
  const T* __restrict__ cb = xyz2 + (size_t)bb * m * 3;
  T dx = 0, dy = 0, dz = 0;
  for (int l = l0; l < l1; ++l) {
    const T d = match[((size_t)bb * m + l) * n + k] * (T)2;
    dx = fmaT<T>(x1 - cb[3 * l], d, dx);
    dy = fmaT<T>(y1 - cb[3 * l + 1], d, dy);
    dz = fmaT<T>(z1 - cb[3 * l + 2], d, dz);
  }
  T* o = part + (size_t)s * b * n * 3 + ((size_t)bb * n + k) * 3;
  o[0] = dx;
  o[1] = dy;
  o[2] = dz;
}

template <typename T>
__global__ void emd_grad1_fin_kernel(const T* __restrict__ part, int S, int b, int n,
                                     const T* __restrict__ gcost, T* __restrict__ grad1) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)b * n * 3;
  if (i >= total) return;
  const int bb = (int)(i / ((size_t)n * 3));
  grad1[i] = sum_parts(part, S, total, i) * gcost[bb];
}

// grad2: one block per (l, b); lanes stride over k, block reduce (:285-323).
template <typename T>
__global__ void __launch_bounds__(kEmdThreads)
    emd_grad2_kernel(const T* __restrict__ xyz1, const T* __restrict__ xyz2,
                     const T* __restrict__ match, const T* __restrict__ gcost, int n, int m,
                     T* __restrict__ grad2) {
  __shared__ T red[kEmdThreads / 64];
  const int l = blockIdx.x, bb = blockIdx.y;
  const T* p2 = xyz2 + ((size_t)bb * m + l) * 3;
  const T x2 = p2[0], y2 = p2[1], z2 = p2[2];
  const T* __restrict__ row = match + ((size_t)bb * m + l) * n;
  const T* __restrict__ pb = xyz1 + (size_t)bb * n * 3;
  T sx = 0, sy = 0, sz = 0;
  for (int k = threadIdx.x; k < n; k += kEmdThreads) {
    const T d = row[k] * (T)2;
    sx = fmaT<T>(x2 - pb[3 * k], d, sx);
    sy = fmaT<T>(y2 - pb[3 * k + 1], d, sy);
    sz = fmaT<T>(z2 - pb[3 * k + 2], d, sz);
  }
  const T tx = block_sum(sx, red);
  const T ty = block_sum(sy, red);
  const T tz = block_sum(sz, red);
  if (threadIdx.x == 0) {
    const T g = gcost[bb];
    T* o = grad2 + ((size_t)bb * m + l) * 3;
    o[0] = tx * g;
    o[1] = ty * g;
    o[2] = tz * g;
  }
}

// ---------------------------------------------------------------------------
// The row passes: ONE launch per pass of each level, its finalize included,
// and no partial-sum buffer.  A level's third pass and the next level's first
// pass walk the same (row k, column l) pairs, so they share one launch and one
// d2 per pair: 21 pass launches + the pack + the match write (with the cost fused).
// ---------------------------------------------------------------------------
// A point with the coefficient it carries into a pass (x, y, z, w = coef),
// float4 / double4: a native vector type, so copies stay in registers.
template <typename T>
struct Vec4Of;
template <>
struct Vec4Of<float> {
  using type = float4;
};
template <>
struct Vec4Of<double> {
  using type = double4;
};
template <typename T>
using Col4 = typename Vec4Of<T>::type;

// packK[b, k] = {xyz1, ratL};  packL0[b, l] = {xyz2, remR};  packL1[b, l] = {xyz2, ratR}
template <typename T>
struct EmdRowState {
  Col4<T>* packK;
  Col4<T>* packL0;
  Col4<T>* packL1;
  T* remL;
  T* levL;  // [kLevels][b * n]
  T* levR;  // [kLevels][b * m]
};

template <typename T>
__global__ void emd_pack_kernel(const T* __restrict__ xyz1, size_t bn, T multiL,
                                const T* __restrict__ xyz2, size_t bm, T multiR,
                                EmdRowState<T> s) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < bn) {
    s.packK[i] = Col4<T>(xyz1[3 * i], xyz1[3 * i + 1], xyz1[3 * i + 2], (T)0);
    s.remL[i] = multiL;
  }
  if (i < bm) {
    const T x = xyz2[3 * i], y = xyz2[3 * i + 1], z = xyz2[3 * i + 2];
    s.packL0[i] = Col4<T>(x, y, z, multiR);
    s.packL1[i] = Col4<T>(x, y, z, (T)0);
  }
}

// a wave's LDS chunk: kColChunk = 128 columns (64 for PH 3: two packs)
template <typename T, int PH>
__device__ __forceinline__ T rowpass_chunk(const Col4<T>* __restrict__ st, int cnt, T x1, T y1,
                                           T z1, T rl, T lvl2, T acc) {
  if (lvl2 == (T)0) {  // level 0: exp(0 * d2) = 1 exactly
#pragma unroll 8
    for (int c = 0; c < cnt; ++c) acc = fmaT<T>(PH == 2 ? rl : (T)1, st[c].w, acc);
    return acc;
  }
#pragma unroll 8
  for (int c = 0; c < cnt; ++c) {
    const Col4<T> q = st[c];
    const T d2 = sqdist3(q.x - x1, q.y - y1, q.z - z1);
    const T e = emd_exp2<T>(d2, lvl2);
    if constexpr (PH == 2) {
      acc = fmaT<T>(e * rl, q.w, acc);
    } else {
      acc = fmaT<T>(e, q.w, acc);
    }
  }
  return acc;
}

// PH 3 = PH 2 of level j fused with PH 0 of level j+1 (same rows k, same
// columns l, one d2 per pair): st[c] = {xyz2, ratR_j}, st[64 + c].w = remR_{j+1}
template <typename T>
__device__ __forceinline__ void rowpass_pair(const Col4<T>* __restrict__ st, int cnt, T x1, T y1,
                                             T z1, T rl, T lvl2, T lvl2b, T& acc2, T& acc0) {
#pragma unroll 8
  for (int c = 0; c < cnt; ++c) {
    const Col4<T> q = st[c];
    const T rr = st[64 + c].w;
    const T d2 = sqdist3(q.x - x1, q.y - y1, q.z - z1);
    const T e2 = emd_exp2<T>(d2, lvl2);
    const T e0 = emd_exp2<T>(d2, lvl2b);
    acc2 = fmaT<T>(e2 * rl, q.w, acc2);
    acc0 = fmaT<T>(e0, rr, acc0);
  }
}

// PH 0: rows k (packK), cols packL0 (coef remR);  suml -> ratL = remL / (1e-9 + suml)  (:57-81)
// PH 1: rows l (packL0), cols packK (coef ratL);  sumr -> ratR, levR[lvl], remR        (:86-116)
// PH 2: rows k (packK, row scale ratL), cols packL1 (coef ratR);  -> remL, levL[lvl]   (:119-151)
// PH 3: PH 2 of level lvl then PH 0 of level lvl+1 (lvl2b), one launch: the
//       column sums of both are taken in the same order as the two launches,
//       so the result is bit-identical (PCFM_EMD_FORM=unfused runs them apart).
// grid = (ceil(nr / 64), b), 1024 threads.  Each wave stages its column slice
// through a wave-private LDS chunk (16-B loads, the next chunk's loads in
// flight while this one is used); the column loop then reads a column as one
// broadcast ds_read, whose in-order completion lets the compiler keep several
// in flight (scalar loads of the columns complete out of order, so every use
// waited for all of them: 13.8 us/pass).
template <typename T, int PH>
__global__ void __launch_bounds__(64 * kRowWaves)
    emd_rowpass_kernel(int nr, int ncol, T lvl2, T lvl2b, int lvl, EmdRowState<T> s) {
  constexpr int CH = PH == 3 ? 64 : kColChunk;
  __shared__ T red[kRowWaves][64];
  __shared__ T red2[PH == 3 ? kRowWaves : 1][64];
  __shared__ Col4<T> stage[kRowWaves][kColChunk];
  Col4<T>* rows = PH == 1 ? s.packL0 : s.packK;
  const Col4<T>* __restrict__ cols = PH == 0 ? s.packL0 : (PH == 1 ? s.packK : s.packL1);
  const int bb = blockIdx.y, lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * 64 + lane;
  const Col4<T> rp = rows[row_at(bb, nr, i)];
  const T rl = rp.w;  // PH 2 / 3: ratL of the row
  const int c0 = (int)(((long long)ncol * w) / kRowWaves);
  const int c1 = (int)(((long long)ncol * (w + 1)) / kRowWaves);
  const Col4<T>* __restrict__ cb = cols + (size_t)bb * ncol;
  const Col4<T>* __restrict__ cb2 = s.packL0 + (size_t)bb * ncol;  // PH 3's remR_{lvl+1}
  Col4<T>* st = stage[w];
  T acc = 0, acc2 = 0;
  // unconditional loads (index clamped to the batch element's last column; the
  // extra columns are never read): no branch around a load in flight
  const int cl = ncol - 1;
  Col4<T> n0, n1;
  auto fetch = [&](int base) {
    n0 = cb[min(base + lane, cl)];
    n1 = PH == 3 ? cb2[min(base + lane, cl)] : cb[min(base + 64 + lane, cl)];
  };
  fetch(c0);
  for (int base = c0; base < c1; base += CH) {
    st[lane] = n0;
    st[64 + lane] = n1;
    fetch(base + CH);
    const int cnt = min(CH, c1 - base);
    if constexpr (PH == 3) {
      rowpass_pair<T>(st, cnt, rp.x, rp.y, rp.z, rl, lvl2, lvl2b, acc2, acc);
    } else {
      acc = rowpass_chunk<T, PH>(st, cnt, rp.x, rp.y, rp.z, rl, lvl2, acc);
    }
  }
  red[w][lane] = acc;
  if constexpr (PH == 3) red2[w][lane] = acc2;
  __syncthreads();
  if (w != 0 || i >= nr) return;
  T t = 0, t2 = 0;
#pragma unroll
  for (int q = 0; q < kRowWaves; ++q) {
    t += red[q][lane];
    if constexpr (PH == 3) t2 += red2[q][lane];
  }
  const size_t idx = (size_t)bb * nr + i;
  const size_t lv = (size_t)lvl * gridDim.y * nr + idx;
  if constexpr (PH == 0) {
    rows[idx].w = emd_ratio_l(s.remL[idx], t);
  } else if constexpr (PH == 1) {
    const T r = rp.w;
    const T sumr = t * r;  // sumr *= remainR (:111)
    const T rat = emd_ratio_r(r, sumr);
    s.packL1[idx].w = rat;
    s.levR[lv] = rat;
    rows[idx].w = emd_remain(r, sumr);
  } else {  // PH 2, and PH 3: level lvl's remainL, then level lvl+1's ratioL
    const T rem = emd_remain(s.remL[idx], PH == 3 ? t2 : t);
    s.remL[idx] = rem;
    s.levL[lv] = rl;
    if constexpr (PH == 3) rows[idx].w = emd_ratio_l(rem, t);
  }
}

// ---------------------------------------------------------------------------
// Host side: the plan (EmdPlan at d = 3), the prologue (emd_entry) and the
// launch sequence (emd_run_levels) are emd_core.hpp's; four entries.
// ---------------------------------------------------------------------------
static_assert(sizeof(Col4<float>) == 4 * sizeof(float) &&
              sizeof(Col4<double>) == 4 * sizeof(double));

// The 21 pass launches, then match (when non-null) and, when cost is non-null,
// the fused matchcost.  PCFM_EMD_FORM=unfused runs PH 2 and the next level's
// PH 0 as separate launches (31): what pins the fused PH 3 bit for bit.
template <typename T>
void launch_approxmatch(const T* xyz1, const T* xyz2, int b, int n, int m, T* match, T* cost,
                        const EmdPlan& p, T* ws, hipStream_t st) {
  auto pack = [ws](size_t at) { return reinterpret_cast<Col4<T>*>(ws + at); };
  const EmdRowState<T> s{pack(p.packK), pack(p.packL0), pack(p.packL1),
                         ws + p.remL,   ws + p.levL,    ws + p.levR};
  const T multiL = n >= m ? (T)1 : (T)(m / n);  // integer ratio of the cloud sizes (:27-33)
  const T multiR = n >= m ? (T)(n / m) : (T)1;
  hipLaunchKernelGGL(emd_pack_kernel<T>, grid1d(std::max(p.bn, p.bm)), dim3(256), 0, st, xyz1,
                     p.bn, multiL, xyz2, p.bm, multiR, s);
  const dim3 gL(ceil_div(n, 64), b), gR(ceil_div(m, 64), b), blk(64 * kRowWaves);
  auto lv2 = [](int j) { return (T)level_log2e(j); };
  emd_run_levels([&](auto ph, int j, int jn) {
    constexpr int PH = decltype(ph)::value;
    constexpr bool rows_k = PH != 1;  // PH 1's rows are the l points
    hipLaunchKernelGGL((emd_rowpass_kernel<T, PH>), rows_k ? gL : gR, blk, 0, st, rows_k ? n : m,
                       rows_k ? m : n, lv2(j), PH == 3 ? lv2(jn) : (T)0, j, s);
  });
  const dim3 gm(ceil_div(n, kEmdThreads), ceil_div(m, kMatchL), b);
  hipLaunchKernelGGL(emd_match_cost_kernel<T>, gm, dim3(kEmdThreads), 0, st, xyz1, xyz2, b, n, m,
                     (const T*)s.levL, (const T*)s.levR, match, ws + p.mpart);
  if (cost != nullptr)
    hipLaunchKernelGGL(emd_cost_fin_kernel<T>, dim3(b), dim3(64), 0, st, (const T*)(ws + p.mpart),
                       (int)(gm.x * gm.y), cost);
}

template <typename T>
int approxmatch(const T* xyz1, const T* xyz2, int b, int n, int m, T* match, void* ws,
                size_t ws_bytes, hipStream_t st) {
  return emd_entry<T>("approxmatch", b, n, m, 3, ws, ws_bytes, st, {}, [&](const EmdPlan& p, T* w) {
    launch_approxmatch<T>(xyz1, xyz2, b, n, m, match, nullptr, p, w, st);
  });
}

// approxmatch + matchcost in one call (the cost from the match kernel's
// partials).  match may be null: the cost alone, match not written.
template <typename T>
int approxmatch_cost(const T* xyz1, const T* xyz2, int b, int n, int m, T* match, T* cost,
                     void* ws, size_t ws_bytes, hipStream_t st) {
  PCFM_CHECK_ARG(cost != nullptr, "approxmatch_cost: cost is required");
  return emd_entry<T>("approxmatch_cost", b, n, m, 3, ws, ws_bytes, st, {{cost, (size_t)b}},
                      [&](const EmdPlan& p, T* w) {
                        launch_approxmatch<T>(xyz1, xyz2, b, n, m, match, cost, p, w, st);
                      });
}

template <typename T>
int matchcost(const T* xyz1, const T* xyz2, const T* match, int b, int n, int m, T* cost,
              void* ws, size_t ws_bytes, hipStream_t st) {
  return emd_entry<T>("matchcost", b, n, m, 3, ws, ws_bytes, st, {{cost, (size_t)b}},
                      [&](const EmdPlan& p, T* w) {
                        const dim3 g(ceil_div(n, kEmdThreads), p.S, b);
                        hipLaunchKernelGGL(emd_cost_kernel<T>, g, dim3(kEmdThreads), 0, st, xyz1,
                                           xyz2, match, b, n, m, p.S, w + p.part);
                        hipLaunchKernelGGL(emd_cost_fin_kernel<T>, dim3(b), dim3(64), 0, st,
                                           (const T*)(w + p.part), p.S * (int)g.x, cost);
                      });
}

template <typename T>
int matchcost_bwd(const T* gcost, const T* xyz1, const T* xyz2, const T* match, int b, int n,
                  int m, T* grad1, T* grad2, void* ws, size_t ws_bytes, hipStream_t st) {
  return emd_entry<T>(
      "matchcost_bwd", b, n, m, 3, ws, ws_bytes, st,
      {{grad1, (size_t)b * n * 3}, {grad2, (size_t)b * m * 3}}, [&](const EmdPlan& p, T* w) {
        hipLaunchKernelGGL(emd_grad1_kernel<T>, dim3(ceil_div(n, kEmdThreads), p.S, b),
                           dim3(kEmdThreads), 0, st, xyz1, xyz2, match, b, n, m, p.S, w + p.part);
        hipLaunchKernelGGL(emd_grad1_fin_kernel<T>, grid1d(p.bn * 3), dim3(256), 0, st,
                           (const T*)(w + p.part), p.S, b, n, gcost, grad1);
        hipLaunchKernelGGL(emd_grad2_kernel<T>, dim3(m, b), dim3(kEmdThreads), 0, st, xyz1, xyz2,
                           match, gcost, n, m, grad2);
      });
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" size_t pcfm_emd_workspace_bytes(int b, int n, int m, int elem_bytes) {
  if (b < 0 || n < 0 || m < 0 || (elem_bytes != 4 && elem_bytes != 8)) return 0;
  return EmdPlan(b, n, m, 3, (size_t)elem_bytes).bytes;
}

extern "C" int pcfm_emd_approxmatch_f32(const float* xyz1, const float* xyz2, int b, int n, int m,
                                        float* match, void* ws, size_t ws_bytes, void* stream) {
  return approxmatch<float>(xyz1, xyz2, b, n, m, match, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pcfm_emd_approxmatch_f64(const double* xyz1, const double* xyz2, int b, int n,
                                        int m, double* match, void* ws, size_t ws_bytes,
                                        void* stream) {
  return approxmatch<double>(xyz1, xyz2, b, n, m, match, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pcfm_emd_approxmatch_cost_f32(const float* xyz1, const float* xyz2, int b, int n,
                                             int m, float* match, float* cost, void* ws,
                                             size_t ws_bytes, void* stream) {
  return approxmatch_cost<float>(xyz1, xyz2, b, n, m, match, cost, ws, ws_bytes,
                                 (hipStream_t)stream);
}
extern "C" int pcfm_emd_approxmatch_cost_f64(const double* xyz1, const double* xyz2, int b, int n,
                                             int m, double* match, double* cost, void* ws,
                                             size_t ws_bytes, void* stream) {
  return approxmatch_cost<double>(xyz1, xyz2, b, n, m, match, cost, ws, ws_bytes,
                                  (hipStream_t)stream);
}
extern "C" int pcfm_emd_matchcost_f32(const float* xyz1, const float* xyz2, const float* match,
                                      int b, int n, int m, float* cost, void* ws,
                                      size_t ws_bytes, void* stream) {
  return matchcost<float>(xyz1, xyz2, match, b, n, m, cost, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pcfm_emd_matchcost_f64(const double* xyz1, const double* xyz2,
                                      const double* match, int b, int n, int m, double* cost,
                                      void* ws, size_t ws_bytes, void* stream) {
  return matchcost<double>(xyz1, xyz2, match, b, n, m, cost, ws, ws_bytes, (hipStream_t)stream);
}
extern "C" int pcfm_emd_matchcost_bwd_f32(const float* grad_cost, const float* xyz1,
                                          const float* xyz2, const float* match, int b, int n,
                                          int m, float* grad1, float* grad2, void* ws,
                                          size_t ws_bytes, void* stream) {
  return matchcost_bwd<float>(grad_cost, xyz1, xyz2, match, b, n, m, grad1, grad2, ws, ws_bytes,
                              (hipStream_t)stream);
}
extern "C" int pcfm_emd_matchcost_bwd_f64(const double* grad_cost, const double* xyz1,
                                          const double* xyz2, const double* match, int b, int n,
                                          int m, double* grad1, double* grad2, void* ws,
                                          size_t ws_bytes, void* stream) {
  return matchcost_bwd<double>(grad_cost, xyz1, xyz2, match, b, n, m, grad1, grad2, ws,
                               ws_bytes, (hipStream_t)stream);
}
