// What the approximate EMD is, once: the level table, the arithmetic of a
// level (exp, the three finalize expressions), the building blocks of the
// kernels, the host plan of the workspace, the prologue of an entry and the
// sequence of pass launches.  The kernels of csrc/emd.hip (include/pcfm.h: three
// components, float and double; include/pcfm_emd_nd.h: D = 2, 3, 5, 6
// components, float) are written over it.
#pragma once

#include "points.hpp"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <type_traits>
#include <utility>

namespace pcfm {

constexpr int kLevels = 10;
// level_j = -4^j for j = 7 .. -1, then 0 (emd_kernel.cu:44-48).
constexpr float h_levels[kLevels] = {-16384.0f, -4096.0f, -1024.0f, -256.0f, -64.0f,
                                     -16.0f,    -4.0f,    -1.0f,    -0.25f,  0.0f};
// level_j * log2(e) in one float factor.  level_j is a power of two, so
// d2 * (level_j * log2 e) rounds exactly as (level_j * d2) * log2 e.
constexpr float level_log2e(int j) { return h_levels[j] * 1.4426950408889634f; }

// exp(level * d2) as the hardware exp2 of float(d2) * lvl2, lvl2 = level * log2(e)
template <typename T>
__device__ __forceinline__ T emd_exp2(T d2, T lvl2) {
  return (T)__builtin_amdgcn_exp2f((float)d2 * (float)lvl2);
}

constexpr int kEmdThreads = 256;  // the match, cost and gradient kernels' block
constexpr int kMatchL = 32;       // columns l per block of the match write
constexpr int kRowWaves = 16;     // column splits per row-pass block, one wave each
constexpr int kColChunk = 128;    // 16-byte slots of a wave's LDS chunk

// Row i of batch element bb, clamped to the element's last row: a lane past
// the end loads a valid row unconditionally and its result is never stored.
__device__ __forceinline__ size_t row_at(int bb, int nr, int i) {
  const int ii = i < nr ? i : nr - 1;
  return (size_t)bb * nr + ii;
}

// The finalize expressions of a level; fminf / fmaxf take float arguments in
// the reference for both dtypes.
// ratioL = remainL / (1e-9 + suml)    (:57, :81)
template <typename T>
__device__ __forceinline__ T emd_ratio_l(T remL, T suml) {
  return remL / ((T)1e-9f + suml);
}
// consumption = min(remainR / (sumr + 1e-9), 1); ratioR = consumption * remainR   (:111-115)
template <typename T>
__device__ __forceinline__ T emd_ratio_r(T remR, T sumr) {
  return (T)fminf((float)(remR / (sumr + (T)1e-9f)), 1.0f) * remR;
}
// remain = max(0, remain - sum): remainR (:116) and remainL (:150)
template <typename T>
__device__ __forceinline__ T emd_remain(T rem, T sum) {
  return (T)fmaxf(0.0f, (float)(rem - sum));
}

template <typename T>
__device__ __forceinline__ T sum_parts(const T* part, int S, size_t stride, size_t i) {
  T v = 0;
  for (int s = 0; s < S; ++s) v += part[(size_t)s * stride + i];
  return v;
}

template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
  // wave_add written out: through the call the f32 kernels' slot store is
  // scheduled differently ("What the point-cloud kernels share")
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  T t = 0;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += red[i];
  return t;  // valid in thread 0
}

// cost[bb] = sum of the batch element's per_b block partials: one wave (the
// block) per batch element, lanes over strided partials, then a fixed xor tree
// (deterministic; the serial form was 9 us at 512 partials).
template <typename T>
__device__ __forceinline__ void emd_cost_fin(const T* __restrict__ part, int per_b,
                                             T* __restrict__ cost) {
  const int bb = blockIdx.x, lane = threadIdx.x;
  T t = 0;
  for (int i = lane; i < per_b; i += 64) t += part[(size_t)bb * per_b + i];
  wave_add(t);
  if (lane == 0) cost[bb] = t;
}

// ---------------------------------------------------------------------------
// Host side: one plan of the workspace, one prologue, one launch sequence.
// ---------------------------------------------------------------------------
// Elements of a pack: a point's d coordinates and the coefficient it carries
// into a pass, in whole 16-byte (float) slots -- one for d <= 3, two above.
constexpr int emd_pack_elems(int d) { return d <= 3 ? 4 : 8; }

// Column splits of matchcost's and matchcost_bwd's partials: ~4 waves per SIMD.
constexpr int emd_splits(int b, int n, int m) {
  const long long rows = (long long)b * std::max(n, m);
  const long long want_lanes = 4LL * kCUs * 4 * 64;
  int s = (int)std::max(1LL, (want_lanes + rows - 1) / std::max(1LL, rows));
  s = std::min(s, std::max(1, std::min(n, m) / 64));
  return std::max(1, std::min(s, 32));
}
constexpr size_t blocks_of(int count, int per) {
  return (size_t)((std::max(count, 1) + per - 1) / per);
}

// The workspace of every EMD entry over d components as offsets in elements
// of T.  The regions of approxmatch follow one another, each starting where the
// one before it ends.  The packs come first and each is a whole number of
// 4-element slots, so they are aligned whenever ws itself is aligned to a slot
// (16 B in f32, 32 B in f64), which every device allocation is -- whatever else
// the workspace holds.  matchcost and matchcost_bwd use nothing but their block
// partials, which therefore start at 0.
struct EmdPlan {
  int S = 1;  // emd_splits
  size_t bn = 0, bm = 0;
  size_t packK = 0, packL0 = 0, packL1 = 0;  // packs [bn], [bm], [bm]
  size_t remL = 0;                           // [bn]
  size_t levL = 0, levR = 0;                 // [kLevels][bn], [kLevels][bm]
  size_t mpart = 0, mpart_elems = 0;         // the match write's block partials
  size_t part = 0, part_elems = 0;           // the cost kernel's / grad1 kernel's partials
  size_t total = 0, bytes = 0;

  constexpr EmdPlan(int b, int n, int m, int d, size_t elem_bytes)
      : S(emd_splits(b, n, m)), bn((size_t)b * n), bm((size_t)b * m) {
    const size_t kblocks = blocks_of(n, kEmdThreads);
    const size_t pack = emd_pack_elems(d);
    mpart_elems = b * blocks_of(m, kMatchL) * kblocks;
    part_elems = std::max((size_t)b * S * kblocks, (size_t)S * bn * d);
    size_t end = 0;
    for (auto [region, elems] : {std::pair<size_t*, size_t>{&packK, pack * bn},
                                 {&packL0, pack * bm},
                                 {&packL1, pack * bm},
                                 {&remL, bn},
                                 {&levL, kLevels * bn},
                                 {&levR, kLevels * bm},
                                 {&mpart, mpart_elems}}) {
      *region = end;
      end += elems;
    }
    total = std::max(end, part + part_elems);
    bytes = total * elem_bytes;
  }
};

// the packs aligned, and the total the end of whichever region ends last
constexpr bool emd_plan_ok() {
  constexpr int sizes[] = {0, 1, 37, 64, 513, 2048, 20000};
  constexpr std::pair<int, size_t> forms[] = {{3, 4}, {3, 8}, {2, 4}, {5, 4}, {6, 4}};
  for (int b : sizes)
    for (int n : sizes)
      for (int m : sizes)
        for (auto [d, e] : forms) {
          const EmdPlan p(b, n, m, d, e);
          if (p.packK % 4 != 0 || p.packL0 % 4 != 0 || p.packL1 % 4 != 0) return false;
          if (p.total != std::max(p.mpart + p.mpart_elems, p.part + p.part_elems)) return false;
          if (p.bytes != p.total * e) return false;
        }
  return true;
}
static_assert(emd_plan_ok(), "EmdPlan: packs unaligned, or the total is not the last region's end");

template <typename T>
using EmdOut = std::pair<T*, size_t>;  // an output and its element count

// The prologue of every entry: argument and workspace checks, then either
// launch(plan, ws) or, for an empty problem, the outputs zero-filled.
template <typename T, typename Launch>
int emd_entry(const char* who, int b, int n, int m, int d, void* ws, size_t ws_bytes,
              hipStream_t st, std::initializer_list<EmdOut<T>> outs, Launch&& launch) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "%s: negative size", who);
  PCFM_CHECK_ARG(point_dim_ok(d), "%s: unsupported dimension %d", who, d);
  const EmdPlan p(b, n, m, d, sizeof(T));
  PCFM_CHECK_ARG(ws_bytes >= p.bytes, "%s: workspace %zu < %zu bytes", who, ws_bytes, p.bytes);
  if (b == 0) return PCFM_OK;
  if (n != 0 && m != 0) {
    launch(p, (T*)ws);
    return check_launch(who);
  }
  for (const EmdOut<T>& o : outs) {
    if (o.first == nullptr || o.second == 0) continue;
    const hipError_t e = hipMemsetAsync(o.first, 0, o.second * sizeof(T), st);
    if (e != hipSuccess) {
      set_error("%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
      return (int)e;
    }
  }
  return PCFM_OK;
}

inline dim3 grid1d(size_t total, int threads = 256) {
  return dim3(ceil_div((long long)std::max<size_t>(total, 1), threads));
}

// The row passes of approxmatch in launch order, pass(EmdPass<PH>, j, jn):
//   PH 0: level j's ratioL;  PH 1: level j's ratioR and remainR;
//   PH 2: level j's remainL; PH 3: PH 2 of level j and PH 0 of level jn = j + 1
//         in one launch.
// 21 launches; PCFM_EMD_FORM=unfused runs PH 2 and the next level's PH 0 apart
// (31): what pins the fused PH 3 bit for bit.
template <int PH>
using EmdPass = std::integral_constant<int, PH>;

template <class Pass>
void emd_run_levels(Pass&& pass) {
  const char* form = std::getenv("PCFM_EMD_FORM");
  const bool fused = form == nullptr || form[0] != 'u';
  pass(EmdPass<0>{}, 0, 0);
  for (int j = 0; j < kLevels; ++j) {
    pass(EmdPass<1>{}, j, 0);
    if (fused && j + 1 < kLevels) {
      pass(EmdPass<3>{}, j, j + 1);
    } else {
      pass(EmdPass<2>{}, j, 0);
      if (j + 1 < kLevels) pass(EmdPass<0>{}, j + 1, 0);
    }
  }
}

}  // namespace pcfm
