// Mean nearest-neighbour distances between two SETS of clouds of D-component
// points, D in {2, 3, 5, 6} (include/pcfm_chamfer_cross.h): the S x R matrices
// the generation metrics reduce (pcfm/metrics.py).
//
// The search is nn_kernel's (csrc/chamfer_nd.hip), over the same query load and
// candidate walk (csrc/chamfer_search.hpp), without everything a mean does not
// need -- no index, no candidate split, no key merge:
//   * a block owns kPerBlock = 2048 queries of ONE cloud, 8 per lane in
//     registers, and walks a tile of consecutive partner clouds of the other set;
//   * after each partner the block adds its minima in float64 in a fixed order
//     (a lane's 8 queries in order, the wave's 64 lanes by xor-butterfly, the 4
//     waves in wave order) and thread 0 stores the mean (one query block per
//     cloud) or the block's partial sum (more: cross_finalize_kernel adds the
//     partials in block order);
//   * both directions are one launch; the pairs are on grid.x.
// The minima are the fp32 values of pcfm_chamfer_nd_fwd (sqdist_nd; a min does
// not depend on the order its operands arrive in).
#include "pcfm_common.hpp"
#include "chamfer_search.hpp"

#include "../../include/pcfm_chamfer_cross.h"

#include <algorithm>

namespace pcfm {
namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kTileMax = 8;    // partner clouds per block, at most

// grid.x = the items of direction 0 (queries a_i, partners b_j -> ab) then of
// direction 1 (queries b_j, partners a_i -> ba); an item = (query cloud,
// partner tile of kt clouds, query block), the query block fastest.  part0 /
// part1 [output element][query blocks]: used when a cloud has more than one.
template <int D>
__global__ void __launch_bounds__(kThreads)
    cross_kernel(const float* __restrict__ a, const float* __restrict__ b, int s, int r, int n,
                 int m, int kt, int items0, float* __restrict__ ab, float* __restrict__ ba,
                 double* __restrict__ part0, double* __restrict__ part1) {
  constexpr int kG = group_of(D);
  __shared__ double red[2][kWaves];
  const bool second = blockIdx.x >= (unsigned)items0;
  const float* __restrict__ qp = second ? b : a;
  const float* __restrict__ cp = second ? a : b;
  float* __restrict__ out = second ? ba : ab;
  double* __restrict__ part = second ? part1 : part0;
  const int nq = second ? m : n, nc = second ? n : m;
  const int ncc = second ? s : r;               // partner clouds
  const int oq = second ? 1 : r, oc = second ? r : 1;  // out[query cloud * oq + partner * oc]
  const int qblocks = (nq + kPerBlock - 1) / kPerBlock;
  const int tiles = (ncc + kt - 1) / kt;
  int item = blockIdx.x - (second ? items0 : 0);
  const int qblk = item % qblocks;
  item /= qblocks;
  const int tile = item % tiles;
  const int qc = item / tiles;
  const int p0 = tile * kt;
  const int p1 = min(p0 + kt, ncc);
  const int qbase = qblk * kPerBlock;

  float qv[kQ][D];
  load_queries<D>(qp + (size_t)qc * nq * D, nq, qbase, qv);  // a ragged tail is not summed
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  for (int pc = p0; pc < p1; ++pc) {
    const float* __restrict__ cb = cp + (size_t)pc * nc * D;
    float best[kQ];
#pragma unroll
    for (int q = 0; q < kQ; ++q) best[q] = __builtin_inff();
    walk_candidates<D>(cb, 0, nc, [&](const float (&c)[D * kG], int, int valid) {
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
#pragma unroll
        for (int g = 0; g < kG; ++g) {
          float d = sqdist_nd<D>(&c[D * g], qv[q]);
          if (g >= valid) d = __builtin_inff();  // uniform: only the ragged tail group
          best[q] = __builtin_fminf(best[q], d);
        }
      }
    });

    // the block's sum, float64, fixed order
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int j = qbase + q * kThreads + threadIdx.x;
      acc += j < nq ? (double)best[q] : 0.0;
    }
    // wave_add written out: through the call the kernel is scheduled differently
    // ("What the point-cloud kernels share")
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    // two slots, alternating: thread 0 reads slot (pc & 1) before it arrives at
    // the next partner's barrier, and that slot is written again only after it
    double* slot = red[(pc - p0) & 1];
    if (lane == 0) slot[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = slot[0];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) t += slot[w];
      const size_t o = (size_t)qc * oq + (size_t)pc * oc;
      if (qblocks == 1) {
        out[o] = (float)(t / (double)nq);
      } else {
        part[o * qblocks + qblk] = t;
      }
    }
  }
}

// out[o] = (float)(sum of part[o][0 .. qblocks) in block order / nq)
__global__ void cross_finalize_kernel(const double* __restrict__ part, size_t total, int qblocks,
                                      int nq, float* __restrict__ out) {
  const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= total) return;
  double t = 0.0;
  for (int k = 0; k < qblocks; ++k) t += part[o * qblocks + k];
  out[o] = (float)(t / (double)nq);
}

// every [s, n] / [r, m] extent and the launch's block count fit 32-bit arithmetic
bool sizes_fit(int s, int r, int n, int m) {
  const long long lim = 1LL << 31;
  const long long qb = (long long)ceil_div(n, kPerBlock) + ceil_div(m, kPerBlock);
  return (long long)s * n < lim && (long long)r * m < lim && (long long)s * r < lim &&
         (long long)s * r * std::max(qb, 1LL) < lim;
}

// Partner clouds per block: 1 until the launch has 64 blocks per CU, then as
// many as keep it there (a block loads its queries once per tile), at most
// kTileMax.
int choose_tile(int s, int r, int n, int m) {
  const long long blocks =
      (long long)s * r * (ceil_div(n, kPerBlock) + ceil_div(m, kPerBlock));
  return (int)std::min<long long>(kTileMax, std::max<long long>(1, blocks / (64LL * kCUs)));
}

template <int D>
void launch(const float* a, const float* b, int s, int r, int n, int m, int kt, int items0,
            int items1, float* ab, float* ba, double* part0, double* part1, hipStream_t st) {
  hipLaunchKernelGGL(cross_kernel<D>, dim3(items0 + items1), dim3(kThreads), 0, st, a, b, s, r, n,
                     m, kt, items0, ab, ba, part0, part1);
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_chamfer_cross_abi_version(void) { return PCFM_CHAMFER_CROSS_ABI_VERSION; }

extern "C" int pcfm_chamfer_cross_supported(int d) { return point_dim_ok(d); }

extern "C" size_t pcfm_chamfer_cross_workspace_bytes(int s, int r, int n, int m, int d) {
  if (s <= 0 || r <= 0 || n <= 0 || m <= 0 || !pcfm_chamfer_cross_supported(d) ||
      !sizes_fit(s, r, n, m))
    return 0;
  const int qb0 = ceil_div(n, kPerBlock), qb1 = ceil_div(m, kPerBlock);
  return (size_t)s * r * ((qb0 > 1 ? qb0 : 0) + (qb1 > 1 ? qb1 : 0)) * sizeof(double);
}

extern "C" int pcfm_chamfer_cross_fwd(const float* a, const float* b, int s, int r, int n, int m,
                                      int d, float* ab, float* ba, void* ws, size_t ws_bytes,
                                      void* stream) {
  PCFM_CHECK_ARG(s >= 0 && r >= 0 && n >= 0 && m >= 0, "chamfer_cross_fwd: negative size");
  PCFM_CHECK_ARG(pcfm_chamfer_cross_supported(d), "chamfer_cross_fwd: unsupported dimension %d",
                 d);
  PCFM_CHECK_ARG(sizes_fit(s, r, n, m), "chamfer_cross_fwd: s = %d, r = %d, n = %d, m = %d too large",
                 s, r, n, m);
  PCFM_CHECK_ARG(ws_bytes >= pcfm_chamfer_cross_workspace_bytes(s, r, n, m, d),
                 "chamfer_cross_fwd: workspace %zu < %zu bytes", ws_bytes,
                 pcfm_chamfer_cross_workspace_bytes(s, r, n, m, d));
  if (s == 0 || r == 0) return PCFM_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t pairs = (size_t)s * r;
  if (n == 0 || m == 0) {
    // as pcfm_chamfer_nd_fwd: the outputs that exist are written 0
    hipError_t e = hipMemsetAsync(ab, 0, pairs * sizeof(float), st);
    if (e == hipSuccess) e = hipMemsetAsync(ba, 0, pairs * sizeof(float), st);
    if (e != hipSuccess) {
      set_error("chamfer_cross_fwd: hipMemsetAsync: %s", hipGetErrorString(e));
      return (int)e;
    }
    return PCFM_OK;
  }
  const int kt = choose_tile(s, r, n, m);
  const int qb0 = ceil_div(n, kPerBlock), qb1 = ceil_div(m, kPerBlock);
  const int t0 = ceil_div(r, kt), t1 = ceil_div(s, kt);
  double* part0 = (double*)ws;
  double* part1 = part0 + (qb0 > 1 ? pairs * qb0 : 0);
  const int items0 = s * t0 * qb0, items1 = r * t1 * qb1;  // <= s * r * (qb0 + qb1) < 2^31
  with_dim(d, [&](auto dc) {
    launch<decltype(dc)::value>(a, b, s, r, n, m, kt, items0, items1, ab, ba, part0, part1, st);
  });
  const dim3 fin(ceil_div((long long)pairs, 256));
  if (qb0 > 1)
    hipLaunchKernelGGL(cross_finalize_kernel, fin, dim3(256), 0, st, (const double*)part0, pairs,
                       qb0, n, ab);
  if (qb1 > 1)
    hipLaunchKernelGGL(cross_finalize_kernel, fin, dim3(256), 0, st, (const double*)part1, pairs,
                       qb1, m, ba);
  return check_launch("chamfer_cross_fwd");
}
