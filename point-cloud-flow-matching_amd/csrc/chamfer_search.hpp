// The brute-force nearest-neighbour search over D-component points, D in
// {2, 3, 5, 6}, once: what csrc/chamfer_nd.hip (nn_kernel<D>: pcfm_chamfer_fwd
// below its culling threshold and pcfm_chamfer_nd_fwd) and
// csrc/chamfer_cross.hip (cross_kernel<D>) are written over, so that all of
// them return the same bits for the same pair of points.
//   * each lane owns kQ = 8 query points in registers (8*D VGPRs);
//   * the candidate walk is wave-uniform, so candidates arrive through scalar
//     loads and every VALU op reads them straight from SGPRs (no LDS, no
//     per-lane address math), in groups of group_of(D) with the next group's
//     loads issued before the current group's arithmetic;
//   * plain scalar-per-lane fp32: the library is built without packed fp32
//     (csrc/Makefile NOPK).
#pragma once

#include "points.hpp"

namespace pcfm {

constexpr int kQ = 8;          // queries per lane
constexpr int kThreads = 256;  // 4 waves
constexpr int kPerBlock = kQ * kThreads;

// candidates per wave-uniform group load: a group and the prefetched next one
// are 2 * group_of(D) * D SGPRs, 48 at most
constexpr int group_of(int d) { return d <= 3 ? 8 : 4; }

// This lane's kQ queries: points qbase + q * kThreads + threadIdx.x of `cloud`
// (nq points).  A ragged tail reads the last point; the caller does not store it.
template <int D>
__device__ __forceinline__ void load_queries(const float* __restrict__ cloud, int nq, int qbase,
                                             float (&qv)[kQ][D]) {
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const int j = qbase + q * kThreads + threadIdx.x;
    const int jj = j < nq ? j : nq - 1;
    const float* p = cloud + (size_t)jj * D;
#pragma unroll
    for (int e = 0; e < D; ++e) qv[q][e] = p[e];
  }
}

// Candidates [k0, k1) of `cloud` (k0, k1 wave-uniform), in groups of
// kG = group_of(D): group(c, k, valid) sees candidates k .. k + kG - 1 in
// c[D * kG], of which the first `valid` exist (kG but for the ragged tail
// group, whose loads are clamped to candidate k1 - 1).
template <int D, class F>
__device__ __forceinline__ void walk_candidates(const float* __restrict__ cloud, int k0, int k1,
                                                F&& group) {
  constexpr int kG = group_of(D);
  const int kg1 = k0 + (k1 - k0) / kG * kG;
  int k = __builtin_amdgcn_readfirstlane(k0);
  if (k < kg1) {
    float c[D * kG], nx[D * kG];
#pragma unroll
    for (int e = 0; e < D * kG; ++e) c[e] = cloud[(size_t)D * k + e];
    for (; k < kg1; k += kG) {
      const int kn = k + kG < kg1 ? k + kG : k;
#pragma unroll
      for (int e = 0; e < D * kG; ++e) nx[e] = cloud[(size_t)D * kn + e];
      group(c, k, kG);
#pragma unroll
      for (int e = 0; e < D * kG; ++e) c[e] = nx[e];
    }
  }
  if (k < k1) {
    float c[D * kG];
#pragma unroll
    for (int e = 0; e < D * kG; ++e) c[e] = cloud[(size_t)D * min(k + e / D, k1 - 1) + e % D];
    group(c, k, k1 - k);
  }
}

// Host side of the brute-force search (csrc/chamfer_nd.hip), shared by the 3-D
// and the N-D entries; `what` names the entry in error texts.  The callers have
// checked their arguments.
size_t brute_workspace_bytes(int b, int n, int m);
int brute_fwd(const char* what, const float* p1, const float* p2, int b, int n, int m, int d,
              float* dist1, float* dist2, int* idx1, int* idx2, void* ws, hipStream_t st);
int brute_bwd(const char* what, const float* p1, const float* p2, int b, int n, int m, int d,
              const float* gd1, const float* gd2, const int* idx1, const int* idx2, float* g1,
              float* g2, hipStream_t st);

}  // namespace pcfm
