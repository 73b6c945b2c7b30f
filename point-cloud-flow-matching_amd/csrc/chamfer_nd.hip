// Chamfer nearest neighbours over D-component points, D in {2, 3, 5, 6}
// (include/pcfm_chamfer_nd.h): forward and backward.
//
// Reference: third_party/ChamferDistancePytorch/chamfer{2,5,6}D/ next to
// chamfer3D/ (same NmDistanceKernel with more components).  The structure is
// csrc/chamfer.hip's brute-force search, over D components:
//   * both directions are one launch (grid.z = 2*B);
//   * each lane owns kQ = 8 query points in registers; the candidate loop is
//     wave-uniform, so candidates arrive through scalar loads and every VALU
//     op reads them straight from SGPRs (no LDS, no per-lane address math);
//   * candidates come in groups of kG (8 for D <= 3, 4 for D = 5, 6: a group
//     and the prefetched next one are 2*kG*D SGPRs, 48 at most);
//   * a split candidate range merges through a 64-bit atomicMin on
//     (float bits of d) << 32 | index: d >= 0, so the packed order is "smaller
//     distance, then lower index" and does not depend on arrival order.
// The distance is ONE fixed fp32 chain (the build has -ffp-contract=off):
//   acc = d1*d1; acc = fma(d0, d0, acc); acc = fma(dk, dk, acc) for k = 2..D-1,
//   dk = candidate[k] - query[k].
// At D = 3 that is sqdist3 (pcfm_common.hpp), so the D = 3 instantiation returns
// the bits of pcfm_chamfer_fwd's brute-force search.  The reference's kernels
// for D != 3 mask their unrolled tail with `end_k & D` instead of `& 3`
// (SURVEY.md): not carried over, every candidate is scored here.
// No culled search: brute force at 8 x 20000^2, D = 6 is 2 * 8 * 20000^2 * 13
// lane-operations.
#include "pcfm_common.hpp"
#include "sqdist_nd.hpp"  // sqdist_nd<D>, group_of: shared with chamfer_cross.hip

#include "../../include/pcfm_chamfer_nd.h"

#include <algorithm>

namespace pcfm {
namespace {

constexpr int kQ = 8;          // queries per lane
constexpr int kThreads = 256;  // 4 waves
constexpr int kPerBlock = kQ * kThreads;

__device__ __forceinline__ unsigned long long pack_key(float d, int idx) {
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)idx;
}

// grid = (query blocks, splits, 2*b).  Per query only each group's minimum
// meets the running best; the exact index inside the winning group is
// recovered at the end (same chain, same bits, first equal one).  Strict `<`
// across groups and first-equal inside a group = a scan with strict `<`.
template <int D>
__global__ void __launch_bounds__(kThreads)
    nn_nd_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int b, int n, int m,
                 int splits, float* __restrict__ dist1, int* __restrict__ idx1,
                 float* __restrict__ dist2, int* __restrict__ idx2,
                 unsigned long long* __restrict__ key1, unsigned long long* __restrict__ key2) {
  constexpr int kG = group_of(D);
  const int dir = blockIdx.z >= (unsigned)b;
  const int bb = blockIdx.z - dir * b;
  const float* __restrict__ qp = dir ? p2 : p1;
  const float* __restrict__ cp = dir ? p1 : p2;
  const int nq = dir ? m : n;
  const int nc = dir ? n : m;
  const int qbase = blockIdx.x * kPerBlock;
  if (qbase >= nq) return;
  const int s = blockIdx.y;
  const int k0 = (int)(((long long)nc * s) / splits);
  const int k1 = (int)(((long long)nc * (s + 1)) / splits);

  float qv[kQ][D];
  float best[kQ];
  int gk[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const int j = qbase + q * kThreads + threadIdx.x;
    const int jj = j < nq ? j : nq - 1;
    const float* p = qp + ((size_t)bb * nq + jj) * D;
#pragma unroll
    for (int e = 0; e < D; ++e) qv[q][e] = p[e];
    best[q] = __builtin_inff();
    gk[q] = k0;
  }
  const float* __restrict__ cb = cp + (size_t)bb * nc * D;
  auto group = [&](const float (&c)[D * kG], int k, int valid) {
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      float gm = 0.0f;
#pragma unroll
      for (int g = 0; g < kG; ++g) {
        float d = sqdist_nd<D>(&c[D * g], qv[q]);
        if (g >= valid) d = __builtin_inff();  // uniform: only the ragged tail group
        gm = g == 0 ? d : __builtin_fminf(gm, d);
      }
      const bool better = gm < best[q];
      best[q] = better ? gm : best[q];
      gk[q] = better ? k : gk[q];
    }
  };
  const int kg1 = k0 + (k1 - k0) / kG * kG;
  int k = __builtin_amdgcn_readfirstlane(k0);
  if (k < kg1) {
    float c[D * kG], nx[D * kG];
#pragma unroll
    for (int e = 0; e < D * kG; ++e) c[e] = cb[(size_t)D * k + e];
    for (; k < kg1; k += kG) {
      const int kn = k + kG < kg1 ? k + kG : k;
#pragma unroll
      for (int e = 0; e < D * kG; ++e) nx[e] = cb[(size_t)D * kn + e];
      group(c, k, kG);
#pragma unroll
      for (int e = 0; e < D * kG; ++e) c[e] = nx[e];
    }
  }
  if (k < k1) {  // ragged tail: one partial group, loads clamped to the last candidate
    float c[D * kG];
#pragma unroll
    for (int e = 0; e < D * kG; ++e) c[e] = cb[(size_t)D * min(k + e / D, k1 - 1) + e % D];
    group(c, k, k1 - k);
  }
  float* __restrict__ dist = dir ? dist2 : dist1;
  int* __restrict__ idx = dir ? idx2 : idx1;
  unsigned long long* __restrict__ key = dir ? key2 : key1;
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    // exact index inside the query's winning group
    int found = gk[q];
    bool done = false;
    const int gend = min(gk[q] + kG, k1);
    for (int kk = gk[q]; kk < gend; ++kk) {
      float c[D];
#pragma unroll
      for (int e = 0; e < D; ++e) c[e] = cb[(size_t)D * kk + e];
      const float d = sqdist_nd<D>(c, qv[q]);
      if (!done && d == best[q]) {
        found = kk;
        done = true;
      }
    }
    const int j = qbase + q * kThreads + threadIdx.x;
    if (j >= nq) continue;
    const size_t o = (size_t)bb * nq + j;
    if (splits == 1) {
      dist[o] = best[q];
      idx[o] = found;
    } else {
      atomicMin(key + o, pack_key(best[q], found));
    }
  }
}

__global__ void nd_key_init_kernel(unsigned long long* __restrict__ key, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) key[i] = ~0ULL;
}

__global__ void nd_key_unpack_kernel(const unsigned long long* __restrict__ key, size_t total,
                                     float* __restrict__ dist, int* __restrict__ idx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) {
    const unsigned long long k = key[i];
    dist[i] = __uint_as_float((unsigned)(k >> 32));
    idx[i] = (int)(unsigned)(k & 0xffffffffu);
  }
}

// Backward: g = 2*grad_dist; own point += g*(q - p_nn), neighbour -= the same
// term, over d components.  Both directions in one launch, so both sides use
// float atomics.  An index outside [0, nc) is skipped.
__global__ void __launch_bounds__(256)
    nn_nd_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int b, int n,
                      int m, int d, const float* __restrict__ gd1, const float* __restrict__ gd2,
                      const int* __restrict__ idx1, const int* __restrict__ idx2,
                      float* __restrict__ g1, float* __restrict__ g2) {
  const int dir = blockIdx.y >= (unsigned)b;
  const int bb = blockIdx.y - dir * b;
  const int nq = dir ? m : n;
  const int nc = dir ? n : m;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= nq) return;
  const float* __restrict__ qp = dir ? p2 : p1;
  const float* __restrict__ cp = dir ? p1 : p2;
  const float* __restrict__ gd = dir ? gd2 : gd1;
  const int* __restrict__ ix = dir ? idx2 : idx1;
  float* gq = dir ? g2 : g1;
  float* gc = dir ? g1 : g2;
  const size_t o = (size_t)bb * nq + j;
  const int j2 = ix[o];
  if ((unsigned)j2 >= (unsigned)nc) return;
  const size_t oc = (size_t)bb * nc + j2;
  const float g = gd[o] * 2.0f;
  for (int e = 0; e < d; ++e) {
    const float t = g * (qp[o * d + e] - cp[oc * d + e]);
    atomicAdd(gq + o * d + e, t);
    atomicAdd(gc + oc * d + e, -t);
  }
}

// Candidate splits so that the launch has >= ~4 waves per SIMD (as
// csrc/chamfer.hip: the same kPerBlock, so the same splits for the same sizes).
int choose_splits(int b, int n, int m) {
  const long long qblocks = (long long)b * (ceil_div(n, kPerBlock) + ceil_div(m, kPerBlock));
  const long long want_blocks = 4LL * kCUs * 4;
  int s = (int)std::max(1LL, (want_blocks + qblocks - 1) / std::max(1LL, qblocks));
  const int cmin = std::max(1, std::min(n, m));
  s = std::min(s, std::max(1, cmin / 256));  // >= 256 candidates per split
  return std::min(s, 64);
}

// grid.z = 2*b and every [b, n] / [b, m] extent fits the kernels' arithmetic
bool sizes_fit(int b, int n, int m) {
  return b <= 32767 && (long long)b * std::max(n, m) < (1LL << 31);
}

template <int D>
void launch_fwd(const float* p1, const float* p2, int b, int n, int m, int splits, float* dist1,
                float* dist2, int* idx1, int* idx2, unsigned long long* key1,
                unsigned long long* key2, hipStream_t st) {
  dim3 grid(ceil_div(std::max(n, m), kPerBlock), splits, 2 * b);
  hipLaunchKernelGGL(nn_nd_kernel<D>, grid, dim3(kThreads), 0, st, p1, p2, b, n, m, splits, dist1,
                     idx1, dist2, idx2, key1, key2);
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_chamfer_nd_abi_version(void) { return PCFM_CHAMFER_ND_ABI_VERSION; }

extern "C" int pcfm_chamfer_nd_supported(int d) { return d == 2 || d == 3 || d == 5 || d == 6; }

extern "C" size_t pcfm_chamfer_nd_workspace_bytes(int b, int n, int m, int d) {
  if (b <= 0 || n < 0 || m < 0 || !pcfm_chamfer_nd_supported(d) || !sizes_fit(b, n, m)) return 0;
  if (n == 0 || m == 0 || choose_splits(b, n, m) == 1) return 0;
  return (size_t)b * ((size_t)n + m) * sizeof(unsigned long long);
}

extern "C" int pcfm_chamfer_nd_fwd(const float* p1, const float* p2, int b, int n, int m, int d,
                                   float* dist1, float* dist2, int* idx1, int* idx2, void* ws,
                                   size_t ws_bytes, void* stream) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "chamfer_nd_fwd: negative size");
  PCFM_CHECK_ARG(pcfm_chamfer_nd_supported(d), "chamfer_nd_fwd: unsupported dimension %d", d);
  PCFM_CHECK_ARG(sizes_fit(b, n, m), "chamfer_nd_fwd: b = %d, max(n, m) = %d too large", b,
                 std::max(n, m));
  PCFM_CHECK_ARG(ws_bytes >= pcfm_chamfer_nd_workspace_bytes(b, n, m, d),
                 "chamfer_nd_fwd: workspace %zu < %zu bytes", ws_bytes,
                 pcfm_chamfer_nd_workspace_bytes(b, n, m, d));
  if (b == 0) return PCFM_OK;
  hipStream_t st = (hipStream_t)stream;
  if (n == 0 || m == 0) {
    // as pcfm_chamfer_fwd: the outputs that exist are written 0
    hipError_t e = hipSuccess;
    if (n) e = hipMemsetAsync(dist1, 0, (size_t)b * n * 4, st);
    if (n && e == hipSuccess) e = hipMemsetAsync(idx1, 0, (size_t)b * n * 4, st);
    if (m && e == hipSuccess) e = hipMemsetAsync(dist2, 0, (size_t)b * m * 4, st);
    if (m && e == hipSuccess) e = hipMemsetAsync(idx2, 0, (size_t)b * m * 4, st);
    if (e != hipSuccess) {
      set_error("chamfer_nd_fwd: hipMemsetAsync: %s", hipGetErrorString(e));
      return (int)e;
    }
    return PCFM_OK;
  }
  const int splits = choose_splits(b, n, m);
  unsigned long long* key1 = nullptr;
  unsigned long long* key2 = nullptr;
  if (splits > 1) {
    key1 = (unsigned long long*)ws;
    key2 = key1 + (size_t)b * n;
    const size_t total = (size_t)b * ((size_t)n + m);
    hipLaunchKernelGGL(nd_key_init_kernel, dim3(ceil_div((long long)total, 256)), dim3(256), 0, st,
                       key1, total);
  }
  switch (d) {
    case 2: launch_fwd<2>(p1, p2, b, n, m, splits, dist1, dist2, idx1, idx2, key1, key2, st); break;
    case 3: launch_fwd<3>(p1, p2, b, n, m, splits, dist1, dist2, idx1, idx2, key1, key2, st); break;
    case 5: launch_fwd<5>(p1, p2, b, n, m, splits, dist1, dist2, idx1, idx2, key1, key2, st); break;
    default: launch_fwd<6>(p1, p2, b, n, m, splits, dist1, dist2, idx1, idx2, key1, key2, st); break;
  }
  if (splits > 1) {
    const size_t t1 = (size_t)b * n, t2 = (size_t)b * m;
    hipLaunchKernelGGL(nd_key_unpack_kernel, dim3(ceil_div((long long)t1, 256)), dim3(256), 0, st,
                       key1, t1, dist1, idx1);
    hipLaunchKernelGGL(nd_key_unpack_kernel, dim3(ceil_div((long long)t2, 256)), dim3(256), 0, st,
                       key2, t2, dist2, idx2);
  }
  return check_launch("chamfer_nd_fwd");
}

extern "C" int pcfm_chamfer_nd_bwd(const float* p1, const float* p2, int b, int n, int m, int d,
                                   const float* grad_dist1, const float* grad_dist2,
                                   const int* idx1, const int* idx2, float* grad_p1,
                                   float* grad_p2, void* stream) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "chamfer_nd_bwd: negative size");
  PCFM_CHECK_ARG(pcfm_chamfer_nd_supported(d), "chamfer_nd_bwd: unsupported dimension %d", d);
  PCFM_CHECK_ARG(sizes_fit(b, n, m), "chamfer_nd_bwd: b = %d, max(n, m) = %d too large", b,
                 std::max(n, m));
  if (b == 0 || n == 0 || m == 0) return PCFM_OK;
  dim3 grid(ceil_div(std::max(n, m), 256), 2 * b);
  hipLaunchKernelGGL(nn_nd_grad_kernel, grid, dim3(256), 0, (hipStream_t)stream, p1, p2, b, n, m,
                     d, grad_dist1, grad_dist2, idx1, idx2, grad_p1, grad_p2);
  return check_launch("chamfer_nd_bwd");
}
