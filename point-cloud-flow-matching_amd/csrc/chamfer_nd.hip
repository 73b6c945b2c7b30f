// Brute-force Chamfer nearest neighbours over D-component points, D in
// {2, 3, 5, 6}, forward and backward: the N-D entries
// (include/pcfm_chamfer_nd.h) and, through brute_fwd / brute_bwd at d = 3, the
// 3-D ones of csrc/chamfer.hip.
//
// Reference: third_party/ChamferDistancePytorch/chamfer{2,3,5,6}D/ (one
// NmDistanceKernel per dimension; chamfer3D.cu:12-195).  The reference runs a
// <<<(32,16),512>>> grid per direction in which only B*16 blocks work, with
// 512-point LDS tiles read by every thread.  Here:
//   * both directions are one launch (grid.z = 2*B);
//   * queries in registers, candidates as wave-uniform grouped scalar loads
//     (csrc/chamfer_search.hpp);
//   * when B*N queries alone cannot fill 256 CUs the candidate range is split
//     and the per-split winners merge through a 64-bit atomicMin on
//     (float bits of d) << 32 | index: "smaller distance, then lower index" --
//     the reference's tie rule (strict `<` inside a tile, chamfer3D.cu:36-68,
//     strict `>` across tiles, :126).
// The distance is sqdist_nd<D>, at D = 3 the oracle's sqdist3.  The reference's
// kernels for D != 3 mask their unrolled tail with `end_k & D` instead of `& 3`
// (SURVEY.md): not carried over, every candidate is scored here.
#include "pcfm_common.hpp"
#include "chamfer_search.hpp"

#include "../../include/pcfm_chamfer_nd.h"

#include <algorithm>

namespace pcfm {
namespace {

// grid = (query blocks, splits, 2*b).  Per query only each group's MINIMUM
// meets the running best (min3 chains: ~0.5 VALU op per pair instead of a
// compare + two selects per pair), which keeps the group's first candidate
// index; the exact index inside the winning group is recovered at the end by
// recomputing its kG distances (same chain, same bits) and taking the first
// equal one.  Strict `<` across groups and first-equal inside a group = the
// reference's scan order.
template <int D>
__global__ void __launch_bounds__(kThreads)
    nn_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int b, int n, int m,
              int splits, float* __restrict__ dist1, int* __restrict__ idx1,
              float* __restrict__ dist2, int* __restrict__ idx2,
              unsigned long long* __restrict__ key1, unsigned long long* __restrict__ key2) {
  constexpr int kG = group_of(D);
  const int dir = blockIdx.z >= (unsigned)b;
  const int bb = blockIdx.z - dir * b;
  const int nq = dir ? m : n;
  const int nc = dir ? n : m;
  const int qbase = blockIdx.x * kPerBlock;
  if (qbase >= nq) return;
  const int s = blockIdx.y;
  const int k0 = (int)(((long long)nc * s) / splits);
  const int k1 = (int)(((long long)nc * (s + 1)) / splits);
  const float* __restrict__ cb = (dir ? p1 : p2) + (size_t)bb * nc * D;

  float qv[kQ][D];
  load_queries<D>((dir ? p2 : p1) + (size_t)bb * nq * D, nq, qbase, qv);
  float best[kQ];
  int gk[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    best[q] = __builtin_inff();
    gk[q] = k0;
  }
  walk_candidates<D>(cb, k0, k1, [&](const float (&c)[D * kG], int k, int valid) {
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
  });
  // exact index inside each query's winning group
  int bi[kQ];
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
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
    bi[q] = found;
  }
  float* __restrict__ dist = dir ? dist2 : dist1;
  int* __restrict__ idx = dir ? idx2 : idx1;
  unsigned long long* __restrict__ key = dir ? key2 : key1;
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const int j = qbase + q * kThreads + threadIdx.x;
    if (j >= nq) continue;
    const size_t o = (size_t)bb * nq + j;
    if (splits == 1) {
      dist[o] = best[q];
      idx[o] = bi[q];
    } else {
      // d >= 0: the smaller distance, then the lower index, whatever the arrival order
      atomicMin(key + o, min_key(__float_as_uint(best[q]), bi[q]));
    }
  }
}

__global__ void key_init_kernel(unsigned long long* __restrict__ key, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) key[i] = ~0ULL;
}

__global__ void key_unpack_kernel(const unsigned long long* __restrict__ key, size_t total,
                                  float* __restrict__ dist, int* __restrict__ idx) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) {
    const unsigned long long k = key[i];
    dist[i] = __uint_as_float(key_hi(k));
    idx[i] = min_key_index(k);
  }
}

// Backward: g = 2*grad_dist; own point += g*(q - p_nn), neighbour -= the same
// term (chamfer3D.cu:155-174), over D components.  Both directions in one
// launch, so both sides use float atomics, as the reference does.  An index
// outside [0, nc) is skipped.
template <int D>
__global__ void __launch_bounds__(256)
    nn_grad_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int b, int n, int m,
                   const float* __restrict__ gd1, const float* __restrict__ gd2,
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
  float t[D];
#pragma unroll
  for (int e = 0; e < D; ++e) t[e] = g * (qp[o * D + e] - cp[oc * D + e]);
#pragma unroll
  for (int e = 0; e < D; ++e) atomicAdd(gq + o * D + e, t[e]);
#pragma unroll
  for (int e = 0; e < D; ++e) atomicAdd(gc + oc * D + e, -t[e]);
}

// Candidate splits so that the launch has >= ~4 waves per SIMD.
int choose_splits(int b, int n, int m) {
  const long long qblocks = (long long)b * (ceil_div(n, kPerBlock) + ceil_div(m, kPerBlock));
  const long long want_blocks = 4LL * kCUs * 4;  // 4 blocks of 4 waves per CU, x4 slack
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
  hipLaunchKernelGGL(nn_kernel<D>, grid, dim3(kThreads), 0, st, p1, p2, b, n, m, splits, dist1,
                     idx1, dist2, idx2, key1, key2);
}

template <int D>
void launch_bwd(const float* p1, const float* p2, int b, int n, int m, const float* gd1,
                const float* gd2, const int* idx1, const int* idx2, float* g1, float* g2,
                hipStream_t st) {
  dim3 grid(ceil_div(std::max(n, m), 256), 2 * b);
  hipLaunchKernelGGL(nn_grad_kernel<D>, grid, dim3(256), 0, st, p1, p2, b, n, m, gd1, gd2, idx1,
                     idx2, g1, g2);
}

}  // namespace

// one key per point of both clouds when the candidate range is split
size_t brute_workspace_bytes(int b, int n, int m) {
  if (choose_splits(b, n, m) == 1) return 0;
  return (size_t)b * ((size_t)n + m) * sizeof(unsigned long long);
}

int brute_fwd(const char* what, const float* p1, const float* p2, int b, int n, int m, int d,
              float* dist1, float* dist2, int* idx1, int* idx2, void* ws, hipStream_t st) {
  if (b == 0) return PCFM_OK;
  if (n == 0 || m == 0) {
    // The reference leaves its zero-initialised outputs untouched: the outputs
    // that exist are written 0.
    hipError_t e = hipSuccess;
    if (n) e = hipMemsetAsync(dist1, 0, (size_t)b * n * 4, st);
    if (n && e == hipSuccess) e = hipMemsetAsync(idx1, 0, (size_t)b * n * 4, st);
    if (m && e == hipSuccess) e = hipMemsetAsync(dist2, 0, (size_t)b * m * 4, st);
    if (m && e == hipSuccess) e = hipMemsetAsync(idx2, 0, (size_t)b * m * 4, st);
    if (e != hipSuccess) {
      set_error("%s: hipMemsetAsync: %s", what, hipGetErrorString(e));
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
    hipLaunchKernelGGL(key_init_kernel, dim3(ceil_div((long long)total, 256)), dim3(256), 0, st,
                       key1, total);
  }
  with_dim(d, [&](auto dc) {
    launch_fwd<decltype(dc)::value>(p1, p2, b, n, m, splits, dist1, dist2, idx1, idx2, key1, key2,
                                    st);
  });
  if (splits > 1) {
    const size_t t1 = (size_t)b * n, t2 = (size_t)b * m;
    hipLaunchKernelGGL(key_unpack_kernel, dim3(ceil_div((long long)t1, 256)), dim3(256), 0, st,
                       key1, t1, dist1, idx1);
    hipLaunchKernelGGL(key_unpack_kernel, dim3(ceil_div((long long)t2, 256)), dim3(256), 0, st,
                       key2, t2, dist2, idx2);
  }
  return check_launch(what);
}

int brute_bwd(const char* what, const float* p1, const float* p2, int b, int n, int m, int d,
              const float* gd1, const float* gd2, const int* idx1, const int* idx2, float* g1,
              float* g2, hipStream_t st) {
  if (b == 0 || n == 0 || m == 0) return PCFM_OK;
  with_dim(d, [&](auto dc) {
    launch_bwd<decltype(dc)::value>(p1, p2, b, n, m, gd1, gd2, idx1, idx2, g1, g2, st);
  });
  return check_launch(what);
}

}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_chamfer_nd_abi_version(void) { return PCFM_CHAMFER_ND_ABI_VERSION; }

extern "C" int pcfm_chamfer_nd_supported(int d) { return point_dim_ok(d); }

extern "C" size_t pcfm_chamfer_nd_workspace_bytes(int b, int n, int m, int d) {
  if (b <= 0 || n < 0 || m < 0 || !pcfm_chamfer_nd_supported(d) || !sizes_fit(b, n, m)) return 0;
  return brute_workspace_bytes(b, n, m);
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
  return brute_fwd("chamfer_nd_fwd", p1, p2, b, n, m, d, dist1, dist2, idx1, idx2, ws,
                   (hipStream_t)stream);
}

extern "C" int pcfm_chamfer_nd_bwd(const float* p1, const float* p2, int b, int n, int m, int d,
                                   const float* grad_dist1, const float* grad_dist2,
                                   const int* idx1, const int* idx2, float* grad_p1,
                                   float* grad_p2, void* stream) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "chamfer_nd_bwd: negative size");
  PCFM_CHECK_ARG(pcfm_chamfer_nd_supported(d), "chamfer_nd_bwd: unsupported dimension %d", d);
  PCFM_CHECK_ARG(sizes_fit(b, n, m), "chamfer_nd_bwd: b = %d, max(n, m) = %d too large", b,
                 std::max(n, m));
  return brute_bwd("chamfer_nd_bwd", p1, p2, b, n, m, d, grad_dist1, grad_dist2, idx1, idx2,
                   grad_p1, grad_p2, (hipStream_t)stream);
}
