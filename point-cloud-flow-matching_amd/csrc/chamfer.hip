// Chamfer-3D nearest neighbours (include/pcfm.h): the 3-D entries and the
// spatially culled search for large clouds.
//
// Reference: third_party/ChamferDistancePytorch/chamfer3D/chamfer3D.cu:12-195.
// Below the culling threshold the forward is the brute-force search shared
// with the N-D entries (brute_fwd at d = 3, csrc/chamfer_nd.hip over
// csrc/chamfer_search.hpp), and the backward is always brute_bwd at d = 3.
#include "pcfm_common.hpp"
#include "chamfer_search.hpp"
#include "segsum.hpp"

#include <algorithm>
#include <cstdlib>

namespace pcfm {
namespace {

// ---------------------------------------------------------------------------
// Spatially culled search (large clouds).  Brute force evaluates all N*M
// pairs at ~9 VALU lane-operations each, i.e. it is VALU-bound; here both
// clouds are put in Morton order over a common 32^3 grid (the stable segment
// sort of segsum.hip), candidates are cut into tiles of 64 consecutive sorted
// points with their bounding boxes, and a wave of 64 x kCQ consecutive sorted
// queries visits the tiles nearest in Morton order first and then every tile
// whose box can still hold a candidate at a distance <= the wave's worst
// current best (box lower bound, with a 1e-5 relative margin against
// rounding).  A skipped tile provably holds only strictly farther candidates,
// and every visited candidate is scored with the same sqdist3 as the oracle,
// keeping (smaller distance, then lower ORIGINAL index) -- the reference's
// answer, bit for bit (chamfer3D.cu:36-68, :126).
// ---------------------------------------------------------------------------
constexpr int kCG = 32;        // Morton grid per axis
constexpr int kCTile = 64;     // candidates per tile
constexpr int kCQ = 2;         // queries per lane
constexpr int kCWaves = 4;     // waves per block (independent)

__device__ __forceinline__ unsigned spread3(unsigned v) {  // 5 bits -> every 3rd bit
  v &= 31u;
  v = (v | (v << 8)) & 0x0000f00fu;
  v = (v | (v << 4)) & 0x000c30c3u;
  v = (v | (v << 2)) & 0x00249249u;
  return v;
}

// per batch element: bbox of xyz1 U xyz2 -> lo[3], scale[3] (cells per unit)
__global__ void __launch_bounds__(1024)
    cham_bbox_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n, int m,
                     float* __restrict__ grid) {
  const int b = blockIdx.x;
  float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
  for (int i = threadIdx.x; i < n + m; i += 1024) {
    const float* p = i < n ? xyz1 + ((size_t)b * n + i) * 3 : xyz2 + ((size_t)b * m + i - n) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], p[a]);
      hi[a] = fmaxf(hi[a], p[a]);
    }
  }
  __shared__ float red[6][16];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64));
    }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[a][w] = lo[a];
      red[3 + a][w] = hi[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    float l = red[a][0], h = red[3 + a][0];
    for (int g = 1; g < 16; ++g) {
      l = fminf(l, red[a][g]);
      h = fmaxf(h, red[3 + a][g]);
    }
    const float ext = h - l;
    grid[b * 6 + a] = l;
    grid[b * 6 + 3 + a] = ext > 0.0f ? (float)kCG / ext : 0.0f;
  }
}

// Morton key of every point of one cloud on its batch element's grid
__global__ void __launch_bounds__(256)
    cham_key_kernel(const float* __restrict__ xyz, int n, const float* __restrict__ grid,
                    int* __restrict__ key) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = xyz + ((size_t)b * n + i) * 3;
  unsigned c[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float f = (p[a] - grid[b * 6 + a]) * grid[b * 6 + 3 + a];
    c[a] = (unsigned)min(kCG - 1, max(0, (int)f));  // NaN -> 0
  }
  key[(size_t)b * n + i] = (int)(spread3(c[0]) << 2 | spread3(c[1]) << 1 | spread3(c[2]));
}

// sorted[b, rank[i]] = (x, y, z, i)
__global__ void __launch_bounds__(256)
    cham_place_kernel(const float* __restrict__ xyz, int n, const int* __restrict__ rank,
                      float4* __restrict__ sorted) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = xyz + ((size_t)b * n + i) * 3;
  sorted[(size_t)b * n + rank[(size_t)b * n + i]] =
      make_float4(p[0], p[1], p[2], __int_as_float(i));
}

// tile boxes of the sorted points: box[b, t] = {lo xyz, hi xyz} (two float4)
__global__ void __launch_bounds__(256)
    cham_tiles_kernel(const float4* __restrict__ sorted, int n, int tiles,
                      float4* __restrict__ box) {
  const int b = blockIdx.y;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (t >= tiles) return;
  const int i = t * kCTile + lane;
  float4 p = sorted[(size_t)b * n + min(i, n - 1)];
  float lx = p.x, ly = p.y, lz = p.z, hx = p.x, hy = p.y, hz = p.z;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lx = fminf(lx, __shfl_xor(lx, o, 64));
    ly = fminf(ly, __shfl_xor(ly, o, 64));
    lz = fminf(lz, __shfl_xor(lz, o, 64));
    hx = fmaxf(hx, __shfl_xor(hx, o, 64));
    hy = fmaxf(hy, __shfl_xor(hy, o, 64));
    hz = fmaxf(hz, __shfl_xor(hz, o, 64));
  }
  if (lane == 0) {
    box[((size_t)b * tiles + t) * 2] = make_float4(lx, ly, lz, 0.0f);
    box[((size_t)b * tiles + t) * 2 + 1] = make_float4(hx, hy, hz, 0.0f);
  }
}

// grid = (ceil(max(n,m) / (64 kCQ kCWaves)), 1, 2b).  s1/s2: sorted clouds,
// box1/box2 their tile boxes, st1/st2 the sort's start[] (Morton cell -> first
// sorted position).
//   phase 1: the kNear tiles around the wave's place in the candidates' Morton
//            order, unconditionally -> a finite worst-best `wmax`;
//   phase 2: 64 tiles at a time, lane l tests tile g0 + l's box against the
//            wave's query box (one vector load + a few VALU ops for 64 tiles);
//            the set bits are visited in order, each re-tested against the
//            shrinking wmax first.
// A visited tile's 64 candidates arrive as ONE coalesced float4 load (lane =
// candidate) and are broadcast to the wave with v_readlane (no per-candidate
// memory latency in the inner loop).
constexpr int kNear = 2;  // phase-1 tiles on each side of the start tile

__global__ void __launch_bounds__(64 * kCWaves)
    nn_cull_kernel(const float4* __restrict__ s1, const float4* __restrict__ s2,
                   const float4* __restrict__ box1, const float4* __restrict__ box2,
                   const int* __restrict__ st1, const int* __restrict__ st2,
                   const float* __restrict__ grid, int b, int n, int m,
                   float* __restrict__ dist1, int* __restrict__ idx1,
                   float* __restrict__ dist2, int* __restrict__ idx2) {
  const int dir = blockIdx.z >= (unsigned)b;
  const int bb = blockIdx.z - dir * b;
  const int nq = dir ? m : n, nc = dir ? n : m;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int q0 = (blockIdx.x * kCWaves + w) * 64 * kCQ;
  if (q0 >= nq) return;  // wave-uniform
  const float4* __restrict__ qs = (dir ? s2 : s1) + (size_t)bb * nq;
  const float4* __restrict__ cs = (dir ? s1 : s2) + (size_t)bb * nc;
  const int tiles = (nc + kCTile - 1) / kCTile;
  const float4* __restrict__ cbox = (dir ? box1 : box2) + (size_t)bb * tiles * 2;
  const int* __restrict__ cst = (dir ? st1 : st2) + (size_t)bb * (kCG * kCG * kCG + 1);

  float qx[kCQ], qy[kCQ], qz[kCQ], best[kCQ];
  int qi[kCQ], bi[kCQ];
  float lx = __builtin_inff(), ly = lx, lz = lx, hx = -lx, hy = -lx, hz = -lx;
#pragma unroll
  for (int j = 0; j < kCQ; ++j) {
    const int q = q0 + j * 64 + lane;
    const float4 p = qs[min(q, nq - 1)];
    qx[j] = p.x;
    qy[j] = p.y;
    qz[j] = p.z;
    qi[j] = q < nq ? __float_as_int(p.w) : -1;
    best[j] = __builtin_inff();
    bi[j] = 0;
    lx = fminf(lx, p.x); ly = fminf(ly, p.y); lz = fminf(lz, p.z);
    hx = fmaxf(hx, p.x); hy = fmaxf(hy, p.y); hz = fmaxf(hz, p.z);
  }
  lx = wave_min(lx); ly = wave_min(ly); lz = wave_min(lz);
  hx = wave_max(hx); hy = wave_max(hy); hz = wave_max(hz);
  int t0;
  {  // the tile where the wave's first query's Morton cell starts among the candidates
    const float4 p = qs[q0];
    const float pc[3] = {p.x, p.y, p.z};
    unsigned c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float f = (pc[a] - grid[bb * 6 + a]) * grid[bb * 6 + 3 + a];
      c[a] = (unsigned)min(kCG - 1, max(0, (int)f));
    }
    const int key = (int)(spread3(c[0]) << 2 | spread3(c[1]) << 1 | spread3(c[2]));
    t0 = __builtin_amdgcn_readfirstlane(min(tiles - 1, cst[key] / kCTile));
  }

  auto visit = [&](int t) {
    const int k = t * kCTile + lane;
    const float4 c = cs[min(k, nc - 1)];
    const int cnt = min(kCTile, nc - t * kCTile);
    for (int e = 0; e < cnt; ++e) {
      const float x = rlf(c.x, e), y = rlf(c.y, e), z = rlf(c.z, e);
      const int ci = __builtin_amdgcn_readlane(__float_as_int(c.w), e);
#pragma unroll
      for (int j = 0; j < kCQ; ++j) {
        // dx = candidate - query (chamfer3D.cu:32-35); lowest original index on ties
        const float d = sqdist3(x - qx[j], y - qy[j], z - qz[j]);
        if (d < best[j] || (d == best[j] && ci < bi[j])) {
          best[j] = d;
          bi[j] = ci;
        }
      }
    }
    float mx = 0.0f;
#pragma unroll
    for (int j = 0; j < kCQ; ++j) mx = fmaxf(mx, qi[j] >= 0 ? best[j] : 0.0f);
    return wave_max(mx);
  };

  const int n0 = max(0, t0 - kNear), n1 = min(tiles, t0 + kNear + 1);
  float wmax = __builtin_inff();
  for (int t = n0; t < n1; ++t) wmax = visit(t);
  for (int g0 = 0; g0 < tiles; g0 += 64) {
    const int t = g0 + lane;
    float lb = __builtin_inff();
    if (t < tiles && (t < n0 || t >= n1)) {
      const float4 blo = cbox[2 * t], bhi = cbox[2 * t + 1];
      const float dx = fmaxf(0.0f, fmaxf(blo.x - hx, lx - bhi.x));
      const float dy = fmaxf(0.0f, fmaxf(blo.y - hy, ly - bhi.y));
      const float dz = fmaxf(0.0f, fmaxf(blo.z - hz, lz - bhi.z));
      // a skipped tile's candidates are all strictly farther than wmax: 1e-5
      // relative margin over the rounding of lb and of the candidates' sqdist3
      lb = (dx * dx + dy * dy + dz * dz) * (1.0f - 1e-5f);
    }
    unsigned long long need = __ballot(lb <= wmax);
    while (need) {
      const int l = __ffsll((long long)need) - 1;
      need &= need - 1;
      if (rlf(lb, l) > wmax) continue;
      // finer test, per query: does the tile's box come within ANY query's own
      // current best?  (the wave box against the wave's worst best passes whole
      // tiles that none of the wave's queries can use -- Gaussian clouds put
      // dense and sparse queries in one wave)
      const int t = g0 + l;
      const float4 blo = cbox[2 * t], bhi = cbox[2 * t + 1];
      bool use = false;
#pragma unroll
      for (int j = 0; j < kCQ; ++j) {
        const float dx = fmaxf(0.0f, fmaxf(blo.x - qx[j], qx[j] - bhi.x));
        const float dy = fmaxf(0.0f, fmaxf(blo.y - qy[j], qy[j] - bhi.y));
        const float dz = fmaxf(0.0f, fmaxf(blo.z - qz[j], qz[j] - bhi.z));
        use = use || (qi[j] >= 0 && (dx * dx + dy * dy + dz * dz) * (1.0f - 1e-5f) <= best[j]);
      }
      if (__ballot(use)) wmax = visit(t);
    }
  }
  float* __restrict__ dist = (dir ? dist2 : dist1) + (size_t)bb * nq;
  int* __restrict__ idx = (dir ? idx2 : idx1) + (size_t)bb * nq;
#pragma unroll
  for (int j = 0; j < kCQ; ++j) {
    if (qi[j] >= 0) {
      dist[qi[j]] = best[j];
      idx[qi[j]] = bi[j];
    }
  }
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

namespace {
// Culled search from this many pairs per batch element.  Brute force runs at
// the VALU issue rate (~7 lane-operations per pair); the culled search scores
// a pair at ~14 (index tie-break, lane broadcasts) and visits a fraction of
// the candidates that depends on the cloud.  Measured on MI355X (round 2, with
// the per-query tile test): C2 (8 x 20000^2, randn) brute 0.90 ms vs culled
// 1.06 ms; C5 (4 x 100000^2) culled 2.25 ms (randn) / 1.51 ms (uniform) vs
// ~11 ms brute; the reference's published 32 x 2000 x 1000: brute 0.08 ms vs
// culled 0.38 ms.  PCFM_CHAMFER_CULL_PAIRS overrides the threshold
// (tests force both paths on the same inputs).
long long cull_pairs() {
  static const long long v = [] {
    const char* e = getenv("PCFM_CHAMFER_CULL_PAIRS");
    return e != nullptr ? atoll(e) : (2LL << 30);
  }();
  return v;
}

bool use_cull(int n, int m) { return (long long)n * m >= cull_pairs() && n >= 256 && m >= 256; }

struct CullWs {
  float* grid;      // B * 6
  int* key1;        // B * n
  int* key2;        // B * m
  int* st1;         // B * (G^3 + 1)
  int* st2;
  int* rank1;       // B * n
  int* rank2;       // B * m
  float4* s1;       // B * n
  float4* s2;       // B * m
  float4* box1;     // B * tiles1 * 2
  float4* box2;     // B * tiles2 * 2
};

size_t cull_ws(int b, int n, int m, CullWs* w) {
  const size_t V1 = (size_t)kCG * kCG * kCG + 1;
  const size_t t1 = (n + kCTile - 1) / kCTile, t2 = (m + kCTile - 1) / kCTile;
  const size_t parts[] = {(size_t)b * 6 * 4, (size_t)b * n * 4, (size_t)b * m * 4, b * V1 * 4,
                          b * V1 * 4, (size_t)b * n * 4, (size_t)b * m * 4, (size_t)b * n * 16,
                          (size_t)b * m * 16, b * t1 * 32, b * t2 * 32};
  size_t off = 0;
  void* ptrs[11];
  for (int i = 0; i < 11; ++i) {
    ptrs[i] = (void*)off;
    off += align256(parts[i]);
  }
  if (w != nullptr) {
    char* base = (char*)w->grid;
    w->grid = (float*)(base + (size_t)ptrs[0]);
    w->key1 = (int*)(base + (size_t)ptrs[1]);
    w->key2 = (int*)(base + (size_t)ptrs[2]);
    w->st1 = (int*)(base + (size_t)ptrs[3]);
    w->st2 = (int*)(base + (size_t)ptrs[4]);
    w->rank1 = (int*)(base + (size_t)ptrs[5]);
    w->rank2 = (int*)(base + (size_t)ptrs[6]);
    w->s1 = (float4*)(base + (size_t)ptrs[7]);
    w->s2 = (float4*)(base + (size_t)ptrs[8]);
    w->box1 = (float4*)(base + (size_t)ptrs[9]);
    w->box2 = (float4*)(base + (size_t)ptrs[10]);
  }
  return off;
}

int chamfer_cull(const float* xyz1, const float* xyz2, int b, int n, int m, float* dist1,
                 float* dist2, int* idx1, int* idx2, void* ws, hipStream_t st) {
  CullWs w;
  w.grid = (float*)ws;
  cull_ws(b, n, m, &w);
  const int V = kCG * kCG * kCG;
  hipLaunchKernelGGL(cham_bbox_kernel, dim3(b), dim3(1024), 0, st, xyz1, xyz2, n, m, w.grid);
  hipLaunchKernelGGL(cham_key_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, xyz1, n, w.grid,
                     w.key1);
  hipLaunchKernelGGL(cham_key_kernel, dim3(ceil_div(m, 256), b), dim3(256), 0, st, xyz2, m, w.grid,
                     w.key2);
  int e = seg_sort(w.key1, (long long)n, b, n, V, 0, w.st1, nullptr, nullptr, w.rank1, st);
  if (e) return e;
  e = seg_sort(w.key2, (long long)m, b, m, V, 0, w.st2, nullptr, nullptr, w.rank2, st);
  if (e) return e;
  hipLaunchKernelGGL(cham_place_kernel, dim3(ceil_div(n, 256), b), dim3(256), 0, st, xyz1, n,
                     w.rank1, w.s1);
  hipLaunchKernelGGL(cham_place_kernel, dim3(ceil_div(m, 256), b), dim3(256), 0, st, xyz2, m,
                     w.rank2, w.s2);
  const int t1 = ceil_div(n, kCTile), t2 = ceil_div(m, kCTile);
  hipLaunchKernelGGL(cham_tiles_kernel, dim3(ceil_div(t1, 4), b), dim3(256), 0, st, w.s1, n, t1,
                     w.box1);
  hipLaunchKernelGGL(cham_tiles_kernel, dim3(ceil_div(t2, 4), b), dim3(256), 0, st, w.s2, m, t2,
                     w.box2);
  const int per_block = 64 * kCQ * kCWaves;
  hipLaunchKernelGGL(nn_cull_kernel, dim3(ceil_div(std::max(n, m), per_block), 1, 2 * b),
                     dim3(64 * kCWaves), 0, st, w.s1, w.s2, w.box1, w.box2, w.st1, w.st2, w.grid,
                     b, n, m, dist1, idx1, dist2, idx2);
  return check_launch("chamfer_fwd (culled)");
}
}  // namespace

extern "C" size_t pcfm_chamfer_workspace_bytes(int b, int n, int m) {
  if (b <= 0 || n < 0 || m < 0) return 0;
  if (use_cull(n, m)) return cull_ws(b, n, m, nullptr);
  return brute_workspace_bytes(b, n, m);
}

extern "C" int pcfm_chamfer_fwd(const float* xyz1, const float* xyz2, int b, int n, int m,
                                float* dist1, float* dist2, int* idx1, int* idx2, void* ws,
                                size_t ws_bytes, void* stream) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "chamfer_fwd: negative size");
  PCFM_CHECK_ARG(ws_bytes >= pcfm_chamfer_workspace_bytes(b, n, m),
                 "chamfer_fwd: workspace %zu < %zu bytes", ws_bytes,
                 pcfm_chamfer_workspace_bytes(b, n, m));
  hipStream_t st = (hipStream_t)stream;
  if (b > 0 && use_cull(n, m))
    return chamfer_cull(xyz1, xyz2, b, n, m, dist1, dist2, idx1, idx2, ws, st);
  return brute_fwd("chamfer_fwd", xyz1, xyz2, b, n, m, 3, dist1, dist2, idx1, idx2, ws, st);
}

extern "C" int pcfm_chamfer_bwd(const float* xyz1, const float* xyz2, int b, int n, int m,
                                const float* grad_dist1, const float* grad_dist2, const int* idx1,
                                const int* idx2, float* grad_xyz1, float* grad_xyz2,
                                void* stream) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "chamfer_bwd: negative size");
  return brute_bwd("chamfer_bwd", xyz1, xyz2, b, n, m, 3, grad_dist1, grad_dist2, idx1, idx2,
                   grad_xyz1, grad_xyz2, (hipStream_t)stream);
}
