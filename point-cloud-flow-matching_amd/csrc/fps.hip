// Farthest-point sampling of a batch of clouds (include/pcfm_fps.h): m dependent
// rounds of "update every point's distance to the chosen set, take the farthest
// point", all in ONE launch, one block per cloud.
//
// Resident form (n <= kResident): thread t owns points t, t + T, ... (at most P,
// a template parameter) and keeps their k = min(d, 3) coordinates and running
// minima in registers for all m rounds; the cloud is read from memory once.  A
// round is
//   * the distance update over the owned points, which also keeps the thread's
//     farthest point (value, index, coordinates; a strict > over rising indices
//     keeps the lowest index among equals);
//   * a block-wide argmax of the key (float bits of dmin) << 32 | ~index: the
//     distances are >= +0, so the bits order like the values, and one unsigned
//     max yields the largest distance and, among equals, the lowest index.  The
//     key goes through a max-scan of cross-lane moves inside the wave (no LDS
//     traffic); the lane that holds the wave's maximum stores key and
//     coordinates to the wave's LDS slot; after
//     ONE barrier every thread reduces the 8 slots itself and so holds the
//     winner and its coordinates for the next round.  The slots are double
//     buffered: slot set (j & 1) is next written in round j + 2, after the
//     barrier of round j + 1, which every reader of round j has passed.
// No round reads global memory, and the only store is thread 0's idx[j].
// The gather into `out` is a tail loop of the same kernel.
//
// Streaming form (n > kResident): the same round, the running minima in the
// workspace (round 1 writes them without reading) and the coordinates read
// again from memory every round.  It exists so that every n works.
//
// A thread without a point (the ragged tail) holds key 0, which no point has
// (~index >= 2^31), and never stores to a slot; a wave without a point leaves
// its slot at the 0 the kernel starts with.  The index a round yields is always
// the index of a point some lane owns, whatever the coordinates hold.
#include "points.hpp"

#include "../../include/pcfm_fps.h"

namespace pcfm {
namespace {

constexpr int kFpsThreads = 512;    // 2 waves per SIMD: at most 256 VGPRs per lane
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsMaxP = 40;        // points per thread, at most: 4 * 40 registers of state
constexpr int kResident = kFpsThreads * kFpsMaxP;

struct FpsSlots {
  u64 key[2][kFpsWaves];
  float4 xyz[2][kFpsWaves];
};

template <int K>
__device__ __forceinline__ float fps_sqdist(const float (&p)[K], const float (&s)[K]) {
  if constexpr (K == 3) {
    return sqdist3(p[0] - s[0], p[1] - s[1], p[2] - s[2]);
  } else {
    const float d0 = p[0] - s[0], d1 = p[1] - s[1];
    return __builtin_fmaf(d0, d0, d1 * d1);
  }
}

__device__ __forceinline__ void fps_init_slots(FpsSlots& sm) {
  if (threadIdx.x < 2 * kFpsWaves) (&sm.key[0][0])[threadIdx.x] = 0;
  __syncthreads();
}

// The block's farthest point of round j: `key` / `c` are the thread's (key 0:
// the thread owns no point).  Returns the index, the coordinates in `sel`.
template <int K>
__device__ __forceinline__ int fps_block_argmax(FpsSlots& sm, int j, u64 key, const float (&c)[K],
                                                float (&sel)[K]) {
  const u64 wmax = wave_umax(key);
  const int buf = j & 1;
  if (key != 0 && key == wmax) {    // one lane of a wave that owns a point
    const int wave = threadIdx.x >> 6;
    sm.key[buf][wave] = key;
    sm.xyz[buf][wave] = make_float4(c[0], c[1], K == 3 ? c[K - 1] : 0.f, 0.f);
  }
  __syncthreads();
  u64 best = sm.key[buf][0];
  int w = 0;
#pragma unroll
  for (int s = 1; s < kFpsWaves; ++s) {
    const u64 k = sm.key[buf][s];
    if (k > best) {
      best = k;
      w = s;
    }
  }
  const float4 v = sm.xyz[buf][w];
  sel[0] = v.x;
  sel[1] = v.y;
  if constexpr (K == 3) sel[2] = v.z;
  return max_key_index(best);
}

// idx[0] and the coordinates of the first pick
template <int K>
__device__ __forceinline__ void fps_first(const float* __restrict__ cp, int n, int d,
                                          const int* __restrict__ start, int* __restrict__ ip,
                                          float (&sel)[K]) {
  int s0 = start ? start[blockIdx.x] : 0;
  s0 = min(max(s0, 0), n - 1);
#pragma unroll
  for (int k = 0; k < K; ++k) sel[k] = cp[(size_t)s0 * d + k];
  if (threadIdx.x == 0) ip[0] = s0;
}

// out[j][:] = pts[idx[j]][:], after the block's last idx store
__device__ __forceinline__ void fps_gather(const float* __restrict__ cp, int d, int m,
                                           const int* ip, float* __restrict__ op) {
  __syncthreads();   // thread 0's idx stores are visible to the block
  const size_t total = (size_t)m * d;
  for (size_t e = threadIdx.x; e < total; e += blockDim.x) {
    const size_t j = e / d;
    const int k = (int)(e - j * d);
    op[e] = cp[(size_t)ip[j] * d + k];
  }
}

template <int K, int P>
__global__ void __launch_bounds__(kFpsThreads)
    fps_resident_kernel(const float* __restrict__ pts, int n, int d, int m,
                        const int* __restrict__ start, int* idx, float* __restrict__ out) {
  __shared__ FpsSlots sm;
  const int T = blockDim.x, t = threadIdx.x;
  const float* __restrict__ cp = pts + (size_t)blockIdx.x * n * d;
  int* ip = idx + (size_t)blockIdx.x * m;

  // a point the thread does not own holds -inf: fmin keeps it and no > takes it
  float x[P][K], dm[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int i = t + p * T;
    const bool own = i < n;
#pragma unroll
    for (int k = 0; k < K; ++k) x[p][k] = own ? cp[(size_t)i * d + k] : 0.f;
    dm[p] = own ? __builtin_inff() : -__builtin_inff();
  }
  float sel[K];
  fps_first<K>(cp, n, d, start, ip, sel);
  fps_init_slots(sm);

  for (int j = 1; j < m; ++j) {
    float bv = -1.f, bc[K];
    int bp = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) bc[k] = 0.f;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      dm[p] = __builtin_fminf(dm[p], fps_sqdist<K>(x[p], sel));
      const bool far = dm[p] > bv;      // selects, not a branch per point
      bv = far ? dm[p] : bv;
      bp = far ? p : bp;
#pragma unroll
      for (int k = 0; k < K; ++k) bc[k] = far ? x[p][k] : bc[k];
    }
    const u64 key = t < n ? max_key(__float_as_uint(bv), t + bp * T) : 0;
    const int win = fps_block_argmax<K>(sm, j, key, bc, sel);
    if (t == 0) ip[j] = win;
  }
  if (out) fps_gather(cp, d, m, ip, out + (size_t)blockIdx.x * m * d);
}

template <int K>
__global__ void __launch_bounds__(kFpsThreads)
    fps_stream_kernel(const float* __restrict__ pts, int n, int d, int m,
                      const int* __restrict__ start, int* idx, float* __restrict__ out,
                      float* __restrict__ dmin) {
  __shared__ FpsSlots sm;
  const int T = blockDim.x, t = threadIdx.x;
  const float* __restrict__ cp = pts + (size_t)blockIdx.x * n * d;
  float* __restrict__ dp = dmin + (size_t)blockIdx.x * n;   // element i: thread i % T only
  int* ip = idx + (size_t)blockIdx.x * m;
  float sel[K];
  fps_first<K>(cp, n, d, start, ip, sel);
  fps_init_slots(sm);

  for (int j = 1; j < m; ++j) {
    float bv = -1.f, bc[K];
    int bi = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) bc[k] = 0.f;
#pragma unroll 4
    for (int i = t; i < n; i += T) {
      float p[K];
#pragma unroll
      for (int k = 0; k < K; ++k) p[k] = cp[(size_t)i * d + k];
      const float old = j == 1 ? __builtin_inff() : dp[i];
      const float now = __builtin_fminf(old, fps_sqdist<K>(p, sel));
      dp[i] = now;
      if (now > bv) {
        bv = now;
        bi = i;
#pragma unroll
        for (int k = 0; k < K; ++k) bc[k] = p[k];
      }
    }
    const u64 key = t < n ? max_key(__float_as_uint(bv), bi) : 0;
    const int win = fps_block_argmax<K>(sm, j, key, bc, sel);
    if (t == 0) ip[j] = win;
  }
  if (out) fps_gather(cp, d, m, ip, out + (size_t)blockIdx.x * m * d);
}

bool fps_sizes_fit(int b, int n, int m) {
  const long long lim = 1LL << 31;
  return (long long)b * n < lim && (long long)b * m < lim;
}

// Points per thread of the resident instance that takes n, and its block size:
// the smallest instance with P * 512 >= n, then as few whole waves as hold
// ceil(n / P) threads.
constexpr int kFpsP[] = {1, 2, 4, 8, 16, 24, 32, kFpsMaxP};

template <int K, int P>
void launch_resident(const float* pts, int b, int n, int d, int m, const int* start, int* idx,
                     float* out, hipStream_t st) {
  const int threads = ceil_div(ceil_div(n, P), 64) * 64;
  hipLaunchKernelGGL((fps_resident_kernel<K, P>), dim3(b), dim3(threads), 0, st, pts, n, d, m,
                     start, idx, out);
}

template <int K>
void launch(const float* pts, int b, int n, int d, int m, const int* start, int* idx, float* out,
            float* dmin, hipStream_t st) {
  if (n > kResident) {
    hipLaunchKernelGGL(fps_stream_kernel<K>, dim3(b), dim3(kFpsThreads), 0, st, pts, n, d, m,
                       start, idx, out, dmin);
    return;
  }
  int p = 0;
  while (kFpsP[p] * kFpsThreads < n) ++p;
  switch (kFpsP[p]) {
    case 1: launch_resident<K, 1>(pts, b, n, d, m, start, idx, out, st); break;
    case 2: launch_resident<K, 2>(pts, b, n, d, m, start, idx, out, st); break;
    case 4: launch_resident<K, 4>(pts, b, n, d, m, start, idx, out, st); break;
    case 8: launch_resident<K, 8>(pts, b, n, d, m, start, idx, out, st); break;
    case 16: launch_resident<K, 16>(pts, b, n, d, m, start, idx, out, st); break;
    case 24: launch_resident<K, 24>(pts, b, n, d, m, start, idx, out, st); break;
    case 32: launch_resident<K, 32>(pts, b, n, d, m, start, idx, out, st); break;
    default: launch_resident<K, kFpsMaxP>(pts, b, n, d, m, start, idx, out, st); break;
  }
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_fps_abi_version(void) { return PCFM_FPS_ABI_VERSION; }

extern "C" int pcfm_fps_supported(int d) { return point_dim_ok(d); }

extern "C" int pcfm_fps_resident_points(void) { return kResident; }

extern "C" size_t pcfm_fps_workspace_bytes(int b, int n, int m, int d) {
  if (b <= 0 || n <= 0 || m <= 0 || !pcfm_fps_supported(d) || !fps_sizes_fit(b, n, m)) return 0;
  return n > kResident ? (size_t)b * n * sizeof(float) : 0;
}

extern "C" int pcfm_fps(const float* pts, int b, int n, int d, int m, const int* start, int* idx,
                        float* out, void* ws, size_t ws_bytes, void* stream) {
  PCFM_CHECK_ARG(b >= 0 && n >= 0 && m >= 0, "fps: negative size");
  PCFM_CHECK_ARG(pcfm_fps_supported(d), "fps: unsupported dimension %d", d);
  PCFM_CHECK_ARG(n > 0 || b == 0 || m == 0, "fps: no point to sample from (n = 0)");
  PCFM_CHECK_ARG(fps_sizes_fit(b, n, m), "fps: b = %d, n = %d, m = %d too large", b, n, m);
  PCFM_CHECK_ARG(ws_bytes >= pcfm_fps_workspace_bytes(b, n, m, d),
                 "fps: workspace %zu < %zu bytes", ws_bytes,
                 pcfm_fps_workspace_bytes(b, n, m, d));
  if (b == 0 || m == 0) return PCFM_OK;
  hipStream_t st = (hipStream_t)stream;
  if (d == 2)
    launch<2>(pts, b, n, d, m, start, idx, out, (float*)ws, st);
  else
    launch<3>(pts, b, n, d, m, start, idx, out, (float*)ws, st);
  return check_launch("fps");
}
