// Assignment EMD by the parallel auction (include/pcfm_emd_auction.h states the
// rule): ONE launch per call, one 1024-thread block per pair of clouds, the whole
// auction -- every phase, every round -- inside the kernel, block barriers the
// only synchronisation, no atomics on global memory and no global traffic after
// the two clouds have been read once.
//
// Resident in LDS for the block's lifetime (n * (8 d + 24) bytes, 144 KiB at
// n = 2048, d = 6):
//   slot[n]      u64   per object: (float bits of the highest bid) << 32 | ~person
//   a[d][n]      f32   p1, one row per component (a lane's column reads have stride 1)
//   q[d][n]      f32   p2, likewise
//   price[n]     f32
//   owner[n]     i32   the person that holds object j, -1: nobody
//   assigned[n]  i32   the object person i holds; -1: unassigned; -2 - j: bid on j
//   list[n]      i32   the unassigned persons of the round, in no particular order
//
// A round is two barrier intervals:
//   BID    one wave per bidder (waves stride over the list).  The lanes scan the n
//          objects, 64 at a time, for the lowest and second-lowest
//          w(j) = c(i, j) + price[j] (= -v(j) of the rule: the same bits, the sign
//          turned); the wave's best is one unsigned max of the key
//          (~float bits of w) << 32 | ~j -- w >= +0, so the bits order like the
//          values, and the max is the lowest w and, among equals, the lowest j --
//          through wave_umax, the cross-lane max-scan; the second best is a second
//          max over "my second best where I hold the winner, my best elsewhere".
//          Lane 0 forms the bid and sends (bid bits) << 32 | ~i to slot[j1] with one
//          64-bit LDS max: the highest bid, the lowest person among equals,
//          whatever order the waves arrive in.
//   APPLY  thread per object: a slot whose bid bits differ from the price's took
//          a bid this round (a bid always exceeds the price, so a slot is never
//          cleared: what it holds from earlier rounds is the price itself, below
//          every later bid); the price becomes the bid, the winner the owner, the
//          previous owner goes to the next round's list.  Thread per person: a
//          bidder that finds itself in its object's slot is assigned, the others go
//          to the list.  The two loops touch disjoint persons (a previous owner did
//          not bid).
// The list is appended through an LDS counter: its order depends on the run, no
// result does (every bidder reads the prices of the round's start; every
// reduction is a max under a total order).
//
// The tail of a phase has one or two bidders per round: one wave scans per
// bidder, the other waves go straight to the barrier, and the round costs one
// scan of n objects (n / 64 steps per lane), two barriers and two passes of
// n / 1024 elements per thread.
//
// Nothing here trusts a float for an address: every index into LDS is a person or
// an object the code itself numbered, so non-finite coordinates change what is
// matched, never where anything is read or written.
#include "points.hpp"

#include <cmath>

#include "../../include/pcfm_emd_auction.h"

namespace pcfm {
namespace {

constexpr int kAucThreads = 1024;   // 4 waves per SIMD: at most 128 VGPRs per lane
constexpr int kAucWaves = kAucThreads / 64;
constexpr int kAucMaxPoints = 2048;

constexpr size_t auc_lds_bytes(int n, int d) { return (size_t)n * (8 * d + 24); }
static_assert(auc_lds_bytes(kAucMaxPoints, 6) <= (size_t)kLdsBytesMax - 1024,
              "the auction's state must fit the dynamic LDS cap");

// Point i of a cloud kept one row per component.
template <int D>
__device__ __forceinline__ void auc_point(const float* __restrict__ rows, int n, int i,
                                          float (&x)[D]) {
#pragma unroll
  for (int k = 0; k < D; ++k) x[k] = rows[k * n + i];
}

struct AucLds {
  u64* slot;
  float* a;
  float* q;
  float* price;
  int* owner;
  int* assigned;
  int* list;
};

// Person i's bid at increment eps, by the whole wave: sent to the slot of the
// object it names, and noted in assigned[i].
template <int D>
__device__ __forceinline__ void auc_bid(const AucLds& s, int n, int i, float eps, int lane) {
  float x[D];
  auc_point<D>(s.a, n, i, x);
  const float inf = __builtin_inff();
  float b1 = inf, b2 = inf;   // the lane's lowest and second-lowest w
  int j1 = lane;
#pragma unroll 4   // four objects' LDS reads in flight; the comparisons keep their order
  for (int j = lane; j < n; j += 64) {
    float y[D];
    auc_point<D>(s.q, n, j, y);
    const float w = sqdist_nd<D>(y, x) + s.price[j];
    const bool best = w < b1;           // strict, over rising j: the lowest index among equals
    b2 = best ? b1 : (w < b2 ? w : b2);
    b1 = best ? w : b1;
    j1 = best ? j : j1;
  }
  const u64 key = lane < n ? max_key(~__float_as_uint(b1), j1) : 0;
  const u64 kmax = wave_umax(key);
  u32 jb = (u32)max_key_index(kmax);
  jb = jb < (u32)n ? jb : (u32)(n - 1);
  const float w1 = __uint_as_float(~key_hi(kmax));
  const float other = key == kmax ? b2 : b1;   // a lane without an object holds +inf
  float w2 = __uint_as_float(~wave_umax((u32)~__float_as_uint(other)));
  if (n == 1) w2 = w1;
  if (lane == 0) {
    const float pj = s.price[jb];
    float bid = pj + ((w2 - w1) + eps);   // v1 - v2 = w2 - w1
    if (!(bid > pj)) bid = __uint_as_float(__float_as_uint(pj) + 1u);
    atomicMax(&s.slot[jb], max_key(__float_as_uint(bid), i));
    s.assigned[i] = -2 - (int)jb;
  }
}

template <int D>
__global__ void __launch_bounds__(kAucThreads)
    emd_auction_kernel(const float* __restrict__ p1, const float* __restrict__ p2, int n,
                       float eps_rel, int max_rounds, int* __restrict__ assignment,
                       float* __restrict__ cost, int* __restrict__ rounds) {
  extern __shared__ __align__(16) unsigned char auc_lds[];
  __shared__ int cnt[2];
  __shared__ float redf[kAucWaves];
  __shared__ double redd[kAucWaves];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const size_t pair = blockIdx.x;
  int* __restrict__ arow = assignment != nullptr ? assignment + pair * n : nullptr;
  if (n == 0) {
    if (t == 0) {
      cost[pair] = 0.0f;
      rounds[pair] = 0;
    }
    return;
  }
  AucLds s;
  s.slot = reinterpret_cast<u64*>(auc_lds);
  s.a = reinterpret_cast<float*>(s.slot + n);
  s.q = s.a + (size_t)D * n;
  s.price = s.q + (size_t)D * n;
  s.owner = reinterpret_cast<int*>(s.price + n);
  s.assigned = s.owner + n;
  s.list = s.assigned + n;

  const float* __restrict__ g1 = p1 + pair * n * D;
  const float* __restrict__ g2 = p2 + pair * n * D;
  for (int e = t; e < n * D; e += kAucThreads) {
    const int i = e / D, k = e - i * D;
    s.a[k * n + i] = g1[e];
    s.q[k * n + i] = g2[e];
  }
  for (int j = t; j < n; j += kAucThreads) {
    s.slot[j] = 0;
    s.price[j] = 0.0f;
  }
  __syncthreads();

  // cmax: two persons per thread share every object's broadcast reads
  float m = 0.0f;
  for (int i0 = t; i0 < n; i0 += 2 * kAucThreads) {
    const int i1 = min(i0 + kAucThreads, n - 1);
    float x0[D], x1[D];
    auc_point<D>(s.a, n, i0, x0);
    auc_point<D>(s.a, n, i1, x1);
    for (int j = 0; j < n; ++j) {
      float y[D];
      auc_point<D>(s.q, n, j, y);
      const float c0 = sqdist_nd<D>(y, x0), c1 = sqdist_nd<D>(y, x1);
      m = c0 > m ? c0 : m;   // a NaN is passed over
      m = c1 > m ? c1 : m;
    }
  }
  const u32 mw = wave_umax(__float_as_uint(m));   // m >= +0: the bits order like the values
  if (lane == 0) redf[wave] = __uint_as_float(mw);
  __syncthreads();
  float cmax = redf[0];
#pragma unroll
  for (int w = 1; w < kAucWaves; ++w) cmax = redf[w] > cmax ? redf[w] : cmax;

  if (cmax == 0.0f) {   // every cost is 0: the identity
    if (arow != nullptr)
      for (int i = t; i < n; i += kAucThreads) arow[i] = i;
    if (t == 0) {
      cost[pair] = 0.0f;
      rounds[pair] = 0;
    }
    return;
  }

  const float eps_final = eps_rel * cmax;
  float eps = fmaxf(eps_final, cmax * 0.5f);
  int nround = 0, cur = 0;
  bool finished = true;
  for (;;) {   // phases
    // cnt[cur] may still be read by a thread leaving the last round: start on the other
    cur ^= 1;
    for (int j = t; j < n; j += kAucThreads) {
      s.owner[j] = -1;
      s.assigned[j] = -1;
      s.list[j] = j;
    }
    if (t == 0) cnt[cur] = n;
    __syncthreads();
    for (;;) {   // rounds
      const int c = min(cnt[cur], n);
      if (c == 0) break;
      if (nround == max_rounds) {
        finished = false;
        break;
      }
      ++nround;
      // last read at the top of the round before, two barriers ago
      if (t == 0) cnt[cur ^ 1] = 0;
      for (int pos = wave; pos < c; pos += kAucWaves) auc_bid<D>(s, n, s.list[pos], eps, lane);
      __syncthreads();
      int* next = &cnt[cur ^ 1];
      for (int j = t; j < n; j += kAucThreads) {
        const u64 sl = s.slot[j];
        const u32 hb = key_hi(sl);
        if (hb != __float_as_uint(s.price[j])) {
          s.price[j] = __uint_as_float(hb);
          const int prev = s.owner[j];
          s.owner[j] = max_key_index(sl);
          if (prev >= 0) {
            s.assigned[prev] = -1;
            const int p = atomicAdd(next, 1);
            if (p < n) s.list[p] = prev;
          }
        }
      }
      for (int i = t; i < n; i += kAucThreads) {
        const int av = s.assigned[i];
        if (av <= -2) {
          const int j = -2 - av;
          if (max_key_index(s.slot[j]) == i) {
            s.assigned[i] = j;
          } else {
            s.assigned[i] = -1;
            const int p = atomicAdd(next, 1);
            if (p < n) s.list[p] = i;
          }
        }
      }
      __syncthreads();
      cur ^= 1;
    }
    if (!finished || eps == eps_final) break;
    eps = fmaxf(eps_final, eps * 0.25f);
  }

  if (!finished) {
    if (arow != nullptr)
      for (int i = t; i < n; i += kAucThreads) arow[i] = -1;
    if (t == 0) {
      cost[pair] = __builtin_nanf("");
      rounds[pair] = -1;
    }
    return;
  }
  // the cost in float64, in one fixed order: the thread's persons, the wave's
  // lanes, the block's waves
  double sum = 0.0;
  for (int i = t; i < n; i += kAucThreads) {
    const int j = s.assigned[i];
    if (arow != nullptr) arow[i] = j;
    if (j >= 0 && j < n) {
      float x[D], y[D];
      auc_point<D>(s.a, n, i, x);
      auc_point<D>(s.q, n, j, y);
      sum += (double)sqdist_nd<D>(y, x);
    }
  }
  wave_add(sum);
  if (lane == 0) redd[wave] = sum;
  __syncthreads();
  if (t == 0) {
    double total = redd[0];
#pragma unroll
    for (int w = 1; w < kAucWaves; ++w) total += redd[w];
    cost[pair] = (float)total;
    rounds[pair] = nround;
  }
}

template <int D>
int launch_auction(const float* p1, const float* p2, int b, int n, float eps_rel, int max_rounds,
                   int* assignment, float* cost, int* rounds, hipStream_t st) {
  const int e = allow_big_lds((const void*)emd_auction_kernel<D>);
  if (e) return e;
  hipLaunchKernelGGL(emd_auction_kernel<D>, dim3(b), dim3(kAucThreads), auc_lds_bytes(n, D), st,
                     p1, p2, n, eps_rel, max_rounds, assignment, cost, rounds);
  return check_launch("emd_auction");
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_emd_auction_abi_version(void) { return PCFM_EMD_AUCTION_ABI_VERSION; }

extern "C" int pcfm_emd_auction_max_points(int d) {
  return point_dim_ok(d) ? kAucMaxPoints : 0;
}

extern "C" size_t pcfm_emd_auction_workspace_bytes(int b, int n, int d) {
  (void)b;
  (void)n;
  (void)d;
  return 0;   // the state lives in LDS
}

extern "C" int pcfm_emd_auction_f32(const float* p1, const float* p2, int b, int n, int d,
                                    float eps_rel, int max_rounds, int* assignment, float* cost,
                                    int* rounds, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  PCFM_CHECK_ARG(b >= 0 && n >= 0, "emd_auction: negative size");
  PCFM_CHECK_ARG(pcfm_emd_auction_max_points(d) > 0, "emd_auction: unsupported dimension %d", d);
  PCFM_CHECK_ARG(n <= pcfm_emd_auction_max_points(d), "emd_auction: n = %d above the %d points "
                 "a block holds", n, pcfm_emd_auction_max_points(d));
  PCFM_CHECK_ARG(std::isfinite(eps_rel) && eps_rel >= 0x1p-20f && eps_rel <= 0.5f,
                 "emd_auction: eps_rel = %g outside [2^-20, 0.5]", (double)eps_rel);
  PCFM_CHECK_ARG(max_rounds >= 1, "emd_auction: max_rounds = %d below 1", max_rounds);
  PCFM_CHECK_ARG(b == 0 || (cost != nullptr && rounds != nullptr),
                 "emd_auction: cost and rounds are required");
  PCFM_CHECK_ARG(ws_bytes >= pcfm_emd_auction_workspace_bytes(b, n, d),
                 "emd_auction: workspace %zu < %zu bytes", ws_bytes,
                 pcfm_emd_auction_workspace_bytes(b, n, d));
  if (b == 0) return PCFM_OK;
  const hipStream_t st = (hipStream_t)stream;
  int rc = PCFM_OK;
  with_dim(d, [&](auto dc) {
    rc = launch_auction<decltype(dc)::value>(p1, p2, b, n, eps_rel, max_rounds, assignment, cost,
                                             rounds, st);
  });
  return rc;
}
