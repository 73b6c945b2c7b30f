// Occupancy counts of a set of clouds on an r^3 grid (include/pcfm_occupancy.h):
// every point of every cloud goes to one kept node, the nodes are counted.
//
// Count kernel: a bounded number of persistent blocks (OccPlan: at most one per
// CU, a function of s * n alone).  A block keeps a private histogram of r^3
// uint32 in dynamic LDS (87 808 bytes at r = 28, 128 KiB at r = 32: the block is
// its CU's only resident workgroup, hence 1024 threads), zeroes it, strides over
// the s * n points one point per thread and round, and adds with LDS integer
// adds.  At the end it stores its r^3 partial counts to its slice of the
// workspace: every word of the slice is written, so the workspace needs no
// memset, and the zero / flush is paid once per block, not once per cloud.
//
// A point's node is rint of its grid coordinates if that node is kept (branch 1);
// otherwise (branch 2) the nearest kept node, lowest flat index among equals.
// Branch 2 keeps no candidate list: the nodes are implicit in three wave-uniform
// loops, the integer kept-test runs on the scalar side (per (i, j) the kept k
// are one interval, symmetric about the centre, walked in rising order), and a
// strict < over rising flat indices keeps the lowest index.  The walk costs
// about ten thousand node evaluations per lane at r = 28 whether one lane of
// the wave needs it or all 64, so the points that need it are queued: in a
// round every thread either adds its point to the histogram (branch 1) or
// appends its grid coordinates to a ring in LDS (2048 entries, 24 KiB behind the
// histogram).  Once 1024 entries wait, the block walks the nodes for them in one
// packed pass, every lane of every wave busy; what is left at the end (fewer
// than 1024) takes one last pass of as many waves as it fills.  The walks are
// then proportional to the number of branch-2 points, not to the number of
// waves that hold one.  The order of the ring depends on the run; the counts,
// being integers, do not.
//
// Finalize kernel: counts[f] = the sum over the blocks of their partial f (the
// pattern of cross_finalize_kernel in chamfer_cross.hip).  Integer sums: no
// float atomics, no global atomics, and the result does not depend on the number
// of blocks.
//
// Loads: a thread reads the three position floats of its row (one 12-byte load)
// at a stride of d floats.  A wave's 64 rows are contiguous, so every fetched
// line is used in full at d = 3 and to one half at d = 6, where the colour
// shares the line.
#include "points.hpp"

#include "../../include/pcfm_occupancy.h"

namespace pcfm {
namespace {

constexpr int kOccThreads = 1024;   // 4 waves per SIMD of the CU the histogram fills
constexpr int kOccBlocks = kCUs;    // the cap: a constant, the workspace query is pure
// ring entries of the search queue: fewer than one pass (1024) wait, a round adds 1024 at most
constexpr int kOccQueue = 2 * kOccThreads;
constexpr int kOccFinCells = 64;    // finalize: cells per block (one wave wide)
constexpr int kOccFinRows = 16;     // finalize: waves per block, each sums every 16th partial

// The dynamic LDS of a counting block: the histogram, then the search queue (a ring
// of kOccQueue grid coordinates, one array per axis, of the points that take branch
// 2) and its counter.
__host__ __device__ inline size_t occ_lds_bytes(int cells) {
  return ((size_t)cells + 3 * kOccQueue + 1) * sizeof(unsigned);
}

// What the workspace query and the launcher share.
struct OccPlan {
  bool ok;            // the arguments are accepted
  long long total;    // s * n
  int cells;          // r^3
  int blocks;         // counting blocks = partial histograms (0: no point)
  size_t lds_bytes;   // one histogram and the search queue (occ_lds_bytes)
  size_t ws_bytes;    // blocks * cells * 4
};

OccPlan occ_plan(int s, int n, int d, int r) {
  OccPlan p = {};
  if (s < 0 || n < 0 || !pcfm_occupancy_supported(d, r)) return p;
  p.total = (long long)s * n;
  if (p.total >= (1LL << 31)) return p;
  p.ok = true;
  p.cells = r * r * r;
  const long long rounds = (p.total + kOccThreads - 1) / kOccThreads;
  p.blocks = (int)(rounds < kOccBlocks ? rounds : kOccBlocks);
  p.lds_bytes = occ_lds_bytes(p.cells);
  p.ws_bytes = (size_t)p.blocks * p.cells * sizeof(unsigned);
  return p;
}

// Branch 2: the kept node of lowest flat index nearest to u (grid units).  Every
// lane of the wave runs the same loops (r is uniform).  A lane whose distances
// are never below +inf (non-finite u) keeps the centre node, which is kept.
__device__ __forceinline__ int occ_nearest_kept(float ux, float uy, float uz, int r) {
  const int r1 = r - 1, lim = r1 * r1;
  const int mid = r1 >> 1;   // the lower of the two centre planes when r is even
  float best = __builtin_inff();
  int node = (mid * r + mid) * r + mid;
  for (int i = 0; i < r; ++i) {
    const int a = 2 * i - r1;
    const float dx = ux - (float)i;
    // The kept k of column (i, j) are those with (2k - (r-1))^2 <= rem: an interval
    // [klo, r-1 - klo] that holds k = mid whenever rem >= 0 ((2 mid - (r-1))^2 <= 1,
    // and rem is odd when r is even).  klo follows rem from column to column; both
    // walks stay inside [0, mid].
    int klo = mid;
    for (int j = 0; j < r; ++j) {
      const int b = 2 * j - r1;
      const int rem = lim - a * a - b * b;
      if (rem < 0) continue;
      const float dy = uy - (float)j;
      const float dxy = __builtin_fmaf(dx, dx, dy * dy);
#pragma clang loop unroll(disable) vectorize(disable)
      while (klo < mid && (2 * klo - r1) * (2 * klo - r1) > rem) ++klo;
#pragma clang loop unroll(disable) vectorize(disable)
      while (klo > 0 && (2 * klo - 2 - r1) * (2 * klo - 2 - r1) <= rem) --klo;
      const int khi = r1 - klo;
      int f = (i * r + j) * r + klo;
      for (int k = klo; k <= khi; ++k, ++f) {
        const float dz = uz - (float)k;
        const float dist = __builtin_fmaf(dz, dz, dxy);   // sqdist3(dx, dy, dz)
        const bool nearer = dist < best;
        best = nearer ? dist : best;
        node = nearer ? f : node;
      }
    }
  }
  return node;
}

// One packed pass over the queue: thread t takes entry `first + t` of the ring if
// t < many.  A wave whose 64 entries lie beyond `many` skips the walk; inside it,
// all lanes run the same loops.
__device__ __forceinline__ void occ_drain(unsigned* hist, const float* lx, const float* ly,
                                          const float* lz, unsigned first, int many, int r) {
  const int t = threadIdx.x;
  if ((t & ~63) >= many) return;
  const bool mine = t < many;
  const unsigned e = (first + t) & (kOccQueue - 1);
  const float half = 0.5f * (float)(r - 1);     // a lane without an entry: the centre
  const int node = occ_nearest_kept(mine ? lx[e] : half, mine ? ly[e] : half,
                                    mine ? lz[e] : half, r);
  if (mine) atomicAdd(&hist[node], 1u);
}

__global__ void __launch_bounds__(kOccThreads)
    occ_count_kernel(const float* __restrict__ pts, long long total, int d, int r,
                     unsigned* __restrict__ partial) {
  extern __shared__ unsigned occ_hist[];
  const int cells = r * r * r;
  float* const lx = reinterpret_cast<float*>(occ_hist + cells);
  float* const ly = lx + kOccQueue;
  float* const lz = ly + kOccQueue;
  unsigned* const fill = reinterpret_cast<unsigned*>(lz + kOccQueue);   // entries ever queued
  const int t = threadIdx.x;
  for (int f = t; f < cells; f += kOccThreads) occ_hist[f] = 0u;
  if (t == 0) *fill = 0u;
  __syncthreads();

  const int r1 = r - 1, lim = r1 * r1;
  const float scale = (float)r1, half = 0.5f * (float)r1, top = (float)r1;
  const long long step = (long long)gridDim.x * kOccThreads;
  // `base`, `done` and `pending` are uniform in the block: every thread makes the
  // same trips and meets the same barriers.  Entries [done, done + pending) of the
  // ring wait for their walk; *fill is only ever touched by the appending adds.
  unsigned done = 0;
  int pending = 0;
  for (long long base = (long long)blockIdx.x * kOccThreads; base < total; base += step) {
    const long long i = base + t;
    bool queue = false;
    if (i < total) {
      const float* __restrict__ p = pts + (size_t)i * d;
      const float ux = __builtin_fmaf(p[0], scale, half);
      const float uy = __builtin_fmaf(p[1], scale, half);
      const float uz = __builtin_fmaf(p[2], scale, half);
      // fmaxf / fminf return the other operand for a NaN: always a node
      const int ci = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(ux), 0.f), top);
      const int cj = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(uy), 0.f), top);
      const int ck = (int)__builtin_fminf(__builtin_fmaxf(__builtin_rintf(uz), 0.f), top);
      const int a = 2 * ci - r1, b = 2 * cj - r1, c = 2 * ck - r1;
      queue = a * a + b * b + c * c > lim;
      if (!queue) {
        atomicAdd(&occ_hist[(ci * r + cj) * r + ck], 1u);                 // branch 1
      } else {
        const unsigned e = atomicAdd(fill, 1u) & (kOccQueue - 1);         // branch 2: queue it
        lx[e] = ux;
        ly[e] = uy;
        lz[e] = uz;
      }
    }
    // the barrier that publishes the round's entries also counts them
    pending += __syncthreads_count(queue);
    if (pending >= kOccThreads) {      // the next round could overrun the ring: one full pass
      occ_drain(occ_hist, lx, ly, lz, done, kOccThreads, r);
      done += kOccThreads;
      pending -= kOccThreads;
      __syncthreads();                 // the entries are read before the next round appends
    }
  }
  occ_drain(occ_hist, lx, ly, lz, done, pending, r);    // the rest, fewer than one pass
  __syncthreads();

  unsigned* __restrict__ out = partial + (size_t)blockIdx.x * cells;
  for (int f = t; f < cells; f += kOccThreads) out[f] = occ_hist[f];
}

// counts[f] = sum over the blocks of partial[block][f]; blocks == 0 writes zeros.
__global__ void __launch_bounds__(kOccFinCells * kOccFinRows)
    occ_finalize_kernel(const unsigned* __restrict__ partial, int blocks, int cells,
                        int* __restrict__ counts) {
  __shared__ unsigned part[kOccFinRows][kOccFinCells];
  const int lane = threadIdx.x, row = threadIdx.y;
  const int f = blockIdx.x * kOccFinCells + lane;
  unsigned sum = 0u;
  if (f < cells)
    for (int b = row; b < blocks; b += kOccFinRows) sum += partial[(size_t)b * cells + f];
  part[row][lane] = sum;
  __syncthreads();
  if (row == 0 && f < cells) {
    unsigned all = 0u;
#pragma unroll
    for (int k = 0; k < kOccFinRows; ++k) all += part[k][lane];
    counts[f] = (int)all;
  }
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" int pcfm_occupancy_abi_version(void) { return PCFM_OCCUPANCY_ABI_VERSION; }

extern "C" int pcfm_occupancy_supported(int d, int r) {
  return point_dim_ok(d) && d >= 3 && r >= 3 && r <= 32;   // the cells are over xyz
}

extern "C" size_t pcfm_occupancy_workspace_bytes(int s, int n, int d, int r) {
  const OccPlan p = occ_plan(s, n, d, r);
  return p.ok ? p.ws_bytes : 0;
}

extern "C" int pcfm_occupancy_counts(const float* pts, int s, int n, int d, int r, int* counts,
                                     void* ws, size_t ws_bytes, void* stream) {
  PCFM_CHECK_ARG(s >= 0 && n >= 0, "occupancy: negative size");
  PCFM_CHECK_ARG(pcfm_occupancy_supported(d, r),
                 "occupancy: unsupported dimension %d or resolution %d", d, r);
  const OccPlan p = occ_plan(s, n, d, r);
  PCFM_CHECK_ARG(p.ok, "occupancy: s = %d, n = %d too large", s, n);
  PCFM_CHECK_ARG(ws_bytes >= p.ws_bytes, "occupancy: workspace %zu < %zu bytes", ws_bytes,
                 p.ws_bytes);
  hipStream_t st = (hipStream_t)stream;
  if (p.blocks > 0) {
    const int e = allow_big_lds((const void*)occ_count_kernel);
    if (e) return e;
    hipLaunchKernelGGL(occ_count_kernel, dim3(p.blocks), dim3(kOccThreads), p.lds_bytes, st, pts,
                       p.total, d, r, (unsigned*)ws);
  }
  hipLaunchKernelGGL(occ_finalize_kernel, dim3(ceil_div(p.cells, kOccFinCells)),
                     dim3(kOccFinCells, kOccFinRows), 0, st, (const unsigned*)ws, p.blocks,
                     p.cells, counts);
  return check_launch("occupancy");
}
