// Sorted, atomic-free scatter ("segment sum") for the PVConv path.
//
// The reference scatters with one float atomic per (item, channel, tap)
// (vox.cu:48-72, trilinear_devox.cu:119-162, grouping.cu:58-77).  On MI355X a
// device-scope float atomic executes at the memory side (~1.3 TB/s of added
// bytes chip-wide) and an LDS float atomic costs ~200 cycles per wave
// instruction (measured, tools/voxel_probe.py), so the scatters are recast as
// gathers over items sorted by their target cell:
//
//   1. seg_sort     stable counting sort, up to 16 blocks per batch element,
//                   per-wave histograms in LDS: start[b, 0..V] and rank[b, i]
//                   (sorted position of item i, item order kept inside a key)
//   2. seg_units    tiles of kTV voxels -> balanced work units (device-built)
//   3. seg_plan_rows  the item's key and tap weights at its sorted position;
//      seg_rows     xs[b, rank[i], :] = in[b, :, i]: channels-last rows in
//                   SORTED order (the main loop then streams contiguous memory
//                   and chases no index)
//   4. seg_unit_gather  output-stationary, lanes = 64 channels: one wave per
//                   unit, register run-accumulators per tap flushed into a
//                   wave-private LDS tile, coalesced tile store
//   5. seg_part_sum adds the partial tiles of tiles split over several units
//   3'. seg_ldsrow1  replaces seg_rows, 4 and 5 for the one-tap scatters whose
//                   item row fits LDS (n <= kLdsRowMaxItems): one block per
//                   (batch, channel) holds the row in sorted order in LDS and
//                   sums every voxel's segment from there -- no transposed copy
//                   in HBM
//
// The sort is stable (items inside one key keep their index order) and every
// float sum runs in a fixed order, so the scatters are deterministic -- unlike
// the reference's float atomics.
#include "segsum.hpp"

#include <cstdlib>

namespace pcfm {
namespace {

// Inclusive prefix sum over the wave's 64 lanes.
__device__ __forceinline__ int wave_incl_scan(int x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  return x;
}

// Block carry of a 16-wave (1024-thread) block: wsum[g] holds wave g's sum
// (written before a barrier); returns {base + sum of the waves before w, sum
// of all}.
constexpr int kBlockWaves = 16;
__device__ __forceinline__ int2 block_carry(const int* wsum, int w, int base) {
  int before = base, total = 0;
#pragma unroll
  for (int g = 0; g < kBlockWaves; ++g) {
    const int s = wsum[g];
    before += g < w ? s : 0;
    total += s;
  }
  return make_int2(before, total);
}

// --------------------------------------------------------------------------
// 1: STABLE counting sort by key.  Block (p, b) owns the key range [p, p+1) *
// span of batch element b (grid = (P, B), 1024 threads = 16 waves): every block
// reads all n keys of its batch element (L2-resident, 80 KB at N = 20000) and
// counts the keys BELOW its range itself -- its base in the sorted order, so
// the P blocks never wait for each other.  Keys are handled in chunks of
// kSortChunk (a wider range takes several passes).  Wave w owns the item
// segment [w n / 16, (w+1) n / 16) and keeps its own per-key counts in LDS:
//   A  count:  per-wave histograms of the chunk (LDS int atomics; counts are
//              order-free);
//   B  scan:   per key the exclusive prefix over keys (-> start) and over the
//              waves (-> each wave's first rank of that key);
//   C  rank:   each wave walks its segment in index order, 64 items per step;
//              the items of one step that share a key are ranked by lane, and
//              only the owning wave advances its counters -- so
//              rank[i] = start[key_i] + #{j < i : key_j = key_i}:
//              the order inside a key is the item order, independent of
//              scheduling.  Every float sum downstream (unit gathers, partial
//              tiles) then runs in a fixed order: the scatters are
//              deterministic (the reference's float atomics are not).
//   start[b, 0..V]  exclusive prefix of the counts (start[b, V] = total)
//   cnt_out[b, v]   the counts (optional: the voxelization's `cnt` output)
//   vinv[b, v]      (float)(1.0 / (double)cnt) (optional, vox.cu:66)
//   rank[b, i]      start[key_i] + rank within the key; -1 when the key is
//                   outside [0, V) (the item contributes nothing)
// Keys are key[i] + koff (seg_koff; V then counts the shifted key range and
// cnt_out / vinv are not asked for).
// --------------------------------------------------------------------------
constexpr int kSortWaves = kBlockWaves;
constexpr int kSortChunk = 2048;   // keys per pass: 16 waves x 2048 ints = 128 KiB of LDS
constexpr int kSortBatch = 8;      // 64-item key loads per wave in flight
constexpr int kSortMinSpan = 32;   // keys per block at least
constexpr int kSortMaxParts = 16;  // blocks per batch element at most

inline int seg_sort_parts(int V) {
  return std::max(1, std::min(kSortMaxParts, V / kSortMinSpan));
}
inline int seg_sort_span(int V) { return (V + seg_sort_parts(V) - 1) / seg_sort_parts(V); }
inline size_t seg_sort_lds(int V) {
  return (size_t)kSortWaves * std::min(seg_sort_span(V), kSortChunk) * sizeof(int);
}

__global__ void __launch_bounds__(1024)
    seg_sort_kernel(const int* __restrict__ key, long long key_bstride, int n, int V, int span,
                    int* __restrict__ start, int* __restrict__ cnt_out, float* __restrict__ vinv,
                    int* __restrict__ rank, int koff) {
  extern __shared__ int hw[];  // [kSortWaves][len]
  __shared__ int wsum[kSortWaves];
  const int p = blockIdx.x, b = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int* __restrict__ kb = key + (size_t)b * key_bstride;
  int* __restrict__ sb = start + (size_t)b * (V + 1);
  int* __restrict__ rb = rank + (size_t)b * n;
  const int pk0 = min(V, p * span), pk1 = min(V, pk0 + span);
  const int i_lo = (int)((long long)n * w / kSortWaves);
  const int i_hi = (int)((long long)n * (w + 1) / kSortWaves);
  int carry = 0;
  for (int k0 = pk0; k0 < pk1; k0 += kSortChunk) {
    const int len = min(kSortChunk, pk1 - k0);
    for (int e = t; e < kSortWaves * len; e += 1024) hw[e] = 0;
    __syncthreads();
    // A: per-wave counts (+ the keys below the block's range: its base)
    int* hmine = hw + w * len;
    int below = 0;
    for (int i0 = i_lo; i0 < i_hi; i0 += 64 * kSortBatch) {
      int kk[kSortBatch];  // keys first (independent loads in flight), then the atomics
#pragma unroll
      for (int q = 0; q < kSortBatch; ++q) {
        const int i = i0 + 64 * q + lane;
        kk[q] = i < i_hi ? kb[i] + koff : -1;
      }
#pragma unroll
      for (int q = 0; q < kSortBatch; ++q) {
        if ((unsigned)(kk[q] - k0) < (unsigned)len) atomicAdd(hmine + (kk[q] - k0), 1);
        below += (k0 == pk0 && (unsigned)kk[q] < (unsigned)pk0) ? 1 : 0;
      }
    }
    if (k0 == pk0) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
      if (lane == 0) wsum[w] = below;
    }
    __syncthreads();
    if (k0 == pk0) carry += block_carry(wsum, w, 0).y;
    __syncthreads();
    // B: wave w owns the 64-aligned key segment [lo, hi)
    const int seg = ((len + kSortWaves - 1) / kSortWaves + 63) & ~63;
    const int lo = min(len, w * seg), hi = min(len, lo + seg);
    int part = 0;
    for (int e = lo + lane; e < hi; e += 64) {
#pragma unroll
      for (int g = 0; g < kSortWaves; ++g) part += hw[g * len + e];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) wsum[w] = part;
    __syncthreads();
    // (block_carry written out: as a call hipcc allocates this kernel anew,
    // 79 -> 62 VGPRs and another schedule)
    int run = carry, total = 0;
#pragma unroll
    for (int g = 0; g < kSortWaves; ++g) {
      const int s = wsum[g];
      run += g < w ? s : 0;
      total += s;
    }
    for (int e0 = lo; e0 < hi; e0 += 64) {
      const int e = e0 + lane;
      int c = 0;
      if (e < hi) {
#pragma unroll
        for (int g = 0; g < kSortWaves; ++g) c += hw[g * len + e];
      }
      const int x = wave_incl_scan(c);
      if (e < hi) {
        int pos = run + x - c;
        sb[k0 + e] = pos;
        if (cnt_out != nullptr) cnt_out[(size_t)b * V + k0 + e] = c;
        if (vinv != nullptr) vinv[(size_t)b * V + k0 + e] = c > 0 ? (float)(1.0 / (double)c) : 0.0f;
#pragma unroll
        for (int g = 0; g < kSortWaves; ++g) {  // first rank of key e for wave g
          const int cg = hw[g * len + e];
          hw[g * len + e] = pos;
          pos += cg;
        }
      }
      run += __shfl(x, 63, 64);
    }
    __syncthreads();
    // C: ranks in item order (only wave w touches its counters)
    const int nbits = len > 1 ? 32 - __clz(len - 1) : 0;
    for (int j0 = i_lo; j0 < i_hi; j0 += 64 * kSortBatch) {
      int kq[kSortBatch];
#pragma unroll
      for (int q = 0; q < kSortBatch; ++q) {
        const int i = j0 + 64 * q + lane;
        kq[q] = i < i_hi ? kb[i] + koff : -1;
      }
#pragma unroll
      for (int q = 0; q < kSortBatch; ++q) {
        const int i = j0 + 64 * q + lane;
        const int k = kq[q];
        const bool inr = i < i_hi && (unsigned)(k - k0) < (unsigned)len;
        const unsigned long long act = __ballot(inr);
        if (act) {
          // lanes of this step with the same key, by bit-plane ballots of the
          // chunk-local key (nbits of them); the lane's rank among them is the
          // count of lower lanes (mbcnt), and the LAST lane of each group alone
          // advances the wave's counter: no lane-order-dependent atomics
          const unsigned kl = inr ? (unsigned)(k - k0) : 0u;
          unsigned long long same = act;
          for (int bit = 0; bit < nbits; ++bit) {
            const bool on = (kl >> bit) & 1u;
            const unsigned long long m = __ballot(on);
            same &= on ? m : ~m;
          }
          if (inr) {
            const int within = __builtin_amdgcn_mbcnt_hi(
                (unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
            const int base = hmine[kl];
            rb[i] = base + within;
            if ((same >> lane) >> 1 == 0ull) hmine[kl] = base + __popcll(same);
          }
        }
        if (p == 0 && k0 == pk0 && i < i_hi && (unsigned)k >= (unsigned)V) rb[i] = -1;
      }
    }
    carry += total;
    __syncthreads();
  }
  if (t == 0 && pk1 == V && (pk0 < V || p == 0)) sb[V] = carry;
}

// --------------------------------------------------------------------------
// 3: rows in sorted order.  xs[b, rank[i], c] = in[b, c, i] (64 x 64 LDS
// tile: 256-B coalesced reads along i, one 256-B row segment per store).  A
// block takes 64 items and every channel group in turn: an item's whole row
// (C floats) is written by one wave within a few hundred cycles, instead of in
// C/64 pieces by blocks dispatched far apart.
// grid = (ceil(n/64), 1, B), 256 threads.
// --------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    seg_rows_kernel(const float* __restrict__ in, const int* __restrict__ rank, int C, int n,
                    float* __restrict__ xs) {
  __shared__ float tile[64][64 + 1];
  __shared__ int rk[64];
  const int b = blockIdx.z;
  const int j0 = blockIdx.x * 64;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int jj = threadIdx.x; jj < 64; jj += 256) {
    const int j = j0 + jj;
    rk[jj] = j < n ? rank[(size_t)b * n + j] : -1;
  }
  const int j = j0 + lane;
  __syncthreads();
  for (int g0 = 0; g0 < C; g0 += 64) {
    float v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = g0 + w + 4 * q;
      v[q] = (c < C && j < n) ? in[((size_t)b * C + c) * n + j] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) tile[w + 4 * q][lane] = v[q];
    __syncthreads();
    const int c = g0 + lane;
    if (c < C) {
      for (int jr = w; jr < 64; jr += 4) {
        const int r = rk[jr];
        if (r >= 0) xs[((size_t)b * n + r) * C + c] = tile[lane][jr];
      }
    }
    __syncthreads();
  }
}

// Plan-side part of step 3: the sorted keys (skey[b, rank[i]] = key[i]) and,
// for the trilinear stencil, the sorted tap weights (ws8[b, rank[i], k] =
// tapw[b, k, i]) -- built once per plan, reused by every scatter over it.
// grid = (ceil(n / 256), B).
__global__ void __launch_bounds__(256)
    seg_plan_rows_kernel(const int* __restrict__ rank, const int* __restrict__ key,
                         long long key_bstride, const float* __restrict__ tapw, int n,
                         int* __restrict__ skey, float* __restrict__ ws8) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int r = rank[(size_t)b * n + i];
  if (r < 0) return;
  const size_t o = (size_t)b * n + r;
  skey[o] = key[(size_t)b * key_bstride + i];
  if (tapw != nullptr) {
    const float* tb = tapw + (size_t)b * 8 * n + i;
    float4* d = reinterpret_cast<float4*>(ws8 + o * 8);
    d[0] = make_float4(tb[0], tb[(size_t)n], tb[(size_t)2 * n], tb[(size_t)3 * n]);
    d[1] = make_float4(tb[(size_t)4 * n], tb[(size_t)5 * n], tb[(size_t)6 * n], tb[(size_t)7 * n]);
  }
}

// --------------------------------------------------------------------------
// 2 + 4 + 5: units, unit gather, partial sums.
//   The output is cut into tiles of kTV consecutive voxels.  Items feeding a
//   tile form NR contiguous sorted ranges:
//   TAPS == 8: column g = (dx, dy) in 0..3, off = dx r^2 + dy r.  A point of
//     cell q adds w[dx,dy,0] * x to voxel q + off and w[dx,dy,1] * x to voxel
//     q + off + 1; the column's source cells are [v0 - off - 1, v0 + kTV - off).
//     (When a fraction is 0 the reference folds that corner onto the low cell
//     with weight exactly 0, trilinear_devox.cu:64-75, so both placements add
//     the same zeros.)
//   TAPS == 1: one range [v0, v0 + kTV); a point of cell q adds x * vscale[q]
//     (or x) to voxel q.
//   A tile with T items (its ranges concatenated) becomes P = ceil(T / kItems)
//   work units of ~T/P items (at least one, so empty tiles are written as
//   zeros).  ONE wave runs a unit: per 64 items one load round fetches the
//   sorted keys and tap weights, the 16 next feature rows (consecutive rows
//   of xs) are loaded back to back, a register accumulator per tap runs over
//   equal target voxels and is added into the wave's private LDS tile when the
//   voxel changes.  Unit 0 of a tile writes the tile to `out`; units 1.. of a
//   crowded tile write partial tiles that seg_part_sum_kernel adds in unit
//   order.  Waves never wait for each other and nothing is atomic.
// --------------------------------------------------------------------------
constexpr int kInFlight = 16;    // feature-row loads issued back to back per wave
constexpr int kUnitWaves = 4;    // waves (independent units) per block

template <int TAPS>
constexpr int seg_ranges() { return TAPS == 8 ? 4 : 1; }

// seg_koff on the device
template <int TAPS>
__device__ __forceinline__ int seg_koff_r(int r) { return TAPS == 8 ? r * r + r + 1 : 0; }

// Column g of the tile at voxel v0: its stencil offset, and its source cells
// [lo, hi) as shifted keys (+ seg_koff) clamped into the start row [0, V + koff].
struct SegCol {
  int off, lo, hi;
};
template <int TAPS>
__device__ __forceinline__ SegCol seg_col_range(int v0, int g, int r, int V) {
  const int koff = seg_koff_r<TAPS>(r);
  const int off = TAPS == 8 ? (g >> 1) * r * r + (g & 1) * r : 0;
  const int lo = TAPS == 8 ? v0 - off - 1 : v0;
  const int hi = v0 + kTV - off;
  return SegCol{off, min(max(lo + koff, 0), V + koff), min(max(hi + koff, 0), V + koff)};
}

// Range g of tile v0: lanes 2g / 2g+1 return the sorted positions [lo, hi).
// sb: the batch element's start row over the V + koff shifted keys.
template <int TAPS>
__device__ __forceinline__ int seg_range_bound(const int* sb, int v0, int V, int r, int lane) {
  int bnd = 0;
  if (lane < 2 * seg_ranges<TAPS>()) {
    const SegCol col = seg_col_range<TAPS>(v0, lane >> 1, r, V);
    bnd = sb[(lane & 1) ? col.hi : col.lo];
  }
  return bnd;
}

// Work-unit list, one block (1024 threads) per batch element:
//   units[b, u] = {tile, part, parts, items}, tinfo[b, tile] = {parts, first
//   partial slot}, nunits[b].
template <int TAPS>
__global__ void __launch_bounds__(1024)
    seg_units_kernel(const int* __restrict__ start, int V, int r, int tiles, int umax,
                     int4* __restrict__ units, int2* __restrict__ tinfo, int* __restrict__ nunits) {
  __shared__ int wsum[kBlockWaves];
  constexpr int NR = seg_ranges<TAPS>();
  const int b = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int* sb = start + (size_t)b * (V + seg_koff_r<TAPS>(r) + 1);
  int carry = 0;
  for (int t0 = 0; t0 < tiles; t0 += 1024) {
    const int tile = t0 + t;
    int T = 0, P = 0;
    if (tile < tiles) {
#pragma unroll
      for (int g = 0; g < NR; ++g) {
        const SegCol col = seg_col_range<TAPS>(tile * kTV, g, r, V);
        T += sb[col.hi] - sb[col.lo];
      }
      P = max(1, (T + kItems - 1) / kItems);
    }
    const int x = wave_incl_scan(P);
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    const int2 bc = block_carry(wsum, w, carry);
    const int U = bc.x + x - P;
    if (tile < tiles) {
      tinfo[(size_t)b * tiles + tile] = make_int2(P, U - tile);
      for (int p = 0; p < P && U + p < umax; ++p)
        units[(size_t)b * umax + U + p] = make_int4(tile, p, P, T);
    }
    carry += bc.y;
    __syncthreads();
  }
  if (t == 0) nunits[b] = min(carry, umax);
}

// Run bookkeeping: when a run of equal target voxels starts, the tile's
// current partials for its slots are READ (p0, p1) without waiting; when it
// ends, p + acc is written back.  The LDS read latency then hides behind the
// run's row loads instead of stalling every flush (LDS ops of one wave stay in
// order, so a read of slot s+1 after the previous run's write of s+1 sees it).
template <int TAPS>
__device__ __forceinline__ void seg_run_end(float* tl, int slot, int lane, float p0, float p1,
                                            float a0, float a1) {
  if ((unsigned)slot < (unsigned)kTV) tl[slot * 65 + lane] = p0 + a0;
  if constexpr (TAPS == 8) {
    if ((unsigned)(slot + 1) < (unsigned)kTV) tl[(slot + 1) * 65 + lane] = p1 + a1;
  }
}
template <int TAPS>
__device__ __forceinline__ void seg_run_begin(const float* tl, int slot, int lane, float& p0,
                                              float& p1) {
  p0 = (unsigned)slot < (unsigned)kTV ? tl[slot * 65 + lane] : 0.0f;
  if constexpr (TAPS == 8) p1 = (unsigned)(slot + 1) < (unsigned)kTV ? tl[(slot + 1) * 65 + lane] : 0.0f;
}

__device__ __forceinline__ float rl_f(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// grid = (ceil(umax / kUnitWaves), ceil(C/64), B), kUnitWaves * 64 threads.
template <int TAPS>
__global__ void __launch_bounds__(kUnitWaves * 64)
    seg_unit_gather_kernel(const float* __restrict__ xs, const int* __restrict__ skey,
                           const float* __restrict__ ws8, const int* __restrict__ start,
                           const float* __restrict__ vscale, const int4* __restrict__ units,
                           const int* __restrict__ nunits, int C, int n, int V, int r, int umax,
                           int slots, float* __restrict__ out, float* __restrict__ partial) {
  __shared__ float lds[kUnitWaves][kTV * 65];
  constexpr int NR = seg_ranges<TAPS>();
  // XCD-contiguous deal: give each XCD a contiguous run of (unit block, channel
  // group, batch) so a row's re-reads by the other stencil columns hit its L2
  // (against dispatch order, tools/scatter_ab.py on MI355X: devox backward
  // 0.183 -> 0.175 ms C128 R32, 0.235 -> 0.215 C256 R16, 0.224 -> 0.207 C256
  // R8; the voxelize forward unchanged)
  const int gx = (int)gridDim.x, gy = (int)gridDim.y;
  const int id = xcd_deal((int)(blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z)),
                          gx * gy * (int)gridDim.z);
  const int bx = id % gx, b = id / (gx * gy), c0 = (id / gx) % gy * 64;
  // readfirstlane: the wave index is uniform, so the whole walk stays scalar
  // (no exec-mask branches, no vmcnt(0) stalls between the row loads)
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nu = nunits[b];
  const int u = bx * kUnitWaves + w;
  if (u >= nu) return;  // wave-uniform; no block barrier below
  const int4 un = units[(size_t)b * umax + u];
  const int tile = un.x, part = un.y, parts = un.z, T = un.w;
  const int v0 = tile * kTV;
  const int c = c0 + lane;
  const bool cok = c < C;
  const int* __restrict__ sb = start + (size_t)b * (V + seg_koff_r<TAPS>(r) + 1);
  const int* __restrict__ kb = skey + (size_t)b * n;
  const float* __restrict__ xb = xs + (size_t)b * n * C + (cok ? c : 0);
  const float* __restrict__ wb = TAPS == 8 ? ws8 + (size_t)b * n * 8 : nullptr;

  const int bnd = seg_range_bound<TAPS>(sb, v0, V, r, lane);
  int rs[NR], pre[NR + 1];
  pre[0] = 0;
#pragma unroll
  for (int g = 0; g < NR; ++g) {
    rs[g] = __builtin_amdgcn_readlane(bnd, 2 * g);
    pre[g + 1] = pre[g] + __builtin_amdgcn_readlane(bnd, 2 * g + 1) - rs[g];
  }
  const int i0 = (int)((long long)T * part / parts);
  const int i1 = (int)((long long)T * (part + 1) / parts);
  float vs = 0.0f;  // TAPS == 1 average pool: lane l holds 1/cnt of voxel v0 + l
  if (TAPS == 1 && vscale != nullptr && lane < kTV && v0 + lane < V)
    vs = vscale[(size_t)b * V + v0 + lane];

  float* tl = lds[w];
  for (int e = lane; e < kTV * 65; e += 64) tl[e] = 0.0f;

  int cur = -1000;
  float a0 = 0.0f, a1 = 0.0f, p0 = 0.0f, p1 = 0.0f, sc = 1.0f;
  for (int base = i0; base < i1; base += 64) {
    const int m = min(64, i1 - base);
    const int it = base + lane;
    int pos = 0, sl = -1000;
    float w0v = 0.0f, w1v = 0.0f;
    if (lane < m) {
      int g = 0;
#pragma unroll
      for (int q = 1; q < NR; ++q) g += it >= pre[q] ? 1 : 0;
      int off = 0, gs = 0;
#pragma unroll
      for (int q = 0; q < NR; ++q)
        if (g == q) {
          pos = rs[q] + it - pre[q];
          off = seg_col_range<TAPS>(v0, q, r, V).off;
          gs = q;
        }
      sl = kb[pos] + off - v0;
      if constexpr (TAPS == 8) {  // taps k = 4dx + 2dy + dz = 2g + dz
        const float2 ww = *reinterpret_cast<const float2*>(wb + (size_t)pos * 8 + 2 * gs);
        w0v = ww.x;
        w1v = ww.y;
      }
    }
    for (int u0 = 0; u0 < m; u0 += kInFlight) {
      float x[kInFlight];
      // unconditional: lanes >= m hold pos = 0, a valid row
#pragma unroll
      for (int q = 0; q < kInFlight; ++q)
        x[q] = xb[(size_t)__builtin_amdgcn_readlane(pos, u0 + q) * C];
      const int cnt = min(kInFlight, m - u0);
#pragma unroll
      for (int q = 0; q < kInFlight; ++q) {
        if (q < cnt) {
          const int slot = __builtin_amdgcn_readlane(sl, u0 + q);
          if (slot != cur) {
            seg_run_end<TAPS>(tl, cur, lane, p0, p1, a0, a1);
            cur = slot;
            seg_run_begin<TAPS>(tl, cur, lane, p0, p1);
            a0 = 0.0f;
            a1 = 0.0f;
            if constexpr (TAPS == 1) sc = rl_f(vs, slot & 63);
          }
          if constexpr (TAPS == 8) {
            a0 = a0 + rl_f(w0v, u0 + q) * x[q];
            a1 = a1 + rl_f(w1v, u0 + q) * x[q];
          } else {
            a0 = vscale != nullptr ? a0 + x[q] * sc : a0 + x[q];
          }
        }
      }
    }
  }
  seg_run_end<TAPS>(tl, cur, lane, p0, p1, a0, a1);

  // tile -> global, 2 channels x 32 voxels (2 x 128 B) per store instruction
  float* dst;
  size_t cstride, bofs;
  if (part == 0) {
    dst = out + v0;
    cstride = (size_t)V;
    bofs = (size_t)b * C * V;
  } else {  // partial slot: units of tiles before this one beyond their first, + part - 1
    dst = partial;
    cstride = (size_t)kTV;
    bofs = ((size_t)b * slots + (size_t)(u - tile - 1)) * C * kTV;
  }
  const int vi = lane & (kTV - 1), ch = lane / kTV;
  const bool vok = part > 0 || v0 + vi < V;
#pragma unroll 4
  for (int k = 0; k < 64; k += 64 / kTV) {
    const int cc = k + ch, cg = c0 + cc;
    if (cg < C && vok) dst[bofs + (size_t)cg * cstride + vi] = tl[vi * 65 + cc];
  }
}

// out += partial tiles 1 .. P-1 of every crowded tile, in unit order.
// grid = (tiles, ceil(C/64), B), 256 threads.
__global__ void __launch_bounds__(256)
    seg_part_sum_kernel(const int2* __restrict__ tinfo, const float* __restrict__ partial,
                        int C, int V, int tiles, int slots, float* __restrict__ out) {
  const int b = blockIdx.z, tile = blockIdx.x, c0 = blockIdx.y * 64;
  const int2 ti = tinfo[(size_t)b * tiles + tile];
  if (ti.x <= 1) return;
  const int v0 = tile * kTV;
  for (int e = threadIdx.x; e < 64 * kTV; e += 256) {
    const int cc = e / kTV, vi = e - cc * kTV;
    const int cg = c0 + cc, v = v0 + vi;
    if (cg < C && v < V) {
      const size_t o = ((size_t)b * C + cg) * V + v;
      const float* pp = partial + (((size_t)b * slots + ti.y) * C + cg) * kTV + vi;
      const size_t ps = (size_t)C * kTV;  // one partial tile
      float sum = out[o];
      int p = 0;
      for (; p + 8 <= ti.x - 1; p += 8) {  // 8 independent loads in flight, summed in order
        float x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = pp[(size_t)(p + q) * ps];
#pragma unroll
        for (int q = 0; q < 8; ++q) sum = sum + x[q];
      }
      for (; p < ti.x - 1; ++p) sum = sum + pp[(size_t)p * ps];
      out[o] = sum;
    }
  }
}

// --------------------------------------------------------------------------
// 3' + 4': the LDS-row apply (TAPS == 1), for item rows that fit LDS.  One
// (batch, channel) item row is 4 n bytes (80 KB at N = 20000), so instead of
// transposing (B, C, N) into channels-last rows in HBM (seg_rows), reading
// them back (seg_unit_gather) and adding partial tiles (seg_part_sum), ONE
// block per (batch, channel):
//   stage   streams in[b, c, 0..n) and rank[b, 0..n) coalesced and stores
//           row[rank[i]] = in[i] (rank is a permutation: no atomics); after one
//           barrier LDS holds the channel's items in sorted order;
//   sum     lane per voxel, 64-voxel chunks dealt round-robin to the waves:
//           out[b, c, v] = sum of row[start[v] .. start[v+1]) * (1 / count when
//           averaging), term by term in sorted (= item) order;
//   crowd   the SAME SUMS IN THE SAME ORDER as the unit gather + seg_part_sum,
//           so both engines return the same bits: a kTV-voxel tile of T > kItems
//           items is cut into P = ceil(T / kItems) pieces [T p / P, T (p+1) / P)
//           of its sorted items (the work units); a voxel's items inside one
//           piece are summed in order from 0, and the voxel's piece sums are
//           added in piece order.  A voxel inside one piece is still one lane's
//           in-order sum.  A voxel that straddles pieces (at most one per piece
//           boundary: <= n / kItems of them, the centre cells of a Gaussian
//           cloud -- 2,372 points in one r = 8 voxel) goes on an LDS list (int
//           atomic: the list's ORDER is arrival order, but a listed voxel's sum
//           does not depend on who takes it) and is summed by a group of 16
//           lanes, a lane per piece, then folded in piece order.
// Every out element is written exactly once (zeros for empty voxels); HBM sees
// the input row once and the output row once.  The sum is bound by instruction
// issue, not by LDS or HBM (measured: DESIGN.md section 4, scatter step 7), so
// it spends instructions per 64-voxel chunk sparingly: start[v + 1] comes from
// the next lane, empty chunks only store zeros, the tile arithmetic runs only
// in a chunk of more than kItems items, 1 / count is computed instead of loaded.
// grid = (C, B), 1024 threads: two blocks per CU while 4 n <= 80 KB.
// --------------------------------------------------------------------------
constexpr int kLdsRowMaxItems = 40000;  // item row + crowd list <= the dynamic-LDS cap
constexpr int kRowThreads = 1024;
constexpr int kRowChunks = 4;  // 64-voxel chunks per wave per round (their plan loads in flight)
// item loads per thread in flight while staging: the whole row of N = 20000 in
// ONE round of 1024 threads (a block's stage is a chain of load round trips)
constexpr int kRowStage = 20;
constexpr int kRowAhead = 8;  // LDS reads in flight per lane in the in-order sum
constexpr int kRowPad = kRowAhead;  // floats past the row, so the read-ahead stays inside LDS
constexpr int kRowGroup = 16;  // lanes (pieces at a time) per listed voxel
static_assert(64 % kTV == 0 && (kTV & (kTV - 1)) == 0, "tiles must not cross 64-voxel chunks");

inline size_t seg_ldsrow_lds(int n) {
  return (size_t)(n + kRowPad) * sizeof(float) + (size_t)(n / kItems + 1) * sizeof(int);
}
static_assert((size_t)(kLdsRowMaxItems + kRowPad) * 4 + (size_t)(kLdsRowMaxItems / kItems + 1) * 4 <=
                  (size_t)kLdsBytesMax - 1024,
              "the LDS row of kLdsRowMaxItems items exceeds the dynamic-LDS cap");
static_assert((long long)kLdsRowMaxItems * (kLdsRowMaxItems / kItems + 2) < (1LL << 31),
              "piece arithmetic is done in int");

// The average pool's per-term factor, the bits seg_sort writes to vinv as
// (float)(1.0 / (double)c) (vox.cu:66).  The correctly rounded fp32 quotient is
// that value: rounding 1/c to double first could only matter if 1/c lay within
// 2^-53 (relative) of the midpoint M / 2^j of two floats (M odd, j <= 25 +
// log2 c), but |1/c - M / 2^j| >= 1 / (c 2^j) unless c is a power of two
// (1/c exact), and 2^j < 2^53 for every c < 2^28.
__device__ __forceinline__ float seg_inv_count(int c) {
  return c > 0 ? 1.0f / (float)c : 0.0f;
}

// The piece (work unit) of a tile's item j, 0 <= j < T: the p with
// T p / P <= j < T (p + 1) / P (integer divisions, as the unit gather cuts).
__device__ __forceinline__ int seg_piece(int j, int T, int P) {
  return ((j + 1) * P - 1) / T;
}

// row[a .. e) * s summed in order from 0, kRowAhead LDS reads in flight; reads
// past e stay inside the padded row.
__device__ __forceinline__ float seg_row_sum(const float* row, int a, int e, float s) {
  float acc = 0.0f;
  int i = a;
  for (; i + kRowAhead <= e; i += kRowAhead) {
    float x[kRowAhead];
#pragma unroll
    for (int q = 0; q < kRowAhead; ++q) x[q] = row[i + q];
#pragma unroll
    for (int q = 0; q < kRowAhead; ++q) acc = acc + x[q] * s;
  }
  if (i < e) {
    float x[kRowAhead - 1];
#pragma unroll
    for (int q = 0; q < kRowAhead - 1; ++q) x[q] = row[i + q];
#pragma unroll
    for (int q = 0; q < kRowAhead - 1; ++q)
      if (i + q < e) acc = acc + x[q] * s;
  }
  return acc;
}

__global__ void __launch_bounds__(kRowThreads)
    seg_ldsrow1_kernel(const float* __restrict__ in, const int* __restrict__ rank,
                       const int* __restrict__ start, int avg, int C, int n, int V,
                       float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float row[];  // [n + pad] items, the crowd list
  __shared__ int nlist;
  int* list = reinterpret_cast<int*>(row + n + kRowPad);
  const int lcap = n / kItems + 1;
  const int c = blockIdx.x, b = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63;
  constexpr int nt = kRowThreads, nw = kRowThreads / 64;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  if (t == 0) nlist = 0;
  const float* __restrict__ ib = in + ((size_t)b * C + c) * n;
  const int* __restrict__ rb = rank + (size_t)b * n;
  for (int i0 = t; i0 < n; i0 += kRowStage * nt) {
    float x[kRowStage];
    int rk[kRowStage];  // loads first (independent, in flight together), then the LDS stores
#pragma unroll
    for (int q = 0; q < kRowStage; ++q) {
      const int i = i0 + q * nt;
      rk[q] = i < n ? rb[i] : -1;
      x[q] = i < n ? nt_ld(ib + i) : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < kRowStage; ++q)
      if ((unsigned)rk[q] < (unsigned)n) row[rk[q]] = x[q];
  }
  __syncthreads();

  const int* __restrict__ sb = start + (size_t)b * (V + 1);
  float* __restrict__ ob = out + ((size_t)b * C + c) * V;
  const int nchunks = (V + 63) >> 6;
  for (int c0 = w; c0 < nchunks; c0 += kRowChunks * nw) {
    int s0[kRowChunks], s1[kRowChunks];
#pragma unroll
    for (int u = 0; u < kRowChunks; ++u) {  // lanes past V: the empty segment at start[V]
      const int ch = min(c0 + u * nw, nchunks - 1);
      s0[u] = sb[min(ch * 64 + lane, V)];
      s1[u] = sb[min(ch * 64 + 64, V)];  // one address per wave: the chunk's end
    }
#pragma unroll
    for (int u = 0; u < kRowChunks; ++u) {
      if (c0 + u * nw >= nchunks) break;  // wave-uniform
      const int v = (c0 + u * nw) * 64 + lane;
      const int nx = __shfl_down(s0[u], 1, 64);  // start[v + 1] from the next lane
      const int a = max(s0[u], 0), e = min(lane < 63 ? nx : s1[u], n);
      if (!__any(e > a)) {  // an empty chunk (most of the r = 32 grid)
        if (v < V) ob[v] = 0.0f;
        continue;
      }
      if (s1[u] - __builtin_amdgcn_readfirstlane(s0[u]) > kItems) {  // wave-uniform
        // the kTV-voxel tile's items (tiles are aligned inside the 64-aligned chunk)
        const int tA = __shfl(a, lane & ~(kTV - 1), 64);
        const int T = __shfl(e, lane | (kTV - 1), 64) - tA;
        if (T > kItems && e > a) {
          const int P = (T + kItems - 1) / kItems;
          if (seg_piece(a - tA, T, P) != seg_piece(e - 1 - tA, T, P)) {
            const int slot = atomicAdd(&nlist, 1);
            if (slot < lcap) list[slot] = v;
            continue;
          }
        }
      }
      const float acc = seg_row_sum(row, a, e, avg ? seg_inv_count(e - a) : 1.0f);
      if (v < V) ob[v] = acc;
    }
  }
  __syncthreads();
  // the listed voxels: a group of kRowGroup lanes each, a lane per piece
  const int nl = min(nlist, lcap);
  const int sub = lane & (kRowGroup - 1), gbase = lane & ~(kRowGroup - 1);
  constexpr int kGroups = kRowThreads / kRowGroup;
  for (int e0 = 0; e0 < nl; e0 += kGroups) {
    const int ei = e0 + t / kRowGroup;
    int v = 0, a = 0, e = 0, tA = 0, T = 1, P = 1, pl = 0, ph = -1;
    if (ei < nl) {
      v = list[ei];
      a = max(sb[v], 0);
      e = min(sb[v + 1], n);
      tA = max(sb[v & ~(kTV - 1)], 0);
      T = max(min(sb[min((v | (kTV - 1)) + 1, V)], n) - tA, 1);
      P = (T + kItems - 1) / kItems;
      pl = seg_piece(a - tA, T, P);
      ph = seg_piece(e - 1 - tA, T, P);
    }
    const float s = avg ? seg_inv_count(e - a) : 1.0f;
    float total = 0.0f;
    for (int k = 0; __any(pl + k <= ph); k += kRowGroup) {
      const int p = pl + k + sub;
      float part = 0.0f;
      if (p <= ph) {
        const int pb = tA + T * p / P, pe = tA + T * (p + 1) / P;
        part = seg_row_sum(row, max(a, pb), min(e, pe), s);
      }
#pragma unroll
      for (int j = 0; j < kRowGroup; ++j) {  // fold in piece order
        const float pj = __shfl(part, gbase + j, 64);
        if (pl + k + j <= ph) total = (k + j == 0) ? pj : total + pj;
      }
    }
    if (sub == 0 && ei < nl) ob[v] = total;
  }
}

// --------------------------------------------------------------------------
// host driver
// --------------------------------------------------------------------------

// PCFM_SEG_LDSROW=0: every scatter on the transposing engine (seg_rows + unit
// gather + partial sums) -- the A/B switch of the LDS-row apply, read once.
bool seg_ldsrow_enabled() {
  static const bool on = [] {
    const char* e = std::getenv("PCFM_SEG_LDSROW");
    return !(e != nullptr && e[0] == '0');
  }();
  return on;
}

// (Round 5 built 2 x 2-column tiles for the trilinear scatter -- a row read by
// 2.25 tiles instead of 4 -- bit-identical to the column tiles and slower:
// the gather is issue-bound; profiles/r05_ab_devox_quad.jsonl.  Removed in
// round 6.  A rocPRIM radix sort of the composite keys, kept opt-in through
// round 5 at ~70 us per sort against seg_sort's 23 us, was removed then too.)

template <int TAPS>
int plan_build(const int* key, long long key_bstride, bool avg, const float* tapw, int r, int B,
               int n, int V, int* cnt_out, const SegPlan& w, hipStream_t st) {
  const int koff = seg_koff(V, TAPS);
  PCFM_CHECK_ARG(koff == 0 || (cnt_out == nullptr && !avg),
                 "segment plan: counts of a shifted-key sort");
  const int e = seg_sort(key, key_bstride, B, n, V + koff, koff, w.start, cnt_out,
                         avg ? w.vinv : nullptr, w.rank, st);
  if (e) return e;
  const int tiles = seg_tiles(V), umax = seg_umax(n, V, TAPS);
  hipLaunchKernelGGL(seg_units_kernel<TAPS>, dim3(B), dim3(1024), 0, st, w.start, V, r, tiles,
                     umax, w.units, w.tinfo, w.nunits);
  if (n > 0)
    hipLaunchKernelGGL(seg_plan_rows_kernel, dim3(ceil_div(n, 256), B), dim3(256), 0, st, w.rank,
                       key, key_bstride, TAPS == 8 ? tapw : nullptr, n, w.skey, w.ws8);
  return PCFM_OK;
}

template <int TAPS>
int apply(const float* in, const SegPlan& w, bool avg, int r, int B, int C, int n, int V,
          float* out, const SegApplyWs& aw, hipStream_t st) {
  if (C == 0) return PCFM_OK;
  if (TAPS == 1 && n <= kLdsRowMaxItems && seg_ldsrow_enabled()) {
    const int e = allow_big_lds((const void*)seg_ldsrow1_kernel);
    if (e) return e;
    hipLaunchKernelGGL(seg_ldsrow1_kernel, dim3(C, B), dim3(kRowThreads), seg_ldsrow_lds(n), st,
                       in, w.rank, w.start, avg ? 1 : 0, C, n, V, out);
    return PCFM_OK;
  }
  const int tiles = seg_tiles(V), umax = seg_umax(n, V, TAPS), slots = umax - tiles;
  if (n > 0)
    hipLaunchKernelGGL(seg_rows_kernel, dim3(ceil_div(n, 64), 1, B), dim3(256), 0, st, in, w.rank,
                       C, n, aw.xs);
  const int gx = ceil_div(umax, kUnitWaves);
  hipLaunchKernelGGL(seg_unit_gather_kernel<TAPS>, dim3(gx, ceil_div(C, 64), B),
                     dim3(kUnitWaves * 64), 0, st, aw.xs, w.skey, w.ws8, w.start,
                     avg ? w.vinv : nullptr, w.units, w.nunits, C, n, V, r, umax, slots, out,
                     aw.partial);
  hipLaunchKernelGGL(seg_part_sum_kernel, dim3(tiles, ceil_div(C, 64), B), dim3(256), 0, st,
                     w.tinfo, aw.partial, C, V, tiles, slots, out);
  return PCFM_OK;
}

}  // namespace

int seg_sort(const int* key, long long key_bstride, int B, int n, int V, int koff, int* start,
             int* cnt_out, float* vinv, int* rank, hipStream_t st) {
  const int e = allow_big_lds((const void*)seg_sort_kernel);
  if (e) return e;
  hipLaunchKernelGGL(seg_sort_kernel, dim3(seg_sort_parts(V), B), dim3(1024), seg_sort_lds(V), st,
                     key, key_bstride, n, V, seg_sort_span(V), start, cnt_out, vinv, rank, koff);
  return PCFM_OK;
}

int seg_plan_build(int taps, const int* key, long long key_bstride, bool avg, const float* tapw,
                   int r, int B, int n, int V, int* cnt_out, const SegPlan& w, hipStream_t st) {
  return taps == 8 ? plan_build<8>(key, key_bstride, avg, tapw, r, B, n, V, cnt_out, w, st)
                   : plan_build<1>(key, key_bstride, avg, tapw, r, B, n, V, cnt_out, w, st);
}

int seg_apply(int taps, const float* in, const SegPlan& w, bool avg, int r, int B, int C, int n,
              int V, float* out, const SegApplyWs& aw, hipStream_t st) {
  return taps == 8 ? apply<8>(in, w, avg, r, B, C, n, V, out, aw, st)
                   : apply<1>(in, w, avg, r, B, C, n, V, out, aw, st);
}

int seg_scatter(int taps, const float* in, const int* key, long long key_bstride, bool avg,
                const float* tapw, int r, int B, int C, int n, int V, int* cnt_out, float* out,
                void* ws, hipStream_t st, const char* what) {
  if (B == 0 || V == 0) return PCFM_OK;
  const SegPlan w = seg_plan_carve(ws, B, n, V, taps);
  const SegApplyWs aw =
      seg_apply_carve((char*)ws + seg_plan_bytes(B, n, V, taps), B, C, n, V, taps);
  int e = seg_plan_build(taps, key, key_bstride, avg, tapw, r, B, n, V, cnt_out, w, st);
  if (e) return e;
  e = seg_apply(taps, in, w, avg, r, B, C, n, V, out, aw, st);
  if (e) return e;
  return check_launch(what);
}

}  // namespace pcfm
