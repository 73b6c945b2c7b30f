// Host interface of the sorted, atomic-free scatter ("segment sum") engine of
// the PVConv path: sizes, buffer layouts and the entry points.  The kernels,
// the host driver and the account of how the engine works are in segsum.hip.
//
// Used by avg_voxelize forward (key = voxel, term = feat * (1/cnt)),
// trilinear devoxelize backward (key = base cell inds[b,0,:], term = wgt * g
// for the 8 corners), grouping backward (key = neighbour index, term = g) and,
// for its stable sort alone, the Chamfer cull.
#pragma once

#include <algorithm>

#include "pcfm_common.hpp"

namespace pcfm {

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Key shift of a scatter's sort.  The trilinear stencil (taps == 8) reaches
// from a point's base cell q to q + dx r^2 + dy r + dz (dx, dy, dz in {0, 1}),
// so a point whose base cell lies below the volume (coordinates outside
// [0, r - 1]: a negative linear index) can still have corners inside it, and
// the forward reads them (trilinear_devox.cu:64-105).  Its sort key is q + koff
// with koff = r^2 + r + 1, over V + koff keys: every point with a corner in
// [0, V) is kept.  (Keys >= V have every corner >= V: dropped.)
constexpr int seg_koff(int V, int taps) {
  if (taps != 8) return 0;
  int r = 1;
  while ((long long)r * r * r < V) ++r;
  return r * r + r + 1;
}
constexpr int seg_keys(int V, int taps) { return V + seg_koff(V, taps); }

constexpr int kTV = 16;      // voxels per output tile
constexpr int kItems = 256;  // target items per work unit

constexpr int seg_tiles(int V) { return (V + kTV - 1) / kTV; }
// Upper bound of work units per batch element: one per tile plus one per
// kItems of range items (an item lies in at most 2 tiles per stencil column).
constexpr int seg_umax(int n, int V, int taps) {
  return seg_tiles(V) + (int)(((long long)(taps == 8 ? 8 : 1) * n + kItems - 1) / kItems) + 1;
}

// A buffer cut into N regions in order, each padded to 256 bytes: the one walk
// that both the byte count and the carve go through.
template <int N>
struct SegLayout {
  size_t at[N] = {}, size[N] = {}, bytes = 0;
  constexpr explicit SegLayout(const size_t (&sizes)[N]) {
    for (int i = 0; i < N; ++i) {
      at[i] = bytes;
      size[i] = sizes[i];
      bytes += align256(sizes[i]);
    }
  }
  // every region starts 256-aligned and past the one before; the walk ends at `bytes`
  constexpr bool ok() const {
    size_t end = 0;
    for (int i = 0; i < N; ++i) {
      if (at[i] % 256 != 0 || at[i] < end) return false;
      end = at[i] + size[i];
    }
    return bytes % 256 == 0 && bytes >= end && bytes - end < 256;
  }
  template <class T>
  T* ptr(void* mem, int i) const { return reinterpret_cast<T*>((char*)mem + at[i]); }
};

// A scatter = plan (sort the items by key, cut the output into work units,
// gather the sorted keys / tap weights) + apply (channels-last rows, unit
// gather, partial sums).  The plan depends only on the keys, so scatters over
// the same points share it (include/pcfm.h, "segment plans").
struct SegPlan {
  int* start;      // B*(VK+1), VK = seg_keys(V, taps)
  float* vinv;     // B*V (per-voxel 1/cnt)
  int* rank;       // B*n
  int* skey;       // B*n
  float* ws8;      // B*n*8 (taps == 8; no bytes and nullptr otherwise)
  int4* units;     // B*umax
  int2* tinfo;     // B*tiles
  int* nunits;     // B
};
struct SegApplyWs {
  float* xs;       // B*n*C
  float* partial;  // B*slots*C*kTV, slots = umax - tiles
};

constexpr SegLayout<8> seg_plan_layout(int B, int n, int V, int taps) {
  const int umax = seg_umax(n, V, taps), tiles = seg_tiles(V);
  return SegLayout<8>({(size_t)B * (seg_keys(V, taps) + 1) * 4, (size_t)B * V * 4,
                       (size_t)B * n * 4, (size_t)B * n * 4,
                       taps == 8 ? (size_t)B * n * 8 * 4 : 0, (size_t)B * umax * 16,
                       (size_t)B * tiles * 8, (size_t)B * 4});
}
constexpr SegLayout<2> seg_apply_layout(int B, int C, int n, int V, int taps) {
  const int slots = seg_umax(n, V, taps) - seg_tiles(V);
  return SegLayout<2>({(size_t)B * n * std::max(C, 1) * 4,
                       (size_t)B * slots * std::max(C, 1) * kTV * 4});
}

constexpr bool seg_layouts_ok() {
  for (int B : {0, 1, 3, 8, 64})
    for (int n : {0, 1, 255, 257, 4097, 20000, 40001})
      for (int V : {0, 1, 8, 64, 4096, 32768})
        for (int taps : {1, 8}) {
          if (!seg_plan_layout(B, n, V, taps).ok()) return false;
          for (int C : {0, 1, 70, 256})
            if (!seg_apply_layout(B, C, n, V, taps).ok()) return false;
        }
  return true;
}
static_assert(seg_layouts_ok(), "segment layouts: a region unaligned, overlapping or past the end");

inline size_t seg_plan_bytes(int B, int n, int V, int taps) {
  return seg_plan_layout(B, n, V, taps).bytes;
}
inline size_t seg_apply_bytes(int B, int C, int n, int V, int taps) {
  return seg_apply_layout(B, C, n, V, taps).bytes;
}
// plan + apply in one workspace: the unshared scatter (seg_scatter)
inline size_t seg_ws_bytes(int B, int C, int n, int V, int taps) {
  return seg_plan_bytes(B, n, V, taps) + seg_apply_bytes(B, C, n, V, taps);
}

inline SegPlan seg_plan_carve(void* mem, int B, int n, int V, int taps) {
  const SegLayout<8> l = seg_plan_layout(B, n, V, taps);
  return SegPlan{l.ptr<int>(mem, 0),  l.ptr<float>(mem, 1),
                 l.ptr<int>(mem, 2),  l.ptr<int>(mem, 3),
                 taps == 8 ? l.ptr<float>(mem, 4) : nullptr,
                 l.ptr<int4>(mem, 5), l.ptr<int2>(mem, 6),
                 l.ptr<int>(mem, 7)};
}
inline SegApplyWs seg_apply_carve(void* mem, int B, int C, int n, int V, int taps) {
  const SegLayout<2> l = seg_apply_layout(B, C, n, V, taps);
  return SegApplyWs{l.ptr<float>(mem, 0), l.ptr<float>(mem, 1)};
}

// Entry points (segsum.hip); taps is 1 or 8.  Each returns PCFM_OK or an error
// code with pcfm_last_error set; launches are checked by the caller
// (check_launch) except in seg_scatter, which does it itself.

// The stable counting sort alone: start[b, 0..V] and rank[b, i] of the keys
// key[b * key_bstride + i] + koff over the key range [0, V); cnt_out [b, V]
// and vinv [b, V] (1 / count) are optional.
int seg_sort(const int* key, long long key_bstride, int B, int n, int V, int koff, int* start,
             int* cnt_out, float* vinv, int* rank, hipStream_t st);

// The plan of a scatter over items with keys at key + b*key_bstride (first n
// used): the stable sort (+ cnt_out [b, V] counts when non-null; 1/cnt when
// avg), the work units and the sorted keys / tap weights (tapw [b, 8, n] for
// taps == 8).
int seg_plan_build(int taps, const int* key, long long key_bstride, bool avg, const float* tapw,
                   int r, int B, int n, int V, int* cnt_out, const SegPlan& w, hipStream_t st);

// out[b, c, v] = sum over items i whose key (+ stencil offset) is v of the tap
// term, on a built plan (avg: scaled by the plan's 1/cnt).
int seg_apply(int taps, const float* in, const SegPlan& w, bool avg, int r, int B, int C, int n,
              int V, float* out, const SegApplyWs& aw, hipStream_t st);

// plan + apply in one workspace of seg_ws_bytes.
int seg_scatter(int taps, const float* in, const int* key, long long key_bstride, bool avg,
                const float* tapw, int r, int B, int C, int n, int V, int* cnt_out, float* out,
                void* ws, hipStream_t st, const char* what);

}  // namespace pcfm
