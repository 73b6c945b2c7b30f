// D-component points, once: which widths the point-cloud kernels take, the
// runtime d -> template D dispatch, the squared distance, and the packed
// (float bits, index) ordering keys of every argmin / argmax over points.
#pragma once

#include "pcfm_common.hpp"

#include <type_traits>
#include <utility>

namespace pcfm {

// The point widths of the N-D entries (Chamfer, cross-set Chamfer, FPS, both
// EMDs): xy, xyz, xyz + 2 and xyz + rgb.
constexpr bool point_dim_ok(int d) { return d == 2 || d == 3 || d == 5 || d == 6; }

// f(integral_constant<int, d>) for a d that point_dim_ok has accepted
template <class F>
void with_dim(int d, F&& f) {
  switch (d) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 6>{}); break;
  }
}

// c, q: D components each, float or double (the EMD's double entries).  ONE
// fixed chain (the build has -ffp-contract=off):
//   acc = d1*d1; acc = fma(d0, d0, acc); acc = fma(dk, dk, acc) for k = 2..D-1,
//   dk = c[k] - q[k]
// (c - q)^2 and (q - c)^2 have the same bits, so the direction does not matter.
// At D = 3 that is sqdist3 (pcfm_common.hpp), the oracle's chain, in both types;
// fmaT is its fused multiply-add by type.
template <int D, typename T>
__device__ __forceinline__ T sqdist_nd(const T* c, const T* q) {
  const T d1 = c[1] - q[1];
  T acc = d1 * d1;
  const T d0 = c[0] - q[0];
  acc = fmaT<T>(d0, d0, acc);
#pragma unroll
  for (int k = 2; k < D; ++k) {
    const T dk = c[k] - q[k];
    acc = fmaT<T>(dk, dk, acc);
  }
  return acc;
}

// Ordering keys: a value's bits in the high word, a point's index in the low
// word, compared as ONE unsigned 64-bit number, so the result of a reduction
// does not depend on the order its operands arrive in.  `hi` is the bits of a
// float >= +0 (they order like the values) or any other 32-bit rank.
//
// Min-ordered: the smallest hi, the lowest index among equals (atomicMin).
__host__ __device__ __forceinline__ u64 min_key(u32 hi, int idx) {
  return ((u64)hi << 32) | (u32)idx;
}
// Max-ordered: the largest hi, the lowest index among equals (wave_umax,
// atomicMax); no index below 2^31 gives key 0, which stands for "nothing".
__host__ __device__ __forceinline__ u64 max_key(u32 hi, int idx) {
  return ((u64)hi << 32) | ~(u32)idx;
}
__host__ __device__ __forceinline__ u32 key_hi(u64 key) { return (u32)(key >> 32); }
__host__ __device__ __forceinline__ int min_key_index(u64 key) { return (int)(u32)key; }
__host__ __device__ __forceinline__ int max_key_index(u64 key) { return (int)~(u32)key; }

}  // namespace pcfm
