// The squared-distance chain of the D-component nearest-neighbour kernels
// (csrc/chamfer_nd.hip, csrc/chamfer_cross.hip; include/pcfm_chamfer_nd.h), in
// one place so that both return the same bits for the same pair of points.
#pragma once

#include <hip/hip_runtime.h>

namespace pcfm {

// candidates per wave-uniform group load: a group and the prefetched next one
// are 2 * group_of(D) * D SGPRs, 48 at most
constexpr int group_of(int d) { return d <= 3 ? 8 : 4; }

// c, q: D components each.  ONE fixed fp32 chain (the build has
// -ffp-contract=off):
//   acc = d1*d1; acc = fma(d0, d0, acc); acc = fma(dk, dk, acc) for k = 2..D-1,
//   dk = c[k] - q[k]
// (c - q)^2 and (q - c)^2 have the same bits, so the direction does not matter.
// At D = 3 that is sqdist3 (pcfm_common.hpp).
template <int D>
__device__ __forceinline__ float sqdist_nd(const float* c, const float* q) {
  const float d1 = c[1] - q[1];
  float acc = d1 * d1;
  const float d0 = c[0] - q[0];
  acc = __builtin_fmaf(d0, d0, acc);
#pragma unroll
  for (int k = 2; k < D; ++k) {
    const float dk = c[k] - q[k];
    acc = __builtin_fmaf(dk, dk, acc);
  }
  return acc;
}

}  // namespace pcfm
