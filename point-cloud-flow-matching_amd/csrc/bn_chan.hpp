// One channel of a training-mode BatchNorm followed by its activation
// (ReLU: slope 0, LeakyReLU: slope 0.1), as every kernel that applies it or
// differentiates through it evaluates it: the contiguous and split apply
// passes and the statistics passes (norm.hip), the GroupNorm passes that read
// a SharedMLP layer as its pre-BatchNorm tensor (norm.hip), and the
// devoxelization gather that stages act(bn(x)) rows (rows.hpp).  The library
// is built with -ffp-contract=off, so these expression trees ARE the results:
// a tensor one kernel does not write is bit-identical to what another kernel
// recomputes because both call the functions below.
#pragma once

#include <hip/hip_runtime.h>

namespace pcfm {

// one channel's constants
struct BnChan {
  float m, is, g, bt, slope;
  // A NaN argument stays NaN at either slope (F.relu, F.leaky_relu): the negative
  // branch takes what compares <= 0, so a NaN is not selected into it.
  static __device__ __forceinline__ float act(float t, float slope) {
    return t <= 0.0f ? (slope == 0.0f ? 0.0f : t * slope) : t;
  }
  // whether the unit passes its gradient unscaled, as torch's backward decides it:
  // ReLU's from its result (0 where that compares <= 0, so a NaN passes),
  // LeakyReLU's from its argument (slope unless that compares > 0)
  static __device__ __forceinline__ bool passes(float t, float slope) {
    return slope == 0.0f ? !(t <= 0.0f) : t > 0.0f;
  }
  // d act / d t
  static __device__ __forceinline__ float dact(float t, float slope) {
    return passes(t, slope) ? 1.0f : slope;
  }
  // dz * dact(t); a dead ReLU unit gives 0 (torch's threshold backward), not
  // dz * 0: a non-finite dz does not pass it
  static __device__ __forceinline__ float gate(float t, float slope, float dz) {
    return passes(t, slope) ? dz : (slope == 0.0f ? 0.0f : dz * slope);
  }
  __device__ __forceinline__ float xhat(float v) const { return (v - m) * is; }
  // the activation's argument bn(v)
  __device__ __forceinline__ float pre(float v) const { return __builtin_fmaf(xhat(v), g, bt); }
  __device__ __forceinline__ float z(float v) const { return act(pre(v), slope); }
  __device__ __forceinline__ float4 z(float4 v) const {
    return make_float4(z(v.x), z(v.y), z(v.z), z(v.w));
  }
  // dz * act'(bn(v)): the gradient entering the BatchNorm
  __device__ __forceinline__ float grad(float v, float dz) const {
    return gate(pre(v), slope, dz);
  }
  // the BatchNorm input's gradient, mg = sum grad / n and mgx = sum grad * xhat / n
  // over the channel
  __device__ __forceinline__ float dx(float v, float dz, float mg, float mgx) const {
    return (g * is) * ((grad(v, dz) - mg) - xhat(v) * mgx);
  }
};

// The operands [C] of such a BatchNorm; mean == nullptr: no BatchNorm (identity).
struct BnParam {
  const float* mean = nullptr;
  const float* invstd = nullptr;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  float slope = 0.0f;
  // mean != nullptr
  __device__ __forceinline__ BnChan at(int c) const {
    return BnChan{mean[c], invstd[c], gamma[c], beta[c], slope};
  }
  // z(v) == v when mean == nullptr
  __device__ __forceinline__ BnChan at_or_identity(int c) const {
    if (mean == nullptr) return BnChan{0.0f, 1.0f, 1.0f, 0.0f, 1.0f};
    return at(c);
  }
  bool complete() const {
    return mean != nullptr && invstd != nullptr && gamma != nullptr && beta != nullptr;
  }
};

}  // namespace pcfm
