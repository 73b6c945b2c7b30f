// Shared helpers for the gfx950 kernels behind include/pcfm.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "../../include/pcfm.h"

namespace pcfm {

// Thread-local last-error text (pcfm_last_error).
void set_error(const char* fmt, ...);

// Host-side argument check: returns PCFM_EINVAL with a message when !cond.
#define PCFM_CHECK_ARG(cond, ...)            \
  do {                                       \
    if (!(cond)) {                           \
      ::pcfm::set_error(__VA_ARGS__);        \
      return PCFM_EINVAL;                    \
    }                                        \
  } while (0)

// After a group of launches: map the sticky launch error to a return code.
int check_launch(const char* what);

// Every 64-bit index computation goes through size_t; kernels take int sizes
// that fit the reference's own int arithmetic.
inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

constexpr int kCUs = 256;           // MI355X: 8 XCDs x 32 CUs
constexpr int kLdsBytesMax = 160 * 1024;

// Raise the dynamic-LDS cap of one kernel to the gfx950 maximum once.
int allow_big_lds(const void* kernel);

// Whole-CU residency for a kernel whose block puts W waves on each SIMD: naming
// register v(512 / W - 1) in a clobber makes the kernel descriptor allocate
// 512 / W VGPRs per lane (granule 8), so the block's waves take every register
// of the CU's four SIMDs and no wave of another kernel (any kernel that needs
// more than 8 VGPRs) can be resident on the CU beside them.  Used by the
// LDS-DMA weight gradient ("co-residence").
#define PCFM_CLAIM_VGPRS(last) asm volatile("" ::: "v" #last)

// Split operands (bf16 hi / lo of an fp32 tensor, channels-last rows of C
// channels, C % 32 == 0) are stored interleaved per 32-channel group: row r
// holds [hi c0..c31 | lo c0..c31 | hi c32..c63 | lo c32..c63 | ...], so the
// hi and lo halves of one K-step of 32 channels share one 128-byte line (a
// step fetches whole lines, not halves of lines it reads the rest of 27 steps
// later).  Element offset of (row, channel c) in hi; its lo is 32 further.
__host__ __device__ inline size_t split_off(size_t row, int c, int C) {
  return row * 2 * (size_t)C + (size_t)(((c >> 5) << 6) + (c & 31));
}
constexpr int kSplitLo = 32;  // element offset of lo from hi

// Squared distance contract shared by every nearest-neighbour kernel and the
// oracle: dx = q - p;  d = fma(dz, dz, fma(dx, dx, dy*dy)).
// (This is how NVVM contracts the reference's `x*x + y*y + z*z`; pinned here
// explicitly so the order does not depend on the compiler.)
__device__ __forceinline__ float sqdist3(float dx, float dy, float dz) {
  return __builtin_fmaf(dz, dz, __builtin_fmaf(dx, dx, dy * dy));
}
__device__ __forceinline__ double sqdist3(double dx, double dy, double dz) {
  return __builtin_fma(dz, dz, __builtin_fma(dx, dx, dy * dy));
}

// The explicit fused multiply-add of a kernel templated on its scalar type.
template <typename T>
__device__ __forceinline__ T fmaT(T a, T b, T c);
template <>
__device__ __forceinline__ float fmaT<float>(float a, float b, float c) {
  return __builtin_fmaf(a, b, c);
}
template <>
__device__ __forceinline__ double fmaT<double>(double a, double b, double c) {
  return __builtin_fma(a, b, c);
}

// Wave-wide (64 lanes) butterfly reductions.  wave_add (float, double, int)
// turns an accumulator into the wave's sum in every lane, added in ONE order --
// xor offsets 32 down to 1 -- which is part of every deterministic sum built on
// it; wave_sum is the same as an expression.  wave_max / wave_min return their
// result wave-uniform (one scalar register).
template <typename T>
__device__ __forceinline__ void wave_add(T& x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
}
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
  wave_add(x);
  return x;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
typedef unsigned int u32;
typedef unsigned long long u64;   // what the 64-bit atomics take

// The wave's largest unsigned value, in every lane: a max-scan by
// data-parallel-primitive moves (a lane without a source reads 0, below every
// key in use) leaves it in lane 63, which is read back wave-uniform.  No LDS
// traffic.  With the ordering keys of points.hpp this is a wave argmax / argmin.
template <int CTRL, int ROWS>
__device__ __forceinline__ u32 dpp_umax(u32 v) {
  const u32 o = __builtin_amdgcn_update_dpp(0u, v, CTRL, ROWS, 0xf, false);
  return o > v ? o : v;
}
template <int CTRL, int ROWS>
__device__ __forceinline__ u64 dpp_umax(u64 v) {
  const u32 lo = __builtin_amdgcn_update_dpp(0u, (u32)v, CTRL, ROWS, 0xf, false);
  const u32 hi = __builtin_amdgcn_update_dpp(0u, (u32)(v >> 32), CTRL, ROWS, 0xf, false);
  const u64 o = ((u64)hi << 32) | lo;
  return o > v ? o : v;
}
__device__ __forceinline__ u32 lane63(u32 v) { return __builtin_amdgcn_readlane(v, 63); }
__device__ __forceinline__ u64 lane63(u64 v) {
  return ((u64)lane63((u32)(v >> 32)) << 32) | lane63((u32)v);
}
template <class T>
__device__ __forceinline__ T wave_umax(T v) {
  v = dpp_umax<0x111, 0xf>(v);   // row_shr:1
  v = dpp_umax<0x112, 0xf>(v);   // row_shr:2
  v = dpp_umax<0x114, 0xf>(v);   // row_shr:4
  v = dpp_umax<0x118, 0xf>(v);   // row_shr:8: lane 15 of a row holds the row's
  v = dpp_umax<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_umax<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3: lane 63 holds all
  return lane63(v);
}

// lane l's value of v, wave-uniform (v_readlane; l uniform)
__device__ __forceinline__ float rlf(float v, int l) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// bf16 bits (low 16 of b; the higher bits are shifted out) widened to fp32, and
// fp32 rounded to bf16 bits by the compiler's cast (v_cvt_pk_bf16_f32, nearest
// even).  mfma_x3.hpp's bf16_bits is the same rounding in integer arithmetic
// with the NaN result pinned to (bits >> 16) | 0x40; the cast leaves a NaN's
// bits to the hardware, so the two are not interchangeable where a NaN's bits
// are part of a pinned result.
__device__ __forceinline__ float bf2f(uint32_t b) { return __uint_as_float(b << 16); }
__device__ __forceinline__ uint32_t f2bf(float x) {
  return (uint32_t)__builtin_bit_cast(uint16_t, (__bf16)x);
}

// The ordered sum of S partials -- the determinism contract of the split
// gradients (pointwise and head weight gradients, column sums, FiLM backward
// sums).  A 256-thread block owns 64 outputs: thread t serves output t % 64 in
// group g = t / 64, and p points at partial 0 of that output, partial q lying
// at p[q * stride].  A thread past the last output passes live = false: it
// reads nothing and still joins the barrier.  Group g adds partials g, g + 4,
// ... in that order, 4 of them loaded before they are added while q + 12 < S (a
// thread otherwise chains S / 4 dependent loads), and the groups combine as
// ((r0 + r1) + r2) + r3.  Every thread returns the sum; one call per kernel
// (the barrier is block-wide).
__device__ __forceinline__ float ordered_sum4(const float* __restrict__ p, size_t stride, int S,
                                              bool live) {
  __shared__ float red[4][64];
  const int cl = threadIdx.x & 63, grp = threadIdx.x >> 6;
  float sum = 0.0f;
  if (live) {
    int q = grp;
    for (; q + 12 < S; q += 16) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = p[(size_t)(q + 4 * u) * stride];
#pragma unroll
      for (int u = 0; u < 4; ++u) sum = sum + v[u];
    }
    for (; q < S; q += 4) sum = sum + p[(size_t)q * stride];
  }
  red[grp][cl] = sum;
  __syncthreads();
  return ((red[0][cl] + red[1][cl]) + red[2][cl]) + red[3][cl];
}

// A 1-D grid's block id dealt to the 8 XCDs in contiguous runs (T1 remap):
// hardware sends block i to XCD i % 8; the id returned makes each XCD sweep one
// contiguous eighth of [0, nwg), so concurrently resident blocks share rows in
// their XCD's L2 instead of streaming them from the Infinity Cache.
__device__ __forceinline__ int xcd_deal(int id, int nwg) {
  const int q = nwg / 8, rr = nwg % 8, xcd = id % 8;
  return (xcd < rr ? xcd * (q + 1) : rr * (q + 1) + (xcd - rr) * q) + id / 8;
}

// Block index walked in reverse (a second pass over data a first pass just
// read in forward order finds its most recent rows in the Infinity Cache).
#ifndef PCFM_REV_APPLY
#define PCFM_REV_APPLY 1
#endif
__device__ __forceinline__ unsigned rev_order(unsigned i, unsigned n) {
  return PCFM_REV_APPLY ? n - 1 - i : i;
}

// Streamed (non-temporal) global accesses for outputs next read by another
// kernel and inputs read once; PCFM_NT=0 builds them as plain accesses
// (measurement / diagnosis switch).
#ifndef PCFM_NT
#define PCFM_NT 1
#endif
template <class T>
__device__ __forceinline__ void nt_st(T v, T* p) {
#if PCFM_NT
  __builtin_nontemporal_store(v, p);
#else
  *p = v;
#endif
}
template <class T>
__device__ __forceinline__ T nt_ld(const T* p) {
#if defined(PCFM_COHERENT_LD) && PCFM_COHERENT_LD
  // diagnosis switch: device-coherent (agent-scope) load, no stale cache line
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#elif PCFM_NT
  return __builtin_nontemporal_load(p);
#else
  return *p;
#endif
}

}  // namespace pcfm
