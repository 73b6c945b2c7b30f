// BatchNorm with batch statistics (training mode) fused with the activation
// that follows it everywhere on the PVConv path:
//   SharedMLP  (third_party/pvcnn/modules/shared_mlp.py:15-27): BN1d -> ReLU
//   PVConv     (third_party/pvcnn/modules/pvconv.py:20-30):     BN3d -> LeakyReLU(0.1)
// over (B, C, S) fp32 tensors (S = points or voxels), the layout the
// reference's Conv1d / Conv3d produce.  torch runs these as MIOpen BN + a
// separate (in-place) activation, and a threshold / leaky backward + MIOpen
// BN backward: ~12 full passes over the tensor per layer.  Here:
//   forward : stats pass (read x) -> per-channel finalize (mean, invstd,
//             running-stat update) -> apply pass (read x, write act(bn(x)))
//   backward: stats pass (read dz, x: sum g, sum g*xhat with g = dz * act')
//             -> finalize (dgamma, dbeta) -> apply pass (read dz, x, write dx)
// 8 passes.  Partial sums are per (channel, part) block and combined in a
// fixed order: deterministic.  The forward sums are shifted by the channel's
// first element (sum (x - K), sum (x - K)^2) against cancellation.
//
// Every pass is assembled from a few pieces, each written once:
//   BnChan (bn_chan.hpp)   one channel's xhat / act(bn(.)) / gradient / dx
//   strip_reduce           the statistics passes' walk over a row strip
//   block_sum2, sum_parts2 the block reduction and the ordered sum of partials
//   BnFwdFin::get/publish  the forward finalize (statistics from partials,
//                          mean / invstd / running statistics written once)
//   tile_store_split, tile_rowsum   the split kernels' 64 x 64 tile epilogues
//   bn_out_store4, gn_out_store4    the store policy of the BN / GN outputs
#include <algorithm>

#include "bn_chan.hpp"
#include "pcfm_common.hpp"

namespace pcfm {
namespace {

// streamed 16-B store (the output is next read by another kernel, > L2)
__device__ __forceinline__ void nt_store4(float4* p, float4 v) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  nt_st(v4f{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f*>(p));
}
// The BatchNorm passes' outputs are streamed: bwd apply 148 -> 128 us at C256
// N20000 (tools/bn_ab.py); -DPCFM_BN_CACHED_STORE builds the plain store.
__device__ __forceinline__ void bn_out_store4(float4* p, float4 v) {
#ifndef PCFM_BN_CACHED_STORE
  nt_store4(p, v);
#else
  *p = v;
#endif
}
// The GroupNorm passes' outputs are plain stores; -DPCFM_GN_NT_STORE streams them.
__device__ __forceinline__ void gn_out_store4(float4* p, float4 v) {
#ifdef PCFM_GN_NT_STORE
  nt_store4(p, v);
#else
  *p = v;
#endif
}

constexpr int kBnParts = 16;  // target blocks per channel in the stats passes
constexpr int kBnUnroll = 4;  // float4 loads per thread issued together in the stats passes
inline int bn_parts(int b) { return b * ((kBnParts + b - 1) / b); }

// Block-wide sum of two values (256 threads); result valid in thread 0.
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off, 64);
    b += __shfl_xor(b, off, 64);
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
    sh[2 * w] = a;
    sh[2 * w + 1] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = ((sh[0] + sh[2]) + sh[4]) + sh[6];
    b = ((sh[1] + sh[3]) + sh[5]) + sh[7];
  }
}

// block_sum2, then thread 0 writes the pair to dst[0], dst[1] (one slot of a
// partials array)
__device__ __forceinline__ void block_sum2_to(float a, float b, float* sh, float* dst) {
  block_sum2(a, b, sh);
  if (threadIdx.x == 0) {
    dst[0] = a;
    dst[1] = b;
  }
}

// s += sum of (v - K), q += sum of (v - K)^2 over a float4: the shifted moments
// of the BatchNorm and GroupNorm forward statistics
__device__ __forceinline__ void add_shifted(float4 v, float K, float& s, float& q) {
  const float d0 = v.x - K, d1 = v.y - K, d2 = v.z - K, d3 = v.w - K;
  s += (d0 + d1) + (d2 + d3);
  q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
}

// Stats passes: part p = (b, ps) of channel c covers float4s
// [ps * chunk, (ps + 1) * chunk) of row (b, c), PS = P / B parts per row.
__device__ __forceinline__ void part_range(int S4, int ps, int PS, int& s0, int& s1) {
  const int chunk = (S4 + PS - 1) / PS;
  s0 = min(S4, chunk * ps);
  s1 = min(S4, chunk * (ps + 1));
}

// A 256-thread block's walk over float4s [s0, s1) of R rows read in step:
// add(v) sees v[r] = row[r][s4] for s4 = s0 + thread, + 256, ... in that order
// (the per-thread summation order of one-at-a-time); only the loads move up,
// kBnUnroll float4s per row in flight per thread before the first use.
template <int R, class F>
__device__ __forceinline__ void strip_reduce(const float4* const (&row)[R], int s0, int s1,
                                             F add) {
  int s4 = s0 + threadIdx.x;
  for (; s4 + (kBnUnroll - 1) * 256 < s1; s4 += kBnUnroll * 256) {
    float4 v[kBnUnroll][R];
#pragma unroll
    for (int u = 0; u < kBnUnroll; ++u)
#pragma unroll
      for (int r = 0; r < R; ++r) v[u][r] = row[r][s4 + u * 256];
#pragma unroll
    for (int u = 0; u < kBnUnroll; ++u) add(v[u]);
  }
  for (; s4 < s1; s4 += 256) {
    float4 v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = row[r][s4];
    add(v);
  }
}

// grid = (C, P), 256 threads.  part[c][p] = (sum (x-K), sum (x-K)^2), K = x[0][c][0].
__global__ void __launch_bounds__(256)
    bn_stats_kernel(const float* __restrict__ x, int B, int C, int S, float* __restrict__ part) {
  __shared__ float sh[8];
  const int c = blockIdx.x, p = blockIdx.y, P = gridDim.y;
  const int S4 = S / 4;
  const float K = x[(size_t)c * S];
  const int PS = P / B, b = p / PS;
  int s0, s1;
  part_range(S4, p - b * PS, PS, s0, s1);
  const float4* const row[1] = {reinterpret_cast<const float4*>(x) + ((size_t)b * C + c) * S4};
  float s = 0.0f, q = 0.0f;
  strip_reduce(row, s0, s1, [&](const float4(&v)[1]) { add_shifted(v[0], K, s, q); });
  block_sum2_to(s, q, sh, part + ((size_t)c * P + p) * 2);
}

// s = sum of part[2p], q = sum of part[2p + 1] over p < P, added in p order;
// 8 partials' loads in flight at a time (the serial form kept the thread that
// derives a block's statistics waiting on one load per partial)
__device__ __forceinline__ void sum_parts2(const float* __restrict__ part, int P, float& s,
                                           float& q) {
  const float2* __restrict__ p2 = reinterpret_cast<const float2*>(part);
  s = 0.0f;
  q = 0.0f;
  int p = 0;
  for (; p + 8 <= P; p += 8) {
    float2 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p2[p + u];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s += v[u].x;
      q += v[u].y;
    }
  }
  for (; p < P; ++p) {
    const float2 v = p2[p];
    s += v.x;
    q += v.y;
  }
}

// The forward finalize: one channel's mean, invstd (biased variance, as BN
// normalises) and the running-stat update with the unbiased variance (torch's
// batch_norm).  It runs as a kernel of its own (bn_finalize_kernel) or folded
// into the apply passes (one launch less): every apply block derives its
// channel's statistics from the P partials with get(), and one designated
// block per channel publishes them.
struct BnStat {
  float m, is, var;
  double n;  // values the statistics are over
};
// a variance's clamp at 0 that keeps a NaN (fmaxf returns its other operand)
__device__ __forceinline__ float clamp_var(float v) { return v < 0.0f ? 0.0f : v; }
// from s = sum (x - K), q = sum (x - K)^2 over n values (GroupNorm's groups too)
__device__ __forceinline__ BnStat stat_of_shifted(float s, float q, double n, float K, float eps) {
  BnStat st;
  st.n = n;
  const float md = (float)(s / n);
  st.var = clamp_var((float)(q / n) - md * md);
  st.m = K + md;
  st.is = rsqrtf(st.var + eps);
  return st;
}
struct BnFwdFin {
  const float* part;  // [C][P] of bn_stats_kernel; NULL: mean / invstd are final already
  int B, S, P;
  float eps, momentum;
  float* rmean;
  float* rvar;
  long long* nbt;  // BatchNorm num_batches_tracked (+1 by channel 0's publisher), or NULL
  __device__ __forceinline__ BnStat get(const float* x, int c) const {
    float s, q;
    sum_parts2(part + (size_t)c * P * 2, P, s, q);
    return stat_of_shifted(s, q, (double)B * S, x[(size_t)c * S], eps);
  }
  __device__ __forceinline__ void publish(int c, const BnStat& st, float* mean,
                                          float* invstd) const {
    mean[c] = st.m;
    invstd[c] = st.is;
    if (rmean != nullptr) {
      rmean[c] = (1.0f - momentum) * rmean[c] + momentum * st.m;
      rvar[c] = (1.0f - momentum) * rvar[c] + momentum * (float)(st.var * st.n / (st.n - 1.0));
    }
    if (nbt != nullptr && c == 0) nbt[0] += 1;
  }
};

// one thread per channel
__global__ void __launch_bounds__(256)
    bn_finalize_kernel(const float* __restrict__ x, BnFwdFin fin, int C, float* __restrict__ mean,
                       float* __restrict__ invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  fin.publish(c, fin.get(x, c), mean, invstd);
}

// Statistics from a producer's epilogue (pw_gemm256_kernel with stats): part
// float2 [C][P], the (mean, centred sum of squares) of P groups of up to 64
// values, group p holding min(gsz, S - (p % G) gsz) values (G = ceil(S / gsz);
// gsz 64 from the 256-row tiles, 32 from the 128-row streaming form).
// Four waves per channel: thread t combines groups t, t + 256, ... in order
// (Chan's update, fp64; 4 groups' loads in flight at a time), then a fixed xor
// tree per wave and the 4 wave results in wave order; thread 0 publishes mean /
// invstd and the running statistics through BnFwdFin::publish.
// Deterministic.  (One wave per channel walked ~40 dependent loads per lane:
// 17 us per launch at P = 2504.)
__device__ __forceinline__ void chan_merge(double& n, double& mu, double& m2, double nb, double mb,
                                           double qb) {
  const double nn = n + nb;
  if (nn > 0.0) {
    const double d = mb - mu;
    mu += d * nb / nn;
    m2 += qb + d * d * n * nb / nn;
  }
  n = nn;
}

__global__ void __launch_bounds__(256)
    bn_fin_parts_kernel(const float2* __restrict__ part, int P, int gsz, BnFwdFin fin,
                        float* __restrict__ mean, float* __restrict__ invstd) {
  const int c = blockIdx.x, t = threadIdx.x, l = t & 63, w = t >> 6;
  const int S = fin.S, G = (S + gsz - 1) / gsz;
  double n = 0.0, mu = 0.0, m2 = 0.0;
  const float2* __restrict__ pc = part + (size_t)c * P;
  int p = t;
  for (; p + 3 * 256 < P; p += 4 * 256) {
    float2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = pc[p + u * 256];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double nb = (double)min(gsz, S - ((p + u * 256) % G) * gsz);
      const double nn = n + nb, d = (double)v[u].x - mu;
      mu += d * nb / nn;
      m2 += (double)v[u].y + d * d * n * nb / nn;
      n = nn;
    }
  }
  for (; p < P; p += 256) {
    const float2 v = pc[p];
    const double nb = (double)min(gsz, S - (p % G) * gsz);
    const double nn = n + nb, d = (double)v.x - mu;
    mu += d * nb / nn;
    m2 += (double)v.y + d * d * n * nb / nn;
    n = nn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
    chan_merge(n, mu, m2, __shfl_xor(n, o, 64), __shfl_xor(mu, o, 64), __shfl_xor(m2, o, 64));
  __shared__ double wr[4][3];
  if (l == 0) {
    wr[w][0] = n;
    wr[w][1] = mu;
    wr[w][2] = m2;
  }
  __syncthreads();
  if (t == 0) {
    n = wr[0][0];
    mu = wr[0][1];
    m2 = wr[0][2];
    for (int k = 1; k < 4; ++k) chan_merge(n, mu, m2, wr[k][0], wr[k][1], wr[k][2]);
    const float var = clamp_var((float)(m2 / n));
    fin.publish(c, BnStat{(float)mu, rsqrtf(var + fin.eps), var, n}, mean, invstd);
  }
}

// The backward apply passes walk their blocks in REVERSE of the statistics
// pass's order (which reads the last batch element last): the rows read most
// recently are the ones still in the 256 MiB Infinity Cache (A/B on MI355X,
// tools/bn_ab.py: 158 -> 147 us at B8 C256 S20000, 123 -> 112 us at C128
// S32768; the forward apply, at 6.4 TB/s already, does not gain).
__device__ __forceinline__ unsigned bn_rev(unsigned i, unsigned n) { return rev_order(i, n); }

#ifndef PCFM_BN_APPLY_U
#define PCFM_BN_APPLY_U 4
#endif
#ifndef PCFM_BN_BWD_U
#define PCFM_BN_BWD_U 2
#endif
constexpr int kApplyU = PCFM_BN_APPLY_U;
constexpr int kBwdU = PCFM_BN_BWD_U;
inline int bn_apply_blocks(int s) { return ceil_div(s / 4, 256 * kApplyU); }
inline int bn_bwd_blocks(int s) { return ceil_div(s / 4, 256 * kBwdU); }

// z = act((x - mean) * invstd * gamma + beta), kApplyU float4 per thread;
// grid = (bn_apply_blocks(S), B * C).  Thread 0 derives the channel's
// statistics from the P partials once per block (LDS broadcast); block 0 of
// the first C rows publishes them.  What becomes of z is the sink:
//   Store : out = y [B][C][S], z written
//   RowSum: out = rowpart [B * C][gridDim.x], the block's sum of z -- the SE
//           pooling of PVConv's second BatchNorm, whose z is never written
enum class BnSink { Store, RowSum };
template <BnSink SINK>
__global__ void __launch_bounds__(256)
    bn_act_apply_kernel(const float* __restrict__ x, BnFwdFin fin, float* __restrict__ mean,
                        float* __restrict__ invstd, const float* __restrict__ gamma,
                        const float* __restrict__ beta, int C, int S4, float slope,
                        float* __restrict__ out) {
  __shared__ float st[2];
  const unsigned row = blockIdx.y, bx = blockIdx.x;
  const int c = (int)(row % C);
  if (threadIdx.x == 0) {
    if (fin.part != nullptr) {
      const BnStat s = fin.get(x, c);
      if (bx == 0 && row < (unsigned)C) fin.publish(c, s, mean, invstd);
      st[0] = s.m;
      st[1] = s.is;
    } else {  // statistics already final (bn_fin_parts_kernel)
      st[0] = mean[c];
      st[1] = invstd[c];
    }
  }
  const float g = gamma[c], bt = beta[c];
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x) + (size_t)row * S4;
  const int s0 = bx * 256 * kApplyU + threadIdx.x;
  float4 v[kApplyU];
#pragma unroll
  for (int u = 0; u < kApplyU; ++u)
    if (s0 + u * 256 < S4) v[u] = x4[s0 + u * 256];
  __syncthreads();
  const BnChan ch{st[0], st[1], g, bt, slope};
  float sum = 0.0f;
#pragma unroll
  for (int u = 0; u < kApplyU; ++u) {
    if (s0 + u * 256 >= S4) break;
    const float4 o = ch.z(v[u]);
    if constexpr (SINK == BnSink::Store)
      bn_out_store4(reinterpret_cast<float4*>(out) + (size_t)row * S4 + s0 + u * 256, o);
    else
      sum += (o.x + o.y) + (o.z + o.w);
  }
  if constexpr (SINK == BnSink::RowSum) {
    __shared__ float sh[8];
    float z = 0.0f;
    block_sum2(sum, z, sh);
    if (threadIdx.x == 0) out[(size_t)row * gridDim.x + bx] = sum;
  }
}

// grid = (C, P): part[c][p] = (sum g, sum g * xhat), g = dz * act'(bn(x)).
__global__ void __launch_bounds__(256)
    bn_bwd_stats_kernel(const float* __restrict__ dz, const float* __restrict__ x, BnParam bn,
                        int B, int C, int S, float* __restrict__ part) {
  __shared__ float sh[8];
  const int c = blockIdx.x, p = blockIdx.y, P = gridDim.y;
  const int S4 = S / 4;
  const BnChan ch = bn.at(c);
  const int PS = P / B, b = p / PS;
  int s0, s1;
  part_range(S4, p - b * PS, PS, s0, s1);
  const size_t r0 = ((size_t)b * C + c) * S4;
  const float4* const row[2] = {reinterpret_cast<const float4*>(x) + r0,
                                reinterpret_cast<const float4*>(dz) + r0};
  float sg = 0.0f, sgx = 0.0f;
  strip_reduce(row, s0, s1, [&](const float4(&v)[2]) {
    const float xv[4] = {v[0].x, v[0].y, v[0].z, v[0].w};
    const float dv[4] = {v[1].x, v[1].y, v[1].z, v[1].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g = ch.grad(xv[e], dv[e]);
      sg += g;
      sgx += g * ch.xhat(xv[e]);
    }
  });
  block_sum2_to(sg, sgx, sh, part + ((size_t)c * P + p) * 2);
}

// dx = gamma * invstd * (g - dbeta / n - xhat * dgamma / n), kBwdU float4
// per thread; grid (bn_bwd_blocks(S), B*C).  (dbeta, dgamma) = the ordered sum
// of the channel's P partials, derived by thread 0 of every block and written
// by block 0 of the first C rows.  With rowpart: the block's sum of dx ->
// rowpart[row][block] (producer bias grad).
__global__ void __launch_bounds__(256)
    bn_bwd_apply_kernel(const float* __restrict__ dz, const float* __restrict__ x, BnParam bn,
                        const float* __restrict__ part, int P, float* __restrict__ dgamma,
                        float* __restrict__ dbeta, int C, int S4, float inv_n,
                        float* __restrict__ dx, float* __restrict__ rowpart) {
  __shared__ float sh[8];
  __shared__ float st[2];
  const unsigned row = bn_rev(blockIdx.y, gridDim.y), bx = bn_rev(blockIdx.x, gridDim.x);
  const int c = (int)(row % C);
  if (threadIdx.x == 0) {
    float sg, sgx;
    sum_parts2(part + (size_t)c * P * 2, P, sg, sgx);
    if (bx == 0 && row < (unsigned)C) {
      dbeta[c] = sg;
      dgamma[c] = sgx;
    }
    st[0] = sg;
    st[1] = sgx;
  }
  const BnChan ch = bn.at(c);
  const size_t r0 = (size_t)row * S4;
  const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x) + r0;
  const float4* __restrict__ d4 = reinterpret_cast<const float4*>(dz) + r0;
  float4* __restrict__ o4 = reinterpret_cast<float4*>(dx) + r0;
  const int s0 = bx * 256 * kBwdU + threadIdx.x;
  float4 v[kBwdU], d[kBwdU];
#pragma unroll
  for (int u = 0; u < kBwdU; ++u)
    if (s0 + u * 256 < S4) {
      v[u] = x4[s0 + u * 256];
      d[u] = d4[s0 + u * 256];
    }
  __syncthreads();
  const float mg = st[0] * inv_n, mgx = st[1] * inv_n;
  float tsum = 0.0f;
#pragma unroll
  for (int u = 0; u < kBwdU; ++u) {
    if (s0 + u * 256 >= S4) break;
    const float4 o = make_float4(ch.dx(v[u].x, d[u].x, mg, mgx), ch.dx(v[u].y, d[u].y, mg, mgx),
                                 ch.dx(v[u].z, d[u].z, mg, mgx), ch.dx(v[u].w, d[u].w, mg, mgx));
    bn_out_store4(o4 + s0 + u * 256, o);
    tsum += (o.x + o.y) + (o.z + o.w);
  }
  if (rowpart != nullptr) {  // block-uniform branch: every thread takes part
    float z = 0.0f;
    block_sum2(tsum, z, sh);
    if (threadIdx.x == 0) rowpart[(size_t)row * gridDim.x + bx] = tsum;
  }
}

// dbias[c] = sum over (b, k) of rowpart[(b * C + c) * nch + k]: one wave per
// channel, lane-strided in a fixed order, then a fixed xor tree (deterministic)
__global__ void __launch_bounds__(256)
    bn_bias_finalize_kernel(const float* __restrict__ rowpart, int B, int C, int nch,
                            float* __restrict__ dbias) {
  const int c = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (c >= C) return;  // wave-uniform
  float s = 0.0f;
  const int tot = B * nch;
  for (int e = lane; e < tot; e += 64) {
    const int b = e / nch, k = e - b * nch;
    s += rowpart[((size_t)b * C + c) * nch + k];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) dbias[c] = s;
}

// dbias[c] = sum over (b, k) of rowpart[(b * C + c) * nch + k] for long rows:
// one block per channel, thread-strided in a fixed order, then a fixed tree.
__global__ void __launch_bounds__(256)
    bn_bias_finalize_block_kernel(const float* __restrict__ rowpart, int B, int C, int nch,
                                  float* __restrict__ dbias) {
  __shared__ float sh[8];
  const int c = blockIdx.x;
  float s = 0.0f;
  for (int bb = 0; bb < B; ++bb) {
    const float* __restrict__ rp = rowpart + ((size_t)bb * C + c) * nch;
    for (int k = threadIdx.x; k < nch; k += 256) s += rp[k];
  }
  float z = 0.0f;
  block_sum2(s, z, sh);
  if (threadIdx.x == 0) dbias[c] = s;
}

// ---------------------------------------------------------------------------
// The split forms: a voxel convolution's input / its backward's operand is
// written directly as the channels-last bf16 hi/lo split the convolution reads
// (conv3_split_cl_kernel), never as fp32 [B][C][V].
// grid = (S / 64, C / 64, B), 256 threads; a 64 x 64 LDS tile.
// ---------------------------------------------------------------------------
typedef __bf16 bn_bf16x2 __attribute__((ext_vector_type(2)));

// A 64 (channel) x 64 (voxel) fp32 LDS tile -> channels-last bf16 hi / lo
// rows [b][v][c] interleaved per 32 channels (conv3_split_cl_kernel's layout,
// split_off, and rounding), 256 threads:
// thread t writes 16 channels of voxel t / 4.
__device__ __forceinline__ void tile_store_split(const float (&tile)[64][65], int b, int C, int S,
                                                 int v0, int c0, int t, uint16_t* __restrict__ h,
                                                 uint16_t* __restrict__ l) {
  const int v = t >> 2, cg = (t & 3) * 16;
  const size_t o = split_off((size_t)b * S + v0 + v, c0 + cg, C);  // l = h + kSplitLo
  uint32_t* h32 = reinterpret_cast<uint32_t*>(h + o);
  uint32_t* l32 = reinterpret_cast<uint32_t*>(l + o);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float f0 = tile[cg + 2 * q][v], f1 = tile[cg + 2 * q + 1][v];
    bn_bf16x2 hi, lo;
    hi.x = (__bf16)f0;
    hi.y = (__bf16)f1;
    lo.x = (__bf16)(f0 - (float)hi.x);
    lo.y = (__bf16)(f1 - (float)hi.y);
    h32[q] = __builtin_bit_cast(uint32_t, hi);
    l32[q] = __builtin_bit_cast(uint32_t, lo);
  }
}

// rowpart[(b * C + c) * (S / 64) + bx] = sum of the tile's channel c over its
// 64 voxels (fixed order: 16 sequential per thread, then a 4-lane xor tree):
// the producer's bias gradient, summed over (b, bx) by
// bn_bias_finalize_block_kernel.
__device__ __forceinline__ void tile_rowsum(const float (&tile)[64][65], int b, int C, int S,
                                            int c0, unsigned bx, int t,
                                            float* __restrict__ rowpart) {
  const int c = t >> 2, vq = (t & 3) * 16;
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < 16; ++q) sum += tile[c][vq + q];
  sum += __shfl_xor(sum, 1, 64);
  sum += __shfl_xor(sum, 2, 64);
  if ((t & 3) == 0) rowpart[((size_t)b * C + c0 + c) * (S / 64) + bx] = sum;
}

// act(bn(x)) written as the next convolution's split input (the fp32
// activation is never materialised)
__global__ void __launch_bounds__(256)
    bn_act_apply_split_kernel(const float* __restrict__ x, BnFwdFin fin,
                              float* __restrict__ mean, float* __restrict__ invstd,
                              const float* __restrict__ gamma,
                              const float* __restrict__ beta, int C, int S, float slope,
                              uint16_t* __restrict__ yh, uint16_t* __restrict__ yl) {
  __shared__ float tile[64][65];
  __shared__ float st_m[64], st_is[64];
  const unsigned bx = blockIdx.x;
  const int v0 = bx * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (t < 64) {
    const BnStat s = fin.get(x, c0 + t);
    st_m[t] = s.m;
    st_is[t] = s.is;
    if (bx == 0 && b == 0) fin.publish(c0 + t, s, mean, invstd);
  }
  __syncthreads();
  const size_t rbase = ((size_t)b * C + c0) * S + v0;
  float xv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) xv[i] = x[rbase + (size_t)(4 * i + w) * S + lane];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int cl = 4 * i + w;
    tile[cl][lane] = BnChan{st_m[cl], st_is[cl], gamma[c0 + cl], beta[c0 + cl], slope}.z(xv[i]);
  }
  __syncthreads();
  tile_store_split(tile, b, C, S, v0, c0, t, yh, yl);
}

// BN backward apply for a voxel convolution's output; with rowpart also the
// tile's row sums of dx (tile_rowsum).  What differs between the two forms is
// the policy SUMS:
//   stage(stg, t, c, b, C, sg, sgx)  thread t < 64 obtains channel c's
//       (sum g, sum g xhat), leaves them in stg.g[t] / stg.gx[t] with whatever
//       else dz needs, and returns them for block (0, 0) to write as d beta /
//       d gamma
//   dz(stg, cl, v)  the gradient entering the BatchNorm at channel c0 + cl from
//       the loaded value v
// (The BatchNorm operands are __restrict__ pointers, not a BnParam: as struct
// members the compiler keeps their loads behind the tile stores and the SE form
// needs 89 registers, 5 waves per SIMD, against 58 and 8.)
// BnPartSums: dz is the loaded tensor, the sums are the ordered sum of the P
// partials [C][P] of bn_bwd_stats_kernel.
struct BnPartSums {
  const float* part;
  int P;
  struct Staged {
    float g[64], gx[64];
  };
  __device__ __forceinline__ void stage(Staged& stg, int t, int c, int, int, float& sg,
                                        float& sgx) const {
    sum_parts2(part + (size_t)c * P * 2, P, sg, sgx);
    stg.g[t] = sg;
    stg.gx[t] = sgx;
  }
  __device__ __forceinline__ float dz(const Staged&, int, float v) const { return v; }
};

template <class SUMS>
__global__ void __launch_bounds__(256)
    bn_bwd_apply_split_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                              const float* __restrict__ mean, const float* __restrict__ invstd,
                              const float* __restrict__ gamma, const float* __restrict__ beta,
                              float slope, SUMS sums, float* __restrict__ dgamma,
                              float* __restrict__ dbeta, int C, int S, float inv_n,
                              uint16_t* __restrict__ dxh, uint16_t* __restrict__ dxl,
                              float* __restrict__ rowpart) {
  __shared__ float tile[64][65];
  __shared__ typename SUMS::Staged stg;
  const unsigned bx = bn_rev(blockIdx.x, gridDim.x);
  const int v0 = bx * 64, c0 = blockIdx.y * 64, b = bn_rev(blockIdx.z, gridDim.z);
  const int t = threadIdx.x, w = t >> 6, lane = t & 63;
  if (t < 64) {
    float sg, sgx;
    sums.stage(stg, t, c0 + t, b, C, sg, sgx);
    if (bx == 0 && b == 0) {
      dbeta[c0 + t] = sg;
      dgamma[c0 + t] = sgx;
    }
  }
  __syncthreads();
  const size_t rbase = ((size_t)b * C + c0) * S + v0;
  float xv[16], dv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const size_t o = rbase + (size_t)(4 * i + w) * S + lane;
    xv[i] = x[o];
    dv[i] = dz[o];
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int cl = 4 * i + w;
    const int c = c0 + cl;
    const BnChan ch{mean[c], invstd[c], gamma[c], beta[c], slope};
    const float mg = stg.g[cl] * inv_n, mgx = stg.gx[cl] * inv_n;
    tile[cl][lane] = ch.dx(xv[i], sums.dz(stg, cl, dv[i]), mg, mgx);
  }
  __syncthreads();
  tile_store_split(tile, b, C, S, v0, c0, t, dxh, dxl);
  if (rowpart != nullptr) tile_rowsum(tile, b, C, S, c0, bx, t, rowpart);
}

// ---------------------------------------------------------------------------
// PVConv's second voxel BatchNorm + LeakyReLU fused with SE3d and the
// devoxelization (pvconv.py:20-39, se.py:6-17): z = act(bn(x)) is never
// written.  Forward: the batch statistics, then ONE pass computing the SE
// pooling m[b][c] = mean_v z (bn_act_apply_kernel<RowSum>); the devoxelization
// gather applies BnChan::z to the rows while staging them (rows.hpp).
// Backward from g = devox_bwd(dout): dz = s[b][c] g + dmv[b][c] (SE's scale and
// the pooling's gradient dm / V), so every sum BatchNorm's backward needs is
// linear in (s, dmv) -- per (b, c) row, with a = act'(bn(x)), xh = xhat:
//   ds = sum z g,  A = sum a g,  N = sum a,  AX = sum a g xh,  NX = sum a xh
//   sum a dz = s A + dmv N,   sum a dz xh = s AX + dmv NX
// ONE pass over (g, x) gives all five (bn_se_bwd_stats_kernel); the SE MLP's
// backward turns ds into dmv; the apply pass writes dx as the conv's split
// operand (bn_bwd_apply_split_kernel<BnSeSums>).  The SE rows_dot passes, the
// rows_affine pass over g and the separate backward statistics pass are gone.
// ---------------------------------------------------------------------------

// one thread per row: out[row] = scale * sum of its nblk partials, in order
__global__ void __launch_bounds__(256)
    rowpart_sum_kernel(const float* __restrict__ rowpart, int rows, int nblk, float scale,
                       float* __restrict__ out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* __restrict__ p = rowpart + (size_t)r * nblk;
  float s = 0.0f;
  for (int k = 0; k < nblk; ++k) s += p[k];
  out[r] = s * scale;
}

// grid (PS, B * C), PS = bn_parts(B) / B blocks per row:
// part[(row * PS + ps) * 5 + k] = the five sums above over the block's range.
constexpr int kSeSums = 5;
__global__ void __launch_bounds__(256)
    bn_se_bwd_stats_kernel(const float* __restrict__ g, const float* __restrict__ x, BnParam bn,
                           int C, int S, float* __restrict__ part) {
  __shared__ float sh[8 * kSeSums];
  const unsigned r = blockIdx.y;
  const int c = (int)(r % C), ps = blockIdx.x, PS = gridDim.x;
  const int S4 = S / 4;
  int s0, s1;
  part_range(S4, ps, PS, s0, s1);
  const BnChan ch = bn.at(c);
  const float4* const row[2] = {reinterpret_cast<const float4*>(x) + (size_t)r * S4,
                                reinterpret_cast<const float4*>(g) + (size_t)r * S4};
  float acc[kSeSums] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // ds, A, N, AX, NX
  strip_reduce(row, s0, s1, [&](const float4(&v)[2]) {
    const float xv[4] = {v[0].x, v[0].y, v[0].z, v[0].w};
    const float dv[4] = {v[1].x, v[1].y, v[1].z, v[1].w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float xh = ch.xhat(xv[e]);
      const float t = ch.pre(xv[e]);
      const float a = BnChan::dact(t, ch.slope);
      const float z = BnChan::act(t, ch.slope);
      const float ag = BnChan::gate(t, ch.slope, dv[e]);  // a * g at every finite g
      acc[0] = __builtin_fmaf(z, dv[e], acc[0]);
      acc[1] += ag;
      acc[2] += a;
      acc[3] = __builtin_fmaf(ag, xh, acc[3]);
      acc[4] = __builtin_fmaf(a, xh, acc[4]);
    }
  });
  // block sum of the five values: xor tree per wave, then the 4 waves in order
#pragma unroll
  for (int k = 0; k < kSeSums; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, 64);
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < kSeSums; ++k) sh[w * kSeSums + k] = acc[k];
  __syncthreads();
  if (threadIdx.x < kSeSums) {
    const int k = threadIdx.x;
    part[((size_t)r * PS + ps) * kSeSums + k] =
        ((sh[k] + sh[kSeSums + k]) + sh[2 * kSeSums + k]) + sh[3 * kSeSums + k];
  }
}

// one thread per (row, sum): rowstats[k][row] = sum over the row's PS parts, in order
__global__ void __launch_bounds__(256)
    bn_se_rowstats_kernel(const float* __restrict__ part, int rows, int PS,
                          float* __restrict__ rowstats) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * kSeSums) return;
  const int row = i / kSeSums, k = i - row * kSeSums;
  const float* __restrict__ p = part + (size_t)row * PS * kSeSums + k;
  float s = 0.0f;
  for (int q = 0; q < PS; ++q) s += p[(size_t)q * kSeSums];
  rowstats[(size_t)k * rows + row] = s;
}

// bn_bwd_apply_split_kernel's sums for dz = s[b][c] g + dmv[b][c]: from
// rowstats [5][B][C], summed over b in order; the row's (s, dmv) are staged too.
struct BnSeSums {
  const float* se_s;      // [B][C]
  const float* dmv;       // [B][C]
  const float* rowstats;  // [5][B][C]
  int B;
  struct Staged {
    float g[64], gx[64], s[64], t[64];
  };
  __device__ __forceinline__ void stage(Staged& stg, int t, int c, int b, int C, float& sg,
                                        float& sgx) const {
    const size_t BC = (size_t)B * C;
    sg = 0.0f;
    sgx = 0.0f;
    for (int bb = 0; bb < B; ++bb) {
      const size_t r = (size_t)bb * C + c;
      const float sv = se_s[r], tv = dmv[r];
      sg += __builtin_fmaf(sv, rowstats[BC + r], tv * rowstats[2 * BC + r]);
      sgx += __builtin_fmaf(sv, rowstats[3 * BC + r], tv * rowstats[4 * BC + r]);
    }
    stg.g[t] = sg;
    stg.gx[t] = sgx;
    stg.s[t] = se_s[(size_t)b * C + c];
    stg.t[t] = dmv[(size_t)b * C + c];
  }
  __device__ __forceinline__ float dz(const Staged& stg, int cl, float v) const {
    return __builtin_fmaf(stg.s[cl], v, stg.t[cl]);  // rows_affine's expression
  }
};

// ---------------------------------------------------------------------------
// GroupNorm + FiLM + residual of the hybrid backbone's PV blocks
// (reference models.py:322-346 _FiLM1d with GroupNorm, :349-368 _PVBlock):
//   out = x + (GN(x) * (1 + gamma[b]) + beta[b])
//   GN(x)[b, c, n] = (x - mean[b, g]) * rstd[b, g] * w[c] + bias[c],  g = c / (C / G)
// evaluated as torch does: y = x * a + s with a = rstd * w, s = bias - mean * a,
// then y * (1 + gamma) + beta, then + x.
// Backward with A2[b, c] = sum_n dout, A3[b, c] = sum_n dout * xhat:
//   d beta = A2, d gamma = w A3 + bias A2, d w = sum_b (1+gamma) A3,
//   d bias = sum_b (1+gamma) A2, and per group
//   dx = dout + rstd (dout (1+gamma) w - mean_g(dy w) - xhat mean_g(dy w xhat)).
//
// IN forms: GroupNorm over the activation of a SharedMLP layer given as its
// pre-BatchNorm tensor y (the PV block's post layer, models.py:349-368): the
// GroupNorm reads z = BnChan::z(y), the function the BatchNorm apply pass
// calls, so z is the activation it no longer writes.
// ---------------------------------------------------------------------------
constexpr int kGnParts = 4;  // blocks per (b, group) row set / per (b, c) row

// fwd stats: grid (G * kGnParts, B); part[(b*G + g)*P + p] = (sum (x-K), sum (x-K)^2)
// IN: over z = act(bn(x)), K = z of the group's first element
template <bool IN>
__global__ void __launch_bounds__(256)
    gn_stats_kernel(const float* __restrict__ x, int C, int N, int G, float* __restrict__ part,
                    BnParam bn) {
  __shared__ float sh[8];
  const int b = blockIdx.y, g = blockIdx.x / kGnParts, p = blockIdx.x % kGnParts;
  const int cpg = C / G, N4 = N / 4;
  const float* base = x + ((size_t)b * C + (size_t)g * cpg) * N;  // cpg rows of N, contiguous
  const float K = IN ? bn.at(g * cpg).z(base[0]) : base[0];
  const int tot = cpg * N4, chunk = (tot + kGnParts - 1) / kGnParts;
  const int f0 = min(tot, p * chunk), f1 = min(tot, f0 + chunk);
  const float4* x4 = reinterpret_cast<const float4*>(base);
  float s = 0.0f, q = 0.0f;
  // IN: the thread's current channel (its stride, 256 float4s, is below a row's N4)
  int f = f0 + threadIdx.x, bnd = 0;
  BnChan tc{};
  if (IN && f < f1) {
    const int cl = f / N4;
    bnd = (cl + 1) * N4;
    tc = bn.at(g * cpg + cl);
  }
  for (; f < f1; f += 256) {
    float4 v = x4[f];
    if (IN) {
      if (f >= bnd) {
        const int cl = f / N4;
        bnd = (cl + 1) * N4;
        tc = bn.at(g * cpg + cl);
      }
      v = tc.z(v);
    }
    add_shifted(v, K, s, q);
  }
  block_sum2_to(s, q, sh, part + (((size_t)b * G + g) * kGnParts + p) * 2);
}

// one thread per (b, c): group stats -> a = rstd*w, s = bias - mean*a, g1 = 1 + gamma
__global__ void __launch_bounds__(256)
    gn_finalize_kernel(const float* __restrict__ part, const float* __restrict__ x,
                       const float* __restrict__ w, const float* __restrict__ bias,
                       const float* __restrict__ gamma, int B, int C, int N, int G, float eps,
                       float* __restrict__ mean_o, float* __restrict__ rstd_o,
                       float* __restrict__ coef, BnParam bn) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * C) return;
  const int b = i / C, c = i - b * C, cpg = C / G, g = c / cpg;
  float s = 0.0f, q = 0.0f;
  for (int p = 0; p < kGnParts; ++p) {
    s += part[(((size_t)b * G + g) * kGnParts + p) * 2];
    q += part[(((size_t)b * G + g) * kGnParts + p) * 2 + 1];
  }
  float K = x[((size_t)b * C + (size_t)g * cpg) * N];
  if (bn.mean != nullptr) K = bn.at(g * cpg).z(K);
  const BnStat st = stat_of_shifted(s, q, (double)cpg * N, K, eps);
  const float mean = st.m, rstd = st.is;
  if (c % cpg == 0) {
    mean_o[b * G + g] = mean;
    rstd_o[b * G + g] = rstd;
  }
  const float a = rstd * w[c];
  coef[3 * (size_t)i] = a;
  coef[3 * (size_t)i + 1] = bias[c] - mean * a;
  coef[3 * (size_t)i + 2] = gamma != nullptr ? 1.0f + gamma[i] : 1.0f;
}

// torch's SiLU x / (1 + exp(-x)) and its derivative s (1 + x (1 - s))
__device__ __forceinline__ float gn_silu(float x) { return x / (1.0f + expf(-x)); }
__device__ __forceinline__ float gn_dsilu(float x) {
  const float sg = 1.0f / (1.0f + expf(-x));
  return sg * (1.0f + x * (1.0f - sg));
}

// ContextNet's head: out = SiLU(GN(x)) = SiLU(x * a + s); grid (ceil(N4 / 256), B * C)
__global__ void __launch_bounds__(256)
    gn_silu_apply_kernel(const float* __restrict__ x, const float* __restrict__ coef, int N4,
                         float* __restrict__ out) {
  const int n4 = blockIdx.x * 256 + threadIdx.x;
  if (n4 >= N4) return;
  const int row = blockIdx.y;
  const float a = coef[3 * (size_t)row], sh = coef[3 * (size_t)row + 1];
  const size_t i = (size_t)row * N4 + n4;
  const float4 v = reinterpret_cast<const float4*>(x)[i];
  float4 o;
  o.x = gn_silu(__builtin_fmaf(v.x, a, sh));
  o.y = gn_silu(__builtin_fmaf(v.y, a, sh));
  o.z = gn_silu(__builtin_fmaf(v.z, a, sh));
  o.w = gn_silu(__builtin_fmaf(v.w, a, sh));
  reinterpret_cast<float4*>(out)[i] = o;
}

// out = x + ((x * a + s) * g1 + beta); grid (ceil(N4 / 256), B * C)
// IN: x -> z = act(bn(x)) first (the residual is z too)
template <bool IN>
__global__ void __launch_bounds__(256)
    gn_film_apply_kernel(const float* __restrict__ x, const float* __restrict__ coef,
                         const float* __restrict__ beta, int N4, float* __restrict__ out, int C,
                         BnParam bn) {
  const int n4 = blockIdx.x * 256 + threadIdx.x;
  if (n4 >= N4) return;
  const int row = blockIdx.y;
  const float a = coef[3 * (size_t)row], s = coef[3 * (size_t)row + 1];
  const float g1 = coef[3 * (size_t)row + 2], bt = beta[row];
  const size_t i = (size_t)row * N4 + n4;
  float4 v = reinterpret_cast<const float4*>(x)[i];
  if (IN) v = bn.at(row % C).z(v);
  float4 o;
  o.x = v.x + (__builtin_fmaf(v.x, a, s) * g1 + bt);
  o.y = v.y + (__builtin_fmaf(v.y, a, s) * g1 + bt);
  o.z = v.z + (__builtin_fmaf(v.z, a, s) * g1 + bt);
  o.w = v.w + (__builtin_fmaf(v.w, a, s) * g1 + bt);
  gn_out_store4(reinterpret_cast<float4*>(out) + i, o);
}

// bwd row sums: grid (kGnParts, B * C); part[row * P + p] = (sum dout, sum dout * xhat)
// ACT (GN + SiLU): the gradient entering GN is dout * SiLU'(x * a + s), recomputed
// IN: over z = act(bn(x))
template <bool ACT, bool IN>
__global__ void __launch_bounds__(256)
    gn_bwd_stats_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                        const float* __restrict__ mean, const float* __restrict__ rstd,
                        const float* __restrict__ w, const float* __restrict__ bias, int C,
                        int N, int G, float* __restrict__ part, BnParam bn) {
  __shared__ float sh[8];
  const int row = blockIdx.y, p = blockIdx.x;
  const int b = row / C, c = row - b * C, g = c / (C / G);
  const float m = mean[b * G + g], rs = rstd[b * G + g];
  const float ca = ACT ? rs * w[c] : 0.0f, cs = ACT ? bias[c] - m * ca : 0.0f;
  const int N4 = N / 4, chunk = (N4 + kGnParts - 1) / kGnParts;
  const int f0 = min(N4, p * chunk), f1 = min(N4, f0 + chunk);
  const float4* x4 = reinterpret_cast<const float4*>(x) + (size_t)row * N4;
  const float4* d4 = reinterpret_cast<const float4*>(dout) + (size_t)row * N4;
  float a2 = 0.0f, a3 = 0.0f;
  BnChan tc{};
  if (IN) tc = bn.at(c);
  for (int f = f0 + threadIdx.x; f < f1; f += 256) {
    float4 v = x4[f];
    if (IN) v = tc.z(v);
    float4 d = d4[f];
    if (ACT) {
      d.x *= gn_dsilu(__builtin_fmaf(v.x, ca, cs));
      d.y *= gn_dsilu(__builtin_fmaf(v.y, ca, cs));
      d.z *= gn_dsilu(__builtin_fmaf(v.z, ca, cs));
      d.w *= gn_dsilu(__builtin_fmaf(v.w, ca, cs));
    }
    a2 += (d.x + d.y) + (d.z + d.w);
    a3 += (d.x * ((v.x - m) * rs) + d.y * ((v.y - m) * rs)) +
          (d.z * ((v.z - m) * rs) + d.w * ((v.w - m) * rs));
  }
  block_sum2_to(a2, a3, sh, part + ((size_t)row * kGnParts + p) * 2);
}

// one block, C threads (C <= 1024): per batch element the group coefficients
// k1 = mean_g(dy w), k2 = mean_g(dy w xhat) -> kc[b][c] = (rstd*g1*w, rstd*k1, rstd*k2)
// and d gamma / d beta [b][c]; summed over b: d w, d bias [c].
__global__ void __launch_bounds__(1024)
    gn_bwd_finalize_kernel(const float* __restrict__ part, const float* __restrict__ w,
                           const float* __restrict__ bias, const float* __restrict__ gamma,
                           const float* __restrict__ rstd, int B, int C, int N, int G,
                           float* __restrict__ kc, float* __restrict__ dgamma,
                           float* __restrict__ dbeta, float* __restrict__ dw,
                           float* __restrict__ dbias) {
  __shared__ float s1[1024], s2[1024];
  const int c = threadIdx.x, cpg = C / G;
  float dws = 0.0f, dbs = 0.0f;
  for (int b = 0; b < B; ++b) {
    float a2 = 0.0f, a3 = 0.0f, g1 = 0.0f, t1 = 0.0f, t2 = 0.0f;
    if (c < C) {
      const size_t row = (size_t)b * C + c;
      for (int p = 0; p < kGnParts; ++p) {
        a2 += part[(row * kGnParts + p) * 2];
        a3 += part[(row * kGnParts + p) * 2 + 1];
      }
      g1 = gamma != nullptr ? 1.0f + gamma[row] : 1.0f;
      if (dbeta != nullptr) dbeta[row] = a2;
      if (dgamma != nullptr) dgamma[row] = w[c] * a3 + bias[c] * a2;
      dws += g1 * a3;
      dbs += g1 * a2;
      t1 = w[c] * g1 * a2;  // sum_n dy w over this channel
      t2 = w[c] * g1 * a3;  // sum_n dy w xhat
    }
    s1[c] = t1;
    s2[c] = t2;
    __syncthreads();
    if (c < C) {
      const int g0 = (c / cpg) * cpg;
      float k1 = 0.0f, k2 = 0.0f;
      for (int j = 0; j < cpg; ++j) {
        k1 += s1[g0 + j];
        k2 += s2[g0 + j];
      }
      const float inv_d = (float)(1.0 / ((double)cpg * N));
      const float rs = rstd[b * G + c / cpg];
      const size_t row = (size_t)b * C + c;
      kc[3 * row] = rs * g1 * w[c];
      kc[3 * row + 1] = rs * k1 * inv_d;
      kc[3 * row + 2] = rs * k2 * inv_d;
    }
    __syncthreads();
  }
  if (c < C) {
    dw[c] = dws;
    dbias[c] = dbs;
  }
}

// dx = dout + dout * kc0 - kc1 - xhat * kc2; grid (ceil(N4 / 256), B * C)
// ACT: dx = dy * kc0 - kc1 - xhat * kc2 with dy = dout * SiLU'(x * a + s) (no residual)
// IN (GroupNorm over z = act(bn(x)), the residual z too): dx is dL/dz, and the
// block's BatchNorm backward sums of g = BnChan::grad(x, dx) -- sum g and
// sum g * xhat_bn, bn_bwd_stats_kernel's terms -- go to bnpart[c][b * nbx + bx]
// (float2; nbx = gridDim.x): the separate BatchNorm statistics pass over
// (dL/dz, x) is not needed.
template <bool ACT, bool IN>
__global__ void __launch_bounds__(256)
    gn_film_bwd_apply_kernel(const float* __restrict__ dout, const float* __restrict__ x,
                             const float* __restrict__ mean, const float* __restrict__ rstd,
                             const float* __restrict__ kc, const float* __restrict__ w,
                             const float* __restrict__ bias, int C, int G, int N4,
                             float* __restrict__ dx, BnParam bn, float* __restrict__ bnpart) {
  // reverse of the statistics pass's row order (Infinity-cache reuse, as BN)
  const unsigned bx = bn_rev(blockIdx.x, gridDim.x);
  const int n4 = bx * 256 + threadIdx.x;
  if (!IN && n4 >= N4) return;  // IN: every thread reaches the block sum
  const int row = bn_rev(blockIdx.y, gridDim.y);
  const int b = row / C, c = row - b * C, g = c / (C / G);
  const float m = mean[b * G + g], rs = rstd[b * G + g];
  const float k0 = kc[3 * (size_t)row], k1 = kc[3 * (size_t)row + 1], k2 = kc[3 * (size_t)row + 2];
  const size_t i = (size_t)row * N4 + n4;
  float sg = 0.0f, sgx = 0.0f;
  if (n4 < N4) {
    const float4 y = reinterpret_cast<const float4*>(x)[i];
    float4 v = y;
    BnChan tc{};
    if (IN) {
      tc = bn.at(c);
      v = tc.z(y);
    }
    const float4 d = reinterpret_cast<const float4*>(dout)[i];
    float4 o;
    if (ACT) {
      const float ca = rs * w[c], cs = bias[c] - m * ca;
      const float dy0 = d.x * gn_dsilu(__builtin_fmaf(v.x, ca, cs));
      const float dy1 = d.y * gn_dsilu(__builtin_fmaf(v.y, ca, cs));
      const float dy2 = d.z * gn_dsilu(__builtin_fmaf(v.z, ca, cs));
      const float dy3 = d.w * gn_dsilu(__builtin_fmaf(v.w, ca, cs));
      o.x = (dy0 * k0 - k1) - ((v.x - m) * rs) * k2;
      o.y = (dy1 * k0 - k1) - ((v.y - m) * rs) * k2;
      o.z = (dy2 * k0 - k1) - ((v.z - m) * rs) * k2;
      o.w = (dy3 * k0 - k1) - ((v.w - m) * rs) * k2;
    } else {
      o.x = d.x + ((d.x * k0 - k1) - ((v.x - m) * rs) * k2);
      o.y = d.y + ((d.y * k0 - k1) - ((v.y - m) * rs) * k2);
      o.z = d.z + ((d.z * k0 - k1) - ((v.z - m) * rs) * k2);
      o.w = d.w + ((d.w * k0 - k1) - ((v.w - m) * rs) * k2);
    }
    gn_out_store4(reinterpret_cast<float4*>(dx) + i, o);
    if (IN) {
      const float yv[4] = {y.x, y.y, y.z, y.w}, ov[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = tc.grad(yv[e], ov[e]);
        sg += gg;
        sgx += gg * tc.xhat(yv[e]);
      }
    }
  }
  if (IN) {
    __shared__ float sh[8];
    const int nbx = (int)gridDim.x, P = (int)(gridDim.y / C) * nbx;
    block_sum2_to(sg, sgx, sh, bnpart + ((size_t)c * P + (size_t)b * nbx + bx) * 2);
  }
}

bool gn_ok(int b, int c, int n, int g) {
  return b > 0 && c > 0 && c <= 1024 && g > 0 && c % g == 0 && n > 0 && n % 4 == 0 &&
         (long long)b * c < 65536 && (long long)(c / g) * n / 4 < (1LL << 31);
}

// group size of a producer's epilogue statistics: P = b * ceil(s / gsz) groups
// per channel, gsz 64 (256-row pointwise tiles) or 32 (128-row streaming form);
// 0 when P matches neither
int parts_gsz(int P, int b, int s) {
  if (P == b * ceil_div(s, 64)) return 64;
  if (P == b * ceil_div(s, 32)) return 32;
  return 0;
}

bool bn_ok(int b, int c, int s) {
  return b > 0 && c > 0 && s > 0 && s % 4 == 0 && (long long)b * c < 65536 &&
         (long long)b * c * s < (1LL << 40);
}

// ---------------------------------------------------------------------------
// Host-side pieces the entries are assembled from.  `what` is the public
// entry's name without its pcfm_ prefix: every message names the entry called.
// ---------------------------------------------------------------------------
#define BN_TRY(expr)               \
  do {                             \
    if (int e_ = (expr)) return e_; \
  } while (0)

enum class BnForm { Contig, Split };  // Split: 64 x 64 tiles, c and s multiples of 64

int bn_check(const char* what, int b, int c, int s, BnForm form, size_t ws_bytes, size_t need) {
  if (form == BnForm::Split)
    PCFM_CHECK_ARG(bn_ok(b, c, s) && c % 64 == 0 && s % 64 == 0,
                   "%s: bad shape b=%d c=%d s=%d (c, s multiples of 64)", what, b, c, s);
  else
    PCFM_CHECK_ARG(bn_ok(b, c, s), "%s: bad shape b=%d c=%d s=%d (s %% 4 == 0 needed)", what, b,
                   c, s);
  PCFM_CHECK_ARG(ws_bytes >= need, "%s: workspace too small", what);
  return PCFM_OK;
}

int bn_check_running(const char* what, const float* running_mean, const float* running_var) {
  PCFM_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr),
                 "%s: running_mean and running_var must both be given or both NULL", what);
  return PCFM_OK;
}

// the forward statistics pass into part [c][bn_parts(b)] -> the BnFwdFin that
// finalizes from those partials
BnFwdFin bn_fwd_stats(const float* x, int b, int c, int s, float eps, float momentum,
                      float* running_mean, float* running_var, long long* nbt, float* part,
                      hipStream_t st) {
  hipLaunchKernelGGL(bn_stats_kernel, dim3(c, bn_parts(b)), dim3(256), 0, st, x, b, c, s, part);
  return BnFwdFin{part, b, s, bn_parts(b), eps, momentum, running_mean, running_var, nbt};
}

// the finalize of a producer's epilogue statistics (part float2 [c][P], see
// bn_fin_parts_kernel) into mean / invstd; the BnFwdFin it returns says so
int bn_fwd_stats_parts(const char* what, const float* part, int P, int b, int c, int s, float eps,
                       float momentum, float* running_mean, float* running_var, long long* nbt,
                       float* mean, float* invstd, hipStream_t st, BnFwdFin* fin) {
  const int gsz = parts_gsz(P, b, s);
  PCFM_CHECK_ARG(part != nullptr && gsz > 0,
                 "%s: need b * ceil(s / 64) = %d or b * ceil(s / 32) = %d groups per channel, "
                 "got %d", what, b * ceil_div(s, 64), b * ceil_div(s, 32), P);
  *fin = BnFwdFin{nullptr, b, s, 0, eps, momentum, running_mean, running_var, nbt};
  hipLaunchKernelGGL(bn_fin_parts_kernel, dim3(c), dim3(256), 0, st,
                     reinterpret_cast<const float2*>(part), P, gsz, *fin, mean, invstd);
  return PCFM_OK;
}

void bn_fwd_apply(const float* x, const BnFwdFin& fin, float* mean, float* invstd,
                  const float* gamma, const float* beta, int b, int c, int s, float slope,
                  float* y, hipStream_t st) {
  hipLaunchKernelGGL(bn_act_apply_kernel<BnSink::Store>, dim3(bn_apply_blocks(s), b * c),
                     dim3(256), 0, st, x, fin, mean, invstd, gamma, beta, c, s / 4, slope, y);
}

// the backward statistics pass into part [c][bn_parts(b)]
void bn_bwd_stats(const float* dz, const float* x, const BnParam& bn, int b, int c, int s,
                  float* part, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_stats_kernel, dim3(c, bn_parts(b)), dim3(256), 0, st, dz, x, bn, b, c,
                     s, part);
}

// dbias_in[c] = the sum of rowpart [b][c][nch], when the caller asks for it
void bn_bias_finalize(BnForm form, const float* rowpart, int b, int c, int nch, float* dbias_in,
                      hipStream_t st) {
  if (dbias_in == nullptr) return;
  if (form == BnForm::Split)  // long rows
    hipLaunchKernelGGL(bn_bias_finalize_block_kernel, dim3(c), dim3(256), 0, st, rowpart, b, c,
                       nch, dbias_in);
  else
    hipLaunchKernelGGL(bn_bias_finalize_kernel, dim3(ceil_div(c, 4)), dim3(256), 0, st, rowpart,
                       b, c, nch, dbias_in);
}

float bn_inv_n(int b, int s) { return (float)(1.0 / ((double)b * s)); }

// the contiguous backward apply on partials [c][P] + the producer's bias
// gradient through rowpart (used when dbias_in is given)
void bn_bwd_apply(const float* dz, const float* x, const BnParam& bn, const float* part, int P,
                  int b, int c, int s, float* dx, float* dgamma, float* dbeta, float* dbias_in,
                  float* rowpart, hipStream_t st) {
  const int nch = bn_bwd_blocks(s);
  if (dbias_in == nullptr) rowpart = nullptr;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nch, b * c), dim3(256), 0, st, dz, x, bn, part, P,
                     dgamma, dbeta, c, s / 4, bn_inv_n(b, s), dx, rowpart);
  bn_bias_finalize(BnForm::Contig, rowpart, b, c, nch, dbias_in, st);
}

// the split backward apply with the sums policy SUMS + the bias gradient
template <class SUMS>
void bn_bwd_apply_split(const float* dz, const float* x, const BnParam& bn, const SUMS& sums,
                        int b, int c, int s, void* dxs, float* dgamma, float* dbeta,
                        float* dbias_in, float* rowpart, hipStream_t st) {
  if (dbias_in == nullptr) rowpart = nullptr;
  uint16_t* dxh = (uint16_t*)dxs;
  hipLaunchKernelGGL(bn_bwd_apply_split_kernel<SUMS>, dim3(s / 64, c / 64, b), dim3(256), 0, st,
                     dz, x, bn.mean, bn.invstd, bn.gamma, bn.beta, bn.slope, sums, dgamma, dbeta, c,
                     s, bn_inv_n(b, s), dxh, dxh + kSplitLo, rowpart);
  bn_bias_finalize(BnForm::Split, rowpart, b, c, s / 64, dbias_in, st);
}

int se_stat_parts(int b, int c, int s) {  // blocks per (b, c) row of the SE statistics pass
  const long long rows = (long long)b * c;
  const int by_len = std::max(1, ceil_div(s / 4, 1024));
  const int by_grid = (int)std::max(1LL, (2048 + rows - 1) / rows);
  return std::min(by_len, by_grid);
}

}  // namespace
}  // namespace pcfm

using namespace pcfm;

extern "C" size_t pcfm_bn_workspace_bytes(int b, int c, int s) {
  if (!bn_ok(b, c, s)) return 0;
  const size_t rowpart = (size_t)b * c * bn_bwd_blocks(s);
  return ((size_t)c * bn_parts(b) * 2 + rowpart) * sizeof(float);
}

extern "C" int pcfm_bn_act_fwd(const float* x, const float* gamma, const float* beta, int b, int c,
                               int s, float eps, float slope, float momentum, float* running_mean,
                               float* running_var, long long* num_batches_tracked, float* y,
                               float* mean, float* invstd, void* ws, size_t ws_bytes,
                               void* stream) {
  const char* what = "bn_act_fwd";
  BN_TRY(bn_check(what, b, c, s, BnForm::Contig, ws_bytes, pcfm_bn_workspace_bytes(b, c, s)));
  BN_TRY(bn_check_running(what, running_mean, running_var));
  hipStream_t st = (hipStream_t)stream;
  const BnFwdFin fin = bn_fwd_stats(x, b, c, s, eps, momentum, running_mean, running_var,
                                    num_batches_tracked, (float*)ws, st);
  bn_fwd_apply(x, fin, mean, invstd, gamma, beta, b, c, s, slope, y, st);
  return check_launch(what);
}

// pcfm_bn_act_fwd with the statistics from the producer's epilogue (part float2
// [c][P], see bn_fin_parts_kernel): no statistics pass over x.
extern "C" int pcfm_bn_act_fwd_parts(const float* x, const float* part, int P, const float* gamma,
                                     const float* beta, int b, int c, int s, float eps,
                                     float slope, float momentum, float* running_mean,
                                     float* running_var, long long* num_batches_tracked, float* y,
                                     float* mean, float* invstd, void* stream) {
  const char* what = "bn_act_fwd_parts";
  BN_TRY(bn_check(what, b, c, s, BnForm::Contig, 0, 0));
  BN_TRY(bn_check_running(what, running_mean, running_var));
  hipStream_t st = (hipStream_t)stream;
  BnFwdFin fin;
  BN_TRY(bn_fwd_stats_parts(what, part, P, b, c, s, eps, momentum, running_mean, running_var,
                            num_batches_tracked, mean, invstd, st, &fin));
  bn_fwd_apply(x, fin, mean, invstd, gamma, beta, b, c, s, slope, y, st);
  return check_launch(what);
}

extern "C" int pcfm_bn_fwd_stats(const float* x, const float* part, int P, int b, int c, int s,
                                 float eps, float momentum, float* running_mean,
                                 float* running_var, long long* num_batches_tracked, float* mean,
                                 float* invstd, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "bn_fwd_stats";
  BN_TRY(bn_check(what, b, c, s, BnForm::Contig, 0, 0));
  BN_TRY(bn_check_running(what, running_mean, running_var));
  hipStream_t st = (hipStream_t)stream;
  if (part != nullptr) {  // the producer's epilogue statistics (pcfm_pointwise_gemm_bnstats)
    BnFwdFin fin;
    BN_TRY(bn_fwd_stats_parts(what, part, P, b, c, s, eps, momentum, running_mean, running_var,
                              num_batches_tracked, mean, invstd, st, &fin));
  } else {
    PCFM_CHECK_ARG(ws_bytes >= pcfm_bn_workspace_bytes(b, c, s), "%s: workspace too small", what);
    const BnFwdFin fin = bn_fwd_stats(x, b, c, s, eps, momentum, running_mean, running_var,
                                      num_batches_tracked, (float*)ws, st);
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(ceil_div(c, 256)), dim3(256), 0, st, x, fin, c,
                       mean, invstd);
  }
  return check_launch(what);
}

extern "C" int pcfm_bn_act_fwd_split(const float* x, const float* gamma, const float* beta, int b,
                                     int c, int s, float eps, float slope, float momentum,
                                     float* running_mean, float* running_var,
                                     long long* num_batches_tracked, void* ys, float* mean,
                                     float* invstd, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "bn_act_fwd_split";
  BN_TRY(bn_check(what, b, c, s, BnForm::Split, ws_bytes, pcfm_bn_workspace_bytes(b, c, s)));
  BN_TRY(bn_check_running(what, running_mean, running_var));
  hipStream_t st = (hipStream_t)stream;
  const BnFwdFin fin = bn_fwd_stats(x, b, c, s, eps, momentum, running_mean, running_var,
                                    num_batches_tracked, (float*)ws, st);
  uint16_t* yh = (uint16_t*)ys;
  hipLaunchKernelGGL(bn_act_apply_split_kernel, dim3(s / 64, c / 64, b), dim3(256), 0, st, x,
                     fin, mean, invstd, gamma, beta, c, s, slope, yh, yh + kSplitLo);
  return check_launch(what);
}

extern "C" int pcfm_bn_act_bwd(const float* dz, const float* x, const float* gamma,
                               const float* beta, const float* mean, const float* invstd, int b,
                               int c, int s, float slope, float* dx, float* dgamma, float* dbeta,
                               float* dbias_in, void* ws, size_t ws_bytes, void* stream) {
  const char* what = "bn_act_bwd";
  BN_TRY(bn_check(what, b, c, s, BnForm::Contig, ws_bytes, pcfm_bn_workspace_bytes(b, c, s)));
  hipStream_t st = (hipStream_t)stream;
  const BnParam bn{mean, invstd, gamma, beta, slope};
  float* part = (float*)ws;
  bn_bwd_stats(dz, x, bn, b, c, s, part, st);
  bn_bwd_apply(dz, x, bn, part, bn_parts(b), b, c, s, dx, dgamma, dbeta, dbias_in,
               part + (size_t)c * bn_parts(b) * 2, st);
  return check_launch(what);
}

// pcfm_bn_act_bwd's apply pass (+ the producer's bias gradient) on statistics
// a neighbouring kernel produced: part float2 [c][P] of (sum g, sum g xhat).
extern "C" int pcfm_bn_act_bwd_apply_parts(const float* dz, const float* x, const float* gamma,
                                           const float* beta, const float* mean,
                                           const float* invstd, const float* part, int P, int b,
                                           int c, int s, float slope, float* dx, float* dgamma,
                                           float* dbeta, float* dbias_in, void* ws,
                                           size_t ws_bytes, void* stream) {
  const char* what = "bn_act_bwd_apply_parts";
  BN_TRY(bn_check(what, b, c, s, BnForm::Contig, 0, 0));
  PCFM_CHECK_ARG(part != nullptr && P > 0, "%s: no statistics", what);
  PCFM_CHECK_ARG(dbias_in == nullptr ||
                     ws_bytes >= (size_t)b * c * bn_bwd_blocks(s) * sizeof(float),
                 "%s: workspace too small", what);
  hipStream_t st = (hipStream_t)stream;
  bn_bwd_apply(dz, x, BnParam{mean, invstd, gamma, beta, slope}, part, P, b, c, s, dx, dgamma,
               dbeta, dbias_in, (float*)ws, st);
  return check_launch(what);
}

extern "C" size_t pcfm_bn_act_bwd_split_workspace_bytes(int b, int c, int s) {
  if (!bn_ok(b, c, s) || c % 64 != 0 || s % 64 != 0) return 0;
  return ((size_t)c * bn_parts(b) * 2 + (size_t)b * c * (s / 64)) * sizeof(float);
}

extern "C" int pcfm_bn_act_bwd_split(const float* dz, const float* x, const float* gamma,
                                     const float* beta, const float* mean, const float* invstd,
                                     int b, int c, int s, float slope, void* dxs, float* dgamma,
                                     float* dbeta, float* dbias_in, void* ws, size_t ws_bytes,
                                     void* stream) {
  const char* what = "bn_act_bwd_split";
  BN_TRY(bn_check(what, b, c, s, BnForm::Split, ws_bytes,
                  pcfm_bn_act_bwd_split_workspace_bytes(b, c, s)));
  hipStream_t st = (hipStream_t)stream;
  const BnParam bn{mean, invstd, gamma, beta, slope};
  float* part = (float*)ws;
  bn_bwd_stats(dz, x, bn, b, c, s, part, st);
  bn_bwd_apply_split(dz, x, bn, BnPartSums{part, bn_parts(b)}, b, c, s, dxs, dgamma, dbeta,
                     dbias_in, part + (size_t)c * bn_parts(b) * 2, st);
  return check_launch(what);
}

// --- PVConv's BN3d + LeakyReLU fused with SE3d and the devoxelization ------
extern "C" size_t pcfm_bn_act_fwd_rowmean_workspace_bytes(int b, int c, int s) {
  if (!bn_ok(b, c, s)) return 0;
  return pcfm_bn_workspace_bytes(b, c, s) + (size_t)b * c * bn_apply_blocks(s) * sizeof(float);
}

extern "C" int pcfm_bn_act_fwd_rowmean(const float* x, const float* gamma, const float* beta,
                                       int b, int c, int s, float eps, float slope,
                                       float momentum, float* running_mean, float* running_var,
                                       long long* num_batches_tracked, float* rowmean,
                                       float* mean, float* invstd, void* ws, size_t ws_bytes,
                                       void* stream) {
  const char* what = "bn_act_fwd_rowmean";
  BN_TRY(bn_check(what, b, c, s, BnForm::Contig, ws_bytes,
                  pcfm_bn_act_fwd_rowmean_workspace_bytes(b, c, s)));
  BN_TRY(bn_check_running(what, running_mean, running_var));
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  float* rowpart = part + pcfm_bn_workspace_bytes(b, c, s) / sizeof(float);
  const BnFwdFin fin = bn_fwd_stats(x, b, c, s, eps, momentum, running_mean, running_var,
                                    num_batches_tracked, part, st);
  const int nblk = bn_apply_blocks(s);
  hipLaunchKernelGGL(bn_act_apply_kernel<BnSink::RowSum>, dim3(nblk, b * c), dim3(256), 0, st, x,
                     fin, mean, invstd, gamma, beta, c, s / 4, slope, rowpart);
  hipLaunchKernelGGL(rowpart_sum_kernel, dim3(ceil_div(b * c, 256)), dim3(256), 0, st,
                     (const float*)rowpart, b * c, nblk, (float)(1.0 / (double)s), rowmean);
  return check_launch(what);
}

extern "C" size_t pcfm_bn_se_bwd_workspace_bytes(int b, int c, int s) {
  if (!bn_ok(b, c, s) || c % 64 != 0 || s % 64 != 0) return 0;
  return ((size_t)b * c * se_stat_parts(b, c, s) * kSeSums + (size_t)b * c * (s / 64)) *
         sizeof(float);
}

extern "C" int pcfm_bn_se_bwd_stats(const float* g, const float* x, const float* mean,
                                    const float* invstd, const float* gamma, const float* beta,
                                    int b, int c, int s, float slope, float* rowstats, void* ws,
                                    size_t ws_bytes, void* stream) {
  const char* what = "bn_se_bwd_stats";
  BN_TRY(bn_check(what, b, c, s, BnForm::Split, ws_bytes, pcfm_bn_se_bwd_workspace_bytes(b, c, s)));
  hipStream_t st = (hipStream_t)stream;
  const int PS = se_stat_parts(b, c, s);
  float* part = (float*)ws;
  hipLaunchKernelGGL(bn_se_bwd_stats_kernel, dim3(PS, b * c), dim3(256), 0, st, g, x,
                     BnParam{mean, invstd, gamma, beta, slope}, c, s, part);
  hipLaunchKernelGGL(bn_se_rowstats_kernel, dim3(ceil_div(b * c * kSeSums, 256)), dim3(256), 0,
                     st, (const float*)part, b * c, PS, rowstats);
  return check_launch(what);
}

extern "C" int pcfm_bn_se_bwd_apply_split(const float* g, const float* x, const float* mean,
                                          const float* invstd, const float* gamma,
                                          const float* beta, const float* se_scale,
                                          const float* dmv, const float* rowstats, int b, int c,
                                          int s, float slope, void* dxs, float* dgamma,
                                          float* dbeta, float* dbias_in, void* ws,
                                          size_t ws_bytes, void* stream) {
  const char* what = "bn_se_bwd_apply_split";
  BN_TRY(bn_check(what, b, c, s, BnForm::Split, ws_bytes, pcfm_bn_se_bwd_workspace_bytes(b, c, s)));
  bn_bwd_apply_split(g, x, BnParam{mean, invstd, gamma, beta, slope},
                     BnSeSums{se_scale, dmv, rowstats, b}, b, c, s, dxs, dgamma, dbeta, dbias_in,
                     (float*)ws + (size_t)b * c * se_stat_parts(b, c, s) * kSeSums,
                     (hipStream_t)stream);
  return check_launch(what);
}

// --- GroupNorm: the FiLM residual (plain, and over a SharedMLP layer's
// pre-BatchNorm tensor) and ContextNet's SiLU head share their passes ---------
extern "C" size_t pcfm_gn_film_workspace_bytes(int b, int c, int n, int groups) {
  if (!gn_ok(b, c, n, groups)) return 0;
  const size_t fwd = ((size_t)b * groups * kGnParts * 2 + 3 * (size_t)b * c) * sizeof(float);
  const size_t bwd = ((size_t)b * c * kGnParts * 2 + 3 * (size_t)b * c) * sizeof(float);
  return fwd > bwd ? fwd : bwd;
}

static int gn_check(const char* what, int b, int c, int n, int groups, bool bn_needed,
                    bool bn_given, size_t ws_bytes) {
  PCFM_CHECK_ARG(gn_ok(b, c, n, groups), "%s: bad shape b=%d c=%d n=%d groups=%d", what, b, c, n,
                 groups);
  PCFM_CHECK_ARG(!bn_needed || bn_given, "%s: BatchNorm operands missing", what);
  PCFM_CHECK_ARG(ws_bytes >= pcfm_gn_film_workspace_bytes(b, c, n, groups),
                 "%s: workspace too small", what);
  return PCFM_OK;
}

// statistics -> per-(b, c) coefficients -> apply.  IN: x is a pre-BatchNorm
// tensor read through bn; SILU: out = SiLU(GN(x)), else the FiLM residual.
template <bool IN, bool SILU>
static int gn_forward(const char* what, const float* x, const BnParam& bn, const float* w,
                      const float* bias, const float* gamma, const float* beta, int b, int c,
                      int n, int groups, float eps, float* out, float* mean, float* rstd, void* ws,
                      size_t ws_bytes, void* stream) {
  BN_TRY(gn_check(what, b, c, n, groups, IN, bn.complete(), ws_bytes));
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  float* coef = part + (size_t)b * groups * kGnParts * 2;
  const dim3 rows(ceil_div(n / 4, 256), b * c);
  hipLaunchKernelGGL(gn_stats_kernel<IN>, dim3(groups * kGnParts, b), dim3(256), 0, st, x, c, n,
                     groups, part, bn);
  hipLaunchKernelGGL(gn_finalize_kernel, dim3(ceil_div((long long)b * c, 256)), dim3(256), 0, st,
                     (const float*)part, x, w, bias, gamma, b, c, n, groups, eps, mean, rstd,
                     coef, bn);
  if (SILU)
    hipLaunchKernelGGL(gn_silu_apply_kernel, rows, dim3(256), 0, st, x, (const float*)coef, n / 4,
                       out);
  else
    hipLaunchKernelGGL(gn_film_apply_kernel<IN>, rows, dim3(256), 0, st, x, (const float*)coef,
                       beta, n / 4, out, c, bn);
  return check_launch(what);
}

// row sums -> group coefficients and the parameter gradients -> apply.  ACT:
// the SiLU head (no residual, no FiLM gradients); IN: dx is dL/dz and bnpart
// receives the BatchNorm's backward partials.
template <bool ACT, bool IN>
static int gn_backward(const char* what, const float* dout, const float* x, const BnParam& bn,
                       const float* w, const float* bias, const float* gamma, const float* mean,
                       const float* rstd, int b, int c, int n, int groups, float* dx, float* dw,
                       float* dbias, float* dgamma, float* dbeta, float* bnpart, void* ws,
                       size_t ws_bytes, void* stream) {
  BN_TRY(gn_check(what, b, c, n, groups, IN, bn.complete() && bnpart != nullptr, ws_bytes));
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  float* kc = part + (size_t)b * c * kGnParts * 2;
  hipLaunchKernelGGL((gn_bwd_stats_kernel<ACT, IN>), dim3(kGnParts, b * c), dim3(256), 0, st, dout,
                     x, mean, rstd, w, bias, c, n, groups, part, bn);
  hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)part, w,
                     bias, gamma, rstd, b, c, n, groups, kc, dgamma, dbeta, dw, dbias);
  hipLaunchKernelGGL((gn_film_bwd_apply_kernel<ACT, IN>), dim3(ceil_div(n / 4, 256), b * c),
                     dim3(256), 0, st, dout, x, mean, rstd, (const float*)kc, w, bias, c, groups,
                     n / 4, dx, bn, bnpart);
  return check_launch(what);
}

extern "C" int pcfm_gn_film_res_fwd(const float* x, const float* w, const float* bias,
                                    const float* gamma, const float* beta, int b, int c, int n,
                                    int groups, float eps, float* out, float* mean, float* rstd,
                                    void* ws, size_t ws_bytes, void* stream) {
  return gn_forward<false, false>("gn_film_res_fwd", x, BnParam{}, w, bias, gamma, beta, b, c, n,
                                  groups, eps, out, mean, rstd, ws, ws_bytes, stream);
}

extern "C" int pcfm_gn_film_res_bwd(const float* dout, const float* x, const float* w,
                                    const float* bias, const float* gamma, const float* mean,
                                    const float* rstd, int b, int c, int n, int groups, float* dx,
                                    float* dw, float* dbias, float* dgamma, float* dbeta,
                                    void* ws, size_t ws_bytes, void* stream) {
  return gn_backward<false, false>("gn_film_res_bwd", dout, x, BnParam{}, w, bias, gamma, mean,
                                   rstd, b, c, n, groups, dx, dw, dbias, dgamma, dbeta, nullptr,
                                   ws, ws_bytes, stream);
}

// --- the PV block's post SharedMLP activation fused into its GroupNorm-FiLM
// residual (models.py:349-368: out = z + GN(z) (1 + gamma) + beta with
// z = ReLU(BN(y)), y = post's 1x1 conv output): z is never written, and the
// BatchNorm's backward statistics come out of the GroupNorm backward's apply.
extern "C" int pcfm_gn_film_res_fwd_bnin(const float* y, const float* bn_mean,
                                         const float* bn_invstd, const float* bn_gamma,
                                         const float* bn_beta, float slope, const float* w,
                                         const float* bias, const float* gamma,
                                         const float* beta, int b, int c, int n, int groups,
                                         float eps, float* out, float* mean, float* rstd,
                                         void* ws, size_t ws_bytes, void* stream) {
  return gn_forward<true, false>("gn_film_res_fwd_bnin", y,
                                 BnParam{bn_mean, bn_invstd, bn_gamma, bn_beta, slope}, w, bias,
                                 gamma, beta, b, c, n, groups, eps, out, mean, rstd, ws, ws_bytes,
                                 stream);
}

extern "C" int pcfm_gn_bnin_parts(int b, int n) {
  if (b <= 0 || n <= 0 || n % 4 != 0) return 0;
  return b * ceil_div(n / 4, 256);
}

extern "C" int pcfm_gn_film_res_bwd_bnin(const float* dout, const float* y, const float* bn_mean,
                                         const float* bn_invstd, const float* bn_gamma,
                                         const float* bn_beta, float slope, const float* w,
                                         const float* bias, const float* gamma, const float* mean,
                                         const float* rstd, int b, int c, int n, int groups,
                                         float* dz, float* dw, float* dbias, float* dgamma,
                                         float* dbeta, float* bnpart, void* ws, size_t ws_bytes,
                                         void* stream) {
  return gn_backward<false, true>("gn_film_res_bwd_bnin", dout, y,
                                  BnParam{bn_mean, bn_invstd, bn_gamma, bn_beta, slope}, w, bias,
                                  gamma, mean, rstd, b, c, n, groups, dz, dw, dbias, dgamma, dbeta,
                                  bnpart, ws, ws_bytes, stream);
}

// ContextNet head: SiLU(GroupNorm(x)) (models.py:460-466 head_norm + head_act)
extern "C" int pcfm_gn_silu_fwd(const float* x, const float* w, const float* bias, int b, int c,
                                int n, int groups, float eps, float* out, float* mean, float* rstd,
                                void* ws, size_t ws_bytes, void* stream) {
  return gn_forward<false, true>("gn_silu_fwd", x, BnParam{}, w, bias, nullptr, nullptr, b, c, n,
                                 groups, eps, out, mean, rstd, ws, ws_bytes, stream);
}

extern "C" int pcfm_gn_silu_bwd(const float* dout, const float* x, const float* w,
                                const float* bias, const float* mean, const float* rstd, int b,
                                int c, int n, int groups, float* dx, float* dw, float* dbias,
                                void* ws, size_t ws_bytes, void* stream) {
  return gn_backward<true, false>("gn_silu_bwd", dout, x, BnParam{}, w, bias, nullptr, mean, rstd,
                                  b, c, n, groups, dx, dw, dbias, nullptr, nullptr, nullptr, ws,
                                  ws_bytes, stream);
}
