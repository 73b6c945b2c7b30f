/* pcfm_emd_nd.h -- the approximate earth mover's distance (approxmatch, matchcost
 * and its gradient) over D-component points (D = 2, 3, 5, 6), float32, for AMD
 * Instinct MI355X (gfx950).  A sibling of pcfm.h, pcfm_chamfer_nd.h,
 * pcfm_chamfer_cross.h, pcfm_fps.h and pcfm_occupancy.h, implemented by the same
 * libpcfm_hip.so (csrc/emd.hip over csrc/emd_core.hpp) and under the same
 * conventions:
 *
 *   - every pointer is a device pointer, row-major contiguous, extents as stated;
 *   - `stream` is a hipStream_t passed as void* (0 = the default stream); calls
 *     enqueue work and return, nothing allocates, nothing synchronises;
 *   - the return value is PCFM_OK (0), PCFM_EINVAL (-1: an argument was refused on
 *     the host and NOTHING was launched or written) or a hipError_t; the message
 *     is pcfm.h's pcfm_last_error;
 *   - the *_workspace_bytes() query returns 0 for arguments the entry points refuse;
 *   - nothing is read or written outside the stated extents, and no result
 *     depends on what an output or the workspace held before the call.
 *
 * Meaning.  What pcfm.h's pcfm_emd_*_f32 entries (csrc/emd.hip) define for three
 * components, with the squared distance taken over all d components:
 *
 *   - d2(k, l) between p1[k] and p2[l] is the ONE fp32 chain of pcfm_chamfer_nd.h
 *     with dc = p2[l][c] - p1[k][c]:
 *       acc = d1*d1;  acc = fma(d0, d0, acc);  acc = fma(dc, dc, acc), c = 2 .. d-1
 *     (at d = 3 the chain of the 3-D entries);
 *   - ten levels, level_j = -4^j for j = 7 .. -1, then 0; remainL starts at
 *     multiL = 1 (n >= m) or m / n, remainR at multiR = n / m (n >= m) or 1, the
 *     integer quotients;
 *   - exp(level * d2) is the hardware exp2 of float(d2) * (level * log2 e), and
 *     level 0 is exactly 1;
 *   - per level: ratioL = remainL / (1e-9 + suml),
 *     ratioR = min(remainR / (sumr + 1e-9), 1) * remainR,
 *     remain = max(0, remain - sum);
 *   - match[l][k] = sum_j (exp(level_j * d2) * ratioL_j[k]) * ratioR_j[l], summed
 *     in level order;
 *   - cost = sum_{k,l} d2(k, l) * match[l][k]; pcfm_emd_nd_approxmatch_cost_f32
 *     sums it from the match kernel's own values (match is not read back).
 *
 * At d = 3 every entry returns the bits of its pcfm.h counterpart.  A component
 * that is one constant in both clouds adds fma(0, 0, acc) = acc to d2: it leaves
 * match and cost unchanged and has a zero gradient.
 *
 * EVERY COMPONENT ENTERS WITH THE SAME WEIGHT.  Scaling colour against position
 * is the caller's data convention, as for the 6-D Chamfer distance.
 *
 * No atomics anywhere: two calls on the same inputs give the same bits, on any
 * stream, and a batch element's result does not depend on b.
 *
 * Refused (PCFM_EINVAL): a negative size, an unsupported d, ws_bytes below the
 * query's answer, cost == NULL with b > 0 in pcfm_emd_nd_approxmatch_cost_f32.
 * Like the 3-D entries, the host refuses no extent: b is a grid dimension of
 * every kernel, so b above 65535 (or m above 65535 * 32) fails at the launch and
 * comes back as a hipError_t.
 *
 * Empty problems, as in the 3-D entries: b == 0 does nothing; n == 0 or m == 0
 * writes zeros to cost, grad1 and grad2 (match then has no element).
 */
#ifndef PCFM_EMD_ND_H
#define PCFM_EMD_ND_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCFM_EMD_ND_ABI_VERSION 1

int pcfm_emd_nd_abi_version(void);

/* 1 for d = 2, 3, 5, 6; 0 otherwise. */
int pcfm_emd_nd_supported(int d);

/* One size for all three entries.  It grows with the pack width: a point and
 * the coefficient it carries take 4 floats for d <= 3 and 8 for d = 5, 6. */
size_t pcfm_emd_nd_workspace_bytes(int b, int n, int m, int d);

/* p1 f32 [b][n][d], p2 f32 [b][m][d] -> match f32 [b][m][n] (NULL: not written,
 * the cost alone) and cost f32 [b]. */
int pcfm_emd_nd_approxmatch_cost_f32(const float* p1, const float* p2, int b, int n, int m,
                                     int d, float* match, float* cost, void* ws,
                                     size_t ws_bytes, void* stream);

/* cost [b] = sum_{k,l} d2(k, l) * match[l][k] of a given match [b][m][n]. */
int pcfm_emd_nd_matchcost_f32(const float* p1, const float* p2, const float* match, int b,
                              int n, int m, int d, float* cost, void* ws, size_t ws_bytes,
                              void* stream);

/* grad1 [b][n][d] = grad_cost[b] * sum_l 2 match[l][k] (p1[k] - p2[l]),
 * grad2 [b][m][d] = grad_cost[b] * sum_k 2 match[l][k] (p2[l] - p1[k]); both fully
 * written. */
int pcfm_emd_nd_matchcost_bwd_f32(const float* grad_cost, const float* p1, const float* p2,
                                  const float* match, int b, int n, int m, int d,
                                  float* grad1, float* grad2, void* ws, size_t ws_bytes,
                                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCFM_EMD_ND_H */
