/* pcfm_chamfer_cross.h -- the S x R matrix of mean nearest-neighbour distances
 * between two SETS of clouds of D-component points (D = 2, 3, 5, 6), for AMD
 * Instinct MI355X (gfx950): every cloud of `a` against every cloud of `b`, no
 * cloud copied and no per-point result written.  What MMD, coverage and 1-NNA
 * under Chamfer distance reduce (pcfm/metrics.py).  A sibling of pcfm.h and
 * pcfm_chamfer_nd.h, implemented by the same libpcfm_hip.so
 * (csrc/chamfer_cross.hip) and under the same conventions:
 *
 *   - every pointer is a device pointer, row-major contiguous, extents as stated;
 *   - `stream` is a hipStream_t passed as void* (0 = the default stream); calls
 *     enqueue work and return, nothing allocates, nothing synchronises;
 *   - the return value is PCFM_OK (0), PCFM_EINVAL (-1: an argument was refused on
 *     the host and NOTHING was launched or written) or a hipError_t; the message
 *     is pcfm.h's pcfm_last_error;
 *   - the *_workspace_bytes() query returns 0 for arguments the entry point refuses;
 *   - nothing is read or written outside the stated extents, and no result
 *     depends on what an output or the workspace held before the call.
 *
 * Arithmetic: each nearest-neighbour minimum is the fp32 value pcfm_chamfer_nd_fwd
 * returns for the same pair of clouds (the one chain of pcfm_chamfer_nd.h).  The
 * minima of one (cloud, partner) are added in float64 in a fixed order, divided
 * by the point count in float64 and rounded to fp32 once.  No floating-point
 * atomics: two calls return the same bits.
 */
#ifndef PCFM_CHAMFER_CROSS_H
#define PCFM_CHAMFER_CROSS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCFM_CHAMFER_CROSS_ABI_VERSION 1

int pcfm_chamfer_cross_abi_version(void);

/* 1 for d = 2, 3, 5, 6; 0 otherwise. */
int pcfm_chamfer_cross_supported(int d);

/* 0 while both n and m are at most 2048 (one block then holds a whole cloud's
 * queries and writes the mean itself); above that, one float64 partial per
 * (pair, block of 2048 queries). */
size_t pcfm_chamfer_cross_workspace_bytes(int s, int r, int n, int m, int d);

/* a f32 [s][n][d], b f32 [r][m][d] (a == b allowed: the inputs are only read)
 *   ab f32 [s][r]: ab[i][j] = mean over the points p of a_i of min_q |b_j[q] - p|^2
 *   ba f32 [s][r]: ba[i][j] = mean over the points q of b_j of min_p |a_i[p] - q|^2
 * n == 0 or m == 0: both outputs are written 0.  s == 0 or r == 0: nothing runs.
 * Refused: a negative size, an unsupported d, s * n >= 2^31, r * m >= 2^31,
 * s * r * (ceil(n / 2048) + ceil(m / 2048)) >= 2^31 (the launch's block count),
 * ws_bytes below the query's answer. */
int pcfm_chamfer_cross_fwd(const float* a, const float* b, int s, int r, int n, int m, int d,
                           float* ab, float* ba, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCFM_CHAMFER_CROSS_H */
