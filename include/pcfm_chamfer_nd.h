/* pcfm_chamfer_nd.h -- Chamfer distance over D-component points (D = 2, 3, 5, 6)
 * for AMD Instinct MI355X (gfx950): a sibling of pcfm.h, implemented by the same
 * libpcfm_hip.so (csrc/chamfer_nd.hip) and under the same conventions:
 *
 *   - every pointer is a device pointer, row-major contiguous, extents as stated;
 *   - `stream` is a hipStream_t passed as void* (0 = the default stream); calls
 *     enqueue work and return, nothing synchronises;
 *   - the return value is PCFM_OK (0), PCFM_EINVAL (-1: an argument was refused on
 *     the host and NOTHING was launched or written) or a hipError_t; the message
 *     is pcfm.h's pcfm_last_error;
 *   - a *_workspace_bytes() query returns 0 for arguments the entry point refuses;
 *   - nothing is read or written outside the stated extents, and no result
 *     depends on what an output or the workspace held before the call.
 *
 * Replaces the reference's chamfer_2D / chamfer_5D / chamfer_6D extension modules
 * (third_party/ChamferDistancePytorch/chamfer{2,5,6}D/); D = 3 is offered so the
 * kernel can be compared with pcfm_chamfer_fwd's brute-force search bit for bit.
 *
 * Squared-distance contract, one fp32 chain with dk = candidate[k] - query[k]:
 *   acc = d1*d1;  acc = fma(d0, d0, acc);  acc = fma(dk, dk, acc), k = 2 .. D-1
 * (at D = 3 the contract of pcfm_chamfer_fwd).  Ties: lowest index.
 */
#ifndef PCFM_CHAMFER_ND_H
#define PCFM_CHAMFER_ND_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCFM_CHAMFER_ND_ABI_VERSION 1

int pcfm_chamfer_nd_abi_version(void);

/* 1 for d = 2, 3, 5, 6; 0 otherwise. */
int pcfm_chamfer_nd_supported(int d);

size_t pcfm_chamfer_nd_workspace_bytes(int b, int n, int m, int d);

/* Forward, both directions.
 *   p1 f32 [b, n, d]  p2 f32 [b, m, d]
 *   dist1 f32 [b, n], idx1 i32 [b, n]: squared distance / index of the nearest
 *   point of p2 (ties -> lowest index); dist2/idx2 [b, m] the same from p2 to p1.
 * n == 0 or m == 0: the outputs that exist are written 0.  b == 0: nothing runs.
 * Refused: a negative size, an unsupported d, b > 32767 or b * max(n, m) >= 2^31,
 * ws_bytes below the query's answer. */
int pcfm_chamfer_nd_fwd(const float* p1, const float* p2, int b, int n, int m, int d,
                        float* dist1, float* dist2, int* idx1, int* idx2, void* ws,
                        size_t ws_bytes, void* stream);

/* Backward: g = 2 * grad_dist; the query's gradient += g * (q - p_nn), the matched
 * point's -= the same term.  ACCUMULATES (float atomics) into grad_p1 [b, n, d] and
 * grad_p2 [b, m, d] (callers zero them); an index outside the other cloud is skipped. */
int pcfm_chamfer_nd_bwd(const float* p1, const float* p2, int b, int n, int m, int d,
                        const float* grad_dist1, const float* grad_dist2, const int* idx1,
                        const int* idx2, float* grad_p1, float* grad_p2, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCFM_CHAMFER_ND_H */
