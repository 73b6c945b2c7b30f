/* pcfm_fps.h -- farthest-point sampling of a batch of clouds of D-component
 * points (D = 2, 3, 5, 6), for AMD Instinct MI355X (gfx950): the even subsample
 * the generation metrics take before they compare clouds (pcfm/metrics.py).  A
 * sibling of pcfm.h, pcfm_chamfer_nd.h and pcfm_chamfer_cross.h, implemented by
 * the same libpcfm_hip.so (csrc/fps.hip) and under the same conventions:
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
 * Meaning, per cloud c, with k = min(d, 3) leading components (the position; a
 * colour does not steer the sampling):
 *   idx[c][0] = start ? clamp(start[c], 0, n - 1) : 0   (clamped in the kernel);
 *   idx[c][j], j >= 1, = the LOWEST index i that maximises
 *       dmin_j(i) = min over t < j of D(i, idx[c][t]),   the minimum starting at +inf;
 *   out[c][j][:] = a bit copy of all d components of pts[c][idx[c][j]].
 * D is the one fp32 chain of pcfm_chamfer_nd.h over the differences p_i - p_sel:
 * at k = 3 fma(dz, dz, fma(dx, dx, dy * dy)), at k = 2 fma(dx, dx, dy * dy).
 * m > n is allowed: once every remaining distance is 0 the rule yields index 0.
 * Non-finite coordinates: the picks are unspecified, every index is in [0, n).
 *
 * Ties: the reference's CUDA kernel (pvcnn sampling.cu) breaks a tie by the slot
 * of the thread that scanned the point in its 512-thread strided scan, an
 * artefact of that launch shape.  Here a tie goes to the lowest index, whatever
 * ran.  No atomics: the result does not depend on b, on the stream or on which
 * of the two kernel forms ran, and two calls return the same bits.
 */
#ifndef PCFM_FPS_H
#define PCFM_FPS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCFM_FPS_ABI_VERSION 1

int pcfm_fps_abi_version(void);

/* 1 for d = 2, 3, 5, 6; 0 otherwise. */
int pcfm_fps_supported(int d);

/* The largest n whose cloud one block keeps in registers for all m rounds (the
 * resident form); above it the streaming form runs.  At least 20000. */
int pcfm_fps_resident_points(void);

/* 0 while n <= pcfm_fps_resident_points(); above that the running minima,
 * b * n * sizeof(float) bytes. */
size_t pcfm_fps_workspace_bytes(int b, int n, int m, int d);

/* pts f32 [b][n][d]; start i32 [b] or NULL; idx i32 [b][m]; out f32 [b][m][d]
 * or NULL (then only idx is written).  m == 0 or b == 0: nothing runs.
 * Refused: a negative size, an unsupported d, n == 0 with b > 0 and m > 0,
 * b * n >= 2^31, b * m >= 2^31, ws_bytes below the query's answer. */
int pcfm_fps(const float* pts, int b, int n, int d, int m, const int* start, int* idx,
             float* out, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCFM_FPS_H */
