/* pcfm_occupancy.h -- occupancy counts of a set of clouds of D-component points
 * (D = 3, 5, 6) on an r x r x r grid over the unit cube, for AMD Instinct MI355X
 * (gfx950): the histogram the Jensen-Shannon divergence of the generation
 * metrics reduces (pcfm/metrics.py).  A sibling of pcfm.h, pcfm_chamfer_nd.h,
 * pcfm_chamfer_cross.h and pcfm_fps.h, implemented by the same libpcfm_hip.so
 * (csrc/occupancy.hip) and under the same conventions:
 *
 *   - every pointer is a device pointer, row-major contiguous, extents as stated;
 *   - `stream` is a hipStream_t passed as void* (0 = the default stream); calls
 *     enqueue work and return, nothing allocates, nothing synchronises;
 *   - the return value is PCFM_OK (0), PCFM_EINVAL (-1: an argument was refused on
 *     the host and NOTHING was launched or written) or a hipError_t; the message
 *     is pcfm.h's pcfm_last_error;
 *   - the *_workspace_bytes() query returns 0 for arguments the entry point refuses;
 *   - nothing is read or written outside the stated extents, and no result
 *     depends on what the output or the workspace held before the call.
 *
 * Meaning.  Only the first three components of a point (the position) take
 * part; the clouds are counted as given, nothing normalises them into the cube
 * [-0.5, 0.5]^3 the grid spans.
 *
 * Nodes: node (i, j, k), 0 <= i, j, k < r, has flat index (i * r + j) * r + k
 * and is KEPT iff a*a + b*b + c*c <= (r-1)*(r-1), with a = 2i - (r-1), b and c
 * likewise from j and k: an integer test, the grid point within radius 0.5 of
 * the centre.  (r = 28: 10144 of 21952 nodes are kept and none lies on the
 * boundary; r = 2 keeps no node.)
 *
 * A point p is counted in exactly one kept node:
 *   1. u = fma(p, r-1, (r-1)/2) per axis in fp32 (grid units);
 *      c = clamp(rint(u), 0, r-1) per axis, rint rounding half to even.
 *      If node c is kept, the point counts there.
 *   2. Otherwise it counts in the kept node (i, j, k) of LOWEST flat index that
 *      minimises the fp32 chain of pcfm_chamfer_nd.h over u minus the node's
 *      integer coordinates: with dx = u.x - i, dy = u.y - j, dz = u.z - k,
 *      fma(dz, dz, fma(dx, dx, dy * dy)).
 * The rule has two branches on purpose: a single argmin would disagree with the
 * rounding at half-way points and at fp32 rounding boundaries.
 *
 * counts[f] = the number of points of all s clouds counted in node f.  Every
 * entry of counts is written, a node that is not kept gets 0, the sum is s * n.
 * Non-finite coordinates: that point's node is unspecified but kept, and the sum
 * still holds.  The counts are integers summed by integer adds: the result does
 * not depend on s, on the launch shape, on the stream or on the run.
 */
#ifndef PCFM_OCCUPANCY_H
#define PCFM_OCCUPANCY_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCFM_OCCUPANCY_ABI_VERSION 1

int pcfm_occupancy_abi_version(void);

/* 1 for d = 3, 5, 6 and 3 <= r <= 32; 0 otherwise (d = 2: the grid is
 * three-dimensional). */
int pcfm_occupancy_supported(int d, int r);

/* The partial histograms of the counting blocks: (number of blocks) * r^3 * 4
 * bytes, the number of blocks a function of s * n alone (at most 256).  0 when
 * s * n == 0. */
size_t pcfm_occupancy_workspace_bytes(int s, int n, int d, int r);

/* pts f32 [s][n][d]; counts i32 [r*r*r].  s == 0 or n == 0: counts is all zeros.
 * Refused: a negative size, an unsupported d or r, s * n >= 2^31, ws_bytes below
 * the query's answer. */
int pcfm_occupancy_counts(const float* pts, int s, int n, int d, int r, int* counts, void* ws,
                          size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCFM_OCCUPANCY_H */
