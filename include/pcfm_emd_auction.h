/* pcfm_emd_auction.h -- the assignment earth mover's distance: a one-to-one match
 * of two clouds of n points of D components each (D = 2, 3, 5, 6), float32, by
 * the parallel (Jacobi) auction with eps scaling, for AMD Instinct MI355X
 * (gfx950).  A sibling of pcfm.h, pcfm_chamfer_nd.h, pcfm_chamfer_cross.h,
 * pcfm_fps.h, pcfm_occupancy.h and pcfm_emd_nd.h, implemented by the same
 * libpcfm_hip.so (csrc/emd_auction.hip) and under the same conventions:
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
 * THE RULE.  The kernel and the CPU backend (pcfm.cpu_ops.emd_auction) both
 * follow it to the fp32 bit.  Every pair of the batch is a problem of its own.
 *
 *   Costs.  c(i, j) = d2(p1[i], p2[j]), the ONE fp32 chain of pcfm_chamfer_nd.h /
 *   pcfm_emd_nd.h with dc = p2[j][c] - p1[i][c]:
 *     acc = d1*d1;  acc = fma(d0, d0, acc);  acc = fma(dc, dc, acc), c = 2 .. d-1
 *   so the cost, and cost / n, are in the units of the approximate EMD's figures.
 *   cmax = max_ij c(i, j) (a NaN is passed over).
 *
 *   cmax == 0: the assignment is the identity, the cost 0, rounds 0.
 *
 *   Otherwise  eps_final = eps_rel * cmax          (one fp32 product),
 *              eps_0     = max(eps_final, cmax * 0.5),
 *              eps_{k+1} = max(eps_final, eps_k * 0.25),
 *   one phase per eps_k, the last the first with eps_k == eps_final.  All prices
 *   start at +0 and are kept across the phases; every phase starts with nobody
 *   assigned and repeats rounds until nobody is unassigned.
 *
 *   One round (Jacobi).  EVERY person unassigned at the start of the round bids,
 *   on the prices of the start of the round.  Person i takes
 *     v(j)  = (-c(i, j)) - price[j]                (one fp32 subtraction),
 *     j1    = the lowest index of the maximum of v,  v1 = v(j1),
 *     v2    = the maximum of v over j != j1 (v1 when n == 1),
 *     bid   = price[j1] + ((v1 - v2) + eps)        (each operation rounded to
 *             fp32, in that order);
 *   a bid that does not exceed price[j1] is the next float above price[j1].
 *   Every object that received bids goes to the highest bid, the lowest person
 *   among equal bids; its price becomes that bid and its previous owner becomes
 *   unassigned.  (The kernel works on w(j) = c(i, j) + price[j] = -v(j), the same
 *   bits with the sign turned: the minimum of w, and v1 - v2 = w2 - w1.)
 *
 *   Results.  assignment[i] = the index in p2 matched to p1[i]; cost = the float64
 *   sum over i of c(i, assignment[i]), rounded to float32; rounds = the number of
 *   rounds of all phases together.  A pair that would need a round beyond
 *   max_rounds is NOT FINISHED: rounds = -1, its assignment row all -1, cost NaN.
 *   Every output is fully written, finished or not.
 *
 * Guarantees.  A finished pair's assignment is a permutation of 0 .. n-1, and
 *   cost <= optimum + n * eps_final
 * (the eps-complementary-slackness bound of the auction's last phase).  Every
 * reduction of the rule is a maximum under a total order, so nothing depends on
 * the launch, the stream, the batch a pair is in, or the run.  Non-finite
 * coordinates give an unspecified result that is in range all the same: rounds
 * in [-1, max_rounds], assignment entries in [-1, n).
 *
 * No atomics on global memory; one launch per call, one block per pair, the whole
 * auction inside the kernel.  The block keeps both clouds and the auction's state
 * in LDS, which bounds n: pcfm_emd_auction_max_points(d).  There is no streaming
 * form: a larger n is refused (pcfm.metrics.subsample brings clouds there).
 *
 * Refused (PCFM_EINVAL): a negative size, an unsupported d, n above
 * pcfm_emd_auction_max_points(d), eps_rel not finite or outside [2^-20, 0.5],
 * max_rounds < 1, cost == NULL or rounds == NULL with b > 0, ws_bytes below the
 * query's answer.
 *
 * Empty problems: b == 0 does nothing; n == 0 writes cost 0 and rounds 0.
 */
#ifndef PCFM_EMD_AUCTION_H
#define PCFM_EMD_AUCTION_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCFM_EMD_AUCTION_ABI_VERSION 1

int pcfm_emd_auction_abi_version(void);

/* The largest n the entry point takes for points of d components: 0 for an
 * unsupported d (anything but 2, 3, 5, 6), else at least 2048. */
int pcfm_emd_auction_max_points(int d);

/* 0 today (the state lives in LDS); callers still ask, so that a later form
 * with a workspace needs no new binding. */
size_t pcfm_emd_auction_workspace_bytes(int b, int n, int d);

/* p1, p2 f32 [b][n][d] -> assignment i32 [b][n] (NULL: not written), cost f32 [b],
 * rounds i32 [b]. */
int pcfm_emd_auction_f32(const float* p1, const float* p2, int b, int n, int d, float eps_rel,
                         int max_rounds, int* assignment, float* cost, int* rounds, void* ws,
                         size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* PCFM_EMD_AUCTION_H */
