/* altro_tracking.h -- following a reference path: per-knot LQR tracking costs whose references live on the device, on a
 * batched handle of include/altro_hip.h.  Exported by libaltro_hip.so.
 *
 * The reference writes path following as a loop, prob.SetCostFunction(LQRCost(Q, R, xref_k, uref_k), k) for every knot
 * (altro/problem/problem.hpp:113-127, one CostFunction per knot).  Here every DISTINCT cost is a cost group and a problem
 * holds a few of them, so that loop does not fit altro_set_lqr_cost; and nothing could move such references along with a
 * receding horizon.  A tracking cost is one group for a whole range of knots: Q and R are the group's, the references are
 * rows of a path that is uploaded once, windowed by an offset, and moved by altro_mpc_advance (include/altro_mpc.h). */
#ifndef ALTRO_TRACKING_H_
#define ALTRO_TRACKING_H_

#include "altro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TRACKING A REFERENCE PATH.  Problem::SetCostFunction(LQRCost(Q, R, xref_k, uref_k), k) for k_begin <= k < k_end with a
 * DIFFERENT xref_k, uref_k on every knot -- the reference's per-knot loop -- as ONE cost group: the references are the
 * handle's reference path (altro_set_reference) at knot k, and the terms q_k = -Q xref_k, r_k = -R uref_k,
 * c_k = 0.5 xref_k'Q xref_k + 0.5 uref_k'R uref_k live on the device, one record per (knot, instance), computed there by
 * one kernel with the rounding of altro_set_lqr_cost's terms (a constant path gives the same bits).  Problem definition:
 * before the first compute call.  The last cost set on a knot wins, whichever kind; several ranges with different Q, R
 * may exist (typically [0, N) and [N, N + 1)), each counts as one of the distinct cost functions a problem may hold.  Knots
 * with an ordinary or a user cost ignore the reference.  A handle with a tracking cost runs on the solver's general kernels,
 * like one with per-knot steps. */
altro_status altro_set_lqr_tracking_cost(altro_handle h, int k_begin, int k_end, const double* Q, const double* R);

/* The reference path: Xref[rows][n], Uref[rows][m] (Uref may be NULL: zeros), [B][rows][.] with per_instance; rows >= 1.
 * Knot k of the horizon uses path row min(offset + k, rows - 1): a window into a longer path whose end is held.  The path
 * belongs to the trajectory side, like altro_set_steps: it may be set at any time between solves, and setting it puts the
 * window offset back to 0.  altro_set_reference_offset moves the window (offset >= 0); altro_mpc_advance and everything built
 * on it add their shift to it on a handle with a tracking cost (altro_mpc.h).  A solve or a cost evaluation that meets a
 * tracking knot before a path is set returns ALTRO_NOT_READY.  Both invalidate a cost-to-go replay as altro_set_trajectory
 * does.  altro_set_reference_device takes fp64 arrays in memory of the handle's device: nothing crosses to the host; like
 * the other *_device calls it creates the device state, so the problem definition must be complete. */
altro_status altro_set_reference(altro_handle h, const double* Xref, const double* Uref, int rows, int per_instance);
altro_status altro_set_reference_device(altro_handle h, const void* Xref_device, const void* Uref_device, int rows,
                                        int per_instance);
altro_status altro_set_reference_offset(altro_handle h, int offset);
altro_status altro_get_reference_offset(altro_handle h, int* offset);
/* The terms as the kernels read them: q[B][N+1][n], r[B][N+1][m], c[B][N+1] (any pointer may be NULL); knots without a
 * tracking cost read zero. */
altro_status altro_get_reference_terms(altro_handle h, double* q, double* r, double* c);

#ifdef __cplusplus
}
#endif

#endif  /* ALTRO_TRACKING_H_ */
