/* altro_multistart.h -- several initial guesses ("starts") per problem on a batched handle of include/altro_hip.h, the best
 * one chosen on the device.  Exported by libaltro_hip.so.
 *
 * A handle of B = P * G instances holds P PROBLEMS with G STARTS each: start g of problem p is instance p * G + g, so the
 * starts of a problem are adjacent columns.  The caller has given the starts of a problem the same initial state,
 * parameters, reference and tracks -- nothing checks this, and nothing of it is ever copied.  Every call takes
 * starts = G and is stateless: no grouping is stored on the handle.  starts = 1 is valid (the winner is 0, a spread is a
 * no-op).
 *
 * THE SELECTION RULE.  Per instance the key is built from exactly the status, cost and violation that altro_get_stats
 * reports (the AL or the iLQR status as altro_get_stats chooses):
 *   class 0   status == ALTRO_SOLVED, cost and violation finite     ordered by cost
 *   class 1   any other status, cost and violation finite           ordered by violation, then cost
 *   class 2   cost or violation NaN or infinite                     (start index only)
 * The lower class wins; comparisons are fp64 `<` (-0.0 and 0.0 tie); every tie goes to the lowest start index.  A total
 * order: the winner does not depend on the order of the reduction.
 *
 * Refused before any device work: starts < 1, B % starts != 0, a NULL handle, a required pointer NULL
 * (ALTRO_INVALID_ARG); no solve has finished on the handle yet (select, spread, get_best) or an asynchronous solve is in
 * flight (ALTRO_NOT_READY); no usable device (ALTRO_HIP_ERROR -- there is no CPU fallback).
 *
 * Every entry point with a pointer argument has a host form and a _device twin whose pointers name memory of the handle's
 * device; a _device form returns when the work on the handle's stream is done. */
#ifndef ALTRO_MULTISTART_H_
#define ALTRO_MULTISTART_H_

#include "altro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* winner[P]: the winning start index in [0, G) of every problem.  Changes nothing on the handle. */
altro_status altro_multistart_select(altro_handle h, int starts, int* winner);
altro_status altro_multistart_select_device(altro_handle h, int starts, void* winner_device);

/* Selects, then copies the winner's column over every other start of its problem: X, U, the gain records as stored
 * (fp32 under ALTRO_F32), duals, penalties, stored constraint values and knot costs.  NOT copied: the initial state,
 * per-instance parameters, reference and track records, expansion and cost-to-go records, the per-instance solver-state
 * scalars and statistics (altro_get_stats still answers per start), the history, and the guess altro_reset_trajectory
 * restores.  Invalidates a cost-to-go replay exactly as altro_set_trajectory does.  winner[P] may be NULL. */
altro_status altro_multistart_spread(altro_handle h, int starts, int* winner);
altro_status altro_multistart_spread_device(altro_handle h, int starts, void* winner_device);

/* U[b][k][i] += dU[...][k][i], a plain fp64 addition (no scale factor).  dU is [G][N][m] -- one block per start, shared by
 * all problems -- or [B][N][m] with per_instance.  X, gains, duals and penalties are untouched (the next solve rolls X out
 * itself).  Needs no finished solve.  Invalidates a cost-to-go replay. */
altro_status altro_multistart_perturb(altro_handle h, int starts, const double* dU, int per_instance);
altro_status altro_multistart_perturb_device(altro_handle h, int starts, const void* dU_device, int per_instance);

/* X[P][N+1][n], U[P][N][m], stats[P], winner[P] of the winners only, in the layouts of altro_get_trajectory and
 * altro_get_stats.  Each pointer may be NULL, but not all of them.  Changes nothing on the handle. */
altro_status altro_multistart_get_best(altro_handle h, int starts, double* X, double* U, altro_stats* stats, int* winner);
altro_status altro_multistart_get_best_device(altro_handle h, int starts, void* X_device, void* U_device, void* stats_device,
                                              void* winner_device);

/* cycles x (altro_solve_al; record iterations and status per instance; spread; altro_mpc_advance by `shift` with x0 = the
 * plan and w[c]; perturb with dU unless it is NULL) -- bit for bit the caller's own loop over the entry points above and
 * those of altro_mpc.h.  w (host [cycles][B][n] or NULL) and dU (host, shaped as altro_multistart_perturb takes it, or NULL)
 * are copied to the device once, before the first cycle; nothing crosses to the host inside the loop.
 * X_cl, U_cl, iterations, status: shaped as altro_mpc_run gives them, per instance -- after a spread the starts of a
 * problem log identical rows of X_cl and U_cl, and the caller who wants one row per problem takes every G-th.
 * winner[P][cycles].  Each output may be NULL.  Refuses what altro_mpc_advance refuses. */
altro_status altro_mpc_run_multistart(altro_handle h, int starts, int cycles, int shift, const double* w, const double* dU,
                                      int dU_per_instance, double* X_cl, double* U_cl, int* iterations, int* status, int* winner);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_MULTISTART_H_ */
