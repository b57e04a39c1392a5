/* altro_lqr.h -- time-varying LQR tracking gains about the plan a batched handle of include/altro_hip.h holds, computed on the
 * device and, on request, installed as the gains of the closed loop.  Exported by libaltro_hip.so.
 *
 * altro_mpc_track, altro_cov_propagate, altro_mpc_ensemble, the lookahead of altro_mpc_trigger and every altro_mpc_run_* run
 * the plant under u = Ubar_k + K_k (x - Xbar_k) with the K the solver's last backward pass left in the gain record.  Those are
 * gains of the augmented-Lagrangian cost, under the regularisation that pass needed, about the iterate before the last
 * accepted step.  The calls below give the tracking controller instead: for every instance b, in fp64 throughout,
 *
 *     [A_k | B_k] = the discrete Jacobian of knot k's own model, step and time at (Xbar_k, Ubar_k)
 *                   (what altro_update_expansions would compute there), k = 0 .. N - 1
 *     P_N = Qf
 *     S   = R + B_k^T P_{k+1} B_k,    G = B_k^T P_{k+1} A_k
 *     K_k = -S^-1 G                   (by the Cholesky factorisation of S without its square roots, S = L D L^T)
 *     P_k = Q + A_k^T P_{k+1} A_k + G^T K_k                                    k = N - 1 .. 0
 *
 * Q [n][n], R [m][m] and Qf [n][n] (NULL: Q) are shared by the batch; only their LOWER triangles (i >= j) are read.  Only the
 * lower triangle of every P_k is computed and the upper one is taken from it: every P_k is symmetric bit for bit.  The order
 * of every sum depends on (n, m) alone -- not on the batch, the launch or an instance's neighbours.  Every model kind is
 * accepted (per-knot steps, times and models, time-varying and discrete user models) with 1 <= m <= 8 controls and
 * n <= 32 states; every (n, m) in that range fits the 64 KiB of LDS the recursion may use, so none of them is refused.
 * What stands behind these limits: the whole call is tested against its numpy statement on models of n <= 13 states and
 * m <= 5 controls (groups of 1 .. 16 lanes); beyond that only the recursion kernel is, driven on its own
 * (tests/cpp/recur_driver.hip: n = 16, 17, 24, 32 and m = 6, 8, up to (n, m) = (32, 8), where it spills registers to scratch:
 * profiles/recur_shapes_resources.txt).  The linearisation of a model of more than 13 states has never run, and a user-model
 * plug-in of more than about 13 states takes minutes to compile (13 states: about five).
 *
 * Outputs (each may be NULL):
 *     K     [B][N][m * n]     column-major m x n per knot, as altro_get_gains returns it
 *     P     [B][N + 1][n][n]
 *     fail  [B]               -1, or the largest k at which a pivot of S_k was not positive or a value of K_k or P_k was not
 *                             finite; K and P of that instance from that knot down to 0 are quiet NaN
 * The call returns ALTRO_OK whatever `fail` says, as a solve does whatever its statuses say.  Q and Qf are not checked for
 * semidefiniteness: an indefinite one shows in `fail`.
 *
 * install != 0: for every instance whose fail is -1, K_k replaces K in the handle's gain record (under ALTRO_F32 rounded to the
 * record's fp32, as the backward pass stores it) and d_k becomes 0; a failed instance keeps its record bit for bit.  The
 * handle counts as holding gains from then on (altro_mpc_track and the others accept a handle that was only rolled out), and
 * a cost-to-go that was not recorded can no longer be read (altro_get_ctg: ALTRO_NOT_READY) -- its replay would write the
 * solver's gains back.  Nothing else changes: trajectory, duals, stored constraint values, statistics, expansion records and
 * cost-to-go records stay.  install == 0 changes nothing on the handle.  The direct calls ignore a solve mask
 * (include/altro_subset.h): they are no solve.
 *
 * The policy: altro_lqr_set_policy copies Q, R, Qf into the handle; while it is on, every whole solve -- altro_solve_al,
 * altro_solve_ilqr, altro_solve_al_async, and the solves inside altro_mpc_run, _run_tracked, _run_triggered, _run_multistart,
 * _run_team, altro_team_solve and altro_team_solve_sequential -- ends, on the handle's stream and before it returns, with the
 * same pass with install = 1.  Under a solve mask only the masked-in instances are installed; a masked-out instance keeps its
 * gain record bit for bit.  Off (the default), a solve does what it did.
 *
 * Refused before any device work, each with a text in altro_last_error.  ALTRO_INVALID_ARG: a NULL handle; Q or R NULL; a
 * lower-triangle entry that is not finite; an R that is not positive definite (a host Cholesky of its lower triangle);
 * install == 0 with K and P both NULL.  ALTRO_UNSUPPORTED: m < 1, m > 8 or n > 32.  ALTRO_NOT_READY: no integration step set;
 * an asynchronous solve in flight.  No usable device: ALTRO_HIP_ERROR -- there is no CPU fallback.  (The _device form reads
 * its weights back to check them: that copy comes first.) */
#ifndef ALTRO_LQR_H_
#define ALTRO_LQR_H_

#include "altro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ALTRO_LQR_MAX_STATES 32
#define ALTRO_LQR_MAX_CONTROLS 8

/* Host arrays.  Returns when the work on the handle's stream is done. */
altro_status altro_lqr_gains(altro_handle h, const double* Q, const double* R, const double* Qf, int install, double* K, double* P,
                             int* fail);
/* Every array in memory of the handle's device (Q, R, Qf, K, P fp64; fail int); stages nothing; returns when the work on the
 * handle's stream is done. */
altro_status altro_lqr_gains_device(altro_handle h, const void* Q_device, const void* R_device, const void* Qf_device, int install,
                                    void* K_device, void* P_device, void* fail_device);

/* Q == NULL: the policy goes off (R and Qf are not read).  May be called before the first compute call of a handle. */
altro_status altro_lqr_set_policy(altro_handle h, const double* Q, const double* R, const double* Qf);
/* on: 0 / 1; Q, R, Qf (each may be NULL) receive the symmetric matrices the policy holds, when it is on. */
altro_status altro_lqr_get_policy(altro_handle h, int* on, double* Q, double* R, double* Qf);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_LQR_H_ */
