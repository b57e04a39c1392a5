/* altro_mpc.h -- receding-horizon (model-predictive control) loops on a batched handle of include/altro_hip.h.
 *
 * The solver exists for MPC: solve, apply the first controls, move the horizon forward, warm-start, solve again.  The
 * warm start itself is two options of the reference -- AugmentedLagrangianiLQR::Init keeps the duals with
 * reset_duals = 0 and the penalties with initial_penalty = 0 (altro/augmented_lagrangian/al_solver.hpp:292-297) -- and
 * the handle keeps trajectory, gains, duals and penalties on the device between solves.  This header adds the missing
 * third part, the ADVANCE of a solved handle by `shift` knots, as one kernel launch on the handle's device: nothing of
 * the warm start crosses to the host.  Exported by libaltro_hip.so.
 *
 * The advance, per instance b (N = segments, 1 <= shift <= N - 1, "old" = the device arrays when the call is made):
 *   controls, gains   U_new[k] = U_old[min(k + shift, N - 1)], likewise the gain records K, d   (k = 0 .. N-1: the tail
 *                     repeats the last stage knot)
 *   states            X_new[k] = X_old[min(k + shift, N)]   (k = 0 .. N; a guess only: the next solve rolls X out again)
 *   initial state     x0_new = (x0 if given, else X_old[shift]) + (w if given), evaluated in fp64
 *   duals, penalties  per CONSTRAINT (the j-th altro_add_constraint / altro_add_user_constraint_type call), not per knot
 *                     class: for a stage knot k with src = min(k + shift, N - 1), a constraint attached to both k and src
 *                     takes lambda and rho of its rows at src; attached to k only, its rows start afresh -- lambda = 0,
 *                     rho = options.initial_penalty if that is > 0, else 1 (a new ConstraintValues,
 *                     altro/constraints/constraint_values.hpp:39-51).  The terminal knot's rows stay.
 *   reference window  on a handle with a tracking cost (altro_set_lqr_tracking_cost): offset_new = offset_old + shift, and
 *                     the term records are recomputed on the device for the new window (altro_set_reference_offset); a
 *                     handle without a tracking cost keeps its offset
 *   track window      on a handle with a knot constraint (altro_add_knot_constraint, altro_knot_params.h): the track offset
 *                     that all its constraint tracks share moves likewise, track offset_new = track offset_old + shift
 *                     (saturating at INT_MAX), and the knot-parameter records are copied anew on the device in the same
 *                     call (altro_set_track_offset); the constraint itself is ONE constraint of the row map above, so its
 *                     duals and penalties travel like any other's; a handle without a knot constraint keeps its offset
 * Everything else stays: options, statistics, history, the guess altro_reset_trajectory restores, and the costs, which
 * remain attached to knot indices (a tracking cost's Q, R too: only its reference moves).  Expansions, knot costs, stored constraint values and cost-to-go records are not moved;
 * the next solve recomputes them (altro_get_ctg answers ALTRO_NOT_READY until then).
 *
 * Refused: shift out of range (ALTRO_INVALID_ARG); a handle with per-knot steps, times or models, or a time-varying or
 * discrete user model (ALTRO_UNSUPPORTED); an asynchronous solve in flight (ALTRO_NOT_READY); no usable device
 * (ALTRO_HIP_ERROR -- there is no CPU fallback). */
#ifndef ALTRO_MPC_H_
#define ALTRO_MPC_H_

#include "altro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host-only: where every dual / penalty row comes from under a shift: src_row[r] in [0, rows), or -1 for a row that
 * starts afresh; src_row holds altro_num_constraints(h) entries (altro_mpc_num_rows(h) says how many without a device).
 * Needs no device for the built-in constraint kinds; works as soon as the constraints are registered. */
altro_status altro_mpc_row_map(altro_handle h, int shift, int* src_row);
int altro_mpc_num_rows(altro_handle h);

/* The advance.  x0 ([n], or [B][n] with x0_per_instance) and w ([B][n]) are host arrays, either may be NULL; they are
 * copied during the call. */
altro_status altro_mpc_advance(altro_handle h, int shift, const double* x0, int x0_per_instance, const double* w);
/* The same with fp64 arrays [B][n] in memory of the handle's device (either may be NULL): nothing crosses to the host.
 * Like altro_pack_*_device it returns when the work on the handle's stream is done. */
altro_status altro_mpc_advance_device(altro_handle h, int shift, const void* x0_device, const void* w_device);

/* cycles x (altro_solve_al with the handle's options as they stand; record; advance with x0 = the plan, w = w[c]) --
 * bit for bit the caller's own loop of altro_solve_al and altro_mpc_advance.  w: host [cycles][B][n] or NULL.
 * Outputs (host, each may be NULL), instance-major like trajectories:
 *   X_cl[B][cycles*shift + 1][n], U_cl[B][cycles*shift][m]: what the loop applied -- rows c*shift .. c*shift+shift-1 are
 *   X, U[0 .. shift) of cycle c's solution (X_cl[b][c*shift] is the initial state cycle c was solved from); the last row
 *   of X_cl is the initial state after the last advance;
 *   iterations[B][cycles], status[B][cycles]: iterations_total and the AL status of every cycle's solve.
 * The log is written on the device by the advance and downloaded once at the end. */
altro_status altro_mpc_run(altro_handle h, int cycles, int shift, const double* w, double* X_cl, double* U_cl, int* iterations,
                           int* status);

/* ---- between two solves: the plant under the plan's time-varying feedback policy ---------------------------------------
 * iLQR::RolloutClosedLoop (altro/ilqr/ilqr.hpp:468-499) with alpha = 0, as an entry point of its own: every (instance b,
 * disturbance sample s) is simulated for `steps` knots under u = Ubar + K (x - Xbar), one GPU lane each, by ONE kernel
 * launch.  Xbar, Ubar and K are the handle's device arrays as they stand (K is what altro_get_gains returns; under
 * ALTRO_F32 its fp32 record is widened to fp64 as the forward pass does):
 *   x_0 = x0[b] + dx0[b][s]
 *   for k = 0 .. steps-1:
 *     u_k     = Ubar_k + K_k (x_k - Xbar_k)              (ilqr.hpp:477-478)
 *     u_k     = min(max(u_k, u_lo), u_hi)                only where the bounds are given
 *     x_{k+1} = f_d(x_k, u_k, t_k, h_k) + w[b][s][k]     the knot's own step, time and model
 *     if options.check_forwardpass_bounds: |x_{k+1}|_2 > state_max -> ALTRO_STATE_LIMIT, else |u_k|_2 > control_max ->
 *       ALTRO_CONTROL_LIMIT (ilqr.hpp:484-495); the sample stops there with steps_done = k
 * A stopped sample keeps X_cl[0 .. steps_done] and U_cl[0 .. steps_done]; the log rows behind them are quiet NaN.
 * The call changes NOTHING on the handle: trajectory, duals, stored constraint values, statistics and cost-to-go state stay.
 * Every model kind is accepted (per-knot steps, times and models, time-varying and discrete user models): nothing moves
 * along the horizon here.
 * Refused before any device work: steps outside [1, N], samples < 1 or exactly one of u_lo / u_hi given
 * (ALTRO_INVALID_ARG); no backward pass has produced gains on this handle yet, or an asynchronous solve is in flight
 * (ALTRO_NOT_READY); no usable device (ALTRO_HIP_ERROR -- there is no CPU fallback). */
typedef struct altro_track_stats { /* one per (instance, sample) */
  int status;       /* ALTRO_UNSOLVED (ran to the end, as ilqr.hpp:497), ALTRO_STATE_LIMIT or ALTRO_CONTROL_LIMIT */
  int steps_done;   /* knots simulated before a limit stopped the sample (== steps otherwise) */
  double cost;      /* sum of the knots' OBJECTIVE cost (the quadratic / the user cost, no augmented-Lagrangian terms) along the
                       path, knots 0 .. steps-1 (0 .. steps_done of a stopped sample), plus the terminal knot's (u = 0) iff it
                       ran to the end and steps == N; added up in knot order */
  double violation; /* max constraint violation along the path, same knots, evaluated like altro_max_violation */
  double max_dx;    /* max_k |x_k - Xbar_k|_inf, k = 0 .. steps_done */
  double max_du;    /* max_k |u_k - Ubar_k|_inf, k = 0 .. min(steps_done, steps - 1) */
} altro_track_stats;

/* Host arrays, each may be NULL: dx0[B][S][n] and w[B][S][steps][n] (NULL = zero), u_lo / u_hi [m] (both or neither;
 * +-inf allowed), X_cl[B][S][steps+1][n], U_cl[B][S][steps][m], stats[B][S] (a large ensemble asks for the statistics only). */
altro_status altro_mpc_track(altro_handle h, int steps, int samples, const double* dx0, const double* w, const double* u_lo,
                             const double* u_hi, double* X_cl, double* U_cl, altro_track_stats* stats);
/* The same with every array pointer in memory of the handle's device: nothing crosses to the host.  Returns when the work
 * on the handle's stream is done. */
altro_status altro_mpc_track_device(altro_handle h, int steps, int samples, const void* dx0_device, const void* w_device,
                                    const void* u_lo_device, const void* u_hi_device, void* X_cl_device, void* U_cl_device,
                                    void* stats_device);
/* cycles x (altro_solve_al; track `shift` knots with ONE sample under w[c]; advance by `shift` with x0 = the tracked
 * x_shift, device to device) -- bit for bit the caller's own loop over altro_solve_al, altro_mpc_track and
 * altro_mpc_advance.  w: host [cycles][B][shift][n] or NULL.  X_cl, U_cl, iterations, status: shaped as altro_mpc_run gives
 * them, but X_cl / U_cl hold the TRACKED states and controls, not the planned ones (the last row of X_cl is the initial
 * state after the last advance); track[B][cycles]: the statistics of every cycle's tracking.  Each may be NULL.  Refuses
 * what altro_mpc_advance refuses. */
altro_status altro_mpc_run_tracked(altro_handle h, int cycles, int shift, const double* w, const double* u_lo, const double* u_hi,
                                   double* X_cl, double* U_cl, int* iterations, int* status, altro_track_stats* track);

/* What the next solve starts from, [B][n]. */
altro_status altro_get_initial_state(altro_handle h, double* x0);
/* Counterpart of altro_set_duals for the penalties, [B][rows]. */
altro_status altro_set_penalties(altro_handle h, const double* rho);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_MPC_H_ */
