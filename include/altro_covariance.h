/* altro_covariance.h -- the closed-loop covariance of a plan under its feedback gains, and circle tracks inflated by it, on a
 * batched handle of include/altro_hip.h.  Exported by libaltro_hip.so.
 *
 * altro_mpc_track (include/altro_mpc.h) answers what happened to S sampled disturbances.  The calls below answer what a
 * planner asks before it commits to a plan: how far the plant will be from the plan at knot k under the gains the solver
 * just produced, and whether the obstacle margin covers it.  For every instance b
 *
 *     Sigma_0     = Sigma0[b]
 *     [A_k | B_k] = the discrete Jacobian of knot k's own model, step and time at (Xbar_k, Ubar_k)
 *                   (what altro_update_expansions would compute there)
 *     F_k         = A_k + B_k K_k          (K as altro_get_gains returns it; under ALTRO_F32 its fp32 record widened, as
 *                                           altro_mpc_track does)
 *     Sigma_{k+1} = F_k Sigma_k F_k^T + W_k        k = 0 .. steps-1
 *
 * in fp64 throughout.  Only the LOWER triangle (i >= j) of Sigma0 and of W is read, so an unsymmetric input cannot matter,
 * and every Sigma_k that comes out is symmetric bit for bit.  The plan, the gains and the Jacobians never leave the device.
 * Every model kind is accepted (per-knot steps, times and models, time-varying and discrete user models) up to 32 states
 * (more: ALTRO_UNSUPPORTED); nothing moves along the horizon.  What stands behind the limit: the whole call is tested
 * against its numpy statement on models of n <= 13 states (groups of 1 .. 16 lanes); beyond that only the recursion kernel
 * is, driven on its own (tests/cpp/recur_driver.hip: n = 16, 17, 24 and 32).  The linearisation of a model of more than 13
 * states has never run, and a user-model plug-in of more than about 13 states takes minutes to compile.
 *
 * The second call turns the covariance into tightened constraints for the next solve: the track of a knot circle constraint
 * (include/altro_knot_params.h) becomes base radius + kappa * position spread at that knot.  A position is (x[0], x[1]), the
 * states the built-in circle reads (as include/altro_team.h).  For a Gaussian position error e with covariance P,
 * |e| <= kappa * sqrt(lambda_max(P)) holds with probability >= 1 - exp(-kappa^2 / 2): kappa * rpos bounds the error with at
 * least that probability.
 *
 * Refused before any device work, each with a text in altro_last_error.  ALTRO_INVALID_ARG: a NULL handle; steps outside
 * [1, N]; all four outputs NULL; w_mode outside 0..3; rpos asked for with n < 2; an index that is no knot constraint or no
 * ALTRO_CON_CIRCLE; rows < 1; kappa negative or not finite; rpos or base NULL in altro_cov_inflate_circles*.
 * ALTRO_NOT_READY: no backward pass has left gains on the handle (altro_cov_propagate*); an asynchronous solve in flight.
 * No usable device: ALTRO_HIP_ERROR -- there is no CPU fallback. */
#ifndef ALTRO_COVARIANCE_H_
#define ALTRO_COVARIANCE_H_

#include "altro_hip.h"
#include "altro_knot_params.h"

#ifdef __cplusplus
extern "C" {
#endif

/* w_mode bits */
#define ALTRO_COV_W_PER_INSTANCE 1
#define ALTRO_COV_W_PER_KNOT 2

/* Sigma0: [n][n], or [B][n][n] with sigma0_per_instance; NULL = zero.
 * W:      [n][n] | [B][n][n] (ALTRO_COV_W_PER_INSTANCE) | [steps][n][n] (ALTRO_COV_W_PER_KNOT) | [B][steps][n][n] (both);
 *         NULL = zero.
 * Sigma:  [B][steps + 1][n][n]
 * sx:     [B][steps + 1][n]   sqrt(diag Sigma_k)
 * su:     [B][steps][m]       sqrt(diag(K_k Sigma_k K_k^T)): the spread of the feedback's control correction
 * rpos:   [B][steps + 1]      sqrt(lambda_max(Sigma_k[0:2, 0:2])), the larger eigenvalue of the symmetric 2 x 2 block in
 *                             closed form, (a + c) / 2 + sqrt(((a - c) / 2)^2 + b^2)
 * A negative argument of a square root is clamped to zero.  Each output may be NULL (not all four).  The call changes nothing
 * on the handle: trajectory, duals, stored constraint values, statistics, expansion records, gains and cost-to-go state all
 * stay.  The _device form takes every array in fp64 memory of the handle's device, stages nothing, and returns when the work
 * on the handle's stream is done. */
altro_status altro_cov_propagate(altro_handle h, int steps, const double* Sigma0, int sigma0_per_instance, const double* W,
                                 int w_mode, double* Sigma, double* sx, double* su, double* rpos);
altro_status altro_cov_propagate_device(altro_handle h, int steps, const void* Sigma0_device, int sigma0_per_instance,
                                        const void* W_device, int w_mode, void* Sigma_device, void* sx_device, void* su_device,
                                        void* rpos_device);

/* `index` names a knot constraint of kind ALTRO_CON_CIRCLE with nparams = 3 * nobs; `base` is its un-inflated track,
 * [rows][3 * nobs], or [B][rows][3 * nobs] with per_instance; rpos is [B][N + 1] (altro_cov_propagate with steps = N).  The
 * call writes the constraint's track, always per instance, on the device: in row r circle i keeps cx, cy of the base, and its
 * radius becomes rad + kappa * rpos[b][min(max(r - offset, 0), N)], offset = the handle's current track offset
 * (altro_get_track_offset), so that the row knot k reads now carries the spread of knot k.  The window offset stays;
 * afterwards the track behaves like any other under altro_set_track_offset and altro_mpc_advance.  A repeated call with the
 * same base does not compound.  Invalidates a cost-to-go replay as altro_set_constraint_track does; X, U, duals and
 * statistics are untouched.  The _device form takes base and rpos in fp64 memory of the handle's device.  Both return when the
 * work on the handle's stream is done. */
altro_status altro_cov_inflate_circles(altro_handle h, int index, const double* base, int rows, int per_instance, double kappa,
                                       const double* rpos);
altro_status altro_cov_inflate_circles_device(altro_handle h, int index, const void* base_device, int rows, int per_instance,
                                              double kappa, const void* rpos_device);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_COVARIANCE_H_ */
