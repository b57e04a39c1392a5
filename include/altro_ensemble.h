/* altro_ensemble.h -- Monte-Carlo ensembles of the closed loop on a batched handle of include/altro_hip.h: Gaussian initial
 * errors and process noise drawn INSIDE the tracking kernel, reduced over the samples on the device to per-knot moments and
 * violation counts.  Exported by libaltro_hip.so.
 *
 * altro_mpc_track (include/altro_mpc.h) simulates S samples per instance that the caller brings; altro_cov_propagate
 * (include/altro_covariance.h) predicts their spread.  The calls below check the prediction against a sample of any size
 * under the real model and the clipped controls, and nothing of size B x S crosses to the host unless it is asked for.
 *
 * THE DRAW (a counter-based generator: a draw is a pure function of its counter, whoever makes it, in any order).
 *   Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, 10 rounds.
 *   key     = (seed & 0xffffffff, seed >> 32)
 *   counter = (k, s, (instance_base + b) mod 2^32, (stream << 16) | j)        j < 65536
 *   One call gives the words r0..r3 and the normal pair (z_{2j}, z_{2j+1}):
 *     u1 = ((r0 >> 5) 2^26 + (r1 >> 6) + 0.5) 2^-53, u2 the same from r2, r3;
 *     rad = sqrt(-2 ln u1), z_{2j} = rad cos(2 pi u2), z_{2j+1} = rad sin(2 pi u2), all in fp64.
 *   stream 0, k = knot: the process noise of knot k of sample s;  stream 0, k = 0xffffffff: the initial error of sample s;
 *   stream 1, k = knot, s = 0: the multi-start control perturbation of knot k.
 *   instance_base shifts the instance index, so that a handle holding instances [base, base + B) of a larger problem draws
 *   what the larger handle would draw for them.
 *
 * THE FACTOR.  Noise of covariance W is L xi with xi = (z_0 .. z_{n-1}) and L the lower factor of the symmetric matrix whose
 * lower triangle (i >= j) is W's -- the upper triangle is never read, as in altro_cov_propagate.  L is a semidefinite
 * Cholesky factor, column by column, with t = 4 n 2^-52 max_i |W_ii|:  d_j = W_jj - sum_{k<j} L_jk^2;  |d_j| <= t: the whole
 * column j of L is zero (a state that carries no noise);  d_j < -t: W is refused;  otherwise L_jj = sqrt(d_j) and
 * L_ij = (W_ij - sum_k L_ik L_jk) / L_jj.  (L xi)_i is accumulated by fused multiply-adds from zero, j = 0 .. i.  The factors
 * are computed on the device; a W or Sigma0 that is refused gives ALTRO_INVALID_ARG with the instance and knot in
 * altro_last_error, before the ensemble is launched.
 *
 * Refused before any device work, each with a text in altro_last_error.  ALTRO_INVALID_ARG: a NULL handle; steps outside
 * [1, N]; samples < 1; w_mode outside 0..3; u_lo without u_hi or the reverse; viol_tol negative or not finite; all outputs
 * NULL; sigma NULL, negative or not finite; starts as altro_multistart_perturb refuses it.  ALTRO_UNSUPPORTED: more than 32
 * states.  ALTRO_NOT_READY: no backward pass has left gains on the handle (the ensemble); an asynchronous solve in flight.
 * No usable device: ALTRO_HIP_ERROR -- there is no CPU fallback. */
#ifndef ALTRO_ENSEMBLE_H_
#define ALTRO_ENSEMBLE_H_

#include "altro_hip.h"
#include "altro_mpc.h"
#include "altro_covariance.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct altro_ensemble_stats { /* one per instance */
  int samples;         /* S */
  int stopped_state;   /* samples that ended with ALTRO_STATE_LIMIT */
  int stopped_control; /* samples that ended with ALTRO_CONTROL_LIMIT */
  int violated;        /* samples whose largest violation exceeds viol_tol */
  double cost_mean;    /* over the samples that ran to the end (NaN if none did) */
  double cost_max;     /* the same samples (NaN if none) */
  double violation_max; /* over all samples, as are max_dx and max_du */
  double max_dx;
  double max_du;
} altro_ensemble_stats;

/* Every (instance b, sample s) is exactly a lane of altro_mpc_track with
 *     dx0[b][s]  = L0 xi,  xi from the stream-0 draw at k = 0xffffffff,  L0 the factor of Sigma0 ([n][n], or [B][n][n] with
 *                  sigma0_per_instance)
 *     w[b][s][k] = L_k xi, xi from the stream-0 draw at knot k,  L_k the factor of W_k (W and w_mode as in
 *                  include/altro_covariance.h)
 * in place of the caller's arrays; the policy, the clip to u_lo / u_hi ([m] each, both or neither), the step, the bound
 * checks, the objective cost, the violation and max_dx / max_du are the track's.  A NULL Sigma0 or W means zero, and no draw
 * is made for it.  With e_k = x_k - Xbar_k and a sample ALIVE AT k when k <= steps_done:
 *   alive      [B][steps + 1]        samples alive at k
 *   dev_mean   [B][steps + 1][n]     mean of e_k over the samples alive at k
 *   dev_mom2   [B][steps + 1][n][n]  mean of e_k e_k^T over the same samples: the second moment ABOUT THE PLAN, which is what
 *                                    Sigma_k of altro_cov_propagate predicts; symmetric bit for bit.  The covariance of the
 *                                    sample is dev_mom2 - dev_mean dev_mean^T.
 *   viol_count [B][steps + 1]        samples alive at k whose violation AT knot k (as altro_max_violation evaluates that
 *                                    knot) exceeds viol_tol; the terminal knot counts only if steps == N, else that entry is 0
 *   summary    [B]
 *   stats      [B][samples]          optional: what altro_mpc_track would report per sample
 * A knot with nobody alive has quiet-NaN moments.  Each output may be NULL (not all of them).  Every sum is taken in an order
 * that depends on (B, samples, steps) alone: a repeated call returns the same bits.  The call changes nothing on the handle.
 * The _device form takes every array in memory of the handle's device (fp64; alive and viol_count int; summary and stats the
 * structs), stages nothing, and returns when the work on the handle's stream is done. */
altro_status altro_mpc_ensemble(altro_handle h, int steps, int samples, unsigned long long seed, unsigned long long instance_base,
                                const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, const double* u_lo,
                                const double* u_hi, double viol_tol, double* dev_mean, double* dev_mom2, int* alive,
                                int* viol_count, altro_ensemble_stats* summary, altro_track_stats* stats);
altro_status altro_mpc_ensemble_device(altro_handle h, int steps, int samples, unsigned long long seed,
                                       unsigned long long instance_base, const void* Sigma0_device, int sigma0_per_instance,
                                       const void* W_device, int w_mode, const void* u_lo_device, const void* u_hi_device,
                                       double viol_tol, void* dev_mean_device, void* dev_mom2_device, void* alive_device,
                                       void* viol_count_device, void* summary_device, void* stats_device);

/* The very arrays altro_mpc_track takes, dx0 [B][samples][n] and w [B][samples][steps][n] (either may be NULL, not both),
 * from the draws the ensemble makes: altro_mpc_track on them reproduces the ensemble's samples bit for bit.  A NULL Sigma0 or
 * W fills zeros.  Needs no gains. */
altro_status altro_noise_fill(altro_handle h, int steps, int samples, unsigned long long seed, unsigned long long instance_base,
                              const double* Sigma0, int sigma0_per_instance, const double* W, int w_mode, double* dx0, double* w);
altro_status altro_noise_fill_device(altro_handle h, int steps, int samples, unsigned long long seed,
                                     unsigned long long instance_base, const void* Sigma0_device, int sigma0_per_instance,
                                     const void* W_device, int w_mode, void* dx0_device, void* w_device);

/* U[b][k][i] += sigma[i] z_i (one fused multiply-add), z from the stream-1 draw at (k, 0, instance_base + b); sigma [m] in
 * host memory.  With keep_first the first start of every problem (instance p * starts) is left bit for bit.  The
 * preconditions and effects on the handle are those of altro_multistart_perturb (include/altro_multistart.h). */
altro_status altro_multistart_perturb_gaussian(altro_handle h, int starts, unsigned long long seed, unsigned long long instance_base,
                                               const double* sigma, int keep_first);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_ENSEMBLE_H_ */
