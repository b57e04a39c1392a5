/* altro_trigger.h -- event-triggered re-planning: THE rule that says which instances need a new plan, evaluated on the device,
 * and a closed-loop run that re-solves only those.  Exported by libaltro_hip.so.  The first user of the solve mask of
 * include/altro_subset.h.
 *
 * THE RULE.  For every instance the reason is the OR of the criteria that hold, and the mask byte is reason != 0:
 *   ALTRO_TRIGGER_AGE        age >= max_age (age: cycles the plan has been followed since it was solved);
 *   ALTRO_TRIGGER_DEVIATION  tracked statistics given, dx_tol >= 0 and !(tracked.max_dx <= dx_tol);
 *   ALTRO_TRIGGER_VIOLATION  the same test on tracked.violation with viol_tol;
 *   ALTRO_TRIGGER_LIMIT      tracked statistics given and tracked.status != ALTRO_UNSOLVED: a limit stopped the sample.  Always on;
 *   ALTRO_TRIGGER_UNSOLVED   on_unsolved is set and the handle's status of the instance -- the one altro_get_stats reports: the
 *                            AL status, or the iLQR status in iLQR mode -- is not ALTRO_SOLVED;
 *   ALTRO_TRIGGER_AHEAD      lookahead > 0 and a one-sample, disturbance-free altro_mpc_track of `lookahead` knots -- from the
 *                            handle's current initial state, under the current plan and gains and the given u_lo / u_hi -- hits
 *                            a limit or has !(violation <= ahead_tol);
 *   ALTRO_TRIGGER_FIRST      set only by altro_mpc_run_triggered, in cycle 0.
 * The comparisons are written !(v <= tol) on purpose: a NaN triggers.  A negative tolerance switches its criterion off.
 * One function states the rule for the host and for the kernel (trigger_reason, altro_common.hpp).
 *
 * REFUSALS, before any device work, each with text in altro_last_error.
 *   ALTRO_INVALID_ARG: a NULL handle or rule; max_age < 1; a NaN tolerance; lookahead outside [0, N]; ahead_tol < 0 with
 *     lookahead > 0; exactly one of u_lo / u_hi given; for the run: cycles < 1, a shift outside [1, N - 1], and
 *     (max_age - 1) * shift + max(shift, lookahead) > N -- a plan that is not renewed would otherwise be followed, or looked
 *     ahead, into the held tail that the advance repeats.
 *   ALTRO_UNSUPPORTED: whatever altro_mpc_advance refuses (per-knot steps, times or models; a time-varying or discrete user
 *     model); a handle that records the cost-to-go (masked solves refuse it); for the run: a handle that carries a solve mask
 *     -- clear it first.
 *   ALTRO_NOT_READY: an asynchronous solve in flight; altro_mpc_trigger with lookahead > 0 before any gains exist; a missing
 *     reference path or constraint track, as altro_mpc_run_tracked answers.
 *   ALTRO_HIP_ERROR: no usable device -- there is no CPU fallback.
 * Left out: teams, multi-start and multi-GPU groups have no triggered run, and the run takes no mask of the caller's. */
#ifndef ALTRO_TRIGGER_H_
#define ALTRO_TRIGGER_H_

#include "altro_hip.h"
#include "altro_mpc.h"
#include "altro_subset.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct altro_trigger_rule {
  int max_age;     /* >= 1: cycles a plan may be followed; an instance whose age reaches it is re-planned */
  double dx_tol;   /* >= 0: tracked max_dx above it triggers; negative: criterion off */
  double viol_tol; /* >= 0: tracked violation above it triggers; negative: off */
  int on_unsolved; /* non-zero: re-plan while the instance's last solve did not end ALTRO_SOLVED */
  int lookahead;   /* 0: off; L in [1, N]: simulate the next L knots of the plan as it stands (ALTRO_TRIGGER_AHEAD) */
  double ahead_tol; /* >= 0, read only with lookahead > 0 */
} altro_trigger_rule;

enum {
  ALTRO_TRIGGER_FIRST = 1,
  ALTRO_TRIGGER_AGE = 2,
  ALTRO_TRIGGER_DEVIATION = 4,
  ALTRO_TRIGGER_VIOLATION = 8,
  ALTRO_TRIGGER_LIMIT = 16,
  ALTRO_TRIGGER_UNSOLVED = 32,
  ALTRO_TRIGGER_AHEAD = 64
};

/* Evaluate the rule for every instance.  Host arrays: tracked[B] (NULL: the three tracked criteria are off), age[B] (NULL:
 * age 0 everywhere), u_lo / u_hi [m] (both or neither; read by the lookahead only), mask[B] and reason[B] (NULL: not
 * written).  The call changes NOTHING on the handle, as altro_mpc_track does not. */
altro_status altro_mpc_trigger(altro_handle h, const altro_trigger_rule* rule, const altro_track_stats* tracked, const int* age,
                               const double* u_lo, const double* u_hi, unsigned char* mask, int* reason);
/* The same with every array pointer in memory of the handle's device: nothing crosses to the host, and mask_device can go
 * straight into altro_set_solve_mask_device.  Returns when the work on the handle's stream is done. */
altro_status altro_mpc_trigger_device(altro_handle h, const altro_trigger_rule* rule, const void* tracked_device,
                                      const void* age_device, const void* u_lo_device, const void* u_hi_device, void* mask_device,
                                      void* reason_device);

/* altro_mpc_run_tracked that re-plans only where the rule says so.  Cycle c, per instance b:
 *   1. the mask: everyone in cycle 0 (reason ALTRO_TRIGGER_FIRST), else what step 6 of cycle c - 1 found; compacted on the
 *      device, only the counts per engine slice come back;
 *   2. altro_solve_al under that mask (an all-zero mask launches nothing); a solved instance's age becomes 0;
 *   3. iterations[b][c] = iterations_total if b was solved in this cycle, else 0; status[b][c] = the handle's status as it
 *      stands; reason[b][c] = why b was solved in this cycle, 0 if it was not;
 *   4. track `shift` knots with one sample under w[c]: track[b][c] and the rows of X_cl / U_cl, as altro_mpc_run_tracked;
 *   5. advance by `shift` from the tracked end state, device to device; age += 1;
 *   6. evaluate the rule on track[b][c], the ages and the handle as it stands (not after the last cycle).
 * Bit for bit the caller's own loop over altro_set_solve_mask, altro_solve_al, altro_mpc_track, altro_mpc_advance and
 * altro_mpc_trigger.  An instance that is not re-planned keeps its shifted X, U, gains, duals and windows, and the next cycle
 * tracks u = Ubar + K (x - Xbar) from the measured state.  Nothing B-sized crosses to the host between the first and the last
 * cycle but the disturbance.  w: host [cycles][B][shift][n] or NULL; the logs are shaped as altro_mpc_run_tracked gives them,
 * plus reason[B][cycles]; each may be NULL.  The run leaves the handle without a mask, also after a failure. */
altro_status altro_mpc_run_triggered(altro_handle h, int cycles, int shift, const double* w, const double* u_lo, const double* u_hi,
                                     const altro_trigger_rule* rule, double* X_cl, double* U_cl, int* iterations, int* status,
                                     altro_track_stats* track, int* reason);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_TRIGGER_H_ */
