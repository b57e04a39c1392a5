/* altro_subset.h -- solve a chosen subset of a handle's instances, and sequential team rounds built on it.  Exported by
 * libaltro_hip.so.
 *
 * THE SOLVE MASK.  A handle of B instances may carry a mask of B bytes; a non-zero byte b means that instance b takes part in
 * the whole solves that follow.  The mask belongs to the handle: it stays until it is changed or cleared, through every
 * setter, altro_mpc_advance and whatever else the handle is asked to do.  A handle that never had a mask, or whose mask was
 * cleared, behaves exactly as a handle of a library without this header: same bits, same launches.
 *
 * WHICH CALLS HONOUR IT.  Every WHOLE solve: altro_solve_al, altro_solve_ilqr, altro_solve_al_async, and the loops made of
 * them (altro_mpc_run*, altro_team_solve, the multi-start runs, altro_group_solve_al).  The step-level calls (altro_al_init,
 * altro_solve_setup, altro_rollout ... altro_update_penalties) IGNORE it and work on every instance, and so does everything
 * that is not a solve: altro_mpc_advance, the team and covariance fills, altro_multistart_select / _spread,
 * altro_mpc_track, altro_cov_propagate.
 *
 * WHAT A MASKED SOLVE DOES.
 *   A masked-out instance: nothing observable changes by a bit -- X, U, x0, multipliers, penalties, the stored constraint
 *     values, gains, expansion records, knot costs, every field of altro_get_stats and its history rows.
 *   A masked-in instance: exactly the solve it gets without a mask (the instances of a batch do not know of each other, and
 *     their order in the engine's lists does not enter their arithmetic).
 *   An all-zero mask: ALTRO_OK, nothing is launched and nothing changes.
 *   altro_get_timing: instance_iterations sums the iterations of the instances the last solve ran.
 *   Cost-to-go records: a masked solve on a handle with altro_set_record_ctg(h, 1) is refused with ALTRO_UNSUPPORTED (text in
 *     altro_last_error) before any device work -- the records are written for whole batches.  After a masked solve
 *     altro_get_ctg has nothing to replay and answers as it does after a setter has changed the handle.
 *
 * REFUSALS, before any device work.  ALTRO_INVALID_ARG: a NULL handle; a NULL pointer where the _device form or the getter
 * need one.  ALTRO_NOT_READY: an asynchronous solve owns the handle.  ALTRO_HIP_ERROR: no usable device -- there is no CPU
 * fallback.  The three calls put the problem on the device if it is not there yet, as the first compute call does, and
 * report what that reports. */
#ifndef ALTRO_SUBSET_H_
#define ALTRO_SUBSET_H_

#include "altro_hip.h"
#include "altro_team.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mask[B], host memory: non-zero bytes are the instances of the solves that follow.  NULL clears the mask (everyone again).
 * The bytes are copied; the array may go when the call returns.  Returns when the work on the handle's stream is done. */
altro_status altro_set_solve_mask(altro_handle h, const unsigned char* mask);

/* The same from B bytes in memory of the handle's device (NULL: ALTRO_INVALID_ARG -- clear with the host form).  The bytes
 * are copied on the device; B-independent, a handful of words (the instances per engine slice) come back to the host once,
 * here, not in the solves. */
altro_status altro_set_solve_mask_device(altro_handle h, const void* mask_device);

/* mask[B]: 1 for an instance that takes part, 0 for one that does not (all ones without a mask); *count, unless NULL: how
 * many take part. */
altro_status altro_get_solve_mask(altro_handle h, unsigned char* mask, int* count);

/* Sequential (Gauss-Seidel) team rounds on a team handle of include/altro_team.h: agent 0 of every team re-plans against
 * everyone's current plan, then agent 1, and so on --
 *     sweeps x ( for a = 0 .. agents - 1:  altro_team_fill_tracks(h, agents, index, radius, radius_per_instance,
 *                                                                  ALTRO_TEAM_ALL, 1.0);
 *                                           mask = (b % agents == a);  altro_solve_al(h) )
 * and afterwards the mask the handle had before the call is back.  Bit for bit the caller's own loop over the three calls;
 * returns the first status that is not ALTRO_OK (the caller's mask is put back then too).  The turn's mask is written on the
 * device and its size is known to the host; the radii go to the device once.  No blend factor: an agent that re-plans sees
 * plans that stay put while it does.  Seeding is the caller's job, as altro_team.h describes.
 * Refused as altro_team_solve refuses, with sweeps < 1 in place of rounds < 1: ALTRO_INVALID_ARG for agents < 2 or
 * B % agents != 0, an index that is no knot ALTRO_CON_CIRCLE with 3 (agents - 1) parameters, a NULL handle or radius, a
 * negative or non-finite radius; ALTRO_NOT_READY while an asynchronous solve owns the handle; ALTRO_HIP_ERROR without a
 * usable device; ALTRO_UNSUPPORTED on a handle that records the cost-to-go (see above). */
altro_status altro_team_solve_sequential(altro_handle h, int agents, int index, const double* radius, int radius_per_instance,
                                         int sweeps);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_SUBSET_H_ */
