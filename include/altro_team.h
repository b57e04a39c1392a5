/* altro_team.h -- teams of agents that avoid each other's plans, on a batched handle of include/altro_hip.h.  Exported by
 * libaltro_hip.so.
 *
 * A handle of B = T * A instances holds T TEAMS of A >= 2 AGENTS each: agent a of team t is instance t * A + a, so the
 * agents of a team are adjacent columns.  For every agent each team-mate is a moving circle whose track is the team-mate's
 * current plan (distributed MPC by plan exchange, or prioritised planning).  The caller registers ONE knot constraint
 * (include/altro_knot_params.h),
 *     altro_add_knot_constraint(h, ALTRO_CON_CIRCLE, 0, k_begin, k_end, 3 * (A - 1), &index),
 * and the calls below fill its track on the device from the plans the handle holds: circle slot i of agent a is peer
 * j = i < a ? i : i + 1 (the peers in ascending order, the agent itself skipped).  A position is (x[0], x[1]), the states the
 * built-in circle reads.  Every call takes agents = A and is stateless in its grouping: nothing of it is stored on the handle.
 * The compiled problem sets no limit on the rows of one knot (only on the constraints of a knot, 4, and on the knot
 * constraints of a handle, 16), so no team size is refused beside a control bound; the tests go up to A = 5, the timing
 * script to A = 8.
 *
 * SEEDING IS THE CALLER'S JOB.  Before any solve the plans may be zeros.  Give the team constraint a shared one-row track
 * whose circles all have radius 0 (never active: c = -d^2 <= 0), solve once -- the uncoupled plans -- and fill from then on.
 *
 * PLAIN SIMULTANEOUS EXCHANGE OSCILLATES: with ALTRO_TEAM_ALL and blend = 1 two agents both dodge, then both see that the other
 * has dodged and go straight again, with period 2 for ever.  Two remedies converge: a damped exchange (ALTRO_TEAM_ALL with
 * blend = 0.5), or priorities (ALTRO_TEAM_PRIORITY: agent a avoids only agents j < a; A rounds settle a team).
 *
 * Refused before any device work with ALTRO_INVALID_ARG: agents < 2 or B % agents != 0; an index that is no knot
 * constraint, no ALTRO_CON_CIRCLE, or whose nparams is not 3 (A - 1); a mode other than the two below; blend outside (0, 1] or
 * not finite; rounds < 1; cycles < 1; a NULL handle, radius or (clearance) output; a negative or non-finite radius.  An
 * asynchronous solve in flight: ALTRO_NOT_READY.  No usable device: ALTRO_HIP_ERROR -- there is no CPU fallback. */
#ifndef ALTRO_TEAM_H_
#define ALTRO_TEAM_H_

#include "altro_hip.h"
#include "altro_knot_params.h"
#include "altro_mpc.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ALTRO_TEAM_ALL = 0, ALTRO_TEAM_PRIORITY = 1 };

/* Makes the track of knot constraint `index` per-instance with N + 1 rows; row r describes the peers at knot r of the horizon
 * as it stands now: for instance t * A + a and slot i (peer j) the centre is X_j[r][0], X_j[r][1] -- X as altro_get_trajectory
 * returns it at this moment -- and the radius is radius[a] + radius[j], one fp64 addition (radius is [A], or [B] with
 * radius_per_instance).  Under ALTRO_TEAM_PRIORITY the slots of peers j > a get the peer's centre and RADIUS 0.
 * blend == 1, or a track that was not last written by this call: the centres are bit copies.  Otherwise
 * centre = old + blend * (new - old), each operation rounded on its own, old = the track as the window shows it now (row
 * min(max(offset - base, 0) + r, N)); radii are written fresh, never blended.
 * THE WINDOW.  All tracks of a handle share one window offset (altro_set_track_offset), and this call leaves it alone; it
 * records the offset at which it wrote the track as the track's BASE, and knot k of this constraint reads row
 * min(max(offset - base, 0) + k, N).  After altro_mpc_advance by s the team's window therefore shows the peers' former plans
 * at knot k + s -- what the peers' advanced plans are, up to the held tail -- while real moving obstacles on the same handle
 * (base 0) move as before.  altro_set_constraint_track* puts the base back to 0.
 * Invalidates a cost-to-go replay as altro_set_constraint_track does; X, U, duals and statistics are untouched.  Returns when
 * the work on the handle's stream is done. */
altro_status altro_team_fill_tracks(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, int mode,
                                    double blend);

/* clear[T]: per team the minimum over knots k in [k_begin, k_end) of the constraint and over pairs a < j of
 * (dx * dx + dy * dy) - R * R, R = radius[a] + radius[j], in exactly this association without contraction; negative exactly
 * when two agents' plans overlap.  Every pair counts whatever the mode; a NaN position gives NaN.  Changes nothing on the
 * handle.  The _device form takes fp64 memory of the handle's device and returns when the stream is done. */
altro_status altro_team_clearance(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, double* clear);
altro_status altro_team_clearance_device(altro_handle h, int agents, int index, const double* radius, int radius_per_instance,
                                         void* clear_device);

/* rounds x (altro_team_fill_tracks; altro_solve_al) -- bit for bit the caller's own loop; returns the first status that is not
 * ALTRO_OK.  Warm starts are the caller's options (reset_duals, initial_penalty), as everywhere else. */
altro_status altro_team_solve(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, int mode,
                              double blend, int rounds);

/* cycles x (altro_team_solve of `rounds`; the clearance into a device log; altro_mpc_advance by `shift` with x0 = the plan and
 * w[c]) -- bit for bit the caller's own loop.  w (host [cycles][B][n] or NULL) and radius go to the device once; X_cl, U_cl,
 * iterations, status as altro_mpc_run gives them (iterations and status of the LAST round's solve of a cycle) and
 * clear[T][cycles] come back once; nothing crosses to the host inside the loop.  Each output may be NULL.  Refuses what
 * altro_mpc_advance refuses. */
altro_status altro_mpc_run_team(altro_handle h, int agents, int index, const double* radius, int radius_per_instance, int mode,
                                double blend, int rounds, int cycles, int shift, const double* w, double* X_cl, double* U_cl,
                                int* iterations, int* status, double* clear);

#ifdef __cplusplus
}
#endif
#endif /* ALTRO_TEAM_H_ */
