/* altro_knot_params.h -- constraints whose parameters change from knot to knot (a moving obstacle, a control bound that
 * tightens along the horizon, a waypoint per knot), on a batched handle of include/altro_hip.h.  Exported by libaltro_hip.so.
 *
 * The reference writes such a constraint as a loop, prob.SetConstraint(std::make_shared<CircleConstraint>(...), k) with a
 * different object on every knot (altro/problem/problem.hpp:66-133).  Here every distinct constraint list is a knot class and
 * a problem holds a few of them, so that loop does not fit altro_add_constraint; and nothing could move such parameters along
 * with a receding horizon.  A KNOT CONSTRAINT is one constraint for a whole range of knots: its parameters at knot k are a
 * row of a parameter TRACK that is uploaded once, windowed by an offset, and moved by altro_mpc_advance (include/altro_mpc.h). */
#ifndef ALTRO_KNOT_PARAMS_H_
#define ALTRO_KNOT_PARAMS_H_

#include "altro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A constraint of `kind` -- ALTRO_CON_GOAL, ALTRO_CON_CONTROL_BOUND, ALTRO_CON_CIRCLE, or ALTRO_CON_USER with `user_type`
 * (ignored otherwise) -- on knots k_begin <= k < k_end whose parameters at knot k are row min(offset + k, rows - 1) of its
 * track (altro_set_constraint_track).  nparams as altro_add_constraint takes it: n, 2m, 3 per circle, the user type's nparams.
 * Problem definition: before the first compute call.  It is ONE constraint, the next in registration order -- for
 * altro_num_constraints*, for the order of the rows on a knot, and for altro_mpc_row_map, so its duals and penalties travel
 * with an advance like any other constraint's -- and one entry in one knot class however many knots it covers.  *index (may be
 * NULL) receives the registration index, which the calls below take.  A knot control bound has all 2m rows on every knot: the
 * rows of a bound are chosen from its finite entries at problem definition (examples/basic_constraints.hpp:138-145), so every
 * entry of its track must be finite.  A handle with a knot constraint runs on the solver's general kernels, like one with a
 * tracking cost. */
altro_status altro_add_knot_constraint(altro_handle h, int kind, int user_type, int k_begin, int k_end, int nparams, int* index);

/* The track of knot constraint `index`: P[rows][nparams], [B][rows][nparams] with per_instance; rows >= 1.  The track belongs
 * to the trajectory side, like altro_set_reference: it may be set at any time between solves.  It leaves the window offset
 * alone (all tracks of a handle share it).  A solve, a cost evaluation or altro_mpc_track that meets a knot constraint without
 * a track returns ALTRO_NOT_READY.  Setting a track invalidates a cost-to-go replay as altro_set_trajectory does.
 * altro_set_constraint_track_device takes fp64 memory of the handle's device: nothing crosses to the host (so the entries of a
 * bound's track are the caller's responsibility there); like the other *_device calls it creates the device state, so the
 * problem definition must be complete. */
altro_status altro_set_constraint_track(altro_handle h, int index, const double* P, int rows, int per_instance);
altro_status altro_set_constraint_track_device(altro_handle h, int index, const void* P_device, int rows, int per_instance);

/* The window offset of ALL constraint tracks of the handle (offset >= 0; separate from altro_set_reference_offset).
 * altro_mpc_advance and everything built on it add their shift to it on a handle with a knot constraint (altro_mpc.h). */
altro_status altro_set_track_offset(altro_handle h, int offset);
altro_status altro_get_track_offset(altro_handle h, int* offset);

/* The parameters of knot constraint `index` as the kernels read them: out[B][k_end - k_begin][nparams]. */
altro_status altro_get_knot_params(altro_handle h, int index, double* out);

#ifdef __cplusplus
}
#endif

#endif  /* ALTRO_KNOT_PARAMS_H_ */
