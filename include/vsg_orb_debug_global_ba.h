/* vsg_orb_debug_global_ba.h -- test and measurement hooks of vsg_mappoints_global_bundle_adjustment
 * (csrc/vsg_global_ba.hip).  Like include/vsg_orb_debug_local_ba.h it is NOT part of the drop-in boundary; the symbols are
 * exported by the same library so that the tests exercise the shipped code object. */
#ifndef VSG_ORB_DEBUG_GLOBAL_BA_H
#define VSG_ORB_DEBUG_GLOBAL_BA_H
#include "vsg_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reduced solve of the global call on a caller's system, on the calling thread's current device: M = n x n doubles
 * row-major of which the LOWER triangle is read (M is not written), b = the right-hand side, x = the n solutions, *ok = 0
 * when a pivot was <= 0 (x is then whatever the sweep gave).  The same chain of kernels, enqueued by the same function, as
 * inside the call.  VSG_ERR_INVALID: n outside [1, 6 * 512] or a NULL pointer, before a device is touched. */
int vsg_debug_ba_reduced_solve(int n, const double *M, const double *b, double *x, int *ok);

/* The solver's constants in force: columns per panel, rows / columns per tile of the trailing update. */
int vsg_debug_ba_solver_geometry(int *panel, int *tile);

#ifdef __cplusplus
}
#endif
#endif
