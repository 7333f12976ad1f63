/* vsg_orb_debug_local_ba.h -- test and measurement hook of vsg_mappoints_local_bundle_adjustment (csrc/vsg_local_ba.hip).
 * Like include/vsg_orb_debug.h it is NOT part of the drop-in boundary: nothing a maintainer of the reference binds.  It has
 * a header of its own because the hooks of vsg_orb_debug.h are a closed list (tests/test_abi.py names them one by one); the
 * symbol is exported by the same library so that the tests exercise the shipped code object. */
#ifndef VSG_ORB_DEBUG_LOCAL_BA_H
#define VSG_ORB_DEBUG_LOCAL_BA_H
#include "vsg_orb.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The number of Levenberg trial slots vsg_mappoints_local_bundle_adjustment enqueues ahead per iteration before it looks at
 * the solver's state record, for the CALLING THREAD's next calls (1 .. 10; 0 = the library's measured default).  The result
 * must not depend on it: every phase kernel decides from the device's record whether it runs.  VSG_ERR_INVALID outside
 * [0, 10]. */
int vsg_debug_local_ba_trial_slots(int slots);

#ifdef __cplusplus
}
#endif
#endif
