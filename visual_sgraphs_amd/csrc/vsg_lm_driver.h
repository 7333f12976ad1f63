// vsg_lm_driver.h -- the host's side of a device-resident Levenberg run (lba::State), ONE copy for vsg_local_ba.hip,
// vsg_sgraph_ba.hip, vsg_global_ba.hip and vsg_essential_graph.hip: how far ahead the host enqueues, when it looks at the
// controller's mirror in the pinned arena, when it stops, and what an error does.  The callers launch their own kernels from
// three callables; every kernel they launch reads the controller first and returns at once when its iteration or trial is not
// to run, so the result does not depend on this policy.
#pragma once
#include <hip/hip_runtime.h>

#include "vsg_local_ba.h"

namespace vsg {

namespace lm {

// Trial slots enqueued ahead per iteration before the host looks.  MEASURED on the local-BA leg of
// tools/resident_points_probe.py (profiles/local_ba_latency.json), medians of 200 calls with S = 1 / 2 / 10:
//   10 + 10 keyframes, 1500 points: 2559 / 2646 / 3357 us;  20 + 20, 3000: 3970 / 4036 / 4727;  40 + 40, 6000: 10526 /
//   10512 / 11181 (the resident call's own repeat gap: 2 / 12 / 1 us at S = 1).
// Those runs take one trial per iteration, so every slot past the first is a chain of launches that return at once; a
// rejected trial costs S = 1 one more look (a stream wait) instead.  1 is the best of the three, or level with 2, at every
// size.  Every call passes this; vsg_debug_local_ba_trial_slots alone passes another count.
enum { kTrialSlots = 1 };

// One call on stream st, whose inputs and set-up kernel are already enqueued.  linearise(it) enqueues iteration it up to
// its one-lane begin step, trial(it, q) the chain of trial q up to its one-lane decide step; both steps mirror the
// controller into *mirror.  slots trials are enqueued ahead of every look.  stop_flag may be null.  final() enqueues the
// kernel that writes the outs.  From the first enqueue on an error does not return at once: the arenas belong to the next
// call, so the stream is waited for first.  true: *S = the controller's record as the result reports it; false: VSG_ERR_HIP.
template <class Linearise, class Trial, class Final>
bool run(hipStream_t st, const lba::State *mirror, int iterations, int slots, const volatile uint8_t *stop_flag,
         Linearise linearise, Trial trial, Final final, lba::State *S) {
  bool failed = false, stopped = false;
  for (int it = 0; it < iterations && !failed; it++) {
    linearise(it);
    bool closed = false;
    for (int q = 0; q < lba::kTrials && !closed && !failed;) {
      for (int s = 0; s < slots && q < lba::kTrials; s++, q++) trial(it, q);
      // the look: the record in the pinned arena as the last one-lane step left it
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) failed = true;
      closed = failed || mirror->finished || !(mirror->iter == it && mirror->trial_open);
    }
    if (failed || mirror->finished) break;
    if (stop_flag && *stop_flag) {  // terminate() between iterations (sparse_optimizer.cpp:423)
      stopped = true;
      break;
    }
  }
  if (!failed) {
    final();
    if (hipGetLastError() != hipSuccess) failed = true;
  }
  if (hipStreamSynchronize(st) != hipSuccess || failed) return false;
  *S = *mirror;
  if (stopped) S->finished = 1, S->stop_reason = lba::kStopFlag;
  return true;
}

}  // namespace lm
}  // namespace vsg
