// vsg_obs_args.h -- the observation lists of vsg_mappoints_refresh_from_observations (include/vsg_orb.h) as the caller
// gives them in host arrays: the check the entry point runs before it touches a device.  Host only and free of HIP:
// compiled into the library and, by tests/_obscore, into a CPU test core and a sanitized program.  The kernel indexes the
// keyframe table with obs_kf, a keyframe's descriptors and keypoints with obs_idx, the store with slots, a point's list
// with ref_pos and the scale table with the reference keypoint's octave: what obs_check accepts is all that reaches a
// device ("an out-of-range gather on a GPU is a fault, not a wrong answer").
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/vsg_orb.h"

namespace vsg {

enum { kObsMaxCandidates = 128 };  // the cap of vsg_distinctive_descriptors (k_distinctive's kDistinctMaxN)

// n points; point i = slot slots[i] with the observations [off[i], off[i + 1]) of kf / idx / bad (bad == nullptr: none is);
// ref_pos[i] = the position of mpRefKF's observation inside point i's list.  Keyframe k has kf_n[k] features whose
// keypoints (for the octaves) are kf_kps[k]; the store has `capacity` slots.
struct ObsView {
  int n;
  const int32_t *slots, *off, *kf, *idx;
  const uint8_t *bad;
  const int32_t *ref_pos;
  int n_kf;
  const int32_t *kf_n;
  const vsg_keypoint *const *kf_kps;
  int capacity, nlevels;
};

// VSG_OK when every rule holds:
//   off starts at 0 and never descends; every observation names a keyframe of [0, n_kf) and a feature of [0, kf_n[kf]);
//   every slot lies in [0, capacity) and is listed once (two workgroups would otherwise write one slot);
//   ref_pos[i] lies inside point i's list whenever that list is not empty (an empty list's ref_pos is not looked at);
//   the referenced keypoint's octave is < nlevels, and nlevels lies in [1, 16];
//   no point has more than kObsMaxCandidates observations that are not bad: VSG_ERR_UNSUPPORTED.
// Every other violation, a missing array included: VSG_ERR_INVALID (it wins over VSG_ERR_UNSUPPORTED, whatever the order
// of the points).  good (optional) gets the number of observations of every point that are not bad.  n == 0 is valid
// whatever the pointers are and nothing is dereferenced.
inline int obs_check(const ObsView &v, std::vector<int32_t> *good) {
  if (good) good->clear();
  if (v.n < 0 || v.n_kf < 0 || v.capacity < 0 || v.nlevels < 1 || v.nlevels > 16) return VSG_ERR_INVALID;
  if (v.n == 0) return VSG_OK;
  if (!v.slots || !v.off || v.off[0] != 0) return VSG_ERR_INVALID;
  for (int i = 0; i < v.n; i++)
    if (v.off[i + 1] < v.off[i]) return VSG_ERR_INVALID;
  const int total = v.off[v.n];
  if (total > 0 && (!v.kf || !v.idx || !v.ref_pos || !v.kf_n || !v.kf_kps)) return VSG_ERR_INVALID;
  for (int k = 0; k < total; k++) {
    if (v.kf[k] < 0 || v.kf[k] >= v.n_kf) return VSG_ERR_INVALID;
    if (v.idx[k] < 0 || v.idx[k] >= v.kf_n[v.kf[k]]) return VSG_ERR_INVALID;
  }
  std::vector<uint64_t> seen(((size_t)v.capacity + 63) / 64, 0);
  for (int i = 0; i < v.n; i++) {
    const int s = v.slots[i];
    if (s < 0 || s >= v.capacity) return VSG_ERR_INVALID;
    const uint64_t bit = (uint64_t)1 << (s & 63);
    if (seen[(size_t)s >> 6] & bit) return VSG_ERR_INVALID;
    seen[(size_t)s >> 6] |= bit;
  }
  bool too_many = false;
  if (good) good->resize((size_t)v.n);
  for (int i = 0; i < v.n; i++) {
    const int o = v.off[i], m = v.off[i + 1] - o;
    int g = m;
    if (v.bad) {
      g = 0;
      for (int j = 0; j < m; j++) g += v.bad[o + j] == 0;
    }
    if (good) (*good)[(size_t)i] = g;
    if (g > kObsMaxCandidates) too_many = true;
    if (m == 0) continue;
    const int r = v.ref_pos[i];
    if (r < 0 || r >= m) return VSG_ERR_INVALID;
    const vsg_keypoint *kps = v.kf_kps[v.kf[o + r]];
    if (!kps) return VSG_ERR_INVALID;
    const int oct = kps[v.idx[o + r]].octave;
    if (oct < 0 || oct >= v.nlevels) return VSG_ERR_INVALID;
  }
  return too_many ? VSG_ERR_UNSUPPORTED : VSG_OK;
}

}  // namespace vsg
