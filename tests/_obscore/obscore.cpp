// Host build of MapPoint::UpdateNormalAndDepth for one point (visual_sgraphs_amd/csrc/vsg_observations.h) and of the
// argument check of vsg_mappoints_refresh_from_observations (csrc/vsg_obs_args.h), for tests/test_observations_hostmath.py,
// tests/test_observations_args.py and the sanitized program: the same source the library compiles.
#include <vector>

#include "vsg_obs_args.h"
#include "vsg_observations.h"

extern "C" {

// vsg::update_normal_and_depth for n points: point i is at P[3 i] and has the observations [off[i], off[i + 1]) of kf
// (index into Ow, 3 floats per keyframe); ref_pos[i] / ref_level[i] = the reference observation's position in the list
// and its keypoint's octave.  A point without observations keeps what normal / min_dist / max_dist hold.
void oc_update_normal_and_depth(int n, const float *P, const int32_t *off, const int32_t *kf, const float *Ow,
                                const int32_t *ref_pos, const int32_t *ref_level, const float *scale_factors, int nlevels,
                                float *normal, float *min_dist, float *max_dist) {
  for (int i = 0; i < n; i++) {
    const int m = off[i + 1] - off[i];
    if (m > 0)
      vsg::update_normal_and_depth(P + 3 * i, m, kf + off[i], Ow, ref_pos[i], ref_level[i], scale_factors, nlevels,
                                   normal + 3 * i, min_dist + i, max_dist + i);
  }
}

// vsg::obs_check.  Keyframe k has kf_n[k] features whose octaves follow one another in kf_oct; good (NULL: not wanted)
// gets every point's count of observations that are not bad when the check got that far.
int oc_obs_check(int n, const int32_t *slots, const int32_t *off, const int32_t *kf, const int32_t *idx, const uint8_t *bad,
                 const int32_t *ref_pos, int n_kf, const int32_t *kf_n, const int32_t *kf_oct, int capacity, int nlevels,
                 int32_t *good) {
  std::vector<std::vector<vsg_keypoint>> keys((size_t)(n_kf > 0 ? n_kf : 0));
  std::vector<const vsg_keypoint *> kps(keys.size());
  size_t at = 0;
  for (size_t k = 0; k < keys.size(); k++) {
    keys[k].resize((size_t)kf_n[k]);
    keys[k].shrink_to_fit();  // exactly kf_n[k] records: a sanitizer sees a step past the end
    for (auto &p : keys[k]) p = vsg_keypoint{0, 0, 0, 0, 0, kf_oct[at++], 0};
    kps[k] = keys[k].data();
  }
  const vsg::ObsView v = {n, slots, off, kf, idx, bad, ref_pos, n_kf, kf_n, kps.data(), capacity, nlevels};
  std::vector<int32_t> g;
  const int rc = vsg::obs_check(v, &g);
  if (good)
    for (size_t i = 0; i < g.size(); i++) good[i] = g[i];
  return rc;
}
}
