// vsg_track_stats.h -- the statistics loop that ends Tracking::TrackLocalMap (Tracking.cc:3074-3095) as a plain function
// over arrays: vsg_frame_track_local_map (vsg_track.hip) runs it on what it read back after its one wait, and
// tests/_trackstatscore builds it without a device.
#pragma once
#include <stdint.h>

namespace vsg {

// feat_slots[i] = the slot of mvpMapPoints[i] (< 0: none), outlier[i] = mvbOutlier[i], feat_observed[i] != 0 =
// mvpMapPoints[i]->Observations() > 0 (read for features with a slot only).  Returns mnMatchesInliers: the features with a
// slot that are no outlier and, unless only_tracking (mbOnlyTracking, :3084-3090), whose point is observed.  drop_outliers
// (mSensor == System::STEREO, :3092-3093): an outlier's slot becomes -1; its flag stays as it is.  IncreaseFound (:3083) is
// the caller's: it is due for every feature that ends with a slot and no outlier flag.
inline int track_local_stats(int nf, int32_t *feat_slots, const uint8_t *outlier, const uint8_t *feat_observed,
                             int only_tracking, int drop_outliers) {
  int inliers = 0;
  for (int i = 0; i < nf; i++) {
    if (feat_slots[i] < 0) continue;
    if (!outlier[i]) {
      if (only_tracking || feat_observed[i]) inliers++;
    } else if (drop_outliers) {
      feat_slots[i] = -1;
    }
  }
  return inliers;
}

}  // namespace vsg
