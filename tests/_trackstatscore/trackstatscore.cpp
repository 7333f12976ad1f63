// csrc/vsg_track_stats.h behind a C interface (tests/test_track_stats.py through ctypes, stats_sanitized.cpp as a program
// of its own): the statistics loop of Tracking::TrackLocalMap over plain arrays.
#include "vsg_track_stats.h"

extern "C" int trackstats_case(int nf, int32_t *feat_slots, const uint8_t *outlier, const uint8_t *feat_observed,
                               int only_tracking, int drop_outliers) {
  return vsg::track_local_stats(nf, feat_slots, outlier, feat_observed, only_tracking, drop_outliers);
}
