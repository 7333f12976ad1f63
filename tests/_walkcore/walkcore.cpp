// The host build of csrc/vsg_walks_dev.h beside csrc/vsg_walks.h behind a C interface (tests/test_walk_rounds.py through
// ctypes, walk_sanitized.cpp as a program of its own): one case is walked twice, by the serial definition
// (walk::search_last / walk::search_local) and by the round form that k_track_walk runs, and both results are handed back.
#include <cstring>
#include <vector>

#include "vsg_walks.h"
#include "vsg_walks_dev.h"

using namespace vsg;

extern "C" {

// form 0: search_last, 1: search_local (nleft == -1).  Lists as the window kernel writes them: off[q] = start, cnt[q] =
// length, n_ent entries in all.  ref_info = {nmatches, n_edges, overwrites, claims dropped by the filter, bins[30]};
// dev_info = {nmatches, n_edges, rounds, status flags, bins[30]}.  *_edges = feat[nf] then slot[nf].
void walkcore_case(int form, int nq, int nf, int n_ent, const uint32_t *ent, const int32_t *off, const int32_t *cnt,
                   const uint8_t *q_valid, const uint8_t *observed, const uint8_t *blocked_in, const float *q_angle,
                   const float *t_angle, const int32_t *q_slot, const int32_t *slots_in, int check_orientation,
                   float nnratio, int32_t *ref_tm, uint8_t *ref_tb, int32_t *ref_edges, int32_t *ref_info, int32_t *dev_tm,
                   uint8_t *dev_tb, int32_t *dev_edges, int32_t *dev_info) {
  // ---- the definition
  for (int i = 0; i < nf; i++) ref_tm[i] = -1, ref_tb[i] = blocked_in ? blocked_in[i] : 0;
  memset(ref_info, 0, 34 * sizeof(int32_t));
  walk::CandView cv;
  cv.ent = ent, cv.off = off, cv.cnt = cnt;
  int nm;
  if (form == walkdev::kFormLast) {
    std::vector<int> claims((size_t)(nf > 0 ? nf : 1), 0);
    int n_claims = 0;
    // t_angle is asked once per claim, right after train_match[i2] = q: the claim's bin and an overwrite are seen here
    auto angle_of = [&](int i2) {
      ref_info[4 + walk::rot_bin(q_angle[ref_tm[i2]], t_angle[i2])]++;
      if (claims[(size_t)i2]++) ref_info[2]++;
      n_claims++;
      return t_angle[i2];
    };
    nm = walk::search_last(cv, nq, -1, q_angle, observed, angle_of, walk::TH_HIGH, check_orientation != 0, ref_tb, ref_tm);
    if (check_orientation) ref_info[3] = n_claims - nm;
  } else {
    std::vector<uint8_t> all((size_t)(nq > 0 ? nq : 1), 1);
    nm = walk::search_local(cv, nq, -1, q_valid ? q_valid : all.data(), nullptr, nullptr, observed, nnratio, nullptr,
                            nullptr, ref_tb, ref_tm);
  }
  ref_info[0] = nm;
  int E = 0;  // the caller-side loop: train_match -> feat_slots -> the edges in feature order
  for (int i = 0; i < nf; i++) {
    const int slot = ref_tm[i] >= 0 ? (q_slot ? q_slot[ref_tm[i]] : -1) : (slots_in ? slots_in[i] : -1);
    if (slot >= 0) ref_edges[E] = i, ref_edges[nf + E] = slot, E++;
  }
  ref_info[1] = E;

  // ---- the round form, every array a block of exactly its size
  std::vector<int32_t> claim((size_t)nf), tm((size_t)nf), choice((size_t)nq), scratch(walkdev::kScratchInts),
      feat_slots((size_t)nf);
  walkdev::Status st;
  walkdev::Args A;
  memset(&A, 0, sizeof(A));
  A.form = form, A.nq = nq, A.nf = nf;
  A.inline_len = 16, A.cap = 0x7FFFFFFF, A.list_total = n_ent;
  A.check_orientation = form == walkdev::kFormLast ? check_orientation : 0, A.min_matches = 0, A.nnratio = nnratio;
  A.ent = ent, A.off = off, A.cnt = cnt, A.q_valid = form == walkdev::kFormLocal ? q_valid : nullptr;
  A.observed = observed, A.blocked_in = blocked_in;
  A.q_angle = q_angle, A.t_angle = t_angle, A.q_angle_stride = A.t_angle_stride = 4;
  A.q_slot = q_slot, A.slots_in = slots_in;
  A.claim = claim.data(), A.tm = tm.data(), A.choice = choice.data(), A.scratch = scratch.data();
  A.train_match = dev_tm, A.train_blocked = dev_tb, A.feat_slots = feat_slots.data();
  A.edge_feat = dev_edges, A.edge_slot = dev_edges + nf;
  A.status = &st, A.status2 = nullptr;
  walkdev::HostTeam T;
  walkdev::run(T, A);
  dev_info[0] = st.nmatches, dev_info[1] = st.n_edges, dev_info[2] = st.rounds, dev_info[3] = st.flags;
  for (int b = 0; b < 30; b++) dev_info[4 + b] = st.bins[b];
}

// The status of a call whose lists overflowed the candidate array: {flags, overflow_sum, nmatches}.  off / cnt as the
// window kernel leaves them then -- the segments that found no room start behind the array's end and were never written.
void walkcore_overflow(int nq, const int32_t *off, const int32_t *cnt, int cap, int list_total, int32_t *out) {
  std::vector<uint32_t> ent((size_t)(list_total > 0 ? list_total : 1), 0u);
  std::vector<int32_t> choice((size_t)nq), scratch(walkdev::kScratchInts);
  walkdev::Status st;
  walkdev::Args A;
  memset(&A, 0, sizeof(A));
  A.form = walkdev::kFormLast, A.nq = nq, A.nf = 0;
  A.inline_len = 16, A.cap = cap, A.list_total = list_total;
  A.ent = ent.data(), A.off = off, A.cnt = cnt;
  A.choice = choice.data(), A.scratch = scratch.data();
  A.status = &st;
  walkdev::HostTeam T;
  walkdev::run(T, A);
  out[0] = st.flags, out[1] = st.overflow_sum, out[2] = st.nmatches;
}
}
