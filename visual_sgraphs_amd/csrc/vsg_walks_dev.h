// vsg_walks_dev.h -- the ordered passes walk::search_last and walk::search_local (vsg_walks.h, which stays the
// definition) in a form that a workgroup can run: k_track_walk (vsg_track.hip) on the device, tests/_walkcore on the host,
// from this one source.  Left / mono block only (nleft == -1).
//
// WHY A FIXED POINT.  In the serial pass query q sees a feature as blocked iff it was blocked on entry or an earlier query
// q' < q with mp_observed[q'] claimed it (a claim by an unobserved point leaves the feature open).  The dependence is
// triangular in q, so the pass is the unique fixed point of
//     claim[i]  = min { q : choice[q] == i, mp_observed[q] }        (-1: blocked on entry, INT_MAX: nobody)
//     choice[q] = the serial pass' scan of list q with "blocked(i) = claim[i] < q"
// Round 0 takes every choice against the entry flags alone; each round rebuilds claim[] from the choices (atomic min) and
// every query chooses again.  After round r the choices of queries 0 .. r-1 are the serial ones (induction on q), so
// nq + 1 rounds bound the loop; it ends at the first round in which no choice changed.  A pile-up of n observed queries
// on one list takes n rounds.
//
// AFTER THE WALK.  train_match[i] = the LAST claimant of i in query order (max), nmatches = number of claims; the
// rotation filter counts CLAIMS per bin (ORBmatcher.cc:1771-1777, :1855-1875) and every claim of a losing bin resets its
// feature whatever other claims the feature has; then the per-feature slot (the claimant's, or the caller's own) and the
// edge list of Optimizer.cc:1109-1180 in ascending feature order.
//
// A Team supplies the workgroup: each(n, f) runs f(i) for i in [0, n) and ends with a barrier; amin / amax / aadd are
// atomics on the team's scratch; compact(n, pred, emit) calls emit(i, position) for the i with pred(i) in ascending order
// and returns their number to everyone.  HostTeam below is the serial replay.
#pragma once
#include <stdint.h>

#include "vsg_walks.h"

namespace vsg {
namespace walkdev {

enum { kFormLast = 0, kFormLocal = 1 };
enum { kNone = 0x7FFFFFFF };  // claim[i]: nobody
enum { kStOverflow = 1, kStFewMatches = 2, kStFewEdges = 4 };
enum { kScratchInts = 40 };  // 30 bins, two `changed` flags, nmatches, three maxima, the overflow sum, one spare

struct Status {
  int32_t nmatches, n_edges, flags, rounds;
  int32_t overflow_sum;  // entries of the lists longer than `inline_len`: what the window kernel took from its counter
  int32_t bins[walk::HISTO_LENGTH];  // claims per rotation bin before the filter
  int32_t pad;
};

struct Args {
  int form, nq, nf;
  int inline_len, cap, list_total;  // lists: a list longer than inline_len lies in the overflow area of `cap` entries
  int check_orientation, min_matches;
  float nnratio;
  const uint32_t *ent;
  const int32_t *off, *cnt;
  const uint8_t *q_valid;     // local form: mbTrackInView (nullptr: every query)
  const uint8_t *observed;    // per query (nullptr: none)
  const uint8_t *blocked_in;  // per feature (nullptr: every feature is free)
  const void *q_angle, *t_angle;  // first angle of the queries' / features' keypoints
  int q_angle_stride, t_angle_stride;  // bytes between two of them
  const int32_t *q_slot;    // the slot of query q's map point (nullptr: none, the slot is -1)
  const int32_t *slots_in;  // the features' own slots on entry (nullptr: -1)
  const uint8_t *slot_observed;  // Observations() > 0 per slot of the store (nullptr: feat_observed is not written)
  int32_t *claim, *tm, *choice, *scratch;  // [nf], [nf], [nq], [kScratchInts]: LDS on the device
  int32_t *train_match;    // [nf] out: last claimant or -1
  uint8_t *train_blocked;  // [nf] out
  int32_t *feat_slots;     // [nf] out
  uint8_t *feat_observed;  // [nf] out: slot_observed of the feature's slot, 0 without one
  int32_t *edge_feat, *edge_slot;  // [nf] out, n_edges used
  Status *status, *status2;  // out (status2 may be nullptr: a second copy, for the host)
};

VSG_WALK_HD int e_idx(uint32_t e) { return (int)(e & 0x7FFFu); }
VSG_WALK_HD int e_dist(uint32_t e) { return (int)((e >> 15) & 0x1FFu); }
VSG_WALK_HD int e_oct(uint32_t e) { return (int)((e >> 24) & 0xFu); }
VSG_WALK_HD float angle_at(const void *base, int stride, int i) {
  return *(const float *)((const char *)base + (size_t)i * (size_t)stride);
}

// Is list q where the arguments say a list can be?  (A window kernel that was given a stale counter base could point
// anywhere; such a call ends as an overflow.)
VSG_WALK_HD bool list_ok(const Args &A, int q) {
  const int n = A.cnt[q], s = A.off[q];
  return n >= 0 && s >= 0 && (long long)s + n <= (long long)A.list_total;
}

// The scan of one query against the claims of earlier queries: the chosen feature or -1.
VSG_WALK_HD int choose(const Args &A, int q) {
  if (A.q_valid && !A.q_valid[q]) return -1;  // ORBmatcher.cc:50-51
  const int n = A.cnt[q];
  if (n <= 0) return -1;
  const uint32_t *e = A.ent + A.off[q];
  int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
  for (int c = 0; c < n; c++) {
    const uint32_t v = e[c];
    const int i2 = e_idx(v);
    if (i2 >= A.nf || A.claim[i2] < q) continue;  // blocked on entry (-1) or claimed by an earlier observed point
    const int d = e_dist(v);
    if (d < bestDist) {
      bestDist2 = bestDist, bestLevel2 = bestLevel;
      bestDist = d, bestLevel = e_oct(v), bestIdx = i2;
    } else if (d < bestDist2) {
      bestDist2 = d, bestLevel2 = e_oct(v);
    }
  }
  if (!(bestDist <= walk::TH_HIGH && bestIdx >= 0)) return -1;  // :1762 / :123
  if (A.form == kFormLocal &&
      !(bestLevel != bestLevel2 || (float)bestDist <= A.nnratio * (float)bestDist2))  // :125-128
    return -1;
  return bestIdx;
}

template <class Team>
VSG_WALK_HD void run(Team &T, const Args &A) {
  int32_t *const S = A.scratch;
  int32_t *const bins = S, *const changed = S + 30, *const nmatch = S + 32, *const ind = S + 33, *const ovf = S + 36,
                 *const bad = S + 37;
  T.each(kScratchInts, [&](int i) { S[i] = 0; });
  // what the window kernel's waves added to their counter, and whether every list lies inside the array
  // (after an overflow the segments that found no room start behind the array's end: they count all the same)
  T.each(A.nq, [&](int q) {
    if (!list_ok(A, q)) *bad = 1;
    if (A.cnt[q] > A.inline_len) T.aadd(ovf, A.cnt[q]);
  });
  Status st;
  st.nmatches = 0, st.n_edges = 0, st.flags = 0, st.rounds = 0, st.overflow_sum = *ovf, st.pad = 0;
  for (int b = 0; b < walk::HISTO_LENGTH; b++) st.bins[b] = 0;
  if (*bad || *ovf > A.cap) {  // the lists are not all there: nothing is walked, nothing is solved
    st.flags = kStOverflow;
    T.each(1, [&](int) {
      *A.status = st;
      if (A.status2) *A.status2 = st;
    });
    return;
  }
  auto init_claims = [&](int i) { A.claim[i] = (A.blocked_in && A.blocked_in[i]) ? -1 : (int)kNone; };
  T.each(A.nf, init_claims);
  T.each(A.nq, [&](int q) { A.choice[q] = choose(A, q); });
  int rounds = 0;
  for (;;) {
    const int flag = rounds & 1;
    rounds++;
    T.each(A.nf, [&](int i) {
      init_claims(i);
      if (i == 0) changed[flag] = 0;
    });
    T.each(A.nq, [&](int q) {
      if (A.choice[q] >= 0 && A.observed && A.observed[q]) T.amin(&A.claim[A.choice[q]], q);
    });
    T.each(A.nq, [&](int q) {
      const int c = choose(A, q);
      if (c != A.choice[q]) A.choice[q] = c, changed[flag] = 1;
    });
    if (A.nf == 0 || !changed[flag] || rounds > A.nq) break;
  }
  // the claims: last writer, count, rotation bins
  T.each(A.nf, [&](int i) { A.tm[i] = -1; });
  T.each(A.nq, [&](int q) {
    const int c = A.choice[q];
    if (c < 0) return;
    T.amax(&A.tm[c], q);
    T.aadd(nmatch, 1);
    if (A.check_orientation) {
      const int b = walk::rot_bin(angle_at(A.q_angle, A.q_angle_stride, q), angle_at(A.t_angle, A.t_angle_stride, c));
      if ((unsigned)b < (unsigned)walk::HISTO_LENGTH) T.aadd(&bins[b], 1);  // (the reference asserts this of its angles)
    }
  });
  for (int b = 0; b < walk::HISTO_LENGTH; b++) st.bins[b] = bins[b];
  if (A.check_orientation) {
    T.each(1, [&](int) {
      int i1 = -1, i2 = -1, i3 = -1;
      walk::three_maxima_of([&](int b) { return bins[b]; }, walk::HISTO_LENGTH, i1, i2, i3);
      ind[0] = i1, ind[1] = i2, ind[2] = i3;
    });
    T.each(A.nq, [&](int q) {
      const int c = A.choice[q];
      if (c < 0) return;
      const int b = walk::rot_bin(angle_at(A.q_angle, A.q_angle_stride, q), angle_at(A.t_angle, A.t_angle_stride, c));
      if (b == ind[0] || b == ind[1] || b == ind[2]) return;
      A.tm[c] = -1, A.claim[c] = (int)kNone;  // mvpMapPoints[i] = NULL: the feature is free again (:1869)
      T.aadd(nmatch, -1);
    });
  }
  // per feature: the match, the flag, the slot; then the edges in feature order
  T.each(A.nf, [&](int i) {
    const int m = A.tm[i];
    A.train_match[i] = m;
    A.train_blocked[i] = A.claim[i] != (int)kNone ? 1 : 0;
    const int slot = m >= 0 ? (A.q_slot ? A.q_slot[m] : -1) : (A.slots_in ? A.slots_in[i] : -1);
    A.feat_slots[i] = slot;
    if (A.slot_observed) A.feat_observed[i] = slot >= 0 ? A.slot_observed[slot] : 0;
    A.tm[i] = slot;
  });
  const int n_edges = T.compact(A.nf, [&](int i) { return A.tm[i] >= 0; },
                                [&](int i, int pos) { A.edge_feat[pos] = i, A.edge_slot[pos] = A.tm[i]; });
  st.nmatches = *nmatch, st.n_edges = n_edges, st.rounds = rounds;
  st.flags = (st.nmatches < A.min_matches ? kStFewMatches : 0) | (n_edges < 3 ? kStFewEdges : 0);
  T.each(1, [&](int) {
    *A.status = st;
    if (A.status2) *A.status2 = st;
  });
}

// the serial replay of a workgroup: every phase runs to its end before the next begins
struct HostTeam {
  template <class F>
  void each(int n, F f) {
    for (int i = 0; i < n; i++) f(i);
  }
  void amin(int32_t *p, int v) {
    if (v < *p) *p = v;
  }
  void amax(int32_t *p, int v) {
    if (v > *p) *p = v;
  }
  void aadd(int32_t *p, int v) { *p += v; }
  template <class P, class E>
  int compact(int n, P pred, E emit) {
    int pos = 0;
    for (int i = 0; i < n; i++)
      if (pred(i)) emit(i, pos++);
    return pos;
  }
};

}  // namespace walkdev
}  // namespace vsg
