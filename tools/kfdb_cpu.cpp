// kfdb_cpu.cpp -- the CPU side of tools/kfdb_latency.py: KeyFrameDatabase as the reference builds it
// (KeyFrameDatabase.cc:36-42, 592-830), restated from scratch on std::list posting lists, std::map BowVectors and the
// L1 merge-loop score (ScoringObject.cpp), timed on the same workload the device database gets.
//
// usage: kfdb_cpu <workload.bin>
//   workload: int32 n_kf, n_query, words, nwords, n_warm; then n_kf + n_query + n_warm BowVectors of `words` (uint32 ids,
//   float64 values).  Warm-up w (untimed, before the timed queries, as the device side runs it): relocalisation with id
//   3 * 10^6 + w and N-best with id 4 * 10^6 + w, both on BowVector n_kf + n_query + w (the queries change the state)
//   keyframe k (id k + 1, map 0) has covisibility neighbours k+1, k-1, k+2, k-2, ... (5 each side); query q of each kind
//   uses id 10^6 + q (relocalisation) / 2 * 10^6 + q (N-best, keyframe (q * 7919) % n_kf + 1, 3 candidates).
// Prints one JSON line: per-add and per-query means (ms) and a checksum of every candidate list.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <list>
#include <map>
#include <set>
#include <vector>

typedef std::map<unsigned, double> BowVector;

struct KF {
  uint64_t mnId = 0;
  int map = 0;
  BowVector bow;
  std::vector<KF *> covis;
  uint64_t mnRelocQuery = 0, mnPlaceRecognitionQuery = 0;
  int mnRelocWords = 0, mnPlaceRecognitionWords = 0;
  float mRelocScore = 0, mPlaceRecognitionScore = 0;
};

static double l1_score(const BowVector &v1, const BowVector &v2) {
  auto a = v1.begin(), b = v2.begin();
  double s = 0;
  while (a != v1.end() && b != v2.end()) {
    if (a->first == b->first) {
      s += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second);
      ++a, ++b;
    } else if (a->first < b->first) {
      a = v1.lower_bound(b->first);
    } else {
      b = v2.lower_bound(a->first);
    }
  }
  return -s / 2.0;
}

struct DB {
  std::vector<std::list<KF *>> inv;
  explicit DB(int nwords) : inv(nwords) {}
  void add(KF *k) {
    for (auto &w : k->bow) inv[w.first].push_back(k);
  }

  std::vector<KF *> reloc(uint64_t qid, const BowVector &q, int map) {
    std::list<KF *> sharing;
    for (auto &w : q)
      for (KF *k : inv[w.first]) {
        if (k->mnRelocQuery != qid) k->mnRelocWords = 0, k->mnRelocQuery = qid, sharing.push_back(k);
        k->mnRelocWords++;
      }
    if (sharing.empty()) return {};
    int maxw = 0;
    for (KF *k : sharing) maxw = std::max(maxw, k->mnRelocWords);
    const int minw = maxw * 0.8f;
    std::list<std::pair<float, KF *>> scored;
    for (KF *k : sharing)
      if (k->mnRelocWords > minw) {
        const float si = l1_score(q, k->bow);
        k->mRelocScore = si;
        scored.push_back({si, k});
      }
    if (scored.empty()) return {};
    std::list<std::pair<float, KF *>> acc;
    float best_acc = 0;
    for (auto &p : scored) {
      float bs = p.first, a = bs;
      KF *best = p.second;
      for (KF *k2 : p.second->covis) {
        if (k2->mnRelocQuery != qid) continue;
        a += k2->mRelocScore;
        if (k2->mRelocScore > bs) best = k2, bs = k2->mRelocScore;
      }
      acc.push_back({a, best});
      if (a > best_acc) best_acc = a;
    }
    const float min_keep = 0.75f * best_acc;
    std::set<KF *> added;
    std::vector<KF *> out;
    for (auto &p : acc)
      if (p.first > min_keep) {
        if (p.second->map != map) continue;
        if (added.insert(p.second).second) out.push_back(p.second);
      }
    return out;
  }

  void nbest(KF *qk, const std::set<KF *> &conn, std::vector<KF *> &loop, std::vector<KF *> &merge, size_t n) {
    const uint64_t qid = qk->mnId;
    std::list<KF *> sharing;
    for (auto &w : qk->bow)
      for (KF *k : inv[w.first]) {
        if (k->mnPlaceRecognitionQuery != qid) {
          k->mnPlaceRecognitionWords = 0;
          if (!conn.count(k)) k->mnPlaceRecognitionQuery = qid, sharing.push_back(k);
        }
        k->mnPlaceRecognitionWords++;
      }
    if (sharing.empty()) return;
    int maxw = 0;
    for (KF *k : sharing) maxw = std::max(maxw, k->mnPlaceRecognitionWords);
    const int minw = maxw * 0.8f;
    std::list<std::pair<float, KF *>> scored;
    for (KF *k : sharing)
      if (k->mnPlaceRecognitionWords > minw) {
        const float si = l1_score(qk->bow, k->bow);
        k->mPlaceRecognitionScore = si;
        scored.push_back({si, k});
      }
    if (scored.empty()) return;
    std::list<std::pair<float, KF *>> acc;
    for (auto &p : scored) {
      float bs = p.first, a = bs;
      KF *best = p.second;
      for (KF *k2 : p.second->covis) {
        if (k2->mnPlaceRecognitionQuery != qid) continue;
        a += k2->mPlaceRecognitionScore;
        if (k2->mPlaceRecognitionScore > bs) best = k2, bs = k2->mPlaceRecognitionScore;
      }
      acc.push_back({a, best});
    }
    acc.sort([](const std::pair<float, KF *> &a, const std::pair<float, KF *> &b) { return a.first > b.first; });
    std::set<KF *> added;
    size_t i = 0;
    for (auto it = acc.begin(); i < acc.size() && (loop.size() < n || merge.size() < n); ++i, ++it) {
      KF *k = it->second;
      if (added.count(k)) continue;
      if (qk->map == k->map && loop.size() < n) loop.push_back(k);
      else if (qk->map != k->map && merge.size() < n) merge.push_back(k);
      added.insert(k);
    }
  }
};

static double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hdr[5];
  if (fread(hdr, 4, 5, f) != 5) return 2;
  const int nkf = hdr[0], nq = hdr[1], words = hdr[2], nwords = hdr[3], nwarm = hdr[4];
  std::vector<BowVector> bows(nkf + nq + nwarm);
  std::vector<uint32_t> ids(words);
  std::vector<double> vals(words);
  for (auto &b : bows) {
    if (fread(ids.data(), 4, words, f) != (size_t)words || fread(vals.data(), 8, words, f) != (size_t)words) return 2;
    for (int j = 0; j < words; j++) b.emplace_hint(b.end(), ids[j], vals[j]);
  }
  fclose(f);
  std::vector<KF> kfs(nkf);
  for (int k = 0; k < nkf; k++) kfs[k].mnId = k + 1, kfs[k].bow = bows[k];
  for (int k = 0; k < nkf; k++)
    for (int d = 1; d <= 5; d++)
      for (int u : {k + d, k - d})
        if (u >= 0 && u < nkf) kfs[k].covis.push_back(&kfs[u]);
  DB db(nwords);
  double t0 = now_ms();
  for (auto &k : kfs) db.add(&k);
  const double add_ms = (now_ms() - t0) / nkf;
  for (int w = 0; w < nwarm; w++) {
    db.reloc(3000000 + w, bows[nkf + nq + w], 0);
    KF qk;  // a keyframe outside the database
    qk.mnId = 4000000 + w, qk.bow = bows[nkf + nq + w];
    std::vector<KF *> loop, merge;
    db.nbest(&qk, std::set<KF *>(), loop, merge, 3);
  }
  uint64_t sum_r = 0, sum_n = 0;
  t0 = now_ms();
  for (int q = 0; q < nq; q++) {
    const BowVector &b = (q % 2) ? bows[nkf + q] : kfs[(q * 7919) % nkf].bow;
    auto out = db.reloc(1000000 + q, b, 0);
    for (size_t i = 0; i < out.size(); i++) sum_r += out[i]->mnId * (i + 1) * (q + 1);
  }
  const double reloc_ms = (now_ms() - t0) / nq;
  t0 = now_ms();
  for (int q = 0; q < nq; q++) {
    KF &qk = kfs[(q * 7919) % nkf];
    const uint64_t saved = qk.mnId;
    qk.mnId = 2000000 + q;  // the query keyframe's id for this query (mnId is what the state compares against)
    std::set<KF *> conn(qk.covis.begin(), qk.covis.end());
    std::vector<KF *> loop, merge;
    db.nbest(&qk, conn, loop, merge, 3);
    qk.mnId = saved;
    for (size_t i = 0; i < loop.size(); i++) sum_n += loop[i]->mnId * (i + 1) * (q + 1);
  }
  const double nbest_ms = (now_ms() - t0) / nq;
  printf("{\"n_kf\": %d, \"words\": %d, \"queries\": %d, \"add_ms\": %.6f, \"reloc_ms\": %.4f, \"nbest_ms\": %.4f, "
         "\"reloc_checksum\": %llu, \"nbest_checksum\": %llu}\n",
         nkf, words, nq, add_ms, reloc_ms, nbest_ms, (unsigned long long)sum_r, (unsigned long long)sum_n);
  return 0;
}
