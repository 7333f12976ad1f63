// trackstatscore.cpp as a program of its own for the AddressSanitizer + UBSan build (tests/test_track_stats.py): reads
// records from argv[1], runs each with every array a heap block of exactly its size, and writes the results to argv[2].
// Record: int32 head[4] = {nf, only_tracking, drop_outliers, 0}, then feat_slots[nf] (int32), outlier[nf], feat_observed[nf]
// (bytes, each padded to 4).  Output per record: int32 inliers, feat_slots[nf] after the loop, outlier[nf] as int32 (the
// loop must leave it alone).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int trackstats_case(int nf, int32_t *feat_slots, const uint8_t *outlier, const uint8_t *feat_observed,
                               int only_tracking, int drop_outliers);

template <class T>
static T *take(const uint8_t *&p, size_t count) {  // a heap block of exactly count elements
  T *a = new T[count ? count : 1];
  memcpy(a, p, count * sizeof(T));
  p += (count * sizeof(T) + 3) & ~(size_t)3;
  return a;
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> in;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) in.insert(in.end(), buf, buf + k);
  fclose(f);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  const uint8_t *p = in.data(), *end = p + in.size();
  while (p < end) {
    int32_t head[4];
    memcpy(head, p, sizeof(head));
    p += sizeof(head);
    const size_t nf = (size_t)head[0];
    int32_t *fs = take<int32_t>(p, nf);
    uint8_t *out = take<uint8_t>(p, nf), *obs = take<uint8_t>(p, nf);
    const int32_t inliers = trackstats_case((int)nf, fs, out, obs, head[1], head[2]);
    fwrite(&inliers, 4, 1, o), fwrite(fs, 4, nf, o);
    for (size_t i = 0; i < nf; i++) {
      const int32_t v = out[i];
      fwrite(&v, 4, 1, o);
    }
    delete[] fs, delete[] out, delete[] obs;
  }
  fclose(o);
  return 0;
}
