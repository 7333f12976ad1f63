// posecore.cpp as a program of its own for the AddressSanitizer + UBSan build (tests/test_sanitizers_pose.py): reads
// records from argv[1], runs each through posecore_run with every array a heap block of exactly its size, and writes the
// results to argv[2].  Record: int32 head[8] = {n, capacity, nlevels, hold_round, has_uright, has_removed, null_slots, 0},
// then feat_slots[n], world_pos[3 capacity], kx[n], ky[n], octave[n], u_right[n]?, pose7, cam5, inv_sigma2[nlevels],
// removed[n]? (bytes, padded to 4).  Output per record: int32 rc, res_i[4], outlier[n] as int32, chi2[n], res_qt[7].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int posecore_run(int n, const int32_t *feat_slots, int capacity, const float *world_pos, const float *kx,
                            const float *ky, const int32_t *octave, const float *u_right, const float *pose7,
                            const float *cam5, const float *inv_level_sigma2, int nlevels, int hold_round,
                            const uint8_t *removed, uint8_t *outlier, float *chi2, double *res_qt, int32_t *res_i,
                            double *held_qt);

template <class T>
static T *take(const uint8_t *&p, size_t count) {  // a heap block of exactly count elements
  T *a = new T[count ? count : 1];
  memcpy(a, p, count * sizeof(T));
  p += (count * sizeof(T) + 3) & ~(size_t)3;
  if (!count) {
    delete[] a;
    return nullptr;
  }
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
    int32_t head[8];
    memcpy(head, p, sizeof(head));
    p += sizeof(head);
    const size_t n = (size_t)head[0], cap = (size_t)head[1], nl = (size_t)head[2];
    int32_t *slots = take<int32_t>(p, n);
    float *pos = take<float>(p, 3 * cap), *kx = take<float>(p, n), *ky = take<float>(p, n);
    int32_t *oct = take<int32_t>(p, n);
    float *ur = head[4] ? take<float>(p, n) : nullptr;
    float *pose7 = take<float>(p, 7), *cam5 = take<float>(p, 5), *sig = take<float>(p, nl > 16 ? 16 : nl);
    uint8_t *rem = head[5] ? take<uint8_t>(p, n) : nullptr;
    uint8_t *outlier = new uint8_t[n ? n : 1];
    float *chi2 = new float[n ? n : 1];
    memset(outlier, 7, n ? n : 1);
    for (size_t i = 0; i < n; i++) chi2[i] = -1.0f;
    double qt[7] = {0, 0, 0, 0, 0, 0, 0};
    int32_t ri[4] = {0, 0, 0, 0};
    const int32_t rc = posecore_run((int)n, head[6] ? nullptr : slots, (int)cap, pos, kx, ky, oct, ur, pose7, cam5, sig,
                                    (int)nl, head[3], rem, outlier, chi2, qt, ri, nullptr);
    fwrite(&rc, 4, 1, o), fwrite(ri, 4, 4, o);
    for (size_t i = 0; i < n; i++) {
      const int32_t v = outlier[i];
      fwrite(&v, 4, 1, o);
    }
    fwrite(chi2, 4, n, o), fwrite(qt, 8, 7, o);
    delete[] slots, delete[] pos, delete[] kx, delete[] ky, delete[] oct, delete[] ur, delete[] pose7, delete[] cam5;
    delete[] sig, delete[] rem, delete[] outlier, delete[] chi2;
  }
  fclose(o);
  return 0;
}
