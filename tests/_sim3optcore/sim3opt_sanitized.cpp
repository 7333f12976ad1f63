// sim3optcore.cpp as a program of its own for the AddressSanitizer + UBSan build (tests/test_sanitizers_sim3opt.py): reads
// records from argv[1], runs each through sim3optcore_run with every array a heap block of exactly its size, and writes
// the results to argv[2].  Record: int32 head[12] = {n1, n2, cap1, cap2, nlevels, fix_scale, all_points, shared, null_slots,
// 0, 0, 0}, then slots1[n1], slots2[n1], idx2[n1], level2[n1], pos1[3 cap1], pos2[3 cap2] (absent when shared), k1x[n1],
// k1y[n1], oct1[n1], k2x[n2], k2y[n2], oct2[n2], pose1[16] (Rcw, tcw, fx, fy, cx, cy), pose2[16], sig1[nlevels],
// sig2[nlevels], th2 (one float), S12 (8 doubles).  Output per record: int32 rc, the 7 counters, state[n1] as int32,
// chi2[2 n1], S12 (8 doubles).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vsg_orb.h"

extern "C" int sim3optcore_run(int n1, int n2, const int32_t *slots1, const int32_t *slots2, const int32_t *idx2,
                               const int32_t *level2, int cap1, int cap2, const float *pos1, const float *pos2,
                               const float *k1x, const float *k1y, const int32_t *oct1, const float *k2x, const float *k2y,
                               const int32_t *oct2, const vsg_frame_pose *pose1, const vsg_frame_pose *pose2,
                               const float *sig1, const float *sig2, int nlevels, const vsg_sim3d *S12, float th2,
                               int fix_scale, int all_points, uint8_t *state, double *chi2, vsg_sim3_opt_result *res);

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

static vsg_frame_pose *pose_of(const float *p) {
  vsg_frame_pose *o = new vsg_frame_pose;
  memset(o, 0, sizeof *o);
  memcpy(o->Rcw, p, 36), memcpy(o->tcw, p + 9, 12);
  o->fx = p[12], o->fy = p[13], o->cx = p[14], o->cy = p[15];
  return o;
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
    int32_t head[12];
    memcpy(head, p, sizeof(head));
    p += sizeof(head);
    const size_t n1 = (size_t)head[0], n2 = (size_t)head[1], cap1 = (size_t)head[2], cap2 = (size_t)head[3];
    const size_t nl = (size_t)(head[4] < 0 ? 0 : head[4] > 16 ? 16 : head[4]);
    int32_t *slots1 = take<int32_t>(p, n1), *slots2 = take<int32_t>(p, n1), *idx2 = take<int32_t>(p, n1),
            *level2 = take<int32_t>(p, n1);
    float *pos1 = take<float>(p, 3 * cap1), *pos2 = head[7] ? pos1 : take<float>(p, 3 * cap2);
    float *k1x = take<float>(p, n1), *k1y = take<float>(p, n1);
    int32_t *oct1 = take<int32_t>(p, n1);
    float *k2x = take<float>(p, n2), *k2y = take<float>(p, n2);
    int32_t *oct2 = take<int32_t>(p, n2);
    float *p1 = take<float>(p, 16), *p2 = take<float>(p, 16), *sig1 = take<float>(p, nl), *sig2 = take<float>(p, nl);
    float *th2 = take<float>(p, 1);
    double *S = take<double>(p, 8);
    vsg_frame_pose *pose1 = pose_of(p1), *pose2 = pose_of(p2);
    vsg_sim3d *S12 = new vsg_sim3d;
    memcpy(S12->q, S, 32), memcpy(S12->t, S + 4, 24), S12->s = S[7];
    uint8_t *state = new uint8_t[n1 ? n1 : 1];
    double *chi2 = new double[2 * (n1 ? n1 : 1)];
    memset(state, 9, n1 ? n1 : 1);
    for (size_t i = 0; i < 2 * n1; i++) chi2[i] = -1.0;
    vsg_sim3_opt_result *res = new vsg_sim3_opt_result;
    memset(res, 0, sizeof *res);
    const int32_t rc = sim3optcore_run((int)n1, (int)n2, head[8] ? nullptr : slots1, slots2, idx2, level2, (int)cap1, (int)cap2,
                                       pos1, pos2, k1x, k1y, oct1, k2x, k2y, oct2, pose1, pose2, sig1, sig2, head[4], S12, *th2,
                                       head[5], head[6], state, chi2, res);
    const int32_t cnt[7] = {res->n_correspondences, res->n_bad, res->n_in, res->n_in_kf2, res->n_out_kf2,
                            res->more_iterations, res->updated};
    fwrite(&rc, 4, 1, o), fwrite(cnt, 4, 7, o);
    for (size_t i = 0; i < n1; i++) {
      const int32_t v = state[i];
      fwrite(&v, 4, 1, o);
    }
    fwrite(chi2, 8, 2 * n1, o), fwrite(&res->S12, 8, 8, o);
    delete[] slots1, delete[] slots2, delete[] idx2, delete[] level2, delete[] pos1;
    if (!head[7]) delete[] pos2;
    delete[] k1x, delete[] k1y, delete[] oct1, delete[] k2x, delete[] k2y, delete[] oct2, delete[] p1, delete[] p2;
    delete[] sig1, delete[] sig2, delete[] th2, delete[] S, delete[] state, delete[] chi2;
    delete pose1, delete pose2, delete S12, delete res;
  }
  fclose(o);
  return 0;
}
