// The host build of csrc/vsg_global_ba.h (gbacore.cpp) as a program of its own for AddressSanitizer + UBSan
// (tests/test_sanitizers_gba.py): reads records from a file, copies every array into a heap block of exactly its size, runs
// gbacore_run and appends the return code, res and every out to a second file.
//   record: int32 head[14] = {capacity, P, n_obs (length of obs_kf / obs_idx), K, nlevels, iterations, stop flag (-1: NULL),
//           mask of NULL arguments, features in all keyframes, length of obs_off, E of the outs, robust, write_store, 0}, then
//           store_pos[3 capacity], slots[P], obs_off, obs_kf, obs_idx, kf_off[K + 1], kx, ky, octave, u_right, nleft[K],
//           Tcw[7 K], fixed[K], cam[5 K], sigma[clamp(nlevels, 0, 16)]
//   usage: gba_sanitized <in.bin> <out.bin>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>

#include "../../include/vsg_orb.h"

extern "C" int gbacore_run(int capacity, float *store_pos, int n_points, const int32_t *slots, const int32_t *obs_off,
                           const int32_t *obs_kf, const int32_t *obs_idx, int n_kf, const int32_t *kf_off, const float *kx,
                           const float *ky, const int32_t *oct, const float *ur, const int32_t *nleft, const vsg_pose_se3 *kf_Tcw,
                           const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam, const float *inv_level_sigma2, int nlevels,
                           int iterations, int robust, int write_store, const volatile uint8_t *stop_flag,
                           vsg_pose_se3d *kf_Tcw_out, float *world_pos_out, uint8_t *included, double *chi2,
                           vsg_global_ba_result *res);

template <class T>
static std::unique_ptr<T[]> block(std::ifstream &f, size_t n) {
  std::unique_ptr<T[]> p(new T[n]);
  if (n) f.read((char *)p.get(), (std::streamsize)(sizeof(T) * n));
  return p;
}
template <class T>
static std::unique_ptr<T[]> filled(size_t n, T v) {
  std::unique_ptr<T[]> p(new T[n]);
  for (size_t i = 0; i < n; i++) p[i] = v;
  return p;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  std::ifstream in(argv[1], std::ios::binary);
  std::ofstream out(argv[2], std::ios::binary);
  if (!in || !out) return 2;
  int records = 0;
  for (;;) {
    int32_t h[14];
    in.read((char *)h, sizeof(h));
    if (!in) break;
    const size_t cap = (size_t)h[0], P = (size_t)h[1], nobs = (size_t)h[2], K = (size_t)h[3], nfeat = (size_t)h[8], noff = (size_t)h[9],
                 E = (size_t)h[10];
    const int nl = h[4] < 0 ? 0 : h[4] > 16 ? 16 : h[4], mask = h[7];
    auto pos = block<float>(in, 3 * cap);
    auto slots = block<int32_t>(in, P), off = block<int32_t>(in, noff), kf = block<int32_t>(in, nobs), idx = block<int32_t>(in, nobs);
    auto kf_off = block<int32_t>(in, K + 1);
    auto kx = block<float>(in, nfeat), ky = block<float>(in, nfeat);
    auto oct = block<int32_t>(in, nfeat);
    auto ur = block<float>(in, nfeat);
    auto nleft = block<int32_t>(in, K);
    auto Tcw = block<vsg_pose_se3>(in, K);
    auto fixed = block<uint8_t>(in, K);
    auto cam = block<vsg_ba_camera>(in, K);
    auto sig = block<float>(in, (size_t)nl);
    if (!in) return 2;
    auto kf_out = filled<double>(7 * K, -7.0);
    auto pos_out = filled<float>(3 * P, -7.0f);
    auto included = filled<uint8_t>(P, 9);
    auto chi2 = filled<double>(E, -7.0);
    vsg_global_ba_result res;
    memset(&res, 0x5A, sizeof(res));
    uint8_t flag = (uint8_t)(h[6] > 0);
    auto arg = [mask](int bit, auto *p) { return (mask >> bit) & 1 ? nullptr : p; };
    const int rc = gbacore_run((int)cap, pos.get(), (int)P, arg(0, slots.get()), arg(1, off.get()), arg(2, kf.get()), arg(3, idx.get()),
                               (int)K, kf_off.get(), kx.get(), ky.get(), oct.get(), ur.get(), nleft.get(), arg(4, Tcw.get()),
                               arg(5, fixed.get()), arg(6, cam.get()), arg(7, sig.get()), h[4], h[5], h[11], h[12],
                               h[6] < 0 ? nullptr : &flag, (vsg_pose_se3d *)arg(8, kf_out.get()), arg(11, pos_out.get()),
                               arg(9, included.get()), chi2.get(), arg(10, &res));
    out.write((const char *)&rc, 4), out.write((const char *)&res, sizeof(res));
    out.write((const char *)kf_out.get(), (std::streamsize)(56 * K)), out.write((const char *)pos_out.get(), (std::streamsize)(12 * P));
    out.write((const char *)included.get(), (std::streamsize)P), out.write((const char *)chi2.get(), (std::streamsize)(8 * E));
    out.write((const char *)pos.get(), (std::streamsize)(12 * cap));
    records++;
  }
  printf("OK %d\n", records);
  return 0;
}
