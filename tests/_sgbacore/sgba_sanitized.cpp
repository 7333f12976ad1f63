// The host build of csrc/vsg_sgraph_ba.h (sgbacore.cpp) as a program of its own for AddressSanitizer + UBSan
// (tests/test_sanitizers_sgba.py): reads records from a file, copies every array into a heap block of exactly its size, runs
// sgbacore_run and appends the return code, res and every out to a second file.
//   record: the record of tests/_localbacore/lba_sanitized.cpp (int32 head[12] and the visual arrays), then int32 sem[6] =
//           {planes, plane observations, rooms, length of pl_obs_off, mask of NULL semantic arguments, 0}, then plane_eq[4 Pl],
//           pl_obs_off, pl_obs_kf, pl_obs_local[4 NO], pl_obs_G[16 NO], w_plane_kf, w_plane_point, room_center[3 R],
//           room_n_walls[R], room_wall[4 R]
//   usage: sgba_sanitized <in.bin> <out.bin>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>

#include "../../include/vsg_orb.h"

extern "C" int sgbacore_run(int capacity, float *store_pos, int n_points, const int32_t *slots, const int32_t *obs_off,
                            const int32_t *obs_kf, const int32_t *obs_idx, int n_kf, const int32_t *kf_off, const float *kx,
                            const float *ky, const int32_t *oct, const float *ur, const int32_t *nleft, const vsg_pose_se3 *kf_Tcw,
                            const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam, const float *inv_level_sigma2, int nlevels,
                            int iterations, const volatile uint8_t *stop_flag, vsg_pose_se3d *kf_Tcw_out, float *world_pos_out,
                            uint8_t *erase, double *chi2, int n_planes, const double *plane_eq, const int32_t *pl_obs_off,
                            const int32_t *pl_obs_kf, const double *pl_obs_local, const double *pl_obs_G, const double *w_plane_kf,
                            const double *w_plane_point, int n_rooms, const double *room_center, const int32_t *room_n_walls,
                            const int32_t *room_wall, double *plane_eq_out, double *room_center_out, uint8_t *erase_plane,
                            double *chi2_plane_kf, double *chi2_plane_point, vsg_sgraph_local_ba_result *res);

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
    int32_t h[12];
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
    int32_t g[6];
    in.read((char *)g, sizeof(g));
    const size_t Pl = (size_t)g[0], NO = (size_t)g[1], R = (size_t)g[2], npo = (size_t)g[3];
    const int smask = g[4];
    auto eq = block<double>(in, 4 * Pl);
    auto poff = block<int32_t>(in, npo), pkf = block<int32_t>(in, NO);
    auto loc = block<double>(in, 4 * NO), G = block<double>(in, 16 * NO), wk = block<double>(in, NO), wp = block<double>(in, NO);
    auto rc0 = block<double>(in, 3 * R);
    auto rn = block<int32_t>(in, R), rw = block<int32_t>(in, 4 * R);
    if (!in) return 2;
    auto kf_out = filled<double>(7 * K, -7.0);
    auto pos_out = filled<float>(3 * P, -7.0f);
    auto erase = filled<uint8_t>(E, 9);
    auto chi2 = filled<double>(E, -7.0);
    auto plane_out = filled<double>(4 * Pl, -7.0), room_out = filled<double>(3 * R, -7.0), c2k = filled<double>(NO, -7.0), c2p = filled<double>(NO, -7.0);
    auto erase_plane = filled<uint8_t>(NO, 9);
    vsg_sgraph_local_ba_result res;
    memset(&res, 0x5A, sizeof(res));
    uint8_t flag = (uint8_t)(h[6] > 0);
    auto arg = [mask](int bit, auto *p) { return (mask >> bit) & 1 ? nullptr : p; };
    auto sarg = [smask](int bit, auto *p) { return (smask >> bit) & 1 ? nullptr : p; };
    const int rc = sgbacore_run((int)cap, pos.get(), (int)P, arg(0, slots.get()), arg(1, off.get()), arg(2, kf.get()), arg(3, idx.get()),
                                (int)K, kf_off.get(), kx.get(), ky.get(), oct.get(), ur.get(), nleft.get(), arg(4, Tcw.get()),
                                arg(5, fixed.get()), arg(6, cam.get()), arg(7, sig.get()), h[4], h[5], h[6] < 0 ? nullptr : &flag,
                                (vsg_pose_se3d *)arg(8, kf_out.get()), pos_out.get(), arg(9, erase.get()), chi2.get(), (int)Pl,
                                sarg(0, eq.get()), sarg(1, poff.get()), sarg(2, pkf.get()), sarg(3, loc.get()), sarg(4, G.get()),
                                sarg(5, wk.get()), sarg(6, wp.get()), (int)R, sarg(7, rc0.get()), sarg(8, rn.get()), sarg(9, rw.get()),
                                sarg(10, plane_out.get()), sarg(11, room_out.get()), sarg(12, erase_plane.get()), c2k.get(), c2p.get(),
                                arg(10, &res));
    out.write((const char *)&rc, 4), out.write((const char *)&res, sizeof(res));
    out.write((const char *)kf_out.get(), (std::streamsize)(56 * K)), out.write((const char *)pos_out.get(), (std::streamsize)(12 * P));
    out.write((const char *)erase.get(), (std::streamsize)E), out.write((const char *)chi2.get(), (std::streamsize)(8 * E));
    out.write((const char *)pos.get(), (std::streamsize)(12 * cap));
    out.write((const char *)plane_out.get(), (std::streamsize)(32 * Pl)), out.write((const char *)room_out.get(), (std::streamsize)(24 * R));
    out.write((const char *)erase_plane.get(), (std::streamsize)NO), out.write((const char *)c2k.get(), (std::streamsize)(8 * NO));
    out.write((const char *)c2p.get(), (std::streamsize)(8 * NO));
    records++;
  }
  printf("OK %d\n", records);
  return 0;
}
