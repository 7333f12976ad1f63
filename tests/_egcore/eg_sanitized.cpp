// egcore.cpp as a program of its own for the AddressSanitizer + UBSan build (tests/test_sanitizers_eg.py): reads records from
// argv[1], runs each through egcore_run with every array a heap block of exactly its size, and writes the results to argv[2].
// Record: int32 head[10] = {capacity (-1: no store), K, E, P, fix_scale, iterations, null mask, n_kf / n_edges / n_points as
// passed}, then store_pos[3 capacity], Scw[8 K], nonc[8 K], has[K], fixed[K], edge_i[E], edge_j[E], edge_loop[E], slots[P],
// point_ref[P], each padded to 4 bytes.  Null mask bits: 0 Scw, 1 nonc, 2 has, 3 fixed, 4 edge_i, 5 edge_j, 6 edge_loop, 7 slots,
// 8 point_ref, 9 kf_out, 10 res, 11 store.  Output per record: int32 rc, res (64 bytes), kf_out[8 K], pos_out[3 P], chi2[E],
// the store [3 capacity]; every out starts as the sentinel -3 (res as 0x5a bytes).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vsg_orb.h"

extern "C" int egcore_run(float *store_pos, int capacity, int n_kf, const vsg_sim3d *kf_Scw, const vsg_sim3d *kf_non_corrected,
                          const uint8_t *kf_has_non_corrected, const uint8_t *kf_fixed, int n_edges, const int32_t *edge_i,
                          const int32_t *edge_j, const uint8_t *edge_loop, int fix_scale, int iterations, int n_points,
                          const int32_t *slots, const int32_t *point_ref, vsg_sim3d *kf_Scw_out, float *world_pos_out, double *chi2,
                          vsg_essential_graph_result *res);

template <class T>
static T *take(const uint8_t *&p, size_t count) {  // a heap block of exactly count elements (count 0: one element, never read)
  T *a = new T[count ? count : 1];
  memcpy(a, p, count * sizeof(T));
  p += (count * sizeof(T) + 3) & ~(size_t)3;
  return a;
}
template <class T>
static T *fresh(size_t count, T v) {
  T *a = new T[count ? count : 1];
  for (size_t i = 0; i < count; i++) a[i] = v;
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
  const uint8_t *p = in.data(), *end = in.data() + in.size();
  int n = 0;
  while (p < end) {
    int32_t h[10];
    memcpy(h, p, sizeof(h));
    p += sizeof(h);
    const bool store = h[0] >= 0;
    const size_t cap = store ? (size_t)h[0] : 0, K = (size_t)h[1], E = (size_t)h[2], P = (size_t)h[3];
    const int mask = h[6];
    float *pos = take<float>(p, 3 * cap);
    double *Scw = take<double>(p, 8 * K), *nonc = take<double>(p, 8 * K);
    uint8_t *has = take<uint8_t>(p, K), *fixed = take<uint8_t>(p, K);
    int32_t *ei = take<int32_t>(p, E), *ej = take<int32_t>(p, E);
    uint8_t *el = take<uint8_t>(p, E);
    int32_t *slots = take<int32_t>(p, P), *ref = take<int32_t>(p, P);
    double *kf_out = fresh<double>(8 * K, -3.0), *chi2 = fresh<double>(E, -3.0);
    float *pos_out = fresh<float>(3 * P, -3.0f);
    vsg_essential_graph_result *res = new vsg_essential_graph_result;
    memset(res, 0x5a, sizeof(*res));
    auto off = [mask](int bit) { return (mask >> bit) & 1; };
    const int32_t rc = egcore_run(
        (store && !off(11)) ? pos : nullptr, (int)cap, h[7], off(0) ? nullptr : (const vsg_sim3d *)Scw, off(1) ? nullptr : (const vsg_sim3d *)nonc,
        off(2) ? nullptr : has, off(3) ? nullptr : fixed, h[8], off(4) ? nullptr : ei, off(5) ? nullptr : ej, off(6) ? nullptr : el, h[4], h[5],
        h[9], off(7) ? nullptr : slots, off(8) ? nullptr : ref, off(9) ? nullptr : (vsg_sim3d *)kf_out, pos_out, chi2, off(10) ? nullptr : res);
    fwrite(&rc, 4, 1, o), fwrite(res, sizeof(*res), 1, o), fwrite(kf_out, 8, 8 * K, o), fwrite(pos_out, 4, 3 * P, o);
    fwrite(chi2, 8, E, o), fwrite(pos, 4, 3 * cap, o);
    delete[] pos, delete[] Scw, delete[] nonc, delete[] has, delete[] fixed, delete[] ei, delete[] ej, delete[] el, delete[] slots;
    delete[] ref, delete[] kf_out, delete[] chi2, delete[] pos_out, delete res;
    n++;
  }
  fclose(o);
  printf("OK %d\n", n);
  return 0;
}
