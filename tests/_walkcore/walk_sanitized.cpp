// walkcore.cpp as a program of its own for the AddressSanitizer + UBSan build (tests/test_sanitizers_walk.py): reads
// records from argv[1], walks each with every array a heap block of exactly its size, and writes the results to argv[2].
// Record: int32 head[8] = {form, nq, nf, n_ent, check_orientation, has (1 q_valid, 2 blocked_in, 4 slots_in, 8 observed),
// nnratio's bits, 0}, then ent[n_ent], off[nq], cnt[nq], q_valid[nq]?, observed[nq]?, blocked_in[nf]? (bytes, each padded
// to 4), q_angle[nq], t_angle[nf], q_slot[nq], slots_in[nf]?.  Output per record: int32 differs (0: the round form equals
// the definition), dev_info[34], train_match[nf], train_blocked[nf] as int32, edges[2 nf].
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" void walkcore_case(int form, int nq, int nf, int n_ent, const uint32_t *ent, const int32_t *off,
                              const int32_t *cnt, const uint8_t *q_valid, const uint8_t *observed,
                              const uint8_t *blocked_in, const float *q_angle, const float *t_angle, const int32_t *q_slot,
                              const int32_t *slots_in, int check_orientation, float nnratio, int32_t *ref_tm,
                              uint8_t *ref_tb, int32_t *ref_edges, int32_t *ref_info, int32_t *dev_tm, uint8_t *dev_tb,
                              int32_t *dev_edges, int32_t *dev_info);

template <class T>
static T *take(const uint8_t *&p, size_t count) {  // a heap block of exactly count elements
  T *a = new T[count ? count : 1];
  memcpy(a, p, count * sizeof(T));
  p += (count * sizeof(T) + 3) & ~(size_t)3;
  return a;
}
template <class T>
static T *blank(size_t count, int fill) {
  T *a = new T[count ? count : 1];
  memset(a, fill, (count ? count : 1) * sizeof(T));
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
  int any = 0;
  while (p < end) {
    int32_t head[8];
    memcpy(head, p, sizeof(head));
    p += sizeof(head);
    const size_t nq = (size_t)head[1], nf = (size_t)head[2], ne = (size_t)head[3];
    float nnratio;
    memcpy(&nnratio, &head[6], 4);
    uint32_t *ent = take<uint32_t>(p, ne);
    int32_t *off = take<int32_t>(p, nq), *cnt = take<int32_t>(p, nq);
    uint8_t *qv = (head[5] & 1) ? take<uint8_t>(p, nq) : nullptr, *obs = (head[5] & 8) ? take<uint8_t>(p, nq) : nullptr;
    uint8_t *blk = (head[5] & 2) ? take<uint8_t>(p, nf) : nullptr;
    float *qa = take<float>(p, nq), *ta = take<float>(p, nf);
    int32_t *qs = take<int32_t>(p, nq), *si = (head[5] & 4) ? take<int32_t>(p, nf) : nullptr;
    int32_t *rtm = blank<int32_t>(nf, 0x55), *dtm = blank<int32_t>(nf, 0x55);
    uint8_t *rtb = blank<uint8_t>(nf, 0x55), *dtb = blank<uint8_t>(nf, 0x55);
    int32_t *re = blank<int32_t>(2 * nf, 0), *de = blank<int32_t>(2 * nf, 0);
    int32_t ri[34], di[34];
    walkcore_case(head[0], (int)nq, (int)nf, (int)ne, ent, off, cnt, qv, obs, blk, qa, ta, qs, si, head[4], nnratio, rtm,
                  rtb, re, ri, dtm, dtb, de, di);
    int32_t differs = (ri[0] != di[0]) | (ri[1] != di[1]) << 1 | (memcmp(rtm, dtm, nf * 4) != 0) << 2 |
                      (memcmp(rtb, dtb, nf) != 0) << 3 | (memcmp(re, de, nf * 8) != 0) << 4 |
                      (memcmp(ri + 4, di + 4, 120) != 0) << 5;
    any |= differs;
    fwrite(&differs, 4, 1, o), fwrite(di, 4, 34, o), fwrite(dtm, 4, nf, o);
    for (size_t i = 0; i < nf; i++) {
      const int32_t v = dtb[i];
      fwrite(&v, 4, 1, o);
    }
    fwrite(de, 4, 2 * nf, o);
    delete[] ent, delete[] off, delete[] cnt, delete[] qv, delete[] obs, delete[] blk, delete[] qa, delete[] ta;
    delete[] qs, delete[] si, delete[] rtm, delete[] dtm, delete[] rtb, delete[] dtb, delete[] re, delete[] de;
  }
  fclose(o);
  return any ? 1 : 0;
}
