// vsg::KeyFrameDatabase and vsg::ORBVocabulary::score through include/vsg_orb_adaptor.hpp from plain C++: a vocabulary
// image and a script of operations (text, written by tests/test_gpu_kfdb_edges.py) go in, one line per query comes out
// and the test compares it with tests/kfdb_reference.py.  Doubles travel as hexadecimal floats (%a): every bit counts.
//   usage: kfdb_check <voc.bin> <script.txt> <out.txt>
// script, one operation per line (ids are decimal uint64, a BowVector is `n id val id val ...`):
//   add <kf> <map> <bow>          erase <kf>          clear          clearmap <map>
//   setmap <n> <kf map>...        cov <kf> <n> <neighbour>...
//   reloc <query id> <map> <bow>                                   -> "reloc <ids...>"
//   nbest <kf> <map> <n candidates> <n> <connected>... <n> <bad maps>... <bow>
//                                                                  -> "nbest <loop ids...> | <merge ids...>"
//   score <bow> <bow>                                              -> "score <%a>"
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>

#include "vsg_orb_adaptor.hpp"

typedef vsg::KeyFrameDatabase::BowVector BowVector;

static bool read_bow(std::istream &in, BowVector &bow) {
  bow.clear();
  int n = -1;
  if (!(in >> n) || n < 0) return false;
  for (int i = 0; i < n; ++i) {
    unsigned id;
    std::string val;
    if (!(in >> id >> val)) return false;
    bow.emplace(id, strtod(val.c_str(), nullptr));
  }
  return (int)bow.size() == n;
}

template <class T>
static bool read_list(std::istream &in, std::vector<T> &v) {
  v.clear();
  int n = -1;
  if (!(in >> n) || n < 0) return false;
  for (int i = 0; i < n; ++i) {
    T x;
    if (!(in >> x)) return false;
    v.push_back(x);
  }
  return true;
}

static void put_ids(FILE *o, const std::vector<uint64_t> &ids) {
  for (uint64_t id : ids) fprintf(o, " %" PRIu64, id);
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  try {
    if (vsg_device_count() <= 0) {
      printf("no HIP device: vsg::KeyFrameDatabase has no CPU fallback\n");
      return 3;
    }
    std::ifstream vf(argv[1], std::ios::binary);
    if (!vf) return 2;
    const std::vector<char> blob((std::istreambuf_iterator<char>(vf)), std::istreambuf_iterator<char>());
    std::ifstream script(argv[2]);
    if (!script) return 2;
    FILE *o = fopen(argv[3], "w");
    if (!o) return 2;
    vsg::ORBVocabulary voc((const uint8_t *)blob.data(), blob.size());
    vsg::KeyFrameDatabase db(voc);
    std::string line;
    int n_ops = 0;
    while (std::getline(script, line)) {
      if (line.empty()) continue;
      std::istringstream in(line);
      std::string op;
      in >> op;
      uint64_t kf = 0;
      int32_t map = 0;
      BowVector bow, bow2;
      bool ok = true;
      if (op == "add") {
        ok = (bool)(in >> kf >> map) && read_bow(in, bow);
        if (ok) db.add(kf, map, bow);
      } else if (op == "erase") {
        ok = (bool)(in >> kf);
        if (ok) db.erase(kf);
      } else if (op == "clear") {
        db.clear();
      } else if (op == "clearmap") {
        ok = (bool)(in >> map);
        if (ok) db.clearMap(map);
      } else if (op == "setmap") {
        int n = -1;
        ok = (bool)(in >> n) && n >= 0;
        std::vector<uint64_t> kfs;
        std::vector<int32_t> maps;
        for (int i = 0; ok && i < n; ++i) {
          ok = (bool)(in >> kf >> map);
          kfs.push_back(kf), maps.push_back(map);
        }
        if (ok) db.SetMap(kfs, maps);
      } else if (op == "cov") {
        std::vector<uint64_t> nb;
        ok = (bool)(in >> kf) && read_list(in, nb);
        if (ok) db.SetCovisibility({kf}, {nb});
      } else if (op == "reloc") {
        ok = (bool)(in >> kf >> map) && read_bow(in, bow);
        if (ok) {
          fprintf(o, "reloc");
          put_ids(o, db.DetectRelocalizationCandidates(kf, bow, map));
          fprintf(o, "\n");
        }
      } else if (op == "nbest") {
        int n_cand = 0;
        std::vector<uint64_t> conn, loop, merge;
        std::vector<int32_t> bad;
        ok = (bool)(in >> kf >> map >> n_cand) && read_list(in, conn) && read_list(in, bad) && read_bow(in, bow);
        if (ok) {
          db.DetectNBestCandidates(kf, bow, conn, map, bad, loop, merge, n_cand);
          fprintf(o, "nbest");
          put_ids(o, loop);
          fprintf(o, " |");
          put_ids(o, merge);
          fprintf(o, "\n");
        }
      } else if (op == "score") {
        ok = read_bow(in, bow) && read_bow(in, bow2);
        if (ok) fprintf(o, "score %a\n", voc.score(bow, bow2));
      } else {
        ok = false;
      }
      if (!ok) {
        fprintf(stderr, "kfdb_check: cannot read operation %d: %s\n", n_ops, line.substr(0, 60).c_str());
        fclose(o);
        return 2;
      }
      ++n_ops;
    }
    if (fclose(o) != 0) return 2;
    printf("OK %d operations\n", n_ops);
    return 0;
  } catch (const std::exception &e) {
    fprintf(stderr, "kfdb_check: %s\n", e.what());
    return 3;
  }
}
