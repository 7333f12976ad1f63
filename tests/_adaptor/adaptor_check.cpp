// End-to-end exercise of include/vsg_orb_adaptor.hpp from plain C++ (no Python, no OpenCV): two synthetic frames
// -> vsg::ORBextractor -> vsg::FrameGrid -> vsg::ORBmatcher::SearchWindow / SearchByBoW (with vsg::ORBVocabulary).
// Every output is dumped to a flat binary file that tests/test_gpu_adaptor.py compares with the CPU oracle.
//   usage: adaptor_check <vocab.bin> <out.bin>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

#include "vsg_orb_adaptor.hpp"
#include "vsg_synth.h"

template <class T>
static void dump(std::ofstream &f, const std::vector<T> &v) {
  int32_t n = (int32_t)v.size();
  f.write((const char *)&n, 4);
  if (n) f.write((const char *)v.data(), sizeof(T) * v.size());
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  try {
    const int W = 640, H = 480;
    std::vector<uint8_t> img[2] = {std::vector<uint8_t>(W * H), std::vector<uint8_t>(W * H)};
    for (int t = 0; t < 2; ++t)
      if (vsg_synth_sequence_frame(W, H, 5, t, 1, 6, img[t].data(), W)) return 2;

    vsg::ORBextractor ex(1000, 1.2f, 8, 20, 7);
    std::vector<vsg_keypoint> kps[2];
    std::vector<uint8_t> desc[2];
    std::vector<int> lap{0, 0};
    int mono[2];
    for (int t = 0; t < 2; ++t) mono[t] = ex(img[t].data(), H, W, W, kps[t], desc[t], lap);

    // window search: frame-0 keypoints looked up in frame 1's grid at the known (3,2) px shift, r = 15 * scale
    std::vector<float> angle[2], qx, qy, qr;
    std::vector<int32_t> octave[2], lo, hi;
    for (int t = 0; t < 2; ++t)
      for (auto &k : kps[t]) angle[t].push_back(k.angle), octave[t].push_back(k.octave);
    const std::vector<float> scale = ex.GetScaleFactors();
    for (auto &k : kps[0]) {
      qx.push_back(k.x - 3.0f), qy.push_back(k.y - 2.0f), qr.push_back(15.0f * scale[k.octave]);
      lo.push_back(k.octave - 1), hi.push_back(k.octave + 1);
    }
    vsg::FrameGrid grid(kps[1].data(), (int)kps[1].size(), 0.f, 0.f, (float)W, (float)H);
    vsg::Candidates cand = grid.GetFeaturesInArea(qx.data(), qy.data(), qr.data(), lo.data(), hi.data(), (int)qx.size());

    vsg::ORBmatcher matcher(0.7f, true);
    vsg::FeatureView q{desc[0].data(), angle[0].data(), octave[0].data(), (int)kps[0].size()};
    vsg::FeatureView tr{desc[1].data(), angle[1].data(), octave[1].data(), (int)kps[1].size()};
    std::vector<int32_t> bestIdx, bestDist, trainMatch;
    std::vector<uint8_t> trainBlocked;
    std::vector<uint8_t> qBlocks(q.n, 1);
    int nwin = matcher.SearchWindow(q, qBlocks.data(), cand, tr, vsg::ORBmatcher::TH_HIGH, bestIdx, bestDist,
                                    &trainBlocked, &trainMatch);

    // BoW: vocabulary image from disk, transform both frames, SearchByBoW(KF = frame 0, F = frame 1)
    std::ifstream vf(argv[1], std::ios::binary);
    std::vector<uint8_t> blob((std::istreambuf_iterator<char>(vf)), std::istreambuf_iterator<char>());
    vsg::ORBVocabulary voc(blob.data(), blob.size());
    std::map<unsigned, double> bow[2];
    vsg::FeatureVectorCSR fv[2];
    for (int t = 0; t < 2; ++t) voc.transform(desc[t].data(), (int)kps[t].size(), bow[t], fv[t], 2);
    // round trip through the reference's container type
    std::map<unsigned, std::vector<unsigned>> featVecMap;
    for (int i = 0; i < fv[0].nodes(); ++i)
      featVecMap[(unsigned)fv[0].node[i]].assign(fv[0].idx.begin() + fv[0].off[i], fv[0].idx.begin() + fv[0].off[i + 1]);
    vsg::FeatureVectorCSR fv0(featVecMap);
    std::vector<uint8_t> kfValid(q.n, 1);
    for (int i = 0; i < q.n; i += 7) kfValid[i] = 0;
    std::vector<int32_t> matchF;
    int nbow = matcher.SearchByBoW(q, kfValid.data(), fv0, tr, fv[1], matchF);

    std::vector<int32_t> init12;
    int ninit = matcher.SearchForInitialization(q, cand, tr, init12);

    // SearchForTriangulation with an arbitrary pure pair predicate standing in for the epipolar test
    std::vector<uint8_t> elig0(q.n, 1), elig1(tr.n, 1);
    for (int i = 0; i < q.n; i += 5) elig0[i] = 0;
    for (int i = 0; i < tr.n; i += 9) elig1[i] = 0;
    std::vector<std::pair<size_t, size_t>> tri;
    int ntri = matcher.SearchForTriangulation(q, elig0.data(), fv0, tr, elig1.data(), fv[1],
                                              [](int i1, int i2) { return (i1 * 7 + i2 * 3) % 5 != 0; }, tri);
    std::vector<int32_t> tri_flat;
    for (auto &pr : tri) tri_flat.push_back((int32_t)pr.first), tri_flat.push_back((int32_t)pr.second);

    const int d01 = vsg::ORBmatcher::DescriptorDistance(desc[0].data(), desc[1].data());

    // ---- the resident path: frame 1 straight out of the extractor (it ran last), frame 0 uploaded from the host
    vsg::ResidentFrame R0(ex.capacity(H, W)), R1(ex.capacity(H, W));
    R1.FromExtractor(ex, kps[1], 0.f, 0.f, (float)W, (float)H);
    R0.Upload(kps[0].data(), desc[0].data(), nullptr, (int)kps[0].size(), -1, 0.f, 0.f, (float)W, (float)H);
    vsg::ProjectedPoints P;
    for (auto &k : kps[0]) {
      P.u.push_back(k.x - 3.0f), P.v.push_back(k.y - 2.0f), P.level.push_back(k.octave), P.angle.push_back(k.angle);
      P.radius.push_back(10.0f * scale[k.octave]), P.observed.push_back(1);
    }
    P.desc = desc[0];
    P.ur = P.u;
    vsg::ResidentMatcher rm(0.7f, true);
    std::vector<uint8_t> rBlocked;
    std::vector<int32_t> rLast, rSim3(kps[1].size(), -1), rFuseIdx, rFuseDist, rInit;
    const int nlast = rm.SearchByProjection(R1, P, 15.0f, 0, scale, rBlocked, rLast);
    const int nsim3 = rm.SearchByProjection(R1, P, 1.0f, rSim3);
    const int nfuse = rm.Fuse(R1, P, false, ex.GetInverseScaleSigmaSquares(), rFuseIdx, rFuseDist);
    std::vector<float> px, py;
    for (auto &k : kps[0]) px.push_back(k.x), py.push_back(k.y);
    const int nrinit = rm.SearchForInitialization(R0, R1, px, py, 100, rInit);
    // the same triangulation search on the two resident frames: identical pairs expected
    std::vector<std::pair<size_t, size_t>> rtri;
    const int nrtri = rm.SearchForTriangulation(R0, elig0.data(), fv0, R1, elig1.data(), fv[1],
                                                [](int i1, int i2) { return (i1 * 7 + i2 * 3) % 5 != 0; }, rtri);
    if (nrtri != ntri || rtri != tri) {
      printf("resident SearchForTriangulation differs from the host-array form (%d vs %d)\n", nrtri, ntri);
      return 4;
    }

    // ComputeBoW on the resident frames (BowVector / FeatureVector assembled on the device, the FeatureVector staying in the
    // frame) and SearchByBoW on the resident FeatureVectors: the host-array forms' results expected, to the byte
    {
      std::map<unsigned, double> rbow[2];
      vsg::FeatureVectorCSR rfv[2];
      voc.ComputeBoW(R0.handle(), rbow[0], rfv[0], 2);
      voc.ComputeBoW(R1.handle(), rbow[1], rfv[1], 2);
      std::vector<int32_t> rmatchF;
      const int nrbow = rm.SearchByBoW(R0, kfValid.data(), R1, rmatchF);
      if (rbow[1] != bow[1] || rfv[1].node != fv[1].node || rfv[1].off != fv[1].off || rfv[1].idx != fv[1].idx ||
          nrbow != nbow || rmatchF != matchF) {
        printf("resident ComputeBoW / SearchByBoW differs from the host-array form (%d vs %d)\n", nrbow, nbow);
        return 4;
      }
    }

    // the NULL-FeatureVector overloads on frames of more than 2048 features (FeatureVector assembled on the host, then copied
    // into the frame) and on an empty frame: equal to the host-array overloads here, to the oracle in the Python test
    const int NB = 3000;
    std::vector<vsg_keypoint> gk[2] = {std::vector<vsg_keypoint>(NB), std::vector<vsg_keypoint>(NB)};
    std::vector<uint8_t> gd[2] = {std::vector<uint8_t>(NB * 32), std::vector<uint8_t>(NB * 32)};
    std::vector<int32_t> gMatchF, gMatch12;
    int ngF = 0, ngKK = 0, neF = 0, neKF = 0, neKK = 0;
    {
      uint64_t s = 0x9E3779B97F4A7C15ull;
      auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
      };
      for (int i = 0; i < NB; ++i) {
        for (int b = 0; b < 32; ++b) gd[0][i * 32 + b] = (uint8_t)rnd();
        gk[0][i] = vsg_keypoint{(float)(rnd() % 640), (float)(rnd() % 480), 31.f, (float)(rnd() % 3600) * 0.1f, 1.f, i % 8, -1};
      }
      for (int i = 0; i < NB; ++i) {  // the Frame: feature (7 i) mod NB of the KeyFrame with up to 8 bits flipped, turned 20 deg
        const int j = (int)((7ull * i) % NB);
        std::copy(gd[0].begin() + j * 32, gd[0].begin() + j * 32 + 32, gd[1].begin() + i * 32);
        for (int r = (int)(rnd() % 9); r > 0; --r) {
          const int bit = (int)(rnd() % 256);
          gd[1][i * 32 + bit / 8] ^= (uint8_t)(1u << (bit % 8));
        }
        gk[1][i] = gk[0][j];
        gk[1][i].angle = std::fmod(gk[0][j].angle + 20.f, 360.f);
      }
      vsg::ResidentFrame G0(NB), G1(NB), E(1);
      G0.Upload(gk[0].data(), gd[0].data(), nullptr, NB, -1, 0.f, 0.f, (float)W, (float)H);
      G1.Upload(gk[1].data(), gd[1].data(), nullptr, NB, -1, 0.f, 0.f, (float)W, (float)H);
      E.Upload(nullptr, nullptr, nullptr, 0, -1, 0.f, 0.f, (float)W, (float)H);
      std::map<unsigned, double> gbow[3];
      vsg::FeatureVectorCSR gfv[3];
      voc.ComputeBoW(G0.handle(), gbow[0], gfv[0], 2);
      voc.ComputeBoW(G1.handle(), gbow[1], gfv[1], 2);
      voc.ComputeBoW(E.handle(), gbow[2], gfv[2], 2);
      std::vector<uint8_t> gv0(NB, 1), gv1(NB, 1);
      for (int i = 0; i < NB; i += 4) gv0[i] = 0;
      for (int i = 0; i < NB; i += 9) gv1[i] = 0;
      std::vector<int32_t> hF, hKK, eF, eKF, eKK;
      const int nhF = rm.SearchByBoW(G0, gv0.data(), gfv[0], G1, gfv[1], hF);
      const int nhKK = rm.SearchByBoW(G0, gv0.data(), gfv[0], G1, gv1.data(), gfv[1], hKK);
      ngF = rm.SearchByBoW(G0, gv0.data(), G1, gMatchF);
      ngKK = rm.SearchByBoW(G0, gv0.data(), G1, gv1.data(), gMatch12);
      if (ngF != nhF || gMatchF != hF || ngKK != nhKK || gMatch12 != hKK) {
        printf("resident SearchByBoW above 2048 features differs from the host-array form (%d vs %d, %d vs %d)\n", ngF, nhF,
               ngKK, nhKK);
        return 4;
      }
      neF = rm.SearchByBoW(G0, gv0.data(), E, eF);                 // empty Frame
      neKF = rm.SearchByBoW(E, gv0.data(), G1, eKF);               // empty KeyFrame
      neKK = rm.SearchByBoW(E, gv0.data(), G1, gv1.data(), eKK);  // empty KF1
      if (gfv[2].nodes() != 0 || !eF.empty() || !eKK.empty() || eKF != std::vector<int32_t>(NB, -1)) {
        printf("resident SearchByBoW with an empty frame left outputs\n");
        return 4;
      }
    }

    // ---- resident frames at the window search's size edges (oracle values in the Python test)
    // (1) a frame of more than 4096 keypoints straight out of the extractor: above that count the grid launch orders its
    //     cells in global memory instead of LDS
    const int WB = 1280, HB = 720;
    std::vector<vsg_keypoint> bk;
    std::vector<uint8_t> bd;
    std::vector<int32_t> bOff, bIdx, bSim3, bLast;
    int nbSim3 = 0, nbLast = 0;
    {
      std::vector<uint8_t> imb((size_t)WB * HB);
      if (vsg_synth_sequence_frame(WB, HB, 21, 0, 1, 6, imb.data(), WB)) return 2;
      vsg::ORBextractor exb(6000, 1.2f, 8, 20, 7);
      exb(imb.data(), HB, WB, WB, bk, bd, lap);
      vsg::ResidentFrame B(exb.capacity(HB, WB));
      B.FromExtractor(exb, bk, 0.f, 0.f, (float)WB, (float)HB);
      vsg::ProjectedPoints Q;   // every third keypoint searched for in its own frame, one pixel off, 12 * scale wide
      for (size_t i = 0; i < bk.size(); i += 3) {
        const vsg_keypoint &k = bk[i];
        Q.u.push_back(k.x + 1.0f), Q.v.push_back(k.y - 1.0f), Q.level.push_back(k.octave), Q.angle.push_back(k.angle);
        Q.radius.push_back(12.0f * scale[k.octave]), Q.observed.push_back(1);
        Q.desc.insert(Q.desc.end(), bd.begin() + i * 32, bd.begin() + i * 32 + 32);
      }
      Q.ur = Q.u;
      const vsg::Candidates c = B.GetFeaturesInArea(Q.u.data(), Q.v.data(), Q.radius.data(), nullptr, nullptr, Q.n());
      bOff = c.off, bIdx = c.idx;
      bSim3.assign(bk.size(), -1);
      nbSim3 = rm.SearchByProjection(B, Q, 1.0f, bSim3);
      std::vector<uint8_t> blk;
      nbLast = rm.SearchByProjection(B, Q, 12.0f, 0, scale, blk, bLast);
    }
    // (2) an uploaded frame whose cells hold 1, 32, 33 and 150 entries: a window chunk with a cell of more than 32 entries
    //     filters twice, every other one through a 32-bit survivor mask
    std::vector<vsg_keypoint> ck;
    std::vector<uint8_t> cd, cqd;
    std::vector<float> cqx, cqy, cqr;
    std::vector<int32_t> cql, cOff, cIdx, cSim3, cFuseIdx, cFuseDist;
    int ncSim3 = 0, ncFuse = 0;
    {
      uint64_t s = 0xD1B54A32D192ED03ull;
      auto rnd = [&]() {
        s ^= s << 13, s ^= s >> 7, s ^= s << 17;
        return s;
      };
      const int cellsX[4] = {10, 20, 30, 40}, count[4] = {1, 32, 33, 150};   // cells (x, 12) of the 64 x 48 grid on 640x480
      for (int c = 0; c < 4; ++c)
        for (int j = 0; j < count[c]; ++j)   // cell px collects x in [10 px - 5, 10 px + 5)
          ck.push_back(vsg_keypoint{cellsX[c] * 10.0f + (float)(rnd() % 900) * 0.01f - 4.5f,
                                    120.0f + (float)(rnd() % 900) * 0.01f - 4.5f, 31.f, (float)(rnd() % 3600) * 0.1f, 1.f,
                                    (int)(rnd() % 3), -1});
      for (size_t i = ck.size(); i > 1; --i) std::swap(ck[i - 1], ck[rnd() % i]);   // cell members spread over the indices
      cd.resize(ck.size() * 32);
      for (auto &b : cd) b = (uint8_t)rnd();
      vsg::ResidentFrame Cf((int)ck.size());
      Cf.Upload(ck.data(), cd.data(), nullptr, (int)ck.size(), -1, 0.f, 0.f, (float)W, (float)H);
      vsg::ProjectedPoints Q;
      for (int c = 0; c < 4; ++c)
        for (int j = 0; j < 6; ++j) {   // radii 4 .. 9 px around the cell centre; the last covers the whole cell
          const int src = (int)(rnd() % ck.size());
          Q.u.push_back(cellsX[c] * 10.0f), Q.v.push_back(120.0f), Q.radius.push_back(4.0f + j);
          Q.level.push_back(1 + j % 2), Q.angle.push_back(0.f), Q.observed.push_back(1);
          Q.desc.insert(Q.desc.end(), cd.begin() + src * 32, cd.begin() + src * 32 + 32);
        }
      Q.ur = Q.u;
      cqx = Q.u, cqy = Q.v, cqr = Q.radius, cqd = Q.desc, cql = Q.level;
      const vsg::Candidates c = Cf.GetFeaturesInArea(Q.u.data(), Q.v.data(), Q.radius.data(), nullptr, nullptr, Q.n());
      cOff = c.off, cIdx = c.idx;
      cSim3.assign(ck.size(), -1);
      ncSim3 = rm.SearchByProjection(Cf, Q, 3.0f, cSim3);
      ncFuse = rm.Fuse(Cf, Q, cFuseIdx, cFuseDist);
    }

    std::ofstream f(argv[2], std::ios::binary);
    std::vector<int32_t> head{mono[0], mono[1], nwin, nbow, ninit, d01, ntri, nlast, nsim3, nfuse, nrinit, ngF, ngKK,
                              neF, neKF, neKK};
    dump(f, head);
    for (int t = 0; t < 2; ++t) dump(f, kps[t]), dump(f, desc[t]);
    dump(f, cand.off), dump(f, cand.idx), dump(f, bestIdx), dump(f, bestDist), dump(f, trainMatch), dump(f, matchF);
    dump(f, init12);
    std::vector<int32_t> bow_ids;
    std::vector<double> bow_vals;
    for (auto &kv : bow[1]) bow_ids.push_back((int32_t)kv.first), bow_vals.push_back(kv.second);
    dump(f, bow_ids), dump(f, bow_vals);
    dump(f, tri_flat);
    dump(f, rLast), dump(f, rSim3), dump(f, rFuseIdx), dump(f, rFuseDist), dump(f, rInit);
    for (int t = 0; t < 2; ++t) dump(f, gk[t]), dump(f, gd[t]);
    dump(f, gMatchF), dump(f, gMatch12);
    dump(f, std::vector<int32_t>{nbSim3, nbLast, ncSim3, ncFuse});
    dump(f, bk), dump(f, bd), dump(f, bOff), dump(f, bIdx), dump(f, bSim3), dump(f, bLast);
    dump(f, ck), dump(f, cd), dump(f, cqx), dump(f, cqy), dump(f, cqr), dump(f, cqd), dump(f, cql), dump(f, cOff), dump(f, cIdx), dump(f, cSim3);
    dump(f, cFuseIdx), dump(f, cFuseDist);
    printf("OK %zu %zu win=%d bow=%d init=%d\n", kps[0].size(), kps[1].size(), nwin, nbow, ninit);
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s\n", e.what());
    return 3;
  }
}
