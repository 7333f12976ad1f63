// vsg_orb_adaptor.hpp -- header-only C++ mirror of the reference's ORBextractor surface over the C ABI.
//
// `vsg::ORBextractor` has the constructor, operator() and getters of VS_GRAPHS::ORBextractor
// (orb_slam3/include/ORBextractor.h:42-119) on POD types, so it compiles without OpenCV.  When OpenCV is
// available (the reference's own build), define VSG_WITH_OPENCV before including this header to get the
// exact reference signature
//     int operator()(cv::InputArray, cv::InputArray, std::vector<cv::KeyPoint>&, cv::OutputArray, std::vector<int>&)
// and a `mvImagePyramid` refresh for Frame::ComputeStereoMatches (Frame.cc:964,1054-1069).
// See INTEGRATION.md for the three-line change in Tracking.cc / Frame.cc that swaps the extractor.
#pragma once
#include <algorithm>
#include <cstring>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "vsg_orb.h"

#ifdef VSG_WITH_OPENCV
#include <opencv2/core/core.hpp>
#include <cstring>
#endif

namespace vsg {

class ORBextractor {
 public:
  enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };  // ORBextractor.h:45-49

  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0)
      : nlevels_(nlevels), scaleFactor_(scaleFactor) {
    int rc = vsg_orb_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, 1, &h_);
    if (rc != VSG_OK) throw std::runtime_error(std::string("vsg_orb_create: ") + vsg_last_error());
    scale_.resize(nlevels), inv_scale_.resize(nlevels), sigma2_.resize(nlevels), inv_sigma2_.resize(nlevels);
    vsg_orb_get_tables(h_, scale_.data(), inv_scale_.data(), sigma2_.data(), inv_sigma2_.data(), nullptr, nullptr);
#ifdef VSG_WITH_OPENCV
    mvImagePyramid.resize(nlevels);
#endif
  }
  ~ORBextractor() { vsg_orb_destroy(h_); }
  ORBextractor(const ORBextractor &) = delete;
  ORBextractor &operator=(const ORBextractor &) = delete;

  // POD form of operator(): gray CV_8UC1 rows x cols, `stride` bytes per row; vLappingArea = {lap0, lap1}.
  // Returns monoIndex, or -1 for an empty image like the reference (ORBextractor.cc:1087-1088).
  int operator()(const uint8_t *gray, int rows, int cols, int stride, std::vector<vsg_keypoint> &keypoints,
                 std::vector<uint8_t> &descriptors, const std::vector<int> &vLappingArea) {
    keypoints.clear();
    descriptors.clear();
    if (!gray || rows <= 0 || cols <= 0) return -1;
    const int cap = vsg_orb_capacity(h_, rows, cols);
    if (cap < 0) throw std::runtime_error(std::string("vsg_orb_capacity: ") + vsg_last_error());
    keypoints.resize(cap);
    descriptors.resize((size_t)cap * 32);
    int n = 0;
    const int mono = vsg_orb_extract(h_, gray, rows, cols, stride, vLappingArea.at(0), vLappingArea.at(1),
                                     keypoints.data(), descriptors.data(), cap, &n);
    if (mono < 0) throw std::runtime_error(std::string("vsg_orb_extract: ") + vsg_last_error());
    keypoints.resize(n);
    descriptors.resize((size_t)n * 32);
    return mono;
  }

#ifdef VSG_WITH_OPENCV
  static_assert(sizeof(cv::KeyPoint) == sizeof(vsg_keypoint), "cv::KeyPoint must be the 28-byte record");
  // The reference signature (ORBextractor.h:59-61).  The mask is ignored, as in the reference (:58).
  int operator()(cv::InputArray _image, cv::InputArray /*_mask*/, std::vector<cv::KeyPoint> &_keypoints,
                 cv::OutputArray _descriptors, std::vector<int> &vLappingArea) {
    if (_image.empty()) return -1;
    cv::Mat image = _image.getMat();
    CV_Assert(image.type() == CV_8UC1);
    const int cap = vsg_orb_capacity(h_, image.rows, image.cols);
    if (cap < 0) CV_Error(cv::Error::StsBadArg, vsg_last_error());
    std::vector<vsg_keypoint> kps(cap);
    cv::Mat desc(cap, 32, CV_8U);
    int n = 0;
    const int mono = vsg_orb_extract(h_, image.data, image.rows, image.cols, (int)image.step, vLappingArea[0],
                                     vLappingArea[1], kps.data(), desc.data, cap, &n);
    if (mono < 0) CV_Error(cv::Error::StsError, vsg_last_error());
    _keypoints.resize(n);
    if (n) std::memcpy((void *)_keypoints.data(), kps.data(), (size_t)n * sizeof(vsg_keypoint));
    if (n == 0)
      _descriptors.release();  // ORBextractor.cc:1105-1106
    else
      desc.rowRange(0, n).copyTo(_descriptors);
    return mono;
  }
  // Refresh mvImagePyramid (bordered buffers + ROI views, as ComputePyramid leaves them) on demand; only the stereo
  // matcher reads it (Frame.cc:964,1054-1069).  ONE device-to-host copy for all levels into a buffer that is reused
  // from call to call; the cv::Mat headers point into it (no allocation, no per-level transfer).
  void DownloadPyramid(int frame = 0) {
    std::vector<size_t> off(nlevels_);
    const int need = vsg_orb_copy_pyramid(h_, frame, nullptr, 0, off.data());
    if (need < 0) CV_Error(cv::Error::StsError, vsg_last_error());
    if (pyr_host_.size() < (size_t)need) pyr_host_.resize((size_t)need);
    if (vsg_orb_copy_pyramid(h_, frame, pyr_host_.data(), pyr_host_.size(), off.data()) < 0)
      CV_Error(cv::Error::StsError, vsg_last_error());
    for (int l = 0; l < nlevels_; l++) {
      int w = 0, h = 0;
      vsg_orb_level_size(h_, l, &w, &h);
      cv::Mat temp(h + 38, w + 38, CV_8UC1, pyr_host_.data() + off[l], (size_t)(w + 38));
      mvImagePyramid[l] = temp(cv::Rect(19, 19, w, h));
    }
  }
  std::vector<cv::Mat> mvImagePyramid;  // ORBextractor.h:93
#endif

  // keypoint capacity per frame for images of this size (>= nfeatures + 3 * nlevels)
  int capacity(int rows, int cols) const {
    const int cap = vsg_orb_capacity(h_, rows, cols);
    if (cap < 0) throw std::runtime_error(std::string("vsg_orb_capacity: ") + vsg_last_error());
    return cap;
  }
  int GetLevels() const { return nlevels_; }
  float GetScaleFactor() const { return scaleFactor_; }
  std::vector<float> GetScaleFactors() const { return scale_; }
  std::vector<float> GetInverseScaleFactors() const { return inv_scale_; }
  std::vector<float> GetScaleSigmaSquares() const { return sigma2_; }
  std::vector<float> GetInverseScaleSigmaSquares() const { return inv_sigma2_; }
  vsg_orb *handle() const { return h_; }

 private:
  vsg_orb *h_ = nullptr;
  int nlevels_;
  float scaleFactor_;
  std::vector<float> scale_, inv_scale_, sigma2_, inv_sigma2_;
#ifdef VSG_WITH_OPENCV
  std::vector<uint8_t> pyr_host_;  // backing store of mvImagePyramid
#endif
};

// static int ORBmatcher::DescriptorDistance(const cv::Mat &a, const cv::Mat &b)  (ORBmatcher.h:40, .cc:2047-2063).
// One pair is eight 32-bit popcounts: host arithmetic (a kernel launch costs four orders of magnitude more); bulk
// distances go through vsg_hamming_pairs / the search entry points.
inline int DescriptorDistance(const uint8_t *a, const uint8_t *b) {
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    uint32_t x, y;
    std::memcpy(&x, a + 4 * i, 4);
    std::memcpy(&y, b + 4 * i, 4);
    dist += __builtin_popcount(x ^ y);
  }
  return dist;
}

inline void check(int rc, const char *what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(rc) + "): " + vsg_last_error());
}

// DBoW2::FeatureVector is std::map<NodeId, std::vector<unsigned>> (FeatureVector.h:25-26); the C ABI takes it as
// CSR with ascending node ids, which is the map's iteration order.
struct FeatureVectorCSR {
  std::vector<int32_t> node, off, idx;
  FeatureVectorCSR() : off(1, 0) {}
  template <class Map>
  explicit FeatureVectorCSR(const Map &fv) : off(1, 0) {
    for (const auto &kv : fv) {
      node.push_back((int32_t)kv.first);
      for (auto i : kv.second) idx.push_back((int32_t)i);
      off.push_back((int32_t)idx.size());
    }
  }
  int nodes() const { return (int)node.size(); }
};

// One side of a match as the reference's Frame / KeyFrame members expose it: mDescriptors rows (Frame.h:280),
// mvKeysUn[i].angle / .octave, and per feature whether it carries a usable MapPoint.
struct FeatureView {
  const uint8_t *desc = nullptr;   // n x 32, contiguous
  const float *angle = nullptr;    // n (may be null when the call does not check orientation)
  const int32_t *octave = nullptr; // n (only SearchByProjection(Frame&, vector<MapPoint*>) / SearchForInitialization)
  int n = 0;
};

// CSR candidate lists = the concatenated results of Frame::GetFeaturesInArea per query (see vsg::FrameGrid).
struct Candidates {
  std::vector<int32_t> off, idx;
};

// Frame::mGrid (Frame.h:290) on the device: AssignFeaturesToGrid + GetFeaturesInArea (Frame.cc:521-553, 802-868).
// The grid of a ResidentFrame on its own (no descriptors): same host build, same kernel, same candidate order.
class FrameGrid {
 public:
  FrameGrid(const vsg_keypoint *keysUn, int n, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, int device = 0) {
    check(vsg_grid_build(device, keysUn, n, mnMinX, mnMinY, mnMaxX, mnMaxY, &g_), "vsg_grid_build");
  }
  ~FrameGrid() { vsg_grid_destroy(g_); }
  FrameGrid(const FrameGrid &) = delete;
  FrameGrid &operator=(const FrameGrid &) = delete;
  // nq windows at once; minLevel/maxLevel may be null (= -1, -1 as KeyFrame::GetFeaturesInArea)
  Candidates GetFeaturesInArea(const float *x, const float *y, const float *r, const int32_t *minLevel,
                               const int32_t *maxLevel, int nq) const {
    Candidates c;
    c.off.resize(nq + 1);
    c.idx.resize(64 * (size_t)nq + 64);
    int total = vsg_grid_query(g_, x, y, r, minLevel, maxLevel, nq, c.off.data(), c.idx.data(), (int)c.idx.size());
    check(total, "vsg_grid_query");
    if (total > (int)c.idx.size()) {
      c.idx.resize(total);
      check(vsg_grid_query(g_, x, y, r, minLevel, maxLevel, nq, c.off.data(), c.idx.data(), total), "vsg_grid_query");
    }
    c.idx.resize(total);
    return c;
  }

 private:
  vsg_grid *g_ = nullptr;
};

// ORBVocabulary (= DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB>, ORBVocabulary.h:29-30): loadFromBinFile
// image + transform() as Frame::ComputeBoW calls it (Frame.cc:882-889).
class ORBVocabulary {
 public:
  ORBVocabulary(const uint8_t *bin_image, size_t size, int device = 0) {
    check(vsg_vocab_load(device, bin_image, size, &v_), "vsg_vocab_load");
  }
  ~ORBVocabulary() { vsg_vocab_destroy(v_); }
  ORBVocabulary(const ORBVocabulary &) = delete;
  ORBVocabulary &operator=(const ORBVocabulary &) = delete;
  // mBowVec as std::map<WordId, WordValue> (BowVector.h:57-58), mFeatVec as CSR
  void transform(const uint8_t *desc, int n, std::map<unsigned, double> &bowVec, FeatureVectorCSR &featVec,
                 int levelsup = 4) const {
    std::vector<int32_t> ids(n > 0 ? n : 1);
    std::vector<double> vals(n > 0 ? n : 1);
    featVec.node.assign(n > 0 ? n : 1, 0);
    featVec.off.assign((n > 0 ? n : 1) + 1, 0);
    featVec.idx.assign(n > 0 ? n : 1, 0);
    int nb = 0, nf = 0;
    check(vsg_bow_transform(v_, desc, n, levelsup, ids.data(), vals.data(), (int)ids.size(), &nb, featVec.node.data(),
                            featVec.off.data(), featVec.idx.data(), (int)featVec.node.size(), &nf, nullptr, nullptr,
                            nullptr),
          "vsg_bow_transform");
    bowVec.clear();
    for (int i = 0; i < nb; ++i) bowVec.emplace_hint(bowVec.end(), (unsigned)ids[i], vals[i]);
    featVec.node.resize(nf);
    featVec.off.resize(nf + 1);
    featVec.idx.resize(featVec.off[nf]);
  }
  // Frame::ComputeBoW / KeyFrame::ComputeBoW (Frame.cc:882-889, KeyFrame.cc:100-110) on a resident frame's descriptors
  // (`frame` = vsg::ResidentFrame::handle()): nothing goes up, mBowVec / mFeatVec come back in final form, and the
  // FeatureVector also STAYS on the device inside the frame (Frame::mFeatVec) for the ResidentMatcher::SearchByBoW
  // overloads that take no FeatureVector.
  void ComputeBoW(vsg_frame *frame, std::map<unsigned, double> &bowVec, FeatureVectorCSR &featVec, int levelsup = 4) const {
    const int n = vsg_frame_size(frame);
    check(n, "vsg_frame_size");
    const int cap = n > 0 ? n : 1;
    std::vector<int32_t> ids(cap);
    std::vector<double> vals(cap);
    featVec.node.assign(cap, 0), featVec.off.assign(cap + 1, 0), featVec.idx.assign(cap, 0);
    int nb = 0, nf = 0;
    check(vsg_frame_bow_transform(v_, frame, levelsup, ids.data(), vals.data(), cap, &nb, featVec.node.data(), featVec.off.data(),
                                  featVec.idx.data(), cap, &nf, nullptr, nullptr, nullptr),
          "vsg_frame_bow_transform");
    bowVec.clear();
    for (int i = 0; i < nb; ++i) bowVec.emplace_hint(bowVec.end(), (unsigned)ids[i], vals[i]);
    featVec.node.resize(nf), featVec.off.resize(nf + 1), featVec.idx.resize(featVec.off[nf]);
  }
  // TemplatedVocabulary::score(v1, v2) (TemplatedVocabulary.h:1214-1219) with the vocabulary's scoring type: the
  // reference's double, bit for bit.  KL scoring throws (VSG_ERR_UNSUPPORTED).
  double score(const std::map<unsigned, double> &v1, const std::map<unsigned, double> &v2) const {
    std::vector<int32_t> a, b;
    std::vector<double> av, bv;
    flatten(v1, a, av), flatten(v2, b, bv);
    const int32_t off[2] = {0, (int32_t)v2.size()};  // not b.size(): flatten() appends a padding element
    double out = 0;
    check(vsg_vocab_score(v_, a.data(), av.data(), (int)v1.size(), off, b.data(), bv.data(), 1, &out), "vsg_vocab_score");
    return out;
  }
  static void flatten(const std::map<unsigned, double> &v, std::vector<int32_t> &ids, std::vector<double> &vals) {
    ids.clear(), vals.clear();  // one padding element: never an empty vector (data() is passed along with the size)
    ids.reserve(v.size() + 1), vals.reserve(v.size() + 1);
    for (const auto &kv : v) ids.push_back((int32_t)kv.first), vals.push_back(kv.second);
    ids.push_back(0), vals.push_back(0.0);
  }
  vsg_vocab *handle() const { return v_; }

 private:
  vsg_vocab *v_ = nullptr;
};

// KeyFrameDatabase (KeyFrameDatabase.h) on the device.  The reference's methods take KeyFrame* / Frame* / Map*; here a
// keyframe is its mnId, a map an int id, and the caller mirrors what the database reads from a KeyFrame: its map
// (add / SetMap when maps merge) and GetBestCovisibilityKeyFrames(10) (SetCovisibility).  INTEGRATION.md shows the glue.
class KeyFrameDatabase {
 public:
  typedef std::map<unsigned, double> BowVector;
  explicit KeyFrameDatabase(const ORBVocabulary &voc) { check(vsg_kfdb_create(voc.handle(), &db_), "vsg_kfdb_create"); }
  ~KeyFrameDatabase() { vsg_kfdb_destroy(db_); }
  KeyFrameDatabase(const KeyFrameDatabase &) = delete;
  KeyFrameDatabase &operator=(const KeyFrameDatabase &) = delete;

  void add(uint64_t kf_id, int32_t map_id, const BowVector &bow) {
    std::vector<int32_t> ids;
    std::vector<double> vals;
    ORBVocabulary::flatten(bow, ids, vals);
    check(vsg_kfdb_add(db_, kf_id, map_id, ids.data(), vals.data(), (int)bow.size()), "vsg_kfdb_add");
    ++n_named_;
  }
  void erase(uint64_t kf_id) { check(vsg_kfdb_erase(db_, kf_id), "vsg_kfdb_erase"); }
  void clear() { check(vsg_kfdb_clear(db_), "vsg_kfdb_clear"); }
  void clearMap(int32_t map_id) { check(vsg_kfdb_clear_map(db_, map_id), "vsg_kfdb_clear_map"); }
  void SetMap(const std::vector<uint64_t> &kf_ids, const std::vector<int32_t> &map_ids) {
    if (kf_ids.size() != map_ids.size()) throw std::runtime_error("vsg_kfdb_set_map: sizes differ");
    check(vsg_kfdb_set_map(db_, kf_ids.data(), map_ids.data(), (int)kf_ids.size()), "vsg_kfdb_set_map");
    n_named_ += kf_ids.size();
  }
  // neighbours[j] = kf_ids[j]->GetBestCovisibilityKeyFrames(10), as mnIds
  void SetCovisibility(const std::vector<uint64_t> &kf_ids, const std::vector<std::vector<uint64_t>> &neighbours) {
    if (kf_ids.size() != neighbours.size()) throw std::runtime_error("vsg_kfdb_set_covisibility: sizes differ");
    std::vector<int32_t> off(1, 0);
    std::vector<uint64_t> flat;
    for (size_t j = 0; j < neighbours.size(); ++j) {
      flat.insert(flat.end(), neighbours[j].begin(), neighbours[j].end());
      off.push_back((int32_t)flat.size());
    }
    flat.push_back(0);
    check(vsg_kfdb_set_covisibility(db_, kf_ids.data(), off.data(), flat.data(), (int)kf_ids.size()),
          "vsg_kfdb_set_covisibility");
    n_named_ += kf_ids.size() + flat.size();
  }
  // DetectRelocalizationCandidates(F, pMap) (KeyFrameDatabase.cc:719-830): F = (F->mnId, F->mBowVec)
  std::vector<uint64_t> DetectRelocalizationCandidates(uint64_t frame_id, const BowVector &bow, int32_t map_id) {
    std::vector<int32_t> ids;
    std::vector<double> vals;
    ORBVocabulary::flatten(bow, ids, vals);
    // a query updates the keyframes' query state and cannot be repeated: room for every keyframe id ever named
    std::vector<uint64_t> out((size_t)n_named_ + 1);
    int n = 0;
    check(vsg_kfdb_detect_relocalization_candidates(db_, frame_id, ids.data(), vals.data(), (int)bow.size(), map_id,
                                                    out.data(), (int)out.size(), &n),
          "vsg_kfdb_detect_relocalization_candidates");
    out.resize(n);
    return out;
  }
  // DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) (KeyFrameDatabase.cc:592-717)
  void DetectNBestCandidates(uint64_t kf_id, const BowVector &bow, const std::vector<uint64_t> &connected, int32_t map_id,
                             const std::vector<int32_t> &bad_maps, std::vector<uint64_t> &vpLoopCand,
                             std::vector<uint64_t> &vpMergeCand, int nNumCandidates) {
    std::vector<int32_t> ids;
    std::vector<double> vals;
    ORBVocabulary::flatten(bow, ids, vals);
    vpLoopCand.assign((size_t)(nNumCandidates > 0 ? nNumCandidates : 1), 0);
    vpMergeCand.assign(vpLoopCand.size(), 0);
    int nl = 0, nm = 0;
    check(vsg_kfdb_detect_n_best_candidates(db_, kf_id, ids.data(), vals.data(), (int)bow.size(),
                                            connected.empty() ? nullptr : connected.data(), (int)connected.size(), map_id,
                                            bad_maps.empty() ? nullptr : bad_maps.data(), (int)bad_maps.size(),
                                            nNumCandidates, vpLoopCand.data(), &nl, vpMergeCand.data(), &nm),
          "vsg_kfdb_detect_n_best_candidates");
    vpLoopCand.resize(nl), vpMergeCand.resize(nm);
  }
  vsg_kfdb *handle() const { return db_; }

 private:
  vsg_kfdb *db_ = nullptr;
  uint64_t n_named_ = 0;  // ids passed to add / SetMap / SetCovisibility: bounds the candidates of a query
};

// VS_GRAPHS::ORBmatcher (ORBmatcher.h:34-99) on flattened views.  The reference's methods take Frame& / KeyFrame* /
// MapPoint* graphs; a maintainer's glue builds the views from those (INTEGRATION.md shows it for each method) and
// writes the returned indices back as MapPoint* assignments.  Same constants, same return values (number of matches).
class ORBmatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;  // ORBmatcher.cc:34-36

  explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0)
      : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device) {}

  static int DescriptorDistance(const uint8_t *a, const uint8_t *b) { return vsg::DescriptorDistance(a, b); }

  // SearchByBoW(KeyFrame *pKF, Frame &F, vector<MapPoint*> &vpMapPointMatches)  (ORBmatcher.cc:226-428)
  // kfValid[i] = (vpMapPointsKF[i] && !isBad()); matchF[iF] = KF feature index or -1.
  int SearchByBoW(const FeatureView &kf, const uint8_t *kfValid, const FeatureVectorCSR &kfFeatVec,
                  const FeatureView &f, const FeatureVectorCSR &fFeatVec, std::vector<int32_t> &matchF) const {
    matchF.assign(f.n, -1);
    int rc = vsg_search_by_bow_kf_f(device_, kf.desc, kf.angle, kfValid, kf.n, kfFeatVec.node.data(),
                                    kfFeatVec.off.data(), kfFeatVec.idx.data(), kfFeatVec.nodes(), f.desc, f.angle,
                                    f.n, fFeatVec.node.data(), fFeatVec.off.data(), fFeatVec.idx.data(),
                                    fFeatVec.nodes(), mfNNratio, mbCheckOrientation, matchF.data());
    check(rc, "vsg_search_by_bow_kf_f");
    return rc;
  }

  // SearchByBoW(KeyFrame *pKF1, KeyFrame *pKF2, vector<MapPoint*> &vpMatches12)  (ORBmatcher.cc:758-900)
  int SearchByBoW(const FeatureView &kf1, const uint8_t *valid1, const FeatureVectorCSR &fv1, const FeatureView &kf2,
                  const uint8_t *valid2, const FeatureVectorCSR &fv2, std::vector<int32_t> &matches12) const {
    matches12.assign(kf1.n, -1);
    int rc = vsg_search_by_bow_kf_kf(device_, kf1.desc, kf1.angle, valid1, kf1.n, fv1.node.data(), fv1.off.data(),
                                     fv1.idx.data(), fv1.nodes(), kf2.desc, kf2.angle, valid2, kf2.n,
                                     fv2.node.data(), fv2.off.data(), fv2.idx.data(), fv2.nodes(), mfNNratio,
                                     mbCheckOrientation, matches12.data());
    check(rc, "vsg_search_by_bow_kf_kf");
    return rc;
  }

  // SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vMatchedPairs, bOnlyStereo, bCoarse)  (ORBmatcher.cc:902-1146)
  // eligible = no MapPoint yet (and stereo when bOnlyStereo).  pairOk(i1, i2, idx1, idx2) is the caller's geometric
  // predicate (:1031-1071: epipole gate, then bCoarse || epipolarConstrain); it is evaluated here for every pair of
  // every shared node and shipped as a bitmask.  Pass nullptr for "every pair passes".
  template <class Pred>
  int SearchForTriangulation(const FeatureView &kf1, const uint8_t *eligible1, const FeatureVectorCSR &fv1,
                             const FeatureView &kf2, const uint8_t *eligible2, const FeatureVectorCSR &fv2, Pred pairOk,
                             std::vector<std::pair<size_t, size_t>> &vMatchedPairs) const {
    std::vector<uint32_t> bits(1, 0u);
    std::vector<int32_t> off(1, 0);
    size_t a = 0, b = 0;
    while (a < fv1.node.size() && b < fv2.node.size()) {  // the reference's merge-join, shared nodes in id order
      if (fv1.node[a] == fv2.node[b]) {
        for (int i1 = fv1.off[a]; i1 < fv1.off[a + 1]; i1++)
          for (int i2 = fv2.off[b]; i2 < fv2.off[b + 1]; i2++) {
            const long long bit = (long long)off.back() + (long long)(i1 - fv1.off[a]) * (fv2.off[b + 1] - fv2.off[b]) +
                                  (i2 - fv2.off[b]);
            if ((size_t)(bit >> 5) >= bits.size()) bits.resize((size_t)(bit >> 5) + 64, 0u);
            if (eligible1[fv1.idx[i1]] && eligible2[fv2.idx[i2]] && pairOk(fv1.idx[i1], fv2.idx[i2]))
              bits[bit >> 5] |= 1u << (bit & 31);
          }
        off.push_back(off.back() + (fv1.off[a + 1] - fv1.off[a]) * (fv2.off[b + 1] - fv2.off[b]));
        a++, b++;
      } else if (fv1.node[a] < fv2.node[b]) {
        a++;
      } else {
        b++;
      }
    }
    bits.resize((size_t)(off.back() >> 5) + 2, 0u);
    std::vector<int32_t> m12(kf1.n > 0 ? kf1.n : 1, -1);
    int rc = vsg_search_for_triangulation(device_, kf1.desc, kf1.angle, eligible1, kf1.n, fv1.node.data(), fv1.off.data(),
                                          fv1.idx.data(), fv1.nodes(), kf2.desc, kf2.angle, eligible2, kf2.n,
                                          fv2.node.data(), fv2.off.data(), fv2.idx.data(), fv2.nodes(), bits.data(),
                                          off.data(), mbCheckOrientation, m12.data());
    check(rc, "vsg_search_for_triangulation");
    vMatchedPairs.clear();
    for (int i = 0; i < kf1.n; i++)
      if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1136-1143
    return rc;
  }

  // SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)  (ORBmatcher.cc:1667-1878).
  // q = LastFrame's map points that project into the image (descriptor + keypoint angle of the last frame's feature),
  // cand = CurrentFrame.GetFeaturesInArea per q; trainBlocked / trainMatch are CurrentFrame-sized.
  int SearchByProjection(const FeatureView &q, const uint8_t *queryBlocks, const Candidates &cand,
                         const FeatureView &cur, std::vector<uint8_t> &trainBlocked,
                         std::vector<int32_t> &trainMatch) const {
    trainMatch.assign(cur.n, -1);
    trainBlocked.resize(cur.n, 0);
    int rc = vsg_search_by_projection_last(device_, q.desc, q.angle, queryBlocks, q.n, cand.off.data(),
                                           cand.idx.data(), cur.desc, cur.angle, trainBlocked.data(), cur.n, TH_HIGH,
                                           mbCheckOrientation, trainMatch.data());
    check(rc, "vsg_search_by_projection_last");
    return rc;
  }

  // SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, th, ...)  (ORBmatcher.cc:42-216)
  int SearchByProjection(const FeatureView &q, const uint8_t *queryBlocks, const Candidates &cand,
                         const FeatureView &frame, std::vector<uint8_t> &trainBlocked,
                         std::vector<int32_t> &trainMatch, bool localMap) const {
    (void)localMap;
    trainMatch.assign(frame.n, -1);
    trainBlocked.resize(frame.n, 0);
    int rc = vsg_search_by_projection_local(device_, q.desc, queryBlocks, q.n, cand.off.data(), cand.idx.data(),
                                            frame.desc, frame.octave, trainBlocked.data(), frame.n, mfNNratio,
                                            trainMatch.data());
    check(rc, "vsg_search_by_projection_local");
    return rc;
  }

  // Common core of SearchByProjection(KeyFrame*, Sim3, ...) x2, SearchByProjection(Frame&, KeyFrame*, ...),
  // SearchBySim3 and Fuse (see include/vsg_orb.h: vsg_search_window).
  int SearchWindow(const FeatureView &q, const uint8_t *queryBlocks, const Candidates &cand, const FeatureView &train,
                   int thHigh, std::vector<int32_t> &qBestIdx, std::vector<int32_t> &qBestDist,
                   std::vector<uint8_t> *trainBlocked = nullptr, std::vector<int32_t> *trainMatch = nullptr) const {
    qBestIdx.assign(q.n, -1);
    qBestDist.assign(q.n, 256);
    if (trainMatch) trainMatch->assign(train.n, -1);
    if (trainBlocked) trainBlocked->resize(train.n, 0);
    int rc = vsg_search_window(device_, q.desc, queryBlocks, q.n, cand.off.data(), cand.idx.data(), train.desc,
                               trainBlocked ? trainBlocked->data() : nullptr, train.n, thHigh, qBestIdx.data(),
                               qBestDist.data(), trainMatch ? trainMatch->data() : nullptr);
    check(rc, "vsg_search_window");
    return rc;
  }

  // SearchForInitialization(Frame &F1, Frame &F2, vbPrevMatched, vnMatches12, windowSize)  (ORBmatcher.cc:643-756)
  int SearchForInitialization(const FeatureView &f1, const Candidates &cand, const FeatureView &f2,
                              std::vector<int32_t> &vnMatches12) const {
    vnMatches12.assign(f1.n, -1);
    int rc = vsg_search_for_initialization(device_, f1.desc, f1.angle, f1.octave, f1.n, cand.off.data(),
                                           cand.idx.data(), f2.desc, f2.angle, f2.n, mfNNratio, mbCheckOrientation,
                                           vnMatches12.data());
    check(rc, "vsg_search_for_initialization");
    return rc;
  }

 protected:
  float mfNNratio;          // ORBmatcher.h:97
  bool mbCheckOrientation;  // ORBmatcher.h:98
  int device_;
};

// Frame::ComputeStereoMatches (Frame.cc:957-1127): mvuRight / mvDepth from the two extractors' device pyramids.
inline int ComputeStereoMatches(const ORBextractor &left, const ORBextractor &right,
                                const std::vector<vsg_keypoint> &kpsL, const uint8_t *descL,
                                const std::vector<vsg_keypoint> &kpsR, const uint8_t *descR, float mb, float mbf,
                                std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
  mvuRight.assign(kpsL.size(), -1.0f);
  mvDepth.assign(kpsL.size(), -1.0f);
  int rc = vsg_stereo_matches(left.handle(), 0, right.handle(), 0, kpsL.data(), descL, (int)kpsL.size(), kpsR.data(),
                              descR, (int)kpsR.size(), mb, mbf, mvuRight.data(), mvDepth.data());
  check(rc, "vsg_stereo_matches");
  return rc;
}

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:380-415) for many map points in one call.
inline std::vector<int32_t> ComputeDistinctiveDescriptors(const uint8_t *desc, const std::vector<int32_t> &off,
                                                          int device = 0) {
  std::vector<int32_t> best(off.empty() ? 0 : off.size() - 1, -1);
  if (!best.empty()) check(vsg_distinctive_descriptors(device, desc, off.data(), (int)best.size(), best.data()),
                           "vsg_distinctive_descriptors");
  return best;
}


// ---------------------------------------------------------------------------------------------------------------
// Device-resident features of a Frame / KeyFrame (include/vsg_orb.h: vsg_frame): what the searches read -- mvKeysUn
// (or mvKeys || mvKeysRight with Nleft), mDescriptors, mvuRight, mGrid / mGridRight (Frame.h:280-290) -- stays on the
// GPU between calls.  A maintainer adds one `std::shared_ptr<vsg::ResidentFrame> mpResident` to Frame and KeyFrame
// (KeyFrame's constructor copies the pointer from the Frame it is built from, like it copies mGrid, KeyFrame.cc:37-60)
// and fills it at the end of the Frame constructors, after UndistortKeyPoints / ComputeStereo* / AssignFeaturesToGrid.
// The camera of one Frame as isInFrustum uses it (vsg_frame_pose): Rcw = mRcw row-major, tcw = mtcw, Ow = mOw,
// fx .. cy = Pinhole::mvParameters, mbf, log_scale_factor = mfLogScaleFactor, n_levels = mnScaleLevels.  Filled per call
// from the Frame's members after SetPose (Frame::UpdatePoseMatrices, Frame.cc:612-619); nothing of it is resident.
typedef vsg_frame_pose FramePose;

// What isInFrustum and SearchByProjection(F, vpMapPoints) read of the local map's MapPoints, resident on the device
// (vsg_mappoints).  A slot is the maintainer's own index of a MapPoint*.  minDist / maxDist are the MEMBERS mfMinDistance /
// mfMaxDistance (PredictScale divides the unscaled one, MapPoint.cc:555), not the getters' 0.8f / 1.2f multiples.
// What ResidentMapPoints::Refresh leaves behind per listed point: best = the position inside the point's observation
// list of the descriptor ComputeDistinctiveDescriptors chose (-1: mDescriptor is kept), and mNormalVector (3 floats per
// point), mfMinDistance, mfMaxDistance as the slot holds them after the call
struct RefreshResult {
  std::vector<int32_t> best;
  std::vector<float> normal, minDist, maxDist;
};

// What vsg::ResidentMapPoints::LocalBundleAdjustment returns: vSE3->estimate() per keyframe (a fixed keyframe, or one
// without an edge: its input, widened), the float position per point (also written into its slot), per observation whether
// (keyframe, point) goes into vToErase and the chi2 compared, and the counters of vsg_local_ba_result.
struct LocalBAResult {
  std::vector<vsg_pose_se3d> kfTcw;
  std::vector<float> worldPos;
  std::vector<uint8_t> erase;
  std::vector<double> chi2;
  vsg_local_ba_result res;
};

// The planes and rooms vsg::ResidentMapPoints::LocalBundleAdjustmentSGraph takes (include/vsg_orb.h names each array):
// planeEq = 4 per plane of localPlaneList (getGlobalEquation().coeffs()); plane i's observations are [planeObsOff[i],
// planeObsOff[i + 1]) of planeObsKf (index into keyFrames), planeObsLocal (4: obs.localPlane), planeObsG (16: obs.Gij
// row-major), wPlaneKf / wPlanePoint (obs.confidence * information_gain, 0 = that edge is not added); roomCenter = 3 per
// room of localRoomList with walls.size() >= 2, roomNWalls = 2 (corridor) or 4, roomWall = 4 plane indices per room.
struct SGraphLists {
  std::vector<double> planeEq;
  std::vector<int32_t> planeObsOff{0}, planeObsKf;
  std::vector<double> planeObsLocal, planeObsG, wPlaneKf, wPlanePoint, roomCenter;
  std::vector<int32_t> roomNWalls, roomWall;
};
// What it returns: LocalBAResult's fields, vPlane->estimate() per plane (a plane without an edge: its input), the room
// vertices' translations, per plane observation whether (keyframe, plane) goes into vToErasePlane and the two chi2
// compared (NaN where the edge does not exist), and the counters of vsg_sgraph_local_ba_result.
struct SGraphLocalBAResult {
  std::vector<vsg_pose_se3d> kfTcw;
  std::vector<float> worldPos;
  std::vector<uint8_t> erase;
  std::vector<double> chi2, planeEq, roomCenter;
  std::vector<uint8_t> erasePlane;
  std::vector<double> chi2PlaneKf, chi2PlanePoint;
  vsg_sgraph_local_ba_result res;
};

// What vsg::ResidentMapPoints::GlobalBundleAdjustment returns: vSE3->estimate() per keyframe (the fixed keyframe, or one
// without an edge: its input, widened), the float position per point (mPosGBA; written into its slot only in the
// nLoopKF == origin case), included[i] = !vbNotIncludedMP[i], the chi2 per observation, and the counters of
// vsg_global_ba_result.
struct GlobalBAResult {
  std::vector<vsg_pose_se3d> kfTcw;
  std::vector<float> worldPos;
  std::vector<uint8_t> included;
  std::vector<double> chi2;
  vsg_global_ba_result res;
};

// What vsg::ResidentMapPoints::OptimizeEssentialGraph returns: VSim3->estimate() per keyframe (a fixed keyframe, or one
// without an edge: its input), the corrected float position per listed point (also written into its slot), chi2 per edge
// and the counters of vsg_essential_graph_result.
struct EssentialGraphResult {
  std::vector<vsg_sim3d> kfScw;
  std::vector<float> worldPos;
  std::vector<double> chi2;
  vsg_essential_graph_result res;
};

// The edge list of Optimizer::OptimizeEssentialGraph (Optimizer.cc:2529-2660) in the reference's insertion order, host only.
struct EssentialGraphEdges {
  std::vector<int32_t> i, j;  // vertex 0 (nIDi), vertex 1 (nIDj)
  std::vector<uint8_t> loop;  // 1: a "Set Loop edges" edge
};
// Keyframes are the map's !isBad() keyframes in ascending mnId and are named by their index in that order, so `index <`
// is `mnId <`; a pointer to a bad (or null) keyframe is the index -1.  Per keyframe k: parent[k] = GetParent(); its
// GetLoopEdges() are loopIdx[loopOff[k] .. loopOff[k + 1]), its children (hasChild) childIdx[childOff[k] ..), its
// GetCovisiblesByWeight(100) in that vector's order covIdx[covOff[k] ..).  LoopConnections in the map's iteration order:
// entry m is keyframe lcKf[m] with the connections lcIdx[lcOff[m] .. lcOff[m + 1]) in the set's order and
// lcWeight = pKF->GetWeight(connection).  curKF / loopKF = pCurKF / pLoopKF.  The filters are the reference's: :2542
// (minFeat, except the pair current -> loop), :2608 (mnId <), :2634-2639 (not the parent, not a child, not bad, mnId <, not
// in sInsertedEdges).  Two edges between one pair of keyframes are legal and both are listed (a loop connection and a
// spanning-tree edge).  The walk over the keyframes is in index order; the reference's is GetAllKeyFrames()' (the map's
// set, by address), which changes the order of the sums and nothing else.
inline EssentialGraphEdges essential_graph_edges(int nKF, const std::vector<int32_t> &parent, const std::vector<int32_t> &loopOff,
                                                 const std::vector<int32_t> &loopIdx, const std::vector<int32_t> &childOff,
                                                 const std::vector<int32_t> &childIdx, const std::vector<int32_t> &covOff,
                                                 const std::vector<int32_t> &covIdx, const std::vector<int32_t> &lcKf,
                                                 const std::vector<int32_t> &lcOff, const std::vector<int32_t> &lcIdx,
                                                 const std::vector<int32_t> &lcWeight, int curKF, int loopKF, int minFeat = 100) {
  const size_t K = (size_t)(nKF < 0 ? 0 : nKF), M = lcKf.size();
  auto csr_ok = [](const std::vector<int32_t> &off, size_t rows, size_t entries) {
    if (off.size() != rows + 1 || off[0] != 0 || (size_t)off[rows] != entries) return false;
    for (size_t r = 0; r < rows; ++r)
      if (off[r + 1] < off[r]) return false;
    return true;
  };
  if (parent.size() != K || !csr_ok(loopOff, K, loopIdx.size()) || !csr_ok(childOff, K, childIdx.size()) ||
      !csr_ok(covOff, K, covIdx.size()) || !csr_ok(lcOff, M, lcIdx.size()) || lcWeight.size() != lcIdx.size())
    throw std::runtime_error("essential_graph_edges: the arrays' sizes do not match");
  auto in_range = [K](int32_t v) { return v >= -1 && (size_t)(v + 1) <= K; };
  for (const std::vector<int32_t> *v : {&parent, &loopIdx, &childIdx, &covIdx, &lcIdx})
    for (int32_t x : *v)
      if (!in_range(x)) throw std::runtime_error("essential_graph_edges: a keyframe index is out of range");
  for (int32_t x : lcKf)
    if (x < 0 || (size_t)x >= K) throw std::runtime_error("essential_graph_edges: a keyframe index is out of range");
  EssentialGraphEdges E;
  auto push = [&E](int i, int j, int loop) { E.i.push_back(i), E.j.push_back(j), E.loop.push_back((uint8_t)loop); };
  std::set<std::pair<int32_t, int32_t>> inserted;  // sInsertedEdges
  for (size_t m = 0; m < M; ++m) {
    const int32_t i = lcKf[m];
    for (int32_t x = lcOff[m]; x < lcOff[m + 1]; ++x) {
      const int32_t j = lcIdx[(size_t)x];
      if (j < 0 || j == i) continue;  // a bad keyframe has no vertex
      if ((i != curKF || j != loopKF) && lcWeight[(size_t)x] < minFeat) continue;
      push(i, j, 1);
      inserted.insert(std::make_pair(std::min(i, j), std::max(i, j)));
    }
  }
  for (int32_t i = 0; i < (int32_t)K; ++i) {
    const int32_t par = parent[(size_t)i];
    if (par >= 0 && par != i) push(i, par, 0);  // spanning tree
    for (int32_t x = loopOff[(size_t)i]; x < loopOff[(size_t)i + 1]; ++x) {
      const int32_t l = loopIdx[(size_t)x];
      if (l >= 0 && l < i) push(i, l, 0);
    }
    for (int32_t x = covOff[(size_t)i]; x < covOff[(size_t)i + 1]; ++x) {
      const int32_t n = covIdx[(size_t)x];
      if (n < 0 || n == par) continue;
      bool child = false;
      for (int32_t y = childOff[(size_t)i]; y < childOff[(size_t)i + 1]; ++y) child = child || childIdx[(size_t)y] == n;
      if (child || !(n < i)) continue;
      if (inserted.count(std::make_pair(std::min(i, n), std::max(i, n)))) continue;
      push(i, n, 0);
    }
  }
  return E;
}

class ResidentMapPoints {
 public:
  explicit ResidentMapPoints(int capacity, int device = 0) {
    check(vsg_mappoints_create(device, capacity, &mp_), "vsg_mappoints_create");
  }
  ~ResidentMapPoints() { vsg_mappoints_destroy(mp_); }
  ResidentMapPoints(const ResidentMapPoints &) = delete;
  ResidentMapPoints &operator=(const ResidentMapPoints &) = delete;
  int capacity() const { return vsg_mappoints_capacity(mp_); }
  // entry i of every non-null array goes to slot slots[i]; nullptr keeps what the slots hold; a slot listed twice takes
  // its last entry.  worldPos / normal: 3 floats per entry, desc: 32 bytes, observed: Observations() > 0.
  void update(const std::vector<int32_t> &slots, const float *worldPos, const float *normal, const float *minDist,
              const float *maxDist, const uint8_t *desc, const uint8_t *observed) {
    check(vsg_mappoints_update(mp_, (int)slots.size(), slots.data(), worldPos, normal, minDist, maxDist, desc, observed),
          "vsg_mappoints_update");
  }
  // MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth of slots.size() points from their
  // observations, on the device (vsg_mappoints_refresh_from_observations): point i has the observations
  // [obsOff[i], obsOff[i + 1]) of obsKf (index into keyFrames = ResidentFrame::handle() of each keyframe), obsIdx
  // (leftIndex) and obsBad (pKF->isBad(); empty: none); refPos[i] = where mpRefKF's observation sits in that list;
  // kfOw = GetCameraCenter(), 3 floats per keyframe.  what = VSG_REFRESH_DESC | VSG_REFRESH_NORMAL or one of them.
  RefreshResult Refresh(const std::vector<int32_t> &slots, const std::vector<int32_t> &obsOff,
                        const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                        const std::vector<uint8_t> &obsBad, const std::vector<int32_t> &refPos,
                        const std::vector<vsg_frame *> &keyFrames, const std::vector<float> &kfOw,
                        const std::vector<float> &mvScaleFactors, int what = VSG_REFRESH_DESC | VSG_REFRESH_NORMAL) {
    const size_t n = slots.size();
    if (obsOff.size() != n + 1 || refPos.size() != n || obsKf.size() != obsIdx.size() ||
        (!obsBad.empty() && obsBad.size() != obsKf.size()) || kfOw.size() != 3 * keyFrames.size() ||
        (n > 0 && (obsOff[n] < 0 || (size_t)obsOff[n] > obsKf.size())))
      throw std::runtime_error("ResidentMapPoints::Refresh: the arrays' sizes do not match");
    RefreshResult r;
    r.best.assign(n, -1), r.normal.assign(3 * n, 0.0f), r.minDist.assign(n, 0.0f), r.maxDist.assign(n, 0.0f);
    check(vsg_mappoints_refresh_from_observations(mp_, (int)n, slots.data(), obsOff.data(), obsKf.data(), obsIdx.data(),
                                                  obsBad.empty() ? nullptr : obsBad.data(), refPos.data(),
                                                  (int)keyFrames.size(), keyFrames.data(), kfOw.data(),
                                                  mvScaleFactors.data(), (int)mvScaleFactors.size(), what, r.best.data(),
                                                  r.normal.data(), r.minDist.data(), r.maxDist.data()),
          "vsg_mappoints_refresh_from_observations");
    return r;
  }
  // The visual part of Optimizer::LocalBundleAdjustment (Optimizer.cc:1454-2454) on the device
  // (vsg_mappoints_local_bundle_adjustment): point i = slot slots[i] with the observations [obsOff[i], obsOff[i + 1]) of
  // obsKf (index into keyFrames: the local keyframes AND the fixed ones, ascending mnId) and obsIdx (leftIndex), as
  // Refresh takes them, filtered by !pKFi->isBad() && GetMap() == pCurrentMap.  kfTcw = GetPose() per keyframe, kfFixed
  // != 0 for lFixedCameras and the map's initial keyframe, kfCam = fx, fy, cx, cy, mbf.  The points' new positions are
  // written into the slots; follow with Refresh(..., VSG_REFRESH_NORMAL).  Marker, plane, room and door vertices are
  // not part of it: keep the reference routine when the keyframe's local lists of those are not empty.
  LocalBAResult LocalBundleAdjustment(const std::vector<int32_t> &slots, const std::vector<int32_t> &obsOff,
                                      const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                                      const std::vector<vsg_frame *> &keyFrames, const std::vector<vsg_pose_se3> &kfTcw,
                                      const std::vector<uint8_t> &kfFixed, const std::vector<vsg_ba_camera> &kfCam,
                                      const std::vector<float> &mvInvLevelSigma2, int iterations = 10,
                                      const volatile uint8_t *pbStopFlag = nullptr) {
    const size_t n = slots.size(), K = keyFrames.size();
    ba_check_sizes("LocalBundleAdjustment", slots, obsOff, obsKf, obsIdx, K, kfTcw.size(), kfFixed.size(), kfCam.size());
    const size_t E = n ? (size_t)obsOff[n] : 0;
    LocalBAResult r;
    r.kfTcw.resize(K), r.worldPos.assign(3 * n, 0.0f), r.erase.assign(E, 0), r.chi2.assign(E, 0.0);
    vsg_pose_se3d none_kf;
    uint8_t none_erase = 0;
    check(vsg_mappoints_local_bundle_adjustment(mp_, (int)n, slots.data(), obsOff.data(), obsKf.data(), obsIdx.data(), (int)K,
                                                keyFrames.data(), kfTcw.data(), kfFixed.data(), kfCam.data(),
                                                mvInvLevelSigma2.data(), (int)mvInvLevelSigma2.size(), iterations, pbStopFlag,
                                                K ? r.kfTcw.data() : &none_kf, n ? r.worldPos.data() : nullptr,
                                                E ? r.erase.data() : &none_erase, E ? r.chi2.data() : nullptr, &r.res),
          "vsg_mappoints_local_bundle_adjustment");
    // the reference returned before optimize: nothing was written
    if (!r.res.ran) ba_outs_are_inputs(slots, kfTcw, &r.kfTcw, &r.worldPos);
    return r;
  }
  // Optimizer::LocalBundleAdjustment WITH its planes and rooms (vsg_mappoints_local_bundle_adjustment_sgraph): the arguments
  // of LocalBundleAdjustment, then the planes and rooms as SGraphLists names them.  A caller
  // with marginalize_planes or the plane_map_point factor keeps the reference routine.
  SGraphLocalBAResult LocalBundleAdjustmentSGraph(const std::vector<int32_t> &slots, const std::vector<int32_t> &obsOff,
                                                  const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                                                  const std::vector<vsg_frame *> &keyFrames, const std::vector<vsg_pose_se3> &kfTcw,
                                                  const std::vector<uint8_t> &kfFixed, const std::vector<vsg_ba_camera> &kfCam,
                                                  const std::vector<float> &mvInvLevelSigma2, const SGraphLists &sg,
                                                  int iterations = 10, const volatile uint8_t *pbStopFlag = nullptr) {
    const size_t n = slots.size(), K = keyFrames.size(), Pl = sg.planeEq.size() / 4, R = sg.roomCenter.size() / 3;
    ba_check_sizes("LocalBundleAdjustmentSGraph", slots, obsOff, obsKf, obsIdx, K, kfTcw.size(), kfFixed.size(), kfCam.size(),
                   sg.planeEq.size() != 4 * Pl || sg.planeObsOff.size() != Pl + 1 || sg.roomCenter.size() != 3 * R ||
                       sg.roomNWalls.size() != R || sg.roomWall.size() != 4 * R);
    const size_t E = n ? (size_t)obsOff[n] : 0, NO = sg.planeObsOff[Pl] > 0 ? (size_t)sg.planeObsOff[Pl] : 0;
    if (sg.planeObsKf.size() < NO || sg.planeObsLocal.size() < 4 * NO || sg.planeObsG.size() < 16 * NO || sg.wPlaneKf.size() < NO ||
        sg.wPlanePoint.size() < NO)
      throw std::runtime_error("ResidentMapPoints::LocalBundleAdjustmentSGraph: planeObsOff runs past the observation arrays");
    SGraphLocalBAResult r;
    r.kfTcw.resize(K), r.worldPos.assign(3 * n, 0.0f), r.erase.assign(E, 0), r.chi2.assign(E, 0.0);
    r.planeEq = sg.planeEq, r.roomCenter = sg.roomCenter, r.erasePlane.assign(NO, 0);
    r.chi2PlaneKf.assign(NO, 0.0), r.chi2PlanePoint.assign(NO, 0.0);
    vsg_pose_se3d none_kf;
    uint8_t none_erase = 0;
    check(vsg_mappoints_local_bundle_adjustment_sgraph(
              mp_, (int)n, slots.data(), obsOff.data(), obsKf.data(), obsIdx.data(), (int)K, keyFrames.data(), kfTcw.data(),
              kfFixed.data(), kfCam.data(), mvInvLevelSigma2.data(), (int)mvInvLevelSigma2.size(), iterations, pbStopFlag,
              K ? r.kfTcw.data() : &none_kf, n ? r.worldPos.data() : nullptr, E ? r.erase.data() : &none_erase,
              E ? r.chi2.data() : nullptr, (int)Pl, sg.planeEq.data(), sg.planeObsOff.data(), sg.planeObsKf.data(),
              sg.planeObsLocal.data(), sg.planeObsG.data(), sg.wPlaneKf.data(), sg.wPlanePoint.data(), (int)R, sg.roomCenter.data(),
              sg.roomNWalls.data(), sg.roomWall.data(), r.planeEq.data(), r.roomCenter.data(), r.erasePlane.data(),
              NO ? r.chi2PlaneKf.data() : nullptr, NO ? r.chi2PlanePoint.data() : nullptr, &r.res),
          "vsg_mappoints_local_bundle_adjustment_sgraph");
    // the reference returned before optimize: nothing was written
    if (!r.res.local.ran) ba_outs_are_inputs(slots, kfTcw, &r.kfTcw, &r.worldPos);
    return r;
  }
  // The visual part of Optimizer::BundleAdjustment as Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag,
  // nLoopKF, bRobust) calls it (Optimizer.cc:45-287, :500-610) on the device (vsg_mappoints_global_bundle_adjustment): the
  // lists are LocalBundleAdjustment's, with keyFrames = EVERY keyframe of the map with !isBad() in ascending mnId and
  // kfFixed != 0 for mnId == GetInitKFid() alone.  loopKFIsOrigin = (nLoopKF == pMap->GetOriginKF()->mnId): the positions
  // are then written into the slots (follow with Refresh(..., VSG_REFRESH_NORMAL)) and the caller SetPose()s kfTcw;
  // otherwise the store is untouched and the caller keeps kfTcw / worldPos as mTcwGBA / mPosGBA.  Tracking.cc:2652 passes
  // 20, nullptr, true and loopKFIsOrigin = true; LoopClosing.cc:2157 passes 10, &mbStopGBA, false.  Marker, plane, room and
  // door vertices are not part of it: keep the reference routine when the map's lists of those are not empty.
  GlobalBAResult GlobalBundleAdjustment(const std::vector<int32_t> &slots, const std::vector<int32_t> &obsOff,
                                        const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx,
                                        const std::vector<vsg_frame *> &keyFrames, const std::vector<vsg_pose_se3> &kfTcw,
                                        const std::vector<uint8_t> &kfFixed, const std::vector<vsg_ba_camera> &kfCam,
                                        const std::vector<float> &mvInvLevelSigma2, int nIterations = 5,
                                        const volatile uint8_t *pbStopFlag = nullptr, bool bRobust = true,
                                        bool loopKFIsOrigin = false) {
    const size_t n = slots.size(), K = keyFrames.size();
    ba_check_sizes("GlobalBundleAdjustment", slots, obsOff, obsKf, obsIdx, K, kfTcw.size(), kfFixed.size(), kfCam.size());
    const size_t E = n ? (size_t)obsOff[n] : 0;
    GlobalBAResult r;
    r.kfTcw.resize(K), r.worldPos.assign(3 * n, 0.0f), r.included.assign(n, 0), r.chi2.assign(E, 0.0);
    vsg_pose_se3d none_kf;
    uint8_t none_included = 0;
    float none_pos[3];
    check(vsg_mappoints_global_bundle_adjustment(mp_, (int)n, slots.data(), obsOff.data(), obsKf.data(), obsIdx.data(), (int)K,
                                                 keyFrames.data(), kfTcw.data(), kfFixed.data(), kfCam.data(),
                                                 mvInvLevelSigma2.data(), (int)mvInvLevelSigma2.size(), nIterations,
                                                 bRobust ? 1 : 0, loopKFIsOrigin ? 1 : 0, pbStopFlag,
                                                 K ? r.kfTcw.data() : &none_kf, n ? r.worldPos.data() : none_pos,
                                                 n ? r.included.data() : &none_included, E ? r.chi2.data() : nullptr, &r.res),
          "vsg_mappoints_global_bundle_adjustment");
    // no edge or the stop flag: only res and included were written
    if (!r.res.ran) ba_outs_are_inputs(slots, kfTcw, &r.kfTcw, &r.worldPos);
    return r;
  }
  // Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
  // (Optimizer.cc:2456-2734) on the device (vsg_mappoints_optimize_essential_graph).  kfScw = vScw per !isBad() keyframe in
  // ascending mnId (CorrectedSim3's entry where present, else (GetPose(), 1.0)); kfNonCorrected / kfHasNonCorrected =
  // NonCorrectedSim3; kfFixed != 0 for mnId == GetInitKFid(); edges = essential_graph_edges(...); slots / pointRef = every
  // !isBad() map point's slot and nIDr (:2712-2721) as a keyframe index.  The corrected positions are written into the
  // slots; follow with Refresh(..., VSG_REFRESH_NORMAL).  The caller SetPose()s from kfScw (t / s, :2700).  Inertial edges
  // are not part of it, and at most 438 keyframes that are not fixed may have an edge (a dense solve): beyond either, keep the
  // reference routine.
  EssentialGraphResult OptimizeEssentialGraph(const std::vector<vsg_sim3d> &kfScw, const std::vector<vsg_sim3d> &kfNonCorrected,
                                              const std::vector<uint8_t> &kfHasNonCorrected, const std::vector<uint8_t> &kfFixed,
                                              const EssentialGraphEdges &edges, bool bFixScale, const std::vector<int32_t> &slots,
                                              const std::vector<int32_t> &pointRef, int iterations = 20) {
    const size_t K = kfScw.size(), E = edges.i.size(), n = slots.size();
    if (kfNonCorrected.size() != K || kfHasNonCorrected.size() != K || kfFixed.size() != K || edges.j.size() != E ||
        edges.loop.size() != E || pointRef.size() != n)
      throw std::runtime_error("ResidentMapPoints::OptimizeEssentialGraph: the arrays' sizes do not match");
    EssentialGraphResult r;
    r.kfScw.resize(K), r.worldPos.assign(3 * n, 0.0f), r.chi2.assign(E, 0.0);
    vsg_sim3d none_kf;
    check(vsg_mappoints_optimize_essential_graph(mp_, (int)K, kfScw.data(), kfNonCorrected.data(), kfHasNonCorrected.data(),
                                                 kfFixed.data(), (int)E, edges.i.data(), edges.j.data(), edges.loop.data(),
                                                 bFixScale ? 1 : 0, iterations, (int)n, slots.data(), pointRef.data(),
                                                 K ? r.kfScw.data() : &none_kf, n ? r.worldPos.data() : nullptr,
                                                 E ? r.chi2.data() : nullptr, &r.res),
          "vsg_mappoints_optimize_essential_graph");
    if (!r.res.ran && n)  // nothing to optimise: the store was not written, the positions are what the slots hold
      check(vsg_mappoints_read(mp_, (int)n, slots.data(), r.worldPos.data(), nullptr, nullptr, nullptr, nullptr, nullptr),
            "vsg_mappoints_read");
    return r;
  }
  // The point correction of LoopClosing::CorrectLoop (LoopClosing.cc:1060-1064) on the device (vsg_mappoints_correct_sim3):
  // slot slots[i] becomes float(SToInverse[r].map(SFrom[r].map(double(pos)))), r = pointRef[i]; there SFrom = g2oSiw and
  // SToInverse = g2oCorrectedSiw.inverse() of connected keyframe r.  Returns the new positions; follow with
  // Refresh(..., VSG_REFRESH_NORMAL).
  std::vector<float> CorrectSim3(const std::vector<int32_t> &slots, const std::vector<int32_t> &pointRef,
                                 const std::vector<vsg_sim3d> &SFrom, const std::vector<vsg_sim3d> &SToInverse) {
    if (pointRef.size() != slots.size() || SFrom.size() != SToInverse.size())
      throw std::runtime_error("ResidentMapPoints::CorrectSim3: the arrays' sizes do not match");
    std::vector<float> out(3 * slots.size(), 0.0f);
    check(vsg_mappoints_correct_sim3(mp_, (int)slots.size(), slots.data(), pointRef.data(), (int)SFrom.size(), SFrom.data(),
                                     SToInverse.data(), slots.empty() ? nullptr : out.data()),
          "vsg_mappoints_correct_sim3");
    return out;
  }
  vsg_mappoints *handle() const { return mp_; }

 private:
  // the lists and per-keyframe arrays the three bundle adjustments take; `more`: a mismatch among the caller's further arrays
  static void ba_check_sizes(const char *who, const std::vector<int32_t> &slots, const std::vector<int32_t> &obsOff,
                             const std::vector<int32_t> &obsKf, const std::vector<int32_t> &obsIdx, size_t K, size_t nTcw,
                             size_t nFixed, size_t nCam, bool more = false) {
    const size_t n = slots.size();
    if (obsOff.size() != n + 1 || obsKf.size() != obsIdx.size() || nTcw != K || nFixed != K || nCam != K ||
        (n > 0 && (obsOff[n] < 0 || (size_t)obsOff[n] > obsKf.size())) || more)
      throw std::runtime_error(std::string("ResidentMapPoints::") + who + ": the arrays' sizes do not match");
  }
  // a bundle adjustment that did not run wrote no pose and no position: the outs are the inputs
  void ba_outs_are_inputs(const std::vector<int32_t> &slots, const std::vector<vsg_pose_se3> &kfTcw,
                          std::vector<vsg_pose_se3d> *kfOut, std::vector<float> *worldPos) {
    for (size_t k = 0; k < kfTcw.size(); ++k)
      for (int d = 0; d < 7; ++d) (d < 4 ? (*kfOut)[k].q[d] : (*kfOut)[k].t[d - 4]) = d < 4 ? kfTcw[k].q[d] : kfTcw[k].t[d - 4];
    if (!slots.empty())
      check(vsg_mappoints_read(mp_, (int)slots.size(), slots.data(), worldPos->data(), nullptr, nullptr, nullptr, nullptr, nullptr),
            "vsg_mappoints_read");
  }
  vsg_mappoints *mp_ = nullptr;
};

// mbTrackInView, mTrackProjX / Y / XR, mTrackDepth, mnTrackScaleLevel, mTrackViewCos of the queried map points
struct FrustumResult {
  std::vector<uint8_t> inView;
  std::vector<float> projX, projY, projXR, depth, viewCos;
  std::vector<int32_t> scaleLevel;
};

// What Tracking::SearchLocalPoints leaves behind: the matches (feature -> index into the queried map points, -1 = none),
// nToMatch, and per map point mbTrackInView with the projection mmProjectPoints takes (Tracking.cc:3462-3465)
struct LocalPointsResult {
  std::vector<int32_t> trainMatch;
  std::vector<uint8_t> inView;
  std::vector<float> projX, projY;
  int nToMatch = 0;
};

class ResidentFrame {
 public:
  explicit ResidentFrame(int capacity, int device = 0) {
    check(vsg_frame_create(device, capacity, &f_), "vsg_frame_create");
  }
  ~ResidentFrame() { vsg_frame_destroy(f_); }
  ResidentFrame(const ResidentFrame &) = delete;
  ResidentFrame &operator=(const ResidentFrame &) = delete;
  // keys = mvKeysUn (Nleft == -1) or mvKeys followed by mvKeysRight; uRight = mvuRight.data() or nullptr
  void Upload(const vsg_keypoint *keys, const uint8_t *desc, const float *uRight, int N, int Nleft, float mnMinX,
              float mnMinY, float mnMaxX, float mnMaxY) {
    check(vsg_frame_upload(f_, keys, desc, uRight, N, Nleft, mnMinX, mnMinY, mnMaxX, mnMaxY), "vsg_frame_upload");
  }
  // straight out of the extractor that just ran (no distortion: mvKeysUn == mvKeys)
  void FromExtractor(const ORBextractor &ex, const std::vector<vsg_keypoint> &keys, float mnMinX, float mnMinY,
                     float mnMaxX, float mnMaxY, int index = 0) {
    check(vsg_frame_from_extractor(f_, ex.handle(), index, keys.data(), (int)keys.size(), mnMinX, mnMinY, mnMaxX, mnMaxY),
          "vsg_frame_from_extractor");
  }
  // The same for a distorted pinhole camera (mDistCoef(0) != 0: TUM1.yaml, RealSense_D435i.yaml): UndistortKeyPoints
  // (Frame.cc:891-921) runs on the device inside the grid launch; mvKeysUn comes back for the host's own use.
  // K4 = {fx, fy, cx, cy} of mK, dist = mDistCoef's 4 or 5 floats, bounds = ImageBounds(...) below.
  void FromExtractorUndistort(const ORBextractor &ex, const std::vector<vsg_keypoint> &mvKeys, const float K4[4],
                              const float *dist, int ndist, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY,
                              std::vector<vsg_keypoint> *mvKeysUn, int index = 0) {
    if (mvKeysUn) mvKeysUn->resize(mvKeys.size());
    check(vsg_frame_from_extractor_undistort(f_, ex.handle(), index, mvKeys.data(), (int)mvKeys.size(), K4, dist, ndist,
                                             mnMinX, mnMinY, mnMaxX, mnMaxY, mvKeysUn ? mvKeysUn->data() : nullptr),
          "vsg_frame_from_extractor_undistort");
  }
  // ExtractORB + UndistortKeyPoints + AssignFeaturesToGrid in one call and one wait (vsg_orb_extract_to_frame): the
  // front end of the monocular / RGB-D Frame constructors.  Returns monoIndex; mvKeys / descriptors sized to N.
  int ExtractInto(ORBextractor &ex, const uint8_t *gray, int rows, int cols, int stride, const int lapping[2],
                  std::vector<vsg_keypoint> &mvKeys, std::vector<uint8_t> &descriptors, const float K4[4],
                  const float *dist, int ndist, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY,
                  std::vector<vsg_keypoint> *mvKeysUn) {
    const int cap = vsg_orb_capacity(ex.handle(), rows, cols);
    check(cap, "vsg_orb_capacity");
    mvKeys.resize(cap), descriptors.resize((size_t)cap * 32);
    if (mvKeysUn) mvKeysUn->resize(cap);
    int n = 0;
    const int mono = vsg_orb_extract_to_frame(ex.handle(), gray, rows, cols, stride, lapping[0], lapping[1], mvKeys.data(),
                                              descriptors.data(), cap, &n, f_, K4, dist, ndist, mnMinX, mnMinY, mnMaxX,
                                              mnMaxY, mvKeysUn ? mvKeysUn->data() : nullptr);
    check(mono, "vsg_orb_extract_to_frame");
    mvKeys.resize(n), descriptors.resize((size_t)n * 32);
    if (mvKeysUn) mvKeysUn->resize(n);
    return mono;
  }
  // The RGB-D Frame constructor's front end (vsg_orb_extract_to_frame_rgbd): ExtractInto + GrabImageRGBD's depth
  // conversion + ComputeStereoFromRGBD (Frame.cc:1129-1150), one call and one wait.  depth: rows x cols of
  // VSG_DEPTH_U16 / VSG_DEPTH_F32, depthStride bytes per row; depthMapFactor = DepthMapScale(RGBD.DepthMapFactor);
  // mbf = Frame::mbf.  The resident frame carries mvuRight; mvuRight / mvDepth come back sized to N.
  int ExtractIntoRGBD(ORBextractor &ex, const uint8_t *gray, int rows, int cols, int stride, const int lapping[2],
                      const void *depth, int depthType, size_t depthStride, float depthMapFactor, float mbf,
                      std::vector<vsg_keypoint> &mvKeys, std::vector<uint8_t> &descriptors, const float K4[4],
                      const float *dist, int ndist, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY,
                      std::vector<vsg_keypoint> *mvKeysUn, std::vector<float> &mvuRight, std::vector<float> &mvDepth) {
    const int cap = vsg_orb_capacity(ex.handle(), rows, cols);
    check(cap, "vsg_orb_capacity");
    mvKeys.resize(cap), descriptors.resize((size_t)cap * 32), mvuRight.resize(cap), mvDepth.resize(cap);
    if (mvKeysUn) mvKeysUn->resize(cap);
    int n = 0;
    const int mono = vsg_orb_extract_to_frame_rgbd(
        ex.handle(), gray, rows, cols, stride, lapping[0], lapping[1], mvKeys.data(), descriptors.data(), cap, &n, f_, K4,
        dist, ndist, mnMinX, mnMinY, mnMaxX, mnMaxY, mvKeysUn ? mvKeysUn->data() : nullptr, depth, depthType,
        depthStride, rows, cols, depthMapFactor, mbf, mvuRight.data(), mvDepth.data());
    check(mono, "vsg_orb_extract_to_frame_rgbd");
    mvKeys.resize(n), descriptors.resize((size_t)n * 32), mvuRight.resize(n), mvDepth.resize(n);
    if (mvKeysUn) mvKeysUn->resize(n);
    return mono;
  }
  // Tracking's mDepthMapFactor from the settings' RGBD.DepthMapFactor (Tracking.cc:638-642)
  static float DepthMapScale(float yamlDepthMapFactor) { return vsg_depth_map_scale(yamlDepthMapFactor); }
  // Frame::ComputeImageBounds (Frame.cc:924-955): {mnMinX, mnMinY, mnMaxX, mnMaxY}
  static void ImageBounds(int cols, int rows, const float K4[4], const float *dist, int ndist, float out[4]) {
    check(vsg_camera_image_bounds(cols, rows, K4, dist, ndist, out), "vsg_camera_image_bounds");
  }
  int N() const { return vsg_frame_size(f_); }
  vsg_frame *handle() const { return f_; }
  // The per-keyframe inputs of CreateNewMapPoints' stereo branches (vsg_frame_set_stereo_points), once per keyframe:
  // x3Dc[3 i ..] = x3Dc of KeyFrame::UnprojectStereo(i) (KeyFrame.cc:887-894, from mvKeys and mvDepth), cosParallax[i] =
  // cos(2 * atan2(mb / 2, mvDepth[i])) (LocalMapping.cc:569); entries of keypoints with mvuRight < 0 are never read.
  void SetStereoPoints(const std::vector<float> &x3Dc, const std::vector<float> &cosParallax) {
    if (x3Dc.size() < 3 * (size_t)N() || cosParallax.size() < (size_t)N()) check(VSG_ERR_INVALID, "vsg_frame_set_stereo_points");
    static const float none[3] = {0.0f, 0.0f, 0.0f};
    check(vsg_frame_set_stereo_points(f_, x3Dc.empty() ? none : x3Dc.data(), cosParallax.empty() ? none : cosParallax.data()),
          "vsg_frame_set_stereo_points");
  }

  // Frame::GetFeaturesInArea / KeyFrame::GetFeaturesInArea for many windows at once
  Candidates GetFeaturesInArea(const float *x, const float *y, const float *r, const int32_t *minLevel,
                               const int32_t *maxLevel, int nq, bool bRight = false) const {
    Candidates c;
    c.off.resize(nq + 1);
    c.idx.resize(32 * (size_t)nq + 64);
    int total = vsg_frame_features_in_area(f_, x, y, r, minLevel, maxLevel, bRight, nq, c.off.data(), c.idx.data(),
                                           (int)c.idx.size());
    check(total, "vsg_frame_features_in_area");
    if (total > (int)c.idx.size()) {
      c.idx.resize(total);
      check(vsg_frame_features_in_area(f_, x, y, r, minLevel, maxLevel, bRight, nq, c.off.data(), c.idx.data(), total),
            "vsg_frame_features_in_area");
    }
    c.idx.resize(total);
    return c;
  }

  // bool Frame::isInFrustum(MapPoint *pMP, float viewingCosLimit) (Frame.cc:656-719) for the map points in `slots`
  // (nullptr: slots 0 .. n-1).  Nleft != -1 frames throw (VSG_ERR_UNSUPPORTED).
  void isInFrustum(const ResidentMapPoints &mp, int n, const int32_t *slots, const FramePose &pose, float viewingCosLimit,
                   FrustumResult &out) const {
    const size_t m = n > 0 ? n : 1;
    out.inView.assign(m, 0), out.projX.assign(m, -1.f), out.projY.assign(m, -1.f), out.projXR.assign(m, 0.f);
    out.depth.assign(m, 0.f), out.viewCos.assign(m, 0.f), out.scaleLevel.assign(m, 0);
    check(vsg_frame_is_in_frustum(f_, mp.handle(), n, slots, &pose, viewingCosLimit, out.inView.data(), out.projX.data(),
                                  out.projY.data(), out.projXR.data(), out.depth.data(), out.scaleLevel.data(),
                                  out.viewCos.data()),
          "vsg_frame_is_in_frustum");
    out.inView.resize(n), out.projX.resize(n), out.projY.resize(n), out.projXR.resize(n), out.depth.resize(n);
    out.viewCos.resize(n), out.scaleLevel.resize(n);
  }

  // Tracking::SearchLocalPoints' second loop and its SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th, bFarPoints,
  // thFarPoints) (Tracking.cc:3446-3493) in one call and one wait.  skip[i] != 0 = mnLastFrameSeen == mnId || isBad()
  // (nullptr: none); trainBlocked[i] = mvpMapPoints[i] && Observations() > 0 (in / out).  Returns nmatches.
  int SearchLocalPoints(const ResidentMapPoints &mp, int n, const int32_t *slots, const uint8_t *skip, const FramePose &pose,
                        float th, float nnratio, bool bFarPoints, float thFarPoints,
                        const std::vector<float> &mvScaleFactors, std::vector<uint8_t> &trainBlocked,
                        LocalPointsResult &out, float viewingCosLimit = 0.5f) const {
    const size_t m = n > 0 ? n : 1;
    out.trainMatch.assign(N() > 0 ? N() : 1, -1);
    trainBlocked.resize(out.trainMatch.size(), 0);
    out.inView.assign(m, 0), out.projX.assign(m, -1.f), out.projY.assign(m, -1.f);
    const int rc = vsg_frame_search_local_points(f_, mp.handle(), n, slots, skip, &pose, viewingCosLimit, th, nnratio,
                                                 bFarPoints ? 1 : 0, thFarPoints, mvScaleFactors.data(),
                                                 (int)mvScaleFactors.size(), trainBlocked.data(), out.trainMatch.data(),
                                                 out.inView.data(), out.projX.data(), out.projY.data(), &out.nToMatch);
    check(rc, "vsg_frame_search_local_points");
    out.trainMatch.resize(N()), trainBlocked.resize(N());
    out.inView.resize(n), out.projX.resize(n), out.projY.resize(n);
    return rc;
  }

  // int Optimizer::PoseOptimization(Frame *pFrame) (Optimizer.cc:1063-1452) in one call and one wait
  // (vsg_frame_pose_optimization).  featSlots[i] = the slot of pFrame->mvpMapPoints[i] or < 0, one per feature; Tcw =
  // pFrame->GetPose() (unit_quaternion() as x y z w, translation()); camera = fx, fy, cx, cy, mbf; outlier = mvbOutlier,
  // written only for features with a slot.  out.q / out.t make the Sophus::SE3f of :1447 for pFrame->SetPose.  Returns
  // nInitialCorrespondences - nBad.  holdForPlaneStep: stop after round 2's optimize() (out.held: run the
  // refine_map_points step of :1270-1335 on out.qd / out.td, then PoseOptimizationResume with the features it dropped;
  // not held: fewer than 10 edges, the call is complete).
  struct PoseOptResult {
    float q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};   // SE3quat_recov.rotation().cast<float>(), translation().cast<float>()
    double qd[4] = {0, 0, 0, 1}, td[3] = {0, 0, 0};  // vSE3_recov->estimate()
    int nInitialCorrespondences = 0, nBad = 0, roundsRun = 0;
    bool held = false;
  };
  int PoseOptimization(const ResidentMapPoints &mp, const std::vector<int32_t> &featSlots, const vsg_pose_se3 &Tcw,
                       const float camera[5], const std::vector<float> &invLevelSigma2, std::vector<uint8_t> &outlier,
                       PoseOptResult &out, bool holdForPlaneStep = false, std::vector<float> *chi2 = nullptr) const {
    if ((int)featSlots.size() != N()) throw std::runtime_error("PoseOptimization: one slot per feature");
    outlier.resize(featSlots.size() ? featSlots.size() : 1, 0);
    if (chi2) chi2->resize(outlier.size(), 0.f);
    vsg_pose_result res;
    const int rc = vsg_frame_pose_optimization(f_, mp.handle(), featSlots.data(), &Tcw, camera[0], camera[1], camera[2],
                                               camera[3], camera[4], invLevelSigma2.data(), (int)invLevelSigma2.size(),
                                               holdForPlaneStep ? 2 : -1, outlier.data(), chi2 ? chi2->data() : nullptr, &res);
    check(rc, "vsg_frame_pose_optimization");
    return poseResult(rc, res, featSlots.size(), outlier, chi2, out);
  }
  // removed[i] != 0: the plane step set mvpMapPoints[i] = NULL and mvbOutlier[i] = true (nullptr: none)
  int PoseOptimizationResume(const std::vector<uint8_t> *removed, std::vector<uint8_t> &outlier, PoseOptResult &out,
                             std::vector<float> *chi2 = nullptr) const {
    const size_t n = (size_t)N();
    if (removed && removed->size() != n) throw std::runtime_error("PoseOptimizationResume: one flag per feature");
    outlier.resize(n ? n : 1, 0);
    if (chi2) chi2->resize(outlier.size(), 0.f);
    vsg_pose_result res;
    const int rc = vsg_frame_pose_optimization_resume(f_, removed ? removed->data() : nullptr, outlier.data(),
                                                      chi2 ? chi2->data() : nullptr, &res);
    check(rc, "vsg_frame_pose_optimization_resume");
    return poseResult(rc, res, n, outlier, chi2, out);
  }

  // bool Tracking::TrackWithMotionModel() (Tracking.cc:2945-3005) in one call and one wait
  // (vsg_frame_track_with_motion_model): this = mCurrentFrame, last = the resident mLastFrame, lastSlots[i] = the slot of
  // its mvpMapPoints[i] (< 0: none, or an outlier); Tcw = the predicted pose, the solve's camera is curPose's.  featSlots =
  // mvpMapPoints after the discard loop, outlier = mvbOutlier (written for matched features only).  Returns nmatches after
  // the discard; the caller applies :3007-3016 to out.nMatches / out.nMatchesMap.
  struct TrackMotionResult {
    PoseOptResult pose;
    std::vector<int32_t> featSlots, trainMatch;
    int nSearch = 0, nMatchesSearched = 0, nMatches = 0, nMatchesMap = 0, direction = 0;
    bool wide = false, optimized = false;
  };
  int TrackWithMotionModel(const ResidentFrame &last, const ResidentMapPoints &mp, const std::vector<int32_t> &lastSlots,
                           const FramePose &curPose, const FramePose &lastPose, float mb, bool bMono, float th,
                           const std::vector<float> &mvScaleFactors, bool checkOrientation, const vsg_pose_se3 &Tcw,
                           const std::vector<float> &invLevelSigma2, std::vector<uint8_t> &outlier, TrackMotionResult &out,
                           bool holdForPlaneStep = false, std::vector<float> *chi2 = nullptr) const {
    if ((int)lastSlots.size() != last.N()) throw std::runtime_error("TrackWithMotionModel: one slot per last-frame feature");
    if (invLevelSigma2.size() != mvScaleFactors.size())
      throw std::runtime_error("TrackWithMotionModel: one sigma per pyramid level");
    const size_t n = (size_t)N(), m = n ? n : 1;
    static const int32_t none = -1;
    outlier.resize(m, 0), out.featSlots.assign(m, -1), out.trainMatch.assign(m, -1);
    if (chi2) chi2->resize(m, 0.f);
    vsg_track_result res;
    const int rc = vsg_frame_track_with_motion_model(
        f_, last.handle(), mp.handle(), lastSlots.empty() ? &none : lastSlots.data(), &curPose, &lastPose, mb, bMono ? 1 : 0,
        th, mvScaleFactors.data(), (int)mvScaleFactors.size(), checkOrientation ? 1 : 0, &Tcw, invLevelSigma2.data(),
        holdForPlaneStep ? 2 : -1, out.featSlots.data(), out.trainMatch.data(), outlier.data(),
        chi2 ? chi2->data() : nullptr, &res);
    check(rc, "vsg_frame_track_with_motion_model");
    out.featSlots.resize(n), out.trainMatch.resize(n);
    out.nSearch = res.n_search, out.nMatchesSearched = res.n_matches_searched, out.nMatches = res.n_matches;
    out.nMatchesMap = res.n_matches_map, out.direction = res.direction;
    out.wide = res.wide != 0, out.optimized = res.optimized != 0;
    return poseResult(rc, res.pose, n, outlier, chi2, out.pose);
  }

  // bool Tracking::TrackLocalMap() (Tracking.cc:3019-3131) from SearchLocalPoints' second loop to the statistics loop in
  // one call and one wait (vsg_frame_track_local_map).  featSlotsIn[i] = the slot of mvpMapPoints[i] on entry (< 0: none;
  // a bad point is the caller's to clear, :3426-3443), skip[i] != 0 = mnLastFrameSeen == mnId || isBad() (nullptr: none).
  // out.featSlots = mvpMapPoints after the search and, with dropOutliers (mSensor == System::STEREO), the drop of :3093;
  // outlier = mvbOutlier, written for features that hold a point after the search.  out.inView drives IncreaseVisible,
  // a feature with a slot and no outlier flag IncreaseFound.  Returns mnMatchesInliers (0 when held: the caller runs the
  // plane step, PoseOptimizationResume and the loop of :3074-3095 itself).
  struct TrackLocalResult {
    PoseOptResult pose;
    std::vector<int32_t> featSlots, trainMatch;
    std::vector<uint8_t> inView;
    std::vector<float> projX, projY;
    int nToMatch = 0, nMatchesSearched = 0, nMatchesInliers = 0, walkRounds = 0;
  };
  int TrackLocalMap(const ResidentMapPoints &mp, int n, const int32_t *slots, const uint8_t *skip, const FramePose &pose,
                    float th, float nnratio, bool bFarPoints, float thFarPoints, const std::vector<float> &mvScaleFactors,
                    const std::vector<int32_t> &featSlotsIn, const vsg_pose_se3 &Tcw,
                    const std::vector<float> &invLevelSigma2, bool bOnlyTracking, bool dropOutliers,
                    std::vector<uint8_t> &outlier, TrackLocalResult &out, bool holdForPlaneStep = false,
                    std::vector<float> *chi2 = nullptr, float viewingCosLimit = 0.5f) const {
    if ((int)featSlotsIn.size() != N()) throw std::runtime_error("TrackLocalMap: one slot per feature");
    if (invLevelSigma2.size() != mvScaleFactors.size()) throw std::runtime_error("TrackLocalMap: one sigma per pyramid level");
    const size_t nf = (size_t)N(), mf = nf ? nf : 1, m = n > 0 ? n : 1;
    static const int32_t none = -1;
    outlier.resize(mf, 0), out.featSlots.assign(mf, -1), out.trainMatch.assign(mf, -1);
    if (chi2) chi2->resize(mf, 0.f);
    out.inView.assign(m, 0), out.projX.assign(m, -1.f), out.projY.assign(m, -1.f);
    vsg_track_local_result res;
    const int rc = vsg_frame_track_local_map(
        f_, mp.handle(), n, slots, skip, &pose, viewingCosLimit, th, nnratio, bFarPoints ? 1 : 0, thFarPoints,
        mvScaleFactors.data(), (int)mvScaleFactors.size(), featSlotsIn.empty() ? &none : featSlotsIn.data(), &Tcw,
        invLevelSigma2.data(), holdForPlaneStep ? 2 : -1, bOnlyTracking ? 1 : 0, dropOutliers ? 1 : 0, out.featSlots.data(),
        out.trainMatch.data(), outlier.data(), chi2 ? chi2->data() : nullptr, out.inView.data(), out.projX.data(),
        out.projY.data(), &res);
    check(rc, "vsg_frame_track_local_map");
    out.featSlots.resize(nf), out.trainMatch.resize(nf);
    out.inView.resize(n > 0 ? n : 0), out.projX.resize(n > 0 ? n : 0), out.projY.resize(n > 0 ? n : 0);
    out.nToMatch = res.n_to_match, out.nMatchesSearched = res.n_matches_searched;
    out.nMatchesInliers = res.n_matches_inliers, out.walkRounds = res.walk_rounds;
    poseResult(rc, res.pose, nf, outlier, chi2, out.pose);
    return rc;
  }

 private:
  static int poseResult(int rc, const vsg_pose_result &res, size_t n, std::vector<uint8_t> &outlier,
                        std::vector<float> *chi2, PoseOptResult &out) {
    for (int k = 0; k < 4; ++k) out.qd[k] = res.q[k], out.q[k] = (float)res.q[k];
    for (int k = 0; k < 3; ++k) out.td[k] = res.t[k], out.t[k] = (float)res.t[k];
    out.nInitialCorrespondences = res.n_initial, out.nBad = res.n_bad, out.roundsRun = res.rounds_run;
    out.held = res.held != 0;
    outlier.resize(n);
    if (chi2) chi2->resize(n);
    return rc;
  }
  vsg_frame *f_ = nullptr;
};

// The stereo Frame constructor's tail and the first tracking step in ONE call and one wait (vsg_frame_stereo_bow_search):
// ComputeStereoMatches (Frame.cc:957-1127) -> ComputeBoW (Frame.cc:882-889) -> SearchByBoW(pKF, F) (ORBmatcher.cc:226-428;
// Tracking::TrackReferenceKeyFrame, Tracking.cc:2766-2777).  left / right = the extractors that just processed the two eyes,
// fl / fr = their resident features; pKF = nullptr: no search (the first Frame).  Returns the number of BoW matches.
struct StereoBowResult {
  std::vector<float> mvuRight, mvDepth;
  int nStereo = 0;
  std::map<unsigned, double> mBowVec;
  FeatureVectorCSR mFeatVec;
  std::vector<int32_t> matchF;  // per feature of F: index of the KeyFrame feature whose map point it takes, or -1
};
inline int StereoBowSearch(const ORBextractor &left, const ORBextractor &right, ResidentFrame &fl, ResidentFrame &fr, float mb,
                           float mbf, const ORBVocabulary &voc, ResidentFrame *pKF, const uint8_t *kfValid, float nnratio,
                           bool checkOri, StereoBowResult &out, int levelsup = 4) {
  const int n = fl.N(), cap = n > 0 ? n : 1;
  out.mvuRight.assign(cap, -1.f), out.mvDepth.assign(cap, -1.f), out.matchF.assign(cap, -1);
  std::vector<int32_t> ids(cap);
  std::vector<double> vals(cap);
  out.mFeatVec.node.assign(cap, 0), out.mFeatVec.off.assign(cap + 1, 0), out.mFeatVec.idx.assign(cap, 0);
  int nb = 0, nf = 0, nm = 0;
  check(vsg_frame_stereo_bow_search(left.handle(), 0, right.handle(), 0, fl.handle(), fr.handle(), mb, mbf, out.mvuRight.data(),
                                    out.mvDepth.data(), &out.nStereo, voc.handle(), levelsup, ids.data(), vals.data(), cap, &nb,
                                    out.mFeatVec.node.data(), out.mFeatVec.off.data(), out.mFeatVec.idx.data(), cap, &nf,
                                    pKF ? pKF->handle() : nullptr, kfValid, nnratio, checkOri ? 1 : 0, out.matchF.data(), &nm),
        "vsg_frame_stereo_bow_search");
  out.mBowVec.clear();
  for (int i = 0; i < nb; ++i) out.mBowVec.emplace_hint(out.mBowVec.end(), (unsigned)ids[i], vals[i]);
  out.mFeatVec.node.resize(nf), out.mFeatVec.off.resize(nf + 1), out.mFeatVec.idx.resize(out.mFeatVec.off[nf]);
  out.mvuRight.resize(n), out.mvDepth.resize(n), out.matchF.resize(n);
  return nm;
}

// Projected map points as the routines' geometry code leaves them (one entry per point that passed the routine's
// visibility / distance tests); see include/vsg_orb.h for which members each search reads.
struct ProjectedPoints {
  std::vector<uint8_t> desc;       // n x 32: pMP->GetDescriptor()
  std::vector<uint8_t> observed;   // pMP->Observations() > 0
  std::vector<float> u, v, ur;     // projection (ur = u - mbf * invz where the routine uses it)
  std::vector<float> radius;       // th * mvScaleFactors[level]
  std::vector<int32_t> level;      // nPredictedLevel / nLastOctave
  std::vector<float> angle;        // keypoint angle of the source feature (rotation check)
  std::vector<float> uR, vR;       // right-camera projection (Nleft != -1)
  int n() const { return (int)level.size(); }
};

// The remaining ORBmatcher searches on resident frames (ORBmatcher.h:44-87).  Outputs are feature -> query-index maps;
// the maintainer's glue writes the MapPoint* assignments back.
// What one neighbour of LocalMapping::CreateNewMapPoints leaves behind (vsg_frame_triangulate_matches /
// vsg_frame_create_new_map_points): per feature of mpCurrentKeyFrame the reason (VSG_TRI_*), the source (VSG_TRI_FROM_*: what
// countStereo counts), x3D and the slot of the point it created (-1: none); vMatchedIndices after the rotation filter.
struct NewMapPointsResult {
  std::vector<uint8_t> reason, source;
  std::vector<float> x3D;  // 3 per feature
  std::vector<int32_t> newSlot;
  std::vector<std::pair<size_t, size_t>> vMatchedIndices;
  int nCreated = 0, nMatches = 0;
  void resize(int n) {
    const size_t m = n > 0 ? (size_t)n : 1;
    reason.assign(m, 0), source.assign(m, 0), x3D.assign(3 * m, 0.0f), newSlot.assign(m, -1);
    vMatchedIndices.clear();
    nCreated = nMatches = 0;
  }
};

class ResidentMatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
  explicit ResidentMatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

  // SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, th, bMono)  (ORBmatcher.cc:1667-1878)
  // direction: 0 neither, 1 bForward, 2 bBackward.  trainBlocked[i] = mvpMapPoints[i] && Observations() > 0 (in/out).
  int SearchByProjection(ResidentFrame &CurrentFrame, const ProjectedPoints &last, float th, int direction,
                         const std::vector<float> &mvScaleFactors, std::vector<uint8_t> &trainBlocked,
                         std::vector<int32_t> &trainMatch) const {
    trainMatch.assign(CurrentFrame.N(), -1);
    trainBlocked.resize(CurrentFrame.N(), 0);
    int rc = vsg_frame_search_by_projection_last(
        CurrentFrame.handle(), last.n(), last.desc.data(), last.observed.data(), last.u.data(), last.v.data(),
        last.ur.empty() ? nullptr : last.ur.data(), last.uR.empty() ? nullptr : last.uR.data(),
        last.vR.empty() ? nullptr : last.vR.data(), last.level.data(), last.angle.data(), th, direction,
        mvScaleFactors.data(), (int)mvScaleFactors.size(), mbCheckOrientation, trainBlocked.data(), trainMatch.data());
    check(rc, "vsg_frame_search_by_projection_last");
    return rc;
  }

  // SearchByProjection(KeyFrame *pKF, Sim3f &Scw, vpPoints, vpMatched, th, ratioHamming)  (ORBmatcher.cc:430-528) and
  // its twin with vpPointsKFs / vpMatchedKF (:530-641): matched[i] != -1 = vpMatched[i] is set; new entries = query index
  int SearchByProjection(ResidentFrame &pKF, const ProjectedPoints &pts, float ratioHamming,
                         std::vector<int32_t> &matched) const {
    matched.resize(pKF.N(), -1);
    int rc = vsg_frame_search_by_projection_sim3(pKF.handle(), pts.n(), pts.desc.data(), pts.u.data(), pts.v.data(),
                                                 pts.radius.data(), pts.level.data(), ratioHamming, matched.data());
    check(rc, "vsg_frame_search_by_projection_sim3");
    return rc;
  }

  // SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, sAlreadyFound, th, ORBdist)  (ORBmatcher.cc:1880-2000)
  int SearchByProjection(ResidentFrame &CurrentFrame, const ProjectedPoints &kfPoints, int ORBdist,
                         std::vector<uint8_t> &occupied, std::vector<int32_t> &trainMatch) const {
    trainMatch.assign(CurrentFrame.N(), -1);
    occupied.resize(CurrentFrame.N(), 0);
    int rc = vsg_frame_search_by_projection_kf(CurrentFrame.handle(), kfPoints.n(), kfPoints.desc.data(),
                                               kfPoints.u.data(), kfPoints.v.data(), kfPoints.radius.data(),
                                               kfPoints.level.data(), kfPoints.angle.data(), ORBdist,
                                               mbCheckOrientation, occupied.data(), trainMatch.data());
    check(rc, "vsg_frame_search_by_projection_kf");
    return rc;
  }

  // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
  // (ORBmatcher.h:50, ORBmatcher.cc:1667-1878) with the geometry on the device (vsg_frame_search_last_frame): LastFrame is
  // resident, lastSlots[i] = the slot of LastFrame.mvpMapPoints[i] in mp, or -1 for "no map point, or mvbOutlier[i]".
  // curPose / lastPose = the two frames' GetPose() as FramePose; mb = CurrentFrame.mb.  trainMatch[i2] = the LAST-FRAME
  // feature whose map point CurrentFrame's feature i2 takes.  The retry of Tracking.cc:2956-2961 is the same call with
  // 2 * th.  out (optional): bForward / bBackward as 1 / 2, and per last-frame feature projected, u, v, ur.
  struct LastFrameProjection {
    int direction = 0;
    std::vector<uint8_t> projected;
    std::vector<float> u, v, ur;
  };
  int SearchByProjection(ResidentFrame &CurrentFrame, ResidentFrame &LastFrame, const ResidentMapPoints &mp,
                         const std::vector<int32_t> &lastSlots, const FramePose &curPose, const FramePose &lastPose, float mb,
                         float th, bool bMono, const std::vector<float> &mvScaleFactors, std::vector<uint8_t> &trainBlocked,
                         std::vector<int32_t> &trainMatch, LastFrameProjection *out = nullptr) const {
    const int n = LastFrame.N();
    if ((int)lastSlots.size() != n) check(VSG_ERR_INVALID, "vsg_frame_search_last_frame");
    trainMatch.assign(CurrentFrame.N() > 0 ? CurrentFrame.N() : 1, -1);
    trainBlocked.resize(trainMatch.size(), 0);
    const size_t m = n > 0 ? n : 1;
    if (out) out->projected.assign(m, 0), out->u.assign(m, 0.f), out->v.assign(m, 0.f), out->ur.assign(m, 0.f);
    std::vector<int32_t> none(1, -1);
    const int rc = vsg_frame_search_last_frame(
        CurrentFrame.handle(), LastFrame.handle(), mp.handle(), n ? lastSlots.data() : none.data(), &curPose, &lastPose, mb,
        bMono ? 1 : 0, th, mvScaleFactors.data(), (int)mvScaleFactors.size(), mbCheckOrientation, trainBlocked.data(),
        trainMatch.data(), out ? &out->direction : nullptr, out ? out->projected.data() : nullptr,
        out ? out->u.data() : nullptr, out ? out->v.data() : nullptr, out ? out->ur.data() : nullptr);
    check(rc, "vsg_frame_search_last_frame");
    trainMatch.resize(CurrentFrame.N()), trainBlocked.resize(CurrentFrame.N());
    if (out) out->projected.resize(n), out->u.resize(n), out->v.resize(n), out->ur.resize(n);
    return rc;
  }

  // int SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint *> &sAlreadyFound, const float th,
  // const int ORBdist) (ORBmatcher.h:54, ORBmatcher.cc:1880-2000) with the geometry on the device
  // (vsg_frame_search_keyframe_points): slots[i] = the slot of the i-th map point of pKF->GetMapPointMatches(), kfAngle[i] =
  // pKF->mvKeysUn[.].angle of its feature, skip[i] != 0 = isBad() || sAlreadyFound.count(pMP) (nullptr: none).
  // occupied[i2] = CurrentFrame.mvpMapPoints[i2] != NULL (in / out); trainMatch[i2] = query index.
  struct KeyFrameProjection {
    std::vector<uint8_t> projected;
    std::vector<float> u, v;
    std::vector<int32_t> level;
  };
  int SearchByProjection(ResidentFrame &CurrentFrame, const ResidentMapPoints &mp, const std::vector<int32_t> &slots,
                         const std::vector<float> &kfAngle, const uint8_t *skip, const FramePose &pose, float th, int ORBdist,
                         const std::vector<float> &mvScaleFactors, std::vector<uint8_t> &occupied,
                         std::vector<int32_t> &trainMatch, KeyFrameProjection *out = nullptr) const {
    const int n = (int)slots.size();
    if (mbCheckOrientation && (int)kfAngle.size() != n) check(VSG_ERR_INVALID, "vsg_frame_search_keyframe_points");
    trainMatch.assign(CurrentFrame.N() > 0 ? CurrentFrame.N() : 1, -1);
    occupied.resize(trainMatch.size(), 0);
    const size_t m = n > 0 ? n : 1;
    if (out) out->projected.assign(m, 0), out->u.assign(m, 0.f), out->v.assign(m, 0.f), out->level.assign(m, 0);
    const int rc = vsg_frame_search_keyframe_points(
        CurrentFrame.handle(), mp.handle(), n, slots.data(), skip, &pose, th, ORBdist, mvScaleFactors.data(),
        (int)mvScaleFactors.size(), mbCheckOrientation, kfAngle.empty() ? nullptr : kfAngle.data(), occupied.data(),
        trainMatch.data(), out ? out->projected.data() : nullptr, out ? out->u.data() : nullptr,
        out ? out->v.data() : nullptr, out ? out->level.data() : nullptr);
    check(rc, "vsg_frame_search_keyframe_points");
    trainMatch.resize(CurrentFrame.N()), occupied.resize(CurrentFrame.N());
    if (out) out->projected.resize(n), out->u.resize(n), out->v.resize(n), out->level.resize(n);
    return rc;
  }

  // SearchBySim3(pKF1, pKF2, vpMatches12, S12, th)  (ORBmatcher.cc:1448-1665): idx1 / idx2 = feature index of every
  // projected point in its own KeyFrame; matches12[i1] = i2 where both directions agree
  int SearchBySim3(ResidentFrame &pKF1, ResidentFrame &pKF2, const std::vector<int32_t> &idx1,
                   const ProjectedPoints &into2, const std::vector<int32_t> &idx2, const ProjectedPoints &into1,
                   std::vector<int32_t> &matches12) const {
    matches12.assign(pKF1.N(), -1);
    int rc = vsg_frame_search_by_sim3(pKF1.handle(), pKF2.handle(), into2.n(), idx1.data(), into2.desc.data(),
                                      into2.u.data(), into2.v.data(), into2.radius.data(), into2.level.data(), into1.n(),
                                      idx2.data(), into1.desc.data(), into1.u.data(), into1.v.data(),
                                      into1.radius.data(), into1.level.data(), matches12.data());
    check(rc, "vsg_frame_search_by_sim3");
    return rc;
  }

  // Fuse(pKF, vpMapPoints, th, bRight)  (ORBmatcher.cc:1148-1329): the search; bestIdx / bestDist per point.  The
  // caller then walks the points in order and does Replace / AddObservation on its MapPoint graph for those with
  // bestDist <= TH_LOW (:1308-1327) -- or hands flattened ids to vsg_fuse_decide.
  int Fuse(ResidentFrame &pKF, const ProjectedPoints &pts, bool bRight, const std::vector<float> &mvInvLevelSigma2,
           std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist) const {
    bestIdx.assign(pts.n(), -1);
    bestDist.assign(pts.n(), 256);
    int rc = vsg_frame_fuse(pKF.handle(), pts.n(), pts.desc.data(), pts.u.data(), pts.v.data(), pts.ur.data(),
                            pts.radius.data(), pts.level.data(), bRight, mvInvLevelSigma2.data(),
                            (int)mvInvLevelSigma2.size(), bestIdx.data(), bestDist.data());
    check(rc, "vsg_frame_fuse");
    return rc;
  }
  // Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)  (ORBmatcher.cc:1331-1446)
  int Fuse(ResidentFrame &pKF, const ProjectedPoints &pts, std::vector<int32_t> &bestIdx,
           std::vector<int32_t> &bestDist) const {
    bestIdx.assign(pts.n(), -1);
    bestDist.assign(pts.n(), 0x7FFFFFFF);
    int rc = vsg_frame_fuse_sim3(pKF.handle(), pts.n(), pts.desc.data(), pts.u.data(), pts.v.data(), pts.radius.data(),
                                 pts.level.data(), bestIdx.data(), bestDist.data());
    check(rc, "vsg_frame_fuse_sim3");
    return rc;
  }

  // The three routines below project the points of a ResidentMapPoints store into ONE KeyFrame on the device
  // (vsg_frame_fuse_points, vsg_frame_fuse_points_sim3, vsg_frame_search_sim3_points): slots[i] = the slot of the i-th
  // point of the routine's list, skip[i] != 0 = the routine `continue`s before GetWorldPos() (nullptr: none).  pose = Tcw /
  // Ow with pKF's intrinsics: pKF->GetPose() / GetCameraCenter(), or the decomposition of Scw the Sim3 routines start with
  // (ORBmatcher.cc:433-434, :1340-1341).  out (optional): per point projected, u, v, ur, level.
  struct IntoKeyFrameProjection {
    std::vector<uint8_t> projected;
    std::vector<float> u, v, ur;
    std::vector<int32_t> level;
    void assign(size_t m) { projected.assign(m, 0), u.assign(m, 0.f), v.assign(m, 0.f), ur.assign(m, 0.f), level.assign(m, 0); }
    void resize(size_t n) { projected.resize(n), u.resize(n), v.resize(n), ur.resize(n), level.resize(n); }
  };
  // int Fuse(KeyFrame *pKF, const vector<MapPoint *> &vpMapPoints, const float th = 3.0, const bool bRight = false)
  // (ORBmatcher.h:84, ORBmatcher.cc:1148-1335; LocalMapping.cc:770, :800) with bRight == false: the search.  skip[i] =
  // !pMP || isBad() || IsInKeyFrame(pKF).  bestIdx / bestDist per point (-1 / 256 when nothing qualifies); the caller then
  // walks them as for the Fuse above.  Returns the count with bestDist <= TH_LOW.
  int Fuse(ResidentFrame &pKF, const ResidentMapPoints &mp, const std::vector<int32_t> &slots, const uint8_t *skip,
           const FramePose &pose, float th, const std::vector<float> &mvScaleFactors,
           const std::vector<float> &mvInvLevelSigma2, std::vector<int32_t> &bestIdx, std::vector<int32_t> &bestDist,
           IntoKeyFrameProjection *out = nullptr) const {
    const int n = (int)slots.size();
    if (mvInvLevelSigma2.size() != mvScaleFactors.size()) check(VSG_ERR_INVALID, "vsg_frame_fuse_points");
    const size_t m = n > 0 ? n : 1;
    bestIdx.assign(m, -1), bestDist.assign(m, 256);
    if (out) out->assign(m);
    const int rc = vsg_frame_fuse_points(
        pKF.handle(), mp.handle(), n, slots.data(), skip, &pose, th, mvScaleFactors.data(), mvInvLevelSigma2.data(),
        (int)mvScaleFactors.size(), bestIdx.data(), bestDist.data(), out ? out->projected.data() : nullptr,
        out ? out->u.data() : nullptr, out ? out->v.data() : nullptr, out ? out->ur.data() : nullptr,
        out ? out->level.data() : nullptr);
    check(rc, "vsg_frame_fuse_points");
    bestIdx.resize(n), bestDist.resize(n);
    if (out) out->resize(n);
    return rc;
  }
  // int Fuse(KeyFrame *pKF, Sophus::Sim3f &Scw, const vector<MapPoint *> &vpPoints, float th, vector<MapPoint *>
  // &vpReplacePoint) (ORBmatcher.h:87, ORBmatcher.cc:1337-1446; LoopClosing.cc:2012, :2054): the search.  skip[i] = isBad() ||
  // spAlreadyFound.count(pMP) (:1356; the set is pKF->GetMapPoints(), :1344).  bestDist is INT_MAX when nothing
  // qualifies.
  int Fuse(ResidentFrame &pKF, const ResidentMapPoints &mp, const std::vector<int32_t> &slots, const uint8_t *skip,
           const FramePose &pose, float th, const std::vector<float> &mvScaleFactors, std::vector<int32_t> &bestIdx,
           std::vector<int32_t> &bestDist, IntoKeyFrameProjection *out = nullptr) const {
    const int n = (int)slots.size();
    const size_t m = n > 0 ? n : 1;
    bestIdx.assign(m, -1), bestDist.assign(m, 0x7FFFFFFF);
    if (out) out->assign(m);
    const int rc = vsg_frame_fuse_points_sim3(
        pKF.handle(), mp.handle(), n, slots.data(), skip, &pose, th, mvScaleFactors.data(), (int)mvScaleFactors.size(),
        bestIdx.data(), bestDist.data(), out ? out->projected.data() : nullptr, out ? out->u.data() : nullptr,
        out ? out->v.data() : nullptr, out ? out->level.data() : nullptr);
    check(rc, "vsg_frame_fuse_points_sim3");
    bestIdx.resize(n), bestDist.resize(n);
    if (out) out->resize(n);
    return rc;
  }
  // int SearchByProjection(KeyFrame *pKF, Sophus::Sim3f &Scw, const vector<MapPoint *> &vpPoints, vector<MapPoint *>
  // &vpMatched, int th, float ratioHamming = 1.0) (ORBmatcher.h:58, ORBmatcher.cc:430-528; LoopClosing.cc:735, :757, :944).
  // skip[i] = isBad() || spAlreadyFound.count(pMP).  matched[i] != -1 = vpMatched[i] is set; new entries = index into slots.
  int SearchByProjection(ResidentFrame &pKF, const ResidentMapPoints &mp, const std::vector<int32_t> &slots,
                         const uint8_t *skip, const FramePose &pose, int th, float ratioHamming,
                         const std::vector<float> &mvScaleFactors, std::vector<int32_t> &matched,
                         IntoKeyFrameProjection *out = nullptr) const {
    const int n = (int)slots.size();
    matched.resize(pKF.N() > 0 ? pKF.N() : 1, -1);
    if (out) out->assign(n > 0 ? n : 1);
    const int rc = vsg_frame_search_sim3_points(
        pKF.handle(), mp.handle(), n, slots.data(), skip, &pose, (float)th, ratioHamming, mvScaleFactors.data(),
        (int)mvScaleFactors.size(), matched.data(), out ? out->projected.data() : nullptr, out ? out->u.data() : nullptr,
        out ? out->v.data() : nullptr, out ? out->level.data() : nullptr);
    check(rc, "vsg_frame_search_sim3_points");
    matched.resize(pKF.N());
    if (out) out->resize(n);
    return rc;
  }

  // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)  (ORBmatcher.cc:643-756)
  int SearchForInitialization(ResidentFrame &F1, ResidentFrame &F2, const std::vector<float> &prevX,
                              const std::vector<float> &prevY, int windowSize, std::vector<int32_t> &vnMatches12) const {
    vnMatches12.assign(F1.N(), -1);
    int rc = vsg_frame_search_for_initialization(F1.handle(), F2.handle(), prevX.data(), prevY.data(), windowSize,
                                                 mfNNratio, mbCheckOrientation, vnMatches12.data());
    check(rc, "vsg_frame_search_for_initialization");
    return rc;
  }

  // SearchByBoW(KeyFrame*, Frame&) / (KeyFrame*, KeyFrame*)  (ORBmatcher.cc:226-428, 758-900) on resident descriptors
  int SearchByBoW(ResidentFrame &pKF, const uint8_t *kfValid, const FeatureVectorCSR &kfFeatVec, ResidentFrame &F,
                  const FeatureVectorCSR &fFeatVec, std::vector<int32_t> &matchF) const {
    matchF.assign(F.N(), -1);
    int rc = vsg_frame_search_by_bow_kf_f(pKF.handle(), kfValid, kfFeatVec.node.data(), kfFeatVec.off.data(),
                                          kfFeatVec.idx.data(), kfFeatVec.nodes(), F.handle(), fFeatVec.node.data(),
                                          fFeatVec.off.data(), fFeatVec.idx.data(), fFeatVec.nodes(), mfNNratio,
                                          mbCheckOrientation, matchF.data());
    check(rc, "vsg_frame_search_by_bow_kf_f");
    return rc;
  }
  // The same two with the FeatureVectors both frames keep resident since their ComputeBoW (ORBVocabulary::ComputeBoW), of
  // any number of features: the join runs on the device, only the "has a map point" flags go up.  An empty frame gives 0
  // matches; a non-empty frame whose features changed after its last ComputeBoW is refused (check() throws)
  int SearchByBoW(ResidentFrame &pKF, const uint8_t *kfValid, ResidentFrame &F, std::vector<int32_t> &matchF) const {
    matchF.assign(F.N(), -1);
    int rc = vsg_frame_search_by_bow_kf_f(pKF.handle(), kfValid, nullptr, nullptr, nullptr, 0, F.handle(), nullptr, nullptr,
                                          nullptr, 0, mfNNratio, mbCheckOrientation, matchF.data());
    check(rc, "vsg_frame_search_by_bow_kf_f");
    return rc;
  }
  int SearchByBoW(ResidentFrame &pKF1, const uint8_t *valid1, ResidentFrame &pKF2, const uint8_t *valid2,
                  std::vector<int32_t> &vMatches12) const {
    vMatches12.assign(pKF1.N(), -1);
    int rc = vsg_frame_search_by_bow_kf_kf(pKF1.handle(), valid1, nullptr, nullptr, nullptr, 0, pKF2.handle(), valid2, nullptr,
                                           nullptr, nullptr, 0, mfNNratio, mbCheckOrientation, vMatches12.data());
    check(rc, "vsg_frame_search_by_bow_kf_kf");
    return rc;
  }
  int SearchByBoW(ResidentFrame &pKF1, const uint8_t *valid1, const FeatureVectorCSR &fv1, ResidentFrame &pKF2,
                  const uint8_t *valid2, const FeatureVectorCSR &fv2, std::vector<int32_t> &vMatches12) const {
    vMatches12.assign(pKF1.N(), -1);
    int rc = vsg_frame_search_by_bow_kf_kf(pKF1.handle(), valid1, fv1.node.data(), fv1.off.data(), fv1.idx.data(),
                                           fv1.nodes(), pKF2.handle(), valid2, fv2.node.data(), fv2.off.data(),
                                           fv2.idx.data(), fv2.nodes(), mfNNratio, mbCheckOrientation, vMatches12.data());
    check(rc, "vsg_frame_search_by_bow_kf_kf");
    return rc;
  }

  // SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vMatchedPairs, bOnlyStereo, bCoarse)  (ORBmatcher.cc:902-1146)
  // with both KeyFrames resident (LocalMapping::CreateNewMapPoints, LocalMapping.cc:389: the current keyframe against
  // each covisible neighbour).  eligible / pairOk as in ORBmatcher::SearchForTriangulation above: the predicate of
  // :1031-1071 is evaluated here for every pair of every shared node and goes up as a bitmask; nullptr_t = all pass.
  template <class Pred>
  int SearchForTriangulation(ResidentFrame &pKF1, const uint8_t *eligible1, const FeatureVectorCSR &fv1,
                             ResidentFrame &pKF2, const uint8_t *eligible2, const FeatureVectorCSR &fv2, Pred pairOk,
                             std::vector<std::pair<size_t, size_t>> &vMatchedPairs) const {
    std::vector<uint32_t> bits(1, 0u);
    std::vector<int32_t> off(1, 0);
    size_t a = 0, b = 0;
    while (a < fv1.node.size() && b < fv2.node.size()) {  // the reference's merge-join, shared nodes in id order
      if (fv1.node[a] == fv2.node[b]) {
        const int n2 = fv2.off[b + 1] - fv2.off[b];
        for (int i1 = fv1.off[a]; i1 < fv1.off[a + 1]; i1++)
          for (int i2 = fv2.off[b]; i2 < fv2.off[b + 1]; i2++) {
            const long long bit = (long long)off.back() + (long long)(i1 - fv1.off[a]) * n2 + (i2 - fv2.off[b]);
            if ((size_t)(bit >> 5) >= bits.size()) bits.resize((size_t)(bit >> 5) + 64, 0u);
            if (eligible1[fv1.idx[i1]] && eligible2[fv2.idx[i2]] && pairOk(fv1.idx[i1], fv2.idx[i2]))
              bits[bit >> 5] |= 1u << (bit & 31);
          }
        off.push_back(off.back() + (fv1.off[a + 1] - fv1.off[a]) * n2);
        a++, b++;
      } else if (fv1.node[a] < fv2.node[b]) {
        a++;
      } else {
        b++;
      }
    }
    bits.resize((size_t)(off.back() >> 5) + 2, 0u);
    std::vector<int32_t> m12(pKF1.N() > 0 ? pKF1.N() : 1, -1);
    int rc = vsg_frame_search_for_triangulation(pKF1.handle(), eligible1, fv1.node.data(), fv1.off.data(), fv1.idx.data(),
                                                fv1.nodes(), pKF2.handle(), eligible2, fv2.node.data(), fv2.off.data(),
                                                fv2.idx.data(), fv2.nodes(), bits.data(), off.data(), mbCheckOrientation,
                                                m12.data());
    check(rc, "vsg_frame_search_for_triangulation");
    vMatchedPairs.clear();
    for (int i = 0; i < pKF1.N(); i++)
      if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1131-1141: pairs in idx1 order
    return rc;
  }

  // int SearchForTriangulation(KeyFrame *pKF1, KeyFrame *pKF2, vector<pair<size_t, size_t>> &vMatchedPairs, const bool
  // bOnlyStereo, const bool bCoarse) (ORBmatcher.h:72, ORBmatcher.cc:902-1146; LocalMapping.cc:389-460) with the predicate of
  // :976-1073 on the device too (vsg_frame_search_for_triangulation_epipolar): no loop over the pairs here and no bitmask.
  // noMpX[i] = !pKFX->GetMapPoint(i).  F12 (row-major) and ep are the caller's, once per pair of keyframes, with the
  // reference's own expressions: F12 = K1.transpose().inverse() * Sophus::SO3f::hat(t12) * R12 * K2.inverse()
  // (Pinhole.cpp:121-124), ep = pKF2->mpCamera->project(T2w * Cw) (:913-915).  mvScaleFactors2 / mvLevelSigma2_2 are pKF2's.
  // fv1 / fv2 == nullptr: the FeatureVectors both frames keep resident since their ComputeBoW are joined on the device.
  int SearchForTriangulation(ResidentFrame &pKF1, const uint8_t *noMp1, ResidentFrame &pKF2, const uint8_t *noMp2,
                             const float F12[9], const float ep[2], const std::vector<float> &mvScaleFactors2,
                             const std::vector<float> &mvLevelSigma2_2, bool bOnlyStereo, bool bCoarse,
                             std::vector<std::pair<size_t, size_t>> &vMatchedPairs, const FeatureVectorCSR *fv1 = nullptr,
                             const FeatureVectorCSR *fv2 = nullptr) const {
    if (mvLevelSigma2_2.size() != mvScaleFactors2.size() || !fv1 != !fv2)
      check(VSG_ERR_INVALID, "vsg_frame_search_for_triangulation_epipolar");
    vMatchedPairs.clear();
    if (fv1 && (fv1->nodes() == 0 || fv2->nodes() == 0)) return 0;  // no shared node (their data() may be NULL)
    std::vector<int32_t> m12(pKF1.N() > 0 ? pKF1.N() : 1, -1);
    const int rc = vsg_frame_search_for_triangulation_epipolar(
        pKF1.handle(), noMp1, fv1 ? fv1->node.data() : nullptr, fv1 ? fv1->off.data() : nullptr,
        fv1 ? fv1->idx.data() : nullptr, fv1 ? fv1->nodes() : 0, pKF2.handle(), noMp2, fv2 ? fv2->node.data() : nullptr,
        fv2 ? fv2->off.data() : nullptr, fv2 ? fv2->idx.data() : nullptr, fv2 ? fv2->nodes() : 0, F12, ep,
        mvScaleFactors2.data(), mvLevelSigma2_2.data(), (int)mvScaleFactors2.size(), bOnlyStereo, bCoarse,
        mbCheckOrientation, m12.data());
    check(rc, "vsg_frame_search_for_triangulation_epipolar");
    for (int i = 0; i < pKF1.N(); i++)
      if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :1131-1141: pairs in idx1 order
    return rc;
  }

  // The loop over one neighbour's matches of LocalMapping::CreateNewMapPoints (LocalMapping.cc:475-708) for a match list the
  // caller holds (matches12[idx1] = idx2 or -1), mpCurrentKeyFrame = pKF1 (vsg_frame_triangulate_matches).  mp == nullptr:
  // geometry only; otherwise the k-th accepted pair in ascending idx1 is written into freeSlots[k] on the device.
  void TriangulateMatches(ResidentFrame &pKF1, ResidentFrame &pKF2, const std::vector<int32_t> &matches12,
                          const vsg_triangulation_params &params, const std::vector<float> &mvScaleFactors1,
                          const std::vector<float> &mvLevelSigma2_1, const std::vector<float> &mvScaleFactors2,
                          const std::vector<float> &mvLevelSigma2_2, ResidentMapPoints *mp,
                          const std::vector<int32_t> &freeSlots, NewMapPointsResult &out) const {
    const size_t nl = mvScaleFactors1.size();
    if (mvLevelSigma2_1.size() != nl || mvScaleFactors2.size() != nl || mvLevelSigma2_2.size() != nl ||
        matches12.size() < (size_t)pKF1.N())
      check(VSG_ERR_INVALID, "vsg_frame_triangulate_matches");
    out.resize(pKF1.N());
    static const int32_t none = -1;
    check(vsg_frame_triangulate_matches(pKF1.handle(), pKF2.handle(), matches12.empty() ? &none : matches12.data(), &params,
                                        mvScaleFactors1.data(), mvLevelSigma2_1.data(), mvScaleFactors2.data(),
                                        mvLevelSigma2_2.data(), (int)nl, mp ? mp->handle() : nullptr, freeSlots.data(),
                                        (int)freeSlots.size(), out.reason.data(), out.source.data(), out.x3D.data(),
                                        out.newSlot.data(), &out.nCreated),
          "vsg_frame_triangulate_matches");
    for (int i = 0; i < pKF1.N(); i++)
      if (matches12[i] >= 0) out.vMatchedIndices.emplace_back((size_t)i, (size_t)matches12[i]), out.nMatches++;
  }

  // One neighbour of LocalMapping::CreateNewMapPoints (LocalMapping.cc:456-708) in one enqueue and one wait
  // (vsg_frame_create_new_map_points): the search of SearchForTriangulation above (F12, ep, noMpX, fv1 / fv2 as there), the
  // rotation filter, the triangulation and the store writes.  Returns nmatches after the filter.
  int CreateNewMapPoints(ResidentFrame &pKF1, const uint8_t *noMp1, ResidentFrame &pKF2, const uint8_t *noMp2,
                         const float F12[9], const float ep[2], bool bOnlyStereo, bool bCoarse,
                         const vsg_triangulation_params &params, const std::vector<float> &mvScaleFactors1,
                         const std::vector<float> &mvLevelSigma2_1, const std::vector<float> &mvScaleFactors2,
                         const std::vector<float> &mvLevelSigma2_2, ResidentMapPoints *mp,
                         const std::vector<int32_t> &freeSlots, NewMapPointsResult &out, const FeatureVectorCSR *fv1 = nullptr,
                         const FeatureVectorCSR *fv2 = nullptr) const {
    const size_t nl = mvScaleFactors1.size();
    if (mvLevelSigma2_1.size() != nl || mvScaleFactors2.size() != nl || mvLevelSigma2_2.size() != nl || !fv1 != !fv2)
      check(VSG_ERR_INVALID, "vsg_frame_create_new_map_points");
    out.resize(pKF1.N());
    std::vector<int32_t> m12(pKF1.N() > 0 ? pKF1.N() : 1, -1);
    if (fv1 && (fv1->nodes() == 0 || fv2->nodes() == 0)) {  // no shared node (their data() may be NULL): no match, no point
      std::fill(out.reason.begin(), out.reason.end(), (uint8_t)VSG_TRI_NO_MATCH);
      return 0;
    }
    const int rc = vsg_frame_create_new_map_points(
        pKF1.handle(), noMp1, fv1 ? fv1->node.data() : nullptr, fv1 ? fv1->off.data() : nullptr,
        fv1 ? fv1->idx.data() : nullptr, fv1 ? fv1->nodes() : 0, pKF2.handle(), noMp2, fv2 ? fv2->node.data() : nullptr,
        fv2 ? fv2->off.data() : nullptr, fv2 ? fv2->idx.data() : nullptr, fv2 ? fv2->nodes() : 0, F12, ep, bOnlyStereo, bCoarse,
        mbCheckOrientation, &params, mvScaleFactors1.data(), mvLevelSigma2_1.data(), mvScaleFactors2.data(),
        mvLevelSigma2_2.data(), (int)nl, mp ? mp->handle() : nullptr, freeSlots.data(), (int)freeSlots.size(), m12.data(),
        out.reason.data(), out.source.data(), out.x3D.data(), out.newSlot.data(), &out.nCreated);
    check(rc, "vsg_frame_create_new_map_points");
    for (int i = 0; i < pKF1.N(); i++)
      if (m12[i] >= 0) out.vMatchedIndices.emplace_back((size_t)i, (size_t)m12[i]);
    return out.nMatches = rc;
  }

 protected:
  float mfNNratio;
  bool mbCheckOrientation;
};

// Asynchronous operator() batches over the handle's pipeline slots (vsg_orb_submit_batch / vsg_orb_wait): H2D of
// batch k+1 beside the kernels of batch k beside the export of batch k-1.  Buffers from vsg_host_alloc (hipHostMalloc) are
// read and written by the device in place; any other memory is staged (include/vsg_orb.h, "Pinned caller memory").
inline int SubmitBatch(const ORBextractor &ex, const uint8_t *gray, int nframes, size_t frameStride, int rows, int cols,
                       int stride, const std::vector<int> &vLappingArea, vsg_keypoint *kps, uint8_t *desc,
                       int capacity) {
  int t = vsg_orb_submit_batch(ex.handle(), gray, nframes, frameStride, rows, cols, stride, vLappingArea.at(0),
                               vLappingArea.at(1), kps, desc, capacity);
  check(t, "vsg_orb_submit_batch");
  return t;
}
inline void WaitBatch(const ORBextractor &ex, int ticket, std::vector<int> &n, std::vector<int> &monoIndex) {
  check(vsg_orb_wait(ex.handle(), ticket, n.data(), monoIndex.data()), "vsg_orb_wait");
}

// Sim3Solver (Sim3Solver.h, Sim3Solver.cc) on resident map points, with the reference's shape so that the loop of
// LoopClosing::DetectCommonRegionsFromBoW (LoopClosing.cc:678-690) stays as it is:
//     vsg::ResidentSim3Solver solver(mp1, mp2, slots1, slots2, maxErr1, maxErr2, mvnIndices1, N1, pose1, pose2, mbFixScale);
//     solver.SetRansacParameters(0.99, nBoWInliers, 300);
//     while (!bConverge && !bNoMore) mTcm = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
// The maintainer's constructor keeps the reference's filter (:68-112: both points exist, neither isBad, both have an index in
// their keyframe) and hands over what survives it: correspondence i = slot slots1[i] of mp1 (pMP1) against slot slots2[i] of
// mp2 (pMP2; the same store or another map's), maxErr1 / maxErr2[i] = Sim3MaxError(mvLevelSigma2[kp.octave]) of pKF1 / pKFm,
// mvnIndices1[i] = i1 and mN1 = vpMatched12.size().  pose1 / pose2 = pKF1's / pKF2's pose and camera (X3Dc2 goes through
// pKF2's pose also for a point matched through pKFm, :107).  The FIRST iterate (or find) computes every hypothesis in one
// device call (vsg_mappoints_sim3_ransac); later calls replay the reference's nIterations-at-a-time view of that result.
// Matrices are row-major arrays (the maintainer maps them: Eigen::Map<Eigen::Matrix<float, 4, 4, Eigen::RowMajor>>).
// The samples come from vsg_sim3_draw_samples with DUtils::Random::RandomInt's formula over rand(), or from randomInt.
inline float Sim3MaxError(float sigmaSquare) { return (float)(size_t)(9.210 * sigmaSquare); }  // :96-97, Sim3Solver.h:72-73
inline float Sim3MaxError(const std::vector<float> &mvLevelSigma2, int octave) { return Sim3MaxError(mvLevelSigma2[(size_t)octave]); }

class ResidentSim3Solver {
 public:
  typedef std::vector<float> Matrix;  // row-major
  ResidentSim3Solver(const ResidentMapPoints &mp1, const ResidentMapPoints &mp2, const std::vector<int32_t> &slots1,
                     const std::vector<int32_t> &slots2, const std::vector<float> &maxErr1, const std::vector<float> &maxErr2,
                     const std::vector<size_t> &mvnIndices1, int mN1, const FramePose &pose1, const FramePose &pose2,
                     bool bFixScale = false, int (*randomInt)(int, int, void *) = nullptr, void *randomCtx = nullptr)
      : mp1_(mp1.handle()), mp2_(mp2.handle()), slots1_(slots1), slots2_(slots2), maxErr1_(maxErr1), maxErr2_(maxErr2),
        mvnIndices1_(mvnIndices1), mN1_(mN1), pose1_(pose1), pose2_(pose2), mbFixScale_(bFixScale), randomInt_(randomInt),
        randomCtx_(randomCtx) {
    N_ = (int)slots1_.size();
    if (slots2_.size() != slots1_.size() || maxErr1_.size() != slots1_.size() || maxErr2_.size() != slots1_.size() ||
        mvnIndices1_.size() != slots1_.size())
      check(VSG_ERR_INVALID, "vsg::ResidentSim3Solver");
    for (size_t i1 : mvnIndices1_)
      if (i1 >= (size_t)(mN1_ > 0 ? mN1_ : 0)) check(VSG_ERR_INVALID, "vsg::ResidentSim3Solver");
    fill_identity();
    SetRansacParameters();
  }
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacMinInliers_ = minInliers;
    mRansacMaxIts_ = vsg_sim3_ransac_iterations(probability, minInliers, maxIterations, N_);
    check(mRansacMaxIts_, "vsg_sim3_ransac_iterations");
    mnIterations_ = 0, solved_ = false;
  }
  // Sim3Solver::iterate (:215-291).  While the solver has not converged the reference returns a stack variable that it may
  // have left unset (bestSim3, :235, :290); mBestT12 is returned there.
  Matrix iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, bool &bConverge) {
    bNoMore = false, bConverge = false;
    vbInliers.assign((size_t)(mN1_ > 0 ? mN1_ : 0), false);
    nInliers = 0;
    if (N_ < mRansacMinInliers_) {  // :222-226
      bNoMore = true;
      return identity4();
    }
    solve();
    // the reference's loop: this call walks hypotheses [mnIterations, mnIterations + nIterations) of at most mRansacMaxIts
    int walked = mRansacMaxIts_ - mnIterations_ < nIterations ? mRansacMaxIts_ - mnIterations_ : nIterations;
    if (walked < 0) walked = 0;
    if (res_.converged && res_.iterations > mnIterations_ && res_.iterations <= mnIterations_ + walked) {
      mnIterations_ = res_.iterations;
      nInliers = res_.n_inliers;
      for (int i = 0; i < N_; ++i)
        if (inlier_[(size_t)i]) vbInliers[mvnIndices1_[(size_t)i]] = true;
      bConverge = true;
      return Matrix(res_.T12, res_.T12 + 16);
    }
    mnIterations_ += walked;
    if (mnIterations_ >= mRansacMaxIts_) bNoMore = true;
    return Matrix(res_.T12, res_.T12 + 16);
  }
  // Sim3Solver::iterate without bConverge (:146-213) returns the identity unless it converged
  Matrix iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers) {
    bool bConverge = false;
    Matrix T = iterate(nIterations, bNoMore, vbInliers, nInliers, bConverge);
    return bConverge ? T : identity4();
  }
  Matrix find(std::vector<bool> &vbInliers12, int &nInliers) {  // :293-297
    bool bFlag;
    return iterate(mRansacMaxIts_, bFlag, vbInliers12, nInliers);
  }
  // mBest* as far as the reference's loop has walked: the device call holds the members of the END of the walk, which is
  // where the reference's caller reads them (after bConverge or bNoMore)
  Matrix GetEstimatedTransformation() const { return Matrix(res_.T12, res_.T12 + 16); }
  Matrix GetEstimatedRotation() const { return Matrix(res_.R12, res_.R12 + 9); }
  std::vector<float> GetEstimatedTranslation() const { return std::vector<float>(res_.t12, res_.t12 + 3); }
  float GetEstimatedScale() const { return res_.s12; }
  int iterations() const { return mnIterations_; }          // mnIterations
  int maxIterations() const { return mRansacMaxIts_; }      // mRansacMaxIts
  const vsg_sim3_result &result() const { return res_; }
  const std::vector<int32_t> &samples() const { return samples_; }

 private:
  static Matrix identity4() {
    Matrix I(16, 0.0f);
    I[0] = I[5] = I[10] = I[15] = 1.0f;
    return I;
  }
  void fill_identity() {
    memset(&res_, 0, sizeof res_);
    res_.R12[0] = res_.R12[4] = res_.R12[8] = res_.s12 = res_.T12[0] = res_.T12[5] = res_.T12[10] = res_.T12[15] = 1.0f;
  }
  void solve() {
    if (solved_) return;
    samples_.assign(3 * (size_t)mRansacMaxIts_, 0);
    check(vsg_sim3_draw_samples(N_, mRansacMaxIts_, randomInt_, randomCtx_, samples_.data()), "vsg_sim3_draw_samples");
    inlier_.assign((size_t)(N_ > 0 ? N_ : 1), 0);
    check(vsg_mappoints_sim3_ransac(mp1_, mp2_, N_, slots1_.data(), slots2_.data(), maxErr1_.data(), maxErr2_.data(), &pose1_,
                                    &pose2_, mbFixScale_ ? 1 : 0, mRansacMinInliers_, mRansacMaxIts_, samples_.data(),
                                    inlier_.data(), &res_, nullptr, nullptr),
          "vsg_mappoints_sim3_ransac");
    solved_ = true;
  }
  vsg_mappoints *mp1_, *mp2_;
  std::vector<int32_t> slots1_, slots2_;
  std::vector<float> maxErr1_, maxErr2_;
  std::vector<size_t> mvnIndices1_;
  int mN1_, N_ = 0;
  FramePose pose1_, pose2_;
  bool mbFixScale_;
  int (*randomInt_)(int, int, void *);
  void *randomCtx_;
  int mRansacMinInliers_ = 6, mRansacMaxIts_ = 300, mnIterations_ = 0;
  bool solved_ = false;
  std::vector<int32_t> samples_;
  std::vector<uint8_t> inlier_;
  vsg_sim3_result res_;
};

// MLPnPsolver (MLPnPsolver.h, MLPnPsolver.cpp) on a resident frame and resident map points, with the reference's shape, so
// that the relocalisation loop of Tracking.cc:3735-3762 stays as it is:
//     vsg::MLPnPsolver *pSolver = new vsg::MLPnPsolver(F, mp, slots, K4, mCurrentFrame.mvLevelSigma2);
//     pSolver->SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991);
//     bool bTcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers, Tcw);   // Tcw: row-major 4 x 4
// The maintainer hands over slots[i] = the slot of vpMapPointMatches[i] in mp, -1 for a NULL or isBad() point, one entry per
// feature of F (the constructor's filter, :66-98); K4 = {fx, fy, cx, cy} of the Pinhole camera.  Every iterate is ONE device
// call (vsg_frame_mlpnp_ransac) that computes every hypothesis drawn so far side by side and selects as the reference's loop
// does from mnIterations on (Refine()'s solve over the best set, whose result the reference never installs, is left out); the library keeps no state, the solver keeps mnIterations and the minimal sets.  The sets come
// from vsg_mlpnp_draw_sets in the reference's drawing order -- DUtils::Random::RandomInt's formula over rand(), or randomInt
// -- and are drawn as far as a call can walk: max(mRansacMaxIts, mnIterations + nIterations) hypotheses, 1024 at the most.
class MLPnPsolver {
 public:
  typedef std::vector<float> Matrix;  // row-major 4 x 4
  MLPnPsolver(const ResidentFrame &F, const ResidentMapPoints &mp, const std::vector<int32_t> &slots, const float K4[4],
              const std::vector<float> &mvLevelSigma2, int (*randomInt)(int, int, void *) = nullptr, void *randomCtx = nullptr)
      : f_(F.handle()), mp_(mp.handle()), slots_(slots), sigma2_(mvLevelSigma2), randomInt_(randomInt), randomCtx_(randomCtx) {
    for (int k = 0; k < 4; ++k) K_[k] = K4[k];
    if ((int)slots_.size() != F.N()) check(VSG_ERR_INVALID, "vsg::MLPnPsolver");
    for (int32_t s : slots_) N_ += s >= 0 ? 1 : 0;
    memset(&res_, 0, sizeof res_);
    SetRansacParameters();
  }
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6,
                           float epsilon = 0.4f, float th2 = 5.991f) {
    if (minSet != 6) check(VSG_ERR_UNSUPPORTED, "vsg::MLPnPsolver::SetRansacParameters");  // the minimal set of the device call
    check(vsg_mlpnp_ransac_parameters(probability, minInliers, maxIterations, minSet, epsilon, N_, &mRansacMinInliers_, &mRansacMaxIts_),
          "vsg_mlpnp_ransac_parameters");
    th2_ = th2;
  }
  // MLPnPsolver::iterate (:104-229)
  bool iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers, Matrix &Tout) {
    Tout.assign(16, 0.0f);
    Tout[0] = Tout[5] = Tout[10] = Tout[15] = 1.0f;
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (N_ < mRansacMinInliers_) {  // :111-115
      bNoMore = true;
      return false;
    }
    if (nIterations < 0) nIterations = 0;
    const int walk = mnIterations_ + nIterations, end = mRansacMaxIts_ > walk ? mRansacMaxIts_ : walk;
    if (end > 1024) check(VSG_ERR_UNSUPPORTED, "vsg::MLPnPsolver::iterate");  // more hypotheses than one call takes
    const int have = (int)(sets_.size() / 6);
    if (end > have) {  // the draw goes on where it stopped: the sequence of RandomInt calls is the reference's
      sets_.resize(6 * (size_t)end);
      check(vsg_mlpnp_draw_sets(N_, end - have, randomInt_, randomCtx_, sets_.data() + 6 * (size_t)have), "vsg_mlpnp_draw_sets");
    }
    inlier_.assign(slots_.size() ? slots_.size() : 1, 0);
    check(vsg_frame_mlpnp_ransac(f_, mp_, slots_.data(), K_[0], K_[1], K_[2], K_[3], sigma2_.data(), (int)sigma2_.size(), th2_,
                                 mRansacMinInliers_, mRansacMaxIts_, mnIterations_, nIterations, (int)(sets_.size() / 6),
                                 sets_.data(), inlier_.data(), &res_, nullptr, nullptr),
          "vsg_frame_mlpnp_ransac");
    mnIterations_ = res_.iterations;
    bNoMore = res_.no_more != 0;
    if (!res_.found) return false;
    nInliers = res_.n_inliers;
    vbInliers.assign(slots_.size(), false);
    for (size_t i = 0; i < slots_.size(); ++i)
      if (inlier_[i]) vbInliers[i] = true;
    Tout.assign(res_.Tcw, res_.Tcw + 16);
    return true;
  }
  int correspondences() const { return N_; }              // N
  int iterations() const { return mnIterations_; }        // mnIterations
  int minInliers() const { return mRansacMinInliers_; }   // mRansacMinInliers
  int maxIterations() const { return mRansacMaxIts_; }    // mRansacMaxIts
  const vsg_mlpnp_result &result() const { return res_; }
  const std::vector<int32_t> &sets() const { return sets_; }

 private:
  vsg_frame *f_;
  vsg_mappoints *mp_;
  std::vector<int32_t> slots_;
  std::vector<float> sigma2_;
  float K_[4], th2_ = 5.991f;
  int (*randomInt_)(int, int, void *);
  void *randomCtx_;
  int N_ = 0, mRansacMinInliers_ = 8, mRansacMaxIts_ = 300, mnIterations_ = 0;
  std::vector<int32_t> sets_;
  std::vector<uint8_t> inlier_;
  vsg_mlpnp_result res_;
};

// Optimizer::OptimizeSim3 (Optimizer.h, Optimizer.cc:3261-3529) on two resident keyframes and resident map points, with
// the reference's shape, so that the call sites of LoopClosing.cc:538 and :747 stay as they are:
//     vsg::ResidentSim3Optimizer opt(kf1, kf2, mp1, mp2, pose1, pose2, mvInvLevelSigma2_1, mvInvLevelSigma2_2);
//     int numOptMatches = opt.OptimizeSim3(slots1, slots2, idx2, level2, nulled, gScm, 10, mbFixScale, mHessian7x7, true);
// The maintainer fills, per feature i of pKF1: slots1[i] = the slot of vpMapPoints1[i] (-1: none or isBad()), slots2[i] =
// the slot of vpMatches1[i] (-1: NULL or isBad()), idx2[i] = get<0>(pMP2->GetIndexInKeyFrame(pKF2)), level2[i] =
// pMP2->mnTrackScaleLevel.  On return nulled[i] != 0 where the reference sets vpMatches1[i] = NULL (:3469, :3516) -- the
// maintainer applies it to the pointers --, g2oS12 is updated unless the routine returned before :3526, and
// mAcumHessian (49 doubles) is zero-filled as :3502 does, and only when that line is reached.
class ResidentSim3Optimizer {
 public:
  ResidentSim3Optimizer(const ResidentFrame &kf1, const ResidentFrame &kf2, const ResidentMapPoints &mp1,
                        const ResidentMapPoints &mp2, const FramePose &pose1, const FramePose &pose2,
                        const std::vector<float> &mvInvLevelSigma2_1, const std::vector<float> &mvInvLevelSigma2_2)
      : kf1_(kf1.handle()), kf2_(kf2.handle()), mp1_(mp1.handle()), mp2_(mp2.handle()), pose1_(pose1), pose2_(pose2),
        sig1_(mvInvLevelSigma2_1), sig2_(mvInvLevelSigma2_2) {
    if (sig1_.size() != sig2_.size()) check(VSG_ERR_INVALID, "vsg::ResidentSim3Optimizer");
  }
  int OptimizeSim3(const std::vector<int32_t> &slots1, const std::vector<int32_t> &slots2, const std::vector<int32_t> &idx2,
                   const std::vector<int32_t> &level2, std::vector<uint8_t> &nulled, vsg_sim3d &g2oS12, float th2,
                   bool bFixScale, double *mAcumHessian, bool bAllPoints = false) {
    const size_t n = slots1.size();
    if (slots2.size() != n || idx2.size() != n || level2.size() != n) check(VSG_ERR_INVALID, "vsg::ResidentSim3Optimizer");
    state_.assign(n ? n : 1, 0), chi2_.assign(2 * (n ? n : 1), 0.0);
    const int nIn = vsg_frame_optimize_sim3(kf1_, kf2_, mp1_, mp2_, slots1.data(), slots2.data(), idx2.data(), level2.data(),
                                            &pose1_, &pose2_, sig1_.data(), sig2_.data(), (int)sig1_.size(), &g2oS12, th2,
                                            bFixScale ? 1 : 0, bAllPoints ? 1 : 0, state_.data(), chi2_.data(), &res_);
    check(nIn, "vsg_frame_optimize_sim3");
    nulled.assign(n, 0);
    for (size_t i = 0; i < n; ++i) nulled[i] = state_[i] == 2 || state_[i] == 3 ? 1 : 0;
    if (res_.updated) {
      g2oS12 = res_.S12;
      if (mAcumHessian)
        for (int k = 0; k < 49; ++k) mAcumHessian[k] = 0.0;  // Eigen::MatrixXd::Zero(7, 7): nothing accumulates into it
    }
    return nIn;
  }
  const vsg_sim3_opt_result &result() const { return res_; }
  const std::vector<uint8_t> &state() const { return state_; }  // per feature, as vsg_frame_optimize_sim3 documents it
  const std::vector<double> &chi2() const { return chi2_; }     // two per feature

 private:
  vsg_frame *kf1_, *kf2_;
  vsg_mappoints *mp1_, *mp2_;
  FramePose pose1_, pose2_;
  std::vector<float> sig1_, sig2_;
  std::vector<uint8_t> state_;
  std::vector<double> chi2_;
  vsg_sim3_opt_result res_ = {};
};

// TwoViewReconstruction (TwoViewReconstruction.h, .cc:31-129) on two resident frames, with the reference's constructor and
// Reconstruct, so that Pinhole::ReconstructWithTwoViews (Pinhole.cpp:91-101) keeps its shape:
//     vsg::ResidentTwoViewReconstruction tvr(K, 1.0f, 200);                          // K = mK row-major
//     bool ok = tvr.Reconstruct(initialFrame, currentFrame, vMatches12, R21, t21, vP3D, vbTriangulated);
// T21 comes back as R21 (row-major) and t21, vP3D as {x, y, z} per keypoint of the first frame.  KEPT as the reference has
// it: vP3D is assigned only when the call succeeds from the fundamental matrix -- ReconstructH never assigns it (:724-730),
// so after a success from the homography it is exactly what the caller passed in -- and nothing is assigned on failure.
// The second form takes the undistorted keypoints themselves (KannalaBrandt8::ReconstructWithTwoViews, which undistorts on
// its own first).  mvSets comes from vsg_two_view_draw_sets with DUtils::Random::RandomInt's formula over rand() -- the caller
// keeps SeedRandOnce(0) -- or from randomInt.
class ResidentTwoViewReconstruction {
 public:
  ResidentTwoViewReconstruction(const float K[9], float sigma = 1.0f, int iterations = 200, int device = 0,
                                int (*randomInt)(int, int, void *) = nullptr, void *randomCtx = nullptr)
      : mMaxIterations_(iterations), device_(device), randomInt_(randomInt), randomCtx_(randomCtx) {
    for (int k = 0; k < 9; ++k) mK_[k] = K[k];
    vsg_two_view_default_params(&params_);
    params_.sigma = sigma;
    memset(&res_, 0, sizeof res_);
  }
  vsg_two_view_params &params() { return params_; }  // rh_threshold, min_parallax, min_triangulated of :116-127
  bool Reconstruct(const ResidentFrame &F1, const ResidentFrame &F2, const std::vector<int> &vMatches12, float R21[9],
                   float t21[3], std::vector<float> &vP3D, std::vector<bool> &vbTriangulated) {
    if ((int)vMatches12.size() != F1.N()) check(VSG_ERR_INVALID, "vsg::ResidentTwoViewReconstruction");
    begin(vMatches12);
    check(vsg_frame_two_view_reconstruct(F1.handle(), F2.handle(), matches_.data(), mK_, &params_, mMaxIterations_, sets_.data(),
                                         &res_, tri_.data(), x3d_.data(), nullptr, nullptr, nullptr, nullptr),
          "vsg_frame_two_view_reconstruct");
    return end(R21, t21, vP3D, vbTriangulated);
  }
  bool Reconstruct(const std::vector<vsg_keypoint> &vKeys1, const std::vector<vsg_keypoint> &vKeys2,
                   const std::vector<int> &vMatches12, float R21[9], float t21[3], std::vector<float> &vP3D,
                   std::vector<bool> &vbTriangulated) {
    if (vMatches12.size() != vKeys1.size()) check(VSG_ERR_INVALID, "vsg::ResidentTwoViewReconstruction");
    std::vector<float> xy1(2 * vKeys1.size() + 2), xy2(2 * vKeys2.size() + 2);
    for (size_t i = 0; i < vKeys1.size(); ++i) xy1[2 * i] = vKeys1[i].x, xy1[2 * i + 1] = vKeys1[i].y;
    for (size_t i = 0; i < vKeys2.size(); ++i) xy2[2 * i] = vKeys2[i].x, xy2[2 * i + 1] = vKeys2[i].y;
    begin(vMatches12);
    check(vsg_two_view_reconstruct(device_, xy1.data(), (int)vKeys1.size(), xy2.data(), (int)vKeys2.size(), matches_.data(), mK_,
                                   &params_, mMaxIterations_, sets_.data(), &res_, tri_.data(), x3d_.data(), nullptr, nullptr,
                                   nullptr, nullptr),
          "vsg_two_view_reconstruct");
    return end(R21, t21, vP3D, vbTriangulated);
  }
  const vsg_two_view_result &result() const { return res_; }
  const std::vector<int32_t> &sets() const { return sets_; }  // mvSets, 8 per iteration

 private:
  void begin(const std::vector<int> &vMatches12) {
    matches_.assign(vMatches12.begin(), vMatches12.end());
    int N = 0;
    for (int m : vMatches12) N += m >= 0 ? 1 : 0;
    if (N < 8 || mMaxIterations_ < 1) check(VSG_ERR_INVALID, "vsg::ResidentTwoViewReconstruction");
    sets_.assign(8 * (size_t)mMaxIterations_, 0);
    check(vsg_two_view_draw_sets(N, mMaxIterations_, randomInt_, randomCtx_, sets_.data()), "vsg_two_view_draw_sets");
    tri_.assign(matches_.size() + 1, 0), x3d_.assign(3 * matches_.size() + 3, 0.0f);
  }
  bool end(float R21[9], float t21[3], std::vector<float> &vP3D, std::vector<bool> &vbTriangulated) {
    if (!res_.ok) return false;
    for (int k = 0; k < 9; ++k) R21[k] = res_.R21[k];
    for (int k = 0; k < 3; ++k) t21[k] = res_.t21[k];
    const size_t n1 = matches_.size();
    vbTriangulated.assign(n1, false);
    for (size_t i = 0; i < n1; ++i) vbTriangulated[i] = tri_[i] != 0;
    if (res_.model == VSG_TWO_VIEW_F) vP3D.assign(x3d_.begin(), x3d_.begin() + 3 * n1);  // :528; never on the H path
    return true;
  }
  float mK_[9];
  vsg_two_view_params params_;
  int mMaxIterations_, device_;
  int (*randomInt_)(int, int, void *);
  void *randomCtx_;
  std::vector<int32_t> matches_, sets_;
  std::vector<uint8_t> tri_;
  std::vector<float> x3d_;
  vsg_two_view_result res_;
};

}  // namespace vsg
