// Host integration shim of the ORB front end (include/defslam_hip.h: dsh_orb_create, dsh_orb_detect, dsh_orb_describe):
//
//   ORBextractorHIP<KeyPointT>(ctx, width, height, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, bit_pattern_31_, distribute)
//   extractor(image, mask, keypoints, descriptors)
//       drop-in for ORB_SLAM2::ORBextractor::operator() (Thirdparty/ORBSLAM_2/src/ORBextractor.cc:1047-1118): ComputePyramid, the FAST
//       corners of ComputeKeyPointsOctTree, the orientations and the descriptors run on the device; between them the caller's own
//       DistributeOctTree runs on the host, per level, over key points built as the reference builds them (:825-830: pt relative to
//       (minBorderX, minBorderY), the response of cv::FAST, size 7, angle -1).  What comes back gets the border added, octave, size
//       (:841-851), the angle, pt *= scale for level > 0 (:1108-1113), and is appended in level order.
//       bit_pattern_31_ is the caller's: the reference's 256 x 4 table (ORBextractor.cc:150-408) is not part of this library.
//       Returns false when the library fails (dsh_last_error of the context has the text) or when a mask is given: ComputePyramid with a
//       mask and runByPixelsMask are not covered.  Not covered either: ComputeKeyPointsOld, Frame's undistortion of the key points.
//   The OpenCV steps behind it (resize, copyMakeBorder, GaussianBlur, FAST, fastAtan2) are the readings stated in include/defslam_hip.h,
//   not verified against an OpenCV build.
//
// Templates over the reference's classes; the type-specific accessors are OrbImageAccess<ImageT> and OrbDescriptorAccess<DescT>: cv::Mat
// in DefSLAM (data, rows, cols, step[0]; create(n, 32, CV_8U) and ptr()), plain members in the stand-ins of the CI driver.
#pragma once
#include <cmath>
#include <cstdint>
#include <functional>
#include <vector>

#include "../include/defslam_hip.h"

namespace defslam_hip {

template <class ImageT>
struct OrbImageAccess {
  static bool empty(const ImageT& m) { return m.data == nullptr || m.rows == 0 || m.cols == 0; }
  static const uint8_t* data(const ImageT& m) { return m.data; }
  static int rows(const ImageT& m) { return m.rows; }
  static int cols(const ImageT& m) { return m.cols; }
  static int64_t step(const ImageT& m) { return (int64_t)m.step; }
};

template <class DescT>
struct OrbDescriptorAccess {
  // n rows of 32 bytes; n == 0 releases
  static uint8_t* create(DescT& d, int n) { d.assign(32 * (size_t)n, 0); return d.data(); }
};

template <class KeyPointT>
class ORBextractorHIP {
 public:
  // the caller's DistributeOctTree(vToDistributeKeys, minX, maxX, minY, maxY, N, level)
  typedef std::function<std::vector<KeyPointT>(const std::vector<KeyPointT>&, int, int, int, int, int, int)> Distribute;

  ORBextractorHIP(dsh_ctx* ctx, int width, int height, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                  const int* bit_pattern_31, Distribute distribute, int capacity = 8192)
      : nlevels_(nlevels), capacity_(capacity), distribute_(distribute) {
    dsh_orb_config cfg;
    cfg.ctx = ctx; cfg.width = width; cfg.height = height; cfg.levels = nlevels; cfg.scale_factor = scaleFactor;
    cfg.ini_th_fast = iniThFAST; cfg.min_th_fast = minThFAST; cfg.capacity = capacity; cfg.pattern = bit_pattern_31;
    status_ = dsh_orb_create(&cfg, &orb_);
    if (status_ != DSH_OK) return;
    wh_.resize(2 * (size_t)nlevels);
    mvScaleFactor.resize(nlevels);
    status_ = dsh_orb_level_sizes(orb_, wh_.data(), mvScaleFactor.data());
    // mnFeaturesPerLevel, ORBextractor.cc:435-446
    mnFeaturesPerLevel.resize(nlevels);
    const float factor = 1.0f / scaleFactor;
    float nDesiredFeaturesPerScale = nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nlevels));
    int sumFeatures = 0;
    for (int level = 0; level < nlevels - 1; level++) {
      mnFeaturesPerLevel[level] = (int)std::rint(nDesiredFeaturesPerScale);
      sumFeatures += mnFeaturesPerLevel[level];
      nDesiredFeaturesPerScale *= factor;
    }
    mnFeaturesPerLevel[nlevels - 1] = nfeatures - sumFeatures > 0 ? nfeatures - sumFeatures : 0;
  }
  ~ORBextractorHIP() { if (orb_) dsh_orb_destroy(orb_); }
  ORBextractorHIP(const ORBextractorHIP&) = delete;
  ORBextractorHIP& operator=(const ORBextractorHIP&) = delete;

  int status() const { return status_; }
  std::vector<float> mvScaleFactor;
  std::vector<int> mnFeaturesPerLevel;

  template <class ImageT, class DescT>
  bool operator()(const ImageT& image, const ImageT& mask, std::vector<KeyPointT>& _keypoints, DescT& _descriptors) {
    typedef OrbImageAccess<ImageT> Im;
    if (status_ != DSH_OK) return false;
    if (Im::empty(image)) return true;                                // :1050
    if (!Im::empty(mask)) return false;                               // not covered
    if (Im::cols(image) != wh_[0] || Im::rows(image) != wh_[1]) return false;
    const int EDGE_THRESHOLD = 19, PATCH_SIZE = 31;
    counts_.resize(nlevels_);
    cand_.resize(3 * (size_t)nlevels_ * capacity_);
    status_ = dsh_orb_detect(orb_, Im::data(image), Im::step(image), counts_.data(), cand_.data());
    if (status_ != DSH_OK) return false;
    std::vector<std::vector<KeyPointT> > allKeypoints(nlevels_);
    std::vector<int32_t> level;
    std::vector<float> xy;
    for (int l = 0; l < nlevels_; l++) {
      const int minBorderX = EDGE_THRESHOLD - 3, minBorderY = minBorderX;
      const int maxBorderX = wh_[2 * l] - EDGE_THRESHOLD + 3, maxBorderY = wh_[2 * l + 1] - EDGE_THRESHOLD + 3;
      std::vector<KeyPointT> vToDistributeKeys(counts_[l]);
      const int32_t* c = &cand_[3 * (size_t)l * capacity_];
      for (int i = 0; i < counts_[l]; i++) {
        KeyPointT& k = vToDistributeKeys[i];
        k.pt.x = (float)(c[3 * i] - minBorderX);
        k.pt.y = (float)(c[3 * i + 1] - minBorderY);
        k.size = 7.f;
        k.angle = -1.f;
        k.response = (float)c[3 * i + 2];
        k.octave = 0;
      }
      std::vector<KeyPointT>& keypoints = allKeypoints[l];
      keypoints = distribute_(vToDistributeKeys, minBorderX, maxBorderX, minBorderY, maxBorderY, mnFeaturesPerLevel[l], l);
      const int scaledPatchSize = (int)(PATCH_SIZE * mvScaleFactor[l]);
      for (KeyPointT& k : keypoints) {                                // :845-851
        k.pt.x += minBorderX;
        k.pt.y += minBorderY;
        k.octave = l;
        k.size = (float)scaledPatchSize;
        level.push_back(l);
        xy.push_back(k.pt.x);
        xy.push_back(k.pt.y);
      }
    }
    const int nkeypoints = (int)level.size();
    uint8_t* desc = OrbDescriptorAccess<DescT>::create(_descriptors, nkeypoints);
    _keypoints.clear();
    _keypoints.reserve(nkeypoints);
    if (nkeypoints == 0) return true;
    angle_.resize(nkeypoints);
    status_ = dsh_orb_describe(orb_, nkeypoints, level.data(), xy.data(), angle_.data(), desc);
    if (status_ != DSH_OK) return false;
    int offset = 0;
    for (int l = 0; l < nlevels_; l++) {
      for (KeyPointT& k : allKeypoints[l]) {
        k.angle = angle_[offset++];
        if (l != 0) { k.pt.x *= mvScaleFactor[l]; k.pt.y *= mvScaleFactor[l]; }   // :1108-1113
      }
      _keypoints.insert(_keypoints.end(), allKeypoints[l].begin(), allKeypoints[l].end());
    }
    return true;
  }

 private:
  dsh_orb* orb_ = nullptr;
  int nlevels_, capacity_, status_ = DSH_OK;
  Distribute distribute_;
  std::vector<int32_t> wh_, counts_, cand_;
  std::vector<float> angle_;
};

}  // namespace defslam_hip
