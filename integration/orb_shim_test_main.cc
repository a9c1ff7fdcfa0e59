// CI driver of integration/orb_extractor_hip.h: one frame through ORBextractorHIP::operator() with stand-in cv::KeyPoint / cv::Mat types,
// the caller's sampling pattern and a stand-in for the caller's DistributeOctTree (the N candidates of largest response, ties by
// position in the list, kept in list order).  Every key point and descriptor is dumped for comparison with the Python path.
//   input:  width height nlevels scaleFactor iniThFAST minThFAST nfeatures capacity, the 1024 pattern integers, the image's bytes as integers
//   output: n, then per key point  pt.x pt.y size angle response octave  and the 32 descriptor bytes
//   usage: orb_shim_test <frame.txt> <output.txt> [device]; exit codes: shim_driver.h
#include <algorithm>
#include <cstdio>
#include <fstream>
#include <numeric>
#include <vector>

#include "orb_extractor_hip.h"
#include "shim_driver.h"

namespace standin {
struct OrbPoint2f { float x, y; };
struct OrbKeyPoint {                           // cv::KeyPoint
  OrbPoint2f pt;
  float size, angle, response;
  int octave;
};
struct OrbMat {                                // cv::Mat, CV_8UC1
  const uint8_t* data = nullptr;
  int rows = 0, cols = 0;
  size_t step = 0;
};
}  // namespace standin

using namespace standin;

static std::vector<OrbKeyPoint> top_n(const std::vector<OrbKeyPoint>& keys, int, int, int, int, int N, int) {
  std::vector<int> order(keys.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return keys[a].response > keys[b].response; });
  if ((int)order.size() > N) order.resize(N > 0 ? N : 0);
  std::sort(order.begin(), order.end());
  std::vector<OrbKeyPoint> out;
  for (int i : order) out.push_back(keys[i]);
  return out;
}

static int drive(const DriverArgs& arg) {
  std::ifstream in(arg.in[0]);
  int width, height, nlevels, ini, min, nfeatures, capacity;
  float scale;
  in >> width >> height >> nlevels >> scale >> ini >> min >> nfeatures >> capacity;
  if (!in || width < 1 || height < 1 || width > 16384 || height > 16384) return driver_bad_input(arg.in[0]);
  std::vector<int> pattern(1024);
  for (int& p : pattern) in >> p;
  const int stride = width + 5;                  // rows with padding, as a cv::Mat view may have
  std::vector<uint8_t> pixels((size_t)stride * height, 0);
  for (int y = 0; y < height; y++)
    for (int x = 0; x < width; x++) { int v; in >> v; pixels[(size_t)y * stride + x] = (uint8_t)v; }
  if (!in) return driver_bad_input(arg.in[0]);

  defslam_hip::ORBextractorHIP<OrbKeyPoint> extractor(arg.ctx, width, height, nfeatures, scale, nlevels, ini, min, pattern.data(), top_n, capacity);
  if (extractor.status() != DSH_OK) return driver_fail(arg.ctx, "ORBextractorHIP");
  OrbMat image, mask;
  image.data = pixels.data(); image.rows = height; image.cols = width; image.step = (size_t)stride;
  std::vector<OrbKeyPoint> keypoints;
  std::vector<uint8_t> descriptors;
  if (!extractor(image, mask, keypoints, descriptors)) return driver_fail(arg.ctx, "ORBextractorHIP::operator()");
  std::fprintf(arg.out, "%zu\n", keypoints.size());
  for (size_t i = 0; i < keypoints.size(); i++) {
    const OrbKeyPoint& k = keypoints[i];
    std::fprintf(arg.out, "%.9g %.9g %.9g %.9g %.9g %d", k.pt.x, k.pt.y, k.size, k.angle, k.response, k.octave);
    for (int b = 0; b < 32; b++) std::fprintf(arg.out, " %d", (int)descriptors[32 * i + b]);
    std::fprintf(arg.out, "\n");
  }
  return 0;
}

int main(int argc, char** argv) { return run_driver(argc, argv, 1, drive); }
