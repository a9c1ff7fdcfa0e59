// CPU check of integration/standin_store_scene.h: reads a tests/store_model.py scene file and dumps it again, as the drivers dump
// their objects.  No call into the library: tests/test_store_scene_cpu.py runs it where there is no GPU.
//   usage: store_scene_roundtrip <scene.txt> <output.txt>
// Behind the dump: per keyframe with appearance a line "file read app slot | Ow and scale factors (bits) | octaves | descriptor bytes",
// which no store call mutates and the drivers do not dump, then the tail of the scene file, a line "tail .." each.
#include <fstream>
#include <string>

#include "standin_store_scene.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s <scene.txt> <output.txt>\n", argv[0]);
    return 2;
  }
  std::ifstream in(argv[1]);
  standin::StoreScene sc;
  if (!sc.read(in)) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 2;
  }
  std::FILE* o = std::fopen(argv[2], "w");
  if (!o) return 2;
  sc.dump(o, "file", "read", std::vector<standin::LmMapPoint*>());
  for (int k = 0; sc.appearance && k < sc.K; k++) {
    const standin::LmKeyFrame& kf = sc.kfs[k];
    std::vector<float> f(kf.Ow, kf.Ow + 3);
    f.insert(f.end(), kf.mvScaleFactors.begin(), kf.mvScaleFactors.end());
    std::fprintf(o, "file read app %d |", k);
    for (float v : f) {
      uint32_t u;
      std::memcpy(&u, &v, 4);
      std::fprintf(o, " %u", u);
    }
    std::fprintf(o, " |");
    for (const standin::KeyPoint& kp : kf.mvKeysUn) std::fprintf(o, " %d", kp.octave);
    std::fprintf(o, " |");
    for (uint8_t b : kf.mDescriptors) std::fprintf(o, " %d", (int)b);
    std::fprintf(o, "\n");
  }
  std::string line;
  while (std::getline(in, line))
    if (!line.empty()) std::fprintf(o, "tail %s\n", line.c_str());
  std::fclose(o);
  return 0;
}
