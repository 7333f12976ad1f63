// The RGB-D Frame through include/vsg_orb_adaptor.hpp from plain C++: a synthetic 640x480 frame and a seeded uint16 depth
// plane with holes, seen through the RealSense D435i camera (BASELINE C5) -> vsg::ResidentFrame::ExtractIntoRGBD.
// mvKeys, mvKeysUn, mvuRight, mvDepth and the depth plane are dumped to a flat binary file that
// tests/test_gpu_rgbd.py compares with tests/rgbd_reference.py.  Without a device the extractor throws (exit 3).
//   usage: rgbd_check <out.bin>
#include <cstdio>
#include <fstream>

#include "vsg_orb_adaptor.hpp"
#include "vsg_synth.h"

template <class T>
static void dump(std::ofstream &f, const std::vector<T> &v) {
  int32_t n = (int32_t)v.size();
  f.write((const char *)&n, 4);
  if (n) f.write((const char *)v.data(), sizeof(T) * v.size());
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  // RGBD.DepthMapFactor: 1000.0 (RealSense_D435i.yaml) -- host arithmetic, no device needed
  const float factor = vsg::ResidentFrame::DepthMapScale(1000.0f);
  printf("DepthMapScale %.9g %.9g\n", factor, vsg::ResidentFrame::DepthMapScale(0.0f));
  try {
    const int W = 640, H = 480;
    std::vector<uint8_t> img(W * H);
    if (vsg_synth_sequence_frame(W, H, 5, 0, 1, 6, img.data(), W)) return 2;
    // depth rows padded to 700 elements; every 7th pixel of a 3-pixel-wide diagonal band is a hole
    const int ds = 700;
    std::vector<uint16_t> depth((size_t)H * ds, 0xFFFF);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        depth[(size_t)y * ds + x] = ((x + y) % 7 == 0) ? 0 : (uint16_t)(500 + (x * 13 + y * 7) % 4000);
    const float K4[4] = {616.5911254882812f, 616.6796264648438f, 324.2193603515625f, 239.42701721191406f};
    const float dist[4] = {0.125323f, -0.251452f, 0.000712f, 0.006217f};
    float bounds[4];
    vsg::ResidentFrame::ImageBounds(W, H, K4, dist, 4, bounds);

    vsg::ORBextractor ex(1000, 1.2f, 8, 20, 7);
    vsg::ResidentFrame f(ex.capacity(H, W));
    std::vector<vsg_keypoint> keys, keysUn;
    std::vector<uint8_t> desc;
    std::vector<float> uRight, mDepth;
    const int lap[2] = {0, 0};
    const float mbf = 40.0f;  // Camera.bf of RealSense_D435i.yaml
    const int mono = f.ExtractIntoRGBD(ex, img.data(), H, W, W, lap, depth.data(), VSG_DEPTH_U16, ds * 2, factor, mbf,
                                       keys, desc, K4, dist, 4, bounds[0], bounds[1], bounds[2], bounds[3], &keysUn,
                                       uRight, mDepth);
    std::ofstream out(argv[1], std::ios::binary);
    const std::vector<int32_t> head = {mono, f.N(), W, H, ds};
    const std::vector<float> params = {factor, mbf};
    dump(out, head);
    dump(out, params);
    dump(out, keys);
    dump(out, keysUn);
    dump(out, uRight);
    dump(out, mDepth);
    dump(out, depth);
    printf("OK %d %zu\n", mono, keys.size());
    return 0;
  } catch (const std::exception &e) {
    printf("THROW %s\n", e.what());
    return 3;
  }
}
