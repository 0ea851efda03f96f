// A C++ consumer of the stereo constructor through psl-slam_amd/host/pslfe.hpp: two extractors with the same settings
// (src/Tracking.cc:128-129), left(imLeft) and right(imRight), then FrameGrid::setStereo - the one-frame seam of
// Frame::Frame(imLeft, imRight, ...) src/Frame.cc:75-131.  tests/test_stereo_gpu.py builds it with g++, runs it as a child process
// and compares its output with the Python path.
//
// usage: stereo_main <pair.bin> <nfeatures> <out.bin>
//   pair.bin: int32 w, h; float fx fy cx cy k1 k2 p1 p2 k3 bf; u8 left[h][w]; u8 right[h][w]
//   out.bin:  int32 n; PslKeyPoint mvKeysUn[n]; float mvuRight[n]; float mvDepth[n]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../psl-slam_amd/host/pslfe.hpp"

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s pair.bin nfeatures out.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int wh[2];
    PslCamera cam;
    if (fread(wh, sizeof(int), 2, f) != 2 || fread(&cam, sizeof(cam), 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int w = wh[0], h = wh[1];
    std::vector<uint8_t> imL((size_t)w * h), imR((size_t)w * h);
    if (fread(imL.data(), 1, imL.size(), f) != imL.size() || fread(imR.data(), 1, imR.size(), f) != imR.size()) {
        fprintf(stderr, "short images\n");
        return 2;
    }
    fclose(f);
    try {
        pslfe::Context ctx(0);
        const int nfeatures = atoi(argv[2]);
        pslfe::ORBextractor left(ctx, nfeatures, 1.2f, 8, 20, 7), right(ctx, nfeatures, 1.2f, 8, 20, 7);
        std::vector<PslKeyPoint> kL, kR;
        std::vector<uint8_t> dL, dR;
        left(imL.data(), w, h, w, kL, dL);
        right(imR.data(), w, h, w, kR, dR);
        const int cap = std::max(pslfe_orb_max_keypoints(left.get(), w, h), 1);
        pslfe::FrameGrid grid(ctx, cap, 1);
        grid.setStereo(0, left, right, cam);
        std::vector<PslKeyPoint> un;
        std::vector<float> depth, uright;
        grid.fetch(0, un, depth, uright, cap);
        FILE* o = fopen(argv[3], "wb");
        if (!o) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        const int n = (int)un.size();
        fwrite(&n, sizeof(int), 1, o);
        fwrite(un.data(), sizeof(PslKeyPoint), n, o);
        fwrite(uright.data(), sizeof(float), n, o);
        fwrite(depth.data(), sizeof(float), n, o);
        fclose(o);
        printf("{\"n\": %d, \"left\": %zu, \"right\": %zu}\n", n, kL.size(), kR.size());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
