// A C++ consumer of the Initializer seam of psl-slam_amd/host/pslfe.hpp (pslfe::Initializer, the two-view map initialisation of
// Tracking::MonocularInitialization src/Tracking.cc:659-760 carried through :710-719), and the plain C++ loop of the same restatement
// on one core.  Who owns what: the arithmetic, the draw and the reference's loop psl_init_initialize_host are
// psl-slam_amd/csrc/initializer_kernels.h; the kernel shares the arithmetic (the header of psl-slam_amd/csrc/pslfe_initializer.hip).
// tests/test_initializer_gpu.py builds this program with g++ against the library and compares both forms with the numpy restatement
// (tests/initializer_cases.py); built with -DPSL_INIT_HOST_ONLY it needs neither the library nor a GPU (tests/test_initializer_cpu.py
// runs that build, also under the address and undefined-behaviour sanitizers; tools/bench_initializer.py times it).
//
// usage: init_main <cases.bin> <out.bin> [repeat]
//        init_main --sets <N> <seed> <iterations> <out.bin>     mvSets, int32 [iterations][8]
//        init_main --acosf <in.bin> <out.bin>                   psl_acosf of every float of in.bin
//        init_main --select <in.bin> <out.bin>                  the floats of in.bin as a vCosParallax: uint32 key of each
//                                                               (psl_init_cos_key), then the float at sorted index min(50, n - 1)
//   cases.bin: int32 K; K x { PslCamera cam; uint32 seed; int32 n1, n2, max_its; float sigma; float keys1[n1][2]; float keys2[n2][2];
//              int32 matches12[n1] }
//   out.bin:   one section per form - "loop", then (library builds) "mirror" (pslfe::Initializer::Initialize) - each K x {
//              PslInitResult; float p3d[n1][3]; u8 triangulated[n1]; int32 mvIniMatches[n1] after :712-719 }
//   stdout:    {"pairs": K, "loop_ms": the host loop over the K pairs, best of `repeat`}
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#ifndef PSL_INIT_HOST_ONLY
#include "../../psl-slam_amd/host/pslfe.hpp"
#else
#include "../../include/pslfe.h"
#endif
#include "../../psl-slam_amd/csrc/initializer_kernels.h"

namespace {

struct Case {
    PslCamera cam;
    uint32_t seed = 0;
    int maxIts = 0;
    float sigma = 1.f;
    std::vector<float> keys1, keys2;
    std::vector<int32_t> matches;
};
struct Result {
    PslInitResult res;
    std::vector<float> p3d;
    std::vector<uint8_t> tri;
    std::vector<int32_t> ini;
};

Result hostLoop(const Case& c) {
    const PslCamera& cam = c.cam;
    const int n1 = (int)c.keys1.size() / 2, n2 = (int)c.keys2.size() / 2;
    std::vector<float> ws(PSL_INIT_WS_F, 0.f);
    std::vector<double> wd(PSL_INIT_WS_D, 0.0);
    std::vector<int32_t> rowI((size_t)n1 + 1);
    std::vector<uint32_t> keybuf((size_t)n1 + 1);
    Result R;
    R.p3d.assign(3 * (size_t)n1 + 3, 0.f);
    R.tri.assign((size_t)n1 + 1, 0);
    R.ini.assign((size_t)n1 + 1, -1);
    psl_init_initialize_host(c.keys1.data(), n1, c.keys2.data(), n2, 2, c.matches.data(), &cam, c.sigma, c.maxIts, c.seed, ws.data(), wd.data(),
                             rowI.data(), keybuf.data(), &R.res, R.p3d.data(), R.tri.data(), R.ini.data());
    R.p3d.resize(3 * (size_t)n1); R.tri.resize((size_t)n1); R.ini.resize((size_t)n1);
    return R;
}

bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs) {
        if (fwrite(&r.res, sizeof(PslInitResult), 1, o) != 1) return false;
        if (!r.p3d.empty() && fwrite(r.p3d.data(), 4, r.p3d.size(), o) != r.p3d.size()) return false;
        if (!r.tri.empty() && fwrite(r.tri.data(), 1, r.tri.size(), o) != r.tri.size()) return false;
        if (!r.ini.empty() && fwrite(r.ini.data(), 4, r.ini.size(), o) != r.ini.size()) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "--sets")) {
        const int N = atoi(argv[2]), its = atoi(argv[4]);
        if (N < 8 || its < 0) { fprintf(stderr, "bad --sets arguments\n"); return 2; }
        PslRsRand G;
        psl_rs_srand(&G, (uint32_t)strtoul(argv[3], nullptr, 10));
        std::vector<int32_t> out(8 * (size_t)its);
        for (int i = 0; i < its; ++i) {
            int idx[8];
            psl_rs_draw<8>(&G, N, idx);
            for (int j = 0; j < 8; ++j) out[8 * (size_t)i + j] = idx[j];
        }
        FILE* o = fopen(argv[5], "wb");
        if (!o || (!out.empty() && fwrite(out.data(), 4, out.size(), o) != out.size())) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
        fclose(o);
        return 0;
    }
    if (argc == 4 && (!strcmp(argv[1], "--acosf") || !strcmp(argv[1], "--select"))) {
        const bool select = !strcmp(argv[1], "--select");
        FILE* f = fopen(argv[2], "rb");
        if (!f) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
        std::vector<float> v;
        float buf[4096];
        size_t n;
        while ((n = fread(buf, 4, 4096, f)) > 0) v.insert(v.end(), buf, buf + n);
        fclose(f);
        std::vector<uint32_t> keys;
        float picked = 0.f;
        if (select) {
            if (v.empty()) { fprintf(stderr, "--select needs at least one float\n"); return 2; }
            for (float x : v) keys.push_back(psl_init_cos_key(x));
            std::vector<uint32_t> work(keys);
            picked = psl_init_cos_unkey(psl_init_select_key(work.data(), (int)work.size()));
        } else {
            for (float& x : v) x = psl_acosf(x);
        }
        FILE* o = fopen(argv[3], "wb");
        const bool ok = o && (select ? fwrite(keys.data(), 4, keys.size(), o) == keys.size() && fwrite(&picked, 4, 1, o) == 1
                                     : (v.empty() || fwrite(v.data(), 4, v.size(), o) == v.size()));
        if (!ok) { fprintf(stderr, "cannot write %s\n", argv[3]); return 2; }
        fclose(o);
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: init_main <cases.bin> <out.bin> [repeat]\n"); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int32_t K = 0;
    if (fread(&K, 4, 1, f) != 1 || K < 0) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<Case> cases((size_t)K);
    for (Case& c : cases) {
        int32_t hdr[3];
        if (fread(&c.cam, sizeof(c.cam), 1, f) != 1 || fread(&c.seed, 4, 1, f) != 1 || fread(hdr, 4, 3, f) != 3 || fread(&c.sigma, 4, 1, f) != 1 || hdr[0] < 0 || hdr[1] < 0) {
            fprintf(stderr, "bad case\n");
            return 2;
        }
        c.maxIts = hdr[2];
        c.keys1.resize(2 * (size_t)hdr[0]); c.keys2.resize(2 * (size_t)hdr[1]); c.matches.resize((size_t)hdr[0]);
        if ((hdr[0] && fread(c.keys1.data(), 8, (size_t)hdr[0], f) != (size_t)hdr[0]) ||
            (hdr[1] && fread(c.keys2.data(), 8, (size_t)hdr[1], f) != (size_t)hdr[1]) ||
            (hdr[0] && fread(c.matches.data(), 4, (size_t)hdr[0], f) != (size_t)hdr[0])) {
            fprintf(stderr, "short case\n");
            return 2;
        }
    }
    fclose(f);
    std::vector<Result> loop;
    double best = 1e300;
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r) {
        loop.clear();
        const auto t0 = std::chrono::steady_clock::now();
        for (const Case& c : cases) loop.push_back(hostLoop(c));
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !writeSection(o, loop)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
#ifndef PSL_INIT_HOST_ONLY
    try {
        pslfe::Context ctx(0);
        std::vector<Result> mirror;
        for (const Case& c : cases) {
            // the loop of INTEGRATION.md §6b: Initializer(mInitialFrame, 1.0, 200), Initialize(mCurrentFrame, mvIniMatches, ...), :712-719
            Result R;
            pslfe::Initializer init(ctx, c.keys1, c.cam, c.sigma, c.maxIts, c.seed);
            float R21[9], t21[3];
            std::vector<bool> vbTriangulated;
            R.ini = c.matches;
            if (init.Initialize(c.keys2, R.ini, R21, t21, R.p3d, vbTriangulated)) {
                for (size_t i = 0; i < R.ini.size(); ++i)
                    if (R.ini[i] >= 0 && !vbTriangulated[i]) R.ini[i] = -1;
            }
            R.res = init.result();
            R.tri.assign(vbTriangulated.size(), 0);
            for (size_t i = 0; i < vbTriangulated.size(); ++i) R.tri[i] = vbTriangulated[i] ? 1 : 0;
            mirror.push_back(R);
        }
        if (!writeSection(o, mirror)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    } catch (const std::exception& e) {
        fprintf(stderr, "init_main: %s\n", e.what());
        return 1;
    }
#endif
    fclose(o);
    printf("{\"pairs\": %d, \"loop_ms\": %.3f}\n", (int)K, best);
    return 0;
}
