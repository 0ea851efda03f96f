// A C++ consumer of the global-bundle-adjustment seam of psl-slam_amd/host/pslfe.hpp (pslfe::Optimizer::BundleAdjustment, the calls
// of Tracking::CreateInitialMapMonocular src/Tracking.cc:782 and LoopClosing::RunGlobalBundleAdjustment src/LoopClosing.cc:650), and
// the plain one-core host loop of the same restatement.  Who owns what: the arithmetic is psl-slam_amd/csrc/ba_kernels.h, the driver
// psl_gba_optimize and its steps psl-slam_amd/csrc/gba_kernels.h, written over an executor; the loop here is that driver on
// PslLmSerial, the library runs it on PslLmGrid (a step = a launch over the whole device).  tests/test_global_ba_gpu.py builds this
// program with g++ and compares all three forms with the restatement of tests/gba_cases.py; built with -DPSL_GBA_HOST_ONLY it needs
// neither the library nor a GPU (tests/test_global_ba_cpu.py runs that build under the address and undefined-behaviour sanitizers;
// tools/bench_global_ba.py times it).
//
// usage: gba_main <cases.bin> <out.bin> [repeat]
//   cases.bin: int32 K, iterations, robust, max_keyframes, max_points, max_edges; PslCamera cam;
//              K x { int32 nkf, nmp, ne; PslBaKeyFrame kf[nkf]; PslMapPointGeom mp[nmp]; PslBaEdge edges[ne] }
//   out.bin:   one section per form - "loop", then (library builds) "device" (rows in HBM, in place) and "host" (host arrays; a
//              refused problem keeps its rows and reports the status alone) - each
//              K x { PslGbaInfo info; PslBaKeyFrame kf[nkf]; PslMapPointGeom mp[nmp]; u8 not_included[nmp] }
//   stdout:    {"problems": K, "loop_ms": the host loop over the K problems, best of `repeat`}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#ifndef PSL_GBA_HOST_ONLY
#include "../../psl-slam_amd/host/pslfe.hpp"
#else
#include "../../include/pslfe.h"
#endif
#include "../../psl-slam_amd/csrc/gba_kernels.h"

namespace {

const double kSinCosTab[444] = {
#include "../../psl-slam_amd/csrc/psl_sincostab.inc"
};

struct Case {
    std::vector<PslBaKeyFrame> kf;
    std::vector<PslMapPointGeom> mp;
    std::vector<PslBaEdge> ed;
};
struct Result {
    PslGbaInfo info;
    std::vector<PslBaKeyFrame> kf;
    std::vector<PslMapPointGeom> mp;
    std::vector<uint8_t> notIncluded;
};

Result unchanged(const Case& c, int status) {
    Result R;
    memset(&R.info, 0, sizeof(R.info));
    R.info.status = status;
    R.kf = c.kf; R.mp = c.mp;
    R.notIncluded.assign(c.mp.size(), 0);
    return R;
}

// one problem on one core: the checks and the lists of pslfe_gba_optimize_device, then psl_gba_optimize
Result hostLoop(const Case& c, const PslCamera& cam, int iterations, int robust, int ckf, int cmp, int ced) {
    const int nkf = (int)c.kf.size(), nmp = (int)c.mp.size(), ne = (int)c.ed.size();
    if (nkf > ckf || nmp > cmp || ne > ced) return unchanged(c, PSLFE_E_CAPACITY);
    if (psl_ba_check_rows(c.ed.data(), nkf, nmp, ne) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    PslGbaWs G;
    std::vector<double> store(psl_gba_carve(nullptr, nkf, nmp, ne, &G) / sizeof(double) + 1, 0.0);
    psl_gba_carve(reinterpret_cast<char*>(store.data()), nkf, nmp, ne, &G);
    PslBaWs& W = G.B;
    W.kf = c.kf.data(); W.mp = c.mp.data(); W.ed = c.ed.data();
    W.nkf = nkf; W.nmp = nmp; W.ne = ne;
    W.K.fx = cam.fx; W.K.fy = cam.fy; W.K.cx = cam.cx; W.K.cy = cam.cy; W.K.bf = cam.bf;
    W.sctab = kSinCosTab;
    if (psl_ba_lists_host(W) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    Result R = unchanged(c, PSLFE_OK);
    PslLmSerial X = {W.scal + 8};
    const PslGbaResult r = psl_gba_optimize(X, G, iterations, robust, R.kf.data(), R.mp.data(), R.notIncluded.data());
    R.info.iterations = r.iterations; R.info.free_keyframes = r.free_keyframes; R.info.included_points = r.included_points;
    R.info.chi2_start = r.chi2_start; R.info.chi2_end = r.chi2_end; R.info.lambda = r.lambda;
    return R;
}

bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs) {
        if (fwrite(&r.info, sizeof(PslGbaInfo), 1, o) != 1) return false;
        if (!r.kf.empty() && fwrite(r.kf.data(), sizeof(PslBaKeyFrame), r.kf.size(), o) != r.kf.size()) return false;
        if (!r.mp.empty() && fwrite(r.mp.data(), sizeof(PslMapPointGeom), r.mp.size(), o) != r.mp.size()) return false;
        if (!r.notIncluded.empty() && fwrite(r.notIncluded.data(), 1, r.notIncluded.size(), o) != r.notIncluded.size()) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin [repeat]\n", argv[0]); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[6];
    PslCamera cam;
    if (fread(hdr, 4, 6, f) != 6 || fread(&cam, sizeof(cam), 1, f) != 1 || hdr[0] < 0 || hdr[1] < 1 || hdr[2] < 0 || hdr[2] > 1 || hdr[3] < 1 || hdr[4] < 1 ||
        hdr[5] < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int K = hdr[0], iterations = hdr[1], robust = hdr[2], ckf = hdr[3], cmp = hdr[4], ced = hdr[5];
    std::vector<Case> cases(K);
    for (Case& c : cases) {
        int32_t n[3] = {0, 0, 0};
        if (fread(n, 4, 3, f) != 3 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[0] > (1 << 20) || n[1] > (1 << 26) || n[2] > (1 << 26)) { fprintf(stderr, "bad case\n"); return 2; }
        c.kf.resize(n[0]); c.mp.resize(n[1]); c.ed.resize(n[2]);
        if ((n[0] && fread(c.kf.data(), sizeof(PslBaKeyFrame), n[0], f) != (size_t)n[0]) || (n[1] && fread(c.mp.data(), sizeof(PslMapPointGeom), n[1], f) != (size_t)n[1]) ||
            (n[2] && fread(c.ed.data(), sizeof(PslBaEdge), n[2], f) != (size_t)n[2])) {
            fprintf(stderr, "short case\n");
            return 2;
        }
    }
    fclose(f);

    std::vector<Result> loop(K);
    double best = -1.0;
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; ++k) loop[k] = hostLoop(cases[k], cam, iterations, robust, ckf, cmp, ced);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (best < 0 || ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !writeSection(o, loop)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
#ifndef PSL_GBA_HOST_ONLY
    try {
        pslfe::Context ctx(0);
        std::vector<Result> dev(K), host(K);
        if (K) {
            pslfe::GlobalBundleAdjuster gba(ctx, ckf, cmp, ced);
            for (int k = 0; k < K; ++k) {
                const Case& c = cases[k];
                // rows in HBM, in place, as the chain behind the Initializer or OptimizeEssentialGraph leaves them
                const size_t kb = c.kf.size() * sizeof(PslBaKeyFrame), pb = c.mp.size() * sizeof(PslMapPointGeom), eb = c.ed.size() * sizeof(PslBaEdge);
                void *dK = nullptr, *dP = nullptr, *dE = nullptr, *dN = nullptr;
                pslfe::check(pslfe_device_alloc(ctx.get(), kb ? kb : 1, &dK), "alloc");
                pslfe::check(pslfe_device_alloc(ctx.get(), pb ? pb : 1, &dP), "alloc");
                pslfe::check(pslfe_device_alloc(ctx.get(), eb ? eb : 1, &dE), "alloc");
                pslfe::check(pslfe_device_alloc(ctx.get(), c.mp.size() ? c.mp.size() : 1, &dN), "alloc");
                if (kb) pslfe::check(pslfe_device_upload(ctx.get(), dK, c.kf.data(), kb), "upload");
                if (pb) pslfe::check(pslfe_device_upload(ctx.get(), dP, c.mp.data(), pb), "upload");
                if (eb) pslfe::check(pslfe_device_upload(ctx.get(), dE, c.ed.data(), eb), "upload");
                dev[k] = unchanged(c, PSLFE_OK);
                const int rc = pslfe_gba_optimize_device(gba.get(), (const PslBaKeyFrame*)dK, (int)c.kf.size(), (const PslMapPointGeom*)dP, (int)c.mp.size(),
                                                         (const PslBaEdge*)dE, (int)c.ed.size(), &cam, iterations, robust, (PslBaKeyFrame*)dK,
                                                         (PslMapPointGeom*)dP, (uint8_t*)dN, &dev[k].info);
                if (rc != PSLFE_OK && rc != PSLFE_E_CAPACITY && rc != PSLFE_E_INVALID) pslfe::check(rc, "pslfe_gba_optimize_device");
                if (kb) pslfe::check(pslfe_device_download(ctx.get(), dev[k].kf.data(), dK, kb), "download");
                if (pb) pslfe::check(pslfe_device_download(ctx.get(), dev[k].mp.data(), dP, pb), "download");
                if (pb) pslfe::check(pslfe_device_download(ctx.get(), dev[k].notIncluded.data(), dN, c.mp.size()), "download");
                for (void* p : {dK, dP, dE, dN}) pslfe_device_free(ctx.get(), p);
                // host arrays, as Tracking and LoopClosing would call it
                host[k] = unchanged(c, PSLFE_OK);
                try {
                    host[k].info = pslfe::Optimizer::BundleAdjustment(gba, host[k].kf, host[k].mp, c.ed, cam, host[k].notIncluded, iterations, robust != 0);
                } catch (const pslfe::Error& e) {
                    if (e.code != PSLFE_E_CAPACITY && e.code != PSLFE_E_INVALID) throw;
                    host[k] = unchanged(c, e.code);
                }
            }
        }
        if (!writeSection(o, dev) || !writeSection(o, host)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
#endif
    if (fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    printf("{\"problems\": %d, \"loop_ms\": %.6f}\n", K, best);
    return 0;
}
