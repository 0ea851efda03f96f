// A C++ consumer of the local-bundle-adjustment seam of psl-slam_amd/host/pslfe.hpp (pslfe::Optimizer::LocalBundleAdjustment, the
// call of LocalMapping::Run src/LocalMapping.cc:84), and the plain one-core host loop of the same restatement.  Who owns what: all
// arithmetic and every decision are psl-slam_amd/csrc/ba_kernels.h, written over an executor; the loop here is that text on
// PslLmSerial, the kernel k_ba_local the same text on a workgroup.  tests/test_local_ba_gpu.py builds this program with g++ and
// compares all three forms with the numpy restatement of tests/ba_cases.py; built with -DPSL_BA_HOST_ONLY it needs neither the
// library nor a GPU (tests/test_local_ba_cpu.py runs that build under the address and undefined-behaviour sanitizers;
// tools/bench_local_ba.py times it).
//
// usage: ba_main <cases.bin> <out.bin> [repeat]
//   cases.bin: int32 K, rounds, max_keyframes, max_points, max_edges; PslCamera cam;
//              K x { int32 nkf, nmp, ne; PslBaKeyFrame kf[nkf]; PslMapPointGeom mp[nmp]; PslBaEdge edges[ne] }
//   out.bin:   one section per form - "loop", then (library builds) "device" (the K problems in one launch) and "host" (problem by
//              problem through LocalBundleAdjustment; a refused problem keeps its rows and reports the status alone) - each
//              K x { PslBaInfo info; PslBaKeyFrame kf[nkf]; PslMapPointGeom mp[nmp]; u8 erase[ne] }
//   stdout:    {"problems": K, "loop_ms": the host loop over the K problems, best of `repeat`}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#ifndef PSL_BA_HOST_ONLY
#include "../../psl-slam_amd/host/pslfe.hpp"
#else
#include "../../include/pslfe.h"
#endif
#include "../../psl-slam_amd/csrc/ba_kernels.h"

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
    PslBaInfo info;
    std::vector<PslBaKeyFrame> kf;
    std::vector<PslMapPointGeom> mp;
    std::vector<uint8_t> erase;
};

Result unchanged(const Case& c, int status) {
    Result R;
    memset(&R.info, 0, sizeof(R.info));
    R.info.status = status;
    R.kf = c.kf; R.mp = c.mp;
    R.erase.assign(c.ed.size(), 0);
    return R;
}

// one problem on one core: the checks of k_ba_check and k_ba_lists, then psl_ba_rounds
Result hostLoop(const Case& c, const PslCamera& cam, int rounds, int ckf, int cmp, int ced) {
    const int nkf = (int)c.kf.size(), nmp = (int)c.mp.size(), ne = (int)c.ed.size();
    if (nkf > ckf || nmp > cmp || ne > ced) return unchanged(c, PSLFE_E_CAPACITY);
    if (psl_ba_check_rows(c.ed.data(), nkf, nmp, ne) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    if (!psl_ba_has_work(c.kf.data(), nkf, ne)) return unchanged(c, PSLFE_OK);
    PslBaWs W;
    std::vector<double> store(psl_ba_carve(nullptr, nkf, nmp, ne, &W) / sizeof(double) + 1, 0.0);
    psl_ba_carve(reinterpret_cast<char*>(store.data()), nkf, nmp, ne, &W);
    W.kf = c.kf.data(); W.mp = c.mp.data(); W.ed = c.ed.data();
    W.nkf = nkf; W.nmp = nmp; W.ne = ne;
    W.K.fx = cam.fx; W.K.fy = cam.fy; W.K.cx = cam.cx; W.K.cy = cam.cy; W.K.bf = cam.bf;
    W.sctab = kSinCosTab;
    if (psl_ba_lists_host(W) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    Result R = unchanged(c, PSLFE_OK);
    PslLmSerial X = {W.scal + 8};
    psl_ba_rounds(X, W, rounds, R.kf.data(), R.mp.data(), R.erase.data(), &R.info);
    return R;
}

bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs) {
        if (fwrite(&r.info, sizeof(PslBaInfo), 1, o) != 1) return false;
        if (!r.kf.empty() && fwrite(r.kf.data(), sizeof(PslBaKeyFrame), r.kf.size(), o) != r.kf.size()) return false;
        if (!r.mp.empty() && fwrite(r.mp.data(), sizeof(PslMapPointGeom), r.mp.size(), o) != r.mp.size()) return false;
        if (!r.erase.empty() && fwrite(r.erase.data(), 1, r.erase.size(), o) != r.erase.size()) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin [repeat]\n", argv[0]); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[5];
    PslCamera cam;
    if (fread(hdr, 4, 5, f) != 5 || fread(&cam, sizeof(cam), 1, f) != 1 || hdr[0] < 0 || hdr[1] < 1 || hdr[1] > 2 || hdr[2] < 1 || hdr[3] < 1 || hdr[4] < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int K = hdr[0], rounds = hdr[1], ckf = hdr[2], cmp = hdr[3], ced = hdr[4];
    std::vector<Case> cases(K);
    for (Case& c : cases) {
        int32_t n[3] = {0, 0, 0};
        if (fread(n, 4, 3, f) != 3 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[0] > (1 << 20) || n[1] > (1 << 24) || n[2] > (1 << 26)) { fprintf(stderr, "bad case\n"); return 2; }
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
        for (int k = 0; k < K; ++k) loop[k] = hostLoop(cases[k], cam, rounds, ckf, cmp, ced);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (best < 0 || ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !writeSection(o, loop)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
#ifndef PSL_BA_HOST_ONLY
    try {
        pslfe::Context ctx(0);
        std::vector<Result> dev(K), host(K);
        if (K) {
            pslfe::BundleAdjuster ba(ctx, K, ckf, cmp, ced);
            // the K problems in one launch, HBM to HBM, in place
            std::vector<PslBaKeyFrame> kf;
            std::vector<PslMapPointGeom> mp;
            std::vector<PslBaEdge> ed;
            std::vector<int32_t> koff(1, 0), poff(1, 0), eoff(1, 0);
            for (const Case& c : cases) {
                kf.insert(kf.end(), c.kf.begin(), c.kf.end());
                mp.insert(mp.end(), c.mp.begin(), c.mp.end());
                ed.insert(ed.end(), c.ed.begin(), c.ed.end());
                koff.push_back((int32_t)kf.size()); poff.push_back((int32_t)mp.size()); eoff.push_back((int32_t)ed.size());
            }
            const size_t kb = kf.size() * sizeof(PslBaKeyFrame), pb = mp.size() * sizeof(PslMapPointGeom), eb = ed.size() * sizeof(PslBaEdge);
            const size_t ob = (size_t)(K + 1) * 4, ib = (size_t)K * sizeof(PslBaInfo);
            void *dK = nullptr, *dP = nullptr, *dE = nullptr, *dKo = nullptr, *dPo = nullptr, *dEo = nullptr, *dX = nullptr, *dI = nullptr;
            pslfe::check(pslfe_device_alloc(ctx.get(), kb ? kb : 1, &dK), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), pb ? pb : 1, &dP), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), eb ? eb : 1, &dE), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob, &dKo), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob, &dPo), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob, &dEo), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ed.size() ? ed.size() : 1, &dX), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ib, &dI), "alloc");
            if (kb) pslfe::check(pslfe_device_upload(ctx.get(), dK, kf.data(), kb), "upload");
            if (pb) pslfe::check(pslfe_device_upload(ctx.get(), dP, mp.data(), pb), "upload");
            if (eb) pslfe::check(pslfe_device_upload(ctx.get(), dE, ed.data(), eb), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dKo, koff.data(), ob), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dPo, poff.data(), ob), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dEo, eoff.data(), ob), "upload");
            pslfe::Optimizer::LocalBundleAdjustmentDevice(ba, K, (const PslBaKeyFrame*)dK, (const int32_t*)dKo, (const PslMapPointGeom*)dP,
                                                          (const int32_t*)dPo, (const PslBaEdge*)dE, (const int32_t*)dEo, cam, rounds,
                                                          (PslBaKeyFrame*)dK, (PslMapPointGeom*)dP, (uint8_t*)dX, (PslBaInfo*)dI);
            ctx.synchronize();
            std::vector<uint8_t> er(ed.size() ? ed.size() : 1, 0);
            std::vector<PslBaInfo> info(K);
            if (kb) pslfe::check(pslfe_device_download(ctx.get(), kf.data(), dK, kb), "download");
            if (pb) pslfe::check(pslfe_device_download(ctx.get(), mp.data(), dP, pb), "download");
            if (eb) pslfe::check(pslfe_device_download(ctx.get(), er.data(), dX, ed.size()), "download");
            pslfe::check(pslfe_device_download(ctx.get(), info.data(), dI, ib), "download");
            for (void* p : {dK, dP, dE, dKo, dPo, dEo, dX, dI}) pslfe_device_free(ctx.get(), p);
            for (int k = 0; k < K; ++k) {
                dev[k].info = info[k];
                dev[k].kf.assign(kf.begin() + koff[k], kf.begin() + koff[k + 1]);
                dev[k].mp.assign(mp.begin() + poff[k], mp.begin() + poff[k + 1]);
                dev[k].erase.assign(er.begin() + eoff[k], er.begin() + eoff[k + 1]);
                // problem by problem, as LocalMapping calls it
                host[k] = unchanged(cases[k], PSLFE_OK);
                try {
                    host[k].info = pslfe::Optimizer::LocalBundleAdjustment(ba, host[k].kf, host[k].mp, cases[k].ed, cam, host[k].erase, rounds == 2);
                } catch (const pslfe::Error& e) {
                    if (e.code != PSLFE_E_CAPACITY && e.code != PSLFE_E_INVALID) throw;
                    host[k] = unchanged(cases[k], e.code);
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
