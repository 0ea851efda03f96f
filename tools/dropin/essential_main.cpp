// A C++ consumer of the essential-graph seam of psl-slam_amd/host/pslfe.hpp (pslfe::Optimizer::OptimizeEssentialGraph, the call of
// LoopClosing::CorrectLoop), and the plain one-core host loop of the same restatement.  Who owns what: all arithmetic and every
// decision are psl-slam_amd/csrc/essential_kernels.h, written over an executor; the loop here is that text on PslLmSerial, the kernel
// k_eg_optimize the same text on a workgroup.  tests/test_essential_graph_gpu.py builds this program with g++ and compares all
// three forms with the Python restatement of tests/essential_cases.py; built with -DPSL_EG_HOST_ONLY it needs neither the library nor
// a GPU (tests/test_essential_graph_cpu.py runs that build under the address and undefined-behaviour sanitizers;
// tools/bench_essential_graph.py times it).
//
// usage: essential_main <cases.bin> <out.bin> [repeat]
//   cases.bin: int32 K, fix_scale, max_keyframes, max_edges, max_points, 0; int64 max_envelope;
//              K x { int32 nkf, ne, nmp; PslEgKeyFrame kf[nkf]; PslEgEdge edges[ne]; PslMapPointGeom mp[nmp]; int32 mp_ref[nmp] }
//   out.bin:   one section per form - "loop", then (library builds) "device" (the K graphs in one launch) and "host" (graph by graph
//              through OptimizeEssentialGraph) - each K x { PslEgInfo info; PslPose pose[nkf]; double S[nkf][8]; PslMapPointGeom mp[nmp] };
//              a refused graph has zero pose rows, S = its Scw and mp = its input
//   stdout:    {"graphs": K, "loop_ms": the host loop over the K graphs, best of `repeat`}
// usage: essential_main --math <in.bin> <out.bin>: the header's psl_acos and psl_s3_log on the host, for the CPU suite
//   in.bin:  int32 nacos, nlog; double x[nacos]; double S[nlog][8] (q x y z w, t, s)
//   out.bin: double acos[nacos]; nlog x { double log[7]; double branch }
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#ifndef PSL_EG_HOST_ONLY
#include "../../psl-slam_amd/host/pslfe.hpp"
#else
#include "../../include/pslfe.h"
#endif
#include "../../psl-slam_amd/csrc/essential_kernels.h"

namespace {

const double kSinCosTab[444] = {
#include "../../psl-slam_amd/csrc/psl_sincostab.inc"
};

struct Case {
    std::vector<PslEgKeyFrame> kf;
    std::vector<PslEgEdge> ed;
    std::vector<PslMapPointGeom> mp;
    std::vector<int32_t> ref;
};
struct Result {
    PslEgInfo info;
    std::vector<PslPose> pose;
    std::vector<double> S;
    std::vector<PslMapPointGeom> mp;
};

Result blank(const Case& c) {
    Result R;
    memset(&R.info, 0, sizeof(R.info));
    R.pose.resize(c.kf.size());
    if (!c.kf.empty()) memset(R.pose.data(), 0, c.kf.size() * sizeof(PslPose));
    R.S.assign(8 * c.kf.size(), 0.0);
    R.mp = c.mp;
    return R;
}

// one graph on one core: the counts against the caps as k_eg_optimize checks them, then psl_eg_run
Result hostLoop(const Case& c, int fix_scale, int ckf, int ced, int cmp, size_t cenv) {
    const int nkf = (int)c.kf.size(), ne = (int)c.ed.size(), nmp = (int)c.mp.size();
    Result R = blank(c);
    const int code = (nkf > ckf || ne > ced || nmp > cmp) ? PSLFE_E_CAPACITY : PSLFE_OK;
    // the workspace has the size of the graph, not of the caps (a refused graph touches none of it); the full lower triangle bounds
    // every envelope, and the cap of the handle stays what refuses one
    PslEgWs W;
    const size_t tri = 7 * (size_t)nkf * (7 * (size_t)nkf + 1) / 2;
    const size_t env = code != PSLFE_OK ? 1 : (tri < cenv ? (tri ? tri : 1) : cenv);
    const int wk = code == PSLFE_OK && nkf ? nkf : 1, we = code == PSLFE_OK && ne ? ne : 1;
    std::vector<double> store(psl_eg_carve(nullptr, wk, we, env, &W) / sizeof(double) + 1, 0.0);
    psl_eg_carve(reinterpret_cast<char*>(store.data()), wk, we, env, &W);
    W.kf = c.kf.data(); W.ed = c.ed.data(); W.mp = c.mp.data(); W.mp_ref = c.ref.data();
    W.nkf = nkf; W.ne = ne; W.nmp = nmp;
    W.fix_scale = fix_scale;
    W.sctab = kSinCosTab;
    PslLmSerial X = {W.scal + 8};
    psl_eg_run(X, W, 1, code, cenv, R.pose.data(), R.S.data(), R.mp.data(), &R.info);
    return R;
}

bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs) {
        if (fwrite(&r.info, sizeof(PslEgInfo), 1, o) != 1) return false;
        if (!r.pose.empty() && fwrite(r.pose.data(), sizeof(PslPose), r.pose.size(), o) != r.pose.size()) return false;
        if (!r.S.empty() && fwrite(r.S.data(), sizeof(double), r.S.size(), o) != r.S.size()) return false;
        if (!r.mp.empty() && fwrite(r.mp.data(), sizeof(PslMapPointGeom), r.mp.size(), o) != r.mp.size()) return false;
    }
    return true;
}

int mathMode(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    int32_t n[2] = {0, 0};
    if (!f || fread(n, 4, 2, f) != 2 || n[0] < 0 || n[1] < 0 || n[0] > (1 << 26) || n[1] > (1 << 24)) { fprintf(stderr, "bad math input\n"); return 2; }
    std::vector<double> x(n[0]), S(8 * (size_t)n[1]), o;
    if ((n[0] && fread(x.data(), 8, x.size(), f) != x.size()) || (n[1] && fread(S.data(), 8, S.size(), f) != S.size())) { fprintf(stderr, "short math input\n"); return 2; }
    fclose(f);
    for (double v : x) o.push_back(psl_acos(v));
    for (int k = 0; k < n[1]; ++k) {
        PslS3 T;
        psl_eg_load(&S[8 * (size_t)k], &T);
        double e[7];
        int br = 0;
        psl_s3_log(&T, kSinCosTab, e, &br);
        o.insert(o.end(), e, e + 7);
        o.push_back((double)br);
    }
    FILE* w = fopen(out, "wb");
    if (!w || (!o.empty() && fwrite(o.data(), 8, o.size(), w) != o.size()) || fclose(w) != 0) { fprintf(stderr, "cannot write %s\n", out); return 2; }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "--math")) return mathMode(argv[2], argv[3]);
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin [repeat]\n", argv[0]); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[6];
    int64_t cenv64 = 0;
    if (fread(hdr, 4, 6, f) != 6 || fread(&cenv64, 8, 1, f) != 1 || hdr[0] < 0 || hdr[2] < 1 || hdr[3] < 1 || hdr[4] < 1 || cenv64 < 1) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int K = hdr[0], fix_scale = hdr[1] ? 1 : 0, ckf = hdr[2], ced = hdr[3], cmp = hdr[4];
    const size_t cenv = (size_t)cenv64;
    std::vector<Case> cases(K);
    for (Case& c : cases) {
        int32_t n[3] = {0, 0, 0};
        if (fread(n, 4, 3, f) != 3 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[0] > (1 << 20) || n[1] > (1 << 24) || n[2] > (1 << 26)) { fprintf(stderr, "bad case\n"); return 2; }
        c.kf.resize(n[0]); c.ed.resize(n[1]); c.mp.resize(n[2]); c.ref.resize(n[2]);
        if ((n[0] && fread(c.kf.data(), sizeof(PslEgKeyFrame), n[0], f) != (size_t)n[0]) || (n[1] && fread(c.ed.data(), sizeof(PslEgEdge), n[1], f) != (size_t)n[1]) ||
            (n[2] && fread(c.mp.data(), sizeof(PslMapPointGeom), n[2], f) != (size_t)n[2]) || (n[2] && fread(c.ref.data(), 4, n[2], f) != (size_t)n[2])) {
            fprintf(stderr, "short case\n");
            return 2;
        }
    }
    fclose(f);

    std::vector<Result> loop(K);
    double best = -1.0;
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; ++k) loop[k] = hostLoop(cases[k], fix_scale, ckf, ced, cmp, cenv);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (best < 0 || ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !writeSection(o, loop)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
#ifndef PSL_EG_HOST_ONLY
    try {
        pslfe::Context ctx(0);
        std::vector<Result> dev(K), host(K);
        if (K) {
            pslfe::EssentialGraph eg(ctx, K, ckf, ced, cmp, (int64_t)cenv);
            // the K graphs in one launch, HBM to HBM
            std::vector<PslEgKeyFrame> kf;
            std::vector<PslEgEdge> ed;
            std::vector<PslMapPointGeom> mp;
            std::vector<int32_t> ref, koff(1, 0), eoff(1, 0), poff(1, 0);
            for (const Case& c : cases) {
                kf.insert(kf.end(), c.kf.begin(), c.kf.end());
                ed.insert(ed.end(), c.ed.begin(), c.ed.end());
                mp.insert(mp.end(), c.mp.begin(), c.mp.end());
                ref.insert(ref.end(), c.ref.begin(), c.ref.end());
                koff.push_back((int32_t)kf.size()); eoff.push_back((int32_t)ed.size()); poff.push_back((int32_t)mp.size());
            }
            const size_t nk = kf.size() ? kf.size() : 1, nn = ed.size() ? ed.size() : 1, np = mp.size() ? mp.size() : 1;
            const size_t ob = (size_t)(K + 1) * 4, ib = (size_t)K * sizeof(PslEgInfo);
            std::vector<PslPose> pose(nk);
            memset(pose.data(), 0, nk * sizeof(PslPose));
            std::vector<double> S(8 * nk, 0.0);
            void *dK = nullptr, *dE = nullptr, *dP = nullptr, *dR = nullptr, *dKo = nullptr, *dEo = nullptr, *dPo = nullptr, *dT = nullptr, *dS = nullptr,
                 *dI = nullptr;
            pslfe::check(pslfe_device_alloc(ctx.get(), nk * sizeof(PslEgKeyFrame), &dK), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), nn * sizeof(PslEgEdge), &dE), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), np * sizeof(PslMapPointGeom), &dP), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), np * 4, &dR), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob, &dKo), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob, &dEo), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob, &dPo), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), nk * sizeof(PslPose), &dT), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), 8 * nk * sizeof(double), &dS), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ib, &dI), "alloc");
            if (!kf.empty()) pslfe::check(pslfe_device_upload(ctx.get(), dK, kf.data(), kf.size() * sizeof(PslEgKeyFrame)), "upload");
            if (!ed.empty()) pslfe::check(pslfe_device_upload(ctx.get(), dE, ed.data(), ed.size() * sizeof(PslEgEdge)), "upload");
            if (!mp.empty()) pslfe::check(pslfe_device_upload(ctx.get(), dP, mp.data(), mp.size() * sizeof(PslMapPointGeom)), "upload");
            if (!ref.empty()) pslfe::check(pslfe_device_upload(ctx.get(), dR, ref.data(), ref.size() * 4), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dKo, koff.data(), ob), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dEo, eoff.data(), ob), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dPo, poff.data(), ob), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dT, pose.data(), nk * sizeof(PslPose)), "upload");   // a refused graph writes no pose row
            pslfe::Optimizer::OptimizeEssentialGraphDevice(eg, K, (const PslEgKeyFrame*)dK, (const int32_t*)dKo, (const PslEgEdge*)dE,
                                                           (const int32_t*)dEo, (const PslMapPointGeom*)dP, (const int32_t*)dR, (const int32_t*)dPo,
                                                           fix_scale != 0, (PslPose*)dT, (double*)dS, (PslMapPointGeom*)dP, (PslEgInfo*)dI);
            ctx.synchronize();
            std::vector<PslEgInfo> info(K);
            pslfe::check(pslfe_device_download(ctx.get(), pose.data(), dT, nk * sizeof(PslPose)), "download");
            pslfe::check(pslfe_device_download(ctx.get(), S.data(), dS, 8 * nk * sizeof(double)), "download");
            if (!mp.empty()) pslfe::check(pslfe_device_download(ctx.get(), mp.data(), dP, mp.size() * sizeof(PslMapPointGeom)), "download");
            pslfe::check(pslfe_device_download(ctx.get(), info.data(), dI, ib), "download");
            for (void* p : {dK, dE, dP, dR, dKo, dEo, dPo, dT, dS, dI}) pslfe_device_free(ctx.get(), p);
            for (int k = 0; k < K; ++k) {
                dev[k].info = info[k];
                dev[k].pose.assign(pose.begin() + koff[k], pose.begin() + koff[k + 1]);
                dev[k].S.assign(S.begin() + 8 * (size_t)koff[k], S.begin() + 8 * (size_t)koff[k + 1]);
                dev[k].mp.assign(mp.begin() + poff[k], mp.begin() + poff[k + 1]);
                // graph by graph, as CorrectLoop calls it
                host[k] = blank(cases[k]);
                try {
                    host[k].info = pslfe::Optimizer::OptimizeEssentialGraph(eg, cases[k].kf, cases[k].ed, host[k].mp, cases[k].ref, fix_scale != 0,
                                                                            host[k].pose, host[k].S);
                } catch (const pslfe::Error& e) {
                    if (e.code != PSLFE_E_CAPACITY && e.code != PSLFE_E_INVALID) throw;
                    host[k] = blank(cases[k]);
                    host[k].info.status = e.code;
                    for (size_t v = 0; v < cases[k].kf.size(); ++v) memcpy(&host[k].S[8 * v], cases[k].kf[v].Scw, 64);
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
    printf("{\"graphs\": %d, \"loop_ms\": %.6f}\n", K, best);
    return 0;
}
