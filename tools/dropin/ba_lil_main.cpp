// The sibling of ba_main.cpp for Optimizer::LocalBundleAdjustmentAndInseclines (the call LocalMapping::Run makes,
// src/LocalMapping.cc:84): a C++ consumer of pslfe::Optimizer::LocalBundleAdjustmentAndInseclines[Device] of
// psl-slam_amd/host/pslfe.hpp, and the plain one-core host loop of the same restatement.  Who owns what: all arithmetic and every
// decision are psl-slam_amd/csrc/ba_kernels.h, written over an executor; the loop here is psl_ba_rounds<true> on PslLmSerial, the
// kernel k_ba_local<true> the same text on a workgroup.  tests/test_local_ba_lil_gpu.py builds this program with g++ and compares all
// three forms with the restatement of tests/ba_lil_cases.py; built with -DPSL_BA_HOST_ONLY it needs neither the library nor a GPU
// (tests/test_local_ba_lil_cpu.py runs that build under the address and undefined-behaviour sanitizers; tools/bench_local_ba.py
// times it).  ba_main.cpp and its case files stay as they are.
//
// usage: ba_lil_main <cases.bin> <out.bin> [repeat]
//   cases.bin: int32 K, rounds, max_keyframes, max_points, max_edges, max_lils, max_lil_edges; PslCamera cam;
//              K x { int32 nkf, nmp, ne, nlil, nle; PslBaKeyFrame kf[nkf]; PslMapPointGeom mp[nmp]; PslBaEdge edges[ne];
//                    PslMapLil lil[nlil]; PslBaLilEdge lil_edges[nle] }
//   out.bin:   one section per form - "loop", then (library builds) "device" (the K problems in one launch) and "host" (problem by
//              problem) - each K x { PslBaInfo info; kf[nkf]; mp[nmp]; u8 erase[ne]; PslMapLil lil[nlil]; u8 erase_lil[nle];
//              int32 nerased_lil }
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
    std::vector<PslMapLil> lil;
    std::vector<PslBaLilEdge> led;
};
struct Result {
    PslBaInfo info;
    std::vector<PslBaKeyFrame> kf;
    std::vector<PslMapPointGeom> mp;
    std::vector<uint8_t> erase;
    std::vector<PslMapLil> lil;
    std::vector<uint8_t> eraseLil;
    int32_t nerasedLil = 0;
};
struct Caps { int kf, mp, ed, lil, led; };

Result unchanged(const Case& c, int status) {
    Result R;
    memset(&R.info, 0, sizeof(R.info));
    R.info.status = status;
    R.kf = c.kf; R.mp = c.mp; R.lil = c.lil;
    R.erase.assign(c.ed.size(), 0);
    R.eraseLil.assign(c.led.size(), 0);
    return R;
}

// one problem on one core: the checks of k_ba_check and k_ba_lists, then psl_ba_rounds with the LILs
Result hostLoop(const Case& c, const PslCamera& cam, int rounds, const Caps& cap) {
    const int nkf = (int)c.kf.size(), nmp = (int)c.mp.size(), ne = (int)c.ed.size(), nlil = (int)c.lil.size(), nle = (int)c.led.size();
    if (nkf > cap.kf || nmp > cap.mp || ne > cap.ed || nlil > cap.lil || nle > cap.led) return unchanged(c, PSLFE_E_CAPACITY);
    if (psl_ba_check_rows(c.ed.data(), nkf, nmp, ne) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    if (psl_ba_check_lil_rows(c.led.data(), nkf, nlil, nle) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    if (!psl_ba_has_work(c.kf.data(), nkf, ne + nle)) return unchanged(c, PSLFE_OK);
    PslBaWs W;
    std::vector<double> store(psl_ba_carve(nullptr, nkf, nmp, ne, &W, nlil, nle) / sizeof(double) + 1, 0.0);
    psl_ba_carve(reinterpret_cast<char*>(store.data()), nkf, nmp, ne, &W, nlil, nle);
    W.kf = c.kf.data(); W.mp = c.mp.data(); W.ed = c.ed.data(); W.lil = c.lil.data(); W.led = c.led.data();
    W.nkf = nkf; W.nmp = nmp; W.ne = ne; W.nlil = nlil; W.nle = nle;
    W.K.fx = cam.fx; W.K.fy = cam.fy; W.K.cx = cam.cx; W.K.cy = cam.cy; W.K.bf = cam.bf;
    W.sctab = kSinCosTab;
    if (psl_ba_lists_host(W) != PSLFE_OK || psl_ba_lil_lists_host(W) != PSLFE_OK) return unchanged(c, PSLFE_E_INVALID);
    Result R = unchanged(c, PSLFE_OK);
    PslLmSerial X = {W.scal + 8};
    psl_ba_rounds<true>(X, W, rounds, R.kf.data(), R.mp.data(), R.erase.data(), &R.info, R.lil.data(), R.eraseLil.data(), &R.nerasedLil);
    return R;
}

template <class T>
bool put(FILE* o, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), o) == v.size(); }
bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs)
        if (fwrite(&r.info, sizeof(PslBaInfo), 1, o) != 1 || !put(o, r.kf) || !put(o, r.mp) || !put(o, r.erase) || !put(o, r.lil) ||
            !put(o, r.eraseLil) || fwrite(&r.nerasedLil, 4, 1, o) != 1)
            return false;
    return true;
}
template <class T>
bool get(FILE* f, std::vector<T>& v, int n) { v.resize(n); return n == 0 || fread(v.data(), sizeof(T), n, f) == (size_t)n; }

#ifndef PSL_BA_HOST_ONLY
// a device copy of a host vector (one byte at least), freed by its owner
struct Dev {
    pslfe::Context& ctx;
    void* p = nullptr;
    size_t bytes;
    template <class T>
    Dev(pslfe::Context& c, const std::vector<T>& v) : ctx(c), bytes(v.size() * sizeof(T)) {
        pslfe::check(pslfe_device_alloc(ctx.get(), bytes ? bytes : 1, &p), "alloc");
        if (bytes) pslfe::check(pslfe_device_upload(ctx.get(), p, v.data(), bytes), "upload");
    }
    ~Dev() { pslfe_device_free(ctx.get(), p); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    template <class T>
    void down(std::vector<T>& v) { if (bytes) pslfe::check(pslfe_device_download(ctx.get(), v.data(), p, bytes), "download"); }
};
#endif

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin [repeat]\n", argv[0]); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[7];
    PslCamera cam;
    if (fread(hdr, 4, 7, f) != 7 || fread(&cam, sizeof(cam), 1, f) != 1 || hdr[0] < 0 || hdr[1] < 1 || hdr[1] > 2 || hdr[2] < 1 || hdr[3] < 1 || hdr[4] < 1 ||
        hdr[5] < 0 || hdr[6] < 0) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int K = hdr[0], rounds = hdr[1];
    const Caps cap = {hdr[2], hdr[3], hdr[4], hdr[5], hdr[6]};
    std::vector<Case> cases(K);
    for (Case& c : cases) {
        int32_t n[5] = {0, 0, 0, 0, 0};
        if (fread(n, 4, 5, f) != 5 || n[0] < 0 || n[1] < 0 || n[2] < 0 || n[3] < 0 || n[4] < 0 || n[0] > (1 << 20) || n[1] > (1 << 24) || n[2] > (1 << 26) ||
            n[3] > (1 << 24) || n[4] > (1 << 26)) {
            fprintf(stderr, "bad case\n");
            return 2;
        }
        if (!get(f, c.kf, n[0]) || !get(f, c.mp, n[1]) || !get(f, c.ed, n[2]) || !get(f, c.lil, n[3]) || !get(f, c.led, n[4])) {
            fprintf(stderr, "short case\n");
            return 2;
        }
    }
    fclose(f);

    std::vector<Result> loop(K);
    double best = -1.0;
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; ++k) loop[k] = hostLoop(cases[k], cam, rounds, cap);
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
            pslfe::BundleAdjuster ba(ctx, K, cap.kf, cap.mp, cap.ed, cap.lil, cap.led);
            // the K problems in one launch, HBM to HBM, in place
            Case all;
            std::vector<int32_t> koff(1, 0), poff(1, 0), eoff(1, 0), loff(1, 0), foff(1, 0);
            for (const Case& c : cases) {
                all.kf.insert(all.kf.end(), c.kf.begin(), c.kf.end());
                all.mp.insert(all.mp.end(), c.mp.begin(), c.mp.end());
                all.ed.insert(all.ed.end(), c.ed.begin(), c.ed.end());
                all.lil.insert(all.lil.end(), c.lil.begin(), c.lil.end());
                all.led.insert(all.led.end(), c.led.begin(), c.led.end());
                koff.push_back((int32_t)all.kf.size()); poff.push_back((int32_t)all.mp.size()); eoff.push_back((int32_t)all.ed.size());
                loff.push_back((int32_t)all.lil.size()); foff.push_back((int32_t)all.led.size());
            }
            std::vector<uint8_t> er(all.ed.size(), 0), erl(all.led.size(), 0);
            std::vector<PslBaInfo> info(K);
            std::vector<int32_t> nel(K, 0);
            {
                Dev dK(ctx, all.kf), dP(ctx, all.mp), dE(ctx, all.ed), dL(ctx, all.lil), dF(ctx, all.led);
                Dev dKo(ctx, koff), dPo(ctx, poff), dEo(ctx, eoff), dLo(ctx, loff), dFo(ctx, foff);
                Dev dX(ctx, er), dXl(ctx, erl), dI(ctx, info), dN(ctx, nel);
                pslfe::Optimizer::LocalBundleAdjustmentAndInseclinesDevice(
                    ba, K, (const PslBaKeyFrame*)dK.p, (const int32_t*)dKo.p, (const PslMapPointGeom*)dP.p, (const int32_t*)dPo.p,
                    (const PslBaEdge*)dE.p, (const int32_t*)dEo.p, (const PslMapLil*)dL.p, (const int32_t*)dLo.p, (const PslBaLilEdge*)dF.p,
                    (const int32_t*)dFo.p, cam, rounds, (PslBaKeyFrame*)dK.p, (PslMapPointGeom*)dP.p, (uint8_t*)dX.p, (PslMapLil*)dL.p,
                    (uint8_t*)dXl.p, (int32_t*)dN.p, (PslBaInfo*)dI.p);
                ctx.synchronize();
                dK.down(all.kf); dP.down(all.mp); dL.down(all.lil); dX.down(er); dXl.down(erl); dI.down(info); dN.down(nel);
            }
            for (int k = 0; k < K; ++k) {
                dev[k].info = info[k];
                dev[k].nerasedLil = nel[k];
                dev[k].kf.assign(all.kf.begin() + koff[k], all.kf.begin() + koff[k + 1]);
                dev[k].mp.assign(all.mp.begin() + poff[k], all.mp.begin() + poff[k + 1]);
                dev[k].erase.assign(er.begin() + eoff[k], er.begin() + eoff[k + 1]);
                dev[k].lil.assign(all.lil.begin() + loff[k], all.lil.begin() + loff[k + 1]);
                dev[k].eraseLil.assign(erl.begin() + foff[k], erl.begin() + foff[k + 1]);
                // problem by problem, as LocalMapping calls it
                host[k] = unchanged(cases[k], PSLFE_OK);
                try {
                    host[k].info = pslfe::Optimizer::LocalBundleAdjustmentAndInseclines(ba, host[k].kf, host[k].mp, cases[k].ed, host[k].lil, cases[k].led,
                                                                                        cam, host[k].erase, host[k].eraseLil, rounds == 2);
                    for (uint8_t b : host[k].eraseLil) host[k].nerasedLil += b;
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
