// A C++ consumer of the pose-optimisation seam of psl-slam_amd/host/pslfe.hpp (pslfe::Optimizer::PoseOptimization, the call of
// TrackReferenceKeyFrame src/Tracking.cc:968, TrackWithMotionModel :1214 and TrackLocalMap :1331; the point edges alone or with the
// LIL edges, PslPoseLilEdge rows), and the plain C++ host loop of the same restatement on one core.  Who owns what: the arithmetic
// and the four rounds are psl-slam_amd/csrc/pose_kernels.h, the Levenberg driver (iterations, trials and every decision between two
// sums) and the solve psl-slam_amd/csrc/lm_kernels.h; HostLoop below is their `Problem` for one core and owns only the order of
// the sums, which copies the one in the header of psl-slam_amd/csrc/pslfe_pose.hip (LIL edge j has the edge index n + j and adds
// its six rows one after the other).  The kernel shares the arithmetic and holds the driver's loop written out in its body.  tests/test_pose_opt_gpu.py and
// tests/test_pose_lil_gpu.py build this program with g++ and compare all three forms with the numpy restatement; built with
// -DPSL_POSE_HOST_ONLY it needs neither the library nor a GPU (tests/test_pose_opt_cpu.py and tests/test_pose_lil_cpu.py run that
// build under the address and undefined-behaviour sanitizers; tools/bench_pose_opt.py times it).
//
// usage: pose_main <cases.bin> <out.bin> [repeat]
//   cases.bin: int32 K, estride, lstride; PslCamera cam; K x { PslPose Tcw; int32 n, m; PslPoseEdge edges[n]; PslPoseLilEdge lil[m] }
//              (n <= estride, m <= lstride)
//   out.bin:   one section per form - "loop", then (library builds) "device" (the K frames in one launch) and "host" (frame by
//              frame through PoseOptimization) - each K x { PslPose Tcw; int32 ngood; int32 rounds, iterations[4]; u8 outlier[n];
//              u8 outlier_lil[m] }; the host form reports no rounds (zeros); below 3 edges in all the outlier bytes are 0
//   stdout:    {"frames": K, "loop_ms": the host loop over the K frames, best of `repeat`}
// In a library build a file with lstride == 0 goes through the point-edge entry points (PoseOptimizationDevice and the five-argument
// PoseOptimization, k_pose_optimize<false>), one with lstride > 0 through the LIL ones (PoseOptimizationLilDevice and the
// seven-argument PoseOptimization, k_pose_optimize<true>): both instantiations keep their compiled consumer.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#ifndef PSL_POSE_HOST_ONLY
#include "../../psl-slam_amd/host/pslfe.hpp"
#else
#include "../../include/pslfe.h"
#endif
#include "../../psl-slam_amd/csrc/pose_kernels.h"

namespace {

const double kSinCosTab[444] = {
#include "../../psl-slam_amd/csrc/psl_sincostab.inc"
};

struct Case {
    PslPose Tcw;
    std::vector<PslPoseEdge> edges;
    std::vector<PslPoseLilEdge> lil;
};
struct Result {
    PslPose Tcw;
    int32_t ngood = 0;
    PslPoseInfo info = {0, {0, 0, 0, 0}};
    std::vector<uint8_t> outlier, outlierLil;
};

// the `Problem` of psl_po_rounds and psl_lm_optimize<6> on one core
struct HostLoop : PslPoseVertex {
    const Case& c;
    PslPoseCamD K;
    const int n, m;
    std::vector<uint8_t> out, outLil;
    std::vector<double> part;   // [28][256]
    PslPoseInfo info = {0, {0, 0, 0, 0}};
    int round = 0;
    bool robust = true;

    HostLoop(const Case& cs, const PslCamera& cam)
        : c(cs), n((int)cs.edges.size()), m((int)cs.lil.size()), out(cs.edges.size(), 0), outLil(cs.lil.size(), 0),
          part((size_t)PSL_POSE_NTERMS * PSL_LM_LANES) {
        sctab = kSinCosTab;
        K.fx = cam.fx; K.fy = cam.fy; K.cx = cam.cx; K.cy = cam.cy; K.bf = cam.bf;
    }
    bool active(int i) const { return round == 0 || !(i < n ? out[i] : outLil[i - n]); }
    const float* row(int i) const { return &c.edges[i].u; }
    const double* lilRow(int j) const { return c.lil[j].line1; }

    // H, b, chi2 at T: step 1 of the order of the sums (the point edges, then LIL edge j at index n + j), then steps 2 and 3 per value
    void sums(double* acc) {
        std::fill(part.begin(), part.end(), 0.0);
        double a[PSL_POSE_NTERMS];
        for (int i = 0; i < n + m; ++i) {
            if (!active(i)) continue;
            const int p = i % PSL_LM_LANES;
            for (int k = 0; k < PSL_POSE_NTERMS; ++k) a[k] = part[(size_t)k * PSL_LM_LANES + p];
            if (i < n) {
                double e[3], Pc[3], rho0, rho1 = 1.0;
                const int mono = psl_po_error(row(i), &T, &K, e, Pc);
                const double is2 = (double)c.edges[i].inv_sigma2;
                const double chi2 = psl_po_chi2(e, is2, mono);
                rho0 = chi2;
                if (robust) psl_lm_huber(chi2, PSL_POSE_DELTA(mono), &rho0, &rho1);
                psl_po_add_terms(e, Pc, mono, is2, rho0, rho1, &K, a);
            } else {
                double e[6], rho0, rho1 = 1.0;
                psl_po_lil_error(lilRow(i - n), &T, &K, e);
                const double chi2 = psl_po_lil_chi2(e);
                rho0 = chi2;
                if (robust) psl_lm_huber(chi2, PSL_POSE_DELTA_LIL, &rho0, &rho1);
                psl_po_lil_add_terms(lilRow(i - n), e, &T, rho0, rho1, &K, a);
            }
            for (int k = 0; k < PSL_POSE_NTERMS; ++k) part[(size_t)k * PSL_LM_LANES + p] = a[k];
        }
        for (int k = 0; k < PSL_POSE_NTERMS; ++k) acc[k] = psl_lm_reduce_lanes(&part[(size_t)k * PSL_LM_LANES]);
    }
    double chi() {   // at the candidate
        const PslSE3& T = Tn;
        std::fill(part.begin(), part.begin() + PSL_LM_LANES, 0.0);
        for (int i = 0; i < n + m; ++i) {
            if (!active(i)) continue;
            double rho0, rho1 = 1.0;
            if (i < n) {
                double e[3], Pc[3];
                const int mono = psl_po_error(row(i), &T, &K, e, Pc);
                const double chi2 = psl_po_chi2(e, (double)c.edges[i].inv_sigma2, mono);
                rho0 = chi2;
                if (robust) psl_lm_huber(chi2, PSL_POSE_DELTA(mono), &rho0, &rho1);
            } else {
                double e[6];
                psl_po_lil_error(lilRow(i - n), &T, &K, e);
                const double chi2 = psl_po_lil_chi2(e);
                rho0 = chi2;
                if (robust) psl_lm_huber(chi2, PSL_POSE_DELTA_LIL, &rho0, &rho1);
            }
            part[i % PSL_LM_LANES] = part[i % PSL_LM_LANES] + rho0;
        }
        return psl_lm_reduce_lanes(part.data());
    }
    void classify(int* nbad, int* nbadLil) {
        *nbad = *nbadLil = 0;
        for (int i = 0; i < n; ++i) {
            double e[3], Pc[3];
            const int mono = psl_po_error(row(i), &T, &K, e, Pc);
            const float chi2 = (float)psl_po_chi2(e, (double)c.edges[i].inv_sigma2, mono);
            out[i] = chi2 > (mono ? 5.991f : 7.815f) ? 1 : 0;
            *nbad += out[i];
        }
        for (int j = 0; j < m; ++j) {
            double e[6];
            psl_po_lil_error(lilRow(j), &T, &K, e);
            outLil[j] = (float)psl_po_lil_chi2(e) > 11.07f ? 1 : 0;
            *nbadLil += outLil[j];
        }
    }
    void round_done(int r, int its) {
        info.rounds = r + 1;
        info.iterations[r] = its;
    }

    Result run() {
        Result R;
        R.Tcw = c.Tcw;
        R.outlier.assign(n, 0);
        R.outlierLil.assign(m, 0);
        if (n + m < 3) return R;
        PslSE3 T0, Tout;
        int nbad = 0;
        psl_po_from_pose(c.Tcw.R, c.Tcw.t, &T0);
        psl_po_rounds(*this, T0, n + m, &Tout, &nbad);
        psl_po_to_pose(&Tout, R.Tcw.R, R.Tcw.t);
        R.ngood = n + m - nbad;
        R.info = info;
        R.outlier = out;
        R.outlierLil = outLil;
        return R;
    }
};

bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs) {
        if (fwrite(&r.Tcw, sizeof(PslPose), 1, o) != 1 || fwrite(&r.ngood, 4, 1, o) != 1 || fwrite(&r.info, sizeof(PslPoseInfo), 1, o) != 1) return false;
        if (!r.outlier.empty() && fwrite(r.outlier.data(), 1, r.outlier.size(), o) != r.outlier.size()) return false;
        if (!r.outlierLil.empty() && fwrite(r.outlierLil.data(), 1, r.outlierLil.size(), o) != r.outlierLil.size()) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin [repeat]\n", argv[0]); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[3];
    PslCamera cam;
    if (fread(hdr, 4, 3, f) != 3 || fread(&cam, sizeof(cam), 1, f) != 1 || hdr[0] < 0 || hdr[1] < 0 || hdr[2] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int K = hdr[0], estride = hdr[1], lstride = hdr[2];
    std::vector<Case> cases(K);
    for (Case& c : cases) {
        int32_t nm[2] = {0, 0};
        if (fread(&c.Tcw, sizeof(PslPose), 1, f) != 1 || fread(nm, 4, 2, f) != 2 || nm[0] < 0 || nm[0] > estride || nm[1] < 0 || nm[1] > lstride) {
            fprintf(stderr, "bad case\n");
            return 2;
        }
        c.edges.resize(nm[0]);
        c.lil.resize(nm[1]);
        if (nm[0] && fread(c.edges.data(), sizeof(PslPoseEdge), nm[0], f) != (size_t)nm[0]) { fprintf(stderr, "short case\n"); return 2; }
        if (nm[1] && fread(c.lil.data(), sizeof(PslPoseLilEdge), nm[1], f) != (size_t)nm[1]) { fprintf(stderr, "short case\n"); return 2; }
    }
    fclose(f);

    std::vector<Result> loop(K);
    double best = -1.0;
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; ++k) loop[k] = HostLoop(cases[k], cam).run();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (best < 0 || ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !writeSection(o, loop)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
#ifndef PSL_POSE_HOST_ONLY
    try {
        pslfe::Context ctx(0);
        // the K frames in one launch, HBM to HBM
        std::vector<PslPose> Tin(K);
        std::vector<PslPoseEdge> edges((size_t)K * estride);
        std::vector<PslPoseLilEdge> lil((size_t)K * lstride);
        std::vector<int32_t> nedges(K), nlil(K);
        for (int k = 0; k < K; ++k) {
            Tin[k] = cases[k].Tcw;
            nedges[k] = (int32_t)cases[k].edges.size();
            nlil[k] = (int32_t)cases[k].lil.size();
            if (nedges[k]) memcpy(&edges[(size_t)k * estride], cases[k].edges.data(), cases[k].edges.size() * sizeof(PslPoseEdge));
            if (nlil[k]) memcpy(&lil[(size_t)k * lstride], cases[k].lil.data(), cases[k].lil.size() * sizeof(PslPoseLilEdge));
        }
        std::vector<Result> dev(K), host(K);
        if (K) {
            void *dT = nullptr, *dE = nullptr, *dL = nullptr, *dN = nullptr, *dM = nullptr, *dO = nullptr, *dOL = nullptr, *dG = nullptr, *dI = nullptr;
            const size_t eb = edges.size() * sizeof(PslPoseEdge), lb = lil.size() * sizeof(PslPoseLilEdge);
            const size_t ob = (size_t)K * estride, olb = (size_t)K * lstride;
            pslfe::check(pslfe_device_alloc(ctx.get(), K * sizeof(PslPose), &dT), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), eb ? eb : 1, &dE), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), lb ? lb : 8, &dL), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), K * 4, &dN), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), K * 4, &dM), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), ob ? ob : 1, &dO), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), olb ? olb : 1, &dOL), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), K * 4, &dG), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), K * sizeof(PslPoseInfo), &dI), "alloc");
            std::vector<uint8_t> zeros(std::max(std::max(ob, olb), (size_t)1), 0), outl(ob ? ob : 1, 0), outll(olb ? olb : 1, 0);
            pslfe::check(pslfe_device_upload(ctx.get(), dT, Tin.data(), K * sizeof(PslPose)), "upload");
            if (eb) pslfe::check(pslfe_device_upload(ctx.get(), dE, edges.data(), eb), "upload");
            if (lb) pslfe::check(pslfe_device_upload(ctx.get(), dL, lil.data(), lb), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dN, nedges.data(), K * 4), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dM, nlil.data(), K * 4), "upload");
            if (ob) pslfe::check(pslfe_device_upload(ctx.get(), dO, zeros.data(), ob), "upload");
            if (olb) pslfe::check(pslfe_device_upload(ctx.get(), dOL, zeros.data(), olb), "upload");
            if (lstride)
                pslfe::Optimizer::PoseOptimizationLilDevice(ctx, K, (const PslPose*)dT, (const PslPoseEdge*)dE, (const int32_t*)dN, estride,
                                                            (const PslPoseLilEdge*)dL, (const int32_t*)dM, lstride, cam, (PslPose*)dT, (uint8_t*)dO,
                                                            (uint8_t*)dOL, (int32_t*)dG, (PslPoseInfo*)dI);
            else
                pslfe::Optimizer::PoseOptimizationDevice(ctx, K, (const PslPose*)dT, (const PslPoseEdge*)dE, (const int32_t*)dN, estride, cam,
                                                         (PslPose*)dT, (uint8_t*)dO, (int32_t*)dG, (PslPoseInfo*)dI);
            ctx.synchronize();
            std::vector<PslPose> Tout(K);
            std::vector<int32_t> ng(K);
            std::vector<PslPoseInfo> info(K);
            pslfe::check(pslfe_device_download(ctx.get(), Tout.data(), dT, K * sizeof(PslPose)), "download");
            pslfe::check(pslfe_device_download(ctx.get(), ng.data(), dG, K * 4), "download");
            pslfe::check(pslfe_device_download(ctx.get(), info.data(), dI, K * sizeof(PslPoseInfo)), "download");
            if (ob) pslfe::check(pslfe_device_download(ctx.get(), outl.data(), dO, ob), "download");
            if (olb) pslfe::check(pslfe_device_download(ctx.get(), outll.data(), dOL, olb), "download");
            for (void* p : {dT, dE, dL, dN, dM, dO, dOL, dG, dI}) pslfe_device_free(ctx.get(), p);
            for (int k = 0; k < K; ++k) {
                dev[k].Tcw = Tout[k]; dev[k].ngood = ng[k]; dev[k].info = info[k];
                dev[k].outlier.assign(outl.begin() + (size_t)k * estride, outl.begin() + (size_t)k * estride + nedges[k]);
                dev[k].outlierLil.assign(outll.begin() + (size_t)k * lstride, outll.begin() + (size_t)k * lstride + nlil[k]);
                // frame by frame, as Tracking calls it
                host[k].Tcw = cases[k].Tcw;
                host[k].ngood = lstride ? pslfe::Optimizer::PoseOptimization(ctx, host[k].Tcw, cases[k].edges, cases[k].lil, cam, host[k].outlier, host[k].outlierLil)
                                        : pslfe::Optimizer::PoseOptimization(ctx, host[k].Tcw, cases[k].edges, cam, host[k].outlier);
            }
        }
        if (!writeSection(o, dev) || !writeSection(o, host)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
#endif
    if (fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    printf("{\"frames\": %d, \"loop_ms\": %.6f}\n", K, best);
    return 0;
}
