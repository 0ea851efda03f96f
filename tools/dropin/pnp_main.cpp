// A C++ consumer of the PnPsolver seam of psl-slam_amd/host/pslfe.hpp (pslfe::PnPsolver, the EPnP RANSAC of Tracking::Relocalization
// src/Tracking.cc:2075-2101), and the plain C++ loop of the same restatement on one core.  Who owns what: the arithmetic, the draw and
// the reference's loop psl_pnp_iterate are psl-slam_amd/csrc/pnp_solver_kernels.h; the kernel shares the arithmetic and runs the loop
// in blocks (the header of psl-slam_amd/csrc/pslfe_pnp.hip).  Every form plays a candidate as Relocalization does: calls of
// iterate(n_iterations) on one solver, each resumed from the state of the one before.  A returned pose that came without bNoMore is
// "rejected by the pose optimisation" `reject` times, and the solver goes on; the play ends at bNoMore or at the first pose after the
// rejections.  tests/test_pnp_solver_gpu.py builds this program with g++ and compares all three forms with the numpy restatement
// (tests/pnp_cases.py); built with -DPSL_PNP_HOST_ONLY it needs neither the library nor a GPU (tests/test_pnp_solver_cpu.py runs that
// build under the address and undefined-behaviour sanitizers; tools/bench_pnp_solver.py times it).
//
// usage: pnp_main <cases.bin> <out.bin> [repeat]
//        pnp_main --draw <N> <seed> <iterations> <out.bin>     the draws of psl_rs_draw<4> on one stream, int32 [iterations][4]
//   cases.bin: int32 K, rstride, min_set; double prob; float th2; PslCamera cam;
//              K x { uint32 seed; int32 n, min_inliers, max_its, n_iterations, reject; float epsilon; PslPnpRow rows[n] }   (n <= rstride)
//   out.bin:   one section per form - "loop", then (library builds) "device" (pslfe::PnPsolver::SolveDevice, one launch per candidate
//              and call) and "host" (pslfe::PnPsolver::iterate) - each K x { int32 ncalls; ncalls x { PslPnpResult; u8 flags[n] by
//              row }; u8 best_flags[n] after the last call }; then (library builds) "candidates": pslfe::PnPsolver::RelocalizeCandidates
//              on the K cases as the candidates of one frame with the parameters of case 0, candidate c seeded cases[0].seed + c, the
//              first `reject` poses handed over refused and the next accepted: int32 matched, count; count x { int32 round, candidate;
//              PslPnpResult; u8 flags[n of that candidate] } in the order they were handed over
//   stdout:    {"candidates": K, "loop_ms": the host loop over the K candidates, best of `repeat`}
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#ifndef PSL_PNP_HOST_ONLY
#include "../../psl-slam_amd/host/pslfe.hpp"
#else
#include "../../include/pslfe.h"
#endif
#include "../../psl-slam_amd/csrc/pnp_solver_kernels.h"

namespace {

struct Params {
    int minInliers, maxIts, minSet, nIterations, reject;
    double prob;
    float epsilon, th2;
    PslCamera cam;
};
struct Case {
    uint32_t seed = 0;
    Params P;
    std::vector<PslPnpRow> rows;
};
struct Call {
    PslPnpResult res;
    std::vector<uint8_t> flags;
};
struct Result {
    std::vector<Call> calls;
    std::vector<uint8_t> bestFlags;
};

// true when the play of a candidate goes on after this call
bool goesOn(const PslPnpResult& r, const Params& P, int* rejected, size_t ncalls) {
    if (r.status < 0 || (r.status & 2) || ncalls >= 100000) return false;
    if (P.nIterations <= 0 && !(r.status & 1)) return false;   // a call without iterations changes nothing
    if (r.status & 1) {
        if (*rejected >= P.reject) return false;
        ++*rejected;
    }
    return true;
}

// the candidate on one core: the calls of psl_pnp_iterate on one solver
Result hostLoop(const Case& c) {
    const Params& P = c.P;
    const int n = (int)c.rows.size();
    const PslPnpCam K = {(double)P.cam.fx, (double)P.cam.fy, (double)P.cam.cx, (double)P.cam.cy};
    int minIn = 0;
    const int maxIts = psl_pnp_max_iterations(P.prob, P.minInliers, P.maxIts, P.minSet, P.epsilon, n, &minIn);
    std::vector<double> ws(PSL_PNP_WS, 0.0);
    std::vector<uint8_t> flags((size_t)n + 1, 0);
    Result R;
    R.bestFlags.assign((size_t)n + 1, 0);
    PslPnpOutcome o = {0, 0, 0, 0};
    float bestT[12] = {0}, T[12];
    int rejected = 0;
    for (;;) {
        o = psl_pnp_iterate(n ? &c.rows[0].u : nullptr, n, &K, P.th2, maxIts, minIn, c.seed, o.iterations, o.best, bestT, R.bestFlags.data(),
                            P.nIterations, ws.data(), T, flags.data());
        Call call;
        memset(&call.res, 0, sizeof(call.res));
        call.res.status = o.status; call.res.iterations = o.iterations; call.res.inliers = o.ninliers; call.res.best_inliers = o.best;
        call.res.min_inliers = minIn;
        memcpy(call.res.Tcw.R, T, 9 * sizeof(float)); memcpy(call.res.Tcw.t, T + 9, 3 * sizeof(float));
        memcpy(call.res.best_Tcw.R, bestT, 9 * sizeof(float)); memcpy(call.res.best_Tcw.t, bestT + 9, 3 * sizeof(float));
        call.flags.assign(flags.begin(), flags.begin() + n);
        R.calls.push_back(call);
        if (!goesOn(call.res, P, &rejected, R.calls.size())) break;
    }
    R.bestFlags.resize((size_t)n);
    return R;
}

bool writeSection(FILE* o, const std::vector<Result>& rs) {
    for (const Result& r : rs) {
        const int32_t nc = (int32_t)r.calls.size();
        if (fwrite(&nc, 4, 1, o) != 1) return false;
        for (const Call& c : r.calls) {
            if (fwrite(&c.res, sizeof(PslPnpResult), 1, o) != 1) return false;
            if (!c.flags.empty() && fwrite(c.flags.data(), 1, c.flags.size(), o) != c.flags.size()) return false;
        }
        if (!r.bestFlags.empty() && fwrite(r.bestFlags.data(), 1, r.bestFlags.size(), o) != r.bestFlags.size()) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 6 && !strcmp(argv[1], "--draw")) {   // --draw N seed iterations out.bin: int32 [iterations][4], psl_rs_draw<4> on one stream
        const int N = atoi(argv[2]), its = atoi(argv[4]);
        if (N < 4 || its < 0) { fprintf(stderr, "bad --draw arguments\n"); return 2; }
        PslRsRand G;
        psl_rs_srand(&G, (uint32_t)strtoul(argv[3], nullptr, 10));
        std::vector<int32_t> out((size_t)its * 4 + 1);
        for (int i = 0; i < its; ++i) {
            int idx[4];
            psl_rs_draw<4>(&G, N, idx);
            for (int k = 0; k < 4; ++k) out[(size_t)i * 4 + k] = idx[k];
        }
        FILE* o = fopen(argv[5], "wb");
        if (!o || fwrite(out.data(), 4, (size_t)its * 4, o) != (size_t)its * 4 || fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
        return 0;
    }
    if (argc < 3) { fprintf(stderr, "usage: %s cases.bin out.bin [repeat]\n", argv[0]); return 2; }
    const int repeat = argc > 3 ? atoi(argv[3]) : 1;
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[3];
    Params G;
    if (fread(hdr, 4, 3, f) != 3 || fread(&G.prob, 8, 1, f) != 1 || fread(&G.th2, 4, 1, f) != 1 || fread(&G.cam, sizeof(G.cam), 1, f) != 1 ||
        hdr[0] < 0 || hdr[1] < 0 || hdr[2] != PSL_PNP_MIN_SET) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    const int K = hdr[0], rstride = hdr[1];
    G.minSet = hdr[2];
    std::vector<Case> cases(K);
    for (Case& c : cases) {
        int32_t h[5];
        c.P = G;
        if (fread(&c.seed, 4, 1, f) != 1 || fread(h, 4, 5, f) != 5 || fread(&c.P.epsilon, 4, 1, f) != 1 || h[0] < 0 || h[0] > rstride || h[1] < 0 ||
            h[2] < 1 || h[3] < 0 || h[4] < 0) {
            fprintf(stderr, "bad case\n");
            return 2;
        }
        const int32_t n = h[0];
        c.P.minInliers = h[1]; c.P.maxIts = h[2]; c.P.nIterations = h[3]; c.P.reject = h[4];
        c.rows.resize(n);
        if (n && fread(c.rows.data(), sizeof(PslPnpRow), n, f) != (size_t)n) { fprintf(stderr, "short case\n"); return 2; }
    }
    fclose(f);

    std::vector<Result> loop(K);
    double best = -1.0;
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int k = 0; k < K; ++k) loop[k] = hostLoop(cases[k]);
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (best < 0 || ms < best) best = ms;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o || !writeSection(o, loop)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
#ifndef PSL_PNP_HOST_ONLY
    try {
        pslfe::Context ctx(0);
        std::vector<Result> dev(K), host(K);
        for (int k = 0; k < K; ++k) {
            const Case& c = cases[k];
            const Params& P = c.P;
            const int n = (int)c.rows.size();
            // the device form: the candidate's arrays in HBM, one launch per call, the state kept in HBM (d_res is the next d_state_in)
            void *dP = nullptr, *dN = nullptr, *dR = nullptr, *dB = nullptr, *dF = nullptr;
            const size_t pb = (size_t)n * sizeof(PslPnpRow);
            pslfe::check(pslfe_device_alloc(ctx.get(), pb ? pb : 1, &dP), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), 4, &dN), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), sizeof(PslPnpResult), &dR), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), n ? (size_t)n : 1, &dB), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), n ? (size_t)n : 1, &dF), "alloc");
            const int32_t n32 = n;
            PslPnpResult r;
            memset(&r, 0, sizeof(r));
            std::vector<uint8_t> zeros((size_t)n + 1, 0);
            if (n) pslfe::check(pslfe_device_upload(ctx.get(), dP, c.rows.data(), pb), "upload");
            if (n) pslfe::check(pslfe_device_upload(ctx.get(), dB, zeros.data(), (size_t)n), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dN, &n32, 4), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dR, &r, sizeof(r)), "upload");
            int rejected = 0;
            for (;;) {
                pslfe::PnPsolver::SolveDevice(ctx, 1, (const PslPnpRow*)dP, (const int32_t*)dN, n, P.cam, P.prob, P.minInliers, P.maxIts, P.minSet,
                                              P.epsilon, P.th2, c.seed, (const PslPnpResult*)dR, (uint8_t*)dB, P.nIterations, (PslPnpResult*)dR,
                                              (uint8_t*)dF);
                ctx.synchronize();
                Call call;
                pslfe::check(pslfe_device_download(ctx.get(), &call.res, dR, sizeof(r)), "download");
                call.flags.assign((size_t)n, 0);
                if (n) pslfe::check(pslfe_device_download(ctx.get(), call.flags.data(), dF, (size_t)n), "download");
                dev[k].calls.push_back(call);
                if (!goesOn(call.res, P, &rejected, dev[k].calls.size())) break;
            }
            dev[k].bestFlags.assign((size_t)n, 0);
            if (n) pslfe::check(pslfe_device_download(ctx.get(), dev[k].bestFlags.data(), dB, (size_t)n), "download");
            for (void* p : {dP, dN, dR, dB, dF}) pslfe_device_free(ctx.get(), p);
            // the host form: the mirror of the reference's class, as Relocalization calls it
            std::vector<int32_t> ind((size_t)n);
            for (int i = 0; i < n; ++i) ind[i] = i;
            pslfe::PnPsolver solver(ctx, c.rows, ind, n, P.cam, c.seed);
            solver.SetRansacParameters(P.prob, P.minInliers, P.maxIts, P.minSet, P.epsilon, P.th2);
            rejected = 0;
            for (;;) {
                bool noMore = false;
                std::vector<bool> inl;
                int nInl = 0;
                const bool got = solver.iterate(P.nIterations, noMore, inl, nInl);
                Call call;
                call.res = solver.result();
                call.flags.assign((size_t)n, 0);
                for (int i = 0; i < n && got; ++i) call.flags[i] = inl[i] ? 1 : 0;
                host[k].calls.push_back(call);
                if (!goesOn(call.res, P, &rejected, host[k].calls.size())) break;
            }
            host[k].bestFlags.assign((size_t)n, 0);   // the mirror keeps mvbBestInliers to itself: written as zeros
        }
        if (!writeSection(o, dev) || !writeSection(o, host)) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        // the candidate loop of Tracking.cc:2088-2180: the K cases as the candidates of one frame, candidate c seeded cases[0].seed + c
        struct Handed { int32_t round, cand; PslPnpResult res; std::vector<uint8_t> flags; };
        std::vector<Handed> handed;
        int32_t matched = -1;
        if (K) {
            const Params& P = cases[0].P;
            const int ps = rstride ? rstride : 1;
            std::vector<PslPnpRow> rows((size_t)K * ps);
            std::vector<int32_t> np(K);
            for (int k = 0; k < K; ++k) {
                np[k] = (int32_t)cases[k].rows.size();
                if (np[k]) memcpy(&rows[(size_t)k * ps], cases[k].rows.data(), cases[k].rows.size() * sizeof(PslPnpRow));
            }
            void *dP = nullptr, *dN = nullptr;
            pslfe::check(pslfe_device_alloc(ctx.get(), rows.size() * sizeof(PslPnpRow), &dP), "alloc");
            pslfe::check(pslfe_device_alloc(ctx.get(), (size_t)K * 4, &dN), "alloc");
            pslfe::check(pslfe_device_upload(ctx.get(), dP, rows.data(), rows.size() * sizeof(PslPnpRow)), "upload");
            pslfe::check(pslfe_device_upload(ctx.get(), dN, np.data(), (size_t)K * 4), "upload");
            int refused = 0;
            matched = pslfe::PnPsolver::RelocalizeCandidates(
                ctx, K, (const PslPnpRow*)dP, (const int32_t*)dN, rstride, P.cam, cases[0].seed,
                [&](int round, int c, const PslPnpResult& r, const uint8_t* rowInliers) {
                    handed.push_back({round, c, r, std::vector<uint8_t>(rowInliers, rowInliers + np[c])});
                    return refused++ >= P.reject;
                },
                P.prob, P.minInliers, P.maxIts, P.epsilon, P.th2, P.nIterations);
            for (void* p : {dP, dN}) pslfe_device_free(ctx.get(), p);
        }
        const int32_t nh = (int32_t)handed.size();
        bool ok = fwrite(&matched, 4, 1, o) == 1 && fwrite(&nh, 4, 1, o) == 1;
        for (const Handed& h : handed) {
            ok = ok && fwrite(&h.round, 4, 1, o) == 1 && fwrite(&h.cand, 4, 1, o) == 1 && fwrite(&h.res, sizeof(h.res), 1, o) == 1;
            ok = ok && (h.flags.empty() || fwrite(h.flags.data(), 1, h.flags.size(), o) == h.flags.size());
        }
        if (!ok) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
#endif
    if (fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    printf("{\"candidates\": %d, \"loop_ms\": %.6f}\n", K, best);
    return 0;
}
