// libpslfe: line extractor object (== ORB_SLAM2::LINEextractor) over the HIP kernels. Product code.
// Reference: add_src/LineExtractor.cpp:6-25, 325-366; add_inc/LineExtractor.h:160-255.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "line_kernels2.h"
#include "line_kernels3.h"
#include "pslfe_internal.h"

#ifndef PSL_NFA_COUNT_WGS
#define PSL_NFA_COUNT_WGS 4   // workgroups (16 scan groups each) per frame of a many-frames k_lsd_nfa_count launch: 12288 dense frames, 8 waves per SIMD: 1: 38.2 ms, 2: 37.3, 3: 36.9,
                              // 4: 36.7; at 4 waves per SIMD 4: 38.1, 8: 39.9 (the default until round 3), 16: 45.2, 32: 59.1 (profiles/r03z_ab_nfa_grid.log)
#endif
// Launches with helper waves keep the `used` bits of their frames in LDS when those fit in this many bytes of the CU's 160 KB (the
// kernel's own arrays take 4 KB): scaled images up to ~1.18 M pixels.  Larger frames keep them in the `used` map in memory, as the
// many-frames launches do.
#define PSL_GROW_LDS_USED_MAX (144u * 1024u)
#ifndef PSL_GROW_HELPER_FRAMES
#define PSL_GROW_HELPER_FRAMES 64   // launches of at most this many frames run k_lsd_grow4 with helper waves (measured: tools/helper_sweep.sh)
#endif
// parts a launch of at least 2 * (PSL_GROW_HELPER_FRAMES + 1) frames is extracted in behind the gradient, alternately on the context's two streams
// (run_extract).  12288 dense frames, ms per step: 1: 373.5, 2: 349.9, 3: 365.7, 4: 382.9; 2 with the auxiliary stream at the highest priority
// 349.4, at the lowest 353.4: no priority stream (profiles/line_split_ab.log)
constexpr unsigned PSL_LINE_PIECES = 2;
// The first of the two parts takes this share of the frames (each part at least PSL_GROW_HELPER_FRAMES + 1).  The second part's grower ends last
// (at 188 of ~236 ms, whatever the share) and its NFA / merge / LBD launches follow it, the last 20 ms of them alone on the chip: the fewer frames
// they cover, the sooner the join.  12288 dense frames, ms per step: 12/24: 334.0 (the parent, same session), 13/24: 333.5, 14/24: 330.4,
// 15/24: 329.3, 16/24: 337.6 (another session, parent 335.7): 14/24, two steps in front of the cliff (profiles/line_pipeline_ab.log)
constexpr unsigned PSL_LINE_FIRST_NUM = 7, PSL_LINE_FIRST_DEN = 12;

// hipFuncSetAttribute acts on the function on the current device, not on an extractor object: the dynamic LDS k_lsd_grow4<3, 1> has
// been allowed is kept per device and only ever raised (an extractor of a smaller geometry must not lower what another one relies on)
#define PSL_GROW_LDS_DEVICES 64
static std::mutex g_grow_lds_mu;
static size_t g_grow_lds_attr[PSL_GROW_LDS_DEVICES];   // 0: the default 64 KB

static hipError_t psl_grow_lds_allow(int device, size_t bytes) {
    if (bytes <= 64u * 1024u) return hipSuccess;
    if (device < 0 || device >= PSL_GROW_LDS_DEVICES) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(g_grow_lds_mu);
    if (bytes <= g_grow_lds_attr[device]) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_lsd_grow4<3, 1>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) g_grow_lds_attr[device] = bytes;
    return e;
}

struct pslfe_line {
    pslfe_ctx* ctx = nullptr;
    int numOctaves = 1, nfeatures = 200, max_batch = 1;
    float scale = 1.2f;
    double min_line_length = 0;
    int refine = 2;  // LSD_REFINE_ADV (what the stock contrib LSDDetector constructs), 1 = LSD_REFINE_STD: pslfe_line_set_refine
    std::vector<float> scaleF, invScaleF, sigma2, invSigma2;

    int gw = 0, gh = 0;
    LineParams P;
    size_t in_fstride = 0;
    int in_pitch = 0;
    int last_nframes = 0;
    int kl_bound = 0;  // no frame's count in d_nkl exceeds this: which pairing kernel run_pair launches

    uint8_t* d_in = nullptr;
    double* d_scaled = nullptr;
    float* d_angdeg = nullptr;
    double* d_modgrad = nullptr;
    float2* d_trig = nullptr;     // (cosf, sinf) of the level-line angle per scaled pixel
    float2* d_seedt = nullptr;    // (float)cos / sin of the double angle for seeds: launches of at most PSL_GROW_HELPER_FRAMES frames only
    uint8_t* d_used = nullptr;    // LSD `used` map, one byte per scaled pixel
    uint32_t* d_reg = nullptr;
    LsdnTables NT = {};           // LSD_REFINE_ADV: log_gamma / log(p) tables of nfa() (NT.lg in HBM)
    double* d_lgamma = nullptr;
    double* d_sctab = nullptr;    // psl_sincostab.inc
    double* d_rects = nullptr;    // LSD_REFINE_ADV: rectangles of k_lsd_grow4 for k_lsd_nfa
    int* d_nrect = nullptr;
    int* d_weight = nullptr;   // [F] defined pixels per frame (k_lsd_grad) and [F] the frames by decreasing weight (k_frame_order)
    int* d_order = nullptr;
    float* d_segtmp = nullptr;
    uint8_t* d_keep = nullptr;
    int2* d_counts = nullptr;     // (n, k) of the five trial rectangles of a rect_improve phase
    int2* d_count0 = nullptr;     // (n, k) of the first test, whose pixel pass also counts phase -1's five trials into d_counts
    uint16_t* d_ulist = nullptr;  // [2][F][maxseg] the undecided rectangles of a frame, as left by the selection of the phase before (read / written alternately)
    int* d_ucount = nullptr;      // [5][F] their number: after the first test and after phases -1 .. 2
    double* d_vals = nullptr;     // their nfa() values
    double2* d_sstate = nullptr;  // (first term, p / (1 - p)) of the binomial tails that have to be summed
    LsdnSeries* d_slist = nullptr;  // ... as one list per frame, by predicted length (d_stmp: in item order, before the bucketing)
    LsdnSeries* d_stmp = nullptr;
    int* d_lcount = nullptr;        // class offsets in the list, [F][PSL_NFA_NCLS + 1]
    float* d_seg = nullptr;
    int* d_nseg = nullptr;
    MergeScratch M = {};
    PslKeyLine* d_kls = nullptr;
    uint8_t* d_ldesc = nullptr;
    float* d_fdesc = nullptr;
    double* d_lineEq = nullptr;
    int* d_nkl = nullptr;
    int* d_status = nullptr;
    short2* d_dxy = nullptr;
    float* d_rawfans = nullptr;
    float* d_fans = nullptr;
    int* d_nfans = nullptr;
    float* d_tmplines = nullptr;  // [NMAX][4] staging for the host-pointer pairing entry point

    PslDeviceBuffers mem;         // owns every d_* buffer above and those of M

    void release() {
        mem.release();
        gw = gh = 0;   // no geometry is prepared any more: the next call allocates again (or fails again) instead of
        last_nframes = 0;  // launching on freed memory
    }

    int prepare(int w, int h) {
        if (w == gw && h == gh) return PSLFE_OK;
        PSL_REQUIRE(w >= 16 && h >= 16 && w <= 8192 && h <= 8192, PSLFE_E_INVALID, "line: image %dx%d out of range", w, h);
        LineParams Q;
        memset(&Q, 0, sizeof(Q));
        Q.w = w; Q.h = h;
        Q.W = (int)nearbyint(w * 0.8);
        Q.H = (int)nearbyint(h * 0.8);
        Q.maxseg = PSL_MERGE_NMAX;
        Q.maxkl = std::max(1024, nfeatures);
        Q.nfeatures = nfeatures;
        {   // getGaussianKernel(7, 0.75, CV_64F): sigma = SIGMA_SCALE / SCALE, ksize = 1 + 2*ceil(sigma*sqrt(2*3*ln 10))
            const double sigma = 0.6 / 0.8;
            const int ksize = 1 + 2 * (int)ceil(sigma * sqrt(2 * 3.0 * log(10.0)));
            PSL_REQUIRE(ksize == 7, PSLFE_E_INVALID, "line: unexpected LSD kernel size %d", ksize);
            const double scale2X = -0.5 / (sigma * sigma);
            double sum = 0;
            for (int i = 0; i < 7; ++i) { const double x = i - 3.0; Q.gk[i] = exp(scale2X * x * x); sum += Q.gk[i]; }
            sum = 1. / sum;
            for (int i = 0; i < 7; ++i) Q.gk[i] *= sum;
        }
        Q.prec = PSL_PI * 22.5 / 180;
        Q.p = 22.5 / 180;
        Q.rho = 2.0 / sin(Q.prec);
        {   // largest q with sqrt(q) <= rho (sqrt correctly rounded and monotone, on the host as on the device): the
            // gradient threshold can then be decided on the squared magnitude, without a square root
            double q = Q.rho * Q.rho;
            while (sqrt(nextafter(q, INFINITY)) <= Q.rho) q = nextafter(q, INFINITY);
            while (sqrt(q) > Q.rho) q = nextafter(q, 0.0);
            Q.rho_q = q;
        }
        const double LOG_NT = 5 * (log10((double)Q.W) + log10((double)Q.H)) / 2 + log10(11.0);
        Q.min_reg_size = (int)(size_t)(-LOG_NT / log10(Q.p));
        Q.log_nt = LOG_NT;
        Q.refine = refine;
        {   // 8-bit GaussianBlur 5x5 sigma 1 -> integer kernel (OpenCV 3.2)
            float cf[5];
            double sum = 0;
            for (int i = 0; i < 5; ++i) { const double x = i - 2.0; cf[i] = (float)exp(-0.5 * x * x); sum += cf[i]; }
            sum = 1. / sum;
            for (int i = 0; i < 5; ++i) { cf[i] = (float)(cf[i] * sum); Q.lbdK[i] = (int)nearbyint((double)cf[i] * 256.0); }
        }
        {   // BinaryDescriptor ctor (binary_descriptor_custom.cpp:219-261), integer divisions as written there
            const int wb = 7, nb = 9;
            double u = (wb * 3 - 1) / 2, sigma = (wb * 2 + 1) / 2, inv = -1 / (2 * sigma * sigma);
            for (int i = 0; i < wb * 3; ++i) { const double d = i - u; Q.gaussL[i] = (float)exp(d * d * inv); }
            u = (nb * wb - 1) / 2; sigma = u; inv = -1 / (2 * sigma * sigma);
            for (int i = 0; i < nb * wb; ++i) { const double d = i - u; Q.gaussG[i] = (float)exp(d * d * inv); }
        }
        PSL_HIP(hipSetDevice(ctx->device));
        PSL_HIP(hipStreamSynchronize(ctx->stream));
        release();  // also forgets the old geometry: a failure below leaves an empty object, never a half-built one
        if (int rc = allocate(Q, w, h)) { release(); return rc; }
        P = Q;
        gw = w; gh = h;
        last_nframes = 0;
        return PSLFE_OK;
    }

    // the buffers of prepare() for max_batch frames of w x h, and the nfa() / sincos tables; Q.sctab set
    int allocate(LineParams& Q, int w, int h) {
        const size_t F = (size_t)max_batch, npx = (size_t)Q.W * Q.H, N = PSL_MERGE_NMAX;
        in_pitch = (int)psl_align_up(w, 16);
        in_fstride = psl_align_up((size_t)in_pitch * h, 256);
        static const double sctab[444] = {
#include "psl_sincostab.inc"
        };
        // nfa() tables: the same functions the device would evaluate, here on the host (bit-identical: single IEEE operations)
        const int lgn = 1 << 16;
        std::vector<double> lg((size_t)lgn, 0.0);
        for (int i = 1; i < lgn; ++i) lg[i] = lsdn_log_gamma((double)i);
        lg.resize((size_t)lgn + 3 * PSL_NFA_NP + PSL_RATIO_BMAX);   // the three log tables and 1 / i follow the log_gamma table in the same allocation
        for (int i = 1; i < PSL_RATIO_BMAX; ++i) lg[(size_t)lgn + 3 * PSL_NFA_NP + i] = 1.0 / (double)i;   // psl_ratio_inv's table (k_lsd_nfa_series)
        double pj = Q.p;
        for (int j = 0; j < PSL_NFA_NP; ++j, pj = pj / 2) {
            lg[(size_t)lgn + j] = psl_log(pj); lg[(size_t)lgn + PSL_NFA_NP + j] = psl_log(1.0 - pj); lg[(size_t)lgn + 2 * PSL_NFA_NP + j] = psl_log10(pj);
        }
        mem.alloc(d_in, in_fstride * F, "d_in");
        mem.alloc(d_scaled, npx * std::min<size_t>(F, PSL_LSD_SUBBATCH), "d_scaled");   // one sub-batch of the f64 working image (run_grad)
        mem.alloc(d_angdeg, npx * F, "d_angdeg");
        mem.alloc(d_modgrad, npx * F, "d_modgrad");
        mem.alloc(d_trig, npx * F, "d_trig");
        mem.alloc(d_seedt, npx * std::min<size_t>(F, PSL_GROW_HELPER_FRAMES), "d_seedt");   // many-frames launches evaluate the seed vector in the grower
        mem.alloc(d_used, npx * F, "d_used");
        mem.alloc(d_reg, npx * F, "d_reg");
        mem.alloc(d_seg, (size_t)Q.maxseg * 4 * F, "d_seg");
        mem.alloc(d_nseg, F, "d_nseg");
        mem.alloc(d_rects, (size_t)Q.maxseg * PSL_LSD_RECT_F64 * F, "d_rects");
        mem.alloc(d_nrect, F, "d_nrect");
        mem.alloc(d_weight, F, "d_weight");
        mem.alloc(d_order, F, "d_order");
        mem.alloc(d_segtmp, (size_t)Q.maxseg * 4 * F, "d_segtmp");
        mem.alloc(d_keep, (size_t)Q.maxseg * F, "d_keep");
        mem.alloc(d_counts, (size_t)Q.maxseg * 5 * F, "d_counts");
        mem.alloc(d_count0, (size_t)Q.maxseg * F, "d_count0");
        mem.alloc(d_ulist, (size_t)Q.maxseg * 2 * F, "d_ulist");
        mem.alloc(d_ucount, 5 * F, "d_ucount");
        mem.alloc(d_vals, (size_t)Q.maxseg * 5 * F, "d_vals");
        mem.alloc(d_sstate, (size_t)Q.maxseg * 5 * F, "d_sstate");
        mem.alloc(d_slist, (size_t)Q.maxseg * 5 * F, "d_slist");
        mem.alloc(d_stmp, (size_t)Q.maxseg * 5 * F, "d_stmp");
        mem.alloc(d_lcount, F * (PSL_NFA_NCLS + 1), "d_lcount");
        mem.alloc(d_sctab, sizeof(sctab) / sizeof(double), "d_sctab");
        mem.alloc(d_lgamma, lg.size(), "d_lgamma");
        mem.alloc(M.lines0, F * N * 4, "M.lines0");
        mem.alloc(M.lines1, F * N * 4, "M.lines1");
        mem.alloc(M.merged, F * N * 4, "M.merged");
        mem.alloc(M.angles, F * N, "M.angles");
        mem.alloc(M.length, F * N, "M.length");
        mem.alloc(M.order, F * N, "M.order");
        mem.alloc(M.pos, F * N, "M.pos");
        mem.alloc(M.adj, F * N * (N / 32), "M.adj");
        mem.alloc(M.code, F * N, "M.code");
        mem.alloc(M.clist, F * PSL_MERGE_CLMAX, "M.clist");
        mem.alloc(M.coff, F * (2 * N + 2), "M.coff");
        mem.alloc(M.work, F * 4 * N, "M.work");
        mem.alloc(M.bits, F * (N / 32), "M.bits");
        mem.alloc(M.stage, F * N, "M.stage");
        mem.alloc(d_kls, F * Q.maxkl, "d_kls");
        mem.alloc(d_ldesc, F * Q.maxkl * 32, "d_ldesc");
        mem.alloc(d_fdesc, F * Q.maxkl * 72, "d_fdesc");
        mem.alloc(d_lineEq, F * Q.maxkl * 3, "d_lineEq");
        mem.alloc(d_nkl, F, "d_nkl");
        mem.alloc(d_status, F, "d_status");
        mem.alloc(d_dxy, F * (size_t)w * h, "d_dxy");
        mem.alloc(d_rawfans, F * PSL_FAN_CAP * 4, "d_rawfans");
        mem.alloc(d_fans, F * PSL_FAN_CAP * 4, "d_fans");
        mem.alloc(d_nfans, F, "d_nfans");
        mem.alloc(d_tmplines, N * 4, "d_tmplines");
        if (int rc = mem.check("line")) return rc;
        PSL_HIP(hipMemcpy(d_sctab, sctab, sizeof(sctab), hipMemcpyHostToDevice));
        Q.sctab = d_sctab;
        PSL_HIP(hipMemcpy(d_lgamma, lg.data(), lg.size() * sizeof(double), hipMemcpyHostToDevice));
        NT.lg = d_lgamma; NT.logs = d_lgamma + lgn; NT.lg_n = lgn; NT.p0 = Q.p; NT.log_nt = Q.log_nt; NT.inv = d_lgamma + lgn + 3 * PSL_NFA_NP;
        return PSLFE_OK;
    }

    // Frames [f0, f0 + n) of a launch of F frames, for the launches of stream `st`: every per-frame array advanced to frame f0.  The kernels
    // count frames from their own blockIdx, so a part needs nothing but these pointers and n; the two arrays laid out [k][F] keep the
    // launch's stride F (ul(), uc()).  order: the part's own segment of d_order, frame indices relative to f0 (k_frame_order on the
    // part's weights).  Parts of one launch share no buffer.
    struct Part {
        unsigned f0, n, F;
        hipStream_t st;
        float* angdeg; double* modgrad; float2* trig; float2* seedt; uint8_t* used; uint32_t* reg;
        double* rects; int* nrect; int* weight; int* order;
        int2* counts; int2* count0; uint16_t* ulist; int* ucount; double* vals; double2* sstate; LsdnSeries* slist; LsdnSeries* stmp; int* lcount;
        uint8_t* keep; float* segtmp; float* seg; int* nseg;
        MergeScratch M;
        PslKeyLine* kls; uint8_t* ldesc; float* fdesc; double* lineEq; int* nkl; int* status; short2* dxy;
        size_t maxseg;
        uint16_t* ul(int k) const { return k >= 0 ? ulist + (size_t)(k & 1) * maxseg * F : nullptr; }
        int* uc(int k) const { return k >= 0 && k < 5 ? ucount + (size_t)k * F : nullptr; }
    };

    Part part(unsigned f0, unsigned n, unsigned F, hipStream_t st) const {
        const size_t npx = (size_t)P.W * P.H, S = (size_t)P.maxseg, K = (size_t)P.maxkl, N = PSL_MERGE_NMAX;
        auto at = [f0](auto* base, size_t per_frame) { return base + (size_t)f0 * per_frame; };
        Part p;
        p.f0 = f0; p.n = n; p.F = F; p.st = st; p.maxseg = S;
        p.angdeg = at(d_angdeg, npx); p.modgrad = at(d_modgrad, npx); p.trig = at(d_trig, npx);
        p.seedt = F <= PSL_GROW_HELPER_FRAMES ? at(d_seedt, npx) : nullptr;   // the table holds the frames of a few-frames launch only
        p.used = at(d_used, npx); p.reg = at(d_reg, npx);
        p.rects = at(d_rects, S * PSL_LSD_RECT_F64); p.nrect = at(d_nrect, 1); p.weight = at(d_weight, 1); p.order = at(d_order, 1);
        p.counts = at(d_counts, S * 5); p.count0 = at(d_count0, S); p.ulist = at(d_ulist, S); p.ucount = at(d_ucount, 1);
        p.vals = at(d_vals, S * 5); p.sstate = at(d_sstate, S * 5); p.slist = at(d_slist, S * 5); p.stmp = at(d_stmp, S * 5);
        p.lcount = at(d_lcount, PSL_NFA_NCLS + 1);
        p.keep = at(d_keep, S); p.segtmp = at(d_segtmp, S * 4); p.seg = at(d_seg, S * 4); p.nseg = at(d_nseg, 1);
        p.M.lines0 = at(M.lines0, N * 4); p.M.lines1 = at(M.lines1, N * 4); p.M.merged = at(M.merged, N * 4);
        p.M.angles = at(M.angles, N); p.M.length = at(M.length, N); p.M.order = at(M.order, N); p.M.pos = at(M.pos, N);
        p.M.adj = at(M.adj, N * (N / 32)); p.M.code = at(M.code, N); p.M.clist = at(M.clist, PSL_MERGE_CLMAX);
        p.M.coff = at(M.coff, 2 * N + 2); p.M.work = at(M.work, 4 * N); p.M.bits = at(M.bits, N / 32); p.M.stage = at(M.stage, N);
        p.kls = at(d_kls, K); p.ldesc = at(d_ldesc, K * 32); p.fdesc = at(d_fdesc, K * 72); p.lineEq = at(d_lineEq, K * 3);
        p.nkl = at(d_nkl, 1); p.status = at(d_status, 1); p.dxy = at(d_dxy, (size_t)P.w * P.h);
        return p;
    }
    Part whole(int nframes) const { return part(0, (unsigned)nframes, (unsigned)nframes, ctx->stream); }

    // A launch of F frames runs as (profiles/r03z_switch_matrix.log, profiles/line_split_ab.log):
    //   F <= PSL_GROW_HELPER_FRAMES (64)   k_lsd_grow4<3, 1> (<3, 0> for frames whose `used` bits do not fit in LDS): helper waves, P.singles
    //                                      and the seed vectors from k_lsd_grad's table d_seedt (larger launches: evaluated by k_lsd_grow4<0, 0>)
    //   F >= 64                            the many-frames NFA grids
    //   F > 64                             k_lsd_grow4<0, 0> on the frames in k_frame_order's order
    //   F > PSL_LSD_SUBBATCH (2048)        scale / gradient in sub-batches
    //   F >= 2 * (64 + 1) = 130            pslfe_line_extract_batch_device: everything behind the gradient in PSL_LINE_PIECES parts on two streams
    //                                      (run_extract), each part a many-frames launch of its own: the first 7/12 of the frames, the second
    //                                      the rest, each at least 65 frames (130: 65 + 65, 131: 66 + 65, 12288: 7168 + 5120); the second
    //                                      part's k_lbd_pre on the first part's stream (profiles/line_pipeline_ab.log)
    // LSD steps 1 + 2 (scaled image, gradient) of every frame, and the launch's memsets; on the context's stream
    int run_grad(const uint8_t* d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
        int rc = prepare(w, h);
        if (rc) return rc;
        PSL_HIP(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const unsigned F = (unsigned)nframes;
        // in sub-batches of PSL_LSD_SUBBATCH frames: the f64 working image (1.57 MB per frame) only lives between the two kernels, so
        // d_scaled holds one sub-batch (3.2 GB instead of 19 GB at 12288 frames); 2048 frames x 192 tiles still fill the chip many times over
        PSL_HIP(hipMemsetAsync(d_used, 0, (size_t)P.W * P.H * F, st));  // the `used` map: 1 byte per scaled pixel
        P.singles = F <= PSL_GROW_HELPER_FRAMES;
        P.full_grad = nframes == 1;  // pslfe_line_debug_gradient reads the whole magnitude image of a single-frame call
        P.refine = refine;
        const bool ordered = F > PSL_GROW_HELPER_FRAMES;   // many-frames launches: k_lsd_grow4 takes the heaviest frames first
        if (ordered) PSL_HIP(hipMemsetAsync(d_weight, 0, (size_t)F * sizeof(int), st));
        if (refine >= 2) PSL_HIP(hipMemsetAsync(d_ucount, 0, (size_t)5 * F * sizeof(int), st));   // the undecided lists of the NFA phases (run_detect)
        const unsigned tx = (P.W + 63) / 64, ty = (P.H + 15) / 16, gy = (P.H + PSL_GRAD_TH - 1) / PSL_GRAD_TH;
        const size_t npx = (size_t)P.W * P.H;
        for (unsigned f0 = 0; f0 < F; f0 += PSL_LSD_SUBBATCH) {
            const unsigned n = std::min<unsigned>(PSL_LSD_SUBBATCH, F - f0);
            const int xcd = n >= 8 ? 1 : 0;
            const size_t po = (size_t)f0 * npx;
            {
                PSL_STAGE_BEGIN(ctx, "line.lsd_scale");
                k_lsd_scale_tiled<<<xcd ? dim3(8, tx * ty, (n + 7) / 8) : dim3(tx, ty, n), 256, 0, st>>>(P, d_gray + (size_t)f0 * frame_stride, stride, frame_stride,
                                                                                                         d_scaled, (int)n, xcd);
                PSL_STAGE_END(ctx, "line.lsd_scale");
            }
            {
                PSL_STAGE_BEGIN(ctx, "line.lsd_grad");
                k_lsd_grad<<<xcd ? dim3(8, tx * gy, (n + 7) / 8) : dim3(tx, gy, n), 256, 0, st>>>(P, d_scaled, d_angdeg + po, d_modgrad + po, d_trig + po, P.singles ? d_seedt + po : nullptr,
                                                                                                  d_used + po, ordered ? d_weight + f0 : nullptr, (int)n, xcd);
                PSL_STAGE_END(ctx, "line.lsd_grad");
            }
        }
        PSL_HIP(hipGetLastError());
        return PSLFE_OK;
    }

    // LSD step 3 on the frames of a part: region growing, and with LSD_REFINE_ADV the NFA validation of its rectangles -> p.seg / p.nseg
    int run_detect(const Part& p) {
        hipStream_t st = p.st;
        const unsigned n = p.n;
        int* const ngrow = refine >= 2 ? p.nrect : p.nseg;
        const bool ordered = n > PSL_GROW_HELPER_FRAMES;   // many-frames launches: the heaviest frames of the part first
        if (ordered) k_frame_order<<<1, 1024, 0, st>>>(p.weight, (int)n, P.W * P.H, p.order);
        {
            PSL_STAGE_BEGIN_ON(ctx, "line.lsd_grow", st);
            // LSD_REFINE_ADV: the kernel leaves rectangles (rects / nrect) for the NFA validation below
            PSL_REQUIRE(ordered || p.seedt != nullptr, PSLFE_E_INVALID, "line: a part of %u frames of a launch of %u has no seed table", n, p.F);
            if (!ordered) {  // few workgroups per XCD: three more waves each keep that XCD's L2 warm in front of the chain (line_kernels.h)
                const size_t ubytes = (((size_t)P.W * P.H + 31) >> 5) * 4;   // the `used` bits of the frame in LDS (24 KB at 640x480, 96 KB at 1280x960)
                if (ubytes <= PSL_GROW_LDS_USED_MAX) {
                    PSL_HIP(psl_grow_lds_allow(ctx->device, ubytes));   // more than the default 64 KB of dynamic LDS needs the attribute
                    k_lsd_grow4<3, 1><<<n, 256, ubytes, st>>>(P, p.angdeg, p.modgrad, p.trig, p.used, p.seedt, p.reg, p.seg, ngrow, p.rects, (int)n, nullptr);
                } else {
                    k_lsd_grow4<3, 0><<<n, 256, 0, st>>>(P, p.angdeg, p.modgrad, p.trig, p.used, p.seedt, p.reg, p.seg, ngrow, p.rects, (int)n, nullptr);
                }
            } else
                k_lsd_grow4<0, 0><<<n, 64, 0, st>>>(P, p.angdeg, p.modgrad, p.trig, p.used, p.seedt, p.reg, p.seg, ngrow, p.rects, (int)n, p.order);
            PSL_STAGE_END_ON(ctx, "line.lsd_grow", st);
            PSL_HIP(hipGetLastError());   // a refused grow launch (e.g. its dynamic LDS) must not hide behind the NFA launches
        }
        if (refine >= 2) {
            // rect_improve + NFA: per phase a pixel-scan launch (16 lanes = rectangle), two nfa() launches (thread = evaluation:
            // set-up, then the binomial tails drawn from a shared counter) and a selection launch (thread = rectangle), line_kernels3.h.  A few hundred rectangles per frame: a many-frames launch fills
            // the chip by frames, a single frame by chunks.  (The stage timers record the launches of a phase as they are issued;
            // with profiling on, every stage costs two event records.)
            // List k holds the rectangles still undecided after the first test (k = 0) and after phases -1 .. 2 (k = 1 .. 4): phase PH
            // walks list PH + 1 and fills list PH + 2.  Phase -1 has no pixel scan of its own: the first test's pass counts its trials.
            const dim3 gc(n >= 64 ? PSL_NFA_COUNT_WGS : 128, n), gs(n >= 64 ? 1 : 4, n);
#define PSL_NFA_COUNT(PH)                                                                                                \
    {                                                                                                                    \
        PSL_STAGE_BEGIN_ON(ctx, "line.nfa_count", st);                                                                   \
        k_lsd_nfa_count<PH><<<gc, 256, 0, st>>>(P, p.angdeg, p.rects, p.nrect, p.ul(PH + 1), p.uc(PH + 1), p.counts, p.count0); \
        PSL_STAGE_END_ON(ctx, "line.nfa_count", st);                                                                     \
    }
#define PSL_NFA_EVAL(PH)                                                                                                 \
    {                                                                                                                    \
        PSL_STAGE_BEGIN_ON(ctx, "line.nfa_eval", st);                                                                    \
        k_lsd_nfa_setup<PH><<<n, 256, 0, st>>>(P, NT, p.rects, p.nrect, p.ul(PH + 1), p.uc(PH + 1), p.counts, p.count0, p.vals, p.sstate, p.stmp, p.slist, p.lcount); \
        k_lsd_nfa_series<PH><<<dim3(PSL_NFA_NCLS, (n + PSL_NFA_FG - 1) / PSL_NFA_FG), 256, 0, st>>>(P, NT, (int)n, p.slist, p.lcount, p.sstate); \
        k_lsd_nfa_select<PH><<<gs, 256, 0, st>>>(P, NT.log_nt, p.rects, p.nrect, p.ul(PH + 1), p.uc(PH + 1), p.keep, p.vals, p.sstate, p.segtmp, \
                                                 PH < 3 ? p.ul(PH + 2) : nullptr, p.uc(PH + 2));                         \
        PSL_STAGE_END_ON(ctx, "line.nfa_eval", st);                                                                      \
    }
            PSL_NFA_COUNT(PSL_NFA_FIRST)
            PSL_NFA_EVAL(PSL_NFA_FIRST)
            PSL_NFA_EVAL(-1)
            PSL_NFA_COUNT(0)
            PSL_NFA_EVAL(0)
            PSL_NFA_COUNT(1)
            PSL_NFA_EVAL(1)
            PSL_NFA_COUNT(2)
            PSL_NFA_EVAL(2)
            PSL_NFA_COUNT(3)
            PSL_NFA_EVAL(3)
#undef PSL_NFA_COUNT
#undef PSL_NFA_EVAL
            k_lsd_emit<<<n, 256, 0, st>>>(P, p.nrect, p.segtmp, p.keep, p.seg, p.nseg);
        }
        PSL_HIP(hipGetLastError());
        return PSLFE_OK;
    }

    // LineSegmentDetector::detect on a launch of its own -> d_seg / d_nseg
    int run_lsd(const uint8_t* d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
        int rc = run_grad(d_gray, nframes, w, h, stride, frame_stride);
        if (rc) return rc;
        if ((rc = run_detect(whole(nframes)))) return rc;
        last_nframes = nframes;
        return PSLFE_OK;
    }

    // optimizeAndMergeLines_lsd + KeyLines + top-N + line equations on the segment lists in p.seg / p.nseg
    int run_merge(const Part& p) {
        PSL_HIP(hipSetDevice(ctx->device));
        kl_bound = std::max(kl_bound, std::min(P.maxkl, std::max(P.nfeatures, 0)));  // the top-N cut of k_line_merge
        PSL_STAGE_BEGIN_ON(ctx, "line.merge", p.st);
        k_line_merge<PSL_MERGE_LDSN_SMALL><<<p.n, 256, 0, p.st>>>(P, p.M, p.seg, p.nseg, p.kls, p.lineEq, p.nkl, p.status);
        k_line_merge<PSL_MERGE_LDSN><<<p.n, 256, 0, p.st>>>(P, p.M, p.seg, p.nseg, p.kls, p.lineEq, p.nkl, p.status);
        PSL_STAGE_END_ON(ctx, "line.merge", p.st);
        PSL_HIP(hipGetLastError());
        return PSLFE_OK;
    }

    // BinaryDescriptor::compute on the keylines in p.kls / p.nkl; d_gray is frame 0 of the launch
    int run_lbd(const Part& p, const uint8_t* d_gray, int stride, size_t frame_stride, bool want_float) {
        const int rc = run_lbd_pre(p, d_gray, stride, frame_stride, p.st);
        return rc ? rc : run_lbd_rows(p, want_float);
    }

    // the derivatives of the blurred image (p.dxy) of the frames of a part: they depend on the gray image alone, so stream st may be
    // another than the part's (run_extract)
    int run_lbd_pre(const Part& p, const uint8_t* d_gray, int stride, size_t frame_stride, hipStream_t st) {
        PSL_HIP(hipSetDevice(ctx->device));
        const int n = (int)p.n;
        PSL_STAGE_BEGIN_ON(ctx, "line.lbd_pre", st);
        const unsigned tx = (P.w + 63) / 64, ty = (P.h + 31) / 32;
        const int xcd = n >= 8 ? 1 : 0;
        k_lbd_pre<<<xcd ? dim3(8, tx * ty, (n + 7) / 8) : dim3(tx, ty, n), 256, 0, st>>>(P, d_gray + (size_t)p.f0 * frame_stride, stride, frame_stride, p.dxy, n, xcd);
        PSL_STAGE_END_ON(ctx, "line.lbd_pre", st);
        PSL_HIP(hipGetLastError());
        return PSLFE_OK;
    }

    // the descriptor rows, from p.dxy and the keylines of the part
    int run_lbd_rows(const Part& p, bool want_float) {
        PSL_HIP(hipSetDevice(ctx->device));
        hipStream_t st = p.st;
        const int n = (int)p.n;
        {
            PSL_STAGE_BEGIN_ON(ctx, "line.lbd", st);
            const int per_frame = std::min(P.maxkl, std::max(P.nfeatures, 1));
            // plain grid: with all line blocks of a frame on one XCD (grid (8, blocks, ceil(n / 8))) the row-major kernel gained 1.1 of 16.4 ms,
            // the kernel with the step-major path nothing (profiles/lbd_layout_ab.log)
            k_lbd<<<dim3((per_frame + 3) / 4, n), 256, 0, st>>>(P, p.dxy, p.kls, p.nkl, p.ldesc, want_float ? p.fdesc : nullptr);
            PSL_STAGE_END_ON(ctx, "line.lbd", st);
        }
        PSL_HIP(hipGetLastError());
        return PSLFE_OK;
    }

    // LSD behind the gradient, merge and LBD of the frames of one part
    int run_part(const Part& p, const uint8_t* d_gray, int stride, size_t frame_stride) {
        int rc = run_detect(p);
        if (rc) return rc;
        if ((rc = run_merge(p))) return rc;
        return run_lbd(p, d_gray, stride, frame_stride, false);
    }

    // run_part of A on its stream and of B on its own, with k_lbd_pre of B on A's stream behind A's launches (ev_pre).  The wait is only
    // issued behind its record: a failed launch leaves no stream waiting for an event of this call that was never recorded.
    int run_halves(const Part& A, const Part& B, const uint8_t* d_gray, int stride, size_t frame_stride) {
        int rc = run_part(A, d_gray, stride, frame_stride);
        if (rc) return rc;
        if ((rc = run_lbd_pre(B, d_gray, stride, frame_stride, A.st))) return rc;
        PSL_HIP(hipEventRecord(ctx->ev_pre, A.st));
        if ((rc = run_detect(B))) return rc;
        if ((rc = run_merge(B))) return rc;
        PSL_HIP(hipStreamWaitEvent(B.st, ctx->ev_pre, 0));
        return run_lbd_rows(B, false);
    }

    // LINEextractor::operator() on every frame of a launch.  The frames are independent, yet each kernel behind the gradient lasts as
    // long as its slowest frame: k_lsd_grow4<0, 0> (one wave per frame, 12288 waves on 8192 slots) holds 6.77 of 8 slots per SIMD on
    // average, and nothing else can start while its tail drains.  So a launch of at least 2 * (PSL_GROW_HELPER_FRAMES + 1) frames runs
    // that part of the work in PSL_LINE_PIECES parts of contiguous frames, alternately on the context's stream and on its auxiliary
    // stream: the NFA / merge / LBD kernels of one part fill the slots the growing of the next one leaves.  Every part is a many-frames
    // launch of its own (own k_frame_order), so a frame's result does not depend on the split.  With stage profiling on, the launch
    // stays on one stream, so that the stage timers keep their meaning.
    //   context's stream:   scale / gradient of all frames | ev_fork | A: grow, NFA, merge, k_lbd_pre, k_lbd | k_lbd_pre of B | ev_pre |      wait ev_join
    //   auxiliary stream:                             wait ev_fork | B: grow,                  NFA, merge | wait ev_pre | k_lbd of B | ev_join
    // The two growers start together; A's workgroups are dispatched first, so A's grower ends early (131 ms into a launch of 12288 dense
    // frames, B's at 187) and A's chain runs in the tail of B's grower and beside the first half of B's chain (until 222); the join is
    // at 232 (profiles/line_pipeline_ab.log).  B's chain ends the launch, so B is the smaller part (PSL_LINE_FIRST_NUM), and its
    // k_lbd_pre, which reads nothing but the gray image, runs on the context's stream behind A's chain instead of behind B's merge.
    int run_extract(const uint8_t* d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
        int rc = run_grad(d_gray, nframes, w, h, stride, frame_stride);
        if (rc) return rc;
        const unsigned F = (unsigned)nframes;
        if (F < PSL_LINE_PIECES * (PSL_GROW_HELPER_FRAMES + 1) || ctx->profile) {
            if ((rc = run_part(whole(nframes), d_gray, stride, frame_stride))) return rc;
        } else {
            const unsigned least = PSL_GROW_HELPER_FRAMES + 1;   // both parts are many-frames launches
            const unsigned fB = std::min(std::max((unsigned)((size_t)F * PSL_LINE_FIRST_NUM / PSL_LINE_FIRST_DEN), least), F - least);
            PSL_HIP(hipEventRecord(ctx->ev_fork, ctx->stream));
            PSL_HIP(hipStreamWaitEvent(ctx->aux_stream, ctx->ev_fork, 0));
            rc = run_halves(part(0, fB, F, ctx->stream), part(fB, F - fB, F, ctx->aux_stream), d_gray, stride, frame_stride);
            // the join, also after a failed launch: the caller's stream must not run ahead of what the auxiliary stream was given
            const hipError_t ej = hipEventRecord(ctx->ev_join, ctx->aux_stream);
            const hipError_t ew = ej == hipSuccess ? hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0) : ej;
            if (ew != hipSuccess) (void)hipStreamSynchronize(ctx->aux_stream);
            if (rc) return rc;
            PSL_HIP(ew);
        }
        last_nframes = nframes;
        return PSLFE_OK;
    }

    int run_pair(int nframes, float radius, float fanThr) {
        PSL_HIP(hipSetDevice(ctx->device));
        PSL_STAGE_BEGIN(ctx, "line.pair");
        // mLines = (startPointX, startPointY, endPointX, endPointY) of every keyline (src/Frame.cc:355-373):
        // these are 4 consecutive floats at offset 7 of the 17-word KeyLine record
        // up to PSL_PAIR_LDSN lines per frame the kernel keeps in LDS
        (kl_bound <= PSL_PAIR_LDSN ? k_lil_pair : k_lil_pair_big)<<<nframes, 256, 0, ctx->stream>>>(
            reinterpret_cast<const float*>(d_kls) + 7, (size_t)P.maxkl * 17, 17, d_nkl, 0, radius, fanThr, P.w, P.h, d_rawfans, d_fans, PSL_FAN_CAP, d_nfans);
        PSL_STAGE_END(ctx, "line.pair");
        PSL_HIP(hipGetLastError());
        return PSLFE_OK;
    }

    int upload(const uint8_t* gray, int nframes, int w, int h, int stride, size_t frame_stride) {
        int rc = prepare(w, h);
        if (rc) return rc;
        PSL_HIP(hipSetDevice(ctx->device));
        for (int f = 0; f < nframes; ++f)
            PSL_HIP(hipMemcpy2DAsync(d_in + (size_t)f * in_fstride, in_pitch, gray + (size_t)f * frame_stride, stride, w, h,
                                     hipMemcpyHostToDevice, ctx->stream));
        return PSLFE_OK;
    }
};

extern "C" {

int pslfe_line_create(pslfe_ctx* ctx, int numOctaves, float scale, int nLSDFeature, double min_line_length, int max_batch,
                      pslfe_line** out) {
    PSL_REQUIRE(ctx && out, PSLFE_E_INVALID, "pslfe_line_create: NULL argument");
    *out = nullptr;
    PSL_REQUIRE(numOctaves >= 1 && numOctaves <= PSLFE_MAX_LEVELS && nLSDFeature >= 1 && nLSDFeature <= 2048 && max_batch >= 1 && max_batch <= 65535,
                PSLFE_E_INVALID, "pslfe_line_create: numOctaves %d nLSDFeature %d max_batch %d", numOctaves, nLSDFeature, max_batch);
    // LINEextractor::operator() calls detect(image, kls, scale, numOctaves) (add_src/LineExtractor.cpp:336-337) whose `int scale` parameter
    // truncates the float member 1.2 to 1.  With numOctaves > 1 the stock contrib LSDDetector the reference links then builds its pyramid with
    // pyrDown(m, m, Size(cols / 1, rows / 1)) - a destination of the SOURCE's size, which pyrDown's size assertion (|2 dst - src| <= 2)
    // rejects with a cv::Exception (opencv_contrib 3.x LSDDetector.cpp: computeGaussianPyramid; the vendored twin, which the reference does not
    // call, discards that Size through a comma expression: Thirdparty/line_descriptor/src/LSDDetector_custom.cpp:71).  So the reference's own
    // call cannot produce a result for numOctaves > 1 - every RGB-D YAML sets LINEextractor.nLevels: 1 - and an error here is its behaviour.
    PSL_REQUIRE(numOctaves == 1, PSLFE_E_INVALID,
                "pslfe_line_create: numOctaves %d: the reference's LSDDetector::detect(image, kls, (int)1.2f, numOctaves) throws for numOctaves > 1 "
                "(pyrDown to the source's own size); only numOctaves == 1 yields lines", numOctaves);
    pslfe_line* l = new pslfe_line();
    l->ctx = ctx; l->numOctaves = numOctaves; l->scale = scale; l->nfeatures = nLSDFeature; l->min_line_length = min_line_length;
    l->max_batch = max_batch;
    // add_src/LineExtractor.cpp:8-24
    l->scaleF.resize(numOctaves); l->sigma2.resize(numOctaves); l->invScaleF.resize(numOctaves); l->invSigma2.resize(numOctaves);
    l->scaleF[0] = 1.0f; l->sigma2[0] = 1.0f;
    for (int i = 1; i < numOctaves; ++i) { l->scaleF[i] = l->scaleF[i - 1] * scale; l->sigma2[i] = l->scaleF[i] * l->scaleF[i]; }
    for (int i = 0; i < numOctaves; ++i) { l->invScaleF[i] = 1.0f / l->scaleF[i]; l->invSigma2[i] = 1.0f / l->sigma2[i]; }
    *out = l;
    return PSLFE_OK;
}

void pslfe_line_destroy(pslfe_line* line) {
    if (!line) return;
    (void)hipSetDevice(line->ctx->device);
    (void)hipStreamSynchronize(line->ctx->stream);
    delete line;   // its buffers go with it
}

int pslfe_line_set_refine(pslfe_line* line, int refine) {
    PSL_REQUIRE(line, PSLFE_E_INVALID, "pslfe_line_set_refine: line is NULL");
    PSL_REQUIRE(refine == PSLFE_LSD_REFINE_STD || refine == PSLFE_LSD_REFINE_ADV, PSLFE_E_INVALID, "pslfe_line_set_refine: mode %d", refine);
    line->refine = refine;
    return PSLFE_OK;
}

int pslfe_line_levels(const pslfe_line* line) { return line ? line->numOctaves : PSLFE_E_INVALID; }
float pslfe_line_scale_factor(const pslfe_line* line) { return line ? line->scale : 0.f; }
int pslfe_line_scale_factors(const pslfe_line* line, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2) {
    PSL_REQUIRE(line, PSLFE_E_INVALID, "pslfe_line_scale_factors: line is NULL");
    for (int i = 0; i < line->numOctaves; ++i) {
        if (scale) scale[i] = line->scaleF[i];
        if (inv_scale) inv_scale[i] = line->invScaleF[i];
        if (sigma2) sigma2[i] = line->sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = line->invSigma2[i];
    }
    return PSLFE_OK;
}

int pslfe_lsd_detect(pslfe_line* line, const uint8_t* gray, int w, int h, int stride, float* segments, int cap, int* n) {
    PSL_REQUIRE(line && n, PSLFE_E_INVALID, "pslfe_lsd_detect: NULL argument");
    *n = 0;
    if (!gray || w <= 0 || h <= 0) return PSLFE_OK;
    PSL_REQUIRE(stride >= w, PSLFE_E_INVALID, "pslfe_lsd_detect: stride %d < width %d", stride, w);
    int rc = line->upload(gray, 1, w, h, stride, (size_t)stride * h);
    if (rc) return rc;
    rc = line->run_lsd(line->d_in, 1, w, h, line->in_pitch, line->in_fstride);
    if (rc) return rc;
    hipStream_t st = line->ctx->stream;
    int cnt = 0;
    PSL_HIP(hipMemcpyAsync(&cnt, line->d_nseg, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *n = cnt;
    PSL_REQUIRE(cnt <= cap, PSLFE_E_CAPACITY, "pslfe_lsd_detect: %d segments, capacity %d", cnt, cap);
    if (cnt > 0 && segments) {
        PSL_HIP(hipMemcpyAsync(segments, line->d_seg, (size_t)cnt * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipStreamSynchronize(st));
    }
    return PSLFE_OK;
}

int pslfe_line_debug_gradient(pslfe_line* line, int frame, int* W, int* H, double* scaled, float* angle_deg, double* modgrad) {
    PSL_REQUIRE(line && W && H, PSLFE_E_INVALID, "pslfe_line_debug_gradient: NULL argument");
    PSL_REQUIRE(line->last_nframes > 0 && frame >= 0 && frame < line->last_nframes, PSLFE_E_STATE, "pslfe_line_debug_gradient: frame %d", frame);
    PSL_HIP(hipSetDevice(line->ctx->device));
    PSL_HIP(hipStreamSynchronize(line->ctx->stream));
    *W = line->P.W; *H = line->P.H;
    const size_t npx = (size_t)line->P.W * line->P.H;
    if (scaled) {   // the working image is kept for one sub-batch only (run_grad)
        PSL_REQUIRE(line->last_nframes <= PSL_LSD_SUBBATCH, PSLFE_E_STATE, "pslfe_line_debug_gradient: the scaled image is kept for launches of at most %d frames", PSL_LSD_SUBBATCH);
        PSL_HIP(hipMemcpy(scaled, line->d_scaled + frame * npx, npx * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (angle_deg) PSL_HIP(hipMemcpy(angle_deg, line->d_angdeg + frame * npx, npx * sizeof(float), hipMemcpyDeviceToHost));
    if (modgrad) PSL_HIP(hipMemcpy(modgrad, line->d_modgrad + frame * npx, npx * sizeof(double), hipMemcpyDeviceToHost));
    return PSLFE_OK;
}


// nfa() on caller-supplied trials: the launches PSL_NFA_EVAL(PH) of run_detect without the selection, on state written here instead of
// counted in an image.  Runs no kernel of its own.
int pslfe_line_debug_nfa(pslfe_line* line, int w, int h, int phase, int nframes, const int32_t* nrect, int rect_cap, const double* p_lognfa,
                         const int32_t* nk, double* vals, double* tail, double* log_nt) {
    PSL_REQUIRE(line && nrect && p_lognfa && nk && vals && tail, PSLFE_E_INVALID, "pslfe_line_debug_nfa: NULL argument");
    PSL_REQUIRE(phase == PSL_NFA_FIRST || (phase >= -1 && phase <= 3), PSLFE_E_INVALID, "pslfe_line_debug_nfa: phase %d", phase);
    PSL_REQUIRE(nframes >= 1 && nframes <= line->max_batch, PSLFE_E_INVALID, "pslfe_line_debug_nfa: nframes %d (max_batch %d)", nframes, line->max_batch);
    PSL_REQUIRE(rect_cap >= 1 && rect_cap <= PSL_MERGE_NMAX, PSLFE_E_INVALID, "pslfe_line_debug_nfa: rect_cap %d (at most %d)", rect_cap, PSL_MERGE_NMAX);
    const int TR = phase == PSL_NFA_FIRST ? 1 : 5;
    for (int f = 0; f < nframes; ++f) {
        PSL_REQUIRE(nrect[f] >= 0 && nrect[f] <= rect_cap, PSLFE_E_INVALID, "pslfe_line_debug_nfa: frame %d has %d rectangles (rect_cap %d)", f, nrect[f], rect_cap);
        for (int r = 0; r < nrect[f]; ++r) {
            const double p = p_lognfa[((size_t)f * rect_cap + r) * 2];
            PSL_REQUIRE(p > 0.0 && p < 1.0, PSLFE_E_INVALID, "pslfe_line_debug_nfa: frame %d rectangle %d: p %g", f, r, p);
            for (int t = 0; t < TR; ++t) {
                const int32_t* c = nk + (((size_t)f * rect_cap + r) * 5 + t) * 2;
                PSL_REQUIRE(c[0] < 0 || (c[1] >= 0 && c[1] <= c[0] && c[0] <= (1 << 24)), PSLFE_E_INVALID,
                            "pslfe_line_debug_nfa: frame %d rectangle %d trial %d: (n, k) = (%d, %d)", f, r, t, c[0], c[1]);
            }
        }
    }
    int rc = line->prepare(w, h);
    if (rc) return rc;
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    const LineParams& P = line->P;
    const size_t F = (size_t)nframes, N = (size_t)P.maxseg;
    // the state the count and select launches of an extraction leave for this phase: rectangles (p, log_nfa), their (n, k), and the list
    // of undecided rectangles the phase walks (every rectangle, in descending order: results are stored by rectangle index)
    std::vector<double> rects(F * N * PSL_LSD_RECT_F64, 0.0);
    std::vector<int2> cnt(F * N * TR, make_int2(-1, 0));
    std::vector<uint16_t> ulist(F * N, 0);
    for (size_t f = 0; f < F; ++f)
        for (int r = 0; r < nrect[f]; ++r) {
            const size_t o = f * N + r, s = f * rect_cap + r;
            rects[o * PSL_LSD_RECT_F64 + 9] = p_lognfa[s * 2];
            rects[o * PSL_LSD_RECT_F64 + 10] = p_lognfa[s * 2 + 1];
            for (int t = 0; t < TR; ++t) cnt[o * TR + t] = make_int2(nk[(s * 5 + t) * 2], nk[(s * 5 + t) * 2 + 1]);
            ulist[f * N + r] = (uint16_t)(nrect[f] - 1 - r);
        }
    PSL_HIP(hipMemcpyAsync(line->d_rects, rects.data(), rects.size() * sizeof(double), hipMemcpyHostToDevice, st));
    PSL_HIP(hipMemcpyAsync(line->d_nrect, nrect, F * sizeof(int), hipMemcpyHostToDevice, st));
    PSL_HIP(hipMemcpyAsync(phase == PSL_NFA_FIRST ? line->d_count0 : line->d_counts, cnt.data(), cnt.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    uint16_t* d_ul = nullptr;
    int* d_uc = nullptr;
    if (phase != PSL_NFA_FIRST) {   // list phase + 1 of run_detect, at the place a launch of `nframes` frames keeps it
        d_ul = line->d_ulist + (size_t)((phase + 1) & 1) * N * F;
        d_uc = line->d_ucount + (size_t)(phase + 1) * F;
        PSL_HIP(hipMemcpyAsync(d_ul, ulist.data(), ulist.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        PSL_HIP(hipMemcpyAsync(d_uc, nrect, F * sizeof(int), hipMemcpyHostToDevice, st));
    }
#define PSL_NFA_DEBUG_EVAL(PH)                                                                                                                  \
    case PH:                                                                                                                                    \
        k_lsd_nfa_setup<PH><<<F, 256, 0, st>>>(P, line->NT, line->d_rects, line->d_nrect, d_ul, d_uc, line->d_counts, line->d_count0, line->d_vals, \
                                               line->d_sstate, line->d_stmp, line->d_slist, line->d_lcount);                                    \
        k_lsd_nfa_series<PH><<<dim3(PSL_NFA_NCLS, (F + PSL_NFA_FG - 1) / PSL_NFA_FG), 256, 0, st>>>(P, line->NT, (int)F, line->d_slist, line->d_lcount, \
                                                                                                    line->d_sstate);                            \
        break;
    switch (phase) {
        PSL_NFA_DEBUG_EVAL(PSL_NFA_FIRST)
        PSL_NFA_DEBUG_EVAL(-1)
        PSL_NFA_DEBUG_EVAL(0)
        PSL_NFA_DEBUG_EVAL(1)
        PSL_NFA_DEBUG_EVAL(2)
        PSL_NFA_DEBUG_EVAL(3)
    }
#undef PSL_NFA_DEBUG_EVAL
    PSL_HIP(hipGetLastError());
    std::vector<double> v(F * N * 5);
    std::vector<double2> ss(F * N * 5);
    PSL_HIP(hipMemcpyAsync(v.data(), line->d_vals, v.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(ss.data(), line->d_sstate, ss.size() * sizeof(double2), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    for (size_t f = 0; f < F; ++f)
        for (int r = 0; r < nrect[f]; ++r)
            for (int t = 0; t < TR; ++t) {
                vals[((size_t)f * rect_cap + r) * 5 + t] = v[(f * N + r) * 5 + t];
                tail[((size_t)f * rect_cap + r) * 5 + t] = ss[(f * N + r) * 5 + t].x;
            }
    if (log_nt) *log_nt = line->NT.log_nt;
    return PSLFE_OK;
}

// ---- full extractor ------------------------------------------------------------------------------
int pslfe_line_extract_batch_device(pslfe_line* line, const uint8_t* d_gray, int nframes, int w, int h, int stride, size_t frame_stride) {
    PSL_REQUIRE(line && d_gray, PSLFE_E_INVALID, "pslfe_line_extract_batch_device: NULL argument");
    PSL_REQUIRE(nframes >= 1 && nframes <= line->max_batch, PSLFE_E_INVALID, "pslfe_line_extract_batch_device: nframes %d (max_batch %d)", nframes, line->max_batch);
    PSL_REQUIRE(stride >= w && (nframes == 1 || frame_stride >= (size_t)stride * h), PSLFE_E_INVALID, "pslfe_line_extract_batch_device: strides");
    return line->run_extract(d_gray, nframes, w, h, stride, frame_stride);
}

int pslfe_line_results_device(pslfe_line* line, const PslKeyLine** d_kls, const uint8_t** d_desc, const double** d_lineEq,
                              const int32_t** d_counts, int* kl_cap) {
    PSL_REQUIRE(line, PSLFE_E_INVALID, "pslfe_line_results_device: line is NULL");
    PSL_REQUIRE(line->last_nframes > 0, PSLFE_E_STATE, "pslfe_line_results_device: no batch extracted yet");
    if (d_kls) *d_kls = line->d_kls;
    if (d_desc) *d_desc = line->d_ldesc;
    if (d_lineEq) *d_lineEq = line->d_lineEq;
    if (d_counts) *d_counts = line->d_nkl;
    if (kl_cap) *kl_cap = line->P.maxkl;
    return PSLFE_OK;
}

int pslfe_line_fetch(pslfe_line* line, int frame, PslKeyLine* kls, uint8_t* desc, double* lineEq, int cap, int* n, int* status) {
    PSL_REQUIRE(line && n, PSLFE_E_INVALID, "pslfe_line_fetch: NULL argument");
    PSL_REQUIRE(line->last_nframes > 0 && frame >= 0 && frame < line->last_nframes, PSLFE_E_STATE, "pslfe_line_fetch: frame %d", frame);
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    int cnt = 0, stt = 0;
    PSL_HIP(hipMemcpyAsync(&cnt, line->d_nkl + frame, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(&stt, line->d_status + frame, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *n = cnt;
    if (status) *status = stt;
    PSL_REQUIRE(cnt <= cap, PSLFE_E_CAPACITY, "pslfe_line_fetch: %d keylines, capacity %d", cnt, cap);
    if (cnt > 0) {
        const size_t o = (size_t)frame * line->P.maxkl;
        if (kls) PSL_HIP(hipMemcpyAsync(kls, line->d_kls + o, (size_t)cnt * sizeof(PslKeyLine), hipMemcpyDeviceToHost, st));
        if (desc) PSL_HIP(hipMemcpyAsync(desc, line->d_ldesc + o * 32, (size_t)cnt * 32, hipMemcpyDeviceToHost, st));
        if (lineEq) PSL_HIP(hipMemcpyAsync(lineEq, line->d_lineEq + o * 3, (size_t)cnt * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipStreamSynchronize(st));
    }
    return PSLFE_OK;
}

int pslfe_line_segments_fetch(pslfe_line* line, int frame, float* segments, int cap, int* n) {
    PSL_REQUIRE(line && n, PSLFE_E_INVALID, "pslfe_line_segments_fetch: NULL argument");
    PSL_REQUIRE(line->last_nframes > 0 && frame >= 0 && frame < line->last_nframes, PSLFE_E_STATE, "pslfe_line_segments_fetch: frame %d", frame);
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    int cnt = 0;
    PSL_HIP(hipMemcpyAsync(&cnt, line->d_nseg + frame, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *n = cnt;
    PSL_REQUIRE(cnt <= cap && cnt <= line->P.maxseg, PSLFE_E_CAPACITY, "pslfe_line_segments_fetch: %d segments, capacity %d (list %d)", cnt, cap,
                line->P.maxseg);
    if (cnt > 0 && segments) {
        PSL_HIP(hipMemcpyAsync(segments, line->d_seg + (size_t)frame * line->P.maxseg * 4, (size_t)cnt * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipStreamSynchronize(st));
    }
    return PSLFE_OK;
}

int pslfe_line_extract(pslfe_line* line, const uint8_t* gray, int w, int h, int stride, PslKeyLine* kls, uint8_t* desc, double* lineEq,
                       int cap, int* n) {
    PSL_REQUIRE(line && n, PSLFE_E_INVALID, "pslfe_line_extract: NULL argument");
    *n = 0;
    if (!gray || w <= 0 || h <= 0) return PSLFE_OK;  // add_src/LineExtractor.cpp:327: empty image -> silent return
    PSL_REQUIRE(stride >= w, PSLFE_E_INVALID, "pslfe_line_extract: stride %d < width %d", stride, w);
    int rc = line->upload(gray, 1, w, h, stride, (size_t)stride * h);
    if (rc) return rc;
    rc = pslfe_line_extract_batch_device(line, line->d_in, 1, w, h, line->in_pitch, line->in_fstride);
    if (rc) return rc;
    return pslfe_line_fetch(line, 0, kls, desc, lineEq, cap, n, nullptr);
}

// ---- stage entry points (also used by the parity tests) ---------------------------------------------
int pslfe_line_optimize_and_merge(pslfe_line* line, const float* segments, int nseg, int w, int h, PslKeyLine* kls, int cap, int* n) {
    PSL_REQUIRE(line && n && (nseg == 0 || segments), PSLFE_E_INVALID, "pslfe_line_optimize_and_merge: NULL argument");
    *n = 0;
    PSL_REQUIRE(nseg >= 0 && nseg <= PSL_MERGE_NMAX, PSLFE_E_CAPACITY, "pslfe_line_optimize_and_merge: %d segments (max %d)", nseg, PSL_MERGE_NMAX);
    int rc = line->prepare(w, h);
    if (rc) return rc;
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    if (nseg) PSL_HIP(hipMemcpyAsync(line->d_seg, segments, (size_t)nseg * 4 * sizeof(float), hipMemcpyHostToDevice, st));
    PSL_HIP(hipMemcpyAsync(line->d_nseg, &nseg, sizeof(int), hipMemcpyHostToDevice, st));
    PSL_HIP(hipStreamSynchronize(st));
    // the top-N cut belongs to LINEextractor::operator(); this entry point is optimizeAndMergeLines_lsd alone
    const int keep = line->P.nfeatures;
    line->P.nfeatures = line->P.maxkl;
    rc = line->run_merge(line->whole(1));
    line->P.nfeatures = keep;
    if (rc) return rc;
    line->last_nframes = 1;
    return pslfe_line_fetch(line, 0, kls, nullptr, nullptr, cap, n, nullptr);
}

int pslfe_lbd_compute(pslfe_line* line, const uint8_t* gray, int w, int h, int stride, const PslKeyLine* kls, int nkl, uint8_t* desc,
                      float* fdesc) {
    PSL_REQUIRE(line && gray && (nkl == 0 || (kls && desc)), PSLFE_E_INVALID, "pslfe_lbd_compute: NULL argument");
    if (nkl == 0) return PSLFE_OK;  // upstream prints "keypoint list is empty" and returns (binary_descriptor_custom.cpp:559-563)
    PSL_REQUIRE(stride >= w, PSLFE_E_INVALID, "pslfe_lbd_compute: stride %d < width %d", stride, w);
    int rc = line->upload(gray, 1, w, h, stride, (size_t)stride * h);
    if (rc) return rc;
    PSL_REQUIRE(nkl <= line->P.maxkl, PSLFE_E_CAPACITY, "pslfe_lbd_compute: %d keylines (max %d)", nkl, line->P.maxkl);
    hipStream_t st = line->ctx->stream;
    PSL_HIP(hipMemcpyAsync(line->d_kls, kls, (size_t)nkl * sizeof(PslKeyLine), hipMemcpyHostToDevice, st));
    PSL_HIP(hipMemcpyAsync(line->d_nkl, &nkl, sizeof(int), hipMemcpyHostToDevice, st));
    PSL_HIP(hipStreamSynchronize(st));
    line->kl_bound = std::max(line->kl_bound, nkl);
    const int keep = line->P.nfeatures;
    line->P.nfeatures = std::max(keep, nkl);
    rc = line->run_lbd(line->whole(1), line->d_in, line->in_pitch, line->in_fstride, fdesc != nullptr);
    line->P.nfeatures = keep;
    if (rc) return rc;
    PSL_HIP(hipMemcpyAsync(desc, line->d_ldesc, (size_t)nkl * 32, hipMemcpyDeviceToHost, st));
    if (fdesc) PSL_HIP(hipMemcpyAsync(fdesc, line->d_fdesc, (size_t)nkl * 72 * sizeof(float), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    line->last_nframes = 1;
    return PSLFE_OK;
}

int pslfe_line_debug_sobel(pslfe_line* line, int frame, int16_t* dx, int16_t* dy) {
    PSL_REQUIRE(line && dx && dy, PSLFE_E_INVALID, "pslfe_line_debug_sobel: NULL argument");
    PSL_REQUIRE(line->last_nframes > 0 && frame >= 0 && frame < line->last_nframes, PSLFE_E_STATE, "pslfe_line_debug_sobel: frame %d", frame);
    PSL_HIP(hipSetDevice(line->ctx->device));
    PSL_HIP(hipStreamSynchronize(line->ctx->stream));
    const size_t npx = (size_t)line->P.w * line->P.h;
    std::vector<short2> tmp(npx);
    PSL_HIP(hipMemcpy(tmp.data(), line->d_dxy + frame * npx, npx * sizeof(short2), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < npx; ++i) { dx[i] = tmp[i].x; dy[i] = tmp[i].y; }
    return PSLFE_OK;
}

// == CPartiallyRecoverConnectivity(mLines, radius, fans, img, fanThr): host matrix in, fans rows out
int pslfe_lil_pair(pslfe_line* line, const float* lines, int nlines, float radius, float fanThr, int imgCols, int imgRows, float* fans,
                   int cap, int* nfans) {
    PSL_REQUIRE(line && nfans && (nlines == 0 || lines), PSLFE_E_INVALID, "pslfe_lil_pair: NULL argument");
    *nfans = 0;
    if (nlines == 0) return PSLFE_OK;
    PSL_REQUIRE(nlines <= PSL_MERGE_NMAX, PSLFE_E_CAPACITY, "pslfe_lil_pair: %d lines (max %d)", nlines, PSL_MERGE_NMAX);
    int rc = line->prepare(line->gw > 0 ? line->gw : std::max(imgCols, 16), line->gh > 0 ? line->gh : std::max(imgRows, 16));
    if (rc) return rc;
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    PSL_HIP(hipMemcpyAsync(line->d_tmplines, lines, (size_t)nlines * 4 * sizeof(float), hipMemcpyHostToDevice, st));
    PSL_HIP(hipStreamSynchronize(st));
    {
        PSL_STAGE_BEGIN(line->ctx, "line.pair");
        (nlines <= PSL_PAIR_LDSN ? k_lil_pair : k_lil_pair_big)<<<1, 256, 0, st>>>(line->d_tmplines, 0, 4, nullptr, nlines, radius, fanThr, imgCols, imgRows,
                                                                                   line->d_rawfans, line->d_fans, PSL_FAN_CAP, line->d_nfans);
        PSL_STAGE_END(line->ctx, "line.pair");
    }
    PSL_HIP(hipGetLastError());
    int k = 0;
    PSL_HIP(hipMemcpyAsync(&k, line->d_nfans, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *nfans = k;
    PSL_REQUIRE(k <= cap, PSLFE_E_CAPACITY, "pslfe_lil_pair: %d fans, capacity %d", k, cap);
    if (k > 0 && fans) {
        PSL_HIP(hipMemcpyAsync(fans, line->d_fans, (size_t)k * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipStreamSynchronize(st));
    }
    return PSLFE_OK;
}

// Pairing of every frame of the last extracted batch, HBM resident (mLines = keyline endpoints, src/Frame.cc:504-505)
int pslfe_line_pair_batch_device(pslfe_line* line, float radius, float fanThr) {
    PSL_REQUIRE(line, PSLFE_E_INVALID, "pslfe_line_pair_batch_device: line is NULL");
    PSL_REQUIRE(line->last_nframes > 0, PSLFE_E_STATE, "pslfe_line_pair_batch_device: no batch extracted yet");
    return line->run_pair(line->last_nframes, radius, fanThr);
}

int pslfe_line_fans_device(pslfe_line* line, const float** d_fans, const int32_t** d_nfans, int* fan_stride) {
    PSL_REQUIRE(line, PSLFE_E_INVALID, "pslfe_line_fans_device: line is NULL");
    PSL_REQUIRE(line->last_nframes > 0, PSLFE_E_STATE, "pslfe_line_fans_device: no batch extracted yet");
    if (d_fans) *d_fans = line->d_fans;
    if (d_nfans) *d_nfans = line->d_nfans;
    if (fan_stride) *fan_stride = PSL_FAN_CAP;
    return PSLFE_OK;
}

int pslfe_line_fans_fetch(pslfe_line* line, int frame, float* fans, int cap, int* nfans) {
    PSL_REQUIRE(line && nfans, PSLFE_E_INVALID, "pslfe_line_fans_fetch: NULL argument");
    PSL_REQUIRE(line->last_nframes > 0 && frame >= 0 && frame < line->last_nframes, PSLFE_E_STATE, "pslfe_line_fans_fetch: frame %d", frame);
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    int k = 0;
    PSL_HIP(hipMemcpyAsync(&k, line->d_nfans + frame, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *nfans = k;
    PSL_REQUIRE(k <= cap, PSLFE_E_CAPACITY, "pslfe_line_fans_fetch: %d fans, capacity %d", k, cap);
    if (k > 0 && fans) {
        PSL_HIP(hipMemcpyAsync(fans, line->d_fans + (size_t)frame * PSL_FAN_CAP * 4, (size_t)k * 4 * sizeof(float), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipStreamSynchronize(st));
    }
    return PSLFE_OK;
}


// == lmatcher.match(mLastFrame.mLdesc, mCurrentFrame.mLdesc, nnr, matches_12) (src/Tracking.cc:901 ->
//    LSDmatcher::match -> matchNNR, add_src/LSDmatcher.cpp:354-413) for every frame f of the last batch
//    against frame (f - shift) mod nframes; HBM resident.  d_matches12: [nframes][cap] (row f indexed by the
//    LAST frame's line, value = index into frame f's lines or -1), d_nmatches: [nframes].
int pslfe_line_match_batch_device(pslfe_line* line, int shift, float nnr, int32_t* d_matches12, int32_t* d_nmatches) {
    PSL_REQUIRE(line && d_matches12 && d_nmatches, PSLFE_E_INVALID, "pslfe_line_match_batch_device: NULL argument");
    PSL_REQUIRE(line->last_nframes > 0, PSLFE_E_STATE, "pslfe_line_match_batch_device: no batch extracted yet");
    PSL_HIP(hipSetDevice(line->ctx->device));
    hipStream_t st = line->ctx->stream;
    const int F = line->last_nframes, cap = line->P.maxkl;
    PSL_HIP(hipMemsetAsync(d_nmatches, 0, (size_t)F * sizeof(int), st));
    {
        PSL_STAGE_BEGIN(line->ctx, "line.match");
        const int qmax = std::min(cap, line->P.nfeatures);
        k_line_match_batch<<<dim3(F, (qmax + 3) / 4), 256, 0, st>>>(line->d_ldesc, line->d_nkl, cap, F, shift, nnr, d_matches12, d_nmatches);
        PSL_STAGE_END(line->ctx, "line.match");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // extern "C"
