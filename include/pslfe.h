/* pslfe — MI355X-native per-frame feature front-end for PSL-SLAM: the C ABI.
 *
 * This is the drop-in boundary.  The reference has no FFI: its seams are plain
 * C++ calls on objects owned by Tracking (ORBextractor::operator(), LINEextractor::operator(),
 * CPartiallyRecoverConnectivity, ORBmatcher / LSDmatcher methods).  Each entry point below names
 * the reference interface it replaces (file:line under the reference tree).  A C++ shim that
 * mirrors those classes over this ABI is in psl-slam_amd/host/pslfe.hpp; the patch a PSL-SLAM
 * maintainer applies is in INTEGRATION.md.
 *
 * Conventions: plain pointers and sizes only; every function returns PSLFE_OK (0) or a negative
 * PSLFE_E_* code and never throws; the caller allocates outputs with a capacity and the callee
 * reports counts; structs are POD with the exact layout of the OpenCV types the reference uses
 * (cv::KeyPoint 28 B, line_descriptor::KeyLine 68 B); one context per GPU; calls on one handle are
 * serialised by the caller (the reference has a single Tracking thread), different handles may be
 * used from different threads.  "d_" arguments are device (HBM) pointers, all others are host.
 * The library needs a gfx950 GPU: there is no CPU fallback, ctx creation fails without one.
 */
#ifndef PSLFE_H
#define PSLFE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSLFE_OK 0
#define PSLFE_E_INVALID (-1)   /* bad argument (null, size, unsupported configuration)        */
#define PSLFE_E_NODEVICE (-2)  /* no usable gfx950 device / HIP runtime error at start-up     */
#define PSLFE_E_HIP (-3)       /* HIP runtime error; text in pslfe_last_error()               */
#define PSLFE_E_CAPACITY (-4)  /* caller-provided capacity too small                          */
#define PSLFE_E_STATE (-5)     /* call order (e.g. fetch before extract)                      */

#define PSLFE_MAX_LEVELS 16
#define PSLFE_FAN_CAP 4096   /* fans rows per frame of the line pairing (pslfe_line_fans_device's fan_stride) */

/* == cv::KeyPoint as filled by ORBextractor (src/ORBextractor.cc:837-847, 1095-1103). */
typedef struct PslKeyPoint {
    float x, y;      /* pt, level-0 pixel coordinates (pt *= mvScaleFactor[octave])            */
    float size;      /* (int)(31 * mvScaleFactor[octave])                                      */
    float angle;     /* IC_Angle, degrees in [0,360)                                            */
    float response;  /* FAST corner score (not Harris: include/ORBextractor.h:49 is unused)    */
    int32_t octave;
    int32_t class_id; /* -1 */
} PslKeyPoint;

/* == cv::line_descriptor::KeyLine, field order of
 * Thirdparty/line_descriptor/include/line_descriptor/descriptor_custom.hpp:107-146. */
typedef struct PslKeyLine {
    float angle;
    int32_t class_id;
    int32_t octave;
    float pt_x, pt_y;
    float response;
    float size;
    float startPointX, startPointY, endPointX, endPointY;
    float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
    float lineLength;
    int32_t numOfPixels;
} PslKeyLine;

typedef struct pslfe_ctx pslfe_ctx;   /* one per GPU                                           */
typedef struct pslfe_orb pslfe_orb;   /* == ORBextractor object                                 */

const char* pslfe_version(void);
/* Last error text of this thread (empty string if none). */
const char* pslfe_last_error(void);

/* ---- context ------------------------------------------------------------------------------- */
int pslfe_ctx_create(int device, pslfe_ctx** out);
void pslfe_ctx_destroy(pslfe_ctx* ctx);
/* Run all work of this context on an existing HIP stream (hipStream_t passed as void*), e.g. the
 * caller framework's current stream; NULL = the context's own stream. */
int pslfe_ctx_set_stream(pslfe_ctx* ctx, void* hip_stream);
int pslfe_ctx_synchronize(pslfe_ctx* ctx);
/* Per-stage device timing with HIP events on the launch stream (for bench/roofline).
 * enable != 0 starts collecting; pslfe_ctx_stage_time returns accumulated milliseconds and the
 * number of launches of a stage name ("orb.pyramid", "orb.fast", "orb.octree", "orb.blur",
 * "orb.describe", "match.window", "match.knn2", ...) and resets nothing. */
int pslfe_ctx_profile(pslfe_ctx* ctx, int enable);
/* Restrict the timing to one stage (NULL or "" = all stages).  Every timed stage puts two event records
 * between kernels (~10 us of idle GPU each on MI355X); timing only the stage of interest keeps a
 * throughput measurement undisturbed. */
int pslfe_ctx_profile_only(pslfe_ctx* ctx, const char* stage);
int pslfe_ctx_profile_reset(pslfe_ctx* ctx);
int pslfe_ctx_stage_time(pslfe_ctx* ctx, const char* stage, double* ms_total, int* launches);

/* Plain HBM helpers for callers without their own device allocator (synchronous copies). */
int pslfe_device_alloc(pslfe_ctx* ctx, size_t bytes, void** d_ptr);
int pslfe_device_free(pslfe_ctx* ctx, void* d_ptr);
int pslfe_device_upload(pslfe_ctx* ctx, void* d_dst, const void* src, size_t bytes);
int pslfe_device_download(pslfe_ctx* ctx, void* dst, const void* d_src, size_t bytes);

/* ---- input conversions (Tracking::GrabImageRGBD src/Tracking.cc:214-240) --------------------- */
/* == cvtColor(im, gray, CV_RGB2GRAY | CV_BGR2GRAY) src/Tracking.cc:219-232 on 8UC3 frames (the 4-channel
 *    variants :226-231 drop alpha first and are the same arithmetic).  is_rgb: mbRGB.  Frame f at
 *    d_rgb + f*frame_stride, rows `stride` bytes apart; d_gray packed [nframes][h][w]. Asynchronous. */
int pslfe_rgb_to_gray_device(pslfe_ctx* ctx, const uint8_t* d_rgb, int nframes, int w, int h, int stride,
                             size_t frame_stride, int is_rgb, uint8_t* d_gray);
int pslfe_rgb_to_gray(pslfe_ctx* ctx, const uint8_t* rgb, int w, int h, int stride, int is_rgb, uint8_t* gray);
/* == imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor) src/Tracking.cc:234-235 on CV_16U depth. */
int pslfe_depth_to_float_device(pslfe_ctx* ctx, const uint16_t* d_depth, size_t n, float factor, float* d_out);
int pslfe_depth_to_float(pslfe_ctx* ctx, const uint16_t* depth, size_t n, float factor, float* out);

/* ---- ORB extractor -------------------------------------------------------------------------- */
/* == ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 *    src/ORBextractor.cc:410-470; object created once in Tracking (src/Tracking.cc:120).
 *    max_batch = most frames one batched call will carry (>=1). */
int pslfe_orb_create(pslfe_ctx* ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                     int minThFAST, int max_batch, pslfe_orb** out);
void pslfe_orb_destroy(pslfe_orb* orb);

/* == GetLevels/GetScaleFactor/GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/
 *    GetInverseScaleSigmaSquares, include/ORBextractor.h:63-84 (read by Frame ctor src/Frame.cc:141-148).
 *    Arrays hold nlevels floats. */
int pslfe_orb_levels(const pslfe_orb* orb);
float pslfe_orb_scale_factor(const pslfe_orb* orb);
int pslfe_orb_scale_factors(const pslfe_orb* orb, float* scale, float* inv_scale, float* sigma2,
                            float* inv_sigma2);
/* mnFeaturesPerLevel (src/ORBextractor.cc:435-446), nlevels ints. */
int pslfe_orb_features_per_level(const pslfe_orb* orb, int* quota);
/* Upper bound on keypoints one frame can return for a w x h image (quota + octree overshoot). */
int pslfe_orb_max_keypoints(pslfe_orb* orb, int w, int h);

/* == ORBextractor::operator()(image, mask, keypoints, descriptors)
 *    include/ORBextractor.h:59-61, src/ORBextractor.cc:1043-1105; called from Frame::ExtractORB
 *    src/Frame.cc:311-317.  One 8UC1 host image in, host outputs; synchronous.
 *    gray==NULL or w/h<=0 -> PSLFE_OK with *n = 0 (reference returns silently, :1046).
 *    desc: n x 32 bytes row-major.  cap = capacity of kps/desc in keypoints. */
int pslfe_orb_extract(pslfe_orb* orb, const uint8_t* gray, int w, int h, int stride,
                      PslKeyPoint* kps, uint8_t* desc, int cap, int* n);

/* Batched many-frames mode (north_star): nframes independent 8UC1 frames already resident in HBM,
 * frame f at d_gray + f*frame_stride, rows `stride` bytes apart.  Asynchronous on the context's
 * stream; results stay in the handle's HBM buffers until the next call. */
int pslfe_orb_extract_batch_device(pslfe_orb* orb, const uint8_t* d_gray, int nframes, int w, int h,
                                   int stride, size_t frame_stride);
/* Device views of the last batch's results: keypoints [nframes][cap] PslKeyPoint, descriptors
 * [nframes][cap][32] u8, counts [nframes] int32; cap = *kp_cap. Valid until the next extract. */
int pslfe_orb_results_device(pslfe_orb* orb, const PslKeyPoint** d_kps, const uint8_t** d_desc,
                             const int32_t** d_counts, int* kp_cap);
/* Copy frame `frame` of the last batch to the host (synchronises the stream). */
int pslfe_orb_fetch(pslfe_orb* orb, int frame, PslKeyPoint* kps, uint8_t* desc, int cap, int* n);
/* Host-buffer convenience: H2D + batch extract + D2H of everything.  kps [nframes][cap],
 * desc [nframes][cap][32], counts [nframes]. */
int pslfe_orb_extract_batch(pslfe_orb* orb, const uint8_t* gray, int nframes, int w, int h, int stride,
                            size_t frame_stride, PslKeyPoint* kps, uint8_t* desc, int cap, int32_t* counts);

/* Stage taps of the last batch, for parity tests against the oracle (host outputs, synchronous):
 *  level image (blurred = 0: pyramid level == mvImagePyramid[level] ROI; 1: the 7x7 sigma-2 blur),
 *  FAST candidates of a level in reference order (x, y relative to minBorder, score) == the
 *  vToDistributeKeys of src/ORBextractor.cc:779-829, and keypoints after DistributeOctTree. */
int pslfe_orb_debug_level_size(pslfe_orb* orb, int level, int* w, int* h);
int pslfe_orb_debug_level_image(pslfe_orb* orb, int frame, int level, int blurred, uint8_t* out, int out_stride);
int pslfe_orb_debug_candidates(pslfe_orb* orb, int frame, int level, int32_t* xys, int cap, int* n);
int pslfe_orb_debug_level_keypoints(pslfe_orb* orb, int frame, int level, int32_t* xys, int cap, int* n);
/* The way in for hand-made keypoints (tests/stereo_cases.py): after an extraction, the n host keypoints and descriptors
 * (n x 32 bytes) replace the results and the count of frame `frame` of the last batch; the pyramid stays as extracted.  The copy
 * is ordered on the context's stream (work queued before it reads the old arrays, work queued after it the new ones) and has
 * completed on return.  pslfe_orb_fetch, pslfe_orb_results_device and every consumer of the handle (pslfe_frame_set_from_orb*)
 * then see the new arrays, until the next extraction.  Nothing is checked about the keypoints themselves: the consumer's own
 * conventions for octaves and coordinates apply.  PSLFE_E_STATE before any extraction; PSLFE_E_INVALID for a NULL argument, a
 * frame outside the last batch or n < 0; PSLFE_E_CAPACITY for n > pslfe_orb_max_keypoints.  Nothing calls it at run time. */
int pslfe_orb_debug_set_results(pslfe_orb* orb, int frame, const PslKeyPoint* kps, const uint8_t* desc, int n);

/* ---- line extractor ---------------------------------------------------------------------------- */
typedef struct pslfe_line pslfe_line;  /* == LINEextractor object                                  */

/* == LINEextractor::LINEextractor(numOctaves, scale, nLSDFeature, min_line_length)
 *    add_src/LineExtractor.cpp:6-25; object created once in Tracking (src/Tracking.cc:127).
 *    numOctaves must be 1 (PSLFE_E_INVALID otherwise): every reference YAML sets LINEextractor.nLevels: 1, and the
 *    contrib detect() call truncates scale 1.2 to int 1 (add_src/LineExtractor.cpp:336-337), with which the stock
 *    LSDDetector's pyramid for numOctaves > 1 is pyrDown(m, m, Size(cols / 1, rows / 1)) - rejected by pyrDown's size
 *    assertion: the reference's own call throws there, it does not yield lines. */
int pslfe_line_create(pslfe_ctx* ctx, int numOctaves, float scale, int nLSDFeature, double min_line_length,
                      int max_batch, pslfe_line** out);
void pslfe_line_destroy(pslfe_line* line);
/* Refinement mode of the LSD behind the extractor (cv::createLineSegmentDetector(refine), OpenCV 3.x lsd.cpp).  The
 * reference calls the STOCK contrib cv::line_descriptor::LSDDetector (add_src/LineExtractor.cpp:336-337, linked by
 * CMakeLists.txt:96), whose source is not in its tree: upstream constructs the detector with LSD_REFINE_ADV
 * (rect_improve + NFA test, log_eps 0), which is the default here; the vendored, never-called LSDDetectorC
 * (Thirdparty/line_descriptor/src/LSDDetector_custom.cpp:185) uses LSD_REFINE_STD (no NFA test). */
#define PSLFE_LSD_REFINE_STD 1
#define PSLFE_LSD_REFINE_ADV 2
int pslfe_line_set_refine(pslfe_line* line, int refine);
/* == GetLevels / GetScaleFactor / GetScaleFactors ... add_inc/LineExtractor.h:211-233 */
int pslfe_line_levels(const pslfe_line* line);
float pslfe_line_scale_factor(const pslfe_line* line);
int pslfe_line_scale_factors(const pslfe_line* line, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);

/* == line_descriptor::LSDDetector::detect(image, keylines, scale=1, numOctaves=1) up to the segment
 *    list: cv::createLineSegmentDetector() defaults + checkLineExtremes
 *    (Thirdparty/line_descriptor/src/LSDDetector_custom.cpp:166-205). segments: n x (x1,y1,x2,y2). */
int pslfe_lsd_detect(pslfe_line* line, const uint8_t* gray, int w, int h, int stride, float* segments, int cap, int* n);
/* Tap for parity tests: LSD working image (f64), level-line angle in degrees (f32, -1024 = NOTDEF;
 * the reference's double angle is exactly (double)deg * CV_PI/180) and gradient norm (f64). */
int pslfe_line_debug_gradient(pslfe_line* line, int frame, int* W, int* H, double* scaled, float* angle_deg, double* modgrad);
/* Tap for parity tests: the kernels' restated libm, evaluated on the device.  One thread per element computes function `fn` of
 * a[i] (and b[i] for the two-argument functions) into out0[i] (and out1[i] for the two-output ones); all four are HOST arrays of
 * n elements.  The file is built with the flags of every kernel file, so the result is what a product kernel computes for that
 * argument.  f32 in -> f32 out unless noted; f64 in -> f64 out unless noted.  Unknown fn, a NULL ctx or a NULL array the function
 * uses: PSLFE_E_INVALID.  n == 0: PSLFE_OK.  Synchronous. */
#define PSLFE_MATH_ATANF 0            /* psl_atanf(a)                                          */
#define PSLFE_MATH_TANF 1             /* psl_tanf(a)                                           */
#define PSLFE_MATH_SINCOSF 2          /* psl_sincosf(a): out0 = sin, out1 = cos                */
#define PSLFE_MATH_FAST_ATAN2 3       /* psl_fast_atan2(y = a, x = b)                          */
#define PSLFE_MATH_ATAN2F 4           /* psl_atan2f(y = a, x = b)                              */
#define PSLFE_MATH_FDIV 5             /* PSL_FDIV(a, b)                                        */
#define PSLFE_MATH_SQRTF 6            /* __builtin_sqrtf(a)                                    */
#define PSLFE_MATH_CVROUND_F 7        /* psl_cvround_f(a): out0 int32                          */
#define PSLFE_MATH_LOG 8              /* psl_log(a)                                            */
#define PSLFE_MATH_EXP 9              /* psl_exp(a)                                            */
#define PSLFE_MATH_LOG10 10           /* psl_log10(a)                                          */
#define PSLFE_MATH_POW_POS 11         /* psl_pow_pos(a, b)                                     */
#define PSLFE_MATH_SINH_SMALL 12      /* psl_sinh_small(a)                                     */
#define PSLFE_MATH_LOG_GAMMA 13       /* lsdn_log_gamma(a)                                     */
#define PSLFE_MATH_GLIBC_SIN 14       /* psl_glibc_sin(a, table)                               */
#define PSLFE_MATH_GLIBC_COS 15       /* psl_glibc_cos(a, table)                               */
#define PSLFE_MATH_COS_SIN_F64 16     /* psl_cos_sin_f64(a): out0 = cos, out1 = sin            */
#define PSLFE_MATH_COS_SIN_2PI_F32 17 /* psl_cos_sin_2pi_f32(a): out0 = cos, out1 = sin, float */
#define PSLFE_MATH_RATIO_INV 18       /* psl_ratio_inv(a, b, 1.0 / b)                          */
#define PSLFE_MATH_DDIV 19            /* a / b                                                 */
#define PSLFE_MATH_DSQRT 20           /* sqrt(a)                                               */
#define PSLFE_MATH_CVROUND_D 21       /* psl_cvround_d(a): out0 int32                          */
#define PSLFE_MATH_COUNT 22
int pslfe_debug_math(pslfe_ctx* ctx, int fn, size_t n, const void* a, const void* b, void* out0, void* out1);
/* Tap for parity tests: nfa(n, k, p) of LSD_REFINE_ADV exactly as an extraction evaluates it - the product's k_lsd_nfa_setup<phase>
 * and k_lsd_nfa_series<phase>, with run_detect's grids, on caller-supplied trials instead of rectangles counted in an image.
 *   w, h       frame size: the geometry is prepared as an extraction of w x h frames prepares it (logNT, the tables);
 *   phase      PSLFE_NFA_FIRST (the first test: one trial per rectangle) or -1 .. 3 (five trials per rectangle; in phases -1 and 3
 *              trial t is evaluated at p / 2^(t+1));
 *   nframes    1 .. max_batch; nrect[f] = rectangles of frame f, 0 .. rect_cap (rect_cap <= the extractor's segment capacity, 4096);
 *   p_lognfa   [nframes][rect_cap][2]: per rectangle its p and the log_nfa it brings into the phase;
 *   nk         [nframes][rect_cap][5][2] int32: (n, k) per trial (the first test reads trial 0 only); n < 0 = a trial the width
 *              guard excludes;
 *   vals, tail [nframes][rect_cap][5] doubles: the value k_lsd_nfa_setup left and sstate[].x after k_lsd_nfa_series - the binomial
 *              tail, 0 where no series was summed (the value is then in vals), +inf where the series ended at its `stop`;
 *   log_nt     the logNT used (may be NULL).
 * Rows beyond nrect[f] and, for the first test, trials 1 .. 4 are not written.  OVERWRITES the rectangle and NFA buffers of the
 * last extraction: fetch its results first.  Synchronous. */
#define PSLFE_NFA_FIRST (-2)
int pslfe_line_debug_nfa(pslfe_line* line, int w, int h, int phase, int nframes, const int32_t* nrect, int rect_cap,
                         const double* p_lognfa, const int32_t* nk, double* vals, double* tail, double* log_nt);

/* == LINEextractor::operator()(image, mask, keylines, descriptors, lineVec2d)
 *    add_inc/LineExtractor.h:167, add_src/LineExtractor.cpp:325-366; called from Frame::ExtractLSD
 *    src/Frame.cc:494.  LSD -> optimizeAndMergeLines_lsd -> top nLSDFeature by response -> LBD -> 2-D
 *    line equations.  desc: n x 32 bytes; lineEq: n x 3 doubles (sp x ep normalised by |xy|).
 *    gray == NULL or w/h <= 0 -> PSLFE_OK with *n = 0 (:327).  mask is not part of the ABI: the
 *    reference always passes an empty one (src/Frame.cc:493-494). */
int pslfe_line_extract(pslfe_line* line, const uint8_t* gray, int w, int h, int stride, PslKeyLine* kls, uint8_t* desc,
                       double* lineEq, int cap, int* n);
/* Batched many-frames mode, HBM resident, asynchronous on the context's stream. */
int pslfe_line_extract_batch_device(pslfe_line* line, const uint8_t* d_gray, int nframes, int w, int h, int stride,
                                    size_t frame_stride);
/* Device views: keylines [nframes][cap], descriptors [nframes][cap][32], line equations
 * [nframes][cap][3] f64, counts [nframes]. */
int pslfe_line_results_device(pslfe_line* line, const PslKeyLine** d_kls, const uint8_t** d_desc, const double** d_lineEq,
                              const int32_t** d_counts, int* kl_cap);
/* Copy one frame of the last batch to the host. *status (may be NULL): 0, or bit 1 = more raw segments
 * than the merge stage holds, bit 2 = cluster list overflow, bit 4 = more merged lines than cap. */
int pslfe_line_fetch(pslfe_line* line, int frame, PslKeyLine* kls, uint8_t* desc, double* lineEq, int cap, int* n, int* status);
/* The LSD segment list (x1, y1, x2, y2 rows, what pslfe_lsd_detect returns for one image) of one frame of the last batch:
 * *n = its length, at most cap rows copied (PSLFE_E_CAPACITY beyond). */
int pslfe_line_segments_fetch(pslfe_line* line, int frame, float* segments, int cap, int* n);

/* == optimizeAndMergeLines_lsd(keylines, img) add_src/uselongline.cpp:449-485 on a segment list
 *    (MergeLines 0.05/5/15 -> drop < 30 px -> MergeLines 0.03/3/30 -> drop < 50 px -> KeyLines). */
int pslfe_line_optimize_and_merge(pslfe_line* line, const float* segments, int nseg, int w, int h, PslKeyLine* kls, int cap, int* n);
/* == BinaryDescriptor::compute(image, keylines, descriptors) for given keylines
 *    (Thirdparty/line_descriptor/src/binary_descriptor_custom.cpp:540-688, 1027-1373). fdesc (may be
 *    NULL): the 72-float LBD vectors before binarisation, n x 72. */
int pslfe_lbd_compute(pslfe_line* line, const uint8_t* gray, int w, int h, int stride, const PslKeyLine* kls, int nkl,
                      uint8_t* desc, float* fdesc);
/* Tap: Sobel dx, dy (s16, w x h) of the LBD pre-processing of the last call. */
int pslfe_line_debug_sobel(pslfe_line* line, int frame, int16_t* dx, int16_t* dy);

/* == CPartiallyRecoverConnectivity(mLines, radius, fans, img, fanThr)
 *    add_inc/PartiallyRecoverConnectivity.h:13, add_src/PartiallyRecoverConnectivity.cpp:14-133; called
 *    from Frame::ExtractLSD src/Frame.cc:505 with radius = 20, fanThr = pi/4.  lines: n x 4
 *    (x1,y1,x2,y2); fans: k x 4 rows (x, y, i, j) after the keep-last de-duplication. */
int pslfe_lil_pair(pslfe_line* line, const float* lines, int nlines, float radius, float fanThr, int imgCols, int imgRows,
                   float* fans, int cap, int* nfans);
/* The same for every frame of the last extracted batch (mLines = keyline end points), HBM resident. */
int pslfe_line_pair_batch_device(pslfe_line* line, float radius, float fanThr);
int pslfe_line_fans_fetch(pslfe_line* line, int frame, float* fans, int cap, int* nfans);
/* Device views of the fans of the last pslfe_line_pair_batch_device: [nframes][fan_stride][4] float, counts [nframes]. */
int pslfe_line_fans_device(pslfe_line* line, const float** d_fans, const int32_t** d_nfans, int* fan_stride);

/* == lmatcher.match(mLastFrame.mLdesc, mCurrentFrame.mLdesc, nnr, matches_12) of src/Tracking.cc:901
 *    (LSDmatcher::match -> matchNNR, add_src/LSDmatcher.cpp:354-413) for every frame f of the last
 *    extracted batch against frame (f - shift) mod nframes, HBM resident, asynchronous.
 *    d_matches12: [nframes][kl_cap] int32, row f indexed by the LAST frame's line; d_nmatches: [nframes]. */
int pslfe_line_match_batch_device(pslfe_line* line, int shift, float nnr, int32_t* d_matches12, int32_t* d_nmatches);

/* ---- descriptor matching --------------------------------------------------------------------- */
/* == cv::BFMatcher(NORM_HAMMING).knnMatch(q, t, k=2) as used by LSDmatcher::matchNNR
 *    add_src/LSDmatcher.cpp:354-376 and FrameBFMatch :492-516.  256-bit descriptors, row-major
 *    32 B.  For query i: idx[2i], idx[2i+1] = best and second-best train rows (lower train index
 *    first on equal distance), dist[...] the Hamming distances; -1 / 0x7fffffff where nt < k. */
int pslfe_hamming_knn2(pslfe_ctx* ctx, const uint8_t* q, int nq, const uint8_t* t, int nt,
                       int32_t* idx, int32_t* dist);
/* Same on HBM-resident descriptors, asynchronous on the context's stream. */
int pslfe_hamming_knn2_device(pslfe_ctx* ctx, const uint8_t* d_q, int nq, const uint8_t* d_t, int nt,
                              int32_t* d_idx, int32_t* d_dist);

/* One projected query of ORBmatcher::SearchByProjection (src/ORBmatcher.cc:1328-1470 and :45-129):
 * what the host-side Tracking code knows about a map point before the window search. */
typedef struct PslProjQuery {
    float u, v;          /* projection into the current frame                                   */
    float radius;        /* th * mvScaleFactors[octave] (:1381) or r * scale (:66)               */
    float ur;            /* expected right coordinate u - mbf*invz (:1415) / mTrackProjXR (:92)  */
    int32_t min_level;   /* GetFeaturesInArea level band (:1385-1390, :66)                       */
    int32_t max_level;
    float angle;         /* LastFrame.mvKeysUn[i].angle, for the rotation histogram (:1433)      */
    int32_t blocks;      /* != 0: the map point has Observations()>0, so a keypoint it takes is
                            skipped by later queries (:1401-1403)                                */
} PslProjQuery;

typedef struct pslfe_frame pslfe_frame;  /* keypoints of up to max_frames frames, each bucketed on
                                             the 64x48 grid of include/Frame.h:45-46            */

/* == Frame::AssignFeaturesToGrid src/Frame.cc:269-284 + PosInGrid :1040-1050 for the keypoints of
 *    one frame, stored in `slot` (0 <= slot < max_frames).  Coordinates are the undistorted ones
 *    (mvKeysUn; PSL-SLAM's RGB-D YAMLs have zero distortion, so these are the extractor outputs).
 *    min_x..max_y = mnMinX..mnMaxY (src/Frame.cc:1135-1168).  uright: mvuRight or NULL (= all -1). */
int pslfe_frame_create(pslfe_ctx* ctx, int max_keypoints, int max_frames, pslfe_frame** out);
void pslfe_frame_destroy(pslfe_frame* f);
int pslfe_frame_set(pslfe_frame* f, int slot, const PslKeyPoint* kps, const uint8_t* desc, const float* uright,
                    int n, float min_x, float min_y, float max_x, float max_y);
/* All frames of the last batch of `orb` -> slots 0..nframes-1, HBM to HBM, asynchronous. */
int pslfe_frame_set_from_orb(pslfe_frame* f, pslfe_orb* orb, float min_x, float min_y, float max_x, float max_y);
/* Pinhole + radial-tangential camera of the settings YAML (Examples/RGB-D/TUM1.yaml; src/Tracking.cc:62-94):
 * mK entries, mDistCoef (k1 k2 p1 p2 k3) and mbf, all as the reference stores them (float). */
typedef struct PslCamera {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3;
    float bf;
} PslCamera;

/* == Frame::ComputeImageBounds src/Frame.cc:1135-1168: bounds = {mnMinX, mnMinY, mnMaxX, mnMaxY}
 *    (the argument order of pslfe_frame_set). */
int pslfe_image_bounds(pslfe_frame* f, const PslCamera* cam, int cols, int rows, float* bounds);

/* == The RGB-D part of the Frame constructor (src/Frame.cc:105-171) for one frame: UndistortKeyPoints
 *    :1062-1092 (cv::undistortPoints with P = K, skipped when k1 == 0 exactly as the reference does),
 *    ComputeStereoFromRGBD :1342-1363 (depth sampled at the DISTORTED keypoint, truncated to integer
 *    pixel; mvuRight = xUn - mbf/d, both -1 where d <= 0), ComputeImageBounds (first-frame statics) and
 *    AssignFeaturesToGrid on the undistorted points.  depth: CV_32F image (metres), host memory,
 *    depth_stride in floats.  The slot then holds mvKeysUn / mvuRight / mvDepth (pslfe_frame_fetch). */
int pslfe_frame_set_rgbd(pslfe_frame* f, int slot, const PslKeyPoint* kps, const uint8_t* desc, int n, const float* depth,
                         int width, int height, int depth_stride, const PslCamera* cam);
/* Same for every frame of the last batch of `orb` (slots 0..nframes-1), HBM to HBM, asynchronous.
 * d_depth: [nframes][height][width] float in HBM. */
int pslfe_frame_set_from_orb_rgbd(pslfe_frame* f, pslfe_orb* orb, const float* d_depth, int width, int height,
                                  const PslCamera* cam);
/* == The stereo Frame constructor src/Frame.cc:75-131 for nframes rectified pairs: Frame::ComputeStereoMatches :1165-1340 on
 *    the DISTORTED keypoints (mvKeys / mvKeysRight), then UndistortKeyPoints, ComputeImageBounds and AssignFeaturesToGrid exactly
 *    as pslfe_frame_set_from_orb_rgbd does.  Left frame left0+p of `left`'s last batch and right frame right0+p of `right`'s last
 *    batch -> slot slot0+p; the slot then holds mvKeysUn, mvuRight (DISTORTED coordinates, as in the reference) and mvDepth.
 *    left == right is allowed (one extraction launch of 2N frames).  Both handles: f's context, the same image size and nlevels,
 *    bitwise-equal scale factors, capacity <= f's.  Asynchronous on the context's stream.  Level 0 of a batch extracted with
 *    pslfe_orb_extract_batch_device is the caller's input buffer: it must stay unchanged until this call's work has run on the
 *    stream (the host entry points copy the image into the handle, so they need no such rule).
 *    Reproduced exactly (integer SAD, float steps rounded as the reference rounds them, no contraction):
 *    - row band :1182-1192: right keypoint iR is a candidate of left keypoint iL when (int)vL (vRowIndices[vL], truncation) lies
 *      in [floor(y - r), ceil(y + r)], r = 2.0f*mvScaleFactors[octave_R]; octave_R within +-1 of octave_L (:1232);
 *      uR in [uL - maxD, uL - minD] (:1237), minD = 0, maxD = mbf/minZ; maxU < 0 skips the keypoint (:1218);
 *    - descriptor choice :1221-1248: the first strict minimum below TH_HIGH = 100 in ascending iR == the least (dist, iR);
 *      the SAD step only when bestDist < thOrbDist = 75 (:1251);
 *    - SAD windows :1253-1291: both pyramids at the LEFT keypoint's octave, positions round(x*invScale) in float, w = L = 5;
 *      skipped when iniu < 0 || endu >= cols with iniu = scaleduR0+L-w (the reference's +L); metric
 *      sum |(IL - IL(w,w)) - (IR - IR(w,w))| over 11x11 (exact in integers); first minimum over incR = -5..5; bestincR == +-L
 *      rejected (:1293);
 *    - parabola and rescale :1297-1324: deltaR = (d1-d3)/(2.0f*(d1+d3-2.0f*d2)), |deltaR| > 1 rejected,
 *      bestuR = mvScaleFactors[octave]*((float)scaleduR0+(float)bestincR+deltaR), disparity = uL - bestuR accepted in
 *      [0, maxD); disparity <= 0 -> disparity = 0.01f, bestuR = (float)((double)uL - 0.01); mvDepth = mbf/disparity;
 *    - median filter :1325-1339 (the inner bestDist shadows the Hamming one: the SAD minimum is filtered): median = the
 *      size/2-th smallest SAD of the accepted keypoints, thDist = 1.5f*1.4f*median, every accepted keypoint with SAD >= thDist
 *      gets mvuRight = mvDepth = -1.
 *    Conventions where the reference is undefined: minZ = mb = mbf/fx in float (the reference reads mb before
 *    :128 assigns it); no accepted keypoint -> nothing is filtered (the reference indexes an empty vector); a row band or a
 *    left row outside the image, and SAD windows outside the level image (where cv::Mat::rowRange/colRange would throw), give
 *    no match - none of them occurs for keypoints of the extractor. */
int pslfe_frame_set_from_orb_stereo(pslfe_frame* f, int slot0, pslfe_orb* left, int left0, pslfe_orb* right, int right0,
                                    int nframes, const PslCamera* cam);
/* == The monocular Frame constructor src/Frame.cc:213-267 for frames first..first+nframes-1 of orb's last batch -> slots
 *    slot0..slot0+nframes-1: UndistortKeyPoints :1062-1092 (skipped when k1 == 0, as the reference does), mvuRight = mvDepth = -1
 *    (:241-243), ComputeImageBounds :1135-1168 (first-frame statics, as the RGB-D and stereo paths keep them: they depend on the
 *    camera and the image size only, so a frame without keypoints - for which the reference returns before both - changes
 *    nothing) and AssignFeaturesToGrid :269-284 on the undistorted points.  A frame with 0 keypoints gives a slot with n = 0 and an
 *    empty grid.  The slot then holds mvKeysUn / mvDepth / mvuRight (pslfe_frame_fetch).  Extractor capacity <= f's
 *    (PSLFE_E_CAPACITY).  Asynchronous on f's context stream. */
int pslfe_frame_set_from_orb_mono(pslfe_frame* f, int slot0, pslfe_orb* orb, int first, int nframes, const PslCamera* cam);
/* Tap per left keypoint of a stereo slot: idx_right = right keypoint chosen by the descriptor stage (-1: none below
 * thOrbDist), sad = the SAD minimum of the window sweep (-1: skipped or rejected before the median filter).  *n = the slot's
 * keypoint count; either array may be NULL.  PSLFE_E_STATE if the slot was not set by pslfe_frame_set_from_orb_stereo. */
int pslfe_frame_debug_stereo(pslfe_frame* f, int slot, int32_t* idx_right, int32_t* sad, int cap, int* n);
/* mvKeysUn, mvDepth, mvuRight of a slot (any pointer may be NULL). */
int pslfe_frame_fetch(pslfe_frame* f, int slot, PslKeyPoint* kps_un, float* depth, float* uright, int cap, int* n);

/* Tap for parity tests: CSR of mGrid in the order GetFeaturesInArea visits it (cell = ix*48+iy):
 * start[64*48+1], idx[n]. */
int pslfe_frame_debug_grid(pslfe_frame* f, int slot, int32_t* start, int32_t* idx, int cap, int* n);

/* == ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) src/ORBmatcher.cc:1328-1470
 *    after the host has projected the last frame's map points: queries[i] / qdesc[i] (32 B) describe
 *    map point i.  taken[c] != 0 (or NULL = none): current keypoint c already holds a map point with
 *    Observations()>0 and is skipped (:1401-1403).  Outputs: match[i] = current keypoint given to
 *    query i or -1 (TH_HIGH = 100 gate, then - if check_orientation - the rotation-histogram filter
 *    :1448-1467); assigned[c] (may be NULL) = query whose map point ends up in
 *    CurrentFrame.mvpMapPoints[c] or -1; *nmatches = the function's return value.  The reference's
 *    sequential first-come-first-served behaviour is reproduced exactly. */
int pslfe_orb_search_by_projection_last(pslfe_frame* cur, int slot, const PslProjQuery* queries, const uint8_t* qdesc,
                                        int nq, const uint8_t* taken, int check_orientation, int32_t* match,
                                        int32_t* assigned, int* nmatches);
/* == ORBmatcher::SearchByProjection(F, vpMapPoints, th) src/ORBmatcher.cc:45-129: best and second
 *    best in the window, ratio test `nnratio` only when both lie on the same octave (:118-125). */
int pslfe_orb_search_by_projection_map(pslfe_frame* cur, int slot, const PslProjQuery* queries, const uint8_t* qdesc,
                                       int nq, const uint8_t* taken, float nnratio, int32_t* match, int32_t* assigned,
                                       int* nmatches);
/* == ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) src/ORBmatcher.cc:1472-1599
 *    (relocalisation) after the host has projected the keyframe's map points (skipping bad ones and those in
 *    sAlreadyFound): window search as above, but every occupied keypoint is skipped (taken[c] != 0 <=>
 *    CurrentFrame.mvpMapPoints[c] != NULL), every match occupies its keypoint, there is no stereo gate and the
 *    distance gate is ORBdist.  queries[i].angle = pKF->mvKeysUn[i].angle; `blocks` is ignored (always 1).  With ORBdist = 256 a
 *    query whose candidates are all at distance 256 has no match (the reference then writes mvpMapPoints[-1], :1555-1557). */
int pslfe_orb_search_by_projection_kf(pslfe_frame* cur, int slot, const PslProjQuery* queries, const uint8_t* qdesc, int nq,
                                      const uint8_t* taken, int orb_dist, int check_orientation, int32_t* match,
                                      int32_t* assigned, int* nmatches);

/* == ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) src/ORBmatcher.cc:159-288, from the point where the two DBoW2
 *    FeatureVectors are walked.  DBoW2 (vocabulary, FeatureVector) stays on the host; the caller passes
 *    fidx: the frame's FeatureVector flattened in node order (F.mFeatVec: for node ascending, its vIndicesF);
 *    one query per keyframe feature in the reference's iteration order (common nodes ascending, vIndicesKF order,
 *    NULL / bad map points dropped): the run [start, start+len) of fidx that is its node's vIndicesF, its descriptor
 *    (qdesc, 32 B) and pKF->mvKeysUn[realIdxKF].angle.
 *    Slot `slot` of `f` holds the frame's keypoints (mvKeys angles) and descriptors.  TH_LOW = 50, ratio test with
 *    mfNNratio against the second best (256 when there is none), a frame feature matched by an earlier query is skipped
 *    (:206-207), rotation histogram as elsewhere.  match[i] = frame feature of query i or -1; assigned[f] = query whose
 *    map point ends up in vpMapPointMatches[f]; *nmatches = the return value. */
typedef struct PslBowQuery {
    int32_t start, len;
    float angle;
} PslBowQuery;
int pslfe_orb_search_by_bow(pslfe_frame* f, int slot, const int32_t* fidx, int nfidx, const PslBowQuery* queries,
                            const uint8_t* qdesc, int nq, float nnratio, int check_orientation, int32_t* match,
                            int32_t* assigned, int* nmatches);

/* Batched, HBM-resident form of pslfe_orb_search_by_projection_last: pair p searches slot
 * slot0 + p with d_nq[p] queries at d_queries + p*qstride (descriptors at d_qdesc + p*qstride*32),
 * writes d_match + p*qstride and d_nmatches[p].  Asynchronous on the context's stream. */
int pslfe_orb_search_by_projection_last_device(pslfe_frame* cur, int slot0, int npairs, const PslProjQuery* d_queries,
                                               const uint8_t* d_qdesc, const int32_t* d_nq, int qstride,
                                               int check_orientation, int32_t* d_match, int32_t* d_nmatches);

/* == ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) src/ORBmatcher.cc:405-520 with
 *    mfNNratio = nnratio, mbCheckOrientation = check_orientation (Tracking::MonocularInitialization: ORBmatcher(0.9, true),
 *    windowSize 100, src/Tracking.cc:696).  F1 = slot slot1 of f1, F2 = slot slot2 of f2 (f1 == f2 allowed; one context).
 *    Reproduced exactly:
 *    - queries: the F1 keypoints of octave 0 (:421-423), in ascending index order;
 *    - candidates: F2.GetFeaturesInArea(prev[i1].x, prev[i1].y, (float)window, 0, 0) src/Frame.cc:985-1038 (window centred at
 *      prev, octave exactly 0, |dx| < r and |dy| < r on mvKeysUn, cells ix outer / iy inner, indices ascending; a cell range
 *      outside the grid is empty);
 *    - a candidate whose vMatchedDistance is <= its distance is skipped (:442-443), for the best and the second best alike;
 *      best = the first strict minimum in visiting order, bestDist2 = the second smallest surviving distance (ties included,
 *      INT_MAX with one survivor); accepted when bestDist <= TH_LOW (50) and bestDist < (float)bestDist2 * nnratio (float
 *      multiply, no contraction);
 *    - an accepted query takes its keypoint from an earlier query for good (:462-466): the earlier one gets -1 and is never
 *      searched again, but its rotHist entry stays and counts in ComputeThreeMaxima :1601-1645;
 *    - rotation histogram (:470-508): rot = angle1 - angle2 (+360 if negative), bin = round(rot * (1.0f/30)); only still
 *      matched queries in non-maximum bins are cleared.
 *    Outputs: matches12[i] for every F1 keypoint (-1: none), *nmatches = the return value, prev_matched[i] = F2 mvKeysUn of
 *    matches12[i] where it is >= 0; every other prev row keeps its value.  prev_matched: host [n1][2], in/out; matches12: host
 *    [n1].  Synchronous. */
int pslfe_orb_search_for_initialization(pslfe_frame* f1, int slot1, pslfe_frame* f2, int slot2, float* prev_matched, int window,
                                        float nnratio, int check_orientation, int32_t* matches12, int* nmatches);
/* Batched, HBM-resident form: pair p has F1 = f1 slot slot1[p], F2 = f2 slot slot2[p] (host int arrays), its own prev rows
 * d_prev + p*prev_stride*2 (float, in/out) and matches d_matches12 + p*prev_stride; d_nmatches[p].  prev_stride >= f1's capacity
 * (PSLFE_E_INVALID).  Pairs are independent.  Returns once the slot tables have been copied; the matching is queued on the
 * context's stream. */
int pslfe_orb_search_for_initialization_device(pslfe_frame* f1, const int32_t* slot1, pslfe_frame* f2, const int32_t* slot2, int npairs,
                                               float* d_prev, int prev_stride, int window, float nnratio, int check_orientation,
                                               int32_t* d_matches12, int32_t* d_nmatches);

/* ---- Projection of 3-D points into a frame: the part of both SearchByProjection variants before the window search.
 *
 * Arithmetic conventions (cv::Mat arithmetic is not in the reference tree):
 *   - a float 3x3 * 3x1 (+ 3x1) product (Rcw*x3Dw+tcw, -Rcw.t()*tcw, Rlw*twc+tlw, mRwc*x3Dc+mOw): every row is the double sum,
 *     in index order, of the exact double products (then + the double of the translation), rounded once to float;
 *   - cv::norm and Mat::dot of float 3-vectors: double sums in index order (norm: sqrt in double, rounded to float);
 *     viewCos = dot / dist in double, rounded to float;
 *   - PredictScale: ceil(psl_log((double)ratio) / (double)mfLogScaleFactor) with ratio = mfMaxDistance / dist in float, clamped to
 *     [0, nlevels-1] (ratio 0 or NaN -> 0, infinite -> nlevels-1); psl_log is the double log of psl-slam_amd/csrc/psl_f64math.h;
 *   - a point with camera depth z <= 0 (z == 0 included, where the reference goes on with inf and reaches undefined behaviour in
 *     GetFeaturesInArea), a NaN depth or a NaN pixel coordinate is not emitted.
 * Every other operation is the reference's float operation, in its order.
 *
 * Emitted rows are compacted in point order (the reference's loop order, so the matchers' first-come-first-served order is the
 * reference's); owner[q] is the point of row q.  A count larger than the row capacity is reported, never truncated silently:
 * the device forms write the first qstride rows and the full count (the window searches read at most qstride rows); the host
 * forms return PSLFE_E_CAPACITY with *nq set. */
typedef struct PslPose {
    float R[9];  /* rows 0..2, columns 0..2 of Frame::mTcw, row-major */
    float t[3];  /* rows 0..2 of column 3 */
} PslPose;
/* LastFrame.mvpMapPoints[i]: state 0 = none, 1 = a map point with Observations()==0, 2 = with Observations()>0; | 8 = mvbOutlier[i].
 * x, y, z = its GetWorldPos(). */
typedef struct PslLastPoint {
    float x, y, z;
    int32_t state;
} PslLastPoint;
/* A local map point: mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance (the 0.8f / 1.2f factors of
 * GetMin/MaxDistanceInvariance are applied inside). */
typedef struct PslMapPointGeom {
    float x, y, z, nx, ny, nz, min_dist, max_dist;
} PslMapPointGeom;

/* == ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) src/ORBmatcher.cc:1338-1390 up to the window search, for
 *    npairs pairs: pair p's last frame is slot last_slot0 + p of `last` (mvKeysUn, mvDepth, descriptors: pslfe_frame_set_rgbd /
 *    _set_from_orb_rgbd), its poses d_Tlw[p] (LastFrame.mTcw) and d_Tcw[p] (CurrentFrame.mTcw).  twc, tlc, bForward / bBackward
 *    against mb = bf/fx and bMono = mono; every existing, non-outlier point is projected (invzc = 1.0/z in double, rounded to
 *    float) and a row u, v, radius = th*mvScaleFactors[octave], ur = u - mbf*invzc, the level band of the three
 *    GetFeaturesInArea calls (:1385-1390), angle = mvKeysUn[i].angle, blocks = Observations()>0 is emitted when u, v lie in
 *    [min_x, max_x] x [min_y, max_y].  d_points: [npairs][last->cap] or NULL (no map points); d_mpdesc: [npairs][cap][32] the map
 *    points' descriptors or NULL (= the slot's keypoint descriptors).  Outputs at p*qstride: d_queries, d_qdesc (32 B per row),
 *    d_owner (may be NULL) = last-frame keypoint of the row; d_nq[p] = the row count.  qstride <= last->cap (PSLFE_E_CAPACITY).
 *    vo != 0: first the "visual odometry" points of Tracking::UpdateLastFrame src/Tracking.cc:1052-1104 (localisation mode): of
 *    the keypoints with mvDepth > 0 sorted by (z, i), the first min(n_valid, max(n_close + 1, 101)) are visited
 *    (n_close = #{0 < z <= th_depth}); those with state 0 or 1 get a new point Frame::UnprojectStereo src/Frame.cc:1365-1379
 *    (invfx = 1.0f/fx) whose descriptor is the keypoint's and which has no observations; state-2 points are kept.  VO on a slot
 *    without depth is PSLFE_E_STATE.  scale_factors: host array of nlevels (<= PSLFE_MAX_LEVELS) floats; cam: host.
 *    Asynchronous on the context's stream. */
int pslfe_orb_project_last_device(pslfe_frame* last, int last_slot0, int npairs, const PslPose* d_Tlw, const PslPose* d_Tcw,
                                  const PslLastPoint* d_points, const uint8_t* d_mpdesc, const PslCamera* cam,
                                  const float* scale_factors, int nlevels, float th, float th_depth, int mono, int vo, float min_x,
                                  float min_y, float max_x, float max_y, PslProjQuery* d_queries, uint8_t* d_qdesc,
                                  int32_t* d_owner, int32_t* d_nq, int qstride);
/* Same for one slot, host arrays: points / mpdesc hold the slot's N entries (or NULL); queries / qdesc / owner (may be NULL)
 * have room for qcap rows; *nq = row count. */
int pslfe_orb_project_last(pslfe_frame* last, int slot, const PslPose* Tlw, const PslPose* Tcw, const PslLastPoint* points,
                           const uint8_t* mpdesc, const PslCamera* cam, const float* scale_factors, int nlevels, float th,
                           float th_depth, int mono, int vo, float min_x, float min_y, float max_x, float max_y,
                           PslProjQuery* queries, uint8_t* qdesc, int32_t* owner, int* nq, int qcap);

/* == Frame::isInFrustum(pMP, view_cos_limit) src/Frame.cc:927-983 + PredictScale src/MapPoint.cc:402-416 for every local map
 *    point, and the query rows of ORBmatcher::SearchByProjection(F, vpMapPoints, th) src/ORBmatcher.cc:45-70 for those in view:
 *    gates z, image bounds (invz = 1.0f/z), 0.8f*min_dist <= |P - Ow| <= 1.2f*max_dist, viewCos >= view_cos_limit; radius
 *    = RadiusByViewingCos (2.5 if (double)viewCos > 0.998 else 4.0, :131-137) * th when th != 1, * mvScaleFactors[level];
 *    levels level-1 .. level; ur = mTrackProjXR = u - mbf*invz; angle 0; blocks 1.  Frame f: d_nmp[f] map points at
 *    d_mp + f*mpstride (descriptors d_mpdesc + f*mpstride*32), pose d_Tcw[f]; rows at f*qstride, d_nq[f] = number of map points
 *    in view (nToMatch of Tracking::SearchLocalPoints src/Tracking.cc:1725-1741; rows beyond qstride are not written).
 *    Per map point (each may be NULL): d_inview (mbTrackInView), d_level (mnTrackScaleLevel, -1 when not in view), d_viewcos
 *    (mTrackViewCos, 0 when not in view).  Asynchronous on the context's stream. */
int pslfe_orb_project_frustum_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw, const PslMapPointGeom* d_mp,
                                     const uint8_t* d_mpdesc, const int32_t* d_nmp, int mpstride, const PslCamera* cam,
                                     const float* scale_factors, int nlevels, float log_scale_factor, float view_cos_limit,
                                     float th, float min_x, float min_y, float max_x, float max_y, PslProjQuery* d_queries,
                                     uint8_t* d_qdesc, int32_t* d_owner, int32_t* d_nq, int qstride, uint8_t* d_inview,
                                     int32_t* d_level, float* d_viewcos);
/* Same for one frame, host arrays: mp / mpdesc / inview / level / viewcos have nmp entries (the last three may be NULL). */
int pslfe_orb_project_frustum(pslfe_ctx* ctx, const PslPose* Tcw, const PslMapPointGeom* mp, const uint8_t* mpdesc, int nmp,
                              const PslCamera* cam, const float* scale_factors, int nlevels, float log_scale_factor,
                              float view_cos_limit, float th, float min_x, float min_y, float max_x, float max_y,
                              PslProjQuery* queries, uint8_t* qdesc, int32_t* owner, int* nq, int qcap, uint8_t* inview,
                              int32_t* level, float* viewcos);
/* Batched, HBM-resident form of pslfe_orb_search_by_projection_map, laid out as pslfe_orb_search_by_projection_last_device;
 * d_taken: [npairs][cur->cap] or NULL. */
int pslfe_orb_search_by_projection_map_device(pslfe_frame* cur, int slot0, int npairs, const PslProjQuery* d_queries,
                                              const uint8_t* d_qdesc, const int32_t* d_nq, int qstride, const uint8_t* d_taken,
                                              float nnratio, int32_t* d_match, int32_t* d_nmatches);

/* == LSDmatcher::matchNNR add_src/LSDmatcher.cpp:354-376 (and LSDmatcher::match :378-413, whose
 *    live branch is matchNNR): matches12[i] = best train row if d0 < d1 * nnr (float compare on
 *    DMatch.distance) else -1; *nmatches = return value.  n2 < 2 is UB in the reference
 *    (:369); defined here as "no match". */
int pslfe_line_match_nnr(pslfe_ctx* ctx, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnr,
                         int32_t* matches12, int* nmatches);

/* == LSDmatcher::SearchByGeomNApearance(CurrentFrame, LastFrame, desc_th) add_src/LSDmatcher.cpp:36-110
 *    (TrackWithMotionModel, src/Tracking.cc:1183): matchNNR, then for last-frame lines that own a map
 *    line (has_mapline[i1] != 0) the 20-degree direction gate and the 10 %-of-image end-point gate.
 *    matches12[n1] as the reference leaves it; assigned[n2] = last-frame line whose map line is given to
 *    current line i2 (or -1); *lmatches = return value. */
int pslfe_line_search_by_geom_appearance(pslfe_ctx* ctx, const PslKeyLine* kl_last, const uint8_t* desc_last, int n1,
                                         const PslKeyLine* kl_cur, const uint8_t* desc_cur, int n2, const uint8_t* has_mapline,
                                         float desc_th, float min_x, float max_x, float min_y, float max_y, int32_t* matches12,
                                         int32_t* assigned, int* lmatches);
/* == LSDmatcher::FrameBFMatch(ldesc1, ldesc2, LineMatches, TH) add_src/LSDmatcher.cpp:492-516 with
 *    lineDescriptorMAD :660-685: kNN-2, gap d1-d0 above half its MAD, d0 < TH, d0 < mfNNratio*d1. */
int pslfe_line_frame_bf_match(pslfe_ctx* ctx, const uint8_t* desc1, int n1, const uint8_t* desc2, int n2, float nnratio, float TH,
                              int32_t* line_matches);
/* == Map::AssociatePlanesByBoundary(pF, dTh, aTh) src/Map.cc:204-272 (live != 0; called from
 *    src/Tracking.cc:967,1209,1329,1531) / InsectLineMatch::SearchMapInsectline
 *    add_src/InsectlineMatch.cpp:9-59 (live == 0; no live caller upstream).  planes: n x 4 world planes of
 *    the frame's LIL pairs (ComputeWorldPlane); points: n x 5 x 3 doubles = start/end of line i, start/end
 *    of line j, 3-D intersection; map_planes: m x 4 in the caller's iteration order (upstream iterates a
 *    std::set of pointers); map_bad: isBad() flags (dead variant only, may be NULL).  The live variant
 *    keeps upstream's running threshold (dTh = dis, shared by all planes) and counts every association. */
int pslfe_associate_planes(pslfe_ctx* ctx, const float* planes, const double* points, int nplanes, const float* map_planes,
                           const uint8_t* map_bad, int nmap, float dTh, float aTh, int live, int32_t* assoc, int* nmatches);

/* One projected map line of LSDmatcher::SearchByProjection: what Tracking knows after isInFrustum. */
typedef struct PslLineQuery {
    float x1, y1, x2, y2;   /* mTrackProjX1, mTrackProjY1, mTrackProjX2, mTrackProjY2                     */
    float radius;           /* th (add_src/LSDmatcher.cpp:151) or RadiusByViewingCos * th (:282-285)       */
    float th_cos;           /* TH of GetFeaturesInAreaForLine: 0.96 (:155) or the default 0.998           */
    float vx, vy;           /* mode 0: LastFrame line direction ePointInOctave - sPointInOctave (:181-183) */
    float length;           /* mode 0: LastFrame.mvKeylinesUn[i].lineLength (:192-196)                     */
    int32_t blocks;         /* the map line has Observations() > 0                                         */
    double wdir[3];         /* mode 1: MapLine::GetNormal() (:293)                                         */
} PslLineQuery;

/* == LSDmatcher::SearchByProjection(CurrentFrame, LastFrame, th) add_src/LSDmatcher.cpp:112-215 (mode 0)
 *    and LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) :260-352 (mode 1), after the host
 *    has projected the map lines; includes Frame::AssignFeaturesToGridForLine (src/Frame.cc:286-309, with
 *    the Bresenham iterator of add_src/lineIterator.cpp) and Frame::GetFeaturesInAreaForLine (:752-826).
 *    kls/desc/lineEq: the frame's mvKeylinesUn, mLdesc, mvKeyLineFunctions; dir3d (mode 1): n x 3 doubles
 *    mvLines3D[i].first - .second.  taken (may be NULL), match, assigned, *nmatches as for the ORB
 *    matchers.  grid_start (CELLS+1) / grid_idx / grid_n (may be NULL): tap of mGridForLine as CSR with
 *    cell = ix*48+iy, for parity tests. */
int pslfe_line_search_by_projection(pslfe_ctx* ctx, const PslKeyLine* kls, const uint8_t* desc, const double* lineEq,
                                    const double* dir3d, int n, float min_x, float min_y, float max_x, float max_y,
                                    const PslLineQuery* queries, const uint8_t* qdesc, int nq, const uint8_t* taken, int mode,
                                    float nnratio, int32_t* match, int32_t* assigned, int* nmatches, int32_t* grid_start,
                                    int32_t* grid_idx, int grid_cap, int* grid_n);
/* Batched, HBM-resident form of pslfe_line_search_by_projection (modes 0 and 1) for npairs pairs; every pair's results equal the
 *    one-frame entry point's on the same inputs.  Pair p: the current frame's keylines / LBD rows (32 B) / line equations at
 *    p*kl_stride (the views of pslfe_line_results_device, offset by a frame to pick "current = f+1"), d_nkl[p] lines;
 *    mode 1: d_lines3d [npairs][lines3d_stride][6] f64 = mvLines3D as pslfe_glue_lines3d_device holds it (lines3d_stride must equal
 *    kl_stride; the kernel forms first - second itself); queries / descriptors at p*qstride, min(d_nq[p], qstride) of them read;
 *    d_taken [npairs][kl_stride] or NULL.  Outputs: d_match at p*qstride, d_assigned [npairs][kl_stride] (may be NULL),
 *    d_nmatches[p].  kl_stride <= 1024.  The 64x48 grid of a pair is built in LDS with 16-bit entries; a pair with more than
 *    8192 (line, cell) entries runs in a second launch whose grid holds every entry of 1024 lines; d_nfallback (may be NULL) = the
 *    number of such pairs.  Asynchronous on the context's stream. */
int pslfe_line_search_by_projection_device(pslfe_ctx* ctx, int npairs, const PslKeyLine* d_kls, const uint8_t* d_desc,
                                           const double* d_lineEq, const int32_t* d_nkl, int kl_stride, const double* d_lines3d,
                                           int lines3d_stride, float min_x, float min_y, float max_x, float max_y,
                                           const PslLineQuery* d_queries, const uint8_t* d_qdesc, const int32_t* d_nq, int qstride,
                                           const uint8_t* d_taken, int mode, float nnratio, int32_t* d_match, int32_t* d_assigned,
                                           int32_t* d_nmatches, int32_t* d_nfallback);

/* ---- Projection of map lines into a frame: the part of both LSDmatcher::SearchByProjection variants before the window search.
 *
 * Conventions: those of the point projections above, and
 *   - SP / EP = MapLine::GetWorldPos() rounded to float; OM = 0.5*(SP+EP) - mOw is, per component, the float sum of the exact
 *     halves 0.5f*SP + 0.5f*EP (one rounding: cv::addWeighted with weights 0.5, whether it sums in float or in double), then the
 *     float difference with mOw.  OpenCV is not in the reference tree, so this is pinned against the in-repo restatement only;
 *   - an endpoint with camera depth z == 0 or NaN, a NaN pixel coordinate, dist or viewCos: the line is not in view (the reference
 *     tests z < 0 only and goes on dividing by zero; dist == 0 gives viewCos = 0/0 and is therefore not in view either);
 *   - MapLine::PredictScale (add_src/MapLine.cpp:381-390) is unclamped float arithmetic: ceil(logf(ratio) / logScaleFactor)
 *     (`using namespace std` makes log(float) std::log(float)).  logf here is the correctly rounded float log, (float)psl_log of the
 *     ratio; the quotient and ceil are the reference's float operations.  A ratio of +inf gives INT32_MAX, 0 gives INT32_MIN, NaN 0;
 *     a finite level is outside [0, nlevels) whenever the ratio is (no clamp, as in the reference).
 *   - RadiusByViewingCos (add_src/LSDmatcher.cpp:986-992): 5.0 if (double)viewCos > 0.998 else 8.0, times th when th != 1. */
typedef struct PslMapLineGeom {
    double sp[3], ep[3];      /* MapLine::GetWorldPos() (Vector6d)                                              */
    double normal[3];         /* GetNormal(): float in isInFrustum, double in the mode-1 gate (LSDmatcher.cpp:293) */
    float min_dist, max_dist; /* mfMinDistance, mfMaxDistance (the 0.8f / 1.2f factors are applied inside)      */
} PslMapLineGeom;
/* LastFrame.mvpMapLines[i]: state 0 = none, 1 = a map line with Observations()==0, 2 = with Observations()>0; | 8 = mvbLineOutlier[i]. */
typedef struct PslLastLine {
    double sp[3], ep[3], normal[3];
    float min_dist, max_dist;
    int32_t state;
    int32_t reserved;
} PslLastLine;
#ifdef __cplusplus
static_assert(sizeof(PslMapLineGeom) == 80 && sizeof(PslLastLine) == 88 && sizeof(PslLineQuery) == 64, "line projection PODs");
#endif

/* == Frame::isInFrustum(pML, view_cos_limit) src/Frame.cc:828-904 + MapLine::PredictScale for every map line of a frame, and the
 *    query rows of LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) add_src/LSDmatcher.cpp:260-289 for those in view.
 *    The caller passes the lines SearchLocalLines would test (src/Tracking.cc:1792-1808: not bad, mnLastFrameSeen != mnId).
 *    Gates in the reference's order: both camera z >= 0, endpoint 1 in [min_x, max_x] x [min_y, max_y], then endpoint 2,
 *    0.8f*min_dist <= |OM| <= 1.2f*max_dist, viewCos >= view_cos_limit.  Row: x1..y2 = mTrackProj{X,Y}{1,2}, radius =
 *    RadiusByViewingCos(viewCos) (* th when th != 1), th_cos = 0.998f (GetFeaturesInAreaForLine's default TH), wdir = normal,
 *    blocks = 1, vx = vy = length = 0.  Frame f: d_nml[f] map lines at d_ml + f*mlstride (descriptors d_mldesc + f*mlstride*32),
 *    pose d_Tcw[f]; rows at f*qstride compacted in map-line order, d_owner (may be NULL) = map line of the row, d_nq[f] = lines in
 *    view (nToMatch; rows beyond qstride are not written).  Per map line (each may be NULL): d_inview, d_level
 *    (mnTrackScaleLevel, -1 when not in view), d_viewcos (mTrackViewCos, 0 when not in view).  Asynchronous. */
int pslfe_line_project_frustum_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw, const PslMapLineGeom* d_ml,
                                      const uint8_t* d_mldesc, const int32_t* d_nml, int mlstride, const PslCamera* cam,
                                      float log_scale_factor, float view_cos_limit, float th, float min_x, float min_y, float max_x,
                                      float max_y, PslLineQuery* d_queries, uint8_t* d_qdesc, int32_t* d_owner, int32_t* d_nq,
                                      int qstride, uint8_t* d_inview, int32_t* d_level, float* d_viewcos);
/* Same for one frame, host arrays: ml / mldesc / inview / level / viewcos have nml entries (the last three may be NULL); rows for
 * qcap; more lines in view than qcap is PSLFE_E_CAPACITY with *nq set. */
int pslfe_line_project_frustum(pslfe_ctx* ctx, const PslPose* Tcw, const PslMapLineGeom* ml, const uint8_t* mldesc, int nml,
                               const PslCamera* cam, float log_scale_factor, float view_cos_limit, float th, float min_x, float min_y,
                               float max_x, float max_y, PslLineQuery* queries, uint8_t* qdesc, int32_t* owner, int* nq, int qcap,
                               uint8_t* inview, int32_t* level, float* viewcos);
/* == LSDmatcher::SearchByProjection(CurrentFrame, LastFrame, th) add_src/LSDmatcher.cpp:112-155 up to GetFeaturesInAreaForLine,
 *    for npairs pairs.  Pair p: the last frame's keylines (mvKeylinesUn) and LBD rows at p*kl_stride, d_nkl_last[p] of them,
 *    its PslLastLine rows d_lines + p*kl_stride, the current pose d_Tcw[p].  Every line with state & 3 != 0 and no outlier bit
 *    that passes isInFrustum(pML, 0.5) against the current pose gives a row: x1..y2, radius = th, th_cos = 0.96f, vx, vy = the
 *    last keyline's ePointInOctave - sPointInOctave, length = its lineLength, blocks = (state & 3) == 2, wdir = 0.  Query
 *    descriptor: d_mldesc + (p*kl_stride + i)*32 (GetDescriptor()) or, when d_mldesc is NULL, the last frame's own LBD row.
 *    Rows at p*qstride in line order, d_owner (may be NULL) = last-frame line, d_nq[p] = the row count.  Asynchronous. */
int pslfe_line_project_last_device(pslfe_ctx* ctx, int npairs, const PslKeyLine* d_kls_last, const uint8_t* d_ldesc_last,
                                   const int32_t* d_nkl_last, int kl_stride, const PslLastLine* d_lines, const uint8_t* d_mldesc,
                                   const PslPose* d_Tcw, const PslCamera* cam, float th, float min_x, float min_y, float max_x,
                                   float max_y, PslLineQuery* d_queries, uint8_t* d_qdesc, int32_t* d_owner, int32_t* d_nq, int qstride);
/* Same for one pair, host arrays of n lines (mldesc may be NULL). */
int pslfe_line_project_last(pslfe_ctx* ctx, const PslKeyLine* kls_last, const uint8_t* ldesc_last, int n, const PslLastLine* lines,
                            const uint8_t* mldesc, const PslPose* Tcw, const PslCamera* cam, float th, float min_x, float min_y,
                            float max_x, float max_y, PslLineQuery* queries, uint8_t* qdesc, int32_t* owner, int* nq, int qcap);

/* ---- Frame::ComputeBoW ------------------------------------------------------------- */
typedef struct pslfe_vocab pslfe_vocab;
/* The DBoW2 vocabulary (ORBvoc.txt: k = 10, L = 6, TF_IDF weighting, L1_NORM scoring) as flat arrays, uploaded once:
 * node i has children child_ids[child_begin[i] .. + child_count[i]) in the order of Node::children
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:297-329), a 32-byte descriptor, its weight and word id; a node without
 * children is a leaf (a word); node 0 is the root; L = depth of the tree (m_L). */
int pslfe_vocab_create(pslfe_ctx* ctx, int nnodes, const int32_t* child_begin, const int32_t* child_count,
                       const int32_t* child_ids, int nchild, const uint8_t* node_desc, const double* node_weight,
                       const int32_t* node_word, int L, pslfe_vocab** out);
void pslfe_vocab_destroy(pslfe_vocab* v);
/* == Frame::ComputeBoW src/Frame.cc:1053-1060 -> mpORBvocabulary->transform(descriptors, mBowVec, mFeatVec, levelsup = 4)
 *    (TemplatedVocabulary.h:1124-1195, 1218-1260).  desc: n x 32.  Per feature (any pointer may be NULL): word id,
 *    weight (features with weight <= 0 are dropped, as the reference drops stopped words) and the node at level
 *    L - levelsup.  mBowVec: nbow ascending (bow_id, bow_val) pairs, L1-normalised.  mFeatVec: nfv ascending node ids
 *    fv_node, node g owning fv_idx[fv_start[g] .. fv_start[g+1]) (feature indices ascending) - exactly the `fidx` /
 *    runs that pslfe_orb_search_by_bow takes. */
int pslfe_compute_bow(pslfe_vocab* v, const uint8_t* desc, int n, int levelsup, int32_t* f_word, double* f_weight,
                      int32_t* f_nid, int32_t* bow_id, double* bow_val, int* nbow, int32_t* fv_node, int32_t* fv_start,
                      int32_t* fv_idx, int* nfv);
/* Same for nframes frames in HBM: descriptors [nframes][stride][32], counts [nframes]; outputs [nframes][stride]
 * (bow_start / fv_start: [nframes][stride + 1]; bow_start is scratch), counts [nframes].  Asynchronous.
 * nframes >= 1, 1 <= stride <= 4096, levelsup >= 0 and no NULL pointer, else PSLFE_E_INVALID.  The counts are read on the device
 * only, so a count outside 0 .. stride cannot be refused here: frame f uses min(max(d_counts[f], 0), stride) features - a count
 * above the stride is the stride, a negative count is an empty frame (nbow = nfv = 0, fv_start[0] = 0).  A frame writes
 * n per-feature rows, nbow (bow_id, bow_val) pairs, nfv nodes, nfv + 1 starts and fv_start[nfv] indices of its own rows and
 * nothing else: not its rows past those extents (bow_start excepted) and no row of another frame.  A feature whose leaf lies
 * above level L - levelsup has node 0 (the reference leaves its node id unset); levelsup >= L gives node 0 for all, as there. */
int pslfe_compute_bow_device(pslfe_vocab* v, const uint8_t* d_desc, const int32_t* d_counts, int nframes, int stride,
                             int levelsup, int32_t* d_fword, double* d_fweight, int32_t* d_fnid, int32_t* d_bow_id,
                             double* d_bow_val, int32_t* d_bow_start, int32_t* d_nbow, int32_t* d_fv_node,
                             int32_t* d_fv_start, int32_t* d_fv_idx, int32_t* d_nfv);

/* ---- KeyFrameDatabase: BoW scores and the candidate queries of loop closing and relocalisation ------------------ */
/* The step between Frame::ComputeBoW and the searches that follow a candidate list.  The reference keeps an inverted file
 * (word -> list of keyframes, src/KeyFrameDatabase.cc:33-73) and scores what a walk over the query's words reaches; here the
 * BowVectors are resident in HBM, one row of at most max_words ascending (word id, f64 value) pairs per slot (a slot is the
 * caller's name for a keyframe, 0 .. max_keyframes-1), and a query visits every live row.  Per slot it gives what the walk of
 * DetectLoopCandidates :86-104 / DetectRelocalizationCandidates :207-222 leaves behind:
 *   words       the number of word ids common to the query and the row (mnLoopWords / mnRelocWords); 0 for a slot that is
 *               dead, excluded or shares no word;
 *   first_word  the smallest common word id, or -1: lKFsSharingWords holds the slots with words > 0 in ascending
 *               (first_word, order of their add) - the order in which the walk meets them;
 *   score       mpVoc->score(query, row) == DBoW2::L1Scoring::score Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68 as f64, the
 *               same additions in the same order (bit-identical); 0.0 where words == 0.  The reference scores only the keyframes
 *               with words > minCommonWords (:129, :246); the others' scores are there to be ignored;
 *   max_common  the maximum of words (maxCommonWords :113-118, :228-233).
 * The covisibility tails (:141-196, :255-308) walk the caller's map graph and stay with the caller; the mirrors
 * (KeyFrameDatabase in psl-slam_amd/host/pslfe.hpp and the Python package) hold them as written.  Everything is allocated by
 * pslfe_kfdb_create.  All calls on one handle come from one thread at a time and run on the context's stream. */
typedef struct pslfe_kfdb pslfe_kfdb;
/* max_keyframes 1 .. 2^24 slots of max_words 1 .. 4096 (the longest BowVector pslfe_compute_bow writes) entries: 12 bytes each */
int pslfe_kfdb_create(pslfe_ctx* ctx, int max_keyframes, int max_words, pslfe_kfdb** out);
void pslfe_kfdb_destroy(pslfe_kfdb* db);
/* == KeyFrameDatabase::add src/KeyFrameDatabase.cc:40-46 of the keyframe in `slot` with mBowVec = n ascending (bow_id, bow_val)
 *    pairs (host arrays; n <= max_words, ids >= 0 and strictly ascending, PSLFE_E_INVALID otherwise).  A live slot is
 *    PSLFE_E_INVALID: erase it first.  Every add takes the next add-sequence number.  Synchronous. */
int pslfe_kfdb_add(pslfe_kfdb* db, int slot, const int32_t* bow_id, const double* bow_val, int n);
/* The same for the nframes BowVectors of a pslfe_compute_bow_device result, device to device: frame f goes to slot0 + f, the
 * sequence numbers follow f.  stride <= max_words (PSLFE_E_INVALID otherwise: a row must fit whatever its count).  Asynchronous. */
int pslfe_kfdb_add_device(pslfe_kfdb* db, int slot0, const int32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow,
                          int nframes, int stride);
/* == KeyFrameDatabase::erase :48-67; a slot that is not live is left alone, as the reference's walk finds nothing to erase. */
int pslfe_kfdb_erase(pslfe_kfdb* db, int slot);
/* == KeyFrameDatabase::clear :69-73 */
int pslfe_kfdb_clear(pslfe_kfdb* db);
/* Slot state (either array may be NULL): live[max_keyframes], seq[max_keyframes] = the add-sequence number, -1 for a dead slot. */
int pslfe_kfdb_state(const pslfe_kfdb* db, uint8_t* live, int64_t* seq);
/* One query on host arrays (n <= max_words, ids as for add); exclude: NULL or max_keyframes bytes, non-zero = the slot is left out
 * (spConnectedKeyFrames :78, :96) and does not count for max_common.  words, first_word, score: max_keyframes entries each.
 * n == 0 or an empty database: zeros, first_word -1, *max_common = 0.  Synchronous. */
int pslfe_kfdb_query(pslfe_kfdb* db, const int32_t* bow_id, const double* bow_val, int n, const uint8_t* exclude, int32_t* words,
                     int32_t* first_word, double* score, int* max_common);
/* nq queries in one launch, read where pslfe_compute_bow_device wrote them: query q = d_nbow[q] pairs at d_bow_id / d_bow_val +
 * q*stride (stride <= 4096).  d_exclude: NULL or [nq][max_keyframes]; outputs [nq][max_keyframes], d_max_common [nq].
 * Asynchronous on the context's stream. */
int pslfe_kfdb_query_device(pslfe_kfdb* db, const int32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nq,
                            int stride, const uint8_t* d_exclude, int32_t* d_words, int32_t* d_first_word, double* d_score,
                            int32_t* d_max_common);
/* == mpORBVocabulary->score(CurrentBowVec, pKF->mBowVec) of the minScore loop of LoopClosing::DetectLoop src/LoopClosing.cc:124-138
 *    for the keyframes in slots[nslots] (host arrays): score[j] as f64; the caller narrows to float as the reference does.  A slot
 *    that is out of range or not live is PSLFE_E_INVALID.  Synchronous. */
int pslfe_kfdb_score(pslfe_kfdb* db, const int32_t* bow_id, const double* bow_val, int n, const int32_t* slots, int nslots,
                     double* score);

/* ---- KeyFrame-rate matchers of LocalMapping / LoopClosing ------------------------------ */
/* These run on other threads than Tracking in the reference (src/LocalMapping.cc:336, 580, 796-872,
 * src/LoopClosing.cc:599, 245-330): give them their own pslfe_ctx (own stream) and one pslfe_kf handle per thread.  A frame
 * slot they read must be complete (its owner's stream synchronised) when it belongs to another context.  All entry points
 * take host pointers and return after the results have arrived. */
typedef struct pslfe_kf pslfe_kf;
int pslfe_kf_create(pslfe_ctx* ctx, pslfe_kf** out);
void pslfe_kf_destroy(pslfe_kf* k);

/* The candidate loop shared by ORBmatcher::Fuse(pKF, vpMapPoints, th) src/ORBmatcher.cc:825-966 (chi2 = 1: the
 * reprojection gates :907-934, 7.8 with a right coordinate and 5.99 without), ORBmatcher::Fuse(pKF, Scw, vpPoints, th,
 * vpReplacePoint) :968-1100 (chi2 = 0) and one direction of SearchBySim3 :1165-1232: KeyFrame::GetFeaturesInArea(u, v,
 * radius) src/KeyFrame.cc:685-724 on the grid of slot `slot`, octaves max_level-1 .. max_level (max_level =
 * nPredictedLevel; min_level, angle, blocks are ignored), the smallest DescriptorDistance, first visited on ties.
 * The caller passes projected rows (pslfe_kf_project makes them on the device; pslfe_kf_fuse_keyframes does both for a set
 * of keyframes); a query with radius < 0 is one the reference dropped before the search.
 * best_idx[i] = keypoint or -1, best_dist[i] = its distance or INT_MAX: the caller applies bestDist <= TH_LOW and
 * mutates the map (:950-964).  inv_level_sigma2: pKF->mvInvLevelSigma2 (nlevels <= 16 entries; chi2 = 1 only). */
int pslfe_kf_window_best(pslfe_kf* k, pslfe_frame* f, int slot, const PslProjQuery* queries, const uint8_t* qdesc, int nq,
                         int chi2, const float* inv_level_sigma2, int nlevels, int32_t* best_idx, int32_t* best_dist);
/* == ORBmatcher::SearchBySim3 src/ORBmatcher.cc:1102-1326 after the projections (pslfe_kf_search_by_sim3_poses projects too): q12[i1] = map point i1 of KF1 in KF2's
 *    image (radius < 0: none / already matched / bad / a gate failed), qdesc1 its descriptor, n1 = N1; q21 / qdesc2 / n2
 *    likewise.  Both directions, TH_HIGH, then the agreement check :1307-1323: match12[i1] = idx2 or -1. */
int pslfe_kf_search_by_sim3(pslfe_kf* k, pslfe_frame* f1, int slot1, pslfe_frame* f2, int slot2, const PslProjQuery* q12,
                            const uint8_t* qdesc1, int n1, const PslProjQuery* q21, const uint8_t* qdesc2, int n2,
                            int32_t* match12, int* nfound);
/* == ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) src/ORBmatcher.cc:522-655 (LoopClosing::ComputeSim3, src/LoopClosing.cc:265),
 *    from the point where the two FeatureVectors are walked.  Slot `slot2` of f2 holds KF2 (mvKeysUn, descriptors).
 *    - fidx2: pKF2->mFeatVec flattened in node order, keeping only the features whose map point exists and is not bad - the
 *      caller applies `!pMP2` :576 and `pMP2->isBad()` :579 by leaving the others out.  A feature appears at most once and the
 *      runs of two nodes do not overlap (PSLFE_E_INVALID otherwise): that is what a FeatureVector is, and what lets nodes run
 *      side by side;
 *    - one query per KF1 feature whose map point exists and is not bad (:558-562), in the reference's iteration order (common
 *      nodes ascending :550-632, f1it->second order :554): [start, start+len) = the run of fidx2 that is the shared node's index
 *      list in KF2, angle = pKF1->mvKeysUn[idx1].angle, qdesc = Descriptors1.row(idx1); the queries of one node are consecutive;
 *    - :566-596: bestDist1 = the first strict minimum in run order, bestDist2 = the second smallest distance (256 when there is
 *      none), a KF2 feature taken by an earlier query is skipped (vbMatched2 :576, set at :603);
 *    - :598-600: accepted when bestDist1 < TH_LOW = 50, STRICTLY (pslfe_orb_search_by_bow, the (pKF, F) overload, has <= :228),
 *      and (float)bestDist1 < nnratio*(float)bestDist2 (float multiply, no contraction);
 *    - :605-615, :634-652: rot = angle1 - angle2 (+360 when negative), bin = round(rot*(1.0f/30)), bin 30 -> 0,
 *      ComputeThreeMaxima :1601-1645; a match in a non-maximum bin is cleared but its KF2 feature stays marked (vbMatched2 is
 *      only read inside the candidate loop).
 *    match[i] = KF2 feature of query i or -1 (vpMatches12[idx1] = vpMapPoints2[match[i]]); *nmatches = the return value. */
int pslfe_kf_search_by_bow(pslfe_kf* k, pslfe_frame* f2, int slot2, const int32_t* fidx2, int nfidx2, const PslBowQuery* queries,
                           const uint8_t* qdesc, int nq, float nnratio, int check_orientation, int32_t* match, int* nmatches);
/* The candidate loop of LoopClosing::ComputeSim3 src/LoopClosing.cc:252-284 in one call: candidate c is slot slots2[c] of f2, its
 * flattened FeatureVector fidx2[fidx2_off[c] .. fidx2_off[c+1]), its queries (those of the CURRENT keyframe against this candidate;
 * start is relative to fidx2_off[c]) queries / qdesc [q_off[c] .. q_off[c+1]); both offset arrays have ncand+1 ascending entries
 * starting at 0.  Candidates are independent: match rows q_off[c].. and nmatches[c] equal what pslfe_kf_search_by_bow gives for
 * candidate c alone.  One upload, one launch chain sized by the queries and node runs of all candidates, one synchronisation. */
int pslfe_kf_search_by_bow_candidates(pslfe_kf* k, pslfe_frame* f2, const int32_t* slots2, int ncand, const int32_t* fidx2,
                                      const int32_t* fidx2_off, const PslBowQuery* queries, const uint8_t* qdesc,
                                      const int32_t* q_off, float nnratio, int check_orientation, int32_t* match,
                                      int32_t* nmatches);
/* == ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) src/ORBmatcher.cc:290-403 (src/LoopClosing.cc:375) after
 *    the projection (pslfe_kf_search_by_projection_sim3_pose projects too).  The host decomposes Scw :299-303, projects and applies the gates of :316-357 (isBad, spAlreadyFound, depth,
 *    IsInImage, distance range, viewing angle, PredictScale) and passes, per map point of vpPoints in order: u, v, radius =
 *    th*mvScaleFactors[nPredictedLevel] :360, max_level = nPredictedLevel (min_level, ur, angle, blocks are ignored), its
 *    descriptor; radius < 0 for a point dropped before the search - exactly the queries of pslfe_kf_window_best.
 *    - :362 KeyFrame::GetFeaturesInArea(u, v, radius) src/KeyFrame.cc:685-724 on the grid of slot `slot`, same visiting order as
 *      pslfe_kf_window_best;
 *    - :375 a keypoint with vpMatched[idx] != NULL is skipped: taken[idx] != 0 on entry (taken: n bytes, NULL = none), or given
 *      to an earlier map point of this call at :396 - the first-come rule, reproduced exactly;
 *    - :380 octaves max_level-1 .. max_level; :387 the smallest distance, first visited on ties;
 *    - :394 accepted when bestDist <= TH_LOW = 50; the keypoint is then occupied :396.
 *    match[i] = keypoint of map point i or -1; assigned[c] (n entries, may be NULL) = the map point now in vpMatched[c] or -1
 *    (entry marks excluded: vpMatched[c] = vpPoints[assigned[c]] where assigned[c] >= 0); *nmatches = the return value. */
int pslfe_kf_search_by_projection_sim3(pslfe_kf* k, pslfe_frame* f, int slot, const PslProjQuery* queries, const uint8_t* qdesc,
                                       int nq, const uint8_t* taken, int32_t* match, int32_t* assigned, int* nmatches);
/* ---- Projection of map points into keyframes: the part of Fuse (both), SearchByProjection(pKF, Scw, ...) and SearchBySim3 before
 * the window search, for K keyframes x M map points in one call.  Conventions: those stated above PslPose (affine products, norm and
 * dot as double sums, PredictScale with psl_log and its clamps, z <= 0 or NaN dropped); the view gate is compared in double
 * (PO.dot(Pn) < 0.5 * (double)dist drops); every other float operation is the reference's, in its order, without contraction:
 * x = X*invz, u = fx*x + cx (Frame::isInFrustum multiplies fx*X first), and KeyFrame::IsInImage src/KeyFrame.cc:726-729 has a
 * STRICT upper bound (u >= min_x && u < max_x).
 *   PSLFE_KF_PROJ_FUSE  Fuse(pKF, vpMapPoints, th) src/ORBmatcher.cc:842-890: p3Dc = Rcw*p3Dw + tcw, invz = 1/z in float, ur =
 *                       u - bf*invz, PO = p3Dw - Ow with Ow = -Rcw.t()*tcw (KeyFrame::SetPose src/KeyFrame.cc:132-145 computes the same product),
 *                       0.8f*min_dist <= |PO| <= 1.2f*max_dist, view gate, MapPoint::PredictScale(dist, pKF) src/MapPoint.cc:385-400,
 *                       radius = th*mvScaleFactors[level];
 *   PSLFE_KF_PROJ_SCW   Fuse(pKF, Scw, ...) :1000-1050 and SearchByProjection(pKF, Scw, ...) :312-360 with the Rcw, tcw the caller
 *                       decomposed from Scw (:299-303, :984-988): the same with invz = 1.0/z rounded to float (:1019; 1/z in :331 is
 *                       the same value); ur is written as in mode 0 and those searches ignore it;
 *   PSLFE_KF_PROJ_SIM3  one direction of SearchBySim3 :1148-1189 / :1228-1269: p3Dc1 = R1w*p3Dw + t1w rounded to float, p3Dc2 =
 *                       sR21*p3Dc1 + t21, invz = 1.0/z, dist = |p3Dc2|, distance gate, NO view gate, PredictScale, radius.  The
 *                       caller forms sR12 = s12*R12, sR21 = (1.0/s12)*R12.t(), t21 = -sR21*t12 (:1119-1121). */
#define PSLFE_KF_PROJ_FUSE 0
#define PSLFE_KF_PROJ_SCW 1
#define PSLFE_KF_PROJ_SIM3 2
typedef struct PslKfView {
    PslPose Tcw;   /* world -> camera of this keyframe (modes 0, 1); R1w, t1w of the SOURCE keyframe (mode 2) */
    PslPose T21;   /* mode 2: sR21, t21 (camera 1 -> camera 2); ignored otherwise */
    int32_t slot;  /* slot of the keyframe whose image is searched */
} PslKfView;
/* Row k*M + i of `queries` = map point mp[i] in keyframe views[k] (rows are NOT compacted: the searches index by map point):
 * u, v, ur, radius, min_level = level-1, max_level = level, angle = 0, blocks = 0; a point that a gate drops, or whose
 * skip[k*M + i] != 0 (isBad, IsInKeyFrame, spAlreadyFound, vbAlreadyMatched, NULL: the map stays with the caller; skip == NULL = none),
 * has radius = -1 and every other field 0.  level[k*M + i] (may be NULL) = nPredictedLevel or -1.  mp holds mfMinDistance /
 * mfMaxDistance; the 0.8f / 1.2f factors are applied inside.  `slot` is not read here.  K == 0 or M == 0: PSLFE_OK, nothing written. */
int pslfe_kf_project(pslfe_kf* k, int mode, const PslKfView* views, int K, const PslMapPointGeom* mp, const uint8_t* skip, int M,
                     const PslCamera* cam, float min_x, float min_y, float max_x, float max_y, const float* scale_factors, int nlevels,
                     float log_scale_factor, float th, PslProjQuery* queries, int32_t* level);
/* == ORBmatcher::Fuse(pKF, vpMapPoints, th) src/ORBmatcher.cc:825-948 (mode 0, reprojection gates :907-934 on) or
 *    ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) :968-1085 (mode 1, gates off) up to bestDist, for the K keyframes
 *    views[k].slot of one frame store against the same M map points: LocalMapping::SearchInNeighbors src/LocalMapping.cc:790-797 and
 *    LoopClosing::SearchAndFuse src/LoopClosing.cc:587-600 in one call.  pslfe_kf_project, then the candidate loop of
 *    pslfe_kf_window_best with mpdesc[i] (M x 32 bytes, shared by all keyframes) as the descriptor of row k*M + i: one upload each of
 *    views, mp, mpdesc and skip, one launch chain, one synchronisation.  best_idx / best_dist [K*M] as pslfe_kf_window_best gives them
 *    for keyframe k alone; queries (K*M rows, may be NULL) = the rows of pslfe_kf_project, for the host tail (:950-964).
 *    inv_level_sigma2: mvInvLevelSigma2 (nlevels entries), required in mode 0. */
int pslfe_kf_fuse_keyframes(pslfe_kf* k, pslfe_frame* f, int mode, const PslKfView* views, int K, const PslMapPointGeom* mp,
                            const uint8_t* mpdesc, const uint8_t* skip, int M, const PslCamera* cam, float min_x, float min_y, float max_x,
                            float max_y, const float* scale_factors, const float* inv_level_sigma2, int nlevels, float log_scale_factor,
                            float th, int32_t* best_idx, int32_t* best_dist, PslProjQuery* queries);
/* == ORBmatcher::SearchBySim3 src/ORBmatcher.cc:1102-1326 with both projections on the device.  view12: Tcw = R1w, t1w, T21 = sR21,
 *    t21, slot = KF2's slot in f2; mp1 / desc1 / skip1: the n1 = N1 entries of pKF1->GetMapPointMatches() (skip1[i1] != 0: NULL,
 *    vbAlreadyMatched1, isBad).  view21: Tcw = R2w, t2w, T21 = sR12, t12, slot = KF1's slot in f1; mp2 / desc2 / skip2 likewise.
 *    Both mode-2 projections, then exactly pslfe_kf_search_by_sim3.  q12 / q21 (n1 / n2 rows, may be NULL): the projected rows. */
int pslfe_kf_search_by_sim3_poses(pslfe_kf* k, pslfe_frame* f1, pslfe_frame* f2, const PslKfView* view12, const PslMapPointGeom* mp1,
                                  const uint8_t* desc1, const uint8_t* skip1, int n1, const PslKfView* view21, const PslMapPointGeom* mp2,
                                  const uint8_t* desc2, const uint8_t* skip2, int n2, const PslCamera* cam, float min_x, float min_y,
                                  float max_x, float max_y, const float* scale_factors, int nlevels, float log_scale_factor, float th,
                                  int32_t* match12, int* nfound, PslProjQuery* q12, PslProjQuery* q21);
/* == ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) src/ORBmatcher.cc:290-403 from :312 on: the mode-1 projection of
 *    the M map points into view->slot of f, then exactly pslfe_kf_search_by_projection_sim3 (taken, match, assigned, *nmatches as
 *    there).  queries (M rows, may be NULL): the projected rows. */
int pslfe_kf_search_by_projection_sim3_pose(pslfe_kf* k, pslfe_frame* f, const PslKfView* view, const PslMapPointGeom* mp,
                                            const uint8_t* mpdesc, const uint8_t* skip, int M, const PslCamera* cam, float min_x,
                                            float min_y, float max_x, float max_y, const float* scale_factors, int nlevels,
                                            float log_scale_factor, float th, const uint8_t* taken, int32_t* match, int32_t* assigned,
                                            int* nmatches, PslProjQuery* queries);
/* One feature of KF1 in ORBmatcher::SearchForTriangulation, in the reference's iteration order (common vocabulary nodes
 * ascending, f1it->second order; features that have a map point and, under bOnlyStereo, those without a right coordinate
 * are dropped by the caller, :699-711). */
typedef struct PslTriQuery {
    int32_t start, len; /* the run of KF2's flattened FeatureVector under the shared node */
    float x, y, angle;  /* pKF1->mvKeysUn[idx1].pt, .angle                                  */
    int32_t stereo;     /* pKF1->mvuRight[idx1] >= 0                                       */
} PslTriQuery;
/* == ORBmatcher::SearchForTriangulation src/ORBmatcher.cc:657-823 with CheckDistEpipolarLine :140-157.  Slot `slot2` of f2
 *    holds KF2 (mvKeysUn, mvuRight, descriptors); fidx2: its FeatureVector flattened in node order; taken2[idx2] != 0 <=>
 *    pKF2->GetMapPoint(idx2) != NULL; F12 row-major 3x3; (ex, ey) the epipole :664-671; scale_factors / level_sigma2 =
 *    pKF2->mvScaleFactors / mvLevelSigma2.  TH_LOW = 50, the LAST candidate wins among equal distances (:738), vbMatched2
 *    is never set by the reference (:686) so queries are independent; rotation histogram :764-775, :793-811.
 *    match[i] = idx2 of query i or -1; *nmatches = the return value. */
int pslfe_kf_search_for_triangulation(pslfe_kf* k, pslfe_frame* f2, int slot2, const int32_t* fidx2, int nfidx2,
                                      const uint8_t* taken2, const PslTriQuery* queries, const uint8_t* qdesc, int nq,
                                      const float* F12, float ex, float ey, int only_stereo, int check_orientation,
                                      const float* scale_factors, const float* level_sigma2, int nlevels, int32_t* match,
                                      int* nmatches);
/* One projected map line of LSDmatcher::Fuse (add_src/LSDmatcher.cpp:885-931). */
typedef struct PslLineFuseQuery {
    float x1, y1, x2, y2; /* u1, v1, u2, v2                                 */
    float radius;         /* th * mvScaleFactorsLine[level]; < 0: dropped   */
    int32_t level;        /* nPredictedLevel                                */
} PslLineFuseQuery;
/* == the search of LSDmatcher::Fuse add_src/LSDmatcher.cpp:933-958: KeyFrame::GetLinesInArea(u1, v1, u2, v2, radius,
 *    TH = 0.998) src/KeyFrame.cc:857-891 over kls = pKF->mvKeyLines, octaves level-1 .. level, smallest distance to
 *    desc row idx, first on ties; best_idx = -1, best_dist = 256 when none - a keyline at distance 256 is none, the
 *    reference starts from bestDist = 256 and takes dist < bestDist.  `desc` (ndesc rows) is the matrix the caller reads rows
 *    from: the reference indexes pKF->mDescriptors (the ORB matrix) with the line index at :945; a line without a row is
 *    skipped. */
int pslfe_kf_line_fuse_best(pslfe_kf* k, const PslKeyLine* kls, int n, const uint8_t* desc, int ndesc,
                            const PslLineFuseQuery* queries, const uint8_t* qdesc, int nq, int32_t* best_idx,
                            int32_t* best_dist);
/* ---- LSDmatcher::Fuse for K keyframes x M map lines: the line half of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:839-872),
 * which calls Fuse(pKFi, vpMapLineMatches) once per target keyframe with the same list.  Per (keyframe k, map line i), following
 * add_src/LSDmatcher.cpp:865-931 with the conventions stated above pslfe_kf_project (affine products, cv::norm and Mat::dot as double
 * sums, every other step one float operation in the reference's order, never contracted):
 *   - skip[k*M + i] != 0 (NULL, isBad(), IsInKeyFrame(pKF) :869-873; the map stays with the caller; skip == NULL = none): dropped,
 *     tested before anything else;
 *   - sp, ep, normal of PslMapLineGeom rounded to float (:877-878, :919); SPc = Rcw*SP + tcw, EPc likewise;
 *   - SPc.z < 0.0f || EPc.z < 0.0f: the reference executes `return false` (:890-891) and leaves the WHOLE function.  stop[k] = the
 *     smallest such i among the lines not skipped, or M when there is none; every row i >= stop[k] of keyframe k is dropped.  The
 *     host tail applies the rows i < stop[k] and returns 0 (false) when stop[k] < M.  A depth of exactly +0, -0 (the comparison is a
 *     float compare, not a sign test) or NaN is no stop: it goes on and fails IsInImage;
 *   - invz = 1.0f/z, u = (fx*X)*invz + cx, v likewise (this product order differs from the point Fuse); KeyFrame::IsInImage
 *     src/KeyFrame.cc:726-729 (>= min && < max) for the first end point, then for the second;
 *   - OM = 0.5*(SP+EP) - Ow: a float sum, an exact halving, a float difference, Ow = -Rcw.t()*tcw; dist = cv::norm(OM); dropped when
 *     dist < 0.8f*min_dist || dist > 1.2f*max_dist; dropped when OM.dot(pn) < 0.5*(double)dist;
 *   - level = MapLine::PredictScale(dist, log_scale_factor_line) as pslfe_line_project_frustum computes it (unclamped float arithmetic
 *     on max_dist/dist with the correctly rounded logf).  A level outside [0, nlevels) is where the reference indexes
 *     mvScaleFactorsLine out of range (undefined behaviour); THE LIBRARY DROPS THE ROW;
 *   - row k*M + i = {u1, v1, u2, v2, radius = th*scale_factors_line[level], level}; a dropped row is radius = -1 and every other
 *     field 0.  Rows are NOT compacted: the host tail indexes by map line.  level[k*M + i] (may be NULL) = the unclamped level of every
 *     row that reached PredictScale, INT32_MIN otherwise.
 * Negative counts or more than 65535 keyframes: PSLFE_E_INVALID.  Otherwise K == 0 or M == 0: PSLFE_OK, nothing written and no other
 * argument looked at.  Otherwise nlevels outside 1..16 or a NULL array or handle: PSLFE_E_INVALID, before any device is touched.
 * Difference from K sequential Fuse calls: keyframe k+1 of the reference sees the IsInKeyFrame / isBad state that the replacements of
 * keyframe k left (:961-981); here every keyframe sees the state the caller put into `skip`.  A caller that needs that order fills
 * skip per keyframe and calls with K = 1. */
int pslfe_kf_line_project(pslfe_kf* k, const PslPose* Tcw, int K, const PslMapLineGeom* ml, const uint8_t* skip, int M,
                          const PslCamera* cam, float min_x, float min_y, float max_x, float max_y, const float* scale_factors_line,
                          int nlevels, float log_scale_factor_line, float th, PslLineFuseQuery* queries, int32_t* level, int32_t* stop);
/* == LSDmatcher::Fuse(pKF, vpMapLines, th) add_src/LSDmatcher.cpp:847-958 up to bestDist for K keyframes against the same M map lines:
 *    pslfe_kf_line_project, then for keyframe k exactly the search of pslfe_kf_line_fuse_best on rows k*M .. with the keylines
 *    kls[kl_off[k] .. kl_off[k+1]) and the descriptor rows desc[desc_off[k] .. desc_off[k+1]) (the matrix the reference indexes with the
 *    line index, :948; a keyline without a row is skipped) and mldesc[i] (M x 32 bytes) as the descriptor of map line i.  One upload,
 *    one launch chain, one synchronisation whatever K is.  best_idx[k*M + i] = index among keyframe k's own keylines or -1, best_dist =
 *    256 when none: the caller applies bestDist <= TH_LOW and mutates the map (:961-981) for the rows i < stop[k].  queries (K*M rows,
 *    may be NULL) = the rows of pslfe_kf_line_project.  Both offset arrays have K+1 ascending entries (PSLFE_E_INVALID otherwise); a
 *    keyframe with more than 65535 keylines is PSLFE_E_INVALID, the limit of pslfe_kf_line_fuse_best.  The difference from K
 *    sequential Fuse calls is the one stated above. */
int pslfe_kf_line_fuse_keyframes(pslfe_kf* k, const PslPose* Tcw, int K, const PslKeyLine* kls, const int32_t* kl_off, const uint8_t* desc,
                                 const int32_t* desc_off, const PslMapLineGeom* ml, const uint8_t* mldesc, const uint8_t* skip, int M,
                                 const PslCamera* cam, float min_x, float min_y, float max_x, float max_y,
                                 const float* scale_factors_line, int nlevels, float log_scale_factor_line, float th, int32_t* best_idx,
                                 int32_t* best_dist, PslLineFuseQuery* queries, int32_t* stop);
/* == LSDmatcher::SearchForTriangulation add_src/LSDmatcher.cpp:705-781 of one keyframe against K neighbours (CreateNewMapLines2,
 *    src/LocalMapping.cc:554-580): the pair-list overload :705-743 is TH = TH_LOW, mutual = 1; the vector<int> overload :745-781 is TH =
 *    TH_HIGH, mutual = isDouble.  desc1: the n1 LBD rows of KF1; neighbour k: rows desc2[off2[k] .. off2[k+1]) (off2: K+1 ascending
 *    entries from 0); has_mapline1[i] / has_mapline2[off2[k] + j] != 0 <=> GetMapLine(i) / GetMapLine(j) != NULL (NULL = none).  Per
 *    neighbour: pslfe_line_frame_bf_match both ways (the reverse way only when mutual), the mutual test, the GetMapLine(i) ||
 *    GetMapLine(j) filter.  match[k*n1 + i] = line of neighbour k or -1; nmatches[k] = the return value.  n1 == 0 or an empty neighbour:
 *    0 matches and a row of -1 (:715-716).  All 2K directions run in one launch chain with one synchronisation.
 *    K == 0: PSLFE_OK, nothing written and no other argument looked at.
 *    Caveat: CreateNewMapLines2 gives lines of KF1 map lines between two neighbours; has_mapline1 is the state at the call, so the
 *    caller checks GetMapLine(i) again when it consumes the pairs of neighbour k. */
int pslfe_kf_line_search_for_triangulation_keyframes(pslfe_kf* k, const uint8_t* desc1, int n1, const uint8_t* has_mapline1,
                                                     const uint8_t* desc2, const int32_t* off2, const uint8_t* has_mapline2, int K,
                                                     float nnratio, float TH, int mutual, int32_t* match, int32_t* nmatches);
/* == MapPoint::ComputeDistinctiveDescriptors src/MapPoint.cc:242-304 and MapLine::ComputeDistinctiveDescriptors
 *    add_src/MapLine.cpp:250-310 for npts map points / lines at once: the observed descriptors of point p are rows
 *    offsets[p] .. offsets[p+1] of desc (at most 1024 per point); best[p] = the row (relative to offsets[p]) with the
 *    least median Hamming distance to the others (median = sorted[0.5*(N-1)], first on ties), -1 for an empty run. */
int pslfe_kf_distinctive_descriptors(pslfe_kf* k, const uint8_t* desc, const int32_t* offsets, int npts, int32_t* best);

/* ---- Map upkeep: the geometry half of the refresh whose descriptor half is pslfe_kf_distinctive_descriptors.  These make the rows
 * (PslMapPointGeom, PslMapLineGeom) that every projection above reads.  The reference calls them wherever the map changes:
 * LocalMapping::ProcessNewKeyFrame src/LocalMapping.cc:160, :183; after both Fuse passes of SearchInNeighbors :834, :884; after
 * triangulation :512, :750; for the local points after local BA src/Optimizer.cc:1950; for EVERY map point after a loop correction or
 * a global BA src/LoopClosing.cc:500, src/Optimizer.cc:227, :2797.
 *
 * Row i has the observation run obs_kf[obs_off[i] .. obs_off[i+1]): indices into centres (nkf x 3 floats, KeyFrame::GetCameraCenter())
 * in the order in which the caller's mObservations iterates.  The reference's std::map<KeyFrame*, size_t> iterates in pointer order and
 * the sums below depend on the order: it belongs to the caller and is kept.  ref_kf[i] = the index of mpRefKF, ref_level[i] = the octave
 * of the observation in mpRefKF (mvKeysUn[observations[pRefKF]].octave / mvKeyLines[...].octave).  A row with an empty run or
 * skip[i] != 0 (mbBad; skip == NULL = none) keeps every byte: the reference's early returns.  Of the other rows the normal, min_dist and
 * max_dist are written in place; the position (x, y, z / sp, ep) is only read.
 *
 * Arithmetic (the conventions above PslPose; OpenCV and Eigen are not in the reference tree, so this is pinned against the in-repo
 * restatement tests/map_upkeep_cases.py only):
 *   points  normali = P - Ow_j, a float subtraction per component; nrm = cv::norm(normali) as the double it returns, the double sqrt of
 *           the double sum in index order of the exact squares, NOT rounded to float; normali/nrm is Mat / double as OpenCV 3.2's
 *           MatExpr evaluates it, a scaling by the reciprocal in the Mat's float: t = (float)(1.0 / nrm), term[c] = normali[c] * t;
 *           normal[c] += term[c] is a float add, sequential in run order; after the run normal[c] * (float)(1.0 / (double)n);
 *           dist = the float-rounded norm of P - centres[ref_kf[i]]; max_dist = dist * scale_factors[ref_level[i]]; min_dist =
 *           max_dist / scale_factors[nlevels-1]; float operations, never contracted.
 *   lines   mid = 0.5*(sp+ep) in double (a sum, then the exact halving); normali = mid - (double)Ow_j; norm = sqrt(x*x + y*y + z*z), the
 *           double sum in index order without contraction; normal += normali / norm, a true double division per component, sequential in
 *           run order; after the run normal / (double)n.  dist: SP, EP = sp, ep rounded to float, MP = the one-rounding half-sum stated
 *           above PslMapLineGeom, CM = MP - Ow_ref in float, dist = the float-rounded double norm of CM; min_dist, max_dist as for
 *           points.  scale_factors is the table the reference reads there, pRefKF->mvScaleFactors: the POINT table, not
 *           mvScaleFactorsLine (add_src/MapLine.cpp:358, :364).
 * There is no special case for a zero distance: the IEEE results (inf, NaN) are the reference's.
 *
 * Checks, before any device is touched: negative M or nkf is PSLFE_E_INVALID; then M == 0 is PSLFE_OK, nothing written and nothing else
 * looked at; then a NULL array (obs_kf may be NULL when there is no observation, centres when nkf == 0, in the host forms) or nlevels
 * outside 1..16 is PSLFE_E_INVALID.  The host forms also refuse, with PSLFE_E_INVALID, offsets that do not ascend from 0, an obs_kf
 * outside [0, nkf) and, for a row that is refreshed, a ref_kf outside [0, nkf) or a ref_level outside [0, nlevels).  The device forms
 * cannot see their arrays: such a row is a caller error there (the kernel reads outside the tables).  In every form obs_kf must be in
 * range for EVERY run, those of skipped rows included: the tiled layout forms the terms of a skipped row before it drops them, so a
 * stale index behind a bad point is read there, while ref_kf and ref_level of a row that is not refreshed are never read.  The device
 * row arrays (d_mp, d_ml) must be 16-byte aligned, as hipMalloc returns them and as any whole-row offset into them keeps them: the
 * kernels read and write rows in 16-byte pieces. */
/* == MapPoint::UpdateNormalAndDepth src/MapPoint.cc:330-371 for M map points.  Host arrays; returns after mp has been updated. */
int pslfe_kf_update_normal_and_depth(pslfe_kf* k, PslMapPointGeom* mp, int M, const int32_t* obs_off, const int32_t* obs_kf,
                                     const float* centres, int nkf, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* skip,
                                     const float* scale_factors, int nlevels);
/* The same on device arrays (scale_factors stays a host array of nlevels floats): queued on the context's stream, no synchronisation.
 * d_mp is the array that pslfe_orb_project_frustum_device reads and that the pslfe_kf_* entry points upload a copy of. */
int pslfe_kf_update_normal_and_depth_device(pslfe_kf* k, PslMapPointGeom* d_mp, int M, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                            const float* d_centres, int nkf, const int32_t* d_ref_kf, const int32_t* d_ref_level,
                                            const uint8_t* d_skip, const float* scale_factors, int nlevels);
/* == MapLine::UpdateAverageDir add_src/MapLine.cpp:320-367 for M map lines.  Host arrays; returns after ml has been updated. */
int pslfe_kf_line_update_average_dir(pslfe_kf* k, PslMapLineGeom* ml, int M, const int32_t* obs_off, const int32_t* obs_kf,
                                     const float* centres, int nkf, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* skip,
                                     const float* scale_factors, int nlevels);
/* The same on device arrays, as pslfe_kf_update_normal_and_depth_device; d_ml is the array pslfe_line_project_frustum_device reads. */
int pslfe_kf_line_update_average_dir_device(pslfe_kf* k, PslMapLineGeom* d_ml, int M, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                            const float* d_centres, int nkf, const int32_t* d_ref_kf, const int32_t* d_ref_level,
                                            const uint8_t* d_skip, const float* scale_factors, int nlevels);
/* The layout of the run-order sums of the four refresh entry points on this handle.  Both give the same bytes.  The default is
 * PSLFE_UPKEEP_SUM_WALK; the two have not been measured against each other, the choice is open and
 * tools/bench_map_upkeep.py is what settles it.
 *   PSLFE_UPKEEP_SUM_WALK   one thread per row walks its run;
 *   PSLFE_UPKEEP_SUM_TILED  one lane per observation forms the terms of a tile in LDS, the row's thread adds them in run order. */
#define PSLFE_UPKEEP_SUM_WALK 0
#define PSLFE_UPKEEP_SUM_TILED 1
int pslfe_kf_set_upkeep_sum(pslfe_kf* k, int layout);
/* == KeyFrame::ComputeSceneMedianDepth(q) src/KeyFrame.cc:749-779 for K keyframes (the monocular CreateNewMapPoints / CreateNewMapLines2
 *    call it once per neighbour, src/LocalMapping.cc:324, :569).  Keyframe j has the world positions x[off[j] .. off[j+1]) (float
 *    triples: GetWorldPos() of its non-NULL mvpMapPoints, in index order) and the pose Tcw[j]; off: K+1 entries ascending from 0
 *    (PSLFE_E_INVALID otherwise).  z = Rcw2.dot(x3Dw) + zcw: the double sum in index order of the exact products, + the double of
 *    tcw[2], rounded once to float; depth[j] = sorted[(n-1)/q] with integer division.  n == 0: depth[j] = -1.0f (the reference indexes
 *    an empty vector there).  A NaN depth is a precondition violation (std::sort's order is then undefined); of +0 and -0, which sort
 *    may leave in either order, the library ranks -0 first.  K < 0, q < 1 or a NULL array: PSLFE_E_INVALID; K == 0: PSLFE_OK, nothing
 *    written.  Host arrays; returns after depth has arrived. */
int pslfe_kf_scene_median_depth(pslfe_kf* k, const PslPose* Tcw, int K, const float* x, const int32_t* off, int q, float* depth);

/* ---- LocalMapping::CreateNewMapPoints src/LocalMapping.cc:275-520 and CreateNewMapLines2 :522-759: the whole neighbour loop of one
 * keyframe KF1 = mpCurrentKeyFrame against K neighbours, behind the two SearchForTriangulation matchers, in one launch chain.  The
 * result equals K sequential iterations of the reference loop: a feature of KF1 that neighbour j gave a point (line) is, for every
 * neighbour k > j, skipped by the search BEFORE its rotation histogram (src/ORBmatcher.cc:699-703; lines: dropped by the GetMapLine
 * filter behind the matching, add_src/LSDmatcher.cpp:705-743).  vbMatched2 is never set (src/ORBmatcher.cc:686): two features of KF1 may
 * take the same idx2, both are triangulated and both reported.  CheckNewKeyFrames() (:307, :555) and the abort flags are not modelled:
 * the caller passes fewer neighbours.  The baseline gates :315-329 / :560-573 stay with the caller (pslfe_kf_scene_median_depth):
 * `active`.  Arithmetic: the conventions above PslPose; psl-slam_amd/csrc/triangulate_kernels.h lists every step and is the text all
 * forms run (the kernels, the host loop of tools/dropin/newpoints_main.cpp); tests/new_points_cases.py is its numpy restatement.
 * OpenCV is not in the reference tree: parity with OpenCV itself is unpinned.  Kept as written:
 *   - the right-image reprojection term of the SECOND keyframe uses mpCurrentKeyFrame->mbf (:474);
 *   - bStereo2 of a line pair is read from the CURRENT keyframe's mvLineEq[idx2] (:607).  With idx2 >= NL1 the reference reads out of
 *     range (undefined behaviour); THE LIBRARY DROPS THE PAIR with PSL_TRIL_IDX2_RANGE;
 *   - KeyFrame::UnprojectStereo (src/KeyFrame.cc:731-747) reads mvKeys, the raw keypoints, and returns an empty Mat for z <= 0, on
 *     which x3D.t() would throw: PSL_TRI_UNPROJECT_EMPTY;
 *   - cos(2*atan2(mb/2, mvDepth)) are the float overloads (`using namespace std` of add_inc/LineExtractor.h:17 reaches the file).
 * Status of a row: every `continue` of the two bodies has its own code. */
#define PSL_TRI_CREATED 0          /* :501-517 */
#define PSL_TRI_NO_MATCH 1         /* the search gave the query no idx2 (or the row is padding, q >= nq[k]) */
#define PSL_TRI_TAKEN 2            /* idx1 received its point from an earlier neighbour: skipped by the search */
#define PSL_TRI_INACTIVE 3         /* the neighbour failed the baseline gate */
#define PSL_TRI_W_ZERO 4           /* x3D.at<float>(3) == 0 :401 */
#define PSL_TRI_UNPROJECT_EMPTY 5  /* UnprojectStereo with z <= 0 */
#define PSL_TRI_LOW_PARALLAX 6     /* :417 */
#define PSL_TRI_DEPTH1 7           /* :423 */
#define PSL_TRI_DEPTH2 8           /* :427 */
#define PSL_TRI_REPROJ1_MONO 9     /* :443 */
#define PSL_TRI_REPROJ1_STEREO 10  /* :454 */
#define PSL_TRI_REPROJ2_MONO 11    /* :469 */
#define PSL_TRI_REPROJ2_STEREO 12  /* :480 */
#define PSL_TRI_DIST_ZERO 13       /* :490 */
#define PSL_TRI_RATIO 14           /* :498 */
#define PSL_TRIL_CREATED 0
#define PSL_TRIL_NO_MATCH 1
#define PSL_TRIL_TAKEN 2
#define PSL_TRIL_INACTIVE 3
#define PSL_TRIL_IDX2_RANGE 4      /* idx2 >= NL1: mvLineEq[idx2] of the current keyframe does not exist */
#define PSL_TRIL_NO_STEREO 5       /* :639 */
#define PSL_TRIL_DEPTH_SP1 6       /* :647 */
#define PSL_TRIL_DEPTH_EP1 7       /* :651 */
#define PSL_TRIL_DEPTH_SP2 8       /* :655 */
#define PSL_TRIL_DEPTH_EP2 9       /* :659 */
#define PSL_TRIL_REPROJ_SP1 10     /* :673 */
#define PSL_TRIL_REPROJ_EP1 11     /* :685 */
#define PSL_TRIL_REPROJ_SP2 12     /* :698 */
#define PSL_TRIL_REPROJ_EP2 13     /* :709 */
#define PSL_TRIL_DIST_ZERO 14      /* :725 */
#define PSL_TRIL_RATIO 15          /* :733 */
#define PSLFE_TRI_MAX_NEIGHBOURS 32
/* mpCurrentKeyFrame: pose, fx fy cx cy, mb, mbf, ratioFactor = 1.5f*mfScaleFactor (:300), and its index in the caller's keyframe table
 * (the `centres` of pslfe_kf_update_normal_and_depth). */
typedef struct PslTriKeyFrame {
    PslPose Tcw;
    float fx, fy, cx, cy, mb, mbf, ratio_factor;
    int32_t kf;
} PslTriKeyFrame;
/* One neighbour pKF2.  The line form reads active, kf, kf_first, Tcw, fx..cy alone. */
typedef struct PslTriNeighbour {
    int32_t active;    /* != 0: the baseline gate let it through                                              */
    int32_t slot;      /* its slot in the frame store (mvKeysUn, mvuRight, descriptors)                      */
    int32_t kf;        /* its index in the caller's keyframe table                                           */
    int32_t kf_first;  /* != 0: the caller's mObservations (pointer order) iterates pKF2 before KF1          */
    float F12[9];      /* ComputeF12(mpCurrentKeyFrame, pKF2), row-major                                     */
    float ex, ey;      /* the epipole, src/ORBmatcher.cc:664-671                                             */
    PslPose Tcw;
    float fx, fy, cx, cy, mb;
} PslTriNeighbour;
typedef struct PslNewMapPoint {
    float x, y, z;             /* x3D */
    int32_t k, idx1, idx2;     /* the neighbour, the feature of KF1, the feature of the neighbour */
} PslNewMapPoint;
typedef struct PslNewMapLine {
    float sp[3], ep[3];        /* the Vector6d of :737-739, as the floats it is filled from */
    int32_t k, idx1, idx2;
} PslNewMapLine;
#ifdef __cplusplus
static_assert(sizeof(PslTriKeyFrame) == 80 && sizeof(PslTriNeighbour) == 128 && sizeof(PslNewMapPoint) == 24 && sizeof(PslNewMapLine) == 36, "new-point PODs");
#else
_Static_assert(sizeof(PslTriKeyFrame) == 80 && sizeof(PslTriNeighbour) == 128 && sizeof(PslNewMapPoint) == 24 && sizeof(PslNewMapLine) == 36, "new-point PODs");
#endif
/* == CreateNewMapPoints :305-519.  Host arrays; returns after the outputs have arrived (one upload, two launches, one synchronisation).
 *    KF1: N1 <= 4096 features: keysun1 = mvKeysUn (pt, octave are read), keys1 = mvKeys[i].pt as N1 x 2 floats, uright1 = mvuRight,
 *    depth1 = mvDepth, taken1[i] != 0 <=> GetMapPoint(i) != NULL at the call.
 *    Neighbour k (K <= PSLFE_TRI_MAX_NEIGHBOURS): nb[k]; its FeatureVector flattened in node order is fidx2[fidx_off[k] ..
 *    fidx_off[k+1]) (at most 65535 entries); taken2, keys2 (x 2 floats: mvKeys[i].pt), depth2 hold its features at kp_off[k] ..
 *    kp_off[k+1]); both offset arrays: K+1 entries ascending from 0.  Its query list, built from the state at the call as for
 *    pslfe_kf_search_for_triangulation: rows k*nqmax .. k*nqmax + nq[k] of queries, idx1 (the feature of KF1 of the row; distinct inside
 *    a neighbour, in [0, N1)) and qdesc (32 bytes per row); nqmax <= 4096, 0 <= nq[k] <= nqmax.  scale_factors / level_sigma2: the
 *    nlevels (1..16) entries of mvScaleFactors / mvLevelSigma2, which the reference reads from both keyframes.
 *    Outputs, rows k*nqmax + q, every row written: match = idx2 of the pair as neighbour k's search returns it or -1; status = PSL_TRI_*;
 *    x3d = the triangulated point where the pair got that far, zeros otherwise (may be NULL).  nmatches[k] = the return value of
 *    neighbour k's search (0 for an inactive one).  created_by[i] = the neighbour that gave feature i its point, or -1.  The list in
 *    the reference's creation order (k ascending, then idx1 ascending: the order of vMatchedPairs): newp[0 .. *nnew), capacity N1;
 *    geom (capacity N1, may be NULL) = the same rows as PslMapPointGeom with the position filled and the other fields 0.  The host
 *    form writes all N1 rows of newp and geom: zeros behind *nnew.  The device form leaves the rows behind *d_nnew as they were.
 *    Checks, before any device is touched: negative counts, N1 or nqmax > 4096, K > 32: PSLFE_E_INVALID; then K == 0: PSLFE_OK, nothing
 *    written and nothing else looked at; then a NULL array or handle, nlevels outside 1..16, offsets that do not ascend from 0, nq[k]
 *    outside [0, nqmax], an idx1 out of range or repeated inside a neighbour: PSLFE_E_INVALID; more than 65535 feature-vector entries
 *    of one neighbour: PSLFE_E_CAPACITY; an ACTIVE neighbour's slot outside the store: PSLFE_E_INVALID, one that is not set:
 *    PSLFE_E_STATE (the slot of an inactive neighbour is never looked at).  A
 *    feature of the slot at or beyond kp_off[k+1] - kp_off[k] has no row in taken2 / keys2 / depth2 and is no candidate.  No output may
 *    overlap an input or another output. */
int pslfe_kf_create_new_map_points(pslfe_kf* k, pslfe_frame* f2, const PslTriKeyFrame* kf1, int N1, const PslKeyPoint* keysun1,
                                   const float* keys1, const float* uright1, const float* depth1, const uint8_t* taken1,
                                   const PslTriNeighbour* nb, int K, const int32_t* fidx2, const int32_t* fidx_off, const uint8_t* taken2,
                                   const float* keys2, const float* depth2, const int32_t* kp_off, const PslTriQuery* queries,
                                   const int32_t* idx1, const uint8_t* qdesc, const int32_t* nq, int nqmax, int only_stereo,
                                   int check_orientation, const float* scale_factors, const float* level_sigma2, int nlevels,
                                   int32_t* match, int32_t* status, float* x3d, int32_t* nmatches, int32_t* created_by,
                                   PslNewMapPoint* newp, int32_t* nnew, PslMapPointGeom* geom);
/* The same on device arrays: kf1, nb, fidx_off, kp_off, nq and the level tables stay host arrays, every other array is device memory;
 * queued on the context's stream, no synchronisation.  The checks that need the contents of a device array (idx1) are the caller's.
 * d_geom (N1 rows, 16-byte aligned; d_x3d too must not be NULL here) is written where pslfe_kf_update_normal_and_depth_device refreshes
 * it in place: with M = N1, d_obs_off (N1 + 1 entries: 2*min(r, *nnew), so the rows behind the list have empty runs and keep their
 * bytes), d_obs_kf (2*N1: the run (kf1->kf, nb[k].kf), the other way round when nb[k].kf_first), d_ref_kf = kf1->kf (the new point's
 * mpRefKF is the current keyframe), d_ref_level = the octave of mvKeysUn[idx1]. */
int pslfe_kf_create_new_map_points_device(pslfe_kf* k, pslfe_frame* f2, const PslTriKeyFrame* kf1, int N1, const PslKeyPoint* d_keysun1,
                                          const float* d_keys1, const float* d_uright1, const float* d_depth1, const uint8_t* d_taken1,
                                          const PslTriNeighbour* nb, int K, const int32_t* d_fidx2, const int32_t* fidx_off,
                                          const uint8_t* d_taken2, const float* d_keys2, const float* d_depth2, const int32_t* kp_off,
                                          const PslTriQuery* d_queries, const int32_t* d_idx1, const uint8_t* d_qdesc, const int32_t* nq,
                                          int nqmax, int only_stereo, int check_orientation, const float* scale_factors,
                                          const float* level_sigma2, int nlevels, int32_t* d_match, int32_t* d_status, float* d_x3d,
                                          int32_t* d_nmatches, int32_t* d_created_by, PslNewMapPoint* d_newp, int32_t* d_nnew,
                                          PslMapPointGeom* d_geom, int32_t* d_obs_off, int32_t* d_obs_kf, int32_t* d_ref_kf,
                                          int32_t* d_ref_level);
/* == CreateNewMapLines2 :554-757: pslfe_kf_line_search_for_triangulation_keyframes on (desc1, has_mapline1, desc2, off2, has_mapline2,
 *    nnratio, TH, mutual) - its launch chain, its checks - followed on the same stream by the pair body for every row.  A pair of
 *    neighbour k whose line of KF1 was created by a neighbour j < k is dropped with PSL_TRIL_TAKEN: that is the whole dependence between
 *    neighbours, so one thread per line of KF1 walks k in order.  kls1 / kls2: mvKeyLines (end points and octave are read); lines3d1 /
 *    lines3d2: mvLines3D as 6 doubles per line (camera frame); lineeq1[i] = mvLineEq[i][2] of KF1, NL1 entries; neighbour k's lines at
 *    off2[k] .. off2[k+1].  scale_factors / level_sigma2: the POINT tables, as the reference reads mvScaleFactors / mvLevelSigma2 there.
 *    Outputs, rows k*NL1 + i, every row written: match = the line of neighbour k or -1 (-1 for a taken pair: the reference's search
 *    does not return it), status = PSL_TRIL_*, sp / ep (3 floats per row) = the world end points where the pair got that far;
 *    nmatches[k] = the return value of neighbour k's search (an inactive neighbour: 0); created_by[i]; newl[0 .. *nnew) in creation
 *    order (k ascending, then idx1 ascending), capacity NL1; geom (capacity NL1, may be NULL): sp, ep filled, the rest 0.  The host form
 *    writes all NL1 rows of newl and geom: zeros behind *nnew; the device form leaves the rows behind *d_nnew as they were.
 *    No output may overlap an input or another output, in either form and for points and lines alike: no aliasing is allowed.
 *    Checks: those of the search first; NL1 > 65535 or K > 32: PSLFE_E_INVALID; K == 0: PSLFE_OK, nothing written; NL1 == 0: *nnew = 0 and
 *    nmatches = 0; then NULL arrays, nlevels outside 1..16: PSLFE_E_INVALID. */
int pslfe_kf_create_new_map_lines(pslfe_kf* k, const PslTriKeyFrame* kf1, int NL1, const uint8_t* desc1, const uint8_t* has_mapline1,
                                  const PslKeyLine* kls1, const double* lines3d1, const float* lineeq1, const PslTriNeighbour* nb, int K,
                                  const uint8_t* desc2, const int32_t* off2, const uint8_t* has_mapline2, const PslKeyLine* kls2,
                                  const double* lines3d2, float nnratio, float TH, int mutual, const float* scale_factors,
                                  const float* level_sigma2, int nlevels, int32_t* match, int32_t* status, float* sp, float* ep,
                                  int32_t* nmatches, int32_t* created_by, PslNewMapLine* newl, int32_t* nnew, PslMapLineGeom* geom);
/* The same on device arrays (kf1, nb, off2 and the level tables stay host arrays); queued on the context's stream.  d_geom (NL1 rows)
 * and the observation runs are what pslfe_kf_line_update_average_dir_device takes with M = NL1, laid out as for the point form
 * (d_ref_level = the octave of mvKeyLines[idx1]). */
int pslfe_kf_create_new_map_lines_device(pslfe_kf* k, const PslTriKeyFrame* kf1, int NL1, const uint8_t* d_desc1, const uint8_t* d_has_mapline1,
                                         const PslKeyLine* d_kls1, const double* d_lines3d1, const float* d_lineeq1, const PslTriNeighbour* nb,
                                         int K, const uint8_t* d_desc2, const int32_t* off2, const uint8_t* d_has_mapline2,
                                         const PslKeyLine* d_kls2, const double* d_lines3d2, float nnratio, float TH, int mutual,
                                         const float* scale_factors, const float* level_sigma2, int nlevels, int32_t* d_match,
                                         int32_t* d_status, float* d_sp, float* d_ep, int32_t* d_nmatches, int32_t* d_created_by,
                                         PslNewMapLine* d_newl, int32_t* d_nnew, PslMapLineGeom* d_geom, int32_t* d_obs_off,
                                         int32_t* d_obs_kf, int32_t* d_ref_kf, int32_t* d_ref_level);

/* ---- Pose optimisation: Optimizer::PoseOptimization (src/Optimizer.cc:239-1023), point edges and LIL edges ------------------
 * Called by TrackReferenceKeyFrame src/Tracking.cc:968, TrackWithMotionModel :1214, TrackLocalMap :1331 and, once per candidate,
 * Relocalization :2130-2161.
 *
 * Scope: the monocular edges (EdgeSE3ProjectXYZOnlyPose), the stereo edges (EdgeStereoSE3ProjectXYZOnlyPose) and the LIL edges
 * (EdgeLILSE3ProjectXYZ with its fixed VertexLIL, add_inc/EdgeLIL.h:210-439, src/Optimizer.cc:619-694, :973-1008): every edge the
 * function creates.  pslfe_pose_optimize[_device] take point edges only and are the reference's for a frame without live
 * mvpMapInsecs entries; pslfe_pose_optimize_lil[_device] take both kinds.
 *
 * Parity: g2o and Eigen cannot be built offline, so this stage is "HIP == restatement", parity with g2o unpinned.
 * The restatement (tests/pose_opt_cases.py) follows g2o's algorithm in double, in the reference's order of decisions: the pose
 * enters as Converter::toSE3Quat(mTcw) and leaves as Converter::toCvMat; information invSigma2 * I; Huber deltas (float)sqrt(5.991)
 * and (float)sqrt(7.815); four rounds of up to 10 Levenberg iterations, each from the input pose (:719), each ended early by
 * Terminate; tau = 1e-5, at most 10 trials after a failure, rho = (chi - chi_new) / (sum x_j (lambda x_j + b_j) + 1e-3), the factor
 * 1 - (2 rho - 1)^3 clamped to [1/3, 2/3] or lambda *= ni, ni *= 2; Terminate after 10 failed trials, rho == 0, or three iterations
 * in a row with (iniChi - chi) * 1e3 < iniChi; a non-finite trial chi2 rejects the step; after every round the plain chi2 of EVERY
 * edge at the round's pose, as a float, against 5.991f / 7.815f sets the flag and the level of the next round; no robust kernel
 * after round index 2; no further round when the frame has fewer than 10 edges (:1011).  A point behind the camera is not guarded
 * in the reference and is not guarded here.  The 6x6 system is solved by LDLt without pivoting; a pivot that is not a finite positive
 * number is "the solve failed": the trial's chi2 is DBL_MAX and the step is rejected.  The order of the sums over the edges is fixed
 * by the edge index and the edge count alone (psl-slam_amd/csrc/pslfe_pose.hip), never by the batch. */
/* One edge, in the order the reference creates them (keypoint order, :282-363). */
typedef struct PslPoseEdge {
    float u, v;         /* mvKeysUn[i].pt (:294, :329)                                                   */
    float ur;           /* mvuRight[i]; < 0: a monocular edge (:288)                                     */
    float inv_sigma2;   /* mvInvLevelSigma2[mvKeysUn[i].octave] (:301, :337)                             */
    float x, y, z;      /* pMP->GetWorldPos() (:312-315, :350-353)                                       */
} PslPoseEdge;
/* What the optimisation of a frame did: rounds run (0..4) and the iterations of each (optimize()'s return value; 0 for a round
 * that had no active edge or was not run). */
typedef struct PslPoseInfo {
    int32_t rounds;
    int32_t iterations[4];
} PslPoseInfo;
/* == Optimizer::PoseOptimization src/Optimizer.cc:239-1023 (point edges) for nframes independent frames in one launch.  Frame f: pose
 *    d_Tcw_in[f] (pFrame->mTcw), d_nedges[f] edges at d_edges + f*estride.  Outputs: d_Tcw_out[f] (the pose :1020 sets; d_Tcw_out
 *    may alias d_Tcw_in), d_outlier [nframes][estride] bytes (mvbOutlier of the edge's keypoint, :739-775), d_ngood[f] (the return
 *    value nInitialCorrespondences - nBad of the last executed round, :1022), d_info[f] (may be NULL).
 *    Fewer than 3 edges (:696): d_ngood[f] = 0, d_Tcw_out[f] = d_Tcw_in[f], the outlier bytes are not written (the reference
 *    clears mvbOutlier of those keypoints during the set-up, :291; a caller that needs this clears them).
 *    d_nedges[f] > estride (an overflow that pslfe_pose_edges_from_matches_device reported): nothing is optimised on a truncated
 *    set; d_ngood[f] = PSLFE_E_CAPACITY, d_Tcw_out[f] = d_Tcw_in[f].
 *    nframes < 0, estride < 0, a NULL array with a non-zero count: PSLFE_E_INVALID; nframes == 0: PSLFE_OK, nothing is done.
 *    A trial step whose rotation angle |omega| is not below 105414350 (the range of the restated sin / cos; NaN included) counts as a
 *    failed solve.  cam: host (fx, fy, cx, cy, bf are read).  Asynchronous on the context's stream. */
int pslfe_pose_optimize_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw_in, const PslPoseEdge* d_edges, const int32_t* d_nedges,
                               int estride, const PslCamera* cam, PslPose* d_Tcw_out, uint8_t* d_outlier, int32_t* d_ngood,
                               PslPoseInfo* d_info);
/* Same for one frame, host arrays: outlier has room for nedges bytes and is an output only (never read; not written for fewer than
 * 3 edges); returns after the results have arrived.  Tcw_out may be Tcw. */
int pslfe_pose_optimize(pslfe_ctx* ctx, const PslPose* Tcw, const PslPoseEdge* edges, int nedges, const PslCamera* cam, PslPose* Tcw_out,
                        uint8_t* outlier, int* ngood);
/* == F.mvpMapPoints[bestIdx] = pMP of ORBmatcher::SearchByProjection(F, vpMapPoints, th) src/ORBmatcher.cc:127 for nframes frames, HBM to
 *    HBM: the rows of pslfe_orb_project_frustum_device (d_owner[f][q] = the map point of row q, d_nq[f] rows) and the matches of
 *    pslfe_orb_search_by_projection_map_device (d_match[f][q] = the keypoint row q took, or -1), both with row stride qstride, become
 *    d_mp_index [nframes][frame's keypoint capacity]: the map point of every keypoint, -1 for a keypoint without one.  Where two rows
 *    took one keypoint the later row stays, as the reference's assignment overwrites.  This is the array
 *    pslfe_pose_edges_from_matches_device reads.  nframes < 0, qstride < 0 or a NULL array: PSLFE_E_INVALID; nframes == 0: PSLFE_OK.
 *    Asynchronous on the frame's context stream. */
int pslfe_pose_mp_index_from_matches_device(pslfe_frame* frame, int nframes, const int32_t* d_match, const int32_t* d_owner, const int32_t* d_nq,
                                            int qstride, int32_t* d_mp_index);
/* == The edge set-up loop src/Optimizer.cc:282-363 from the matches of nframes frames, HBM to HBM: d_mp_index[f][i] (row stride
 *    frame's keypoint capacity) is the row in frame f's PslMapPointGeom array (d_mp + f*mpstride) of keypoint i's map point
 *    (pFrame->mvpMapPoints[i]), or -1; an index outside [0, mpstride) counts as -1.  mvKeysUn, mvuRight and the octave come from slot
 *    slot0 + f; inv_level_sigma2: host array of nlevels (mvInvLevelSigma2).  The edges are compacted in keypoint order at
 *    d_edges + f*estride, d_edge_kp (may be NULL) gets the keypoint of each edge.  d_nedges[f] is the full count: a count above
 *    estride is reported, never truncated silently (the first estride rows are written).  Asynchronous on the frame's context
 *    stream.  With it the chain projection -> search -> pose -> next projection needs no host copy. */
int pslfe_pose_edges_from_matches_device(pslfe_frame* frame, int slot0, int nframes, const int32_t* d_mp_index, const PslMapPointGeom* d_mp,
                                         int mpstride, const float* inv_level_sigma2, int nlevels, PslPoseEdge* d_edges, int32_t* d_edge_kp,
                                         int32_t* d_nedges, int estride);
/* One LIL edge (EdgeLILSE3ProjectXYZ with its fixed VertexLIL, add_inc/EdgeLIL.h:210-439), in the order the reference creates them
 * (plane order, src/Optimizer.cc:631-693).  All double, as the reference holds them. */
typedef struct PslPoseLilEdge {
    double line1[6];    /* pLIL->line1: start, end (:639-640, :679-680)                                  */
    double line2[6];    /* pLIL->line2: start, end (:641-642, :681-682)                                  */
    double cross[3];    /* pLIL->crosspoint (:643, :683)                                                 */
    double obs1[3];     /* pFrame->mvle_l[i].first (:658, :685)                                          */
    double obs2[3];     /* pFrame->mvle_l[i].second (:659, :686)                                         */
    double obs_ins[2];  /* pFrame->CrossPoint_2D[i] (:660)                                               */
} PslPoseLilEdge;
/* A map LIL (InsectLine) as the set-up loop reads it: line1, line2, crosspoint (15 doubles, :639-643) and mbBad (:634). */
typedef struct PslMapLil {
    double w[15];
    uint8_t bad;
    uint8_t pad[7];
} PslMapLil;
#ifdef __cplusplus
static_assert(sizeof(PslPoseLilEdge) == 184 && sizeof(PslMapLil) == 128, "LIL PODs");
#else
_Static_assert(sizeof(PslPoseLilEdge) == 184 && sizeof(PslMapLil) == 128, "LIL PODs");
#endif
/* == Optimizer::PoseOptimization src/Optimizer.cc:239-1023 whole: the point edges as in pslfe_pose_optimize_device plus the LIL
 *    edges (:619-694, the classification :973-1008).  Frame f has d_nlil[f] LIL edges at d_lil + f*lstride; LIL edge j has the edge
 *    index d_nedges[f] + j (g2o adds them after the point edges), which fixes its place in the order of the sums.
 *    d_outlier_lil [nframes][lstride] bytes: mvbOutlier_Insec of the edge's plane ((float)chi2 > 11.07f, :993-1004).  Error
 *    (EdgeLIL.h:220-256), Jacobian (_jacobianOplusXj :339-379; row 2 is evaluated at line 2's END point, :273-275, as the
 *    reference does), information 1.0 (:241, :668), Huber delta (float)sqrt(11.07) (:628), no robust kernel after round index 2 (:1006).
 *    The `< 3` early return (:696) and the `< 10` rule (:1011) count point and LIL edges together.  d_ngood[f] =
 *    nInitialCorrespondences - nBad (:1022): the LIL edges are in the first number, nBad counts point edges only, so an outlying LIL
 *    edge counts as good.  Fewer than 3 edges in total: d_ngood[f] = 0, the pose is copied, no outlier byte of either kind is
 *    written.  d_nedges[f] > estride or d_nlil[f] > lstride: d_ngood[f] = PSLFE_E_CAPACITY, the pose is copied, nothing is optimised.
 *    A negative d_nedges[f] or d_nlil[f] (an error code that pslfe_pose_lil_edges_device left there, for instance): d_ngood[f] =
 *    PSLFE_E_INVALID, the pose is copied, nothing is optimised.
 *    lstride == 0: d_lil and d_outlier_lil may be NULL; with every d_nlil[f] == 0 the results are the bits of
 *    pslfe_pose_optimize_device.  The other rules and d_info are those of pslfe_pose_optimize_device. */
int pslfe_pose_optimize_lil_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw_in, const PslPoseEdge* d_edges, const int32_t* d_nedges,
                                   int estride, const PslPoseLilEdge* d_lil, const int32_t* d_nlil, int lstride, const PslCamera* cam,
                                   PslPose* d_Tcw_out, uint8_t* d_outlier, uint8_t* d_outlier_lil, int32_t* d_ngood, PslPoseInfo* d_info);
/* Same for one frame, host arrays (outlier: nedges bytes, outlier_lil: nlil bytes; outputs only, not written below 3 edges in total). */
int pslfe_pose_optimize_lil(pslfe_ctx* ctx, const PslPose* Tcw, const PslPoseEdge* edges, int nedges, const PslPoseLilEdge* lil, int nlil,
                            const PslCamera* cam, PslPose* Tcw_out, uint8_t* outlier, uint8_t* outlier_lil, int* ngood);
/* == The LIL set-up loop src/Optimizer.cc:631-693 for nframes frames, HBM to HBM.  Frame f has d_nplanes[f] planes (N_LJL =
 *    mvPlanes.size()); d_lil_index[f][i] (row stride plane_stride) is the row of plane i's map LIL (pFrame->mvpMapInsecs[i]) in
 *    d_map (nmap rows, shared by the frames), or -1; an index outside [0, nmap) counts as -1; a row with bad != 0 gives no edge
 *    (:634).  The observation of plane i is row i of d_le_l (mvle_l, one row per CROSSING, src/Frame.cc:528, row stride le_stride)
 *    and row i of d_cross2d (CrossPoint_2D, one row per PLANE, :643, row stride plane_stride): i is a plane index, so the two rows
 *    need not belong to the same crossing - the reference indexes them so (:658-660) and this is kept.  The edges are compacted in
 *    plane order at d_lil + f*lstride, d_edge_plane (may be NULL) gets the plane of each edge, d_nlil[f] the full count: a count
 *    above lstride is reported, never truncated silently (the first lstride rows are written).  d_nplanes[f] above plane_stride or
 *    above le_stride (rows the arrays cannot hold; impossible with the glue's own buffers): d_nlil[f] = PSLFE_E_CAPACITY and no edge
 *    of that frame is written; pslfe_pose_optimize_lil_device answers such a count with PSLFE_E_INVALID.  pslfe_glue_lil_obs_device gives the
 *    observation arrays.  Asynchronous on the context's stream. */
int pslfe_pose_lil_edges_device(pslfe_ctx* ctx, int nframes, const double* d_le_l, int le_stride, const double* d_cross2d, int plane_stride,
                                const int32_t* d_nplanes, const int32_t* d_lil_index, const PslMapLil* d_map, int nmap, PslPoseLilEdge* d_lil,
                                int32_t* d_edge_plane, int32_t* d_nlil, int lstride);

/* ---- Sim3 optimisation of loop candidates: Optimizer::OptimizeSim3 (src/Optimizer.cc:2801-2996) -------------------------------
 * Called once per candidate by LoopClosing::ComputeSim3 (src/LoopClosing.cc:326), between pslfe_kf_search_by_sim3_poses and
 * pslfe_kf_search_by_projection_sim3_pose.  One free 7-DoF vertex (VertexSim3Expmap), every map point vertex fixed, two edges per
 * matched pair: e12 (EdgeSim3ProjectXYZ, obs1 - cam_map1(project(S12.map(P2c)))) and e21 (EdgeInverseSim3ProjectXYZ, obs2 -
 * cam_map2(project(S12^-1.map(P1c)))).
 *
 * Parity: g2o and Eigen cannot be built offline, so this stage is "HIP == restatement", parity with g2o unpinned, as
 * for the pose optimisation.  The restatement (tests/sim3_opt_cases.py) follows g2o in double, in the reference's order of
 * decisions: the estimate enters as Sim3(R, t, s) with Quaterniond(R) NOT normalised (sim3.h:64-67); the Jacobians are g2o's
 * NUMERIC ones (linearizeOplus of both edges is commented out, types_seven_dof_expmap.h:147, :169: central differences with delta =
 * 1e-9, base_binary_edge.hpp:131-205) and are restated as such; information invSigma2 * I; Huber delta = the float root of th2
 * widened to double (:2850), on in both calls; optimize(5); a pair leaves the graph when the plain chi2 of either of its edges
 * exceeds (double)th2 (:2948); return 0 when fewer than 10 pairs remain (:2966; g2oS12 is then not written back); optimize(10) when a
 * pair left, optimize(5) otherwise, from the estimate the first call left, lambda / ni / _nBad re-initialised; the final test counts
 * nIn (:2974-2989).  Inside a call the Levenberg rules are those stated above PslPoseEdge, in seven unknowns; the update is
 * Sim3(update) * estimate with the four branches of sim3.h:70-142 (exp is the library's psl_exp, fdlibm's, at most one ulp off
 * glibc's); with a fixed scale update[6] = 0 and the scale keeps its bits.  A point behind a camera is not guarded in the reference
 * and is not guarded here.  The order of the sums over the pairs is fixed by the pair index and the pair count alone
 * (psl-slam_amd/csrc/pslfe_sim3.hip), never by the batch. */
/* What Sim3Solver::GetEstimatedRotation / Translation / Scale hand over (src/LoopClosing.cc:320-325). */
typedef struct PslSim3 {
    float R[9];   /* row-major */
    float t[3];
    float s;
} PslSim3;
/* The g2o::Sim3 that comes back (LoopClosing goes on in double with it, :333-334): the quaternion as Eigen holds it. */
typedef struct PslSim3D {
    double q[4];  /* x y z w, not normalised */
    double t[3];
    double s;
} PslSim3D;
/* One matched pair, in the order the reference creates them (KF1 keypoint order, :2854-2933). */
typedef struct PslSim3Pair {
    float u1, v1;         /* pKF1->mvKeysUn[i].pt (:2897)                                             */
    float inv_sigma2_1;   /* pKF1->mvInvLevelSigma2[kpUn1.octave] (:2904)                             */
    float u2, v2;         /* pKF2->mvKeysUn[i2].pt (:2914)                                            */
    float inv_sigma2_2;   /* pKF2->mvInvLevelSigma2[kpUn2.octave] (:2922)                             */
    float P1c[3];         /* R1w*P3D1w + t1w (:2873)                                                  */
    float P2c[3];         /* R2w*P3D2w + t2w (:2881)                                                  */
} PslSim3Pair;
/* What the optimisation of a candidate did: optimize() calls run (0..2), the iterations of each, and which branches of the Sim3
 * exponential its trial steps took (bit (|sigma| >= 1e-5) * 2 + (theta >= 1e-5)); pslfe_sim3_optimize_device reports it, the one-candidate host form does not. */
typedef struct PslSim3Info {
    int32_t calls;
    int32_t iterations[2];
    int32_t exp_branches;
} PslSim3Info;
#ifdef __cplusplus
static_assert(sizeof(PslSim3) == 52 && sizeof(PslSim3D) == 64 && sizeof(PslSim3Pair) == 48 && sizeof(PslSim3Info) == 16, "Sim3 PODs");
#else
_Static_assert(sizeof(PslSim3) == 52 && sizeof(PslSim3D) == 64 && sizeof(PslSim3Pair) == 48 && sizeof(PslSim3Info) == 16, "Sim3 PODs");
#endif
/* == Optimizer::OptimizeSim3 src/Optimizer.cc:2801-2996 for ncand independent candidates in one launch.  Candidate c: start
 *    d_S12_in[c], d_npairs[c] pairs at d_pairs + c*pstride.  cam1 / cam2: host, pKF1->mK / pKF2->mK (fx, fy, cx, cy are read).
 *    Outputs: d_bad [ncand][pstride] bytes, 1 where the reference nulls vpMatches1[idx] in either test and 0 for the other pairs of
 *    the candidate (bytes beyond the count are not touched); d_nin[c] = the return value; d_S12_out[c] = the optimised Sim3, or
 *    Sim3(R, t, s) of the input where the reference returns 0 before writing g2oS12 back (fewer than 10 pairs left after the first
 *    call); d_info[c] (may be NULL).  No pair: d_nin[c] = 0, nothing is optimised.  1..9 pairs: the first call runs and flags, as
 *    in the reference, then 0.  d_npairs[c] > pstride: d_nin[c] = PSLFE_E_CAPACITY; d_npairs[c] < 0 (an error code the set-up left
 *    there): d_nin[c] = PSLFE_E_INVALID; neither is clamped, nothing is optimised, no byte of d_bad is written and d_S12_out[c]
 *    is the input's Sim3.  ncand < 0, pstride < 0, a NULL array with a non-zero count: PSLFE_E_INVALID; ncand == 0: PSLFE_OK,
 *    nothing is done.  A trial step whose rotation angle is not below 105414350 counts as a failed solve.  Asynchronous on the
 *    context's stream. */
int pslfe_sim3_optimize_device(pslfe_ctx* ctx, int ncand, const PslSim3* d_S12_in, const PslSim3Pair* d_pairs, const int32_t* d_npairs,
                               int pstride, const PslCamera* cam1, const PslCamera* cam2, float th2, int fix_scale, PslSim3D* d_S12_out,
                               uint8_t* d_bad, int32_t* d_nin, PslSim3Info* d_info);
/* Same for one candidate, host arrays: bad has room for npairs bytes and is an output only; returns after the results have
 * arrived. */
int pslfe_sim3_optimize(pslfe_ctx* ctx, const PslSim3* S12, const PslSim3Pair* pairs, int npairs, const PslCamera* cam1, const PslCamera* cam2,
                        float th2, int fix_scale, PslSim3D* S12_out, uint8_t* bad, int* nin);
/* == The set-up loop src/Optimizer.cc:2854-2933 for ncand candidates of one current keyframe, HBM to HBM.  KF1 is slot slot1 of f1,
 *    candidate c is slot d_slots2[c] of f2 (mvKeysUn and octaves, already resident; a slot outside f2: d_npairs[c] =
 *    PSLFE_E_INVALID; the caller has set every slot it names: the slot numbers are in HBM, so only slot1 is checked against the
 *    store's record, and a slot of f2 that was never set holds 0 keypoints since pslfe_frame_create and gives 0 pairs).  d_i2[c][i] (row stride f1's keypoint capacity) = pMP2->GetIndexInKeyFrame(pKF2) of vpMatches1[i], or -1 for
 *    a NULL match.  d_mp1 / d_skip1 (n1 rows): pKF1->GetMapPointMatches(), skip != 0 for NULL or bad; d_mp2 / d_skip2
 *    [ncand][mp2stride]: the same per candidate, indexed by the KF2 keypoint.  d_T1w, d_T2w[c]: the keyframe poses.
 *    P3D1c = R1w*P3D1w + t1w and P3D2c are float products under the convention above PslPose (a double sum in index order, rounded
 *    once), the value PSLFE_KF_PROJ_SIM3 uses.  inv_level_sigma2: host array of nlevels (mvInvLevelSigma2).  Rows are compacted in
 *    i order at d_pairs + c*pstride; d_pair_kp (may be NULL) gets the i of each row; d_npairs[c] is the full count: a count above
 *    pstride is reported, never truncated silently (the first pstride rows are written).  An index outside its array drops the
 *    pair.  Asynchronous on the frame stores' context stream (both stores belong to one context). */
int pslfe_sim3_pairs_from_matches_device(pslfe_frame* f1, int slot1, pslfe_frame* f2, const int32_t* d_slots2, int ncand, const int32_t* d_i2,
                                         const PslMapPointGeom* d_mp1, const uint8_t* d_skip1, int n1, const PslMapPointGeom* d_mp2,
                                         const uint8_t* d_skip2, int mp2stride, const PslPose* d_T1w, const PslPose* d_T2w,
                                         const float* inv_level_sigma2, int nlevels, PslSim3Pair* d_pairs, int32_t* d_pair_kp,
                                         int32_t* d_npairs, int pstride);
/* The same set-up with one more output: d_sigma2 [ncand][pstride][2] (may be NULL) gets pKF1->mvLevelSigma2[kp1.octave] and
 * pKF2->mvLevelSigma2[kp2.octave] of each row (src/Sim3Solver.cc:84-85), read from the host table level_sigma2 of nlevels entries
 * (may be NULL when d_sigma2 is): what pslfe_sim3_solve_device needs next to the rows.  Everything else is
 * pslfe_sim3_pairs_from_matches_device, byte for byte. */
int pslfe_sim3_pairs_sigma2_from_matches_device(pslfe_frame* f1, int slot1, pslfe_frame* f2, const int32_t* d_slots2, int ncand,
                                                const int32_t* d_i2, const PslMapPointGeom* d_mp1, const uint8_t* d_skip1, int n1,
                                                const PslMapPointGeom* d_mp2, const uint8_t* d_skip2, int mp2stride, const PslPose* d_T1w,
                                                const PslPose* d_T2w, const float* inv_level_sigma2, int nlevels, PslSim3Pair* d_pairs,
                                                int32_t* d_pair_kp, int32_t* d_npairs, int pstride, const float* level_sigma2,
                                                float* d_sigma2);

/* ---- The Sim3 RANSAC of loop candidates: Sim3Solver (src/Sim3Solver.cc) ---------------------------------------------------------
 * Step 2 of LoopClosing::ComputeSim3 (src/LoopClosing.cc:284-345), between the set-up above and pslfe_sim3_optimize_device: for each
 * candidate up to max_its hypotheses from three drawn pairs (Horn's closed form), each tested on every pair by two projections.
 * The solver consumes the PslSim3Pair rows as they are (P1c, P2c; the constructor's gates are those of the set-up) plus
 * mvLevelSigma2 of the two octaves per row.  Parity: OpenCV cannot be built offline, so this stage is "HIP == restatement", parity
 * with OpenCV unpinned (DESIGN.md §3 lists the conventions: reduce, the Mat products, cv::eigen's Jacobi, norm, Rodrigues, the
 * MatExpr scales, atan2 as psl_atan2).  rand() is glibc's generator; candidate c is seeded as srand(seed0 + c) at its first
 * iteration and every iteration takes three draws (the reference shares one unseeded process-wide stream; convention H7). */
typedef struct PslSim3SolverResult {   /* per candidate */
    int32_t status;       /* 1 = a Sim3 was returned, 0 = the budget of this call is used up, 2 = bNoMore; PSLFE_E_CAPACITY /
                             PSLFE_E_INVALID for a count above pstride / a negative count or state */
    int32_t iterations;   /* mnIterations after the call */
    int32_t ninliers;     /* nInliers of the returned hypothesis, else 0 */
    int32_t best_inliers; /* mnBestInliers after the call */
    PslSim3 S12;          /* mBestRotation / mBestTranslation / mBestScale (what LoopClosing.cc:320-325 reads): the returned
                             hypothesis with status 1, zeros otherwise */
} PslSim3SolverResult;
#ifdef __cplusplus
static_assert(sizeof(PslSim3SolverResult) == 68, "Sim3 solver POD");
#else
_Static_assert(sizeof(PslSim3SolverResult) == 68, "Sim3 solver POD");
#endif
/* == Sim3Solver::iterate(n_iterations, ...) for ncand independent candidates in one launch, after SetRansacParameters(prob,
 *    min_inliers, max_its) (LoopClosing: 0.99, 20, 300).  Candidate c: d_npairs[c] rows at d_pairs + c*pstride and their sigma2 at
 *    d_sigma2 + 2*c*pstride.  n_iterations is iterate's argument (5 in ComputeSim3; max_its or more gives find()).  d_start_it[c] /
 *    d_best_in[c] (either may be NULL: 0) are mnIterations and mnBestInliers a former call left (PslSim3SolverResult.iterations /
 *    .best_inliers): the call reseeds seed0 + c and skips 3 * start_it draws, so rounds of calls continue one solver exactly.
 *    Outputs: d_res[c]; d_inliers [ncand][pstride] bytes indexed by pair row (the caller scatters them through d_pair_kp to
 *    vbInliers[mvnIndices1[i]]): the flags of the returned hypothesis with status 1, zeros with 0 and 2, for the rows of the candidate
 *    (bytes beyond the count are not touched).  d_npairs[c] > pstride: status = PSLFE_E_CAPACITY; d_npairs[c] < 0, d_start_it[c] < 0
 *    or d_best_in[c] < 0: PSLFE_E_INVALID; nothing is clamped, nothing is solved, no byte of d_inliers is written, the other fields
 *    are 0.  min_inliers < 3, max_its < 1,
 *    n_iterations < 0, ncand < 0, pstride < 0, a NULL array with a non-zero count, prob outside (0, 1): PSLFE_E_INVALID; ncand == 0:
 *    PSLFE_OK, nothing is done.  The iteration budget of every pair count is tabulated on the host (the host's log and pow) and
 *    uploaded; no logarithm runs on the device.  Asynchronous on the context's stream; per-call buffers come from the scratch arena. */
int pslfe_sim3_solve_device(pslfe_ctx* ctx, int ncand, const PslSim3Pair* d_pairs, const float* d_sigma2, const int32_t* d_npairs, int pstride,
                            const PslCamera* cam1, const PslCamera* cam2, double prob, int min_inliers, int max_its, int fix_scale,
                            uint32_t seed0, const int32_t* d_start_it, const int32_t* d_best_in, int n_iterations, PslSim3SolverResult* d_res,
                            uint8_t* d_inliers);
/* Same for one candidate, host arrays (sigma2 [npairs][2], inliers [npairs], an output only); the candidate is seeded with `seed`;
 * returns after the results have arrived. */
int pslfe_sim3_solve(pslfe_ctx* ctx, const PslSim3Pair* pairs, const float* sigma2, int npairs, const PslCamera* cam1, const PslCamera* cam2,
                     double prob, int min_inliers, int max_its, int fix_scale, uint32_t seed, int start_it, int best_in, int n_iterations,
                     PslSim3SolverResult* res, uint8_t* inliers);

/* ---- The EPnP RANSAC of relocalisation candidates: PnPsolver (src/PnPsolver.cc) -------------------------------------------------------
 * The step of Tracking::Relocalization (src/Tracking.cc:2031-2190) between SearchByBoW (:2067) and PoseOptimization (:2130): the
 * PnPsolver constructor (:2075), SetRansacParameters (:2076) and iterate(5, ...) (:2101).  For each candidate keyframe up to
 * mRansacMaxIts hypotheses from four drawn rows (EPnP, all in double), each tested on every row; every hypothesis with at least
 * mRansacMinInliers inliers is refined on the best inlier set so far.  Parity: OpenCV cannot be built offline, so this stage is "HIP ==
 * host compile of the same header == restatement", parity with OpenCV unpinned (DESIGN.md §3 lists the readings of cvMulTransposed,
 * cvSVD, cvInvert and cvSolve).  rand() is glibc's generator; candidate c is seeded as srand(seed0 + c) at its first iteration and every
 * iteration takes four draws (the reference shares one unseeded process-wide stream; convention H7). */
typedef struct PslPnpRow {   /* one correspondence of the constructor's loop (src/PnPsolver.cc:78-101) */
    float u, v;      /* mvP2D: F.mvKeysUn[i].pt (:89)                          */
    float X, Y, Z;   /* mvP3Dw: pMP->GetWorldPos() (:92-93)                    */
    float sigma2;    /* mvSigma2: F.mvLevelSigma2[kp.octave] (:90)             */
} PslPnpRow;
typedef struct PslPnpResult {   /* per candidate */
    int32_t status;        /* bit 0: a pose was returned (Tcw valid); bit 1: bNoMore; or PSLFE_E_CAPACITY / PSLFE_E_INVALID for a count
                              above rstride / a negative count or state */
    int32_t iterations;    /* mnIterations after the call */
    int32_t inliers;       /* nInliers of the returned pose, 0 without one */
    int32_t best_inliers;  /* mnBestInliers after the call */
    int32_t min_inliers;   /* mRansacMinInliers after the clamps of SetRansacParameters (:134-139) */
    PslPose Tcw;           /* mRefinedTcw (:235) or mBestTcw (:253), whichever iterate() returned; zeros otherwise */
    PslPose best_Tcw;      /* mBestTcw: state for the next call */
} PslPnpResult;
#ifdef __cplusplus
static_assert(sizeof(PslPnpRow) == 24 && sizeof(PslPnpResult) == 116, "PnP solver PODs");
#else
_Static_assert(sizeof(PslPnpRow) == 24 && sizeof(PslPnpResult) == 116, "PnP solver PODs");
#endif
/* == The constructor's loop src/PnPsolver.cc:78-101 for ncand candidates of one frame, HBM to HBM: d_mp_index[c][i] (row stride: the
 *    frame's keypoint capacity) is the row in candidate c's PslMapPointGeom array (d_mp + c*mpstride) of the map point SearchByBoW gave
 *    keypoint i (vvpMapPointMatches[c][i]), or -1; a bad or missing point is -1, and an index outside [0, mpstride) counts as -1.  It is
 *    the array pslfe_pose_edges_from_matches_device reads.  mvKeysUn[i].pt and the octave come from slot `slot` of `frame`;
 *    level_sigma2: host array of nlevels (mvLevelSigma2).  The rows are written in ascending i at d_rows + c*rstride; d_row_kp (may be
 *    NULL) gets mvKeyPointIndices.  d_nrows[c] is the full count: a count above rstride is reported, never truncated silently (the first
 *    rstride rows are written).  ncand < 0, rstride < 0, mpstride < 0, a NULL array with a non-zero count, nlevels outside
 *    1..PSLFE_MAX_LEVELS: PSLFE_E_INVALID; ncand == 0: PSLFE_OK.  Asynchronous on the frame's context stream. */
int pslfe_pnp_rows_from_matches_device(pslfe_frame* frame, int slot, int ncand, const int32_t* d_mp_index, const PslMapPointGeom* d_mp,
                                       int mpstride, const float* level_sigma2, int nlevels, PslPnpRow* d_rows, int32_t* d_row_kp,
                                       int32_t* d_nrows, int rstride);
/* == SetRansacParameters (:121-152) for a solver of N rows, on the host: *max_its_out = mRansacMaxIts and *min_inliers_out =
 *    mRansacMinInliers after the clamps, the values pslfe_pnp_solve_device tabulates.  N < 0, max_its < 1, min_inliers < 0, min_set
 *    != 4, prob outside (0, 1), a NaN epsilon or a NULL output: PSLFE_E_INVALID.  Touches no device. */
int pslfe_pnp_ransac_parameters(double prob, int min_inliers, int max_its, int min_set, float epsilon, int N, int* max_its_out,
                                int* min_inliers_out);
/* == PnPsolver::iterate(n_iterations, ...) (:165-258, with Refine :260-305 and CheckInliers :308-339) for ncand independent candidates
 *    in one launch, after SetRansacParameters(prob, min_inliers, max_its, min_set, epsilon, th2) (:121-157; Relocalization: 0.99, 10,
 *    300, 4, 0.5, 5.991).  Candidate c: d_nrows[c] rows at d_rows + c*rstride.  cam: fx, fy, cx, cy are read and widened to double.
 *    min_set must be 4, the only value the reference passes (PSLFE_E_INVALID otherwise).  The solver's state between calls is the
 *    caller's: d_state_in[c] (may be NULL: a fresh solver) is the PslPnpResult a former call left (iterations, best_inliers and
 *    best_Tcw are read; it may be d_res), and d_best_flags [ncand][rstride] (mvbBestInliers, by row) is read and written.  A call
 *    reseeds seed0 + c and skips 4 * iterations draws, so rounds of calls continue one solver exactly, also after a returned pose.
 *    The loop is the reference's `while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations)`: a call runs
 *    max(mRansacMaxIts - iterations, n_iterations) iterations unless a Refine succeeds first.
 *    Outputs: d_res[c]; d_inliers [ncand][rstride] bytes indexed by row (the caller scatters them through d_row_kp, or calls
 *    pslfe_pnp_mp_index_from_inliers_device): the flags of the returned pose, zeros without one, for the rows of the candidate.
 *    d_nrows[c] > rstride: status = PSLFE_E_CAPACITY; d_nrows[c] < 0 or a negative iterations / best_inliers in the state:
 *    PSLFE_E_INVALID; nothing is clamped, nothing is solved, no byte of d_inliers or d_best_flags is written, the other fields are 0.
 *    min_inliers < 0, max_its < 1, n_iterations < 0, ncand < 0, rstride < 0, a NULL array with a non-zero count, prob outside (0, 1), a
 *    NaN epsilon or th2: PSLFE_E_INVALID; ncand == 0: PSLFE_OK, nothing is done.  The budget and mRansacMinInliers of every row count
 *    are tabulated on the host (the host's log and pow) and uploaded; no logarithm runs on the device.  Asynchronous on the context's
 *    stream; per-call buffers come from the scratch arena. */
int pslfe_pnp_solve_device(pslfe_ctx* ctx, int ncand, const PslPnpRow* d_rows, const int32_t* d_nrows, int rstride, const PslCamera* cam,
                           double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2, uint32_t seed0,
                           const PslPnpResult* d_state_in, uint8_t* d_best_flags, int n_iterations, PslPnpResult* d_res, uint8_t* d_inliers);
/* Same for one candidate, host arrays: state (may be NULL) and best_flags [nrows] (read and written) are the solver's state, inliers
 * [nrows] an output only; the candidate is seeded with `seed`; returns after the results have arrived. */
int pslfe_pnp_solve(pslfe_ctx* ctx, const PslPnpRow* rows, int nrows, const PslCamera* cam, double prob, int min_inliers, int max_its,
                    int min_set, float epsilon, float th2, uint32_t seed, const PslPnpResult* state, uint8_t* best_flags, int n_iterations,
                    PslPnpResult* res, uint8_t* inliers);
/* == src/Tracking.cc:2119-2128 for ncand candidates, HBM to HBM: keypoint j keeps its map point (d_mp_index_out[c][j] =
 *    d_mp_index[c][j]) if it is the keypoint d_row_kp[c][r] of a row r < min(d_nrows[c], rstride) with d_inliers[c][r] set;
 *    every other keypoint becomes -1.  kpstride: the row stride of both index arrays (the frame's keypoint capacity); a row whose
 *    keypoint is outside [0, kpstride) is ignored.  d_mp_index_out may not alias d_mp_index.  The result feeds
 *    pslfe_pose_edges_from_matches_device unchanged.  Negative counts or a NULL array: PSLFE_E_INVALID; ncand == 0: PSLFE_OK.
 *    Asynchronous on the context's stream. */
int pslfe_pnp_mp_index_from_inliers_device(pslfe_ctx* ctx, int ncand, const int32_t* d_mp_index, const int32_t* d_row_kp, const uint8_t* d_inliers,
                                           const int32_t* d_nrows, int rstride, int kpstride, int32_t* d_mp_index_out);

/* ---- Monocular map initialisation: Initializer (src/Initializer.cc) -----------------------------------------------------------------
 * The step of Tracking::MonocularInitialization (src/Tracking.cc:659-760) behind SearchForInitialization (:696): the Initializer
 * constructor (src/Initializer.cc:33-42) and Initialize (:44-121) with everything it calls: max_its sets of eight matches, a homography
 * and a fundamental matrix from each set, both scored on every match, the winner of the ratio RH decomposed into 8 or 4 motion
 * hypotheses, each triangulated over the winner's inliers.  Parity: "HIP == host compile of the same header == restatement", parity
 * with OpenCV unpinned (DESIGN.md §3 lists the readings of the float SVD, the Mat products, inv, determinant and norm).  rand() is
 * glibc's generator; pair p is seeded as srand(seed0 + p) and takes 8 * max_its draws (the reference seeds once per process with 0 and
 * shares the stream: seed0 = 0, p = 0 is the first Initialize of a process; convention H7).
 * Cases the reference leaves undefined:
 *   - fewer than 8 matches: nothing is drawn or solved, status 0, nmatches the count, every other field 0 (the three indices -1);
 *   - no model: neither search has a hypothesis with a score above 0.0 (identical keypoints give sX = inf and NaN scores): status
 *     bit 2, nothing is reconstructed (the reference would hand an empty cv::Mat to ReconstructF);
 *   - a NaN in vCosParallax is ordered by its bit pattern: with the sign bit set below -inf, with it clear above +inf (std::sort
 *     is undefined there);
 *   - a match that names a keypoint outside frame 2 (matches12[i] >= nkeys2): status PSLFE_E_INVALID for that pair.
 *   FindFundamental sizes its vectors from the still empty vbMatchesInliers (:178); CheckFundamental resizes them (:404). */
typedef struct PslInitResult {   /* per pair */
    int32_t status;            /* bit 0: Initialize returned true; bit 1: the homography branch was taken (RH > 0.40, :115); bit 2: no
                                  model; or PSLFE_E_CAPACITY / PSLFE_E_INVALID for a count above its stride / a negative count or a match
                                  outside frame 2 */
    int32_t nmatches;          /* mvMatches12.size() (:65) */
    float SH, SF, RH;          /* :101, :112 */
    int32_t best_it_h, best_it_f;   /* the iteration whose H / F won (:165, :216), -1: none */
    int32_t inliers_h, inliers_f;   /* set flags of vbMatchesInliersH / F */
    float H21[9], F21[9];      /* the winners, zeros without one */
    int32_t ngood[8];          /* nGood of every CheckRT (:494-497: four; :703: eight) */
    float parallax[8];
    int32_t best_hypothesis;   /* ReconstructH: bestSolutionIdx (:709); ReconstructF: the hypothesis of the else-if ladder (:523-567),
                                  -1 when the ladder is not reached */
    float R21[9], t21[3];      /* zeros unless bit 0 */
    int32_t ntriangulated;     /* set flags of vbTriangulated */
} PslInitResult;
#ifdef __cplusplus
static_assert(sizeof(PslInitResult) == 228, "Initializer POD");
#else
_Static_assert(sizeof(PslInitResult) == 228, "Initializer POD");
#endif
/* == mvSets (src/Initializer.cc:77-97) on the host: srand(seed), then max_its sets of 8 from RandomInt(0, size - 1) on
 *    vAvailableIndices with swap-with-back removal; sets [max_its][8].  N < 8, max_its < 0 or NULL sets: PSLFE_E_INVALID.  Touches no
 *    device. */
int pslfe_init_sets(uint32_t seed, int N, int max_its, int32_t* sets);
/* == Initializer(ReferenceFrame, sigma, max_its) + Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated)
 *    (src/Initializer.cc:33-121) for npairs independent frame pairs in one launch, HBM to HBM.  Pair p: d_nkeys1[p] keypoints of the
 *    reference frame at d_keys1 + p * kstride * key_stride_bytes and d_nkeys2[p] of the current frame at d_keys2 + ... ; a keypoint is
 *    two floats (mvKeysUn[i].pt.x, .y) at the start of an element of key_stride_bytes (a multiple of 4, >= 8): plain float pairs or
 *    PslKeyPoint records.  d_matches12 + p * mstride: vMatches12, one entry per reference keypoint (-1: none).  cam: fx, fy, cx, cy
 *    (mK, :35); sigma, max_its: the constructor's (Tracking: 1.0, 200).  minParallax = 1.0 and minTriangulated = 50 as at :116-118.
 *    Outputs: d_res[p]; d_p3d [npairs][mstride][3] (vP3D) and d_triangulated [npairs][mstride] bytes (vbTriangulated), indexed by
 *    reference keypoint, the first d_nkeys1[p] entries of a pair written: zeros unless Initialize returned true; d_matches12_out
 *    (may be NULL) [npairs][mstride]: mvIniMatches after src/Tracking.cc:712-719, i.e. vMatches12 with -1 where a match was not
 *    triangulated when Initialize returned true, vMatches12 otherwise.  Bytes beyond the counts are not touched.
 *    d_nkeys1[p] or d_nkeys2[p] > kstride, d_nkeys1[p] > mstride: status = PSLFE_E_CAPACITY; a negative count, a match >= d_nkeys2[p]:
 *    PSLFE_E_INVALID; nothing is clamped, nothing is solved, no output byte of that pair but its record is written (other fields 0).
 *    npairs < 0, kstride < 0, mstride < 0, max_its < 1, a NaN sigma, a bad key_stride_bytes, a NULL array with a non-zero count:
 *    PSLFE_E_INVALID; npairs == 0: PSLFE_OK, nothing is done.  Asynchronous on the context's stream; per-call buffers come from the
 *    scratch arena. */
int pslfe_init_initialize_device(pslfe_ctx* ctx, int npairs, const void* d_keys1, const int32_t* d_nkeys1, const void* d_keys2,
                                 const int32_t* d_nkeys2, int key_stride_bytes, int kstride, const int32_t* d_matches12, int mstride,
                                 const PslCamera* cam, float sigma, int max_its, uint32_t seed0, PslInitResult* d_res, float* d_p3d,
                                 uint8_t* d_triangulated, int32_t* d_matches12_out);
/* Same with the keypoints of frame slots: pair p has the reference frame in slot slot1[p] of f1 and the current frame in slot
 * slot2[p] of f2 (host int arrays, as for pslfe_orb_search_for_initialization_device, whose d_matches12 this call takes as it is;
 * mstride >= f1's capacity, PSLFE_E_INVALID otherwise; a slot that is not set: PSLFE_E_STATE).  Returns once the slot tables have been
 * copied; the solver is queued on the context's stream. */
int pslfe_init_initialize_frames_device(pslfe_frame* f1, const int32_t* slot1, pslfe_frame* f2, const int32_t* slot2, int npairs,
                                        const int32_t* d_matches12, int mstride, const PslCamera* cam, float sigma, int max_its,
                                        uint32_t seed0, PslInitResult* d_res, float* d_p3d, uint8_t* d_triangulated,
                                        int32_t* d_matches12_out);
/* One pair, host arrays: keys1 [n1][2], keys2 [n2][2] floats, matches12 [n1]; res, p3d [n1][3], triangulated [n1]; returns after the
 * results have arrived.  A negative status of the pair is also the return value. */
int pslfe_init_initialize(pslfe_ctx* ctx, const float* keys1, int n1, const float* keys2, int n2, const int32_t* matches12,
                          const PslCamera* cam, float sigma, int max_its, uint32_t seed, PslInitResult* res, float* p3d,
                          uint8_t* triangulated);

/* For the tests: the order of vCosParallax and the kernel's selection alone.  cosines [n >= 1] (host) -> keys [n] (the ordered keys:
 * ascending keys are the stated order, NaNs included), *selected = the cosine at sorted index min(50, n - 1), *parallax = its
 * acos * 180 / CV_PI (src/Initializer.cc:898-901).  Synchronous. */
int pslfe_init_debug_select(pslfe_ctx* ctx, const float* cosines, int n, uint32_t* keys, float* selected, float* parallax);

/* ---- Local bundle adjustment: the point edges of Optimizer::LocalBundleAdjustment ---------------------------------------------------
 * Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1025-1966, the call of LocalMapping::Run src/LocalMapping.cc:84) and the
 * EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ part of LocalBundleAdjustmentAndInseclines (:1968-2534) from the optimiser's set-up on:
 * the two rounds optimize(5) with Huber and optimize(10) without the outliers (:1642-1790, :2356-2456) over g2o's Levenberg, the
 * Schur complement of BlockSolver<6,3> and a dense solve of the reduced camera system.  The VertexLIL vertices are not part of these entry points (pslfe_ba_local_lil[_device] below add them).
 * Building the lists (lLocalKeyFrames, lFixedCameras, lLocalMapPoints) and the tail (erase, SetPose, SetWorldPos) stay host code:
 * INTEGRATION.md "LocalBundleAdjustment".  Parity: "HIP == host compile of the same header == restatement", bit for bit; parity with
 * g2o itself is unpinned (DESIGN.md §3 lists what is pinned to g2o's text and what is this library's reading: the 3x3 inverse, the
 * dense LDLt in place of LinearSolverEigen, the block order).  The abort flag inside optimize() is not modelled; rounds = 1 is
 * bDoMore == false (:1645-1651).
 * Blocks follow the caller's row order: a caller who wants g2o's index mapping passes keyframes and points in ascending mnId.
 * Edges are given in the order the reference creates them (per map point, its observations in GetObservations() order): that
 * order is the order of every sum. */
typedef struct PslBaEdge {
    int32_t point, kf;           /* rows of the problem's point and keyframe arrays */
    float u, v, ur, inv_sigma2;  /* kpUn.pt, mvuRight (ur < 0: a monocular edge), mvInvLevelSigma2[kpUn.octave] */
} PslBaEdge;
typedef struct PslBaKeyFrame {
    PslPose Tcw;                 /* GetPose() */
    int32_t fixed;               /* mnId == 0 or a keyframe of lFixedCameras */
} PslBaKeyFrame;
typedef struct PslBaInfo {
    int32_t status;              /* PSLFE_OK, PSLFE_E_CAPACITY or PSLFE_E_INVALID of this problem */
    int32_t rounds;              /* rounds run: 0 (nothing to optimise or a refused problem), 1 or 2 */
    int32_t iterations[2];
    int32_t nerased;             /* set erase bytes */
    double chi2_start, chi2_round1, chi2_end;   /* the active robust chi2 before round one, after it (under Huber) and after the last round */
} PslBaInfo;
#ifdef __cplusplus
static_assert(sizeof(PslBaEdge) == 24 && sizeof(PslBaKeyFrame) == 52 && sizeof(PslBaInfo) == 48, "local BA PODs");
#else
_Static_assert(sizeof(PslBaEdge) == 24 && sizeof(PslBaKeyFrame) == 52 && sizeof(PslBaInfo) == 48, "local BA PODs");
#endif
typedef struct pslfe_ba pslfe_ba;
/* The HBM workspaces of up to max_problems problems per launch, each of up to max_keyframes keyframes (free and fixed), max_points
 * points and max_edges edges: per edge the Jacobian and error rows and the Hpl block, Hpp, Hll, Dinv, S (N x N doubles, N = 6 x
 * max_keyframes), b, x, the candidate estimates and the four edge lists.  A count below 1 or a NULL argument: PSLFE_E_INVALID. */
int pslfe_ba_create(pslfe_ctx* ctx, int max_problems, int max_keyframes, int max_points, int max_edges, pslfe_ba** out);
void pslfe_ba_destroy(pslfe_ba* ba);
/* == the optimisation of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1642-1790 with the vertices and edges of :1100-1640 given
 *    as rows) for K independent problems in one launch, HBM to HBM.  Problem k has the keyframes d_kf[d_kf_off[k] .. d_kf_off[k+1]),
 *    the points d_mp[d_mp_off[k] ..) (only x, y, z are read and written; the other fields are copied) and the edges
 *    d_edges[d_edge_off[k] ..), whose point / kf are rows of that problem.  The offset arrays have K+1 ascending entries.  cam: fx, fy,
 *    cx, cy, bf (host).  rounds: 2, or 1 for bDoMore == false.  Outputs, indexed as the inputs: d_kf_out (free keyframes: toCvMat of
 *    the optimised SE3Quat, also when nothing moved them, as SetPose gets it; fixed ones: the input), d_mp_out, d_erase (one byte per
 *    edge: vToErase, :1755, :1770), d_info[k].  d_kf_out may be d_kf and d_mp_out may be d_mp.
 *    Per problem, in d_info[k].status, never a silent truncation: a count above the handle's caps: PSLFE_E_CAPACITY; descending or
 *    negative offsets, an edge that names a row outside its problem, or a duplicate (point, keyframe) pair: PSLFE_E_INVALID; such a
 *    problem leaves its outputs equal to its inputs (erase bytes 0), rounds = 0, and does not disturb its neighbours.  No free
 *    keyframe, or no edge: PSLFE_OK with rounds = 0, outputs equal to inputs bit for bit (g2o is never called that way: the reference
 *    always has pKF itself and its observations).
 *    Whole call, before any device is touched: K < 0, rounds outside 1..2, K > max_problems, a NULL argument with K > 0:
 *    PSLFE_E_INVALID; K == 0: PSLFE_OK, nothing is done.  Asynchronous on the context's stream. */
int pslfe_ba_local_device(pslfe_ba* ba, int K, const PslBaKeyFrame* d_kf, const int32_t* d_kf_off, const PslMapPointGeom* d_mp,
                          const int32_t* d_mp_off, const PslBaEdge* d_edges, const int32_t* d_edge_off, const PslCamera* cam, int rounds,
                          PslBaKeyFrame* d_kf_out, PslMapPointGeom* d_mp_out, uint8_t* d_erase, PslBaInfo* d_info);
/* One problem, host arrays; returns after the results have arrived.  Negative counts, NULL with a non-zero count, rounds outside
 * 1..2: PSLFE_E_INVALID before any device is touched.  A negative status of the problem is also the return value. */
int pslfe_ba_local(pslfe_ba* ba, const PslBaKeyFrame* kf, int nkf, const PslMapPointGeom* mp, int nmp, const PslBaEdge* edges, int nedges,
                   const PslCamera* cam, int rounds, PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* erase, PslBaInfo* info);

/* ---- Local bundle adjustment with the VertexLIL vertices: Optimizer::LocalBundleAdjustmentAndInseclines ------------------------------
 * The call LocalMapping::Run makes (src/LocalMapping.cc:84; src/Optimizer.cc:1968-2534): the point edges above plus one VertexLIL per
 * local InsectLine (:2250-2290: 15 doubles, marginalised, ids above every map point id, so the LILs follow the points) and one
 * EdgeLILSE3ProjectXYZ per (LIL, observing keyframe) (:2295-2346, add_inc/EdgeLIL.h:210-439), created after all point edges:
 * information 0.01 * I6 (`double invSigma = 0.01`, :1970), Huber with delta (float)sqrt(11.07), levels and erase flags by
 * `chi2() > 11.07 || !isDepthPositive()` in double (:2401-2414, :2464-2478).  VertexLIL::oplusImpl adds FIFTEEN doubles of the update
 * vector to a vertex that owns three (add_inc/VertexLIL.h:23-27, sparse_optimizer.cpp:425-434): segment m of an active LIL receives the
 * step of the m-th next active LIL; past the end of the active update vector this library reads 0.0, where the reference's value is
 * indeterminate (solver.cpp:51-57) - parity at the last four active LILs is unpinned even against a g2o build. */
typedef struct PslBaLilEdge {
    int32_t lil, kf;             /* rows of the problem's LIL and keyframe arrays */
    double obs1[3];              /* pKF->mvle_l[idx].first  (src/Optimizer.cc:2305-2307) */
    double obs2[3];              /* pKF->mvle_l[idx].second */
    double obs_ins[2];           /* pKF->CrossPoint_2D[idx] */
} PslBaLilEdge;
#ifdef __cplusplus
static_assert(sizeof(PslBaLilEdge) == 72, "local BA LIL edge");
#else
_Static_assert(sizeof(PslBaLilEdge) == 72, "local BA LIL edge");
#endif
/* pslfe_ba_create with room for up to max_lils LILs and max_lil_edges LIL edges per problem (both >= 0).  A handle from
 * pslfe_ba_create has LIL caps of 0: a problem with a LIL row or a LIL edge is refused with PSLFE_E_CAPACITY. */
int pslfe_ba_create_lil(pslfe_ctx* ctx, int max_problems, int max_keyframes, int max_points, int max_edges, int max_lils, int max_lil_edges,
                        pslfe_ba** out);
/* == pslfe_ba_local_device with the LILs of src/Optimizer.cc:2250-2533.  Problem k has also the LIL rows d_lil[d_lil_off[k] ..)
 *    (PslMapLil: w is read and written, `bad` is copied and not read - the pML->isBad() skip is the caller's) and the LIL edges
 *    d_lil_edges[d_lil_edge_off[k] ..) in the order the reference creates them.  Outputs: d_lil_out (the 15 doubles of every LIL,
 *    :2526-2531; a LIL without an edge is copied; may be d_lil; it is what pslfe_pose_lil_edges_device reads as d_map), d_erase_lil
 *    (one byte per LIL edge, :2464-2478), d_nerased_lil (may be NULL: the set bytes of d_erase_lil per problem).  d_info[k]: its chi2
 *    values cover both kinds of edges, nerased counts point edges.  nmp == 0 is allowed.  Per problem: a LIL edge that names a row
 *    outside the problem or a duplicate (LIL, keyframe) pair: PSLFE_E_INVALID; counts above the caps: PSLFE_E_CAPACITY; such a
 *    problem leaves all three outputs equal to its inputs.  With every LIL count 0 the results are the bytes of
 *    pslfe_ba_local_device.  The whole-call rules are those of pslfe_ba_local_device (every array but d_nerased_lil is required). */
int pslfe_ba_local_lil_device(pslfe_ba* ba, int K, const PslBaKeyFrame* d_kf, const int32_t* d_kf_off, const PslMapPointGeom* d_mp,
                              const int32_t* d_mp_off, const PslBaEdge* d_edges, const int32_t* d_edge_off, const PslMapLil* d_lil,
                              const int32_t* d_lil_off, const PslBaLilEdge* d_lil_edges, const int32_t* d_lil_edge_off, const PslCamera* cam,
                              int rounds, PslBaKeyFrame* d_kf_out, PslMapPointGeom* d_mp_out, uint8_t* d_erase, PslMapLil* d_lil_out,
                              uint8_t* d_erase_lil, int32_t* d_nerased_lil, PslBaInfo* d_info);
/* One problem, host arrays, as pslfe_ba_local. */
int pslfe_ba_local_lil(pslfe_ba* ba, const PslBaKeyFrame* kf, int nkf, const PslMapPointGeom* mp, int nmp, const PslBaEdge* edges, int nedges,
                       const PslMapLil* lil, int nlil, const PslBaLilEdge* lil_edges, int nlil_edges, const PslCamera* cam, int rounds,
                       PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* erase, PslMapLil* lil_out, uint8_t* erase_lil, PslBaInfo* info);

/* ---- Global bundle adjustment: Optimizer::BundleAdjustment / GlobalBundleAdjustemnt ------------------------------------------------
 * src/Optimizer.cc:37-237: the call of Tracking::CreateInitialMapMonocular (src/Tracking.cc:782, 20 iterations, robust) and of
 * LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:650, 10 iterations, bRobust = false), from the optimiser's set-up on: one
 * optimize(nIterations) over g2o's Levenberg with BlockSolver_6_3, no levels, no erase pass.  ONE problem spread over the whole
 * device (the local BA gives a workgroup to each of K problems).  The arithmetic, the order of every sum and the readings of
 * DESIGN.md §3 are those of the local BA above; parity is "HIP == host compile of the same headers == restatement", bit for bit.
 * Rows: PslBaKeyFrame (fixed = mnId == 0, :79), PslMapPointGeom and PslBaEdge in the order the reference creates the edges
 * (:89-173: per map point, its observations in GetObservations() order).  Bad keyframes, bad points and observations in bad
 * keyframes are the caller's filter (:74, :92, :109), as is the choice between SetPose / SetWorldPos and mTcwGBA / mPosGBA (nLoopKF,
 * :200-210, :224-234).  The abort flag (pbStopFlag) is not modelled. */
typedef struct PslGbaInfo {
    int32_t status;              /* PSLFE_OK, PSLFE_E_CAPACITY or PSLFE_E_INVALID */
    int32_t iterations;          /* iterations run */
    int32_t free_keyframes;      /* F: pose blocks of the system (not fixed, with an edge) */
    int32_t included_points;     /* points with at least one edge */
    double chi2_start, chi2_end, lambda;   /* the active (robust) chi2 of iteration 0 and at the end; the lambda then */
} PslGbaInfo;
#ifdef __cplusplus
static_assert(sizeof(PslGbaInfo) == 40, "global BA POD");
#else
_Static_assert(sizeof(PslGbaInfo) == 40, "global BA POD");
#endif
typedef struct pslfe_gba pslfe_gba;
/* The HBM workspace of one problem of up to max_keyframes keyframes (at most 4096: S has 36 max_keyframes^2 doubles, counted in
 * size_t), max_points points and max_edges edges (at most 2^26 each: every index of a step is an int).  A count below 1, above
 * these bounds or a NULL argument: PSLFE_E_INVALID. */
int pslfe_gba_create(pslfe_ctx* ctx, int max_keyframes, int max_points, int max_edges, pslfe_gba** out);
void pslfe_gba_destroy(pslfe_gba* gba);
/* == Optimizer::BundleAdjustment (src/Optimizer.cc:49-237) on rows in HBM.  cam: fx, fy, cx, cy, bf (host).  iterations >= 1 (the
 *    reference passes 5, 10 or 20).  robust: 1 sets Huber on every edge with THIS function's deltas, (float)sqrt(5.99) =
 *    2.4474475383758545 for a monocular edge (:85; not the local BA's (float)sqrt(5.991)) and (float)sqrt(7.815) for a stereo
 *    edge (:86); 0 runs without a kernel.
 *    Outputs, indexed as the inputs: d_kf_out: EVERY keyframe gets toCvMat of its SE3Quat, the fixed ones and those without an edge
 *    too (the reference calls SetPose or fills mTcwGBA for every keyframe, :193-210), so a fixed keyframe comes back through the
 *    quaternion; this differs from pslfe_ba_local, which leaves fixed rows alone.  d_not_included[p] = vbNotIncludedMP (:175-183): 1
 *    when point p has no edge.  d_mp_out: an included point gets (float) of its estimate in x, y, z; the other points and fields
 *    keep their values; it is what pslfe_kf_update_normal_and_depth_device (:227) and ComputeSceneMedianDepth take.  d_kf_out may
 *    be d_kf and d_mp_out may be d_mp.
 *    info is a HOST pointer.  The call drives the Levenberg loop from the host (a decision is a small read-back, a step a launch
 *    over the whole device on the context's stream) and returns when the outputs are written.
 *    Never a silent truncation: a count above the handle's caps: PSLFE_E_CAPACITY; an edge that names a row outside the problem
 *    or a duplicate (point, keyframe) pair: PSLFE_E_INVALID; both are the return value and info->status, the outputs then equal
 *    the inputs and d_not_included is 0.  No edge, or no free keyframe with an edge: PSLFE_OK with 0 iterations; the keyframes
 *    are still round-tripped.  Negative counts, NULL with a non-zero count (gba, cam and info always), iterations < 1, robust
 *    outside 0..1: PSLFE_E_INVALID before any device is touched. */
int pslfe_gba_optimize_device(pslfe_gba* gba, const PslBaKeyFrame* d_kf, int nkf, const PslMapPointGeom* d_mp, int nmp, const PslBaEdge* d_edges,
                              int nedges, const PslCamera* cam, int iterations, int robust, PslBaKeyFrame* d_kf_out, PslMapPointGeom* d_mp_out,
                              uint8_t* d_not_included, PslGbaInfo* info);
/* The same on host arrays, as pslfe_ba_local. */
int pslfe_gba_optimize(pslfe_gba* gba, const PslBaKeyFrame* kf, int nkf, const PslMapPointGeom* mp, int nmp, const PslBaEdge* edges, int nedges,
                       const PslCamera* cam, int iterations, int robust, PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* not_included,
                       PslGbaInfo* info);

/* ---- The essential graph: Optimizer::OptimizeEssentialGraph -----------------------------------------------------------------------
 * The call of LoopClosing::CorrectLoop (src/LoopClosing.cc, src/Optimizer.cc:2536-2799) from the vertices on: the measurements of
 * the EdgeSim3 edges (:2607-2738), optimize(20) over g2o's Levenberg with setUserLambdaInit(1e-16) (:2549, :2741-2742), the pose
 * recovery (:2747-2765) and the map point correction (:2768-2798, up to SetWorldPos; UpdateNormalAndDepth is
 * pslfe_kf_update_normal_and_depth_device on d_mp_out).  Walking the pointer graph (the spanning tree, the loop edges, the
 * covisibility lists, LoopConnections, the two Sim3 maps) stays host code: the mirrors' edge builder, INTEGRATION.md "CorrectLoop".
 * Parity: "HIP == host compile of the same header == restatement" (tests/essential_cases.py), bit for bit; parity with g2o itself is
 * unpinned (LinearSolverEigen is an LDLt without pivoting on row envelopes in the caller's row order, the
 * 3x3 LU of Sim3::log and the order of every sum are this library's reading).  The global bundle adjustment CorrectLoop starts
 * afterwards is not part of the library. */
typedef struct PslEgKeyFrame {   /* a keyframe that is not bad, rows in ascending mnId (:2564-2599) */
    double Scw[8];               /* vScw: q x y z w (not normalised), t, s: the CorrectedSim3 entry or Sim3(Rcw, tcw, 1.0) (:2573-2587) */
    double Snc[8];               /* the NonCorrectedSim3 entry; read only when has_nc is set */
    int32_t has_nc;              /* NonCorrectedSim3.find(pKF) != end() (:2646, :2662, :2689, :2720) */
    int32_t fixed;               /* pKF == pLoopKF (:2589) */
} PslEgKeyFrame;
typedef struct PslEgEdge {       /* in the order the reference creates them (:2607-2738) */
    int32_t i, j;                /* rows of the graph's keyframes: vertex 0 = i, vertex 1 = j */
    int32_t loop;                /* 1: an edge of LoopConnections (:2607-2635), measured with vScw of both ends */
} PslEgEdge;
typedef struct PslEgInfo {
    int32_t status;              /* PSLFE_OK, PSLFE_E_CAPACITY or PSLFE_E_INVALID of this graph */
    int32_t iterations;          /* Levenberg iterations run (0 .. 20) */
    int32_t log_branches;        /* bit k set when an evaluation of Sim3::log took branch k = (|sigma| >= 1e-5) * 2 + !(d > 1 - 1e-5) */
    int32_t nfree;               /* free keyframes: the system has 7 nfree unknowns */
    double chi2_start, chi2_end; /* the chi2 of all edges before the first iteration and after the last */
    double lambda;               /* the damping when the call returned */
} PslEgInfo;
#ifdef __cplusplus
static_assert(sizeof(PslEgKeyFrame) == 136 && sizeof(PslEgEdge) == 12 && sizeof(PslEgInfo) == 40, "essential graph PODs");
#else
_Static_assert(sizeof(PslEgKeyFrame) == 136 && sizeof(PslEgEdge) == 12 && sizeof(PslEgInfo) == 40, "essential graph PODs");
#endif
typedef struct pslfe_eg pslfe_eg;
/* The HBM workspaces of up to max_graphs graphs per launch, each of up to max_keyframes keyframes, max_edges edges, max_points map
 * points and max_envelope doubles of envelope: the lower triangle of H is stored per 7x7 block row from the lowest block column an
 * edge gives it to the diagonal, sum over the scalar rows r of (r - 7 first_block(r) + 1) doubles (a chain: about 77 per free keyframe;
 * a loop edge adds 49 per keyframe it spans).  A count below 1 or a NULL argument: PSLFE_E_INVALID. */
int pslfe_eg_create(pslfe_ctx* ctx, int max_graphs, int max_keyframes, int max_edges, int max_points, int64_t max_envelope, pslfe_eg** out);
void pslfe_eg_destroy(pslfe_eg* eg);
/* == the optimisation, the pose recovery and the point correction of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2607-2798
 *    with the vertices and edges given as rows) for K independent graphs in one launch, HBM to HBM.  Graph k has the keyframes
 *    d_kf[d_kf_off[k] .. d_kf_off[k+1]), the edges d_edges[d_edge_off[k] ..) and the points d_mp[d_mp_off[k] ..) with
 *    d_mp_ref[same index] = the keyframe row nIDr of :2775-2784 (the mnCorrectedByKF test is the caller's) or -1 for a point that
 *    is copied unchanged (a bad one).  The offset arrays have K+1 ascending entries.  fix_scale: bFixScale.
 *    Outputs, indexed as the inputs: d_pose_out (Tiw of :2762 for EVERY keyframe), d_S_out ([8] doubles per keyframe: the optimised
 *    Sim3, laid out as Scw), d_mp_out (x, y, z corrected, the other fields copied; may be d_mp; it is what
 *    pslfe_kf_update_normal_and_depth_device takes), d_info[k].
 *    Per graph, in d_info[k].status, never a silent truncation: counts or an envelope above the handle's caps: PSLFE_E_CAPACITY;
 *    descending or negative offsets, an edge that names a row outside its graph or has i == j, a point whose reference row is
 *    below -1 or not a row of its graph: PSLFE_E_INVALID; such a graph gets d_S_out = its Scw and d_mp_out = its d_mp, no pose row
 *    is written, and its neighbours are not disturbed.  Any number of keyframes may be fixed.  No free keyframe, or no edge:
 *    PSLFE_OK with 0 iterations; the poses and points then come from the Sim3s as given.  A free keyframe without an edge gets a
 *    zero block plus lambda and a zero step.
 *    Whole call, before any device is touched: K < 0, K > max_graphs, a NULL argument with K > 0: PSLFE_E_INVALID; K == 0:
 *    PSLFE_OK, nothing is done.  Asynchronous on the context's stream. */
int pslfe_eg_optimize_device(pslfe_eg* eg, int K, const PslEgKeyFrame* d_kf, const int32_t* d_kf_off, const PslEgEdge* d_edges,
                             const int32_t* d_edge_off, const PslMapPointGeom* d_mp, const int32_t* d_mp_ref, const int32_t* d_mp_off,
                             int fix_scale, PslPose* d_pose_out, double* d_S_out, PslMapPointGeom* d_mp_out, PslEgInfo* d_info);
/* One graph, host arrays; returns after the results have arrived.  Negative counts or NULL with a non-zero count: PSLFE_E_INVALID
 * before any device is touched.  A negative status of the graph is also the return value. */
int pslfe_eg_optimize(pslfe_eg* eg, const PslEgKeyFrame* kf, int nkf, const PslEgEdge* edges, int nedges, const PslMapPointGeom* mp,
                      const int32_t* mp_ref, int nmp, int fix_scale, PslPose* pose_out, double* S_out, PslMapPointGeom* mp_out, PslEgInfo* info);

/* ---- RGB-D line glue of the Frame constructor ------------------------------ */
typedef struct pslfe_glue pslfe_glue;
/* Buffers for up to max_batch frames of max_lines keylines and max_fans LIL rows each. */
int pslfe_glue_create(pslfe_ctx* ctx, int max_lines, int max_fans, int max_batch, pslfe_glue** out);
void pslfe_glue_destroy(pslfe_glue* g);
/* == the part of Frame::ExtractLSD after the extractor (src/Frame.cc:490-660) for one frame, host pointers:
 *    Frame::isLineGood(im, imDepth, K) :662-750 with LINEextractor::compPt3dCov / extract3dline_mahdist
 *    (add_src/LineExtractor.cpp:40-322): per keyline <= 21 depth samples, back-projection, RANSAC 3-D line by
 *    Mahalanobis distance -> mvLines3D, mvLineEq;
 *    Frame::convertFansToKeyLines(fans, mvKeylinesUn) :426-472 with Frame_shortestDistance :381-424 ->
 *    intersection_lines_plane; the plane loop :505-660 with Frame::OldPlane :474-488 -> mvPlanes, mvPlaneNormal,
 *    mvPlaneLineNo, CrossPoint_3D, CrossPoint_2D, mvle_l.
 *    kls: mvKeylinesUn (n); fans: the n x 4 matrix of CPartiallyRecoverConnectivity (x, y, index1, index2);
 *    depth: CV_32F image (metres), stride in floats; cam: fx, fy, cx, cy are used.
 *    rand() is glibc's generator seeded as srand(seed) at the start of the frame (the reference never seeds: its
 *    stream position depends on the process history; convention H7).  Asynchronous; results via pslfe_glue_fetch. */
int pslfe_glue_run(pslfe_glue* g, const PslKeyLine* kls, int nlines, const float* fans, int nfans, const float* depth,
                   int width, int height, int depth_stride, const PslCamera* cam, uint32_t seed);
/* Same for nframes frames resident in HBM: keylines [nframes][kl_stride] (kl_stride == max_lines), counts
 * [nframes], fans [nframes][fan_stride][4], counts [nframes], depth [nframes][height][width] float; frame f is
 * seeded with seed0 + f.  (pslfe_line_results_device / pslfe_line_pair_batch_device give exactly these views.)
 * Counts that the views cannot hold are clamped, not refused (they live in HBM): frame f uses its first
 * min(d_nkl[f], kl_stride) keylines and its first min(d_nfans[f], fan_stride) fan rows; a negative count is an empty frame.
 * Fan-index contract: a fan row that names a line outside [0, min(d_nkl[f], kl_stride)) yields no crossing and is not counted
 * (pslfe_glue_run refuses such a row with PSLFE_E_INVALID; this entry point cannot look at the rows).  The rows of mvLines3D /
 * mvLineEq past a frame's count are not written by a launch, so they are never read by it either. */
int pslfe_glue_run_batch_device(pslfe_glue* g, int nframes, const PslKeyLine* d_kls, int kl_stride, const int32_t* d_nkl,
                                const float* d_fans, int fan_stride, const int32_t* d_nfans, const float* d_depth,
                                int width, int height, const PslCamera* cam, uint32_t seed0);
/* Results of frame `frame` (any pointer may be NULL):
 *   lines3d [nlines][6] f64 = mvLines3D (start, end; zeros when the line failed), lineEq [nlines][3] = mvLineEq
 *   (-1,-1,-1 when failed); crossings (intersection_lines_plane, fan order): pair [k][2], xy [k][2], cross [k][3]
 *   f64, le_l [k][6] f64 = mvle_l; planes: planes [p][4] = mvPlanes, normals [p][3] f64 = mvPlaneNormal, lineNo
 *   [p][2] = mvPlaneLineNo, cross3d [p][3] = CrossPoint_3D, cross2d [p][2] f64 = CrossPoint_2D. */
int pslfe_glue_fetch(pslfe_glue* g, int frame, int nlines, double* lines3d, float* lineEq, int32_t* pair, float* xy,
                     double* cross, double* le_l, int int_cap, int* nint, float* planes, double* normals, int32_t* lineNo,
                     double* cross3d, double* cross2d, int plane_cap, int* nplanes);

/* ---- batched many-frames mode across the GPUs of one node (BASELINE configs[3]) -----------------------
 * The reference has no counterpart (it is single-process, single-camera: src/System.cc:91-101); north_star asks for
 * independent frames / streams sharded over the 8 GPUs with RCCL over xGMI for the result gather.  Stream s -> rank
 * s mod world, no data-path collective; the one exchange is a gather (to the consuming rank, or to all) of fixed-size per-frame
 * RESULT RECORDS holding what Tracking.cc reads of a Frame on this path.  Record (little endian, sections 16-byte aligned, zero padded):
 *   header  8 x int32: n_kp, n_match, n_kl, n_lmatch, n_fan, n_planes (true counts), flags (bit0 kps / bit1 lines / bit2 fans /
 *           bit3 planes truncated to the capacity), frame index inside the rank's batch
 *   kps     [kp_cap] PslKeyPoint    = mvKeys               desc   [kp_cap][32] = mDescriptors
 *   match   [kp_cap] int32          = ORBmatcher::SearchByProjection result (query i -> keypoint of this frame, -1 none; all kp_cap rows of the
 *                                     caller's buffer, which holds -1 beyond the query count; rows beyond match_stride read -1)
 *   kls     [kl_cap] PslKeyLine     = mvKeylinesUn         ldesc  [kl_cap][32] = mLdesc
 *   lineEq  [kl_cap][3] f64         = mvKeyLineFunctions   lmatch [kl_cap] int32 = LSDmatcher::match result
 *   fans    [fan_cap][4] f32        = CPartiallyRecoverConnectivity rows (x, y, i, j)
 *   planes  [plane_cap][4] f32      = mvPlanes             plane_lines [plane_cap][2] int32 = mvPlaneLineNo          */
typedef struct PslRecordCaps { int32_t kp_cap, kl_cap, fan_cap, plane_cap; } PslRecordCaps;
typedef struct PslRecordLayout {
    int64_t bytes;  /* size of one record, a multiple of 256 */
    int64_t off_kps, off_desc, off_match, off_kls, off_ldesc, off_lineEq, off_lmatch, off_fans, off_planes, off_plane_lines;
} PslRecordLayout;
/* Pure host arithmetic (no GPU needed): the offsets every consumer of a record uses. */
int pslfe_record_layout(const PslRecordCaps* caps, PslRecordLayout* out);
/* Where the results of a batch live in HBM (the *_results_device / *_fans_device views and the caller's match buffers);
 * a NULL pointer leaves its section empty.  Strides are in rows per frame. */
typedef struct PslRecordSources {
    const PslKeyPoint* d_kps; const uint8_t* d_desc; const int32_t* d_kp_counts; int32_t kp_stride;
    const int32_t* d_match; const int32_t* d_nmatches; int32_t match_stride;
    const PslKeyLine* d_kls; const uint8_t* d_ldesc; const double* d_lineEq; const int32_t* d_kl_counts; int32_t kl_stride;
    const int32_t* d_lmatch; const int32_t* d_nlmatches; int32_t lmatch_stride;
    const float* d_fans; const int32_t* d_fan_counts; int32_t fan_stride;
    const float* d_planes; const int32_t* d_plane_lines; const int32_t* d_plane_counts; int32_t plane_stride;
} PslRecordSources;
/* Packs the records of nframes frames into d_records ([nframes][layout.bytes]), asynchronously on the context's stream. */
int pslfe_record_pack_device(pslfe_ctx* ctx, const PslRecordCaps* caps, const PslRecordSources* src, int nframes, void* d_records);
/* mvPlanes / mvPlaneLineNo / their counts of the last pslfe_glue_run_batch_device, HBM resident ([nframes][plane_stride][..]). */
/* Device view of the last batch's mvLines3D: [max_batch][stride][6] f64 (start, end), stride = max_lines. */
int pslfe_glue_lines3d_device(pslfe_glue* g, const double** d_lines3d, int* stride);
int pslfe_glue_planes_device(pslfe_glue* g, const float** d_planes, const int32_t** d_plane_lines, const int32_t** d_plane_counts,
                             int* plane_stride);
/* Device view of the last batch's mvle_l ([max_batch][le_stride][6] f64, one row per crossing, src/Frame.cc:517-528; d_ncross = the
 * crossings of each frame) and CrossPoint_2D ([max_batch][plane_stride][2] f64, one row per plane, :643; d_plane_counts as above):
 * what pslfe_pose_lil_edges_device reads (src/Optimizer.cc:658-660).  Any pointer may be NULL. */
int pslfe_glue_lil_obs_device(pslfe_glue* g, const double** d_le_l, int* le_stride, const int32_t** d_ncross, const double** d_cross2d,
                              int* plane_stride, const int32_t** d_plane_counts);

/* RCCL gather of the records, one communicator per context.  RCCL is loaded at run time (librccl.so.1).
 *   pslfe_gather_unique_id  rank 0 obtains the 128-byte ncclUniqueId and hands it to the other ranks by whatever channel the
 *                           host has (MPI, a socket, torch.distributed, a file);
 *   pslfe_gather_create     ncclCommInitRank - collective: every rank calls it with the same id;
 *   pslfe_gather_all        d_recv[world][bytes_per_rank] <- every rank's d_send[bytes_per_rank]; runs on the gather's own
 *                           stream AFTER everything issued on the context's stream so far, so the next batch's kernels
 *                           overlap it; one exchange may be in flight;
 *   pslfe_gather_to_root    the same towards ONE consuming rank (SURVEY.md §8e "ncclGather-by-send/recv"): rank `root` receives
 *                           d_recv[world][bytes_per_rank] (its own part included), the other ranks only send and need no receive
 *                           buffer (d_recv may be NULL there) - one group of ncclSend / ncclRecv; collective: every rank of the
 *                           communicator calls it with the same root and bytes_per_rank;
 *   pslfe_gather_wait       host_blocking != 0: the host waits for the exchange; 0: the context's stream waits for it (the host
 *                           may read the received records only after a host-blocking wait). */
typedef struct pslfe_gather pslfe_gather;
int pslfe_gather_unique_id(uint8_t id[128]);
int pslfe_gather_create(pslfe_ctx* ctx, int rank, int world, const uint8_t id[128], pslfe_gather** out);
void pslfe_gather_destroy(pslfe_gather* g);
int pslfe_gather_all(pslfe_gather* g, const void* d_send, size_t bytes_per_rank, void* d_recv);
int pslfe_gather_to_root(pslfe_gather* g, const void* d_send, size_t bytes_per_rank, int root, void* d_recv);
int pslfe_gather_wait(pslfe_gather* g, int host_blocking);
int pslfe_gather_world(const pslfe_gather* g, int* rank, int* world);

#ifdef __cplusplus
}
#endif
#endif
