// C++ host-side mirror of the reference's extractor / matcher classes over the C ABI
// (include/pslfe.h).  Header-only, no OpenCV: keypoints are PslKeyPoint (layout == cv::KeyPoint),
// descriptors std::vector<uint8_t> (N x 32 row-major == cv::Mat N x 32 CV_8U).  The OpenCV-typed
// adapter a PSL-SLAM maintainer adds on top is shown in INTEGRATION.md.
//
// Names, argument meaning and error behaviour follow the reference:
//   ORBextractor  include/ORBextractor.h:45-114   (operator(), getters)
//   ORBmatcher    include/ORBmatcher.h:36-104     (SearchByProjection, DescriptorDistance, TH_*)
//   LSDmatcher    add_inc/LSDmatcher.h:18-75      (matchNNR / match)
#ifndef PSLFE_HPP
#define PSLFE_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pslfe.h"

namespace pslfe {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what + ": " + pslfe_last_error()), code(c) {}
};
inline void check(int rc, const char* what) { if (rc != PSLFE_OK) throw Error(rc, what); }

class Context {
public:
    explicit Context(int device = 0) : device_(device) { check(pslfe_ctx_create(device, &h_), "pslfe_ctx_create"); }
    int device() const { return device_; }
    ~Context() { pslfe_ctx_destroy(h_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    pslfe_ctx* get() const { return h_; }
    void setStream(void* hipStream) { check(pslfe_ctx_set_stream(h_, hipStream), "pslfe_ctx_set_stream"); }
    void synchronize() { check(pslfe_ctx_synchronize(h_), "pslfe_ctx_synchronize"); }
private:
    pslfe_ctx* h_ = nullptr;
    int device_ = 0;
};

class ORBextractor {
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(Context& ctx, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int maxBatch = 1)
        : nlevels_(nlevels) {
        check(pslfe_orb_create(ctx.get(), nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, maxBatch, &h_), "pslfe_orb_create");
    }
    ~ORBextractor() { pslfe_orb_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // operator()(image, mask, keypoints, descriptors): mask is ignored, as in the reference;
    // an empty image leaves the outputs untouched (src/ORBextractor.cc:1046).
    void operator()(const uint8_t* image, int cols, int rows, int step, std::vector<PslKeyPoint>& keypoints,
                    std::vector<uint8_t>& descriptors) {
        if (!image || cols <= 0 || rows <= 0) return;
        const int cap = pslfe_orb_max_keypoints(h_, cols, rows);
        if (cap < 0) throw Error(cap, "pslfe_orb_max_keypoints");
        keypoints.resize(cap);
        descriptors.resize((size_t)cap * 32);
        int n = 0;
        check(pslfe_orb_extract(h_, image, cols, rows, step, keypoints.data(), descriptors.data(), cap, &n), "pslfe_orb_extract");
        keypoints.resize(n);
        descriptors.resize((size_t)n * 32);  // n == 0 <=> descriptors.release() (:1064-1065)
    }

    int GetLevels() const { return pslfe_orb_levels(h_); }
    float GetScaleFactor() const { return pslfe_orb_scale_factor(h_); }
    std::vector<float> GetScaleFactors() const { return factors(0); }
    std::vector<float> GetInverseScaleFactors() const { return factors(1); }
    std::vector<float> GetScaleSigmaSquares() const { return factors(2); }
    std::vector<float> GetInverseScaleSigmaSquares() const { return factors(3); }
    pslfe_orb* get() const { return h_; }

private:
    std::vector<float> factors(int which) const {
        std::vector<float> v[4];
        for (auto& x : v) x.resize(nlevels_);
        check(pslfe_orb_scale_factors(h_, v[0].data(), v[1].data(), v[2].data(), v[3].data()), "pslfe_orb_scale_factors");
        return v[which];
    }
    pslfe_orb* h_ = nullptr;
    int nlevels_;
};

// The part of ORB_SLAM2::Frame the matchers read (mvKeysUn, mDescriptors, mvuRight, mGrid).
class FrameGrid {
public:
    FrameGrid(Context& ctx, int maxKeypoints, int maxFrames = 1) {
        check(pslfe_frame_create(ctx.get(), maxKeypoints, maxFrames, &h_), "pslfe_frame_create");
    }
    ~FrameGrid() { pslfe_frame_destroy(h_); }
    FrameGrid(const FrameGrid&) = delete;
    FrameGrid& operator=(const FrameGrid&) = delete;
    void set(int slot, const std::vector<PslKeyPoint>& keysUn, const std::vector<uint8_t>& descriptors, const float* uRight,
             float mnMinX, float mnMinY, float mnMaxX, float mnMaxY) {
        check(pslfe_frame_set(h_, slot, keysUn.data(), descriptors.data(), uRight, (int)keysUn.size(), mnMinX, mnMinY, mnMaxX, mnMaxY),
              "pslfe_frame_set");
    }
    // The RGB-D part of the Frame constructor (src/Frame.cc:105-171): UndistortKeyPoints, ComputeStereoFromRGBD,
    // ComputeImageBounds and AssignFeaturesToGrid from the raw keypoints and the CV_32F depth image.
    void setRGBD(int slot, const std::vector<PslKeyPoint>& keys, const std::vector<uint8_t>& descriptors, const float* depth, int cols,
                 int rows, int strideFloats, const PslCamera& cam) {
        check(pslfe_frame_set_rgbd(h_, slot, keys.data(), descriptors.data(), (int)keys.size(), depth, cols, rows, strideFloats, &cam),
              "pslfe_frame_set_rgbd");
    }
    // The stereo Frame constructor (src/Frame.cc:75-131: ComputeStereoMatches, UndistortKeyPoints, ComputeImageBounds,
    // AssignFeaturesToGrid) for one rectified pair, after left(imLeft, ...) and right(imRight, ...) have run: the last frame of
    // each extractor -> `slot`.  The two extractors are built with the same settings (src/Tracking.cc:128-129).
    void setStereo(int slot, ORBextractor& left, ORBextractor& right, const PslCamera& cam) {
        check(pslfe_frame_set_from_orb_stereo(h_, slot, left.get(), 0, right.get(), 0, 1, &cam), "pslfe_frame_set_from_orb_stereo");
    }
    // The same for nframes pairs of device batches: frame left0+p of `left`'s last batch and frame right0+p of `right`'s -> slot
    // slot0+p (left and right may be one extractor that extracted both images of every pair).  Asynchronous; a device batch's input
    // images must stay unchanged until the work has run (include/pslfe.h).
    void setStereoDevice(int slot0, ORBextractor& left, int left0, ORBextractor& right, int right0, int nframes, const PslCamera& cam) {
        check(pslfe_frame_set_from_orb_stereo(h_, slot0, left.get(), left0, right.get(), right0, nframes, &cam),
              "pslfe_frame_set_from_orb_stereo");
    }
    // The monocular Frame constructor (src/Frame.cc:213-267: UndistortKeyPoints, mvuRight = mvDepth = -1, ComputeImageBounds,
    // AssignFeaturesToGrid) for frames first..first+nframes-1 of `orb`'s last batch -> slots slot0..  Asynchronous.
    void setMono(int slot0, ORBextractor& orb, int first, int nframes, const PslCamera& cam) {
        check(pslfe_frame_set_from_orb_mono(h_, slot0, orb.get(), first, nframes, &cam), "pslfe_frame_set_from_orb_mono");
    }
    // mvKeysUn, mvDepth, mvuRight of a slot
    void fetch(int slot, std::vector<PslKeyPoint>& keysUn, std::vector<float>& depth, std::vector<float>& uRight, int capacity) {
        keysUn.resize(capacity); depth.resize(capacity); uRight.resize(capacity);
        int n = 0;
        check(pslfe_frame_fetch(h_, slot, keysUn.data(), depth.data(), uRight.data(), capacity, &n), "pslfe_frame_fetch");
        keysUn.resize(n); depth.resize(n); uRight.resize(n);
    }
    // mnMinX, mnMinY, mnMaxX, mnMaxY (src/Frame.cc:1135-1168)
    void imageBounds(const PslCamera& cam, int cols, int rows, float bounds[4]) {
        check(pslfe_image_bounds(h_, &cam, cols, rows, bounds), "pslfe_image_bounds");
    }
    // SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1338-1390, up to the window search: slot `slot` is
    // the last frame; points / mpdesc: LastFrame.mvpMapPoints as PslLastPoint[N] / [N][32] (either may be NULL); vo: first the
    // visual-odometry points of Tracking::UpdateLastFrame (src/Tracking.cc:1052-1104).  Fills the queries SearchByProjection takes;
    // owner[q] = last-frame keypoint of query q.
    void ProjectLast(int slot, const PslPose& Tlw, const PslPose& Tcw, const PslLastPoint* points, const uint8_t* mpdesc, const PslCamera& cam,
                     const std::vector<float>& scaleFactors, float th, float thDepth, bool bMono, bool vo, float mnMinX, float mnMinY,
                     float mnMaxX, float mnMaxY, int capacity, std::vector<PslProjQuery>& queries, std::vector<uint8_t>& qdesc,
                     std::vector<int32_t>& owner) {
        queries.resize(capacity); qdesc.resize((size_t)capacity * 32); owner.resize(capacity);
        int n = 0;
        check(pslfe_orb_project_last(h_, slot, &Tlw, &Tcw, points, mpdesc, &cam, scaleFactors.data(), (int)scaleFactors.size(), th, thDepth,
                                     bMono ? 1 : 0, vo ? 1 : 0, mnMinX, mnMinY, mnMaxX, mnMaxY, queries.data(), qdesc.data(), owner.data(),
                                     &n, capacity),
              "pslfe_orb_project_last");
        queries.resize(n); qdesc.resize((size_t)n * 32); owner.resize(n);
    }
    pslfe_frame* get() const { return h_; }
private:
    pslfe_frame* h_ = nullptr;
};

class ORBmatcher {
public:
    static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;  // src/ORBmatcher.cc:37-39
    ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}

    // SearchByProjection(CurrentFrame, LastFrame, th, bMono), src/ORBmatcher.cc:1328: the caller has
    // projected LastFrame's map points (queries / qdesc); returns nmatches.
    int SearchByProjection(FrameGrid& cur, int slot, const std::vector<PslProjQuery>& queries, const std::vector<uint8_t>& qdesc,
                           const uint8_t* taken, std::vector<int32_t>& match, std::vector<int32_t>* assigned = nullptr) {
        match.assign(queries.size(), -1);
        int nm = 0;
        check(pslfe_orb_search_by_projection_last(cur.get(), slot, queries.data(), qdesc.data(), (int)queries.size(), taken,
                                                  mbCheckOrientation ? 1 : 0, match.data(), assigned ? assigned->data() : nullptr, &nm),
              "pslfe_orb_search_by_projection_last");
        return nm;
    }
    // SearchByProjection(F, vpMapPoints, th), src/ORBmatcher.cc:45.
    int SearchByProjectionMap(FrameGrid& cur, int slot, const std::vector<PslProjQuery>& queries, const std::vector<uint8_t>& qdesc,
                              const uint8_t* taken, std::vector<int32_t>& match, std::vector<int32_t>* assigned = nullptr) {
        match.assign(queries.size(), -1);
        int nm = 0;
        check(pslfe_orb_search_by_projection_map(cur.get(), slot, queries.data(), qdesc.data(), (int)queries.size(), taken, mfNNratio,
                                                 match.data(), assigned ? assigned->data() : nullptr, &nm),
              "pslfe_orb_search_by_projection_map");
        return nm;
    }
    // SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist), src/ORBmatcher.cc:1472 (relocalisation): the caller has
    // projected the keyframe's map points; taken[c] != 0 <=> CurrentFrame.mvpMapPoints[c] != NULL.
    int SearchByProjectionKF(FrameGrid& cur, int slot, const std::vector<PslProjQuery>& queries, const std::vector<uint8_t>& qdesc,
                             const uint8_t* taken, int ORBdist, std::vector<int32_t>& match, std::vector<int32_t>* assigned = nullptr) {
        match.assign(queries.size(), -1);
        int nm = 0;
        check(pslfe_orb_search_by_projection_kf(cur.get(), slot, queries.data(), qdesc.data(), (int)queries.size(), taken, ORBdist,
                                                mbCheckOrientation ? 1 : 0, match.data(), assigned ? assigned->data() : nullptr, &nm),
              "pslfe_orb_search_by_projection_kf");
        return nm;
    }
    // SearchByBoW(pKF, F, vpMapPointMatches), src/ORBmatcher.cc:159, on host-side DBoW2 FeatureVectors: fidx = F.mFeatVec flattened
    // in node order; one query (node run of fidx, angle) + descriptor per keyframe feature, in the reference's iteration order.
    int SearchByBoW(FrameGrid& frame, int slot, const std::vector<int32_t>& fidx, const std::vector<PslBowQuery>& queries,
                    const std::vector<uint8_t>& qdesc, std::vector<int32_t>& match, std::vector<int32_t>* assigned = nullptr) {
        match.assign(queries.size(), -1);
        int nm = 0;
        check(pslfe_orb_search_by_bow(frame.get(), slot, fidx.data(), (int)fidx.size(), queries.data(), qdesc.data(), (int)queries.size(),
                                      mfNNratio, mbCheckOrientation ? 1 : 0, match.data(), assigned ? assigned->data() : nullptr, &nm),
              "pslfe_orb_search_by_bow");
        return nm;
    }
    // Frame::isInFrustum(pMP, viewCosLimit) (src/Frame.cc:927-983) for every local map point, and the queries of
    // SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cc:45-70) for those in view, in map-point order; inView / level /
    // viewCos per map point (mbTrackInView, mnTrackScaleLevel, mTrackViewCos).  Returns nToMatch.
    static int ProjectFrustum(Context& ctx, const PslPose& Tcw, const std::vector<PslMapPointGeom>& mps, const std::vector<uint8_t>& mpdesc,
                              const PslCamera& cam, const std::vector<float>& scaleFactors, float mfLogScaleFactor, float viewCosLimit, float th,
                              float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, std::vector<PslProjQuery>& queries,
                              std::vector<uint8_t>& qdesc, std::vector<int32_t>& owner, std::vector<uint8_t>& inView,
                              std::vector<int32_t>& level, std::vector<float>& viewCos) {
        const size_t M = mps.size();
        queries.resize(M); qdesc.resize(M * 32); owner.resize(M); inView.resize(M); level.resize(M); viewCos.resize(M);
        int n = 0;
        check(pslfe_orb_project_frustum(ctx.get(), &Tcw, mps.data(), mpdesc.data(), (int)M, &cam, scaleFactors.data(), (int)scaleFactors.size(),
                                        mfLogScaleFactor, viewCosLimit, th, mnMinX, mnMinY, mnMaxX, mnMaxY, queries.data(), qdesc.data(),
                                        owner.data(), &n, (int)M, inView.data(), level.data(), viewCos.data()),
              "pslfe_orb_project_frustum");
        queries.resize(n); qdesc.resize((size_t)n * 32); owner.resize(n);
        return n;
    }
    // Batched, HBM-resident SearchByProjection(F, vpMapPoints, th) over slots slot0.. of `cur` (pointers are device memory).
    void SearchByProjectionMapDevice(FrameGrid& cur, int slot0, int npairs, const PslProjQuery* d_queries, const uint8_t* d_qdesc,
                                     const int32_t* d_nq, int qstride, const uint8_t* d_taken, int32_t* d_match, int32_t* d_nmatches) {
        check(pslfe_orb_search_by_projection_map_device(cur.get(), slot0, npairs, d_queries, d_qdesc, d_nq, qstride, d_taken, mfNNratio,
                                                        d_match, d_nmatches),
              "pslfe_orb_search_by_projection_map_device");
    }
    // SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize), src/ORBmatcher.cc:405: F1 = slot1 of f1, F2 = slot2
    // of f2; vbPrevMatched as [n1][2] floats (updated in place), n1 = F1's keypoint count.  Returns nmatches.
    int SearchForInitialization(FrameGrid& f1, int slot1, FrameGrid& f2, int slot2, std::vector<float>& vbPrevMatched,
                                std::vector<int32_t>& vnMatches12, int windowSize = 10) {
        vnMatches12.assign(vbPrevMatched.size() / 2, -1);
        int nm = 0;
        check(pslfe_orb_search_for_initialization(f1.get(), slot1, f2.get(), slot2, vbPrevMatched.data(), windowSize, mfNNratio,
                                                  mbCheckOrientation ? 1 : 0, vnMatches12.data(), &nm),
              "pslfe_orb_search_for_initialization");
        return nm;
    }
    // Batched, HBM-resident SearchForInitialization: pair p = (f1 slot slot1[p], f2 slot slot2[p]) with prev rows
    // d_prev + p*prevStride*2, matches d_matches12 + p*prevStride, count d_nmatches[p] (device memory).
    void SearchForInitializationDevice(FrameGrid& f1, const std::vector<int32_t>& slot1, FrameGrid& f2, const std::vector<int32_t>& slot2,
                                       float* d_prev, int prevStride, int windowSize, int32_t* d_matches12, int32_t* d_nmatches) {
        check(slot1.size() == slot2.size() ? PSLFE_OK : PSLFE_E_INVALID, "SearchForInitializationDevice: slot tables differ in length");
        check(pslfe_orb_search_for_initialization_device(f1.get(), slot1.data(), f2.get(), slot2.data(), (int)slot1.size(), d_prev, prevStride,
                                                         windowSize, mfNNratio, mbCheckOrientation ? 1 : 0, d_matches12, d_nmatches),
              "pslfe_orb_search_for_initialization_device");
    }
    // DescriptorDistance, src/ORBmatcher.cc:1647-1663 (host helper, same SWAR popcount)
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
        const uint32_t* pa = reinterpret_cast<const uint32_t*>(a);
        const uint32_t* pb = reinterpret_cast<const uint32_t*>(b);
        int dist = 0;
        for (int i = 0; i < 8; ++i) dist += __builtin_popcount(pa[i] ^ pb[i]);
        return dist;
    }
    float mfNNratio;
    bool mbCheckOrientation;
};

// == ORB_SLAM2::LINEextractor (add_inc/LineExtractor.h:160-255)
class LINEextractor {
public:
    LINEextractor(Context& ctx, int numOctaves, float scale, unsigned int nLSDFeature, double min_line_length, int maxBatch = 1)
        : numOctaves_(numOctaves) {
        check(pslfe_line_create(ctx.get(), numOctaves, scale, (int)nLSDFeature, min_line_length, maxBatch, &h_), "pslfe_line_create");
    }
    ~LINEextractor() { pslfe_line_destroy(h_); }
    LINEextractor(const LINEextractor&) = delete;
    LINEextractor& operator=(const LINEextractor&) = delete;

    // operator()(image, mask, keylines, descriptors, lineVec2d): empty image leaves the outputs untouched
    // (add_src/LineExtractor.cpp:327); lineVec2d holds 3 doubles per line (Eigen::Vector3d layout).
    void operator()(const uint8_t* image, int cols, int rows, int step, std::vector<PslKeyLine>& keylines, std::vector<uint8_t>& descriptors,
                    std::vector<double>& lineVec2d) {
        if (!image || cols <= 0 || rows <= 0) return;
        const int cap = 2048;
        keylines.resize(cap); descriptors.resize((size_t)cap * 32); lineVec2d.resize((size_t)cap * 3);
        int n = 0;
        check(pslfe_line_extract(h_, image, cols, rows, step, keylines.data(), descriptors.data(), lineVec2d.data(), cap, &n), "pslfe_line_extract");
        keylines.resize(n); descriptors.resize((size_t)n * 32); lineVec2d.resize((size_t)n * 3);
    }
    // CPartiallyRecoverConnectivity(mLines, radius, fans, img, fanThr): mLines n x 4 floats, fans k x 4
    void PartiallyRecoverConnectivity(const std::vector<float>& mLines, float radius, std::vector<float>& fans, int imgCols, int imgRows, float fanThr) {
        const int n = (int)mLines.size() / 4, cap = 4096;
        fans.resize((size_t)cap * 4);
        int k = 0;
        check(pslfe_lil_pair(h_, mLines.data(), n, radius, fanThr, imgCols, imgRows, fans.data(), cap, &k), "pslfe_lil_pair");
        fans.resize((size_t)k * 4);
    }
    // PSLFE_LSD_REFINE_ADV (default, what the stock contrib LSDDetector constructs) or PSLFE_LSD_REFINE_STD
    void SetRefine(int mode) { check(pslfe_line_set_refine(h_, mode), "pslfe_line_set_refine"); }
    int GetLevels() const { return pslfe_line_levels(h_); }
    float GetScaleFactor() const { return pslfe_line_scale_factor(h_); }
    std::vector<float> GetScaleFactors() const { return factors(0); }
    std::vector<float> GetInverseScaleFactors() const { return factors(1); }
    std::vector<float> GetScaleSigmaSquares() const { return factors(2); }
    std::vector<float> GetInverseScaleSigmaSquares() const { return factors(3); }
    pslfe_line* get() const { return h_; }

private:
    std::vector<float> factors(int which) const {
        std::vector<float> v[4];
        for (auto& x : v) x.resize(numOctaves_);
        check(pslfe_line_scale_factors(h_, v[0].data(), v[1].data(), v[2].data(), v[3].data()), "pslfe_line_scale_factors");
        return v[which];
    }
    pslfe_line* h_ = nullptr;
    int numOctaves_;
};

class LSDmatcher {
public:
    static const int TH_HIGH = 80, TH_LOW = 50;  // add_src/LSDmatcher.cpp:12-14
    LSDmatcher(Context& ctx, float nnratio = 0.95f, bool checkOri = true) : ctx_(ctx), mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    // matchNNR(desc1, desc2, nnr, matches_12), add_src/LSDmatcher.cpp:354-376
    int matchNNR(const std::vector<uint8_t>& desc1, const std::vector<uint8_t>& desc2, float nnr, std::vector<int>& matches_12) {
        const int n1 = (int)desc1.size() / 32, n2 = (int)desc2.size() / 32;
        matches_12.assign(n1, -1);
        int nm = 0;
        check(pslfe_line_match_nnr(ctx_.get(), desc1.data(), n1, desc2.data(), n2, nnr, matches_12.data(), &nm), "pslfe_line_match_nnr");
        return nm;
    }
    int match(const std::vector<uint8_t>& d1, const std::vector<uint8_t>& d2, float nnr, std::vector<int>& m12) { return matchNNR(d1, d2, nnr, m12); }
    // SearchByGeomNApearance(CurrentFrame, LastFrame, desc_th), add_src/LSDmatcher.cpp:36-110: assigned[i2] = last-frame line
    // whose map line CurrentFrame.mvpMapLines[i2] receives
    int SearchByGeomNApearance(const std::vector<PslKeyLine>& klLast, const std::vector<uint8_t>& descLast, const std::vector<PslKeyLine>& klCur,
                               const std::vector<uint8_t>& descCur, const std::vector<uint8_t>& lastHasMapLine, float desc_th, float mnMinX,
                               float mnMaxX, float mnMinY, float mnMaxY, std::vector<int32_t>& matches_12, std::vector<int32_t>& assigned) {
        matches_12.assign(klLast.size(), -1);
        assigned.assign(klCur.size(), -1);
        int n = 0;
        check(pslfe_line_search_by_geom_appearance(ctx_.get(), klLast.data(), descLast.data(), (int)klLast.size(), klCur.data(), descCur.data(),
                                                   (int)klCur.size(), lastHasMapLine.data(), desc_th, mnMinX, mnMaxX, mnMinY, mnMaxY,
                                                   matches_12.data(), assigned.data(), &n), "pslfe_line_search_by_geom_appearance");
        return n;
    }
    // FrameBFMatch(ldesc1, ldesc2, LineMatches, TH), add_src/LSDmatcher.cpp:492-516
    void FrameBFMatch(const std::vector<uint8_t>& ldesc1, const std::vector<uint8_t>& ldesc2, std::vector<int>& LineMatches, float TH) {
        LineMatches.assign(ldesc1.size() / 32, -1);
        check(pslfe_line_frame_bf_match(ctx_.get(), ldesc1.data(), (int)ldesc1.size() / 32, ldesc2.data(), (int)ldesc2.size() / 32, mfNNratio, TH,
                                        LineMatches.data()), "pslfe_line_frame_bf_match");
    }
    // SearchByProjection(CurrentFrame, LastFrame, th) :112-215 (mode 0) / SearchByProjection(F, vpMapLines, eval_orient, th) :260-352 (mode 1)
    int SearchByProjection(const std::vector<PslKeyLine>& kls, const std::vector<uint8_t>& ldesc, const std::vector<double>& keyLineFunctions,
                           const double* lines3dDir, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY, const std::vector<PslLineQuery>& queries,
                           const std::vector<uint8_t>& qdesc, const uint8_t* taken, int mode, std::vector<int32_t>& match,
                           std::vector<int32_t>* assigned = nullptr) {
        match.assign(queries.size(), -1);
        if (assigned) assigned->assign(kls.size(), -1);
        int n = 0;
        check(pslfe_line_search_by_projection(ctx_.get(), kls.data(), ldesc.data(), keyLineFunctions.data(), lines3dDir, (int)kls.size(), mnMinX,
                                              mnMinY, mnMaxX, mnMaxY, queries.data(), qdesc.data(), (int)queries.size(), taken, mode, mfNNratio,
                                              match.data(), assigned ? assigned->data() : nullptr, &n, nullptr, nullptr, 0, nullptr),
              "pslfe_line_search_by_projection");
        return n;
    }
    // Batched, HBM-resident SearchByProjection (mode 0 / 1) over npairs pairs of device-resident frames (pointers are device memory;
    // layout in include/pslfe.h).  Asynchronous on the context's stream.
    void SearchByProjectionDevice(int npairs, const PslKeyLine* d_kls, const uint8_t* d_ldesc, const double* d_lineEq, const int32_t* d_nkl,
                                  int klStride, const double* d_lines3d, int lines3dStride, float mnMinX, float mnMinY, float mnMaxX,
                                  float mnMaxY, const PslLineQuery* d_queries, const uint8_t* d_qdesc, const int32_t* d_nq, int qstride,
                                  const uint8_t* d_taken, int mode, int32_t* d_match, int32_t* d_assigned, int32_t* d_nmatches,
                                  int32_t* d_nfallback = nullptr) {
        check(pslfe_line_search_by_projection_device(ctx_.get(), npairs, d_kls, d_ldesc, d_lineEq, d_nkl, klStride, d_lines3d, lines3dStride,
                                                     mnMinX, mnMinY, mnMaxX, mnMaxY, d_queries, d_qdesc, d_nq, qstride, d_taken, mode,
                                                     mfNNratio, d_match, d_assigned, d_nmatches, d_nfallback),
              "pslfe_line_search_by_projection_device");
    }
    // Frame::isInFrustum(MapLine*, viewCosLimit) src/Frame.cc:828-904 for every map line and the query rows of
    // SearchByProjection(F, vpMapLines, eval_orient, th) :260-289 for those in view, in map-line order; inView / level / viewCos per line.
    void ProjectMapLines(const PslPose& Tcw, const std::vector<PslMapLineGeom>& mls, const std::vector<uint8_t>& mldesc, const PslCamera& cam,
                         float logScaleFactor, float viewCosLimit, float th, float mnMinX, float mnMinY, float mnMaxX, float mnMaxY,
                         std::vector<PslLineQuery>& queries, std::vector<uint8_t>& qdesc, std::vector<int32_t>& owner,
                         std::vector<uint8_t>* inView = nullptr, std::vector<int32_t>* level = nullptr, std::vector<float>* viewCos = nullptr) {
        const size_t M = mls.size();
        queries.resize(M); qdesc.resize(M * 32); owner.resize(M);
        if (inView) inView->resize(M);
        if (level) level->resize(M);
        if (viewCos) viewCos->resize(M);
        int nq = 0;
        check(pslfe_line_project_frustum(ctx_.get(), &Tcw, mls.data(), mldesc.data(), (int)M, &cam, logScaleFactor, viewCosLimit, th, mnMinX,
                                         mnMinY, mnMaxX, mnMaxY, queries.data(), qdesc.data(), owner.data(), &nq, (int)M,
                                         inView ? inView->data() : nullptr, level ? level->data() : nullptr, viewCos ? viewCos->data() : nullptr),
              "pslfe_line_project_frustum");
        queries.resize(nq); qdesc.resize((size_t)nq * 32); owner.resize(nq);
    }
    // SearchByProjection(CurrentFrame, LastFrame, th) :112-155 up to the window search: the last frame's keylines / LBD rows and
    // mvpMapLines as PslLastLine records (mldesc: the map lines' descriptors, or empty for the last frame's own rows).
    void ProjectLastFrameLines(const std::vector<PslKeyLine>& klsLast, const std::vector<uint8_t>& ldescLast, const std::vector<PslLastLine>& lines,
                               const std::vector<uint8_t>& mldesc, const PslPose& Tcw, const PslCamera& cam, float th, float mnMinX,
                               float mnMinY, float mnMaxX, float mnMaxY, std::vector<PslLineQuery>& queries, std::vector<uint8_t>& qdesc,
                               std::vector<int32_t>& owner) {
        const size_t n = klsLast.size();
        queries.resize(n); qdesc.resize(n * 32); owner.resize(n);
        int nq = 0;
        check(pslfe_line_project_last(ctx_.get(), klsLast.data(), ldescLast.data(), (int)n, lines.data(), mldesc.empty() ? nullptr : mldesc.data(),
                                      &Tcw, &cam, th, mnMinX, mnMinY, mnMaxX, mnMaxY, queries.data(), qdesc.data(), owner.data(), &nq, (int)n),
              "pslfe_line_project_last");
        queries.resize(nq); qdesc.resize((size_t)nq * 32); owner.resize(nq);
    }
private:
    Context& ctx_;
public:
    float mfNNratio;
    bool mbCheckOrientation;
};

// The part of Frame::ExtractLSD after the extractor (src/Frame.cc:490-660): isLineGood, convertFansToKeyLines, planes.
class FrameGlue {
public:
    struct Result {
        std::vector<double> lines3d;   // mvLines3D, n x 6
        std::vector<float> lineEq;     // mvLineEq, n x 3
        std::vector<int32_t> pair;     // intersection_lines_plane: line indices, k x 2
        std::vector<float> xy;         // ... 2-D crossing, k x 2
        std::vector<double> cross;     // ... 3-D crossing, k x 3
        std::vector<double> le_l;      // mvle_l, k x 6
        std::vector<float> planes;     // mvPlanes, p x 4
        std::vector<double> normals;   // mvPlaneNormal, p x 3
        std::vector<int32_t> lineNo;   // mvPlaneLineNo, p x 2
        std::vector<double> cross3d;   // CrossPoint_3D, p x 3
        std::vector<double> cross2d;   // CrossPoint_2D, p x 2
    };
    FrameGlue(Context& ctx, int maxLines = 1024, int maxFans = 4096, int maxBatch = 1) : maxFans_(maxFans) {
        check(pslfe_glue_create(ctx.get(), maxLines, maxFans, maxBatch, &h_), "pslfe_glue_create");
    }
    ~FrameGlue() { pslfe_glue_destroy(h_); }
    FrameGlue(const FrameGlue&) = delete;
    FrameGlue& operator=(const FrameGlue&) = delete;
    // fans: the n x 4 matrix of CPartiallyRecoverConnectivity; seed: srand(seed) of the frame (convention H7)
    Result run(const std::vector<PslKeyLine>& keylines, const std::vector<float>& fans, const float* depth, int cols, int rows, int strideFloats,
               const PslCamera& cam, uint32_t seed) {
        const int n = (int)keylines.size(), nf = (int)fans.size() / 4;
        check(pslfe_glue_run(h_, keylines.data(), n, fans.data(), nf, depth, cols, rows, strideFloats, &cam, seed), "pslfe_glue_run");
        return fetch(0, n);
    }
    // results of frame `frame` of the last run / pslfe_glue_run_batch_device; n = that frame's keyline count
    Result fetch(int frame, int n) {
        const int cap = maxFans_;
        Result r;
        r.lines3d.resize((size_t)n * 6); r.lineEq.resize((size_t)n * 3);
        r.pair.resize((size_t)cap * 2); r.xy.resize((size_t)cap * 2); r.cross.resize((size_t)cap * 3); r.le_l.resize((size_t)cap * 6);
        r.planes.resize((size_t)cap * 4); r.normals.resize((size_t)cap * 3); r.lineNo.resize((size_t)cap * 2);
        r.cross3d.resize((size_t)cap * 3); r.cross2d.resize((size_t)cap * 2);
        int k = 0, p = 0;
        check(pslfe_glue_fetch(h_, frame, n, r.lines3d.data(), r.lineEq.data(), r.pair.data(), r.xy.data(), r.cross.data(), r.le_l.data(), cap, &k,
                               r.planes.data(), r.normals.data(), r.lineNo.data(), r.cross3d.data(), r.cross2d.data(), cap, &p),
              "pslfe_glue_fetch");
        r.pair.resize((size_t)k * 2); r.xy.resize((size_t)k * 2); r.cross.resize((size_t)k * 3); r.le_l.resize((size_t)k * 6);
        r.planes.resize((size_t)p * 4); r.normals.resize((size_t)p * 3); r.lineNo.resize((size_t)p * 2);
        r.cross3d.resize((size_t)p * 3); r.cross2d.resize((size_t)p * 2);
        return r;
    }
    pslfe_glue* get() const { return h_; }
    // device view of the last batch's mvLines3D: [maxBatch][stride][6] doubles, stride = maxLines
    const double* lines3dDevice(int* stride) const {
        const double* d = nullptr;
        check(pslfe_glue_lines3d_device(h_, &d, stride), "pslfe_glue_lines3d_device");
        return d;
    }
    // device view of the last batch's mvle_l ([maxBatch][leStride][6]) and CrossPoint_2D ([maxBatch][planeStride][2]) with their counts
    struct LilObs {
        const double* d_leL = nullptr;
        const double* d_cross2d = nullptr;
        const int32_t* d_ncross = nullptr;
        const int32_t* d_nplanes = nullptr;
        int leStride = 0, planeStride = 0;
    };
    LilObs lilObsDevice() const {
        LilObs o;
        check(pslfe_glue_lil_obs_device(h_, &o.d_leL, &o.leStride, &o.d_ncross, &o.d_cross2d, &o.planeStride, &o.d_nplanes),
              "pslfe_glue_lil_obs_device");
        return o;
    }
private:
    pslfe_glue* h_ = nullptr;
    int maxFans_;
};

// == Look-ahead extraction for the Tracking loop.  The reference's caller is a sequential loop over the frames of a recording
//    (Examples/RGB-D/rgbd_tum.cc:88-130) that constructs one Frame per image (src/Tracking.cc:240 -> src/Frame.cc:133-208); nothing the
//    Frame constructor computes depends on the pose of an earlier frame, so the extraction of frames t+1 .. t+K can run in ONE batched
//    launch while frame t is being tracked.  push() stages a frame (gray + CV_32F depth, copied to HBM); a full batch of `lookahead`
//    frames is launched at once -
//        pslfe_orb_extract_batch_device, pslfe_line_extract_batch_device, pslfe_line_pair_batch_device,
//        pslfe_glue_run_batch_device, pslfe_frame_set_from_orb_rgbd, pslfe_record_pack_device
//    - asynchronously, on one of TWO lanes (each with its own context / stream, extractor objects and frame grid): while the tracker
//    works through the frames of one lane, the next batch is extracted on the other.  pop() hands out the oldest frame's Frame
//    members (the packed per-frame records come back in one copy per batch).  A frame's grid slot - grid() after its pop(), or
//    frame.grid / frame.slot - stays valid until `lookahead` further frames have been popped: call the matchers for a frame before
//    popping the next one (as a Tracking thread does).  isLineGood's rand() stream is seeded with 1 + the frame's running index
//    (convention H7), so the results are those of the one-frame-at-a-time path, bit for bit, whatever the look-ahead.
//    A live camera pays up to 2 K - 1 frames of latency for this; a recording pays nothing.
class FramePrefetcher {
public:
    struct Frame {   // the members of ORB_SLAM2::Frame this path fills
        uint64_t index = 0;          // running index of the frame (push order)
        int slot = 0;                // its slot in *grid: SearchByProjection(*frame.grid, frame.slot, ...)
        FrameGrid* grid = nullptr;
        std::vector<PslKeyPoint> mvKeys, mvKeysUn;
        std::vector<uint8_t> mDescriptors;
        std::vector<float> mvDepth, mvuRight;
        std::vector<PslKeyLine> mvKeylinesUn;
        std::vector<uint8_t> mLdesc;
        std::vector<double> mvKeyLineFunctions;
        std::vector<float> fans;
        FrameGlue::Result glue;
    };

    FramePrefetcher(Context& ctx, int cols, int rows, int lookahead, int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                    int nLSDFeature, const PslCamera& cam, float pairRadius = 20.0f, float fanThr = 0.78539816339744830962f)
        : w_(cols), h_(rows), K_(lookahead < 1 ? 1 : lookahead), cam_(cam), radius_(pairRadius), fanThr_(fanThr) {
        for (int l = 0; l < 2; ++l) {
            Lane& L = lane_[l];
            L.ctx = std::make_unique<Context>(ctx.device());   // a context (= a stream) of its own per lane: the caller's context stays free for
                                                             // the per-frame calls of the tracker (LSDmatcher, plane association ...) while a lane extracts
            L.orb = std::make_unique<ORBextractor>(*L.ctx, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, K_);
            L.lsd = std::make_unique<LINEextractor>(*L.ctx, 1, 1.2f, (unsigned)nLSDFeature, 0.0, K_);
            kpCap_ = pslfe_orb_max_keypoints(L.orb->get(), cols, rows);
            if (kpCap_ < 0) throw Error(kpCap_, "pslfe_orb_max_keypoints");
            L.grid = std::make_unique<FrameGrid>(*L.ctx, kpCap_ > 0 ? kpCap_ : 1, K_);
            L.d_gray = DeviceBuffer(*L.ctx, (size_t)K_ * w_ * h_);
            L.d_depth = DeviceBuffer(*L.ctx, (size_t)K_ * w_ * h_ * sizeof(float));
            caps_.kp_cap = kpCap_; caps_.kl_cap = nLSDFeature; caps_.fan_cap = PSLFE_FAN_CAP; caps_.plane_cap = 0;
            check(pslfe_record_layout(&caps_, &lay_), "pslfe_record_layout");
            L.d_rec = DeviceBuffer(*L.ctx, (size_t)K_ * lay_.bytes);
            L.rec.resize((size_t)K_ * lay_.bytes);
        }
    }
    FramePrefetcher(const FramePrefetcher&) = delete;
    FramePrefetcher& operator=(const FramePrefetcher&) = delete;

    int lookahead() const { return K_; }
    // frames pushed and not yet popped / of those, the ones whose extraction has been launched or collected
    size_t staged() const { return (size_t)(lane_[0].staged + lane_[1].staged - lane_[0].next - lane_[1].next); }
    size_t ready() const { return (size_t)((lane_[0].collected ? lane_[0].staged - lane_[0].next : 0) + (lane_[1].collected ? lane_[1].staged - lane_[1].next : 0)); }
    FrameGrid& grid() { return *lane_[last_].grid; }   // of the frame popped last
    ORBextractor& orbExtractor() { return *lane_[0].orb; }
    LINEextractor& lineExtractor() { return *lane_[0].lsd; }

    // true when push() would accept a frame now (a lane is free or being filled)
    bool canPush() const {
        const Lane& L = lane_[stage_];
        return !L.launched || (L.collected && L.next == L.staged);
    }

    // Stages one frame: gray 8UC1 (`grayStep` bytes per row), depth CV_32F in metres (`depthStep` floats per row); the batch is launched
    // when `lookahead` frames are staged.  Returns false (and stages nothing) while both lanes hold frames that have not been popped.
    bool push(const uint8_t* gray, int grayStep, const float* depth, int depthStep) {
        if (!gray || !depth) return false;
        Lane& L = lane_[stage_];
        if (L.launched) {
            if (!(L.collected && L.next == L.staged)) return false;   // still being popped (or not popped at all)
            L.launched = L.collected = false; L.staged = L.next = 0;   // every frame of this lane has been handed out: it takes the next batch
        }
        uint8_t* dg = static_cast<uint8_t*>(L.d_gray.get()) + (size_t)L.staged * w_ * h_;
        float* dd = static_cast<float*>(L.d_depth.get()) + (size_t)L.staged * w_ * h_;
        if (grayStep != w_) {   // rows with padding: packed on the host first, one copy either way
            tmp8_.resize((size_t)w_ * h_);
            for (int y = 0; y < h_; ++y) memcpy(tmp8_.data() + (size_t)y * w_, gray + (size_t)y * grayStep, (size_t)w_);
            gray = tmp8_.data();
        }
        if (depthStep != w_) {
            tmp32_.resize((size_t)w_ * h_);
            for (int y = 0; y < h_; ++y) memcpy(tmp32_.data() + (size_t)y * w_, depth + (size_t)y * depthStep, (size_t)w_ * sizeof(float));
            depth = tmp32_.data();
        }
        check(pslfe_device_upload(L.ctx->get(), dg, gray, (size_t)w_ * h_), "pslfe_device_upload");
        check(pslfe_device_upload(L.ctx->get(), dd, depth, (size_t)w_ * h_ * sizeof(float)), "pslfe_device_upload");
        if (++L.staged == K_) { launch(stage_); stage_ ^= 1; }
        return true;
    }

    // Launches the extraction of a partly filled batch now (pop() does it when it runs out of launched frames).
    void flush() {
        Lane& L = lane_[stage_];
        if (!L.launched && L.staged > 0) { launch(stage_); stage_ ^= 1; }
    }

    // The oldest frame not handed out yet; false when nothing is staged.  Lanes are filled and emptied alternately, so the oldest frame is
    // always in lane cur_.
    bool pop(Frame& out) {
        Lane& L = lane_[cur_];
        if (L.launched && L.collected && L.next == L.staged) return false;   // used up, and nothing has been pushed since
        if (!L.launched) {                                                   // a partly filled batch: extract it now
            if (L.staged == 0) return false;
            launch(cur_);
            if (stage_ == cur_) stage_ ^= 1;
        }
        if (!L.collected) {   // the batch's packed records, one copy (waits for the lane's stream)
            check(pslfe_device_download(L.ctx->get(), L.rec.data(), L.d_rec.get(), (size_t)L.staged * lay_.bytes), "pslfe_device_download");
            L.collected = true;
        }
        const int k = L.next;
        const uint8_t* r = L.rec.data() + (size_t)k * lay_.bytes;
        int32_t hd[8];
        memcpy(hd, r, sizeof(hd));
        const int nkp = hd[0], nkl = hd[2], nfan = hd[4];
        if ((hd[6] & 7) != 0) throw Error(PSLFE_E_CAPACITY, "FramePrefetcher: a frame's results exceed the record capacities");
        ++L.next;   // only once the record is known to be whole: after a throw above, a retry sees the same frame
        out.index = L.index0 + (uint64_t)k; out.slot = k; out.grid = L.grid.get();
        out.mvKeys.resize(nkp); out.mDescriptors.resize((size_t)nkp * 32);
        out.mvKeylinesUn.resize(nkl); out.mLdesc.resize((size_t)nkl * 32); out.mvKeyLineFunctions.resize((size_t)nkl * 3);
        out.fans.resize((size_t)nfan * 4);
        if (nkp) { memcpy(out.mvKeys.data(), r + lay_.off_kps, (size_t)nkp * sizeof(PslKeyPoint)); memcpy(out.mDescriptors.data(), r + lay_.off_desc, (size_t)nkp * 32); }
        if (nkl) {
            memcpy(out.mvKeylinesUn.data(), r + lay_.off_kls, (size_t)nkl * sizeof(PslKeyLine));
            memcpy(out.mLdesc.data(), r + lay_.off_ldesc, (size_t)nkl * 32);
            memcpy(out.mvKeyLineFunctions.data(), r + lay_.off_lineEq, (size_t)nkl * 3 * sizeof(double));
        }
        if (nfan) memcpy(out.fans.data(), r + lay_.off_fans, (size_t)nfan * 4 * sizeof(float));
        out.glue = L.glue->fetch(k, nkl);                                            // mvLines3D, crossings, mvPlanes ...
        if (nkp) L.grid->fetch(k, out.mvKeysUn, out.mvDepth, out.mvuRight, kpCap_);   // mvKeysUn, mvDepth, mvuRight
        else { out.mvKeysUn.clear(); out.mvDepth.clear(); out.mvuRight.clear(); }
        last_ = cur_;
        if (L.next == L.staged) cur_ ^= 1;   // this lane is used up: the next frame is the other lane's first
        return true;
    }

private:
    // One pslfe_device_alloc block of a lane, freed once the lane's context has finished with it.
    class DeviceBuffer {
    public:
        DeviceBuffer() = default;
        DeviceBuffer(Context& ctx, size_t bytes) : ctx_(&ctx) { check(pslfe_device_alloc(ctx.get(), bytes, &p_), "pslfe_device_alloc"); }
        DeviceBuffer(DeviceBuffer&& o) noexcept : ctx_(o.ctx_), p_(o.p_) { o.p_ = nullptr; }
        DeviceBuffer& operator=(DeviceBuffer&& o) noexcept { std::swap(ctx_, o.ctx_); std::swap(p_, o.p_); return *this; }
        ~DeviceBuffer() {
            if (!p_) return;
            pslfe_ctx_synchronize(ctx_->get());
            pslfe_device_free(ctx_->get(), p_);
        }
        void* get() const { return p_; }
    private:
        Context* ctx_ = nullptr;
        void* p_ = nullptr;
    };
    // members are destroyed in reverse order: the buffers and extractors before the lane's context
    struct Lane {
        std::unique_ptr<Context> ctx;
        std::unique_ptr<ORBextractor> orb;
        std::unique_ptr<LINEextractor> lsd;
        std::unique_ptr<FrameGrid> grid;
        std::unique_ptr<FrameGlue> glue;   // created after the first batch: its row stride is the line extractor's (pslfe_line_results_device)
        DeviceBuffer d_gray, d_depth, d_rec;
        std::vector<uint8_t> rec;
        int staged = 0, next = 0;            // frames staged in this lane / handed out
        bool launched = false, collected = false;
        uint64_t index0 = 0;
    };

    // every staged frame of the lane through the extractors, asynchronously on the lane's stream
    void launch(int l) {
        Lane& L = lane_[l];
        const int F = L.staged;
        const uint8_t* dg = static_cast<const uint8_t*>(L.d_gray.get());
        const float* dd = static_cast<const float*>(L.d_depth.get());
        check(pslfe_orb_extract_batch_device(L.orb->get(), dg, F, w_, h_, w_, (size_t)w_ * h_), "pslfe_orb_extract_batch_device");       // ExtractORB
        check(pslfe_line_extract_batch_device(L.lsd->get(), dg, F, w_, h_, w_, (size_t)w_ * h_), "pslfe_line_extract_batch_device");   // ExtractLSD: extractor
        check(pslfe_line_pair_batch_device(L.lsd->get(), radius_, fanThr_), "pslfe_line_pair_batch_device");                              // src/Frame.cc:505
        PslRecordSources S;
        memset(&S, 0, sizeof(S));
        check(pslfe_orb_results_device(L.orb->get(), &S.d_kps, &S.d_desc, &S.d_kp_counts, &S.kp_stride), "pslfe_orb_results_device");
        check(pslfe_line_results_device(L.lsd->get(), &S.d_kls, &S.d_ldesc, &S.d_lineEq, &S.d_kl_counts, &S.kl_stride), "pslfe_line_results_device");
        check(pslfe_line_fans_device(L.lsd->get(), &S.d_fans, &S.d_fan_counts, &S.fan_stride), "pslfe_line_fans_device");
        if (!L.glue) L.glue = std::make_unique<FrameGlue>(*L.ctx, S.kl_stride, S.fan_stride, K_);
        check(pslfe_glue_run_batch_device(L.glue->get(), F, S.d_kls, S.kl_stride, S.d_kl_counts, S.d_fans, S.fan_stride, S.d_fan_counts, dd, w_, h_, &cam_,
                                          (uint32_t)(1u + next_index_)), "pslfe_glue_run_batch_device");                               // isLineGood, fans, planes
        check(pslfe_frame_set_from_orb_rgbd(L.grid->get(), L.orb->get(), dd, w_, h_, &cam_), "pslfe_frame_set_from_orb_rgbd");          // Undistort .. AssignFeaturesToGrid
        check(pslfe_record_pack_device(L.ctx->get(), &caps_, &S, F, L.d_rec.get()), "pslfe_record_pack_device");
        L.index0 = next_index_;
        next_index_ += (uint64_t)F;
        L.launched = true; L.collected = false; L.next = 0;
    }

    int w_, h_, K_;
    PslCamera cam_;
    float radius_, fanThr_;
    int kpCap_ = 0;
    Lane lane_[2];
    PslRecordCaps caps_;
    PslRecordLayout lay_;
    std::vector<uint8_t> tmp8_;
    std::vector<float> tmp32_;
    int stage_ = 0, cur_ = 0, last_ = 0;   // the lane being filled / popped from next / of the frame popped last
    uint64_t next_index_ = 0;
};

// DBoW2 ORBVocabulary as far as Frame::ComputeBoW needs it (src/Frame.cc:1053-1060): the tree as flat arrays, transform on the device.
class ORBVocabulary {
public:
    struct Result {
        std::vector<int32_t> word, nid;        // per feature
        std::vector<double> weight;
        std::vector<int32_t> bowId;            // mBowVec, ascending
        std::vector<double> bowVal;
        std::vector<int32_t> fvNode, fvStart, fvIdx;  // mFeatVec: node g owns fvIdx[fvStart[g] .. fvStart[g+1])
    };
    // node i: children childIds[childBegin[i] .. + childCount[i]) in Node::children order; node 0 = root; L = m_L
    ORBVocabulary(Context& ctx, const std::vector<int32_t>& childBegin, const std::vector<int32_t>& childCount, const std::vector<int32_t>& childIds,
                  const std::vector<uint8_t>& nodeDesc, const std::vector<double>& nodeWeight, const std::vector<int32_t>& nodeWord, int L) {
        check(pslfe_vocab_create(ctx.get(), (int)childBegin.size(), childBegin.data(), childCount.data(), childIds.data(), (int)childIds.size(),
                                 nodeDesc.data(), nodeWeight.data(), nodeWord.data(), L, &h_), "pslfe_vocab_create");
    }
    ~ORBVocabulary() { pslfe_vocab_destroy(h_); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;
    Result transform(const std::vector<uint8_t>& descriptors, int levelsup = 4) {
        const int n = (int)descriptors.size() / 32;
        Result r;
        r.word.resize(n); r.nid.resize(n); r.weight.resize(n); r.bowId.resize(n); r.bowVal.resize(n);
        r.fvNode.resize(n); r.fvStart.resize(n + 1); r.fvIdx.resize(n);
        int nb = 0, nf = 0;
        check(pslfe_compute_bow(h_, descriptors.data(), n, levelsup, r.word.data(), r.weight.data(), r.nid.data(), r.bowId.data(), r.bowVal.data(),
                                &nb, r.fvNode.data(), r.fvStart.data(), r.fvIdx.data(), &nf), "pslfe_compute_bow");
        r.bowId.resize(nb); r.bowVal.resize(nb); r.fvNode.resize(nf); r.fvStart.resize(nf + 1);
        r.fvIdx.resize(nf ? r.fvStart[nf] : 0);
        return r;
    }
private:
    pslfe_vocab* h_ = nullptr;
};

// == KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) on resident BowVectors (pslfe_kfdb).  A keyframe is a
//    slot 0 .. maxKeyFrames-1; a BowVector is ascending word ids with their values (ORBVocabulary::Result::bowId / bowVal).  The
//    device gives the common words, the first common word and the L1 score of every slot; the covisibility tails run here as the
//    reference writes them, on the caller's graph: connected = pKF->GetConnectedKeyFrames(), neighbours[slot] = that keyframe's
//    GetBestCovisibilityKeyFrames(10), both as slots (neighbours may be shorter than the database: a missing entry is empty).
//    mLoopScore / mRelocScore live per slot between queries and are written only when the slot is scored; add sets them to 0.0f
//    (the reference leaves them uninitialised, src/KeyFrame.cc:35).
class KeyFrameDatabase {
public:
    KeyFrameDatabase(Context& ctx, int maxKeyFrames, int maxWords = 4096)
        : K_(maxKeyFrames > 0 ? maxKeyFrames : 0), mLoopScore_(K_, 0.0f), mRelocScore_(K_, 0.0f) {
        check(pslfe_kfdb_create(ctx.get(), maxKeyFrames, maxWords, &h_), "pslfe_kfdb_create");
    }
    ~KeyFrameDatabase() { pslfe_kfdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;
    pslfe_kfdb* get() const { return h_; }

    void add(int slot, const std::vector<int32_t>& bowId, const std::vector<double>& bowVal) {
        sameLength(bowId, bowVal, "KeyFrameDatabase::add");
        check(pslfe_kfdb_add(h_, slot, bowId.data(), bowVal.data(), (int)bowId.size()), "pslfe_kfdb_add");
        mLoopScore_[slot] = mRelocScore_[slot] = 0.0f;
    }
    // the BowVectors of a pslfe_compute_bow_device result -> slots slot0 .. slot0 + nframes - 1
    void addDevice(int slot0, const int32_t* d_bowId, const double* d_bowVal, const int32_t* d_nbow, int nframes, int stride) {
        check(pslfe_kfdb_add_device(h_, slot0, d_bowId, d_bowVal, d_nbow, nframes, stride), "pslfe_kfdb_add_device");
        std::fill(mLoopScore_.begin() + slot0, mLoopScore_.begin() + slot0 + nframes, 0.0f);
        std::fill(mRelocScore_.begin() + slot0, mRelocScore_.begin() + slot0 + nframes, 0.0f);
    }
    void erase(int slot) { check(pslfe_kfdb_erase(h_, slot), "pslfe_kfdb_erase"); }
    void clear() { check(pslfe_kfdb_clear(h_), "pslfe_kfdb_clear"); }

    // mpORBVocabulary->score(bow, mBowVec of each slot), the minScore loop of LoopClosing::DetectLoop (src/LoopClosing.cc:124-138)
    std::vector<double> Score(const std::vector<int32_t>& bowId, const std::vector<double>& bowVal, const std::vector<int32_t>& slots) {
        sameLength(bowId, bowVal, "KeyFrameDatabase::Score");
        std::vector<double> s(slots.size(), 0.0);
        check(pslfe_kfdb_score(h_, bowId.data(), bowVal.data(), (int)bowId.size(), slots.data(), (int)slots.size(), s.data()), "pslfe_kfdb_score");
        return s;
    }
    // == DetectLoopCandidates(pKF, minScore) src/KeyFrameDatabase.cc:76-197: the candidate slots in the reference's order
    std::vector<int32_t> DetectLoopCandidates(const std::vector<int32_t>& bowId, const std::vector<double>& bowVal, const std::vector<int32_t>& connected,
                                              float minScore, const std::vector<std::vector<int32_t>>& neighbours) {
        std::vector<uint8_t> exclude(K_, 0);
        for (int32_t s : connected) {
            if (s < 0 || (size_t)s >= K_) throw Error(PSLFE_E_INVALID, "KeyFrameDatabase::DetectLoopCandidates: connected slot out of range");
            exclude[s] = 1;
        }
        const int minCommonWords = sharing(bowId, bowVal, exclude.data(), "KeyFrameDatabase::DetectLoopCandidates");
        std::vector<std::pair<float, int32_t>> lScoreAndMatch, lAccScoreAndMatch;
        for (int32_t s : sharing_) {
            if (words_[s] > minCommonWords) {
                const float si = (float)score_[s];
                mLoopScore_[s] = si;
                if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, s));
            }
        }
        if (lScoreAndMatch.empty()) return std::vector<int32_t>();
        float bestAccScore = minScore;
        for (const auto& it : lScoreAndMatch) {
            float bestScore = it.first, accScore = it.first;
            int32_t best = it.second;
            for (int32_t s2 : neigh(neighbours, it.second)) {
                if (words_[s2] > 0 && words_[s2] > minCommonWords) {   // reached by this query (never a connected one) and scored
                    accScore += mLoopScore_[s2];
                    if (mLoopScore_[s2] > bestScore) { best = s2; bestScore = mLoopScore_[s2]; }
                }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, best));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        return retain(lAccScoreAndMatch, 0.75f * bestAccScore);
    }
    // == DetectRelocalizationCandidates(F) src/KeyFrameDatabase.cc:199-309
    std::vector<int32_t> DetectRelocalizationCandidates(const std::vector<int32_t>& bowId, const std::vector<double>& bowVal,
                                                        const std::vector<std::vector<int32_t>>& neighbours) {
        const int minCommonWords = sharing(bowId, bowVal, nullptr, "KeyFrameDatabase::DetectRelocalizationCandidates");
        std::vector<std::pair<float, int32_t>> lScoreAndMatch, lAccScoreAndMatch;
        for (int32_t s : sharing_) {
            if (words_[s] > minCommonWords) {
                const float si = (float)score_[s];
                mRelocScore_[s] = si;
                lScoreAndMatch.push_back(std::make_pair(si, s));
            }
        }
        if (lScoreAndMatch.empty()) return std::vector<int32_t>();
        float bestAccScore = 0;
        for (const auto& it : lScoreAndMatch) {
            float bestScore = it.first, accScore = bestScore;
            int32_t best = it.second;
            for (int32_t s2 : neigh(neighbours, it.second)) {
                if (words_[s2] <= 0) continue;   // mnRelocQuery != F->mnId; no minCommonWords test (:273-281): the score may be an earlier query's
                accScore += mRelocScore_[s2];
                if (mRelocScore_[s2] > bestScore) { best = s2; bestScore = mRelocScore_[s2]; }
            }
            lAccScoreAndMatch.push_back(std::make_pair(accScore, best));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        return retain(lAccScoreAndMatch, 0.75f * bestAccScore);
    }

private:
    static void sameLength(const std::vector<int32_t>& id, const std::vector<double>& val, const char* who) {
        if (id.size() != val.size()) throw Error(PSLFE_E_INVALID, std::string(who) + ": word ids and values differ in length");
    }
    // the query; sharing_ = lKFsSharingWords as slots: words > 0 in ascending (first common word, order of the adds); returns minCommonWords
    int sharing(const std::vector<int32_t>& bowId, const std::vector<double>& bowVal, const uint8_t* exclude, const char* who) {
        sameLength(bowId, bowVal, who);
        words_.resize(K_); first_.resize(K_); score_.resize(K_); seq_.resize(K_);
        int maxCommonWords = 0;
        check(pslfe_kfdb_query(h_, bowId.data(), bowVal.data(), (int)bowId.size(), exclude, words_.data(), first_.data(), score_.data(), &maxCommonWords),
              "pslfe_kfdb_query");
        check(pslfe_kfdb_state(h_, nullptr, seq_.data()), "pslfe_kfdb_state");
        sharing_.clear();
        for (size_t s = 0; s < K_; ++s)
            if (words_[s] > 0) sharing_.push_back((int32_t)s);
        std::sort(sharing_.begin(), sharing_.end(), [this](int32_t a, int32_t b) {
            return first_[a] != first_[b] ? first_[a] < first_[b] : seq_[a] < seq_[b];
        });
        return (int)(maxCommonWords * 0.8f);
    }
    const std::vector<int32_t>& neigh(const std::vector<std::vector<int32_t>>& neighbours, int32_t slot) const {
        static const std::vector<int32_t> none;
        if ((size_t)slot >= neighbours.size()) return none;
        for (int32_t s2 : neighbours[slot])
            if (s2 < 0 || (size_t)s2 >= K_) throw Error(PSLFE_E_INVALID, "KeyFrameDatabase: neighbour slot out of range");
        return neighbours[slot];
    }
    static std::vector<int32_t> retain(const std::vector<std::pair<float, int32_t>>& lAccScoreAndMatch, float minScoreToRetain) {
        std::vector<int32_t> out;
        for (const auto& it : lAccScoreAndMatch)
            if (it.first > minScoreToRetain && std::find(out.begin(), out.end(), it.second) == out.end()) out.push_back(it.second);
        return out;
    }
    pslfe_kfdb* h_ = nullptr;
    size_t K_ = 0;
    std::vector<float> mLoopScore_, mRelocScore_;
    std::vector<int32_t> words_, first_, sharing_;
    std::vector<double> score_;
    std::vector<int64_t> seq_;
};

// == the KeyFrame-rate searches of LocalMapping / LoopClosing (pslfe_kf): ORBmatcher::Fuse (both overloads), SearchBySim3,
//    SearchForTriangulation (src/ORBmatcher.cc:657-1326), the search of LSDmatcher::Fuse (add_src/LSDmatcher.cpp:933-958) and
//    Map{Point,Line}::ComputeDistinctiveDescriptors, from the point where the host has projected its map points.  One per host
//    thread, on that thread's own Context.
class KeyFrameMatcher {
public:
    static constexpr int TH_HIGH = 100, TH_LOW = 50;
    explicit KeyFrameMatcher(Context& ctx) { check(pslfe_kf_create(ctx.get(), &h_), "pslfe_kf_create"); }
    ~KeyFrameMatcher() { pslfe_kf_destroy(h_); }
    KeyFrameMatcher(const KeyFrameMatcher&) = delete;
    KeyFrameMatcher& operator=(const KeyFrameMatcher&) = delete;

    // candidate loop of Fuse / SearchBySim3; invLevelSigma2 != nullptr selects the reprojection gates of Fuse(pKF, vpMapPoints, th)
    void WindowBest(FrameGrid& kf, int slot, const std::vector<PslProjQuery>& q, const std::vector<uint8_t>& qdesc,
                    const std::vector<float>* invLevelSigma2, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
        bestIdx.assign(q.size(), -1); bestDist.assign(q.size(), 0x7fffffff);
        check(pslfe_kf_window_best(h_, kf.get(), slot, q.data(), qdesc.data(), (int)q.size(), invLevelSigma2 ? 1 : 0,
                                   invLevelSigma2 ? invLevelSigma2->data() : nullptr, invLevelSigma2 ? (int)invLevelSigma2->size() : 0,
                                   bestIdx.data(), bestDist.data()), "pslfe_kf_window_best");
    }
    int SearchBySim3(FrameGrid& kf1, int slot1, FrameGrid& kf2, int slot2, const std::vector<PslProjQuery>& q12, const std::vector<uint8_t>& qdesc1,
                     const std::vector<PslProjQuery>& q21, const std::vector<uint8_t>& qdesc2, std::vector<int32_t>& match12) {
        match12.assign(q12.size(), -1);
        int nf = 0;
        check(pslfe_kf_search_by_sim3(h_, kf1.get(), slot1, kf2.get(), slot2, q12.data(), qdesc1.data(), (int)q12.size(), q21.data(), qdesc2.data(),
                                      (int)q21.size(), match12.data(), &nf), "pslfe_kf_search_by_sim3");
        return nf;
    }
    int SearchForTriangulation(FrameGrid& kf2, int slot2, const std::vector<int32_t>& fidx2, const std::vector<uint8_t>& taken2,
                               const std::vector<PslTriQuery>& q, const std::vector<uint8_t>& qdesc, const float F12[9], float ex, float ey,
                               bool bOnlyStereo, bool checkOrientation, const std::vector<float>& scaleFactors, const std::vector<float>& levelSigma2,
                               std::vector<int32_t>& match) {
        match.assign(q.size(), -1);
        int nm = 0;
        check(pslfe_kf_search_for_triangulation(h_, kf2.get(), slot2, fidx2.data(), (int)fidx2.size(), taken2.data(), q.data(), qdesc.data(),
                                                (int)q.size(), F12, ex, ey, bOnlyStereo, checkOrientation, scaleFactors.data(), levelSigma2.data(),
                                                (int)scaleFactors.size(), match.data(), &nm), "pslfe_kf_search_for_triangulation");
        return nm;
    }
    // SearchByBoW(pKF1, pKF2, vpMatches12) src/ORBmatcher.cc:522: fidx2 = KF2's FeatureVector flattened in node order without the
    // features that have no good map point; one query per KF1 feature with a good map point.  Returns nmatches.
    int SearchByBoW(FrameGrid& kf2, int slot2, const std::vector<int32_t>& fidx2, const std::vector<PslBowQuery>& q,
                    const std::vector<uint8_t>& qdesc, std::vector<int32_t>& match, float nnratio = 0.75f, bool checkOrientation = true) {
        match.assign(q.size(), -1);
        int nm = 0;
        check(pslfe_kf_search_by_bow(h_, kf2.get(), slot2, fidx2.data(), (int)fidx2.size(), q.data(), qdesc.data(), (int)q.size(), nnratio,
                                     checkOrientation, match.data(), &nm), "pslfe_kf_search_by_bow");
        return nm;
    }
    // the candidate loop of LoopClosing::ComputeSim3 src/LoopClosing.cc:252-284: candidate c = slot slots2[c], fidx2 / q / qdesc
    // concatenated over the candidates with fidx2Off / qOff (ncand + 1 entries from 0); nmatches[c] per candidate
    void SearchByBoWCandidates(FrameGrid& kf2, const std::vector<int32_t>& slots2, const std::vector<int32_t>& fidx2,
                               const std::vector<int32_t>& fidx2Off, const std::vector<PslBowQuery>& q, const std::vector<uint8_t>& qdesc,
                               const std::vector<int32_t>& qOff, std::vector<int32_t>& match, std::vector<int32_t>& nmatches,
                               float nnratio = 0.75f, bool checkOrientation = true) {
        if (fidx2Off.size() != slots2.size() + 1 || qOff.size() != slots2.size() + 1)
            throw Error(PSLFE_E_INVALID, "SearchByBoWCandidates: the offset arrays need one entry more than there are candidates");
        match.assign(q.size(), -1);
        nmatches.assign(slots2.size(), 0);
        check(pslfe_kf_search_by_bow_candidates(h_, kf2.get(), slots2.data(), (int)slots2.size(), fidx2.data(), fidx2Off.data(), q.data(),
                                                qdesc.data(), qOff.data(), nnratio, checkOrientation, match.data(), nmatches.data()),
              "pslfe_kf_search_by_bow_candidates");
    }
    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) src/ORBmatcher.cc:290 after the projection; taken: vpMatched[idx] != NULL
    // on entry, one byte per keypoint of the slot (empty = none).  assigned[c] = the map point now in vpMatched[c] or -1, sized here
    // by the slot's own keypoint count.  Returns nmatches.
    int SearchByProjectionSim3(FrameGrid& kf, int slot, const std::vector<PslProjQuery>& q, const std::vector<uint8_t>& qdesc,
                               const std::vector<uint8_t>& taken, std::vector<int32_t>& match, std::vector<int32_t>& assigned) {
        int n = 0;
        check(pslfe_frame_fetch(kf.get(), slot, nullptr, nullptr, nullptr, 0x7fffffff, &n), "pslfe_frame_fetch");
        if (!taken.empty() && (int)taken.size() != n) throw Error(PSLFE_E_INVALID, "SearchByProjectionSim3: taken needs one entry per keypoint of the slot");
        match.assign(q.size(), -1);
        assigned.assign(n, -1);
        int nm = 0;
        check(pslfe_kf_search_by_projection_sim3(h_, kf.get(), slot, q.data(), qdesc.data(), (int)q.size(), taken.empty() ? nullptr : taken.data(),
                                                 match.data(), assigned.data(), &nm), "pslfe_kf_search_by_projection_sim3");
        return nm;
    }
    // pslfe_kf_project: rows k*M + i = map point i in keyframe views[k] (mode PSLFE_KF_PROJ_FUSE / _SCW / _SIM3); skip: K*M bytes or
    // empty; bounds = {mnMinX, mnMinY, mnMaxX, mnMaxY}; level (may be nullptr) = nPredictedLevel or -1
    void Project(int mode, const std::vector<PslKfView>& views, const std::vector<PslMapPointGeom>& mp, const std::vector<uint8_t>& skip,
                 const PslCamera& cam, const float bounds[4], const std::vector<float>& scaleFactors, float logScaleFactor, float th,
                 std::vector<PslProjQuery>& rows, std::vector<int32_t>* level = nullptr) {
        const size_t n = views.size() * mp.size();
        checkSkip(skip, n, "Project");
        rows.assign(n, PslProjQuery{});
        if (level) level->assign(n, -1);
        check(pslfe_kf_project(h_, mode, views.data(), (int)views.size(), mp.data(), skip.empty() ? nullptr : skip.data(), (int)mp.size(), &cam,
                               bounds[0], bounds[1], bounds[2], bounds[3], scaleFactors.data(), (int)scaleFactors.size(), logScaleFactor, th,
                               rows.data(), level ? level->data() : nullptr), "pslfe_kf_project");
    }
    // Fuse(pKF, vpMapPoints, th) (PSLFE_KF_PROJ_FUSE, invLevelSigma2 required) or Fuse(pKF, Scw, ...) (PSLFE_KF_PROJ_SCW) up to bestDist for
    // the keyframes views[k].slot of `kf` against the same map points, projection included; rows (may be nullptr) for the host tail
    void FuseKeyFrames(FrameGrid& kf, int mode, const std::vector<PslKfView>& views, const std::vector<PslMapPointGeom>& mp,
                       const std::vector<uint8_t>& mpdesc, const std::vector<uint8_t>& skip, const PslCamera& cam, const float bounds[4],
                       const std::vector<float>& scaleFactors, const std::vector<float>* invLevelSigma2, float logScaleFactor, float th,
                       std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist, std::vector<PslProjQuery>* rows = nullptr) {
        const size_t n = views.size() * mp.size();
        checkSkip(skip, n, "FuseKeyFrames");
        if (mpdesc.size() != mp.size() * 32) throw Error(PSLFE_E_INVALID, "FuseKeyFrames: mpdesc needs 32 bytes per map point");
        if (invLevelSigma2 && invLevelSigma2->size() != scaleFactors.size())
            throw Error(PSLFE_E_INVALID, "FuseKeyFrames: invLevelSigma2 needs one entry per level");
        bestIdx.assign(n, -1); bestDist.assign(n, 0x7fffffff);
        if (rows) rows->assign(n, PslProjQuery{});
        check(pslfe_kf_fuse_keyframes(h_, kf.get(), mode, views.data(), (int)views.size(), mp.data(), mpdesc.data(),
                                      skip.empty() ? nullptr : skip.data(), (int)mp.size(), &cam, bounds[0], bounds[1], bounds[2], bounds[3],
                                      scaleFactors.data(), invLevelSigma2 ? invLevelSigma2->data() : nullptr, (int)scaleFactors.size(),
                                      logScaleFactor, th, bestIdx.data(), bestDist.data(), rows ? rows->data() : nullptr),
              "pslfe_kf_fuse_keyframes");
    }
    // SearchBySim3 with both projections on the device: view12 = {R1w t1w, sR21 t21, KF2's slot in kf2}, view21 = {R2w t2w, sR12 t12,
    // KF1's slot in kf1}; mp / desc / skip per entry of GetMapPointMatches() (skip may be empty).  Returns nFound.
    int SearchBySim3Poses(FrameGrid& kf1, FrameGrid& kf2, const PslKfView& view12, const std::vector<PslMapPointGeom>& mp1,
                          const std::vector<uint8_t>& desc1, const std::vector<uint8_t>& skip1, const PslKfView& view21,
                          const std::vector<PslMapPointGeom>& mp2, const std::vector<uint8_t>& desc2, const std::vector<uint8_t>& skip2,
                          const PslCamera& cam, const float bounds[4], const std::vector<float>& scaleFactors, float logScaleFactor, float th,
                          std::vector<int32_t>& match12, std::vector<PslProjQuery>* rows12 = nullptr, std::vector<PslProjQuery>* rows21 = nullptr) {
        checkSkip(skip1, mp1.size(), "SearchBySim3Poses");
        checkSkip(skip2, mp2.size(), "SearchBySim3Poses");
        if (desc1.size() != mp1.size() * 32 || desc2.size() != mp2.size() * 32)
            throw Error(PSLFE_E_INVALID, "SearchBySim3Poses: descriptors need 32 bytes per map point");
        match12.assign(mp1.size(), -1);
        if (rows12) rows12->assign(mp1.size(), PslProjQuery{});
        if (rows21) rows21->assign(mp2.size(), PslProjQuery{});
        int nf = 0;
        check(pslfe_kf_search_by_sim3_poses(h_, kf1.get(), kf2.get(), &view12, mp1.data(), desc1.data(), skip1.empty() ? nullptr : skip1.data(),
                                            (int)mp1.size(), &view21, mp2.data(), desc2.data(), skip2.empty() ? nullptr : skip2.data(),
                                            (int)mp2.size(), &cam, bounds[0], bounds[1], bounds[2], bounds[3], scaleFactors.data(),
                                            (int)scaleFactors.size(), logScaleFactor, th, match12.data(), &nf, rows12 ? rows12->data() : nullptr,
                                            rows21 ? rows21->data() : nullptr), "pslfe_kf_search_by_sim3_poses");
        return nf;
    }
    // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) from :312 on, projection included: view = {the decomposed Scw, -, the
    // keyframe's slot}; taken / match / assigned as SearchByProjectionSim3.  Returns nmatches.
    int SearchByProjectionSim3Pose(FrameGrid& kf, const PslKfView& view, const std::vector<PslMapPointGeom>& mp, const std::vector<uint8_t>& mpdesc,
                                   const std::vector<uint8_t>& skip, const PslCamera& cam, const float bounds[4],
                                   const std::vector<float>& scaleFactors, float logScaleFactor, float th, const std::vector<uint8_t>& taken,
                                   std::vector<int32_t>& match, std::vector<int32_t>& assigned, std::vector<PslProjQuery>* rows = nullptr) {
        checkSkip(skip, mp.size(), "SearchByProjectionSim3Pose");
        if (mpdesc.size() != mp.size() * 32) throw Error(PSLFE_E_INVALID, "SearchByProjectionSim3Pose: mpdesc needs 32 bytes per map point");
        int n = 0;
        check(pslfe_frame_fetch(kf.get(), view.slot, nullptr, nullptr, nullptr, 0x7fffffff, &n), "pslfe_frame_fetch");
        if (!taken.empty() && (int)taken.size() != n)
            throw Error(PSLFE_E_INVALID, "SearchByProjectionSim3Pose: taken needs one entry per keypoint of the slot");
        match.assign(mp.size(), -1);
        assigned.assign(n, -1);
        if (rows) rows->assign(mp.size(), PslProjQuery{});
        int nm = 0;
        check(pslfe_kf_search_by_projection_sim3_pose(h_, kf.get(), &view, mp.data(), mpdesc.data(), skip.empty() ? nullptr : skip.data(),
                                                      (int)mp.size(), &cam, bounds[0], bounds[1], bounds[2], bounds[3], scaleFactors.data(),
                                                      (int)scaleFactors.size(), logScaleFactor, th, taken.empty() ? nullptr : taken.data(),
                                                      match.data(), assigned.data(), &nm, rows ? rows->data() : nullptr),
              "pslfe_kf_search_by_projection_sim3_pose");
        return nm;
    }
    void LineFuse(const std::vector<PslKeyLine>& kls, const std::vector<uint8_t>& desc, const std::vector<PslLineFuseQuery>& q,
                  const std::vector<uint8_t>& qdesc, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist) {
        bestIdx.assign(q.size(), -1); bestDist.assign(q.size(), 256);
        check(pslfe_kf_line_fuse_best(h_, kls.data(), (int)kls.size(), desc.data(), (int)desc.size() / 32, q.data(), qdesc.data(), (int)q.size(),
                                      bestIdx.data(), bestDist.data()), "pslfe_kf_line_fuse_best");
    }
    // pslfe_kf_line_project: rows k*M + i = map line i in the keyframe with pose Tcw[k] (LSDmatcher::Fuse add_src/LSDmatcher.cpp:865-931);
    // skip: K*M bytes or empty; stop[k] = the line at which the reference returned, or M; level (may be nullptr) unclamped or INT32_MIN
    void LineProject(const std::vector<PslPose>& Tcw, const std::vector<PslMapLineGeom>& ml, const std::vector<uint8_t>& skip,
                     const PslCamera& cam, const float bounds[4], const std::vector<float>& scaleFactorsLine, float logScaleFactorLine, float th,
                     std::vector<PslLineFuseQuery>& rows, std::vector<int32_t>& stop, std::vector<int32_t>* level = nullptr) {
        const size_t n = Tcw.size() * ml.size();
        checkSkip(skip, n, "LineProject");
        rows.assign(n, PslLineFuseQuery{});
        stop.assign(Tcw.size(), (int32_t)ml.size());
        if (level) level->assign(n, INT32_MIN);
        check(pslfe_kf_line_project(h_, Tcw.data(), (int)Tcw.size(), ml.data(), skip.empty() ? nullptr : skip.data(), (int)ml.size(), &cam,
                                    bounds[0], bounds[1], bounds[2], bounds[3], scaleFactorsLine.data(), (int)scaleFactorsLine.size(),
                                    logScaleFactorLine, th, rows.data(), level ? level->data() : nullptr, stop.data()), "pslfe_kf_line_project");
    }
    // LSDmatcher::Fuse(pKF, vpMapLines, th) up to bestDist for the keyframes Tcw[k] against the same map lines, projection included:
    // keyframe k owns kls[klOff[k] .. klOff[k+1]) and the descriptor rows desc[descOff[k] .. descOff[k+1]); rows (may be nullptr) and
    // stop for the host tail, which applies the rows i < stop[k]
    void LineFuseKeyFrames(const std::vector<PslPose>& Tcw, const std::vector<PslKeyLine>& kls, const std::vector<int32_t>& klOff,
                           const std::vector<uint8_t>& desc, const std::vector<int32_t>& descOff, const std::vector<PslMapLineGeom>& ml,
                           const std::vector<uint8_t>& mldesc, const std::vector<uint8_t>& skip, const PslCamera& cam, const float bounds[4],
                           const std::vector<float>& scaleFactorsLine, float logScaleFactorLine, float th, std::vector<int32_t>& bestIdx,
                           std::vector<int32_t>& bestDist, std::vector<int32_t>& stop, std::vector<PslLineFuseQuery>* rows = nullptr) {
        const size_t n = Tcw.size() * ml.size();
        checkSkip(skip, n, "LineFuseKeyFrames");
        if (klOff.size() != Tcw.size() + 1 || descOff.size() != Tcw.size() + 1)
            throw Error(PSLFE_E_INVALID, "LineFuseKeyFrames: the offset arrays need one entry more than there are keyframes");
        if ((size_t)klOff.back() > kls.size() || (size_t)descOff.back() * 32 > desc.size())
            throw Error(PSLFE_E_INVALID, "LineFuseKeyFrames: the offsets run past the keylines or descriptors");
        if (mldesc.size() != ml.size() * 32) throw Error(PSLFE_E_INVALID, "LineFuseKeyFrames: mldesc needs 32 bytes per map line");
        bestIdx.assign(n, -1); bestDist.assign(n, 256);
        stop.assign(Tcw.size(), (int32_t)ml.size());
        if (rows) rows->assign(n, PslLineFuseQuery{});
        check(pslfe_kf_line_fuse_keyframes(h_, Tcw.data(), (int)Tcw.size(), kls.data(), klOff.data(), desc.data(), descOff.data(), ml.data(),
                                           mldesc.data(), skip.empty() ? nullptr : skip.data(), (int)ml.size(), &cam, bounds[0], bounds[1],
                                           bounds[2], bounds[3], scaleFactorsLine.data(), (int)scaleFactorsLine.size(), logScaleFactorLine, th,
                                           bestIdx.data(), bestDist.data(), rows ? rows->data() : nullptr, stop.data()),
              "pslfe_kf_line_fuse_keyframes");
    }
    // LSDmatcher::SearchForTriangulation of one keyframe against K neighbours (CreateNewMapLines2): neighbour k owns the LBD rows
    // ldesc2[off2[k] .. off2[k+1]); hasMapLine1 / hasMapLine2 (may be empty = none) one byte per line; TH_LOW + mutual for the pair-list
    // overload, TH_HIGH + isDouble for the vector<int> one.  match[k*n1 + i] = line of neighbour k or -1, nmatches[k] the return value
    void LineSearchForTriangulationKeyFrames(const std::vector<uint8_t>& ldesc1, const std::vector<uint8_t>& hasMapLine1,
                                             const std::vector<uint8_t>& ldesc2, const std::vector<int32_t>& off2,
                                             const std::vector<uint8_t>& hasMapLine2, float nnratio, float TH, bool mutual,
                                             std::vector<int32_t>& match, std::vector<int32_t>& nmatches) {
        if (off2.empty()) throw Error(PSLFE_E_INVALID, "LineSearchForTriangulationKeyFrames: off2 needs K + 1 entries");
        const size_t K = off2.size() - 1, n1 = ldesc1.size() / 32;
        if ((size_t)off2.back() * 32 > ldesc2.size() || (!hasMapLine1.empty() && hasMapLine1.size() != n1) ||
            (!hasMapLine2.empty() && hasMapLine2.size() != (size_t)off2.back()))
            throw Error(PSLFE_E_INVALID, "LineSearchForTriangulationKeyFrames: descriptor or GetMapLine arrays do not fit the offsets");
        match.assign(K * n1, -1);
        nmatches.assign(K, 0);
        check(pslfe_kf_line_search_for_triangulation_keyframes(h_, ldesc1.data(), (int)n1, hasMapLine1.empty() ? nullptr : hasMapLine1.data(),
                                                               ldesc2.data(), off2.data(), hasMapLine2.empty() ? nullptr : hasMapLine2.data(),
                                                               (int)K, nnratio, TH, mutual, match.data(), nmatches.data()),
              "pslfe_kf_line_search_for_triangulation_keyframes");
    }
    // offsets: npts + 1 entries; returns the best row of every point relative to its run
    std::vector<int32_t> ComputeDistinctiveDescriptors(const std::vector<uint8_t>& desc, const std::vector<int32_t>& offsets) {
        std::vector<int32_t> best(offsets.empty() ? 0 : offsets.size() - 1, -1);
        check(pslfe_kf_distinctive_descriptors(h_, desc.data(), offsets.data(), (int)best.size(), best.data()), "pslfe_kf_distinctive_descriptors");
        return best;
    }
    // MapPoint::UpdateNormalAndDepth src/MapPoint.cc:330-371 for every row of mp, in place: row i is observed from the camera centres
    // centres[3*obsKf[j]..] (KeyFrame::GetCameraCenter()), j in [obsOff[i], obsOff[i+1]), in the order in which mObservations iterates;
    // refKf / refLevel = mpRefKF and the octave of its observation; scaleFactors = mvScaleFactors; skip (mbBad): one byte per row or
    // empty.  Rows with an empty run or a skip byte keep every byte.
    void UpdateNormalAndDepth(std::vector<PslMapPointGeom>& mp, const std::vector<int32_t>& obsOff, const std::vector<int32_t>& obsKf,
                              const std::vector<float>& centres, const std::vector<int32_t>& refKf, const std::vector<int32_t>& refLevel,
                              const std::vector<uint8_t>& skip, const std::vector<float>& scaleFactors) {
        checkUpkeep(mp.size(), obsOff, obsKf, refKf, refLevel, skip, "UpdateNormalAndDepth");
        check(pslfe_kf_update_normal_and_depth(h_, mp.data(), (int)mp.size(), obsOff.data(), obsKf.data(), centres.data(), (int)centres.size() / 3,
                                               refKf.data(), refLevel.data(), skip.empty() ? nullptr : skip.data(), scaleFactors.data(),
                                               (int)scaleFactors.size()), "pslfe_kf_update_normal_and_depth");
    }
    // the same on device arrays, queued on the context's stream: the rows pslfe_orb_project_frustum_device reads, refreshed where they are
    void UpdateNormalAndDepthDevice(PslMapPointGeom* d_mp, int M, const int32_t* d_obsOff, const int32_t* d_obsKf, const float* d_centres, int nkf,
                                    const int32_t* d_refKf, const int32_t* d_refLevel, const uint8_t* d_skip,
                                    const std::vector<float>& scaleFactors) {
        check(pslfe_kf_update_normal_and_depth_device(h_, d_mp, M, d_obsOff, d_obsKf, d_centres, nkf, d_refKf, d_refLevel, d_skip,
                                                      scaleFactors.data(), (int)scaleFactors.size()), "pslfe_kf_update_normal_and_depth_device");
    }
    // MapLine::UpdateAverageDir add_src/MapLine.cpp:320-367, arguments as UpdateNormalAndDepth; scaleFactors = pRefKF->mvScaleFactors,
    // the point table, as the reference reads it
    void LineUpdateAverageDir(std::vector<PslMapLineGeom>& ml, const std::vector<int32_t>& obsOff, const std::vector<int32_t>& obsKf,
                              const std::vector<float>& centres, const std::vector<int32_t>& refKf, const std::vector<int32_t>& refLevel,
                              const std::vector<uint8_t>& skip, const std::vector<float>& scaleFactors) {
        checkUpkeep(ml.size(), obsOff, obsKf, refKf, refLevel, skip, "LineUpdateAverageDir");
        check(pslfe_kf_line_update_average_dir(h_, ml.data(), (int)ml.size(), obsOff.data(), obsKf.data(), centres.data(), (int)centres.size() / 3,
                                               refKf.data(), refLevel.data(), skip.empty() ? nullptr : skip.data(), scaleFactors.data(),
                                               (int)scaleFactors.size()), "pslfe_kf_line_update_average_dir");
    }
    void LineUpdateAverageDirDevice(PslMapLineGeom* d_ml, int M, const int32_t* d_obsOff, const int32_t* d_obsKf, const float* d_centres, int nkf,
                                    const int32_t* d_refKf, const int32_t* d_refLevel, const uint8_t* d_skip,
                                    const std::vector<float>& scaleFactors) {
        check(pslfe_kf_line_update_average_dir_device(h_, d_ml, M, d_obsOff, d_obsKf, d_centres, nkf, d_refKf, d_refLevel, d_skip,
                                                      scaleFactors.data(), (int)scaleFactors.size()), "pslfe_kf_line_update_average_dir_device");
    }
    // the layout of the run-order sums of the four refresh calls: PSLFE_UPKEEP_SUM_WALK or PSLFE_UPKEEP_SUM_TILED (same results)
    void SetUpkeepSum(int layout) { check(pslfe_kf_set_upkeep_sum(h_, layout), "pslfe_kf_set_upkeep_sum"); }
    // KeyFrame::ComputeSceneMedianDepth(q) src/KeyFrame.cc:749-779 for the keyframes Tcw[k]: keyframe k owns the world positions
    // x[3*off[k] .. 3*off[k+1]) of its map points (off: K + 1 entries from 0); -1 for a keyframe without map points
    std::vector<float> ComputeSceneMedianDepth(const std::vector<PslPose>& Tcw, const std::vector<float>& x, const std::vector<int32_t>& off, int q) {
        if (off.size() != Tcw.size() + 1 || (size_t)off.back() * 3 > x.size())
            throw Error(PSLFE_E_INVALID, "ComputeSceneMedianDepth: off needs K + 1 entries that stay inside x");
        std::vector<float> depth(Tcw.size(), 0.f);
        check(pslfe_kf_scene_median_depth(h_, Tcw.data(), (int)Tcw.size(), x.data(), off.data(), q, depth.data()), "pslfe_kf_scene_median_depth");
        return depth;
    }
    // LocalMapping::CreateNewMapPoints src/LocalMapping.cc:305-519 for mpCurrentKeyFrame against K neighbours in one call
    // (pslfe_kf_create_new_map_points; include/pslfe.h states every array).  The arrays of neighbour k lie at fidxOff[k] / kpOff[k]; its
    // query list at rows k*nqmax .. of queries, idx1 and qdesc.
    struct NewPointsIn {
        PslTriKeyFrame kf1;
        std::vector<PslKeyPoint> keysUn1;
        std::vector<float> keys1, uRight1, depth1;      // keys1: mvKeys[i].pt, 2 floats per feature
        std::vector<uint8_t> taken1;
        std::vector<PslTriNeighbour> neighbours;
        std::vector<int32_t> fidx2, fidxOff, kpOff;
        std::vector<uint8_t> taken2;
        std::vector<float> keys2, depth2;
        std::vector<PslTriQuery> queries;
        std::vector<int32_t> idx1, nq;
        std::vector<uint8_t> qdesc;
        int nqmax = 0;
        bool onlyStereo = false, checkOrientation = false;
        std::vector<float> scaleFactors, levelSigma2;
    };
    struct NewPointsOut {
        std::vector<int32_t> match, status, nmatches, createdBy;
        std::vector<float> x3d;
        std::vector<PslNewMapPoint> created;            // creation order: the order of mlpRecentAddedMapPoints
        std::vector<PslMapPointGeom> geom;
    };
    NewPointsOut CreateNewMapPoints(FrameGrid& kf2, const NewPointsIn& in) {
        const size_t K = in.neighbours.size(), N1 = in.keysUn1.size(), rows = K * (size_t)in.nqmax;
        if (in.keys1.size() != 2 * N1 || in.uRight1.size() != N1 || in.depth1.size() != N1 || in.taken1.size() != N1 || in.fidxOff.size() != K + 1 ||
            in.kpOff.size() != K + 1 || in.nq.size() != K || in.queries.size() != rows || in.idx1.size() != rows || in.qdesc.size() != rows * 32 ||
            in.scaleFactors.size() != in.levelSigma2.size() || (size_t)in.fidxOff.back() > in.fidx2.size() || (size_t)in.kpOff.back() > in.taken2.size() ||
            in.keys2.size() != 2 * in.taken2.size() || in.depth2.size() != in.taken2.size())
            throw Error(PSLFE_E_INVALID, "CreateNewMapPoints: the arrays do not fit the counts");
        NewPointsOut o;
        o.match.assign(rows, -1); o.status.assign(rows, PSL_TRI_NO_MATCH); o.x3d.assign(rows * 3, 0.f); o.nmatches.assign(K, 0);
        o.createdBy.assign(N1, -1); o.created.resize(N1); o.geom.resize(N1);
        int32_t nnew = 0;
        check(pslfe_kf_create_new_map_points(h_, kf2.get(), &in.kf1, (int)N1, in.keysUn1.data(), in.keys1.data(), in.uRight1.data(), in.depth1.data(),
                                             in.taken1.data(), in.neighbours.data(), (int)K, in.fidx2.data(), in.fidxOff.data(), in.taken2.data(),
                                             in.keys2.data(), in.depth2.data(), in.kpOff.data(), in.queries.data(), in.idx1.data(), in.qdesc.data(),
                                             in.nq.data(), in.nqmax, in.onlyStereo ? 1 : 0, in.checkOrientation ? 1 : 0, in.scaleFactors.data(),
                                             in.levelSigma2.data(), (int)in.scaleFactors.size(), o.match.data(), o.status.data(), o.x3d.data(),
                                             o.nmatches.data(), o.createdBy.data(), o.created.data(), &nnew, o.geom.data()),
              "pslfe_kf_create_new_map_points");
        o.created.resize(nnew); o.geom.resize(nnew);
        return o;
    }
    // The same on device arrays (pslfe_kf_create_new_map_points_device), queued on the context's stream: the per-neighbour host arrays and
    // the level tables stay host vectors, everything else is HBM.  d_geom and the four observation arrays are what
    // UpdateNormalAndDepthDevice takes with M = N1, so MapPoint::UpdateNormalAndDepth (:512) needs no read-back of the count.
    struct NewPointsDevice {
        const PslKeyPoint* d_keysUn1; const float* d_keys1; const float* d_uRight1; const float* d_depth1; const uint8_t* d_taken1;
        const int32_t* d_fidx2; const uint8_t* d_taken2; const float* d_keys2; const float* d_depth2;
        const PslTriQuery* d_queries; const int32_t* d_idx1; const uint8_t* d_qdesc;
        int32_t* d_match; int32_t* d_status; float* d_x3d; int32_t* d_nmatches; int32_t* d_createdBy; PslNewMapPoint* d_created; int32_t* d_nnew;
        PslMapPointGeom* d_geom; int32_t* d_obsOff; int32_t* d_obsKf; int32_t* d_refKf; int32_t* d_refLevel;
    };
    void CreateNewMapPointsDevice(FrameGrid& kf2, const PslTriKeyFrame& kf1, int N1, const std::vector<PslTriNeighbour>& neighbours,
                                  const std::vector<int32_t>& fidxOff, const std::vector<int32_t>& kpOff, const std::vector<int32_t>& nq, int nqmax,
                                  bool onlyStereo, bool checkOrientation, const std::vector<float>& scaleFactors,
                                  const std::vector<float>& levelSigma2, const NewPointsDevice& d) {
        const size_t K = neighbours.size();
        if (fidxOff.size() != K + 1 || kpOff.size() != K + 1 || nq.size() != K || scaleFactors.size() != levelSigma2.size())
            throw Error(PSLFE_E_INVALID, "CreateNewMapPointsDevice: the host arrays do not fit the neighbours");
        check(pslfe_kf_create_new_map_points_device(h_, kf2.get(), &kf1, N1, d.d_keysUn1, d.d_keys1, d.d_uRight1, d.d_depth1, d.d_taken1,
                                                    neighbours.data(), (int)K, d.d_fidx2, fidxOff.data(), d.d_taken2, d.d_keys2, d.d_depth2, kpOff.data(),
                                                    d.d_queries, d.d_idx1, d.d_qdesc, nq.data(), nqmax, onlyStereo ? 1 : 0, checkOrientation ? 1 : 0,
                                                    scaleFactors.data(), levelSigma2.data(), (int)scaleFactors.size(), d.d_match, d.d_status, d.d_x3d,
                                                    d.d_nmatches, d.d_createdBy, d.d_created, d.d_nnew, d.d_geom, d.d_obsOff, d.d_obsKf, d.d_refKf,
                                                    d.d_refLevel), "pslfe_kf_create_new_map_points_device");
    }
    // LocalMapping::CreateNewMapLines2 :554-757 (pslfe_kf_create_new_map_lines): the search of LineSearchForTriangulationKeyFrames, then
    // the pair body.  Neighbour k's lines lie at off2[k] .. off2[k+1] of desc2, hasMapLine2 (may be empty), keyLines2, lines3d2.
    struct NewLinesIn {
        PslTriKeyFrame kf1;
        std::vector<uint8_t> desc1, hasMapLine1;        // hasMapLine1 may be empty: none
        std::vector<PslKeyLine> keyLines1;
        std::vector<double> lines3d1;                   // mvLines3D, 6 per line
        std::vector<float> lineEq1;                     // mvLineEq[i][2]
        std::vector<PslTriNeighbour> neighbours;
        std::vector<uint8_t> desc2, hasMapLine2;
        std::vector<int32_t> off2;
        std::vector<PslKeyLine> keyLines2;
        std::vector<double> lines3d2;
        float nnratio = 0.95f, TH = 50.f;
        bool mutual = true;
        std::vector<float> scaleFactors, levelSigma2;   // the POINT tables
    };
    struct NewLinesOut {
        std::vector<int32_t> match, status, nmatches, createdBy;
        std::vector<float> sp, ep;
        std::vector<PslNewMapLine> created;
        std::vector<PslMapLineGeom> geom;
    };
    NewLinesOut CreateNewMapLines(const NewLinesIn& in) {
        const size_t K = in.neighbours.size(), n1 = in.keyLines1.size(), rows = K * n1;
        if (in.desc1.size() != n1 * 32 || (!in.hasMapLine1.empty() && in.hasMapLine1.size() != n1) || in.lines3d1.size() != 6 * n1 || in.lineEq1.size() != n1 ||
            in.off2.size() != K + 1 || (size_t)in.off2.back() > in.keyLines2.size() || in.desc2.size() != in.keyLines2.size() * 32 ||
            in.lines3d2.size() != in.keyLines2.size() * 6 || (!in.hasMapLine2.empty() && in.hasMapLine2.size() != in.keyLines2.size()) ||
            in.scaleFactors.size() != in.levelSigma2.size())
            throw Error(PSLFE_E_INVALID, "CreateNewMapLines: the arrays do not fit the counts");
        NewLinesOut o;
        o.match.assign(rows, -1); o.status.assign(rows, PSL_TRIL_NO_MATCH); o.sp.assign(rows * 3, 0.f); o.ep.assign(rows * 3, 0.f);
        o.nmatches.assign(K, 0); o.createdBy.assign(n1, -1); o.created.resize(n1); o.geom.resize(n1);
        int32_t nnew = 0;
        check(pslfe_kf_create_new_map_lines(h_, &in.kf1, (int)n1, in.desc1.data(), in.hasMapLine1.empty() ? nullptr : in.hasMapLine1.data(),
                                            in.keyLines1.data(), in.lines3d1.data(), in.lineEq1.data(), in.neighbours.data(), (int)K, in.desc2.data(),
                                            in.off2.data(), in.hasMapLine2.empty() ? nullptr : in.hasMapLine2.data(), in.keyLines2.data(),
                                            in.lines3d2.data(), in.nnratio, in.TH, in.mutual ? 1 : 0, in.scaleFactors.data(), in.levelSigma2.data(),
                                            (int)in.scaleFactors.size(), o.match.data(), o.status.data(), o.sp.data(), o.ep.data(), o.nmatches.data(),
                                            o.createdBy.data(), o.created.data(), &nnew, o.geom.data()),
              "pslfe_kf_create_new_map_lines");
        o.created.resize(nnew); o.geom.resize(nnew);
        return o;
    }
    // The same on device arrays (pslfe_kf_create_new_map_lines_device); d_geom and the runs are what LineUpdateAverageDirDevice takes with
    // M = NL1.  d_hasMapLine1 / d_hasMapLine2 may be nullptr: none.
    struct NewLinesDevice {
        const uint8_t* d_desc1; const uint8_t* d_hasMapLine1; const PslKeyLine* d_keyLines1; const double* d_lines3d1; const float* d_lineEq1;
        const uint8_t* d_desc2; const uint8_t* d_hasMapLine2; const PslKeyLine* d_keyLines2; const double* d_lines3d2;
        int32_t* d_match; int32_t* d_status; float* d_sp; float* d_ep; int32_t* d_nmatches; int32_t* d_createdBy; PslNewMapLine* d_created;
        int32_t* d_nnew; PslMapLineGeom* d_geom; int32_t* d_obsOff; int32_t* d_obsKf; int32_t* d_refKf; int32_t* d_refLevel;
    };
    void CreateNewMapLinesDevice(const PslTriKeyFrame& kf1, int NL1, const std::vector<PslTriNeighbour>& neighbours, const std::vector<int32_t>& off2,
                                 float nnratio, float TH, bool mutual, const std::vector<float>& scaleFactors, const std::vector<float>& levelSigma2,
                                 const NewLinesDevice& d) {
        if (off2.size() != neighbours.size() + 1 || scaleFactors.size() != levelSigma2.size())
            throw Error(PSLFE_E_INVALID, "CreateNewMapLinesDevice: the host arrays do not fit the neighbours");
        check(pslfe_kf_create_new_map_lines_device(h_, &kf1, NL1, d.d_desc1, d.d_hasMapLine1, d.d_keyLines1, d.d_lines3d1, d.d_lineEq1, neighbours.data(),
                                                   (int)neighbours.size(), d.d_desc2, off2.data(), d.d_hasMapLine2, d.d_keyLines2, d.d_lines3d2, nnratio, TH,
                                                   mutual ? 1 : 0, scaleFactors.data(), levelSigma2.data(), (int)scaleFactors.size(), d.d_match, d.d_status,
                                                   d.d_sp, d.d_ep, d.d_nmatches, d.d_createdBy, d.d_created, d.d_nnew, d.d_geom, d.d_obsOff, d.d_obsKf,
                                                   d.d_refKf, d.d_refLevel), "pslfe_kf_create_new_map_lines_device");
    }
private:
    static void checkUpkeep(size_t n, const std::vector<int32_t>& obsOff, const std::vector<int32_t>& obsKf, const std::vector<int32_t>& refKf,
                            const std::vector<int32_t>& refLevel, const std::vector<uint8_t>& skip, const char* who) {
        if (obsOff.size() != n + 1 || refKf.size() != n || refLevel.size() != n || (!skip.empty() && skip.size() != n) ||
            (size_t)obsOff.back() > obsKf.size())
            throw Error(PSLFE_E_INVALID, std::string(who) + ": the offsets, references or skip bytes do not fit the rows");
    }
    static void checkSkip(const std::vector<uint8_t>& skip, size_t n, const char* who) {
        if (!skip.empty() && skip.size() != n) throw Error(PSLFE_E_INVALID, std::string(who) + ": skip needs one byte per (keyframe, map point)");
    }
    pslfe_kf* h_ = nullptr;
};

// == Optimizer (include/Optimizer.h:58): PoseOptimization, src/Optimizer.cc:239-1023: the monocular and stereo point edges and the
//    LIL edges (EdgeLILSE3ProjectXYZ, :619-694, :973-1008; the overloads and methods that take PslPoseLilEdge rows).  Parity with g2o
//    itself is unpinned.
// The workspaces of the local bundle adjustment (pslfe_ba): up to maxProblems problems per launch of up to maxKeyframes keyframes
// (free and fixed), maxPoints points and maxEdges edges each.  A single owner frees every buffer.
class BundleAdjuster {
public:
    BundleAdjuster(Context& ctx, int maxProblems, int maxKeyframes, int maxPoints, int maxEdges) {
        check(pslfe_ba_create(ctx.get(), maxProblems, maxKeyframes, maxPoints, maxEdges, &h_), "pslfe_ba_create");
    }
    // with room for maxLils VertexLIL rows and maxLilEdges LIL edges per problem (LocalBundleAdjustmentAndInseclines)
    BundleAdjuster(Context& ctx, int maxProblems, int maxKeyframes, int maxPoints, int maxEdges, int maxLils, int maxLilEdges) {
        check(pslfe_ba_create_lil(ctx.get(), maxProblems, maxKeyframes, maxPoints, maxEdges, maxLils, maxLilEdges, &h_), "pslfe_ba_create_lil");
    }
    ~BundleAdjuster() { pslfe_ba_destroy(h_); }
    BundleAdjuster(const BundleAdjuster&) = delete;
    BundleAdjuster& operator=(const BundleAdjuster&) = delete;
    pslfe_ba* get() const { return h_; }
private:
    pslfe_ba* h_ = nullptr;
};

// The workspace of the global bundle adjustment (pslfe_gba): one problem of up to maxKeyframes keyframes (at most 4096), maxPoints
// points and maxEdges edges, spread over the whole device.  A single owner frees every buffer.
class GlobalBundleAdjuster {
public:
    GlobalBundleAdjuster(Context& ctx, int maxKeyframes, int maxPoints, int maxEdges) {
        check(pslfe_gba_create(ctx.get(), maxKeyframes, maxPoints, maxEdges, &h_), "pslfe_gba_create");
    }
    ~GlobalBundleAdjuster() { pslfe_gba_destroy(h_); }
    GlobalBundleAdjuster(const GlobalBundleAdjuster&) = delete;
    GlobalBundleAdjuster& operator=(const GlobalBundleAdjuster&) = delete;
    pslfe_gba* get() const { return h_; }
private:
    pslfe_gba* h_ = nullptr;
};

// The workspaces of the essential-graph optimisation (pslfe_eg): up to maxGraphs graphs per launch of up to maxKeyframes keyframes,
// maxEdges edges, maxPoints map points and maxEnvelope doubles of envelope each.  A single owner frees every buffer.
class EssentialGraph {
public:
    EssentialGraph(Context& ctx, int maxGraphs, int maxKeyframes, int maxEdges, int maxPoints, int64_t maxEnvelope) {
        check(pslfe_eg_create(ctx.get(), maxGraphs, maxKeyframes, maxEdges, maxPoints, maxEnvelope, &h_), "pslfe_eg_create");
    }
    ~EssentialGraph() { pslfe_eg_destroy(h_); }
    EssentialGraph(const EssentialGraph&) = delete;
    EssentialGraph& operator=(const EssentialGraph&) = delete;
    pslfe_eg* get() const { return h_; }
private:
    pslfe_eg* h_ = nullptr;
};

// What Optimizer::OptimizeEssentialGraph reads off the pointer graph, as arrays over the keyframe rows (ascending mnId, bad keyframes
// left out, so comparing rows compares mnIds).
struct EssentialGraphLinks {
    std::vector<int32_t> parent;                                  // the row of GetParent() or -1
    std::vector<std::vector<int32_t>> loopEdges;                  // the rows of GetLoopEdges(), in the set's order
    std::vector<std::vector<int32_t>> covisibles;                 // the rows of GetCovisiblesByWeight(100), in its order, bad ones left out
    struct Connection { int32_t kf; std::vector<std::pair<int32_t, int>> to; };   // (row, GetWeight(row))
    std::vector<Connection> loopConnections;                      // in the order the map and its sets iterate
    int32_t loopKF = -1, curKF = -1;                              // the rows of pLoopKF / pCurKF
};

class Optimizer {
public:
    // The edge rows of Optimizer::OptimizeEssentialGraph in the order the reference creates them (src/Optimizer.cc:2607-2738): the
    // LoopConnections pairs with weight >= minFeat or (curKF, loopKF) itself, flagged loop (they fill sInsertedEdges); then per row i its
    // spanning-tree edge (i, parent), its loop edges (i, l) with l < i, and its covisibility edges (i, n) with n < i that are neither the
    // parent, a child, a loop edge nor in sInsertedEdges.
    static std::vector<PslEgEdge> EssentialGraphEdges(const EssentialGraphLinks& g, int minFeat = 100) {
        std::vector<PslEgEdge> out;
        std::vector<std::pair<int32_t, int32_t>> inserted;
        auto key = [](int32_t a, int32_t b) { return std::make_pair(a < b ? a : b, a < b ? b : a); };
        for (const auto& c : g.loopConnections)
            for (const auto& jw : c.to) {
                if ((c.kf != g.curKF || jw.first != g.loopKF) && jw.second < minFeat) continue;
                out.push_back(PslEgEdge{c.kf, jw.first, 1});
                inserted.push_back(key(c.kf, jw.first));
            }
        for (int32_t i = 0; i < (int32_t)g.parent.size(); ++i) {
            const int32_t p = g.parent[i];
            if (p >= 0) out.push_back(PslEgEdge{i, p, 0});
            const std::vector<int32_t>& le = g.loopEdges[i];
            for (int32_t l : le)
                if (l < i) out.push_back(PslEgEdge{i, l, 0});
            for (int32_t n : g.covisibles[i]) {
                if (n < 0 || n == p || g.parent[n] == i || n >= i) continue;
                bool skip = false;
                for (int32_t l : le) skip = skip || l == n;
                for (const auto& k : inserted) skip = skip || k == key(i, n);
                if (!skip) out.push_back(PslEgEdge{i, n, 0});
            }
        }
        return out;
    }
    // void Optimizer::OptimizeEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale)
    // src/Optimizer.cc:2536-2799 from the measurements on: kfs = one row per keyframe that is not bad in ascending mnId, edges =
    // EssentialGraphEdges, mps with mpRef[p] = the row nIDr of :2775-2784 or -1 for a point that is copied.  mps come back as
    // SetWorldPos gets them, poses = Tiw of :2762 for SetPose, S = the optimised Sim3s ([8] doubles per keyframe).  A refused graph
    // (capacity, an edge or a point outside it) throws.  Parity with g2o itself is unpinned.
    static PslEgInfo OptimizeEssentialGraph(EssentialGraph& eg, const std::vector<PslEgKeyFrame>& kfs, const std::vector<PslEgEdge>& edges,
                                            std::vector<PslMapPointGeom>& mps, const std::vector<int32_t>& mpRef, bool fixScale,
                                            std::vector<PslPose>& poses, std::vector<double>& S) {
        poses.resize(kfs.size());
        S.resize(8 * kfs.size());
        PslEgInfo info = {};
        check(mpRef.size() == mps.size() ? PSLFE_OK : PSLFE_E_INVALID, "OptimizeEssentialGraph: mpRef needs one entry per map point");
        check(pslfe_eg_optimize(eg.get(), kfs.data(), (int)kfs.size(), edges.data(), (int)edges.size(), mps.data(), mpRef.data(), (int)mps.size(),
                                fixScale ? 1 : 0, poses.data(), S.data(), mps.data(), &info), "pslfe_eg_optimize");
        return info;
    }
    // K graphs in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_eg_optimize_device
    static void OptimizeEssentialGraphDevice(EssentialGraph& eg, int K, const PslEgKeyFrame* d_kf, const int32_t* d_kfOff, const PslEgEdge* d_edges,
                                             const int32_t* d_edgeOff, const PslMapPointGeom* d_mp, const int32_t* d_mpRef, const int32_t* d_mpOff,
                                             bool fixScale, PslPose* d_poseOut, double* d_SOut, PslMapPointGeom* d_mpOut, PslEgInfo* d_info) {
        check(pslfe_eg_optimize_device(eg.get(), K, d_kf, d_kfOff, d_edges, d_edgeOff, d_mp, d_mpRef, d_mpOff, fixScale ? 1 : 0, d_poseOut, d_SOut,
                                       d_mpOut, d_info), "pslfe_eg_optimize_device");
    }
    // int Optimizer::PoseOptimization(Frame* pFrame): edges = one PslPoseEdge per non-NULL pFrame->mvpMapPoints[i] in keypoint order
    // (:282-363); Tcw = pFrame->mTcw, replaced by the pose :1020 sets; outlier[e] = mvbOutlier of the edge's keypoint; returns
    // nInitialCorrespondences - nBad.  Fewer than 3 edges: returns 0, Tcw unchanged, outlier all false (:291, :696).
    static int PoseOptimization(Context& ctx, PslPose& Tcw, const std::vector<PslPoseEdge>& edges, const PslCamera& cam,
                                std::vector<uint8_t>& outlier) {
        outlier.assign(edges.size(), 0);
        int ngood = 0;
        check(pslfe_pose_optimize(ctx.get(), &Tcw, edges.data(), (int)edges.size(), &cam, &Tcw, outlier.data(), &ngood), "pslfe_pose_optimize");
        return ngood;
    }
    // The same with the frame's LIL edges: lil = one PslPoseLilEdge per live, not bad pFrame->mvpMapInsecs[i] in plane order (:631-693);
    // outlierLil[e] = mvbOutlier_Insec of the edge's plane.  The return value counts every LIL edge as good (:1022).
    static int PoseOptimization(Context& ctx, PslPose& Tcw, const std::vector<PslPoseEdge>& edges, const std::vector<PslPoseLilEdge>& lil,
                                const PslCamera& cam, std::vector<uint8_t>& outlier, std::vector<uint8_t>& outlierLil) {
        outlier.assign(edges.size(), 0);
        outlierLil.assign(lil.size(), 0);
        int ngood = 0;
        check(pslfe_pose_optimize_lil(ctx.get(), &Tcw, edges.data(), (int)edges.size(), lil.data(), (int)lil.size(), &cam, &Tcw, outlier.data(),
                                      outlierLil.data(), &ngood), "pslfe_pose_optimize_lil");
        return ngood;
    }
    // K frames in one launch, HBM to HBM, asynchronous on the context's stream (the many-frames mode): pslfe_pose_optimize_device
    static void PoseOptimizationDevice(Context& ctx, int nframes, const PslPose* d_TcwIn, const PslPoseEdge* d_edges, const int32_t* d_nedges,
                                       int estride, const PslCamera& cam, PslPose* d_TcwOut, uint8_t* d_outlier, int32_t* d_ngood,
                                       PslPoseInfo* d_info = nullptr) {
        check(pslfe_pose_optimize_device(ctx.get(), nframes, d_TcwIn, d_edges, d_nedges, estride, &cam, d_TcwOut, d_outlier, d_ngood, d_info),
              "pslfe_pose_optimize_device");
    }
    // the same with LIL edges: pslfe_pose_optimize_lil_device
    static void PoseOptimizationLilDevice(Context& ctx, int nframes, const PslPose* d_TcwIn, const PslPoseEdge* d_edges, const int32_t* d_nedges,
                                          int estride, const PslPoseLilEdge* d_lil, const int32_t* d_nlil, int lstride, const PslCamera& cam,
                                          PslPose* d_TcwOut, uint8_t* d_outlier, uint8_t* d_outlierLil, int32_t* d_ngood,
                                          PslPoseInfo* d_info = nullptr) {
        check(pslfe_pose_optimize_lil_device(ctx.get(), nframes, d_TcwIn, d_edges, d_nedges, estride, d_lil, d_nlil, lstride, &cam, d_TcwOut,
                                             d_outlier, d_outlierLil, d_ngood, d_info), "pslfe_pose_optimize_lil_device");
    }
    // the LIL set-up loop :631-693 for nframes frames, HBM to HBM: pslfe_pose_lil_edges_device (the observation arrays are those of
    // FrameGlue::lilObsDevice)
    static void LilEdgesDevice(Context& ctx, int nframes, const double* d_leL, int leStride, const double* d_cross2d, int planeStride,
                               const int32_t* d_nplanes, const int32_t* d_lilIndex, const PslMapLil* d_map, int nmap, PslPoseLilEdge* d_lil,
                               int32_t* d_edgePlane, int32_t* d_nlil, int lstride) {
        check(pslfe_pose_lil_edges_device(ctx.get(), nframes, d_leL, leStride, d_cross2d, planeStride, d_nplanes, d_lilIndex, d_map, nmap, d_lil,
                                          d_edgePlane, d_nlil, lstride), "pslfe_pose_lil_edges_device");
    }
    // F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:127) for nframes frames, HBM to HBM: pslfe_pose_mp_index_from_matches_device
    static void MapPointIndexFromMatchesDevice(FrameGrid& frame, int nframes, const int32_t* d_match, const int32_t* d_owner, const int32_t* d_nq,
                                               int qstride, int32_t* d_mpIndex) {
        check(pslfe_pose_mp_index_from_matches_device(frame.get(), nframes, d_match, d_owner, d_nq, qstride, d_mpIndex),
              "pslfe_pose_mp_index_from_matches_device");
    }
    // the edge set-up loop :282-363 from the matches of nframes frames, HBM to HBM: pslfe_pose_edges_from_matches_device
    static void EdgesFromMatchesDevice(FrameGrid& frame, int slot0, int nframes, const int32_t* d_mpIndex, const PslMapPointGeom* d_mp, int mpStride,
                                       const std::vector<float>& invLevelSigma2, PslPoseEdge* d_edges, int32_t* d_edgeKp, int32_t* d_nedges,
                                       int estride) {
        check(pslfe_pose_edges_from_matches_device(frame.get(), slot0, nframes, d_mpIndex, d_mp, mpStride, invLevelSigma2.data(),
                                                   (int)invLevelSigma2.size(), d_edges, d_edgeKp, d_nedges, estride),
              "pslfe_pose_edges_from_matches_device");
    }
    // void Optimizer::LocalBundleAdjustment(pKF, pbStopFlag, pMap) src/Optimizer.cc:1025-1966 from optimizer.initializeOptimization()
    // (:1642) on, its point edges: kfs = lLocalKeyFrames then lFixedCameras (fixed set for those and for mnId == 0), mps =
    // lLocalMapPoints, edges in the order the reference creates them (INTEGRATION.md "LocalBundleAdjustment").  kfs and mps come
    // back optimised, erase[e] = 1 where the reference puts the edge's pair into vToErase.  doMore = false is bDoMore == false.
    // A refused problem (capacity, an edge outside it, a duplicate pair) throws.  Parity with g2o itself is unpinned.
    static PslBaInfo LocalBundleAdjustment(BundleAdjuster& ba, std::vector<PslBaKeyFrame>& kfs, std::vector<PslMapPointGeom>& mps,
                                           const std::vector<PslBaEdge>& edges, const PslCamera& cam, std::vector<uint8_t>& erase,
                                           bool doMore = true) {
        erase.assign(edges.size(), 0);
        PslBaInfo info = {};
        check(pslfe_ba_local(ba.get(), kfs.data(), (int)kfs.size(), mps.data(), (int)mps.size(), edges.data(), (int)edges.size(), &cam,
                             doMore ? 2 : 1, kfs.data(), mps.data(), erase.data(), &info), "pslfe_ba_local");
        return info;
    }
    // K problems in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_ba_local_device
    static void LocalBundleAdjustmentDevice(BundleAdjuster& ba, int K, const PslBaKeyFrame* d_kf, const int32_t* d_kfOff, const PslMapPointGeom* d_mp,
                                            const int32_t* d_mpOff, const PslBaEdge* d_edges, const int32_t* d_edgeOff, const PslCamera& cam,
                                            int rounds, PslBaKeyFrame* d_kfOut, PslMapPointGeom* d_mpOut, uint8_t* d_erase, PslBaInfo* d_info) {
        check(pslfe_ba_local_device(ba.get(), K, d_kf, d_kfOff, d_mp, d_mpOff, d_edges, d_edgeOff, &cam, rounds, d_kfOut, d_mpOut, d_erase, d_info),
              "pslfe_ba_local_device");
    }
    // void Optimizer::LocalBundleAdjustmentAndInseclines(pKF, pbStopFlag, pMap) src/Optimizer.cc:1968-2534, the call of LocalMapping::Run
    // (src/LocalMapping.cc:84): LocalBundleAdjustment plus lils = one PslMapLil per local InsectLine (:2250-2290, ascending mnId for
    // g2o's order) and lilEdges = one PslBaLilEdge per (LIL, observing keyframe that is not bad) in the order the reference creates
    // them (:2295-2346).  lils come back with their 15 doubles (:2526-2531), eraseLil[e] = 1 where :2464-2478 flag the edge.  ba needs
    // LIL caps.  The update of a VertexLIL follows add_inc/VertexLIL.h:23-27 under the reading of DESIGN.md §3; parity with g2o is unpinned.
    static PslBaInfo LocalBundleAdjustmentAndInseclines(BundleAdjuster& ba, std::vector<PslBaKeyFrame>& kfs, std::vector<PslMapPointGeom>& mps,
                                                        const std::vector<PslBaEdge>& edges, std::vector<PslMapLil>& lils,
                                                        const std::vector<PslBaLilEdge>& lilEdges, const PslCamera& cam, std::vector<uint8_t>& erase,
                                                        std::vector<uint8_t>& eraseLil, bool doMore = true) {
        erase.assign(edges.size(), 0);
        eraseLil.assign(lilEdges.size(), 0);
        PslBaInfo info = {};
        check(pslfe_ba_local_lil(ba.get(), kfs.data(), (int)kfs.size(), mps.data(), (int)mps.size(), edges.data(), (int)edges.size(), lils.data(),
                                 (int)lils.size(), lilEdges.data(), (int)lilEdges.size(), &cam, doMore ? 2 : 1, kfs.data(), mps.data(), erase.data(),
                                 lils.data(), eraseLil.data(), &info), "pslfe_ba_local_lil");
        return info;
    }
    // K problems in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_ba_local_lil_device (d_nerasedLil may be NULL)
    static void LocalBundleAdjustmentAndInseclinesDevice(BundleAdjuster& ba, int K, const PslBaKeyFrame* d_kf, const int32_t* d_kfOff,
                                                         const PslMapPointGeom* d_mp, const int32_t* d_mpOff, const PslBaEdge* d_edges,
                                                         const int32_t* d_edgeOff, const PslMapLil* d_lil, const int32_t* d_lilOff,
                                                         const PslBaLilEdge* d_lilEdges, const int32_t* d_lilEdgeOff, const PslCamera& cam, int rounds,
                                                         PslBaKeyFrame* d_kfOut, PslMapPointGeom* d_mpOut, uint8_t* d_erase, PslMapLil* d_lilOut,
                                                         uint8_t* d_eraseLil, int32_t* d_nerasedLil, PslBaInfo* d_info) {
        check(pslfe_ba_local_lil_device(ba.get(), K, d_kf, d_kfOff, d_mp, d_mpOff, d_edges, d_edgeOff, d_lil, d_lilOff, d_lilEdges, d_lilEdgeOff, &cam,
                                        rounds, d_kfOut, d_mpOut, d_erase, d_lilOut, d_eraseLil, d_nerasedLil, d_info), "pslfe_ba_local_lil_device");
    }
    // void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust) src/Optimizer.cc:49-237 from the
    // optimiser's set-up on: kfs = the keyframes that are not bad (fixed = mnId == 0, :79), mps = the points that are not bad, edges
    // in the order the reference creates them (:89-173).  EVERY keyframe comes back as toCvMat of its SE3Quat (the fixed one too,
    // :193-210), a point with an edge as (float) of its estimate; notIncluded[p] = vbNotIncludedMP (:175-183).  Whether the rows
    // go to SetPose / SetWorldPos or to mTcwGBA / mPosGBA (nLoopKF) is the caller's matter.  robust = true sets Huber with
    // (float)sqrt(5.99) / (float)sqrt(7.815) (:85-86).  A refused problem throws.  Parity with g2o itself is unpinned.
    static PslGbaInfo BundleAdjustment(GlobalBundleAdjuster& gba, std::vector<PslBaKeyFrame>& kfs, std::vector<PslMapPointGeom>& mps,
                                       const std::vector<PslBaEdge>& edges, const PslCamera& cam, std::vector<uint8_t>& notIncluded,
                                       int nIterations = 5, bool robust = true) {
        notIncluded.assign(mps.size(), 0);
        PslGbaInfo info = {};
        check(pslfe_gba_optimize(gba.get(), kfs.data(), (int)kfs.size(), mps.data(), (int)mps.size(), edges.data(), (int)edges.size(), &cam, nIterations,
                                 robust ? 1 : 0, kfs.data(), mps.data(), notIncluded.data(), &info), "pslfe_gba_optimize");
        return info;
    }
    // the same on rows in HBM (pslfe_gba_optimize_device): returns when the outputs are written; d_kfOut may be d_kf, d_mpOut d_mp
    static PslGbaInfo BundleAdjustmentDevice(GlobalBundleAdjuster& gba, const PslBaKeyFrame* d_kf, int nkf, const PslMapPointGeom* d_mp, int nmp,
                                             const PslBaEdge* d_edges, int nedges, const PslCamera& cam, int nIterations, bool robust,
                                             PslBaKeyFrame* d_kfOut, PslMapPointGeom* d_mpOut, uint8_t* d_notIncluded) {
        PslGbaInfo info = {};
        check(pslfe_gba_optimize_device(gba.get(), d_kf, nkf, d_mp, nmp, d_edges, nedges, &cam, nIterations, robust ? 1 : 0, d_kfOut, d_mpOut,
                                        d_notIncluded, &info), "pslfe_gba_optimize_device");
        return info;
    }
    // void Optimizer::GlobalBundleAdjustemnt(pMap, nIterations, pbStopFlag, nLoopKF, bRobust) src/Optimizer.cc:37-46 (the reference's
    // spelling): BundleAdjustment over GetAllKeyFrames() and GetAllMapPoints()
    static PslGbaInfo GlobalBundleAdjustemnt(GlobalBundleAdjuster& gba, std::vector<PslBaKeyFrame>& kfs, std::vector<PslMapPointGeom>& mps,
                                             const std::vector<PslBaEdge>& edges, const PslCamera& cam, std::vector<uint8_t>& notIncluded,
                                             int nIterations = 5, bool robust = true) {
        return BundleAdjustment(gba, kfs, mps, edges, cam, notIncluded, nIterations, robust);
    }
    static PslGbaInfo GlobalBundleAdjustemntDevice(GlobalBundleAdjuster& gba, const PslBaKeyFrame* d_kf, int nkf, const PslMapPointGeom* d_mp, int nmp,
                                                   const PslBaEdge* d_edges, int nedges, const PslCamera& cam, int nIterations, bool robust,
                                                   PslBaKeyFrame* d_kfOut, PslMapPointGeom* d_mpOut, uint8_t* d_notIncluded) {
        return BundleAdjustmentDevice(gba, d_kf, nkf, d_mp, nmp, d_edges, nedges, cam, nIterations, robust, d_kfOut, d_mpOut, d_notIncluded);
    }
    // int Optimizer::OptimizeSim3(pKF1, pKF2, vpMatches1, g2oS12, th2, bFixScale) src/Optimizer.cc:2801-2996: pairs = one PslSim3Pair per
    // match that passes the set-up loop (:2854-2933), in KF1 keypoint order; S12 = what Sim3Solver hands over (src/LoopClosing.cc:
    // 320-325); S12Out = the g2o::Sim3 that comes back, or Sim3(R, t, s) of the input where the reference returns 0 before writing
    // g2oS12 (:2966); bad[p] = 1 where the reference nulls vpMatches1[idx]; returns nIn.  Parity with g2o itself is unpinned.
    static int OptimizeSim3(Context& ctx, const PslSim3& S12, const std::vector<PslSim3Pair>& pairs, const PslCamera& cam1, const PslCamera& cam2,
                            float th2, bool fixScale, PslSim3D& S12Out, std::vector<uint8_t>& bad) {
        bad.assign(pairs.size(), 0);
        int nin = 0;
        check(pslfe_sim3_optimize(ctx.get(), &S12, pairs.data(), (int)pairs.size(), &cam1, &cam2, th2, fixScale ? 1 : 0, &S12Out, bad.data(), &nin),
              "pslfe_sim3_optimize");
        return nin;
    }
    // K candidates in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_sim3_optimize_device
    static void OptimizeSim3Device(Context& ctx, int ncand, const PslSim3* d_S12In, const PslSim3Pair* d_pairs, const int32_t* d_npairs, int pstride,
                                   const PslCamera& cam1, const PslCamera& cam2, float th2, bool fixScale, PslSim3D* d_S12Out, uint8_t* d_bad,
                                   int32_t* d_nin, PslSim3Info* d_info = nullptr) {
        check(pslfe_sim3_optimize_device(ctx.get(), ncand, d_S12In, d_pairs, d_npairs, pstride, &cam1, &cam2, th2, fixScale ? 1 : 0, d_S12Out, d_bad,
                                         d_nin, d_info), "pslfe_sim3_optimize_device");
    }
    // the set-up loop :2854-2933 for ncand candidates of one current keyframe, HBM to HBM: pslfe_sim3_pairs_from_matches_device
    static void Sim3PairsFromMatchesDevice(FrameGrid& f1, int slot1, FrameGrid& f2, const int32_t* d_slots2, int ncand, const int32_t* d_i2,
                                           const PslMapPointGeom* d_mp1, const uint8_t* d_skip1, int n1, const PslMapPointGeom* d_mp2,
                                           const uint8_t* d_skip2, int mp2Stride, const PslPose* d_T1w, const PslPose* d_T2w,
                                           const std::vector<float>& invLevelSigma2, PslSim3Pair* d_pairs, int32_t* d_pairKp, int32_t* d_npairs,
                                           int pstride) {
        check(pslfe_sim3_pairs_from_matches_device(f1.get(), slot1, f2.get(), d_slots2, ncand, d_i2, d_mp1, d_skip1, n1, d_mp2, d_skip2, mp2Stride,
                                                   d_T1w, d_T2w, invLevelSigma2.data(), (int)invLevelSigma2.size(), d_pairs, d_pairKp, d_npairs,
                                                   pstride), "pslfe_sim3_pairs_from_matches_device");
    }
    // the same set-up with mvLevelSigma2 of both octaves of each row in d_sigma2 [ncand][pstride][2], what Sim3Solver needs next to the rows
    static void Sim3PairsSigma2FromMatchesDevice(FrameGrid& f1, int slot1, FrameGrid& f2, const int32_t* d_slots2, int ncand, const int32_t* d_i2,
                                                 const PslMapPointGeom* d_mp1, const uint8_t* d_skip1, int n1, const PslMapPointGeom* d_mp2,
                                                 const uint8_t* d_skip2, int mp2Stride, const PslPose* d_T1w, const PslPose* d_T2w,
                                                 const std::vector<float>& invLevelSigma2, const std::vector<float>& levelSigma2,
                                                 PslSim3Pair* d_pairs, int32_t* d_pairKp, int32_t* d_npairs, int pstride, float* d_sigma2) {
        if (levelSigma2.size() != invLevelSigma2.size()) throw Error(PSLFE_E_INVALID, "Sim3PairsSigma2FromMatchesDevice: the two level tables differ in size");
        check(pslfe_sim3_pairs_sigma2_from_matches_device(f1.get(), slot1, f2.get(), d_slots2, ncand, d_i2, d_mp1, d_skip1, n1, d_mp2, d_skip2,
                                                          mp2Stride, d_T1w, d_T2w, invLevelSigma2.data(), (int)invLevelSigma2.size(), d_pairs,
                                                          d_pairKp, d_npairs, pstride, levelSigma2.data(), d_sigma2),
              "pslfe_sim3_pairs_sigma2_from_matches_device");
    }
};

// Sim3Solver (src/Sim3Solver.cc) of one candidate, with the reference's method names.  The constructor takes what the reference's
// constructor builds (:62-103): the rows of the set-up loop (P1c, P2c are read), mvLevelSigma2 of the two octaves of each row,
// mvnIndices1 (row -> KF1 keypoint) and vpMatched12.size().  rand() is glibc's generator seeded with `seed` at the solver's first
// iteration; iterate() resumes the solver through (mnIterations, mnBestInliers), so rounds of iterate(5) are one find().
class Sim3Solver {
public:
    Sim3Solver(Context& ctx, std::vector<PslSim3Pair> pairs, std::vector<float> sigma2, std::vector<int32_t> indices1, int nKeys1,
               const PslCamera& cam1, const PslCamera& cam2, bool fixScale, uint32_t seed)
        : ctx_(&ctx), pairs_(std::move(pairs)), sigma2_(std::move(sigma2)), indices1_(std::move(indices1)), nKeys1_(nKeys1), cam1_(cam1),
          cam2_(cam2), fixScale_(fixScale), seed_(seed) {
        if (sigma2_.size() != 2 * pairs_.size() || indices1_.size() != pairs_.size()) throw Error(PSLFE_E_INVALID, "Sim3Solver: array sizes differ");
        std::memset(&res_, 0, sizeof(res_));
        SetRansacParameters();
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
        prob_ = probability; minInliers_ = minInliers; maxIts_ = maxIterations;
        res_.iterations = 0;   // mnIterations = 0 (:137); mnBestInliers stays
    }
    // cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers): true when a Sim3 was returned (GetEstimated* then hold it)
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        std::vector<uint8_t> flags(pairs_.size() ? pairs_.size() : 1, 0);
        PslSim3SolverResult r;
        check(pslfe_sim3_solve(ctx_->get(), pairs_.data(), sigma2_.data(), (int)pairs_.size(), &cam1_, &cam2_, prob_, minInliers_, maxIts_,
                               fixScale_ ? 1 : 0, seed_, res_.iterations, res_.best_inliers, nIterations, &r, flags.data()),
              "pslfe_sim3_solve");
        if (r.status < 0) throw Error(r.status, "pslfe_sim3_solve");
        const PslSim3 kept = res_.S12;
        res_ = r;
        if (r.status != 1) res_.S12 = kept;   // mBestRotation / Translation / Scale as the last returned hypothesis left them
        bNoMore = r.status == 2;
        nInliers = r.ninliers;
        vbInliers.assign((size_t)nKeys1_, false);
        if (r.status == 1)
            for (size_t i = 0; i < pairs_.size(); ++i)
                if (flags[i] && indices1_[i] >= 0 && indices1_[i] < nKeys1_) vbInliers[(size_t)indices1_[i]] = true;
        rowFlags_.assign(flags.begin(), flags.begin() + pairs_.size());
        return r.status == 1;
    }
    bool find(std::vector<bool>& vbInliers12, int& nInliers) {
        bool flag;
        return iterate(maxIts_, flag, vbInliers12, nInliers);
    }
    const float* GetEstimatedRotation() const { return res_.S12.R; }      // 3x3 row-major
    const float* GetEstimatedTranslation() const { return res_.S12.t; }
    float GetEstimatedScale() const { return res_.S12.s; }
    const PslSim3SolverResult& result() const { return res_; }            // of the last call
    const std::vector<uint8_t>& rowInliers() const { return rowFlags_; }  // the flags of the last call by pair row

    // K candidates in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_sim3_solve_device
    static void SolveDevice(Context& ctx, int ncand, const PslSim3Pair* d_pairs, const float* d_sigma2, const int32_t* d_npairs, int pstride,
                            const PslCamera& cam1, const PslCamera& cam2, double prob, int minInliers, int maxIts, bool fixScale, uint32_t seed0,
                            const int32_t* d_startIt, const int32_t* d_bestIn, int nIterations, PslSim3SolverResult* d_res, uint8_t* d_inliers) {
        check(pslfe_sim3_solve_device(ctx.get(), ncand, d_pairs, d_sigma2, d_npairs, pstride, &cam1, &cam2, prob, minInliers, maxIts,
                                      fixScale ? 1 : 0, seed0, d_startIt, d_bestIn, nIterations, d_res, d_inliers),
              "pslfe_sim3_solve_device");
    }

    // The candidate loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:284-345) for K candidates resident in HBM: rounds of
    // iterate(5) for every candidate that is still in the race, one launch per round.  A candidate that returns a Sim3 is handed to
    // `accept(round, c, result, rowInliers)` in the order the reference would try it (by round, then by index); accept does what :313-340 do
    // (SearchBySim3, OptimizeSim3) and returns true to end the loop (bMatch).  bNoMore discards a candidate; a count below 0 or above
    // pstride discards it at once.  Returns the accepted candidate or -1.
    template <class Accept>
    static int ComputeSim3Candidates(Context& ctx, int ncand, const PslSim3Pair* d_pairs, const float* d_sigma2, const int32_t* d_npairs,
                                     int pstride, const PslCamera& cam1, const PslCamera& cam2, bool fixScale, uint32_t seed0, Accept accept,
                                     double prob = 0.99, int minInliers = 20, int maxIts = 300, int perRound = 5) {
        if (ncand <= 0) return -1;
        std::vector<int32_t> startIt((size_t)ncand, 0), bestIn((size_t)ncand, 0);
        std::vector<uint8_t> discarded((size_t)ncand, 0), flags((size_t)ncand * (pstride ? pstride : 1));
        std::vector<PslSim3SolverResult> res((size_t)ncand);
        void *dS = nullptr, *dB = nullptr, *dR = nullptr, *dF = nullptr;
        auto release = [&]() { for (void* p : {dS, dB, dR, dF}) if (p) pslfe_device_free(ctx.get(), p); };
        try {
            check(pslfe_device_alloc(ctx.get(), (size_t)ncand * 4, &dS), "pslfe_device_alloc");
            check(pslfe_device_alloc(ctx.get(), (size_t)ncand * 4, &dB), "pslfe_device_alloc");
            check(pslfe_device_alloc(ctx.get(), (size_t)ncand * sizeof(PslSim3SolverResult), &dR), "pslfe_device_alloc");
            check(pslfe_device_alloc(ctx.get(), flags.size(), &dF), "pslfe_device_alloc");
            int live = ncand;
            for (int round = 0; live > 0; ++round) {
                check(pslfe_device_upload(ctx.get(), dS, startIt.data(), (size_t)ncand * 4), "pslfe_device_upload");
                check(pslfe_device_upload(ctx.get(), dB, bestIn.data(), (size_t)ncand * 4), "pslfe_device_upload");
                SolveDevice(ctx, ncand, d_pairs, d_sigma2, d_npairs, pstride, cam1, cam2, prob, minInliers, maxIts, fixScale, seed0,
                            (const int32_t*)dS, (const int32_t*)dB, perRound, (PslSim3SolverResult*)dR, (uint8_t*)dF);
                check(pslfe_device_download(ctx.get(), res.data(), dR, (size_t)ncand * sizeof(PslSim3SolverResult)), "pslfe_device_download");
                check(pslfe_device_download(ctx.get(), flags.data(), dF, flags.size()), "pslfe_device_download");
                for (int c = 0; c < ncand; ++c) {
                    if (discarded[c]) continue;
                    const PslSim3SolverResult& r = res[c];
                    if (r.status < 0 || r.status == 2) { discarded[c] = 1; --live; }
                    if (r.status < 0) continue;
                    startIt[c] = r.iterations;
                    bestIn[c] = r.best_inliers;
                    if (r.status == 1 && accept(round, c, r, (const uint8_t*)flags.data() + (size_t)c * pstride)) { release(); return c; }
                }
                // a discarded candidate runs no further iteration: its start is at the end of every budget
                for (int c = 0; c < ncand; ++c)
                    if (discarded[c]) startIt[c] = maxIts;
            }
        } catch (...) {
            release();
            throw;
        }
        release();
        return -1;
    }

private:
    Context* ctx_;
    std::vector<PslSim3Pair> pairs_;
    std::vector<float> sigma2_;
    std::vector<int32_t> indices1_;
    int nKeys1_;
    PslCamera cam1_, cam2_;
    bool fixScale_;
    uint32_t seed_;
    double prob_ = 0.99;
    int minInliers_ = 6, maxIts_ = 300;
    PslSim3SolverResult res_;
    std::vector<uint8_t> rowFlags_;
};

// PnPsolver (src/PnPsolver.cc) of one relocalisation candidate, with the reference's method names.  The constructor takes what the
// reference's constructor builds (:67-110): the rows of its loop (mvP2D, mvP3Dw, mvSigma2), mvKeyPointIndices (row -> keypoint of F)
// and vpMapPointMatches.size().  rand() is glibc's generator seeded with `seed` at the solver's first iteration; iterate() resumes the
// solver through (mnIterations, mnBestInliers, mBestTcw, mvbBestInliers), also after a returned pose.
class PnPsolver {
public:
    PnPsolver(Context& ctx, std::vector<PslPnpRow> rows, std::vector<int32_t> keyPointIndices, int nKeys, const PslCamera& cam, uint32_t seed)
        : ctx_(&ctx), rows_(std::move(rows)), kp_(std::move(keyPointIndices)), nKeys_(nKeys), cam_(cam), seed_(seed) {
        if (kp_.size() != rows_.size()) throw Error(PSLFE_E_INVALID, "PnPsolver: array sizes differ");
        std::memset(&res_, 0, sizeof(res_));
        bestFlags_.assign(rows_.size() ? rows_.size() : 1, 0);
        SetRansacParameters();
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                             float th2 = 5.991f) {
        prob_ = probability; minInliers_ = minInliers; maxIts_ = maxIterations; minSet_ = minSet; epsilon_ = epsilon; th2_ = th2;
    }
    // cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers): true when a pose was returned (Tcw() then holds it)
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
        std::vector<uint8_t> flags(rows_.size() ? rows_.size() : 1, 0);
        PslPnpResult r;
        check(pslfe_pnp_solve(ctx_->get(), rows_.data(), (int)rows_.size(), &cam_, prob_, minInliers_, maxIts_, minSet_, epsilon_, th2_, seed_, &res_,
                              bestFlags_.data(), nIterations, &r, flags.data()),
              "pslfe_pnp_solve");
        if (r.status < 0) throw Error(r.status, "pslfe_pnp_solve");
        res_ = r;
        bNoMore = (r.status & 2) != 0;
        nInliers = r.inliers;
        vbInliers.clear();
        if (r.status & 1) {
            vbInliers.assign((size_t)nKeys_, false);
            for (size_t i = 0; i < rows_.size(); ++i)
                if (flags[i] && kp_[i] >= 0 && kp_[i] < nKeys_) vbInliers[(size_t)kp_[i]] = true;
        }
        rowFlags_.assign(flags.begin(), flags.begin() + rows_.size());
        return (r.status & 1) != 0;
    }
    bool find(std::vector<bool>& vbInliers, int& nInliers) {
        bool flag;
        int its = 0, minIn = 0;   // mRansacMaxIts after the clamps
        check(pslfe_pnp_ransac_parameters(prob_, minInliers_, maxIts_, minSet_, epsilon_, (int)rows_.size(), &its, &minIn), "pslfe_pnp_ransac_parameters");
        return iterate(its, flag, vbInliers, nInliers);
    }
    const PslPose& Tcw() const { return res_.Tcw; }                       // the pose the last call returned
    const PslPnpResult& result() const { return res_; }                   // of the last call
    const std::vector<uint8_t>& rowInliers() const { return rowFlags_; }  // the flags of the last call by row

    // K candidates in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_pnp_solve_device
    static void SolveDevice(Context& ctx, int ncand, const PslPnpRow* d_rows, const int32_t* d_nrows, int rstride, const PslCamera& cam, double prob,
                            int minInliers, int maxIts, int minSet, float epsilon, float th2, uint32_t seed0, const PslPnpResult* d_stateIn,
                            uint8_t* d_bestFlags, int nIterations, PslPnpResult* d_res, uint8_t* d_inliers) {
        check(pslfe_pnp_solve_device(ctx.get(), ncand, d_rows, d_nrows, rstride, &cam, prob, minInliers, maxIts, minSet, epsilon, th2, seed0,
                                     d_stateIn, d_bestFlags, nIterations, d_res, d_inliers),
              "pslfe_pnp_solve_device");
    }

    // The candidate loop of Tracking::Relocalization (src/Tracking.cc:2088-2180) for K candidates resident in HBM: rounds of iterate(5)
    // for every candidate that is still in the race, one launch per round.  A candidate that returns a pose is handed to
    // `accept(round, c, result, rowInliers)` in the order the reference would try it (by round, then by index); accept does what
    // :2107-2172 do (PoseOptimization, the two SearchByProjection) and returns true to end the loop (bMatch).  bNoMore discards a
    // candidate (:2103-2107; its pose, if it came with one, is still tried); a count below 0 or above rstride discards it at once.  A
    // discarded candidate is parked with a negative state, which the kernel answers without solving.  A candidate whose every call
    // returns a refined pose never says bNoMore (the reference's loop ends on it only through bMatch): the loop gives up after
    // maxRounds rounds.  Returns the accepted candidate or -1.
    template <class Accept>
    static int RelocalizeCandidates(Context& ctx, int ncand, const PslPnpRow* d_rows, const int32_t* d_nrows, int rstride, const PslCamera& cam,
                                    uint32_t seed0, Accept accept, double prob = 0.99, int minInliers = 10, int maxIts = 300,
                                    float epsilon = 0.5f, float th2 = 5.991f, int perRound = 5, int maxRounds = 1000) {
        if (ncand <= 0) return -1;
        std::vector<uint8_t> discarded((size_t)ncand, 0), flags((size_t)ncand * (rstride ? rstride : 1));
        std::vector<PslPnpResult> state((size_t)ncand), res((size_t)ncand);
        std::memset(state.data(), 0, state.size() * sizeof(PslPnpResult));
        void *dS = nullptr, *dB = nullptr, *dR = nullptr, *dF = nullptr;
        auto release = [&]() { for (void* p : {dS, dB, dR, dF}) if (p) pslfe_device_free(ctx.get(), p); };
        try {
            check(pslfe_device_alloc(ctx.get(), state.size() * sizeof(PslPnpResult), &dS), "pslfe_device_alloc");
            check(pslfe_device_alloc(ctx.get(), state.size() * sizeof(PslPnpResult), &dR), "pslfe_device_alloc");
            check(pslfe_device_alloc(ctx.get(), flags.size(), &dB), "pslfe_device_alloc");
            check(pslfe_device_alloc(ctx.get(), flags.size(), &dF), "pslfe_device_alloc");
            check(pslfe_device_upload(ctx.get(), dB, flags.data(), flags.size()), "pslfe_device_upload");
            int live = ncand;
            for (int round = 0; live > 0 && round < maxRounds; ++round) {
                check(pslfe_device_upload(ctx.get(), dS, state.data(), state.size() * sizeof(PslPnpResult)), "pslfe_device_upload");
                SolveDevice(ctx, ncand, d_rows, d_nrows, rstride, cam, prob, minInliers, maxIts, 4, epsilon, th2, seed0, (const PslPnpResult*)dS,
                            (uint8_t*)dB, perRound, (PslPnpResult*)dR, (uint8_t*)dF);
                check(pslfe_device_download(ctx.get(), res.data(), dR, res.size() * sizeof(PslPnpResult)), "pslfe_device_download");
                check(pslfe_device_download(ctx.get(), flags.data(), dF, flags.size()), "pslfe_device_download");
                for (int c = 0; c < ncand; ++c) {
                    if (discarded[c]) continue;
                    const PslPnpResult& r = res[c];
                    if (r.status < 0 || (r.status & 2)) { discarded[c] = 1; --live; state[c].iterations = -1; }
                    if (r.status < 0) continue;
                    if (!discarded[c]) state[c] = r;
                    if ((r.status & 1) && accept(round, c, r, (const uint8_t*)flags.data() + (size_t)c * rstride)) { release(); return c; }
                }
            }
        } catch (...) {
            release();
            throw;
        }
        release();
        return -1;
    }

private:
    Context* ctx_;
    std::vector<PslPnpRow> rows_;
    std::vector<int32_t> kp_;
    int nKeys_;
    PslCamera cam_;
    uint32_t seed_;
    double prob_ = 0.99;
    int minInliers_ = 8, maxIts_ = 300, minSet_ = 4;
    float epsilon_ = 0.4f, th2_ = 5.991f;
    PslPnpResult res_;
    std::vector<uint8_t> bestFlags_, rowFlags_;
};

// == ORB_SLAM2::Initializer (src/Initializer.cc) of one reference frame: the constructor takes what the reference's takes from the
// frame (:33-42): its undistorted keypoints (x, y pairs) and K; sigma = 1.0 and iterations = 200 as in include/Initializer.h.
// rand() is glibc's generator seeded with `seed` at every Initialize (the reference seeds once per process with 0: seed 0 is its first
// Initialize).  Parity with OpenCV is unpinned.
class Initializer {
public:
    Initializer(Context& ctx, std::vector<float> referenceKeysXY, const PslCamera& K, float sigma = 1.0f, int iterations = 200, uint32_t seed = 0)
        : ctx_(&ctx), keys1_(std::move(referenceKeysXY)), cam_(K), sigma_(sigma), maxIts_(iterations), seed_(seed) {
        if (keys1_.size() % 2) throw Error(PSLFE_E_INVALID, "Initializer: an odd number of coordinates");
        std::memset(&res_, 0, sizeof(res_));
    }
    // bool Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) (:44-121): currentKeysXY = CurrentFrame.mvKeysUn as
    // x, y pairs; R21 [9] row-major and t21 [3]; vP3D [n1][3] flattened
    bool Initialize(const std::vector<float>& currentKeysXY, const std::vector<int32_t>& vMatches12, float* R21, float* t21,
                    std::vector<float>& vP3D, std::vector<bool>& vbTriangulated) {
        const int n1 = (int)(keys1_.size() / 2), n2 = (int)(currentKeysXY.size() / 2);
        if ((int)vMatches12.size() != n1) throw Error(PSLFE_E_INVALID, "Initializer: vMatches12 has one entry per reference keypoint");
        std::vector<uint8_t> tri((size_t)n1 ? (size_t)n1 : 1, 0);
        vP3D.assign(3 * (size_t)n1, 0.f);
        check(pslfe_init_initialize(ctx_->get(), keys1_.data(), n1, currentKeysXY.data(), n2, vMatches12.data(), &cam_, sigma_, maxIts_, seed_,
                                    &res_, vP3D.data(), tri.data()),
              "pslfe_init_initialize");
        vbTriangulated.assign((size_t)n1, false);
        for (int i = 0; i < n1; ++i) vbTriangulated[(size_t)i] = tri[(size_t)i] != 0;
        for (int k = 0; k < 9; ++k) R21[k] = res_.R21[k];
        for (int k = 0; k < 3; ++k) t21[k] = res_.t21[k];
        return (res_.status & 1) != 0;
    }
    const PslInitResult& result() const { return res_; }   // of the last call

    // mvSets (:77-97) of a pair with N matches: [iterations][8]
    static std::vector<int32_t> Sets(uint32_t seed, int N, int iterations) {
        std::vector<int32_t> s(8 * (size_t)(iterations > 0 ? iterations : 0) + 1);
        check(pslfe_init_sets(seed, N, iterations, s.data()), "pslfe_init_sets");
        s.resize(8 * (size_t)iterations);
        return s;
    }
    // K pairs in one launch, HBM to HBM, asynchronous on the context's stream: pslfe_init_initialize_device
    static void InitializeDevice(Context& ctx, int npairs, const void* d_keys1, const int32_t* d_nkeys1, const void* d_keys2, const int32_t* d_nkeys2,
                                 int keyStrideBytes, int kstride, const int32_t* d_matches12, int mstride, const PslCamera& K, float sigma,
                                 int iterations, uint32_t seed0, PslInitResult* d_res, float* d_p3d, uint8_t* d_triangulated,
                                 int32_t* d_matches12Out) {
        check(pslfe_init_initialize_device(ctx.get(), npairs, d_keys1, d_nkeys1, d_keys2, d_nkeys2, keyStrideBytes, kstride, d_matches12, mstride, &K,
                                           sigma, iterations, seed0, d_res, d_p3d, d_triangulated, d_matches12Out),
              "pslfe_init_initialize_device");
    }
    // The same with the keypoints of frame slots, straight behind ORBmatcher::SearchForInitializationDevice with its d_matches12:
    // pair p = (f1 slot slot1[p], f2 slot slot2[p]); mstride >= f1's capacity.  pslfe_init_initialize_frames_device
    static void InitializeFramesDevice(FrameGrid& f1, const std::vector<int32_t>& slot1, FrameGrid& f2, const std::vector<int32_t>& slot2,
                                       const int32_t* d_matches12, int mstride, const PslCamera& K, float sigma, int iterations, uint32_t seed0,
                                       PslInitResult* d_res, float* d_p3d, uint8_t* d_triangulated, int32_t* d_matches12Out) {
        if (slot1.size() != slot2.size()) throw Error(PSLFE_E_INVALID, "Initializer: slot1 and slot2 differ in length");
        check(pslfe_init_initialize_frames_device(f1.get(), slot1.data(), f2.get(), slot2.data(), (int)slot1.size(), d_matches12, mstride, &K, sigma,
                                                  iterations, seed0, d_res, d_p3d, d_triangulated, d_matches12Out),
              "pslfe_init_initialize_frames_device");
    }

private:
    Context* ctx_;
    std::vector<float> keys1_;
    PslCamera cam_;
    float sigma_;
    int maxIts_;
    uint32_t seed_;
    PslInitResult res_;
};

}  // namespace pslfe
#endif
