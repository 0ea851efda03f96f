// libpslfe: the stereo Frame constructor (src/Frame.cc:75-131) on rectified pairs already extracted on the device.  Product code.
// Reference behaviour reproduced: Frame::ComputeStereoMatches src/Frame.cc:1165-1340 (stereo_kernels.h), then
// UndistortKeyPoints, ComputeImageBounds and AssignFeaturesToGrid as the RGB-D path does them (pslfe_match.hip).
#include <string.h>

#include <algorithm>

#include "pslfe_internal.h"
#include "match_kernels.h"
#include "stereo_kernels.h"

namespace {

// The stereo buffers of f, sized for this call: the taps ([max_frames][cap], once) and the right keypoints' row CSR (grown).
// All or nothing: after a failed allocation every stereo buffer is released and its size reset, so the next call on f allocates
// them all again (or fails again) - no call ever launches with one of them missing.
int st_buffers(pslfe_frame* f, size_t taps, size_t rowstart, size_t rowidx) {
    if (f->d_st_idx && f->d_st_sad && f->d_st_rowstart && f->d_st_rowidx && rowstart <= f->st_rowstart_cap && rowidx <= f->st_rowidx_cap)
        return PSLFE_OK;
    PSL_HIP(hipStreamSynchronize(f->ctx->stream));   // earlier work may still read the buffers replaced here
    PslDeviceBuffers& m = f->mem;
    if (!f->d_st_idx || !f->d_st_sad) {
        m.release(f->d_st_idx); m.release(f->d_st_sad);
        m.alloc(f->d_st_idx, taps, "d_st_idx");
        m.alloc(f->d_st_sad, taps, "d_st_sad");
    }
    if (!f->d_st_rowstart || rowstart > f->st_rowstart_cap) {
        m.release(f->d_st_rowstart);
        m.alloc(f->d_st_rowstart, rowstart, "d_st_rowstart");
        f->st_rowstart_cap = rowstart;
    }
    if (!f->d_st_rowidx || rowidx > f->st_rowidx_cap) {
        m.release(f->d_st_rowidx);
        m.alloc(f->d_st_rowidx, rowidx, "d_st_rowidx");
        f->st_rowidx_cap = rowidx;
    }
    const int rc = m.check("pslfe_frame_set_from_orb_stereo");
    if (rc) {
        m.release(f->d_st_idx); m.release(f->d_st_sad); m.release(f->d_st_rowstart); m.release(f->d_st_rowidx);
        f->st_rowstart_cap = f->st_rowidx_cap = 0;
        std::fill(f->slot_stereo.begin(), f->slot_stereo.end(), 0);   // the taps of earlier stereo slots are gone with them
    }
    return rc;
}

void st_pyr(const PslOrbPyramid& O, StereoPyr* P) {
    memset(P, 0, sizeof(*P));
    P->img0 = O.img0; P->fstride0 = O.fstride0; P->pyr = O.pyr; P->pyr_fstride = O.pyr_fstride;
    for (int l = 0; l < O.nlevels; ++l) { P->w[l] = O.w[l]; P->h[l] = O.h[l]; P->pitch[l] = O.pitch[l]; P->off[l] = O.off[l]; }
}

}  // namespace

extern "C" {

int pslfe_frame_set_from_orb_stereo(pslfe_frame* f, int slot0, pslfe_orb* left, int left0, pslfe_orb* right, int right0, int nframes,
                                    const PslCamera* cam) {
    const char* who = "pslfe_frame_set_from_orb_stereo";
    PSL_REQUIRE(f && left && right && cam, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nframes >= 1, PSLFE_E_INVALID, "%s: %d pairs", who, nframes);
    PslOrbPyramid L, R;
    int rc = pslfe_orb_internal_pyramid(left, &L);
    if (!rc) rc = pslfe_orb_internal_pyramid(right, &R);
    if (rc) return rc;
    PSL_REQUIRE(L.ctx == f->ctx && R.ctx == f->ctx, PSLFE_E_INVALID, "%s: handles belong to different contexts", who);
    PSL_REQUIRE(L.w[0] == R.w[0] && L.h[0] == R.h[0], PSLFE_E_INVALID, "%s: left %dx%d, right %dx%d", who, L.w[0], L.h[0], R.w[0], R.h[0]);
    PSL_REQUIRE(L.nlevels == R.nlevels && memcmp(L.scale, R.scale, sizeof(float) * L.nlevels) == 0, PSLFE_E_INVALID,
                "%s: the extractors differ in levels or scale factors", who);
    PSL_REQUIRE(left0 >= 0 && left0 + nframes <= L.nframes && right0 >= 0 && right0 + nframes <= R.nframes, PSLFE_E_INVALID,
                "%s: left frames %d..%d of %d, right frames %d..%d of %d", who, left0, left0 + nframes - 1, L.nframes, right0,
                right0 + nframes - 1, R.nframes);
    PSL_REQUIRE(slot0 >= 0, PSLFE_E_INVALID, "%s: slot %d", who, slot0);
    PSL_REQUIRE(slot0 + nframes <= f->max_frames, PSLFE_E_CAPACITY, "%s: slots %d..%d, %d slots", who, slot0, slot0 + nframes - 1, f->max_frames);
    PSL_REQUIRE(L.cap <= f->cap && R.cap <= f->cap, PSLFE_E_CAPACITY, "%s: extractor capacity %d / %d > frame capacity %d", who, L.cap, R.cap,
                f->cap);
    const int rows = L.h[0];
    PSL_REQUIRE(rows <= PSL_ST_MAX_ROWS, PSLFE_E_INVALID, "%s: %d rows", who, rows);
    PSL_HIP(hipSetDevice(f->ctx->device));
    const size_t F = (size_t)f->max_frames, K = (size_t)f->cap;
    if ((rc = st_buffers(f, F * K, (size_t)nframes * (rows + 1), (size_t)nframes * R.cap))) return rc;

    StereoArgs A;
    memset(&A, 0, sizeof(A));
    A.kpsL = L.kps + (size_t)left0 * L.cap; A.descL = L.desc + (size_t)left0 * L.cap * 32; A.cntL = L.counts + left0;
    A.capL = L.cap; A.left0 = left0;
    A.kpsR = R.kps + (size_t)right0 * R.cap; A.descR = R.desc + (size_t)right0 * R.cap * 32; A.cntR = R.counts + right0;
    A.capR = R.cap; A.right0 = right0;
    st_pyr(L, &A.PL);
    st_pyr(R, &A.PR);
    for (int l = 0; l < L.nlevels; ++l) { A.scale[l] = L.scale[l]; A.inv_scale[l] = L.inv_scale[l]; }
    A.nlevels = L.nlevels; A.rows = rows;
    // a candidate's own row lies within 2*scale + 1 of the left row; two more rows cover the rounding of y +- r
    A.band = (int)ceilf(2.0f * L.scale[L.nlevels - 1]) + 3;
    const float mb = cam->bf / cam->fx;   // minZ = mb (convention: the reference reads mb before assigning it)
    A.maxD = cam->bf / mb;
    A.bf = cam->bf;
    A.rowstart = f->d_st_rowstart; A.rowidx = f->d_st_rowidx;
    A.uright = f->S.uright; A.depth = f->d_depth; A.tidx = f->d_st_idx; A.tsad = f->d_st_sad;
    A.slot0 = slot0; A.cap = f->cap;

    if ((rc = psl_frame_import(f, slot0, A.kpsL, A.descL, A.cntL, L.cap, nframes))) return rc;
    hipStream_t st = f->ctx->stream;
    {
        PSL_STAGE_BEGIN(f->ctx, "frame.stereo");
        k_stereo_rows<<<nframes, 1024, 0, st>>>(A);
        k_stereo_match<<<dim3((L.cap + 4 * PSL_ST_KPW - 1) / (4 * PSL_ST_KPW), nframes), 256, 0, st>>>(A);
        k_stereo_filter<<<nframes, 256, 0, st>>>(A);
        PSL_STAGE_END(f->ctx, "frame.stereo");
    }
    PSL_HIP(hipGetLastError());
    return psl_frame_finish_stereo(f, slot0, nframes, L.w[0], rows, cam);
}

int pslfe_frame_debug_stereo(pslfe_frame* f, int slot, int32_t* idx_right, int32_t* sad, int cap, int* n) {
    PSL_REQUIRE(f && n, PSLFE_E_INVALID, "pslfe_frame_debug_stereo: NULL argument");
    PSL_REQUIRE(slot >= 0 && slot < f->max_frames && f->slot_stereo[slot] && f->d_st_idx && f->d_st_sad, PSLFE_E_STATE, "pslfe_frame_debug_stereo: slot %d not set by a stereo call",
                slot);
    PSL_HIP(hipSetDevice(f->ctx->device));
    PSL_HIP(hipStreamSynchronize(f->ctx->stream));
    FrameMeta m;
    PSL_HIP(hipMemcpy(&m, f->S.meta + slot, sizeof(m), hipMemcpyDeviceToHost));
    *n = m.n;
    PSL_REQUIRE(m.n <= cap, PSLFE_E_CAPACITY, "pslfe_frame_debug_stereo: %d keypoints, capacity %d", m.n, cap);
    const size_t o = (size_t)slot * f->cap;
    if (idx_right && m.n > 0) PSL_HIP(hipMemcpy(idx_right, f->d_st_idx + o, (size_t)m.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sad && m.n > 0) PSL_HIP(hipMemcpy(sad, f->d_st_sad + o, (size_t)m.n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PSLFE_OK;
}

}  // extern "C"
