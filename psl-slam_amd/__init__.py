"""psl-slam_amd — MI355X-native feature front-end for PSL-SLAM (host-side Python mirror).

Thin ctypes layer over the C ABI in include/pslfe.h (libpslfe.so, HIP/gfx950).  The class and
method names follow the reference's C++ interfaces (include/ORBextractor.h:59,
add_inc/LineExtractor.h:167, include/ORBmatcher.h, add_inc/LSDmatcher.h) so that the parity tests
read like calls into the reference.  There is no CPU fallback: without the built library or
without a gfx950 GPU every entry point raises.

Import name: ``psl_slam_amd`` (root shim psl_slam_amd.py; the directory keeps the project's
hyphenated name).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpslfe.so")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                          ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                          ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                          ("lineLength", "<f4"), ("numOfPixels", "<i4")])
PROJQUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("min_level", "<i4"),
                            ("max_level", "<i4"), ("angle", "<f4"), ("blocks", "<i4")])
BOWQUERY_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("angle", "<f4")])
CAMERA_DTYPE = np.dtype([(k, "<f4") for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf")])
assert KEYPOINT_DTYPE.itemsize == 28 and KEYLINE_DTYPE.itemsize == 68 and PROJQUERY_DTYPE.itemsize == 32
# projection of 3-D points (include/pslfe.h: PslPose, PslLastPoint, PslMapPointGeom)
POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,))])
LASTPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("state", "<i4")])
MAPPOINT_DTYPE = np.dtype([(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")])
assert POSE_DTYPE.itemsize == 48 and LASTPOINT_DTYPE.itemsize == 16 and MAPPOINT_DTYPE.itemsize == 32
LASTPOINT_NONE, LASTPOINT_NO_OBS, LASTPOINT_OBS, LASTPOINT_OUTLIER = 0, 1, 2, 8
# pose optimisation (include/pslfe.h: PslPoseEdge, PslPoseInfo)
POSEEDGE_DTYPE = np.dtype([(k, "<f4") for k in ("u", "v", "ur", "inv_sigma2", "x", "y", "z")])
POSEINFO_DTYPE = np.dtype([("rounds", "<i4"), ("iterations", "<i4", (4,))])
assert POSEEDGE_DTYPE.itemsize == 28 and POSEINFO_DTYPE.itemsize == 20
# the LIL edge and the map LIL it is made from (include/pslfe.h: PslPoseLilEdge, PslMapLil)
POSELIL_DTYPE = np.dtype([("line1", "<f8", (6,)), ("line2", "<f8", (6,)), ("cross", "<f8", (3,)), ("obs1", "<f8", (3,)), ("obs2", "<f8", (3,)),
                          ("obs_ins", "<f8", (2,))])
MAPLIL_DTYPE = np.dtype([("w", "<f8", (15,)), ("bad", "u1"), ("pad", "u1", (7,))])
assert POSELIL_DTYPE.itemsize == 184 and MAPLIL_DTYPE.itemsize == 128
# Sim3 optimisation (include/pslfe.h: PslSim3, PslSim3D, PslSim3Pair, PslSim3Info)
SIM3_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("s", "<f4")])
SIM3D_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
SIM3PAIR_DTYPE = np.dtype([("u1", "<f4"), ("v1", "<f4"), ("inv_sigma2_1", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("inv_sigma2_2", "<f4"),
                           ("P1c", "<f4", (3,)), ("P2c", "<f4", (3,))])
SIM3INFO_DTYPE = np.dtype([("calls", "<i4"), ("iterations", "<i4", (2,)), ("exp_branches", "<i4")])
assert SIM3_DTYPE.itemsize == 52 and SIM3D_DTYPE.itemsize == 64 and SIM3PAIR_DTYPE.itemsize == 48 and SIM3INFO_DTYPE.itemsize == 16
# Sim3Solver (include/pslfe.h: PslSim3SolverResult)
SIM3SOLVERRESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("ninliers", "<i4"), ("best_inliers", "<i4"), ("S12", SIM3_DTYPE)])
assert SIM3SOLVERRESULT_DTYPE.itemsize == 68
# PnPsolver (include/pslfe.h: PslPnpRow, PslPnpResult)
PNPROW_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4"), ("sigma2", "<f4")])
PNPRESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("inliers", "<i4"), ("best_inliers", "<i4"), ("min_inliers", "<i4"),
                            ("Tcw", POSE_DTYPE), ("best_Tcw", POSE_DTYPE)])
assert PNPROW_DTYPE.itemsize == 24 and PNPRESULT_DTYPE.itemsize == 116
# Initializer (include/pslfe.h: PslInitResult)
INITRESULT_DTYPE = np.dtype([("status", "<i4"), ("nmatches", "<i4"), ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"), ("best_it_h", "<i4"),
                             ("best_it_f", "<i4"), ("inliers_h", "<i4"), ("inliers_f", "<i4"), ("H21", "<f4", (9,)), ("F21", "<f4", (9,)),
                             ("ngood", "<i4", (8,)), ("parallax", "<f4", (8,)), ("best_hypothesis", "<i4"), ("R21", "<f4", (9,)),
                             ("t21", "<f4", (3,)), ("ntriangulated", "<i4")])
assert INITRESULT_DTYPE.itemsize == 228
# local bundle adjustment (include/pslfe.h: PslBaEdge, PslBaKeyFrame, PslBaInfo)
BAEDGE_DTYPE = np.dtype([("point", "<i4"), ("kf", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4")])
BAKEYFRAME_DTYPE = np.dtype([("Tcw", POSE_DTYPE), ("fixed", "<i4")])
BAINFO_DTYPE = np.dtype({"names": ["status", "rounds", "iterations", "nerased", "chi2_start", "chi2_round1", "chi2_end"],
                         "formats": ["<i4", "<i4", ("<i4", (2,)), "<i4", "<f8", "<f8", "<f8"], "offsets": [0, 4, 8, 16, 24, 32, 40], "itemsize": 48})
BALILEDGE_DTYPE = np.dtype([("lil", "<i4"), ("kf", "<i4"), ("obs1", "<f8", (3,)), ("obs2", "<f8", (3,)), ("obs_ins", "<f8", (2,))])
assert BALILEDGE_DTYPE.itemsize == 72
assert BAEDGE_DTYPE.itemsize == 24 and BAKEYFRAME_DTYPE.itemsize == 52 and BAINFO_DTYPE.itemsize == 48
# global bundle adjustment (include/pslfe.h: PslGbaInfo)
GBAINFO_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("free_keyframes", "<i4"), ("included_points", "<i4"), ("chi2_start", "<f8"),
                          ("chi2_end", "<f8"), ("lambda", "<f8")])
assert GBAINFO_DTYPE.itemsize == 40
# essential graph (include/pslfe.h: PslEgKeyFrame, PslEgEdge, PslEgInfo)
EGKEYFRAME_DTYPE = np.dtype([("Scw", "<f8", (8,)), ("Snc", "<f8", (8,)), ("has_nc", "<i4"), ("fixed", "<i4")])
EGEDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("loop", "<i4")])
EGINFO_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("log_branches", "<i4"), ("nfree", "<i4"), ("chi2_start", "<f8"),
                         ("chi2_end", "<f8"), ("lambda", "<f8")])
assert EGKEYFRAME_DTYPE.itemsize == 136 and EGEDGE_DTYPE.itemsize == 12 and EGINFO_DTYPE.itemsize == 40


def pose(Tcw):
    """A 4x4 (or 3x4) Frame::mTcw -> one POSE_DTYPE record."""
    T = np.asarray(Tcw, np.float32)
    p = np.zeros((), POSE_DTYPE)
    p["R"], p["t"] = T[:3, :3].reshape(9), T[:3, 3]
    return p


class PslfeError(RuntimeError):
    pass


_lib = None


def build(force=False):
    """Compile libpslfe.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_pslfe_build", os.path.join(_HERE, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(force=force)


def lib():
    """The loaded C-ABI library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PslfeError(f"{LIB_PATH} is missing: run `python psl-slam_amd/build.py` (needs hipcc); "
                             "there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.pslfe_version.restype = C.c_char_p
        L.pslfe_last_error.restype = C.c_char_p
        L.pslfe_orb_scale_factor.restype = C.c_float
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise PslfeError(f"{what} failed with code {rc}: {lib().pslfe_last_error().decode()}")


def _ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


class Context:
    """One per GPU (pslfe_ctx)."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        _check(lib().pslfe_ctx_create(C.c_int(device), C.byref(self._h)), "pslfe_ctx_create")
        if stream is not None:
            self.set_stream(stream)

    def set_stream(self, hip_stream):
        _check(lib().pslfe_ctx_set_stream(self._h, C.c_void_p(hip_stream)), "pslfe_ctx_set_stream")

    def synchronize(self):
        _check(lib().pslfe_ctx_synchronize(self._h), "pslfe_ctx_synchronize")

    def profile(self, enable=True):
        _check(lib().pslfe_ctx_profile(self._h, C.c_int(1 if enable else 0)), "pslfe_ctx_profile")

    def profile_only(self, stage=None):
        _check(lib().pslfe_ctx_profile_only(self._h, None if not stage else stage.encode()), "pslfe_ctx_profile_only")

    def profile_reset(self):
        _check(lib().pslfe_ctx_profile_reset(self._h), "pslfe_ctx_profile_reset")

    def stage_time(self, stage):
        ms, n = C.c_double(), C.c_int()
        _check(lib().pslfe_ctx_stage_time(self._h, stage.encode(), C.byref(ms), C.byref(n)), "pslfe_ctx_stage_time")
        return ms.value, n.value

    def device_array(self, host_array):
        """Upload a numpy array into freshly allocated HBM; returns (device address, nbytes)."""
        a = np.ascontiguousarray(host_array)
        d = C.c_void_p()
        _check(lib().pslfe_device_alloc(self._h, C.c_size_t(a.nbytes), C.byref(d)), "pslfe_device_alloc")
        _check(lib().pslfe_device_upload(self._h, d, _ptr(a), C.c_size_t(a.nbytes)), "pslfe_device_upload")
        return d.value, a.nbytes

    def device_free(self, d_ptr):
        _check(lib().pslfe_device_free(self._h, C.c_void_p(d_ptr)), "pslfe_device_free")

    def close(self):
        if self._h:
            lib().pslfe_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class ORBextractor:
    """== ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-114)."""

    HARRIS_SCORE, FAST_SCORE = 0, 1

    def __init__(self, nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, ctx=None, max_batch=1):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        self.nlevels = nlevels
        self.max_batch = max_batch
        _check(lib().pslfe_orb_create(self.ctx._h, C.c_int(nfeatures), C.c_float(scaleFactor), C.c_int(nlevels),
                                      C.c_int(iniThFAST), C.c_int(minThFAST), C.c_int(max_batch), C.byref(self._h)),
               "pslfe_orb_create")

    # getters of include/ORBextractor.h:63-84
    def GetLevels(self):
        return lib().pslfe_orb_levels(self._h)

    def GetScaleFactor(self):
        return lib().pslfe_orb_scale_factor(self._h)

    def _factors(self):
        a = [np.zeros(self.nlevels, np.float32) for _ in range(4)]
        _check(lib().pslfe_orb_scale_factors(self._h, *[_ptr(x) for x in a]), "pslfe_orb_scale_factors")
        return a

    def GetScaleFactors(self):
        return self._factors()[0]

    def GetInverseScaleFactors(self):
        return self._factors()[1]

    def GetScaleSigmaSquares(self):
        return self._factors()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._factors()[3]

    def features_per_level(self):
        q = np.zeros(self.nlevels, np.int32)
        _check(lib().pslfe_orb_features_per_level(self._h, _ptr(q)), "pslfe_orb_features_per_level")
        return q

    def max_keypoints(self, w, h):
        n = lib().pslfe_orb_max_keypoints(self._h, C.c_int(w), C.c_int(h))
        if n < 0:
            _check(n, "pslfe_orb_max_keypoints")
        return n

    def __call__(self, image, mask=None):
        """operator()(image, mask, keypoints, descriptors): mask is ignored as in the reference."""
        if image is None or image.size == 0:
            return np.zeros(0, KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2, "CV_8UC1 image expected"
        h, w = image.shape
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        _check(lib().pslfe_orb_extract(self._h, _ptr(image), C.c_int(w), C.c_int(h), C.c_int(image.strides[0]),
                                       _ptr(kps), _ptr(desc), C.c_int(cap), C.byref(n)), "pslfe_orb_extract")
        return kps[:n.value].copy(), desc[:n.value].copy()

    def extract_batch(self, images):
        """images: (F, h, w) uint8 host array -> list of (keypoints, descriptors)."""
        assert images.dtype == np.uint8 and images.ndim == 3 and images.flags.c_contiguous
        F, h, w = images.shape
        cap = self.max_keypoints(w, h)
        kps = np.zeros((F, cap), KEYPOINT_DTYPE)
        desc = np.zeros((F, cap, 32), np.uint8)
        counts = np.zeros(F, np.int32)
        _check(lib().pslfe_orb_extract_batch(self._h, _ptr(images), C.c_int(F), C.c_int(w), C.c_int(h), C.c_int(w),
                                             C.c_size_t(w * h), _ptr(kps), _ptr(desc), C.c_int(cap), _ptr(counts)),
               "pslfe_orb_extract_batch")
        return [(kps[f, :counts[f]].copy(), desc[f, :counts[f]].copy()) for f in range(F)]

    def extract_batch_device(self, d_ptr, nframes, w, h, stride, frame_stride):
        """Asynchronous extraction of frames resident in HBM (d_ptr = device address as int)."""
        _check(lib().pslfe_orb_extract_batch_device(self._h, C.c_void_p(d_ptr), C.c_int(nframes), C.c_int(w), C.c_int(h),
                                                    C.c_int(stride), C.c_size_t(frame_stride)),
               "pslfe_orb_extract_batch_device")

    def results_device(self):
        k, d, c, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
        _check(lib().pslfe_orb_results_device(self._h, C.byref(k), C.byref(d), C.byref(c), C.byref(cap)),
               "pslfe_orb_results_device")
        return k.value, d.value, c.value, cap.value

    def fetch(self, frame, w, h):
        cap = self.max_keypoints(w, h)
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = C.c_int()
        _check(lib().pslfe_orb_fetch(self._h, C.c_int(frame), _ptr(kps), _ptr(desc), C.c_int(cap), C.byref(n)), "pslfe_orb_fetch")
        return kps[:n.value].copy(), desc[:n.value].copy()

    # stage taps (parity tests)
    def debug_level_image(self, frame, level, blurred=False):
        w, h = C.c_int(), C.c_int()
        _check(lib().pslfe_orb_debug_level_size(self._h, C.c_int(level), C.byref(w), C.byref(h)), "pslfe_orb_debug_level_size")
        out = np.zeros((h.value, w.value), np.uint8)
        _check(lib().pslfe_orb_debug_level_image(self._h, C.c_int(frame), C.c_int(level), C.c_int(1 if blurred else 0),
                                                 _ptr(out), C.c_int(w.value)), "pslfe_orb_debug_level_image")
        return out

    def _debug_xys(self, fn, frame, level):
        n = C.c_int()
        _check(fn(self._h, C.c_int(frame), C.c_int(level), None, C.c_int(0), C.byref(n)), "pslfe_orb_debug")
        out = np.zeros((max(n.value, 1), 3), np.int32)
        _check(fn(self._h, C.c_int(frame), C.c_int(level), _ptr(out), C.c_int(out.shape[0]), C.byref(n)), "pslfe_orb_debug")
        return out[:n.value]

    def debug_candidates(self, frame, level):
        return self._debug_xys(lib().pslfe_orb_debug_candidates, frame, level)

    def debug_level_keypoints(self, frame, level):
        return self._debug_xys(lib().pslfe_orb_debug_level_keypoints, frame, level)

    def debug_set_results(self, frame, kps, desc):
        """pslfe_orb_debug_set_results: hand-made keypoints / descriptors as the results of frame `frame` of the last batch (the
        pyramid stays as extracted); fetch() and every consumer of the handle then see them."""
        n = len(kps)
        k = np.zeros(max(n, 1), KEYPOINT_DTYPE)
        d = np.zeros((max(n, 1), 32), np.uint8)
        k[:n], d[:n] = kps, np.asarray(desc, np.uint8).reshape(n, 32)
        _check(lib().pslfe_orb_debug_set_results(self._h, C.c_int(frame), _ptr(k), _ptr(d), C.c_int(n)), "pslfe_orb_debug_set_results")

    def close(self):
        if self._h:
            lib().pslfe_orb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rgb_to_gray(rgb, is_rgb=True, ctx=None):
    """cvtColor(im, gray, CV_RGB2GRAY if mbRGB else CV_BGR2GRAY), src/Tracking.cc:219-232. rgb: (h, w, 3) u8."""
    ctx = ctx or default_context()
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    gray = np.zeros((h, w), np.uint8)
    _check(lib().pslfe_rgb_to_gray(ctx._h, _ptr(rgb), C.c_int(w), C.c_int(h), C.c_int(3 * w), C.c_int(1 if is_rgb else 0),
                                   _ptr(gray)), "pslfe_rgb_to_gray")
    return gray


def depth_to_float(depth, factor, ctx=None):
    """imDepth.convertTo(imDepth, CV_32F, mDepthMapFactor), src/Tracking.cc:234-235. depth: u16 array."""
    ctx = ctx or default_context()
    depth = np.ascontiguousarray(depth, np.uint16)
    out = np.zeros(depth.shape, np.float32)
    _check(lib().pslfe_depth_to_float(ctx._h, _ptr(depth), C.c_size_t(depth.size), C.c_float(factor), _ptr(out)),
           "pslfe_depth_to_float")
    return out


class FrameGrid:
    """Keypoints of up to `max_frames` frames on the 64x48 grid of include/Frame.h:45-46
    (== the part of ORB_SLAM2::Frame the matchers read: mvKeysUn, mDescriptors, mvuRight, mGrid)."""

    def __init__(self, max_keypoints, max_frames=1, ctx=None):
        self.ctx = ctx or default_context()
        self.cap, self.max_frames = max_keypoints, max_frames
        self._h = C.c_void_p()
        _check(lib().pslfe_frame_create(self.ctx._h, C.c_int(max_keypoints), C.c_int(max_frames), C.byref(self._h)),
               "pslfe_frame_create")
        self.n = [0] * max_frames

    def set(self, slot, kps, desc, bounds, uright=None):
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
        _check(lib().pslfe_frame_set(self._h, C.c_int(slot), _ptr(kps), _ptr(desc), _ptr(ur), C.c_int(len(kps)),
                                     *[C.c_float(b) for b in bounds]), "pslfe_frame_set")
        self.n[slot] = len(kps)

    def set_from_orb(self, orb, bounds):
        _check(lib().pslfe_frame_set_from_orb(self._h, orb._h, *[C.c_float(b) for b in bounds]), "pslfe_frame_set_from_orb")

    def image_bounds(self, cam, cols, rows):
        """Frame::ComputeImageBounds src/Frame.cc:1135-1168 -> (mnMinX, mnMinY, mnMaxX, mnMaxY)."""
        b = np.zeros(4, np.float32)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_image_bounds(self._h, _ptr(cam), C.c_int(cols), C.c_int(rows), _ptr(b)), "pslfe_image_bounds")
        return b

    def set_rgbd(self, slot, kps, desc, depth, cam):
        """UndistortKeyPoints + ComputeStereoFromRGBD + AssignFeaturesToGrid (src/Frame.cc:105-171) for one frame.
        depth: CV_32F image in metres."""
        kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
        desc = np.ascontiguousarray(desc, np.uint8)
        depth = np.ascontiguousarray(depth, np.float32)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_frame_set_rgbd(self._h, C.c_int(slot), _ptr(kps), _ptr(desc), C.c_int(len(kps)), _ptr(depth),
                                          C.c_int(depth.shape[1]), C.c_int(depth.shape[0]), C.c_int(depth.shape[1]), _ptr(cam)),
               "pslfe_frame_set_rgbd")
        self.n[slot] = len(kps)

    def set_from_orb_rgbd(self, orb, d_depth, width, height, cam):
        """Batched, HBM to HBM: d_depth is a device pointer to [nframes][height][width] float."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_frame_set_from_orb_rgbd(self._h, orb._h, C.c_void_p(int(d_depth)), C.c_int(width), C.c_int(height),
                                                   _ptr(cam)), "pslfe_frame_set_from_orb_rgbd")

    def set_from_orb_stereo(self, slot0, left, left0, right, right0, nframes, cam):
        """The stereo Frame constructor (src/Frame.cc:75-131: ComputeStereoMatches, UndistortKeyPoints, AssignFeaturesToGrid) for
        nframes rectified pairs, HBM to HBM: frame left0+p of `left`'s last batch and frame right0+p of `right`'s -> slot slot0+p.
        `left` and `right` may be the same extractor.  Asynchronous."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_frame_set_from_orb_stereo(self._h, C.c_int(slot0), left._h, C.c_int(left0), right._h, C.c_int(right0),
                                                     C.c_int(nframes), _ptr(cam)), "pslfe_frame_set_from_orb_stereo")

    def set_from_orb_mono(self, slot0, orb, first, nframes, cam):
        """The monocular Frame constructor (src/Frame.cc:213-267: UndistortKeyPoints, mvuRight = mvDepth = -1, ComputeImageBounds,
        AssignFeaturesToGrid) for frames first..first+nframes-1 of `orb`'s last batch -> slots slot0.., HBM to HBM.  Asynchronous."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_frame_set_from_orb_mono(self._h, C.c_int(slot0), orb._h, C.c_int(first), C.c_int(nframes), _ptr(cam)),
               "pslfe_frame_set_from_orb_mono")

    def debug_stereo(self, slot):
        """Taps of a stereo slot: (right index of the descriptor stage or -1, SAD minimum of an accepted keypoint or -1)."""
        idx = np.zeros(self.cap, np.int32)
        sad = np.zeros(self.cap, np.int32)
        n = C.c_int()
        _check(lib().pslfe_frame_debug_stereo(self._h, C.c_int(slot), _ptr(idx), _ptr(sad), C.c_int(self.cap), C.byref(n)),
               "pslfe_frame_debug_stereo")
        return idx[:n.value], sad[:n.value]

    def fetch(self, slot):
        """(mvKeysUn, mvDepth, mvuRight) of a slot."""
        kps = np.zeros(self.cap, KEYPOINT_DTYPE)
        dep = np.zeros(self.cap, np.float32)
        ur = np.zeros(self.cap, np.float32)
        n = C.c_int()
        _check(lib().pslfe_frame_fetch(self._h, C.c_int(slot), _ptr(kps), _ptr(dep), _ptr(ur), C.c_int(self.cap), C.byref(n)),
               "pslfe_frame_fetch")
        self.n[slot] = n.value
        return kps[:n.value], dep[:n.value], ur[:n.value]

    def project_last(self, slot, Tlw, Tcw, points, mpdesc, cam, scale_factors, th, th_depth, mono, vo, bounds):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) src/ORBmatcher.cc:1338-1390 up to the window search, slot `slot` as
        the last frame (vo: with UpdateLastFrame's visual-odometry points).  points: LASTPOINT_DTYPE[N] or None, mpdesc: [N, 32]
        or None.  -> (queries PROJQUERY_DTYPE, qdesc [nq, 32], owner [nq])."""
        Tl, Tc = np.ascontiguousarray(Tlw, POSE_DTYPE).reshape(1), np.ascontiguousarray(Tcw, POSE_DTYPE).reshape(1)
        pts = None if points is None else np.ascontiguousarray(points, LASTPOINT_DTYPE)
        md = None if mpdesc is None else np.ascontiguousarray(mpdesc, np.uint8)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        sc = np.ascontiguousarray(scale_factors, np.float32)
        q = np.zeros(self.cap, PROJQUERY_DTYPE)
        qd = np.zeros((self.cap, 32), np.uint8)
        ow = np.zeros(self.cap, np.int32)
        nq = C.c_int()
        _check(lib().pslfe_orb_project_last(self._h, C.c_int(slot), _ptr(Tl), _ptr(Tc), _ptr(pts), _ptr(md), _ptr(cam), _ptr(sc),
                                            C.c_int(len(sc)), C.c_float(th), C.c_float(th_depth), C.c_int(1 if mono else 0),
                                            C.c_int(1 if vo else 0), *[C.c_float(b) for b in bounds], _ptr(q), _ptr(qd), _ptr(ow),
                                            C.byref(nq), C.c_int(self.cap)), "pslfe_orb_project_last")
        return q[:nq.value], qd[:nq.value], ow[:nq.value]

    def project_last_device(self, slot0, npairs, d_Tlw, d_Tcw, d_points, d_mpdesc, cam, scale_factors, th, th_depth, mono, vo, bounds,
                            d_queries, d_qdesc, d_owner, d_nq, qstride):
        """Batched, HBM-resident project_last: all d_* are device addresses (ints; d_points / d_mpdesc / d_owner may be 0)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        sc = np.ascontiguousarray(scale_factors, np.float32)
        _check(lib().pslfe_orb_project_last_device(
            self._h, C.c_int(slot0), C.c_int(npairs), C.c_void_p(d_Tlw), C.c_void_p(d_Tcw), C.c_void_p(d_points or None),
            C.c_void_p(d_mpdesc or None), _ptr(cam), _ptr(sc), C.c_int(len(sc)), C.c_float(th), C.c_float(th_depth),
            C.c_int(1 if mono else 0), C.c_int(1 if vo else 0), *[C.c_float(b) for b in bounds], C.c_void_p(d_queries),
            C.c_void_p(d_qdesc), C.c_void_p(d_owner or None), C.c_void_p(d_nq), C.c_int(qstride)), "pslfe_orb_project_last_device")

    def debug_grid(self, slot):
        start = np.zeros(64 * 48 + 1, np.int32)
        idx = np.zeros(self.cap, np.int32)
        n = C.c_int()
        _check(lib().pslfe_frame_debug_grid(self._h, C.c_int(slot), _ptr(start), _ptr(idx), C.c_int(self.cap), C.byref(n)),
               "pslfe_frame_debug_grid")
        return start, idx[:n.value]

    def close(self):
        if self._h:
            lib().pslfe_frame_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ORBmatcher:
    """== ORB_SLAM2::ORBmatcher (include/ORBmatcher.h:36-104), the per-frame projection searches."""

    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, checkOri=True):
        self.mfNNratio, self.mbCheckOrientation = nnratio, checkOri

    def _run(self, fn, frame, slot, queries, qdesc, taken, extra):
        queries = np.ascontiguousarray(queries, PROJQUERY_DTYPE)
        qdesc = np.ascontiguousarray(qdesc, np.uint8)
        nq = len(queries)
        match = np.full(max(nq, 1), -1, np.int32)
        assigned = np.full(max(frame.n[slot], 1), -1, np.int32)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        nm = C.c_int()
        _check(fn(frame._h, C.c_int(slot), _ptr(queries), _ptr(qdesc), C.c_int(nq), _ptr(tk), extra, _ptr(match),
                  _ptr(assigned), C.byref(nm)), "pslfe_orb_search_by_projection")
        return nm.value, match[:nq], assigned[:frame.n[slot]]

    def SearchByProjectionLast(self, frame, slot, queries, qdesc, taken=None):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) src/ORBmatcher.cc:1328."""
        return self._run(lib().pslfe_orb_search_by_projection_last, frame, slot, queries, qdesc, taken,
                         C.c_int(1 if self.mbCheckOrientation else 0))

    def SearchByProjectionKF(self, frame, slot, queries, qdesc, taken=None, ORBdist=100):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) src/ORBmatcher.cc:1472 (relocalisation)."""
        queries = np.ascontiguousarray(queries, PROJQUERY_DTYPE)
        qdesc = np.ascontiguousarray(qdesc, np.uint8)
        nq = len(queries)
        match = np.full(max(nq, 1), -1, np.int32)
        assigned = np.full(max(frame.n[slot], 1), -1, np.int32)
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        nm = C.c_int()
        _check(lib().pslfe_orb_search_by_projection_kf(frame._h, C.c_int(slot), _ptr(queries), _ptr(qdesc), C.c_int(nq), _ptr(tk),
                                                       C.c_int(ORBdist), C.c_int(1 if self.mbCheckOrientation else 0), _ptr(match),
                                                       _ptr(assigned), C.byref(nm)), "pslfe_orb_search_by_projection_kf")
        return nm.value, match[:nq], assigned[:frame.n[slot]]

    def SearchByBoW(self, frame, slot, fidx, runs, qangle, qdesc):
        """SearchByBoW(pKF, F, vpMapPointMatches) src/ORBmatcher.cc:159 on host-provided FeatureVectors: fidx = F.mFeatVec
        flattened in node order; runs[i] = (start, len) of query i's node in fidx; qangle / qdesc per query."""
        fidx = np.ascontiguousarray(fidx, np.int32)
        q = np.zeros(len(runs), BOWQUERY_DTYPE)
        if len(runs):
            r = np.asarray(runs, np.int32).reshape(-1, 2)
            q["start"], q["len"], q["angle"] = r[:, 0], r[:, 1], np.asarray(qangle, np.float32)
        qdesc = np.ascontiguousarray(qdesc, np.uint8)
        nq = len(q)
        match = np.full(max(nq, 1), -1, np.int32)
        assigned = np.full(max(frame.n[slot], 1), -1, np.int32)
        nm = C.c_int()
        _check(lib().pslfe_orb_search_by_bow(frame._h, C.c_int(slot), _ptr(fidx), C.c_int(len(fidx)), _ptr(q), _ptr(qdesc), C.c_int(nq),
                                             C.c_float(self.mfNNratio), C.c_int(1 if self.mbCheckOrientation else 0), _ptr(match),
                                             _ptr(assigned), C.byref(nm)), "pslfe_orb_search_by_bow")
        return nm.value, match[:nq], assigned[:frame.n[slot]]

    def SearchByProjectionMap(self, frame, slot, queries, qdesc, taken=None):
        """SearchByProjection(F, vpMapPoints, th) src/ORBmatcher.cc:45."""
        return self._run(lib().pslfe_orb_search_by_projection_map, frame, slot, queries, qdesc, taken,
                         C.c_float(self.mfNNratio))

    def SearchForInitialization(self, f1, slot1, f2, slot2, prev_matched, window=100):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize) src/ORBmatcher.cc:405: F1 = slot1 of f1, F2 =
        slot2 of f2.  prev_matched: float32 [n1, 2] (n1 = F1's keypoint count), updated in place.  -> (nmatches, matches12)."""
        if not (isinstance(prev_matched, np.ndarray) and prev_matched.dtype == np.float32 and prev_matched.flags.c_contiguous):
            raise TypeError("prev_matched must be a C-contiguous float32 array [n1, 2] (it is updated in place)")
        n1 = prev_matched.size // 2
        m12 = np.full(max(n1, 1), -1, np.int32)
        nm = C.c_int()
        _check(lib().pslfe_orb_search_for_initialization(f1._h, C.c_int(slot1), f2._h, C.c_int(slot2), _ptr(prev_matched), C.c_int(window),
                                                         C.c_float(self.mfNNratio), C.c_int(1 if self.mbCheckOrientation else 0),
                                                         _ptr(m12), C.byref(nm)), "pslfe_orb_search_for_initialization")
        return nm.value, m12[:n1]


def hamming_knn2(q, t, ctx=None):
    """cv::BFMatcher(NORM_HAMMING).knnMatch(q, t, 2) -> (idx[nq,2], dist[nq,2])."""
    ctx = ctx or default_context()
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    idx = np.zeros((max(len(q), 1), 2), np.int32)
    dist = np.zeros((max(len(q), 1), 2), np.int32)
    _check(lib().pslfe_hamming_knn2(ctx._h, _ptr(q), C.c_int(len(q)), _ptr(t), C.c_int(len(t)), _ptr(idx), _ptr(dist)),
           "pslfe_hamming_knn2")
    return idx[:len(q)], dist[:len(q)]


class LSDmatcher:
    """== ORB_SLAM2::LSDmatcher (add_inc/LSDmatcher.h:18-75), descriptor part."""

    TH_HIGH, TH_LOW = 80, 50

    def __init__(self, nnratio=0.95, checkOri=True, ctx=None):
        self.mfNNratio, self.mbCheckOrientation = nnratio, checkOri
        self.ctx = ctx or default_context()

    def matchNNR(self, desc1, desc2, nnr):
        """add_src/LSDmatcher.cpp:354-376 -> (matches, matches_12)."""
        d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 32)
        m12 = np.full(max(len(d1), 1), -1, np.int32)
        nm = C.c_int()
        _check(lib().pslfe_line_match_nnr(self.ctx._h, _ptr(d1), C.c_int(len(d1)), _ptr(d2), C.c_int(len(d2)),
                                          C.c_float(nnr), _ptr(m12), C.byref(nm)), "pslfe_line_match_nnr")
        return nm.value, m12[:len(d1)]

    match = matchNNR  # LSDmatcher::match's live branch is matchNNR (:378-413)


class _DevArray:
    """Zero-copy view of library-owned HBM for frameworks that read __cuda_array_interface__
    (torch.as_tensor(view, device='cuda') aliases the memory; nothing is copied)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"data": (int(ptr), False), "shape": tuple(shape), "typestr": typestr,
                                         "version": 2, "strides": None}


def orb_results_as_arrays(orb, nframes):
    """(kps [F,cap,7] f32-view, desc [F,cap,32] u8, counts [F] i32) device views of the last batch."""
    k, d, c, cap = orb.results_device()
    return (_DevArray(k, (nframes, cap, 7), "<f4"), _DevArray(d, (nframes, cap, 32), "|u1"),
            _DevArray(c, (nframes,), "<i4"), cap)


def search_by_projection_last_device(frame, slot0, npairs, d_queries, d_qdesc, d_nq, qstride, check_orientation,
                                     d_match, d_nmatches):
    """Batched HBM-resident SearchByProjection(cur,last); all d_* are device addresses (ints)."""
    _check(lib().pslfe_orb_search_by_projection_last_device(
        frame._h, C.c_int(slot0), C.c_int(npairs), C.c_void_p(d_queries), C.c_void_p(d_qdesc), C.c_void_p(d_nq),
        C.c_int(qstride), C.c_int(1 if check_orientation else 0), C.c_void_p(d_match), C.c_void_p(d_nmatches)),
        "pslfe_orb_search_by_projection_last_device")


def search_for_initialization_device(f1, slot1, f2, slot2, d_prev, prev_stride, d_matches12, d_nmatches, window=100, nnratio=0.9,
                                     check_orientation=True):
    """Batched HBM-resident SearchForInitialization: pair p = (f1 slot slot1[p], f2 slot slot2[p]) with prev rows
    d_prev + p*prev_stride*2 (float32, in/out), matches d_matches12 + p*prev_stride and d_nmatches[p]; d_* are device addresses."""
    s1 = np.ascontiguousarray(slot1, np.int32).reshape(-1)
    s2 = np.ascontiguousarray(slot2, np.int32).reshape(-1)
    if len(s1) != len(s2):
        raise ValueError("slot1 and slot2 differ in length")
    _check(lib().pslfe_orb_search_for_initialization_device(
        f1._h, _ptr(s1), f2._h, _ptr(s2), C.c_int(len(s1)), C.c_void_p(d_prev), C.c_int(prev_stride), C.c_int(window),
        C.c_float(nnratio), C.c_int(1 if check_orientation else 0), C.c_void_p(d_matches12), C.c_void_p(d_nmatches)),
        "pslfe_orb_search_for_initialization_device")


def project_frustum(Tcw, mp, mpdesc, cam, scale_factors, log_scale_factor, view_cos_limit, th, bounds, ctx=None):
    """Frame::isInFrustum src/Frame.cc:927-983 for every map point (MAPPOINT_DTYPE[M], descriptors [M, 32]) and the query rows of
    SearchByProjection(F, vpMapPoints, th) src/ORBmatcher.cc:45-70 for those in view.
    -> (queries, qdesc, owner, inview [M] u8, level [M] i32, viewcos [M] f32)."""
    ctx = ctx or default_context()
    T = np.ascontiguousarray(Tcw, POSE_DTYPE).reshape(1)
    mp = np.ascontiguousarray(mp, MAPPOINT_DTYPE)
    md = np.ascontiguousarray(mpdesc, np.uint8).reshape(-1, 32)
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    sc = np.ascontiguousarray(scale_factors, np.float32)
    M = len(mp)
    q = np.zeros(max(M, 1), PROJQUERY_DTYPE)
    qd = np.zeros((max(M, 1), 32), np.uint8)
    ow = np.zeros(max(M, 1), np.int32)
    inview, level, vc = np.zeros(max(M, 1), np.uint8), np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1), np.float32)
    nq = C.c_int()
    _check(lib().pslfe_orb_project_frustum(ctx._h, _ptr(T), _ptr(mp), _ptr(md), C.c_int(M), _ptr(cam), _ptr(sc), C.c_int(len(sc)),
                                           C.c_float(log_scale_factor), C.c_float(view_cos_limit), C.c_float(th),
                                           *[C.c_float(b) for b in bounds], _ptr(q), _ptr(qd), _ptr(ow), C.byref(nq), C.c_int(M),
                                           _ptr(inview), _ptr(level), _ptr(vc)), "pslfe_orb_project_frustum")
    n = nq.value
    return q[:n], qd[:n], ow[:n], inview[:M], level[:M], vc[:M]


def project_frustum_device(nframes, d_Tcw, d_mp, d_mpdesc, d_nmp, mpstride, cam, scale_factors, log_scale_factor, view_cos_limit, th,
                           bounds, d_queries, d_qdesc, d_owner, d_nq, qstride, d_inview=0, d_level=0, d_viewcos=0, ctx=None):
    """Batched, HBM-resident project_frustum; all d_* are device addresses (ints; d_owner / d_inview / d_level / d_viewcos may be 0).
    d_nq[f] > qstride: more map points in view than rows (the first qstride are written)."""
    ctx = ctx or default_context()
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    sc = np.ascontiguousarray(scale_factors, np.float32)
    _check(lib().pslfe_orb_project_frustum_device(
        ctx._h, C.c_int(nframes), C.c_void_p(d_Tcw), C.c_void_p(d_mp), C.c_void_p(d_mpdesc), C.c_void_p(d_nmp), C.c_int(mpstride),
        _ptr(cam), _ptr(sc), C.c_int(len(sc)), C.c_float(log_scale_factor), C.c_float(view_cos_limit), C.c_float(th),
        *[C.c_float(b) for b in bounds], C.c_void_p(d_queries), C.c_void_p(d_qdesc), C.c_void_p(d_owner or None), C.c_void_p(d_nq),
        C.c_int(qstride), C.c_void_p(d_inview or None), C.c_void_p(d_level or None), C.c_void_p(d_viewcos or None)),
        "pslfe_orb_project_frustum_device")


def search_by_projection_map_device(frame, slot0, npairs, d_queries, d_qdesc, d_nq, qstride, d_taken, nnratio, d_match, d_nmatches):
    """Batched HBM-resident SearchByProjection(F, vpMapPoints); all d_* are device addresses (ints; d_taken may be 0)."""
    _check(lib().pslfe_orb_search_by_projection_map_device(
        frame._h, C.c_int(slot0), C.c_int(npairs), C.c_void_p(d_queries), C.c_void_p(d_qdesc), C.c_void_p(d_nq), C.c_int(qstride),
        C.c_void_p(d_taken or None), C.c_float(nnratio), C.c_void_p(d_match), C.c_void_p(d_nmatches)),
        "pslfe_orb_search_by_projection_map_device")


class BundleAdjuster:
    """The HBM workspaces of the local bundle adjustment (pslfe_ba): up to max_problems problems per launch of up to max_keyframes
    keyframes (free and fixed), max_points points and max_edges edges each; with max_lils / max_lil_edges (both given) also of that
    many VertexLIL rows and LIL edges (pslfe_ba_create_lil), without them the LIL caps are 0."""

    def __init__(self, max_problems, max_keyframes, max_points, max_edges, max_lils=None, max_lil_edges=None, ctx=None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        if max_lils is None and max_lil_edges is None:
            _check(lib().pslfe_ba_create(self.ctx._h, C.c_int(max_problems), C.c_int(max_keyframes), C.c_int(max_points), C.c_int(max_edges),
                                         C.byref(self._h)), "pslfe_ba_create")
        else:
            _check(lib().pslfe_ba_create_lil(self.ctx._h, C.c_int(max_problems), C.c_int(max_keyframes), C.c_int(max_points), C.c_int(max_edges),
                                             C.c_int(max_lils or 0), C.c_int(max_lil_edges or 0), C.byref(self._h)), "pslfe_ba_create_lil")

    def close(self):
        if self._h:
            lib().pslfe_ba_destroy.restype = None
            lib().pslfe_ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GlobalBundleAdjuster:
    """The HBM workspace of the global bundle adjustment (pslfe_gba): one problem of up to max_keyframes keyframes (at most 4096),
    max_points points and max_edges edges, spread over the whole device."""

    def __init__(self, max_keyframes, max_points, max_edges, ctx=None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        _check(lib().pslfe_gba_create(self.ctx._h, C.c_int(max_keyframes), C.c_int(max_points), C.c_int(max_edges), C.byref(self._h)),
               "pslfe_gba_create")

    def close(self):
        if self._h:
            lib().pslfe_gba_destroy.restype = None
            lib().pslfe_gba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EssentialGraph:
    """The HBM workspaces of the essential-graph optimisation (pslfe_eg): up to max_graphs graphs per launch of up to max_keyframes
    keyframes, max_edges edges, max_points map points and max_envelope doubles of envelope each (include/pslfe.h, pslfe_eg_create)."""

    def __init__(self, max_graphs, max_keyframes, max_edges, max_points, max_envelope, ctx=None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        _check(lib().pslfe_eg_create(self.ctx._h, C.c_int(max_graphs), C.c_int(max_keyframes), C.c_int(max_edges), C.c_int(max_points),
                                     C.c_int64(max_envelope), C.byref(self._h)), "pslfe_eg_create")

    def close(self):
        if self._h:
            lib().pslfe_eg_destroy.restype = None
            lib().pslfe_eg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Optimizer:
    """Optimizer::PoseOptimization src/Optimizer.cc:239-1023: the point edges (EdgeSE3ProjectXYZOnlyPose and
    EdgeStereoSE3ProjectXYZOnlyPose) and the LIL edges (EdgeLILSE3ProjectXYZ, :619-694, :973-1008; the `lil` argument and the *Lil*
    methods); Optimizer::LocalBundleAdjustment :1025-1966, its point edges, and LocalBundleAdjustmentAndInseclines :1968-2534 with the
    VertexLIL vertices.  Parity with g2o itself is unpinned."""

    @staticmethod
    def EssentialGraphEdges(parent, loop_edges, covisibles, loop_connections, loop_kf, cur_kf, min_feat=100):
        """The edge rows of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2607-2738) from what the reference reads off the pointer
        graph, as arrays over the keyframe rows (ascending mnId, bad keyframes left out, so comparing rows compares mnIds):
        parent[i] = the row of GetParent() or -1; loop_edges[i] = the rows of GetLoopEdges() in the set's order; covisibles[i] = the
        rows of GetCovisiblesByWeight(min_feat) in its order (bad ones left out); loop_connections = [(row i, [(row j, GetWeight(j)),
        ...]), ...] in the order the map and its sets iterate; loop_kf / cur_kf = the rows of pLoopKF / pCurKF.
        -> EGEDGE_DTYPE rows in the order the reference creates the edges: the LoopConnections pairs with weight >= min_feat or
        (cur_kf, loop_kf) itself, flagged loop (they fill sInsertedEdges); then per row i its spanning-tree edge (i, parent), its loop
        edges (i, l) with l < i, and its covisibility edges (i, n) with n < i that are neither the parent, a child, a loop edge
        nor in sInsertedEdges."""
        out, inserted = [], set()
        for i, conns in loop_connections:
            for j, w in conns:
                if (i != cur_kf or j != loop_kf) and w < min_feat:
                    continue
                out.append((i, j, 1))
                inserted.add((min(i, j), max(i, j)))
        for i in range(len(parent)):
            p = int(parent[i])
            if p >= 0:
                out.append((i, p, 0))
            le = [int(l) for l in loop_edges[i]]
            for l in le:
                if l < i:
                    out.append((i, l, 0))
            for n in covisibles[i]:
                n = int(n)
                if n >= 0 and n != p and int(parent[n]) != i and n not in le and n < i:
                    if (min(i, n), max(i, n)) in inserted:
                        continue
                    out.append((i, n, 0))
        ed = np.zeros(len(out), EGEDGE_DTYPE)
        for e, (i, j, loop) in enumerate(out):
            ed["i"][e], ed["j"][e], ed["loop"][e] = i, j, loop
        return ed

    @staticmethod
    def OptimizeEssentialGraph(eg, kfs, edges, mps, mp_ref, fix_scale):
        """Optimizer::OptimizeEssentialGraph src/Optimizer.cc:2536-2799 (the call of LoopClosing::CorrectLoop), one graph, host arrays:
        kfs EGKEYFRAME_DTYPE[nkf] (rows in ascending mnId: vScw, the NonCorrectedSim3 entry and its flag, fixed for pLoopKF), edges
        EGEDGE_DTYPE[ne] (EssentialGraphEdges builds them), mps MAPPOINT_DTYPE[nmp] with mp_ref int32[nmp] = the row nIDr of :2775-2784
        or -1 for a point that is copied.  -> (poses POSE_DTYPE[nkf] = Tiw of :2762, S float64 [nkf][8] = the optimised Sim3s,
        mps_out = what SetWorldPos gets, info EGINFO_DTYPE record).  A refused graph raises PslfeError."""
        k = np.ascontiguousarray(kfs, EGKEYFRAME_DTYPE).reshape(-1)
        e = np.ascontiguousarray(edges, EGEDGE_DTYPE).reshape(-1)
        m = np.ascontiguousarray(mps, MAPPOINT_DTYPE).reshape(-1)
        r = np.ascontiguousarray(mp_ref, np.int32).reshape(-1)
        if len(r) != len(m):
            raise PslfeError("OptimizeEssentialGraph: mp_ref needs one entry per map point")
        po, So, mo = np.zeros(max(len(k), 1), POSE_DTYPE), np.zeros((max(len(k), 1), 8), np.float64), np.zeros(max(len(m), 1), MAPPOINT_DTYPE)
        info = np.zeros(1, EGINFO_DTYPE)
        p = lambda a, n: _ptr(a) if n else None
        _check(lib().pslfe_eg_optimize(eg._h, p(k, len(k)), C.c_int(len(k)), p(e, len(e)), C.c_int(len(e)), p(m, len(m)), p(r, len(m)),
                                       C.c_int(len(m)), C.c_int(1 if fix_scale else 0), p(po, len(k)), p(So, len(k)), p(mo, len(m)), _ptr(info)),
               "pslfe_eg_optimize")
        return po[:len(k)], So[:len(k)], mo[:len(m)], info[0]

    @staticmethod
    def OptimizeEssentialGraphDevice(eg, K, d_kf, d_kf_off, d_edges, d_edge_off, d_mp, d_mp_ref, d_mp_off, fix_scale, d_pose_out, d_S_out,
                                     d_mp_out, d_info):
        """K independent graphs in one launch, HBM to HBM, asynchronous; all d_* are device addresses (ints).  The offset arrays have
        K + 1 ascending int32 entries; d_mp_out may be d_mp and is what update_normal_and_depth_device takes; d_info EGINFO_DTYPE [K]
        with the status of each graph (-4 capacity, -1 invalid: d_S_out = its Scw, d_mp_out = its d_mp, no pose row written)."""
        _check(lib().pslfe_eg_optimize_device(
            eg._h, C.c_int(K), C.c_void_p(d_kf or None), C.c_void_p(d_kf_off or None), C.c_void_p(d_edges or None), C.c_void_p(d_edge_off or None),
            C.c_void_p(d_mp or None), C.c_void_p(d_mp_ref or None), C.c_void_p(d_mp_off or None), C.c_int(1 if fix_scale else 0),
            C.c_void_p(d_pose_out or None), C.c_void_p(d_S_out or None), C.c_void_p(d_mp_out or None), C.c_void_p(d_info or None)),
            "pslfe_eg_optimize_device")

    @staticmethod
    def BundleAdjustment(gba, kfs, mps, edges, cam, iterations=5, robust=True):
        """Optimizer::BundleAdjustment src/Optimizer.cc:49-237, host arrays: kfs BAKEYFRAME_DTYPE[nkf] (the keyframes that are not bad;
        fixed = mnId == 0), mps MAPPOINT_DTYPE[nmp], edges BAEDGE_DTYPE[ne] in the order the reference creates them; robust sets Huber
        with (float)sqrt(5.99) / (float)sqrt(7.815).  -> (kfs_out: EVERY keyframe as toCvMat of its SE3Quat, the fixed one too;
        mps_out: a point with an edge as (float) of its estimate; not_included u8 [nmp] = vbNotIncludedMP; info GBAINFO_DTYPE record).
        Whether the rows go to SetPose / SetWorldPos or to mTcwGBA / mPosGBA is the caller's matter.  A refused problem (capacity,
        an edge outside it, a duplicate pair) raises PslfeError."""
        k = np.ascontiguousarray(kfs, BAKEYFRAME_DTYPE).reshape(-1)
        m = np.ascontiguousarray(mps, MAPPOINT_DTYPE).reshape(-1)
        e = np.ascontiguousarray(edges, BAEDGE_DTYPE).reshape(-1)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        ko, mo, ni = np.zeros(max(len(k), 1), BAKEYFRAME_DTYPE), np.zeros(max(len(m), 1), MAPPOINT_DTYPE), np.zeros(max(len(m), 1), np.uint8)
        info = np.zeros(1, GBAINFO_DTYPE)
        p = lambda a, n: _ptr(a) if n else None
        _check(lib().pslfe_gba_optimize(gba._h, p(k, len(k)), C.c_int(len(k)), p(m, len(m)), C.c_int(len(m)), p(e, len(e)), C.c_int(len(e)), _ptr(cam),
                                        C.c_int(iterations), C.c_int(1 if robust else 0), p(ko, len(k)), p(mo, len(m)), p(ni, len(m)), _ptr(info)),
               "pslfe_gba_optimize")
        return ko[:len(k)], mo[:len(m)], ni[:len(m)], info[0]

    @staticmethod
    def BundleAdjustmentDevice(gba, d_kf, nkf, d_mp, nmp, d_edges, nedges, cam, iterations, robust, d_kf_out, d_mp_out, d_not_included):
        """The same on rows in HBM (device addresses as ints); d_kf_out may be d_kf and d_mp_out may be d_mp, which is what
        update_normal_and_depth_device takes next.  Returns the GBAINFO_DTYPE record when the outputs are written; a refused problem
        does not raise: its status is in the record, its outputs equal its inputs and d_not_included is 0."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        info = np.zeros(1, GBAINFO_DTYPE)
        rc = lib().pslfe_gba_optimize_device(
            gba._h, C.c_void_p(d_kf or None), C.c_int(nkf), C.c_void_p(d_mp or None), C.c_int(nmp), C.c_void_p(d_edges or None), C.c_int(nedges),
            _ptr(cam), C.c_int(iterations), C.c_int(1 if robust else 0), C.c_void_p(d_kf_out or None), C.c_void_p(d_mp_out or None),
            C.c_void_p(d_not_included or None), _ptr(info))
        if rc != 0 and rc != int(info[0]["status"]):
            _check(rc, "pslfe_gba_optimize_device")
        return info[0]

    @staticmethod
    def GlobalBundleAdjustemnt(gba, kfs, mps, edges, cam, iterations=5, robust=True):
        """Optimizer::GlobalBundleAdjustemnt src/Optimizer.cc:37-46 (the reference's spelling): BundleAdjustment over GetAllKeyFrames()
        and GetAllMapPoints()."""
        return Optimizer.BundleAdjustment(gba, kfs, mps, edges, cam, iterations, robust)

    @staticmethod
    def GlobalBundleAdjustemntDevice(gba, d_kf, nkf, d_mp, nmp, d_edges, nedges, cam, iterations, robust, d_kf_out, d_mp_out, d_not_included):
        return Optimizer.BundleAdjustmentDevice(gba, d_kf, nkf, d_mp, nmp, d_edges, nedges, cam, iterations, robust, d_kf_out, d_mp_out, d_not_included)

    @staticmethod
    def LocalBundleAdjustment(ba, kfs, mps, edges, cam, rounds=2):
        """One problem, host arrays: kfs BAKEYFRAME_DTYPE[nkf] (lLocalKeyFrames, then lFixedCameras with fixed set), mps
        MAPPOINT_DTYPE[nmp] (lLocalMapPoints; x, y, z are read and written), edges BAEDGE_DTYPE[ne] in the order the reference
        creates them; rounds = 1 is bDoMore == false.  -> (kfs_out, mps_out, erase u8 [ne] = vToErase, info BAINFO_DTYPE record).
        A refused problem (capacity, an edge outside it, a duplicate pair) raises PslfeError."""
        k = np.ascontiguousarray(kfs, BAKEYFRAME_DTYPE).reshape(-1)
        m = np.ascontiguousarray(mps, MAPPOINT_DTYPE).reshape(-1)
        e = np.ascontiguousarray(edges, BAEDGE_DTYPE).reshape(-1)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        ko, mo, er = np.zeros(max(len(k), 1), BAKEYFRAME_DTYPE), np.zeros(max(len(m), 1), MAPPOINT_DTYPE), np.zeros(max(len(e), 1), np.uint8)
        info = np.zeros(1, BAINFO_DTYPE)
        _check(lib().pslfe_ba_local(ba._h, _ptr(k) if len(k) else None, C.c_int(len(k)), _ptr(m) if len(m) else None, C.c_int(len(m)),
                                    _ptr(e) if len(e) else None, C.c_int(len(e)), _ptr(cam), C.c_int(rounds), _ptr(ko) if len(k) else None,
                                    _ptr(mo) if len(m) else None, _ptr(er) if len(e) else None, _ptr(info)), "pslfe_ba_local")
        return ko[:len(k)], mo[:len(m)], er[:len(e)], info[0]

    @staticmethod
    def LocalBundleAdjustmentDevice(ba, K, d_kf, d_kf_off, d_mp, d_mp_off, d_edges, d_edge_off, cam, rounds, d_kf_out, d_mp_out, d_erase, d_info):
        """K independent problems in one launch, HBM to HBM, asynchronous; all d_* are device addresses (ints).  The offset arrays have
        K + 1 ascending int32 entries; d_kf_out may be d_kf and d_mp_out may be d_mp; d_erase one byte per edge; d_info BAINFO_DTYPE [K]
        with the status of each problem (-4 capacity, -1 invalid: its outputs equal its inputs)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_ba_local_device(
            ba._h, C.c_int(K), C.c_void_p(d_kf or None), C.c_void_p(d_kf_off or None), C.c_void_p(d_mp or None), C.c_void_p(d_mp_off or None),
            C.c_void_p(d_edges or None), C.c_void_p(d_edge_off or None), _ptr(cam), C.c_int(rounds), C.c_void_p(d_kf_out or None),
            C.c_void_p(d_mp_out or None), C.c_void_p(d_erase or None), C.c_void_p(d_info or None)), "pslfe_ba_local_device")

    @staticmethod
    def LocalBundleAdjustmentAndInseclines(ba, kfs, mps, edges, lils, lil_edges, cam, rounds=2):
        """Optimizer::LocalBundleAdjustmentAndInseclines src/Optimizer.cc:1968-2534 (the call of LocalMapping::Run), one problem, host
        arrays: LocalBundleAdjustment's arguments plus lils MAPLIL_DTYPE[nlil] (w is read and written) and lil_edges
        BALILEDGE_DTYPE[nle] in the order the reference creates them.  -> (kfs_out, mps_out, erase u8 [ne], lils_out, erase_lil u8
        [nle], info).  ba needs LIL caps.  A refused problem raises PslfeError."""
        k = np.ascontiguousarray(kfs, BAKEYFRAME_DTYPE).reshape(-1)
        m = np.ascontiguousarray(mps, MAPPOINT_DTYPE).reshape(-1)
        e = np.ascontiguousarray(edges, BAEDGE_DTYPE).reshape(-1)
        l = np.ascontiguousarray(lils, MAPLIL_DTYPE).reshape(-1)
        f = np.ascontiguousarray(lil_edges, BALILEDGE_DTYPE).reshape(-1)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        ko, mo, er = np.zeros(max(len(k), 1), BAKEYFRAME_DTYPE), np.zeros(max(len(m), 1), MAPPOINT_DTYPE), np.zeros(max(len(e), 1), np.uint8)
        lo, el = np.zeros(max(len(l), 1), MAPLIL_DTYPE), np.zeros(max(len(f), 1), np.uint8)
        info = np.zeros(1, BAINFO_DTYPE)
        p = lambda a, n: _ptr(a) if n else None
        _check(lib().pslfe_ba_local_lil(ba._h, p(k, len(k)), C.c_int(len(k)), p(m, len(m)), C.c_int(len(m)), p(e, len(e)), C.c_int(len(e)),
                                        p(l, len(l)), C.c_int(len(l)), p(f, len(f)), C.c_int(len(f)), _ptr(cam), C.c_int(rounds), p(ko, len(k)),
                                        p(mo, len(m)), p(er, len(e)), p(lo, len(l)), p(el, len(f)), _ptr(info)), "pslfe_ba_local_lil")
        return ko[:len(k)], mo[:len(m)], er[:len(e)], lo[:len(l)], el[:len(f)], info[0]

    @staticmethod
    def LocalBundleAdjustmentAndInseclinesDevice(ba, K, d_kf, d_kf_off, d_mp, d_mp_off, d_edges, d_edge_off, d_lil, d_lil_off, d_lil_edges,
                                                 d_lil_edge_off, cam, rounds, d_kf_out, d_mp_out, d_erase, d_lil_out, d_erase_lil, d_nerased_lil,
                                                 d_info):
        """K problems in one launch, HBM to HBM, asynchronous: LocalBundleAdjustmentDevice plus the LIL rows, LIL edges and their
        offsets; d_lil_out may be d_lil and is what pose_lil_edges_device reads as its map; d_nerased_lil (int32 [K]) may be 0."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        v = lambda d: C.c_void_p(d or None)
        _check(lib().pslfe_ba_local_lil_device(
            ba._h, C.c_int(K), v(d_kf), v(d_kf_off), v(d_mp), v(d_mp_off), v(d_edges), v(d_edge_off), v(d_lil), v(d_lil_off), v(d_lil_edges),
            v(d_lil_edge_off), _ptr(cam), C.c_int(rounds), v(d_kf_out), v(d_mp_out), v(d_erase), v(d_lil_out), v(d_erase_lil), v(d_nerased_lil),
            v(d_info)), "pslfe_ba_local_lil_device")

    @staticmethod
    def PoseOptimization(Tcw, edges, cam, ctx=None, lil=None):
        """One frame, host arrays: Tcw a POSE_DTYPE record (pFrame->mTcw), edges POSEEDGE_DTYPE[n] in keypoint order.
        -> (ngood = the return value, Tcw_out, outlier u8 [n] = mvbOutlier of each edge's keypoint).  Fewer than 3 edges: (0, Tcw,
        zeros), as the reference leaves them (:291, :696).
        lil: POSELIL_DTYPE[m] in plane order (:631-693) -> (ngood, Tcw_out, outlier, outlier_lil u8 [m] = mvbOutlier_Insec of each
        edge's plane); ngood counts every LIL edge as good (:1022) and "fewer than 3" counts both kinds."""
        ctx = ctx or default_context()
        T = np.ascontiguousarray(Tcw, POSE_DTYPE).reshape(1)
        e = np.ascontiguousarray(edges, POSEEDGE_DTYPE)
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        out = np.zeros(1, POSE_DTYPE)
        outlier = np.zeros(max(len(e), 1), np.uint8)
        ng = C.c_int()
        if lil is not None:
            l = np.ascontiguousarray(lil, POSELIL_DTYPE)
            outlier_lil = np.zeros(max(len(l), 1), np.uint8)
            _check(lib().pslfe_pose_optimize_lil(ctx._h, _ptr(T), _ptr(e) if len(e) else None, C.c_int(len(e)), _ptr(l) if len(l) else None,
                                                 C.c_int(len(l)), _ptr(cam), _ptr(out), _ptr(outlier) if len(e) else None,
                                                 _ptr(outlier_lil) if len(l) else None, C.byref(ng)), "pslfe_pose_optimize_lil")
            return ng.value, out[0], outlier[:len(e)], outlier_lil[:len(l)]
        _check(lib().pslfe_pose_optimize(ctx._h, _ptr(T), _ptr(e) if len(e) else None, C.c_int(len(e)), _ptr(cam), _ptr(out),
                                         _ptr(outlier) if len(e) else None, C.byref(ng)), "pslfe_pose_optimize")
        return ng.value, out[0], outlier[:len(e)]

    @staticmethod
    def PoseOptimizationDevice(nframes, d_Tcw_in, d_edges, d_nedges, estride, cam, d_Tcw_out, d_outlier, d_ngood, d_info=0, ctx=None):
        """nframes independent frames in one launch, HBM to HBM, asynchronous; all d_* are device addresses (ints; d_info may be 0,
        d_Tcw_out may be d_Tcw_in).  d_ngood[f] = PSLFE_E_CAPACITY (-4) for a frame whose count exceeds estride."""
        ctx = ctx or default_context()
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_pose_optimize_device(ctx._h, C.c_int(nframes), C.c_void_p(d_Tcw_in or None), C.c_void_p(d_edges or None),
                                                C.c_void_p(d_nedges or None), C.c_int(estride), _ptr(cam), C.c_void_p(d_Tcw_out or None),
                                                C.c_void_p(d_outlier or None), C.c_void_p(d_ngood or None), C.c_void_p(d_info or None)),
               "pslfe_pose_optimize_device")

    @staticmethod
    def PoseOptimizationLilDevice(nframes, d_Tcw_in, d_edges, d_nedges, estride, d_lil, d_nlil, lstride, cam, d_Tcw_out, d_outlier,
                                  d_outlier_lil, d_ngood, d_info=0, ctx=None):
        """PoseOptimizationDevice with the LIL edges of every frame: d_lil POSELIL_DTYPE [nframes][lstride], d_nlil [nframes],
        d_outlier_lil [nframes][lstride] bytes.  LIL edge j of a frame has the edge index d_nedges[f] + j."""
        ctx = ctx or default_context()
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_pose_optimize_lil_device(
            ctx._h, C.c_int(nframes), C.c_void_p(d_Tcw_in or None), C.c_void_p(d_edges or None), C.c_void_p(d_nedges or None), C.c_int(estride),
            C.c_void_p(d_lil or None), C.c_void_p(d_nlil or None), C.c_int(lstride), _ptr(cam), C.c_void_p(d_Tcw_out or None),
            C.c_void_p(d_outlier or None), C.c_void_p(d_outlier_lil or None), C.c_void_p(d_ngood or None), C.c_void_p(d_info or None)),
            "pslfe_pose_optimize_lil_device")

    @staticmethod
    def LilEdgesDevice(nframes, d_le_l, le_stride, d_cross2d, plane_stride, d_nplanes, d_lil_index, d_map, nmap, d_lil, d_edge_plane, d_nlil,
                       lstride, ctx=None):
        """The LIL set-up loop :631-693 on the device: d_lil_index [nframes][plane_stride] = the MAPLIL_DTYPE row of each plane's map
        LIL or -1; plane i takes row i of mvle_l and row i of CrossPoint_2D (FrameGlue.lil_obs_device), as the reference does; edges
        compacted in plane order; d_nlil[f] = the full count, also above lstride."""
        ctx = ctx or default_context()
        _check(lib().pslfe_pose_lil_edges_device(
            ctx._h, C.c_int(nframes), C.c_void_p(d_le_l or None), C.c_int(le_stride), C.c_void_p(d_cross2d or None), C.c_int(plane_stride),
            C.c_void_p(d_nplanes or None), C.c_void_p(d_lil_index or None), C.c_void_p(d_map or None), C.c_int(nmap), C.c_void_p(d_lil or None),
            C.c_void_p(d_edge_plane or None), C.c_void_p(d_nlil or None), C.c_int(lstride)), "pslfe_pose_lil_edges_device")

    @staticmethod
    def OptimizeSim3(S12, pairs, cam1, cam2, th2, fix_scale, ctx=None):
        """Optimizer::OptimizeSim3 src/Optimizer.cc:2801-2996 for one candidate, host arrays: S12 a SIM3_DTYPE record (what Sim3Solver
        hands over), pairs SIM3PAIR_DTYPE[n] in KF1 keypoint order.  -> (nIn = the return value, S12_out SIM3D_DTYPE record, bad u8 [n]
        = 1 where the reference nulls vpMatches1[idx]).  S12_out is Sim3(R, t, s) of the input where the reference returns 0 before
        writing g2oS12 back."""
        ctx = ctx or default_context()
        S = np.ascontiguousarray(S12, SIM3_DTYPE).reshape(1)
        p = np.ascontiguousarray(pairs, SIM3PAIR_DTYPE)
        cam1 = np.ascontiguousarray(cam1, CAMERA_DTYPE).reshape(1)
        cam2 = np.ascontiguousarray(cam2, CAMERA_DTYPE).reshape(1)
        out = np.zeros(1, SIM3D_DTYPE)
        bad = np.zeros(max(len(p), 1), np.uint8)
        nin = C.c_int()
        _check(lib().pslfe_sim3_optimize(ctx._h, _ptr(S), _ptr(p) if len(p) else None, C.c_int(len(p)), _ptr(cam1), _ptr(cam2), C.c_float(th2),
                                         C.c_int(1 if fix_scale else 0), _ptr(out), _ptr(bad) if len(p) else None, C.byref(nin)),
               "pslfe_sim3_optimize")
        return nin.value, out[0], bad[:len(p)]

    @staticmethod
    def OptimizeSim3Device(ncand, d_S12_in, d_pairs, d_npairs, pstride, cam1, cam2, th2, fix_scale, d_S12_out, d_bad, d_nin, d_info=0, ctx=None):
        """ncand independent candidates in one launch, HBM to HBM, asynchronous; all d_* are device addresses (ints; d_info may be 0).
        d_nin[c] = PSLFE_E_CAPACITY (-4) for a count above pstride, PSLFE_E_INVALID (-1) for a negative one."""
        ctx = ctx or default_context()
        cam1 = np.ascontiguousarray(cam1, CAMERA_DTYPE).reshape(1)
        cam2 = np.ascontiguousarray(cam2, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_sim3_optimize_device(
            ctx._h, C.c_int(ncand), C.c_void_p(d_S12_in or None), C.c_void_p(d_pairs or None), C.c_void_p(d_npairs or None), C.c_int(pstride),
            _ptr(cam1), _ptr(cam2), C.c_float(th2), C.c_int(1 if fix_scale else 0), C.c_void_p(d_S12_out or None), C.c_void_p(d_bad or None),
            C.c_void_p(d_nin or None), C.c_void_p(d_info or None)), "pslfe_sim3_optimize_device")

    @staticmethod
    def Sim3PairsFromMatchesDevice(f1, slot1, f2, d_slots2, ncand, d_i2, d_mp1, d_skip1, n1, d_mp2, d_skip2, mp2stride, d_T1w, d_T2w,
                                   inv_level_sigma2, d_pairs, d_pair_kp, d_npairs, pstride):
        """The set-up loop :2854-2933 on the device for ncand candidates of the keyframe in slot slot1 of f1: d_i2 [ncand][f1 capacity] =
        the KF2 keypoint of each match or -1; rows compacted in KF1 keypoint order; d_npairs[c] = the full count, also above pstride."""
        s2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
        _check(lib().pslfe_sim3_pairs_from_matches_device(
            f1._h, C.c_int(slot1), f2._h, C.c_void_p(d_slots2 or None), C.c_int(ncand), C.c_void_p(d_i2 or None), C.c_void_p(d_mp1 or None),
            C.c_void_p(d_skip1 or None), C.c_int(n1), C.c_void_p(d_mp2 or None), C.c_void_p(d_skip2 or None), C.c_int(mp2stride),
            C.c_void_p(d_T1w or None), C.c_void_p(d_T2w or None), _ptr(s2), C.c_int(len(s2)), C.c_void_p(d_pairs or None),
            C.c_void_p(d_pair_kp or None), C.c_void_p(d_npairs or None), C.c_int(pstride)), "pslfe_sim3_pairs_from_matches_device")

    @staticmethod
    def MapPointIndexFromMatchesDevice(frame, nframes, d_match, d_owner, d_nq, qstride, d_mp_index):
        """F.mvpMapPoints[bestIdx] = pMP (src/ORBmatcher.cc:127) on the device: the owner rows of project_frustum_device and the matches
        of search_by_projection_map_device -> d_mp_index [nframes][frame capacity], the array EdgesFromMatchesDevice reads."""
        _check(lib().pslfe_pose_mp_index_from_matches_device(frame._h, C.c_int(nframes), C.c_void_p(d_match or None), C.c_void_p(d_owner or None),
                                                             C.c_void_p(d_nq or None), C.c_int(qstride), C.c_void_p(d_mp_index or None)),
               "pslfe_pose_mp_index_from_matches_device")

    @staticmethod
    def EdgesFromMatchesDevice(frame, slot0, nframes, d_mp_index, d_mp, mpstride, inv_level_sigma2, d_edges, d_edge_kp, d_nedges, estride):
        """The edge set-up loop :282-363 on the device: d_mp_index [nframes][frame capacity] = the PslMapPointGeom row of each
        keypoint's map point or -1; edges compacted in keypoint order; d_nedges[f] = the full count, also above estride."""
        s2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
        _check(lib().pslfe_pose_edges_from_matches_device(
            frame._h, C.c_int(slot0), C.c_int(nframes), C.c_void_p(d_mp_index or None), C.c_void_p(d_mp or None), C.c_int(mpstride), _ptr(s2),
            C.c_int(len(s2)), C.c_void_p(d_edges or None), C.c_void_p(d_edge_kp or None), C.c_void_p(d_nedges or None), C.c_int(estride)),
            "pslfe_pose_edges_from_matches_device")

    @staticmethod
    def Sim3PairsSigma2FromMatchesDevice(f1, slot1, f2, d_slots2, ncand, d_i2, d_mp1, d_skip1, n1, d_mp2, d_skip2, mp2stride, d_T1w, d_T2w,
                                         inv_level_sigma2, level_sigma2, d_pairs, d_pair_kp, d_npairs, pstride, d_sigma2):
        """Sim3PairsFromMatchesDevice with one more output: d_sigma2 [ncand][pstride][2] (may be 0) = mvLevelSigma2 of the two octaves of
        each row (src/Sim3Solver.cc:84-85), what Sim3Solver needs next to the rows."""
        s2 = np.ascontiguousarray(inv_level_sigma2, np.float32)
        l2 = np.ascontiguousarray(level_sigma2, np.float32)
        if len(l2) != len(s2):
            raise PslfeError(f"Sim3PairsSigma2FromMatchesDevice: {len(l2)} level sigma2 for {len(s2)} inverse ones")
        _check(lib().pslfe_sim3_pairs_sigma2_from_matches_device(
            f1._h, C.c_int(slot1), f2._h, C.c_void_p(d_slots2 or None), C.c_int(ncand), C.c_void_p(d_i2 or None), C.c_void_p(d_mp1 or None),
            C.c_void_p(d_skip1 or None), C.c_int(n1), C.c_void_p(d_mp2 or None), C.c_void_p(d_skip2 or None), C.c_int(mp2stride),
            C.c_void_p(d_T1w or None), C.c_void_p(d_T2w or None), _ptr(s2), C.c_int(len(s2)), C.c_void_p(d_pairs or None),
            C.c_void_p(d_pair_kp or None), C.c_void_p(d_npairs or None), C.c_int(pstride), _ptr(l2), C.c_void_p(d_sigma2 or None)),
            "pslfe_sim3_pairs_sigma2_from_matches_device")


class Sim3Solver:
    """== ORB_SLAM2::Sim3Solver (src/Sim3Solver.cc) of one candidate, with the reference's method names.  The constructor takes what the
    reference's constructor builds (:62-103): pairs SIM3PAIR_DTYPE[n] (the rows of the set-up loop; P1c and P2c are read), sigma2 [n][2]
    = mvLevelSigma2 of the two octaves of each row, indices1 [n] = mvnIndices1 (row -> KF1 keypoint), n_keys1 = vpMatched12.size().
    rand() is glibc's generator seeded with `seed` at the solver's first iteration; iterate() resumes the solver through
    (mnIterations, mnBestInliers), so rounds of iterate(5) are one find().  Parity with OpenCV is unpinned."""

    def __init__(self, pairs, sigma2, indices1, n_keys1, cam1, cam2, fix_scale, seed, ctx=None):
        self.ctx = ctx or default_context()
        self.pairs = np.ascontiguousarray(pairs, SIM3PAIR_DTYPE)
        self.sigma2 = np.ascontiguousarray(sigma2, np.float32).reshape(-1, 2)
        self.indices1 = np.ascontiguousarray(indices1, np.int32)
        if len(self.sigma2) != len(self.pairs) or len(self.indices1) != len(self.pairs):
            raise PslfeError("Sim3Solver: pairs, sigma2 and indices1 differ in length")
        self.n_keys1 = int(n_keys1)
        self.cam1 = np.ascontiguousarray(cam1, CAMERA_DTYPE).reshape(1)
        self.cam2 = np.ascontiguousarray(cam2, CAMERA_DTYPE).reshape(1)
        self.fix_scale, self.seed = bool(fix_scale), int(seed) & 0xffffffff
        self.result = np.zeros((), SIM3SOLVERRESULT_DTYPE)     # of the last call
        self.row_inliers = np.zeros(len(self.pairs), np.uint8)  # the flags of the last call by pair row
        self._best = np.zeros((), SIM3_DTYPE)
        self._iterations = self._best_inliers = 0
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.prob, self.min_inliers, self.max_its = float(probability), int(minInliers), int(maxIterations)
        self._iterations = 0                                   # mnIterations = 0 (:137); mnBestInliers stays

    def iterate(self, nIterations):
        """-> (ok = a Sim3 was returned, bNoMore, vbInliers bool [n_keys1], nInliers); GetEstimated* hold the Sim3 when ok"""
        n = len(self.pairs)
        res = np.zeros(1, SIM3SOLVERRESULT_DTYPE)
        flags = np.zeros(max(n, 1), np.uint8)
        _check(lib().pslfe_sim3_solve(self.ctx._h, _ptr(self.pairs) if n else None, _ptr(self.sigma2) if n else None, C.c_int(n), _ptr(self.cam1),
                                      _ptr(self.cam2), C.c_double(self.prob), C.c_int(self.min_inliers), C.c_int(self.max_its),
                                      C.c_int(1 if self.fix_scale else 0), C.c_uint32(self.seed), C.c_int(self._iterations),
                                      C.c_int(self._best_inliers), C.c_int(nIterations), _ptr(res), _ptr(flags) if n else None), "pslfe_sim3_solve")
        r = res[0]
        if r["status"] < 0:
            _check(int(r["status"]), "pslfe_sim3_solve")
        self.result, self.row_inliers = r, flags[:n]
        self._iterations, self._best_inliers = int(r["iterations"]), int(r["best_inliers"])
        ok = r["status"] == 1
        if ok:
            self._best = r["S12"].copy()
        vb = np.zeros(self.n_keys1, bool)
        if ok:
            rows = np.flatnonzero(flags[:n])
            vb[self.indices1[rows]] = True
        return bool(ok), bool(r["status"] == 2), vb, int(r["ninliers"])

    def find(self):
        """-> (ok, vbInliers12, nInliers)"""
        ok, _, vb, nin = self.iterate(self.max_its)
        return ok, vb, nin

    def GetEstimatedRotation(self):
        return self._best["R"].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self._best["t"].copy()

    def GetEstimatedScale(self):
        return np.float32(self._best["s"])

    @staticmethod
    def SolveDevice(ncand, d_pairs, d_sigma2, d_npairs, pstride, cam1, cam2, fix_scale, seed0, n_iterations, d_res, d_inliers, d_start_it=0,
                    d_best_in=0, prob=0.99, min_inliers=20, max_its=300, ctx=None):
        """Sim3Solver::iterate(n_iterations) for ncand candidates in one launch, HBM to HBM, asynchronous; all d_* are device addresses
        (ints; d_start_it / d_best_in may be 0: a fresh solver).  d_res SIM3SOLVERRESULT_DTYPE [ncand]; d_inliers [ncand][pstride] bytes by
        pair row.  status = PSLFE_E_CAPACITY (-4) for a count above pstride, PSLFE_E_INVALID (-1) for a negative one."""
        ctx = ctx or default_context()
        cam1 = np.ascontiguousarray(cam1, CAMERA_DTYPE).reshape(1)
        cam2 = np.ascontiguousarray(cam2, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_sim3_solve_device(
            ctx._h, C.c_int(ncand), C.c_void_p(d_pairs or None), C.c_void_p(d_sigma2 or None), C.c_void_p(d_npairs or None), C.c_int(pstride),
            _ptr(cam1), _ptr(cam2), C.c_double(prob), C.c_int(min_inliers), C.c_int(max_its), C.c_int(1 if fix_scale else 0),
            C.c_uint32(int(seed0) & 0xffffffff), C.c_void_p(d_start_it or None), C.c_void_p(d_best_in or None), C.c_int(n_iterations),
            C.c_void_p(d_res or None), C.c_void_p(d_inliers or None)), "pslfe_sim3_solve_device")

    @staticmethod
    def ComputeSim3Candidates(ncand, d_pairs, d_sigma2, d_npairs, pstride, cam1, cam2, fix_scale, seed0, prob=0.99, min_inliers=20, max_its=300,
                              per_round=5, ctx=None):
        """The candidate loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:284-345) for ncand candidates resident in HBM: rounds of
        iterate(5) for every candidate still in the race, one launch per round.  A generator: yields (round, c, result record, inlier
        flags by pair row u8 [pstride]) for every candidate that returns a Sim3, in the order the reference would try them (by round,
        then by index); the caller does what :313-340 do with it (SearchBySim3, OptimizeSim3) and stops iterating on bMatch.  bNoMore
        discards a candidate, as does a count below 0 or above pstride; the generator ends when none is left."""
        ctx = ctx or default_context()
        start, best = np.zeros(ncand, np.int32), np.zeros(ncand, np.int32)
        discarded = np.zeros(ncand, bool)
        res, flags = np.zeros(ncand, SIM3SOLVERRESULT_DTYPE), np.zeros((ncand, max(pstride, 1)), np.uint8)
        d_res, d_flags = ctx.device_array(res)[0], ctx.device_array(flags)[0]
        try:
            rnd = 0
            while ncand > 0 and not discarded.all():
                d_s, d_b = ctx.device_array(start)[0], ctx.device_array(best)[0]
                try:
                    Sim3Solver.SolveDevice(ncand, d_pairs, d_sigma2, d_npairs, pstride, cam1, cam2, fix_scale, seed0, per_round, d_res, d_flags, d_s,
                                           d_b, prob, min_inliers, max_its, ctx=ctx)
                    for d, a in ((d_res, res), (d_flags, flags)):
                        _check(lib().pslfe_device_download(ctx._h, _ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
                finally:
                    ctx.device_free(d_s)
                    ctx.device_free(d_b)
                for c in range(ncand):
                    if discarded[c]:
                        continue
                    st = int(res[c]["status"])
                    if st < 0 or st == 2:
                        discarded[c] = True
                        start[c] = max_its                      # runs no further iteration: its start is the end of every budget
                    if st < 0:
                        continue
                    if st != 2:
                        start[c] = res[c]["iterations"]
                    best[c] = res[c]["best_inliers"]
                    if st == 1:
                        yield rnd, c, res[c].copy(), flags[c, :pstride].copy()
                rnd += 1
        finally:
            ctx.device_free(d_res)
            ctx.device_free(d_flags)


class PnPsolver:
    """== ORB_SLAM2::PnPsolver (src/PnPsolver.cc) of one relocalisation candidate, with the reference's method names.  The constructor
    takes what the reference's constructor builds (:67-110): rows PNPROW_DTYPE[n] (mvP2D, mvP3Dw, mvSigma2), key_point_indices [n] =
    mvKeyPointIndices (row -> keypoint of F), n_keys = vpMapPointMatches.size().  rand() is glibc's generator seeded with `seed` at the
    solver's first iteration; iterate() resumes the solver through (mnIterations, mnBestInliers, mBestTcw, mvbBestInliers), also after a
    returned pose.  Parity with OpenCV is unpinned."""

    def __init__(self, rows, key_point_indices, n_keys, cam, seed, ctx=None):
        self.ctx = ctx or default_context()
        self.rows = np.ascontiguousarray(rows, PNPROW_DTYPE)
        self.key_point_indices = np.ascontiguousarray(key_point_indices, np.int32)
        if len(self.key_point_indices) != len(self.rows):
            raise PslfeError("PnPsolver: rows and key_point_indices differ in length")
        self.n_keys = int(n_keys)
        self.cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        self.seed = int(seed) & 0xffffffff
        self.result = np.zeros((), PNPRESULT_DTYPE)            # of the last call: the solver's state
        self.row_inliers = np.zeros(len(self.rows), np.uint8)  # the flags of the last call by row
        self.best_flags = np.zeros(max(len(self.rows), 1), np.uint8)   # mvbBestInliers
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.prob, self.min_inliers, self.max_its, self.min_set = float(probability), int(minInliers), int(maxIterations), int(minSet)
        self.epsilon, self.th2 = float(epsilon), float(th2)

    @staticmethod
    def RansacParameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4):
        """-> (mRansacMaxIts, mRansacMinInliers) after SetRansacParameters (:134-152) for a solver of N rows; no device is touched"""
        its, mn = C.c_int(), C.c_int()
        _check(lib().pslfe_pnp_ransac_parameters(C.c_double(probability), C.c_int(minInliers), C.c_int(maxIterations), C.c_int(minSet),
                                                 C.c_float(epsilon), C.c_int(N), C.byref(its), C.byref(mn)), "pslfe_pnp_ransac_parameters")
        return its.value, mn.value

    def iterate(self, nIterations):
        """-> (Tcw POSE_DTYPE record or None, bNoMore, vbInliers bool [n_keys] (empty without a pose), nInliers)"""
        n = len(self.rows)
        res = np.zeros(1, PNPRESULT_DTYPE)
        flags = np.zeros(max(n, 1), np.uint8)
        state = np.ascontiguousarray(self.result, PNPRESULT_DTYPE).reshape(1)
        _check(lib().pslfe_pnp_solve(self.ctx._h, _ptr(self.rows) if n else None, C.c_int(n), _ptr(self.cam), C.c_double(self.prob),
                                     C.c_int(self.min_inliers), C.c_int(self.max_its), C.c_int(self.min_set), C.c_float(self.epsilon),
                                     C.c_float(self.th2), C.c_uint32(self.seed), _ptr(state), _ptr(self.best_flags) if n else None,
                                     C.c_int(nIterations), _ptr(res), _ptr(flags) if n else None), "pslfe_pnp_solve")
        r = res[0]
        if r["status"] < 0:
            _check(int(r["status"]), "pslfe_pnp_solve")
        self.result, self.row_inliers = r.copy(), flags[:n]
        ok = bool(r["status"] & 1)
        vb = np.zeros(self.n_keys if ok else 0, bool)
        if ok:
            vb[self.key_point_indices[np.flatnonzero(flags[:n])]] = True
        return (r["Tcw"].copy() if ok else None), bool(r["status"] & 2), vb, int(r["inliers"])

    def find(self):
        """-> (Tcw or None, vbInliers, nInliers)"""
        its, _ = PnPsolver.RansacParameters(len(self.rows), self.prob, self.min_inliers, self.max_its, self.min_set, self.epsilon)
        T, _, vb, nin = self.iterate(its)
        return T, vb, nin

    @staticmethod
    def RowsFromMatchesDevice(frame, slot, ncand, d_mp_index, d_mp, mpstride, level_sigma2, d_rows, d_row_kp, d_nrows, rstride):
        """The constructor's loop :78-101 on the device for ncand candidates of the frame in `slot`: d_mp_index [ncand][frame capacity] =
        the PslMapPointGeom row (of candidate c's array d_mp + c*mpstride) of each keypoint's match or -1; rows compacted in keypoint
        order; d_row_kp = mvKeyPointIndices; d_nrows[c] = the full count, also above rstride."""
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        _check(lib().pslfe_pnp_rows_from_matches_device(
            frame._h, C.c_int(slot), C.c_int(ncand), C.c_void_p(d_mp_index or None), C.c_void_p(d_mp or None), C.c_int(mpstride), _ptr(s2),
            C.c_int(len(s2)), C.c_void_p(d_rows or None), C.c_void_p(d_row_kp or None), C.c_void_p(d_nrows or None), C.c_int(rstride)),
            "pslfe_pnp_rows_from_matches_device")

    @staticmethod
    def SolveDevice(ncand, d_rows, d_nrows, rstride, cam, seed0, n_iterations, d_state_in, d_best_flags, d_res, d_inliers, prob=0.99,
                    min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991, ctx=None):
        """PnPsolver::iterate(n_iterations) for ncand candidates in one launch, HBM to HBM, asynchronous; all d_* are device addresses
        (ints; d_state_in may be 0: fresh solvers, or d_res).  d_res PNPRESULT_DTYPE [ncand]; d_best_flags (read and written) and
        d_inliers [ncand][rstride] bytes by row.  status = PSLFE_E_CAPACITY (-4) for a count above rstride, PSLFE_E_INVALID (-1) for a
        negative count or state.  The defaults are Relocalization's (src/Tracking.cc:2076)."""
        ctx = ctx or default_context()
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_pnp_solve_device(
            ctx._h, C.c_int(ncand), C.c_void_p(d_rows or None), C.c_void_p(d_nrows or None), C.c_int(rstride), _ptr(cam), C.c_double(prob),
            C.c_int(min_inliers), C.c_int(max_its), C.c_int(min_set), C.c_float(epsilon), C.c_float(th2), C.c_uint32(int(seed0) & 0xffffffff),
            C.c_void_p(d_state_in or None), C.c_void_p(d_best_flags or None), C.c_int(n_iterations), C.c_void_p(d_res or None),
            C.c_void_p(d_inliers or None)), "pslfe_pnp_solve_device")

    @staticmethod
    def MapPointIndexFromInliersDevice(ncand, d_mp_index, d_row_kp, d_inliers, d_nrows, rstride, kpstride, d_mp_index_out, ctx=None):
        """src/Tracking.cc:2119-2128 on the device: keypoint j keeps its map point if its row is an inlier, everything else becomes -1;
        the result feeds Optimizer.EdgesFromMatchesDevice unchanged."""
        ctx = ctx or default_context()
        _check(lib().pslfe_pnp_mp_index_from_inliers_device(
            ctx._h, C.c_int(ncand), C.c_void_p(d_mp_index or None), C.c_void_p(d_row_kp or None), C.c_void_p(d_inliers or None),
            C.c_void_p(d_nrows or None), C.c_int(rstride), C.c_int(kpstride), C.c_void_p(d_mp_index_out or None)),
            "pslfe_pnp_mp_index_from_inliers_device")

    @staticmethod
    def RelocalizeCandidates(ncand, d_rows, d_nrows, rstride, cam, seed0, prob=0.99, min_inliers=10, max_its=300, epsilon=0.5, th2=5.991,
                             per_round=5, max_rounds=1000, ctx=None):
        """The candidate loop of Tracking::Relocalization (src/Tracking.cc:2088-2180) for ncand candidates resident in HBM: rounds of
        iterate(5) for every candidate still in the race, one launch per round.  A generator: yields (round, c, result record, inlier
        flags by row u8 [rstride]) for every candidate that returns a pose, in the order the reference would try them (by round, then
        by index); the caller does what :2107-2172 do with it (PoseOptimization, the two SearchByProjection) and stops iterating on
        bMatch.  bNoMore discards a candidate (its pose, if it came with one, is still yielded), as does a count below 0 or above
        rstride; a discarded candidate is parked with a negative state, which the kernel answers without solving.  The generator ends
        when no candidate is left, or after max_rounds rounds: a candidate whose every call returns a refined pose never says
        bNoMore, and the reference's loop ends on it only through bMatch."""
        ctx = ctx or default_context()
        state, res = np.zeros(ncand, PNPRESULT_DTYPE), np.zeros(ncand, PNPRESULT_DTYPE)
        discarded = np.zeros(ncand, bool)
        flags = np.zeros((ncand, max(rstride, 1)), np.uint8)
        d_res, d_flags, d_best = ctx.device_array(res)[0], ctx.device_array(flags)[0], ctx.device_array(flags)[0]
        try:
            rnd = 0
            while ncand > 0 and not discarded.all() and rnd < max_rounds:
                d_state = ctx.device_array(state)[0]
                try:
                    PnPsolver.SolveDevice(ncand, d_rows, d_nrows, rstride, cam, seed0, per_round, d_state, d_best, d_res, d_flags, prob,
                                          min_inliers, max_its, 4, epsilon, th2, ctx=ctx)
                    for d, a in ((d_res, res), (d_flags, flags)):
                        _check(lib().pslfe_device_download(ctx._h, _ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
                finally:
                    ctx.device_free(d_state)
                for c in range(ncand):
                    if discarded[c]:
                        continue
                    st = int(res[c]["status"])
                    if st < 0 or st & 2:
                        discarded[c] = True
                        state[c]["iterations"] = -1
                    if st < 0:
                        continue
                    if not discarded[c]:
                        state[c] = res[c]
                    if st & 1:
                        yield rnd, c, res[c].copy(), flags[c, :rstride].copy()
                rnd += 1
        finally:
            for d in (d_res, d_flags, d_best):
                ctx.device_free(d)


class Initializer:
    """== ORB_SLAM2::Initializer (src/Initializer.cc) of one reference frame, with the reference's method names.  The constructor takes
    what the reference's takes from ReferenceFrame (:33-42): mvKeysUn as float32 [n1][2] (x, y) and K (a CAMERA_DTYPE record; fx, fy,
    cx, cy are read), sigma = 1.0, iterations = 200.  rand() is glibc's generator seeded with `seed` at every Initialize (the reference
    seeds once per process with 0: seed 0 is its first Initialize).  Parity with OpenCV is unpinned."""

    def __init__(self, ReferenceKeys, K, sigma=1.0, iterations=200, seed=0, ctx=None):
        self.ctx = ctx or default_context()
        self.keys1 = np.ascontiguousarray(ReferenceKeys, np.float32).reshape(-1, 2)
        self.cam = np.ascontiguousarray(K, CAMERA_DTYPE).reshape(1)
        self.sigma, self.max_its, self.seed = float(sigma), int(iterations), int(seed) & 0xffffffff
        self.result = np.zeros((), INITRESULT_DTYPE)   # of the last call

    def Initialize(self, CurrentKeys, vMatches12):
        """-> (bool, R21 float32 [3][3], t21 float32 [3], vP3D float32 [n1][3], vbTriangulated bool [n1]); CurrentKeys = CurrentFrame's
        mvKeysUn as float32 [n2][2], vMatches12 int32 [n1]"""
        keys2 = np.ascontiguousarray(CurrentKeys, np.float32).reshape(-1, 2)
        m = np.ascontiguousarray(vMatches12, np.int32).reshape(-1)
        n1, n2 = len(self.keys1), len(keys2)
        if len(m) != n1:
            raise PslfeError("Initializer: vMatches12 has one entry per reference keypoint")
        res = np.zeros(1, INITRESULT_DTYPE)
        p3d, tri = np.zeros((max(n1, 1), 3), np.float32), np.zeros(max(n1, 1), np.uint8)
        _check(lib().pslfe_init_initialize(self.ctx._h, _ptr(self.keys1) if n1 else None, C.c_int(n1), _ptr(keys2) if n2 else None, C.c_int(n2),
                                           _ptr(m) if n1 else None, _ptr(self.cam), C.c_float(self.sigma), C.c_int(self.max_its),
                                           C.c_uint32(self.seed), _ptr(res), _ptr(p3d) if n1 else None, _ptr(tri) if n1 else None),
               "pslfe_init_initialize")
        self.result = res[0].copy()
        return (bool(res[0]["status"] & 1), res[0]["R21"].reshape(3, 3).copy(), res[0]["t21"].copy(), p3d[:n1], tri[:n1].astype(bool))

    @staticmethod
    def Sets(seed, N, iterations):
        """mvSets (:77-97) of a pair with N matches -> int32 [iterations][8]; no device is touched"""
        s = np.zeros((max(iterations, 1), 8), np.int32)
        _check(lib().pslfe_init_sets(C.c_uint32(int(seed) & 0xffffffff), C.c_int(N), C.c_int(iterations), _ptr(s)), "pslfe_init_sets")
        return s[:max(iterations, 0)]

    @staticmethod
    def DebugSelect(cosines, ctx=None):
        """For the tests: a vCosParallax (float32 [n >= 1]) through the kernel's ordered keys and radix selection -> (keys uint32 [n],
        the cosine at sorted index min(50, n - 1), its parallax in degrees)"""
        ctx = ctx or default_context()
        c = np.ascontiguousarray(cosines, np.float32).reshape(-1)
        keys, sel, par = np.zeros(max(len(c), 1), np.uint32), np.zeros(1, np.float32), np.zeros(1, np.float32)   # arrays: a NaN keeps its bits
        _check(lib().pslfe_init_debug_select(ctx._h, _ptr(c) if len(c) else None, C.c_int(len(c)), _ptr(keys), _ptr(sel), _ptr(par)),
               "pslfe_init_debug_select")
        return keys[:len(c)], sel[0], par[0]

    @staticmethod
    def InitializeDevice(npairs, d_keys1, d_nkeys1, d_keys2, d_nkeys2, key_stride_bytes, kstride, d_matches12, mstride, K, d_res, d_p3d,
                         d_triangulated, d_matches12_out=0, sigma=1.0, iterations=200, seed0=0, ctx=None):
        """Initialize for npairs independent frame pairs in one launch, HBM to HBM, asynchronous; all d_* are device addresses (ints).
        d_res INITRESULT_DTYPE [npairs]; d_p3d float32 [npairs][mstride][3] and d_triangulated bytes [npairs][mstride] by reference
        keypoint; d_matches12_out (may be 0) = mvIniMatches after src/Tracking.cc:712-719.  status = PSLFE_E_CAPACITY (-4) for a count
        above its stride, PSLFE_E_INVALID (-1) for a negative count or a match outside frame 2."""
        ctx = ctx or default_context()
        cam = np.ascontiguousarray(K, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_init_initialize_device(
            ctx._h, C.c_int(npairs), C.c_void_p(d_keys1 or None), C.c_void_p(d_nkeys1 or None), C.c_void_p(d_keys2 or None),
            C.c_void_p(d_nkeys2 or None), C.c_int(key_stride_bytes), C.c_int(kstride), C.c_void_p(d_matches12 or None), C.c_int(mstride), _ptr(cam),
            C.c_float(sigma), C.c_int(iterations), C.c_uint32(int(seed0) & 0xffffffff), C.c_void_p(d_res or None), C.c_void_p(d_p3d or None),
            C.c_void_p(d_triangulated or None), C.c_void_p(d_matches12_out or None)), "pslfe_init_initialize_device")

    @staticmethod
    def InitializeFramesDevice(f1, slot1, f2, slot2, d_matches12, mstride, K, d_res, d_p3d, d_triangulated, d_matches12_out=0, sigma=1.0,
                               iterations=200, seed0=0):
        """The same with the keypoints of frame slots, straight behind search_for_initialization_device with its d_matches12: pair p =
        (f1 slot slot1[p], f2 slot slot2[p]); mstride >= f1's capacity."""
        s1 = np.ascontiguousarray(slot1, np.int32).reshape(-1)
        s2 = np.ascontiguousarray(slot2, np.int32).reshape(-1)
        if len(s1) != len(s2):
            raise ValueError("slot1 and slot2 differ in length")
        cam = np.ascontiguousarray(K, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_init_initialize_frames_device(
            f1._h, _ptr(s1), f2._h, _ptr(s2), C.c_int(len(s1)), C.c_void_p(d_matches12 or None), C.c_int(mstride), _ptr(cam), C.c_float(sigma),
            C.c_int(iterations), C.c_uint32(int(seed0) & 0xffffffff), C.c_void_p(d_res or None), C.c_void_p(d_p3d or None),
            C.c_void_p(d_triangulated or None), C.c_void_p(d_matches12_out or None)), "pslfe_init_initialize_frames_device")


class LINEextractor:
    """== ORB_SLAM2::LINEextractor (add_inc/LineExtractor.h:160-255)."""

    def __init__(self, numOctaves=1, scale=1.2, nLSDFeature=200, min_line_length=0.0, ctx=None, max_batch=1):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        self.numOctaves = numOctaves
        _check(lib().pslfe_line_create(self.ctx._h, C.c_int(numOctaves), C.c_float(scale), C.c_int(nLSDFeature),
                                       C.c_double(min_line_length), C.c_int(max_batch), C.byref(self._h)), "pslfe_line_create")
        lib().pslfe_line_scale_factor.restype = C.c_float

    LSD_REFINE_STD, LSD_REFINE_ADV = 1, 2

    def set_refine(self, mode):
        """cv::createLineSegmentDetector(refine) behind the extractor: LSD_REFINE_ADV (default: rect_improve + NFA test, what
        the stock contrib LSDDetector constructs) or LSD_REFINE_STD (the vendored, never-called LSDDetectorC)."""
        _check(lib().pslfe_line_set_refine(self._h, C.c_int(mode)), "pslfe_line_set_refine")

    def GetLevels(self):
        return lib().pslfe_line_levels(self._h)

    def GetScaleFactor(self):
        return lib().pslfe_line_scale_factor(self._h)

    def GetScaleFactors(self):
        a = np.zeros(self.numOctaves, np.float32)
        _check(lib().pslfe_line_scale_factors(self._h, _ptr(a), None, None, None), "pslfe_line_scale_factors")
        return a

    def lsd_detect(self, image, cap=8192):
        """LSDDetector::detect up to the clamped segment list -> (n, 4) float32."""
        assert image.dtype == np.uint8 and image.ndim == 2
        h, w = image.shape
        seg = np.zeros((cap, 4), np.float32)
        n = C.c_int()
        _check(lib().pslfe_lsd_detect(self._h, _ptr(image), C.c_int(w), C.c_int(h), C.c_int(image.strides[0]), _ptr(seg),
                                      C.c_int(cap), C.byref(n)), "pslfe_lsd_detect")
        return seg[:n.value].copy()

    def debug_gradient(self, frame=0):
        W, H = C.c_int(), C.c_int()
        _check(lib().pslfe_line_debug_gradient(self._h, C.c_int(frame), C.byref(W), C.byref(H), None, None, None), "pslfe_line_debug_gradient")
        scaled = np.zeros((H.value, W.value), np.float64)
        ang = np.zeros((H.value, W.value), np.float32)
        mod = np.zeros((H.value, W.value), np.float64)
        _check(lib().pslfe_line_debug_gradient(self._h, C.c_int(frame), C.byref(W), C.byref(H), _ptr(scaled), _ptr(ang), _ptr(mod)),
               "pslfe_line_debug_gradient")
        return scaled, ang, mod

    def close(self):
        if self._h:
            lib().pslfe_line_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _line_call(self, image, mask=None):
    """operator()(image, mask, keylines, descriptors, lineVec2d) -> (keylines, descriptors, lineEq)."""
    if image is None or image.size == 0:
        return np.zeros(0, KEYLINE_DTYPE), np.zeros((0, 32), np.uint8), np.zeros((0, 3))
    assert image.dtype == np.uint8 and image.ndim == 2
    h, w = image.shape
    cap = 1024
    kls = np.zeros(cap, KEYLINE_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    eq = np.zeros((cap, 3), np.float64)
    n = C.c_int()
    _check(lib().pslfe_line_extract(self._h, _ptr(image), C.c_int(w), C.c_int(h), C.c_int(image.strides[0]), _ptr(kls), _ptr(desc),
                                    _ptr(eq), C.c_int(cap), C.byref(n)), "pslfe_line_extract")
    return kls[:n.value].copy(), desc[:n.value].copy(), eq[:n.value].copy()


def _line_extract_batch_device(self, d_ptr, nframes, w, h, stride, frame_stride):
    _check(lib().pslfe_line_extract_batch_device(self._h, C.c_void_p(d_ptr), C.c_int(nframes), C.c_int(w), C.c_int(h), C.c_int(stride),
                                                 C.c_size_t(frame_stride)), "pslfe_line_extract_batch_device")


def _line_fetch(self, frame, cap=1024):
    kls = np.zeros(cap, KEYLINE_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    eq = np.zeros((cap, 3), np.float64)
    n, st = C.c_int(), C.c_int()
    _check(lib().pslfe_line_fetch(self._h, C.c_int(frame), _ptr(kls), _ptr(desc), _ptr(eq), C.c_int(cap), C.byref(n), C.byref(st)),
           "pslfe_line_fetch")
    return kls[:n.value].copy(), desc[:n.value].copy(), eq[:n.value].copy(), st.value


def _line_segments_fetch(self, frame, cap=8192):
    """The LSD segment list of one frame of the last batch -> (n, 4) float32 (what lsd_detect returns for that image)."""
    seg = np.zeros((cap, 4), np.float32)
    n = C.c_int()
    _check(lib().pslfe_line_segments_fetch(self._h, C.c_int(frame), _ptr(seg), C.c_int(cap), C.byref(n)), "pslfe_line_segments_fetch")
    return seg[:n.value].copy()


def _line_results_device(self):
    k, d, e, c, cap = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int()
    _check(lib().pslfe_line_results_device(self._h, C.byref(k), C.byref(d), C.byref(e), C.byref(c), C.byref(cap)), "pslfe_line_results_device")
    return k.value, d.value, e.value, c.value, cap.value


def _line_optimize_and_merge(self, segments, w, h, cap=1024):
    seg = np.ascontiguousarray(segments, np.float32).reshape(-1, 4)
    kls = np.zeros(cap, KEYLINE_DTYPE)
    n = C.c_int()
    _check(lib().pslfe_line_optimize_and_merge(self._h, _ptr(seg), C.c_int(len(seg)), C.c_int(w), C.c_int(h), _ptr(kls), C.c_int(cap),
                                               C.byref(n)), "pslfe_line_optimize_and_merge")
    return kls[:n.value].copy()


def _line_lbd(self, image, keylines, want_float=False):
    kls = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
    h, w = image.shape
    desc = np.zeros((max(len(kls), 1), 32), np.uint8)
    fdesc = np.zeros((max(len(kls), 1), 72), np.float32) if want_float else None
    _check(lib().pslfe_lbd_compute(self._h, _ptr(image), C.c_int(w), C.c_int(h), C.c_int(image.strides[0]), _ptr(kls), C.c_int(len(kls)),
                                   _ptr(desc), _ptr(fdesc)), "pslfe_lbd_compute")
    return (desc[:len(kls)], fdesc[:len(kls)]) if want_float else desc[:len(kls)]


def _line_debug_sobel(self, w, h, frame=0):
    dx = np.zeros((h, w), np.int16)
    dy = np.zeros((h, w), np.int16)
    _check(lib().pslfe_line_debug_sobel(self._h, C.c_int(frame), _ptr(dx), _ptr(dy)), "pslfe_line_debug_sobel")
    return dx, dy


def _line_pair(self, lines, radius, fanThr, cols, rows, cap=4096):
    """CPartiallyRecoverConnectivity(mLines, radius, fans, img, fanThr) -> fans (k, 4)."""
    L = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
    fans = np.zeros((cap, 4), np.float32)
    k = C.c_int()
    _check(lib().pslfe_lil_pair(self._h, _ptr(L), C.c_int(len(L)), C.c_float(radius), C.c_float(fanThr), C.c_int(cols), C.c_int(rows),
                                _ptr(fans), C.c_int(cap), C.byref(k)), "pslfe_lil_pair")
    return fans[:k.value].copy()


def _line_pair_batch_device(self, radius=20.0, fanThr=np.pi / 4):
    _check(lib().pslfe_line_pair_batch_device(self._h, C.c_float(radius), C.c_float(fanThr)), "pslfe_line_pair_batch_device")


def _line_fans_fetch(self, frame, cap=4096):
    fans = np.zeros((cap, 4), np.float32)
    k = C.c_int()
    _check(lib().pslfe_line_fans_fetch(self._h, C.c_int(frame), _ptr(fans), C.c_int(cap), C.byref(k)), "pslfe_line_fans_fetch")
    return fans[:k.value].copy()


def _line_match_batch_device(self, shift, nnr, d_matches12, d_nmatches):
    _check(lib().pslfe_line_match_batch_device(self._h, C.c_int(shift), C.c_float(nnr), C.c_void_p(d_matches12), C.c_void_p(d_nmatches)),
           "pslfe_line_match_batch_device")


LINEextractor.match_batch_device = _line_match_batch_device
LINEextractor.__call__ = _line_call
LINEextractor.extract_batch_device = _line_extract_batch_device
LINEextractor.fetch = _line_fetch
LINEextractor.segments_fetch = _line_segments_fetch
LINEextractor.results_device = _line_results_device
LINEextractor.optimize_and_merge = _line_optimize_and_merge
LINEextractor.lbd_compute = _line_lbd
LINEextractor.debug_sobel = _line_debug_sobel
LINEextractor.pair = _line_pair
LINEextractor.pair_batch_device = _line_pair_batch_device
def _line_fans_device(self):
    f, n, st = C.c_void_p(), C.c_void_p(), C.c_int()
    _check(lib().pslfe_line_fans_device(self._h, C.byref(f), C.byref(n), C.byref(st)), "pslfe_line_fans_device")
    return f.value, n.value


LINEextractor.fans_fetch = _line_fans_fetch
LINEextractor.fans_device = _line_fans_device


# ---- pslfe_debug_math: the kernels' restated libm on the device (include/pslfe.h: PSLFE_MATH_*) ----
MATH_FUNCTIONS = ("atanf", "tanf", "sincosf", "fast_atan2", "atan2f", "fdiv", "sqrtf", "cvround_f", "log", "exp", "log10", "pow_pos",
                  "sinh_small", "log_gamma", "glibc_sin", "glibc_cos", "cos_sin_f64", "cos_sin_2pi_f32", "ratio_inv", "ddiv", "dsqrt",
                  "cvround_d")
_F4, _F8, _I4 = np.dtype("<f4"), np.dtype("<f8"), np.dtype("<i4")
# name -> (input dtype, takes b, out0 dtype, out1 dtype or None)
MATH_SIGNATURES = {
    "atanf": (_F4, False, _F4, None), "tanf": (_F4, False, _F4, None), "sincosf": (_F4, False, _F4, _F4),
    "fast_atan2": (_F4, True, _F4, None), "atan2f": (_F4, True, _F4, None), "fdiv": (_F4, True, _F4, None),
    "sqrtf": (_F4, False, _F4, None), "cvround_f": (_F4, False, _I4, None),
    "log": (_F8, False, _F8, None), "exp": (_F8, False, _F8, None), "log10": (_F8, False, _F8, None), "pow_pos": (_F8, True, _F8, None),
    "sinh_small": (_F8, False, _F8, None), "log_gamma": (_F8, False, _F8, None), "glibc_sin": (_F8, False, _F8, None),
    "glibc_cos": (_F8, False, _F8, None), "cos_sin_f64": (_F8, False, _F8, _F8), "cos_sin_2pi_f32": (_F8, False, _F4, _F4),
    "ratio_inv": (_F8, True, _F8, None), "ddiv": (_F8, True, _F8, None), "dsqrt": (_F8, False, _F8, None),
    "cvround_d": (_F8, False, _I4, None),
}


def math_arrays(fn, a, b=None):
    """(id, a, b, out0, out1) for function `fn` (a name of MATH_FUNCTIONS): the arguments as contiguous arrays of the function's
    input type and zeroed outputs of its output types.  Shared by debug_math and the oracle's twin (tests/oracle_lib.py)."""
    ti, binary, t0, t1 = MATH_SIGNATURES[fn]
    a = np.ascontiguousarray(a, ti).ravel()
    if binary:
        b = np.ascontiguousarray(b, ti).ravel()
        assert b.shape == a.shape, "a and b differ in length"
    else:
        assert b is None, f"{fn} takes one argument"
    return MATH_FUNCTIONS.index(fn), a, b, np.zeros(len(a), t0), None if t1 is None else np.zeros(len(a), t1)


def debug_math(fn, a, b=None, ctx=None):
    """pslfe_debug_math: function `fn` of the kernels' restated libm evaluated on the device, one thread per element -> out0, or
    (out0, out1) for sincosf (sin, cos), cos_sin_f64 and cos_sin_2pi_f32 (cos, sin)."""
    ctx = ctx or default_context()
    i, a, b, o0, o1 = math_arrays(fn, a, b)
    _check(lib().pslfe_debug_math(ctx._h, C.c_int(i), C.c_size_t(len(a)), _ptr(a), _ptr(b), _ptr(o0), _ptr(o1)), "pslfe_debug_math")
    return o0 if o1 is None else (o0, o1)


NFA_FIRST = -2


def _line_debug_nfa(self, w, h, phase, nrect, p_lognfa, nk):
    """pslfe_line_debug_nfa: k_lsd_nfa_setup<phase> + k_lsd_nfa_series<phase> on caller-supplied trials.  nrect: [F] rectangles per
    frame; p_lognfa: [F, R, 2] (p, incoming log_nfa); nk: [F, R, 5, 2] int32 (n, k) per trial, n < 0 = excluded by the width guard.
    -> (vals [F, R, 5], tail [F, R, 5], logNT).  Entries beyond nrect[f] (and trials 1 .. 4 of NFA_FIRST) are NaN.  Overwrites the
    rectangle and NFA buffers of the last extraction."""
    nrect = np.ascontiguousarray(nrect, np.int32).ravel()
    F = len(nrect)
    pl = np.ascontiguousarray(p_lognfa, np.float64)
    nk = np.ascontiguousarray(nk, np.int32)
    R = pl.shape[1]
    assert pl.shape == (F, R, 2) and nk.shape == (F, R, 5, 2), (pl.shape, nk.shape)
    vals = np.full((F, R, 5), np.nan)
    tail = np.full((F, R, 5), np.nan)
    lognt = C.c_double()
    _check(lib().pslfe_line_debug_nfa(self._h, C.c_int(w), C.c_int(h), C.c_int(phase), C.c_int(F), _ptr(nrect), C.c_int(R), _ptr(pl), _ptr(nk),
                                      _ptr(vals), _ptr(tail), C.byref(lognt)), "pslfe_line_debug_nfa")
    return vals, tail, lognt.value


LINEextractor.debug_nfa = _line_debug_nfa


def _lsd_search_by_geom_appearance(self, kl_last, desc_last, kl_cur, desc_cur, has_mapline, desc_th, bounds):
    """LSDmatcher::SearchByGeomNApearance(CurrentFrame, LastFrame, desc_th) -> (lmatches, matches12, assigned).
    bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY)."""
    k1 = np.ascontiguousarray(kl_last, KEYLINE_DTYPE)
    k2 = np.ascontiguousarray(kl_cur, KEYLINE_DTYPE)
    d1 = np.ascontiguousarray(desc_last, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(desc_cur, np.uint8).reshape(-1, 32)
    hm = np.ascontiguousarray(has_mapline, np.uint8)
    m12 = np.full(max(len(k1), 1), -1, np.int32)
    asg = np.full(max(len(k2), 1), -1, np.int32)
    n = C.c_int()
    _check(lib().pslfe_line_search_by_geom_appearance(self.ctx._h, _ptr(k1), _ptr(d1), C.c_int(len(k1)), _ptr(k2), _ptr(d2), C.c_int(len(k2)),
                                                      _ptr(hm), C.c_float(desc_th), *[C.c_float(b) for b in bounds], _ptr(m12), _ptr(asg),
                                                      C.byref(n)), "pslfe_line_search_by_geom_appearance")
    return n.value, m12[:len(k1)], asg[:len(k2)]


def _lsd_frame_bf_match(self, ldesc1, ldesc2, TH):
    """LSDmatcher::FrameBFMatch(ldesc1, ldesc2, LineMatches, TH) -> LineMatches."""
    d1 = np.ascontiguousarray(ldesc1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(ldesc2, np.uint8).reshape(-1, 32)
    lm = np.full(max(len(d1), 1), -1, np.int32)
    _check(lib().pslfe_line_frame_bf_match(self.ctx._h, _ptr(d1), C.c_int(len(d1)), _ptr(d2), C.c_int(len(d2)), C.c_float(self.mfNNratio),
                                           C.c_float(TH), _ptr(lm)), "pslfe_line_frame_bf_match")
    return lm[:len(d1)]


LSDmatcher.SearchByGeomNApearance = _lsd_search_by_geom_appearance
LSDmatcher.FrameBFMatch = _lsd_frame_bf_match


def associate_planes(planes, points, map_planes, dTh, aTh, live=True, map_bad=None, ctx=None):
    """Map::AssociatePlanesByBoundary (live) / InsectLineMatch::SearchMapInsectline (dead) -> (nmatches, assoc)."""
    ctx = ctx or default_context()
    p = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
    q = np.ascontiguousarray(points, np.float64).reshape(-1, 15)
    m = np.ascontiguousarray(map_planes, np.float32).reshape(-1, 4)
    b = None if map_bad is None else np.ascontiguousarray(map_bad, np.uint8)
    assoc = np.full(max(len(p), 1), -1, np.int32)
    n = C.c_int()
    _check(lib().pslfe_associate_planes(ctx._h, _ptr(p), _ptr(q), C.c_int(len(p)), _ptr(m), _ptr(b), C.c_int(len(m)), C.c_float(dTh),
                                        C.c_float(aTh), C.c_int(1 if live else 0), _ptr(assoc), C.byref(n)), "pslfe_associate_planes")
    return n.value, assoc[:len(p)]


LINEQUERY_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("radius", "<f4"), ("th_cos", "<f4"),
                            ("vx", "<f4"), ("vy", "<f4"), ("length", "<f4"), ("blocks", "<i4"), ("wdir", "<f8", (3,))])
assert LINEQUERY_DTYPE.itemsize == 64


def _lsd_search_by_projection(self, kls, desc, lineEq, bounds, queries, qdesc, mode=0, dir3d=None, taken=None, want_grid=False):
    """LSDmatcher::SearchByProjection: mode 0 = (CurrentFrame, LastFrame, th), mode 1 = (F, vpMapLines, ...).
    bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY) -> (nmatches, match, assigned[, grid_start, grid_idx])."""
    k = np.ascontiguousarray(kls, KEYLINE_DTYPE)
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    eq = np.ascontiguousarray(lineEq, np.float64).reshape(-1, 3)
    q = np.ascontiguousarray(queries, LINEQUERY_DTYPE)
    qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    d3 = None if dir3d is None else np.ascontiguousarray(dir3d, np.float64).reshape(-1, 3)
    tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
    match = np.full(max(len(q), 1), -1, np.int32)
    asg = np.full(max(len(k), 1), -1, np.int32)
    nm, gn = C.c_int(), C.c_int()
    gs = np.zeros(64 * 48 + 1, np.int32) if want_grid else None
    gi = np.zeros(max(len(k), 1) * 112, np.int32) if want_grid else None
    _check(lib().pslfe_line_search_by_projection(self.ctx._h, _ptr(k), _ptr(d), _ptr(eq), _ptr(d3), C.c_int(len(k)),
                                                 *[C.c_float(b) for b in bounds], _ptr(q), _ptr(qd), C.c_int(len(q)), _ptr(tk),
                                                 C.c_int(mode), C.c_float(self.mfNNratio), _ptr(match), _ptr(asg), C.byref(nm),
                                                 _ptr(gs), _ptr(gi), C.c_int(0 if gi is None else len(gi)), C.byref(gn)),
           "pslfe_line_search_by_projection")
    out = (nm.value, match[:len(q)], asg[:len(k)])
    return out + (gs, gi[:gn.value]) if want_grid else out


LSDmatcher.SearchByProjection = _lsd_search_by_projection

MAPLINE_DTYPE = np.dtype([("sp", "<f8", (3,)), ("ep", "<f8", (3,)), ("normal", "<f8", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4")])
LASTLINE_DTYPE = np.dtype([("sp", "<f8", (3,)), ("ep", "<f8", (3,)), ("normal", "<f8", (3,)), ("min_dist", "<f4"), ("max_dist", "<f4"),
                           ("state", "<i4"), ("reserved", "<i4")])
assert MAPLINE_DTYPE.itemsize == 80 and LASTLINE_DTYPE.itemsize == 88


def line_project_frustum(Tcw, ml, mldesc, cam, log_scale_factor, view_cos_limit, th, bounds, ctx=None):
    """Frame::isInFrustum(MapLine*) src/Frame.cc:828-904 for every map line (MAPLINE_DTYPE[M], descriptors [M, 32]) and the query rows of
    LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) add_src/LSDmatcher.cpp:260-289 for those in view.
    bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY) -> (queries LINEQUERY_DTYPE, qdesc, owner, inview [M] u8, level [M] i32, viewcos [M] f32)."""
    ctx = ctx or default_context()
    T = np.ascontiguousarray(Tcw, POSE_DTYPE).reshape(1)
    ml = np.ascontiguousarray(ml, MAPLINE_DTYPE)
    md = np.ascontiguousarray(mldesc, np.uint8).reshape(-1, 32)
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    M = len(ml)
    q = np.zeros(max(M, 1), LINEQUERY_DTYPE)
    qd = np.zeros((max(M, 1), 32), np.uint8)
    ow = np.zeros(max(M, 1), np.int32)
    inview, level, vc = np.zeros(max(M, 1), np.uint8), np.zeros(max(M, 1), np.int32), np.zeros(max(M, 1), np.float32)
    nq = C.c_int()
    _check(lib().pslfe_line_project_frustum(ctx._h, _ptr(T), _ptr(ml), _ptr(md), C.c_int(M), _ptr(cam), C.c_float(log_scale_factor),
                                            C.c_float(view_cos_limit), C.c_float(th), *[C.c_float(b) for b in bounds], _ptr(q), _ptr(qd),
                                            _ptr(ow), C.byref(nq), C.c_int(M), _ptr(inview), _ptr(level), _ptr(vc)),
           "pslfe_line_project_frustum")
    n = nq.value
    return q[:n], qd[:n], ow[:n], inview[:M], level[:M], vc[:M]


def line_project_frustum_device(nframes, d_Tcw, d_ml, d_mldesc, d_nml, mlstride, cam, log_scale_factor, view_cos_limit, th, bounds,
                                d_queries, d_qdesc, d_owner, d_nq, qstride, d_inview=0, d_level=0, d_viewcos=0, ctx=None):
    """Batched, HBM-resident line_project_frustum; all d_* are device addresses (ints; d_owner / d_inview / d_level / d_viewcos may be
    0).  d_nq[f] > qstride: more map lines in view than rows (the first qstride are written)."""
    ctx = ctx or default_context()
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    _check(lib().pslfe_line_project_frustum_device(
        ctx._h, C.c_int(nframes), C.c_void_p(d_Tcw), C.c_void_p(d_ml), C.c_void_p(d_mldesc), C.c_void_p(d_nml), C.c_int(mlstride),
        _ptr(cam), C.c_float(log_scale_factor), C.c_float(view_cos_limit), C.c_float(th), *[C.c_float(b) for b in bounds],
        C.c_void_p(d_queries), C.c_void_p(d_qdesc), C.c_void_p(d_owner or None), C.c_void_p(d_nq), C.c_int(qstride),
        C.c_void_p(d_inview or None), C.c_void_p(d_level or None), C.c_void_p(d_viewcos or None)), "pslfe_line_project_frustum_device")


def line_project_last(kls_last, ldesc_last, lines, mldesc, Tcw, cam, th, bounds, ctx=None):
    """LSDmatcher::SearchByProjection(CurrentFrame, LastFrame, th) add_src/LSDmatcher.cpp:112-155 up to the window search: the last
    frame's keylines / LBD rows and LASTLINE_DTYPE[n] (mvpMapLines, outliers), mldesc [n, 32] or None.
    -> (queries LINEQUERY_DTYPE, qdesc, owner)."""
    ctx = ctx or default_context()
    k = np.ascontiguousarray(kls_last, KEYLINE_DTYPE)
    d = np.ascontiguousarray(ldesc_last, np.uint8).reshape(-1, 32)
    L = np.ascontiguousarray(lines, LASTLINE_DTYPE)
    md = None if mldesc is None else np.ascontiguousarray(mldesc, np.uint8).reshape(-1, 32)
    T = np.ascontiguousarray(Tcw, POSE_DTYPE).reshape(1)
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    n = len(k)
    q = np.zeros(max(n, 1), LINEQUERY_DTYPE)
    qd = np.zeros((max(n, 1), 32), np.uint8)
    ow = np.zeros(max(n, 1), np.int32)
    nq = C.c_int()
    _check(lib().pslfe_line_project_last(ctx._h, _ptr(k), _ptr(d), C.c_int(n), _ptr(L), _ptr(md), _ptr(T), _ptr(cam), C.c_float(th),
                                         *[C.c_float(b) for b in bounds], _ptr(q), _ptr(qd), _ptr(ow), C.byref(nq), C.c_int(n)),
           "pslfe_line_project_last")
    m = nq.value
    return q[:m], qd[:m], ow[:m]


def line_project_last_device(npairs, d_kls_last, d_ldesc_last, d_nkl_last, kl_stride, d_lines, d_mldesc, d_Tcw, cam, th, bounds,
                             d_queries, d_qdesc, d_owner, d_nq, qstride, ctx=None):
    """Batched, HBM-resident line_project_last; all d_* are device addresses (ints; d_mldesc / d_owner may be 0)."""
    ctx = ctx or default_context()
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    _check(lib().pslfe_line_project_last_device(
        ctx._h, C.c_int(npairs), C.c_void_p(d_kls_last), C.c_void_p(d_ldesc_last), C.c_void_p(d_nkl_last), C.c_int(kl_stride),
        C.c_void_p(d_lines), C.c_void_p(d_mldesc or None), C.c_void_p(d_Tcw), _ptr(cam), C.c_float(th), *[C.c_float(b) for b in bounds],
        C.c_void_p(d_queries), C.c_void_p(d_qdesc), C.c_void_p(d_owner or None), C.c_void_p(d_nq), C.c_int(qstride)),
        "pslfe_line_project_last_device")


def line_search_by_projection_device(npairs, d_kls, d_desc, d_lineEq, d_nkl, kl_stride, d_lines3d, lines3d_stride, bounds, d_queries,
                                     d_qdesc, d_nq, qstride, d_taken, mode, nnratio, d_match, d_assigned, d_nmatches, d_nfallback=0,
                                     ctx=None):
    """Batched, HBM-resident LSDmatcher::SearchByProjection (mode 0 / 1) on pairs of HBM-resident frames; all d_* are device addresses
    (ints; d_lines3d in mode 0, d_taken, d_assigned and d_nfallback may be 0).  bounds = (mnMinX, mnMinY, mnMaxX, mnMaxY)."""
    ctx = ctx or default_context()
    _check(lib().pslfe_line_search_by_projection_device(
        ctx._h, C.c_int(npairs), C.c_void_p(d_kls), C.c_void_p(d_desc), C.c_void_p(d_lineEq), C.c_void_p(d_nkl), C.c_int(kl_stride),
        C.c_void_p(d_lines3d or None), C.c_int(lines3d_stride), *[C.c_float(b) for b in bounds], C.c_void_p(d_queries),
        C.c_void_p(d_qdesc), C.c_void_p(d_nq), C.c_int(qstride), C.c_void_p(d_taken or None), C.c_int(mode), C.c_float(nnratio),
        C.c_void_p(d_match), C.c_void_p(d_assigned or None), C.c_void_p(d_nmatches), C.c_void_p(d_nfallback or None)),
        "pslfe_line_search_by_projection_device")


class FrameGlue:
    """== the part of Frame::ExtractLSD after the extractor (src/Frame.cc:490-660): isLineGood (3-D RANSAC per keyline),
    convertFansToKeyLines (3-D crossing of paired lines) and the plane-from-pair loop.  `seed`: srand(seed) of the frame."""

    def __init__(self, max_lines=1024, max_fans=4096, max_batch=1, ctx=None):
        self.ctx = ctx or default_context()
        self.max_lines, self.max_fans, self.max_batch = max_lines, max_fans, max_batch
        self._h = C.c_void_p()
        _check(lib().pslfe_glue_create(self.ctx._h, C.c_int(max_lines), C.c_int(max_fans), C.c_int(max_batch), C.byref(self._h)),
               "pslfe_glue_create")

    def run(self, keylines, fans, depth, cam, seed=1, depth_stride=None):
        """depth: the [height][width] f32 image.  depth_stride=None copies it to tight rows; depth_stride=s passes it as it lies in
        memory: it must then be the first `width` columns of a C-contiguous f32 buffer [height][s] (buf[:, :width]), padding included."""
        kls = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
        fans = np.ascontiguousarray(fans, np.float32).reshape(-1, 4)
        if depth_stride is None:
            depth = np.ascontiguousarray(depth, np.float32)
            depth_stride = depth.shape[1]
        elif depth.dtype != np.float32 or depth.ndim != 2 or depth.strides != (4 * depth_stride, 4) or depth.base is None or \
                depth.base.shape != (depth.shape[0], depth_stride) or not depth.base.flags.c_contiguous:
            raise PslfeError(f"FrameGlue.run: depth is not the first columns of a contiguous f32 buffer with rows of {depth_stride} floats")
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        self._n = len(kls)
        _check(lib().pslfe_glue_run(self._h, _ptr(kls), C.c_int(len(kls)), _ptr(fans), C.c_int(len(fans)), _ptr(depth),
                                    C.c_int(depth.shape[1]), C.c_int(depth.shape[0]), C.c_int(depth_stride), _ptr(cam),
                                    C.c_uint32(seed)), "pslfe_glue_run")
        return self.fetch(0, self._n)

    def run_batch_device(self, nframes, d_kls, kl_stride, d_nkl, d_fans, fan_stride, d_nfans, d_depth, width, height, cam, seed0=1):
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
        _check(lib().pslfe_glue_run_batch_device(self._h, C.c_int(nframes), C.c_void_p(int(d_kls)), C.c_int(kl_stride),
                                                 C.c_void_p(int(d_nkl)), C.c_void_p(int(d_fans)), C.c_int(fan_stride),
                                                 C.c_void_p(int(d_nfans)), C.c_void_p(int(d_depth)), C.c_int(width), C.c_int(height),
                                                 _ptr(cam), C.c_uint32(seed0)), "pslfe_glue_run_batch_device")

    def lines3d_device(self):
        """(device address of mvLines3D [max_batch][stride][6] f64, stride = max_lines) of the last batch."""
        d, st = C.c_void_p(), C.c_int()
        _check(lib().pslfe_glue_lines3d_device(self._h, C.byref(d), C.byref(st)), "pslfe_glue_lines3d_device")
        return d.value, st.value

    def lil_obs_device(self):
        """Device view of the last batch's mvle_l and CrossPoint_2D -> dict(le_l, le_stride, ncross, cross2d, plane_stride, nplanes):
        le_l [max_batch][le_stride][6] f64 (one row per crossing), cross2d [max_batch][plane_stride][2] f64 (one row per plane)."""
        le, c2, nc, npl, ls, ps = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(), C.c_int()
        _check(lib().pslfe_glue_lil_obs_device(self._h, C.byref(le), C.byref(ls), C.byref(nc), C.byref(c2), C.byref(ps), C.byref(npl)),
               "pslfe_glue_lil_obs_device")
        return dict(le_l=le.value, le_stride=ls.value, ncross=nc.value, cross2d=c2.value, plane_stride=ps.value, nplanes=npl.value)

    def fetch(self, frame, nlines):
        """dict with mvLines3D, mvLineEq, the crossings (pair, xy, cross, le_l) and the planes."""
        I = P = self.max_fans
        out = dict(lines3d=np.zeros((nlines, 6), np.float64), lineEq=np.zeros((nlines, 3), np.float32),
                   pair=np.zeros((I, 2), np.int32), xy=np.zeros((I, 2), np.float32), cross=np.zeros((I, 3), np.float64),
                   le_l=np.zeros((I, 6), np.float64), planes=np.zeros((P, 4), np.float32), normals=np.zeros((P, 3), np.float64),
                   lineNo=np.zeros((P, 2), np.int32), cross3d=np.zeros((P, 3), np.float64), cross2d=np.zeros((P, 2), np.float64))
        ni, npl = C.c_int(), C.c_int()
        _check(lib().pslfe_glue_fetch(self._h, C.c_int(frame), C.c_int(nlines), _ptr(out["lines3d"]), _ptr(out["lineEq"]), _ptr(out["pair"]),
                                      _ptr(out["xy"]), _ptr(out["cross"]), _ptr(out["le_l"]), C.c_int(I), C.byref(ni), _ptr(out["planes"]),
                                      _ptr(out["normals"]), _ptr(out["lineNo"]), _ptr(out["cross3d"]), _ptr(out["cross2d"]), C.c_int(P),
                                      C.byref(npl)), "pslfe_glue_fetch")
        for k in ("pair", "xy", "cross", "le_l"):
            out[k] = out[k][:ni.value]
        for k in ("planes", "normals", "lineNo", "cross3d", "cross2d"):
            out[k] = out[k][:npl.value]
        return out

    def close(self):
        if self._h:
            lib().pslfe_glue_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ORBVocabulary:
    """== DBoW2 ORBVocabulary as far as Frame::ComputeBoW needs it: transform(descriptors, BowVector, FeatureVector, levelsup).
    Built from flat arrays (the host keeps parsing ORBvoc.txt): children[i] = list of child node ids of node i (node 0 = root),
    node_desc (nnodes x 32 u8), node_weight (f64), node_word (i32), L = depth."""

    def __init__(self, children, node_desc, node_weight, node_word, L, ctx=None):
        self.ctx = ctx or default_context()
        nn = len(children)
        cb = np.zeros(nn, np.int32)
        cc = np.array([len(c) for c in children], np.int32)
        cb[1:] = np.cumsum(cc)[:-1]
        ids = np.array([x for c in children for x in c], np.int32)
        self.arrays = (cb, cc, ids, np.ascontiguousarray(node_desc, np.uint8), np.ascontiguousarray(node_weight, np.float64),
                       np.ascontiguousarray(node_word, np.int32), int(L))
        self._h = C.c_void_p()
        _check(lib().pslfe_vocab_create(self.ctx._h, C.c_int(nn), _ptr(cb), _ptr(cc), _ptr(ids), C.c_int(len(ids)), _ptr(self.arrays[3]),
                                        _ptr(self.arrays[4]), _ptr(self.arrays[5]), C.c_int(L), C.byref(self._h)), "pslfe_vocab_create")

    def transform(self, desc, levelsup=4):
        """-> dict(word, weight, nid per feature; bow_id, bow_val; fv_node, fv_start, fv_idx)"""
        desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(desc)
        m = max(n, 1)
        o = dict(word=np.zeros(m, np.int32), weight=np.zeros(m, np.float64), nid=np.zeros(m, np.int32), bow_id=np.zeros(m, np.int32),
                 bow_val=np.zeros(m, np.float64), fv_node=np.zeros(m, np.int32), fv_start=np.zeros(m + 1, np.int32), fv_idx=np.zeros(m, np.int32))
        nb, nf = C.c_int(), C.c_int()
        _check(lib().pslfe_compute_bow(self._h, _ptr(desc), C.c_int(n), C.c_int(levelsup), _ptr(o["word"]), _ptr(o["weight"]), _ptr(o["nid"]),
                                       _ptr(o["bow_id"]), _ptr(o["bow_val"]), C.byref(nb), _ptr(o["fv_node"]), _ptr(o["fv_start"]),
                                       _ptr(o["fv_idx"]), C.byref(nf)), "pslfe_compute_bow")
        for k in ("word", "weight", "nid"):
            o[k] = o[k][:n]
        o["bow_id"], o["bow_val"] = o["bow_id"][:nb.value], o["bow_val"][:nb.value]
        o["fv_node"], o["fv_start"] = o["fv_node"][:nf.value], o["fv_start"][:nf.value + 1]
        o["fv_idx"] = o["fv_idx"][:int(o["fv_start"][nf.value])] if nf.value else o["fv_idx"][:0]
        return o

    def close(self):
        if self._h:
            lib().pslfe_vocab_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KeyFrameDatabase:
    """== KeyFrameDatabase (src/KeyFrameDatabase.cc) on resident BowVectors (pslfe_kfdb).  A keyframe is a slot
    0 .. max_keyframes-1; a BowVector is a pair (bow_id ascending int32, bow_val float64), e.g. ORBVocabulary.transform's.  The
    device gives words / first_word / score per slot; the covisibility tails of the reference run here as written, on the
    caller's graph: connected_slots = pKF->GetConnectedKeyFrames(), neighbours[slot] = that keyframe's
    GetBestCovisibilityKeyFrames(10) as slots (a dict or a sequence; a missing entry is an empty list).
    mLoopScore / mRelocScore are kept per slot between queries, written only when the slot is scored; they are 0.0f after add
    (the reference leaves them uninitialised, src/KeyFrame.cc:35)."""

    def __init__(self, max_keyframes, max_words=4096, ctx=None):
        self.ctx = ctx or default_context()
        self.max_keyframes, self.max_words = int(max_keyframes), int(max_words)
        self._h = C.c_void_p()
        _check(lib().pslfe_kfdb_create(self.ctx._h, C.c_int(max_keyframes), C.c_int(max_words), C.byref(self._h)), "pslfe_kfdb_create")
        self.mLoopScore = np.zeros(self.max_keyframes, np.float32)
        self.mRelocScore = np.zeros(self.max_keyframes, np.float32)

    @staticmethod
    def _bow(bow):
        ids, vals = np.ascontiguousarray(bow[0], np.int32), np.ascontiguousarray(bow[1], np.float64)
        if ids.ndim != 1 or ids.shape != vals.shape:
            raise PslfeError("KeyFrameDatabase: a BowVector is a pair of equally long 1-D arrays (ids, values)")
        return ids, vals

    def add(self, slot, bow):
        ids, vals = self._bow(bow)
        _check(lib().pslfe_kfdb_add(self._h, C.c_int(slot), _ptr(ids), _ptr(vals), C.c_int(len(ids))), "pslfe_kfdb_add")
        self.mLoopScore[slot] = self.mRelocScore[slot] = 0.0

    def add_device(self, slot0, d_bow_id, d_bow_val, d_nbow, nframes, stride):
        """the BowVectors of a pslfe_compute_bow_device result (device addresses) -> slots slot0 .. slot0 + nframes - 1"""
        _check(lib().pslfe_kfdb_add_device(self._h, C.c_int(slot0), C.c_void_p(d_bow_id), C.c_void_p(d_bow_val), C.c_void_p(d_nbow), C.c_int(nframes),
                                           C.c_int(stride)), "pslfe_kfdb_add_device")
        self.mLoopScore[slot0:slot0 + nframes] = 0.0
        self.mRelocScore[slot0:slot0 + nframes] = 0.0

    def erase(self, slot):
        _check(lib().pslfe_kfdb_erase(self._h, C.c_int(slot)), "pslfe_kfdb_erase")

    def clear(self):
        _check(lib().pslfe_kfdb_clear(self._h), "pslfe_kfdb_clear")

    def state(self):
        """-> live (u8 per slot), seq (add-sequence number per slot, -1 for a dead one)"""
        live, seq = np.zeros(self.max_keyframes, np.uint8), np.zeros(self.max_keyframes, np.int64)
        _check(lib().pslfe_kfdb_state(self._h, _ptr(live), _ptr(seq)), "pslfe_kfdb_state")
        return live, seq

    def query(self, bow, exclude=None):
        """-> words, first_word, score (per slot), max_common; exclude: None or one byte per slot"""
        ids, vals = self._bow(bow)
        if exclude is not None:
            exclude = np.ascontiguousarray(exclude, np.uint8)
            if exclude.shape != (self.max_keyframes,):
                raise PslfeError("KeyFrameDatabase.query: exclude needs one byte per slot")
        K = self.max_keyframes
        words, first, score, maxc = np.zeros(K, np.int32), np.zeros(K, np.int32), np.zeros(K, np.float64), C.c_int()
        _check(lib().pslfe_kfdb_query(self._h, _ptr(ids), _ptr(vals), C.c_int(len(ids)), _ptr(exclude), _ptr(words), _ptr(first), _ptr(score),
                                      C.byref(maxc)), "pslfe_kfdb_query")
        return words, first, score, maxc.value

    def query_device(self, d_bow_id, d_bow_val, d_nbow, nq, stride, d_exclude, d_words, d_first_word, d_score, d_max_common):
        """nq queries in one launch on device addresses (d_exclude may be None); asynchronous"""
        _check(lib().pslfe_kfdb_query_device(self._h, C.c_void_p(d_bow_id), C.c_void_p(d_bow_val), C.c_void_p(d_nbow), C.c_int(nq), C.c_int(stride),
                                             C.c_void_p(d_exclude), C.c_void_p(d_words), C.c_void_p(d_first_word), C.c_void_p(d_score),
                                             C.c_void_p(d_max_common)), "pslfe_kfdb_query_device")

    def Score(self, bow, slots):
        """mpORBVocabulary->score(bow, mBowVec of each slot) -> float64 (the minScore loop of LoopClosing::DetectLoop narrows to float)"""
        ids, vals = self._bow(bow)
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        out = np.zeros(len(slots), np.float64)
        _check(lib().pslfe_kfdb_score(self._h, _ptr(ids), _ptr(vals), C.c_int(len(ids)), _ptr(slots), C.c_int(len(slots)), _ptr(out)),
               "pslfe_kfdb_score")
        return out

    def _sharing(self, bow, exclude):
        """the query, lKFsSharingWords as slots in the reference's order, and minCommonWords"""
        words, first, score, maxc = self.query(bow, exclude)
        _, seq = self.state()
        sharing = np.flatnonzero(words > 0)
        sharing = sharing[np.lexsort((seq[sharing], first[sharing]))]
        return words, score, [int(s) for s in sharing], int(np.float32(maxc) * np.float32(0.8))

    @staticmethod
    def _neigh(neighbours, slot):
        if isinstance(neighbours, dict):
            return neighbours.get(slot, ())
        return neighbours[slot] if slot < len(neighbours) else ()

    @staticmethod
    def _retain(acc, best_acc):
        keep = np.float32(np.float32(0.75) * best_acc)
        out, added = [], set()
        for a, s in acc:
            if a > keep and s not in added:
                out.append(s)
                added.add(s)
        return out

    def DetectLoopCandidates(self, bow, connected_slots, min_score, neighbours):
        """== KeyFrameDatabase::DetectLoopCandidates(pKF, minScore) src/KeyFrameDatabase.cc:76-197 -> candidate slots, in its order"""
        exclude = np.zeros(self.max_keyframes, np.uint8)
        exclude[np.asarray(list(connected_slots), np.int64)] = 1
        min_score = np.float32(min_score)
        words, score, sharing, min_common = self._sharing(bow, exclude)
        scored = []
        for s in sharing:
            if words[s] > min_common:
                si = np.float32(score[s])
                self.mLoopScore[s] = si
                if si >= min_score:
                    scored.append((si, s))
        if not scored:
            return []
        acc, best_acc = [], min_score
        for si, s in scored:
            best_score, acc_score, best = si, si, s
            for s2 in self._neigh(neighbours, s):
                if words[s2] > 0 and words[s2] > min_common:   # reached by this query (never a connected one) and scored
                    acc_score = np.float32(acc_score + self.mLoopScore[s2])
                    if self.mLoopScore[s2] > best_score:
                        best, best_score = int(s2), self.mLoopScore[s2]
            acc.append((acc_score, best))
            if acc_score > best_acc:
                best_acc = acc_score
        return self._retain(acc, best_acc)

    def DetectRelocalizationCandidates(self, bow, neighbours):
        """== KeyFrameDatabase::DetectRelocalizationCandidates(F) src/KeyFrameDatabase.cc:199-309 -> candidate slots, in its order"""
        words, score, sharing, min_common = self._sharing(bow, None)
        scored = []
        for s in sharing:
            if words[s] > min_common:
                si = np.float32(score[s])
                self.mRelocScore[s] = si
                scored.append((si, s))
        if not scored:
            return []
        acc, best_acc = [], np.float32(0)
        for si, s in scored:
            best_score, acc_score, best = si, si, s
            for s2 in self._neigh(neighbours, s):
                if words[s2] <= 0:   # mnRelocQuery != F->mnId; no minCommonWords test here (:273-281): mRelocScore may be an earlier query's
                    continue
                acc_score = np.float32(acc_score + self.mRelocScore[s2])
                if self.mRelocScore[s2] > best_score:
                    best, best_score = int(s2), self.mRelocScore[s2]
            acc.append((acc_score, best))
            if acc_score > best_acc:
                best_acc = acc_score
        return self._retain(acc, best_acc)

    def close(self):
        if self._h:
            lib().pslfe_kfdb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


TRIQUERY_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("stereo", "<i4")])
LINEFUSEQUERY_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("radius", "<f4"), ("level", "<i4")])
assert TRIQUERY_DTYPE.itemsize == 24 and LINEFUSEQUERY_DTYPE.itemsize == 24
# PslKfView: a keyframe as the device projection of map points sees it (include/pslfe.h)
KFVIEW_DTYPE = np.dtype([("Tcw", POSE_DTYPE), ("T21", POSE_DTYPE), ("slot", "<i4")])
assert KFVIEW_DTYPE.itemsize == 100
KF_PROJ_FUSE, KF_PROJ_SCW, KF_PROJ_SIM3 = 0, 1, 2
# the PODs of CreateNewMapPoints / CreateNewMapLines2 (include/pslfe.h): PslTriKeyFrame, PslTriNeighbour, PslNewMapPoint, PslNewMapLine
TRIKEYFRAME_DTYPE = np.dtype([("Tcw", POSE_DTYPE)] + [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "mb", "mbf", "ratio_factor")] + [("kf", "<i4")])
TRINEIGHBOUR_DTYPE = np.dtype([("active", "<i4"), ("slot", "<i4"), ("kf", "<i4"), ("kf_first", "<i4"), ("F12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4"),
                               ("Tcw", POSE_DTYPE)] + [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "mb")])
NEWMAPPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("k", "<i4"), ("idx1", "<i4"), ("idx2", "<i4")])
NEWMAPLINE_DTYPE = np.dtype([("sp", "<f4", (3,)), ("ep", "<f4", (3,)), ("k", "<i4"), ("idx1", "<i4"), ("idx2", "<i4")])
assert (TRIKEYFRAME_DTYPE.itemsize, TRINEIGHBOUR_DTYPE.itemsize, NEWMAPPOINT_DTYPE.itemsize, NEWMAPLINE_DTYPE.itemsize) == (80, 128, 24, 36)
TRI_MAX_NEIGHBOURS = 32
TRI_STATUS = ("CREATED", "NO_MATCH", "TAKEN", "INACTIVE", "W_ZERO", "UNPROJECT_EMPTY", "LOW_PARALLAX", "DEPTH1", "DEPTH2", "REPROJ1_MONO",
              "REPROJ1_STEREO", "REPROJ2_MONO", "REPROJ2_STEREO", "DIST_ZERO", "RATIO")                      # PSL_TRI_*
TRIL_STATUS = ("CREATED", "NO_MATCH", "TAKEN", "INACTIVE", "IDX2_RANGE", "NO_STEREO", "DEPTH_SP1", "DEPTH_EP1", "DEPTH_SP2", "DEPTH_EP2",
               "REPROJ_SP1", "REPROJ_EP1", "REPROJ_SP2", "REPROJ_EP2", "DIST_ZERO", "RATIO")                # PSL_TRIL_*
UPKEEP_SUM_WALK, UPKEEP_SUM_TILED = 0, 1   # PSLFE_UPKEEP_SUM_*: KeyFrameMatcher.set_upkeep_sum


def _proj_args(cam, bounds, scale_factors, log_scale_factor, th):
    """cam, bounds, scale_factors, nlevels, log_scale_factor, th as the pslfe_kf_* projections take them (keeps the arrays alive)"""
    cam = np.ascontiguousarray(cam, CAMERA_DTYPE).reshape(1)
    sf = np.ascontiguousarray(scale_factors, np.float32)
    return cam, sf, (_ptr(cam), *[C.c_float(b) for b in bounds], _ptr(sf)), (C.c_int(len(sf)), C.c_float(log_scale_factor), C.c_float(th))


class KeyFrameMatcher:
    """The KeyFrame-rate searches of LocalMapping / LoopClosing (pslfe_kf): ORBmatcher::Fuse (both), SearchBySim3,
    SearchForTriangulation (src/ORBmatcher.cc:657-1326), SearchByBoW(pKF1, pKF2) and SearchByProjection(pKF, Scw, ...) of
    LoopClosing::ComputeSim3 (src/ORBmatcher.cc:290-403, 522-655), LSDmatcher::Fuse / SearchForTriangulation
    (add_src/LSDmatcher.cpp:705-984) and Map{Point,Line}::ComputeDistinctiveDescriptors, from the point where the host has
    projected its map points.  Give each host thread its own Context + KeyFrameMatcher."""

    TH_HIGH, TH_LOW = 100, 50

    def __init__(self, ctx=None):
        self.ctx = ctx or default_context()
        self._h = C.c_void_p()
        _check(lib().pslfe_kf_create(self.ctx._h, C.byref(self._h)), "pslfe_kf_create")

    def window_best(self, frame, slot, queries, qdesc, chi2=False, inv_level_sigma2=None):
        """Candidate loop of Fuse / SearchBySim3 -> (best_idx, best_dist) per projected map point."""
        q = np.ascontiguousarray(queries, PROJQUERY_DTYPE)
        qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        nq = len(q)
        bi = np.full(max(nq, 1), -1, np.int32)
        bd = np.full(max(nq, 1), 0x7fffffff, np.int32)
        s2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        _check(lib().pslfe_kf_window_best(self._h, frame._h, C.c_int(slot), _ptr(q), _ptr(qd), C.c_int(nq), C.c_int(1 if chi2 else 0),
                                          _ptr(s2), C.c_int(0 if s2 is None else len(s2)), _ptr(bi), _ptr(bd)), "pslfe_kf_window_best")
        return bi[:nq], bd[:nq]

    def Fuse(self, frame, slot, queries, qdesc, inv_level_sigma2):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) src/ORBmatcher.cc:825: -> (bestIdx, fused) with fused = bestDist <= TH_LOW;
        the caller replaces / adds map points (:950-964)."""
        bi, bd = self.window_best(frame, slot, queries, qdesc, True, inv_level_sigma2)
        return bi, bd <= self.TH_LOW

    def FuseSim3(self, frame, slot, queries, qdesc):
        """ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) src/ORBmatcher.cc:968."""
        bi, bd = self.window_best(frame, slot, queries, qdesc, False)
        return bi, bd <= self.TH_LOW

    def SearchBySim3(self, frame1, slot1, frame2, slot2, q12, qdesc1, q21, qdesc2):
        """src/ORBmatcher.cc:1102 -> (nFound, match12)."""
        q1 = np.ascontiguousarray(q12, PROJQUERY_DTYPE)
        q2 = np.ascontiguousarray(q21, PROJQUERY_DTYPE)
        d1 = np.ascontiguousarray(qdesc1, np.uint8).reshape(-1, 32)
        d2 = np.ascontiguousarray(qdesc2, np.uint8).reshape(-1, 32)
        m = np.full(max(len(q1), 1), -1, np.int32)
        nf = C.c_int()
        _check(lib().pslfe_kf_search_by_sim3(self._h, frame1._h, C.c_int(slot1), frame2._h, C.c_int(slot2), _ptr(q1), _ptr(d1),
                                             C.c_int(len(q1)), _ptr(q2), _ptr(d2), C.c_int(len(q2)), _ptr(m), C.byref(nf)),
               "pslfe_kf_search_by_sim3")
        return nf.value, m[:len(q1)]

    def SearchForTriangulation(self, frame2, slot2, fidx2, taken2, queries, qdesc, F12, epipole, scale_factors, level_sigma2,
                               bOnlyStereo=False, checkOri=True):
        """src/ORBmatcher.cc:657 -> (nmatches, match per query); vMatchedPairs = the matched (idx1, idx2) sorted by idx1."""
        fidx = np.ascontiguousarray(fidx2, np.int32)
        tk = np.ascontiguousarray(taken2, np.uint8)
        q = np.ascontiguousarray(queries, TRIQUERY_DTYPE)
        qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        F = np.ascontiguousarray(F12, np.float32).reshape(9)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        match = np.full(max(len(q), 1), -1, np.int32)
        nm = C.c_int()
        _check(lib().pslfe_kf_search_for_triangulation(self._h, frame2._h, C.c_int(slot2), _ptr(fidx), C.c_int(len(fidx)), _ptr(tk), _ptr(q),
                                                       _ptr(qd), C.c_int(len(q)), _ptr(F), C.c_float(epipole[0]), C.c_float(epipole[1]),
                                                       C.c_int(1 if bOnlyStereo else 0), C.c_int(1 if checkOri else 0), _ptr(sf), _ptr(s2),
                                                       C.c_int(len(sf)), _ptr(match), C.byref(nm)), "pslfe_kf_search_for_triangulation")
        return nm.value, match[:len(q)]

    @staticmethod
    def _bow_queries(runs, qangle, qdesc):
        q = np.zeros(len(runs), BOWQUERY_DTYPE)
        if len(runs):
            r = np.asarray(runs, np.int32).reshape(-1, 2)
            q["start"], q["len"], q["angle"] = r[:, 0], r[:, 1], np.asarray(qangle, np.float32)
        return q, np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)

    def SearchByBoW(self, frame, slot2, fidx2, runs, qangle, qdesc, nnratio=0.75, check_ori=True):
        """SearchByBoW(pKF1, pKF2, vpMatches12) src/ORBmatcher.cc:522: slot2 holds KF2; fidx2 = its FeatureVector flattened in node
        order, features without a good map point left out; runs[i] = (start, len) of query i's node in fidx2; qangle / qdesc per
        KF1 feature with a good map point.  -> (nmatches, match per query)."""
        fidx = np.ascontiguousarray(fidx2, np.int32)
        q, qd = self._bow_queries(runs, qangle, qdesc)
        match = np.full(max(len(q), 1), -1, np.int32)
        nm = C.c_int()
        _check(lib().pslfe_kf_search_by_bow(self._h, frame._h, C.c_int(slot2), _ptr(fidx), C.c_int(len(fidx)), _ptr(q), _ptr(qd),
                                            C.c_int(len(q)), C.c_float(nnratio), C.c_int(1 if check_ori else 0), _ptr(match),
                                            C.byref(nm)), "pslfe_kf_search_by_bow")
        return nm.value, match[:len(q)]

    def SearchByBoWCandidates(self, frame, slots2, fidx2, runs, qangle, qdesc, nnratio=0.75, check_ori=True):
        """The candidate loop of LoopClosing::ComputeSim3 src/LoopClosing.cc:252-284: one list entry per candidate in every argument
        (slots2[c], fidx2[c], runs[c], qangle[c], qdesc[c] as SearchByBoW takes them).  -> (nmatches[c], [match of candidate c])."""
        nc = len(slots2)
        slots = np.ascontiguousarray(slots2, np.int32)
        fl = [np.ascontiguousarray(f, np.int32).reshape(-1) for f in fidx2]
        ql = [self._bow_queries(runs[c], qangle[c], qdesc[c]) for c in range(nc)]
        foff = np.zeros(nc + 1, np.int32)
        qoff = np.zeros(nc + 1, np.int32)
        foff[1:] = np.cumsum([len(f) for f in fl])
        qoff[1:] = np.cumsum([len(q) for q, _ in ql])
        fidx = np.concatenate(fl) if nc else np.zeros(0, np.int32)
        q = np.concatenate([q for q, _ in ql]) if nc else np.zeros(0, BOWQUERY_DTYPE)
        qd = np.concatenate([d for _, d in ql]) if nc else np.zeros((0, 32), np.uint8)
        match = np.full(max(len(q), 1), -1, np.int32)
        nm = np.zeros(max(nc, 1), np.int32)
        _check(lib().pslfe_kf_search_by_bow_candidates(self._h, frame._h, _ptr(slots), C.c_int(nc), _ptr(fidx), _ptr(foff), _ptr(q), _ptr(qd),
                                                       _ptr(qoff), C.c_float(nnratio), C.c_int(1 if check_ori else 0), _ptr(match), _ptr(nm)),
               "pslfe_kf_search_by_bow_candidates")
        return nm[:nc], [match[qoff[c]:qoff[c + 1]] for c in range(nc)]

    def SearchByProjectionSim3(self, frame, slot, queries, qdesc, taken=None):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) src/ORBmatcher.cc:290 after the projection: queries as for
        FuseSim3, taken[idx] = vpMatched[idx] != NULL on entry.  -> (nmatches, match per map point, assigned per keypoint)."""
        q = np.ascontiguousarray(queries, PROJQUERY_DTYPE)
        qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        n = frame.n[slot]
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        if tk is not None and len(tk) != n:
            raise PslfeError(f"SearchByProjectionSim3: taken has {len(tk)} entries, the keyframe {n} keypoints")
        match = np.full(max(len(q), 1), -1, np.int32)
        assigned = np.full(max(n, 1), -1, np.int32)
        nm = C.c_int()
        _check(lib().pslfe_kf_search_by_projection_sim3(self._h, frame._h, C.c_int(slot), _ptr(q), _ptr(qd), C.c_int(len(q)), _ptr(tk),
                                                        _ptr(match), _ptr(assigned), C.byref(nm)), "pslfe_kf_search_by_projection_sim3")
        return nm.value, match[:len(q)], assigned[:n]

    def project(self, mode, views, mp, cam, bounds, scale_factors, log_scale_factor, th, skip=None):
        """pslfe_kf_project: the per-point arithmetic of Fuse (mode KF_PROJ_FUSE), Fuse / SearchByProjection with a decomposed Scw
        (KF_PROJ_SCW) or one direction of SearchBySim3 (KF_PROJ_SIM3) for K keyframes (KFVIEW_DTYPE[K]) x M map points
        (MAPPOINT_DTYPE[M]); skip [K, M] bytes or None.  -> (rows PROJQUERY_DTYPE [K, M], level [K, M])."""
        v = np.ascontiguousarray(views, KFVIEW_DTYPE).reshape(-1)
        g = np.ascontiguousarray(mp, MAPPOINT_DTYPE).reshape(-1)
        K, M = len(v), len(g)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, M)
        cam, sf, a, b = _proj_args(cam, bounds, scale_factors, log_scale_factor, th)
        q = np.zeros((K, M), PROJQUERY_DTYPE)
        lvl = np.full((K, M), -1, np.int32)
        _check(lib().pslfe_kf_project(self._h, C.c_int(mode), _ptr(v), C.c_int(K), _ptr(g), _ptr(sk), C.c_int(M), *a, *b, _ptr(q), _ptr(lvl)),
               "pslfe_kf_project")
        return q, lvl

    def FuseKeyFrames(self, frame, mode, views, mp, mpdesc, cam, bounds, scale_factors, log_scale_factor, th, inv_level_sigma2=None,
                      skip=None):
        """ORBmatcher::Fuse(pKF, vpMapPoints, th) (mode KF_PROJ_FUSE, needs inv_level_sigma2) or Fuse(pKF, Scw, ...) (KF_PROJ_SCW) up to
        bestDist for the K keyframes views[k]["slot"] of `frame` against the same M map points, projection included.
        -> (bestIdx [K, M], bestDist [K, M], rows [K, M]); fused = bestDist <= TH_LOW, the caller mutates the map."""
        v = np.ascontiguousarray(views, KFVIEW_DTYPE).reshape(-1)
        g = np.ascontiguousarray(mp, MAPPOINT_DTYPE).reshape(-1)
        K, M = len(v), len(g)
        d = np.ascontiguousarray(mpdesc, np.uint8).reshape(M, 32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, M)
        s2 = None if inv_level_sigma2 is None else np.ascontiguousarray(inv_level_sigma2, np.float32)
        cam, sf, a, b = _proj_args(cam, bounds, scale_factors, log_scale_factor, th)
        if s2 is not None and len(s2) != len(sf):
            raise PslfeError(f"FuseKeyFrames: {len(s2)} inverse sigmas for {len(sf)} levels")
        bi = np.full((K, M), -1, np.int32)
        bd = np.full((K, M), 0x7fffffff, np.int32)
        q = np.zeros((K, M), PROJQUERY_DTYPE)
        _check(lib().pslfe_kf_fuse_keyframes(self._h, frame._h, C.c_int(mode), _ptr(v), C.c_int(K), _ptr(g), _ptr(d), _ptr(sk), C.c_int(M), *a,
                                             _ptr(s2), *b, _ptr(bi), _ptr(bd), _ptr(q)), "pslfe_kf_fuse_keyframes")
        return bi, bd, q

    def SearchBySim3Poses(self, frame1, frame2, view12, mp1, desc1, skip1, view21, mp2, desc2, skip2, cam, bounds, scale_factors,
                          log_scale_factor, th):
        """ORBmatcher::SearchBySim3 src/ORBmatcher.cc:1102 with both projections on the device.  view12: R1w, t1w / sR21, t21 / KF2's slot
        in frame2; view21: R2w, t2w / sR12, t12 / KF1's slot in frame1; mp / desc / skip per entry of GetMapPointMatches().
        -> (nFound, match12, rows12, rows21)."""
        v12 = np.ascontiguousarray(view12, KFVIEW_DTYPE).reshape(1)
        v21 = np.ascontiguousarray(view21, KFVIEW_DTYPE).reshape(1)
        g1, g2 = np.ascontiguousarray(mp1, MAPPOINT_DTYPE).reshape(-1), np.ascontiguousarray(mp2, MAPPOINT_DTYPE).reshape(-1)
        n1, n2 = len(g1), len(g2)
        d1, d2 = np.ascontiguousarray(desc1, np.uint8).reshape(n1, 32), np.ascontiguousarray(desc2, np.uint8).reshape(n2, 32)
        s1 = None if skip1 is None else np.ascontiguousarray(skip1, np.uint8).reshape(n1)
        s2 = None if skip2 is None else np.ascontiguousarray(skip2, np.uint8).reshape(n2)
        cam, sf, a, b = _proj_args(cam, bounds, scale_factors, log_scale_factor, th)
        m = np.full(max(n1, 1), -1, np.int32)
        q12, q21 = np.zeros(max(n1, 1), PROJQUERY_DTYPE), np.zeros(max(n2, 1), PROJQUERY_DTYPE)
        nf = C.c_int()
        _check(lib().pslfe_kf_search_by_sim3_poses(self._h, frame1._h, frame2._h, _ptr(v12), _ptr(g1), _ptr(d1), _ptr(s1), C.c_int(n1), _ptr(v21),
                                                   _ptr(g2), _ptr(d2), _ptr(s2), C.c_int(n2), *a, *b, _ptr(m), C.byref(nf), _ptr(q12), _ptr(q21)),
               "pslfe_kf_search_by_sim3_poses")
        return nf.value, m[:n1], q12[:n1], q21[:n2]

    def SearchByProjectionSim3Pose(self, frame, view, mp, mpdesc, cam, bounds, scale_factors, log_scale_factor, th, skip=None, taken=None):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) src/ORBmatcher.cc:290 from :312 on, projection included: view = the
        decomposed Scw and the keyframe's slot.  -> (nmatches, match per map point, assigned per keypoint, rows)."""
        v = np.ascontiguousarray(view, KFVIEW_DTYPE).reshape(1)
        g = np.ascontiguousarray(mp, MAPPOINT_DTYPE).reshape(-1)
        M = len(g)
        d = np.ascontiguousarray(mpdesc, np.uint8).reshape(M, 32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(M)
        n = frame.n[int(v["slot"][0])]
        tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
        if tk is not None and len(tk) != n:
            raise PslfeError(f"SearchByProjectionSim3Pose: taken has {len(tk)} entries, the keyframe {n} keypoints")
        cam, sf, a, b = _proj_args(cam, bounds, scale_factors, log_scale_factor, th)
        match = np.full(max(M, 1), -1, np.int32)
        assigned = np.full(max(n, 1), -1, np.int32)
        q = np.zeros(max(M, 1), PROJQUERY_DTYPE)
        nm = C.c_int()
        _check(lib().pslfe_kf_search_by_projection_sim3_pose(self._h, frame._h, _ptr(v), _ptr(g), _ptr(d), _ptr(sk), C.c_int(M), *a, *b, _ptr(tk),
                                                             _ptr(match), _ptr(assigned), C.byref(nm), _ptr(q)),
               "pslfe_kf_search_by_projection_sim3_pose")
        return nm.value, match[:M], assigned[:n], q[:M]

    def LineFuse(self, keylines, desc, queries, qdesc):
        """Search of LSDmatcher::Fuse add_src/LSDmatcher.cpp:933-958 -> (bestIdx, bestDist)."""
        kl = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        q = np.ascontiguousarray(queries, LINEFUSEQUERY_DTYPE)
        qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
        bi = np.full(max(len(q), 1), -1, np.int32)
        bd = np.full(max(len(q), 1), 256, np.int32)
        _check(lib().pslfe_kf_line_fuse_best(self._h, _ptr(kl), C.c_int(len(kl)), _ptr(d), C.c_int(len(d)), _ptr(q), _ptr(qd), C.c_int(len(q)),
                                             _ptr(bi), _ptr(bd)), "pslfe_kf_line_fuse_best")
        return bi[:len(q)], bd[:len(q)]

    def line_project(self, poses, ml, cam, bounds, scale_factors_line, log_scale_factor_line, th, skip=None):
        """pslfe_kf_line_project: the per-line arithmetic of LSDmatcher::Fuse add_src/LSDmatcher.cpp:865-931 for K keyframe poses
        (POSE_DTYPE[K]) x M map lines (MAPLINE_DTYPE[M]); skip [K, M] bytes or None.
        -> (rows LINEFUSEQUERY_DTYPE [K, M], level [K, M], stop [K]): rows i >= stop[k] are dropped, the reference returned there."""
        T = np.ascontiguousarray(poses, POSE_DTYPE).reshape(-1)
        g = np.ascontiguousarray(ml, MAPLINE_DTYPE).reshape(-1)
        K, M = len(T), len(g)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, M)
        cam, sf, a, b = _proj_args(cam, bounds, scale_factors_line, log_scale_factor_line, th)
        q = np.zeros((K, M), LINEFUSEQUERY_DTYPE)
        lvl = np.full((K, M), -2**31, np.int32)
        stop = np.full(K, M, np.int32)
        _check(lib().pslfe_kf_line_project(self._h, _ptr(T), C.c_int(K), _ptr(g), _ptr(sk), C.c_int(M), *a, *b, _ptr(q), _ptr(lvl), _ptr(stop)),
               "pslfe_kf_line_project")
        return q, lvl, stop

    def LineFuseKeyFrames(self, poses, keylines, descs, ml, mldesc, cam, bounds, scale_factors_line, log_scale_factor_line, th, skip=None):
        """LSDmatcher::Fuse(pKF, vpMapLines, th) add_src/LSDmatcher.cpp:847-958 up to bestDist for K keyframes against the same M map
        lines, projection included: keylines[k] (KEYLINE_DTYPE) and descs[k] (rows x 32, the matrix the reference indexes with the line
        index) per keyframe.  -> (bestIdx [K, M], bestDist [K, M], rows [K, M], stop [K]); fused = bestDist <= TH_LOW for the rows
        i < stop[k], the caller mutates the map and returns 0 for a keyframe with stop[k] < M."""
        T = np.ascontiguousarray(poses, POSE_DTYPE).reshape(-1)
        g = np.ascontiguousarray(ml, MAPLINE_DTYPE).reshape(-1)
        K, M = len(T), len(g)
        if len(keylines) != K or len(descs) != K:
            raise PslfeError(f"LineFuseKeyFrames: {len(keylines)} keyline lists and {len(descs)} descriptor matrices for {K} keyframes")
        kl = [np.ascontiguousarray(x, KEYLINE_DTYPE).reshape(-1) for x in keylines]
        dd = [np.ascontiguousarray(x, np.uint8).reshape(-1, 32) for x in descs]
        koff, doff = np.zeros(K + 1, np.int32), np.zeros(K + 1, np.int32)
        koff[1:], doff[1:] = np.cumsum([len(x) for x in kl]), np.cumsum([len(x) for x in dd])
        kls = np.concatenate(kl) if K else np.zeros(0, KEYLINE_DTYPE)
        desc = np.concatenate(dd) if K else np.zeros((0, 32), np.uint8)
        d = np.ascontiguousarray(mldesc, np.uint8).reshape(M, 32)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(K, M)
        cam, sf, a, b = _proj_args(cam, bounds, scale_factors_line, log_scale_factor_line, th)
        bi = np.full((K, M), -1, np.int32)
        bd = np.full((K, M), 256, np.int32)
        q = np.zeros((K, M), LINEFUSEQUERY_DTYPE)
        stop = np.full(K, M, np.int32)
        _check(lib().pslfe_kf_line_fuse_keyframes(self._h, _ptr(T), C.c_int(K), _ptr(kls), _ptr(koff), _ptr(desc), _ptr(doff), _ptr(g), _ptr(d),
                                                  _ptr(sk), C.c_int(M), *a, *b, _ptr(bi), _ptr(bd), _ptr(q), _ptr(stop)),
               "pslfe_kf_line_fuse_keyframes")
        return bi, bd, q, stop

    def LineSearchForTriangulationKeyFrames(self, ldesc1, ldescs2, has_mapline1, has_maplines2, nnratio, TH, mutual=True):
        """pslfe_kf_line_search_for_triangulation_keyframes (LSDmatcher.SearchForTriangulationKeyFrames is the reference-shaped call)
        -> (nmatches [K], match [K, n1])."""
        d1 = np.ascontiguousarray(ldesc1, np.uint8).reshape(-1, 32)
        K, n1 = len(ldescs2), len(d1)
        dd = [np.ascontiguousarray(x, np.uint8).reshape(-1, 32) for x in ldescs2]
        off = np.zeros(K + 1, np.int32)
        off[1:] = np.cumsum([len(x) for x in dd])
        d2 = np.concatenate(dd) if K else np.zeros((0, 32), np.uint8)
        h1 = None if has_mapline1 is None else np.ascontiguousarray(has_mapline1, np.uint8).reshape(n1)
        h2 = None
        if has_maplines2 is not None:
            h2 = np.concatenate([np.ascontiguousarray(x, np.uint8).reshape(-1) for x in has_maplines2]) if K else np.zeros(0, np.uint8)
            if len(h2) != off[K]:
                raise PslfeError(f"SearchForTriangulationKeyFrames: {len(h2)} GetMapLine bytes for {off[K]} neighbour lines")
        match = np.full((K, n1), -1, np.int32)
        nm = np.zeros(max(K, 1), np.int32)
        _check(lib().pslfe_kf_line_search_for_triangulation_keyframes(self._h, _ptr(d1), C.c_int(n1), _ptr(h1), _ptr(d2), _ptr(off), _ptr(h2),
                                                                      C.c_int(K), C.c_float(nnratio), C.c_float(TH), C.c_int(1 if mutual else 0),
                                                                      _ptr(match), _ptr(nm)),
               "pslfe_kf_line_search_for_triangulation_keyframes")
        return nm[:K], match

    @staticmethod
    def _new_points_args(kf1, keysun1, keys1, uright1, depth1, taken1, neighbours, fidx2, taken2, keys2, depth2, queries, idx1, qdesc,
                         scale_factors, level_sigma2):
        """the host arrays of pslfe_kf_create_new_map_points from per-neighbour lists -> a dict (kept alive by the caller)"""
        a = {"kf1": np.ascontiguousarray(kf1, TRIKEYFRAME_DTYPE).reshape(1), "ku1": np.ascontiguousarray(keysun1, KEYPOINT_DTYPE).reshape(-1)}
        N1 = a["N1"] = len(a["ku1"])
        a["k1"] = np.ascontiguousarray(keys1, np.float32).reshape(N1, 2)
        a["ur1"], a["dp1"] = np.ascontiguousarray(uright1, np.float32).reshape(N1), np.ascontiguousarray(depth1, np.float32).reshape(N1)
        a["tk1"] = np.ascontiguousarray(taken1, np.uint8).reshape(N1)
        a["nb"] = np.ascontiguousarray(neighbours, TRINEIGHBOUR_DTYPE).reshape(-1)
        K = a["K"] = len(a["nb"])
        if not all(len(x) == K for x in (fidx2, taken2, keys2, depth2, queries, idx1, qdesc)):
            raise PslfeError(f"CreateNewMapPoints: the per-neighbour lists do not have {K} entries")
        fl = [np.ascontiguousarray(f, np.int32).reshape(-1) for f in fidx2]
        tl = [np.ascontiguousarray(t, np.uint8).reshape(-1) for t in taken2]
        kl = [np.ascontiguousarray(x, np.float32).reshape(-1, 2) for x in keys2]
        dl = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in depth2]
        if any(len(t) != len(x) or len(t) != len(d) for t, x, d in zip(tl, kl, dl)):
            raise PslfeError("CreateNewMapPoints: taken2, keys2 and depth2 of a neighbour differ in length")
        a["foff"], a["koff"] = np.zeros(K + 1, np.int32), np.zeros(K + 1, np.int32)
        a["foff"][1:], a["koff"][1:] = np.cumsum([len(f) for f in fl]), np.cumsum([len(t) for t in tl])
        a["fidx"] = np.concatenate(fl + [np.zeros(0, np.int32)])
        a["tk2"] = np.concatenate(tl + [np.zeros(0, np.uint8)])
        a["k2"] = np.concatenate(kl + [np.zeros((0, 2), np.float32)])
        a["dp2"] = np.concatenate(dl + [np.zeros(0, np.float32)])
        ql = [np.ascontiguousarray(q, TRIQUERY_DTYPE).reshape(-1) for q in queries]
        a["nq"] = np.array([len(q) for q in ql], np.int32).reshape(K)
        nqmax = a["nqmax"] = int(a["nq"].max()) if K else 0
        a["q"], a["i1"], a["qd"] = np.zeros((K, nqmax), TRIQUERY_DTYPE), np.zeros((K, nqmax), np.int32), np.zeros((K, nqmax, 32), np.uint8)
        for k in range(K):
            n = len(ql[k])
            a["q"][k, :n], a["i1"][k, :n] = ql[k], np.asarray(idx1[k], np.int32).reshape(n)
            a["qd"][k, :n] = np.asarray(qdesc[k], np.uint8).reshape(n, 32)
        a["sf"], a["s2"] = np.ascontiguousarray(scale_factors, np.float32).reshape(-1), np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        if len(a["sf"]) != len(a["s2"]):
            raise PslfeError("CreateNewMapPoints: mvScaleFactors and mvLevelSigma2 differ in length")
        return a

    def CreateNewMapPoints(self, frame2, kf1, keysun1, keys1, uright1, depth1, taken1, neighbours, fidx2, taken2, keys2, depth2, queries, idx1,
                           qdesc, scale_factors, level_sigma2, bOnlyStereo=False, checkOri=False, want_geom=True):
        """LocalMapping::CreateNewMapPoints src/LocalMapping.cc:305-519 for KF1 against K neighbours in one call
        (pslfe_kf_create_new_map_points).  kf1: TRIKEYFRAME_DTYPE; keysun1 (KEYPOINT_DTYPE[N1]) = mvKeysUn, keys1 [N1, 2] = mvKeys[i].pt,
        uright1, depth1, taken1 [N1]; neighbours: TRINEIGHBOUR_DTYPE[K] (slots of frame2); per neighbour k the lists fidx2[k], taken2[k],
        keys2[k], depth2[k] and its query list queries[k] (TRIQUERY_DTYPE), idx1[k], qdesc[k] built from the state at the call.
        -> dict: match, status [K, nqmax], x3d [K, nqmax, 3], nmatches [K], created_by [N1], new (NEWMAPPOINT_DTYPE[nnew], creation order),
        geom (MAPPOINT_DTYPE[nnew], position filled)."""
        a = self._new_points_args(kf1, keysun1, keys1, uright1, depth1, taken1, neighbours, fidx2, taken2, keys2, depth2, queries, idx1, qdesc,
                                  scale_factors, level_sigma2)
        K, N1, nqmax = a["K"], a["N1"], a["nqmax"]
        match, status = np.full((K, nqmax), -1, np.int32), np.full((K, nqmax), 1, np.int32)
        x3d, nm, by = np.zeros((K, nqmax, 3), np.float32), np.zeros(max(K, 1), np.int32), np.full(max(N1, 1), -1, np.int32)
        newp, geom, nnew = np.zeros(max(N1, 1), NEWMAPPOINT_DTYPE), np.zeros(max(N1, 1), MAPPOINT_DTYPE), C.c_int(0)
        _check(lib().pslfe_kf_create_new_map_points(
            self._h, frame2._h, _ptr(a["kf1"]), C.c_int(N1), _ptr(a["ku1"]), _ptr(a["k1"]), _ptr(a["ur1"]), _ptr(a["dp1"]), _ptr(a["tk1"]), _ptr(a["nb"]),
            C.c_int(K), _ptr(a["fidx"]), _ptr(a["foff"]), _ptr(a["tk2"]), _ptr(a["k2"]), _ptr(a["dp2"]), _ptr(a["koff"]), _ptr(a["q"]), _ptr(a["i1"]),
            _ptr(a["qd"]), _ptr(a["nq"]), C.c_int(nqmax), C.c_int(1 if bOnlyStereo else 0), C.c_int(1 if checkOri else 0), _ptr(a["sf"]), _ptr(a["s2"]),
            C.c_int(len(a["sf"])), _ptr(match), _ptr(status), _ptr(x3d), _ptr(nm), _ptr(by), _ptr(newp), C.byref(nnew),
            _ptr(geom) if want_geom else None), "pslfe_kf_create_new_map_points")
        n = nnew.value
        return {"match": match, "status": status, "x3d": x3d, "nmatches": nm[:K], "created_by": by[:N1], "new": newp[:n], "geom": geom[:n]}

    def CreateNewMapPointsDevice(self, frame2, kf1, N1, d_keysun1, d_keys1, d_uright1, d_depth1, d_taken1, neighbours, d_fidx2, fidx_off, d_taken2,
                                 d_keys2, d_depth2, kp_off, d_queries, d_idx1, d_qdesc, nq, nqmax, scale_factors, level_sigma2, d_match, d_status,
                                 d_x3d, d_nmatches, d_created_by, d_newp, d_nnew, d_geom, d_obs_off, d_obs_kf, d_ref_kf, d_ref_level,
                                 bOnlyStereo=False, checkOri=False):
        """The same on device addresses (pslfe_kf_create_new_map_points_device): queued on the context's stream; d_geom and the
        observation runs are what update_normal_and_depth_device takes with M = N1."""
        k1, nb = np.ascontiguousarray(kf1, TRIKEYFRAME_DTYPE).reshape(1), np.ascontiguousarray(neighbours, TRINEIGHBOUR_DTYPE).reshape(-1)
        foff, koff, nqa = (np.ascontiguousarray(x, np.int32).reshape(-1) for x in (fidx_off, kp_off, nq))
        sf, s2 = np.ascontiguousarray(scale_factors, np.float32).reshape(-1), np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        v = lambda d: C.c_void_p(d) if d else None
        _check(lib().pslfe_kf_create_new_map_points_device(
            self._h, frame2._h, _ptr(k1), C.c_int(N1), v(d_keysun1), v(d_keys1), v(d_uright1), v(d_depth1), v(d_taken1), _ptr(nb), C.c_int(len(nb)),
            v(d_fidx2), _ptr(foff), v(d_taken2), v(d_keys2), v(d_depth2), _ptr(koff), v(d_queries), v(d_idx1), v(d_qdesc), _ptr(nqa), C.c_int(nqmax),
            C.c_int(1 if bOnlyStereo else 0), C.c_int(1 if checkOri else 0), _ptr(sf), _ptr(s2), C.c_int(len(sf)), v(d_match), v(d_status), v(d_x3d),
            v(d_nmatches), v(d_created_by), v(d_newp), v(d_nnew), v(d_geom), v(d_obs_off), v(d_obs_kf), v(d_ref_kf), v(d_ref_level)),
            "pslfe_kf_create_new_map_points_device")

    @staticmethod
    def _new_lines_args(kf1, ldesc1, has_mapline1, keylines1, lines3d1, lineeq1, neighbours, ldescs2, has_maplines2, keylines2, lines3d2,
                        scale_factors, level_sigma2):
        a = {"kf1": np.ascontiguousarray(kf1, TRIKEYFRAME_DTYPE).reshape(1), "d1": np.ascontiguousarray(ldesc1, np.uint8).reshape(-1, 32)}
        n1 = a["n1"] = len(a["d1"])
        a["h1"] = None if has_mapline1 is None else np.ascontiguousarray(has_mapline1, np.uint8).reshape(n1)
        a["kl1"] = np.ascontiguousarray(keylines1, KEYLINE_DTYPE).reshape(n1)
        a["l1"], a["eq1"] = np.ascontiguousarray(lines3d1, np.float64).reshape(n1, 6), np.ascontiguousarray(lineeq1, np.float32).reshape(n1)
        a["nb"] = np.ascontiguousarray(neighbours, TRINEIGHBOUR_DTYPE).reshape(-1)
        K = a["K"] = len(a["nb"])
        if not all(len(x) == K for x in (ldescs2, keylines2, lines3d2)) or (has_maplines2 is not None and len(has_maplines2) != K):
            raise PslfeError(f"CreateNewMapLines: the per-neighbour lists do not have {K} entries")
        dd = [np.ascontiguousarray(x, np.uint8).reshape(-1, 32) for x in ldescs2]
        kk = [np.ascontiguousarray(x, KEYLINE_DTYPE).reshape(-1) for x in keylines2]
        ll = [np.ascontiguousarray(x, np.float64).reshape(-1, 6) for x in lines3d2]
        if any(len(d) != len(k) or len(d) != len(l) for d, k, l in zip(dd, kk, ll)):
            raise PslfeError("CreateNewMapLines: descriptors, keylines and 3-D lines of a neighbour differ in length")
        a["off"] = np.zeros(K + 1, np.int32)
        a["off"][1:] = np.cumsum([len(x) for x in dd])
        a["d2"] = np.concatenate(dd + [np.zeros((0, 32), np.uint8)])
        a["kl2"] = np.concatenate(kk + [np.zeros(0, KEYLINE_DTYPE)])
        a["l2"] = np.concatenate(ll + [np.zeros((0, 6), np.float64)])
        a["h2"] = None
        if has_maplines2 is not None:
            a["h2"] = np.concatenate([np.ascontiguousarray(x, np.uint8).reshape(-1) for x in has_maplines2] + [np.zeros(0, np.uint8)])
            if len(a["h2"]) != a["off"][K]:
                raise PslfeError("CreateNewMapLines: the GetMapLine bytes do not fit the neighbour lines")
        a["sf"], a["s2"] = np.ascontiguousarray(scale_factors, np.float32).reshape(-1), np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        if len(a["sf"]) != len(a["s2"]):
            raise PslfeError("CreateNewMapLines: mvScaleFactors and mvLevelSigma2 differ in length")
        return a

    def CreateNewMapLines(self, kf1, ldesc1, has_mapline1, keylines1, lines3d1, lineeq1, neighbours, ldescs2, has_maplines2, keylines2, lines3d2,
                          scale_factors, level_sigma2, nnratio=0.95, TH=None, mutual=True, want_geom=True):
        """LocalMapping::CreateNewMapLines2 src/LocalMapping.cc:554-757 for KF1 against K neighbours in one call
        (pslfe_kf_create_new_map_lines): the search of LineSearchForTriangulationKeyFrames, then the pair body.  keylines1
        (KEYLINE_DTYPE[NL1]), lines3d1 [NL1, 6] doubles = mvLines3D, lineeq1 [NL1] = mvLineEq[i][2]; per neighbour ldescs2[k],
        has_maplines2[k], keylines2[k], lines3d2[k]; scale_factors / level_sigma2 are the POINT tables.
        -> dict: match, status [K, NL1], sp, ep [K, NL1, 3], nmatches [K], created_by [NL1], new (NEWMAPLINE_DTYPE[nnew]), geom."""
        a = self._new_lines_args(kf1, ldesc1, has_mapline1, keylines1, lines3d1, lineeq1, neighbours, ldescs2, has_maplines2, keylines2, lines3d2,
                                 scale_factors, level_sigma2)
        K, n1 = a["K"], a["n1"]
        match, status = np.full((K, n1), -1, np.int32), np.full((K, n1), 1, np.int32)
        sp, ep = np.zeros((K, n1, 3), np.float32), np.zeros((K, n1, 3), np.float32)
        nm, by = np.zeros(max(K, 1), np.int32), np.full(max(n1, 1), -1, np.int32)
        newl, geom, nnew = np.zeros(max(n1, 1), NEWMAPLINE_DTYPE), np.zeros(max(n1, 1), MAPLINE_DTYPE), C.c_int(0)
        _check(lib().pslfe_kf_create_new_map_lines(
            self._h, _ptr(a["kf1"]), C.c_int(n1), _ptr(a["d1"]), _ptr(a["h1"]), _ptr(a["kl1"]), _ptr(a["l1"]), _ptr(a["eq1"]), _ptr(a["nb"]), C.c_int(K),
            _ptr(a["d2"]), _ptr(a["off"]), _ptr(a["h2"]), _ptr(a["kl2"]), _ptr(a["l2"]), C.c_float(nnratio), C.c_float(self.TH_LOW if TH is None else TH),
            C.c_int(1 if mutual else 0), _ptr(a["sf"]), _ptr(a["s2"]), C.c_int(len(a["sf"])), _ptr(match), _ptr(status), _ptr(sp), _ptr(ep), _ptr(nm),
            _ptr(by), _ptr(newl), C.byref(nnew), _ptr(geom) if want_geom else None), "pslfe_kf_create_new_map_lines")
        n = nnew.value
        return {"match": match, "status": status, "sp": sp, "ep": ep, "nmatches": nm[:K], "created_by": by[:n1], "new": newl[:n], "geom": geom[:n]}

    def CreateNewMapLinesDevice(self, kf1, NL1, d_desc1, d_has_mapline1, d_kls1, d_lines3d1, d_lineeq1, neighbours, d_desc2, off2, d_has_mapline2,
                                d_kls2, d_lines3d2, scale_factors, level_sigma2, d_match, d_status, d_sp, d_ep, d_nmatches, d_created_by, d_newl,
                                d_nnew, d_geom, d_obs_off, d_obs_kf, d_ref_kf, d_ref_level, nnratio=0.95, TH=None, mutual=True):
        """The same on device addresses (pslfe_kf_create_new_map_lines_device); d_geom and the runs are what
        line_update_average_dir_device takes with M = NL1."""
        k1, nb = np.ascontiguousarray(kf1, TRIKEYFRAME_DTYPE).reshape(1), np.ascontiguousarray(neighbours, TRINEIGHBOUR_DTYPE).reshape(-1)
        off = np.ascontiguousarray(off2, np.int32).reshape(-1)
        sf, s2 = np.ascontiguousarray(scale_factors, np.float32).reshape(-1), np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        v = lambda d: C.c_void_p(d) if d else None
        _check(lib().pslfe_kf_create_new_map_lines_device(
            self._h, _ptr(k1), C.c_int(NL1), v(d_desc1), v(d_has_mapline1), v(d_kls1), v(d_lines3d1), v(d_lineeq1), _ptr(nb), C.c_int(len(nb)), v(d_desc2),
            _ptr(off), v(d_has_mapline2), v(d_kls2), v(d_lines3d2), C.c_float(nnratio), C.c_float(self.TH_LOW if TH is None else TH),
            C.c_int(1 if mutual else 0), _ptr(sf), _ptr(s2), C.c_int(len(sf)), v(d_match), v(d_status), v(d_sp), v(d_ep), v(d_nmatches), v(d_created_by),
            v(d_newl), v(d_nnew), v(d_geom), v(d_obs_off), v(d_obs_kf), v(d_ref_kf), v(d_ref_level)), "pslfe_kf_create_new_map_lines_device")

    def ComputeDistinctiveDescriptors(self, desc, offsets):
        """src/MapPoint.cc:242-304 for many map points / lines at once -> best row per point (relative to its run)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        off = np.ascontiguousarray(offsets, np.int32)
        npts = len(off) - 1
        best = np.full(max(npts, 1), -1, np.int32)
        _check(lib().pslfe_kf_distinctive_descriptors(self._h, _ptr(d), _ptr(off), C.c_int(npts), _ptr(best)),
               "pslfe_kf_distinctive_descriptors")
        return best[:npts]

    def set_upkeep_sum(self, layout):
        """The layout of the run-order sums of the refresh methods below: UPKEEP_SUM_WALK or UPKEEP_SUM_TILED (same bytes)."""
        _check(lib().pslfe_kf_set_upkeep_sum(self._h, C.c_int(layout)), "pslfe_kf_set_upkeep_sum")

    @staticmethod
    def _upkeep_args(n, obs_off, obs_kf, centres, ref_kf, ref_level, scale_factors, skip, who):
        off = np.ascontiguousarray(obs_off, np.int32).reshape(-1)
        okf = np.ascontiguousarray(obs_kf, np.int32).reshape(-1)
        ow = np.ascontiguousarray(centres, np.float32).reshape(-1, 3)
        rk, rl = np.ascontiguousarray(ref_kf, np.int32).reshape(-1), np.ascontiguousarray(ref_level, np.int32).reshape(-1)
        sk = None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(-1)
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        if len(off) != n + 1 or len(rk) != n or len(rl) != n or (sk is not None and len(sk) != n) or (n and len(okf) < off[-1]):
            raise PslfeError(f"{who}: the offsets, references or skip bytes do not fit {n} rows")
        keep = (off, okf, ow, rk, rl, sk, sf)
        return keep, (_ptr(off), _ptr(okf), _ptr(ow), C.c_int(len(ow)), _ptr(rk), _ptr(rl), _ptr(sk), _ptr(sf), C.c_int(len(sf)))

    def UpdateNormalAndDepth(self, mp, obs_off, obs_kf, centres, ref_kf, ref_level, scale_factors, skip=None):
        """MapPoint::UpdateNormalAndDepth src/MapPoint.cc:330-371 for every row of mp (MAPPOINT_DTYPE[M]): row i is observed from the
        camera centres centres[obs_kf[obs_off[i]:obs_off[i+1]]] in the caller's mObservations order; ref_kf / ref_level = mpRefKF and
        the octave of its observation; scale_factors = mvScaleFactors.  -> a copy of mp with nx..max_dist refreshed; rows with an empty
        run or a skip byte unchanged."""
        g = np.array(mp, MAPPOINT_DTYPE).reshape(-1)
        keep, a = self._upkeep_args(len(g), obs_off, obs_kf, centres, ref_kf, ref_level, scale_factors, skip, "UpdateNormalAndDepth")
        _check(lib().pslfe_kf_update_normal_and_depth(self._h, _ptr(g), C.c_int(len(g)), *a), "pslfe_kf_update_normal_and_depth")
        return g

    def update_normal_and_depth_device(self, d_mp, M, d_obs_off, d_obs_kf, d_centres, nkf, d_ref_kf, d_ref_level, d_skip, scale_factors):
        """The same on device addresses (d_skip 0 = none), in place, queued on the context's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        v = lambda d: C.c_void_p(d) if d else None
        _check(lib().pslfe_kf_update_normal_and_depth_device(self._h, v(d_mp), C.c_int(M), v(d_obs_off), v(d_obs_kf), v(d_centres), C.c_int(nkf),
                                                             v(d_ref_kf), v(d_ref_level), v(d_skip), _ptr(sf), C.c_int(len(sf))),
               "pslfe_kf_update_normal_and_depth_device")

    def LineUpdateAverageDir(self, ml, obs_off, obs_kf, centres, ref_kf, ref_level, scale_factors, skip=None):
        """MapLine::UpdateAverageDir add_src/MapLine.cpp:320-367 for every row of ml (MAPLINE_DTYPE[M]), arguments as
        UpdateNormalAndDepth; scale_factors = pRefKF->mvScaleFactors (the point table, as the reference reads it).
        -> a copy of ml with normal, min_dist, max_dist refreshed."""
        g = np.array(ml, MAPLINE_DTYPE).reshape(-1)
        keep, a = self._upkeep_args(len(g), obs_off, obs_kf, centres, ref_kf, ref_level, scale_factors, skip, "LineUpdateAverageDir")
        _check(lib().pslfe_kf_line_update_average_dir(self._h, _ptr(g), C.c_int(len(g)), *a), "pslfe_kf_line_update_average_dir")
        return g

    def line_update_average_dir_device(self, d_ml, M, d_obs_off, d_obs_kf, d_centres, nkf, d_ref_kf, d_ref_level, d_skip, scale_factors):
        """The same on device addresses, in place, queued on the context's stream."""
        sf = np.ascontiguousarray(scale_factors, np.float32).reshape(-1)
        v = lambda d: C.c_void_p(d) if d else None
        _check(lib().pslfe_kf_line_update_average_dir_device(self._h, v(d_ml), C.c_int(M), v(d_obs_off), v(d_obs_kf), v(d_centres), C.c_int(nkf),
                                                             v(d_ref_kf), v(d_ref_level), v(d_skip), _ptr(sf), C.c_int(len(sf))),
               "pslfe_kf_line_update_average_dir_device")

    def ComputeSceneMedianDepth(self, poses, positions, q):
        """KeyFrame::ComputeSceneMedianDepth(q) src/KeyFrame.cc:749-779 for K keyframes: poses POSE_DTYPE[K], positions[k] = the world
        positions (n_k x 3) of keyframe k's map points.  -> depth float32[K]; -1 for a keyframe without map points."""
        T = np.ascontiguousarray(poses, POSE_DTYPE).reshape(-1)
        K = len(T)
        if len(positions) != K:
            raise PslfeError(f"ComputeSceneMedianDepth: {len(positions)} position lists for {K} keyframes")
        xs = [np.ascontiguousarray(p, np.float32).reshape(-1, 3) for p in positions]
        off = np.zeros(K + 1, np.int32)
        off[1:] = np.cumsum([len(p) for p in xs])
        x = np.concatenate(xs) if K else np.zeros((0, 3), np.float32)
        depth = np.zeros(max(K, 1), np.float32)
        _check(lib().pslfe_kf_scene_median_depth(self._h, _ptr(T), C.c_int(K), _ptr(x), _ptr(off), C.c_int(q), _ptr(depth)),
               "pslfe_kf_scene_median_depth")
        return depth[:K]

    def close(self):
        if self._h:
            lib().pslfe_kf_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _lsd_search_for_triangulation(self, ldesc1, ldesc2, has_mapline1, has_mapline2, TH=None, isDouble=True):
    """LSDmatcher::SearchForTriangulation add_src/LSDmatcher.cpp:705-781: FrameBFMatch both ways, mutual check, lines that
    already have a MapLine dropped.  TH = TH_LOW with the pair-vector overload (:705), TH_HIGH with the vector<int> one (:744).
    -> (nmatches, vMatchedPairs as an int array: index in KF2 or -1)."""
    TH = self.TH_LOW if TH is None else TH
    d1 = np.ascontiguousarray(ldesc1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(ldesc2, np.uint8).reshape(-1, 32)
    out = np.full(len(d1), -1, np.int32)
    if len(d1) == 0 or len(d2) == 0:
        return 0, out
    m12 = self.FrameBFMatch(d1, d2, TH)
    m21 = self.FrameBFMatch(d2, d1, TH)
    n = 0
    for i, j in enumerate(m12):
        if j < 0 or (isDouble and m21[j] != i) or has_mapline1[i] or has_mapline2[j]:
            continue
        out[i] = j
        n += 1
    return n, out


def _lsd_search_for_triangulation_keyframes(self, ldesc1, ldescs2, has_mapline1, has_maplines2, TH=None, isDouble=True):
    """LSDmatcher::SearchForTriangulation add_src/LSDmatcher.cpp:705-781 of one keyframe against the K neighbours of CreateNewMapLines2
    (src/LocalMapping.cc:554-580) in one call: ldescs2[k] / has_maplines2[k] per neighbour, TH and isDouble as SearchForTriangulation.
    -> (nmatches [K], vMatchedPairs [K, n1]).  has_mapline1 is the state at the call: a caller that gives KF1's lines map lines between
    neighbours checks GetMapLine(i) again when it consumes neighbour k's pairs."""
    if getattr(self, "_kf", None) is None:
        self._kf = KeyFrameMatcher(self.ctx)
    return self._kf.LineSearchForTriangulationKeyFrames(ldesc1, ldescs2, has_mapline1, has_maplines2, self.mfNNratio,
                                                        self.TH_LOW if TH is None else TH, isDouble)


LSDmatcher.SearchForTriangulation = _lsd_search_for_triangulation
LSDmatcher.SearchForTriangulationKeyFrames = _lsd_search_for_triangulation_keyframes


class LocalMapping:
    """LocalMapping::CreateNewMapPoints / CreateNewMapLines2 (src/LocalMapping.cc:275-520, :522-759) played on arrays, the way
    Sim3Solver.ComputeSim3Candidates and PnPsolver.RelocalizeCandidates play their callers: the keyframes are dicts of the members the
    reference reads, the map mutations (:502-517, :741-755) come back as lists."""

    @staticmethod
    def TriQueries(fvec1, fvec2, keysun1, uright1, taken1, only_stereo=False):
        """the head of ORBmatcher::SearchForTriangulation src/ORBmatcher.cc:689-711: fvec = [(node, [features])] ascending by node.
        -> (queries TRIQUERY_DTYPE, idx1, fidx2) in the reference's iteration order over the shared nodes."""
        fidx2, start2 = [], {}
        for node, feats in fvec2:
            start2[node] = (len(fidx2), len(feats))
            fidx2 += list(feats)
        rows, idx1 = [], []
        for node, feats in fvec1:
            if node not in start2:
                continue
            for i in feats:
                if taken1[i] or (only_stereo and not uright1[i] >= 0):
                    continue
                rows.append((start2[node][0], start2[node][1], keysun1["x"][i], keysun1["y"][i], keysun1["angle"][i], int(uright1[i] >= 0)))
                idx1.append(i)
        return np.array(rows, TRIQUERY_DTYPE).reshape(-1), np.array(idx1, np.int32), np.array(fidx2, np.int32)

    @staticmethod
    def CreateNewMapPoints(matcher, frame2, kf1, cur, neighbours, neigh, scale_factors, level_sigma2, checkOri=False):
        """cur: dict(keysun, keys, uright, depth, taken, fvec, desc) of mpCurrentKeyFrame; neigh[k]: dict(keys, depth, taken, fvec) of
        neighbour k, whose mvKeysUn / mvuRight / descriptors are slot neighbours[k]["slot"] of frame2.
        -> (the dict of KeyFrameMatcher.CreateNewMapPoints, [(k, idx1, idx2, x3D)] in creation order = mlpRecentAddedMapPoints)."""
        qs, i1s, fs, qds = [], [], [], []
        for nb in neigh:
            q, i1, f = LocalMapping.TriQueries(cur["fvec"], nb["fvec"], cur["keysun"], cur["uright"], cur["taken"])
            qs.append(q); i1s.append(i1); fs.append(f); qds.append(np.asarray(cur["desc"], np.uint8).reshape(-1, 32)[i1])
        r = matcher.CreateNewMapPoints(frame2, kf1, cur["keysun"], cur["keys"], cur["uright"], cur["depth"], cur["taken"], neighbours, fs,
                                       [nb["taken"] for nb in neigh], [nb["keys"] for nb in neigh], [nb["depth"] for nb in neigh], qs, i1s, qds,
                                       scale_factors, level_sigma2, False, checkOri)
        return r, [(int(p["k"]), int(p["idx1"]), int(p["idx2"]), np.array([p["x"], p["y"], p["z"]], np.float32)) for p in r["new"]]

    @staticmethod
    def CreateNewMapLines(matcher, kf1, cur, neighbours, neigh, scale_factors, level_sigma2, nnratio=0.95):
        """cur: dict(ldesc, has_mapline, keylines, lines3d, lineeq); neigh[k]: dict(ldesc, has_mapline, keylines, lines3d).
        -> (the dict of KeyFrameMatcher.CreateNewMapLines, [(k, idx1, idx2, sp, ep)] in creation order = mlpRecentAddedMapLines)."""
        r = matcher.CreateNewMapLines(kf1, cur["ldesc"], cur["has_mapline"], cur["keylines"], cur["lines3d"], cur["lineeq"], neighbours,
                                      [nb["ldesc"] for nb in neigh], [nb["has_mapline"] for nb in neigh], [nb["keylines"] for nb in neigh],
                                      [nb["lines3d"] for nb in neigh], scale_factors, level_sigma2, nnratio)
        return r, [(int(p["k"]), int(p["idx1"]), int(p["idx2"]), p["sp"].copy(), p["ep"].copy()) for p in r["new"]]
