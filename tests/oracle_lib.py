"""ctypes access to the ORACLE (oracle/libpsl_oracle.so): test infrastructure only."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ODIR = os.path.join(ROOT, "oracle")
SO = os.path.join(ODIR, "libpsl_oracle.so")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])


def build():
    srcs = [os.path.join(ODIR, f) for f in os.listdir(ODIR) if f.endswith((".cpp", ".h", ".inc", "Makefile"))]
    if not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.run(["make", "-C", ODIR], check=True, capture_output=True)
    return SO


_lib = None


def load():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(SO)
        L.pso_orb_create.restype = C.c_void_p
        L.pso_orb_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int]
        L.pso_orb_destroy.argtypes = [C.c_void_p]
        L.pso_orb_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.pso_orb_quota.argtypes = [C.c_void_p, C.c_int]
        L.pso_orb_scale.argtypes = [C.c_void_p, C.c_int]
        L.pso_orb_scale.restype = C.c_float
        L.pso_orb_umax.argtypes = [C.c_void_p, C.c_int]
        L.pso_orb_level_size.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.pso_orb_level_ptr.argtypes = [C.c_void_p, C.c_int]
        L.pso_orb_level_ptr.restype = C.c_void_p
        L.pso_orb_blur_ptr.argtypes = [C.c_void_p, C.c_int]
        L.pso_orb_blur_ptr.restype = C.c_void_p
        L.pso_orb_level_candidates.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.pso_orb_level_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        L.pso_distribute_octree.argtypes = [C.c_void_p, C.c_int] + [C.c_int] * 5 + [C.c_void_p, C.c_int]
        L.pso_resize_linear_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
        L.pso_gaussian_blur_u8.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p]
        L.pso_gaussian_kernel_q8.argtypes = [C.c_int, C.c_double, C.c_void_p]
        L.pso_fast_subimage.argtypes = [C.c_void_p] + [C.c_int] * 7 + [C.c_void_p, C.c_int]
        for f in ("pso_fast_atan2_f",):
            getattr(L, f).argtypes = [C.c_float, C.c_float]
            getattr(L, f).restype = C.c_float
        for f in ("pso_sinf_f", "pso_cosf_f", "pso_libm_sinf", "pso_libm_cosf"):
            getattr(L, f).argtypes = [C.c_float]
            getattr(L, f).restype = C.c_float
        L.pso_cvround_d.argtypes = [C.c_double]
        L.pso_orb_pattern.restype = C.POINTER(C.c_int8)
        _lib = L
    return _lib


class OracleORB:
    """CPU restatement of ORBextractor (oracle/orb_oracle.cpp) with stage taps."""

    def __init__(self, nfeatures=1000, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7):
        self.L = load()
        self.nlevels = nlevels
        self.h = self.L.pso_orb_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
        assert self.h

    def __call__(self, image):
        image = np.ascontiguousarray(image)
        hh, ww = image.shape
        cap = 8 * 4096
        kps = np.zeros(cap, KEYPOINT_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n = self.L.pso_orb_extract(self.h, image.ctypes.data, ww, hh, image.strides[0], kps.ctypes.data, desc.ctypes.data, cap)
        assert n >= 0
        return kps[:n].copy(), desc[:n].copy()

    def quota(self):
        return [self.L.pso_orb_quota(self.h, l) for l in range(self.nlevels)]

    def level_image(self, level, blurred=False):
        w, h = C.c_int(), C.c_int()
        assert self.L.pso_orb_level_size(self.h, level, C.byref(w), C.byref(h)) == 0
        p = self.L.pso_orb_blur_ptr(self.h, level) if blurred else self.L.pso_orb_level_ptr(self.h, level)
        if not p:
            return None
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (h.value, w.value)).copy()

    def candidates(self, level):
        n = self.L.pso_orb_level_candidates(self.h, level, None, 0)
        out = np.zeros((max(n, 1), 3), np.int32)
        self.L.pso_orb_level_candidates(self.h, level, out.ctypes.data, n)
        return out[:n]

    def level_keypoints(self, level):
        n = self.L.pso_orb_level_keypoints(self.h, level, None, 0)
        out = np.zeros(max(n, 1), KEYPOINT_DTYPE)
        self.L.pso_orb_level_keypoints(self.h, level, out.ctypes.data, n)
        return out[:n]

    def __del__(self):
        try:
            self.L.pso_orb_destroy(self.h)
        except Exception:
            pass


PROJQUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("min_level", "<i4"),
                            ("max_level", "<i4"), ("angle", "<f4"), ("blocks", "<i4")])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def grid_build(kps, bounds):
    L = load()
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    start = np.zeros(64 * 48 + 1, np.int32)
    idx = np.zeros(max(len(kps), 1), np.int32)
    L.pso_grid_build.argtypes = [C.c_void_p, C.c_int] + [C.c_float] * 4 + [C.c_void_p, C.c_void_p]
    n = L.pso_grid_build(_p(kps), len(kps), *bounds, _p(start), _p(idx))
    return start, idx[:n]


def _search(fn_name, kps, desc, uright, bounds, queries, qdesc, taken, extra_type, extra):
    L = load()
    fn = getattr(L, fn_name)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_float] * 4 + [C.c_void_p, C.c_void_p, C.c_int,
                                                                                     C.c_void_p, extra_type, C.c_void_p, C.c_void_p]
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(desc, np.uint8)
    queries = np.ascontiguousarray(queries, PROJQUERY_DTYPE)
    qdesc = np.ascontiguousarray(qdesc, np.uint8)
    ur = None if uright is None else np.ascontiguousarray(uright, np.float32)
    tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
    match = np.full(max(len(queries), 1), -1, np.int32)
    assigned = np.full(max(len(kps), 1), -1, np.int32)
    nm = fn(_p(kps), _p(desc), _p(ur), len(kps), *bounds, _p(queries), _p(qdesc), len(queries), _p(tk), extra, _p(match), _p(assigned))
    return nm, match[:len(queries)], assigned[:len(kps)]


def search_by_projection_last(kps, desc, uright, bounds, queries, qdesc, taken, check_ori):
    return _search("pso_search_by_projection_last", kps, desc, uright, bounds, queries, qdesc, taken, C.c_int, int(check_ori))


def search_by_projection_map(kps, desc, uright, bounds, queries, qdesc, taken, nnratio):
    return _search("pso_search_by_projection_map", kps, desc, uright, bounds, queries, qdesc, taken, C.c_float, float(nnratio))


def hamming_knn2(q, t):
    L = load()
    q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
    t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
    idx = np.zeros((max(len(q), 1), 2), np.int32)
    dist = np.zeros((max(len(q), 1), 2), np.int32)
    L.pso_hamming_knn2.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.pso_hamming_knn2(_p(q), len(q), _p(t), len(t), _p(idx), _p(dist))
    return idx[:len(q)], dist[:len(q)]


def line_match_nnr(d1, d2, nnr):
    L = load()
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
    m12 = np.full(max(len(d1), 1), -1, np.int32)
    L.pso_line_match_nnr.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    n = L.pso_line_match_nnr(_p(d1), len(d1), _p(d2), len(d2), nnr, _p(m12))
    return n, m12[:len(d1)]


def hamming256(a, b):
    L = load()
    L.pso_hamming256.argtypes = [C.c_void_p, C.c_void_p]
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    return L.pso_hamming256(_p(a), _p(b))


KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                          ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                          ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                          ("lineLength", "<f4"), ("numOfPixels", "<i4")])


def lsd_detect(img, cap=20000):
    L = load()
    img = np.ascontiguousarray(img)
    h, w = img.shape
    seg = np.zeros((cap, 4), np.float32)
    L.pso_lsd_detect.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = L.pso_lsd_detect(_p(img), w, h, img.strides[0], _p(seg), cap)
    return seg[:n].copy()


def lsd_refine_stats(img):
    """Lsd::debug_refine of one frame: regions of min_reg_size or more, refinements entered, their pixels, regrown pixels, reduce_region_radius calls, its
    radius steps, the list entries it visits, the pixels of its region2rect calls, the largest (list length + pixels removed) of a step, W * H."""
    L = load()
    img = np.ascontiguousarray(img)
    h, w = img.shape
    out = np.zeros(10, np.int64)
    L.pso_lsd_refine_stats.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.pso_lsd_refine_stats(_p(img), w, h, img.strides[0], _p(out))
    return out


def lsd_gradient(img):
    L = load()
    img = np.ascontiguousarray(img)
    h, w = img.shape
    W, H = int(round(w * 0.8)), int(round(h * 0.8))
    scaled = np.zeros((H, W)); ang = np.zeros((H, W)); mod = np.zeros((H, W))
    Wc, Hc = C.c_int(), C.c_int()
    L.pso_lsd_gradient.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pso_lsd_gradient(_p(img), w, h, img.strides[0], _p(scaled), _p(ang), _p(mod), C.byref(Wc), C.byref(Hc))
    assert (Wc.value, Hc.value) == (W, H)
    return scaled, ang, mod


def optimize_and_merge(segs, w, h, cap=4096):
    L = load()
    segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 4)
    out = np.zeros(cap, KEYLINE_DTYPE)
    L.pso_optimize_and_merge.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = L.pso_optimize_and_merge(_p(segs), len(segs), w, h, _p(out), cap)
    return out[:n].copy()


def merge_lines(segs, ang, dist, ep, cap=8192):
    L = load()
    segs = np.ascontiguousarray(segs, np.float32).reshape(-1, 4)
    out = np.zeros((cap, 4), np.float32)
    L.pso_merge_lines.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int]
    n = L.pso_merge_lines(_p(segs), len(segs), ang, dist, ep, _p(out), cap)
    return out[:n].copy()


def lbd_compute(img, kls, want_float=False):
    L = load()
    img = np.ascontiguousarray(img)
    kls = np.ascontiguousarray(kls, KEYLINE_DTYPE)
    h, w = img.shape
    desc = np.zeros((max(len(kls), 1), 32), np.uint8)
    fdesc = np.zeros((max(len(kls), 1), 72), np.float32)
    L.pso_lbd_compute.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.pso_lbd_compute(_p(img), w, h, img.strides[0], _p(kls), len(kls), _p(desc), _p(fdesc))
    return (desc[:len(kls)], fdesc[:len(kls)]) if want_float else desc[:len(kls)]


def lbd_sobel(img):
    L = load()
    img = np.ascontiguousarray(img)
    h, w = img.shape
    dx = np.zeros((h, w), np.int16); dy = np.zeros((h, w), np.int16)
    L.pso_lbd_sobel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.pso_lbd_sobel(_p(img), w, h, img.strides[0], _p(dx), _p(dy))
    return dx, dy


def line_extract(img, nfeatures=200, cap=4096):
    L = load()
    img = np.ascontiguousarray(img)
    h, w = img.shape
    kls = np.zeros(cap, KEYLINE_DTYPE); desc = np.zeros((cap, 32), np.uint8); eq = np.zeros((cap, 3))
    L.pso_line_extract.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    n = L.pso_line_extract(_p(img), w, h, img.strides[0], nfeatures, _p(kls), _p(desc), _p(eq), cap)
    assert n >= 0
    return kls[:n].copy(), desc[:n].copy(), eq[:n].copy()


def lil_pair(lines, radius, fan_thr, cols, rows, cap=65536):
    L = load()
    lines = np.ascontiguousarray(lines, np.float32).reshape(-1, 4)
    fans = np.zeros((cap, 4), np.float32)
    L.pso_lil_pair.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = L.pso_lil_pair(_p(lines), len(lines), radius, fan_thr, cols, rows, _p(fans), cap)
    return fans[:n].copy()


def search_by_geom_appearance(kl_last, d_last, kl_cur, d_cur, has_mapline, desc_th, bounds):
    L = load()
    k1 = np.ascontiguousarray(kl_last, KEYLINE_DTYPE); k2 = np.ascontiguousarray(kl_cur, KEYLINE_DTYPE)
    d1 = np.ascontiguousarray(d_last, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(d_cur, np.uint8).reshape(-1, 32)
    hm = np.ascontiguousarray(has_mapline, np.uint8)
    m12 = np.full(max(len(k1), 1), -1, np.int32); asg = np.full(max(len(k2), 1), -1, np.int32)
    L.pso_search_by_geom_appearance.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float,
                                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    n = L.pso_search_by_geom_appearance(_p(k1), _p(d1), len(k1), _p(k2), _p(d2), len(k2), _p(hm), desc_th, *bounds, _p(m12), _p(asg))
    return n, m12[:len(k1)], asg[:len(k2)]


def frame_bf_match(d1, d2, nnratio, TH):
    L = load()
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32); d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
    lm = np.full(max(len(d1), 1), -1, np.int32)
    L.pso_frame_bf_match.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.pso_frame_bf_match(_p(d1), len(d1), _p(d2), len(d2), nnratio, TH, _p(lm))
    return lm[:len(d1)]


def associate_planes(planes, points, map_planes, dTh, aTh, live, map_bad=None):
    L = load()
    p = np.ascontiguousarray(planes, np.float32).reshape(-1, 4); q = np.ascontiguousarray(points, np.float64).reshape(-1, 15)
    m = np.ascontiguousarray(map_planes, np.float32).reshape(-1, 4)
    b = None if map_bad is None else np.ascontiguousarray(map_bad, np.uint8)
    assoc = np.full(max(len(p), 1), -1, np.int32)
    L.pso_associate_planes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_void_p]
    n = L.pso_associate_planes(_p(p), _p(q), len(p), _p(m), _p(b), len(m), dTh, aTh, int(live), _p(assoc))
    return n, assoc[:len(p)]


LINEQUERY_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("radius", "<f4"), ("th_cos", "<f4"),
                            ("vx", "<f4"), ("vy", "<f4"), ("length", "<f4"), ("blocks", "<i4"), ("wdir", "<f8", (3,))])


def line_grid_build(kls, bounds):
    L = load()
    k = np.ascontiguousarray(kls, KEYLINE_DTYPE)
    start = np.zeros(64 * 48 + 1, np.int32)
    idx = np.zeros(max(len(k), 1) * 112, np.int32)
    L.pso_line_grid_build.argtypes = [C.c_void_p, C.c_int] + [C.c_float] * 4 + [C.c_void_p, C.c_void_p, C.c_int]
    n = L.pso_line_grid_build(_p(k), len(k), *bounds, _p(start), _p(idx), len(idx))
    return start, idx[:n]


def line_search_by_projection(kls, desc, eq, bounds, queries, qdesc, mode=0, dir3d=None, taken=None, nnratio=0.95):
    L = load()
    k = np.ascontiguousarray(kls, KEYLINE_DTYPE); d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    e = np.ascontiguousarray(eq, np.float64).reshape(-1, 3)
    q = np.ascontiguousarray(queries, LINEQUERY_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    d3 = None if dir3d is None else np.ascontiguousarray(dir3d, np.float64).reshape(-1, 3)
    tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
    match = np.full(max(len(q), 1), -1, np.int32); asg = np.full(max(len(k), 1), -1, np.int32)
    L.pso_line_search_by_projection.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_float] * 4 + \
        [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
    n = L.pso_line_search_by_projection(_p(k), _p(d), _p(e), _p(d3), len(k), *bounds, _p(q), _p(qd), len(q), _p(tk), mode, nnratio, _p(match), _p(asg))
    return n, match[:len(q)], asg[:len(k)]


CAMERA_DTYPE = np.dtype([(k, "<f4") for k in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "bf")])


def rgb_to_gray(rgb, is_rgb=True):
    L = load()
    rgb = np.ascontiguousarray(rgb, np.uint8)
    h, w = rgb.shape[:2]
    gray = np.zeros((h, w), np.uint8)
    L.pso_rgb_to_gray.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.pso_rgb_to_gray(_p(rgb), w, h, 3 * w, 1 if is_rgb else 0, _p(gray))
    return gray


def depth_to_float(depth, factor):
    L = load()
    depth = np.ascontiguousarray(depth, np.uint16)
    out = np.zeros(depth.shape, np.float32)
    L.pso_depth_to_float.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    L.pso_depth_to_float(_p(depth), depth.size, factor, _p(out))
    return out


def _cam_arrays(cam):
    cam = np.asarray(cam, CAMERA_DTYPE).reshape(())
    K = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"]], np.float32)
    dist = np.array([cam["k1"], cam["k2"], cam["p1"], cam["p2"], cam["k3"]], np.float32)
    return K, dist, float(cam["bf"])


def image_bounds(cam, cols, rows):
    L = load()
    K, dist, _ = _cam_arrays(cam)
    b = np.zeros(4, np.float32)
    L.pso_image_bounds.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pso_image_bounds(cols, rows, _p(K), _p(dist), _p(b))
    return b


def frame_post_rgbd(kps, depth, cam):
    L = load()
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    depth = np.ascontiguousarray(depth, np.float32)
    K, dist, bf = _cam_arrays(cam)
    n = len(kps)
    un = np.zeros(max(n, 1), KEYPOINT_DTYPE)
    dep = np.zeros(max(n, 1), np.float32)
    ur = np.zeros(max(n, 1), np.float32)
    L.pso_frame_post_rgbd.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.pso_frame_post_rgbd(_p(kps), n, _p(depth), depth.shape[1], depth.shape[0], depth.shape[1], _p(K), _p(dist), bf, _p(un), _p(dep), _p(ur))
    return un[:n], dep[:n], ur[:n]


LINETRACE_DTYPE = np.dtype([(k, "<i4") for k in ("tried", "outside", "int_branch", "clamped", "holes", "np", "rand_drawn", "iterations",
                                                  "degenerate", "verify_calls", "verify_passes", "replaced", "ransac_inliers", "refine_grew",
                                                  "final_inliers", "exit_reason")])
LINE_NO_SAMPLES, LINE_FEW_POINTS, LINE_NO_VERIFIED_SET, LINE_SHORT_3D, LINE_ACCEPTED = range(5)   # PsoLineTrace.exit_reason
FAN_BAD_INDEX, FAN_DET_ZERO, FAN_DISTMID, FAN_ZERO_CROSSING, FAN_ACCEPTED = range(5)              # per fan row
PLANE_NOT_GOOD, PLANE_SPREAD, PLANE_OLD, PLANE_ACCEPTED = range(4)                                # per crossing


def frame_glue(keylines, fans, depth, cam, seed=1, depth_stride=None, trace=False):
    """oracle chain isLineGood -> convertFansToKeyLines -> planes, same dict as psl_slam_amd.FrameGlue.run (depth_stride as there:
    depth = buf[:, :width] of a contiguous [height][depth_stride] buffer).  trace=True adds line_trace (LINETRACE_DTYPE per line),
    fan_reason (FAN_* per fan row) and plane_trace ([crossings][3]: PLANE_*, flipped, the plane that made it old or -1)."""
    L = load()
    kls = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
    fans = np.ascontiguousarray(fans, np.float32).reshape(-1, 4)
    if depth_stride is None:
        depth = np.ascontiguousarray(depth, np.float32)
        depth_stride = depth.shape[1]
    else:
        assert depth.dtype == np.float32 and depth.strides == (4 * depth_stride, 4), "depth must be buf[:, :width] of a padded f32 buffer"
    K, _, _ = _cam_arrays(cam)
    n, nf = len(kls), len(fans)
    out = dict(lines3d=np.zeros((max(n, 1), 6), np.float64), lineEq=np.zeros((max(n, 1), 3), np.float32))
    good = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    args = (_p(kls), n, C.c_void_p(depth.ctypes.data), depth.shape[1], depth.shape[0], depth_stride, _p(K), seed, _p(out["lines3d"]), _p(out["lineEq"]))
    lt = np.zeros(max(n, 1), LINETRACE_DTYPE)
    if trace:
        L.pso_line_good_trace.argtypes = good + [C.c_void_p]
        L.pso_line_good_trace(*args, _p(lt))
    else:
        L.pso_line_good.argtypes = good
        L.pso_line_good(*args)
    cap = max(nf, 1)
    pair, xy, cross = np.zeros((cap, 2), np.int32), np.zeros((cap, 2), np.float32), np.zeros((cap, 3), np.float64)
    fr, pt = np.zeros(cap, np.int32), np.zeros((cap, 3), np.int32)
    L.pso_fans_to_intersections.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    ni = L.pso_fans_to_intersections(_p(fans), nf, _p(out["lines3d"]), n, _p(pair), _p(xy), _p(cross), cap, _p(fr) if trace else None)
    planes, normals, lineNo = np.zeros((cap, 4), np.float32), np.zeros((cap, 3), np.float64), np.zeros((cap, 2), np.int32)
    c3, c2, le_l = np.zeros((cap, 3), np.float64), np.zeros((cap, 2), np.float64), np.zeros((cap, 6), np.float64)
    L.pso_planes_from_pairs.argtypes = [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    npl = L.pso_planes_from_pairs(_p(kls), _p(out["lineEq"]), _p(out["lines3d"]), _p(pair), _p(xy), _p(cross), ni, _p(planes), _p(normals),
                                  _p(lineNo), _p(c3), _p(c2), _p(le_l), cap, _p(pt) if trace else None)
    out["lines3d"], out["lineEq"] = out["lines3d"][:n], out["lineEq"][:n]
    out.update(pair=pair[:ni], xy=xy[:ni], cross=cross[:ni], le_l=le_l[:ni], planes=planes[:npl], normals=normals[:npl], lineNo=lineNo[:npl],
               cross3d=c3[:npl], cross2d=c2[:npl])
    if trace:
        out.update(line_trace=lt[:n], fan_reason=fr[:nf], plane_trace=pt[:ni])
    return out


def glibc_rand(seed, n):
    L = load()
    out = np.zeros(n, np.int32)
    L.pso_glibc_rand.argtypes = [C.c_uint32, C.c_int, C.c_void_p]
    L.pso_glibc_rand(seed, n, _p(out))
    return out


def search_by_projection_kf(kps, desc, bounds, queries, qdesc, taken, orb_dist, check_ori):
    L = load()
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    queries = np.ascontiguousarray(queries, PROJQUERY_DTYPE); qdesc = np.ascontiguousarray(qdesc, np.uint8)
    n, nq = len(kps), len(queries)
    tk = None if taken is None else np.ascontiguousarray(taken, np.uint8)
    match = np.full(max(nq, 1), -1, np.int32); assigned = np.full(max(n, 1), -1, np.int32)
    L.pso_search_by_projection_kf.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_float] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                                                                                 C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    nm = L.pso_search_by_projection_kf(_p(kps), _p(desc), n, *bounds, _p(queries), _p(qdesc), nq, _p(tk) if tk is not None else None,
                                       int(orb_dist), int(check_ori), _p(match), _p(assigned))
    return nm, match[:nq], assigned[:n]


def search_by_bow(fdesc, fangle, fidx, runs, qdesc, qangle, nnratio, check_ori):
    L = load()
    fdesc = np.ascontiguousarray(fdesc, np.uint8); fangle = np.ascontiguousarray(fangle, np.float32)
    fidx = np.ascontiguousarray(fidx, np.int32); runs = np.ascontiguousarray(runs, np.int32).reshape(-1, 2)
    qdesc = np.ascontiguousarray(qdesc, np.uint8); qangle = np.ascontiguousarray(qangle, np.float32)
    nf, nq = len(fangle), len(runs)
    match = np.full(max(nq, 1), -1, np.int32); assigned = np.full(max(nf, 1), -1, np.int32)
    L.pso_search_by_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int,
                                    C.c_void_p, C.c_void_p]
    nm = L.pso_search_by_bow(_p(fdesc), _p(fangle), nf, _p(fidx), _p(runs), _p(qdesc), _p(qangle), nq, float(nnratio), int(check_ori),
                             _p(match), _p(assigned))
    return nm, match[:nq], assigned[:nf]


def compute_bow(children, node_desc, node_weight, node_word, L, desc, levelsup=4):
    Lb = load()
    nn = len(children)
    cb = np.zeros(nn, np.int32)
    cc = np.array([len(c) for c in children], np.int32)
    cb[1:] = np.cumsum(cc)[:-1]
    ids = np.array([x for c in children for x in c], np.int32)
    nd = np.ascontiguousarray(node_desc, np.uint8); nw = np.ascontiguousarray(node_weight, np.float64); nwd = np.ascontiguousarray(node_word, np.int32)
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    n = len(desc); m = max(n, 1)
    o = dict(word=np.zeros(m, np.int32), weight=np.zeros(m, np.float64), nid=np.zeros(m, np.int32), bow_id=np.zeros(m, np.int32),
             bow_val=np.zeros(m, np.float64), fv_node=np.zeros(m, np.int32), fv_start=np.zeros(m + 1, np.int32), fv_idx=np.zeros(m, np.int32))
    nf = C.c_int()
    Lb.pso_compute_bow.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    nb = Lb.pso_compute_bow(_p(cb), _p(cc), _p(ids), _p(nd), _p(nw), _p(nwd), int(L), int(levelsup), _p(desc), n, _p(o["word"]), _p(o["weight"]),
                            _p(o["nid"]), _p(o["bow_id"]), _p(o["bow_val"]), _p(o["fv_node"]), _p(o["fv_start"]), _p(o["fv_idx"]), C.byref(nf))
    for k in ("word", "weight", "nid"):
        o[k] = o[k][:n]
    o["bow_id"], o["bow_val"] = o["bow_id"][:nb], o["bow_val"][:nb]
    o["fv_node"], o["fv_start"] = o["fv_node"][:nf.value], o["fv_start"][:nf.value + 1]
    o["fv_idx"] = o["fv_idx"][:int(o["fv_start"][nf.value])] if nf.value else o["fv_idx"][:0]
    return o


# ---- KeyFrame-rate matchers (oracle/kf_oracle.cpp) ------------------------------------------------------------------
TRIQUERY_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("stereo", "<i4")])
LINEFUSEQUERY_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("radius", "<f4"), ("level", "<i4")])


def window_best(kps, desc, uright, bounds, queries, qdesc, chi2=False, inv_sigma2=None):
    L = load()
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
    ur = np.full(len(kps), -1, np.float32) if uright is None else np.ascontiguousarray(uright, np.float32)
    q = np.ascontiguousarray(queries, PROJQUERY_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
    b = np.array(bounds, np.float32)
    s2 = np.zeros(16, np.float32) if inv_sigma2 is None else np.ascontiguousarray(inv_sigma2, np.float32)
    bi = np.full(max(len(q), 1), -1, np.int32); bd = np.zeros(max(len(q), 1), np.int32)
    L.pso_window_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    L.pso_window_best.restype = None
    L.pso_window_best(_p(kps), _p(desc), _p(ur), len(kps), _p(b), _p(q), _p(qd), len(q), int(chi2), _p(s2), _p(bi), _p(bd))
    return bi[:len(q)], bd[:len(q)]


def search_by_sim3(kps1, desc1, bounds1, kps2, desc2, bounds2, q12, qdesc1, q21, qdesc2):
    L = load()
    kps1 = np.ascontiguousarray(kps1, KEYPOINT_DTYPE); kps2 = np.ascontiguousarray(kps2, KEYPOINT_DTYPE)
    desc1 = np.ascontiguousarray(desc1, np.uint8); desc2 = np.ascontiguousarray(desc2, np.uint8)
    q12 = np.ascontiguousarray(q12, PROJQUERY_DTYPE); q21 = np.ascontiguousarray(q21, PROJQUERY_DTYPE)
    qdesc1 = np.ascontiguousarray(qdesc1, np.uint8); qdesc2 = np.ascontiguousarray(qdesc2, np.uint8)
    assert len(q12) == len(kps1) and len(q21) == len(kps2)
    b1 = np.array(bounds1, np.float32); b2 = np.array(bounds2, np.float32)
    m = np.full(max(len(kps1), 1), -1, np.int32)
    L.pso_search_by_sim3.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 5
    nf = L.pso_search_by_sim3(_p(kps1), _p(desc1), len(kps1), _p(b1), _p(kps2), _p(desc2), len(kps2), _p(b2), _p(q12), _p(qdesc1), _p(q21),
                              _p(qdesc2), _p(m))
    return nf, m[:len(kps1)]


def search_for_triangulation(kps2, desc2, uright2, taken2, fidx2, queries, qdesc, F12, epipole, scale_factors, level_sigma2, only_stereo,
                             check_ori):
    L = load()
    kps2 = np.ascontiguousarray(kps2, KEYPOINT_DTYPE); desc2 = np.ascontiguousarray(desc2, np.uint8)
    ur = np.ascontiguousarray(uright2, np.float32); tk = np.ascontiguousarray(taken2, np.uint8)
    fidx = np.ascontiguousarray(fidx2, np.int32); q = np.ascontiguousarray(queries, TRIQUERY_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
    F = np.ascontiguousarray(F12, np.float32).reshape(9)
    sf = np.ascontiguousarray(scale_factors, np.float32); s2 = np.ascontiguousarray(level_sigma2, np.float32)
    match = np.full(max(len(q), 1), -1, np.int32)
    L.pso_search_for_triangulation.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                                                   C.c_void_p, C.c_void_p]
    nm = L.pso_search_for_triangulation(_p(kps2), _p(desc2), _p(ur), _p(tk), _p(fidx), _p(q), _p(qd), len(q), _p(F), float(epipole[0]),
                                        float(epipole[1]), int(only_stereo), int(check_ori), _p(sf), _p(s2), _p(match))
    return nm, match[:len(q)]


def line_fuse_best(kls, desc, queries, qdesc):
    L = load()
    kls = np.ascontiguousarray(kls, KEYLINE_DTYPE); desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    q = np.ascontiguousarray(queries, LINEFUSEQUERY_DTYPE); qd = np.ascontiguousarray(qdesc, np.uint8)
    bi = np.full(max(len(q), 1), -1, np.int32); bd = np.zeros(max(len(q), 1), np.int32)
    L.pso_line_fuse_best.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.pso_line_fuse_best.restype = None
    L.pso_line_fuse_best(_p(kls), len(kls), _p(desc), len(desc), _p(q), _p(qd), len(q), _p(bi), _p(bd))
    return bi[:len(q)], bd[:len(q)]


def distinctive_descriptors(desc, offsets):
    L = load()
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32); off = np.ascontiguousarray(offsets, np.int32)
    best = np.full(max(len(off) - 1, 1), -1, np.int32)
    L.pso_distinctive_descriptors.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.pso_distinctive_descriptors.restype = None
    L.pso_distinctive_descriptors(_p(desc), _p(off), len(off) - 1, _p(best))
    return best[:len(off) - 1]


def set_lsd_refine(mode):
    """1 = LSD_REFINE_STD, 2 = LSD_REFINE_ADV (the oracle's default); returns the previous mode."""
    L = load()
    return L.pso_set_lsd_refine(int(mode))


def set_nfa_math(restated):
    """0 = host libm in nfa() (default), 1 = the product's restated log / exp / log10 (psl_f64math.h)."""
    L = load()
    return L.pso_set_nfa_math(int(restated))


def lsd_nfa(n, k, p, W, H):
    L = load()
    L.pso_lsd_nfa.restype = C.c_double
    L.pso_lsd_nfa.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]
    return L.pso_lsd_nfa(n, k, p, W, H)


def lsd_nfa_lognt_tail(n, k, p, log_nt):
    """nfa(n, k, p) with log(NT) given, and the binomial tail it was taken from (0 = no series was summed), for arrays of trials."""
    L = load()
    n = np.ascontiguousarray(n, np.int32).ravel()
    k = np.ascontiguousarray(k, np.int32).ravel()
    p = np.ascontiguousarray(p, np.float64).ravel()
    assert len(n) == len(k) == len(p)
    v, tail = np.zeros(len(n)), np.zeros(len(n))
    L.pso_lsd_nfa_lognt_tail_n.restype = None
    L.pso_lsd_nfa_lognt_tail_n.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    L.pso_lsd_nfa_lognt_tail_n(len(n), _p(n), _p(k), _p(p), float(log_nt), _p(v), _p(tail))
    return v, tail


def lsd_log_gamma(x):
    """log_gamma() of the oracle's nfa() for an array of arguments (host libm, or the restated functions under set_nfa_math(1))."""
    L = load()
    L.pso_lsd_log_gamma.restype = C.c_double
    L.pso_lsd_log_gamma.argtypes = [C.c_double]
    return np.array([L.pso_lsd_log_gamma(float(v)) for v in np.asarray(x).ravel()], np.float64)


def math_eval(fn, a, b=None):
    """Host twin of psl_slam_amd.debug_math (oracle/math_oracle.cpp): the host compile of the product's math headers."""
    import psl_slam_amd as P
    L = load()
    i, a, b, o0, o1 = P.math_arrays(fn, a, b)
    L.pso_math_eval.argtypes = [C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    rc = L.pso_math_eval(i, len(a), _p(a), None if b is None else _p(b), _p(o0), None if o1 is None else _p(o1))
    assert rc == 0, f"pso_math_eval({fn}) -> {rc}"
    return o0 if o1 is None else (o0, o1)


LSD_RECT_FIELDS = ("x1", "y1", "x2", "y2", "width", "x", "y", "theta", "dx", "dy", "prec", "p")


def lsd_rects(img, cap=20000):
    """The rectangles LSD hands to rect_improve (LSD_REFINE_ADV), in seed order: (n, 12) float64."""
    L = load()
    img = np.ascontiguousarray(img)
    h, w = img.shape
    r = np.zeros((cap, 12), np.float64)
    L.pso_lsd_rects.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = L.pso_lsd_rects(_p(img), w, h, img.strides[0], _p(r), cap)
    return r[:n].copy()


# ---- sequential checkers of the device projections (oracle/project_oracle.cpp, oracle/line_project_oracle.cpp) ------
# Poses, cameras, map points and map lines are passed as the records of psl_slam_amd (POSE_DTYPE, CAMERA_DTYPE, ...).
def _c(a):
    return None if a is None else np.ascontiguousarray(a)


def _sizes(name, n):
    fn = getattr(load(), name)
    sz = np.zeros(n, np.int32)
    fn.argtypes = [C.c_void_p]
    fn(_p(sz))
    return sz


def pr_sizes():
    """sizeof(PslPose), PslLastPoint, PslMapPointGeom, PslProjQuery as the checker's compiler sees them."""
    return _sizes("pr_sizes", 4)


def pr_vo_select(depth, th_depth):
    """UpdateLastFrame's selection: (number of keypoints visited, sel[i] = 1 for the visited ones)."""
    L = load()
    depth = np.ascontiguousarray(depth, np.float32)
    sel = np.zeros(max(len(depth), 1), np.uint8)
    L.pr_vo_select.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
    n = L.pr_vo_select(_p(depth), len(depth), float(th_depth), _p(sel))
    return n, sel[:len(depth)]


def pr_predict_level(ratio, log_scale_factor, nlevels):
    L = load()
    L.pr_predict_level.argtypes = [C.c_float, C.c_float, C.c_int]
    return L.pr_predict_level(float(ratio), float(log_scale_factor), nlevels)


def pr_level_sweep(lo, hi, log_scale_factor, nlevels):
    """Every float ratio in [lo, hi]: (levels that differ between psl_log and the host's log, ratios visited)."""
    L = load()
    n = C.c_long()
    L.pr_level_sweep.restype = C.c_long
    L.pr_level_sweep.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int, C.POINTER(C.c_long)]
    bad = L.pr_level_sweep(float(lo), float(hi), float(log_scale_factor), nlevels, C.byref(n))
    return bad, n.value


def pr_project_last(kps, desc, depth, Tlw, Tcw, points, mpdesc, cam, scale, th, th_depth, mono, vo, bounds):
    """The query rows of SearchByProjection(CurrentFrame, LastFrame): (queries, qdesc, owner)."""
    L = load()
    kps, desc, depth, Tlw, Tcw, points, mpdesc, cam = (_c(a) for a in (kps, desc, depth, Tlw, Tcw, points, mpdesc, cam))
    scale, b = np.ascontiguousarray(scale, np.float32), np.asarray(bounds, np.float32)
    n = len(kps)
    q = np.zeros(max(n, 1), PROJQUERY_DTYPE)
    qd = np.zeros((max(n, 1), 32), np.uint8)
    ow = np.zeros(max(n, 1), np.int32)
    L.pr_project_last.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_float, C.c_float, C.c_int, C.c_int] + \
        [C.c_void_p] * 4
    nq = L.pr_project_last(_p(kps), _p(desc), _p(depth), n, _p(Tlw), _p(Tcw), _p(points), _p(mpdesc), _p(cam), _p(scale), len(scale), th,
                           th_depth, int(mono), int(vo), _p(b), _p(q), _p(qd), _p(ow))
    return q[:nq], qd[:nq], ow[:nq]


def pr_project_frustum(Tcw, mp, mpdesc, cam, scale, log_scale_factor, view_cos_limit, th, bounds):
    """isInFrustum + the query rows of SearchByProjection(F, vpMapPoints): (queries, qdesc, owner, inview, level, viewcos)."""
    L = load()
    Tcw, mp, mpdesc, cam = (_c(a) for a in (Tcw, mp, mpdesc, cam))
    scale, b = np.ascontiguousarray(scale, np.float32), np.asarray(bounds, np.float32)
    n = len(mp)
    m = max(n, 1)
    q, qd = np.zeros(m, PROJQUERY_DTYPE), np.zeros((m, 32), np.uint8)
    ow, iv, lv, vc = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.int32), np.zeros(m, np.float32)
    L.pr_project_frustum.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int, C.c_float, C.c_float, C.c_float] + \
        [C.c_void_p] * 7
    nq = L.pr_project_frustum(_p(Tcw), _p(mp), _p(mpdesc), n, _p(cam), _p(scale), len(scale), log_scale_factor, view_cos_limit, th, _p(b),
                              _p(q), _p(qd), _p(ow), _p(iv), _p(lv), _p(vc))
    return q[:nq], qd[:nq], ow[:nq], iv[:n], lv[:n], vc[:n]


def lr_sizes():
    """sizeof(PslMapLineGeom), PslLastLine, PslLineQuery as the checker's compiler sees them."""
    return _sizes("lr_sizes", 3)


def lr_level(ratio, lsf, how):
    """MapLine::PredictScale; how: 0 = the library's logf, 1 = the host's logf, 2 = the point projections' double path."""
    L = load()
    L.lr_level.argtypes = [C.c_float, C.c_float, C.c_int]
    return L.lr_level(float(ratio), float(lsf), how)


def lr_level_sweep(lo, hi, lsf):
    """Every float ratio in [lo, hi]: (ratios visited, [levels that differ from the host's logf, from the double path])."""
    L = load()
    flips = np.zeros(2, np.int64)
    L.lr_level_sweep.restype = C.c_long
    L.lr_level_sweep.argtypes = [C.c_float, C.c_float, C.c_float, C.c_void_p]
    n = L.lr_level_sweep(float(lo), float(hi), float(lsf), _p(flips))
    return n, flips


def lr_in_frustum(G, T, cam, bounds, limit, lsf):
    """Frame::isInFrustum of one map line: (in view, [u1, v1, u2, v2, viewCos], level)."""
    L = load()
    G, T, cam, b = _c(G), _c(T), _c(cam), np.asarray(bounds, np.float32)
    out = np.zeros(5, np.float32)
    lvl = C.c_int32()
    L.lr_in_frustum.argtypes = [C.c_void_p] * 4 + [C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    got = L.lr_in_frustum(_p(G), _p(T), _p(cam), _p(b), float(limit), float(lsf), _p(out), C.byref(lvl))
    return got, out, lvl.value


def lr_project_frustum(Tcw, ml, mldesc, cam, log_scale_factor, view_cos_limit, th, bounds):
    """isInFrustum + the query rows of SearchByProjection(F, vpMapLines): (queries, qdesc, owner, inview, level, viewcos)."""
    L = load()
    Tcw, ml, mldesc, cam, b = _c(Tcw), _c(ml), np.ascontiguousarray(mldesc, np.uint8), _c(cam), np.asarray(bounds, np.float32)
    n = len(ml)
    m = max(n, 1)
    q, qd = np.zeros(m, LINEQUERY_DTYPE), np.zeros((m, 32), np.uint8)
    ow, iv, lv, vc = np.zeros(m, np.int32), np.zeros(m, np.uint8), np.zeros(m, np.int32), np.zeros(m, np.float32)
    L.lr_project_frustum.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_float, C.c_float, C.c_float] + [C.c_void_p] * 7
    nq = L.lr_project_frustum(_p(Tcw), _p(ml), _p(mldesc), n, _p(cam), log_scale_factor, view_cos_limit, th, _p(b), _p(q), _p(qd), _p(ow),
                              _p(iv), _p(lv), _p(vc))
    return q[:nq], qd[:nq], ow[:nq], iv[:n], lv[:n], vc[:n]


def lr_project_last(kls, ldesc, lines, mldesc, Tcw, cam, th, bounds):
    """The query rows of SearchByProjection(CurrentFrame, LastFrame) of the last frame's lines: (queries, qdesc, owner)."""
    L = load()
    kls, ldesc, lines, Tcw, cam, b = _c(kls), _c(ldesc), _c(lines), _c(Tcw), _c(cam), np.asarray(bounds, np.float32)
    md = None if mldesc is None else np.ascontiguousarray(mldesc, np.uint8)
    n = len(kls)
    q, qd, ow = np.zeros(max(n, 1), LINEQUERY_DTYPE), np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.int32)
    L.lr_project_last.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 4 + [C.c_float] + [C.c_void_p] * 4
    nq = L.lr_project_last(_p(kls), _p(ldesc), n, _p(lines), _p(md), _p(Tcw), _p(cam), th, _p(b), _p(q), _p(qd), _p(ow))
    return q[:nq], qd[:nq], ow[:nq]


# ---- sequential checkers of the stereo constructor and the monocular initialiser (oracle/stereo_oracle.cpp, mono_init_oracle.cpp)
def restate_stereo(kL, dL, kR, dR, levL, levR, scale, inv_scale, bf, fx):
    """(uright, depth, idx_right, sad) of the restatement.  levL / levR: level images (2-D uint8 arrays of any row pitch)."""
    L = load()
    kL, kR = np.ascontiguousarray(kL, KEYPOINT_DTYPE), np.ascontiguousarray(kR, KEYPOINT_DTYPE)
    dL = np.ascontiguousarray(dL, np.uint8).reshape(-1, 32)
    dR = np.ascontiguousarray(dR, np.uint8).reshape(-1, 32)
    nl = len(levL)
    ptr = lambda levs: (C.c_void_p * nl)(*[lv.ctypes.data for lv in levs])
    pit = lambda levs: np.array([lv.strides[0] for lv in levs], np.int32)
    for a, b in zip(levL, levR):
        assert a.shape == b.shape and a.strides[1] == 1 and b.strides[1] == 1
    lw = np.array([lv.shape[1] for lv in levL], np.int32)
    lh = np.array([lv.shape[0] for lv in levL], np.int32)
    pL, pR, sL, sR = ptr(levL), ptr(levR), pit(levL), pit(levR)
    sc, isc = np.ascontiguousarray(scale, np.float32), np.ascontiguousarray(inv_scale, np.float32)
    n = len(kL)
    ur, dep = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    idx, sad = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    L.sr_stereo.argtypes = [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_float, C.c_float] + \
        [C.c_void_p] * 4
    L.sr_stereo(_p(kL), _p(dL), n, _p(kR), _p(dR), len(kR), C.cast(pL, C.c_void_p), _p(sL), C.cast(pR, C.c_void_p), _p(sR), _p(lw), _p(lh),
                _p(sc), _p(isc), nl, float(bf), float(fx), _p(ur), _p(dep), _p(idx), _p(sad))
    return ur[:n], dep[:n], idx[:n], sad[:n]


def restate_grid(kps, bounds):
    """CSR of the frame grid as the monocular checker builds it: (start[64 * 48 + 1], idx)."""
    L = load()
    kps = np.ascontiguousarray(kps, KEYPOINT_DTYPE)
    b = np.asarray(bounds, np.float32)
    start = np.zeros(64 * 48 + 1, np.int32)
    idx = np.zeros(max(len(kps), 1), np.int32)
    L.mr_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    n = L.mr_grid(_p(kps), len(kps), _p(b), _p(start), _p(idx))
    return start, idx[:n]


def restate_search(k1, d1, k2, d2, bounds2, prev, window=100, nnratio=0.9, check_ori=True):
    """(nmatches, matches12, prev after the call, accepted) of the restatement; `prev` itself is not modified."""
    L = load()
    k1, k2 = np.ascontiguousarray(k1, KEYPOINT_DTYPE), np.ascontiguousarray(k2, KEYPOINT_DTYPE)
    d1 = np.ascontiguousarray(d1, np.uint8).reshape(-1, 32)
    d2 = np.ascontiguousarray(d2, np.uint8).reshape(-1, 32)
    b = np.asarray(bounds2, np.float32)
    pv = np.array(prev, np.float32).reshape(-1, 2).copy()
    n1 = len(k1)
    m12 = np.zeros(max(n1, 1), np.int32)
    acc = np.zeros(max(n1, 1), np.int32)
    L.mr_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                            C.c_int, C.c_void_p, C.c_void_p]
    nm = L.mr_search(_p(k1), _p(d1), n1, _p(k2), _p(d2), len(k2), _p(b), _p(pv), int(window), float(nnratio), int(bool(check_ori)), _p(m12),
                     _p(acc))
    return nm, m12[:n1], pv, acc[:n1]
