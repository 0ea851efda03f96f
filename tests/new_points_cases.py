"""LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:275-520) and CreateNewMapLines2 (:522-759) restated in numpy from the reference
text, operation by operation with the widths psl-slam_amd/csrc/triangulate_kernels.h states, and the cases the tests run: a general
scene, one hand-built pair per branch and gate, and the order dependence between neighbours.  Pure numpy: float operations are
numpy float32 scalars, double operations float64; atan2f / cosf are the host libm's (the float overloads the reference's translation
unit picks), the float Jacobi SVD is tests/initializer_cases.jacobi.

A point case is a dict: kf1 (P.TRIKEYFRAME_DTYPE[1]), cur (keysun, keys, uright, depth, taken, desc), nb (P.TRINEIGHBOUR_DTYPE[K]),
store[k] (kps, desc, uright of neighbour k's slot), neigh[k] (fidx, taken, keys, depth), q[k] / idx1[k] / qd[k] (the query list built
from the state at the call), sf / sig2, only_stereo, check_ori.  create_points(case) is the literal loop of the reference: neighbour after
neighbour, SearchForTriangulation with the GetMapPoint state of the moment, then the pairs in the order of vMatchedPairs."""
import ctypes as C

import numpy as np

from initializer_cases import jacobi
from window_cases import KEYPOINT_DTYPE, T, keypoints

F, D = np.float32, np.float64
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")
_libm = C.CDLL("libm.so.6")
_libm.atan2f.restype = _libm.cosf.restype = C.c_float
_libm.atan2f.argtypes = [C.c_float, C.c_float]
_libm.cosf.argtypes = [C.c_float]

POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,))])
TRIKEYFRAME_DTYPE = np.dtype([("Tcw", POSE_DTYPE)] + [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "mb", "mbf", "ratio_factor")] + [("kf", "<i4")])
TRINEIGHBOUR_DTYPE = np.dtype([("active", "<i4"), ("slot", "<i4"), ("kf", "<i4"), ("kf_first", "<i4"), ("F12", "<f4", (9,)), ("ex", "<f4"), ("ey", "<f4"),
                               ("Tcw", POSE_DTYPE)] + [(k, "<f4") for k in ("fx", "fy", "cx", "cy", "mb")])
TRIQUERY_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("x", "<f4"), ("y", "<f4"), ("angle", "<f4"), ("stereo", "<i4")])
NEWMAPPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("k", "<i4"), ("idx1", "<i4"), ("idx2", "<i4")])
NEWMAPLINE_DTYPE = np.dtype([("sp", "<f4", (3,)), ("ep", "<f4", (3,)), ("k", "<i4"), ("idx1", "<i4"), ("idx2", "<i4")])
KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                          ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                          ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                          ("lineLength", "<f4"), ("numOfPixels", "<i4")])
ST = {n: i for i, n in enumerate(("CREATED", "NO_MATCH", "TAKEN", "INACTIVE", "W_ZERO", "UNPROJECT_EMPTY", "LOW_PARALLAX", "DEPTH1", "DEPTH2",
                                  "REPROJ1_MONO", "REPROJ1_STEREO", "REPROJ2_MONO", "REPROJ2_STEREO", "DIST_ZERO", "RATIO"))}
STL = {n: i for i, n in enumerate(("CREATED", "NO_MATCH", "TAKEN", "INACTIVE", "IDX2_RANGE", "NO_STEREO", "DEPTH_SP1", "DEPTH_EP1", "DEPTH_SP2",
                                   "DEPTH_EP2", "REPROJ_SP1", "REPROJ_EP1", "REPROJ_SP2", "REPROJ_EP2", "DIST_ZERO", "RATIO"))}
POINT_ROW_STATUS = [v for n, v in ST.items() if n not in ("NO_MATCH", "TAKEN", "INACTIVE")]    # what psl_tri_point_row returns
LINE_ROW_STATUS = [v for n, v in STL.items() if n not in ("NO_MATCH", "TAKEN", "INACTIVE", "IDX2_RANGE")]
TH_LOW, HISTO = 50, 30
LEVELS = 16


# ---- the conventions above PslPose -------------------------------------------------------------------------------------------------
def affine(m, x, t):
    """one row of M*x + t: the double sum in index order of the exact products, + the double of t, rounded once"""
    return F(((D(m[0]) * D(x[0]) + D(m[1]) * D(x[1])) + D(m[2]) * D(x[2])) + D(t))


def dot(a, b):
    return (D(a[0]) * D(b[0]) + D(a[1]) * D(b[1])) + D(a[2]) * D(b[2])


def norm_d(a):
    return np.sqrt(dot(a, a))


class Cam:
    """a keyframe as both bodies read it: Rcw, tcw, Ow = -Rcw.t()*tcw, fx fy cx cy, invfx = 1.0f/fx, mb"""

    def __init__(self, pose, fx, fy, cx, cy, mb):
        self.R = np.asarray(pose["R"], F).reshape(3, 3).copy()
        self.t = np.asarray(pose["t"], F).reshape(3).copy()
        with np.errstate(**_ERR):
            self.Ow = np.array([-affine(self.R[:, r], self.t, F(0)) for r in range(3)], F)
            self.fx, self.fy, self.cx, self.cy, self.mb = F(fx), F(fy), F(cx), F(cy), F(mb)
            self.invfx, self.invfy = F(1) / self.fx, F(1) / self.fy

    def to_world(self, xc):                       # Twc.rowRange(0,3).colRange(0,3)*xc + Twc.rowRange(0,3).col(3)
        return np.array([affine(self.R[:, r], xc, self.Ow[r]) for r in range(3)], F)

    def row(self, r, p):                          # Rcw.row(r).dot(x3Dt) + tcw(r), assigned to a float
        return F(dot(self.R[r], p) + D(self.t[r]))

    def dist(self, p):                            # cv::norm(x3D - Ow)
        return F(norm_d(np.array([p[0] - self.Ow[0], p[1] - self.Ow[1], p[2] - self.Ow[2]], F)))


def cam_of(row):
    return Cam(row["Tcw"], row["fx"], row["fy"], row["cx"], row["cy"], row["mb"])


def reproj_mono(C_, p, z, u0, v0, sigma2):
    x, y = C_.row(0, p), C_.row(1, p)
    invz = F(D(1.0) / D(z))
    u, v = (C_.fx * x) * invz + C_.cx, (C_.fy * y) * invz + C_.cy
    ex, ey = u - F(u0), v - F(v0)
    return bool(D(ex * ex + ey * ey) > D(5.991) * D(sigma2))


def reproj_stereo(C_, mbf, p, z, u0, v0, ur0, sigma2):
    x, y = C_.row(0, p), C_.row(1, p)
    invz = F(D(1.0) / D(z))
    u = (C_.fx * x) * invz + C_.cx
    u_r = u - F(mbf) * invz
    v = (C_.fy * y) * invz + C_.cy
    ex, ey, er = u - F(u0), v - F(v0), u_r - F(ur0)
    return bool(D((ex * ex + ey * ey) + er * er) > D(7.8) * D(sigma2))


def ratio_out(ratio_dist, ratio_factor, ratio_octave):
    return bool(ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor)


def tables(c):
    sf, s2 = np.zeros(LEVELS, F), np.zeros(LEVELS, F)
    sf[:len(c["sf"])], s2[:len(c["sig2"])] = c["sf"], c["sig2"]
    return sf, s2


def cos_parallax_rays(C1, C2, u1, v1, u2, v2):
    xn1 = np.array([(F(u1) - C1.cx) * C1.invfx, (F(v1) - C1.cy) * C1.invfy, F(1)], F)
    xn2 = np.array([(F(u2) - C2.cx) * C2.invfx, (F(v2) - C2.cy) * C2.invfy, F(1)], F)
    ray1 = np.array([affine(C1.R[:, r], xn1, F(0)) for r in range(3)], F)
    ray2 = np.array([affine(C2.R[:, r], xn2, F(0)) for r in range(3)], F)
    return F(dot(ray1, ray2) / (norm_d(ray1) * norm_d(ray2))), xn1, xn2


# ---- :354-499 for one pair ------------------------------------------------------------------------------------------------------------
def point_row(C1, C2, mbf1, o1, o2, sf, sig2, ratio_factor):
    """o = (ux, uy, rawx, rawy, uright, depth, octave) -> (status, x3d)"""
    with np.errstate(**_ERR):
        zero = np.zeros(3, F)
        st1, st2 = bool(F(o1[4]) >= 0), bool(F(o2[4]) >= 0)
        cos_rays, xn1, xn2 = cos_parallax_rays(C1, C2, o1[0], o1[1], o2[0], o2[1])
        cs1 = cs2 = cos_rays + F(1)
        if st1:
            cs1 = F(_libm.cosf(F(2) * F(_libm.atan2f(C1.mb / F(2), F(o1[5])))))
        elif st2:
            cs2 = F(_libm.cosf(F(2) * F(_libm.atan2f(C2.mb / F(2), F(o2[5])))))
        cs = cs2 if cs2 < cs1 else cs1
        if cos_rays < cs and cos_rays > 0 and (st1 or st2 or D(cos_rays) < D(0.9998)):
            A = np.zeros((4, 4), F)
            T1, T2 = np.hstack([C1.R, C1.t.reshape(3, 1)]), np.hstack([C2.R, C2.t.reshape(3, 1)])
            A[0], A[1] = xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1]
            A[2], A[3] = xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]
            At = np.ascontiguousarray(A.T).reshape(4, 4, 1).copy()
            _, V = jacobi(At, True)
            x = V[3, :, 0]
            if x[3] == 0:
                return ST["W_ZERO"], zero
            inv = D(1.0) / D(x[3])
            p = np.array([F(D(x[k]) * inv) for k in range(3)], F)
        elif st1 and cs1 < cs2:
            z = F(o1[5])
            if not z > 0:
                return ST["UNPROJECT_EMPTY"], zero
            p = C1.to_world(np.array([((F(o1[2]) - C1.cx) * z) * C1.invfx, ((F(o1[3]) - C1.cy) * z) * C1.invfy, z], F))
        elif st2 and cs2 < cs1:
            z = F(o2[5])
            if not z > 0:
                return ST["UNPROJECT_EMPTY"], zero
            p = C2.to_world(np.array([((F(o2[2]) - C2.cx) * z) * C2.invfx, ((F(o2[3]) - C2.cy) * z) * C2.invfy, z], F))
        else:
            return ST["LOW_PARALLAX"], zero
        z1 = C1.row(2, p)
        if z1 <= 0:
            return ST["DEPTH1"], p
        z2 = C2.row(2, p)
        if z2 <= 0:
            return ST["DEPTH2"], p
        s1 = sig2[int(o1[6]) & (LEVELS - 1)]
        if not st1:
            if reproj_mono(C1, p, z1, o1[0], o1[1], s1):
                return ST["REPROJ1_MONO"], p
        elif reproj_stereo(C1, mbf1, p, z1, o1[0], o1[1], o1[4], s1):
            return ST["REPROJ1_STEREO"], p
        s2 = sig2[int(o2[6]) & (LEVELS - 1)]
        if not st2:
            if reproj_mono(C2, p, z2, o2[0], o2[1], s2):
                return ST["REPROJ2_MONO"], p
        elif reproj_stereo(C2, mbf1, p, z2, o2[0], o2[1], o2[4], s2):     # mpCurrentKeyFrame->mbf, :474
            return ST["REPROJ2_STEREO"], p
        d1, d2 = C1.dist(p), C2.dist(p)
        if d1 == 0 or d2 == 0:
            return ST["DIST_ZERO"], p
        if ratio_out(d2 / d1, F(ratio_factor), sf[int(o1[6]) & (LEVELS - 1)] / sf[int(o2[6]) & (LEVELS - 1)]):
            return ST["RATIO"], p
        return ST["CREATED"], p


# ---- ORBmatcher::SearchForTriangulation src/ORBmatcher.cc:657-823 -------------------------------------------------------------------
def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def rot_bin(a1, a2):
    rot = F(a1) - F(a2)
    if rot < 0:
        rot = rot + F(360)
    v = float(rot * F(1.0 / HISTO))
    b = int(np.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))          # roundf: halves away from zero
    return 0 if b == HISTO else b


def three_maxima(hist):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F(max2) < F(0.1) * F(max1):
        ind2 = ind3 = -1
    elif F(max3) < F(0.1) * F(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search(kps2, desc2, uright2, taken2, fidx2, q, qd, skip, F12, epipole, only_stereo, check_ori, sf, sig2):
    """-> (nmatches, match per query); skip[q]: pKF1->GetMapPoint(idx1) by now (:699-703)"""
    match = np.full(len(q), -1, np.int32)
    hist = [0] * HISTO
    Fm = np.asarray(F12, F).reshape(9)
    n2 = min(len(kps2), len(taken2))
    for qi in range(len(q)):
        if skip[qi]:
            continue
        x, y = F(q["x"][qi]), F(q["y"][qi])
        a, b, c = (x * Fm[0] + y * Fm[3]) + Fm[6], (x * Fm[1] + y * Fm[4]) + Fm[7], (x * Fm[2] + y * Fm[5]) + Fm[8]
        den = a * a + b * b
        start = max(int(q["start"][qi]), 0)
        ln = min(int(q["len"][qi]), len(fidx2) - start)
        best_dist, best = TH_LOW, -1
        for j in range(ln):
            i2 = int(fidx2[start + j])
            if i2 < 0 or i2 >= n2 or taken2[i2]:
                continue
            stereo2 = bool(uright2[i2] >= 0)
            if only_stereo and not stereo2:
                continue
            dist = hamming(qd[qi], desc2[i2])
            if dist > TH_LOW or dist > best_dist:
                continue
            octave = int(kps2["octave"][i2]) & (LEVELS - 1)
            if not q["stereo"][qi] and not stereo2:
                dx, dy = F(epipole[0]) - kps2["x"][i2], F(epipole[1]) - kps2["y"][i2]
                if dx * dx + dy * dy < F(100) * sf[octave]:
                    continue
            num = (a * kps2["x"][i2] + b * kps2["y"][i2]) + c
            if den == 0:
                continue
            if not D((num * num) / den) < D(3.84) * D(sig2[octave]):
                continue
            best, best_dist = i2, dist
        match[qi] = best
        if best >= 0 and check_ori:
            hist[rot_bin(q["angle"][qi], kps2["angle"][best])] += 1
    if check_ori:
        keep = three_maxima(hist)
        for qi in range(len(q)):
            if match[qi] >= 0 and rot_bin(q["angle"][qi], kps2["angle"][match[qi]]) not in keep:
                match[qi] = -1
    return int((match >= 0).sum()), match


# ---- :305-519 ---------------------------------------------------------------------------------------------------------------------------
def create_points(c, apply_taken_late=False):
    """the reference loop on a point case -> the dict KeyFrameMatcher.CreateNewMapPoints returns.  apply_taken_late: the WRONG order (the
    features taken by earlier neighbours dropped behind the rotation histogram), for the test that tells the two apart."""
    K, cur = len(c["nb"]), c["cur"]
    N1 = len(cur["keysun"])
    nqmax = max([len(q) for q in c["q"]] + [0])
    sf, sig2 = tables(c)
    kf1 = c["kf1"][0]
    C1 = cam_of(kf1)
    out = {"match": np.full((K, nqmax), -1, np.int32), "status": np.full((K, nqmax), ST["NO_MATCH"], np.int32), "x3d": np.zeros((K, nqmax, 3), F),
           "nmatches": np.zeros(K, np.int32), "created_by": np.full(N1, -1, np.int32)}
    taken = np.array(cur["taken"], np.uint8) != 0
    new = []
    for k in range(K):
        nb, q, idx1 = c["nb"][k], c["q"][k], c["idx1"][k]
        if not nb["active"]:
            out["status"][k, :len(q)] = ST["INACTIVE"]
            continue
        skip = taken[idx1] if len(q) else np.zeros(0, bool)
        st, ng = c["store"][k], c["neigh"][k]
        nm, match = search(st["kps"], st["desc"], st["uright"], ng["taken"], ng["fidx"], q, c["qd"][k], np.zeros(len(q), bool) if apply_taken_late else skip,
                           nb["F12"], (nb["ex"], nb["ey"]), c["only_stereo"], c["check_ori"], sf, sig2)
        if apply_taken_late:
            match[skip] = -1
            nm = int((match >= 0).sum())
        out["nmatches"][k] = nm
        out["match"][k, :len(q)] = match
        out["status"][k, :len(q)][skip] = ST["TAKEN"]
        C2 = cam_of(nb)
        pairs = sorted((int(idx1[qi]), qi) for qi in range(len(q)) if match[qi] >= 0)        # vMatchedPairs: idx1 ascending
        for i1, qi in pairs:
            i2 = int(match[qi])
            o1 = (cur["keysun"]["x"][i1], cur["keysun"]["y"][i1], cur["keys"][i1][0], cur["keys"][i1][1], cur["uright"][i1], cur["depth"][i1],
                  cur["keysun"]["octave"][i1])
            o2 = (st["kps"]["x"][i2], st["kps"]["y"][i2], ng["keys"][i2][0], ng["keys"][i2][1], st["uright"][i2], ng["depth"][i2], st["kps"]["octave"][i2])
            s, p = point_row(C1, C2, kf1["mbf"], o1, o2, sf, sig2, kf1["ratio_factor"])
            out["status"][k, qi], out["x3d"][k, qi] = s, p
            if s == ST["CREATED"]:
                taken[i1] = True
                out["created_by"][i1] = k
                new.append((p[0], p[1], p[2], k, i1, i2))
    out["new"] = np.array(new, NEWMAPPOINT_DTYPE).reshape(-1)
    return out


def observation_runs(c, r, n1, octaves):
    """obs_off, obs_kf, ref_kf, ref_level as the device forms write them for the list r["new"]"""
    nnew = len(r["new"])
    kf1 = int(c["kf1"][0]["kf"])
    off = np.array([2 * min(i, nnew) for i in range(n1 + 1)], np.int32)
    okf = np.zeros(2 * nnew, np.int32)
    for j, p in enumerate(r["new"]):
        nb = c["nb"][int(p["k"])]
        okf[2 * j], okf[2 * j + 1] = (nb["kf"], kf1) if nb["kf_first"] else (kf1, nb["kf"])
    return off, okf, np.full(nnew, kf1, np.int32), np.array([octaves[int(p["idx1"])] for p in r["new"]], np.int32)


# ---- :599-735 for one pair, :554-757 behind the search ------------------------------------------------------------------------------
def obtain_line(C_, l3d):
    return C_.to_world(np.asarray(l3d[:3], D).astype(F)), C_.to_world(np.asarray(l3d[3:], D).astype(F))


def line_row(C1, C2, kl1, kl2, l3d1, l3d2, stereo1, stereo2, sf, sig2, ratio_factor):
    with np.errstate(**_ERR):
        zero = np.zeros(3, F)
        if stereo1:
            sp, ep = obtain_line(C1, l3d1)
        elif stereo2:
            sp, ep = obtain_line(C2, l3d2)
        else:
            return STL["NO_STEREO"], zero, zero
        zsp1 = C1.row(2, sp)
        if zsp1 <= 0:
            return STL["DEPTH_SP1"], sp, ep
        zep1 = C1.row(2, ep)
        if zep1 <= 0:
            return STL["DEPTH_EP1"], sp, ep
        zsp2 = C2.row(2, sp)
        if zsp2 <= 0:
            return STL["DEPTH_SP2"], sp, ep
        zep2 = C2.row(2, ep)
        if zep2 <= 0:
            return STL["DEPTH_EP2"], sp, ep
        s1 = sig2[int(kl1["octave"]) & (LEVELS - 1)]
        if reproj_mono(C1, sp, zsp1, kl1["startPointX"], kl1["startPointY"], s1):
            return STL["REPROJ_SP1"], sp, ep
        if reproj_mono(C1, ep, zep1, kl1["endPointX"], kl1["endPointY"], s1):
            return STL["REPROJ_EP1"], sp, ep
        s2 = sig2[int(kl2["octave"]) & (LEVELS - 1)]
        if reproj_mono(C2, sp, zsp2, kl2["startPointX"], kl2["startPointY"], s2):
            return STL["REPROJ_SP2"], sp, ep
        if reproj_mono(C2, ep, zep2, kl2["endPointX"], kl2["endPointY"], s2):
            return STL["REPROJ_EP2"], sp, ep
        dsp1, dep1, dsp2, dep2 = C1.dist(sp), C1.dist(ep), C2.dist(sp), C2.dist(ep)
        if dsp1 == 0 or dep1 == 0 or dsp2 == 0 or dep2 == 0:
            return STL["DIST_ZERO"], sp, ep
        ro = sf[int(kl1["octave"]) & (LEVELS - 1)] / sf[int(kl2["octave"]) & (LEVELS - 1)]
        if ratio_out(dsp2 / dsp1, F(ratio_factor), ro) or ratio_out(dep2 / dep1, F(ratio_factor), ro):
            return STL["RATIO"], sp, ep
        return STL["CREATED"], sp, ep


def create_lines(c, match0):
    """a line case (kf1, nb, cur: keylines, lines3d, lineeq; neigh[k]: keylines, lines3d; sf, sig2) and match0 [K, NL1] = the rows of
    LSDmatcher::SearchForTriangulation with the GetMapLine state at the call -> the dict KeyFrameMatcher.CreateNewMapLines returns.
    Neighbour after neighbour: the search's filter drops the pairs whose line of KF1 has its map line by now."""
    K, cur = len(c["nb"]), c["cur"]
    n1 = len(cur["keylines"])
    sf, sig2 = tables(c)
    kf1 = c["kf1"][0]
    C1 = cam_of(kf1)
    out = {"match": np.full((K, n1), -1, np.int32), "status": np.full((K, n1), STL["NO_MATCH"], np.int32), "sp": np.zeros((K, n1, 3), F),
           "ep": np.zeros((K, n1, 3), F), "nmatches": np.zeros(K, np.int32), "created_by": np.full(n1, -1, np.int32)}
    has = np.zeros(n1, bool)
    new = []
    for k in range(K):
        nb, ng = c["nb"][k], c["neigh"][k]
        if not nb["active"]:
            out["status"][k] = STL["INACTIVE"]
            continue
        C2 = cam_of(nb)
        for i in range(n1):
            j = int(match0[k][i])
            if j < 0 or j >= len(ng["keylines"]):
                continue
            if has[i]:
                out["status"][k, i] = STL["TAKEN"]
                continue
            out["match"][k, i] = j
            out["nmatches"][k] += 1
            if j >= n1:
                out["status"][k, i] = STL["IDX2_RANGE"]
                continue
            s, sp, ep = line_row(C1, C2, cur["keylines"][i], ng["keylines"][j], cur["lines3d"][i], ng["lines3d"][j], cur["lineeq"][i] > 0,
                                 cur["lineeq"][j] > 0, sf, sig2, kf1["ratio_factor"])       # mpCurrentKeyFrame->mvLineEq[idx2], :607
            out["status"][k, i], out["sp"][k, i], out["ep"][k, i] = s, sp, ep
            if s == STL["CREATED"]:
                has[i] = True
                out["created_by"][i] = k
                new.append((sp, ep, k, i, j))
    out["new"] = np.array(new, NEWMAPLINE_DTYPE).reshape(-1)
    return out


# ==== cases ==============================================================================================================================
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
SF = np.array([1.2 ** i for i in range(8)], F)
SIG2 = (SF * SF).astype(F)
FAR = (-3000.0, -3000.0)
F_DY = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], F)      # x1' F12 = (0, 1, -y1): the distance to the epipolar line is |y2 - y1|
ROT_Y90 = np.array([0, 0, -1, 0, 1, 0, 1, 0, 0], F)   # Rcw of a camera that looks along +x: Rwc*(0,0,1) = (1,0,0)


def pose(R=None, t=(0, 0, 0)):
    p = np.zeros((), POSE_DTYPE)
    p["R"], p["t"] = np.eye(3, dtype=F).reshape(9) if R is None else np.asarray(R, F).reshape(9), np.asarray(t, F)
    return p


def keyframe1(T_=None, mb=0.1, mbf=50.0, kf=0, ratio=1.5 * 1.2):
    k = np.zeros(1, TRIKEYFRAME_DTYPE)
    k["Tcw"], k["fx"], k["fy"], k["cx"], k["cy"], k["mb"], k["mbf"], k["ratio_factor"], k["kf"] = pose() if T_ is None else T_, FX, FY, CX, CY, mb, mbf, ratio, kf
    return k


def neighbour(T_, slot, kf, F12=F_DY, epipole=FAR, active=1, mb=0.1, kf_first=0):
    n = np.zeros((), TRINEIGHBOUR_DTYPE)
    n["active"], n["slot"], n["kf"], n["kf_first"], n["F12"], n["ex"], n["ey"], n["Tcw"] = active, slot, kf, kf_first, F12, epipole[0], epipole[1], T_
    n["fx"], n["fy"], n["cx"], n["cy"], n["mb"] = FX, FY, CX, CY, mb
    return n


def project(T_, X):
    """pixel of the world point X in the camera T_ (double arithmetic, rounded to float: an input, not a restated step)"""
    R, t = np.asarray(T_["R"], D).reshape(3, 3), np.asarray(T_["t"], D)
    xc = R @ np.asarray(X, D) + t
    return F(FX * xc[0] / xc[2] + CX), F(FY * xc[1] / xc[2] + CY), F(xc[2])


class Builder:
    """KF1 and K neighbours, features added pair by pair: every pair has its own vocabulary node, so a query's run holds exactly the
    features it is meant to see"""

    def __init__(self, kf1, nbs, only_stereo=False, check_ori=False, sf=SF, sig2=SIG2):
        self.kf1, self.nb = kf1, np.array(nbs, TRINEIGHBOUR_DTYPE).reshape(-1)
        K = len(self.nb)
        self.f1 = []                                   # (ux, uy, rawx, rawy, ur, depth, octave, angle, desc, taken)
        self.f2 = [[] for _ in range(K)]               # (ux, uy, rawx, rawy, ur, depth, octave, angle, desc, taken)
        self.fidx = [[] for _ in range(K)]
        self.q = [[] for _ in range(K)]                # (start, len, idx1)
        self.opt = dict(only_stereo=only_stereo, check_ori=check_ori, sf=np.asarray(sf, F), sig2=np.asarray(sig2, F))
        self.want = {}                                 # (k, idx1) -> status name, written down from the construction

    def feat1(self, u, v, desc, ur=-1.0, depth=-1.0, octave=0, angle=0.0, raw=None, taken=0):
        self.f1.append((u, v, *(raw or (u, v)), ur, depth, octave, angle, desc, taken))
        return len(self.f1) - 1

    def feat2(self, k, u, v, desc, ur=-1.0, depth=-1.0, octave=0, angle=0.0, raw=None, taken=0):
        self.f2[k].append((u, v, *(raw or (u, v)), ur, depth, octave, angle, desc, taken))
        return len(self.f2[k]) - 1

    def ask(self, k, i1, cands, want=None):
        """feature i1 of KF1 meets the features `cands` of neighbour k under one node"""
        self.q[k].append((len(self.fidx[k]), len(cands), i1))
        self.fidx[k] += list(cands)
        if want is not None:
            self.want[(k, i1)] = want

    def pair(self, k, uv1, uv2, d, want=None, **kw):
        """one new feature in KF1 and one in neighbour k with the same descriptor T(d); kw: ur1, depth1, oct1, raw1, ang1 and the same with 2"""
        g = lambda n, dflt: kw.get(n, dflt)
        i1 = self.feat1(*uv1, T(d), g("ur1", -1.0), g("depth1", -1.0), g("oct1", 0), g("ang1", 0.0), g("raw1", None))
        i2 = self.feat2(k, *uv2, T(d), g("ur2", -1.0), g("depth2", -1.0), g("oct2", 0), g("ang2", 0.0), g("raw2", None))
        self.ask(k, i1, [i2], want)
        return i1, i2

    def world(self, k, X, d, want=None, **kw):
        """a pair that sees the world point X: both keypoints are its projections"""
        u1, v1, _ = project(self.kf1[0]["Tcw"], X)
        u2, v2, _ = project(self.nb[k]["Tcw"], X)
        return self.pair(k, (u1, v1), (u2, v2), d, want, **kw)

    def case(self, name):
        K = len(self.nb)
        f1 = self.f1
        cur = {"keysun": keypoints([(f[0], f[1]) for f in f1] or np.zeros((0, 2)), octave=np.array([f[6] for f in f1], np.int32),
                                   angle=np.array([f[7] for f in f1], F)),
               "keys": np.array([(f[2], f[3]) for f in f1], F).reshape(-1, 2), "uright": np.array([f[4] for f in f1], F),
               "depth": np.array([f[5] for f in f1], F), "taken": np.array([f[9] for f in f1], np.uint8),
               "desc": np.array([f[8] for f in f1], np.uint8).reshape(-1, 32)}
        store, neigh, qs, i1s, qds = [], [], [], [], []
        for k in range(K):
            f2 = self.f2[k]
            store.append({"kps": keypoints([(f[0], f[1]) for f in f2] or np.zeros((0, 2)), octave=np.array([f[6] for f in f2], np.int32),
                                           angle=np.array([f[7] for f in f2], F)),
                          "desc": np.array([f[8] for f in f2], np.uint8).reshape(-1, 32), "uright": np.array([f[4] for f in f2], F)})
            neigh.append({"fidx": np.array(self.fidx[k], np.int32), "taken": np.array([f[9] for f in f2], np.uint8),
                          "keys": np.array([(f[2], f[3]) for f in f2], F).reshape(-1, 2), "depth": np.array([f[5] for f in f2], F)})
            q = np.zeros(len(self.q[k]), TRIQUERY_DTYPE)
            i1 = np.array([e[2] for e in self.q[k]], np.int32)
            for j, (s, ln, i) in enumerate(self.q[k]):
                q[j] = (s, ln, cur["keysun"]["x"][i], cur["keysun"]["y"][i], cur["keysun"]["angle"][i], int(cur["uright"][i] >= 0))
            qs.append(q); i1s.append(i1); qds.append(cur["desc"][i1].reshape(-1, 32))
        return dict(name=name, kf1=self.kf1, cur=cur, nb=self.nb, store=store, neigh=neigh, q=qs, idx1=i1s, qd=qds, want=dict(self.want), **self.opt)


def T_x(b, R=None):
    """a camera whose centre is (b, 0, 0) with rotation R (Rcw): tcw = -R*(b, 0, 0)"""
    Rm = np.eye(3) if R is None else np.asarray(R, D).reshape(3, 3)
    return pose(Rm, -(Rm @ np.array([b, 0.0, 0.0])))


def gates_case():
    """One pair per branch and gate of :354-499.  KF1 is the world frame; neighbour 0 sits 0.2 to the right (wide baseline: the SVD branch),
    neighbour 1 0.02 to the right (narrower than the stereo baseline mb = 0.1: the UnprojectStereo branches), neighbour 2 looks along +x
    from (-4, 0, 4) (rays at right angles), neighbour 3 has a NaN in its pose, neighbour 4 equals neighbour 0 with mb2 = 0.3.  All points
    lie in the plane Y = 0, so every keypoint has v = cy and F_DY lets every intended pair through the epipolar gate."""
    nbs = [neighbour(T_x(0.2), 0, 1), neighbour(T_x(0.02), 1, 2), neighbour(pose(ROT_Y90, -(ROT_Y90.reshape(3, 3).astype(D) @ np.array([-4.0, 0, 4.0]))), 2, 3),
           neighbour(T_x(0.2), 3, 4), neighbour(T_x(0.2), 4, 5, mb=0.3), neighbour(pose(None, (0.0, 0.0, -5.0)), 5, 6),
           neighbour(T_x(0.2), 6, 7, active=0)]
    nbs[3]["Tcw"]["R"][1] = np.nan
    b = Builder(keyframe1(mbf=50.0), nbs)
    d = iter(range(1, 250))
    z_of = lambda ur_, u: F(50.0) / (F(u) - F(ur_))
    # neighbour 0: mono / mono through the SVD
    b.world(0, (0.3, 0.0, 4.0), next(d), "CREATED")
    b.world(0, (0.0, 0.0, 9.5), next(d), "CREATED")                       # cos just under 0.9998
    b.world(0, (0.0, 0.0, 10.5), next(d), "LOW_PARALLAX")                 # cos just over 0.9998
    u1, v1, _ = project(b.kf1[0]["Tcw"], (0.3, 0, 4.0)); u2, v2, _ = project(nbs[0]["Tcw"], (0.3, 0, 4.0))
    b.pair(0, (u1 + 8, v1), (u2, v2), next(d), "CREATED")                  # rays in one plane always meet: a wrong disparity is a nearer point
    b.pair(0, (u1, v1 + 3), (u2, v2 - 3), next(d), "REPROJ1_MONO", oct2=7)   # 6 px of vertical disparity pass the epipolar gate of level 7 only
    b.pair(0, (u1, v1), (u2 + 60, v2), next(d), "DEPTH1")                 # negative disparity: the rays meet behind the cameras
    b.world(0, (0.3, 0.0, 4.0), next(d), "RATIO", oct1=7, oct2=0)         # ratioOctave = 1.2^7 > ratioDist * 1.8
    # stereo in KF1 with the wide baseline: SVD branch, stereo gate in KF1
    X = (0.2, 0.0, 3.0)
    u1, v1, z1 = project(b.kf1[0]["Tcw"], X)
    b.world(0, X, next(d), "CREATED", ur1=float(u1 - F(50.0) / z1), depth1=float(z1))
    b.world(0, X, next(d), "REPROJ1_STEREO", ur1=float(u1 - F(50.0) / z1) + 9.0, depth1=float(z1))
    # stereo in the neighbour alone, different mbf in the two keyframes: the right-image term uses KF1's mbf = 50 (:474)
    u2, v2, z2 = project(nbs[0]["Tcw"], X)
    b.world(0, X, next(d), "CREATED", ur2=float(u2 - F(50.0) / z2), depth2=float(z2))          # consistent with KF1's mbf: passes
    b.world(0, X, next(d), "REPROJ2_STEREO", ur2=float(u2 - F(150.0) / z2), depth2=float(z2))  # consistent with pKF2's own mbf = 150: rejected
    # neighbour 1, narrow baseline: UnprojectStereo of KF1 / of KF2
    X = (0.1, 0.0, 3.0)
    u1, v1, z1 = project(b.kf1[0]["Tcw"], X); u2, v2, z2 = project(nbs[1]["Tcw"], X)
    b.world(1, X, next(d), "CREATED", ur1=float(u1 - F(50.0) / z1), depth1=float(z1))
    b.world(1, X, next(d), "CREATED", ur2=float(u2 - F(50.0) / z2), depth2=float(z2))
    b.world(1, X, next(d), "CREATED", ur1=float(u1 - F(50.0) / z1), depth1=float(z1), ur2=float(u2 - F(50.0) / z2), depth2=float(z2))   # both: c1 < c2
    b.world(1, X, next(d), "UNPROJECT_EMPTY", ur1=5.0, depth1=0.0)
    b.world(1, X, next(d), "UNPROJECT_EMPTY", ur2=5.0, depth2=-1.0)
    b.world(1, X, next(d), "CREATED", ur1=float(u1 - F(50.0) / z1), depth1=float(z1), raw1=(float(u1) + 0.5, float(v1)))  # mvKeys, not mvKeysUn
    b.world(1, X, next(d), "REPROJ1_STEREO", ur1=float(u1 - F(50.0) / z1), depth1=float(z1), raw1=(float(u1) + 40.0, float(v1)))
    b.world(1, X, next(d), "REPROJ2_MONO", ur1=float(u1 - F(50.0) / F(1.0)), depth1=1.0)   # a wrong but self-consistent depth: pKF2 sees it 6.7 px off
    b.world(1, (0.0, 0.0, 200.0), next(d), "LOW_PARALLAX")                # mono / mono, cos ~ 1
    # neighbour 2, rays at right angles through the principal points: cosParallaxRays == 0
    b.pair(2, (CX, CY), (CX, CY), next(d), "LOW_PARALLAX")                                  # mono: cos > 0 fails, no stereo
    b.pair(2, (CX, CY), (CX, CY), next(d), "LOW_PARALLAX", ur1=1.0, depth1=1.0e30)          # stereo1 alone: c1 = cosf(2*atan2f(0.05, 1e30)) = 1 = c2
    # both stereo: `if(bStereo1) ... else if(bStereo2)` (:379-382) leaves cosParallaxStereo2 = cosParallaxRays + 1 although bStereo2 is true
    b.pair(2, (CX, CY), (CX, CY), next(d), "LOW_PARALLAX", ur1=1.0, depth1=1.0e30, ur2=1.0, depth2=4.0)   # equal cosines, 1 == 0 + 1: no branch
    Xo = (-1.0, 0.0, 4.0)                         # seen at 104 degrees between the rays: cos = -0.24, c2 = 0.76 < c1: UnprojectStereo of pKF2
    uo1, _, zo1 = project(b.kf1[0]["Tcw"], Xo); uo2, _, zo2 = project(nbs[2]["Tcw"], Xo)
    b.world(2, Xo, next(d), "CREATED", ur1=float(uo1 - F(50.0) / zo1), depth1=float(zo1), ur2=float(uo2 - F(50.0) / zo2), depth2=float(zo2))
    b.pair(2, (CX, CY), (CX, CY), next(d), "CREATED", ur1=float(CX - 50.0 / 4.0), depth1=4.0, ur2=float(CX - 50.0 / 4.0), depth2=4.0)   # c1 < c2 = 1
    b.pair(2, (CX - 100, CY), (CX + 100, CY), next(d), None, ur2=1.0, depth2=4.0)           # cos < 0: stereo2 alone, c2 < c1
    # neighbour 3: NaN in the pose
    b.world(0, (0.3, 0.0, 4.0), next(d), "CREATED")
    u1, v1, _ = project(b.kf1[0]["Tcw"], (0.3, 0, 4.0)); u2, v2, _ = project(nbs[0]["Tcw"], (0.3, 0, 4.0))
    b.pair(3, (u1, v1), (u2, v2), next(d), None)
    # neighbour 4: stereo2 alone reads pKF2->mb
    X = (0.2, 0.0, 3.0)
    u2, v2, z2 = project(nbs[4]["Tcw"], X)
    b.world(4, X, next(d), "CREATED", ur2=float(u2 - F(50.0) / z2), depth2=float(z2))
    # neighbour 5 stands 5 ahead of KF1 on its axis: the rays meet at (0.5, 0, 3), in front of KF1 and behind pKF2
    b.pair(5, (float(F(CX) + F(500.0 * 0.5 / 3.0)), CY), (CX - 125.0, CY), next(d), "DEPTH2")
    # neighbour 6 failed the baseline gate
    b.world(6, (0.3, 0.0, 4.0), next(d), "INACTIVE")
    return b.case("gates")


def degenerate_case():
    """x3D[3] == 0 and a zero distance need poses no SetPose would produce (a proper pose gives parallel rays cos = 1, which never enter
    the SVD branch, and z = 0 at its own centre); the pose is an input like any other.
      neighbour 0: Rcw = [1 0 s; 0 1 0; 0 0 1] (a shear, s = 0.05), tcw = (-0.2, 0, 0), keypoints (cx, cy) and (cx + fx*s, cy): the third
                   column of A is exactly zero, a rank-deficient A whose null vector is (0, 0, 1, 0), while the rays are 2.9 degrees apart.
      neighbour 1: Rcw = diag(1, 1, 2), tcw = (0, 0, -1): Ow2 = (0, 0, 2), where z2 = 3 > 0.  KF1 sees a stereo point on its axis at depth
                   2: UnprojectStereo gives exactly Ow2."""
    s_ = 0.05
    nbs = [neighbour(pose([1, 0, s_, 0, 1, 0, 0, 0, 1], (-0.2, 0.0, 0.0)), 0, 1), neighbour(pose([1, 0, 0, 0, 1, 0, 0, 0, 2], (0.0, 0.0, -1.0)), 1, 2)]
    b = Builder(keyframe1(), nbs)
    b.pair(0, (CX, CY), (float(F(CX) + F(FX) * F(s_)), CY), 1, "W_ZERO")
    b.pair(1, (CX, CY), (CX, CY), 2, "DIST_ZERO", ur1=float(F(CX) - F(50.0) * F(1.0 / 2.0)), depth1=2.0)
    return b.case("degenerate")


def _angles_pair(b, k, X, d, ang, want=None, i1=None):
    """a pair on the world point X whose rotation difference is `ang` degrees; i1: an existing feature of KF1 meets a new one of neighbour k"""
    u2, v2, _ = project(b.nb[k]["Tcw"], X)
    if i1 is None:
        u1, v1, _ = project(b.kf1[0]["Tcw"], X)
        i1 = b.feat1(u1, v1, T(d), angle=ang)
    i2 = b.feat2(k, u2, v2, b.f1[i1][8])
    b.ask(k, i1, [i2], want)
    return i1, i2


def order_case(K=3):
    """The dependence between neighbours, with the rotation check on.  Neighbours 0..2 sit 0.2, 0.3, 0.4 to the right.
      a  created by neighbour 0, has a passing match in neighbour 1: TAKEN there.
      h  neighbour 1's histogram is {bin 0: a + 2 others = 3, bin 4: 3, bin 8: 3, bin 12: 3} with a counted and {2, 3, 3, 3} without:
         ComputeThreeMaxima keeps bins 0, 4, 8 with a (strict >: the first three of equal counts) and 4, 8, 12 without, so the three
         features of bin 12 are created by neighbour 1 only if a is dropped BEFORE the histogram, and the two others of bin 0 only if
         it is dropped behind it.
      s  two features of KF1 take the same idx2 of neighbour 0; both are created.
      g  rejected by a reprojection gate in neighbour 0, no query in neighbour 1, created in neighbour 2."""
    nbs = [neighbour(T_x(0.2 + 0.1 * k), k, k + 1) for k in range(K)]
    b = Builder(keyframe1(), nbs, check_ori=True)
    d = iter(range(1, 250))
    note = {}
    X = lambda j: (0.05 * j - 0.3, 0.0, 3.0 + 0.1 * j)
    a, _ = _angles_pair(b, 0, X(0), next(d), 0.0, "CREATED")
    note["a"] = a
    if K > 1:
        _angles_pair(b, 1, X(0), 200, 0.0, "TAKEN", i1=a)
        note["bin0"] = [_angles_pair(b, 1, X(1 + j), next(d), 0.0, "NO_MATCH")[0] for j in range(2)]
        for bin_, name in ((4, "bin4"), (8, "bin8"), (12, "bin12")):
            note[name] = [_angles_pair(b, 1, X(3 + bin_ + j), next(d), 30.0 * bin_, "CREATED")[0] for j in range(3)]
    # two features of KF1 on one feature of neighbour 0
    u1, v1, _ = project(b.kf1[0]["Tcw"], X(20)); u2, v2, _ = project(nbs[0]["Tcw"], X(20))
    s1, s2 = b.feat1(u1, v1, T(100)), b.feat1(u1, v1, T(101))
    i2 = b.feat2(0, u2, v2, T(100))
    b.ask(0, s1, [i2], "CREATED"); b.ask(0, s2, [i2], "CREATED")
    note["same_idx2"] = (s1, s2, i2)
    if K > 2:
        u1, v1, _ = project(b.kf1[0]["Tcw"], X(21)); u2, v2, _ = project(nbs[0]["Tcw"], X(21)); u3, v3, _ = project(nbs[2]["Tcw"], X(21))
        g = b.feat1(u1, v1 + 3.0, T(110))
        b.ask(0, g, [b.feat2(0, u2, v2 - 3.0, T(110), octave=7)], "REPROJ1_MONO")   # 6 px of vertical disparity: through the epipolar gate of level 7
        b.ask(2, g, [b.feat2(2, u3, v3 + 3.0, T(110))], "CREATED")
        note["g"] = g
    c = b.case(f"order-K{K}")
    c["note"] = note
    return c


def _rot(rx, ry, rz):
    cx_, sx, cy_, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]]) @
            np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]]))


def f12_of(T1, T2):
    """ComputeF12 src/LocalMapping.cc:998-1014 in double, rounded: an input of the call"""
    R1, t1 = np.asarray(T1["R"], D).reshape(3, 3), np.asarray(T1["t"], D)
    R2, t2 = np.asarray(T2["R"], D).reshape(3, 3), np.asarray(T2["t"], D)
    R12, t12 = R1 @ R2.T, -R1 @ R2.T @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    Km = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]])
    return (np.linalg.inv(Km).T @ tx @ R12 @ np.linalg.inv(Km)).astype(F).reshape(9)


def general_case(seed=5, npts=60, K=3, nq_pad=None, name=None, stereo_every=4, inactive=()):
    """A seeded scene: npts world points in front of KF1, K neighbours with baselines 0.2 .. and small rotations, every point seen by
    KF1 and by about two thirds of the neighbours with sub-pixel noise, every `stereo_every`-th feature with a right coordinate and a
    depth; the true F12 and epipole; 10 vocabulary nodes.  Some features of KF1 have a map point already."""
    rng = np.random.default_rng(seed)
    kf1 = keyframe1(pose(_rot(0.01, -0.02, 0.005), (0.02, -0.01, 0.03)), mbf=50.0)
    nbs = []
    for k in range(K):
        R = _rot(*(rng.uniform(-0.03, 0.03, 3)))
        c = np.array([0.2 + 0.12 * k, rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)]) * (1 if k % 2 == 0 else -1)
        T2 = pose(R, -(R @ c))
        F12 = f12_of(kf1[0]["Tcw"], T2)
        R2 = np.asarray(T2["R"], D).reshape(3, 3)
        c1 = -np.asarray(kf1[0]["Tcw"]["R"], D).reshape(3, 3).T @ np.asarray(kf1[0]["Tcw"]["t"], D)    # the epipole: KF1's centre in pKF2
        e = R2 @ c1 + np.asarray(T2["t"], D)
        nbs.append(neighbour(T2, k, k + 1, F12=F12, epipole=(FX * e[0] / e[2] + CX, FY * e[1] / e[2] + CY), active=0 if k in inactive else 1,
                             kf_first=k % 2))
    b = Builder(kf1, nbs, check_ori=True)
    pts = np.stack([rng.uniform(-1.5, 1.5, npts), rng.uniform(-1.0, 1.0, npts), rng.uniform(2.5, 7.0, npts)], 1)
    descs = rng.integers(0, 256, (npts, 32), dtype=np.uint8)
    node_of = rng.integers(0, 10, npts)
    i1_of, fvec2 = [], []
    for j in range(npts):
        u, v, z = project(kf1[0]["Tcw"], pts[j])
        u, v = u + F(rng.normal(0, 0.3)), v + F(rng.normal(0, 0.3))
        st = j % stereo_every == 0
        i1_of.append(b.feat1(u, v, descs[j], ur=float(u - F(50.0) / z) if st else -1.0, depth=float(z) if st else -1.0, octave=int(rng.integers(0, 3)),
                             angle=float(rng.uniform(0, 360)), taken=int(j % 11 == 0)))
    for k in range(K):
        seen = [j for j in range(npts) if rng.uniform() < 0.67]
        i2_of = {}
        for j in seen:
            u, v, z = project(nbs[k]["Tcw"], pts[j])
            if z <= 0.5:
                continue
            u, v = u + F(rng.normal(0, 0.3)), v + F(rng.normal(0, 0.3))
            st = (j + k) % stereo_every == 1
            a1 = b.f1[i1_of[j]][7]
            i2_of[j] = b.feat2(k, u, v, descs[j], ur=float(u - F(50.0) / z) if st else -1.0, depth=float(z) if st else -1.0,
                               octave=b.f1[i1_of[j]][6], angle=float((a1 + (5.0 if j % 9 else 95.0)) % 360.0), taken=int(j % 13 == 5))
        fvec2.append([])
        for node in range(10):                      # FeatureVector order: node ascending, feature index ascending
            cands = [i2_of[j] for j in sorted(i2_of) if node_of[j] == node]
            if cands:
                fvec2[k].append((node, cands))
            for j in range(npts):
                if node_of[j] == node and not b.f1[i1_of[j]][9] and cands:
                    b.q[k].append((len(b.fidx[k]), len(cands), i1_of[j]))
            b.fidx[k] += cands
    c = b.case(name or f"general-s{seed}-n{npts}-K{K}")
    c["fvec1"] = [(node, [i1_of[j] for j in range(npts) if node_of[j] == node]) for node in range(10) if (node_of == node).any()]
    c["fvec2"] = fvec2
    if nq_pad:                                      # queries without candidates, to reach a query count
        for k in range(K):
            have = set(c["idx1"][k].tolist())
            extra = [i for i in range(len(c["cur"]["keysun"])) if i not in have][:max(nq_pad - len(c["q"][k]), 0)]
            q = np.zeros(len(extra), TRIQUERY_DTYPE)
            q["x"], q["y"] = c["cur"]["keysun"]["x"][extra], c["cur"]["keysun"]["y"][extra]
            c["q"][k] = np.concatenate([c["q"][k], q]); c["idx1"][k] = np.concatenate([c["idx1"][k], np.array(extra, np.int32)])
            c["qd"][k] = np.concatenate([c["qd"][k], c["cur"]["desc"][extra].reshape(-1, 32)])
    return c


def count_case(nq, n1=None):
    """nq queries against one neighbour (the trips of the finish stage: 63 / 64 / 65, 1023 / 1024 / 1025, N1 = 4096): feature i of KF1 and
    feature i % 64 of the neighbour see a world point of a small grid; every fifth query has no candidate."""
    n1 = n1 or max(nq, 1)
    nbs = [neighbour(T_x(0.25), 0, 1)]
    b = Builder(keyframe1(), nbs, check_ori=True)
    X = [(0.1 * (j % 8) - 0.4, 0.0, 3.0 + 0.2 * (j // 8)) for j in range(64)]
    for j in range(64):
        u2, v2, _ = project(nbs[0]["Tcw"], X[j])
        b.feat2(0, u2, v2, T(3 * j), angle=0.0)
    for i in range(n1):
        u1, v1, _ = project(b.kf1[0]["Tcw"], X[i % 64])
        b.feat1(u1, v1, T(3 * (i % 64)))
    for i in range(nq):
        b.ask(0, i, [i % 64] if i % 5 != 4 else [])
    return b.case(f"count-nq{nq}-n{n1}")


def write_point_case(path, c):
    """the file tools/dropin/newpoints_main.cpp reads (its header comment states the layout)"""
    K, N1 = len(c["nb"]), len(c["cur"]["keysun"])
    nqmax = max([len(q) for q in c["q"]] + [0])
    with open(path, "wb") as f:
        f.write(np.array([0, K, N1, nqmax, len(c["sf"]), int(c["only_stereo"]), int(c["check_ori"])], np.int32).tobytes())
        f.write(np.asarray(c["sf"], F).tobytes()); f.write(np.asarray(c["sig2"], F).tobytes())
        f.write(c["kf1"].tobytes())
        cur = c["cur"]
        for a, t in ((cur["keysun"], KEYPOINT_DTYPE), (cur["keys"], F), (cur["uright"], F), (cur["depth"], F), (cur["taken"], np.uint8), (cur["desc"], np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())
        f.write(np.ascontiguousarray(c["nb"], TRINEIGHBOUR_DTYPE).tobytes())
        for k in range(K):
            st, ng = c["store"][k], c["neigh"][k]
            f.write(np.array([len(st["kps"]), len(ng["fidx"]), len(c["q"][k])], np.int32).tobytes())
            for a, t in ((st["kps"], KEYPOINT_DTYPE), (st["desc"], np.uint8), (st["uright"], F), (ng["fidx"], np.int32), (ng["taken"], np.uint8),
                         (ng["keys"], F), (ng["depth"], F), (c["q"][k], TRIQUERY_DTYPE), (c["idx1"][k], np.int32), (c["qd"][k], np.uint8)):
                f.write(np.ascontiguousarray(a, t).tobytes())


def read_point_section(f, c):
    """one form's outputs as newpoints_main writes them -> the dict of create_points"""
    K, N1 = len(c["nb"]), len(c["cur"]["keysun"])
    nqmax = max([len(q) for q in c["q"]] + [0])
    rd = lambda t, n: np.frombuffer(f.read(np.dtype(t).itemsize * n), t).copy()
    out = {"match": rd(np.int32, K * nqmax).reshape(K, nqmax), "status": rd(np.int32, K * nqmax).reshape(K, nqmax),
           "x3d": rd(F, K * nqmax * 3).reshape(K, nqmax, 3), "nmatches": rd(np.int32, K), "created_by": rd(np.int32, N1)}
    nnew = int(rd(np.int32, 1)[0])
    out["new"] = rd(NEWMAPPOINT_DTYPE, nnew)
    return out


def assert_same_points(got, ref, what):
    for key in ("nmatches", "match", "status", "created_by"):
        assert np.array_equal(got[key], ref[key]), (what, key, got[key], ref[key])
    assert got["x3d"].tobytes() == ref["x3d"].tobytes(), (what, "x3d", np.argwhere(got["x3d"].view(np.uint32) != ref["x3d"].view(np.uint32))[:5])
    assert got["new"].tobytes() == ref["new"].tobytes(), (what, "new", got["new"], ref["new"])


# ---- line cases -------------------------------------------------------------------------------------------------------------------------
def keyline(sp, ep, octave=0):
    k = np.zeros((), KEYLINE_DTYPE)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"], k["octave"], k["class_id"] = sp[0], sp[1], ep[0], ep[1], octave, -1
    return k


class LineBuilder:
    """lines of KF1 and of K neighbours; a pair is made by giving both the same random LBD row (distance 0, everybody else ~128 away),
    so the search's answer follows from the construction: match0"""

    def __init__(self, kf1, nbs, seed=3):
        self.kf1, self.nb = kf1, np.array(nbs, TRINEIGHBOUR_DTYPE).reshape(-1)
        self.rng = np.random.default_rng(seed)
        self.l1, self.l2 = [], [[] for _ in nbs]      # (keyline, lines3d, lineeq | -, desc)
        self.pairs, self.want = {}, {}

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def cam_line(self, T_, Xs, Xe):
        """the segment Xs-Xe (world) in the camera T_: (keyline, its 6 camera-frame doubles)"""
        R, t = np.asarray(T_["R"], D).reshape(3, 3), np.asarray(T_["t"], D)
        a, e = R @ np.asarray(Xs, D) + t, R @ np.asarray(Xe, D) + t
        px = lambda x: (F(FX * x[0] / x[2] + CX), F(FY * x[1] / x[2] + CY))
        return (px(a), px(e)), np.concatenate([a, e])

    def line1(self, kl, l3d, lineeq, desc):
        self.l1.append((keyline(*kl[:2], octave=kl[2] if len(kl) > 2 else 0), np.asarray(l3d, D), F(lineeq), desc))
        return len(self.l1) - 1

    def line2(self, k, kl, l3d, desc):
        self.l2[k].append((keyline(*kl[:2], octave=kl[2] if len(kl) > 2 else 0), np.asarray(l3d, D), desc))
        return len(self.l2[k]) - 1

    def filler1(self, lineeq=-1.0):
        return self.line1(((10.0, 10.0), (20.0, 20.0)), np.zeros(6), lineeq, self.desc())

    def filler2(self, k):
        return self.line2(k, ((10.0, 10.0), (20.0, 20.0)), np.zeros(6), self.desc())

    def world(self, k, Xs, Xe, want, lineeq=1.0, i1=None, oct1=0, oct2=0, shift1=(0, 0, 0, 0), shift2=(0, 0, 0, 0), l3d1=None):
        """a matched pair on the world segment; shift: pixels added to (sx, sy, ex, ey) of the keyline"""
        kl2, c2 = self.cam_line(self.nb[k]["Tcw"], Xs, Xe)
        d = self.desc() if i1 is None else self.l1[i1][3]
        if i1 is None:
            kl1, c1 = self.cam_line(self.kf1[0]["Tcw"], Xs, Xe)
            kl1 = ((kl1[0][0] + shift1[0], kl1[0][1] + shift1[1]), (kl1[1][0] + shift1[2], kl1[1][1] + shift1[3]), oct1)
            i1 = self.line1(kl1, c1 if l3d1 is None else l3d1, lineeq, d)
        kl2 = ((kl2[0][0] + shift2[0], kl2[0][1] + shift2[1]), (kl2[1][0] + shift2[2], kl2[1][1] + shift2[3]), oct2)
        i2 = self.line2(k, kl2, c2, d)
        self.pairs[(k, i1)] = i2
        if want is not None:
            self.want[(k, i1)] = want
        return i1, i2

    def case(self, name):
        K, n1 = len(self.nb), len(self.l1)
        cur = {"keylines": np.array([l[0] for l in self.l1], KEYLINE_DTYPE).reshape(-1), "lines3d": np.array([l[1] for l in self.l1], D).reshape(-1, 6),
               "lineeq": np.array([l[2] for l in self.l1], F), "ldesc": np.array([l[3] for l in self.l1], np.uint8).reshape(-1, 32),
               "has_mapline": np.zeros(n1, np.uint8)}
        neigh = [{"keylines": np.array([l[0] for l in self.l2[k]], KEYLINE_DTYPE).reshape(-1), "lines3d": np.array([l[1] for l in self.l2[k]], D).reshape(-1, 6),
                  "ldesc": np.array([l[2] for l in self.l2[k]], np.uint8).reshape(-1, 32), "has_mapline": np.zeros(len(self.l2[k]), np.uint8)} for k in range(K)]
        match0 = np.full((K, n1), -1, np.int32)
        for (k, i1), i2 in self.pairs.items():
            match0[k, i1] = i2
        return dict(name=name, kf1=self.kf1, nb=self.nb, cur=cur, neigh=neigh, match0=match0, want=dict(self.want), sf=SF, sig2=SIG2)


def line_gates_case():
    """One pair per gate of :599-735 against neighbour 0 (0.3 to the right); the taken chain over neighbours 0..2; the bStereo2 oddity;
    idx2 >= NL1; an empty neighbour (3) and an inactive one (4); neighbours 5 and 6 for the depth gates of pKF2 and the zero distance."""
    nbs = [neighbour(T_x(0.3), 0, 1), neighbour(T_x(-0.3), 1, 2, kf_first=1), neighbour(T_x(0.5), 2, 3), neighbour(T_x(0.7), 3, 4),
           neighbour(T_x(0.9), 4, 5, active=0), neighbour(pose(None, (0.0, 0.0, -5.0)), 5, 6),
           neighbour(pose([1, 0, 0, 0, 1, 0, 0, 0, 2], (0.0, 0.0, -1.0)), 6, 7)]
    b = LineBuilder(keyframe1(), nbs)
    S, E = (-0.5, -0.2, 4.0), (0.6, 0.3, 5.0)
    for k in (0, 1, 2, 5, 6):                             # fillers so that a KNN of two always exists and idx2 < NL1 has lines to point at
        for _ in range(3):
            b.filler2(k)
    f_mono = [b.filler1(-1.0) for _ in range(2)]          # lines 0, 1 of KF1: mvLineEq[.][2] <= 0
    f_st = b.filler1(1.0)                                 # line 2: > 0
    # the chain: created by 0, taken in 1 and 2
    a, _ = b.world(0, S, E, "CREATED")
    b.world(1, S, E, "TAKEN", i1=a); b.world(2, S, E, "TAKEN", i1=a)
    # rejected by 0 (reprojection of the start point in pKF2), created by 1, taken in 2
    r, _ = b.world(0, S, (0.7, 0.3, 5.0), "REPROJ_SP2", shift2=(9, 0, 0, 0))
    b.world(1, S, (0.7, 0.3, 5.0), "CREATED", i1=r); b.world(2, S, (0.7, 0.3, 5.0), "TAKEN", i1=r)
    b.world(0, (-0.4, 0.1, 3.0), (0.2, 0.2, 3.5), "REPROJ_EP2", shift2=(0, 0, 0, 9))
    b.world(0, (-0.4, 0.1, 3.0), (0.2, 0.2, 3.6), "REPROJ_SP1", shift1=(0, 9, 0, 0))
    b.world(0, (-0.4, 0.1, 3.0), (0.2, 0.2, 3.7), "REPROJ_EP1", shift1=(0, 0, 9, 0))
    b.world(0, (-0.4, 0.1, 3.0), (0.2, 0.2, 3.8), "RATIO", oct1=7)
    b.world(0, (-0.4, 0.1, 3.0), (0.2, 0.2, 3.9), "DEPTH_SP1", l3d1=(0, 0, -1.0, 0.2, 0.2, 3.9))
    b.world(0, (-0.4, 0.1, 3.0), (0.2, 0.2, 4.1), "DEPTH_EP1", l3d1=(-0.4, 0.1, 3.0, 0, 0, 0.0))
    # neighbour 5 stands 5 ahead of KF1 on its axis: an end point at z = 3 is in front of KF1 and behind it
    b.world(5, (-0.4, 0.1, 3.0), (0.2, 0.2, 7.0), "DEPTH_SP2")
    b.world(5, (-0.4, 0.1, 7.0), (0.2, 0.2, 3.0), "DEPTH_EP2")
    # neighbour 6: Rcw = diag(1, 1, 2), tcw = (0, 0, -1), no pose SetPose would make: its centre (0, 0, 2) has depth 3 in it.  The start point IS the centre
    b.world(6, (0.0, 0.0, 2.0), (0.2, 0.2, 4.0), "DIST_ZERO")
    # bStereo1 false: bStereo2 is KF1's mvLineEq[idx2].  idx2 = 0..2 are the neighbour's fillers; KF1's lines 0, 1 say mono, line 2 stereo
    n0 = len(b.l1)
    i_ns = b.line1(((100.0, 100.0), (150.0, 120.0)), np.zeros(6), -1.0, b.desc())     # KF1 line, mono; its partner is neighbour 0's line 0
    b.l2[0][0] = (b.l2[0][0][0], b.l2[0][0][1], b.l1[i_ns][3]); b.pairs[(0, i_ns)] = 0; b.want[(0, i_ns)] = "NO_STEREO"
    # ... partner is neighbour 0's line 2, KF1's line 2 says stereo: pKF2->obtain3DLine(2) is used although that line is what it is
    kl, c1 = b.cam_line(b.kf1[0]["Tcw"], S, (0.5, 0.25, 4.5))
    kl2, c2 = b.cam_line(nbs[0]["Tcw"], S, (0.5, 0.25, 4.5))
    i_s2 = b.line1(kl, c1, -1.0, b.desc())
    b.l2[0][2] = (keyline(*kl2), c2, b.l1[i_s2][3]); b.pairs[(0, i_s2)] = 2; b.want[(0, i_s2)] = "CREATED"
    # idx2 >= NL1: pad neighbour 2 with lines until an index beyond KF1's count exists
    i_far = b.line1(kl, c1, 1.0, b.desc())
    while len(b.l2[2]) <= len(b.l1) + 2:
        b.filler2(2)
    b.l2[2][-1] = (keyline(*kl2), c2, b.l1[i_far][3]); b.pairs[(2, i_far)] = len(b.l2[2]) - 1; b.want[(2, i_far)] = "IDX2_RANGE"
    c = b.case("line-gates")
    c["note"] = {"chain": a, "second": r, "mono_says": f_mono, "stereo_says": f_st, "n0": n0}
    return c


def write_line_case(path, c):
    K, n1 = len(c["nb"]), len(c["cur"]["keylines"])
    with open(path, "wb") as f:
        f.write(np.array([1, K, n1, 0, len(c["sf"]), 0, 0], np.int32).tobytes())
        f.write(np.asarray(c["sf"], F).tobytes()); f.write(np.asarray(c["sig2"], F).tobytes())
        f.write(c["kf1"].tobytes())
        cur = c["cur"]
        for a, t in ((cur["keylines"], KEYLINE_DTYPE), (cur["lines3d"], D), (cur["lineeq"], F), (cur["ldesc"], np.uint8)):
            f.write(np.ascontiguousarray(a, t).tobytes())
        f.write(np.ascontiguousarray(c["nb"], TRINEIGHBOUR_DTYPE).tobytes())
        for ng in c["neigh"]:
            f.write(np.array([len(ng["keylines"])], np.int32).tobytes())
            for a, t in ((ng["keylines"], KEYLINE_DTYPE), (ng["lines3d"], D), (ng["ldesc"], np.uint8)):
                f.write(np.ascontiguousarray(a, t).tobytes())
        f.write(np.ascontiguousarray(c["match0"], np.int32).tobytes())


def read_line_section(f, c):
    K, n1 = len(c["nb"]), len(c["cur"]["keylines"])
    rd = lambda t, n: np.frombuffer(f.read(np.dtype(t).itemsize * n), t).copy()
    out = {"match": rd(np.int32, K * n1).reshape(K, n1), "status": rd(np.int32, K * n1).reshape(K, n1), "sp": rd(F, K * n1 * 3).reshape(K, n1, 3),
           "ep": rd(F, K * n1 * 3).reshape(K, n1, 3), "nmatches": rd(np.int32, K), "created_by": rd(np.int32, n1)}
    out["new"] = rd(NEWMAPLINE_DTYPE, int(rd(np.int32, 1)[0]))
    return out


def assert_same_lines(got, ref, what):
    for key in ("nmatches", "match", "status", "created_by"):
        assert np.array_equal(got[key], ref[key]), (what, key, got[key], ref[key])
    for key in ("sp", "ep", "new"):
        assert got[key].tobytes() == ref[key].tobytes(), (what, key)


def status_names(table, st):
    inv = {v: k for k, v in table.items()}
    return [inv[int(s)] for s in np.asarray(st).reshape(-1)]
