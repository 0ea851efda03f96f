"""Expected rows and inputs for the device projection of map points into keyframes (tests/test_kf_project_{cpu,gpu}.py).

restate_project is a numpy restatement of the three loops in front of the KeyFrame-rate window searches, written from the reference
lines (src/ORBmatcher.cc needs OpenCV, so it cannot be compiled as an oracle: these rows are "HIP = restatement"):
  mode 0  ORBmatcher::Fuse(pKF, vpMapPoints, th)                          src/ORBmatcher.cc:842-890
  mode 1  Fuse(pKF, Scw, ...) :1000-1050, SearchByProjection(pKF, Scw, ...) :312-360
  mode 2  one direction of SearchBySim3                                    :1148-1189 / :1228-1269
with the conventions of include/pslfe.h: a 3x3 * 3x1 + 3x1 product is the double sum in index order rounded once to float, cv::norm
and Mat::dot are double sums (the norm's sqrt in double, rounded to float), the view gate compares in double, z <= 0 or NaN is
dropped, every other operation is one float operation in the reference's order.  Arithmetic here is float64 with an explicit
np.float32 rounding wherever the convention rounds; float32 numpy operations are single correctly rounded operations.  The level is
the C++ oracle's PredictScale (oracle_lib.pr_predict_level).

The file also holds the scene: 24 poses along a short trajectory, map points unprojected from the keypoints of kf_scene.keyframes()
at random depths and perturbed, normals and distance ranges chosen so that every gate drops something, and constructed rows for the
limit cases."""
import numpy as np

import kf_scene as ks

F32, F64 = np.float32, np.float64
FUSE, SCW, SIM3 = 0, 1, 2
KEPT, SKIP, DEPTH, IMAGE, MIN_DIST, MAX_DIST, VIEW = range(7)      # why a (keyframe, point) pair gives no row
NLEVELS = 8
LOG_SCALE = F32(np.log(F32(1.2)))                                   # mfLogScaleFactor = log(mfScaleFactor) src/ORBextractor.cc
NVIEWS = 24


def camera(fx=525.0, fy=525.0, cx=319.5, cy=239.5, bf=40.0):
    import psl_slam_amd as P
    cam = np.zeros((), P.CAMERA_DTYPE)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["bf"] = fx, fy, cx, cy, bf
    return cam


def affine(R, t, p):
    """rows of R*p + t for p [M, 3] float32: double products (exact), summed in index order, + t, one rounding to float"""
    R, t, p = np.asarray(R, F32).astype(F64).reshape(3, 3), np.asarray(t, F32).astype(F64), np.asarray(p, F32).astype(F64)
    return (((R[:, 0] * p[:, 0:1] + R[:, 1] * p[:, 1:2]) + R[:, 2] * p[:, 2:3]) + t).astype(F32)


def centre(pose):
    """Ow = -Rcw.t()*tcw"""
    R = np.asarray(pose["R"], F32).reshape(3, 3)
    return -affine(R.T, np.zeros(3, F32), np.asarray(pose["t"], F32).reshape(1, 3))[0]


def norm3(p):
    p = p.astype(F64)
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]).astype(F32)


def dot3(p, n):
    p, n = p.astype(F64), n.astype(F64)
    return (p[:, 0] * n[:, 0] + p[:, 1] * n[:, 1]) + p[:, 2] * n[:, 2]


def geometry(view, mp, cam, mode):
    """The per-point values of one keyframe up to the gates: dict of u, v, invz, z, dist (float32) and dot (float64, modes 0 / 1)."""
    pw = np.stack([mp["x"], mp["y"], mp["z"]], 1).astype(F32)
    pc = affine(view["Tcw"]["R"], view["Tcw"]["t"], pw)                          # :853 / :324 / :1159
    if mode == SIM3:
        pc = affine(view["T21"]["R"], view["T21"]["t"], pc)                      # :1160
    z = pc[:, 2]
    with np.errstate(all="ignore"):
        invz = (F32(1.0) / z) if mode == FUSE else (1.0 / z.astype(F64)).astype(F32)   # :859 `1/z`; :1019, :1166 `1.0/z`
        x, y = pc[:, 0] * invz, pc[:, 1] * invz                                  # :860-861
        u, v = F32(cam["fx"]) * x + F32(cam["cx"]), F32(cam["fy"]) * y + F32(cam["cy"])   # :863-864
        if mode == SIM3:
            dist, dot = norm3(pc), None                                          # :1179
        else:
            po = pw - centre(view["Tcw"])                                        # :874
            dist = norm3(po)                                                     # :875
            dot = dot3(po, np.stack([mp["nx"], mp["ny"], mp["nz"]], 1).astype(F32))   # :884
    return dict(u=u, v=v, invz=invz, z=z, dist=dist, dot=dot, pc=pc)


def restate_project(mode, views, mp, cam, bounds, scale, th, skip=None, log_scale=LOG_SCALE):
    """-> (rows PROJQUERY_DTYPE [K, M], level [K, M], reason [K, M]) as pslfe_kf_project gives the first two"""
    import oracle_lib
    import psl_slam_amd as P
    views = np.asarray(views).reshape(-1)
    K, M = len(views), len(mp)
    rows = np.zeros((K, M), P.PROJQUERY_DTYPE)
    level = np.full((K, M), -1, np.int32)
    reason = np.zeros((K, M), np.int32)
    minX, minY, maxX, maxY = (F32(b) for b in bounds)
    scale = np.asarray(scale, F32)
    for k in range(K):
        g = geometry(views[k], mp, cam, mode)
        u, v, dist = g["u"], g["v"], g["dist"]
        with np.errstate(all="ignore"):
            minD, maxD = F32(0.8) * mp["min_dist"], F32(1.2) * mp["max_dist"]   # Get{Min,Max}DistanceInvariance src/MapPoint.cc:373-383
            r = np.zeros(M, np.int32)
            alive = np.ones(M, bool)

            def drop(cond, why):
                hit = alive & cond
                r[hit] = why
                alive[hit] = False

            if skip is not None:
                drop(np.asarray(skip).reshape(K, M)[k] != 0, SKIP)
            drop(~(g["z"] > 0), DEPTH)                                           # :856 `z < 0`; z == 0 and NaN dropped by convention
            drop(~((u >= minX) & (u < maxX) & (v >= minY) & (v < maxY)), IMAGE)  # KeyFrame::IsInImage src/KeyFrame.cc:726-729
            drop(dist < minD, MIN_DIST)                                          # :878
            drop(dist > maxD, MAX_DIST)
            if mode != SIM3:
                drop(g["dot"] < 0.5 * dist.astype(F64), VIEW)                    # :884
            ratio = mp["max_dist"] / dist                                        # MapPoint::PredictScale src/MapPoint.cc:385-400
        reason[k] = r
        idx = np.nonzero(alive)[0]
        lvl = np.array([oracle_lib.pr_predict_level(ratio[i], log_scale, len(scale)) for i in idx], np.int32).reshape(-1)
        level[k, idx] = lvl
        rows["u"][k, idx], rows["v"][k, idx] = u[idx], v[idx]
        rows["ur"][k, idx] = u[idx] - F32(cam["bf"]) * g["invz"][idx]               # :870
        rows["radius"][k, idx] = F32(th) * scale[lvl]                                # :890
        rows["min_level"][k, idx], rows["max_level"][k, idx] = lvl - 1, lvl
        rows["radius"][k][~alive] = -1.0
    return rows, level, reason


# ---- the scene -----------------------------------------------------------------------------------------------------------------

def pose_record(R, t):
    import psl_slam_amd as P
    p = np.zeros((), P.POSE_DTYPE)
    p["R"], p["t"] = np.asarray(R, F32).reshape(9), np.asarray(t, F32)
    return p


def trajectory(n=NVIEWS):
    """world -> camera poses of a camera that slides sideways and turns a little"""
    import project_cases as pc
    out = []
    for k in range(n):
        R = pc.rot(0.004 * k, 0.012 * k - 0.1, 0.006 * k)
        c = np.array([0.035 * k - 0.3, 0.01 * np.sin(0.5 * k), 0.015 * k])       # camera centre in the world
        out.append(pose_record(R, -R @ c))
    return out


def views(nslots=2, n=NVIEWS, sim3_scale=1.05):
    """KFVIEW_DTYPE[n]: Tcw = pose k, slot = k % nslots; T21 = the identity for even k (mode 2 then differs from mode 1 only by its
    own rules: dist = |p3Dc2|, no view gate) and a small similarity for odd k"""
    import psl_slam_amd as P
    import project_cases as pc
    v = np.zeros(n, P.KFVIEW_DTYPE)
    for k, T in enumerate(trajectory(n)):
        v[k]["Tcw"] = T
        v[k]["slot"] = k % nslots
        if k % 2 == 0:
            v[k]["T21"] = pose_record(np.eye(3), np.zeros(3))
        else:
            v[k]["T21"] = pose_record(sim3_scale * pc.rot(0.01, -0.02, 0.005), [0.04, -0.01, 0.02])
    return v


def map_points(M, seed=5, n=NVIEWS):
    """(MAPPOINT_DTYPE[M], descriptors [M, 32]): point i is keypoint j of keyframe (i % n) % 2 unprojected through pose i % n at a random
    depth and perturbed; its normal is the viewing direction of that pose (turned away for some), its distance range puts the
    predicted level anywhere in 0..7 (and outside the invariance region for some); some lie behind the camera."""
    import psl_slam_amd as P
    rng = np.random.default_rng(seed)
    kfs = ks.keyframes()
    tr = trajectory(n)
    cam = camera()
    mp = np.zeros(M, P.MAPPOINT_DTYPE)
    desc = np.zeros((M, 32), np.uint8)
    src = np.arange(M) % n
    for i in range(M):
        T = tr[src[i]]
        kps, d = kfs[src[i] % 2]
        j = rng.integers(0, len(kps))
        z = rng.uniform(0.6, 6.0)
        if rng.random() < 0.05:
            z = -rng.uniform(0.5, 3.0)                                           # behind every camera of the trajectory
        pc = np.array([(kps["x"][j] - cam["cx"]) / cam["fx"] * z, (kps["y"][j] - cam["cy"]) / cam["fy"] * z, z], F64)
        R, t = T["R"].reshape(3, 3).astype(F64), T["t"].astype(F64)
        pw = R.T @ (pc - t) + rng.normal(0, 0.02, 3)
        po = pw - (-R.T @ t)
        dist = np.linalg.norm(po)
        nrm = po / dist
        if rng.random() < 0.10:                                                  # seen from elsewhere: the 60 degree gate
            nrm = rng.normal(0, 1, 3)
            nrm /= np.linalg.norm(nrm)
        lvl = rng.integers(0, NLEVELS)
        maxd = dist * 1.2 ** (lvl - rng.uniform(0.1, 0.9))                       # ceil(log(max / dist) / log 1.2) == lvl from pose src
        mind = maxd / 1.2 ** (NLEVELS - 1)
        w = rng.random()
        if w < 0.05:
            mind = dist * rng.uniform(1.3, 2.0)                                  # closer than the invariance region allows
            maxd = mind * 1.2 ** (NLEVELS - 1)
        elif w < 0.10:
            maxd = dist * rng.uniform(0.3, 0.8)                                  # farther
            mind = maxd / 1.2 ** (NLEVELS - 1)
        mp[i] = (*pw, *nrm, mind, maxd)
        desc[i] = d[j]
    return mp, ks.noisy_desc(desc, rng, flips=12)


def skip_bytes(K, M, seed=9, p=0.05):
    return (np.random.default_rng(seed).random((K, M)) < p).astype(np.uint8)


# ---- limit cases ---------------------------------------------------------------------------------------------------------------

LIMIT_BOUNDS = (0.0, 0.0, 640.0, 480.0)


def limit_camera():
    """fx*x + cx is exact for x = +-0.625: u lands on 0 and on 640 exactly"""
    return camera(512.0, 512.0, 320.0, 240.0, 40.0)


def _solve(fn, target, start):
    """a float32 near `start` with fn(x) == target exactly"""
    lo = hi = F32(start)
    for _ in range(256):
        for c in (lo, hi):
            if fn(c) == F32(target):
                return c
        lo, hi = np.nextafter(lo, F32(-np.inf)), np.nextafter(hi, F32(np.inf))
    raise AssertionError("no float32 solves the limit case")


def limit_cases():
    """(views KFVIEW_DTYPE[2], MAPPOINT_DTYPE[n], names): view 0 is the identity pose (Ow = 0, p3Dc = p3Dw exactly), view 1 a translated
    one.  names[i] = (what, expected reason in view 0 for modes 0 / 1)."""
    import psl_slam_amd as P
    v = np.zeros(2, P.KFVIEW_DTYPE)
    v[0]["Tcw"] = v[0]["T21"] = v[1]["T21"] = pose_record(np.eye(3), np.zeros(3))
    v[1]["Tcw"] = pose_record(np.eye(3), [0.5, 0.0, 0.0])                        # Ow = (-0.5, 0, 0)
    v["slot"] = 0
    rows, names = [], []

    def add(what, expect, p, n=(0, 0, 1), mind=0.1, maxd=100.0):
        rows.append((*p, *n, mind, maxd))
        names.append((what, expect))

    add("u == min_x is kept", KEPT, (-0.625, 0.0, 1.0), (-0.625, 0, 1))
    add("u == max_x is dropped", IMAGE, (0.625, 0.0, 1.0), (0.625, 0, 1))
    add("v == min_y is kept", KEPT, (0.0, -0.46875, 1.0), (0, -0.46875, 1))
    add("v == max_y is dropped", IMAGE, (0.0, 0.46875, 1.0), (0, 0.46875, 1))
    add("z == 0", DEPTH, (0.1, 0.1, 0.0))
    add("z < 0", DEPTH, (0.0, 0.0, -1.0))
    add("NaN x (every row of Rcw*p3Dw is NaN: the depth is)", DEPTH, (np.nan, 0.0, 1.0))
    add("NaN z", DEPTH, (0.0, 0.0, np.nan))
    mind = _solve(lambda m: F32(0.8) * m, 2.0, 2.5)
    add("dist == 0.8f*min_dist is kept", KEPT, (0.0, 0.0, 2.0), mind=mind, maxd=mind * F32(3.0))
    up = np.nextafter(mind, F32(np.inf))
    while not F32(0.8) * up > F32(2.0):
        up = np.nextafter(up, F32(np.inf))
    add("dist just below 0.8f*min_dist is dropped", MIN_DIST, (0.0, 0.0, 2.0), mind=up, maxd=up * F32(3.0))
    maxd = _solve(lambda m: F32(1.2) * m, 3.0, 2.5)
    add("dist == 1.2f*max_dist is kept", KEPT, (0.0, 0.0, 3.0), mind=0.1, maxd=maxd)
    dn = np.nextafter(maxd, F32(-np.inf))
    while not F32(1.2) * dn < F32(3.0):
        dn = np.nextafter(dn, F32(-np.inf))
    add("dist just above 1.2f*max_dist is dropped", MAX_DIST, (0.0, 0.0, 3.0), mind=0.1, maxd=dn)
    add("dot == 0.5*dist is kept", KEPT, (0.0, 0.0, 2.0), (0, 0, 0.5))
    add("dot just below 0.5*dist is dropped", VIEW, (0.0, 0.0, 2.0), (0, 0, np.nextafter(F32(0.5), F32(0))))
    add("dist == 0 in view 1 (the point is its camera centre: z == 0)", KEPT, (-0.5, 0.0, 0.0), (-0.5, 0, 0), mind=0.0, maxd=1.0)
    names[-1] = (names[-1][0], DEPTH)                                           # z == 0 in view 0 as well
    add("max_dist == 0 with min_dist == 0: ratio 0, level 0", MAX_DIST, (0.0, 0.0, 1.0), mind=0.0, maxd=0.0)
    add("an infinite ratio cannot pass the depth gate; a huge one gives the last level", KEPT, (0.0, 0.0, 1e-3), mind=0.0, maxd=1e30)
    return v, np.array(rows, P.MAPPOINT_DTYPE), names


def points_onto(kps, desc, view, cam, mode, rng, noise_px=1.0, flips=12):
    """(MAPPOINT_DTYPE[n], descriptors): map point i projects through `view` in `mode` within about noise_px of keypoint i, is seen
    head-on, lies inside its invariance region and predicts the keypoint's octave; its descriptor is the keypoint's with a few bits
    flipped.  What a map that really contains the keyframe's points looks like to the searches."""
    import psl_slam_amd as P
    n = len(kps)
    R1, t1 = view["Tcw"]["R"].reshape(3, 3).astype(F64), view["Tcw"]["t"].astype(F64)
    R2, t2 = view["T21"]["R"].reshape(3, 3).astype(F64), view["T21"]["t"].astype(F64)
    z = rng.uniform(0.8, 5.0, n)
    px = kps["x"].astype(F64) + rng.normal(0, noise_px, n)
    py = kps["y"].astype(F64) + rng.normal(0, noise_px, n)
    pc = np.stack([(px - cam["cx"]) / cam["fx"] * z, (py - cam["cy"]) / cam["fy"] * z, z], 1)
    if mode == SIM3:
        dist = np.linalg.norm(pc, axis=1)                                        # |p3Dc2|
        pc = (pc - t2) @ np.linalg.inv(R2).T
    pw = (pc - t1) @ np.linalg.inv(R1).T
    po = pw - (-R1.T @ t1)
    if mode != SIM3:
        dist = np.linalg.norm(po, axis=1)
    mp = np.zeros(n, P.MAPPOINT_DTYPE)
    mp["x"], mp["y"], mp["z"] = pw.T
    mp["nx"], mp["ny"], mp["nz"] = (po / np.linalg.norm(po, axis=1)[:, None]).T
    mp["max_dist"] = dist * 1.2 ** (kps["octave"] - 0.5)
    mp["min_dist"] = mp["max_dist"] / 1.2 ** (NLEVELS - 1)
    return mp, ks.noisy_desc(desc, rng, flips=flips)
