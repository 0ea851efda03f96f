"""Expected rows and inputs for the device projection of map lines into keyframes (tests/test_kf_line_project_{cpu,gpu}.py).

restate_line_project is a numpy restatement of the loop of LSDmatcher::Fuse(pKF, vpMapLines, th) in front of GetLinesInArea,
add_src/LSDmatcher.cpp:865-931, written from the reference lines (the file needs OpenCV, so it cannot be compiled as an oracle: these
rows are "HIP = restatement") with the conventions of include/pslfe.h: a 3x3 * 3x1 + 3x1 product is the double sum in index order
rounded once to float, cv::norm and Mat::dot are double sums, the view gate compares in double, OM = 0.5*(SP+EP) - Ow is a float sum, an
exact halving and a float difference, every other operation is one float operation in the reference's order.  float32 numpy operations
are single correctly rounded operations.  The level is the C++ oracle's MapLine::PredictScale (oracle_lib.lr_level, the library's logf).

`return false` at :890-891 leaves the whole function: stop[k] is the first line, among those not skipped, with an end point behind the
camera, and every row from there on is dropped.

The file also holds the scene (poses of kf_project_cases.views(), map lines unprojected from the end points of synthetic keylines at
random depths, 8 levels of scale 1.2 so that the level band matters), constructed rows for the limit cases and map lines that really
project onto the keylines of a keyframe."""
import numpy as np

import kf_project_cases as kc
from kf_project_cases import F32, F64, affine, centre, dot3, norm3

KEPT, SKIP, STOP, IMAGE1, IMAGE2, MIN_DIST, MAX_DIST, VIEW, LEVEL = range(9)   # why a (keyframe, line) pair gives no row
REASONS = ("kept", "skip", "stop", "image-1", "image-2", "min-dist", "max-dist", "view", "level-out-of-range")
NLEVELS = 8
SCALE_LINE = (F32(1.2) ** np.arange(NLEVELS)).astype(F32)           # mvScaleFactorsLine
LOG_SCALE = kc.LOG_SCALE                                            # mfLogScaleFactorLine = log(1.2f)
INT32_MIN = -2**31
BOUNDS = (0.0, 0.0, 640.0, 480.0)


def _poses(views):
    views = np.asarray(views).reshape(-1)
    return views["Tcw"] if views.dtype.names and "Tcw" in views.dtype.names else views


def restate_line_project(views, ml, cam, bounds, scale_line, th, skip=None, log_scale=LOG_SCALE):
    """-> (rows LINEFUSEQUERY_DTYPE [K, M], level [K, M], stop [K], reason [K, M]) as pslfe_kf_line_project gives the first three"""
    import oracle_lib
    import psl_slam_amd as P
    poses = _poses(views)
    K, M = len(poses), len(ml)
    rows = np.zeros((K, M), P.LINEFUSEQUERY_DTYPE)
    rows["radius"] = -1.0
    level = np.full((K, M), INT32_MIN, np.int32)
    stop = np.full(K, M, np.int32)
    reason = np.zeros((K, M), np.int32)
    minX, minY, maxX, maxY = (F32(b) for b in bounds)
    fx, fy, cx, cy = (F32(cam[f]) for f in ("fx", "fy", "cx", "cy"))
    scale_line = np.asarray(scale_line, F32)
    SP, EP, PN = (np.asarray(ml[f], F64).astype(F32) for f in ("sp", "ep", "normal"))   # Mat_<float> initialisers :877-878, :919
    for k in range(K):
        R, t = poses[k]["R"], poses[k]["t"]
        r = np.zeros(M, np.int32)
        alive = np.ones(M, bool)

        def drop(cond, why):
            hit = alive & cond
            r[hit] = why
            alive[hit] = False

        with np.errstate(all="ignore"):
            if skip is not None:
                drop(np.asarray(skip).reshape(K, M)[k] != 0, SKIP)                 # :869-873
            SPc, EPc = affine(R, t, SP), affine(R, t, EP)                         # :880, :885
            behind = alive & ((SPc[:, 2] < F32(0.0)) | (EPc[:, 2] < F32(0.0)))    # :890 -> return false
            if behind.any():
                stop[k] = np.nonzero(behind)[0][0]
            invz1 = F32(1.0) / SPc[:, 2]                                          # :893-895
            u1, v1 = (fx * SPc[:, 0]) * invz1 + cx, (fy * SPc[:, 1]) * invz1 + cy
            drop(~((u1 >= minX) & (u1 < maxX) & (v1 >= minY) & (v1 < maxY)), IMAGE1)   # KeyFrame::IsInImage src/KeyFrame.cc:726-729
            invz2 = F32(1.0) / EPc[:, 2]                                          # :900-902
            u2, v2 = (fx * EPc[:, 0]) * invz2 + cx, (fy * EPc[:, 1]) * invz2 + cy
            drop(~((u2 >= minX) & (u2 < maxX) & (v2 >= minY) & (v2 < maxY)), IMAGE2)
            OM = F32(0.5) * (SP + EP) - centre(poses[k])                          # :911
            dist = norm3(OM)                                                      # :912
            drop(dist < F32(0.8) * ml["min_dist"], MIN_DIST)                      # :914 with Get{Min,Max}DistanceInvariance
            drop(dist > F32(1.2) * ml["max_dist"], MAX_DIST)
            drop(dot3(OM, PN) < 0.5 * dist.astype(F64), VIEW)                     # :921
            ratio = ml["max_dist"] / dist                                         # MapLine::PredictScale add_src/MapLine.cpp:381-390
        idx = np.nonzero(alive)[0]
        lvl = np.array([oracle_lib.lr_level(ratio[i], log_scale, 0) for i in idx], np.int64).reshape(-1)
        level[k, idx] = lvl
        drop(np.isin(np.arange(M), idx[(lvl < 0) | (lvl >= len(scale_line))]), LEVEL)   # mvScaleFactorsLine[level] out of range
        idx = np.nonzero(alive)[0]
        lvl = level[k, idx]
        for f, val in (("x1", u1), ("y1", v1), ("x2", u2), ("y2", v2)):
            rows[f][k, idx] = val[idx]
        rows["radius"][k, idx] = F32(th) * scale_line[lvl]                         # :927
        rows["level"][k, idx] = lvl
        gone = np.arange(M) >= stop[k]                                            # never reached
        rows[k][gone] = np.zeros((), rows.dtype)
        rows["radius"][k][gone] = -1.0
        level[k][gone] = INT32_MIN
        r[gone] = STOP
        reason[k] = r
    return rows, level, stop, reason


# ---- the scene -----------------------------------------------------------------------------------------------------------------

def keylines(n, rng, octaves=2):
    """n synthetic keylines of a 640 x 480 image: a few dominant directions, lengths 20..120 px, pt = the middle"""
    import psl_slam_amd as P
    kl = np.zeros(n, P.KEYLINE_DTYPE)
    sx, sy = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
    ang = rng.choice([0.0, 0.01, np.pi / 2, 0.7, -0.7], n) + rng.normal(0, 0.01, n)
    ln = rng.uniform(20, 120, n)
    kl["startPointX"], kl["startPointY"] = sx, sy
    kl["endPointX"], kl["endPointY"] = sx + ln * np.cos(ang), sy + ln * np.sin(ang)
    kl["pt_x"] = (kl["startPointX"] + kl["endPointX"]) / 2
    kl["pt_y"] = (kl["startPointY"] + kl["endPointY"]) / 2
    kl["octave"] = rng.integers(0, octaves, n)
    kl["lineLength"] = ln
    return kl


def _unproject(px, py, z, pose, cam):
    R, t = np.asarray(pose["R"], F64).reshape(3, 3), np.asarray(pose["t"], F64)
    pc = np.stack([(px - cam["cx"]) / cam["fx"] * z, (py - cam["cy"]) / cam["fy"] * z, z], -1)
    return (pc - t) @ R          # R.T @ (pc - t) per row


def _line_record(sp, ep, pose, lvl, rng, nrm=None):
    """a PslMapLineGeom tuple seen head-on from `pose` whose PredictScale from there is lvl"""
    R, t = np.asarray(pose["R"], F64).reshape(3, 3), np.asarray(pose["t"], F64)
    om = 0.5 * (sp + ep) - (-R.T @ t)
    dist = np.linalg.norm(om)
    if nrm is None:
        nrm = om / dist
    maxd = dist * 1.2 ** (lvl - rng.uniform(0.1, 0.9))
    return sp, ep, nrm, maxd / 1.2 ** (NLEVELS - 1), maxd, dist


def map_lines(M, poses, seed=21, nbehind=2):
    """(MAPLINE_DTYPE[M], descriptors [M, 32]): line i joins the end points of a synthetic keyline unprojected through pose i % K at
    two random depths; its normal is the viewing direction from there (turned away for some), its distance range puts the predicted
    level anywhere in 0..7, outside the scale table or outside the invariance region for some.  The last lines of the list lie behind
    every camera: the reference returns there."""
    import psl_slam_amd as P
    rng = np.random.default_rng(seed)
    poses = _poses(poses)
    cam = kc.camera()
    kl = keylines(M, rng)
    ml = np.zeros(M, P.MAPLINE_DTYPE)
    for i in range(M):
        pose = poses[i % len(poses)]
        z1 = rng.uniform(0.8, 6.0)
        z2 = z1 * rng.uniform(0.8, 1.25)
        if i >= M - nbehind:
            z2 = -z2
        sp = _unproject(kl["startPointX"][i], kl["startPointY"][i], z1, pose, cam)
        ep = _unproject(kl["endPointX"][i], kl["endPointY"][i], z2, pose, cam)
        nrm = None
        if rng.random() < 0.10:                                                  # seen from elsewhere: the 60 degree gate
            nrm = rng.normal(0, 1, 3)
            nrm /= np.linalg.norm(nrm)
        w = rng.random()
        lvl = NLEVELS if w < 0.06 else rng.integers(0, NLEVELS)                  # level 8: past the end of mvScaleFactorsLine
        sp, ep, nrm, mind, maxd, dist = _line_record(sp, ep, pose, lvl, rng, nrm)
        if 0.06 <= w < 0.11:
            mind = dist * rng.uniform(1.3, 2.0)                                  # closer than the invariance region allows
            maxd = mind * 1.2 ** (NLEVELS - 1)
        elif 0.11 <= w < 0.16:
            maxd = dist * rng.uniform(0.3, 0.8)                                  # farther
            mind = maxd / 1.2 ** (NLEVELS - 1)
        ml[i] = (sp, ep, nrm, mind, maxd)
    return ml, rng.integers(0, 256, (M, 32), dtype=np.uint8)


def skip_bytes(K, M, seed=9, p=0.05):
    return (np.random.default_rng(seed).random((K, M)) < p).astype(np.uint8)


def lines_onto(kls, desc, pose, cam, rng, flips=8):
    """(MAPLINE_DTYPE[n], descriptors): map line i projects through `pose` onto keyline i, is seen head-on, lies inside its invariance
    region and predicts the keyline's octave; its descriptor is row i of `desc` (cycled when desc is short) with a few bits flipped."""
    import kf_scene as ks
    import psl_slam_amd as P
    n = len(kls)
    ml = np.zeros(n, P.MAPLINE_DTYPE)
    for i in range(n):
        z1 = rng.uniform(1.0, 5.0)
        z2 = z1 * rng.uniform(0.9, 1.1)
        sp = _unproject(float(kls["startPointX"][i]), float(kls["startPointY"][i]), z1, pose, cam)
        ep = _unproject(float(kls["endPointX"][i]), float(kls["endPointY"][i]), z2, pose, cam)
        ml[i] = _line_record(sp, ep, pose, int(kls["octave"][i]), rng)[:5]
    d = desc[np.arange(n) % max(len(desc), 1)] if len(desc) else np.zeros((n, 32), np.uint8)
    return ml, ks.noisy_desc(d, rng, flips=flips)


# ---- limit cases ---------------------------------------------------------------------------------------------------------------

def limit_cases():
    """(POSE_DTYPE[3], MAPLINE_DTYPE[n], names): every pose is the identity with tcw = (0, 0, -0.0f) (Ow = 0, SPc = SP exactly; the
    negative zero lets a depth sum stay -0.0f: x + -0.0 is x for every other x, +0.0 included), the camera is
    kc.limit_camera() (u = 512*x/z + 320 is exact for the values used) with bounds 0..640 x 0..480.  names[i] = (what, expected reason,
    expected level or None).  The last line lies behind the camera: with it the reference returns at index n - 1."""
    import psl_slam_amd as P
    poses = np.zeros(3, P.POSE_DTYPE)
    for k in range(3):
        poses[k] = kc.pose_record(np.eye(3), [0.0, 0.0, -0.0])
    rows, names = [], []

    def add(what, expect, sp, ep, n=None, mind=0.1, maxd=None, lvl=None):
        om = 0.5 * (np.array(sp, F64) + np.array(ep, F64))
        if maxd is None:
            maxd = np.linalg.norm(om) * 1.2 ** 2.5                                 # level 3 unless the case says otherwise
        rows.append((sp, ep, om if n is None else n, mind, maxd))
        names.append((what, expect, lvl))

    far = (0.0, 0.0, 2.5)
    add("u1 == min_x is kept", KEPT, (-0.625, 0.0, 1.0), (0.0, 0.0, 1.0))
    add("u1 == max_x is dropped", IMAGE1, (0.625, 0.0, 1.0), (0.0, 0.0, 1.0))
    add("u2 == min_x is kept", KEPT, (0.0, 0.0, 1.0), (-0.625, 0.0, 1.0))
    add("u2 == max_x is dropped", IMAGE2, (0.0, 0.0, 1.0), (0.625, 0.0, 1.0))
    add("v1 == max_y is dropped", IMAGE1, (0.0, 0.46875, 1.0), (0.0, 0.0, 1.0))
    add("z1 == 0 is no stop: 1/0 = inf fails IsInImage", IMAGE1, (0.1, 0.1, 0.0), far)
    # 0*(-0.1) + 0*(-0.1) + 1*(-0.0) + (-0.0): every term and the sum are -0.0; invz = -inf, u = (512*(-0.1))*(-inf) + 320 = +inf
    add("z1 == -0.0f is not < 0: no stop, 1/-0 = -inf, u = +inf fails IsInImage", IMAGE1, (-0.1, -0.1, -0.0), far)
    add("z1 NaN is no stop", IMAGE1, (0.0, 0.0, np.nan), far)
    add("z2 == 0 is no stop", IMAGE2, (0.0, 0.0, 1.5), (0.1, 0.1, 0.0))
    add("z2 == -0.0f is not < 0: no stop", IMAGE2, (0.0, 0.0, 1.5), (-0.1, -0.1, -0.0))
    add("z2 NaN is no stop", IMAGE2, (0.0, 0.0, 1.5), (0.0, 0.0, np.nan))
    mind = kc._solve(lambda m: F32(0.8) * m, 2.0, 2.5)
    add("dist == 0.8f*min_dist is kept", KEPT, (0.0, 0.0, 1.5), far, mind=mind, maxd=mind * F32(2.0))
    up = np.nextafter(mind, F32(np.inf))
    while not F32(0.8) * up > F32(2.0):
        up = np.nextafter(up, F32(np.inf))
    add("dist just below 0.8f*min_dist is dropped", MIN_DIST, (0.0, 0.0, 1.5), far, mind=up, maxd=up * F32(2.0))
    far3 = ((0.0, 0.0, 2.5), (0.0, 0.0, 3.5))                                    # dist == 3
    maxd = kc._solve(lambda m: F32(1.2) * m, 3.0, 2.5)
    add("dist == 1.2f*max_dist passes the distance gate", None, *far3, maxd=maxd)   # its level: worked out in the CPU test
    dn = np.nextafter(maxd, F32(-np.inf))
    while not F32(1.2) * dn < F32(3.0):
        dn = np.nextafter(dn, F32(-np.inf))
    add("dist just above 1.2f*max_dist is dropped", MAX_DIST, *far3, maxd=dn)
    add("dot == 0.5*dist is kept", KEPT, (0.0, 0.0, 1.5), far, n=(0, 0, 0.5))
    add("dot just below 0.5*dist is dropped", VIEW, (0.0, 0.0, 1.5), far, n=(0, 0, np.nextafter(F32(0.5), F32(0))))
    add("ratio == 1: logf(1) = 0, level 0", KEPT, (0.0, 0.0, 1.5), far, maxd=2.0, lvl=0)
    r12 = F32(1.0) / F32(1.2)
    add("ratio == 1/1.2f", None, (0.0, 0.0, 1.5), far, maxd=F32(2.0) * r12)      # expectation worked out in the CPU test
    add("level 7 is the last of the table", KEPT, (0.0, 0.0, 1.5), far, maxd=2.0 * 1.2 ** 6.5, lvl=7)
    add("level 8 is past the table", LEVEL, (0.0, 0.0, 1.5), far, maxd=2.0 * 1.2 ** 7.5, lvl=8)
    add("behind the camera: the reference returns here", STOP, (0.0, 0.0, 1.5), (0.0, 0.0, -1.0))
    ml = np.zeros(len(rows), P.MAPLINE_DTYPE)
    for i, rrow in enumerate(rows):
        ml[i] = rrow
    return poses, ml, names
