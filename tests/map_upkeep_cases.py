"""Expected rows and inputs for the map refresh on the device (tests/test_map_upkeep_{cpu,gpu}.py).

The restatements are written from the reference lines with the conventions of include/pslfe.h above pslfe_kf_update_normal_and_depth:
  restate_points*  MapPoint::UpdateNormalAndDepth      src/MapPoint.cc:330-371
  restate_lines*   MapLine::UpdateAverageDir           add_src/MapLine.cpp:320-367
  restate_median   KeyFrame::ComputeSceneMedianDepth   src/KeyFrame.cc:749-779
The rounding of the first two lives in OpenCV's MatExpr (Mat / double scales by the reciprocal in the Mat's float) and in Eigen's
fixed-size expressions; neither library is in the reference tree, so nothing here can be compiled against them and parity is
"HIP == this restatement", unpinned, as for every other stage whose rounding lives in OpenCV.

The *_scalar forms are the definition: float32 / float64 numpy scalars (each operation one correctly rounded IEEE operation) and
explicit loops in run order.  restate_points / restate_lines are the same operations taken a run position at a time over all rows (every
row still adds its terms in run order); tests/test_map_upkeep_cpu.py shows the two forms equal byte for byte, and the GPU tests use the
second, which does the 160 000 observations of the launch-indexing case in a fraction of a second."""
from decimal import Decimal, getcontext

import numpy as np

F32, F64 = np.float32, np.float64
NLEVELS = 8
SCALE = (F32(1.2) ** np.arange(NLEVELS)).astype(F32)        # mvScaleFactors
NKF = 40
RUN_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 200)
POINT_SIZES = (1, 63, 64, 65, 257)
CANARY = 0x0A5E00


def _live(off, skip, i):
    return off[i + 1] > off[i] and not (skip is not None and skip[i])


def _ordered_sum(terms, order, zero):
    """the three sums of the order test: run order and reversed are sequential from zero, pairwise is a tree over the terms"""
    if order == "pairwise":
        def tree(t):
            return t[0] if len(t) == 1 else tree(t[:len(t) // 2]) + tree(t[len(t) // 2:])
        return [tree([t[c] for t in terms]) for c in range(3)]
    acc = [zero, zero, zero]
    for t in (terms if order == "run" else terms[::-1]):
        acc = [acc[c] + t[c] for c in range(3)]
    return acc


def _range(dist, scale, level):
    max_dist = dist * scale[level]                               # mfMaxDistance = dist*levelScaleFactor
    return max_dist / scale[len(scale) - 1], max_dist            # mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1]


def _norm_d(n):
    """cv::norm of a float triple as a double: the double sum of the exact squares in index order, sqrt in double"""
    d = [F64(v) for v in n]
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def point_dist(mp, centres, ref_kf, i):
    """const float dist = cv::norm(Pos - pRefKF->GetCameraCenter()) of row i"""
    ow = centres[ref_kf[i]]
    return F32(_norm_d([F32(mp[f][i]) - F32(ow[c]) for c, f in enumerate(("x", "y", "z"))]))


def restate_points_scalar(mp, off, okf, centres, ref_kf, ref_level, scale, skip=None, order="run"):
    out = mp.copy()
    scale = np.asarray(scale, F32)
    with np.errstate(all="ignore"):
        for i in range(len(mp)):
            if not _live(off, skip, i):                          # mbBad, observations.empty(): :338-346
                continue
            P = [F32(mp[f][i]) for f in ("x", "y", "z")]
            terms = []
            for o in range(off[i], off[i + 1]):
                ow = centres[okf[o]]
                n = [P[c] - F32(ow[c]) for c in range(3)]        # normali = mWorldPos - Owi
                t = F32(F64(1.0) / _norm_d(n))                   # Mat / double: the reciprocal, in the Mat's float
                terms.append([n[c] * t for c in range(3)])
            normal = _ordered_sum(terms, order, F32(0.0))        # normal = normal + ...
            t = F32(F64(1.0) / F64(off[i + 1] - off[i]))         # normal/n
            dist = point_dist(mp, centres, ref_kf, i)
            out["nx"][i], out["ny"][i], out["nz"][i] = (normal[c] * t for c in range(3))
            out["min_dist"][i], out["max_dist"][i] = _range(dist, scale, ref_level[i])
    return out


def _half_sum(a, b):
    """0.5*(SP+EP) on float Mats: the float sum of the exact halves (include/pslfe.h above PslMapLineGeom)"""
    return F32(0.5) * a + F32(0.5) * b


def line_dist(ml, centres, ref_kf, i):
    """SP, EP as Mat_<float>, MP = 0.5*(SP+EP), CM = MP - Ow, const float dist = cv::norm(CM) of row i"""
    ow = centres[ref_kf[i]]
    return F32(_norm_d([_half_sum(F32(ml["sp"][i][c]), F32(ml["ep"][i][c])) - F32(ow[c]) for c in range(3)]))


def restate_lines_scalar(ml, off, okf, centres, ref_kf, ref_level, scale, skip=None, order="run"):
    out = ml.copy()
    scale = np.asarray(scale, F32)
    with np.errstate(all="ignore"):
        for i in range(len(ml)):
            if not _live(off, skip, i):
                continue
            sp, ep = [F64(v) for v in ml["sp"][i]], [F64(v) for v in ml["ep"][i]]
            mid = [F64(0.5) * (sp[c] + ep[c]) for c in range(3)]         # 0.5*(mWorldPos.head(3)+mWorldPos.tail(3))
            terms = []
            for o in range(off[i], off[i + 1]):
                ow = centres[okf[o]]
                n = [mid[c] - F64(F32(ow[c])) for c in range(3)]         # middlePos - OWi
                nrm = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                terms.append([n[c] / nrm for c in range(3)])             # normali/normali.norm()
            normal = _ordered_sum(terms, order, F64(0.0))
            dn = F64(off[i + 1] - off[i])
            dist = line_dist(ml, centres, ref_kf, i)
            out["normal"][i] = [normal[c] / dn for c in range(3)]
            out["min_dist"][i], out["max_dist"][i] = _range(dist, scale, ref_level[i])
    return out


def _by_step(off, skip, M):
    """(live rows, their run lengths): the rows that are refreshed"""
    lens = np.diff(off)
    live = lens > 0
    if skip is not None:
        live &= np.asarray(skip) == 0
    idx = np.nonzero(live)[0]
    return idx, lens[idx]


def _norm_rows(n):
    d = n.astype(F64)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def restate_points(mp, off, okf, centres, ref_kf, ref_level, scale, skip=None):
    out = mp.copy()
    scale, centres = np.asarray(scale, F32), np.asarray(centres, F32)
    idx, lens = _by_step(off, skip, len(mp))
    if not len(idx):
        return out
    P = np.stack([mp["x"][idx], mp["y"][idx], mp["z"][idx]], 1).astype(F32)
    acc = np.zeros((len(idx), 3), F32)
    with np.errstate(all="ignore"):
        for s in range(int(lens.max())):
            act = lens > s
            n = P[act] - centres[okf[off[idx[act]] + s]]
            t = (F64(1.0) / _norm_rows(n)).astype(F32)
            acc[act] = acc[act] + n * t[:, None]
        t = (F64(1.0) / lens.astype(F64)).astype(F32)
        dist = _norm_rows(P - centres[ref_kf[idx]]).astype(F32)
        max_dist = dist * scale[ref_level[idx]]
        out["nx"][idx], out["ny"][idx], out["nz"][idx] = (acc * t[:, None]).T
        out["max_dist"][idx], out["min_dist"][idx] = max_dist, max_dist / scale[len(scale) - 1]
    return out


def restate_lines(ml, off, okf, centres, ref_kf, ref_level, scale, skip=None):
    out = ml.copy()
    scale, centres = np.asarray(scale, F32), np.asarray(centres, F32)
    idx, lens = _by_step(off, skip, len(ml))
    if not len(idx):
        return out
    sp, ep = ml["sp"][idx].astype(F64), ml["ep"][idx].astype(F64)
    mid = F64(0.5) * (sp + ep)
    acc = np.zeros((len(idx), 3), F64)
    with np.errstate(all="ignore"):
        for s in range(int(lens.max())):
            act = lens > s
            n = mid[act] - centres[okf[off[idx[act]] + s]].astype(F64)
            nrm = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
            acc[act] = acc[act] + n / nrm[:, None]
        cm = _half_sum(sp.astype(F32), ep.astype(F32)) - centres[ref_kf[idx]]
        dist = _norm_rows(cm).astype(F32)
        max_dist = dist * scale[ref_level[idx]]
        out["normal"][idx] = acc / lens.astype(F64)[:, None]
        out["max_dist"][idx], out["min_dist"][idx] = max_dist, max_dist / scale[len(scale) - 1]
    return out


# ---- the same formulas without rounding (50 significant digits) ----------------------------------------------------------------------

def _D(v):
    return Decimal(float(v))


def exact_point(mp, off, okf, centres, ref_kf, ref_level, scale, i):
    """(normal [3], dist) of row i as Decimals: every operation exact to 50 digits"""
    getcontext().prec = 50
    P = [_D(mp[f][i]) for f in ("x", "y", "z")]
    acc = [Decimal(0)] * 3
    for o in range(off[i], off[i + 1]):
        n = [P[c] - _D(centres[okf[o]][c]) for c in range(3)]
        nrm = (n[0] * n[0] + n[1] * n[1] + n[2] * n[2]).sqrt()
        acc = [acc[c] + n[c] / nrm for c in range(3)]
    cnt = Decimal(int(off[i + 1] - off[i]))
    pc = [P[c] - _D(centres[ref_kf[i]][c]) for c in range(3)]
    dist = (pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]).sqrt()
    return [a / cnt for a in acc], dist


def exact_line(ml, off, okf, centres, ref_kf, ref_level, scale, i):
    """the same for a line.  dist starts from the float Mat MP = 0.5*(SP+EP) as the reference holds it: that rounding comes before a
    subtraction that can cancel (|MP - Ow| far below |MP|), so no bound in ulps of dist holds for it; everything after it is exact"""
    getcontext().prec = 50
    sp, ep = [_D(v) for v in ml["sp"][i]], [_D(v) for v in ml["ep"][i]]
    mid = [(sp[c] + ep[c]) / 2 for c in range(3)]
    acc = [Decimal(0)] * 3
    for o in range(off[i], off[i + 1]):
        n = [mid[c] - _D(centres[okf[o]][c]) for c in range(3)]
        nrm = (n[0] * n[0] + n[1] * n[1] + n[2] * n[2]).sqrt()
        acc = [acc[c] + n[c] / nrm for c in range(3)]
    cnt = Decimal(int(off[i + 1] - off[i]))
    cm = [_D(_half_sum(F32(ml["sp"][i][c]), F32(ml["ep"][i][c]))) - _D(centres[ref_kf[i]][c]) for c in range(3)]
    dist = (cm[0] * cm[0] + cm[1] * cm[1] + cm[2] * cm[2]).sqrt()
    return [a / cnt for a in acc], dist


def exact_line_dist_unrounded(ml, centres, ref_kf, i):
    """(dist of row i from the unrounded half-sum of the float end points, the bound of what the half-sum's rounding can move it by: half
    an ulp of every component of MP, taken through the norm, sqrt(sum (ulp(MP_c)/2)^2))"""
    getcontext().prec = 50
    sp, ep = [F32(v) for v in ml["sp"][i]], [F32(v) for v in ml["ep"][i]]
    cm = [(_D(sp[c]) + _D(ep[c])) / 2 - _D(centres[ref_kf[i]][c]) for c in range(3)]
    slack = sum((_D(np.spacing(_half_sum(sp[c], ep[c]))) / 2) ** 2 for c in range(3)).sqrt()
    return (cm[0] * cm[0] + cm[1] * cm[1] + cm[2] * cm[2]).sqrt(), slack


# ---- median depth ---------------------------------------------------------------------------------------------------------------------

def depths(pose, x):
    """float z = Rcw2.dot(x3Dw)+zcw: the double sum in index order of the exact products, + the double of tcw[2], one rounding"""
    r = np.asarray(pose["R"], F32).astype(F64)[6:9]
    x = np.asarray(x, F32).reshape(-1, 3).astype(F64)
    return (((r[0] * x[:, 0] + r[1] * x[:, 1]) + r[2] * x[:, 2]) + F64(F32(pose["t"][2]))).astype(F32)


def restate_median(poses, xs, q):
    """vDepths[(vDepths.size()-1)/q] of the sorted depths, by rank: the value with at most `rank` depths below it and more than `rank`
    depths not above it; -1 for a keyframe without map points (the library's definition; the reference indexes an empty vector)"""
    out = np.zeros(len(poses), F32)
    for k, (pose, x) in enumerate(zip(poses, xs)):
        z = depths(pose, x)
        if len(z) == 0:
            out[k] = -1.0
            continue
        rank = (len(z) - 1) // q
        for v in z:
            if (z < v).sum() <= rank < (z <= v).sum():
                out[k] = v
                break
    return out


# ---- seeded cases ---------------------------------------------------------------------------------------------------------------------

def _runs(M, rng, lengths):
    """run lengths for M rows: every length of `lengths` once when M allows, the rest drawn from it, shuffled"""
    lens = rng.choice(lengths, M)
    if M >= len(lengths):
        lens[:len(lengths)] = lengths
    rng.shuffle(lens)
    return lens.astype(np.int64)


def _observations(lens, nkf, rng, third_skip=True):
    """CSR runs over nkf keyframes, mpRefKF = a keyframe of the run (-1 where there is none), the octave of its observation, skip bytes"""
    M = len(lens)
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum(lens)
    okf = rng.integers(0, nkf, int(off[-1])).astype(np.int32)
    ref_kf = np.full(M, -1, np.int32)
    for i in np.nonzero(lens > 0)[0]:
        ref_kf[i] = okf[off[i] + rng.integers(0, lens[i])]
    ref_level = rng.integers(0, NLEVELS, M).astype(np.int32)
    skip = (np.arange(M) % 3 == 1).astype(np.uint8) if third_skip else np.zeros(M, np.uint8)
    rng.shuffle(skip)
    ref_level[(skip != 0) & (np.arange(M) % 2 == 0)] = -7         # a bad point's reference is never read
    return off, okf, ref_kf, ref_level, skip


def centres(nkf, rng):
    return rng.uniform(-3.0, 3.0, (nkf, 3)).astype(F32)


def _canary(a, fields):
    """the fields a refresh writes, filled with a pattern that no refresh produces (a different NaN payload per word)"""
    for f in fields:
        single = a[f].dtype == F32
        w = a[f].view(np.uint32 if single else np.uint64)
        count = np.arange(w.size, dtype=np.uint64).reshape(w.shape) % 251
        w[...] = (count + (0x7FC00000 if single else 0x7FF8 << 48) + CANARY).astype(w.dtype)
    return a


POINT_OUT = ("nx", "ny", "nz", "min_dist", "max_dist")
LINE_OUT = ("normal", "min_dist", "max_dist")


def point_case(M, seed=3, nkf=NKF, lengths=RUN_LENGTHS, lens=None):
    """(mp with canaries, off, okf, centres, ref_kf, ref_level, skip)"""
    import psl_slam_amd as P
    rng = np.random.default_rng(seed + 1000 * M)
    lens = _runs(M, rng, lengths) if lens is None else lens
    off, okf, ref_kf, ref_level, skip = _observations(lens, nkf, rng)
    mp = np.zeros(M, P.MAPPOINT_DTYPE)
    mp["x"], mp["y"], mp["z"] = rng.uniform(-8.0, 8.0, (3, M)).astype(F32)
    return _canary(mp, POINT_OUT), off, okf, centres(nkf, rng), ref_kf, ref_level, skip


def line_case(M, seed=5, nkf=NKF, lengths=RUN_LENGTHS, lens=None):
    """the same over MAPLINE_DTYPE; the first row that is refreshed has sp == ep"""
    import psl_slam_amd as P
    rng = np.random.default_rng(seed + 1000 * M)
    lens = _runs(M, rng, lengths) if lens is None else lens
    off, okf, ref_kf, ref_level, skip = _observations(lens, nkf, rng)
    ml = np.zeros(M, P.MAPLINE_DTYPE)
    ml["sp"] = rng.uniform(-8.0, 8.0, (M, 3))
    ml["ep"] = ml["sp"] + rng.normal(0.0, 0.5, (M, 3))
    live = np.nonzero((np.diff(off) > 0) & (skip == 0))[0]
    if len(live):
        ml["ep"][live[0]] = ml["sp"][live[0]]
    return _canary(ml, LINE_OUT), off, okf, centres(nkf, rng), ref_kf, ref_level, skip


def whole_map_lengths(M, rng, mean=8):
    """run lengths of a map: geometric with the given mean, at least 2 (a map point has two observations when it is created)"""
    return np.maximum(2, rng.geometric(1.0 / mean, M)).astype(np.int64)


def big_point_case(M=20000, seed=11):
    """the launch-indexing case: 20 000 points, about 160 000 observations"""
    rng = np.random.default_rng(seed)
    return point_case(M, seed, nkf=500, lens=whole_map_lengths(M, rng))


def big_line_case(M=20000, seed=13):
    rng = np.random.default_rng(seed)
    return line_case(M, seed, nkf=500, lens=whole_map_lengths(M, rng))


def median_case(K, n, seed=17):
    """(poses POSE_DTYPE[K], positions [K] of n x 3): depths in front of and behind the camera, none exactly zero, a fifth of them
    copies of another point's (equal depths)"""
    import psl_slam_amd as P
    rng = np.random.default_rng(seed + 100 * n + K)
    poses = np.zeros(K, P.POSE_DTYPE)
    xs = []
    for k in range(K):
        a = rng.normal(0, 0.3, 3)
        Rx = np.array([[1, 0, 0], [0, np.cos(a[0]), -np.sin(a[0])], [0, np.sin(a[0]), np.cos(a[0])]])
        Ry = np.array([[np.cos(a[1]), 0, np.sin(a[1])], [0, 1, 0], [-np.sin(a[1]), 0, np.cos(a[1])]])
        poses[k]["R"], poses[k]["t"] = (Rx @ Ry).astype(F32).reshape(9), rng.normal(0, 0.5, 3).astype(F32)
        x = rng.uniform(-4.0, 6.0, (n, 3)).astype(F32)
        if n >= 2:
            dup = rng.random(n) < 0.2
            x[dup] = x[rng.integers(0, n, int(dup.sum()))]
        assert (depths(poses[k], x) != 0).all()
        xs.append(x)
    return poses, xs
