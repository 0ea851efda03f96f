"""Expected answers and inputs for the two ORBmatcher searches of LoopClosing::ComputeSim3 (tests/test_loop_match_{cpu,gpu}.py).

restate_search_by_bow / restate_search_by_projection_sim3 are restatements of the reference's loops in plain Python, statement by
statement with the line numbers of src/ORBmatcher.cc (ORBmatcher.cc needs OpenCV, so it cannot be compiled as an oracle: these rows
are "HIP = restatement").  tests/test_loop_match_cpu.py pins them against the C++ oracle where the oracle has a function with the
same rule.  Besides the results they return what the tests need to show that a case is not vacuous."""
import math

import numpy as np

import kf_scene as ks

TH_LOW, HISTO_LENGTH = 50, 30      # src/ORBmatcher.cc:38-39
GRID_COLS, GRID_ROWS = 64, 48      # include/Frame.h:45-46
F32 = np.float32


def _ints(desc):
    return [int.from_bytes(bytes(r), "little") for r in np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)]


def _distance(a, b):
    """ORBmatcher::DescriptorDistance :1647-1665: the number of differing bits"""
    return bin(a ^ b).count("1")


def _round(x):
    """C round() of a non-negative float: halves away from zero"""
    return int(math.floor(float(x) + 0.5))


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima :1601-1642 on the bin sizes"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i in range(len(sizes)):
        s = sizes[i]
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def restate_search_by_bow(angle2, desc2, fidx2, runs, qangle, qdesc, nnratio, check_ori):
    """ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12) :522-655 on the flattened inputs of pslfe_kf_search_by_bow: query i is the
    i-th KF1 feature with a good map point in the order of :550-554, runs[i] the run of fidx2 that is its node's list in KF2 with
    the features of :576-580 (no map point, bad) already left out.
    -> dict: nmatches, match [nq], pre = matches before the histogram, contested = queries whose best candidate was already in
    vbMatched2, removed = matches the histogram cleared, best1 = bestDist1 per query (256: no candidate)."""
    d2, qd = _ints(desc2), _ints(qdesc)
    nq = len(qd)
    vbMatched2 = [False] * len(d2)                       # :535
    match = [-1] * nq                                    # vpMatches12 :534
    rotHist = [[] for _ in range(HISTO_LENGTH)]          # :537
    factor = F32(1.0) / F32(HISTO_LENGTH)                # :541
    nmatches, contested, best1 = 0, 0, []
    for i in range(nq):                                  # :554 (the node walk :550-632 is in `runs`)
        start, ln = int(runs[i][0]), int(runs[i][1])
        bestDist1, bestIdx2, bestDist2 = 256, -1, 256    # :566-568
        freeDist, freeIdx = 256, -1                      # the same search without vbMatched2 (for `contested` only)
        for p in range(start, start + ln):               # :570
            idx2 = int(fidx2[p])
            dist = _distance(qd[i], d2[idx2])            # :584
            if dist < freeDist:
                freeDist, freeIdx = dist, idx2
            if vbMatched2[idx2]:                         # :576
                continue
            if dist < bestDist1:                         # :586-591
                bestDist2, bestDist1, bestIdx2 = bestDist1, dist, idx2
            elif dist < bestDist2:                       # :592-595
                bestDist2 = dist
        best1.append(bestDist1)
        contested += freeIdx >= 0 and vbMatched2[freeIdx]
        if bestDist1 < TH_LOW:                           # :598
            if F32(bestDist1) < F32(nnratio) * F32(bestDist2):   # :600
                match[i] = bestIdx2                      # :602
                vbMatched2[bestIdx2] = True              # :603
                if check_ori:                            # :605-615
                    rot = F32(qangle[i]) - F32(angle2[bestIdx2])
                    if rot < 0.0:
                        rot = rot + F32(360.0)
                    b = _round(rot * factor)
                    if b == HISTO_LENGTH:
                        b = 0
                    assert 0 <= b < HISTO_LENGTH
                    rotHist[b].append(i)
                nmatches += 1                            # :616
    pre = nmatches
    if check_ori:                                        # :634-652
        ind = three_maxima([len(h) for h in rotHist])
        for b in range(HISTO_LENGTH):
            if b in ind:
                continue
            for i in rotHist[b]:
                match[i] = -1
                nmatches -= 1
    return dict(nmatches=nmatches, match=np.array(match, np.int32).reshape(-1), pre=pre, contested=contested, removed=pre - nmatches,
                best1=np.array(best1, np.int32).reshape(-1))


class KeyFrameGrid:
    """mGrid of a KeyFrame (Frame::AssignFeaturesToGrid src/Frame.cc:269-284 with PosInGrid :1040-1050, copied by the KeyFrame
    constructor) and KeyFrame::GetFeaturesInArea src/KeyFrame.cc:685-724, in float as the reference computes them."""

    def __init__(self, kps, bounds):
        self.x = [F32(v) for v in kps["x"]]
        self.y = [F32(v) for v in kps["y"]]
        self.minX, self.minY = F32(bounds[0]), F32(bounds[1])
        self.invW = F32(GRID_COLS) / (F32(bounds[2]) - F32(bounds[0]))
        self.invH = F32(GRID_ROWS) / (F32(bounds[3]) - F32(bounds[1]))
        self.cell = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
        for i in range(len(kps)):
            px, py = (self.x[i] - self.minX) * self.invW, (self.y[i] - self.minY) * self.invH
            posX = int(math.floor(float(px) + 0.5)) if px >= 0 else -int(math.floor(-float(px) + 0.5))
            posY = int(math.floor(float(py) + 0.5)) if py >= 0 else -int(math.floor(-float(py) + 0.5))
            if posX < 0 or posX >= GRID_COLS or posY < 0 or posY >= GRID_ROWS:
                continue
            self.cell[posX][posY].append(i)

    def area(self, x, y, r):
        out = []
        nMinCellX = max(0, math.floor(float((x - self.minX - r) * self.invW)))          # :690
        if nMinCellX >= GRID_COLS:
            return out
        nMaxCellX = min(GRID_COLS - 1, math.ceil(float((x - self.minX + r) * self.invW)))   # :694
        if nMaxCellX < 0:
            return out
        nMinCellY = max(0, math.floor(float((y - self.minY - r) * self.invH)))          # :698
        if nMinCellY >= GRID_ROWS:
            return out
        nMaxCellY = min(GRID_ROWS - 1, math.ceil(float((y - self.minY + r) * self.invH)))   # :702
        if nMaxCellY < 0:
            return out
        for ix in range(nMinCellX, nMaxCellX + 1):       # :706-721
            for iy in range(nMinCellY, nMaxCellY + 1):
                for j in self.cell[ix][iy]:
                    if abs(self.x[j] - x) < r and abs(self.y[j] - y) < r:
                        out.append(j)
        return out


def restate_search_by_projection_sim3(kps, desc, bounds, queries, qdesc, taken=None):
    """ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) :290-403 from :362 on: query i is map point i after the
    gates of :316-357 (radius < 0: it did not pass), max_level = nPredictedLevel, radius = th*mvScaleFactors[nPredictedLevel] :360.
    -> dict: nmatches, match [nq], assigned [n] (-1 where vpMatched[c] is NULL or was set before the call), lost = queries whose
    best free-on-entry keypoint had been given to an earlier query, deep = queries that found 8 or more acceptable candidates (free on
    entry, right octave, distance <= TH_LOW) ahead of their choice, in (distance, visiting order), given away already."""
    G = KeyFrameGrid(kps, bounds)
    d, qd = _ints(desc), _ints(qdesc)
    n, nq = len(d), len(qd)
    octave = [int(o) for o in kps["octave"]]
    entry = [bool(taken[i]) if taken is not None else False for i in range(n)]
    vpMatched = list(entry)
    match, assigned = [-1] * nq, [-1] * n
    nmatches = lost = deep = 0
    for iMP in range(nq):                                # :312
        q = queries[iMP]
        if not (q["radius"] >= 0):                       # :316-357 on the host
            continue
        u, v, radius = F32(q["u"]), F32(q["v"]), F32(q["radius"])
        nPredictedLevel = int(q["max_level"])
        vIndices = G.area(u, v, radius)                  # :362
        if not vIndices:                                 # :364
            continue
        bestDist, bestIdx = 256, -1                      # :370-371
        freeDist, freeIdx = 256, -1                      # the same search against the entry marks only (for `lost`)
        ahead = []                                       # distances of the acceptable candidates already given away (for `deep`)
        for idx in vIndices:                             # :372
            kpLevel = octave[idx]
            if vpMatched[idx] and entry[idx]:
                continue
            if kpLevel < nPredictedLevel - 1 or kpLevel > nPredictedLevel:   # :380
                continue
            dist = _distance(qd[iMP], d[idx])            # :385
            if dist < freeDist:
                freeDist, freeIdx = dist, idx
            if vpMatched[idx]:                           # :375
                if dist <= TH_LOW:
                    ahead.append(dist)
                continue
            if dist < bestDist:                          # :387-391
                bestDist, bestIdx = dist, idx
        lost += freeDist <= TH_LOW and vpMatched[freeIdx]
        deep += sum(a <= bestDist for a in ahead) >= 8
        if bestDist <= TH_LOW:                           # :394
            vpMatched[bestIdx] = True                    # :396
            match[iMP], assigned[bestIdx] = bestIdx, iMP
            nmatches += 1                                # :397
    return dict(nmatches=nmatches, match=np.array(match, np.int32).reshape(-1), assigned=np.array(assigned, np.int32).reshape(-1), lost=lost,
                deep=deep)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def flip_bits(row, nbits, rng):
    """a copy of one descriptor with `nbits` different bits flipped"""
    out = np.array(row, np.uint8).copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def loop_pair(seed=3):
    """The current keyframe KF1 (first keyframe of kf_scene) and a loop candidate KF2: the second keyframe's keypoints, most of them
    carrying a noisy copy of a KF1 descriptor and an angle 10 degrees off KF1's (a revisit under a small roll); some KF1 features are
    near-copies of the feature before them, so that two queries of one node want the same KF2 feature."""
    (k0, d0), (k1, d1) = ks.keyframes()
    rng = np.random.default_rng(seed)
    k0, d0, k2, d2 = k0.copy(), d0.copy(), k1.copy(), d1.copy()
    for i in rng.choice(len(k0) - 1, 80, replace=False):
        d0[i + 1] = d0[i]
        d0[i + 1, 8 + rng.integers(0, 24)] ^= np.uint8(1 << rng.integers(0, 8))    # bytes 0 and 5 (the node hash) stay
    m = min(len(k0), len(k2))
    d2[:m] = ks.noisy_desc(d0[:m], rng, flips=12)
    ang = k0["angle"][:m] + np.float32(10.0) + rng.normal(0, 4.0, m).astype(np.float32)
    wild = rng.random(m) < 0.15
    ang[wild] = rng.uniform(0, 360, wild.sum()).astype(np.float32)
    k2["angle"][:m] = np.mod(ang, np.float32(360.0)).astype(np.float32)
    perm = rng.permutation(len(k2))                      # KF2's feature order has nothing to do with KF1's
    return k0, d0, k2[perm], d2[perm]


def perturbed(k2, d2, valid2, rng, keep=None):
    """another candidate: a prefix of KF2's features, descriptor bits flipped, the map-point mask reshuffled"""
    n = len(k2) if keep is None else keep
    return k2[:n].copy(), ks.noisy_desc(d2[:n], rng, flips=6), rng.permutation(valid2)[:n]


def bow_inputs(d1, angle1, valid1, fv1, fv2, valid2):
    """(fidx2, runs, qangle, qdesc, idx1) as pslfe_kf_search_by_bow takes them: KF2's FeatureVector flattened in node order without
    the features that have no good map point (:576-580); one query per KF1 feature with a good map point (:558-562), common nodes
    ascending (:550-632), the node's own order inside (:554)."""
    fidx, start = [], {}
    for nd in sorted(fv2):
        keep = [int(i) for i in fv2[nd] if valid2[i]]
        start[nd] = (len(fidx), len(keep))
        fidx.extend(keep)
    runs, qa, qd, idx1 = [], [], [], []
    for nd in sorted(fv1):
        if nd not in start:
            continue
        for i in fv1[nd]:
            if valid1[i]:
                runs.append(start[nd]); qa.append(angle1[i]); qd.append(d1[i]); idx1.append(int(i))
    return (np.array(fidx, np.int32).reshape(-1), np.array(runs, np.int32).reshape(-1, 2), np.array(qa, np.float32).reshape(-1),
            np.array(qd, np.uint8).reshape(-1, 32), np.array(idx1, np.int32).reshape(-1))


def boundary_pair(nbits, rng):
    """one KF2 feature alone in its node and a query that is its descriptor with `nbits` bits flipped"""
    d2 = rng.integers(0, 256, (3, 32), dtype=np.uint8)
    import oracle_lib
    k2 = np.zeros(3, oracle_lib.KEYPOINT_DTYPE)
    k2["x"], k2["y"] = [10.0, 20.0, 30.0], [10.0, 20.0, 30.0]
    fidx = np.array([1], np.int32)
    return k2, d2, fidx, np.array([[0, 1]], np.int32), np.zeros(1, np.float32), flip_bits(d2[1], nbits, rng).reshape(1, 32)


def loop_map_points(k, d, rng, th=10.0, copies=6, flips=30):
    """mvpLoopMapPoints seen from the current keyframe: `copies` map points per keypoint (the loop keyframe's neighbours observe
    the same places), projected near it, with the descriptor of another observation"""
    rep = np.concatenate([rng.permutation(len(k)) for _ in range(copies)])
    q = ks.proj_queries(k[rep], rng, th=th, jitter=3.0)
    return q, ks.noisy_desc(d[rep], rng, flips=flips)
