"""CPU checks of the monocular initialiser's matcher (include/pslfe.h: pslfe_orb_search_for_initialization): the sequential
restatement the GPU tests compare with (oracle/mono_init_oracle.cpp) against a literal numpy-float32 transcription of
ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:405-520), GetFeaturesInArea (src/Frame.cc:985-1038),
AssignFeaturesToGrid / PosInGrid and ComputeThreeMaxima, on random keypoint sets and constructed cases; and the argument checks
of the library, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

from mono_init_cases import BOUNDS, Case, constructed, one_tenth, random_pair, stolen_decides
from oracle_lib import KEYPOINT_DTYPE, restate_grid, restate_search

F32 = np.float32
INT_MAX = 2**31 - 1


def _round(x):
    """std::round of a float (half away from zero), exact."""
    x = np.float64(x)
    return F32(np.copysign(np.floor(abs(x) + 0.5), x))


def _popcount(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def transcription(k1, d1, k2, d2, bounds, prev, window, nnratio, check_ori):
    """src/ORBmatcher.cc:405-520 line by line in numpy float32, with the grid of src/Frame.cc:269-284 / 1040-1050 and
    GetFeaturesInArea :985-1038 (minLevel = maxLevel = 0) -> (nmatches, vnMatches12, vbPrevMatched)."""
    mnMinX, mnMinY, mnMaxX, mnMaxY = (F32(b) for b in bounds)
    invW = F32(F32(64) / F32(mnMaxX - mnMinX))
    invH = F32(F32(48) / F32(mnMaxY - mnMinY))
    grid = [[[] for _ in range(48)] for _ in range(64)]
    for i in range(len(k2)):
        posX = int(_round(F32(F32(k2["x"][i]) - mnMinX) * invW))
        posY = int(_round(F32(F32(k2["y"][i]) - mnMinY) * invH))
        if 0 <= posX < 64 and 0 <= posY < 48:
            grid[posX][posY].append(i)

    def get_features_in_area(x, y, r, minLevel, maxLevel):
        v = []
        nMinCellX = max(0, int(np.floor(F32(F32(F32(x - mnMinX) - r) * invW))))
        if nMinCellX >= 64:
            return v
        nMaxCellX = min(63, int(np.ceil(F32(F32(F32(x - mnMinX) + r) * invW))))
        if nMaxCellX < 0:
            return v
        nMinCellY = max(0, int(np.floor(F32(F32(F32(y - mnMinY) - r) * invH))))
        if nMinCellY >= 48:
            return v
        nMaxCellY = min(47, int(np.ceil(F32(F32(F32(y - mnMinY) + r) * invH))))
        if nMaxCellY < 0:
            return v
        bCheckLevels = minLevel > 0 or maxLevel >= 0
        for ix in range(nMinCellX, nMaxCellX + 1):
            for iy in range(nMinCellY, nMaxCellY + 1):
                for j in grid[ix][iy]:
                    if bCheckLevels:
                        if k2["octave"][j] < minLevel:
                            continue
                        if maxLevel >= 0 and k2["octave"][j] > maxLevel:
                            continue
                    distx = F32(F32(k2["x"][j]) - x)
                    disty = F32(F32(k2["y"][j]) - y)
                    if abs(distx) < r and abs(disty) < r:
                        v.append(j)
        return v

    HISTO_LENGTH, TH_LOW = 30, 50
    vbPrevMatched = np.array(prev, F32).reshape(-1, 2).copy()
    nmatches = 0
    vnMatches12 = [-1] * len(k1)
    rotHist = [[] for _ in range(HISTO_LENGTH)]
    factor = F32(F32(1.0) / F32(HISTO_LENGTH))
    vMatchedDistance = [INT_MAX] * len(k2)
    vnMatches21 = [-1] * len(k2)
    r = F32(window)
    for i1 in range(len(k1)):
        level1 = int(k1["octave"][i1])
        if level1 > 0:
            continue
        vIndices2 = get_features_in_area(vbPrevMatched[i1, 0], vbPrevMatched[i1, 1], r, level1, level1)
        if not vIndices2:
            continue
        bestDist, bestDist2, bestIdx2 = INT_MAX, INT_MAX, -1
        for i2 in vIndices2:
            dist = _popcount(d1[i1], d2[i2])
            if vMatchedDistance[i2] <= dist:
                continue
            if dist < bestDist:
                bestDist2, bestDist, bestIdx2 = bestDist, dist, i2
            elif dist < bestDist2:
                bestDist2 = dist
        if bestDist <= TH_LOW:
            if F32(bestDist) < F32(F32(bestDist2) * F32(nnratio)):
                if vnMatches21[bestIdx2] >= 0:
                    vnMatches12[vnMatches21[bestIdx2]] = -1
                    nmatches -= 1
                vnMatches12[i1] = bestIdx2
                vnMatches21[bestIdx2] = i1
                vMatchedDistance[bestIdx2] = bestDist
                nmatches += 1
                if check_ori:
                    rot = F32(F32(k1["angle"][i1]) - F32(k2["angle"][bestIdx2]))
                    if rot < 0.0:
                        rot = F32(rot + F32(360.0))
                    b = int(_round(F32(rot * factor)))
                    if b == HISTO_LENGTH:
                        b = 0
                    assert 0 <= b < HISTO_LENGTH
                    rotHist[b].append(i1)
    if check_ori:
        max1 = max2 = max3 = 0
        ind1 = ind2 = ind3 = -1
        for i in range(HISTO_LENGTH):
            s = len(rotHist[i])
            if s > max1:
                max3, max2, max1 = max2, max1, s
                ind3, ind2, ind1 = ind2, ind1, i
            elif s > max2:
                max3, max2 = max2, s
                ind3, ind2 = ind2, i
            elif s > max3:
                max3, ind3 = s, i
        if F32(max2) < F32(F32(0.1) * F32(max1)):
            ind2 = ind3 = -1
        elif F32(max3) < F32(F32(0.1) * F32(max1)):
            ind3 = -1
        for i in range(HISTO_LENGTH):
            if i in (ind1, ind2, ind3):
                continue
            for idx1 in rotHist[i]:
                if vnMatches12[idx1] >= 0:
                    vnMatches12[idx1] = -1
                    nmatches -= 1
    for i1 in range(len(vnMatches12)):
        if vnMatches12[i1] >= 0:
            vbPrevMatched[i1] = (k2["x"][vnMatches12[i1]], k2["y"][vnMatches12[i1]])
    return nmatches, np.array(vnMatches12, np.int32), vbPrevMatched


def assert_same(got, want, what):
    nm, m12, pv = got[:3]
    wnm, wm12, wpv = want[:3]
    assert nm == wnm, f"{what}: nmatches {nm} != {wnm}"
    assert np.array_equal(np.asarray(m12), wm12), f"{what}: matches differ"
    assert np.asarray(pv, F32).tobytes() == np.asarray(wpv, F32).tobytes(), f"{what}: prev differs"



@pytest.mark.parametrize("check_ori", [True, False])
def test_restatement_equals_transcription_random(check_ori):
    rng = np.random.default_rng(11 if check_ori else 12)
    for rep in range(8):
        n1, n2 = (300, 300) if rep == 0 else (int(rng.integers(0, 400)), int(rng.integers(0, 400)))
        k1, d1, k2, d2, prev = random_pair(rng, n1, n2)
        window = 100 if rep == 0 else int(rng.choice([10, 50, 100]))
        got = restate_search(k1, d1, k2, d2, BOUNDS, prev, window, 0.9, check_ori)
        want = transcription(k1, d1, k2, d2, BOUNDS, prev, window, 0.9, check_ori)
        assert_same(got, want, f"rep {rep}")
        if rep == 0:
            assert got[0] > 0


@pytest.mark.parametrize("check_ori", [True, False])
def test_constructed_cases(check_ori):
    rng = np.random.default_rng(3)
    c = Case()
    ids = constructed(c, rng)
    k1, d1, k2, d2, prev = c.arrays()
    got = restate_search(k1, d1, k2, d2, BOUNDS, prev, 20, 0.9, check_ori)
    assert_same(got, transcription(k1, d1, k2, d2, BOUNDS, prev, 20, 0.9, check_ori), "constructed")
    loose = restate_search(k1, d1, k2, d2, BOUNDS, prev, 20, 1.5, check_ori)
    assert_same(loose, transcription(k1, d1, k2, d2, BOUNDS, prev, 20, 1.5, check_ori), "constructed, nnratio 1.5")
    nm, m12, pv, acc = got
    k, qs = ids["chain"]
    assert [acc[q] for q in qs] == [k, k, k] and [m12[q] for q in qs] == [-1, -1, k]
    q, left, right = ids["tie"]
    assert acc[q] == -1 and loose[3][q] == left   # equal best and second best fail 0.9; with 1.5 the first visited wins
    q, X, Y, Z = ids["filt"]
    assert acc[q] == -1 and loose[3][q] == Y      # X filtered: 20 against the second best 22 (not 12 against 20, which passes)
    q, k = ids["single"]
    assert m12[q] == k
    q, q0, k, k_hi = ids["skip"]
    assert acc[q] == -1 and acc[q0] == -1
    assert acc[ids["out"]] == -1 and pv[ids["out"]].tolist() == [-500.0, 2000.0]


def test_stolen_entry_decides_the_maxima():
    rng = np.random.default_rng(8)
    c = Case()
    A, B, kA, CD = stolen_decides(c, rng)
    k1, d1, k2, d2, prev = c.arrays()
    got = restate_search(k1, d1, k2, d2, BOUNDS, prev, 10, 0.9, True)
    assert_same(got, transcription(k1, d1, k2, d2, BOUNDS, prev, 10, 0.9, True), "stolen entry")
    nm, m12, _, acc = got
    assert acc[A] == kA and m12[A] == -1 and m12[B] == kA
    assert all(m12[q] >= 0 for q in CD) and nm == 24 + 1 + 2


def test_three_maxima_at_one_tenth():
    rng = np.random.default_rng(9)
    c = Case()
    q5, q8, q10 = one_tenth(c, rng)
    k1, d1, k2, d2, prev = c.arrays()
    got = restate_search(k1, d1, k2, d2, BOUNDS, prev, 10, 0.9, True)
    assert_same(got, transcription(k1, d1, k2, d2, BOUNDS, prev, 10, 0.9, True), "one tenth")
    nm, m12 = got[0], got[1]
    assert m12[q5] >= 0 and m12[q8] >= 0 and m12[q10] == -1 and nm == 12


def test_grid_equals_transcription():
    rng = np.random.default_rng(4)
    n = 500
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(-10, 650, n), rng.uniform(-10, 490, n)
    bounds = (-3.5, -2.25, 641.0, 482.5)
    start, idx = restate_grid(k, bounds)
    mnMinX, mnMinY, mnMaxX, mnMaxY = (F32(b) for b in bounds)
    invW, invH = F32(F32(64) / F32(mnMaxX - mnMinX)), F32(F32(48) / F32(mnMaxY - mnMinY))
    cells = [[] for _ in range(64 * 48)]
    for i in range(n):
        px = int(_round(F32(F32(k["x"][i]) - mnMinX) * invW))
        py = int(_round(F32(F32(k["y"][i]) - mnMinY) * invH))
        if 0 <= px < 64 and 0 <= py < 48:
            cells[px * 48 + py].append(i)
    assert idx.tolist() == [i for cl in cells for i in cl]
    assert start.tolist() == [0] + [int(v) for v in np.cumsum([len(cl) for cl in cells])]


def test_mono_entry_points_reject_null_arguments_without_a_gpu():
    import psl_slam_amd as P
    P.build()
    L = P.lib()
    E = -1  # PSLFE_E_INVALID
    n = C.c_int(3)
    prev = np.zeros(2, F32)
    m = np.zeros(1, np.int32)
    s = np.zeros(1, np.int32)
    assert L.pslfe_frame_set_from_orb_mono(None, 0, None, 0, 1, None) == E
    assert "NULL" in L.pslfe_last_error().decode()
    assert L.pslfe_orb_search_for_initialization(None, 0, None, 0, C.c_void_p(prev.ctypes.data), 100, C.c_float(0.9), 1,
                                                 C.c_void_p(m.ctypes.data), C.byref(n)) == E
    assert "NULL" in L.pslfe_last_error().decode()
    assert L.pslfe_orb_search_for_initialization_device(None, C.c_void_p(s.ctypes.data), None, C.c_void_p(s.ctypes.data), 1, None, 1, 100,
                                                        C.c_float(0.9), 1, None, None) == E
    assert "NULL" in L.pslfe_last_error().decode()
