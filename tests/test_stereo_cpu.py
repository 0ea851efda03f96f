"""CPU checks of the stereo constructor (include/pslfe.h: pslfe_frame_set_from_orb_stereo): the sequential restatement the GPU
tests compare with (oracle/stereo_oracle.cpp) against a literal numpy-float32 transcription of Frame::ComputeStereoMatches
(src/Frame.cc:1165-1340) on random keypoint sets, level images and edge cases; the depth it recovers on a constant-disparity
pair; and the argument checks of the library, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

import synth_frames as sf
import stereo_scene as ss
from oracle_lib import KEYPOINT_DTYPE, restate_stereo

F32 = np.float32


def _round(x):
    """std::round of a float (half away from zero), exact."""
    x = np.float64(x)
    return F32(np.copysign(np.floor(abs(x) + 0.5), x))


def transcription(kL, dL, kR, dR, levL, levR, scale, inv_scale, bf, fx):
    """src/Frame.cc:1165-1340 line by line in numpy float32, with the conventions of include/pslfe.h where the reference is
    undefined (mb = mbf/fx, empty vDistIdx, rows / windows outside the image)."""
    N, Nr = len(kL), len(kR)
    mvuRight = np.full(N, -1.0, F32)
    mvDepth = np.full(N, -1.0, F32)
    t_idx, t_sad = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    thOrbDist = (100 + 50) // 2
    nRows = levL[0].shape[0]
    vRowIndices = [[] for _ in range(nRows)]
    for iR in range(Nr):
        kpY = F32(kR["y"][iR])
        r = F32(F32(2.0) * F32(scale[kR["octave"][iR]]))
        maxr = int(np.ceil(F32(kpY + r)))
        minr = int(np.floor(F32(kpY - r)))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < nRows:
                vRowIndices[yi].append(iR)
    mbf = F32(bf)
    mb = F32(mbf / F32(fx))
    minZ = mb
    minD = F32(0)
    maxD = F32(mbf / minZ)
    vDistIdx = []
    for iL in range(N):
        levelL = int(kL["octave"][iL])
        vL, uL = F32(kL["y"][iL]), F32(kL["x"][iL])
        if not (0 <= vL < nRows):
            continue
        vCandidates = vRowIndices[int(vL)]
        if not vCandidates:
            continue
        minU = F32(uL - maxD)
        maxU = F32(uL - minD)
        if maxU < 0:
            continue
        bestDist, bestIdxR = 100, 0
        for iR in vCandidates:
            if kR["octave"][iR] < levelL - 1 or kR["octave"][iR] > levelL + 1:
                continue
            uR = F32(kR["x"][iR])
            if uR >= minU and uR <= maxU:
                dist = int(np.unpackbits(dL[iL] ^ dR[iR]).sum())
                if dist < bestDist:
                    bestDist, bestIdxR = dist, iR
        if bestDist < thOrbDist:
            t_idx[iL] = bestIdxR
            uR0 = F32(kR["x"][bestIdxR])
            scaleFactor = F32(inv_scale[levelL])
            scaleduL = _round(F32(uL * scaleFactor))
            scaledvL = _round(F32(vL * scaleFactor))
            scaleduR0 = _round(F32(uR0 * scaleFactor))
            w = L = 5
            IMl, IMr = levL[levelL], levR[levelL]
            iniu = F32(F32(scaleduR0 + F32(L)) - F32(w))
            endu = F32(F32(F32(scaleduR0 + F32(L)) + F32(w)) + F32(1))
            if iniu < 0 or endu >= IMr.shape[1]:
                continue
            rows, cols = IMl.shape
            if not (scaledvL >= 5 and scaledvL + 5 < rows and scaleduL >= 5 and scaleduL + 5 < cols and scaleduR0 >= 10 and
                    scaleduR0 + 10 < cols):
                continue
            y0, xl, xr = int(scaledvL), int(scaleduL), int(scaleduR0)
            IL = IMl[y0 - w:y0 + w + 1, xl - w:xl + w + 1].astype(F32)
            IL = IL - IL[w, w] * np.ones(IL.shape, F32)
            best, bestincR = 2 ** 31 - 1, 0
            vDists = [F32(0)] * (2 * L + 1)
            for incR in range(-L, L + 1):
                IR = IMr[y0 - w:y0 + w + 1, xr + incR - w:xr + incR + w + 1].astype(F32)
                IR = IR - IR[w, w] * np.ones(IR.shape, F32)
                dist = F32(np.abs(IL - IR).astype(np.float64).sum())    # cv::norm NORM_L1 (exact: integers below 2^24)
                if dist < best:
                    best, bestincR = int(dist), incR
                vDists[L + incR] = dist
            if bestincR == -L or bestincR == L:
                continue
            dist1, dist2, dist3 = vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1]
            deltaR = F32(F32(dist1 - dist3) / F32(F32(2.0) * F32(F32(dist1 + dist3) - F32(F32(2.0) * dist2))))
            if deltaR < -1 or deltaR > 1:
                continue
            bestuR = F32(F32(scale[levelL]) * F32(F32(scaleduR0 + F32(bestincR)) + deltaR))
            disparity = F32(uL - bestuR)
            if disparity >= minD and disparity < maxD:
                if disparity <= 0:
                    disparity = F32(0.01)
                    bestuR = F32(np.float64(uL) - 0.01)
                mvDepth[iL] = F32(mbf / disparity)
                mvuRight[iL] = bestuR
                t_sad[iL] = best
                vDistIdx.append((best, iL))
    if vDistIdx:
        vDistIdx.sort()
        median = F32(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F32(F32(F32(1.5) * F32(1.4)) * median)
        for i in range(len(vDistIdx) - 1, -1, -1):
            if vDistIdx[i][0] < thDist:
                break
            mvuRight[vDistIdx[i][1]] = -1
            mvDepth[vDistIdx[i][1]] = -1
    return mvuRight, mvDepth, t_idx, t_sad


def level_sizes(w, h, inv_scale):
    return [(int(np.rint(F32(w) * F32(s))), int(np.rint(F32(h) * F32(s)))) for s in inv_scale]


def random_case(rng, kind):
    """Random keypoints / descriptors / level images with a planted fraction of true matches."""
    nlevels = 8
    scale = sf.orb_scale_factors(nlevels, 1.2)
    inv = (F32(1.0) / scale).astype(F32)
    w, h = int(rng.integers(140, 260)), int(rng.integers(100, 200))
    levL, levR = [], []
    shift = int(rng.integers(-3, 9))
    for lw, lh in level_sizes(w, h, inv):
        if kind == "periodic":
            a = ss.periodic(lw, lh, 6)
        else:
            a = rng.integers(0, 256, (lh, lw), dtype=np.uint8)
        pad = int(rng.integers(0, 9))                                  # any pitch
        A = np.zeros((lh, lw + pad), np.uint8)
        A[:, :lw] = a
        B = np.zeros((lh, lw + pad), np.uint8)
        B[:, :lw] = np.roll(a, -shift, axis=1) if kind != "flat" else 128
        if kind == "noise_r":
            B[:, :lw] = np.clip(B[:, :lw].astype(int) + rng.integers(-6, 7, (lh, lw)), 0, 255)
        levL.append(A[:, :lw])
        levR.append(B[:, :lw])
    nL = int(rng.integers(0, 120)) if kind != "empty_left" else 0
    nR = int(rng.integers(0, 150)) if kind != "empty_right" else 0
    oct_hi = 8

    def kps(n, lo_oct):
        k = np.zeros(n, KEYPOINT_DTYPE)
        k["octave"] = rng.integers(lo_oct, oct_hi, n)
        s = scale[k["octave"]]
        k["x"] = (rng.uniform(8, (w / s) - 8, n) * s).astype(F32)     # near the level borders too: windows outside the image
        k["y"] = (rng.uniform(8, (h / s) - 8, n) * s).astype(F32)
        return k
    lo = 6 if kind == "high_octave" else 0
    kL, kR = kps(nL, lo), kps(nR, lo)
    dL = rng.integers(0, 256, (nL, 32), dtype=np.uint8)
    dR = rng.integers(0, 256, (nR, 32), dtype=np.uint8)
    # plant matches: right keypoints near a left one (same row band, shifted left), descriptors a few bits apart
    for j in range(min(nL, nR, int(rng.integers(0, 80)))):
        i = int(rng.integers(0, nL))
        kR[j]["octave"] = int(np.clip(kL[i]["octave"] + rng.integers(-1, 2), lo, 7))
        kR[j]["y"] = F32(kL[i]["y"] + rng.uniform(-3, 3))
        kR[j]["x"] = F32(kL[i]["x"] - shift * scale[kL[i]["octave"]] + rng.choice([0.0, rng.uniform(-8, 8), 6.0 * scale[kL[i]["octave"]]]))
        flips = rng.integers(0, 256, 32, dtype=np.uint8) & rng.choice([0, 1, 3, 0x11, 0xff], 32).astype(np.uint8)
        dR[j] = dL[i] ^ flips
        if kind == "ties" and j + 1 < nR:                               # an equal-distance twin at a higher index
            kR[j + 1] = kR[j]
            dR[j + 1] = dR[j]
    if kind == "maxu_negative":
        kL["x"][: nL // 2] = F32(-3.0)
    if kind == "outside_rows":
        kL["y"][: nL // 3] = F32(h + 5.0)
        kR["y"][: nR // 3] = F32(-4.0)
    return kL, dL, kR, dR, levL, levR, scale, inv


KINDS = ["noise", "noise_r", "periodic", "ties", "high_octave", "maxu_negative", "outside_rows", "flat", "empty_left", "empty_right"]
CAMS = [(40.0, 517.3), (47.906, 435.2), (386.1448, 718.856), (0.5, 500.0)]


@pytest.mark.parametrize("kind", KINDS)
def test_restatement_equals_transcription(kind):
    rng = np.random.default_rng(zlib_seed(kind))
    seen = dict(sad=0, filtered=0, edge=0, empty=0)
    for rep in range(30):
        kL, dL, kR, dR, levL, levR, scale, inv = random_case(rng, kind)
        bf, fx = CAMS[rep % len(CAMS)]
        got = restate_stereo(kL, dL, kR, dR, levL, levR, scale, inv, bf, fx)
        want = transcription(kL, dL, kR, dR, levL, levR, scale, inv, bf, fx)
        for g, x, name in zip(got, want, ("uright", "depth", "idx", "sad")):
            assert g.tobytes() == x.tobytes(), f"{kind} #{rep}: {name} differs"
        seen["sad"] += int((got[3] >= 0).sum())
        seen["filtered"] += int(((got[3] >= 0) & (got[0] < 0)).sum())
        seen["edge"] += int(((got[2] >= 0) & (got[3] < 0)).sum())
        seen["empty"] += int((got[3] >= 0).sum() == 0)
    if kind in ("noise", "noise_r", "ties", "periodic"):
        assert seen["sad"] > 0 and seen["edge"] > 0, seen
    if kind in ("flat", "empty_left", "empty_right"):
        assert seen["empty"] == 30


def zlib_seed(s):
    import zlib
    return zlib.crc32(s.encode())


def test_restatement_bestinc_edges_and_median():
    """A window sweep whose minimum sits at incR = +-5 is rejected; the median filter drops the worst SADs."""
    rng = np.random.default_rng(5)
    scale = sf.orb_scale_factors(8, 1.2)
    inv = (F32(1.0) / scale).astype(F32)
    w, h = 200, 120
    levL, levR = [], []
    for lw, lh in level_sizes(w, h, inv):
        a = rng.integers(0, 256, (lh, lw), dtype=np.uint8)
        levL.append(a)
        b = np.roll(a, -20, axis=1) if lw == w else a          # level 0: the true disparity 20 px, plus noise (SAD minima > 0)
        levR.append(np.clip(b.astype(int) + rng.integers(-8, 9, b.shape), 0, 255).astype(np.uint8))
    n = 40
    kL = np.zeros(n, KEYPOINT_DTYPE)
    kL["x"], kL["y"] = rng.uniform(60, 180, n).astype(F32), rng.uniform(20, 100, n).astype(F32)
    kR = kL.copy()
    kR["x"] = kL["x"] - F32(20.0)
    kR["x"][:10] += F32(5.0)       # right keypoint 5 px off: the minimum at incR = -5 -> rejected
    kR["x"][10:20] += F32(3.0)
    dL = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    ur, dep, idx, sad = restate_stereo(kL, dL, kR, dL.copy(), levL, levR, scale, inv, 40.0, 500.0)
    want = transcription(kL, dL, kR, dL.copy(), levL, levR, scale, inv, 40.0, 500.0)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((ur, dep, idx, sad), want))
    assert (idx == np.arange(n)).all()
    assert (sad[:10] == -1).all() and (sad[10:] >= 0).all()
    assert (dep[10:] > 0).any()


def test_constant_disparity_depth():
    """On a pair shifted by a constant disparity the recovered depth is bf/d within 1 % for most accepted keypoints (sanity,
    not parity).  Keypoints and pyramids from the CPU oracle of the extractor."""
    import oracle_lib
    w, h, d, bf = 640, 480, 64.0, 40.0   # the parabola's bias is a fraction of a pixel: 1 % of depth needs a wide disparity
    left = ss.textured(w, h)
    right = ss.sample_rows(left, d)
    oL, oR = oracle_lib.OracleORB(1000, 1.2, 8, 20, 7), oracle_lib.OracleORB(1000, 1.2, 8, 20, 7)
    kL, dL = oL(left)
    kR, dR = oR(right)
    levL = [oL.level_image(l) for l in range(8)]
    levR = [oR.level_image(l) for l in range(8)]
    scale = sf.orb_scale_factors(8, 1.2)
    inv = (F32(1.0) / scale).astype(F32)
    ur, dep, idx, sad = restate_stereo(kL, dL, kR, dR, levL, levR, scale, inv, bf, 517.3)
    ok = dep > 0
    assert ok.sum() >= 100, ok.sum()
    rel = np.abs(dep[ok] / (bf / d) - 1.0)
    assert (rel < 0.01).mean() >= 0.8, (rel < 0.01).mean()


def test_stereo_entry_points_reject_null_arguments_without_a_gpu():
    import psl_slam_amd as P
    P.build()
    L = P.lib()
    E = -1  # PSLFE_E_INVALID
    n = C.c_int(3)
    assert L.pslfe_frame_set_from_orb_stereo(None, 0, None, 0, None, 0, 1, None) == E
    assert "NULL" in L.pslfe_last_error().decode()
    assert L.pslfe_frame_debug_stereo(None, 0, None, None, 0, C.byref(n)) == E
    assert L.pslfe_frame_debug_stereo(None, 0, None, None, 0, None) == E
