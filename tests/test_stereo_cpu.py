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
from stereo_cases import level_sizes, random_keypoints, transcription   # shared with the hand-made cases and their GPU run

F32 = np.float32


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
    kL, dL, kR, dR = random_keypoints(rng, kind, w, h, scale, shift)
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
