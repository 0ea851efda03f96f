"""The three image kernels of the ORB extractor that work on whole levels or patches (k_pyr_resize_tiled, k_blur7, k_orient_describe of
psl-slam_amd/csrc/orb_kernels.h) at the inputs where their index arithmetic can go wrong, bit-exact against the oracle, stage by
stage as tests/test_orb_gpu.py does it: level images, FAST candidates, octree keypoints, blurred levels, keypoints with their angles,
descriptors.

  k_pyr_resize_tiled   the `staged && fits` path cuts a tap pair out of three dwords with a selector formed once per thread: every
                       byte offset of the last tap, pixels 2 and 3 in the first and in the second dword pair, and a last pair that
                       starts at byte 7 (the only one that needs the third dword); level widths of every rest mod 4, and the
                       thread whose four pixels straddle the level's last column (width sweep with three levels; the sweep
                       of tests/test_orb_edges_gpu.py has one level and never resizes)
  k_orient_describe    one loop for both half-discs, bounded per column by vmax(|u|): a single bright pixel at every octant, on and
                       just outside the rim of the disc, and on the row v = 0; keypoints at the smallest distance from every border
                       (the patch loads clamp there) and on all eight levels; waves that leave early (1 feature) and the cap
                       (4 nIni); the byte-wise orientation patch of unaligned device input; 1 and 9 frames per launch
"""
import numpy as np
import pytest

import orb_cases as oc
import synth_frames as sf
from test_orb_gpu import _assert_same_stages

on_gpu = pytest.mark.gpu      # the two tests without it restate tables and need no GPU

UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]    # src/ORBextractor.cc:452-469 (tests/test_oracle_cpu.py)


def _pair(max_batch=1, **cfg):
    import psl_slam_amd as P
    import oracle_lib
    return P.ORBextractor(max_batch=max_batch, **cfg), oracle_lib.OracleORB(**cfg)


# ---- width sweep ---------------------------------------------------------------------------------------------------------------
def _sweep_case(w, sf_):
    """Three levels where the third still holds a FAST cell (at h = 92: factors 1.1 and 1.2; 92 / 1.3^2 = 54 rows hold none and both
    the extractor and the reference reject it), else two: level 1 is the resize that the factor is there for."""
    for nl in (3, 2):
        c = oc._case(f"width_{w}_x{sf_}", w, 92, sf_, nl, 100, image="noise")
        if oc.case_geometry(c)["error"] is None:
            return c
    raise AssertionError((w, sf_))


SWEEP = [_sweep_case(w, 1.2) for w in range(92, 157)] + [_sweep_case(w, s) for s in (1.1, 1.3) for w in range(92, 157, 4)]


def _thread_ofs(sw, dw):
    """ofs[0..3] of every 4-pixel thread of k_pyr_resize_tiled that makes pixels of a level of width dw from one of width sw, and x4."""
    xofs = oc._linear_ofs(sw, dw, True)
    dpitch = (dw + 15) // 16 * 16
    out = []
    for x0 in range(0, dpitch, 64):
        cbase = int(xofs[min(x0, dw - 1)]) & ~3
        for x4 in range(x0, min(x0 + 64, dpitch), 4):
            sx = [int(xofs[min(x4 + j, dw - 1)]) for j in range(4)]
            d0 = (sx[0] - cbase) >> 2
            out.append((x4, [s - cbase - 4 * d0 for s in sx]))
    return out


def test_width_sweep_reaches_every_selector_of_the_fits_path():
    """No GPU: the claims about the sweep that make it a test of the selector, from the restated tables alone."""
    assert [c["nlevels"] for c in SWEEP if c["scaleFactor"] != 1.3] == [3] * (65 + 17) and len(SWEEP) == 65 + 2 * 17
    last, pix2, pix3, rests, straddle = set(), set(), set(), set(), 0
    for c in SWEEP:
        lv = oc.case_geometry(c)["levels"]
        assert lv[-1]["cells"] >= 1
        for l in range(1, c["nlevels"]):
            # a host image is copied to rows of 16-byte pitch, as every derived level has them (orb_cases.geometry takes w for level 0)
            blocks = oc._pyr_blocks(lv[l - 1]["w"], lv[l - 1]["h"], lv[l - 1]["pitch"], lv[l]["w"], lv[l]["h"], True)
            assert all(b["staged"] and b["unfit"] == 0 for b in blocks), c["name"]
            rests.add(lv[l]["w"] % 4)
            for x4, ofs in _thread_ofs(lv[l - 1]["w"], lv[l]["w"]):
                assert 0 <= ofs[0] <= 3 and ofs[0] <= ofs[1] <= ofs[2] <= ofs[3] <= 7
                if x4 < lv[l]["w"]:
                    last.add(ofs[3]); pix2.add(ofs[2]); pix3.add(ofs[3])
                    straddle += x4 + 4 > lv[l]["w"]
    assert last >= {3, 4, 5, 6, 7}, last                               # the last tap at bytes 3 .. 7
    for seen in (pix2, pix3):                                          # pixels 2 and 3 in the first dword pair and in the second
        assert any(o <= 3 for o in seen) and any(4 <= o <= 6 for o in seen), seen
    assert 7 in pix3 and 7 not in pix2                                 # the pair that starts at byte 7 and needs the third dword
    assert rests == {0, 1, 2, 3}
    assert straddle > len(SWEEP) // 2                                  # a last thread whose four pixels straddle L.w


def test_umax_does_not_increase():
    """No GPU: k_orient_describe bounds a column of the disc by vmax(|u|), the largest v with |u| <= umax[v]; that is the same set of
    rows as the reference's `for u in -umax[v] .. umax[v]` only if umax[] never increases with v."""
    import oracle_lib
    o = oracle_lib.OracleORB(100, 1.2, 1, 20, 7)
    umax = [o.L.pso_orb_umax(o.h, v) for v in range(16)]
    assert umax == UMAX and all(umax[v] <= umax[v - 1] for v in range(1, 16)) and umax[0] == 15


@on_gpu
def test_width_sweep_with_three_levels_equals_the_oracle():
    for c in SWEEP:
        gpu, orc = _pair(**oc.case_config(c))
        img = oc.case_image(c)
        _assert_same_stages(gpu, orc, gpu(img), orc(img), c["nlevels"], c["name"])


# ---- orientation of one keypoint -----------------------------------------------------------------------------------------------
def _blob_offsets():
    octants = [(5, 2), (2, 5), (-2, 5), (-5, 2), (-5, -2), (-2, -5), (2, -5), (5, -2)]
    rim = [(15, 0), (-15, 0), (0, 15), (0, -15)]
    for v in range(16):
        for su in (1, -1):
            for sv in ((1, -1) if v else (1,)):
                rim += [(su * UMAX[v], sv * v), (su * (UMAX[v] + 1), sv * v)]
    row0 = [(7, 0), (-7, 0), (1, 0), (-1, 0), (14, 0), (-14, 0)]
    return octants, rim, row0


def _blob_image(u, v):
    """92 x 92, dark: a pixel of 200 at (46, 46), which is the one FAST corner, and a pixel of 5 (no corner: it scores 4) at (46 + u,
    46 + v).  The intensity centroid over the disc is then m10 = 5 u, m01 = 5 v, or 0, 0 when the second pixel lies outside it."""
    img = np.zeros((92, 92), np.uint8)
    img[46, 46] = 200
    img[46 + v, 46 + u] = 5
    return img


@on_gpu
def test_one_keypoint_with_a_second_pixel_across_the_disc():
    octants, rim, row0 = _blob_offsets()
    cases = octants + rim + row0
    assert len({(u > 0, v > 0, abs(u) > abs(v)) for u, v in octants}) == 8
    frames = np.stack([_blob_image(u, v) for u, v in cases])
    gpu, orc = _pair(max_batch=len(cases), nfeatures=100, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7)
    res = gpu.extract_batch(frames)
    inside = outside = 0
    for f, (u, v) in enumerate(cases):
        ref = orc(frames[f])
        _assert_same_stages(gpu, orc, res[f], ref, 1, f"second pixel at ({u}, {v})", frame=f)
        k = res[f][0]
        assert len(k) == 1 and (k["x"][0], k["y"][0]) == (46.0, 46.0)
        if abs(v) <= 15 and abs(u) <= UMAX[abs(v)]:
            want = np.degrees(np.arctan2(v, u)) % 360.0               # fastAtan2 is good to 0.3 degrees
            assert abs((k["angle"][0] - want + 180.0) % 360.0 - 180.0) < 0.3, (u, v, k["angle"][0], want)
            inside += 1
        else:
            assert k["angle"][0] == 0.0, (u, v, k["angle"][0])         # nothing but the centre inside the disc: fastAtan2(0, 0)
            outside += 1
    assert inside > 60 and outside > 50


# ---- keypoint placement --------------------------------------------------------------------------------------------------------
@on_gpu
def test_keypoints_on_all_eight_levels():
    img = sf.Scene(320, 240, "desk", seed=320 * 7 + 240).gray(1)
    cfg = dict(nfeatures=500, scaleFactor=1.2, nlevels=8, iniThFAST=20, minThFAST=7)
    gpu, orc = _pair(**cfg)
    got, ref = gpu(img), orc(img)
    _assert_same_stages(gpu, orc, got, ref, 8, "320x240, 8 levels")
    assert set(got[0]["octave"]) == set(range(8))


@on_gpu
def test_keypoints_at_the_smallest_distance_from_every_border():
    """FAST scans a cell from its fourth pixel on, so the first and last keypoint columns are 19 and w - 20 (rows likewise).  The
    descriptor patch of such a keypoint starts at row 1 / ends at row h - 2, and its dword loads are the ones that the kernel clamps
    to the level.  The background is faint noise, so that a sample taken from a wrong place shows in the descriptor."""
    L = oc.geometry(oc.DOT_W, oc.DOT_H, 1.2, 1, 1)["levels"][0]
    X1, Y1 = L["W"] - 4, L["H"] - 4
    dots = [(3, 3, 60), (X1, 3, -60), (3, Y1, -60), (X1, Y1, 60), (150, 3, 60), (150, Y1, -60), (3, 100, 60), (X1, 100, -60), (150, 100, 60)]
    img = oc.dot_image(dots)
    noise = sf.random_gray(oc.DOT_W, oc.DOT_H, 5, "noise") % 3
    img = (img + noise).astype(np.uint8)
    gpu, orc = _pair(nfeatures=300, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7)
    got, ref = gpu(img), orc(img)
    _assert_same_stages(gpu, orc, got, ref, 1, "border dots")
    k = got[0]
    assert len(k) == len(dots)
    assert {(int(x), int(y)) for x, y in zip(k["x"], k["y"])} == {(X + oc.EDGE, Y + oc.EDGE) for X, Y, _ in dots}
    assert k["x"].min() == 19 and k["x"].max() == oc.DOT_W - 20 and k["y"].min() == 19 and k["y"].max() == oc.DOT_H - 20


# ---- feature caps --------------------------------------------------------------------------------------------------------------
@on_gpu
@pytest.mark.parametrize("nfeatures,nlevels,image", [(1, 8, "desk"), (4, 8, "desk"), (1, 1, "noise"), (4, 1, "noise")])
def test_feature_caps(nfeatures, nlevels, image):
    """nfeatures = 1: all but a few waves of k_orient_describe find no keypoint and leave, and a level's capacity is 4 nIni, not
    quota + 3.  nfeatures = 4 = 4 nIni of level 0 (320 x 240: nIni = 1).  On noise the octree fills what it is given."""
    c = oc._case("cap", 320, 240, 1.2, nlevels, nfeatures, image=image)
    lv = oc.case_geometry(c)["levels"]
    assert lv[0]["nIni"] == 1 and (nfeatures > 1 or all(L["kp_cap"] == 4 * L["nIni"] for L in lv))
    gpu, orc = _pair(**oc.case_config(c))
    img = oc.case_image(c)
    got, ref = gpu(img), orc(img)
    _assert_same_stages(gpu, orc, got, ref, nlevels, f"nfeatures {nfeatures}, {nlevels} levels")
    assert 0 < len(got[0]) <= sum(L["kp_cap"] for L in lv) == gpu.max_keypoints(320, 240)
    if image == "noise":
        assert len(got[0]) >= nfeatures


# ---- device input layouts ------------------------------------------------------------------------------------------------------
W, H = 320, 240
DEV_CFG = dict(nfeatures=500, scaleFactor=1.2, nlevels=3, iniThFAST=20, minThFAST=7)
# (name, base offset, stride): the single-frame layouts of tests/test_orb_edges_gpu.py
LAYOUTS = [("aligned", 0, 320), ("base+1", 1, 320), ("base+2", 2, 320), ("base+3", 3, 320),
           ("stride321", 0, 321), ("stride322", 0, 322), ("stride323", 0, 323), ("stride324", 0, 324)]


@on_gpu
def test_device_input_layouts_with_three_levels():
    import torch
    import psl_slam_amd as P
    import oracle_lib
    frame = sf.stream(1, W, H, "desk", seed=31)[0]
    orc = oracle_lib.OracleORB(**DEV_CFG)
    ref = orc(frame)
    dev = torch.device("cuda", 0)
    first = None
    for name, base, stride in LAYOUTS:
        host = sf.random_gray(base + stride * H + 4096, 1, 77, "noise").reshape(-1)
        np.lib.stride_tricks.as_strided(host[base:], (H, W), (stride, 1))[:] = frame
        buf = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize(dev)
        assert buf.data_ptr() % 256 == 0
        gpu = P.ORBextractor(max_batch=1, **DEV_CFG)
        gpu.extract_batch_device(buf.data_ptr() + base, 1, W, H, stride, stride * H)
        got = gpu.fetch(0, W, H)
        _assert_same_stages(gpu, orc, got, ref, DEV_CFG["nlevels"], name)
        first = first or got
        assert got[0].tobytes() == first[0].tobytes() and got[1].tobytes() == first[1].tobytes(), name
        del gpu, buf
    assert len(first[0]) > 300


# ---- frame counts --------------------------------------------------------------------------------------------------------------
@on_gpu
def test_one_frame_and_nine_frames_per_launch_give_identical_bytes():
    """9 frames: the XCD-aware grid (8, items, 2) with a ragged last group of 1 frame and 7 idle slots; 1 frame: the plain grid."""
    cfg = dict(nfeatures=500, scaleFactor=1.2, nlevels=4, iniThFAST=20, minThFAST=7)
    frames = sf.stream(9, W, H, "desk", seed=13)
    many, orc = _pair(max_batch=9, **cfg)
    one, _ = _pair(max_batch=1, **cfg)
    res = many.extract_batch(frames)
    for f in range(9):
        k, d = one(frames[f])
        assert len(k) > 100
        assert res[f][0].tobytes() == k.tobytes() and res[f][1].tobytes() == d.tobytes(), f"frame {f}"
        if f in (0, 8):
            _assert_same_stages(many, orc, res[f], orc(frames[f]), 4, f"frame {f} of 9", frame=f)
