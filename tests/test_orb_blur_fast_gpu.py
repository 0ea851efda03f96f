"""k_blur7 and k_fast_cells4 (psl-slam_amd/csrc/orb_kernels.h) at the inputs where their addressing, staging, reductions and stores take
another path, bit-exact against the oracle, stage by stage as tests/test_orb_gpu.py does it: level images, FAST candidates, octree
keypoints, blurred levels, keypoints and descriptors.  Every case takes its claim from the geometry restatement of tests/orb_cases.py
(the tests without the gpu mark), so that a case which no longer reaches its edge fails here and not silently.

  k_blur7         a 64 x 64 tile stages by dwords when x0 >= 4 and x0 + 68 <= w and the rows are 4-byte aligned: level widths on both
                  sides of the first (131 / 132 / 133) and the second (195 / 196 / 197) such tile column; tile rows that reflect at the
                  top, at the bottom, at both (height 63) and nowhere (the stepping loads without psl_reflect101); a tile with all 70
                  rows whose last rows reflect (height 129: unclamped column reads over reflected staging); last tile rows of 1, 3, 4
                  and 5 output rows (a last group of four rows that is partly valid, and the clamped column reads); the byte path of
                  unaligned device input; 1 and 9 frames per launch
  k_fast_cells4   cells whose scanned width leaves each rest mod 4; cells clipped by maxBorderX / maxBorderY; one, two and three passes of
                  the quick test; a cell with no listed pixel; a cell where only minTh finds something; survivors in the first and last
                  row and column of a cell and in both words of a row mask; the densest cell (thresholds 255 / 0 on noise); the byte
                  tile loads of unaligned device input

Two cases cannot exist and are restated as what prevents them: a level under 7 rows (prepare() rejects a level that holds no 30-px FAST
cell: the lowest level has 62 rows), and a cell with more survivors than cellcap (cv::FAST's strict NMS keeps at most one pixel of
every 2 x 2 block, and cellcap is ceil(wCell / 2) * ceil(hCell / 2) of the largest cell).
"""
import numpy as np
import pytest

import orb_cases as oc
import synth_frames as sf
from test_orb_gpu import _assert_same_stages

on_gpu = pytest.mark.gpu      # the tests without it restate geometry and need no GPU

BLUR_TH = 64                  # PSL_BLUR_TH: a workgroup of k_blur7 makes 64 x 64 pixels from 70 staged rows


def _pair(max_batch=1, **cfg):
    import psl_slam_amd as P
    import oracle_lib
    return P.ORBextractor(max_batch=max_batch, **cfg), oracle_lib.OracleORB(**cfg)


def _run(case):
    gpu, orc = _pair(**oc.case_config(case))
    img = oc.case_image(case)
    got, ref = gpu(img), orc(img)
    _assert_same_stages(gpu, orc, got, ref, case["nlevels"], case["name"])
    return gpu, orc, got


# ---- k_blur7: the tiles of a level ---------------------------------------------------------------------------------------------
def blur_tiles(L, aligned=True):
    """The 64 x 64 tiles of k_blur7 on a level: dword (staged by dwords), orows (output rows), top / bottom (a staged row reflects
    there) and full (all 70 rows: the column pass reads its ten row sums unclamped)."""
    out = []
    for y0 in range(0, L["h"], BLUR_TH):
        for x0 in range(0, L["w"], 64):
            orows = min(BLUR_TH, L["h"] - y0)
            out.append(dict(x0=x0, y0=y0, orows=orows, full=orows == BLUR_TH, top=y0 < 3, bottom=y0 + orows + 3 > L["h"],
                            dword=aligned and x0 >= 4 and x0 + 68 <= L["w"]))
    return out


BLUR_WIDTHS = (131, 132, 133, 195, 196, 197)
BLUR_HEIGHTS = (63, 129, 131, 132, 133)
BLUR_CASES = [oc._case(f"blur_{w}x{h}", w, h, 1.2, 1, 100, image="noise") for w in BLUR_WIDTHS for h in BLUR_HEIGHTS]
BLUR_LEVELS = oc._case("blur_3_levels", 236, 160, 1.2, 3, 100, image="noise")


def test_blur_cases_reach_their_tiles():
    """No GPU.  Which tile columns stage by dwords, which tile rows reflect, and how many rows the last tile row has."""
    cols = {}
    for c in BLUR_CASES:
        g = oc.case_geometry(c)
        assert g["error"] is None, c["name"]
        T = blur_tiles(g["levels"][0])
        cols[c["w"]] = sorted({t["x0"] // 64 for t in T if t["dword"]})
        last = [t for t in T if t["y0"] + t["orows"] == c["h"]]
        if c["h"] == 63:       # one tile row that reflects at the top and at the bottom
            assert all(t["top"] and t["bottom"] and not t["full"] for t in T)
        else:                  # 64 k + 1, 3, 4, 5: the last tile row has that many rows
            assert {t["orows"] for t in last} == {c["h"] - 128} and c["h"] - 128 in (1, 3, 4, 5)
            mid = [t for t in T if t["y0"] == 64]
            assert all(t["full"] and not t["top"] for t in mid)
            # 129: the middle tile has all 70 rows and its last two reflect; 131 and up: no row of it reflects
            assert all(t["bottom"] == (c["h"] == 129) for t in mid)
    assert cols == {131: [], 132: [1], 133: [1], 195: [1], 196: [1, 2], 197: [1, 2]}
    # tiles that stage by dwords and reflect nowhere, at the top only, at the bottom only, and at both ends
    kinds = {(t["top"], t["bottom"]) for c in BLUR_CASES for t in blur_tiles(oc.case_geometry(c)["levels"][0]) if t["dword"]}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    lv = oc.case_geometry(BLUR_LEVELS)["levels"]
    assert [(L["w"], L["h"]) for L in lv] == [(236, 160), (197, 133), (164, 111)]
    assert any(t["dword"] and not t["top"] and not t["bottom"] for t in blur_tiles(lv[1]))
    assert {t["orows"] for t in blur_tiles(lv[2])} == {64, 47}     # 47 rows: a last group of four with three valid rows


def test_no_level_has_fewer_than_seven_rows():
    """No GPU.  A level of under 7 rows (fewer rows than the kernel has taps) cannot reach k_blur7: a level must hold a 30-px FAST
    cell inside its 16-px borders, so 62 rows are the least; 61 and everything below, 6 included, are rejected before any launch."""
    assert oc.geometry(132, 62, 1.2, 1, 100)["error"] is None
    for h in (61, 7, 6, 1):
        assert oc.geometry(132, h, 1.2, 1, 100)["error"] is not None
    # and as a higher level of an accepted level 0: 74 / 1.2 = 62 rows pass, 73 / 1.2 = 61 do not
    assert oc.geometry(132, 74, 1.2, 2, 100)["error"] is None and oc.geometry(132, 73, 1.2, 2, 100)["error"] is not None


@on_gpu
@pytest.mark.parametrize("w", BLUR_WIDTHS)
def test_blur_widths_and_heights_equal_the_oracle(w):
    for c in BLUR_CASES:
        if c["w"] == w:
            _run(c)


@on_gpu
def test_blur_on_three_levels_equals_the_oracle():
    _run(BLUR_LEVELS)


# ---- device input layouts and frame counts -------------------------------------------------------------------------------------
W, H = 197, 133
DEV_CFG = dict(nfeatures=200, scaleFactor=1.2, nlevels=2, iniThFAST=20, minThFAST=7)
# (name, base offset, stride): the single-frame layouts of tests/test_orb_edges_gpu.py at this width
LAYOUTS = [("aligned", 0, 200), ("base+1", 1, 200), ("base+2", 2, 200), ("base+3", 3, 200),
           ("stride197", 0, 197), ("stride198", 0, 198), ("stride199", 0, 199), ("stride204", 0, 204)]


def test_device_layouts_take_both_paths():
    """No GPU.  Level 0 of the aligned layouts has tiles that stage by dwords and FAST cells that load aligned dwords; the others have
    none (the kernels ask for (frame pointer | stride) & 3 == 0)."""
    L = oc.geometry(W, H, 1.2, 2, 200)["levels"][0]
    aligned = {name: (base | stride) & 3 == 0 for name, base, stride in LAYOUTS}
    assert [n for n, a in aligned.items() if a] == ["aligned", "stride204"]
    assert sum(t["dword"] for t in blur_tiles(L, True)) == 6 and sum(t["dword"] for t in blur_tiles(L, False)) == 0


@on_gpu
def test_device_input_layouts_equal_the_oracle():
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
    assert len(first[0]) > 50


@on_gpu
def test_one_frame_and_nine_frames_per_launch_give_identical_bytes():
    """9 frames: the XCD-aware grid (8, items, 2) with a ragged last group; 1 frame: the plain grid.  Blurred levels, candidates and
    results of every frame are those of the same frame extracted alone."""
    frames = sf.stream(9, W, H, "desk", seed=13)
    many, orc = _pair(max_batch=9, **DEV_CFG)
    one, _ = _pair(max_batch=1, **DEV_CFG)
    res = many.extract_batch(frames)
    for f in range(9):
        k, d = one(frames[f])
        assert len(k) > 50
        assert res[f][0].tobytes() == k.tobytes() and res[f][1].tobytes() == d.tobytes(), f"frame {f}"
        for l in range(DEV_CFG["nlevels"]):
            np.testing.assert_array_equal(many.debug_level_image(f, l, blurred=True), one.debug_level_image(0, l, blurred=True), err_msg=f"blur, frame {f}, level {l}")
            np.testing.assert_array_equal(many.debug_candidates(f, l), one.debug_candidates(0, l), err_msg=f"FAST, frame {f}, level {l}")
        if f in (0, 8):
            _assert_same_stages(many, orc, res[f], orc(frames[f]), DEV_CFG["nlevels"], f"frame {f} of 9", frame=f)


# ---- k_fast_cells4: cell shapes ------------------------------------------------------------------------------------------------
FAST_WIDTHS = [c for c in oc.WIDTH_SWEEP if 92 <= c["w"] <= 103]                           # 2 and 3 cell columns at h = 92
FAST_BIG = next(c for c in oc.REGIMES if c["name"] == "one_big_cell")                        # 91 x 91: one cell of 53 x 53 scanned pixels
FAST_DENSE = oc._case("dense_cell", 91, 91, 1.2, 1, 100, 255, 0, image="noise")              # every pixel is listed, as many survivors as there can be


def test_fast_cases_reach_their_cells():
    """No GPU.  Rests mod 4 of the scanned width, clipped cells, one pass and several passes of the quick test."""
    rests, clipped_x, clipped_y, passes = set(), 0, 0, set()
    for c in FAST_WIDTHS + [FAST_BIG]:
        L = oc.case_geometry(c)["levels"][0]
        cells = oc.fast_cells(L)
        assert all(k is not None for k in cells)
        rests |= {k["iw"] % 4 for k in cells}
        passes |= {k["npass"] for k in cells}
        clipped_x += sum(k["tw"] < L["wCell"] + 6 for k in cells)      # the tile stops at maxBorderX
        clipped_y += sum(k["th"] < L["hCell"] + 6 for k in cells)      # ... at maxBorderY
    assert rests == {0, 1, 2, 3} and passes == {1, 2, 3} and clipped_x >= len(FAST_WIDTHS) and clipped_y >= len(FAST_WIDTHS)
    big = oc.fast_cells(oc.case_geometry(FAST_BIG)["levels"][0])[0]
    assert (big["iw"], big["ih"]) == (53, 53)                          # more than 32 columns: both words of a row mask


def test_survivors_never_exceed_cellcap():
    """No GPU.  cv::FAST keeps a pixel only if it scores strictly more than its 8 neighbours, so a 2 x 2 block holds at most one
    survivor and a cell at most ceil(iw / 2) * ceil(ih / 2); iw <= wCell and ih <= hCell, and cellcap is that product for the
    largest cell of any level.  `pos < cellcap` in the output pass therefore never drops a survivor, on any input."""
    for c in FAST_WIDTHS + [FAST_BIG, BLUR_LEVELS] + BLUR_CASES:
        lv = oc.case_geometry(c)["levels"]
        cellcap = max(((L["wCell"] + 1) // 2) * ((L["hCell"] + 1) // 2) for L in lv)
        for L in lv:
            for k in oc.fast_cells(L):
                if k is not None and k["iw"] > 0 and k["ih"] > 0:
                    assert ((k["iw"] + 1) // 2) * ((k["ih"] + 1) // 2) <= cellcap


@on_gpu
def test_fast_cell_widths_equal_the_oracle():
    for c in FAST_WIDTHS:
        _run(c)


@on_gpu
def test_the_densest_cell_equals_the_oracle():
    """Thresholds 255 / 0 on noise: no pixel reaches 255, so the cell falls back to minTh = 0, where every pixel passes the quick test
    (three passes, a list of 2809 pixels: eleven trips of the list loops) and every strict local maximum of the score survives."""
    gpu, orc, _ = _run(FAST_DENSE)
    n = len(orc.candidates(0))
    cellcap = 30 * 30      # ceil(59 / 2)^2
    assert 100 <= n <= cellcap, n
    _run(FAST_BIG)


# ---- k_fast_cells4: dot images with written-down answers -----------------------------------------------------------------------
def small_dots():
    """130 x 130: 3 x 3 cells of 33 x 33 (the last column and row clipped to 26 scanned pixels).  Border-relative (X, Y, contrast)."""
    return [
        # cell (0, 0), scanned X, Y in 3 .. 35: nothing - no pixel passes the quick test
        (50, 20, 8),                                   # cell (1, 0): alone, S = 7: nothing at iniTh = 20, found at minTh = 7
        (69, 3, 60), (94, 3, -60), (80, 20, 8),        # cell (2, 0), clipped: first row, first and last column; the 8 vanishes at 20
        (3, 36, 40), (35, 68, -40),                    # cell (0, 1): first row and column, last row and column
        (50, 50, 40), (51, 50, 40),                    # cell (1, 1): an equal pair - listed and scored, no survivor
        (94, 94, 30), (69, 94, -30), (94, 69, 30),     # cell (2, 2), clipped both ways: its last row and last column
    ]


def big_cell_dots():
    """91 x 91: one cell, scanned X, Y in 3 .. 55 (53 columns: x = X - 3 in words 0 and 1 of a row mask)."""
    return [(3, 3, 60), (55, 3, -60), (3, 55, -60), (55, 55, 60),      # the four corners: first / last row and column
            (34, 10, 50), (35, 20, 50),                                  # x = 31 and x = 32: the last bit of word 0, the first of word 1
            (20, 30, 40), (45, 30, -40), (50, 30, 40),                   # one row with survivors in both words
            (30, 40, 8)]                                                 # vanishes at iniTh


def test_dot_images_hold_the_named_cells():
    """No GPU.  The expected candidates (tests/orb_cases.py restates the loop of the reference) show each named cell."""
    dots = small_dots()
    L = oc.geometry(130, 130, 1.2, 1, 300)["levels"][0]
    assert (L["nCols"], L["nRows"], L["wCell"], L["hCell"], L["W"], L["H"]) == (3, 3, 33, 33, 98, 98)
    exp = {tuple(r) for r in oc.expected_candidates(dots, 20, 7, 130, 130).tolist()}
    assert exp == {(50, 20, 7), (69, 3, 59), (94, 3, 59), (3, 36, 39), (35, 68, 39), (94, 94, 29), (69, 94, 29), (94, 69, 29)}
    exp = oc.expected_candidates(big_cell_dots(), 20, 7, 91, 91)
    assert len(exp) == 9 and {31, 32} <= {int(x) - 3 for x in exp[:, 0]} and exp[:, 2].min() >= 20
    assert exp[:, 0].min() == 3 and exp[:, 0].max() == 55 and exp[:, 1].min() == 3 and exp[:, 1].max() == 55


def _dots(dots, w, h, what):
    gpu, orc = _pair(nfeatures=300, scaleFactor=1.2, nlevels=1, iniThFAST=20, minThFAST=7)
    img = oc.dot_image(dots, w=w, h=h)
    got, ref = gpu(img), orc(img)
    expected = oc.expected_candidates(dots, 20, 7, w, h)
    gc = gpu.debug_candidates(0, 0)
    assert gc.shape == expected.shape, f"{what}: {len(gc)} candidates, {len(expected)} written down"
    np.testing.assert_array_equal(gc, expected, err_msg=f"{what}: written-down candidates")
    np.testing.assert_array_equal(gc, orc.candidates(0), err_msg=f"{what}: oracle candidates")
    _assert_same_stages(gpu, orc, got, ref, 1, what)


@on_gpu
def test_dots_in_empty_fallback_and_clipped_cells():
    _dots(small_dots(), 130, 130, "small dots")


@on_gpu
def test_dots_in_both_words_of_a_row_mask():
    _dots(big_cell_dots(), 91, 91, "big cell dots")
