"""Hand-built inputs of the ORB extractor (tests/test_orb_cases_cpu.py pins them to the oracle, tests/test_orb_edges_gpu.py runs
the HIP kernels on them).  numpy only: no GPU, no oracle.

1. Dot images with written-down FAST answers.  On a flat background a lone pixel of contrast c has cornerScore |c| - 1 (all 16
   ring pixels are background), and no background pixel is a corner (at most a few ring pixels differ, never 9 in a row).  Two
   adjacent pixels do not lie on each other's radius-3 ring, so each keeps its lone score and only cv::FAST's strict NMS decides.
   `expected_candidates` restates the loop of src/ORBextractor.cc:789-829 on such a sparse score map.
2. `geometry`: prepare() of psl-slam_amd/csrc/pslfe_orb.hip in a few lines, plus the source rows / bytes a 64 x 32 block of
   k_pyr_resize_tiled needs, so that every case of `REGIMES` asserts the kernel path it was built for.
3. `REGIMES`: the smallest inputs found that reach each fallback path of psl-slam_amd/csrc/orb_kernels.h.

Coordinates (X, Y) are relative to the 16-px border (minBorderX = EDGE_THRESHOLD - 3), as the candidate lists of both the oracle and
pslfe_orb_debug_candidates are."""
import math

import numpy as np

F32 = np.float32
EDGE = 16
PYR_TD, PYR_TR, PYR_BH = 36, 48, 32    # k_pyr_resize_tiled: tile pitch in dwords, tile rows, block height


# ------------------------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------------------------
def _cv_round(v):
    return int(np.rint(np.float64(v)))


def _linear_ofs(ssize, dsize, clamp):
    """xofs / yofs of cv::resize INTER_LINEAR (the coefficient half of the table is restated in resize_tables)."""
    scale = 1.0 / (float(dsize) / ssize)
    f = ((np.arange(dsize) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    if clamp:
        s = np.clip(s, 0, ssize - 1)
    return s


def resize_tables(ssize, dsize):
    """(ofs, coef0, coef1) of cv::resize INTER_LINEAR 8UC1 (OpenCV 3.2, 11-bit fixed point), unclamped."""
    scale = 1.0 / (float(dsize) / ssize)
    d = np.arange(dsize)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    a1 = np.rint(f * np.float32(2048)).astype(np.int64)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int64)
    return s, a0, a1


def resize_numpy(src, dw, dh):
    """cv::resize(src, (dw, dh), INTER_LINEAR) of a u8 image in numpy: taps past the last column / row repeat it."""
    sh, sw = src.shape
    sx, a0, a1 = resize_tables(sw, dw)
    sy, b0, b1 = resize_tables(sh, dh)
    S = src.astype(np.int64)
    x0, x1 = np.clip(sx, 0, sw - 1), np.clip(sx + 1, 0, sw - 1)
    y0, y1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)
    hor = S[:, x0] * a0 + S[:, x1] * a1
    out = (((b0[:, None] * (hor[y0] >> 4)) >> 16) + ((b1[:, None] * (hor[y1] >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def _pyr_blocks(sw, sh, spitch, dw, dh, src_aligned):
    """Per 64 x 32 block of k_pyr_resize_tiled: source rows, source bytes (dwords * 4) and whether it is staged through LDS; per
    4-pixel thread: whether its 8 taps fit the three-dword read (`fits`)."""
    dpitch = (dw + 15) // 16 * 16
    xofs, yofs = _linear_ofs(sw, dw, True), _linear_ofs(sh, dh, False)
    blocks = []
    for y0 in range(0, dh, PYR_BH):
        ye = min(y0 + PYR_BH - 1, dh - 1)
        rfirst = min(max(int(yofs[y0]), 0), sh - 1)
        rlast = min(max(int(yofs[ye]) + 1, 0), sh - 1)
        for x0 in range(0, dpitch, 64):
            xe = min(x0 + 63, dw - 1)
            cfirst, clast = int(xofs[min(x0, dw - 1)]), min(int(xofs[xe]) + 1, sw - 1)
            cbase = cfirst & ~3
            ndw, nrows = ((clast - cbase) >> 2) + 1, rlast - rfirst + 1
            staged = ndw <= PYR_TD and nrows <= PYR_TR and src_aligned and cbase + ndw * 4 <= spitch
            fit = unfit = maxofs = 0
            for x4 in range(x0, min(x0 + 64, dpitch), 4):
                sx = [int(xofs[min(x4 + j, dw - 1)]) for j in range(4)]
                ofs3 = sx[3] - (sx[0] & ~3)     # byte offset of the last left tap from the dword that holds the first
                maxofs = max(maxofs, ofs3)
                if ofs3 <= 7:
                    fit += 1
                else:
                    unfit += 1
            blocks.append(dict(rows=nrows, bytes=ndw * 4, staged=staged, fit=fit, unfit=unfit, maxofs=maxofs))
    return blocks


def geometry(w, h, scaleFactor, nlevels, nfeatures, src_aligned=True):
    """prepare() restated.  Returns dict(levels=[...], error=None | reason, oct_bs=256 | 512).  A level holds w, h, pitch, nCols,
    nRows, wCell, hCell, W, H (the bordered size), nIni, quota, kp_cap, cells and, from level 1 on, `blocks` (_pyr_blocks)."""
    sf = float(F32(scaleFactor))                                    # the C ABI takes a float, the member is a double
    scale = [F32(1.0)]
    for _ in range(1, nlevels):
        scale.append(F32(float(scale[-1]) * sf))
    factor = F32(1.0 / sf)
    nd = F32(nfeatures) * (F32(1) - factor) / (F32(1) - F32(math.pow(float(factor), float(nlevels))))
    quota, tot = [], 0
    for _ in range(nlevels - 1):
        quota.append(_cv_round(nd))
        tot += quota[-1]
        nd = F32(nd * factor)
    quota.append(max(nfeatures - tot, 0))
    levels, error = [], None
    for l in range(nlevels):
        inv = F32(1.0) / scale[l]
        L = dict(w=_cv_round(F32(w) * inv), h=_cv_round(F32(h) * inv), quota=quota[l])
        L["pitch"] = (L["w"] + 15) // 16 * 16
        L["W"], L["H"] = L["w"] - 2 * EDGE, L["h"] - 2 * EDGE
        L["nCols"], L["nRows"] = int(F32(L["W"]) / F32(30)), int(F32(L["H"]) / F32(30))
        if L["nCols"] < 1 or L["nRows"] < 1:
            error = f"level {l} ({L['w']}x{L['h']}) is smaller than one FAST cell"
            levels.append(L)
            break
        L["wCell"] = int(math.ceil(F32(L["W"]) / F32(L["nCols"])))
        L["hCell"] = int(math.ceil(F32(L["H"]) / F32(L["nRows"])))
        r = F32(L["W"]) / F32(L["H"])
        L["nIni"] = int(math.floor(float(r) + 0.5))                 # roundf of a positive value
        if L["nIni"] < 1:
            error = f"level {l} is more than twice as tall as wide"
            levels.append(L)
            break
        L["kp_cap"] = max(L["quota"] + 3, 4 * L["nIni"])
        L["cells"] = L["nCols"] * L["nRows"]
        if l > 0:
            P = levels[l - 1]
            L["blocks"] = _pyr_blocks(P["w"], P["h"], P["pitch"] if l > 1 else w, L["w"], L["h"], src_aligned or l > 1)
        levels.append(L)
    oct_bs = None
    if error is None:
        cap = max(L["kp_cap"] for L in levels)
        if cap > 512:
            error = f"{cap} features on one level exceed the 512-node octree workgroup"
        else:
            oct_bs = 256 if cap <= 256 else 512
    return dict(levels=levels, error=error, oct_bs=oct_bs)


def fast_cells(L):
    """The FAST cells of one level as k_fast_cells4 (and src/ORBextractor.cc:789-806) lays them out: per cell None when the loop
    skips it (iniY >= maxBorderY - 3, iniX >= maxBorderX - 6), else dict(tw, th, iw, ih, npass): tile size, scanned interior and
    passes of the quick test (256 threads x 4 pixels).  A tile under 7 px that the loop does not skip (th of 4..6: the row test is the
    weaker one) is handed to cv::FAST, which finds nothing: iw or ih <= 0 and npass = 0."""
    out = []
    maxBX, maxBY = L["w"] - EDGE, L["h"] - EDGE
    for i in range(L["nRows"]):
        for j in range(L["nCols"]):
            iniY, iniX = EDGE + i * L["hCell"], EDGE + j * L["wCell"]
            if iniY >= maxBY - 3 or iniX >= maxBX - 6:
                out.append(None)
                continue
            tw, th = min(iniX + L["wCell"] + 6, maxBX) - iniX, min(iniY + L["hCell"] + 6, maxBY) - iniY
            iw, ih = tw - 6, th - 6
            out.append(dict(tw=tw, th=th, iw=iw, ih=ih, npass=(((iw + 3) >> 2) * ih + 255) >> 8 if iw > 0 and ih > 0 else 0))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# dot images
# ------------------------------------------------------------------------------------------------------------------------------
DOT_W, DOT_H = 320, 240
CONTRASTS = (6, 7, 8, 19, 20, 21, 60, 155)       # |c|; the dark 155 does not exist on background 100 and is built as -100


def _spaced(dots, X, Y):
    """True when (X, Y) can hold a new lone dot: no existing dot within Chebyshev distance 3 (nothing adjacent, nothing on the ring)."""
    return all(max(abs(X - x), abs(Y - y)) >= 4 for x, y, _ in dots)


def dot_image(dots, bg=100, w=DOT_W, h=DOT_H):
    """Flat image with single pixels of contrast c at border-relative (X, Y).  Two dots are either adjacent (Chebyshev distance 1) or
    at least 4 apart, so no dot lies on another dot's ring and every dot scores |c| - 1."""
    img = np.full((h, w), bg, np.uint8)
    for a, (x, y, c) in enumerate(dots):
        assert 0 <= bg + c <= 255 and c != 0
        assert 0 <= x + EDGE < w and 0 <= y + EDGE < h
        for x2, y2, _ in dots[:a]:
            d = max(abs(x - x2), abs(y - y2))
            assert d == 1 or d >= 4, ((x, y), (x2, y2))
        img[y + EDGE, x + EDGE] = bg + c
    return img


def expected_candidates(dots, iniTh, minTh, w=DOT_W, h=DOT_H):
    """The FAST candidates of level 0 of dot_image(dots), as (n, 3) int32 rows X, Y, S in the reference's order: cells row-major,
    raster order inside a cell; a cell gives its NMS survivors at iniTh if there are any, else those at minTh.  Scores outside the
    scanned interior of a cell count as 0 in its NMS (cv::FAST runs on the cell's sub-image)."""
    L = geometry(w, h, 1.2, 1, 1)["levels"][0]
    score = {(x, y): min(abs(c) - 1, 255) for x, y, c in dots}
    out = []
    for i in range(L["nRows"]):
        for j in range(L["nCols"]):
            iniX, iniY = j * L["wCell"], i * L["hCell"]
            maxX, maxY = min(iniX + L["wCell"] + 6, L["W"]), min(iniY + L["hCell"] + 6, L["H"])
            if iniY >= L["H"] - 3 or iniX >= L["W"] - 6 or maxX - iniX < 7 or maxY - iniY < 7:
                continue
            inside = sorted(((y, x) for (x, y) in score if iniX + 3 <= x < maxX - 3 and iniY + 3 <= y < maxY - 3))
            for t in (min(max(iniTh, 0), 255), min(max(minTh, 0), 255)):
                corner = {(x, y): score[(x, y)] for y, x in inside if score[(x, y)] >= t}
                keep = [(x, y, s) for (y, x) in inside if (s := corner.get((x, y), 0)) > 0 and
                        all(s > corner.get((x + dx, y + dy), 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if dx or dy)]
                if keep:
                    break
            out += keep
    return np.array(out, np.int32).reshape(-1, 3)


def dot_lattice():
    """320x240 (9 x 6 cells of 32 x 35), background 100: every cell holds a lattice of lone dots whose contrasts cycle through
    +-CONTRASTS.  Cells of parity (i + j) even put dots on their first and last interior column and row (the seams); odd cells stay 4
    px inside, so that no two dots of neighbouring cells touch.  Cell kinds alternate in 2-row bands: strong cells hold dots of every
    contrast (their dots below iniTh must vanish), weak cells only |c| <= 20 (all their dots with S >= minTh must appear).  Dots in the
    3-px frame that FAST never scans, and in the border outside it, carry contrast 60 and must never appear."""
    L = geometry(DOT_W, DOT_H, 1.2, 1, 1)["levels"][0]
    strong = [21, -60, 6, -7, 8, -19, 20, 155, -21, 60, -6, 7, -8, 19, -20, -100]
    weak = [6, -7, 8, -19, 20, -6, 7, -8, 19, -20]
    dots, ks, kw = [], 0, 0
    for i in range(L["nRows"]):
        for j in range(L["nCols"]):
            x0, y0 = j * L["wCell"] + 3, i * L["hCell"] + 3
            nx, ny = min(x0 + L["wCell"], L["W"] - 3) - x0, min(y0 + L["hCell"], L["H"] - 3) - y0
            if (i + j) % 2 == 0:
                cols = [c for c in (0, 9, 18) if c <= nx - 5] + [nx - 1]
                rows = [r for r in (0, 9, 18, 27) if r <= ny - 5] + [ny - 1]
            else:
                cols = [c for c in (4, 13, 22, 27) if c <= nx - 5]
                rows = [r for r in (4, 13, 22, 31) if r <= ny - 5]
            for r in rows:
                for c in cols:
                    if (i + j) % 2 == 0 and r == ny - 1 and c in (0, nx - 1):
                        continue        # would touch the first dot of the diagonal neighbour cell
                    if ((i // 2) + j) % 2 == 0:
                        v, ks = strong[ks % len(strong)], ks + 1
                    else:
                        v, kw = weak[kw % len(weak)], kw + 1
                    dots.append((x0 + c, y0 + r, v))
    for t in range(6, L["W"] - 6, 7):       # the unscanned 3-px frame and the border outside it, all four sides
        for X, Y in ((t, t % 3), (t, L["H"] - 1 - t % 3), (t, -5), (t, L["H"] + 4)):
            if _spaced(dots, X, Y):
                dots.append((X, Y, 60 if t % 2 else -60))
    for t in range(6, L["H"] - 6, 7):
        for X, Y in ((t % 3, t), (L["W"] - 1 - t % 3, t), (-5, t), (L["W"] + 4, t)):
            if _spaced(dots, X, Y):
                dots.append((X, Y, 60 if t % 2 else -60))
    return dot_image(dots), dots


def ceiling_dots():
    """|c| = 255, S = 254 (the u8 score ceiling is 255): a bright dot on background 0 and a dark dot on background 255, each on a seam
    column of cell (1, 2), with a weak dot next door that must vanish and one in another cell that must stay."""
    return [(2 * 32 + 3, 1 * 35 + 3, 255), (2 * 32 + 20, 1 * 35 + 20, 19), (5 * 32 + 10, 3 * 35 + 10, 8)]


def pair_dots():
    """Adjacent pairs for cv::FAST's strict NMS, one group per cell (cells are 32 x 35).  Returns (dots, expected): `expected` is the
    hand-written candidate list for iniTh / minTh = 20 / 7 in the reference's order."""
    def cell(j, i, dx=10, dy=10):
        return j * 32 + 3 + dx, i * 35 + 3 + dy
    dots, exp = [], []
    # cell row 0: equal pairs vanish - horizontal, diagonal, anti-diagonal, vertical; +30 / -30 both score 29
    for j, (ox, oy, a, b) in enumerate([(1, 0, 40, 40), (1, 1, 40, 40), (-1, 1, 40, 40), (0, 1, -40, -40), (1, 0, 30, -30), (1, 1, -30, 30)]):
        x, y = cell(j, 0)
        dots += [(x, y, a), (x + ox, y + oy, b)]
    # cell row 1: (c, c + 1) keeps the larger - horizontal, vertical, diagonal, anti-diagonal, and in the dark polarity
    for j, (ox, oy, a, b) in enumerate([(1, 0, 40, 41), (0, 1, 41, 40), (1, 1, 40, 41), (-1, 1, 41, 40), (1, 0, -40, -41), (0, 1, -41, -40),
                                        (1, 0, 41, -40)]):
        x, y = cell(j, 1)
        dots += [(x, y, a), (x + ox, y + oy, b)]
        big = (x, y, a) if abs(a) > abs(b) else (x + ox, y + oy, b)
        exp.append((big[0], big[1], abs(big[2]) - 1))
    # cell row 2: the two thresholds.  (8, 30): only 30 is a corner at 20.  (8, 9) alone in a cell: the cell falls back to 7 and keeps
    # S = 8.  (7, 8): S = 6 is no corner at 7, S = 7 stays.  (20, 21): S = 19 / 20, the cell is not empty at 20 and keeps S = 20.
    # (20, 20): S = 19 twice, equal at 7.  (21, 20) + a lone 8 elsewhere in the cell: the 8 vanishes.
    x, y = cell(0, 2); dots += [(x, y, 8), (x + 1, y, 30)]; exp.append((x + 1, y, 29))
    x, y = cell(1, 2); dots += [(x, y, 8), (x + 1, y + 1, 9)]; exp.append((x + 1, y + 1, 8))
    x, y = cell(2, 2); dots += [(x, y, -7), (x, y + 1, -8)]; exp.append((x, y + 1, 7))
    x, y = cell(3, 2); dots += [(x, y, 20), (x + 1, y, 21)]; exp.append((x + 1, y, 20))
    x, y = cell(4, 2); dots += [(x, y, 20), (x + 1, y, 20)]
    x, y = cell(5, 2); dots += [(x, y, 21), (x, y + 1, -20), (x + 12, y + 12, 8)]; exp.append((x, y, 20))
    # cell row 3: pairs across a seam.  The scanned interior of cell column j ends at X = 32 (j + 1) + 2 and that of cell row i at
    # Y = 35 (i + 1) + 2; the neighbour across the seam scores 0 in this cell's NMS, so both pixels of an equal pair survive, each in
    # its own cell.  Vertical seam between columns 0 | 1 (equal) and 2 | 3 (c, c + 1); horizontal seam between rows 3 | 4 (equal,
    # then diagonal); the four-cell corner between columns 6 | 7 and rows 3 | 4.
    y = 3 * 35 + 3 + 10
    dots += [(34, y, 40), (35, y, 40), (98, y, -40), (99, y, -41)]
    exp += [(34, y, 39), (35, y, 39), (98, y, 39), (99, y, 40)]
    dots += [(4 * 32 + 13, 142, 40), (4 * 32 + 13, 143, 40), (5 * 32 + 13, 142, 50), (5 * 32 + 14, 143, 50)]
    dots += [(7 * 32 + 2, 142, 33), (7 * 32 + 3, 143, 33)]
    exp += [(4 * 32 + 13, 142, 39), (5 * 32 + 13, 142, 49), (7 * 32 + 2, 142, 32)]                   # cell row 3 ends at Y = 142
    exp += [(4 * 32 + 13, 143, 39), (5 * 32 + 14, 143, 49), (7 * 32 + 3, 143, 32)]                   # cell row 4 starts at Y = 143
    return dots, np.array(exp, np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# the regime table
# ------------------------------------------------------------------------------------------------------------------------------
def _case(name, w, h, sf, nl, nf, ini=20, mn=7, image="desk", accept=True):
    return dict(name=name, w=w, h=h, scaleFactor=sf, nlevels=nl, nfeatures=nf, iniThFAST=ini, minThFAST=mn, image=image, accept=accept)


REGIMES = [
    _case("scale_1.1", 320, 240, 1.1, 4, 300),
    _case("scale_1.3", 320, 240, 1.3, 4, 300),
    _case("scale_1.35", 320, 240, 1.35, 4, 300),
    _case("scale_1.5", 320, 240, 1.5, 3, 300),
    _case("scale_2.0", 320, 240, 2.0, 2, 300),
    _case("scale_2.0_level_too_small", 320, 240, 2.0, 3, 300, accept=False),
    _case("th_7_7", 320, 240, 1.2, 4, 300, 7, 7),
    _case("th_40_40", 320, 240, 1.2, 4, 300, 40, 40),
    _case("th_7_20", 320, 240, 1.2, 4, 300, 7, 20),
    _case("th_255_0", 320, 240, 1.2, 4, 300, 255, 0, image="noise"),
    _case("one_big_cell", 91, 91, 1.2, 1, 100, image="noise"),
    _case("narrow_tall_cell", 91, 124, 1.2, 1, 100, image="noise"),
    _case("skipped_cell_column", 1233, 92, 1.2, 1, 300, image="noise"),
    _case("nini_bound", 1233, 92, 1.2, 1, 5, image="noise"),
    # The last cell column / row is W - (n - 1) * cell wide.  It gets narrow only when W = 30 n + 1 with n >= 22 (cell 31): these are
    # the smallest sizes with a scanned interior of 3, 2 and 1 px, with a 6-px rest that the loop skips (iniX >= maxBorderX - 6),
    # and, for rows, with a 6-px rest that the loop does not skip (iniY >= maxBorderY - 3 is weaker) but cv::FAST returns empty
    # (the kernel's th < 7), and with a 3-px rest that it skips.
    _case("last_col_iw3", 723, 92, 1.2, 1, 300, image="noise"),
    _case("last_col_iw2", 753, 92, 1.2, 1, 300, image="noise"),
    _case("last_col_iw1", 783, 92, 1.2, 1, 300, image="noise"),
    _case("last_col_rest6", 813, 92, 1.2, 1, 300, image="noise"),
    _case("last_row_ih1", 432, 783, 1.2, 1, 300, image="noise"),
    _case("last_row_th6", 432, 813, 1.2, 1, 300, image="noise"),
    _case("last_row_rest3", 482, 903, 1.2, 1, 300, image="noise"),
    _case("quota_0", 320, 240, 1.2, 8, 1),
    _case("bs_256", 320, 240, 1.2, 1, 253, image="noise"),
    _case("bs_512", 320, 240, 1.2, 1, 254, image="noise"),
    _case("cap_512", 320, 240, 1.2, 1, 509, image="noise"),
    _case("cap_513", 320, 240, 1.2, 1, 510, image="noise", accept=False),
    _case("global_offsets_256", 1030, 1030, 1.2, 1, 200, image="noise"),
    _case("global_offsets_512", 1920, 1080, 1.2, 8, 2000),
]
WIDTH_SWEEP = [_case(f"width_{w}", w, 92, 1.2, 1, 100, image="noise") for w in range(92, 157)]


def case_geometry(c, src_aligned=True):
    return geometry(c["w"], c["h"], c["scaleFactor"], c["nlevels"], c["nfeatures"], src_aligned)


def case_image(c):
    import synth_frames as sf
    if c["image"] == "noise":
        return sf.random_gray(c["w"], c["h"], 11 + c["w"], "noise")
    return sf.Scene(c["w"], c["h"], "desk", seed=c["w"] * 7 + c["h"]).gray(1)


def case_config(c):
    return {k: c[k] for k in ("nfeatures", "scaleFactor", "nlevels", "iniThFAST", "minThFAST")}


def _blocks(g):
    return [b for L in g["levels"][1:] for b in L["blocks"]]


def regime_claims(c):
    """The claim of the table row as a list of (text, bool) computed from the geometry restatement alone."""
    g = case_geometry(c)
    n, lv = c["name"], g["levels"]
    if not c["accept"]:
        claims = [("prepare() rejects it", g["error"] is not None)]
        if n == "scale_2.0_level_too_small":
            claims += [("level 2 is 80x60", (lv[2]["w"], lv[2]["h"]) == (80, 60)), ("its nRows is 0", lv[2]["nRows"] == 0)]
        if n == "cap_513":
            claims += [("kp_cap is 513", lv[0]["kp_cap"] == 513)]
        return claims
    claims = [("prepare() accepts it", g["error"] is None)]
    B = _blocks(g) if c["nlevels"] > 1 else []
    if n == "scale_1.1":
        claims += [("every block is staged", all(b["staged"] for b in B)), ("every thread fits", all(b["unfit"] == 0 for b in B))]
    if n == "scale_1.3":    # 4 pixels span at most 4 source bytes and start at most 3 bytes into a dword: 1.3 is the last factor that always fits
        claims += [("every block is staged", all(b["staged"] for b in B)),
                   ("every thread fits, some with the last tap at byte 7, the last that does", all(b["unfit"] == 0 for b in B) and max(b["maxofs"] for b in B) == 7)]
    if n == "scale_1.35":
        claims += [("every block is staged", all(b["staged"] for b in B)),
                   ("some threads do not fit, some do", any(b["unfit"] for b in B) and any(b["fit"] for b in B))]
    if n == "scale_1.5":
        claims += [("staged and unstaged blocks are mixed", any(b["staged"] for b in B) and any(not b["staged"] for b in B)),
                   ("the unstaged ones need 49 source rows, one more than the tile holds", {b["rows"] for b in B if not b["staged"]} == {PYR_TR + 1}),
                   ("a staged block fills the tile: 48 rows", any(b["staged"] and b["rows"] == PYR_TR for b in B))]
    if n == "scale_2.0":
        full = [b for b in B if b["rows"] > PYR_TR]
        claims += [("full-height blocks need 64 or 65 source rows, more than the tile holds, and are unstaged",
                    len(full) > 0 and not any(b["staged"] for b in full) and {b["rows"] for b in full} <= {64, 65}),
                   ("their width alone would fit the tile", all(b["bytes"] <= 4 * PYR_TD for b in B))]
    if n == "one_big_cell":
        cells = fast_cells(lv[0])
        claims += [("one cell of 59 x 59", (lv[0]["cells"], lv[0]["wCell"], lv[0]["hCell"]) == (1, 59, 59)),
                   # wCell <= 59 and the single cell is clipped to the border, so 53 x 53 scanned pixels = 14 groups x 53 rows is the
                   # largest cell there is: 3 of the 4 passes that the 64 x 64 tile would allow
                   ("the largest scanned interior there is: 53 x 53, 3 passes of the quick test", (cells[0]["iw"], cells[0]["ih"], cells[0]["npass"]) == (53, 53, 3))]
    if n == "narrow_tall_cell":
        claims += [("cells of 59 x 31", (lv[0]["wCell"], lv[0]["hCell"], lv[0]["nCols"], lv[0]["nRows"]) == (59, 31, 1, 3))]
    if n in ("skipped_cell_column", "nini_bound"):
        cells = fast_cells(lv[0])
        claims += [("W = 1201, 40 x 2 cells, nIni = 20", (lv[0]["W"], lv[0]["nCols"], lv[0]["nRows"], lv[0]["nIni"]) == (1201, 40, 2, 20)),
                   ("the 40th cell column is skipped", cells[39] is None and cells[79] is None and all(cells[k] is not None for k in range(39)))]
    if n.startswith("last_col_") or n.startswith("last_row_"):
        cells = fast_cells(lv[0])
        last = cells[lv[0]["nCols"] - 1] if n.startswith("last_col_") else cells[-1]
        want = {"last_col_iw3": ("iw", 3), "last_col_iw2": ("iw", 2), "last_col_iw1": ("iw", 1), "last_row_ih1": ("ih", 1)}
        if n in want:
            claims += [(f"the last cell's scanned interior is {want[n][1]} px", last is not None and last[want[n][0]] == want[n][1])]
        if n in ("last_col_rest6", "last_row_rest3"):
            claims += [("the loop skips the last cell", last is None and sum(k is None for k in cells) == (lv[0]["nRows"] if "col" in n else lv[0]["nCols"]))]
        if n == "last_row_th6":
            claims += [("the loop keeps the last cell row, whose tile is 6 px high", last is not None and last["th"] == 6 and last["npass"] == 0)]
    if n == "nini_bound":
        claims += [("kp_cap = 4 nIni = 80 exceeds quota + 3", lv[0]["kp_cap"] == 80 and lv[0]["quota"] == 5)]
    if n == "quota_0":
        claims += [("quotas are 0 x 7, 1", [L["quota"] for L in lv] == [0] * 7 + [1])]
    if n == "bs_256":
        claims += [("kp_cap 256 selects k_octree<256>", lv[0]["kp_cap"] == 256 and g["oct_bs"] == 256)]
    if n == "bs_512":
        claims += [("kp_cap 257 selects k_octree<512>", lv[0]["kp_cap"] == 257 and g["oct_bs"] == 512)]
    if n == "cap_512":
        claims += [("kp_cap 512 is the last accepted", lv[0]["kp_cap"] == 512 and g["oct_bs"] == 512)]
    if n == "global_offsets_256":
        claims += [("1089 cells > 4 * 256 under k_octree<256>", lv[0]["cells"] == 1089 and g["oct_bs"] == 256)]
    if n == "global_offsets_512":
        claims += [("level 0 has more than 4 * 512 cells under k_octree<512>", lv[0]["cells"] > 2048 and g["oct_bs"] == 512),
                   ("no other level has", all(L["cells"] <= 2048 for L in lv[1:]))]
    return claims


def width_sweep_claims():
    """The 65 widths 92..156 at h = 92 (2, 3 and 4 cell columns), claims about the set as a whole.  No width this small has a
    last column under 7 px or a skipped one (that needs 22 columns and more: the last_col_* rows of REGIMES)."""
    iws, ncols, partial, skipped = set(), set(), 0, 0
    for c in WIDTH_SWEEP:
        L = case_geometry(c)["levels"][0]
        cells = fast_cells(L)
        skipped += sum(k is None for k in cells)
        iws |= {k["iw"] for k in cells if k is not None}
        ncols.add(L["nCols"])
        partial += cells[L["nCols"] - 1]["iw"] < cells[0]["iw"]
    return [("2, 3 and 4 cell columns", ncols == {2, 3, 4}),
            ("every scanned width from 22 to 45 px occurs, so every rest of the last 4-pixel group", iws == set(range(22, 46))),
            ("most widths have a partial last cell", partial > len(WIDTH_SWEEP) // 2),
            ("no cell is skipped", skipped == 0)]
