"""Hand-built inputs of the RGB-D line glue with written-down answers (pure numpy; used by test_glue_cases_cpu.py and
test_glue_edges_gpu.py).  glue_scene.py draws random segments in one room corner; a failure there says "frame 2, key lines3d".
Every case here is built so that ONE rule of Frame::isLineGood / extract3dline_mahdist / convertFansToKeyLines / the plane loop
decides its answer, and it carries that answer.

Camera: fx = fy = 512 with the principal point in the image centre (320, 240 at 640x480; 32, 24 at 64x48; 16, 12 at 32x24), so
1 / fx and every (col - cx) are exact in f32.  On a noise-free fronto-parallel wall at z = 2 the point behind pixel (col, row) is
((col - cx) / 256, (row - cy) / 256, 2) exactly, every sample is an inlier of every pair, the RANSAC stops after its first
iteration (2 rand() values) and the end points are the first and the last valid sample.  Which of the two is the start is
decided by the sign of a Jacobi vector, so the written answer is the unordered pair and the order is held to the oracle only.

`sample_line` restates the sampler of Frame.cc:674-716 (j / numSmp weights, float products, the integer-coordinate branch with its
max(int(p - 1), 0) clamp, the border test); the cases derive their pixel lists and sample counts from it and the CPU test holds it
to the oracle's trace.

A case is a dict: name, kls, fans, depth ([h][w] f32; with depth_stride the first w columns of a padded buffer), depth_stride,
cam, seeds, and the answers: accepted (per line), np (samples that became points, per line), ends (per accepted line the pixels
of its two end points, unordered), ncross, nplanes, and `regime` - what the oracle's trace must show for the case to test what it
claims (per line index: {trace field: value})."""
import functools

import numpy as np

import oracle_lib

F32 = np.float32
WALL = 2.0


def camera(w, h, fx=512.0):
    c = np.zeros((), oracle_lib.CAMERA_DTYPE)
    c["fx"], c["fy"], c["cx"], c["cy"], c["bf"] = fx, fx, w / 2, h / 2, 40.0
    return c


def keylines(segs):
    """segs: rows (sx, sy, ex, ey)"""
    segs = np.asarray(segs, np.float32).reshape(-1, 4)
    k = np.zeros(len(segs), oracle_lib.KEYLINE_DTYPE)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = segs.T
    k["sPointInOctaveX"], k["sPointInOctaveY"], k["ePointInOctaveX"], k["ePointInOctaveY"] = segs.T
    k["lineLength"] = np.hypot(segs[:, 0] - segs[:, 2], segs[:, 1] - segs[:, 3])
    k["class_id"] = np.arange(len(segs))
    return k


def sample_line(seg, w, h):
    """The sampler of Frame.cc:674-716 restated: for j = 0 .. numSmp the tuple (kind, col, row), kind one of "outside" (col = row =
    None), "frac" (col, row = int(pt)), "int" (both coordinates integral: max(int(pt - 1), 0)) and "clamp" (an "int" sample whose
    clamp binds).  None for a line shorter than 1 px (numSmp == 0)."""
    sx, sy, ex, ey = (F32(v) for v in seg)
    dx, dy = F32(sx - ex), F32(sy - ey)
    n = min(int(np.sqrt(float(dx) * float(dx) + float(dy) * float(dy))), 20)
    if n == 0:
        return None
    out = []
    for j in range(n + 1):
        w1, w2 = 1 - j / n, j / n
        ax, ay, bx, by = F32(float(sx) * w1), F32(float(sy) * w1), F32(float(ex) * w2), F32(float(ey) * w2)
        ptx, pty = float(F32(ax + bx)), float(F32(ay + by))
        if ptx < 0 or pty < 0 or ptx >= w or pty >= h:
            out.append(("outside", None, None))
        elif np.floor(ptx) == ptx and np.floor(pty) == pty:
            c, r = int(ptx - 1), int(pty - 1)
            out.append(("clamp" if c < 0 or r < 0 else "int", max(c, 0), max(r, 0)))
        else:
            out.append(("frac", int(ptx), int(pty)))
    return out


def sample_counts(seg, depth, w, h):
    """(tried, outside, int_branch, clamped, holes, np, pixels of the samples that became points) as the trace counts them"""
    s = sample_line(seg, w, h)
    if s is None:
        return (0, 0, 0, 0, 0, 0, [])
    inside = [(c, r) for kind, c, r in s if kind != "outside"]
    pts = [(c, r) for c, r in inside if not depth[r, c] <= 0.01]   # NaN is no hole
    kinds = [k for k, _, _ in s]
    return (len(s), kinds.count("outside"), kinds.count("int") + kinds.count("clamp"), kinds.count("clamp"), len(inside) - len(pts), len(pts),
            pts)


def point3d(col, row, z, cam):
    """the back-projection of isLineGood, exact for this file's cameras and dyadic depths"""
    return np.array([(col - float(cam["cx"])) * z / float(cam["fx"]), (row - float(cam["cy"])) * z / float(cam["fy"]), z])


def wall(w, h, z=WALL):
    return np.full((h, w), z, np.float32)


def _case(name, segs, depth, cam, fans=None, seeds=(1,), depth_stride=None, **answers):
    h, w = depth.shape
    kls = keylines(segs)
    counts = [sample_counts(s, depth, w, h) for s in np.asarray(segs, np.float32).reshape(-1, 4)]
    c = dict(name=name, segs=np.asarray(segs, np.float32).reshape(-1, 4), kls=kls, fans=np.zeros((0, 4), np.float32) if fans is None else
             np.asarray(fans, np.float32).reshape(-1, 4), depth=depth, depth_stride=depth_stride, cam=cam, seeds=tuple(seeds), w=w, h=h,
             counts=counts, np=[k[5] for k in counts], regime={}, ncross=0, nplanes=0, ends="wall")
    c.update(answers)
    assert len(c["accepted"]) == len(kls), name
    return c


def wall_ends(case, i):
    """first and last sample that became a point: the end points of an accepted line on a noise-free wall"""
    px = case["counts"][i][6]
    return px[0], px[-1]


# ---- lengths ------------------------------------------------------------------------------------------------------------------
LENGTHS = (3.5, 4.5, 5.5, 6.5, 7.5, 8.5, 9.5, 20.5, 21.5)


def lengths(z=2.0, reverse=False, w=64, h=48, x0=10.25, lens=LENGTHS):
    """Horizontal lines of growing length from x0 on a wall at z.  3.5 px: 4 samples, np < 5.  4.5 .. 6.5: 5 .. 7 points, all ten
    iterations (20 rand() values each) without ever passing verify3dLine, whose 8-of-10 decile rule needs 8 points: a line after them
    sees a shifted rand() stream.  From 7.5 px on RANSAC succeeds at once; at z = 2 the 7 px between the end points are 7 / 256 m
    > 0.02, at z = 1 they are 7 / 512 m < 0.02 (short in 3-D) and only the 20-sample lines survive (20 / 512 m)."""
    segs = [(x0, 8.5 + 4 * i, x0 + L, 8.5 + 4 * i) for i, L in enumerate(lens)]
    acc = [L >= 7.5 if z == 2.0 else L >= 20.5 for L in lens]
    reg = {}
    for i, L in enumerate(lens):
        if L < 4.5:
            reg[i] = dict(exit_reason=oracle_lib.LINE_FEW_POINTS, rand_drawn=0, np=4)
        elif L < 7.5:
            reg[i] = dict(exit_reason=oracle_lib.LINE_NO_VERIFIED_SET, rand_drawn=20, iterations=10, verify_passes=0)
        else:
            reg[i] = dict(exit_reason=oracle_lib.LINE_ACCEPTED if acc[i] else oracle_lib.LINE_SHORT_3D, rand_drawn=2, iterations=1, verify_passes=1,
                          refine_grew=0)
    if reverse:
        segs, acc = segs[::-1], acc[::-1]
        reg = {len(lens) - 1 - i: v for i, v in reg.items()}
    return _case(f"lengths_z{z:g}{'_rev' if reverse else ''}", segs, wall(w, h, z), camera(w, h), accepted=acc, regime=reg)


# ---- holes --------------------------------------------------------------------------------------------------------------------
def holes():
    """9.5 px lines (10 samples) with 1, 2, 3 leading samples zeroed: 9, 8, 7 points - accepted, accepted, rejected (7 points fill at
    most 7 deciles).  Then the hole threshold itself on 4.5 px lines (5 samples, np < 5 decides): a depth of exactly float32(0.01) is
    a hole (4 points, no rand() drawn), the next float above it is a sample (5 points, 20 rand() values).  Then a 20.5 px line with a
    NaN and a +Inf sample in the middle: both become points (NaN <= 0.01 is false) that are in no inlier set; the line is accepted
    with finite outputs and the end points of the clean line.  The last line straddles a depth step, so its answer depends on the
    rand() values the lines before it drew."""
    w, h = 64, 48
    d = wall(w, h)
    segs = [(10.25, 4.5 + 3 * i, 19.75, 4.5 + 3 * i) for i in range(3)]
    for i in range(3):
        d[4 + 3 * i, 10:10 + i + 1] = 0.0
    segs += [(10.25, 16.5, 14.75, 16.5), (10.25, 19.5, 14.75, 19.5)]
    d[16, 12] = F32(0.01)
    d[19, 12] = np.nextafter(F32(0.01), F32(1))
    segs += [(10.25, 22.5, 30.75, 22.5)]
    d[22, 17], d[22, 23] = np.nan, np.inf
    d[30:40, 30:] = 2.5
    segs += [(19.25, 34.5, 39.75, 34.5)]
    reg = {0: dict(np=9, holes=1), 1: dict(np=8, holes=2), 2: dict(np=7, holes=3, exit_reason=oracle_lib.LINE_NO_VERIFIED_SET),
           3: dict(np=4, holes=1, rand_drawn=0, exit_reason=oracle_lib.LINE_FEW_POINTS),
           4: dict(np=5, holes=0, rand_drawn=20, exit_reason=oracle_lib.LINE_NO_VERIFIED_SET),
           5: dict(np=21, holes=0, final_inliers=19, exit_reason=oracle_lib.LINE_ACCEPTED), 6: dict(iterations=10, ransac_inliers=11)}
    return _case("holes", segs, d, camera(w, h), accepted=[True, True, False, False, False, True, True], regime=reg, seeds=(1, 2),
                 ends={0: ((11, 4), (19, 4)), 1: ((12, 7), (19, 7)), 5: ((10, 22), (30, 22)), 6: ((19, 34), (29, 34))})


# ---- borders ------------------------------------------------------------------------------------------------------------------
def borders(w=64, h=48):
    """Lines on and across the image border on the wall at z = 2: along row 0 and column 0 from the corner (integer coordinates: every
    sample takes the max(int(p - 1), 0) branch and the clamp binds on the whole line), along row 10 (the clamp binds on the first
    sample only), ending half a pixel inside the right border, ending exactly ON x = w in the last row (that sample is outside),
    starting 5.5 px left of the image, ending 10.5 px right of it, starting 3.5 px above it."""
    lh, lv = min(30, w - 2), min(30, h - 2)
    segs = [(0, 0, lh, 0), (0, 0, 0, lv), (0, 10, lh, 10), (w - 20.5, 5.5, w - 0.5, 5.5), (w - 20, h - 1, w, h - 1), (-5.5, 7.5, 15.25, 7.5),
            (w - 10.25, 9.5, w + 10.5, 9.5), (12.5, -3.5, 12.5, 17.25)]
    return _case(f"borders_{w}x{h}", segs, wall(w, h), camera(w, h), accepted=[True] * 8)


# borders(32, 24) written out: per line (samples outside, in the integer branch, clamped, points) and the pixels (col, row) read.
# Line 0 steps 1.5 px: every second sample is integral and reads the pixel to its left; line 2 alternates between rows 9 and 10.
BORDERS_32x24 = [
    (0, 11, 11, 21, [(0, 0), (1, 0), (2, 0), (4, 0), (5, 0), (7, 0), (8, 0), (10, 0), (11, 0), (13, 0), (14, 0), (16, 0), (17, 0), (19, 0), (20, 0),
                     (22, 0), (23, 0), (25, 0), (26, 0), (28, 0), (29, 0)]),
    (0, 3, 3, 21, [(0, r) for r in range(22) if r != 11]),
    (0, 11, 1, 21, [(0, 9), (1, 10), (2, 9), (4, 10), (5, 9), (7, 10), (8, 9), (10, 10), (11, 9), (13, 10), (14, 9), (16, 10), (17, 9), (19, 10),
                    (20, 9), (22, 10), (23, 9), (25, 10), (26, 9), (28, 10), (29, 9)]),
    (0, 0, 0, 21, [(c, 5) for c in range(11, 32)]),
    (1, 20, 0, 20, [(c, 22) for c in range(11, 31)]),
    (6, 0, 0, 15, [(c, 7) for c in range(16) if c != 8]),
    (11, 0, 0, 10, [(c, 9) for c in range(21, 32) if c != 28]),
    (4, 0, 0, 17, [(12, r) for r in range(18) if r != 10]),
]
# all eight lines together: (samples tried, outside, integer branch, clamped, points)
BORDERS_TOTALS = {(32, 24): (168, 22, 45, 15, 146), (64, 48): (168, 22, 53, 23, 146), (640, 480): (168, 22, 53, 23, 146)}


def stride_case():
    """The borders and lengths lines of one 640x480 frame whose depth rows are 647 floats apart; the 7 floats of padding hold a wall at
    0.5 m, so a sampler that steps through the rows with the width reads another wall.  Answers as with a tight stride.
    A few samples of the other wall are outliers that most lines survive, so the last line is placed where they decide: 7.5 px
    (8 samples, verify3dLine needs all 8) in row 477, where 477 * 640 + 100 .. 103 are the padding of row 471 (7 * 477 = 104 mod 647)."""
    w, h, s = 640, 480, 647
    b, ln = borders(w, h), lengths(w=w, h=h, x0=100.25)
    buf = np.full((h, s), 0.5, np.float32)
    buf[:, :w] = WALL
    segs = np.concatenate([b["segs"], ln["segs"] + np.float32([0, 100, 0, 100]), np.float32([[100.25, 477.5, 107.75, 477.5]])])
    reg = {8 + i: v for i, v in ln["regime"].items()}
    return _case("stride", segs, buf[:, :w], camera(w, h), depth_stride=s, accepted=b["accepted"] + ln["accepted"] + [True], regime=reg)


# ---- step ---------------------------------------------------------------------------------------------------------------------
def step(left, seed):
    """One 20.5 px line (21 samples) across a depth step from 2 m to 2.5 m with `left` samples on the near side: two collinear 3-D
    segments half a metre apart in depth.  Which side wins, how many iterations that takes and what the refinement does depends on
    the pairs drawn: the regimes are in STEP_REGIMES, read from the oracle's trace."""
    w, h = 64, 48
    d = wall(w, h)
    d[:, 30:] = 2.5
    x0 = 30 - left
    near = left > 10   # the larger side wins
    ends = {0: ((x0, 20), (29, 20)) if near else ((30, 20), (x0 + 20, 20))}
    return _case(f"step_{left}_{21 - left}_seed{seed}", [(x0 + 0.25, 20.5, x0 + 20.75, 20.5)], d, camera(w, h), seeds=(seed,), accepted=[True],
                 regime={0: dict(STEP_REGIMES[(left, seed)], ransac_inliers=max(left, 21 - left), refine_grew=0, exit_reason=oracle_lib.LINE_ACCEPTED)},
                 ends=ends)


# read from the oracle's trace.  11 / 10: neither side exceeds 0.6 * 21 = 12.6, all ten iterations run; with seeds 2 and 12345 a set of
# 10 is verified first and replaced by the 11.  6 / 15 and 3 / 18: the break `> np * 0.6` comes in the first iteration when the first
# pair lies on the large side, in the second otherwise.
STEP_REGIMES = {(11, 1): dict(iterations=10, rand_drawn=20, verify_passes=1, replaced=0), (11, 2): dict(iterations=10, rand_drawn=20, verify_passes=2, replaced=1),
                (11, 12345): dict(iterations=10, rand_drawn=20, verify_passes=2, replaced=1),
                (6, 1): dict(iterations=2, verify_calls=2, verify_passes=1), (6, 2): dict(iterations=1, verify_calls=1), (6, 12345): dict(iterations=2, verify_calls=2),
                (3, 1): dict(iterations=2, verify_calls=2, verify_passes=1), (3, 2): dict(iterations=1, verify_calls=1), (3, 12345): dict(iterations=2, verify_calls=2)}


def crease(a):
    """The wall bends away right of column 29: depth 2 + a * (col - 29) / 10 there.  The pair the RANSAC draws (seed 1) fits one side and
    part of the other; the SVD refit over those inliers reaches further.  Found by a search over a and the seed on the oracle: a = 0.04
    -> 20 inliers, the refinement grows once to 21; a = 0.08 -> 15 inliers, it grows twice to 21."""
    w, h = 64, 48
    u = np.arange(w)
    d = wall(w, h)
    d[:] = (2 + a * np.maximum(u - 29, 0) / 10.0).astype(np.float32)[None, :]
    grew, first = {0.04: (1, 20), 0.08: (2, 15)}[a]
    return _case(f"crease_{a:g}", [(19.25, 20.5, 39.75, 20.5)], d, camera(w, h), accepted=[True],
                 regime={0: dict(ransac_inliers=first, refine_grew=grew, final_inliers=21, exit_reason=oracle_lib.LINE_ACCEPTED)},
                 ends={0: ((19, 20), (39, 20))})


# ---- slant / planes / fan_order: crossing pairs ------------------------------------------------------------------------------------
def slant(flat=False):
    """Two COLLINEAR segments of one image diagonal on the wall 2 / (0.3 x + 0.1 y + 0.9), paired by one fan row.  Their 3-D directions
    agree to about 7 digits; det = -(d11 * d22 - d12 * d12) cancels to a rounding residue that is not zero, so a crossing exists, and the
    plane normal is the normalised difference of two nearly equal float directions: any contraction or reassociation of the float cross
    product or of the f64 dot products changes it.  On the flat wall the same pair has det == 0 exactly: no crossing."""
    w, h = 640, 480
    cam = camera(w, h)
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = (u - 320) / 512, (v - 240) / 512
    d = wall(w, h) if flat else (2.0 / (0.3 * x + 0.1 * y + 0.9)).astype(np.float32)
    segs = [(50.5, 50.5, 150.5, 150.5), (200.5, 200.5, 260.5, 260.5)]
    return _case("slant_flat" if flat else "slant", segs, d, cam, fans=[(175.0, 175.0, 0, 1)], accepted=[True, True], ends="wall" if flat else None,
                 ncross=0 if flat else 1, nplanes=None if not flat else 0)


def _cross_lines(x, y, n=21.5):
    """a horizontal and a vertical segment from (x, y): they meet in their common start pixel"""
    return [(x + 0.25, y + 0.5, x + n, y + 0.5), (x + 0.5, y + 0.25, x + 0.5, y + n)]


def planes_parallel(gap):
    """Two crossing pairs on two fronto-parallel walls `gap` apart (left and right half of the image).  Both planes are (0, 0, 1, -z)
    flipped to (-0, -0, -1, z).  OldPlane calls the second one old when |d| <= 0.2 (and the normals agree): gap 0.15 -> one plane, gap
    0.25 -> two."""
    w, h = 64, 48
    d = wall(w, h)
    d[:, 32:] = F32(WALL + gap)
    segs = _cross_lines(4, 4) + _cross_lines(36, 4)
    return _case(f"planes_gap{gap:g}", segs, d, camera(w, h), fans=[(4.5, 4.5, 0, 1), (36.5, 4.5, 2, 3)], accepted=[True] * 4, ncross=2,
                 nplanes=1 if gap < 0.2 else 2, plane_reasons=[oracle_lib.PLANE_ACCEPTED, oracle_lib.PLANE_OLD if gap < 0.2 else oracle_lib.PLANE_ACCEPTED])


def planes_tilt(deg):
    """A fronto-parallel wall on the left, a wall turned by `deg` degrees about the vertical axis on the right, both 2 m from the camera
    centre along their normals (d equal: the distance test of OldPlane passes).  cos 15 deg = 0.966 > 0.9397 -> old, cos 25 deg =
    0.906 < 0.9397 -> a second plane."""
    w, h = 64, 48
    t = np.deg2rad(deg)
    u = np.arange(w, dtype=np.float64)
    d = wall(w, h)
    d[:, 32:] = (WALL / (np.sin(t) * (u[32:] - 32) / 512 + np.cos(t))).astype(np.float32)[None, :]
    segs = _cross_lines(4, 4) + _cross_lines(36, 4)
    return _case(f"planes_tilt{deg}", segs, d, camera(w, h), fans=[(4.5, 4.5, 0, 1), (36.5, 4.5, 2, 3)], accepted=[True] * 4, ncross=2,
                 nplanes=1 if deg < 20 else 2, ends=None,
                 plane_reasons=[oracle_lib.PLANE_ACCEPTED, oracle_lib.PLANE_OLD if deg < 20 else oracle_lib.PLANE_ACCEPTED])


def planes_spread(delta):
    """A horizontal line on the wall at 2 m and a vertical one on a ridge `delta` nearer (columns 4 .. 5 below row 5; the horizontal line
    runs in row 4, the vertical one in column 4 from row 5 on): skew perpendicular lines.  The normal is the z axis, the five
    distances are 2, 2, 2 - delta, 2 - delta and the crossing half way, so their spread is delta: 3/64 = 0.046875 passes the 0.05
    test, 7/128 = 0.0546875 fails it."""
    w, h = 64, 48
    d = wall(w, h)
    d[5:, 4:6] = F32(WALL - delta)
    segs = [(4.25, 4.5, 25.5, 4.5), (4.5, 5.25, 4.5, 26.5)]
    ok = delta < 0.05
    return _case(f"planes_spread{delta:g}", segs, d, camera(w, h), fans=[(4.5, 4.5, 0, 1)], accepted=[True, True], ncross=1, nplanes=1 if ok else 0,
                 plane_reasons=[oracle_lib.PLANE_ACCEPTED if ok else oracle_lib.PLANE_SPREAD])


FLAT_PLANE = np.array([-0.0, -0.0, -1.0, 2.0], np.float32)   # the plane of a crossing pair on the wall at 2 m, negative zeros included


def plane_flip():
    """One crossing pair on the wall: (0, 0, 1, -2) has a negative distance and is flipped to FLAT_PLANE - compared as bytes."""
    w, h = 64, 48
    return _case("plane_flip", _cross_lines(4, 4), wall(w, h), camera(w, h), fans=[(4.5, 4.5, 0, 1)], accepted=[True, True], ncross=1, nplanes=1,
                 plane_reasons=[oracle_lib.PLANE_ACCEPTED], planes=FLAT_PLANE[None, :])


FAN_ORDER_HITS = (0, 63, 64, 65, 127, 128, 129)


def fan_order():
    """130 fan rows over a horizontal (0) and a vertical (1) good line and a rejected 3.5 px line (2).  Rows FAN_ORDER_HITS pair the two
    good lines - alternately as (0, 1) and (1, 0) - and give a crossing; every other row pairs a good line with the rejected one, whose
    3-D line is all zeros: det == 0.  The hits sit on both sides of the 64-row rounds of the ballot compaction; x = the row number."""
    w, h = 64, 48
    segs = _cross_lines(4, 4) + [(40.25, 40.5, 43.75, 40.5), (50.25, 40.5, 51.0, 40.5)]   # line 3: shorter than 1 px, no sample at all
    fans = np.zeros((130, 4), np.float32)
    for i in range(130):
        fans[i] = (i, 2 * i, i % 2, 2) if i % 3 else (i, 2 * i, 2, i % 2)
    for k, i in enumerate(FAN_ORDER_HITS):
        fans[i, 2:] = (0, 1) if k % 2 == 0 else (1, 0)
    pair = np.array([(0, 1) if k % 2 == 0 else (1, 0) for k in range(7)], np.int32)
    xy = np.array([(i, 2 * i) for i in FAN_ORDER_HITS], np.float32)
    return _case("fan_order", segs, wall(w, h), camera(w, h), fans=fans, accepted=[True, True, False, False], ncross=7, nplanes=1, pair=pair, xy=xy,
                 regime={2: dict(exit_reason=oracle_lib.LINE_FEW_POINTS), 3: dict(exit_reason=oracle_lib.LINE_NO_SAMPLES, tried=0)},
                 plane_reasons=[oracle_lib.PLANE_ACCEPTED] + [oracle_lib.PLANE_OLD] * 6, planes=FLAT_PLANE[None, :])


def duplicate_pixel():
    """(0, 0) - (6, 0): seven integral samples one pixel apart; x = 0 is clamped onto the pixel that x = 1 reads, so two of the seven
    points coincide.  Seven points never pass verify3dLine, all ten iterations run, and with seed 1 one of them draws the coinciding
    pair: the `norm(B - A) < 1e-10` continue of the RANSAC."""
    w, h = 64, 48
    return _case("duplicate_pixel", [(0, 0, 6, 0)], wall(w, h), camera(w, h), accepted=[False],
                 regime={0: dict(np=7, clamped=7, iterations=10, degenerate=1, verify_calls=9, exit_reason=oracle_lib.LINE_NO_VERIFIED_SET)})


def tie_ends():
    """Two DIFFERENT points with exactly the same projection on the line: with cx = 160 the columns 31 and 32 are 129 and 128 px left of
    the principal point, and the wall is at 2 m up to column 31 and at 2 * 129 / 128 = 2.015625 m from column 32 on (1.3 sigma of the
    depth noise model: all 21 samples are inliers), so both points have x = -129 / 256.  With seed 1 the RANSAC draws samples 1 and 7,
    both on the farther part: the direction is exactly (dx, 0, 0), the projections of samples 0 and 1 tie exactly, and the reference's
    `if (dproduct < minv)` keeps the FIRST: the end point is the pixel (31, 20) at 2 m, not (32, 20)."""
    w, h = 64, 48
    cam = camera(w, h)
    cam["cx"] = 160.0
    d = wall(w, h)
    d[:, 32:] = F32(2.015625)
    return _case("tie_ends", [(31.25, 20.5, 51.75, 20.5)], d, cam, accepted=[True], ends={0: ((31, 20), (51, 20))},
                 regime={0: dict(np=21, iterations=1, ransac_inliers=21, refine_grew=0, final_inliers=21)})


def full_groups():
    """every line has all 21 samples valid (the neighbour of lane 63 in the last group of a wave is a full group)"""
    w, h = 64, 48
    segs = [(10.25 + i, 2.5 + 2 * i, 31.75 + i, 2.5 + 2 * i) for i in range(12)]
    return _case("full_groups", segs, wall(w, h), camera(w, h), accepted=[True] * 12)


def stale_rows_second():
    """10 lines, a crossing pair in rows 3 and 5, and three fan rows, two of which name lines 40 and 41 that the frame does not have:
    only (3, 5) can give a crossing."""
    w, h = 64, 48
    cr = _cross_lines(4, 4)
    segs = [(10.25, 30.5 + i, 31.75, 30.5 + i) for i in range(10)]
    segs[3], segs[5] = cr[0], cr[1]
    return _case("stale_rows", segs, wall(w, h), camera(w, h), fans=[(1, 1, 3, 40), (2, 2, 40, 41), (4.5, 4.5, 3, 5)], accepted=[True] * 10, ncross=1,
                 nplanes=1, pair=np.array([(3, 5)], np.int32))   # no written plane: the signs of its zeros follow the pair the seed draws


def stale_rows_first():
    """64 good lines; rows 40 and 41 are verticals that cross the horizontal row 3 of this frame and of stale_rows_second, so that a
    kernel that reads the rows 40 / 41 an earlier launch left behind finds a crossing"""
    w, h = 64, 48
    segs = [(4.25, 4.5 + (i % 20), 25.75, 4.5 + (i % 20)) for i in range(64)]
    segs[40] = (4.5, 4.25, 4.5, 25.75)
    segs[41] = (8.5, 4.25, 8.5, 25.75)
    return _case("stale_rows_first", segs, wall(w, h), camera(w, h), fans=[(4.5, 7.5, 3, 40), (8.5, 7.5, 3, 41)], accepted=[True] * 64, ncross=2,
                 nplanes=None)


STEP_SPLITS, STEP_SEEDS = (11, 6, 3), (1, 2, 12345)


@functools.lru_cache(maxsize=None)
def small_cases():
    """every 64x48 case frame (one image size; one camera but for tie_ends)"""
    cs = [lengths(2.0), lengths(1.0), lengths(2.0, reverse=True), lengths(1.0, reverse=True), holes(), borders(64, 48)]
    cs += [step(l, s) for l in STEP_SPLITS for s in STEP_SEEDS] + [crease(0.04), crease(0.08)]
    cs += [planes_parallel(0.15), planes_parallel(0.25), planes_tilt(15), planes_tilt(25), planes_spread(3 / 64), planes_spread(7 / 128), plane_flip(),
           fan_order(), duplicate_pixel(), tie_ends(), full_groups()]
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def other_cases():
    """32x24 and 640x480 frames"""
    return (borders(32, 24), borders(640, 480), stride_case(), slant(), slant(flat=True))


def all_cases():
    return small_cases() + other_cases()


KEYS = ("lines3d", "lineEq", "pair", "xy", "cross", "le_l", "planes", "normals", "lineNo", "cross3d", "cross2d")


def check_answers(case, out):
    """the written-down answers of `case` against one result dict (the oracle's or the device's)"""
    name = case["name"]
    for k in KEYS:
        assert not np.isnan(out[k]).any() and not np.isinf(out[k]).any(), (name, k, "NaN or Inf in an output")
    acc = np.abs(out["lines3d"]).sum(1) > 0
    assert acc.tolist() == [bool(a) for a in case["accepted"]], (name, "accepted lines", acc.astype(int).tolist())
    assert np.all(out["lineEq"][~acc] == -1), (name, "lineEq of a rejected line")
    for i in np.flatnonzero(acc):
        e = case["ends"]
        if e is None or (isinstance(e, dict) and i not in e):
            continue
        a, b = wall_ends(case, i) if isinstance(e, str) else e[i]
        pa, pb = (point3d(c, r, float(case["depth"][r, c]), case["cam"]) for c, r in (a, b))
        got = out["lines3d"][i].reshape(2, 3)
        assert (np.array_equal(got[0], pa) and np.array_equal(got[1], pb)) or (np.array_equal(got[0], pb) and np.array_equal(got[1], pa)), \
            (name, "end points of line", int(i), got.tolist(), pa.tolist(), pb.tolist())
    if case["ncross"] is not None:
        assert len(out["pair"]) == case["ncross"], (name, "crossings", len(out["pair"]))
    if case["nplanes"] is not None:
        assert len(out["planes"]) == case["nplanes"], (name, "planes", out["planes"].tolist())
    for k in ("pair", "xy", "planes"):
        if k in case:
            assert out[k].tobytes() == case[k].tobytes(), (name, k, out[k].tolist())
