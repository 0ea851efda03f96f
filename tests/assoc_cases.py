"""Hand-built inputs with known answers for the association routines of psl-slam_amd/csrc/pslfe_assoc.hip, in the style of
tests/window_cases.py: LSDmatcher::SearchByGeomNApearance, LSDmatcher::FrameBFMatch (+ lineDescriptorMAD) and
Map::AssociatePlanesByBoundary (live) / InsectLineMatch::SearchMapInsectline.  Pure numpy, nothing is run to obtain an answer;
tests/test_assoc_cases_cpu.py holds the answers to oracle/assoc_oracle.cpp, tests/test_assoc_gpu.py holds the kernels to both.

Descriptors are thermometer codes (window_cases.T / TT): every Hamming distance is chosen.  Answers that depend on float
arithmetic (the nearest-neighbour ratio, the MAD threshold) are computed here in numpy.float32 / float64 in the reference's order
of operations."""
import numpy as np

from window_cases import T, TT
from line_window_cases import keylines

F32, F64 = np.float32, np.float64
up = lambda v: np.nextafter(F32(v), F32(np.inf))


# ---- LSDmatcher::SearchByGeomNApearance (add_src/LSDmatcher.cpp:36-110) -----------------------------------------------------------
GEOM_BOUNDS = (0.0, 640.0, 0.0, 480.0)        # (mnMinX, mnMaxX, mnMinY, mnMaxY)
DELTA_W, DELTA_H = F64(F32(640.0) - F32(0.0)) * 0.1, F64(F32(480.0) - F32(0.0)) * 0.1
assert DELTA_W == 64.0 and DELTA_H == 48.0    # so |dx| == deltaWidth can be hit exactly in float32


class GeomCase:
    """Ten current lines with descriptors T(20 j); last-frame line i aims at current line j with T(20 j + e): its nearest neighbours
    are j at distance e and j + 1 (j - 1 for the last) at 20 - e, and matchNNR keeps j iff e < (20 - e) * desc_th in float32.
    `spec[i]` = (j, e, segment, has_mapline, outcome); outcome: "match" | "dir" (20 degree gate) | "far" (both end points farther
    than a tenth of the image) | "skip0" (the current line's startPointX == 0: left as matchNNR found it, not assigned) | "nomap"
    (no map line: left as matchNNR found it) | "tie" (both neighbours at 10: the ratio fails for every desc_th <= 1)."""

    def __init__(self, name, cur_segs, spec):
        self.name, self.bounds, self.spec = name, GEOM_BOUNDS, spec
        self.kl_cur, _ = keylines(cur_segs)
        self.kl_cur["startPointX"][2] = -0.0
        assert self.kl_cur["startPointX"][1] == 0.0 and np.signbit(self.kl_cur["startPointX"][2])
        self.d_cur = np.array([T(20 * j) for j in range(len(cur_segs))], np.uint8)
        self.kl_last, _ = keylines([s[2] for s in spec])
        self.d_last = np.array([T(20 * s[0] + s[1]) for s in spec], np.uint8)
        self.has = np.array([s[3] for s in spec], np.uint8)

    def __repr__(self):
        return self.name

    def expected(self, desc_th):
        """-> (lmatches, matches12, assigned)"""
        m12, asg, n = np.full(len(self.spec), -1, np.int32), np.full(len(self.kl_cur), -1, np.int32), 0
        for i, (j, e, _, has, outcome) in enumerate(self.spec):
            if outcome == "tie" or not F32(e) < F32(20 - e) * F32(desc_th):
                continue
            if outcome in ("match", "skip0", "nomap"):
                m12[i] = j
            if outcome == "match":
                asg[j], n = i, n + 1          # a later last-frame line overwrites an earlier one (:104)
        return n, m12, asg


def geom_case():
    """n1 = 300 (the kernel strides by 256 threads).  Current lines: 0 the target of a crowd, 1 and 2 with startPointX 0.0 and
    -0.0, 3 the end-point gate's, 4 (40 px) the direction gate's, 5 the fillers', 6 / 7 the tie's.
    Lines 250 .. 289 all have current line 0 as nearest neighbour, in the cycle match / dir / far / nomap: the largest passing one
    is 286, the largest overall, 289, has no map line."""
    cur = [(100, 100, 200, 100), (0, 150, 100, 150), (0, 170, 100, 170), (100, 200, 200, 200), (100, 300, 140, 300),
           (300, 100, 400, 100), (300, 200, 400, 200), (300, 300, 400, 300), (450, 100, 550, 100), (450, 200, 550, 200)]
    ray = lambda x, y, a: (x, y, x + 40 * np.cos(np.deg2rad(a)), y + 40 * np.sin(np.deg2rad(a)))
    spec = [(3, 0, (100, 200, 200, 200), 1, "match"),
            (3, 1, (165, 200, 200, 200), 1, "match"),                 # start far only
            (3, 2, (100, 200, 265, 200), 1, "match"),                 # end far only
            (3, 0, (165, 200, 265, 200), 1, "far"),
            (3, 1, (164, 200, 265, 200), 1, "match"),                 # |dx| of the start == deltaWidth: > is strict
            (3, 2, (up(164), 200, 265, 200), 1, "far"),
            (3, 0, (100, 248, 200, 248), 1, "match"),                 # |dy| of both == deltaHeight
            (3, 1, (100, up(248), 200, up(248)), 1, "far"),
            (4, 0, ray(100, 300, 18), 1, "match"), (4, 1, ray(100, 300, 22), 1, "dir"),
            (4, 2, ray(100, 300, -18), 1, "match"), (4, 0, ray(100, 300, -22), 1, "dir"),
            (4, 1, ray(140, 300, 198), 1, "match"), (4, 2, ray(140, 300, 202), 1, "dir"),   # anti-parallel: fabs
            (1, 0, (0, 150, 100, 150), 1, "skip0"), (1, 1, (0, 150, 0, 250), 1, "skip0"),   # skipped before the direction gate
            (2, 0, (0, 170, 100, 170), 1, "skip0"), (2, 2, (300, 170, 400, 170), 1, "skip0"),
            (6, 10, (300, 200, 400, 200), 1, "tie"), (6, 10, (300, 200, 400, 200), 0, "tie"),
            (5, 0, (300, 100, 300, 200), 0, "nomap"), (3, 2, (165, 200, 265, 200), 0, "nomap")]
    while len(spec) < 250:
        spec.append((5, len(spec) % 3, (300, 100, 400, 100), 1, "match"))
    crowd = [("match", (100, 100, 200, 100)), ("dir", (100, 100, 100, 200)), ("far", (170, 100, 270, 100)), ("nomap", (100, 100, 200, 100))]
    for k in range(40):
        outcome, seg = crowd[k % 4]
        spec.append((0, k % 3, seg, 0 if outcome == "nomap" else 1, outcome))
    while len(spec) < 300:
        spec.append((8, len(spec) % 3, (450, 100, 550, 100), 1, "match"))
    c = GeomCase("geom-300", cur, spec)
    assert [s[4] for s in spec[286:290]] == ["match", "dir", "far", "nomap"] and c.expected(0.95)[2][0] == 286
    return c


# ---- LSDmatcher::FrameBFMatch (add_src/LSDmatcher.cpp:492-516, lineDescriptorMAD :660-685) -----------------------------------------
BF_TRAIN = np.array([TT(0, 0), TT(128, 0), TT(0, 127)], np.uint8)


def bf_query(a, kind):
    """a query at distance a from its nearest train row: "x0" / "x1": nearest row 0 / 1, the second at 128 - a (an even margin
    128 - 2 a); "z0" / "z2": nearest row 0 / 2, the second at 127 - a (an odd margin 127 - 2 a)"""
    assert 1 <= a <= 63 or (a == 64 and kind == "x0")
    return {"x0": TT(a, 0), "x1": TT(128 - a, 0), "z0": TT(0, a), "z2": TT(0, 127 - a)}[kind]


def bf_expected(d1, d2, nnratio, TH):
    """knnMatch(k = 2) by brute force, then FrameBFMatch's gates with the MAD threshold as the reference computes it: float
    margins, the element of rank n1 / 2, fabsf of a double difference, a double product.  -> (lineMatches, margins, threshold)"""
    d1, d2 = np.asarray(d1, np.uint8).reshape(-1, 32), np.asarray(d2, np.uint8).reshape(-1, 32)
    n1 = len(d1)
    if n1 == 0 or len(d2) < 2:
        return np.full(n1, -1, np.int32), None, None
    D = np.unpackbits(d1[:, None, :] ^ d2[None, :, :], axis=2).sum(2).astype(np.int64)
    order = np.argsort(D, axis=1, kind="stable")
    a, b = D[np.arange(n1), order[:, 0]].astype(F32), D[np.arange(n1), order[:, 1]].astype(F32)
    margin = (b - a).astype(F32)
    median = F64(np.sort(margin)[n1 // 2])
    dev = np.abs((b.astype(F64) - a.astype(F64) - median).astype(F32))
    th = F64(1.4826) * F64(np.sort(dev)[n1 // 2])
    th = th * 0.5
    ok = (margin.astype(F64) > th) & (a < F32(TH)) & (a < F32(nnratio) * b)
    return np.where(ok, order[:, 0], -1).astype(np.int32), margin, th


class BFCase:
    def __init__(self, name, queries, nnratio=0.95, TH=80.0, train=BF_TRAIN, seed=0):
        q = [bf_query(a, k) for a, k in queries]
        perm = np.random.default_rng(seed).permutation(len(q))
        self.name, self.d1, self.d2, self.nnratio, self.TH = name, np.array(q, np.uint8).reshape(-1, 32)[perm], train, nnratio, TH
        self.expected, self.margin, self.th = bf_expected(self.d1, self.d2, nnratio, TH)

    def __repr__(self):
        return self.name


def bf_spread(n1, nnratio=0.95, TH=80.0):
    """A third of the margins at 4, a third at 40 (the median, one of many equal values), the rest at 76 / 77: the MAD is 36, one
    of many equal deviations, and the threshold 0.5 * 1.4826 * 36 = 26.69.  Two queries sit on either side of it, margins 26 and
    27; distances 29 / 30 around TH = 30 and a ratio that fails (62 against 66 at 0.85) come with the lows and highs."""
    third = n1 // 3
    qs = [(62, "x0" if i % 2 else "x1") for i in range(third)] + [(44, ("x0", "x1")[i % 2]) for i in range(third)] + [(51, "x1"), (50, "z2")]
    qs += [((26, "x0"), (25, "z0"), (26, "x1"), (25, "z2"))[i % 4] for i in range(n1 - len(qs))]
    c = BFCase(f"bf-spread-n{n1}-r{nnratio}-TH{TH}", qs, nnratio, TH, seed=n1)
    assert c.th == 0.5 * (1.4826 * 36.0) and (c.margin == 40).sum() >= 3 and np.sort(c.margin)[n1 // 2] == 40
    lo, hi = c.expected[c.margin == 26], c.expected[c.margin == 27]
    assert len(lo) == 1 and len(hi) == 1 and lo[0] == -1 and (hi[0] == 2 or TH <= 50)
    return c


def bf_cases():
    cs = [bf_spread(n) for n in (255, 256, 257)] + [bf_spread(257, 0.85), bf_spread(256, 0.95, 30.0), bf_spread(255, 0.95, 26.0)]
    cs += [BFCase("bf-one", [(44, "x1")]),                                          # n1 = 1: the MAD is 0, the gate is > 0
           BFCase("bf-two-4-76", [(62, "x0"), (26, "x1")]),                         # n1 = 2: MAD = 72, threshold 53.4: the 4 fails
           BFCase("bf-two-40-50", [(44, "x0"), (39, "x1")]),
           BFCase("bf-all-equal-256", [(44, ("x0", "x1")[i % 2]) for i in range(256)]),   # MAD 0: every margin 40 > 0 passes
           BFCase("bf-all-zero-65", [(64, "x0")] * 65),                             # margins 0: 0 > 0 fails
           BFCase("bf-two-rows-100", [((10 + i % 50), ("x0", "x1")[i % 2]) for i in range(100)], train=BF_TRAIN[:2])]   # n2 = 2
    assert cs[6].th == 0 and cs[6].expected[0] == 1 and list(np.sort(cs[7].expected)) == [-1, 1] and cs[9].th == 0 and (cs[9].expected >= 0).all()
    assert (cs[10].expected == -1).all() and (cs[10].margin == 0).all() and (cs[4].expected >= 0).sum() < (cs[1].expected >= 0).sum()
    return cs


# ---- Map::AssociatePlanesByBoundary (src/Map.cc:204-272) / InsectLineMatch::SearchMapInsectline (add_src/InsectlineMatch.cpp:9-59) ----
class PlaneCase:
    """Map planes (0, 0, +-1, d); the five boundary points of a frame plane all lie at height z, so its distance to (0, 0, 1, d) is
    z + d, exact in the binary fractions used.  frame: (normal, z) per plane."""

    def __init__(self, name, live, frame, map_planes, expected, nmatches, dTh=0.5, aTh=0.5, bad=None):
        self.name, self.live, self.dTh, self.aTh = name, live, dTh, aTh
        self.planes = np.array([tuple(nrm) + (0.0,) for nrm, _ in frame], np.float32)
        xy = np.array([(0, 0), (1, 0), (0, 1), (-1, 0), (0.5, -1)], F64)
        self.points = np.array([np.concatenate([xy, np.full((5, 1), z)], 1) for _, z in frame], F64)
        self.map = np.array(map_planes, np.float32).reshape(-1, 4)
        self.bad = None if bad is None else np.array(bad, np.uint8)
        self.expected, self.nmatches = np.array(expected, np.int32), nmatches

    def __repr__(self):
        return self.name


def plane_cases():
    Z = (0.0, 0.0, 1.0)
    a, b, c = (Z, -1.25), (Z, -0.875), (Z, -0.9375)       # distances to (0, 0, 1, 1): -0.25, 0.125, 0.0625
    W0, W1, W3 = (0, 0, 1, 1.0), (0, 0, 1, 0.9375), (0, 0, 1, 0.875)
    half_up = float(up(0.5))
    tilt = lambda s: (0.0, 0.8660254, s)
    cs = [
        # live: the threshold is the signed distance and outlives the plane (:249-251).  a leaves -0.25: nothing matches after it
        PlaneCase("live-a-b-c", True, [a, b, c], [W0, W1], [0, -1, -1], 1),
        # b: W0 at 0.125, then W1 at 0.0625 (two updates); c: W0 at 0.0625 is not < 0.0625, W1 at 0 is; a: nothing is < 0
        PlaneCase("live-b-c-a", True, [b, c, a], [W0, W1], [1, 1, -1], 3),
        # live: (0, 0, -1, -1) is flipped to (0, 0, 1, 1): a's distance is -0.25, not +0.25, and b finds nothing
        PlaneCase("live-flip", True, [a, b], [(0, 0, -1, -1.0)], [0, -1], 1),
        PlaneCase("live-no-flip-at-zero", True, [b], [(0, 0, -1, 0.0)], [-1], 0),     # d = 0 is not flipped: distance 0.875
        # dead: bad map planes are skipped, the threshold starts again at dTh with every plane, one match per plane
        PlaneCase("dead-a-b-c", False, [a, b, c], [W0, W1, W3], [1, 2, 1], 3, bad=[1, 0, 0]),
        PlaneCase("dead-not-flipped", False, [a, b], [(0, 0, -1, -1.0)], [0, 0], 2),  # +0.25 and -0.125: no flip in this variant
    ]
    # the angle gate is strict: a dot product of exactly +-aTh does not pass, the next float does
    frame = [(tilt(0.5), -0.875), (tilt(-0.5), -0.875), (tilt(half_up), -0.875), (tilt(-half_up), -0.9375)]
    for live in (True, False):
        cs.append(PlaneCase(f"angle-{'live' if live else 'dead'}", live, frame, [W0], [-1, -1, 0, 0], 2))
    return cs
