"""Hand-built inputs with known answers for the line window search, LSDmatcher::SearchByProjection mode 0 (cur, last) and mode 1
(F, MapLines): psl-slam_amd/csrc/pslfe_linematch.hip against oracle/linematch_oracle.cpp.  Pure numpy, nothing is run to obtain an
answer.  The pattern is tests/window_cases.py's: a case carries its inputs, `expected` / `assigned` / `nmatches` written down from
the construction, and `facts`, the regime it claims to reach, which tests/test_line_window_cases_cpu.py recomputes from
oracle_lib.line_grid_build and plain numpy.  tests/test_line_window_edges_gpu.py runs the same cases through the kernels.

Descriptors are window_cases' thermometer codes, so every Hamming distance is chosen.  The bounds are (0, 0, 1024, 768): a cell
is 16 x 16 px and 1 / 16 is exact in float32.  Unless a case says otherwise a candidate is a horizontal line 40 px long, its line
equation is (0, 1, -y), so its distance to a probe point (x, y') is y' - y exactly; queries carry th_cos = 0 (the 2-D angle gate
of GetFeaturesInAreaForLine lets everything through), v = (1, 0), length = 40 and wdir = (1, 0, 0), every line dir3d = (1, 0, 0):
all gates of the searches pass unless a case sets them.

facts (each recomputed by the CPU test; q = query index):
  grid_n           entries of the line grid                       max_cell   upper bound of the entries of one cell
  list[q]          the candidate list, in list order              ncand[q]   its length
  probe[q][line]   the probe point (0, 1, 2) that accepted line   gate[q][line]  "taken" | "dir" | "len" | "dir3d": what removed it
  best_second[q]   list positions of the best and the second best among the candidates left, (pos, -1) for a lone one
  lanes[q]         these positions % 64                            cells[line]  the grid cells the line occupies"""
import numpy as np

from window_cases import T, TT, owners

KEYLINE_DTYPE = np.dtype([("angle", "<f4"), ("class_id", "<i4"), ("octave", "<i4"), ("pt_x", "<f4"), ("pt_y", "<f4"),
                          ("response", "<f4"), ("size", "<f4"), ("startPointX", "<f4"), ("startPointY", "<f4"),
                          ("endPointX", "<f4"), ("endPointY", "<f4"), ("sPointInOctaveX", "<f4"),
                          ("sPointInOctaveY", "<f4"), ("ePointInOctaveX", "<f4"), ("ePointInOctaveY", "<f4"),
                          ("lineLength", "<f4"), ("numOfPixels", "<i4")])
LINEQUERY_DTYPE = np.dtype([("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("radius", "<f4"), ("th_cos", "<f4"),
                            ("vx", "<f4"), ("vy", "<f4"), ("length", "<f4"), ("blocks", "<i4"), ("wdir", "<f8", (3,))])
BOUNDS = (0.0, 0.0, 1024.0, 768.0)
CELL = 16.0
LINE_TH = 95            # add_src/LSDmatcher.cpp:205, :342
LINE_MAX, BATCH_MAX, SMALL_GRID, BIG_GRID = 2048, 1024, 8192, 65536   # PSL_LINE_MAX, PSL_LGD_MAXN, PSL_LGD_SMALL, PSL_LGD_BIG
F32, F64 = np.float32, np.float64
COS10, COS15 = np.cos(10.0 / 180.0 * np.pi), np.cos(15.0 / 180.0 * np.pi)


def keylines(segs, octave=0):
    """segs [n, 4] = (x1, y1, x2, y2) -> (KEYLINE_DTYPE[n] with every field filled from the segment, octave scale 1, and the
    normalised line equations [n, 3] float64, a x + b y + c = 0 through both end points).  A zero-length segment gets (0, 1, -y)."""
    s = np.asarray(segs, F32).reshape(-1, 4)
    n = len(s)
    k = np.zeros(n, KEYLINE_DTYPE)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    k["sPointInOctaveX"], k["sPointInOctaveY"], k["ePointInOctaveX"], k["ePointInOctaveY"] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    d = s.astype(F64)
    dx, dy = d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]
    length = np.hypot(dx, dy)
    k["lineLength"], k["numOfPixels"] = length, np.maximum(np.abs(dx), np.abs(dy)).astype(np.int32)
    k["pt_x"], k["pt_y"] = (d[:, 0] + d[:, 2]) / 2, (d[:, 1] + d[:, 3]) / 2
    k["angle"], k["size"], k["response"] = np.arctan2(dy, dx), np.abs(dx) * np.abs(dy), length / 1024.0
    k["octave"], k["class_id"] = octave, np.arange(n)
    a, b, c = -dy, dx, d[:, 0] * d[:, 3] - d[:, 2] * d[:, 1]
    nz = length > 0
    eq = np.zeros((n, 3))
    eq[nz] = np.stack([a[nz], b[nz], c[nz]], 1) / length[nz, None]
    eq[~nz] = np.stack([np.zeros((~nz).sum()), np.ones((~nz).sum()), -d[~nz, 1]], 1)
    return k, eq


def line_queries(segs, radius, blocks=1, v=(1.0, 0.0), length=40.0, wdir=(1.0, 0.0, 0.0), th_cos=0.0):
    s = np.asarray(segs, F32).reshape(-1, 4)
    q = np.zeros(len(s), LINEQUERY_DTYPE)
    q["x1"], q["y1"], q["x2"], q["y2"] = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    q["radius"], q["blocks"], q["th_cos"], q["length"] = radius, blocks, th_cos, length
    v = np.asarray(v, F32).reshape(-1, 2)
    q["vx"], q["vy"] = v[:, 0], v[:, 1]
    q["wdir"] = np.asarray(wdir, F64).reshape(-1, 3)
    return q


class Case:
    def __init__(self, name, mode, kls, eq, desc, q, qd, expected, facts, nnratio=0.95, dir3d=None, taken=None, assigned=None):
        self.name, self.mode, self.nnratio, self.bounds = name, mode, nnratio, BOUNDS
        self.kls, self.eq = kls, np.ascontiguousarray(eq, F64).reshape(-1, 3)
        self.desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.q, self.qd = q, np.ascontiguousarray(qd, np.uint8).reshape(-1, 32)
        n = len(kls)
        self.dir3d = np.tile(np.array([1.0, 0.0, 0.0]), (n, 1)) if dir3d is None else np.ascontiguousarray(dir3d, F64).reshape(-1, 3)
        self.taken, self.facts = taken, facts
        self.expected = self.assigned = self.nmatches = None   # a retargeted case has the oracle's answer alone
        if expected is not None:
            self.expected = np.asarray(expected, np.int32)
            self.assigned = owners(self.expected, n) if assigned is None else np.asarray(assigned, np.int32)
            self.nmatches = int((self.expected >= 0).sum())
            assert len(self.expected) == len(self.q)
        assert len(self.q) == len(self.qd) and len(self.desc) == n == len(self.eq) == len(self.dir3d)
        # no case is meant to walk long or to leave the surroundings of the image
        for f in ("startPointX", "endPointX"):
            assert n == 0 or (kls[f].min() >= -64 and kls[f].max() <= 1024 + 64)
        for f in ("startPointY", "endPointY"):
            assert n == 0 or (kls[f].min() >= -64 and kls[f].max() <= 768 + 64)
        assert len(q) == 0 or (min(q["x1"].min(), q["x2"].min(), q["y1"].min(), q["y2"].min()) >= -64
                               and max(q["x1"].max(), q["x2"].max()) <= 1088 and max(q["y1"].max(), q["y2"].max()) <= 832)

    def __repr__(self):
        return self.name

    def retarget(self, name, mode=None, nnratio=None, q=None, qd=None, taken=None):
        """the same lines under another mode / ratio / query order / mask: no written-down answer, the oracle's alone"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.name, c.expected, c.assigned, c.nmatches, c.facts = name, None, None, None, {}
        c.mode = self.mode if mode is None else mode
        c.nnratio = self.nnratio if nnratio is None else nnratio
        if q is not None:
            c.q, c.qd = q, qd
        if taken is not None:
            c.taken = taken
        return c


def run_oracle(case):
    """the sequential CPU oracle on a case -> (nmatches, match, assigned)"""
    import oracle_lib
    return oracle_lib.line_search_by_projection(case.kls, case.desc, case.eq, case.bounds, case.q, case.qd, case.mode,
                                                case.dir3d if case.mode == 1 else None, case.taken, case.nnratio)


def walk(x1, y1, x2, y2):
    """add_src/lineIterator.cpp:34-77 on the grid coordinates of a segment given in pixels (float32 x 1/16, exact) -> the in-grid
    cells in walking order.  Used for the sloped lines of grid_walk(); the axis-parallel and diagonal ones are written out."""
    x1, y1, x2, y2 = (F64(F32(t) * F32(1.0 / CELL)) for t in (x1, y1, x2, y2))
    steep = abs(y2 - y1) > abs(x2 - x1)
    if steep:
        x1, y1, x2, y2 = y1, x1, y2, x2
    if x1 > x2:
        x1, x2, y1, y2 = x2, x1, y2, y1
    dx, dy = x2 - x1, abs(y2 - y1)
    err, ystep, y = dx / 2.0, (1 if y1 < y2 else -1), int(y1)
    out = []
    for x in range(int(x1), int(x2) + 1):
        c = (y, x) if steep else (x, y)
        if 0 <= c[0] < 64 and 0 <= c[1] < 48:
            out.append(c)
        err -= dy
        if err < 0:
            y, err = y + ystep, err + dx
    return out


# ---- groups: independent clusters of lines, one query each -------------------------------------------------------------------------
class _Groups:
    """Group g lives at x0 = 100 + 96 g (at most 9 groups): its lines are horizontal, x0 .. x0 + 40, 0.5 px apart from y0 =
    16 row + 2, all in one cell row and listed in index order; its query is the horizontal segment (x0 + 10 .. x0 + 30, y0 + 4)
    with radius 6, so every probe point sees lines 0 .. 15 of the group and no line of another group."""

    def __init__(self, row=10):
        self.segs, self.oct, self.desc, self.d3, self.qsegs, self.qopt, self.expected, self.row = [], [], [], [], [], [], [], row
        self.facts = {"ncand": {}, "best_second": {}, "lanes": {}, "gate": {}}

    def add(self, lines, want, best_second=None, gate=None, **qopt):
        """lines: (distance, octave[, {"x1":, "dir3d":, "seg":}]) per line; want: the group's line that is matched, or -1"""
        g, base = len(self.qsegs), len(self.segs)
        assert g < 9 and len(lines) <= 16
        x0, y0 = 100.0 + 96 * g, CELL * self.row + 2
        for k, ln in enumerate(lines):
            o = ln[2] if len(ln) > 2 else {}
            self.segs.append(tuple(np.add(o["seg"], (x0, y0, x0, y0))) if "seg" in o else (x0, y0 + 0.5 * k, x0 + o.get("len", 40.0), y0 + 0.5 * k))
            self.oct.append(ln[1]); self.desc.append(T(ln[0])); self.d3.append(o.get("dir3d", (1.0, 0.0, 0.0)))
        self.qsegs.append((x0 + 10, y0 + 4, x0 + 30, y0 + 4))
        self.qopt.append(qopt)
        self.expected.append(base + want if want >= 0 else -1)
        self.facts["ncand"][g] = len(lines)
        if best_second is not None:
            self.facts["best_second"][g] = best_second
            self.facts["lanes"][g] = tuple(p % 64 if p >= 0 else -1 for p in best_second)
        if gate:
            self.facts["gate"][g] = {base + k: why for k, why in gate.items()}

    def case(self, name, mode, nnratio=0.95):
        kls, eq = keylines(self.segs, np.array(self.oct))
        q = line_queries(self.qsegs, 6.0)
        for g, o in enumerate(self.qopt):
            for k, v in o.items():
                if k == "v":
                    q["vx"][g], q["vy"][g] = v
                else:
                    q[k][g] = v
        return Case(name, mode, kls, eq, self.desc, q, [T(0)] * len(q), self.expected, self.facts, nnratio, dir3d=self.d3)


def ties(mode):
    """Equal distances.  Mode 0 keeps the first in list order (strict <, add_src/LSDmatcher.cpp:199-203).  Mode 1, nnratio 0.5 (a
    best of 20 or 30 against a second of 30 fails the ratio test, 20 > 15): the second best is the first of the equal ones to
    arrive, or the displaced best (:330-340), and the ratio test applies only if its octave is the best's."""
    G = _Groups()
    if mode == 0:
        G.add([(30, 0), (30, 0)], 0, (0, 1))
        G.add([(30, 0), (30, 0), (30, 0)], 0, (0, 1))
        G.add([(40, 0), (30, 0), (30, 0)], 1, (1, 2))
        return G.case("ties-mode0", 0)
    G.add([(30, 0), (30, 0)], -1, (0, 1))                 # best and second tie, one octave: 30 > 0.5f * 30
    G.add([(30, 0), (30, 1)], 0, (0, 1))                  # ... two octaves: no test
    G.add([(30, 0), (30, 0), (30, 1)], -1, (0, 1))        # three equal: the second is the second to arrive
    G.add([(20, 0), (30, 1), (30, 0)], 0, (0, 1))         # tie for second place: the first to arrive has octave 1: no test
    G.add([(20, 0), (30, 0), (30, 1)], -1, (0, 1))        # ... octave 0: refused
    G.add([(30, 0), (30, 1), (20, 1)], 2, (2, 0))         # the displaced best (octave 0) is the second, not the 30 of octave 1
    G.add([(30, 1), (30, 0), (20, 1)], -1, (2, 0))
    G.add([(30, 0), (25, 1), (25, 0)], 1, (1, 2))         # second = the later 25 (octave 0), the best has octave 1
    return G.case("ties-mode1", 1, 0.5)


def thresholds(mode, nnratio=0.75):
    """bestDist <= 95 accepts, 96 does not; mode 1's ratio test bestDist > nnratio * bestDist2 in float32 at equality (0.75f * 60.f
    == 45.f: 45 passes, 46 fails); a second best of another octave; a lone candidate; distance 256, which the reference's strict
    dist < bestDist2 with bestDist2 = 256 at the start never takes for the second best (add_src/LSDmatcher.cpp:296-345)."""
    G = _Groups()
    if mode == 0:
        G.add([(95, 0)], 0, (0, -1))
        G.add([(96, 0)], -1, (0, -1))
        G.add([(96, 0), (95, 0)], 1, (1, 0))
        G.add([(0, 0)], 0, (0, -1))
        G.add([(256, 0)], -1, (0, -1))
        G.add([(256, 0), (95, 0)], 1, (1, 0))
        return G.case("thresholds-mode0", 0)
    r = F32(nnratio)
    passes = lambda d1, d2: not (F32(d1) > r * F32(d2))   # the ratio test as the reference evaluates it
    if nnratio == 0.75:
        assert passes(45, 60) and not passes(46, 60) and r * F32(60) == F32(45)
        G.add([(45, 0), (60, 0)], 0, (0, 1))
        G.add([(46, 0), (60, 0)], -1, (0, 1))
        G.add([(60, 0), (45, 0)], 1, (1, 0))
        G.add([(50, 0), (60, 1)], 0, (0, 1))              # 50 > 45 fails the ratio, but the octaves differ
        G.add([(95, 0)], 0, (0, -1))
        G.add([(96, 0)], -1, (0, -1))
        G.add([(95, 0), (127, 0)], 0, (0, 1))             # 0.75f * 127 = 95.25
        G.add([(95, 0), (126, 0)], -1, (0, 1))            # 94.5
        G.add([(95, 0), (256, 0)], 0, (0, 1))
    else:
        # no second best at 256: a best of 95 / 90 is matched although 0.3f * 256 = 76.8 would refuse it
        assert nnratio != 0.3 or (not passes(95, 256) and not passes(90, 256) and not passes(80, 255) and passes(20, 255))
        G.add([(95, 0), (256, 0)], 0, (0, 1))
        G.add([(256, 0), (90, 0)], 1, (1, 0))             # a first-listed candidate at 256
        G.add([(256, 0)], -1, (0, -1))
        G.add([(256, 0), (256, 0)], -1, (0, 1))
        G.add([(80, 0), (255, 0)], -1 if nnratio == 0.3 else 0, (0, 1))
        G.add([(20, 0), (255, 0)], 0, (0, 1))
        G.add([(90, 0), (256, 0), (256, 1)], 0, (0, 1))
    return G.case(f"thresholds-mode1-{nnratio}", 1, nnratio)


def mode0_gates():
    """The length ratio min / max < 0.75 in float32 -> double (:190-195) and the 10 degree direction gate on the in-octave vectors
    (:178-184), which apply before the distance counts."""
    G = _Groups()
    below = np.nextafter(F32(30.0), F32(0.0))
    assert F64(F32(30.0) / F32(40.0)) == 0.75 and F64(below / F32(40.0)) < 0.75
    G.add([(10, 0)], 0, (0, -1), length=30.0)                                    # 30 / 40 == 0.75 passes
    G.add([(10, 0)], -1, (-1, -1), gate={0: "len"}, length=below)
    G.add([(0, 0, {"len": 28.0}), (50, 0)], 1, (1, -1), gate={0: "len"})          # a gated line at distance 0 must not win
    deg = lambda a: (np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a)))
    G.add([(10, 0)], 0, (0, -1), v=deg(8.0))
    G.add([(10, 0)], -1, (-1, -1), gate={0: "dir"}, v=deg(12.0))
    G.add([(10, 0)], 0, (0, -1), v=deg(188.0))                                   # anti-parallel: fabs
    G.add([(10, 0)], -1, (-1, -1), gate={0: "dir"}, v=deg(168.0))
    # a line 14 degrees off the query's v, at distance 0, next to a parallel one at 50
    G.add([(0, 0, {"seg": (0.0, 0.0, 40.0, 10.0)}), (50, 0, {"seg": (0.0, 6.0, 40.0, 6.0)})], 1, (1, -1), gate={0: "dir"})
    return G.case("gates-mode0", 0)


def mode1_gate():
    """the 15 degree gate on the 3-D directions, in float32 after a double dot product (:305-313)"""
    G = _Groups()
    off = (np.cos(np.deg2rad(16.0)), np.sin(np.deg2rad(16.0)), 0.0)
    G.add([(10, 0, {"dir3d": (2.0, 0.0, 0.0)})], 0, (0, -1))
    G.add([(10, 0, {"dir3d": (-1.0, 0.0, 0.0)})], 0, (0, -1))
    G.add([(10, 0, {"dir3d": off})], -1, (-1, -1), gate={0: "dir3d"})
    G.add([(0, 0, {"dir3d": off}), (50, 0)], 1, (1, -1), gate={0: "dir3d"})
    G.add([(0, 0, {"dir3d": (np.cos(np.deg2rad(14.0)), 0.0, -np.sin(np.deg2rad(14.0)))}), (50, 0)], 0, (0, 1))
    return G.case("gate-mode1", 1, 0.95)


# ---- the best and the second best in one wave lane ---------------------------------------------------------------------------------
def _stack140():
    """140 horizontal lines 0.5 px apart, y = 160 .. 229.5 (cell rows 10 .. 14), x 100 .. 140.  The line at list position p has y =
    160 + p / 2; the rows' index blocks are reversed (row 14 holds lines 0 .. 11, row 10 lines 108 .. 139), so a list position is
    never the line's index.  -> (segments by index, index of list position)"""
    sizes = [32, 32, 32, 32, 12]
    first = {b: sum(sizes[b + 1:]) for b in range(5)}
    idx_of_pos = np.array([first[p // 32] + p % 32 for p in range(140)])
    segs = np.zeros((140, 4), F32)
    for p in range(140):
        segs[idx_of_pos[p]] = (100.0, 160.0 + 0.5 * p, 140.0, 160.0 + 0.5 * p)
    return segs, idx_of_pos


def same_lane(mode, order="3-67-131", nnratio=0.6, second_octave=0):
    """A window of 140 candidates (radius 40 around y = 195): the three smallest distances 20, 30, 40 sit at list positions 3, 67,
    131 (order "3-67-131") or 67, 3, 131 ("67-3-131"), all in lane 3 of the wave that evaluates the list; everything else is at
    120.  Mode 0: three identical blocking queries take them one after the other, a fourth finds nothing within 95.  Mode 1, one
    query: with the second best in the best's octave 0, nnratio 0.6 refuses (20 > 18; the third, 40, would let it pass); with
    the second best in octave 1 and the third in octave 0, nnratio 0.4 accepts (no test; the third would refuse, 20 > 16)."""
    segs, idx_of_pos = _stack140()
    pos = {"3-67-131": (3, 67, 131), "67-3-131": (67, 3, 131)}[order]
    dist = np.full(140, 120)
    octave = np.zeros(140, np.int32)
    for p, d in zip(pos, (20, 30, 40)):
        dist[idx_of_pos[p]] = d
    octave[idx_of_pos[pos[1]]] = second_octave
    kls, eq = keylines(segs, octave)
    desc = [T(d) for d in dist]
    nq = 4 if mode == 0 else 1
    q = line_queries([(110.0, 195.0, 130.0, 195.0)] * nq, 40.0)
    L = idx_of_pos.tolist()
    if mode == 0:
        expected = [idx_of_pos[p] for p in pos] + [-1]
        facts = {"grid_n": 140 * 3, "ncand": {i: 140 for i in range(4)}, "list": {0: L},
                 "best_second": {0: (pos[0], pos[1]), 1: (pos[1], pos[2])}, "lanes": {0: (3, 3), 1: (3, 3)},
                 "gate": {1: {idx_of_pos[pos[0]]: "taken"}}}
    else:
        refused = second_octave == 0 and F32(20) > F32(nnratio) * F32(30)
        assert refused == (nnratio == 0.6) and (second_octave == 0 or F32(20) > F32(nnratio) * F32(40))
        expected = [-1 if refused else idx_of_pos[pos[0]]]
        facts = {"ncand": {0: 140}, "list": {0: L}, "best_second": {0: (pos[0], pos[1])}, "lanes": {0: (3, 3)}}
    return Case(f"same-lane-mode{mode}-{order}-{nnratio}-oct{second_octave}", mode, kls, eq, desc, q, [T(0)] * nq, expected, facts, nnratio)


# ---- the three probe points ----------------------------------------------------------------------------------------------------------
def probe_order(mode):
    """GetFeaturesInAreaForLine's list (src/Frame.cc:752-826) in probe -> column -> row -> cell order.
      q0  (110, 100) -> (130, 120), r 4: line 0 (y 122) lies in the first probe's cells (rows 6 .. 7) but 22 and 12 px from the first
          two probe points; the third accepts it, behind lines 1 (y 101) and 2 (y 99) that the first accepted.  Lines 0 and 2
          tie at distance 30, line 1 has 40: the earlier list position wins, line 2, not the lower index.
      q1  horizontal through y 100, r 4: lines 1 and 2 at all three probe points, each listed once.  In mode 1 both have octave 0
          and the distances 40 / 30 fail nnratio 0.5 ... but a line listed twice would fail it with any two octaves.
      q2  line 3 alone (y 300, distance 20), seen three times, listed once: matched; listed twice it would be its own second best.
      q3  (1000, 20) -> (1060, 32), r 8: the third probe's minCX is 65: skipped; line 4 (y 21) comes from the first, line 5 (y 30,
          x 1010 .. 1023) is 10 px from the first and accepted by the mid-point.
      q4  (100, -30) -> (100, 30), r 8: the first probe's maxCY is -1: skipped; line 6 (y 3) from the mid-point, line 7 (y 27) from
          the last.
      q5  radius 0 on line 3: |dist| < 0 never holds.
      q6  radius 1100: every cell; all 9 lines are candidates in column-major cell order, line 8 (x 40, the first column) first."""
    segs = [(100, 122, 140, 122), (100, 101, 140, 101), (100, 99, 140, 99), (300, 300, 340, 300), (960, 21, 1000, 21),
            (1010, 30, 1023, 30), (80, 3, 120, 3), (80, 27, 120, 27), (40, 700, 80, 700)]
    dist = [30, 40, 30, 20, 10, 12, 14, 16, 5]
    octave = [0, 0, 0, 0, 0, 1, 0, 1, 1]
    kls, eq = keylines(segs, np.array(octave))
    qs = [(110, 100, 130, 120), (110, 100, 130, 100), (310, 300, 330, 300), (1000, 20, 1060, 32), (100, -30, 100, 30),
          (310, 300, 330, 300), (500, 400, 540, 400)]
    q = line_queries(qs, [4.0, 4.0, 4.0, 8.0, 8.0, 0.0, 1100.0], blocks=0)
    q["length"][3] = 17.0     # mode 0's length gate at q3: line 5 (13 px) passes, 13 / 17; line 4 (40 px) fails, 17 / 40
    facts = {"ncand": {0: 3, 1: 2, 2: 1, 3: 2, 4: 2, 5: 0, 6: 9},
             "list": {0: [1, 2, 0], 1: [1, 2], 2: [3], 3: [4, 5], 4: [6, 7], 5: [], 6: [8, 6, 7, 1, 2, 0, 3, 4, 5]},
             "probe": {0: {1: 0, 2: 0, 0: 2}, 1: {1: 0, 2: 0}, 2: {3: 0}, 3: {4: 0, 5: 1}, 4: {6: 1, 7: 2}},
             "best_second": {0: (1, 2), 2: (0, -1)}, "lanes": {0: (1, 2), 2: (0, -1)}}
    if mode == 0:
        # q3: line 4 fails the length gate (17 / 40), line 5 passes (13 / 17 = 0.76); q6: length 40 gates line 5 (13 / 40)
        expected = [2, 2, 3, 5, 6, -1, 8]
        facts["gate"] = {3: {4: "len"}, 6: {5: "len"}}
        nnratio = 0.95
    else:
        # nnratio 0.5.  q0: best line 2 (30), second line 0 (30), one octave: refused.  q1: line 2 (30) against line 1 (40): refused.
        # q2: lone.  q3: 10 against 12 in octaves 0 / 1.  q4: 14 / 16, octaves 0 / 1.  q6: line 8 (5, octave 1) against line 4 (10, octave 0).
        expected = [-1, -1, 3, 4, 6, -1, 8]
        nnratio = 0.5
    return Case(f"probe-order-mode{mode}", mode, kls, eq, [T(d) for d in dist], q, [T(0)] * len(q), expected, facts, nnratio)


# ---- blocking ----------------------------------------------------------------------------------------------------------------------
def blocking(mode):
    """Four lines at distances 10, 20, 30, 40 (octaves alternate: no ratio test), line 0 `taken`.  q0 blocks line 1; q1 and q2 do not
    block and both take line 2; q3 blocks line 2 (`assigned` holds the last query); q4 takes line 3; q5 finds nothing."""
    G = _Groups()
    G.add([(10, 0), (20, 1), (30, 0), (40, 1)], 0)
    c = G.case("x", mode)
    q = np.repeat(c.q, 6)
    q["blocks"] = [1, 0, 0, 1, 1, 1]
    facts = {"ncand": {i: 4 for i in range(6)}, "gate": {0: {0: "taken"}, 1: {0: "taken", 1: "taken"}, 4: {0: "taken", 1: "taken", 2: "taken"}},
             "best_second": {0: (1, 2), 1: (2, 3), 2: (2, 3), 3: (2, 3), 4: (3, -1), 5: (-1, -1)}}
    return Case(f"blocking-mode{mode}", mode, c.kls, c.eq, c.desc, q, [T(0)] * 6, [1, 2, 2, 2, 3, -1], facts, 0.95,
                taken=np.array([1, 0, 0, 0], np.uint8), assigned=[-1, 0, 3, 4])


def chain(mode, L=64):
    """L + 1 lines 2 px apart (y = 100 + 2 j); query j (y = 99 + 2 j, radius 1.5) reaches lines j - 1 and j and carries line j - 1's
    descriptor: everybody but query 0 is pushed to the second choice, at distance 20, by the query before."""
    kls, eq = keylines([(100.0, 100.0 + 2 * j, 140.0, 100.0 + 2 * j) for j in range(L + 1)], np.arange(L + 1) % 2)
    desc = [T(20 * (j % 3)) for j in range(L + 1)]
    q = line_queries([(110.0, 99.0 + 2 * j, 130.0, 99.0 + 2 * j) for j in range(L)], 1.5)
    qd = [T(20 * ((j - 1) % 3)) for j in range(L)]
    facts = {"ncand": {0: 1, 1: 2, L - 1: 2}, "gate": {j: {j - 1: "taken"} for j in (1, L // 2, L - 1)},
             "best_second": {0: (0, -1), 1: (1, -1), L - 1: (1, -1)}}
    return Case(f"chain-mode{mode}-L{L}", mode, kls, eq, desc, q, qd, np.arange(L), facts, 0.95)


# ---- the Bresenham walk of AssignFeaturesToGridForLine -----------------------------------------------------------------------------------
def grid_walk(mode=0):
    """One line per shape, the cells written down from lineIterator.cpp's rule (grid coordinates = px / 16; the start is truncated,
    the walk runs over the longer axis from the smaller to the larger coordinate up to the truncated end, inclusive; cells outside
    64 x 48 are dropped).  The sloped ones (10 .. 13) come from walk() above.  Queries sit on four of the lines."""
    cols = lambda a, b, y: [(x, y) for x in range(a, b + 1)]
    rows = lambda x, a, b: [(x, y) for y in range(a, b + 1)]
    spec = [((32, 40, 100, 40), cols(2, 6, 2)),                      # 0 horizontal
            ((40, 32, 40, 100), rows(2, 2, 6)),                      # 1 vertical
            ((160, 160, 224, 224), [(c, c) for c in range(10, 15)]),  # 2 exactly diagonal: |dy| > |dx| is false, walks x
            ((100, 72, 32, 72), cols(2, 6, 4)),                      # 3 start right of end: swapped
            ((320, 320, 384, 320), cols(20, 24, 20)),                # 4 end points on cell boundaries: cell 24 is entered
            ((500, 300, 500, 300), [(31, 18)]),                      # 5 zero length: one cell
            ((-8, 200, 40, 200), cols(0, 2, 12)),                    # 6 x = -0.5 truncates to cell 0
            ((-40, 232, 40, 232), cols(0, 2, 14)),                   # 7 cells -2 and -1 dropped
            ((1000, 100, 1040, 100), cols(62, 63, 6)),               # 8 ends in column 65
            ((100, 750, 100, 784), rows(6, 46, 47)),                 # 9 ends in row 49
            ((200, 400, 330, 440), None),                            # 10 shallow
            ((600, 100, 640, 250), None),                            # 11 steep
            ((700, 500, 620, 460), None),                            # 12 shallow, right to left
            ((900, 300, 880, 180), None),                            # 13 steep, bottom to top
            ((224, 160, 160, 224), [(10, 14), (11, 13), (12, 12), (13, 11), (14, 10)])]   # 14 anti-diagonal, swapped: y steps down
    segs = [s for s, _ in spec]
    cells = {i: (c if c is not None else walk(*s)) for i, (s, c) in enumerate(spec)}
    assert len(cells[10]) == 9 and len(cells[11]) == 10 and cells[12][0] == (38, 28) and cells[13][0] == (55, 11)
    kls, eq = keylines(segs, 0)
    desc = [TT(2 * i, 4) for i in range(len(segs))]
    on = [0, 4, 10, 12]
    q = line_queries([segs[i] for i in on], 3.0, v=[(segs[i][2] - segs[i][0], segs[i][3] - segs[i][1]) for i in on],
                     length=[float(kls["lineLength"][i]) for i in on],
                     wdir=[(1.0, 0.0, 0.0)] * len(on))
    facts = {"cells": cells, "grid_n": sum(len(c) for c in cells.values())}
    return Case(f"grid-walk-mode{mode}", mode, kls, eq, desc, q, [desc[i] for i in on], on, facts, 0.95)


# ---- capacity ----------------------------------------------------------------------------------------------------------------------
def capacity_one_frame(mode, n=LINE_MAX):
    """PSL_LINE_MAX lines of 40 px in 16 column groups 60 px apart and 128 rows 5.9 px apart: a cell holds at most 4.  Query k sits on
    line n - 1 - k with its descriptor (distance 0 is unique: TT codes differ by 2 or more); radius 8 also lists the lines 5.9 px
    above and below."""
    i = np.arange(n)
    x0, y = 20.0 + 60.0 * (i % 16), 5.0 + 5.9 * (i // 16)
    kls, eq = keylines(np.stack([x0, y, x0 + 40.0, y], 1), i % 3)
    desc = np.array([TT(2 * (k % 64), 2 * (k // 64)) for k in range(n)], np.uint8)
    target = n - 1 - i
    q = line_queries(np.stack([x0[target] + 10, y[target], x0[target] + 20, y[target]], 1), 8.0)   # stays clear of the next group's cells
    facts = {"max_cell": 4, "ncand": {0: 2, 1: 2, 100: 3, n - 1: 2}}
    return Case(f"capacity-one-frame-mode{mode}-n{n}", mode, kls, eq, desc, q, desc[target], target, facts, 0.95)


def capacity_batched(mode, entries):
    """Full-width lines x = 0.5 .. 1023.5, 0.7 px apart from y = 3: 64 grid entries each, at most 23 in a cell.  128 lines make
    8192 entries (PSL_LGD_SMALL, the first launch's grid), 1024 lines 65536 (the second launch's); 8191: the last line ends at
    x = 1007.5 (63 cells); 8193: a 129th line of one cell.  16 queries sit on lines spread over the frame, radius 1 (the
    neighbours 0.7 px away are listed too), with the line's descriptor."""
    n = {8191: 128, 8192: 128, 8193: 129, 65536: 1024}[entries]
    y = (3.0 + 0.7 * np.arange(n)).astype(F32)
    segs = np.stack([np.full(n, 0.5, F32), y, np.full(n, 1023.5, F32), y], 1)
    if entries == 8191:
        segs[-1, 2] = 1007.5
    if entries == 8193:
        segs[-1, 2] = 8.0
    kls, eq = keylines(segs, np.arange(n) % 2)
    desc = np.array([TT(2 * (k % 64), 2 * (k // 64)) for k in range(n)], np.uint8)
    target = (np.arange(16) * (n - 3) // 15 + 1)[::-1].copy()
    x = 100.0 + 50.0 * np.arange(16)
    q = line_queries(np.stack([x, y[target], x + 40.0, y[target]], 1), 1.0, length=float(kls["lineLength"][0]))
    facts = {"grid_n": entries, "max_cell": 23, "ncand": {15: 3}}
    return Case(f"capacity-batched-mode{mode}-{entries}", mode, kls, eq, desc, q, desc[target], target, facts, 0.95)


def overflow_pair(mode, p):
    """pair p of the second batched launch: 129 + p % 8 full-width lines (more than 8192 entries), descriptors and queries of its own"""
    rng = np.random.default_rng(1000 + p)
    n = 129 + p % 8
    y = (3.0 + 0.7 * np.arange(n) + 5.0 * (p % 90)).astype(F32)
    segs = np.stack([np.full(n, 0.5, F32), y, np.full(n, 1023.5, F32), y], 1)
    kls, eq = keylines(segs, rng.integers(0, 2, n))
    desc = np.array([TT(int(a), int(b)) for a, b in rng.integers(0, 60, (n, 2))], np.uint8)
    target = rng.integers(0, n, 8)
    x = 50.0 + 100.0 * np.arange(8)
    q = line_queries(np.stack([x, y[target], x + 40.0, y[target]], 1), 2.0, blocks=rng.integers(0, 2, 8), length=float(kls["lineLength"][0]))
    qd = desc[target].copy()
    taken = (rng.random(n) < 0.1).astype(np.uint8)
    return Case(f"overflow-mode{mode}-{p}", mode, kls, eq, desc, q, qd, None, {}, 0.8, taken=taken)


# ---- the lists the tests walk --------------------------------------------------------------------------------------------------------
def host_cases():
    cs = []
    for mode in (0, 1):
        cs += [ties(mode), probe_order(mode), blocking(mode), chain(mode), grid_walk(mode), capacity_one_frame(mode)]
        cs += [capacity_batched(mode, e) for e in (8191, 8192, 8193, 65536)]
    cs += [thresholds(0), thresholds(1, 0.75), thresholds(1, 0.3), thresholds(1, 0.95), mode0_gates(), mode1_gate()]
    cs += [same_lane(0, "3-67-131"), same_lane(0, "67-3-131")]
    for order in ("3-67-131", "67-3-131"):
        cs += [same_lane(1, order, 0.6, 0), same_lane(1, order, 0.75, 0), same_lane(1, order, 0.4, 1)]
    return cs


def grid_cases():
    """the cases whose grid the host form is asked for"""
    return [grid_walk(0), capacity_one_frame(0)] + [capacity_batched(0, e) for e in (8191, 8192, 8193, 65536)]


def device_cases(mode):
    """the small cases of one batched launch (at most PSL_LGD_MAXN lines and 64 queries); the capacity pairs come on top"""
    cs = [c for c in host_cases() if c.mode == mode and len(c.kls) <= BATCH_MAX and len(c.q) <= 64 and not c.name.startswith("capacity")]
    return cs
