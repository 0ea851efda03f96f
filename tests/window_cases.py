"""Hand-built inputs with known answers for the ORB window searches (SearchByProjection(cur,last), SearchByProjection(F,MapPoints),
SearchByProjection(cur,KF), SearchByBoW).  Pure numpy: no images, no extractor, nothing is run to obtain an answer.

Descriptors are thermometer codes, T(a) = the first a bits set, so hamming(T(a), T(b)) == |a - b| and every distance in a case is
chosen.  A case carries its inputs, the function it is meant for (`fn`), `expected` (the match table written down from the
construction) and `facts` (the regime it claims to reach, as numbers that tests/test_window_cases_cpu.py recomputes from
oracle_lib.grid_build and plain numpy).  tests/test_window_edges_gpu.py runs the same cases through the kernels.

The image bounds are (0, 0, 1024, 768): a grid cell is 16 x 16 pixels and 1 / 16 is exact in float32, so the cell of a keypoint
and the cell range of a window follow from the construction without rounding (PosInGrid: cell = round(x / 16), halves away from
zero; GetFeaturesInArea: cells floor((u - r) / 16) .. ceil((u + r) / 16), visited column by column, a cell in ascending index).

Other searches that use the shared matcher primitives (pslfe_kf, pslfe_mono, pslfe_loop, pslfe_stereo) can take the same arrays:
a case is just (kps, desc, uright, bounds, q, qd, taken); tests/kf_cases.py does so for pslfe_kf."""
import numpy as np

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
PROJQUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("ur", "<f4"), ("min_level", "<i4"),
                            ("max_level", "<i4"), ("angle", "<f4"), ("blocks", "<i4")])
BOUNDS = (0.0, 0.0, 1024.0, 768.0)
CELL = 16.0
TH_HIGH, TH_LOW, HISTO_LENGTH, TOPK = 100, 50, 30, 8   # src/ORBmatcher.cc:37-39; the kernels' cached list (PSL_TOPK)
F32 = np.float32


def T(a, bits=256, offset=0):
    """thermometer code: bits offset .. offset + a - 1 set"""
    b = np.zeros(256, np.uint8)
    assert 0 <= a <= bits and offset + bits <= 256
    b[offset:offset + a] = 1
    return np.packbits(b, bitorder="little")


def TT(a, b):
    """two thermometers of 128 bits side by side: hamming(TT(a, b), TT(c, d)) == |a - c| + |b - d|"""
    return T(a, 128, 0) | T(b, 128, 128)


def keypoints(xy, octave=0, angle=0.0):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k["x"], k["y"], k["size"], k["octave"], k["angle"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, octave, angle, -1
    return k


def queries(uv, radius, blocks=1, min_level=-1, max_level=-1, angle=0.0, ur=0.0):
    q = np.zeros(len(uv), PROJQUERY_DTYPE)
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    q["u"], q["v"], q["radius"], q["blocks"] = uv[:, 0], uv[:, 1], radius, blocks
    q["min_level"], q["max_level"], q["angle"], q["ur"] = min_level, max_level, angle, ur
    return q


def owners(chosen, n, filtered=None):
    """`assigned`: the last query that chose a keypoint; -1 once a choice of that keypoint was filtered by the rotation check
    (src/ORBmatcher.cc:1456-1466 clears mvpMapPoints[idx] whoever holds it by then)."""
    a = np.full(n, -1, np.int32)
    for i, c in enumerate(chosen):
        if c >= 0:
            a[c] = i
    if filtered is not None:
        for i, c in enumerate(chosen):
            if c >= 0 and filtered[i]:
                a[c] = -1
    return a


class Case:
    """fn: "last" | "map" | "kf" | "bow".  opts: check_ori, nnratio, orb_dist; for "bow" also fidx, runs, qangle."""

    def __init__(self, name, fn, kps, desc, q, qd, expected, facts, uright=None, taken=None, assigned=None, **opts):
        self.name, self.fn, self.bounds = name, fn, BOUNDS
        self.kps, self.desc = kps, np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        self.q, self.qd = q, np.ascontiguousarray(qd, np.uint8).reshape(-1, 32)
        self.uright, self.taken, self.opts, self.facts = uright, taken, opts, facts
        self.expected = self.assigned = self.nmatches = None   # a case retargeted to another function has the oracle's answer alone
        if expected is not None:
            self.expected = np.asarray(expected, np.int32)
            self.assigned = owners(self.expected, len(kps)) if assigned is None else np.asarray(assigned, np.int32)
            self.nmatches = int((self.expected >= 0).sum())
            assert len(self.expected) == len(self.qd)
        assert len(self.q) == len(self.qd) and len(self.desc) == len(kps)

    def __repr__(self):
        return self.name

    def with_opts(self, name=None, **opts):
        """the same inputs and answer under other options (the caller knows that the answer does not depend on them)"""
        c = Case.__new__(Case)
        c.__dict__.update(self.__dict__)
        c.opts = dict(self.opts, **opts)
        c.name = name or self.name + "".join(f"-{k}={v}" for k, v in opts.items())
        return c

    def retarget(self, fn, taken=None, **opts):
        """the same inputs for another function: no written-down answer, the oracle's alone (the batched launches)"""
        c = self.with_opts(self.name + "-as-" + fn, **opts)
        c.fn, c.expected, c.assigned, c.nmatches, c.facts = fn, None, None, None, {}
        if taken is not None:
            c.taken = taken
        return c


def run_oracle(case):
    """the sequential CPU oracle on a case -> (nmatches, match, assigned)"""
    import oracle_lib
    o = case.opts
    if case.fn == "last":
        return oracle_lib.search_by_projection_last(case.kps, case.desc, case.uright, case.bounds, case.q, case.qd, case.taken,
                                                    o.get("check_ori", False))
    if case.fn == "map":
        return oracle_lib.search_by_projection_map(case.kps, case.desc, case.uright, case.bounds, case.q, case.qd, case.taken,
                                                   o["nnratio"])
    if case.fn == "kf":
        return oracle_lib.search_by_projection_kf(case.kps, case.desc, case.bounds, case.q, case.qd, case.taken, o["orb_dist"],
                                                  o.get("check_ori", False))
    return oracle_lib.search_by_bow(case.desc, case.kps["angle"], o["fidx"], o["runs"], case.qd, o["qangle"], o["nnratio"],
                                    o.get("check_ori", False))


# ---- a. chain ----------------------------------------------------------------------------------------------------------------
def chain(L=300, fn="last", blocks=1):
    """L keypoints 2 px apart on one row; query j reaches keypoints j - 1 and j (radius 1.5 around the midpoint) and its
    descriptor is keypoint j - 1's.  Query 0 has keypoint 0 alone.  Blocking: query j finds j - 1 taken and keeps j, which query
    j + 1 learns only after query j has moved: the fixpoint needs about L iterations.  Not blocking: everybody keeps j - 1."""
    kps = keypoints([(100.0 + 2 * j, 100.0) for j in range(L)], octave=np.arange(L) % 2)   # octaves alternate: no ratio test in "map"
    desc = [T(20 * (j % 3)) for j in range(L)]
    q = queries([(99.0 + 2 * j, 100.0) for j in range(L)], 1.5, blocks)
    qd = [T(20 * ((j - 1) % 3)) for j in range(L)]
    expected = np.arange(L) if blocks else np.maximum(np.arange(L) - 1, 0)
    facts = {"depth": L if blocks else 1, "gated_max": 2}
    opts = {"nnratio": 0.8} if fn == "map" else {"orb_dist": 100} if fn == "kf" else {}
    return Case(f"chain-{fn}-L{L}-blocks{blocks}", fn, kps, desc, q, qd, expected, facts, **opts)


# ---- b. exhausted_list -------------------------------------------------------------------------------------------------------
def exhausted_list(fn="last", octaves="equal", orb_dist=100):
    """12 keypoints T(10 i) in one cell; queries 0..7 carry T(10 i) and own keypoints 0..7, queries 8..11 carry T(0): their 8
    cached candidates are taken and the window holds 4 more, at distances 80, 90, 100, 110."""
    oct_ = np.zeros(12, np.int32) if octaves == "equal" else np.arange(12) % 2
    kps = keypoints([(200.0 + 0.25 * i, 200.0) for i in range(12)], octave=oct_)
    desc = [T(10 * i) for i in range(12)]
    q = queries([(201.5, 200.0)] * 12, 10.0)
    qd = [T(10 * i) for i in range(8)] + [T(0)] * 4
    opts = {}
    if fn == "last" or (fn == "map" and octaves == "alternating"):
        expected = list(range(11)) + [-1]          # 100 <= TH_HIGH is accepted, 110 is not
    elif fn == "map":
        expected = list(range(8)) + [-1] * 4       # 80 > 0.8f * 90: the ratio test rejects, keypoint 8 stays free and so on
    else:
        expected = [i if 10 * i <= orb_dist or i < 8 else -1 for i in range(12)]
        opts["orb_dist"] = orb_dist
    if fn == "map":
        opts["nnratio"] = 0.8
    uright = np.full(12, 5000.0, np.float32) if fn == "kf" else None   # would reject everything if "kf" had the stereo gate
    return Case(f"exhausted-{fn}-{octaves}" + (f"-orb{orb_dist}" if fn == "kf" else ""), fn, kps, desc, q, qd, expected,
                {"one_cell": 12, "window_T": 12, "gated_max": 12, "list_exhausted": 4}, uright=uright, **opts)


# ---- c. pile_up --------------------------------------------------------------------------------------------------------------
def pile_up(fn="last", octaves="equal", nk=150, step=1, pad=0):
    """nk keypoints T(step j) on a 15-wide lattice of 1 px inside one window, nk identical blocking queries T(0): query i takes
    keypoint i while step * i <= TH_HIGH.  Every query after the eighth finds its whole cached list taken, on every iteration.
    `pad` queries whose windows lie wholly outside the image come first, so that the contended queries are rows r = 1, 2, 3 of
    the resolving threads (query index >= 1024, 2048, 3072)."""
    oct_ = np.zeros(nk, np.int32) if octaves == "equal" else np.arange(nk) % 2
    kps = keypoints([(300.0 + j % 15, 300.0 + j // 15) for j in range(nk)], octave=oct_)
    desc = [T(step * j) for j in range(nk)]
    outside = [(-500.0, 300.0), (1600.0, 300.0), (300.0, -500.0), (300.0, 1400.0)]
    q = queries([outside[i % 4] for i in range(pad)] + [(307.0, 300.0 + nk // 30)] * nk, 20.0)
    qd = [T(3)] * pad + [T(0)] * nk
    if fn == "map" and octaves == "equal":
        assert step == 1
        good = np.arange(nk) <= 4                  # i > 0.8f * (i + 1) first at i = 5 (4 > 0.8f * 5 == 4.0f is false)
        opts = {"nnratio": 0.8}
    else:
        good = step * np.arange(nk) <= TH_HIGH
        opts = {"nnratio": 0.8} if fn == "map" else {}
    expected = np.concatenate([np.full(pad, -1), np.where(good, np.arange(nk), -1)])
    # queries whose cached 8 best (keypoints 0..7) hold fewer free ones than the decision needs (one; two in "map")
    slow = nk - TOPK if fn != "map" else 0 if octaves == "equal" else nk - TOPK + 1
    facts = {"window_T": nk, "gated_max": nk, "list_exhausted": slow, "first_contended_query": pad}
    return Case(f"pile-{fn}-{octaves}-nk{nk}-step{step}-pad{pad}", fn, kps, desc, q, qd, expected, facts, **opts)


# ---- d. ties -----------------------------------------------------------------------------------------------------------------
def _visit_order(cx, cy):
    """GetFeaturesInArea's order: cell column, cell row, index"""
    return np.lexsort((np.arange(len(cx)), cy, cx))


def ties(fn="last", orb_dist=100, n=100, cells=5, near=40):
    """n keypoints scattered over cells x cells grid cells (seeded; the index order is unrelated to the cell order).  The last
    `near` keypoints in visiting order all carry T(7), the others T(70): for a query T(0) the 8 cached candidates are a tie that
    straddles the 64-candidate rounds of the wide pass (visiting ranks n - near .. n - near + 7).  n + 4 identical blocking
    queries take the keypoints in visiting order: the T(7) ones first, then the T(70) ones, then nothing is left."""
    rng = np.random.default_rng(12)
    cx, cy = rng.integers(20, 20 + cells, n), rng.integers(20, 20 + cells, n)
    # inside its cell: cell * 16 + (-6 .. 6)
    kps = keypoints(np.stack([cx * CELL + rng.integers(-6, 7, n), cy * CELL + rng.integers(-6, 7, n)], 1))
    order = _visit_order(cx, cy)
    kps["octave"][order] = np.arange(n) % 2      # "map": the best and the next in visiting order never share an octave: no ratio test
    desc = np.zeros((n, 32), np.uint8)
    desc[order[:n - near]] = T(70)
    desc[order[n - near:]] = T(7)
    c = (20 + cells / 2.0) * CELL - 8.0
    q = queries([(c, c)] * (n + 4), cells * CELL)
    qd = [T(0)] * (n + 4)
    seq = np.concatenate([order[n - near:], order[:n - near]])
    opts, uright = {"nnratio": 0.8} if fn == "map" else {}, None
    if fn == "kf":
        opts["orb_dist"] = orb_dist
        uright = np.full(n, 5000.0, np.float32)
        if orb_dist < 70:
            seq = seq[:near]
    expected = np.concatenate([seq, np.full(n + 4 - len(seq), -1)])
    facts = {"window_T": n, "gated_max": n, "list_exhausted": n + 4 - TOPK + (fn == "map"), "tie_ranks": (n - near, n - 1)}
    return Case(f"ties-{fn}-n{n}" + (f"-orb{orb_dist}" if fn == "kf" else ""), fn, kps, desc, q, qd, expected, facts,
                uright=uright, **opts)


def ties_map(d=5, b=3, nnratio=0.5):
    """SearchByProjection(F, MapPoints): which candidate is the second best when distances are equal (src/ORBmatcher.cc:97-110:
    strict <, and a displaced best hands its level to the second).  Octaves o1, o2, o3 below are the literal values; b < d and
    b > nnratio * d, so a best of distance b is refused exactly when the second (distance d) has its octave.
      group 0: d/1, d/2, b/1 in this order of arrival: second = the first d (octave 1) = the best's octave -> refused
      group 1: d/1, b/2, d/2: second = the first d (octave 1), the best has octave 2 -> keypoint 1 of the group
      group 2: d/1, d/2: best = the first, second has another octave -> keypoint 0 of the group
      group 3: d/1, d/1: best = the first, d > nnratio * d -> refused
      group 4: over two cells: Y = d/2 with the higher index sits in the earlier cell, X = d/1 and Z = b/1 in the later one: arrival
               Y, X, Z: second = Y (octave 2) -> Z; a tie broken by index instead would make X (octave 1) the second and refuse."""
    assert b < d and F32(b) > F32(nnratio) * F32(d)
    groups = [[(d, 1), (d, 2), (b, 1)], [(d, 1), (b, 2), (d, 2)], [(d, 1), (d, 2)], [(d, 1), (d, 1)]]
    xy, oc, desc, uv, expected = [], [], [], [], []
    for g, grp in enumerate(groups):
        x0 = 160.0 + 96 * g
        for k, (dist, o) in enumerate(grp):
            xy.append((x0 + k, 160.0)); oc.append(o); desc.append(T(dist))
        uv.append((x0 + 1, 160.0))
    base = len(xy)
    expected = [-1, 4, 6, -1, base + 1]
    # group 4: X (index base) and Z (base + 1) in cell column 40, Y (base + 2) in cell column 39
    xy += [(40 * CELL - 4, 160.0), (40 * CELL - 3, 160.0), (40 * CELL - 12, 160.0)]
    oc += [1, 1, 2]
    desc += [T(d), T(b), T(d)]
    uv.append((40 * CELL - 8, 160.0))
    kps = keypoints(xy, octave=np.array(oc))
    q = queries(uv, 8.0)
    return Case(f"ties-map-{d}-{b}-{nnratio}", "map", kps, desc, q, [T(0)] * len(uv), expected, {"gated_max": 3}, nnratio=nnratio)


# ---- e. capacity, f. whole_image -----------------------------------------------------------------------------------------------
def lattice(nx=64, ny=64, n=None, octaves=False):
    """nx x ny keypoints, 15.5 x 11.5 px apart from (10, 10): every one inside the grid, at most one per cell column / row pair
    for nx, ny <= 64.  Keypoint i * ny + j carries TT(2 i, 2 j): distinct, and a neighbour is at distance 2 per step."""
    xy = [(10.0 + 15.5 * i, 10.0 + 11.5 * j) for i in range(nx) for j in range(ny)]
    desc = np.array([TT(2 * i, 2 * j) for i in range(nx) for j in range(ny)], np.uint8)
    n = len(xy) if n is None else n
    kps = keypoints(xy[:n], octave=(np.arange(n) % 8) if octaves else 0)
    return kps, desc[:n]


def capacity(fn="last", n=4096, nq=None, reverse=False, radius=20.0):
    """Every query sits on a keypoint of the 64 x 64 lattice with its descriptor: distance 0 is unique, so query k matches the
    keypoint it sits on, whatever else its window holds (radius 20: the 3 x 3 neighbourhood, 9 > PSL_TOPK candidates; radius
    1000: all n).  reverse: query k sits on keypoint n - 1 - k, so that the row r of a thread's query and of its keypoint differ.
    "map": octaves 0..7 by index and the level band (octave - 1, octave) of src/ORBmatcher.cc:66."""
    kps, desc = lattice(n=n, octaves=fn == "map")
    nq = n if nq is None else nq
    target = (n - 1 - np.arange(nq)) if reverse else np.arange(nq)
    q = queries(np.stack([kps["x"][target], kps["y"][target]], 1), radius)
    opts = {}
    if fn == "map":
        q["min_level"], q["max_level"] = kps["octave"][target] - 1, kps["octave"][target]
        opts["nnratio"] = 0.8
    facts = {"grid_kept": n, "nq": nq, "max_index": int(target.max())}
    if fn != "map":
        facts["gated_max"] = 9 if radius == 20.0 else n
    return Case(f"capacity-{fn}-n{n}-nq{nq}-{'rev' if reverse else 'fwd'}-r{int(radius)}", fn, kps, desc, q, desc[target], target, facts,
                **opts)


def whole_image(nq=4096, reverse=True):
    """the 4096-keypoint frame, every query with radius 1000: all 64 x 48 cells, T = 4096 candidates, 64 rounds of the wide pass"""
    c = capacity("last", 4096, nq, reverse, radius=1000.0)
    c.name = f"whole-image-nq{nq}"
    c.facts = dict(c.facts, window_T_all=4096)
    return c


# ---- restatements for the two families whose answers are float32 decisions ---------------------------------------------------------
def features_in_area(kps, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea src/Frame.cc:985-1043 in float32 and in the reference's statement order, on the grid of
    AssignFeaturesToGrid / PosInGrid (:1040-1050).  -> keypoint indices in visiting order."""
    mnx, mny, mxx, mxy = (F32(b) for b in bounds)
    iw, ih = F32(64) / F32(mxx - mnx), F32(48) / F32(mxy - mny)
    rnd = lambda t: int(np.floor(np.float64(t) + 0.5)) if t >= 0 else -int(np.floor(-np.float64(t) + 0.5))   # round(): halves away from zero
    x, y, r = F32(x), F32(y), F32(r)
    c0x = max(0, int(np.floor(F32(F32(x - mnx) - r) * iw)))
    if c0x >= 64: return []
    c1x = min(63, int(np.ceil(F32(F32(x - mnx) + r) * iw)))
    if c1x < 0: return []
    c0y = max(0, int(np.floor(F32(F32(y - mny) - r) * ih)))
    if c0y >= 48: return []
    c1y = min(47, int(np.ceil(F32(F32(y - mny) + r) * ih)))
    if c1y < 0: return []
    check = min_level > 0 or max_level >= 0
    cell = [(rnd(F32(k["x"] - mnx) * iw), rnd(F32(k["y"] - mny) * ih)) for k in kps]
    out = []
    for ix in range(c0x, c1x + 1):
        for iy in range(c0y, c1y + 1):
            for j, k in enumerate(kps):
                if cell[j] != (ix, iy): continue
                if check and (k["octave"] < min_level or (max_level >= 0 and k["octave"] > max_level)): continue
                if abs(F32(k["x"] - x)) < r and abs(F32(k["y"] - y)) < r: out.append(j)
    return out


def rot_bin(a1, a2):
    """src/ORBmatcher.cc:607-612 in float32"""
    rot = F32(a1) - F32(a2)
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    b = int(np.floor(np.float64(F32(rot * (F32(1.0) / F32(HISTO_LENGTH)))) + 0.5))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima src/ORBmatcher.cc:1601-1645 on the bin counts"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2:
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def restate_last(kps, desc, uright, bounds, q, qd, taken, check_ori, th=TH_HIGH, stereo=True):
    """SearchByProjection(cur,last) src/ORBmatcher.cc:1392-1467 from the queries on, over features_in_area: the answer of the
    border and rotation cases.  -> (match, assigned)"""
    n = len(kps)
    dist = lambda a, b: int(np.unpackbits(np.bitwise_xor(a, b)).sum())
    blocked = np.zeros(n, bool) if taken is None else np.asarray(taken, bool).copy()
    chosen = np.full(len(q), -1, np.int32)
    for i, e in enumerate(q):
        best, bi = 256, -1
        for j in features_in_area(kps, bounds, e["u"], e["v"], e["radius"], e["min_level"], e["max_level"]):
            if blocked[j]: continue
            if stereo and uright is not None and uright[j] > 0 and abs(F32(e["ur"] - uright[j])) > e["radius"]: continue
            d = dist(qd[i], desc[j])
            if d < best: best, bi = d, j
        if best <= th:
            chosen[i] = bi
            blocked[bi] = bool(e["blocks"])
    filtered = np.zeros(len(q), bool)
    if check_ori:
        bins = [rot_bin(q["angle"][i], kps["angle"][c]) if c >= 0 else -1 for i, c in enumerate(chosen)]
        keep = three_maxima([bins.count(b) for b in range(HISTO_LENGTH)])
        filtered = np.array([b >= 0 and b not in keep for b in bins], bool)
    return np.where(filtered, -1, chosen).astype(np.int32), owners(chosen, n, filtered)


# ---- g. borders --------------------------------------------------------------------------------------------------------------
def borders(with_taken=True, with_uright=True):
    """Windows at and beyond the four bounds, radius 0, |dx| == r, the level band's forms, keypoints that PosInGrid drops, the
    mvuRight gate at er == radius, a `taken` mask.  Queries do not block (one blocking pair aside), every distance is distinct;
    the answer is restate_last."""
    xy = [(2, 2), (1015, 5), (5, 755), (1015, 755),          # 0-3: inside, near the corners
          (1020, 5), (1016, 300), (5, 760), (-9, 5), (5, -9),  # 4-8: cell 64, 63.5 -> 64, row 48, column -1, row -1: dropped
          (-7, 5), (5, -7),                                  # 9-10: outside the image but cell 0: kept
          (500, 300), (510, 300), (500, 310)]                # 11-13: the |dx| == r probes
    oc = [0] * len(xy)
    band0 = len(xy)
    xy += [(700 + o, 500) for o in range(8)]                 # the level band cluster: octave o carries T(10 (7 - o))
    oc += list(range(8))
    st0 = len(xy)
    xy += [(300, 600), (302, 600), (304, 600)]               # the stereo cluster
    oc += [0, 0, 0]
    kps = keypoints(xy, octave=np.array(oc))
    n = len(kps)
    desc = np.array([T(3 + 2 * i) for i in range(n)], np.uint8)
    for o in range(8):
        desc[band0 + o] = T(10 * (7 - o) + 1)
    desc[9], desc[10] = T(1), T(2)                           # nearer than keypoint 0: a window over the corner picks them
    uright = np.full(n, -1.0, np.float32)
    uright[st0], uright[st0 + 1], uright[st0 + 2] = 100.0, 0.0, 100.0      # 0: mvuRight > 0 is false, no gate
    desc[st0], desc[st0 + 1], desc[st0 + 2] = T(1), T(30), T(20)
    up = lambda v: np.nextafter(F32(v), F32(np.inf))
    Q = []   # (u, v, radius, min_level, max_level, ur, blocks)
    for u, v in [(-50, 5), (-5, 5), (0, 5), (1024, 5), (1030, 5), (1100, 5), (5, -50), (5, -5), (5, 0), (5, 768), (5, 770), (5, 900),
                 (1015, 770), (-5, -5), (1030, 775), (1015, 755)]:
        Q.append((u, v, 20.0, -1, -1, 0.0, 0))
    Q += [(500, 300, 0.0, -1, -1, 0.0, 0), (2, 2, 0.0, -1, -1, 0.0, 0)]                         # radius 0: nothing is < 0
    Q += [(490, 300, 10.0, -1, -1, 0.0, 0), (490, 300, up(10.0), -1, -1, 0.0, 0),                # |dx| == r is outside
          (520, 300, 10.0, -1, -1, 0.0, 0), (520, 300, up(10.0), -1, -1, 0.0, 0),
          (500, 320, 10.0, -1, -1, 0.0, 0), (500, 320, up(10.0), -1, -1, 0.0, 0), (505, 305, 5.0, -1, -1, 0.0, 0), (505, 305, up(5.0), -1, -1, 0.0, 0)]
    for lo, hi in [(-1, -1), (0, -1), (0, 3), (0, 0), (5, -1), (2, 2), (3, 5), (6, 4), (8, -1), (-1, 0), (1, 1), (7, 7)]:
        Q.append((703.5, 500, 12.0, lo, hi, 0.0, 0))
    for ur in (100.0 + 6.0, up(106.0), 100.0 - 6.0, np.nextafter(F32(94.0), F32(-np.inf)), 100.0, 500.0):   # er == radius passes
        Q.append((302, 600, 6.0, -1, -1, ur, 0))
    Q += [(302, 600, 6.0, -1, -1, 100.0, 1), (302, 600, 6.0, -1, -1, 100.0, 0)]                  # a blocking query, then the same again
    q = np.zeros(len(Q), PROJQUERY_DTYPE)
    for i, (u, v, r, lo, hi, ur, b) in enumerate(Q):
        q[i] = (u, v, r, ur, lo, hi, 0.0, b)
    qd = [T(0)] * len(Q)
    taken = None
    if with_taken:
        taken = np.zeros(n, np.uint8)
        taken[[3, band0 + 7]] = 1
    ur_ = uright if with_uright else None
    match, assigned = restate_last(kps, desc, ur_, BOUNDS, q, qd, taken, False)
    facts = {"grid_kept": n - 5, "dropped": [4, 5, 6, 7, 8]}
    return Case(f"borders-taken{int(with_taken)}-ur{int(with_uright)}", "last", kps, desc, q, qd, match, facts, uright=ur_, taken=taken,
                assigned=assigned)


# ---- h. rotation -------------------------------------------------------------------------------------------------------------
# bin -> matches, and (bin of the first query, bin of the last query) of the keypoint that two queries share
ROT_HISTS = {"10-10-10-10": ({0: 10, 3: 10, 7: 10, 12: 10}, (12, 0)),  # ties among the maxima: strict > keeps the first three bins
             "20-2-2": ({5: 20, 2: 2, 9: 2}, (9, 5)),                 # 2 < 0.1f * 20 is false: all three kept
             "20-2-1": ({5: 20, 2: 2, 9: 1}, (9, 5)),                 # the third goes
             "20-1": ({5: 20, 11: 1}, (11, 5)),                       # the second goes
             "7": ({4: 7}, None)}


def rotation(hist_name, check_ori=True):
    """One keypoint per match, far apart, each with a unique descriptor and a query on it (distance 0): the match is certain and
    only the angles decide.  Angle pairs put ROT_HISTS[hist_name][bin] matches into each bin: differences 30 b, 30 b -+ 14 and,
    where float32 rounds them into the bin, 30 b -+ 15; negative differences (the + 360 wrap); 359.99 for bin 12.  Then two
    shared keypoint: the first query of the case (not blocking) and the last one sit on one keypoint, in two bins; where the
    first one's bin is filtered, the keypoint loses its owner although the later match stays (src/ORBmatcher.cc:1456-1466)."""
    target, shared = ROT_HISTS[hist_name]
    pairs = []   # (bin, (query angle, keypoint angle))
    for b, cnt in target.items():
        cand = []
        for rot in (30.0 * b, 30.0 * b - 14.0, 30.0 * b + 14.0, 30.0 * b - 15.0, 30.0 * b + 15.0, 30.0 * b - 14.99, 30.0 * b + 7.5):
            if rot < 0 or rot >= 360:
                continue
            cand += [(rot + 37.5, 37.5), (rot, 0.0), (3.25, 3.25 - rot + 360.0), (0.0, 360.0 - rot)]   # the last two: negative differences
        if b == 12:
            cand.insert(0, (359.99, 0.0))
        cand = [p for p in cand if 0 <= p[0] < 360.0 and 0 <= p[1] <= 360.0 and rot_bin(*p) == b]
        assert len(cand) >= 4, (b, cand)
        pairs += [(b, cand[k % len(cand)]) for k in range(cnt)]
    extra = None
    if shared:
        first = next(i for i, p in enumerate(pairs) if p[0] == shared[0])
        pairs.insert(0, pairs.pop(first))
        last = max(i for i, p in enumerate(pairs) if p[0] == shared[1])
        pairs.pop(last)                                    # its match goes to the shared keypoint instead of one of its own
        extra = F32(pairs[0][1][1]) + F32(30.0 * shared[1])
        extra = extra - F32(360.0) if extra >= 360.0 else extra
        assert rot_bin(extra, pairs[0][1][1]) == shared[1]
    nk = len(pairs)
    kps = keypoints([(40.0 + 48 * (i % 20), 40.0 + 48 * (i // 20)) for i in range(nk)], angle=np.array([p[1][1] for p in pairs], np.float32))
    desc = np.array([TT(2 * (i % 20), 2 * (i // 20)) for i in range(nk)], np.uint8)
    q = queries(np.stack([kps["x"], kps["y"]], 1), 5.0, angle=np.array([p[1][0] for p in pairs], np.float32))
    qd = desc.copy()
    if shared:
        q["blocks"][0] = 0
        q = np.concatenate([q, queries([(kps["x"][0], kps["y"][0])], 5.0, angle=extra)])
        qd = np.concatenate([qd, desc[:1]])
    match, assigned = restate_last(kps, desc, None, BOUNDS, q, qd, None, check_ori)
    facts = {"hist": dict(target), "shared_keypoint": shared is not None}
    return Case(f"rotation-{hist_name}-ori{int(check_ori)}", "last", kps, desc, q, qd, match, facts, assigned=assigned, check_ori=check_ori)


# ---- i. bow ------------------------------------------------------------------------------------------------------------------
def bow(nnratio=0.8):
    """SearchByBoW (src/ORBmatcher.cc:159-288) on feature-vector runs.
      run A: 80 entries (> 64: two rounds), in a shuffled order of feature indices; entry k carries T(k) for k < 8,
             T(8 + 10 (k - 8)) for 8 <= k <= 13 and T(200) behind.  Queries 0..7 carry T(k) and own entries 0..7; queries 8..12
             carry T(0): the 8 cached best are taken; 8 / 18, 18 / 28, 28 / 38, 38 / 48 pass the ratio 0.8, 48 / 58 does not.
      run B: T(40), T(50): 40 < 0.8f * 50 == 40.0f is false -> refused (the opposite of SearchByProjection(F, MapPoints)).
      run C: T(39), T(50): accepted.         run D: one entry T(50): 50 <= TH_LOW, second = 256 -> accepted.
      run E: one entry T(51): refused.       run F: empty.
    With nnratio = 3 / 16: 0.1875f * 256 == 48 exactly, so a lone T(48) is refused and a lone T(47) accepted (runs G, H); run A's
    and B's / C's queries are then all refused except the distance-0 ones."""
    rng = np.random.default_rng(4)
    nf = 100
    perm = rng.permutation(nf)
    fidx, runs_of = [], {}
    def add(name, feats):
        runs_of[name] = (len(fidx), len(feats))
        fidx.extend(int(f) for f in feats)
    desc = np.zeros((nf, 32), np.uint8)
    A = perm[:80]
    add("A", A)
    for k, f in enumerate(A):
        desc[f] = T(k) if k < 8 else T(8 + 10 * (k - 8)) if k <= 13 else T(200)
    rest = list(perm[80:])
    def feats(*codes):
        fs = [rest.pop() for _ in codes]
        for f, c in zip(fs, codes):
            desc[f] = c
        return fs
    add("B", feats(T(40), T(50)))
    add("C", feats(T(39), T(50)))
    add("D", feats(T(50)))
    add("E", feats(T(51)))
    add("F", [])
    add("G", feats(T(48)))
    add("H", feats(T(47)))
    runs, qd, expected = [], [], []
    def ask(name, code, want):
        runs.append(runs_of[name]); qd.append(code); expected.append(want)
    first = lambda name, k=0: fidx[runs_of[name][0] + k]
    exact = nnratio == 0.8
    assert exact or nnratio == 0.1875
    for k in range(8):
        ask("A", T(k), first("A", k))                                        # 0 < nnratio * 1
    for k in range(8, 13):
        ask("A", T(0), first("A", k) if exact and k < 12 else -1)
    ask("B", T(0), -1)
    ask("C", T(0), first("C") if exact else -1)                              # 39 < 0.1875f * 50 is false
    ask("D", T(0), first("D") if exact else -1)                              # 50 < 48 is false
    ask("E", T(0), -1)
    ask("F", T(0), -1)
    ask("G", T(0), -1 if not exact else first("G"))
    ask("H", T(0), first("H"))
    kps = keypoints([(50.0 + 7 * (i % 30), 50.0 + 9 * (i // 30)) for i in range(nf)])
    q = queries([(0.0, 0.0)] * len(runs), 0.0)
    return Case(f"bow-{nnratio}", "bow", kps, desc, q, qd, expected, {"window_T": 80, "list_exhausted": 5, "empty_runs": 1},
                nnratio=nnratio, fidx=np.array(fidx, np.int32), runs=np.array(runs, np.int32).reshape(-1, 2),
                qangle=np.zeros(len(runs), np.float32))


# ---- decision equalities of SearchByProjection(F, MapPoints) ---------------------------------------------------------------------
def map_equalities():
    """bestDist > nnratio * bestDist2 at equality: 0.8f * 50.f is exactly 40.f, so 40 against 50 in one octave is accepted and 41
    is refused; bestDist == TH_HIGH is accepted with a second best of another octave, 101 is not.  Each entry: (best, second,
    expected), a candidate as (distance, octave)."""
    spec = [((40, 0), (50, 0), 0), ((41, 0), (50, 0), -1), ((100, 0), (101, 1), 0), ((101, 0), (120, 1), -1),
            ((100, 0), (126, 0), 0), ((100, 0), (124, 0), -1)]   # 0.8f * 126 = 100.8: accepted; 0.8f * 124 = 99.2: refused
    xy, oc, desc, uv, expected = [], [], [], [], []
    for g, ((d1, o1), (d2, o2), want) in enumerate(spec):
        x0 = 100.0 + 64 * g
        xy += [(x0, 400.0), (x0 + 1, 400.0)]; oc += [o1, o2]; desc += [T(d1), T(d2)]
        uv.append((x0, 400.0)); expected.append(2 * g if want == 0 else -1)
    return Case("map-equalities", "map", keypoints(xy, octave=np.array(oc)), desc, queries(uv, 6.0), [T(0)] * len(uv), expected,
                {"gated_max": 2}, nnratio=0.8)


# ---- the complement of the query: distance 256 -------------------------------------------------------------------------------------
def complement(fn):
    """A candidate at distance 256 never passes the reference's strict dist < bestDist with bestDist = 256 at the start
    (src/ORBmatcher.cc:76-78, :102, :110, :1535, :1548): it is neither the best nor the second best.
      "kf" with ORBdist = 256: a lone T(256) -> the reference writes mvpMapPoints[-1]; defined as no match.  T(256) next to T(255):
           the T(255) one.  Two T(256): no match.
      "map" with nnratio 0.25: T(80) and T(256) in one octave: the second best stays "none" (level -1), so no ratio test: matched;
           were T(256) the second best, 80 > 0.25f * 256 would refuse.  T(80) and T(255): refused."""
    kps = keypoints([(100, 100), (300, 100), (301, 100), (500, 100), (501, 100)])
    q = queries([(100, 100), (300, 100), (500, 100)], 5.0)
    if fn == "kf":
        return Case("complement-kf", fn, kps, [T(256), T(256), T(255), T(256), T(256)], q, [T(0)] * 3, [-1, 2, -1], {"gated_max": 2},
                    orb_dist=256)
    return Case("complement-map", fn, kps, [T(256), T(80), T(256), T(80), T(255)], q, [T(0)] * 3, [-1, 1, -1], {"gated_max": 2},
                nnratio=0.25)


def second_at_256(nnratio=0.3):
    """SearchByProjection(F, MapPoints) at the acceptance threshold with a second candidate at distance 256 in the best's octave:
    bestDist2 stays 256 with level -1 (src/ORBmatcher.cc:76-78, :102-110), no ratio test, T(100) is matched although 100 > 0.3f *
    256; next to it T(100) against T(255) (refused) and T(101) against T(256) (above TH_HIGH)."""
    kps = keypoints([(100, 100), (101, 100), (300, 100), (301, 100), (500, 100), (501, 100), (700, 100), (701, 100)])
    q = queries([(100, 100), (300, 100), (500, 100), (700, 100)], 5.0)
    return Case(f"second-at-256-{nnratio}", "map", kps, [T(100), T(256), T(256), T(100), T(100), T(255), T(101), T(256)], q, [T(0)] * 4,
                [0, 3, -1, -1], {"gated_max": 2}, nnratio=nnratio)


# ---- the lists the tests walk --------------------------------------------------------------------------------------------------
def host_cases():
    """every case for the host entry points, by the function it is meant for"""
    cs = []
    for fn in ("last", "map", "kf"):
        cs += [chain(300, fn, 1), chain(300, fn, 0) if fn != "kf" else chain(64, fn, 1)]   # "kf" forces blocking
    cs += [exhausted_list("last"), exhausted_list("map", "equal"), exhausted_list("map", "alternating")]
    cs += [exhausted_list("kf", orb_dist=d) for d in (64, 80, 100)]
    cs += [pile_up("last"), pile_up("map", "equal"), pile_up("map", "alternating")]
    cs += [pile_up("last", nk=40, step=3, pad=p) for p in (1030, 2050, 3080)]
    cs += [pile_up("map", "alternating", nk=40, step=3, pad=3080)]
    cs += [ties("last"), ties("map"), ties("kf", 64), ties("kf", 100), ties_map(5, 3, 0.5), ties_map(10, 9, 0.8), map_equalities(), complement("kf"), complement("map"),
           second_at_256()]
    cs += [capacity("last"), capacity("last", nq=2049), capacity("last", nq=3073), capacity("last", n=4095), capacity("last", reverse=True),
           capacity("map"), capacity("map", reverse=True), capacity("kf").with_opts(orb_dist=100)]
    cs += [whole_image()]
    cs += [borders(), borders(False, True), borders(True, False)]
    cs += [rotation(h, o) for h in ROT_HISTS for o in (True, False)]
    cs += [bow(0.8), bow(0.1875)]
    out = []
    for c in cs:
        # angles are zero outside the rotation cases: the orientation check keeps everything, so both settings share one answer
        if c.fn in ("last", "kf", "bow") and "check_ori" not in c.opts:
            out += [c.with_opts(check_ori=True), c.with_opts(check_ori=False)] if len(c.q) <= 400 else [c.with_opts(check_ori=True)]
        else:
            out.append(c)
    return out


def device_cases(mode, cap=1280):
    """the cases of one batched launch (mode 0: SearchByProjection(cur,last) with check_ori on, mode 1: SearchByProjection(F,
    MapPoints) with nnratio 0.8 and a `taken` mask), each of at most `cap` keypoints and queries"""
    if mode == 0:
        kps, desc = lattice(40, 32)
        lat = Case("lattice-1280", "last", kps, desc, queries(np.stack([kps["x"], kps["y"]], 1)[::-1], 20.0), desc[::-1],
                   np.arange(1280)[::-1], {"grid_kept": 1280, "nq": 1280, "gated_max": 9})
        return [chain(300), chain(300, blocks=0), exhausted_list(), pile_up(), pile_up(nk=40, step=3, pad=1030), ties(),
                borders(False, True), borders(False, False), lat] + [rotation(h, True) for h in ROT_HISTS]
    kps, desc = lattice(40, 32, octaves=True)
    q = queries(np.stack([kps["x"], kps["y"]], 1)[::-1], 20.0, min_level=kps["octave"][::-1] - 1, max_level=kps["octave"][::-1])
    lat = Case("lattice-1280-map", "map", kps, desc, q, desc[::-1], np.arange(1280)[::-1], {"grid_kept": 1280, "nq": 1280}, nnratio=0.8)
    return [chain(300, "map"), chain(300, "map", 0), exhausted_list("map", "equal"), exhausted_list("map", "alternating"),
            pile_up("map", "equal"), pile_up("map", "alternating"), pile_up("map", "alternating", nk=40, step=3, pad=1030),
            ties_map(10, 9, 0.8), map_equalities(), lat, ties("map"), borders(True, True).retarget("map", nnratio=0.8),
            borders(True, False).retarget("map", nnratio=0.8), rotation("20-2-1").retarget("map", nnratio=0.8)]
