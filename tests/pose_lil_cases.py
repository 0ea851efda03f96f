"""The restatement of the LIL edges of Optimizer::PoseOptimization (EdgeLILSE3ProjectXYZ with its fixed VertexLIL,
add_inc/EdgeLIL.h:210-439, src/Optimizer.cc:619-694, :973-1008) on top of tests/pose_opt_cases.py, the restated set-up loop
(:631-693) and the seeded cases of tests/test_pose_lil_cpu.py / test_pose_lil_gpu.py.

_Lil mirrors the psl_po_lil_* functions of psl-slam_amd/csrc/pose_kernels.h operation by operation; it is an edge kind of
pose_opt_cases.levenberg_rounds, which holds the rounds for both kinds (their iterations and trials are lm_cases.levenberg).  A LIL
edge adds its 28 terms ROW BY ROW: each of its six Jacobian rows is a rank-one contribution that is added to the running sum before the next row is made, so an
edge is a sequence of six additions (a point edge is one).  order="device" runs these sequences in the device's order of the sums
(LIL edge j has the edge index n + j), order="edge" edge by edge, points first, which is g2o's.

Two oddities of the reference are restated on purpose:
  * linearizeOplus reads segment<3>(9) for xyz2_s and xyz2_e (EdgeLIL.h:273-275): row 2 of the Jacobian is evaluated at line 2's END
    point while e2 is the error at its START point (fix_row2=True is the "corrected" variant, for the test that tells them apart);
  * the set-up loop takes mvle_l[i] and CrossPoint_2D[i] with i a PLANE index, though mvle_l has one row per CROSSING
    (src/Frame.cc:528 before the `continue`s, :643; aligned=True is the variant that follows the plane to its crossing)."""
import functools
import math

import numpy as np

import pose_opt_cases as pc

LIL_DTYPE = np.dtype([("line1", "<f8", (6,)), ("line2", "<f8", (6,)), ("cross", "<f8", (3,)), ("obs1", "<f8", (3,)), ("obs2", "<f8", (3,)),
                      ("obs_ins", "<f8", (2,))])
MAPLIL_DTYPE = np.dtype([("w", "<f8", (15,)), ("bad", "u1"), ("pad", "u1", (7,))])
DELTA_LIL = float(np.float32(math.sqrt(11.07)))       # float deltaLJL = sqrt(11.07)  (src/Optimizer.cc:628)
CHI2_LIL = np.float32(11.07)
MARGIN = pc.MARGIN


class _Lil:
    def __init__(self, lil, cam, fix_row2=False):
        l = np.ascontiguousarray(lil, LIL_DTYPE)
        self.m = len(l)
        W = np.concatenate([l["line1"], l["line2"], l["cross"]], 1).reshape(self.m, 15)
        self.X = [[W[:, 3 * p + a].copy() for a in range(3)] for p in range(5)]      # X1s X1e X2s X2e Xins
        self.l = [[l["obs1"][:, a].copy() for a in range(3)], [l["obs2"][:, a].copy() for a in range(3)]]
        self.ins = [l["obs_ins"][:, 0].copy(), l["obs_ins"][:, 1].copy()]
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy"))
        self.fix_row2 = fix_row2
        self.thr = np.full(self.m, CHI2_LIL)                                     # chi2LLIL (src/Optimizer.cc:704, :993)

    # an edge kind of pc.levenberg_rounds: six additions per edge; an outlier does NOT lower the return value (nBad counts the point
    # edges only, src/Optimizer.cc:1022)
    steps, counted = 6, False
    count = property(lambda self: self.m)

    def chi(self, T):
        e = self.error(T)
        return e, self.chi2(e)

    def additions(self, e, T, rho0, rho1):
        return self.rows(e, T, rho0, rho1)

    def _map(self, T, X):
        r = pc._rotate(T[0], X)
        return [r[0] + T[1][0], r[1] + T[1][1], r[2] + T[1][2]]

    def _project(self, T, X):
        Pc = self._map(T, X)
        return (Pc[0] / Pc[2]) * self.fx + self.cx, (Pc[1] / Pc[2]) * self.fy + self.cy

    def error(self, T):
        """computeError (EdgeLIL.h:220-256): six arrays [m]"""
        e = []
        for r in range(4):
            u, v = self._project(T, self.X[r])
            l = self.l[r >> 1]
            e.append((u * l[0] + v * l[1]) + l[2])
        u, v = self._project(T, self.X[4])
        e.append(self.ins[0] - u)
        e.append(self.ins[1] - v)
        return e

    @staticmethod
    def chi2(e):
        c = e[0] * e[0]
        for r in range(1, 6):
            c = c + e[r] * e[r]
        return c

    @staticmethod
    def huber(c):
        dsqr = DELTA_LIL * DELTA_LIL
        sq = np.sqrt(c)
        inl = c <= dsqr
        return np.where(inl, c, (2.0 * sq) * DELTA_LIL - dsqr), np.where(inl, 1.0, DELTA_LIL / sq)

    def _row_line(self, Pc, l0, l1):
        x, y = Pc[0], Pc[1]
        invz = 1.0 / Pc[2]
        invz2 = invz * invz
        fx, fy = self.fx, self.fy
        return [((((-fx) * x) * y) * invz2) * l0 - (fy * (1.0 + (y * y) * invz2)) * l1,
                (fx * (1.0 + (x * x) * invz2)) * l0 + (((fy * x) * y) * invz2) * l1,
                (((-fx) * y) * invz) * l0 + ((fy * x) * invz) * l1,
                (fx * invz) * l0,
                (fy * invz) * l1,
                (((-fx) * x) * l0 - (fy * y) * l1) * invz2]

    def _row_ins(self, Pc, second):
        x, y = Pc[0], Pc[1]
        invz = 1.0 / Pc[2]
        invz2 = invz * invz
        fx, fy = self.fx, self.fy
        zero = np.zeros(self.m)
        if not second:
            return [((x * y) * invz2) * fx, (-(1.0 + (x * x) * invz2)) * fx, (y * invz) * fx, (-fx) * invz, zero, (x * invz2) * fx]
        return [(1.0 + (y * y) * invz2) * fy, (((-fy) * x) * y) * invz2, ((-fy) * x) * invz, zero, (-fy) * invz, (fy * y) * invz2]

    def rows(self, e, T, rho0, rho1):
        """The six additions of every edge: [m][6][28] - row r's rank-one contribution; rho in the last one."""
        out = np.zeros((self.m, 6, 28))
        for r in range(6):
            if r < 4:
                src = 3 if (r == 2 and not self.fix_row2) else r       # EdgeLIL.h:273-275: segment<3>(9) twice
                l = self.l[r >> 1]
                J = self._row_line(self._map(T, self.X[src]), l[0], l[1])
            else:
                J = self._row_ins(self._map(T, self.X[4]), r - 4)
            h = 0
            for j in range(6):
                wj = rho1 * J[j]
                for k in range(j, 6):
                    out[:, r, h] = wj * J[k]
                    h += 1
                out[:, r, 21 + j] = wj * e[r]
        out[:, 5, 27] = rho0
        return out


def optimize(Tcw, edges, lil, cam, order="device", fix_row2=False):
    """The point edges, then the LIL edges (LIL edge j has the edge index n + j)
    -> (pose_out, outlier u8 [n] or None, outlier_lil u8 [m] or None, ngood, info, margin); None when nothing is written"""
    pose, flags, ngood, info, margin = pc.levenberg_rounds(Tcw, [pc._Edges(edges, cam), _Lil(lil, cam, fix_row2)], order)
    outlier, outlier_lil = (None, None) if flags is None else flags
    return pose, outlier, outlier_lil, ngood, info, margin


# ---- the set-up loop src/Optimizer.cc:631-693 ------------------------------------------------------------------------------------------
def lil_edges(le_l, cross2d, lil_index, lil_map, cross_of_plane=None):
    """-> (LIL_DTYPE edges in plane order, the plane of each edge).  le_l [k][6]: mvle_l, one row per crossing; cross2d [p][2]:
    CrossPoint_2D, one row per plane; lil_index [p]: the row of plane i's map LIL in lil_map (MAPLIL_DTYPE) or -1.  Plane i takes
    mvle_l[i] and CrossPoint_2D[i] (:658-660).  cross_of_plane: the "aligned" variant - plane i takes mvle_l[cross_of_plane[i]]."""
    le_l, cross2d = np.asarray(le_l, np.float64).reshape(-1, 6), np.asarray(cross2d, np.float64).reshape(-1, 2)
    planes = [i for i in range(min(len(cross2d), len(le_l))) if 0 <= lil_index[i] < len(lil_map) and not lil_map["bad"][lil_index[i]]]
    e = np.zeros(len(planes), LIL_DTYPE)
    for k, i in enumerate(planes):
        w = lil_map["w"][lil_index[i]]
        row = i if cross_of_plane is None else cross_of_plane[i]
        e["line1"][k], e["line2"][k], e["cross"][k] = w[0:6], w[6:12], w[12:15]
        e["obs1"][k], e["obs2"][k], e["obs_ins"][k] = le_l[row, 0:3], le_l[row, 3:6], cross2d[i]
    return e, np.array(planes, np.int32)


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def _line_eq(ps, pe):
    """le_l of src/Frame.cc:520-526: (sp x ep) / sqrt(a^2 + b^2)"""
    l = np.cross(np.concatenate([ps, np.ones((len(ps), 1))], 1), np.concatenate([pe, np.ones((len(pe), 1))], 1))
    return l / np.sqrt(l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1])[:, None]


def make_lil(rng, Ttrue, cam, m, outliers, noise=True):
    """m LIL edges seen from Ttrue: two 3-D segments that cross 1.5 to 6 m in front of the camera, each 0.2 to 0.6 m to one side of
    the crossing and 0.3 to 0.8 m to the other (so start and end of line 2 are clearly different points); the observations are the
    projections at Ttrue with 0.5 px of noise on the end points and the crossing; a planted outlier is 20 to 60 px off.
    -> (LIL_DTYPE [m], planted u8 [m])"""
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    Rt, tt = Ttrue["R"].astype(np.float64).reshape(3, 3), Ttrue["t"].astype(np.float64)
    z = rng.uniform(1.5, 6.0, m)
    u, v = rng.uniform(120.0, 520.0, m), rng.uniform(100.0, 380.0, m)
    Cc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    pts = []
    for _ in range(2):
        d = rng.normal(size=(m, 3)) * np.array([1.0, 1.0, 0.3])
        d /= np.linalg.norm(d, axis=1)[:, None]
        pts += [Cc - rng.uniform(0.2, 0.6, m)[:, None] * d, Cc + rng.uniform(0.3, 0.8, m)[:, None] * d]
    pts.append(Cc)
    W = [(p - tt) @ Rt for p in pts]                    # Rt^T (Pc - t): the world data, held as doubles
    P2 = []
    for w in W:
        p = w @ Rt.T + tt
        P2.append(np.stack([p[:, 0] / p[:, 2] * fx + cx, p[:, 1] / p[:, 2] * fy + cy], 1))
    if noise:
        P2 = [p + rng.normal(size=p.shape) * 0.5 for p in P2]
    planted = np.zeros(m, np.uint8)
    k = int(round(outliers * m))
    if k:
        idx = rng.choice(m, k, replace=False)
        ang, mag = rng.uniform(0, 2 * math.pi, k), rng.uniform(20.0, 60.0, k)
        off = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
        for p in P2:
            p[idx] += off * rng.uniform(0.5, 1.0, (k, 1)) * rng.choice([-1.0, 1.0], (k, 1))
        planted[idx] = 1
    e = np.zeros(m, LIL_DTYPE)
    e["line1"], e["line2"], e["cross"] = np.concatenate([W[0], W[1]], 1), np.concatenate([W[2], W[3]], 1), W[4]
    e["obs1"], e["obs2"], e["obs_ins"] = _line_eq(P2[0], P2[1]), _line_eq(P2[2], P2[3]), P2[4]
    return e, planted


def make_case(seed, n, kind, outliers, m, lil_outliers):
    """the point edges of pc.make_case(seed, n, kind, outliers) and m LIL edges seen from the same true pose"""
    c = pc.make_case(seed, n, kind, outliers)
    rng = np.random.default_rng(seed + 500000)
    c["lil"], c["planted_lil"] = make_lil(rng, c["Ttrue"], c["cam"], m, lil_outliers)
    return c


def make_setup_case(seed, n=30, nplanes=12, ncross=20, nmap=16):
    """a frame with more crossings than planes: plane i comes from crossing cross_of_plane[i] >= i (crossings in between gave no
    plane); the map LILs of the planes, two planes without one (-1, and an index outside the map) and one bad one.
    -> the case with le_l [ncross][6], cross2d [nplanes][2], lil_index, lil_map, cross_of_plane, and lil = the edges of the loop"""
    c = pc.make_case(seed, n, "mixed", 0.0)
    rng = np.random.default_rng(seed + 700000)
    e, _ = make_lil(rng, c["Ttrue"], c["cam"], ncross, 0.0)
    cross_of_plane = np.sort(rng.choice(np.arange(1, ncross), nplanes, replace=False))      # never the identity: row 0 gives no plane
    lil_map = np.zeros(nmap, MAPLIL_DTYPE)
    lil_index = np.full(nplanes, -1, np.int32)
    rows = rng.permutation(nmap)[:nplanes]
    for i in range(nplanes):
        k = cross_of_plane[i]
        lil_map["w"][rows[i]] = np.concatenate([e["line1"][k], e["line2"][k], e["cross"][k]])
        lil_index[i] = rows[i]
    lil_index[3], lil_index[7] = -1, nmap + 2
    lil_map["bad"][lil_index[5]] = 1
    c["le_l"] = np.concatenate([e["obs1"], e["obs2"]], 1)
    c["cross2d"] = e["obs_ins"][cross_of_plane].copy()
    c["lil_index"], c["lil_map"], c["cross_of_plane"] = lil_index, lil_map, cross_of_plane
    c["lil"], c["edge_plane"] = lil_edges(c["le_l"], c["cross2d"], lil_index, lil_map)
    c["planted_lil"] = np.zeros(len(c["lil"]), np.uint8)
    return c


# name -> (point edges, kind, their outlier share, LIL edges, their outlier share)
CASE_SPECS = {
    "p2_l0": (2, "mixed", 0.0, 0, 0.0),            # 2 edges in all: the early return
    "p2_l1": (2, "mixed", 0.0, 1, 0.0),            # 3: optimised only because of the LIL edge
    "p2_l7": (2, "mixed", 0.0, 7, 0.0),            # 9: one round
    "p2_l8": (2, "mixed", 0.0, 8, 0.3),            # 10: four rounds only because of the LIL edges
    "p0_l3": (0, "mixed", 0.0, 3, 0.0),            # LIL edges only
    "p0_l64": (0, "mixed", 0.0, 64, 0.3),
    "p0_l65": (0, "mixed", 0.0, 65, 0.0),
    "p250_l10": (250, "mixed", 0.3, 10, 0.3),      # the LIL indices cross the 256 boundary
    "p257_l3": (257, "stereo", 0.0, 3, 0.0),
    "p2048_l4": (2048, "mixed", 0.3, 4, 0.0),      # the point rows in LDS
    "p2100_l4": (2100, "mono", 0.0, 4, 0.3),       # and in HBM
    "p40_l512": (40, "mixed", 0.3, 512, 0.3),      # the most LIL rows a frame of the record layout can have
    "p40_l512_0": (40, "mono", 0.0, 512, 0.0),
    "p100_l8_allout": (100, "mixed", 0.0, 8, 1.0),  # every LIL edge an outlier: the return value still counts them
    "p63_l30": (63, "stereo", 0.3, 30, 0.0),
}
CASE_NAMES = list(CASE_SPECS) + ["setup"]


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its two references: ref[order] = (pose, outlier, outlier_lil, ngood, info).  A seed for which, in either order, a
    classification chi2 (point or LIL) lies within a relative MARGIN of its threshold is rejected: the next seed is taken."""
    base = 100000 + 1000 * (CASE_NAMES.index(name) + 1)
    for seed in range(base, base + 50):
        c = make_setup_case(seed) if name == "setup" else make_case(seed, *CASE_SPECS[name])
        res = {o: optimize(c["Tcw"], c["edges"], c["lil"], c["cam"], o) for o in ("device", "edge")}
        if all(r[5] > MARGIN for r in res.values()):
            c["seed"] = seed
            c["ref"] = {o: r[:5] for o, r in res.items()}
            return c
    raise AssertionError(f"no seed for {name}")


def order_difference():
    """The largest difference of a pose float between the two orders of the restatement over every case."""
    return max(float(np.abs(pc.pose_floats(case(nm)["ref"]["device"][0]).astype(np.float64)
                            - pc.pose_floats(case(nm)["ref"]["edge"][0]).astype(np.float64)).max()) for nm in CASE_NAMES)
