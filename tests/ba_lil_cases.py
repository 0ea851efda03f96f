"""The restatement of Optimizer::LocalBundleAdjustmentAndInseclines (src/Optimizer.cc:1968-2534): the point edges of tests/ba_cases.py
plus the VertexLIL vertices and the EdgeLILSE3ProjectXYZ edges (:2250-2533, add_inc/EdgeLIL.h:210-439, add_inc/VertexLIL.h), in Python
floats, and the seeded scenes of tests/test_local_ba_lil_cpu.py / test_local_ba_lil_gpu.py.

It mirrors the LIL parts of psl-slam_amd/csrc/ba_kernels.h operation by operation and shares no text with it.  The point edges, the
quadratic form of a point edge, the ordered sum and the whole of BlockSolver::solve are the pieces of tests/ba_cases.py (_Problem,
_quad, _sum256, _solve): a LIL is landmark nmp + j of a combined problem and LIL edge j its edge ne + j, so _solve takes the
landmarks - points, then LILs - in ascending row, which is the stated order of S, of the coefficients and of cl.

The update (VertexLIL::oplusImpl maps 15 doubles where the vertex owns 3): segment m of active LIL a(i) receives the step of a(i + m);
past the end of the active update vector the step is 0.0, which is this library's reading - the reference's value is indeterminate
there, so parity with g2o is unpinned."""
import functools
import math
import struct

import numpy as np

import ba_cases as bc
from ba_cases import (DBL_MAX, E_CAPACITY, E_INVALID, EDGE_DTYPE, INFO_DTYPE, KF_DTYPE, MP_DTYPE, _Problem, _finite, _quad, _solve, _sqrt, _sum256,
                      _tri, make_scene)
from lm_cases import _div
from pose_lil_cases import DELTA_LIL, MAPLIL_DTYPE, _line_eq
from pose_opt_cases import _quat_to_R, _rotate, from_pose, se3_exp, se3_mul, to_pose

LILEDGE_DTYPE = np.dtype([("lil", "<i4"), ("kf", "<i4"), ("obs1", "<f8", (3,)), ("obs2", "<f8", (3,)), ("obs_ins", "<f8", (2,))])
assert LILEDGE_DTYPE.itemsize == 72 and MAPLIL_DTYPE.itemsize == 128
LIL_INFO = 0.01              # double invSigma = 0.01 (src/Optimizer.cc:1970)
CHI2_LIL = 11.07             # :2406, :2469, a double comparison


def _map(T, X):
    r = _rotate(T[0], X)
    return [r[0] + T[1][0], r[1] + T[1][1], r[2] + T[1][2]]


class _Lils:
    """the LIL rows and edges of one problem"""

    def __init__(self, lils, ledges, P):
        self.lil = np.ascontiguousarray(lils, MAPLIL_DTYPE).reshape(-1)
        self.ed = np.ascontiguousarray(ledges, LILEDGE_DTYPE).reshape(-1)
        self.n, self.ne = len(self.lil), len(self.ed)
        self.e_kf = [int(v) for v in self.ed["kf"]]
        self.e_lil = [int(v) for v in self.ed["lil"]]
        self.l = [[[float(x) for x in self.ed["obs1"][e]], [float(x) for x in self.ed["obs2"][e]]] for e in range(self.ne)]
        self.ins = [[float(x) for x in self.ed["obs_ins"][e]] for e in range(self.ne)]
        self.fx, self.fy, self.cx, self.cy = P.fx, P.fy, P.cx, P.cy

    def lists(self, nkf):
        self.kf_edges = [[e for e in range(self.ne) if self.e_kf[e] == k] for k in range(nkf)]
        self.lil_edges = [[e for e in range(self.ne) if self.e_lil[e] == j] for j in range(self.n)]

    def project(self, T, X):
        Pc = _map(T, X)
        return _div(Pc[0], Pc[2]) * self.fx + self.cx, _div(Pc[1], Pc[2]) * self.fy + self.cy

    def error(self, e, T, L):
        """computeError (EdgeLIL.h:220-256)"""
        Tk, w = T[self.e_kf[e]], L[self.e_lil[e]]
        er = []
        for r in range(4):
            u, v = self.project(Tk, w[3 * r:3 * r + 3])
            l = self.l[e][r >> 1]
            er.append((u * l[0] + v * l[1]) + l[2])
        u, v = self.project(Tk, w[12:15])
        return er + [self.ins[e][0] - u, self.ins[e][1] - v]

    @staticmethod
    def chi2(er):
        c = er[0] * (LIL_INFO * er[0])
        for r in range(1, 6):
            c = c + er[r] * (LIL_INFO * er[r])
        return c

    @staticmethod
    def huber(c):
        dsqr = DELTA_LIL * DELTA_LIL
        if c <= dsqr:
            return c, 1.0
        sq = _sqrt(c)
        return (2.0 * sq) * DELTA_LIL - dsqr, _div(DELTA_LIL, sq)

    def depth_positive(self, e, T, L):
        """isDepthPositive (EdgeLIL.h:258-262): all five mapped points"""
        Tk, w = T[self.e_kf[e]], L[self.e_lil[e]]
        return all(_map(Tk, w[3 * m:3 * m + 3])[2] > 0.0 for m in range(5))

    def jacobians(self, e, T, L, fix_row2=False):
        """_jacobianOplusXj [6][6] and _jacobianOplusXi [6][3] (EdgeLIL.h:264-381); row 2 at line 2's END point (:273-275)"""
        Tk, w = T[self.e_kf[e]], L[self.e_lil[e]]
        R = _quat_to_R(Tk[0])
        fx, fy = self.fx, self.fy
        Jp, Jl = [], []
        for r in range(4):
            src = 3 if (r == 2 and not fix_row2) else r
            x, y, z = _map(Tk, w[3 * src:3 * src + 3])
            invz = _div(1.0, z)
            invz2 = invz * invz
            l0, l1 = self.l[e][r >> 1][0], self.l[e][r >> 1][1]
            Jp.append([((((-fx) * x) * y) * invz2) * l0 - (fy * (1.0 + (y * y) * invz2)) * l1,
                       (fx * (1.0 + (x * x) * invz2)) * l0 + (((fy * x) * y) * invz2) * l1,
                       (((-fx) * y) * invz) * l0 + ((fy * x) * invz) * l1,
                       (fx * invz) * l0,
                       (fy * invz) * l1,
                       (((-fx) * x) * l0 - (fy * y) * l1) * invz2])
            a, b = (fx * l0) * invz, (fy * l1) * invz
            g = ((fx * x) * l0) * invz2 + ((fy * y) * l1) * invz2
            Jl.append([(a * R[c] + b * R[3 + c]) - g * R[6 + c] for c in range(3)])
        x, y, z = _map(Tk, w[12:15])
        invz = _div(1.0, z)
        invz2 = invz * invz
        Jp.append([((x * y) * invz2) * fx, (-(1.0 + (x * x) * invz2)) * fx, (y * invz) * fx, (-fx) * invz, 0.0, (x * invz2) * fx])
        Jp.append([(1.0 + (y * y) * invz2) * fy, (((-fy) * x) * y) * invz2, ((-fy) * x) * invz, 0.0, (-fy) * invz, (fy * y) * invz2])
        Jl.append([((-fx) * invz) * R[0] + ((fx * x) * invz2) * R[6],
                   ((-fx) * R[1]) * invz + ((fx * x) * R[7]) * invz2,
                   ((-fx) * R[2]) * invz + ((fx * x) * R[8]) * invz2])
        Jl.append([((-fy) * invz) * R[3 + c] + ((fy * y) * invz2) * R[6 + c] for c in range(3)])
        return Jp, Jl


def _quad6(J, n, w, er):
    """_quad of a six-row edge: ((w J0j) J0k + (w J1j) J1k) + ... + (w J5j) J5k"""
    out = []
    for j in range(n):
        for k in range(j, n):
            s = (w * J[0][j]) * J[0][k]
            for r in range(1, 6):
                s = s + (w * J[r][j]) * J[r][k]
            out.append(s)
    for j in range(n):
        s = (w * J[0][j]) * er[0]
        for r in range(1, 6):
            s = s + (w * J[r][j]) * er[r]
        out.append(s)
    return out


class _Combined:
    """what ba_cases._solve reads of a problem: the landmarks are the points and then the LILs"""

    def __init__(self, P, Q):
        self.nmp = P.nmp + Q.n
        self.e_kf = P.e_kf + Q.e_kf
        self.pt_edges = P.pt_edges + [[P.ne + e for e in Q.lil_edges[j]] for j in range(Q.n)]


def lil_update(L, xl_of, active):
    """VertexLIL::oplusImpl under this library's reading: active = a(0) < a(1) < ...; xl_of[j] the step of LIL j -> the candidates"""
    Ln = [list(w) for w in L]
    for i, j in enumerate(active):
        for m in range(5):
            for c in range(3):
                step = xl_of[active[i + m]][c] if i + m < len(active) else 0.0
                Ln[j][3 * m + c] = L[j][3 * m + c] + step
    return Ln


def local_ba(kfs, mps, edges, lils, ledges, cam, rounds=2, caps=None):
    """-> dict(info, kf, mp, erase, lil MAPLIL_DTYPE[nlil], erase_lil u8 [nle], nerased_lil, trace).  trace as ba_cases.local_ba's, with
    llevel, lact, bad_lil, depth_bad_lil, chi2_lil, L and updates: [(active rows, {row: xl}, L before, candidate Ln)] per solved trial"""
    P = _Problem(kfs, mps, edges, cam)
    Q = _Lils(lils, ledges, P)
    info = np.zeros((), INFO_DTYPE)
    res = {"info": info, "kf": P.kf.copy(), "mp": P.mp.copy(), "erase": np.zeros(P.ne, np.uint8), "lil": Q.lil.copy(),
           "erase_lil": np.zeros(Q.ne, np.uint8), "nerased_lil": 0, "trace": []}
    if caps is not None and (P.nkf > caps[0] or P.nmp > caps[1] or P.ne > caps[2] or Q.n > caps[3] or Q.ne > caps[4]):
        info["status"] = E_CAPACITY
        return res
    for e in range(P.ne):
        if not (0 <= P.e_kf[e] < P.nkf and 0 <= P.e_pt[e] < P.nmp):
            info["status"] = E_INVALID
            return res
    for e in range(Q.ne):
        if not (0 <= Q.e_kf[e] < P.nkf and 0 <= Q.e_lil[e] < Q.n):
            info["status"] = E_INVALID
            return res
    if len({(P.e_pt[e], P.e_kf[e]) for e in range(P.ne)}) != P.ne or len({(Q.e_lil[e], Q.e_kf[e]) for e in range(Q.ne)}) != Q.ne:
        info["status"] = E_INVALID
        return res
    if P.ne + Q.ne == 0 or all(P.fixed):
        return res
    Q.lists(P.nkf)
    CP = _Combined(P, Q)
    ne, nland = P.ne, P.nmp + Q.n

    T = [from_pose(P.kf["Tcw"][k]) for k in range(P.nkf)]
    X = [[float(P.mp[k][p]) for k in ("x", "y", "z")] for p in range(P.nmp)]
    L = [[float(v) for v in Q.lil["w"][j]] for j in range(Q.n)]
    level = [False] * (ne + Q.ne)                    # by global edge index
    err = [[0.0, 0.0, 0.0] for _ in range(ne)] + [[0.0] * 6 for _ in range(Q.ne)]
    rho0 = [0.0] * (ne + Q.ne)

    def evaluate(Tx, Xx, Lx, robust, linearize):
        rows = {}
        for e in range(ne):
            if level[e]:
                continue
            Pc = P.camera_point(e, Tx, Xx)
            er = P.error(e, Pc)
            c = P.chi2(e, er)
            r0, r1 = P.huber(e, c) if robust else (c, 1.0)
            err[e], rho0[e] = er, r0
            if linearize:
                Jp, Jl = P.jacobians(e, Pc, _quat_to_R(Tx[P.e_kf[e]][0]))
                rows[e] = (Jp, Jl, r1 * P.is2[e])
        for e in range(Q.ne):
            if level[ne + e]:
                continue
            er = Q.error(e, Tx, Lx)
            c = Q.chi2(er)
            r0, r1 = Q.huber(c) if robust else (c, 1.0)
            err[ne + e], rho0[ne + e] = er, r0
            if linearize:
                Jp, Jl = Q.jacobians(e, Tx, Lx)
                rows[ne + e] = (Jp, Jl, r1 * LIL_INFO)
        return rows

    def chi_active():
        return _sum256(rho0, [not l for l in level])

    chi_start, chi_r, its_r = 0.0, [0.0, 0.0], [0, 0]
    with np.errstate(all="ignore"):
        for r in range(rounds):
            robust = r == 0
            tr = {"level": level[:ne], "llevel": level[ne:], "trials": [], "updates": [], "its": 0, "stopped": "iterations"}
            in_sys = [not P.fixed[k] and (any(not level[e] for e in P.kf_edges[k]) or any(not level[ne + e] for e in Q.kf_edges[k]))
                      for k in range(P.nkf)]
            pact = [any(not level[e] for e in CP.pt_edges[p]) for p in range(nland)]
            active = [j for j in range(Q.n) if pact[P.nmp + j]]
            kfof = [k for k in range(P.nkf) if in_sys[k]]
            pidx = {k: i for i, k in enumerate(kfof)}
            F = len(kfof)
            N = 6 * F
            tr.update(F=F, in_system=in_sys, pact=pact[:P.nmp], lact=pact[P.nmp:])
            first, last = 0.0, (chi_r[0] if r else 0.0)
            if F == 0:
                evaluate(T, X, L, robust, False)
                first = last = chi_active()
            lam, ni, nbad = 0.0, 2.0, 0
            for it in range((5 if r == 0 else 10) if F else 0):
                rows = evaluate(T, X, L, robust, True)
                chi = chi_active()
                ini_chi = chi
                if it == 0:
                    first = chi
                Hpp, bp = [[0.0] * 21 for _ in range(F)], [0.0] * N
                for i, k in enumerate(kfof):         # a keyframe's point edges and then its LIL edges: ascending global edge index
                    acc = [0.0] * 27
                    for e in P.kf_edges[k]:
                        if not level[e]:
                            acc = [a + b for a, b in zip(acc, _quad(rows[e][0], 6, rows[e][2], P.mono[e], err[e]))]
                    for e in Q.kf_edges[k]:
                        if not level[ne + e]:
                            acc = [a + b for a, b in zip(acc, _quad6(rows[ne + e][0], 6, rows[ne + e][2], err[ne + e]))]
                    Hpp[i] = acc[:21]
                    bp[6 * i:6 * i + 6] = [-a for a in acc[21:]]
                Hll, bl = [[0.0] * 6 for _ in range(nland)], [[0.0] * 3 for _ in range(nland)]
                for p in range(nland):
                    if pact[p]:
                        acc = [0.0] * 9
                        for e in CP.pt_edges[p]:
                            if not level[e]:
                                q = _quad(rows[e][1], 3, rows[e][2], P.mono[e], err[e]) if e < ne else _quad6(rows[e][1], 3, rows[e][2], err[e])
                                acc = [a + b for a, b in zip(acc, q)]
                        Hll[p], bl[p] = acc[:6], [-a for a in acc[6:]]
                B = {}
                for e, (Jp, Jl, w) in rows.items():
                    if CP.e_kf[e] in pidx:
                        blk = [[0.0] * 3 for _ in range(6)]
                        for rr in range(6):
                            for m in range(3):
                                if e < ne:
                                    s = (w * Jp[0][rr]) * Jl[0][m] + (w * Jp[1][rr]) * Jl[1][m]
                                    blk[rr][m] = s if P.mono[e] else s + (w * Jp[2][rr]) * Jl[2][m]
                                else:
                                    s = (w * Jp[0][rr]) * Jl[0][m]
                                    for a in range(1, 6):
                                        s = s + (w * Jp[a][rr]) * Jl[a][m]
                                    blk[rr][m] = s
                        B[e] = blk
                if it == 0:
                    m = 0.0
                    for i in range(F):
                        for j in range(6):
                            a = abs(Hpp[i][_tri(6, j, j)])
                            m = m if a < m else a
                    for p in range(nland):
                        if pact[p]:
                            for j in range(3):
                                a = abs(Hll[p][_tri(3, j, j)])
                                m = m if a < m else a
                    lam, ni, nbad = 1e-5 * m, 2.0, 0
                rho, qmax = 0.0, 0
                while True:
                    step, why = _solve(CP, F, kfof, pidx, pact, level, Hpp, bp, Hll, bl, B, lam)
                    temp_chi, scale = DBL_MAX, 0.0
                    if step is not None:
                        xp, xl = step
                        Tn, Xn = list(T), [list(x) for x in X]
                        for i, k in enumerate(kfof):
                            Tn[k] = se3_mul(se3_exp(xp[6 * i:6 * i + 6]), T[k])
                        for p in range(P.nmp):
                            if pact[p]:
                                Xn[p] = [X[p][j] + xl[p][j] for j in range(3)]
                        xl_of = {j: xl[P.nmp + j] for j in active}
                        Ln = lil_update(L, xl_of, active)
                        tr["updates"].append((list(active), xl_of, [list(w) for w in L], [list(w) for w in Ln]))
                        evaluate(Tn, Xn, Ln, robust, False)
                        temp_chi = chi_active()
                        for j in range(N):
                            scale = scale + xp[j] * (lam * xp[j] + bp[j])
                        for p in range(nland):
                            if pact[p]:
                                for j in range(3):
                                    scale = scale + xl[p][j] * (lam * xl[p][j] + bl[p][j])
                    scale = scale + 1e-3
                    rho = _div(chi - temp_chi, scale)
                    tr["trials"].append((it, step is not None, why, rho, lam))
                    if rho > 0 and _finite(temp_chi):
                        t = 2.0 * rho - 1.0
                        alpha = 1.0 - (t * t) * t
                        alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
                        lam = lam * (alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0))
                        ni, chi = 2.0, temp_chi
                        if step is not None:
                            T, X, L = Tn, Xn, Ln
                    else:
                        lam = lam * ni
                        ni = ni * 2.0
                    qmax += 1
                    if not (rho < 0 and qmax < 10):
                        break
                tr["its"] += 1
                last = chi
                if qmax == 10 or rho == 0:
                    tr["stopped"] = "terminate"
                    break
                nbad = nbad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
                if nbad >= 3:
                    tr["stopped"] = "nbad"
                    break
            its_r[r] = tr["its"]
            if r == 0:
                chi_start = first
            chi_r[r] = last
            bad = []
            for e in range(ne):
                c = P.chi2(e, err[e])
                z = P.camera_point(e, T, X)[2]
                bad.append(bool(c > (bc.CHI2_MONO if P.mono[e] else bc.CHI2_STEREO)) or not (z > 0.0))
            tr["chi2_lil"] = [Q.chi2(err[ne + e]) for e in range(Q.ne)]
            tr["depth_bad_lil"] = [not Q.depth_positive(e, T, L) for e in range(Q.ne)]
            bad_lil = [bool(c > CHI2_LIL) or d for c, d in zip(tr["chi2_lil"], tr["depth_bad_lil"])]
            tr["bad"], tr["bad_lil"] = bad, bad_lil
            tr["X"], tr["T"], tr["L"] = [list(x) for x in X], list(T), [list(w) for w in L]
            res["trace"].append(tr)
            if r + 1 == rounds:
                res["erase"], res["erase_lil"] = np.array(bad, np.uint8), np.array(bad_lil, np.uint8).reshape(-1)
            else:
                level = bad + bad_lil
    for k in range(P.nkf):
        if not P.fixed[k]:
            res["kf"]["Tcw"][k] = to_pose(T[k])
    for p in range(P.nmp):
        for j, nm in enumerate(("x", "y", "z")):
            res["mp"][nm][p] = np.float64(X[p][j]).astype(np.float32)
    for j in range(Q.n):
        res["lil"]["w"][j] = L[j]
    info["rounds"], info["iterations"][0], info["iterations"][1] = rounds, its_r[0], its_r[1]
    info["nerased"] = int(res["erase"].sum())
    res["nerased_lil"] = int(res["erase_lil"].sum())
    info["chi2_start"], info["chi2_round1"], info["chi2_end"] = chi_start, chi_r[0], chi_r[rounds - 1]
    return res


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
LIL_NOISE_PX = 0.5           # on the projected end points and the crossing
LIL_OUTLIER_PX = (80.0, 160.0)   # a planted outlier: with the information 0.01 an edge needs about 33 px of error to pass 11.07


def _observe(w, R, t, cam, rng=None, shift=None):
    """the observation of the LIL w [15] from (R, t): the lines through the (noisy) projections of its segments and the crossing"""
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    P2 = []
    for m in range(5):
        Pc = R @ w[3 * m:3 * m + 3] + t
        P2.append(np.array([Pc[0] / Pc[2] * fx + cx, Pc[1] / Pc[2] * fy + cy]))
    if rng is not None:
        P2 = [p + rng.normal(size=2) * LIL_NOISE_PX for p in P2]
    if shift is not None:
        P2 = [p + shift for p in P2]
    return _line_eq(P2[0][None], P2[1][None])[0], _line_eq(P2[2][None], P2[3][None])[0], P2[4]


def plant_lils(c, seed, nlil, nobs=3, noise=True, dw=0.02, outliers=()):
    """nlil LILs in the scene c of ba_cases.make_scene: two coplanar 3-D segments through a crossing inside the point cloud, each 0.2 to
    0.5 m to one side of it and 0.3 to 0.7 m to the other, seen by nobs keyframes (a seeded choice in a seeded order, as
    GetObservations() iterates in pointer order) with LIL_NOISE_PX of noise; the start is the truth plus dw of noise per double.
    outliers: (lil, k-th observation) pairs moved by LIL_OUTLIER_PX.  -> the scene with lil, lil_true, ledges, planted_lil"""
    rng = np.random.default_rng(seed + 900000)
    nkf = len(c["kf"])
    true = np.zeros(nlil, MAPLIL_DTYPE)
    rows, planted = [], []
    for j in range(nlil):
        C = np.array([0.0, 0.0, 6.0]) + rng.uniform(-1.0, 1.0, 3)
        pts = []
        for _ in range(2):
            d = rng.normal(size=3) * np.array([1.0, 1.0, 0.3])
            d /= np.linalg.norm(d)
            pts += [C - rng.uniform(0.2, 0.5) * d, C + rng.uniform(0.3, 0.7) * d]
        true["w"][j] = np.concatenate(pts + [C])
        ks = rng.permutation(nkf)[:min(nobs, nkf)]
        for i, k in enumerate(ks):
            R = c["kf_true"]["Tcw"]["R"][k].astype(np.float64).reshape(3, 3)
            t = c["kf_true"]["Tcw"]["t"][k].astype(np.float64)
            shift = None
            if (j, i) in outliers:
                ang, mag = rng.uniform(0, 2 * math.pi), rng.uniform(*LIL_OUTLIER_PX)
                shift = np.array([mag * math.cos(ang), mag * math.sin(ang)])
            o1, o2, ins = _observe(true["w"][j], R, t, c["cam"], rng if noise else None, shift)
            rows.append((j, int(k), o1, o2, ins))
            planted.append(shift is not None)
    c = dict(c)
    c["lil_true"] = true
    c["lil"] = true.copy()
    c["lil"]["w"] += rng.normal(size=(nlil, 15)) * dw
    c["ledges"] = np.array(rows, LILEDGE_DTYPE).reshape(-1) if rows else np.zeros(0, LILEDGE_DTYPE)
    c["planted_lil"] = np.array(planted, np.uint8)
    return c


def _true_ledge(c, j, k):
    R = c["kf_true"]["Tcw"]["R"][k].astype(np.float64).reshape(3, 3)
    t = c["kf_true"]["Tcw"]["t"][k].astype(np.float64)
    o1, o2, ins = _observe(c["lil_true"]["w"][j], R, t, c["cam"])
    return (j, k, o1, o2, ins)


def _add_ledges(c, rows):
    c = dict(c)
    c["ledges"] = np.concatenate([c["ledges"], np.array(rows, LILEDGE_DTYPE).reshape(-1)])
    c["planted_lil"] = np.concatenate([c["planted_lil"], np.zeros(len(rows), np.uint8)])
    return c


SHAPES = {   # name -> (seed, nfree, nfixed, npts, kind, point outliers, nedges, nlil, observations per LIL)
    "f2_x1_p6_l1": (701, 2, 1, 6, "mixed", 0.0, None, 1, 2),          # the smallest: 1 LIL with 2 edges
    "f2_x1_p8_l4": (702, 2, 1, 8, "mixed", 0.0, None, 4, 3),          # the update: 4 active LILs - every follower past the end but one chain
    "f2_x1_p8_l5": (703, 2, 1, 8, "stereo", 0.0, None, 5, 3),         # 5: the first LIL has all four followers
    "f2_x2_p8_l6": (704, 2, 2, 8, "mono", 0.0, None, 6, 3),
    "f5_x3_p40_l8": (705, 5, 3, 40, "mixed", 0.3, None, 8, 4),        # the mixed scene
    "caps_8_64_256_8_32": (706, 5, 3, 64, "mixed", 0.2, 256, 8, 4),   # every count at the caps
    "p0_l3": (707, 2, 1, 0, "mixed", 0.0, None, 3, 3),                # no map point at all (the reference would index an empty vector, :2247)
}
CAPS = (8, 64, 256, 8, 32)
CAPS_WIDE = (16, 128, 512, 16, 64)
EDGE_CASES = ["lil_level1", "lil_depth_only", "lil_only_fixed", "lil_no_edges", "lil_middle_inactive", "lil_rounds_1"]
CASE_NAMES = list(SHAPES) + EDGE_CASES


def _edge_case(name):
    if name == "lil_level1":                 # one observation of LIL 1 is 80 .. 160 px off: on level 1 after round one, erased by its chi2
        return plant_lils(make_scene(801, 3, 1, 10, "mixed"), 801, 3, 3, outliers=((1, 0),))
    if name == "lil_depth_only":             # a fixed keyframe that looks away sees LIL 0 behind it, where it projects to
        c = make_scene(802, 2, 1, 10, "stereo", noise=False, rot_deg=0.2, dt=0.005, dpt=0.01)
        R, t = bc._arc_pose(0.1)
        flip = np.diag([-1.0, 1.0, -1.0])
        c = bc._extend(c, kf_rows=[(flip @ R, flip @ t, 1)])
        c = plant_lils(c, 802, 2, 2, noise=False, dw=0.002)
        c["ledges"] = c["ledges"][c["ledges"]["kf"] != len(c["kf"]) - 1]
        c["planted_lil"] = np.zeros(len(c["ledges"]), np.uint8)
        c = _add_ledges(c, [_true_ledge(c, 0, len(c["kf"]) - 1)])
        c["behind_edge"] = len(c["ledges"]) - 1
        return c
    if name == "lil_only_fixed":             # LIL 0 is seen by the two fixed keyframes alone
        c = plant_lils(make_scene(803, 2, 2, 10, "mixed"), 803, 3, 3)
        c["ledges"] = c["ledges"][c["ledges"]["lil"] != 0]
        c["planted_lil"] = np.zeros(len(c["ledges"]), np.uint8)
        return _add_ledges(c, [_true_ledge(c, 0, 2), _true_ledge(c, 0, 3)])
    if name == "lil_no_edges":               # LIL 1 of 3 has no edge: it is not in the system and comes back as it went in
        c = plant_lils(make_scene(804, 2, 1, 8, "mixed"), 804, 3, 3)
        c["ledges"] = c["ledges"][c["ledges"]["lil"] != 1]
        c["planted_lil"] = np.zeros(len(c["ledges"]), np.uint8)
        return c
    if name == "lil_middle_inactive":        # LIL 2 of 6 is seen only by two fixed keyframes that look away: both its edges go to level 1
        c = make_scene(805, 3, 1, 10, "mixed")                                     # for their depth, and it is inactive in round two
        flip = np.diag([-1.0, 1.0, -1.0])
        c = bc._extend(c, kf_rows=[(flip @ R, flip @ t, 1) for R, t in (bc._arc_pose(0.1), bc._arc_pose(-0.2))])
        c = plant_lils(c, 805, 6, 3)
        nkf = len(c["kf"])
        e = c["ledges"]
        c["ledges"] = e[(e["kf"] < nkf - 2) & (e["lil"] != 2)]
        c["planted_lil"] = np.zeros(len(c["ledges"]), np.uint8)
        return _add_ledges(c, [_true_ledge(c, 2, nkf - 2), _true_ledge(c, 2, nkf - 1)])
    if name == "lil_rounds_1":
        return bc._with(plant_lils(make_scene(806, 2, 1, 10, "mixed", outliers=0.3), 806, 4, 3, outliers=((0, 1),)), rounds=1)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case with its reference: dict(kf, mp, edges, lil, ledges, cam, rounds, ref = local_ba(...))."""
    if name in SHAPES:
        seed, nfree, nfixed, npts, kind, out, nedges, nlil, nobs = SHAPES[name]
        c = plant_lils(make_scene(seed, nfree, nfixed, npts, kind, outliers=out, nedges=nedges), seed, nlil, nobs)
    else:
        c = _edge_case(name)
    c.setdefault("rounds", 2)
    c["ref"] = local_ba(c["kf"], c["mp"], c["edges"], c["lil"], c["ledges"], c["cam"], c["rounds"])
    return c


def without_lils(c):
    """the point part of a case, with empty LIL arrays"""
    return dict(c, lil=np.zeros(0, MAPLIL_DTYPE), ledges=np.zeros(0, LILEDGE_DTYPE))


# ---- the files of tools/dropin/ba_lil_main.cpp -----------------------------------------------------------------------------------------
def write_cases(path, cases, rounds, caps):
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", len(cases), rounds, *caps))
        f.write(bc.camera_record(cases[0]["cam"] if cases else bc.camera()).tobytes())
        for c in cases:
            f.write(struct.pack("<5i", len(c["kf"]), len(c["mp"]), len(c["edges"]), len(c["lil"]), len(c["ledges"])))
            for key, dt in (("kf", KF_DTYPE), ("mp", MP_DTYPE), ("edges", EDGE_DTYPE), ("lil", MAPLIL_DTYPE), ("ledges", LILEDGE_DTYPE)):
                f.write(np.ascontiguousarray(c[key], dt).tobytes())


def read_sections(path, cases, nsections):
    """-> [section][case] dict(info, kf, mp, erase, lil, erase_lil, nerased_lil)"""
    buf = open(path, "rb").read()
    at, out = 0, []
    for _ in range(nsections):
        sec = []
        for c in cases:
            r = {}
            for key, dt, n in (("info", INFO_DTYPE, 1), ("kf", KF_DTYPE, len(c["kf"])), ("mp", MP_DTYPE, len(c["mp"])), ("erase", np.uint8, len(c["edges"])),
                               ("lil", MAPLIL_DTYPE, len(c["lil"])), ("erase_lil", np.uint8, len(c["ledges"])), ("nerased_lil", np.int32, 1)):
                dt = np.dtype(dt)
                r[key] = np.frombuffer(buf, dt, n, at).copy()
                at += n * dt.itemsize
            r["info"], r["nerased_lil"] = r["info"][0], int(r["nerased_lil"][0])
            sec.append(r)
        out.append(sec)
    assert at == len(buf), (at, len(buf))
    return out


def assert_equal_ref(got, ref, what):
    """bit for bit: what ba_cases.assert_equal_ref compares, the 15 doubles (and the copied bytes) of every LIL, the LIL erase flags"""
    bc.assert_equal_ref(got, ref, what)
    assert np.ascontiguousarray(got["lil"], MAPLIL_DTYPE).tobytes() == np.ascontiguousarray(ref["lil"], MAPLIL_DTYPE).tobytes(), what
    assert np.asarray(got["erase_lil"], np.uint8).tobytes() == np.asarray(ref["erase_lil"], np.uint8).tobytes(), what
    if got.get("nerased_lil") is not None:
        assert int(got["nerased_lil"]) == int(ref["nerased_lil"]), what
