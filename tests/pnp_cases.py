"""PnPsolver (src/PnPsolver.cc) restated in Python floats and numpy, rounding by rounding, next to psl-slam_amd/csrc/pnp_solver_kernels.h
(which says where each step comes from and lists this library's readings of the OpenCV calls), and the cases the tests share.

Python's float is the IEEE double and its + - * / and math.sqrt are single correctly rounded operations; float32 steps go through
numpy.float32.  A sum over the rows of one entry is always taken row by row; where numpy arrays are used they run across entries
(elementwise), never across rows.  The solver is an object that lives across calls of iterate(), as the reference's does: its rand()
stream is never reseeded, so the kernel's reseed-and-skip is checked against a stream that simply goes on.

USE_LAPACK = True replaces the Jacobi-based calls (cvSVD, cvInvert, cvSolve) by numpy.linalg.svd / pinv / lstsq: an independent check
of the Jacobi reading, not bit for bit."""
import math

import numpy as np

from sim3_solver_cases import GlibcRand, draw, random_int, same_floats  # noqa: F401  (glibc's generator and the draw are restated once)

F = np.float32
POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,))])
ROW_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("X", "<f4"), ("Y", "<f4"), ("Z", "<f4"), ("sigma2", "<f4")])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("inliers", "<i4"), ("best_inliers", "<i4"), ("min_inliers", "<i4"),
                         ("Tcw", POSE_DTYPE), ("best_Tcw", POSE_DTYPE)])
assert ROW_DTYPE.itemsize == 24 and RESULT_DTYPE.itemsize == 116
DBL_EPSILON = 2.220446049250313e-16
DBL_MIN = 2.2250738585072014e-308
NAN = float("nan")
USE_LAPACK = False
# Relocalization's parameters (src/Tracking.cc:2076) and the constructor's defaults (include/PnPsolver.h:70)
RELOC = dict(prob=0.99, min_inliers=10, max_its=300, min_set=4, epsilon=0.5, th2=5.991)
DEFAULT = dict(prob=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4, th2=5.991)
CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)


def _div(a, b):
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else NAN


# ---- SetRansacParameters (:121-152) ---------------------------------------------------------------------------------------------------
def ransac_parameters(N, prob, min_inliers, max_its, min_set, epsilon):
    """-> (mRansacMaxIts, mRansacMinInliers)"""
    eps = F(epsilon)
    n_min = int(F(N) * eps)
    n_min = max(n_min, min_inliers, min_set)
    if N < 1:
        return 1, n_min
    with np.errstate(all="ignore"):
        if eps < F(n_min) / F(N):
            eps = F(n_min) / F(N)
    if n_min == N:
        n = 1
    else:
        x = 1 - math.pow(float(eps), 3)             # pow(float, int) is the double pow
        den = math.log(x) if x > 0 else (-math.inf if x == 0 else NAN)
        ratio = _div(math.log(1 - prob), den)
        v = math.ceil(ratio) if math.isfinite(ratio) else ratio
        n = int(v) if (v == v and -1.0 < v < max_its) else max_its   # a NaN, infinite or negative ratio counts as max_its
    return max(1, min(n, max_its)), n_min


# ---- this library's reading of JacobiSVDImpl_<double> ------------------------------------------------------------------------------------
def jacobi_rows(At, want_v):
    """At: n lists of length m, changed in place into U^T (rows normalised); -> (w descending, Vt or None)"""
    W, Vt = jacobi_sweeps(At, want_v)
    for i in range(len(At)):
        s = _div(1.0, W[i]) if W[i] > DBL_MIN else 0.0
        At[i] = [t * s for t in At[i]]
    return W, Vt


def jacobi_sweeps(At, want_v):
    """jacobi_rows before its normalisation: the rows of At are left as the rotations and the sort leave them"""
    n, m = len(At), len(At[0])
    eps = DBL_EPSILON * 10
    W = []
    for i in range(n):
        sd = 0.0
        for t in At[i]:
            sd = sd + t * t
        W.append(sd)
    Vt = [[1.0 if k == i else 0.0 for k in range(n)] for i in range(n)] if want_v else None
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                ri, rj = At[i], At[j]
                a, b, p = W[i], W[j], 0.0
                for k in range(m):
                    p = p + ri[k] * rj[k]
                if abs(p) <= eps * _sqrt(a * b):
                    continue
                p = p * 2
                beta = a - b
                gamma = _sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = _sqrt(_div(delta, gamma))
                    c = _div(p, (gamma * s) * 2)
                else:
                    c = _sqrt(_div(gamma + beta, gamma * 2))
                    s = _div(p, (gamma * c) * 2)
                a = b = 0.0
                for k in range(m):
                    x, y = ri[k], rj[k]
                    t0 = c * x + s * y
                    t1 = -s * x + c * y
                    ri[k], rj[k] = t0, t1
                    a = a + t0 * t0
                    b = b + t1 * t1
                W[i], W[j] = a, b
                changed = True
                if want_v:
                    vi, vj = Vt[i], Vt[j]
                    for k in range(n):
                        x, y = vi[k], vj[k]
                        vi[k], vj[k] = c * x + s * y, -s * x + c * y
        if not changed:
            break
    for i in range(n):
        sd = 0.0
        for t in At[i]:
            sd = sd + t * t
        W[i] = _sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            if want_v:
                Vt[i], Vt[j] = Vt[j], Vt[i]
    return W, Vt


def _threshold(W):
    t = 0.0
    for w in W:
        t = t + w
    return t * (DBL_EPSILON * 2)


def svd_ut(A):
    """cvSVD(A, W, Ut, 0, MODIFY_A | U_T) on a square matrix (lists): -> (w, Ut rows)"""
    n = len(A)
    if USE_LAPACK:
        U, s, _ = np.linalg.svd(np.array(A, np.float64))
        return list(s), [list(U[:, i]) for i in range(n)]
    At = [[A[j][i] for j in range(n)] for i in range(n)]
    W, _ = jacobi_rows(At, False)
    return W, At


def invert3(A):
    """cvInvert(A, Ainv, CV_SVD) on 3x3"""
    if USE_LAPACK:
        return [list(r) for r in np.linalg.pinv(np.array(A, np.float64), rcond=2 * DBL_EPSILON)]
    At = [[A[j][i] for j in range(3)] for i in range(3)]
    W, Vt = jacobi_rows(At, True)
    thr = _threshold(W)
    X = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        if abs(W[i]) <= thr:
            continue
        wi = _div(1.0, W[i])
        for r in range(3):
            for c in range(3):
                X[r][c] = X[r][c] + Vt[i][r] * (At[i][c] * wi)
    return X


def solve6(L, cols, rho):
    """cvSolve(L[:, cols], rho, x, CV_SVD)"""
    n = len(cols)
    if USE_LAPACK:
        A = np.array([[L[j][c] for c in cols] for j in range(6)], np.float64)
        return list(np.linalg.lstsq(A, np.array(rho, np.float64), rcond=None)[0])
    At = [[L[j][cols[i]] for j in range(6)] for i in range(n)]
    W, Vt = jacobi_rows(At, True)
    thr = _threshold(W)
    x = [0.0] * n
    for i in range(n):
        if abs(W[i]) <= thr:
            continue
        wi = _div(1.0, W[i])
        s = 0.0
        for j in range(6):
            s = s + At[i][j] * rho[j]
        s = s * wi
        for j in range(n):
            x[j] = x[j] + s * Vt[i][j]
    return x


def svd_uv3(A):
    """cvSVD(A, W, U, V, MODIFY_A) on 3x3: -> U, V as row-indexed matrices"""
    if USE_LAPACK:
        U, _, Vt = np.linalg.svd(np.array(A, np.float64))
        return [list(r) for r in U], [list(r) for r in Vt.T]
    At = [[A[j][i] for j in range(3)] for i in range(3)]
    _, Vt = jacobi_rows(At, True)
    return [[At[k][i] for k in range(3)] for i in range(3)], [[Vt[k][j] for k in range(3)] for j in range(3)]


# ---- compute_pose (:477-525) -------------------------------------------------------------------------------------------------------------
def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


_TRI12 = [(p, q) for p in range(12) for q in range(p, 12)]
_TP = np.array([p for p, _ in _TRI12])
_TQ = np.array([q for _, q in _TRI12])
_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def qr_solve(A, b, x):
    """qr_solve (:860-950) on 6x4 lists, in place; x keeps its values on the early return"""
    nr, nc = 6, 4
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        eta = abs(A[k][k])
        for i in range(k + 1, nr):
            elt = abs(A[i - 1][k])        # the reference's pointer is one row behind its index
            if eta < elt:
                eta = elt
        if eta == 0:
            return
        s = 0.0
        inv_eta = _div(1.0, eta)
        for i in range(k, nr):
            A[i][k] = A[i][k] * inv_eta
            s = s + A[i][k] * A[i][k]
        sigma = _sqrt(s)
        if A[k][k] < 0:
            sigma = -sigma
        A[k][k] = A[k][k] + sigma
        A1[k] = sigma * A[k][k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s = s + A[i][k] * A[i][j]
            tau = _div(s, A1[k])
            for i in range(k, nr):
                A[i][j] = A[i][j] - tau * A[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau = tau + A[i][j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i][j]
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s = s + A[i][j] * x[j]
        x[i] = _div(b[i] - s, A2[i])


def gauss_newton(L, rho, betas):
    x = [0.0] * 4   # the reference's x[4] is not initialised; the library starts it at 0
    for _ in range(5):
        b0, b1, b2, b3 = betas
        A, b = [], []
        for i in range(6):
            l = L[i]
            A.append([(((2 * l[0]) * b0 + l[1] * b1) + l[3] * b2) + l[6] * b3,
                      ((l[1] * b0 + (2 * l[2]) * b1) + l[4] * b2) + l[7] * b3,
                      ((l[3] * b0 + l[4] * b1) + (2 * l[5]) * b2) + l[8] * b3,
                      ((l[6] * b0 + l[7] * b1) + l[8] * b2) + (2 * l[9]) * b3])
            s = (l[0] * b0) * b0
            for t in ((l[1] * b0) * b1, (l[2] * b1) * b1, (l[3] * b0) * b2, (l[4] * b1) * b2, (l[5] * b2) * b2, (l[6] * b0) * b3,
                      (l[7] * b1) * b3, (l[8] * b2) * b3, (l[9] * b3) * b3):
                s = s + t
            b.append(rho[i] - s)
        qr_solve(A, b, x)
        for i in range(4):
            betas[i] = betas[i] + x[i]


def betas_approx(L, rho, which):
    if which == 1:
        b = solve6(L, (0, 1, 3, 6), rho)
        if b[0] < 0:
            t0 = _sqrt(-b[0])
            return [t0, _div(-b[1], t0), _div(-b[2], t0), _div(-b[3], t0)]
        t0 = _sqrt(b[0])
        return [t0, _div(b[1], t0), _div(b[2], t0), _div(b[3], t0)]
    b = solve6(L, (0, 1, 2) if which == 2 else (0, 1, 2, 3, 4), rho)
    if b[0] < 0:
        t0 = _sqrt(-b[0])
        t1 = _sqrt(-b[2]) if b[2] < 0 else 0.0
    else:
        t0 = _sqrt(b[0])
        t1 = _sqrt(b[2]) if b[2] > 0 else 0.0
    if b[1] < 0:
        t0 = -t0
    return [t0, t1, _div(b[3], t0) if which == 3 else 0.0, 0.0]


def compute_pose(pws, us, cam):
    """pws [n][3], us [n][2] (Python floats) -> (R [3][3], t [3]) in double"""
    n = len(pws)
    fu, fv, uc, vc = cam
    dn = float(n)
    # choose_control_points
    c0 = [0.0, 0.0, 0.0]
    for p in pws:
        for j in range(3):
            c0[j] = c0[j] + p[j]
    c0 = [_div(c, dn) for c in c0]
    pw0 = [[p[j] - c0[j] for j in range(3)] for p in pws]
    PtP = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            s = 0.0
            for r in pw0:
                s = s + r[a] * r[b]
            PtP[a][b] = PtP[b][a] = s
    dc, uct = svd_ut(PtP)
    cws = [c0]
    for i in range(1, 4):
        k = _sqrt(_div(dc[i - 1], dn))
        cws.append([c0[j] + k * uct[i - 1][j] for j in range(3)])
    # compute_barycentric_coordinates
    cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
    ci = invert3(cc)
    alphas = []
    for p in pws:
        d = [p[0] - c0[0], p[1] - c0[1], p[2] - c0[2]]
        a = [0.0] + [(ci[j][0] * d[0] + ci[j][1] * d[1]) + ci[j][2] * d[2] for j in range(3)]
        a[0] = ((1.0 - a[1]) - a[2]) - a[3]
        alphas.append(a)
    # fill_M, cvMulTransposed: the 78 entries side by side, the rows of M one after the other
    acc = np.zeros(78)
    with np.errstate(all="ignore"):
        for a, (u, v) in zip(alphas, us):
            M1, M2 = np.zeros(12), np.zeros(12)
            for i in range(4):
                M1[3 * i], M1[3 * i + 2] = a[i] * fu, a[i] * (uc - u)
                M2[3 * i + 1], M2[3 * i + 2] = a[i] * fv, a[i] * (vc - v)
            acc = acc + M1[_TP] * M1[_TQ]
            acc = acc + M2[_TP] * M2[_TQ]
    MtM = [[0.0] * 12 for _ in range(12)]
    for (p, q), v in zip(_TRI12, acc):
        MtM[p][q] = MtM[q][p] = float(v)
    _, ut = svd_ut(MtM)
    # compute_L_6x10, compute_rho
    L, rho = [], []
    for a, b in _PAIRS:
        dv = [[ut[11 - v][3 * a + k] - ut[11 - v][3 * b + k] for k in range(3)] for v in range(4)]
        L.append([_dot3(dv[0], dv[0]), 2.0 * _dot3(dv[0], dv[1]), _dot3(dv[1], dv[1]), 2.0 * _dot3(dv[0], dv[2]), 2.0 * _dot3(dv[1], dv[2]),
                  _dot3(dv[2], dv[2]), 2.0 * _dot3(dv[0], dv[3]), 2.0 * _dot3(dv[1], dv[3]), 2.0 * _dot3(dv[2], dv[3]), _dot3(dv[3], dv[3])])
        e = [cws[a][k] - cws[b][k] for k in range(3)]
        rho.append((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    best = None
    for which in (1, 2, 3):
        betas = betas_approx(L, rho, which)
        gauss_newton(L, rho, betas)
        # compute_ccs, compute_pcs, solve_for_sign
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            v = ut[11 - i]
            for j in range(4):
                for k in range(3):
                    ccs[j][k] = ccs[j][k] + betas[i] * v[3 * j + k]
        pcs = [[((a[0] * ccs[0][j] + a[1] * ccs[1][j]) + a[2] * ccs[2][j]) + a[3] * ccs[3][j] for j in range(3)] for a in alphas]
        if pcs[0][2] < 0.0:
            pcs = [[-x for x in pc] for pc in pcs]
        # estimate_R_and_t
        pc0, pw0m = [0.0] * 3, [0.0] * 3
        for pc, pw in zip(pcs, pws):
            for j in range(3):
                pc0[j] = pc0[j] + pc[j]
                pw0m[j] = pw0m[j] + pw[j]
        pc0 = [_div(x, dn) for x in pc0]
        pw0m = [_div(x, dn) for x in pw0m]
        abt = [[0.0] * 3 for _ in range(3)]
        for pc, pw in zip(pcs, pws):
            for j in range(3):
                for c in range(3):
                    abt[j][c] = abt[j][c] + (pc[j] - pc0[j]) * (pw[c] - pw0m[c])
        U, V = svd_uv3(abt)
        R = [[_dot3(U[i], V[j]) for j in range(3)] for i in range(3)]
        det = (((((R[0][0] * R[1][1]) * R[2][2] + (R[0][1] * R[1][2]) * R[2][0]) + (R[0][2] * R[1][0]) * R[2][1]) - (R[0][2] * R[1][1]) * R[2][0]) -
               (R[0][1] * R[1][0]) * R[2][2]) - (R[0][0] * R[1][2]) * R[2][1]
        if det < 0:
            R[2] = [-x for x in R[2]]
        t = [pc0[i] - _dot3(R[i], pw0m) for i in range(3)]
        # reprojection_error
        sum2 = 0.0
        for pw, (u, v) in zip(pws, us):
            Xc = _dot3(R[0], pw) + t[0]
            Yc = _dot3(R[1], pw) + t[1]
            inv_Zc = _div(1.0, _dot3(R[2], pw) + t[2])
            ue = uc + (fu * Xc) * inv_Zc
            ve = vc + (fv * Yc) * inv_Zc
            sum2 = sum2 + _sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve))
        err = _div(sum2, dn)
        if best is None or err < best[0]:
            best = (err, R, t)
    return best[1], best[2]


# ---- CheckInliers (:308-339) over all rows, elementwise -----------------------------------------------------------------------------------
def check_inliers(rows, maxerr, R, t, cam):
    fu, fv, uc, vc = cam
    x, y, z = (rows[k].astype(np.float64) for k in ("X", "Y", "Z"))
    with np.errstate(all="ignore"):
        Xc = (((R[0][0] * x + R[0][1] * y) + R[0][2] * z) + t[0]).astype(F)
        Yc = (((R[1][0] * x + R[1][1] * y) + R[1][2] * z) + t[1]).astype(F)
        invZc = (1.0 / (((R[2][0] * x + R[2][1] * y) + R[2][2] * z) + t[2])).astype(F)
        ue = uc + (fu * Xc.astype(np.float64)) * invZc.astype(np.float64)
        ve = vc + (fv * Yc.astype(np.float64)) * invZc.astype(np.float64)
        dX = (rows["u"].astype(np.float64) - ue).astype(F)
        dY = (rows["v"].astype(np.float64) - ve).astype(F)
        err2 = dX * dX + dY * dY
        return (err2 < maxerr).astype(np.uint8)


def _pose32(R, t):
    p = np.zeros((), POSE_DTYPE)
    with np.errstate(all="ignore"):
        p["R"] = np.array([R[i][j] for i in range(3) for j in range(3)], np.float64).astype(F)
        p["t"] = np.array(t, np.float64).astype(F)
    return p


class Solver:
    """PnPsolver: the constructor's staging, SetRansacParameters, iterate, Refine, find.  trace: one tuple per iteration
    (iteration, draw, count, new best?, Refine's count or None)."""

    def __init__(self, rows, cam, seed, prob=0.99, min_inliers=8, max_its=300, min_set=4, epsilon=0.4, th2=5.991):
        assert min_set == 4
        self.rows = np.ascontiguousarray(rows, ROW_DTYPE)
        self.N = len(self.rows)
        self.cam = tuple(float(F(cam[k])) for k in ("fx", "fy", "cx", "cy"))
        self.maxerr = self.rows["sigma2"] * F(th2)            # float x float
        self.max_its, self.min_inliers = ransac_parameters(self.N, prob, min_inliers, max_its, min_set, epsilon)
        self.G = GlibcRand(seed)
        self.iterations = self.best = 0
        self.best_T = np.zeros((), POSE_DTYPE)
        self.best_flags = np.zeros(self.N, np.uint8)
        self.trace = []

    def _corr(self, idx):
        r = self.rows
        return ([[float(r["X"][i]), float(r["Y"][i]), float(r["Z"][i])] for i in idx], [[float(r["u"][i]), float(r["v"][i])] for i in idx])

    def _result(self, status, inliers, T):
        res = np.zeros((), RESULT_DTYPE)
        res["status"], res["iterations"], res["inliers"], res["best_inliers"] = status, self.iterations, inliers, self.best
        res["min_inliers"] = self.min_inliers
        if T is not None:
            res["Tcw"] = T
        res["best_Tcw"] = self.best_T
        return res

    def iterate(self, n_iterations):
        """-> (RESULT_DTYPE record, flags by row u8 [N])"""
        zeros = np.zeros(self.N, np.uint8)
        if self.N < self.min_inliers:
            return self._result(2, 0, None), zeros
        cur = 0
        while self.iterations < self.max_its or cur < n_iterations:
            cur += 1
            self.iterations += 1
            idx = draw(self.G, self.N, 4)
            R, t = compute_pose(*self._corr(idx), self.cam)
            flags = check_inliers(self.rows, self.maxerr, R, t, self.cam)
            cnt = int(flags.sum())
            ev = [self.iterations, tuple(idx), cnt, False, None]
            self.trace.append(ev)
            if cnt >= self.min_inliers:
                if cnt > self.best:
                    self.best_flags, self.best, self.best_T = flags.copy(), cnt, _pose32(R, t)
                    ev[3] = True
                R, t = compute_pose(*self._corr(np.flatnonzero(self.best_flags)), self.cam)
                rflags = check_inliers(self.rows, self.maxerr, R, t, self.cam)
                rc = int(rflags.sum())
                ev[4] = rc
                if rc > self.min_inliers:
                    return self._result(1, rc, _pose32(R, t)), rflags
        if self.iterations >= self.max_its:
            if self.best >= self.min_inliers:
                return self._result(3, self.best, self.best_T), self.best_flags.copy()
            return self._result(2, 0, None), zeros
        return self._result(0, 0, None), zeros

    def find(self):
        return self.iterate(self.max_its)


def play(rows, cam, seed, params, n_iterations, reject=0):
    """A candidate as tools/dropin/pnp_main.cpp plays it: calls of iterate(n_iterations) on one solver; a pose that came without bNoMore
    is refused `reject` times.  -> ([(result, flags)], best_flags, trace)"""
    S = Solver(rows, cam, seed, **params)
    calls, rejected = [], 0
    while True:
        res, flags = S.iterate(n_iterations)
        calls.append((res, flags))
        st = int(res["status"])
        if st & 2 or (n_iterations <= 0 and not st & 1):
            break
        if st & 1:
            if rejected >= reject:
                break
            rejected += 1
    return calls, S.best_flags.copy(), S.trace


def same_result(a, b):
    """bit for bit (a NaN equals any NaN)"""
    for k in ("status", "iterations", "inliers", "best_inliers", "min_inliers"):
        if int(a[k]) != int(b[k]):
            return False
    return all(same_floats(a[p][k], b[p][k]) for p in ("Tcw", "best_Tcw") for k in ("R", "t"))


# ---- scenes ------------------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def ground_truth(data_seed):
    rng = np.random.RandomState(1000 + data_seed)
    return _rot(*rng.uniform(-0.4, 0.4, 3)), rng.uniform(-0.5, 0.5, 3) + np.array([0.0, 0.0, 0.3])


def make_rows(data_seed, n, ngood, kind="box", noise_px=0.0):
    """n rows of which the first-shuffled ngood are projections of their points under ground_truth(data_seed); the others carry a random
    pixel.  kind: box (points in a box 2..6 m in front of the camera), planar (all on one plane), identical (every row the same), behind
    (box, and the last outlier's point lies behind the camera)."""
    rng = np.random.RandomState(data_seed)
    R, t = ground_truth(data_seed)
    Pc = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)], 1)
    if kind == "planar":
        Pc[:, 2] = 4.0 + 0.3 * Pc[:, 0] - 0.2 * Pc[:, 1]
    if kind == "identical":
        Pc[:] = Pc[0]
    Pw = (Pc - t) @ R                      # R^T (Pc - t)
    rows = np.zeros(n, ROW_DTYPE)
    rows["X"], rows["Y"], rows["Z"] = Pw[:, 0], Pw[:, 1], Pw[:, 2]
    Pw32 = np.stack([rows["X"], rows["Y"], rows["Z"]], 1).astype(np.float64)
    Pc2 = Pw32 @ R.T + t
    u = CAM["cx"] + CAM["fx"] * Pc2[:, 0] / Pc2[:, 2] + noise_px * rng.standard_normal(n)
    v = CAM["cy"] + CAM["fy"] * Pc2[:, 1] / Pc2[:, 2] + noise_px * rng.standard_normal(n)
    good = np.zeros(n, bool)
    good[rng.permutation(n)[:ngood]] = True
    if kind == "identical":
        good[:] = True
    u = np.where(good, u, rng.uniform(0, 640, n))
    v = np.where(good, v, rng.uniform(0, 480, n))
    rows["u"], rows["v"] = u, v
    rows["sigma2"] = (F(1.2) ** rng.randint(0, 8, n).astype(F)) ** 2
    if kind == "behind":
        i = int(np.flatnonzero(~good)[-1]) if (~good).any() else n - 1
        pb = (np.array([0.3, -0.2, -3.0]) - t) @ R
        rows["X"][i], rows["Y"][i], rows["Z"][i] = pb
    return rows, good


# name -> (data_seed, n, ngood, kind, noise_px, parameter overrides, n_iterations of the rounds test, reject)
_R = dict(RELOC, max_its=24)
CASE_SPECS = {
    "n3": (1, 3, 3, "box", 0.0, _R, 5, 0),                                           # below min_set: bNoMore, nothing solved
    "n4_min4": (2, 4, 4, "box", 0.0, dict(_R, min_inliers=4), 5, 0),                # N == minInliers: budget 1, all four drawn
    "n5": (3, 5, 5, "box", 0.0, _R, 5, 0),                                           # below the clamp of 10
    "n9": (4, 9, 9, "box", 0.0, _R, 5, 0),
    "n15": (5, 15, 15, "box", 0.0, _R, 5, 1),                                        # Relocalization's floor
    "n63": (6, 63, 63, "box", 0.0, _R, 5, 1),
    "n64_half": (7, 64, 32, "box", 0.0, _R, 5, 0),
    "n65_half": (8, 65, 33, "box", 0.3, _R, 5, 2),
    "n384_half": (9, 384, 192, "box", 0.0, _R, 5, 0),                                # the last row count that lies in LDS in full
    "n385_half": (10, 385, 193, "box", 0.0, _R, 5, 0),                               # one row read from HBM
    "n400_half": (11, 400, 200, "box", 0.3, _R, 5, 1),                               # rstride itself in the batch
    "n60_fifth": (12, 60, 12, "box", 0.0, dict(_R, min_inliers=12, epsilon=0.2), 5, 0),  # the budget runs out with a best pose (Refine == min)
    "n60_fifth_none": (13, 60, 12, "box", 0.0, _R, 5, 0),                             # 12 consistent rows below the 30 wanted: never qualifies
    "planar30": (14, 30, 30, "planar", 0.0, _R, 5, 0),                                # the pseudo-inverse path of cvInvert
    "identical20": (15, 20, 20, "identical", 0.0, _R, 5, 0),                          # singular everywhere
    "behind30": (16, 30, 24, "behind", 0.0, _R, 5, 0),                                # a point behind the camera
    "eq_min20": (17, 20, 10, "box", 0.0, _R, 5, 0),                                   # 10 consistent == minInliers: every Refine fails at ==
    "noisy40_eq": (19, 40, 24, "box", 2.0, _R, 5, 3),      # seed searched: a Refine fails at == min (it 16), a later one succeeds (it 18)
    "noisy40_notbest": (19, 40, 24, "box", 2.0, _R, 5, 3),  # seed searched: it 9 qualifies without being a new best and Refine still runs
    "its15": (20, 20, 10, "box", 0.0, dict(_R, max_its=15), 5, 0),                    # the budget ends inside a block, on its last
    "its16": (20, 20, 10, "box", 0.0, dict(_R, max_its=16), 5, 0),                    # hypothesis, and one past it
    "its17": (20, 20, 10, "box", 0.0, dict(_R, max_its=17), 7, 0),
}
CASE_NAMES = list(CASE_SPECS)
# seeds found by a search over the draws (the first draw of four consistent rows falls at the wanted iteration) or over the trace
SEEDS = {"n4_min4": 2, "n64_half": 151, "n384_half": 3, "n385_half": 1, "n400_half": 10, "n60_fifth": 11, "eq_min20": 1, "its15": 253, "its16": 86, "its17": 17,
         "noisy40_eq": 194, "noisy40_notbest": 239}

_cache = {}


def case(name):
    """-> dict(rows, good, cam, seed, params, n_iterations, reject, find = play(.., max_its, 0), rounds = play(.., n_iterations, reject))"""
    if name not in _cache:
        ds, n, ngood, kind, noise, params, nit, reject = CASE_SPECS[name]
        rows, good = make_rows(ds, n, ngood, kind, noise)
        seed = SEEDS.get(name, 100 + ds)
        c = dict(rows=rows, good=good, cam=CAM, seed=seed, params=params, n_iterations=nit, reject=reject)
        c["find_its"] = ransac_parameters(n, *(params[k] for k in ("prob", "min_inliers", "max_its", "min_set", "epsilon")))[0]
        c["find"] = play(rows, CAM, seed, params, c["find_its"], 0)
        c["rounds"] = play(rows, CAM, seed, params, nit, reject)
        _cache[name] = c
    return _cache[name]


# ---- the files of tools/dropin/pnp_main.cpp ---------------------------------------------------------------------------------------------------
def write_cases(path, cases, mode, camera_dtype):
    """cases.bin; mode "find": every case as one find(); "rounds": its n_iterations and rejections.  Every case of a file shares prob
    and th2."""
    rstride = max(max(len(c["rows"]) for c in cases), 1)
    cam = np.zeros((), camera_dtype)
    for k, v in cases[0]["cam"].items():
        cam[k] = v
    p0 = cases[0]["params"]
    assert all(c["params"]["prob"] == p0["prob"] and c["params"]["th2"] == p0["th2"] for c in cases)
    with open(path, "wb") as f:
        np.array([len(cases), rstride, 4], np.int32).tofile(f)
        np.array([p0["prob"]], np.float64).tofile(f)
        np.array([p0["th2"]], np.float32).tofile(f)
        cam.tofile(f)
        for c in cases:
            P = c["params"]
            nit, rej = (c["find_its"], 0) if mode == "find" else (c["n_iterations"], c["reject"])
            np.array([c["seed"]], np.uint32).tofile(f)
            np.array([len(c["rows"]), P["min_inliers"], P["max_its"], nit, rej], np.int32).tofile(f)
            np.array([P["epsilon"]], np.float32).tofile(f)
            c["rows"].tofile(f)
    return rstride


def read_section(f, cases):
    """one section of out.bin -> [([(result, flags)], best_flags)]"""
    out = []
    for c in cases:
        n = len(c["rows"])
        calls = []
        for _ in range(int(np.fromfile(f, np.int32, 1)[0])):
            res = np.fromfile(f, RESULT_DTYPE, 1)[0]
            calls.append((res, np.fromfile(f, np.uint8, n)))
        out.append((calls, np.fromfile(f, np.uint8, n)))
    return out


def assert_play_equal(got, ref, what, best_flags=True):
    """every call bit for bit: status, iterations, the counts, min_inliers, both poses, every flag; then mvbBestInliers"""
    calls, bf = got
    rcalls, rbf = ref[0], ref[1]
    assert len(calls) == len(rcalls), (what, len(calls), len(rcalls))
    for k, ((res, flags), (rres, rflags)) in enumerate(zip(calls, rcalls)):
        assert same_result(res, rres), (what, k, res, rres)
        assert (np.asarray(flags) == rflags).all(), (what, k, np.flatnonzero(np.asarray(flags) != rflags)[:8])
    if best_flags and len(rcalls) and int(rcalls[-1][0]["best_inliers"]) > 0:
        assert (np.asarray(bf) == rbf).all(), (what, "best flags")
