"""Sim3Solver (src/Sim3Solver.cc) restated in numpy, rounding by rounding, and the cases of tests/test_sim3_solver_{cpu,gpu}.py.

The text follows psl-slam_amd/csrc/sim3_solver_kernels.h function by function (DESIGN.md §3 lists the conventions): np.float32 scalars
for every float operation, Python floats for every double one, math.sin / math.cos / math.sqrt for glibc's (the library's restated
sin / cos are bit-identical to them by contract), fdlibm's atan2 as psl_atan2, glibc's rand() and OpenCV 3.2's Jacobi written out.
`horn_f64` is the same closed form in plain float64 with numpy.linalg.eigh and nothing rounded to float: what the restatement is
checked against."""
import functools
import math
import struct
from fractions import Fraction

import numpy as np

from sim3_opt_cases import PAIR_DTYPE, SIM3_DTYPE, cameras, sim3_rec
from pose_opt_cases import _rodrigues

F = np.float32
RESULT_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("ninliers", "<i4"), ("best_inliers", "<i4"), ("S12", SIM3_DTYPE)])
HYP_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("s", "<f4"), ("T12", "<f4", (12,)), ("T21", "<f4", (12,))])
TRACE_DTYPE = np.dtype([("idx", "<i4", (3,)), ("cnt", "<i4"), ("h", HYP_DTYPE)])
assert RESULT_DTYPE.itemsize == 68 and HYP_DTYPE.itemsize == 148 and TRACE_DTYPE.itemsize == 164
PROB, MIN_INLIERS, MAX_ITS = 0.99, 20, 300          # src/LoopClosing.cc:281
LEVEL_SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
SINCOS_RANGE = 105414350.0


# ---- fdlibm atan / atan2 (psl_f64math.h) -------------------------------------------------------------------------------------------
def _hi_lo(x):
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    hx = u >> 32
    return (hx - (1 << 32) if hx & 0x80000000 else hx), u & 0xffffffff


_ATANHI = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
_ATANLO = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
_AT = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
       9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
       4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)


def _fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the correctly rounded conversion)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def fdlibm_atan(x, dx=0.0):
    """psl_atan_lo: fdlibm's atan with the low part dx of the argument carried into the low-order sum"""
    hx, lx = _hi_lo(x)
    ix = hx & 0x7fffffff
    corr = 0.0 if dx == 0.0 else dx / (1.0 + x * x)
    if ix >= 0x44100000:
        if ix > 0x7ff00000 or (ix == 0x7ff00000 and lx != 0):
            return x + x
        return _ATANHI[3] + _ATANLO[3] if hx > 0 else -_ATANHI[3] - _ATANLO[3]
    if ix < 0x3fdc0000:
        if ix < 0x3e200000:
            return x
        idn = -1
    else:
        x = abs(x)
        if ix < 0x3ff30000:
            if ix < 0x3fe60000:
                idn, x = 0, (2.0 * x - 1.0) / (2.0 + x)
            else:
                idn, x = 1, (x - 1.0) / (x + 1.0)
        elif ix < 0x40038000:
            idn, x = 2, (x - 1.5) / (1.0 + 1.5 * x)
        else:
            idn, x = 3, -1.0 / x
    z = x * x
    w = z * z
    a = _AT
    s1 = z * (a[0] + w * (a[2] + w * (a[4] + w * (a[6] + w * (a[8] + w * a[10])))))
    s2 = w * (a[1] + w * (a[3] + w * (a[5] + w * (a[7] + w * a[9]))))
    if idn < 0:
        return x - (x * (s1 + s2) - corr)
    r = _ATANHI[idn] - (((x * (s1 + s2) - _ATANLO[idn]) - (-corr if hx < 0 else corr)) - x)
    return -r if hx < 0 else r


def fdlibm_atan2(y, x):
    tiny, pi_o_2, pi, pi_lo = 1.0e-300, 1.5707963267948965580E+00, 3.1415926535897931160E+00, 1.2246467991473531772E-16
    if x != x or y != y:
        return x + y
    hx, lx = _hi_lo(x)
    hy, ly = _hi_lo(y)
    ix, iy = hx & 0x7fffffff, hy & 0x7fffffff
    if hx == 0x3ff00000 and lx == 0:
        return fdlibm_atan(y)
    m = (1 if hy < 0 else 0) | (2 if hx < 0 else 0)
    if (iy | ly) == 0:
        return y if m < 2 else (pi + tiny if m == 2 else -pi - tiny)
    if (ix | lx) == 0:
        return -pi_o_2 - tiny if hy < 0 else pi_o_2 + tiny
    k = (iy - ix) >> 20
    if k > 60:
        z = pi_o_2 + 0.5 * pi_lo
    elif hx < 0 and k < -60:
        z = 0.0
    else:
        q = y / x
        dq = _fma(-q, x, y) / x
        z = fdlibm_atan(-q, -dq) if q < 0 else fdlibm_atan(q, dq)
    if m == 0:
        return z
    if m == 1:
        return -z
    if m == 2:
        return pi - (z - pi_lo)
    return (z - pi_lo) - pi


# ---- glibc rand(), the draw -----------------------------------------------------------------------------------------------------------
class GlibcRand:
    """srand(seed); rand(): the TYPE_3 additive feedback generator"""

    def __init__(self, seed):
        seed &= 0xffffffff
        prev = 1 if seed == 0 else (seed - (1 << 32) if seed & 0x80000000 else seed)
        r = [prev & 0xffffffff]
        for _ in range(1, 31):
            hi, lo = (prev // 127773, prev % 127773) if prev >= 0 else (-(-prev // 127773), -(-prev % 127773))   # C truncates
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            prev = word
            r.append(prev & 0xffffffff)
        r += r[0:3]
        for k in range(34, 344):
            r[k % 34] = (r[(k - 31) % 34] + r[(k - 3) % 34]) & 0xffffffff
        self.r, self.k = r, 344

    def rand(self):
        k = self.k
        v = (self.r[(k - 31) % 34] + self.r[(k - 3) % 34]) & 0xffffffff
        self.r[k % 34] = v
        self.k = k + 1
        return v >> 1


def random_int(r, d):
    """DUtils::Random::RandomInt(0, d - 1), the double expression as it is written (Random.cpp:47-50)"""
    return int((float(r) / (2147483647.0 + 1.0)) * d)


def draw(G, N, k=3):
    """the k draws of one iteration with the vector of available indices written out (Sim3Solver.cc:163-177 with k = 3,
    PnPsolver.cc:188-201 with 4, Initializer.cc:82-97 with 8)"""
    avail = list(range(N))
    out = []
    for _ in range(k):
        randi = random_int(G.rand(), len(avail))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


# ---- SetRansacParameters -------------------------------------------------------------------------------------------------------------
def max_iterations(N, prob=PROB, min_inliers=MIN_INLIERS, max_its=MAX_ITS):
    if N == min_inliers:
        n = 1
    else:
        eps = F(min_inliers) / F(N)
        d = math.log(1 - math.pow(float(eps), 3))
        v = math.inf if d == 0.0 else math.ceil(math.log(1 - prob) / d)
        n = int(v) if v < max_its else max_its
    return max(1, min(n, max_its))


# ---- staging --------------------------------------------------------------------------------------------------------------------------
def max_error(sigma2):
    """(float)(size_t)(9.210 * sigma2) per element"""
    v = 9.210 * np.asarray(sigma2, np.float32).astype(np.float64)
    return np.floor(v).astype(np.uint64).astype(np.float32)


def to_image(X, cam):
    """FromCameraToImage on rows of X (float32 [n][3])"""
    with np.errstate(all="ignore"):
        invz = F(1.0) / X[:, 2]
        x, y = X[:, 0] * invz, X[:, 1] * invz
        return np.stack([cam["fx"] * x + cam["cx"], cam["fy"] * y + cam["cy"]], 1).astype(np.float32)


def stage(pairs, sigma2, cam1, cam2):
    X1, X2 = np.ascontiguousarray(pairs["P1c"], np.float32), np.ascontiguousarray(pairs["P2c"], np.float32)
    sigma2 = np.asarray(sigma2, np.float32).reshape(-1, 2)
    return {"X1": X1, "X2": X2, "p1": to_image(X1, cam1), "p2": to_image(X2, cam2), "th1": max_error(sigma2[:, 0]), "th2": max_error(sigma2[:, 1])}


# ---- ComputeSim3 ------------------------------------------------------------------------------------------------------------------------
def centroid(P):
    """P float32 [3][3], column i = point i -> (Pr, C)"""
    third = F(1.0 / 3.0)
    C = np.zeros(3, np.float32)
    Pr = np.zeros((3, 3), np.float32)
    for r in range(3):
        C[r] = ((P[r, 0] + P[r, 2]) + P[r, 1]) * third
        for i in range(3):
            Pr[r, i] = P[r, i] - C[r]
    return Pr, C


def _hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * math.sqrt(1.0 + b * b)
    if b > 0:
        a = a / b
        return b * math.sqrt(1.0 + a * a)
    return 0.0


def _ind_r(A, k):
    m, mv = k + 1, abs(A[k, k + 1])
    for i in range(k + 2, 4):
        if mv < abs(A[k, i]):
            mv, m = abs(A[k, i]), i
    return m


def _ind_c(A, k):
    m, mv = 0, abs(A[0, k])
    for i in range(1, k):
        if mv < abs(A[i, k]):
            mv, m = abs(A[i, k]), i
    return m


def jacobi4(A_in):
    """cv::eigen on a symmetric 4x4 CV_32F (OpenCV 3.2 JacobiImpl_<float>) -> (W decreasing, V rows, rotations)"""
    n = 4
    A = np.array(A_in, np.float32).reshape(4, 4).copy()
    V = np.eye(4, dtype=np.float32)
    W = np.array([A[k, k] for k in range(4)], np.float32)
    indR, indC = [0] * 4, [0] * 4
    for k in range(n):
        if k < n - 1:
            indR[k] = _ind_r(A, k)
        if k > 0:
            indC[k] = _ind_c(A, k)
    eps = F(1.1920928955078125e-07)
    iters = 0
    with np.errstate(all="ignore"):
        while iters < n * n * 30:
            k, mv = 0, abs(A[0, indR[0]])
            for i in range(1, n - 1):
                v = abs(A[i, indR[i]])
                if mv < v:
                    mv, k = v, i
            l = indR[k]
            for i in range(1, n):
                v = abs(A[indC[i], i])
                if mv < v:
                    mv, k, l = v, indC[i], i
            p = A[k, l]
            if not abs(p) > eps:
                break
            pd, y = float(p), float(W[l] - W[k]) * 0.5
            td = abs(y) + _hypot(pd, y)
            sd = _hypot(pd, td)
            cd = td / sd
            sd = pd / sd
            td = (pd / td) * pd
            if y < 0:
                sd, td = -sd, -td
            c, s, t = F(cd), F(sd), F(td)
            A[k, l] = F(0)
            W[k] = W[k] - t
            W[l] = W[l] + t

            def rot(M, i0, j0, i1, j1):
                a0, b0 = M[i0, j0], M[i1, j1]
                M[i0, j0] = a0 * c - b0 * s
                M[i1, j1] = a0 * s + b0 * c
            for i in range(0, k):
                rot(A, i, k, i, l)
            for i in range(k + 1, l):
                rot(A, k, i, i, l)
            for i in range(l + 1, n):
                rot(A, k, i, l, i)
            for i in range(n):
                rot(V, k, i, l, i)
            for idx in (k, l):
                if idx < n - 1:
                    indR[idx] = _ind_r(A, idx)
                if idx > 0:
                    indC[idx] = _ind_c(A, idx)
            iters += 1
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[[m, k]] = W[[k, m]]
            V[[m, k]] = V[[k, m]]
    return W, V, iters


def rodrigues_f32(v):
    r = [float(v[0]), float(v[1]), float(v[2])]
    theta = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if theta < 2.220446049250313e-16:
        return np.eye(3, dtype=np.float32)
    if not theta < SINCOS_RANGE:
        return np.full((3, 3), np.nan, np.float32)
    c, s = math.cos(theta), math.sin(theta)
    c1 = 1.0 - c
    it = 1.0 / theta
    r = [r[0] * it, r[1] * it, r[2] * it]
    rx = [[0.0, -r[2], r[1]], [r[2], 0.0, -r[0]], [-r[1], r[0], 0.0]]
    R = np.zeros((3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            R[i, j] = F((c * (1.0 if i == j else 0.0) + c1 * (r[i] * r[j])) + s * rx[i][j])
    return R


def _row3(M, X):
    return (float(M[0]) * float(X[0]) + float(M[1]) * float(X[1])) + float(M[2]) * float(X[2])


def hypothesis(P1, P2, fix_scale):
    """ComputeSim3(P1, P2) -> a HYP_DTYPE record"""
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(np.asarray(P1, np.float32))
        Pr2, O2 = centroid(np.asarray(P2, np.float32))
        M = np.zeros((3, 3), np.float32)
        for i in range(3):
            for j in range(3):
                M[i, j] = F(_row3(Pr2[i], Pr1[j]))
        N11, N12, N13, N14 = (M[0, 0] + M[1, 1]) + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
        N22, N23, N24 = (M[0, 0] - M[1, 1]) - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
        N33, N34, N44 = (-M[0, 0] + M[1, 1]) - M[2, 2], M[1, 2] + M[2, 1], (-M[0, 0] - M[1, 1]) + M[2, 2]
        A = np.array([N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44], np.float32)
        W, V, _ = jacobi4(A)
        q = V[0]
        nrm = math.sqrt((float(q[1]) * float(q[1]) + float(q[2]) * float(q[2])) + float(q[3]) * float(q[3]))
        ang = fdlibm_atan2(nrm, float(q[0]))
        alpha = F(np.float64(2.0 * ang) / np.float64(nrm))
        vec = np.array([q[1] * alpha, q[2] * alpha, q[3] * alpha], np.float32)
        R = rodrigues_f32(vec)
        if not fix_scale:
            P3 = np.zeros((3, 3), np.float32)
            for i in range(3):
                for j in range(3):
                    P3[i, j] = F(_row3(R[i], Pr2[:, j]))
            nom = den = 0.0
            for a, b in zip(Pr1.reshape(9), P3.reshape(9)):
                nom = nom + float(a) * float(b)
            for b in P3.reshape(9):
                den = den + float(b * b)
            s = F(np.float64(nom) / np.float64(den))
        else:
            s = F(1.0)
        h = np.zeros((), HYP_DTYPE)
        t = np.zeros(3, np.float32)
        for r in range(3):
            t[r] = F(_row3(R[r], O2) * float(-s) + float(O1[r]))
        inv = F(np.float64(1.0) / np.float64(s))
        T12, T21 = np.zeros((3, 4), np.float32), np.zeros((3, 4), np.float32)
        for i in range(3):
            for j in range(3):
                T12[i, j] = s * R[i, j]
                T21[i, j] = inv * R[j, i]
        for r in range(3):
            T12[r, 3] = t[r]
            T21[r, 3] = F(-_row3(T21[r, :3], t))
        h["R"], h["t"], h["s"], h["T12"], h["T21"] = R.reshape(9), t, s, T12.reshape(12), T21.reshape(12)
        return h


# ---- Project, CheckInliers on all pairs ---------------------------------------------------------------------------------------------------
def project(T, X, cam):
    T = np.asarray(T, np.float32).reshape(3, 4).astype(np.float64)
    Xd = X.astype(np.float64)
    with np.errstate(all="ignore"):
        Pc = np.stack([(((T[r, 0] * Xd[:, 0] + T[r, 1] * Xd[:, 1]) + T[r, 2] * Xd[:, 2]) + T[r, 3]).astype(np.float32) for r in range(3)], 1)
    return to_image(Pc, cam)


def _err(a, b):
    with np.errstate(all="ignore"):
        d = (a - b).astype(np.float32).astype(np.float64)
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float32)


def errors(S, h, cam1, cam2):
    return _err(S["p1"], project(h["T12"], S["X2"], cam1)), _err(project(h["T21"], S["X1"], cam2), S["p2"])


def inliers(S, h, cam1, cam2):
    e1, e2 = errors(S, h, cam1, cam2)
    with np.errstate(all="ignore"):
        return ((e1 < S["th1"]) & (e2 < S["th2"])).astype(np.uint8)


# ---- iterate -------------------------------------------------------------------------------------------------------------------------------
def iterate(pairs, sigma2, cam1, cam2, fix_scale, seed, n_iterations, start_it=0, best_in=0, prob=PROB, min_inliers=MIN_INLIERS, max_its=MAX_ITS):
    """Sim3Solver::iterate(n_iterations) of the candidate seeded with `seed`, resumed at (start_it, best_in)
    -> (RESULT_DTYPE record, flags u8 [n] by pair row, trace TRACE_DTYPE [iterations run])"""
    N = len(pairs)
    res = np.zeros((), RESULT_DTYPE)
    res["iterations"], res["best_inliers"] = start_it, best_in
    flags = np.zeros(N, np.uint8)
    trace = []
    if N < min_inliers:
        res["status"] = 2
        return res, flags, np.zeros(0, TRACE_DTYPE)
    S = stage(pairs, sigma2, cam1, cam2)
    mx = max_iterations(N, prob, min_inliers, max_its)
    G = GlibcRand(seed)
    for _ in range(3 * start_it):
        G.rand()
    it, best, cur = start_it, best_in, 0
    while it < mx and cur < n_iterations:
        cur += 1
        it += 1
        idx = draw(G, N)
        h = hypothesis(S["X1"][idx].T, S["X2"][idx].T, fix_scale)
        fl = inliers(S, h, cam1, cam2)
        cnt = int(fl.sum())
        tr = np.zeros((), TRACE_DTYPE)
        tr["idx"], tr["cnt"], tr["h"] = idx, cnt, h
        trace.append(tr)
        if cnt >= best:
            best = cnt
            if cnt > min_inliers:
                res["status"], res["iterations"], res["ninliers"], res["best_inliers"] = 1, it, cnt, best
                res["S12"]["R"], res["S12"]["t"], res["S12"]["s"] = h["R"], h["t"], h["s"]
                return res, fl, _stack(trace)
    res["status"] = 2 if it >= mx else 0
    res["iterations"], res["best_inliers"] = it, best
    return res, flags, _stack(trace)


def _stack(trace):
    out = np.zeros(len(trace), TRACE_DTYPE)
    for k, t in enumerate(trace):
        out[k] = t
    return out


def find(pairs, sigma2, cam1, cam2, fix_scale, seed, **kw):
    return iterate(pairs, sigma2, cam1, cam2, fix_scale, seed, kw.get("max_its", MAX_ITS), **kw)


def same_floats(a, b):
    """bit for bit, a NaN equal to any NaN (the payload of a NaN is not part of the contract)"""
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def hyp_floats(h):
    return np.concatenate([np.asarray(h[k], np.float32).reshape(-1) for k in ("R", "t", "s", "T12", "T21")])


# ---- the float64 Horn solution ---------------------------------------------------------------------------------------------------------
def horn_f64(P1, P2, fix_scale):
    """Horn 1987 in float64: (R, t, s) with P1 ~ s R P2 + t for the columns of the two 3x3 matrices"""
    P1, P2 = np.asarray(P1, np.float64), np.asarray(P2, np.float64)
    O1, O2 = P1.mean(1), P2.mean(1)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, v = np.linalg.eigh(N)
    q = v[:, -1]
    nv = np.linalg.norm(q[1:])
    ang = math.atan2(nv, q[0])
    R = _rodrigues(2 * ang * q[1:] / nv) if nv > 0 else np.eye(3)
    P3 = R @ Pr2
    s = 1.0 if fix_scale else float((Pr1 * P3).sum() / (P3 * P3).sum())
    return R, O1 - s * R @ O2, s


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def make_pairs(data_seed, n, ngood, fix_scale, collinear=False, noise_px=0.0):
    """n pairs of which the first-listed `good` (a random subset of ngood rows) agree with one true Sim3 to float precision; the others
    pair camera-2 points with unrelated camera-1 points.  -> (pairs, sigma2 [n][2], good u8 [n], true Sim3 record)"""
    rng = np.random.default_rng(data_seed)
    cam1, cam2 = cameras()
    Rt = _rodrigues(rng.normal(size=3) * 0.2)
    Strue = sim3_rec(Rt, rng.normal(size=3) * 0.3, 1.0 if fix_scale else 1.15)
    Rt, tt, st = Strue["R"].astype(np.float64).reshape(3, 3), Strue["t"].astype(np.float64), float(Strue["s"])
    fx2, fy2, cx2, cy2 = (float(cam2[k]) for k in ("fx", "fy", "cx", "cy"))
    z, u, v = rng.uniform(2.0, 8.0, n), rng.uniform(120.0, 520.0, n), rng.uniform(100.0, 380.0, n)
    P2 = np.stack([(u - cx2) / fx2 * z, (v - cy2) / fy2 * z, z], 1)
    if collinear:   # every point within 1e-4 of one line: every triple is near-collinear
        a, d = np.array([0.2, -0.1, 4.0]), np.array([0.5, 0.3, 0.4])
        P2 = a + np.outer(rng.uniform(-2.0, 2.0, n), d) + rng.normal(size=(n, 3)) * 1e-4
    P2 = P2.astype(np.float32)
    P1 = st * (P2.astype(np.float64) @ Rt.T) + tt
    if noise_px:    # the camera-1 points move sideways by about noise_px pixels: the counts of the all-good triples then differ
        P1[:, :2] += rng.normal(size=(n, 2)) * (noise_px * P1[:, 2:3] / 500.0)
    P1 = P1.astype(np.float32)
    good = np.zeros(n, np.uint8)
    good[rng.choice(n, ngood, replace=False)] = 1
    z1, u1, v1 = rng.uniform(2.0, 8.0, n), rng.uniform(120.0, 520.0, n), rng.uniform(100.0, 380.0, n)
    other = np.stack([(u1 - 320.0) / 500.0 * z1, (v1 - 240.0) / 500.0 * z1, z1], 1).astype(np.float32)
    P1[good == 0] = other[good == 0]
    p = np.zeros(n, PAIR_DTYPE)
    p["P1c"], p["P2c"] = P1, P2
    S = stage(p, np.ones((n, 2), np.float32), cam1, cam2)
    p["u1"], p["v1"], p["u2"], p["v2"] = S["p1"][:, 0], S["p1"][:, 1], S["p2"][:, 0], S["p2"][:, 1]
    o1, o2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    sigma2 = np.stack([LEVEL_SIGMA2[o1], LEVEL_SIGMA2[o2]], 1).astype(np.float32)
    p["inv_sigma2_1"], p["inv_sigma2_2"] = F(1.0) / sigma2[:, 0], F(1.0) / sigma2[:, 1]
    return p, sigma2, good, Strue


def first_all_good(seed, good, mx):
    """the first iteration (1-based) whose three draws are all good rows, or 0: integer work only (the seed searches)"""
    G = GlibcRand(seed)
    N = len(good)
    for it in range(1, mx + 1):
        if all(good[i] for i in draw(G, N)):
            return it
    return 0


# name -> (data seed, n, ngood, fix_scale, rand seed, the iteration that succeeds or 0, extra)
# The rand seeds of the rows with a fixed success iteration are the smallest seeds >= 1 whose first all-good triple falls on that
# iteration (first_all_good); case() asserts that the solver then succeeds exactly there.
CASE_SPECS = {
    "n19": (1, 19, 19, False, 5, 0, None),                  # N < minInliers: bNoMore at once
    "n20": (2, 20, 20, False, 5, 0, None),                  # N == minInliers: one iteration; 20 inliers are not > 20
    "n21": (3, 21, 21, False, 5, 1, None),
    "n63": (4, 63, 40, False, None, 1, None),
    "n64": (5, 64, 40, True, None, 5, None),
    "n65": (6, 65, 40, False, None, 6, None),               # the first qualifying iteration is the 6th: the second iterate(5)
    "n127": (7, 127, 50, False, None, 5, None),
    "n129": (8, 129, 50, True, None, 6, None),
    "n200_it64": (9, 200, 60, False, None, 64, None),       # the last hypothesis of the kernel's first block
    "n200_it65": (10, 200, 60, False, None, 65, None),      # the first of its second block
    "n200_it300": (11, 200, 30, False, None, 300, None),    # the last iteration of the budget
    "n200_never": (12, 200, 0, False, 7, 0, None),          # no consistent set: 300 iterations, bNoMore
    "n300_fixed": (13, 300, 150, True, None, 1, None),
    "n1024": (14, 1024, 400, False, None, 5, None),         # the LDS capacity of the kernel
    "n1025": (15, 1025, 400, False, None, 6, None),         # one pair staged from its HBM row
    "n65_truncation": (16, 65, 40, False, None, 1, "truncation"),
    "n65_behind_nan": (17, 65, 40, False, None, 6, "behind_nan"),
    "n40_collinear": (18, 40, 40, False, 3, -1, "collinear"),   # near-collinear triples: compared bit for bit only
    "n150_noisy": (19, 150, 60, False, 9, 210, "noisy6"),       # 6 px of noise: the best rises 11, 16, 20 (not > 20), then 21 at iteration 210
    "n150_noisy_never": (19, 150, 45, False, 10, 0, "noisy4"),  # 4 px: the best reaches 17 and stays there
}
CASE_NAMES = list(CASE_SPECS)


@functools.lru_cache(maxsize=None)
def _seed_for(data_seed, n, ngood, fix_scale, target):
    p, sigma2, good, _ = make_pairs(data_seed, n, ngood, fix_scale)
    mx = max_iterations(n)
    for seed in range(1, 200000):
        if first_all_good(seed, good, mx) == target:
            return seed
    raise AssertionError("no seed")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(pairs, sigma2, good, Strue, fix_scale, cam1, cam2, seed, ref = find(): (result, flags, trace))"""
    data_seed, n, ngood, fix, seed, target, extra = CASE_SPECS[name]
    p, sigma2, good, Strue = make_pairs(data_seed, n, ngood, fix, collinear=extra == "collinear", noise_px={"noisy6": 6.0, "noisy4": 4.0}.get(extra, 0.0))
    cam1, cam2 = cameras()
    if seed is None:
        seed = SEEDS[name]
    if extra == "truncation":
        # good row g moves sideways in camera 1 by 3.02 px at sigma2 = 1: err1 ~ 9.12 lies between floor(9.21) = 9 and 9.21; its
        # second threshold is that of the coarsest level, so that the first test alone decides
        g = int(np.flatnonzero(good)[0])
        sigma2[g] = (1.0, LEVEL_SIGMA2[7])
        p["P1c"][g, 0] += F(3.02 * float(p["P1c"][g, 2]) / 500.0)
        good[g] = 0
    if extra == "behind_nan":
        b = np.flatnonzero(good == 0)
        p["P2c"][b[0], 2] = -p["P2c"][b[0], 2]              # behind camera 2 and, mapped, behind camera 1
        p["P1c"][b[1]] = np.nan                             # a NaN pair: never an inlier; a triple that holds it gives a NaN hypothesis
    c = {"pairs": p, "sigma2": sigma2, "good": good, "Strue": Strue, "fix_scale": fix, "cam1": cam1, "cam2": cam2, "seed": seed, "target": target}
    c["ref"] = find(p, sigma2, cam1, cam2, fix, seed)
    r = c["ref"][0]
    if target > 0:
        assert r["status"] == 1 and r["iterations"] == target, (name, r)
    elif target == 0:
        assert r["status"] == 2 and r["ninliers"] == 0, (name, r)
    return c


# found by _seed_for (tests/test_sim3_solver_cpu.py::test_the_listed_seeds_are_the_smallest checks two of them again)
SEEDS = {'n63': 2, 'n64': 3, 'n65': 4, 'n127': 23, 'n129': 5, 'n200_it64': 222, 'n200_it65': 24, 'n200_it300': 851, 'n300_fixed': 6, 'n1024': 11,
         'n1025': 5, 'n65_truncation': 3, 'n65_behind_nan': 16}
