"""Initializer (src/Initializer.cc) restated in numpy float32 / float64, rounding by rounding, next to
psl-slam_amd/csrc/initializer_kernels.h (which says where each step comes from and lists this library's readings of the OpenCV calls),
and the cases the tests share.

Every array carries a trailing "lane" axis: the hypotheses of a search, or the rows of a CheckRT.  numpy runs across lanes
(elementwise: the same single IEEE operation in every lane), never across the terms of a sum: a sum over the elements of a row, over
the rows of a score or over the keypoints of Normalize is always taken term by term in the reference's order.  A lane that the C code
would skip (the `continue` of a Jacobi pair, a row whose flag is clear) computes and is masked out.  The Jacobi sweeps of all lanes run
until no lane changes: a lane that has converged repeats its last, rotation-free sweep, which changes nothing."""
import math

import numpy as np

from sim3_solver_cases import GlibcRand, draw, random_int, same_floats  # noqa: F401  (glibc's generator and the draw are restated once)

F = np.float32
D = np.float64
RESULT_DTYPE = np.dtype([("status", "<i4"), ("nmatches", "<i4"), ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"), ("best_it_h", "<i4"),
                         ("best_it_f", "<i4"), ("inliers_h", "<i4"), ("inliers_f", "<i4"), ("H21", "<f4", (9,)), ("F21", "<f4", (9,)),
                         ("ngood", "<i4", (8,)), ("parallax", "<f4", (8,)), ("best_hypothesis", "<i4"), ("R21", "<f4", (9,)),
                         ("t21", "<f4", (3,)), ("ntriangulated", "<i4")])
assert RESULT_DTYPE.itemsize == 228
FLT_EPSILON = float(F(1.1920928955078125e-07))
FLT_MIN = 1.17549435082228750797e-38
CAM = dict(fx=517.3, fy=516.5, cx=318.6, cy=255.3)
E_INVALID, E_CAPACITY = -1, -4
LDS_ROWS, BLOCK = 512, 16          # PSL_INIT_LDS_ROWS, PSL_INIT_B of pslfe_initializer.hip
_ERR = dict(divide="ignore", invalid="ignore", over="ignore", under="ignore")


def f64(x):
    return np.asarray(x).astype(D)


def f32(x):
    return np.asarray(x).astype(F)


# ---- the draw (:77-97) ---------------------------------------------------------------------------------------------------------------
def sets(seed, N, max_its):
    G = GlibcRand(seed)
    return np.array([draw(G, N, 8) for _ in range(max_its)], np.int32).reshape(max_its, 8)


# ---- Normalize (:749-795) ------------------------------------------------------------------------------------------------------------
def normalize(keys):
    """keys float32 [n][2] -> (mx, my, sx, sy) float32"""
    n = len(keys)
    out = []
    with np.errstate(**_ERR):
        for comp in (0, 1):
            m = F(0)
            for v in keys[:, comp]:
                m = F(m + v)
            m = F(m / F(n)) if n else F(np.nan)
            dev = F(0)
            for v in keys[:, comp]:
                dev = F(dev + np.abs(F(v - m)))
            dev = F(dev / F(n)) if n else F(np.nan)
            out.append((m, F(D(1.0) / D(dev))))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def t_matrix(nm):
    mx, my, sx, sy = nm
    T = np.zeros((3, 3, 1), F)
    T[0, 0], T[0, 2], T[1, 1], T[1, 2], T[2, 2] = sx, F(-mx) * sx, sy, F(-my) * sy, F(1)
    return T


# ---- small matrices with a lane axis: [3][3][B] float32 ------------------------------------------------------------------------------
def mul33(a, b):
    return np.stack([np.stack([(a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j] for j in range(b.shape[1])]) for i in range(3)])


def mul33_t(a, b, ta):
    """a^T b (ta) or a b^T: double accumulators from 0.0"""
    rows = []
    for i in range(3):
        row = []
        for j in range(3):
            s = np.zeros(a.shape[-1], D)
            for k in range(3):
                s = s + f64(a[k, i] if ta else a[i, k]) * f64(b[k, j] if ta else b[j, k])
            row.append(f32(s))
        rows.append(np.stack(row))
    return np.stack(rows)


def det3(m):
    m = f64(m)
    return ((m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])) +
            m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def inv3(S):
    with np.errstate(**_ERR):
        d = det3(S)
        zero = d == 0.0
        d = 1.0 / d
        S = f64(S)
        t = [[(S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) * d, (S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]) * d, (S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]) * d],
             [(S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]) * d, (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) * d, (S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]) * d],
             [(S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]) * d, (S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]) * d, (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) * d]]
        out = f32(np.stack([np.stack(r) for r in t]))
        out[:, :, zero] = F(0)
    return out


def unit3(v):
    """v [3][B] / cv::norm(v)"""
    with np.errstate(**_ERR):
        d = f64(v)
        n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        return f32(d * (1.0 / n))


# ---- this library's reading of JacobiSVDImpl_<float> ---------------------------------------------------------------------------------
def jacobi(A, want_v):
    """A float32 [n][m][B], changed in place; -> (W float64 [n][B] descending, Vt float32 [n][n][B] or None)"""
    n, m, B = A.shape
    eps = 2.0 * FLT_EPSILON
    lanes = np.arange(B)
    W = np.zeros((n, B), D)
    for i in range(n):
        sd = np.zeros(B, D)
        for k in range(m):
            t = f64(A[i, k])
            sd = sd + t * t
        W[i] = sd
    V = None
    if want_v:
        V = np.zeros((n, n, B), F)
        for i in range(n):
            V[i, i] = F(1)
    with np.errstate(**_ERR):
        for _ in range(max(m, 30)):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a, b, p = W[i].copy(), W[j].copy(), np.zeros(B, D)
                    for k in range(m):
                        p = p + f64(A[i, k]) * f64(A[j, k])
                    act = ~(np.abs(p) <= eps * np.sqrt(a * b))
                    if not act.any():
                        continue
                    changed = True
                    p = p * 2
                    beta = a - b
                    gamma = np.sqrt(p * p + beta * beta)
                    delta = (gamma - beta) * 0.5
                    s_n = np.sqrt(delta / gamma)
                    c_n = p / ((gamma * s_n) * 2)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2))
                    s_p = p / ((gamma * c_p) * 2)
                    neg = beta < 0
                    c, s = np.where(neg, c_n, c_p), np.where(neg, s_n, s_p)
                    aa, bb = np.zeros(B, D), np.zeros(B, D)
                    for k in range(m):
                        x, y = f64(A[i, k]), f64(A[j, k])
                        t0, t1 = f32(c * x + s * y), f32(-s * x + c * y)
                        A[i, k], A[j, k] = np.where(act, t0, A[i, k]), np.where(act, t1, A[j, k])
                        aa = aa + f64(t0) * f64(t0)
                        bb = bb + f64(t1) * f64(t1)
                    W[i], W[j] = np.where(act, aa, W[i]), np.where(act, bb, W[j])
                    if want_v:
                        for k in range(n):
                            x, y = f64(V[i, k]), f64(V[j, k])
                            V[i, k], V[j, k] = np.where(act, f32(c * x + s * y), V[i, k]), np.where(act, f32(-s * x + c * y), V[j, k])
            if not changed:
                break
        for i in range(n):
            sd = np.zeros(B, D)
            for k in range(m):
                t = f64(A[i, k])
                sd = sd + t * t
            W[i] = np.sqrt(sd)
    for i in range(n - 1):
        j = np.full(B, i)
        for k in range(i + 1, n):
            j = np.where(W[j, lanes] < W[k], k, j)
        wi = W[i].copy()
        W[i] = W[j, lanes]
        W[j, lanes] = wi
        ai = A[i].copy()
        A[i] = A[j, :, lanes].T
        A[j, :, lanes] = ai.T
        if want_v:
            vi = V[i].copy()
            V[i] = V[j, :, lanes].T
            V[j, :, lanes] = vi.T
    return W, V


def complete(A, n, W):
    """A float32 [n1][m][B] (rows n.. are storage), W [n][B]: the left side, in place"""
    n1, m, B = A.shape
    eps = F(FLT_EPSILON) * F(2)
    state = np.full(B, 0x12345678, np.uint64)
    val0 = F(1.0 / float(m))
    with np.errstate(**_ERR):
        for i in range(n1):
            sd = W[i].copy() if i < n else np.zeros(B, D)
            for _ in range(100):
                need = sd <= FLT_MIN
                if not need.any():
                    break
                row = A[i].copy()
                st = state.copy()
                for k in range(m):
                    st = (st & np.uint64(0xffffffff)) * np.uint64(4164903690) + (st >> np.uint64(32))
                    row[k] = np.where((st & np.uint64(256)) != 0, val0, -val0)
                for _it in range(2):
                    for j in range(i):
                        s = np.zeros(B, D)
                        for k in range(m):
                            s = s + f64(row[k] * A[j, k])
                        asum = np.zeros(B, F)
                        for k in range(m):
                            t = f32(f64(row[k]) - s * f64(A[j, k]))
                            row[k] = t
                            asum = asum + np.abs(t)
                        asum = np.where(asum > eps * F(100), F(1) / asum, F(0)).astype(F)
                        for k in range(m):
                            row[k] = row[k] * asum
                s = np.zeros(B, D)
                for k in range(m):
                    t = f64(row[k])
                    s = s + t * t
                s = np.sqrt(s)
                A[i] = np.where(need, row, A[i])
                state = np.where(need, st, state)
                sd = np.where(need, s, sd)
            sc = f32(np.where(sd > FLT_MIN, 1.0 / sd, 0.0))
            A[i] = A[i] * sc


def svd3(M):
    """cv::SVD::compute of [3][3][B] -> (u, w float32 [3][B], vt)"""
    if USE_LAPACK:
        u, w, vt = np.zeros(M.shape, F), np.zeros((3, M.shape[2]), F), np.zeros(M.shape, F)
        for b in range(M.shape[2]):
            u[:, :, b], w[:, b], vt[:, :, b] = np.linalg.svd(f64(M[:, :, b]))
        return u, w, vt
    A = np.ascontiguousarray(np.transpose(M, (1, 0, 2))).astype(F)
    W, V = jacobi(A, True)
    complete(A, 3, W)
    return np.ascontiguousarray(np.transpose(A, (1, 0, 2))), f32(W), V


USE_LAPACK = False   # numpy.linalg.svd in float64 in place of the reading (for the yardstick of the ground-truth test; not bit for bit)


def _lapack_last_row(A):
    """A [r][c][B]: the last right singular vector of every lane, float32 [c][B]"""
    out = np.zeros((A.shape[1], A.shape[2]), F)
    for b in range(A.shape[2]):
        out[:, b] = np.linalg.svd(f64(A[:, :, b]), full_matrices=True)[2][-1]
    return out


# ---- ComputeH21 / ComputeF21 with the de-normalisation ---------------------------------------------------------------------------------
def _normalized(rows, idx, nm1, nm2):
    """rows float32 [N][4], idx int [B][8] -> u1, v1, u2, v2 float32 [8][B]"""
    q = rows[idx.T]                                   # [8][B][4]
    with np.errstate(**_ERR):
        return ((q[..., 0] - nm1[0]) * nm1[2], (q[..., 1] - nm1[1]) * nm1[3], (q[..., 2] - nm2[0]) * nm2[2], (q[..., 3] - nm2[1]) * nm2[3])


def hyp_h(rows, idx, nm1, nm2):
    """-> H21, H12 float32 [3][3][B]"""
    u1, v1, u2, v2 = _normalized(rows, idx, nm1, nm2)
    B = idx.shape[0]
    A = np.zeros((9, 16, B), F)                       # At
    one, zero = np.ones(B, F), np.zeros(B, F)
    for i in range(8):
        r0 = [zero, zero, zero, -u1[i], -v1[i], -one, v2[i] * u1[i], v2[i] * v1[i], v2[i]]
        r1 = [u1[i], v1[i], one, zero, zero, zero, -u2[i] * u1[i], -u2[i] * v1[i], -u2[i]]
        for c in range(9):
            A[c, 2 * i], A[c, 2 * i + 1] = r0[c], r1[c]
    if USE_LAPACK:
        Hn = _lapack_last_row(np.transpose(A, (1, 0, 2))).reshape(3, 3, B)
    else:
        _, V = jacobi(A, True)
        Hn = V[8].reshape(3, 3, B)
    T1, T2 = t_matrix(nm1), t_matrix(nm2)
    H21 = mul33(mul33(inv3(T2), Hn), T1)
    return H21, inv3(H21)


def hyp_f(rows, idx, nm1, nm2):
    """-> F21 float32 [3][3][B]"""
    u1, v1, u2, v2 = _normalized(rows, idx, nm1, nm2)
    B = idx.shape[0]
    A = np.zeros((9, 9, B), F)
    one = np.ones(B, F)
    for i in range(8):
        r = [u2[i] * u1[i], u2[i] * v1[i], u2[i], v2[i] * u1[i], v2[i] * v1[i], v2[i], u1[i], v1[i], one]
        for c in range(9):
            A[i, c] = r[c]
    if USE_LAPACK:
        Fpre = _lapack_last_row(A[:8]).reshape(3, 3, B)
        Fn = np.zeros((3, 3, B), F)
        for b in range(B):
            u, w, vt = np.linalg.svd(f64(Fpre[:, :, b]))
            w[2] = 0
            Fn[:, :, b] = (u * w) @ vt
    else:
        W, _ = jacobi(A[:8], False)
        complete(A, 8, W)
        Fpre = A[8].reshape(3, 3, B).copy()
        u, w, vt = svd3(Fpre)
        w[2] = F(0)
        Dg = np.zeros((3, 3, B), F)
        for i in range(3):
            Dg[i, i] = w[i]
        Fn = mul33(mul33(u, Dg), vt)
    T1, T2 = t_matrix(nm1), t_matrix(nm2)
    return mul33(mul33(np.ascontiguousarray(np.transpose(T2, (1, 0, 2))), Fn), T1)


# ---- CheckHomography / CheckFundamental for one row (lanes: hypotheses) or for all rows (lanes: rows) ---------------------------------
def inv_sigma2(sigma):
    return F(D(1.0) / D(F(sigma) * F(sigma)))


def score_h(H21, H12, q, inv_s2, score):
    """-> (bIn, score); H [3][3][B] or scalars, q: u1 v1 u2 v2 scalars or arrays"""
    th = F(5.991)
    u1, v1, u2, v2 = q
    with np.errstate(**_ERR):
        w2 = f32(1.0 / f64((H12[2, 0] * u2 + H12[2, 1] * v2) + H12[2, 2]))
        u2in1 = ((H12[0, 0] * u2 + H12[0, 1] * v2) + H12[0, 2]) * w2
        v2in1 = ((H12[1, 0] * u2 + H12[1, 1] * v2) + H12[1, 2]) * w2
        chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2
        out1 = chi1 > th
        score = np.where(out1, score, score + (th - chi1)).astype(F)
        w1 = f32(1.0 / f64((H21[2, 0] * u1 + H21[2, 1] * v1) + H21[2, 2]))
        u1in2 = ((H21[0, 0] * u1 + H21[0, 1] * v1) + H21[0, 2]) * w1
        v1in2 = ((H21[1, 0] * u1 + H21[1, 1] * v1) + H21[1, 2]) * w1
        chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2
        out2 = chi2 > th
        score = np.where(out2, score, score + (th - chi2)).astype(F)
    return ~(out1 | out2), score


def score_f(Fm, q, inv_s2, score):
    th, th_score = F(3.841), F(5.991)
    u1, v1, u2, v2 = q
    with np.errstate(**_ERR):
        a2 = (Fm[0, 0] * u1 + Fm[0, 1] * v1) + Fm[0, 2]
        b2 = (Fm[1, 0] * u1 + Fm[1, 1] * v1) + Fm[1, 2]
        c2 = (Fm[2, 0] * u1 + Fm[2, 1] * v1) + Fm[2, 2]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2
        out1 = chi1 > th
        score = np.where(out1, score, score + (th_score - chi1)).astype(F)
        a1 = (Fm[0, 0] * u2 + Fm[1, 0] * v2) + Fm[2, 0]
        b1 = (Fm[0, 1] * u2 + Fm[1, 1] * v2) + Fm[2, 1]
        c1 = (Fm[0, 2] * u2 + Fm[1, 2] * v2) + Fm[2, 2]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2
        out2 = chi2 > th
        score = np.where(out2, score, score + (th_score - chi2)).astype(F)
    return ~(out1 | out2), score


def _cols(rows):
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


# ---- fdlibm acosf ---------------------------------------------------------------------------------------------------------------------
def acosf(x):
    x = F(x)
    one, pi, pio2_hi, pio2_lo = F(1.0), F(3.1415925026e+00), F(1.5707962513e+00), F(7.5497894159e-08)
    pS = [F(v) for v in (1.6666667163e-01, -3.2556581497e-01, 2.0121252537e-01, -4.0055535734e-02, 7.9153501429e-04, 3.4793309169e-05)]
    qS = [F(v) for v in (-2.4033949375e+00, 2.0209457874e+00, -6.8828397989e-01, 7.7038154006e-02)]
    hx = int(np.array(x, F).view(np.int32))
    ix = hx & 0x7fffffff

    def pq(z):
        p = z * (pS[0] + z * (pS[1] + z * (pS[2] + z * (pS[3] + z * (pS[4] + z * pS[5])))))
        q = one + z * (qS[0] + z * (qS[1] + z * (qS[2] + z * qS[3])))
        return F(p / q)

    with np.errstate(**_ERR):
        if ix == 0x3f800000:
            return F(0.0) if hx > 0 else F(pi + F(2.0) * pio2_lo)
        if ix > 0x3f800000:
            return F(np.nan)
        if ix < 0x3f000000:
            if ix <= 0x23000000:
                return F(pio2_hi + pio2_lo)
            r = pq(F(x * x))
            return F(pio2_hi - (x - (pio2_lo - x * r)))
        if hx < 0:
            z = F((one + x) * F(0.5))
            s = F(np.sqrt(z))
            w = F(pq(z) * s - pio2_lo)
            return F(pi - F(2.0) * (s + w))
        z = F((one - x) * F(0.5))
        s = F(np.sqrt(z))
        df = np.array(np.array(s, F).view(np.uint32) & np.uint32(0xfffff000), np.uint32).view(F)[()]
        c = F((z - df * df) / (s + df))
        w = F(pq(z) * s + c)
        return F(F(2.0) * (df + w))


def parallax_of(cosv):
    return F(D(F(acosf(cosv) * F(180.0))) / D(3.1415926535897932384626433832795))


def cos_key(c):
    b = np.asarray(c, F).view(np.uint32).astype(np.uint64)
    return np.where(b >> 31, (~b) & 0xffffffff, b | 0x80000000).astype(np.uint32)


# ---- the stated order of vCosParallax, NaNs included, and selections to check it with ---------------------------------------------------
def _nan(sign, payload=2):
    """a quiet NaN (a signalling one does not survive a conversion) with a sign and a payload"""
    return np.array((sign << 31) | 0x7fc00000 | payload, np.uint32).view(F)[()]


# a vCosParallax in the stated order: NaNs with the sign bit set (by descending payload), -inf, the reals, +inf, NaNs with it clear
ORDERED = [_nan(1, 0x3fffff), _nan(1), _nan(1, 1), F(-np.inf), F(-1.0), F(-1e-30), F(-0.0), F(0.0), F(1e-30), F(0.5), F(0.99998), F(1.0),
           F(np.inf), _nan(0, 1), _nan(0), _nan(0, 0x3fffff)]


def selection_cases():
    """(cosines, the element at sorted index min(50, n - 1) in the stated order)"""
    rng = np.random.RandomState(5)
    out = [([c], c) for c in (ORDERED[0], ORDERED[-1], F(0.25))]
    out.append((list(ORDERED[::-1]), ORDERED[-1]))                       # 16 elements: the last in order, a NaN with the sign bit clear
    many = [F(v) for v in rng.uniform(0.9, 1.0, 300)]
    for extra in ([], [_nan(1)] * 3 + [F(-np.inf)], [_nan(1, k + 1) for k in range(60)], [_nan(0)] * 5 + [F(np.inf)]):
        v = many + list(extra)
        order = sorted(range(len(v)), key=lambda i: int(cos_key(v[i])))
        out.append(([v[i] for i in rng.permutation(len(v))], v[order[min(50, len(v) - 1)]]))
    return out


# ---- the motion hypotheses -----------------------------------------------------------------------------------------------------------
def k_matrix(cam):
    K = np.zeros((3, 3, 1), F)
    K[0, 0], K[0, 2], K[1, 1], K[1, 2], K[2, 2] = F(cam["fx"]), F(cam["cx"]), F(cam["fy"]), F(cam["cy"]), F(1)
    return K


def motion_f(F21, K):
    """-> [(R [3][3][1], t [3][1])] * 4"""
    E = mul33(mul33_t(K, F21, True), K)
    u, _, vt = svd3(E)
    t = unit3(u[:, 2].copy())
    Wm = np.zeros((3, 3, 1), F)
    Wm[0, 1], Wm[1, 0], Wm[2, 2] = F(-1), F(1), F(1)
    R1 = mul33(mul33(u, Wm), vt)
    if det3(R1)[0] < 0:
        R1 = -R1
    R2 = mul33(mul33_t(u, Wm, False), vt)
    if det3(R2)[0] < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def motion_h(H21, K):
    """-> None at the d1/d2, d2/d3 gate, or [(R, t)] * 8"""
    A = mul33(mul33(inv3(K), H21), K)
    U, w, Vt = svd3(A)
    s = F(det3(U)[0] * det3(Vt)[0])
    d1, d2, d3 = F(w[0, 0]), F(w[1, 0]), F(w[2, 0])
    with np.errstate(**_ERR):
        if D(d1 / d2) < 1.00001 or D(d2 / d3) < 1.00001:
            return None
        aux1 = F(np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)))
        aux3 = F(np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3)))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = F(np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2))
        ctheta = F((d2 * d2 + d1 * d3) / ((d1 + d3) * d2))
        stheta = [aux_st, -aux_st, -aux_st, aux_st]
        aux_sp = F(np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2))
        cphi = F((d1 * d3 - d2 * d2) / ((d1 - d3) * d2))
        sphi = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        out = []
        for h in range(8):
            i = h & 3
            Rp = np.zeros((3, 3, 1), F)
            Rp[0, 0] = Rp[1, 1] = Rp[2, 2] = F(1)
            tp = np.zeros((3, 1, 1), F)
            if h < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
                tp[0, 0], tp[1, 0], tp[2, 0] = x1[i] * (d1 - d3), F(0) * (d1 - d3), -x3[i] * (d1 - d3)
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], F(-1), sphi[i], -cphi
                tp[0, 0], tp[1, 0], tp[2, 0] = x1[i] * (d1 + d3), F(0) * (d1 + d3), x3[i] * (d1 + d3)
            R = mul33(f32(mul33(U, Rp) * s), Vt)
            t = unit3(mul33(U, tp)[:, 0])
            out.append((R, t))
    return out


# ---- CheckRT (:798-907), lanes: the rows whose flag is set ----------------------------------------------------------------------------
def check_rt(R, t, K, th2, rows, flags):
    """R [3][3][1], t [3][1]; rows float32 [N][4]; flags bool [N] -> (nGood, parallax, counted bool [N], good bool [N], p3d float32 [N][3])"""
    N = len(rows)
    counted, good, p3d = np.zeros(N, bool), np.zeros(N, bool), np.zeros((N, 3), F)
    sel = np.flatnonzero(flags)
    if len(sel) == 0:
        return 0, F(0), counted, good, p3d
    u1, v1, u2, v2 = _cols(rows[sel])
    B = len(sel)
    Rt = np.concatenate([R, t[:, None, :]], 1)                  # [3][4][1]
    P1 = np.concatenate([K, np.zeros((3, 1, 1), F)], 1)
    P2 = mul33(K, Rt)
    O2 = np.zeros((3, 1), F)
    for i in range(3):
        s = np.zeros(1, D)
        for k in range(3):
            s = s + f64(R[k, i]) * f64(t[k])
        O2[i] = f32(s * -1.0)
    with np.errstate(**_ERR):
        A = np.zeros((4, 4, B), F)                              # At
        for j in range(4):
            A[j, 0] = u1 * P1[2, j] - P1[0, j]
            A[j, 1] = v1 * P1[2, j] - P1[1, j]
            A[j, 2] = u2 * P2[2, j] - P2[0, j]
            A[j, 3] = v2 * P2[2, j] - P2[1, j]
        if USE_LAPACK:
            V3 = _lapack_last_row(np.transpose(A, (1, 0, 2)))
        else:
            _, V = jacobi(A, True)
            V3 = V[3]
        inv = 1.0 / f64(V3[3])
        p = f32(f64(V3[:3]) * inv)                             # [3][B]
        fin = np.isfinite(p).all(0)
        pd = f64(p)
        dist1 = f32(np.sqrt((pd[0] * pd[0] + pd[1] * pd[1]) + pd[2] * pd[2]))
        n2 = p - O2
        nd = f64(n2)
        dist2 = f32(np.sqrt((nd[0] * nd[0] + nd[1] * nd[1]) + nd[2] * nd[2]))
        dot = (pd[0] * nd[0] + pd[1] * nd[1]) + pd[2] * nd[2]
        cosp = f32(dot / f64(dist1 * dist2))
        low = f64(cosp) < 0.99998
        ok = fin & ~((p[2] <= 0) & low)
        p2 = mul33(R, p[:, None, :])[:, 0] + t
        ok &= ~((p2[2] <= 0) & low)
        invz1 = f32(1.0 / f64(p[2]))
        im1x, im1y = (K[0, 0] * p[0]) * invz1 + K[0, 2], (K[1, 1] * p[1]) * invz1 + K[1, 2]
        ok &= ~(((im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1)) > th2)
        invz2 = f32(1.0 / f64(p2[2]))
        im2x, im2y = (K[0, 0] * p2[0]) * invz2 + K[0, 2], (K[1, 1] * p2[1]) * invz2 + K[1, 2]
        ok &= ~(((im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2)) > th2)
    n_good = int(ok.sum())
    counted[sel], good[sel] = ok, ok & low
    p3d[sel[ok]] = p.T[ok]
    par = F(0)
    if n_good:
        keys = np.sort(cos_key(cosp[ok]))
        k = keys[min(50, n_good - 1)]
        b = np.uint32(k & np.uint32(0x7fffffff)) if (k >> 31) else np.uint32(~k)
        par = parallax_of(np.array(b, np.uint32).view(F)[()])
    return n_good, par, counted, good, p3d


def decide_f(g, par, N, min_parallax=F(1.0), min_tri=50):
    max_good = max(g[0], max(g[1], max(g[2], g[3])))
    n_min = max(int(0.9 * N), min_tri)
    nsimilar = sum(1 for k in range(4) if g[k] > 0.7 * max_good)
    if max_good < n_min or nsimilar > 1:
        return False, -1
    k = 0 if max_good == g[0] else (1 if max_good == g[1] else (2 if max_good == g[2] else 3))
    return bool(par[k] > min_parallax), k


def decide_h(g, par, N, min_parallax=F(1.0), min_tri=50):
    best_good, second, best_idx, best_par = 0, 0, -1, F(-1)
    for i in range(8):
        if g[i] > best_good:
            second, best_good, best_idx, best_par = best_good, g[i], i, par[i]
        elif g[i] > second:
            second = g[i]
    ok = second < 0.75 * best_good and best_par >= min_parallax and best_good > min_tri and best_good > 0.9 * N
    return bool(ok), best_idx


# ---- Initialize (:44-121) ------------------------------------------------------------------------------------------------------------
def initialize(keys1, keys2, matches12, cam, sigma, max_its, seed, trace=None):
    """-> dict(res RESULT_DTYPE record, p3d float32 [n1][3], tri uint8 [n1], ini int32 [n1] = mvIniMatches after Tracking.cc:712-719)"""
    keys1, keys2 = np.ascontiguousarray(keys1, F).reshape(-1, 2), np.ascontiguousarray(keys2, F).reshape(-1, 2)
    m12 = np.ascontiguousarray(matches12, np.int32)
    n1, n2 = len(keys1), len(keys2)
    res = np.zeros((), RESULT_DTYPE)
    out = dict(res=res, p3d=np.zeros((n1, 3), F), tri=np.zeros(n1, np.uint8), ini=m12.copy())
    if (m12 >= n2).any():
        res["status"] = E_INVALID
        return out
    res["best_it_h"] = res["best_it_f"] = res["best_hypothesis"] = -1
    row_i = np.flatnonzero(m12 >= 0)
    N = len(row_i)
    res["nmatches"] = N
    if N < 8:
        return out
    rows = np.concatenate([keys1[row_i], keys2[m12[row_i]]], 1)            # u1 v1 u2 v2
    nm1, nm2 = normalize(keys1), normalize(keys2)
    idx = sets(seed, N, max_its)
    inv_s2 = inv_sigma2(sigma)
    H21, H12 = hyp_h(rows, idx, nm1, nm2)
    F21 = hyp_f(rows, idx, nm1, nm2)
    sh, sf = np.zeros(max_its, F), np.zeros(max_its, F)
    for r in range(N):
        q = tuple(rows[r])
        _, sh = score_h(H21, H12, q, inv_s2, sh)
        _, sf = score_f(F21, q, inv_s2, sf)
    SH = SF = F(0)
    for it in range(max_its):
        if sh[it] > SH:
            SH, res["best_it_h"] = sh[it], it
        if sf[it] > SF:
            SF, res["best_it_f"] = sf[it], it
    res["SH"], res["SF"] = SH, SF
    bh, bf = int(res["best_it_h"]), int(res["best_it_f"])
    fl_h, fl_f = np.zeros(N, bool), np.zeros(N, bool)
    if bh >= 0:
        MH, MH12 = H21[:, :, bh], H12[:, :, bh]
        fl_h, _ = score_h(MH, MH12, _cols(rows), inv_s2, np.zeros(N, F))
        res["H21"] = MH.reshape(9)
    if bf >= 0:
        MF = F21[:, :, bf]
        fl_f, _ = score_f(MF, _cols(rows), inv_s2, np.zeros(N, F))
        res["F21"] = MF.reshape(9)
    res["inliers_h"], res["inliers_f"] = int(fl_h.sum()), int(fl_f.sum())
    if trace is not None:
        trace.update(sets=idx, sh=sh, sf=sf, rows=rows, fl_h=fl_h, fl_f=fl_f)
    if bh < 0 and bf < 0:
        res["status"] = 4
        return out
    with np.errstate(**_ERR):
        res["RH"] = F(SH / F(SH + SF))
    homography = D(res["RH"]) > 0.40
    with np.errstate(**_ERR):
        return _reconstruct(res, out, trace, homography, cam, sigma, rows, row_i, m12, fl_h, fl_f,
                            MH if bh >= 0 else None, MF if bf >= 0 else None)


def _reconstruct(res, out, trace, homography, cam, sigma, rows, row_i, m12, fl_h, fl_f, MH, MF):
    """ReconstructH / ReconstructF (:470-732) on the winner"""
    K = k_matrix(cam)
    th2 = F(4.0 * D(F(sigma) * F(sigma)))
    if homography:
        res["status"] |= 2
        hyps = motion_h(MH[:, :, None], K)
        if hyps is None:
            return out
        flags, nin = fl_h, int(fl_h.sum())
    else:
        hyps = motion_f(MF[:, :, None], K)
        flags, nin = fl_f, int(fl_f.sum())
    runs = [check_rt(R, t, K, th2, rows, flags) for R, t in hyps]
    for h, r in enumerate(runs):
        res["ngood"][h], res["parallax"][h] = r[0], r[1]
    g, par = [int(v) for v in res["ngood"]], res["parallax"]
    ok, best = decide_h(g, par, nin) if homography else decide_f(g, par, nin)
    res["best_hypothesis"] = best
    if trace is not None:
        trace.update(hyps=hyps, runs=runs)
    if not ok:
        return out
    res["status"] |= 1
    _, _, counted, good, p3d = runs[best]
    out["p3d"][row_i[counted]] = p3d[counted]
    out["tri"][row_i[good]] = 1
    res["R21"], res["t21"] = hyps[best][0].reshape(9), hyps[best][1].reshape(3)
    res["ntriangulated"] = int(good.sum())
    out["ini"][(m12 >= 0) & (out["tri"] == 0)] = -1
    return out


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def make_scene(data_seed, nmatch, kind="general", consistent=1.0, extra1=0, extra2=0, baseline=0.3, noise_px=0.0, zrange=(4.0, 9.0),
               tdir=(1.0, 0.0667, 0.1667), tilt=(0.2, -0.1)):
    """-> (keys1 [n1][2], keys2 [n2][2], matches12 [n1], (R21, t21 unit) ground truth).  The matched keypoints are spread among `extra`
    unmatched ones; keys2 is a permutation; a fraction 1 - consistent of the matches points at a random keypoint position."""
    rng = np.random.RandomState(1000 + data_seed)
    R = _rot(0.03, -0.05, 0.02)
    t = baseline * np.array(tdir)
    if kind == "rotation":
        t = np.zeros(3)
    X = np.stack([rng.uniform(-2, 2, nmatch), rng.uniform(-1.5, 1.5, nmatch), rng.uniform(zrange[0], zrange[1], nmatch)], 1)
    if kind == "planar":
        X[:, 2] = 6.0 + tilt[0] * X[:, 0] + tilt[1] * X[:, 1]
    if kind == "mixed":                             # a quarter of the points near, the others far: little parallax but no plane
        near = rng.permutation(nmatch)[:nmatch // 4]
        X[near, 2] = rng.uniform(1.0, 2.0, len(near))
        X[near, :2] *= 0.25
    if kind == "identical":
        X[:] = X[0]
    fx, fy, cx, cy = CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]

    def proj(P):
        return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], 1)

    p1, p2 = proj(X), proj(X @ R.T + t)
    if noise_px:
        p1, p2 = p1 + rng.normal(0, noise_px, p1.shape), p2 + rng.normal(0, noise_px, p2.shape)
    nbad = nmatch - int(round(consistent * nmatch))
    if nbad:
        bad = rng.choice(nmatch, nbad, replace=False)
        p2[bad] = np.stack([rng.uniform(20, 620, nbad), rng.uniform(20, 460, nbad)], 1)
    n1, n2 = nmatch + extra1, nmatch + extra2
    pos1 = np.sort(rng.choice(n1, nmatch, replace=False))
    pos2 = rng.permutation(n2)[:nmatch]
    keys1 = np.stack([rng.uniform(20, 620, n1), rng.uniform(20, 460, n1)], 1)
    keys2 = np.stack([rng.uniform(20, 620, n2), rng.uniform(20, 460, n2)], 1)
    if kind == "identical":
        keys1[:], keys2[:] = p1[0], p2[0]
    keys1[pos1], keys2[pos2] = p1, p2
    m = np.full(n1, -1, np.int32)
    m[pos1] = pos2
    nt = np.linalg.norm(t)
    return keys1.astype(F), keys2.astype(F), m, (R, t / nt if nt else t)


INF_CAM = dict(CAM, fx=float("inf"))   # K with an infinite entry: E, every (R, t), P2 and every triangulated point are not finite
# name: (data seed, matches, make_scene keywords, max_its, seed[, camera])
CASE_SPECS = {
    # match counts: nothing solved; every set takes all rows; the wave loops; the LDS row limit and one block of rows past it
    "n7": (1, 7, dict(), 24, 1), "n8": (2, 8, dict(), 24, 2), "n9": (3, 9, dict(), 24, 3),
    "n63": (4, 63, dict(), 24, 4), "n64": (5, 64, dict(), 24, 5), "n65": (6, 65, dict(), 24, 6),
    "n512": (7, LDS_ROWS, dict(), 17, 7), "n530": (8, LDS_ROWS + 18, dict(), 17, 8),
    # -1 holes: nkeys far above nmatches is what Normalize sees
    "holes": (9, 80, dict(extra1=420, extra2=300), 24, 9),
    # iteration budgets around the block of 16, and the reference's 200
    "its1": (10, 100, dict(), 1, 10), "its15": (10, 100, dict(), BLOCK - 1, 11), "its16": (10, 100, dict(), BLOCK, 12),
    "its17": (10, 100, dict(), BLOCK + 1, 13), "its200": (11, 150, dict(noise_px=0.1), 200, 0),
    # scenes
    "general": (12, 120, dict(), 24, 14),                                                   # F branch, true
    "planar": (13, 120, dict(kind="planar", tilt=(1.5, 0.5), baseline=0.5), 24, 15),        # H branch, RH > 0.40, true
    "planar_twin": (13, 120, dict(kind="planar"), 24, 15),    # a plane seen head-on: two hypotheses see every point, secondBestGood
    "rotation": (14, 120, dict(kind="rotation"), 24, 16),     # d1/d2 < 1.00001 in ReconstructH
    "lowpar": (15, 120, dict(baseline=0.14, zrange=(2.0, 20.0)), 24, 17),   # F branch, one clear winner, parallax below 1 degree
    "similar": (16, 120, dict(baseline=0.012), 24, 18),       # cosines above 0.99998: t and -t both pass, the maximum nGood is shared
    "similar_f": (16, 120, dict(kind="mixed", baseline=0.04, zrange=(8.0, 30.0)), 24, 19),   # F branch: nGood 90 and 120, nsimilar > 1
    "infinite": (12, 120, dict(), 24, 14, INF_CAM),           # every inlier row leaves CheckRT at the isfinite gate (:841): nGood 0
    "few": (17, 30, dict(), 24, 19),                          # fewer than 50 triangulated
    "half": (18, 100, dict(consistent=0.5), 200, 21),         # maxGood == nMinGood == 50: true at the edge of :517
    "fifth": (19, 200, dict(consistent=0.2), 200, 21),
    "identical": (20, 40, dict(kind="identical"), 24, 22),
    "noisy": (21, 140, dict(noise_px=0.5, extra1=30, extra2=10), 24, 23),
    "planar_noisy": (22, 140, dict(kind="planar", noise_px=0.4), 24, 24),
}
CASE_NAMES = list(CASE_SPECS)
_cache = {}


def case(name):
    """the scene and its restated result, computed once and shared"""
    if name not in _cache:
        ds, n, kw, its, seed = CASE_SPECS[name][:5]
        cam = CASE_SPECS[name][5] if len(CASE_SPECS[name]) > 5 else CAM
        k1, k2, m, truth = make_scene(ds, n, **kw)
        trace = {}
        r = initialize(k1, k2, m, cam, 1.0, its, seed, trace)
        _cache[name] = dict(keys1=k1, keys2=k2, matches=m, truth=truth, max_its=its, seed=seed, sigma=1.0, cam=cam, ref=r, trace=trace)
    return _cache[name]


def write_cases(path, cases, camera_dtype):
    with open(path, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            cam = np.zeros(1, camera_dtype)
            for k, v in c.get("cam", CAM).items():
                cam[k] = v
            f.write(cam.tobytes())
            f.write(np.uint32(c["seed"]).tobytes())
            f.write(np.array([len(c["keys1"]), len(c["keys2"]), c["max_its"]], np.int32).tobytes())
            f.write(np.float32(c["sigma"]).tobytes())
            f.write(c["keys1"].tobytes() + c["keys2"].tobytes() + c["matches"].tobytes())


def read_section(f, cases):
    out = []
    for c in cases:
        n1 = len(c["keys1"])
        res = np.frombuffer(f.read(RESULT_DTYPE.itemsize), RESULT_DTYPE)[0]
        p3d = np.frombuffer(f.read(12 * n1), F).reshape(n1, 3)
        tri = np.frombuffer(f.read(n1), np.uint8)
        ini = np.frombuffer(f.read(4 * n1), np.int32)
        out.append(dict(res=res, p3d=p3d, tri=tri, ini=ini))
    return out


def assert_same(got, ref, what, ini=True):
    """status, scores, both winning iterations, H, F, every nGood and parallax, R, t, every point and flag: bit for bit"""
    g, r = got["res"], ref["res"]
    for k in ("status", "nmatches", "best_it_h", "best_it_f", "inliers_h", "inliers_f", "best_hypothesis", "ntriangulated"):
        assert int(g[k]) == int(r[k]), (what, k, int(g[k]), int(r[k]))
    assert (g["ngood"] == r["ngood"]).all(), (what, g["ngood"], r["ngood"])
    for k in ("SH", "SF", "RH", "H21", "F21", "parallax", "R21", "t21"):
        assert same_floats(g[k], r[k]), (what, k, g[k], r[k])
    assert same_floats(got["p3d"], ref["p3d"]), (what, "p3d")
    assert (np.asarray(got["tri"]) == ref["tri"]).all(), (what, "tri")
    if ini:
        assert (np.asarray(got["ini"]) == ref["ini"]).all(), (what, "ini")
