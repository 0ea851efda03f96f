"""Optimizer::OptimizeEssentialGraph restated on Python floats: the same single IEEE operations, in the same order, as
psl-slam_amd/csrc/essential_kernels.h (the kernel k_eg_optimize and the host loop of tools/dropin/essential_main.cpp), and the graphs
the tests use.  Python floats are IEEE doubles and Python never contracts a product into a sum, so every function here is its C++
twin line by line: fdlibm_acos = psl_acos, fdlibm_log = psl_log, glibc_sin / glibc_cos = psl_glibc_sin / psl_glibc_cos on the table of
psl_sincostab.inc, s3_log = psl_s3_log, lu3 = psl_eg_lu3, Graph = psl_eg_run.  sqrt is the host's.
Restated from the reference: src/Optimizer.cc:2536-2799, Thirdparty/g2o/g2o/types/sim3.h:148-230, types_seven_dof_expmap.h:106-114,
core/base_binary_edge.hpp:55-205, core/optimization_algorithm_levenberg.cpp:61-189."""
import functools
import math
import os
import re
import struct

import numpy as np

from pose_opt_cases import _mat3mul, _quat_from_R, _quat_to_R
from sim3_opt_cases import DELTA, SCALAR, fdlibm_exp, s3_inverse, s3_map, s3_mul

KF_DTYPE = np.dtype([("Scw", "<f8", (8,)), ("Snc", "<f8", (8,)), ("has_nc", "<i4"), ("fixed", "<i4")])
EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("loop", "<i4")])
INFO_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("log_branches", "<i4"), ("nfree", "<i4"), ("chi2_start", "<f8"),
                       ("chi2_end", "<f8"), ("lambda", "<f8")])
POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,))])
MP_DTYPE = np.dtype([(k, "<f4") for k in ("x", "y", "z", "nx", "ny", "nz", "min_dist", "max_dist")])
assert KF_DTYPE.itemsize == 136 and EDGE_DTYPE.itemsize == 12 and INFO_DTYPE.itemsize == 40 and MP_DTYPE.itemsize == 32
E_INVALID, E_CAPACITY = -1, -4
ITERATIONS, LAMBDA_INIT = 20, 1e-16
EPS = 0.00001
DBL_MAX = 1.79769313486231570815e+308
THETA_MAX = 105414350.0
NAN = float("nan")
LANES = 256
CAPS = (128, 512, 512, 200000)      # keyframes, edges, points, envelope doubles: the handle of the tests


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else NAN


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def _i32(u):
    return u - (1 << 32) if u & 0x80000000 else u


_PS = (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
       7.91534994289814532176e-04, 3.47933107596021167570e-05)
_QS = (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)


def _acos_pq(z):
    p = z * (_PS[0] + z * (_PS[1] + z * (_PS[2] + z * (_PS[3] + z * (_PS[4] + z * _PS[5])))))
    q = 1.0 + z * (_QS[0] + z * (_QS[1] + z * (_QS[2] + z * _QS[3])))
    return p, q


def fdlibm_acos(x):
    """psl_acos (psl_f64math.h)"""
    pio2_hi, pio2_lo, pi = 1.57079632679489655800e+00, 6.12323399573676603587e-17, 3.14159265358979311600e+00
    u = _bits(x)
    hx = _i32(u >> 32)
    ix = hx & 0x7FFFFFFF
    if ix >= 0x3FF00000:
        if ((ix - 0x3FF00000) | (u & 0xFFFFFFFF)) == 0:
            return 0.0 if hx > 0 else pi + 2.0 * pio2_lo
        return NAN
    if ix < 0x3FE00000:
        if ix <= 0x3C600000:
            return pio2_hi + pio2_lo
        p, q = _acos_pq(x * x)
        r = p / q
        return pio2_hi - (x - (pio2_lo - r * x))
    if hx < 0:
        z = (1.0 + x) * 0.5
        p, q = _acos_pq(z)
        s = math.sqrt(z)
        r = p / q
        w = r * s - pio2_lo
        return pi - 2.0 * (s + w)
    z = (1.0 - x) * 0.5
    s = math.sqrt(z)
    df = _from_bits(_bits(s) & 0xFFFFFFFF00000000)
    c = (z - df * df) / (s + df)
    p, q = _acos_pq(z)
    r = p / q
    w = r * s + c
    return 2.0 * (df + w)


def fdlibm_log(x):
    """psl_log (psl_f64math.h), x > 0 finite"""
    ln2_hi, ln2_lo, two54 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.80143985094819840000e+16
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    u = _bits(x)
    hx = _i32(u >> 32)
    k = 0
    if hx < 0x00100000:
        k -= 54
        x *= two54
        u = _bits(x)
        hx = _i32(u >> 32)
    k += (hx >> 20) - 1023
    hx &= 0x000FFFFF
    i = (hx + 0x95F64) & 0x100000
    u = ((hx | (i ^ 0x3FF00000)) << 32) | (u & 0xFFFFFFFF)
    x = _from_bits(u)
    k += i >> 20
    f = x - 1.0
    if (0x000FFFFF & (2 + hx)) < 3:
        if f == 0.0:
            if k == 0:
                return 0.0
            dk = float(k)
            return dk * ln2_hi + dk * ln2_lo
        R = f * f * (0.5 - 0.33333333333333333 * f)
        if k == 0:
            return f - R
        dk = float(k)
        return dk * ln2_hi - ((R - dk * ln2_lo) - f)
    s = f / (2.0 + f)
    dk = float(k)
    z = s * s
    ii = hx - 0x6147A
    w = z * z
    j = 0x6B851 - hx
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
    t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    ii |= j
    R = t2 + t1
    if ii > 0:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f)


# ---- sin / cos as psl_sincos_glibc.h evaluates them (the restated tables; this host's libm differs from them by an ulp at a few angles) --
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TAB = [float.fromhex(v) for v in re.findall(r"-?0x[0-9a-fA-F.]+p[+-]\d+", re.sub(r"//.*", "", open(os.path.join(
    _ROOT, "psl-slam_amd", "csrc", "psl_sincostab.inc")).read()))]
assert len(_TAB) == 444
_BIG = float.fromhex("0x1.8000000000000p45")
_SN3, _SN5 = -1.66666666666664880952546298448555E-01, 8.33333214285722277379541354343671E-03
_CS2, _CS4, _CS6 = 4.99999999999999999999950396842453E-01, -4.16666666666664434524222570944589E-02, 1.38888874007937613028114285595617E-03


def _sg_do_sin(x, dx):
    xold = x
    if abs(x) < 0.126:
        xx = x * x
        s1, s2, s3, s4, s5 = (float.fromhex(v) for v in ("-0x1.5555555555555p-3", "0x1.1111111110ECEp-7", "-0x1.A01A019DB08B8p-13",
                                                         "0x1.71DE27B9A7ED9p-19", "-0x1.ADDFFC2FCDF59p-26"))
        t = ((((((s5 * xx + s4) * xx + s3) * xx + s2) * xx) + s1) * x - 0.5 * dx) * xx + dx
        return x + t
    if x <= 0:
        dx = -dx
    u = _BIG + abs(x)
    x = abs(x) - (u - _BIG)
    k = (_bits(u) & 0xFFFFFFFF) * 4
    xx = x * x
    s = x + (dx + x * xx * (_SN3 + xx * _SN5))
    c = x * dx + xx * (_CS2 + xx * (_CS4 + xx * _CS6))
    sn, ssn, cs, ccs = _TAB[k:k + 4]
    cor = (ssn + s * ccs - sn * c) + cs * s
    return math.copysign(sn + cor, xold)


def _sg_do_cos(x, dx):
    if x < 0:
        dx = -dx
    u = _BIG + abs(x)
    x = abs(x) - (u - _BIG) + dx
    k = (_bits(u) & 0xFFFFFFFF) * 4
    xx = x * x
    s = x + x * xx * (_SN3 + xx * _SN5)
    c = xx * (_CS2 + xx * (_CS4 + xx * _CS6))
    sn, ssn, cs, ccs = _TAB[k:k + 4]
    cor = (ccs - s * ssn - cs * c) - sn * s
    return cs + cor


_HP0, _HP1 = 1.5707963267948966, 6.123233995736766e-17


def glibc_sin(x):
    """psl_glibc_sin for |x| < 2.426265 (every angle here is at most pi: the larger ones go to the host's libm, which the restated
    reduction equals)"""
    ax = abs(x)
    if ax < 2.0 ** -26:
        return x
    if ax < 0.855469:
        return _sg_do_sin(x, 0.0)
    if ax < 2.426265:
        return math.copysign(_sg_do_cos(_HP0 - ax, _HP1), x)
    return math.sin(x)


def glibc_cos(x):
    ax = abs(x)
    if ax < 2.0 ** -27:
        return 1.0
    if ax < 0.855469:
        return _sg_do_cos(x, 0.0)
    if ax < 2.426265:
        y = _HP0 - ax
        a = y + _HP1
        return _sg_do_sin(a, (y - a) + _HP1)
    return math.cos(x)


def s3_exp(x):
    """psl_s3_exp (sim3_kernels.h), as sim3_opt_cases.s3_exp with the restated sin / cos -> (Sim3, branch)"""
    sigma = x[6]
    theta = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    O = [0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0]
    s = fdlibm_exp(sigma)
    O2 = _mat3mul(O, O)
    eye = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    big_sigma, big_theta = not (abs(sigma) < EPS), not (theta < EPS)
    if big_theta:
        sn, cs = glibc_sin(theta), glibc_cos(theta)
        a, b = _div(sn, theta), _div(1.0 - cs, theta * theta)
        R = [(eye[i] + a * O[i]) + b * O2[i] for i in range(9)]
        if not big_sigma:
            theta2 = theta * theta
            C, A, B = 1.0, _div(1.0 - cs, theta2), _div(theta - sn, theta2 * theta)
        else:
            C = _div(s - 1.0, sigma)
            sa, sb = s * sn, s * cs
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = _div(sa * sigma + (1.0 - sb) * theta, theta * c)
            B = _div(C - _div((sb - 1.0) * sigma + sa * theta, c), theta2)
    else:
        R = [(eye[i] + O[i]) + O2[i] for i in range(9)]
        if not big_sigma:
            C, A, B = 1.0, 1.0 / 2.0, 1.0 / 6.0
        else:
            C = _div(s - 1.0, sigma)
            sigma2 = sigma * sigma
            A = _div((sigma - 1.0) * s + 1.0, sigma2)
            B = _div(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma)
    q = _quat_from_R(R)
    W = [(A * O[i] + B * O2[i]) + C * eye[i] for i in range(9)]
    t = [(W[3 * i] * x[3] + W[3 * i + 1] * x[4]) + W[3 * i + 2] * x[5] for i in range(3)]
    return (q, t, s), int(big_sigma) * 2 + int(big_theta)


def s3_oplus(x, fix_scale, S):
    """VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69) -> (Sim3, branch)"""
    u = list(x)
    if fix_scale:
        u[6] = 0.0
    d, branch = s3_exp(u)
    return s3_mul(d, S), branch


def lu3(W, t):
    """psl_eg_lu3: W x = t by LU with partial pivoting, the first largest |entry| of the column"""
    a, b, c = [W[0], W[1], W[2], t[0]], [W[3], W[4], W[5], t[1]], [W[6], W[7], W[8], t[2]]
    fa, fb, fc = abs(a[0]), abs(b[0]), abs(c[0])
    p = 2 if (fc > fa and fc > fb) else (1 if fb > fa else 0)
    if p == 1:
        a, b = b, a
    elif p == 2:
        a, c = c, a
    f1, f2 = _div(b[0], a[0]), _div(c[0], a[0])
    for k in range(1, 4):
        b[k] = b[k] - f1 * a[k]
        c[k] = c[k] - f2 * a[k]
    if abs(c[1]) > abs(b[1]):
        b, c = c, b
    f = _div(c[1], b[1])
    for k in range(2, 4):
        c[k] = c[k] - f * b[k]
    x2 = _div(c[3], c[2])
    x1 = _div(b[3] - b[2] * x2, b[1])
    x0 = _div((a[3] - a[1] * x1) - a[2] * x2, a[0])
    return [x0, x1, x2]


def s3_log(S):
    """psl_s3_log -> ([omega, upsilon, sigma], branch = (|sigma| >= eps) * 2 + !(d > 1 - eps))"""
    q, t, s = S
    sigma = fdlibm_log(s)
    R = _quat_to_R(q)
    d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0)
    dR = [R[7] - R[5], R[2] - R[6], R[3] - R[1]]
    big_sigma, big_theta = not (abs(sigma) < EPS), not (d > 1.0 - EPS)
    branch = int(big_sigma) * 2 + int(big_theta)
    if not big_theta:
        om = [0.5 * v for v in dR]
        if not big_sigma:
            C, A, B = 1.0, 1.0 / 2.0, 1.0 / 6.0
        else:
            C = _div(s - 1.0, sigma)
            sigma2 = sigma * sigma
            A = _div((sigma - 1.0) * s + 1.0, sigma2)
            B = _div(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma)
    else:
        theta = fdlibm_acos(d)
        if theta != theta:
            return [theta] * 6 + [sigma], branch
        f = _div(theta, 2.0 * _sqrt(1.0 - d * d))
        om = [f * v for v in dR]
        theta2 = theta * theta
        sn, cs = glibc_sin(theta), glibc_cos(theta)
        if not big_sigma:
            C, A, B = 1.0, _div(1.0 - cs, theta2), _div(theta - sn, theta2 * theta)
        else:
            C = _div(s - 1.0, sigma)
            a, bb = s * sn, s * cs
            c = theta2 + sigma * sigma
            A = _div(a * sigma + (1.0 - bb) * theta, theta * c)
            B = _div(C - _div((bb - 1.0) * sigma + a * theta, c), theta2)
    O = [0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0]
    BOO = _mat3mul([B * v for v in O], O)
    W = [(A * O[i] + BOO[i]) + C * (1.0 if i % 4 == 0 else 0.0) for i in range(9)]
    return om + lu3(W, t) + [sigma], branch


def load(r):
    r = [float(v) for v in r]
    return r[0:4], r[4:7], r[7]


def store(S):
    return list(S[0]) + list(S[1]) + [S[2]]


def edge_error(C, v1, v2i):
    """EdgeSim3::computeError: log((C * v1) * v2^-1)"""
    return s3_log(s3_mul(s3_mul(C, v1), v2i))


def chi2(e):
    c = e[0] * e[0]
    for r in range(1, 7):
        c = c + e[r] * e[r]
    return c


def sum256(vals):
    """the ordered sum of lm_device.h on one value per edge: partial sum p takes the edges p, p + 256, ...; a butterfly in each group
    of 64; ((G0 + G1) + G2) + G3"""
    part = [0.0] * LANES
    for p in range(LANES):
        s = 0.0
        for e in range(p, len(vals), LANES):
            s = s + vals[e]
        part[p] = s
    G = []
    for g in range(4):
        p = part[64 * g:64 * g + 64]
        s = 32
        while s >= 1:
            for l in range(s):
                p[l] = p[l] + p[l + s]
            s >>= 1
        G.append(p[0])
    return ((G[0] + G[1]) + G[2]) + G[3]


def good_scale(rho):
    t = 2.0 * rho - 1.0
    alpha = 1.0 - (t * t) * t
    alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
    return alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0)


def dense_ldlt_solve(A, b):
    """the dense LDLt of ba_kernels.h / psl_lm_solve on a full symmetric matrix (lists): the arithmetic the envelope form restricts.
    -> (x, L, D) or None for a pivot that is not a finite positive number"""
    n = len(b)
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    for j in range(n):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * (L[j][k] * D[k])
        if not (d > 0.0) or not (d <= DBL_MAX):
            return None
        D[j] = d
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * (L[j][k] * D[k])
            L[i][j] = _div(s, d)
    y = [0.0] * n
    for i in range(n):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [0.0] * n
    for i in range(n - 1, -1, -1):
        s = _div(y[i], D[i])
        for k in range(i + 1, n):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x, L, D


class Graph:
    """psl_eg_run on one graph.  kf, edges: KF_DTYPE / EDGE_DTYPE arrays; mp: MP_DTYPE; mp_ref int32."""

    def __init__(self, kf, edges, mp, mp_ref, fix_scale, caps=CAPS):
        self.kf, self.edges, self.mp, self.mp_ref = kf, edges, mp, np.asarray(mp_ref, np.int32)
        self.nkf, self.ne, self.nmp = len(kf), len(edges), len(mp)
        self.fix_scale, self.caps = bool(fix_scale), caps
        self.ei = [int(v) for v in edges["i"]]
        self.ej = [int(v) for v in edges["j"]]
        self.mask = 0
        self.trials = []

    # ---- the checks and the lists
    def check(self):
        ckf, ced, cmp_, cenv = self.caps
        if self.nkf > ckf or self.ne > ced or self.nmp > cmp_:
            return E_CAPACITY
        for i, j in zip(self.ei, self.ej):
            if i < 0 or i >= self.nkf or j < 0 or j >= self.nkf or i == j:
                return E_INVALID
        if ((self.mp_ref < -1) | (self.mp_ref >= self.nkf)).any():
            return E_INVALID
        self.S0 = [load(r) for r in self.kf["Scw"]]
        self.S = list(self.S0)
        self.pidx, self.kfof = [], []
        for v in range(self.nkf):
            self.pidx.append(-1 if self.kf["fixed"][v] else len(self.kfof))
            if not self.kf["fixed"][v]:
                self.kfof.append(v)
        self.F = len(self.kfof)
        self.items = [[] for _ in range(self.nkf)]
        for e in range(self.ne):
            self.items[self.ei[e]].append(2 * e)
            self.items[self.ej[e]].append(2 * e + 1)
        self.fb = []
        for bi, v in enumerate(self.kfof):
            lo = bi
            for it in self.items[v]:
                o = self.pidx[self.other(it)]
                if 0 <= o < lo:
                    lo = o
            self.fb.append(lo)
        self.env_size = sum(r - 7 * self.fb[r // 7] + 1 for r in range(7 * self.F))
        if self.env_size > cenv:
            return E_CAPACITY
        self.lastblk = []
        for bj in range(self.F):
            bi = self.F - 1
            while bi > bj and self.fb[bi] > bj:
                bi -= 1
            self.lastblk.append(bi)
        return 0

    def other(self, it):
        return self.ei[it >> 1] if it & 1 else self.ej[it >> 1]

    def measure(self):
        self.meas = []
        for e in range(self.ne):
            loop = int(self.edges["loop"][e])
            pick = lambda v: load(self.kf["Snc"][v] if (not loop and self.kf["has_nc"][v]) else self.kf["Scw"][v])
            self.meas.append(s3_mul(pick(self.ej[e]), s3_inverse(pick(self.ei[e]))))

    # ---- one linearisation: errors, Jacobians, blocks
    def linearize(self):
        S, fs = self.S, self.fix_scale
        Si = [s3_inverse(s) for s in S]
        pert = {}
        for v in range(self.nkf):
            if self.pidx[v] < 0:
                continue
            row = []
            for k in range(14):
                u = [0.0] * 7
                u[k >> 1] = -DELTA if k & 1 else DELTA
                Sp = s3_oplus(u, fs, S[v])[0]
                row.append((Sp, s3_inverse(Sp)))
            pert[v] = row
        self.err, self.rho0, self.J = [], [], []
        for e in range(self.ne):
            i, j, C = self.ei[e], self.ej[e], self.meas[e]
            er, br = edge_error(C, S[i], Si[j])
            self.mask |= 1 << br
            self.err.append(er)
            self.rho0.append(chi2(er))
            halves = []
            for half, v in ((0, i), (1, j)):
                if self.pidx[v] < 0:
                    halves.append(None)
                    continue
                J = [0.0] * 49
                for d in range(7):
                    if half == 0:
                        ep, b1 = edge_error(C, pert[v][2 * d][0], Si[j])
                        em, b2 = edge_error(C, pert[v][2 * d + 1][0], Si[j])
                    else:
                        ep, b1 = edge_error(C, S[i], pert[v][2 * d][1])
                        em, b2 = edge_error(C, S[i], pert[v][2 * d + 1][1])
                    self.mask |= (1 << b1) | (1 << b2)
                    for r in range(7):
                        J[7 * r + d] = SCALAR * (ep[r] - em[r])
                halves.append(J)
            self.J.append(halves)

    def item_J(self, it):
        return self.J[it >> 1][it & 1]

    def build(self):
        F = self.F
        self.Hd = [[0.0] * 49 for _ in range(F)]
        self.b = [0.0] * (7 * F)
        for bi, v in enumerate(self.kfof):
            for h in range(56):
                a, c = (h // 7, h % 7) if h < 49 else (h - 49, 0)
                acc = 0.0
                for it in self.items[v]:
                    J, er = self.item_J(it), self.err[it >> 1]
                    if h < 49:
                        s = J[a] * J[c]
                        for r in range(1, 7):
                            s = s + J[7 * r + a] * J[7 * r + c]
                    else:
                        s = J[a] * er[0]
                        for r in range(1, 7):
                            s = s + J[7 * r + a] * er[r]
                    acc = acc + s
                if h < 49:
                    self.Hd[bi][h] = acc
                else:
                    self.b[7 * bi + a] = -acc
        self.Henv = []
        for r in range(7 * F):
            bi, a = r // 7, r % 7
            v = self.kfof[bi]
            row = [0.0] * (r - 7 * self.fb[bi] + 1)
            for c in range(a + 1):
                row[7 * bi + c - 7 * self.fb[bi]] = self.Hd[bi][7 * a + c]
            for bj in range(self.fb[bi], bi):
                u = self.kfof[bj]
                for c in range(7):
                    acc = 0.0
                    for it in self.items[v]:
                        if self.other(it) != u:
                            continue
                        J, Jo = self.item_J(it), self.item_J(it ^ 1)
                        s = J[a] * Jo[c]
                        for k in range(1, 7):
                            s = s + J[7 * k + a] * Jo[7 * k + c]
                        acc = acc + s
                    row[7 * bj + c - 7 * self.fb[bi]] = acc
            self.Henv.append(row)

    def dense(self, lam=0.0):
        """H + lam I as a full symmetric matrix of lists (zeros outside the envelope)"""
        n = 7 * self.F
        A = [[0.0] * n for _ in range(n)]
        for r, row in enumerate(self.Henv):
            k0 = 7 * self.fb[r // 7]
            for k, v in enumerate(row):
                A[r][k0 + k] = v
                A[k0 + k][r] = v
            A[r][r] = row[r - k0] + lam
        return A

    def solve(self, lam):
        """psl_eg_solve -> (x or None, why)"""
        N, fb = 7 * self.F, self.fb
        L = [list(r) for r in self.Henv]
        for r in range(N):
            L[r][-1] = self.Henv[r][-1] + lam
        D = [0.0] * N
        for j in range(N):
            j0, rj = 7 * fb[j // 7], L[j]
            d = rj[j - j0]
            for k in range(j0, j):
                d = d - rj[k - j0] * (rj[k - j0] * D[k])
            if not (d > 0.0) or not (d <= DBL_MAX):
                return None, "pivot"
            D[j] = d
            for i in range(j + 1, 7 * self.lastblk[j // 7] + 7):
                i0 = 7 * fb[i // 7]
                if i0 > j:
                    continue
                ri = L[i]
                s = ri[j - i0]
                for k in range(max(i0, j0), j):
                    s = s - ri[k - i0] * (rj[k - j0] * D[k])
                ri[j - i0] = _div(s, d)
        y = [0.0] * N
        for i in range(N):
            s, k0 = self.b[i], 7 * fb[i // 7]
            for k in range(k0, i):
                s = s - L[i][k - k0] * y[k]
            y[i] = s
        x = [0.0] * N
        for i in range(N - 1, -1, -1):
            s = _div(y[i], D[i])
            for k in range(i + 1, 7 * self.lastblk[i // 7] + 7):
                k0 = 7 * fb[k // 7]
                if k0 > i:
                    continue
                s = s - L[k][i - k0] * x[k]
            x[i] = s
        self.L, self.D = L, D
        for i in range(self.F):
            th = _sqrt((x[7 * i] * x[7 * i] + x[7 * i + 1] * x[7 * i + 1]) + x[7 * i + 2] * x[7 * i + 2])
            if not (th < THETA_MAX):
                return None, "step"
        return x, "ok"

    def levenberg(self, iterations=ITERATIONS, lambda_init=LAMBDA_INIT):
        its, lam, ni, nbad = 0, 0.0, 2.0, 0
        chi_first = chi_last = 0.0
        for it in range(iterations):
            self.linearize()
            chi = sum256(self.rho0)
            ini_chi = chi
            if it == 0:
                chi_first = chi
            self.build()
            if it == 0:
                lam, ni, nbad = lambda_init, 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                x, why = self.solve(lam)
                temp_chi, scale = DBL_MAX, 0.0
                if x is not None:
                    Sn = list(self.S)
                    for v in range(self.nkf):
                        i = self.pidx[v]
                        if i < 0:
                            continue
                        if self.fix_scale:
                            x[7 * i + 6] = 0.0
                        Sn[v] = s3_oplus(x[7 * i:7 * i + 7], self.fix_scale, self.S[v])[0]
                    Sni = [s3_inverse(s) for s in Sn]
                    rho0 = []
                    for e in range(self.ne):
                        er, br = edge_error(self.meas[e], Sn[self.ei[e]], Sni[self.ej[e]])
                        self.mask |= 1 << br
                        rho0.append(chi2(er))
                    temp_chi = sum256(rho0)
                    for j in range(7 * self.F):
                        scale = scale + x[j] * (lam * x[j] + self.b[j])
                scale = scale + 1e-3
                rho = _div(chi - temp_chi, scale)
                self.trials.append((it, x is not None, why, rho, lam))
                if rho > 0 and abs(temp_chi) <= DBL_MAX:
                    lam = lam * good_scale(rho)
                    ni = 2.0
                    chi = temp_chi
                    if x is not None:
                        self.S = Sn
                else:
                    lam = lam * ni
                    ni = ni * 2.0
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            its += 1
            chi_last = chi
            if qmax == 10 or rho == 0:
                break
            nbad = nbad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
            if nbad >= 3:
                break
        return its, chi_first, chi_last, lam

    def run(self):
        info = np.zeros((), INFO_DTYPE)
        pose = np.zeros(self.nkf, POSE_DTYPE)
        code = self.check()
        if code != 0:
            info["status"] = code
            return dict(info=info, pose=pose, S=np.array(self.kf["Scw"], np.float64).reshape(self.nkf, 8), mp=self.mp.copy(), graph=self)
        its, c0, c1, lam = 0, 0.0, 0.0, 0.0
        if self.F > 0 and self.ne > 0:
            self.measure()
            its, c0, c1, lam = self.levenberg()
        info["iterations"], info["log_branches"], info["nfree"] = its, self.mask if its else 0, self.F
        info["chi2_start"], info["chi2_end"], info["lambda"] = c0, c1, lam
        S_out = np.zeros((self.nkf, 8))
        Swc = []
        for v, S in enumerate(self.S):
            Swc.append(s3_inverse(S))
            R = _quat_to_R(S[0])
            inv = _div(1.0, S[2])
            pose["R"][v] = np.array(R, np.float64).astype(np.float32)
            pose["t"][v] = np.array([S[1][k] * inv for k in range(3)], np.float64).astype(np.float32)
            S_out[v] = store(S)
        mp = self.mp.copy()
        for p in range(self.nmp):
            r = int(self.mp_ref[p])
            if r < 0:
                continue
            P = [float(mp[k][p]) for k in "xyz"]
            c = s3_map(Swc[r], s3_map(self.S0[r], P))
            for k, v in zip("xyz", c):
                mp[k][p] = np.float32(v)
        return dict(info=info, pose=pose, S=S_out, mp=mp, graph=self)


def optimize(kf, edges, mp, mp_ref, fix_scale, caps=CAPS):
    return Graph(kf, edges, mp, mp_ref, fix_scale, caps).run()


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------
def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = 0.5 * angle
    return [float(a[0] * math.sin(h)), float(a[1] * math.sin(h)), float(a[2] * math.sin(h)), float(math.cos(h))]


def sim3(axis, angle, t, s=1.0):
    return quat(axis, angle), [float(v) for v in t], float(s)


def kf_rows(Scw, Snc=None, fixed=(0,)):
    kf = np.zeros(len(Scw), KF_DTYPE)
    for v, S in enumerate(Scw):
        kf["Scw"][v] = store(S)
        kf["Snc"][v] = store(S)
        if Snc is not None and Snc[v] is not None:
            kf["Snc"][v] = store(Snc[v])
            kf["has_nc"][v] = 1
    for v in fixed:
        kf["fixed"][v] = 1
    return kf


def edge_rows(pairs):
    ed = np.zeros(len(pairs), EDGE_DTYPE)
    for e, p in enumerate(pairs):
        ed["i"][e], ed["j"][e], ed["loop"][e] = p[0], p[1], p[2] if len(p) > 2 else 0
    return ed


def points(rng, n, nkf, unchanged=()):
    mp = np.zeros(n, MP_DTYPE)
    for k in "xyz":
        mp[k] = rng.uniform(-4, 4, n).astype(np.float32)
    mp["nx"], mp["min_dist"], mp["max_dist"] = 1.0, 0.5, 20.0
    ref = rng.randint(0, nkf, n).astype(np.int32) if nkf else np.full(n, -1, np.int32)
    for p in unchanged:
        ref[p] = -1
    return mp, ref


def ring(n, seed, drift=0.01, scale_drift=0.0, span=(1, 2), loops=1, fixed=(0,), npoints=0, fix_scale=False, corrected=2, bias=False):
    """n keyframes on a circle looking inwards; the estimates drift along the chain (rotation, translation and, with scale_drift, scale;
    an independent random step per keyframe, or with `bias` the same step every time, as an odometry bias accumulates);
    edges (i, i - d) for d in span in the reference's order per keyframe; `loops` loop connections from the last rows to the first
    ones, carrying the true relative Sim3 (the last `corrected` rows have their true Sim3 as the CorrectedSim3 entry and the drifted one
    as the NonCorrectedSim3 entry).  -> case dict with the ground truth"""
    rng = np.random.RandomState(seed)
    true, est, step = [], [], None
    for v in range(n):
        a = 2 * math.pi * v / n * 0.9
        T = sim3([0.1, 1.0, 0.05], a, [2.0 * math.sin(a) + 0.1 * v / n, 0.05 * v, 2.0 * math.cos(a)])
        true.append(T)
        if v and not (bias and v > 1):
            step = sim3(rng.uniform(-1, 1, 3), drift * rng.uniform(0.5, 1.0), drift * rng.uniform(-1, 1, 3), 1.0 + scale_drift * rng.uniform(0.5, 1.0))
        # odometry: the relative motion is measured up to a small step error, which accumulates along the chain
        est.append(s3_mul(step, s3_mul(s3_mul(T, s3_inverse(true[v - 1])), est[v - 1])) if v else T)
    Scw, Snc = list(est), [None] * n
    for v in range(n - corrected, n):
        Scw[v], Snc[v] = true[v], est[v]
    pairs = []
    for l in range(loops):                      # LoopConnections first (:2607-2635)
        pairs.append((n - 1 - l, l, 1))
    for i in range(n):
        for d in span:
            if i - d >= 0 and not any(p[2] and {p[0], p[1]} == {i, i - d} for p in pairs):
                pairs.append((i, i - d, 0))
    kf, ed = kf_rows(Scw, Snc, fixed), edge_rows(pairs)
    mp, ref = points(rng, npoints, n, unchanged=range(0, npoints, 17))
    return dict(kf=kf, edges=ed, mp=mp, mp_ref=ref, fix_scale=fix_scale, true=true)


def branches_graph():
    """all four branches of log in one graph: the NonCorrectedSim3 entry of rows 1..4 differs from vScw by nothing, a pure scale, a pure
    rotation and both, so the first errors are log of exactly those; a chain holds the rows together"""
    base = [sim3([0.2, 1, 0.1], 0.3 * v, [0.5 * v, 0.1 * v, 0.2]) for v in range(5)]
    deltas = [None, sim3([0, 0, 1], 0.0, [0, 0, 0], 1.0), sim3([0, 0, 1], 0.0, [0, 0, 0], 1.25), sim3([1, 2, 0.5], 0.4, [0.05, 0, 0.02], 1.0),
              sim3([0.3, -1, 0.5], 0.7, [0.01, 0.03, 0], 0.8)]
    Snc = [None] + [s3_mul(deltas[v], base[v]) for v in range(1, 5)]
    kf = kf_rows(base, Snc, fixed=(0,))
    ed = edge_rows([(0, 1), (0, 2), (0, 3), (0, 4), (2, 1), (3, 2), (4, 3)])
    rng = np.random.RandomState(5)
    mp, ref = points(rng, 9, 5)
    return dict(kf=kf, edges=ed, mp=mp, mp_ref=ref, fix_scale=False)


SPECS = {
    "two_one_fixed": lambda: ring(2, 1, span=(1,), loops=0, corrected=1, npoints=3),
    "fixed_in_middle": lambda: ring(5, 2, span=(1,), loops=0, fixed=(2,), corrected=1, npoints=5),
    "chain5_loop": lambda: ring(5, 3, span=(1,), loops=1, fixed=(1,), npoints=7, scale_drift=0.01),
    "chain5_loop_fix_scale": lambda: ring(5, 3, span=(1,), loops=1, fixed=(1,), npoints=7, fix_scale=True),
    "free_without_edge": lambda: _isolated(),
    "ring12": lambda: ring(12, 4, drift=0.02, scale_drift=0.01, npoints=20, bias=True),
    "ring12_fix_scale": lambda: ring(12, 4, drift=0.02, npoints=20, fix_scale=True, bias=True),
    "two_long_rows": lambda: ring(10, 6, span=(1, 2), loops=2, fixed=(4,), npoints=4),
    "big_100_300": lambda: ring(100, 7, drift=0.002, scale_drift=0.001, span=(1, 2, 3), loops=6, npoints=300),
    "branches": branches_graph,
}
CASE_NAMES = list(SPECS)


def _isolated():
    c = ring(5, 8, span=(1, 2), loops=0, corrected=1, npoints=4)
    c["edges"] = c["edges"][(c["edges"]["i"] != 3) & (c["edges"]["j"] != 3)]       # row 3 keeps no edge
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    c = SPECS[name]()
    c["name"] = name
    c["ref"] = optimize(c["kf"], c["edges"], c["mp"], c["mp_ref"], c["fix_scale"])
    return c


def refused_cases():
    """an empty graph, one above the keyframe cap, one with an edge outside its rows, one with i == j, one with a point outside"""
    empty = dict(kf=np.zeros(0, KF_DTYPE), edges=np.zeros(0, EDGE_DTYPE), mp=np.zeros(0, MP_DTYPE), mp_ref=np.zeros(0, np.int32), fix_scale=False)
    over = ring(CAPS[0] + 1, 9, span=(1,), loops=0, corrected=0, npoints=2)
    base = case("chain5_loop")
    outside = dict(base, edges=base["edges"].copy())
    outside["edges"]["j"][1] = 5
    selfloop = dict(base, edges=base["edges"].copy())
    selfloop["edges"]["j"][2] = selfloop["edges"]["i"][2]
    badpoint = dict(base, mp_ref=base["mp_ref"].copy())
    badpoint["mp_ref"][1] = 5
    out = []
    for c, st in ((empty, 0), (over, E_CAPACITY), (outside, E_INVALID), (selfloop, E_INVALID), (badpoint, E_INVALID)):
        c = dict(c)
        c["ref"] = optimize(c["kf"], c["edges"], c["mp"], c["mp_ref"], c["fix_scale"])
        assert int(c["ref"]["info"]["status"]) == st, (st, c["ref"]["info"])
        out.append(c)
    return out


# ---- the case file of tools/dropin/essential_main.cpp --------------------------------------------------------------------------------
def write_cases(path, cases, fix_scale, caps=CAPS):
    with open(path, "wb") as f:
        f.write(struct.pack("<6iq", len(cases), int(fix_scale), caps[0], caps[1], caps[2], 0, caps[3]))
        for c in cases:
            f.write(struct.pack("<3i", len(c["kf"]), len(c["edges"]), len(c["mp"])))
            f.write(c["kf"].tobytes() + c["edges"].tobytes() + c["mp"].tobytes() + np.asarray(c["mp_ref"], np.int32).tobytes())


def read_sections(path, cases, nsections):
    buf = open(path, "rb").read()
    at, out = 0, []
    for _ in range(nsections):
        sec = []
        for c in cases:
            nkf, nmp = len(c["kf"]), len(c["mp"])
            info = np.frombuffer(buf, INFO_DTYPE, 1, at)[0]
            at += INFO_DTYPE.itemsize
            pose = np.frombuffer(buf, POSE_DTYPE, nkf, at)
            at += nkf * POSE_DTYPE.itemsize
            S = np.frombuffer(buf, np.float64, 8 * nkf, at).reshape(nkf, 8)
            at += 64 * nkf
            mp = np.frombuffer(buf, MP_DTYPE, nmp, at)
            at += nmp * MP_DTYPE.itemsize
            sec.append(dict(info=info, pose=pose, S=S, mp=mp))
        out.append(sec)
    assert at == len(buf), (at, len(buf))
    return out


def assert_equal_ref(got, ref, what=""):
    """every output byte; a refused graph has no pose rows"""
    assert got["info"].tobytes() == ref["info"].tobytes(), (what, got["info"], ref["info"])
    assert np.asarray(got["S"], np.float64).tobytes() == np.asarray(ref["S"], np.float64).tobytes(), (what, "S")
    assert got["mp"].tobytes() == ref["mp"].tobytes(), (what, "mp")
    if int(ref["info"]["status"]) == 0:
        assert got["pose"].tobytes() == ref["pose"].tobytes(), (what, "pose")
