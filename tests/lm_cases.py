"""g2o's Levenberg loop on one vertex in numpy float64 and Python floats: the restatement of psl-slam_amd/csrc/lm_kernels.h that
tests/pose_opt_cases.py (six unknowns, with tests/pose_lil_cases.py) and tests/sim3_opt_cases.py (seven) share - the LDLt solve, lambda,
the two orders of the sums and levenberg(), one optimize() call.  It mirrors the C++ operation by operation and decision by decision
(every numpy ufunc is one IEEE operation; nothing here goes through BLAS) and shares no text with it."""
import math

import numpy as np

DBL_MAX = 1.79769313486231570815e+308
LANES, GROUP = 256, 64
THETA_MAX = 105414350.0           # PSL_LM_THETA_MAX: the range of the device's sin / cos


def _div(a, b):
    """IEEE a / b for Python floats."""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def sum_device(seq, active):
    """The order of the sums of pslfe_pose.hip and pslfe_sim3.hip on seq [nt][A][k], the up to A additions of every edge (a point
    edge has one, a LIL edge six, a Sim3 pair two; the rest is +0): partial sum p of 256 takes the edges p, p + 256, ... in ascending
    order and, of each, its additions in order; a butterfly in each group of 64; the four group sums from left to right.  (A partial
    sum starts at +0 and is never -0, so adding +0 for an edge the device skips, or for an addition an edge does not have, changes no
    bit.)"""
    nt, A, k = seq.shape
    c = max(-(-nt // LANES), 1)
    P = np.zeros((c * LANES, A, k))
    P[:nt] = np.where(active[:, None, None], seq, 0.0)
    P = P.reshape(c, LANES, A, k)
    part = np.zeros((LANES, k))
    for ci in range(c):
        for s in range(A):
            part = part + P[ci, :, s]
    g = part.reshape(LANES // GROUP, GROUP, k)
    s = GROUP // 2
    while s >= 1:
        g[:, :s] = g[:, :s] + g[:, s:2 * s]
        s //= 2
    G = g[:, 0]
    return ((G[0] + G[1]) + G[2]) + G[3]


def sum_edge(seq, active, steps=None):
    """Edge by edge in index order, of each edge its steps[i] additions (all A without steps) in order: g2o's order of the edges."""
    s = np.zeros(seq.shape[2])
    for i in np.flatnonzero(active):
        for r in range(seq.shape[1] if steps is None else steps[i]):
            s = s + seq[i, r]
    return s


def solve(n, H, lam, b):
    """(H + lam I) x = b in n unknowns by LDLt without pivoting, H: the n (n + 1) / 2 upper-triangle values row by row; None when a
    pivot is not a finite positive number."""
    A = [[0.0] * n for _ in range(n)]
    h = 0
    for j in range(n):
        for k in range(j, n):
            A[j][k] = A[k][j] = float(H[h])
            h += 1
    for j in range(n):
        A[j][j] = A[j][j] + lam
    L = [[0.0] * n for _ in range(n)]
    D = [0.0] * n
    ok = True
    for j in range(n):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * (L[j][k] * D[k])
        if not (d > 0.0) or not (d <= DBL_MAX):
            ok = False
        D[j] = d
        for i in range(j + 1, n):
            s = A[i][j]
            for k in range(j):
                s = s - L[i][k] * (L[j][k] * D[k])
            L[i][j] = _div(s, d)
    if not ok:
        return None
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
    return x


def lambda_init(n, H):
    """computeLambdaInit: tau * max |H_jj|"""
    m, h = 0.0, 0
    for j in range(n):
        a = abs(float(H[h]))
        m = m if a < m else a
        h += n - j
    return 1e-5 * m


def levenberg(problem, iterations):
    """One optimize(iterations) call of g2o on one vertex -> the iterations run.  problem holds the estimate and a candidate for it and
    has: n, the unknowns; sums() -> the n (n + 1) / 2 values of H, the n of b (before the sign) and the robust chi2 at the estimate;
    candidate(x), which forms the candidate from the step x and may edit x (what it leaves there enters rho); chi() -> the robust
    chi2 at the candidate; accept(), the candidate becomes the estimate."""
    n = problem.n
    nh = n * (n + 1) // 2
    its = 0
    lam, ni, nbad = 0.0, 2.0, 0
    for it in range(iterations):
        acc = problem.sums()
        b = [-float(v) for v in acc[nh:nh + n]]
        chi = float(acc[nh + n])
        ini_chi = chi
        if it == 0:
            lam, ni, nbad = lambda_init(n, acc), 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            x = solve(n, acc, lam, b)
            if x is not None and not (math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) < THETA_MAX):
                x = None        # a rotation angle outside the range of the device's sin / cos: as a failed solve
            ok = x is not None
            temp_chi = DBL_MAX
            if ok:
                problem.candidate(x)
                temp_chi = problem.chi()
            else:
                x = [0.0] * n
            scale = 0.0
            for j in range(n):
                scale = scale + x[j] * (lam * x[j] + b[j])
            scale = scale + 1e-3
            rho = _div(chi - temp_chi, scale)
            if rho > 0 and math.isfinite(temp_chi):
                t = 2.0 * rho - 1.0
                alpha = 1.0 - (t * t) * t
                alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
                lam = lam * (alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0))
                ni, chi = 2.0, temp_chi
                if ok:
                    problem.accept()
            else:
                lam = lam * ni
                ni = ni * 2.0
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        its += 1
        if qmax == 10 or rho == 0:
            break
        nbad = nbad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
        if nbad >= 3:
            break
    return its
