"""The restatement of the point edges of Optimizer::PoseOptimization (src/Optimizer.cc:239-1023 over the reference's g2o) in numpy
float64, and the seeded cases of tests/test_pose_opt_cpu.py / test_pose_opt_gpu.py.

The restatement mirrors the arithmetic of psl-slam_amd/csrc/pose_kernels.h operation by operation (every numpy ufunc is one IEEE
operation; nothing here goes through BLAS) and its rounds psl_po_rounds decision by decision, with math.sin / math.cos; it shares no
text with the C++ and is what the kernel and the host loop are judged against.  levenberg_rounds is the one place where the rounds
are written here: it runs over a list of edge kinds (_Edges below; _Lil of tests/pose_lil_cases.py), each round is one call of
lm_cases.levenberg (the iterations and trials, shared with tests/sim3_opt_cases.py), and optimize() here and in pose_lil_cases are
calls of it.  order="device" sums H, b and the robust chi2 in the device's order (the
header of psl-slam_amd/csrc/pslfe_pose.hip); order="edge" sums them edge by edge, which is g2o's.
Eigen and g2o cannot be built offline: parity with g2o itself is unpinned."""
import functools
import math

import numpy as np

from lm_cases import levenberg, sum_device, sum_edge

EDGE_DTYPE = np.dtype([(k, "<f4") for k in ("u", "v", "ur", "inv_sigma2", "x", "y", "z")])
POSE_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,))])
INFO_DTYPE = np.dtype([("rounds", "<i4"), ("iterations", "<i4", (4,))])
DELTA_MONO = float(np.float32(math.sqrt(5.991)))      # const float deltaMono = sqrt(5.991)  (src/Optimizer.cc:274)
DELTA_STEREO = float(np.float32(math.sqrt(7.815)))
CHI2_MONO, CHI2_STEREO = np.float32(5.991), np.float32(7.815)


# ---- SE3Quat (se3quat.h) on Python floats: q = [x, y, z, w] ---------------------------------------------------------------------------
def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _normalize(q):
    if q[3] < 0:
        q = [-q[0], -q[1], -q[2], -q[3]]
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [q[0] / n, q[1] / n, q[2] / n, q[3] / n]


def _quat_from_R(R):
    t = (R[0] + R[4]) + R[8]
    q = [0.0] * 4
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t
    else:
        i = 0
        if R[4] > R[0]:
            i = 1
        if R[8] > R[4 * i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[3 * k + j] - R[3 * j + k]) * t
        q[j] = (R[3 * j + i] + R[3 * i + j]) * t
        q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def _quat_to_R(q):
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def _rotate(q, v):
    """q * v for a vector of Python floats or of numpy columns."""
    uv = _cross(q, v)
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    c = _cross(q, uv)
    return [(v[0] + q[3] * uv[0]) + c[0], (v[1] + q[3] * uv[1]) + c[1], (v[2] + q[3] * uv[2]) + c[2]]


def from_pose(pose):
    """Converter::toSE3Quat: (q, t)."""
    R = [float(v) for v in np.asarray(pose["R"], np.float32).reshape(9)]
    t = [float(v) for v in np.asarray(pose["t"], np.float32).reshape(3)]
    return _normalize(_quat_from_R(R)), t


def to_pose(T):
    """Converter::toCvMat."""
    p = np.zeros((), POSE_DTYPE)
    p["R"] = np.array(_quat_to_R(T[0]), np.float64).astype(np.float32)
    p["t"] = np.array(T[1], np.float64).astype(np.float32)
    return p


def _mat3mul(A, B):
    return [(A[3 * i] * B[k] + A[3 * i + 1] * B[3 + k]) + A[3 * i + 2] * B[6 + k] for i in range(3) for k in range(3)]


def se3_exp(x):
    theta = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    O = [0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0]
    O2 = _mat3mul(O, O)
    eye = [1.0 if i % 4 == 0 else 0.0 for i in range(9)]
    if theta < 0.00001:
        R = [(eye[i] + O[i]) + O2[i] for i in range(9)]
        V = R
    else:
        s, c = math.sin(theta), math.cos(theta)
        th2 = theta * theta
        a, b, g = s / theta, (1.0 - c) / th2, (theta - s) / (th2 * theta)
        R = [(eye[i] + a * O[i]) + b * O2[i] for i in range(9)]
        V = [(eye[i] + b * O[i]) + g * O2[i] for i in range(9)]
    q = _normalize(_quat_from_R(R))
    t = [(V[3 * i] * x[3] + V[3 * i + 1] * x[4]) + V[3 * i + 2] * x[5] for i in range(3)]
    return q, t


def se3_mul(A, B):
    r = _rotate(A[0], B[1])
    a, b = A[0], B[0]
    q = [((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1],
         ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2],
         ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0],
         ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]]
    return _normalize(q), [A[1][0] + r[0], A[1][1] + r[1], A[1][2] + r[2]]


# ---- the edges, vectorised over the edge index ------------------------------------------------------------------------------------------
class _Edges:
    def __init__(self, edges, cam):
        e = np.ascontiguousarray(edges, EDGE_DTYPE)
        self.n = len(e)
        self.u, self.v, self.ur = (e[k].astype(np.float64) for k in ("u", "v", "ur"))
        self.is2 = e["inv_sigma2"].astype(np.float64)
        self.X = [e[k].astype(np.float64) for k in ("x", "y", "z")]
        self.mono = e["ur"] < np.float32(0)
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(np.float32(cam[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
        self.delta = np.where(self.mono, DELTA_MONO, DELTA_STEREO)
        self.thr = np.where(self.mono, CHI2_MONO, CHI2_STEREO)

    # an edge kind of levenberg_rounds: one addition per edge; an outlier lowers the return value
    steps, counted = 1, True
    count = property(lambda self: self.n)

    def chi(self, T):
        ev = self.error(T)
        return ev, self.chi2(ev[0])

    def additions(self, ev, T, rho0, rho1):
        return self.terms(ev[0], ev[1], rho0, rho1)[:, None]

    def error(self, T):
        """computeError of every edge: e [3][n] (e[2] = 0 for a monocular edge), Pc [3][n]."""
        r = _rotate(T[0], self.X)
        Pc = [r[0] + T[1][0], r[1] + T[1][1], r[2] + T[1][2]]
        m0 = self.u - ((Pc[0] / Pc[2]) * self.fx + self.cx)
        m1 = self.v - ((Pc[1] / Pc[2]) * self.fy + self.cy)
        invz = (1.0 / Pc[2]).astype(np.float32).astype(np.float64)     # const float invz (types_six_dof_expmap.cpp:300)
        r0 = (Pc[0] * invz) * self.fx + self.cx
        s0 = self.u - r0
        s1 = self.v - ((Pc[1] * invz) * self.fy + self.cy)
        s2 = self.ur - (r0 - self.bf * invz)
        return [np.where(self.mono, m0, s0), np.where(self.mono, m1, s1), np.where(self.mono, 0.0, s2)], Pc

    def chi2(self, e):
        c = e[0] * (self.is2 * e[0]) + e[1] * (self.is2 * e[1])
        return np.where(self.mono, c, c + e[2] * (self.is2 * e[2]))

    def huber(self, c):
        dsqr = self.delta * self.delta
        sq = np.sqrt(c)
        inl = c <= dsqr
        return np.where(inl, c, (2.0 * sq) * self.delta - dsqr), np.where(inl, 1.0, self.delta / sq)

    def terms(self, e, Pc, rho0, rho1):
        """The 28 terms of every edge: [n][28]."""
        x, y = Pc[0], Pc[1]
        invz = 1.0 / Pc[2]
        invz2 = invz * invz
        fx, fy, bf = self.fx, self.fy, self.bf
        zero = np.zeros(self.n)
        J0 = [((x * y) * invz2) * fx, (-(1.0 + (x * x) * invz2)) * fx, (y * invz) * fx, (-invz) * fx, zero, (x * invz2) * fx]
        J1 = [(1.0 + (y * y) * invz2) * fy, (((-x) * y) * invz2) * fy, ((-x) * invz) * fy, zero, (-invz) * fy, (y * invz2) * fy]
        J2 = [J0[0] - (bf * y) * invz2, J0[1] + (bf * x) * invz2, J0[2], J0[3], zero, J0[5] - bf * invz2]
        w = rho1 * self.is2
        out = np.zeros((self.n, 28))
        h = 0
        for j in range(6):
            w0, w1, w2 = w * J0[j], w * J1[j], w * J2[j]
            for k in range(j, 6):
                s = w0 * J0[k] + w1 * J1[k]
                out[:, h] = np.where(self.mono, s, s + w2 * J2[k])
                h += 1
            s = w0 * e[0] + w1 * e[1]
            out[:, 21 + j] = np.where(self.mono, s, s + w2 * e[2])
        out[:, 27] = rho0
        return out


def levenberg_rounds(Tcw, kinds, order="device"):
    """The four rounds of PoseOptimization, each one lm_cases.levenberg(problem, 10), over a list of edge kinds, which share one edge
    index space in list order.  A kind has: count; steps, the additions one of its edges makes to a sum; counted, whether its outliers
    lower the return value; thr, the float32 thresholds of its classification; chi(T) -> (what it evaluated at T, chi2 [count]);
    huber(chi2) -> (rho, rho'); additions(evaluated, T, rho, rho') -> [count][steps][28].
    -> (pose_out POSE_DTYPE record, [outlier u8 [count] of each kind] or None when nothing is written, ngood, info INFO_DTYPE record,
    margin): margin = the least relative distance |chi2 - threshold| / threshold of a classification, over every round."""
    info = np.zeros((), INFO_DTYPE)
    Tcw = np.ascontiguousarray(Tcw, POSE_DTYPE).reshape(())
    nt = sum(k.count for k in kinds)
    if nt < 3:
        return Tcw.copy(), None, 0, info, math.inf
    steps = np.concatenate([np.full(k.count, k.steps) for k in kinds])
    bounds = np.cumsum([0] + [k.count for k in kinds])

    def red(parts):
        """[count][<= steps][w] of each kind, the additions of its edges -> the w sums over the active edges in the chosen order"""
        seq = np.zeros((nt, max(k.steps for k in kinds), parts[0].shape[2]))
        for k, p, i0 in zip(kinds, parts, bounds):
            seq[i0:i0 + k.count, :p.shape[1]] = p
        return sum_device(seq, active) if order == "device" else sum_edge(seq, active, steps)

    def system(Tx, robust):
        parts = []
        for k in kinds:
            ev, c = k.chi(Tx)
            rho0, rho1 = k.huber(c) if robust else (c, np.ones(k.count))
            parts.append(k.additions(ev, Tx, rho0, rho1))
        return red(parts)

    def chi_of(Tx, robust):
        parts = []
        for k in kinds:
            c = k.chi(Tx)[1]
            parts.append((k.huber(c)[0] if robust else c)[:, None, None])
        return float(red(parts)[0])

    class Problem:
        """the SE3 vertex and the sums of a round: the `problem` of lm_cases.levenberg"""
        n = 6

        def sums(self):
            return system(self.T, robust)

        def candidate(self, x):
            self.Tn = se3_mul(se3_exp(x), self.T)

        def chi(self):
            return chi_of(self.Tn, robust)

        def accept(self):
            self.T = self.Tn

    T0 = from_pose(Tcw)
    outlier = [np.zeros(k.count, bool) for k in kinds]
    nbad, margin, P = [0] * len(kinds), math.inf, Problem()
    with np.errstate(all="ignore"):
        for r in range(4):
            P.T = T0
            robust = r < 3
            active = np.concatenate([~o for o in outlier])
            its = levenberg(P, 10) if nt - sum(nbad) > 0 else 0
            T = P.T
            for i, k in enumerate(kinds):
                c = k.chi(T)[1]
                outlier[i] = c.astype(np.float32) > k.thr
                if k.count:
                    margin = min(margin, float(np.nanmin(np.abs(c - k.thr.astype(np.float64)) / k.thr)))
                nbad[i] = int(outlier[i].sum())
            info["rounds"] = r + 1
            info["iterations"][r] = its
            if nt < 10:
                break
    ngood = nt - sum(b for k, b in zip(kinds, nbad) if k.counted)     # nInitialCorrespondences - nBad (src/Optimizer.cc:1022)
    return to_pose(T), [o.astype(np.uint8) for o in outlier], ngood, info, margin


def optimize(Tcw, edges, cam, order="device"):
    """The point edges alone -> (pose_out, outlier u8 [n] or None when nothing is written, ngood, info, margin)"""
    pose, flags, ngood, info, margin = levenberg_rounds(Tcw, [_Edges(edges, cam)], order)
    return pose, None if flags is None else flags[0], ngood, info, margin


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
def camera():
    """fx = fy = 500, cx = 320, cy = 240, bf = 40 (a dict of float32)."""
    return {k: np.float32(v) for k, v in (("fx", 500.0), ("fy", 500.0), ("cx", 320.0), ("cy", 240.0), ("bf", 40.0))}


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def _pose_rec(R, t):
    p = np.zeros((), POSE_DTYPE)
    p["R"], p["t"] = np.asarray(R, np.float64).reshape(9).astype(np.float32), np.asarray(t, np.float64).astype(np.float32)
    return p


def make_case(seed, n, kind, outliers, noise=True, behind=False):
    """-> dict(Tcw start pose, Ttrue, edges, planted u8 [n]).  kind: "mono" | "stereo" | "mixed"."""
    rng = np.random.default_rng(seed)
    cam = camera()
    fx, fy, cx, cy, bf = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    Rt = _rodrigues(rng.normal(size=3) * 0.3)
    tt = rng.normal(size=3) * 0.5
    Ttrue = _pose_rec(Rt, tt)
    Rt, tt = Ttrue["R"].astype(np.float64).reshape(3, 3), Ttrue["t"].astype(np.float64)    # the true pose is the float one
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    dR = _rodrigues(ax * math.radians(2.0))
    dt = rng.normal(size=3)
    dt *= 0.05 / np.linalg.norm(dt)
    Tcw = _pose_rec(dR @ Rt, dR @ tt + dt)             # the true pose moved by 2 degrees and 5 cm
    z = rng.uniform(1.0, 8.0, n)
    u = rng.uniform(20.0, 620.0, n)
    v = rng.uniform(20.0, 460.0, n)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((Pc - tt) @ Rt).astype(np.float32)           # Rt^T (Pc - t), held as float as a map point is
    Pc = Xw.astype(np.float64) @ Rt.T + tt
    pu, pv = Pc[:, 0] / Pc[:, 2] * fx + cx, Pc[:, 1] / Pc[:, 2] * fy + cy
    pr = pu - bf / Pc[:, 2]
    octave = rng.integers(0, 8, n)
    scale = np.float32(1.2) ** octave.astype(np.float32)
    if noise:
        s = 0.5 * scale.astype(np.float64)
        pu, pv, pr = pu + rng.normal(size=n) * s, pv + rng.normal(size=n) * s, pr + rng.normal(size=n) * s
    planted = np.zeros(n, np.uint8)
    k = int(round(outliers * n))
    if k:
        idx = rng.choice(n, k, replace=False)
        ang = rng.uniform(0, 2 * math.pi, k)
        mag = rng.uniform(20.0, 60.0, k)
        pu[idx] += mag * np.cos(ang)
        pv[idx] += mag * np.sin(ang)
        planted[idx] = 1
    e = np.zeros(n, EDGE_DTYPE)
    e["u"], e["v"], e["ur"] = pu, pv, pr
    if kind == "mono":
        e["ur"] = -1
    elif kind == "mixed":
        e["ur"][rng.random(n) < 0.5] = -1
    e["inv_sigma2"] = np.float32(1.0) / (scale * scale)
    e["x"], e["y"], e["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    if behind:     # the last point 2 m BEHIND the camera of the start pose; its observation stays
        Rs, ts = Tcw["R"].astype(np.float64).reshape(3, 3), Tcw["t"].astype(np.float64)
        xb = (Rs.T @ (np.array([0.3, -0.2, -2.0]) - ts)).astype(np.float32)
        e["x"][-1], e["y"][-1], e["z"][-1] = xb
        planted[-1] = 1
    return {"Tcw": Tcw, "Ttrue": Ttrue, "edges": e, "planted": planted, "cam": cam}


def exact_case(n=40):
    """Data that are exact at the start pose (identity; depths that are powers of two, pixel offsets that are dyadic): chi2 = 0,
    b = 0, the step is 0, so rho == 0 ends the first iteration of every round."""
    e = np.zeros(n, EDGE_DTYPE)
    i = np.arange(n)
    z = np.float32(2.0) ** (1 + i % 3).astype(np.float32)
    ku, kv = (i * 7) % 33 - 16, (i * 5) % 25 - 12
    e["x"], e["y"], e["z"] = ku * z / 64, kv * z / 64, z
    e["u"], e["v"] = ku * (500.0 / 64) + 320.0, kv * (500.0 / 64) + 240.0
    e["ur"] = np.where(i % 2 == 0, e["u"] - np.float32(40.0) / z, np.float32(-1))
    e["inv_sigma2"] = 1.0
    T = _pose_rec(np.eye(3), np.zeros(3))
    return {"Tcw": T, "Ttrue": T, "edges": e, "planted": np.zeros(n, np.uint8), "cam": camera()}


# name -> (n, kind, outlier share, behind)
CASE_SPECS = {}
for _n in (2, 3, 9, 10, 63, 64, 65, 257, 2048):
    for _kind, _out in ((("mixed", 0.0),) if _n < 9 else (("mono", 0.0), ("stereo", 0.3), ("mixed", 0.3)) if _n < 2048 else
                        (("mono", 0.3), ("stereo", 0.0), ("mixed", 0.3), ("mixed", 0.0))):
        CASE_SPECS[f"n{_n}_{_kind}_{int(_out * 100)}"] = (_n, _kind, _out, False)
CASE_SPECS["n65_mixed_0_behind"] = (65, "mixed", 0.0, True)
CASE_SPECS["n300_mono_0_noisefree"] = (300, "mono", 0.0, False)
CASE_SPECS["n2100_mixed_30"] = (2100, "mixed", 0.3, False)      # more edges than the kernel keeps in LDS: the rows are read from HBM
# every kind with and without outliers at 3 (the smallest frame that is optimised), 64, 65 and 257, and every kind at 2 (a seed
# follows from a case's position in this table, so new cases go to its end)
for _n in (2, 3, 64, 65, 257):
    for _kind in ("mono", "stereo", "mixed"):
        for _out in ((0.0,) if _n == 2 else (0.0, 0.3)):
            CASE_SPECS.setdefault(f"n{_n}_{_kind}_{int(_out * 100)}", (_n, _kind, _out, False))
CASE_NAMES = list(CASE_SPECS) + ["exact", "huge"]
MARGIN = 1e-6


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its two references: dict(..., ref={"device": (pose, outlier, ngood, info), "edge": ...}).  A seed for which, in
    either order, a classification chi2 lies within a relative MARGIN of its threshold is rejected: the next seed is taken."""
    if name == "exact":
        c = exact_case()
        c["ref"] = {o: optimize(c["Tcw"], c["edges"], c["cam"], o)[:4] for o in ("device", "edge")}
        return c
    if name == "huge":     # non-physical data: one map point at 1e18 m
        c = make_case(77, 20, "mixed", 0.0)
        c["edges"]["x"][3] = 1e18
        c["ref"] = {o: optimize(c["Tcw"], c["edges"], c["cam"], o)[:4] for o in ("device", "edge")}
        return c
    n, kind, out, behind = CASE_SPECS[name]
    base = 1000 * (list(CASE_SPECS).index(name) + 1)
    for seed in range(base, base + 50):
        c = make_case(seed, n, kind, out, noise="noisefree" not in name, behind=behind)
        res = {o: optimize(c["Tcw"], c["edges"], c["cam"], o) for o in ("device", "edge")}
        if all(r[4] > MARGIN for r in res.values()):
            c["seed"] = seed
            c["ref"] = {o: r[:4] for o, r in res.items()}
            return c
    raise AssertionError(f"no seed for {name}")


def pose_floats(p):
    return np.concatenate([np.asarray(p["R"], np.float32).reshape(9), np.asarray(p["t"], np.float32).reshape(3)])


def order_difference():
    """The largest difference of a pose float between the two orders of the restatement over every case."""
    return max(float(np.abs(pose_floats(case(nm)["ref"]["device"][0]).astype(np.float64)
                            - pose_floats(case(nm)["ref"]["edge"][0]).astype(np.float64)).max()) for nm in CASE_NAMES)
