"""The restatement of Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:37-237 over the reference's g2o) in Python
floats, and the seeded scenes of tests/test_global_ba_cpu.py / test_global_ba_gpu.py and tools/bench_global_ba.py.

It builds on tests/ba_cases.py (the edges, the quadratic form, the Schur complement landmark by landmark, the dense LDLt) and
differs from local_ba where the reference does: ONE optimize(iterations) call, no levels and no erase pass; the Huber deltas are this
function's own, (float)sqrt(5.99) for a monocular edge (:85, not LocalBundleAdjustment's (float)sqrt(5.991)) and (float)sqrt(7.815)
for a stereo edge; `robust` switches the kernel on every edge; EVERY keyframe row comes back as toCvMat of its SE3Quat, the fixed
ones too (:193-210); not_included is vbNotIncludedMP (:175-183) and a point without an edge keeps its row.  It shares no text with
psl-slam_amd/csrc/gba_kernels.h.  Parity with g2o itself is unpinned."""
import functools
import math
import struct

import numpy as np

import ba_cases as bc
from ba_cases import E_CAPACITY, E_INVALID, EDGE_DTYPE, KF_DTYPE, MP_DTYPE, _Problem, _quad, _solve, _sqrt, _sum256, _tri
from lm_cases import DBL_MAX, _div
from pose_opt_cases import DELTA_STEREO, _pose_rec, _quat_to_R, _rodrigues, camera, from_pose, se3_exp, se3_mul, to_pose

INFO_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("free_keyframes", "<i4"), ("included_points", "<i4"), ("chi2_start", "<f8"),
                       ("chi2_end", "<f8"), ("lambda", "<f8")])
assert INFO_DTYPE.itemsize == 40
DELTA_MONO_GBA = float(np.float32(math.sqrt(5.99)))      # const float thHuber2D = sqrt(5.99)  (src/Optimizer.cc:85)
assert DELTA_MONO_GBA == 2.4474475383758545 and DELTA_MONO_GBA != bc.DELTA_MONO


class _GbaProblem(_Problem):
    def huber(self, e, c):
        d = DELTA_MONO_GBA if self.mono[e] else DELTA_STEREO
        dsqr = d * d
        if c <= dsqr:
            return c, 1.0
        sq = _sqrt(c)
        return (2.0 * sq) * d - dsqr, _div(d, sq)


def global_ba(kfs, mps, edges, cam, iterations=5, robust=1, caps=None):
    """-> dict(info INFO_DTYPE record, kf KF_DTYPE[nkf], mp MP_DTYPE[nmp], not_included u8 [nmp], trials [(iteration, ok, why, rho,
    lambda)], stopped)"""
    P = _GbaProblem(kfs, mps, edges, cam)
    info = np.zeros((), INFO_DTYPE)
    res = {"info": info, "kf": P.kf.copy(), "mp": P.mp.copy(), "not_included": np.zeros(P.nmp, np.uint8), "trials": [], "stopped": "iterations"}
    if caps is not None and (P.nkf > caps[0] or P.nmp > caps[1] or P.ne > caps[2]):
        info["status"] = E_CAPACITY
        return res
    pairs = set()
    for e in range(P.ne):
        if not (0 <= P.e_kf[e] < P.nkf and 0 <= P.e_pt[e] < P.nmp):
            info["status"] = E_INVALID
            return res
    for e in range(P.ne):
        if (P.e_pt[e], P.e_kf[e]) in pairs:
            info["status"] = E_INVALID
            return res
        pairs.add((P.e_pt[e], P.e_kf[e]))

    T = [from_pose(P.kf["Tcw"][k]) for k in range(P.nkf)]
    X = [[float(P.mp[k][p]) for k in ("x", "y", "z")] for p in range(P.nmp)]
    level = [False] * P.ne
    err = [[0.0, 0.0, 0.0] for _ in range(P.ne)]
    rho0 = [0.0] * P.ne
    in_sys = [not P.fixed[k] and bool(P.kf_edges[k]) for k in range(P.nkf)]
    pact = [bool(P.pt_edges[p]) for p in range(P.nmp)]
    kfof = [k for k in range(P.nkf) if in_sys[k]]
    pidx = {k: i for i, k in enumerate(kfof)}
    F = len(kfof)
    N = 6 * F

    def evaluate(Tx, Xx, linearize):
        rows = {}
        for e in range(P.ne):
            Pc = P.camera_point(e, Tx, Xx)
            er = P.error(e, Pc)
            c = P.chi2(e, er)
            r0, r1 = P.huber(e, c) if robust else (c, 1.0)
            err[e], rho0[e] = er, r0
            if linearize:
                Jp, Jl = P.jacobians(e, Pc, _quat_to_R(Tx[P.e_kf[e]][0]))
                rows[e] = (Jp, Jl, r1 * P.is2[e])
        return rows

    chi_active = lambda: _sum256(rho0, [True] * P.ne)
    first = last = 0.0
    lam, ni, nbad, its = 0.0, 2.0, 0, 0
    with np.errstate(all="ignore"):
        for it in range(iterations if F and P.ne else 0):
            rows = evaluate(T, X, True)
            chi = chi_active()
            ini_chi = chi
            if it == 0:
                first = chi
            Hpp, bp = [[0.0] * 21 for _ in range(F)], [0.0] * N
            for i, k in enumerate(kfof):
                acc = [0.0] * 27
                for e in P.kf_edges[k]:
                    acc = [a + b for a, b in zip(acc, _quad(rows[e][0], 6, rows[e][2], P.mono[e], err[e]))]
                Hpp[i] = acc[:21]
                bp[6 * i:6 * i + 6] = [-a for a in acc[21:]]
            Hll, bl = [[0.0] * 6 for _ in range(P.nmp)], [[0.0] * 3 for _ in range(P.nmp)]
            for p in range(P.nmp):
                if pact[p]:
                    acc = [0.0] * 9
                    for e in P.pt_edges[p]:
                        acc = [a + b for a, b in zip(acc, _quad(rows[e][1], 3, rows[e][2], P.mono[e], err[e]))]
                    Hll[p], bl[p] = acc[:6], [-a for a in acc[6:]]
            B = {}
            for e, (Jp, Jl, w) in rows.items():
                if P.e_kf[e] in pidx:
                    blk = [[0.0] * 3 for _ in range(6)]
                    for rr in range(6):
                        w0, w1, w2 = w * Jp[0][rr], w * Jp[1][rr], w * Jp[2][rr]
                        for m in range(3):
                            s = w0 * Jl[0][m] + w1 * Jl[1][m]
                            blk[rr][m] = s if P.mono[e] else s + w2 * Jl[2][m]
                    B[e] = blk
            if it == 0:
                m = 0.0
                for i in range(F):
                    for j in range(6):
                        a = abs(Hpp[i][_tri(6, j, j)])
                        m = m if a < m else a
                for p in range(P.nmp):
                    if pact[p]:
                        for j in range(3):
                            a = abs(Hll[p][_tri(3, j, j)])
                            m = m if a < m else a
                lam, ni, nbad = 1e-5 * m, 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                step, why = _solve(P, F, kfof, pidx, pact, level, Hpp, bp, Hll, bl, B, lam)
                temp_chi, scale = DBL_MAX, 0.0
                if step is not None:
                    xp, xl = step
                    Tn, Xn = list(T), [list(x) for x in X]
                    for i, k in enumerate(kfof):
                        Tn[k] = se3_mul(se3_exp(xp[6 * i:6 * i + 6]), T[k])
                    for p in range(P.nmp):
                        if pact[p]:
                            Xn[p] = [X[p][j] + xl[p][j] for j in range(3)]
                    evaluate(Tn, Xn, False)
                    temp_chi = chi_active()
                    for j in range(N):
                        scale = scale + xp[j] * (lam * xp[j] + bp[j])
                    for p in range(P.nmp):
                        if pact[p]:
                            for j in range(3):
                                scale = scale + xl[p][j] * (lam * xl[p][j] + bl[p][j])
                scale = scale + 1e-3
                rho = _div(chi - temp_chi, scale)
                res["trials"].append((it, step is not None, why, rho, lam))
                if rho > 0 and abs(temp_chi) <= DBL_MAX:
                    t = 2.0 * rho - 1.0
                    alpha = 1.0 - (t * t) * t
                    alpha = (2.0 / 3.0) if (2.0 / 3.0) < alpha else alpha
                    lam = lam * (alpha if (1.0 / 3.0) < alpha else (1.0 / 3.0))
                    ni, chi = 2.0, temp_chi
                    if step is not None:
                        T, X = Tn, Xn
                else:
                    lam = lam * ni
                    ni = ni * 2.0
                qmax += 1
                if not (rho < 0 and qmax < 10):
                    break
            its += 1
            last = chi
            if qmax == 10 or rho == 0:
                res["stopped"] = "terminate"
                break
            nbad = nbad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
            if nbad >= 3:
                res["stopped"] = "nbad"
                break
    for k in range(P.nkf):                      # SetPose / mTcwGBA of every keyframe: the fixed one goes through the quaternion too
        res["kf"]["Tcw"][k] = to_pose(T[k])
    for p in range(P.nmp):
        res["not_included"][p] = 0 if pact[p] else 1
        if pact[p]:
            for j, nm in enumerate(("x", "y", "z")):
                res["mp"][nm][p] = np.float64(X[p][j]).astype(np.float32)
    info["iterations"], info["free_keyframes"], info["included_points"] = its, F, sum(pact)
    info["chi2_start"], info["chi2_end"], info["lambda"] = first, last, lam
    return res


# ---- the scenes --------------------------------------------------------------------------------------------------------------------------
def make_window_scene(seed, nkf, npts, kind="mixed", window=4, noise=True, nfixed=1, rot_deg=0.5, dt=0.02, dpt=0.03):
    """A camera that moves along x past a band of points; every point is seen by `window` consecutive keyframes, so most keyframe
    pairs share no point and S is banded.  The first `nfixed` keyframes are fixed (mnId == 0).  Edges per point, its keyframes in a
    seeded order.  Vectorised: tools/bench_global_ba.py builds maps of 10^5 points with it.  -> dict(kf, mp, edges, cam)"""
    rng = np.random.default_rng(seed)
    cam = camera()
    fx, fy, cx, cy, bf = (float(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf"))
    window = min(window, nkf)
    step = 0.3
    kf_true = np.zeros(nkf, KF_DTYPE)
    Rs, ts = np.zeros((nkf, 3, 3)), np.zeros((nkf, 3))
    for k in range(nkf):
        R = _rodrigues(np.array([0.0, 0.05 * math.sin(0.7 * k), 0.0]))
        pos = np.array([step * k, 0.02 * math.cos(1.3 * k), 0.0])
        Rs[k], ts[k] = R, -R @ pos
        kf_true["Tcw"][k] = _pose_rec(R, ts[k])
        kf_true["fixed"][k] = 1 if k < nfixed else 0
    Rs, ts = kf_true["Tcw"]["R"].astype(np.float64).reshape(nkf, 3, 3), kf_true["Tcw"]["t"].astype(np.float64)
    xs = rng.uniform(0.0, step * max(nkf - 1, 1), npts)
    xs[:min(npts, nkf)] = step * np.arange(min(npts, nkf))      # every keyframe sees a point
    Xw = np.stack([xs, rng.uniform(-1.0, 1.0, npts), rng.uniform(4.0, 8.0, npts)], 1).astype(np.float32)
    mp_true = np.zeros(npts, MP_DTYPE)
    mp_true["x"], mp_true["y"], mp_true["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    mp_true["min_dist"], mp_true["max_dist"], mp_true["nz"] = 0.5, 20.0, -1.0
    start = np.clip(np.rint(xs / step).astype(np.int64) - window // 2, 0, nkf - window)
    order = np.argsort(rng.random((npts, window)), axis=1)
    ekf = (start[:, None] + order).reshape(-1)
    ept = np.repeat(np.arange(npts), window)
    ne = len(ekf)
    Pc = np.einsum("eij,ej->ei", Rs[ekf], Xw[ept].astype(np.float64)) + ts[ekf]
    u, v = Pc[:, 0] / Pc[:, 2] * fx + cx, Pc[:, 1] / Pc[:, 2] * fy + cy
    ur = u - bf / Pc[:, 2]
    scale = (np.float32(1.2) ** rng.integers(0, 4, ne).astype(np.float32)).astype(np.float64)
    if noise:
        u, v, ur = (a + rng.normal(size=ne) * bc.NOISE_PX * scale for a in (u, v, ur))
    stereo = np.ones(ne, bool) if kind == "stereo" else np.zeros(ne, bool) if kind == "mono" else rng.random(ne) < 0.5
    e = np.zeros(ne, EDGE_DTYPE)
    e["point"], e["kf"], e["u"], e["v"] = ept, ekf, u, v
    e["ur"] = np.where(stereo, ur, -1.0)
    e["inv_sigma2"] = np.float32(1.0) / (scale * scale).astype(np.float32)
    kf = kf_true.copy()
    for k in range(nfixed, nkf):
        ax = rng.normal(size=3)
        dR = _rodrigues(ax / np.linalg.norm(ax) * math.radians(rot_deg))
        kf["Tcw"][k] = _pose_rec(dR @ Rs[k], dR @ ts[k] + rng.normal(size=3) * dt)
    mp = mp_true.copy()
    d = (rng.normal(size=(npts, 3)) * dpt).astype(np.float32)
    mp["x"], mp["y"], mp["z"] = mp["x"] + d[:, 0], mp["y"] + d[:, 1], mp["z"] + d[:, 2]
    return {"kf": kf, "mp": mp, "edges": e, "cam": cam, "kf_true": kf_true, "mp_true": mp_true}


def _global_rows(c):
    """a local-BA scene as the global BA sees it: same rows"""
    return {k: c[k] for k in ("kf", "mp", "edges", "cam")}


MODES = [(5, 1), (10, 0), (20, 1)]             # (iterations, robust): LocalBundleAdjustment's round one, the loop-closing call, the monocular start
LOCAL_NAMES = list(bc.CASE_NAMES)              # the shapes and edge cases of ba_cases, as rows
EXTRA_NAMES = ["no_fixed", "point_without_edge", "keyframe_without_edge"]
STEREO_ONLY = ["f2_x1_p8_stereo", "point_only_fixed", "stopped_by_nbad"]
# The widths of the whole-device solve (lm_grid.h) and the F on both sides of each, N = 6 F:
#   32 columns per LDLt panel                      F = 5 | 6 (N = 30 | 36); F = 1, 2 (N = 6, 12) lie inside one panel
#   64 rows per workgroup below a panel, and 64    F = 10 | 11 (N = 60 | 66); F = 16 (N = 96 = 32 + 64: exactly one full row tile)
#   128                                            F = 21 | 22 (N = 126 | 132)
#   256, and 256 rows per workgroup of the forward substitution: a second workgroup needs more than 256 rows below the first
#   panel, N > 288                                 F = 43 (N = 258), F = 48 | 49 (N = 288 | 294)
#   512 doubles per chunk of a chain of additions: the backward substitution's longest row has N - 1 products
#                                                  F = 85 | 86 (N = 510 | 516: 509 | 515 products, one chunk | two)
#   ... and computeScale's chain has 6 F + 3 P     chain_P126 | chain_P127 (F = 22: 510 | 513), restated; F = 85 | 86 have three chunks
# Python restates up to F = 22; F = 43 and above are compared with the one-core loop alone.
WINDOW_F = [1, 2, 5, 6, 10, 11, 16, 21, 22]
LOOP_ONLY_F = [43, 48, 49, 85, 86]
CHAIN_NAMES = ["chain_P126", "chain_P127"]
CAPS = (96, 384, 2048)                         # holds every scene here


def parity_cases():
    """[(scene name, iterations, robust)] that Python restates: every ba_cases row set and the three extra ones in all three modes; the
    windowed scenes at (5, robust), the small ones also at (10, plain); the dense scene at F = 22 and the two chain scenes at (5, robust)"""
    out = [(n, it, rb) for n in LOCAL_NAMES + EXTRA_NAMES for it, rb in MODES]
    out += [(f"window_F{F}", 5, 1) for F in WINDOW_F] + [(f"window_F{F}", 10, 0) for F in WINDOW_F if F <= 6]
    return out + [("dense_F22", 5, 1)] + [(n, 5, 1) for n in CHAIN_NAMES]


@functools.lru_cache(maxsize=None)
def scene(name):
    """name -> the rows (no reference): a ba_cases name; "window_F<F>"; "dense_F22"; "no_fixed"; "point_without_edge";
    "keyframe_without_edge" """
    if name in bc.CASE_NAMES:
        return _global_rows(bc.case(name))
    if name.startswith("window_F"):
        F = int(name[len("window_F"):])
        return make_window_scene(700 + F, F + 1, 3 * F + 2, "mixed")
    if name.startswith("chain_P"):              # 22 free keyframes and P points: computeScale adds 132 + 3 P terms
        return make_window_scene(740, 23, int(name[len("chain_P"):]), "mixed")
    if name == "dense_F22":
        return _global_rows(bc.make_scene(722, 22, 1, 30, "mixed", pobs=0.5))
    if name == "no_fixed":                      # no keyframe is fixed: the gauge is free, lambda holds the system
        c = make_window_scene(731, 4, 12, "stereo", nfixed=0)
        return c
    if name == "point_without_edge":            # vbNotIncludedMP: point 2 loses its edges and keeps its row
        c = dict(make_window_scene(732, 4, 12, "mixed"))
        c["edges"] = c["edges"][c["edges"]["point"] != 2]
        return c
    if name == "keyframe_without_edge":         # free keyframe 2 has no edge: no block, still round-tripped
        c = dict(make_window_scene(733, 5, 14, "mixed", window=5))
        c["edges"] = c["edges"][c["edges"]["kf"] != 2]
        return c
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def ref(name, iterations, robust):
    c = scene(name)
    return global_ba(c["kf"], c["mp"], c["edges"], c["cam"], iterations, robust)


def refused_cases(iterations, robust, caps):
    """[(rows, status)]: a duplicate pair, an edge outside the problem, a count above the caps, no free keyframe, no edge"""
    base = scene("f2_x1_p8_mixed")
    dup = dict(base, edges=np.concatenate([base["edges"], base["edges"][:1]]))
    outside = dict(base, edges=base["edges"].copy())
    outside["edges"]["point"][0] = -1
    big = make_window_scene(77, 3, caps[1] + 1, "mono")
    still = dict(base, kf=base["kf"].copy())
    still["kf"]["fixed"] = 1
    bare = dict(base, edges=base["edges"][:0])
    out = []
    for c, st in ((dup, E_INVALID), (outside, E_INVALID), (big, E_CAPACITY), (still, 0), (bare, 0)):
        c = dict(c, ref=global_ba(c["kf"], c["mp"], c["edges"], c["cam"], iterations, robust, caps=caps))
        assert int(c["ref"]["info"]["status"]) == st and int(c["ref"]["info"]["iterations"]) == 0
        out.append((c, st))
    return out


# ---- the files of tools/dropin/gba_main.cpp ---------------------------------------------------------------------------------------------
def write_cases(path, cases, iterations, robust, caps):
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", len(cases), iterations, robust, *caps))
        f.write(bc.camera_record(cases[0]["cam"] if cases else camera()).tobytes())
        for c in cases:
            f.write(struct.pack("<3i", len(c["kf"]), len(c["mp"]), len(c["edges"])))
            f.write(np.ascontiguousarray(c["kf"], KF_DTYPE).tobytes())
            f.write(np.ascontiguousarray(c["mp"], MP_DTYPE).tobytes())
            f.write(np.ascontiguousarray(c["edges"], EDGE_DTYPE).tobytes())


def read_sections(path, cases, nsections):
    """-> [section][case] dict(info, kf, mp, not_included)"""
    buf = open(path, "rb").read()
    at, out = 0, []
    for _ in range(nsections):
        sec = []
        for c in cases:
            r = {}
            for key, dt, n in (("info", INFO_DTYPE, 1), ("kf", KF_DTYPE, len(c["kf"])), ("mp", MP_DTYPE, len(c["mp"])), ("not_included", np.uint8, len(c["mp"]))):
                dt = np.dtype(dt)
                r[key] = np.frombuffer(buf, dt, n, at).copy()
                at += n * dt.itemsize
            r["info"] = r["info"][0]
            sec.append(r)
        out.append(sec)
    assert at == len(buf), (at, len(buf))
    return out


def assert_equal(got, want, what):
    """bit for bit: poses, points, not_included and every PslGbaInfo field (a NaN equals a NaN: its sign and payload are not part of
    the contract)"""
    gi, wi = got["info"], want["info"]
    for k in ("status", "iterations", "free_keyframes", "included_points"):
        assert int(gi[k]) == int(wi[k]), (what, k, gi, wi)
    for k in ("chi2_start", "chi2_end", "lambda"):
        assert np.float64(gi[k]).tobytes() == np.float64(wi[k]).tobytes() or (np.isnan(gi[k]) and np.isnan(wi[k])), (what, k, float(gi[k]), float(wi[k]))
    assert np.asarray(got["not_included"], np.uint8).tobytes() == np.asarray(want["not_included"], np.uint8).tobytes(), what
    assert np.ascontiguousarray(got["kf"], KF_DTYPE).tobytes() == np.ascontiguousarray(want["kf"], KF_DTYPE).tobytes(), what
    assert np.ascontiguousarray(got["mp"], MP_DTYPE).tobytes() == np.ascontiguousarray(want["mp"], MP_DTYPE).tobytes(), what
