"""CPU checks of the map-line projection entry points (include/pslfe.h: pslfe_line_project_frustum[_device],
pslfe_line_project_last[_device], pslfe_line_search_by_projection_device, pslfe_glue_lines3d_device): the restatement the GPU tests
compare with (oracle/line_project_oracle.cpp) against a literal Python transcription of Frame::isInFrustum(MapLine*), the log of
MapLine::PredictScale swept over every float ratio the gates admit, the POD layouts, and the argument checks, which need no GPU."""
import ctypes as C
import math

import numpy as np

import oracle_lib

TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0, 0, 0, 0, 0, 40.0)
BOUNDS = (0.0, 0.0, 640.0, 480.0)
F32 = np.float32


def camera():
    import psl_slam_amd as P
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, TUM1):
        cam[k] = F32(v)
    return cam


def is_in_frustum(G, T, cam, bounds, limit, lsf):
    """src/Frame.cc:828-904 transcribed with numpy float32 / Python double arithmetic under the conventions of include/pslfe.h.
    -> None or (u1, v1, u2, v2, viewCos, level)."""
    R, t = T["R"].reshape(3, 3), T["t"]

    def cam_of(X):
        return [F32(float(R[r, 0]) * float(X[0]) + float(R[r, 1]) * float(X[1]) + float(R[r, 2]) * float(X[2]) + float(t[r])) for r in range(3)]
    SP, EP = [F32(v) for v in G["sp"]], [F32(v) for v in G["ep"]]
    Ow = [-F32(float(R[0, r]) * float(t[0]) + float(R[1, r]) * float(t[1]) + float(R[2, r]) * float(t[2])) for r in range(3)]
    S, E = cam_of(SP), cam_of(EP)
    if S[2] < 0 or E[2] < 0:
        return None
    if not (S[2] > 0 and E[2] > 0):                 # z == 0 or NaN: not in view
        return None
    fx, fy, cx, cy = F32(cam["fx"]), F32(cam["fy"]), F32(cam["cx"]), F32(cam["cy"])
    b = [F32(v) for v in bounds]
    with np.errstate(all="ignore"):
        i1 = F32(1) / S[2]
        u1, v1 = fx * S[0] * i1 + cx, fy * S[1] * i1 + cy
        if not (b[0] <= u1 <= b[2]) or not (b[1] <= v1 <= b[3]):
            return None
        i2 = F32(1) / E[2]
        u2, v2 = fx * E[0] * i2 + cx, fy * E[1] * i2 + cy
        if not (b[0] <= u2 <= b[2]) or not (b[1] <= v2 <= b[3]):
            return None
        mx, mn = F32(1.2) * F32(G["max_dist"]), F32(0.8) * F32(G["min_dist"])
        OM = [(F32(0.5) * SP[k] + F32(0.5) * EP[k]) - Ow[k] for k in range(3)]
        dist = F32(math.sqrt(sum(float(o) * float(o) for o in OM)))
        if not (mn <= dist <= mx):
            return None
        pn = [F32(v) for v in G["normal"]]
        dot = float(OM[0]) * float(pn[0]) + float(OM[1]) * float(pn[1]) + float(OM[2]) * float(pn[2])
        vc = F32(dot / float(dist)) if dist != 0 else F32("nan")
        if not (vc >= F32(limit)):
            return None
        ratio = F32(G["max_dist"]) / dist
        lf = F32(math.log(float(ratio)))
        level = int(math.ceil(lf / F32(lsf)))
    return (u1, v1, u2, v2, vc, level)


def random_lines(rng, T, n):
    """Map lines around the camera of pose T: mostly in front, some behind, beside, far, with odd distances and normals."""
    import psl_slam_amd as P
    Rw = T["R"].reshape(3, 3).astype(np.float64).T
    cw = -Rw @ T["t"].astype(np.float64)
    G = np.zeros(n, P.MAPLINE_DTYPE)
    for j in range(n):
        z = rng.uniform(-1.0, 6.0)
        a = np.array([rng.uniform(-3, 3) * max(z, 0.2), rng.uniform(-2, 2) * max(z, 0.2), z])
        d = rng.normal(0, 0.5, 3)
        G[j]["sp"], G[j]["ep"] = Rw @ a + cw, Rw @ (a + d) + cw
        m = 0.5 * (a + a + d)
        nrm = m / np.linalg.norm(m) if rng.random() < 0.8 else rng.normal(0, 1, 3)
        G[j]["normal"] = Rw @ nrm
        dm = np.linalg.norm(m)
        k = rng.random()
        G[j]["max_dist"] = dm * (rng.uniform(0.9, 3.0) if k < 0.7 else rng.uniform(0.1, 20.0))
        G[j]["min_dist"] = G[j]["max_dist"] / (1.2 ** 7) if k < 0.9 else 0.0
    return G


def test_restatement_equals_transcription():
    import psl_slam_amd as P
    rng = np.random.default_rng(11)
    cam = np.ascontiguousarray(camera()).reshape(1)
    lsf = F32(np.log(F32(1.2)))
    n_in = n_all = 0
    for trial in range(40):
        T = P.pose(np.eye(4)) if trial == 0 else P.pose(np.vstack([np.hstack([np.linalg.qr(rng.normal(0, 1, (3, 3)))[0] * (1 if trial % 2 else 1),
                                                                               rng.normal(0, 1, (3, 1))]), [0, 0, 0, 1]]))
        T = np.ascontiguousarray(T).reshape(1)
        G = random_lines(rng, T[0], 200)
        G[:5]["sp"][:, 2] = np.nan if trial % 3 == 0 else G[:5]["sp"][:, 2]
        for j in range(len(G)):
            got, out, lvl = oracle_lib.lr_in_frustum(G[j:j + 1], T, cam, BOUNDS, 0.5, lsf)
            want = is_in_frustum(G[j], T[0], cam[0], BOUNDS, 0.5, lsf)
            n_all += 1
            assert bool(got) == (want is not None), (trial, j)
            if want is not None:
                n_in += 1
                assert out.tobytes() == np.asarray(want[:5], np.float32).tobytes() and lvl == want[5], (trial, j)
    assert n_in > 100 and n_all - n_in > 1000


# ratios of the sweep whose level with ceil(psl_log(ratio) / (double)lsf) differs from the float path (2 of 20.6 M)
DOUBLE_PATH_FLIPS = 2


def test_predict_scale_log_sweep():
    """MapLine::PredictScale for every float ratio isInFrustum lets through (mfMaxDistance / dist with 0.8 * min <= dist <= 1.2 * max,
    max / min = 1.2^7 as MapLine::UpdateAverageDir sets it): the library's level (correctly rounded logf of psl_log, float quotient and
    ceil) against the host's logf and against the double path of the point projections."""
    lsf = F32(np.log(F32(1.2)))
    lo = F32(1.0) / F32(1.2)
    hi = F32(F32(1.2) ** 7) / F32(0.8)
    n, flips = oracle_lib.lr_level_sweep(lo, hi, lsf)
    assert n > 20_000_000
    assert flips[0] == 0, f"{flips[0]} ratios of {n} give another level with the host's logf"
    # the double path differs where logf(ratio) / lsf rounds onto an integer: the reason the float path is restated
    assert flips[1] == DOUBLE_PATH_FLIPS, flips[1]
    # unclamped levels and the defined edge cases
    assert oracle_lib.lr_level(0.5, lsf, 0) == -3
    assert oracle_lib.lr_level(1000.0, lsf, 0) == 38
    assert oracle_lib.lr_level(np.inf, lsf, 0) == 2**31 - 1
    assert oracle_lib.lr_level(0.0, lsf, 0) == -2**31
    assert oracle_lib.lr_level(np.nan, lsf, 0) == 0


def test_line_projection_dtypes_match_header():
    import psl_slam_amd as P
    sz = oracle_lib.lr_sizes()
    assert list(sz) == [P.MAPLINE_DTYPE.itemsize, P.LASTLINE_DTYPE.itemsize, P.LINEQUERY_DTYPE.itemsize] == [80, 88, 64]
    assert P.LASTLINE_DTYPE.fields["state"][1] == 80 and P.MAPLINE_DTYPE.fields["min_dist"][1] == 72


def test_line_projection_entry_points_reject_bad_arguments_without_a_gpu():
    import psl_slam_amd as P
    P.build()
    L = P.lib()
    fb = [C.c_float(v) for v in BOUNDS]
    cam = np.ascontiguousarray(camera()).reshape(1)
    nq = C.c_int(7)
    E, ECAP = -1, -4  # PSLFE_E_INVALID, PSLFE_E_CAPACITY
    f = C.c_float
    assert L.pslfe_line_project_frustum(None, None, None, None, 0, None, f(0.18), f(0.5), f(1.0), *fb, None, None, None, C.byref(nq), 0,
                                        None, None, None) == E
    assert L.pslfe_line_project_frustum_device(None, 1, None, None, None, None, 16, None, f(0.18), f(0.5), f(1.0), *fb, None, None, None,
                                               None, 16, None, None, None) == E
    assert L.pslfe_line_project_last(None, None, None, 0, None, None, None, None, f(10.0), *fb, None, None, None, C.byref(nq), 0) == E
    assert L.pslfe_line_project_last_device(None, 1, None, None, None, 16, None, None, None, None, f(10.0), *fb, None, None, None, None,
                                            16) == E
    assert L.pslfe_glue_lines3d_device(None, None, None) == E
    assert "NULL" in L.pslfe_last_error().decode() or "glue" in L.pslfe_last_error().decode()


def test_line_search_device_rejects_bad_arguments_without_a_gpu():
    import psl_slam_amd as P
    P.build()
    L = P.lib()
    fb = [C.c_float(v) for v in BOUNDS]
    x = C.c_void_p(16)
    f = C.c_float
    E, ECAP = -1, -4
    s = L.pslfe_line_search_by_projection_device
    # the argument checks come before any use of the context or of a device address
    args = lambda mode, d3, st3, klst, ctx=None: (ctx, 1, x, x, x, x, klst, d3, st3, *fb, x, x, x, 16, None, mode, f(0.95), x, None, x, None)
    assert s(*args(2, None, 0, 64)) == E and "mode 2" in L.pslfe_last_error().decode()              # unknown mode
    assert s(*args(1, None, 64, 64)) == E and "mvLines3D" in L.pslfe_last_error().decode()         # mode 1 without mvLines3D
    assert s(*args(1, x, 128, 64)) == E and "stride 128" in L.pslfe_last_error().decode()          # glue stride != keyline stride
    assert s(*args(0, None, 0, 2048)) == ECAP and "kl_stride 2048" in L.pslfe_last_error().decode()  # more lines than the LDS grid holds
    assert s(*args(0, None, 0, 64)) == E and "NULL" in L.pslfe_last_error().decode()               # no context
