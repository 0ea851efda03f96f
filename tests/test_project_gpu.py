"""GPU parity of the projection entry points (pslfe_orb_project_last[_device], pslfe_orb_project_frustum[_device]) with the
sequential restatement oracle/project_oracle.cpp, field by field and bit for bit, and of the device chain
set_from_orb_rgbd -> project_last_device -> search_by_projection_last_device (and project_frustum_device ->
search_by_projection_map_device) with the sequential matcher oracle run on the restated queries."""
import ctypes as C
import zlib

import numpy as np
import pytest

import oracle_lib
import synth_frames as sf
from project_cases import T4, moved, restated_last, rot

pytestmark = pytest.mark.gpu

W, H = 640, 480
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0)
TUM1_NODIST = TUM1[:4] + (0, 0, 0, 0, 0) + TUM1[9:]
NLEVELS, SCALE = 8, 1.2
E_STATE, E_CAPACITY = -5, -4


def camera(vals):
    import psl_slam_amd as P
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, vals):
        cam[k] = np.float32(v)
    return cam


def depth_image(t):
    return (sf.Scene(W, H, "desk", seed=3).depth_u16(t).astype(np.float32) / np.float32(5000.0))


@pytest.fixture(scope="module")
def slots():
    """Two 'desk' frames on TUM1 (distorted) and on the same camera without distortion, through pslfe_frame_set_rgbd."""
    import psl_slam_amd as P
    orb = P.ORBextractor(1000, SCALE, NLEVELS, 20, 7)
    sc = sf.Scene(W, H, "desk", seed=3)
    frames = [orb(sc.gray(t)) for t in range(2)]
    cap = orb.max_keypoints(W, H)
    out = {}
    for name, vals in (("tum1", TUM1), ("nodist", TUM1_NODIST)):
        cam = camera(vals)
        g = P.FrameGrid(cap, 3)
        for s, (k, d) in enumerate(frames):
            g.set_rgbd(s, k, d, depth_image(s), cam)
        g.set(2, frames[0][0], frames[0][1], (0.0, 0.0, float(W), float(H)))   # no depth
        bounds = tuple(float(b) for b in g.image_bounds(cam, W, H))
        out[name] = (g, cam, bounds, [g.fetch(s) + (frames[s][1],) for s in range(2)])
    return out, orb.GetScaleFactors().astype(np.float32)


def caller_points(rng, slot_data, cam, Tlw):
    """LastFrame.mvpMapPoints: back-projected keypoints with noise, every state, outliers, and points far behind / beside the view."""
    import psl_slam_amd as P
    kun, dep, _, _ = slot_data
    n = len(kun)
    z = np.where(dep > 0, dep, rng.uniform(0.5, 4.0, n)).astype(np.float64)
    xc = (kun["x"] - cam["cx"]) * z / cam["fx"] + rng.normal(0, 0.01, n)
    yc = (kun["y"] - cam["cy"]) * z / cam["fy"] + rng.normal(0, 0.01, n)
    Xc = np.stack([xc, yc, z], 1)
    k = rng.random(n)
    Xc[k < 0.05, 2] *= -1.0                         # behind the camera
    Xc[(k >= 0.05) & (k < 0.1), 0] += 30.0          # outside the image
    Twl = np.linalg.inv(Tlw)
    Xw = Xc @ Twl[:3, :3].T + Twl[:3, 3]
    pts = np.zeros(n, P.LASTPOINT_DTYPE)
    pts["x"], pts["y"], pts["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    pts["state"] = rng.choice([0, 1, 2, 2, 2], n) | np.where(rng.random(n) < 0.1, 8, 0)
    mpdesc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return pts, mpdesc


POSES = {   # displacement of the current camera in the last camera's coordinates (mb = bf / fx = 0.077)
    "forward": ((0.0, 0.01, 0.2), False),
    "backward": ((0.02, 0.0, -0.2), False),
    "neither": ((0.03, -0.02, 0.05), False),
    "mono": ((0.0, 0.0, 0.2), True),
}


@pytest.mark.parametrize("camname", ["tum1", "nodist"])
@pytest.mark.parametrize("case", list(POSES))
@pytest.mark.parametrize("vo", [0, 1])
def test_project_last_equals_restatement(slots, camname, case, vo):
    out, scale = slots
    g, cam, bounds, data = out[camname]
    rng = np.random.default_rng(zlib.crc32(f"{camname} {case} {vo}".encode()))
    Tlw = T4(rot(0.1, -0.2, 0.05), (0.3, -0.1, 0.5))
    d, mono = POSES[case]
    Tcw = moved(Tlw, d, rot(0.0, 0.02, 0.01))
    pts, mpd = caller_points(rng, data[0], cam, Tlw)
    for th in (7.0, 15.0):
        for with_points in (True, False):
            p_, m_ = (pts, mpd) if with_points else (None, None)
            if not with_points and not vo:
                continue
            q, qd, ow = g.project_last(0, Tlw_p(Tlw), Tlw_p(Tcw), p_, m_, cam, scale, th, 3.0, mono, vo, bounds)
            rq, rqd, row = restated_last(data[0], Tlw, Tcw, p_, m_, cam, scale, th, 3.0, mono, vo, bounds)
            assert len(q) == len(rq) and len(q) > 50
            assert q.tobytes() == rq.tobytes(), "query rows differ from the restatement"
            np.testing.assert_array_equal(qd, rqd)
            np.testing.assert_array_equal(ow, row)
            lv = q["min_level"]
            if case == "forward":
                assert (q["max_level"] == -1).all()
            elif case == "backward":
                assert (lv == 0).all()
            else:
                assert (q["max_level"] - lv == 2).all()


def Tlw_p(T):
    import psl_slam_amd as P
    return P.pose(T)


def test_project_last_depth_zero_and_bounds(slots):
    """Points exactly at z == 0 of the current camera, just behind it and at the image border are not emitted (or emitted) exactly as
    the restatement says; VO with a depth cut of 0 visits the 101 closest keypoints."""
    import psl_slam_amd as P
    out, scale = slots
    g, cam, bounds, data = out["nodist"]
    n = len(data[0][0])
    Tlw = np.eye(4)
    Tcw = T4(np.eye(3), (0.0, 0.0, -1.0))
    pts = np.zeros(n, P.LASTPOINT_DTYPE)
    rng = np.random.default_rng(2)
    pts["x"], pts["y"] = rng.uniform(-0.5, 0.5, n), rng.uniform(-0.4, 0.4, n)
    pts["z"] = rng.choice(np.float32([1.0, 0.999, 1.001, 3.0, -2.0]), n)       # z == 1: camera depth exactly 0
    pts["state"] = 2
    q, qd, ow = g.project_last(0, P.pose(Tlw), P.pose(Tcw), pts, None, cam, scale, 10.0, 3.0, False, False, bounds)
    rq, rqd, row = restated_last(data[0], Tlw, Tcw, pts, None, cam, scale, 10.0, 3.0, False, False, bounds)
    assert q.tobytes() == rq.tobytes() and (ow == row).all() and (qd == rqd).all()
    assert not np.isin(ow, np.flatnonzero(pts["z"] == np.float32(1.0))).any()
    assert np.isin(ow, np.flatnonzero(pts["z"] == np.float32(3.0))).any()
    q, qd, ow = g.project_last(0, P.pose(Tlw), P.pose(Tlw), None, None, cam, scale, 10.0, 0.0, False, True, bounds)
    rq, rqd, row = restated_last(data[0], Tlw, Tlw, None, None, cam, scale, 10.0, 0.0, False, True, bounds)
    assert q.tobytes() == rq.tobytes() and (ow == row).all()
    assert 90 <= len(q) <= 101


def test_self_projection_matches_own_keypoints(slots):
    """Slot s projected onto itself (Tcw == Tlw) in VO mode: the window search gives >= 95 % of the rows their own keypoint."""
    import psl_slam_amd as P
    out, scale = slots
    for camname in ("tum1", "nodist"):
        g, cam, bounds, data = out[camname]
        T = T4(rot(0.2, 0.1, -0.3), (1.0, 2.0, -0.5))
        for s in (0, 1):
            q, qd, ow = g.project_last(s, P.pose(T), P.pose(T), None, None, cam, scale, 7.0, 100.0, False, True, bounds)
            assert len(q) > 300
            nm, match, _ = P.ORBmatcher(0.9, True).SearchByProjectionLast(g, s, q, qd)
            assert (match == ow).mean() >= 0.95, (camname, s, (match == ow).mean())


def test_project_last_error_paths(slots):
    import psl_slam_amd as P
    out, scale = slots
    g, cam, bounds, data = out["nodist"]
    T = P.pose(np.eye(4))
    with pytest.raises(P.PslfeError, match="code -5"):
        g.project_last(2, T, T, None, None, cam, scale, 7.0, 3.0, False, True, bounds)     # VO on a slot without depth
    g.project_last(2, T, T, None, None, cam, scale, 7.0, 3.0, False, False, bounds)        # without VO it is fine
    L = P.lib()
    cam1 = np.ascontiguousarray(cam).reshape(1)
    fb = [C.c_float(b) for b in bounds]
    rc = L.pslfe_orb_project_last_device(g._h, 0, 1, C.c_void_p(16), C.c_void_p(16), None, None, P._ptr(cam1), P._ptr(scale), NLEVELS,
                                         C.c_float(7.0), C.c_float(3.0), 0, 0, *fb, C.c_void_p(16), C.c_void_p(16), None,
                                         C.c_void_p(16), g.cap + 1)
    assert rc == E_CAPACITY
    rc = L.pslfe_orb_project_last_device(g._h, 2, 1, C.c_void_p(16), C.c_void_p(16), None, None, P._ptr(cam1), P._ptr(scale), NLEVELS,
                                         C.c_float(7.0), C.c_float(3.0), 0, 1, *fb, C.c_void_p(16), C.c_void_p(16), None,
                                         C.c_void_p(16), g.cap)
    assert rc == E_STATE


def map_points(rng, n, Tcw):
    """Local map points around the view of Tcw with every frustum gate in play."""
    import psl_slam_amd as P
    Twc = np.linalg.inv(Tcw)
    z = rng.uniform(0.5, 6.0, n)
    Xc = np.stack([rng.uniform(-0.8, 0.8, n) * z, rng.uniform(-0.6, 0.6, n) * z, z], 1)
    k = rng.random(n)
    Xc[k < 0.05, 2] *= -1.0
    Xc[(k >= 0.05) & (k < 0.08), 2] = 0.0
    Xw = Xc @ Twc[:3, :3].T + Twc[:3, 3]
    dist = np.linalg.norm(Xc, axis=1)
    nrm = Xc / np.maximum(dist, 1e-9)[:, None]
    tilt = rng.choice([0.0, 0.01, 0.05, 0.5, 1.2, 2.5], n)                 # viewCos > 0.998, below, and below the 0.5 limit
    nrm = nrm + tilt[:, None] * rng.normal(0, 1, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    mp = np.zeros(n, P.MAPPOINT_DTYPE)
    mp["x"], mp["y"], mp["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
    mp["nx"], mp["ny"], mp["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    lvl = rng.integers(-2, 10, n)                                         # predicted levels below 0 and beyond 7: the clamps
    mx = dist * SCALE ** lvl * rng.uniform(0.95, 1.05, n)
    mx = np.where(rng.random(n) < 0.05, dist / 2.0, mx)                   # too far for the scale range
    mn = mx / SCALE ** 7
    mn = np.where(rng.random(n) < 0.05, dist * 2.0, mn)                   # too close
    mp["max_dist"], mp["min_dist"] = mx, mn
    return mp, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def restated_frustum(Tcw, mp, mpd, cam, scale, lsf, limit, th, bounds):
    import psl_slam_amd as P
    return oracle_lib.pr_project_frustum(P.pose(Tcw).reshape(1), mp, mpd, np.ascontiguousarray(cam).reshape(1), scale, lsf, limit, th, bounds)


@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
def test_project_frustum_equals_restatement(slots, th):
    import psl_slam_amd as P
    out, scale = slots
    _, cam, bounds, _ = out["tum1"]
    lsf = np.float32(np.log(np.float32(SCALE)))
    rng = np.random.default_rng(int(th))
    Tcw = T4(rot(0.3, -0.1, 0.2), (0.5, 0.2, -1.0))
    mp, mpd = map_points(rng, 6000, Tcw)
    got = P.project_frustum(P.pose(Tcw), mp, mpd, cam, scale, lsf, 0.5, th, bounds)
    ref = restated_frustum(Tcw, mp, mpd, cam, scale, lsf, 0.5, th, bounds)
    for a, b, name in zip(got, ref, ("queries", "qdesc", "owner", "inview", "level", "viewcos")):
        assert len(a) == len(b) and a.tobytes() == b.tobytes(), f"{name} differ from the restatement"
    q, _, ow, iv, lv, vc = got
    assert 500 < len(q) < len(mp) * 4 // 5 and iv.sum() == len(q)
    assert (lv[iv == 1] == 0).any() and (lv[iv == 1] == NLEVELS - 1).any()           # both clamps
    r = q["radius"] / scale[q["max_level"]] / (np.float32(th) if th != 1 else np.float32(1))
    assert np.isclose(r, 2.5).any() and np.isclose(r, 4.0).any()                    # both radius branches
    assert (vc[iv == 1] >= 0.5).all()
    # every gate rejects something: behind / at z == 0, outside the image, too far, too close, viewing angle
    X = np.stack([mp["x"], mp["y"], mp["z"]], 1).astype(np.float64)
    Pc = X @ Tcw[:3, :3].T + Tcw[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = cam["fx"] * Pc[:, 0] / Pc[:, 2] + cam["cx"], cam["fy"] * Pc[:, 1] / Pc[:, 2] + cam["cy"]
    img = (Pc[:, 2] > 1e-3) & (u > bounds[0] + 1) & (u < bounds[2] - 1) & (v > bounds[1] + 1) & (v < bounds[3] - 1)
    O = -Tcw[:3, :3].T @ Tcw[:3, 3]
    dist = np.linalg.norm(X - O, axis=1)
    far, near = dist > 1.2 * mp["max_dist"] * 1.001, dist < 0.8 * mp["min_dist"] * 0.999
    cosv = np.sum((X - O) * np.stack([mp["nx"], mp["ny"], mp["nz"]], 1), 1) / dist
    assert ((Pc[:, 2] <= 0) & (iv == 0)).any() and (~img & (Pc[:, 2] > 1e-3) & (iv == 0)).any()
    assert (img & far & (iv == 0)).any() and (img & near & (iv == 0)).any()
    assert (img & ~far & ~near & (cosv < 0.499) & (iv == 0)).any()


def test_project_frustum_capacity_is_reported(slots):
    import psl_slam_amd as P
    out, scale = slots
    _, cam, bounds, _ = out["tum1"]
    lsf = float(np.log(np.float32(SCALE)))
    Tcw = T4(np.eye(3), (0, 0, 0))
    mp, mpd = map_points(np.random.default_rng(4), 300, Tcw)
    q, *_ = P.project_frustum(P.pose(Tcw), mp, mpd, cam, scale, lsf, 0.5, 1.0, bounds)
    k = len(q)
    assert k > 20
    T = P.pose(Tcw).reshape(1)
    cam1 = np.ascontiguousarray(cam).reshape(1)
    qq = np.zeros(k, P.PROJQUERY_DTYPE)
    qd = np.zeros((k, 32), np.uint8)
    nq = C.c_int()
    rc = P.lib().pslfe_orb_project_frustum(P.default_context()._h, P._ptr(T), P._ptr(mp), P._ptr(mpd), len(mp), P._ptr(cam1), P._ptr(scale),
                                           NLEVELS, C.c_float(lsf), C.c_float(0.5), C.c_float(1.0), *[C.c_float(b) for b in bounds],
                                           P._ptr(qq), P._ptr(qd), None, C.byref(nq), k - 1, None, None, None)
    assert rc == E_CAPACITY and nq.value == k


def _chain(style, B, seed):
    """extract_batch_device -> set_from_orb_rgbd -> project_last_device (VO, pair p: slot p -> slot p + 1) ->
    search_by_projection_last_device, and project_frustum_device -> search_by_projection_map_device, all on the device."""
    import torch
    import psl_slam_amd as P
    dev = torch.device("cuda", 0)
    sc = sf.Scene(W, H, style, seed)
    gray = np.ascontiguousarray(np.stack([sc.gray(t) for t in range(B)], 0))
    depth = np.ascontiguousarray(np.stack([sc.depth_u16(t).astype(np.float32) / np.float32(5000.0) for t in range(B)], 0))
    cam = camera(TUM1_NODIST)
    ctx = P.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    orb = P.ORBextractor(1000, SCALE, NLEVELS, 20, 7, ctx=ctx, max_batch=B)
    cap = orb.max_keypoints(W, H)
    g = P.FrameGrid(cap, B, ctx=ctx)
    scale = orb.GetScaleFactors().astype(np.float32)
    d_gray, d_depth = torch.from_numpy(gray).to(dev), torch.from_numpy(depth).to(dev)
    orb.extract_batch_device(d_gray.data_ptr(), B, W, H, W, W * H)
    g.set_from_orb_rgbd(orb, d_depth.data_ptr(), W, H, cam)
    bounds = tuple(float(b) for b in g.image_bounds(cam, W, H))
    npairs = B - 1
    rng = np.random.default_rng(seed)
    Tl = [T4(rot(*rng.normal(0, 0.05, 3)), rng.normal(0, 0.1, 3)) for _ in range(npairs)]
    Tc = [moved(T, rng.normal(0, 0.01, 3)) for T in Tl]
    poses = lambda Ts: torch.from_numpy(np.stack([P.pose(T) for T in Ts]).view(np.uint8)).to(dev)
    d_Tl, d_Tc = poses(Tl), poses(Tc)
    q = torch.zeros((npairs, cap, 32), dtype=torch.uint8, device=dev)
    qd = torch.zeros((npairs, cap, 32), dtype=torch.uint8, device=dev)
    ow = torch.zeros((npairs, cap), dtype=torch.int32, device=dev)
    nq = torch.zeros((npairs,), dtype=torch.int32, device=dev)
    match = torch.full((npairs, cap), -1, dtype=torch.int32, device=dev)
    nm = torch.zeros((npairs,), dtype=torch.int32, device=dev)
    g.project_last_device(0, npairs, d_Tl.data_ptr(), d_Tc.data_ptr(), 0, 0, cam, scale, 15.0, 3.0, False, True, bounds, q.data_ptr(),
                          qd.data_ptr(), ow.data_ptr(), nq.data_ptr(), cap)
    P.search_by_projection_last_device(g, 1, npairs, q.data_ptr(), qd.data_ptr(), nq.data_ptr(), cap, True, match.data_ptr(), nm.data_ptr())
    # the local map of frame p + 1: the last frame's keypoints with depth as map points (world = last camera of pair p)
    M = cap
    mps = np.zeros((npairs, M), P.MAPPOINT_DTYPE)
    mpd = np.zeros((npairs, M, 32), np.uint8)
    nmp = np.zeros(npairs, np.int32)
    samples = sorted({0, 1, npairs // 2, npairs - 1})
    data = {}
    for p in range(npairs):
        if p not in samples and p % 8:
            continue
        kun, dep, ur = g.fetch(p)
        _, desc = orb.fetch(p, W, H)
        data[p] = (kun, dep, ur, desc)
        data_next = g.fetch(p + 1) + (orb.fetch(p + 1, W, H)[1],)
        data[p + 1] = data_next
        ok = np.flatnonzero(dep > 0)
        z = dep[ok].astype(np.float64)
        Xc = np.stack([(kun["x"][ok] - cam["cx"]) * z / cam["fx"], (kun["y"][ok] - cam["cy"]) * z / cam["fy"], z], 1)
        Tw = np.linalg.inv(Tl[p])
        Xw = Xc @ Tw[:3, :3].T + Tw[:3, 3]
        k = len(ok)
        mps[p, :k]["x"], mps[p, :k]["y"], mps[p, :k]["z"] = Xw[:, 0], Xw[:, 1], Xw[:, 2]
        nrm = Xc / np.linalg.norm(Xc, axis=1)[:, None] @ Tw[:3, :3].T
        mps[p, :k]["nx"], mps[p, :k]["ny"], mps[p, :k]["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
        d = np.linalg.norm(Xc, axis=1) * scale[kun["octave"][ok]]
        mps[p, :k]["max_dist"], mps[p, :k]["min_dist"] = d, d / scale[NLEVELS - 1]
        mpd[p, :k] = desc[ok]
        nmp[p] = k
    d_mp = torch.from_numpy(mps.view(np.uint8).reshape(npairs, -1)).to(dev)
    d_mpd, d_nmp = torch.from_numpy(mpd).to(dev), torch.from_numpy(nmp).to(dev)
    fq = torch.zeros((npairs, cap, 32), dtype=torch.uint8, device=dev)
    fqd = torch.zeros((npairs, cap, 32), dtype=torch.uint8, device=dev)
    fnq = torch.zeros((npairs,), dtype=torch.int32, device=dev)
    fmatch = torch.full((npairs, cap), -1, dtype=torch.int32, device=dev)
    fnm = torch.zeros((npairs,), dtype=torch.int32, device=dev)
    lsf = float(np.log(np.float32(SCALE)))
    P.project_frustum_device(npairs, d_Tc.data_ptr(), d_mp.data_ptr(), d_mpd.data_ptr(), d_nmp.data_ptr(), M, cam, scale, lsf, 0.5, 1.0,
                             bounds, fq.data_ptr(), fqd.data_ptr(), 0, fnq.data_ptr(), cap, ctx=ctx)
    P.search_by_projection_map_device(g, 1, npairs, fq.data_ptr(), fqd.data_ptr(), fnq.data_ptr(), cap, 0, 0.8, fmatch.data_ptr(),
                                      fnm.data_ptr())
    torch.cuda.synchronize(dev)
    Q = q.cpu().numpy().view(P.PROJQUERY_DTYPE).reshape(npairs, cap)
    QD, OW, NQ, MATCH, NM = qd.cpu().numpy(), ow.cpu().numpy(), nq.cpu().numpy(), match.cpu().numpy(), nm.cpu().numpy()
    FQ = fq.cpu().numpy().view(P.PROJQUERY_DTYPE).reshape(npairs, cap)
    FQD, FNQ, FMATCH, FNM = fqd.cpu().numpy(), fnq.cpu().numpy(), fmatch.cpu().numpy(), fnm.cpu().numpy()
    checked = 0
    for p in sorted(k for k in data if k < npairs and nmp[k] > 0):
        rq, rqd, row = restated_last(data[p], Tl[p], Tc[p], None, None, cam, scale, 15.0, 3.0, False, True, bounds)
        n = NQ[p]
        assert n == len(rq) and Q[p, :n].tobytes() == rq.tobytes(), f"pair {p}: query rows differ"
        assert (QD[p, :n] == rqd).all() and (OW[p, :n] == row).all()
        kun1, _, ur1, desc1 = data[p + 1]
        rnm, rmatch, _ = oracle_lib.search_by_projection_last(kun1, desc1, ur1, bounds, rq, rqd, None, True)
        assert NM[p] == rnm and (MATCH[p, :n] == rmatch).all(), f"pair {p}: matches differ from the oracle"
        fr = restated_frustum(Tc[p], mps[p, :nmp[p]], mpd[p, :nmp[p]], cam, scale, np.float32(lsf), 0.5, 1.0, bounds)
        m = FNQ[p]
        assert m == len(fr[0]) and m <= cap and FQ[p, :m].tobytes() == fr[0].tobytes() and (FQD[p, :m] == fr[1]).all()
        fnm_, fm_, _ = oracle_lib.search_by_projection_map(kun1, desc1, ur1, bounds, fr[0], fr[1], None, 0.8)
        assert FNM[p] == fnm_ and (FMATCH[p, :m] == fm_).all(), f"pair {p}: map matches differ from the oracle"
        assert rnm > 0 and fnm_ > 0
        checked += 1
    assert checked >= 4
    ctx.synchronize()


@pytest.mark.parametrize("style", ["desk", "sticks"])
@pytest.mark.parametrize("B", [32, 97])
def test_device_chain_equals_oracle(style, B):
    _chain(style, B, seed=40 + B)
