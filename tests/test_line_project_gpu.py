"""GPU parity of the map-line projections (pslfe_line_project_frustum[_device], pslfe_line_project_last[_device]) with the sequential
restatement oracle/line_project_oracle.cpp, bit for bit; of the batched line window search (pslfe_line_search_by_projection_device, both
modes) with the one-frame entry point and the oracle; and of the device chain line extraction -> pairing -> glue -> projections ->
batched search with a host chain that fetches each frame, projects with the restatement and searches with the oracle."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import synth_frames as sf
from project_cases import T4, rot

pytestmark = pytest.mark.gpu

W, H = 640, 480
TUM1_NODIST = (517.306408, 516.469215, 318.643040, 255.313989, 0, 0, 0, 0, 0, 40.0)
BOUNDS = (0.0, 0.0, float(W), float(H))
F32 = np.float32
LSF = float(np.log(F32(1.2)))
NNR = 0.95
E_CAPACITY = -4


def camera():
    import psl_slam_amd as P
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, TUM1_NODIST):
        cam[k] = F32(v)
    return cam


class Batch:
    """B frames of a synthetic style through the batched line extractor, the pairing and the glue, all on the device."""

    def __init__(self, style, B, seed, ctx):
        import torch
        import psl_slam_amd as P
        self.dev = torch.device("cuda", 0)
        sc = sf.Scene(W, H, style, seed)
        gray = np.ascontiguousarray(np.stack([sc.gray(t) for t in range(B)], 0))
        depth = np.ascontiguousarray(np.stack([sc.depth_u16(t).astype(np.float32) / F32(5000.0) for t in range(B)], 0))
        self.d_gray, self.d_depth = torch.from_numpy(gray).to(self.dev), torch.from_numpy(depth).to(self.dev)
        self.cam = camera()
        self.le = P.LINEextractor(1, 1.2, 200, 0.0, ctx=ctx, max_batch=B)
        self.le.extract_batch_device(self.d_gray.data_ptr(), B, W, H, W, W * H)
        self.le.pair_batch_device(20.0, float(F32(np.pi / 4)))
        self.d_kls, self.d_desc, self.d_eq, self.d_nkl, self.cap = self.le.results_device()
        d_fans, d_nfans = self.le.fans_device()
        self.glue = P.FrameGlue(max_lines=self.cap, max_fans=4096, max_batch=B, ctx=ctx)
        self.glue.run_batch_device(B, self.d_kls, self.cap, self.d_nkl, d_fans, 4096, d_nfans, self.d_depth.data_ptr(), W, H, self.cam, 1)
        self.d_l3, self.l3_stride = self.glue.lines3d_device()
        self.B = B

    def frame(self, f):
        k, d, e, st = self.le.fetch(f, self.cap)
        l3 = self.glue.fetch(f, len(k))["lines3d"]
        return k, d, e, l3


def world_lines(rng, l3, Twc, state=True):
    """Map lines from a frame's mvLines3D (camera coordinates) moved to the world by Twc; normals from the camera centre."""
    import psl_slam_amd as P
    n = len(l3)
    G = np.zeros(n, P.LASTLINE_DTYPE)
    R, t = Twc[:3, :3], Twc[:3, 3]
    sp, ep = l3[:, :3] @ R.T + t, l3[:, 3:] @ R.T + t
    G["sp"], G["ep"] = sp, ep
    mid = 0.5 * (l3[:, :3] + l3[:, 3:])
    nm = np.linalg.norm(mid, axis=1)
    ok = nm > 0
    G["normal"][ok] = (mid[ok] / nm[ok, None]) @ R.T
    G["max_dist"] = (nm * 1.2).astype(np.float32)
    G["min_dist"] = (G["max_dist"] / F32(1.2 ** 7)).astype(np.float32)
    if state:
        G["state"] = np.where(ok, rng.choice([0, 1, 2, 2, 2], n), 0) | np.where(rng.random(n) < 0.1, 8, 0)
    return G


def adversarial_lines(T, cam, lsf):
    """Map lines at the edges of every gate of isInFrustum for the camera pose T (4x4 Tcw)."""
    import psl_slam_amd as P
    Twc = np.linalg.inv(T)
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    out = []

    def add(a, b, mn=0.5, mx=10.0, nrm=None, cam_coords=True):
        g = np.zeros((), P.LASTLINE_DTYPE)
        if cam_coords:
            a = Twc[:3, :3] @ np.asarray(a, float) + Twc[:3, 3]
            b = Twc[:3, :3] @ np.asarray(b, float) + Twc[:3, 3]
        g["sp"], g["ep"] = a, b
        m = 0.5 * (np.asarray(a) + np.asarray(b)) - Twc[:3, 3]
        g["normal"] = m / np.linalg.norm(m) if nrm is None else nrm
        g["min_dist"], g["max_dist"] = mn, mx
        g["state"] = 2
        out.append(g)

    add([0, 0, 2], [0.1, 0, -1])                        # one endpoint behind
    add([0, 0, 2], [0.0, 0, 0.0])                       # at z == 0, on the axis: the reference's u = 0*inf
    add([0, 0, 2], [0.3, 0, 0.0])                       # at z == 0 beside the axis
    add([np.nan, 0, 2], [0, 0, 2.5])                    # NaN coordinate
    add([0, 0, 2], [0, 0, 2.5], nrm=[np.nan, 0, 1])      # NaN normal
    # an endpoint around each image bound: u = fx*x/z + cx with z = 2 at the bound, one float step in and out
    for ub in (0.0, float(W)):
        x = (ub - cx) * 2.0 / fx
        for d in (-1e-6, 0.0, 1e-6):
            add([x + d, 0.0, 2.0], [0.0, 0.1, 2.2])
    for vb in (0.0, float(H)):
        y = (vb - cy) * 2.0 / fy
        for d in (-1e-6, 0.0, 1e-6):
            add([0.0, 0.1, 2.2], [0.05, y + d, 2.0])
    # dist exactly at 0.8f*min and 1.2f*max (and one float step beyond): dist as the kernel computes it
    a, b = np.array([-0.1, 0.0, 2.0]), np.array([0.1, 0.0, 2.0])
    d = line_dist(Twc[:3, :3] @ a + Twc[:3, 3], Twc[:3, :3] @ b + Twc[:3, 3], T)
    for f, lo in ((F32(1.2), False), (F32(0.8), True)):
        v = F32(d / f)
        for _ in range(8):
            if f * v == d:
                break
            v = np.nextafter(v, F32(np.inf) if f * v < d else F32(0), dtype=np.float32)
        for w in (v, np.nextafter(v, F32(np.inf) if lo else F32(0), dtype=np.float32)):
            add(a, b, mn=w if lo else 0.1, mx=5.0 if lo else w)
    # viewCos at the limit 0.5: normal at 60 degrees to the viewing ray
    for a in (np.pi / 3 - 1e-7, np.pi / 3, np.pi / 3 + 1e-7):
        add([-0.1, 0.0, 2.0], [0.1, 0.0, 2.0], nrm=Twc[:3, :3] @ np.array([np.sin(a), 0, np.cos(a)]))
    # negative and above-range levels (unclamped), a ratio of +inf (min 0 lets dist reach 0), min 0 with dist > 0
    add([-0.1, 0.0, 2.0], [0.1, 0.0, 2.0], mn=0.1, mx=2.0 * 1.2 ** -3)
    add([-0.1, 0.0, 2.0], [0.1, 0.0, 2.0], mn=0.1, mx=2.0 * 1.2 ** 12 / 1.2)
    add([-0.1, 0.0, 2.0], [0.1, 0.0, 2.0], mn=0.0, mx=1e30)
    add([-0.1, 0.0, 2.0], [0.1, 0.0, 2.0], mn=0.0, mx=0.0)                  # ratio 0
    add(Twc[:3, 3], Twc[:3, 3], mn=0.0, mx=3.0, nrm=[0.0, 0.0, 1.0], cam_coords=False)   # both endpoints at the camera centre
    # on the optical axis at 2.5e38: 0.5f*SP + 0.5f*EP stays finite (in view, a finite level), SP + EP would be +inf
    add([0, 0, 2.5e38], [0, 0, 2.5e38], mn=1.0, mx=3e38, nrm=Twc[:3, :3] @ np.array([0.0, 0.0, 1.0]))
    G = np.stack(out)
    G[1]["state"], G[2]["state"], G[3]["state"] = 1, 9, 2   # state and outlier bits
    return G


def line_dist(sp, ep, T):
    """|0.5f*SP + 0.5f*EP - mOw| under the conventions of include/pslfe.h (world endpoints, 4x4 Tcw)."""
    P_ = np.ascontiguousarray(T[:3, :3], np.float32)
    t = np.asarray(T[:3, 3], np.float32)
    Ow = [-F32(float(P_[0, r]) * float(t[0]) + float(P_[1, r]) * float(t[1]) + float(P_[2, r]) * float(t[2])) for r in range(3)]
    OM = [(F32(0.5) * F32(sp[k]) + F32(0.5) * F32(ep[k])) - Ow[k] for k in range(3)]
    return F32(np.sqrt(sum(float(o) * float(o) for o in OM)))


def restated_frustum(T, G, gd, cam, limit, th):
    import psl_slam_amd as P
    ml = G[list(P.MAPLINE_DTYPE.names)].astype(P.MAPLINE_DTYPE)
    return oracle_lib.lr_project_frustum(P.pose(T).reshape(1), ml, gd, np.ascontiguousarray(cam).reshape(1), LSF, limit, th, BOUNDS)


def restated_last(kls, ldesc, L, mldesc, T, cam, th):
    import psl_slam_amd as P
    return oracle_lib.lr_project_last(kls, ldesc, L, mldesc, P.pose(T).reshape(1), np.ascontiguousarray(cam).reshape(1), th, BOUNDS)


def _t(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


@pytest.fixture(scope="module")
def batches():
    import torch
    import psl_slam_amd as P
    ctx = P.Context(0, torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    return ctx, {s: Batch(s, 66, 21, ctx) for s in ("sticks", "struct")}


@pytest.mark.parametrize("style", ["sticks", "struct"])
@pytest.mark.parametrize("th", [1.0, 3.0])
def test_line_projections_equal_restatement(batches, style, th):
    """Both projections, device and host forms, against the restatement: every row byte, owner, count, in-view flag, level and
    viewCos, on map lines from real frames plus the adversarial ones; qstride smaller than the count is reported."""
    import psl_slam_amd as P
    ctx, bs = batches
    b = bs[style]
    dev = b.dev
    rng = np.random.default_rng(7 if style == "sticks" else 8)
    cam = b.cam
    npairs = 8
    stride = b.cap + 64
    Gs = np.zeros((npairs, stride), P.MAPLINE_DTYPE)
    Ls = np.zeros((npairs, b.cap), P.LASTLINE_DTYPE)
    Gd = rng.integers(0, 256, (npairs, stride, 32), dtype=np.uint8)
    nml = np.zeros(npairs, np.int32)
    Ts, data = [], []
    for p in range(npairs):
        k, d, e, l3 = b.frame(p)
        Tlw = T4(rot(*rng.normal(0, 0.05, 3)), rng.normal(0, 0.2, 3))
        Tcw = T4(rot(*rng.normal(0, 0.01, 3)), rng.normal(0, 0.02, 3)) @ Tlw
        L = world_lines(rng, l3, np.linalg.inv(Tlw))
        A = adversarial_lines(Tcw, cam, LSF)
        G = np.concatenate([L, A[:-1]])
        G = G[rng.permutation(len(G))] if p % 2 else G
        G = np.concatenate([G, A[-1:]])   # the overflow line after the permutation: the draws stay those the scene checks below were written on
        n = min(len(G), stride)
        Gs[p, :n] = G[:n][list(P.MAPLINE_DTYPE.names)].astype(P.MAPLINE_DTYPE)
        nml[p] = n
        Ls[p, :len(L)] = L
        Ts.append(Tcw)
        data.append((k, d, L, n))
    d_T = _t(np.stack([P.pose(T) for T in Ts]).view(np.uint8), dev)
    # frustum, device, full capacity and a qstride smaller than some counts
    for qstride in (stride, 24):
        q = _t(np.zeros((npairs, qstride, 64), np.uint8), dev)
        qd, ow, nq = _t(np.zeros((npairs, qstride, 32), np.uint8), dev), _t(np.zeros((npairs, qstride), np.int32), dev), _t(np.zeros(npairs, np.int32), dev)
        iv, lv, vc = _t(np.zeros((npairs, stride), np.uint8), dev), _t(np.zeros((npairs, stride), np.int32), dev), _t(np.zeros((npairs, stride), np.float32), dev)
        d_G, d_Gd, d_n = _t(Gs.view(np.uint8), dev), _t(Gd, dev), _t(nml, dev)
        P.line_project_frustum_device(npairs, d_T.data_ptr(), d_G.data_ptr(), d_Gd.data_ptr(), d_n.data_ptr(), stride, cam, LSF, 0.5, th,
                                      BOUNDS, q.data_ptr(), qd.data_ptr(), ow.data_ptr(), nq.data_ptr(), qstride, iv.data_ptr(), lv.data_ptr(),
                                      vc.data_ptr(), ctx=ctx)
        ctx.synchronize()
        Q, QD, OW, NQ = _np(q, P.LINEQUERY_DTYPE).reshape(npairs, qstride), _np(qd), _np(ow), _np(nq)
        IV, LV, VC = _np(iv), _np(lv), _np(vc)
        small = 0
        for p in range(npairs):
            n = nml[p]
            rq, rqd, row, riv, rlv, rvc = restated_frustum(Ts[p], Gs[p, :n], Gd[p, :n], cam, 0.5, th)
            m = min(len(rq), qstride)
            small += len(rq) > qstride
            assert NQ[p] == len(rq) and Q[p, :m].tobytes() == rq[:m].tobytes(), f"pair {p}: frustum rows differ"
            assert (QD[p, :m] == rqd[:m]).all() and (OW[p, :m] == row[:m]).all()
            assert (IV[p, :n] == riv).all() and (LV[p, :n] == rlv).all() and VC[p, :n].tobytes() == rvc.tobytes()
            if qstride == stride:
                hq, hqd, how, hiv, hlv, hvc = P.line_project_frustum(P.pose(Ts[p]), Gs[p, :n], Gd[p, :n], cam, LSF, 0.5, th, BOUNDS, ctx=ctx)
                assert hq.tobytes() == rq.tobytes() and (hqd == rqd).all() and (how == row).all()
                assert (hiv == riv).all() and (hlv == rlv).all() and hvc.tobytes() == rvc.tobytes()
                assert len(rq) > 10 and len(set(rlv[riv == 1].tolist())) >= 3
                assert riv[-1] == 1 and rlv[-1] >= 0   # the overflow line, last of every pair: in view under 0.5f*SP + 0.5f*EP
        assert qstride == stride or small > 0
    # the adversarial lines: levels outside [0, 8) and the infinite ratio occur
    _, _, _, riv, rlv, _ = restated_frustum(Ts[0], Gs[0, :nml[0]], Gd[0, :nml[0]], cam, 0.5, th)
    assert (rlv[riv == 1] >= 8).any() and (riv == 0).any()
    with pytest.raises(P.PslfeError):  # the host form reports a count above its capacity
        _check_capacity(ctx, Ts[0], Gs[0, :nml[0]], Gd[0, :nml[0]], cam)
    # last-frame projection: device (with and without map-line descriptors) and host forms
    nk = np.array([len(x[0]) for x in data], np.int32)
    for use_md in (False, True):
        for qstride in (b.cap, 16):
            q = _t(np.zeros((npairs, qstride, 64), np.uint8), dev)
            qd, ow, nq = _t(np.zeros((npairs, qstride, 32), np.uint8), dev), _t(np.zeros((npairs, qstride), np.int32), dev), _t(np.zeros(npairs, np.int32), dev)
            d_L = _t(Ls.view(np.uint8), dev)
            MD = Gd[:, :b.cap]
            d_md = _t(MD, dev) if use_md else None
            P.line_project_last_device(npairs, b.d_kls, b.d_desc, b.d_nkl, b.cap, d_L.data_ptr(), d_md.data_ptr() if use_md else 0,
                                       d_T.data_ptr(), cam, 10.0 * th, BOUNDS, q.data_ptr(), qd.data_ptr(), ow.data_ptr(), nq.data_ptr(),
                                       qstride, ctx=ctx)
            ctx.synchronize()
            Q, QD, OW, NQ = _np(q, P.LINEQUERY_DTYPE).reshape(npairs, qstride), _np(qd), _np(ow), _np(nq)
            for p in range(npairs):
                k, d, L, _ = data[p]
                n = nk[p]
                md = MD[p, :n] if use_md else None
                rq, rqd, row = restated_last(k, d, Ls[p, :n], md, Ts[p], cam, 10.0 * th)
                m = min(len(rq), qstride)
                assert NQ[p] == len(rq) and Q[p, :m].tobytes() == rq[:m].tobytes(), f"pair {p}: last-frame rows differ"
                assert (QD[p, :m] == rqd[:m]).all() and (OW[p, :m] == row[:m]).all()
                if qstride == b.cap:
                    hq, hqd, how = P.line_project_last(k, d, Ls[p, :n], md, P.pose(Ts[p]), cam, 10.0 * th, BOUNDS, ctx=ctx)
                    assert hq.tobytes() == rq.tobytes() and (hqd == rqd).all() and (how == row).all()
                    assert len(rq) > 5 and (rq["blocks"] == 0).any() and (rq["blocks"] == 1).any()


def _check_capacity(ctx, T, G, Gd, cam):
    import psl_slam_amd as P
    ml = np.ascontiguousarray(G, P.MAPLINE_DTYPE)
    md = np.ascontiguousarray(Gd, np.uint8)
    q = np.zeros(2, P.LINEQUERY_DTYPE)
    qd = np.zeros((2, 32), np.uint8)
    nq = C.c_int()
    Tp = np.ascontiguousarray(P.pose(T)).reshape(1)
    c = np.ascontiguousarray(cam).reshape(1)
    rc = P.lib().pslfe_line_project_frustum(ctx._h, P._ptr(Tp), P._ptr(ml), P._ptr(md), len(ml), P._ptr(c), C.c_float(LSF), C.c_float(0.5),
                                            C.c_float(1.0), *[C.c_float(v) for v in BOUNDS], P._ptr(q), P._ptr(qd), None, C.byref(nq), 2,
                                            None, None, None)
    assert rc == E_CAPACITY and nq.value > 2
    P._check(rc, "pslfe_line_project_frustum")


def long_line_frame(rng, n=300):
    """Keylines spanning the image: far more (line, cell) entries than the LDS grid of the first launch holds."""
    import psl_slam_amd as P
    k = np.zeros(n, P.KEYLINE_DTYPE)
    y0, y1 = rng.uniform(1, H - 1, n), rng.uniform(1, H - 1, n)
    k["startPointX"], k["startPointY"], k["endPointX"], k["endPointY"] = 0.5, y0, W - 0.5, y1
    k["sPointInOctaveX"], k["sPointInOctaveY"], k["ePointInOctaveX"], k["ePointInOctaveY"] = 0.5, y0, W - 0.5, y1
    k["lineLength"] = np.hypot(W - 1.0, y1 - y0)
    k["octave"] = 0
    a, bb = y0 - y1, (W - 0.5) - 0.5
    c = 0.5 * y1 - (W - 0.5) * y0
    nrm = np.hypot(a, bb)
    eq = np.stack([a / nrm, bb / nrm, c / nrm], 1)
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    l3 = rng.normal(0, 1, (n, 6))
    return k, d, eq, l3


@pytest.mark.parametrize("style", ["sticks", "struct"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("with_taken", [False, True])
def test_line_search_device_equals_one_frame_and_oracle(batches, style, mode, with_taken):
    """pslfe_line_search_by_projection_device on 65 pairs (current = frame p + 1) with queries from the last frame's lines moved a
    little: every match, assignment and count equals the one-frame entry point and the oracle; one pair has long lines enough to take
    the second launch."""
    import psl_slam_amd as P
    ctx, bs = batches
    b = bs[style]
    dev = b.dev
    rng = np.random.default_rng(100 + mode + 2 * with_taken)
    npairs, K = b.B - 1, b.cap
    qstride = K
    kls = np.zeros((npairs, K), P.KEYLINE_DTYPE)
    desc = np.zeros((npairs, K, 32), np.uint8)
    eq = np.zeros((npairs, K, 3), np.float64)
    l3 = np.zeros((npairs, K, 6), np.float64)
    nkl = np.zeros(npairs, np.int32)
    Q = np.zeros((npairs, qstride), P.LINEQUERY_DTYPE)
    QD = np.zeros((npairs, qstride, 32), np.uint8)
    nq = np.zeros(npairs, np.int32)
    taken = np.zeros((npairs, K), np.uint8)
    frames = [b.frame(f) for f in range(b.B)]
    big = npairs // 2
    for p in range(npairs):
        k, d, e, L3 = frames[p + 1] if p != big else long_line_frame(rng)
        n = len(k)
        kls[p, :n], desc[p, :n], eq[p, :n], l3[p, :n], nkl[p] = k, d, e, L3, n
        kl0, d0, _, L30 = frames[p] if p != big else (k, d, e, L3)
        m = min(len(kl0), qstride)
        q = np.zeros(m, P.LINEQUERY_DTYPE)
        sh = rng.normal(0, 1.5, (m, 2)).astype(np.float32)
        q["x1"], q["y1"] = kl0["startPointX"][:m] + sh[:, 0], kl0["startPointY"][:m] + sh[:, 1]
        q["x2"], q["y2"] = kl0["endPointX"][:m] + sh[:, 0], kl0["endPointY"][:m] + sh[:, 1]
        q["radius"] = np.where(rng.random(m) < 0.5, F32(10.0), F32(20.0)) if mode == 0 else np.where(rng.random(m) < 0.5, F32(5.0), F32(8.0))
        q["th_cos"] = F32(0.96) if mode == 0 else F32(0.998)
        q["vx"] = kl0["ePointInOctaveX"][:m] - kl0["sPointInOctaveX"][:m]
        q["vy"] = kl0["ePointInOctaveY"][:m] - kl0["sPointInOctaveY"][:m]
        q["length"] = kl0["lineLength"][:m]
        q["blocks"] = rng.random(m) < 0.7
        q["wdir"] = (L30[:m, :3] - L30[:m, 3:]) + rng.normal(0, 0.01, (m, 3))
        Q[p, :m], nq[p] = q, m
        QD[p, :m] = np.where(rng.random((m, 1)) < 0.8, d0[:m], rng.integers(0, 256, (m, 32), dtype=np.uint8))
        if with_taken:
            taken[p, :n] = rng.random(n) < 0.2
    nq[1] = qstride + 5                                  # a count above qstride reads qstride rows
    d = {k_: _t(v, dev) for k_, v in dict(kls=kls.view(np.uint8), desc=desc, eq=eq, l3=l3, nkl=nkl, q=Q.view(np.uint8), qd=QD, nq=nq,
                                            taken=taken).items()}
    match = _t(np.full((npairs, qstride), -7, np.int32), dev)
    asg = _t(np.full((npairs, K), -7, np.int32), dev)
    nm, nfb = _t(np.zeros(npairs, np.int32), dev), _t(np.zeros(1, np.int32), dev)
    P.line_search_by_projection_device(npairs, d["kls"].data_ptr(), d["desc"].data_ptr(), d["eq"].data_ptr(), d["nkl"].data_ptr(), K,
                                       d["l3"].data_ptr() if mode == 1 else 0, K, BOUNDS, d["q"].data_ptr(), d["qd"].data_ptr(),
                                       d["nq"].data_ptr(), qstride, d["taken"].data_ptr() if with_taken else 0, mode, NNR, match.data_ptr(),
                                       asg.data_ptr(), nm.data_ptr(), nfb.data_ptr(), ctx=ctx)
    ctx.synchronize()
    M, A, NM, NFB = _np(match), _np(asg), _np(nm), _np(nfb)
    assert NFB[0] >= 1
    lm = P.LSDmatcher(NNR, ctx=ctx)
    total = 0
    for p in range(npairs):
        n, m = nkl[p], min(nq[p], qstride)
        dir3d = l3[p, :n, :3] - l3[p, :n, 3:]
        tk = taken[p, :n] if with_taken else None
        hn, hm, ha = lm.SearchByProjection(kls[p, :n], desc[p, :n], eq[p, :n], BOUNDS, Q[p, :m], QD[p, :m], mode=mode,
                                           dir3d=dir3d if mode == 1 else None, taken=tk)
        on, om, oa = oracle_lib.line_search_by_projection(kls[p, :n], desc[p, :n], eq[p, :n], BOUNDS, Q[p, :m], QD[p, :m], mode,
                                                          dir3d if mode == 1 else None, tk, NNR)
        assert hn == on and (hm == om).all() and (ha == oa).all(), f"pair {p}: one-frame entry point differs from the oracle"
        assert NM[p] == on and (M[p, :m] == om).all() and (A[p, :n] == oa).all(), f"pair {p}: batched search differs"
        assert (M[p, m:] == -7).all()
        total += on
    assert total > npairs


def test_line_device_chain_equals_host_chain():
    """line_extract_batch_device -> pair_batch_device -> glue_run_batch_device -> line_project_last_device / line_project_frustum_device
    -> line_search_by_projection_device (mode 0 on the last-frame rows, mode 1 on the frustum rows) on 257 'sticks' frames with no
    host round trip, against a host chain on sampled pairs: fetch, restated projections, oracle searches."""
    import torch
    import psl_slam_amd as P
    ctx = P.Context(0, torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    B = 257
    b = Batch("sticks", B, 5, ctx)
    dev, cam, K = b.dev, b.cam, b.cap
    npairs = B - 1
    rng = np.random.default_rng(3)
    torch.manual_seed(3)
    Tl = [T4(rot(*rng.normal(0, 0.03, 3)), rng.normal(0, 0.1, 3)) for _ in range(npairs)]
    Tc = [T4(rot(*rng.normal(0, 0.005, 3)), rng.normal(0, 0.01, 3)) @ T for T in Tl]
    d_Tc = _t(np.stack([P.pose(T) for T in Tc]).view(np.uint8), dev)
    # the caller's map-line records: on the device, from the glue's mvLines3D of frame p (world = camera p moved by Tl[p]^-1)
    l3 = torch.as_tensor(P._DevArray(b.d_l3, (B, K, 6), "<f8"), device=dev)
    Twl = torch.from_numpy(np.stack([np.linalg.inv(T) for T in Tl])).to(dev)
    sp = torch.einsum("pij,pkj->pki", Twl[:, :3, :3], l3[:npairs, :, :3]) + Twl[:, None, :3, 3]
    ep = torch.einsum("pij,pkj->pki", Twl[:, :3, :3], l3[:npairs, :, 3:]) + Twl[:, None, :3, 3]
    mid = 0.5 * (l3[:npairs, :, :3] + l3[:npairs, :, 3:])
    nmid = mid.norm(dim=2, keepdim=True)
    nrm = torch.einsum("pij,pkj->pki", Twl[:, :3, :3], mid / nmid.clamp_min(1e-300))
    rec = torch.zeros((npairs, K, 11), dtype=torch.float64, device=dev)
    rec[:, :, 0:3], rec[:, :, 3:6], rec[:, :, 6:9] = sp, ep, nrm
    mx = (nmid[:, :, 0] * 1.2).float()
    dist = torch.stack([(mx / F32(1.2 ** 7)), mx], 2).contiguous()
    state = torch.where(nmid[:, :, 0] > 0, torch.randint(1, 3, (npairs, K), device=dev), torch.zeros((), dtype=torch.int64, device=dev)).int()
    recb = rec.view(torch.uint8).view(npairs, K, 88)
    recb[:, :, 72:80] = dist.view(torch.uint8).view(npairs, K, 8)
    recb[:, :, 80:84] = state.contiguous().view(torch.uint8).view(npairs, K, 4)
    recb[:, :, 84:88] = 0
    d_last = recb.contiguous()
    d_geom = recb[:, :, :80].contiguous()
    # last-frame rows (pair p: last = frame p) and the mode-0 search on current = frame p + 1
    q0 = torch.zeros((npairs, K, 64), dtype=torch.uint8, device=dev)
    qd0, nq0 = torch.zeros((npairs, K, 32), dtype=torch.uint8, device=dev), torch.zeros(npairs, dtype=torch.int32, device=dev)
    P.line_project_last_device(npairs, b.d_kls, b.d_desc, b.d_nkl, K, d_last.data_ptr(), 0, d_Tc.data_ptr(), cam, 20.0, BOUNDS,
                               q0.data_ptr(), qd0.data_ptr(), 0, nq0.data_ptr(), K, ctx=ctx)
    kls_sz = P.KEYLINE_DTYPE.itemsize
    cur = lambda base, row: base + row * K  # frame p + 1 of every view
    m0 = torch.full((npairs, K), -1, dtype=torch.int32, device=dev)
    nm0 = torch.zeros(npairs, dtype=torch.int32, device=dev)
    P.line_search_by_projection_device(npairs, cur(b.d_kls, kls_sz), cur(b.d_desc, 32), cur(b.d_eq, 24), b.d_nkl + 4, K, 0, K, BOUNDS,
                                       q0.data_ptr(), qd0.data_ptr(), nq0.data_ptr(), K, 0, 0, NNR, m0.data_ptr(), 0, nm0.data_ptr(), ctx=ctx)
    # frustum rows of the same map lines and the mode-1 search
    nml = b.d_nkl  # frame p's line count for pair p
    q1 = torch.zeros((npairs, K, 64), dtype=torch.uint8, device=dev)
    qd1, nq1 = torch.zeros((npairs, K, 32), dtype=torch.uint8, device=dev), torch.zeros(npairs, dtype=torch.int32, device=dev)
    P.line_project_frustum_device(npairs, d_Tc.data_ptr(), d_geom.data_ptr(), b.d_desc, nml, K, cam, LSF, 0.5, 1.0, BOUNDS, q1.data_ptr(),
                                  qd1.data_ptr(), 0, nq1.data_ptr(), K, ctx=ctx)
    m1 = torch.full((npairs, K), -1, dtype=torch.int32, device=dev)
    nm1 = torch.zeros(npairs, dtype=torch.int32, device=dev)
    P.line_search_by_projection_device(npairs, cur(b.d_kls, kls_sz), cur(b.d_desc, 32), cur(b.d_eq, 24), b.d_nkl + 4, K,
                                       b.d_l3 + K * 6 * 8, b.l3_stride, BOUNDS, q1.data_ptr(), qd1.data_ptr(), nq1.data_ptr(), K, 0, 1, NNR,
                                       m1.data_ptr(), 0, nm1.data_ptr(), ctx=ctx)
    ctx.synchronize()
    LAST = d_last.cpu().numpy().view(P.LASTLINE_DTYPE).reshape(npairs, K)
    M0, NM0, NQ0 = m0.cpu().numpy(), nm0.cpu().numpy(), nq0.cpu().numpy()
    M1, NM1, NQ1 = m1.cpu().numpy(), nm1.cpu().numpy(), nq1.cpu().numpy()
    checked = tot0 = 0
    for p in sorted({0, 1, npairs // 2, npairs - 1} | set(range(0, npairs, 16))):
        k, d, e, _ = b.frame(p)
        k1, d1, e1, l31 = b.frame(p + 1)
        n = len(k)
        rq, rqd, _ = restated_last(k, d, LAST[p, :n], None, Tc[p], cam, 20.0)
        rn, rm, _ = oracle_lib.line_search_by_projection(k1, d1, e1, BOUNDS, rq, rqd, 0, None, None, NNR)
        assert NQ0[p] == len(rq) and NM0[p] == rn and (M0[p, :len(rq)] == rm).all(), f"pair {p}: mode-0 chain differs"
        G = LAST[p, :n]
        fq, fqd, _, _, _, _ = restated_frustum(Tc[p], G, d, cam, 0.5, 1.0)
        fn, fm, _ = oracle_lib.line_search_by_projection(k1, d1, e1, BOUNDS, fq, fqd, 1, l31[:, :3] - l31[:, 3:], None, NNR)
        assert NQ1[p] == len(fq) and NM1[p] == fn and (M1[p, :len(fq)] == fm).all(), f"pair {p}: mode-1 chain differs"
        tot0 += rn
        checked += 1
    assert checked >= 16 and tot0 > 0 and int(NM0.sum()) > npairs
