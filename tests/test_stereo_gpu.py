"""GPU parity of the stereo constructor (pslfe_frame_set_from_orb_stereo): mvuRight, mvDepth, the taps, mvKeysUn and the grid CSR
equal, bit for bit, the sequential restatement oracle/stereo_oracle.cpp fed with the extractor's keypoints and pyramid (and with
the CPU oracle's), plus the oracle's undistortion and grid; at the TUM1 (distorted), EuRoC and KITTI geometries, for one-pair
calls, 257-pair batches through one or two extractors, the edge cases of tests/stereo_scene.py, the device chain into
SearchByProjection, the argument checks and the compiled C++ consumer of host/pslfe.hpp."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import stereo_scene as ss
from oracle_lib import restate_stereo
from project_cases import T4, moved, restated_last, rot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLEVELS, SCALE = 8, 1.2
E_INVALID, E_CAPACITY, E_STATE = -1, -4, -5


def camera(vals):
    import psl_slam_amd as P
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, vals):
        cam[k] = np.float32(v)
    return cam


def expected(kL, dL, kR, dR, levL, levR, scale, inv, cam, w, h):
    """The restatement's mvuRight / mvDepth / taps, the oracle's UndistortKeyPoints, ComputeImageBounds and grid."""
    import oracle_lib
    ur, dep, idx, sad = restate_stereo(kL, dL, kR, dR, levL, levR, scale, inv, float(cam["bf"]), float(cam["fx"]))
    un, _, _ = oracle_lib.frame_post_rgbd(kL, np.zeros((h, w), np.float32), cam)
    start, gidx = oracle_lib.grid_build(un, oracle_lib.image_bounds(cam, w, h))
    return dict(uright=ur, depth=dep, idx=idx, sad=sad, kun=un, start=start, gidx=gidx)


def slot_outputs(g, slot):
    kun, dep, ur = g.fetch(slot)
    idx, sad = g.debug_stereo(slot)
    start, gidx = g.debug_grid(slot)
    return dict(uright=ur, depth=dep, idx=idx, sad=sad, kun=kun, start=start, gidx=gidx)


def assert_same(got, want, what):
    for k in ("uright", "depth", "idx", "sad", "kun", "start", "gidx"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: {k} differs"


def host_pair(left, right, nfeatures, cam, ctx=None):
    """The one-pair seam: two extractors, left(imLeft), right(imRight), then the stereo constructor into slot 0."""
    import psl_slam_amd as P
    h, w = left.shape
    oL = P.ORBextractor(nfeatures, SCALE, NLEVELS, 20, 7, ctx=ctx)
    oR = P.ORBextractor(nfeatures, SCALE, NLEVELS, 20, 7, ctx=ctx)
    kL, dL = oL(left)
    kR, dR = oR(right)
    g = P.FrameGrid(oL.max_keypoints(w, h), 1, ctx=ctx)
    g.set_from_orb_stereo(0, oL, 0, oR, 0, 1, cam)
    return g, oL, oR, (kL, dL, kR, dR)


def levels(orb, frame):
    return [orb.debug_level_image(frame, l) for l in range(NLEVELS)]


def factors(orb):
    return orb.GetScaleFactors().astype(np.float32), orb.GetInverseScaleFactors().astype(np.float32)


@pytest.mark.parametrize("geom", list(ss.GEOMETRIES))
def test_one_pair_equals_restatement_and_oracle(geom):
    import oracle_lib
    G = ss.GEOMETRIES[geom]
    w, h, cam = G["w"], G["h"], camera(G["cam"])
    left, right, _ = ss.scene_pair(w, h, float(cam["bf"]), G["zscale"], seed=3)
    g, oL, oR, (kL, dL, kR, dR) = host_pair(left, right, G["nfeatures"], cam)
    got = slot_outputs(g, 0)
    scale, inv = factors(oL)
    want = expected(kL, dL, kR, dR, levels(oL, 0), levels(oR, 0), scale, inv, cam, w, h)
    assert_same(got, want, f"{geom}: device keypoints and pyramids")
    acc = (got["sad"] >= 0).sum()
    assert len(kL) > 0.5 * G["nfeatures"] and acc > 0.3 * len(kL) and (got["depth"] > 0).sum() > 0.2 * len(kL), (len(kL), acc)
    if G["cam"][4] != 0:   # distorted camera: mvuRight stays in distorted coordinates, mvKeysUn moved
        assert (got["kun"]["x"] != kL["x"]).any()
    # the loop through the oracle: its keypoints and pyramids give the same outputs
    xL, xR = oracle_lib.OracleORB(G["nfeatures"], SCALE, NLEVELS, 20, 7), oracle_lib.OracleORB(G["nfeatures"], SCALE, NLEVELS, 20, 7)
    okL, odL = xL(left)
    okR, odR = xR(right)
    want_o = expected(okL, odL, okR, odR, [xL.level_image(l) for l in range(NLEVELS)], [xR.level_image(l) for l in range(NLEVELS)],
                      scale, inv, cam, w, h)
    assert_same(got, want_o, f"{geom}: oracle keypoints and pyramids")


@pytest.mark.parametrize("geom", list(ss.GEOMETRIES))
def test_edge_cases_equal_restatement(geom):
    G = ss.GEOMETRIES[geom]
    w, h, cam = G["w"], G["h"], camera(G["cam"])
    for name, (left, right) in ss.edge_cases(w, h).items():
        g, oL, oR, (kL, dL, kR, dR) = host_pair(left, right, G["nfeatures"], cam)
        got = slot_outputs(g, 0)
        scale, inv = factors(oL)
        want = expected(kL, dL, kR, dR, levels(oL, 0), levels(oR, 0), scale, inv, cam, w, h)
        assert_same(got, want, f"{geom}/{name}")
        if name == "flat_right":
            assert len(kR) == 0 and (got["idx"] == -1).all() and (got["uright"] == -1).all()
        if name == "flat_left":
            assert len(kL) == 0 and len(got["uright"]) == 0
        if name == "shift_int":
            assert (got["depth"] > 0).sum() > 0.2 * len(kL)


def _batch_images(w, h, bf, zscale, npairs, ndistinct=12):
    base = [ss.scene_pair(w, h, bf, zscale, style=("desk", "sticks")[k % 2], seed=100 + k, t=k % 3)[:2] for k in range(ndistinct)]
    L = np.stack([base[p % ndistinct][0] for p in range(npairs)], 0)
    R = np.stack([base[p % ndistinct][1] for p in range(npairs)], 0)
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


@pytest.mark.parametrize("geom", list(ss.GEOMETRIES))
def test_batch_one_and_two_handles_equal_per_pair_calls(geom):
    import torch
    import psl_slam_amd as P
    G = ss.GEOMETRIES[geom]
    w, h, cam, nf = G["w"], G["h"], camera(G["cam"]), G["nfeatures"]
    N = 257
    Ls, Rs = _batch_images(w, h, float(cam["bf"]), G["zscale"], N)
    dev = torch.device("cuda", 0)
    ctx = P.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    both = torch.from_numpy(np.concatenate([Ls, Rs], 0)).to(dev)       # one handle: lefts 0..N-1, rights N..2N-1
    o2 = P.ORBextractor(nf, SCALE, NLEVELS, 20, 7, ctx=ctx, max_batch=2 * N)
    o2.extract_batch_device(both.data_ptr(), 2 * N, w, h, w, w * h)
    cap = o2.max_keypoints(w, h)
    g1 = P.FrameGrid(cap, N + 3, ctx=ctx)
    g1.set_from_orb_stereo(3, o2, 0, o2, N, N, cam)                     # slots 3..N+2
    dL, dR = torch.from_numpy(Ls).to(dev), torch.from_numpy(Rs).to(dev)
    oa = P.ORBextractor(nf, SCALE, NLEVELS, 20, 7, ctx=ctx, max_batch=N)
    ob = P.ORBextractor(nf, SCALE, NLEVELS, 20, 7, ctx=ctx, max_batch=N)
    oa.extract_batch_device(dL.data_ptr(), N, w, h, w, w * h)
    ob.extract_batch_device(dR.data_ptr(), N, w, h, w, w * h)
    g2 = P.FrameGrid(cap, N, ctx=ctx)
    g2.set_from_orb_stereo(0, oa, 0, ob, 0, N, cam)
    torch.cuda.synchronize(dev)
    scale, inv = factors(oa)
    samples = sorted({0, 1, 2, 11, 12, N // 2, N - 2, N - 1})
    accepted = 0
    for p in range(N):
        a, b = slot_outputs(g1, 3 + p), slot_outputs(g2, p)
        assert_same(a, b, f"{geom} pair {p}: one handle vs two")
        accepted += int((a["sad"] >= 0).sum())
        if p in samples:
            kL, dLp = oa.fetch(p, w, h)
            kR, dRp = ob.fetch(p, w, h)
            want = expected(kL, dLp, kR, dRp, levels(oa, p), levels(ob, p), scale, inv, cam, w, h)
            assert_same(a, want, f"{geom} pair {p}: batch vs restatement")
            gs, _, _, _ = host_pair(Ls[p], Rs[p], nf, cam, ctx=ctx)
            assert_same(a, slot_outputs(gs, 0), f"{geom} pair {p}: batch vs one-pair call")
    assert accepted > 0.05 * N * nf
    ctx.synchronize()


def test_device_chain_into_search_by_projection():
    """Stereo slots -> project_last_device (visual-odometry points from the stereo mvDepth) -> search_by_projection_last_device,
    against oracle/project_oracle.cpp fed with the stereo restatement's mvKeysUn / mvDepth / mvuRight and the sequential matcher oracle."""
    import torch
    import psl_slam_amd as P
    import oracle_lib
    G = ss.GEOMETRIES["euroc"]
    w, h, cam, nf = G["w"], G["h"], camera(G["cam"]), G["nfeatures"]
    B = 6
    pairs = [ss.scene_pair(w, h, float(cam["bf"]), G["zscale"], seed=21, t=t)[:2] for t in range(B)]
    imgs = np.ascontiguousarray(np.stack([p[0] for p in pairs] + [p[1] for p in pairs], 0))
    dev = torch.device("cuda", 0)
    ctx = P.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    orb = P.ORBextractor(nf, SCALE, NLEVELS, 20, 7, ctx=ctx, max_batch=2 * B)
    d_img = torch.from_numpy(imgs).to(dev)
    orb.extract_batch_device(d_img.data_ptr(), 2 * B, w, h, w, w * h)
    cap = orb.max_keypoints(w, h)
    g = P.FrameGrid(cap, B, ctx=ctx)
    g.set_from_orb_stereo(0, orb, 0, orb, B, B, cam)
    bounds = tuple(float(b) for b in g.image_bounds(cam, w, h))
    scale, inv = factors(orb)
    npairs = B - 1
    rng = np.random.default_rng(9)
    Tl = [T4(rot(*rng.normal(0, 0.03, 3)), rng.normal(0, 0.1, 3)) for _ in range(npairs)]
    Tc = [moved(T, rng.normal(0, 0.01, 3)) for T in Tl]
    poses = lambda Ts: torch.from_numpy(np.stack([P.pose(T) for T in Ts]).view(np.uint8)).to(dev)
    d_Tl, d_Tc = poses(Tl), poses(Tc)
    q = torch.zeros((npairs, cap, 32), dtype=torch.uint8, device=dev)
    qd = torch.zeros((npairs, cap, 32), dtype=torch.uint8, device=dev)
    ow = torch.zeros((npairs, cap), dtype=torch.int32, device=dev)
    nq = torch.zeros((npairs,), dtype=torch.int32, device=dev)
    match = torch.full((npairs, cap), -1, dtype=torch.int32, device=dev)
    nm = torch.zeros((npairs,), dtype=torch.int32, device=dev)
    g.project_last_device(0, npairs, d_Tl.data_ptr(), d_Tc.data_ptr(), 0, 0, cam, scale, 15.0, 35.0 * float(cam["bf"]) / float(cam["fx"]),
                          False, True, bounds, q.data_ptr(), qd.data_ptr(), ow.data_ptr(), nq.data_ptr(), cap)
    P.search_by_projection_last_device(g, 1, npairs, q.data_ptr(), qd.data_ptr(), nq.data_ptr(), cap, True, match.data_ptr(), nm.data_ptr())
    torch.cuda.synchronize(dev)
    Q = q.cpu().numpy().view(P.PROJQUERY_DTYPE).reshape(npairs, cap)
    QD, OW, NQ, MATCH, NM = qd.cpu().numpy(), ow.cpu().numpy(), nq.cpu().numpy(), match.cpu().numpy(), nm.cpu().numpy()
    restated = []
    for t in range(B):
        kL, dL = orb.fetch(t, w, h)
        kR, dR = orb.fetch(B + t, w, h)
        e = expected(kL, dL, kR, dR, levels(orb, t), levels(orb, B + t), scale, inv, cam, w, h)
        assert_same(slot_outputs(g, t), e, f"chain frame {t}")
        restated.append((e["kun"], e["depth"], e["uright"], dL))
    for p in range(npairs):
        rq, rqd, row = restated_last(restated[p], Tl[p], Tc[p], None, None, cam, scale, 15.0,
                                     np.float32(35.0 * float(cam["bf"]) / float(cam["fx"])), False, True, bounds)
        n = NQ[p]
        assert n == len(rq) and n > 50 and Q[p, :n].tobytes() == rq.tobytes(), f"pair {p}: query rows differ"
        assert (QD[p, :n] == rqd).all() and (OW[p, :n] == row).all()
        kun1, _, ur1, desc1 = restated[p + 1]
        rnm, rmatch, _ = oracle_lib.search_by_projection_last(kun1, desc1, ur1, bounds, rq, rqd, None, True)
        assert NM[p] == rnm and (MATCH[p, :n] == rmatch).all(), f"pair {p}: matches differ from the oracle"
        assert rnm > 0
    ctx.synchronize()


def test_error_paths():
    import psl_slam_amd as P
    L = P.lib()
    cam = camera(ss.TUM1)
    img = ss.textured(320, 240)

    def orb(w=320, h=240, scale=SCALE, nlevels=NLEVELS, ctx=None, nf=500):
        o = P.ORBextractor(nf, scale, nlevels, 20, 7, ctx=ctx)
        o(np.ascontiguousarray(img[:h, :w]))
        return o
    a, b = orb(), orb()
    g = P.FrameGrid(a.max_keypoints(320, 240), 2)
    c1 = np.ascontiguousarray(cam).reshape(1)
    call = lambda s0, l, l0, r, r0, n, f=g: L.pslfe_frame_set_from_orb_stereo(f._h, s0, l._h, l0, r._h, r0, n, P._ptr(c1))
    assert call(0, a, 0, b, 0, 1) == 0
    assert call(0, a, 0, orb(w=300), 0, 1) == E_INVALID                     # image size
    assert call(0, a, 0, orb(scale=1.19), 0, 1) == E_INVALID                # scale factors
    assert call(0, a, 0, orb(nlevels=7), 0, 1) == E_INVALID                 # levels
    assert call(0, a, 0, orb(ctx=P.Context(0)), 0, 1) == E_INVALID          # contexts
    assert call(0, a, 1, b, 0, 1) == E_INVALID and call(0, a, 0, b, 1, 1) == E_INVALID and call(0, a, -1, b, 0, 1) == E_INVALID
    assert call(0, a, 0, b, 0, 2) == E_INVALID                             # beyond the last batch
    assert call(0, a, 0, b, 0, 0) == E_INVALID and call(-1, a, 0, b, 0, 1) == E_INVALID
    assert call(2, a, 0, b, 0, 1) == E_CAPACITY                            # too few slots
    small = P.FrameGrid(16, 2)
    assert call(0, a, 0, b, 0, 1, small) == E_CAPACITY                     # extractor capacity > frame capacity
    fresh = P.ORBextractor(500, SCALE, NLEVELS, 20, 7)
    assert call(0, fresh, 0, b, 0, 1) == E_STATE                           # nothing extracted yet
    g.set(1, *a.fetch(0, 320, 240), (0.0, 0.0, 320.0, 240.0))
    n = C.c_int()
    assert L.pslfe_frame_debug_stereo(g._h, 1, None, None, 0, C.byref(n)) == E_STATE   # not a stereo slot
    assert L.pslfe_frame_debug_stereo(g._h, 0, None, None, 0, C.byref(n)) == E_CAPACITY and n.value > 0
    g.debug_stereo(0)


def test_cpp_consumer_equals_python_path(tmp_path):
    """tools/dropin/stereo_main.cpp: two pslfe::ORBextractor + FrameGrid::setStereo, built with g++ and run as a child process."""
    import psl_slam_amd as P
    exe = str(tmp_path / "stereo_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "stereo_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    G = ss.GEOMETRIES["kitti"]
    w, h, cam = G["w"], G["h"], camera(G["cam"])
    left, right, _ = ss.scene_pair(w, h, float(cam["bf"]), G["zscale"], seed=5)
    pair = str(tmp_path / "pair.bin")
    with open(pair, "wb") as f:
        np.array([w, h], np.int32).tofile(f)
        np.ascontiguousarray(cam).tofile(f)
        left.tofile(f)
        right.tofile(f)
    out = str(tmp_path / "out.bin")
    p = subprocess.run([exe, pair, str(G["nfeatures"]), out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    summary = json.loads(p.stdout.strip().splitlines()[-1])
    raw = open(out, "rb").read()
    n = int(np.frombuffer(raw[:4], np.int32)[0])
    kun = np.frombuffer(raw[4:4 + 28 * n], P.KEYPOINT_DTYPE)
    ur = np.frombuffer(raw[4 + 28 * n:4 + 32 * n], np.float32)
    dep = np.frombuffer(raw[4 + 32 * n:4 + 36 * n], np.float32)
    g, _, _, _ = host_pair(left, right, G["nfeatures"], cam)
    pk, pd, pu = g.fetch(0)
    assert n == summary["n"] == len(pk) and n > 0
    assert kun.tobytes() == pk.tobytes() and ur.tobytes() == pu.tobytes() and dep.tobytes() == pd.tobytes()
    assert (dep > 0).sum() > 0.2 * n
