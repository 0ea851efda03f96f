"""GPU parity of the device projection of map points into keyframes and of the three searches that chain it, through the C ABI:
pslfe_kf_project rows == the numpy restatement of tests/kf_project_cases.py byte for byte; pslfe_kf_fuse_keyframes,
pslfe_kf_search_by_sim3_poses and pslfe_kf_search_by_projection_sim3_pose == the oracle / restated searches on the restated rows, and ==
the existing entry points fed with those rows.  Every comparison is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

import kf_project_cases as kc
import kf_scene as ks
import loop_cases as lc

pytestmark = pytest.mark.gpu

TH = 3.0


@functools.lru_cache(maxsize=None)
def _points(M):
    return kc.map_points(M)


def _uright(kps, seed):
    """mvuRight: a right coordinate for about half of the keypoints"""
    rng = np.random.default_rng(seed)
    ur = (kps["x"] - np.float32(40.0) / rng.uniform(0.6, 6.0, len(kps)).astype(np.float32)).astype(np.float32)
    ur[rng.random(len(kps)) < 0.5] = -1.0
    return ur


def _store(P, ctx=None):
    """three keyframes in one frame store: the two of kf_scene and a prefix of the first; -> (grid, [(kps, desc, uright)])"""
    (k0, d0), (k1, d1) = ks.keyframes()
    slots = [(k0, d0, _uright(k0, 1)), (k1, d1, _uright(k1, 2)), (k0[:600], d0[:600], None)]
    g = P.FrameGrid(2048, 3, ctx=ctx)
    for s, (k, d, ur) in enumerate(slots):
        g.set(s, k, d, ks.BOUNDS, ur)
    return g, slots


@pytest.mark.parametrize("mode", [kc.FUSE, kc.SCW, kc.SIM3])
@pytest.mark.parametrize("K", [1, 24])
@pytest.mark.parametrize("M", [1, 1500, 5000])
@pytest.mark.parametrize("with_skip", [False, True])
def test_project_rows_equal_restatement(mode, K, M, with_skip):
    """M = 5000 is more than a slot's keypoint capacity: the projection does not depend on the store"""
    import psl_slam_amd as P
    views = kc.views()[:K] if K > 1 else kc.views()[5:6]
    mp, _ = _points(M)
    cam = kc.camera()
    skip = kc.skip_bytes(K, M) if with_skip else None
    want, wlevel, why = kc.restate_project(mode, views, mp, cam, ks.BOUNDS, ks.SCALE, TH, skip)
    if M >= 1500:
        assert (why == kc.KEPT).mean() > 0.3 and (why == kc.IMAGE).sum() > 0 and (why == kc.MAX_DIST).sum() > 0
    kf = P.KeyFrameMatcher()
    rows, level = kf.project(mode, views, mp, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, TH, skip)
    assert rows.shape == (K, M)
    np.testing.assert_array_equal(level, wlevel)
    bad = np.nonzero((rows.view(np.uint8).reshape(K, M, 32) != want.view(np.uint8).reshape(K, M, 32)).any(-1))
    assert len(bad[0]) == 0, (len(bad[0]), rows[bad][:3], want[bad][:3])
    assert rows.tobytes() == want.tobytes()
    rows2, level2 = kf.project(mode, views, mp, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, TH, skip)
    assert rows2.tobytes() == rows.tobytes() and level2.tobytes() == level.tobytes()


@pytest.mark.parametrize("mode", [kc.FUSE, kc.SCW, kc.SIM3])
def test_project_limit_cases(mode):
    import psl_slam_amd as P
    views, mp, names = kc.limit_cases()
    cam = kc.limit_camera()
    want, wlevel, why = kc.restate_project(mode, views, mp, cam, kc.LIMIT_BOUNDS, ks.SCALE, TH)
    if mode != kc.SIM3:
        assert [int(w) for w in why[0]] == [e for _, e in names]
    rows, level = P.KeyFrameMatcher().project(mode, views, mp, cam, kc.LIMIT_BOUNDS, ks.SCALE, kc.LOG_SCALE, TH)
    for i, (what, _) in enumerate(names):
        assert rows[:, i].tobytes() == want[:, i].tobytes() and (level[:, i] == wlevel[:, i]).all(), (what, rows[:, i], want[:, i])


@pytest.mark.parametrize("mode", [kc.FUSE, kc.SCW])
def test_fuse_keyframes(mode):
    """every keyframe of the set == the oracle's candidate loop on the restated rows (chi2 gates on for Fuse(pKF, vpMapPoints), off for
    Fuse(pKF, Scw, ...)) == a single call of pslfe_kf_window_best on those rows"""
    import oracle_lib
    import psl_slam_amd as P
    g, slots = _store(P)
    K, M = kc.NVIEWS, 1500
    views = kc.views(nslots=3)
    mp, desc = _points(M)
    # a third of the map really is in the keyframes: points that project onto keypoints of view 4's keyframe
    k4, d4, _ = slots[int(views[4]["slot"])]
    mp, desc = mp.copy(), desc.copy()
    on, ond = kc.points_onto(k4[:500], d4[:500], views[4], kc.camera(), mode, np.random.default_rng(3))
    mp[:500], desc[:500] = on, ond
    cam, skip = kc.camera(), kc.skip_bytes(K, M)
    chi2 = mode == kc.FUSE
    want, _, _ = kc.restate_project(mode, views, mp, cam, ks.BOUNDS, ks.SCALE, TH, skip)
    kf = P.KeyFrameMatcher()
    bi, bd, rows = kf.FuseKeyFrames(g, mode, views, mp, desc, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, TH, ks.INV_SIGMA2 if chi2 else None, skip)
    assert rows.tobytes() == want.tobytes()
    fused = 0
    for k in range(K):
        kps, d, ur = slots[int(views[k]["slot"])]
        obi, obd = oracle_lib.window_best(kps, d, ur, ks.BOUNDS, want[k], desc, chi2, ks.INV_SIGMA2)
        obd = np.where(obi < 0, 0x7fffffff, obd)
        np.testing.assert_array_equal(bi[k], obi)
        np.testing.assert_array_equal(np.where(bi[k] < 0, 0x7fffffff, bd[k]), obd)
        sbi, sbd = kf.window_best(g, int(views[k]["slot"]), want[k], desc, chi2, ks.INV_SIGMA2 if chi2 else None)
        np.testing.assert_array_equal(bi[k], sbi)
        np.testing.assert_array_equal(bd[k], sbd)
        fused += int((bd[k] <= 50).sum())
    assert (bd[4][:500] <= 50).sum() > 200 and fused > 300


def test_search_by_sim3_poses():
    import oracle_lib
    import psl_slam_amd as P
    g, slots = _store(P)
    (k0, d0, _), (k1, d1, _) = slots[0], slots[1]
    V = kc.views(nslots=3)
    cam = kc.camera()
    v12, v21 = V[3].copy(), V[8].copy()
    v12["slot"], v21["slot"] = 1, 0                                  # KF1's points are searched in KF2 (slot 1) and the other way round
    rng = np.random.default_rng(12)
    n = min(len(k0), len(k1))
    pair = rng.permutation(n)                                        # map point i1 of KF1 is KF2's keypoint pair[i1], for most
    mp1, desc1 = kc.map_points(len(k0), seed=21)
    mp2, desc2 = kc.map_points(len(k1), seed=22)
    a, ad = kc.points_onto(k1[pair], d1[pair], v12, cam, kc.SIM3, rng)
    inv = np.argsort(pair)
    b, bdsc = kc.points_onto(k0[inv], d0[inv], v21, cam, kc.SIM3, rng)
    real = rng.random(n) < 0.7
    mp1[:n][real], desc1[:n][real] = a[real], ad[real]
    mp2[:n][real[inv]], desc2[:n][real[inv]] = b[real[inv]], bdsc[real[inv]]
    skip1 = (rng.random(len(k0)) < 0.1).astype(np.uint8)
    skip2 = (rng.random(len(k1)) < 0.1).astype(np.uint8)
    th = 7.5
    q12, _, why12 = kc.restate_project(kc.SIM3, v12.reshape(1), mp1, cam, ks.BOUNDS, ks.SCALE, th, skip1.reshape(1, -1))
    q21, _, why21 = kc.restate_project(kc.SIM3, v21.reshape(1), mp2, cam, ks.BOUNDS, ks.SCALE, th, skip2.reshape(1, -1))
    onf, omatch = oracle_lib.search_by_sim3(k0, d0, ks.BOUNDS, k1, d1, ks.BOUNDS, q12[0], desc1, q21[0], desc2)
    assert onf > 100 and (why12 == kc.SKIP).sum() > 20 and (why21 != kc.KEPT).sum() > 50
    kf = P.KeyFrameMatcher()
    nf, match, r12, r21 = kf.SearchBySim3Poses(g, g, v12, mp1, desc1, skip1, v21, mp2, desc2, skip2, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, th)
    assert r12.tobytes() == q12[0].tobytes() and r21.tobytes() == q21[0].tobytes()
    np.testing.assert_array_equal(match, omatch)
    assert nf == onf
    enf, ematch = kf.SearchBySim3(g, 0, g, 1, q12[0], desc1, q21[0], desc2)
    np.testing.assert_array_equal(match, ematch)
    assert nf == enf


def test_search_by_projection_sim3_pose():
    import psl_slam_amd as P
    g, slots = _store(P)
    k, d, _ = slots[1]
    view = kc.views(nslots=3)[10].copy()
    view["slot"] = 1
    cam = kc.camera()
    rng = np.random.default_rng(17)
    rep = np.concatenate([rng.permutation(len(k)) for _ in range(3)])        # three map points per keypoint: they contend
    mp, desc = kc.points_onto(k[rep], d[rep], view, cam, kc.SCW, rng, noise_px=2.0, flips=30)
    far, fard = kc.map_points(300, seed=23)
    mp, desc = np.concatenate([mp, far]), np.concatenate([desc, fard])
    skip = (rng.random(len(mp)) < 0.1).astype(np.uint8)
    taken = (rng.random(len(k)) < 0.1).astype(np.uint8)
    th = 10.0
    want, _, why = kc.restate_project(kc.SCW, view.reshape(1), mp, cam, ks.BOUNDS, ks.SCALE, th, skip.reshape(1, -1))
    r = lc.restate_search_by_projection_sim3(k, d, ks.BOUNDS, want[0], desc, taken)
    assert r["nmatches"] > 200 and r["lost"] >= 20 and taken.sum() > 20 and (why != kc.KEPT).sum() > 100
    kf = P.KeyFrameMatcher()
    nm, match, assigned, rows = kf.SearchByProjectionSim3Pose(g, view, mp, desc, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, th, skip, taken)
    assert rows.tobytes() == want[0].tobytes()
    np.testing.assert_array_equal(match, r["match"])
    np.testing.assert_array_equal(assigned, r["assigned"])
    assert nm == r["nmatches"]
    enm, ematch, eassigned = kf.SearchByProjectionSim3(g, 1, want[0], desc, taken)
    np.testing.assert_array_equal(match, ematch)
    np.testing.assert_array_equal(assigned, eassigned)
    assert nm == enm


def test_empty_and_invalid_arguments():
    import psl_slam_amd as P
    g, slots = _store(P)
    kf = P.KeyFrameMatcher()
    views = kc.views(nslots=3)
    mp, desc = _points(1500)
    cam = kc.camera()
    args = (cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, TH)
    rows, level = kf.project(kc.FUSE, views[:0], mp, *args)
    assert rows.shape == (0, 1500) and level.shape == (0, 1500)
    rows, level = kf.project(kc.FUSE, views, mp[:0], *args)
    assert rows.shape == (24, 0)
    bi, bd, rows = kf.FuseKeyFrames(g, kc.SCW, views[:0], mp, desc, *args)
    assert bi.shape == (0, 1500)
    bi, bd, rows = kf.FuseKeyFrames(g, kc.SCW, views, mp[:0], desc[:0], *args)
    assert bi.shape == (24, 0)
    # K == 0 / M == 0 write nothing: outputs handed over keep their content
    lib = P.lib()
    q = np.full(4, 7, P.PROJQUERY_DTYPE)
    lv = np.full(4, 7, np.int32)
    v = np.ascontiguousarray(views)
    camr = np.ascontiguousarray(cam).reshape(1)
    sf = np.ascontiguousarray(ks.SCALE, np.float32)
    tail = (C.c_void_p(camr.ctypes.data), *[C.c_float(b) for b in ks.BOUNDS], C.c_void_p(sf.ctypes.data))
    lsf, th = C.c_float(kc.LOG_SCALE), C.c_float(TH)
    vp, mpp = C.c_void_p(v.ctypes.data), C.c_void_p(mp.ctypes.data)
    assert lib.pslfe_kf_project(kf._h, 0, vp, 0, mpp, None, 4, *tail, 8, lsf, th, C.c_void_p(q.ctypes.data), C.c_void_p(lv.ctypes.data)) == 0
    assert lib.pslfe_kf_project(kf._h, 0, vp, 4, mpp, None, 0, *tail, 8, lsf, th, C.c_void_p(q.ctypes.data), C.c_void_p(lv.ctypes.data)) == 0
    assert (lv == 7).all() and (q["blocks"] == 7).all()
    # PSLFE_E_INVALID: NULL output, mode, nlevels, a slot outside the store, chi2 gates without mvInvLevelSigma2
    assert lib.pslfe_kf_project(kf._h, 0, vp, 1, mpp, None, 4, *tail, 8, lsf, th, None, None) == -1
    assert lib.pslfe_kf_project(kf._h, 3, vp, 1, mpp, None, 4, *tail, 8, lsf, th, C.c_void_p(q.ctypes.data), None) == -1
    assert b"mode" in lib.pslfe_last_error()
    for nl in (0, 17):
        assert lib.pslfe_kf_project(kf._h, 0, vp, 1, mpp, None, 4, *tail, nl, lsf, th, C.c_void_p(q.ctypes.data), None) == -1
        assert b"nlevels" in lib.pslfe_last_error()
    with pytest.raises(P.PslfeError, match="code -1"):
        kf.FuseKeyFrames(g, kc.SIM3, views, mp, desc, *args)
    with pytest.raises(P.PslfeError, match="code -1.*mvInvLevelSigma2"):
        kf.FuseKeyFrames(g, kc.FUSE, views, mp, desc, *args)
    out = views.copy()
    out["slot"][7] = 3
    with pytest.raises(P.PslfeError, match="code -1.*slot 3"):
        kf.FuseKeyFrames(g, kc.SCW, out, mp, desc, *args)
    out["slot"][7] = -1
    with pytest.raises(P.PslfeError, match="code -1"):
        kf.SearchByProjectionSim3Pose(g, out[7], mp, desc, *args)
    with pytest.raises(P.PslfeError, match="code -1"):
        kf.SearchBySim3Poses(g, g, out[7], mp, desc, None, out[6], mp, desc, None, *args)


def test_matcher_of_a_second_context_reads_the_first_contexts_store():
    """the KeyFrame-rate matchers run on their own thread's context while Tracking's context owns the frame store"""
    import psl_slam_amd as P
    g, slots = _store(P)
    g.ctx.synchronize()
    other = P.Context(0)
    views = kc.views(nslots=3)
    mp, desc = _points(1500)
    args = (kc.camera(), ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, TH)
    a = P.KeyFrameMatcher().FuseKeyFrames(g, kc.FUSE, views, mp, desc, *args, ks.INV_SIGMA2)
    b = P.KeyFrameMatcher(ctx=other).FuseKeyFrames(g, kc.FUSE, views, mp, desc, *args, ks.INV_SIGMA2)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[1] <= 50).sum() > 0
