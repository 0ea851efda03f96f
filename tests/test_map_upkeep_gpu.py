"""GPU parity of the map refresh with the restatement of tests/map_upkeep_cases.py, byte for byte: pslfe_kf_update_normal_and_depth and
pslfe_kf_line_update_average_dir (host and device forms, both layouts of the run-order sums), pslfe_kf_scene_median_depth, the refreshed
rows handed on to the projections that read them, and the C++ consumer tools/dropin/map_main.cpp."""
import ctypes as C
import functools
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import kf_project_cases as kc
import kf_scene as ks
import map_upkeep_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = ("walk", "tiled")


def _matcher(P, layout, ctx=None):
    kf = P.KeyFrameMatcher(ctx=ctx)
    kf.set_upkeep_sum(P.UPKEEP_SUM_TILED if layout == "tiled" else P.UPKEEP_SUM_WALK)
    return kf


@functools.lru_cache(maxsize=None)
def _point_case(M):
    case = mc.big_point_case() if M == "big" else mc.point_case(M)
    return case, mc.restate_points(*case[:6], mc.SCALE, case[6])


@functools.lru_cache(maxsize=None)
def _line_case(M):
    case = mc.big_line_case() if M == "big" else mc.line_case(M)
    return case, mc.restate_lines(*case[:6], mc.SCALE, case[6])


def _check_rows(got, want, rows, off, skip, pos):
    live = (np.diff(off) > 0) & (skip == 0)
    size = rows.dtype.itemsize
    bad = np.nonzero((got.view(np.uint8).reshape(-1, size) != want.view(np.uint8).reshape(-1, size)).any(1))[0]
    assert len(bad) == 0, (len(bad), bad[:5], got[bad[:3]], want[bad[:3]])
    assert got[~live].tobytes() == rows[~live].tobytes()           # untouched rows keep the canary
    for f in pos:
        assert got[f].tobytes() == rows[f].tobytes()               # the position is only read
    return live


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", mc.POINT_SIZES + ("big",))
def test_points_equal_restatement(M, layout):
    """M = 257 holds every run length (0, 1, 2, 3, 63, 64, 65, 200: around a wave, longer than a workgroup has threads) and more than one
    workgroup; "big" is 20 000 points with about 160 000 observations, whose runs cross the tiles of the tiled layout"""
    import psl_slam_amd as P
    (mp, off, okf, ce, rk, rl, skip), want = _point_case(M)
    if M == "big":
        assert len(mp) == 20000 and 150000 <= off[-1] <= 170000
    got = _matcher(P, layout).UpdateNormalAndDepth(mp, off, okf, ce, rk, rl, mc.SCALE, skip)
    live = _check_rows(got, want, mp, off, skip, ("x", "y", "z"))
    assert M == 1 or (live.any() and (~live).any())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M", mc.POINT_SIZES + ("big",))
def test_lines_equal_restatement(M, layout):
    import psl_slam_amd as P
    (ml, off, okf, ce, rk, rl, skip), want = _line_case(M)
    got = _matcher(P, layout).LineUpdateAverageDir(ml, off, okf, ce, rk, rl, mc.SCALE, skip)
    live = _check_rows(got, want, ml, off, skip, ("sp", "ep"))
    if M != 1:
        assert any((ml["sp"][i] == ml["ep"][i]).all() for i in np.nonzero(live)[0])


def test_without_skip_bytes_and_empty_calls():
    import psl_slam_amd as P
    mp, off, okf, ce, rk, rl, skip = mc.point_case(65)
    rl = np.where(rl < 0, 0, rl).astype(np.int32)                  # without skip bytes every reference of a run is read
    want = mc.restate_points(mp, off, okf, ce, rk, rl, mc.SCALE, None)
    kf = P.KeyFrameMatcher()
    assert kf.UpdateNormalAndDepth(mp, off, okf, ce, rk, rl, mc.SCALE).tobytes() == want.tobytes()
    assert want.tobytes() != mc.restate_points(mp, off, okf, ce, rk, rl, mc.SCALE, skip).tobytes()
    assert len(kf.UpdateNormalAndDepth(mp[:0], off[:1], okf[:0], ce, rk[:0], rl[:0], mc.SCALE)) == 0
    assert len(kf.LineUpdateAverageDir(np.zeros(0, P.MAPLINE_DTYPE), off[:1], okf[:0], ce, rk[:0], rl[:0], mc.SCALE)) == 0
    assert len(kf.ComputeSceneMedianDepth(np.zeros(0, P.POSE_DTYPE), [], 2)) == 0
    bad = okf.copy()
    bad[3] = mc.NKF
    with pytest.raises(P.PslfeError, match="code -1.*obs_kf"):
        kf.UpdateNormalAndDepth(mp, off, bad, ce, rk, rl, mc.SCALE)
    with pytest.raises(P.PslfeError, match="code -1"):
        kf.set_upkeep_sum(2)


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


@pytest.mark.parametrize("layout", LAYOUTS)
def test_device_forms_equal_the_host_forms(layout):
    import psl_slam_amd as P
    ctx = P.default_context()
    kf = _matcher(P, layout, ctx)
    for case_of, host, device, dtype in ((_point_case, kf.UpdateNormalAndDepth, kf.update_normal_and_depth_device, P.MAPPOINT_DTYPE),
                                         (_line_case, kf.LineUpdateAverageDir, kf.line_update_average_dir_device, P.MAPLINE_DTYPE)):
        (rows, off, okf, ce, rk, rl, skip), want = case_of(257)
        ptrs = [_dev(ctx, a) for a in (rows, off, okf, ce, rk, rl, skip)]
        device(ptrs[0], len(rows), ptrs[1], ptrs[2], ptrs[3], len(ce), ptrs[4], ptrs[5], ptrs[6], mc.SCALE)
        ctx.synchronize()
        got = _down(P, ctx, ptrs[0], np.zeros(len(rows), dtype))
        assert got.tobytes() == host(rows, off, okf, ce, rk, rl, mc.SCALE, skip).tobytes() == want.tobytes()
        for d in ptrs:
            ctx.device_free(d)


# ---- a map whose refreshed rows mean something to the projections ---------------------------------------------------------------------

def _uright(kps, seed):
    rng = np.random.default_rng(seed)
    ur = (kps["x"] - np.float32(40.0) / rng.uniform(0.6, 6.0, len(kps)).astype(np.float32)).astype(np.float32)
    ur[rng.random(len(kps)) < 0.5] = -1.0
    return ur


@functools.lru_cache(maxsize=None)
def _world():
    """Three keyframes in a store, 24 neighbour views, 1200 map points: 500 that lie on the keypoints of view 4's keyframe and were
    created there (mpRefKF = view 4, the keypoint's octave), 700 elsewhere.  Every point is observed from 0..9 of the views; a tenth is
    bad.  The rows hold the geometry of an earlier state of the map; the refresh replaces it for the points it reaches."""
    (k0, d0), (k1, d1) = ks.keyframes()
    slots = [(k0, d0, _uright(k0, 1)), (k1, d1, _uright(k1, 2)), (k0[:600], d0[:600], _uright(k0[:600], 3))]
    views = kc.views(nslots=3)
    cam = kc.camera()
    rng = np.random.default_rng(29)
    k4, d4, _ = slots[int(views[4]["slot"])]
    on, _ = kc.points_onto(k4[:500], d4[:500], views[4], cam, kc.FUSE, rng)
    far, _ = kc.map_points(700, seed=31)
    mp = np.concatenate([on, far])
    M, nkf = len(mp), len(views)
    centres = np.stack([kc.centre(v["Tcw"]) for v in views]).astype(np.float32)
    lens = rng.integers(0, 10, M)
    lens[:500] = np.maximum(lens[:500], 1)
    off = np.zeros(M + 1, np.int32)
    off[1:] = np.cumsum(lens)
    okf = np.zeros(off[-1], np.int32)
    obs_desc = rng.integers(0, 256, (off[-1], 32), dtype=np.uint8)
    ref_kf, ref_level = np.full(M, -1, np.int32), rng.integers(0, kc.NLEVELS, M).astype(np.int32)
    for i in range(M):
        run = rng.permutation(nkf)[:lens[i]]
        if i < 500:
            run[rng.integers(0, lens[i])] = 4
            run = np.array(sorted(set(run.tolist())), np.int32)      # a std::map: every keyframe once
            run = np.concatenate([run, rng.permutation(np.setdiff1d(np.arange(nkf), run))[:lens[i] - len(run)]]).astype(np.int32)
            ref_kf[i], ref_level[i] = 4, k4["octave"][i]
            obs_desc[off[i]:off[i + 1]] = ks.noisy_desc(np.repeat(d4[i:i + 1], lens[i], 0), rng, flips=6)
        elif lens[i]:
            ref_kf[i] = run[rng.integers(0, lens[i])]
        okf[off[i]:off[i + 1]] = run
    bad = (rng.random(M) < 0.1).astype(np.uint8)
    return dict(slots=slots, views=views, cam=cam, mp=mp, off=off, okf=okf, obs_desc=obs_desc, centres=centres, ref_kf=ref_kf,
                ref_level=ref_level, bad=bad, fuse_skip=(kc.skip_bytes(nkf, M) | bad[None, :]).astype(np.uint8))


def _store(P, slots, ctx=None):
    g = P.FrameGrid(2048, len(slots), ctx=ctx)
    for s, (k, d, ur) in enumerate(slots):
        g.set(s, k, d, ks.BOUNDS, ur)
    return g


def _restated_world(W):
    return mc.restate_points(W["mp"], W["off"], W["okf"], W["centres"], W["ref_kf"], W["ref_level"], ks.SCALE, W["bad"])


def test_rows_refreshed_on_the_device_feed_the_projections():
    """device refresh -> pslfe_orb_project_frustum_device on the same array, and -> download -> pslfe_kf_fuse_keyframes: the rows and
    matches are those of the restated geometry handed to the same calls, and not those of the geometry before the refresh"""
    import psl_slam_amd as P
    W = _world()
    ctx = P.default_context()
    kf = P.KeyFrameMatcher(ctx=ctx)
    want = _restated_world(W)
    M, views, cam = len(want), W["views"], W["cam"]
    live = (np.diff(W["off"]) > 0) & (W["bad"] == 0)
    assert 900 < live.sum() < M and want[live].tobytes() != W["mp"][live].tobytes()
    d_mp = _dev(ctx, W["mp"])
    inputs = [_dev(ctx, W[k]) for k in ("off", "okf", "centres", "ref_kf", "ref_level", "bad")]
    kf.update_normal_and_depth_device(d_mp, M, inputs[0], inputs[1], inputs[2], len(views), inputs[3], inputs[4], inputs[5], ks.SCALE)
    # Frame::isInFrustum of every point from four of the poses, on the refreshed array and on an upload of the restated one
    nf = 4
    poses = np.ascontiguousarray(views["Tcw"][[2, 4, 9, 20]])
    mpdesc = np.random.default_rng(1).integers(0, 256, (M, 32), dtype=np.uint8)
    d_T, d_desc, d_nmp = _dev(ctx, poses), _dev(ctx, mpdesc), _dev(ctx, np.full(1, M, np.int32))
    d_want, d_before = _dev(ctx, want), _dev(ctx, W["mp"])
    d_q, d_qd, d_ow, d_nq = (_dev(ctx, np.zeros(s, t)) for s, t in ((M, P.PROJQUERY_DTYPE), ((M, 32), np.uint8), (M, np.int32), (1, np.int32)))
    out = []
    for d_rows in (d_mp, d_want, d_before):
        q, ow, nq = np.zeros((nf, M), P.PROJQUERY_DTYPE), np.zeros((nf, M), np.int32), np.zeros(nf, np.int32)
        for f in range(nf):                                         # one frame per call: every pose sees the one map
            P.project_frustum_device(1, d_T + f * P.POSE_DTYPE.itemsize, d_rows, d_desc, d_nmp, M, cam, ks.SCALE, kc.LOG_SCALE, 0.5, 1.0,
                                     ks.BOUNDS, d_q, d_qd, d_ow, d_nq, M, ctx=ctx)
            ctx.synchronize()
            _down(P, ctx, d_q, q[f])
            _down(P, ctx, d_ow, ow[f])
            nq[f] = _down(P, ctx, d_nq, np.zeros(1, np.int32))[0]
        out.append((q, ow, nq))
    for d in (d_q, d_qd, d_ow, d_nq):
        ctx.device_free(d)
    (q, ow, nq), (wq, wow, wnq), (bq, bow_, bnq) = out
    assert (nq == wnq).all() and nq.min() > 100
    for f in range(nf):
        assert q[f, :nq[f]].tobytes() == wq[f, :nq[f]].tobytes() and (ow[f, :nq[f]] == wow[f, :nq[f]]).all()
    assert any(bnq[f] != nq[f] or bq[f, :nq[f]].tobytes() != q[f, :nq[f]].tobytes() for f in range(nf))
    # ... and through a download into Fuse for the 24 neighbours
    got = _down(P, ctx, d_mp, np.zeros(M, P.MAPPOINT_DTYPE))
    assert got.tobytes() == want.tobytes()
    g = _store(P, W["slots"], ctx)
    fdesc = np.zeros((M, 32), np.uint8)
    fdesc[:500] = W["slots"][int(views[4]["slot"])][1][:500]
    args = (cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, 3.0, ks.INV_SIGMA2, W["fuse_skip"])
    a = kf.FuseKeyFrames(g, kc.FUSE, views, got, fdesc, *args)
    b = kf.FuseKeyFrames(g, kc.FUSE, views, want, fdesc, *args)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    rows, _, _ = kc.restate_project(kc.FUSE, views, want, cam, ks.BOUNDS, ks.SCALE, 3.0, W["fuse_skip"])
    assert a[2].tobytes() == rows.tobytes()
    assert (a[1][4][:500] <= 50).sum() > 200                        # the points created in view 4's keyframe are found there again
    for d in [d_mp, d_T, d_desc, d_nmp, d_want, d_before] + inputs:
        ctx.device_free(d)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 64, 65, 1000, 2049])
def test_scene_median_depth(K, n):
    import psl_slam_amd as P
    poses, xs = mc.median_case(K, n)
    kf = P.KeyFrameMatcher()
    for q in (1, 2, 3):
        got = kf.ComputeSceneMedianDepth(poses, xs, q)
        assert got.tobytes() == mc.restate_median(poses, xs, q).tobytes(), (K, n, q)
    if K == 3 and n >= 3:                                           # keyframes of different sizes in one call, an empty one among them
        xs = [xs[0][:n // 2], xs[1][:0], xs[2]]
        got = kf.ComputeSceneMedianDepth(poses, xs, 2)
        assert got.tobytes() == mc.restate_median(poses, xs, 2).tobytes() and got[1] == -1.0


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/map_main.cpp: distinctive descriptors, the refresh, Fuse on the refreshed rows and the median depths on pslfe.hpp,
    built with g++, run as a child process"""
    import oracle_lib
    import psl_slam_amd as P
    W = _world()
    views, cam, M = W["views"], W["cam"], len(W["mp"])
    K, q = len(views), 2
    exe = str(tmp_path / "map_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "map_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    rng = np.random.default_rng(41)
    med = [W["mp"][rng.random(M) < 0.3] for _ in range(K)]
    med[5] = med[5][:0]
    med_x = [np.stack([m["x"], m["y"], m["z"]], 1).astype(np.float32) for m in med]
    med_off = np.zeros(K + 1, np.int32)
    med_off[1:] = np.cumsum([len(x) for x in med_x])
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()
    blob = [struct.pack("<6i", len(W["slots"]), K, M, K, kc.NLEVELS, q), f32(ks.BOUNDS), np.ascontiguousarray(cam).tobytes(), f32(ks.SCALE),
            f32(ks.INV_SIGMA2), f32([kc.LOG_SCALE, 3.0])]
    for kps, d, ur in W["slots"]:
        blob += [struct.pack("<i", len(kps)), np.ascontiguousarray(kps).tobytes(), np.ascontiguousarray(d).tobytes(), f32(ur)]
    blob += [np.ascontiguousarray(a).tobytes() for a in (views, W["mp"], W["off"], W["okf"], W["obs_desc"], W["centres"], W["ref_kf"],
                                                        W["ref_level"], W["bad"], W["fuse_skip"], med_off, np.concatenate(med_x))]
    path, out = str(tmp_path / "map.bin"), str(tmp_path / "out.bin")
    with open(path, "wb") as fh:
        fh.write(b"".join(blob))
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    said = json.loads(p.stdout.strip().splitlines()[-1])
    with open(out, "rb") as fh:
        best = np.fromfile(fh, np.int32, M)
        mp = np.fromfile(fh, P.MAPPOINT_DTYPE, M)
        bi = np.fromfile(fh, np.int32, K * M).reshape(K, M)
        bd = np.fromfile(fh, np.int32, K * M).reshape(K, M)
        rows = np.fromfile(fh, P.PROJQUERY_DTYPE, K * M).reshape(K, M)
        depth = np.fromfile(fh, np.float32, K)
        assert fh.read() == b""
    want = _restated_world(W)
    assert mp.tobytes() == want.tobytes()
    kf = P.KeyFrameMatcher()
    assert (best == kf.ComputeDistinctiveDescriptors(W["obs_desc"], W["off"])).all() and (best[np.diff(W["off"]) == 0] == -1).all()
    mpdesc = np.zeros((M, 32), np.uint8)
    has = best >= 0
    mpdesc[has] = W["obs_desc"][W["off"][:-1][has] + best[has]]
    wrows, _, _ = kc.restate_project(kc.FUSE, views, want, cam, ks.BOUNDS, ks.SCALE, 3.0, W["fuse_skip"])
    assert rows.tobytes() == wrows.tobytes()
    fused = 0
    for k in range(K):
        kps, d, ur = W["slots"][int(views[k]["slot"])]
        obi, obd = oracle_lib.window_best(kps, d, ur, ks.BOUNDS, wrows[k], mpdesc, True, ks.INV_SIGMA2)
        np.testing.assert_array_equal(bi[k], obi)
        np.testing.assert_array_equal(np.where(bi[k] < 0, 0x7fffffff, bd[k]), np.where(obi < 0, 0x7fffffff, obd))
        fused += int((bd[k] <= 50).sum())
    poses = np.ascontiguousarray(views["Tcw"])
    assert depth.tobytes() == mc.restate_median(poses, med_x, q).tobytes() and depth[5] == -1.0
    live = (np.diff(W["off"]) > 0) & (W["bad"] == 0)
    assert said["points"] == M and said["refreshed"] == int(live.sum()) and said["fused"] == fused > 100
    assert np.allclose(said["depth"], depth, rtol=1e-5)
