"""GPU parity of the pose optimisation with LIL edges (psl-slam_amd/csrc/pslfe_pose.hip, k_pose_optimize<true>) with the restatement
of tests/pose_lil_cases.py in the device's order of the sums, bit for bit: pose floats, both outlier arrays, return value, rounds and
iterations; the host form, nlil = 0 against the point-edge entry point, a batch against single launches, the error rules, the LIL
set-up loop and the chain glue -> LIL edges -> pose on a glue_scene frame, and the C++ consumer tools/dropin/pose_main.cpp on LIL cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_lil_cases as lc
import pose_opt_cases as pc
from test_pose_lil_cpu import ORDER_DIFFERENCE, assert_equal_ref, read_section, write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# four times the CPU-measured difference between the two orders of the restatement (tests/test_pose_lil_cpu.py), the margin and the
# reasoning of tests/test_pose_opt_gpu.py
ORDER_BOUND = 4 * ORDER_DIFFERENCE


def _cam(P, c=None):
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in (c or pc.camera()).items():
        cam[k] = v
    return cam


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _run_device(P, ctx, cases, estride=None, lstride=None, alias=False, counts=None, lcounts=None, cam=None):
    """the cases as one launch -> [(pose, outlier, outlier_lil, ngood, info)]; both kinds of outlier bytes start as 0xAA"""
    K = len(cases)
    estride = estride or max(max(len(c["edges"]) for c in cases), 1)
    lstride = lstride or max(max(len(c["lil"]) for c in cases), 1)
    T = np.zeros(K, P.POSE_DTYPE)
    E, L = np.zeros((K, estride), P.POSEEDGE_DTYPE), np.zeros((K, lstride), P.POSELIL_DTYPE)
    n, m = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for k, c in enumerate(cases):
        T[k] = c["Tcw"]
        a, b = min(len(c["edges"]), estride), min(len(c["lil"]), lstride)
        E[k, :a], L[k, :b] = c["edges"][:a], c["lil"][:b]
        n[k] = len(c["edges"]) if counts is None else counts[k]
        m[k] = len(c["lil"]) if lcounts is None else lcounts[k]
    d_T, d_E, d_L, d_n, d_m = _dev(ctx, T), _dev(ctx, E), _dev(ctx, L), _dev(ctx, n), _dev(ctx, m)
    d_To = d_T if alias else _dev(ctx, np.zeros(K, P.POSE_DTYPE))
    d_o, d_ol = _dev(ctx, np.full((K, estride), 0xAA, np.uint8)), _dev(ctx, np.full((K, lstride), 0xAA, np.uint8))
    d_g, d_i = _dev(ctx, np.full(K, -99, np.int32)), _dev(ctx, np.zeros(K, P.POSEINFO_DTYPE))
    P.Optimizer.PoseOptimizationLilDevice(K, d_T, d_E, d_n, estride, d_L, d_m, lstride, cam if cam is not None else _cam(P), d_To, d_o, d_ol, d_g,
                                          d_i, ctx=ctx)
    ctx.synchronize()
    To, o = _down(P, ctx, d_To, np.zeros(K, P.POSE_DTYPE)), _down(P, ctx, d_o, np.zeros((K, estride), np.uint8))
    ol = _down(P, ctx, d_ol, np.zeros((K, lstride), np.uint8))
    g, i = _down(P, ctx, d_g, np.zeros(K, np.int32)), _down(P, ctx, d_i, np.zeros(K, P.POSEINFO_DTYPE))
    for d in {d_T, d_E, d_L, d_n, d_m, d_To, d_o, d_ol, d_g, d_i}:
        ctx.device_free(d)
    return [(To[k], o[k, :min(len(c["edges"]), estride)], ol[k, :min(len(c["lil"]), lstride)], int(g[k]), i[k]) for k, c in enumerate(cases)]


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]


@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_device_and_host_forms_equal_restatement(name):
    """totals of 2, 3, 9 and 10 edges made up with LIL edges; LIL edges alone at 3, 64, 65; LIL indices across the 256 boundary
    (250 + 10, 257 + 3); point rows in LDS (2048 + 4) and in HBM (2100 + 4); 40 + 512; every LIL edge an outlier; the edges of the
    set-up loop with bad and missing planes; 0 % and 30 % planted outliers"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = lc.case(name)
    ref = c["ref"]["device"]
    got = _run_device(P, ctx, [c])[0]
    print(name, "ngood", got[3], "rounds", got[4], "pose", pc.pose_floats(got[0]))
    assert_equal_ref(got, ref, name)
    if ref[1] is None:
        assert (got[1] == 0xAA).all() and (got[2] == 0xAA).all()        # fewer than 3 edges in all: no byte of either kind is written
    ngood, pose, outlier, outlier_lil = P.Optimizer.PoseOptimization(c["Tcw"], c["edges"], _cam(P), ctx=ctx, lil=c["lil"])
    assert ngood == got[3] and pose.tobytes() == got[0].tobytes()
    assert (outlier == (got[1] if ref[1] is not None else 0)).all() and (outlier_lil == (got[2] if ref[1] is not None else 0)).all()
    # against g2o's edge order: the same decisions, the pose within the bound
    edge = c["ref"]["edge"]
    assert got[3] == edge[3] and (edge[1] is None or ((got[1] == edge[1]).all() and (got[2] == edge[2]).all()))
    d = np.abs(pc.pose_floats(got[0]).astype(np.float64) - pc.pose_floats(edge[0]).astype(np.float64)).max()
    print(name, "difference to the edge order", d)
    assert d <= ORDER_BOUND, (name, d)


@pytest.mark.parametrize("name", ["n10_mixed_30", "n257_stereo_30", "n2100_mixed_30"])
def test_without_lil_edges_the_bits_are_those_of_the_point_entry_point(name):
    import psl_slam_amd as P
    ctx = P.default_context()
    c = dict(pc.case(name))
    c["lil"] = np.zeros(0, P.POSELIL_DTYPE)
    got = _run_device(P, ctx, [c])[0]
    n = len(c["edges"])
    d_T, d_E, d_n = _dev(ctx, np.array([c["Tcw"]])), _dev(ctx, c["edges"]), _dev(ctx, np.array([n], np.int32))
    d_o, d_g, d_i = _dev(ctx, np.full(n, 0xAA, np.uint8)), _dev(ctx, np.zeros(1, np.int32)), _dev(ctx, np.zeros(1, P.POSEINFO_DTYPE))
    P.Optimizer.PoseOptimizationDevice(1, d_T, d_E, d_n, n, _cam(P), d_T, d_o, d_g, d_i, ctx=ctx)
    ctx.synchronize()
    T, o = _down(P, ctx, d_T, np.zeros(1, P.POSE_DTYPE))[0], _down(P, ctx, d_o, np.zeros(n, np.uint8))
    g, i = int(_down(P, ctx, d_g, np.zeros(1, np.int32))[0]), _down(P, ctx, d_i, np.zeros(1, P.POSEINFO_DTYPE))[0]
    for d in (d_T, d_E, d_n, d_o, d_g, d_i):
        ctx.device_free(d)
    assert got[0].tobytes() == T.tobytes() and got[1].tobytes() == o.tobytes() and got[3] == g and got[4].tobytes() == i.tobytes()
    ref = c["ref"]["device"]
    assert T.tobytes() == ref[0].tobytes() and g == ref[2]
    # lstride = 0 with NULL LIL arrays is the same call
    d_T, d_E, d_n, d_m = _dev(ctx, np.array([c["Tcw"]])), _dev(ctx, c["edges"]), _dev(ctx, np.array([n], np.int32)), _dev(ctx, np.zeros(1, np.int32))
    d_o, d_g = _dev(ctx, np.zeros(n, np.uint8)), _dev(ctx, np.zeros(1, np.int32))
    P.Optimizer.PoseOptimizationLilDevice(1, d_T, d_E, d_n, n, 0, d_m, 0, _cam(P), d_T, d_o, 0, d_g, ctx=ctx)
    ctx.synchronize()
    assert _down(P, ctx, d_T, np.zeros(1, P.POSE_DTYPE))[0].tobytes() == T.tobytes()
    for d in (d_T, d_E, d_n, d_m, d_o, d_g):
        ctx.device_free(d)


def test_batch_equals_single_launches_and_poses_may_alias():
    """K = 5 mixed frames in one launch (one below 3 edges in all, one without LIL edges, one without points), out of place and in
    place, reversed and with other strides"""
    import psl_slam_amd as P
    ctx = P.default_context()
    names = ["p250_l10", "p2_l0", "p2048_l4", "p0_l65"]
    cases = [lc.case(nm) for nm in names]
    nolil = dict(pc.case("n65_mixed_0_behind"))
    nolil["lil"] = np.zeros(0, P.POSELIL_DTYPE)
    cases[1:1] = [nolil]
    single = [_run_device(P, ctx, [c], estride=2048, lstride=65)[0] for c in cases]
    for alias in (False, True):
        batch = _run_device(P, ctx, cases, estride=2048, lstride=65, alias=alias)
        for b, s in zip(batch, single):
            assert _same(b, s) and b[4].tobytes() == s[4].tobytes()
    for c, s in zip(cases, single):
        if "ref" in c and len(c["ref"]["device"]) == 5:
            assert_equal_ref(s, c["ref"]["device"], "single")
    rev = _run_device(P, ctx, cases[::-1], estride=2100, lstride=80)[::-1]
    for b, s in zip(rev, single):
        assert _same(b, s)


def test_a_count_above_either_stride_is_reported():
    import psl_slam_amd as P
    ctx = P.default_context()
    cases = [lc.case("p63_l30"), lc.case("p0_l65"), lc.case("p2_l7")]
    got = _run_device(P, ctx, cases, estride=64, lstride=64, counts=[65, 0, 2], lcounts=[30, 65, 7])
    for k in (0, 1):     # the point count above estride; the LIL count above lstride
        assert got[k][3] == -4 and got[k][0].tobytes() == cases[k]["Tcw"].tobytes() and got[k][4]["rounds"] == 0
        assert (got[k][1] == 0xAA).all() and (got[k][2] == 0xAA).all()
    assert_equal_ref(got[2], cases[2]["ref"]["device"], "p2_l7")


def test_a_negative_count_of_either_kind_is_reported():
    """a negative point or LIL count (an error code left by the set-up loop, for instance) is answered with PSLFE_E_INVALID: the pose
    is copied and no outlier byte is written; the frame next to it is optimised as usual"""
    import psl_slam_amd as P
    ctx = P.default_context()
    cases = [lc.case("p63_l30"), lc.case("p63_l30"), lc.case("p2_l7")]
    got = _run_device(P, ctx, cases, counts=[63, -1, 2], lcounts=[-4, 30, 7])
    for k in (0, 1):
        assert got[k][3] == -1 and got[k][0].tobytes() == cases[k]["Tcw"].tobytes() and got[k][4]["rounds"] == 0
        assert (got[k][1] == 0xAA).all() and (got[k][2] == 0xAA).all()
    assert_equal_ref(got[2], cases[2]["ref"]["device"], "p2_l7")


def test_more_planes_than_either_stride_holds_are_reported():
    """the set-up loop with a plane count above le_stride (frame 0) and above plane_stride (frame 1): d_nlil = PSLFE_E_CAPACITY and
    no row of those frames is written; frame 2 is within both and gives its edges"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = lc.case("setup")
    npl, ncr = len(c["cross2d"]), len(c["le_l"])
    le, c2, idx = np.zeros((3, ncr, 6)), np.zeros((3, npl, 2)), np.full((3, npl), -1, np.int32)
    le[:], c2[:], idx[:] = c["le_l"], c["cross2d"], c["lil_index"]
    for le_stride, plane_stride, counts in ((npl - 1, npl, [npl, npl - 1]), (ncr, npl, [npl + 1, npl])):
        d_le, d_c2, d_idx, d_map = _dev(ctx, le[:2, :le_stride].copy()), _dev(ctx, c2[:2]), _dev(ctx, idx[:2]), _dev(ctx, c["lil_map"])
        d_np, d_l, d_nl = _dev(ctx, np.array(counts, np.int32)), _dev(ctx, np.zeros((2, 16), P.POSELIL_DTYPE)), _dev(ctx, np.zeros(2, np.int32))
        P.Optimizer.LilEdgesDevice(2, d_le, le_stride, d_c2, plane_stride, d_np, d_idx, d_map, len(c["lil_map"]), d_l, 0, d_nl, 16, ctx=ctx)
        ctx.synchronize()
        nl, l = _down(P, ctx, d_nl, np.zeros(2, np.int32)), _down(P, ctx, d_l, np.zeros((2, 16), P.POSELIL_DTYPE))
        want, _ = lc.lil_edges(c["le_l"][:le_stride], c["cross2d"][:counts[1]], c["lil_index"], c["lil_map"])
        assert nl[0] == -4 and l[0].tobytes() == np.zeros(16, P.POSELIL_DTYPE).tobytes()
        assert nl[1] == len(want) and l[1, :len(want)].tobytes() == want.tobytes()
        for d in (d_le, d_c2, d_idx, d_map, d_np, d_l, d_nl):
            ctx.device_free(d)


def test_below_three_edges_in_all_nothing_is_written():
    import psl_slam_amd as P
    ctx = P.default_context()
    c = lc.case("p2_l1")
    for n, m in ((2, 0), (1, 1), (0, 2), (0, 0)):
        sub = {"Tcw": c["Tcw"], "edges": c["edges"][:n], "lil": np.concatenate([c["lil"], c["lil"]])[:m]}
        got = _run_device(P, ctx, [sub], estride=4, lstride=4, counts=[n], lcounts=[m])[0]
        assert got[3] == 0 and got[0].tobytes() == c["Tcw"].tobytes() and got[4]["rounds"] == 0
    K = 1
    d_T, d_E, d_L = _dev(ctx, np.array([c["Tcw"]])), _dev(ctx, np.zeros(4, P.POSEEDGE_DTYPE)), _dev(ctx, np.zeros(4, P.POSELIL_DTYPE))
    d_n, d_m = _dev(ctx, np.array([1], np.int32)), _dev(ctx, np.array([1], np.int32))
    d_o, d_ol, d_g = _dev(ctx, np.full(4, 0xAA, np.uint8)), _dev(ctx, np.full(4, 0xAA, np.uint8)), _dev(ctx, np.zeros(1, np.int32))
    P.Optimizer.PoseOptimizationLilDevice(K, d_T, d_E, d_n, 4, d_L, d_m, 4, _cam(P), d_T, d_o, d_ol, d_g, ctx=ctx)
    ctx.synchronize()
    assert (_down(P, ctx, d_o, np.zeros(4, np.uint8)) == 0xAA).all() and (_down(P, ctx, d_ol, np.zeros(4, np.uint8)) == 0xAA).all()
    for d in (d_T, d_E, d_L, d_n, d_m, d_o, d_ol, d_g):
        ctx.device_free(d)
    ngood, pose, outlier, outlier_lil = P.Optimizer.PoseOptimization(c["Tcw"], c["edges"][:1], _cam(P), ctx=ctx, lil=c["lil"][:1])
    assert ngood == 0 and pose.tobytes() == c["Tcw"].tobytes() and not outlier.any() and not outlier_lil.any()


def test_error_codes():
    import psl_slam_amd as P
    ctx = P.default_context()
    L = P.lib()
    cam = np.zeros(1, P.CAMERA_DTYPE)
    d = _dev(ctx, np.zeros(256, np.int32))
    p, null, i = C.c_void_p(d), C.c_void_p(None), C.c_int
    f = L.pslfe_pose_optimize_lil_device
    assert f(ctx._h, i(1), p, p, p, i(1), p, p, i(-1), P._ptr(cam), p, p, p, p, null) == -1
    assert f(ctx._h, i(0), null, null, null, i(1), null, null, i(1), P._ptr(cam), null, null, null, null, null) == 0
    for bad in range(9):
        a = [p] * 9
        a[bad] = null
        assert f(ctx._h, i(1), a[0], a[1], a[2], i(1), a[3], a[4], i(1), P._ptr(cam), a[5], a[6], a[7], a[8], null) == -1, bad
    T, e, l = np.zeros(1, P.POSE_DTYPE), np.zeros(4, P.POSEEDGE_DTYPE), np.zeros(4, P.POSELIL_DTYPE)
    o, ng = np.zeros(4, np.uint8), C.c_int()
    h = L.pslfe_pose_optimize_lil
    assert h(ctx._h, P._ptr(T), P._ptr(e), i(4), P._ptr(l), i(-1), P._ptr(cam), P._ptr(T), P._ptr(o), P._ptr(o), C.byref(ng)) == -1
    assert h(ctx._h, P._ptr(T), P._ptr(e), i(4), None, i(4), P._ptr(cam), P._ptr(T), P._ptr(o), P._ptr(o), C.byref(ng)) == -1
    assert h(ctx._h, P._ptr(T), P._ptr(e), i(4), P._ptr(l), i(4), P._ptr(cam), P._ptr(T), P._ptr(o), None, C.byref(ng)) == -1
    g = L.pslfe_pose_lil_edges_device
    assert g(ctx._h, i(1), p, i(4), p, i(4), p, p, p, i(2), p, null, p, i(-1)) == -1
    assert g(ctx._h, i(1), p, i(4), p, i(4), null, p, p, i(2), p, null, p, i(4)) == -1
    assert g(ctx._h, i(1), p, i(4), p, i(4), p, null, p, i(2), p, null, p, i(4)) == -1
    assert g(ctx._h, i(1), p, i(4), p, i(4), p, p, null, i(2), p, null, p, i(4)) == -1
    assert g(ctx._h, i(0), null, i(4), null, i(4), null, null, null, i(2), null, null, null, i(4)) == 0
    ctx.device_free(d)


# ---- the set-up loop and the chain on glue_scene frames -------------------------------------------------------------------------------
def _glue_batch(P, ctx):
    """two glue_scene frames through pslfe_glue_run_batch_device -> (glue, fetched results per frame, cam, device arrays to free)"""
    import glue_scene
    F, ML, MF = 2, 64, 128
    scenes = [glue_scene.scene(seed=10 + f, nlines=50 + f, nfans=100 + 5 * f) for f in range(F)]
    kls, fans = np.zeros((F, ML), P.KEYLINE_DTYPE), np.zeros((F, MF, 4), np.float32)
    nkl, nfans = np.zeros(F, np.int32), np.zeros(F, np.int32)
    depth = np.zeros((F, glue_scene.H, glue_scene.W), np.float32)
    for f, (k, fa, d, cam, _) in enumerate(scenes):
        kls[f, :len(k)], fans[f, :len(fa)], depth[f] = k, fa, d
        nkl[f], nfans[f] = len(k), len(fa)
    dev = [_dev(ctx, a) for a in (kls, fans, nkl, nfans, depth)]
    g = P.FrameGlue(max_lines=ML, max_fans=MF, max_batch=F, ctx=ctx)
    g.run_batch_device(F, dev[0], ML, dev[2], dev[1], MF, dev[3], dev[4], glue_scene.W, glue_scene.H, scenes[0][3], seed0=7)
    res = [g.fetch(f, int(nkl[f])) for f in range(F)]
    return g, res, scenes[0][3], dev


def _map_lils(rng, res, nmap):
    """a map of LILs for the planes of every frame (the plane's own two 3-D lines and crossing, as the camera of an identity pose
    sees them) in a shuffled order, and lil_index per frame with a missing (-1), an outside and a bad entry"""
    lil_map = np.zeros(nmap, lc.MAPLIL_DTYPE)
    lil_map["w"] = rng.normal(size=(nmap, 15)) + np.array([0, 0, 3.0] * 5)
    rows = rng.permutation(nmap)
    index, k = [], 0
    for r in res:
        idx = np.full(len(r["planes"]), -1, np.int32)
        for i in range(len(idx)):
            a, b = r["lineNo"][i]
            lil_map["w"][rows[k]] = np.concatenate([r["lines3d"][a], r["lines3d"][b], r["cross3d"][i]])
            idx[i] = rows[k]
            k += 1
        index.append(idx)
    index[0][2], index[0][6], index[1][0], index[1][9] = -1, nmap, -3, nmap + 5
    lil_map["bad"][index[0][4]] = 1
    lil_map["bad"][index[1][11]] = 1
    return lil_map, index


def test_lil_edges_equal_the_restated_set_up_loop():
    """two glue_scene frames (81 and 78 crossings, 14 and 17 planes: plane i is not crossing i), map LILs in a shuffled order with
    missing (-1), outside and bad entries; then lstride below the count: the overflow is reported and the first rows are written"""
    import psl_slam_amd as P
    ctx = P.default_context()
    g, res, cam, dev = _glue_batch(P, ctx)
    rng = np.random.default_rng(9)
    nmap = 40
    lil_map, index = _map_lils(rng, res, nmap)
    v = g.lil_obs_device()
    assert v["le_stride"] == 128 and v["plane_stride"] == 128
    ncross, nplanes = _down(P, ctx, v["ncross"], np.zeros(2, np.int32)), _down(P, ctx, v["nplanes"], np.zeros(2, np.int32))
    assert [len(r["le_l"]) for r in res] == list(ncross) and [len(r["planes"]) for r in res] == list(nplanes)
    assert all(len(r["le_l"]) > len(r["planes"]) > 12 for r in res)
    assert any((r["pair"][:len(r["lineNo"])] != r["lineNo"]).any() for r in res)            # plane i is not crossing i
    idx = np.full((2, v["plane_stride"]), -1, np.int32)
    for f in range(2):
        idx[f, :len(index[f])] = index[f]
    d_idx, d_map = _dev(ctx, idx), _dev(ctx, lil_map)
    want = [lc.lil_edges(r["le_l"], r["cross2d"], index[f], lil_map) for f, r in enumerate(res)]
    assert [len(w[0]) for w in want] == [len(res[0]["planes"]) - 3, len(res[1]["planes"]) - 3]
    for lstride in (32, 8):
        d_l, d_pl, d_nl = _dev(ctx, np.zeros((2, lstride), P.POSELIL_DTYPE)), _dev(ctx, np.full((2, lstride), -1, np.int32)), _dev(ctx, np.zeros(2, np.int32))
        P.Optimizer.LilEdgesDevice(2, v["le_l"], v["le_stride"], v["cross2d"], v["plane_stride"], v["nplanes"], d_idx, d_map, nmap, d_l, d_pl, d_nl,
                                   lstride, ctx=ctx)
        ctx.synchronize()
        l, pl, nl = _down(P, ctx, d_l, np.zeros((2, lstride), P.POSELIL_DTYPE)), _down(P, ctx, d_pl, np.zeros((2, lstride), np.int32)), _down(P, ctx, d_nl, np.zeros(2, np.int32))
        for f, (we, wp) in enumerate(want):
            assert nl[f] == len(we)                                                     # the full count, also above lstride
            k = min(len(we), lstride)
            assert l[f, :k].tobytes() == we[:k].tobytes() and (pl[f, :k] == wp[:k]).all() and (pl[f, k:] == -1).all()
        assert lstride == 32 or (nl > lstride).all()
        for d in (d_l, d_pl, d_nl):
            ctx.device_free(d)
    # without d_edge_plane, one frame, the second
    d_l, d_nl = _dev(ctx, np.zeros(32, P.POSELIL_DTYPE)), _dev(ctx, np.zeros(1, np.int32))
    P.Optimizer.LilEdgesDevice(1, v["le_l"] + 128 * 48, 128, v["cross2d"] + 128 * 16, 128, v["nplanes"] + 4, d_idx + 128 * 4, d_map, nmap, d_l, 0, d_nl, 32,
                               ctx=ctx)
    ctx.synchronize()
    assert _down(P, ctx, d_nl, np.zeros(1, np.int32))[0] == len(want[1][0])
    assert _down(P, ctx, d_l, np.zeros(len(want[1][0]), P.POSELIL_DTYPE)).tobytes() == want[1][0].tobytes()
    for d in [d_l, d_nl, d_idx, d_map] + dev:
        ctx.device_free(d)
    g.close()


def test_chain_glue_lil_edges_pose_without_the_host():
    """pslfe_glue_run_batch_device -> pslfe_pose_lil_edges_device -> pslfe_pose_optimize_lil_device on two glue_scene frames: the LIL
    rows, their counts and the poses stay in HBM; nothing is copied to the host before the end.  The point edges are the frame's own
    3-D crossings, seen where the identity pose projects them.  Equal to the same steps through the host forms and to the restatement."""
    import psl_slam_amd as P
    ctx = P.default_context()
    g, res, camt, dev = _glue_batch(P, ctx)
    cam = np.ascontiguousarray(camt, P.CAMERA_DTYPE).reshape(())
    camd = {k: cam[k] for k in ("fx", "fy", "cx", "cy", "bf")}
    rng = np.random.default_rng(17)
    nmap, estride, lstride = 40, 128, 32
    lil_map, index = _map_lils(rng, res, nmap)
    v = g.lil_obs_device()
    idx = np.full((2, v["plane_stride"]), -1, np.int32)
    T0 = np.zeros(2, P.POSE_DTYPE)
    E, n = np.zeros((2, estride), P.POSEEDGE_DTYPE), np.zeros(2, np.int32)
    for f, r in enumerate(res):
        idx[f, :len(index[f])] = index[f]
        T0[f] = pc._pose_rec(pc._rodrigues(np.array([0.004, -0.003, 0.002]) * (f + 1)), np.array([0.01, -0.005, 0.008]))
        ok = r["cross"][:, 2] > 0.5
        n[f] = int(ok.sum())
        X = r["cross"][ok]
        E[f, :n[f]]["u"], E[f, :n[f]]["v"] = X[:, 0] / X[:, 2] * float(cam["fx"]) + float(cam["cx"]), X[:, 1] / X[:, 2] * float(cam["fy"]) + float(cam["cy"])
        E[f, :n[f]]["ur"], E[f, :n[f]]["inv_sigma2"] = -1, 1
        E[f, :n[f]]["x"], E[f, :n[f]]["y"], E[f, :n[f]]["z"] = r["cross"][ok].T
    assert (n > 20).all()
    d_idx, d_map, d_T, d_E, d_n = _dev(ctx, idx), _dev(ctx, lil_map), _dev(ctx, T0), _dev(ctx, E), _dev(ctx, n)
    d_l, d_nl = _dev(ctx, np.zeros((2, lstride), P.POSELIL_DTYPE)), _dev(ctx, np.zeros(2, np.int32))
    d_o, d_ol, d_g = _dev(ctx, np.zeros((2, estride), np.uint8)), _dev(ctx, np.zeros((2, lstride), np.uint8)), _dev(ctx, np.zeros(2, np.int32))
    P.Optimizer.LilEdgesDevice(2, v["le_l"], v["le_stride"], v["cross2d"], v["plane_stride"], v["nplanes"], d_idx, d_map, nmap, d_l, 0, d_nl, lstride,
                               ctx=ctx)
    P.Optimizer.PoseOptimizationLilDevice(2, d_T, d_E, d_n, estride, d_l, d_nl, lstride, cam, d_T, d_o, d_ol, d_g, ctx=ctx)
    ctx.synchronize()
    T, gd = _down(P, ctx, d_T, np.zeros(2, P.POSE_DTYPE)), _down(P, ctx, d_g, np.zeros(2, np.int32))
    o, ol = _down(P, ctx, d_o, np.zeros((2, estride), np.uint8)), _down(P, ctx, d_ol, np.zeros((2, lstride), np.uint8))
    for d in [d_idx, d_map, d_T, d_E, d_n, d_l, d_nl, d_o, d_ol, d_g] + dev:
        ctx.device_free(d)
    g.close()
    for f, r in enumerate(res):
        lil, _ = lc.lil_edges(r["le_l"], r["cross2d"], index[f], lil_map)
        assert len(lil) >= 11
        ngood, pose, outlier, outlier_lil = P.Optimizer.PoseOptimization(T0[f], E[f, :n[f]], cam, ctx=ctx, lil=lil)
        assert gd[f] == ngood and T[f].tobytes() == pose.tobytes()
        assert (o[f, :n[f]] == outlier).all() and (ol[f, :len(lil)] == outlier_lil).all()
        ref = lc.optimize(T0[f], E[f, :n[f]], lil, camd)
        assert pose.tobytes() == ref[0].tobytes() and ngood == ref[3] and (outlier == ref[1]).all() and (outlier_lil == ref[2]).all()
        assert pose.tobytes() != T0[f].tobytes()


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/pose_main.cpp on pslfe.hpp with LIL edges (the LIL entry points): the batched device form, the frame-by-frame host form and its own plain C++ loop,
    each against the restatement in the device's order"""
    exe = str(tmp_path / "pose_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "pose_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    names = ["p2_l0", "p2_l1", "p2_l8", "p0_l65", "p250_l10", "p2048_l4", "p40_l512", "p100_l8_allout", "setup"]
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = write_cases(path, names)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        loop, dev, host = read_section(f, cases), read_section(f, cases), read_section(f, cases)
        assert f.read() == b""
    for nm, c, a, b, h in zip(names, cases, loop, dev, host):
        assert_equal_ref(a, c["ref"]["device"], nm + " loop")
        assert_equal_ref(b, c["ref"]["device"], nm + " device")
        assert_equal_ref(h, c["ref"]["device"], nm + " host", info=False)
        assert b[0].tobytes() == a[0].tobytes() and b[3] == a[3]            # the device equals the program's own host loop
