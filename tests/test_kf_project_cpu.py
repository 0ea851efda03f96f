"""CPU checks of the device projection of map points into keyframes (pslfe_kf_project and the three searches that chain it):
the numpy restatement of tests/kf_project_cases.py, which gives the GPU tests their expected rows, is pinned against the C++
oracle's isInFrustum where the two loops have the same rule; the scene is shown to exercise every gate; the limit cases land on the
side the reference's comparisons put them; the new symbols exist and check their arguments; the C++ mirror compiles."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import kf_project_cases as kc
import kf_scene as ks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1500
TH = 3.0


@pytest.fixture(scope="module")
def scene():
    mp, desc = kc.map_points(M)
    return kc.views(), mp, desc, kc.camera(), kc.skip_bytes(kc.NVIEWS, M)


@pytest.mark.parametrize("k", [0, 7, 23])
def test_restatement_equals_oracle_frustum_where_the_rules_coincide(scene, k):
    """Frame::isInFrustum (oracle: pr_project_frustum, view_cos_limit 0.5) and Fuse's loop share the pose product, the depth gate,
    1.0f/z, the distance gates and PredictScale.  They differ in three places, and a point is left out of the comparison of the
    accepted sets only when THIS test finds it on one of them: (fx*X)*invz + cx against fx*(X*invz) + cx (last ulp of u / v) and
    <= max against < max, which matter when the two in-image decisions differ; float(dot / dist) < 0.5f against dot < 0.5*dist in
    double, which matters when those two decisions differ."""
    import oracle_lib
    views, mp, desc, cam, _ = scene
    rows, level, why = kc.restate_project(kc.FUSE, views[k:k + 1], mp, cam, ks.BOUNDS, ks.SCALE, TH)
    _, _, _, inview, olevel, _ = oracle_lib.pr_project_frustum(views[k]["Tcw"].reshape(1), mp, desc, np.asarray(cam).reshape(1), ks.SCALE,
                                                              kc.LOG_SCALE, np.float32(0.5), np.float32(TH), ks.BOUNDS)
    g = kc.geometry(views[k], mp, cam, kc.FUSE)
    F32 = np.float32
    with np.errstate(all="ignore"):
        ub = (F32(cam["fx"]) * g["pc"][:, 0]) * g["invz"] + F32(cam["cx"])          # src/Frame.cc:946-947
        vb = (F32(cam["fy"]) * g["pc"][:, 1]) * g["invz"] + F32(cam["cy"])
        in_a = (g["u"] >= 0) & (g["u"] < 640) & (g["v"] >= 0) & (g["v"] < 480)
        in_b = (ub >= 0) & (ub <= 640) & (vb >= 0) & (vb <= 480)
        view_a = ~(g["dot"] < 0.5 * g["dist"].astype(np.float64))
        view_b = ~((g["dot"] / g["dist"].astype(np.float64)).astype(F32) < F32(0.5))
    excluded = (in_a != in_b) | (view_a != view_b)
    assert excluded.sum() <= 0.01 * M, excluded.sum()
    mine = why[0] == kc.KEPT
    both = mine & (inview != 0)
    assert both.sum() > 0.3 * M
    np.testing.assert_array_equal(level[0][both], olevel[both])
    np.testing.assert_array_equal(mine[~excluded], (inview != 0)[~excluded])


def test_scene_carries_load(scene):
    views, mp, desc, cam, skip = scene
    r = {mode: kc.restate_project(mode, views, mp, cam, ks.BOUNDS, ks.SCALE, TH, skip) for mode in (kc.FUSE, kc.SCW, kc.SIM3)}
    rows, level, why = r[kc.FUSE]
    counts = np.bincount(why.ravel(), minlength=7)
    for gate in (kc.SKIP, kc.DEPTH, kc.IMAGE, kc.MIN_DIST, kc.MAX_DIST, kc.VIEW):
        assert counts[gate] >= 20, (gate, counts)
    assert counts[kc.KEPT] >= 0.3 * why.size
    assert set(np.unique(level[level >= 0]).tolist()) == set(range(8))
    # dropped rows are radius -1 and zeros; kept ones carry the level band
    dead = rows[why != kc.KEPT]
    assert (dead["radius"] == -1).all() and all((dead[f] == 0).all() for f in ("u", "v", "ur", "min_level", "max_level", "angle", "blocks"))
    live = why == kc.KEPT
    assert (rows["max_level"][live] == level[live]).all() and (rows["min_level"][live] == level[live] - 1).all()
    # mode 1 differs from mode 0 only through 1.0/z against 1/z: the same value
    assert r[kc.SCW][0].tobytes() == rows.tobytes()
    # mode 2 has its own distance and no view gate
    r2, r1 = r[kc.SIM3][0], r[kc.SCW][0]
    differ = (r2["radius"] >= 0) & (r2.view(np.uint8).reshape(*r2.shape, 32) != r1.view(np.uint8).reshape(*r1.shape, 32)).any(-1)
    assert differ.sum() >= 1
    assert (r[kc.SIM3][2] == kc.VIEW).sum() == 0


@pytest.mark.parametrize("mode", [kc.FUSE, kc.SCW])
def test_limit_cases_fall_where_the_reference_puts_them(mode):
    views, mp, names = kc.limit_cases()
    rows, level, why = kc.restate_project(mode, views, mp, kc.limit_camera(), kc.LIMIT_BOUNDS, ks.SCALE, TH)
    for i, (what, expect) in enumerate(names):
        assert why[0, i] == expect, (what, why[0, i])
    by = {what: i for i, (what, _) in enumerate(names)}
    assert rows[0, by["u == min_x is kept"]]["u"] == 0 and rows[0, by["v == min_y is kept"]]["v"] == 0
    g = kc.geometry(views[0], mp, kc.limit_camera(), mode)
    assert g["u"][by["u == max_x is dropped"]] == 640 and g["v"][by["v == max_y is dropped"]] == 480
    i = by["dist == 0.8f*min_dist is kept"]
    assert g["dist"][i] == np.float32(0.8) * mp["min_dist"][i]
    i = by["dist == 1.2f*max_dist is kept"]
    assert g["dist"][i] == np.float32(1.2) * mp["max_dist"][i]
    i = by["dot == 0.5*dist is kept"]
    assert g["dot"][i] == 0.5 * float(g["dist"][i])
    # the camera centre of view 1 projected into view 1: dist == 0 and z == 0
    i = by["dist == 0 in view 1 (the point is its camera centre: z == 0)"]
    g1 = kc.geometry(views[1], mp, kc.limit_camera(), mode)
    assert g1["dist"][i] == 0 and g1["z"][i] == 0 and why[1, i] == kc.DEPTH
    assert level[0, by["an infinite ratio cannot pass the depth gate; a huge one gives the last level"]] == 7


def test_new_entry_points_exist_and_check_their_arguments():
    import psl_slam_amd as P
    P.build()
    lib = P.lib()
    f = [C.c_float(0.0), C.c_float(0.0), C.c_float(640.0), C.c_float(480.0)]
    lsf, th = C.c_float(0.18), C.c_float(3.0)
    nm = C.c_int(7)
    E = -1  # PSLFE_E_INVALID
    assert lib.pslfe_kf_project(None, 0, None, 1, None, None, 1, None, *f, None, 8, lsf, th, None, None) == E
    assert b"pslfe_kf_project" in lib.pslfe_last_error()
    assert lib.pslfe_kf_fuse_keyframes(None, None, 0, None, 1, None, None, None, 1, None, *f, None, None, 8, lsf, th, None, None, None) == E
    assert b"pslfe_kf_fuse_keyframes" in lib.pslfe_last_error()
    assert lib.pslfe_kf_search_by_sim3_poses(None, None, None, None, None, None, None, 0, None, None, None, None, 0, None, *f, None, 8, lsf, th,
                                             None, C.byref(nm), None, None) == E
    assert b"pslfe_kf_search_by_sim3_poses" in lib.pslfe_last_error()
    assert lib.pslfe_kf_search_by_projection_sim3_pose(None, None, None, None, None, None, 0, None, *f, None, 8, lsf, th, None, None, None,
                                                       C.byref(nm), None) == E
    assert b"pslfe_kf_search_by_projection_sim3_pose" in lib.pslfe_last_error()
    # the records the mirror passes have the header's layout
    assert P.KFVIEW_DTYPE.itemsize == 100 and P.KFVIEW_DTYPE.fields["T21"][1] == 48 and P.KFVIEW_DTYPE.fields["slot"][1] == 96
    assert (P.KF_PROJ_FUSE, P.KF_PROJ_SCW, P.KF_PROJ_SIM3) == (0, 1, 2)
    for name in ("project", "FuseKeyFrames", "SearchBySim3Poses", "SearchByProjectionSim3Pose"):
        assert callable(getattr(P.KeyFrameMatcher, name))


def test_cpp_mirror_compiles():
    src = r"""
#include "pslfe.hpp"
static_assert(sizeof(PslKfView) == 100, "PslKfView");
void use(pslfe::KeyFrameMatcher& m, pslfe::FrameGrid& g, const std::vector<PslKfView>& views, const std::vector<PslMapPointGeom>& mp,
         const std::vector<uint8_t>& desc, const std::vector<uint8_t>& skip, const PslCamera& cam, const float bounds[4],
         const std::vector<float>& scale, const std::vector<float>& inv_sigma2) {
    std::vector<PslProjQuery> rows, rows2;
    std::vector<int32_t> level, best_idx, best_dist, match, assigned;
    m.Project(PSLFE_KF_PROJ_SIM3, views, mp, skip, cam, bounds, scale, 0.18f, 3.0f, rows, &level);
    m.FuseKeyFrames(g, PSLFE_KF_PROJ_FUSE, views, mp, desc, skip, cam, bounds, scale, &inv_sigma2, 0.18f, 3.0f, best_idx, best_dist, &rows);
    int nf = m.SearchBySim3Poses(g, g, views[0], mp, desc, skip, views[1], mp, desc, skip, cam, bounds, scale, 0.18f, 7.5f, match, &rows, &rows2);
    int nm = m.SearchByProjectionSim3Pose(g, views[0], mp, desc, skip, cam, bounds, scale, 0.18f, 10.0f, skip, match, assigned, &rows);
    (void)nf; (void)nm;
}
"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "use_kf_project.cpp")
        with open(path, "w") as fh:
            fh.write(src)
        r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "psl-slam_amd", "host"),
                            "-I", os.path.join(ROOT, "include"), path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
