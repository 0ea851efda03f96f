"""The restatement of the local bundle adjustment (tests/ba_cases.py) and the stand-alone host program of tools/dropin/ba_main.cpp (the
shared header psl-slam_amd/csrc/ba_kernels.h compiled for the host with g++, under the address and undefined-behaviour sanitizers),
bit for bit with each other; the restatement's Schur + LDLt step against a dense numpy solve; both Jacobian halves of both edge
types against central differences; the properties that need no number; what the cases exercise; the ABI.  No GPU.

The Schur path against an independent solve (test_schur_step_against_dense_solve): for the first iteration of each scene the full
(6 F + 3 P) system is built densely from the restatement's per-edge Jacobians and (H + lambda I) x = b solved by numpy.linalg.solve.
The bound is |x - x_np| / |x_np| <= k cond2(H + lambda I) 2^-52.  Measured here over the scenes of SCHUR_SCENES: the largest ratio
|x - x_np| / |x_np| / (cond2 2^-52) is 0.0664 (lambda_grows; every other scene is below 0.0091; cond2 is 4.4e4 .. 1.4e5), so
k = 4 x 0.0664 = 0.266; the margin covers the different summation orders.

Jacobians (test_jacobians_against_central_differences): tests/test_pose_opt_cpu.py has no such check to take a step from, so the
bound is measured the same way.  Central differences of computeError with the step 1e-3 in every oplus coordinate; the deviation of
an edge is the largest |J - J_fd| over the largest |J| of that half.  Measured here, worst edge per kind:
    pose half, monocular 2.68e-05   pose half, stereo 1.03e-05   point half, monocular 3.45e-06   point half, stereo 7.56e-05
(the stereo error keeps its `const float invz`, whose rounding the differences see) and the bound is four times each.

Outliers (test_properties): pixel noise sigma 0.5 px times the octave's scale, a planted outlier 30 .. 60 px away on a point with at
least four observations and no other outlier (ba_cases.NOISE_PX, OUTLIER_PX): every planted outlier of f5_x3_p40 (31) and
caps_8_64_256 (30) is flagged by the restatement.

Distance from the ground truth, reported, not gated (test_properties prints it): largest point coordinate error /
largest translation error, start -> end:
    f1_x1_p6 0.129 -> 0.862 / 0.028 -> 0.192    f2_x1_p8_stereo 0.199 -> 0.585 / 0.062 -> 0.349    f2_x2_p8_mono 0.102 -> 0.028 / 0.080 -> 0.182
    f2_x1_p8_mixed 0.111 -> 0.117 / 0.075 -> 0.350    f5_x3_p40 0.158 -> 0.102 / 0.081 -> 0.039    caps_8_64_256 0.116 -> 1.26 / 0.074 -> 0.023
(two or three keyframes and two observations per point leave depth weakly determined at 0.5 px of noise; the chi2 falls in all)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ba_cases as bc
from pose_opt_cases import se3_exp, se3_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHYSICAL = list(bc.SHAPES) + ["fixed_among_local", "point_only_fixed", "single_observation", "depth_only", "lambda_grows", "stopped_by_nbad", "rounds_1"]
SCHUR_SCENES = PHYSICAL + ["noise_free"]
SCHUR_RATIO, SCHUR_K = 0.0664, 4 * 0.0664
JACOBIAN_STEP = 1e-3
JACOBIAN_WORST = {"pose_mono": 2.68e-05, "pose_stereo": 1.03e-05, "point_mono": 3.45e-06, "point_stereo": 7.56e-05}


def _case(name):
    return bc.noise_free_case() if name == "noise_free" else bc.case(name)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the header's host form as a stand-alone program, built once with g++ alone under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("local_ba") / "ba_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DPSL_BA_HOST_ONLY", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "ba_main.cpp")],
                   check=True, capture_output=True)
    return exe


def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path):
    """every case: poses, points, erase flags, status, rounds, iterations and the three chi2 values; refused problems too"""
    two = [bc.case(n) for n in bc.CASE_NAMES if bc.case(n)["rounds"] == 2] + [bc.noise_free_case()]
    big = bc.make_scene(77, 2, 1, 12, "mono")
    big["ref"] = bc.local_ba(big["kf"], big["mp"], big["edges"], big["cam"], 2, caps=(16, 11, 512))
    assert int(big["ref"]["info"]["status"]) == bc.E_CAPACITY
    dup = dict(two[0], edges=np.concatenate([two[0]["edges"], two[0]["edges"][:1]]))
    outside = dict(two[0], edges=two[0]["edges"].copy())
    outside["edges"]["point"][0] = -1
    still = dict(two[0], kf=two[0]["kf"].copy())
    still["kf"]["fixed"] = 1
    for c, st in ((dup, bc.E_INVALID), (outside, bc.E_INVALID), (still, 0)):
        c["ref"] = bc.local_ba(c["kf"], c["mp"], c["edges"], c["cam"], 2)
        assert int(c["ref"]["info"]["status"]) == st and int(c["ref"]["info"]["rounds"]) == 0
    one = [bc.case(n) for n in bc.CASE_NAMES if bc.case(n)["rounds"] == 1]
    assert len(one) == 2
    for rounds, group, caps in ((2, two + [dup, outside, still], (16, 128, 512)), (1, one, (16, 128, 512)), (2, [big], (16, 11, 512))):
        path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
        bc.write_cases(path, group, rounds, caps)
        p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        for k, (g, c) in enumerate(zip(bc.read_sections(out, group, 1)[0], group)):
            bc.assert_equal_ref(g, c["ref"], (rounds, k))


def _dense_step(c):
    """-> (|x - x_np| / |x_np|, cond2(H + lambda I)) of the first iteration"""
    s = bc.first_system(c["kf"], c["mp"], c["edges"], c["cam"])
    P, kfof = s["P"], s["kfof"]
    F = len(kfof)
    pts = [p for p in range(P.nmp) if s["pact"][p]]
    n = 6 * F + 3 * len(pts)
    pcol = {k: 6 * i for i, k in enumerate(kfof)}
    lcol = {p: 6 * F + 3 * i for i, p in enumerate(pts)}
    H, b = np.zeros((n, n)), np.zeros(n)
    for e, (Jp, Jl, w) in s["rows"].items():
        J = np.zeros((3, n))
        if P.e_kf[e] in pcol:                   # a fixed vertex gets no block
            J[:, pcol[P.e_kf[e]]:pcol[P.e_kf[e]] + 6] = np.array(Jp)
        J[:, lcol[P.e_pt[e]]:lcol[P.e_pt[e]] + 3] = np.array(Jl)
        H += w * J.T @ J
        b -= w * J.T @ np.array(s["err"][e])
    A = H + s["lam"] * np.eye(n)
    x_np = np.linalg.solve(A, b)
    x = np.array(list(s["xp"]) + [v for p in pts for v in s["xl"][p]])
    return float(np.linalg.norm(x - x_np) / np.linalg.norm(x_np)), float(np.linalg.cond(A, 2))


def test_schur_step_against_dense_solve():
    worst = 0.0
    for name in SCHUR_SCENES:
        rel, cond = _dense_step(_case(name))
        ratio = rel / (cond * 2.0 ** -52)
        print(f"{name}: |x - x_np| / |x_np| = {rel:.3g}, cond2 = {cond:.3g}, ratio = {ratio:.3g}")
        worst = max(worst, ratio)
        assert rel <= SCHUR_K * cond * 2.0 ** -52, (name, rel, cond, ratio)
    print(f"largest ratio {worst:.3g} (recorded {SCHUR_RATIO}, k = {SCHUR_K:.3g})")


def _jacobian_deviation(c):
    s = bc.first_system(c["kf"], c["mp"], c["edges"], c["cam"])
    P, T, X, h = s["P"], s["T"], s["X"], JACOBIAN_STEP
    worst = dict.fromkeys(JACOBIAN_WORST, 0.0)
    for e, (Jp, Jl, _) in s["rows"].items():
        k, p = P.e_kf[e], P.e_pt[e]

        def err(Tk, Xp):
            T2, X2 = list(T), [list(x) for x in X]
            T2[k], X2[p] = Tk, Xp
            return np.array(P.error(e, P.camera_point(e, T2, X2)))

        nr = 2 if P.mono[e] else 3
        Jfd, Lfd = np.zeros((3, 6)), np.zeros((3, 3))
        for j in range(6):                      # VertexSE3Expmap::oplusImpl: exp(update) * estimate
            d = [0.0] * 6
            d[j] = h
            ep = err(se3_mul(se3_exp(d), T[k]), X[p])
            d[j] = -h
            Jfd[:, j] = (ep - err(se3_mul(se3_exp(d), T[k]), X[p])) / (2 * h)
        for j in range(3):                      # VertexSBAPointXYZ::oplusImpl: estimate += update
            xp, xm = list(X[p]), list(X[p])
            xp[j] += h
            xm[j] -= h
            Lfd[:, j] = (err(T[k], xp) - err(T[k], xm)) / (2 * h)
        Ja, La = np.array(Jp), np.array(Jl)
        kind = "mono" if P.mono[e] else "stereo"
        worst["pose_" + kind] = max(worst["pose_" + kind], float(np.abs(Ja[:nr] - Jfd[:nr]).max() / np.abs(Ja[:nr]).max()))
        worst["point_" + kind] = max(worst["point_" + kind], float(np.abs(La[:nr] - Lfd[:nr]).max() / np.abs(La[:nr]).max()))
        if P.mono[e]:
            assert not np.array(Jp[2]).any() and not np.array(Jl[2]).any()
    return worst


def test_jacobians_against_central_differences():
    seen = dict.fromkeys(JACOBIAN_WORST, 0.0)
    for name in PHYSICAL:
        for kind, v in _jacobian_deviation(bc.case(name)).items():
            seen[kind] = max(seen[kind], v)
            assert v <= 4 * JACOBIAN_WORST[kind], (name, kind, v)
    print({k: f"{v:.3g}" for k, v in seen.items()})
    assert all(v > 0 for v in seen.values())      # every kind of half was met


def test_properties():
    """the driver accepts only reductions; a noise-free scene with two fixed keyframes erases nothing; every planted gross outlier
    is flagged; the distance from the ground truth is printed"""
    for name in PHYSICAL:
        c = bc.case(name)
        i = c["ref"]["info"]
        assert int(i["status"]) == 0 and float(i["chi2_round1"]) <= float(i["chi2_start"]), (name, i)
        assert float(i["chi2_end"]) <= float(i["chi2_round1"]), (name, i)
    nf = bc.noise_free_case()
    assert int(nf["kf"]["fixed"].sum()) == 2 and not nf["ref"]["erase"].any() and float(nf["ref"]["info"]["chi2_end"]) < 1e-6
    planted = 0
    for name in bc.SHAPES:
        c = bc.case(name)
        planted += int(c["planted"].sum())
        assert not ((c["planted"] == 1) & (c["ref"]["erase"] == 0)).any(), name
        xyz = lambda a: np.array([a[k] for k in "xyz"], np.float64)
        t = lambda a: a["Tcw"]["t"].astype(np.float64)
        print(f"{name}: point {np.abs(xyz(c['mp']) - xyz(c['mp_true'])).max():.3g} -> {np.abs(xyz(c['ref']['mp']) - xyz(c['mp_true'])).max():.3g}, "
              f"t {np.abs(t(c['kf']) - t(c['kf_true'])).max():.3g} -> {np.abs(t(c['ref']['kf']) - t(c['kf_true'])).max():.3g}")
    assert planted >= 60
    assert int(bc.case("f5_x3_p40")["planted"].sum()) == 31 and int(bc.case("caps_8_64_256")["planted"].sum()) == 30


def test_cases_are_what_their_names_say():
    """the restated results and traces alone: this test reads no product code, it pins what the cases exercise; the header and the
    kernel are held to these results by the bit-for-bit parity tests (here and in tests/test_local_ba_gpu.py)"""
    shape = lambda c: (int((c["kf"]["fixed"] == 0).sum()), int((c["kf"]["fixed"] != 0).sum()), len(c["mp"]))
    assert shape(bc.case("f1_x1_p6")) == (1, 1, 6) and shape(bc.case("f2_x1_p8_stereo")) == (2, 1, 8) and shape(bc.case("f2_x2_p8_mono")) == (2, 2, 8)
    assert (bc.case("f2_x1_p8_stereo")["edges"]["ur"] >= 0).all() and (bc.case("f2_x2_p8_mono")["edges"]["ur"] < 0).all()
    ur = bc.case("f2_x1_p8_mixed")["edges"]["ur"]
    assert (ur >= 0).any() and (ur < 0).any() and shape(bc.case("f5_x3_p40")) == (5, 3, 40)
    c = bc.case("caps_8_64_256")
    assert (len(c["kf"]), len(c["mp"]), len(c["edges"])) == bc.CAPS
    for name in bc.CASE_NAMES:                  # every case runs, with the rounds it asks for
        c = bc.case(name)
        assert int(c["ref"]["info"]["status"]) == 0 and int(c["ref"]["info"]["rounds"]) == c["rounds"] == len(c["ref"]["trace"]), name

    c = bc.case("fixed_among_local")            # a fixed keyframe between two free ones: no block, its pose comes back untouched
    assert list(c["kf"]["fixed"]) == [0, 1, 0, 1] and c["ref"]["trace"][0]["in_system"] == [True, False, True, False]
    assert c["ref"]["kf"][1].tobytes() == c["kf"][1].tobytes() and c["ref"]["kf"][0].tobytes() != c["kf"][0].tobytes()

    c = bc.case("point_only_fixed")             # seen by fixed keyframes alone: no pose coupling, still optimised
    e = c["edges"]
    assert set(e["kf"][e["point"] == 0]) == {2, 3} and all(c["kf"]["fixed"][[2, 3]]) and c["ref"]["trace"][0]["pact"][0]
    assert c["ref"]["mp"][0].tobytes() != c["mp"][0].tobytes()

    c = bc.case("single_observation")
    assert int((c["edges"]["point"] == 0).sum()) == 1 and c["ref"]["trace"][1]["pact"][0] and c["ref"]["mp"][0].tobytes() != c["mp"][0].tobytes()

    c = bc.case("point_drops_out")              # all edges of point 0 on level 1: out of round two, its row is the round-one value
    t0, t1 = c["ref"]["trace"]
    mine = np.flatnonzero(c["edges"]["point"] == 0)
    assert len(mine) >= 2 and all(t1["level"][i] for i in mine) and not t1["pact"][0] and all(t1["pact"][1:])
    assert t1["X"][0] == t0["X"][0] and t1["X"][1] != t0["X"][1]
    assert [np.float32(v) for v in t0["X"][0]] == [c["ref"]["mp"][k][0] for k in "xyz"]

    c = bc.case("keyframe_drops_out")           # likewise free keyframe 1
    t0, t1 = c["ref"]["trace"]
    mine = np.flatnonzero(c["edges"]["kf"] == 1)
    assert len(mine) >= 3 and all(t1["level"][i] for i in mine) and t0["in_system"][1] and not t1["in_system"][1] and t1["F"] == t0["F"] - 1
    assert t1["T"][1] == t0["T"][1] and t1["T"][0] != t0["T"][0]

    c = bc.case("depth_only")                   # erased for its depth alone: its chi2 is far below the threshold
    t1 = c["ref"]["trace"][1]
    b = c["behind_edge"]
    assert t1["depth_bad"][b] and t1["chi2"][b] < 1e-3 and c["ref"]["erase"][b] == 1 and int(c["ref"]["erase"].sum()) == 1
    assert sum(t1["depth_bad"]) == 1

    c = bc.case("threshold_ulps")               # nothing moves; the four chi2 are the neighbours of 5.991 and 7.815 as doubles
    tr = c["ref"]["trace"][0]
    assert all(not ok and why == "landmark" for _, ok, why, _, _ in tr["trials"]) and tr["its"] == 5
    for e, chi2, above in c["planted_chi2"]:
        assert tr["chi2"][e] == chi2 and bool(c["ref"]["erase"][e]) == above and not tr["depth_bad"][e]
    targets = sorted(t for _, t, _ in c["planted_chi2"])
    assert targets == [float(np.nextafter(5.991, 0)), float(np.nextafter(5.991, 9)), float(np.nextafter(7.815, 0)), float(np.nextafter(7.815, 9))]

    tr = bc.case("lambda_grows")["ref"]["trace"][0]["trials"]       # the first trials of the first iteration are rejected
    assert tr[0][0] == 0 and tr[0][1] and tr[0][3] < 0 and tr[1][0] == 0 and tr[1][4] == 2 * tr[0][4] and tr[2][4] == 8 * tr[0][4]

    assert any(t["stopped"] == "nbad" and t["its"] < 10 for t in bc.case("stopped_by_nbad")["ref"]["trace"])

    t0, t1 = bc.case("failed_solve")["ref"]["trace"]                 # the degenerate point: no finite landmark inverse in round one
    assert all(not ok and why == "landmark" for _, ok, why, _, _ in t0["trials"]) and t1["F"] >= 1 and all(ok for _, ok, _, _, _ in t1["trials"])
    assert not t1["pact"][len(t1["pact"]) - 1]                       # ... it is on level 1 in round two

    t0 = bc.case("failed_pivot")["ref"]["trace"][0]["trials"]        # finite numbers, a pivot that is not positive, until lambda has grown
    fails = [t for t in t0 if not t[1]]
    assert len(fails) >= 3 and all(t[2] == "pivot" and t[3] == -math.inf for t in fails) and t0[0][0] == 0 and not t0[0][1]
    assert any(t[1] and t[0] == 0 for t in t0)                       # the same iteration ends with a trial that solves

    c = bc.case("rounds_1")
    assert int(c["ref"]["info"]["iterations"][1]) == 0 and float(c["ref"]["info"]["chi2_end"]) == float(c["ref"]["info"]["chi2_round1"])
    two = bc.local_ba(c["kf"], c["mp"], c["edges"], c["cam"], 2)
    assert int(two["info"]["iterations"][1]) > 0 and two["mp"].tobytes() != c["ref"]["mp"].tobytes()


def test_abi_pods_and_error_codes_without_a_device():
    import psl_slam_amd as P
    assert P.BAEDGE_DTYPE.itemsize == bc.EDGE_DTYPE.itemsize == 24 and P.BAKEYFRAME_DTYPE.itemsize == bc.KF_DTYPE.itemsize == 52
    assert P.BAINFO_DTYPE.itemsize == bc.INFO_DTYPE.itemsize == 48 and P.BAINFO_DTYPE.fields["chi2_start"][1] == 24
    assert P.BAEDGE_DTYPE == bc.EDGE_DTYPE and P.BAKEYFRAME_DTYPE == bc.KF_DTYPE and P.MAPPOINT_DTYPE == bc.MP_DTYPE
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslBaEdge) == 24 && sizeof(PslBaKeyFrame) == 52 && sizeof(PslBaInfo) == 48" in hdr
    L = P.lib()
    null = C.c_void_p(None)
    dev = lambda K, rounds: L.pslfe_ba_local_device(null, C.c_int(K), null, null, null, null, null, null, null, C.c_int(rounds), null, null, null, null)
    assert dev(0, 2) == 0 and dev(0, 1) == 0                        # K == 0: nothing is done
    assert dev(-1, 2) == -1 and dev(0, 0) == -1 and dev(0, 3) == -1 and dev(1, 2) == -1
    assert b"pslfe_ba_local_device" in L.pslfe_last_error()
    host = lambda nkf, nmp, ne, rounds: L.pslfe_ba_local(null, null, C.c_int(nkf), null, C.c_int(nmp), null, C.c_int(ne), null, C.c_int(rounds),
                                                         null, null, null, null)
    assert host(-1, 0, 0, 2) == -1 and host(0, -1, 0, 2) == -1 and host(0, 0, -1, 2) == -1 and host(0, 0, 0, 0) == -1 and host(0, 0, 0, 2) == -1
    out = C.c_void_p()
    assert L.pslfe_ba_create(null, 1, 1, 1, 1, C.byref(out)) == -1 and L.pslfe_ba_create(null, 1, 1, 1, 1, None) == -1
    L.pslfe_ba_destroy.restype = None
    L.pslfe_ba_destroy(null)
