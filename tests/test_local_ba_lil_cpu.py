"""The restatement of LocalBundleAdjustmentAndInseclines (tests/ba_lil_cases.py) and the stand-alone host program of
tools/dropin/ba_lil_main.cpp (psl-slam_amd/csrc/ba_kernels.h with its LIL parts compiled for the host with g++, under the address and
undefined-behaviour sanitizers), bit for bit with each other; both Jacobian halves of the LIL edge against central differences; the
update rule of a VertexLIL by construction; what the cases exercise; the identity with tests/ba_cases.py without LILs; the ABI.  No GPU.

Jacobians (test_lil_jacobians_against_central_differences): central differences of computeError with the step 1e-3, for row r in the
3-vector of the estimate that row names (0: line 1 start, 1: line 1 end, 3: line 2 end, 4 and 5: the crosspoint) and in the six oplus
coordinates of the pose.  Row 2 is not compared: it is evaluated at line 2's END point (EdgeLIL.h:273-275) while e2 is the error at its
START point, so it equals row 3 bit for bit in both halves, which is asserted.  The deviation of an edge is the largest |J - J_fd|
over the largest |J| of the compared rows of that half.  Measured here over the edges of PHYSICAL, worst edge:
    pose half 3.83e-07   LIL half 1.72e-08
and the bound is four times each."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_cases as bc
import ba_lil_cases as lc
from pose_opt_cases import from_pose, se3_exp, se3_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHYSICAL = list(lc.SHAPES) + ["lil_level1", "lil_only_fixed", "lil_no_edges", "lil_middle_inactive"]
JACOBIAN_STEP = 1e-3
JACOBIAN_WORST = {"pose": 3.83e-07, "lil": 1.72e-08}
ROW_SEGMENT = {0: 0, 1: 1, 3: 3, 4: 4, 5: 4}


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the header's host form with the LILs as a stand-alone program, built once with g++ alone under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("local_ba_lil") / "ba_lil_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DPSL_BA_HOST_ONLY", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "ba_lil_main.cpp")],
                   check=True, capture_output=True)
    return exe


def _ref(c, rounds=2, caps=None):
    return lc.local_ba(c["kf"], c["mp"], c["edges"], c["lil"], c["ledges"], c["cam"], rounds, caps=caps)


def refused_cases():
    """a duplicate (LIL, keyframe) pair, a LIL edge outside the problem (both ways), no free keyframe -> [(case with ref, status)]"""
    base = lc.case("f2_x1_p8_l4")
    dup = dict(base, ledges=np.concatenate([base["ledges"], base["ledges"][:1]]))
    out_lil = dict(base, ledges=base["ledges"].copy())
    out_lil["ledges"]["lil"][1] = len(base["lil"])
    out_kf = dict(base, ledges=base["ledges"].copy())
    out_kf["ledges"]["kf"][0] = -1
    still = dict(base, kf=base["kf"].copy())
    still["kf"]["fixed"] = 1
    res = []
    for c, st in ((dup, bc.E_INVALID), (out_lil, bc.E_INVALID), (out_kf, bc.E_INVALID), (still, 0)):
        c["ref"] = _ref(c)
        assert int(c["ref"]["info"]["status"]) == st and int(c["ref"]["info"]["rounds"]) == 0
        res.append((c, st))
    return res


def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path):
    """every named case: poses, points, the 15 doubles per LIL, both erase arrays, iterations and the three chi2; refused problems too"""
    two = [lc.case(n) for n in lc.CASE_NAMES if lc.case(n)["rounds"] == 2] + [c for c, _ in refused_cases()]
    one = [lc.case(n) for n in lc.CASE_NAMES if lc.case(n)["rounds"] == 1]
    assert len(one) == 1
    tight = (16, 128, 512, 3, 64)                        # one LIL too many for f2_x1_p8_l4
    big = dict(lc.case("f2_x1_p8_l4"))
    big["ref"] = _ref(big, caps=tight)
    assert int(big["ref"]["info"]["status"]) == bc.E_CAPACITY
    plain = [lc.without_lils(lc.case("f5_x3_p40_l8"))]    # no LIL row at all through the LIL text
    plain[0]["ref"] = _ref(plain[0])
    for rounds, group, caps in ((2, two + plain, lc.CAPS_WIDE), (1, one, lc.CAPS_WIDE), (2, [big], tight), (2, [lc.case("caps_8_64_256_8_32")], lc.CAPS)):
        path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
        lc.write_cases(path, group, rounds, caps)
        p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        for k, (g, c) in enumerate(zip(lc.read_sections(out, group, 1)[0], group)):
            lc.assert_equal_ref(g, c["ref"], (rounds, k))


def _lil_jacobian_deviation(c):
    P = bc._Problem(c["kf"], c["mp"], c["edges"], c["cam"])
    Q = lc._Lils(c["lil"], c["ledges"], P)
    T = [from_pose(P.kf["Tcw"][k]) for k in range(P.nkf)]
    L = [[float(v) for v in Q.lil["w"][j]] for j in range(Q.n)]
    h = JACOBIAN_STEP
    worst = dict.fromkeys(JACOBIAN_WORST, 0.0)
    rows = [0, 1, 3, 4, 5]
    for e in range(Q.ne):
        k, j = Q.e_kf[e], Q.e_lil[e]
        Jp, Jl = Q.jacobians(e, T, L)
        assert Jp[2] == Jp[3] and Jl[2] == Jl[3]             # bit for bit: Python floats compare by value, and no entry is a NaN

        def err(Tk, w):
            T2, L2 = list(T), [list(x) for x in L]
            T2[k], L2[j] = Tk, w
            return np.array(Q.error(e, T2, L2))

        Jfd = np.zeros((6, 6))
        for a in range(6):                                   # VertexSE3Expmap::oplusImpl: exp(update) * estimate
            d = [0.0] * 6
            d[a] = h
            ep = err(se3_mul(se3_exp(d), T[k]), L[j])
            d[a] = -h
            Jfd[:, a] = (ep - err(se3_mul(se3_exp(d), T[k]), L[j])) / (2 * h)
        Lfd = np.zeros((6, 3))
        for r in rows:                                       # row r with respect to the 3-vector it names
            for a in range(3):
                wp, wm = list(L[j]), list(L[j])
                wp[3 * ROW_SEGMENT[r] + a] += h
                wm[3 * ROW_SEGMENT[r] + a] -= h
                Lfd[r, a] = (err(T[k], wp)[r] - err(T[k], wm)[r]) / (2 * h)
        Ja, La = np.array(Jp), np.array(Jl)
        worst["pose"] = max(worst["pose"], float(np.abs(Ja[rows] - Jfd[rows]).max() / np.abs(Ja[rows]).max()))
        worst["lil"] = max(worst["lil"], float(np.abs(La[rows] - Lfd[rows]).max() / np.abs(La[rows]).max()))
        # the "corrected" row 2 (at line 2's start) is what the differences of e2 see; the reference's row 2 is not
        Jp2, Jl2 = Q.jacobians(e, T, L, fix_row2=True)
        assert Jp2[2] != Jp[2] and Jl2[2] != Jl[2]
    return worst


def test_lil_jacobians_against_central_differences():
    seen = dict.fromkeys(JACOBIAN_WORST, 0.0)
    for name in PHYSICAL:
        for kind, v in _lil_jacobian_deviation(lc.case(name)).items():
            seen[kind] = max(seen[kind], v)
            assert v <= 4 * JACOBIAN_WORST[kind], (name, kind, v)
    print({k: f"{v:.3g}" for k, v in seen.items()})
    assert all(v > 0 for v in seen.values())


@pytest.mark.parametrize("name,count", [("f2_x1_p6_l1", 1), ("f2_x1_p8_l4", 4), ("f2_x1_p8_l5", 5), ("f2_x2_p8_l6", 6), ("lil_middle_inactive", 6)])
def test_update_rule_by_construction(name, count):
    """the candidate of active LIL a(i), segment m, is the estimate plus xl of a(i + m), or the estimate itself past the end; an
    inactive LIL is skipped as a follower and keeps its estimate"""
    c = lc.case(name)
    nlil = len(c["lil"])
    solved = 0
    for r, tr in enumerate(c["ref"]["trace"]):
        act = [j for j in range(nlil) if tr["lact"][j]]
        if r == 0:
            assert len(act) == count
        if name == "lil_middle_inactive" and r == 1:
            assert act == [0, 1, 3, 4, 5]                    # LIL 2 went inactive in round two
        for active, xl, L, Ln in tr["updates"]:
            solved += 1
            assert active == act
            for j in range(nlil):
                if j not in act:
                    assert Ln[j] == L[j]
                    continue
                i = act.index(j)
                for m in range(5):
                    for a in range(3):
                        if i + m < len(act):
                            assert Ln[j][3 * m + a] == L[j][3 * m + a] + xl[act[i + m]][a], (name, r, j, m, a)
                        else:
                            assert Ln[j][3 * m + a] == L[j][3 * m + a], (name, r, j, m, a)
            if len(act) > 1:                                 # segment 1 of the first LIL moves with the SECOND LIL's step
                assert Ln[act[0]][3:6] == [L[act[0]][3 + a] + xl[act[1]][a] for a in range(3)]
    assert solved >= 2


def test_cases_are_what_their_names_say():
    """the restated results and traces alone: this test reads no product code, it pins what the cases exercise"""
    shape = lambda c: (int((c["kf"]["fixed"] == 0).sum()), int((c["kf"]["fixed"] != 0).sum()), len(c["mp"]), len(c["lil"]), len(c["ledges"]))
    assert shape(lc.case("f2_x1_p6_l1")) == (2, 1, 6, 1, 2) and shape(lc.case("f5_x3_p40_l8"))[:4] == (5, 3, 40, 8)
    assert shape(lc.case("f2_x1_p8_l4"))[3] == 4 and shape(lc.case("f2_x1_p8_l5"))[3] == 5 and shape(lc.case("f2_x2_p8_l6"))[3] == 6
    c = lc.case("caps_8_64_256_8_32")
    assert (len(c["kf"]), len(c["mp"]), len(c["edges"]), len(c["lil"]), len(c["ledges"])) == lc.CAPS
    assert shape(lc.case("p0_l3"))[2] == 0 and len(lc.case("p0_l3")["edges"]) == 0
    for name in lc.CASE_NAMES:
        c = lc.case(name)
        i = c["ref"]["info"]
        assert int(i["status"]) == 0 and int(i["rounds"]) == c["rounds"] == len(c["ref"]["trace"]), name
        assert int(i["iterations"][0]) >= 1 and c["ref"]["lil"].tobytes() != c["lil"].tobytes(), name        # the LILs moved
        assert (c["ref"]["lil"]["bad"] == c["lil"]["bad"]).all()

    c = lc.case("lil_level1")                   # the planted observation: on level 1 after round one, erased by its chi2, not its depth
    t0, t1 = c["ref"]["trace"]
    e = int(np.flatnonzero(c["planted_lil"])[0])
    assert t1["llevel"][e] and t0["chi2_lil"][e] > lc.CHI2_LIL and not t0["depth_bad_lil"][e] and not t1["depth_bad_lil"][e]
    assert c["ref"]["erase_lil"][e] == 1 and t1["chi2_lil"][e] == t0["chi2_lil"][e]      # the cached error of round one
    assert all(t1["lact"])                                                               # its LIL stays in through its other edges

    c = lc.case("lil_depth_only")               # erased for its depth alone
    b = c["behind_edge"]
    t1 = c["ref"]["trace"][1]
    assert t1["depth_bad_lil"][b] and t1["chi2_lil"][b] < 1e-2 and c["ref"]["erase_lil"][b] == 1 and int(c["ref"]["erase_lil"].sum()) == 1
    assert sum(t1["depth_bad_lil"]) == 1 and c["kf"]["fixed"][c["ledges"]["kf"][b]] == 1

    c = lc.case("lil_only_fixed")               # seen by fixed keyframes alone: no pose coupling, still optimised
    e = c["ledges"]
    assert set(e["kf"][e["lil"] == 0]) == {2, 3} and all(c["kf"]["fixed"][[2, 3]]) and c["ref"]["trace"][0]["lact"][0]
    assert c["ref"]["lil"]["w"][0].tobytes() != c["lil"]["w"][0].tobytes()

    c = lc.case("lil_no_edges")                 # not in the system: copied
    assert not (c["ledges"]["lil"] == 1).any() and not c["ref"]["trace"][0]["lact"][1] and c["ref"]["trace"][0]["lact"][0]
    assert c["ref"]["lil"][1].tobytes() == c["lil"][1].tobytes() and c["ref"]["lil"][0].tobytes() != c["lil"][0].tobytes()

    c = lc.case("lil_middle_inactive")          # all edges of LIL 2 on level 1: out of round two, its row is the round-one value
    t0, t1 = c["ref"]["trace"]
    mine = np.flatnonzero(c["ledges"]["lil"] == 2)
    assert len(mine) == 2 and all(t1["llevel"][i] for i in mine) and t0["lact"][2] and not t1["lact"][2]
    assert sum(t1["llevel"]) == 2 and t1["lact"] == [True, True, False, True, True, True]
    assert t1["L"][2] == t0["L"][2] and t1["L"][3] != t0["L"][3] and list(c["ref"]["lil"]["w"][2]) == t0["L"][2]

    c = lc.case("lil_rounds_1")
    assert int(c["ref"]["info"]["iterations"][1]) == 0 and float(c["ref"]["info"]["chi2_end"]) == float(c["ref"]["info"]["chi2_round1"])


@pytest.mark.parametrize("name", ["f1_x1_p6", "f2_x1_p8_mixed", "f5_x3_p40", "depth_only", "failed_solve", "failed_pivot", "rounds_1", "threshold_ulps"])
def test_without_lils_the_restatement_is_ba_cases(name):
    c = bc.case(name)
    got = lc.local_ba(c["kf"], c["mp"], c["edges"], np.zeros(0, lc.MAPLIL_DTYPE), np.zeros(0, lc.LILEDGE_DTYPE), c["cam"], c["rounds"])
    bc.assert_equal_ref(got, c["ref"], name)
    assert [(t["its"], t["stopped"], len(t["trials"])) for t in got["trace"]] == [(t["its"], t["stopped"], len(t["trials"])) for t in c["ref"]["trace"]]


def test_abi_pods_and_error_codes_without_a_device():
    import psl_slam_amd as P
    assert P.BALILEDGE_DTYPE.itemsize == lc.LILEDGE_DTYPE.itemsize == 72 and P.BALILEDGE_DTYPE == lc.LILEDGE_DTYPE and P.MAPLIL_DTYPE == lc.MAPLIL_DTYPE
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslBaLilEdge) == 72" in hdr
    L = P.lib()
    null = C.c_void_p(None)
    dev = lambda K, rounds: L.pslfe_ba_local_lil_device(null, C.c_int(K), *([null] * 10), null, C.c_int(rounds), *([null] * 7))
    assert dev(0, 2) == 0 and dev(0, 1) == 0
    assert dev(-1, 2) == -1 and dev(0, 0) == -1 and dev(0, 3) == -1 and dev(1, 2) == -1
    assert b"pslfe_ba_local_lil_device" in L.pslfe_last_error()
    host = lambda n, rounds: L.pslfe_ba_local_lil(null, null, C.c_int(n[0]), null, C.c_int(n[1]), null, C.c_int(n[2]), null, C.c_int(n[3]), null,
                                                  C.c_int(n[4]), null, C.c_int(rounds), *([null] * 6))
    for i in range(5):
        n = [0] * 5
        n[i] = -1
        assert host(n, 2) == -1
    assert host([0] * 5, 0) == -1 and host([0] * 5, 2) == -1
    out = C.c_void_p()
    assert L.pslfe_ba_create_lil(null, 1, 1, 1, 1, 1, 1, C.byref(out)) == -1 and L.pslfe_ba_create_lil(null, 1, 1, 1, 1, 1, 1, None) == -1
