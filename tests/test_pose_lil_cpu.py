"""The restatement of the LIL edges of the pose optimisation (tests/pose_lil_cases.py) on its own, the two reference oddities made
visible, the restatement pinned against what its two separate drivers returned before they became one, the ABI of the LIL entry
points, and the stand-alone host program of tools/dropin/pose_main.cpp on the LIL cases, plain and under the address and
undefined-behaviour sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_lil_cases as lc
import pose_opt_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the largest difference of a pose float between the two orders of the restatement over lc.CASE_NAMES, measured here as
# pose_opt_cases.order_difference() was for the point edges: 0.0 - the sums differ in double (by up to 4e-7 in an
# entry of H of 4e8) but no pose FLOAT of this case set changes.  tests/test_pose_lil_gpu.py allows four times that: on these cases
# the device's pose floats equal the edge order's.
# A case added to lc.CASE_SPECS whose two orders differ in a pose float makes test_order_difference_is_the_documented_one fail: the
# figure is then measured again, here and in DESIGN.md, and the GPU bound follows from it.
ORDER_DIFFERENCE = 0.0


def write_cases(path, names):
    """cases.bin of tools/dropin/pose_main.cpp"""
    import psl_slam_amd as P
    cases = [lc.case(nm) for nm in names]
    estride, lstride = max(len(c["edges"]) for c in cases), max(len(c["lil"]) for c in cases)
    camrec = np.zeros((), P.CAMERA_DTYPE)
    for k, v in pc.camera().items():
        camrec[k] = v
    with open(path, "wb") as f:
        np.array([len(cases), estride, lstride], np.int32).tofile(f)
        camrec.tofile(f)
        for c in cases:
            c["Tcw"].tofile(f)
            np.array([len(c["edges"]), len(c["lil"])], np.int32).tofile(f)
            c["edges"].tofile(f)
            c["lil"].tofile(f)
    return cases


def read_section(f, cases):
    """one section of out.bin -> [(pose, outlier, outlier_lil, ngood, info)]"""
    out = []
    for c in cases:
        pose = np.fromfile(f, pc.POSE_DTYPE, 1)[0]
        ngood = int(np.fromfile(f, np.int32, 1)[0])
        info = np.fromfile(f, pc.INFO_DTYPE, 1)[0]
        o = np.fromfile(f, np.uint8, len(c["edges"]))
        out.append((pose, o, np.fromfile(f, np.uint8, len(c["lil"])), ngood, info))
    return out


def assert_equal_ref(got, ref, what, info=True):
    """bit for bit: pose floats, both outlier arrays, return value, rounds and iterations"""
    pose, outlier, outlier_lil, ngood, inf = got
    rpose, routlier, routlier_lil, rngood, rinf = ref
    assert pose.tobytes() == rpose.tobytes(), (what, pc.pose_floats(pose), pc.pose_floats(rpose))
    assert ngood == rngood, (what, ngood, rngood)
    if routlier is not None:
        assert (np.asarray(outlier) == routlier).all(), (what, np.flatnonzero(np.asarray(outlier) != routlier)[:8])
        assert (np.asarray(outlier_lil) == routlier_lil).all(), (what, np.flatnonzero(np.asarray(outlier_lil) != routlier_lil)[:8])
    if info:
        assert inf.tobytes() == rinf.tobytes(), (what, inf, rinf)


@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_both_orders_give_the_same_flags_and_return_value(name):
    c = lc.case(name)
    d, e = c["ref"]["device"], c["ref"]["edge"]
    assert d[3] == e[3] and d[4]["rounds"] == e[4]["rounds"]
    assert (d[1] is None and e[1] is None) or ((d[1] == e[1]).all() and (d[2] == e[2]).all())


def test_order_difference_is_the_documented_one():
    """the two orders of the restatement differ by at most ORDER_DIFFERENCE in a pose float on this case set"""
    d = lc.order_difference()
    print("order difference", d)
    assert d <= ORDER_DIFFERENCE


def test_the_one_driver_returns_what_the_two_drivers_returned():
    """tests/golden/pose_restatement_pins.npz holds what pose_opt_cases.optimize and pose_lil_cases.optimize returned while each had
    its own copy of the rounds, iterations and trials (tests/golden/make_golden.py pose_pins, run on that code): pose bytes, flags,
    return value, rounds and iterations, and the margin as a float64.  The one driver returns the same bits on every case of both
    case sets in both orders, and without LIL edges pose_lil_cases.optimize is pose_opt_cases.optimize on every point case."""
    pins = np.load(os.path.join(ROOT, "tests", "golden", "pose_restatement_pins.npz"))

    def check(key, pose, flags, ngood, info, margin):
        assert pose.tobytes() == pins[key + "/pose"].tobytes(), key
        for k, f in flags.items():
            assert (f is None) == bool(pins[f"{key}/{k}_none"]), (key, k)
            assert f is None or (f.dtype == np.uint8 and f.tobytes() == pins[f"{key}/{k}"].tobytes()), (key, k)
        assert ngood == int(pins[key + "/ngood"]) and info.tobytes() == pins[key + "/info"].tobytes(), key
        assert np.float64(margin).tobytes() == pins[key + "/margin"].tobytes(), (key, margin)

    checked = 0
    for nm in pc.CASE_NAMES:
        c = pc.case(nm)
        for order in ("device", "edge"):
            pose, outlier, ngood, info, margin = pc.optimize(c["Tcw"], c["edges"], c["cam"], order)
            check(f"points/{nm}/{order}", pose, {"outlier": outlier}, ngood, info, margin)
            pose, outlier, outlier_lil, ngood, info, margin = lc.optimize(c["Tcw"], c["edges"], np.zeros(0, lc.LIL_DTYPE), c["cam"], order)
            assert outlier_lil is None or len(outlier_lil) == 0
            check(f"points/{nm}/{order}", pose, {"outlier": outlier}, ngood, info, margin)
            checked += 1
    for nm in lc.CASE_NAMES:
        c = lc.case(nm)
        for order in ("device", "edge"):
            pose, outlier, outlier_lil, ngood, info, margin = lc.optimize(c["Tcw"], c["edges"], c["lil"], c["cam"], order)
            check(f"lil/{nm}/{order}", pose, {"outlier": outlier, "outlier_lil": outlier_lil}, ngood, info, margin)
            checked += 1
    assert checked == 2 * (len(pc.CASE_NAMES) + len(lc.CASE_NAMES)) and len(pins.files) == 12 * len(pc.CASE_NAMES) + 16 * len(lc.CASE_NAMES)


def test_early_return_and_one_round_rule_count_both_kinds():
    """2 points: nothing is optimised; 2 points + 1 LIL: one round; 2 + 7 = 9: one round; 2 + 8 = 10: four; 3 LIL alone: one"""
    for nm, rounds in (("p2_l0", 0), ("p2_l1", 1), ("p2_l7", 1), ("p2_l8", 4), ("p0_l3", 1), ("p0_l64", 4)):
        c = lc.case(nm)
        pose, outlier, outlier_lil, ngood, info = c["ref"]["device"]
        assert info["rounds"] == rounds, (nm, info)
        if rounds == 0:
            assert ngood == 0 and outlier is None and outlier_lil is None and pose.tobytes() == c["Tcw"].tobytes()
        else:
            assert info["iterations"][0] >= 1 and pose.tobytes() != c["Tcw"].tobytes()


def test_an_outlying_lil_edge_still_counts_in_the_return_value():
    """every LIL edge is planted 20 to 60 px off among 100 good points: all are flagged, and nInitialCorrespondences - nBad (:1022)
    still holds them, because nBad counts point edges only"""
    c = lc.case("p100_l8_allout")
    for order in ("device", "edge"):
        _, outlier, outlier_lil, ngood, _ = c["ref"][order]
        assert outlier_lil.all() and len(outlier_lil) == 8
        assert ngood == 100 - int(outlier.sum()) + 8


def test_planted_lil_outliers_are_found_among_many_inliers():
    for nm in ("p40_l512", "p0_l64", "p250_l10"):
        c = lc.case(nm)
        assert c["planted_lil"].any()
        assert (c["ref"]["device"][2] == c["planted_lil"]).all(), nm


def test_row2_quirk_is_visible():
    """EdgeLIL.h:273-275: the Jacobian's row 2 at line 2's END point.  Start and end of line 2 are at least 0.5 m apart in these
    cases, and the "corrected" Jacobian gives another pose: the GPU tests can tell the two apart."""
    for nm in ("p0_l65", "p2_l8", "p63_l30"):
        c = lc.case(nm)
        assert np.linalg.norm(c["lil"]["line2"][:, :3] - c["lil"]["line2"][:, 3:], axis=1).min() >= 0.5
        fixed = lc.optimize(c["Tcw"], c["edges"], c["lil"], c["cam"], "device", fix_row2=True)
        assert fixed[0].tobytes() != c["ref"]["device"][0].tobytes(), nm


def test_plane_index_quirk_is_visible():
    """src/Optimizer.cc:658: mvle_l[i] with i a plane index.  The frame has 20 crossings and 12 planes; the edges of the loop differ
    from those of the aligned variant in their line observations (never in CrossPoint_2D), and so does the pose"""
    c = lc.case("setup")
    assert len(c["le_l"]) > len(c["cross2d"]) and (c["cross_of_plane"] != np.arange(len(c["cross2d"]))).all()
    assert list(c["edge_plane"]) == [i for i in range(12) if i not in (3, 5, 7)]           # -1, bad, outside the map
    aligned, planes = lc.lil_edges(c["le_l"], c["cross2d"], c["lil_index"], c["lil_map"], c["cross_of_plane"])
    assert (planes == c["edge_plane"]).all()
    assert aligned["obs_ins"].tobytes() == c["lil"]["obs_ins"].tobytes() and aligned["line1"].tobytes() == c["lil"]["line1"].tobytes()
    assert (aligned["obs1"] != c["lil"]["obs1"]).any(axis=1).all()
    got = lc.optimize(c["Tcw"], c["edges"], aligned, c["cam"], "device")
    assert got[0].tobytes() != c["ref"]["device"][0].tobytes()


def test_abi_and_dtypes():
    import psl_slam_amd as P
    L = P.lib()
    for fn in ("pslfe_pose_optimize_lil_device", "pslfe_pose_optimize_lil", "pslfe_pose_lil_edges_device", "pslfe_glue_lil_obs_device"):
        assert hasattr(L, fn), fn
    assert P.POSELIL_DTYPE == lc.LIL_DTYPE and P.MAPLIL_DTYPE == lc.MAPLIL_DTYPE
    assert P.POSELIL_DTYPE.itemsize == 184 and P.MAPLIL_DTYPE.itemsize == 128
    with open(os.path.join(ROOT, "include", "pslfe.h")) as f:
        assert "sizeof(PslPoseLilEdge) == 184 && sizeof(PslMapLil) == 128" in f.read()
    # the argument checks that need no device: counts first, then an empty call, then the arrays
    cam = np.zeros(1, P.CAMERA_DTYPE)
    null, i = C.c_void_p(None), C.c_int
    f = L.pslfe_pose_optimize_lil_device
    assert f(null, i(-1), null, null, null, i(4), null, null, i(4), P._ptr(cam), null, null, null, null, null) == -1
    assert f(null, i(1), null, null, null, i(4), null, null, i(-1), P._ptr(cam), null, null, null, null, null) == -1
    assert f(null, i(0), null, null, null, i(4), null, null, i(4), P._ptr(cam), null, null, null, null, null) == 0
    assert f(null, i(1), null, null, null, i(4), null, null, i(4), P._ptr(cam), null, null, null, null, null) == -1
    assert L.pslfe_pose_optimize_lil(null, null, null, i(0), null, i(-1), P._ptr(cam), null, null, null, null) == -1
    g = L.pslfe_pose_lil_edges_device
    assert g(null, i(-1), null, i(4), null, i(4), null, null, null, i(0), null, null, null, i(4)) == -1
    assert g(null, i(1), null, i(4), null, i(4), null, null, null, i(0), null, null, null, i(-4)) == -1
    assert g(null, i(0), null, i(4), null, i(4), null, null, null, i(0), null, null, null, i(4)) == 0
    assert g(null, i(1), null, i(4), null, i(4), null, null, null, i(0), null, null, null, i(4)) == -1
    assert L.pslfe_glue_lil_obs_device(null, null, null, null, null, null, null) == -1


def _build_host(tmp_path, sanitize):
    exe = str(tmp_path / ("pose_lil_host_san" if sanitize else "pose_lil_host"))
    src = os.path.join(ROOT, "tools", "dropin", "pose_main.cpp")
    if sanitize:
        cmd = [HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPSL_POSE_HOST_ONLY", "-Xarch_host",
               "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, src]
    else:
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-DPSL_POSE_HOST_ONLY", "-o", exe, src]
    subprocess.run(cmd, check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "sanitizers"])
def test_host_program_equals_restatement(tmp_path, sanitize):
    """tools/dropin/pose_main.cpp with -DPSL_POSE_HOST_ONLY on every LIL case: its plain C++ loop equals the restatement in the
    device's order bit for bit; built as a stand-alone program under -fsanitize=address,undefined the sanitizers stay silent"""
    exe = _build_host(tmp_path, sanitize)
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = write_cases(path, lc.CASE_NAMES)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        got = read_section(f, cases)
        assert f.read() == b""
    for nm, c, g in zip(lc.CASE_NAMES, cases, got):
        assert_equal_ref(g, c["ref"]["device"], nm)
