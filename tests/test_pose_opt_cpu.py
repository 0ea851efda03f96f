"""The restatement of the pose optimisation (tests/pose_opt_cases.py) on its own, the ABI of the three entry points, and the
stand-alone host program of tools/dropin/pose_main.cpp under the address and undefined-behaviour sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pose_opt_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def write_cases(path, names, cam=None):
    """cases.bin of tools/dropin/pose_main.cpp without LIL edges (lstride = 0, m = 0)"""
    import psl_slam_amd as P
    cases = [pc.case(nm) for nm in names]
    estride = max(len(c["edges"]) for c in cases)
    camrec = np.zeros((), P.CAMERA_DTYPE)
    for k, v in (cam or pc.camera()).items():
        camrec[k] = v
    with open(path, "wb") as f:
        np.array([len(cases), estride, 0], np.int32).tofile(f)
        camrec.tofile(f)
        for c in cases:
            c["Tcw"].tofile(f)
            np.array([len(c["edges"]), 0], np.int32).tofile(f)
            c["edges"].tofile(f)
    return cases


def read_section(f, cases):
    """one section of out.bin -> [(pose, outlier, ngood, info)]"""
    out = []
    for c in cases:
        pose = np.fromfile(f, pc.POSE_DTYPE, 1)[0]
        ngood = int(np.fromfile(f, np.int32, 1)[0])
        info = np.fromfile(f, pc.INFO_DTYPE, 1)[0]
        out.append((pose, np.fromfile(f, np.uint8, len(c["edges"])), ngood, info))
    return out


def assert_equal_ref(got, ref, what, info=True):
    """bit for bit: pose floats, flags, return value, rounds and iterations"""
    pose, outlier, ngood, inf = got
    rpose, routlier, rngood, rinf = ref
    assert pose.tobytes() == rpose.tobytes(), (what, pc.pose_floats(pose), pc.pose_floats(rpose))
    assert ngood == rngood, (what, ngood, rngood)
    if routlier is not None:
        assert (np.asarray(outlier) == routlier).all(), (what, np.flatnonzero(np.asarray(outlier) != routlier)[:8])
    if info:
        assert inf.tobytes() == rinf.tobytes(), (what, inf, rinf)


def test_noise_free_case_recovers_the_true_pose():
    """300 monocular edges without noise, started 2 degrees and 5 cm off.  What keeps the minimum from the true pose is the rounding
    of the observations to float (the map points are floats already): below 640 px a coordinate is off by at most
    d = 2^-16 / 2 = 3.1e-5 px.  To first order the minimum moves by dx = (A^T A)^-1 A^T r with A = W^1/2 J at the true pose and r the
    weighted rounding errors, so |dx| <= |r| / sqrt(lambda_min(H)), H = A^T A, |r|^2 <= 2 d^2 sum(invSigma2).  H comes from the
    Jacobians at the TRUE pose, not from a result.  A rotation entry then differs by at most |dx| (an entry of exp(w) - I is below
    |w|) plus 2^-24 / 2 from its own rounding to float; a translation entry by at most |dx| (1 + |t|) (upsilon plus omega x t) plus
    2^-22 / 2 (|t_i| < 4).  A factor 2 is allowed for the second-order terms and for the point at which the Levenberg rule stops
    (chi2 there is below 1e-3 of the chi2 of the rounding itself); that factor is an assumption, not derived."""
    c = pc.case("n300_mono_0_noisefree")
    pose, outlier, ngood, info = c["ref"]["device"]
    assert ngood == 300 and not outlier.any() and info["rounds"] == 4
    E = pc._Edges(c["edges"], c["cam"])
    e, Pc = E.error(pc.from_pose(c["Ttrue"]))
    acc = pc.sum_edge(E.terms(e, Pc, np.zeros(E.n), np.ones(E.n))[:, None], np.ones(E.n, bool))
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = acc[:21]
    H = H + np.triu(H, 1).T
    dx = np.sqrt(2.0 * E.is2.sum()) * 2.0 ** -17 / np.sqrt(np.linalg.eigvalsh(H)[0])
    tnorm = float(np.linalg.norm(c["Ttrue"]["t"].astype(np.float64)))
    tol_R, tol_t = 2 * dx + 2.0 ** -25, 2 * dx * (1 + tnorm) + 2.0 ** -23
    assert np.abs(c["Ttrue"]["t"]).max() < 4 and tol_R < 2e-6 and tol_t < 1e-5
    d = np.abs(pc.pose_floats(pose).astype(np.float64) - pc.pose_floats(c["Ttrue"]).astype(np.float64))
    start = np.abs(pc.pose_floats(c["Tcw"]).astype(np.float64) - pc.pose_floats(c["Ttrue"]).astype(np.float64))
    assert start[:9].max() > 1e-2 and start[9:].max() > 1e-2
    assert d[:9].max() < tol_R and d[9:].max() < tol_t, (d[:9].max(), tol_R, d[9:].max(), tol_t)


@pytest.mark.parametrize("name", [nm for nm in pc.CASE_SPECS if pc.CASE_SPECS[nm][0] >= 63 and not pc.CASE_SPECS[nm][3]])
def test_flags_equal_the_planted_outliers(name):
    """from 63 edges on the inliers outvote the planted ones (20 to 60 px off, against 0.5 px of noise) in every case of the set; a
    frame of 9 or 10 edges with three of them planted has too few inliers for that to be a property of the algorithm"""
    c = pc.case(name)
    for order in ("device", "edge"):
        _, outlier, ngood, _ = c["ref"][order]
        assert (outlier == c["planted"]).all(), (order, np.flatnonzero(outlier != c["planted"]))
        assert ngood == len(c["planted"]) - int(c["planted"].sum())


def test_two_edges_return_zero_and_keep_the_pose():
    c = pc.case("n2_mixed_0")
    for order in ("device", "edge"):
        pose, outlier, ngood, info = c["ref"][order]
        assert ngood == 0 and outlier is None and info["rounds"] == 0 and pose.tobytes() == c["Tcw"].tobytes()
    assert pc.case("n3_mixed_0")["ref"]["device"][3]["rounds"] == 1
    for kind in ("mono", "stereo"):
        assert pc.case(f"n2_{kind}_0")["ref"]["device"][2] == 0


def test_non_physical_data_leave_a_finite_pose():
    """a map point at 1e18 m: the damping and the Huber weights keep every step small, all four rounds run and the pose stays finite.
    (No input was found that drives a step's rotation angle past 105414350, where the kernel, the host loop and the restatement
    treat the trial as a failed solve; that guard is a bound on a table index, not a path these cases reach.)"""
    c = pc.case("huge")
    pose, outlier, ngood, info = c["ref"]["device"]
    assert np.isfinite(pc.pose_floats(pose)).all() and info["rounds"] == 4


def test_one_round_for_nine_edges_four_for_ten():
    for nm, spec in pc.CASE_SPECS.items():
        if spec[0] > 300:
            continue
        rounds = int(pc.case(nm)["ref"]["device"][3]["rounds"])
        assert rounds == (0 if spec[0] < 3 else 1 if spec[0] < 10 else 4), (nm, rounds)
    info = pc.case("n9_mono_0")["ref"]["device"][3]
    assert info["iterations"][0] >= 1 and (info["iterations"][1:] == 0).all()


def test_exact_data_end_every_round_after_one_iteration():
    """chi2 = 0 and b = 0 give a zero step and rho == 0: Terminate in the first iteration of each of the four rounds"""
    c = pc.case("exact")
    for order in ("device", "edge"):
        pose, outlier, ngood, info = c["ref"][order]
        assert info["rounds"] == 4 and (info["iterations"] == 1).all() and ngood == len(c["edges"]) and not outlier.any()
        assert pose.tobytes() == c["Tcw"].tobytes()


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_both_orders_give_the_same_flags_and_return_value(name):
    """every case of the GPU test; the builder has rejected seeds with a classification chi2 within a relative 1e-6 of its threshold"""
    d, e = pc.case(name)["ref"]["device"], pc.case(name)["ref"]["edge"]
    assert d[2] == e[2] and d[3]["rounds"] == e[3]["rounds"]
    assert (d[1] is None and e[1] is None) or (d[1] == e[1]).all()
    if name != "exact":
        c = pc.case(name)
        for order in ("device", "edge"):
            assert pc.optimize(c["Tcw"], c["edges"], c["cam"], order)[4] > pc.MARGIN


def test_the_behind_case_has_a_point_behind_the_camera():
    c = pc.case("n65_mixed_0_behind")
    R, t = c["Tcw"]["R"].astype(np.float64).reshape(3, 3), c["Tcw"]["t"].astype(np.float64)
    e = c["edges"][-1]
    assert (R @ np.array([e["x"], e["y"], e["z"]], np.float64) + t)[2] < -1.0
    assert c["ref"]["device"][1][-1] == 1


def test_order_difference_is_the_documented_one():
    """the two orders of the restatement differ by at most 3.73e-9 in a pose float on this case set (one ulp of an
    entry below 2^-5); tests/test_pose_opt_gpu.py allows four times that against the edge order"""
    assert pc.order_difference() <= 3.73e-9


def test_abi_and_dtypes():
    import psl_slam_amd as P
    L = P.lib()
    for fn in ("pslfe_pose_optimize_device", "pslfe_pose_optimize", "pslfe_pose_edges_from_matches_device"):
        assert hasattr(L, fn), fn
    assert P.POSEEDGE_DTYPE == pc.EDGE_DTYPE and P.POSEINFO_DTYPE == pc.INFO_DTYPE and P.POSE_DTYPE == pc.POSE_DTYPE
    # the argument checks that need no device: counts first, then an empty call, then the arrays
    cam = np.zeros(1, P.CAMERA_DTYPE)
    null = C.c_void_p(None)
    assert L.pslfe_pose_optimize_device(null, C.c_int(-1), null, null, null, C.c_int(4), P._ptr(cam), null, null, null, null) == -1
    assert L.pslfe_pose_optimize_device(null, C.c_int(1), null, null, null, C.c_int(-1), P._ptr(cam), null, null, null, null) == -1
    assert L.pslfe_pose_optimize_device(null, C.c_int(0), null, null, null, C.c_int(4), P._ptr(cam), null, null, null, null) == 0
    assert L.pslfe_pose_optimize_device(null, C.c_int(1), null, null, null, C.c_int(4), P._ptr(cam), null, null, null, null) == -1
    assert L.pslfe_pose_optimize(null, null, null, C.c_int(-1), P._ptr(cam), null, null, null) == -1
    assert L.pslfe_pose_edges_from_matches_device(null, C.c_int(0), C.c_int(-1), null, null, C.c_int(0), null, C.c_int(8), null, null, null,
                                                  C.c_int(4)) == -1
    assert L.pslfe_pose_edges_from_matches_device(null, C.c_int(0), C.c_int(0), null, null, C.c_int(0), null, C.c_int(8), null, null, null,
                                                  C.c_int(4)) == 0
    assert L.pslfe_pose_edges_from_matches_device(null, C.c_int(0), C.c_int(1), null, null, C.c_int(0), null, C.c_int(8), null, null, null,
                                                  C.c_int(4)) == -1


def test_host_program_under_sanitizers_equals_restatement(tmp_path):
    """tools/dropin/pose_main.cpp with -DPSL_POSE_HOST_ONLY, host code under -fsanitize=address,undefined, on every case: its plain
    C++ loop equals the restatement in the device's order bit for bit, and the sanitizers stay silent"""
    exe = str(tmp_path / "pose_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPSL_POSE_HOST_ONLY", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "pose_main.cpp")], check=True, capture_output=True)
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = write_cases(path, pc.CASE_NAMES)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        got = read_section(f, cases)
        assert f.read() == b""
    for nm, c, g in zip(pc.CASE_NAMES, cases, got):
        assert_equal_ref(g, c["ref"]["device"], nm)
