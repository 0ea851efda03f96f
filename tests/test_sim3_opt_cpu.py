"""The restatement of Optimizer::OptimizeSim3 (tests/sim3_opt_cases.py) on its own, the restatement pinned against what it returned
while it had its own copy of the Levenberg loop, the ABI of the three entry points, and the stand-alone host program of tools/dropin/sim3_main.cpp under the address and undefined-behaviour sanitizers.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the largest difference of an output double (q, t, s) between the device's order of the sums and g2o's edge order, measured over
# every case of the set by test_order_difference_is_the_documented_one: 3.61e-8 (the numeric Jacobian turns a last-bit difference
# of a sum into a 1e-5 relative difference of a Jacobian entry, so the orders part ways far earlier than in the pose optimisation,
# whose figure is 3.73e-9 in a float)
ORDER_DIFFERENCE = 3.61e-8
# numeric against analytic Jacobian, measured over the case set by test_numeric_jacobian_agrees_with_the_analytic_one: 1.46e-4 px per
# unit of the update.  An error below 1024 px carries a rounding error of a few ulp(1024) = 1.1e-13; the central difference divides
# the difference of two of them by 2e-9, so 8 ulp give 8 * 1.1e-13 * 5e8 = 4.5e-4.
JACOBIAN_TOLERANCE = 4.5e-4


def write_cases(path, names, fix_scale):
    """cases.bin of tools/dropin/sim3_main.cpp; every case of a file shares fix_scale"""
    import psl_slam_amd as P
    cases = [sc.case(nm) for nm in names]
    assert all(c["fix_scale"] == fix_scale for c in cases)
    pstride = max(max(len(c["pairs"]) for c in cases), 1)
    cams = []
    for cam in (cases[0]["cam1"], cases[0]["cam2"]):
        rec = np.zeros((), P.CAMERA_DTYPE)
        for k, v in cam.items():
            rec[k] = v
        cams.append(rec)
    with open(path, "wb") as f:
        np.array([len(cases), pstride, int(fix_scale)], np.int32).tofile(f)
        np.array([sc.TH2], np.float32).tofile(f)
        cams[0].tofile(f)
        cams[1].tofile(f)
        for c in cases:
            c["S12"].tofile(f)
            np.array([len(c["pairs"])], np.int32).tofile(f)
            c["pairs"].tofile(f)
    return cases


def read_section(f, cases):
    """one section of out.bin -> [(S12_out, bad, nin, info)]"""
    out = []
    for c in cases:
        S = np.fromfile(f, sc.SIM3D_DTYPE, 1)[0]
        nin = int(np.fromfile(f, np.int32, 1)[0])
        info = np.fromfile(f, sc.INFO_DTYPE, 1)[0]
        out.append((S, np.fromfile(f, np.uint8, len(c["pairs"])), nin, info))
    return out


def assert_equal_ref(got, ref, what, info=True):
    """bit for bit: the 8 doubles, the flags, the return value, the calls and iterations and the branches taken"""
    S, bad, nin, inf = got
    rS, rbad, rnin, rinf = ref
    assert S.tobytes() == rS.tobytes(), (what, sc.sim3_doubles(S), sc.sim3_doubles(rS))
    assert nin == rnin, (what, nin, rnin)
    assert (np.asarray(bad) == rbad).all(), (what, np.flatnonzero(np.asarray(bad) != rbad)[:8])
    if info:
        assert inf.tobytes() == rinf.tobytes(), (what, inf, rinf)


def _names(fix):
    return [nm for nm in sc.CASE_NAMES if sc.case(nm)["fix_scale"] == fix]


def _true_system(c):
    """H (7x7) of the pairs at the TRUE Sim3 without the robust kernel, and the sum of the information weights"""
    E = sc._Pairs(c["pairs"], c["cam1"], c["cam2"], np.float32(1e30))      # th2 so large that rho' = 1
    S = sc.s3_from_rts(c["Strue"])
    Si = sc.s3_inverse(S)
    pert = sc.s3_perturbed(S, False)
    acc = sc.sum_edge(np.stack([E.terms(0, S, Si, pert), E.terms(1, S, Si, pert)], 1), np.ones(E.n, bool))
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = acc[:28]
    return H + np.triu(H, 1).T, float(E.is2[0].sum() + E.is2[1].sum())


@pytest.mark.parametrize("name", ["n300_0_free_noisefree", "n300_0_fixed_noisefree"])
def test_noise_free_case_recovers_the_true_sim3(name):
    """300 pairs without noise, started 2 degrees, 5 cm and (free scale) 3 % off.  The observations are the projections under the
    true Sim3 rounded to float, so what keeps the minimum from the truth is that rounding: below 1024 px a coordinate is off by at
    most d = 2^-15 px.  To first order the minimum moves by dx = (A^T A)^-1 A^T r with A = W^1/2 J at the true Sim3 and r the weighted
    rounding errors, so |dx| <= |r| / sqrt(lambda_min(H)), H = A^T A, |r|^2 <= 2 d^2 sum(invSigma2) over both edges of every pair.  H
    comes from the Jacobians at the TRUE Sim3, not from a result (with the scale fixed, from its 6x6 block).  An entry of R then
    differs by at most |dx|, an entry of t by at most |dx| (1 + |t|) (upsilon, omega x t and sigma t), s by at most s |dx|.  A factor
    2 is allowed for the second-order terms and for the point at which the Levenberg rule stops; that factor is an assumption,
    not derived (tests/test_pose_opt_cpu.py makes the same one)."""
    c = sc.case(name)
    S, bad, nin, info = c["ref"]["device"]
    assert nin == 300 and not bad.any() and info["calls"] == 2
    H, wsum = _true_system(c)
    if c["fix_scale"]:
        H = H[:6, :6]
    dx = np.sqrt(2.0 * wsum) * 2.0 ** -15 / np.sqrt(np.linalg.eigvalsh(H)[0])
    T = c["Strue"]
    Rt, tt, st = T["R"].astype(np.float64).reshape(3, 3), T["t"].astype(np.float64), float(T["s"])
    tol_R, tol_t, tol_s = 2 * dx, 2 * dx * (1 + np.linalg.norm(tt)), 2 * dx * st
    assert tol_R < 2e-5 and tol_t < 5e-5          # the start is more than 1e-2 off (below)
    R, t, s = sc.s3_matrix((list(S["q"]), list(S["t"]), float(S["s"])))
    R0, t0, s0 = sc.s3_matrix(sc.s3_from_rts(c["S12"]))
    assert np.abs(R0 - Rt).max() > 1e-2 and np.abs(t0 - tt).max() > 1e-2
    assert np.abs(R - Rt).max() < tol_R and np.abs(t - tt).max() < tol_t, (np.abs(R - Rt).max(), tol_R, np.abs(t - tt).max(), tol_t)
    if c["fix_scale"]:
        assert s == s0 == st
    else:
        assert abs(s0 - st) > 1e-2 and abs(s - st) < tol_s, (abs(s - st), tol_s)      # a free scale of 1.1 is recovered
        assert abs(st - 1.1) < 1e-7


def _analytic_jacobian(E, side, S):
    """d e / d update of one edge of every pair for the left update exp(update) * S: [2][7][n].  side 0: p = S.map(X), dp = [-[p]x, I,
    p]; side 1: p = S^-1.map(X), dp = (1/s) R^T [[X]x, -I, -X]."""
    R, t, s = sc.s3_matrix(S)
    X = np.stack(E.X[side], 1)
    fx, fy, cx, cy = E.K[side]
    n = len(X)
    dp = np.zeros((n, 3, 7))
    if side == 0:
        p = s * X @ R.T + t
        dp[:, 0, 1], dp[:, 0, 2], dp[:, 1, 0], dp[:, 1, 2], dp[:, 2, 0], dp[:, 2, 1] = p[:, 2], -p[:, 1], -p[:, 2], p[:, 0], p[:, 1], -p[:, 0]
        dp[:, :, 3:6] = np.eye(3)
        dp[:, :, 6] = p
    else:
        p = ((X - t) @ R) / s
        M = np.zeros((n, 3, 7))
        M[:, 0, 1], M[:, 0, 2], M[:, 1, 0], M[:, 1, 2], M[:, 2, 0], M[:, 2, 1] = -X[:, 2], X[:, 1], X[:, 2], -X[:, 0], -X[:, 1], X[:, 0]
        M[:, :, 3:6] = -np.eye(3)
        M[:, :, 6] = -X
        dp = np.einsum("ij,njk->nik", R.T / s, M)
    J = np.zeros((2, 7, n))
    J[0] = -(fx * (dp[:, 0, :] / p[:, 2:3] - p[:, 0:1] * dp[:, 2, :] / p[:, 2:3] ** 2)).T
    J[1] = -(fy * (dp[:, 1, :] / p[:, 2:3] - p[:, 1:2] * dp[:, 2, :] / p[:, 2:3] ** 2)).T
    return J


def test_numeric_jacobian_agrees_with_the_analytic_one():
    """g2o's central differences with delta = 1e-9 against the derivative of the same error, at the start of every case with pairs"""
    worst = 0.0
    for nm in sc.CASE_NAMES:
        c = sc.case(nm)
        if len(c["pairs"]) == 0 or "behind" in nm:
            continue
        E = sc._Pairs(c["pairs"], c["cam1"], c["cam2"], sc.TH2)
        S = sc.s3_from_rts(c["S12"])
        pert = sc.s3_perturbed(S, False)
        for side in (0, 1):
            Jn = np.array(E.jacobian(side, pert))
            Ja = _analytic_jacobian(E, side, S)
            worst = max(worst, float(np.abs(Jn - Ja).max()))
    print("numeric - analytic Jacobian, largest entry difference:", worst)
    assert worst <= JACOBIAN_TOLERANCE, worst


def test_a_fixed_scale_gives_a_zero_seventh_column_and_keeps_its_bits():
    c = sc.case("n65_0_fixed")
    E = sc._Pairs(c["pairs"], c["cam1"], c["cam2"], sc.TH2)
    S = sc.s3_from_rts(c["S12"])
    pert = sc.s3_perturbed(S, True)
    for side in (0, 1):
        J = E.jacobian(side, pert)
        assert (J[0][6] == 0).all() and (J[1][6] == 0).all()
    for nm in sc.CASE_NAMES:
        c = sc.case(nm)
        if c["fix_scale"]:
            for order in ("device", "edge"):
                assert float(c["ref"][order][0]["s"]) == float(np.float32(c["S12"]["s"])), nm


@pytest.mark.parametrize("name", [nm for nm, spec in sc.CASE_SPECS.items() if spec[0] >= 64 and "behind" not in nm])
def test_flags_equal_the_planted_outliers(name):
    """from 64 pairs on the inliers outvote the planted pairs (20 to 60 px off, against 0.5 px of noise) in every case of the set"""
    c = sc.case(name)
    for order in ("device", "edge"):
        _, bad, nin, _ = c["ref"][order]
        assert (bad == c["planted"]).all(), (order, np.flatnonzero(bad != c["planted"]))
        assert nin == len(c["planted"]) - int(c["planted"].sum())


def test_fewer_than_ten_pairs_return_zero_and_keep_the_sim3():
    """0 pairs: nothing runs.  1 and 9 pairs: the first call runs and classifies, then 0.  11 pairs of which 3 leave: 0 after the
    removal.  10 and 11 pairs without outliers: both calls.  Where 0 is returned before the write-back, the Sim3 is Sim3(R, t, s)."""
    for fix in ("fixed", "free"):
        for nm, calls, zero in ((f"n0_0_{fix}", 0, True), (f"n1_0_{fix}", 1, True), (f"n9_0_{fix}", 1, True), (f"n9_30_{fix}", 1, True),
                                (f"n10_0_{fix}", 2, False), (f"n10_30_{fix}", 1, True), (f"n11_0_{fix}", 2, False), (f"n11_30_{fix}", 1, True)):
            c = sc.case(nm)
            for order in ("device", "edge"):
                S, bad, nin, info = c["ref"][order]
                assert info["calls"] == calls, (nm, info)
                start = sc.s3_record(sc.s3_from_rts(c["S12"]))
                if zero:
                    assert nin == 0 and S.tobytes() == start.tobytes(), nm
                    assert info["iterations"][1] == 0 and (calls == 0 or info["iterations"][0] >= 1)
                else:
                    assert nin == len(c["pairs"]) and S.tobytes() != start.tobytes(), nm
    assert sc.case("n11_30_free")["ref"]["device"][1].sum() == 3       # the flags of the first test stay although 0 is returned


def test_five_more_iterations_without_outliers_ten_with():
    """nBad == 0 after the first call: optimize(5); otherwise optimize(10) (:2960-2964).  In most cases Terminate ends the second call
    first; the two limit cases are those in which the limit decides.  n100_0_free_limit5: no pair leaves and the second call runs
    exactly 5 iterations, where a limit of 10 would run more.  n100_30_free_limit10: pairs leave and the second call runs more than 5
    iterations, where a limit of 5 would stop it.  Both are in CASE_NAMES, so the kernel and the host loop are compared with them bit
    for bit: a driver that always allowed 5, or always 10, differs in the iterations and in the Sim3 of one of them."""
    for nm, spec in sc.CASE_SPECS.items():
        info = sc.case(nm)["ref"]["device"][3]
        assert info["iterations"][0] <= 5
        assert info["iterations"][1] <= (10 if sc.case(nm)["ref"]["device"][1].any() else 5), nm
    c5, c10 = sc.case("n100_0_free_limit5"), sc.case("n100_30_free_limit10")
    for order in ("device", "edge"):
        S, bad, nin, info = c5["ref"][order]
        assert not bad.any() and nin == 100 and info["calls"] == 2 and info["iterations"][1] == 5
        always10 = sc.run_case(c5, order, 10)
        assert always10[3]["iterations"][1] > 5 and always10[0].tobytes() != S.tobytes()
        S, bad, nin, info = c10["ref"][order]
        assert bad.any() and info["calls"] == 2 and 5 < info["iterations"][1] <= 10
        always5 = sc.run_case(c10, order, 5)
        assert always5[3]["iterations"][1] == 5 and always5[0].tobytes() != S.tobytes()


def test_exact_data_end_both_calls_after_one_iteration():
    """chi2 = 0 and b = 0 give a zero step and rho == 0: Terminate in the first iteration of both calls; the Sim3 keeps its bits"""
    c = sc.case("exact")
    for order in ("device", "edge"):
        S, bad, nin, info = c["ref"][order]
        assert info["calls"] == 2 and (info["iterations"] == 1).all() and nin == len(c["pairs"]) and not bad.any()
        assert S.tobytes() == sc.s3_record(sc.s3_from_rts(c["S12"])).tobytes()


def test_every_branch_of_the_exponential_is_taken_in_a_trial_step():
    """bit (|sigma| >= 1e-5) * 2 + (theta >= 1e-5) of exp_branches; the perturbations of the numeric Jacobian (always branch 0) are not
    counted"""
    assert sc.case("n40_0_fixed_tiny_rotation")["ref"]["device"][3]["exp_branches"] & 1          # both small
    assert sc.case("n65_0_fixed")["ref"]["device"][3]["exp_branches"] & 2                        # sigma = 0, a real rotation
    assert sc.case("n40_0_free_tiny_rotation")["ref"]["device"][3]["exp_branches"] & 4           # a scale step, a rotation below 1e-5
    assert sc.case("n65_0_free")["ref"]["device"][3]["exp_branches"] & 8                         # both large
    for br, x in ((0, [1e-6, 0, 0, 1, 2, 3, 1e-6]), (1, [0.1, 0.2, -0.1, 1, 2, 3, 0.0]), (2, [1e-6, 0, 0, 1, 2, 3, 0.02]), (3, [0.1, 0.2, -0.1, 1, 2, 3, 0.02])):
        S, b = sc.s3_exp([float(v) for v in x])
        assert b == br
        # against the closed form: s = e^sigma, R = exp(omega), t = W upsilon with W = int_0^1 e^(sigma u) exp(u omega) du
        us = (np.arange(20000) + 0.5) / 20000
        W = sum(np.exp(x[6] * u) * sc._rodrigues(np.array(x[:3]) * u) for u in us) / len(us)
        R, t, s = sc.s3_matrix(S)
        assert abs(s - np.exp(x[6])) < 1e-15 and np.abs(R - sc._rodrigues(np.array(x[:3]))).max() < 1e-9
        # below eps = 1e-5 sim3.h takes the limit (C = 1, A = 1/2, B = 1/6, or the theta -> 0 forms): off by at most eps |upsilon|
        tol = 1e-7 if br in (1, 3) else 1e-5 * float(np.linalg.norm(x[3:6]))
        assert np.abs(t - W @ np.array(x[3:6])).max() < tol


def test_fdlibm_exp_is_within_one_ulp_of_the_host():
    xs = np.concatenate([np.linspace(-2.0, 2.0, 4001), [0.0, -0.0, 1e-9, -1e-9, 3e-9, 1e-5, -1e-5, 0.3465, 0.35, 1.03, 1.04, 700.0, -700.0]])
    for x in xs:
        a, b = sc.fdlibm_exp(float(x)), float(np.exp(x))
        assert abs(a - b) <= np.spacing(b), x
    assert sc.fdlibm_exp(0.0) == 1.0 and sc.fdlibm_exp(-0.0) == 1.0 and sc.fdlibm_exp(1e-9) == 1.0 + 1e-9


def test_the_behind_case_has_a_point_behind_the_camera():
    c = sc.case("n65_0_free_behind")
    S = sc.s3_from_rts(c["S12"])
    assert sc.s3_map(S, [float(v) for v in c["pairs"]["P2c"][-1]])[2] < -1.0
    assert c["ref"]["device"][1][-1] == 1 and c["ref"]["device"][2] == 64


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_both_orders_give_the_same_flags_and_return_value(name):
    """every case of the GPU test; the builder has rejected seeds with a tested chi2 within a relative 1e-6 of th2"""
    c = sc.case(name)
    d, e = c["ref"]["device"], c["ref"]["edge"]
    assert d[2] == e[2] and d[3]["calls"] == e[3]["calls"] and (d[1] == e[1]).all()
    if name != "exact":
        for order in ("device", "edge"):
            assert sc.run_case(c, order)[4] > sc.MARGIN


def test_order_difference_is_the_documented_one():
    d = sc.order_difference()
    print("largest difference of an output double between the two orders:", d)
    assert d <= ORDER_DIFFERENCE


def test_the_shared_loop_returns_what_the_written_out_loop_returned():
    """tests/golden/sim3_restatement_pins.npz holds what sim3_opt_cases.optimize returned while the iterations, the trials and solve7
    were written out in it (tests/golden/make_golden.py sim3_pins, run on that code): the bytes of S12_out, bad, info and of the margin
    as a float64, and nin.  On lm_cases.levenberg it returns the same bits on every case in both orders."""
    pins = np.load(os.path.join(ROOT, "tests", "golden", "sim3_restatement_pins.npz"))
    checked = 0
    for nm in sc.CASE_NAMES:
        c = sc.case(nm)
        for order in ("device", "edge"):
            S, bad, nin, info, margin = sc.run_case(c, order)
            key = f"{nm}/{order}"
            assert S.tobytes() == pins[key + "/S12_out"].tobytes(), key
            assert bad.dtype == np.uint8 and bad.tobytes() == pins[key + "/bad"].tobytes(), key
            assert nin == int(pins[key + "/nin"]) and info.tobytes() == pins[key + "/info"].tobytes(), key
            assert np.float64(margin).tobytes() == pins[key + "/margin"].tobytes(), (key, margin)
            checked += 1
    assert checked == 2 * len(sc.CASE_NAMES) and len(pins.files) == 10 * len(sc.CASE_NAMES)


def test_abi_and_dtypes():
    import psl_slam_amd as P
    L = P.lib()
    for fn in ("pslfe_sim3_optimize_device", "pslfe_sim3_optimize", "pslfe_sim3_pairs_from_matches_device"):
        assert hasattr(L, fn), fn
    assert P.SIM3_DTYPE == sc.SIM3_DTYPE and P.SIM3D_DTYPE == sc.SIM3D_DTYPE and P.SIM3PAIR_DTYPE == sc.PAIR_DTYPE and P.SIM3INFO_DTYPE == sc.INFO_DTYPE
    assert hasattr(P.Optimizer, "OptimizeSim3") and hasattr(P.Optimizer, "OptimizeSim3Device")
    # the argument checks that need no device: counts first, then an empty call, then the arrays
    cam = np.zeros(1, P.CAMERA_DTYPE)
    null, th2 = C.c_void_p(None), C.c_float(10.0)
    f = L.pslfe_sim3_optimize_device
    assert f(null, C.c_int(-1), null, null, null, C.c_int(4), P._ptr(cam), P._ptr(cam), th2, C.c_int(0), null, null, null, null) == -1
    assert f(null, C.c_int(1), null, null, null, C.c_int(-1), P._ptr(cam), P._ptr(cam), th2, C.c_int(0), null, null, null, null) == -1
    assert f(null, C.c_int(0), null, null, null, C.c_int(4), P._ptr(cam), P._ptr(cam), th2, C.c_int(0), null, null, null, null) == 0
    assert f(null, C.c_int(1), null, null, null, C.c_int(4), P._ptr(cam), P._ptr(cam), th2, C.c_int(0), null, null, null, null) == -1
    assert L.pslfe_sim3_optimize(null, null, null, C.c_int(-1), P._ptr(cam), P._ptr(cam), th2, C.c_int(0), null, null, null) == -1
    assert L.pslfe_sim3_optimize(null, null, null, C.c_int(4), P._ptr(cam), P._ptr(cam), th2, C.c_int(0), null, null, null) == -1
    g = L.pslfe_sim3_pairs_from_matches_device
    s2 = np.ones(8, np.float32)
    a = lambda ncand, n1, mp2s, ps: g(null, C.c_int(0), null, null, C.c_int(ncand), null, null, null, C.c_int(n1), null, null, C.c_int(mp2s), null, null,
                                      P._ptr(s2), C.c_int(8), null, null, null, C.c_int(ps))
    assert a(-1, 4, 4, 4) == -1 and a(1, -1, 4, 4) == -1 and a(1, 4, -1, 4) == -1 and a(1, 4, 4, -1) == -1
    assert a(0, 4, 4, 4) == 0 and a(1, 4, 4, 4) == -1


def test_host_program_under_sanitizers_equals_restatement(tmp_path):
    """tools/dropin/sim3_main.cpp with -DPSL_SIM3_HOST_ONLY, host code under -fsanitize=address,undefined, on every case: its plain
    C++ loop equals the restatement in the device's order bit for bit - the 8 doubles, the flags, the return value, the calls, the
    iterations and the branches - and the sanitizers stay silent"""
    exe = str(tmp_path / "sim3_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPSL_SIM3_HOST_ONLY", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "sim3_main.cpp")], check=True, capture_output=True)
    for fix in (True, False):
        names = _names(fix)
        path, out = str(tmp_path / f"cases{int(fix)}.bin"), str(tmp_path / f"out{int(fix)}.bin")
        cases = write_cases(path, names, fix)
        p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        with open(out, "rb") as f:
            got = read_section(f, cases)
            assert f.read() == b""
        for nm, c, g in zip(names, cases, got):
            assert_equal_ref(g, c["ref"]["device"], nm)
