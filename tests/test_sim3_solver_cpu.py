"""The restatement of Sim3Solver (tests/sim3_solver_cases.py) on its own - against a float64 Horn solution, its Jacobi against
numpy.linalg.eigh, its atan2 and rand() against the host's libc, its rules - the ABI of the new entry points, and the stand-alone
host program of tools/dropin/sim3_solver_main.cpp (the shared header psl-slam_amd/csrc/sim3_solver_kernels.h compiled for the host)
under the address and undefined-behaviour sanitizers, bit for bit with the restatement.  No GPU."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

import sim3_solver_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# The restatement (float, OpenCV's roundings) against horn_f64 on the hand-built well-conditioned triples of _TRIPLES, the worst over
# the set as test_restatement_agrees_with_the_float64_horn prints it: an entry of R 2.65e-7, an entry of t 1.73e-6, s 4.84e-8.  The
# points are a few metres from the origin, so a coordinate carries a float rounding error of 2^-22 = 2.4e-7 and R, s (ratios of
# differences of such coordinates over a triangle of about a metre) inherit a few of them; t = O1 - s R O2 multiplies the error of
# R by |O2| of about 5 m.  Asserted with a factor 4.
HORN_R, HORN_T, HORN_S = 2.65e-7, 1.73e-6, 4.84e-8
# eigenvalues of the float Jacobi against eigh on symmetric 4x4 matrices with entries of size 1 (the largest eigenvalue is at most
# 4): the worst over 200 matrices is 2.24e-7, about an ulp of a float in [2, 4); asserted with a factor 4
JACOBI_EIGENVALUE = 2.24e-7


def _cam_rec(P, cam):
    rec = np.zeros((), P.CAMERA_DTYPE)
    for k, v in cam.items():
        rec[k] = v
    return rec


def write_cases(path, names, fix_scale, n_iterations, min_inliers=sc.MIN_INLIERS, max_its=sc.MAX_ITS, prob=sc.PROB):
    """cases.bin of tools/dropin/sim3_solver_main.cpp; every case of a file shares fix_scale and the RANSAC parameters"""
    import psl_slam_amd as P
    cases = [sc.case(nm) for nm in names]
    assert all(c["fix_scale"] == fix_scale for c in cases)
    pstride = max(max(len(c["pairs"]) for c in cases), 1)
    with open(path, "wb") as f:
        np.array([len(cases), pstride, int(fix_scale), min_inliers, max_its, n_iterations], np.int32).tofile(f)
        np.array([prob], np.float64).tofile(f)
        _cam_rec(P, cases[0]["cam1"]).tofile(f)
        _cam_rec(P, cases[0]["cam2"]).tofile(f)
        for c in cases:
            np.array([c["seed"]], np.uint32).tofile(f)
            np.array([len(c["pairs"])], np.int32).tofile(f)
            c["pairs"].tofile(f)
            np.ascontiguousarray(c["sigma2"], np.float32).tofile(f)
    return cases


def read_section(f, cases):
    """one section of out.bin -> [(result record, flags, trace)]"""
    out = []
    for c in cases:
        res = np.fromfile(f, sc.RESULT_DTYPE, 1)[0]
        flags = np.fromfile(f, np.uint8, len(c["pairs"]))
        nt = int(np.fromfile(f, np.int32, 1)[0])
        out.append((res, flags, np.fromfile(f, sc.TRACE_DTYPE, nt)))
    return out


def assert_equal_ref(got, ref, what, trace=True):
    """bit for bit: status, iterations, both counts, R, t, s, every flag; with the trace every draw, every hypothesis (R, t, s, T12,
    T21) and every count.  A NaN equals any NaN."""
    res, flags, tr = got
    rres, rflags, rtr = ref
    for k in ("status", "iterations", "ninliers", "best_inliers"):
        assert res[k] == rres[k], (what, k, res, rres)
    for k in ("R", "t", "s"):
        assert sc.same_floats(res["S12"][k], rres["S12"][k]), (what, k, res["S12"], rres["S12"])
    assert (np.asarray(flags) == rflags).all(), (what, np.flatnonzero(np.asarray(flags) != rflags)[:8])
    if trace:
        assert len(tr) == len(rtr), (what, len(tr), len(rtr))
        assert (tr["idx"] == rtr["idx"]).all(), (what, "draws", np.flatnonzero((tr["idx"] != rtr["idx"]).any(1))[:4])
        for k in ("R", "t", "s", "T12", "T21"):
            assert sc.same_floats(tr["h"][k], rtr["h"][k]), (what, k)
        assert (tr["cnt"] == rtr["cnt"]).all(), (what, "counts")


def _names(fix):
    return [nm for nm in sc.CASE_NAMES if sc.CASE_SPECS[nm][3] == fix]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the header's host form as a stand-alone program, host code under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("sim3_solver") / "sim3_solver_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPSL_SIM3_SOLVER_HOST_ONLY", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "sim3_solver_main.cpp")], check=True, capture_output=True)
    return exe


def _run_host(exe, tmp_path, names, fix, n_iterations, tag):
    path, out = str(tmp_path / f"cases_{tag}.bin"), str(tmp_path / f"out_{tag}.bin")
    cases = write_cases(path, names, fix, n_iterations)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        got = read_section(f, cases)
        assert f.read() == b""
    return cases, got


@pytest.mark.parametrize("fix", [False, True])
def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path, fix):
    """every case as one find(): R, t, s, T12, T21 of every hypothesis, every draw, every count, every flag, iterations and status"""
    names = _names(fix)
    cases, got = _run_host(host_exe, tmp_path, names, fix, sc.MAX_ITS, f"find{int(fix)}")
    for nm, c, g in zip(names, cases, got):
        assert_equal_ref(g, c["ref"], nm)


@pytest.mark.parametrize("fix", [False, True])
def test_host_program_in_rounds_of_five_equals_find(host_exe, tmp_path, fix):
    """resumed calls of iterate(5) through (iterations, best_inliers) give what one long call gives, trace included"""
    names = _names(fix)
    cases, got = _run_host(host_exe, tmp_path, names, fix, 5, f"rounds{int(fix)}")
    for nm, c, g in zip(names, cases, got):
        assert_equal_ref(g, c["ref"], nm)


def test_resume_equals_one_long_call_in_the_restatement():
    for nm in ("n65", "n200_it65", "n150_noisy", "n150_noisy_never", "n20", "n19"):
        c = sc.case(nm)
        args = (c["pairs"], c["sigma2"], c["cam1"], c["cam2"], c["fix_scale"], c["seed"])
        for step in (5, 7, 64):
            it = best = 0
            traces = []
            while True:
                res, flags, tr = sc.iterate(*args, step, start_it=it, best_in=best)
                traces.append(tr)
                it, best = int(res["iterations"]), int(res["best_inliers"])
                if res["status"] != 0:
                    break
            assert_equal_ref((res, flags, np.concatenate(traces)), c["ref"], (nm, step))


def test_the_first_qualifying_iteration_is_the_sixth():
    """n65: iterate(5) uses its budget up and returns nothing, bNoMore stays false; the second iterate(5) returns at iteration 6"""
    c = sc.case("n65")
    args = (c["pairs"], c["sigma2"], c["cam1"], c["cam2"], c["fix_scale"], c["seed"])
    r1, f1, t1 = sc.iterate(*args, 5)
    assert r1["status"] == 0 and r1["iterations"] == 5 and r1["ninliers"] == 0 and not f1.any() and len(t1) == 5
    assert r1["best_inliers"] <= sc.MIN_INLIERS and not r1["S12"]["R"].any()
    r2, f2, t2 = sc.iterate(*args, 5, start_it=5, best_in=int(r1["best_inliers"]))
    assert r2["status"] == 1 and r2["iterations"] == 6 and r2["ninliers"] == 40 and len(t2) == 1
    assert (f2 == c["good"]).all()
    # the running best: >= against the best, > against the minimum.  n150_noisy meets a count of exactly 20 on the way
    c = sc.case("n150_noisy")
    cnt = c["ref"][2]["cnt"]
    assert sc.MIN_INLIERS in cnt[:-1] and cnt[-1] == 21 and (cnt[:-1] <= sc.MIN_INLIERS).all()
    assert c["ref"][0]["best_inliers"] == 21 and sc.case("n150_noisy_never")["ref"][0]["best_inliers"] == 17
    # a best carried in above the counts of the call keeps a qualifying count from returning: 21 >= 30 fails at iteration 210
    res, flags, tr = sc.iterate(c["pairs"], c["sigma2"], c["cam1"], c["cam2"], False, c["seed"], 300, start_it=200, best_in=30)
    assert res["status"] == 2 and res["iterations"] == 300 and res["best_inliers"] == 30 and tr["cnt"][9] == 21 and tr["cnt"].max() < 30


def test_bnomore_in_both_places():
    r = sc.case("n19")["ref"][0]
    assert r["status"] == 2 and r["iterations"] == 0                     # N < minInliers: at once
    r = sc.case("n20")["ref"][0]
    assert r["status"] == 2 and r["iterations"] == 1 and r["best_inliers"] == 20 and r["ninliers"] == 0   # 20 is not > 20; the budget of N == min is 1
    r = sc.case("n200_never")["ref"][0]
    assert r["status"] == 2 and r["iterations"] == 300


def test_set_ransac_parameters():
    """N == min gives 1; N == min + 1: epsilon = 20/21 in float, ceil(log(0.01) / log(1 - eps^3)); a budget clipped at 300; the C
    function of the shared header gives the same table (the host program runs the cases with it)"""
    assert sc.max_iterations(20) == 1
    eps = float(np.float32(20) / np.float32(21))
    want = math.ceil(math.log(1 - 0.99) / math.log(1 - eps ** 3))
    assert sc.max_iterations(21) == want == 3
    assert sc.max_iterations(80) == 293 and sc.max_iterations(81) == 300 and sc.max_iterations(5000) == 300
    assert sc.max_iterations(200, max_its=10000) == math.ceil(math.log(0.01) / math.log(1 - float(np.float32(20) / np.float32(200)) ** 3)) == 4603
    assert sc.max_iterations(200, max_its=1000) == 1000
    assert sc.max_iterations(10 ** 9) == 300                             # eps^3 below an ulp of 1: the ratio is infinite
    assert sc.max_iterations(6, min_inliers=6) == 1 and sc.max_iterations(7, 0.99, 6, 2) == 2


def test_draw_follows_the_host_rand():
    """glibc's rand() restated against the host libc's for three seeds, and the draw written with the vector against its definition"""
    libc = C.CDLL(None)
    libc.rand.restype = C.c_int
    for seed in (0, 1, 12345, 0x80000001):
        libc.srand(C.c_uint(seed))
        G = sc.GlibcRand(seed)
        assert [libc.rand() for _ in range(2000)] == [G.rand() for _ in range(2000)], seed
    libc.srand(C.c_uint(77))
    G = sc.GlibcRand(77)
    for N in (3, 4, 20, 21, 65, 1025):
        for _ in range(50):
            want, avail = [], list(range(N))
            for _k in range(3):
                randi = int((float(libc.rand()) / (2147483647.0 + 1.0)) * len(avail))
                want.append(avail[randi])
                avail[randi] = avail[-1]
                avail.pop()
            got = sc.draw(G, N)
            assert got == want and len(set(got)) == 3 and all(0 <= i < N for i in got)
    for r in (0, 1, 2147483647, 1 << 30, 123456789):
        for d in (1, 3, 21, 1025, 2048):
            assert sc.random_int(r, d) == (r * d) >> 31                  # what the shared header computes in integers


def test_the_listed_seeds_are_the_smallest():
    for nm in ("n65", "n200_it65"):
        ds, n, ng, fix, _, target, _ = sc.CASE_SPECS[nm]
        assert sc._seed_for(ds, n, ng, fix, target) == sc.SEEDS[nm]


def test_thresholds_are_truncated_to_integers():
    """mvnMaxError is a vector<size_t>: floor(9.21 sigma2) converted to float.  In n65_truncation a pair of level 0 lies 3.02 px off
    in image 1: its error is between floor(9.21) = 9 and 9.21, so it is no inlier, and it would be one against 9.21"""
    s2 = np.array([1.0, 1.44, 2.0736, sc.LEVEL_SIGMA2[7]], np.float32)
    th = sc.max_error(s2)
    assert th.dtype == np.float32 and list(th) == [9.0, 13.0, 19.0, float(math.floor(9.21 * float(sc.LEVEL_SIGMA2[7])))]
    c = sc.case("n65_truncation")
    res, flags, tr = c["ref"]
    g = int(np.flatnonzero(sc.make_pairs(16, 65, 40, False)[2])[0])
    S = sc.stage(c["pairs"], c["sigma2"], c["cam1"], c["cam2"])
    e1, e2 = sc.errors(S, tr["h"][-1], c["cam1"], c["cam2"])
    assert S["th1"][g] == 9.0 and 9.0 < e1[g] < 9.21 and e2[g] < S["th2"][g] and flags[g] == 0
    assert res["status"] == 1 and res["ninliers"] == 39 and flags.sum() == 39


def test_behind_the_camera_and_nan_pairs_are_no_inliers():
    c = sc.case("n65_behind_nan")
    res, flags, tr = c["ref"]
    b = np.flatnonzero(sc.make_pairs(17, 65, 40, False)[2] == 0)
    assert c["pairs"]["P2c"][b[0], 2] < 0 and np.isnan(c["pairs"]["P1c"][b[1]]).all()
    assert res["status"] == 1 and flags[b[0]] == 0 and flags[b[1]] == 0 and (flags == c["good"]).all()
    # a triple that holds the NaN pair gives a NaN hypothesis and no inlier
    h = sc.hypothesis(c["pairs"]["P1c"][[b[1], 0, 1]].T, c["pairs"]["P2c"][[b[1], 0, 1]].T, False)
    assert np.isnan(h["R"]).all() and sc.inliers(sc.stage(c["pairs"], c["sigma2"], c["cam1"], c["cam2"]), h, c["cam1"], c["cam2"]).sum() == 0


def test_fixed_scale_gives_one_and_the_transpose():
    for nm in _names(True):
        tr = sc.case(nm)["ref"][2]
        for h in tr["h"]:
            if np.isnan(h["R"]).any():
                continue
            assert h["s"].tobytes() == np.float32(1.0).tobytes()
            R, T12, T21 = h["R"].reshape(3, 3), h["T12"].reshape(3, 4), h["T21"].reshape(3, 4)
            assert T12[:, :3].tobytes() == R.tobytes() and T21[:, :3].tobytes() == np.ascontiguousarray(R.T).tobytes()
    assert any(sc.case(nm)["ref"][0]["status"] == 1 for nm in _names(True))


# hand-built triples: the corners of triangles with sides of 0.8 to 3 m, 3 to 7 m in front of the camera, far from collinear
_TRIPLES = [np.array(t, np.float64).T for t in (
    [[0.0, 0.0, 4.0], [1.5, 0.2, 4.5], [0.3, 1.2, 5.0]],
    [[-1.0, -0.5, 3.0], [1.0, -0.4, 3.5], [0.1, 1.0, 6.0]],
    [[0.5, 0.5, 5.0], [-0.7, 0.6, 5.5], [0.4, -0.9, 4.2]],
    [[-1.2, 0.8, 6.5], [1.3, 0.9, 6.0], [0.0, -1.1, 7.0]],
    [[0.2, -0.3, 3.2], [1.0, 0.4, 3.1], [0.3, 0.6, 4.0]],
    [[-0.6, -0.6, 4.4], [0.9, -0.8, 5.6], [0.2, 0.7, 3.6]],
)]
_TRUTHS = [((0.1, -0.2, 0.15), (0.3, -0.1, 0.2), 1.15), ((-0.4, 0.1, 0.3), (-0.2, 0.25, -0.1), 0.9), ((0.02, 0.01, -0.03), (0.05, 0.0, 0.1), 1.0),
           ((1.2, -0.8, 0.5), (0.4, 0.3, -0.3), 1.3)]


def test_restatement_agrees_with_the_float64_horn():
    """well-conditioned triples under four true Sim3s, the scale free and fixed: the float restatement against the float64 closed
    form of the SAME float inputs.  No triple is drawn at random, so none is excluded"""
    worst = np.zeros(3)
    for P2 in _TRIPLES:
        for rv, t, s in _TRUTHS:
            for fix in (False, True):
                st = 1.0 if fix else s
                P2f = P2.astype(np.float32)
                P1f = (st * sc._rodrigues(np.array(rv)) @ P2f.astype(np.float64) + np.array(t)[:, None]).astype(np.float32)
                h = sc.hypothesis(P1f, P2f, fix)
                R, tt, ss = sc.horn_f64(P1f, P2f, fix)
                worst = np.maximum(worst, [np.abs(h["R"].reshape(3, 3) - R).max(), np.abs(h["t"] - tt).max(), abs(float(h["s"]) - ss)])
                # and the closed form recovers the truth the points were built from, to the rounding of the float points
                assert np.abs(R - sc._rodrigues(np.array(rv))).max() < 5e-6 and abs(ss - st) < 5e-6
    print("restatement - float64 Horn, worst R, t, s:", worst)
    assert worst[0] <= 4 * HORN_R and worst[1] <= 4 * HORN_T and worst[2] <= 4 * HORN_S, worst


def test_jacobi_agrees_with_eigh():
    """OpenCV's Jacobi restated against numpy.linalg.eigh on symmetric 4x4 matrices: the eigenvalues within the measured float bound,
    in decreasing order, the eigenvectors as rows (A v = w v), the N of a Horn problem among them"""
    rng = np.random.default_rng(3)
    worst = 0.0
    mats = [rng.uniform(-1, 1, (4, 4)) for _ in range(199)] + [np.diag([3.0, -1.0, 2.0, 0.5])]
    for B in mats:
        A = ((B + B.T) / 2).astype(np.float32)
        W, V, its = sc.jacobi4(A)
        w = np.linalg.eigvalsh(A.astype(np.float64))[::-1]
        assert (np.diff(W) <= 0).all() and its <= 480
        worst = max(worst, float(np.abs(W.astype(np.float64) - w).max()))
        assert np.abs(A.astype(np.float64) @ V.astype(np.float64).T - V.astype(np.float64).T * W.astype(np.float64)).max() < 2e-6
        assert np.abs(V.astype(np.float64) @ V.astype(np.float64).T - np.eye(4)).max() < 2e-6
    print("Jacobi - eigh, worst eigenvalue difference:", worst)
    assert worst <= 4 * JACOBI_EIGENVALUE, worst
    W, V, its = sc.jacobi4(np.diag([3.0, -1.0, 2.0, 0.5]).astype(np.float32))
    assert its == 0 and list(W) == [3.0, 2.0, 0.5, -1.0] and V[0, 0] == 1.0 and V[1, 2] == 1.0 and V[3, 1] == 1.0


def test_atan2_is_within_one_ulp_of_the_host(host_exe):
    """psl_atan2 (the C text, through the host program) on 4e6 samples of [0, 1] x [-1, 1] against the host's atan2: never more than
    one representable double apart.  Measured: 470130 of the 4e6 samples (11.8 %) differ, by one, and for none of them does the float
    (2 ang / nrm) * v that ComputeSim3 forms change.  The numpy text of the same function on a coarser grid, and the
    exact arguments."""
    p = subprocess.run([host_exe, "--atan2", "4000000"], capture_output=True, text=True, timeout=300)
    assert not p.stderr, p.stderr[-2000:]
    rep = json.loads(p.stdout)
    print("psl_atan2 against the host:", rep)
    assert p.returncode == 0 and rep["samples"] == 4000000 and rep["above_one_ulp"] == 0 and rep["worst_ulp"] <= 1
    assert rep["float_flips"] == 0                                       # the count DESIGN.md §3 quotes
    rng = np.random.default_rng(5)
    for y, x in zip(rng.uniform(0, 1, 20000), rng.uniform(-1, 1, 20000)):
        a, b = sc.fdlibm_atan2(float(y), float(x)), math.atan2(y, x)
        assert abs(a - b) <= np.spacing(min(abs(a), abs(b))), (y, x)
    assert sc.fdlibm_atan2(0.0, 1.0) == 0.0 and sc.fdlibm_atan2(0.0, -1.0) == math.pi and sc.fdlibm_atan2(1.0, 0.0) == math.pi / 2
    assert sc.fdlibm_atan2(0.5, 1.0) == sc.fdlibm_atan(0.5) and math.isnan(sc.fdlibm_atan2(float("nan"), 1.0))


def test_a_degenerate_quaternion_gives_a_nan_hypothesis():
    """P1 == P2: N has the eigenvector (1, 0, 0, 0), norm(vec) = 0 and 2 ang vec / norm is 0 / 0: every entry of R is NaN, as in the
    reference, and the hypothesis has no inlier"""
    P = _TRIPLES[0].astype(np.float32)
    h = sc.hypothesis(P, P, False)
    assert np.isnan(h["R"]).all()


def test_abi_and_dtypes():
    import psl_slam_amd as P
    L = P.lib()
    for fn in ("pslfe_sim3_solve_device", "pslfe_sim3_solve", "pslfe_sim3_pairs_sigma2_from_matches_device", "pslfe_sim3_pairs_from_matches_device"):
        assert hasattr(L, fn), fn
    assert P.SIM3SOLVERRESULT_DTYPE == sc.RESULT_DTYPE and P.SIM3SOLVERRESULT_DTYPE.itemsize == 68 and P.SIM3PAIR_DTYPE.itemsize == 48
    assert sc.HYP_DTYPE.itemsize == 37 * 4 and sc.TRACE_DTYPE.itemsize == 41 * 4
    for m in ("SetRansacParameters", "iterate", "find", "GetEstimatedRotation", "GetEstimatedTranslation", "GetEstimatedScale", "SolveDevice",
              "ComputeSim3Candidates"):
        assert hasattr(P.Sim3Solver, m), m
    assert hasattr(P.Optimizer, "Sim3PairsSigma2FromMatchesDevice")
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslSim3SolverResult) == 68" in hdr and "sizeof(PslSim3Pair) == 48" in hdr
    # the argument checks that need no device: counts and parameters first, then an empty call, then the arrays
    cam = np.zeros(1, P.CAMERA_DTYPE)
    null, cm = C.c_void_p(None), P._ptr(cam)
    f = L.pslfe_sim3_solve_device

    def call(ncand=1, pstride=4, prob=0.99, mn=20, mx=300, nit=5, cam1=cm, cam2=cm):
        return f(null, C.c_int(ncand), null, null, null, C.c_int(pstride), cam1, cam2, C.c_double(prob), C.c_int(mn), C.c_int(mx), C.c_int(0),
                 C.c_uint32(1), null, null, C.c_int(nit), null, null)
    assert call(ncand=-1) == -1 and call(pstride=-1) == -1 and call(mn=2) == -1 and call(mx=0) == -1 and call(nit=-1) == -1
    assert call(prob=0.0) == -1 and call(prob=1.0) == -1 and call(prob=float("nan")) == -1
    assert call(ncand=0) == 0 and call() == -1
    h = L.pslfe_sim3_solve
    res = np.zeros(1, P.SIM3SOLVERRESULT_DTYPE)

    def one(n=4, prob=0.99, mn=20, start=0, best=0):
        return h(null, null, null, C.c_int(n), cm, cm, C.c_double(prob), C.c_int(mn), C.c_int(300), C.c_int(0), C.c_uint32(1), C.c_int(start),
                 C.c_int(best), C.c_int(5), P._ptr(res), null)
    assert one(n=-1) == -1 and one(prob=2.0) == -1 and one(mn=1) == -1 and one(start=-1) == -1 and one(best=-1) == -1 and one() == -1
    g = L.pslfe_sim3_pairs_sigma2_from_matches_device
    s2 = np.ones(8, np.float32)
    a = lambda ncand, ps: g(null, C.c_int(0), null, null, C.c_int(ncand), null, null, null, C.c_int(4), null, null, C.c_int(4), null, null,
                            P._ptr(s2), C.c_int(8), null, null, null, C.c_int(ps), P._ptr(s2), null)
    assert a(-1, 4) == -1 and a(1, -1) == -1 and a(0, 4) == 0 and a(1, 4) == -1
