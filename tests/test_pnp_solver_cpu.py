"""The restatement of PnPsolver (tests/pnp_cases.py) and the stand-alone host program of tools/dropin/pnp_main.cpp (the shared header
psl-slam_amd/csrc/pnp_solver_kernels.h compiled for the host, under the address and undefined-behaviour sanitizers), bit for bit with
each other; the Jacobi reading against LAPACK; the budget table; the draw; the ABI.  No GPU.

The Jacobi reading against an independent SVD (test_jacobi_reading_against_lapack): on the noise-free, non-planar scenes of
_CLEAN_SCENES the poses of find() are compared with the ground truth, once with this library's reading of OpenCV's Jacobi SVD and once
with numpy.linalg.svd / pinv / lstsq in its place (pnp_cases.USE_LAPACK).  Measured here on the CPU, the worst entry over the scenes:
    LAPACK variant   R 3.37e-08   t 1.22e-07
    Jacobi reading   R 3.51e-08   t 1.80e-07
(the returned pose is a float matrix, so both carry its rounding, 6e-8 at entries near 1, and the 3e-5 px rounding of the float pixels).
The bound for the reading is the LAPACK variant's worst deviation times 8, for the different order of rotations: R 2.70e-07, t 9.76e-07
(DESIGN.md §3).  The test computes the LAPACK figure again and asserts against 8 times what it finds, and against the recorded bound."""
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LAPACK_R, LAPACK_T, MARGIN = 3.37e-08, 1.22e-07, 8.0
# (data seed, rows): every row consistent, points in a box, no noise beyond the float pixels
_CLEAN_SCENES = [(5, 15), (6, 63), (31, 20), (32, 30), (33, 40), (34, 100), (35, 12), (36, 25)]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the header's host form as a stand-alone program, host code under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("pnp_solver") / "pnp_host")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPSL_PNP_HOST_ONLY", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "pnp_main.cpp")], check=True, capture_output=True)
    return exe


def _run_host(exe, tmp_path, names, mode):
    import psl_slam_amd as P
    path, out = str(tmp_path / f"cases_{mode}.bin"), str(tmp_path / f"out_{mode}.bin")
    cases = [pc.case(nm) for nm in names]
    pc.write_cases(path, cases, mode, P.CAMERA_DTYPE)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        got = pc.read_section(f, cases)
        assert f.read() == b""
    return cases, got


@pytest.mark.parametrize("mode", ["find", "rounds"])
def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path, mode):
    """every case as one find(), and as rounds of iterate(n) on one solver with poses refused in between: status, iterations, the
    counts, min_inliers, both poses, every flag of every call, and mvbBestInliers at the end"""
    cases, got = _run_host(host_exe, tmp_path, pc.CASE_NAMES, mode)
    for nm, c, g in zip(pc.CASE_NAMES, cases, got):
        pc.assert_play_equal(g, c[mode], nm)


def test_cases_are_what_their_names_say():
    st = {nm: int(pc.case(nm)["find"][0][-1][0]["status"]) for nm in pc.CASE_NAMES}
    for nm in ("n3", "n5", "n9"):                                        # N < mRansacMinInliers: bNoMore, nothing solved
        r = pc.case(nm)["find"][0][-1][0]
        assert st[nm] == 2 and r["iterations"] == 0 and not pc.case(nm)["find"][2]
    r = pc.case("n4_min4")["find"][0][-1][0]
    assert (int(r["iterations"]), int(r["min_inliers"]), int(r["best_inliers"])) == (1, 4, 4) and st["n4_min4"] == 3
    assert sorted(pc.case("n4_min4")["find"][2][0][1]) == [0, 1, 2, 3]  # all four drawn
    assert st["n15"] == st["n63"] == st["n385_half"] == st["planar30"] == st["behind30"] == 1
    assert st["n60_fifth"] == 3 and st["n60_fifth_none"] == 2 and st["identical20"] == 2
    assert st["n384_half"] == 3 and st["n400_half"] == 3
    tr = pc.case("n64_half")["find"][2]
    assert [e[0] for e in tr if e[4] is not None][0] == 17              # the first qualifying hypothesis opens the second block of 16
    # a Refine that fails at == min_inliers, a later one that succeeds
    tr, mn = pc.case("noisy40_eq")["find"][2], int(pc.case("noisy40_eq")["find"][0][-1][0]["min_inliers"])
    ref = [e for e in tr if e[4] is not None]
    assert ref[0][4] == mn and ref[-1][4] > mn and ref[-1][0] > ref[0][0]
    # a qualifying hypothesis that is not a new best, and Refine runs all the same (after a pose that was refused)
    tr = pc.case("noisy40_notbest")["rounds"][2]
    assert any(e[4] is not None and not e[3] for e in tr)
    assert [int(r["status"]) for r, _ in pc.case("noisy40_notbest")["rounds"][0]] == [1, 1, 3]
    # the budget ends inside the first block of 16, on its last hypothesis, and one past it; the last iteration is the one that qualifies
    for nm, its in (("its15", 15), ("its16", 16), ("its17", 17)):
        c = pc.case(nm)
        assert int(c["find"][0][-1][0]["iterations"]) == its and st[nm] == 3 and [e[0] for e in c["find"][2] if e[4] is not None] == [its]
    behind = pc.case("behind30")
    R, t = pc.ground_truth(16)
    z = np.stack([behind["rows"][k] for k in ("X", "Y", "Z")], 1).astype(np.float64) @ R[2] + t[2]
    assert (z < 0).sum() == 1


def test_rounds_equal_find_when_nothing_is_refused():
    """a first call that ends by budget equals find(); rounds of iterate(5) up to the first pose give the same pose as find()"""
    for nm in ("n60_fifth", "its17", "n64_half", "n385_half", "noisy40_eq"):
        c = pc.case(nm)
        calls, bf, _ = pc.play(c["rows"], c["cam"], c["seed"], c["params"], 5, 0)
        assert len(calls) == 1                                           # the loop's || runs a first call on to mRansacMaxIts
        pc.assert_play_equal((calls, bf), c["find"], nm)


def _pose_dev(res, data_seed):
    R, t = pc.ground_truth(data_seed)
    return (np.abs(res["Tcw"]["R"].astype(np.float64).reshape(3, 3) - R).max(), np.abs(res["Tcw"]["t"].astype(np.float64) - t).max())


def test_jacobi_reading_against_lapack():
    worst = {}
    for lapack in (True, False):
        pc.USE_LAPACK = lapack
        try:
            devs = []
            for ds, n in _CLEAN_SCENES:
                rows, good = pc.make_rows(ds, n, n)
                calls, _, _ = pc.play(rows, pc.CAM, 100 + ds, pc.RELOC, 300, 0)
                res, flags = calls[-1]
                assert res["status"] & 1 and flags.all() and res["inliers"] == n, (lapack, ds, res)   # every row an inlier: a condition
                devs.append(_pose_dev(res, ds))
        finally:
            pc.USE_LAPACK = False
        worst[lapack] = (max(d[0] for d in devs), max(d[1] for d in devs))
    print("LAPACK variant R %.3g t %.3g; Jacobi reading R %.3g t %.3g" % (worst[True] + worst[False]))
    assert worst[False][0] <= MARGIN * worst[True][0] and worst[False][1] <= MARGIN * worst[True][1]
    assert worst[False][0] <= MARGIN * LAPACK_R and worst[False][1] <= MARGIN * LAPACK_T


def _budget(N, prob, min_inliers, max_its, min_set, epsilon):
    """src/PnPsolver.cc:134-152 as written, in numpy float32 / float64"""
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps)                                     # int nMinInliers = N*mRansacEpsilon
    if n_min < min_inliers:
        n_min = min_inliers
    if n_min < min_set:
        n_min = min_set
    if eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    if n_min == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(np.float64(1) - np.float64(prob)) / np.log(np.float64(1) - np.power(np.float64(eps), 3)))
        n_it = int(v) if np.isfinite(v) and v < max_its else max_its
    return max(1, min(n_it, max_its)), n_min


def test_budget_table_equals_the_expressions():
    import psl_slam_amd as P
    sets = [(0.99, 8, 300, 4, 0.4), (0.99, 10, 300, 4, 0.5)]
    for ps in sets:
        for N in range(1, 401):
            want = _budget(N, *ps)
            assert P.PnPsolver.RansacParameters(N, *ps) == want == pc.ransac_parameters(N, *ps), (ps, N)
    assert P.PnPsolver.RansacParameters(10, 0.99, 10, 300, 4, 0.5) == (1, 10)          # N == minInliers
    assert P.PnPsolver.RansacParameters(9, 0.99, 10, 300, 4, 0.5)[1] == 10             # N < minInliers: iterate leaves at once
    assert P.PnPsolver.RansacParameters(50, 0.99, 10, 300, 4, 1.0) == (1, 50)          # epsilon = 1: nMinInliers == N
    assert P.PnPsolver.RansacParameters(50, 0.99, 2, 300, 4, 0.01) == _budget(50, 0.99, 2, 300, 4, 0.01) == (300, 4)   # the minSet clamp
    its = [P.PnPsolver.RansacParameters(N, *sets[1])[0] for N in range(20, 401)]
    assert set(its) == {35}                                              # ceil(log(0.01) / log(1 - 0.5^3))
    for bad in ((0.0, 10, 300, 4, 0.5), (0.99, 10, 0, 4, 0.5), (0.99, 10, 300, 3, 0.5), (0.99, 10, 300, 5, 0.5), (0.99, -1, 300, 4, 0.5),
                (0.99, 10, 300, 4, float("nan"))):
        with pytest.raises(P.PslfeError):
            P.PnPsolver.RansacParameters(20, *bad)


@pytest.mark.parametrize("N", [4, 5, 6, 7, 300])
def test_draw_equals_swap_and_pop(host_exe, tmp_path, N):
    out, seed, its = str(tmp_path / "draw.bin"), 1234 + N, 10000
    p = subprocess.run([host_exe, "--draw", str(N), str(seed), str(its), out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    got = np.fromfile(out, np.int32).reshape(its, 4)
    G = pc.GlibcRand(seed)
    want = np.array([pc.draw(G, N, 4) for _ in range(its)], np.int32)
    assert (got == want).all()
    assert all(len(set(r)) == 4 for r in got[:200]) and got.max() == N - 1 and got.min() == 0


def test_abi():
    import psl_slam_amd as P
    assert P.PNPROW_DTYPE == pc.ROW_DTYPE and P.PNPRESULT_DTYPE.itemsize == pc.RESULT_DTYPE.itemsize == 116
    assert P.PNPRESULT_DTYPE.names == pc.RESULT_DTYPE.names
    for name in ("pslfe_pnp_rows_from_matches_device", "pslfe_pnp_solve_device", "pslfe_pnp_solve", "pslfe_pnp_mp_index_from_inliers_device",
                 "pslfe_pnp_ransac_parameters"):
        assert getattr(P.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslPnpRow) == 24 && sizeof(PslPnpResult) == 116" in hdr
