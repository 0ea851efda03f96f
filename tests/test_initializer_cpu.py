"""The restatement of Initializer (tests/initializer_cases.py) and the stand-alone host program of tools/dropin/init_main.cpp (the shared
header psl-slam_amd/csrc/initializer_kernels.h compiled for the host with g++, under the address and undefined-behaviour sanitizers),
bit for bit with each other; the sets; the float Jacobi reading against LAPACK; psl_acosf against the host's acosf; the stated order of a NaN in vCosParallax and the selection; the
ground truth of two noise-free scenes; the ABI.  No GPU.

The float Jacobi reading against LAPACK (test_jacobi_reading_against_lapack): on the 16x9, 8x9, 3x3 and 4x4 matrices of the cases, the
singular values (relative to the largest) and the last right singular vector (up to sign) of the reading and of LAPACK in float32
(torch's CPU gesdd: numpy.linalg computes a float32 input in double) are both compared with the float64 SVD of the same matrix.  The
yardstick is LAPACK float32's own worst deviation per shape, and the reading may deviate at most 8 times that.  A matrix whose last
vector is not determined to float precision (relative gap below 1e-4: the 8-point F of a planar scene) is compared by its values alone.
Measured here (reading / LAPACK float32, worst over the matrices of a shape):
    16x9   values 1.7e-07 / 4.3e-07   vector 2.0e-07 / 4.8e-07
    8x9    values 1.2e-07 / 3.0e-07   vector 4.9e-06 / 1.7e-05 (the completed ninth row; its worst dot product with the eight others
                                       8.2e-08, against the same yardstick)
    3x3    values 1.1e-07 / 2.5e-07   vector 1.1e-07 / 2.5e-07
    4x4    values 1.4e-07 / 4.1e-07   vector 1.5e-07 / 4.0e-07
so the worst ratio is 0.46.

psl_acosf against the host's acosf (test_acosf_against_host): no deviation on the 36769 points of the grid, 0 ulp; no
grid point changes the side of parallax > 1.0.

Ground truth (test_ground_truth_of_the_clean_scenes): the worst entry of R21 - R and of t21 - t / |t| on the noise-free general and
planar scene.  Measured here:
    float64 LAPACK in place of the reading   general R 8.8e-07 t 3.1e-05   planar R 2.2e-07 t 1.5e-06
    the reading                              general R 1.5e-06 t 6.2e-05   planar R 4.9e-07 t 1.6e-06
The allowance is 8 times the LAPACK run's deviation on the same scene and sets."""
import ctypes as C
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

import initializer_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, MARGIN = np.float32, 8.0


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the header's host form as a stand-alone program, built once with g++ alone under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("initializer") / "init_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-DPSL_INIT_HOST_ONLY", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tools", "dropin", "init_main.cpp")],
                   check=True, capture_output=True)
    return exe


def _camera_dtype():
    import psl_slam_amd as P
    return P.CAMERA_DTYPE


def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path):
    """every case: status, scores, both winning iterations, H, F, every nGood and parallax, R, t, every point and flag, mvIniMatches"""
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = [ic.case(nm) for nm in ic.CASE_NAMES]
    ic.write_cases(path, cases, _camera_dtype())
    p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        got = ic.read_section(f, cases)
        assert f.read() == b""
    for nm, c, g in zip(ic.CASE_NAMES, cases, got):
        ic.assert_same(g, c["ref"], nm)


def test_cases_are_what_their_names_say():
    """the restated results alone: this test reads no product code, it pins what the cases exercise; the header and the kernel are held
    to these results by the bit-for-bit parity tests (here and in tests/test_initializer_gpu.py)"""
    r = {nm: ic.case(nm)["ref"]["res"] for nm in ic.CASE_NAMES}
    st = {nm: int(v["status"]) for nm, v in r.items()}
    assert st["n7"] == 0 and r["n7"]["nmatches"] == 7 and r["n7"]["best_it_h"] == -1 and r["n7"]["SF"] == 0          # nothing solved
    assert all(sorted(s) == list(range(8)) for s in ic.case("n8")["trace"]["sets"]) and r["n8"]["SF"] > 0            # all rows in every set
    assert [int(r[nm]["nmatches"]) for nm in ("n9", "n63", "n64", "n65", "n512", "n530")] == [9, 63, 64, 65, ic.LDS_ROWS, ic.LDS_ROWS + 18]
    assert st["n63"] == st["n64"] == st["n65"] == st["n512"] == st["n530"] == 1
    h = ic.case("holes")
    assert len(h["keys1"]) == 500 and len(h["keys2"]) == 380 and r["holes"]["nmatches"] == 80 and st["holes"] == 1
    assert [ic.case(nm)["max_its"] for nm in ("its1", "its15", "its16", "its17", "its200")] == [1, ic.BLOCK - 1, ic.BLOCK, ic.BLOCK + 1, 200]
    assert r["its17"]["best_it_h"] < 17 and r["its200"]["best_it_h"] >= ic.BLOCK and st["its200"] == 1
    assert st["general"] == 1 and r["general"]["RH"] <= 0.40 and r["general"]["ntriangulated"] == 120                # F branch, true
    assert st["planar"] == 3 and r["planar"]["RH"] > 0.40                                                             # H branch, true
    g = sorted(int(v) for v in r["planar_twin"]["ngood"])
    assert st["planar_twin"] == 2 and g[-1] == g[-2] == 120                                                           # secondBestGood == bestGood
    assert st["rotation"] == 2 and not r["rotation"]["ngood"].any() and r["rotation"]["best_hypothesis"] == -1       # the d1/d2 gate
    lp = r["lowpar"]
    assert st["lowpar"] == 0 and lp["best_hypothesis"] >= 0 and lp["ngood"].max() == 120 and 0 < lp["parallax"][lp["best_hypothesis"]] < 1.0
    sm = r["similar"]
    assert not (st["similar"] & 1) and sorted(int(v) for v in sm["ngood"])[-2] == sm["ngood"].max() > 100           # a shared maximum
    sf = r["similar_f"]                                                                                              # nsimilar > 1 at :517
    assert st["similar_f"] == 0 and sf["best_hypothesis"] == -1 and sorted(int(v) for v in sf["ngood"][:4])[-2:] == [90, 120]
    nf = r["infinite"]                                   # the isfinite gate (:841): the searches never read K, CheckRT sees only NaN
    assert st["infinite"] == 0 and nf["inliers_f"] == 120 and nf["RH"] <= 0.40 and not nf["ngood"].any() and not nf["parallax"].any()
    assert st["few"] == 0 and 0 < r["few"]["ngood"].max() < 50 and r["few"]["best_hypothesis"] == -1
    assert st["half"] == 1 and r["half"]["ngood"].max() == 50 and r["half"]["inliers_f"] < 56                        # maxGood == nMinGood
    assert not (st["fifth"] & 1) and r["fifth"]["SF"] > 0
    assert st["identical"] == 4 and r["identical"]["SH"] == 0 and r["identical"]["SF"] == 0                          # no model
    assert st["noisy"] == 1 and 100 < r["noisy"]["ntriangulated"] < 140
    # an accepted initialisation leaves exactly its triangulated matches in mvIniMatches
    for nm in ic.CASE_NAMES:
        c = ic.case(nm)
        if st[nm] & 1:
            assert ((c["ref"]["ini"] >= 0) == (c["ref"]["tri"] != 0)).all() and (c["ref"]["ini"] >= 0).sum() == r[nm]["ntriangulated"]
        else:
            assert (c["ref"]["ini"] == c["matches"]).all() and not c["ref"]["tri"].any() and not c["ref"]["p3d"].any()
    # no parallax that decides lies within psl_acosf's deviation of one degree
    for nm in ic.CASE_NAMES:
        assert all(abs(float(v) - 1.0) > 1e-3 for v in r[nm]["parallax"]), nm


@pytest.mark.parametrize("N", [8, 9, 64, 300])
def test_sets_equal_swap_and_pop(host_exe, tmp_path, N):
    import psl_slam_amd as P
    out, seed, its = str(tmp_path / "sets.bin"), 1234 + N, 2000
    p = subprocess.run([host_exe, "--sets", str(N), str(seed), str(its), out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    got = np.fromfile(out, np.int32).reshape(its, 8)
    want = ic.sets(seed, N, its)
    assert (got == want).all() and (P.Initializer.Sets(seed, N, its) == want).all()
    assert all(len(set(r)) == 8 for r in got) and got.max() == N - 1 and got.min() == 0
    if N == 8:
        assert all(sorted(r) == list(range(8)) for r in got)
    for bad in ((7, 10), (8, -1)):
        with pytest.raises(P.PslfeError):
            P.Initializer.Sets(1, *bad)


def _matrices():
    """the matrices the cases hand to the SVD: {shape: [A [r][c] float32]}"""
    out = {"16x9": [], "8x9": [], "3x3": [], "4x4": []}
    for nm in ("general", "planar", "noisy", "holes"):
        c = ic.case(nm)
        tr = c["trace"]
        rows, idx = tr["rows"], tr["sets"][:6]
        nm1, nm2 = ic.normalize(c["keys1"]), ic.normalize(c["keys2"])
        u1, v1, u2, v2 = ic._normalized(rows, idx, nm1, nm2)
        for b in range(len(idx)):
            A = np.zeros((16, 9), F)
            Af = np.zeros((8, 9), F)
            for i in range(8):
                a, bb, cc, d = u1[i, b], v1[i, b], u2[i, b], v2[i, b]
                A[2 * i] = [0, 0, 0, -a, -bb, -1, d * a, d * bb, d]
                A[2 * i + 1] = [a, bb, 1, 0, 0, 0, -cc * a, -cc * bb, -cc]
                Af[i] = [cc * a, cc * bb, cc, d * a, d * bb, d, a, bb, 1]
            out["16x9"].append(A)
            out["8x9"].append(Af)
            out["3x3"].append(np.linalg.svd(Af.astype(np.float64))[2][-1].reshape(3, 3).astype(F))   # Fpre
        K = ic.k_matrix(ic.CAM)
        if "hyps" in tr:
            R, t = tr["hyps"][max(int(c["ref"]["res"]["best_hypothesis"]), 0)]
            P1 = np.concatenate([K, np.zeros((3, 1, 1), F)], 1)[:, :, 0]
            P2 = ic.mul33(K, np.concatenate([R, t[:, None, :]], 1))[:, :, 0]
            for q in rows[:12]:
                out["4x4"].append(np.stack([q[0] * P1[2] - P1[0], q[1] * P1[2] - P1[1], q[2] * P2[2] - P2[0], q[3] * P2[2] - P2[1]]).astype(F))
    return out


def _reading(A):
    """-> (w float64 [min], last right vector float32 [c], the other rows of the 'vt' side) under this library's reading"""
    r, c = A.shape
    if r >= c:
        At = np.ascontiguousarray(A.T)[:, :, None].copy()
        W, V = ic.jacobi(At, True)
        return W[:, 0], V[c - 1, :, 0], V[:c - 1, :, 0]
    At = np.zeros((c, c, 1), F)
    At[:r, :, 0] = A
    W, _ = ic.jacobi(At[:r], False)
    ic.complete(At, r, W)
    return W[:, 0], At[c - 1, :, 0], At[:c - 1, :, 0]


GAP = 1e-4   # below this the last right vector is not determined to float precision (eps / gap above 1e-3): values only


def _dev(w, v, A):
    """-> (worst singular value deviation relative to the largest, deviation of the last right vector up to sign or None)"""
    u64, w64, vt64 = np.linalg.svd(A.astype(np.float64), full_matrices=True)
    dw = np.abs(np.asarray(w, np.float64) - w64).max() / w64[0]
    r, c = A.shape
    gap = (w64[c - 2] - w64[c - 1] if r >= c else w64[r - 1]) / w64[0]
    if gap < GAP:
        return dw, None
    v = np.asarray(v, np.float64)
    return dw, min(np.abs(v - vt64[-1]).max(), np.abs(v + vt64[-1]).max())


def _lapack32(A):
    """LAPACK's float32 SVD (numpy.linalg computes a float32 input in double): torch's CPU gesdd"""
    import torch
    _, w, vt = torch.linalg.svd(torch.from_numpy(np.ascontiguousarray(A, F)), full_matrices=True)
    assert w.dtype == torch.float32
    return w.numpy(), vt.numpy()


def test_jacobi_reading_against_lapack():
    """the numpy text of the reading alone (ic.jacobi, ic.complete); the header and the kernel are held to that text by the bit-for-bit
    parity tests"""
    worst_ratio = 0.0
    for shape, mats in _matrices().items():
        assert len(mats) >= 12
        rd, lp, orth, orth_lp = [], [], 0.0, 0.0
        for A in mats:
            w, v, others = _reading(A)
            rd.append(_dev(w, v, A))
            w32, vt32 = _lapack32(A)
            lp.append(_dev(w32, vt32[-1], A))
            if shape == "8x9" and rd[-1][1] is not None:
                orth = max(orth, np.abs(others.astype(np.float64) @ v.astype(np.float64)).max())
        assert sum(d[1] is not None for d in rd) >= 12
        rw, rv = max(d[0] for d in rd), max(d[1] for d in rd if d[1] is not None)
        lw, lv = max(d[0] for d in lp), max(d[1] for d in lp if d[1] is not None)
        print("%s values %.2g / %.2g vector %.2g / %.2g orth %.2g" % (shape, rw, lw, rv, lv, orth))
        assert rw <= MARGIN * lw and rv <= MARGIN * lv, (shape, rw, lw, rv, lv)
        assert orth <= MARGIN * lv, (shape, orth, lv)
        worst_ratio = max(worst_ratio, rw / lw, rv / lv)
    print("worst ratio %.2f" % worst_ratio)


def _ulps(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7fffffff), ia), np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def test_acosf_against_host(host_exe, tmp_path):
    libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.acosf.restype, libm.acosf.argtypes = C.c_float, [C.c_float]
    near = np.nextafter(F(np.cos(np.pi / 180)), F(2), dtype=F)
    around = [near]
    for _ in range(400):                                         # every float around cos(1 degree)
        around.append(np.nextafter(around[-1], F(-2), dtype=F))
    grid = np.unique(np.concatenate([np.linspace(-1, 1, 20001), np.linspace(0.999, 1, 60001), np.array(around, np.float64),
                                     [0.0, 0.5, -0.5, 1.0, -1.0, 1e-20, 0.99998]]).astype(F))
    src, dst = str(tmp_path / "x.bin"), str(tmp_path / "acos.bin")
    grid.tofile(src)
    p = subprocess.run([host_exe, "--acosf", src, dst], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    got = np.fromfile(dst, F)
    host = np.array([libm.acosf(float(x)) for x in grid], F)
    worst = int(_ulps(got, host).max())
    print("psl_acosf against the host's acosf: %d ulp at most on %d points" % (worst, len(grid)))
    assert worst <= 4                                            # a restatement of fdlibm, not another function

    def par(a):
        return ((a * F(180.0)).astype(np.float64) / 3.1415926535897932384626433832795).astype(F)
    assert ((par(got) > 1.0) == (par(host) > 1.0)).all()
    for x in list(grid[::997]) + around[:50]:                    # the numpy text is the same function
        assert ic.same_floats(ic.acosf(x), got[np.searchsorted(grid, x)]), x
    assert np.isnan(ic.acosf(F(1.5))) and np.isnan(ic.acosf(F(np.nan)))


def test_nan_order_and_selection_of_the_host_compile(host_exe, tmp_path):
    """psl_init_cos_key and psl_init_select_key of the header: ascending keys are the stated order (a NaN with the sign bit set below
    -inf, one with it clear above +inf, -0 below +0), the key is invertible, and the element at sorted index min(50, n - 1) is the one
    that order gives, with NaNs of both signs and both infinities among the cosines; the numpy text has the same keys"""
    def run(v):
        src, dst = str(tmp_path / "c.bin"), str(tmp_path / "k.bin")
        np.array(v, F).tofile(src)
        p = subprocess.run([host_exe, "--select", src, dst], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        raw = np.fromfile(dst, np.uint32)
        return raw[:-1], raw[-1:].view(F)[0]
    keys, _ = run(ic.ORDERED)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (keys == ic.cos_key(np.array(ic.ORDERED, F))).all()
    for v, want in ic.selection_cases():
        k, got = run(v)
        assert (k == ic.cos_key(np.array(v, F))).all()
        assert np.array(got, F).view(np.uint32) == np.array(want, F).view(np.uint32), (len(v), got, want)   # bit for bit: the NaN's payload too


def _truth_dev(res, truth):
    R, t = truth
    return (np.abs(res["R21"].astype(np.float64).reshape(3, 3) - R).max(), np.abs(res["t21"].astype(np.float64) - t).max())


def test_ground_truth_of_the_clean_scenes():
    """the numpy restatement alone, with and without LAPACK in place of the reading; the header and the kernel are held to the
    restatement by the bit-for-bit parity tests"""
    for nm in ("general", "planar"):
        c = ic.case(nm)
        assert c["ref"]["res"]["status"] & 1
        ic.USE_LAPACK = True
        try:
            lap = ic.initialize(c["keys1"], c["keys2"], c["matches"], ic.CAM, c["sigma"], c["max_its"], c["seed"])["res"]
        finally:
            ic.USE_LAPACK = False
        assert lap["status"] & 1 and lap["best_hypothesis"] >= 0
        dl, dr = _truth_dev(lap, c["truth"]), _truth_dev(c["ref"]["res"], c["truth"])
        print("%s: LAPACK R %.2g t %.2g; reading R %.2g t %.2g" % (nm, dl[0], dl[1], dr[0], dr[1]))
        assert dr[0] <= MARGIN * dl[0] and dr[1] <= MARGIN * dl[1], (nm, dl, dr)


def test_abi():
    import psl_slam_amd as P
    assert P.INITRESULT_DTYPE == ic.RESULT_DTYPE and P.INITRESULT_DTYPE.itemsize == 228
    for name in ("pslfe_init_debug_select", "pslfe_init_sets", "pslfe_init_initialize_device", "pslfe_init_initialize_frames_device", "pslfe_init_initialize"):
        assert getattr(P.lib(), name)
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslInitResult) == 228" in hdr
