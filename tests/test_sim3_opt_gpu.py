"""GPU parity of the Sim3 optimisation (psl-slam_amd/csrc/pslfe_sim3.hip) with the restatement of tests/sim3_opt_cases.py in the
device's order of the sums, bit for bit: the 8 doubles, the flags, the return value, the calls, iterations and branches; the host
form, a batch against single launches, the error paths, the pair set-up from matches, a chain from SearchBySim3's matches to the
optimised Sim3, and the C++ consumer tools/dropin/sim3_main.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_opt_cases as sc
from test_sim3_opt_cpu import ORDER_DIFFERENCE, assert_equal_ref, read_section, write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_sim3_opt_cpu.py measures ORDER_DIFFERENCE on the CPU; four times that covers cases that are not in the set, the
# project's margin (tests/test_pose_opt_gpu.py)
ORDER_BOUND = 4 * ORDER_DIFFERENCE


def _cam(P, c):
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in c.items():
        cam[k] = v
    return cam


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _run_device(P, ctx, cases, pstride=None, counts=None, fix_scale=None):
    """the cases as one launch -> [(S12_out, bad, nin, info)]; the outlier bytes start as 0xAA"""
    K = len(cases)
    pstride = pstride or max(max(len(c["pairs"]) for c in cases), 1)
    fix = cases[0]["fix_scale"] if fix_scale is None else fix_scale
    S = np.zeros(K, P.SIM3_DTYPE)
    Pr = np.zeros((K, pstride), P.SIM3PAIR_DTYPE)
    n = np.zeros(K, np.int32)
    for k, c in enumerate(cases):
        S[k] = c["S12"]
        m = min(len(c["pairs"]), pstride)
        Pr[k, :m] = c["pairs"][:m]
        n[k] = len(c["pairs"]) if counts is None else counts[k]
    d_S, d_P, d_n = _dev(ctx, S), _dev(ctx, Pr), _dev(ctx, n)
    d_o, d_b = _dev(ctx, np.zeros(K, P.SIM3D_DTYPE)), _dev(ctx, np.full((K, pstride), 0xAA, np.uint8))
    d_g, d_i = _dev(ctx, np.full(K, -99, np.int32)), _dev(ctx, np.zeros(K, P.SIM3INFO_DTYPE))
    P.Optimizer.OptimizeSim3Device(K, d_S, d_P, d_n, pstride, _cam(P, cases[0]["cam1"]), _cam(P, cases[0]["cam2"]), sc.TH2, fix, d_o, d_b, d_g, d_i,
                                   ctx=ctx)
    ctx.synchronize()
    So, b = _down(P, ctx, d_o, np.zeros(K, P.SIM3D_DTYPE)), _down(P, ctx, d_b, np.zeros((K, pstride), np.uint8))
    g, i = _down(P, ctx, d_g, np.zeros(K, np.int32)), _down(P, ctx, d_i, np.zeros(K, P.SIM3INFO_DTYPE))
    for d in (d_S, d_P, d_n, d_o, d_b, d_g, d_i):
        ctx.device_free(d)
    return [(So[k], b[k], int(g[k]), i[k]) for k in range(K)]


def _cut(got, c):
    return got[0], got[1][:len(c["pairs"])], got[2], got[3]


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_device_and_host_forms_equal_restatement(name):
    """0 and 1 pairs; 9, 10, 11: the `< 10` return before and after the removal; 64, 65: a second wave; 256, 257: a second pair per
    thread; 1024, 1025: the LDS capacity and the rows read from HBM; 0 % and 30 % planted outliers; the scale fixed and free; no noise;
    exact data (rho == 0); steps in every branch of the exponential; a point behind a camera"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = sc.case(name)
    ref = c["ref"]["device"]
    full = _run_device(P, ctx, [c])[0]
    got = _cut(full, c)
    assert_equal_ref(got, ref, name)
    assert (full[1][len(c["pairs"]):] == 0xAA).all()                    # bytes beyond the count are not touched
    nin, S, bad = P.Optimizer.OptimizeSim3(c["S12"], c["pairs"], _cam(P, c["cam1"]), _cam(P, c["cam2"]), sc.TH2, c["fix_scale"], ctx=ctx)
    assert nin == got[2] and S.tobytes() == got[0].tobytes() and (bad == got[1]).all()
    # against g2o's edge order: the same decisions, every output double within the bound
    edge = c["ref"]["edge"]
    assert got[2] == edge[2] and (got[1] == edge[1]).all() and got[3]["calls"] == edge[3]["calls"]
    d = np.abs(sc.sim3_doubles(got[0]) - sc.sim3_doubles(edge[0])).max()
    assert d <= ORDER_BOUND, (name, d)


@pytest.mark.parametrize("fix", ["fixed", "free"])
def test_batch_equals_single_launches(fix):
    """K = 5 candidates of different counts in one launch, one without pairs and one with fewer than 10; the position in the batch
    and the row stride do not matter"""
    import psl_slam_amd as P
    ctx = P.default_context()
    names = [f"n257_30_{fix}", f"n0_0_{fix}", f"n1024_30_{fix}", f"n9_30_{fix}", f"n65_0_{fix}"]
    cases = [sc.case(nm) for nm in names]
    single = [_cut(_run_device(P, ctx, [c])[0], c) for c in cases]
    batch = _run_device(P, ctx, cases, pstride=1024)
    for nm, b, s, c in zip(names, batch, single, cases):
        b = _cut(b, c)
        assert b[0].tobytes() == s[0].tobytes() and b[1].tobytes() == s[1].tobytes() and b[2] == s[2] and b[3].tobytes() == s[3].tobytes(), nm
        assert_equal_ref(b, c["ref"]["device"], nm)
    rev = _run_device(P, ctx, cases[::-1], pstride=1100)[::-1]           # 1100: every candidate's rows now come from HBM or LDS as before
    for b, s, c in zip(rev, single, cases):
        b = _cut(b, c)
        assert b[0].tobytes() == s[0].tobytes() and b[1].tobytes() == s[1].tobytes() and b[2] == s[2]


def test_overflowing_and_negative_counts_are_reported_and_nothing_is_written():
    import psl_slam_amd as P
    ctx = P.default_context()
    cases = [sc.case("n65_0_free"), sc.case("n64_0_free"), sc.case("n64_30_free")]
    got = _run_device(P, ctx, cases, pstride=64, counts=[65, 64, -4])
    start = [sc.s3_record(sc.s3_from_rts(c["S12"])) for c in cases]
    assert got[0][2] == -4 and got[0][0].tobytes() == start[0].tobytes() and (got[0][1] == 0xAA).all() and got[0][3]["calls"] == 0
    assert got[2][2] == -1 and got[2][0].tobytes() == start[2].tobytes() and (got[2][1] == 0xAA).all() and got[2][3]["calls"] == 0
    assert_equal_ref(got[1], cases[1]["ref"]["device"], "n64")


def test_error_codes():
    import psl_slam_amd as P
    ctx = P.default_context()
    L = P.lib()
    cam = np.zeros(1, P.CAMERA_DTYPE)
    d = _dev(ctx, np.zeros(256, np.int32))
    p, null, th2 = C.c_void_p(d), C.c_void_p(None), C.c_float(10.0)
    f = L.pslfe_sim3_optimize_device
    cm = P._ptr(cam)
    assert f(ctx._h, C.c_int(-1), p, p, p, C.c_int(1), cm, cm, th2, C.c_int(0), p, p, p, null) == -1
    assert f(ctx._h, C.c_int(1), p, p, p, C.c_int(-1), cm, cm, th2, C.c_int(0), p, p, p, null) == -1
    assert f(ctx._h, C.c_int(0), null, null, null, C.c_int(1), cm, cm, th2, C.c_int(0), null, null, null, null) == 0
    for bad in range(6):
        a = [p, p, p, p, p, p]
        a[bad] = null
        assert f(ctx._h, C.c_int(1), a[0], a[1], a[2], C.c_int(1), cm, cm, th2, C.c_int(0), a[3], a[4], a[5], null) == -1, bad
    assert f(ctx._h, C.c_int(1), p, p, p, C.c_int(1), None, cm, th2, C.c_int(0), p, p, p, null) == -1
    assert f(ctx._h, C.c_int(1), p, p, p, C.c_int(1), cm, None, th2, C.c_int(0), p, p, p, null) == -1
    S, pr, out = np.zeros(1, P.SIM3_DTYPE), np.zeros(4, P.SIM3PAIR_DTYPE), np.zeros(1, P.SIM3D_DTYPE)
    nin = C.c_int()
    h = L.pslfe_sim3_optimize
    b4 = np.zeros(4, np.uint8)
    assert h(ctx._h, P._ptr(S), P._ptr(pr), C.c_int(-1), cm, cm, th2, C.c_int(0), P._ptr(out), P._ptr(b4), C.byref(nin)) == -1
    assert h(ctx._h, P._ptr(S), None, C.c_int(4), cm, cm, th2, C.c_int(0), P._ptr(out), P._ptr(b4), C.byref(nin)) == -1
    assert h(ctx._h, None, P._ptr(pr), C.c_int(4), cm, cm, th2, C.c_int(0), P._ptr(out), P._ptr(b4), C.byref(nin)) == -1
    g = P.FrameGrid(64, 2, ctx=ctx)
    m = L.pslfe_sim3_pairs_from_matches_device
    s2 = np.ones(8, np.float32)
    call = lambda f1, slot1, ncand, n1, mp2s, ps, arr=p: m(f1, C.c_int(slot1), g._h, arr, C.c_int(ncand), arr, arr, arr, C.c_int(n1), arr, arr,
                                                          C.c_int(mp2s), arr, arr, P._ptr(s2), C.c_int(8), arr, null, arr, C.c_int(ps))
    assert call(g._h, 0, -1, 4, 4, 4) == -1 and call(g._h, 0, 1, 4, 4, -1) == -1 and call(g._h, 0, 1, -1, 4, 4) == -1
    assert call(g._h, 0, 0, 4, 4, 4, null) == 0
    assert call(None, 0, 1, 4, 4, 4) == -1 and call(g._h, 2, 1, 4, 4, 4) == -1      # no store; slot 2 of 2
    assert call(g._h, 0, 1, 4, 4, 4) == -5                               # slot not set
    ctx.device_free(d)


def _setup_loop(kps1, kps2, i2, mp1, skip1, mp2, skip2, T1w, T2w, inv_sigma2):
    """the set-up loop src/Optimizer.cc:2854-2933 in numpy -> (rows, the i of each row)"""
    import kf_project_cases as kc
    keep = [i for i in range(min(len(kps1), len(mp1))) if 0 <= i2[i] < min(len(kps2), len(mp2)) and not skip1[i] and not skip2[i2[i]]]
    keep = np.array(keep, np.int64)
    j = i2[keep].astype(np.int64)
    p = np.zeros(len(keep), sc.PAIR_DTYPE)
    p["u1"], p["v1"], p["inv_sigma2_1"] = kps1["x"][keep], kps1["y"][keep], inv_sigma2[kps1["octave"][keep]]
    p["u2"], p["v2"], p["inv_sigma2_2"] = kps2["x"][j], kps2["y"][j], inv_sigma2[kps2["octave"][j]]
    X1 = np.stack([mp1["x"][keep], mp1["y"][keep], mp1["z"][keep]], 1)
    X2 = np.stack([mp2["x"][j], mp2["y"][j], mp2["z"][j]], 1)
    if len(keep):
        p["P1c"], p["P2c"] = kc.affine(T1w["R"], T1w["t"], X1), kc.affine(T2w["R"], T2w["t"], X2)
    return p, keep.astype(np.int32)


def _pairs_device(P, ctx, g, slot1, slots2, i2, mp1, skip1, mp2, skip2, T1w, T2w, inv_sigma2, pstride):
    """pslfe_sim3_pairs_from_matches_device -> (device addresses of pairs and counts, rows, pair_kp, counts)"""
    K = len(slots2)
    d_in = [_dev(ctx, a) for a in (np.asarray(slots2, np.int32), i2, mp1, skip1, mp2, skip2, np.asarray(T1w).reshape(1), T2w)]
    d_p, d_kp, d_n = _dev(ctx, np.zeros((K, pstride), P.SIM3PAIR_DTYPE)), _dev(ctx, np.full((K, pstride), -1, np.int32)), _dev(ctx, np.zeros(K, np.int32))
    P.Optimizer.Sim3PairsFromMatchesDevice(g, slot1, g, d_in[0], K, d_in[1], d_in[2], d_in[3], len(mp1), d_in[4], d_in[5], mp2.shape[1], d_in[6],
                                           d_in[7], inv_sigma2, d_p, d_kp, d_n, pstride)
    ctx.synchronize()
    rows = _down(P, ctx, d_p, np.zeros((K, pstride), P.SIM3PAIR_DTYPE))
    kp, n = _down(P, ctx, d_kp, np.zeros((K, pstride), np.int32)), _down(P, ctx, d_n, np.zeros(K, np.int32))
    for d in d_in + [d_kp]:
        ctx.device_free(d)
    return d_p, d_n, rows, kp, n


def test_pairs_from_matches_equal_the_numpy_set_up_loop():
    """KF1 = keyframe 0 of kf_scene (more than one chunk of 256 keypoints, a ragged tail), two candidates: keyframe 1 and a prefix of
    keyframe 0; NULL matches, a bad map point on either side, an index outside its array, and a count above the stride that is
    reported and not truncated silently"""
    import kf_project_cases as kc
    import kf_scene as ks
    import psl_slam_amd as P
    ctx = P.default_context()
    (k0, d0), (k1, d1) = ks.keyframes()
    slots = [(k0, d0), (k1, d1), (k0[:600], d0[:600])]
    cap = 2048
    g = P.FrameGrid(cap, 3, ctx=ctx)
    for s, (k, d) in enumerate(slots):
        g.set(s, k, d, ks.BOUNDS, None)
    rng = np.random.default_rng(31)
    n1, M2 = len(k0), 1900
    V = kc.views(nslots=3)
    T1w, T2w = V[3]["Tcw"].copy(), np.array([V[8]["Tcw"], V[5]["Tcw"]])
    mp1, _ = kc.map_points(n1, seed=41)
    mp2 = np.stack([kc.map_points(M2, seed=42)[0], kc.map_points(M2, seed=43)[0]])
    skip1 = (rng.random(n1) < 0.05).astype(np.uint8)
    skip2 = (rng.random((2, M2)) < 0.05).astype(np.uint8)
    i2 = np.full((2, cap), -1, np.int32)
    for c, kk in enumerate((k1, k0[:600])):
        i2[c, :n1] = np.where(rng.random(n1) < 0.6, rng.integers(0, len(kk), n1), -1)
        i2[c, 5], i2[c, 7] = len(kk), -7                                # outside KF2's keypoints; a NULL match
        i2[c, n1:n1 + 4] = 3                                            # beyond KF1's keypoints: never read as a match
    i2[0, 9] = min(len(k1), M2) - 1
    skip1[9], skip2[0, i2[0, 9]] = 0, 1                                 # pMP2->isBad()
    want = [_setup_loop(k0, kk, i2[c], mp1, skip1, mp2[c], skip2[c], T1w, T2w[c], ks.INV_SIGMA2) for c, kk in enumerate((k1, k0[:600]))]
    assert all(len(w[0]) > 300 for w in want) and 9 not in want[0][1] and 5 not in want[0][1]
    for pstride in (cap, 256):
        d_p, d_n, rows, kp, n = _pairs_device(P, ctx, g, 0, [1, 2], i2, mp1, skip1, mp2, skip2, T1w, T2w, ks.INV_SIGMA2, pstride)
        for c, (wp, wkp) in enumerate(want):
            assert n[c] == len(wp)
            m = min(len(wp), pstride)
            assert rows[c, :m].tobytes() == wp[:m].tobytes() and (kp[c, :m] == wkp[:m]).all() and (kp[c, m:] == -1).all()
        assert pstride == cap or n.min() > pstride
        ctx.device_free(d_p)
        ctx.device_free(d_n)
    # a slot outside the store is reported in the count
    d_p, d_n, rows, kp, n = _pairs_device(P, ctx, g, 0, [1, 3], i2, mp1, skip1, mp2, skip2, T1w, T2w, ks.INV_SIGMA2, cap)
    assert n[0] == len(want[0][0]) and n[1] == -1
    ctx.device_free(d_p)
    ctx.device_free(d_n)


def test_chain_search_by_sim3_pairs_optimise():
    """SearchBySim3Poses on two kf_scene keyframes whose map points agree with one true Sim3 -> its matches -> pairs -> the optimised
    Sim3: the pairs and their counts stay in HBM between the set-up and the optimisation.  Equal to the numpy set-up loop and the
    restatement fed the same matches, which brings the Sim3 back towards the true one."""
    import kf_project_cases as kc
    import kf_scene as ks
    import psl_slam_amd as P
    ctx = P.default_context()
    (k0, d0), (k1, d1) = ks.keyframes()
    cap = 2048
    g = P.FrameGrid(cap, 2, ctx=ctx)
    g.set(0, k0, d0, ks.BOUNDS, None)
    g.set(1, k1, d1, ks.BOUNDS, None)
    V = kc.views(nslots=2)
    cam = kc.camera()
    v12, v21 = V[3].copy(), V[8].copy()
    v12["slot"], v21["slot"] = 1, 0
    sR21, t21 = v12["T21"]["R"].astype(np.float64).reshape(3, 3), v12["T21"]["t"].astype(np.float64)
    s21 = np.cbrt(np.linalg.det(sR21))
    R12, s12 = (sR21 / s21).T, 1.0 / s21
    t12 = -s12 * R12 @ t21
    v21["T21"] = kc.pose_record(s12 * R12, t12)                         # sR12, t12: the inverse of v12's similarity (:1119-1121)
    rng = np.random.default_rng(12)
    n = min(len(k0), len(k1))
    pair = rng.permutation(n)
    inv = np.argsort(pair)
    mp1, desc1 = kc.map_points(len(k0), seed=21)
    mp2, desc2 = kc.map_points(len(k1), seed=22)
    a, ad = kc.points_onto(k1[pair], d1[pair], v12, cam, kc.SIM3, rng, noise_px=0.5)
    b, bd = kc.points_onto(k0[inv], d0[inv], v21, cam, kc.SIM3, rng, noise_px=0.5)
    real = rng.random(n) < 0.7
    mp1[:n][real], desc1[:n][real] = a[real], ad[real]
    mp2[:n][real[inv]], desc2[:n][real[inv]] = b[real[inv]], bd[real[inv]]
    skip1, skip2 = np.zeros(len(k0), np.uint8), np.zeros(len(k1), np.uint8)
    kf = P.KeyFrameMatcher()
    nf, match, _, _ = kf.SearchBySim3Poses(g, g, v12, mp1, desc1, skip1, v21, mp2, desc2, skip2, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, 7.5)
    assert nf > 100
    i2 = np.full((1, cap), -1, np.int32)
    i2[0, :len(match)] = match
    # the start: the true Sim3 1 degree, 2 cm and 2 % off, as floats
    dR = sc._rodrigues(np.array([0.6, -0.5, 0.62]) * np.radians(1.0))
    S12 = sc.sim3_rec(dR @ R12, dR @ t12 + np.array([0.012, -0.012, 0.01]), s12 * 1.02)
    camd = {k: cam[k] for k in ("fx", "fy", "cx", "cy")}
    T2w = np.array([v21["Tcw"]])
    d_p, d_n, rows, kp, cnt = _pairs_device(P, ctx, g, 0, [1], i2, mp1, skip1, mp2[None], skip2[None], v12["Tcw"], T2w, ks.INV_SIGMA2, cap)
    d_S, d_o = _dev(ctx, np.array([S12])), _dev(ctx, np.zeros(1, P.SIM3D_DTYPE))
    d_b, d_g, d_i = _dev(ctx, np.zeros(cap, np.uint8)), _dev(ctx, np.zeros(1, np.int32)), _dev(ctx, np.zeros(1, P.SIM3INFO_DTYPE))
    P.Optimizer.OptimizeSim3Device(1, d_S, d_p, d_n, cap, cam, cam, sc.TH2, False, d_o, d_b, d_g, d_i, ctx=ctx)
    ctx.synchronize()
    got = (_down(P, ctx, d_o, np.zeros(1, P.SIM3D_DTYPE))[0], _down(P, ctx, d_b, np.zeros(cap, np.uint8))[:cnt[0]],
           int(_down(P, ctx, d_g, np.zeros(1, np.int32))[0]), _down(P, ctx, d_i, np.zeros(1, P.SIM3INFO_DTYPE))[0])
    for d in (d_p, d_n, d_S, d_o, d_b, d_g, d_i):
        ctx.device_free(d)
    wp, wkp = _setup_loop(k0, k1, i2[0], mp1, skip1, mp2, skip2, v12["Tcw"], v21["Tcw"], ks.INV_SIGMA2)
    assert cnt[0] == len(wp) == nf and rows[0, :cnt[0]].tobytes() == wp.tobytes() and (kp[0, :cnt[0]] == wkp).all()
    ref = sc.optimize(S12, wp, camd, camd, sc.TH2, False)
    assert_equal_ref(got, ref[:4], "chain")
    R, t, s = sc.s3_matrix((list(got[0]["q"]), list(got[0]["t"]), float(got[0]["s"])))
    R0, t0, s0 = sc.s3_matrix(sc.s3_from_rts(S12))
    assert got[2] > 0.8 * nf and abs(s - s12) < 0.25 * abs(s0 - s12) and np.abs(R - R12).max() < 0.25 * np.abs(R0 - R12).max()


@pytest.mark.parametrize("fix", [True, False])
def test_cpp_consumer_equals_restatement(tmp_path, fix):
    """tools/dropin/sim3_main.cpp on pslfe.hpp: the batched device form, the candidate-by-candidate host form and its own plain C++
    loop, each against the restatement in the device's order"""
    exe = str(tmp_path / "sim3_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "sim3_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    f_ = "fixed" if fix else "free"
    names = [f"n0_0_{f_}", f"n9_30_{f_}", f"n11_30_{f_}", f"n64_0_{f_}", f"n257_30_{f_}", f"n1025_30_{f_}"] + ([] if fix else ["exact", "n100_0_free_limit5", "n100_30_free_limit10"])
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = write_cases(path, names, fix)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        loop, dev, host = read_section(f, cases), read_section(f, cases), read_section(f, cases)
        assert f.read() == b""
    for nm, c, a, b, h in zip(names, cases, loop, dev, host):
        assert_equal_ref(a, c["ref"]["device"], nm + " loop")
        assert_equal_ref(b, c["ref"]["device"], nm + " device")
        assert_equal_ref(h, c["ref"]["device"], nm + " host", info=False)
