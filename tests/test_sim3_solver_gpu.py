"""GPU parity of the Sim3 RANSAC (psl-slam_amd/csrc/pslfe_sim3_solver.hip) with the restatement of tests/sim3_solver_cases.py, bit for
bit: status, iterations, both counts, R, t, s and every flag; the host form, calls resumed in rounds of 5 against find(), a batch of
67 candidates against single launches, the error paths, a keyframe-sized stride, the sigma2 output of the pair set-up, the candidate
loop of ComputeSim3 in both mirrors, the C++ consumer tools/dropin/sim3_solver_main.cpp, and the chain of LoopClosing::ComputeSim3
from SearchByBoW to OptimizeSim3 with every stage held to its restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sim3_solver_cases as sc
from test_sim3_solver_cpu import _cam_rec, _names, assert_equal_ref, read_section, write_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _run_device(P, ctx, cands, seed0, n_iterations, fix_scale, pstride=None, counts=None, start=None, best=None, cams=None):
    """cands [(pairs, sigma2)] as one launch, candidate c seeded seed0 + c -> [(result, flags [pstride])]; the flags start as 0xAA"""
    K = len(cands)
    pstride = pstride or max(max(len(p) for p, _ in cands), 1)
    Pr, Sg, n = np.zeros((K, pstride), P.SIM3PAIR_DTYPE), np.zeros((K, pstride, 2), np.float32), np.zeros(K, np.int32)
    for k, (p, s) in enumerate(cands):
        m = min(len(p), pstride)
        Pr[k, :m], Sg[k, :m] = p[:m], np.asarray(s, np.float32).reshape(-1, 2)[:m]
        n[k] = len(p) if counts is None else counts[k]
    cam1, cam2 = cams or sc.cameras()
    ds = [_dev(ctx, a) for a in (Pr, Sg, n, np.zeros(K, P.SIM3SOLVERRESULT_DTYPE), np.full((K, pstride), 0xAA, np.uint8))]
    d_s = _dev(ctx, np.asarray(start, np.int32)) if start is not None else 0
    d_b = _dev(ctx, np.asarray(best, np.int32)) if best is not None else 0
    P.Sim3Solver.SolveDevice(K, ds[0], ds[1], ds[2], pstride, _cam_rec(P, cam1), _cam_rec(P, cam2), fix_scale, seed0, n_iterations, ds[3], ds[4], d_s,
                             d_b, ctx=ctx)
    ctx.synchronize()
    res, fl = _down(P, ctx, ds[3], np.zeros(K, P.SIM3SOLVERRESULT_DTYPE)), _down(P, ctx, ds[4], np.zeros((K, pstride), np.uint8))
    for d in ds + [d for d in (d_s, d_b) if d]:
        ctx.device_free(d)
    return [(res[k], fl[k]) for k in range(K)]


def _same(got, ref, what):
    """(result, flags) against (result, flags, trace) of the restatement"""
    assert_equal_ref((got[0], got[1][:len(ref[1])], None), ref, what, trace=False)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_device_and_host_forms_equal_restatement(name):
    """19 pairs (bNoMore at once), 20 (one iteration), 21; 63 / 64 / 65 and 127 / 129 around the wave loop; 1024 = the LDS capacity and
    1025 with a pair staged from HBM; success at iteration 1, 5, 6, 64, 65 (the block boundary), 300 and never; a running best on
    noisy data; the threshold truncation; a pair behind the camera and a NaN pair; near-collinear triples; the scale fixed and free.
    pstride is the pair count itself."""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = sc.case(name)
    n = len(c["pairs"])
    got = _run_device(P, ctx, [(c["pairs"], c["sigma2"])], c["seed"], sc.MAX_ITS, c["fix_scale"], pstride=n + 3)[0]
    _same(got, c["ref"], name)
    assert (got[1][n:] == 0xAA).all()                                   # bytes beyond the count are not touched
    got = _run_device(P, ctx, [(c["pairs"], c["sigma2"])], c["seed"], sc.MAX_ITS, c["fix_scale"], pstride=n)[0]
    _same(got, c["ref"], name + " pstride == n")
    idx = np.arange(n, dtype=np.int32)[::-1].copy()                     # mvnIndices1: row i is KF1 keypoint n - 1 - i
    s = P.Sim3Solver(c["pairs"], c["sigma2"], idx, n, _cam_rec(P, c["cam1"]), _cam_rec(P, c["cam2"]), c["fix_scale"], c["seed"], ctx=ctx)
    s.SetRansacParameters(sc.PROB, sc.MIN_INLIERS, sc.MAX_ITS)
    ok, vb, nin = s.find()
    ref = c["ref"]
    assert ok == (ref[0]["status"] == 1) and nin == ref[0]["ninliers"] and (vb[::-1] == ref[1].astype(bool)).all()
    _same((s.result, s.row_inliers), ref, name + " host")
    if ok:
        assert s.GetEstimatedRotation().tobytes() == ref[0]["S12"]["R"].tobytes() and s.GetEstimatedScale() == ref[0]["S12"]["s"]
        assert s.GetEstimatedTranslation().tobytes() == ref[0]["S12"]["t"].tobytes()


@pytest.mark.parametrize("name", ["n20", "n65", "n200_it64", "n200_it65", "n150_noisy", "n150_noisy_never", "n129"])
def test_rounds_of_five_equal_find(name):
    """iterate(5) resumed through d_start_it / d_best_in until a Sim3 or bNoMore: the result of one find(); and the mirror's iterate"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = sc.case(name)
    it = best = rounds = 0
    while True:
        res, fl = _run_device(P, ctx, [(c["pairs"], c["sigma2"])], c["seed"], 5, c["fix_scale"], start=[it], best=[best])[0]
        rounds += 1
        assert res["iterations"] <= it + 5
        it, best = int(res["iterations"]), int(res["best_inliers"])
        if res["status"] != 0:
            break
        assert res["ninliers"] == 0 and not fl.any() and not res["S12"]["R"].any()
    _same((res, fl), c["ref"], name)
    assert rounds == (int(c["ref"][0]["iterations"]) + 4) // 5
    n = len(c["pairs"])
    s = P.Sim3Solver(c["pairs"], c["sigma2"], np.arange(n, dtype=np.int32), n, _cam_rec(P, c["cam1"]), _cam_rec(P, c["cam2"]), c["fix_scale"],
                     c["seed"], ctx=ctx)
    s.SetRansacParameters(sc.PROB, sc.MIN_INLIERS, sc.MAX_ITS)
    while True:
        ok, no_more, vb, nin = s.iterate(5)
        if ok or no_more:
            break
    _same((s.result, s.row_inliers), c["ref"], name + " mirror")


def _mixed_batch(K, seed0):
    """K candidates of mixed counts and shares of consistent pairs; candidate c is seeded seed0 + c"""
    rng = np.random.default_rng(88)
    counts = [19, 20, 21, 63, 64, 65, 127, 129, 256, 300] + list(rng.integers(22, 300, K - 10))
    return [sc.make_pairs(1000 + k, int(n), int(n * (0.25 + 0.5 * rng.random())), False)[:2] for k, n in enumerate(counts)]


def test_batch_of_67_equals_single_launches():
    """the position in the batch and the row stride do not matter; a third of the batch against the restatement too"""
    import psl_slam_amd as P
    ctx = P.default_context()
    K, seed0 = 67, 4000
    cands = _mixed_batch(K, seed0)
    batch = _run_device(P, ctx, cands, seed0, sc.MAX_ITS, False, pstride=300)
    statuses = set()
    c1, c2 = sc.cameras()
    for k, (p, s) in enumerate(cands):
        single = _run_device(P, ctx, [(p, s)], seed0 + k, sc.MAX_ITS, False)[0]
        assert batch[k][0].tobytes() == single[0].tobytes() and (batch[k][1][:len(p)] == single[1][:len(p)]).all(), k
        assert (batch[k][1][len(p):] == 0xAA).all()
        statuses.add(int(single[0]["status"]))
        if k % 3 == 0 and single[0]["iterations"] <= 40:
            _same(batch[k], sc.find(p, s, c1, c2, False, seed0 + k), k)
    assert statuses == {1, 2}
    # rounds of 5 over the whole batch, every candidate resumed from its own state
    start, best = np.zeros(K, np.int32), np.zeros(K, np.int32)
    done = [None] * K
    for _ in range(60):
        out = _run_device(P, ctx, cands, seed0, 5, False, pstride=300, start=start, best=best)
        for k, (res, fl) in enumerate(out):
            if done[k] is None:
                start[k], best[k] = res["iterations"], res["best_inliers"]
                if res["status"] != 0:
                    done[k] = (res, fl)
        if all(d is not None for d in done):
            break
    for k in range(K):
        assert done[k][0].tobytes() == batch[k][0].tobytes() and (done[k][1] == batch[k][1]).all(), k


def test_overflowing_and_negative_counts_are_reported_and_nothing_is_written():
    import psl_slam_amd as P
    ctx = P.default_context()
    cs = [sc.case("n65"), sc.case("n63"), sc.case("n127")]
    got = _run_device(P, ctx, [(c["pairs"], c["sigma2"]) for c in cs], 0, sc.MAX_ITS, False, pstride=64, counts=[65, 63, -4])
    zero = np.zeros((), P.SIM3SOLVERRESULT_DTYPE)
    for k, code in ((0, -4), (2, -1)):
        want = zero.copy()
        want["status"] = code
        assert got[k][0].tobytes() == want.tobytes() and (got[k][1] == 0xAA).all()
    c = cs[1]
    _same(got[1], sc.find(c["pairs"], c["sigma2"], c["cam1"], c["cam2"], False, 1), "n63 in the middle")


def test_error_codes():
    import psl_slam_amd as P
    ctx = P.default_context()
    L = P.lib()
    cam = np.zeros(1, P.CAMERA_DTYPE)
    d = _dev(ctx, np.zeros(1024, np.int32))
    p, null, cm = C.c_void_p(d), C.c_void_p(None), P._ptr(cam)
    f = L.pslfe_sim3_solve_device

    def call(a, ncand=1, pstride=1, prob=0.99, mn=20, mx=300, nit=5, cam1=cm, cam2=cm, h=ctx._h):
        return f(h, C.c_int(ncand), a[0], a[1], a[2], C.c_int(pstride), cam1, cam2, C.c_double(prob), C.c_int(mn), C.c_int(mx), C.c_int(0), C.c_uint32(1),
                 null, null, C.c_int(nit), a[3], a[4])
    ok = [p, p, p, p, p]
    assert call(ok, ncand=-1) == -1 and call(ok, pstride=-1) == -1 and call(ok, mn=2) == -1 and call(ok, prob=1.5) == -1 and call(ok, prob=0.0) == -1
    assert call(ok, mx=0) == -1 and call(ok, nit=-1) == -1
    assert call([null] * 5, ncand=0) == 0
    for bad in range(5):
        a = list(ok)
        a[bad] = null
        assert call(a) == -1, bad
    assert call(ok, cam1=None) == -1 and call(ok, cam2=None) == -1 and call(ok, h=None) == -1
    assert call([null, null, p, p, null], pstride=0) == 0                # no room for a pair: the arrays may be NULL
    assert call(ok) == 0                                                 # count 0 < 20: bNoMore
    ctx.synchronize()
    h = L.pslfe_sim3_solve
    res, pr, sg, fl = np.zeros(1, P.SIM3SOLVERRESULT_DTYPE), np.zeros(4, P.SIM3PAIR_DTYPE), np.ones((4, 2), np.float32), np.zeros(4, np.uint8)

    def one(pairs=P._ptr(pr), n=4, prob=0.99, mn=20, start=0, r=P._ptr(res)):
        return h(ctx._h, pairs, P._ptr(sg), C.c_int(n), cm, cm, C.c_double(prob), C.c_int(mn), C.c_int(300), C.c_int(0), C.c_uint32(1), C.c_int(start),
                 C.c_int(0), C.c_int(5), r, P._ptr(fl))
    assert one(n=-1) == -1 and one(pairs=None) == -1 and one(prob=1.0) == -1 and one(mn=2) == -1 and one(start=-1) == -1 and one(r=None) == -1
    assert one() == 0 and res[0]["status"] == 2 and res[0]["iterations"] == 0
    assert one(n=0, pairs=None) == 0 and res[0]["status"] == 2
    ctx.device_free(d)


def test_pair_set_up_hands_the_level_sigma2_over():
    """pslfe_sim3_pairs_sigma2_from_matches_device: the rows, their keypoints and the counts byte for byte those of
    pslfe_sim3_pairs_from_matches_device, with and without the new output; sigma2 = mvLevelSigma2 of the two octaves of each row"""
    import kf_project_cases as kc
    import kf_scene as ks
    import psl_slam_amd as P
    from test_sim3_opt_gpu import _pairs_device
    ctx = P.default_context()
    (k0, d0), (k1, d1) = ks.keyframes()
    cap = 2048
    g = P.FrameGrid(cap, 2, ctx=ctx)
    g.set(0, k0, d0, ks.BOUNDS, None)
    g.set(1, k1, d1, ks.BOUNDS, None)
    rng = np.random.default_rng(5)
    n1, M2 = len(k0), len(k1)
    V = kc.views(nslots=3)
    T1w, T2w = V[3]["Tcw"].copy(), np.array([V[8]["Tcw"], V[5]["Tcw"]])
    mp1, _ = kc.map_points(n1, seed=41)
    mp2 = np.stack([kc.map_points(M2, seed=42)[0], kc.map_points(M2, seed=43)[0]])
    skip1, skip2 = (rng.random(n1) < 0.05).astype(np.uint8), (rng.random((2, M2)) < 0.05).astype(np.uint8)
    i2 = np.full((2, cap), -1, np.int32)
    for c in range(2):
        i2[c, :n1] = np.where(rng.random(n1) < 0.6, rng.integers(0, M2, n1), -1)
    level_sigma2 = (np.float32(1.0) / np.asarray(ks.INV_SIGMA2, np.float32)).astype(np.float32)
    for pstride in (cap, 256):
        d_p0, d_n0, rows0, kp0, n0 = _pairs_device(P, ctx, g, 0, [1, 1], i2, mp1, skip1, mp2, skip2, T1w, T2w, ks.INV_SIGMA2, pstride)
        for with_sigma in (True, False):
            d_in = [_dev(ctx, a) for a in (np.array([1, 1], np.int32), i2, mp1, skip1, mp2, skip2, np.asarray(T1w).reshape(1), T2w)]
            d_p, d_kp, d_n = _dev(ctx, np.zeros((2, pstride), P.SIM3PAIR_DTYPE)), _dev(ctx, np.full((2, pstride), -1, np.int32)), _dev(ctx, np.zeros(2, np.int32))
            d_sg = _dev(ctx, np.full((2, pstride, 2), -7.0, np.float32))
            P.Optimizer.Sim3PairsSigma2FromMatchesDevice(g, 0, g, d_in[0], 2, d_in[1], d_in[2], d_in[3], n1, d_in[4], d_in[5], M2, d_in[6], d_in[7],
                                                         ks.INV_SIGMA2, level_sigma2, d_p, d_kp, d_n, pstride, d_sg if with_sigma else 0)
            ctx.synchronize()
            rows, kp = _down(P, ctx, d_p, np.zeros((2, pstride), P.SIM3PAIR_DTYPE)), _down(P, ctx, d_kp, np.zeros((2, pstride), np.int32))
            n, sg = _down(P, ctx, d_n, np.zeros(2, np.int32)), _down(P, ctx, d_sg, np.zeros((2, pstride, 2), np.float32))
            for d in d_in + [d_p, d_kp, d_n, d_sg]:
                ctx.device_free(d)
            assert rows.tobytes() == rows0.tobytes() and kp.tobytes() == kp0.tobytes() and n.tobytes() == n0.tobytes()
            for c in range(2):
                m = min(int(n[c]), pstride)
                assert m > 200
                if with_sigma:
                    j = i2[c, kp[c, :m]]
                    assert (sg[c, :m, 0] == level_sigma2[k0["octave"][kp[c, :m]]]).all() and (sg[c, :m, 1] == level_sigma2[k1["octave"][j]]).all()
                    assert (sg[c, m:] == -7.0).all()
                else:
                    assert (sg[c] == -7.0).all()
        ctx.device_free(d_p0)
        ctx.device_free(d_n0)


def test_compute_sim3_candidates_plays_the_reference_loop():
    """LoopClosing.cc:284-345 on 6 candidates: rounds of iterate(5), candidates handed back by round, then by index; a candidate
    that is not accepted goes on with its best carried over; bNoMore discards.  Against the same loop
    played with the restatement."""
    import psl_slam_amd as P
    ctx = P.default_context()
    seed0, pstride, max_its = 50, 200, 60                              # a budget of 60 keeps the loop short
    specs = [(21, 150, 0), (22, 19, 19), (23, 150, 70), (24, 200, 60), (25, 120, 60), (26, 64, 40)]
    cands = [sc.make_pairs(ds, n, ng, False, noise_px=3.0 if k == 3 else 0.0)[:2] for k, (ds, n, ng) in enumerate(specs)]
    K = len(cands)
    c1, c2 = sc.cameras()
    # the reference loop on the restatement, never accepting: every success of every candidate until all are discarded
    want, state, live, rnd = [], [[0, 0] for _ in range(K)], [True] * K, 0
    while any(live) and rnd < 100:   # a call that returns a Sim3 ends early, so a round may advance a candidate by one iteration only
        for k, (p, s) in enumerate(cands):
            if not live[k]:
                continue
            res, fl, _ = sc.iterate(p, s, c1, c2, False, seed0 + k, 5, start_it=state[k][0], best_in=state[k][1], max_its=max_its)
            state[k] = [int(res["iterations"]), int(res["best_inliers"])]
            if res["status"] == 2:
                live[k] = False
            if res["status"] == 1:
                want.append((rnd, k, res, fl))
        rnd += 1
    assert not any(live) and len(want) >= 4 and len({k for _, k, _, _ in want}) >= 3
    Pr, Sg, n = np.zeros((K, pstride), P.SIM3PAIR_DTYPE), np.zeros((K, pstride, 2), np.float32), np.zeros(K, np.int32)
    for k, (p, s) in enumerate(cands):
        Pr[k, :len(p)], Sg[k, :len(p)], n[k] = p, s, len(p)
    d_p, d_s, d_n = _dev(ctx, Pr), _dev(ctx, Sg), _dev(ctx, n)
    got = list(P.Sim3Solver.ComputeSim3Candidates(K, d_p, d_s, d_n, pstride, _cam_rec(P, c1), _cam_rec(P, c2), False, seed0, max_its=max_its, ctx=ctx))
    assert [(r, k) for r, k, _, _ in got] == [(r, k) for r, k, _, _ in want]
    for (r, k, res, fl), (_, _, wres, wfl) in zip(got, want):
        _same((res, fl), (wres, wfl, None), (r, k))
    # bMatch: the caller stops at the first candidate it accepts
    gen = P.Sim3Solver.ComputeSim3Candidates(K, d_p, d_s, d_n, pstride, _cam_rec(P, c1), _cam_rec(P, c2), False, seed0, max_its=max_its, ctx=ctx)
    first = next(gen)
    gen.close()
    assert (first[0], first[1]) == (want[0][0], want[0][1])
    for d in (d_p, d_s, d_n):
        ctx.device_free(d)


def _build_consumer(tmp_path):
    exe = str(tmp_path / "sim3_solver_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "sim3_solver_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    return exe


def _read_handed(f, cases):
    """the "candidates" section of out.bin -> [(round, candidate, result, flags)]"""
    out = []
    for _ in range(int(np.fromfile(f, np.int32, 1)[0])):
        rnd, c = (int(v) for v in np.fromfile(f, np.int32, 2))
        res = np.fromfile(f, sc.RESULT_DTYPE, 1)[0]
        out.append((rnd, c, res, np.fromfile(f, np.uint8, len(cases[c]["pairs"]))))
    return out


@pytest.mark.parametrize("fix", [True, False])
def test_cpp_consumer_equals_restatement(tmp_path, fix):
    """tools/dropin/sim3_solver_main.cpp on pslfe.hpp in rounds of 5: the device form, the mirror class and its own plain C++ loop,
    each against the restatement's find()"""
    exe = _build_consumer(tmp_path)
    names = _names(fix)
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = write_cases(path, names, fix, 5)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        loop, dev, host = read_section(f, cases), read_section(f, cases), read_section(f, cases)
        handed = _read_handed(f, cases)
        assert f.read() == b""
    for nm, c, a, b, h in zip(names, cases, loop, dev, host):
        assert_equal_ref(a, c["ref"], nm + " loop")
        assert_equal_ref(b, c["ref"], nm + " device", trace=False)
        assert_equal_ref(h, c["ref"], nm + " host", trace=False)
    order = [(r, c) for r, c, _, _ in handed]
    assert len(order) > len(names) and order == sorted(order)           # by round, then by index


def test_cpp_compute_sim3_candidates_plays_the_reference_loop(tmp_path):
    """pslfe::Sim3Solver::ComputeSim3Candidates through the consumer: five cases as the candidates of one keyframe, candidate c seeded
    seed0 + c, a budget of 40, none accepted.  Every (round, candidate) it hands over, with its result and flags, is what
    LoopClosing.cc:284-345 played on the restatement hands over, in that order."""
    exe = _build_consumer(tmp_path)
    names, max_its = ["n63", "n21", "n65", "n127", "n150_noisy"], 40
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    cases = write_cases(path, names, False, 5, max_its=max_its)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        for _ in range(3):
            read_section(f, cases)
        handed = _read_handed(f, cases)
        assert f.read() == b""
    seed0, K = cases[0]["seed"], len(cases)
    want, state, live, rnd = [], [[0, 0] for _ in range(K)], [True] * K, 0
    while any(live) and rnd < 100:
        for k, c in enumerate(cases):
            if not live[k]:
                continue
            res, fl, _ = sc.iterate(c["pairs"], c["sigma2"], c["cam1"], c["cam2"], False, seed0 + k, 5, start_it=state[k][0], best_in=state[k][1],
                                    max_its=max_its)
            state[k] = [int(res["iterations"]), int(res["best_inliers"])]
            if res["status"] == 2:
                live[k] = False
            if res["status"] == 1:
                want.append((rnd, k, res, fl))
        rnd += 1
    assert not any(live) and len(want) >= 6 and len({k for _, k, _, _ in want}) >= 3 and max(r for r, _, _, _ in want) >= 3
    assert [(r, k) for r, k, _, _ in handed] == [(r, k) for r, k, _, _ in want]
    for (r, k, res, fl), (_, _, wres, wfl) in zip(handed, want):
        _same((res, fl), (wres, wfl, None), (r, k))


def test_negative_state_is_reported_and_nothing_is_written():
    """d_start_it[c] < 0 or d_best_in[c] < 0: status PSLFE_E_INVALID, the other fields 0, no flag byte written - as for a bad count"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = sc.case("n63")
    cands = [(c["pairs"], c["sigma2"])] * 3
    got = _run_device(P, ctx, cands, c["seed"], sc.MAX_ITS, False, start=[-1, 0, 0], best=[0, 0, -5])
    want = np.zeros((), P.SIM3SOLVERRESULT_DTYPE)
    want["status"] = -1
    for k in (0, 2):
        assert got[k][0].tobytes() == want.tobytes() and (got[k][1] == 0xAA).all()
    _same(got[1], sc.find(c["pairs"], c["sigma2"], c["cam1"], c["cam2"], False, c["seed"] + 1), "the candidate between them")


def test_a_keyframe_sized_stride():
    """pstride = 2048, the capacity of a keyframe's rows as INTEGRATION.md calls it: a budget table of 2029 counts; candidates of 1025,
    65 and 2048 pairs (the last one: the rows of n1025 twice, less two)"""
    import psl_slam_amd as P
    ctx = P.default_context()
    a, b = sc.case("n1025"), sc.case("n65")
    big = (np.concatenate([a["pairs"], a["pairs"][:1023]]), np.concatenate([a["sigma2"], a["sigma2"][:1023]]))
    cands = [(a["pairs"], a["sigma2"]), (b["pairs"], b["sigma2"]), big]
    seed0 = 31
    got = _run_device(P, ctx, cands, seed0, sc.MAX_ITS, False, pstride=2048)
    c1, c2 = sc.cameras()
    for k, (p, s) in enumerate(cands):
        _same(got[k], sc.find(p, s, c1, c2, False, seed0 + k), k)
        assert (got[k][1][len(p):] == 0xAA).all()
    assert {int(g[0]["status"]) for g in got} == {1}
    s = P.Sim3Solver(big[0], big[1], np.arange(2048, dtype=np.int32), 2048, _cam_rec(P, c1), _cam_rec(P, c2), False, seed0 + 2, ctx=ctx)
    s.SetRansacParameters(sc.PROB, sc.MIN_INLIERS, sc.MAX_ITS)
    s.find()
    _same((s.result, s.row_inliers), (got[2][0], got[2][1][:2048], None), "host form")


def _chain_world():
    """The loop pair of tests/loop_cases.py (the kf_scene keyframes test_sim3_opt_gpu.py chains, KF2 carrying noisy copies of KF1's
    descriptors so that SearchByBoW finds them) with one geometry under it: every KF2 feature is a physical point on its ray, its KF1
    partner (the feature whose descriptor it copies) sees the same point through a true Sim3, and that partner's keypoint is moved
    onto the point's image in KF1.  -> dict"""
    import kf_project_cases as kc
    import kf_scene as ks
    import loop_cases as lc
    import psl_slam_amd as P
    rng = np.random.default_rng(123)
    k1, d1, k2, d2 = lc.loop_pair()
    k1 = k1.copy()
    n1, n2 = len(k1), len(k2)
    cam = kc.camera()
    fx, fy, cx, cy = (float(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    V = kc.views(nslots=2)
    T1w, T2w = V[3]["Tcw"].copy(), V[8]["Tcw"].copy()
    R1, t1 = T1w["R"].astype(np.float64).reshape(3, 3), T1w["t"].astype(np.float64)
    R2, t2 = T2w["R"].astype(np.float64).reshape(3, 3), T2w["t"].astype(np.float64)
    R12, t12, s12 = sc._rodrigues(np.array([0.03, -0.05, 0.02])), np.array([0.12, -0.06, 0.1]), 1.06
    # the partner of KF2 feature j: the KF1 feature at the smallest Hamming distance (loop_pair flips at most 12 bits)
    bits = np.unpackbits(d1, axis=1).astype(np.int16), np.unpackbits(d2, axis=1).astype(np.int16)
    ham = bits[1].sum(1)[:, None] + bits[0].sum(1)[None, :] - 2 * bits[1] @ bits[0].T          # [n2][n1]
    partner = np.where(ham.min(1) <= 12, ham.argmin(1), -1)
    z = rng.uniform(2.0, 6.0, n2)
    P2c = np.stack([(k2["x"].astype(np.float64) - cx) / fx * z, (k2["y"].astype(np.float64) - cy) / fy * z, z], 1)
    P1c = s12 * (P2c @ R12.T) + t12
    u1, v1 = P1c[:, 0] / P1c[:, 2] * fx + cx, P1c[:, 1] / P1c[:, 2] * fy + cy
    inside = (u1 > 20) & (u1 < 620) & (v1 > 20) & (v1 < 460)
    first = np.zeros(n2, bool)
    first[np.unique(partner, return_index=True)[1]] = True              # a KF1 feature is the partner of one KF2 feature
    linked = np.flatnonzero((partner >= 0) & inside & first & (rng.random(n2) < 0.65))   # the others' map points are unrelated points
    mp1, desc1 = kc.map_points(n1, seed=21)
    mp2, desc2 = kc.map_points(n2, seed=22)

    def points(mp, Pc_own, R, t, Pc_other, octave):
        """the map points whose camera coordinates are Pc_own under (R, t); seen from the other keyframe at Pc_other"""
        W = (Pc_own - t) @ R
        Ow = -R.T @ t
        mp["x"], mp["y"], mp["z"] = W.T
        nrm = W - Ow
        mp["nx"], mp["ny"], mp["nz"] = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).T
        mp["max_dist"] = np.linalg.norm(Pc_other, axis=1) * 1.2 ** (octave - 0.5)
        mp["min_dist"] = mp["max_dist"] / 1.2 ** 7
    i = partner[linked]
    a, b = mp1[i].copy(), mp2[linked].copy()
    points(a, P1c[linked], R1, t1, P2c[linked], k2["octave"][linked])    # KF1's point is searched in KF2: the distance there, KF2's octave
    points(b, P2c[linked], R2, t2, P1c[linked], k1["octave"][i])
    mp1[i], mp2[linked] = a, b
    desc1[i], desc2[linked] = ks.noisy_desc(d1[i], rng, flips=6), ks.noisy_desc(d2[linked], rng, flips=6)
    k1["x"][i] = u1[linked] + rng.normal(0, 0.3, len(linked))
    k1["y"][i] = v1[linked] + rng.normal(0, 0.3, len(linked))
    valid1, valid2 = rng.random(n1) < 0.9, rng.random(n2) < 0.9         # the features with a good map point
    return dict(k1=k1, d1=d1, k2=k2, d2=d2, cam=cam, T1w=T1w, T2w=T2w, R12=R12, t12=t12, s12=s12, mp1=mp1, desc1=desc1, mp2=mp2, desc2=desc2,
                valid1=valid1, valid2=valid2, partner=partner, linked=linked)


def test_chain_bow_pairs_solve_search_by_sim3_optimise():
    """LoopClosing::ComputeSim3 for one candidate, every step on the library: pslfe_kf_search_by_bow_candidates -> the pair set-up with
    sigma2 -> pslfe_sim3_solve_device in rounds of 5 on the rows as they lie in HBM -> the inliers are vpMapPointMatches (:313-318) ->
    pslfe_kf_search_by_sim3_poses with sR12, t12 and their inverse from the solver's S12 (:320-323) adds matches -> OptimizeSim3's
    set-up -> pslfe_sim3_optimize_device started from the S12 record inside the solver's result, which never leaves HBM (:326).
    Every stage is held to its restatement: loop_cases.restate_search_by_bow, the numpy set-up loop, sim3_solver_cases.iterate,
    kf_project_cases.restate_project + the oracle's search_by_sim3, sim3_opt_cases.optimize.  A third of the BoW matches join map points
    that are not one physical point, which the RANSAC has to outvote."""
    import kf_project_cases as kc
    import kf_scene as ks
    import loop_cases as lc
    import oracle_lib
    import psl_slam_amd as P
    import sim3_opt_cases as so
    from test_sim3_opt_gpu import _setup_loop
    from test_sim3_opt_cpu import assert_equal_ref as assert_opt_equal
    ctx = P.default_context()
    w = _chain_world()
    k1, d1, k2, d2, cam, T1w, T2w, mp1, mp2 = (w[k] for k in ("k1", "d1", "k2", "d2", "cam", "T1w", "T2w", "mp1", "mp2"))
    camd = {k: cam[k] for k in ("fx", "fy", "cx", "cy")}
    n1, n2, cap, seed0 = len(k1), len(k2), 2048, 17
    g = P.FrameGrid(cap, 2, ctx=ctx)
    g.set(0, k1, d1, ks.BOUNDS, None)
    g.set(1, k2, d2, ks.BOUNDS, None)
    kf = P.KeyFrameMatcher()
    # 1. SearchByBoW(mpCurrentKF, pKF, vvpMapPointMatches[i]) (:265)
    fidx, runs, qa, qd, idx1 = lc.bow_inputs(d1, k1["angle"], w["valid1"], ks.feature_vector(d1, 7), ks.feature_vector(d2, 7), w["valid2"])
    nms, matches = kf.SearchByBoWCandidates(g, [1], [fidx], [runs], [qa], [qd])
    r = lc.restate_search_by_bow(k2["angle"], d2, fidx, runs, qa, qd, 0.75, True)
    np.testing.assert_array_equal(matches[0], r["match"])
    assert nms[0] == r["nmatches"] >= 20                                 # :267
    i2 = np.full((1, cap), -1, np.int32)
    i2[0, idx1] = matches[0]
    right = w["partner"][np.maximum(i2[0, :n1], 0)] == np.arange(n1)
    assert ((i2[0, :n1] >= 0) & ~right).sum() >= 10                      # wrong matches are among them, next to the unrelated points
    skip1, skip2 = (~w["valid1"]).astype(np.uint8), (~w["valid2"]).astype(np.uint8)[None]

    def set_up(i2_now, d_sg):
        d_in = [_dev(ctx, a) for a in (np.array([1], np.int32), i2_now, mp1, skip1, mp2[None], skip2, np.asarray(T1w).reshape(1), np.asarray(T2w).reshape(1))]
        d_p, d_kp, d_n = _dev(ctx, np.zeros((1, cap), P.SIM3PAIR_DTYPE)), _dev(ctx, np.full((1, cap), -1, np.int32)), _dev(ctx, np.zeros(1, np.int32))
        P.Optimizer.Sim3PairsSigma2FromMatchesDevice(g, 0, g, d_in[0], 1, d_in[1], d_in[2], d_in[3], n1, d_in[4], d_in[5], n2, d_in[6], d_in[7],
                                                     ks.INV_SIGMA2, ks.SIGMA2, d_p, d_kp, d_n, cap, d_sg)
        ctx.synchronize()
        cnt = int(_down(P, ctx, d_n, np.zeros(1, np.int32))[0])
        got = _down(P, ctx, d_p, np.zeros((1, cap), P.SIM3PAIR_DTYPE))[0, :cnt], _down(P, ctx, d_kp, np.zeros((1, cap), np.int32))[0, :cnt]
        for d in d_in + [d_kp]:
            ctx.device_free(d)
        wp, wkp = _setup_loop(k1, k2, i2_now[0], mp1, skip1, mp2, skip2[0], T1w, T2w, ks.INV_SIGMA2)
        assert cnt == len(wp) and got[0].tobytes() == wp.tobytes() and (got[1] == wkp).all()
        return d_p, d_n, wp, wkp

    # 2. the Sim3Solver's constructor (:274) and its rounds of iterate(5) (:301)
    d_sg = _dev(ctx, np.zeros((1, cap, 2), np.float32))
    d_p, d_n, wp, wkp = set_up(i2, d_sg)
    assert len(wp) == nms[0]
    sg = _down(P, ctx, d_sg, np.zeros((1, cap, 2), np.float32))[0, :len(wp)]
    assert (sg[:, 0] == ks.SIGMA2[k1["octave"][wkp]]).all() and (sg[:, 1] == ks.SIGMA2[k2["octave"][i2[0, wkp]]]).all()
    d_res, d_fl = _dev(ctx, np.zeros(1, P.SIM3SOLVERRESULT_DTYPE)), _dev(ctx, np.zeros((1, cap), np.uint8))
    start = best = 0
    for _ in range(60):
        d_s, d_b = _dev(ctx, np.array([start], np.int32)), _dev(ctx, np.array([best], np.int32))
        P.Sim3Solver.SolveDevice(1, d_p, d_sg, d_n, cap, cam, cam, False, seed0, 5, d_res, d_fl, d_s, d_b, ctx=ctx)
        ctx.synchronize()
        res = _down(P, ctx, d_res, np.zeros(1, P.SIM3SOLVERRESULT_DTYPE))[0]
        fl = _down(P, ctx, d_fl, np.zeros((1, cap), np.uint8))[0, :len(wp)]
        ctx.device_free(d_s)
        ctx.device_free(d_b)
        _same((res, fl), sc.iterate(wp, sg, camd, camd, False, seed0, 5, start_it=start, best_in=best), "solver round")
        start, best = int(res["iterations"]), int(res["best_inliers"])
        if res["status"] != 0:
            break
    assert res["status"] == 1 and res["ninliers"] > 20 and 0 < (fl == 0).sum()
    R, t, s = res["S12"]["R"].reshape(3, 3).astype(np.float64), res["S12"]["t"].astype(np.float64), float(res["S12"]["s"])
    assert np.abs(R - w["R12"]).max() < 2e-3 and abs(s - w["s12"]) < 5e-3
    # 3. SearchBySim3(mpCurrentKF, pKF, vpMapPointMatches, s, R, t, 7.5) (:323): the inliers are matched already, the others are searched
    matched = np.full(n1, -1, np.int32)
    matched[wkp[fl == 1]] = i2[0, wkp[fl == 1]]
    sk1, sk2 = skip1.copy(), skip2[0].copy()
    sk1[matched >= 0] = 1                                               # vbAlreadyMatched1 / 2 (src/ORBmatcher.cc:1131-1146)
    sk2[matched[matched >= 0]] = 1
    v12, v21 = np.zeros((), P.KFVIEW_DTYPE), np.zeros((), P.KFVIEW_DTYPE)
    v12["Tcw"], v12["slot"], v12["T21"] = T1w, 1, kc.pose_record(R.T / s, -(R.T / s) @ t)   # sR21, t21 (:1119-1121)
    v21["Tcw"], v21["slot"], v21["T21"] = T2w, 0, kc.pose_record(s * R, t)                  # sR12, t12
    nf, match, r12, r21 = kf.SearchBySim3Poses(g, g, v12, mp1, w["desc1"], sk1, v21, mp2, w["desc2"], sk2, cam, ks.BOUNDS, ks.SCALE, kc.LOG_SCALE, 7.5)
    q12, _, _ = kc.restate_project(kc.SIM3, v12.reshape(1), mp1, cam, ks.BOUNDS, ks.SCALE, 7.5, sk1.reshape(1, -1))
    q21, _, _ = kc.restate_project(kc.SIM3, v21.reshape(1), mp2, cam, ks.BOUNDS, ks.SCALE, 7.5, sk2.reshape(1, -1))
    onf, omatch = oracle_lib.search_by_sim3(k1, d1, ks.BOUNDS, k2, d2, ks.BOUNDS, q12[0], w["desc1"], q21[0], w["desc2"])
    assert r12.tobytes() == q12[0].tobytes() and r21.tobytes() == q21[0].tobytes()
    np.testing.assert_array_equal(match, omatch)
    assert nf == onf >= 5                                                # the search finds partners the BoW walk missed
    found = np.flatnonzero(np.asarray(match) >= 0)
    assert (matched[found] < 0).all() and (w["partner"][match[found]] == found).mean() > 0.9
    matched[found] = match[found]
    # 4. OptimizeSim3(mpCurrentKF, pKF, vpMapPointMatches, gScm, 10, mbFixScale) (:326) on the inliers and the new matches
    i2_all = np.full((1, cap), -1, np.int32)
    i2_all[0, :n1] = matched
    ctx.device_free(d_p)
    ctx.device_free(d_n)
    d_p, d_n, wp2, wkp2 = set_up(i2_all, 0)
    assert len(wp2) == res["ninliers"] + nf
    d_o, d_b2 = _dev(ctx, np.zeros(1, P.SIM3D_DTYPE)), _dev(ctx, np.zeros(cap, np.uint8))
    d_g, d_i = _dev(ctx, np.zeros(1, np.int32)), _dev(ctx, np.zeros(1, P.SIM3INFO_DTYPE))
    d_S12 = d_res + P.SIM3SOLVERRESULT_DTYPE.fields["S12"][1]           # &d_res[0].S12
    P.Optimizer.OptimizeSim3Device(1, d_S12, d_p, d_n, cap, cam, cam, so.TH2, False, d_o, d_b2, d_g, d_i, ctx=ctx)
    ctx.synchronize()
    got = (_down(P, ctx, d_o, np.zeros(1, P.SIM3D_DTYPE))[0], _down(P, ctx, d_b2, np.zeros(cap, np.uint8))[:len(wp2)],
           int(_down(P, ctx, d_g, np.zeros(1, np.int32))[0]), _down(P, ctx, d_i, np.zeros(1, P.SIM3INFO_DTYPE))[0])
    assert_opt_equal(got, so.optimize(res["S12"], wp2, camd, camd, so.TH2, False)[:4], "chain")
    assert got[2] >= 20                                                  # :329: bMatch
    Ro, to, so_ = so.s3_matrix((list(got[0]["q"]), list(got[0]["t"]), float(got[0]["s"])))
    assert np.abs(Ro - w["R12"]).max() < 2e-3 and abs(so_ - w["s12"]) < 5e-3
    for d in (d_p, d_n, d_sg, d_res, d_fl, d_o, d_b2, d_g, d_i):
        ctx.device_free(d)
