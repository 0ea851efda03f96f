"""GPU parity of the EPnP RANSAC (psl-slam_amd/csrc/pslfe_pnp.hip) with the restatement of tests/pnp_cases.py, bit for bit: status,
iterations, the counts, min_inliers, both poses and every flag of every call; the host form; calls of iterate(5) resumed through the
state in HBM after poses that were refused; a batch of 67 candidates against single launches; the error paths; the constructor's loop
and the masking of the matches on the device; the candidate loop of Relocalization in both mirrors; the C++ consumer
tools/dropin/pnp_main.cpp; and the chain of Tracking::Relocalization from SearchByBoW to PoseOptimization with every stage held to its
restatement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _cam_rec(P, cam=pc.CAM):
    rec = np.zeros((), P.CAMERA_DTYPE)
    for k, v in cam.items():
        rec[k] = v
    return rec


def _solver_kw(params):
    return dict(prob=params["prob"], min_inliers=params["min_inliers"], max_its=params["max_its"], min_set=params["min_set"],
                epsilon=params["epsilon"], th2=params["th2"])


class _Device:
    """K candidates resident in HBM with their solver state; the flags start as 0xAA"""

    def __init__(self, P, ctx, rows_list, rstride=None, counts=None, state=None):
        self.P, self.ctx, self.K = P, ctx, len(rows_list)
        self.rstride = rstride if rstride is not None else max(max(len(r) for r in rows_list), 1)
        R, n = np.zeros((self.K, max(self.rstride, 1)), P.PNPROW_DTYPE), np.zeros(self.K, np.int32)
        for k, r in enumerate(rows_list):
            m = min(len(r), self.rstride)
            R[k, :m] = r[:m]
            n[k] = len(r) if counts is None else counts[k]
        st = np.zeros(self.K, P.PNPRESULT_DTYPE) if state is None else state
        self.shape = (self.K, max(self.rstride, 1))
        self.d_rows, self.d_n, self.d_res = _dev(ctx, R), _dev(ctx, n), _dev(ctx, st)
        self.d_best, self.d_fl = _dev(ctx, np.full(self.shape, 0xAA, np.uint8)), _dev(ctx, np.full(self.shape, 0xAA, np.uint8))

    def call(self, seed0, n_iterations, params, fresh=False):
        """one launch, the state read from and written to d_res -> [(result, flags [rstride])]"""
        P, ctx = self.P, self.ctx
        P.PnPsolver.SolveDevice(self.K, self.d_rows, self.d_n, self.rstride, _cam_rec(P), seed0, n_iterations, 0 if fresh else self.d_res, self.d_best,
                                self.d_res, self.d_fl, ctx=ctx, **_solver_kw(params))
        ctx.synchronize()
        res, fl = _down(P, ctx, self.d_res, np.zeros(self.K, P.PNPRESULT_DTYPE)), _down(P, ctx, self.d_fl, np.zeros(self.shape, np.uint8))
        return [(res[k].copy(), fl[k].copy()) for k in range(self.K)]

    def best_flags(self):
        return _down(self.P, self.ctx, self.d_best, np.zeros(self.shape, np.uint8))

    def free(self):
        for d in (self.d_rows, self.d_n, self.d_res, self.d_best, self.d_fl):
            self.ctx.device_free(d)


def _play_device(P, ctx, c, n_iterations, reject, rstride=None):
    """pnp_cases.play on the device: -> ([(result, flags[:n])], best_flags[:n], every flag byte beyond n untouched?)"""
    n = len(c["rows"])
    D = _Device(P, ctx, [c["rows"]], rstride=rstride)
    calls, rejected, untouched = [], 0, True
    while True:
        res, fl = D.call(c["seed"], n_iterations, c["params"])[0]
        calls.append((res, fl[:n]))
        untouched = untouched and (fl[n:] == 0xAA).all()
        st = int(res["status"])
        if st < 0 or st & 2 or (n_iterations <= 0 and not st & 1) or len(calls) > 200:
            break
        if st & 1:
            if rejected >= reject:
                break
            rejected += 1
    bf = D.best_flags()[0]
    D.free()
    return calls, bf[:n], untouched and (bf[n:] == 0xAA).all()


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_device_and_host_forms_equal_restatement(name):
    """3 rows (bNoMore, nothing solved), 4 with min_inliers 4 (budget 1, all four drawn), 5 and 9 below the clamp of 10, 15, 63 / 64 /
    65 around the wave loop, 384 = the LDS row limit, 385 with a row staged from HBM, 400; consistent rows at 100 %, 50 % and 20 %; a
    planar point set, identical rows, a point behind the camera; a Refine on a hypothesis that is not a new best, a Refine that fails
    at == min_inliers before one that succeeds; budgets of 15, 16 and 17 around the block of 16.  As one find(), with the row count as
    the stride and with a larger one, and through the mirror class."""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = pc.case(name)
    n = len(c["rows"])
    for rstride in (n + 3, max(n, 1)):
        calls, bf, untouched = _play_device(P, ctx, c, c["find_its"], 0, rstride=rstride)
        pc.assert_play_equal((calls, bf), c["find"], (name, rstride))
        assert untouched                                                 # bytes beyond the count are not touched
    s = P.PnPsolver(c["rows"], np.arange(n, dtype=np.int32)[::-1].copy(), n, _cam_rec(P), c["seed"], ctx=ctx)   # row i is keypoint n - 1 - i
    s.SetRansacParameters(*(c["params"][k] for k in ("prob", "min_inliers", "max_its", "min_set", "epsilon", "th2")))
    T, vb, nin = s.find()
    rres, rfl = c["find"][0][-1]
    assert pc.same_result(s.result, rres) and (s.row_inliers == rfl).all()
    assert (T is not None) == bool(rres["status"] & 1) and nin == rres["inliers"]
    if T is not None:
        assert (vb[::-1] == rfl.astype(bool)).all() and pc.same_floats(T["R"], rres["Tcw"]["R"])
    else:
        assert len(vb) == 0


@pytest.mark.parametrize("name", ["n15", "n63", "n65_half", "n400_half", "noisy40_eq", "noisy40_notbest", "its17", "n60_fifth"])
def test_rounds_resumed_through_the_state_equal_one_solver_object(name):
    """iterate(5) (7 for its17) repeated through (state, best_flags) in HBM, also after a returned pose that was refused, equals the
    restatement's loop continued on one solver object whose rand() stream is never reseeded; and the mirror's iterate"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = pc.case(name)
    calls, bf, untouched = _play_device(P, ctx, c, c["n_iterations"], c["reject"])
    pc.assert_play_equal((calls, bf), c["rounds"], name)
    n = len(c["rows"])
    s = P.PnPsolver(c["rows"], np.arange(n, dtype=np.int32), n, _cam_rec(P), c["seed"], ctx=ctx)
    s.SetRansacParameters(*(c["params"][k] for k in ("prob", "min_inliers", "max_its", "min_set", "epsilon", "th2")))
    for rres, rfl in c["rounds"][0]:
        T, no_more, vb, nin = s.iterate(c["n_iterations"])
        assert pc.same_result(s.result, rres) and (s.row_inliers == rfl).all() and no_more == bool(rres["status"] & 2)
    if int(c["rounds"][0][-1][0]["best_inliers"]) > 0:
        assert (s.best_flags[:n] == c["rounds"][1]).all()


def test_a_first_call_that_ends_by_budget_equals_find():
    """the loop's condition is an ||: iterate(5) on a fresh solver runs on to mRansacMaxIts"""
    import psl_slam_amd as P
    ctx = P.default_context()
    for nm in ("n60_fifth", "n64_half"):
        c = pc.case(nm)
        calls, bf, _ = _play_device(P, ctx, c, 5, 0)
        assert len(calls) == 1
        pc.assert_play_equal((calls, bf), c["find"], nm)


def _mixed_batch(K):
    """K candidates of mixed row counts and shares of consistent rows"""
    rng = np.random.default_rng(88)
    counts = [3, 4, 9, 10, 15, 63, 64, 65, 120, 200] + list(rng.integers(12, 130, K - 10))
    return [pc.make_rows(2000 + k, int(n), max(int(n * (0.45 + 0.5 * rng.random())), min(int(n), 4)), noise_px=0.3)[0] for k, n in enumerate(counts)]


def test_batch_of_67_equals_single_launches():
    """the position in the batch and the row stride do not matter; candidates with an overflowing or a negative count are reported and
    leave their outputs untouched while their neighbours are solved; a fifth of the batch against the restatement too"""
    import psl_slam_amd as P
    ctx = P.default_context()
    K, seed0, params = 67, 500, dict(pc.RELOC, max_its=20)
    cands = _mixed_batch(K)
    counts = [len(r) for r in cands]
    counts[20], counts[41] = 300, -1                                     # above the stride of 200; an error code left by the set-up
    D = _Device(P, ctx, cands, rstride=200, counts=counts)
    got = D.call(seed0, 5, params, fresh=True)
    bf = D.best_flags()
    D.free()
    want = np.zeros((), P.PNPRESULT_DTYPE)
    for k, code in ((20, -4), (41, -1)):
        want["status"] = code
        assert got[k][0].tobytes() == want.tobytes() and (got[k][1] == 0xAA).all() and (bf[k] == 0xAA).all()
    statuses = set()
    for k, rows in enumerate(cands):
        if k in (20, 41):
            continue
        n = len(rows)
        single = _Device(P, ctx, [rows])
        one = single.call(seed0 + k, 5, params, fresh=True)[0]
        single.free()
        assert pc.same_result(got[k][0], one[0]) and (got[k][1][:n] == one[1][:n]).all() and (got[k][1][n:] == 0xAA).all(), k
        statuses.add(int(one[0]["status"]))
        if k % 5 == 0:
            res, fl = pc.Solver(rows, pc.CAM, seed0 + k, **params).iterate(5)
            assert pc.same_result(got[k][0], res) and (got[k][1][:n] == fl).all(), k
    assert {1, 2, 3} <= statuses


def test_negative_state_is_reported_and_nothing_is_written():
    import psl_slam_amd as P
    ctx = P.default_context()
    c = pc.case("n63")
    state = np.zeros(3, P.PNPRESULT_DTYPE)
    state["iterations"][0], state["best_inliers"][2] = -1, -5
    D = _Device(P, ctx, [c["rows"]] * 3, state=state)
    got = D.call(c["seed"], c["find_its"], c["params"])
    bf = D.best_flags()
    D.free()
    want = np.zeros((), P.PNPRESULT_DTYPE)
    want["status"] = -1
    for k in (0, 2):
        assert got[k][0].tobytes() == want.tobytes() and (got[k][1] == 0xAA).all() and (bf[k] == 0xAA).all()
    res, fl = pc.Solver(c["rows"], pc.CAM, c["seed"] + 1, **c["params"]).find()
    assert pc.same_result(got[1][0], res) and (got[1][1] == fl).all()


def test_errors():
    import psl_slam_amd as P
    ctx = P.default_context()
    c = pc.case("n15")
    D = _Device(P, ctx, [c["rows"]])
    cam = _cam_rec(P)

    def solve(ncand=1, d_rows=D.d_rows, d_n=D.d_n, rstride=15, n_iterations=5, d_best=D.d_best, d_res=D.d_res, d_fl=D.d_fl, **kw):
        P.PnPsolver.SolveDevice(ncand, d_rows, d_n, rstride, cam, 1, n_iterations, 0, d_best, d_res, d_fl, ctx=ctx, **dict(_solver_kw(pc.RELOC), **kw))

    solve(ncand=0, d_rows=0, d_n=0, d_res=0)                             # PSLFE_OK, nothing looked at
    for kw in (dict(ncand=-1), dict(rstride=-1), dict(n_iterations=-1), dict(prob=0.0), dict(prob=1.0), dict(max_its=0), dict(min_inliers=-1),
               dict(min_set=3), dict(min_set=5), dict(epsilon=float("nan")), dict(th2=float("nan")), dict(d_rows=0), dict(d_n=0), dict(d_res=0),
               dict(d_best=0), dict(d_fl=0)):
        with pytest.raises(P.PslfeError, match="code -1"):
            solve(**kw)
    res, fl = D.call(c["seed"], c["find_its"], c["params"], fresh=True)[0]   # the context still works
    assert pc.same_result(res, c["find"][0][-1][0])
    D.free()
    s = P.PnPsolver(c["rows"], np.arange(15, dtype=np.int32), 15, cam, 1, ctx=ctx)
    s.SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991)
    with pytest.raises(P.PslfeError, match="code -1"):
        s.iterate(5)
    with pytest.raises(P.PslfeError):
        P.PnPsolver(c["rows"], np.arange(14, dtype=np.int32), 15, cam, 1, ctx=ctx)
    with pytest.raises(P.PslfeError, match="code -1"):
        P.PnPsolver.MapPointIndexFromInliersDevice(1, D.d_n, D.d_n, D.d_n, D.d_n, 4, 4, D.d_n, ctx=ctx)   # aliased index arrays


def _ctor_loop(kps, idx, mp, sigma2):
    """src/PnPsolver.cc:78-101 in numpy -> rows, mvKeyPointIndices"""
    keep = np.flatnonzero((idx >= 0) & (idx < len(mp)))
    rows = np.zeros(len(keep), pc.ROW_DTYPE)
    rows["u"], rows["v"] = kps["x"][keep], kps["y"][keep]
    for a, b in (("X", "x"), ("Y", "y"), ("Z", "z")):
        rows[a] = mp[b][idx[keep]]
    rows["sigma2"] = sigma2[kps["octave"][keep]]
    return rows, keep.astype(np.int32)


def test_rows_from_matches_and_mp_index_from_inliers():
    """the constructor's loop on a slot of 600 keypoints for two candidates (more than one chunk of 256, a ragged tail), -1 entries, indices
    outside the array counted as none, and a count above rstride that is reported and not truncated silently; then Tracking.cc:2119-2128"""
    import psl_slam_amd as P
    ctx = P.default_context()
    rng = np.random.default_rng(5)
    cap, M, nlev, n = 640, 500, 8, 600
    sigma2 = ((np.float32(1.2) ** np.arange(nlev, dtype=np.float32)) ** 2).astype(np.float32)
    g = P.FrameGrid(cap, 2, ctx=ctx)
    kps = np.zeros(n, P.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.integers(0, nlev, n)
    g.set(1, kps, rng.integers(0, 256, (n, 32), dtype=np.uint8), (0.0, 0.0, 640.0, 480.0))
    idx = np.full((2, cap), -1, np.int32)
    mp = np.zeros((2, M), P.MAPPOINT_DTYPE)
    for c, share in enumerate((0.7, 0.2)):
        idx[c, :n] = np.where(rng.random(n) < share, rng.integers(0, M, n), -1)
        idx[c, 5], idx[c, 7] = M, -7                                    # outside the array: no map point
        for k in ("x", "y", "z"):
            mp[c][k] = rng.normal(size=M)
    d_idx, d_mp = _dev(ctx, idx), _dev(ctx, mp)
    for rstride in (cap, 256):
        d_r, d_kp, d_n = _dev(ctx, np.zeros((2, rstride), P.PNPROW_DTYPE)), _dev(ctx, np.full((2, rstride), -1, np.int32)), _dev(ctx, np.zeros(2, np.int32))
        P.PnPsolver.RowsFromMatchesDevice(g, 1, 2, d_idx, d_mp, M, sigma2, d_r, d_kp, d_n, rstride)
        ctx.synchronize()
        r, kp, cnt = _down(P, ctx, d_r, np.zeros((2, rstride), P.PNPROW_DTYPE)), _down(P, ctx, d_kp, np.zeros((2, rstride), np.int32)), _down(P, ctx, d_n, np.zeros(2, np.int32))
        for c in range(2):
            wr, wkp = _ctor_loop(kps, idx[c, :n], mp[c], sigma2)
            m = min(len(wr), rstride)
            assert cnt[c] == len(wr) and r[c, :m].tobytes() == wr[:m].tobytes() and (kp[c, :m] == wkp[:m]).all() and (kp[c, m:] == -1).all()
        assert rstride == cap or cnt[0] > rstride > cnt[1]              # candidate 0 overflows 256, candidate 1 does not
        # the masking: a third of the rows are inliers
        inl = (rng.random((2, rstride)) < 0.33).astype(np.uint8)
        d_inl, d_out = _dev(ctx, inl), _dev(ctx, np.full((2, cap), -9, np.int32))
        P.PnPsolver.MapPointIndexFromInliersDevice(2, d_idx, d_kp, d_inl, d_n, rstride, cap, d_out, ctx=ctx)
        ctx.synchronize()
        out = _down(P, ctx, d_out, np.zeros((2, cap), np.int32))
        for c in range(2):
            m = min(int(cnt[c]), rstride)
            want = np.full(cap, -1, np.int32)
            keep = kp[c, :m][inl[c, :m] == 1]
            want[keep] = idx[c, keep]
            assert (out[c] == want).all() and (want >= 0).sum() > 10
        for d in (d_r, d_kp, d_n, d_inl, d_out):
            ctx.device_free(d)
    d_n = _dev(ctx, np.zeros(1, np.int32))
    P.PnPsolver.RowsFromMatchesDevice(g, 1, 1, d_idx + cap * 4, d_mp + M * 32, M, sigma2, 0, 0, d_n, 0)   # counting alone
    ctx.synchronize()
    assert _down(P, ctx, d_n, np.zeros(1, np.int32))[0] == len(_ctor_loop(kps, idx[1, :n], mp[1], sigma2)[0])
    with pytest.raises(P.PslfeError, match="code -5"):
        P.PnPsolver.RowsFromMatchesDevice(g, 0, 1, d_idx, d_mp, M, sigma2, 0, 0, d_n, 0)     # slot 0 was never set
    for d in (d_idx, d_mp, d_n):
        ctx.device_free(d)


def _relocalize_reference(cases, seed0, params, per_round, accept_after):
    """src/Tracking.cc:2088-2180 on the restatement: -> (matched candidate or -1, [(round, candidate, result, flags)])"""
    solvers = [pc.Solver(c["rows"], pc.CAM, seed0 + k, **params) for k, c in enumerate(cases)]
    live, handed, rnd = [True] * len(cases), [], 0
    while any(live) and rnd < 100:
        for k, s in enumerate(solvers):
            if not live[k]:
                continue
            res, fl = s.iterate(per_round)
            if res["status"] & 2:
                live[k] = False
            if res["status"] & 1:
                handed.append((rnd, k, res, fl))
                if len(handed) > accept_after:
                    return k, handed
        rnd += 1
    return -1, handed


def test_relocalize_candidates_plays_the_reference_loop():
    """RelocalizeCandidates on three candidates: the stand-in for the pose optimisation refuses the first pose handed over (the first
    candidate's) and accepts the second; then with nothing accepted until every candidate is discarded by bNoMore"""
    import psl_slam_amd as P
    ctx = P.default_context()
    names, seed0, params = ["n65_half", "noisy40_notbest", "noisy40_eq"], 33, dict(pc.RELOC, max_its=24)   # seed searched
    cases = [pc.case(nm) for nm in names]
    D = _Device(P, ctx, [c["rows"] for c in cases])
    kw = dict(prob=params["prob"], min_inliers=params["min_inliers"], max_its=params["max_its"], epsilon=params["epsilon"], th2=params["th2"])
    for accept_after in (1, 10 ** 6):
        want_c, want = _relocalize_reference(cases, seed0, params, 5, accept_after)
        got = []
        gen = P.PnPsolver.RelocalizeCandidates(D.K, D.d_rows, D.d_n, D.rstride, _cam_rec(P), seed0, per_round=5, max_rounds=50, ctx=ctx, **kw)
        matched = -1
        for rnd, c, res, fl in gen:
            got.append((rnd, c, res, fl))
            if len(got) > accept_after:
                matched = c
                gen.close()
                break
        assert matched == want_c and [(r, c) for r, c, _, _ in got] == [(r, c) for r, c, _, _ in want]
        for (_, c, res, fl), (_, _, wres, wfl) in zip(got, want):
            assert pc.same_result(res, wres) and (fl[:len(wfl)] == wfl).all()
        if accept_after == 1:
            assert want[0][1] == 0 and want_c != 0 and len(want) == 2   # the first is refused, the second accepted
        else:
            assert matched == -1 and len({c for _, c, _, _ in want}) == 3 and len(want) >= 4
    D.free()


def _build_consumer(tmp_path):
    exe = str(tmp_path / "pnp_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "pnp_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    return exe


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/pnp_main.cpp on pslfe.hpp, every case in rounds with poses refused: the device form, the mirror class and its own
    plain C++ loop, each against the restatement; and pslfe::PnPsolver::RelocalizeCandidates with the first pose refused"""
    import psl_slam_amd as P
    exe = _build_consumer(tmp_path)
    names = ["n65_half"] + [nm for nm in pc.CASE_NAMES if nm != "n65_half"]
    cases = [pc.case(nm) for nm in names]
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    pc.write_cases(path, cases, "rounds", P.CAMERA_DTYPE)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        loop, dev, host = pc.read_section(f, cases), pc.read_section(f, cases), pc.read_section(f, cases)
        matched, nh = (int(v) for v in np.fromfile(f, np.int32, 2))
        handed = []
        for _ in range(nh):
            rnd, c = (int(v) for v in np.fromfile(f, np.int32, 2))
            res = np.fromfile(f, pc.RESULT_DTYPE, 1)[0]
            handed.append((rnd, c, res, np.fromfile(f, np.uint8, len(cases[c]["rows"]))))
        assert f.read() == b""
    for nm, c, a, b, h in zip(names, cases, loop, dev, host):
        pc.assert_play_equal(a, c["rounds"], nm + " loop")
        pc.assert_play_equal(b, c["rounds"], nm + " device")
        pc.assert_play_equal(h, c["rounds"], nm + " host", best_flags=False)
    c0 = cases[0]
    want_c, want = _relocalize_reference(cases, c0["seed"], c0["params"], c0["n_iterations"], c0["reject"])
    assert matched == want_c and [(r, c) for r, c, _, _ in handed] == [(r, c) for r, c, _, _ in want] and len(want) == c0["reject"] + 1
    for (_, _, res, fl), (_, _, wres, wfl) in zip(handed, want):
        assert pc.same_result(res, wres) and (fl == wfl).all()


def test_chain_bow_rows_solve_mask_edges_pose():
    """Tracking::Relocalization for one candidate keyframe, every step on the library: SearchByBoW(pKF, F, vvpMapPointMatches[i])
    (:2067) -> the PnPsolver's constructor -> pslfe_pnp_solve_device in rounds of 5 on the rows as they lie in HBM -> the inliers mask
    the matches (:2119-2128) -> the edge set-up -> pslfe_pose_optimize_device started from the Tcw record inside the solver's result,
    which never leaves HBM (:2109).  Every stage is held to its restatement: the oracle's search_by_bow, the numpy constructor loop,
    pnp_cases.Solver, the numpy mask, the numpy gather and pose_opt_cases.optimize.  A quarter of the keyframe's map points are not the
    points its features show, which the RANSAC has to outvote."""
    import kf_scene as ks
    import loop_cases as lc
    import oracle_lib
    import pose_opt_cases as po
    import psl_slam_amd as P
    from test_pose_opt_gpu import _cam, _gather, _kf_world
    ctx = P.default_context()
    kps, desc, uright, mp, Ttrue, T0 = _kf_world(P)
    n = len(kps)
    cap, seed0 = n + 17, 23
    rng = np.random.default_rng(77)
    cam = _cam(P)
    camd = {k: float(cam[k]) for k in ("fx", "fy", "cx", "cy")}
    g = P.FrameGrid(cap, 1, ctx=ctx)
    g.set(0, kps, desc, ks.BOUNDS, uright=uright)
    # the candidate keyframe: its features are noisy copies of F's in another order; feature j's map point is the point F's keypoint
    # perm[j] shows, or (a quarter) some other point
    perm = rng.permutation(n)
    dK, aK = ks.noisy_desc(desc[perm], rng, flips=6), kps["angle"][perm]
    mpK = mp[perm].copy()
    wrong = np.flatnonzero(rng.random(n) < 0.25)
    mpK[wrong] = mp[rng.integers(0, n, len(wrong))]
    validK = rng.random(n) < 0.9
    # 1. SearchByBoW(pKF, F, vvpMapPointMatches[i])
    fidx, runs, qa, qd, idxK = lc.bow_inputs(dK, aK, validK, ks.feature_vector(dK, 7), ks.feature_vector(desc, 7), np.ones(n, bool))
    nm, match, assigned = P.ORBmatcher(0.75, True).SearchByBoW(g, 0, fidx, runs, qa, qd)
    onm, omatch, oassigned = oracle_lib.search_by_bow(desc, kps["angle"], fidx, runs, qd, qa, 0.75, True)
    assert nm == onm >= 15 and (match == omatch).all() and (assigned == oassigned).all()   # :2068: nmatches < 15 discards
    mp_index = np.full((1, cap), -1, np.int32)
    hit = np.flatnonzero(assigned >= 0)
    mp_index[0, hit] = idxK[assigned[hit]]                              # vpMapPointMatches[F keypoint] = the keyframe's map point
    # 2. the PnPsolver's constructor and its rounds of iterate(5)
    d_idx, d_mp = _dev(ctx, mp_index), _dev(ctx, mpK)
    d_rows, d_kp, d_n = _dev(ctx, np.zeros(cap, P.PNPROW_DTYPE)), _dev(ctx, np.full(cap, -1, np.int32)), _dev(ctx, np.zeros(1, np.int32))
    P.PnPsolver.RowsFromMatchesDevice(g, 0, 1, d_idx, d_mp, n, ks.SIGMA2, d_rows, d_kp, d_n, cap)
    ctx.synchronize()
    wrows, wkp = _ctor_loop(kps, mp_index[0, :n], mpK, np.asarray(ks.SIGMA2, np.float32))
    cnt = int(_down(P, ctx, d_n, np.zeros(1, np.int32))[0])
    assert cnt == len(wrows) == nm and _down(P, ctx, d_rows, np.zeros(cap, P.PNPROW_DTYPE))[:cnt].tobytes() == wrows.tobytes()
    assert (_down(P, ctx, d_kp, np.zeros(cap, np.int32))[:cnt] == wkp).all()
    d_res, d_best, d_fl = _dev(ctx, np.zeros(1, P.PNPRESULT_DTYPE)), _dev(ctx, np.zeros(cap, np.uint8)), _dev(ctx, np.zeros(cap, np.uint8))
    S = pc.Solver(wrows, camd, seed0, **pc.RELOC)
    for _ in range(70):
        P.PnPsolver.SolveDevice(1, d_rows, d_n, cap, cam, seed0, 5, d_res, d_best, d_res, d_fl, ctx=ctx)
        ctx.synchronize()
        res = _down(P, ctx, d_res, np.zeros(1, P.PNPRESULT_DTYPE))[0]
        fl = _down(P, ctx, d_fl, np.zeros(cap, np.uint8))[:cnt]
        wres, wfl = S.iterate(5)
        assert pc.same_result(res, wres) and (fl == wfl).all()
        if res["status"] != 0:
            break
    assert res["status"] == 1 and res["inliers"] > 50 and 0 < (fl == 0).sum()
    Rt, tt = Ttrue["R"].astype(np.float64).reshape(3, 3), Ttrue["t"].astype(np.float64)
    assert np.abs(res["Tcw"]["R"].reshape(3, 3) - Rt).max() < 5e-3 and np.abs(res["Tcw"]["t"] - tt).max() < 2e-2
    # 3. the inliers mask the matches (:2119-2128); 4. PoseOptimization(&mCurrentFrame) (:2130)
    d_idx2 = _dev(ctx, np.full((1, cap), -9, np.int32))
    P.PnPsolver.MapPointIndexFromInliersDevice(1, d_idx, d_kp, d_fl, d_n, cap, cap, d_idx2, ctx=ctx)
    d_e, d_ekp, d_ne = _dev(ctx, np.zeros(cap, P.POSEEDGE_DTYPE)), _dev(ctx, np.zeros(cap, np.int32)), _dev(ctx, np.zeros(1, np.int32))
    d_T, d_o, d_g = _dev(ctx, np.zeros(1, P.POSE_DTYPE)), _dev(ctx, np.zeros(cap, np.uint8)), _dev(ctx, np.zeros(1, np.int32))
    P.Optimizer.EdgesFromMatchesDevice(g, 0, 1, d_idx2, d_mp, n, ks.INV_SIGMA2, d_e, d_ekp, d_ne, cap)
    d_Tcw = d_res + P.PNPRESULT_DTYPE.fields["Tcw"][1]                  # &d_res[0].Tcw
    P.Optimizer.PoseOptimizationDevice(1, d_Tcw, d_e, d_ne, cap, cam, d_T, d_o, d_g, ctx=ctx)
    ctx.synchronize()
    masked = np.full(cap, -1, np.int32)
    masked[wkp[fl == 1]] = mp_index[0, wkp[fl == 1]]
    assert (_down(P, ctx, d_idx2, np.zeros((1, cap), np.int32))[0] == masked).all()
    edges, ekp = _gather(kps, uright, masked[:n], mpK, ks.INV_SIGMA2)
    ne = int(_down(P, ctx, d_ne, np.zeros(1, np.int32))[0])
    assert ne == len(edges) == res["inliers"] and _down(P, ctx, d_e, np.zeros(cap, P.POSEEDGE_DTYPE))[:ne].tobytes() == edges.tobytes()
    ngood, pose, outlier = P.Optimizer.PoseOptimization(res["Tcw"], edges, cam, ctx=ctx)
    got_T, got_g = _down(P, ctx, d_T, np.zeros(1, P.POSE_DTYPE))[0], int(_down(P, ctx, d_g, np.zeros(1, np.int32))[0])
    assert got_g == ngood >= 50 and got_T.tobytes() == pose.tobytes() and (_down(P, ctx, d_o, np.zeros(cap, np.uint8))[:ne] == outlier).all()
    ref = po.optimize(res["Tcw"], edges, po.camera())
    assert ref[2] == ngood and ref[0].tobytes() == pose.tobytes()
    assert np.abs(got_T["R"].reshape(3, 3) - Rt).max() < 2e-3 and np.abs(got_T["t"] - tt).max() < 1e-2
    for d in (d_idx, d_mp, d_rows, d_kp, d_n, d_res, d_best, d_fl, d_idx2, d_e, d_ekp, d_ne, d_T, d_o, d_g):
        ctx.device_free(d)
