"""The restatement of Optimizer::OptimizeEssentialGraph (tests/essential_cases.py) and the stand-alone host program of
tools/dropin/essential_main.cpp (the shared header psl-slam_amd/csrc/essential_kernels.h compiled for the host with g++, under the address
and undefined-behaviour sanitizers), bit for bit with each other; psl_acos against the host's libm; log against exp; the envelope LDLt
against a dense one and against numpy; the numeric Jacobian against wider differences; the behaviour on a ring with planted drift;
the mirrors' edge builder; the ABI.  No GPU.

psl_acos against libm's acos (test_acos_against_libm): a grid over [-1, 1], 20001 even steps, the 2000 doubles next to each of -1, -0.5,
0, 0.5 and 1 on both sides, geometric steps towards 0 and towards +-1 (1 - 2^-k), and the values just outside [-1, 1].  Measured
here over 36243 arguments: the largest distance is ACOS_ULPS = 1 ulp (4.0 % of the grid differs by one, none by more); both give NaN outside and the
same doubles at +-1 and 0.  Gate: 2 ulps.

log(exp(x)) against x (test_log_of_exp_round_trip): 400 random x per branch, |upsilon| <= 2; |omega| from 1e-7 to 3e-6 or from 1e-2
to 2.8, |sigma| from 1e-7 to 3e-6 or from 0.05 to 0.7, so that exp and log take the SAME branch k = (|sigma| >= 1e-5) * 2 + (angle
large): exp switches at theta = 1e-5 and log at d = 1 - 1e-5 (theta = 4.5e-3), and between the two log's small-angle series is cut at
theta^3 / 6 <= 1.5e-8.  Deviation = the largest |log(exp(x)) - x| over max(1, |x|_inf).  Measured here, worst per branch:
LOG_EXP_WORST = {0: 4.02e-16, 1: 8.75e-15, 2: 1.08e-15, 3: 4.47e-15}.  Gate: four times each.
Branch 2 (small angle, |sigma| >= 1e-5) holds only because exp and log share the reference's B = ((sigma^2 / 2 - sigma + 1) s) /
sigma^3, which lacks the "- 1" of the series it stands for and grows like 1 / sigma^3: it multiplies Omega^2, so it cancels in the
round trip and is harmless only while theta^2 / sigma^3 is small.  Restated as it is (sim3.h:117-119, :199).

The envelope step against numpy (test_linear_step_against_numpy): (H + lambda I) x = b of the first iteration with lambda = 1e-16 is
solved by numpy.linalg.solve on the dense matrix; bound |x - x_np| / |x_np| <= k cond2 2^-52.  Measured here over LINEAR_GRAPHS:
chain5 rel 1.07e-15, cond2 21.6, ratio 0.224; chain5_loop 3.65e-16, 11.6, 0.142; two_long_rows 1.01e-15, 19.5, 0.232; the largest
ratio is LINEAR_RATIO = 0.232, so k = 4 x 0.232 = 0.928.

The numeric Jacobian (test_numeric_jacobian_against_wider_differences): the delta = 1e-9 differences of the restatement against
differences of step 1e-4 of the same error, on the two edges of `branches` whose error has a rotation of 0.4 .. 0.7 rad and a scale of
0.8 (the closed-form branch); deviation = largest |J - J_w| over largest |J| of the half.  Measured here: JACOBIAN_WORST = 3.54e-7
(the 1e-9 step leaves about 1e-7 of rounding noise); the sanity bound is four times that.

Behaviour (test_ring_with_planted_drift), reported and gated only in direction: ring12 chi2 0.0516 -> 0.00418, largest error of a
keyframe position against the ground truth 0.0991 -> 0.0789; ring12_fix_scale chi2 0.0464 -> 0.00392, 0.103 -> 0.0829, every scale 1.0
to the bit.  (A single loop edge of information I7 against a chain of eleven odometry edges and ten second-neighbour edges: the
corrected keyframes are pulled back by about a third of the closure error, so the gain is modest on so short a ring.)"""
import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import essential_cases as ec
from essential_cases import s3_exp, s3_oplus
from sim3_opt_cases import s3_inverse, s3_mul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACOS_ULPS = 1
LOG_EXP_WORST = {0: 4.02e-16, 1: 8.75e-15, 2: 1.08e-15, 3: 4.47e-15}
LINEAR_GRAPHS = ("chain5", "chain5_loop", "two_long_rows")
LINEAR_RATIO, LINEAR_K = 0.232, 4 * 0.232
JACOBIAN_WORST = 3.54e-7


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the header's host form as a stand-alone program, built once with g++ alone under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("essential") / "essential_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DPSL_EG_HOST_ONLY", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "essential_main.cpp")],
                   check=True, capture_output=True)
    return exe


def _math(host_exe, tmp_path, xs, sims):
    path, out = str(tmp_path / "math.bin"), str(tmp_path / "math_out.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<2i", len(xs), len(sims)))
        f.write(np.asarray(xs, np.float64).tobytes())
        f.write(np.asarray([ec.store(S) for S in sims], np.float64).tobytes())
    p = subprocess.run([host_exe, "--math", path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    o = np.fromfile(out, np.float64)
    return o[:len(xs)], o[len(xs):].reshape(len(sims), 8)


def _ulps(a, b):
    ia, ib = np.asarray(a, np.float64).view(np.int64), np.asarray(b, np.float64).view(np.int64)
    return np.abs(ia - ib)


def _acos_grid():
    g = [np.linspace(-1.0, 1.0, 20001)]
    for c in (-1.0, -0.5, 0.0, 0.5, 1.0):
        for direction in (-2.0, 2.0):
            x, row = c, []
            for _ in range(2000):
                x = float(np.nextafter(x, direction))
                row.append(x)
            g.append(np.array(row))
    k = np.arange(1, 60, dtype=np.float64)
    g += [2.0 ** -k, -(2.0 ** -k), 1.0 - 2.0 ** -k, -(1.0 - 2.0 ** -k), np.array([-1.0, -0.5, 0.0, -0.0, 0.5, 1.0, 1.5, -1.5, 1e300, np.nan])]
    return np.concatenate(g)


def test_acos_against_libm(host_exe, tmp_path):
    """the header's psl_acos on the host == the restatement's fdlibm_acos bit for bit; against libm at most ACOS_ULPS (module docstring)"""
    x = _acos_grid()
    got, _ = _math(host_exe, tmp_path, x, [])
    mine = np.array([ec.fdlibm_acos(float(v)) for v in x])
    assert got.tobytes() == mine.tobytes()
    inside = np.abs(x) <= 1.0
    assert np.isnan(got[~inside]).all() and not np.isnan(got[inside]).any()
    ref = np.arccos(x[inside])
    d = _ulps(got[inside], ref)
    print(f"psl_acos against libm: {len(ref)} arguments, largest distance {int(d.max())} ulp, {float((d > 0).mean()):.3%} differ")
    assert int(d.max()) <= 2 * ACOS_ULPS
    for v in (-1.0, 0.0, 1.0):
        assert ec.fdlibm_acos(v) == math.acos(v)


def _updates(rng, n, big_theta, big_sigma):
    out = []
    for _ in range(n):
        w = rng.normal(size=3)
        w *= (10.0 ** rng.uniform(-2, 0.45) if big_theta else 10.0 ** rng.uniform(-7, -5.5)) / np.linalg.norm(w)
        s = (rng.uniform(0.05, 0.7) if big_sigma else 10.0 ** rng.uniform(-7, -5.5)) * rng.choice([-1.0, 1.0])
        out.append([float(v) for v in w] + [float(v) for v in rng.uniform(-2, 2, 3)] + [float(s)])
    return out


def test_log_of_exp_round_trip(host_exe, tmp_path):
    """all four branches of log and of exp; log of the identity is exactly zero; the header's log on the host == the restatement's"""
    rng = np.random.RandomState(11)
    worst, seen_log, seen_exp, sims = {}, set(), set(), []
    for big_theta in (0, 1):
        for big_sigma in (0, 1):
            worst[2 * big_sigma + big_theta] = 0.0
            extra = {(0, 1): [[0.0] * 6 + [0.3]], (1, 0): [[0.2, 0.0, 0.0, 1.0, 2.0, 3.0, 0.0]]}.get((big_theta, big_sigma), [])
            for x in _updates(rng, 400, big_theta, big_sigma) + extra:
                S, be = s3_exp(x)
                y, bl = ec.s3_log(S)
                seen_exp.add(be)
                seen_log.add(bl)
                sims.append(S)
                dev = max(abs(a - b) for a, b in zip(x, y)) / max(1.0, max(abs(v) for v in x))
                assert be == bl == 2 * big_sigma + big_theta
                worst[bl] = max(worst[bl], dev)
    print("log(exp(x)) - x, worst per branch:", {k: f"{v:.3g}" for k, v in worst.items()}, "recorded", LOG_EXP_WORST)
    assert all(worst[k] <= 4 * LOG_EXP_WORST[k] for k in worst)
    assert seen_log == {0, 1, 2, 3} and seen_exp == {0, 1, 2, 3}
    ident = ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], 1.0)
    y, b = ec.s3_log(ident)
    assert b == 0 and all(v == 0.0 for v in y)
    _, got = _math(host_exe, tmp_path, [], sims + [ident])
    want = np.array([list(ec.s3_log(S)[0]) + [float(ec.s3_log(S)[1])] for S in sims + [ident]])
    assert got.tobytes() == want.tobytes()


def test_log_keeps_the_nan_of_acos():
    """d < -1 by rounding: omega and upsilon are NaN, sigma is not, and the driver rejects such a trial"""
    q = [1.0 + 1e-9, 0.0, 0.0, 0.0]              # a half turn whose unnormalised quaternion pushes d below -1
    y, b = ec.s3_log((q, [0.1, 0.2, 0.3], 1.0))
    assert b == 1 and all(v != v for v in y[:6]) and y[6] == 0.0


def _first(name):
    c = ec.case("chain5_loop") if name == "chain5" else ec.case(name)
    edges = c["edges"][c["edges"]["loop"] == 0] if name == "chain5" else c["edges"]
    g = ec.Graph(c["kf"], edges, c["mp"], c["mp_ref"], c["fix_scale"])
    assert g.check() == 0
    g.measure()
    g.linearize()
    g.build()
    return g


def test_linear_step_against_numpy():
    worst, bad = 0.0, False
    for name in LINEAR_GRAPHS:
        g = _first(name)
        x, why = g.solve(ec.LAMBDA_INIT)
        assert why == "ok"
        A = np.array(g.dense(ec.LAMBDA_INIT))
        x_np = np.linalg.solve(A, np.array(g.b))
        rel, cond = float(np.linalg.norm(np.array(x) - x_np) / np.linalg.norm(x_np)), float(np.linalg.cond(A, 2))
        ratio = rel / (cond * 2.0 ** -52)
        print(f"{name}: |x - x_np| / |x_np| = {rel:.3g}, cond2 = {cond:.3g}, ratio = {ratio:.3g}")
        worst = max(worst, ratio)
        bad = bad or not rel <= LINEAR_K * cond * 2.0 ** -52
    print(f"largest ratio {worst:.3g} (recorded {LINEAR_RATIO}, k = {LINEAR_K:.3g})")
    assert not bad


def test_envelope_equals_dense_ldlt():
    """finite input: the envelope LDLt and the dense LDLt of the same arithmetic give the same bytes; the envelopes are what the names say"""
    for name in LINEAR_GRAPHS:
        g = _first(name)
        x, why = g.solve(ec.LAMBDA_INIT)
        xd, L, D = ec.dense_ldlt_solve(g.dense(ec.LAMBDA_INIT), g.b)
        assert struct.pack(f"<{len(x)}d", *x) == struct.pack(f"<{len(xd)}d", *xd), name
        assert struct.pack(f"<{len(D)}d", *D) == struct.pack(f"<{len(D)}d", *g.D), name
        for r, row in enumerate(g.L):
            k0 = 7 * g.fb[r // 7]
            assert all(L[r][k] == 0.0 for k in range(k0)), (name, r)                  # nothing outside the envelope
            assert all(L[r][k0 + k] == row[k] for k in range(r - k0)), (name, r)
    assert _first("chain5").fb == [0, 1, 1, 2] and _first("chain5_loop").fb == [0, 1, 1, 0]      # the loop row spans the matrix
    fb = _first("two_long_rows").fb
    assert fb[-1] == 0 and fb[-2] == 1


def test_numeric_jacobian_against_wider_differences():
    c = ec.case("branches")
    g = ec.Graph(c["kf"], c["edges"], c["mp"], c["mp_ref"], False)
    assert g.check() == 0
    g.measure(), g.linearize()
    h, worst = 1e-4, 0.0
    for e in (3, 6):                             # rotations of 0.4 and 0.7 rad and scales of 0.8 in the error: the closed-form branch
        i, j, C = g.ei[e], g.ej[e], g.meas[e]
        for half, v in ((0, i), (1, j)):
            J = g.J[e][half]
            if J is None:
                assert g.pidx[v] < 0
                continue
            Jw = [0.0] * 49
            for d in range(7):
                u = [0.0] * 7
                u[d] = h
                Sp = s3_oplus(u, False, g.S[v])[0]
                u[d] = -h
                Sm = s3_oplus(u, False, g.S[v])[0]
                if half == 0:
                    ep, em = ec.edge_error(C, Sp, s3_inverse(g.S[j]))[0], ec.edge_error(C, Sm, s3_inverse(g.S[j]))[0]
                else:
                    ep, em = ec.edge_error(C, g.S[i], s3_inverse(Sp))[0], ec.edge_error(C, g.S[i], s3_inverse(Sm))[0]
                for r in range(7):
                    Jw[7 * r + d] = (ep[r] - em[r]) / (2 * h)
            dev = max(abs(a - b) for a, b in zip(J, Jw)) / max(abs(a) for a in J)
            worst = max(worst, dev)
    print(f"numeric Jacobian against step 1e-4: worst {worst:.3g} (recorded {JACOBIAN_WORST})")
    assert worst <= 4 * JACOBIAN_WORST


def _t_error(pose, true):
    """the largest error of a keyframe's position, the translation of Twc = -R^T t, as an absolute trajectory error measures it (the t
    of Tcw would mix in the rotation error times the distance of the world origin, which depends on where that origin is)"""
    worst = 0.0
    for v, T in enumerate(true):
        R, t = pose["R"][v].astype(np.float64).reshape(3, 3), pose["t"][v].astype(np.float64)
        worst = max(worst, float(np.abs(-R.T @ t - np.array(s3_inverse(T)[1])).max()))
    return worst


def test_ring_with_planted_drift():
    """chi2 falls and the largest translation error against the ground truth is smaller at the end; with fix_scale every scale stays 1"""
    for name in ("ring12", "ring12_fix_scale"):
        c = ec.case(name)
        r = c["ref"]
        start = ec.optimize(c["kf"], c["edges"][:0], c["mp"], c["mp_ref"], c["fix_scale"])     # no edge: the poses of the Sim3s as given
        assert int(start["info"]["iterations"]) == 0 and int(r["info"]["iterations"]) >= 1
        e0, e1 = _t_error(start["pose"], c["true"]), _t_error(r["pose"], c["true"])
        print(f"{name}: chi2 {float(r['info']['chi2_start']):.3g} -> {float(r['info']['chi2_end']):.3g}, translation error {e0:.3g} -> {e1:.3g}")
        assert float(r["info"]["chi2_end"]) < float(r["info"]["chi2_start"]) and e1 < e0
        if c["fix_scale"]:
            g = r["graph"]
            assert all(float(row[7]) == 1.0 for row in c["kf"]["Scw"])          # the restatement's inputs have scale 1 ...
            assert any(t[1] for t in g.trials) and int(r["info"]["log_branches"]) & 0b1100 == 0   # ... steps were taken, sigma stayed 0
            assert (r["S"][:, 7] == 1.0).all()
        else:
            assert (r["S"][:, 7] != 1.0).any()


def test_edge_builder():
    """a parent edge, a loop edge kept once, a covisibility edge dropped by sInsertedEdges, a child excluded, and a LoopConnections pair
    under minFeat kept only for (cur, loop)"""
    import psl_slam_amd as P
    parent = [-1, 0, 1, 2, 3]
    loop_edges = [[3], [], [], [0], []]                      # an old loop between rows 3 and 0: created once, at row 3
    covis = [[1, 4], [0, 2], [1, 3, 0], [2, 4], [3, 0, 1, 2]]
    conns = [(4, [(0, 30), (1, 150), (2, 20)]), (0, [(4, 30)])]      # cur = 4, loop = 0
    ed = P.Optimizer.EssentialGraphEdges(parent, loop_edges, covis, conns, loop_kf=0, cur_kf=4)
    rows = [(int(e["i"]), int(e["j"]), int(e["loop"])) for e in ed]
    assert rows == [(4, 0, 1), (4, 1, 1),                    # (4, 0) under minFeat kept for (cur, loop); (4, 2) and (0, 4) dropped
                    (1, 0, 0),
                    (2, 1, 0), (2, 0, 0),                    # the covisible 1 is the parent; 3 is a child; 0 stays
                    (3, 2, 0), (3, 0, 0),                    # the loop edge at its higher row; covisible 4 is a child
                    (4, 3, 0), (4, 2, 0)]                    # covisibles 0 and 1 are in sInsertedEdges; 2 stays
    assert ed.dtype == P.EGEDGE_DTYPE == ec.EDGE_DTYPE
    hpp = open(os.path.join(ROOT, "psl-slam_amd", "host", "pslfe.hpp")).read()
    assert "EssentialGraphEdges" in hpp and "OptimizeEssentialGraphDevice" in hpp


def test_abi_pods_and_error_codes_without_a_device():
    import psl_slam_amd as P
    assert P.EGKEYFRAME_DTYPE == ec.KF_DTYPE and P.EGKEYFRAME_DTYPE.itemsize == 136 and P.EGEDGE_DTYPE.itemsize == 12
    assert P.EGINFO_DTYPE == ec.INFO_DTYPE and P.EGINFO_DTYPE.itemsize == 40 and P.EGINFO_DTYPE.fields["chi2_start"][1] == 16
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslEgKeyFrame) == 136 && sizeof(PslEgEdge) == 12 && sizeof(PslEgInfo) == 40" in hdr
    L = P.lib()
    null = C.c_void_p(None)
    dev = lambda K: L.pslfe_eg_optimize_device(null, C.c_int(K), null, null, null, null, null, null, null, C.c_int(0), null, null, null, null)
    assert dev(0) == 0                                       # K == 0: nothing is done
    assert dev(-1) == -1 and dev(1) == -1
    assert b"pslfe_eg_optimize_device" in L.pslfe_last_error()
    host = lambda nkf, ne, nmp: L.pslfe_eg_optimize(null, null, C.c_int(nkf), null, C.c_int(ne), null, null, C.c_int(nmp), C.c_int(0), null, null,
                                                    null, null)
    assert host(-1, 0, 0) == -1 and host(0, -1, 0) == -1 and host(0, 0, -1) == -1 and host(0, 0, 0) == -1
    assert b"pslfe_eg_optimize" in L.pslfe_last_error()
    out = C.c_void_p()
    assert L.pslfe_eg_create(null, 1, 1, 1, 1, C.c_int64(1), C.byref(out)) == -1 and L.pslfe_eg_create(null, 1, 1, 1, 1, C.c_int64(1), None) == -1
    L.pslfe_eg_destroy.restype = None
    L.pslfe_eg_destroy(null)


def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path):
    """every case and the refused graphs: poses, Sim3s, points, status, iterations, both chi2, lambda and the branch mask"""
    for fs in (False, True):
        group = [ec.case(n) for n in ec.CASE_NAMES if ec.case(n)["fix_scale"] == fs]
        if not fs:
            group += ec.refused_cases()
        path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
        ec.write_cases(path, group, fs)
        p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        for k, (g, c) in enumerate(zip(ec.read_sections(out, group, 1)[0], group)):
            ec.assert_equal_ref(g, c["ref"], (fs, k, c.get("name")))
    small = ec.case("two_long_rows")                         # an envelope above the handle's cap
    caps = (ec.CAPS[0], ec.CAPS[1], ec.CAPS[2], small["ref"]["graph"].env_size - 1)
    ref = ec.optimize(small["kf"], small["edges"], small["mp"], small["mp_ref"], False, caps)
    assert int(ref["info"]["status"]) == ec.E_CAPACITY
    path, out = str(tmp_path / "cap.bin"), str(tmp_path / "cap_out.bin")
    ec.write_cases(path, [small], False, caps)
    p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    ec.assert_equal_ref(ec.read_sections(out, [small], 1)[0][0], ref, "envelope cap")


def test_cases_are_what_their_names_say():
    c = ec.case("two_one_fixed")
    assert len(c["kf"]) == 2 and len(c["edges"]) == 1 and int(c["ref"]["info"]["nfree"]) == 1
    c = ec.case("fixed_in_middle")
    assert list(c["kf"]["fixed"]) == [0, 0, 1, 0, 0] and c["ref"]["S"][2].tobytes() == c["kf"]["Scw"][2].tobytes()
    c = ec.case("free_without_edge")
    assert 3 not in set(c["edges"]["i"]) | set(c["edges"]["j"]) and not c["kf"]["fixed"][3]
    assert c["ref"]["S"][3].tobytes() == np.array(ec.store(s3_mul(s3_exp([0.0] * 7)[0], ec.load(c["kf"]["Scw"][3])))).tobytes()   # a zero step
    assert int(c["ref"]["info"]["status"]) == 0 and int(c["ref"]["info"]["iterations"]) >= 1
    c = ec.case("big_100_300")
    assert len(c["kf"]) == 100 and len(c["edges"]) == 300 and len(c["mp"]) == 300 and 7 * int(c["ref"]["info"]["nfree"]) > 256
    assert int(c["ref"]["info"]["iterations"]) >= 1 and float(c["ref"]["info"]["chi2_end"]) < float(c["ref"]["info"]["chi2_start"])
    c = ec.case("branches")
    assert int(c["ref"]["info"]["log_branches"]) == 15
    first = ec.Graph(c["kf"], c["edges"], c["mp"], c["mp_ref"], False)
    first.check(), first.measure()
    Si = [s3_inverse(s) for s in first.S]
    assert [ec.edge_error(first.meas[e], first.S[0], Si[e + 1])[1] for e in range(4)] == [0, 2, 1, 3]
    for name in ec.CASE_NAMES:
        r = ec.case(name)["ref"]
        assert int(r["info"]["status"]) == 0 and float(r["info"]["chi2_end"]) <= float(r["info"]["chi2_start"]), name
        unchanged = ec.case(name)["mp_ref"] < 0
        assert r["mp"][unchanged].tobytes() == ec.case(name)["mp"][unchanged].tobytes()
