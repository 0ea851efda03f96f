"""CreateNewMapPoints / CreateNewMapLines2 on the device (psl-slam_amd/csrc/pslfe_kf.hip: k_new_points_choice, k_new_points_finish;
pslfe_kf_line.hip: k_new_lines_walk, k_new_lines_list) against the numpy restatement of tests/new_points_cases.py, bit for bit in every
output array and count, statuses included: the host-array form, the device form with its chain into the normal / depth refresh, the
LocalMapping helper and the compiled consumer tools/dropin/newpoints_main.cpp (whose one-core loop is the same header compiled for the
host).  tests/test_new_points_cpu.py shows without a GPU what the cases reach."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import new_points_cases as nc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = (0.0, 0.0, 1024.0, 768.0)
_ref = {}


def ref_points(c):
    if c["name"] not in _ref:
        _ref[c["name"]] = nc.create_points(c)
    return _ref[c["name"]]


def store(P, c):
    """the frame store with neighbour k in slot k"""
    K = len(c["nb"])
    g = P.FrameGrid(max(1, max([len(s["kps"]) for s in c["store"]] + [1])), max(K, 1))
    for k, s in enumerate(c["store"]):
        g.set(k, s["kps"], s["desc"], BOUNDS, s["uright"])
    return g


def run_points(P, c, matcher=None, grid=None):
    cur = c["cur"]
    kf = matcher or P.KeyFrameMatcher()
    return kf.CreateNewMapPoints(grid or store(P, c), c["kf1"], cur["keysun"], cur["keys"], cur["uright"], cur["depth"], cur["taken"], c["nb"],
                                 [n["fidx"] for n in c["neigh"]], [n["taken"] for n in c["neigh"]], [n["keys"] for n in c["neigh"]],
                                 [n["depth"] for n in c["neigh"]], c["q"], c["idx1"], c["qd"], c["sf"], c["sig2"], c["only_stereo"], c["check_ori"])


def hold_points(got, c):
    ref = ref_points(c)
    nc.assert_same_points(got, ref, c["name"])
    assert len(got["geom"]) == len(ref["new"])
    for f in ("x", "y", "z"):
        assert got["geom"][f].tobytes() == ref["new"][f].tobytes()
    for f in ("nx", "ny", "nz", "min_dist", "max_dist"):
        assert not got["geom"][f].any()


@pytest.mark.parametrize("make", [nc.gates_case, nc.degenerate_case, lambda: nc.order_case(2), lambda: nc.order_case(3), nc.general_case,
                                  lambda: nc.general_case(7, 40, 4, inactive=(1,))],
                         ids=["gates", "degenerate", "order-K2", "order-K3", "general", "general-inactive-middle"])
def test_host_form_equals_restatement(make):
    """one pair per branch and gate (the NaN pose row, the mbf of the current keyframe in pKF2's right-image term, UnprojectStereo with
    z <= 0, x3D[3] == 0 among them); the dependence between neighbours with the rotation check on (fails if taken1 is applied behind
    the histogram: tests/test_new_points_cpu.py shows that the two orders differ on this case); an inactive neighbour in the middle"""
    import psl_slam_amd as P
    c = make()
    hold_points(run_points(P, c), c)


@pytest.mark.parametrize("nq,n1", [(0, None), (1, None), (63, None), (64, None), (65, None), (1023, None), (1024, None), (1025, None), (1030, 4096)])
def test_query_counts_at_the_trips_of_the_finish_stage(nq, n1):
    """nq around a wave and around the 256 threads x 4 of a trip; N1 at PSL_QMAX"""
    import psl_slam_amd as P
    c = nc.count_case(nq, n1)
    got = run_points(P, c)
    hold_points(got, c)
    assert len(got["new"]) == sum(1 for i in range(nq) if i % 5 != 4)


def test_one_neighbour_equals_the_search_followed_by_the_host_loop():
    """K = 1: match and nmatches are pslfe_kf_search_for_triangulation's on the same inputs"""
    import psl_slam_amd as P
    c = nc.general_case(9, 50, 1)
    g, kf = store(P, c), P.KeyFrameMatcher()
    got = run_points(P, c, kf, g)
    nb, n = c["nb"][0], c["neigh"][0]
    nm, match = kf.SearchForTriangulation(g, 0, n["fidx"], n["taken"], c["q"][0], c["qd"][0], nb["F12"], (nb["ex"], nb["ey"]), c["sf"], c["sig2"], False,
                                          c["check_ori"])
    assert nm == got["nmatches"][0] > 10 and np.array_equal(match, got["match"][0])
    hold_points(got, c)


def test_no_neighbour_and_refused_arguments_leave_the_outputs_alone():
    import psl_slam_amd as P
    c = nc.order_case(2)
    g, kf = store(P, c), P.KeyFrameMatcher()
    empty = dict(c, nb=c["nb"][:0], store=[], neigh=[], q=[], idx1=[], qd=[])
    r = run_points(P, empty, kf, g)
    assert len(r["new"]) == 0 and (r["created_by"] == -1).all() and r["match"].shape == (0, 0)
    a = kf._new_points_args(c["kf1"], c["cur"]["keysun"], c["cur"]["keys"], c["cur"]["uright"], c["cur"]["depth"], c["cur"]["taken"], c["nb"],
                            [n["fidx"] for n in c["neigh"]], [n["taken"] for n in c["neigh"]], [n["keys"] for n in c["neigh"]],
                            [n["depth"] for n in c["neigh"]], c["q"], c["idx1"], c["qd"], c["sf"], c["sig2"])
    K, N1, nqmax = a["K"], a["N1"], a["nqmax"]
    out = {k: np.full(n, 77, t) for k, n, t in (("match", K * nqmax, np.int32), ("status", K * nqmax, np.int32), ("x3d", K * nqmax * 3, np.float32),
                                                 ("nm", K, np.int32), ("by", N1, np.int32), ("new", N1 * 6, np.int32), ("nnew", 1, np.int32))}

    def call(**kw):
        b = dict(a, **kw)
        return P.lib().pslfe_kf_create_new_map_points(
            kf._h, g._h, P._ptr(b["kf1"]), C.c_int(b["N1"]), P._ptr(b["ku1"]), P._ptr(b["k1"]), P._ptr(b["ur1"]), P._ptr(b["dp1"]), P._ptr(b["tk1"]),
            P._ptr(b["nb"]), C.c_int(K), P._ptr(b["fidx"]), P._ptr(b["foff"]), P._ptr(b["tk2"]), P._ptr(b["k2"]), P._ptr(b["dp2"]), P._ptr(b["koff"]),
            P._ptr(b["q"]), P._ptr(b["i1"]), P._ptr(b["qd"]), P._ptr(b["nq"]), C.c_int(nqmax), C.c_int(0), C.c_int(1), P._ptr(b["sf"]), P._ptr(b["s2"]),
            C.c_int(b.get("nlevels", len(b["sf"]))), P._ptr(out["match"]), P._ptr(out["status"]), P._ptr(out["x3d"]), P._ptr(out["nm"]), P._ptr(out["by"]),
            P._ptr(out["new"]), P._ptr(out["nnew"]), None)
    bad_slot, dup, far, desc = a["nb"].copy(), a["i1"].copy(), a["i1"].copy(), a["foff"].copy()
    bad_slot["slot"][1] = 5
    dup[0, 1] = dup[0, 0]
    far[1, 0] = N1
    desc[1] = desc[2] + 1
    assert call(nlevels=0) == -1 and call(nlevels=17) == -1 and call(nb=bad_slot) == -1 and call(i1=dup) == -1 and call(i1=far) == -1
    assert call(foff=desc) == -1 and call(nq=np.array([nqmax + 1, 0], np.int32)) == -1 and call(ku1=None) == -1
    g2 = P.FrameGrid(64, 4)                               # a store whose slot 1 was never set
    g2.set(0, c["store"][0]["kps"], c["store"][0]["desc"], BOUNDS, c["store"][0]["uright"])
    g, g2 = g2, g
    assert call() == -5
    g, g2 = g2, g
    assert all((v.view(np.int32) == (77 if v.dtype == np.int32 else np.float32(77).view(np.int32))).all() for v in out.values())
    inactive = a["nb"].copy()                             # the slot of a neighbour that failed the baseline gate is never looked at
    inactive["active"][1], inactive["slot"][1] = 0, 99
    assert call(nb=inactive) == 0 and out["nm"][1] == 0 and (out["status"].reshape(K, nqmax)[1, :a["nq"][1]] == nc.ST["INACTIVE"]).all()
    assert (out["new"].reshape(N1, 6)[out["nnew"][0]:] == 0).all()      # the rows behind the list come back as zeros
    hold_points(run_points(P, c, kf, g), c)               # the handle is fine afterwards


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def test_device_form_and_the_chain_into_the_refresh(ctx):
    """the device form writes the same arrays, and its rows go through pslfe_kf_update_normal_and_depth_device with M = N1 where they
    are: equal to the host refresh fed the same rows and runs"""
    import psl_slam_amd as P
    c = nc.general_case()
    ref = ref_points(c)
    g, kf = store(P, c), P.KeyFrameMatcher()
    a = kf._new_points_args(c["kf1"], c["cur"]["keysun"], c["cur"]["keys"], c["cur"]["uright"], c["cur"]["depth"], c["cur"]["taken"], c["nb"],
                            [n["fidx"] for n in c["neigh"]], [n["taken"] for n in c["neigh"]], [n["keys"] for n in c["neigh"]],
                            [n["depth"] for n in c["neigh"]], c["q"], c["idx1"], c["qd"], c["sf"], c["sig2"])
    K, N1, nqmax = a["K"], a["N1"], a["nqmax"]
    ins = [_dev(ctx, a[k]) for k in ("ku1", "k1", "ur1", "dp1", "tk1", "fidx", "tk2", "k2", "dp2", "q", "i1", "qd")]
    host = {"match": np.full((K, nqmax), 9, np.int32), "status": np.full((K, nqmax), 9, np.int32), "x3d": np.full((K, nqmax, 3), 9, np.float32),
            "nmatches": np.full(K, 9, np.int32), "created_by": np.full(N1, 9, np.int32), "new": np.zeros(N1, P.NEWMAPPOINT_DTYPE),
            "nnew": np.full(1, 9, np.int32), "geom": np.full(N1, 9, P.MAPPOINT_DTYPE), "obs_off": np.full(N1 + 1, 9, np.int32),
            "obs_kf": np.full(2 * N1, 9, np.int32), "ref_kf": np.full(N1, 9, np.int32), "ref_level": np.full(N1, 9, np.int32)}
    names = ("match", "status", "x3d", "nmatches", "created_by", "new", "nnew", "geom", "obs_off", "obs_kf", "ref_kf", "ref_level")
    d = {k: _dev(ctx, host[k]) for k in names}
    kf.CreateNewMapPointsDevice(g, c["kf1"], N1, *ins[:5], c["nb"], ins[5], a["foff"], ins[6], ins[7], ins[8], a["koff"], ins[9], ins[10], ins[11], a["nq"],
                                nqmax, c["sf"], c["sig2"], *[d[k] for k in names], False, c["check_ori"])
    centres = np.random.default_rng(1).uniform(-1, 1, (K + 1, 3)).astype(np.float32)
    d_c = _dev(ctx, centres)
    got = {k: _down(P, ctx, d[k], host[k].copy()) for k in names}
    kf.update_normal_and_depth_device(d["geom"], N1, d["obs_off"], d["obs_kf"], d_c, K + 1, d["ref_kf"], d["ref_level"], 0, c["sf"])
    refreshed = _down(P, ctx, d["geom"], host["geom"].copy())
    ctx.synchronize()
    n = int(got["nnew"][0])
    got["new"] = got["new"][:n]
    nc.assert_same_points(got, ref, "device form")
    off, okf, rk, rl = nc.observation_runs(c, ref, N1, c["cur"]["keysun"]["octave"])
    assert np.array_equal(got["obs_off"], off) and np.array_equal(got["obs_kf"][:2 * n], okf) and np.array_equal(got["ref_kf"][:n], rk)
    assert np.array_equal(got["ref_level"][:n], rl) and n == len(ref["new"]) > 10
    assert any(nb["kf_first"] for nb in c["nb"][ref["new"]["k"]])         # both observation orders occur
    want = kf.UpdateNormalAndDepth(got["geom"][:n], off[:n + 1], okf, centres, rk, rl, c["sf"])
    assert refreshed[:n].tobytes() == want.tobytes() and want["max_dist"].all()
    assert refreshed[n:].tobytes() == host["geom"][n:].tobytes()         # the rows behind the list keep every byte
    for p in ins + list(d.values()) + [d_c]:
        ctx.device_free(p)


def test_local_mapping_helper_on_the_device():
    import psl_slam_amd as P
    from test_new_points_cpu import helper_inputs, literal_loop
    c = nc.general_case()
    cur, neigh = helper_inputs(c)
    r, created = P.LocalMapping.CreateNewMapPoints(P.KeyFrameMatcher(), store(P, c), c["kf1"], cur, c["nb"], neigh, c["sf"], c["sig2"], checkOri=True)
    want = literal_loop(c)
    assert len(created) == len(want) > 10
    for g, w in zip(created, want):
        assert g[:3] == w[:3] and g[3].tobytes() == w[3].tobytes()


# ---- lines ------------------------------------------------------------------------------------------------------------------------------
def run_lines(P, c, kf=None, **kw):
    cur = c["cur"]
    return (kf or P.KeyFrameMatcher()).CreateNewMapLines(c["kf1"], cur["ldesc"], cur["has_mapline"], cur["keylines"], cur["lines3d"], cur["lineeq"], c["nb"],
                                                         [n["ldesc"] for n in c["neigh"]], [n["has_mapline"] for n in c["neigh"]],
                                                         [n["keylines"] for n in c["neigh"]], [n["lines3d"] for n in c["neigh"]], c["sf"], c["sig2"], **kw)


def test_lines_every_gate_the_taken_chain_and_the_kept_oddities():
    """each gate; bStereo2 read from KF1's table (idx2 < NL1, either answer); idx2 >= NL1; the taken chain over three neighbours; an empty
    and an inactive neighbour.  The search inside is the library's own: its rows are what the construction says"""
    import psl_slam_amd as P
    c = nc.line_gates_case()
    kf = P.KeyFrameMatcher()
    cur = c["cur"]
    nm0, match0 = kf.LineSearchForTriangulationKeyFrames(cur["ldesc"], [n["ldesc"] for n in c["neigh"]], cur["has_mapline"],
                                                         [n["has_mapline"] for n in c["neigh"]], 0.95, 50, True)
    assert np.array_equal(match0, c["match0"])
    ref = nc.create_lines(c, match0)
    got = run_lines(P, c, kf)
    nc.assert_same_lines(got, ref, c["name"])
    n = len(ref["new"])
    assert n == 3 and got["geom"]["sp"].astype(np.float32).tobytes() == ref["new"]["sp"].tobytes() and not got["geom"]["normal"].any()
    assert set(ref["status"].reshape(-1).tolist()) == set(nc.STL.values())


def test_lines_device_form_and_the_chain_into_update_average_dir(ctx):
    import psl_slam_amd as P
    c = nc.line_gates_case()
    ref = nc.create_lines(c, c["match0"])
    kf = P.KeyFrameMatcher()
    a = kf._new_lines_args(c["kf1"], c["cur"]["ldesc"], c["cur"]["has_mapline"], c["cur"]["keylines"], c["cur"]["lines3d"], c["cur"]["lineeq"], c["nb"],
                           [n["ldesc"] for n in c["neigh"]], [n["has_mapline"] for n in c["neigh"]], [n["keylines"] for n in c["neigh"]],
                           [n["lines3d"] for n in c["neigh"]], c["sf"], c["sig2"])
    K, n1 = a["K"], a["n1"]
    ins = {k: _dev(ctx, a[k]) for k in ("d1", "h1", "kl1", "l1", "eq1", "d2", "h2", "kl2", "l2")}
    host = {"match": np.full((K, n1), 9, np.int32), "status": np.full((K, n1), 9, np.int32), "sp": np.full((K, n1, 3), 9, np.float32),
            "ep": np.full((K, n1, 3), 9, np.float32), "nmatches": np.full(K, 9, np.int32), "created_by": np.full(n1, 9, np.int32),
            "new": np.zeros(n1, P.NEWMAPLINE_DTYPE), "nnew": np.full(1, 9, np.int32), "geom": np.zeros(n1, P.MAPLINE_DTYPE),
            "obs_off": np.full(n1 + 1, 9, np.int32), "obs_kf": np.full(2 * n1, 9, np.int32), "ref_kf": np.full(n1, 9, np.int32),
            "ref_level": np.full(n1, 9, np.int32)}
    host["geom"]["min_dist"] = 9
    names = tuple(host)
    d = {k: _dev(ctx, host[k]) for k in names}
    kf.CreateNewMapLinesDevice(c["kf1"], n1, ins["d1"], ins["h1"], ins["kl1"], ins["l1"], ins["eq1"], c["nb"], ins["d2"], a["off"], ins["h2"], ins["kl2"],
                               ins["l2"], c["sf"], c["sig2"], *[d[k] for k in names])
    centres = np.random.default_rng(2).uniform(-1, 1, (K + 1, 3)).astype(np.float32)
    d_c = _dev(ctx, centres)
    got = {k: _down(P, ctx, d[k], host[k].copy()) for k in names}
    kf.line_update_average_dir_device(d["geom"], n1, d["obs_off"], d["obs_kf"], d_c, K + 1, d["ref_kf"], d["ref_level"], 0, c["sf"])
    refreshed = _down(P, ctx, d["geom"], host["geom"].copy())
    ctx.synchronize()
    n = int(got["nnew"][0])
    got["new"] = got["new"][:n]
    nc.assert_same_lines(got, ref, "device form")
    off, okf, rk, rl = nc.observation_runs(c, ref, n1, c["cur"]["keylines"]["octave"])
    assert np.array_equal(got["obs_off"], off) and np.array_equal(got["obs_kf"][:2 * n], okf) and np.array_equal(got["ref_kf"][:n], rk)
    assert np.array_equal(got["ref_level"][:n], rl) and n == 3 and c["nb"][1]["kf_first"] and 1 in ref["new"]["k"]
    want = kf.LineUpdateAverageDir(got["geom"][:n], off[:n + 1], okf, centres, rk, rl, c["sf"])
    assert refreshed[:n].tobytes() == want.tobytes() and want["max_dist"].all()
    assert refreshed[n:].tobytes() == host["geom"][n:].tobytes()
    for p in list(ins.values()) + list(d.values()) + [d_c]:
        ctx.device_free(p)


def test_lines_without_lines_without_neighbours_and_refused():
    import psl_slam_amd as P
    c = nc.line_gates_case()
    kf = P.KeyFrameMatcher()
    none = dict(c, cur={k: v[:0] for k, v in c["cur"].items()})
    r = run_lines(P, none, kf)
    assert len(r["new"]) == 0 and not r["nmatches"].any() and r["match"].shape == (len(c["nb"]), 0)
    alone = dict(c, nb=c["nb"][:0], neigh=[])
    r = run_lines(P, alone, kf)
    assert len(r["new"]) == 0 and (r["created_by"] == -1).all()
    with pytest.raises(P.PslfeError, match="levels"):
        run_lines(P, dict(c, sf=np.ones(17, np.float32), sig2=np.ones(17, np.float32)), kf)
    # refused calls leave every output as it was
    a = kf._new_lines_args(c["kf1"], c["cur"]["ldesc"], c["cur"]["has_mapline"], c["cur"]["keylines"], c["cur"]["lines3d"], c["cur"]["lineeq"], c["nb"],
                           [n["ldesc"] for n in c["neigh"]], [n["has_mapline"] for n in c["neigh"]], [n["keylines"] for n in c["neigh"]],
                           [n["lines3d"] for n in c["neigh"]], c["sf"], c["sig2"])
    K, n1 = a["K"], a["n1"]
    out = [np.full(n, 77, np.int32) for n in (K * n1, K * n1, K * n1 * 3, K * n1 * 3, K, n1, n1 * 9, 1)]

    def call(K_=K, n1_=n1, nlevels=len(a["sf"]), **kw):
        b = dict(a, **kw)
        return P.lib().pslfe_kf_create_new_map_lines(
            kf._h, P._ptr(b["kf1"]), C.c_int(n1_), P._ptr(b["d1"]), P._ptr(b["h1"]), P._ptr(b["kl1"]), P._ptr(b["l1"]), P._ptr(b["eq1"]), P._ptr(b["nb"]),
            C.c_int(K_), P._ptr(b["d2"]), P._ptr(b["off"]), P._ptr(b["h2"]), P._ptr(b["kl2"]), P._ptr(b["l2"]), C.c_float(0.95), C.c_float(50), C.c_int(1),
            P._ptr(b["sf"]), P._ptr(b["s2"]), C.c_int(nlevels), *[P._ptr(o) for o in out], None)
    desc = a["off"].copy()
    desc[2] = desc[1] - 1
    assert call(nlevels=0) == -1 and call(nlevels=17) == -1 and call(K_=33) == -1 and call(n1_=65536) == -1 and call(off=desc) == -1
    assert call(kl1=None) == -1 and call(l2=None) == -1 and call(eq1=None) == -1 and call(nb=None) == -1 and call(d1=None) == -1
    assert all((o == 77).all() for o in out)
    nc.assert_same_lines(run_lines(P, c, kf), nc.create_lines(c, c["match0"]), "after a refusal")


def test_compiled_consumer(tmp_path):
    """tools/dropin/newpoints_main.cpp linked against the library: its one-core loop and the host-array form through pslfe.hpp, points
    and lines, against the restatement"""
    exe = str(tmp_path / "newpoints_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-o", exe,
                    os.path.join(ROOT, "tools", "dropin", "newpoints_main.cpp"), "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe",
                    "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")], check=True, capture_output=True)
    for c in (nc.gates_case(), nc.order_case(3), nc.general_case()):
        path, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        nc.write_point_case(path, c)
        p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        with open(out, "rb") as f:
            for form in ("loop", "host"):
                nc.assert_same_points(nc.read_point_section(f, c), ref_points(c), (c["name"], form))
    c = nc.line_gates_case()
    path, out = str(tmp_path / "lines.bin"), str(tmp_path / "lines_out.bin")
    nc.write_line_case(path, c)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    ref = nc.create_lines(c, c["match0"])
    with open(out, "rb") as f:
        for form in ("loop", "host"):
            nc.assert_same_lines(nc.read_line_section(f, c), ref, form)
