"""CreateNewMapPoints / CreateNewMapLines2 without a GPU: the numpy restatement of tests/new_points_cases.py against the stand-alone host
program of tools/dropin/newpoints_main.cpp (the loops of psl-slam_amd/csrc/triangulate_kernels.h compiled with g++ alone under the
address and undefined-behaviour sanitizers, run as its own process), bit for bit on every case; what the hand-built cases reach; the
restated search against the sequential oracle; the LocalMapping helper against a literal transcription of the reference loop that
rebuilds the queries of every neighbour from the GetMapPoint state of the moment; the ABI and the argument checks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import new_points_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("new_points") / "newpoints_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DPSL_TRI_HOST_ONLY", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tools", "dropin", "newpoints_main.cpp")],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def point_cases():
    cs = [nc.gates_case(), nc.degenerate_case(), nc.order_case(2), nc.order_case(3), nc.general_case(), nc.general_case(7, 40, 4, inactive=(1,)),
          nc.count_case(0), nc.count_case(1), nc.count_case(65)]
    return [(c, nc.create_points(c)) for c in cs]


@pytest.fixture(scope="module")
def line_case():
    c = nc.line_gates_case()
    return c, nc.create_lines(c, c["match0"])


def test_host_program_under_sanitizers_equals_restatement(host_exe, point_cases, line_case, tmp_path):
    for c, ref in point_cases:
        path, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
        nc.write_point_case(path, c)
        p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0 and not p.stderr, (c["name"], p.stderr[-2000:])
        with open(out, "rb") as f:
            nc.assert_same_points(nc.read_point_section(f, c), ref, c["name"])
    c, ref = line_case
    path, out = str(tmp_path / "lines.bin"), str(tmp_path / "lines_out.bin")
    nc.write_line_case(path, c)
    p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    with open(out, "rb") as f:
        nc.assert_same_lines(nc.read_line_section(f, c), ref, c["name"])


def test_every_status_occurs_and_the_general_scene_creates(point_cases, line_case):
    """the coverage condition, on the restatement alone: every status code of both row functions, at least half of the matched pairs of
    the general scene created, and every hand-built pair ends where its construction says"""
    seen = set()
    for c, ref in point_cases:
        for k in range(len(c["nb"])):
            seen |= set(ref["status"][k, :len(c["q"][k])].tolist())
        for (k, i1), want in c["want"].items():
            qi = c["idx1"][k].tolist().index(i1)
            assert nc.status_names(nc.ST, ref["status"][k, qi]) == [want], (c["name"], k, i1)
    assert seen == set(nc.ST.values()), sorted(set(nc.ST.values()) - seen)
    c, ref = next((c, r) for c, r in point_cases if c["name"].startswith("general-s5"))
    matched = int(ref["nmatches"].sum())
    assert matched >= 30 and 2 * len(ref["new"]) >= matched and len(set(ref["new"]["k"].tolist())) >= 2
    assert (ref["status"] == nc.ST["TAKEN"]).any()
    c, ref = line_case
    assert set(ref["status"].reshape(-1).tolist()) == set(nc.STL.values())
    for (k, i1), want in c["want"].items():
        assert nc.status_names(nc.STL, ref["status"][k, i1]) == [want], (k, i1)


def test_hand_built_cases_are_what_their_docstrings_say(point_cases, line_case):
    by = {c["name"]: (c, r) for c, r in point_cases}
    c, r = by["gates"]
    C1 = nc.cam_of(c["kf1"][0])
    cos = []
    for qi in (1, 2):                                          # the 0.9998 edge: the two mono pairs at depth 9.5 and 10.5
        i1, i2 = int(c["idx1"][0][qi]), int(r["match"][0, qi])
        k1, k2 = c["cur"]["keysun"][i1], c["store"][0]["kps"][i2]
        cos.append(float(nc.cos_parallax_rays(C1, nc.cam_of(c["nb"][0]), k1["x"], k1["y"], k2["x"], k2["y"])[0]))
    assert cos[0] < 0.9998 < cos[1] and cos[1] - cos[0] < 5e-5
    assert np.isnan(c["nb"][3]["Tcw"]["R"]).any() and float(c["kf1"][0]["mbf"]) == 50.0
    # both keypoints stereo (neighbour 2): cosParallaxStereo2 stays cosParallaxRays + 1.  Equal cosines: no branch.  c1 < c2: UnprojectStereo
    # of KF1.  cosParallaxRays < 0, so c2 < c1: UnprojectStereo of pKF2 although bStereo1 holds
    both = []
    for qi, i1 in enumerate(c["idx1"][2]):
        i2 = int(c["q"][2]["start"][qi])                       # one feature per node: the run starts at its partner
        i2 = int(c["neigh"][2]["fidx"][i2])
        if c["cur"]["uright"][i1] >= 0 and c["store"][2]["uright"][i2] >= 0:
            k1, k2 = c["cur"]["keysun"][i1], c["store"][2]["kps"][i2]
            cr = nc.cos_parallax_rays(C1, nc.cam_of(c["nb"][2]), k1["x"], k1["y"], k2["x"], k2["y"])[0]
            c1_ = nc.F(nc._libm.cosf(nc.F(2) * nc.F(nc._libm.atan2f(C1.mb / nc.F(2), c["cur"]["depth"][i1]))))
            both.append((nc.status_names(nc.ST, r["status"][2, qi])[0], np.sign(float(c1_) - float(cr + nc.F(1))), float(cr) > 0))
    assert sorted(both) == sorted([("LOW_PARALLAX", 0.0, False), ("CREATED", -1.0, False), ("CREATED", 1.0, False)]), both
    # the order dependence: dropped BEFORE the histogram, bin 12 survives and the two others of bin 0 go; dropped behind it, the other way round
    c, r = by["order-K3"]
    late = nc.create_points(c, apply_taken_late=True)
    n = c["note"]
    st = lambda res, k, i1: int(res["status"][k, c["idx1"][k].tolist().index(i1)])
    assert st(r, 1, n["a"]) == nc.ST["TAKEN"] and r["created_by"][n["a"]] == 0
    assert all(st(r, 1, i) == nc.ST["CREATED"] for i in n["bin12"]) and all(st(r, 1, i) == nc.ST["NO_MATCH"] for i in n["bin0"])
    assert all(st(late, 1, i) == nc.ST["NO_MATCH"] for i in n["bin12"]) and all(st(late, 1, i) == nc.ST["CREATED"] for i in n["bin0"])
    assert r["nmatches"][1] == 9 and late["nmatches"][1] == 8
    s1, s2, i2 = n["same_idx2"]
    assert r["created_by"][s1] == 0 and r["created_by"][s2] == 0 and sorted(p["idx2"] for p in r["new"] if p["idx1"] in (s1, s2)) == [i2, i2]
    assert st(r, 0, n["g"]) == nc.ST["REPROJ1_MONO"] and r["created_by"][n["g"]] == 2
    assert np.array_equal(r["new"]["k"], np.sort(r["new"]["k"]))      # creation order: k ascending, idx1 ascending inside
    for k in range(3):
        i = r["new"]["idx1"][r["new"]["k"] == k]
        assert np.array_equal(i, np.sort(i))
    # lines
    c, r = line_case
    n = c["note"]
    assert r["created_by"][n["chain"]] == 0 and r["status"][1, n["chain"]] == nc.STL["TAKEN"] and r["status"][2, n["chain"]] == nc.STL["TAKEN"]
    assert r["created_by"][n["second"]] == 1 and r["status"][2, n["second"]] == nc.STL["TAKEN"] and r["match"][2, n["second"]] == -1
    assert (c["cur"]["lineeq"][n["mono_says"]] <= 0).all() and c["cur"]["lineeq"][n["stereo_says"]] > 0
    assert len(c["neigh"][3]["keylines"]) == 0 and not c["nb"][4]["active"] and (c["match0"] >= len(c["cur"]["keylines"])).sum() == 1


def test_restated_search_equals_the_sequential_oracle(point_cases):
    """the numpy SearchForTriangulation on the first neighbour of every case (nobody is taken yet) against oracle/kf_oracle.cpp"""
    import oracle_lib
    for c, _ in point_cases:
        if not len(c["q"][0]) or not c["nb"][0]["active"]:
            continue
        st, ng, nb = c["store"][0], c["neigh"][0], c["nb"][0]
        sf, sig2 = nc.tables(c)
        nm, m = nc.search(st["kps"], st["desc"], st["uright"], ng["taken"], ng["fidx"], c["q"][0], c["qd"][0], np.zeros(len(c["q"][0]), bool), nb["F12"],
                          (nb["ex"], nb["ey"]), c["only_stereo"], c["check_ori"], sf, sig2)
        onm, om = oracle_lib.search_for_triangulation(st["kps"], st["desc"], st["uright"], ng["taken"], ng["fidx"], c["q"][0], c["qd"][0], nb["F12"],
                                                      (nb["ex"], nb["ey"]), sf, sig2, c["only_stereo"], c["check_ori"])
        assert nm == onm and np.array_equal(m, om), c["name"]


def literal_loop(c):
    """src/LocalMapping.cc:305-519 transcribed: per neighbour the head of SearchForTriangulation (src/ORBmatcher.cc:689-711) walks both
    feature vectors with GetMapPoint as it is NOW, the search and the triangulation run, AddMapPoint changes GetMapPoint"""
    import psl_slam_amd as P
    cur = c["cur"]
    taken = np.array(cur["taken"], np.uint8).copy()
    sf, sig2 = nc.tables(c)
    C1 = nc.cam_of(c["kf1"][0])
    created = []
    for k, nb in enumerate(c["nb"]):
        if not nb["active"]:
            continue
        q, idx1, fidx2 = P.LocalMapping.TriQueries(c["fvec1"], c["fvec2"][k], cur["keysun"], cur["uright"], taken)
        st, ng = c["store"][k], c["neigh"][k]
        _, match = nc.search(st["kps"], st["desc"], st["uright"], ng["taken"], fidx2, q, cur["desc"][idx1].reshape(-1, 32), np.zeros(len(q), bool),
                             nb["F12"], (nb["ex"], nb["ey"]), False, c["check_ori"], sf, sig2)
        C2 = nc.cam_of(nb)
        for i1, qi in sorted((int(idx1[qi]), qi) for qi in range(len(q)) if match[qi] >= 0):
            i2 = int(match[qi])
            o1 = (cur["keysun"]["x"][i1], cur["keysun"]["y"][i1], *cur["keys"][i1], cur["uright"][i1], cur["depth"][i1], cur["keysun"]["octave"][i1])
            o2 = (st["kps"]["x"][i2], st["kps"]["y"][i2], *ng["keys"][i2], st["uright"][i2], ng["depth"][i2], st["kps"]["octave"][i2])
            s, p = nc.point_row(C1, C2, c["kf1"][0]["mbf"], o1, o2, sf, sig2, c["kf1"][0]["ratio_factor"])
            if s == nc.ST["CREATED"]:
                taken[i1] = 1
                created.append((k, i1, i2, p))
    return created


class RestatedMatcher:
    """stands where a KeyFrameMatcher goes: CreateNewMapPoints answered by the restatement on the arrays the helper built"""

    def __init__(self, c):
        self.c = c

    def CreateNewMapPoints(self, frame2, kf1, keysun1, keys1, uright1, depth1, taken1, neighbours, fidx2, taken2, keys2, depth2, queries, idx1, qdesc,
                           scale_factors, level_sigma2, bOnlyStereo=False, checkOri=False):
        c = dict(self.c, q=queries, idx1=idx1, qd=qdesc, only_stereo=bOnlyStereo, check_ori=checkOri,
                 neigh=[dict(n, fidx=f) for n, f in zip(self.c["neigh"], fidx2)])
        return nc.create_points(c)


def helper_inputs(c):
    cur = dict(c["cur"], fvec=c["fvec1"])
    neigh = [dict(keys=n["keys"], depth=n["depth"], taken=n["taken"], fvec=f) for n, f in zip(c["neigh"], c["fvec2"])]
    return cur, neigh


def test_local_mapping_helper_equals_the_literal_loop(point_cases):
    import psl_slam_amd as P
    for name in ("general-s5", "general-s7"):
        c = next(c for c, _ in point_cases if c["name"].startswith(name))
        cur, neigh = helper_inputs(c)
        r, created = P.LocalMapping.CreateNewMapPoints(RestatedMatcher(c), None, c["kf1"], cur, c["nb"], neigh, c["sf"], c["sig2"], checkOri=c["check_ori"])
        want = literal_loop(c)
        assert len(created) == len(want) >= 10
        for g, w in zip(created, want):
            assert g[:3] == w[:3] and g[3].tobytes() == w[3].tobytes(), (name, g, w)
        for k in range(len(c["nb"])):                           # the helper's query lists are the case's own
            assert np.array_equal(r["match"][k, :len(c["q"][k])] >= 0, nc.create_points(c)["match"][k, :len(c["q"][k])] >= 0)


def test_abi_pods_and_error_codes_without_a_device():
    import psl_slam_amd as P
    assert P.TRIKEYFRAME_DTYPE == nc.TRIKEYFRAME_DTYPE and P.TRINEIGHBOUR_DTYPE == nc.TRINEIGHBOUR_DTYPE
    assert P.NEWMAPPOINT_DTYPE == nc.NEWMAPPOINT_DTYPE and P.NEWMAPLINE_DTYPE == nc.NEWMAPLINE_DTYPE
    assert (P.TRIKEYFRAME_DTYPE.itemsize, P.TRINEIGHBOUR_DTYPE.itemsize, P.NEWMAPPOINT_DTYPE.itemsize, P.NEWMAPLINE_DTYPE.itemsize) == (80, 128, 24, 36)
    assert P.TRINEIGHBOUR_DTYPE.fields["Tcw"][1] == 60 and P.TRIKEYFRAME_DTYPE.fields["kf"][1] == 76
    assert list(P.TRI_STATUS) == list(nc.ST) and list(P.TRIL_STATUS) == list(nc.STL)
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    for i, n in enumerate(P.TRI_STATUS):
        assert f"#define PSL_TRI_{n} {i} " in hdr or f"#define PSL_TRI_{n} {i}\n" in hdr, n
    for i, n in enumerate(P.TRIL_STATUS):
        assert f"#define PSL_TRIL_{n} {i} " in hdr or f"#define PSL_TRIL_{n} {i}\n" in hdr, n
    assert "sizeof(PslTriNeighbour) == 128" in hdr
    L = P.lib()
    null = C.c_void_p(None)
    i = lambda v: C.c_int(v)
    sent = np.full(4, 77, np.int32)
    s = P._ptr(sent)

    def points(fn, N1=0, K=0, nqmax=0, nlevels=8, extra=0):
        args = [null, null, null, i(N1)] + [null] * 5 + [null, i(K)] + [null] * 9 + [null, i(nqmax), i(0), i(0), null, null, i(nlevels)] + [s] * 8
        return fn(*args, *([s] * extra))
    for fn, extra in ((L.pslfe_kf_create_new_map_points, 0), (L.pslfe_kf_create_new_map_points_device, 4)):
        assert points(fn, extra=extra) == 0                                                     # K == 0: nothing looked at, nothing written
        assert points(fn, N1=-1, extra=extra) == -1 and points(fn, N1=4097, extra=extra) == -1 and points(fn, nqmax=4097, extra=extra) == -1
        assert points(fn, K=-1, extra=extra) == -1 and points(fn, K=33, extra=extra) == -1
        assert points(fn, K=1, extra=extra) == -1                                               # NULL handle and arrays
        assert b"pslfe_kf_create_new_map_points" in L.pslfe_last_error()
    assert (sent == 77).all()

    def lines(fn, NL1=0, K=0, nlevels=8, extra=0):
        args = [null, null, i(NL1)] + [null] * 5 + [null, i(K)] + [null] * 5 + [C.c_float(0.95), C.c_float(50), i(1), null, null, i(nlevels)] + [s] * 9
        return fn(*args, *([s] * extra))
    for fn, extra in ((L.pslfe_kf_create_new_map_lines, 0), (L.pslfe_kf_create_new_map_lines_device, 4)):
        assert lines(fn, extra=extra) == 0
        assert lines(fn, NL1=-1, extra=extra) == -1 and lines(fn, K=-1, extra=extra) == -1 and lines(fn, K=33, extra=extra) == -1
        assert lines(fn, NL1=65536, extra=extra) == -1
        assert lines(fn, NL1=4, K=1, extra=extra) == -1
        assert b"pslfe_kf_create_new_map_lines" in L.pslfe_last_error()
    assert (sent == 77).all()
