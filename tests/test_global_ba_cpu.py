"""The restatement of the global bundle adjustment (tests/gba_cases.py) and the stand-alone host program of tools/dropin/gba_main.cpp
(the driver psl_gba_optimize of psl-slam_amd/csrc/gba_kernels.h on PslLmSerial, compiled with g++ under the address and
undefined-behaviour sanitizers), bit for bit with each other on every case that Python runs; the restatement against the local
BA's first round where the two must agree (stereo edges only) and where they must not (a monocular edge above the Huber threshold:
(float)sqrt(5.99) against (float)sqrt(5.991)); what the extra cases exercise; the ABI.  No GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_cases as bc
import gba_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = gc.CAPS


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    """the driver's host form as a stand-alone program, built once with g++ alone under -fsanitize=address,undefined"""
    exe = str(tmp_path_factory.mktemp("global_ba") / "gba_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-DPSL_GBA_HOST_ONLY", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "gba_main.cpp")],
                   check=True, capture_output=True)
    return exe


def test_host_program_under_sanitizers_equals_restatement(host_exe, tmp_path):
    """every case of gba_cases.parity_cases(): poses, points, not_included and every PslGbaInfo field; refused problems too"""
    groups = {}
    for name, it, rb in gc.parity_cases():
        groups.setdefault((it, rb), []).append(dict(gc.scene(name), ref=gc.ref(name, it, rb), name=name))
    for (it, rb), group in groups.items():
        group = group + [c for c, _ in gc.refused_cases(it, rb, CAPS)]
        path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
        gc.write_cases(path, group, it, rb, CAPS)
        p = subprocess.run([host_exe, path, out], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
        for k, (g, c) in enumerate(zip(gc.read_sections(out, group, 1)[0], group)):
            gc.assert_equal(g, c["ref"], (it, rb, k, c.get("name")))


def test_restatement_meets_local_ba_where_the_deltas_agree():
    """robust, 5 iterations on stereo edges alone is LocalBundleAdjustment's round one: equal in the free keyframes and in all points.
    On a monocular scene the two differ in an output bit: the test sees 5.99 against 5.991."""
    for name in gc.STEREO_ONLY:
        c = gc.scene(name)
        assert (c["edges"]["ur"] >= 0).all(), name
        g, l = gc.ref(name, 5, 1), bc.local_ba(c["kf"], c["mp"], c["edges"], c["cam"], rounds=1)
        free = c["kf"]["fixed"] == 0
        assert free.any() and g["kf"][free].tobytes() == l["kf"][free].tobytes(), name
        assert g["mp"].tobytes() == l["mp"].tobytes(), name
        assert int(g["info"]["iterations"]) == int(l["info"]["iterations"][0]), name
        assert float(g["info"]["chi2_start"]) == float(l["info"]["chi2_start"]) and float(g["info"]["chi2_end"]) == float(l["info"]["chi2_round1"]), name
    c = gc.scene("f2_x2_p8_mono")
    assert (c["edges"]["ur"] < 0).all()
    g, l = gc.ref("f2_x2_p8_mono", 5, 1), bc.local_ba(c["kf"], c["mp"], c["edges"], c["cam"], rounds=1)
    free = c["kf"]["fixed"] == 0
    assert g["kf"][free].tobytes() != l["kf"][free].tobytes() or g["mp"].tobytes() != l["mp"].tobytes()
    plain = gc.ref("f2_x2_p8_mono", 10, 0)          # without the kernel the delta is not read
    assert int(plain["info"]["status"]) == 0 and float(plain["info"]["chi2_end"]) <= float(plain["info"]["chi2_start"])


def test_cases_are_what_their_names_say():
    """the restated results alone: what the extra cases exercise, which the parity tests then hold the product code to"""
    for name, it, rb in gc.parity_cases():
        r = gc.ref(name, it, rb)
        assert int(r["info"]["status"]) == 0 and 1 <= int(r["info"]["iterations"]) <= it, (name, it, rb)
    for F in gc.WINDOW_F:                           # the panel and tile edges: the system has exactly F pose blocks
        r, c = gc.ref(f"window_F{F}", 5, 1), gc.scene(f"window_F{F}")
        assert int(r["info"]["free_keyframes"]) == F and len(c["kf"]) == F + 1 and not r["not_included"].any()
        assert float(r["info"]["chi2_end"]) < float(r["info"]["chi2_start"])
    c = gc.scene("window_F22")                      # most keyframe pairs share no point
    seen = [set(c["edges"]["point"][c["edges"]["kf"] == k]) for k in range(len(c["kf"]))]
    pairs = [(a, b) for a in range(len(seen)) for b in range(a + 1, len(seen))]
    assert sum(1 for a, b in pairs if seen[a] & seen[b]) < len(pairs) / 2
    assert int(gc.ref("dense_F22", 5, 1)["info"]["free_keyframes"]) == 22
    for name, terms in zip(gc.CHAIN_NAMES, (510, 513)):     # computeScale's chain on both sides of one chunk of 512
        r = gc.ref(name, 5, 1)
        assert 6 * int(r["info"]["free_keyframes"]) + 3 * len(gc.scene(name)["mp"]) == terms and not r["not_included"].any()
    for F in gc.LOOP_ONLY_F:                                # rows only: every keyframe has an edge, so the system has F blocks
        c = gc.scene(f"window_F{F}")
        assert len(c["kf"]) == F + 1 and len(set(c["edges"]["kf"])) == F + 1 and all(n <= cap for n, cap in zip((len(c["kf"]), len(c["mp"]), len(c["edges"])), CAPS))

    c, r = gc.scene("f2_x1_p8_mixed"), gc.ref("f2_x1_p8_mixed", 5, 1)      # the fixed keyframe comes back through the quaternion
    k = int(np.flatnonzero(c["kf"]["fixed"])[0])
    want = gc.to_pose(gc.from_pose(c["kf"]["Tcw"][k]))
    assert r["kf"]["Tcw"][k].tobytes() == want.tobytes() and int(r["kf"]["fixed"][k]) == 1
    c, r = gc.scene("no_fixed"), gc.ref("no_fixed", 5, 1)
    assert not c["kf"]["fixed"].any() and int(r["info"]["free_keyframes"]) == len(c["kf"])
    c, r = gc.scene("point_without_edge"), gc.ref("point_without_edge", 5, 1)
    assert list(np.flatnonzero(r["not_included"])) == [2] and r["mp"][2].tobytes() == c["mp"][2].tobytes()
    assert int(r["info"]["included_points"]) == len(c["mp"]) - 1 and r["mp"][1].tobytes() != c["mp"][1].tobytes()
    c, r = gc.scene("keyframe_without_edge"), gc.ref("keyframe_without_edge", 5, 1)
    assert int(c["kf"]["fixed"][2]) == 0 and int(r["info"]["free_keyframes"]) == len(c["kf"]) - 2
    assert r["kf"]["Tcw"][2].tobytes() == gc.to_pose(gc.from_pose(c["kf"]["Tcw"][2])).tobytes()
    tr = gc.ref("lambda_grows", 20, 1)["trials"]
    assert tr[0][0] == 0 and tr[0][1] and tr[0][3] < 0 and tr[1][4] == 2 * tr[0][4]
    assert gc.ref("stopped_by_nbad", 20, 1)["stopped"] == "nbad"
    assert all(not ok and why == "landmark" for _, ok, why, _, _ in gc.ref("failed_solve", 5, 1)["trials"])
    assert any(not ok and why == "pivot" for _, ok, why, _, _ in gc.ref("failed_pivot", 5, 1)["trials"])


def test_abi_pods_and_error_codes_without_a_device():
    import psl_slam_amd as P
    assert P.GBAINFO_DTYPE == gc.INFO_DTYPE and P.GBAINFO_DTYPE.itemsize == 40 and P.GBAINFO_DTYPE.fields["chi2_start"][1] == 16
    hdr = open(os.path.join(ROOT, "include", "pslfe.h")).read()
    assert "sizeof(PslGbaInfo) == 40" in hdr and "2.4474475383758545" in hdr
    L = P.lib()
    null = C.c_void_p(None)
    info = np.zeros(1, P.GBAINFO_DTYPE)
    for f in (L.pslfe_gba_optimize_device, L.pslfe_gba_optimize):
        call = lambda nkf=0, nmp=0, ne=0, it=5, rb=1, inf=P._ptr(info): f(null, null, C.c_int(nkf), null, C.c_int(nmp), null, C.c_int(ne), null, C.c_int(it),
                                                                          C.c_int(rb), null, null, null, inf)
        assert call(nkf=-1) == -1 and call(nmp=-1) == -1 and call(ne=-1) == -1 and call(it=0) == -1 and call(rb=2) == -1 and call(rb=-1) == -1
        assert call() == -1 and call(inf=null) == -1                # a NULL handle, camera or info
        assert b"pslfe_gba_optimize" in L.pslfe_last_error()
    out = C.c_void_p()
    assert L.pslfe_gba_create(null, 1, 1, 1, C.byref(out)) == -1 and L.pslfe_gba_create(null, 1, 1, 1, None) == -1
    L.pslfe_gba_destroy.restype = None
    L.pslfe_gba_destroy(null)
