"""GPU parity of the essential-graph optimisation (psl-slam_amd/csrc/pslfe_essential.hip) with the restatement of
tests/essential_cases.py, bit for bit: poses, optimised Sim3s, corrected points, status, iterations, both chi2, the final lambda and
the mask of log branches, for the kernel, the library's host-array form and the C++ consumer tools/dropin/essential_main.cpp; the
smallest shapes, more than one item per thread, one launch of four graphs with refused ones in the middle, the whole-call error
paths, and the chain into pslfe_kf_update_normal_and_depth_device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import essential_cases as ec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["two_one_fixed", "fixed_in_middle", "chain5_loop", "chain5_loop_fix_scale", "free_without_edge", "ring12", "ring12_fix_scale",
         "two_long_rows", "branches"]


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


@pytest.fixture(scope="module")
def handle():
    import psl_slam_amd as P
    eg = P.EssentialGraph(4, *ec.CAPS)
    yield eg
    eg.close()


def _run_device(P, eg, cases, fix_scale, alias=False, offsets=None):
    """the cases as one launch -> [dict(info, pose, S, mp)]; pose rows start as zeros (a refused graph writes none), S as 0xAA bytes"""
    ctx = eg.ctx
    K = len(cases)
    cat = lambda k, dt: np.concatenate([np.ascontiguousarray(c[k], dt).reshape(-1) for c in cases] + [np.zeros(1, dt)])   # never empty
    kf, ed, mp, ref = cat("kf", P.EGKEYFRAME_DTYPE), cat("edges", P.EGEDGE_DTYPE), cat("mp", P.MAPPOINT_DTYPE), cat("mp_ref", np.int32)
    off = offsets or [np.cumsum([0] + [len(c[k]) for c in cases]).astype(np.int32) for k in ("kf", "edges", "mp")]
    d_kf, d_ed, d_mp, d_ref = _dev(ctx, kf), _dev(ctx, ed), _dev(ctx, mp), _dev(ctx, ref)
    d_off = [_dev(ctx, o) for o in off]
    d_pose, d_S = _dev(ctx, np.zeros(len(kf), P.POSE_DTYPE)), _dev(ctx, np.full(64 * len(kf), 0xAA, np.uint8))
    d_mo = d_mp if alias else _dev(ctx, np.zeros(len(mp), P.MAPPOINT_DTYPE))
    d_info = _dev(ctx, np.zeros(K, P.EGINFO_DTYPE))
    P.Optimizer.OptimizeEssentialGraphDevice(eg, K, d_kf, d_off[0], d_ed, d_off[1], d_mp, d_ref, d_off[2], fix_scale, d_pose, d_S, d_mo, d_info)
    ctx.synchronize()
    pose, S = _down(P, ctx, d_pose, np.zeros(len(kf), P.POSE_DTYPE)), _down(P, ctx, d_S, np.zeros((len(kf), 8), np.float64))
    mo, info = _down(P, ctx, d_mo, np.zeros(len(mp), P.MAPPOINT_DTYPE)), _down(P, ctx, d_info, np.zeros(K, P.EGINFO_DTYPE))
    for d in {d_kf, d_ed, d_mp, d_ref, d_pose, d_S, d_mo, d_info, *d_off}:
        ctx.device_free(d)
    o = [np.cumsum([0] + [len(c[k]) for c in cases]) for k in ("kf", "mp")]
    return [{"info": info[k], "pose": pose[o[0][k]:o[0][k + 1]], "S": S[o[0][k]:o[0][k + 1]], "mp": mo[o[1][k]:o[1][k + 1]]} for k in range(K)]


@pytest.mark.parametrize("name", SMALL)
def test_device_and_host_forms_equal_restatement(name, handle):
    """2 keyframes / 1 edge with one fixed (7 unknowns); the fixed keyframe in a middle row; a chain of 5 with a loop edge from the last
    to the first row (one envelope row spans the matrix), with and without fix_scale; a free keyframe without an edge; the ring of
    12; two long rows; all four branches of log in one graph (the mask equals the restatement's) - each through the kernel, in and
    out of place, and through the host-array form"""
    import psl_slam_amd as P
    c = ec.case(name)
    for alias in (False, True):
        ec.assert_equal_ref(_run_device(P, handle, [c], c["fix_scale"], alias=alias)[0], c["ref"], (name, alias))
    pose, S, mp, info = P.Optimizer.OptimizeEssentialGraph(handle, c["kf"], c["edges"], c["mp"], c["mp_ref"], c["fix_scale"])
    ec.assert_equal_ref({"info": info, "pose": pose, "S": S, "mp": mp}, c["ref"], name + " (host form)")
    if name == "branches":
        assert int(info["log_branches"]) == 15
    if name == "chain5_loop":
        assert c["ref"]["graph"].fb == [0, 1, 1, 0]


def test_more_than_one_item_per_thread(handle):
    """100 keyframes / 300 edges (more edges than threads, 693 unknowns) and 300 map points spread over the keyframes"""
    import psl_slam_amd as P
    c = ec.case("big_100_300")
    assert len(c["kf"]) == 100 and len(c["edges"]) == 300 and len(c["mp"]) == 300 and 7 * int(c["ref"]["info"]["nfree"]) > 256
    assert len(set(c["mp_ref"][c["mp_ref"] >= 0])) > 50
    ec.assert_equal_ref(_run_device(P, handle, [c], False)[0], c["ref"], "big_100_300")


def test_one_launch_of_four_with_refused_graphs(handle):
    """a normal graph, an empty one, one above a cap and one with an edge outside its rows in one launch: the statuses, the refused
    graphs' outputs equal to their inputs, the neighbours unaffected; then the other refusals and the host form's return values"""
    import psl_slam_amd as P
    good = ec.case("chain5_loop")
    empty, over, outside, selfloop, badpoint = ec.refused_cases()
    for group, want in (([good, empty, over, outside], [0, 0, ec.E_CAPACITY, ec.E_INVALID]), ([selfloop, good, badpoint, empty], [ec.E_INVALID, 0, ec.E_INVALID, 0])):
        for alias in (False, True):
            got = _run_device(P, handle, group, False, alias=alias)
            for k, (g, c, st) in enumerate(zip(got, group, want)):
                assert int(g["info"]["status"]) == st, (k, g["info"])
                ec.assert_equal_ref(g, c["ref"], (k, alias))
                if st < 0:
                    assert g["S"].tobytes() == np.ascontiguousarray(c["kf"]["Scw"]).tobytes() and not g["pose"].view(np.uint8).any()
                    assert g["mp"].tobytes() == np.ascontiguousarray(c["mp"], P.MAPPOINT_DTYPE).tobytes()
    small = ec.case("two_long_rows")                       # an envelope above the handle's cap
    eg = P.EssentialGraph(1, ec.CAPS[0], ec.CAPS[1], ec.CAPS[2], small["ref"]["graph"].env_size - 1)
    try:
        g = _run_device(P, eg, [small], False)[0]
        assert int(g["info"]["status"]) == ec.E_CAPACITY and g["S"].tobytes() == np.ascontiguousarray(small["kf"]["Scw"]).tobytes()
        with pytest.raises(P.PslfeError, match="-4"):
            P.Optimizer.OptimizeEssentialGraph(eg, small["kf"], small["edges"], small["mp"], small["mp_ref"], False)
    finally:
        eg.close()
    with pytest.raises(P.PslfeError, match="-1"):
        P.Optimizer.OptimizeEssentialGraph(handle, outside["kf"], outside["edges"], outside["mp"], outside["mp_ref"], False)
    # descending offsets are an invalid graph, not a crash
    off = [np.array([0, len(good[k])], np.int32) for k in ("kf", "edges", "mp")]
    off[1] = np.array([len(good["edges"]), 0], np.int32)
    g = _run_device(P, handle, [good], False, offsets=off)[0]
    assert int(g["info"]["status"]) == ec.E_INVALID and (g["S"].view(np.uint8) == 0xAA).all() and not g["mp"].view(np.uint8).any()


def test_whole_call_errors_and_empty_launch(handle):
    import psl_slam_amd as P
    ctx = handle.ctx
    L = P.lib()
    d = _dev(ctx, np.zeros(256, np.int32))
    p, null = C.c_void_p(d), C.c_void_p(None)
    f = L.pslfe_eg_optimize_device
    names = ("kf", "kf_off", "ed", "ed_off", "mp", "ref", "mp_off", "pose", "S", "mo", "info")
    def args(eg=handle._h, K=1, **kw):
        a = [kw.get(n, p) for n in names]
        return [eg, C.c_int(K)] + a[:7] + [C.c_int(0)] + a[7:]
    assert f(*args(K=0)) == 0 and f(*args(K=0, eg=null, kf=null)) == 0            # K == 0: nothing is looked at
    assert f(*args(K=-1)) == -1 and f(*args(K=5)) == -1 and f(*args(eg=null)) == -1   # above max_graphs; no handle
    for n in names:
        assert f(*args(**{n: null})) == -1, n
    c = L.pslfe_eg_create
    out = C.c_void_p()
    assert c(ctx._h, 0, 1, 1, 1, C.c_int64(1), C.byref(out)) == -1 and c(ctx._h, 1, 1, 1, 1, C.c_int64(0), C.byref(out)) == -1
    ctx.device_free(d)


def test_chain_into_update_normal_and_depth(handle):
    """d_mp_out goes into pslfe_kf_update_normal_and_depth_device without a host copy; the result is the restatement of both steps"""
    import psl_slam_amd as P
    import map_upkeep_cases as mc
    ctx = handle.ctx
    c = ec.case("ring12")
    ref = c["ref"]
    M, nkf = len(c["mp"]), len(c["kf"])
    obs = [[(p + k) % nkf for k in range(1 + p % 3)] for p in range(M)]          # mObservations of every point
    off = np.cumsum([0] + [len(o) for o in obs]).astype(np.int32)
    okf = np.array([k for o in obs for k in o], np.int32)
    ref_kf, ref_level = np.array([o[0] for o in obs], np.int32), np.ones(M, np.int32)
    centres = np.zeros((nkf, 3), np.float32)
    for k in range(nkf):          # Ow = -Rcw^T tcw of the corrected poses, in float as the upkeep takes them
        R, t = ref["pose"]["R"][k].reshape(3, 3).astype(np.float64), ref["pose"]["t"][k].astype(np.float64)
        centres[k] = (-R.T @ t).astype(np.float32)
    want = mc.restate_points(np.ascontiguousarray(ref["mp"], P.MAPPOINT_DTYPE), off, okf, centres, ref_kf, ref_level, mc.SCALE, None)
    d_kf, d_ed = _dev(ctx, np.ascontiguousarray(c["kf"], P.EGKEYFRAME_DTYPE)), _dev(ctx, np.ascontiguousarray(c["edges"], P.EGEDGE_DTYPE))
    d_mp, d_ref = _dev(ctx, np.ascontiguousarray(c["mp"], P.MAPPOINT_DTYPE)), _dev(ctx, np.ascontiguousarray(c["mp_ref"], np.int32))
    d_off = [_dev(ctx, np.array([0, n], np.int32)) for n in (nkf, len(c["edges"]), M)]
    d_pose, d_S, d_info = _dev(ctx, np.zeros(nkf, P.POSE_DTYPE)), _dev(ctx, np.zeros((nkf, 8))), _dev(ctx, np.zeros(1, P.EGINFO_DTYPE))
    ins = [_dev(ctx, a) for a in (off, okf, centres, ref_kf, ref_level)]
    P.Optimizer.OptimizeEssentialGraphDevice(handle, 1, d_kf, d_off[0], d_ed, d_off[1], d_mp, d_ref, d_off[2], False, d_pose, d_S, d_mp, d_info)
    P.KeyFrameMatcher(ctx=ctx).update_normal_and_depth_device(d_mp, M, ins[0], ins[1], ins[2], nkf, ins[3], ins[4], 0, mc.SCALE)
    ctx.synchronize()
    got = _down(P, ctx, d_mp, np.zeros(M, P.MAPPOINT_DTYPE))
    for d in [d_kf, d_ed, d_mp, d_ref, d_pose, d_S, d_info] + d_off + ins:
        ctx.device_free(d)
    assert got.tobytes() == want.tobytes()
    assert want.tobytes() != np.ascontiguousarray(ref["mp"], P.MAPPOINT_DTYPE).tobytes()        # the second step did something


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/essential_main.cpp on pslfe.hpp: the batched device form (points in place), the graph-by-graph host form and its
    own plain C++ loop agree with the restatement in every output byte; refused graphs in the file as well"""
    exe = str(tmp_path / "essential_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "essential_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    for fs in (False, True):
        group = [ec.case(n) for n in SMALL if ec.case(n)["fix_scale"] == fs]
        if not fs:
            refused = ec.refused_cases()
            group = group[:2] + refused[:3] + group[2:] + refused[3:]
        path, out = str(tmp_path / f"cases{int(fs)}.bin"), str(tmp_path / f"out{int(fs)}.bin")
        ec.write_cases(path, group, fs)
        p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        for form, sec in zip(("loop", "device", "host"), ec.read_sections(out, group, 3)):
            for k, (g, c) in enumerate(zip(sec, group)):
                ec.assert_equal_ref(g, c["ref"], (form, fs, k))
