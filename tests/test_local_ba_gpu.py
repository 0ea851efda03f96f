"""GPU parity of the local bundle adjustment (psl-slam_amd/csrc/pslfe_ba.hip) with the restatement of tests/ba_cases.py, bit for bit:
poses, points, erase flags, status, rounds, iterations and the three chi2 values (a NaN equals a NaN), for the kernel, the library's
host form and the C++ consumer tools/dropin/ba_main.cpp; launches of 1, 3 and 65 problems of unequal sizes, refused problems in the
middle of a launch, aliased outputs, the whole-call error paths, and the chain into pslfe_kf_update_normal_and_depth_device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_cases as bc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS_WIDE = (16, 128, 512)       # holds every case of ba_cases.CASE_NAMES


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _cam(P, c):
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in c.items():
        cam[k] = v
    return cam


@pytest.fixture(scope="module")
def wide():
    import psl_slam_amd as P
    ba = P.BundleAdjuster(65, *CAPS_WIDE)
    yield ba
    ba.close()


def _run_device(P, ba, cases, rounds, alias=False, offsets=None):
    """the cases as one launch -> [dict(info, kf, mp, erase)]; the erase bytes start as 0xAA, out-of-place outputs as zeros"""
    ctx = ba.ctx
    K = len(cases)
    kf = np.concatenate([np.ascontiguousarray(c["kf"], P.BAKEYFRAME_DTYPE) for c in cases])
    mp = np.concatenate([np.ascontiguousarray(c["mp"], P.MAPPOINT_DTYPE) for c in cases])
    ed = np.concatenate([np.ascontiguousarray(c["edges"], P.BAEDGE_DTYPE) for c in cases])
    off = offsets or [np.cumsum([0] + [len(c[k]) for c in cases]).astype(np.int32) for k in ("kf", "mp", "edges")]
    d_kf, d_mp, d_ed = _dev(ctx, kf), _dev(ctx, mp), _dev(ctx, ed)
    d_off = [_dev(ctx, o) for o in off]
    d_ko = d_kf if alias else _dev(ctx, np.zeros(len(kf), P.BAKEYFRAME_DTYPE))
    d_mo = d_mp if alias else _dev(ctx, np.zeros(len(mp), P.MAPPOINT_DTYPE))
    d_er, d_info = _dev(ctx, np.full(max(len(ed), 1), 0xAA, np.uint8)), _dev(ctx, np.zeros(K, P.BAINFO_DTYPE))
    P.Optimizer.LocalBundleAdjustmentDevice(ba, K, d_kf, d_off[0], d_mp, d_off[1], d_ed, d_off[2], _cam(P, cases[0]["cam"]), rounds, d_ko, d_mo, d_er, d_info)
    ctx.synchronize()
    ko, mo = _down(P, ctx, d_ko, np.zeros(len(kf), P.BAKEYFRAME_DTYPE)), _down(P, ctx, d_mo, np.zeros(len(mp), P.MAPPOINT_DTYPE))
    er, info = _down(P, ctx, d_er, np.zeros(max(len(ed), 1), np.uint8)), _down(P, ctx, d_info, np.zeros(K, P.BAINFO_DTYPE))
    for d in {d_kf, d_mp, d_ed, d_ko, d_mo, d_er, d_info, *d_off}:
        ctx.device_free(d)
    o = [np.cumsum([0] + [len(c[k]) for c in cases]) for k in ("kf", "mp", "edges")]
    return [{"info": info[k], "kf": ko[o[0][k]:o[0][k + 1]], "mp": mo[o[1][k]:o[1][k + 1]], "erase": er[o[2][k]:o[2][k + 1]]} for k in range(K)]


def _same(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("kf", "mp", "erase")) and \
        bytes(np.asarray(a["info"]).tobytes()[:20]) == bytes(np.asarray(b["info"]).tobytes()[:20])


@pytest.mark.parametrize("name", bc.CASE_NAMES)
def test_device_and_host_forms_equal_restatement(name, wide):
    """the shapes (1 + 1 keyframes / 6 points; 2 + 1 / 8 stereo; 2 + 2 / 8 monocular; mixed; 5 + 3 / 40; the caps 8 / 64 / 256 exactly,
    on a handle created with those caps) and the edge cases of ba_cases.EDGE_CASES, each through the kernel and the host form"""
    import psl_slam_amd as P
    c = bc.case(name)
    ba = P.BundleAdjuster(1, *bc.CAPS) if name == "caps_8_64_256" else wide
    try:
        if name == "caps_8_64_256":
            assert (len(c["kf"]), len(c["mp"]), len(c["edges"])) == bc.CAPS
        got = _run_device(P, ba, [c], c["rounds"])[0]
        bc.assert_equal_ref(got, c["ref"], name)
        ko, mo, er, info = P.Optimizer.LocalBundleAdjustment(ba, c["kf"], c["mp"], c["edges"], _cam(P, c["cam"]), c["rounds"])
        bc.assert_equal_ref({"info": info, "kf": ko, "mp": mo, "erase": er}, c["ref"], name + " (host form)")
    finally:
        if ba is not wide:
            ba.close()


@pytest.mark.parametrize("K", [1, 3, 65])
def test_launches_of_unequal_problems(K, wide):
    """K problems of unequal sizes in one launch, out of place and in place: a problem's result depends neither on its neighbours nor
    on its position"""
    import psl_slam_amd as P
    names = [n for n in bc.CASE_NAMES if n not in ("threshold_ulps", "rounds_1")]
    cases = [bc.case(names[(3 * k + 1) % len(names)]) for k in range(K)]
    for alias in (False, True):
        got = _run_device(P, wide, cases, 2, alias=alias)
        for k, (g, c) in enumerate(zip(got, cases)):
            bc.assert_equal_ref(g, c["ref"], (K, k, alias))
    rev = _run_device(P, wide, cases[::-1], 2)[::-1]
    assert all(_same(a, b) for a, b in zip(rev, got))


def test_refused_problems_leave_their_neighbours_alone(wide):
    """one problem above the handle's caps, one with an edge outside it, one with a duplicate (point, keyframe) pair and one without a
    free keyframe in the middle of a launch: each keeps its rows and reports its status; the others equal the restatement"""
    import psl_slam_amd as P
    good = [bc.case(n) for n in ("f2_x1_p8_mixed", "f5_x3_p40", "f1_x1_p6")]
    big = bc.make_scene(77, 2, 1, CAPS_WIDE[1] + 1, "mono", pobs=0.9)                      # one point too many
    outside = dict(good[0], edges=good[0]["edges"].copy())
    outside["edges"]["kf"][3] = len(outside["kf"])
    dup = dict(good[0], edges=np.concatenate([good[0]["edges"], good[0]["edges"][2:3]]))
    still = dict(good[0], kf=good[0]["kf"].copy())
    still["kf"]["fixed"] = 1
    cases = [good[0], big, good[1], outside, dup, still, good[2]]
    want = [0, bc.E_CAPACITY, 0, bc.E_INVALID, bc.E_INVALID, 0, 0]
    for alias in (False, True):
        got = _run_device(P, wide, cases, 2, alias=alias)
        for k, (g, c, st) in enumerate(zip(got, cases, want)):
            assert int(g["info"]["status"]) == st, (k, g["info"])
            if "ref" in c and c is not outside and c is not dup and c is not still:
                bc.assert_equal_ref(g, c["ref"], k)
            else:
                assert int(g["info"]["rounds"]) == 0 and g["kf"].tobytes() == np.ascontiguousarray(c["kf"], P.BAKEYFRAME_DTYPE).tobytes()
                assert g["mp"].tobytes() == np.ascontiguousarray(c["mp"], P.MAPPOINT_DTYPE).tobytes() and not g["erase"].any()
            r = bc.local_ba(c["kf"], c["mp"], c["edges"], c["cam"], 2, caps=CAPS_WIDE)
            assert int(r["info"]["status"]) == st and int(r["info"]["rounds"]) == int(g["info"]["rounds"])
    # the host form returns the status of a refused problem
    with pytest.raises(P.PslfeError, match="-4"):
        P.Optimizer.LocalBundleAdjustment(wide, big["kf"], big["mp"], big["edges"], _cam(P, big["cam"]))
    with pytest.raises(P.PslfeError, match="-1"):
        P.Optimizer.LocalBundleAdjustment(wide, dup["kf"], dup["mp"], dup["edges"], _cam(P, dup["cam"]))
    # descending offsets are an invalid problem, not a crash
    c = good[2]
    off = [np.array([0, len(c[k])], np.int32) for k in ("kf", "mp", "edges")]
    off[2] = np.array([len(c["edges"]), 0], np.int32)
    g = _run_device(P, wide, [c], 2, offsets=off)[0]
    assert int(g["info"]["status"]) == bc.E_INVALID and (g["erase"] == 0xAA).all() and not g["kf"].view(np.uint8).any()


def test_whole_call_errors_and_empty_launch(wide):
    import psl_slam_amd as P
    ctx = wide.ctx
    L = P.lib()
    cam = np.zeros(1, P.CAMERA_DTYPE)
    d = _dev(ctx, np.zeros(256, np.int32))
    p, null = C.c_void_p(d), C.c_void_p(None)
    f = L.pslfe_ba_local_device
    args = lambda **kw: [kw.get("ba", wide._h), C.c_int(kw.get("K", 1)), kw.get("kf", p), p, kw.get("mp", p), p, p, kw.get("eoff", p), kw.get("cam", P._ptr(cam)),
                         C.c_int(kw.get("rounds", 2)), p, p, kw.get("erase", p), kw.get("info", p)]
    assert f(*args(K=0)) == 0 and f(*args(K=0, ba=null, cam=null, kf=null)) == 0          # K == 0: nothing is looked at
    assert f(*args(K=-1)) == -1 and f(*args(rounds=0)) == -1 and f(*args(rounds=3)) == -1
    assert f(*args(K=66)) == -1                                                           # above max_problems
    for k in ("ba", "kf", "mp", "eoff", "cam", "erase", "info"):
        assert f(*args(**{k: null})) == -1, k
    h = L.pslfe_ba_local
    one = np.zeros(1, P.BAKEYFRAME_DTYPE)
    info = np.zeros(1, P.BAINFO_DTYPE)
    hargs = lambda nkf=1, kf=P._ptr(one), rounds=2, info=P._ptr(info), ba=wide._h: [ba, kf, C.c_int(nkf), None, C.c_int(0), None, C.c_int(0), P._ptr(cam),
                                                                                   C.c_int(rounds), P._ptr(one), None, None, info]
    assert h(*hargs(nkf=-1)) == -1 and h(*hargs(kf=None)) == -1 and h(*hargs(rounds=5)) == -1 and h(*hargs(info=None)) == -1 and h(*hargs(ba=null)) == -1
    assert h(*hargs()) == 0 and info[0]["rounds"] == 0                                      # a keyframe and nothing else: nothing to do
    c = L.pslfe_ba_create
    out = C.c_void_p()
    assert c(ctx._h, 0, 1, 1, 1, C.byref(out)) == -1 and c(ctx._h, 1, 1, 1, 0, C.byref(out)) == -1 and c(null, 1, 1, 1, 1, C.byref(out)) == -1
    ctx.device_free(d)


def test_chain_into_update_normal_and_depth(wide):
    """d_mp_out goes into pslfe_kf_update_normal_and_depth_device without a host copy; the result is the restatement of both steps"""
    import psl_slam_amd as P
    import map_upkeep_cases as mc
    ctx = wide.ctx
    c = bc.case("f5_x3_p40")
    ref = c["ref"]
    M, nkf = len(c["mp"]), len(c["kf"])
    # mObservations of every point: its edges' keyframes in edge order; the reference keyframe is the first of them at level 1
    obs = [[int(e["kf"]) for e in c["edges"] if e["point"] == p] for p in range(M)]
    off = np.cumsum([0] + [len(o) for o in obs]).astype(np.int32)
    okf = np.array([k for o in obs for k in o], np.int32)
    ref_kf, ref_level = np.array([o[0] for o in obs], np.int32), np.ones(M, np.int32)
    centres = np.zeros((nkf, 3), np.float32)
    for k in range(nkf):          # Ow = -Rcw^T tcw of the optimised poses, in float as the upkeep takes them
        R, t = ref["kf"]["Tcw"]["R"][k].reshape(3, 3).astype(np.float64), ref["kf"]["Tcw"]["t"][k].astype(np.float64)
        centres[k] = (-R.T @ t).astype(np.float32)
    want = mc.restate_points(np.ascontiguousarray(ref["mp"], P.MAPPOINT_DTYPE), off, okf, centres, ref_kf, ref_level, mc.SCALE, None)
    kf = np.ascontiguousarray(c["kf"], P.BAKEYFRAME_DTYPE)
    d_kf, d_mp, d_ed = _dev(ctx, kf), _dev(ctx, np.ascontiguousarray(c["mp"], P.MAPPOINT_DTYPE)), _dev(ctx, np.ascontiguousarray(c["edges"], P.BAEDGE_DTYPE))
    d_off = [_dev(ctx, np.array([0, n], np.int32)) for n in (nkf, M, len(c["edges"]))]
    d_er, d_info = _dev(ctx, np.zeros(len(c["edges"]), np.uint8)), _dev(ctx, np.zeros(1, P.BAINFO_DTYPE))
    ins = [_dev(ctx, a) for a in (off, okf, centres, ref_kf, ref_level)]
    P.Optimizer.LocalBundleAdjustmentDevice(wide, 1, d_kf, d_off[0], d_mp, d_off[1], d_ed, d_off[2], _cam(P, c["cam"]), 2, d_kf, d_mp, d_er, d_info)
    P.KeyFrameMatcher(ctx=ctx).update_normal_and_depth_device(d_mp, M, ins[0], ins[1], ins[2], nkf, ins[3], ins[4], 0, mc.SCALE)
    ctx.synchronize()
    got = _down(P, ctx, d_mp, np.zeros(M, P.MAPPOINT_DTYPE))
    for d in [d_kf, d_mp, d_ed, d_er, d_info] + d_off + ins:
        ctx.device_free(d)
    assert got.tobytes() == want.tobytes()
    assert want.tobytes() != np.ascontiguousarray(ref["mp"], P.MAPPOINT_DTYPE).tobytes()        # the second step did something


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/ba_main.cpp on pslfe.hpp: the batched device form (in place), the problem-by-problem host form and its own plain
    C++ loop, each against the restatement; a refused problem in the file as well"""
    exe = str(tmp_path / "ba_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "ba_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    names = [n for n in bc.CASE_NAMES if n not in ("threshold_ulps", "rounds_1")]
    cases = [bc.case(n) for n in names]
    dup = dict(cases[0], edges=np.concatenate([cases[0]["edges"], cases[0]["edges"][:1]]))
    dup["ref"] = bc.local_ba(dup["kf"], dup["mp"], dup["edges"], dup["cam"], 2)
    cases.insert(2, dup)
    for rounds, group in ((2, cases), (1, [bc.case("threshold_ulps"), bc.case("rounds_1")])):
        path, out = str(tmp_path / f"cases{rounds}.bin"), str(tmp_path / f"out{rounds}.bin")
        bc.write_cases(path, group, rounds, CAPS_WIDE)
        p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        for form, sec in zip(("loop", "device", "host"), bc.read_sections(out, group, 3)):
            for k, (g, c) in enumerate(zip(sec, group)):
                bc.assert_equal_ref(g, c["ref"], (form, rounds, k))
