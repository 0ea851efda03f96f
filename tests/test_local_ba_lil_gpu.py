"""GPU parity of LocalBundleAdjustmentAndInseclines (k_ba_local<true> of psl-slam_amd/csrc/pslfe_ba.hip) with the restatement of
tests/ba_lil_cases.py, bit for bit: poses, points, the 15 doubles of every LIL, both erase arrays, status, rounds, iterations and the
three chi2 values, for the kernel, the library's host form and the C++ consumer tools/dropin/ba_lil_main.cpp; launches of 1, 3 and 65
problems of unequal sizes with a refused one in the middle; zero LILs against pslfe_ba_local_device byte for byte; the error paths;
the chain into pslfe_pose_lil_edges_device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_cases as bc
import ba_lil_cases as lc
import pose_lil_cases as plc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("kf", "mp", "edges", "lil", "ledges")


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


def _dtypes(P):
    return (P.BAKEYFRAME_DTYPE, P.MAPPOINT_DTYPE, P.BAEDGE_DTYPE, P.MAPLIL_DTYPE, P.BALILEDGE_DTYPE)


@pytest.fixture(scope="module")
def wide():
    import psl_slam_amd as P
    ba = P.BundleAdjuster(65, *lc.CAPS_WIDE)
    yield ba
    ba.close()


def _run_device(P, ba, cases, rounds, alias=False, lil_form=True):
    """the cases as one launch -> [dict(info, kf, mp, erase, lil, erase_lil, nerased_lil)]; the erase bytes start as 0xAA, out-of-place
    outputs as zeros; every array has one row of padding at its end, so that no count of 0 makes an empty allocation"""
    ctx = ba.ctx
    K = len(cases)
    rows = [np.concatenate([np.ascontiguousarray(c[k], dt) for c in cases] + [np.zeros(1, dt)]) for k, dt in zip(KEYS, _dtypes(P))]
    o = [np.cumsum([0] + [len(c[k]) for c in cases]).astype(np.int32) for k in KEYS]
    d_in = [_dev(ctx, a) for a in rows]
    d_off = [_dev(ctx, a) for a in o]
    outs = [rows[0], rows[1], rows[3]]
    d_out = [d_in[0], d_in[1], d_in[3]] if alias else [_dev(ctx, np.zeros_like(a)) for a in outs]
    d_er, d_erl = _dev(ctx, np.full(len(rows[2]), 0xAA, np.uint8)), _dev(ctx, np.full(len(rows[4]), 0xAA, np.uint8))
    d_info, d_nel = _dev(ctx, np.zeros(K, P.BAINFO_DTYPE)), _dev(ctx, np.full(K, -7, np.int32))
    if lil_form:
        P.Optimizer.LocalBundleAdjustmentAndInseclinesDevice(ba, K, d_in[0], d_off[0], d_in[1], d_off[1], d_in[2], d_off[2], d_in[3], d_off[3], d_in[4],
                                                             d_off[4], _cam(P, cases[0]["cam"]), rounds, d_out[0], d_out[1], d_er, d_out[2], d_erl, d_nel,
                                                             d_info)
    else:
        P.Optimizer.LocalBundleAdjustmentDevice(ba, K, d_in[0], d_off[0], d_in[1], d_off[1], d_in[2], d_off[2], _cam(P, cases[0]["cam"]), rounds, d_out[0],
                                                d_out[1], d_er, d_info)
    ctx.synchronize()
    got = [_down(P, ctx, d, np.zeros_like(a)) for d, a in zip(d_out, outs)]
    er, erl = _down(P, ctx, d_er, np.zeros(len(rows[2]), np.uint8)), _down(P, ctx, d_erl, np.zeros(len(rows[4]), np.uint8))
    info, nel = _down(P, ctx, d_info, np.zeros(K, P.BAINFO_DTYPE)), _down(P, ctx, d_nel, np.zeros(K, np.int32))
    for d in {*d_in, *d_off, *d_out, d_er, d_erl, d_info, d_nel}:
        ctx.device_free(d)
    return [{"info": info[k], "kf": got[0][o[0][k]:o[0][k + 1]], "mp": got[1][o[1][k]:o[1][k + 1]], "erase": er[o[2][k]:o[2][k + 1]],
             "lil": got[2][o[3][k]:o[3][k + 1]], "erase_lil": erl[o[4][k]:o[4][k + 1]], "nerased_lil": int(nel[k])} for k in range(K)]


def _untouched(P, g, c, status):
    assert int(g["info"]["status"]) == status and int(g["info"]["rounds"]) == 0, g["info"]
    for k, key, dt in (("kf", "kf", P.BAKEYFRAME_DTYPE), ("mp", "mp", P.MAPPOINT_DTYPE), ("lil", "lil", P.MAPLIL_DTYPE)):
        assert g[k].tobytes() == np.ascontiguousarray(c[key], dt).tobytes(), k
    assert not g["erase"].any() and not g["erase_lil"].any() and g["nerased_lil"] == 0


def _refused(kind):
    base = lc.case("f2_x1_p8_l4")
    if kind == "dup":
        return dict(base, ledges=np.concatenate([base["ledges"], base["ledges"][2:3]]))
    c = dict(base, ledges=base["ledges"].copy())
    if kind == "outside_lil":
        c["ledges"]["lil"][3] = len(base["lil"])
    else:
        c["ledges"]["kf"][0] = len(base["kf"])
    return c


@pytest.mark.parametrize("name", lc.CASE_NAMES)
def test_device_and_host_forms_equal_restatement(name, wide):
    """2 + 1 keyframes / 6 points / 1 LIL with 2 edges; 4, 5 and 6 LILs; 5 + 3 / 40 / 8; the caps exactly, on a handle created with
    those caps; no map point; the edge cases; rounds = 1 - each through the kernel and the host form"""
    import psl_slam_amd as P
    c = lc.case(name)
    ba = P.BundleAdjuster(1, *lc.CAPS) if name == "caps_8_64_256_8_32" else wide
    try:
        got = _run_device(P, ba, [c], c["rounds"])[0]
        lc.assert_equal_ref(got, c["ref"], name)
        ko, mo, er, lo, el, info = P.Optimizer.LocalBundleAdjustmentAndInseclines(ba, c["kf"], c["mp"], c["edges"], c["lil"], c["ledges"], _cam(P, c["cam"]),
                                                                                  c["rounds"])
        lc.assert_equal_ref({"info": info, "kf": ko, "mp": mo, "erase": er, "lil": lo, "erase_lil": el}, c["ref"], name + " (host form)")
    finally:
        if ba is not wide:
            ba.close()


@pytest.mark.parametrize("K", [1, 3, 65])
def test_launches_of_unequal_problems_with_a_refused_one_in_the_middle(K, wide):
    """K problems of unequal sizes in one launch, out of place and in place; the middle one (K > 1) has a duplicate (LIL, keyframe) pair:
    it keeps its rows, its neighbours equal the restatement; a problem's result depends neither on its neighbours nor on its position"""
    import psl_slam_amd as P
    names = [n for n in lc.CASE_NAMES if n != "lil_rounds_1"]
    cases = [lc.case(names[(5 * k + 2) % len(names)]) for k in range(K)]
    mid = K // 2 if K > 1 else -1
    if mid >= 0:
        cases[mid] = _refused("dup")
    for alias in (False, True):
        got = _run_device(P, wide, cases, 2, alias=alias)
        for k, (g, c) in enumerate(zip(got, cases)):
            if k == mid:
                _untouched(P, g, c, bc.E_INVALID)
            else:
                lc.assert_equal_ref(g, c["ref"], (K, k, alias))
    rev = _run_device(P, wide, cases[::-1], 2)[::-1]
    for a, b in zip(rev, got):
        assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("kf", "mp", "erase", "lil", "erase_lil")) and a["nerased_lil"] == b["nerased_lil"]


@pytest.mark.parametrize("rounds", [2, 1])
def test_without_lils_the_bytes_are_those_of_the_point_form(rounds, wide):
    """every LIL count 0: pslfe_ba_local_lil_device writes what pslfe_ba_local_device writes, on a LIL handle and on a plain one"""
    import psl_slam_amd as P
    names = ["f1_x1_p6", "f2_x1_p8_mixed", "f5_x3_p40", "depth_only", "failed_solve", "failed_pivot", "point_drops_out", "keyframe_drops_out"]
    cases = [lc.without_lils(bc.case(n)) for n in names]
    plain = P.BundleAdjuster(len(cases), 16, 128, 512)
    try:
        want = _run_device(P, plain, cases, rounds, lil_form=False)
        for ba in (wide, plain):
            got = _run_device(P, ba, cases, rounds)
            for k, (g, w) in enumerate(zip(got, want)):
                for key in ("kf", "mp", "erase"):
                    assert g[key].tobytes() == w[key].tobytes(), (k, key)
                for f in ("status", "rounds", "iterations", "nerased", "chi2_start", "chi2_round1", "chi2_end"):
                    assert np.asarray(g["info"][f]).tobytes() == np.asarray(w["info"][f]).tobytes(), (k, f)
                assert g["nerased_lil"] == 0
                if rounds == 2:
                    bc.assert_equal_ref(g, bc.case(names[k])["ref"], names[k])
    finally:
        plain.close()


def test_refused_problems_keep_their_rows(wide):
    """LIL counts above the caps, a LIL edge that names a LIL or a keyframe outside its problem, a duplicate pair, and a handle from
    pslfe_ba_create given a LIL: the status, and all three outputs equal to the inputs; the neighbours equal the restatement"""
    import psl_slam_amd as P
    good = [lc.case(n) for n in ("f2_x1_p6_l1", "f5_x3_p40_l8")]
    many = lc.plant_lils(bc.make_scene(77, 2, 1, 8, "mono"), 77, lc.CAPS_WIDE[3] + 1, 2)                 # one LIL too many
    edgy = lc.plant_lils(bc.make_scene(78, 3, 1, 8, "mono"), 78, lc.CAPS_WIDE[3], 4)                     # 64 LIL edges: exactly the cap
    assert len(edgy["ledges"]) == lc.CAPS_WIDE[4]
    over = lc.plant_lils(bc.make_scene(79, 4, 1, 8, "mono"), 79, 13, 5)                                  # 65: one LIL edge too many
    assert len(over["ledges"]) == lc.CAPS_WIDE[4] + 1 and len(over["lil"]) <= lc.CAPS_WIDE[3]
    cases = [good[0], many, _refused("outside_lil"), good[1], _refused("outside_kf"), over, _refused("dup"), good[0]]
    want = [0, bc.E_CAPACITY, bc.E_INVALID, 0, bc.E_INVALID, bc.E_CAPACITY, bc.E_INVALID, 0]
    for alias in (False, True):
        got = _run_device(P, wide, cases, 2, alias=alias)
        for k, (g, c, st) in enumerate(zip(got, cases, want)):
            if st == 0:
                lc.assert_equal_ref(g, c["ref"], k)
            else:
                _untouched(P, g, c, st)
            r = lc.local_ba(c["kf"], c["mp"], c["edges"], c["lil"], c["ledges"], c["cam"], 2, caps=lc.CAPS_WIDE)
            assert int(r["info"]["status"]) == st
    g = _run_device(P, wide, [edgy], 2)[0]                                                                 # exactly at the LIL edge cap: runs
    assert int(g["info"]["status"]) == 0 and int(g["info"]["rounds"]) == 2
    with pytest.raises(P.PslfeError, match="-4"):
        P.Optimizer.LocalBundleAdjustmentAndInseclines(wide, many["kf"], many["mp"], many["edges"], many["lil"], many["ledges"], _cam(P, many["cam"]))
    d = _refused("dup")
    with pytest.raises(P.PslfeError, match="-1"):
        P.Optimizer.LocalBundleAdjustmentAndInseclines(wide, d["kf"], d["mp"], d["edges"], d["lil"], d["ledges"], _cam(P, d["cam"]))
    plain = P.BundleAdjuster(3, 16, 128, 512)                                                              # LIL caps of 0
    try:
        c = good[0]
        nolil = lc.without_lils(c)
        row_only = dict(nolil, lil=c["lil"])                                                               # a LIL row without an edge is a LIL too
        got = _run_device(P, plain, [c, nolil, row_only], 2)
        _untouched(P, got[0], c, bc.E_CAPACITY)
        _untouched(P, got[2], row_only, bc.E_CAPACITY)
        assert int(got[1]["info"]["status"]) == 0 and int(got[1]["info"]["rounds"]) == 2
    finally:
        plain.close()


def test_whole_call_errors_and_empty_launch(wide):
    import psl_slam_amd as P
    ctx = wide.ctx
    L = P.lib()
    cam = np.zeros(1, P.CAMERA_DTYPE)
    d, d2 = _dev(ctx, np.zeros(256, np.int32)), _dev(ctx, np.zeros(256, np.int32))          # inputs (all offsets 0) and outputs
    p, q, null = C.c_void_p(d), C.c_void_p(d2), C.c_void_p(None)
    f = L.pslfe_ba_local_lil_device
    names = ["kf", "kf_off", "mp", "mp_off", "edges", "edge_off", "lil", "lil_off", "lil_edges", "lil_edge_off"]
    outs = ["kf_out", "mp_out", "erase", "lil_out", "erase_lil", "nerased_lil", "info"]
    args = lambda **kw: [kw.get("ba", wide._h), C.c_int(kw.get("K", 1))] + [kw.get(n, p) for n in names] + [kw.get("cam", P._ptr(cam)), C.c_int(kw.get("rounds", 2))] + \
        [kw.get(n, q) for n in outs]
    assert f(*args(K=0)) == 0 and f(*args(K=0, ba=null, cam=null, kf=null, lil=null)) == 0     # K == 0: nothing is looked at
    assert f(*args(K=-1)) == -1 and f(*args(rounds=0)) == -1 and f(*args(rounds=3)) == -1
    assert f(*args(K=66)) == -1                                                               # above max_problems
    for k in ["ba", "cam"] + names + [n for n in outs if n != "nerased_lil"]:
        assert f(*args(**{k: null})) == -1, k
    assert f(*args(nerased_lil=null)) == 0                                                    # optional: all offsets 0, nothing to do
    ctx.synchronize()
    h = L.pslfe_ba_local_lil
    one, info = np.zeros(1, P.BAKEYFRAME_DTYPE), np.zeros(1, P.BAINFO_DTYPE)
    lil = np.zeros(1, P.MAPLIL_DTYPE)
    hargs = lambda nkf=1, nlil=0, lil=None, lil_out=None, rounds=2, info=P._ptr(info), ba=wide._h: [
        ba, P._ptr(one), C.c_int(nkf), None, C.c_int(0), None, C.c_int(0), lil, C.c_int(nlil), None, C.c_int(0), P._ptr(cam), C.c_int(rounds), P._ptr(one),
        None, None, lil_out, None, info]
    assert h(*hargs(nkf=-1)) == -1 and h(*hargs(nlil=-1)) == -1 and h(*hargs(nlil=1)) == -1 and h(*hargs(nlil=1, lil=P._ptr(lil))) == -1
    assert h(*hargs(rounds=5)) == -1 and h(*hargs(info=None)) == -1 and h(*hargs(ba=null)) == -1
    assert h(*hargs()) == 0 and info[0]["rounds"] == 0                                          # a keyframe and nothing else
    assert h(*hargs(nlil=1, lil=P._ptr(lil), lil_out=P._ptr(lil))) == 0 and info[0]["rounds"] == 0   # ... and a LIL without an edge
    c = L.pslfe_ba_create_lil
    out = C.c_void_p()
    assert c(ctx._h, 0, 1, 1, 1, 1, 1, C.byref(out)) == -1 and c(ctx._h, 1, 1, 1, 1, -1, 1, C.byref(out)) == -1 and c(ctx._h, 1, 1, 1, 1, 1, -1, C.byref(out)) == -1
    assert c(null, 1, 1, 1, 1, 1, 1, C.byref(out)) == -1
    ctx.device_free(d)
    ctx.device_free(d2)


def test_chain_into_pose_lil_edges(wide):
    """d_lil_out goes into pslfe_pose_lil_edges_device as d_map without a host copy: the edges are those the same rows give when they
    are copied through the host, and those of the restated set-up loop on the restated rows"""
    import psl_slam_amd as P
    ctx = wide.ctx
    c = lc.case("f5_x3_p40_l8")
    nlil = len(c["lil"])
    rng = np.random.default_rng(5)
    le_l = np.ascontiguousarray(np.concatenate([c["ledges"]["obs1"][:nlil], c["ledges"]["obs2"][:nlil]], 1))
    cross2d = np.ascontiguousarray(c["ledges"]["obs_ins"][:nlil])
    lil_index = rng.permutation(nlil).astype(np.int32)
    want, _ = plc.lil_edges(le_l, cross2d, lil_index, c["ref"]["lil"])
    rows = [np.ascontiguousarray(c[k], dt) for k, dt in zip(KEYS, _dtypes(P))]
    d_in = [_dev(ctx, a) for a in rows]
    d_off = [_dev(ctx, np.array([0, len(a)], np.int32)) for a in rows]
    d_er, d_erl, d_info = _dev(ctx, np.zeros(len(rows[2]), np.uint8)), _dev(ctx, np.zeros(len(rows[4]), np.uint8)), _dev(ctx, np.zeros(1, P.BAINFO_DTYPE))
    d_le, d_c2, d_np, d_idx = _dev(ctx, le_l), _dev(ctx, cross2d), _dev(ctx, np.array([nlil], np.int32)), _dev(ctx, lil_index)
    d_l, d_nl = _dev(ctx, np.zeros(nlil, P.POSELIL_DTYPE)), _dev(ctx, np.zeros(1, np.int32))
    P.Optimizer.LocalBundleAdjustmentAndInseclinesDevice(wide, 1, d_in[0], d_off[0], d_in[1], d_off[1], d_in[2], d_off[2], d_in[3], d_off[3], d_in[4], d_off[4],
                                                         _cam(P, c["cam"]), 2, d_in[0], d_in[1], d_er, d_in[3], d_erl, 0, d_info)
    P.Optimizer.LilEdgesDevice(1, d_le, nlil, d_c2, nlil, d_np, d_idx, d_in[3], nlil, d_l, 0, d_nl, nlil, ctx=ctx)
    ctx.synchronize()
    direct = _down(P, ctx, d_l, np.zeros(nlil, P.POSELIL_DTYPE))
    assert _down(P, ctx, d_nl, np.zeros(1, np.int32))[0] == nlil
    d_map = _dev(ctx, _down(P, ctx, d_in[3], np.zeros(nlil, P.MAPLIL_DTYPE)))          # the same rows through the host
    P.Optimizer.LilEdgesDevice(1, d_le, nlil, d_c2, nlil, d_np, d_idx, d_map, nlil, d_l, 0, d_nl, nlil, ctx=ctx)
    ctx.synchronize()
    through_host = _down(P, ctx, d_l, np.zeros(nlil, P.POSELIL_DTYPE))
    for x in d_in + d_off + [d_er, d_erl, d_info, d_le, d_c2, d_np, d_idx, d_l, d_nl, d_map]:
        ctx.device_free(x)
    assert direct.tobytes() == through_host.tobytes() == np.ascontiguousarray(want, P.POSELIL_DTYPE).tobytes()
    assert c["ref"]["lil"].tobytes() != c["lil"].tobytes()


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/ba_lil_main.cpp on pslfe.hpp, on a case file with LIL rows: the batched device form (in place), the problem-by-problem
    host form and its own plain C++ loop, each against the restatement; a refused problem in the file as well"""
    exe = str(tmp_path / "ba_lil_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "ba_lil_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    cases = [lc.case(n) for n in lc.CASE_NAMES if n != "lil_rounds_1"]
    dup = _refused("dup")
    dup["ref"] = lc.local_ba(dup["kf"], dup["mp"], dup["edges"], dup["lil"], dup["ledges"], dup["cam"], 2)
    cases.insert(2, dup)
    for rounds, group in ((2, cases), (1, [lc.case("lil_rounds_1")])):
        path, out = str(tmp_path / f"cases{rounds}.bin"), str(tmp_path / f"out{rounds}.bin")
        lc.write_cases(path, group, rounds, lc.CAPS_WIDE)
        p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        for form, sec in zip(("loop", "device", "host"), lc.read_sections(out, group, 3)):
            for k, (g, c) in enumerate(zip(sec, group)):
                lc.assert_equal_ref(g, c["ref"], (form, rounds, k))
