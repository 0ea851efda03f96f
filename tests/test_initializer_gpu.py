"""GPU parity of the monocular map initialisation (psl-slam_amd/csrc/pslfe_initializer.hip) with the restatement of
tests/initializer_cases.py, bit for bit: status, scores, both winning iterations, H, F, every nGood and parallax, R, t, every point and
flag, mvIniMatches; the host-array form and the Python mirror; a batch of 67 pairs against single launches; strides above the counts;
the error paths; the frame-slot form behind the monocular Frame constructor and SearchForInitialization; the C++ consumer
tools/dropin/init_main.cpp on the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import initializer_cases as ic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _dev(ctx, a):
    return ctx.device_array(a)[0]


def _down(P, ctx, d, a):
    P._check(P.lib().pslfe_device_download(ctx._h, P._ptr(a), C.c_void_p(d), C.c_size_t(a.nbytes)), "pslfe_device_download")
    return a


def _cam_rec(P, cam=ic.CAM):
    rec = np.zeros((), P.CAMERA_DTYPE)
    for k, v in cam.items():
        rec[k] = v
    return rec


def _launch(P, ctx, cases, kstride=None, mstride=None, counts=None, key_floats=2, max_its=None, seed0=None, want_out=True):
    """one launch over the pairs; every output starts as 0xAA -> ([dict(res, p3d, tri, ini) over the full strides], untouched beyond)"""
    K = len(cases)
    kstride = kstride if kstride is not None else max(max(len(c["keys1"]), len(c["keys2"])) for c in cases)
    mstride = mstride if mstride is not None else max(len(c["keys1"]) for c in cases)
    k1, k2 = np.full((K, max(kstride, 1), key_floats), 7.5, F), np.full((K, max(kstride, 1), key_floats), 7.5, F)
    m = np.full((K, max(mstride, 1)), -1, np.int32)
    n1, n2 = np.zeros(K, np.int32), np.zeros(K, np.int32)
    for k, c in enumerate(cases):
        a, b = min(len(c["keys1"]), kstride), min(len(c["keys2"]), kstride)
        k1[k, :a, :2], k2[k, :b, :2] = c["keys1"][:a], c["keys2"][:b]
        mm = min(len(c["matches"]), mstride)
        m[k, :mm] = c["matches"][:mm]
        n1[k], n2[k] = (len(c["keys1"]), len(c["keys2"])) if counts is None else counts[k]
    res = np.zeros(K, P.INITRESULT_DTYPE)
    res.view(np.uint8)[:] = 0xAA
    ms = max(mstride, 1)
    bufs = [_dev(ctx, a) for a in (k1, k2, n1, n2, m, res, np.full((K, ms * 12), 0xAA, np.uint8), np.full((K, ms), 0xAA, np.uint8),
                                   np.full((K, ms * 4), 0xAA, np.uint8))]
    d_k1, d_k2, d_n1, d_n2, d_m, d_res, d_p3d, d_tri, d_ini = bufs
    its = max_its if max_its is not None else cases[0]["max_its"]
    P.Initializer.InitializeDevice(K, d_k1, d_n1, d_k2, d_n2, 4 * key_floats, kstride, d_m, mstride, _cam_rec(P, cases[0].get("cam", ic.CAM)), d_res, d_p3d, d_tri,
                                   d_ini if want_out else 0, sigma=cases[0]["sigma"], iterations=its,
                                   seed0=cases[0]["seed"] if seed0 is None else seed0, ctx=ctx)
    ctx.synchronize()
    res = _down(P, ctx, d_res, res)
    p3d = _down(P, ctx, d_p3d, np.zeros((K, max(mstride, 1), 3), F))
    tri = _down(P, ctx, d_tri, np.zeros((K, max(mstride, 1)), np.uint8))
    ini = _down(P, ctx, d_ini, np.zeros((K, max(mstride, 1)), np.int32))
    for d in bufs:
        ctx.device_free(d)
    return [dict(res=res[k], p3d=p3d[k], tri=tri[k], ini=ini[k]) for k in range(K)]


_AA32 = np.frombuffer(b"\xaa" * 4, np.int32)[0]


def _untouched(g, n):
    """nothing beyond the first n entries of the pair's outputs was written"""
    return bool((g["p3d"][n:].view(np.uint8) == 0xAA).all() and (g["tri"][n:] == 0xAA).all() and (g["ini"][n:] == _AA32).all())


def _head(g, n):
    return dict(res=g["res"], p3d=g["p3d"][:n], tri=g["tri"][:n], ini=g["ini"][:n])


@pytest.mark.parametrize("name", ic.CASE_NAMES)
def test_device_host_and_mirror_forms_equal_restatement(name):
    """the match counts 7 / 8 / 9 / 63 / 64 / 65 / the LDS row limit and past it, -1 holes under many keypoints, the iteration budgets
    1 / 15 / 16 / 17 / 200, and the scenes; strides above the counts leave the bytes beyond the counts untouched"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = ic.case(name)
    n1 = len(c["keys1"])
    g = _launch(P, ctx, [c], kstride=max(n1, len(c["keys2"])) + 5, mstride=n1 + 3)[0]
    ic.assert_same(_head(g, n1), c["ref"], name + " device")
    assert _untouched(g, n1)
    g7 = _launch(P, ctx, [c], key_floats=7, want_out=False)[0]            # the keypoint records of a frame slot: 28 bytes apart
    ic.assert_same(_head(g7, n1), c["ref"], name + " stride 28", ini=False)
    assert (g7["ini"] == _AA32).all()
    init = P.Initializer(c["keys1"], _cam_rec(P, c["cam"]), c["sigma"], c["max_its"], seed=c["seed"], ctx=ctx)
    ok, R21, t21, p3d, tri = init.Initialize(c["keys2"], c["matches"])
    ref = c["ref"]
    ic.assert_same(dict(res=init.result, p3d=p3d, tri=tri.astype(np.uint8), ini=ref["ini"]), ref, name + " mirror")
    assert ok == bool(ref["res"]["status"] & 1) and ic.same_floats(R21, ref["res"]["R21"]) and ic.same_floats(t21, ref["res"]["t21"])


def test_selection_and_nan_order_on_the_device():
    """the kernel's ordered keys and its radix selection alone: the stated order of a NaN in vCosParallax (sign bit set below -inf, clear
    above +inf), NaNs of both signs and both infinities among the cosines, 1 / 16 / 300 and more elements"""
    import psl_slam_amd as P
    keys, sel, _ = P.Initializer.DebugSelect(ic.ORDERED)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (keys == ic.cos_key(np.array(ic.ORDERED, F))).all()
    for v, want in ic.selection_cases():
        keys, sel, par = P.Initializer.DebugSelect(v)
        assert (keys == ic.cos_key(np.array(v, F))).all()
        assert np.array(sel, F).view(np.uint32) == np.array(want, F).view(np.uint32), (len(v), sel, want)
        assert ic.same_floats(par, ic.parallax_of(want))


def test_empty_frames_through_the_host_form():
    """no reference keypoints, no current keypoints, neither: zero-length uploads and NULL arrays; status 0, nothing matched"""
    import psl_slam_amd as P
    ctx = P.default_context()
    c = ic.case("n9")
    for k1, k2, m in ((np.zeros((0, 2), F), c["keys2"], np.zeros(0, np.int32)),
                      (c["keys1"], np.zeros((0, 2), F), np.full(len(c["keys1"]), -1, np.int32)),
                      (np.zeros((0, 2), F), np.zeros((0, 2), F), np.zeros(0, np.int32))):
        init = P.Initializer(k1, _cam_rec(P), 1.0, 8, seed=1, ctx=ctx)
        ok, R21, t21, p3d, tri = init.Initialize(k2, m)
        ref = ic.initialize(k1, k2, m, ic.CAM, 1.0, 8, 1)
        ic.assert_same(dict(res=init.result, p3d=p3d, tri=tri.astype(np.uint8), ini=ref["ini"]), ref, "empty %d %d" % (len(k1), len(k2)))
        assert not ok and init.result["status"] == 0 and init.result["nmatches"] == 0 and len(p3d) == len(k1) and not R21.any()
    with pytest.raises(P.PslfeError):                                    # a match with no frame 2 to point into
        P.Initializer(c["keys1"], _cam_rec(P), 1.0, 8, ctx=ctx).Initialize(np.zeros((0, 2), F), c["matches"])


def test_batch_of_67_equals_single_launches():
    """pairs of different sizes and outcomes in one launch, pair p seeded seed0 + p"""
    import psl_slam_amd as P
    ctx = P.default_context()
    names = ["general", "n7", "planar", "n530", "holes", "rotation", "identical", "n65", "few", "lowpar", "noisy"]
    cases = [dict(ic.case(names[p % len(names)])) for p in range(67)]
    got = _launch(P, ctx, cases, max_its=17, seed0=100)
    st = set()
    for p, (c, g) in enumerate(zip(cases, got)):
        n1 = len(c["keys1"])
        one = _launch(P, ctx, [c], max_its=17, seed0=100 + p)[0]
        ic.assert_same(_head(g, n1), _head(one, n1), "pair %d" % p)
        assert _untouched(g, n1)
        st.add(int(g["res"]["status"]))
    assert {0, 1, 2, 4} <= st
    for p in (0, 13, 66):                                                # and the restatement with that seed
        c = cases[p]
        ref = ic.initialize(c["keys1"], c["keys2"], c["matches"], ic.CAM, c["sigma"], 17, 100 + p)
        ic.assert_same(_head(got[p], len(c["keys1"])), ref, "pair %d against the restatement" % p)


def test_errors_are_reported_and_nothing_is_written():
    import psl_slam_amd as P
    ctx = P.default_context()
    good, other = ic.case("n65"), ic.case("n9")
    n1, n2 = len(good["keys1"]), len(good["keys2"])
    bad_match = dict(good, matches=good["matches"].copy())
    bad_match["matches"][3] = n2                                         # a match outside frame 2
    cases = [good, good, good, good, bad_match, other]
    counts = [(-1, n2), (n1, -2), (n1 + 50, n2), (n1, n2 + 50), (n1, n2), (len(other["keys1"]), len(other["keys2"]))]
    got = _launch(P, ctx, cases, kstride=n1 + 10, mstride=n1 + 10, counts=counts, seed0=(other["seed"] - 5) & 0xffffffff)   # pair 5: its own seed
    want = [ic.E_INVALID, ic.E_INVALID, ic.E_CAPACITY, ic.E_CAPACITY, ic.E_INVALID]
    for k, w in enumerate(want):
        rec = np.zeros((), P.INITRESULT_DTYPE)
        rec["status"] = w
        assert got[k]["res"].tobytes() == rec.tobytes(), k                # the status alone, the other fields 0
        assert _untouched(got[k], 0), k                                   # no output byte of that pair
    ic.assert_same(_head(got[5], len(other["keys1"])), other["ref"], "the good pair of the batch")
    # a count above mstride alone
    g = _launch(P, ctx, [good], kstride=n1 + 10, mstride=n1 - 1)[0]
    assert g["res"]["status"] == ic.E_CAPACITY and _untouched(g, 0)
    L, cam = P.lib(), _cam_rec(P).reshape(1)
    one = C.c_void_p(8)                                                   # never dereferenced: the checks come first
    args = lambda **kw: [kw.get("ctx", ctx._h), C.c_int(kw.get("npairs", 1)), one, one, one, one, C.c_int(kw.get("kb", 8)),  # noqa: E731
                         C.c_int(kw.get("kstride", 4)), one, C.c_int(kw.get("mstride", 4)), P._ptr(cam), C.c_float(kw.get("sigma", 1.0)),
                         C.c_int(kw.get("its", 10)), C.c_uint32(0), kw.get("res", one), one, one, None]
    for kw in (dict(npairs=-1), dict(kstride=-1), dict(mstride=-1), dict(its=0), dict(sigma=float("nan")), dict(kb=6), dict(kb=4),
               dict(res=None), dict(ctx=None)):
        assert L.pslfe_init_initialize_device(*args(**kw)) == ic.E_INVALID, kw
    assert L.pslfe_init_initialize_device(*args(npairs=0, its=5)) == 0    # nothing is done
    with pytest.raises(P.PslfeError):
        P.Initializer(bad_match["keys1"], cam, 1.0, 10, ctx=ctx).Initialize(bad_match["keys2"], bad_match["matches"])
    with pytest.raises(P.PslfeError):
        P.Initializer(good["keys1"], cam, 1.0, 0, ctx=ctx).Initialize(good["keys2"], good["matches"])


def test_frame_slot_form_behind_the_constructor_and_the_search():
    """two synthetic images through the extractor, the monocular Frame constructor and SearchForInitialization on the device,
    then pslfe_init_initialize_frames_device on the slots: equal to the array form fed with the fetched mvKeysUn and matches, and to the
    restatement on them; d_matches12_out equals src/Tracking.cc:712-719"""
    import torch
    import psl_slam_amd as P
    import synth_frames as sf
    w, h = 640, 480
    dev = torch.device("cuda", 0)
    ctx = P.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    cam = np.zeros((), P.CAMERA_DTYPE)
    cam["fx"], cam["fy"], cam["cx"], cam["cy"] = 520.0, 520.0, 319.5, 239.5
    sc = sf.Scene(w, h, "desk", 7)
    imgs = np.ascontiguousarray(np.stack([sc.gray(0), sc.gray(2)]))
    orb = P.ORBextractor(1000, 1.2, 8, 20, 7, ctx=ctx, max_batch=2)
    orb.extract_batch(imgs)
    cap = orb.max_keypoints(w, h)
    G = P.FrameGrid(cap, 2, ctx=ctx)
    G.set_from_orb_mono(0, orb, 0, 2, cam)
    k1, k2 = G.fetch(0)[0], G.fetch(1)[0]
    n1 = len(k1)
    prev = np.zeros((2, cap, 2), F)
    prev[:, :n1, 0], prev[:, :n1, 1] = k1["x"], k1["y"]
    d_prev = torch.from_numpy(prev).to(dev)
    mm = torch.full((2, cap), -1, dtype=torch.int32, device=dev)
    nn = torch.zeros(2, dtype=torch.int32, device=dev)
    s1, s2 = np.zeros(2, np.int32), np.array([1, 0], np.int32)          # pair 1: the frame against itself
    P.search_for_initialization_device(G, s1, G, s2, d_prev.data_ptr(), cap, mm.data_ptr(), nn.data_ptr())
    res = torch.zeros(2 * P.INITRESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    p3d = torch.full((2, cap, 3), 7.0, dtype=torch.float32, device=dev)
    tri = torch.full((2, cap), 0xAA, dtype=torch.uint8, device=dev)
    ini = torch.full((2, cap), -7, dtype=torch.int32, device=dev)
    P.Initializer.InitializeFramesDevice(G, s1, G, s2, mm.data_ptr(), cap, cam, res.data_ptr(), p3d.data_ptr(), tri.data_ptr(), ini.data_ptr(),
                                         iterations=32, seed0=5)
    torch.cuda.synchronize(dev)
    M, R = mm.cpu().numpy(), res.cpu().numpy().view(P.INITRESULT_DTYPE)
    P3, TR, INI = p3d.cpu().numpy(), tri.cpu().numpy(), ini.cpu().numpy()
    assert nn.cpu().numpy().min() >= 8
    xy = [np.ascontiguousarray(np.stack([k["x"], k["y"]], 1).astype(F)) for k in (k1, k2)]
    camd = dict(fx=520.0, fy=520.0, cx=319.5, cy=239.5)
    for p in range(2):
        keys2 = xy[int(s2[p])]
        got = dict(res=R[p], p3d=P3[p, :n1], tri=TR[p, :n1], ini=INI[p, :n1])
        ref = ic.initialize(xy[0], keys2, M[p, :n1], camd, 1.0, 32, 5 + p)
        ic.assert_same(got, ref, "frames pair %d against the restatement" % p)
        assert (P3[p, n1:] == 7.0).all() and (TR[p, n1:] == 0xAA).all() and (INI[p, n1:] == -7).all()
        c = dict(keys1=xy[0], keys2=keys2, matches=M[p, :n1].copy(), max_its=32, sigma=1.0, seed=5 + p)
        arr = _launch_cam(P, ctx, c, cam)
        ic.assert_same(got, _head(arr, n1), "frames pair %d against the array form" % p)
    assert R[1]["status"] in (2, 0) and not (R[1]["status"] & 1)        # no baseline: never an initialisation
    with pytest.raises(P.PslfeError):
        P.Initializer.InitializeFramesDevice(G, s1, G, s2, mm.data_ptr(), cap - 1, cam, res.data_ptr(), p3d.data_ptr(), tri.data_ptr(), 0)
    G2 = P.FrameGrid(cap, 3, ctx=ctx)
    with pytest.raises(P.PslfeError):                                    # a slot that was never set
        P.Initializer.InitializeFramesDevice(G2, s1, G2, s2, mm.data_ptr(), cap, cam, res.data_ptr(), p3d.data_ptr(), tri.data_ptr(), 0)


def _launch_cam(P, ctx, c, cam):
    """the array form with another camera than the cases'"""
    n1, n2 = len(c["keys1"]), len(c["keys2"])
    ks = max(n1, n2)
    k1, k2 = np.zeros((ks, 2), F), np.zeros((ks, 2), F)
    k1[:n1], k2[:n2] = c["keys1"], c["keys2"]
    bufs = [_dev(ctx, a) for a in (k1, k2, np.array([n1], np.int32), np.array([n2], np.int32), c["matches"], np.zeros(1, P.INITRESULT_DTYPE),
                                   np.zeros((n1, 3), F), np.zeros(n1, np.uint8), np.zeros(n1, np.int32))]
    P.Initializer.InitializeDevice(1, bufs[0], bufs[2], bufs[1], bufs[3], 8, ks, bufs[4], n1, cam, bufs[5], bufs[6], bufs[7], bufs[8],
                                   sigma=c["sigma"], iterations=c["max_its"], seed0=c["seed"], ctx=ctx)
    ctx.synchronize()
    out = dict(res=_down(P, ctx, bufs[5], np.zeros(1, P.INITRESULT_DTYPE))[0], p3d=_down(P, ctx, bufs[6], np.zeros((n1, 3), F)),
               tri=_down(P, ctx, bufs[7], np.zeros(n1, np.uint8)), ini=_down(P, ctx, bufs[8], np.zeros(n1, np.int32)))
    for d in bufs:
        ctx.device_free(d)
    return out


def test_cpp_consumer_equals_restatement(tmp_path):
    """tools/dropin/init_main.cpp linked with the library: pslfe::Initializer prints the same record as its own plain C++ loop, and
    both equal the restatement"""
    import psl_slam_amd as P
    exe = str(tmp_path / "init_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "dropin", "init_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    cases = [ic.case(nm) for nm in ic.CASE_NAMES]
    path, out = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    ic.write_cases(path, cases, P.CAMERA_DTYPE)
    p = subprocess.run([exe, path, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    with open(out, "rb") as f:
        loop, mirror = ic.read_section(f, cases), ic.read_section(f, cases)
        assert f.read() == b""
    for nm, c, a, b in zip(ic.CASE_NAMES, cases, loop, mirror):
        ic.assert_same(a, c["ref"], nm + " loop")
        ic.assert_same(b, c["ref"], nm + " mirror")
        assert a["res"].tobytes() == b["res"].tobytes() or np.isnan(a["res"]["RH"]), nm
