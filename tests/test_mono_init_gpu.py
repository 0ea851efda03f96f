"""GPU parity of the monocular Frame constructor (pslfe_frame_set_from_orb_mono) and ORBmatcher::SearchForInitialization
(pslfe_orb_search_for_initialization / _device) against the CPU oracle's undistortion and the sequential restatement
oracle/mono_init_oracle.cpp (itself checked against a numpy transcription of the reference in tests/test_mono_init_cpu.py)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import synth_frames as sf
from mono_init_cases import BOUNDS, Case, constructed, one_tenth, random_pair, stolen_decides
from oracle_lib import restate_grid, restate_search

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_CAPACITY, E_STATE = -1, -4, -5
# Examples/Monocular/TUM1.yaml (k1 != 0) and KITTI00-02.yaml (no distortion)
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0)
PLAIN = (517.306408, 516.469215, 318.643040, 255.313989, 0, 0, 0, 0, 0, 40.0)
KITTI = (718.856, 718.856, 607.1928, 185.2157, 0, 0, 0, 0, 0, 386.1448)


def camera(vals):
    import psl_slam_amd as P
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, vals):
        cam[k] = np.float32(v)
    return cam


def sequence(w, h, n, seed=7):
    sc = sf.Scene(w, h, "desk", seed)
    return [sc.gray(t) for t in range(n)]


def xy(k):
    return np.ascontiguousarray(np.stack([k["x"], k["y"]], 1).astype(np.float32))


@pytest.mark.parametrize("cam_vals", [TUM1, PLAIN], ids=["tum1", "plain"])
def test_constructor_equals_rgbd_undistortion_and_grid(cam_vals):
    """mvKeysUn equal to the RGB-D path's undistortion, mvDepth = mvuRight = -1, the grid equal to the restatement's; empty frames
    (first and in the middle) give n = 0 and an empty grid."""
    import psl_slam_amd as P
    import oracle_lib
    w, h = 640, 480
    cam = camera(cam_vals)
    flat = np.full((h, w), 128, np.uint8)
    imgs = [flat] + sequence(w, h, 3) + [flat]
    imgs.insert(2, flat)
    orb = P.ORBextractor(2000, 1.2, 8, 20, 7, max_batch=len(imgs))
    orb.extract_batch(np.ascontiguousarray(np.stack(imgs)))
    g = P.FrameGrid(orb.max_keypoints(w, h), len(imgs) + 2)
    g.set_from_orb_mono(2, orb, 0, len(imgs), cam)
    bounds = oracle_lib.image_bounds(cam, w, h)
    assert (bounds == g.image_bounds(cam, w, h)).all()
    for t in range(len(imgs)):
        k, _ = orb.fetch(t, w, h)
        kun, dep, ur = g.fetch(2 + t)
        start, gidx = g.debug_grid(2 + t)
        if imgs[t] is flat:
            assert len(k) == 0 and len(kun) == 0 and (start == 0).all() and len(gidx) == 0
            continue
        assert len(k) > 500
        want, _, _ = oracle_lib.frame_post_rgbd(k, np.zeros((h, w), np.float32), cam)
        assert kun.tobytes() == want.tobytes(), f"frame {t}: mvKeysUn differs"
        assert (dep == -1).all() and (ur == -1).all()
        rs, ri = restate_grid(want, bounds)
        assert start.tobytes() == rs.tobytes() and gidx.tobytes() == ri.tobytes(), f"frame {t}: grid differs"
        if cam_vals is TUM1:
            assert kun.tobytes() != k.tobytes()


def _chain(g, f1_slot, k1un, d1, frames, bounds, set_f2):
    """prev chained over the frames against one initial frame: the library's host path vs the restatement."""
    import psl_slam_amd as P
    m = P.ORBmatcher(0.9, True)
    prev, rprev = xy(k1un), xy(k1un)
    counts = []
    for t, fr in enumerate(frames):
        k2un, d2 = set_f2(fr)
        nm, m12 = m.SearchForInitialization(g, f1_slot, g, 1, prev, 100)
        rnm, rm12, rprev, _ = restate_search(k1un, d1, k2un, d2, bounds, rprev, 100, 0.9, True)
        assert nm == rnm and (m12 == rm12).all(), f"frame {t}: matches differ ({nm} vs {rnm})"
        assert prev.tobytes() == rprev.tobytes(), f"frame {t}: prev differs"
        counts.append(nm)
    return counts


def test_single_pair_chain_tum():
    """TUM1 640x480, the initialiser's 2000 features, prev chained over 6 frames against frame 0."""
    import psl_slam_amd as P
    import oracle_lib
    w, h = 640, 480
    cam = camera(TUM1)
    imgs = sequence(w, h, 7, seed=3)
    orb = P.ORBextractor(2000, 1.2, 8, 20, 7)
    g = P.FrameGrid(orb.max_keypoints(w, h), 2)
    _, d1 = orb(imgs[0])
    g.set_from_orb_mono(0, orb, 0, 1, cam)
    k1un = g.fetch(0)[0]

    def set_f2(img):
        _, d2 = orb(img)
        g.set_from_orb_mono(1, orb, 0, 1, cam)
        return g.fetch(1)[0], d2
    counts = _chain(g, 0, k1un, d1, imgs[1:], oracle_lib.image_bounds(cam, w, h), set_f2)
    assert counts[0] > 100, counts


def test_single_pair_chain_kitti_4000():
    """KITTI 1241x376 with 4000 initialiser features: the device extractor refuses them (a level quota above its 512-node octree,
    PSLFE_E_INVALID), so the keypoints come from the CPU oracle of the extractor through pslfe_frame_set."""
    import psl_slam_amd as P
    import oracle_lib
    w, h = 1241, 376
    o = P.ORBextractor(4000, 1.2, 8, 20, 7)
    assert P.lib().pslfe_orb_max_keypoints(o._h, w, h) == E_INVALID
    imgs = sequence(w, h, 6, seed=5)
    orc = oracle_lib.OracleORB(4000, 1.2, 8, 20, 7)
    bounds = (0.0, 0.0, float(w), float(h))
    k1, d1 = orc(imgs[0])
    assert 2000 < len(k1) <= 4096
    g = P.FrameGrid(4096, 2)
    g.set(0, k1, d1, bounds)

    def set_f2(img):
        k2, d2 = orc(img)
        g.set(1, k2, d2, bounds)
        return k2, d2
    counts = _chain(g, 0, k1, d1, imgs[1:], bounds, set_f2)
    assert counts[0] > 100, counts


def _host_case(k1, d1, k2, d2, prev, window, nnratio=0.9, check_ori=True, cap=None):
    import psl_slam_amd as P
    g = P.FrameGrid(cap or max(len(k1), len(k2), 1), 2)
    g.set(0, k1, d1, BOUNDS)
    g.set(1, k2, d2, BOUNDS)
    pv = np.ascontiguousarray(prev, np.float32).copy()
    nm, m12 = P.ORBmatcher(nnratio, check_ori).SearchForInitialization(g, 0, g, 1, pv, window)
    want = restate_search(k1, d1, k2, d2, BOUNDS, prev, window, nnratio, check_ori)
    assert nm == want[0] and (m12 == want[1]).all() and pv.tobytes() == want[2].tobytes()
    return want


def rewalk(c):
    """Ten F2 keypoints in one window with disjoint bit sets P_j of 10 + j bits; nine earlier queries E_j = P_j take keypoints
    0..8 at distance 0; the last query (no bits) is at 10 + j from keypoint j, so its eight cached candidates are all held and the
    window holds ten: only the re-walk finds keypoint 9 (distance 19, the single survivor)."""
    off, P = 0, []
    for j in range(10):
        b = np.zeros(256, np.uint8)
        b[off:off + 10 + j] = 1
        off += 10 + j
        P.append(np.packbits(b))
    ks = [c.f2(200 + j, 200, P[j]) for j in range(10)]
    for j in range(9):
        c.f1(200 + j, 200, P[j])
    return c.f1(205, 200, np.zeros(32, np.uint8)), ks


@pytest.mark.parametrize("check_ori", [True, False])
def test_adversarial_pairs(check_ori):
    rng = np.random.default_rng(21)
    c = Case()
    constructed(c, rng)
    k1, d1, k2, d2, prev = c.arrays()
    for nnratio in (0.9, 1.5):
        _host_case(k1, d1, k2, d2, prev, 20, nnratio, check_ori)
    c = Case()
    q, ks = rewalk(c)
    want = _host_case(*c.arrays(), 20, 0.9, check_ori)
    assert want[1][q] == ks[9] and want[0] == 10
    c = Case()
    A, B, kA, CD = stolen_decides(c, rng)
    want = _host_case(*c.arrays(), 10, 0.9, check_ori)
    if check_ori:
        assert want[1][A] == -1 and want[1][B] == kA and all(want[1][q] >= 0 for q in CD)
    c = Case()
    one_tenth(c, rng)
    _host_case(*c.arrays(), 10, 0.9, check_ori)


def test_full_capacity_and_empty_f2():
    """4096 octave-0 keypoints in F2 (the frame store's capacity, 16-bit candidate positions at their limit), and an empty F2."""
    rng = np.random.default_rng(5)
    k1, d1, k2, d2, prev = random_pair(rng, 4096, 4096, p0=1.0)
    want = _host_case(k1, d1, k2, d2, prev, 100, cap=4096)
    assert want[0] > 100
    k1, d1, _, _, prev = random_pair(rng, 300, 300)
    e = np.zeros(0, k1.dtype)
    want = _host_case(k1, d1, e, np.zeros((0, 32), np.uint8), prev, 100)
    assert want[0] == 0 and (want[1] == -1).all() and want[2].tobytes() == prev.tobytes()


def test_batch_equals_per_pair_calls():
    """257 pairs in one device call, F1 and F2 in one store (f1 == f2) and in two stores, against the per-pair host calls and the
    restatement; then a device-resident chain (batch extraction -> set_from_orb_mono -> _device search) against the host path."""
    import torch
    import psl_slam_amd as P
    import oracle_lib
    w, h, N, K = 640, 480, 257, 8
    dev = torch.device("cuda", 0)
    ctx = P.Context(0, torch.cuda.current_stream(dev).cuda_stream)
    cam = camera(TUM1)
    imgs = np.ascontiguousarray(np.stack(sequence(w, h, K + 1, seed=11)))
    orb = P.ORBextractor(2000, 1.2, 8, 20, 7, ctx=ctx, max_batch=K + 1)
    res = orb.extract_batch(imgs)
    cap = orb.max_keypoints(w, h)
    G = P.FrameGrid(cap, K + 1, ctx=ctx)             # slot 0 = F1, slots 1..K = F2
    G.set_from_orb_mono(0, orb, 0, K + 1, cam)
    GA, GB = P.FrameGrid(cap, 1, ctx=ctx), P.FrameGrid(cap, K, ctx=ctx)
    GA.set_from_orb_mono(0, orb, 0, 1, cam)
    GB.set_from_orb_mono(0, orb, 1, K, cam)
    k1un = G.fetch(0)[0]
    n1 = len(k1un)
    base = np.zeros((N, cap, 2), np.float32)
    for p in range(N):
        base[p, :n1] = xy(k1un) + np.float32(p % 7) * np.float32(3.0)
    s2 = np.array([1 + p % K for p in range(N)], np.int32)
    d_prev1, d_prev2 = torch.from_numpy(base).to(dev), torch.from_numpy(base).to(dev)
    m1 = torch.full((N, cap), -7, dtype=torch.int32, device=dev)
    m2 = torch.full((N, cap), -7, dtype=torch.int32, device=dev)
    nm1 = torch.zeros(N, dtype=torch.int32, device=dev)
    nm2 = torch.zeros(N, dtype=torch.int32, device=dev)
    P.search_for_initialization_device(G, np.zeros(N, np.int32), G, s2, d_prev1.data_ptr(), cap, m1.data_ptr(), nm1.data_ptr())
    P.search_for_initialization_device(GA, np.zeros(N, np.int32), GB, s2 - 1, d_prev2.data_ptr(), cap, m2.data_ptr(), nm2.data_ptr())
    torch.cuda.synchronize(dev)
    PV1, PV2, M1, M2, NM1, NM2 = (t.cpu().numpy() for t in (d_prev1, d_prev2, m1, m2, nm1, nm2))
    assert PV1.tobytes() == PV2.tobytes() and (M1 == M2).all() and (NM1 == NM2).all()
    assert (M1[:, n1:] == -7).all() and (PV1[:, n1:] == 0).all()     # nothing past F1's keypoints is written
    bounds = oracle_lib.image_bounds(cam, w, h)
    m = P.ORBmatcher(0.9, True)
    for p in sorted({0, 1, 7, 8, 100, N // 2, N - 2, N - 1}):
        pv = np.ascontiguousarray(base[p, :n1]).copy()
        nm, m12 = m.SearchForInitialization(G, 0, G, int(s2[p]), pv, 100)
        assert nm == NM1[p] and (m12 == M1[p, :n1]).all() and pv.tobytes() == PV1[p, :n1].tobytes(), f"pair {p}: batch vs host"
        k2un = G.fetch(int(s2[p]))[0]
        rnm, rm12, rpv, _ = restate_search(k1un, res[0][1], k2un, res[int(s2[p])][1], bounds, base[p, :n1], 100, 0.9, True)
        assert rnm == nm and (rm12 == m12).all() and rpv.tobytes() == pv.tobytes(), f"pair {p}: batch vs restatement"
    assert NM1.min() > 50

    # device-resident chain: no distortion, so prev starts from the extractor's own keypoints on the device
    plain = camera(PLAIN)
    d_img = torch.from_numpy(imgs).to(dev)
    orb.extract_batch_device(d_img.data_ptr(), K + 1, w, h, w, w * h)
    G.set_from_orb_mono(0, orb, 0, K + 1, plain)
    kv, _, _, _ = P.orb_results_as_arrays(orb, K + 1)
    kp = torch.as_tensor(kv, device=dev)
    d_prev = kp[0:1, :, 0:2].repeat(K, 1, 1).contiguous()
    mm = torch.full((K, cap), -1, dtype=torch.int32, device=dev)
    nn = torch.zeros(K, dtype=torch.int32, device=dev)
    P.search_for_initialization_device(G, np.zeros(K, np.int32), G, np.arange(1, K + 1, dtype=np.int32), d_prev.data_ptr(), cap,
                                       mm.data_ptr(), nn.data_ptr())
    torch.cuda.synchronize(dev)
    MM, NN, DP = mm.cpu().numpy(), nn.cpu().numpy(), d_prev.cpu().numpy()
    k0 = G.fetch(0)[0]
    for t in range(K):
        pv = xy(k0)
        nm, m12 = m.SearchForInitialization(G, 0, G, t + 1, pv, 100)
        assert nm == NN[t] and (m12 == MM[t, :len(k0)]).all() and pv.tobytes() == DP[t, :len(k0)].tobytes(), f"chain pair {t}"
    ctx.synchronize()


def test_error_paths():
    import psl_slam_amd as P
    L = P.lib()
    cam = np.ascontiguousarray(camera(TUM1)).reshape(1)
    img = sequence(320, 240, 1)[0]
    o = P.ORBextractor(500, 1.2, 8, 20, 7)
    o(img)
    cap = o.max_keypoints(320, 240)
    g = P.FrameGrid(cap, 2)
    mono = lambda f, s0, first, n: L.pslfe_frame_set_from_orb_mono(f._h, s0, o._h, first, n, P._ptr(cam))
    assert mono(g, 0, 0, 1) == 0
    assert mono(g, 0, 1, 1) == E_INVALID and mono(g, 0, -1, 1) == E_INVALID and mono(g, 0, 0, 0) == E_INVALID
    assert mono(g, -1, 0, 1) == E_INVALID and mono(g, 2, 0, 1) == E_CAPACITY
    assert mono(P.FrameGrid(16, 1), 0, 0, 1) == E_CAPACITY
    assert L.pslfe_frame_set_from_orb_mono(g._h, 0, P.ORBextractor(500, 1.2, 8, 20, 7)._h, 0, 1, P._ptr(cam)) == E_STATE
    other = P.FrameGrid(cap, 1, ctx=P.Context(0))
    assert L.pslfe_frame_set_from_orb_mono(other._h, 0, o._h, 0, 1, P._ptr(cam)) == E_INVALID   # contexts
    n1 = g.fetch(0)[0].size
    prev = np.zeros((n1, 2), np.float32)
    m12 = np.zeros(n1, np.int32)
    n = C.c_int()
    call = lambda f1, s1, f2, s2, window=100: L.pslfe_orb_search_for_initialization(f1._h, s1, f2._h, s2, P._ptr(prev), window,
                                                                                    C.c_float(0.9), 1, P._ptr(m12), C.byref(n))
    assert call(g, 0, g, 1) == E_STATE and call(g, 1, g, 0) == E_STATE and call(g, 0, g, 5) == E_STATE
    assert call(g, 0, g, 0, -1) == E_INVALID
    other.set(0, *o.fetch(0, 320, 240), (0.0, 0.0, 320.0, 240.0))
    assert call(g, 0, other, 0) == E_INVALID                                                  # contexts
    assert call(g, 0, g, 0) == 0 and n.value > 0                                             # a frame against itself
    s = np.zeros(1, np.int32)
    dev = lambda stride, s1=s, s2=s: L.pslfe_orb_search_for_initialization_device(g._h, P._ptr(s1), g._h, P._ptr(s2), 1, C.c_void_p(16),
                                                                                 stride, 100, C.c_float(0.9), 1, C.c_void_p(16),
                                                                                 C.c_void_p(16))
    assert dev(cap - 1) == E_INVALID                                                          # rows shorter than F1's capacity
    assert dev(cap, s2=np.ones(1, np.int32)) == E_STATE and dev(cap, s1=np.full(1, 9, np.int32)) == E_STATE


def test_cpp_consumer_equals_python_path(tmp_path):
    """tools/dropin/mono_main.cpp: GrabImageMonocular + MonocularInitialization's matching, built with g++, run as a child process."""
    import psl_slam_amd as P
    exe = str(tmp_path / "mono_main")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tools", "dropin", "mono_main.cpp"),
                    "-L" + os.path.join(ROOT, "psl-slam_amd"), "-lpslfe", "-Wl,-rpath," + os.path.join(ROOT, "psl-slam_amd")],
                   check=True, capture_output=True)
    w, h, nf = 640, 480, 1000
    cam = camera(TUM1)
    frames = sequence(w, h, 9, seed=13)
    frames[4] = np.full((h, w), 128, np.uint8)      # no keypoints: the initialiser is dropped, the next frame starts again
    seq = str(tmp_path / "seq.bin")
    with open(seq, "wb") as f:
        np.array([w, h, len(frames)], np.int32).tofile(f)
        np.ascontiguousarray(cam).tofile(f)
        for fr in frames:
            fr.tofile(f)
    p = subprocess.run([exe, seq, str(nf)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    # the Python path
    ini = P.ORBextractor(2 * nf, 1.2, 8, 20, 7)
    g = P.FrameGrid(ini.max_keypoints(w, h), 2)
    m = P.ORBmatcher(0.9, True)
    initializing, prev, nk, nms = False, None, [], []
    for fr in frames:
        k, _ = ini(fr)
        nk.append(len(k))
        nm = -1
        if not initializing:
            if len(k) > 100:
                g.set_from_orb_mono(0, ini, 0, 1, cam)
                prev = xy(g.fetch(0)[0])
                initializing = True
        elif len(k) <= 100:
            initializing = False
        else:
            g.set_from_orb_mono(1, ini, 0, 1, cam)
            nm, _ = m.SearchForInitialization(g, 0, g, 1, prev, 100)
            if nm < 100:
                initializing = False
        nms.append(nm)
    assert got["keypoints"] == nk and got["matches"] == nms, (got, nk, nms)
    assert nms[0] == -1 and nms[4] == -1 and nms[5] == -1 and max(nms) >= 100
