"""CPU checks of the projection entry points (include/pslfe.h: pslfe_orb_project_last[_device], pslfe_orb_project_frustum[_device],
pslfe_orb_search_by_projection_map_device): the restatement the GPU tests compare with (oracle/project_oracle.cpp) against a literal
transcription of Tracking::UpdateLastFrame's loop, the double log of PredictScale against the host's libm, the POD layouts, and the
argument checks of the library, which need no GPU."""
import ctypes as C

import numpy as np

import oracle_lib


def update_last_frame_loop(depth, th_depth):
    """src/Tracking.cc:1065-1103, transcribed: the keypoints the loop visits."""
    vDepthIdx = sorted((float(z), i) for i, z in enumerate(depth) if z > 0)
    visited, nPoints = set(), 0
    for z, i in vDepthIdx:
        visited.add(i)
        nPoints += 1
        if z > th_depth and nPoints > 100:
            break
    return visited


def depth_cases(rng):
    th = np.float32(3.0)
    yield np.zeros(0, np.float32), th
    yield np.zeros(50, np.float32), th                                     # no depth at all
    yield np.full(300, np.nan, np.float32), th
    for n_close in (0, 1, 99, 100, 101, 102, 250):                           # exactly 100 / 101 / 102 close points among others
        close = rng.uniform(0.1, 3.0, n_close).astype(np.float32)
        far = rng.uniform(3.01, 9.0, 200).astype(np.float32)
        d = np.concatenate([close, far, np.zeros(30, np.float32), np.full(5, np.nan, np.float32), -np.ones(7, np.float32)])
        yield rng.permutation(d), th
    yield rng.uniform(0.1, 2.9, 500).astype(np.float32), th                 # all close
    yield rng.uniform(3.5, 9.0, 500).astype(np.float32), th                 # all far
    yield rng.uniform(3.5, 9.0, 60).astype(np.float32), th                  # fewer valid than 101
    yield np.full(400, np.float32(2.0)), th                                 # all equal, close
    yield np.full(400, np.float32(5.0)), th                                 # all equal, far: ties broken by index
    yield np.where(rng.random(400) < 0.5, np.float32(3.0), np.float32(4.0)).astype(np.float32), th   # z == th_depth exactly
    for _ in range(300):
        n = int(rng.integers(0, 1300))
        d = rng.choice(np.float32([0.5, 1.0, 2.0, 3.0, 4.0, 0.0, np.nan]), n).astype(np.float32)
        d = np.where(rng.random(n) < 0.5, d, rng.uniform(-1, 8, n).astype(np.float32))
        yield d, np.float32(rng.choice([0.0, 1.0, 3.0, 100.0]))


def test_vo_selection_equals_update_last_frame_loop():
    rng = np.random.default_rng(5)
    ncases = 0
    for d, th in depth_cases(rng):
        d = np.ascontiguousarray(d, np.float32)
        L, sel = oracle_lib.pr_vo_select(d, th)
        want = update_last_frame_loop(d, float(th))
        got = set(np.flatnonzero(sel).tolist())
        assert got == want and L == len(want), (len(d), float(th), L, len(want))
        ncases += 1
    assert ncases > 300


def test_predicted_level_psl_log_equals_host_log():
    """PredictScale's level with the library's double log (psl_log) and with the host's log agree for every float ratio of the range
    isInFrustum lets through: mfMaxDistance / dist with 0.8 * min <= dist <= 1.2 * max, max / min up to 1.2^7 (8 levels)."""
    scale, nlevels = np.float32(1.2), 8
    lsf = np.float32(np.log(scale))
    lo = np.float32(1.0) / np.float32(1.2)
    hi = np.float32(scale ** (nlevels - 1)) / np.float32(0.8)
    bad, n = oracle_lib.pr_level_sweep(lo, hi, lsf, nlevels)
    assert n > 20_000_000 and bad == 0, (n, bad)
    # the clamps of src/MapPoint.cc:409-412 and the defined edge cases
    assert oracle_lib.pr_predict_level(0.5, lsf, nlevels) == 0
    assert oracle_lib.pr_predict_level(1000.0, lsf, nlevels) == nlevels - 1
    assert oracle_lib.pr_predict_level(np.inf, lsf, nlevels) == nlevels - 1
    assert oracle_lib.pr_predict_level(0.0, lsf, nlevels) == 0
    assert oracle_lib.pr_predict_level(np.nan, lsf, nlevels) == 0


def test_projection_dtypes_match_header():
    import psl_slam_amd as P
    sz = oracle_lib.pr_sizes()
    assert list(sz) == [P.POSE_DTYPE.itemsize, P.LASTPOINT_DTYPE.itemsize, P.MAPPOINT_DTYPE.itemsize, P.PROJQUERY_DTYPE.itemsize]
    assert list(sz) == [48, 16, 32, 32]
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (1, 2, 3)
    p = P.pose(T)
    assert p["R"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1] and p["t"].tolist() == [1, 2, 3]


def test_projection_entry_points_reject_null_arguments_without_a_gpu():
    import psl_slam_amd as P
    P.build()
    L = P.lib()
    f0 = C.c_float(0.0)
    fb = [C.c_float(0.0), C.c_float(0.0), C.c_float(640.0), C.c_float(480.0)]
    nq = C.c_int(7)
    E = -1  # PSLFE_E_INVALID
    assert L.pslfe_orb_project_last(None, 0, None, None, None, None, None, None, 8, C.c_float(15.0), C.c_float(3.0), 0, 1, *fb,
                                    None, None, None, C.byref(nq), 0) == E
    assert L.pslfe_orb_project_last_device(None, 0, 1, None, None, None, None, None, None, 8, C.c_float(15.0), C.c_float(3.0), 0, 0,
                                           *fb, None, None, None, None, 16) == E
    assert L.pslfe_orb_project_frustum(None, None, None, None, 0, None, None, 8, f0, C.c_float(0.5), C.c_float(1.0), *fb, None, None,
                                       None, C.byref(nq), 0, None, None, None) == E
    assert L.pslfe_orb_project_frustum_device(None, 1, None, None, None, None, 16, None, None, 8, f0, C.c_float(0.5), C.c_float(1.0),
                                              *fb, None, None, None, None, 16, None, None, None) == E
    assert L.pslfe_orb_search_by_projection_map_device(None, 0, 1, None, None, None, 16, None, C.c_float(0.8), None, None) == E
    assert "NULL" in L.pslfe_last_error().decode()
