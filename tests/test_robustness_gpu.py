"""Failure paths of the C ABI on the GPU: a prepare() whose allocations fail must leave the object empty - the next call with
the same geometry has to fail again (or allocate cleanly), never launch kernels on freed or undersized buffers."""
import numpy as np
import pytest

import synth_frames as sf

pytestmark = pytest.mark.gpu


def test_line_prepare_allocation_failure_is_clean_and_repeatable():
    import psl_slam_amd as P
    import oracle_lib
    img = sf.Scene(640, 480, "struct", 3).gray(0)
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=65535)   # ~17 MB of working buffers per frame: > 1 TB, cannot be allocated
    for _ in range(2):
        with pytest.raises(P.PslfeError):
            le(img)
    with pytest.raises(P.PslfeError):
        le.lsd_detect(img)
    le.close()
    ok = P.LINEextractor(1, 1.2, 200, 0.0)                    # the context is still healthy
    k, d, e = ok(img)
    rk, rd, re_ = oracle_lib.line_extract(img, 200)
    assert k.tobytes() == rk.tobytes() and (d == rd).all()


def test_orb_prepare_allocation_failure_is_clean_and_repeatable():
    import psl_slam_amd as P
    import oracle_lib
    small = sf.Scene(640, 480, "desk", 3).gray(0)
    big = sf.Scene(1280, 960, "desk", 3).gray(0)
    orb = P.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=60000)  # 1280x960: ~18 MB per frame -> > 1 TB
    for _ in range(2):
        with pytest.raises(P.PslfeError):
            orb(big)
    orb.close()
    ok = P.ORBextractor(1000, 1.2, 8, 20, 7)
    k, d = ok(small)
    rk, rd = oracle_lib.OracleORB(1000, 1.2, 8, 20, 7)(small)
    assert k.tobytes() == rk.tobytes() and (d == rd).all()
    # a geometry change after a successful prepare, then back: results unchanged
    k2, d2 = ok(big)
    k3, d3 = ok(small)
    assert len(k2) > 0 and k3.tobytes() == k.tobytes() and (d3 == d).all()


def test_frame_create_allocation_failure_is_clean():
    import psl_slam_amd as P
    import oracle_lib
    ctx = P.default_context()
    for _ in range(2):
        with pytest.raises(P.PslfeError):
            P.FrameGrid(4096, 10_000_000, ctx=ctx)                # 10 M frames of 4096 keypoints: > 1 TB, cannot be allocated
    orc = oracle_lib.OracleORB()
    sc = sf.Scene(640, 480, "desk", seed=11)
    (k0, d0), (k1, d1) = orc(sc.gray(0)), orc(sc.gray(1))
    bounds = (0.0, 0.0, 640.0, 480.0)
    q = np.zeros(len(k0), P.PROJQUERY_DTYPE)
    q["u"], q["v"] = k0["x"], k0["y"]
    q["radius"] = np.float32(15.0) * sf.orb_scale_factors()[k0["octave"]]
    q["min_level"], q["max_level"] = k0["octave"] - 1, k0["octave"] + 1
    q["angle"], q["blocks"] = k0["angle"], 1
    g = P.FrameGrid(2048, 1, ctx=ctx)                            # the context is still healthy
    g.set(0, k1, d1, bounds)
    nm, match, assigned = P.ORBmatcher(0.9, True).SearchByProjectionLast(g, 0, q, d0)
    rnm, rmatch, rassigned = oracle_lib.search_by_projection_last(k1, d1, None, bounds, q, d0, None, True)
    assert nm == rnm and nm > 300
    np.testing.assert_array_equal(match, rmatch)
    np.testing.assert_array_equal(assigned, rassigned)


def test_glue_create_allocation_failure_is_clean():
    import psl_slam_amd as P
    import oracle_lib
    import glue_scene
    ctx = P.default_context()
    for _ in range(2):
        with pytest.raises(P.PslfeError):                        # the first buffers (~4 GB) fit, the per-fan ones (> 1 TB) do not
            P.FrameGlue(max_lines=64, max_fans=1 << 20, max_batch=1 << 20, ctx=ctx)
    kls, fans, depth, cam, _ = glue_scene.scene(seed=3)
    got = P.FrameGlue(max_lines=256, max_fans=512, ctx=ctx).run(kls, fans, depth, cam, seed=1)
    ref = oracle_lib.frame_glue(kls, fans, depth, cam, seed=1)
    assert len(ref["planes"]) > 0
    for k in ("lines3d", "lineEq", "pair", "xy", "cross", "le_l", "planes", "normals", "lineNo", "cross3d", "cross2d"):
        assert got[k].shape == ref[k].shape and got[k].tobytes() == ref[k].tobytes(), k
