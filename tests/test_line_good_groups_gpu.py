"""k_line_good packs several frames into one wave, one per group of lanes (PSL_GOOD_GROUPS, psl-slam_amd/csrc/pslfe_glue.hip).
These cases put frames that take different paths side by side in one block - different line counts, a frame without depth,
a frame of very short lines, dead groups in the last block, the same frame under different rand() seeds - and compare every
output of every frame byte for byte with the sequential oracle run with that frame's seed."""
import functools

import numpy as np
import pytest

import glue_scene
from test_glue_gpu import KEYS

pytestmark = pytest.mark.gpu

ML, MF = 64, 128


def _same(a, b, what):
    for k in KEYS:
        assert a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@functools.lru_cache(maxsize=None)
def _scene(seed, nlines, nfans=100):
    kls, fans, depth, cam, _ = glue_scene.scene(seed=seed, nlines=nlines, nfans=nfans)
    for a in (kls, fans, depth):
        a.setflags(write=False)
    return kls, fans, depth, cam


def _batch(frames, seed0):
    """frames: (kls, fans, depth, cam) per frame.  One launch of run_batch_device; returns (got, ref) lists, ref = the oracle with seed0 + f."""
    import psl_slam_amd as P
    import oracle_lib
    ctx = P.default_context()
    F = len(frames)
    kls = np.zeros((F, ML), P.KEYLINE_DTYPE)
    fans = np.zeros((F, MF, 4), np.float32)
    nkl, nfans = np.zeros(F, np.int32), np.zeros(F, np.int32)
    depth = np.zeros((F, glue_scene.H, glue_scene.W), np.float32)
    for f, (k, fa, d, _) in enumerate(frames):
        kls[f, :len(k)] = k
        fans[f, :len(fa)] = fa
        nkl[f], nfans[f] = len(k), len(fa)
        depth[f] = d
    ptrs = [ctx.device_array(a)[0] for a in (kls, fans, nkl, nfans, depth)]
    d_kls, d_fans, d_nkl, d_nfans, d_depth = ptrs
    g = P.FrameGlue(max_lines=ML, max_fans=MF, max_batch=F)
    g.run_batch_device(F, d_kls, ML, d_nkl, d_fans, MF, d_nfans, d_depth, glue_scene.W, glue_scene.H, frames[0][3], seed0=seed0)
    got = [g.fetch(f, len(k)) for f, (k, _, _, _) in enumerate(frames)]
    ctx.synchronize()
    for p in ptrs:
        ctx.device_free(p)
    ref = [oracle_lib.frame_glue(k, fa, d, cam, seed=seed0 + f) for f, (k, fa, d, cam) in enumerate(frames)]
    return got, ref


def _accepted(r):
    return int((np.abs(r["lines3d"]).sum(1) > 0).sum())


def _check(frames, seed0):
    got, ref = _batch(frames, seed0)
    for f, (a, b) in enumerate(zip(got, ref)):
        _same(a, b, f"frame {f} of {len(frames)}")
    return ref


def _fans_within(fans, nlines):
    """the fan rows whose two lines exist among the first nlines"""
    return fans[(fans[:, 2] < nlines) & (fans[:, 3] < nlines)]


@pytest.mark.parametrize("F", [1, 2, 3, 4, 7])
def test_tail_sizes(F):
    """a lone group, full blocks, and a last block with one or two dead groups"""
    frames = [_scene(20 + f, 40 + 4 * f) for f in range(F)]   # 40 .. 64 lines, a scene of its own each
    ref = _check(frames, seed0=7)
    for r in ref:
        assert _accepted(r) > 10 and len(r["planes"]) > 0


@pytest.mark.parametrize("order", [(0, 5, 64), (64, 0, 5), (5, 64, 0)])
def test_unequal_line_counts(order):
    """0, 5 and 64 lines in the three groups of one block, in each rotation: a group that is done waits for the others"""
    kls, fans, depth, cam = _scene(31, 64)
    frames = [(kls[:n], _fans_within(fans, n), depth, cam) for n in order]
    ref = _check(frames, seed0=100)
    big = ref[order.index(64)]
    assert _accepted(big) > 20 and len(big["planes"]) > 0
    assert len(ref[order.index(0)]["lines3d"]) == 0


@pytest.mark.parametrize("where", [0, 1, 2])
def test_frame_without_depth_beside_normal_frames(where):
    """every line of the depthless frame stops at np < 5 while its neighbours run the RANSAC"""
    frames = [_scene(41 + f, 50 + f) for f in range(3)]
    k, fa, d, cam = frames[where]
    frames[where] = (k, fa, np.zeros_like(d), cam)
    ref = _check(frames, seed0=3)
    for f, r in enumerate(ref):
        if f == where:
            assert _accepted(r) == 0 and np.all(r["lineEq"] == -1) and len(r["planes"]) == 0
        else:
            assert _accepted(r) > 10 and len(r["planes"]) > 0


@pytest.mark.parametrize("where", [0, 1, 2])
def test_frame_of_very_short_lines_beside_normal_frames(where):
    """a frame that keeps only its lines shorter than 5 pixels (at most 5 samples each, some with none)"""
    frames = [_scene(51 + f, 60) for f in range(3)]
    k, fa, d, cam = frames[where]
    ln = np.hypot(k["startPointX"] - k["endPointX"], k["startPointY"] - k["endPointY"])
    short = k[ln < 5]
    assert len(short) >= 4
    frames[where] = (short, np.zeros((0, 4), np.float32), d, cam)
    ref = _check(frames, seed0=11)
    for f, r in enumerate(ref):
        if f != where:
            assert _accepted(r) > 10 and len(r["planes"]) > 0


def test_same_frame_in_every_group():
    """three copies of one scene in one block, seeds seed0 .. seed0 + 2: a ring or stream position shared between groups would
    make the copies agree with each other, or with the wrong oracle run"""
    frames = [_scene(61, 64)] * 3
    ref = _check(frames, seed0=12345)
    assert all(_accepted(r) > 20 and len(r["planes"]) > 0 for r in ref)
    # the seeds matter: the oracle runs differ from each other, so equality with the own run is no accident
    assert any(ref[0][k].tobytes() != ref[1][k].tobytes() for k in KEYS) and any(ref[1][k].tobytes() != ref[2][k].tobytes() for k in KEYS)


@pytest.mark.parametrize("seed", [1, 12345])
def test_single_frame_entry_point(seed):
    """FrameGlue.run: one frame, one live group"""
    import psl_slam_amd as P
    import oracle_lib
    kls, fans, depth, cam, _ = glue_scene.scene(seed=3)
    got = P.FrameGlue(max_lines=256, max_fans=512).run(kls, fans, depth, cam, seed=seed)
    ref = oracle_lib.frame_glue(kls, fans, depth, cam, seed=seed)
    assert _accepted(ref) > 20 and len(ref["planes"]) > 0
    _same(got, ref, f"seed {seed}")
