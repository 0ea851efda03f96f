"""The stereo kernels (k_stereo_rows, k_stereo_match, k_stereo_filter) on the hand-made cases of tests/stereo_cases.py: the case's
images are extracted (the device level images equal the oracle's), pslfe_orb_debug_set_results puts the case's keypoints and
descriptors into both handles, and mvuRight, mvDepth, the two taps, mvKeysUn and the grid CSR equal the restatement
oracle/stereo_oracle.cpp and the written-down answers byte for byte - no tolerance anywhere.  Also the random kinds of
tests/test_stereo_cpu.py on the device, three pairs of one call with left0, right0 and slot0 all different (from two handles with
other frame strides, and from one handle), and the error paths of the tap."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases as sc
from stereo_cases import INV, SCALE
from test_stereo_gpu import assert_same, camera, slot_outputs

pytestmark = pytest.mark.gpu

E_INVALID, E_CAPACITY, E_STATE = -1, -4, -5
CASES = sc.all_cases()
BY_NAME = {c["name"]: c for c in CASES}


class Rig:
    """one context and, per geometry, a left and a right extractor and a FrameGrid"""

    def __init__(self):
        import torch
        import psl_slam_amd as P
        self.P, self.torch = P, torch
        self.dev = torch.device("cuda", 0)
        self.ctx = P.Context(0, torch.cuda.current_stream(self.dev).cuda_stream)
        self.by_geom, self.keep = {}, []

    def handles(self, geom):
        P = self.P
        if geom not in self.by_geom:
            g = sc.GEOMS[geom]
            oL, oR = P.ORBextractor(*sc.ORB, ctx=self.ctx), P.ORBextractor(*sc.ORB, ctx=self.ctx)
            self.by_geom[geom] = (oL, oR, P.FrameGrid(oL.max_keypoints(g["w"], g["h"]), 1, ctx=self.ctx))
        return self.by_geom[geom]

    def extract(self, orb, img, pad):
        """through the host entry, or from device memory with `pad` bytes of 0xff after every row (another level-0 pitch)"""
        if not pad:
            orb(img)
            return
        h, w = img.shape
        wide = np.full((h, w + pad), 0xff, np.uint8)
        wide[:, :w] = img
        d = self.torch.from_numpy(wide).to(self.dev)
        self.keep = [d]                                                 # level 0 of the handle is this buffer
        orb.extract_batch_device(d.data_ptr(), 1, w, h, w + pad, (w + pad) * h)

    def run(self, geom, left, right, kL, dL, kR, dR, cam):
        oL, oR, grid = self.handles(geom)
        self.extract(oL, left, sc.GEOMS[geom]["pad"])
        self.extract(oR, right, 0)
        for orb, img in ((oL, left), (oR, right)):
            for l, want in enumerate(sc.oracle_levels(img)):
                assert orb.debug_level_image(0, l).tobytes() == want.tobytes(), f"level {l} differs from the oracle's"
        oL.debug_set_results(0, kL, dL)
        oR.debug_set_results(0, kR, dR)
        grid.set_from_orb_stereo(0, oL, 0, oR, 0, 1, camera(cam))
        return slot_outputs(grid, 0)


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.ctx.synchronize()


def wanted(c, taps=None):
    """the restatement's outputs and, the cameras of the cases being free of distortion, mvKeysUn = mvKeys and their grid"""
    import oracle_lib
    ur, dep, idx, sad = taps if taps is not None else sc.restated(c)
    assert c["cam"][4] == 0
    start, gidx = oracle_lib.grid_build(c["kL"], oracle_lib.image_bounds(camera(c["cam"]), c["w"], c["h"]))
    return dict(uright=ur, depth=dep, idx=idx, sad=sad, kun=c["kL"], start=start, gidx=gidx)


def check(c, got):
    sc.assert_expected(c, (got["uright"], got["depth"], got["idx"], got["sad"]), c["name"])
    assert_same(got, wanted(c), c["name"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_case_equals_restatement_and_written_answers(rig, case):
    c = case
    check(c, rig.run(c["geom"], c["left"], c["right"], c["kL"], c["dL"], c["kR"], c["dR"], c["cam"]))
    if c["pad"]:
        oL = rig.handles(c["geom"])[0]
        assert oL.fetch(0, c["w"], c["h"])[0].tobytes() == c["kL"].tobytes()    # the handle extracted from device memory


def test_every_slot_of_the_handle(rig):
    """nL equal to the keypoint capacity of the handle"""
    oL, _, _ = rig.handles("base")
    cap = oL.max_keypoints(320, 240)
    c = sc.capacity_case(cap)
    assert len(c["kL"]) == cap > 2000
    check(c, rig.run(c["geom"], c["left"], c["right"], c["kL"], c["dL"], c["kR"], c["dR"], c["cam"]))


@pytest.mark.parametrize("kind", sc.DEVICE_KINDS)
def test_random_kinds_on_the_device(rig, kind):
    from oracle_lib import restate_stereo
    rng = np.random.default_rng(sc.device_seed(kind))
    seen = dict(sad=0, filtered=0, edge=0)
    for rep in range(sc.DEVICE_REPS):
        left, right, kL, dL, kR, dR = sc.random_device_pair(rng, kind)
        cam = (sc.CAM_A, sc.CAM_B)[rep % 2]
        got = rig.run("base", left, right, kL, dL, kR, dR, cam)
        c = dict(kL=kL, cam=cam, w=320, h=240)
        taps = restate_stereo(kL, dL, kR, dR, sc.oracle_levels(left), sc.oracle_levels(right), SCALE, INV, cam[9], cam[0])
        assert_same(got, wanted(c, taps), f"{kind} #{rep}")
        seen["sad"] += int((got["sad"] >= 0).sum())
        seen["filtered"] += int(((got["sad"] >= 0) & (got["uright"] < 0)).sum())
        seen["edge"] += int(((got["idx"] >= 0) & (got["sad"] < 0)).sum())
    if kind in ("noise", "noise_r", "ties"):
        assert seen["sad"] > 0 and seen["edge"] > 0 and seen["filtered"] > 0, seen


def test_three_pairs_of_one_call_with_offsets(rig):
    """One call of 3 pairs, left0 = 1, right0 = 5, slot0 = 2, both sides frames of one handle; against the same pairs run one by one
    through two handles, and against the restatement."""
    P = rig.P
    cs = [BY_NAME[n] for n in sc.BATCH]
    assert len({(c["geom"], c["cam"]) for c in cs}) == 1 and len({c["name"] for c in cs}) == 3
    w, h = cs[0]["w"], cs[0]["h"]
    filler = np.full((h, w), 50, np.uint8)
    imgs = np.ascontiguousarray(np.stack([filler] + [c["left"] for c in cs] + [filler] + [c["right"] for c in cs]))
    orb = P.ORBextractor(*sc.ORB, ctx=rig.ctx, max_batch=8)
    orb.extract_batch(imgs)
    for p, c in enumerate(cs):
        orb.debug_set_results(1 + p, c["kL"], c["dL"])
        orb.debug_set_results(5 + p, c["kR"], c["dR"])
    assert orb.fetch(2, w, h)[1].tobytes() == cs[1]["dL"].tobytes() and len(orb.fetch(4, w, h)[0]) == 0 == len(orb.fetch(0, w, h)[0])
    grid = P.FrameGrid(orb.max_keypoints(w, h), 6, ctx=rig.ctx)
    grid.set_from_orb_stereo(2, orb, 1, orb, 5, 3, camera(cs[0]["cam"]))
    for p, c in enumerate(cs):
        got = slot_outputs(grid, 2 + p)
        check(c, got)
        one = rig.run(c["geom"], c["left"], c["right"], c["kL"], c["dL"], c["kR"], c["dR"], c["cam"])
        assert_same(got, one, f"{c['name']}: pair {p} of the batch vs alone")


def test_three_pairs_of_one_call_from_two_handles(rig):
    """One call of 3 pairs from two handles with other frame strides: the left batch of 5 frames extracted from device memory at a
    wider pitch (left0 = 1), the right batch of 7 frames through the host entry (right0 = 3), slot0 = 2; against the restatement
    and against the pairs run alone.  The frames around the pairs hold other keypoints, so a base taken from the wrong handle or
    the wrong frame shows."""
    P, torch = rig.P, rig.torch
    cs = [BY_NAME[n] for n in sc.BATCH]
    w, h, pad = cs[0]["w"], cs[0]["h"], sc.GEOMS["pitch"]["pad"]
    filler = np.full((h, w), 50, np.uint8)
    lefts = [filler] + [c["left"] for c in cs] + [filler]
    wide = np.full((len(lefts), h, w + pad), 0xff, np.uint8)
    wide[:, :, :w] = np.stack(lefts)
    d_left = torch.from_numpy(wide).to(rig.dev)
    oL = P.ORBextractor(*sc.ORB, ctx=rig.ctx, max_batch=5)
    oL.extract_batch_device(d_left.data_ptr(), 5, w, h, w + pad, (w + pad) * h)
    oR = P.ORBextractor(*sc.ORB, ctx=rig.ctx, max_batch=7)
    oR.extract_batch(np.ascontiguousarray(np.stack([filler] * 3 + [c["right"] for c in cs] + [filler])))
    decoy = cs[1]
    for f in (0, 4):
        oL.debug_set_results(f, decoy["kR"], decoy["dR"])
    for f in (0, 1, 2, 6):
        oR.debug_set_results(f, decoy["kL"], decoy["dL"])
    for p, c in enumerate(cs):
        oL.debug_set_results(1 + p, c["kL"], c["dL"])
        oR.debug_set_results(3 + p, c["kR"], c["dR"])
        for l, want in enumerate(sc.oracle_levels(c["left"])):
            assert oL.debug_level_image(1 + p, l).tobytes() == want.tobytes()
    grid = P.FrameGrid(oL.max_keypoints(w, h), 6, ctx=rig.ctx)
    grid.set_from_orb_stereo(2, oL, 1, oR, 3, 3, camera(cs[0]["cam"]))
    for p, c in enumerate(cs):
        got = slot_outputs(grid, 2 + p)
        check(c, got)
        one = rig.run("pitch", c["left"], c["right"], c["kL"], c["dL"], c["kR"], c["dR"], c["cam"])
        assert_same(got, one, f"{c['name']}: pair {p} of the two-handle batch vs alone")
    del d_left


def test_error_paths_of_the_tap(rig):
    P = rig.P
    L = P.lib()
    k, d = np.zeros(4, P.KEYPOINT_DTYPE), np.zeros((4, 32), np.uint8)
    call = lambda o, frame, kk, dd, n: L.pslfe_orb_debug_set_results(o._h, C.c_int(frame), P._ptr(kk), P._ptr(dd), C.c_int(n))
    fresh = P.ORBextractor(*sc.ORB, ctx=rig.ctx)
    assert call(fresh, 0, k, d, 4) == E_STATE                               # nothing extracted yet
    fresh(BY_NAME["descriptor"]["left"])
    cap = fresh.max_keypoints(320, 240)
    before = fresh.fetch(0, 320, 240)
    assert call(fresh, 0, None, d, 4) == E_INVALID and call(fresh, 0, k, None, 4) == E_INVALID
    assert b"NULL" in L.pslfe_last_error()
    assert call(fresh, 1, k, d, 4) == E_INVALID and call(fresh, -1, k, d, 4) == E_INVALID   # outside the last batch
    assert call(fresh, 0, k, d, -1) == E_INVALID
    big_k, big_d = np.zeros(cap + 1, P.KEYPOINT_DTYPE), np.zeros((cap + 1, 32), np.uint8)
    assert call(fresh, 0, big_k, big_d, cap + 1) == E_CAPACITY
    after = fresh.fetch(0, 320, 240)
    assert len(before[0]) > 0 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))   # a refused call changes nothing
    k["x"], k["octave"] = (1.5, 2.5, 3.5, 4.5), (0, 1, 2, 7)
    d[:] = np.arange(128, dtype=np.uint8).reshape(4, 32)
    assert call(fresh, 0, k, d, 4) == 0
    fk, fd = fresh.fetch(0, 320, 240)
    assert fk.tobytes() == k.tobytes() and fd.tobytes() == d.tobytes()
    assert call(fresh, 0, k, d, 0) == 0 and len(fresh.fetch(0, 320, 240)[0]) == 0
    assert call(fresh, 0, big_k[:cap], big_d[:cap], cap) == 0 and len(fresh.fetch(0, 320, 240)[0]) == cap
