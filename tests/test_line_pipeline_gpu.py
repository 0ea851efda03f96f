"""The two-part schedule of pslfe_line_extract_batch_device on launches of at least 130 frames (pslfe_line.hip: run_extract, run_halves).
Behind the gradient the launch runs as A = the first 7/12 of the frames on the context's stream and B = the rest on the auxiliary
stream (each at least 65 frames), each on the per-frame arrays advanced to its first frame; k_lbd_pre of B runs on the context's stream
behind A's launches and B's k_lbd waits for it by an event.  tests/test_line_split_gpu.py pins F = 129 / 130 / 131, where the 65-frame
minimum decides the boundary; here the launches are large enough for the 7/12 share (F = 259 / 260 / 261: A = 151 / 151 / 152 frames),
span the sub-batches of scale and gradient, follow one another on one extractor, and are read back through pslfe_line_debug_gradient.

Every frame of a launch is compared byte for byte with the single-frame extractor on the same image (one frame per launch: no split, no
offset; pinned to the oracle in test_line_gpu.py): keylines, LBD rows, line equations, the overflow flags of d_status and the fans of
the batched pairing, in both refine modes.  The 640x480 images and their single-frame results are those of tests/test_line_split_gpu.py
(built once per session).  The heavy and the light frames change place between the cases, so that either part is the one whose grower
ends last, and the constant frame and the heaviest frame stand on both sides of the boundary between A and B and of the boundaries a
split in halves, thirds or quarters would have."""
import numpy as np
import pytest

import test_line_batch_regimes_gpu as R
import test_line_split_gpu as S
from line_cases import ADV, adversarial_images

pytestmark = pytest.mark.gpu

Q = 65                       # PSL_GROW_HELPER_FRAMES + 1 (pslfe_line.hip): the fewest frames of a part
SUB = R.LSD_SUBBATCH
_small = {}


def _first_of_b(F):
    """First frame of B (run_extract: PSL_LINE_FIRST_NUM / PSL_LINE_FIRST_DEN, both parts at least Q frames)."""
    return min(max(F * 7 // 12, Q), F - Q)


def _edges(F):
    """First and last frame of A and B, and those of every part of a split in 2, 3 or 4."""
    fb = _first_of_b(F)
    return sorted(set(S._edges(F)) | {0, fb - 1, fb, F - 1})


def _arrangement(F, edge, heavy_part):
    """Image names of the F frames: part `heavy_part` (0 = A, 1 = B) of the heavy images, the other mostly of the constant one,
    `edge` on both sides of every boundary."""
    heavy, light = ("adv blobs", "sticks/0", "sticks/1"), ("blank", "struct", "blank", "blank", "sticks/1")
    src = [heavy[f % 3] if (f >= _first_of_b(F)) == bool(heavy_part) else light[f % 5] for f in range(F)]
    for f in _edges(F):
        src[f] = edge
    return src


def test_the_arrangements_are_what_the_cases_assume():
    assert S._weight("blank") == 0 and S._heaviest() != "blank"
    assert [_first_of_b(F) for F in (130, 131, 4 * Q - 1, 4 * Q, 4 * Q + 1, 12288)] == [65, 66, 151, 151, 152, 7168]
    for F in (4 * Q - 1, 4 * Q, 4 * Q + 1):
        fb = _first_of_b(F)
        for hh in (0, 1):
            src = _arrangement(F, "blank", hh)
            w = [sum(S._weight(n) for n in src[:fb]), sum(S._weight(n) for n in src[fb:])]
            print(f"F={F} heavy part {'AB'[hh]}: defined pixels of A = [0, {fb}) {w[0]}, of B = [{fb}, {F}) {w[1]}")
            assert w[hh] > 2 * w[1 - hh]
            assert all(src[f] == "blank" for f in (0, fb - 1, fb, F // 2 - 1, F // 2, F - 1))


@R.MODES
@pytest.mark.parametrize("heavy_part", [0, 1], ids=["heavyA", "heavyB"])
@pytest.mark.parametrize("F", [4 * Q - 1, 4 * Q, 4 * Q + 1])
def test_two_part_launch_equals_the_single_frame_extractor(F, heavy_part, mode):
    """Both arrangements on one extractor: the constant frame, then the heaviest frame, on both sides of every boundary."""
    le = R._extractor(mode, F)
    try:
        for edge in ("blank", S._heaviest()):
            got = S._check_launch(le, F, _arrangement(F, edge, heavy_part), mode, f"edges {edge}, heavy part {'AB'[heavy_part]}:")
            assert sum(len(g[0]) for g in got) > 20 * (F // 2)
    finally:
        le.close()


@R.MODES
def test_two_calls_on_one_extractor_261_then_260(mode):
    """The parts of the second call start at other frames than those of the first, on other contents (the heavy part swapped):
    nothing of a part's state, and no event of the first call, may act on the second.  The results are read right after each call:
    the join holds, for B's k_lbd behind the k_lbd_pre on the other stream too."""
    le = R._extractor(mode, 4 * Q + 1)
    try:
        S._check_launch(le, 4 * Q + 1, _arrangement(4 * Q + 1, S._heaviest(), 0), mode, "first call")
        S._check_launch(le, 4 * Q, _arrangement(4 * Q, "blank", 1), mode, "second call")
    finally:
        le.close()


def _small_images():
    """Five distinct 64x48 images: tiles of line_cases' stripes, rings and frame that give 4, 5 and 2 keylines in both refine modes (CPU
    oracle), of the blobs (regions, no keyline), and a constant one."""
    if not _small:
        adv = adversarial_images()
        for name, y, x in (("stripes", 60, 140), ("rings", 240, 160), ("frame", 0, 320), ("blobs", 100, 100)):
            _small[f"{name} @{x},{y}"] = np.ascontiguousarray(adv[name][y:y + 48, x:x + 64])
        _small["const"] = np.full((48, 64), 93, np.uint8)
    return _small


@R.MODES
def test_sub_batch_boundaries_of_a_two_part_launch_4098_frames(mode):
    """F = 2 * 2048 + 2 small frames: scale and gradient run in three sub-batches, the last of two frames (the non-XCD grids), and
    the boundary between A and B (frame 2390) lies inside the second one.  The frames around every sub-batch boundary, around the
    middle of the launch and around the part boundary, and a seeded sample of 32 others, equal the single-frame result of their image."""
    small = _small_images()
    names = list(small)
    F = 2 * SUB + 2
    src = [f % len(names) for f in range(F)]
    ref = {n: R._single_result("small " + n, small[n], mode) for n in names}
    with_lines = [n for n in names if len(ref[n][0]) > 0]
    print(f"64x48, refine {mode}: keylines per image " + ", ".join(f"{n} {len(ref[n][0])}" for n in names))
    assert len(with_lines) >= 3, "LSD must still find segments at this frame size"
    want = {0, SUB - 1, SUB, SUB + 1, 2 * SUB, 2 * SUB + 1, _first_of_b(F) - 1, _first_of_b(F)}
    want |= {int(f) for f in np.random.default_rng(4098).choice(F, 32, replace=False)}
    batch = np.ascontiguousarray(np.stack([small[names[i]] for i in src], 0))
    le = R._extractor(mode, F)
    d_ptr, _ = le.ctx.device_array(batch)
    try:
        le.extract_batch_device(d_ptr, F, 64, 48, 64, 64 * 48)
        le.pair_batch_device(R.FAN_R, R.FAN_THR)
        seen = set()
        for f in sorted(want):
            k, d, e, st = le.fetch(f)
            assert st == 0, f
            R._equal((k, d, e, le.fans_fetch(f)), ref[names[src[f]]], f"4098-frame launch refine {mode} frame {f} ({names[src[f]]}) vs single frame")
            seen.add(names[src[f]])
        assert seen == set(names)
    finally:
        le.ctx.device_free(d_ptr)
        le.close()


def test_debug_gradient_after_a_split_launch_of_130_frames():
    """A launch that fits in d_scaled keeps frame f at place f: after a launch in two parts (A = frames 0 .. 64, B = 65 .. 129) the
    first and last frame of each part return the single-frame extractor's scaled image, angles and - where the angle is defined,
    which is where a many-frames launch stores it - gradient magnitude."""
    F = 2 * Q
    src = S._arrangement(F, S._heaviest())
    for f, name in ((0, "sticks/0"), (Q - 1, "struct"), (Q, "sticks/1"), (F - 1, "adv blobs")):
        src[f] = name
    imgs = S._images()
    le = R._extractor(ADV, F)
    d_ptr, _ = le.ctx.device_array(np.ascontiguousarray(np.stack([imgs[n] for n in src], 0)))
    try:
        le.extract_batch_device(d_ptr, F, S.W, S.H, S.W, S.W * S.H)
        got = {f: le.debug_gradient(f) for f in (0, Q - 1, Q, F - 1)}
    finally:
        le.ctx.device_free(d_ptr)
        le.close()
    S._single(src[0], ADV)   # creates the single-frame extractor
    one = R._single_le[ADV]
    for f, (scaled, ang, mod) in got.items():
        one(imgs[src[f]])
        rs, ra, rm = one.debug_gradient(0)
        defined = ra != S.NOTDEF
        assert defined.any(), f
        assert scaled.tobytes() == rs.tobytes(), f"frame {f} ({src[f]}): scaled image"
        assert ang.tobytes() == ra.tobytes(), f"frame {f} ({src[f]}): angles"
        assert mod[defined].tobytes() == rm[defined].tobytes(), f"frame {f} ({src[f]}): gradient magnitude"


def test_stage_profiling_keeps_the_serial_schedule_and_the_bytes_261():
    """With the context's stage profiling on, a launch of 261 frames stays on one stream: one grower launch, the same bytes."""
    import psl_slam_amd as P
    F = 4 * Q + 1
    ctx = P.Context(0)
    ctx.profile(True)
    le = P.LINEextractor(1, 1.2, 200, 0.0, ctx=ctx, max_batch=F)
    try:
        le.set_refine(ADV)
        S._check_launch(le, F, _arrangement(F, S._heaviest(), 1), ADV, "profiling on")
        ms, launches = ctx.stage_time("line.lsd_grow")
        assert launches == 1 and ms > 0, (ms, launches)
    finally:
        le.close()   # before its context
        ctx.profile(False)
        ctx.close()
