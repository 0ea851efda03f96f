"""pslfe_line_extract_batch_device on launches of at least 130 frames (pslfe_line.hip: run_extract): everything behind the gradient runs
in parts of contiguous frames on two streams, each part a many-frames launch of its own on the per-frame arrays advanced to its first
frame.  F = 129 is the last launch that is not split, 130 the first that is, 131 splits unevenly.  Every frame of a launch is compared
byte for byte with the single-frame extractor on the same image (one frame per launch: no split, no offset; pinned to the oracle in
test_line_gpu.py): keylines, LBD rows, line equations, the overflow flags of d_status, and the fans of the batched pairing.

The frames are five distinct 640x480 images, repeated: two 'sticks' frames, a 'struct' frame, a constant frame (no segment at all) and
line_cases' adversarial blobs (tiled to the frame size).  The first half of a launch is made of the heavy images, the second mostly of
the constant one, and the frames on both sides of every boundary a split in two, three or four parts has - where a wrong offset would
show - are all the constant frame in one arrangement and all the heaviest frame in the other.  The scenes and the single-frame results
are those of tests/test_line_batch_regimes_gpu.py (built once per session)."""
import numpy as np
import pytest

import test_line_batch_regimes_gpu as R
from line_cases import ADV, STD, adversarial_images

pytestmark = pytest.mark.gpu

W, H = R.W, R.H
NOTDEF = np.float32(-1024.0)   # PSL_LSD_NOTDEF (line_kernels.h): the angle of a pixel without a defined gradient
_set, _extra = {}, {}


def _images():
    """name -> image, in a fixed order."""
    if not _set:
        blobs = adversarial_images()["blobs"]   # 400 x 300
        _set.update({"sticks/0": R._frame("sticks", R.STICKS[0], 0), "sticks/1": R._frame("sticks", R.STICKS[0], 1),
                     "struct": R._frame("struct", 3, 0), "blank": np.full((H, W), 93, np.uint8),
                     "adv blobs": np.ascontiguousarray(np.tile(blobs, (2, 2))[:H, :W])})
    return _set


def _single(name, mode):
    """(keylines, LBD, lineEq, fans, status) of the single-frame extractor."""
    img = _images()[name]
    ref = R._single_result("split " + name, img, mode)
    if (name, mode) not in _extra:
        le = R._single_le[mode]
        le(img)
        st = le.fetch(0)[3]
        _extra[(name, mode)] = st, int(np.count_nonzero(le.debug_gradient(0)[1] != NOTDEF))
    return ref + (_extra[(name, mode)][0],)


def _weight(name):
    """Pixels with a defined gradient: what k_lsd_grad counts for k_frame_order."""
    _single(name, ADV)
    return _extra[(name, ADV)][1]


def _edges(F):
    """First and last frame of every part of a launch split in 2, 3 or 4."""
    return sorted({i for p in (2, 3, 4) for k in range(p) for i in (F * k // p, F * (k + 1) // p - 1)})


def _arrangement(F, edge):
    """Image names of the F frames: heavy first half, light second half, `edge` at every part boundary."""
    heavy, light = ("adv blobs", "sticks/0", "sticks/1"), ("blank", "struct", "blank", "blank", "sticks/1")
    src = [heavy[f % 3] if f < F // 2 else light[f % 5] for f in range(F)]
    for f in _edges(F):
        src[f] = edge
    return src


def _heaviest():
    return max(_images(), key=_weight)


def _check_launch(le, F, src, mode, what):
    imgs = _images()
    got = R._run_batch(le, np.stack([imgs[n] for n in src], 0))
    assert len(got) == F
    for f, name in enumerate(src):
        ref = _single(name, mode)
        w = f"{what} F={F} refine {mode} frame {f} ({name})"
        assert got[f][4] == ref[4], f"{w}: status {got[f][4]} vs {ref[4]} of the single-frame extractor"
        R._equal(got[f], ref, w + " vs single frame")
    return got


def test_the_frames_are_what_the_arrangements_assume():
    names = list(_images())
    assert _weight("blank") == 0 and len(_single("blank", ADV)[0]) == 0 and len(_single("blank", STD)[0]) == 0
    assert min(len(_single(n, m)[0]) for n in ("sticks/0", "sticks/1", "struct") for m in (ADV, STD)) > 20
    for F in (129, 130, 131):
        src = _arrangement(F, "blank")
        wa, wb = sum(_weight(n) for n in src[:F // 2]), sum(_weight(n) for n in src[F // 2:])
        print(f"F={F}: defined pixels of the first half {wa}, of the second {wb}; heaviest image {_heaviest()}; " +
              ", ".join(f"{n} {_weight(n)}" for n in names))
        assert wa > 2 * wb
        assert {0, F // 2 - 1, F // 2, F - 1} <= set(_edges(F))


@R.MODES
@pytest.mark.parametrize("F", [129, 130, 131])
def test_split_launch_equals_the_single_frame_extractor(F, mode):
    """Both arrangements on one extractor: the constant frame, then the heaviest frame, first and last of every part."""
    le = R._extractor(mode, F)
    for edge in ("blank", _heaviest()):
        got = _check_launch(le, F, _arrangement(F, edge), mode, f"edges {edge}:")
        assert sum(len(g[0]) for g in got) > 20 * F // 2


@R.MODES
def test_two_calls_on_one_extractor_131_then_130(mode):
    """The parts of the second call start at other frames than those of the first, on other contents (halves swapped): nothing of a
    part's state may survive the call.  The results are read right after each call: the join holds."""
    le = R._extractor(mode, 131)
    _check_launch(le, 131, _arrangement(131, _heaviest()), mode, "first call")
    _check_launch(le, 130, _arrangement(130, "blank")[::-1], mode, "second call")


def test_stage_profiling_keeps_the_serial_schedule_and_the_bytes():
    """With the context's stage profiling on, a launch of 131 frames stays on one stream (the stage timers keep their meaning)."""
    import psl_slam_amd as P
    ctx = P.Context(0)
    ctx.profile(True)
    le = P.LINEextractor(1, 1.2, 200, 0.0, ctx=ctx, max_batch=131)
    try:
        le.set_refine(ADV)
        _check_launch(le, 131, _arrangement(131, _heaviest()), ADV, "profiling on")
        ms, launches = ctx.stage_time("line.lsd_grow")
        assert launches == 1 and ms > 0, (ms, launches)
    finally:
        le.close()   # before its context
        ctx.profile(False)
        ctx.close()
