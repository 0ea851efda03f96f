"""The rect_improve / NFA launches of LSD_REFINE_ADV (line_kernels3.h) on small frames chosen for WHERE their rectangles are decided.

k_lsd_nfa_count<first test> counts the first test's tolerance and the five of the first finer-precision phase in one pixel pass, and every
k_lsd_nfa_select appends the rectangles it leaves undecided to the per-frame list that the launches of the next phase walk.  The
segments after the refinement are compared bit for bit with the CPU oracle (oracle/line_oracle.cpp) and with the same image run
alone, in a launch of 67 frames (many-frames grids: PSL_NFA_COUNT_WGS count workgroups, one select workgroup per frame) and in one
of 3 frames (few-frames grids: 128 count workgroups, 4 select workgroups per frame); an image that occurs at several positions of a
launch must give the same bytes at each (nothing leaks from one frame's list into another's).

The images (136 x 104) and what rect_improve does with their rectangles, counted once on the CPU with tools/nfa_phase_stats.py (the
oracle's rectangles, angles and nfa() with rect_improve's control flow restated; it accepts exactly as many rectangles as the oracle
returns segments).  `leave` = rectangles accepted by the first test, after phases -1, 0, 1, 2, 3, and rejected after phase 3;
`guarded` = trials of phases 0 - 3 that the width guard (width - 0.5 < 0.5) excludes, stored as (-1, 0):
  flat      no rectangle: cnt == 0, every list empty
  clean     2 rectangles, leave [2, 0, 0, 0, 0, 0, 0], guarded 0: one high-contrast bar through the image under the 0.6 px blur of
            synth_frames - both edges accepted by the first test, the lists are empty from phase -1 on
  weak_a    13 rectangles, leave [0, 0, 0, 0, 0, 0, 13], guarded 176: low-contrast bars under noise: all survive into every phase and are
            rejected after phase 3
  weak_b    12 rectangles, leave [1, 3, 1, 0, 0, 0, 7], guarded 49: accepted by the first test, after phase -1 and after phase 0, or rejected
  thin      11 rectangles, leave [0, 0, 0, 0, 0, 0, 11], guarded 160: one-pixel lines: most trials of phases 0 - 3 fall under the width guard
  ramp      38 rectangles, leave [15, 0, 0, 0, 0, 0, 23], guarded 37: the noisy diagonal ramp of test_line_gpu.py (slope 3.26 per pixel as at
            40 x 40, folded at 255 so that it fits the larger frame)
  texture   260 rectangles (> 256: more than one trip of k_lsd_nfa_select's loop and of the list append per workgroup), leave
            [22, 2, 10, 2, 2, 0, 222], guarded 949: accepted in the first test and after phases -1, 0, 1 and 2, rejected after phase 3
"""
import numpy as np
import pytest

from line_cases import ADV

pytestmark = pytest.mark.gpu

W, H = 136, 104
_cache = {}


def _bars(seed, contrast, noise, n, thick, blur):
    """n short bars of +-contrast on a grey ground, blurred, under Gaussian noise."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 120.0, np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    for i in range(n):
        cx, cy = rng.uniform(20, W - 20), rng.uniform(15, H - 15)
        L, Wd = rng.uniform(20, 40) / 2, rng.uniform(*thick) / 2
        th = rng.uniform(0, np.pi)
        c, s = np.cos(th), np.sin(th)
        u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
        img[(np.abs(u) < L) & (np.abs(v) < Wd)] = 120 + contrast * (1 if i % 2 else -1)
    img = gaussian_filter(img, blur)
    if noise:
        img = img + rng.normal(0, noise, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _through(seed):
    """One dark bar, 6 px wide, that leaves the image at both ends (no short edges), with the point spread of synth_frames' 'sticks'."""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 120.0, np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    th, off = rng.uniform(0.2, 1.3), rng.uniform(-25, 25)
    img[np.abs(-(xx - W / 2) * np.sin(th) + (yy - H / 2) * np.cos(th) - off) < 3] = 30
    return np.clip(np.rint(gaussian_filter(img, 0.6)), 0, 255).astype(np.uint8)


def _ramp(noise, seed):
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.abs((3.26 * (xx + yy)) % 510 - 255)
    return np.clip(v + np.random.default_rng(seed).normal(0, noise, (H, W)), 0, 255).astype(np.uint8)


def _texture(seed, sigma):
    from scipy.ndimage import gaussian_filter
    n = gaussian_filter(np.random.default_rng(seed).standard_normal((H, W)), sigma)
    n = (n - n.min()) / (n.max() - n.min())
    return (n * 255).astype(np.uint8)


def images():
    """name -> image, in a fixed order"""
    if "images" not in _cache:
        _cache["images"] = {
            "flat": np.full((H, W), 128, np.uint8),
            "clean": _through(1),
            "weak_a": _bars(40, 18, 2.0, 6, (4, 6), 0.6),
            "weak_b": _bars(41, 25, 2.5, 6, (4, 6), 0.6),
            "thin": _bars(20, 20, 1.0, 8, (1, 2), 0.4),
            "ramp": _ramp(0.6, 2),
            "texture": _texture(1, 2.5),
        }
    return _cache["images"]


def _reference(name):
    """(segments of the CPU oracle, segments of the image run alone on the device): computed once per image"""
    if ("ref", name) not in _cache:
        import oracle_lib
        import psl_slam_amd as P
        if "le1" not in _cache:
            _cache["le1"] = P.LINEextractor(1, 1.2, 200, 0.0)
            _cache["le1"].set_refine(ADV)
        img = images()[name]
        _cache[("ref", name)] = (oracle_lib.lsd_detect(img), _cache["le1"].lsd_detect(img))
    return _cache[("ref", name)]


def _launch(names):
    """One launch over the named images -> the LSD segments of every frame"""
    import psl_slam_amd as P
    F = len(names)
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=F)
    le.set_refine(ADV)
    frames = np.ascontiguousarray(np.stack([images()[n] for n in names], 0))
    d_ptr, _ = le.ctx.device_array(frames)
    try:
        le.extract_batch_device(d_ptr, F, W, H, W, W * H)
        return [le.segments_fetch(f) for f in range(F)]
    finally:
        le.ctx.device_free(d_ptr)


def _check(names, segs):
    first = {}
    for f, name in enumerate(names):
        ref, alone = _reference(name)
        what = f"launch of {len(names)} frames, frame {f} ({name})"
        assert segs[f].shape == ref.shape and segs[f].tobytes() == ref.tobytes(), f"{what}: {len(segs[f])} segments vs {len(ref)} of the oracle, or their bits differ"
        assert segs[f].tobytes() == alone.tobytes(), f"{what}: differs from the image run alone"
        assert segs[f].tobytes() == segs[first.setdefault(name, f)].tobytes(), f"{what}: differs from frame {first[name]} of the same launch"


def test_oracle_counts_of_the_images():
    """The segment counts the docstring's `leave` rows add up to (accepted = all but the last entry)."""
    want = {"flat": 0, "clean": 2, "weak_a": 0, "weak_b": 5, "thin": 0, "ramp": 15, "texture": 38}
    assert {n: len(_reference(n)[0]) for n in images()} == want


def test_many_frames_launch():
    """67 frames: every image at 9 or 10 positions, the texture frame next to the flat one at both ends of the cycle"""
    order = ["texture", "flat", "clean", "weak_a", "thin", "weak_b", "ramp"]
    names = [order[f % len(order)] for f in range(67)]
    _check(names, _launch(names))


def test_few_frames_launch():
    """3 frames: the frame with more than 256 rectangles twice around the one with none (4 select workgroups per frame append to one list)"""
    names = ["texture", "flat", "texture"]
    _check(names, _launch(names))


def test_few_frames_launch_of_the_weak_frames():
    """3 frames whose rectangles are decided late or never, many of their trials under the width guard"""
    names = ["weak_a", "thin", "weak_b"]
    _check(names, _launch(names))
