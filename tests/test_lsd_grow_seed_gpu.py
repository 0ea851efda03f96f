"""Two places of k_lsd_grow4 (line_kernels.h) on images of 64 x 48: the seed's (float)cos / sin of the double angle, which the grower
of a many-frames launch (F > 64: <0, 0>) evaluates at each region start and that of a few-frames launch (<3, 1>) reads from
k_lsd_grad's table (lsdg_region_grow4), and the rectangle step (lsdw_region2rect) with its sums staged in
blocks of 64 lanes and its four extents reduced over the wave.  Every frame is compared bit for bit with the CPU oracle
(oracle/line_oracle.cpp) in the launch's refine mode: the LSD segment list (with LSD_REFINE_STD it comes straight from the
rectangle) and the keylines, LBD rows and line equations.
  1. one straight edge per frame, the bright side at every 15 degrees - the four axis directions among them, where the quadrant of
     the restricted-range cos / sin switches - at F = 1 (<3, 1>, one launch per frame), 24 (<3, 1>), 66 (<0, 0>) and 132 (the two-part
     schedule on two streams);
  2. one bar per frame, lengths 4 .. 70 pixels: region sizes on both sides of the 64-lane block.  The oracle's growth log must show
     a region of fewer than 4 pixels and sizes = 63, 0 and 1 (mod 64) before anything runs.
<3, 0> (a few frames whose `used` bits do not fit in LDS: beyond 1280 x 960) cannot be reached with images this small; it shares the
seed table's path with <3, 1>."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from line_cases import ADV, STD, assert_extract_equal

pytestmark = pytest.mark.gpu

W, H = 64, 48
MODES = pytest.mark.parametrize("mode", [ADV, STD], ids=["adv", "std"])
ANGLES = tuple(range(0, 360, 15))
ADV_DROPPED = (30, 45, 60, 150, 165, 210, 225, 240, 330, 345)   # directions whose rectangle the oracle's NFA test rejects (LSD_REFINE_ADV)
BAR_LENGTHS = tuple(range(4, 71))
BAR_ANGLE, BAR_THICK = 33.0, 7.0   # degrees, pixels: chosen so that the oracle's region sizes meet the condition of test 2

_oracle, _images = {}, {}


@contextlib.contextmanager
def _oracle_mode(mode):
    import oracle_lib
    oracle_lib.set_lsd_refine(mode)
    try:
        yield oracle_lib
    finally:
        oracle_lib.set_lsd_refine(ADV)


def _ramp(d):
    """An anti-aliased step: 0 below -0.5, 1 above +0.5 (signed distance d in pixels)."""
    return np.clip(d + 0.5, 0.0, 1.0)


def edge_image(deg):
    """A half plane through the centre of the frame whose bright side lies in direction `deg`."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.deg2rad(deg)
    d = (xx - (W - 1) / 2) * np.cos(a) + (yy - (H - 1) / 2) * np.sin(a)
    return np.rint(40.0 + 170.0 * _ramp(d)).astype(np.uint8)


def bar_image(length, deg=BAR_ANGLE, thick=BAR_THICK):
    """A bright bar of `length` x `thick` pixels through the centre of the frame, its long side in direction `deg`."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    a = np.deg2rad(deg)
    u = (xx - (W - 1) / 2) * np.cos(a) + (yy - (H - 1) / 2) * np.sin(a)
    v = -(xx - (W - 1) / 2) * np.sin(a) + (yy - (H - 1) / 2) * np.cos(a)
    return np.rint(30.0 + 190.0 * _ramp(length / 2 - np.abs(u)) * _ramp(thick / 2 - np.abs(v))).astype(np.uint8)


def _image(kind, v):
    if (kind, v) not in _images:
        _images[(kind, v)] = np.ascontiguousarray(edge_image(v) if kind == "edge" else bar_image(v))
    return _images[(kind, v)]


def _oracle_result(kind, v, mode):
    """(segments, keylines, LBD, lineEq) of the CPU oracle, computed once per image and mode."""
    if (kind, v, mode) not in _oracle:
        img = _image(kind, v)
        with _oracle_mode(mode) as O:
            _oracle[(kind, v, mode)] = (O.lsd_detect(img),) + tuple(O.line_extract(img, 200))
    return _oracle[(kind, v, mode)]


def region_sizes(img):
    """Sizes of all regions the oracle grows on `img` (its growth log: every region_grow call, the refinement's among them)."""
    import oracle_lib
    L = oracle_lib.load()
    cap = 1 << 20
    out = np.empty(cap, np.int32)
    L.pso_lsd_growlog.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    n = L.pso_lsd_growlog(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0], out.ctypes.data, cap)
    assert n <= cap
    sizes, p = [], 0
    while p < n and out[p] == -1:
        sizes.append(int(out[p + 1]))
        p += 2 + 3 * int(out[p + 1])
    assert p < n and out[p] == -2
    return sizes


def _same_bits(got, ref, what):
    assert got.shape == ref.shape and (got.view(np.uint32) == ref.view(np.uint32)).all(), \
        f"{what}: {len(got)} segments vs {len(ref)} of the oracle, or their bits differ"


def _check_launch(mode, kind, values, F, le=None):
    """One launch of F frames (the images of `values`, tiled), or one single-frame call per image for F = 1; every frame against the
    oracle's result for its image.  Returns the number of segments over the distinct images.  `le`: an extractor to run on (kept open)."""
    import psl_slam_amd as P
    own = le is None
    if own:
        le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=F)
        le.set_refine(mode)
    try:
        if F == 1:
            for v in values:
                img = _image(kind, v)
                ref = _oracle_result(kind, v, mode)
                what = f"{kind} {v} refine {mode}, single frame"
                _same_bits(le.lsd_detect(img), ref[0], what)
                assert_extract_equal(le(img), ref[1:], what)
        else:
            src = [values[f % len(values)] for f in range(F)]
            frames = np.ascontiguousarray(np.stack([_image(kind, v) for v in src], 0))
            d_ptr, _ = le.ctx.device_array(frames)
            try:
                le.extract_batch_device(d_ptr, F, W, H, W, W * H)
                for f, v in enumerate(src):
                    ref = _oracle_result(kind, v, mode)
                    what = f"{kind} {v} refine {mode}, frame {f} of {F}"
                    k, d, e, st = le.fetch(f)
                    assert st == 0, what
                    _same_bits(le.segments_fetch(f), ref[0], what)
                    assert_extract_equal((k, d, e), ref[1:], what)
            finally:
                le.ctx.device_free(d_ptr)
    finally:
        if own:
            le.close()
    return sum(len(_oracle_result(kind, v, mode)[0]) for v in values)


@MODES
@pytest.mark.parametrize("F", [1, 24, 66, 132])
def test_seed_angle_sweep(F, mode):
    """Every frame's one edge is one region whose seed angle is the edge's level-line angle: 24 directions, every launch regime.
    Conditions on the oracle alone: with LSD_REFINE_STD it gives exactly the edge's segment in every direction, so every seed angle
    is observable there; with LSD_REFINE_ADV the NFA test drops the rectangle of the oblique edges listed in ADV_DROPPED (they run
    into the frame's border; softer, weaker, shifted or fading edges lose the same or more directions), never an axis direction's.
    The frames it drops still go through the same growth, rectangle and NFA launches and must come out empty."""
    found = [len(_oracle_result("edge", a, mode)[0]) for a in ANGLES]
    if mode == STD:
        assert found == [1] * len(ANGLES), found
    else:
        assert found == [0 if a in ADV_DROPPED else 1 for a in ANGLES], found
    assert _check_launch(mode, "edge", ANGLES, F) == sum(found)


@MODES
def test_one_extractor_alternates_between_table_and_evaluation(mode):
    """An extractor for 66 frames takes 66 (the grower evaluates the seed vector), then 24 (k_lsd_grad fills the table, which holds at
    most 64 frames), then 66 again."""
    import psl_slam_amd as P
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=66)
    le.set_refine(mode)
    try:
        for F in (66, 24, 66):
            _check_launch(mode, "edge", ANGLES, F, le=le)
    finally:
        le.close()


def _bar_sizes():
    if "bar_sizes" not in _oracle:
        _oracle["bar_sizes"] = [region_sizes(_image("bar", n)) for n in BAR_LENGTHS]
    return _oracle["bar_sizes"]


@MODES
@pytest.mark.parametrize("F", [64, 67])
def test_region_sizes_around_the_64_lane_block(F, mode):
    """Bars of 4 .. 70 pixels, one per frame: F = 67 is one launch of <0, 0>, F = 64 runs them as launches of 64 and 3 frames of <3, 1>."""
    sizes = sorted({s for per in _bar_sizes() for s in per})
    assert min(sizes) < 4, sizes
    for r in (63, 0, 1):
        assert any(s >= 63 and s % 64 == r for s in sizes), (r, sizes)
    nseg = 0
    for lo in range(0, len(BAR_LENGTHS), F):
        part = BAR_LENGTHS[lo:lo + F]
        nseg += _check_launch(mode, "bar", part, len(part))
    assert nseg >= 2 * 40, nseg   # the two long sides of most bars
