"""k_lbd's two sample paths (psl-slam_amd/csrc/line_kernels2.h): a wave whose line has |dL0| >= |dL1| gathers step-major through its
LDS scratch in chunks of PSL_LBD_T steps, every other wave row-major as before; and the batch entry at 7 and 9 frames (either side of
the 8 frames from which the tiled kernels of the extractor change their grid).  Every case compares the 72 floats and the 32 code bytes bit for bit with the CPU oracle
(oracle_lib.lbd_compute); two NaNs count as equal whatever their sign bit (x86 produces 0xFFC00000 for 0 / 0, a GPU may produce
0x7FC00000).  Which path a line takes is decided on the CPU by the kernel's own comparison on the oracle's sincosf (the host compile
of the kernel's), and every set of lines is asserted to hold what its case is about, so that no case passes empty."""
import ctypes as C
import os
import re

import numpy as np
import pytest

W, H = 640, 480
SIZES = [(64, 48), (640, 480), (150, 101)]      # the support region taller than the image; the bench's; a width that is no multiple of 4


def chunk_steps():
    """PSL_LBD_T as the kernel is built."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "psl-slam_amd", "csrc", "line_kernels2.h")).read()
    return int(re.search(r"^#define PSL_LBD_T (\d+)$", src, re.M).group(1))


T = chunk_steps()
LENGTHS = sorted({1, 2, 7, 8, 9, T - 1, T, T + 1, 2 * T, 2 * T + 1, 201})     # around the chunk, the row-major path's block of 8, a long line


def _keylines(ends, w=W, h=H):
    import psl_slam_amd as P
    import oracle_lib
    kls = np.zeros(len(ends), P.KEYLINE_DTYPE)
    for i, (x1, y1, x2, y2) in enumerate(ends):
        for a, b in (("startPointX", x1), ("startPointY", y1), ("endPointX", x2), ("endPointY", y2), ("sPointInOctaveX", x1),
                     ("sPointInOctaveY", y1), ("ePointInOctaveX", x2), ("ePointInOctaveY", y2)):
            kls[a][i] = b
        kls["angle"][i] = np.float32(np.arctan2(np.float32(y2) - np.float32(y1), np.float32(x2) - np.float32(x1)))
        kls["numOfPixels"][i] = oracle_lib.load().pso_line_iterator_count(w, h, *[C.c_float(v) for v in (x1, y1, x2, y2)])
        kls["class_id"][i] = i
    return kls


def step_major(kls):
    """True where k_lbd takes the step-major path: fabsf(dL0) >= fabsf(dL1) with (dL1, dL0) = sincosf(angle), floats."""
    import oracle_lib
    s, c = oracle_lib.math_eval("sincosf", np.ascontiguousarray(kls["angle"], np.float32))
    return np.abs(c) >= np.abs(s)


def _image(w=W, h=H, seed=11):
    """Gradients everywhere and of every direction: smooth blobs."""
    import synth_frames as sf
    return sf.random_gray(w, h, seed, "blobs")


def _assert_floats_equal(got, ref, what):
    """Bit patterns, except that a NaN equals a NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert (gn == rn).all(), f"{what}: NaNs in different places"
    same = (got.view(np.uint32) == ref.view(np.uint32)) | gn
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} floats differ (lines {sorted(set(np.nonzero(~same)[0].tolist()))})"


def _check(img, kls, what):
    import psl_slam_amd as P
    import oracle_lib
    desc, fdesc = P.LINEextractor().lbd_compute(img, kls, want_float=True)
    rdesc, rfdesc = oracle_lib.lbd_compute(img, kls, want_float=True)
    _assert_floats_equal(fdesc, rfdesc, what)
    np.testing.assert_array_equal(desc, rdesc, err_msg=what)
    return rdesc, rfdesc


# ---- the sets of lines ----------------------------------------------------------------------------------------------------------

def _ray(deg, n=70, cx=320.0, cy=240.0):
    """n + 1 pixels from the centre in direction deg (a multiple of 45: the end point is exact)."""
    d = {0: (1, 0), 45: (1, 1), 90: (0, 1), 135: (-1, 1), 180: (-1, 0), -90: (0, -1), -45: (1, -1), -135: (-1, -1)}[deg]
    return (cx, cy, cx + n * d[0], cy + n * d[1])


def angle_lines():
    return _keylines([_ray(d) for d in (0, 90, 180, -90, 45, 135)])


def boundary_lines():
    """The float angles up to two ulps either side of the four diagonals: |dL0| == |dL1| lies among them."""
    kls, ang = [], []
    for deg in (45, 135, -45, -135):
        k = _keylines([_ray(deg)])
        a0 = k["angle"][0]
        for n in (-2, -1, 0, 1, 2):
            a = a0
            for _ in range(abs(n)):
                a = np.nextafter(a, np.float32(10 if n > 0 else -10))
            kls.append(k.copy())
            ang.append(a)
    kls = np.concatenate(kls)
    kls["angle"] = np.array(ang, np.float32)
    kls["class_id"] = np.arange(len(kls))
    return kls


def length_lines(vertical=False):
    ends = [(100, 100 + i, 100, 100 + i + n - 1) if vertical else (100 + i, 100, 100 + i + n - 1, 100) for i, n in enumerate(LENGTHS)]
    return _keylines(ends)


BORDER_ENDS = [(-30, 100, 60, 103), (600, 200, 700, 195), (100, 3, 300, 5), (100, 477, 300, 474)]   # left, right, top, bottom


def border_lines():
    kls = _keylines(BORDER_ENDS + [(700, 500, 800, 505), (700, 500, 800, 505)])
    kls["numOfPixels"][5] = 37      # the line iterator finds no pixel of a line outside the image: once as it is (no sample), once with samples, all clamped
    return kls


def mixed_lines():
    """7 lines, two blocks of four waves: both blocks hold lines of both paths."""
    return _keylines([_ray(0), _ray(90, 60, 200, 100), _ray(45, 50, 400, 100), _ray(-90, 40, 500, 300), (50, 400, 250, 410), (600, 50, 610, 250), _ray(135, 64, 300, 300)])


def size_lines(w, h):
    return _keylines([(w * 0.1, h * 0.5, w * 0.9, h * 0.55), (w * 0.5, h * 0.1, w * 0.45, h * 0.9), (2, 2, w - 3, h - 3), (w - 3, h * 0.3, 1, h * 0.25),
                      (w * 0.3, h - 2, w * 0.8, h - 1)], w, h)


def batch_frames(n):
    """n frames whose keyline counts differ, none among them: flat frames, an edge down the image, boxes (edges along and down), structure scenes."""
    import synth_frames as sf
    flat = np.full((H, W), 128, np.uint8)
    down = np.full((H, W), 77, np.uint8)
    down[:, 320:] = 200

    def box(x0, y0, x1, y1):
        im = np.full((H, W), 70, np.uint8)
        im[y0:y1, x0:x1] = 200
        return im
    frames = [flat, down, box(100, 200, 540, 300), sf.Scene(W, H, "struct", 3).gray(0), box(50, 40, 600, 90), sf.Scene(W, H, "struct", 5).gray(0), flat,
              box(200, 100, 260, 400), down]
    return np.stack(frames[:n], 0)


# ---- CPU twins ------------------------------------------------------------------------------------------------------------------

def test_every_set_holds_lines_of_both_paths_cpu():
    assert step_major(angle_lines()).tolist() == [True, False, True, False, True, True]
    b = step_major(boundary_lines()).reshape(4, 5)
    assert (b.any(1) & ~b.all(1)).all(), b       # every diagonal: a step-major and a row-major line within two ulps
    k = boundary_lines()
    assert len(set(k["angle"].view(np.uint32).tolist())) == len(k)
    for vertical in (False, True):
        k = length_lines(vertical)
        assert k["numOfPixels"].tolist() == LENGTHS
        assert LENGTHS[0] == 1 and (step_major(k)[1:] != vertical).all()   # a line of one pixel has angle atan2(0, 0) = 0 either way
    m = step_major(mixed_lines())
    assert len(m) % 4 and m[:4].any() and not m[:4].all() and m[4:].any() and not m[4:].all()
    for w, h in SIZES:
        s = step_major(size_lines(w, h))
        assert s.any() and not s.all() and (size_lines(w, h)["numOfPixels"] > 0).all()


def test_border_lines_are_step_major_and_cross_their_border_cpu():
    k = border_lines()
    assert step_major(k).all()
    assert k["numOfPixels"].tolist()[4:] == [0, 37] and (k["numOfPixels"][:4] > 0).all()
    # the support region (63 rows, numOfPixels steps, centred on the line's midpoint) leaves the image on the side named
    for (x1, y1, x2, y2), n, side in zip(BORDER_ENDS, k["numOfPixels"][:4], ("left", "right", "top", "bottom")):
        mx, my = (x1 + x2) / 2, (y1 + y2) / 2
        assert {"left": mx - n / 2 < 0, "right": mx + n / 2 > W, "top": my - 31 < 0, "bottom": my + 31 > H - 1}[side]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_angles():
    _check(_image(), angle_lines(), "axes and diagonals")


@pytest.mark.gpu
def test_path_boundary():
    _check(_image(), boundary_lines(), "within two ulps of |dL0| == |dL1|")


@pytest.mark.gpu
@pytest.mark.parametrize("vertical", [False, True])
def test_lengths(vertical):
    rdesc, _ = _check(_image(), length_lines(vertical), f"numOfPixels {LENGTHS}, {'row' if vertical else 'step'}-major")
    assert len(rdesc) == len(LENGTHS)


@pytest.mark.gpu
def test_clamping_step_major():
    _check(_image(), border_lines(), "near-horizontal lines across the four borders and one outside")


@pytest.mark.gpu
def test_block_with_both_paths():
    _check(_image(), mixed_lines(), "7 lines, both paths in both blocks")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_image_sizes(w, h):
    _check(_image(w, h, 5), size_lines(w, h), f"{w} x {h}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [7, 9])
def test_batch_grids(n):
    """7 and 9 frames (k_lbd_pre and the LSD kernels run 9 on their XCD-aware grid, whose second slice of 8 holds one frame; k_lbd keeps the plain
    grid): every frame as the single-frame entry has it."""
    import psl_slam_amd as P
    frames = batch_frames(n)
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=n)
    d_ptr, _ = le.ctx.device_array(frames)
    le.extract_batch_device(d_ptr, n, W, H, W, W * H)
    single = P.LINEextractor(1, 1.2, 200, 0.0)
    counts, both = [], np.zeros(2, bool)
    for f in range(n):
        k, dsc, eq, st = le.fetch(f)
        k1, d1, e1 = single(frames[f])
        assert st == 0 and k.tobytes() == k1.tobytes() and eq.tobytes() == e1.tobytes(), f"frame {f}"
        assert dsc.tobytes() == d1.tobytes(), f"descriptors of frame {f}"
        counts.append(len(k))
        if len(k):
            s = step_major(k)
            both |= [s.any(), (~s).any()]
    le.ctx.device_free(d_ptr)
    assert counts[0] == 0 and counts[6] == 0 and min(counts[1:3]) >= 1 and max(counts) > 4 and len(set(counts)) >= 4 and both.all(), counts


def test_batch_frames_differ_in_keylines_cpu():
    import oracle_lib
    kls = [oracle_lib.line_extract(im, 200)[0] for im in batch_frames(7)]     # frames 7 and 8 are a third box and frame 1 again
    n = [len(k) for k in kls]
    assert n[0] == 0 and n[6] == 0 and min(n[1:3]) >= 1 and max(n) > 4 and len(set(n)) >= 4, n
    s = step_major(np.concatenate(kls))
    assert s.any() and (~s).any()
