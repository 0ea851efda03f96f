"""k_lbd behind its sample loop: the 72 band-sum chains on one lane each and the 72-float normalisation on a full wave
(psl-slam_amd/csrc/line_kernels2.h).  Every case compares the 72 floats and the 32 code bytes bit for bit with the CPU oracle
(oracle_lib.lbd_compute); two NaNs count as equal whatever their sign bit (x86 produces 0xFFC00000 for 0 / 0, a GPU may
produce 0x7FC00000).  The CPU twins assert what each case relies on, so that no case can pass empty."""
import ctypes as C

import numpy as np
import pytest

W, H = 640, 480
STEP_ENDS = [(320, 100, 320, y2) for y2 in (101, 107, 108, 109, 300)]
STEP_PIXELS = [2, 8, 9, 10, 201]     # both sides of the 8-sample block of the sample loop, and the long-line regime
BORDER_ENDS = [(0, 0, 639, 479), (-20.5, 100.2, 300.7, -10.0), (620, 5, 700, 470), (5.5, 470.25, 630.25, 478.5)]


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


def _step_image():
    img = np.full((H, W), 77, np.uint8)
    img[:, 320:] = 200
    return img


def _flat_image():
    return np.full((H, W), 128, np.uint8)


def _desk():
    import synth_frames as sf
    return sf.Scene(W, H, "desk", 12).gray(0)


def _assert_floats_equal(got, ref, what):
    """Bit patterns, except that a NaN equals a NaN."""
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, what
    gn, rn = np.isnan(got), np.isnan(ref)
    assert (gn == rn).all(), f"{what}: NaNs in different places"
    same = (got.view(np.uint32) == ref.view(np.uint32)) | gn
    assert same.all(), f"{what}: {np.count_nonzero(~same)} of {same.size} floats differ"


def _check(img, kls, what):
    import psl_slam_amd as P
    import oracle_lib
    desc, fdesc = P.LINEextractor().lbd_compute(img, kls, want_float=True)
    rdesc, rfdesc = oracle_lib.lbd_compute(img, kls, want_float=True)
    _assert_floats_equal(fdesc, rfdesc, what)
    np.testing.assert_array_equal(desc, rdesc, err_msg=what)
    return rdesc, rfdesc


# ---- CPU twins -------------------------------------------------------------------------------------------------------------

def test_step_edge_lines_take_the_clamp_cpu():
    import oracle_lib
    kls = _keylines(STEP_ENDS)
    assert kls["numOfPixels"].tolist() == STEP_PIXELS
    desc, f = oracle_lib.lbd_compute(_step_image(), kls, want_float=True)
    # 0.4 renormalised is 0.4082...: entries at 0.39 or more were cut by the clamp
    assert ((f >= 0.39).sum(1) > 0).all() and (f.max(1) > 0.4).all() and np.isfinite(f).all()
    assert desc.any(1).all()


def test_flat_image_is_the_nan_path_cpu():
    import oracle_lib
    desc, f = oracle_lib.lbd_compute(_flat_image(), _keylines(STEP_ENDS[4:]), want_float=True)
    assert np.isnan(f).all() and not desc.any()


def test_border_lines_have_pixels_cpu():
    assert (_keylines(BORDER_ENDS)["numOfPixels"] > 0).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_step_edge_lines():
    _, rf = _check(_step_image(), _keylines(STEP_ENDS), "step edge")
    assert ((rf >= 0.39).sum(1) > 0).all()


@pytest.mark.gpu
def test_flat_image():
    _, rf = _check(_flat_image(), _keylines(STEP_ENDS[4:]), "flat image")
    assert np.isnan(rf).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_ragged_last_block(n):
    """Four waves per workgroup, one line each: n lines leave idle waves beside working ones (n = 5: a second workgroup of one)."""
    ends = (STEP_ENDS + BORDER_ENDS)[:n]
    img = _step_image()
    rdesc, _ = _check(img, _keylines(ends), f"{n} lines")
    assert len(rdesc) == n


@pytest.mark.gpu
def test_border_lines():
    _check(_desk(), _keylines(BORDER_ENDS), "border lines")


@pytest.mark.gpu
def test_batch_with_0_1_and_many_keylines():
    """Frames with no keyline, one and more than four in one launch against the single-frame extractor."""
    import psl_slam_amd as P
    import synth_frames as sf
    frames = np.stack([_flat_image(), _step_image(), sf.Scene(W, H, "struct", 3).gray(0)], 0)
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=3)
    d_ptr, _ = le.ctx.device_array(frames)
    le.extract_batch_device(d_ptr, 3, W, H, W, W * H)
    single = P.LINEextractor(1, 1.2, 200, 0.0)
    counts = []
    for f in range(3):
        k, dsc, eq, st = le.fetch(f)
        k1, d1, e1 = single(frames[f])
        assert st == 0 and k.tobytes() == k1.tobytes() and eq.tobytes() == e1.tobytes()
        np.testing.assert_array_equal(dsc, d1)
        counts.append(len(k))
    assert counts[0] == 0 and counts[1] == 1 and counts[2] > 4, counts


def test_batch_frames_have_0_1_and_many_keylines_cpu():
    import oracle_lib
    import synth_frames as sf
    n = [len(oracle_lib.line_extract(im, 200)[0]) for im in (_flat_image(), _step_image(), sf.Scene(W, H, "struct", 3).gray(0))]
    assert n[0] == 0 and n[1] == 1 and n[2] > 4, n
