"""The front of the LSD: k_lsd_scale_tiled (Gaussian blur + 0.8 resize on doubles; staged bytes, row sums and blurred samples in
one LDS array, each written in place of the one before) and k_lsd_grad (2 x 2 gradient) at the sizes where their paths and the
in-place stage boundaries change (psl-slam_amd/csrc/line_kernels.h).  Scaled size = 0.8 x input.

  40 x 40            one partial tile, every column reflected: the byte-wise staging path
  81 x 21, 82 x 22   a second tile column of one or two pixels and a second tile row of one or two rows: the last stage of the
                     column pass writes a single row
  331 x 247          odd width, rows not 4-byte aligned
  640 x 480          all three column-pass stages in interior tiles; also as a view into a buffer with a row stride of 644 and
                     of 641, on the host (lsd_detect) and on the device, where the stride reaches the kernel: the dword staging
                     path with and without its stride condition

Every single-frame case is compared with the CPU oracle, array for array and bit for bit.  The many-frames launches (XCD-aware
grid, magnitudes stored only where the angle is defined) are compared with the single-frame result of the same image."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DEG2RAD = np.pi / 180
NOTDEF = np.float32(-1024.0)
_ref = {}
_le = {}


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _const(w, h):
    return np.full((h, w), 117, np.uint8)


def _checker(w, h):
    """Cells of one pixel, 0 / 255: the largest row sums of alternating bytes (the blur levels it: no pixel reaches the threshold)."""
    y, x = np.mgrid[0:h, 0:w]
    return (((x + y) & 1) * 255).astype(np.uint8)


def _ramp(w, h):
    """A horizontal ramp 0 .. 255 with noise of sigma 1: the gradient crosses the threshold in runs of pixels."""
    g = np.linspace(0.0, 255.0, w)[None, :] + np.random.default_rng(w * 1000 + h).normal(0.0, 1.0, (h, w))
    return np.clip(np.rint(g), 0, 255).astype(np.uint8)


SIZES = [(40, 40), (81, 21), (82, 22), (331, 247), (640, 480)]
CASES = [(f"noise {w}x{h}", lambda w=w, h=h: _noise(w, h, 100 * w + h)) for w, h in SIZES]
for _w, _h in ((640, 480), (40, 40)):
    CASES += [(f"const {_w}x{_h}", lambda w=_w, h=_h: _const(w, h)),
              (f"checker {_w}x{_h}", lambda w=_w, h=_h: _checker(w, h)),
              (f"ramp {_w}x{_h}", lambda w=_w, h=_h: _ramp(w, h))]


def _single():
    import psl_slam_amd as P
    if "one" not in _le:
        _le["one"] = P.LINEextractor()
    return _le["one"]


def _oracle(name, img):
    """(scaled, angle in radians or -1024, magnitude) of the CPU oracle, computed once per image."""
    if name not in _ref:
        import oracle_lib
        _ref[name] = oracle_lib.lsd_gradient(img)
    return _ref[name]


def _assert_oracle(got, ref, what):
    scaled, angdeg, mod = got
    rs, ra, rm = ref
    np.testing.assert_array_equal(scaled, rs, err_msg=f"{what}: scaled")
    np.testing.assert_array_equal(mod[:-1, :-1], rm[:-1, :-1], err_msg=f"{what}: magnitude")
    gang = np.where(angdeg == NOTDEF, -1024.0, angdeg.astype(np.float64) * DEG2RAD)
    np.testing.assert_array_equal(gang, ra, err_msg=f"{what}: angle")
    return int((angdeg != NOTDEF).sum())


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_single_frame_equals_the_oracle(name, make):
    img = make()
    le = _single()
    le.lsd_detect(img, cap=32768)
    ndef = _assert_oracle(le.debug_gradient(0), _oracle(name, img), name)
    print(f"{name}: {ndef} of {img.shape[0] * img.shape[1] * 16 // 25} pixels defined")
    if name.startswith("const"):
        assert ndef == 0
    elif name.startswith("noise"):
        assert ndef > 0


@pytest.mark.parametrize("stride", [644, 641])
def test_view_into_a_wider_buffer(stride):
    """On the host the stride ends at the upload; on the device it reaches the kernel (one frame per launch: every magnitude stored)."""
    import psl_slam_amd as P
    img = _noise(640, 480, 100 * 640 + 480)   # the image of CASES: one oracle run
    ref = _oracle("noise 640x480", img)
    buf = np.random.default_rng(stride).integers(0, 256, (480, stride), dtype=np.uint8)   # the padding is not zero
    buf[:, :640] = img
    view = buf[:, :640]
    assert view.strides[0] == stride and not view.flags["C_CONTIGUOUS"]
    le = _single()
    le.lsd_detect(view, cap=32768)
    _assert_oracle(le.debug_gradient(0), ref, f"host view, stride {stride}")
    dev = P.LINEextractor()
    d_ptr, _ = dev.ctx.device_array(buf)
    try:
        dev.extract_batch_device(d_ptr, 1, 640, 480, stride, stride * 480)
        _assert_oracle(dev.debug_gradient(0), ref, f"device buffer, stride {stride}")
    finally:
        dev.ctx.device_free(d_ptr)
        dev.close()


def _angle_and_magnitude(le, frame):
    """debug_gradient without the working image, which a launch of more than one sub-batch does not keep."""
    import psl_slam_amd as P
    W, H = C.c_int(), C.c_int()
    fn = P.lib().pslfe_line_debug_gradient
    assert fn(le._h, C.c_int(frame), C.byref(W), C.byref(H), None, None, None) == 0
    ang = np.zeros((H.value, W.value), np.float32)
    mod = np.zeros((H.value, W.value), np.float64)
    assert fn(le._h, C.c_int(frame), C.byref(W), C.byref(H), None, ang.ctypes.data_as(C.c_void_p), mod.ctypes.data_as(C.c_void_p)) == 0
    return ang, mod


@pytest.mark.parametrize("F,frames", [(66, (0, 65)), (2050, (2049,))], ids=["66", "2050"])
def test_many_frames_launch_equals_the_single_frame_result(F, frames):
    """82 x 22 noise images, five distinct ones in turn: 66 frames are one launch on the XCD-aware grid; 2050 frames are two
    sub-batches, the second of two frames."""
    import psl_slam_amd as P
    imgs = [_noise(82, 22, 8222 + i) for i in range(5)]
    batch = np.ascontiguousarray(np.stack([imgs[f % 5] for f in range(F)], 0))
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=F)
    d_ptr, _ = le.ctx.device_array(batch)
    try:
        le.extract_batch_device(d_ptr, F, 82, 22, 82, 82 * 22)
        got = {f: _angle_and_magnitude(le, f) for f in frames}
    finally:
        le.ctx.device_free(d_ptr)
        le.close()
    one = _single()
    for f, (ang, mod) in got.items():
        one.lsd_detect(imgs[f % 5], cap=32768)
        _, ra, rm = one.debug_gradient(0)
        defined = ra != NOTDEF
        assert defined.any(), f
        np.testing.assert_array_equal(ang, ra, err_msg=f"{F} frames, frame {f}: angle")
        np.testing.assert_array_equal(mod[defined], rm[defined], err_msg=f"{F} frames, frame {f}: magnitude where defined")
