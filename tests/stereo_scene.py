"""Rectified stereo pairs for the stereo-constructor tests (pslfe_frame_set_from_orb_stereo).  Test infrastructure, numpy only.

The left image is a tools/synth_frames.Scene view; the right image samples it at x + bf / Z(x, y) along the row (bilinear,
rounded), Z from the scene's depth_u16 (metres, times `zscale` so that wide baselines keep disparities inside the image).
The edge cases shift one textured image by a constant, leave it unchanged, shift it the wrong way, flatten it, or replace the
scene by a periodic texture."""
import numpy as np

import synth_frames as sf

# Examples/Stereo/*.yaml (and the TUM1 RGB-D camera, whose distortion checks that mvuRight stays distorted):
# (fx, fy, cx, cy, k1, k2, p1, p2, k3, bf), image size, nFeatures, depth scale of the synthetic scene
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0)
EUROC = (435.2046959714599, 435.2046959714599, 367.4517211914062, 252.2008514404297, 0, 0, 0, 0, 0, 47.90639384423901)
KITTI = (718.856, 718.856, 607.1928, 185.2157, 0, 0, 0, 0, 0, 386.1448)
GEOMETRIES = {
    "tum": dict(w=640, h=480, cam=TUM1, nfeatures=1000, zscale=1.0),
    "euroc": dict(w=752, h=480, cam=EUROC, nfeatures=1200, zscale=1.5),
    "kitti": dict(w=1241, h=376, cam=KITTI, nfeatures=2000, zscale=10.0),
}


def sample_rows(img, shift):
    """img sampled at (x + shift(x, y), y), bilinear along the row, rounded; shift: scalar or (h, w) array."""
    h, w = img.shape
    src = img.astype(np.float64)
    xs = np.arange(w, dtype=np.float64)[None, :] + np.broadcast_to(np.asarray(shift, np.float64), (h, w))
    xs = np.clip(xs, 0.0, w - 1.0)
    x0 = np.minimum(np.floor(xs).astype(np.int64), w - 2)
    a = xs - x0
    rows = np.arange(h)[:, None]
    v = (1.0 - a) * src[rows, x0] + a * src[rows, x0 + 1]
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def scene_pair(w, h, bf, zscale=1.0, style="desk", seed=7, t=0):
    """(left, right, disparity) of a Scene view: right(x, y) = left(x + bf / Z(x, y), y)."""
    sc = sf.Scene(w, h, style, seed)
    left = sc.gray(t)
    Z = sc.depth_u16(t).astype(np.float64) / 5000.0 * zscale
    d = bf / Z
    return left, sample_rows(left, d), d


def textured(w, h, seed=11):
    return sf.Scene(w, h, "desk", seed).gray(0)


def periodic(w, h, period=16):
    yy, xx = np.mgrid[0:h, 0:w]
    v = 128 + 60 * np.sin(2 * np.pi * xx / period) * np.cos(2 * np.pi * yy / period) + 40 * (((xx // period + yy // period) & 1) - 0.5)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def edge_cases(w, h):
    """name -> (left, right): the pairs every geometry runs besides the scene pair."""
    base = textured(w, h)
    flat = np.full((h, w), 128, np.uint8)
    per = periodic(w, h)
    return {
        "shift_int": (base, sample_rows(base, 12.0)),
        "shift_frac": (base, sample_rows(base, 7.4)),
        "identical": (base, base.copy()),               # disparity 0: the disparity <= 0 branch
        "wrong_way": (base, sample_rows(base, -9.0)),   # true matches lie at uR > uL: (nearly) everything rejected
        "flat_right": (base, flat),                     # textureless right image: no right keypoints
        "flat_left": (flat, base),                      # no left keypoints
        "periodic": (per, sample_rows(per, 5.0)),       # Hamming and SAD ties
    }
