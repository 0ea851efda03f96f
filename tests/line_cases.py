"""Inputs and comparisons of the line extractor tests: the LSD refinement modes, the ramp and adversarial images, and the bit-for-bit
comparison of keylines, descriptors and line equations.  Shared by tests/test_line_gpu.py and tests/test_line_batch_regimes_gpu.py."""
import numpy as np

ADV, STD = 2, 1   # LSD_REFINE_ADV (the default), LSD_REFINE_STD


RAMP_CASES = [(40, 40, 0.3, 0), (40, 40, 0.3, 9), (40, 40, 0.3, 14), (40, 40, 0.45, 5), (40, 40, 0.6, 2), (40, 40, 0.6, 3), (40, 40, 0.8, 6),
              (36, 36, 0.6, 21), (36, 36, 0.8, 17)]   # (w, h, noise, seed)


def ramp_image(w, h, noise, seed):
    """A noisy diagonal ramp: one LSD region is most of the image (test_lsd_reduce_region_radius_on_a_queue_of_most_of_the_image)."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(254.0 / (w + h - 2) * (xx + yy) + np.random.default_rng(seed).normal(0, noise, (h, w)), 0, 255).astype(np.uint8)


def adversarial_images():
    """Inputs that stress the queue order of the region growing rather than look like a room: rings (regions that turn and close on
    themselves), stripes of every thickness in both diagonals (frontiers several entries wide, growth up and to the left of the seed),
    smoothed noise (blobs, many tiny regions), a checker board (corners everywhere), raw noise, and a frame that touches all four
    borders."""
    import synth_frames as sf
    h, w = 300, 400
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = {}
    r = np.hypot(xx - 190.3, yy - 140.7)
    out["rings"] = np.clip(128 + 100 * np.sin(r / 3.1), 0, 255).astype(np.uint8)
    st = np.zeros((h, w))
    for k, (t, s) in enumerate([(1, 1), (2, -1), (3, 1), (5, -1), (8, 1), (13, -1)]):
        d = (xx + s * yy * (0.35 + 0.2 * k)) - (40 + 55 * k) - (0 if s > 0 else -120)
        st += 170.0 * (np.abs(d) < t)
    out["stripes"] = np.clip(30 + st, 0, 255).astype(np.uint8)
    out["blobs"] = sf.random_gray(w, h, 12, "blobs")
    out["checker"] = sf.random_gray(w, h, 13, "checker")
    out["noise"] = sf.random_gray(w, h, 14, "noise")
    fr = np.full((h, w), 60, np.uint8)
    fr[:3] = 250; fr[-3:] = 250; fr[:, :3] = 250; fr[:, -3:] = 250
    fr[40:44, :] = 200; fr[:, 100:103] = 10
    out["frame"] = fr
    # one region of 22 000 pixels whose breadth-first frontier is 85 entries behind the queue's end (tools/grow_stats.py): the queue's
    # LDS ring wraps 20 times; in a build with -DPSL_LSD_RING=128 the frontier is mapped from the HBM copy of the queue
    by, bx = np.mgrid[0:200, 0:640].astype(np.float64)
    out["band"] = np.rint(np.clip(4.4 * (by - 40 + 0.05 * np.abs(bx - 320)), 0, 255)).astype(np.uint8)
    return out


def kl_equal(a, b, what, skip=()):
    assert len(a) == len(b), f"{what}: {len(a)} vs {len(b)} keylines"
    for name in a.dtype.names:
        if name in skip:
            continue
        x, y = a[name], b[name]
        bad = np.flatnonzero(x.view(np.uint32) != y.view(np.uint32)) if x.dtype.kind == "f" else np.flatnonzero(x != y)
        assert bad.size == 0, f"{what}: field {name} differs at {bad[:5]}: {x[bad[:5]]} vs {y[bad[:5]]}"


def assert_extract_equal(got, ref, what):
    gk, gd, ge = got
    rk, rd, re_ = ref
    kl_equal(gk, rk, what)
    np.testing.assert_array_equal(gd, rd, err_msg=what)
    np.testing.assert_array_equal(ge.view(np.uint64), re_.view(np.uint64), err_msg=what)
