"""k_lil_pair (per-line rectangles once, 64 candidates per instruction, rows placed by one scan over the per-line counts, keys of the
de-duplication in LDS) and k_lil_pair_big (more than PSL_PAIR_LDSN lines) at the sizes where they change path
(psl-slam_amd/csrc/line_kernels2.h).  Every case compares bit patterns with the CPU oracle (oracle_lib.lil_pair), except the one above
the cap of raw rows, which the oracle does not have: that one is compared with what the kernel of the commit before this file gave
(tests/golden/lil_pair_overcap.npz).  The CPU twins assert what each case relies on.

Regenerate the fixture on a GPU with   PSL_WRITE_LIL_PAIR_GOLDEN=1 python tests/test_lil_pair_shapes_gpu.py"""
import os

import numpy as np
import pytest

RADIUS, FAN_THR = 20.0, np.float32(np.pi / 4)
FAN_CAP = 4096          # PSLFE_FAN_CAP (include/pslfe.h): raw rows per frame before the de-duplication
PAIR_LDSN = 256         # PSL_PAIR_LDSN: lines per frame k_lil_pair holds in LDS; more go to k_lil_pair_big
PAIR_TRIP = 64          # candidates per trip of k_lil_pair: one wave
OLD_TRIP = 128          # the kernel before tested 2 * rows candidate points in trips of 256 threads
MERGE_NMAX = 4096       # PSL_MERGE_NMAX: most lines pslfe_lil_pair accepts
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lil_pair_overcap.npz")

# every trip boundary of the new kernel, its LDS boundary and the old kernel's trip boundary, each with both neighbours
BOUNDARY_N = sorted({n + d for n in (PAIR_TRIP, 2 * PAIR_TRIP, 3 * PAIR_TRIP, PAIR_LDSN, OLD_TRIP) for d in (-1, 0, 1)})
FIELD_W = FIELD_H = 1000


def star(n, cx=320.0, cy=240.0, rng=None):
    """n lines around (cx, cy): angles spread over [0, pi) with 0.01 rad jitter, centres jittered by 3 px, radius 12 to 60."""
    rng = rng or np.random.default_rng(1)
    ang = np.arange(n) * np.pi / n + rng.normal(0, 0.01, n)
    x, y = cx + rng.normal(0, 3, n), cy + rng.normal(0, 3, n)
    c, s = np.cos(ang), np.sin(ang)
    return np.stack([x + 12 * c, y + 12 * s, x + 60 * c, y + 60 * s], 1).astype(np.float32)


def field(n, per=16, pitch=180, cols=5):
    """n lines as stars of `per` lines at well-separated centres (the last one takes a single left-over line), so that the
    number of fans stays under a quarter of the cap of raw rows."""
    rng = np.random.default_rng(1)
    out, k = [np.zeros((0, 4), np.float32)], 0
    while n > 0:
        m = n if n - per == 1 else min(per, n)
        out.append(star(m, 100 + pitch * (k % cols), 100 + pitch * (k // cols), rng))
        n, k = n - m, k + 1
    return np.concatenate(out, 0)


def crossing_pair():
    """Two lines with both endpoints inside each other's rectangle: the pair comes up four times, as (0, 1) twice and (1, 0) twice."""
    return np.array([[305, 240, 335, 240], [320, 225, 320, 255]], np.float32)


def big_field():
    """MERGE_NMAX lines: 4032 short near-horizontal ones packed so closely that most rectangle tests pass and the angle test
    rejects them, and a star of 64 below them."""
    rng = np.random.default_rng(2)
    gx, gy = np.meshgrid(np.arange(63) * 10 + 5.0, np.arange(64) * 2 + 6.0)
    a = rng.normal(0, 0.01, gx.size)
    flat = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 6 * np.cos(a), gy.ravel() + 6 * np.sin(a)], 1).astype(np.float32)
    return np.concatenate([flat, star(64, 320.0, 350.0)], 0)


def raw_row_count(lines):
    """Candidate tests that pass, in float64 (for well-conditioned lines only): endpoints of j in line i's rectangle, the two
    directions more than FAN_THR apart, the intersection in the rectangle."""
    n, rows = len(lines), 0
    L = lines.astype(np.float64)
    for i in range(n):
        c = (L[i, :2] + L[i, 2:]) / 2
        d = L[i, 2:] - L[i, :2]
        ang = np.arctan2(d[1], d[0])
        length = abs(d[1]) if abs(np.tan(ang)) > 1 else abs(d[0])
        hw, hh = int(length + 2 * RADIUS) / 2, int(2 * RADIUS) / 2
        u, v = np.array([np.cos(ang), np.sin(ang)]), np.array([np.sin(ang), -np.cos(ang)])

        def inside(p):
            return -hw <= (p - c) @ u < hw and -hh <= (p - c) @ v < hh
        for j in range(n):
            if j == i:
                continue
            e = L[j, 2:] - L[j, :2]
            t = abs(ang - np.arctan2(e[1], e[0])) % np.pi
            if t < FAN_THR or np.pi - t < FAN_THR:
                continue
            o = L[j, :2] - L[i, :2]
            X = L[i, :2] + d * (o[0] * e[1] - o[1] * e[0]) / (d[0] * e[1] - d[1] * e[0])
            rows += sum(inside(p) and inside(X) for p in (L[j, :2], L[j, 2:]))
    return rows


def _oracle(lines, w, h):
    import oracle_lib
    return oracle_lib.lil_pair(lines, RADIUS, FAN_THR, w, h)


def _check(lines, w, h, what):
    import psl_slam_amd as P
    ref = _oracle(lines, w, h)
    got = P.LINEextractor().pair(lines, RADIUS, FAN_THR, w, h)
    assert got.shape == ref.shape, f"{what}: {len(got)} fans, oracle {len(ref)}"
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=what)
    return ref


# ---- CPU twins -------------------------------------------------------------------------------------------------------------

def test_crossing_pair_is_found_four_times_and_kept_once_cpu():
    L = crossing_pair()
    fans = _oracle(L, 640, 480)
    assert raw_row_count(L) == 4 and len(fans) == 1
    assert fans[0].tolist() == [320.0, 240.0, 1.0, 0.0]     # the last occurrence: line 1's test of line 0's end point


def test_star_and_fields_stay_under_the_cap_cpu():
    assert len(_oracle(star(64), 640, 480)) == 895
    for n in BOUNDARY_N:
        L = field(n)
        fans = _oracle(L, FIELD_W, FIELD_H)
        assert len(L) == n and 0 < len(fans) * 4 < FAN_CAP, (n, len(fans))
        assert L.min() > 4 and L.max() < FIELD_W - 4
    assert BOUNDARY_N == [63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257]


def test_big_field_pairs_only_in_its_star_cpu():
    L = big_field()
    fans = _oracle(L, 640, 480)
    assert len(L) == MERGE_NMAX > PAIR_LDSN and len(fans) == 895 and (fans[:, 2:] >= MERGE_NMAX - 64).all()


def test_star_of_200_is_above_the_cap_cpu():
    assert len(_oracle(star(200), 640, 480)) > FAN_CAP   # fans are at most the raw rows: the kernel cuts these off


def test_golden_holds_results_only_cpu():
    with np.load(GOLDEN) as z:
        assert sorted(z.files) == ["fans"] and z["fans"].dtype == np.float32 and z["fans"].shape[1] == 4
        assert 0 < len(z["fans"]) <= FAN_CAP and os.path.getsize(GOLDEN) <= 64 * 1024


def test_batch_frames_have_0_1_and_about_170_lines_cpu():
    import oracle_lib
    n = [len(oracle_lib.line_extract(im, 200)[0]) for im in _batch_frames()]
    assert n[0] == 0 and n[1] == 1 and 150 < n[2] <= 200, n


def _batch_frames():
    import synth_frames as sf
    step = np.full((480, 640), 77, np.uint8)
    step[:, 320:] = 200
    return np.stack([np.full((480, 640), 128, np.uint8), step, sf.Scene(640, 480, "sticks", 14).gray(0)], 0)


# ---- GPU -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 2])
def test_smallest(n):
    assert len(_check(crossing_pair()[:n], 640, 480, f"{n} lines")) == (1 if n == 2 else 0)


@pytest.mark.gpu
def test_star_of_64():
    assert len(_check(star(64), 640, 480, "star of 64")) == 895


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOUNDARY_N)
def test_line_counts_at_the_boundaries(n):
    assert len(_check(field(n), FIELD_W, FIELD_H, f"{n} lines")) > 0


@pytest.mark.gpu
def test_more_lines_than_the_lds_layout_holds():
    assert len(_check(big_field(), 640, 480, "4096 lines")) == 895


@pytest.mark.gpu
def test_above_the_cap_of_raw_rows():
    import psl_slam_amd as P
    got = P.LINEextractor().pair(star(200), RADIUS, FAN_THR, 640, 480)
    with np.load(GOLDEN) as z:
        ref = z["fans"]
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.gpu
def test_batch_with_0_1_and_about_170_lines():
    import psl_slam_amd as P
    frames = _batch_frames()
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=3)
    d_ptr, _ = le.ctx.device_array(frames)
    le.extract_batch_device(d_ptr, 3, 640, 480, 640, 640 * 480)
    le.pair_batch_device(RADIUS, FAN_THR)
    counts = []
    for f in range(3):
        k = le.fetch(f)[0]
        lines = np.stack([k[n] for n in ("startPointX", "startPointY", "endPointX", "endPointY")], 1).astype(np.float32).reshape(-1, 4)
        fans, ref = le.fans_fetch(f), _oracle(lines, 640, 480)
        assert fans.shape == ref.shape and fans.tobytes() == ref.tobytes(), f"frame {f}"
        counts.append((len(k), len(ref)))
    assert counts[0] == (0, 0) and counts[1] == (1, 0) and counts[2][0] > 150 and counts[2][1] > 0, counts


if __name__ == "__main__" and os.environ.get("PSL_WRITE_LIL_PAIR_GOLDEN") == "1":
    # results only: the fans the library in the tree gives for the star of 200 lines (record with the commit before the kernel changes)
    import sys
    sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
    import psl_slam_amd as P
    out = P.LINEextractor().pair(star(200), RADIUS, FAN_THR, 640, 480)
    np.savez_compressed(os.environ.get("PSL_LIL_PAIR_GOLDEN_OUT", GOLDEN), fans=out)
    print(f"{len(out)} fans written")
