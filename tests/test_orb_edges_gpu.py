"""The ORB extractor outside its one tested configuration (scaleFactor 1.2, thresholds 20 / 7, aligned pointers, stride == w), bit-exact
against the oracle, stage by stage.  The cases are those of tests/orb_cases.py (pinned to the oracle by tests/test_orb_cases_cpu.py);
each reaches a path of psl-slam_amd/csrc/orb_kernels.h that the scene tests of tests/test_orb_gpu.py never take:

  k_pyr_resize_tiled   staged && fits (1.1, 1.3), staged && !fits (1.35), staged and unstaged mixed (1.5), unstaged (2.0, and level 1
                       of every unaligned device input)
  k_fast_cells4        byte tile loads (unaligned device input), the threshold floor, the per-cell fallback, the strict NMS, the
                       seams (dot and pair images with written-down answers), partial 4-pixel groups and partial, narrow and skipped
                       last cells (width sweep, last_col_*, last_row_*), the largest cell (one_big_cell)
  k_octree             <256> / <512> at kp_cap 256 / 257 / 512, cell offsets in global memory (more than 4 * BS cells), quota 0,
                       kp_cap = 4 nIni
  k_blur7              the per-byte reflect path in the tile interior (unaligned device input)
  k_orient_describe    the byte-wise orientation patch (unaligned device input)
"""
import numpy as np
import pytest

import orb_cases as oc
import synth_frames as sf
from test_orb_gpu import _assert_same_stages

pytestmark = pytest.mark.gpu

PSLFE_E_INVALID = -1


def _run_case(case):
    import psl_slam_amd as P
    import oracle_lib
    cfg, img = oc.case_config(case), oc.case_image(case)
    gpu, orc = P.ORBextractor(**cfg), oracle_lib.OracleORB(**cfg)
    got, ref = gpu(img), orc(img)
    assert len(ref[0]) > 0
    _assert_same_stages(gpu, orc, got, ref, case["nlevels"], case["name"])
    return got


@pytest.mark.parametrize("case", [c for c in oc.REGIMES if c["accept"]], ids=lambda c: c["name"])
def test_accepted_regimes_equal_the_oracle(case):
    k, _ = _run_case(case)
    if case["name"] == "th_7_20":
        # iniThFAST < minThFAST: the reference runs FAST(7) first, so corners scoring 7..19 stay.  k_fast_cells4 used minThFAST as
        # its score floor and dropped them (before the floor became min(iniTh, minTh): 260 candidates on level 0 against the
        # oracle's 1704 here, and 153 against 526 on the dot lattice)
        assert k["response"].min() < 20


def test_width_sweep_equals_the_oracle():
    for case in oc.WIDTH_SWEEP:
        _run_case(case)


@pytest.mark.parametrize("case", [c for c in oc.REGIMES if not c["accept"]], ids=lambda c: c["name"])
def test_rejected_regimes_raise(case):
    import psl_slam_amd as P
    gpu = P.ORBextractor(**oc.case_config(case))
    with pytest.raises(P.PslfeError):
        gpu(oc.case_image(case))
    if case["name"] == "cap_513":
        assert P.lib().pslfe_orb_max_keypoints(gpu._h, case["w"], case["h"]) == PSLFE_E_INVALID
    with pytest.raises(P.PslfeError):
        gpu.max_keypoints(case["w"], case["h"])


def _dots_against_both(img, expected, ini, mn, what):
    import psl_slam_amd as P
    import oracle_lib
    gpu, orc = P.ORBextractor(300, 1.2, 1, ini, mn), oracle_lib.OracleORB(300, 1.2, 1, ini, mn)
    got, ref = gpu(img), orc(img)
    gc = gpu.debug_candidates(0, 0)
    assert gc.shape == expected.shape, f"{what}: {len(gc)} candidates, {len(expected)} written down"
    np.testing.assert_array_equal(gc, expected, err_msg=f"{what}: written-down candidates")
    np.testing.assert_array_equal(gc, orc.candidates(0), err_msg=f"{what}: oracle candidates")
    _assert_same_stages(gpu, orc, got, ref, 1, what)


@pytest.fixture(scope="module")
def lattice():
    return oc.dot_lattice()


@pytest.mark.parametrize("ini,mn", [(20, 7), (7, 20), (7, 7), (40, 40), (21, 8), (255, 0)])
def test_dot_lattice_gives_the_written_down_candidates(lattice, ini, mn):
    img, dots = lattice
    _dots_against_both(img, oc.expected_candidates(dots, ini, mn), ini, mn, f"dot lattice {ini}/{mn}")


@pytest.mark.parametrize("bg,sign", [(0, 1), (255, -1)])
def test_score_ceiling(bg, sign):
    dots = [(x, y, sign * c) for x, y, c in oc.ceiling_dots()]
    _dots_against_both(oc.dot_image(dots, bg=bg), np.array([[67, 38, 254], [170, 115, 7]], np.int32), 20, 7, f"ceiling on {bg}")


def test_adjacent_pairs_follow_the_strict_nms():
    dots, hand = oc.pair_dots()
    _dots_against_both(oc.dot_image(dots), hand, 20, 7, "pairs")


# ---- unaligned device input ----------------------------------------------------------------------------------------------------
W, H = 320, 240
DEV_CFG = dict(nfeatures=500, scaleFactor=1.2, nlevels=4, iniThFAST=20, minThFAST=7)
# (name, frames, base offset, stride, frame_stride - stride * h)
LAYOUTS = [("aligned", 1, 0, 320, 0), ("base+1", 1, 1, 320, 0), ("base+2", 1, 2, 320, 0), ("base+3", 1, 3, 320, 0),
           ("stride321", 1, 0, 321, 0), ("stride322", 1, 0, 322, 0), ("stride323", 1, 0, 323, 0), ("stride324", 1, 0, 324, 0),
           ("two frames, the second unaligned", 2, 0, 320, 1), ("nine frames on the XCD grid", 9, 0, 320, 1)]


@pytest.fixture(scope="module")
def dev_frames():
    import oracle_lib
    frames = sf.stream(2, W, H, "desk", seed=31)
    refs = []
    for f in range(2):
        orc = oracle_lib.OracleORB(**DEV_CFG)
        refs.append((orc, orc(frames[f])))
    return frames, refs


def test_unaligned_device_input_equals_the_oracle(dev_frames):
    """A ROI of a larger device image: odd base pointers, odd strides, and frame strides that leave every other frame unaligned.
    Everything around the frames is noise, so a read outside a frame's rows that reaches a result shows."""
    import torch
    import psl_slam_amd as P
    frames, refs = dev_frames
    dev = torch.device("cuda", 0)
    results = {}
    for name, F, base, stride, extra in LAYOUTS:
        fstride = stride * H + extra
        host = sf.random_gray(base + F * fstride + 4096, 1, 77, "noise").reshape(-1)
        for f in range(F):
            o = base + f * fstride
            view = np.lib.stride_tricks.as_strided(host[o:], (H, W), (stride, 1))
            view[:] = frames[f % 2]
        buf = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize(dev)
        # the kernels take their dword paths only if (frame pointer | stride) is a multiple of 4.  Stride 324 is: it is the aligned
        # stride that is neither w nor a multiple of 16.  Every other layout but the first has a frame that is not, and the batches
        # have both kinds in one launch
        assert buf.data_ptr() % 256 == 0
        odd = [((base + f * fstride) | stride) & 3 != 0 for f in range(F)]
        assert any(odd) == (name not in ("aligned", "stride324")) and (F == 1 or not all(odd))
        gpu = P.ORBextractor(max_batch=F, **DEV_CFG)
        gpu.extract_batch_device(buf.data_ptr() + base, F, W, H, stride, fstride)
        for f in range(F):
            got = gpu.fetch(f, W, H)
            orc, ref = refs[f % 2]
            _assert_same_stages(gpu, orc, got, ref, DEV_CFG["nlevels"], f"{name}, frame {f}", frame=f)
            results.setdefault(f % 2, []).append((name, f, got))
        del gpu, buf
    for twin, rs in results.items():
        k0, d0 = rs[0][2]
        assert len(k0) > 300
        for name, f, (k, d) in rs[1:]:
            assert k.tobytes() == k0.tobytes() and d.tobytes() == d0.tobytes(), f"{name}, frame {f} differs from {rs[0][0]}"
