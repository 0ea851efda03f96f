"""The launch regimes of the batched line extractor (pslfe_line.hip: run_lsd) on the dense 'sticks' scene of the headline bench and on
adversarial inputs.  A launch of F frames takes:
  F <= 64 (PSL_GROW_HELPER_FRAMES)  k_lsd_grow4<3, 1>: helper waves, the `used` bits in LDS
  F >= 64                           the many-frames NFA grids (PSL_NFA_COUNT_WGS count workgroups, one select workgroup per frame)
  F > 64                            k_lsd_grow4<0, 0>: `used` in memory, frames in k_frame_order's order (heaviest first)
  F > 2048 (PSL_LSD_SUBBATCH)       scale / gradient in sub-batches; a last one of fewer than 8 frames on the non-XCD grids
Every frame of a launch is compared byte for byte with the single-frame extractor on the same image (one frame per launch, pinned to
the oracle in test_line_gpu.py), and sampled frames directly with the CPU oracle (oracle/line_oracle.cpp), in the launch's refine
mode: keylines, LBD rows, line equations and the fans of the batched pairing."""
import contextlib
import time
import zlib

import numpy as np
import pytest

import synth_frames as sf
from line_cases import ADV, STD, RAMP_CASES, adversarial_images, assert_extract_equal, ramp_image

try:   # PyTorch's HIP runtime before libpslfe's in a process that uses both (tests/test_gather_gpu.py; test 1d runs the torch pipeline)
    import torch
    torch.cuda.is_available()
except Exception:
    pass

pytestmark = pytest.mark.gpu

W, H = 640, 480
STICKS = (13, 14)            # seeds of the two dense scenes
MERGE_NMAX = 4096            # PSL_MERGE_NMAX (line_kernels2.h): raw segments per frame the merge takes
LSD_SUBBATCH = 2048          # PSL_LSD_SUBBATCH (line_kernels.h)
FAN_R, FAN_THR = 20.0, np.float32(np.pi / 4)
MODES = pytest.mark.parametrize("mode", [ADV, STD], ids=["adv", "std"])

# built once per module: a 'sticks' Scene costs ~8 s of CPU, a frame of it ~0.05 s
_scenes, _frames, _sets, _single, _single_le, _oracle = {}, {}, {}, {}, {}, {}


def _scene(style, seed):
    if (style, seed) not in _scenes:
        _scenes[(style, seed)] = sf.Scene(W, H, style, seed)
    return _scenes[(style, seed)]


def _frame(style, seed, t):
    if (style, seed, t) not in _frames:
        _frames[(style, seed, t)] = _scene(style, seed).gray(t)
    return _frames[(style, seed, t)]


@contextlib.contextmanager
def _oracle_mode(mode):
    import oracle_lib
    oracle_lib.set_lsd_refine(mode)
    try:
        yield oracle_lib
    finally:
        oracle_lib.set_lsd_refine(ADV)


def _lines(kls):
    if len(kls) == 0:
        return np.zeros((0, 4), np.float32)
    return np.stack([kls[n] for n in ("startPointX", "startPointY", "endPointX", "endPointY")], 1).astype(np.float32)


def _oracle_result(name, img, mode):
    """(keylines, LBD, lineEq, fans) of the CPU oracle."""
    if (name, mode) not in _oracle:
        h, w = img.shape
        with _oracle_mode(mode) as O:
            k, d, e = O.line_extract(img, 200)
            _oracle[(name, mode)] = (k, d, e, O.lil_pair(_lines(k), FAN_R, FAN_THR, w, h))
    return _oracle[(name, mode)]


def _single_result(name, img, mode):
    """(keylines, LBD, lineEq, fans) of the single-frame extractor (k_lsd_grow4<3, 1>, the one-frame NFA grids)."""
    if (name, mode) not in _single:
        import psl_slam_amd as P
        h, w = img.shape
        if mode not in _single_le:
            _single_le[mode] = P.LINEextractor(1, 1.2, 200, 0.0)
            _single_le[mode].set_refine(mode)
        le = _single_le[mode]
        k, d, e = le(img)
        _single[(name, mode)] = (k, d, e, le.pair(_lines(k), FAN_R, FAN_THR, w, h))
    return _single[(name, mode)]


def _run_batch(le, frames):
    """One launch over frames [F][h][w] + the batched pairing -> per frame (keylines, LBD, lineEq, fans, status)."""
    F, h, w = frames.shape
    d_ptr, _ = le.ctx.device_array(np.ascontiguousarray(frames))
    try:
        le.extract_batch_device(d_ptr, F, w, h, w, w * h)
        le.pair_batch_device(FAN_R, FAN_THR)
        out = []
        for f in range(F):
            k, d, e, st = le.fetch(f)
            out.append((k, d, e, le.fans_fetch(f), st))
    finally:
        le.ctx.device_free(d_ptr)
    return out


def _equal(got, ref, what):
    assert_extract_equal(got[:3], ref[:3], what)
    assert got[3].tobytes() == ref[3].tobytes(), f"{what}: fans differ ({len(got[3])} vs {len(ref[3])} rows)"


def _crc(r):
    return zlib.crc32(r[0].tobytes()) ^ zlib.crc32(r[1].tobytes()) ^ zlib.crc32(r[2].tobytes()) ^ zlib.crc32(r[3].tobytes())


def _extractor(mode, max_batch):
    import psl_slam_amd as P
    le = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=max_batch)
    le.set_refine(mode)
    return le


def _launch_set():
    """21 distinct 640x480 frames: 2 'sticks' scenes x 8 time steps, a 'struct' and a 'desk' frame, a constant frame (no gradient: weight 0,
    the lightest order class, no seeds), smoothed-noise blobs (the heaviest order class: 170 k defined pixels against 88 k of 'sticks') and a
    'sticks' frame under that texture (heavy, with keylines in both refine modes)."""
    if "640" not in _sets:
        names, imgs = [], []
        for s in STICKS:
            for t in range(8):
                names.append(f"sticks{s}/{t}")
                imgs.append(_frame("sticks", s, t))
        blobs = sf.random_gray(W, H, 12, "blobs")
        mixed = np.clip(0.75 * _frame("sticks", STICKS[0], 0).astype(np.float64) + 0.5 * (blobs.astype(np.float64) - 128), 0, 255).astype(np.uint8)
        for name, img in (("struct", _frame("struct", 3, 0)), ("desk", _frame("desk", 4, 0)), ("const", np.full((H, W), 93, np.uint8)),
                          ("blobs", blobs), ("sticks+blobs", mixed)):
            names.append(name)
            imgs.append(img)
        _sets["640"] = names, imgs
    return _sets["640"]


HEAVY = ("blobs", "sticks+blobs")


@MODES
@pytest.mark.parametrize("F", [63, 64, 65])
def test_launch_size_boundaries_on_the_dense_scene(F, mode):
    """F = 63: <3, 1> and the few-frames NFA grids; 64: <3, 1> with the many-frames NFA grids; 65: <0, 0>, k_frame_order and the
    many-frames grids.  Every frame equals the single-frame extractor; the 'sticks' frames, the heavy frames and the last frame of the
    launch equal the oracle."""
    names, imgs = _launch_set()
    with _oracle_mode(mode) as O:   # a frame that overflows the merge's segment list belongs in an overflow test, not here
        for name in HEAVY:
            assert len(O.lsd_detect(imgs[names.index(name)])) < MERGE_NMAX, name
    src = [i % len(imgs) for i in range(F)]
    got = _run_batch(_extractor(mode, F), np.stack([imgs[i] for i in src], 0))
    for f, i in enumerate(src):
        what = f"F={F} refine {mode} frame {f} ({names[i]})"
        assert got[f][4] == 0, what
        _equal(got[f], _single_result(names[i], imgs[i], mode), what + " vs single frame")
        if names[i].startswith("sticks") or names[i] in HEAVY or f == F - 1:
            _equal(got[f], _oracle_result(names[i], imgs[i], mode), what + " vs oracle")
    assert len(got[names.index("const")][0]) == 0
    sticks = [len(got[f][0]) for f, i in enumerate(src) if names[i].startswith("sticks")]
    assert np.mean(sticks) >= 150 and len(got[names.index("sticks+blobs")][0]) > 20, (np.mean(sticks), len(got[names.index("sticks+blobs")][0]))


@MODES
def test_adversarial_inputs_through_the_many_frames_grow_kernel(mode):
    """The queue-order images of test_line_gpu.py and the noisy ramps whose reduce_region_radius starts on most of the image, through
    k_lsd_grow4<0, 0> (`used` in memory): one launch of 65 frames per geometry, its distinct images tiled.  Twins are byte-identical and
    one occurrence of every image equals the oracle: its LSD segment list (the ramps give segments but no keylines) and its keylines,
    LBD rows, line equations and fans."""
    groups = {}
    for name, img in adversarial_images().items():
        groups.setdefault(img.shape, []).append((name, np.ascontiguousarray(img)))
    for w, h, noise, seed in RAMP_CASES:
        groups.setdefault((h, w), []).append((f"ramp {w}x{h} {noise} {seed}", ramp_image(w, h, noise, seed)))
    assert sorted(groups) == [(36, 36), (40, 40), (200, 640), (300, 400)]
    F = 65
    le = _extractor(mode, F)
    nkl = nseg = 0
    for shape, items in groups.items():
        src = [i % len(items) for i in range(F)]
        got = _run_batch(le, np.stack([items[i][1] for i in src], 0))
        segs = [le.segments_fetch(f) for f in range(F)]
        last = {}
        for f, i in enumerate(src):
            assert got[f][4] == 0, (shape, f)
            last[i] = f
        for f, i in enumerate(src):
            assert _crc(got[f]) == _crc(got[last[i]]) and segs[f].tobytes() == segs[last[i]].tobytes(), \
                f"{items[i][0]} refine {mode}: frame {f} differs from its twin {last[i]}"
        with _oracle_mode(mode) as O:
            ref_segs = {i: O.lsd_detect(items[i][1]) for i in last}
        for i, f in last.items():
            what = f"{items[i][0]} refine {mode} frame {f}"
            assert segs[f].shape == ref_segs[i].shape and (segs[f].view(np.uint32) == ref_segs[i].view(np.uint32)).all(), \
                f"{what}: {len(segs[f])} segments vs {len(ref_segs[i])} of the oracle, or their bits differ"
            _equal(got[f], _oracle_result(items[i][0], items[i][1], mode), what + " vs oracle")
            nkl += len(got[f][0])
            nseg += len(segs[f])
    assert nkl > 30 and nseg > 200, (nkl, nseg)


def _small_set():
    """51 distinct 320x240 frames: 3 crops of each of the 16 'sticks' frames, then the blobs (heaviest) and the blobs-under-sticks frame,
    then a constant one (lightest)."""
    if "320" not in _sets:
        names, imgs = [], []
        big_names, big = _launch_set()
        for n, img in zip(big_names[:16], big[:16]):
            for y, x in ((0, 0), (120, 160), (240, 320)):
                names.append(f"{n} @{x},{y}")
                imgs.append(np.ascontiguousarray(img[y:y + 240, x:x + 320]))
        names += ["blobs320", "sticks+blobs320", "const320"]
        imgs += [sf.random_gray(320, 240, 12, "blobs"), np.ascontiguousarray(big[big_names.index("sticks+blobs")][120:360, 160:480]),
                 np.full((240, 320), 93, np.uint8)]
        _sets["320"] = names, imgs
    return _sets["320"]


@MODES
def test_sub_batch_boundary_2053_frames(mode):
    """F = 2048 + 5: scale and gradient run in two sub-batches (the second at frame offset 2048 of the input and of d_weight, 5 frames:
    the non-XCD grids) and k_frame_order ranks more than 1024 frames.  Every frame equals the single-frame result of its source image,
    a second run is byte-identical, and frames 0, 2047, 2048, 2052 and the heaviest and lightest ones equal the oracle."""
    names, imgs = _small_set()
    n, F = len(imgs), LSD_SUBBATCH + 5
    off = (n - 3 - LSD_SUBBATCH) % n   # the second sub-batch: blobs, sticks+blobs, constant, then two crops
    src = [(f + off) % n for f in range(F)]
    assert [names[src[f]] for f in range(LSD_SUBBATCH, LSD_SUBBATCH + 3)] == ["blobs320", "sticks+blobs320", "const320"]
    batch = np.ascontiguousarray(np.stack([imgs[i] for i in src], 0))
    want = [_crc(_single_result(names[i], imgs[i], mode)) for i in range(n)]
    le = _extractor(mode, F)
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.time()
    runs = []
    for rep in range(2):
        got = _run_batch(le, batch)
        if rep == 0:
            print(f"2053 x 320x240, refine {mode}: extractor allocation {(free0 - torch.cuda.mem_get_info()[0]) / 2**30:.2f} GiB "
                  f"(device free memory before / after), {time.time() - t0:.1f} s per launch + fetch")
        for f in range(F):
            assert got[f][4] == 0, f
            assert _crc(got[f]) == want[src[f]], f"frame {f} ({names[src[f]]}) differs from the single-frame result of its image"
        runs.append([_crc(r) for r in got])
    assert runs[0] == runs[1], "a second run of the same launch differs"
    counts = [len(r[0]) for r in got]
    check = {0, LSD_SUBBATCH - 1, LSD_SUBBATCH, F - 1, int(np.argmax(counts)), int(np.argmin(counts))}
    for f in sorted(check):
        _equal(got[f], _oracle_result(names[src[f]], imgs[src[f]], mode), f"2053-frame launch refine {mode} frame {f} ({names[src[f]]}) vs oracle")
    assert min(counts) == 0 and max(counts) > 30


def test_batched_step_on_the_dense_scene():
    """tools/batch_pipeline.py's step (ORB, window match, lines, pairing, line match, glue) over 96 frames = 2 'sticks' scenes x 48
    consecutive time steps, depth a tilted plane per scene as the bench builds it: the headline load through k_lsd_grow4<0, 0>.  Sampled
    frames (the ends, the scene cut, the most and the fewest keylines) equal the oracle."""
    import psl_slam_amd as P
    import batch_pipeline as BP
    import oracle_lib
    B, nt = 96, 48
    gray = np.ascontiguousarray(np.stack([_frame("sticks", s, t) for s in STICKS for t in range(nt)], 0))
    plane = [oracle_lib.depth_to_float(_scene("sticks", s).depth_u16(0), np.float32(1.0 / 5000.0)) for s in STICKS]
    depth = np.ascontiguousarray(np.stack([plane[f // nt] for f in range(B)], 0))
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    pipe = BP.BatchPipeline(P, torch, dev, stream, 0, B, W, H, lines=True)
    d_gray, d_depth = torch.from_numpy(gray).to(dev), torch.from_numpy(depth).to(dev)
    pipe.step(d_gray.data_ptr(), d_depth.data_ptr())
    torch.cuda.synchronize(dev)
    counts = [len(pipe.le.fetch(f)[0]) for f in range(B)]
    assert np.mean(counts) >= 150, np.mean(counts)
    cache = {}
    frames = sorted({0, 1, 24, nt - 1, nt, 71, B - 1, int(np.argmax(counts)), int(np.argmin(counts))})
    for f in frames:
        pf = (f - 1) % B
        ref = BP.oracle_frame((pf, gray[pf]), (f, gray[f]), depth[f], f, W, H, True, pipe.cam, cache=cache)
        BP.compare_frame(pipe.fetch_frame(f), ref, f"frame {f}: ")
    print(f"batched step, 96 'sticks' frames: {np.mean(counts):.1f} keylines per frame ({min(counts)} - {max(counts)}), frames {frames} equal the oracle")
