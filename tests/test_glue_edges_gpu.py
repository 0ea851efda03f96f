"""The hand-built cases of tests/glue_cases.py on the device (psl-slam_amd/csrc/pslfe_glue.hip: k_line_good, k_fans_planes): every
case through FrameGlue.run and through run_batch_device, all 11 output arrays byte for byte against the sequential oracle run
with that frame's seed AND against the answers written down in the case, the batch form with the case in each of the three lane
groups of a wave beside frames of other line counts.  No output of these cases holds a NaN (check_answers asserts it), so no
byte comparison rests on a NaN payload.  test_glue_cases_cpu.py holds the cases themselves to the oracle's trace."""
import functools

import numpy as np
import pytest

import glue_cases as G

pytestmark = pytest.mark.gpu

ML, MF = 64, 192
SMALL = {c["name"]: c for c in G.small_cases()}
OTHER = {c["name"]: c for c in G.other_cases()}


def _same(a, b, what):
    for k in G.KEYS:
        assert a[k].shape == b[k].shape, (what, k, a[k].shape, b[k].shape)
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


@functools.lru_cache(maxsize=None)
def _glue():
    import psl_slam_amd as P
    return P.FrameGlue(max_lines=ML, max_fans=MF, max_batch=3)


@functools.lru_cache(maxsize=None)
def _oracle(name, seed):
    import oracle_lib
    c = SMALL.get(name) or OTHER.get(name) or _extra()[name]
    return oracle_lib.frame_glue(c["kls"], c["fans"], c["depth"], c["cam"], seed=seed, depth_stride=c["depth_stride"])


@functools.lru_cache(maxsize=None)
def _extra():
    """fillers (frames of other line counts that ride in the other groups of the wave) per image size, and the stale_rows frames"""
    out = {}
    for w, h, x0 in ((64, 48, 10.25), (32, 24, 10.25), (640, 480, 100.25)):
        full = G.lengths(w=w, h=h, x0=x0)
        for n in (9, 5):
            c = dict(full, name=f"filler{n}_{w}x{h}", kls=full["kls"][:n], accepted=full["accepted"][:n], counts=full["counts"][:n])
            out[c["name"]] = c
    for c in (G.stale_rows_first(), G.stale_rows_second()):
        out[c["name"]] = c
    return out


def _run_batch(g, frames, seed0, fan_stride=None, nkl=None, nfans=None):
    """frames: cases of one image size.  One launch of run_batch_device on handle g; returns the fetched dict of every frame."""
    import psl_slam_amd as P
    ctx = P.default_context()
    F, fs = len(frames), fan_stride or g.max_fans
    w, h = frames[0]["w"], frames[0]["h"]
    kls = np.zeros((F, g.max_lines), P.KEYLINE_DTYPE)
    fans = np.zeros((F, fs, 4), np.float32)
    cnt = np.zeros((2, F), np.int32)
    depth = np.zeros((F, h, w), np.float32)
    for f, c in enumerate(frames):
        assert (c["w"], c["h"]) == (w, h) and c["depth_stride"] is None
        k, fa = c["kls"][:g.max_lines], c["fans"][:fs]
        kls[f, :len(k)], fans[f, :len(fa)], depth[f] = k, fa, c["depth"]
        cnt[0, f], cnt[1, f] = len(c["kls"]), len(c["fans"])
    if nkl is not None:
        cnt[0] = nkl
    if nfans is not None:
        cnt[1] = nfans
    ptrs = [ctx.device_array(a)[0] for a in (kls, fans, cnt[0], cnt[1], depth)]
    try:
        g.run_batch_device(F, ptrs[0], g.max_lines, ptrs[2], ptrs[1], fs, ptrs[3], ptrs[4], w, h, frames[0]["cam"], seed0=seed0 % 2 ** 32)
        got = [g.fetch(f, min(len(c["kls"]), g.max_lines)) for f, c in enumerate(frames)]
        ctx.synchronize()
    finally:
        for p in ptrs:
            ctx.device_free(p)
    return got


def _in_every_group(g, case, seed):
    """the case in group 0, 1 and 2 of one wave, seeded with `seed` each time (frame f is seeded seed0 + f), beside the two fillers"""
    size = f"{case['w']}x{case['h']}"
    fill = [_extra()[f"filler9_{size}"], _extra()[f"filler5_{size}"]]
    if case["cam"] != fill[0]["cam"]:   # a batch has one camera: the fillers take the case's
        fill = [dict(c, cam=case["cam"], name=f"{c['name']}_cam_of_{case['name']}") for c in fill]
        _extra().update({c["name"]: c for c in fill})
    want = _oracle(case["name"], seed)
    for pos in range(3):
        frames = fill[:pos] + [case] + fill[pos:]
        got = _run_batch(g, frames, seed - pos)
        for f, (c, r) in enumerate(zip(frames, got)):
            _same(r, _oracle(c["name"], (seed - pos + f) % 2 ** 32), f"{case['name']} in group {pos}: frame {f} ({c['name']})")
        G.check_answers(case, got[pos])
    return want


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_case_host_and_batch(name):
    """64x48: FrameGlue.run == oracle == the written answers; run_batch_device the same in every group of the wave; host == device"""
    case = SMALL[name]
    for seed in case["seeds"]:
        host = _glue().run(case["kls"], case["fans"], case["depth"], case["cam"], seed=seed)
        _same(host, _oracle(name, seed), f"{name} seed {seed} (host form)")
        G.check_answers(case, host)
        _in_every_group(_glue(), case, seed)


@pytest.mark.parametrize("name", ["borders_32x24", "borders_640x480", "slant", "slant_flat"])
def test_other_sizes_host_and_batch(name):
    case = OTHER[name]
    host = _glue().run(case["kls"], case["fans"], case["depth"], case["cam"], seed=1)
    _same(host, _oracle(name, 1), f"{name} (host form)")
    G.check_answers(case, host)
    _in_every_group(_glue(), case, 1)


def test_depth_stride():
    """rows 647 floats apart with another wall in the padding: the answers of the tight image"""
    case = OTHER["stride"]
    assert case["depth"].strides == (4 * 647, 4) and case["depth"].base[0, 640] == 0.5
    got = _glue().run(case["kls"], case["fans"], case["depth"], case["cam"], seed=1, depth_stride=case["depth_stride"])
    _same(got, _oracle("stride", 1), "stride")
    G.check_answers(case, got)
    tight = _glue().run(case["kls"], case["fans"], np.ascontiguousarray(case["depth"]), case["cam"], seed=1)
    _same(got, tight, "stride vs tight")


def test_batch_clamps_counts_to_strides():
    """fan_stride = 96 under max_fans = 128, nfans[f] = 130 > fan_stride, nkl[f] = 70 > kl_stride = 64: both counts are clamped
    (include/pslfe.h), so the frame is its first 64 lines and its first 96 fan rows"""
    import oracle_lib
    import psl_slam_amd as P
    fo = SMALL["fan_order"]
    g = P.FrameGlue(max_lines=ML, max_fans=128, max_batch=3)
    lines = np.concatenate([fo["kls"], G.full_groups()["kls"], G.lengths()["kls"]] * 3)[:70]   # 70 lines, the crossing pair first
    frame = dict(fo, name="clamped", kls=lines)
    for pos in range(3):
        fill = [_extra()["filler9_64x48"], _extra()["filler5_64x48"]]
        frames = fill[:pos] + [frame] + fill[pos:]
        nkl = [len(c["kls"]) for c in frames]
        nf = [len(c["fans"]) for c in frames]
        assert nkl[pos] == 70 and nf[pos] == 130
        got = _run_batch(g, frames, 5, fan_stride=96, nkl=nkl, nfans=nf)[pos]
        ref = oracle_lib.frame_glue(lines[:64], fo["fans"][:96], fo["depth"], fo["cam"], seed=5 + pos)
        _same(got, ref, f"clamped frame in group {pos}")
        assert got["xy"][:, 0].tolist() == [0, 63, 64, 65] and len(got["planes"]) == 1


def test_full_group_beside_lane_63():
    """the third group of the wave (lanes 42 .. 62, lane 63 riding along) holds a frame whose lines all have 21 valid samples"""
    case = SMALL["full_groups"]
    assert all(n == 21 for n in case["np"])
    frames = [_extra()["filler5_64x48"], SMALL["holes"], case]
    got = _run_batch(_glue(), frames, 1)
    for f, (c, r) in enumerate(zip(frames, got)):
        _same(r, _oracle(c["name"], 1 + f), c["name"])
    G.check_answers(case, got[2])


def test_fan_rows_past_the_line_count():
    """A fan row that names a line in [nkl[f], kl_stride) must not read what an earlier launch left in that row of mvLines3D
    (include/pslfe.h, fan-index contract).  First a batch of frames with 64 good lines whose rows 40 and 41 would cross row 3 of the
    second batch; then frames of 10 lines with fan rows (3, 40), (40, 41), (3, 5): only the last can give a crossing, the result is
    the oracle's on the 10 lines without the two rows, and a fresh handle gives the same bytes."""
    import oracle_lib
    import psl_slam_amd as P
    first, second = _extra()["stale_rows_first"], _extra()["stale_rows"]
    g = P.FrameGlue(max_lines=ML, max_fans=MF, max_batch=3)
    got1 = _run_batch(g, [first] * 3, 1)
    for f, r in enumerate(got1):
        _same(r, _oracle("stale_rows_first", 1 + f), f"first batch, frame {f}")
        assert len(r["pair"]) == 2   # rows 40 and 41 do cross row 3: the stale rows are loaded
    got2 = _run_batch(g, [second] * 3, 1)
    fresh = _run_batch(P.FrameGlue(max_lines=ML, max_fans=MF, max_batch=3), [second] * 3, 1)
    for f in range(3):
        only = oracle_lib.frame_glue(second["kls"], second["fans"][2:], second["depth"], second["cam"], seed=1 + f)
        assert got2[f]["pair"].tolist() == [[3, 5]], (f"frame {f}: crossings", got2[f]["pair"].tolist())
        _same(got2[f], only, f"second batch, frame {f}")
        _same(got2[f], _oracle("stale_rows", 1 + f), f"second batch vs the oracle with the rows, frame {f}")
        _same(fresh[f], got2[f], f"fresh handle, frame {f}")
        G.check_answers(second, got2[f])
