"""The hand-built cases of tests/glue_cases.py on the CPU: the restated sampler against the oracle's trace, the written answers
against the oracle, and the regime each case claims against the trace.  test_cases_reach_every_branch is a condition on the
cases themselves: it fails when a case silently stops reaching its branch.  The device runs the same cases in
test_glue_edges_gpu.py."""
import functools

import numpy as np
import pytest

import glue_cases as G
import oracle_lib as O

CASES = {c["name"]: c for c in G.all_cases() + (G.stale_rows_second(), G.stale_rows_first())}
COUNTERS = ("tried", "outside", "int_branch", "clamped", "holes", "np")


@functools.lru_cache(maxsize=None)
def _oracle(name, seed):
    c = CASES[name]
    return O.frame_glue(c["kls"], c["fans"], c["depth"], c["cam"], seed=seed, depth_stride=c["depth_stride"], trace=True)


@pytest.mark.parametrize("name", sorted(CASES))
def test_sampler_restated(name):
    """sample_line gives the oracle's per-line counts: samples tried, outside, integer branch, clamped, holes, points"""
    c = CASES[name]
    t = _oracle(name, c["seeds"][0])["line_trace"]
    for i, cnt in enumerate(c["counts"]):
        assert tuple(int(t[i][k]) for k in COUNTERS) == cnt[:6], (name, i)


def test_borders_pixel_lists():
    """the written pixel lists of the 32x24 border case and the written totals of all three sizes"""
    c = CASES["borders_32x24"]
    for i, (outside, integer, clamped, npts, pixels) in enumerate(G.BORDERS_32x24):
        cnt = c["counts"][i]
        assert (cnt[1], cnt[2], cnt[3], cnt[5], cnt[6]) == (outside, integer, clamped, npts, pixels), i
    for (w, h), tot in G.BORDERS_TOTALS.items():
        cs = CASES[f"borders_{w}x{h}"]["counts"]
        assert tuple(sum(k[j] for k in cs) for j in (0, 1, 2, 3, 5)) == tot, (w, h)
    # the clamp binds and samples fall outside: the branches the scene tests never took
    assert all(t[1] > 0 and t[3] > 0 for t in G.BORDERS_TOTALS.values())


@pytest.mark.parametrize("name", sorted(CASES))
def test_written_answers(name):
    c = CASES[name]
    for seed in c["seeds"]:
        r = _oracle(name, seed)
        G.check_answers(c, r)
        if "plane_reasons" in c:
            assert r["plane_trace"][:, 0].tolist() == c["plane_reasons"], name


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["regime"]))
def test_claimed_regime(name):
    c = CASES[name]
    t = _oracle(name, c["seeds"][0])["line_trace"]
    for i, want in c["regime"].items():
        got = {k: int(t[i][k]) for k in want}
        assert got == want, (name, "line", i)


def test_untraced_equals_traced():
    """the trace only counts: the untraced call gives the same bytes"""
    for name in ("holes", "step_11_10_seed2", "fan_order", "planes_tilt25"):
        c = CASES[name]
        a = O.frame_glue(c["kls"], c["fans"], c["depth"], c["cam"], seed=c["seeds"][0])
        b = _oracle(name, c["seeds"][0])
        for k in G.KEYS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


def test_lengths_answers_do_not_depend_on_the_order():
    """reversed, the lines draw another part of the rand() stream; every line's answer is the same"""
    for z in (2.0, 1.0):
        a, b = _oracle(f"lengths_z{z:g}", 1), _oracle(f"lengths_z{z:g}_rev", 1)
        assert a["lines3d"].tobytes() != b["lines3d"].tobytes()
        assert (np.abs(a["lines3d"]).sum(1) > 0).tolist() == (np.abs(b["lines3d"]).sum(1) > 0).tolist()[::-1]


def test_stride_equals_tight():
    c = CASES["stride"]
    tight = O.frame_glue(c["kls"], c["fans"], np.ascontiguousarray(c["depth"]), c["cam"], seed=1)
    for k in G.KEYS:
        assert tight[k].tobytes() == _oracle("stride", 1)[k].tobytes(), k
    # the padding is another wall: indexing the rows with the width would not give these answers
    wrong = O.frame_glue(c["kls"], c["fans"], c["depth"].base.reshape(-1)[:c["w"] * c["h"]].reshape(c["h"], c["w"]), c["cam"], seed=1)
    assert (np.abs(wrong["lines3d"]).sum(1) > 0).tolist() == c["accepted"][:-1] + [False]


def test_slant_canary():
    """collinear segments: a crossing from a rounding residue on the slanted wall, det == 0 exactly on the flat one"""
    r, f = _oracle("slant", 1), _oracle("slant_flat", 1)
    assert r["fan_reason"].tolist() == [O.FAN_ACCEPTED] and f["fan_reason"].tolist() == [O.FAN_DET_ZERO]
    assert len(r["planes"]) == 1
    np.testing.assert_allclose(r["normals"][0], [0.685, -0.728, 0.0], atol=5e-4)
    # the two directions agree to 6 digits: the normal is what their roundings leave
    assert np.abs(np.abs(r["lineEq"][0]) - np.abs(r["lineEq"][1])).max() < 2e-6


def test_fan_rows_outside_the_frame():
    """a fan row that names a line the frame does not have gives no crossing; the rest is as if the row were not there"""
    c = CASES["stale_rows"]
    r = _oracle("stale_rows", 1)
    assert r["fan_reason"].tolist() == [O.FAN_BAD_INDEX, O.FAN_BAD_INDEX, O.FAN_ACCEPTED]
    only = O.frame_glue(c["kls"], c["fans"][2:], c["depth"], c["cam"], seed=1)
    for k in G.KEYS:
        assert only[k].tobytes() == r[k].tobytes(), k
    neg = O.frame_glue(c["kls"], np.float32([[1, 1, -1, 3], [4.5, 4.5, 3, 5]]), c["depth"], c["cam"], seed=1, trace=True)
    assert neg["fan_reason"].tolist() == [O.FAN_BAD_INDEX, O.FAN_ACCEPTED]


# Branches no depth image can reach through the chain, named here so that the condition below stays honest:
#   FAN_DISTMID       needs end points on both sides of the camera centre (a camera wider than anything the reference runs), and falls
#                     off the end of Frame_shortestDistance upstream;
#   FAN_ZERO_CROSSING needs two lines that meet IN the camera centre, i.e. two viewing rays, which are points in the image;
#   PLANE_NOT_GOOD    needs a crossing with a rejected line, whose 3-D line is all zeros and gives det == 0 before.
UNREACHED_FAN, UNREACHED_PLANE = {O.FAN_DISTMID, O.FAN_ZERO_CROSSING}, {O.PLANE_NOT_GOOD}


def test_cases_reach_every_branch():
    runs = [_oracle(n, s) for n, c in CASES.items() for s in c["seeds"]]
    lt = np.concatenate([r["line_trace"] for r in runs])
    assert set(lt["exit_reason"].tolist()) == {O.LINE_NO_SAMPLES, O.LINE_FEW_POINTS, O.LINE_NO_VERIFIED_SET, O.LINE_SHORT_3D, O.LINE_ACCEPTED}
    for k in O.LINETRACE_DTYPE.names:
        if k != "exit_reason":
            assert lt[k].max() > 0, f"no case reaches the counter {k}"
    assert {1, 2}.issubset(set(lt["refine_grew"].tolist())), "refinement that grows once and twice"
    assert lt["iterations"].max() == 10 and ((lt["iterations"] > 1) & (lt["iterations"] < 10) & (lt["exit_reason"] == O.LINE_ACCEPTED)).any(), \
        "all ten iterations, and the `> np * 0.6` break on a later iteration"
    assert (lt["int_branch"] > lt["clamped"]).any() and (lt["clamped"] > 0).any()
    fr = set(np.concatenate([r["fan_reason"] for r in runs]).tolist())
    assert fr == set(range(5)) - UNREACHED_FAN, fr
    pt = np.concatenate([r["plane_trace"] for r in runs])
    assert set(pt[:, 0].tolist()) == set(range(4)) - UNREACHED_PLANE
    assert set(pt[:, 1].tolist()) == {0, 1}, "a plane that is flipped and one that is not"
    assert pt[:, 2].max() >= 0, "a plane made old by an earlier one"
