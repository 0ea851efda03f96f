"""Measurement of the line half of LocalMapping at keyframe rate.
Fuse: ONE call of pslfe_kf_line_fuse_keyframes - projection of M map lines into K keyframes and the search, on the device - next to
what the library offered before for the same work: K calls of pslfe_kf_line_fuse_best on rows projected beforehand.  That projection
was the caller's host loop; here the numpy restatement of tests/kf_line_project_cases.py makes the rows and is NOT timed, which favours
the old path.  Triangulation: ONE call of pslfe_kf_line_search_for_triangulation_keyframes next to the per-neighbour composition
(2K calls of pslfe_line_frame_bf_match and the host loop).  All take host buffers and return when the results are back, so the times
are a host clock around the call(s): the median of `reps` after warm-up, the two paths alternating for two passes each and the
smaller of a path's two medians reported.  Prints one JSON line (and writes it with --out).  Also meant to run under `rocprofv3 --kernel-trace --stats -- python tools/bench_kf_line_fuse.py --quick`.

Usage: python tools/bench_kf_line_fuse.py [--keyframes 1,8,20] [--lines 200,1000] [--keylines 200] [--neighbours 10,20] [--reps 20]
                                          [--quick] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TH = 3.0


def clock(run, reps, ctx):
    for _ in range(3):
        run()
    ctx.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def measure_fuse(P, kc, lc, ctx, n, K, M, reps, rng):
    views = kc.views(nslots=1, n=max(K, 2))[:K]
    cam = kc.camera()
    kls = [lc.keylines(n, rng, octaves=lc.NLEVELS) for _ in range(K)]
    descs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for _ in range(K)]
    ml, mld = lc.map_lines(M, views, seed=int(rng.integers(1 << 30)), nbehind=0)
    third = M // 3                                           # a third of the map lines lie on keylines of keyframe 0
    take = rng.integers(0, n, third)
    ml[:third], mld[:third] = lc.lines_onto(kls[0][take], descs[0][take], views[0]["Tcw"], cam, rng)
    rows, _, stop, why = lc.restate_line_project(views, ml, cam, lc.BOUNDS, lc.SCALE_LINE, TH)
    kf = P.KeyFrameMatcher(ctx)
    out = {}

    def set_call():
        out["set"] = kf.LineFuseKeyFrames(views["Tcw"], kls, descs, ml, mld, cam, lc.BOUNDS, lc.SCALE_LINE, lc.LOG_SCALE, TH)

    def per_keyframe_calls():
        out["single"] = [kf.LineFuse(kls[k], descs[k], rows[k], mld) for k in range(K)]

    a1, b1 = clock(set_call, reps, ctx), clock(per_keyframe_calls, reps, ctx)
    a2, b2 = clock(set_call, reps, ctx), clock(per_keyframe_calls, reps, ctx)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        set_call()
    ctx.synchronize()
    stage = {s: ctx.stage_time(s)[0] / reps for s in ("kf.line_project", "kf.line_fuse_set")}
    ctx.profile(False)
    bi, bd, drows, dstop = out["set"]
    same = sum(int((bi[k] == out["single"][k][0]).all() and (bd[k] == out["single"][k][1]).all()) for k in range(K))
    a, b = min(a1[0], a2[0]), min(b1[0], b2[0])
    return dict(keylines=n, keyframes=K, lines=M, rows=int(K * M), rows_kept=int((why == lc.KEPT).sum()), fused=int((bd <= 50).sum()),
                set_call_ms=dict(median=a, runs=[a1, a2]), line_fuse_best_calls_ms=dict(median=b, runs=[b1, b2]), stage_ms=stage,
                ratio_calls_over_set=b / a, rows_equal_restatement=bool(drows.tobytes() == rows.tobytes() and (dstop == stop).all()),
                keyframes_with_equal_results=same)


def measure_tri(P, ctx, n, K, reps, rng):
    import kf_scene as ks
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    neigh = [np.concatenate([ks.noisy_desc(d1[:n * 3 // 4], rng, flips=16)[rng.permutation(n * 3 // 4)],
                             rng.integers(0, 256, (n - n * 3 // 4, 32), dtype=np.uint8)]) for _ in range(K)]
    has1 = (rng.random(n) < 0.2).astype(np.uint8)
    has2 = [(rng.random(n) < 0.2).astype(np.uint8) for _ in range(K)]
    lm = P.LSDmatcher(0.95, True, ctx=ctx)
    out = {}

    def set_call():
        out["set"] = lm.SearchForTriangulationKeyFrames(d1, neigh, has1, has2, lm.TH_LOW, True)

    def per_neighbour_calls():
        out["single"] = [lm.SearchForTriangulation(d1, neigh[k], has1, has2[k], lm.TH_LOW, True) for k in range(K)]

    a1, b1 = clock(set_call, reps, ctx), clock(per_neighbour_calls, reps, ctx)
    a2, b2 = clock(set_call, reps, ctx), clock(per_neighbour_calls, reps, ctx)
    nm, match = out["set"]
    same = sum(int(nm[k] == out["single"][k][0] and (match[k] == out["single"][k][1]).all()) for k in range(K))
    a, b = min(a1[0], a2[0]), min(b1[0], b2[0])
    return dict(lines=n, neighbours=K, matches=int(nm.sum()), set_call_ms=dict(median=a, runs=[a1, a2]),
                frame_bf_match_calls_ms=dict(median=b, runs=[b1, b2]), ratio_calls_over_set=b / a, neighbours_with_equal_results=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="1,8,20")
    ap.add_argument("--lines", default="200,1000")
    ap.add_argument("--keylines", type=int, default=200)
    ap.add_argument("--neighbours", default="10,20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import kf_line_project_cases as lc
    import kf_project_cases as kc
    import psl_slam_amd as P
    ctx = P.default_context()
    Ks = [8] if a.quick else [int(v) for v in a.keyframes.split(",")]
    Ms = [200] if a.quick else [int(v) for v in a.lines.split(",")]
    Ns = [10] if a.quick else [int(v) for v in a.neighbours.split(",")]
    reps = 5 if a.quick else a.reps
    rng = np.random.default_rng(5)
    fuse = [measure_fuse(P, kc, lc, ctx, a.keylines, K, M, reps, rng) for M in Ms for K in Ks]
    tri = [measure_tri(P, ctx, a.keylines, K, reps, rng) for K in Ns]
    res = dict(bench="kf_line_fuse", th=TH, reps=reps, fuse=fuse, triangulation=tri,
               note="ms per call chain, host clock, host buffers in and out.  Every `runs` entry is (median, min, max) of `reps` calls after 3 "
                    "warm-up runs; the two paths alternate, two passes each, and `median` - which ratio_calls_over_set uses - is the SMALLER "
                    "of a path's two pass medians.  fuse.set_call_ms: one "
                    "pslfe_kf_line_fuse_keyframes (projection on the device).  fuse.line_fuse_best_calls_ms: K calls of "
                    "pslfe_kf_line_fuse_best on rows projected beforehand by the numpy restatement of the tests; that host projection is "
                    "NOT timed, which favours the K-calls side of ratio_calls_over_set.  triangulation.set_call_ms: one "
                    "pslfe_kf_line_search_for_triangulation_keyframes; frame_bf_match_calls_ms: 2K pslfe_line_frame_bf_match calls and the "
                    "host loop of the per-neighbour composition.")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
