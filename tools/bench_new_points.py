"""First timings of CreateNewMapPoints / CreateNewMapLines2 on the device: one keyframe of `--features` features and `--lines` lines against
K neighbours.  Not gated by anything.

points  new_call_ms        ONE pslfe_kf_create_new_map_points: upload, two launches, one synchronisation.
        search_calls_ms    what the library offered before for the same keyframe: K calls of pslfe_kf_search_for_triangulation, each with
                           its upload and synchronisation, the query list of neighbour k cut down (a numpy mask, timed) to the features
                           that have no point yet.  The triangulation between two calls is NOT in this number: the state after neighbour k
                           is taken from the new call's created_by.
        host_loop_ms       the one-core loop of tools/dropin/newpoints_main.cpp (g++ -O2, best of 5) over the WHOLE stage, its own
                           sequential search included: an upper bound of the host triangulation the old path needs on top of
                           search_calls_ms.  The old path therefore costs between search_calls_ms and search_calls_ms + host_loop_ms.
lines   new_call_ms        ONE pslfe_kf_create_new_map_lines; search_call_ms: pslfe_kf_line_search_for_triangulation_keyframes alone (the
                           pair body was the caller's host loop).
Host clock around calls that return when the results are back: the median of `reps` after 3 warm-up runs, the paths alternating for two
passes and the smaller of a path's two medians reported.  Prints one JSON line (and writes it with --out).

Usage: python tools/bench_new_points.py [--features 2000] [--lines 200] [--neighbours 10,20] [--reps 20] [--quick] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
BOUNDS = (0.0, 0.0, 1024.0, 768.0)


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


def measure_points(P, nc, ctx, n, K, reps, exe):
    c = nc.general_case(seed=11, npts=n, K=K, name=f"bench-n{n}-K{K}")
    cur = c["cur"]
    grid = P.FrameGrid(max(len(s["kps"]) for s in c["store"]), K, ctx=ctx)
    for k, s in enumerate(c["store"]):
        grid.set(k, s["kps"], s["desc"], BOUNDS, s["uright"])
    kf = P.KeyFrameMatcher(ctx)
    lists = ([g["fidx"] for g in c["neigh"]], [g["taken"] for g in c["neigh"]], [g["keys"] for g in c["neigh"]], [g["depth"] for g in c["neigh"]])
    out = {}

    def new_call():
        out["new"] = kf.CreateNewMapPoints(grid, c["kf1"], cur["keysun"], cur["keys"], cur["uright"], cur["depth"], cur["taken"], c["nb"], *lists, c["q"],
                                           c["idx1"], c["qd"], c["sf"], c["sig2"], False, True, want_geom=False)
    new_call()
    by = out["new"]["created_by"]

    def search_calls():
        res = []
        for k, nb in enumerate(c["nb"]):
            free = ~((by[c["idx1"][k]] >= 0) & (by[c["idx1"][k]] < k))       # GetMapPoint(idx1) after the neighbours before k
            res.append(kf.SearchForTriangulation(grid, k, lists[0][k], lists[1][k], c["q"][k][free], c["qd"][k][free], nb["F12"], (nb["ex"], nb["ey"]),
                                                 c["sf"], c["sig2"], False, True))
        out["old"] = res
    a1, b1 = clock(new_call, reps, ctx), clock(search_calls, reps, ctx)
    a2, b2 = clock(new_call, reps, ctx), clock(search_calls, reps, ctx)
    same = sum(int(out["old"][k][0] == out["new"]["nmatches"][k]) for k in range(K))
    with tempfile.TemporaryDirectory() as tmp:
        nc.write_point_case(os.path.join(tmp, "c.bin"), c)
        p = subprocess.run([exe, os.path.join(tmp, "c.bin"), os.path.join(tmp, "o.bin"), "5"], capture_output=True, text=True, check=True)
        host = json.loads(p.stdout)
        with open(os.path.join(tmp, "o.bin"), "rb") as f:
            loop = nc.read_point_section(f, c)
    equal = bool(loop["new"].tobytes() == out["new"]["new"].tobytes() and np.array_equal(loop["status"], out["new"]["status"]))
    a, b = min(a1[0], a2[0]), min(b1[0], b2[0])
    return dict(features=len(cur["keysun"]), neighbours=K, queries=int(sum(len(q) for q in c["q"])), matched=int(out["new"]["nmatches"].sum()),
                created=len(out["new"]["new"]), new_call_ms=dict(median=a, runs=[a1, a2]), search_calls_ms=dict(median=b, runs=[b1, b2]),
                host_loop_ms=host["loop_ms"], old_path_ms_between=[b, b + host["loop_ms"]], neighbours_with_equal_nmatches=same,
                host_loop_equals_device=equal)


def measure_lines(P, ctx, n, K, reps, rng):
    import new_points_cases as nc
    d1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    kl = np.zeros(n, nc.KEYLINE_DTYPE)
    kl["startPointX"], kl["startPointY"] = rng.uniform(50, 590, n), rng.uniform(50, 430, n)
    kl["endPointX"], kl["endPointY"] = kl["startPointX"] + 40, kl["startPointY"] + 10
    z = rng.uniform(2, 6, (n, 2))
    l3d = np.zeros((n, 6))
    for e, (px, py) in enumerate((("startPointX", "startPointY"), ("endPointX", "endPointY"))):
        l3d[:, 3 * e], l3d[:, 3 * e + 1], l3d[:, 3 * e + 2] = (kl[px] - nc.CX) / nc.FX * z[:, e], (kl[py] - nc.CY) / nc.FY * z[:, e], z[:, e]
    nbs = [nc.neighbour(nc.T_x(0.2 + 0.1 * k), k, k + 1) for k in range(K)]
    neigh = []
    for k in range(K):
        perm = rng.permutation(n)
        kl2 = kl[perm].copy()
        kl2["startPointX"] -= nc.FX * (0.2 + 0.1 * k) / z[perm, 0]
        kl2["endPointX"] -= nc.FX * (0.2 + 0.1 * k) / z[perm, 1]
        l2 = l3d[perm].copy()
        l2[:, 0] -= 0.2 + 0.1 * k
        l2[:, 3] -= 0.2 + 0.1 * k
        d2 = d1[perm].copy()
        d2[rng.random(n) < 0.25] = rng.integers(0, 256, 32, dtype=np.uint8)
        neigh.append(dict(ldesc=d2, keylines=kl2, lines3d=l2, has_mapline=(rng.random(n) < 0.2).astype(np.uint8)))
    cur = dict(ldesc=d1, keylines=kl, lines3d=l3d, lineeq=np.where(rng.random(n) < 0.7, 1.0, -1.0).astype(np.float32),
               has_mapline=(rng.random(n) < 0.2).astype(np.uint8))
    kf = P.KeyFrameMatcher(ctx)
    out = {}

    def new_call():
        out["new"] = kf.CreateNewMapLines(nc.keyframe1(), cur["ldesc"], cur["has_mapline"], cur["keylines"], cur["lines3d"], cur["lineeq"], nbs,
                                          [g["ldesc"] for g in neigh], [g["has_mapline"] for g in neigh], [g["keylines"] for g in neigh],
                                          [g["lines3d"] for g in neigh], nc.SF, nc.SIG2, want_geom=False)

    def search_call():
        out["old"] = kf.LineSearchForTriangulationKeyFrames(cur["ldesc"], [g["ldesc"] for g in neigh], cur["has_mapline"], [g["has_mapline"] for g in neigh],
                                                            0.95, 50, True)
    a1, b1 = clock(new_call, reps, ctx), clock(search_call, reps, ctx)
    a2, b2 = clock(new_call, reps, ctx), clock(search_call, reps, ctx)
    a, b = min(a1[0], a2[0]), min(b1[0], b2[0])
    return dict(lines=n, neighbours=K, search_matches=int(out["old"][0].sum()), matched=int(out["new"]["nmatches"].sum()), created=len(out["new"]["new"]),
                new_call_ms=dict(median=a, runs=[a1, a2]), search_call_ms=dict(median=b, runs=[b1, b2]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", type=int, default=2000)
    ap.add_argument("--lines", type=int, default=200)
    ap.add_argument("--neighbours", default="10,20")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import new_points_cases as nc
    import psl_slam_amd as P
    ctx = P.default_context()
    Ks = [3] if a.quick else [int(v) for v in a.neighbours.split(",")]
    n, nl, reps = (200, 50, 3) if a.quick else (a.features, a.lines, a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "newpoints_host")
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-DPSL_TRI_HOST_ONLY", "-o", exe, os.path.join(ROOT, "tools", "dropin", "newpoints_main.cpp")],
                       check=True, capture_output=True)
        points = [measure_points(P, nc, ctx, n, K, reps, exe) for K in Ks]
    rng = np.random.default_rng(5)
    lines = [measure_lines(P, ctx, nl, K, reps, rng) for K in Ks]
    res = dict(bench="new_points", reps=reps, points=points, lines=lines,
               note="ms, host clock around calls that return when the results are back; every `runs` entry is (median, min, max) of `reps` calls after 3 "
                    "warm-up runs, two alternating passes per path, `median` the smaller of the two pass medians.  points.search_calls_ms leaves out the "
                    "host triangulation between the K search calls; host_loop_ms is the one-core loop over the whole stage (its own search included), so "
                    "the old path lies in old_path_ms_between.  One keyframe: the new call wins, where it wins, through the removed round trips.")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
