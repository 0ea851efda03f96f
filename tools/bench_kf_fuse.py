"""Measurement of ORBmatcher::Fuse for a set of keyframes (LocalMapping::SearchInNeighbors, LoopClosing::SearchAndFuse): ONE call of
pslfe_kf_fuse_keyframes - projection of M map points into K keyframes and the candidate loop, on the device - next to what the
library offered before for the same work: the projection on the host (here the numpy restatement of tests/kf_project_cases.py, timed
on its own and named as such: it is test code, not a tuned host loop) and K calls of pslfe_kf_window_best on its rows.  All take host
buffers and return when the results are back, so the times are a host clock around the call(s); the device share of the set call is
its two event-timed stages `kf.project` and `kf.window_best_set`.  Inputs: K keyframes of n random keypoints with random 256-bit
descriptors along a short trajectory, M map points unprojected from random pixels through those poses, every gate of Fuse dropping a
few per cent.  Prints one JSON line (and writes it with --out).  Also meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_kf_fuse.py --quick`.

Usage: python tools/bench_kf_fuse.py [--keyframes 1,8,24,64] [--features 1000,2000] [--points 2000,8000] [--reps 20] [--quick] [--out FILE]
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

BOUNDS = (0.0, 0.0, 640.0, 480.0)
TH = 3.0


def make_inputs(P, kc, n, K, M, rng):
    """-> (keyframes [(kps, desc, uright)], views, map points, their descriptors)"""
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    kfs = []
    for _ in range(K):
        k = np.zeros(n, P.KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.uniform(0, 640, n), rng.uniform(0, 480, n)
        k["octave"] = rng.integers(0, 8, n)
        ur = (k["x"] - 40.0 / rng.uniform(0.6, 6.0, n)).astype(np.float32)
        ur[rng.random(n) < 0.5] = -1.0
        kfs.append((k, rng.integers(0, 256, (n, 32), dtype=np.uint8), ur))
    views = kc.views(nslots=K, n=K)
    src = rng.integers(0, K, M)
    R = np.stack([views[s]["Tcw"]["R"].reshape(3, 3) for s in src]).astype(np.float64)
    t = np.stack([views[s]["Tcw"]["t"] for s in src]).astype(np.float64)
    kp = rng.integers(0, n, M)
    px = np.array([kfs[s][0]["x"][j] for s, j in zip(src, kp)]) + rng.normal(0, 1.0, M)
    py = np.array([kfs[s][0]["y"][j] for s, j in zip(src, kp)]) + rng.normal(0, 1.0, M)
    octave = np.array([kfs[s][0]["octave"][j] for s, j in zip(src, kp)])
    z = rng.uniform(0.6, 6.0, M)
    z[rng.random(M) < 0.05] *= -1.0
    pc = np.stack([(px - 319.5) / 525.0 * z, (py - 239.5) / 525.0 * z, z], 1)
    pw = np.einsum("mji,mj->mi", R, pc - t)
    po = pw + np.einsum("mji,mj->mi", R, t)
    dist = np.linalg.norm(po, axis=1)
    nrm = po / dist[:, None]
    away = rng.random(M) < 0.1
    nrm[away] = rng.normal(0, 1, (away.sum(), 3))
    nrm[away] /= np.linalg.norm(nrm[away], axis=1)[:, None]
    maxd = dist * 1.2 ** (octave - rng.uniform(0.1, 0.9, M))
    far = rng.random(M) < 0.05
    maxd[far] = dist[far] * rng.uniform(0.3, 0.8, far.sum())
    mp = np.zeros(M, P.MAPPOINT_DTYPE)
    mp["x"], mp["y"], mp["z"] = pw.T
    mp["nx"], mp["ny"], mp["nz"] = nrm.T
    mp["max_dist"], mp["min_dist"] = maxd, maxd / 1.2 ** 7
    desc = np.stack([kfs[s][1][j] for s, j in zip(src, kp)])
    flips = rng.integers(0, 256, (M, 10))
    for j in range(10):
        on = rng.random(M) < 0.6
        desc[np.arange(M)[on], flips[on, j] >> 3] ^= (1 << (flips[on, j] & 7)).astype(np.uint8)
    return kfs, views, mp, desc, scale


def measure(P, kc, ctx, n, K, M, reps, rng):
    kfs, views, mp, desc, scale = make_inputs(P, kc, n, K, M, rng)
    inv_sigma2 = (np.float32(1.0) / (scale * scale)).astype(np.float32)
    cam = kc.camera()
    g = P.FrameGrid(max(n, 1), K, ctx=ctx)
    for s, (k, d, ur) in enumerate(kfs):
        g.set(s, k, d, BOUNDS, ur)
    kf = P.KeyFrameMatcher(ctx)
    out = {}

    def set_call():
        out["set"] = kf.FuseKeyFrames(g, kc.FUSE, views, mp, desc, cam, BOUNDS, scale, kc.LOG_SCALE, TH, inv_sigma2)

    t = time.perf_counter()
    rows, _, why = kc.restate_project(kc.FUSE, views, mp, cam, BOUNDS, scale, TH)
    numpy_ms = (time.perf_counter() - t) * 1e3

    def per_keyframe_calls():
        out["single"] = [kf.window_best(g, s, rows[s], desc, True, inv_sigma2) for s in range(K)]

    def clock(run):
        for _ in range(3):
            run()
        ctx.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))

    # the two paths alternate so that a drift of the host hits both
    a1, b1 = clock(set_call), clock(per_keyframe_calls)
    a2, b2 = clock(set_call), clock(per_keyframe_calls)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        set_call()
    ctx.synchronize()
    stage = {s: ctx.stage_time(s)[0] / reps for s in ("kf.project", "kf.window_best_set")}
    ctx.profile(False)
    bi, bd, drows = out["set"]
    same = sum(int((bi[s] == out["single"][s][0]).all() and (bd[s] == out["single"][s][1]).all()) for s in range(K))
    a, b = min(a1[0], a2[0]), min(b1[0], b2[0])
    return dict(features=n, keyframes=K, points=M, rows=int(K * M), rows_kept=int((why == kc.KEPT).sum()), fused=int((bd <= 50).sum()),
                set_call_ms=dict(median=a, runs=[a1, a2]), window_best_calls_ms=dict(median=b, runs=[b1, b2]),
                numpy_projection_ms=numpy_ms, stage_ms=stage, ratio_calls_over_set=b / a,
                rows_equal_restatement=bool(drows.tobytes() == rows.tobytes()), keyframes_with_equal_results=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="1,8,24,64")
    ap.add_argument("--features", default="1000,2000")
    ap.add_argument("--points", default="2000,8000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import kf_project_cases as kc
    import psl_slam_amd as P
    ctx = P.default_context()
    Ks = [8] if a.quick else [int(v) for v in a.keyframes.split(",")]
    feats = [1000] if a.quick else [int(v) for v in a.features.split(",")]
    Ms = [2000] if a.quick else [int(v) for v in a.points.split(",")]
    rng = np.random.default_rng(5)
    rows = [measure(P, kc, ctx, n, K, M, 5 if a.quick else a.reps, rng) for n in feats for M in Ms for K in Ks]
    res = dict(bench="kf_fuse", mode="PSLFE_KF_PROJ_FUSE", th=TH, reps=a.reps, rows=rows,
               note="ms per Fuse of M map points into K keyframes, host clock, host buffers in and out.  set_call_ms: one "
                    "pslfe_kf_fuse_keyframes (projection on the device).  window_best_calls_ms: K calls of pslfe_kf_window_best on rows "
                    "projected beforehand; numpy_projection_ms: that projection by the numpy restatement of the tests, once, a test "
                    "helper and not a tuned host loop, so it is reported and not added.  ratio_calls_over_set leaves the host projection "
                    "out of the K-calls side.")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
