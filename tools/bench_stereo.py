"""Measurement of the stereo constructor (pslfe_frame_set_from_orb_stereo) beside the extraction it follows, at the TUM-like
640x480, EuRoC 752x480 and KITTI 1241x376 geometries (tests/stereo_scene.py): for N pairs extracted as ONE batch of 2N frames
(lefts, then rights) it reports the event-timed `orb.*` stages and `frame.stereo` per launch, pairs/s, the one-pair latency
through the host path (two extractors + the stereo call + fetch, and the part the stereo call adds), and the restatement
oracle/stereo_oracle.cpp timed on one host core.  Prints one JSON line (and writes it with --out).  Also meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_stereo.py --quick`.

Usage: python tools/bench_stereo.py [--pairs 1,32,12288] [--kitti-max 6144] [--reps 3] [--quick] [--out FILE]
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

ORB_STAGES = ("orb.pyramid", "orb.fast", "orb.octree", "orb.blur", "orb.describe")


def camera(P, vals):
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, vals):
        cam[k] = np.float32(v)
    return cam


def batch(P, torch, dev, ctx, G, cam, N, reps, uniq_pairs):
    w, h, nf = G["w"], G["h"], G["nfeatures"]
    uniq = len(uniq_pairs)
    Ls = torch.from_numpy(np.stack([uniq_pairs[k % uniq][0] for k in range(min(N, uniq))])).to(dev)
    Rs = torch.from_numpy(np.stack([uniq_pairs[k % uniq][1] for k in range(min(N, uniq))])).to(dev)
    r = (N + uniq - 1) // uniq
    imgs = torch.cat([Ls.repeat(r, 1, 1)[:N], Rs.repeat(r, 1, 1)[:N]], 0).contiguous()
    del Ls, Rs
    orb = P.ORBextractor(nf, 1.2, 8, 20, 7, ctx=ctx, max_batch=2 * N)
    cap = orb.max_keypoints(w, h)
    g = P.FrameGrid(cap, N, ctx=ctx)
    run = lambda: (orb.extract_batch_device(imgs.data_ptr(), 2 * N, w, h, w, w * h), g.set_from_orb_stereo(0, orb, 0, orb, N, N, cam))
    run()
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) / reps * 1e3
    st = {}
    for s in ORB_STAGES + ("frame.stereo", "match.grid"):
        ms, n = ctx.stage_time(s)
        st[s] = ms / max(reps, 1)
    ctx.profile(False)
    orb_ms = sum(st[s] for s in ORB_STAGES)
    # per-pair outputs: accepted keypoints of the first pair
    _, dep, _ = g.fetch(0)
    out = dict(pairs=N, stages_ms=st, orb_ms=orb_ms, stereo_ms=st["frame.stereo"], stereo_over_orb=st["frame.stereo"] / orb_ms if orb_ms else None,
               wall_ms_profiled=wall, pairs_per_s=N / (orb_ms + st["frame.stereo"] + st["match.grid"]) * 1e3,
               depth_pair0=int((dep > 0).sum()), keypoints_pair0=len(dep))
    del g, orb, imgs
    torch.cuda.empty_cache()
    return out


def one_pair(P, ctx, G, cam, pair, reps):
    w, h, nf = G["w"], G["h"], G["nfeatures"]
    oL, oR = P.ORBextractor(nf, 1.2, 8, 20, 7, ctx=ctx), P.ORBextractor(nf, 1.2, 8, 20, 7, ctx=ctx)
    g = P.FrameGrid(oL.max_keypoints(w, h), 1, ctx=ctx)
    left, right = pair
    ext, full = [], []
    for k in range(reps + 2):
        t0 = time.perf_counter()
        oL(left)
        oR(right)
        t1 = time.perf_counter()
        g.set_from_orb_stereo(0, oL, 0, oR, 0, 1, cam)
        g.fetch(0)
        t2 = time.perf_counter()
        if k >= 2:
            ext.append((t1 - t0) * 1e3)
            full.append((t2 - t0) * 1e3)
    return dict(extract_two_ms=float(np.median(ext)), with_stereo_ms=float(np.median(full)),
                stereo_added_ms=float(np.median(np.array(full) - np.array(ext))))


def restatement_ms(P, ctx, G, cam, pair, reps):
    import oracle_lib
    w, h, nf = G["w"], G["h"], G["nfeatures"]
    oL, oR = P.ORBextractor(nf, 1.2, 8, 20, 7, ctx=ctx), P.ORBextractor(nf, 1.2, 8, 20, 7, ctx=ctx)
    kL, dL = oL(pair[0])
    kR, dR = oR(pair[1])
    levL = [oL.debug_level_image(0, l) for l in range(8)]
    levR = [oR.debug_level_image(0, l) for l in range(8)]
    sc, inv = oL.GetScaleFactors().astype(np.float32), oL.GetInverseScaleFactors().astype(np.float32)
    oracle_lib.load()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        oracle_lib.restate_stereo(kL, dL, kR, dR, levL, levR, sc, inv, float(cam["bf"]), float(cam["fx"]))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,32,12288")
    ap.add_argument("--kitti-max", type=int, default=6144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="one geometry (640x480), 1 and 32 pairs: for a kernel trace")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psl_slam_amd as P
    import stereo_scene as ss
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    ctx = P.Context(0, st.cuda_stream)
    res = {"tool": "bench_stereo", "geometries": {}}
    geoms = ["tum"] if a.quick else list(ss.GEOMETRIES)
    for name in geoms:
        G = ss.GEOMETRIES[name]
        cam = camera(P, G["cam"])
        pairs = [ss.scene_pair(G["w"], G["h"], float(cam["bf"]), G["zscale"], style=("desk", "sticks")[k % 2], seed=200 + k, t=k % 3)[:2]
                 for k in range(8)]
        Ns = [1, 32] if a.quick else [int(x) for x in a.pairs.split(",")]
        r = {"w": G["w"], "h": G["h"], "nfeatures": G["nfeatures"], "batches": []}
        for N in Ns:
            if name == "kitti":
                N = min(N, a.kitti_max)
            try:
                r["batches"].append(batch(P, torch, dev, ctx, G, cam, N, a.reps, pairs))
            except (P.PslfeError, RuntimeError) as e:   # out of device memory at the largest batches: recorded, not fatal
                r["batches"].append({"pairs": N, "error": str(e)[:300]})
                torch.cuda.empty_cache()
            print(json.dumps({name: r["batches"][-1]}), file=sys.stderr, flush=True)
        r["one_pair"] = one_pair(P, ctx, G, cam, pairs[0], 20)
        r["restatement_one_core_ms"] = restatement_ms(P, ctx, G, cam, pairs[0], 5)
        res["geometries"][name] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
