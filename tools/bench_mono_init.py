"""Measurement of the monocular initialiser's matcher (pslfe_orb_search_for_initialization_device) beside the ORB extraction of
the second frames it matches, at TUM1 640x480 with the initialiser's 2000 features and KITTI 1241x376 with 4000: for N pairs per
launch it reports the event-timed `match.mono_init` stage next to the `orb.*` stages (and `frame.mono`, `match.grid`) of the N
F2 frames extracted as one batch, the one-pair latency through the host path, and the restatement oracle/mono_init_oracle.cpp
timed on one host core.  The device extractor refuses 4000 features (a level quota above its 512-node octree), so at KITTI the
frames come from the CPU oracle of the extractor (8 distinct F2 frames, pair p matching frame 1 + p % 8) and the ORB column is
the 2000-feature extraction of the same N frames, for scale.  Prints one JSON line (and writes it with --out).  Also meant to run
under `rocprofv3 --kernel-trace --stats -- python tools/bench_mono_init.py --quick`.

Usage: python tools/bench_mono_init.py [--pairs 1,32,4096,12288] [--reps 3] [--quick] [--out FILE]
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
TUM1 = (517.306408, 516.469215, 318.643040, 255.313989, 0.262383, -0.953104, -0.005358, 0.002628, 1.163314, 40.0)
KITTI = (718.856, 718.856, 607.1928, 185.2157, 0, 0, 0, 0, 0, 386.1448)
GEOMETRIES = {"tum": dict(w=640, h=480, cam=TUM1, nfeatures=2000), "kitti": dict(w=1241, h=376, cam=KITTI, nfeatures=4000)}


def camera(P, vals):
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, vals):
        cam[k] = np.float32(v)
    return cam


def timed(ctx, reps, run, stages):
    run()
    ctx.synchronize()
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(reps):
        run()
    ctx.synchronize()
    st = {s: ctx.stage_time(s)[0] / max(reps, 1) for s in stages}
    ctx.profile(False)
    return st


def batch(P, torch, dev, ctx, G, cam, N, reps, frames, oracle_frames):
    w, h = G["w"], G["h"]
    uniq = len(frames)
    imgs = torch.from_numpy(np.stack([frames[1 + k % (uniq - 1)] for k in range(min(N, uniq - 1))])).to(dev)
    r = (N + imgs.shape[0] - 1) // imgs.shape[0]
    imgs = imgs.repeat(r, 1, 1)[:N].contiguous()
    nf_dev = min(G["nfeatures"], 2000)
    orb = P.ORBextractor(nf_dev, 1.2, 8, 20, 7, ctx=ctx, max_batch=N)
    cap = orb.max_keypoints(w, h)
    g2 = P.FrameGrid(cap, N, ctx=ctx)
    st_orb = timed(ctx, reps, lambda: (orb.extract_batch_device(imgs.data_ptr(), N, w, h, w, w * h), g2.set_from_orb_mono(0, orb, 0, N, cam)),
                   ORB_STAGES + ("frame.mono", "match.grid"))
    orb_ms = sum(st_orb[s] for s in ORB_STAGES)
    if oracle_frames is None:   # F1 = frame 0 through the same extractor, F2 = the N slots just built
        o1 = P.ORBextractor(nf_dev, 1.2, 8, 20, 7, ctx=ctx)
        o1(frames[0])
        g1 = P.FrameGrid(cap, 1, ctx=ctx)
        g1.set_from_orb_mono(0, o1, 0, 1, cam)
        f2, s2 = g2, np.arange(N, dtype=np.int32)
        k1 = g1.fetch(0)[0]
    else:                       # oracle keypoints: F1 = slot 0, F2 = slots 1..8
        g1 = P.FrameGrid(4096, len(oracle_frames), ctx=ctx)
        bounds = (0.0, 0.0, float(w), float(h))
        for s, (k, d) in enumerate(oracle_frames):
            g1.set(s, k, d, bounds)
        f2, s2 = g1, np.array([1 + p % (len(oracle_frames) - 1) for p in range(N)], np.int32)
        k1 = oracle_frames[0][0]
    stride = g1.cap
    base = torch.zeros((N, stride, 2), dtype=torch.float32, device=dev)
    base[:, :len(k1)] = torch.from_numpy(np.stack([k1["x"], k1["y"]], 1).astype(np.float32)).to(dev)
    d_prev = base.clone()
    m12 = torch.empty((N, stride), dtype=torch.int32, device=dev)
    nm = torch.empty(N, dtype=torch.int32, device=dev)
    s1 = np.zeros(N, np.int32)

    def run():
        d_prev.copy_(base)
        P.search_for_initialization_device(g1, s1, f2, s2, d_prev.data_ptr(), stride, m12.data_ptr(), nm.data_ptr())
    st = timed(ctx, reps, run, ("match.mono_init",))
    mono = st["match.mono_init"]
    NM = nm.cpu().numpy()
    out = dict(pairs=N, orb_features=nf_dev, stages_ms={**st_orb, **st}, orb_ms=orb_ms, match_ms=mono,
               match_over_orb=mono / orb_ms if orb_ms else None, matches_pair0=int(NM[0]), matches_mean=float(NM.mean()))
    del g2, orb, imgs, base, d_prev, m12
    torch.cuda.empty_cache()
    return out


def one_pair(P, ctx, G, cam, frames, oracle_frames, reps):
    """The host path of one pair: SearchForInitialization with prev and matches in host memory (the frames are on the device)."""
    w, h = G["w"], G["h"]
    if oracle_frames is None:
        orb = P.ORBextractor(G["nfeatures"], 1.2, 8, 20, 7, ctx=ctx)
        g = P.FrameGrid(orb.max_keypoints(w, h), 2, ctx=ctx)
        for s in (0, 1):
            orb(frames[s])
            g.set_from_orb_mono(s, orb, 0, 1, cam)
    else:
        g = P.FrameGrid(4096, 2, ctx=ctx)
        for s in (0, 1):
            g.set(s, *oracle_frames[s], (0.0, 0.0, float(w), float(h)))
    k1 = g.fetch(0)[0]
    p0 = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1).astype(np.float32))
    m = P.ORBmatcher(0.9, True)
    ts = []
    for k in range(reps + 2):
        pv = p0.copy()
        t0 = time.perf_counter()
        nm, _ = m.SearchForInitialization(g, 0, g, 1, pv, 100)
        if k >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    return dict(search_ms=float(np.median(ts)), matches=nm, keypoints=len(k1))


def restatement_ms(P, ctx, G, cam, frames, oracle_frames, reps):
    import oracle_lib
    w, h = G["w"], G["h"]
    if oracle_frames is None:
        orb = P.ORBextractor(G["nfeatures"], 1.2, 8, 20, 7, ctx=ctx)
        g = P.FrameGrid(orb.max_keypoints(w, h), 2, ctx=ctx)
        kd = []
        for s in (0, 1):
            _, d = orb(frames[s])
            g.set_from_orb_mono(s, orb, 0, 1, cam)
            kd.append((g.fetch(s)[0], d))
        bounds = oracle_lib.image_bounds(cam, w, h)
    else:
        kd, bounds = oracle_frames[:2], (0.0, 0.0, float(w), float(h))
    prev = np.stack([kd[0][0]["x"], kd[0][0]["y"]], 1).astype(np.float32)
    oracle_lib.load()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        oracle_lib.restate_search(kd[0][0], kd[0][1], kd[1][0], kd[1][1], bounds, prev, 100, 0.9, True)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,32,4096,12288")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="640x480 only, 1 and 32 pairs: for a kernel trace")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psl_slam_amd as P
    import synth_frames as sf
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    ctx = P.Context(0, st.cuda_stream)
    res = {"tool": "bench_mono_init", "geometries": {}}
    for name in (["tum"] if a.quick else list(GEOMETRIES)):
        G = GEOMETRIES[name]
        cam = camera(P, G["cam"])
        sc = sf.Scene(G["w"], G["h"], "desk", 31)
        frames = [sc.gray(t) for t in range(9)]
        oracle_frames = None
        if G["nfeatures"] > 2000:
            import oracle_lib
            orc = oracle_lib.OracleORB(G["nfeatures"], 1.2, 8, 20, 7)
            oracle_frames = [orc(f) for f in frames]
        r = {"w": G["w"], "h": G["h"], "nfeatures": G["nfeatures"], "batches": []}
        for N in ([1, 32] if a.quick else [int(x) for x in a.pairs.split(",")]):
            try:
                r["batches"].append(batch(P, torch, dev, ctx, G, cam, N, a.reps, frames, oracle_frames))
            except (P.PslfeError, RuntimeError) as e:   # out of device memory at the largest batches: recorded, not fatal
                r["batches"].append({"pairs": N, "error": str(e)[:300]})
                torch.cuda.empty_cache()
            print(json.dumps({name: r["batches"][-1]}), file=sys.stderr, flush=True)
        r["one_pair"] = one_pair(P, ctx, G, cam, frames, oracle_frames, 20)
        r["restatement_one_core_ms"] = restatement_ms(P, ctx, G, cam, frames, oracle_frames, 5)
        res["geometries"][name] = r
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
