"""Driver for a kernel-trace measurement of the projection kernels (pslfe_orb_project_last_device with and without the
visual-odometry selection, pslfe_orb_project_frustum_device) beside the bench's stand-in query builder (k_queries_from_prev,
tools/bench_kernels) on the same frames: F 'sticks' frames (24 distinct ones, repeated) at 640x480, extracted and set as RGB-D
slots on the device.  Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/bench_project.py`; it also prints
event-timed milliseconds per launch as one JSON line.

Usage: python tools/bench_project.py [--frames 12288] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12288)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import psl_slam_amd as P
    import batch_pipeline as BP
    import synth_frames as sf
    F, W, H = a.frames, 640, 480
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    sc = sf.Scene(W, H, "sticks", 33)
    uniq = 24
    g8 = torch.from_numpy(np.stack([sc.gray(t) for t in range(uniq)])).to(dev)
    dz = torch.from_numpy(np.stack([sc.depth_u16(t).astype(np.float32) / np.float32(5000.0) for t in range(uniq)])).to(dev)
    reps = (F + uniq - 1) // uniq
    gray = g8.repeat(reps, 1, 1)[:F].contiguous()
    depth = dz.repeat(reps, 1, 1)[:F].contiguous()
    del g8, dz
    ctx = P.Context(0, st.cuda_stream)
    orb = P.ORBextractor(BP.NFEATURES, BP.SCALE, BP.NLEVELS, BP.INI_TH, BP.MIN_TH, ctx=ctx, max_batch=F)
    cap = orb.max_keypoints(W, H)
    grid = P.FrameGrid(cap, F, ctx=ctx)
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, BP.TUM1):
        cam[k] = np.float32(v)
    orb.extract_batch_device(gray.data_ptr(), F, W, H, W, W * H)
    grid.set_from_orb_rgbd(orb, depth.data_ptr(), W, H, cam)
    del gray, depth
    bounds = tuple(float(b) for b in grid.image_bounds(cam, W, H))
    scale = np.asarray(BP.scale_factors(), np.float32)
    lsf = float(np.log(np.float32(BP.SCALE)))
    npairs = F - 1
    rng = np.random.default_rng(0)
    Tl = np.zeros(npairs, P.POSE_DTYPE)
    Tl["R"] = np.eye(3, dtype=np.float32).reshape(9)
    Tc = Tl.copy()
    Tc["t"] = rng.normal(0, 0.02, (npairs, 3)).astype(np.float32)
    d_Tl = torch.from_numpy(Tl.view(np.uint8)).to(dev)
    d_Tc = torch.from_numpy(Tc.view(np.uint8)).to(dev)
    # caller points: a map point (Observations() > 0) 2 m in front of every keypoint's pixel ray
    pts = torch.zeros((npairs, cap, 4), dtype=torch.float32, device=dev)
    pts[:, :, 0].uniform_(-1.0, 1.0)
    pts[:, :, 1].uniform_(-0.8, 0.8)
    pts[:, :, 2] = 2.0
    pts.view(torch.int32)[:, :, 3] = 2
    # local map points: as many per frame as the frame has keypoints
    mp = torch.zeros((npairs, cap, 8), dtype=torch.float32, device=dev)
    mp[:, :, 0].uniform_(-1.5, 1.5)
    mp[:, :, 1].uniform_(-1.2, 1.2)
    mp[:, :, 2].uniform_(0.5, 4.0)
    mp[:, :, 5] = 1.0
    mp[:, :, 6], mp[:, :, 7] = 0.3, 5.0
    mpdesc = torch.randint(0, 256, (npairs, cap, 32), dtype=torch.uint8, device=dev)
    nmp = torch.full((npairs,), cap, dtype=torch.int32, device=dev)
    q = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    qd = torch.zeros((F, cap, 32), dtype=torch.uint8, device=dev)
    ow = torch.zeros((F, cap), dtype=torch.int32, device=dev)
    nq = torch.zeros((F,), dtype=torch.int32, device=dev)
    BK = BP.bench_kernels()
    k, d, c, _ = orb.results_device()
    scale_t = torch.tensor(scale, device=dev)

    def stand_in():
        assert BK.bench_queries_from_prev(st.cuda_stream, k, d, c, F, cap, BP.NLEVELS, scale_t.data_ptr(), 15.0, q.data_ptr(), qd.data_ptr(),
                                          nq.data_ptr()) == 0

    def last(vo):
        grid.project_last_device(0, npairs, d_Tl.data_ptr(), d_Tc.data_ptr(), 0 if vo else pts.data_ptr(), 0, cam, scale, 15.0, 3.0, False,
                                 vo, bounds, q.data_ptr(), qd.data_ptr(), ow.data_ptr(), nq.data_ptr(), cap)

    def frustum():
        P.project_frustum_device(npairs, d_Tc.data_ptr(), mp.data_ptr(), mpdesc.data_ptr(), nmp.data_ptr(), cap, cam, scale, lsf, 0.5, 1.0,
                                 bounds, q.data_ptr(), qd.data_ptr(), ow.data_ptr(), nq.data_ptr(), cap, ctx=ctx)

    res = {"frames": F, "cap": cap}
    for name, fn in (("k_queries_from_prev", stand_in), ("project_last", lambda: last(False)), ("project_last_vo", lambda: last(True)),
                     ("project_frustum", frustum)):
        fn()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(a.reps):
            fn()
        e1.record(st)
        torch.cuda.synchronize(dev)
        res[name + "_ms"] = round(e0.elapsed_time(e1) / a.reps, 4)
        res[name + "_rows"] = int(nq[:npairs].sum().item())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
