"""Driver for a kernel-trace measurement of the map-line projection and line window search kernels
(pslfe_line_project_last_device, pslfe_line_project_frustum_device, pslfe_line_search_by_projection_device in modes 0 and 1) on
F - 1 pairs of 'sticks' frames at 640x480: 24 distinct frames go through the batched line extractor, the pairing and the glue,
and their device views are tiled to F frames.  Pair p projects frame p's lines (world = its camera moved a little) into frame
p + 1.  Meant to run under `rocprofv3 --kernel-trace --stats -- python tools/bench_line_project.py`; it also prints event-timed
milliseconds per launch as one JSON line.

Usage: python tools/bench_line_project.py [--frames 12289] [--reps 5]
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
    ap.add_argument("--frames", type=int, default=12289)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    import psl_slam_amd as P
    import batch_pipeline as BP
    import synth_frames as sf
    F, W, H, U = a.frames, 640, 480, 24
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    ctx = P.Context(0, st.cuda_stream)
    sc = sf.Scene(W, H, "sticks", 33)
    gray = torch.from_numpy(np.stack([sc.gray(t) for t in range(U)])).to(dev)
    depth = torch.from_numpy(np.stack([sc.depth_u16(t).astype(np.float32) / np.float32(5000.0) for t in range(U)])).to(dev)
    cam = np.zeros((), P.CAMERA_DTYPE)
    for k, v in zip(P.CAMERA_DTYPE.names, BP.TUM1):
        cam[k] = np.float32(v)
    cam["k1"] = cam["k2"] = cam["p1"] = cam["p2"] = cam["k3"] = 0
    le = P.LINEextractor(1, 1.2, 200, 0.0, ctx=ctx, max_batch=U)
    le.extract_batch_device(gray.data_ptr(), U, W, H, W, W * H)
    le.pair_batch_device(20.0, float(np.float32(np.pi / 4)))
    d_kls, d_desc, d_eq, d_nkl, K = le.results_device()
    d_fans, d_nfans = le.fans_device()
    glue = P.FrameGlue(max_lines=K, max_fans=4096, max_batch=U, ctx=ctx)
    glue.run_batch_device(U, d_kls, K, d_nkl, d_fans, 4096, d_nfans, depth.data_ptr(), W, H, cam, 1)
    d_l3, _ = glue.lines3d_device()
    ctx.synchronize()
    view = lambda ptr, shape, ts: torch.as_tensor(P._DevArray(ptr, shape, ts), device=dev)
    idx = torch.arange(F, device=dev) % U
    kls = view(d_kls, (U, K * P.KEYLINE_DTYPE.itemsize), "|u1")[idx].contiguous()
    desc = view(d_desc, (U, K, 32), "|u1")[idx].contiguous()
    eq = view(d_eq, (U, K, 3), "<f8")[idx].contiguous()
    nkl = view(d_nkl, (U,), "<i4")[idx].contiguous()
    l3 = view(d_l3, (U, K, 6), "<f8")[idx].contiguous()
    npairs = F - 1
    # map-line records of frame p in its own camera (world = camera p), current pose: a small motion
    mid = 0.5 * (l3[:npairs, :, :3] + l3[:npairs, :, 3:])
    nm = mid.norm(dim=2, keepdim=True)
    rec = torch.zeros((npairs, K, 11), dtype=torch.float64, device=dev)
    rec[:, :, 0:6] = l3[:npairs]
    rec[:, :, 6:9] = mid / nm.clamp_min(1e-300)
    recb = rec.view(torch.uint8).view(npairs, K, 88)
    mx = (nm[:, :, 0] * 1.2).float()
    recb[:, :, 72:80] = torch.stack([mx / np.float32(1.2 ** 7), mx], 2).contiguous().view(torch.uint8).view(npairs, K, 8)
    recb[:, :, 80:84] = torch.where(nm[:, :, 0] > 0, 2, 0).int().contiguous().view(torch.uint8).view(npairs, K, 4)
    recb[:, :, 84:88] = 0
    d_last = recb.contiguous()
    d_geom = recb[:, :, :80].contiguous()
    Tc = np.zeros(npairs, P.POSE_DTYPE)
    Tc["R"] = np.eye(3, dtype=np.float32).reshape(9)
    Tc["t"] = np.float32([0.005, -0.003, 0.01])
    d_Tc = torch.from_numpy(Tc.view(np.uint8)).to(dev)
    bounds = (0.0, 0.0, float(W), float(H))
    lsf = float(np.log(np.float32(1.2)))
    q0 = torch.zeros((npairs, K, 64), dtype=torch.uint8, device=dev)
    qd0, nq0 = torch.zeros((npairs, K, 32), dtype=torch.uint8, device=dev), torch.zeros(npairs, dtype=torch.int32, device=dev)
    q1, qd1, nq1 = torch.zeros_like(q0), torch.zeros_like(qd0), torch.zeros_like(nq0)
    m0 = torch.full((npairs, K), -1, dtype=torch.int32, device=dev)
    m1, nm0, nm1 = torch.full_like(m0, -1), torch.zeros_like(nq0), torch.zeros_like(nq0)
    nfb = torch.zeros(2, dtype=torch.int32, device=dev)
    ksz = P.KEYLINE_DTYPE.itemsize
    cur = dict(kls=kls.data_ptr() + K * ksz, desc=desc.data_ptr() + K * 32, eq=eq.data_ptr() + K * 24, nkl=nkl.data_ptr() + 4,
               l3=l3.data_ptr() + K * 48)

    def run():
        P.line_project_last_device(npairs, kls.data_ptr(), desc.data_ptr(), nkl.data_ptr(), K, d_last.data_ptr(), 0, d_Tc.data_ptr(), cam,
                                   20.0, bounds, q0.data_ptr(), qd0.data_ptr(), 0, nq0.data_ptr(), K, ctx=ctx)
        P.line_project_frustum_device(npairs, d_Tc.data_ptr(), d_geom.data_ptr(), desc.data_ptr(), nkl.data_ptr(), K, cam, lsf, 0.5, 1.0,
                                      bounds, q1.data_ptr(), qd1.data_ptr(), 0, nq1.data_ptr(), K, ctx=ctx)
        P.line_search_by_projection_device(npairs, cur["kls"], cur["desc"], cur["eq"], cur["nkl"], K, 0, K, bounds, q0.data_ptr(),
                                           qd0.data_ptr(), nq0.data_ptr(), K, 0, 0, 0.95, m0.data_ptr(), 0, nm0.data_ptr(), nfb.data_ptr(),
                                           ctx=ctx)
        P.line_search_by_projection_device(npairs, cur["kls"], cur["desc"], cur["eq"], cur["nkl"], K, cur["l3"], K, bounds, q1.data_ptr(),
                                           qd1.data_ptr(), nq1.data_ptr(), K, 0, 1, 0.95, m1.data_ptr(), 0, nm1.data_ptr(),
                                           nfb.data_ptr() + 4, ctx=ctx)

    run()
    torch.cuda.synchronize(dev)
    ctx.profile(True)
    ctx.profile_reset()
    for _ in range(a.reps):
        run()
    ctx.synchronize()
    out = {"pairs": npairs, "kl_stride": K, "reps": a.reps,
           "lines_per_frame": float(nkl.float().mean().item()), "rows_last": float(nq0.float().mean().item()),
           "rows_frustum": float(nq1.float().mean().item()), "matches_mode0": float(nm0.float().mean().item()),
           "matches_mode1": float(nm1.float().mean().item()), "fallback_pairs": nfb.cpu().tolist()}
    for s in ("line.project_last", "line.project_frustum", "line.proj_match_batch"):
        ms, n = ctx.stage_time(s)
        out[s + "_ms_per_launch"] = ms / max(n, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
