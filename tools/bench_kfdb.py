"""Measurement of the keyframe database query (pslfe_kfdb_query_device, stage `kfdb.query`): one query and 32 queries per launch
against 1024 and 4096 resident keyframes of about 1000 words each.  The rows and the queries are BowVectors that
pslfe_compute_bow_device writes from synthetic descriptors (uniform random bits: a query shares about a tenth of its words with
every row, so every row is walked and scored) on a 10-ary vocabulary of depth 4 (tests/bow_vocab.py).  Reports, per
configuration, the event-timed kernel time per launch, us per query, and the bytes of the live rows (12 per entry) that the
queries of a launch walk over that time, beside the HBM peak; with 32 queries per launch the rows are read 32 times and mostly
not from HBM, so that figure is a walk rate, not an HBM rate.  Also the host path: pslfe_kfdb_query on host arrays, wall clock.
Prints one JSON line (and writes it with --out).  Also meant to run under `rocprofv3 --kernel-trace --stats`.

Usage: python tools/bench_kfdb.py [--keyframes 1024,4096] [--queries 1,32] [--reps 50] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK = 8.0e12      # bytes/s, MI355X specification
STRIDE, NFEAT = 1280, 1100


def bow_device(P, torch, dev, V, nframes, seed):
    """nframes BowVectors of NFEAT random descriptors each -> (bow_id, bow_val, nbow) tensors at STRIDE"""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    desc = torch.randint(0, 256, (nframes, STRIDE, 32), dtype=torch.uint8, device=dev, generator=g)
    counts = torch.full((nframes,), NFEAT, dtype=torch.int32, device=dev)
    i4 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    f8 = lambda *s: torch.zeros(s, dtype=torch.float64, device=dev)
    fword, fw, fnid, bid, bval, bstart, nbow = i4(nframes, STRIDE), f8(nframes, STRIDE), i4(nframes, STRIDE), i4(nframes, STRIDE), f8(nframes, STRIDE), \
        i4(nframes, STRIDE + 1), i4(nframes)
    fvn, fvs, fvi, nfv = i4(nframes, STRIDE), i4(nframes, STRIDE + 1), i4(nframes, STRIDE), i4(nframes)
    torch.cuda.current_stream().synchronize()
    P._check(P.lib().pslfe_compute_bow_device(V._h, *[C.c_void_p(t.data_ptr()) for t in (desc, counts)], nframes, STRIDE, 4,
                                              *[C.c_void_p(t.data_ptr()) for t in (fword, fw, fnid, bid, bval, bstart, nbow, fvn, fvs, fvi, nfv)]),
             "pslfe_compute_bow_device")
    V.ctx.synchronize()
    return bid, bval, nbow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", default="1024,4096")
    ap.add_argument("--queries", default="1,32")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import psl_slam_amd as P
    import bow_vocab
    dev = torch.device("cuda", 0)
    st = torch.cuda.Stream(dev)
    torch.cuda.set_stream(st)
    ctx = P.Context(0, st.cuda_stream)
    V = P.ORBVocabulary(*bow_vocab.make_vocab(10, 4, seed=3), ctx=ctx)
    nqs = [int(x) for x in a.queries.split(",")]
    qid, qval, qn = bow_device(P, torch, dev, V, max(nqs), 99)
    res = {"tool": "bench_kfdb", "hbm_peak_bytes_per_s": HBM_PEAK, "stride": STRIDE, "features_per_frame": NFEAT, "configs": []}
    for K in [int(x) for x in a.keyframes.split(",")]:
        bid, bval, nbow = bow_device(P, torch, dev, V, K, 7)
        db = P.KeyFrameDatabase(K, STRIDE, ctx=ctx)
        db.add_device(0, bid.data_ptr(), bval.data_ptr(), nbow.data_ptr(), K, STRIDE)
        ctx.synchronize()
        row_bytes = int(nbow.sum().item()) * 12
        for nq in nqs:
            words = torch.zeros((nq, K), dtype=torch.int32, device=dev)
            first = torch.zeros((nq, K), dtype=torch.int32, device=dev)
            score = torch.zeros((nq, K), dtype=torch.float64, device=dev)
            maxc = torch.zeros(nq, dtype=torch.int32, device=dev)
            torch.cuda.current_stream().synchronize()
            run = lambda: db.query_device(qid.data_ptr(), qval.data_ptr(), qn.data_ptr(), nq, STRIDE, None, words.data_ptr(), first.data_ptr(),
                                          score.data_ptr(), maxc.data_ptr())
            for _ in range(a.warmup):
                run()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                run()
            ctx.synchronize()
            wall_us = (time.perf_counter() - t0) / a.reps * 1e6      # back-to-back launches, one synchronise
            ctx.profile(True)
            ctx.profile_only("kfdb.query")
            ctx.profile_reset()
            for _ in range(a.reps):
                run()
            ctx.synchronize()
            ms, n = ctx.stage_time("kfdb.query")
            ctx.profile_only(None)
            ctx.profile(False)
            kernel_us = ms / max(n, 1) * 1e3
            r = dict(keyframes=K, queries=nq, mean_words_per_row=row_bytes / 12 / K, mean_common_words=float(words.float().mean().item()),
                     max_common=int(maxc.max().item()), kernel_us_per_launch=kernel_us, kernel_us_per_query=kernel_us / nq,
                     launch_to_launch_us=wall_us, row_bytes_per_query=row_bytes, rows_walked_bytes_per_s=row_bytes * nq / (kernel_us * 1e-6),
                     share_of_hbm_peak=row_bytes * nq / (kernel_us * 1e-6) / HBM_PEAK)
            if nq == 1:   # the host path: upload of the query, kernel, download of three arrays of K entries
                ids = qid[0, :int(qn[0].item())].cpu().numpy()
                vals = qval[0, :int(qn[0].item())].cpu().numpy()
                ts = []
                for k in range(a.warmup + 20):
                    t0 = time.perf_counter()
                    db.query((ids, vals))
                    ts.append((time.perf_counter() - t0) * 1e6)
                r["host_query_us_median"] = float(np.median(ts[a.warmup:]))
            res["configs"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        db.close()
        del bid, bval, nbow
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
