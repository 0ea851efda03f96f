"""What k_lbd pays for the orientation of its lines: the same bars drawn near-horizontal and near-vertical, through the batched line
extractor, line.lbd per million samples of each set.  (The kernel gathers with lane = row of the 63-row support region: along a
horizontal line the 63 lanes of a load sit in 63 image rows, along a vertical one in one.)

Usage: python tools/lbd_layout_ab.py [frames per launch, default 2048] [launches, default 5]

The bars are drawn once in a square of H x H pixels, within +-10 degrees of horizontal; the near-vertical set is the same square
transposed, so both sets carry the same bars.  The sum of numOfPixels over the keylines of both sets is printed and must agree
within 5 %.  A sample is one pixel of one support-region row: 63 per line pixel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import psl_slam_amd as P  # noqa: E402

W, H, NDISTINCT = 640, 480, 8


def bars_square(seed, side=H, spread_deg=10.0):
    """side x side float image of non-overlapping thin bars (58 - 80 px long, 4 - 6 px wide, 2 px clearance) within spread_deg of
    horizontal, as the 'sticks' scene of tools/synth_frames.py draws them, on a flat background."""
    rng = np.random.default_rng(seed)
    img = np.full((side, side), float(rng.uniform(90, 160)), np.float32)
    occ = np.zeros((side, side), bool)
    want, done, tries = int(400 * side * side / (640.0 * 480.0)), 0, 0
    while tries < want * 20 and done < want:
        tries += 1
        cx, cy = rng.uniform(0, side, 2)
        L, Wd = rng.uniform(58, 80) / 2, rng.uniform(4, 6) / 2
        th = np.deg2rad(rng.uniform(-spread_deg, spread_deg))
        c, s = np.cos(th), np.sin(th)
        r = int(np.ceil(L + Wd + 4))
        x0, y0, x1, y1 = max(int(cx) - r, 0), max(int(cy) - r, 0), min(int(cx) + r + 1, side), min(int(cy) + r + 1, side)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
        if (occ[y0:y1, x0:x1] & (np.abs(u) < L + 2) & (np.abs(v) < Wd + 2)).any():
            continue
        inside = (np.abs(u) < L) & (np.abs(v) < Wd)
        occ[y0:y1, x0:x1] |= inside
        img[y0:y1, x0:x1][inside] = rng.uniform(20, 70) if rng.random() < 0.5 else rng.uniform(190, 240)
        done += 1
    return img


def frame(square, seed):
    """The square in the middle of a W x H frame: a 0.6 px point spread and noise of sigma 1, as 'sticks' has them."""
    from scipy.ndimage import gaussian_filter
    img = np.full((H, W), square[0, 0], np.float32)
    x0 = (W - square.shape[1]) // 2
    img[:, x0:x0 + square.shape[1]] = square
    img = gaussian_filter(img, 0.6) + np.random.default_rng(seed).standard_normal((H, W)).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def frame_sets():
    """{"horizontal": [NDISTINCT][H][W] u8, "vertical": the same bars transposed}; both sets get the same noise field per frame."""
    squares = [bars_square(1000 + i) for i in range(NDISTINCT)]
    return {"horizontal": np.stack([frame(s, 7000 + i) for i, s in enumerate(squares)], 0),
            "vertical": np.stack([frame(np.ascontiguousarray(s.T), 7000 + i) for i, s in enumerate(squares)], 0)}


def measure(base, B, launches):
    frames = np.ascontiguousarray(np.concatenate([base] * ((B + len(base) - 1) // len(base)), 0)[:B])
    ctx = P.default_context()
    le = P.LINEextractor(1, 1.2, 200, 0.0, ctx=ctx, max_batch=B)
    d_ptr, _ = ctx.device_array(frames)
    le.extract_batch_device(d_ptr, B, W, H, W, W * H)   # warm-up
    ctx.synchronize()
    kls = [le.fetch(f)[0] for f in range(len(base))]
    per = np.array([int(k["numOfPixels"].sum()) for k in kls], np.int64)
    pixels = int(sum(per[f % len(base)] for f in range(B)))
    near_h = sum(int((np.abs(np.cos(k["angle"])) >= np.abs(np.sin(k["angle"]))).sum()) for k in kls)
    ctx.profile_reset()
    ctx.profile(True)
    for _ in range(launches):
        le.extract_batch_device(d_ptr, B, W, H, W, W * H)
    ctx.synchronize()
    ctx.profile(False)
    ms, _ = ctx.stage_time("line.lbd")
    le.close()
    ctx.device_free(d_ptr)
    return {"keylines": sum(len(k) for k in kls), "near_horizontal_keylines": near_h, "pixels": pixels, "lbd_ms": ms / launches}


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    res = {name: measure(base, B, launches) for name, base in frame_sets().items()}
    for name, r in res.items():
        msamples = r["pixels"] * 63 / 1e6
        print(f"{name:10s} {B} frames per launch: {r['keylines']} keylines on the {NDISTINCT} distinct frames ({r['near_horizontal_keylines']} with |cos| >= |sin|), "
              f"sum numOfPixels {r['pixels']}, line.lbd {r['lbd_ms']:.3f} ms per launch = {r['lbd_ms'] * 1e3 / msamples:.4f} us per million samples")
    a, b = res["horizontal"], res["vertical"]
    diff = abs(a["pixels"] - b["pixels"]) / max(a["pixels"], b["pixels"])
    print(f"sum numOfPixels differs by {100 * diff:.2f} % (must be within 5 %)")
    assert diff <= 0.05, "the two sets do not carry the same line load"
    print(f"near-horizontal / near-vertical per sample: {(a['lbd_ms'] / a['pixels']) / (b['lbd_ms'] / b['pixels']):.3f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
