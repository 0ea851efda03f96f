"""Where rect_improve decides its rectangles (analysis only; the oracle is read through its existing taps, not changed).

rect_improve() of LSD_REFINE_ADV is restated here in Python on top of the oracle's taps - the rectangles handed to rect_improve
(`pso_lsd_rects`), the level-line angles (`pso_lsd_gradient`) and nfa() (`pso_lsd_nfa`) - so that the phase in which every rectangle
is accepted or rejected can be counted: the number of rectangles the launches of each phase of line_kernels3.h still have to
look at.  The restatement is checked against the oracle: the rectangles it accepts are as many as the segments `pso_lsd_detect`
returns for the frame.

usage: python tools/nfa_phase_stats.py [sticks struct ...]   (the frames of bench.py: scenes seed + 17 s, time steps 0 and 16)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tests"))
sys.path.insert(0, os.path.dirname(__file__))

PI = 3.1415926535897932384626433832795
NOTDEF = -1024.0
STAGES = ("first", "-1", "0", "1", "2", "3")   # the test / phase after which a rectangle leaves; index 6 = rejected after phase 3


def _tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def rect_counts(ang, r, prec):
    """(total_pts, alg_pts) of rect_nfa() as OpenCV 3.x behaves (oracle/line_oracle.cpp: rect_counts)."""
    H, W = ang.shape
    x1, y1, x2, y2, width, theta, dx, dy = r
    hw = width / 2.0
    dyhw, dxhw = dy * hw, dx * hw
    e = sorted([(int(x1 - dyhw), int(y1 + dxhw)), (int(x2 - dyhw), int(y2 + dxhw)), (int(x2 + dyhw), int(y2 - dxhw)), (int(x1 + dyhw), int(y1 - dxhw))])
    mn = mx = 0
    for i in range(1, 4):
        if e[mn][1] > e[i][1]: mn = i
        if e[mx][1] < e[i][1]: mx = i
    taken = {mn}
    left = None
    for i in range(4):
        if i not in taken and (left is None or e[left][0] > e[i][0]): left = i
    taken.add(left)
    right = None
    for i in range(4):
        if i not in taken and (right is None or e[right][0] < e[i][0]): right = i
    taken.add(right)
    tail = [i for i in range(4) if i not in taken][0]
    (mnx, mny), (lx, ly), (rx, ry), tx = e[mn], e[left], e[right], e[tail][0]
    fl = _tdiv(mnx - lx, mny - ly) if mny != ly else 0
    sl = _tdiv(lx - tx, ly - tx) if ly != tx else 0
    fr = _tdiv(mnx - rx, mny - ry) if mny != ry else 0
    sr = _tdiv(rx - tx, ry - tx) if ry != tx else 0
    lstep, rstep, left_x, right_x = fl, fr, mnx, mnx
    n = k = 0
    for y in range(mny, e[mx][1] + 1):
        if y < 0 or y >= H:
            continue
        xa, xb = max(left_x, 0), min(right_x, W - 1)
        if xb >= xa:
            a = ang[y, xa:xb + 1]
            d = np.abs(theta - a)
            d = np.where(d > 3 * PI / 2, np.abs(d - 2 * PI), d)
            n += xb - xa + 1
            k += int(((a != NOTDEF) & (d <= prec)).sum())
        if y >= ly: lstep = sl
        if y >= ry: rstep = sr
        left_x += lstep
        right_x += rstep
    return n, k


def rect_improve(ang, rec, nfa):
    """(stage at which the rectangle leaves: 0 .. 5 accepted after STAGES[i], 6 rejected; trials the width guard excluded)."""
    x1, y1, x2, y2, width, theta, dx, dy, prec, p = rec

    def rn(g, prec, p):
        n, k = rect_counts(ang, g + [theta, dx, dy], prec)
        return nfa(n, k, p)
    best = [x1, y1, x2, y2, width]
    bprec, bp = prec, p
    log_nfa = rn(best, prec, p)
    if log_nfa > 0: return 0, 0
    guarded = 0
    rp = p
    for _ in range(5):
        rp /= 2
        v = rn(best, rp * PI, rp)
        if v > log_nfa: log_nfa, bprec, bp = v, rp * PI, rp
    if log_nfa > 0: return 1, 0
    for ph in (0, 1, 2):
        r = list(best)
        for _ in range(5):
            if (r[4] - 0.5) >= 0.5:
                if ph == 1:
                    r[0] += -dy * 0.25; r[1] += dx * 0.25; r[2] += -dy * 0.25; r[3] += dx * 0.25
                elif ph == 2:
                    r[0] -= -dy * 0.25; r[1] -= dx * 0.25; r[2] -= -dy * 0.25; r[3] -= dx * 0.25
                r[4] -= 0.5
                v = rn(r, bprec, bp)
                if v > log_nfa: log_nfa, best = v, list(r)
            else:
                guarded += 1
        if log_nfa > 0: return 2 + ph, guarded
    rp = bp
    for _ in range(5):
        if (best[4] - 0.5) >= 0.5:
            rp /= 2
            v = rn(best, rp * PI, rp)
            if v > log_nfa: log_nfa = v
        else:
            guarded += 1
    return (5 if log_nfa > 0 else 6), guarded


def frame_stats(img):
    """leave[i] = rectangles that leave at stage i (0 .. 5 accepted, 6 rejected), trials excluded by the width guard; checked against the oracle."""
    import oracle_lib as ol
    img = np.ascontiguousarray(img)
    h, w = img.shape
    W, H = int(round(w * 0.8)), int(round(h * 0.8))
    _, ang, _ = ol.lsd_gradient(img)
    R = ol.lsd_rects(img)
    leave = np.zeros(7, int)
    guarded = 0
    for r in R:
        st, g = rect_improve(ang, [r[0], r[1], r[2], r[3], r[4], r[7], r[8], r[9], r[10], r[11]], lambda n, k, p: ol.lsd_nfa(n, k, p, W, H))
        leave[st] += 1
        guarded += g
    nseg = len(ol.lsd_detect(img))
    assert leave[:6].sum() == nseg, (leave, nseg)
    return leave, guarded


def entering(leave):
    """rectangles entering the first test and phases -1, 0, 1, 2, 3"""
    return [int(leave.sum() - leave[:i].sum()) for i in range(6)]


if __name__ == "__main__":
    import synth_frames as sf
    for style in sys.argv[1:] or ["sticks", "struct"]:
        tot = np.zeros(7, int)
        nf = 0
        for s in range(8):
            sc = sf.Scene(640, 480, style, sf.SEED + 17 * s)
            for t in (0, 16):
                leave, _ = frame_stats(sc.gray(t))
                tot += leave
                nf += 1
        e = entering(tot)
        print(f"{style}: {nf} frames, rectangles per frame {e[0] / nf:.1f}; accepted by the first test {tot[0] / nf:.1f} ({100.0 * tot[0] / max(e[0], 1):.1f} %); "
              f"undecided entering phases -1 0 1 2 3: " + " ".join(f"{x / nf:.1f}" for x in e[1:]) + f"; accepted late {tot[1:6].sum() / nf:.1f}, rejected {tot[6] / nf:.1f}")
