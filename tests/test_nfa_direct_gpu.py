"""nfa(n, k, p) of LSD_REFINE_ADV on the trials of tests/nfa_cases.py, run through the product's own k_lsd_nfa_setup / k_lsd_nfa_series
(pslfe_line_debug_nfa, a 640 x 480 extractor) and compared bit for bit with the CPU oracle over the restated functions
(oracle_lib.set_nfa_math(1)): the value where no series is summed, the binomial tail where one is.  tests/test_debug_math_cpu.py shows
without a GPU which branches of the kernels the list reaches."""
import numpy as np
import pytest

import nfa_cases
import oracle_lib

pytestmark = pytest.mark.gpu

W, H = nfa_cases.W, nfa_cases.H
FMAX = 17
_cache = {}


def _le():
    if "le" not in _cache:
        import psl_slam_amd as P
        _cache["le"] = P.LINEextractor(1, 1.2, 200, 0.0, max_batch=FMAX)
    return _cache["le"]


def _log_nt():
    if "lognt" not in _cache:
        _, _, _cache["lognt"] = _le().debug_nfa(W, H, -2, [0], np.zeros((1, 1, 2)) + 0.5, np.zeros((1, 1, 5, 2), np.int32))
    return _cache["lognt"]


def _trials():
    cs = nfa_cases.cases()
    return tuple(np.array([c[i] for c in cs]) for i in (1, 2, 3))


def _ref(shift):
    """(v, tail) of the oracle for every trial at p / 2^shift: computed once"""
    if ("ref", shift) not in _cache:
        n, k, p = _trials()
        old = oracle_lib.set_nfa_math(1)
        try:
            _cache[("ref", shift)] = oracle_lib.lsd_nfa_lognt_tail(n, k, p / 2.0 ** shift, _log_nt())
        finally:
            oracle_lib.set_nfa_math(old)
        assert np.isfinite(_cache[("ref", shift)][0]).all()
    return _cache[("ref", shift)]


def _layout(per_rect, per_frame):
    """Where every trial goes: rectangles hold `per_rect` trials of ONE p (the last rectangle of a p is filled up with trials the
    width guard excludes), frames hold `per_frame` rectangles.  -> (frame, rect, slot) per trial, rectangles per frame"""
    if ("layout", per_rect, per_frame) not in _cache:
        n, k, p = _trials()
        where = np.zeros((len(n), 3), np.int64)
        rect = 0
        for q in np.unique(p):
            idx = np.flatnonzero(p == q)
            for j, i in enumerate(idx):
                where[i] = ((rect + j // per_rect) // per_frame, (rect + j // per_rect) % per_frame, j % per_rect)
            rect += (len(idx) + per_rect - 1) // per_rect
        F = (rect + per_frame - 1) // per_frame
        assert F <= FMAX
        nrect = np.full(F, per_frame, np.int32)
        nrect[-1] = rect - (F - 1) * per_frame
        _cache[("layout", per_rect, per_frame)] = (where, nrect)
    return _cache[("layout", per_rect, per_frame)]


def _run(phase, lin, per_rect=None):
    """every trial through phase `phase` with incoming log_nfa lin[trial] -> (vals, tail) per trial, and those of the padding"""
    n, k, p = _trials()
    first = phase == -2
    per_rect = per_rect or (1 if first else 5)
    where, nrect = _layout(per_rect, 4096 if first else (128 if per_rect == 5 else 600))
    F, R = len(nrect), int(nrect.max())
    pl = np.zeros((F, R, 2))
    pl[..., 0], pl[..., 1] = 0.5, -1000.0
    nk = np.zeros((F, R, 5, 2), np.int32)
    nk[..., 0] = -1
    f, r, t = where.T
    pl[f, r, 0] = p
    pl[f, r, 1] = lin   # a rectangle carries ONE log_nfa: per trial only with one trial per rectangle
    nk[f, r, t, 0], nk[f, r, t, 1] = n, k
    vals, tail, lognt = _le().debug_nfa(W, H, phase, nrect, pl, nk)
    assert lognt == _log_nt()
    used = np.zeros((F, R, 5), bool)
    used[f, r, t] = True
    live = np.arange(R)[None, :, None] < nrect[:, None, None]
    pad = live & ~used & (np.arange(5)[None, None, :] < (1 if first else 5))
    return vals[f, r, t], tail[f, r, t], vals[pad], tail[pad], t


def _same(a, b):
    return a.view(np.uint64) == b.view(np.uint64)


def _report(what, n, k, p, bad, got, ref):
    i = np.flatnonzero(bad)[:6]
    return f"{what}: {bad.sum()} trials differ; (n, k, p, device, oracle): {[(int(n[j]), int(k[j]), float(p[j]), float(got[j]).hex(), float(ref[j]).hex()) for j in i]}"


@pytest.mark.parametrize("phase", [-2, -1, 0, 1, 2, 3])
def test_every_trial_without_an_early_stop(phase):
    """incoming log_nfa = -1000: `stop` stays +inf, every series is summed to the reference's own truncation point.  In phases -1 and
    3 trial t is evaluated at p / 2^(t+1).  The padding trials (n < 0, the width guard) give -inf and no series."""
    n, k, p = _trials()
    v, tail, vpad, tpad, slot = _run(phase, -1000.0)
    if phase in (-1, 3):
        refs = [_ref(s) for s in range(1, 6)]
        v_ref = np.choose(slot, [r[0] for r in refs])
        t_ref = np.choose(slot, [r[1] for r in refs])
        p_eff = p / 2.0 ** (slot + 1)
    else:
        (v_ref, t_ref), p_eff = _ref(0), p
    series = t_ref > 0
    print(f"phase {phase}: {len(n)} trials, {series.sum()} with a series, {len(vpad)} excluded")
    bad_t = ~_same(tail, t_ref)
    assert not bad_t.any(), _report("binomial tail", n, k, p_eff, bad_t, tail, t_ref)
    bad_v = ~series & ~_same(v, v_ref)
    assert not bad_v.any(), _report("value without a series", n, k, p_eff, bad_v, v, v_ref)
    if phase != -2:
        assert len(vpad) > 0
    assert (vpad == -np.inf).all() and (tpad == 0).all()


@pytest.mark.parametrize("phase", [0, 1, 2])
def test_near_the_threshold(phase):
    """incoming log_nfa = the trial's own value + d: a trial that still wins (log_nfa_in < v) must be summed to the end, bit for bit;
    one that has lost may come back as +inf (the series ended at its `stop`) or complete"""
    n, k, p = _trials()
    v_ref, t_ref = _ref(0)
    # one trial per rectangle (slot 0; the other four are excluded by the width guard), since a rectangle carries one log_nfa
    wins = loses_equal = loses_inf = 0
    ds = [1e-3, -1e-3, 1e-5, -1e-5, 1e-6, -1e-6, 4e-7, -4e-7, 1e-7, -1e-7, 1e-9, -1e-9, 0.0, "+ulp", "-ulp"]
    for d in ds:
        if d == "+ulp":
            lin = np.nextafter(v_ref, np.inf)
        elif d == "-ulp":
            lin = np.nextafter(v_ref, -np.inf)
        else:
            lin = v_ref + d
        v, tail, vpad, tpad, _ = _run(phase, lin, per_rect=1)
        assert (vpad == -np.inf).all() and (tpad == 0).all()
        win = lin < v_ref
        bad = win & ~_same(tail, t_ref)
        assert not bad.any(), _report(f"d = {d}: a winning trial", n, k, p, bad, tail, t_ref)
        inf = ~win & (tail == np.inf)
        bad = ~win & ~inf & ~_same(tail, t_ref)
        assert not bad.any(), _report(f"d = {d}: a lost trial that was summed", n, k, p, bad, tail, t_ref)
        noser = (t_ref == 0) & ~_same(v, v_ref)
        assert not noser.any(), _report(f"d = {d}: value without a series", n, k, p, noser, v, v_ref)
        wins += int(win.sum())
        loses_inf += int(inf.sum())
        loses_equal += int((~win & ~inf).sum())
    print(f"phase {phase}: {wins} winning trials summed to the end, {loses_inf} lost trials ended at their stop, {loses_equal} lost trials summed to the end")
    assert wins >= 500 and loses_inf > 0 and loses_equal > 0


def test_several_frames():
    """17 frames = two PSL_NFA_FG groups, with 0, 1 and 300 rectangles (more than 256 items of one class), the same rectangles in frames
    0 and 16: every frame as in a launch of its own"""
    n, k, p = _trials()
    rng = np.random.default_rng(5)
    pick = rng.permutation(np.flatnonzero((_ref(0)[1] > 0) & (p == nfa_cases.P0) & (n < 3000)))[:1500]
    R = 300
    counts = [300, 0, 1, 7, 300, 64, 0, 256, 257, 1, 33, 300, 5, 128, 255, 2, 300]
    assert len(counts) == FMAX
    pl = np.zeros((FMAX, R, 2))
    pl[..., 0], pl[..., 1] = nfa_cases.P0, -1000.0
    nk = np.zeros((FMAX, R, 5, 2), np.int32)
    nk[..., 0] = -1
    for f in range(FMAX):
        sel = rng.choice(pick, (R, 5))
        nk[f, :, :, 0], nk[f, :, :, 1] = n[sel], k[sel]
        nk[f, ::7, 3, 0] = -1   # some excluded trials
    nk[16], pl[16] = nk[0], pl[0]
    for phase in (-2, 0, 3):
        v, t, _ = _le().debug_nfa(W, H, phase, counts, pl, nk)
        for f in range(FMAX):
            c = counts[f]
            v1, t1, _ = _le().debug_nfa(W, H, phase, [c], pl[f:f + 1], nk[f:f + 1])
            tr = 1 if phase == -2 else 5
            assert v[f, :c, :tr].tobytes() == v1[0, :c, :tr].tobytes() and t[f, :c, :tr].tobytes() == t1[0, :c, :tr].tobytes(), (phase, f)
            assert np.isnan(v[f, c:]).all()   # rows beyond the frame's count are not written
        assert v[0].tobytes() == v[16].tobytes() and t[0].tobytes() == t[16].tobytes()


def test_width_guard_and_arguments():
    import psl_slam_amd as P
    pl = np.zeros((1, 4, 2))
    pl[..., 0], pl[..., 1] = nfa_cases.P0, -1000.0
    nk = np.zeros((1, 4, 5, 2), np.int32)
    nk[0, :, :, 0], nk[0, :, :, 1] = 100, 30
    nk[0, 1, 2] = (-1, 0)
    nk[0, 3, :] = (-1, 0)
    v, t, lognt = _le().debug_nfa(W, H, 1, [4], pl, nk)
    excluded = nk[0, :, :, 0] < 0
    assert (v[0][excluded] == -np.inf).all() and (t[0][excluded] == 0).all()
    assert np.isfinite(v[0][~excluded]).all() and (t[0][~excluded] > 0).all()
    assert abs(lognt - nfa_cases.LOG_NT) < 1e-12
    for bad in (dict(phase=4), dict(phase=-3), dict(nrect=[5]), dict(nrect=[-1])):
        with pytest.raises(P.PslfeError):
            _le().debug_nfa(W, H, bad.get("phase", 0), bad.get("nrect", [4]), pl, nk)
    nk2 = nk.copy()
    nk2[0, 0, 0] = (10, 11)   # k > n
    with pytest.raises(P.PslfeError):
        _le().debug_nfa(W, H, 0, [4], pl, nk2)
    with pytest.raises(P.PslfeError):
        _le().debug_nfa(W, H, 0, [1] * (FMAX + 1), np.tile(pl, (FMAX + 1, 1, 1)), np.tile(nk, (FMAX + 1, 1, 1, 1)))
