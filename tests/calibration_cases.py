"""Inputs of the calibration edge tests (test_gpu_calibration_edges.py), built with numpy and the CPU oracle alone and held to
their conditions by test_calibration_cases_host.py.

  statistic_ladder   caller-supplied clip statistics whose candidate scales s_c = fl32(fl32(xm * r_c) / gmax) sit at chosen
                     places relative to the scale domain [2^-40, 2^40] of the kernels (Scale::ok, `usable` of the sorted search),
                     at the denormals, at FLT_MAX, and the special values (+-0, NaN, +Inf, a negative statistic)
  ladder_rows        the rows that go under the rungs: ONE base row times the rung's statistic, rounded once, with elements
                     on and one ulp around decision boundaries of two candidates
  degenerate_rows    rows whose OWN statistic (abs-max, 3-sigma) is degenerate
  pick / type rules  search_mse's selection (best starts at 1e10, strict '<', first best) and the type rule (first smallest
                     score, NaN last, all-NaN gives type 0) restated, with a switch for each classic mistake

Nothing here imports the HIP library."""
import math

import numpy as np

LO, HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)
FLT_MAX = np.float32(np.finfo(np.float32).max)
EPL = {"float32": 4, "bfloat16": 8, "float16": 8}
SEED = 4242
WITNESS_XM = np.float32(0.0371)             # an ordinary statistic: the witness row's


def ratios_of(lo, hi, step):
    return np.asarray([np.float32(i * 0.01) for i in range(int(lo), int(hi), int(step))], dtype=np.float32)


def scales_of(xm, ratios, gmax):
    """s_c = fl32(fl32(xm * r_c) / gmax), the reference's sequence (AQ:300, :536) in fp32 numpy: (alpha [ncand], s [ncand])"""
    with np.errstate(all="ignore"):
        alpha = (np.float32(xm) * np.asarray(ratios, np.float32)).astype(np.float32)
        return alpha, (alpha / np.float32(gmax)).astype(np.float32)


def classify(s):
    """(below, inside, above, nan) counts of candidate scales relative to [2^-40, 2^40]: zeros and negative scales count as
    below, +Inf as above"""
    s = np.asarray(s, np.float32)
    nan = np.isnan(s)
    below = ~nan & (s < LO)
    above = ~nan & (s > HI)
    return int(below.sum()), int((~nan & ~below & ~above).sum()), int(above.sum()), int(nan.sum())


def usable(s):
    """The sorted search's condition on a row's candidate scales: every one inside the domain, positive, non-decreasing"""
    s = np.asarray(s, np.float32)
    return bool(np.all(np.isfinite(s)) and np.all(s >= LO) and np.all(s <= HI) and np.all(np.diff(s) >= 0))


def _step(v, k):
    """the float32 k ulps above (k < 0: below) the positive float32 v"""
    return np.int32(int(np.float32(v).view(np.int32)) + int(k)).view(np.float32)


def _search_xm(start, want, up):
    """The float32 nearest to `start` in direction `up` (True: the smallest at or above that satisfies, found by walking ulps;
    the predicate is monotone in xm because every step of scales_of is)."""
    xm = np.float32(start)
    # walk away from the edge until `want` fails, then back to the first float where it holds
    for _ in range(64):
        if not want(xm):
            break
        xm = _step(xm, -1 if up else 1)
    for _ in range(128):
        if want(xm):
            return xm
        xm = _step(xm, 1 if up else -1)
    raise AssertionError("no statistic found near %r" % start)


def statistic_ladder(gmax, ratios):
    """[(name, xm float32, (below, inside, above, nan))]: the rungs, each landing where its name says (asserted here in fp32
    numpy; the counts are what test_calibration_cases_host.py restates)."""
    ratios = np.asarray(ratios, np.float32)
    n = ratios.size
    assert n >= 3 and np.all(np.diff(ratios) > 0)
    g = np.float64(gmax)
    S = lambda xm: scales_of(xm, ratios, gmax)[1]
    rungs = []

    def add(name, xm, counts):
        xm = np.float32(xm)
        got = classify(S(xm))
        assert got == counts, (name, xm, got, counts)
        rungs.append((name, xm, counts))

    ks = sorted({1, n // 2, n - 1})
    # ---- the lower end
    add("all below 2^-40", _search_xm(2.0 ** -40 * g / ratios[-1], lambda v: S(v)[-1] < LO, up=False), (n, 0, 0, 0))
    for k in ks:
        xm = _search_xm(2.0 ** -40 * g / ratios[k], lambda v: S(v)[k] >= LO, up=True)
        assert S(xm)[k - 1] < LO
        add("straddling 2^-40, first %d outside" % k, xm, (k, n - k, 0, 0))
    xm = _search_xm(2.0 ** -40 * g / ratios[0], lambda v: S(v)[0] >= LO, up=True)
    assert S(_step(xm, -1))[0] < LO                         # the first statistic whose candidate 0 is inside
    add("first float inside 2^-40 at c = 0", xm, (0, n, 0, 0))
    # ---- the upper end
    xm = _search_xm(2.0 ** 40 * g / ratios[-1], lambda v: S(v)[-1] <= HI, up=False)
    assert S(_step(xm, 1))[-1] > HI                         # the last statistic whose last candidate is inside
    add("last float inside 2^40 at c = n - 1", xm, (0, n, 0, 0))
    for k in ks:
        xm = _search_xm(2.0 ** 40 * g / ratios[n - k], lambda v: S(v)[n - k] > HI, up=True)
        assert S(xm)[n - k - 1] <= HI
        add("straddling 2^40, last %d outside" % k, xm, (0, n - k, k, 0))
    add("all above 2^40", _search_xm(2.0 ** 40 * g / ratios[0], lambda v: S(v)[0] > HI, up=True), (0, 0, n, 0))
    # ---- denormal alphas (every scale far below 2^-40; at 2^-149 the scales themselves are 0 or one denormal)
    tiny = np.float32(np.finfo(np.float32).tiny)
    for name, xm in (("xm = 2^-149", np.float32(2.0 ** -149)), ("every alpha denormal", np.float32(2.0 ** -140)),
                     ("some alphas denormal", np.float32(float(tiny) / float(ratios[n // 2])))):
        a = scales_of(xm, ratios, gmax)[0]
        den = int(((a > 0) & (a < tiny)).sum())
        assert den == n if "some" not in name else 0 < den < n, (name, den)
        add(name, xm, (n, 0, 0, 0))
    # ---- FLT_MAX: fl32(xm * r) overflows to +Inf for r > 1 (and for r > 1.2 below)
    for name, xm in (("xm = FLT_MAX", FLT_MAX), ("xm = FLT_MAX / 1.2", np.float32(float(FLT_MAX) / 1.2))):
        a = scales_of(xm, ratios, gmax)[0]
        ninf = int(np.isinf(a).sum())
        assert 0 < ninf < n and np.all(np.isinf(a[n - ninf:])), (name, ninf)
        add(name, xm, (0, 0, n, 0))
    # ---- special statistics
    add("xm = +0", np.float32(0.0), (n, 0, 0, 0))
    add("xm = -0", np.float32(-0.0), (n, 0, 0, 0))
    add("xm = NaN", np.float32(np.nan), (0, 0, 0, n))
    add("xm = +Inf", np.float32(np.inf), (0, 0, n, 0))
    add("xm = -0.05", np.float32(-0.05), (n, 0, 0, 0))
    return rungs


def row_multiplier(xm):
    """What the base row is multiplied by under a rung: the statistic itself, or an ordinary value where the statistic is no
    positive finite number (the row stays ordinary, only the statistic is special)"""
    xm = np.float32(xm)
    if np.isfinite(xm) and xm > 0:
        return np.float64(xm)
    if np.isfinite(xm) and xm < 0:
        return np.float64(-xm)
    return np.float64(0.05)


def base_row(K, seed=SEED):
    """float64 [K]: magnitudes in (2^-15, 1] with the largest exactly 1, both signs, exact zeros of both signs, duplicates"""
    rng = np.random.default_rng(seed + K)
    b = np.clip(np.abs(rng.standard_normal(K)) * 0.3, 2.0 ** -6, 1.0) * rng.choice([-1.0, 1.0], K)
    b[rng.permutation(K)[:max(1, K // 16)]] = 2.0 ** -14 * 1.37            # a few far below the statistic, still within 2^15
    if K >= 8:
        b[1], b[2], b[3], b[4] = 0.0, -0.0, b[5], -b[5]                    # zeros of both signs, duplicates
    if K >= 64:
        b[8:K:16] = 0.0
        b[9:K:32] = -0.0
        b[10:K:16] = b[11]
    b[0] = 1.0 if K < 8 else -1.0
    b[K - 1] = 1.0
    return b


ROUND = {"float32": lambda v: np.asarray(v, np.float64).astype(np.float32),
         "float16": lambda v: np.asarray(v, np.float64).astype(np.float16).astype(np.float32)}


def _round_bf16(v):
    v = np.asarray(v, np.float64).astype(np.float32)          # (double -> float -> bf16: the base values carry few enough bits)
    u = v.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(v), np.float32(np.nan), r).astype(np.float32)


ROUND["bfloat16"] = _round_bf16


def thresholds(grid):
    u = np.unique(np.asarray(grid, np.float64))
    return ((u[1:] + u[:-1]) / 2).astype(np.float32)


def ladder_rows(rungs, K, ratios, books, dtype="float32", cands=None):
    """(x float32 image [len(rungs) + 1, K], xm float32 [len(rungs) + 1]): row i is base_row(K) times rung i's multiplier in
    float64, rounded ONCE to dtype, its head overwritten by elements ON the decision boundaries T * s_c (and one ulp of dtype to
    either side, both signs) of two candidates c of every book (grid, gmax) -- only where s_c is a positive finite normal number
    and the element is representable.  The LAST row is the witness: the same recipe at WITNESS_XM."""
    rnd = ROUND[dtype]
    ratios = np.asarray(ratios, np.float32)
    cands = (0, ratios.size - 1) if cands is None else cands
    b = base_row(K)
    xs, xms = [], []
    for name, xm, _ in list(rungs) + [("witness", WITNESS_XM, None)]:
        with np.errstate(all="ignore"):
            row = rnd(b * row_multiplier(xm))
            vals = []
            for g, gmax in books:
                s = scales_of(xm, ratios, gmax)[1]
                for c in cands:
                    if np.isfinite(s[c]) and s[c] >= np.finfo(np.float32).tiny:
                        vals.append((thresholds(g) * s[c]).astype(np.float32))
            if vals and K >= 64:
                v = rnd(np.concatenate(vals).astype(np.float64))
                top = np.abs(row).max()
                v = v[np.isfinite(v) & (v != 0) & (np.abs(v) < top)]          # (the row's abs-max stays where base_row put it)
                v = np.concatenate([v, -v])
                nb = _neighbours(v, dtype).reshape(3, -1)                     # whole triples: a boundary with both neighbours
                nb = nb[:, np.all(np.isfinite(nb) & (np.abs(nb) < top), axis=0)]
                m = min(nb.shape[1], K // 6)
                sel = np.random.default_rng(SEED + K + len(xs)).permutation(nb.shape[1])[:m]
                row[16:16 + 3 * m] = nb[:, sel].T.reshape(-1)
        xs.append(row)
        xms.append(np.float32(xm))
    return np.stack(xs).astype(np.float32), np.asarray(xms, np.float32)


def _neighbours(v, dtype):
    """v (already representable in dtype) with its two neighbours in dtype, as float32"""
    v = np.asarray(v, np.float32)
    if dtype == "float32":
        i = v.view(np.int32)
        return np.concatenate([v, (i + 1).view(np.float32), (i - 1).view(np.float32)])
    if dtype == "float16":
        h = v.astype(np.float16)
        i = h.view(np.int16)
        with np.errstate(all="ignore"):
            return np.concatenate([h, (i + 1).view(np.float16), (i - 1).view(np.float16)]).astype(np.float32)
    i = v.view(np.int32)
    return np.concatenate([v, (i + 0x10000).view(np.float32), (i - 0x10000).view(np.float32)])


def well_scaled(x, xm, rows):
    """_well_scaled's condition (tests/test_gpu_search_exact.py) on the named rows: abs-max and statistic within 2^15 of one
    another, the domain in which the closed form's fixed-point sums are exact"""
    for r in rows:
        a, s = float(np.abs(x[r]).max()), float(xm[r])
        assert np.isfinite(a) and a > 0 and s < 2.0 ** 15 * a and a < 2.0 ** 15 * s, (r, a, s)


# ---------------------------------------------------------------------------------------------------------------------------
# rows whose own statistic is degenerate
# ---------------------------------------------------------------------------------------------------------------------------
DTYPE_MAX = {"float32": float(FLT_MAX), "bfloat16": float(np.uint32(0x7f7f0000).view(np.float32)), "float16": 65504.0}
DTYPE_MIN_SUB = {"float32": 2.0 ** -149, "bfloat16": 2.0 ** -133, "float16": 2.0 ** -24}
DEGENERATE_NAMES = ("all +0", "all -0", "mixed zeros", "one non-zero element", "constant", "all negative", "a NaN", "a +Inf", "a -Inf",
                    "NaN and Inf", "one huge element", "denormals only", "largest finite", "witness")


def degenerate_rows(dtype, K, pad=0):
    """(x float32 image [14 + pad, K] of values representable in dtype, names): DEGENERATE_NAMES in order, the last of them
    ordinary, then `pad` further ordinary rows ("ordinary 0", ...: Gaussian rows of their own seed and size, 0.005 .. 0.16).
    'one huge element' is 1e30 among 0.02-sized ones (float16, whose largest value is 65504: 60000)."""
    rnd = ROUND[dtype]
    rng = np.random.default_rng(SEED + 7 * K)
    ordinary = lambda sd=0.02: rnd(np.clip(rng.standard_normal(K), -4, 4) * sd)
    x = np.zeros((len(DEGENERATE_NAMES) + pad, K), np.float32)
    x[1] = -0.0
    x[2, 1::2] = -0.0
    x[3, K // 2] = rnd(0.37)
    x[4] = rnd(0.5)
    x[5] = rnd(-np.abs(ordinary()).astype(np.float64) - 2.0 ** -10)
    for r, spec in ((6, [np.nan]), (7, [np.inf]), (8, [-np.inf]), (9, [np.nan, np.inf])):
        x[r] = ordinary()
        for i, v in enumerate(spec):
            x[r, (K // 3 + 2 * i) % K] = v
    x[10] = ordinary()
    x[10, min(11, K - 1)] = rnd(60000.0 if dtype == "float16" else 1e30)
    x[11] = rnd(rng.integers(-3, 4, K).astype(np.float64) * DTYPE_MIN_SUB[dtype])
    x[11, 0] = DTYPE_MIN_SUB[dtype]
    x[12] = ordinary()
    x[12, K - 1] = -DTYPE_MAX[dtype]
    x[13] = ordinary()
    for i in range(pad):
        x[14 + i] = ordinary(0.005 * 2.0 ** (i % 6))
    return x, DEGENERATE_NAMES + tuple("ordinary %d" % i for i in range(pad))


# (K, what it reaches) of the per-row launches; the one-scale sizes per dtype: the smallest that knob 20 = 2 (fp32 sorted form)
# and knob 14 = 2 (16-bit histogram: any whole number of 16-byte vectors; 1024 so that the witness' bits can differ) accept
ROW_LENS = {"float32": (8, 147, 72, 128 * 4, 1024, 576 * 2, 4096 + 64), "bfloat16": (8, 147, 72, 128 * 8, 576 * 2, 4096 + 64),
            "float16": (8, 147, 72, 128 * 8, 576 * 2, 4096 + 64)}
ONE_SCALE_N = {"float32": 4096, "bfloat16": 1024, "float16": 1024}


# ---------------------------------------------------------------------------------------------------------------------------
# the selection rules, restated -- with a switch per classic mistake
# ---------------------------------------------------------------------------------------------------------------------------
MISTAKES = ("denormal scale flushed to zero", "<= instead of <", "best started at +Inf", "NaN score treated as small",
            "type pick not skipping NaN", "last type on ties")


def pick_rule(trace, xm, ratios, mistake=None):
    """search_mse's selection on a [ncand, na] float32 trace (AQ:299-306): (best [na], alpha [na]) float32; best starts at
    1e10, candidates ascending, strict '<'; alpha = fl32(xm * r_c) of the pick, xm itself without one."""
    trace = np.asarray(trace, np.float32)
    ncand, na = trace.shape
    best = np.full(na, np.float32(np.inf if mistake == "best started at +Inf" else 1e10), np.float32)
    alpha = np.asarray(xm, np.float32).copy()
    with np.errstate(all="ignore"):
        for c in range(ncand):
            t = trace[c]
            better = (t <= best) if mistake == "<= instead of <" else (t < best)
            if mistake == "NaN score treated as small":
                better = better | (np.isnan(t) & ~np.isnan(best))
            alpha = np.where(better, (np.asarray(xm, np.float32) * np.float32(ratios[c])).astype(np.float32), alpha)
            best = np.where(better, t, best).astype(np.float32)
    return best, alpha


def type_rule(score, mistake=None):
    """np.argsort(score)[0] (AQ:413-415) spelled out: the first smallest score, NaN last, all-NaN gives type 0"""
    score = np.asarray(score, np.float32)
    bt, have = 0, False
    for t in range(score.size):
        v = score[t]
        if np.isnan(v) and mistake != "type pick not skipping NaN":
            continue
        if not have:
            bt, have = t, True
        elif mistake == "type pick not skipping NaN":
            if not (score[bt] <= v):                      # (a comparison chain that lets NaN through: min-by-not-greater)
                bt = t
        elif v < score[bt] or (mistake == "last type on ties" and v == score[bt]):
            bt = t
    return bt


def type_score(best):
    """score[t] of antq_calibrate: fl32 of the exact sum of the rows' best MSEs (a double sum of a few thousand floats lies far
    inside half a float ulp of it)"""
    return np.float32(math.fsum(float(v) for v in np.asarray(best, np.float32)))


def flushed_trace(oracle, x, xm, lb, ub, step, grid, gmax, ovp, per_row=True):
    """oracle.search_mse's trace with the mistake `a denormal scale flushed to zero` applied: candidates whose alpha or scale is
    denormal are scored as the oracle scores a ZERO alpha"""
    ratios = ratios_of(lb, ub, step)
    best, alpha, trace = oracle.search_mse(x, xm, lb, ub, step, grid, gmax, ovp, per_row)
    trace = trace.copy()
    tiny = np.finfo(np.float32).tiny
    for c in range(ratios.size):
        a, s = scales_of(np.asarray(xm, np.float32), ratios[c:c + 1].repeat(np.size(xm)), gmax)
        den = ((np.abs(a) > 0) & (np.abs(a) < tiny)) | ((np.abs(s) > 0) & (np.abs(s) < tiny))
        if den.any():
            with np.errstate(all="ignore"):
                z = np.where(den, np.float32(0.0), a).astype(np.float32)
                out = oracle.forward(x, z if per_row and x.shape[0] > 1 else z[:1], grid, gmax, ovp, want_idx=False)[0]
                sc = oracle.mse(out, x, per_row)
            trace[c] = np.where(den, sc, trace[c])
    return trace


# planted score vectors for the type rule (the scores a calibration can produce never hold a NaN: a row's best is a finite
# mean squared error or 1e10 -- so the NaN clauses of the rule are pinned on planted vectors)
_N = np.float32(np.nan)
PLANTED_SCORES = tuple(np.float32(v) for v in (
    [1.0], [_N], [2.0, 1.0], [1.0, 1.0], [_N, 1.0], [1.0, _N], [_N, _N], [3.0, 1.0, 1.0], [1.0, 3.0, 1.0], [_N, 2.0, 1.0], [2.0, _N, 1.0],
    [2.0, 1.0, _N], [_N, _N, _N], [1e10, 1e10, 1e10, 1e10], [_N, 1e10, _N, 5.0], [5.0, 4.0, 3.0, 2.0, 1.0], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
    [_N, 7.0, 7.0, _N, 7.0, 2.0, 2.0], [9.0, 8.0, 7.0, 6.0, 5.0, 4.0, 3.0, 3.0], [_N, _N, _N, _N, _N, _N, _N, 0.0]))
