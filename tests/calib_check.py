"""Clip-pick / type-pick parity against the reference's OWN per-candidate scores.

`tests/golden/*_traces.npz` (make_golden.py, round 2) hold, for every complete `TensorQuantizer(x)` calibration
recorded from the reference's Python, the [ncand, rows] matrix of `mse_loss` values its final `search_mse` saw and the
per-type sums its type selection compared.  A replacement may pick a different clip candidate than the reference only
where the REFERENCE's scores of the two candidates tie within its own fp32 reduction noise; these helpers
assert exactly that, row by row, instead of allowing a percentage of rows to differ -- with the noise MEASURED on the
reference (round 6: tests/golden/*_traces64.npz) rather than guessed, and a ledger of how much of it was used.
"""
import glob
import os

import numpy as np


def reference_score_noise():
    """max |fp32 score - fp64 score| / score over EVERY score the reference computed while the trace fixtures were recorded
    (tests/golden/*_traces64.npz, make_golden.py round 6: the same float32 element terms, the mean taken in float64).  This
    is the reference's own reduction noise -- how far one of its MSE values can sit from the number it stands for.
    Returns (max, number of scores compared)."""
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    worst, n = 0.0, 0
    for f64 in sorted(glob.glob(os.path.join(gold, "*_traces64.npz"))):
        d64 = np.load(f64)
        srcs = [np.load(p) for p in (f64.replace("_traces64", "_traces"), f64.replace("_traces64", "")) if os.path.exists(p)]
        for k in d64.files:
            k32 = k[:-2]                                        # "...trace64" -> "...trace"
            src = next((d for d in srcs if k32 in d.files), None)
            assert src is not None, (f64, k)
            a, b = src[k32].astype(np.float64).reshape(d64[k].shape), d64[k]
            ok = np.isfinite(a) & np.isfinite(b) & (b != 0)
            if ok.any():
                worst = max(worst, float((np.abs(a[ok] - b[ok]) / np.abs(b[ok])).max()))
                n += int(ok.sum())
    assert n > 100000, "the *_traces64.npz fixtures are missing"
    return worst, n


REFERENCE_SCORE_NOISE, _N_SCORES = reference_score_noise()
# Two correct implementations may pick different candidates a (the reference: argmin of its noisy fp32 scores s32) and c
# (ours: argmin of sums formed in float64, s64) only when  s32(c) - s32(a) <= |s32(c) - s64(c)| + |s64(a) - s32(a)|, i.e.
# within TWICE the reference's reduction noise.  Round 5 used 2e-5 (20 x SURVEY 8c's 1e-6); measured on the fixtures the
# noise is 3.0e-7, so the rule is 5.9e-7 -- tighter than the survey's.
NEAR_TIE_RTOL = 2.0 * REFERENCE_SCORE_NOISE

# every call of check_alpha_picks / check_type_pick leaves a line here: (key, rows, identical picks, largest certified gap)
LEDGER = []


def ledger_summary(prefix=""):
    """(rows, identical picks, fraction, largest certified gap) over the ledger entries whose key starts with `prefix`."""
    rows = [e for e in LEDGER if e[0].startswith(prefix)]
    n, same = sum(e[1] for e in rows), sum(e[2] for e in rows)
    return n, same, (same / n if n else 1.0), max([e[3] for e in rows] + [0.0])


def ratios_of(lo, hi, step):
    """fl32(i * 0.01) for the reference's `range(lo, hi, step)` (AQ:298-300 / OQ:206-207)."""
    return np.asarray([np.float32(i * 0.01) for i in range(int(lo), int(hi), int(step))], dtype=np.float32)


def reference_pick(trace):
    """Index of the reference's pick per row: best starts at 1e10, strict '<', ascending candidates (AQ:299-306)."""
    ncand, rows = trace.shape
    best = np.full(rows, np.float32(1e10), dtype=np.float32)
    pick = np.full(rows, -1, dtype=np.int64)
    for c in range(ncand):
        better = trace[c] < best
        pick[better] = c
        best[better] = trace[c][better]
    return pick, best


def check_alpha_picks(key, got_alpha, ref_alpha, trace, ratios, xmax_rtol=2e-6):
    """Every row: the candidate we picked is the reference's, or one whose REFERENCE score is within NEAR_TIE_RTOL of
    the reference's best.  Also pins x_max (abs-max / 3-sigma rule): alpha / ratio must agree with the reference's.
    Returns the boolean mask of rows whose pick is identical to the reference's."""
    got = np.asarray(got_alpha, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref_alpha, dtype=np.float32).reshape(-1)
    trace = np.asarray(trace, dtype=np.float32)
    assert trace.shape == (ratios.size, ref.size), (key, trace.shape, ratios.size, ref.size)
    pick, best = reference_pick(trace)
    same = np.zeros(ref.size, dtype=bool)
    max_gap = 0.0
    for r in range(ref.size):
        if pick[r] < 0:                       # no candidate qualified: alpha stays x_max
            assert np.isclose(got[r], ref[r], rtol=xmax_rtol), (key, r, got[r], ref[r])
            same[r] = True
            continue
        xmax = np.float64(ref[r]) / np.float64(ratios[pick[r]])
        if xmax == 0.0 or not np.isfinite(xmax):
            assert got[r] == ref[r] or (np.isnan(got[r]) and np.isnan(ref[r])), (key, r)
            same[r] = True
            continue
        rel = np.abs(np.float64(got[r]) / xmax - ratios.astype(np.float64))
        c = int(np.argmin(rel))
        tol = (4 * xmax_rtol + 3e-7) * ratios[c]        # 3e-7: the reference's alpha is itself a rounded product
        assert rel[c] <= tol, (key, r, "alpha is not x_max times a candidate ratio", got[r], xmax)
        if c == pick[r]:
            same[r] = True
            continue
        gap = (np.float64(trace[c, r]) - np.float64(best[r])) / np.float64(best[r])
        assert gap <= NEAR_TIE_RTOL, (key, r, "picked candidate %d, reference %d, reference MSE gap %.3g (allowed %.3g)" % (
            c, pick[r], gap, NEAR_TIE_RTOL))
        max_gap = max(max_gap, float(gap))
    LEDGER.append((str(key), int(ref.size), int(same.sum()), max_gap))
    return same


def check_type_pick(key, got_mode, ref_mode, types, type_sums):
    """A different winning type is acceptable only when the reference's own summed scores of the two tie."""
    if got_mode == ref_mode:
        LEDGER.append(("type:" + str(key), 1, 1, 0.0))
        return
    sums = dict(zip(types, [float(v) for v in type_sums]))
    assert got_mode in sums and ref_mode in sums, (key, got_mode, ref_mode, types)
    gap = abs(sums[got_mode] - sums[ref_mode]) / sums[ref_mode]
    assert gap <= NEAR_TIE_RTOL, (key, "type %s vs reference %s, reference sums differ by %.3g" % (got_mode, ref_mode, gap))
    LEDGER.append(("type:" + str(key), 1, 0, float(gap)))


# Bars of the GPU tests against the yardstick (tests/test_gpu_search_exact.py).  Each is derived from the worst relative
# deviation measured on the MI355X over every (codebook, candidate, row) cell of every case, against the yardstick and never
# against another kernel (profiles/search_exactness.md: 8.7e5 cells):
#   closed forms (sorted-row search, sweep) vs `exact`: worst 2.0e-13 (rows of 256 elements under OliVe's codebooks, where a few
#     exactly-represented outliers make sum x^2 a thousand times the sum of squared errors: 2^-53 times that condition
#     number).  8 x worst = 1.6e-12 exceeds the ceiling of 1e-12 -- the point where a single misplaced element of a
#     16 384-wide row (1 %-quantile 1.6e-10) stops being resolved with two orders of margin -- so the ceiling is the bar.
#   histogram search vs `terms32`: worst 1.4e-15, bar 8 x, rounded up.
#   direct kernels vs `terms32`: worst 1.3e-7 (ANT) / 1.5e-7 (OliVe): they add a lane's float32 terms in float32.  Bar 2 x.
EXACT_RTOL = 1e-12                  # sorted-row search and sweep vs `exact`
EXACT_RTOL_FAR_STATISTIC = 7e-14    # ... the named row whose statistic lies 2^15 and more above its elements (worst 8.2e-15)
HIST_RTOL = 2e-14                   # histogram search vs `terms32`
DIRECT_RTOL = 3e-7                  # direct kernels vs `terms32`, ANT codebooks
DIRECT_RTOL_OLIVE = 3e-7            # direct kernels vs `terms32`, OliVe codebooks


def exact_sse(oracle, x2d_f32, xmax, ratios, grid, gmax, ovp, per_row):
    """The yardstick of every clip-search kernel: the float64 sums of squared errors of the oracle's per-element outputs.

    For every candidate c:  alpha = fl32(xmax * ratios[c])  (the reference's scale, `ratios_of`),  out = oracle.forward(x, alpha),
    d = fl32(out - x).  Returns two float64 arrays [ncand, rows] (per_row) or [ncand, 1] (one scale for the tensor):
      exact   = sum of float64(d)^2             -- what the closed forms of the sorted-row search and the sweep stand for
      terms32 = sum of float64(fl32(d * d))     -- what the direct kernels and the histogram search stand for, and what the
                                                   reference's *_traces64.npz record (its float32 element terms, mean in float64)
    Both sums are numpy's float64 pairwise sums over a row (error <= log2(n) * 2^-53 relative on non-negative terms).  A
    16-bit tensor enters as its float32 image.  NaN / Inf / zero-statistic rows give what the float64 arithmetic gives."""
    x = np.ascontiguousarray(x2d_f32, dtype=np.float32)
    assert x.ndim == 2
    rows = x.shape[0]
    na = rows if per_row else 1
    xmax = np.asarray(xmax, dtype=np.float32).reshape(-1)
    assert xmax.size == na, (xmax.size, na)
    ratios = np.asarray(ratios, dtype=np.float32).reshape(-1)
    exact = np.empty((ratios.size, na), dtype=np.float64)
    terms32 = np.empty((ratios.size, na), dtype=np.float64)
    with np.errstate(all="ignore"):
        for c in range(ratios.size):
            alpha = (xmax * ratios[c]).astype(np.float32)
            if per_row and rows == 1:        # (oracle.forward reads a single alpha as one scale for the tensor: the same thing)
                alpha = alpha[:1]
            out = oracle.forward(x, alpha, grid, gmax, ovp, want_idx=False)[0]
            d = (out - x).astype(np.float32)
            d64 = d.astype(np.float64)
            t32 = (d * d).astype(np.float32).astype(np.float64)
            if per_row:
                exact[c], terms32[c] = (d64 * d64).sum(axis=1), t32.sum(axis=1)
            else:
                exact[c, 0], terms32[c, 0] = (d64 * d64).sum(), t32.sum()
    return exact, terms32


def _round_bf16(v):
    """float32 -> the nearest bfloat16 (ties to even) as float32; NaN stays NaN."""
    v = np.asarray(v, dtype=np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(v), np.float32(np.nan), r).astype(np.float32)


ROUND_TO = {"float32": lambda v: np.asarray(v, dtype=np.float32),
            "bfloat16": _round_bf16,
            "float16": lambda v: np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float32)}


def exact_three_sigma(x, per_row, dtype="float32"):
    """The yardstick of antq_moments + antq_xmax_3sigma: OliVe's clip statistic max(|mean + 3 std|, |mean - 3 std|)
    (OQ:193-197, :213-218) from the EXACT mean and the exact centred second moment -- no one-pass sums, no cancellation.

    x: 2-D array holding the tensor's values (a 16-bit tensor as its float32 image); per row, or over everything.  The
    mean is math.fsum(row) / n (the sum correctly rounded), the variance math.fsum((v - mean)^2) / (n - 1) (unbiased,
    torch.std's default; each term carries two float64 roundings, 2^-52 relative), then the roundings include/antq.h
    documents for `dtype`: float32 -- mean and std rounded to float, 3 * std, the sum and the difference in float;
    bfloat16 / float16 -- each of the five rounded to the tensor's dtype.  One element: NaN (0 / 0), like torch.std.
    Returns float32 [rows or 1]."""
    import math
    rnd = ROUND_TO[dtype]
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1) if per_row else x.reshape(1, -1)
    n = x.shape[1]
    mean, std = np.empty(x.shape[0]), np.empty(x.shape[0])
    for r in range(x.shape[0]):
        mean[r] = math.fsum(x[r].tolist()) / n
        d = x[r] - mean[r]
        std[r] = math.sqrt(math.fsum((d * d).tolist()) / (n - 1)) if n > 1 else np.nan
    with np.errstate(all="ignore"):
        m, sd = rnd(mean.astype(np.float32)), rnd(std.astype(np.float32))
        t3 = rnd(np.float32(3.0) * sd)
        a, b = np.abs(rnd(m + t3)), np.abs(rnd(m - t3))
        return np.where(np.isnan(a) | np.isnan(b), np.float32(np.nan), np.maximum(a, b)).astype(np.float32)


def _three_sigma_reference(x, per_row):
    """OliVe's clip statistic in the reference's own op sequence (OQ:193-195 / :213-215: torch float32 mean, std, 3 * std, sum,
    difference).  The recorded scores depend on this float32 value to the bit, and a float64 restatement of it lands one ulp
    away on about half of the rows -- so the statistic (an INPUT of the search, not the thing under test) is restated with
    the library the recorder ran: torch on the CPU."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if per_row:
        mean, std = t.view(t.shape[0], -1).mean(dim=-1), t.view(t.shape[0], -1).std(dim=-1)
    else:
        mean, std = t.mean(), t.std()
    return torch.maximum((mean + 3 * std).abs(), (mean - 3 * std).abs()).reshape(-1).numpy().astype(np.float32)


def _absmax(x, per_row):
    return (np.abs(x).max(1) if per_row else np.abs(x).max(keepdims=True).reshape(1)).astype(np.float32)


def restated_traces64(oracle, path):
    """Every calibration recorded in one tests/golden/*_traces64.npz, restated as the arguments of its FINAL clip search
    (the one on the installed grid): a list of dicts with key, x [rows, K] float32, xmax, lo / up / step, ratios, grid, gmax,
    ovp, per_row and trace64 [ncand, rows or 1] (the reference's float32 element terms, averaged in float64).
    OliVe: grid = the normal values followed by the outliers, gmax = normal.max(), 3-sigma statistic under the pair rule and
    abs-max without outliers (OQ:193-218), as tests/test_oracle_golden.py restates them."""
    name = os.path.basename(path)
    tree = name.split("_")[0]
    t64 = np.load(path)
    base = np.load(path.replace("_traces64", ""))
    step = 1 if tree == "ant" else 2
    cases = []
    for k64 in t64.files:
        trace64 = t64[k64]
        if k64.endswith("__trace64"):                            # a complete TensorQuantizer calibration
            k = k64[:-len("__trace64")]
            parts = k.split("__")
            tname = parts[0]
            xkey = next(c for c in (tname + "__x", tname[5:] + "_x" if tname.startswith("full_") else "") if c in base.files)
            per_row = tname.startswith(("w", "full_w"))
            bit = int(parts[2][1:]) if len(parts) > 2 else 4
            lo, up = map(int, parts[3].split("_")) if len(parts) > 3 else (75, 150 if tree == "ant" else 250)
            if tree == "ant" and bit > 6:
                lo = 95                                          # AQ:296-297
            normal = base[k + "__grid"]
            ovp = tree == "olive" and not k.endswith("__noout")
            grid = np.concatenate([normal, base[k + "__outliers"]]) if ovp else normal
        else:                                                    # a single search_mse of the round-1 fixtures
            k = k64[:-len("_trace64")]
            parts = k.split("_")
            tname, t = parts[0], parts[1]
            xkey = ("a_x" if tname.startswith("a") else "w_x")
            per_row = tname == "w"
            lo, up = 75, 150 if tree == "ant" else 250
            if tree == "ant":
                normal, ovp = oracle.ant_grid(t, 4, tname != "au"), False
                grid = normal
            else:
                normal, ovp = oracle.olive_grid(t, 4, True), parts[2] == "ovp"
                grid = np.concatenate([normal, oracle.olive_outlier_value(4, True)]) if ovp else normal
        x = np.asarray(base[xkey], dtype=np.float32)
        x = x.reshape(x.shape[0], -1)
        if tname == "au":
            x = np.abs(x)
        xmax = _three_sigma_reference(x, per_row) if ovp else _absmax(x, per_row)
        cases.append(dict(key=k, x=x, xmax=xmax, lo=lo, up=up, step=step, ratios=ratios_of(lo, up, step),
                          grid=np.asarray(grid, dtype=np.float32), gmax=float(np.max(normal)), ovp=ovp, per_row=per_row,
                          trace64=trace64))
    return cases
