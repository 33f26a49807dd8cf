"""The input builders of the calibration edge tests (calibration_cases.py) against the CPU oracle alone, no GPU: every rung of
the statistic ladder has the stated number of candidate scales below, inside and above [2^-40, 2^40]; the oracle's NaN pattern
and its `no eligible candidate` rows (best = 1e10, alpha = x_max bit for bit) are where the builder says; the rows under usable
rungs are inside the closed form's exact domain; and each classic mistake of the selection, restated on the oracle's side,
changes the expected pick, score or type of at least one case (the counts are printed).  A failure of
test_gpu_calibration_edges.py is then the kernels', not the inputs'."""
import numpy as np
import pytest

import calib_check
import calibration_cases as cc

ANT = (75, 150, 1)
OLIVE = (75, 250, 2)


def _books(oracle):
    ant = [(oracle.ant_grid(t, 4, True), 10.0) for t in ("int", "flint")]
    oo = oracle.olive_outlier_value(4, True)
    olive = [(np.concatenate([oracle.olive_grid(t, 4, True), oo]), float(oracle.olive_grid(t, 4, True).max())) for t in ("int", "flint")]
    return ant, olive


def _no_eligible_said(name):
    """The rungs said to have no eligible candidate: a zero, NaN or Inf scale for every candidate, or -- from s = 2^40 / 1.5 up --
    a mean squared error of the order of (s / 3)^2 = 1e22 and more, which is not below 1e10 (at FLT_MAX the float32 terms
    overflow to Inf)"""
    return "2^40" in name or "FLT_MAX" in name or name in ("xm = 2^-149", "xm = +0", "xm = -0", "xm = NaN", "xm = +Inf")


@pytest.mark.parametrize("family", ["ant", "olive"])
def test_every_rung_lands_where_it_says(oracle, family):
    ant, olive = _books(oracle)
    lo, up, step = ANT if family == "ant" else OLIVE
    ratios = cc.ratios_of(lo, up, step)
    assert np.array_equal(ratios, calib_check.ratios_of(lo, up, step))
    n = ratios.size
    for g, gmax in (ant if family == "ant" else olive):
        rungs = cc.statistic_ladder(gmax, ratios)
        names = [r[0] for r in rungs]
        assert len(set(names)) == len(names) == 20, names
        for name, xm, counts in rungs:
            with np.errstate(all="ignore"):
                s64 = (np.float32(xm) * ratios).astype(np.float32).astype(np.float64) / np.float64(np.float32(gmax))
            s = s64.astype(np.float32)                 # (the float32 quotient, correctly rounded from its exact value)
            nan = int(np.isnan(s).sum())
            below = int((s < 2.0 ** -40).sum())
            above = int((s > 2.0 ** 40).sum())
            assert (below, n - below - above - nan, above, nan) == counts and sum(counts) == n, (name, counts)
            assert cc.usable(s) == (counts[1] == n), name
        by = dict((r[0], r) for r in rungs)
        assert by["first float inside 2^-40 at c = 0"][2] == (0, n, 0, 0) and by["all below 2^-40"][2] == (n, 0, 0, 0)
        assert by["straddling 2^-40, first 1 outside"][2] == (1, n - 1, 0, 0) and by["straddling 2^40, last 1 outside"][2] == (0, n - 1, 1, 0)
        assert np.signbit(by["xm = -0"][1]) and not np.signbit(by["xm = +0"][1])


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_rows_under_usable_rungs_are_well_scaled(oracle, dtype):
    ant, _ = _books(oracle)
    ratios = cc.ratios_of(*ANT)
    rungs = cc.statistic_ladder(10.0, ratios)
    for K in cc.ROW_LENS[dtype] + (cc.ONE_SCALE_N[dtype],):
        x, xm = cc.ladder_rows(rungs, K, ratios, ant, dtype)
        assert x.shape == (len(rungs) + 1, K) and xm[-1] == cc.WITNESS_XM
        assert np.array_equal(cc.ROUND[dtype](x.astype(np.float64)), x, equal_nan=True), "a value is not representable in the dtype"
        ok = [i for i, (name, v, counts) in enumerate(rungs) if counts[1] == ratios.size and cc.DTYPE_MIN_SUB[dtype] * 2.0 ** 40 < v < cc.DTYPE_MAX[dtype]]
        # (one out-of-domain candidate makes the whole row unusable: the two rungs at the first / last float inside, where the
        #  dtype can hold them -- float16 cannot -- and the witness)
        assert len(ok) == (2 if dtype != "float16" else 0), (dtype, K, ok)
        cc.well_scaled(x, xm, ok + [len(rungs)])
        b = cc.base_row(K)
        assert np.abs(b).max() == 1.0 and np.all((b == 0) | (np.abs(b) > 2.0 ** -15))
        if K >= 8:
            assert (b == 0).sum() >= 2 and np.signbit(b[b == 0]).any() and not np.signbit(b[b == 0]).all() and np.unique(b).size < K
        if K >= 64 and dtype == "float32":
            # the planted elements straddle a decision: under the first candidate of the witness row the oracle's index changes
            # between neighbours that are one ulp apart
            with np.errstate(all="ignore"):
                _, idx = oracle.forward(x[-1:], cc.scales_of(xm[-1], ratios, 10.0)[0][:1], ant[0][0], 10.0, False)
            order = np.argsort(x[-1], kind="stable")
            u = x[-1][order].view(np.int32).astype(np.int64)
            adjacent = np.abs(np.diff(u)) == 1
            assert (adjacent & (np.diff(idx[0][order]) != 0)).any(), (K, "no pair of adjacent floats on two sides of a decision")


def test_degenerate_rows_are_what_they_say():
    for dtype in ("float32", "bfloat16", "float16"):
        for K in (1, 8, 147, 1024):
            x, names = cc.degenerate_rows(dtype, K)
            assert np.array_equal(cc.ROUND[dtype](x.astype(np.float64)), x, equal_nan=True)
            by = dict(zip(names, x))
            assert not np.signbit(by["all +0"]).any() and np.signbit(by["all -0"]).all() and (by["mixed zeros"] == 0).all()
            assert (by["one non-zero element"] != 0).sum() == 1 and np.unique(by["constant"]).size == 1 and (by["all negative"] < 0).all()
            assert np.isnan(by["a NaN"]).sum() == 1 or K == 1
            assert np.isposinf(by["a +Inf"]).any() and np.isneginf(by["a -Inf"]).any()
            assert K < 3 or (np.isnan(by["NaN and Inf"]).any() and np.isinf(by["NaN and Inf"]).any())
            tiny = {"float32": 2.0 ** -126, "bfloat16": 2.0 ** -126, "float16": 2.0 ** -14}[dtype]
            assert (np.abs(by["denormals only"]) < tiny).all() and (by["denormals only"] != 0).any()
            assert np.abs(by["largest finite"]).max() == cc.DTYPE_MAX[dtype]
            assert np.isfinite(by["witness"]).all() and (K == 1 or np.unique(by["witness"]).size > 1)


def test_oracle_nan_pattern_and_rows_without_an_eligible_candidate(oracle):
    """Per rung: exact_sse is NaN exactly for the candidates whose scale is zero, NaN or Inf; search_mse returns best = 1e10 and
    alpha = x_max bit for bit exactly on the rungs said to have no eligible candidate, and x_max times a candidate elsewhere."""
    ant, _ = _books(oracle)
    ratios = cc.ratios_of(*ANT)
    rungs = cc.statistic_ladder(10.0, ratios)
    said = np.array([_no_eligible_said(r[0]) for r in rungs] + [False])
    assert 8 <= said.sum() <= len(rungs) - 6
    for K in (8, 72):
        x, xm = cc.ladder_rows(rungs, K, ratios, ant)
        for g, gmax in ant:
            ex = calib_check.exact_sse(oracle, x, xm, ratios, g, gmax, False, True)[0]
            for r in range(x.shape[0]):
                s = cc.scales_of(xm[r], ratios, gmax)[1]
                assert np.array_equal(np.isnan(ex[:, r]), ~np.isfinite(s) | (s == 0)), (K, r, rungs[r][0] if r < len(rungs) else "witness")
            with np.errstate(all="ignore"):
                best, alpha, trace = oracle.search_mse(x, xm, *ANT, g, gmax, False, True)
            none = best == np.float32(1e10)
            assert np.array_equal(none, said), (K, [rungs[i][0] for i in np.flatnonzero(none != said)])
            assert np.array_equal(alpha[none].view(np.uint32), xm[none].view(np.uint32)), "alpha is not x_max bit for bit"
            b2, a2 = cc.pick_rule(trace, xm, ratios)
            assert np.array_equal(b2.view(np.uint32), best.view(np.uint32)) and np.array_equal(a2.view(np.uint32), alpha.view(np.uint32))


def test_each_restated_mistake_changes_an_expected_value(oracle):
    """The case set: the ladder's rows (K = 8 and 72, two ANT books) under their given statistics, the degenerate rows under
    their abs-max and under a given statistic of 0.05, and -- for the type rule -- the per-book scores of those launches with
    one book passed twice, plus the planted score vectors."""
    ant, _ = _books(oracle)
    ratios = cc.ratios_of(*ANT)
    rungs = cc.statistic_ladder(10.0, ratios)
    launches = []
    for K in (8, 72):
        launches.append(cc.ladder_rows(rungs, K, ratios, ant))
        x, _ = cc.degenerate_rows("float32", K)
        launches.append((x, oracle.absmax(x, True)))
        launches.append((x, np.full(x.shape[0], 0.05, np.float32)))
    changed = dict.fromkeys(cc.MISTAKES, 0)
    rows = 0
    score_vectors = list(cc.PLANTED_SCORES)
    for x, xm in launches:
        per_book = []
        for g, gmax in ant:
            with np.errstate(all="ignore"):
                best, alpha, trace = oracle.search_mse(x, xm, *ANT, g, gmax, False, True)
            rows += x.shape[0]
            per_book.append(cc.type_score(best))
            for m in cc.MISTAKES[:4]:
                t = cc.flushed_trace(oracle, x, xm, *ANT, g, gmax, False) if m == cc.MISTAKES[0] else trace
                b2, a2 = cc.pick_rule(t, xm, ratios, None if m == cc.MISTAKES[0] else m)
                diff = (b2.view(np.uint32) != best.view(np.uint32)) | (a2.view(np.uint32) != alpha.view(np.uint32))
                changed[m] += int(diff.sum())
        score_vectors.append(np.float32([per_book[0], per_book[1], per_book[0]]))
        score_vectors.append(np.float32([per_book[1], per_book[0], per_book[1], per_book[0]]))
    for sv in score_vectors:
        want = cc.type_rule(sv)
        assert want == int(np.argsort(sv, kind="stable")[0]), sv               # the reference's np.argsort(mse)[0]
        for m in cc.MISTAKES[4:]:
            changed[m] += int(cc.type_rule(sv, m) != want)
    print("calibration edge cases: %d rows x books, %d score vectors" % (rows, len(score_vectors)))
    for m in cc.MISTAKES:
        print("MISTAKE | %s | changes %d cases" % (m, changed[m]))
        assert changed[m] > 0, m
