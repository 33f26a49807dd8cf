"""Calibration at its edges: the clip-search sums where the candidate scales leave the kernels' scale domain, the per-row pick,
the type pick and the install forward (antq_search_sse / _multi, antq_calibrate, antq_calibrate_batch, antq_calibrate_install).

  a. sums     the statistic ladder and the degenerate rows of calibration_cases.py through the direct kernels, the sorted search
              (forced, default, knob 21 both ways), the sweep, the 16-bit histogram search and the one-scale fp32 sorted form,
              against calib_check.exact_sse at the bars of tests/test_gpu_search_exact.py (its _hold rules; NAMED_ROWS below)
  b. picks    antq_calibrate (GIVEN / ABSMAX / 3SIGMA, per row and one scale) and antq_calibrate_batch against
              oracle.search_mse; alpha == x_max bit for bit where no candidate is eligible; the summation tree of score[t]
  c. types    the type rule with planted ties, NaN codebooks, 1 .. 8 types, empty ranges, long candidate lists, the ratio
              rounding; the one-scale kernel against the per-row kernels
  d. install  antq_calibrate_install with planted picks (clamped ones too), mixed plan kinds, fp32 decision edges and all 65 536
              16-bit patterns, the grid-stride loop, guard bands, refusals

The reference side of every assert is the CPU oracle, float64 arithmetic or a value the test planted -- never the HIP library,
except where two library calls are required to return the SAME bits (batch == single call, one scale == two identical rows,
install == antq_fakequant), and those are compared with the oracle as well.  The inputs are held to their conditions without a
GPU by test_calibration_cases_host.py.  Every test says in an assert which kernel it meant to run: by the witness row, whose bits
must differ from the direct kernels', or by the knob / shape rule restated from csrc/antq_search.hip.

A codebook made NaN through gmax = NaN scores 1e10 per row like every row without an eligible candidate (best starts at 1e10
and a NaN is never below it), in the oracle as in the kernels: a calibration cannot produce a NaN score, so the `NaN last`
clause of the type rule is pinned on the host side (calibration_cases.PLANTED_SCORES) and here only through what such a
codebook really scores."""
import functools

import numpy as np
import pytest

import calib_check
import calibration_cases as cc
import fakequant_cases as fc
import operator_cases as oc
import test_gpu_search_exact as se
from calib_check import exact_sse, exact_three_sigma

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bfloat16", "float16")
ANT = (75, 150, 1)
OLIVE = (75, 250, 2)
ANT_RATIOS = cc.ratios_of(*ANT)
OLIVE_RATIOS = cc.ratios_of(*OLIVE)
SIGMA_BAR = {"float32": 2.4e-6, "bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}      # tests/test_gpu_reductions_exact.py, one rounding step of the dtype


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _t(img, dtype_name, dev):
    """the float32 image on the device in its dtype (every value is representable: exact)"""
    return torch.from_numpy(np.ascontiguousarray(img, np.float32)).to(dev).to(getattr(torch, dtype_name))


def _f(v, dev):
    return torch.from_numpy(np.ascontiguousarray(np.atleast_1d(v), np.float32)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


def _ant_books(L, grids, types=("int", "pot", "flint", "float")):
    return se._ant(L, grids, types=types)


# =========================================================================================================== a. the sums
def _row_paths(K, epl, ovp, closed_forms=True):
    """[(family, path, knob 21, yardstick: 0 exact / 1 terms32, other than the direct kernels?)] that antq_search.hip takes for
    rows of K elements (sort_shape_ok / sweep_shape_ok restated): forced sorted search from 128 elements, the default rule
    from 128 (256 with the pair rule), the forced sweep from 256; whole vectors, whole pairs."""
    out = [("direct kernels", se.DIRECT, 1, 1, False)]
    if K % epl or (ovp and K % 2) or not closed_forms:
        return out
    if K >= 128:
        out += [("sorted rows", se.SORTED, 1, 0, True), ("sorted rows", se.SORTED, 0, 0, True)]
    if K >= (256 if ovp else 128):
        out.append(("sorted rows", se.SORTED_DEFAULT, 1, 0, True))
    if 256 <= K <= 65536:
        out.append(("sweep rows", se.SWEEP, 1, 0, True))
    return out


def _bar(family, olive):
    if family.startswith("direct"):
        return calib_check.DIRECT_RTOL_OLIVE if olive else calib_check.DIRECT_RTOL
    return calib_check.HIST_RTOL if family.startswith("histogram") else calib_check.EXACT_RTOL


# The degenerate rows on which the closed forms (sorted search, sweep) legitimately lose digits: the sum of squared errors is a
# small remainder of terms of the size of sum x^2, and a closed form in double resolves 2^-53 of THOSE --
#   one non-zero element: sum x^2 is that element's square, the sum its squared error (1e-6 of it and less where the element
#       sits next to a codebook value: the case of `every element 0.5` in tests/test_gpu_search_exact.py);
#   float16 only -- one element of 60000 or 65504 among 0.02-sized ones (sum x^2 = 4e9 against a sum of 0.4: 2^-53 x 1e10), and
#       denormals only (small multiples of 2^-24: every element ON a value for many candidates).
#   (bfloat16 / float32 hold 1e30 and 3.4e38 there: every other element quantises to zero -- nothing is left to cancel.  The
#    constant row needs no name at these lengths: worst 2.3e-14.)
# Named under _hold's cap (5 % of a launch's rows: these launches carry 86 further ordinary rows); the bar of each is 8 x the
# largest deviation measured against the yardstick on the MI355X over every launch below, the convention of
# EXACT_RTOL_FAR_STATISTIC (profiles/search_exactness.md: 9.41e-10 / 1.89e-10 / 5.82e-9; 2.06e-6, 2.02e-11, 1.45e-6; 1.01e-12).
NAMED_ROWS = {
    "float32": {"one non-zero element": 7.6e-9},
    "bfloat16": {"one non-zero element": 1.6e-9},
    "float16": {"one non-zero element": 4.7e-8, "one huge element": 1.7e-5, "denormals only": 1.7e-10, "largest finite": 1.2e-5},
}
NAMED_ONE_SCALE_FP32 = {"one non-zero element": 8.1e-12}       # k_search_sorted<.., PT> on 4096 elements: worst 1.01e-12
DEG_PAD = 86


def _held(errors, family, case, dtype_name, got, want, bar, row_names=None, loose=None):
    """se._hold, every miss collected (a case goes on to its other paths and rows; the test fails at its end with all of them);
    a NaN / Inf pattern that differs is located first"""
    for what, f in (("NaN", np.isnan), ("Inf", np.isinf)):
        diff = np.argwhere(f(got) != f(want))
        if diff.size:
            t, c, r = diff[0]
            rows = sorted(set(int(v) for v in diff[:, 2]))
            errors.append("%s | %s | %s: %s pattern differs in %d cells, rows %s%s; first: type %d cand %d row %d got %r yardstick %r" % (
                family, case, dtype_name, what, len(diff), rows[:8], "" if row_names is None else " " + str([row_names[v] for v in rows[:8]]),
                t, c, r, got[t, c, r], want[t, c, r]))
            return
    try:
        se._hold(family, case, dtype_name, got, want, bar, loose=loose)
    except AssertionError as e:
        errors.append("%s%s" % (str(e)[:700], "" if row_names is None else " | rows: " + str(list(enumerate(row_names)))[:400]))


def _hold_rows(errors, L, oracle, dev, dtype_name, tag, img, xm, ratios, cbs, plans, gm, ovp, olive, witness, row_names, closed_forms=True, named=None):
    """One per-row launch per path of _row_paths: every cell against the yardstick; where a path other than the direct kernels
    was meant, the witness row's bits differ from the direct kernels'.  named: {row: bar} for the closed forms only."""
    rows, K = img.shape
    x, xmt, rt = _t(img, dtype_name, dev), _f(xm, dev), se._rt(ratios, dev)
    yard = np.stack([np.stack(exact_sse(oracle, img, xm, ratios, g, m, ovp, True)) for g, m in cbs])          # [ntypes, 2, ncand, rows]
    direct = None
    for family, path, k21, which, other in _row_paths(K, cc.EPL[dtype_name], ovp, closed_forms):
        got = se._search(L, path, x, rows, K, xmt, True, rt, plans, gm, ovp, k21=k21)
        if not other:
            direct = got
        else:
            assert not np.array_equal(got[:, :, witness], direct[:, :, witness]), \
                "%s (knobs 19/20 = %s, 21 = %d) did not run on %s: the witness row has the direct kernels' bits" % (family, path, k21, tag)
        name = "%s, %s" % (family, "OliVe pairs" if ovp else "OliVe no pairs" if olive else "ANT")
        _held(errors, name, "%s knobs %s/%d" % (tag, path, k21), dtype_name, got, yard[:, which], _bar(family, olive), row_names, named if other else None)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_sums_of_rows_at_the_scale_edges(dev, oracle, dtype_name):
    """The ladder (given statistics) as per-row launches of every row length of cc.ROW_LENS: element kernel (8, 147), short
    direct (72), short sorted form (128 * EPL, 1024), two-chunk rows with the pair rule (1152, 4160) -- through every path the
    length has, no row named.  The degenerate rows (their own abs-max and exact 3-sigma statistic, computed on the host): through
    the direct kernels at every length; through the closed forms at 128 * EPL (short form, and the 4096-key kernel with knob
    21 = 0; the sweep) and 1152 (the 4096-key kernel by default), in launches of 100 rows so that NAMED_ROWS fit under the cap."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids)
    ocb, oplans, ogm = se._olive(L, grids)
    rungs_a = cc.statistic_ladder(10.0, ANT_RATIOS)
    rungs_o = cc.statistic_ladder(ocb[0][1], OLIVE_RATIOS)
    errors = []
    lad_a, lad_o = [r[0] for r in rungs_a] + ["witness"], [r[0] for r in rungs_o] + ["witness"]
    two = [0, 2]                                                        # int and flint: the degenerate launches' ANT books
    for K in cc.ROW_LENS[dtype_name]:
        img, xm = cc.ladder_rows(rungs_a, K, ANT_RATIOS, acb[:2], dtype_name)
        _hold_rows(errors, L, oracle, dev, dtype_name, "ladder %dx%d" % img.shape, img, xm, ANT_RATIOS, acb, aplans, agm, False, False, img.shape[0] - 1, lad_a)
        closed = K in (128 * cc.EPL[dtype_name], 576 * 2)
        deg, names = cc.degenerate_rows(dtype_name, K, DEG_PAD if closed else 0)
        named = {names.index(k): v for k, v in NAMED_ROWS[dtype_name].items()} if closed else None
        w = names.index("witness")
        with np.errstate(all="ignore"):
            _hold_rows(errors, L, oracle, dev, dtype_name, "degenerate, abs-max %dx%d" % deg.shape, deg, oracle.absmax(deg, True), ANT_RATIOS,
                       [acb[i] for i in two], [aplans[i] for i in two], [agm[i] for i in two], False, False, w, names, closed, named)
        if K % 2 == 0:
            img, xm = cc.ladder_rows(rungs_o, K, OLIVE_RATIOS, ocb, dtype_name)
            with np.errstate(all="ignore"):
                sig = exact_three_sigma(deg, True, dtype_name)
            for ovp in (True, False):
                _hold_rows(errors, L, oracle, dev, dtype_name, "ladder %dx%d" % img.shape, img, xm, OLIVE_RATIOS, ocb, oplans, ogm, ovp, True, img.shape[0] - 1, lad_o)
                _hold_rows(errors, L, oracle, dev, dtype_name, "degenerate, 3-sigma %dx%d" % deg.shape, deg, sig, OLIVE_RATIOS, ocb, oplans, ogm, ovp, True, w, names,
                           closed, named)
    assert not errors, "%d misses:\n%s" % (len(errors), "\n".join(errors))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_sums_of_one_scale_tensors_at_the_scale_edges(dev, oracle, dtype_name):
    """Every rung and every degenerate row as a tensor of its own with ONE scale, the smallest the forced paths accept: fp32
    4096 elements through k_search_sorted<.., PT> (knob 20 = 2), bf16 / f16 1024 elements through the histogram search (knob
    14 = 2; hist_eligible: whole 16-byte vectors, an aligned tensor), both also through the direct kernels.  The witness tensor
    is the proof that the other path ran.  The 35 tensors of a codebook family are held together, one `row` each; the fp32
    tensor with one non-zero element is named for the sorted form (NAMED_ONE_SCALE_FP32)."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids)
    ocb, oplans, ogm = se._olive(L, grids)
    n = cc.ONE_SCALE_N[dtype_name]
    assert n % 8 == 0 and (dtype_name != "float32" or n >= 4096)
    fp32 = dtype_name == "float32"
    family = "sorted one scale" if fp32 else "histogram one scale"
    errors = []
    for label, ratios, cbs, plans, gm, ovps in (("ANT", ANT_RATIOS, acb, aplans, agm, (False,)), ("OliVe", OLIVE_RATIOS, ocb, oplans, ogm, (True, False))):
        rungs = cc.statistic_ladder(cbs[0][1], ratios)
        img, xm = cc.ladder_rows(rungs, n, ratios, cbs[:2], dtype_name)
        deg, names = cc.degenerate_rows(dtype_name, n)
        row_names = [r[0] for r in rungs] + ["witness"] + list(names)
        with np.errstate(all="ignore"):
            stat = np.stack([oracle.absmax(deg[r:r + 1], False) if label == "ANT" else exact_three_sigma(deg[r:r + 1], False, dtype_name) for r in range(len(names))]).reshape(-1)
        img, xm = np.concatenate([img, deg]), np.concatenate([xm, stat])
        rt = se._rt(ratios, dev)
        named = {row_names.index(k): v for k, v in NAMED_ONE_SCALE_FP32.items()} if fp32 else None
        for ovp in ovps:
            ds, os_, exs = [], [], []
            for r in range(img.shape[0]):
                x, xmt = _t(img[r], dtype_name, dev), _f(xm[r], dev)
                assert x.data_ptr() % 16 == 0
                exs.append(np.stack([np.stack(exact_sse(oracle, img[r:r + 1], xm[r:r + 1], ratios, g, m, ovp, False)) for g, m in cbs]))
                ds.append(se._search(L, se.DIRECT, x, 1, n, xmt, False, rt, plans, gm, ovp, k14=0))
                os_.append(se._search(L, se.SORTED if fp32 else se.DIRECT, x, 1, n, xmt, False, rt, plans, gm, ovp, k14=2))
                if row_names[r] == "witness":                                            # the two witnesses: ordinary tensors
                    assert not np.array_equal(os_[-1], ds[-1]), "%s did not run on the witness tensor %d of %s" % (family, r, label)
            d, o, ex = np.concatenate(ds, axis=2), np.concatenate(os_, axis=2), np.concatenate(exs, axis=3)
            kind = "%s, %s" % (label, "pairs" if ovp else "no pairs") if label == "OliVe" else label
            tag = "%s, %d tensors of %d" % (label, img.shape[0], n)
            _held(errors, "direct kernels one scale, " + kind, tag, dtype_name, d, ex[:, 1], _bar("direct", label == "OliVe"), row_names)
            _held(errors, family + ", " + kind, tag, dtype_name, o, ex[:, 0 if fp32 else 1], _bar(family, label == "OliVe"), row_names, named)
            print("%s, %s, pairs %s: %d of %d tensors with other bits than the direct kernels'" % (
                family, label, ovp, sum(int(not np.array_equal(a, b)) for a, b in zip(os_, ds)), img.shape[0]))
    assert not errors, "%d misses:\n%s" % (len(errors), "\n".join(errors))


# =========================================================================================================== b. the picks
SCORE_MISSES = []            # (key, type, got, want, ulps) of _check_picks: asserted empty at the end of every test that calls it


def _no_score_misses():
    misses, SCORE_MISSES[:] = list(SCORE_MISSES), []
    assert not misses, ("score[t] further than 1 float ulp from fl32(fsum(oracle best))", len(misses), misses[:12])


def _expect(oracle, img, xm, cbs, rng3, ovp, per_row):
    """[(best, alpha, trace)] per codebook from oracle.search_mse"""
    x2 = img if per_row else img.reshape(1, -1)
    with np.errstate(all="ignore"):
        return [oracle.search_mse(x2, xm, rng3[0], rng3[1], rng3[2], g, m, ovp, per_row) for g, m in cbs]


def _check_picks(key, alpha, score, xm_got, xm_want, expect, rng3, xmax_rtol=0.0):
    """alpha [ntypes, na] / score [ntypes] of one calibration against the oracle's search on the statistic xm_want.
    Rows without an eligible candidate (the oracle's best is 1e10): alpha == x_max bit for bit.  Every other row: alpha is, bit
    for bit, x_max times a candidate whose ORACLE score ties the oracle's best within NEAR_TIE_RTOL (calib_check.
    check_alpha_picks where the statistic is a normal number, its rule restated on the bits everywhere).  score[t] within one
    float ulp of fl32(fsum(best))."""
    ratios = cc.ratios_of(*rng3)
    alpha, score = alpha.cpu().numpy(), score.cpu().numpy()
    xm_got = xm_got.cpu().numpy()
    if xmax_rtol == 0.0:
        assert _same32(xm_got, xm_want).all(), (key, "x_max", xm_got[~_same32(xm_got, xm_want)][:4], xm_want[~_same32(xm_got, xm_want)][:4])
    for t, (best, ref_alpha, trace) in enumerate(expect):
        none = best == np.float32(1e10)
        assert _same32(alpha[t][none], xm_got[none]).all(), (key, t, "alpha is not x_max bit for bit on rows without an eligible candidate",
                                                             np.flatnonzero(none)[~_same32(alpha[t][none], xm_got[none])][:6])
        for r in np.flatnonzero(~none):
            with np.errstate(all="ignore"):
                cand = (np.float32(xm_got[r]) * ratios).astype(np.float32)
            hit = np.flatnonzero(_bits(cand) == _bits(alpha[t, r:r + 1])[0])
            assert hit.size, (key, t, r, "alpha is not fl32(x_max * ratio) of any candidate", alpha[t, r], xm_got[r])
            gap = (np.float64(trace[hit, r].min()) - np.float64(best[r])) / np.float64(best[r]) if best[r] > 0 else np.float64(trace[hit, r].min())
            assert gap <= calib_check.NEAR_TIE_RTOL, (key, t, r, "picked candidate %s, oracle best %.9g, gap %.3g" % (hit.tolist(), best[r], gap))
        ordinary = ~none & np.isfinite(xm_want) & (np.abs(xm_want) >= 2.0 ** -100)
        if ordinary.any():
            calib_check.check_alpha_picks("%s type %d" % (key, t), alpha[t][ordinary], ref_alpha[ordinary], trace[:, ordinary], ratios, xmax_rtol=xmax_rtol)
        want = cc.type_score(best)
        ulps = abs(float(score[t]) - float(want)) / float(np.spacing(np.abs(want)))
        print("SCORE | %s | type %d | rows %d | got %.9g | fl32(fsum(best)) %.9g | %.2f ulp" % (key, t, best.size, score[t], want, ulps), flush=True)
        if not ulps <= 1.0:
            SCORE_MISSES.append((key, t, float(score[t]), float(want), ulps))
    return np.float32([cc.type_score(e[0]) for e in expect])


def _check_type(key, typ, want_scores, same_plan=None):
    """the first smallest oracle score; another type only where the oracle's two scores tie within NEAR_TIE_RTOL and the two
    are different codebooks (identical plans have identical bits: there the first must win)"""
    want = cc.type_rule(want_scores)
    if typ != want:
        gap = abs(float(want_scores[typ]) - float(want_scores[want])) / float(want_scores[want])
        assert (same_plan is None or same_plan[typ] != same_plan[want]) and gap <= calib_check.NEAR_TIE_RTOL, (key, "type", typ, "oracle", want, want_scores)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_picks_under_given_statistics(dev, oracle, dtype_name):
    """antq_calibrate(ANTQ_XMAX_GIVEN) over the ladder, per row (every row length) and as one-scale tensors (the forced paths'
    smallest size); antq_calibrate_batch over the same jobs returns the same bits.
    (One-scale tensors of 8 elements are not in this set.  With one row, score[t] IS the row's mean squared error, and the
    direct kernels add a lane's float32 terms in float32 where the oracle adds them in double: measured on the MI355X, the
    8-element tensor of the rung `straddling 2^-40, first 37 outside` scored 2.11619703e-26 against the oracle's
    2.11619734e-26, 2 float ulps and inside DIRECT_RTOL, which is what holds such sums in section a.  The one-ulp bound on
    score[t] concerns the summation over rows; rows of 8 elements stay in the per-row launches of 21 rows, which meet it.)"""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids, ("int", "pot", "flint"))
    ocb, oplans, ogm = se._olive(L, grids)
    rungs = cc.statistic_ladder(10.0, ANT_RATIOS)
    jobs, stats, singles, keys, expects = [], [], [], [], []
    for K in cc.ROW_LENS[dtype_name]:
        img, xm = cc.ladder_rows(rungs, K, ANT_RATIOS, acb[:2], dtype_name)
        jobs.append((_t(img, dtype_name, dev), img.shape[0], K, True, aplans, agm) + ANT)
        stats.append(_f(xm, dev))
        # which sums antq_calibrate's default rule forms for this length (antq_calibrate and antq_search_sse_multi share the
        # dispatch): the sorted search from 128 elements in whole vectors -- the witness row's bits differ from the direct
        # kernels' -- and the direct kernels below
        w = img.shape[0] - 1
        d = se._search(L, se.DIRECT, jobs[-1][0], img.shape[0], K, stats[-1], True, se._rt(ANT_RATIOS, dev), aplans, agm, False)
        s = se._search(L, se.SORTED_DEFAULT, jobs[-1][0], img.shape[0], K, stats[-1], True, se._rt(ANT_RATIOS, dev), aplans, agm, False)
        assert (not np.array_equal(s[:, :, w], d[:, :, w])) == (K % cc.EPL[dtype_name] == 0 and K >= 128), \
            "rows of %d: the default rule was meant to take the %s" % (K, "sorted search" if K >= 128 and K % cc.EPL[dtype_name] == 0 else "direct kernels")
        keys.append("given, rows %dx%d %s" % (img.shape + (dtype_name,)))
        expects.append((_expect(oracle, img, xm, acb, ANT, False, True), xm))
    for n in (cc.ONE_SCALE_N[dtype_name],):
        img, xm = cc.ladder_rows(rungs, n, ANT_RATIOS, acb[:2], dtype_name)
        for r in range(img.shape[0]):
            jobs.append((_t(img[r], dtype_name, dev), 1, n, False, aplans, agm) + ANT)
            stats.append(_f(xm[r], dev))
            keys.append("given, one scale, rung %d of %d %s" % (r, n, dtype_name))
            expects.append((_expect(oracle, img[r:r + 1], xm[r:r + 1], acb, ANT, False, False), xm[r:r + 1]))
    for job, st, key, (exp, xm) in zip(jobs, stats, keys, expects):
        alpha, score, typ, xo = L.calibrate(*job, xmax=st.clone())
        ws = _check_picks(key, alpha, score, xo, xm, exp, ANT)
        _check_type(key, int(typ.item()), ws)
        singles.append((alpha.cpu().numpy(), score.cpu().numpy(), int(typ.item())))
    results, types = L.calibrate_batch(jobs, xmax=stats)
    types = types.cpu().numpy()
    for i, ((alpha, score, xo), key, (exp, xm)) in enumerate(zip(results, keys, expects)):
        ws = _check_picks("batch: " + key, alpha, score, xo, xm, exp, ANT)
        _check_type("batch: " + key, int(types[i]), ws)
        a1, s1, t1 = singles[i]
        assert np.array_equal(_bits(alpha.cpu().numpy()), _bits(a1)) and np.array_equal(_bits(score.cpu().numpy()), _bits(s1)) and int(types[i]) == t1, \
            (key, "antq_calibrate_batch and antq_calibrate disagree")
    # OliVe's books with the pair rule under their own ladder
    rungs_o = cc.statistic_ladder(ocb[0][1], OLIVE_RATIOS)
    for K in (72, 576 * 2):
        img, xm = cc.ladder_rows(rungs_o, K, OLIVE_RATIOS, ocb, dtype_name)
        for ovp in (True, False):
            alpha, score, typ, xo = L.calibrate(_t(img, dtype_name, dev), img.shape[0], K, True, oplans, ogm, *OLIVE, xmax=_f(xm, dev), ovp=ovp)
            key = "given, OliVe pairs %s, rows %dx%d %s" % ((ovp,) + img.shape + (dtype_name,))
            _check_type(key, int(typ.item()), _check_picks(key, alpha, score, xo, xm, _expect(oracle, img, xm, ocb, OLIVE, ovp, True), OLIVE))
    _no_score_misses()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_picks_under_the_rows_own_statistics(dev, oracle, dtype_name):
    """antq_calibrate(ANTQ_XMAX_ABSMAX / _3SIGMA) over the degenerate rows, per row and as one-scale tensors, and over rows of ONE
    element (the unbiased std is NaN); the statistic itself against oracle.absmax (bit for bit) and calib_check.
    exact_three_sigma (its documented bar); antq_calibrate_batch returns the same bits."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids, ("int", "flint"))
    ocb, oplans, ogm = se._olive(L, grids)
    for mode, cbs, plans, gm, rng3, ovp in (("absmax", acb, aplans, agm, ANT, False), ("3sigma", ocb, oplans, ogm, OLIVE, True)):
        jobs, keys, wants = [], [], []
        shapes = [(K, True) for K in (8, 72, 128 * cc.EPL[dtype_name], 576 * 2)] + [(8, False), (cc.ONE_SCALE_N[dtype_name], False)]
        for K, per_row in shapes:
            deg, names = cc.degenerate_rows(dtype_name, K)
            for img in ([deg] if per_row else [deg[r:r + 1] for r in range(len(names))]):
                jobs.append((_t(img, dtype_name, dev), img.shape[0] if per_row else 1, K, per_row, plans, gm) + rng3)
                keys.append("%s, %s %dx%d %s" % ((mode, "rows" if per_row else "one scale") + img.shape + (dtype_name,)))
                wants.append((img, per_row))
        one = cc.ROUND[dtype_name](np.float64([[0.75], [-0.0], [np.nan], [3e-5], [-2.0]]))
        jobs.append((_t(one, dtype_name, dev), 5, 1, True, plans, gm) + rng3)
        keys.append("%s, rows of one element %s" % (mode, dtype_name))
        wants.append((one, True))
        singles = []

        def check(key, alpha, score, typ, xo, img, per_row):
            with np.errstate(all="ignore"):
                xm = oracle.absmax(img, per_row) if mode == "absmax" else exact_three_sigma(img, per_row, dtype_name)
            got = xo.cpu().numpy()
            if mode == "3sigma":
                fin = np.isfinite(xm)
                assert np.array_equal(np.isnan(got), np.isnan(xm)) and np.array_equal(np.isinf(got), np.isinf(xm)), (key, "3-sigma statistic", got, xm)
                assert np.all(np.abs(got[fin].astype(np.float64) - xm[fin]) <= SIGMA_BAR[dtype_name] * np.abs(xm[fin])), (key, "3-sigma statistic", got, xm)
            exp = _expect(oracle, img, xm, cbs, rng3, ovp, per_row)
            _check_type(key, typ, _check_picks(key, alpha, score, xo, xm, exp, rng3, xmax_rtol=0.0 if mode == "absmax" else 2e-6))

        for job, key, (img, per_row) in zip(jobs, keys, wants):
            alpha, score, typ, xo = L.calibrate(*job, xmax=mode, ovp=ovp)
            check(key, alpha, score, int(typ.item()), xo, img, per_row)
            singles.append((alpha.cpu().numpy(), score.cpu().numpy(), int(typ.item()), xo.cpu().numpy()))
        results, types = L.calibrate_batch(jobs, xmax=mode, ovp=ovp)
        types = types.cpu().numpy()
        for i, ((alpha, score, xo), key, (img, per_row)) in enumerate(zip(results, keys, wants)):
            check("batch: " + key, alpha, score, int(types[i]), xo, img, per_row)
            a1, s1, t1, x1 = singles[i]
            assert np.array_equal(_bits(alpha.cpu().numpy()), _bits(a1)) and np.array_equal(_bits(score.cpu().numpy()), _bits(s1)) and \
                int(types[i]) == t1 and np.array_equal(_bits(xo.cpu().numpy()), _bits(x1)), (key, "antq_calibrate_batch and antq_calibrate disagree")
    _no_score_misses()


def test_score_summation_tree(dev, oracle):
    """score[t] = the float of the sum over rows of the best MSE, for 1, 255, 256, 257 and 1000 rows (k_calib_type_score_pick:
    thread-strided partials, then a tree over 256 threads): rows drawn in turn from the ladder, once all of them (the 1e10 of
    the rows without a candidate dominates) and once only rows with a pick."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids, ("int", "flint"))
    rungs = cc.statistic_ladder(10.0, ANT_RATIOS)
    img, xm = cc.ladder_rows(rungs, 8, ANT_RATIOS, acb)
    best = _expect(oracle, img, xm, acb[:1], ANT, False, True)[0][0]
    eligible = np.flatnonzero(best != np.float32(1e10))
    assert 6 <= eligible.size < img.shape[0]
    for na in (1, 255, 256, 257, 1000):
        for label, pool in (("all rows", np.arange(img.shape[0])), ("rows with a pick", eligible)):
            sel = pool[(np.arange(na) * 7 + 3) % pool.size]
            # every row gets a scale of its own (powers of two: the picks stay, the scores differ from row to row)
            f = np.float32(2.0) ** ((np.arange(na) % 5) - 2)
            with np.errstate(all="ignore"):
                xi, xmi = (img[sel] * f[:, None]).astype(np.float32), (xm[sel] * f).astype(np.float32)
            alpha, score, typ, xo = L.calibrate(_t(xi, "float32", dev), na, 8, True, aplans, agm, *ANT, xmax=_f(xmi, dev))
            key = "summation tree, %d rows, %s" % (na, label)
            _check_type(key, int(typ.item()), _check_picks(key, alpha, score, xo, xmi, _expect(oracle, xi, xmi, acb, ANT, False, True), ANT))
    _no_score_misses()


# =========================================================================================================== c. the type rule
TYPE_LISTS = ([0], [1, 1], [0, 1], [1, 0], [0, 0, 0], [2, 0, 0], [0, 2, 0], [0, 0, 2], [0, 1, 2, 3], [3, 2, 1, 0], [0, 1, 2, 3, 0], [1, 1, 1, 1, 2],
              [3, 3, 0, 3, 3, 0], [1, 2, 3, 1, 2, 3, 0], [3, 3, 3, 3, 2, 2, 2, 2], [1, 0, 1, 0, 1, 0, 1, 0], [3, 2, 1, 3, 2, 1, 3, 0])
NAN_LISTS = (([0, 1, 2], (0,)), ([0, 1, 2], (1,)), ([0, 1, 2], (2,)), ([0, 1, 2], (0, 1, 2)), ([0], (0,)), ([0, 1, 2, 3, 2], (4,)), ([2, 1, 2, 3, 0, 1], (0, 4)),
             ([0, 1, 2, 3, 0, 1, 2, 3], tuple(range(8))))


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_type_rule_with_planted_ties_and_nan_codebooks(dev, oracle, dtype_name):
    """1 .. 8 types (batches of kMaxTypes = 4 in the searches, four types per wavefront pass in the one-scale kernel): the same
    plan two, three and four times -- its scores are bit-identical, so the first must win -- with a better or worse book
    before, between and behind; codebooks made NaN through gmax = NaN first, in the middle, last and all of them (every
    type then scores rows x 1e10 and type 0 wins).  Per row (k_search_pick + k_calib_type_score_pick: 3 rows of 8, 5 rows of
    128 * EPL) and one scale (k_calib_pick_one_scale: 8 elements and the forced paths' smallest size)."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids)
    epl = cc.EPL[dtype_name]
    rng = np.random.default_rng(77)
    for rows, K, per_row in ((3, 8, True), (5, 128 * epl, True), (1, 8, False), (1, cc.ONE_SCALE_N[dtype_name], False)):
        img = cc.ROUND[dtype_name](np.clip(rng.standard_normal((rows, K)), -4, 4) * 0.03)
        with np.errstate(all="ignore"):
            xm = oracle.absmax(img, per_row)
        exp = _expect(oracle, img, xm, acb, ANT, False, per_row)
        with np.errstate(all="ignore"):
            exp_nan = _expect(oracle, img, xm, [(acb[0][0], float("nan"))], ANT, False, per_row)[0]
        assert (exp_nan[0] == np.float32(1e10)).all() and np.isnan(exp_nan[2]).all(), "the oracle scores a NaN codebook 1e10 per row"
        x = _t(img, dtype_name, dev)
        assert per_row == (rows > 1), "na == 1 sends antq_calibrate to k_calib_pick_one_scale, na > 1 to k_search_pick + k_calib_type_score_pick"
        cases = [(ids, ()) for ids in TYPE_LISTS] + list(NAN_LISTS)
        won = set()
        for ids, nans in cases:
            plans = [aplans[i] for i in ids]
            gm = [float("nan") if p in nans else agm[i] for p, i in enumerate(ids)]
            e = [exp_nan if p in nans else exp[i] for p, i in enumerate(ids)]
            alpha, score, typ, xo = L.calibrate(x, rows, K, per_row, plans, gm, *ANT, xmax="absmax")
            key = "types %s NaN %s, %s %dx%d %s" % (ids, list(nans), "rows" if per_row else "one scale", rows, K, dtype_name)
            ws = _check_picks(key, alpha, score, xo, xm, e, ANT)
            same = [-1 - p if p in nans else i for p, i in enumerate(ids)]
            _check_type(key, int(typ.item()), ws, same_plan=same)
            sc = _bits(score.cpu().numpy())
            for p in range(len(ids)):
                for q in range(p):
                    if same[p] == same[q]:
                        assert sc[p] == sc[q], (key, "the same plan scored differently at positions %d and %d" % (q, p))
            if len(nans) == len(ids):
                assert int(typ.item()) == 0 and (ws == cc.type_score(np.full(exp[0][0].size, 1e10, np.float32))).all(), (key, "all types NaN: type 0")
            won.add(int(typ.item()))
        assert len(won) >= 3, ("the winner sat at fewer than three different positions", won)
    _no_score_misses()


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_one_scale_kernel_agrees_with_the_per_row_kernels(dev, oracle, dtype_name):
    """A tensor with one scale through k_calib_pick_one_scale and the same data as two identical rows through k_search_pick +
    k_calib_type_score_pick: each against the oracle; for ONE vector (every kernel adds its four / eight terms in the same
    order) the per-row values and the pick are also equal bit for bit."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids)
    rng = np.random.default_rng(78)
    for n in (cc.EPL[dtype_name], 72, 1024):
        for ids in ([0, 1, 2, 3], [2, 2, 1], [3, 0, 3, 0, 1, 1, 2]):
            img = cc.ROUND[dtype_name](np.clip(rng.standard_normal((1, n)), -4, 4) * 0.05)
            two = np.concatenate([img, img])
            plans, gm, cbs = [aplans[i] for i in ids], [agm[i] for i in ids], [acb[i] for i in ids]
            xm1, xm2 = oracle.absmax(img, False), oracle.absmax(two, True)
            a1, s1, t1, x1 = L.calibrate(_t(img, dtype_name, dev), 1, n, False, plans, gm, *ANT, xmax="absmax")
            a2, s2, t2, x2 = L.calibrate(_t(two, dtype_name, dev), 2, n, True, plans, gm, *ANT, xmax="absmax")
            key = "one scale vs two rows, n %d types %s %s" % (n, ids, dtype_name)
            w1 = _check_picks(key + " (one scale)", a1, s1, x1, xm1, _expect(oracle, img, xm1, cbs, ANT, False, False), ANT)
            w2 = _check_picks(key + " (two rows)", a2, s2, x2, xm2, _expect(oracle, two, xm2, cbs, ANT, False, True), ANT)
            _check_type(key, int(t1.item()), w1, same_plan=ids)
            _check_type(key, int(t2.item()), w2, same_plan=ids)
            if n == cc.EPL[dtype_name]:
                a1, a2, s1, s2 = a1.cpu().numpy(), a2.cpu().numpy(), s1.cpu().numpy(), s2.cpu().numpy()
                assert np.array_equal(_bits(a2[:, 0]), _bits(a1[:, 0])) and np.array_equal(_bits(a2[:, 1]), _bits(a1[:, 0])), (key, "alpha")
                assert np.array_equal(_bits(s2), _bits((s1.astype(np.float64) * 2).astype(np.float32))), (key, "score of two equal rows")
                assert int(t1.item()) == int(t2.item()), (key, "type")
    _no_score_misses()


def test_empty_ranges_long_candidate_lists_and_the_ratio_rounding(dev, oracle):
    """lb >= ub (k_calib_none: best = 1e10, alpha = x_max, type 0) for one scale and for rows; candidate lists of 1, 64, 65 and
    280 (a lane of the pick kernels walks c, c + 64, ...); and the ratio of every single-candidate range [i, i + 1), i = 1 ..
    300: alpha == fl32(x_max * fl32(i * 0.01)), i * 0.01 formed in double as Python does."""
    from ant_quantization_amd import _lib as L, grids
    acb, aplans, agm = _ant_books(L, grids, ("int", "flint", "pot"))
    rng = np.random.default_rng(79)
    img = (np.clip(rng.standard_normal((6, 72)), -4, 4) * 0.04).astype(np.float32)
    for rows, per_row in ((6, True), (1, False)):
        x2 = img if per_row else img[:1]
        xm = oracle.absmax(x2, per_row)
        for rng3 in ((100, 100, 1), (120, 75, 1), (100, 101, 1), (75, 139, 1), (75, 140, 1), (20, 300, 1), (75, 250, 2)):
            alpha, score, typ, xo = L.calibrate(_t(x2, "float32", dev), rows, 72, per_row, aplans, agm, *rng3, xmax="absmax")
            key = "range %s, %s" % (rng3, "rows" if per_row else "one scale")
            exp = _expect(oracle, x2, xm, acb, rng3, False, per_row)
            assert exp[0][2].shape[0] == len(range(*rng3))
            ws = _check_picks(key, alpha, score, xo, xm, exp, rng3)
            _check_type(key, int(typ.item()), ws)
            if rng3[0] >= rng3[1]:
                assert int(typ.item()) == 0 and (ws == cc.type_score(np.full(xm.size, 1e10, np.float32))).all(), key
                assert np.array_equal(_bits(alpha.cpu().numpy()), _bits(np.tile(xm, (3, 1)))), (key, "alpha == x_max")
    tiny = np.float32([[0.3, -0.7, 0.11, 0.05]])
    xm = oracle.absmax(tiny, False)
    x = _t(tiny, "float32", dev)
    results, types = L.calibrate_batch([(x, 1, 4, False, aplans[:1], agm[:1], i, i + 1, 1) for i in range(1, 301)], xmax="absmax")
    for i, (alpha, score, xo) in zip(range(1, 301), results):
        want = np.float32(xm[0] * np.float32(i * 0.01))
        got = alpha.cpu().numpy().reshape(-1)
        assert got.size == 1 and _bits(got)[0] == _bits(want)[0], ("ratio %d" % i, got, want)
        best = _expect(oracle, tiny, xm, acb[:1], (i, i + 1, 1), False, False)[0][0]
        assert best[0] < 1e10 and abs(float(score.cpu().numpy()[0]) - float(best[0])) <= float(np.spacing(best[0])), ("ratio %d" % i, score, best)
    assert (types.cpu().numpy() == 0).all()
    _no_score_misses()


# =========================================================================================================== d. the install forward
class Carved:
    """n elements between two guard bands of oc.GUARD (+ lead) poisoned elements"""

    def __init__(self, n, dtype_name, dev, lead=0):
        raw, self.poison = ("int32", oc.POISON32) if dtype_name == "float32" else ("int16", oc.POISON16)
        self.lo, self.n = oc.GUARD + lead, n
        self.buf = torch.full((self.lo + n + oc.GUARD,), self.poison, dtype=getattr(torch, raw), device=dev)
        assert self.buf.data_ptr() % 16 == 0 and (oc.GUARD * self.buf.element_size()) % 16 == 0
        self.view = self.buf[self.lo:self.lo + n].view(getattr(torch, dtype_name))

    def bits(self, tag):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == self.poison).all() and (b[self.lo + self.n:] == self.poison).all(), (tag, "guard elements changed")
        v = b[self.lo:self.lo + self.n]
        return v.view(np.uint16 if v.itemsize == 2 else np.uint32)

    def untouched(self, tag):
        assert (self.buf == self.poison).all().item(), (tag, "a refused call wrote")


@functools.lru_cache(maxsize=None)
def _install_books():
    """name -> (name, grid, gmax, n_normal, pair rule): a 4-bit table plan, a second one, int-8 (a big table), a scan plan, an
    OliVe book"""
    return {n: (oc.f64_book(n) if n == "scan_list" else fc.book(n)) for n in ("flint_b4_s", "int_b4_s", "int_b8_s", "scan_list", "olive_flint")}


INSTALL_LISTS = (("flint_b4_s",), ("int_b4_s", "flint_b4_s"), ("flint_b4_s", "int_b8_s", "scan_list"), ("int_b8_s", "flint_b4_s", "scan_list", "olive_flint"),
                 ("olive_flint", "scan_list", "int_b4_s", "int_b8_s"))


def _install(L, dev, dtype_name, tag, x_bits_src, names, t_planted, ovp, alphas, want_of, grid_len, optional=True, fq=None):
    """One antq_calibrate_install with *type_dev = t_planted: out, alpha_out, mse_out, grid_out, outl_out between guard bands
    == the picked (clamped) entries and want_of(t) (the oracle's output bits); x unchanged.  optional=False: mse_out, outl
    and outl_out NULL."""
    books = [_install_books()[n] for n in names]
    nt = len(books)
    t = min(max(t_planted, 0), nt - 1)                                  # the kernels clamp the pick (include/antq.h)
    plans = [L.plan_for(b[1]) for b in books]
    gmaxs = [b[2] for b in books]
    stack = np.zeros((nt, grid_len), np.float32)
    for i, b in enumerate(books):
        stack[i, :min(grid_len, b[1].size)] = b[1][:grid_len]
        stack[i, min(grid_len, b[1].size):] = -(i + 1.5)                # (padding that names its row)
    outl = np.arange(nt * 7, dtype=np.float32).reshape(nt, 7) * np.float32(1.25) + np.float32(33)
    scores = (np.arange(nt, dtype=np.float32) + np.float32(0.1)) * np.float32(3e-5)
    raw = torch.int32 if dtype_name == "float32" else torch.int16
    x = torch.from_numpy(x_bits_src.view(np.int32 if dtype_name == "float32" else np.int16).copy()).to(dev)
    assert x.data_ptr() % 16 == 0
    n = x.numel()
    out, a_out, m_out, g_out, o_out = (Carved(n, dtype_name, dev), Carved(1, "float32", dev), Carved(1, "float32", dev), Carved(grid_len, "float32", dev),
                                       Carved(7, "float32", dev))
    typ = torch.tensor([t_planted], dtype=torch.int32, device=dev)
    ok = L.calibrate_install(x.view(getattr(torch, dtype_name)), out.view, plans, gmaxs, typ, _f(alphas, dev), _f(scores, dev), _f(stack.reshape(-1), dev).view(nt, grid_len),
                             g_out.view, a_out.view, m_out.view if optional else None, ovp=ovp, outl=_f(outl.reshape(-1), dev).view(nt, 7) if optional else None,
                             outl_out=o_out.view if optional else None)
    assert ok is True, (tag, "refused")
    want = want_of(t)
    got = out.bits(tag)
    if dtype_name == "float32":
        bad = np.flatnonzero(~_same32(got.view(np.float32), want.view(np.float32)))
    else:
        wf = fc.widen16(_oracle_mod(), want, dtype_name)
        gf = fc.widen16(_oracle_mod(), got, dtype_name)
        bad = np.flatnonzero((got != want) & ~(np.isnan(gf) & np.isnan(wf)))
    assert bad.size == 0, (tag, "%d of %d outputs differ from the oracle" % (bad.size, n), "at", bad[:6].tolist(), "got", [hex(int(v)) for v in got[bad[:6]]],
                           "want", [hex(int(v)) for v in want[bad[:6]]])
    assert a_out.bits(tag)[0] == _bits(alphas[t:t + 1])[0], (tag, "alpha_out is not alpha[%d]" % t)
    assert np.array_equal(g_out.bits(tag), _bits(stack[t])), (tag, "grid_out is not row %d" % t)
    if optional:
        assert m_out.bits(tag)[0] == _bits(scores[t:t + 1])[0], (tag, "mse_out is not score[%d]" % t)
        assert np.array_equal(o_out.bits(tag), _bits(outl[t])), (tag, "outl_out is not row %d" % t)
    else:
        m_out.untouched(tag)
        o_out.untouched(tag)
    assert np.array_equal(x.cpu().numpy().view(x_bits_src.dtype), x_bits_src), (tag, "x changed")
    if fq is not None:                                  # the same plan through per-tensor antq_fakequant: the same bits
        f = L.fakequant(x.view(getattr(torch, dtype_name)), _f(alphas[t:t + 1], dev), plans[t], gmaxs[t], 1, n, False, ovp=ovp)
        fb = f.view(raw).cpu().numpy().view(got.dtype)
        if dtype_name == "float32":
            same = _same32(fb.view(np.float32), want.view(np.float32))
        else:
            same = (fb == want) | (np.isnan(fc.widen16(_oracle_mod(), fb, dtype_name)) & np.isnan(fc.widen16(_oracle_mod(), want, dtype_name)))
        assert same.all(), (tag, "per-tensor antq_fakequant differs from the oracle")


def _oracle_mod():
    from oracle import antq_oracle
    return antq_oracle


# of fakequant_cases.scales_for(rng(5), gmax, 16): an awkward scale, a short-mantissa one (3 * 2^-9), the float below s = 2^-40 and
# the one above s = 2^40 (both outside Scale::ok: the literal division)
SCALE_PICKS = (0, 7, 8, 11)


def _picks(nt):
    return list(range(nt)) + [-1, nt, -2 ** 31, 2 ** 31 - 1]


def test_install_fp32_decision_edges_every_pick(dev, oracle):
    """fp32: per type list (one to four types; a 4-bit table plan, int-8 whose table sizes the LDS, a scan plan and an OliVe book
    mixed in one call) the decision-edge cases of fakequant_cases.edges_case of EVERY book of the list at its own alpha (an
    awkward one, a short-mantissa one, one just below s = 2^-40, one just above s = 2^40) in one tensor; picks 0 .. ntypes - 1, and -1, ntypes,
    INT_MIN, INT_MAX (clamped to the ends); with and without ANTQ_FLAG_OVP; sizes of one vector, 255 vectors and the whole
    tensor; grid_len 16, 256 and 300."""
    from ant_quantization_amd import _lib as L
    for li, names in enumerate(INSTALL_LISTS):
        books = [_install_books()[n] for n in names]
        heads = [fc.plan_header(L.plan_for(b[1]).host) for b in books]
        if len(names) >= 3:
            assert {h["kind"] for h in heads} == {fc.PLAN_SCAN, fc.PLAN_TABLE} and max(b[1].size for b in books) >= 255, "the list does not mix plan kinds"
        for si in range(len(SCALE_PICKS)):
            rng = np.random.default_rng(900 + 10 * li + si)
            alphas = np.float32([fc.scales_for(np.random.default_rng(5), b[2], 16)[SCALE_PICKS[si]] for b in books])
            parts = [fc.edges_case(oracle, rng, b, h, 72, alpha=[a])["x"].reshape(-1) for b, h, a in zip(books, heads, alphas)]
            x_all = np.concatenate(parts + [np.float32([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-42, -3e38, 1e30])]).astype(np.float32)
            x_all = x_all[:x_all.size // 4 * 4]
            for n in (4, 255 * 4, x_all.size):
                xs = np.resize(x_all[rng.permutation(x_all.size)], n) if n < x_all.size else x_all
                for ovp in (False, True):
                    @functools.lru_cache(maxsize=None)
                    def want_of(t, xs=xs, ovp=ovp):
                        with np.errstate(all="ignore"):
                            return _bits(oracle.forward(xs.reshape(1, -1), alphas[t:t + 1], books[t][1], books[t][2], ovp, want_idx=False)[0].reshape(-1))
                    for t in (_picks(len(names)) if n != 4 else [0, len(names) - 1]):
                        grid_len = (16, 256, 300)[(li + si + t) % 3] if max(b[1].size for b in books) <= 16 else (256, 300)[(si + t) % 2]
                        _install(L, dev, "float32", ("fp32", names, "scale set %d" % si, "n %d" % n, "ovp %s" % ovp, "pick %d" % t), _bits(xs), names, t, ovp,
                                 alphas, want_of, grid_len, optional=(t + si) % 2 == 0, fq=True if n == x_all.size else None)


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float16"])
def test_install_all_16bit_patterns_every_pick(dev, oracle, dtype_name):
    """bf16 / f16: all 65 536 patterns in order and shuffled (8192 vectors: 32 workgroups), one vector and 255 vectors of
    them; the oracle's fp32 sequence rounded once to the type."""
    from ant_quantization_amd import _lib as L
    pats = np.arange(65536, dtype=np.uint16)
    shuffled = np.random.default_rng(31).permutation(pats)
    for li, names in enumerate(INSTALL_LISTS):
        books = [_install_books()[n] for n in names]
        alphas = np.float32([fc.scales_for(np.random.default_rng(5), b[2], 16)[SCALE_PICKS[(li + i) % 4]] for i, b in enumerate(books)])
        for label, xs in (("in order", pats), ("shuffled", shuffled), ("one vector", shuffled[:8]), ("255 vectors", shuffled[1000:1000 + 255 * 8])):
            xf = fc.widen16(oracle, xs, dtype_name)
            for ovp in (False, True):
                @functools.lru_cache(maxsize=None)
                def want_of(t, xf=xf, ovp=ovp):
                    with np.errstate(all="ignore"):
                        return fc.round16(oracle, oracle.forward(xf.reshape(1, -1), alphas[t:t + 1], books[t][1], books[t][2], ovp, want_idx=False)[0].reshape(-1), dtype_name)
                for t in (_picks(len(names)) if xs.size == 65536 else [0, len(names) - 1]):
                    grid_len = (16, 256, 300)[(li + t) % 3] if max(b[1].size for b in books) <= 16 else (256, 300)[t % 2]
                    _install(L, dev, dtype_name, (dtype_name, names, label, "ovp %s" % ovp, "pick %d" % t), xs, names, t, ovp, alphas, want_of, grid_len,
                             optional=t % 2 == 0, fq=True if label == "shuffled" else None)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_install_grid_stride_loop(dev, oracle, dtype_name):
    """k_fq_select launches at most 256 * 16 workgroups of 256 lanes: a tensor of 256 * 16 * 256 + 3 vectors makes the first
    three lanes walk a second vector.  4-bit books only (two of them, the second picked)."""
    from ant_quantization_amd import _lib as L
    names = ("flint_b4_s", "int_b4_s")
    books = [_install_books()[n] for n in names]
    nv = 256 * 16 * 256 + 3
    n = nv * cc.EPL[dtype_name]
    rng = np.random.default_rng(41)
    alphas = np.float32([0.731, 1.37])
    if dtype_name == "float32":
        xf = (np.clip(rng.standard_normal(n), -5, 5) * 0.4).astype(np.float32)
        xf[-12:] = np.float32([0.0, -0.0, np.nan, np.inf, 1.37, -1.37, 0.6850001, 5.0, -9.0, 1e-40, 2.74, -0.3])
        src = _bits(xf)
    else:
        src = np.resize(rng.permutation(np.arange(65536, dtype=np.uint16)), n)
        xf = fc.widen16(oracle, src, dtype_name)

    def want_of(t):
        with np.errstate(all="ignore"):
            o = oracle.forward(xf.reshape(1, -1), alphas[t:t + 1], books[t][1], books[t][2], False, want_idx=False)[0].reshape(-1)
        return _bits(o) if dtype_name == "float32" else fc.round16(oracle, o, dtype_name)
    assert (nv + 255) // 256 > 256 * 16, "the launch is not capped: no lane loops"
    _install(L, dev, dtype_name, (dtype_name, "grid stride", nv), src, names, 1, False, alphas, want_of, 16)


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_install_refusals_write_nothing(dev, dtype_name):
    """A ragged n, an unaligned x or an unaligned out: ANTQ_ERR_UNSUPPORTED (the binding's False) with every output still
    poisoned."""
    from ant_quantization_amd import _lib as L
    books = [_install_books()[n] for n in ("flint_b4_s", "int_b4_s")]
    plans, gmaxs = [L.plan_for(b[1]) for b in books], [b[2] for b in books]
    epl = cc.EPL[dtype_name]
    dt = getattr(torch, dtype_name)
    stack = _f(np.stack([b[1] for b in books]).reshape(-1), dev).view(2, 16)
    typ = torch.tensor([1], dtype=torch.int32, device=dev)
    for label, n, xlead, olead in (("ragged n", 64 * epl + 1, 0, 0), ("ragged n", epl - 1, 0, 0), ("unaligned x", 64 * epl, 1, 0), ("unaligned out", 64 * epl, 0, 1),
                                   ("both unaligned", 64 * epl, epl // 2, epl // 2)):
        full = torch.zeros(n + 32, dtype=dt, device=dev)
        assert full.data_ptr() % 16 == 0
        x = full[xlead:xlead + n]
        out, a_out, m_out, g_out, o_out = Carved(n, dtype_name, dev, lead=olead), Carved(1, "float32", dev), Carved(1, "float32", dev), Carved(16, "float32", dev), Carved(7, "float32", dev)
        assert (x.data_ptr() % 16 != 0) == bool(xlead) and (out.view.data_ptr() % 16 != 0) == bool(olead)
        ok = L.calibrate_install(x, out.view, plans, gmaxs, typ, _f([0.5, 0.7], dev), _f([1e-4, 2e-4], dev), stack, g_out.view, a_out.view, m_out.view,
                                 outl=_f(np.arange(14), dev).view(2, 7), outl_out=o_out.view)
        assert ok is False, (label, "antq_calibrate_install accepted the call")
        for c in (out, a_out, m_out, g_out, o_out):
            c.untouched((dtype_name, label))
