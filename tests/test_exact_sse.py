"""The clip-search yardstick (calib_check.exact_sse) against the reference's recorded float64 scores, against itself and
against the oracle's own search -- CPU only.  The GPU kernels meet the yardstick in tests/test_gpu_search_exact.py."""
import glob
import os

import numpy as np
import pytest

import calib_check
from calib_check import exact_sse, restated_traces64
from conftest import GOLDEN

# Calibrations of a *_traces64.npz file whose final search the helper cannot restate, by name, with the reason.  (None today:
# with OliVe's 3-sigma statistic taken in the reference's own float32 op sequence every recorded calibration restates.)
NOT_RESTATED = {}

TRACE_FILES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*_traces64.npz")))


def _k(c):
    return c["x"].shape[1] if c["per_row"] else c["x"].size


@pytest.mark.parametrize("fname", TRACE_FILES)
def test_terms32_equals_the_reference_recorded_float64_scores(oracle, fname):
    """terms32 / K == the recorded __trace64 of every calibration, rtol 1e-14: two float64 sums of n <= 16 K non-negative
    terms in different orders differ by about sqrt(n) * 2^-53 ~ 1.4e-14 at the very most; measured <= 5e-16."""
    cases = restated_traces64(oracle, os.path.join(GOLDEN, fname))
    skip = NOT_RESTATED.get(fname, {})
    assert len(skip) <= 0.1 * len(cases), (fname, len(skip), len(cases))
    n = cells = 0
    worst = 0.0
    for c in cases:
        if c["key"] in skip:
            continue
        assert c["trace64"].shape[0] == c["ratios"].size, c["key"]
        _, t32 = exact_sse(oracle, c["x"], c["xmax"], c["ratios"], c["grid"], c["gmax"], c["ovp"], c["per_row"])
        got, ref = t32 / _k(c), c["trace64"].reshape(t32.shape)
        np.testing.assert_allclose(got, ref, rtol=1e-14, atol=0, err_msg="%s %s" % (fname, c["key"]))
        worst = max(worst, float((np.abs(got - ref) / ref).max()))
        n += 1
        cells += ref.size
    print("%s: %d of %d calibrations restated (%d scores), worst relative deviation %.2g" % (fname, n, len(cases), cells, worst))
    assert n >= 0.9 * len(cases)


def _gauss_rows(rows, K, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((rows, K)) * 0.03).astype(np.float32)


def _codebooks(oracle):
    ant = [(t, oracle.ant_grid(t, 4, True), 10.0, False, calib_check.ratios_of(75, 150, 1)) for t in ("int", "flint")]
    oo = oracle.olive_outlier_value(4, True)
    ol = [("olive-" + t, np.concatenate([oracle.olive_grid(t, 4, True), oo]), float(oracle.olive_grid(t, 4, True).max()), True,
           calib_check.ratios_of(75, 250, 2)) for t in ("int", "flint")]
    return ant + ol


def test_exact_and_terms32_differ_by_the_float32_rounding_of_the_terms(oracle):
    """Each term of terms32 is ONE float32 rounding of a non-negative number, so the two sums differ by at most 2^-24
    relative (terms that underflow float32 would add 2^-149 each: no row here comes near) -- and they do differ."""
    for K in (768, 4096, 16384):
        x = _gauss_rows(4, K, K)
        x[1, ::301] *= 20.0
        for name, grid, gmax, ovp, ratios in _codebooks(oracle):
            xmax = calib_check._three_sigma_reference(x, True) if ovp else calib_check._absmax(x, True)
            ex, t32 = exact_sse(oracle, x, xmax, ratios, grid, gmax, ovp, True)
            rel = np.abs(ex - t32) / ex
            assert (ex != t32).mean() > 0.99, (K, name)
            assert float(rel.max()) <= 2.0 ** -24, (K, name, float(rel.max()))
            # one scale for the whole tensor: the same elements, one sum
            ex1, t1 = exact_sse(oracle, x[:1], xmax[:1], ratios, grid, gmax, ovp, False)
            np.testing.assert_allclose(ex1[:, 0], ex[:, 0], rtol=1e-15)
            np.testing.assert_allclose(t1[:, 0], t32[:, 0], rtol=1e-15)


def test_oracle_search_trace_is_terms32_within_the_reference_score_noise(oracle):
    """oracle.search_mse's float32-accumulated mean times K against terms32: within calib_check.REFERENCE_SCORE_NOISE, the
    measured distance between a float32 score of the reference and the number it stands for."""
    for K in (256, 1024, 4096):
        x = _gauss_rows(6, K, 7 + K)
        for name, grid, gmax, ovp, ratios in _codebooks(oracle):
            xmax = calib_check._three_sigma_reference(x, True) if ovp else calib_check._absmax(x, True)
            lo, up, step = (75, 250, 2) if ovp else (75, 150, 1)
            _, _, trace = oracle.search_mse(x, xmax, lo, up, step, grid, gmax, ovp, True)
            _, t32 = exact_sse(oracle, x, xmax, ratios, grid, gmax, ovp, True)
            rel = np.abs(trace.astype(np.float64) * K - t32) / t32
            assert float(rel.max()) <= calib_check.REFERENCE_SCORE_NOISE, (K, name, float(rel.max()))


def test_yardstick_resolves_one_misplaced_element_in_a_4096_wide_row(oracle):
    """The resolving power the GPU tests rely on: in a Gaussian row of 4096 elements, give the ONE element nearest a decision
    boundary the neighbouring grid value instead (what a `<` for a `<=`, a bisection off by one position or a prefix sum read
    one slot late does).  `exact` then moves by more than 100 x the bar the sorted search is held to
    (calib_check.EXACT_RTOL) in at least 99 % of the (row, candidate) cells."""
    rows, K = 16, 4096
    x = _gauss_rows(rows, K, 11)
    xmax = calib_check._absmax(x, True)
    ratios = calib_check.ratios_of(75, 150, 1)
    for t in ("int", "flint"):
        grid = oracle.ant_grid(t, 4, True)
        gs = np.unique(grid.astype(np.float64))                      # (ascending; flint lists 0 twice)
        mid = (gs[1:] + gs[:-1]) / 2
        ex, _ = exact_sse(oracle, x, xmax, ratios, grid, 10.0, False, True)
        moved = np.empty_like(ex)
        for c in range(ratios.size):
            alpha = (xmax * ratios[c]).astype(np.float32)
            scale = (alpha / np.float32(10.0)).astype(np.float32)
            out = oracle.forward(x, alpha, grid, 10.0, False, want_idx=False)[0]
            u = x.astype(np.float64) / scale.astype(np.float64)[:, None]
            dist = np.abs(u[:, :, None] - mid[None, None, :])
            j = dist.min(2).argmin(1)                                   # the element nearest any boundary, per row
            k = dist[np.arange(rows), j].argmin(1)                      # ... and that boundary: between gs[k] and gs[k + 1]
            xj, oj = x[np.arange(rows), j], out[np.arange(rows), j]
            lo_v, hi_v = (gs[k].astype(np.float32) * scale).astype(np.float32), (gs[k + 1].astype(np.float32) * scale).astype(np.float32)
            assert np.all((oj == lo_v) | (oj == hi_v))
            other = np.where(oj == lo_v, hi_v, lo_v)
            d0 = (oj - xj).astype(np.float32).astype(np.float64)
            d1 = (other - xj).astype(np.float32).astype(np.float64)
            moved[c] = ex[c] - d0 * d0 + d1 * d1
        rel = np.abs(moved - ex) / ex
        frac = float((rel > 100 * calib_check.EXACT_RTOL).mean())
        print("%s: relative change of exact, median %.2g, 1%%-quantile %.2g; %.4f of the cells above 100 x %.1g"
              % (t, np.median(rel), np.quantile(rel, 0.01), frac, calib_check.EXACT_RTOL))
        assert frac >= 0.99, (t, frac)
