"""Every clip-search kernel against the exact float64 sums of the oracle's per-element outputs (calib_check.exact_sse).

The sorted-row search (csrc/antq_k_sortsearch.h: the 4096-key kernel, the one-row-per-wavefront short form, the one-scale
form), the threshold sweep (antq_k_sweep.h), the 16-bit histogram search (antq_k_hist.h) and the direct kernels
(antq_k_search.h) are compared with a yardstick that is no kernel of this library:
  * the closed forms (sorted search, sweep) with `exact`   = sum of float64(fl32(out - x))^2,
  * the histogram search and the direct kernels with `terms32` = sum of float64(fl32(d * d)), what the reference's recorded
    *_traces64.npz scores are.
EVERY (codebook, candidate, row) cell is compared, the NaN pattern separately; every case first proves that the intended
kernel ran (its bits differ from the direct kernels').  Bars: calib_check.EXACT_RTOL / HIST_RTOL / DIRECT_RTOL, derived from
the worst deviation measured over all cells on the MI355X (profiles/search_exactness.md).  One misplaced element in a row of
4096 moves `exact` by 3e-9 and more in 99 % of the cells (tests/test_exact_sse.py).
"""
import glob
import os

import numpy as np
import pytest

import calib_check
from calib_check import exact_sse, ratios_of
from conftest import GOLDEN

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DIRECT, SORTED, SORTED_DEFAULT, SWEEP = (0, 0), (1, 2), (1, 1), (2, 0)        # (knob 19, knob 20)
MEASURED = {}          # (family, dtype) -> [cells, worst, case of the worst]: printed by every test (pytest -s)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rt(ratios, dev):
    return torch.from_numpy(np.ascontiguousarray(ratios, dtype=np.float32)).to(dev)


def _search(L, path, x, rows, K, xm, per_row, rt, plans, gmaxs, ovp, k21=1, k14=1):
    """[ntypes, ncand, rows or 1] float64 through one path: knobs 19 / 20 (/ 21 / 14) set, always restored."""
    knob = L.lib().antq_debug_set
    knob(19, path[0]); knob(20, path[1]); knob(21, k21); knob(14, k14)
    try:
        s = L.search_sse_multi(x, rows, K, xm, per_row, rt, plans, gmaxs, ovp=ovp) if len(plans) > 1 else None
        if s is None:
            s = torch.stack([L.search_sse(x, rows, K, xm, per_row, rt, p, g, ovp=ovp) for p, g in zip(plans, gmaxs)])
        return s.clone().cpu().numpy()
    finally:
        knob(19, 1); knob(20, 1); knob(21, 1); knob(14, 1)


def _yard(oracle, x, xm, ratios, cbs, ovp, per_row, which):
    """The yardstick for every codebook: [ntypes, ncand, rows or 1]; x: the tensor on the device (its float32 image is used)."""
    xn = x.float().cpu().numpy()
    xn = xn.reshape(xn.shape[0], -1) if per_row else xn.reshape(1, -1)
    xmn = xm.cpu().numpy()
    return np.stack([exact_sse(oracle, xn, xmn, ratios, g, m, ovp, per_row)[which] for g, m in cbs])


def _hold(family, case, dtype_name, got, want, bar, loose=None):
    """Every cell of `got` within `bar` of the yardstick (relative), the same NaN / Inf pattern, noise only where the
    yardstick is zero.  loose = {row: bar}: rows named by the caller for which the closed form legitimately loses digits."""
    assert got.shape == want.shape, (case, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (family, case, "NaN pattern")
    assert np.array_equal(np.isinf(got), np.isinf(want)), (family, case, "Inf pattern")
    fin = np.isfinite(want)
    # a yardstick sum of exactly zero (every element ON a codebook value) has no relative error: there the closed form's
    # cancellation noise is held to `bar` times the row's largest finite sum over the candidates (the scale of its terms)
    top = np.broadcast_to(np.where(fin, want, 0.0).max(axis=1, keepdims=True), want.shape)
    zero = fin & (want == 0)
    assert np.all(np.abs(got[zero]) <= bar * top[zero]), (family, case, "zero sums", got[zero])
    ok = fin & (want != 0)
    with np.errstate(all="ignore"):
        rel = np.where(ok, np.abs(got - want) / np.abs(want), 0.0)
    if loose:
        lrows = sorted(loose)
        assert len(lrows) <= 0.05 * got.shape[2], (case, "more than 5 % of the rows named")
        for r in lrows:
            sub = rel[:, :, r]
            t, c = np.unravel_index(int(sub.argmax()), sub.shape)
            _note(family + " (named rows)", dtype_name, int(ok[:, :, r].sum()), float(sub.max()), "%s, row %d" % (case, r))
            assert float(sub.max()) <= loose[r], (family, case, "named row %d" % r, "type %d cand %d" % (t, c), got[t, c, r], want[t, c, r], float(sub.max()), loose[r])
        rel = rel.copy()
        rel[:, :, lrows] = 0.0
        ok = ok.copy()
        ok[:, :, lrows] = False
    worst = float(rel.max()) if rel.size else 0.0
    _note(family, dtype_name, int(ok.sum()), worst, case)
    if worst > bar:
        t, c, r = np.unravel_index(int(rel.argmax()), rel.shape)
        raise AssertionError((family, case, dtype_name, "type %d cand %d row %d" % (t, c, r), "got %.17g" % got[t, c, r],
                              "yardstick %.17g" % want[t, c, r], "rel %.3g > %.3g" % (worst, bar)))


def _note(family, dtype_name, cells, worst, case):
    m = MEASURED.setdefault((family, dtype_name), [0, 0.0, None])
    m[0] += cells
    if worst >= m[1]:
        m[1], m[2] = worst, case
    print("EXACTNESS | %s | %s | %s | %d | %.3g" % (family, dtype_name, case, cells, worst), flush=True)


def _ant(L, grids, signed=True, types=("int", "pot", "flint", "float")):
    cbs = [(grids.ant_grid(t, 4, signed), 10.0) for t in types]
    return cbs, [L.plan_for(g) for g, _ in cbs], [m for _, m in cbs]


def _olive(L, grids):
    oo = grids.olive_outliers(4, True)
    cbs = [(np.concatenate([grids.olive_grid(t, 4, True), oo]), float(grids.olive_grid(t, 4, True).max())) for t in ("int", "flint")]
    return cbs, [L.plan_for(g) for g, _ in cbs], [m for _, m in cbs]


def _laplace_outliers(rows, K, dev, gen):
    """The existing recipe (test_gpu_sort_r6.py): small values with one element in 300 blown up 8 .. 64 times."""
    x = torch.randn(rows, K, device=dev, generator=gen) * 0.02
    n = max(1, x.numel() // 300)
    idx = torch.randint(0, x.numel(), (n,), device=dev, generator=gen)
    x.view(-1)[idx] *= torch.empty(n, device=dev).uniform_(8, 64, generator=gen)
    return x


def _well_scaled(x, xm, named=()):
    """CPU check of the inputs: outside the named rows no statistic lies 2^15 or more above its row's elements (the domain
    in which the fixed-point sums of the closed form are exact), so no case below may ask for a looser bar there."""
    a = x.float().abs().amax(1).cpu().numpy().astype(np.float64)
    s = xm.cpu().numpy().astype(np.float64)
    for r in range(a.size):
        if r not in named:
            assert np.isfinite(a[r]) and a[r] > 0 and s[r] < 2.0 ** 15 * a[r] and a[r] < 2.0 ** 15 * s[r], (r, a[r], s[r])


EPL = {"float32": 4, "bfloat16": 8, "float16": 8}
ANT_RATIOS = ratios_of(75, 150, 1)            # 75 candidates
OLIVE_RATIOS = ratios_of(75, 250, 2)          # 88 candidates


def _row_shapes(epl):
    """(K, rows): where the sorted search can go wrong.  1024 is the last row of the short form, 1024 + EPL the first of the
    4096-key kernel; the short form packs four rows per workgroup, so 2 .. 5 rows exercise a partial last workgroup."""
    ks = [128, 256, 264, 576, 768, 1024, 1024 + epl, 4096, 4096 + epl, 4096 + 64, 2 * 4096 - epl, 3 * 4096, 11008, 16384]
    counts = [2, 3, 4, 5, 9]
    out = [(K, counts[i % 5]) for i, K in enumerate(ks)]
    out += [(K, r) for K in (128, 1024, 1024 + epl, 4096) for r in counts if (K, r) not in out]
    return out


# ------------------------------------------------------------------------------------------- a. the sorted search, rows
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16", "float16"])
def test_sorted_rows_every_shape_vs_exact(dev, oracle, dtype_name):
    from ant_quantization_amd import _lib as L, grids
    dt = getattr(torch, dtype_name)
    gen = torch.Generator(device=dev).manual_seed(8101)
    acb, aplans, agm = _ant(L, grids)
    ocb, oplans, ogm = _olive(L, grids)
    for K, rows in _row_shapes(EPL[dtype_name]):
        x = torch.randn(rows, K, device=dev, generator=gen) * 0.03
        x[::3] *= 0.2
        x = x.to(dt)
        xm = L.absmax(x, rows, K)
        _well_scaled(x, xm)
        d = _search(L, DIRECT, x, rows, K, xm, True, _rt(ANT_RATIOS, dev), aplans, agm, False)
        s = _search(L, SORTED, x, rows, K, xm, True, _rt(ANT_RATIOS, dev), aplans, agm, False)
        assert not np.array_equal(d, s), "the sorted search did not run: the comparison would prove nothing"
        _hold("sorted rows, ANT", "gauss %dx%d" % (rows, K), dtype_name, s, _yard(oracle, x, xm, ANT_RATIOS, acb, False, True, 0), calib_check.EXACT_RTOL)
        if K < 256:
            continue                                       # (the pair rule's entry is 256)
        x = _laplace_outliers(rows, K, dev, gen).to(dt)
        xm = L.xmax_3sigma(x, rows, K, per_row=True)
        _well_scaled(x, xm)
        for ovp in (True, False):
            d = _search(L, DIRECT, x, rows, K, xm, True, _rt(OLIVE_RATIOS, dev), oplans, ogm, ovp)
            s = _search(L, SORTED, x, rows, K, xm, True, _rt(OLIVE_RATIOS, dev), oplans, ogm, ovp)
            assert not np.array_equal(d, s), "the sorted search did not run"
            _hold("sorted rows, OliVe pairs" if ovp else "sorted rows, OliVe no pairs", "laplace+outliers %dx%d" % (rows, K), dtype_name, s,
                  _yard(oracle, x, xm, OLIVE_RATIOS, ocb, ovp, True, 0), calib_check.EXACT_RTOL)


def _neighbours(v, dt):
    """v (float32, any sign) in dtype dt with its two neighbours in dt: [3, n]."""
    w = v.to(dt)
    it = torch.int32 if dt == torch.float32 else torch.int16
    bits = w.view(it)
    return torch.stack([w, (bits + 1).view(dt), (bits - 1).view(dt)])


def _boundary_rows(x, xm, cands, cbs, dt):
    """Overwrite the head of every row of x with elements ON decision boundaries: for the candidate scales s of `cands` and
    every threshold T_k (the midpoints of adjacent codebook values) of every codebook, fl(T_k * s) and its two neighbours,
    both signs.  xm: the statistic given to the search (the planted values do not change it)."""
    rows, K = x.shape
    for r in range(rows):
        vals = []
        for (g, gmax), c in [(cb, c) for cb in cbs for c in cands]:
            alpha = np.float32(xm[r].item()) * np.float32(c)
            s = np.float32(alpha / np.float32(gmax))
            u = np.unique(g.astype(np.float64))
            T = ((u[1:] + u[:-1]) / 2).astype(np.float32)
            vals.append((T * s).astype(np.float32))
        v = torch.from_numpy(np.concatenate(vals)).to(x.device)
        v = v[v != 0]
        nb = _neighbours(torch.cat([v, -v]), dt).reshape(-1)
        n = min(nb.numel(), K - K // 4)
        x[r, :n] = nb[torch.randperm(nb.numel(), device=x.device)[:n]]
    return x


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16", "float16"])
def test_sorted_rows_hard_contents_vs_exact(dev, oracle, dtype_name):
    """Duplicates and exact zeros, elements on decision boundaries, pairs of outliers, outliers at the seam of two chunks, the
    pair list's overflow, the 4096-key kernel on short rows (knob 21 = 0), a 280-candidate list, irregular / descending lists."""
    from ant_quantization_amd import _lib as L, grids
    dt = getattr(torch, dtype_name)
    epl = EPL[dtype_name]
    gen = torch.Generator(device=dev).manual_seed(8102)
    torch.manual_seed(8102)
    acb, aplans, agm = _ant(L, grids)
    ocb, oplans, ogm = _olive(L, grids)
    art, ort = _rt(ANT_RATIOS, dev), _rt(OLIVE_RATIOS, dev)

    def ant(case, x, xm, k21=1, ratios=ANT_RATIOS, cbs=acb, plans=aplans, gm=agm, differ=True):
        rows, K = x.shape
        s = _search(L, SORTED, x, rows, K, xm, True, _rt(ratios, dev), plans, gm, False, k21=k21)
        if differ:
            assert not np.array_equal(s, _search(L, DIRECT, x, rows, K, xm, True, _rt(ratios, dev), plans, gm, False)), "the sorted search did not run"
        _hold("sorted rows, ANT", case, dtype_name, s, _yard(oracle, x, xm, ratios, cbs, False, True, 0), calib_check.EXACT_RTOL)
        return s

    def olive(case, x, xm, k21=1):
        rows, K = x.shape
        for ovp in (True, False):
            s = _search(L, SORTED, x, rows, K, xm, True, ort, oplans, ogm, ovp, k21=k21)
            assert not np.array_equal(s, _search(L, DIRECT, x, rows, K, xm, True, ort, oplans, ogm, ovp)), "the sorted search did not run"
            _hold("sorted rows, OliVe pairs" if ovp else "sorted rows, OliVe no pairs", case, dtype_name, s,
                  _yard(oracle, x, xm, OLIVE_RATIOS, ocb, ovp, True, 0), calib_check.EXACT_RTOL)

    for rows, K in ((5, 768), (3, 4096 + 64), (2, 16384)):
        # ReLU rows: half the elements exactly zero (+0 and -0), the rest drawn from 40 distinct values; signed and unsigned codebooks
        pool = (torch.randn(40, device=dev, generator=gen).abs() * 0.05).to(dt)
        x = pool[torch.randint(0, 40, (rows, K), device=dev, generator=gen)]
        x = torch.where(torch.rand(rows, K, device=dev, generator=gen) < 0.5, torch.zeros_like(x), x)
        x[:, 1::16] = -0.0
        xm = L.absmax(x, rows, K)
        _well_scaled(x, xm)
        ant("duplicates, zeros %dx%d" % (rows, K), x, xm)
        ucb, uplans, ugm = _ant(L, grids, signed=False, types=("int", "flint"))
        ant("duplicates, zeros, unsigned codebooks %dx%d" % (rows, K), x, xm, cbs=ucb, plans=uplans, gm=ugm)
        # elements ON the decision boundaries of five candidate scales (and one ulp to either side)
        x = (torch.randn(rows, K, device=dev, generator=gen) * 0.03).to(dt)
        xm = L.absmax(x, rows, K)
        x = _boundary_rows(x, xm, [ANT_RATIOS[i] for i in (0, 1, 37, 73, 74)], acb, dt)
        _well_scaled(x, xm)
        ant("boundaries %dx%d" % (rows, K), x, xm)
        x = _laplace_outliers(rows, K, dev, gen).to(dt)
        xm = L.xmax_3sigma(x, rows, K, per_row=True)
        x = _boundary_rows(x, xm, [OLIVE_RATIOS[i] for i in (0, 1, 44, 87)], ocb, dt)
        _well_scaled(x, xm)
        olive("boundaries %dx%d" % (rows, K), x, xm)
    # pairs: both members outliers; an outlier in the last pair of a chunk and in the first pair of the next; an outlier
    # beside a far-clipped element; the statistic is given (the planted values would move a 3-sigma statistic)
    for rows, K in ((4, 2 * 4096), (3, 3 * 4096), (5, 1024), (4, 576)):
        x = _laplace_outliers(rows, K, dev, gen)
        xm = L.xmax_3sigma(x.to(dt), rows, K, per_row=True)
        x[0, 10:14] = torch.tensor([0.9, -1.1, 0.8, 0.7], device=dev)
        x[1, 20] = 30.0
        for e in (K // 2 - 2, K // 2 - 1, K // 2, K // 2 + 1, K - 2, K - 1, 0, 1):
            x[2, e] = 0.7 if e % 3 else -0.9
        if K > 4096:
            x[1, 4094:4098] = torch.tensor([0.8, 0.01, 0.02, -0.9], device=dev)
            x[rows - 1, 4095] = 1.2
            x[rows - 1, 4096] = -1.3
        x = x.to(dt)
        _well_scaled(x, xm)
        olive("planted pairs %dx%d" % (rows, K), x, xm)
    x = _laplace_outliers(20, 1024, dev, gen)
    x[:, ::8] *= 12.0                                    # an outlier in every fourth pair: the short form's pair list overflows
    x = x.to(dt)
    xm = L.xmax_3sigma(x, 20, 1024, per_row=True)
    _well_scaled(x, xm)
    olive("pair list overflow 20x1024", x, xm)
    # the short shapes through the 4096-key kernel (knob 21 = 0), a 280-candidate list (goes out in pieces), a list from 0.3
    for rows, K in ((5, 128), (7, 768), (6, 1024)):
        x = (torch.randn(rows, K, device=dev, generator=gen) * 0.03).to(dt)
        xm = L.absmax(x, rows, K)
        _well_scaled(x, xm)
        a = ant("knob 21 = 0, %dx%d" % (rows, K), x, xm, k21=0)
        b = ant("short form, %dx%d" % (rows, K), x, xm)
        assert a.shape == b.shape
        for k21 in (1, 0):
            ant("280 candidates, knob 21 = %d, %dx%d" % (k21, rows, K), x, xm, k21=k21, ratios=ratios_of(20, 300, 1))
        if K >= 256:
            xo = _laplace_outliers(rows, K, dev, gen).to(dt)
            olive("knob 21 = 0, %dx%d" % (rows, K), xo, L.xmax_3sigma(xo, rows, K, per_row=True), k21=0)
    x = (torch.randn(6, 4096 + epl, device=dev, generator=gen) * 0.03).to(dt)
    xm = L.absmax(x, 6, 4096 + epl)
    ant("280 candidates 6x%d" % (4096 + epl), x, xm, ratios=ratios_of(20, 300, 1))
    irregular = np.float32([0.5, 0.51, 0.7, 0.71, 0.72, 0.9, 1.3, 1.31, 2.0])
    for K in (1024, 4096 + 64):
        x = (torch.randn(5, K, device=dev, generator=gen) * 0.03).to(dt)
        xm = L.absmax(x, 5, K)
        ant("irregular ratios 5x%d" % K, x, xm, ratios=irregular)
        ant("descending ratios 5x%d" % K, x, xm, ratios=ANT_RATIOS[::-1].copy(), differ=False)


def test_sorted_rows_literal_elements_vs_exact(dev, oracle):
    """NaN, +-Inf, 1e30 and far-clipped elements take the literal sequence; a zero statistic gives NaN for every candidate.
    Two of the 48 rows are named, with bars of their own:
      row 4: one element of 1e30 in a row of 0.02-sized ones -- a statistic 2^100 above the elements (every output is zero);
             measured 8.2e-15, bar 8 x that;
      row 5: every element 0.5 -- for some candidates the row sits ON a codebook value to a float32 rounding, the sum is 1e-14
             of sum x^2 and a closed form in double, whose terms are of the size of sum x^2, cannot resolve it: the bar is
             EXACT_RTOL relative to sum x^2 (the size of the terms) instead of to the sum itself."""
    from ant_quantization_amd import _lib as L, grids
    torch.manual_seed(8103)
    cbs, plans, gm = _ant(L, grids, types=("int", "flint"))
    for K, k21 in ((1024, 1), (1024, 0), (4096 + 64, 1)):
        x = torch.randn(48, K, device=dev) * 0.02
        x[0] = 0.0
        x[1, 5] = float("nan")
        x[2, 7] = float("inf")
        x[3, 9] = -float("inf")
        x[4, 11] = 1e30
        x[5] = 0.5
        x[6, ::2] = 0.0
        x[7] = -x[7].abs()
        x[8, 100:140] *= 300.0                   # far-clipped against the given statistic below
        x[10, 3] = -0.0
        xm = L.absmax(x, 48, K)
        xm[8] = 0.05
        s = _search(L, SORTED, x, 48, K, xm, True, _rt(ANT_RATIOS, dev), plans, gm, False, k21=k21)
        want = _yard(oracle, x, xm, ANT_RATIOS, cbs, False, True, 0)
        assert np.isnan(want[:, :, 0:4]).all() and np.isfinite(want[:, :, 4:]).all()
        w5 = want[:, :, 5]
        bar5 = calib_check.EXACT_RTOL * float((x[5].double() ** 2).sum()) / float(w5[w5 > 0].min())
        _hold("sorted rows, ANT", "literal elements 48x%d knob 21 = %d" % (K, k21), "float32", s, want, calib_check.EXACT_RTOL,
              loose={4: calib_check.EXACT_RTOL_FAR_STATISTIC, 5: bar5})


# ------------------------------------------------------------------------------------------- b. the sweep, d. the direct kernels
@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16", "float16"])
def test_sweep_and_direct_kernels_vs_yardstick(dev, oracle, dtype_name):
    """The threshold sweep (knob 20 = 0, knob 19 = 2) against `exact`, the direct kernels (both off) against `terms32`, on a
    subset of the sorted search's shapes and contents."""
    from ant_quantization_amd import _lib as L, grids
    dt = getattr(torch, dtype_name)
    epl = EPL[dtype_name]
    gen = torch.Generator(device=dev).manual_seed(8104)
    acb, aplans, agm = _ant(L, grids)
    ocb, oplans, ogm = _olive(L, grids)
    art, ort = _rt(ANT_RATIOS, dev), _rt(OLIVE_RATIOS, dev)
    for K, rows in ((128, 5), (256, 2), (264, 3), (768, 4), (1024, 5), (1024 + epl, 9), (4096, 3), (4096 + 64, 2), (3 * 4096, 4), (11008, 2), (16384, 2)):
        x = torch.randn(rows, K, device=dev, generator=gen) * 0.03
        x[::3] *= 0.2
        x = x.to(dt)
        xm = L.absmax(x, rows, K)
        if rows >= 3:
            x = _boundary_rows(x, xm, [ANT_RATIOS[i] for i in (0, 37, 74)], acb, dt)
        _well_scaled(x, xm)
        ex = _yard(oracle, x, xm, ANT_RATIOS, acb, False, True, slice(None))          # [ntypes, 2, ncand, rows]
        d = _search(L, DIRECT, x, rows, K, xm, True, art, aplans, agm, False)
        _hold("direct kernels, ANT", "%dx%d" % (rows, K), dtype_name, d, ex[:, 1], calib_check.DIRECT_RTOL)
        if K >= 256:
            s = _search(L, SWEEP, x, rows, K, xm, True, art, aplans, agm, False)
            assert not np.array_equal(d, s), "the sweep did not run: the comparison would prove nothing"
            _hold("sweep rows, ANT", "%dx%d" % (rows, K), dtype_name, s, ex[:, 0], calib_check.EXACT_RTOL)
        if K < 256 or K % 2:
            continue
        x = _laplace_outliers(rows, K, dev, gen)
        x[0, 10:14] = torch.tensor([0.9, -1.1, 0.8, 0.7], device=dev)
        x = x.to(dt)
        xm = L.xmax_3sigma(x, rows, K, per_row=True)
        _well_scaled(x, xm)
        for ovp in (True, False):
            ex = _yard(oracle, x, xm, OLIVE_RATIOS, ocb, ovp, True, slice(None))
            d = _search(L, DIRECT, x, rows, K, xm, True, ort, oplans, ogm, ovp)
            _hold("direct kernels, OliVe pairs" if ovp else "direct kernels, OliVe no pairs", "%dx%d" % (rows, K), dtype_name, d, ex[:, 1],
                  calib_check.DIRECT_RTOL_OLIVE)
            s = _search(L, SWEEP, x, rows, K, xm, True, ort, oplans, ogm, ovp)
            assert not np.array_equal(d, s), "the sweep did not run"
            _hold("sweep rows, OliVe pairs" if ovp else "sweep rows, OliVe no pairs", "%dx%d" % (rows, K), dtype_name, s, ex[:, 0], calib_check.EXACT_RTOL)


# ------------------------------------------------------------------------------------------- c. one scale per tensor
def test_sorted_one_scale_fp32_vs_exact(dev, oracle):
    """k_search_sorted<.., PT> on fp32 tensors with ONE scale: GELU and unsigned ReLU tensors of 2^22 elements under the default
    rule, a 280 000-element tensor forced onto it, OliVe's codebooks with and without the pair rule."""
    from ant_quantization_amd import _lib as L, grids
    torch.manual_seed(8105)
    ratios = ratios_of(80, 150, 1)
    rt = _rt(ratios, dev)
    scb, splans, sgm = _ant(L, grids, types=("int", "flint"))
    ucb, uplans, ugm = _ant(L, grids, signed=False, types=("int", "flint"))
    for case, x, cbs, plans, gm, path in (("gelu 2^22", torch.nn.functional.gelu(torch.randn(1 << 22, device=dev)), scb, splans, sgm, SORTED_DEFAULT),
                                          ("relu 2^22+4096+8, unsigned", torch.relu(torch.randn((1 << 22) + 4096 + 8, device=dev)), ucb, uplans, ugm, SORTED_DEFAULT),
                                          ("gauss 280000, forced", torch.randn(70000 * 4, device=dev) * 0.3, scb, splans, sgm, SORTED)):
        n = x.numel()
        xm = L.absmax(x, 1, n, per_row=False)
        d = _search(L, DIRECT, x, 1, n, xm, False, rt, plans, gm, False)
        s = _search(L, path, x, 1, n, xm, False, rt, plans, gm, False)
        assert not np.array_equal(d, s), "the sorted search did not run"
        ex = _yard(oracle, x.reshape(1, -1), xm, ratios, cbs, False, False, slice(None))
        _hold("sorted one scale, ANT", case, "float32", s, ex[:, 0], calib_check.EXACT_RTOL)
        _hold("direct kernels one scale, ANT", case, "float32", d, ex[:, 1], calib_check.DIRECT_RTOL)
    ocb, oplans, ogm = _olive(L, grids)
    x = torch.randn((1 << 20) + 4096 * 3 + 16, device=dev) * 0.02
    idx = torch.randint(0, x.numel(), (x.numel() // 300,), device=dev)
    x[idx] *= torch.empty(idx.numel(), device=dev).uniform_(8, 64)
    xm = L.xmax_3sigma(x, 1, x.numel(), per_row=False)
    for ovp in (True, False):
        d = _search(L, DIRECT, x, 1, x.numel(), xm, False, _rt(OLIVE_RATIOS, dev), oplans, ogm, ovp)
        s = _search(L, SORTED_DEFAULT, x, 1, x.numel(), xm, False, _rt(OLIVE_RATIOS, dev), oplans, ogm, ovp)
        assert not np.array_equal(d, s), "the sorted search did not run"
        _hold("sorted one scale, OliVe pairs" if ovp else "sorted one scale, OliVe no pairs", "2^20+3*4096+16", "float32", s,
              _yard(oracle, x.reshape(1, -1), xm, OLIVE_RATIOS, ocb, ovp, False, 0), calib_check.EXACT_RTOL)


@pytest.mark.parametrize("dtype_name", ["bfloat16", "float16"])
def test_histogram_one_scale_16bit_vs_terms32(dev, oracle, dtype_name):
    """The histogram search of a 16-bit tensor with one scale (knob 14 = 2: every eligible tensor) against `terms32`: ANT and
    OliVe's pair rule on 2^21 elements (the 25 M-element shape, reduced to what the yardstick does in under a minute), and
    the tensor whose outlier-capable pairs overflow the segment list, which falls back to the direct kernels."""
    from ant_quantization_amd import _lib as L, grids
    dt = getattr(torch, dtype_name)
    torch.manual_seed(8106)
    acb, aplans, agm = _ant(L, grids, types=("int", "flint"))
    ocb, oplans, ogm = _olive(L, grids)
    n = 1 << 21
    x = (torch.randn(n, device=dev) * 0.3).to(dt)
    xm = L.absmax(x, 1, n, per_row=False)
    h = _search(L, DIRECT, x, 1, n, xm, False, _rt(ANT_RATIOS, dev), aplans, agm, False, k14=2)
    d = _search(L, DIRECT, x, 1, n, xm, False, _rt(ANT_RATIOS, dev), aplans, agm, False, k14=0)
    assert not np.array_equal(h, d), "the histogram search did not run"
    t32 = _yard(oracle, x.reshape(1, -1), xm, ANT_RATIOS, acb, False, False, 1)
    _hold("histogram one scale, ANT", "gauss 2^21", dtype_name, h, t32, calib_check.HIST_RTOL)
    _hold("direct kernels one scale, ANT", "gauss 2^21", dtype_name, d, t32, calib_check.DIRECT_RTOL)
    x = torch.randn(n, device=dev) * 0.02
    idx = torch.randint(0, n, (n // 300,), device=dev)
    x[idx] *= torch.empty(idx.numel(), device=dev).uniform_(8, 64)
    x = x.to(dt)
    xm = L.xmax_3sigma(x, 1, n, per_row=False)
    h = _search(L, DIRECT, x, 1, n, xm, False, _rt(OLIVE_RATIOS, dev), oplans, ogm, True, k14=2)
    d = _search(L, DIRECT, x, 1, n, xm, False, _rt(OLIVE_RATIOS, dev), oplans, ogm, True, k14=0)
    assert not np.array_equal(h, d), "the histogram search did not run"
    t32 = _yard(oracle, x.reshape(1, -1), xm, OLIVE_RATIOS, ocb, True, False, 1)
    _hold("histogram one scale, OliVe pairs", "laplace+outliers 2^21", dtype_name, h, t32, calib_check.HIST_RTOL)
    _hold("direct kernels one scale, OliVe pairs", "laplace+outliers 2^21", dtype_name, d, t32, calib_check.DIRECT_RTOL_OLIVE)
    # a clip statistic of ONE sigma makes a third of the elements outlier-capable: the list of segments overflows and the
    # direct kernels, enqueued behind the histogram, answer (the same bits as with the histogram switched off)
    n = 1 << 20
    x = (torch.randn(n, device=dev) * 0.05).to(dt)
    xm = torch.tensor([0.05], dtype=torch.float32, device=dev)
    h = _search(L, DIRECT, x, 1, n, xm, False, _rt(OLIVE_RATIOS, dev), oplans, ogm, True, k14=2)
    d = _search(L, DIRECT, x, 1, n, xm, False, _rt(OLIVE_RATIOS, dev), oplans, ogm, True, k14=0)
    assert np.array_equal(h.view(np.uint64), d.view(np.uint64)), "the overflowing tensor was not answered by the direct kernels"
    _hold("direct kernels one scale, OliVe pairs", "segment overflow 2^20 (behind the histogram)", dtype_name, h,
          _yard(oracle, x.reshape(1, -1), xm, OLIVE_RATIOS, ocb, True, False, 1), calib_check.DIRECT_RTOL_OLIVE)


# ------------------------------------------------------------------------------------------- e. the product entry points
def _check_calibration(case, dtype_name, oracle, x, rows, K, cbs, ovp, lo, up, step, alpha, score, typ, xm, bar):
    """antq_calibrate's outputs restated from the yardstick as include/antq.h defines them: per (type, row) the candidate with
    the smallest fl32(sse / K), the first on ties (best starts at 1e10, strict <) -- or one whose yardstick score ties the
    minimum within `bar`; score[t] = the float of the double sum over rows of the best mean squared error."""
    ratios = ratios_of(lo, up, step)
    xmn = xm.cpu().numpy()
    ex = _yard(oracle, x.reshape(rows, K), xm, ratios, cbs, ovp, True, 0)
    alpha, score = alpha.cpu().numpy(), score.cpu().numpy()
    for t in range(len(cbs)):
        mse = ex[t] / K
        best = mse.min(0)
        want_score = 0.0
        for r in range(rows):
            cand = (xmn[r] * ratios).astype(np.float32)
            hit = np.flatnonzero(cand == alpha[t, r])
            assert hit.size, (case, t, r, "alpha is not x_max times a candidate", alpha[t, r], xmn[r])
            assert min(mse[c, r] for c in hit) <= best[r] * (1 + bar), (case, t, r, "picked candidate", hit, "yardstick minimum at", int(mse[:, r].argmin()))
            want_score += float(np.float32(best[r]))
        np.testing.assert_allclose(score[t], np.float32(want_score), rtol=2.0 ** -22, err_msg=str((case, t)))
    _note("antq_calibrate picks", dtype_name, len(cbs) * rows, 0.0, case)


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
def test_calibrate_and_batch_picks_minimise_the_yardstick(dev, oracle, dtype_name):
    from ant_quantization_amd import _lib as L, grids
    dt = getattr(torch, dtype_name)
    epl = EPL[dtype_name]
    gen = torch.Generator(device=dev).manual_seed(8107)
    acb, aplans, agm = _ant(L, grids, types=("int", "pot", "flint"))
    ocb, oplans, ogm = _olive(L, grids)
    jobs, xs = [], []
    for K, rows in ((128, 5), (768, 4), (1024, 3), (1024 + epl, 2), (4096, 9), (4096 + 64, 3), (3 * 4096, 2), (16384, 2)):
        x = (torch.randn(rows, K, device=dev, generator=gen) * 0.03).to(dt)
        alpha, score, typ, xm = L.calibrate(x, rows, K, True, aplans, agm, 75, 150, 1, xmax="absmax")
        assert torch.equal(xm, L.absmax(x, rows, K))
        _check_calibration("calibrate %dx%d" % (rows, K), dtype_name, oracle, x, rows, K, acb, False, 75, 150, 1, alpha, score, typ, xm, calib_check.EXACT_RTOL)
        assert int(typ.item()) == int(np.argmin(np.where(np.isnan(score.cpu().numpy()), np.inf, score.cpu().numpy())))
        jobs.append((x, rows, K, True, aplans, agm, 75, 150, 1))
        xs.append((alpha.clone(), score.clone(), int(typ.item())))
        if K >= 256:
            xo = _laplace_outliers(rows, K, dev, gen).to(dt)
            alpha, score, typ, xm = L.calibrate(xo, rows, K, True, oplans, ogm, 75, 250, 2, xmax="3sigma", ovp=True)
            _check_calibration("calibrate OliVe pairs %dx%d" % (rows, K), dtype_name, oracle, xo, rows, K, ocb, True, 75, 250, 2, alpha, score, typ, xm,
                               calib_check.EXACT_RTOL)
    results, types = L.calibrate_batch(jobs, xmax="absmax")
    types = types.cpu().numpy()
    for i, ((x, rows, K, *_), (a1, s1, t1), (alpha, score, xm)) in enumerate(zip(jobs, xs, results)):
        _check_calibration("calibrate_batch job %d %dx%d" % (i, rows, K), dtype_name, oracle, x, rows, K, acb, False, 75, 150, 1, alpha, score, None, xm,
                           calib_check.EXACT_RTOL)
        assert torch.equal(alpha, a1) and torch.equal(score, s1) and int(types[i]) == t1, "the batch and the single call disagree"


# ------------------------------------------------------------------------------------------- f. the reference's recorded scores
@pytest.mark.parametrize("fname", sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLDEN, "*_select*_traces64.npz"))))
def test_reference_recorded_float64_scores_on_the_gpu(dev, oracle, fname):
    """search_sse / K of the installed codebook against the __trace64 the REFERENCE recorded (its float32 element terms,
    averaged in float64): the direct kernels at their terms32 bar, the sorted search and the sweep -- where the shape lets
    them run -- at the distance between `exact` and `terms32` (2^-24, tests/test_exact_sse.py) plus their own bar."""
    from ant_quantization_amd import _lib as L
    cases = calib_check.restated_traces64(oracle, os.path.join(GOLDEN, fname))
    ran = {"direct": 0, "sorted": 0, "sweep": 0}
    for c in cases:
        x = torch.from_numpy(c["x"]).to(dev)
        rows, K = c["x"].shape
        r_, k_ = (rows, K) if c["per_row"] else (1, rows * K)
        xm = torch.from_numpy(c["xmax"]).to(dev)
        plan, rt = L.plan_for(c["grid"]), _rt(c["ratios"], dev)
        want = (c["trace64"].reshape(c["ratios"].size, -1) * k_)[None]
        olive = fname.startswith("olive")
        d = _search(L, DIRECT, x, r_, k_, xm, c["per_row"], rt, [plan], [c["gmax"]], c["ovp"], k14=0)
        _hold("direct kernels vs reference trace64", fname[:-4], "float32", d, want, calib_check.DIRECT_RTOL_OLIVE if olive else calib_check.DIRECT_RTOL)
        ran["direct"] += 1
        for name, path in (("sorted", SORTED), ("sweep", SWEEP)):
            s = _search(L, path, x, r_, k_, xm, c["per_row"], rt, [plan], [c["gmax"]], c["ovp"], k14=0)
            if np.array_equal(s, d):
                continue                                      # (this shape / codebook has no such path: the direct kernels ran again)
            _hold("%s vs reference trace64" % name, fname[:-4], "float32", s, want, 2.0 ** -24 + calib_check.EXACT_RTOL)
            ran[name] += 1
    print("%s: %d calibrations; direct %d, sorted %d, sweep %d" % (fname, len(cases), ran["direct"], ran["sorted"], ran["sweep"]))
    assert ran["direct"] == len(cases)
    if "long" in fname:                      # (rows of 1024 elements and more; the "wide" files' rows are too short for the sorted search)
        assert ran["sorted"] >= len([c for c in cases if c["per_row"]]), ran
