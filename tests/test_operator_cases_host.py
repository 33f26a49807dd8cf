"""The input builders of the operator edge tests (operator_cases.py) against the CPU oracle alone, no GPU: every midpoint
window of a book holds two oracle indices, every float64 narrowing triple narrows to two floats, the ties of duplicate and
unsorted grids go to the later scan index (once the lower value, once the upper), the horizon windows hold both an index and
ANTQ_IDX_NONE, the affine tie windows hold two levels, the float64 pair layouts hold every (form, position) and both
odd-count wrap cases, and no expected output contains a poison pattern.  A failure of test_gpu_operator_edges.py is then the
kernels', not the inputs'.  Each test prints the counts it measured (-s shows them)."""
import numpy as np
import pytest

import operator_cases as oc


def _header(antq_lib, g):
    return oc.plan_header(antq_lib.plan_for(g).host)


def _nearest(oracle, x, g):
    with np.errstate(all="ignore"):
        return oracle.nearest(x, g)


def test_the_grid_set_is_the_one_the_gpu_test_claims():
    grids = oc.nearest_grids()
    sizes = {g.size for k, g in grids.items() if k not in oc.BOOK_GRIDS and not k.startswith("random_")}
    assert set(oc.HAND_SIZES) <= sizes, sorted(sizes)
    assert grids["olive_flint_b8"].size == 509
    g = oc.grid32("m65_unsorted")
    assert g.size == 65 and not (g[:-1] <= g[1:]).all() and oc.fastlim_of(g) == 0
    for k in ("m63_unsorted", "m64_unsorted", "zeros_unsorted", "m3_dup_lower", "olive_flint"):
        g = oc.grid32(k)
        assert g.size <= 64 and not (g[:-1] <= g[1:]).all() and oc.fastlim_of(g) > 0, k
    # values that float cannot hold, both signed zeros, 65536 and the float above it, NaN and Inf
    assert (grids["tenths"] != grids["tenths"].astype(np.float32)).any()
    for k in ("zeros_pn", "zeros_np", "zeros_unsorted", "m64_unsorted"):
        z = oc.grid32(k)
        assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any(), k
    # (an outermost magnitude above 34133 leaves no |x| < 102399 - |v| beyond 2 |v|: both grids take the literal scan, one by
    # that rule and one as a "huge entry")
    assert np.abs(oc.grid32("mag65536")).max() == 65536 and oc.fastlim_of(oc.grid32("mag65536_next")) == 0
    assert oc.grid32("mag65536_next")[2].view(np.uint32) == np.float32(65536).view(np.uint32) + 1
    assert np.isnan(oc.grid32("nan_entry")).any() and np.isinf(oc.grid32("inf_entry")).any()
    # the gap ratio just under, at and just over 2^19; the rounding plateau is refused by the same rule
    ratio = {}
    for tag in ("under", "at", "over"):
        gs = oc.sorted_distinct(oc.grid32("ratio_" + tag)).astype(np.float64)
        gaps = np.diff(gs)
        ratio[tag] = gaps.max() / gaps.min()
    assert ratio["under"] < 2.0 ** 19 == ratio["at"] < ratio["over"] and ratio["over"] / ratio["under"] < 1 + 1e-6
    assert oc.fastlim_of(oc.grid32("ratio_under")) > 0 and oc.fastlim_of(oc.grid32("ratio_at")) > 0
    assert oc.fastlim_of(oc.grid32("ratio_over")) == 0 and oc.fastlim_of(oc.grid32("plateau")) == 0
    assert all(oc.fastlim_of(oc.grid32(k)) == 0 for k in ("m257_sorted", "m1024_sorted", "nan_entry", "inf_entry"))
    assert all(oc.fastlim_of(oc.grid32(k)) > 0 for k in ("m65_sorted", "m128_sorted", "m255_sorted", "m256_sorted", "m2"))


@pytest.mark.parametrize("name", oc.BOOK_GRIDS)
def test_every_midpoint_window_of_a_book_holds_two_indices(oracle, name, capsys):
    g64 = oc.nearest_grids()[name]
    g = g64.astype(np.float32)
    case = oc.nearest_case(g)
    _, idx = _nearest(oracle, case["x"], g)
    good, total = oc.windows_with_two(idx, case["mids"]), case["mids"].shape[0]
    assert total == oc.sorted_distinct(g).size - 1 and good == total, (name, good, total)
    c64 = oc.nearest_case_f64(g64)
    with np.errstate(all="ignore"):
        narrowed = c64["x"].astype(np.float32)
    two = oc.windows_with_two(narrowed.view(np.uint32), c64["triples"])
    assert c64["triples"].shape[0] == 2 * total and two == 2 * total, (name, two)
    with capsys.disabled():
        print("\n%s: %d/%d midpoint windows hold two indices, %d/%d narrowing triples two floats, %d exact ties"
              % (name, good, total, two, 2 * total, case["ties"].size))


def test_ties_of_duplicate_and_unsorted_grids_go_to_the_later_scan_index(oracle):
    for name, want_idx, want_z in (("m3_dup_lower", 2, 1.0), ("m3_dup_upper", 2, 3.0)):
        g = oc.grid32(name)
        case = oc.nearest_case(g)
        z, idx = _nearest(oracle, case["x"], g)
        assert case["ties"].size == 1 and case["x"][case["ties"][0]] == 2.0
        assert idx[case["ties"][0]] == want_idx and z[case["ties"][0]] == want_z, name
    # without the duplicate the same tie goes the other way
    assert _nearest(oracle, np.float32([2.0]), np.float32([1.0, 3.0]))[0][0] == 3.0
    assert _nearest(oracle, np.float32([2.0]), np.float32([3.0, 1.0]))[0][0] == 1.0
    for name in ("m63_unsorted", "m64_unsorted", "zeros_unsorted", "zeros_pn", "zeros_np"):
        g = oc.grid32(name)
        case = oc.nearest_case(g)
        z, idx = _nearest(oracle, case["x"], g)
        for at in case["ties"]:
            d = np.abs(case["x"][at] - g)
            assert idx[at] == np.flatnonzero(d == d.min())[-1]
    # the sign of a zero output is that of the LAST zero in scan order
    for name, neg in (("zeros_pn", True), ("zeros_np", False), ("zeros_unsorted", False)):
        g = oc.grid32(name)
        z, _ = _nearest(oracle, np.float32([0.0, -0.0, 1e-3, -1e-3]), g)
        assert (z == 0).all() and (np.signbit(z) == neg).all(), name


@pytest.mark.parametrize("name", sorted(oc.nearest_grids()))
def test_horizon_windows_hold_an_index_and_none(oracle, name):
    g64 = oc.nearest_grids()[name]
    g = g64.astype(np.float32)
    case = oc.nearest_case(g)
    z, idx = _nearest(oracle, case["x"], g)
    assert case["horizon"].shape == (2, oc.WIN)
    v = idx[case["horizon"]]
    assert ((v == oracle.IDX_NONE).any(1) & (v >= 0).any(1)).all(), (name, v)
    # no expected output holds a poison pattern
    assert not (z.view(np.uint32) == oc.POISON32).any() and not (idx == oc.POISON_IDX).any()
    z64, _ = _nearest(oracle, oc.nearest_case_f64(g64)["x"], g64)
    assert not (z64.view(np.uint64) == oc.POISON64).any()


@pytest.mark.parametrize("k", oc.AFFINE_K)
def test_affine_tie_windows_hold_two_levels(oracle, k, capsys):
    rng = np.random.default_rng(400 + k)
    ranges = oc.random_ranges(rng, 64)
    case = oc.affine_case(rng, k, ranges, 1028)
    with np.errstate(all="ignore"):
        out, q = oracle.affine(case["x"], k, case["xmin"], case["xmax"])
    inner = oc.affine_inner(case, k)
    qw = q.reshape(-1)[case["windows"]]
    rows_of = np.repeat(np.arange(ranges.shape[0]), case["x"].shape[0] // ranges.shape[0])
    two = qw.max(1) != qw.min(1)
    share = two[inner].mean()
    with capsys.disabled():
        print("\nk = %d: %.2f %% of %d inner tie windows hold two levels" % (k, 100 * share, int(inner.sum())))
    assert inner.sum() >= 64 * min(150, (1 << k) - 1) and share >= 0.95, (k, share)
    if k <= 8:
        half = 1 << (k - 1)
        for r in range(ranges.shape[0]):
            got = np.unique(q[rows_of == r][~np.isnan(case["x"][rows_of == r])])
            assert np.array_equal(got, np.arange(-half, half)), (k, r)
    assert not (out.view(np.uint32) == oc.POISON32).any() and not (q == oc.POISON_Q).any()
    # the special ranges reach what they are there for
    sp = oc.special_ranges(k)
    scale = np.float32([oc.affine_params(k, a, b)[0] for a, b in sp])
    zp = np.float32([oc.affine_params(k, a, b)[1] for a, b in sp])
    assert np.isnan(scale).sum() == 2 and (zp == np.float32(1 << (k - 1))).any()          # NaN ranges; min = 0: num == 0 occurs
    big = np.isfinite(zp) & (np.abs(zp) > 2.0 ** 60)                                       # min = 1e20: true division
    assert big.any() and ((2.0 ** -40 <= scale[big]) & (scale[big] <= 2.0 ** 40)).all() == (k <= 8)
    for edge in (2.0 ** -40, 2.0 ** 40):
        d = scale.view(np.uint32).astype(np.int64) - int(np.float32(edge).view(np.uint32))
        if edge < 1 or k == 24:
            assert (d == 0).any() or ((d < 0) & (d > -8)).any() and ((d > 0) & (d < 8)).any(), (k, edge, d)


@pytest.mark.parametrize("name", oc.F64_BOOKS)
def test_f64_threshold_windows_and_pairs(antq_lib, oracle, name, capsys):
    bk = oc.f64_book(name)
    _, g, gmax, nn, ovp = bk
    h = _header(antq_lib, g)
    assert (oc.plan_class(h) == "scan") == (name == "scan_list")
    alphas = oc.F64_ALPHAS_8BIT if g.size > 64 else oc.F64_ALPHAS
    case = oc.f64_case(bk, h, alphas)
    assert (case["alpha"].astype(np.float32).astype(np.float64) != case["alpha"])[np.isfinite(case["alpha"]) & (case["alpha"] != 0)].all()
    out, idx, victim = oc.f64_forward_parts(oracle, case["x"], case["alpha"], g, gmax, False, True)
    n_thr = oc.sorted_distinct(g).size - 1
    usable = int((np.isfinite(case["alpha"]) & (case["alpha"] != 0)).sum())
    assert case["windows"].shape[0] == usable * 2 * n_thr
    two = oc.windows_with_two(idx, case["windows"])
    with capsys.disabled():
        print("\n%s: %d of %d float64 threshold windows hold two indices" % (name, two, case["windows"].shape[0]))
    assert 2 * two >= case["windows"].shape[0]
    assert not (out.view(np.uint64) == oc.POISON64).any()
    if not ovp:
        return
    pc = oc.f64_pair_case(bk)
    seen = oc.pair_forms_present(oc.F64Decisions(oracle), pc, g, gmax, nn)
    assert seen == {(f, p) for f in range(4) for p in range(4)}, sorted(seen)
    # both odd-count wrap cases, by the restatement's victim mask
    for shape, per_row in ((oc.ODD_SHAPES[0], True), (oc.ODD_SHAPES[1], False), (oc.ODD_SHAPES[1], True)):
        for first in (True, False):
            c = oc.f64_odd_case(bk, shape, first, per_row)
            assert c["x"].size % 2 == 1
            _, idx, victim = oc.f64_forward_parts(oracle, c["x"], c["alpha"], g, gmax, True, per_row)
            if first:
                assert idx[0] >= nn and 0 <= idx[-1] < nn and victim[-1]
            else:
                assert 0 <= idx[0] < nn and idx[-1] >= nn and not victim[-1]


def test_plan_classes_and_altered_grids(antq_lib, oracle):
    want = dict(small="small", big_linear="big", big="big", scan="scan")
    for key, gname in oc.PLAN_GRIDS.items():
        g = oc.grid32(gname)
        h = _header(antq_lib, g)
        assert oc.plan_class(h) == want[key] and h["m"] == g.size, (key, oc.plan_class(h))
        assert (h["kind"] == oc.PLAN_TABLE) == antq_lib.plan_for(g).is_table
        case = oc.plan_case(g, h)
        assert case["x"].size % 8 == 0 and case["n_mixed"] % 4 == 0
        # a window at EVERY bucket edge of the plan's table, its centre the edge itself
        edges = oc.bucket_edges(h)
        assert case["edges"].shape == (edges.size, oc.WIN) and np.array_equal(case["x"][case["edges"][:, oc.ULPS]], edges), key
        mv = case["x"][:case["n_mixed"]].reshape(-1, 4)
        lim = h["fastlim"] if h["fastlim"] > 0 else oc.HORIZON
        with np.errstate(all="ignore"):
            beyond = ~(np.abs(mv) < lim)
        assert (beyond.sum(1) == 1).all() and set(np.argmax(beyond, 1)) == {0, 1, 2, 3}
        alt = oc.altered_grids(g)
        assert len(alt) == (6 if g.size > 256 else 4 if (g == 0).any() else 3), (key, [t for t, _ in alt])
        for tag, a in alt:
            assert (a.view(np.uint32) != g.view(np.uint32)).sum() == 1, (key, tag)
            # the inputs at the front of the hinted test tell the two grids apart: a kernel that kept the plan's grid would fail
            front = oc.altered_front(g, a)
            assert front.size % 8 == 0
            (z0, j0), (z1, j1) = _nearest(oracle, front, g), _nearest(oracle, front, a)
            assert (z0.view(np.uint32) != z1.view(np.uint32)).any() or (j0 != j1).any(), (key, tag)
