"""The input builders of the fp32 fake-quant edge tests (fakequant_cases.py) against the CPU oracle alone, no GPU: every
threshold window straddles a decision for every book, row length and scale set the GPU tests use, the pair layouts hold every
(form, position), the windows at the end of the exact straight-through step hold both kinds of element, the dynamic case's
planned scales are the oracle's abs-max scales, and the plan-header helper agrees with Plan.  A failure of
test_gpu_fakequant_edges.py is then the kernels', not the inputs'."""
import numpy as np
import pytest

import encode4_cases as ec
import fakequant_cases as fc

HOST_ROW_LENS = fc.ROW_LENS


def _header(antq_lib, g):
    return fc.plan_header(antq_lib.plan_for(g).host)


@pytest.mark.parametrize("name", fc.BOOK_NAMES)
def test_every_threshold_window_straddles_a_decision(antq_lib, oracle, name):
    """Every row length of the GPU test (the per-tensor and ragged ones included: they reuse these scale sets), 64 scales (16
    for the 8-bit books) with the short-mantissa scales and the six around s = 2^-40 / 2^40 among them."""
    _, g, gmax, nn, ovp = fc.book(name)
    h = _header(antq_lib, g)
    n_mid = int(ec.centres(g, 1.0)[0].size)
    for rl in HOST_ROW_LENS + fc.RAGGED_ROW_LENS + (4099,):
        case = fc.static_case(oracle, name, h, rl)
        good, total = fc.windows_straddle(oracle, case, g, gmax)
        assert total == fc.n_scales_of(g) * n_mid and good == total, (name, rl, good, total)
        assert case["x"].shape[1] == rl
        # the scales that were asked for are there: fl(alpha / gmax) with a short mantissa, and the floats around 2^-40 / 2^40
        s = np.unique((case["alpha"] / np.float32(gmax)).astype(np.float32))
        mant = s.view(np.uint32) & 0x7fffff
        assert np.isin(mant, [0, 0x400000, 0x200000, 0x600000]).sum() >= min(6, fc.n_scales_of(g) // 3), (name, rl)
        for edge in fc.OK_EDGES:
            k = s.view(np.uint32).astype(np.int64) - int(np.float32(edge).view(np.uint32))
            if fc.n_scales_of(g) >= 16:
                assert (k == 0).any() and ((k < 0) & (k >= -4)).any() and ((k > 0) & (k <= 4)).any(), (name, rl, edge)
            else:
                assert (np.abs(k) <= 4).any(), (name, rl, edge)


@pytest.mark.parametrize("name", fc.OLIVE_NAMES)
def test_all_pair_forms_at_all_positions(oracle, name):
    _, g, gmax, nn, ovp = fc.book(name)
    for rl in fc.PAIR_ROW_LENS:
        case = fc.pair_case(np.random.default_rng(17), g, gmax, nn, rl, n_scales=16)
        seen = ec.pair_forms_present(oracle, case, g, gmax, nn)
        assert seen == {(f, p) for f in range(4) for p in range(4)}, (name, rl, sorted(seen))
        with np.errstate(all="ignore"):
            _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, True)
        assert (ridx == oracle.IDX_VICTIM).any() and (ridx >= nn).any()


# Books whose every value v is a multiple of ulp(d) for every d the scan can reach (|d| < 102400): (v - d) + d is then v
# exactly, at +/-2 v and far beyond, so there is NO element whose output differs from fl(q * s).  After the normalisation to a
# largest value of 10 (ANT) or 32 (OliVe) these books' values are short dyadic numbers; only the int books with a negative
# end of -2^(b-1) * fl(10 / (2^(b-1) - 1)) carry a full mantissa.
NO_STE_EDGE = ("flint_b4_s", "pot_b4_s", "flint_b4_u", "int_b3_u", "olive_flint", "olive_int", "int_b8_u", "flint_b8_s", "flint_b6_s",
               "float_b5_s", "olive_int_b8", "olive_flint_b8")


def test_windows_where_the_straight_through_step_stops_being_exact(antq_lib, oracle):
    """The windows at +/-2 * (outermost value) * s sit where the kernels stop relying on (q - d) + d == q (xlim).  In the
    oracle's own arithmetic the identity holds there for every book of the set (all of these windows hold only elements with
    output fl(q * s): asserted), so the elements whose output is NOT fl(q * s) are planted where the identity really ends,
    found per scale by bisection (ste_edges): every such window holds both kinds.  Only int_b4_s and int_b8_s have such an
    end inside the scan's horizon; the books without one are named (NO_STE_EDGE), each shown to have none on a dense sweep of
    its clipped region, and nothing else may be left out."""
    left_out = []
    for name in fc.BOOK_NAMES:
        _, g, gmax, nn, ovp = fc.book(name)
        h = _header(antq_lib, g)
        for rl in (72, 4004):
            case = fc.static_case(oracle, name, h, rl)
            mixed, total = fc.windows_mixed(oracle, case, g, gmax, "ste")
            assert mixed == total, (name, rl, mixed, total)
            lit_mixed, lit_total = fc.windows_mixed(oracle, case, g, gmax, "outer")
            assert lit_total > 0 and lit_mixed == 0, (name, rl, lit_mixed, lit_total)
            if total == 0 and rl == 72:
                left_out.append(name)
                # nothing to find: a log sweep of both clipped regions, 2 |v| s .. the far end of the search, 4096 points a sign
                a = np.unique(case["alpha"])
                a = a[(a > 1e-20) & (a < 1e20)][:8]
                top = np.float64([2 * g.max(), 2 * g.min()] if g.min() < 0 else [2 * g.max()])
                d = np.concatenate([np.sign(t) * np.exp(np.linspace(np.log(abs(t)), np.log(fc.STE_FAR_D), 4096)) for t in top])
                x = (d[None, :] * (a[:, None].astype(np.float64) / gmax)).astype(np.float32)
                assert fc._output_is_qs(oracle, x, a, g, gmax).all(), name
            elif rl == 72:
                assert total >= fc.n_scales_of(g) // 2, (name, total)
    print("books without an end of the exact straight-through step inside the scan's horizon:", left_out)
    assert tuple(left_out) == tuple(n for n in fc.BOOK_NAMES if n in NO_STE_EDGE), left_out


@pytest.mark.parametrize("name", fc.BOOK_NAMES)
def test_per_tensor_scale_sets_straddle(antq_lib, oracle, name):
    """The one-scale cases the per-tensor GPU test cuts its tensors from: every threshold window straddles a decision"""
    _, g, gmax, nn, ovp = fc.book(name)
    cases = fc.per_tensor_cases(oracle, name, _header(antq_lib, g))
    assert len(cases) == 3
    for a, c72, c4099 in cases:
        for case in (c72, c4099):
            good, total = fc.windows_straddle(oracle, case, g, gmax)
            assert total == int(ec.centres(g, np.float32(a) / np.float32(gmax))[0].size) > 0 and good == total, (name, float(a), good, total)


@pytest.mark.parametrize("name", ["flint_b4_s", "int_b4_s", "olive_flint", "int_b8_s", "flint_b8_s", "olive_int_b8"])
def test_dynamic_case_scales_are_known_before_the_launch(antq_lib, oracle, name):
    """The planned alpha of every row is oracle.absmax(x, True, ratio); every row holds its maximum exactly once and nothing
    at or beyond it; the smaller ratio brings windows beyond gmax * s in."""
    _, g, gmax, nn, ovp = fc.book(name)
    h = _header(antq_lib, g)
    for vpr in fc.DYN_VPR:
        for ratio in fc.DYN_RATIOS:
            case = fc.dynamic_case(oracle, name, h, vpr, ratio)
            x, a = case["x"], case["alpha"]
            assert x.shape[1] == 4 * vpr and 3 <= x.shape[0] and np.isfinite(x).all()
            assert np.array_equal(oracle.absmax(x, True, ratio), a), (name, vpr, ratio)
            assert ((np.abs(x) == case["absmax"][:, None]).sum(1) == 1).all() and (np.abs(x) <= case["absmax"][:, None]).all()
            # every window below the row's maximum is there and straddles (one may have lost an element to a planted maximum)
            good, total = fc.windows_straddle(oracle, case, g, gmax)
            assert total > 0 and good == total, (name, vpr, ratio, good, total)
            if ratio < 1 and not ovp:
                assert len(case["outer"]) > 0, (name, vpr)
    assert 0 < fc.DYN_RATIOS[1] < 1 and fc.DYN_RATIOS[0] == 1.0 and (np.float32(fc.DYN_RATIOS[1]).view(np.uint32) & 0xfff) != 0


def test_header_helper_agrees_with_plan(antq_lib):
    """m, kind and n_entries as Plan and antq_plan_bytes see them, for every book; the bucket edges lie inside the table."""
    L = antq_lib.lib()
    for name in fc.BOOK_NAMES:
        _, g, gmax, nn, ovp = fc.book(name)
        plan = antq_lib.plan_for(g)
        h = fc.plan_header(plan.host)
        assert h["m"] == g.size == plan.grid.size and h["m_pad"] == (g.size + 3) // 4 * 4, name
        assert h["kind"] == plan.kind == int(L.antq_plan_kind(plan.host_ptr())) and (h["kind"] == fc.PLAN_TABLE) == plan.is_table, name
        assert h["bytes"] == plan.host.size, name
        assert h["n_entries"] == h["nb"] + h["nbneg"] and h["nb"] == h["kmax"] - h["kmin"] + 1, name
        # the blob holds the header, the grid, n_entries 16-byte entries (and, behind them, what the other paths need)
        assert h["bytes"] >= 128 + 4 * h["m_pad"] + 16 * h["n_entries"], name
        e = fc.bucket_edges(h)
        assert e.size == (h["kmax"] if h["linear"] else (h["nb"] - 1) * (2 if h["nbneg"] else 1)), (name, e.size)
        assert np.all(np.diff(e) > 0) and np.isfinite(e).all(), name
        assert h["xdom"] in (0, 1) and h["adom"] in (0, 1) and 0 < h["xlim"] <= 2 * float(np.abs(g).max()), name
    # the set holds every plan form the kernels distinguish: x-domain tables, linear keys, keyed tables with and without adom
    forms = {(h["xdom"], h["linear"], h["adom"]) for h in (_header(antq_lib, fc.book(n)[1]) for n in fc.BOOK_NAMES)}
    assert forms >= {(1, 0, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0)}, forms


def test_pattern_rows_hold_every_pattern_once_per_scale():
    for rl in (16, 72, 4096):
        x, a = fc.pattern_rows(rl, np.random.default_rng(1))
        assert x.shape[1] == rl and x.shape[0] == a.size and a.size % 8 == 0
        per = x.reshape(8, -1)
        assert all(np.array_equal(np.sort(per[k][:65536]), np.arange(65536)) for k in range(8))
        assert np.array_equal(a.reshape(8, -1)[:, 0].view(np.uint32), fc.PATTERN_ROW_SCALES.view(np.uint32))
