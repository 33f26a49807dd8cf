"""The input builders of the 16-bit dynamic edge tests (dynamic16_cases.py) against the CPU oracle alone, no GPU: every planted
maximum is the strict maximum of its row and taking it away changes both the oracle's scale and the oracle's outputs; the
pattern rows reach every entry of a signed book, the outliers, the victims and the far-clipped region; and every restated
mistake in taking the abs-max changes the oracle's output of at least one row of the case set.  A failure of
test_gpu_dynamic16_edges.py is then the kernels', not the inputs'."""
import numpy as np
import pytest

import dynamic16_cases as dc
import fakequant_cases as fc


def _header(antq_lib, g):
    return fc.plan_header(antq_lib.plan_for(g).host)


def test_row_lengths_sit_at_every_boundary_of_the_launch_shapes():
    """1, 4 and 16 wavefronts per row, every number of vector steps from 2 to 8 at both ends, a last wavefront with nothing to
    do (513: 3 of 4 in use; 2049: 11 of 16), and the three shapes of the two-pass fall-back"""
    shapes = {v: dc.shape_of(v) for v in dc.VPRS if v >= 128}
    assert {s[0] for s in shapes.values()} == {1, 4, 16}
    for nv in range(3, 9):
        assert shapes[64 * (nv - 1) + 1] == (1, nv) and shapes[64 * nv] == (1, nv)
    assert shapes[128] == (1, 2) and shapes[513] == (4, 3) and shapes[2048] == (4, 8) and shapes[2049] == (16, 3) and shapes[8192] == (16, 8)
    assert -(-513 // (64 * 3)) == 3 and -(-2049 // (64 * 3)) == 11
    assert {1, 2, 16, 64} <= set(dc.VPRS) and all(v & (v - 1) == 0 for v in dc.GROUPS["lane"])
    assert [s[1:] for s in dc.FALLBACK] == [(8 * 8193, 0), (8 * 129 + 3, 0), (8 * 128, 1)]
    # the positions: lane 0 and lane 63 of the first and of the (partially filled) last vector step, first / middle / last wavefront
    assert dc.vector_positions(129) == [0, 63, 128]
    assert dc.vector_positions(512) == [0, 63, 448, 511]
    assert dc.vector_positions(513) == [0, 63, 128, 191, 192, 255, 320, 383, 384, 447, 512]
    assert dc.vector_positions(8192) == [0, 63, 448, 511, 4096, 4159, 4544, 4607, 7680, 7743, 8128, 8191]
    assert max(dc.vector_positions(2049)) == 2048 and 1920 in dc.vector_positions(2049)


@pytest.mark.parametrize("dtype_name", dc.DTYPES)
@pytest.mark.parametrize("name", dc.BOOKS)
def test_every_planted_maximum_decides_scale_and_outputs(oracle, name, dtype_name):
    """For 100 % of the planted rows, at every row length: the planted element(s) hold the strict maximum; zeroing them changes
    oracle.absmax of the row and at least one element of oracle.forward of the row."""
    bk = dc.book(name)
    n_rows = 0
    for label, rl, lead in dc.ALL_SHAPES:
        case = dc.planted_case(dtype_name, rl)
        x, planted = case["x"], case["planted"]
        assert x.shape == (len(planted), rl) and x.shape[0] >= 5
        mag = dc.widen16(oracle, x & 0x7fff, dtype_name)
        m = dc.value(oracle, case["m16"], dtype_name)
        z = x.copy()
        for r, ps in enumerate(planted):
            others = np.ones(rl, bool)
            others[list(ps)] = False
            assert (mag[r, list(ps)] == m[r]).all() and (mag[r, others] <= m[r] / 4).all(), (label, r)
            z[r, list(ps)] = 0
        a, out, _ = dc.reference(oracle, x, dtype_name, bk)
        az, outz, _ = dc.reference(oracle, z, dtype_name, bk)
        assert np.array_equal(a, m) and (az != a).all(), label
        changed = (~dc.same16(oracle, out, outz, dtype_name)).any(axis=1)
        assert changed.all(), (label, np.flatnonzero(~changed).tolist())
        # rows of both signs: the row with +M and -M, and the one whose only maximum is negative
        assert len(planted[-2]) == (2 if rl >= 2 else 1) and (x[-1, planted[-1][0]] & 0x8000)
        n_rows += x.shape[0]
    print("planted rows held to their conditions:", name, dtype_name, n_rows)


@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_magnitude_rows_have_the_scales_they_were_built_for(oracle, dtype_name):
    F = dc.FMT[dtype_name]
    for vpr in dc.MAG_VPRS:
        case = dc.magnitude_case(dtype_name, vpr)
        x = case["x"]
        assert x.shape == (len(dc.MAG_ROWS), 8 * vpr)
        a = oracle.absmax(dc.widen16(oracle, x, dtype_name), True, 1.0)
        want = dc.value(oracle, case["m16"], dtype_name)
        assert dc.same32(a, want).all(), (vpr, a, want)
        assert np.isnan(a[[7, 10, 11]]).all() and np.isinf(a[[8, 9]]).all() and a[6] == 0 and (a[:6] > 0).all()
        assert a[2] == dc.value(oracle, [F["max"]], dtype_name)[0] and a[5] == dc.value(oracle, [1], dtype_name)[0]
        # NaN and Inf of the two-special rows sit in different wavefronts (different vectors of a lane group)
        wpr, nv = dc.shape_of(vpr)
        for r in (10, 11):
            p, q = case["planted"][r]
            assert p // 8 != q // 8 and (wpr == 1 or p // (512 * nv) != q // (512 * nv))
    # ratios: alpha underflows for some rows with the smallest ratio, and rounds to zero for others
    a = oracle.absmax(dc.widen16(oracle, dc.magnitude_case(dtype_name, 128)["x"], dtype_name), True, dc.RATIOS[-1])
    assert ((a > 0) & (a < np.float32(2.0 ** -126))).any() and (a[3:6] == 0).all()


def _counts(oracle, x, dtype_name, bk, h, ratio, pair):
    _, g, gmax, nn, ovp = bk
    a, out, idx = dc.reference(oracle, x, dtype_name, bk, ratio, pair)
    xf = dc.widen16(oracle, x, dtype_name).astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(xf) / (a.astype(np.float32) / np.float32(gmax)).astype(np.float64)[:, None]
    lim = min(h["fastlim"] * 0.99999, h["xlim"])
    return dict(entries=int(np.unique(idx[idx >= 0]).size), outliers=int((idx >= nn).sum()) if nn else 0,
                victims=int((idx == oracle.IDX_VICTIM).sum()), far=int((d >= lim).sum()),
                inf=int(np.isinf(dc.widen16(oracle, out, dtype_name)).sum()))


@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_pattern_rows_reach_every_entry_outliers_victims_and_the_far_region(antq_lib, oracle, dtype_name):
    """Per row set (the one long row, and the rows of 128 / 512 / 2048 vectors).  An ordinary M and ratio 1: the oracle's
    indices cover every entry of a signed book.  Ratio 0.25: the ANT books have far-clipped elements (|x / s| beyond the
    table's limit); the OliVe book with the pair rule has outlier outputs and victims -- its table reaches 24 * gmax, which
    no element of a row with alpha = max / 4 does, so its far-clipped elements come with the ratio 2^-5, where it still has
    outliers and victims.  f16, largest finite M: at least one oracle output is +/-Inf."""
    for name in dc.BOOKS:
        bk = dc.book(name)
        _, g, gmax, nn, ovp = bk
        h = _header(antq_lib, g)
        for top in dc.PATTERN_TOPS:
            for k, x in enumerate(dc.pattern_case(dtype_name, top)):
                c1 = _counts(oracle, x, dtype_name, bk, h, 1.0, None)
                c4 = _counts(oracle, x, dtype_name, bk, h, 0.25, None)
                tag = (name, dtype_name, top, k)
                distinct = np.unique(g + np.float32(0))
                if top != "max" and g.min() < 0:
                    # (with ratio 1 no quotient leaves [-gmax, gmax]: int-4's -8 / 7 * gmax and the outliers need the smaller ratios)
                    assert c1["entries"] == int((np.abs(distinct) <= gmax).sum()), (tag, c1)
                    c_small = c4 if not ovp else _counts(oracle, x, dtype_name, bk, h, dc.PAIR_FAR_RATIO, None)
                    # (M a few binades above the smallest normal: at 2^-5 the inner entries fall between bf16's subnormals)
                    assert c_small["entries"] == distinct.size or (ovp and top == "low"), (tag, c_small)
                if ovp:
                    c32 = _counts(oracle, x, dtype_name, bk, h, dc.PAIR_FAR_RATIO, None)
                    assert c4["outliers"] > 0 and c4["victims"] > 0 and c4["far"] == 0, (tag, c4)
                    assert c32["outliers"] > 0 and c32["victims"] > 0 and c32["far"] > 0, (tag, c32)
                    assert _counts(oracle, x, dtype_name, bk, h, 0.25, False)["victims"] == 0
                else:
                    assert c4["far"] > 0, (tag, c4)
                    c32 = None
                assert dc.pattern_ratios(top, ovp) == (1.0, 0.25) + ((dc.PAIR_FAR_RATIO,) if ovp else ()) + ((dc.OVERFLOW_RATIO,) if top == "max" else ())
                if dtype_name == "float16" and top == "max":
                    # (ratio <= 1: no output exceeds gmax * s <= M, none is Inf; the row set is also run with 1.0625)
                    assert c1["inf"] == 0 and _counts(oracle, x, dtype_name, bk, h, dc.OVERFLOW_RATIO, None)["inf"] > 0, (tag, c1)
                if k == 0:
                    print("pattern rows", tag[:3], "elements", x.size, "ratio 1:", c1, "ratio 0.25:", c4, "ratio 2^-5:", c32)


@pytest.mark.parametrize("dtype_name", dc.DTYPES)
def test_every_restated_mistake_changes_an_output(oracle, dtype_name):
    """Each wrong abs-max of dynamic16_cases.MISTAKES, restated in numpy, gives at least one row of the case set (planted rows
    at ratio 1, magnitude rows at every ratio) an oracle output that differs from out_ref: a kernel that made it would fail."""
    bk = dc.book("flint_b4_s")
    gmax = bk[2]
    caught = {k: 0 for k in dc.MISTAKES}
    sets = [(dc.planted_case(dtype_name, rl)["x"], 1.0) for _, rl, _ in dc.ALL_SHAPES if rl <= 8 * 2049]
    sets += [(dc.magnitude_case(dtype_name, vpr)["x"], r) for vpr in dc.MAG_VPRS[:4] for r in dc.RATIOS]
    for x, ratio in sets:
        _, out_ref, _ = dc.reference(oracle, x, dtype_name, bk, ratio)
        for kind in dc.MISTAKES:
            a = dc.mistaken_alpha(oracle, kind, x, dtype_name, ratio, gmax)
            if a is None:
                continue
            out = dc.forward16(oracle, x, dtype_name, bk, a)
            caught[kind] += int((~dc.same16(oracle, out, out_ref, dtype_name)).any(axis=1).sum())
    print("rows that tell each mistake from the right abs-max:", dtype_name, caught)
    for kind, n in caught.items():
        if kind == "f16 subnormal as zero" and dtype_name != "float16":
            continue
        assert n > 0, (kind, caught)
