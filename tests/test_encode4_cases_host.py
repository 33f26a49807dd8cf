"""The input builders of the packed 4-bit encoder's edge tests (encode4_cases.py) against the CPU oracle alone: every planted
window straddles a decision, the pair layouts hold every (form, position), the IDX_NONE bisection converged, the fuzz books are
well-formed, every special value is present.  A failure of test_gpu_encode4_edges.py is then the kernels', not the inputs'."""
import numpy as np
import pytest

import encode4_cases as ec

ROW_LENS = (504, 520, 1032)


@pytest.mark.parametrize("name", ec.BOOK_NAMES)
def test_every_window_straddles_a_decision(oracle, name):
    _, g, gmax, nn, ovp = ec.book(name)
    n_mid = int((ec.centres(g, 1.0)[0]).size)
    for rl in ROW_LENS:
        case = ec.threshold_case(np.random.default_rng(99), g, gmax, rl)
        good, total = ec.windows_straddle(oracle, case, g, gmax)
        assert total == 64 * n_mid and good == total, (name, rl, good, total)
        assert case["x"].shape[1] == rl and case["x"].shape[0] % 64 == 0
    # one scale for the whole tensor
    for a in ec.awkward_alpha(np.random.default_rng(5), 3):
        case = ec.threshold_case(np.random.default_rng(7), g, gmax, 2080, n_scales=1, alpha=[a])
        good, total = ec.windows_straddle(oracle, case, g, gmax)
        assert good == total == n_mid, (name, float(a))


def test_window_counts_of_the_reference_books():
    counts = [64 * ec.centres(b[1], 1.0)[0].size for b in ec.books()]
    assert counts == [896, 960, 896, 960, 448, 1792, 1792]


@pytest.mark.parametrize("name", ["olive_flint", "olive_int"])
def test_all_pair_forms_at_all_positions(oracle, name):
    _, g, gmax, nn, ovp = ec.book(name)
    mids, edge = ec.midpoints(g)
    assert edge.sum() == 2 and mids[edge][0] == -mids[edge][1]
    for rl in ROW_LENS:
        case = ec.pair_case(np.random.default_rng(17), g, gmax, nn, rl)
        seen = ec.pair_forms_present(oracle, case, g, gmax, nn)
        assert seen == {(f, p) for f in range(4) for p in range(4)}, (name, rl, sorted(seen))
        # a member of every listed pair lies within 16 ulps of a boundary centre of its row's scale
        x, a = case["x"].reshape(-1), case["alpha"]
        for at, pos in case["pairs"][::37]:
            s = np.float32(a[at // rl]) / np.float32(gmax)
            c, e = ec.centres(g, s)
            near = np.concatenate([ec.ulp_window(v) for v in c[e]])
            assert np.isin(x[at:at + 2], near).any(), (name, rl, int(at))
        # with the pair rule on there are victims and outliers
        with np.errstate(all="ignore"):
            _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, True)
        assert (ridx == oracle.IDX_VICTIM).any() and (ridx >= nn).any()


@pytest.mark.parametrize("name", ec.BOOK_NAMES)
def test_magnitudes_specials_and_the_none_edge(oracle, name):
    _, g, gmax, nn, ovp = ec.book(name)
    case = ec.magnitude_case(oracle, np.random.default_rng(3), g, gmax, 1032)
    x = case["x"].reshape(-1)
    assert len(case["edges"]) == len(ec.ROW_SCALES) == 10
    with np.errstate(all="ignore"):
        _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, False)
    ridx = ridx.reshape(-1)
    for i, (st, ln) in enumerate(case["spans"]):
        bits = x[st:st + ln].view(np.uint32)
        # both signs of all 255 finite exponents (0 = denormals), every mantissa; the specials
        for sign in (0, 0x80000000):
            have = set(((bits[(bits & 0x80000000) == sign] >> 23) & 0xff).tolist())
            assert have >= set(range(255)), (name, i)
        for m in ec.MANTISSAS:
            assert ((bits & 0x7fffff) == m).sum() >= 2 * 254
        assert np.isin(ec.SPECIALS.view(np.uint32), bits).all(), (name, i)
        a = ec.ROW_SCALES[i]
        for sign in (1, -1):
            ed = case["edges"][i][sign]
            if np.isfinite(a) and a > 0:
                assert ed is not None, (name, float(a), sign)       # an ordinary scale has the edge, and the bisection found it
            if ed is not None:
                lo, hi = ed
                assert hi.view(np.uint32) - lo.view(np.uint32) == 1
                w = ec.ulp_window(hi * np.float32(sign)).view(np.uint32)
                assert np.isin(w, bits).all()
                sel = np.isin(bits, w)
                got = ridx[st:st + ln][sel]
                assert (got == oracle.IDX_NONE).any() and (got != oracle.IDX_NONE).any(), (name, float(a), sign)
    # the scales whose every element is beyond the scan: nothing but IDX_NONE
    assert sum(e[1] is None and e[-1] is None for e in case["edges"]) >= 2


@pytest.mark.parametrize("name", ec.BOOK_NAMES)
def test_split_octets(oracle, name):
    _, g, gmax, nn, ovp = ec.book(name)
    for rl in (520, 1032):
        case = ec.split_octet_case(np.random.default_rng(29), g, gmax, rl)
        x = case["x"].reshape(-1)
        far = set(ec.FAR.view(np.uint32).tolist())
        n_full = 0
        for w, s in case["halves"]:
            assert w // 8 == s // 8 and abs(w - s) == 4 and w // rl == s // rl       # one octet, one row
            sp = x[s:s + 4].view(np.uint32)
            assert any(int(b) in far for b in sp) and not any(int(b) in far for b in x[w:w + 4].view(np.uint32))
            n_full += all(int(b) in far for b in sp)
        assert 0 < n_full < len(case["halves"])
        with np.errstate(all="ignore"):
            _, ridx = oracle.forward(case["x"], case["alpha"], g, gmax, False)
        wi = ridx.reshape(-1)[(case["halves"][:, :1] + np.arange(4)).reshape(-1)]
        assert np.unique(wi).size >= np.unique(g).size - 1            # the window halves hold (nearly) every code


def test_shapes_reach_every_form():
    for rows, rl in ec.SHAPES_16:
        assert rl % 8 == 0
    opr = [rl // 8 for _, rl in ec.SHAPES_F32]
    assert any(o & (o - 1) for o in opr) and any(not (o & (o - 1)) for o in opr)
    n = [r * rl for r, rl in ec.SHAPES_F32]
    for want in (ec.TASK - 8, ec.TASK, ec.TASK + 8, 2 * ec.TASK - 8, 3 * ec.TASK):
        assert want in n
    assert -(-ec.LOOP_SHAPE[0] * ec.LOOP_SHAPE[1] // ec.TASK) == 7
    assert -(-ec.BIG_SHAPE[0] * ec.BIG_SHAPE[1] // ec.TASK) == 2049
    # partial last tasks: fp32 rows at / above 512 elements that are no multiple of 512 (2-vector tasks) or 1024 (4-vector)
    assert {(3, 520), (2, 1016), (2, 1032)} <= set(ec.PARTIAL_SHAPES)


@pytest.mark.parametrize("seed", range(ec.fuzz_seeds()))
def test_fuzz_books_are_well_formed(oracle, seed):
    for ovp, rng in ec.fuzz_books_rng(seed):
        g, gmax, nn = ec.random_book(rng, ovp)
        assert ec.book_well_formed(g, gmax, nn, ovp), (seed, ovp, g)
        n_win = n_good = 0
        for (rows, rl), _ in ec.FUZZ_SHAPES:
            case = ec.fuzz_case(rng, g, gmax, rows, rl)
            x = case["x"].reshape(-1)
            assert np.isnan(x).any() and np.isinf(x).any() and (x == 0).any() and (x.view(np.uint32) == 0x80000000).any()
            good, total = ec.windows_straddle(oracle, case, g, gmax)
            n_win, n_good = n_win + total, n_good + good
        # (entries one ulp apart, or closer than 16 ulps of the centre, share a window: most windows still straddle)
        assert n_win > 0 or np.unique(g + np.float32(0)).size < 2, (seed, ovp, g)
        assert n_good >= 0.9 * n_win, (seed, ovp, n_good, n_win)
