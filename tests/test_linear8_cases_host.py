"""The inputs of tests/test_gpu_linear8.py (tests/linear8_cases.py) held to their premises with numpy and the CPU oracle alone:
the exact-sum cases are exact in any order, the one-hot code sets hold what they claim, the tiny scales make subnormal
weights, and the general data's codes hold the pair identifier."""
import numpy as np
import pytest

import byte_codes_cases as bc
import encode4_cases as ec
import linear8_cases as lc


@pytest.mark.parametrize("name,dtype_name", lc.EXACT_CASES)
def test_exact_sum_cases_are_exact_in_any_order(oracle, name, dtype_name):
    """Every term a whole multiple of one power of two and the magnitude sums below 2^24 units (the assertions of the packed
    4-bit linear's exact case), recomputed here from the arrays the GPU test uploads; scales are powers of two times gmax."""
    _, g, gmax, nn, ovp = bc.book(name)
    seen_n, seen_per_row = set(), set()
    for K in lc.EXACT_K:
        per_row, cases = lc.exact_cases_of(oracle, name, K, dtype_name)
        seen_per_row.add(per_row)
        for ns, c in cases:
            N = max(ns)
            assert c["codes"].shape == (N, K) and c["codes"].dtype == np.uint8 and c["x"].shape == (8, K)
            assert c["alpha"].size == (N if per_row else 1)
            s = (c["alpha"] / np.float32(gmax)).astype(np.float32)
            assert np.array_equal(np.exp2(np.round(np.log2(s))), s)
            assert np.abs(c["x"]).max() <= 3 and np.array_equal(c["x"], np.round(c["x"])) and (c["x"][:, 0] != 0).all()
            # the weights are the decoder's rule in this type, and the type holds x and the bias exactly
            W = lc.value(lc.image_ref(oracle, c["codes"], c["alpha"], per_row, name, dtype_name), dtype_name)
            assert np.array_equal(W, c["W"]) and np.abs(c["bias"]).max() <= 8
            lc.assert_exact_premise(c["x"], W, c["bias"])
            assert np.array_equal(c["y"], (c["x"][:, None, :] * W[None, :, :]).sum(-1))
            # the result and every prefix of rows fits the type after ONE rounding: nothing to check, the test rounds the exact sum
            if ovp and N * K >= 1024:
                assert (c["codes"] == bc.IDENT).any()
            seen_n.update(ns)
            # the same arguments give the same arrays (the GPU test builds them again)
            if K == lc.EXACT_K[0]:
                again = lc.exact_cases_of(oracle, name, K, dtype_name)[1][0][1]
                assert np.array_equal(again["codes"], cases[0][1]["codes"]) and np.array_equal(again["x"], cases[0][1]["x"])
    assert seen_n == set(lc.EXACT_N) and seen_per_row == {True, False}
    # K on both sides of one and two steps of both code paths (512 / 1024 elements per step)
    for step, path in ((512, [k for k in lc.EXACT_K if k % 16]), (1024, [k for k in lc.EXACT_K if k % 16 == 0])):
        for edge in (step, 2 * step):
            assert any(k < edge for k in path) and any(edge < k < edge + step for k in path), (step, edge)
    assert {512, 1024, 2048} <= set(lc.EXACT_K)


@pytest.mark.parametrize("name", lc.ONE_HOT_BOOKS)
def test_one_hot_code_sets_hold_every_byte_and_every_pair_form(name):
    _, g, gmax, nn, ovp = bc.book(name)
    no = g.size - nn
    assert [k % 16 == 0 for k in lc.ONE_HOT_K] == [False, True] and all(512 < k < 1024 or 1024 < k < 2048 for k in lc.ONE_HOT_K)
    for K in lc.ONE_HOT_K:
        c = lc.one_hot_codes(name, K).astype(np.int64)
        assert c.shape == (lc.ONE_HOT_N, K) and K % 8 == 0
        for n in range(c.shape[0]):
            assert np.unique(c[n]).size == 256, (name, K, n)
            if not ovp:
                assert (c[n] >= g.size).any() or g.size == 256           # codes beyond the book, where a byte can hold one
                continue
            lo, hi = c[n].reshape(-1, 2)[:, 0], c[n].reshape(-1, 2)[:, 1]
            assert ((lo == 255) & (hi != 255)).any() and ((hi == 255) & (lo != 255)).any() and ((lo == 255) & (hi == 255)).any()
            for idx in (0, no - 1):                                       # both ends of the outlier list, on either side
                assert ((lo == 255) & (hi == idx)).any() and ((hi == 255) & (lo == idx)).any(), (name, K, n, idx)
            if no < 255:                                                  # an outlier index beyond the list
                assert ((lo == 255) & (hi >= no) & (hi != 255)).any() and ((hi == 255) & (lo >= no) & (lo != 255)).any()
            if nn < 255:                                                  # a normal code beyond the list, no identifier in the pair
                assert ((lo >= nn) & (lo != 255) & (hi != 255)).any() and ((hi >= nn) & (hi != 255) & (lo != 255)).any()
        # 255 is the low byte of its pair in one row's run of all bytes and the high byte in another's
        pos = [int(np.flatnonzero(c[n, :256] == 255)[0]) % 2 for n in range(c.shape[0])]
        assert set(pos) == {0, 1}


@pytest.mark.parametrize("dtype_name", lc.DTYPES)
@pytest.mark.parametrize("name", lc.ONE_HOT_BOOKS)
def test_tiny_scales_make_subnormal_weights(oracle, name, dtype_name):
    lim = lc.SUBNORMAL_BELOW[dtype_name]
    c = lc.one_hot_codes(name, lc.ONE_HOT_K[0])
    n_tiny = 0
    for per_row, a in lc.one_hot_scales(dtype_name):
        v = np.abs(lc.value(lc.image_ref(oracle, c, a, per_row, name, dtype_name), dtype_name))
        assert np.isfinite(v).all()
        if a.min() <= lc.tiny_scale(dtype_name):
            rows = np.flatnonzero(a <= np.float32(lc.tiny_scale(dtype_name))) if per_row else np.arange(c.shape[0])
            assert ((v[rows] > 0) & (v[rows] < lim)).any(), (name, dtype_name, per_row)
            n_tiny += 1
        else:
            assert (v >= lim).any()
    assert n_tiny == 2


@pytest.mark.parametrize("name", lc.GENERAL_BOOKS)
def test_general_data_codes_hold_the_pair_identifier(oracle, name):
    bk = bc.book(name)
    _, g, gmax, nn, ovp = bk
    for dtype_name in lc.DTYPES:
        for K in lc.GENERAL_K:
            d = lc.gauss_weights(name, dtype_name, K)
            assert d["w"].shape == (lc.GENERAL_N, K) and d["alpha"].shape == (lc.GENERAL_N,) and (d["alpha"] > 0).all()
            _, wf = ec.as_dtype(oracle, d["w"], dtype_name)
            codes = bc.oracle_codes(oracle, wf, d["alpha"], bk)
            assert codes.min() >= 0 and codes.max() <= 255
            if ovp:
                assert (codes == bc.IDENT).any(), (name, dtype_name, K)
                assert (codes == bc.IDENT).mean() < 0.05
            else:
                assert codes.max() < g.size
