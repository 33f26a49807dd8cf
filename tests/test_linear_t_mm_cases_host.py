"""The inputs of antq_linear4_t_mm's GPU tests (tests/linear_t_mm_cases.py) held to their premises on the CPU: the codes hold
all 256 byte values where the tests say so, pair identifiers are present under the pair rule, a subnormal weight is present in
the tiny-scale cases, the order-free exact sums are exact -- and the builder's own assertion fires when they are not."""
import numpy as np
import pytest

import linear_t_cases as lt
import linear_t_mm_cases as mc


def test_grids_sit_at_the_switch_points():
    # steps of 32 k dealt to eight wavefronts
    steps = {K: -(-K // 32) for K in mc.GRID_K}
    assert min(steps.values()) == 1 and any(K % 32 for K in mc.GRID_K) and any(K % 32 == 0 for K in mc.GRID_K)
    assert {8, 24} <= set(mc.GRID_K)                                     # a partial step, seven wavefronts without any
    assert steps[32] == 1 and steps[40] == 2 and steps[256] == 8 and steps[264] == 9
    assert any(s > 8 and s % 8 for s in steps.values())                   # several passes, unequal step counts
    # both sides of a 32-, 64- and 128-column tile, and a partial column group of each
    for tile in (32, 64, 128):
        assert {tile, tile + 8} <= set(mc.GRID_N) and any(N < tile for N in mc.GRID_N)
    assert all(N % 8 == 0 for N in mc.GRID_N) and all(K % 8 == 0 for K in mc.GRID_K)
    # both sides of every tile of 16 rows of x, and the most rows
    for edge in (16, 32, 48):
        assert {edge, edge + 1} <= set(mc.GRID_M)
    assert {1, 9, 15, mc.MAX_M} <= set(mc.GRID_M) and max(mc.GRID_M) == mc.MAX_M == 64
    assert mc.STAGED_K == 8192 and mc.ONE_HOT_K % 32 and mc.ONE_HOT_K > 256


@pytest.mark.parametrize("dtype_name", mc.DTYPES)
def test_one_hot_case(dtype_name):
    K, N = mc.ONE_HOT_K, mc.ONE_HOT_N
    codes = mc.all_byte_codes(K, N)
    assert codes.size == K * N // 2 and np.unique(codes).size == 256
    assert mc.has_pair_identifier(codes)
    # the identity in calls of 64 rows covers every k once
    seen = np.zeros(K, int)
    for k0 in range(0, K, mc.MAX_M):
        x = mc.one_hot_x(K, k0)
        assert x.shape == (mc.MAX_M, K) and set(np.unique(x)) <= {0.0, 1.0}
        seen += x.sum(0).astype(int)
    assert (seen == 1).all()
    lim = mc.subnormal_limit(dtype_name)
    variants = mc.one_hot_scales(dtype_name, K)
    assert [v[0] for v in variants] == [True, False, False] and any(v[2] for v in variants) and not all(v[2] for v in variants)
    for book in lt.books():
        for per_row, alpha, has_tiny in variants:
            assert alpha.size == (K if per_row else 1) and alpha.dtype == np.float32
            mag = np.abs(lt.value(lt.image_bits(codes, alpha, K, N, per_row, book, dtype_name), dtype_name))
            assert np.isfinite(mag).all()
            assert bool(((mag > 0) & (mag < lim)).any()) == has_tiny, (book[0], per_row, float(alpha.min()))


@pytest.mark.parametrize("dtype_name", mc.DTYPES)
def test_exact_cases_are_exact_in_any_order(dtype_name):
    rng = np.random.default_rng(5)
    for bname in mc.EXACT_BOOKS:
        book = lt.book(bname)
        for K, per_row in ((8, True), (264, False), (1600, True)):
            codes, alpha, x, bias, y, density = mc.exact_case(rng, K, book, dtype_name, per_row, 136)
            assert x.shape == (mc.MAX_M, K) and y.shape == (mc.MAX_M, 136) and np.abs(x).max() <= 3 and (x[:, 0] != 0).all()
            if book[4]:
                assert mc.has_pair_identifier(codes)
            W = lt.value(lt.image_bits(codes, alpha, K, 136, per_row, book, dtype_name), dtype_name)
            # x and the bias are the type's own values, and so is the exact result's rounding input (an fp32 number)
            assert np.array_equal(lt.value(lt.round_bits(x.astype(np.float32), dtype_name), dtype_name), x)
            assert np.array_equal(lt.value(lt.round_bits(bias.astype(np.float32), dtype_name), dtype_name), bias)
            total = y + bias[None, :]
            assert np.array_equal(total.astype(np.float32).astype(np.float64), total)
            # two very different orders of the sum, in fp32, give the float64 result
            xf, Wf = x.astype(np.float32), W.astype(np.float32)
            fwd = np.zeros((mc.MAX_M, 136), np.float32)
            for k in range(K):
                fwd = fwd + xf[:, k:k + 1] * Wf[k:k + 1, :]
            order = np.argsort(-np.abs(W).max(1), kind="stable")
            big_first = np.zeros((mc.MAX_M, 136), np.float32)
            for k in order:
                big_first = big_first + xf[:, k:k + 1] * Wf[k:k + 1, :]
            assert np.array_equal(fwd.astype(np.float64), y) and np.array_equal(big_first.astype(np.float64), y)
            # a prefix of the rows and of the columns is a case of its own
            assert np.array_equal(x[:9] @ W[:, :40], y[:9, :40])


def test_the_exactness_assertion_fires():
    rng = np.random.default_rng(7)
    book = lt.book("olive_int")
    codes, alpha, x, bias, y, density = mc.exact_case(rng, 264, book, "bfloat16", True, 72)
    W = lt.value(lt.image_bits(codes, alpha, 264, 72, True, book, "bfloat16"), "bfloat16")
    unit = 2.0 ** min(int(lt.lowest_bit_exponent(W).min()), 0)
    mc.check_exact(x, W, bias, unit)
    with pytest.raises(AssertionError, match="2\\^24"):
        mc.check_exact(x * 2.0 ** 24, W, bias, unit)                      # a deliberately too-large x
    with pytest.raises(AssertionError):
        mc.check_exact(x + 0.5, W, bias, unit)                            # x no whole number
    with pytest.raises(AssertionError):
        mc.check_exact(x, W, bias, unit * 2 ** 20)                        # a unit the weights are no multiples of


@pytest.mark.parametrize("dtype_name", mc.DTYPES)
def test_gauss_cases(dtype_name):
    for bname in ("flint_b4_s", "olive_flint"):
        a = mc.gauss_case(dtype_name, 264, 136, bname)
        b = mc.gauss_case(dtype_name, 264, 136, bname)
        for k in ("codes", "alpha", "W", "x", "bias", "y64", "S"):
            assert np.array_equal(a[k], b[k]), k                         # deterministic
        assert a["codes"].shape == (264, 68) and a["x"].shape == (mc.MAX_M, 264) and a["y64"].shape == (mc.MAX_M, 136)
        assert (a["alpha"] > 0).all() and np.isfinite(a["y64"]).all() and (a["S"] >= np.abs(a["y64"]) - 1e-9).all()
        if a["book"][4]:                                                  # planted outliers: beyond every normal value
            assert mc.has_pair_identifier(a["codes"])
            W = np.abs(lt.value(a["W"], dtype_name))
            normal_max = np.abs(a["book"][1][:a["book"][3]]).max() * (a["alpha"] / np.float32(a["book"][2]))
            assert (W > normal_max[:, None] * 1.01).any()
        # the narrower and the shifted layer hold the same columns
        d, s = lt.columns(a, 8), mc.shifted(a, 8)
        assert np.array_equal(d["W"], a["W"][:, :8]) and d["codes"].shape == (264, 4)
        assert np.array_equal(s["W"], a["W"][:, 8:]) and s["N"] == 128 and np.array_equal(s["bias"], a["bias"][8:])
        assert np.array_equal(lt.image_bits(s["codes"], a["alpha"], 264, 128, True, a["book"], dtype_name), s["W"])
