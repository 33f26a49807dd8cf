"""The inputs of tests/test_gpu_linear8_mm.py (tests/linear8_mm_cases.py) held to their premises with numpy and the CPU oracle
alone: the exact-sum cases are exact in any order (for every case the GPU test runs), the K list holds the kernel's
boundaries, the staggered launches cover every N, M, offset, tile shape and bias form, and the one-hot code sets hold what
they claim at N = 37."""
import numpy as np
import pytest

import byte_codes_cases as bc
import linear8_cases as lc
import linear8_mm_cases as mc


@pytest.mark.parametrize("name,dtype_name", mc.MM_EXACT_CASES)
def test_exact_sum_cases_are_exact_in_any_order(oracle, name, dtype_name):
    _, g, gmax, nn, ovp = bc.book(name)
    seen_n, seen_per_row = set(), set()
    for K in mc.EXACT_K:
        per_row, cases = mc.exact_cases_of(oracle, name, K, dtype_name)
        seen_per_row.add(per_row)
        for ns, c in cases:
            N = max(ns)
            assert c["codes"].shape == (N, K) and c["codes"].dtype == np.uint8 and c["x"].shape == (mc.ROWS, K) and mc.ROWS == 64
            assert c["alpha"].size == (N if per_row else 1)
            s = (c["alpha"] / np.float32(gmax)).astype(np.float32)
            assert np.array_equal(np.exp2(np.round(np.log2(s))), s)
            assert np.abs(c["x"]).max() <= 3 and (c["x"][:, 0] != 0).all() and np.abs(c["bias"]).max() <= 8
            assert c["density"] >= 2.0 ** -12
            # the weights are the decoder's rule in this type; the premise in float64, in matmul form
            W = lc.value(lc.image_ref(oracle, c["codes"], c["alpha"], per_row, name, dtype_name), dtype_name)
            assert np.array_equal(W, c["W"])
            mc.assert_exact_premise(c["x"], W, c["bias"])
            unit = lc.unit_of(W)
            mass = np.abs(c["x"]) @ np.abs(W / unit).T + np.abs(c["bias"])[None, :] / unit
            assert mass.max() < 2.0 ** 24 and np.array_equal(W / unit, np.round(W / unit))
            assert np.array_equal(c["y"], (c["x"] @ (W / unit).T) * unit)
            # (small K: the same sums term by term, as linear8_cases forms them)
            if K <= 64:
                lc.assert_exact_premise(c["x"], W, c["bias"])
                assert np.array_equal(c["y"], (c["x"][:, None, :] * W[None, :, :]).sum(-1))
            seen_n.update(ns)
            if K == mc.EXACT_K[0]:        # the same arguments give the same arrays (the GPU test builds them again)
                again = mc.exact_cases_of(oracle, name, K, dtype_name)[1][0][1]
                assert np.array_equal(again["codes"], cases[0][1]["codes"]) and np.array_equal(again["x"], cases[0][1]["x"])
    assert seen_n == set(mc.EXACT_N) and seen_per_row == {True, False}


def test_exact_cases_are_the_16_bit_ones_of_the_row_kernel():
    assert mc.MM_EXACT_CASES == tuple(c for c in lc.EXACT_CASES if c[1] != "float32")
    assert ("int_b8_s", "bfloat16") in mc.MM_EXACT_CASES and ("int_b8_s", "float16") not in mc.MM_EXACT_CASES


def test_exact_k_holds_the_kernels_boundaries():
    ks = set(mc.EXACT_K)
    assert {8, 16, 24, 32, 40, 4096} <= ks and all(k % 8 == 0 and k > 0 for k in ks)
    for w in range(1, 9):
        assert {32 * w - 8, 32 * w, 32 * w + 8} <= ks and {64 * w - 16, 64 * w, 64 * w + 16} <= ks
    # the 8-byte path is reached at every K of its list: by K % 16 != 0, or by the offset of 8 bytes
    for k in mc.EXACT_K_8 + mc.EXACT_K_RING[8]:
        assert k % 16 != 0 or 8 in mc.exact_offsets(k)
    for k in mc.EXACT_K_16 + mc.EXACT_K_RING[16]:
        assert k % 16 == 0 and 0 in mc.exact_offsets(k)
    # ring refill: 8 D chunks fill the rings exactly, one more is the first refill
    for b, chunk in ((8, 32), (16, 64)):
        for D in (4, 3, 2):
            assert {chunk * (8 * D - 1), chunk * 8 * D, chunk * (8 * D + 1)} <= set(mc.EXACT_K_RING[b])
    # a ring depth goes with the tiles of x: every depth's M is in the list on both sides
    assert {1, 16} & set(mc.EXACT_M) and {17, 32} <= set(mc.EXACT_M) and {33, 48, 64} <= set(mc.EXACT_M)


def test_staggered_launches_cover_every_value():
    for K in mc.EXACT_K:
        runs = mc.exact_runs(K)
        assert {r[0] for r in runs} == set(range(len(mc.EXACT_N))) and {r[1] for r in runs} == set(range(len(mc.EXACT_M)))
        assert {r[2] for r in runs} == set(mc.exact_offsets(K)) and {r[3] for r in runs} == set(mc.TILES)
        assert {f for r in runs for f in r[4]} == {True, False}
        # every ring depth (tiles of x: M <= 16, <= 32, more) with every offset
        for off in mc.exact_offsets(K):
            ms = {mc.EXACT_M[r[1]] for r in runs if r[2] == off}
            assert any(m <= 16 for m in ms) and any(16 < m <= 32 for m in ms) and any(m > 32 for m in ms), (K, off)
    # over the K list every pair (N, M) runs with every tile shape
    pairs = {(r[0], r[1], r[3]) for K in mc.EXACT_K for r in mc.exact_runs(K)}
    assert len(pairs) == len(mc.EXACT_N) * len(mc.EXACT_M) * len(mc.TILES)


@pytest.mark.parametrize("name", mc.ONE_HOT_BOOKS)
def test_one_hot_code_sets_hold_every_byte_and_every_pair_form(name):
    _, g, gmax, nn, ovp = bc.book(name)
    no = g.size - nn
    assert [k % 16 == 0 for k in mc.ONE_HOT_K] == [False, True]
    for K in mc.ONE_HOT_K:
        c = lc.one_hot_codes(name, K, N=mc.ONE_HOT_N).astype(np.int64)
        assert c.shape == (37, K)
        for n in range(c.shape[0]):
            assert np.unique(c[n]).size == 256, (name, K, n)
            if not ovp:
                assert (c[n] >= g.size).any() or g.size == 256
                continue
            lo, hi = c[n].reshape(-1, 2)[:, 0], c[n].reshape(-1, 2)[:, 1]
            assert ((lo == 255) & (hi != 255)).any() and ((hi == 255) & (lo != 255)).any() and ((lo == 255) & (hi == 255)).any()
            for idx in (0, no - 1):
                assert ((lo == 255) & (hi == idx)).any() and ((hi == 255) & (lo == idx)).any(), (name, K, n, idx)
        # every byte value sits at every position of a lane's 8 bytes (k % 8) and in both steps of a 16-byte chunk (k % 16) in
        # some row: a wrong byte, word, step or partner shows at every code
        for mod in (8, 16):
            for v in (0, 1, 254, 255):
                assert {int(np.flatnonzero(c[n, :256] == v)[0]) % mod for n in range(c.shape[0])} == set(range(mod)), (name, K, v, mod)


def test_one_hot_scales_cycle_over_the_rows():
    for dtype_name in mc.DTYPES:
        for per_row, a in lc.one_hot_scales(dtype_name):
            if per_row:
                s = mc.scale_rows(a, mc.ONE_HOT_N)
                assert s.shape == (37,) and set(s.tolist()) == set(a.tolist()) and (s[:a.size] == a).all()
