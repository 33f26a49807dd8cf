"""The inputs of tests/test_gpu_linear8_gemm.py (tests/linear8_gemm_cases.py) held to their premises with numpy and the CPU
oracle alone: the one-hot code sets hold every byte value their book allows, the exact-sum cases are exact in any order for every
case the GPU test runs (and x stays dense enough to mean something), each K is on the code path claimed for it, M, N and K lie
on both sides of every tile, step and path boundary, and three restated mistakes each change compared elements."""
import numpy as np
import pytest

import byte_codes_cases as bc
import linear8_cases as lc
import linear8_gemm_cases as gc


@pytest.mark.parametrize("name", gc.ONE_HOT_BOOKS)
def test_one_hot_code_sets_hold_every_byte_and_every_pair_form(name):
    _, g, gmax, nn, ovp = bc.book(name)
    no = g.size - nn
    assert [(gc.vec_path(k), gc.has_tail(k), k % 32) for k in gc.ONE_HOT_K] == [(False, True, 8), (True, True, 16), (True, False, 0)]
    for K in gc.ONE_HOT_K:
        c = lc.one_hot_codes(name, K, N=gc.ONE_HOT_N).astype(np.int64)
        assert c.shape == (37, K) and gc.ONE_HOT_N < gc.BN and K > 2 * gc.CALL and K % gc.CALL
        for n in range(c.shape[0]):
            # every byte value -- those of the book, those beyond it and the identifier -- in every row
            assert np.unique(c[n]).size == 256, (name, K, n)
            if not ovp:
                assert (c[n] >= g.size).any() or g.size == 256
                continue
            lo, hi = c[n].reshape(-1, 2)[:, 0], c[n].reshape(-1, 2)[:, 1]
            assert ((lo == 255) & (hi != 255)).any() and ((hi == 255) & (lo != 255)).any() and ((lo == 255) & (hi == 255)).any()
            for idx in (0, no - 1):
                assert ((lo == 255) & (hi == idx)).any() and ((hi == 255) & (lo == idx)).any(), (name, K, n, idx)
        # every byte value sits at every position of a lane's 8 bytes (k % 8), in both 16-byte loads of a lane (k % 32) and in
        # every MFMA of a step on both paths (k % 128 covers k % 32 and (k // 32) % 4) in some row
        for mod in (8, 16, 32):
            for v in (0, 1, 254, 255):
                assert {int(np.flatnonzero(c[n, :256] == v)[0]) % mod for n in range(c.shape[0])} == set(range(mod)), (name, K, v, mod)


@pytest.mark.parametrize("name,dtype_name", gc.EXACT_CASES)
def test_exact_sum_cases_are_exact_in_any_order(oracle, name, dtype_name):
    seen_n, seen_per_row, lowest, set_name = set(), set(), (2.0, (0, 0)), name
    for K in gc.EXACT_K:
        name = gc.exact_book(set_name, K)
        assert name in lc.EXACT_BOOKS and (name == set_name or (set_name, K) == ("int_b8_s", 4096))
        _, g, gmax, nn, ovp = bc.book(name)
        per_row, cases = gc.exact_cases_of(oracle, name, K, dtype_name)
        seen_per_row.add(per_row)
        for ns, c in cases:
            N = max(ns)
            assert c["codes"].shape == (N, K) and c["codes"].dtype == np.uint8 and c["x"].shape == (gc.ROWS, K) and gc.ROWS == 515
            assert c["alpha"].size == (N if per_row else 1)
            s = (c["alpha"] / np.float32(gmax)).astype(np.float32)
            assert np.array_equal(np.exp2(np.round(np.log2(s))), s)
            assert np.abs(c["x"]).max() <= 3 and np.abs(c["bias"]).max() <= 8
            # x means something: every row has a non-zero and at least 1 / 64 of all of x is non-zero
            filled = float((c["x"] != 0).mean())
            assert (c["x"] != 0).any(1).all() and c["density"] >= gc.MIN_DENSITY and filled >= gc.MIN_DENSITY, (name, dtype_name, K, N, c["density"], filled)
            lowest = min(lowest, (c["density"], (K, N)))
            # the weights are the decoder's rule in this type; the premise in float64, in matmul form
            W = lc.value(lc.image_ref(oracle, c["codes"], c["alpha"], per_row, name, dtype_name), dtype_name)
            assert np.array_equal(W, c["W"])
            gc.assert_exact_premise(c["x"], W, c["bias"])
            unit = lc.unit_of(W)
            mass = np.abs(c["x"]) @ np.abs(W / unit).T + np.abs(c["bias"])[None, :] / unit
            assert mass.max() < 2.0 ** 24 and np.array_equal(W / unit, np.round(W / unit))
            assert np.array_equal(c["y"], (c["x"] @ (W / unit).T) * unit)
            if K <= 24:                   # (small K: the same sums term by term, as linear8_cases forms them)
                lc.assert_exact_premise(c["x"][:64], W, c["bias"])
                assert np.array_equal(c["y"][:64], (c["x"][:64, None, :] * W[None, :, :]).sum(-1))
            seen_n.update(ns)
            if K == gc.EXACT_K[0]:        # the same arguments give the same arrays (the GPU test builds them again)
                again = gc.exact_cases_of(oracle, name, K, dtype_name)[1][0][1]
                assert np.array_equal(again["codes"], cases[0][1]["codes"]) and np.array_equal(again["x"], cases[0][1]["x"])
    assert seen_n == set(gc.EXACT_N) and seen_per_row == {True, False}
    print("%s %s: lowest density of x %.4g at (K, N) = %s" % (set_name, dtype_name, lowest[0], lowest[1]))


def test_exact_cases_are_the_16_bit_ones_of_the_row_kernel():
    assert gc.EXACT_CASES == tuple(c for c in lc.EXACT_CASES if c[1] != "float32") and {c[0] for c in gc.EXACT_CASES} == set(lc.EXACT_BOOKS)


def test_k_m_and_n_lie_on_both_sides_of_every_boundary():
    ks, ns, ms = set(gc.EXACT_K), set(gc.EXACT_N), set(gc.EXACT_M)
    assert ks >= {8, 16, 24, 40, 120, 128, 136, 144, 248, 256, 264, 272, 504, 512, 520, 528, 2056, 4096}
    assert all(k % 8 == 0 and k > 0 for k in ks)
    # the staged step: one short, exact, one group and one 16-byte unit over -- for one, two and four steps
    for steps in (1, 2, 4):
        assert {gc.BK * steps - 8, gc.BK * steps, gc.BK * steps + 8, gc.BK * steps + 16} <= ks
    # each K is on the path claimed for it: K % 16 != 0 is the 8-byte path; K % 16 == 0 runs the 16-byte path with aligned
    # codes and the 8-byte path 8 bytes off a 16-byte boundary
    for k in ks:
        offs = gc.exact_offsets(k)
        assert {gc.vec_path(k, o) for o in offs} == ({True, False} if k % 16 == 0 else {False}), k
        assert all(o % 8 == 0 for o in offs)
    # the 16-byte path with the second load of the last lane group past the row's end (K % 32 == 16), with a whole lane group
    # last (K % 32 == 0), with a tail and without; the 8-byte path with a tail and (offset) without
    vec = {k for k in ks if k % 16 == 0}
    assert {k for k in vec if k % 32 == 16} >= {16, 144, 272, 528} and {k for k in vec if k % 32 == 0 and gc.has_tail(k)} >= {160}
    assert {k for k in vec if not gc.has_tail(k)} >= {128, 256, 512, 4096} and {k for k in ks if k % 16 and gc.has_tail(k)} >= {8, 24, 120, 136, 520}
    # a tail that ends inside every MFMA of the step on the 8-byte path (k = 128 c + 32 j + 8 kg: j = (K % 128) // 32)
    assert {(k % gc.BK) // 32 for k in ks if gc.has_tail(k)} == {0, 1, 3} or {(k % gc.BK) // 32 for k in ks if gc.has_tail(k)} == {0, 1, 2, 3}
    # output rows around the 16-row MFMA tile and the workgroup's 64; rows of x around the wavefront's 64 and both tiles
    assert {15, 16, 17, gc.BN - 1, gc.BN, gc.BN + 1, 2 * gc.BN + 1, 1} <= ns
    assert {1, 9, 64, 65} <= ms
    for bm in gc.BMS:
        assert {bm - 1, bm, bm + 1, 2 * bm + 3} <= ms
    assert gc.BMS == (128, 256) and gc.TILES == (2, 4) and [64 * w for w in gc.TILES] == list(gc.BMS)
    assert max(gc.GENERAL_M) > gc.BMS[1] and min(gc.GENERAL_M) > 64


def test_staggered_launches_cover_every_value():
    for K in gc.EXACT_K:
        runs = gc.exact_runs(K)
        assert {r[0] for r in runs} == set(range(len(gc.EXACT_N))) and {r[1] for r in runs} == set(range(len(gc.EXACT_M)))
        assert {r[2] for r in runs} == set(gc.exact_offsets(K)) and {r[3] for r in runs} == {0, 2, 4}
        assert {f for r in runs for f in r[4]} == {True, False}
        for off in gc.exact_offsets(K):                     # every offset with rows of x in one, two and more tiles
            ms = {gc.EXACT_M[r[1]] for r in runs if r[2] == off}
            assert any(m <= 128 for m in ms) and any(128 < m <= 256 for m in ms) and any(m > 256 for m in ms), (K, off)
    pairs = {(r[0], r[1], r[3]) for K in gc.EXACT_K for r in gc.exact_runs(K)}
    assert len(pairs) == len(gc.EXACT_N) * len(gc.EXACT_M) * 3


# ---------------------------------------------------------------------------------------------------------------------------
# three mistakes, restated: each changes elements the GPU test compares
# ---------------------------------------------------------------------------------------------------------------------------
def test_swapped_16_byte_loads_would_show(oracle):
    """a lane's two 16-byte loads of a step exchanged: the one-hot image and the exact sums of the 16-byte path both change"""
    name, dtype_name = "flint_b6_s", "bfloat16"
    for K in (528, 512):
        codes = lc.one_hot_codes(name, K, N=gc.ONE_HOT_N)
        a = gc.scale_rows(lc.one_hot_scales(dtype_name)[0][1], gc.ONE_HOT_N)
        W = lc.image_ref(oracle, codes, a, True, name, dtype_name)
        assert (gc.swap_16_byte_loads(W) != W).sum() > 0, K
    changed = 0
    for K in (16, 144, 256, 4096):
        assert gc.vec_path(K)
        per_row, cases = gc.exact_cases_of(oracle, name, K, dtype_name)
        c = cases[0][1]
        y2 = c["x"] @ gc.swap_16_byte_loads(c["W"]).T
        n = int((y2 != c["y"]).sum())
        assert n > 0 or K == 16, K         # (K = 16 is one load: nothing to exchange)
        changed += n
    assert changed > 0


def test_tables_built_with_the_wrong_stride_would_show(oracle):
    """mm_build's stride of 8 wavefronts in a workgroup of 2 or 4: only rows w, w + 8, ... of the tile have a table.  With
    per-row scales every other output row of every tile would read an unbuilt table: its exact sum is not the bias alone."""
    for waves in gc.TILES:
        built = gc.rows_built_with_stride(waves)
        assert built.sum() == 8 * waves and gc.rows_built_with_stride(waves, stride=waves).all()
    name, dtype_name = "olive_int_b8", "float16"
    hit = 0
    for K in gc.EXACT_K:
        per_row, cases = gc.exact_cases_of(oracle, name, K, dtype_name)
        if not per_row:
            continue
        c = cases[0][1]
        N = c["codes"].shape[0]
        unbuilt = ~gc.rows_built_with_stride(2)[np.arange(N) % gc.BN]
        assert unbuilt[2] and not unbuilt[8]
        W0 = np.where(unbuilt[:, None], 0.0, c["W"])                   # (any table but the row's own: here, all zeros)
        hit += int(((c["x"] @ W0.T) != c["y"])[:, unbuilt].sum())
    assert hit > 0


def test_a_tail_that_is_not_zeroed_would_show():
    """(the k >= K fragment multiplied with the row's repeated last unit, an Inf in it: 0 * Inf is NaN.  The exact-sum cases
    hold finite weights only, so this one shows in the special-value cases: test_linear8_gemm_specials_host.py, mistake (a),
    asserted there at every K with a tail.)  Here: every exact K with a tail has lanes past the end of the row on both paths."""
    for K in gc.EXACT_K:
        if gc.has_tail(K):
            groups = K // 8
            assert groups % 16 != 0                                     # the last step holds fewer than its 16 groups of 8
